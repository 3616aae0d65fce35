"""
CPU tests of the displacement gradient's argument checks: the Python entry points refuse bad shapes and
dtypes before anything touches a device, and the C entry points answer fake descriptors with the status
codes of edhip_deform -- no GPU needed, nothing is launched.
"""
import os

import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _lib


def _disp(shape=(2, 3, 3)):
    return np.zeros(shape)


def test_wrong_dy_shape_raises_before_launch():
    X = np.zeros((10, 12), np.float32)
    with pytest.raises(ValueError, match="dY does not match"):
        ed.deform_grid_displacement_gradient(X, np.zeros((10, 11), np.float32), _disp())
    with pytest.raises(ValueError, match="dY does not match"):
        ed.deform_grid_displacement_gradient(X, np.zeros((4, 5), np.float32), _disp(), crop=(slice(0, 4), slice(0, 6)))
    with pytest.raises(ValueError, match="dY does not match"):
        ed.deform_grid_displacement_gradient([X, X], [np.zeros((10, 12), np.float32)], _disp())


def test_wrong_displacement_shape_has_deform_grid_messages():
    X = np.zeros((10, 12), np.float32)
    with pytest.raises(AssertionError, match="Number of dimensions of displacement does not match input"):
        ed.deform_grid_displacement_gradient(X, X, np.zeros((2, 3)))
    with pytest.raises(AssertionError, match="First dimension of displacement should match"):
        ed.deform_grid_displacement_gradient(X, X, np.zeros((3, 3, 3)))
    with pytest.raises(RuntimeError, match="boundary mode not supported"):
        ed.deform_grid_displacement_gradient(X, X, _disp(), mode="bogus")


@pytest.mark.parametrize("dtype", ["int32", "uint8", "bool", "float16", "int16"])
def test_integer_and_16bit_volumes_refused(dtype):
    X = np.zeros((10, 12), dtype)
    dY = np.zeros((10, 12), np.float32)
    with pytest.raises(RuntimeError, match="data type not supported"):
        ed.deform_grid_displacement_gradient(X, dY, _disp())
    with pytest.raises(RuntimeError, match="data type not supported"):
        ed.deform_grid_displacement_gradient(dY, X, _disp())
    with pytest.raises(RuntimeError, match="data type not supported"):
        ed.deform_grid_displacement_gradient_batch(X[None], dY[None], _disp()[None])


def test_batch_shape_checks():
    X = np.zeros((2, 10, 12), np.float32)
    with pytest.raises(ValueError, match="dY does not match"):
        ed.deform_grid_displacement_gradient_batch(X, np.zeros((2, 10, 11), np.float32), np.zeros((2, 2, 3, 3)))
    with pytest.raises(AssertionError, match="One displacement grid per sample"):
        ed.deform_grid_displacement_gradient_batch(X, X, np.zeros((3, 2, 3, 3)))


# ---- the C entry points on fake descriptors (no device memory is touched) ---------------------------------

pytestmark_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                                    reason="libedhip.so not built (run __graft_entry__.build())")


def _desc(shape, dtype="float32", ptr=0x1000):
    a = np.empty(shape, dtype=dtype)
    return _lib.describe(ptr, a.dtype.name, a.shape, a.strides)


def _status(ins, disp, outs, axis, ddisp=None, orders=None, modes=None, flags=0):
    import ctypes
    n = len(ins)
    a = _lib.DeformArgs(n, axis, orders or [3] * n, modes or [4] * n, [0.0] * n, None, None)
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)
    ddisp = ddisp if ddisp is not None else _desc(tuple(disp.shape[:disp.ndim]), "float64")
    st = L.edhip_deform_displacement_gradient(n, (_lib.EdhipArray * n)(*ins), ctypes.byref(disp), a.off,
                                              (_lib.EdhipArray * n)(*outs), a.naxis, a.axis, a.orders, a.modes,
                                              a.cvals, a.aff, ctypes.byref(ddisp), flags, None, buf, 256)
    return st, buf.value.decode()


@pytestmark_lib
def test_c_entry_validation_codes():
    x = _desc((8, 9))
    d2 = _desc((2, 3, 3), "float64")
    dd = _desc((2, 3, 3), "float64")
    assert _status([x], d2, [_desc((8, 9, 1))], [(0, 1)], dd)[0] == 1          # ndim mismatch
    assert _status([x], d2, [x], [(0, 2)], dd)[0] == 1                         # bad axis
    assert _status([x], _desc((3, 3, 3), "float64"), [x], [(0, 1)], dd)[0] == 1   # displacement shape
    assert _status([x], d2, [x], [(0, 1)], _desc((2, 3, 4), "float64"))[0] == 1   # ddisplacement shape
    assert _status([x], d2, [x], [(0, 1)], dd, orders=[6])[0] == 1
    assert _status([x], d2, [x], [(0, 1)], dd, modes=[9])[0] == 1
    for dt in ("int32", "uint8", "int16", "bool", "float16"):
        st, msg = _status([_desc((8, 9), dt)], d2, [x], [(0, 1)], dd)
        assert st == 2 and msg == "data type not supported", dt
        st, msg = _status([x], d2, [_desc((8, 9), dt)], [(0, 1)], dd)
        assert st == 2, dt
    # raw grids above 4096 points: outside this build's limits
    assert _status([_desc((80, 90))], _desc((2, 50, 50), "float64"), [_desc((80, 90))], [(0, 1)],
                   _desc((2, 50, 50), "float64"), flags=_lib.FLAG_RAW_DISPLACEMENT)[0] == 5
    # too dense along the last axis for the row kernel's band
    assert _status([_desc((80, 900))], _desc((2, 3, 200), "float64"), [_desc((80, 900))], [(0, 1)],
                   _desc((2, 3, 200), "float64"))[0] == 5


@pytestmark_lib
def test_c_batch_entry_validation_codes():
    import ctypes
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)
    x, d, dd = _desc((8, 9)), _desc((2, 3, 3), "float64"), _desc((2, 3, 3), "float64")
    ax = (ctypes.c_int32 * 2)(0, 1)
    assert L.edhip_deform_displacement_gradient_batch_strided(
        -1, ctypes.byref(x), 0, ctypes.byref(d), 0, None, ctypes.byref(x), 0, 2, ax, 3, 3, 0.0, None,
        ctypes.byref(dd), 0, 0, None, buf, 256) == 1
    assert L.edhip_deform_displacement_gradient_batch_strided(
        0, None, 0, None, 0, None, None, 0, 2, ax, 3, 3, 0.0, None, None, 0, 0, None, buf, 256) == 0
    xi = _desc((8, 9), "int32")
    for flags in (0, _lib.FLAG_RAW_DISPLACEMENT):
        assert L.edhip_deform_displacement_gradient_batch_strided(
            2, ctypes.byref(xi), 288, ctypes.byref(d), 144, None, ctypes.byref(x), 288, 2, ax, 3, 3, 0.0, None,
            ctypes.byref(dd), 144, flags, None, buf, 256) == 2
