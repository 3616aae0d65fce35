"""
CPU tests of the host layer of deform_grid_inverse / deform_grid_inverse_batch: every argument error is raised before
the device or the library is touched -- `_lib.load` is replaced by a function that fails, and no GPU is visible here
anyway -- and edhip_deform_inverse answers its shape / dtype / flag checks with the documented status codes on
descriptors of memory that does not exist.
"""
import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _lib

CALLS = [ed.deform_grid_inverse, ed.deform_grid_inverse_batch]


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def _raises(exc, fn, *args, **kw):
    with pytest.raises(exc) as info:
        fn(*args, **kw)
    assert "the library was loaded" not in str(info.value) and "needs a ROCm GPU" not in str(info.value)
    return str(info.value)


I2 = (13, 17)
CROP2 = (slice(2, 11), slice(3, 15))
Y2 = np.zeros((9, 12))                 # the crop's shape
D2 = np.zeros((2, 3, 3))


def _args(fn, Y, D):
    """the single call's arguments, or the same with a leading batch axis of 2"""
    if fn is ed.deform_grid_inverse:
        return Y, D
    return np.stack([Y, Y]), np.stack([D, D])


def test_the_names_are_exported():
    import elasticdeform_amd.torch as et
    for name in ("deform_grid_inverse", "deform_grid_inverse_batch"):
        assert callable(getattr(ed, name))
        assert getattr(et, name) is getattr(ed, name)
    assert "edhip_deform_inverse" in _lib.EXPORTS


@pytest.mark.parametrize("fn", CALLS)
def test_x_shape_is_required_and_has_one_extent_per_dimension(fn):
    Y, D = _args(fn, Y2, D2)
    assert "X_shape is required" in _raises(ValueError, fn, Y, D, None, crop=CROP2)
    assert "one extent per dimension" in _raises(ValueError, fn, Y, D, (13, 17, 4), crop=CROP2)
    assert "one extent per dimension" in _raises(ValueError, fn, Y, D, (13,), crop=CROP2)


@pytest.mark.parametrize("fn", CALLS)
def test_y_must_have_the_shape_the_forward_call_returns(fn):
    Y, D = _args(fn, Y2, D2)
    assert "Expected shape of Y" in _raises(ValueError, fn, Y, D, I2)                                # no crop given
    assert "Expected shape of Y" in _raises(ValueError, fn, Y, D, I2, crop=(slice(2, 11), slice(3, 14)))
    Y, D = _args(fn, np.zeros((4, 9, 12)), D2)
    assert "Expected shape of Y" in _raises(ValueError, fn, Y, D, (5, 13, 17), crop=CROP2, axis=(1, 2))


@pytest.mark.parametrize("fn", CALLS)
def test_crop_outside_x_shape(fn):
    Y, D = _args(fn, Y2, D2)
    _raises(AssertionError, fn, Y, D, (10, 17), crop=CROP2)                  # slice(2, 11) of an axis of 10
    _raises(AssertionError, fn, Y, D, I2, crop=(slice(2, 11),))              # one slice for two axes


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("kw, match", [(dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"),
                                       (dict(max_iter=-3), "max_iter"), (dict(tol=0.0), "tol"),
                                       (dict(tol=-1e-9), "tol"), (dict(tol=float("nan")), "tol")])
def test_iteration_controls_are_checked(fn, kw, match):
    Y, D = _args(fn, Y2, D2)
    assert match in _raises(ValueError, fn, Y, D, I2, crop=CROP2, **kw)


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("dtype", [np.float16, np.complex64])
def test_unsupported_dtypes_are_refused(fn, dtype):
    Y, D = _args(fn, Y2.astype(dtype), D2)
    assert "data type not supported" in _raises(RuntimeError, fn, Y, D, I2, crop=CROP2)


def test_float16_stays_refused_with_reduced_precision():
    """16-bit floats are out of scope for this call, whatever deform_grid's opt-in says"""
    ed.set_reduced_precision(True)
    try:
        assert "data type not supported" in _raises(RuntimeError, ed.deform_grid_inverse, Y2.astype(np.float16), D2, I2,
                                                    crop=CROP2)
    finally:
        ed.set_reduced_precision(False)


def test_list_inputs_with_mismatched_per_input_lists():
    Ys = [Y2, np.zeros((9, 12, 3))]
    shapes = [I2, I2 + (3,)]
    axis = [(0, 1), (0, 1)]
    assert "order" in _raises(AssertionError, ed.deform_grid_inverse, Ys, D2, shapes, crop=CROP2, axis=axis,
                              order=[3, 1, 0])
    assert "mode" in _raises(AssertionError, ed.deform_grid_inverse, Ys, D2, shapes, crop=CROP2, axis=axis,
                             mode=["mirror"])
    assert "cval" in _raises(AssertionError, ed.deform_grid_inverse, Ys, D2, shapes, crop=CROP2, axis=axis,
                             cval=[0.0, 1.0, 2.0])
    assert "axis" in _raises(AssertionError, ed.deform_grid_inverse, Ys, D2, shapes, crop=CROP2, axis=[(0, 1)])
    assert "X_shape" in _raises(AssertionError, ed.deform_grid_inverse, Ys, D2, [I2], crop=CROP2, axis=axis)
    # one shape for inputs of different dimensionality
    assert "one extent per dimension" in _raises(ValueError, ed.deform_grid_inverse, Ys, D2, I2, crop=CROP2, axis=axis)


@pytest.mark.parametrize("kw", [
    dict(displacement=np.zeros((3, 3, 3))),                      # first dimension
    dict(displacement=np.zeros((2, 3))),                         # dimensions
    dict(displacement=[[0.0]]),                                  # not an array
    dict(affine=np.eye(4)),                                      # wrong shape
    dict(axis=(1, 0)),                                           # unsorted
    dict(mode="periodic"),                                       # unknown mode
    dict(order=6),                                               # unknown order
])
def test_plan_errors_equal_deform_grid(kw):
    """every other argument error is deform_grid's own, on an array of shape X_shape"""
    kw = dict(kw)
    D = kw.pop("displacement", D2)
    with pytest.raises(Exception) as want:
        ed.deform_grid(np.zeros(I2), D, crop=CROP2, **kw)
    with pytest.raises(Exception) as got:
        ed.deform_grid_inverse(Y2, D, I2, crop=CROP2, **kw)
    assert (type(got.value), str(got.value)) == (type(want.value), str(want.value))
    assert "the library was loaded" not in str(got.value) and "needs a ROCm GPU" not in str(got.value)


def test_batch_shape_mismatches():
    Yb, Db = np.stack([Y2] * 3), np.stack([D2] * 3)
    assert "One displacement grid per sample" in _raises(AssertionError, ed.deform_grid_inverse_batch, Yb[:2], Db, I2,
                                                         crop=CROP2)
    assert "leading batch axis" in _raises(Exception, ed.deform_grid_inverse_batch, np.zeros(8), Db, (8,))
    assert "shared by the batch" in _raises(AssertionError, ed.deform_grid_inverse_batch, Yb, Db, I2, crop=CROP2,
                                            order=[3, 3, 3])
    assert "ONE sample" in _raises(ValueError, ed.deform_grid_inverse_batch, Yb, Db, [I2, I2, I2], crop=CROP2)


def test_more_than_three_deformed_axes():
    Y = np.zeros((3, 3, 3, 3), dtype=np.int32)
    assert "1 to 3 deformed axes" in _raises(RuntimeError, ed.deform_grid_inverse, Y, np.zeros((4, 2, 2, 2, 2)),
                                             (3, 3, 3, 3))


def test_short_axes_are_decided_on_the_host():
    """a deformed axis of X of length 1: cval everywhere, nothing valid -- no device, no library; a deformed axis of Y
    of length 1 (a one-voxel crop) is refused"""
    Y = np.full((1, 9), 7, dtype=np.int16)
    Z = ed.deform_grid_inverse(Y, D2, (1, 9), cval=-3)
    assert Z.shape == (1, 9) and Z.dtype == np.int16 and (Z == -3).all()
    Z, valid = ed.deform_grid_inverse(Y, D2, (1, 9), cval=-3, return_valid=True)
    assert (Z == -3).all() and valid.shape == (1, 9) and valid.dtype == np.uint8 and not valid.any()
    res = ed.deform_grid_inverse([Y[:, 2:6], np.zeros((1, 4, 2), dtype=np.float32)], D2, [(1, 9), (1, 9, 2)],
                                 cval=[2, 0.5], crop=(slice(0, 1), slice(2, 6)), axis=[(0, 1), (0, 1)],
                                 return_valid=True)
    assert isinstance(res, list) and len(res) == 2
    assert res[0][0].shape == (1, 9) and (res[0][0] == 2).all()
    assert res[1][0].shape == (1, 9, 2) and res[1][0].dtype == np.float32 and (res[1][0] == 0.5).all()
    assert res[1][1].shape == (1, 9) and not res[1][1].any()
    Zb, vb = ed.deform_grid_inverse_batch(np.stack([Y, Y]), np.stack([D2, D2]), (1, 9), cval=1, return_valid=True)
    assert Zb.shape == (2, 1, 9) and (Zb == 1).all() and vb.shape == (2, 1, 9) and not vb.any()
    assert "at least 2 elements" in _raises(ValueError, ed.deform_grid_inverse, np.zeros((1, 12)), D2, I2,
                                            crop=(slice(4, 5), slice(3, 15)))


def test_c_abi_checks_answer_before_any_launch(monkeypatch):
    """edhip_deform_inverse: shape, dtype and flag checks with the existing status codes, on descriptors of memory
    that does not exist -- nothing is launched (no GPU here)."""
    import ctypes
    import os
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libedhip.so not built (run __graft_entry__.build())")
    monkeypatch.undo()
    INVALID, DTYPE, UNSUPPORTED = 1, 2, _lib.ERR_UNSUPPORTED

    def desc(shape, dtype="float64"):
        a = np.empty(shape, dtype=dtype)
        return _lib.describe(0x1000, a.dtype.name, a.shape, a.strides)

    def status(inp=desc((9, 12)), disp=desc((2, 3, 3)), in_len=(13, 17), off=(2, 3), out=desc((13, 17)), valid=None,
               axis=(0, 1), order=3, mode=0, cval=0.0, K=None, M=None, max_iter=32, tol=1e-9, flags=0, nb=1):
        """the raw status code and the message"""
        L = _lib.load()
        ax = (ctypes.c_int32 * len(axis))(*axis)
        il = (ctypes.c_int64 * len(in_len))(*in_len)
        of = (ctypes.c_int64 * len(off))(*off) if off is not None else None
        Kp = (ctypes.c_double * len(K))(*K) if K is not None else None
        Mp = (ctypes.c_double * len(M))(*M) if M is not None else None
        buf = ctypes.create_string_buffer(256)
        st = L.edhip_deform_inverse(nb, ctypes.byref(inp), 0, ctypes.byref(disp), 0, il, of, ctypes.byref(out), 0,
                                    ctypes.byref(valid) if valid is not None else None, 0, len(axis), ax, order, mode,
                                    cval, Kp, Mp, max_iter, tol, flags, None, buf, 256)
        return st, buf.value.decode()

    def check(code, match, **kw):
        st, msg = status(**kw)
        assert st == code and match in msg, (st, msg)

    check(INVALID, "prefiltered", flags=_lib.FLAG_RAW_DISPLACEMENT)
    check(DTYPE, "uint8", valid=desc((13, 17), "bool"))
    check(DTYPE, "uint8", valid=desc((13, 17), "float32"))
    check(INVALID, "deformed shape", valid=desc((9, 12), "uint8"))          # the input's extents, not the output's
    check(INVALID, "deformed shape", valid=desc((13, 17, 1), "uint8"))
    check(UNSUPPORTED, "1 to 3 deformed axes", inp=desc((3, 3, 3, 3)), out=desc((3, 3, 3, 3)),
          disp=desc((4, 2, 2, 2, 2)), axis=(0, 1, 2, 3), in_len=(3, 3, 3, 3), off=None)
    check(DTYPE, "one dtype", out=desc((13, 17), "float32"))
    check(DTYPE, "one dtype", inp=desc((9, 12), "int16"))
    check(DTYPE, "not supported", inp=desc((9, 12), "float16"), out=desc((13, 17), "float16"))
    check(INVALID, "max_iter", max_iter=0)
    check(INVALID, "tol", tol=0.0)
    check(INVALID, "tol", tol=float("nan"))
    check(INVALID, "at least 2 elements", inp=desc((9, 1)))
    check(INVALID, "at least 2 elements", in_len=(13, 1), out=desc((13, 1)))
    check(INVALID, "extents in_len", out=desc((13, 16)))
    check(INVALID, "dimensions should match", out=desc((13, 17, 1)))
    check(INVALID, "invalid axis", axis=(0, 2))
    check(INVALID, "invalid axis", axis=(1, 0))
    check(INVALID, "spline order", order=6)
    check(INVALID, "boundary mode", mode=5)
    check(INVALID, "invalid displacement shape", disp=desc((3, 3, 3)))
    check(INVALID, "non-deformed axes", inp=desc((4, 9, 12)), out=desc((5, 13, 17)), axis=(1, 2))
    check(INVALID, "forward_linear", K=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
    check(UNSUPPORTED, "too many samples", nb=65536)
    # the wrapper maps the codes to the exceptions of the other entry points
    with pytest.raises(RuntimeError, match="prefiltered"):
        _lib.deform_inverse(1, desc((9, 12)), 0, desc((2, 3, 3)), 0, (13, 17), (2, 3), desc((13, 17)), 0, None, 0,
                            (0, 1), 3, 0, 0.0, None, None, 32, 1e-9, _lib.FLAG_RAW_DISPLACEMENT, 0)
    # no samples: validated, nothing launched, EDHIP_OK
    assert status(nb=0, valid=desc((13, 17), "uint8"))[0] == 0
    assert status(nb=0, K=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), M=(1.0, 0.0, 0.0, 1.0))[0] == 0
