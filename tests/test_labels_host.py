"""
CPU tests of the host layer of deform_grid_labels / deform_grid_labels_batch: every argument error is raised before the
device or the library is touched -- `_lib.load` is replaced by a function that fails, and no GPU is visible here
anyway -- and edhip_deform_labels answers its shape / dtype / flag checks with the documented status codes on
descriptors of memory that does not exist.
"""
import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _lib

CALLS = [ed.deform_grid_labels, ed.deform_grid_labels_batch]


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


L2 = np.zeros((8, 9), dtype=np.uint8)
D2 = np.zeros((2, 3, 3))


def _args(fn, L, D):
    """the single call's arguments, or the same with a leading batch axis of 2"""
    if fn is ed.deform_grid_labels:
        return L, D
    return np.stack([L, L]), np.stack([D, D])


def test_the_names_are_exported():
    import elasticdeform_amd.torch as et
    for name in ("deform_grid_labels", "deform_grid_labels_batch"):
        assert callable(getattr(ed, name))
        assert getattr(et, name) is getattr(ed, name)
    assert "edhip_deform_labels" in _lib.EXPORTS


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.float16, np.complex64])
def test_float_inputs_are_refused(fn, dtype):
    L, D = _args(fn, L2.astype(dtype), D2)
    assert "data type not supported" in _raises(RuntimeError, fn, L, D)


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("dtype,cval", [
    (np.uint8, 2.5), (np.uint8, 300), (np.uint8, -1), (np.uint16, -1), (np.uint64, -1), (np.int8, 128),
    (np.int8, -129), (np.bool_, 2), (np.int32, float("nan")), (np.int32, float("inf")), (np.int64, 2 ** 63),
    (np.uint64, 2 ** 64), (np.int64, 2 ** 53 + 1), (np.int16, "3"),
])
def test_cval_must_be_an_integer_value_of_the_dtype(fn, dtype, cval):
    L, D = _args(fn, L2.astype(dtype), D2)
    assert "cval" in _raises(ValueError, fn, L, D, cval=cval)


def test_per_input_cvals_are_checked_against_their_own_dtype():
    Ls = [L2, L2.astype(np.int16)]
    assert "uint8" in _raises(ValueError, ed.deform_grid_labels, Ls, D2, cval=[-4, -4])
    assert "int16" in _raises(ValueError, ed.deform_grid_labels, Ls, D2, cval=[4, 40000])


@pytest.mark.parametrize("kw", [
    dict(displacement=np.zeros((3, 3, 3))),                      # first dimension
    dict(displacement=np.zeros((2, 3))),                         # dimensions
    dict(displacement=[[0.0]]),                                  # not an array
    dict(crop=(slice(0, 4),)),                                   # one slice for two axes
    dict(crop=(slice(0, 40), slice(0, 4))),                      # beyond the array
    dict(affine=np.eye(4)),                                      # wrong shape
    dict(axis=(1, 0)),                                           # unsorted
    dict(mode="periodic"),                                       # unknown mode
])
def test_plan_errors_equal_deform_grid(kw):
    """a displacement whose shape does not match the axes, and every other argument error, is deform_grid's own"""
    kw = dict(kw)
    D = kw.pop("displacement", D2)
    with pytest.raises(Exception) as want:
        ed.deform_grid(L2, D, order=1, **kw)
    with pytest.raises(Exception) as got:
        ed.deform_grid_labels(L2, D, **kw)
    assert (type(got.value), str(got.value)) == (type(want.value), str(want.value))
    assert "the library was loaded" not in str(got.value) and "needs a ROCm GPU" not in str(got.value)


def test_batch_shape_mismatches():
    Lb, Db = np.stack([L2] * 3), np.stack([D2] * 3)
    assert "One displacement grid per sample" in _raises(AssertionError, ed.deform_grid_labels_batch, Lb[:2], Db)
    assert "leading batch axis" in _raises(Exception, ed.deform_grid_labels_batch, np.zeros(8, dtype=np.uint8), Db)
    assert "displacements should be an array of shape" in _raises(Exception, ed.deform_grid_labels_batch, Lb, D2[0])
    assert "First dimension of displacement" in _raises(AssertionError, ed.deform_grid_labels_batch, Lb,
                                                        np.zeros((3, 3, 3, 3)))
    assert "shared by the batch" in _raises(AssertionError, ed.deform_grid_labels_batch, Lb, Db, cval=[1, 2, 3])


def test_more_than_three_deformed_axes():
    L = np.zeros((3, 3, 3, 3), dtype=np.int32)
    assert "1 to 3 deformed axes" in _raises(RuntimeError, ed.deform_grid_labels, L, np.zeros((4, 2, 2, 2, 2)))


def test_length_one_axis_is_decided_on_the_host():
    """a deformed axis of length 1: cval everywhere with weight 1.0 -- no device, no library"""
    L = np.full((1, 9), 7, dtype=np.int16)
    out = ed.deform_grid_labels(L, D2, cval=-3)
    assert out.shape == (1, 9) and out.dtype == np.int16 and (out == -3).all()
    out, wt = ed.deform_grid_labels(L, D2, cval=-3, return_weight=True)
    assert (out == -3).all() and wt.shape == (1, 9) and wt.dtype == np.float32 and (wt == 1.0).all()
    res = ed.deform_grid_labels([L, L.astype(np.uint64)], D2, cval=[2, 2 ** 53], crop=(slice(0, 1), slice(2, 6)),
                                return_weight=True)
    assert isinstance(res, list) and len(res) == 2
    assert res[1][0].shape == (1, 4) and res[1][0].dtype == np.uint64 and (res[1][0] == 2 ** 53).all()
    assert (res[0][0] == 2).all() and (res[1][1] == 1.0).all()
    outb, wtb = ed.deform_grid_labels_batch(np.stack([L, L]), np.stack([D2, D2]), cval=1, return_weight=True)
    assert outb.shape == (2, 1, 9) and (outb == 1).all() and wtb.shape == (2, 1, 9) and (wtb == 1.0).all()
    B = np.ones((9, 1), dtype=np.bool_)
    assert not ed.deform_grid_labels(B, D2).any() and ed.deform_grid_labels(B, D2, cval=1).all()


def test_c_abi_checks_answer_before_any_launch(monkeypatch):
    """edhip_deform_labels: shape, dtype and flag checks with the existing status codes, on descriptors of memory
    that does not exist -- nothing is launched (no GPU here)."""
    import ctypes
    import os
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libedhip.so not built (run __graft_entry__.build())")
    monkeypatch.undo()
    INVALID, DTYPE, UNSUPPORTED = 1, 2, _lib.ERR_UNSUPPORTED

    def desc(shape, dtype="uint8"):
        a = np.empty(shape, dtype=dtype)
        return _lib.describe(0x1000, a.dtype.name, a.shape, a.strides)

    def status(inp=desc((8, 9)), disp=desc((2, 3, 3), "float64"), off=None, out=desc((8, 9)), wt=None, axis=(0, 1),
               mode=0, cval=0.0, K=None, flags=0, nb=1):
        """the raw status code and the message"""
        L = _lib.load()
        ax = (ctypes.c_int32 * len(axis))(*axis)
        buf = ctypes.create_string_buffer(256)
        st = L.edhip_deform_labels(nb, ctypes.byref(inp), 0, ctypes.byref(disp), 0, off, ctypes.byref(out), 0,
                                   ctypes.byref(wt) if wt is not None else None, 0, len(axis), ax, mode, cval, K,
                                   flags, None, buf, 256)
        return st, buf.value.decode()

    def check(code, match, **kw):
        st, msg = status(**kw)
        assert st == code and match in msg, (st, msg)

    check(INVALID, "integer or bool", inp=desc((8, 9), "float32"), out=desc((8, 9), "float32"))
    check(INVALID, "integer or bool", inp=desc((8, 9), "float64"), out=desc((8, 9), "float64"))
    check(INVALID, "one dtype", out=desc((8, 9), "int8"))
    check(INVALID, "prefiltered", flags=_lib.FLAG_RAW_DISPLACEMENT)
    check(UNSUPPORTED, "1 to 3 deformed axes", inp=desc((3, 3, 3, 3)), out=desc((3, 3, 3, 3)),
          disp=desc((4, 2, 2, 2, 2), "float64"), axis=(0, 1, 2, 3))
    check(INVALID, "at least 2 elements", inp=desc((8, 1)))
    for dtype, cval in (("uint8", 2.5), ("uint8", 256.0), ("uint8", -1.0), ("int8", -129.0), ("bool", 2.0),
                        ("int32", float("nan")), ("int64", 2.0 ** 63), ("uint64", 2.0 ** 64), ("uint64", -1.0)):
        check(INVALID, "cval", inp=desc((8, 9), dtype), out=desc((8, 9), dtype), cval=cval)
    check(INVALID, "dimensions should match", out=desc((8, 9, 1)))
    check(INVALID, "invalid axis", axis=(0, 2))
    check(INVALID, "invalid axis", axis=(1, 0))
    check(INVALID, "boundary mode", mode=5)
    check(INVALID, "invalid displacement shape", disp=desc((3, 3, 3), "float64"))
    check(INVALID, "non-deformed axes", inp=desc((4, 8, 9)), out=desc((5, 8, 9)), axis=(1, 2))
    check(INVALID, "shape of the output", wt=desc((8, 8), "float32"))
    check(DTYPE, "float32", wt=desc((8, 9), "float64"))
    # the wrapper maps the codes to the exceptions of the other entry points
    with pytest.raises(RuntimeError, match="prefiltered"):
        _lib.deform_labels(1, desc((8, 9)), 0, desc((2, 3, 3), "float64"), 0, None, desc((8, 9)), 0, None, 0, (0, 1),
                           0, 0.0, None, _lib.FLAG_RAW_DISPLACEMENT, 0)
    # accepted extremes of cval, no samples / no voxels: validated, nothing launched, EDHIP_OK
    for dtype, cval in (("int64", -2.0 ** 63), ("uint64", 2.0 ** 63), ("int8", -128.0), ("bool", 1.0)):
        assert status(inp=desc((8, 9), dtype), out=desc((8, 9), dtype), cval=cval, nb=0)[0] == 0
    assert status(out=desc((0, 9)), wt=desc((0, 9), "float32"))[0] == 0
