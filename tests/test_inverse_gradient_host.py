"""
CPU tests of the host layer of deform_grid_inverse_gradient / deform_grid_inverse_gradient_batch: every argument error
is raised before the device or the library is touched -- `_lib.load` is replaced by a function that fails, and no GPU
is visible here anyway -- and edhip_deform_inverse_gradient answers its shape / dtype / flag checks with the documented
status codes on descriptors of memory that does not exist.
"""
import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _lib

CALLS = [ed.deform_grid_inverse_gradient, ed.deform_grid_inverse_gradient_batch]


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
DZ2 = np.zeros(I2)                     # the shape of X
D2 = np.zeros((2, 3, 3))


def _args(fn, dZ, D):
    """the single call's arguments, or the same with a leading batch axis of 2"""
    if fn is ed.deform_grid_inverse_gradient:
        return dZ, D
    return np.stack([dZ, dZ]), np.stack([D, D])


def test_the_names_are_exported():
    import elasticdeform_amd.torch as et
    for name in ("deform_grid_inverse_gradient", "deform_grid_inverse_gradient_batch"):
        assert callable(getattr(ed, name))
        assert getattr(et, name) is getattr(ed, name)
    assert "edhip_deform_inverse_gradient" in _lib.EXPORTS


@pytest.mark.parametrize("fn", CALLS)
def test_crop_outside_the_cotangent(fn):
    """dZ has the shape of X: a crop that does not fit it is deform_grid's own error"""
    dZ, D = _args(fn, np.zeros((10, 17)), D2)
    _raises(AssertionError, fn, dZ, D, crop=CROP2)                           # slice(2, 11) of an axis of 10
    dZ, D = _args(fn, DZ2, D2)
    _raises(AssertionError, fn, dZ, D, crop=(slice(2, 11),))                 # one slice for two axes
    _raises(AssertionError, fn, dZ, D, crop=(slice(2, 11), slice(3, 18)))    # past the end


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("kw, match", [(dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"),
                                       (dict(max_iter=-3), "max_iter"), (dict(tol=0.0), "tol"),
                                       (dict(tol=-1e-9), "tol"), (dict(tol=float("nan")), "tol")])
def test_iteration_controls_are_checked(fn, kw, match):
    dZ, D = _args(fn, DZ2, D2)
    assert match in _raises(ValueError, fn, dZ, D, crop=CROP2, **kw)


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("dtype", [np.int32, np.uint8, np.int64, np.bool_, np.float16, np.complex64])
def test_only_float32_and_float64_cotangents(fn, dtype):
    dZ, D = _args(fn, DZ2.astype(dtype), D2)
    assert "data type not supported" in _raises(RuntimeError, fn, dZ, D, crop=CROP2)


def test_float16_stays_refused_with_reduced_precision():
    ed.set_reduced_precision(True)
    try:
        assert "data type not supported" in _raises(RuntimeError, ed.deform_grid_inverse_gradient,
                                                    DZ2.astype(np.float16), D2, crop=CROP2)
    finally:
        ed.set_reduced_precision(False)


def test_more_than_three_deformed_axes():
    assert "1 to 3 deformed axes" in _raises(RuntimeError, ed.deform_grid_inverse_gradient, np.zeros((3, 3, 3, 3)),
                                             np.zeros((4, 2, 2, 2, 2)))


def test_list_inputs_with_mismatched_per_input_lists():
    dZs = [DZ2, np.zeros(I2 + (3,))]
    axis = [(0, 1), (0, 1)]
    fn = ed.deform_grid_inverse_gradient
    assert "order" in _raises(AssertionError, fn, dZs, D2, crop=CROP2, axis=axis, order=[3, 1, 0])
    assert "mode" in _raises(AssertionError, fn, dZs, D2, crop=CROP2, axis=axis, mode=["mirror"])
    assert "axis" in _raises(AssertionError, fn, dZs, D2, crop=CROP2, axis=[(0, 1)])
    # inputs whose deformed shapes differ
    _raises(AssertionError, fn, [DZ2, np.zeros((13, 16))], D2, crop=CROP2)


def test_batch_shape_mismatches():
    dZb, Db = np.stack([DZ2] * 3), np.stack([D2] * 3)
    fn = ed.deform_grid_inverse_gradient_batch
    assert "One displacement grid per sample" in _raises(AssertionError, fn, dZb[:2], Db, crop=CROP2)
    assert "leading batch axis" in _raises(Exception, fn, np.zeros(8), Db)
    assert "shared by the batch" in _raises(AssertionError, fn, dZb, Db, crop=CROP2, order=[3, 3, 3])


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
    """every other argument error is deform_grid's own, on an array of dZ's shape"""
    kw = dict(kw)
    D = kw.pop("displacement", D2)
    with pytest.raises(Exception) as want:
        ed.deform_grid(np.zeros(I2), D, crop=CROP2, **kw)
    with pytest.raises(Exception) as got:
        ed.deform_grid_inverse_gradient(DZ2, D, crop=CROP2, **kw)
    assert (type(got.value), str(got.value)) == (type(want.value), str(want.value))
    assert "the library was loaded" not in str(got.value) and "needs a ROCm GPU" not in str(got.value)


def test_short_axes_are_decided_on_the_host():
    """a deformed axis of X of length 1: nothing depends on Y -- zeros of Y's shape and dZ's dtype, no device, no
    library; a deformed axis of Y of length 1 (a one-voxel crop) is refused as in the forward"""
    dZ = np.ones((1, 9), dtype=np.float32)
    g = ed.deform_grid_inverse_gradient(dZ, D2)
    assert isinstance(g, np.ndarray) and g.shape == (1, 9) and g.dtype == np.float32 and not g.any()
    res = ed.deform_grid_inverse_gradient([dZ, np.ones((1, 9, 2))], D2, crop=(slice(0, 1), slice(2, 6)),
                                          axis=[(0, 1), (0, 1)])
    assert isinstance(res, list) and len(res) == 2
    assert res[0].shape == (1, 4) and res[0].dtype == np.float32 and not res[0].any()
    assert res[1].shape == (1, 4, 2) and res[1].dtype == np.float64 and not res[1].any()
    gb = ed.deform_grid_inverse_gradient_batch(np.stack([dZ, dZ]), np.stack([D2, D2]))
    assert gb.shape == (2, 1, 9) and gb.dtype == np.float32 and not gb.any()
    assert "at least 2 elements" in _raises(ValueError, ed.deform_grid_inverse_gradient, DZ2, D2,
                                            crop=(slice(4, 5), slice(3, 15)))


def test_c_abi_checks_answer_before_any_launch(monkeypatch):
    """edhip_deform_inverse_gradient: shape, dtype and flag checks with the existing status codes, on descriptors of
    memory that does not exist -- nothing is launched (no GPU here)."""
    import ctypes
    import os
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libedhip.so not built (run __graft_entry__.build())")
    monkeypatch.undo()
    INVALID, DTYPE, UNSUPPORTED = 1, 2, _lib.ERR_UNSUPPORTED

    def desc(shape, dtype="float64"):
        a = np.empty(shape, dtype=dtype)
        return _lib.describe(0x1000, a.dtype.name, a.shape, a.strides)

    def status(cot=desc((13, 17)), disp=desc((2, 3, 3)), in_len=(13, 17), off=(2, 3), din=desc((9, 12)), axis=(0, 1),
               order=3, mode=0, K=None, M=None, max_iter=32, tol=1e-9, flags=0, nb=1):
        """the raw status code and the message"""
        L = _lib.load()
        ax = (ctypes.c_int32 * len(axis))(*axis)
        il = (ctypes.c_int64 * len(in_len))(*in_len)
        of = (ctypes.c_int64 * len(off))(*off) if off is not None else None
        Kp = (ctypes.c_double * len(K))(*K) if K is not None else None
        Mp = (ctypes.c_double * len(M))(*M) if M is not None else None
        buf = ctypes.create_string_buffer(256)
        st = L.edhip_deform_inverse_gradient(nb, ctypes.byref(cot), 0, ctypes.byref(disp), 0, il, of,
                                             ctypes.byref(din), 0, len(axis), ax, order, mode, Kp, Mp, max_iter, tol,
                                             flags, None, buf, 256)
        return st, buf.value.decode()

    def check(code, match, **kw):
        st, msg = status(**kw)
        assert st == code and match in msg, (st, msg)

    check(INVALID, "prefiltered", flags=_lib.FLAG_RAW_DISPLACEMENT)
    check(UNSUPPORTED, "1 to 3 deformed axes", cot=desc((3, 3, 3, 3)), din=desc((3, 3, 3, 3)),
          disp=desc((4, 2, 2, 2, 2)), axis=(0, 1, 2, 3), in_len=(3, 3, 3, 3), off=None)
    check(DTYPE, "one dtype", din=desc((9, 12), "float32"))
    check(DTYPE, "one dtype", cot=desc((13, 17), "float32"))
    for name in ("int32", "uint8", "int64", "bool", "float16"):
        check(DTYPE, "not supported", cot=desc((13, 17), name), din=desc((9, 12), name))
    check(INVALID, "max_iter", max_iter=0)
    check(INVALID, "tol", tol=0.0)
    check(INVALID, "tol", tol=float("nan"))
    check(INVALID, "at least 2 elements", din=desc((9, 1)))
    check(INVALID, "at least 2 elements", in_len=(13, 1), cot=desc((13, 1)))
    check(INVALID, "extents in_len", cot=desc((13, 16)))
    check(INVALID, "dimensions should match", cot=desc((13, 17, 1)))
    check(INVALID, "invalid axis", axis=(0, 2))
    check(INVALID, "invalid axis", axis=(1, 0))
    check(INVALID, "spline order", order=6)
    check(INVALID, "boundary mode", mode=5)
    check(INVALID, "invalid displacement shape", disp=desc((3, 3, 3)))
    check(INVALID, "non-deformed axes", din=desc((4, 9, 12)), cot=desc((5, 13, 17)), axis=(1, 2))
    check(INVALID, "forward_linear", K=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
    check(UNSUPPORTED, "too many samples", nb=65536)
    check(INVALID, "invalid batch", nb=-1)
    # the wrapper maps the codes to the exceptions of the other entry points
    with pytest.raises(RuntimeError, match="prefiltered"):
        _lib.deform_inverse_gradient(1, desc((13, 17)), 0, desc((2, 3, 3)), 0, (13, 17), (2, 3), desc((9, 12)), 0,
                                     (0, 1), 3, 0, None, None, 32, 1e-9, _lib.FLAG_RAW_DISPLACEMENT, 0)
    # no samples: validated, nothing launched, EDHIP_OK
    assert status(nb=0)[0] == 0
    assert status(nb=0, K=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), M=(1.0, 0.0, 0.0, 1.0))[0] == 0
