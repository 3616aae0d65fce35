"""
CPU tests of the host layer of deform_grid_inverse_displacement_gradient / deform_grid_inverse_affine_gradient and their
batch forms: every argument error is raised before the device or the library is touched -- `_lib.load` is replaced by
a function that fails, and no GPU is visible here anyway -- and edhip_deform_inverse_transform_gradient answers its
shape / dtype / flag checks with the documented status codes on descriptors of memory that does not exist.
"""
import inspect

import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _lib

SINGLE = [ed.deform_grid_inverse_displacement_gradient, ed.deform_grid_inverse_affine_gradient]
BATCH = [ed.deform_grid_inverse_displacement_gradient_batch, ed.deform_grid_inverse_affine_gradient_batch]
CALLS = SINGLE + BATCH


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
Y2 = np.zeros((9, 12))                 # the shape the forward returns for the crop
DZ2 = np.zeros(I2)                     # the shape of X
D2 = np.zeros((2, 3, 3))


def _args(fn, Y, dZ, D):
    """the single call's arguments, or the same with a leading batch axis of 2"""
    if fn in SINGLE:
        return Y, dZ, D
    return np.stack([Y, Y]), np.stack([dZ, dZ]), np.stack([D, D])


def test_the_names_are_exported():
    import elasticdeform_amd.torch as et
    for fn in CALLS:
        assert getattr(ed, fn.__name__) is fn and getattr(et, fn.__name__) is fn
    assert "edhip_deform_inverse_transform_gradient" in _lib.EXPORTS
    assert et.deform_grid_inverse is ed.deform_grid_inverse
    for fn in (ed.deform_grid_inverse, ed.deform_grid_inverse_batch):
        p = inspect.signature(fn).parameters
        for name in ("displacement_grad", "affine_grad"):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is False


def test_the_signature_of_the_issue():
    names = list(inspect.signature(ed.deform_grid_inverse_displacement_gradient).parameters)
    assert names == ["Y", "dZ", "displacement", "order", "mode", "crop", "prefilter", "axis", "affine", "rotate", "zoom",
                     "max_iter", "tol"]


@pytest.mark.parametrize("fn", CALLS)
def test_y_must_have_the_shape_the_forward_returns(fn):
    Y, dZ, D = _args(fn, np.zeros((9, 13)), DZ2, D2)
    assert "Expected shape of Y" in _raises(ValueError, fn, Y, dZ, D, crop=CROP2)
    Y, dZ, D = _args(fn, DZ2, DZ2, D2)                                      # Y of X's shape under a crop
    assert "Expected shape of Y" in _raises(ValueError, fn, Y, dZ, D, crop=CROP2)
    Y, dZ, D = _args(fn, Y2, np.zeros((10, 17)), D2)
    _raises(AssertionError, fn, Y, dZ, D, crop=CROP2)                       # slice(2, 11) of an axis of 10


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("kw, match", [(dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"),
                                       (dict(tol=0.0), "tol"), (dict(tol=float("nan")), "tol")])
def test_iteration_controls_are_checked(fn, kw, match):
    Y, dZ, D = _args(fn, Y2, DZ2, D2)
    assert match in _raises(ValueError, fn, Y, dZ, D, crop=CROP2, **kw)


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("dtype", [np.int32, np.uint8, np.bool_, np.float16, np.complex64])
@pytest.mark.parametrize("which", ["Y", "dZ"])
def test_only_float32_and_float64_volumes(fn, dtype, which):
    Y, dZ = (Y2.astype(dtype), DZ2) if which == "Y" else (Y2, DZ2.astype(dtype))
    Y, dZ, D = _args(fn, Y, dZ, D2)
    assert "data type not supported" in _raises(RuntimeError, fn, Y, dZ, D, crop=CROP2)


@pytest.mark.parametrize("fn", [ed.deform_grid_inverse_affine_gradient, ed.deform_grid_inverse_affine_gradient_batch])
def test_zoom_0_has_no_gradient(fn):
    Y, dZ, D = _args(fn, Y2, DZ2, D2)
    assert "zoom=0" in _raises(ValueError, fn, Y, dZ, D, crop=CROP2, rotate=10, zoom=0)


def test_more_than_three_deformed_axes():
    assert "1 to 3 deformed axes" in _raises(RuntimeError, ed.deform_grid_inverse_displacement_gradient,
                                             np.zeros((3, 3, 3, 3)), np.zeros((3, 3, 3, 3)), np.zeros((4, 2, 2, 2, 2)))


def test_list_inputs_with_mismatched_lists():
    fn = ed.deform_grid_inverse_displacement_gradient
    Ys, dZs = [Y2, np.zeros((9, 12, 3))], [DZ2, np.zeros(I2 + (3,))]
    axis = [(0, 1), (0, 1)]
    assert "order" in _raises(AssertionError, fn, Ys, dZs, D2, crop=CROP2, axis=axis, order=[3, 1, 0])
    assert "Expected shape of Y" in _raises(ValueError, fn, Ys[:1], dZs, D2, crop=CROP2, axis=axis)
    assert "Expected shape of Y" in _raises(ValueError, fn, Ys[::-1], dZs, D2, crop=CROP2, axis=axis)


def test_batch_shape_mismatches():
    fn = ed.deform_grid_inverse_displacement_gradient_batch
    Yb, dZb, Db = np.stack([Y2] * 3), np.stack([DZ2] * 3), np.stack([D2] * 3)
    assert "One displacement grid per sample" in _raises(AssertionError, fn, Yb[:2], dZb[:2], Db, crop=CROP2)
    assert "leading batch axis" in _raises(Exception, fn, Yb, np.zeros(8), Db)
    assert "Expected shape of Y" in _raises(ValueError, fn, Yb[:2], dZb, Db, crop=CROP2)


@pytest.mark.parametrize("kw", [
    dict(displacement=np.zeros((3, 3, 3))),                      # first dimension
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
        ed.deform_grid_inverse_displacement_gradient(Y2, DZ2, D, crop=CROP2, **kw)
    assert (type(got.value), str(got.value)) == (type(want.value), str(want.value))
    assert "the library was loaded" not in str(got.value) and "needs a ROCm GPU" not in str(got.value)


def test_zeros_are_decided_on_the_host():
    """order 0 and a deformed axis of X of length 1: zeros of the displacement's shape and dtype, no device, no
    library; a deformed axis of Y of length 1 (a one-voxel crop) is refused as in the forward"""
    D32 = np.zeros((2, 3, 3), dtype=np.float32)
    for Y, dZ, kw in ((Y2, DZ2, dict(crop=CROP2, order=0)), (np.ones((1, 9)), np.ones((1, 9)), dict())):
        g = ed.deform_grid_inverse_displacement_gradient(Y, dZ, D32, **kw)
        assert isinstance(g, np.ndarray) and g.shape == D32.shape and g.dtype == np.float32 and not g.any()
        a = ed.deform_grid_inverse_affine_gradient(Y, dZ, D32, rotate=10, **kw)
        assert a.affine.shape == (2, 3) and not a.affine.any() and a.rotate == 0.0 and a.zoom is None
        assert not a.inverse_map.any()
        gb = ed.deform_grid_inverse_displacement_gradient_batch(np.stack([Y, Y]), np.stack([dZ, dZ]),
                                                                np.stack([D32, D32]), **kw)
        assert gb.shape == (2,) + D32.shape and not gb.any()
    Di = np.zeros((2, 3, 3), dtype=np.int16)                     # an integer grid: float64
    assert ed.deform_grid_inverse_displacement_gradient(Y2, DZ2, Di, crop=CROP2, order=0).dtype == np.float64
    assert "at least 2 elements" in _raises(ValueError, ed.deform_grid_inverse_displacement_gradient,
                                            np.zeros((1, 12)), DZ2, D2, crop=(slice(4, 5), slice(3, 15)))


def test_c_abi_checks_answer_before_any_launch(monkeypatch):
    """edhip_deform_inverse_transform_gradient: shape, dtype and flag checks with the existing status codes, on
    descriptors of memory that does not exist -- nothing is launched (no GPU here)."""
    import ctypes
    import os
    assert os.path.exists(_lib.LIB_PATH), "libedhip.so not built (run __graft_entry__.build())"
    monkeypatch.undo()
    INVALID, DTYPE, UNSUPPORTED = 1, 2, _lib.ERR_UNSUPPORTED

    def desc(shape, dtype="float64"):
        a = np.empty(shape, dtype=dtype)
        return _lib.describe(0x1000, a.dtype.name, a.shape, a.strides)

    NONE = object()

    def status(inp=desc((9, 12)), cot=desc((13, 17)), disp=desc((2, 3, 3)), in_len=(13, 17), off=(2, 3),
               ddisp=desc((2, 3, 3)), dinv=desc((2, 3)), axis=(0, 1), order=3, mode=0, K=None, M=None, max_iter=32,
               tol=1e-9, flags=0, nb=1):
        """the raw status code and the message"""
        L = _lib.load()
        ax = (ctypes.c_int32 * len(axis))(*axis)
        il = (ctypes.c_int64 * len(in_len))(*in_len)
        of = (ctypes.c_int64 * len(off))(*off) if off is not None else None
        Kp = (ctypes.c_double * len(K))(*K) if K is not None else None
        Mp = (ctypes.c_double * len(M))(*M) if M is not None else None
        ref = lambda d: None if d is NONE else ctypes.byref(d)   # noqa: E731
        buf = ctypes.create_string_buffer(256)
        st = L.edhip_deform_inverse_transform_gradient(nb, ctypes.byref(inp), 0, ctypes.byref(cot), 0,
                                                       ctypes.byref(disp), 0, il, of, ref(ddisp), 0, ref(dinv), 0,
                                                       len(axis), ax, order, mode, Kp, Mp, max_iter, tol, flags, None,
                                                       buf, 256)
        return st, buf.value.decode()

    def check(code, match, **kw):
        st, msg = status(**kw)
        assert st == code and match in msg, (st, msg)

    check(INVALID, "prefiltered", flags=_lib.FLAG_RAW_DISPLACEMENT)
    check(UNSUPPORTED, "1 to 3 deformed axes", inp=desc((3, 3, 3, 3)), cot=desc((3, 3, 3, 3)),
          disp=desc((4, 2, 2, 2, 2)), ddisp=desc((4, 2, 2, 2, 2)), dinv=desc((4, 5)), axis=(0, 1, 2, 3),
          in_len=(3, 3, 3, 3), off=None)
    check(DTYPE, "one dtype", inp=desc((9, 12), "float32"))
    check(DTYPE, "one dtype", cot=desc((13, 17), "float32"))
    for name in ("int32", "uint8", "int64", "bool", "float16"):
        check(DTYPE, "not supported", cot=desc((13, 17), name), inp=desc((9, 12), name))
    check(INVALID, "neither ddisplacement nor dinverse_affine", ddisp=NONE, dinv=NONE)
    check(INVALID, "shape of displacement", ddisp=desc((2, 3, 4)))
    check(DTYPE, "floating-point", ddisp=desc((2, 3, 3), "int32"))
    check(INVALID, "(naxis, naxis + 1)", dinv=desc((3, 2)))
    check(DTYPE, "float64", dinv=desc((2, 3), "float32"))
    check(INVALID, "max_iter", max_iter=0)
    check(INVALID, "tol", tol=0.0)
    check(INVALID, "tol", tol=float("nan"))
    check(INVALID, "at least 2 elements", inp=desc((9, 1)))
    check(INVALID, "at least 2 elements", in_len=(13, 1), cot=desc((13, 1)))
    check(INVALID, "extents in_len", cot=desc((13, 16)))
    check(INVALID, "dimensions should match", cot=desc((13, 17, 1)))
    check(INVALID, "invalid axis", axis=(0, 2))
    check(INVALID, "invalid axis", axis=(1, 0))
    check(INVALID, "spline order", order=6)
    check(INVALID, "boundary mode", mode=5)
    check(INVALID, "invalid displacement shape", disp=desc((3, 3, 3)), ddisp=desc((3, 3, 3)))
    check(INVALID, "non-deformed axes", inp=desc((4, 9, 12)), cot=desc((5, 13, 17)), axis=(1, 2))
    check(INVALID, "forward_linear", K=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0))
    check(UNSUPPORTED, "too many samples", nb=65536)
    check(INVALID, "invalid batch", nb=-1)
    # one of the two results is enough; every floating dtype serves for ddisplacement
    assert status(nb=0, dinv=NONE)[0] == 0 and status(nb=0, ddisp=NONE)[0] == 0
    assert status(nb=0, ddisp=desc((2, 3, 3), "float16"))[0] == 0
    # the wrapper maps the codes to the exceptions of the other entry points
    with pytest.raises(RuntimeError, match="prefiltered"):
        _lib.deform_inverse_transform_gradient(1, desc((9, 12)), 0, desc((13, 17)), 0, desc((2, 3, 3)), 0, (13, 17),
                                               (2, 3), desc((2, 3, 3)), 0, desc((2, 3)), 0, (0, 1), 3, 0, None, None,
                                               32, 1e-9, _lib.FLAG_RAW_DISPLACEMENT, 0)
    # no samples: validated, nothing launched, EDHIP_OK
    assert status(nb=0)[0] == 0
    assert status(nb=0, K=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), M=(1.0, 0.0, 0.0, 1.0))[0] == 0
