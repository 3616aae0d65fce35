"""
CPU tests of the host layer of deform_grid_coordinates_gradient / deform_points_gradient (and their batch forms): every
argument error is raised before the device or the library is touched -- `_lib.load` is replaced by a function that
fails, and no GPU is visible here anyway -- the crop / affine / rotate / zoom errors are the ones deform_grid raises,
and edhip_deform_points_gradient answers its shape / dtype / flag checks with the documented status codes on
descriptors of memory that does not exist.
"""
import ctypes

import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _lib

CALLS = [ed.deform_grid_coordinates_gradient, ed.deform_points_gradient]
BATCH_CALLS = [ed.deform_grid_coordinates_gradient_batch, ed.deform_points_gradient_batch]


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def _error_of(fn, *args, **kw):
    with pytest.raises(Exception) as info:
        fn(*args, **kw)
    assert "the library was loaded" not in str(info.value) and "needs a ROCm GPU" not in str(info.value)
    return type(info.value), str(info.value)


P2 = np.zeros((5, 2))
D2 = np.zeros((2, 3, 3))


def test_the_names_are_exported():
    for name in ("deform_grid_coordinates_gradient", "deform_points_gradient",
                 "deform_grid_coordinates_gradient_batch", "deform_points_gradient_batch"):
        assert callable(getattr(ed, name))
    assert ed.PointsGradient._fields == ("points", "displacement", "affine", "rotate", "zoom", "inverse_map")
    assert "edhip_deform_points_gradient" in _lib.EXPORTS


@pytest.mark.parametrize("fn", CALLS)
def test_cotangent_must_have_the_shape_of_the_points(fn):
    for cot in (np.zeros((4, 2)), np.zeros((5, 2, 1)), np.zeros(10)):
        assert _error_of(fn, P2, cot, D2, (8, 9))[0] is ValueError
    with pytest.raises(ValueError, match="cotangent"):
        fn(P2, np.zeros((4, 2)), D2, (8, 9))
    with pytest.raises(ValueError, match="positions"):
        ed.deform_points_gradient(P2, P2, D2, (8, 9), positions=np.zeros((4, 2)))


@pytest.mark.parametrize("fn", CALLS)
def test_last_dimension_must_equal_naxis(fn):
    with pytest.raises(ValueError, match="last dimension"):
        fn(np.zeros((5, 3)), np.zeros((5, 3)), D2, (8, 9))
    with pytest.raises(ValueError, match="last dimension"):
        fn(np.zeros((4, 5, 1)), np.zeros((4, 5, 1)), D2, (8, 9))
    with pytest.raises(ValueError, match="last dimension"):
        fn(P2, P2, np.zeros((1, 3)), (8, 9), axis=(1,))


@pytest.mark.parametrize("fn", CALLS + BATCH_CALLS)
def test_x_shape_is_required(fn):
    with pytest.raises(ValueError, match="X_shape"):
        fn(P2, P2, D2, None)


@pytest.mark.parametrize("fn", CALLS)
def test_zoom_zero_has_no_gradient(fn):
    with pytest.raises(ValueError, match="zoom=0"):
        fn(P2, P2, D2, (8, 9), zoom=0)


@pytest.mark.parametrize("fn", CALLS)
@pytest.mark.parametrize("kw", [
    dict(crop=(slice(0, 4),)),                                   # one slice for two axes
    dict(crop=(slice(0, 4), 3)),                                 # not a slice
    dict(crop=(slice(0, 4, 2), slice(0, 4))),                    # a step
    dict(crop=(slice(5, 4), slice(0, 4))),                       # empty
    dict(crop=(slice(0, 40), slice(0, 4))),                      # beyond the array
    dict(affine=np.eye(4)),                                      # wrong shape
    dict(affine=np.array([[1.0, 0, 0], [0, 1, 0], [0, 1, 1]])),  # homogeneous row
    dict(affine=np.zeros((2, 3))),                               # singular
    dict(displacement=np.zeros((3, 3, 3))),                      # first dimension
    dict(displacement=np.zeros((2, 3))),                         # dimensions
    dict(displacement=[[0.0]]),                                  # not an array
    dict(axis=(1, 0)),                                           # unsorted
    dict(axis=(0, 2)),                                           # out of range
])
def test_plan_errors_equal_deform_grid(fn, kw):
    kw = dict(kw)
    D = kw.pop("displacement", D2)
    X = np.zeros((8, 9), dtype=np.float32)
    want = _error_of(ed.deform_grid, X, D, **kw)
    assert _error_of(fn, P2, P2, D, X.shape, **kw) == want


@pytest.mark.parametrize("fn", CALLS)
def test_rotate_and_zoom_are_2d_only_like_deform_grid(fn):
    X = np.zeros((6, 7, 8), dtype=np.float32)
    D = np.zeros((3, 3, 3, 3))
    for kw in (dict(rotate=10.0), dict(zoom=1.5)):
        want = _error_of(ed.deform_grid, X, D, **kw)
        assert _error_of(fn, np.zeros((4, 3)), np.zeros((4, 3)), D, X.shape, **kw) == want
        assert want[0] is AssertionError


@pytest.mark.parametrize("fn", BATCH_CALLS)
def test_batch_shape_mismatches(fn):
    Db = np.zeros((3, 2, 3, 3))
    P3 = np.zeros((3, 5, 2))
    with pytest.raises(ValueError, match="batch, N, naxis"):
        fn(P2, P2, Db, (8, 9))                                   # no batch axis
    with pytest.raises(ValueError, match="batch, N, naxis"):
        fn(np.zeros((3, 2, 5, 2)), np.zeros((3, 2, 5, 2)), Db, (8, 9))
    with pytest.raises(AssertionError, match="One displacement grid per sample"):
        fn(P3[:2], P3[:2], Db, (8, 9))
    with pytest.raises(ValueError, match="last dimension"):
        fn(np.zeros((3, 5, 3)), np.zeros((3, 5, 3)), Db, (8, 9))
    with pytest.raises(ValueError, match="cotangent"):
        fn(P3, P3[:, :4], Db, (8, 9))
    with pytest.raises(Exception, match="displacements should be an array of shape"):
        fn(P3, P3, D2[0], (8, 9))
    with pytest.raises(AssertionError, match="First dimension of displacement"):
        fn(P3, P3, np.zeros((3, 3, 3, 3)), (8, 9))


@pytest.mark.parametrize("fn", CALLS)
def test_unsupported_dtypes(fn):
    for bad in (np.float16, np.complex64):
        with pytest.raises(RuntimeError, match="data type not supported"):
            fn(P2.astype(bad), P2, D2, (8, 9))
        with pytest.raises(RuntimeError, match="data type not supported"):
            fn(P2, P2.astype(bad), D2, (8, 9))


def test_solver_parameters():
    for tol in (0.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            ed.deform_points_gradient(P2, P2, D2, (8, 9), tol=tol)
    for max_iter in (0, -3, 2.5):
        with pytest.raises(ValueError, match="max_iter"):
            ed.deform_points_gradient(P2, P2, D2, (8, 9), max_iter=max_iter)


def test_length_one_axis_is_decided_on_the_host():
    """a deformed axis of length 1: zeros everywhere -- no device, no library"""
    P = np.zeros((2, 3, 2), dtype=np.float32)
    for fn in CALLS:
        g = fn(P, np.ones_like(P), D2.astype(np.float32), (1, 9), rotate=10.0)
        assert g.points.shape == P.shape and g.points.dtype == np.float32 and (g.points == 0).all()
        assert g.displacement.shape == D2.shape and g.displacement.dtype == np.float32 and (g.displacement == 0).all()
        assert g.affine.shape == (2, 3) and (g.affine == 0).all() and g.rotate == 0.0 and g.zoom is None
        assert g.inverse_map.shape == (2, 3) and (g.inverse_map == 0).all()
    for fn in BATCH_CALLS:
        g = fn(P, np.ones_like(P), np.zeros((2, 2, 3, 3)), (8, 1))
        assert g.points.shape == P.shape and g.displacement.shape == (2, 2, 3, 3) and (g.displacement == 0).all()
        assert g.inverse_map.shape == (2, 3) and (g.inverse_map == 0).all()


def test_c_abi_checks_answer_before_any_launch(monkeypatch):
    """edhip_deform_points_gradient: every shape, dtype and flag check with the existing status codes, on descriptors of
    memory that does not exist -- nothing is launched (no GPU here)."""
    import os
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libedhip.so not built (run __graft_entry__.build())")
    monkeypatch.undo()
    INVALID, DTYPE, UNSUPPORTED = 1, 2, _lib.ERR_UNSUPPORTED

    def desc(shape, dtype="float64"):
        a = np.empty(shape, dtype=dtype)
        return _lib.describe(0x1000, a.dtype.name, a.shape, a.strides)

    def ref(d):
        return ctypes.byref(d) if d is not None else None

    def status(inverse=0, nb=1, pos=desc((5, 2)), cot=desc((5, 2)), st=None, disp=desc((2, 3, 3)), in_len=(8, 9),
               naxis=2, K=None, dpts=desc((5, 2)), ddisp=desc((2, 3, 3)), dinv=desc((2, 3)), flags=0):
        L = _lib.load()
        lens = (ctypes.c_int64 * len(in_len))(*in_len)
        buf = ctypes.create_string_buffer(256)
        code = L.edhip_deform_points_gradient(inverse, nb, ref(pos), 0, ref(cot), 0, ref(st), 0, ref(disp), 0, lens,
                                              None, naxis, K, ref(dpts), 0, ref(ddisp), 0, ref(dinv), 0, flags, None,
                                              buf, 256)
        return code, buf.value.decode()

    def check(code, match, **kw):
        got, msg = status(**kw)
        assert got == code and match in msg, (got, msg)

    check(INVALID, "invalid batch", nb=-1)
    check(INVALID, "invalid batch", cot=None)
    check(INVALID, "invalid axis list", naxis=0)
    check(UNSUPPORTED, "deformed axes", naxis=8)
    check(INVALID, "prefiltered", flags=_lib.FLAG_RAW_DISPLACEMENT)
    check(INVALID, "none of", dpts=None, ddisp=None, dinv=None)
    check(INVALID, "positions must have shape", pos=desc((5, 3)))
    check(INVALID, "cotangent must have the shape", cot=desc((4, 2)))
    check(DTYPE, "data type not supported", pos=desc((5, 2), "int32"))
    check(DTYPE, "data type not supported", cot=desc((5, 2), "float16"))
    check(INVALID, "inverse direction", st=desc((5,), "uint8"))
    check(INVALID, "status must have shape", inverse=1, st=desc((4,), "uint8"))
    check(DTYPE, "status must be uint8", inverse=1, st=desc((5,), "bool"))
    check(INVALID, "invalid displacement shape", disp=desc((3, 3, 3)))
    check(INVALID, "dpoints must have the shape", dpts=desc((5, 3)))
    check(DTYPE, "data type not supported", dpts=desc((5, 2), "int64"))
    check(INVALID, "ddisplacement must have the shape", ddisp=desc((2, 3, 4)))
    check(DTYPE, "floating-point", ddisp=desc((2, 3, 3), "int32"))
    check(INVALID, "dinverse_affine must have shape", dinv=desc((3, 2)))
    check(DTYPE, "dinverse_affine must be float64", dinv=desc((2, 3), "float32"))
    check(UNSUPPORTED, "too many samples", nb=65536)
    check(INVALID, "at least 2 elements", in_len=(8, 1))
    # no samples; no points and only their rows wanted: validated, nothing launched, EDHIP_OK
    assert status(nb=0)[0] == 0
    assert status(pos=desc((0, 2)), cot=desc((0, 2)), dpts=desc((0, 2)), ddisp=None, dinv=None)[0] == 0
    # the wrapper maps the codes to the exceptions of the other entry points
    with pytest.raises(RuntimeError, match="inverse direction"):
        _lib.deform_points_gradient(0, 1, desc((5, 2)), 0, desc((5, 2)), 0, desc((5,), "uint8"), 0, desc((2, 3, 3)), 0,
                                    (8, 9), None, None, desc((5, 2)), 0, None, 0, None, 0, 0, 0)
