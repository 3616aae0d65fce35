"""
CPU tests of the host layer of deform_grid_coordinates / deform_points (and their batch forms): every argument error
is raised before the device or the library is touched -- `_lib.load` is replaced by a function that fails, and no
GPU is visible here anyway -- and the crop / affine / rotate / zoom errors are the ones deform_grid raises.
"""
import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _lib

CALLS = [ed.deform_grid_coordinates, ed.deform_points]
BATCH_CALLS = [ed.deform_grid_coordinates_batch, ed.deform_points_batch]


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


def test_the_four_names_are_exported():
    for name in ("deform_grid_coordinates", "deform_points", "deform_grid_coordinates_batch", "deform_points_batch"):
        assert callable(getattr(ed, name))
    assert "edhip_deform_points" in _lib.EXPORTS


@pytest.mark.parametrize("fn", CALLS)
def test_last_dimension_must_equal_naxis(fn):
    with pytest.raises(ValueError, match="last dimension"):
        fn(np.zeros((5, 3)), D2, (8, 9))
    with pytest.raises(ValueError, match="last dimension"):
        fn(np.zeros((4, 5, 1)), D2, (8, 9))
    # with `axis` the deformed axes are a subset of X's: naxis = 1 here
    with pytest.raises(ValueError, match="last dimension"):
        fn(P2, np.zeros((1, 3)), (8, 9), axis=(1,))


@pytest.mark.parametrize("fn", CALLS + BATCH_CALLS)
def test_x_shape_is_required(fn):
    with pytest.raises(ValueError, match="X_shape"):
        fn(P2, D2, None)


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
    assert _error_of(fn, P2, D, X.shape, **kw) == want


@pytest.mark.parametrize("fn", CALLS)
def test_rotate_and_zoom_are_2d_only_like_deform_grid(fn):
    X = np.zeros((6, 7, 8), dtype=np.float32)
    D = np.zeros((3, 3, 3, 3))
    for kw in (dict(rotate=10.0), dict(zoom=1.5)):
        want = _error_of(ed.deform_grid, X, D, **kw)
        assert _error_of(fn, np.zeros((4, 3)), D, X.shape, **kw) == want
        assert want[0] is AssertionError


@pytest.mark.parametrize("fn", BATCH_CALLS)
def test_batch_shape_mismatches(fn):
    Db = np.zeros((3, 2, 3, 3))
    with pytest.raises(ValueError, match="batch, N, naxis"):
        fn(P2, Db, (8, 9))                                       # no batch axis
    with pytest.raises(ValueError, match="batch, N, naxis"):
        fn(np.zeros((3, 2, 5, 2)), Db, (8, 9))
    with pytest.raises(AssertionError, match="One displacement grid per sample"):
        fn(np.zeros((2, 5, 2)), Db, (8, 9))
    with pytest.raises(ValueError, match="last dimension"):
        fn(np.zeros((3, 5, 3)), Db, (8, 9))
    with pytest.raises(Exception, match="displacements should be an array of shape"):
        fn(np.zeros((3, 5, 2)), D2[0], (8, 9))
    with pytest.raises(AssertionError, match="First dimension of displacement"):
        fn(np.zeros((3, 5, 2)), np.zeros((3, 3, 3, 3)), (8, 9))


@pytest.mark.parametrize("fn", [ed.deform_points, ed.deform_points_batch])
def test_solver_parameters(fn):
    P = P2 if fn is ed.deform_points else P2[None]
    D = D2 if fn is ed.deform_points else D2[None]
    for tol in (0.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            fn(P, D, (8, 9), tol=tol)
    for max_iter in (0, -3, 2.5):
        with pytest.raises(ValueError, match="max_iter"):
            fn(P, D, (8, 9), max_iter=max_iter)


@pytest.mark.parametrize("fn", CALLS)
def test_unsupported_point_dtypes(fn):
    with pytest.raises(RuntimeError, match="data type not supported"):
        fn(P2.astype(np.float16), D2, (8, 9))
    with pytest.raises(RuntimeError, match="data type not supported"):
        fn(P2.astype(np.complex64), D2, (8, 9))


def test_length_one_axis_is_decided_on_the_host():
    """a deformed axis of length 1: NaN coordinates, nothing converged -- no device, no library"""
    P = np.zeros((2, 3, 2), dtype=np.float32)
    r, J = ed.deform_grid_coordinates(P, D2, (1, 9), jacobian=True)
    assert r.shape == (2, 3, 2) and r.dtype == np.float32 and np.isnan(r).all()
    assert J.shape == (2, 3, 2, 2) and J.dtype == np.float64 and np.isnan(J).all()
    q, ok = ed.deform_points(P.astype(np.int32), D2, (8, 1), return_converged=True)
    assert q.shape == (2, 3, 2) and q.dtype == np.float64 and np.isnan(q).all()
    assert ok.shape == (2, 3) and ok.dtype == np.bool_ and not ok.any()
    qb, okb = ed.deform_points_batch(P, np.zeros((2, 2, 3, 3)), (8, 1), return_converged=True)
    assert np.isnan(qb).all() and okb.shape == (2, 3) and not okb.any()


def test_c_abi_checks_answer_before_any_launch(monkeypatch):
    """edhip_deform_points: shape, dtype and flag checks with the existing status codes, on descriptors of memory
    that does not exist -- nothing is launched (no GPU here)."""
    import os
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libedhip.so not built (run __graft_entry__.build())")
    monkeypatch.undo()

    def desc(shape, dtype="float64"):
        a = np.empty(shape, dtype=dtype)
        return _lib.describe(0x1000, a.dtype.name, a.shape, a.strides)

    def call(inverse=False, pts=desc((5, 2)), disp=desc((2, 3, 3)), in_len=(8, 9), off=None, K=None, M=None,
             res=desc((5, 2)), jac=None, st=None, max_iter=32, tol=1e-9, flags=0, nb=1):
        _lib.deform_points(inverse, nb, pts, 0, disp, 0, in_len, off, K, M, res, 0, jac, 0, st, 0, max_iter, tol,
                           flags, 0)

    with pytest.raises(RuntimeError, match="points must have shape"):
        call(pts=desc((5, 3)))
    with pytest.raises(RuntimeError, match="result must have the shape of points"):
        call(res=desc((4, 2)))
    with pytest.raises(RuntimeError, match="data type not supported"):
        call(pts=desc((5, 2), "int32"))
    with pytest.raises(RuntimeError, match="data type not supported"):
        call(res=desc((5, 2), "float16"))
    with pytest.raises(RuntimeError, match="jacobian must have shape"):
        call(jac=desc((5, 2, 3)))
    with pytest.raises(RuntimeError, match="jacobian must be float64"):
        call(jac=desc((5, 2, 2), "float32"))
    with pytest.raises(RuntimeError, match="forward direction"):
        call(inverse=True, jac=desc((5, 2, 2)))
    with pytest.raises(RuntimeError, match="inverse direction"):
        call(st=desc((5,), "uint8"))
    with pytest.raises(RuntimeError, match="status must have shape"):
        call(inverse=True, st=desc((4,), "uint8"))
    with pytest.raises(RuntimeError, match="status must be uint8"):
        call(inverse=True, st=desc((5,), "bool"))
    with pytest.raises(RuntimeError, match="invalid displacement shape"):
        call(disp=desc((3, 3, 3)))
    with pytest.raises(RuntimeError, match="prefiltered"):
        call(flags=_lib.FLAG_RAW_DISPLACEMENT)
    with pytest.raises(RuntimeError, match="max_iter"):
        call(inverse=True, max_iter=0)
    with pytest.raises(RuntimeError, match="tol"):
        call(inverse=True, tol=0.0)
    with pytest.raises(RuntimeError, match="forward_linear"):
        call(inverse=True, K=np.array([[1.0, 0, 0], [0, 1, 0]]))
    with pytest.raises(RuntimeError, match="at least 2 elements"):
        call(in_len=(8, 1))
    # no points, or no samples: validated, nothing launched, EDHIP_OK
    call(pts=desc((0, 2)), res=desc((0, 2)))
    call(nb=0)
