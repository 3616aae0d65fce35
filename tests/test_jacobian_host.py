"""
CPU tests of the host layer of deform_grid_jacobian / deform_grid_jacobian_gradient (and their batch forms): every
argument error is raised before the device or the library is touched -- `_lib.load` is replaced by a function that
fails, and no GPU is visible here anyway -- and the crop / affine / rotate / zoom / displacement errors are the ones
deform_grid raises.  The results for a deformed axis of length 1 come back without the library.
"""
import numpy as np
import pytest

import elasticdeform_amd as ed
import elasticdeform_amd.torch as etorch
from elasticdeform_amd import _lib

torch = pytest.importorskip("torch")


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


D2 = np.zeros((2, 3, 3))
G2 = np.zeros((8, 9))


def _forward(D, X_shape, **kw):
    return ed.deform_grid_jacobian(D, X_shape, **kw)


def _gradient(D, X_shape, **kw):
    return ed.deform_grid_jacobian_gradient(G2, D, X_shape, **kw)


CALLS = [_forward, _gradient]


def test_the_names_are_exported():
    for name in ("deform_grid_jacobian", "deform_grid_jacobian_gradient", "deform_grid_jacobian_batch",
                 "deform_grid_jacobian_gradient_batch"):
        assert callable(getattr(ed, name))
        assert callable(getattr(etorch, name))
    assert ed.JacobianGradient._fields == ("displacement", "affine", "rotate", "zoom", "inverse_map")
    assert "edhip_deform_jacobian" in _lib.EXPORTS and "edhip_deform_jacobian_gradient" in _lib.EXPORTS
    assert "deform_grid_jacobian" in ed.__doc__


def test_x_shape_is_required():
    for fn in (ed.deform_grid_jacobian, ed.deform_grid_jacobian_batch, etorch.deform_grid_jacobian):
        with pytest.raises(ValueError, match="X_shape"):
            fn(D2, None)
    for fn in (ed.deform_grid_jacobian_gradient, ed.deform_grid_jacobian_gradient_batch):
        with pytest.raises(ValueError, match="X_shape"):
            fn(G2, D2, None)


def test_more_than_three_axes():
    D4 = np.zeros((4, 3, 3, 3, 3))
    with pytest.raises(ValueError, match="1 to 3 deformed axes"):
        ed.deform_grid_jacobian(D4, (5, 6, 7, 8))
    with pytest.raises(ValueError, match="1 to 3 deformed axes"):
        ed.deform_grid_jacobian_gradient(np.zeros((5, 6, 7, 8)), D4, (5, 6, 7, 8))
    with pytest.raises(ValueError, match="1 to 3 deformed axes"):
        ed.deform_grid_jacobian_batch(D4[None], (5, 6, 7, 8))


@pytest.mark.parametrize("dtype", ["float16", "int32", np.complex64, "bfloat16", torch.float16, torch.int64, 3.5,
                                   object()])
def test_a_bad_dtype(dtype):
    with pytest.raises(ValueError, match="dtype"):
        ed.deform_grid_jacobian(D2, (8, 9), dtype=dtype)
    with pytest.raises(ValueError, match="dtype"):
        ed.deform_grid_jacobian_batch(D2[None], (8, 9), dtype=dtype)


def test_the_cotangent():
    with pytest.raises(ValueError, match="shape of det"):
        ed.deform_grid_jacobian_gradient(np.zeros((8, 8)), D2, (8, 9))
    with pytest.raises(ValueError, match="shape of det"):                       # the crop applies
        ed.deform_grid_jacobian_gradient(G2, D2, (8, 9), crop=(slice(1, 5), slice(0, 9)))
    with pytest.raises(ValueError, match="shape of det"):                       # the deformed axes only
        ed.deform_grid_jacobian_gradient(np.zeros((4, 8, 9)), D2, (4, 8, 9), axis=(1, 2))
    with pytest.raises(ValueError, match="shape of det"):                       # the batch axis
        ed.deform_grid_jacobian_gradient_batch(G2, D2[None, :].repeat(2, 0), (8, 9))
    for dtype in (np.float16, np.int32, np.complex128):
        with pytest.raises(ValueError, match="float32 or float64"):
            ed.deform_grid_jacobian_gradient(G2.astype(dtype), D2, (8, 9))
    with pytest.raises(ValueError, match="float32 or float64"):
        ed.deform_grid_jacobian_gradient(torch.zeros((8, 9), dtype=torch.bfloat16), D2, (8, 9))


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
    assert _error_of(fn, D, X.shape, **kw) == want


@pytest.mark.parametrize("fn", CALLS)
def test_rotate_and_zoom_are_2d_only_like_deform_grid(fn):
    X = np.zeros((6, 7, 8), dtype=np.float32)
    D = np.zeros((3, 3, 3, 3))
    for kw in (dict(rotate=10.0), dict(zoom=1.5)):
        want = _error_of(ed.deform_grid, X, D, **kw)
        assert _error_of(fn, D, X.shape, **kw) == want
        assert want[0] is AssertionError


def test_batch_shape_mismatches():
    with pytest.raises(Exception, match="displacements should be an array of shape"):
        ed.deform_grid_jacobian_batch(D2[0], (8, 9))
    with pytest.raises(AssertionError, match="First dimension of displacement"):
        ed.deform_grid_jacobian_batch(np.zeros((3, 3, 3, 3)), (8, 9))
    with pytest.raises(Exception, match="displacements should be an array of shape"):
        ed.deform_grid_jacobian_gradient_batch(G2[None], D2[0], (8, 9))


def test_zoom_zero_has_no_gradient():
    with pytest.raises(ValueError, match="zoom=0"):
        ed.deform_grid_jacobian_gradient(G2, D2, (8, 9), zoom=0)
    with pytest.raises(ValueError, match="zoom=0"):
        ed.deform_grid_jacobian_gradient_batch(G2[None], D2[None], (8, 9), zoom=0.0)


def test_length_one_axis_is_decided_on_the_host():
    """a deformed axis of length 1: NaN det, zero gradients -- no device, no library"""
    det = ed.deform_grid_jacobian(D2, (1, 9))
    assert det.shape == (1, 9) and det.dtype == np.float64 and np.isnan(det).all()
    det = ed.deform_grid_jacobian(D2.astype(np.float32), (8, 1), dtype="float32")
    assert det.shape == (8, 1) and det.dtype == np.float32 and np.isnan(det).all()
    det = ed.deform_grid_jacobian_batch(np.zeros((3, 2, 3, 3)), (8, 1), crop=(slice(2, 6), slice(0, 1)))
    assert det.shape == (3, 4, 1) and np.isnan(det).all()
    t = ed.deform_grid_jacobian(torch.zeros((2, 3, 3)), (1, 9), dtype=np.float32)
    assert torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == (1, 9) and bool(torch.isnan(t).all())

    t = ed.deform_grid_jacobian(torch.zeros((2, 3, 3)), (1, 9), dtype=torch.float32)      # a torch dtype names it too
    assert t.dtype == torch.float32
    assert ed.deform_grid_jacobian(D2, (1, 9), dtype=torch.float64).dtype == np.float64

    r = ed.deform_grid_jacobian_gradient(np.ones((1, 9), dtype=np.float32), D2.astype(np.float32), (1, 9), rotate=10.0)
    assert isinstance(r, ed.JacobianGradient)
    assert r.displacement.shape == D2.shape and r.displacement.dtype == np.float32 and not r.displacement.any()
    assert r.inverse_map.shape == (2, 3) and not r.inverse_map.any()
    assert r.rotate == 0.0 and r.zoom is None and not np.asarray(r.affine).any()
    rb = ed.deform_grid_jacobian_gradient_batch(np.ones((3, 8, 1)), np.zeros((3, 2, 3, 3), dtype=np.int16), (8, 1))
    assert rb.displacement.shape == (3, 2, 3, 3) and rb.displacement.dtype == np.float64 and not rb.displacement.any()
    assert rb.inverse_map.shape == (2, 3) and not rb.inverse_map.any()
