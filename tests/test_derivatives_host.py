"""
CPU tests of the host layer of deform_grid_derivatives / deform_grid_derivatives_gradient (and their batch forms): every
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
Q2 = np.zeros((5, 2))


def _forward(D, X_shape, **kw):
    return ed.deform_grid_derivatives(Q2, D, X_shape, **kw)


def _gradient(D, X_shape, **kw):
    return ed.deform_grid_derivatives_gradient(Q2, D, X_shape, d_hessian=np.zeros((5, 2, 2, 2)), **kw)


CALLS = [_forward, _gradient]


def test_the_names_are_exported():
    for name in ("deform_grid_derivatives", "deform_grid_derivatives_batch", "deform_grid_derivatives_gradient",
                 "deform_grid_derivatives_gradient_batch", "MapDerivatives"):
        assert callable(getattr(ed, name))
        assert callable(getattr(etorch, name))
    assert etorch.deform_grid_derivatives is not ed.deform_grid_derivatives          # the autograd wrapper
    assert ed.MapDerivatives._fields == ("coordinates", "jacobian", "hessian")
    assert "edhip_deform_points_derivatives" in _lib.EXPORTS
    assert "edhip_deform_points_derivatives_gradient" in _lib.EXPORTS
    assert "deform_grid_derivatives" in ed.__doc__


def test_x_shape_is_required():
    for fn in (ed.deform_grid_derivatives, ed.deform_grid_derivatives_batch, etorch.deform_grid_derivatives,
               ed.deform_grid_derivatives_gradient, ed.deform_grid_derivatives_gradient_batch):
        with pytest.raises(ValueError, match="X_shape"):
            fn(Q2, D2, None)


def test_more_than_three_axes():
    D4 = np.zeros((4, 3, 3, 3, 3))
    Q4 = np.zeros((5, 4))
    with pytest.raises(RuntimeError, match="1 to 3 deformed axes"):
        ed.deform_grid_derivatives(Q4, D4, (5, 6, 7, 8))
    with pytest.raises(RuntimeError, match="1 to 3 deformed axes"):
        ed.deform_grid_derivatives_batch(Q4[None], D4[None], (5, 6, 7, 8), hessian=False)
    with pytest.raises(RuntimeError, match="1 to 3 deformed axes"):
        ed.deform_grid_derivatives_gradient(Q4, D4, (5, 6, 7, 8), d_coordinates=Q4)


def test_the_positions():
    with pytest.raises(ValueError, match="last dimension of the points"):
        ed.deform_grid_derivatives(np.zeros((5, 3)), D2, (8, 9))
    with pytest.raises(ValueError, match=r"\(batch, N, naxis\)"):
        ed.deform_grid_derivatives_batch(Q2, D2[None], (8, 9))
    for dtype in (np.float16, np.complex64):
        with pytest.raises(RuntimeError, match="data type not supported"):
            ed.deform_grid_derivatives(Q2.astype(dtype), D2, (8, 9))
    with pytest.raises(RuntimeError, match="data type not supported"):
        ed.deform_grid_derivatives(torch.zeros((5, 2), dtype=torch.bfloat16), D2, (8, 9))


def test_the_cotangents():
    with pytest.raises(ValueError, match="At least one of d_coordinates, d_jacobian and d_hessian"):
        ed.deform_grid_derivatives_gradient(Q2, D2, (8, 9))
    with pytest.raises(ValueError, match="At least one of"):
        ed.deform_grid_derivatives_gradient_batch(Q2[None], D2[None], (8, 9))
    with pytest.raises(ValueError, match="shape of the points"):
        ed.deform_grid_derivatives_gradient(Q2, D2, (8, 9), d_coordinates=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="d_jacobian should have shape"):
        ed.deform_grid_derivatives_gradient(Q2, D2, (8, 9), d_jacobian=np.zeros((5, 2)))
    with pytest.raises(ValueError, match="d_hessian should have shape"):
        ed.deform_grid_derivatives_gradient(Q2, D2, (8, 9), d_hessian=np.zeros((5, 2, 2)))
    with pytest.raises(ValueError, match="d_hessian should have shape"):                # the batch axis
        ed.deform_grid_derivatives_gradient_batch(Q2[None], D2[None], (8, 9), d_hessian=np.zeros((5, 2, 2, 2)))
    for name, shape in (("d_coordinates", (5, 2)), ("d_jacobian", (5, 2, 2)), ("d_hessian", (5, 2, 2, 2))):
        with pytest.raises(RuntimeError, match="data type not supported"):
            ed.deform_grid_derivatives_gradient(Q2, D2, (8, 9), **{name: np.zeros(shape, dtype=np.float16)})


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


def test_zoom_zero_has_no_gradient():
    with pytest.raises(ValueError, match="zoom=0"):
        ed.deform_grid_derivatives_gradient(Q2, D2, (8, 9), d_coordinates=Q2, zoom=0)


def test_length_one_axis_is_decided_on_the_host():
    """a deformed axis of length 1: NaN r, J and H, zero gradients -- no device, no library"""
    out = ed.deform_grid_derivatives(Q2.astype(np.float32), D2, (1, 9))
    assert isinstance(out, ed.MapDerivatives)
    assert out.coordinates.shape == (5, 2) and out.coordinates.dtype == np.float32 and np.isnan(out.coordinates).all()
    assert out.jacobian.shape == (5, 2, 2) and out.jacobian.dtype == np.float64 and np.isnan(out.jacobian).all()
    assert out.hessian.shape == (5, 2, 2, 2) and out.hessian.dtype == np.float64 and np.isnan(out.hessian).all()
    out = ed.deform_grid_derivatives_batch(torch.zeros((3, 5, 2)), torch.zeros((3, 2, 3, 3)), (8, 1), hessian=False)
    assert torch.is_tensor(out.jacobian) and tuple(out.jacobian.shape) == (3, 5, 2, 2) and out.hessian is None
    r = ed.deform_grid_derivatives_gradient(Q2, D2.astype(np.float32), (1, 9), d_jacobian=np.ones((5, 2, 2)), rotate=10.0)
    assert isinstance(r, ed.PointsGradient)
    assert r.points.shape == (5, 2) and not r.points.any()
    assert r.displacement.shape == D2.shape and r.displacement.dtype == np.float32 and not r.displacement.any()
    assert r.inverse_map.shape == (2, 3) and not r.inverse_map.any() and r.rotate == 0.0
