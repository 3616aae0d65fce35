"""
CPU tests of the host side of deform_grid_sample and its gradients: every refusal happens before the library or a
device is touched (no GPU is needed: a call that got past its checks would fail with "needs a ROCm GPU"), the names are
exported, and the degenerate geometry is answered on the host.
"""
import importlib

import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _lib

X = np.zeros((6, 7))
Q = np.zeros((5, 2))
D = np.zeros((2, 3, 3))
DV = np.zeros((5,))

NAMES = ["deform_grid_sample", "deform_grid_sample_gradient", "deform_grid_sample_coordinate_gradient",
         "deform_grid_sample_points_gradient"]


def test_the_names_are_exported():
    for name in NAMES:
        assert callable(getattr(ed, name)) and callable(getattr(ed, name + "_batch"))
    assert "edhip_deform_sample" in _lib.EXPORTS and "edhip_deform_sample_gradient" in _lib.EXPORTS
    assert "deform_grid_sample" in ed.__doc__


def test_the_torch_module_exports_the_names():
    etorch = pytest.importorskip("elasticdeform_amd.torch")
    for name in NAMES:
        assert callable(getattr(etorch, name)) and callable(getattr(etorch, name + "_batch"))
    assert etorch.deform_grid_sample is not ed.deform_grid_sample           # the autograd wrapper
    assert etorch.deform_grid_sample_batch is ed.deform_grid_sample_batch   # re-exported without autograd
    import elasticdeform.torch as alias
    assert alias.deform_grid_sample is etorch.deform_grid_sample


REFUSALS = [
    ("positions-last-axis", lambda: ed.deform_grid_sample(X, np.zeros((5, 3)), D), ValueError,
     "last dimension of the points"),
    ("positions-scalar-rows", lambda: ed.deform_grid_sample(X, np.zeros((5,)), D), ValueError,
     "last dimension of the points"),
    ("positions-half", lambda: ed.deform_grid_sample(X, Q.astype(np.float16), D), RuntimeError,
     "data type not supported"),
    ("half-input", lambda: ed.deform_grid_sample(X.astype(np.float16), Q, D), RuntimeError, "data type not supported"),
    ("complex-input", lambda: ed.deform_grid_sample(X.astype(np.complex64), Q, D), RuntimeError,
     "data type not supported"),
    ("order-6", lambda: ed.deform_grid_sample(X, Q, D, order=6), AssertionError, "order"),
    ("mode", lambda: ed.deform_grid_sample(X, Q, D, mode="clamp"), Exception, ""),
    ("four-axes", lambda: ed.deform_grid_sample(np.zeros((3,) * 4), np.zeros((5, 4)), np.zeros((4,) + (3,) * 4)),
     RuntimeError, "1 to 3 deformed axes"),
    ("displacement-shape", lambda: ed.deform_grid_sample(X, Q, np.zeros((3, 3, 3))), Exception, ""),
    ("dV-shape", lambda: ed.deform_grid_sample_gradient(np.zeros((4,)), Q, D, X.shape), ValueError,
     "dV does not match"),
    ("dV-shape-channels", lambda: ed.deform_grid_sample_gradient(np.zeros((5, 2)), Q, D, (2, 6, 7), axis=(1, 2)),
     ValueError, "dV does not match"),
    ("dV-integer", lambda: ed.deform_grid_sample_gradient(np.zeros((5,), np.int32), Q, D, X.shape), RuntimeError,
     "data type not supported"),
    ("X_shape-missing", lambda: ed.deform_grid_sample_gradient(DV, Q, D, None), ValueError, "X_shape is required"),
    ("coordinate-dV-shape", lambda: ed.deform_grid_sample_coordinate_gradient(X, np.zeros((6,)), Q, D), ValueError,
     "dV does not match"),
    ("coordinate-integer-X", lambda: ed.deform_grid_sample_coordinate_gradient(X.astype(np.int16), DV, Q, D),
     RuntimeError, "data type not supported"),
    ("points-integer-X", lambda: ed.deform_grid_sample_points_gradient(X.astype(np.uint8), DV, Q, D), RuntimeError,
     "data type not supported"),
    ("points-zoom-0", lambda: ed.deform_grid_sample_points_gradient(X, DV, Q, D, zoom=0), ValueError, "zoom=0"),
    ("batch-positions-rank", lambda: ed.deform_grid_sample_batch(np.zeros((2, 6, 7)), np.zeros((5, 2)),
                                                                np.zeros((2, 2, 3, 3))), ValueError,
     "(batch, N, naxis)"),
    ("batch-positions-count", lambda: ed.deform_grid_sample_batch(np.zeros((2, 6, 7)), np.zeros((3, 5, 2)),
                                                                 np.zeros((2, 2, 3, 3))), ValueError,
     "one set of points per sample"),
    ("list-lengths", lambda: ed.deform_grid_sample_coordinate_gradient([X, X], [DV], Q, D), ValueError,
     "one array per input"),
]


@pytest.mark.parametrize("name,call,exc,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_happen_before_any_library_call(name, call, exc, text, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "deform_sample", boom)
    monkeypatch.setattr(_lib, "deform_sample_gradient", boom)
    monkeypatch.setattr(_lib, "deform_points_gradient", boom)
    monkeypatch.setattr(importlib.import_module("elasticdeform_amd.deform_grid"), "_device_for", boom)
    with pytest.raises(exc) as info:
        call()
    assert "the library was called" not in str(info.value)
    assert text in str(info.value)


def test_a_deformed_axis_of_length_one_is_answered_on_the_host():
    X1 = np.ones((6, 1))
    V, inside = ed.deform_grid_sample(X1, Q, D, cval=2.0, return_inside=True)
    np.testing.assert_array_equal(V, np.full(5, 2.0))
    assert inside.shape == (5,) and not inside.any()
    assert not ed.deform_grid_sample_gradient(DV, Q, D, X1.shape).any()
    g = ed.deform_grid_sample_coordinate_gradient(X1, DV, Q, D)
    assert g.shape == Q.shape and g.dtype == np.float64 and not g.any()


def test_autograd_wrapper_without_gradients_is_the_plain_call():
    etorch = pytest.importorskip("elasticdeform_amd.torch")
    with pytest.raises(ValueError, match="last dimension of the points"):
        etorch.deform_grid_sample(X, np.zeros((5, 3)), D)
