"""
CPU tests of the affine gradient (deform_grid_affine_gradient, edhip_deform_transform_gradient): the argument
checks raise before anything touches a device, the float64 torch restatement of the inverse map equals the NumPy
algebra the forward uses and its chain rule agrees with central differences, and the C entry points answer fake
descriptors with the expected status codes -- no GPU needed, nothing is launched.
"""
import ctypes
import os

import numpy as np
import pytest

import elasticdeform_amd as ed
from elasticdeform_amd import _host, _lib

torch = pytest.importorskip("torch")
from elasticdeform_amd import _affine_grad  # noqa: E402


def _disp(shape=(2, 3, 3)):
    return np.zeros(shape)


def test_wrong_dy_shape_raises_before_launch():
    X = np.zeros((10, 12), np.float32)
    with pytest.raises(ValueError, match="dY does not match"):
        ed.deform_grid_affine_gradient(X, np.zeros((10, 11), np.float32), _disp())
    with pytest.raises(ValueError, match="dY does not match"):
        ed.deform_grid_affine_gradient(X, np.zeros((4, 5), np.float32), _disp(), crop=(slice(0, 4), slice(0, 6)))
    with pytest.raises(ValueError, match="dY does not match"):
        ed.deform_grid_affine_gradient_batch(X[None], np.zeros((1, 10, 11), np.float32), _disp()[None])


def test_affine_shape_rotate_zoom_checks():
    X = np.zeros((10, 12), np.float32)
    with pytest.raises(AssertionError, match="Affine matrix should have shape"):
        ed.deform_grid_affine_gradient(X, X, _disp(), affine=np.eye(2))
    X3 = np.zeros((6, 7, 8), np.float32)
    with pytest.raises(AssertionError, match="Affine matrix should have shape"):
        ed.deform_grid_affine_gradient(X3, X3, _disp((3, 3, 3, 3)), affine=np.eye(3))
    with pytest.raises(AssertionError, match="only implemented for 2D"):
        ed.deform_grid_affine_gradient(X3, X3, _disp((3, 3, 3, 3)), rotate=10.0)
    with pytest.raises(AssertionError, match="only implemented for 2D"):
        ed.deform_grid_affine_gradient(X3, X3, _disp((3, 3, 3, 3)), zoom=1.1)
    with pytest.raises(ValueError, match="zoom=0"):
        ed.deform_grid_affine_gradient(X, X, _disp(), zoom=0)
    with pytest.raises(ValueError, match="zoom=0"):
        ed.deform_grid_affine_gradient_batch(X[None], X[None], _disp()[None], zoom=0.0)


@pytest.mark.parametrize("dtype", ["int32", "uint8", "bool", "float16", "int16"])
def test_integer_and_16bit_volumes_refused(dtype):
    X = np.zeros((10, 12), dtype)
    dY = np.zeros((10, 12), np.float32)
    with pytest.raises(RuntimeError, match="data type not supported"):
        ed.deform_grid_affine_gradient(X, dY, _disp())
    with pytest.raises(RuntimeError, match="data type not supported"):
        ed.deform_grid_affine_gradient(dY, X, _disp())
    with pytest.raises(RuntimeError, match="data type not supported"):
        ed.deform_grid_affine_gradient_batch(X[None], dY[None], _disp()[None])


def _cases():
    rng = np.random.default_rng(2024)
    for t in range(120):
        n = (2, 3, 1, 4)[t % 4]
        A = np.concatenate([np.eye(n) + 0.25 * rng.standard_normal((n, n)), 6 * rng.standard_normal((n, 1))], 1)
        if t % 9 == 0:
            A = None
        elif n == 2 and t % 7 == 0:
            A = np.vstack([A, [0.0, 0.0, 1.0]])              # the homogeneous 3 x 3
        shape = [int(v) for v in rng.integers(4, 300, n)]
        rot = zoom = None
        if n == 2:
            rot = float(rng.uniform(-50, 50)) if t % 3 else None
            zoom = float(rng.uniform(0.6, 1.6)) if t % 5 else None
            if t % 11 == 0:
                rot = 0.0
        yield A, rot, zoom, n, shape


def _numpy_k(A, rot, zoom, n, shape):
    k = _host.compose_rotation_zoom(rot, zoom, _host.inverse_of_affine(A, n), shape)
    return np.concatenate([np.eye(n), np.zeros((n, 1))], 1) if k is None else k


def _t(v):
    return None if v is None else torch.tensor(v, dtype=torch.float64)


def test_torch_restatement_equals_numpy_inverse_map():
    for A, rot, zoom, n, shape in _cases():
        want = _numpy_k(A, rot, zoom, n, shape)
        got = _affine_grad.inverse_map(_t(A), _t(rot), _t(zoom), n, shape).numpy()
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 4e-16 * np.abs(want).max(), (A, rot, zoom, shape)


def test_chain_rule_against_central_differences():
    rng = np.random.default_rng(7)
    for A, rot, zoom, n, shape in _cases():
        G = rng.standard_normal((n, n + 1))
        J, ashape = _affine_grad.jacobian(A, rot, zoom, n, shape)
        theta = J.T @ G.reshape(-1)
        Aref = np.concatenate([np.eye(n), np.zeros((n, 1))], 1) if A is None else np.array(A, dtype=np.float64)
        params = [("affine", idx) for idx in np.ndindex(*Aref.shape)]
        params += [("rotate", None)] if rot is not None else []
        params += [("zoom", None)] if zoom is not None else []
        assert J.shape == (n * (n + 1), len(params)) and tuple(ashape) == Aref.shape
        for p, (what, idx) in enumerate(params):
            if what == "affine" and Aref.shape[0] == n + 1 and idx[0] == n:
                assert theta[p] == 0.0          # the homogeneous row does not enter the map
                continue
            h = 1e-6
            vals = []
            for sgn in (1, -1):
                a, r, z = Aref.copy(), rot, zoom
                if what == "affine":
                    a[idx] += sgn * h
                elif what == "rotate":
                    r = rot + sgn * h
                else:
                    z = zoom + sgn * h
                vals.append(float(np.sum(G * _numpy_k(a if (A is not None or what == "affine") else None, r, z,
                                                      n, shape))))
            fd = (vals[0] - vals[1]) / (2 * h)
            scale = max(1.0, float(np.abs(G).sum() * max(1.0, np.abs(_numpy_k(A, rot, zoom, n, shape)).max())))
            assert abs(theta[p] - fd) <= 1e-7 * scale, (what, idx, theta[p], fd)


# ---- the C entry points on fake descriptors (no device memory is touched) ---------------------------------

pytestmark_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                                    reason="libedhip.so not built (run __graft_entry__.build())")


def _desc(shape, dtype="float32", ptr=0x1000):
    a = np.empty(shape, dtype=dtype)
    return _lib.describe(ptr, a.dtype.name, a.shape, a.strides)


def _status(ddisp, dinv, x=None, disp=None):
    x = x if x is not None else _desc((8, 9))
    disp = disp if disp is not None else _desc((2, 3, 3), "float64")
    a = _lib.DeformArgs(1, [(0, 1)], [3], [4], [0.0], None, None)
    buf = ctypes.create_string_buffer(256)
    L = _lib.load()
    st = L.edhip_deform_transform_gradient(1, (_lib.EdhipArray * 1)(x), ctypes.byref(disp), a.off,
                                           (_lib.EdhipArray * 1)(x), a.naxis, a.axis, a.orders, a.modes, a.cvals,
                                           a.aff, None if ddisp is None else ctypes.byref(ddisp),
                                           None if dinv is None else ctypes.byref(dinv), 0, None, buf, 256)
    return st, buf.value.decode()


@pytestmark_lib
def test_c_entry_validation_codes():
    dd = _desc((2, 3, 3), "float64")
    st, msg = _status(None, None)
    assert st == 1 and "neither" in msg
    assert _status(None, _desc((2, 2), "float64"))[0] == 1          # shape
    assert _status(None, _desc((3, 3), "float64"))[0] == 1          # shape (the homogeneous form is refused here)
    assert _status(None, _desc((2, 3, 1), "float64"))[0] == 1       # ndim
    assert _status(dd, _desc((2, 3), "float32"))[0] == 2            # dtype
    assert _status(None, _desc((2, 3), "float32"))[0] == 2
    assert _status(_desc((2, 3, 4), "float64"), _desc((2, 3), "float64"))[0] == 1   # ddisplacement shape
    st, msg = _status(None, _desc((2, 3), "float64"), x=_desc((8, 9), "int32"))
    assert st == 2 and msg == "data type not supported"


@pytestmark_lib
def test_c_batch_entry_validation_codes():
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)
    x, d, dd = _desc((8, 9)), _desc((2, 3, 3), "float64"), _desc((2, 3, 3), "float64")
    ax = (ctypes.c_int32 * 2)(0, 1)

    def call(nbatch, ddisp, dinv, flags=0, xin=x):
        return L.edhip_deform_transform_gradient_batch_strided(
            nbatch, ctypes.byref(xin), 288, ctypes.byref(d), 144, None, ctypes.byref(x), 288, 2, ax, 3, 3, 0.0, None,
            None if ddisp is None else ctypes.byref(ddisp), 144, None if dinv is None else ctypes.byref(dinv), 48,
            flags, None, buf, 256)

    assert call(2, None, None) == 1
    assert call(-1, dd, None) == 1
    for flags in (0, _lib.FLAG_RAW_DISPLACEMENT):
        assert call(2, None, _desc((2, 4), "float64"), flags) == 1
        assert call(2, None, _desc((2, 3), "float32"), flags) == 2
        assert call(2, dd, _desc((2, 3), "float64"), flags, xin=_desc((8, 9), "int32")) == 2
    # the displacement-only entry point keeps its contract
    assert L.edhip_deform_displacement_gradient_batch_strided(
        0, None, 0, None, 0, None, None, 0, 2, ax, 3, 3, 0.0, None, None, 0, 0, None, buf, 256) == 0
