"""
Analytic float64 reference of the gradients of deform_grid_inverse with respect to the control-point displacement
and to the inverse map.  TEST INFRASTRUCTURE ONLY: NumPy / SciPy and oracle/dgrad_reference.py, no code shared with
the kernels.

For L = sum_{p, step} dZ[p, step] Z[p, step], Z[p] = S_Y(q(p)), r(q(p)) = p:

    g(p)  = dL/dq at q(p): the spatial derivative of the spline interpolant of Y through the boundary map
            (dgrad_reference._voxel_gradient on Y at q), a(p) the same sum with every tap term's absolute value
    J(p)  = dr/dq at q(p): K[:, :n] + sum_j P[h, j] d beta(q, j) / dq_l, the cubic weight derivatives
            (-z^2/2, x(1.5x - 2), -z(1.5z - 2), x^2/2) times (ncp_l - 1) / (I_l - 1)
    u(p)  = -J^-T g                                   s(p) = |J^-1|^T a
    dP    = sum_p u_h(p) beta(q(p), j)                dD = (order-3 mirror grid prefilter)^T dP
    dK    = sum_p u(p) [q(p), 1]^T
    S_D, S_K: the same contractions with s for u, |filter^T| for the filter and |q| for q (the absolute-value scales
    of dgrad_reference.Result)

The solved positions q and their mask come from the caller (deform_points on the voxel lattice of X in the GPU tests,
a NumPy Newton in the CPU test): a voxel that is not solved contributes nothing.
"""
import collections
import itertools

import numpy as np

from oracle import dgrad_reference as dref
from oracle import ed_oracle as orc

CROP2 = (slice(2, 11), slice(3, 15))
# the geometries tests/test_inverse.py asserts mild (every voxel solved, det J > 0.4), with its _grid / _image seeds
CASES = {
    "1d-affine": dict(I=(40,), ncp=(5,), sigma=2.0, seed=0, affine=np.array([[1.1, -1.5]])),
    "2d-crop-mild": dict(I=(13, 17), ncp=(4, 5), sigma=0.8, seed=91, crop=CROP2),
    "3d-mild": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=0.25, seed=88),
    # more than 7680 grid values: the global-memory routes of the solve and of the cells
    "2d-global-grid": dict(I=(70, 70), ncp=(62, 62), sigma=0.08, seed=1),
    "2d-rz": dict(I=(13, 17), ncp=(3, 3), sigma=0.6, seed=5, crop=CROP2, rotate=20, zoom=1.3),
}
MIN_DET = {"1d-affine": 0.71, "2d-crop-mild": 0.68, "3d-mild": 0.59, "2d-global-grid": 0.57, "2d-rz": 0.40}


def case(name):
    """(I, O, D, geometry keywords, Y in [0, 1] of shape O, dZ standard normal of shape I), float64"""
    c = dict(CASES[name])
    I, ncp, sigma, seed = c.pop("I"), c.pop("ncp"), c.pop("sigma"), c.pop("seed")
    D = np.random.default_rng(seed).standard_normal((len(I),) + tuple(ncp)) * sigma
    crop = c.get("crop")
    O = tuple(I) if crop is None else tuple((s.stop or i) - (s.start or 0) for s, i in zip(crop, I))
    Y = np.random.default_rng(7 + len(I)).uniform(0.0, 1.0, size=O)
    dZ = np.random.default_rng(1000 + seed).standard_normal(I)
    return tuple(I), O, D, c, Y, dZ


def lattice(I):
    return np.stack(np.indices(I), axis=-1).reshape(-1, len(I)).astype(np.float64)


def near_boundary(q, O, order, eps=1e-6):
    """(V,) mask: q_h within eps of a point where the gather is not differentiable or the reference and the kernel
    may pick different windows -- an integer (odd orders: the window changes; order 1: a kink), a half-integer (even
    orders: the window changes), and 0 / O_h - 1 (the boundary map folds, clamps or cuts there)"""
    q = np.asarray(q)
    near = np.zeros(q.shape[0], dtype=bool)
    for h in range(q.shape[1]):
        x = q[:, h] if order & 1 else q[:, h] + 0.5
        near |= np.abs(x - np.round(x)) < eps
        near |= (np.abs(q[:, h]) < eps) | (np.abs(q[:, h] - (O[h] - 1)) < eps)
    return near


Result = collections.namedtuple("Result", ["dD", "dK", "S_D", "S_K"])


def cubic_weight_derivatives(x):
    """d/dx of dgrad_reference.cubic_weights at fraction x in [0, 1); shape x.shape + (4,)"""
    z = 1.0 - x
    return np.stack([-0.5 * z * z, x * (1.5 * x - 2.0), -z * (1.5 * z - 2.0), 0.5 * x * x], axis=-1)


def geometry(dZ, D, order=3, mode="constant", crop=None, axis=None, affine=None, rotate=None, zoom=None):
    """(deformed axes of the one input, I, O, offsets, K) of the call whose X has the shape of dZ"""
    n = D.shape[0]
    axes, out_shapes, offset, _, _, _, K = orc.prepare([dZ], D, order, mode, 0.0, crop, axis, affine, rotate, zoom)
    I = [dZ.shape[d] for d in axes[0]]
    O = [out_shapes[0][d] for d in axes[0]]
    off = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
    K = np.concatenate([np.eye(n), np.zeros((n, 1))], axis=1) if K is None else np.asarray(K, dtype=np.float64)
    return axes[0], I, O, off, K


def jacobian(q, D, I, off, K):
    """J[v, h, l] = d r_h / d q_l at the positions q (V, n): the analytic Jacobian of dgrad_reference.coordinate"""
    n = D.shape[0]
    ncp = D.shape[1:]
    P = dref.prefiltered(D)
    idx, W, dW = [], [], []
    for k in range(n):
        i, w = dref.control_taps(q[:, k], ncp[k], I[k], off[k])
        cp = (ncp[k] - 1) * (q[:, k] + off[k]) / (I[k] - 1)
        idx.append(i)
        W.append(w)
        dW.append(cubic_weight_derivatives(cp - np.floor(cp)) * ((ncp[k] - 1) / (I[k] - 1)))
    J = np.zeros((q.shape[0], n, n))
    for taps in itertools.product(range(4), repeat=n):
        Pt = P[(slice(None),) + tuple(idx[k][:, taps[k]] for k in range(n))].T          # (V, n)
        for l in range(n):
            w = dW[l][:, taps[l]]
            for e in range(n):
                if e != l:
                    w = w * W[e][:, taps[e]]
            J[:, :, l] += Pt * w[:, None]
    return J + K[None, :, :n]


def reference(Y, dZ, D, q, ok, order=3, mode="constant", crop=None, prefilter=True, axis=None, affine=None,
              rotate=None, zoom=None):
    """The gradients of L = <dZ, deform_grid_inverse(Y, D, dZ.shape, ...)> for one input, as a Result.  q (V, n), ok
    (V,): the solved positions of the voxel lattice of X (last deformed axis fastest) and their mask."""
    n = D.shape[0]
    ncp = D.shape[1:]
    axes, I, O, off, K = geometry(dZ, D, order, mode, crop, axis, affine, rotate, zoom)
    ok = np.asarray(ok, dtype=bool)
    q = np.where(ok[:, None], np.asarray(q, dtype=np.float64), 0.0)
    V = q.shape[0]
    g, a, _ = dref._voxel_gradient(Y, np.asarray(dZ, dtype=np.float64), axes, order, mode, q.T, O, prefilter, False)
    g[:, ~ok] = 0.0
    a[:, ~ok] = 0.0
    J = jacobian(q, D, I, off, K)
    J[~ok] = np.eye(n)
    Jinv = np.linalg.inv(J)
    u = -np.einsum("vhl,hv->lv", Jinv, g)                         # u = -J^-T g: u_l = -sum_h Jinv[h, l] g_h
    s = np.einsum("vhl,hv->lv", np.abs(Jinv), a)
    taps = [dref.control_taps(q[:, k], ncp[k], I[k], off[k]) for k in range(n)]
    dP = np.zeros((n,) + tuple(ncp))
    S_P = np.zeros((n,) + tuple(ncp))
    for t in itertools.product(range(4), repeat=n):
        w = np.ones(V)
        for k in range(n):
            w = w * taps[k][1][:, t[k]]
        cell = tuple(taps[k][0][:, t[k]] for k in range(n))
        for h in range(n):
            np.add.at(dP[h], cell, u[h] * w)
            np.add.at(S_P[h], cell, s[h] * np.abs(w))
    dD, S_D = dP, S_P
    for d in range(n):
        M = dref._transposed_filter_matrix(ncp[d])
        dD = dref._along(M, dD, d + 1)
        S_D = dref._along(np.abs(M), S_D, d + 1)
    q1 = np.concatenate([q, np.ones((V, 1))], axis=1)
    return Result(dD, u @ q1, S_D, s @ np.abs(q1))


def newton(p, D, I, off, K, tol=1e-12, max_iter=50):
    """q with dgrad_reference.coordinate(q) = p for the points p (V, n): plain Newton from the affine part's inverse.
    Returns (q, steps taken, largest residual)."""
    n = D.shape[0]
    q = (p - off - K[:, n]) @ np.linalg.inv(K[:, :n]).T
    for step in range(max_iter + 1):
        r = dref.coordinate(q, D, I, off, K) - p
        res = float(np.abs(r).max())
        if res <= tol or step == max_iter:
            return q, step, res
        q = q - np.linalg.solve(jacobian(q, D, I, off, K), r[:, :, None])[:, :, 0]
