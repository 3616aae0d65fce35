"""
Analytic float64 reference of the gradients of deform_grid with respect to the control-point displacement and to
the inverse map.  TEST INFRASTRUCTURE ONLY (NumPy, SciPy and the ed_oracle helpers; no code shared with the kernels).

Written from the formulas in the header of elasticdeform_amd/csrc/deform_dgrad.hip and the semantics of ed_device.h:

    u_d(o)      = (ncp_d - 1) (o_d + off_d) / (len_d - 1)              control coordinate of output index o on axis d
    b_d(o, j)   = sum of the cubic weights of the 4 taps floor(u_d) - 1 + t whose mirror fold is j
    beta(o, j)  = prod_d b_d(o_d, j_d)
    c_h(o)      = (K [o; 1])_h + off_h + sum_j P[h, j] beta(o, j)      P: the order-3 mirror prefilter of D
    m_h, m'_h   = map_coordinate(c_h, len_h, mode) and its slope
    g_h(o)      = sum_i sum_step dY_i[o, step] m'_h sum_k C_i[k, step] w'(m_h, k_h) prod_{e != h} w(m_e, k_e)
    dP[h, j]    = sum_o g_h(o) beta(o, j)          dD = (prefilter)^T dP along every grid axis
    dK[h, l]    = sum_o g_h(o) o_l                 dK[h, n] = sum_o g_h(o)

The value weights w and their derivatives w' are scipy.interpolate.BSpline.basis_element of the centred B-spline of
the order and its .derivative(), at the (order + 1) taps of the window (window start floor(m) - order // 2 for odd
orders, floor(m + 1/2) - order // 2 for even ones); a tap outside the axis is mirror-folded whatever the mode.  A
voxel with an axis outside under 'constant' contributes nothing; the slope is 0 where 'nearest' clamps.

`coordinate` (the coordinate map at real positions), `prefiltered`, `mirror` and `cubic_weights` are also what
tests/test_points.py checks the point kernels against.
"""
import collections
import itertools

import numpy as np
from scipy.interpolate import BSpline

from oracle import ed_oracle as orc

MODES = ("constant", "nearest", "mirror", "reflect", "wrap")
EXTENDED = np.longdouble


# ---- the control grid: prefilter, folded taps, cubic weights ------------------------------------------------------

def prefiltered(D):
    """the order-3 mirror prefilter of the grid along every grid axis, float64 (scipy.ndimage)"""
    import scipy.ndimage
    P = np.array(D, dtype=np.float64)
    for d in range(1, P.ndim):
        P = scipy.ndimage.spline_filter1d(P, order=3, axis=d, mode="mirror")
    return P


def mirror(i, n):
    """mirror fold of integer tap indices onto [0, n)"""
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    j = np.mod(i, period)
    return np.where(j >= n, period - j, j)


def cubic_weights(x):
    """the 4 cubic B-spline weights at fraction x in [0, 1), last weight = 1 - the others; shape x.shape + (4,)"""
    z = 1.0 - x
    w0 = z * z * z / 6.0
    w1 = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], axis=-1)


def control_taps(q, ncp, in_len, off, dtype=np.float64):
    """(folded control indices (N, 4), cubic weights (N, 4) in `dtype`) of the positions q (N,) on one axis"""
    cp = (ncp - 1) * (q + off) / (in_len - 1)
    fl = np.floor(cp)
    return (mirror(fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], ncp),
            cubic_weights((cp - fl).astype(dtype)))


def control_matrix(out_len, ncp, in_len, off, dtype=np.float64):
    """b_d(o, j) for o = 0 .. out_len - 1: (out_len, ncp), taps that fold onto one j added"""
    idx, w = control_taps(np.arange(out_len, dtype=np.float64), ncp, in_len, float(off), dtype)
    B = np.zeros((out_len, ncp), dtype=dtype)
    np.add.at(B, (np.arange(out_len)[:, None], idx), w)
    return B


def coordinate(q, D, I, off=None, K=None):
    """c(q) for real positions q of shape (N, n): K [q; 1] + off + the displacement, vectorised over the points"""
    q = np.asarray(q, dtype=np.float64)
    n = D.shape[0]
    ncp = D.shape[1:]
    P = prefiltered(D)
    off = np.zeros(n) if off is None else np.asarray(off, dtype=np.float64)
    K = np.concatenate([np.eye(n), np.zeros((n, 1))], axis=1) if K is None else np.asarray(K, dtype=np.float64)
    idx, W = [], []
    for k in range(n):
        i, w = control_taps(q[:, k], ncp[k], I[k], off[k])
        idx.append(i)
        W.append(w)
    delta = np.zeros((q.shape[0], n))
    for taps in itertools.product(range(4), repeat=n):
        w = np.ones(q.shape[0])
        for k in range(n):
            w = w * W[k][:, taps[k]]
        delta += P[(slice(None),) + tuple(idx[k][:, taps[k]] for k in range(n))].T * w[:, None]
    return q @ K[:, :n].T + K[:, n] + off + delta


# ---- the boundary map and the value weights -------------------------------------------------------------------------

def map_coordinate(c, length, mode):
    """(m, slope, outside) of the coordinates c on an axis of `length` samples: the legacy boundary maps of
    ed_device.h (map_coordinate, map_coordinate_slope); outside = c < 0 or c > length - 1"""
    c = np.asarray(c)
    m = c.copy()
    s = np.ones_like(c)
    lo, hi = c < 0, c > length - 1
    out = lo | hi
    L = c.dtype.type(length)
    if mode == "constant":
        m[out], s[out] = -1.0, 0.0
    elif mode == "nearest":
        m[lo], m[hi], s[out] = 0.0, L - 1, 0.0
    elif length <= 1:
        m[out], s[out] = 0.0, 0.0
    elif mode == "mirror":
        p = 2 * L - 2
        x = c[lo]
        x = p * np.trunc(-x / p) + x
        up = x <= 1 - L
        m[lo], s[lo] = np.where(up, x + p, -x), np.where(up, 1.0, -1.0)
        x = c[hi]
        x = x - p * np.trunc(x / p)
        down = x >= L
        m[hi], s[hi] = np.where(down, p - x, x), np.where(down, -1.0, 1.0)
    elif mode == "reflect":
        # legacy semantics: -c - 1 just below 0 (c + 2 len below -len), the coordinate left alone in (len - 1, len)
        p = 2 * L
        x = c[lo]
        x = np.where(x < -p, p * np.trunc(-x / p) + x, x)
        up = x < -L
        m[lo], s[lo] = np.where(up, x + p, -x - 1), np.where(up, 1.0, -1.0)
        x = c[hi]
        x = x - p * np.trunc(x / p)
        down = x >= L
        m[hi], s[hi] = np.where(down, p - x - 1, x), np.where(down, -1.0, 1.0)
    elif mode == "wrap":
        p = L - 1
        m[lo] = c[lo] + p * (np.trunc(-c[lo] / p) + 1)
        m[hi] = c[hi] - p * np.trunc(c[hi] / p)
    else:
        raise ValueError(mode)
    return m, s, out


_BASIS = {}


def _basis(order):
    if order not in _BASIS:
        b = BSpline.basis_element(np.arange(order + 2) - (order + 1) / 2.0, extrapolate=False)
        _BASIS[order] = (b, b.derivative())
    return _BASIS[order]


def value_taps(m, order, length):
    """(folded sample indices, weights, weight derivatives), each (N, order + 1), of the window around m (N,)"""
    start = (np.floor(m) if order & 1 else np.floor(m + 0.5)).astype(np.int64) - order // 2
    taps = start[:, None] + np.arange(order + 1)[None, :]
    x = (m[:, None] - taps).astype(np.float64)
    b, db = _basis(order)
    return mirror(taps, length), np.nan_to_num(b(x)), np.nan_to_num(db(x))


# ---- the gradients --------------------------------------------------------------------------------------------------

Result = collections.namedtuple("Result", ["dD", "dK", "S_D", "S_K", "outside", "cmax", "dmax"])


def _transposed_filter_matrix(ncp):
    """the transposed order-3 grid filter of one axis of ncp points as a matrix (the filter of the identity)"""
    eye = np.eye(ncp)
    return orc.spline_filter1d_grad(eye, np.zeros_like(eye), 0, 3)


def _along(M, a, axis):
    """M applied along `axis` of a"""
    return np.moveaxis(np.tensordot(M, a, axes=([1], [axis])), 0, axis)


def _voxel_gradient(X, dY, axes, order, mode, c, in_len, prefilter, f32):
    """(g, |g| at tap level, outside mask (n, V)) of one input: g[h, v] for the V voxels whose coordinates are c (n, V)"""
    n, V = c.shape
    if prefilter and order > 1:
        for d in axes:
            X = orc.spline_filter1d(X, order, d)
    T = np.float32 if f32 else np.float64
    C = np.moveaxis(X, axes, range(n))
    C = C.reshape(C.shape[:n] + (-1,)).astype(T)
    y = np.moveaxis(dY, axes, range(n)).astype(np.float64).reshape(V, -1)
    idx, w, dw, outs = [], [], [], []
    for h in range(n):
        m, slope, out = map_coordinate(c[h], in_len[h], mode)
        i, wv, dwv = value_taps(m, order, in_len[h])
        idx.append(i)
        w.append(wv.astype(T))
        dw.append((dwv * slope[:, None]).astype(T))
        outs.append(out)
    outs = np.array(outs)
    val = np.zeros((n, V, C.shape[-1]), dtype=T)
    mag = np.zeros((n, V, C.shape[-1]))
    for taps in itertools.product(range(order + 1), repeat=n):
        Ck = C[tuple(idx[e][:, taps[e]] for e in range(n))]
        for h in range(n):
            p = dw[h][:, taps[h]]
            for e in range(n):
                if e != h:
                    p = p * w[e][:, taps[e]]
            val[h] += Ck * p[:, None]
            if not f32:
                mag[h] += np.abs(Ck) * np.abs(p)[:, None]
    g = (y[None] * val.astype(np.float64)).sum(-1)
    a = (np.abs(y)[None] * mag).sum(-1)
    if mode == "constant":
        dead = outs.any(0)
        g[:, dead] = 0.0
        a[:, dead] = 0.0
    return g, a, outs


def reference(X, dY, D, order=3, mode="constant", crop=None, prefilter=True, axis=None, affine=None, rotate=None,
              zoom=None, f32=False):
    """The gradients of L = sum_i <dY_i, deform_grid(X, D, ...)_i> for one call, as a Result:

    dD       with respect to the raw displacement (deform_grid_displacement_gradient), float64
    dK       with respect to the inverse map K (AffineGradient.inverse_map), (n, n + 1)
    S_D, S_K the same two contractions with every term replaced by its absolute value at tap level (S_D through the
             entrywise absolute value of the transposed grid filter): the scales of the rounding error
    outside  the fraction of (voxel, axis) coordinates outside [0, len - 1]
    cmax, dmax  the largest |coordinate| and the largest sum_j |P[h, j]| beta(o, j) (the conditioning of the coordinates)

    f32: the tap sums in float32 (C, w and dw * slope cast to float32, their products and sum in float32), everything
    after them in float64 -- what the kernels do for float32 volumes.  S_D and S_K are then zero.
    """
    Xs = X if isinstance(X, list) else [X]
    dYs = dY if isinstance(dY, list) else [dY]
    n = D.shape[0]
    ncp = D.shape[1:]
    axes, out_shapes, offset, orders, modes, _, K = orc.prepare(Xs, D, order, mode, 0.0, crop, axis, affine, rotate,
                                                                zoom)
    names = {v: k for k, v in orc._MODE_CODES.items()}
    in_len = [Xs[0].shape[d] for d in axes[0]]
    O = [out_shapes[0][d] for d in axes[0]]
    off = np.zeros(n) if offset is None else offset.astype(np.float64)
    K = np.concatenate([np.eye(n), np.zeros((n, 1))], axis=1) if K is None else np.asarray(K, dtype=np.float64)

    P = orc._prefilter_displacement(D).astype(np.float64)       # (in the grid's dtype after every axis, as the forward)
    B = [control_matrix(O[d], ncp[d], in_len[d], off[d]) for d in range(n)]
    # the coordinates in extended precision (EXTENDED: a 64-bit significand), so that their rounding is the kernel's
    # alone; the control coordinate u_d itself is the same float64 expression as the kernel's
    Bx = [control_matrix(O[d], ncp[d], in_len[d], off[d], EXTENDED) for d in range(n)]
    delta, dabs = P.astype(EXTENDED), np.abs(P)
    for d in range(n):
        delta = _along(Bx[d], delta, d + 1)                      # (n, O_0 .. O_{n-1})
        dabs = _along(np.abs(B[d]), dabs, d + 1)
    o = np.indices(O).reshape(n, -1).astype(np.float64)
    c = K[:, :n].astype(EXTENDED) @ o.astype(EXTENDED) + K[:, n:] + off[:, None] + delta.reshape(n, -1)

    g = np.zeros(c.shape)
    a = np.zeros(c.shape)
    outside = []
    for i in range(len(Xs)):
        gi, ai, out = _voxel_gradient(Xs[i], dYs[i], axes[i], int(orders[i]), names[int(modes[i])], c, in_len,
                                      prefilter, f32)
        g += gi
        a += ai
        outside.append(out.mean())

    dP, S_P = g.reshape([n] + O), a.reshape([n] + O)
    for d in range(n):
        dP = _along(B[d].T, dP, d + 1)
        S_P = _along(np.abs(B[d]).T, S_P, d + 1)
    dD, S_D = dP, S_P
    for d in range(n):
        dD = orc.spline_filter1d_grad(np.ascontiguousarray(dD), np.zeros(dD.shape), d + 1, 3)
        S_D = _along(np.abs(_transposed_filter_matrix(ncp[d])), S_D, d + 1)
    o1 = np.concatenate([o, np.ones((1, o.shape[1]))])
    return Result(dD, g @ o1.T, S_D, a @ np.abs(o1).T, float(np.mean(outside)), float(np.abs(c).max()),
                  float(dabs.max()))
