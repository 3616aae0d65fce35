"""
NumPy reference of deform_grid_sample and its gradients.  TEST INFRASTRUCTURE ONLY: built from oracle.dgrad_reference
(coordinate, map_coordinate, value_taps, mirror) and the oracle's spline_filter1d / spline_filter1d_grad; no code
shared with the kernels.

For source coordinates r (N, n) on the array X whose deformed axes `axes` have the extents I:

    m_h, m'_h   = map_coordinate(r_h, I_h, mode) and its slope
    taps, w, w' = value_taps(m_h, order, I_h): the (order + 1) mirror-folded taps of the window, their B-spline weights
                  and the weights' derivatives (order 0, which value_taps does not have: ONE tap at floor(m + 1/2)
                  with weight 1 and derivative 0)
    V[i, s]     = sum_k C[k, s] prod_h w_h(k_h)          C: X prefiltered along its deformed axes (order > 1)
    g_h(i)      = sum_s dV[i, s] m'_h sum_k C[k, s] w'_h(k_h) prod_{e != h} w_e(k_e)
    A[i, j]     = the sum of prod_h w_h over the taps that fold onto cell j       (V = A C per step)

A point is `dead` -- V = cval, an empty row of A, g = 0 -- where r is not finite, and where the mode is 'constant' and
r lies outside [0, I_h - 1] on some axis.  S_V and S_g are the same contractions with every term replaced by its
absolute value: the scales of the rounding error.
"""
import collections
import itertools

import numpy as np

from oracle import ed_oracle as orc
from oracle.dgrad_reference import coordinate, map_coordinate, mirror, value_taps  # noqa: F401

Sample = collections.namedtuple("Sample", ["V", "inside", "dead", "g", "S_V", "S_g", "A", "T", "C", "m"])


def coefficients(X, axes, order, prefilter=True):
    """X as the forward reads it: filtered along its deformed axes for order > 1, each pass stored in X's own dtype
    (as deform_grid prepares its input), then taken as float64"""
    C = np.ascontiguousarray(X)
    if prefilter and order > 1:
        for d in axes:
            C = orc.spline_filter1d(C, order, d)
    return C.astype(np.float64)


def taps(r, I, order, mode):
    """per axis (folded indices, weights, weight derivatives times the slope), each (N, order + 1); m (n, N); the
    outside mask (n, N)"""
    idx, w, dw, ms, outs = [], [], [], [], []
    for h in range(r.shape[1]):
        m, slope, out = map_coordinate(r[:, h], I[h], mode)
        if order == 0:
            i = mirror(np.floor(np.where(out & (mode == "constant"), 0.0, m) + 0.5).astype(np.int64)[:, None], I[h])
            wv, dwv = np.ones(i.shape), np.zeros(i.shape)
        else:
            i, wv, dwv = value_taps(np.where(out & (mode == "constant"), 0.0, m), order, I[h])
        idx.append(i)
        w.append(wv)
        dw.append(dwv * slope[:, None])
        ms.append(m)
        outs.append(out)
    return idx, w, dw, np.array(ms), np.array(outs)


def reference(X, r, axes, order, mode, cval=0.0, prefilter=True, dV=None, matrix=False):
    """The Sample of X (any dtype; taken as float64) at the coordinates r (N, n): V (N, steps) float64 before the
    store rule, inside (N,), dead (N,), and with dV (N, steps) also g and S_g (N, n); with `matrix` the dense A
    (N, prod I) and T, the number of taps of point i that land on cell j.  The steps are X's non-deformed axes,
    flattened in their order."""
    r = np.asarray(r, dtype=np.float64)
    N, n = r.shape
    axes = list(axes)
    I = [X.shape[d] for d in axes]
    C = np.moveaxis(coefficients(X, axes, order, prefilter), axes, range(n))
    C = C.reshape(tuple(I) + (-1,))
    finite = np.isfinite(r).all(1)
    rr = np.where(finite[:, None], r, 0.0)
    idx, w, dw, m, outs = taps(rr, I, order, mode)
    inside = finite & ~outs.any(0)
    dead = ~finite | (outs.any(0) if mode == "constant" else False)
    V = np.zeros((N, C.shape[-1]))
    S_V = np.zeros((N, C.shape[-1]))
    val = np.zeros((n, N, C.shape[-1]))
    mag = np.zeros((n, N, C.shape[-1]))
    A = np.zeros((N, int(np.prod(I)))) if matrix else None
    T = np.zeros((N, int(np.prod(I)))) if matrix else None       # how many taps of point i land on cell j
    for t in itertools.product(range(order + 1), repeat=n):
        cell = tuple(idx[e][:, t[e]] for e in range(n))
        Ck = C[cell]
        p = np.ones(N)
        for e in range(n):
            p = p * w[e][:, t[e]]
        V += Ck * p[:, None]
        S_V += np.abs(Ck) * np.abs(p)[:, None]
        if matrix:
            np.add.at(A, (np.arange(N), np.ravel_multi_index(cell, I)), p)
            np.add.at(T, (np.arange(N), np.ravel_multi_index(cell, I)), 1.0)
        if dV is not None:
            for h in range(n):
                p = dw[h][:, t[h]]
                for e in range(n):
                    if e != h:
                        p = p * w[e][:, t[e]]
                val[h] += Ck * p[:, None]
                mag[h] += np.abs(Ck) * np.abs(p)[:, None]
    V[dead] = cval
    S_V[dead] = 0.0
    if matrix:
        A[dead] = 0.0
        T[dead] = 0.0
    g = S_g = None
    if dV is not None:
        y = np.asarray(dV, dtype=np.float64).reshape(N, -1)
        g = (y[None] * val).sum(-1).T
        S_g = (np.abs(y)[None] * mag).sum(-1).T
        g[dead] = 0.0
        S_g[dead] = 0.0
    return Sample(V, inside, dead, g, S_V, S_g, A, T, C, m)


def store(V, dtype):
    """the reference's store rule (deform.c:292-306): round half away from zero and clamp for integers"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return V.astype(dtype)
    if dtype.kind == "b":
        return V != 0
    info = np.iinfo(dtype)
    t = np.where(V > 0, V + 0.5, V - 0.5) if info.min < 0 else np.where(V > 0, V + 0.5, 0.0)
    return np.trunc(np.clip(t, info.min, info.max)).astype(dtype)


def boundary_distance(r, I, order, mode, integer_output=False):
    """(N,) the distance of r to the nearest decision boundary of the gather: half-integers of the mapped coordinate
    (order 0, and integer outputs), 0 and I_k - 1 ('constant' and `inside`: always counted), the fold points ('wrap')"""
    r = np.asarray(r, dtype=np.float64)
    d = np.full(r.shape[0], np.inf)
    for h in range(r.shape[1]):
        x = r[:, h]
        d = np.minimum(d, np.minimum(np.abs(x), np.abs(x - (I[h] - 1))))
        if mode == "wrap":
            p = I[h] - 1
            d = np.minimum(d, np.abs(x / p - np.round(x / p)) * p)
        if order == 0 or integer_output:
            m = map_coordinate(x, I[h], "nearest" if mode == "constant" else mode)[0]
            d = np.minimum(d, np.abs(m - np.floor(m) - 0.5))
    return d


def adjoint(A, dV, axes, shape, order, prefilter=True):
    """A^T dV in long double, then the transposed prefilter: dX of `shape` (float64).  dV: (N, steps)."""
    n = len(axes)
    I = [shape[d] for d in axes]
    steps = [s for d, s in enumerate(shape) if d not in axes]
    acc = (A.astype(np.longdouble).T @ np.asarray(dV, dtype=np.longdouble)).astype(np.float64)
    acc = acc.reshape(tuple(I) + tuple(steps))
    rest = [d for d in range(len(shape)) if d not in axes]
    acc = np.moveaxis(acc, list(range(len(shape))), list(axes) + rest)
    acc = np.ascontiguousarray(acc)
    if prefilter and order > 1:
        for d in axes:
            acc = orc.spline_filter1d_grad(np.ascontiguousarray(acc), np.zeros(acc.shape), d, order)
    return acc
