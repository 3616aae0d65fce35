"""
Analytic float64 reference of deform_grid_derivatives and of its adjoint.  TEST INFRASTRUCTURE ONLY: NumPy,
oracle/dgrad_reference.py (prefiltered, control_taps' conventions, mirror, cubic_weights, _transposed_filter_matrix,
_along) and the geometry / weight_derivatives of tests/jacobian_reference.py; no code shared with the kernels.

For a crop-local real position q, cp_k = s_k (q_k + off_k), s_k = (ncp_k - 1) / (I_k - 1), x_k = cp_k - floor(cp_k),
the four taps of axis k start at floor(cp_k) - 1 and are folded by the mirror map.  With w^(a) the a-th derivative of the
cubic weights in the knot cell of floor(cp),

    w    = dref.cubic_weights(x)                       w'   = jacobian_reference.weight_derivatives(x)
    w''  = [1 - x, 3x - 2, 1 - 3x, x]                  w''' = [-1, 3, -3, 1]

and a multi-index a, S_h[a](q) = sum_taps P[h, m(t)] prod_k s_k^{a_k} w_k^(a_k)[t_k]:

    r_h = sum_l K[h, l] q_l + K[h, n] + off_h + S_h[0]       J[h, l] = K[h, l] + S_h[e_l]
    H[h, l, m] = S_h[e_l + e_m]                              T[h, l, m, p] = S_h[e_l + e_m + e_p]

and for the cotangents u = dL/dr, A = dL/dJ, G = dL/dH (any absent), W[a] the weight product of one tap:

    dP[h, j]   = sum_i sum_{taps folding to j} u[i,h] W[0] + sum_l A[i,h,l] W[e_l] + sum_lm G[i,h,l,m] W[e_l + e_m]
    dD         = (order-3 mirror grid prefilter)^T dP along every grid axis
    dK[h, l<n] = sum_i u[i,h] q_i[l] + A[i,h,l]              dK[h, n] = sum_i u[i,h]
    dq_i[p]    = sum_h u[i,h] J[h,p] + sum_hl A[i,h,l] H[h,l,p] + sum_hlm G[i,h,l,m] T[h,l,m,p]

A_H, A_P, A_D, A_K, A_q are the same contractions with every term replaced by its absolute value (A_D through the entrywise
absolute value of the transposed filter): the scales of the rounding error.  A position that is not finite, or whose
control coordinate reaches 4e15, is not "sane": NaN in r, J, H, T, a zero dq row, no contribution to any sum.
"""
import collections
import itertools

import numpy as np

from oracle import dgrad_reference as dref

import jacobian_reference as jref

MAX_COORDINATE = 4e15

Result = collections.namedtuple("Result", ["r", "J", "H", "T", "A_H", "dP", "dD", "dK", "dq", "A_P", "A_D", "A_K",
                                           "A_q", "K", "sane"])


def weight_jet(x):
    """the cubic weights at fraction x in [0, 1) and their three derivatives: (4 orders,) + x.shape + (4 taps,)"""
    x = np.asarray(x, dtype=np.float64)
    w2 = np.stack([1.0 - x, 3.0 * x - 2.0, 1.0 - 3.0 * x, x], axis=-1)
    w3 = np.broadcast_to(np.array([-1.0, 3.0, -3.0, 1.0]), x.shape + (4,))
    return np.stack([dref.cubic_weights(x), jref.weight_derivatives(x), w2, w3], axis=0)


def axis_taps(q, ncp, in_len, off):
    """(folded control indices (N, 4), W (4 orders, N, 4 taps) with W[a] = s^a w^(a), sane (N,)) of one axis"""
    s = (ncp - 1) / (in_len - 1)
    cp = (ncp - 1) * (q + off) / (in_len - 1)
    sane = np.abs(cp) < MAX_COORDINATE                      # (False for NaN)
    cp = np.where(sane, cp, 0.0)
    fl = np.floor(cp)
    idx = dref.mirror(fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], ncp)
    W = weight_jet(cp - fl) * (s ** np.arange(4))[:, None, None]
    return idx, W, sane


def _unit(n, *axes):
    a = [0] * n
    for k in axes:
        a[k] += 1
    return tuple(a)


def reference(D, X_shape, q, u=None, A=None, G=None, crop=None, axis=None, affine=None, rotate=None, zoom=None,
              inverse_map=None):
    """r, J, H, T at the positions q (N, n) and, with cotangents, the gradients of L = sum u r + A J + G H.
    `inverse_map` replaces the K that affine / rotate / zoom give."""
    D = np.asarray(D, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = D.shape[0]
    N = q.shape[0]
    ncp = D.shape[1:]
    I, _, off, K = jref.geometry(X_shape, D, crop, axis, affine, rotate, zoom)
    if inverse_map is not None:
        K = np.asarray(inverse_map, dtype=np.float64)
    P = dref.prefiltered(D)
    idx, W, sane = [], [], np.ones(N, dtype=bool)
    for k in range(n):
        i, w, ok = axis_taps(q[:, k], ncp[k], I[k], off[k])
        idx.append(i)
        W.append(w)
        sane &= ok
    qs = np.where(sane[:, None], q, 0.0)
    orders = [a for a in itertools.product(range(4), repeat=n) if sum(a) <= 3]
    S = {a: np.zeros((n, N)) for a in orders}
    Sabs = {a: np.zeros((n, N)) for a in orders}
    cot = u is not None or A is not None or G is not None
    zero = lambda *tail: np.zeros((N,) + tail)              # noqa: E731
    u = zero(n) if u is None else np.where(sane[:, None], np.asarray(u, dtype=np.float64), 0.0)
    A = zero(n, n) if A is None else np.where(sane[:, None, None], np.asarray(A, dtype=np.float64), 0.0)
    G = zero(n, n, n) if G is None else np.where(sane[:, None, None, None], np.asarray(G, dtype=np.float64), 0.0)
    dP = np.zeros((n,) + tuple(ncp))
    A_P = np.zeros((n,) + tuple(ncp))
    for taps in itertools.product(range(4), repeat=n):
        cell = tuple(idx[k][:, taps[k]] for k in range(n))
        Pt = P[(slice(None),) + cell]                        # (n, N)
        prod = {}
        for a in orders:
            w = np.ones(N)
            for k in range(n):
                w = w * W[k][a[k]][:, taps[k]]
            prod[a] = w
            S[a] += Pt * w
            Sabs[a] += np.abs(Pt) * np.abs(w)
        if cot:
            c = u.T * prod[_unit(n)]                         # (n, N)
            cabs = np.abs(u.T) * np.abs(prod[_unit(n)])
            for l in range(n):
                c = c + A[:, :, l].T * prod[_unit(n, l)]
                cabs = cabs + np.abs(A[:, :, l].T) * np.abs(prod[_unit(n, l)])
                for m in range(n):
                    c = c + G[:, :, l, m].T * prod[_unit(n, l, m)]
                    cabs = cabs + np.abs(G[:, :, l, m].T) * np.abs(prod[_unit(n, l, m)])
            for h in range(n):
                np.add.at(dP[h], cell, c[h])
                np.add.at(A_P[h], cell, cabs[h])
    r = qs @ K[:, :n].T + K[:, n] + off + S[_unit(n)].T
    J = np.empty((N, n, n))
    H = np.empty((N, n, n, n))
    T = np.empty((N, n, n, n, n))
    A_H = np.empty((N, n, n, n))
    A_J = np.empty((N, n, n))
    A_T = np.empty((N, n, n, n, n))
    for l in range(n):
        J[:, :, l] = K[:, l] + S[_unit(n, l)].T
        A_J[:, :, l] = np.abs(K[:, l]) + Sabs[_unit(n, l)].T
        for m in range(n):
            H[:, :, l, m] = S[_unit(n, l, m)].T
            A_H[:, :, l, m] = Sabs[_unit(n, l, m)].T
            for p in range(n):
                T[:, :, l, m, p] = S[_unit(n, l, m, p)].T
                A_T[:, :, l, m, p] = Sabs[_unit(n, l, m, p)].T
    dD = dK = dq = A_D = A_K = A_q = None
    if cot:
        dD, A_D = dP, A_P
        for k in range(n):
            M = dref._transposed_filter_matrix(ncp[k])
            dD = dref._along(M, dD, k + 1)
            A_D = dref._along(np.abs(M), A_D, k + 1)
        dK = np.zeros((n, n + 1))
        A_K = np.zeros((n, n + 1))
        dK[:, :n] = np.einsum("ih,il->hl", u, qs) + A.sum(0)
        dK[:, n] = u.sum(0)
        A_K[:, :n] = np.einsum("ih,il->hl", np.abs(u), np.abs(qs)) + np.abs(A).sum(0)
        A_K[:, n] = np.abs(u).sum(0)
        dq = (np.einsum("ih,ihp->ip", u, J) + np.einsum("ihl,ihlp->ip", A, H) + np.einsum("ihlm,ihlmp->ip", G, T))
        A_q = (np.einsum("ih,ihp->ip", np.abs(u), A_J) + np.einsum("ihl,ihlp->ip", np.abs(A), A_H)
               + np.einsum("ihlm,ihlmp->ip", np.abs(G), A_T))
        dq[~sane] = 0.0
    for a in (r, J, H, T):
        a[~sane] = np.nan
    return Result(r, J, H, T, A_H, dP, dD, dK, dq, A_P, A_D, A_K, A_q, K, sane)


def loss(res, u=None, A=None, G=None):
    """L = sum u r + A J + G H over the sane points"""
    L = 0.0
    for c, v in ((u, res.r), (A, res.J), (G, res.H)):
        if c is not None:
            L += float((np.asarray(c, dtype=np.float64)[res.sane] * v[res.sane]).sum())
    return L
