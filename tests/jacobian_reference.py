"""
Analytic float64 reference of deform_grid_jacobian and of its gradients.  TEST INFRASTRUCTURE ONLY: NumPy and
oracle/dgrad_reference.py (prefiltered, mirror, cubic_weights / control_taps, _transposed_filter_matrix, _along), no
code shared with the kernels.

On the voxel lattice of the output (O_0 x ... x O_{n-1}, crop-local o) everything is separable:

    B_k(o, j)   = sum of the cubic weights of the 4 taps of o on axis k whose mirror fold is j
    dB_k(o, j)  = the same sum of the weight derivatives [-z^2/2, (3x^2 - 4x)/2, (-3x^2 + 2x + 1)/2, x^2/2] s_k,
                  z = 1 - x, s_k = (ncp_k - 1) / (I_k - 1)
    J[h, l](o)  = K[h, l] + P[h] contracted with dB_l along axis l and B_k along every other axis
    det(o)      = det J(o);   C(o) = the cofactor matrix of J(o)  (d det / dJ = C, also at det = 0)
    dP[h, j]    = sum_o g(o) sum_l C[h, l](o) d_l beta_j(o)     (dB_l^T along axis l, B_k^T along the others)
    dD          = (order-3 mirror grid prefilter)^T dP along every grid axis
    dK[h, l<n]  = sum_o g(o) C[h, l](o),   dK[h, n] = 0
    A_D, A_K    = the same contractions with every term replaced by its absolute value (A_D through the entrywise
                  absolute value of the transposed filter): the scales of the rounding error
    B           = prod_h (sum_l |K[h, l]| + 1.5 max|P[h]| sum_l s_l): bounds every product in det (sum_t |w'_t| <= 1.5)

affine / rotate / zoom follow from dK by the derivative of the reference's own matrix algebra (ed_oracle._inverse_affine),
written out here: K = (T(c) Z(1/zoom) R(-rotate) T(-c) [A^-1, -A^-1 t; 0 1])[:n].
"""
import collections

import numpy as np

from oracle import dgrad_reference as dref
from oracle import ed_oracle as orc

Result = collections.namedtuple("Result", ["J", "det", "dP", "dD", "dK", "A_D", "A_K", "B", "K", "O", "S", "C"])


def weight_derivatives(x):
    """d/dx of the 4 cubic B-spline weights at fraction x in [0, 1); shape x.shape + (4,)"""
    z = 1.0 - x
    return np.stack([-z * z / 2.0, (3.0 * x * x - 4.0 * x) / 2.0, (-3.0 * x * x + 2.0 * x + 1.0) / 2.0, x * x / 2.0],
                    axis=-1)


def axis_matrices(out_len, ncp, in_len, off):
    """(B_k, dB_k), each (out_len, ncp): folded taps added; dB_k carries s_k"""
    o = np.arange(out_len, dtype=np.float64)
    idx, w = dref.control_taps(o, ncp, in_len, float(off))
    cp = (ncp - 1) * (o + float(off)) / (in_len - 1)
    dw = weight_derivatives(cp - np.floor(cp)) * ((ncp - 1) / (in_len - 1))
    B = np.zeros((out_len, ncp))
    dB = np.zeros((out_len, ncp))
    rows = np.arange(out_len)[:, None]
    np.add.at(B, (rows, idx), w)
    np.add.at(dB, (rows, idx), dw)
    return B, dB


def geometry(X_shape, D, crop=None, axis=None, affine=None, rotate=None, zoom=None):
    """(I, O, offsets, K) of deform_grid on an array of X_shape"""
    n = D.shape[0]
    X = np.zeros(tuple(X_shape), dtype=np.uint8)
    axes, out_shapes, offset, _, _, _, K = orc.prepare([X], D, 3, "constant", 0.0, crop, axis, affine, rotate, zoom)
    I = [X.shape[d] for d in axes[0]]
    O = [out_shapes[0][d] for d in axes[0]]
    off = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
    K = np.concatenate([np.eye(n), np.zeros((n, 1))], axis=1) if K is None else np.asarray(K, dtype=np.float64)
    return I, O, off, K


def cofactors(J):
    """C[..., h, l] with d det / dJ[..., h, l] = C[..., h, l]; J (..., n, n), n = 1, 2, 3"""
    n = J.shape[-1]
    C = np.empty_like(J)
    if n == 1:
        C[..., 0, 0] = 1.0
    elif n == 2:
        C[..., 0, 0], C[..., 0, 1] = J[..., 1, 1], -J[..., 1, 0]
        C[..., 1, 0], C[..., 1, 1] = -J[..., 0, 1], J[..., 0, 0]
    else:
        for h in range(3):
            C[..., h, :] = np.cross(J[..., (h + 1) % 3, :], J[..., (h + 2) % 3, :])
    return C


def determinant(J):
    n = J.shape[-1]
    if n == 1:
        return J[..., 0, 0].copy()
    return (J[..., 0, :] * cofactors(J)[..., 0, :]).sum(-1)


def displacement_part(P, mats, n):
    """S[o, h, l] = P[h] contracted with dB_l along axis l and B_k along the others: (O_0, ..., n, n)"""
    cols = []
    for l in range(n):
        a = P
        for k in range(n):
            a = dref._along(mats[k][1] if k == l else mats[k][0], a, k + 1)      # (n, O_0 .. O_{n-1})
        cols.append(np.moveaxis(a, 0, -1))
    return np.stack(cols, axis=-1)


def reference(D, X_shape, g=None, crop=None, axis=None, affine=None, rotate=None, zoom=None):
    """det J on the lattice and, with the cotangent g (the shape of det), the gradients of L = sum g det"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    ncp = D.shape[1:]
    I, O, off, K = geometry(X_shape, D, crop, axis, affine, rotate, zoom)
    P = dref.prefiltered(D)
    mats = [axis_matrices(O[k], ncp[k], I[k], off[k]) for k in range(n)]
    S = displacement_part(P, mats, n)
    J = S + K[:, :n]
    det = determinant(J)
    s = np.array([(ncp[k] - 1) / (I[k] - 1) for k in range(n)])
    bound = float(np.prod([np.abs(K[h, :n]).sum() + 1.5 * np.abs(P[h]).max() * s.sum() for h in range(n)]))
    if g is None:
        return Result(J, det, None, None, None, None, None, bound, K, tuple(O), S, None)
    g = np.asarray(g, dtype=np.float64)
    C = cofactors(J)
    G = g[..., None, None] * C                                   # (O..., h, l)
    dP = np.zeros((n,) + tuple(ncp))
    A_P = np.zeros((n,) + tuple(ncp))
    for l in range(n):
        a = np.moveaxis(G[..., l], -1, 0)                        # (h, O_0 .. O_{n-1})
        b = np.abs(a)
        for k in range(n):
            M = mats[k][1] if k == l else mats[k][0]
            a = dref._along(M.T, a, k + 1)
            b = dref._along(np.abs(M).T, b, k + 1)
        dP += a
        A_P += b
    dD, A_D = dP, A_P
    for k in range(n):
        M = dref._transposed_filter_matrix(ncp[k])
        dD = dref._along(M, dD, k + 1)
        A_D = dref._along(np.abs(M), A_D, k + 1)
    lat = tuple(range(n))
    dK = np.zeros((n, n + 1))
    A_K = np.zeros((n, n + 1))
    dK[:, :n] = G.sum(axis=lat)
    A_K[:, :n] = np.abs(G).sum(axis=lat)
    return Result(J, det, dP, dD, dK, A_D, A_K, bound, K, tuple(O), S, C)


def loss(S, K, g):
    """L = sum g det(K[:, :n] + S): the loss as a function of the inverse map alone"""
    n = S.shape[-1]
    return float((g * determinant(S + np.asarray(K)[:, :n])).sum())


def parameter_gradients(dK, O, affine=None, rotate=None, zoom=None):
    """(d affine in its own shape or None, d rotate per degree or None, d zoom or None) from dK (n, n + 1)"""
    n = dK.shape[0]
    spin = rotate is not None or zoom is not None
    m = np.eye(n + 1)
    base = np.eye(n + 1)
    if affine is not None:
        A = np.asarray(affine, dtype=np.float64)[:n, :]
        Ainv = np.linalg.inv(A[:, :n])
        base[:n, :n] = Ainv
        base[:n, n] = -Ainv @ A[:, n]
    d_rot = d_zoom = None
    if spin:
        c = np.array(O, dtype=np.float64) / 2 - 0.5
        th = np.radians(-float(rotate or 0))
        z = 1.0 / float(zoom or 1)
        Tm = np.array([[1, 0, -c[0]], [0, 1, -c[1]], [0, 0, 1.0]])
        Tp = np.array([[1, 0, c[0]], [0, 1, c[1]], [0, 0, 1.0]])
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
        dR = np.array([[-np.sin(th), -np.cos(th), 0], [np.cos(th), -np.sin(th), 0], [0, 0, 0.0]])
        Z = np.diag([z, z, 1.0])
        m = Tp @ Z @ R @ Tm
        if rotate is not None:
            d_rot = float((dK * ((Tp @ Z @ dR @ Tm) @ base)[:n] * (-np.pi / 180.0)).sum())
        if zoom is not None:
            d_zoom = float((dK * ((Tp @ np.diag([1.0, 1.0, 0.0]) @ R @ Tm) @ base)[:n]).sum() * (-z * z))
    d_aff = None
    if affine is not None:
        shape = np.asarray(affine).shape
        d_aff = np.zeros(shape)
        for i in range(n):
            for j in range(n + 1):
                dbase = np.zeros((n + 1, n + 1))
                if j < n:
                    E = np.zeros((n, n))
                    E[i, j] = 1.0
                    dinv = -Ainv @ E @ Ainv
                    dbase[:n, :n] = dinv
                    dbase[:n, n] = -dinv @ A[:, n]
                else:
                    dbase[:n, n] = -Ainv[:, i]
                d_aff[i, j] = float((dK * (m @ dbase)[:n]).sum())
    return d_aff, d_rot, d_zoom
