"""
GPU tests of the gradients through the coordinate map and its inverse: elasticdeform_amd.deform_grid_coordinates_gradient,
deform_points_gradient, their batch forms, the autograd wrappers of elasticdeform_amd.torch
(edhip_deform_points_gradient).

Expected values come from a NumPy restatement that shares nothing with the kernel (the formulas of tests/test_points.py,
restated here): dP_want is numpy.add.at of u[:, h] prod(w) at the mirrored tap indices, dD_want = M^T dP_want with M
built column by column from scipy.ndimage.spline_filter1d(order=3, mode='mirror'), dK_want = u^T [q, 1].

Tolerances: an fp64 or 2^-61-resolved sum errs below 1e-13 of sum_i |u[i, h]|, a wrong tap, fold or weight at 1e-3 of
it: 1e-10 sum|u| is asserted.  Per-point rows are compared with central differences of the restatement at the bound of
the existing Jacobian test, 1e-6 max(1, |J|max) |u|max; the inverse direction at 1 / 0.2 (det J > 0.2) times these.
"""
import itertools

import numpy as np
import pytest

from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402


# ---- the NumPy restatement -----------------------------------------------------------------------------------

def _prefiltered(D):
    import scipy.ndimage
    P = np.array(D, dtype=np.float64)
    for d in range(1, P.ndim):
        P = scipy.ndimage.spline_filter1d(P, order=3, axis=d, mode="mirror")
    return P


def _mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    j = np.mod(i, period)
    return np.where(j >= n, period - j, j)


def _weights(x):
    z = 1.0 - x
    w0 = z * z * z / 6.0
    w1 = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], axis=-1)


def _taps(q, ncp, I, off):
    idx, W = [], []
    for k in range(len(ncp)):
        cp = (ncp[k] - 1) * (q[:, k] + off[k]) / (I[k] - 1)
        fl = np.floor(cp)
        W.append(_weights(cp - fl))
        idx.append(_mirror(fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], ncp[k]))
    return idx, W


def restate(q, D, I, off=None, K=None):
    """r(q) for q of shape (N, n)"""
    q = np.asarray(q, dtype=np.float64)
    n = D.shape[0]
    ncp = D.shape[1:]
    P = _prefiltered(D)
    off = np.zeros(n) if off is None else np.asarray(off, dtype=np.float64)
    K = np.concatenate([np.eye(n), np.zeros((n, 1))], axis=1) if K is None else np.asarray(K, dtype=np.float64)
    idx, W = _taps(q, ncp, I, off)
    delta = np.zeros((q.shape[0], n))
    for taps in itertools.product(range(4), repeat=n):
        w = np.ones(q.shape[0])
        for k in range(n):
            w = w * W[k][:, taps[k]]
        delta += P[(slice(None),) + tuple(idx[k][:, taps[k]] for k in range(n))].T * w[:, None]
    return q @ K[:, :n].T + K[:, n] + off + delta


def restate_jacobian(q, D, I, off=None, K=None, h=1e-4):
    n = D.shape[0]
    J = np.zeros((q.shape[0], n, n))
    for l in range(n):
        e = np.zeros(n)
        e[l] = h
        J[:, :, l] = (restate(q + e, D, I, off, K) - restate(q - e, D, I, off, K)) / (2 * h)
    return J


def adjoint(q, u, D, I, off=None):
    """(dD_want, dK_want) of L = sum_i <u_i, r(q_i)>"""
    import scipy.ndimage
    q = np.asarray(q, dtype=np.float64)
    n = D.shape[0]
    ncp = D.shape[1:]
    off = np.zeros(n) if off is None else np.asarray(off, dtype=np.float64)
    idx, W = _taps(q, ncp, I, off)
    dP = np.zeros((n,) + tuple(ncp))
    for taps in itertools.product(range(4), repeat=n):
        w = np.ones(q.shape[0])
        for k in range(n):
            w = w * W[k][:, taps[k]]
        where = tuple(idx[k][:, taps[k]] for k in range(n))
        for h in range(n):
            np.add.at(dP[h], where, u[:, h] * w)
    dD = dP
    for k in range(n):
        M = np.stack([scipy.ndimage.spline_filter1d(e, order=3, mode="mirror") for e in np.eye(ncp[k])], axis=1)
        dD = np.moveaxis(np.tensordot(M.T, np.moveaxis(dD, k + 1, 0), axes=1), 0, k + 1)     # M^T along grid axis k
    dK = u.T @ np.concatenate([q, np.ones((q.shape[0], 1))], axis=1)
    return dD, dK


def _offsets(crop, n):
    return np.zeros(n) if crop is None else np.array([float(s.start or 0) for s in crop])


def _out_shape(I, crop):
    return tuple(I) if crop is None else tuple((s.stop or i) - (s.start or 0) for s, i in zip(crop, I))


def _K(I, crop=None, affine=None, rotate=None, zoom=None):
    if affine is None and rotate is None and zoom is None:
        return None
    return orc._inverse_affine(affine, rotate, zoom, len(I), list(_out_shape(I, crop)))


def _grid(seed, n, ncp, sigma):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(ncp)) * sigma


def _random_positions(seed, O, count):
    rng = np.random.default_rng(seed)
    O = np.asarray(O, dtype=np.float64)
    return rng.uniform(-O, 2 * O - 1, size=(count, len(O)))


AFFINE2 = np.array([[1.1, 0.15, -1.5], [-0.1, 0.9, 2.0]])
AFFINE3 = np.array([[1.05, 0.1, 0.0, -1.0], [-0.08, 0.95, 0.05, 0.5], [0.02, -0.04, 1.1, 1.5]])

RANDOM = {
    "1d": dict(I=(40,), ncp=(5,), sigma=2.0),
    "2d": dict(I=(13, 17), ncp=(4, 5), sigma=3.0),
    "3d": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5),
    "4d-generic": dict(I=(6, 7, 8, 9), ncp=(3, 3, 3, 3), sigma=0.7),
    "2d-crop": dict(I=(13, 17), ncp=(4, 5), sigma=3.0, crop=(slice(2, 11), slice(3, 15))),
    "3d-crop": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5, crop=(slice(1, 9), slice(0, 14), slice(2, 7))),
    "2d-affine": dict(I=(13, 17), ncp=(4, 5), sigma=3.0, affine=AFFINE2),
    "3d-affine": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5, affine=AFFINE3),
    "2d-rotate-zoom-crop": dict(I=(13, 17), ncp=(4, 5), sigma=3.0, crop=(slice(2, 11), slice(3, 15)), rotate=20.0,
                                zoom=1.3),
    "2d-global-grid": dict(I=(70, 70), ncp=(64, 64), sigma=0.5),   # 2 x 64 x 64 values: cells in global memory
    "1d-short-grid": dict(I=(9,), ncp=(2,), sigma=1.0),            # two control points: the taps fold onto one cell
}

INVERTIBLE = {
    "2d": dict(I=(40, 52), ncp=(5, 5), sigma=2.0, seed=12),
    "2d-crop-affine": dict(I=(40, 52), ncp=(5, 5), sigma=2.0, seed=12, crop=(slice(4, 36), slice(6, 50)),
                           affine=AFFINE2),
    "3d": dict(I=(24, 28, 20), ncp=(4, 4, 4), sigma=0.5, seed=4),
    "3d-crop-affine": dict(I=(24, 28, 20), ncp=(4, 4, 4), sigma=0.5, seed=4,
                           crop=(slice(2, 22), slice(3, 27), slice(0, 18)), affine=AFFINE3),
}


def _case(name):
    c = dict(RANDOM[name])
    I, ncp, sigma = c.pop("I"), c.pop("ncp"), c.pop("sigma")
    return I, _grid(31 + len(name), len(I), ncp, sigma), c


def _contract_case():
    I = (13, 17)
    D = _grid(41, 2, (4, 5), 1.5)
    q = _random_positions(13, I, 700)
    u = np.random.default_rng(14).standard_normal(q.shape)
    return I, D, q, u, dict(crop=(slice(1, 12), slice(2, 16)), affine=AFFINE2)


def _same_bits(a, b):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def _check_sums(got, dD, dK, u, q, factor=1.0):
    n = u.shape[1]
    for h in range(n):
        s = np.abs(u[:, h]).sum()
        err = np.abs(got.displacement[h] - dD[h]).max()
        print("component %d: max |dD err| %.3g, sum|u| %.3g" % (h, err, s))
        assert err <= factor * 1e-10 * s
    bound = factor * 1e-10 * np.abs(u).sum() * max(1.0, np.abs(q).max())
    errk = np.abs(got.inverse_map - dK).max()
    print("max |dK err| %.3g (bound %.3g)" % (errk, bound))
    assert errk <= bound


# ---- 1. forward direction ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(RANDOM))
def test_forward_direction_equals_the_restatement(name):
    I, D, kw = _case(name)
    n = len(I)
    O = _out_shape(I, kw.get("crop"))
    off, K = _offsets(kw.get("crop"), n), _K(I, **kw)
    q = _random_positions(5, O, 600)
    u = np.random.default_rng(6).standard_normal(q.shape)
    got = ed.deform_grid_coordinates_gradient(q, u, D, I, **kw)
    assert isinstance(got, ed.PointsGradient) and isinstance(got.points, np.ndarray)
    assert got.points.shape == q.shape and got.points.dtype == np.float64
    assert got.displacement.shape == D.shape and got.displacement.dtype == D.dtype
    assert got.inverse_map.shape == (n, n + 1) and got.inverse_map.dtype == np.float64
    dD, dK = adjoint(q, u, D, I, off)
    _check_sums(got, dD, dK, u, q)
    J = restate_jacobian(q, D, I, off, K)
    dq = np.einsum("ihl,ih->il", J, u)
    err = np.abs(got.points - dq).max()
    print("%s: max |dq err| %.3g" % (name, err))
    assert err <= 1e-6 * max(1.0, np.abs(J).max()) * np.abs(u).max()


# ---- 2. parameters -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, kw", [
    ("2d", dict(rotate=20.0, zoom=1.3, crop=(slice(2, 11), slice(3, 15)))),
    ("3d", dict(affine=AFFINE3)),
])
def test_parameters_against_central_differences(name, kw):
    I, D, _ = _case(name)
    n = len(I)
    off = _offsets(kw.get("crop"), n)
    q = _random_positions(5, _out_shape(I, kw.get("crop")), 600)
    u = np.random.default_rng(6).standard_normal(q.shape)

    def loss(**params):
        return float((u * restate(q, D, I, off, _K(I, crop=kw.get("crop"), **params))).sum())

    A = kw.get("affine")
    A0 = np.concatenate([np.eye(n), np.zeros((n, 1))], 1) if A is None else np.array(A, dtype=np.float64)
    params = {k: kw.get(k) for k in ("rotate", "zoom")}
    want = []
    for idx in np.ndindex(*A0.shape):
        h = 1e-6 * max(1.0, abs(A0[idx]))
        vals = []
        for s in (1, -1):
            a = A0.copy()
            a[idx] += s * h
            vals.append(loss(affine=a, **params))
        want.append((vals[0] - vals[1]) / (2 * h))
    for pname in ("rotate", "zoom"):
        v = params[pname]
        if v is not None:
            h = 1e-6 * max(1.0, abs(v))
            want.append((loss(affine=A, **dict(params, **{pname: v + h}))
                         - loss(affine=A, **dict(params, **{pname: v - h}))) / (2 * h))
    got = ed.deform_grid_coordinates_gradient(q, u, D, I, **kw)
    have = np.concatenate([got.affine.reshape(-1)] + [np.array([v]) for v in (got.rotate, got.zoom) if v is not None])
    want = np.array(want)
    assert got.affine.shape == A0.shape and have.shape == want.shape
    assert (got.rotate is None) == (kw.get("rotate") is None) and (got.zoom is None) == (kw.get("zoom") is None)
    scale = np.abs(want).max()
    err = np.abs(have - want).max()
    print("%s: max |err| %.3g of %.3g" % (name, err, scale))
    assert scale > 0 and err <= 1e-6 * scale


# ---- 3. inverse direction ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(INVERTIBLE))
def test_inverse_direction_on_invertible_fields(name):
    c = dict(INVERTIBLE[name])
    I, ncp, sigma, seed = c.pop("I"), c.pop("ncp"), c.pop("sigma"), c.pop("seed")
    n = len(I)
    D = np.random.default_rng(seed).standard_normal((n,) + ncp) * sigma
    O = _out_shape(I, c.get("crop"))
    off, K = _offsets(c.get("crop"), n), _K(I, **c)
    rng = np.random.default_rng(9)
    q0 = rng.uniform(0, np.asarray(O, dtype=np.float64) - 1, size=(400, n))
    p = np.concatenate([restate(q0, D, I, off, K), rng.uniform(0, np.asarray(I) - 1.0, size=(100, n))])
    g = rng.standard_normal(p.shape)
    q, ok = ed.deform_points(p, D, I, return_converged=True, **c)
    assert ok.all()
    J = restate_jacobian(q, D, I, off, K)
    u = -np.linalg.solve(np.transpose(J, (0, 2, 1)), g[..., None])[..., 0]
    dD, dK = adjoint(q, u, D, I, off)
    got = ed.deform_points_gradient(p, g, D, I, **c)
    factor = 1e4 / 0.2                                               # 1e-6 (1 / 0.2) in units of 1e-10
    _check_sums(got, dD, dK, u, q, factor)
    err = np.abs(got.points + u).max()
    print("%s: max |dp err| %.3g" % (name, err))
    assert err <= 1e-6 / 0.2 * max(1.0, np.abs(J).max()) * np.abs(u).max()
    # the solved positions handed in: the same bits, nothing is solved again
    again = ed.deform_points_gradient(p, g, D, I, positions=q, **c)
    for a, b in zip(got, again):
        _same_bits(a, b)


# ---- 4. points that contribute nothing -----------------------------------------------------------------------

def test_unsolved_points_change_nothing_but_their_own_row():
    I = (32, 32)
    D = np.random.default_rng(5).standard_normal((2, 5, 5)) * 6.0
    p = np.random.default_rng(10).uniform(0, 31, size=(1500, 2))
    g = np.random.default_rng(11).standard_normal(p.shape)
    q, ok = ed.deform_points(p, D, I, return_converged=True)
    print("solved %d of %d" % (ok.sum(), ok.size))
    assert (~ok).any() and ok.sum() >= ok.size // 2
    full = ed.deform_points_gradient(p, g, D, I)
    part = ed.deform_points_gradient(p[ok], g[ok], D, I)
    _same_bits(full.displacement, part.displacement)
    _same_bits(full.inverse_map, part.inverse_map)
    _same_bits(full.points[ok], part.points)
    assert (full.points[~ok] == 0).all()
    assert np.isfinite(full.displacement).all() and np.abs(full.displacement).max() > 0
    # a non-finite cotangent on an unsolved point is ignored
    g2 = g.copy()
    g2[np.flatnonzero(~ok)[0]] = np.nan
    _same_bits(ed.deform_points_gradient(p, g2, D, I).displacement, full.displacement)


def test_insane_positions_change_nothing_but_their_own_row():
    I, D, kw = _case("2d")
    q = _random_positions(5, I, 600)
    u = np.random.default_rng(6).standard_normal(q.shape)
    clean = ed.deform_grid_coordinates_gradient(q, u, D, I, **kw)
    bad = np.array([[np.nan, 3.0], [2.0, np.inf], [1e300, 1.0], [-np.inf, np.nan]])
    where = np.array([0, 17, 300, 603])
    qm = np.insert(q, where - np.arange(4), bad, axis=0)
    um = np.insert(u, where - np.arange(4), np.array([[1.0, 2.0], [np.nan, 1.0], [3.0, np.inf], [4.0, 5.0]]), axis=0)
    assert np.array_equal(qm[where], bad, equal_nan=True)
    mixed = ed.deform_grid_coordinates_gradient(qm, um, D, I, **kw)
    _same_bits(mixed.displacement, clean.displacement)
    _same_bits(mixed.inverse_map, clean.inverse_map)
    keep = np.ones(len(qm), dtype=bool)
    keep[where] = False
    _same_bits(mixed.points[keep], clean.points)
    assert (mixed.points[where] == 0).all()


# ---- 5. bit contracts ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_repeats_permutations_batches_and_slices_give_the_same_bits(inverse):
    I, D, q, u, kw = _contract_case()
    single = ed.deform_points_gradient if inverse else ed.deform_grid_coordinates_gradient
    batch = ed.deform_points_gradient_batch if inverse else ed.deform_grid_coordinates_gradient_batch
    if inverse:
        q = restate(q, D, I, _offsets(kw["crop"], 2), _K(I, **kw))            # points that have a pre-image
    first = single(q, u, D, I, **kw)
    assert np.isfinite(first.displacement).all() and np.abs(first.displacement).max() > 0
    for a, b in zip(first, single(q, u, D, I, **kw)):                         # a repeat
        _same_bits(a, b)
    perm = np.random.default_rng(15).permutation(len(q))
    for order in (slice(None, None, -1), perm):                               # any order of the points
        other = single(q[order], u[order], D, I, **kw)
        _same_bits(other.displacement, first.displacement)
        _same_bits(other.inverse_map, first.inverse_map)
        _same_bits(other.points, first.points[order])
    _same_bits(single(q[300:437], u[300:437], D, I, **kw).points, first.points[300:437])     # a slice's rows
    # a 3-sample batch against three single calls
    Db = np.stack([D, -0.5 * D, _grid(42, 2, (4, 5), 1.0)])
    qb = np.stack([q, q[::-1], q[perm]])
    ub = np.stack([u, 2.0 * u, u[::-1]])
    gb = batch(qb, ub, Db, I, **kw)
    singles = [single(qb[b], ub[b], Db[b], I, **kw) for b in range(3)]
    assert gb.points.shape == qb.shape and gb.displacement.shape == Db.shape
    for b in range(3):
        _same_bits(gb.points[b], singles[b].points)
        _same_bits(gb.displacement[b], singles[b].displacement)
    _same_bits(gb.inverse_map, singles[0].inverse_map + singles[1].inverse_map + singles[2].inverse_map)
    _same_bits(gb.affine, singles[0].affine + singles[1].affine + singles[2].affine)
    # one NaN cotangent in sample 1: that sample's sums are NaN, the others' unchanged
    un = ub.copy()
    un[1, 123, 0] = np.nan
    gn = batch(qb, un, Db, I, **kw)
    assert np.isnan(gn.displacement[1]).all() and np.isnan(gn.inverse_map).all()
    _same_bits(gn.displacement[0], gb.displacement[0])
    _same_bits(gn.displacement[2], gb.displacement[2])
    one = single(qb[1], un[1], Db[1], I, **kw)
    assert np.isnan(one.displacement).all() and np.isnan(one.inverse_map).all() and np.isnan(one.affine).all()
    keep = np.arange(len(q)) != 123
    _same_bits(one.points[keep], singles[1].points[keep])


# ---- 6. more points than one launch covers ---------------------------------------------------------------------

def test_more_points_than_one_launch_covers():
    I, D = (40,), _grid(43, 1, (5,), 2.0)
    N = 2048 * 256 + 1000
    q = torch.linspace(-5.0, 50.0, N, dtype=torch.float64, device="cuda").reshape(N, 1)
    u = torch.sin(torch.arange(N, dtype=torch.float64, device="cuda")).reshape(N, 1)
    got = ed.deform_grid_coordinates_gradient(q, u, torch.from_numpy(D).cuda(), I)
    assert torch.is_tensor(got.displacement) and got.displacement.is_cuda and got.points.shape == (N, 1)
    un = u.cpu().numpy()
    dD, dK = adjoint(q.cpu().numpy(), un, D, I)
    s = np.abs(un).sum()
    err = np.abs(got.displacement.cpu().numpy() - dD).max()
    print("N = %d: max |dD err| %.3g, sum|u| %.3g" % (N, err, s))
    assert err <= 1e-10 * s
    assert np.abs(got.inverse_map.cpu().numpy() - dK).max() <= 1e-10 * s * 50.0
    tail = ed.deform_grid_coordinates_gradient(q[-1500:], u[-1500:], torch.from_numpy(D).cuda(), I)
    assert torch.equal(got.points[-1500:], tail.points)


# ---- 7. autograd ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_autograd_gives_the_bits_of_the_gradient_functions(inverse):
    I, D, q, u, kw = _contract_case()
    if inverse:
        q = restate(q, D, I, _offsets(kw["crop"], 2), _K(I, **kw))
    fn = etorch.deform_points if inverse else etorch.deform_grid_coordinates
    # (device tensors in: the chain from dK to the affine runs where the autograd backward runs it)
    want = (ed.deform_points_gradient if inverse else ed.deform_grid_coordinates_gradient)(
        torch.from_numpy(q).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(D).cuda(), I, **kw)
    want = ed.PointsGradient(*[v.cpu().numpy() if torch.is_tensor(v) else v for v in want])

    def leaves():
        return (torch.from_numpy(q).cuda().requires_grad_(), torch.from_numpy(D).cuda().requires_grad_(),
                torch.from_numpy(kw["affine"]).cuda().requires_grad_())
    ut = torch.from_numpy(u).cuda()
    qt, Dt, At = leaves()
    extra = dict(return_converged=True) if inverse else dict(jacobian=True)
    out, aux = fn(qt, Dt, I, crop=kw["crop"], affine=At, displacement_grad=True, affine_grad=True, **extra)
    assert out.requires_grad and not aux.requires_grad
    (out * ut).sum().backward()
    _same_bits(qt.grad.cpu().numpy(), want.points)
    _same_bits(Dt.grad.cpu().numpy(), want.displacement)
    _same_bits(At.grad.cpu().numpy(), want.affine)
    plain = (ed.deform_points if inverse else ed.deform_grid_coordinates)(q, D, I, **kw)
    _same_bits(out.detach().cpu().numpy(), plain)
    # the switches off: only the points get a gradient
    qt, Dt, At = leaves()
    out = fn(qt, Dt, I, crop=kw["crop"], affine=At)
    (out * ut).sum().backward()
    _same_bits(qt.grad.cpu().numpy(), want.points)
    assert Dt.grad is None and At.grad is None
    # nothing requires a gradient: today's call
    out, aux = fn(qt.detach(), Dt.detach(), I, crop=kw["crop"], affine=At.detach(), **extra)
    assert not out.requires_grad and not aux.requires_grad and out.grad_fn is None
    _same_bits(out.cpu().numpy(), plain)
    assert isinstance(fn(q, D, I, **kw), np.ndarray)
    # only the displacement: the points' rows are not asked for
    qt, Dt, At = leaves()
    out = fn(qt.detach(), Dt, I, crop=kw["crop"], affine=kw["affine"], displacement_grad=True)
    (out * ut).sum().backward()
    _same_bits(Dt.grad.cpu().numpy(), want.displacement)


_SUBSETS = [s for s in itertools.product([False, True], repeat=3) if any(s)]


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("want", _SUBSETS, ids=["+".join(n for n, w in zip(("rows", "ddisp", "dK"), s) if w)
                                                for s in _SUBSETS])
def test_every_subset_of_the_results_has_the_bits_of_the_full_call(inverse, want):
    """the one library call behind both gradients, asked for any subset of (rows, d displacement, dK) as the autograd
    backward asks it: what is asked for has the bits of the call that asks for all three, the rest is None"""
    I, D, q, u, kw = _contract_case()
    if inverse:
        q = restate(q, D, I, _offsets(kw["crop"], 2), _K(I, **kw))
    args = (q, u, D, I, kw["crop"], None, kw["affine"], None, None, inverse, False)
    full = etorch._api._points_gradient(*args)[1:]
    got = etorch._api._points_gradient(*args, want_points=want[0], want_disp=want[1], want_map=want[2])[1:]
    for g, f, wanted in zip(got, full, want):
        if wanted:
            _same_bits(g.cpu().numpy() if torch.is_tensor(g) else g, f.cpu().numpy() if torch.is_tensor(f) else f)
        else:
            assert g is None


# ---- 8. a landmark fit's derivative ----------------------------------------------------------------------------

def test_landmark_fit_derivative_and_descent():
    I = (40, 52)
    D = _grid(51, 2, (5, 5), 2.0)
    rng = np.random.default_rng(52)
    p = rng.uniform(4, np.asarray(I) - 5.0, size=(200, 2))
    t = ed.deform_points(p, _grid(53, 2, (5, 5), 2.0), I, tol=1e-12)
    assert np.isfinite(t).all()
    pt, tt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()

    def loss(Dn):
        q, ok = ed.deform_points(p, Dn, I, tol=1e-12, return_converged=True)
        assert ok.all()
        return float(((q - t) ** 2).sum())

    Dt = torch.from_numpy(D).cuda().requires_grad_()
    L = ((etorch.deform_points(pt, Dt, I, tol=1e-12, displacement_grad=True) - tt) ** 2).sum()
    L.backward()
    grad = Dt.grad.cpu().numpy()
    assert abs(float(L.detach()) - loss(D)) <= 1e-9 * loss(D)
    E = rng.standard_normal(D.shape)
    h = 1e-5
    fd = (loss(D + h * E) - loss(D - h * E)) / (2 * h)
    have = float((grad * E).sum())
    print("<grad, E> = %.12g, central difference %.12g" % (have, fd))
    assert abs(have - fd) <= 1e-5 * abs(fd)
    eps = 1e-3 / np.abs(grad).max()
    assert loss(D - eps * grad) < loss(D)


# ---- 9. graph capture ----------------------------------------------------------------------------------------

def test_capture_into_a_graph():
    I, D, q, u, kw = _contract_case()
    p = restate(q, D, I, _offsets(kw["crop"], 2), _K(I, **kw))
    qt, pt, ut, Dt = (torch.from_numpy(a).cuda() for a in (q, p, u, D))
    f0 = ed.deform_grid_coordinates_gradient(qt, ut, Dt, I, **kw)              # eager
    i0 = ed.deform_points_gradient(pt, ut, Dt, I, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ed.deform_grid_coordinates_gradient(qt, ut, Dt, I, **kw)               # warm-up: the stream's workspace
        ed.deform_points_gradient(pt, ut, Dt, I, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        f = ed.deform_grid_coordinates_gradient(qt, ut, Dt, I, **kw)
        i = ed.deform_points_gradient(pt, ut, Dt, I, **kw)
    for _ in range(3):
        for r in (f, i):
            r.points.zero_()
            r.displacement.fill_(7.0)
            r.inverse_map.fill_(7.0)
        with torch.cuda.stream(side):
            ed.deform_grid_coordinates_gradient(qt[:333], 3.0 * ut[:333], Dt, I, **kw)   # an eager call of another N
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in ((f, f0), (i, i0)):
            assert torch.equal(got.points, want.points) and torch.equal(got.displacement, want.displacement)
            assert torch.equal(got.inverse_map, want.inverse_map)


# ---- 10. empty, degenerate, float32, array families ------------------------------------------------------------

def test_no_points_and_length_one_axis():
    I, D, q, u, kw = _contract_case()
    for fn in (ed.deform_grid_coordinates_gradient, ed.deform_points_gradient):
        g = fn(q[:0], u[:0], D, I, **kw)
        assert g.points.shape == (0, 2) and (g.displacement == 0).all() and g.displacement.shape == D.shape
        assert (g.inverse_map == 0).all() and (g.affine == 0).all()
        gt = fn(torch.zeros((4, 2), dtype=torch.float64, device="cuda"), torch.ones((4, 2), device="cuda"),
                np.zeros((2, 3, 3)), (1, 9))
        assert gt.points.is_cuda and (gt.points == 0).all() and (gt.displacement == 0).all()
        assert (gt.inverse_map == 0).all()
    gb = ed.deform_grid_coordinates_gradient_batch(np.zeros((2, 0, 2)), np.zeros((2, 0, 2)), np.stack([D, D]), I, **kw)
    assert gb.points.shape == (2, 0, 2) and (gb.displacement == 0).all() and gb.displacement.shape == (2,) + D.shape


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_float32_points_round_once_and_array_families(inverse):
    I, D, q, u, kw = _contract_case()
    fn = ed.deform_points_gradient if inverse else ed.deform_grid_coordinates_gradient
    if inverse:
        q = restate(q, D, I, _offsets(kw["crop"], 2), _K(I, **kw))
    q32, u32 = q.astype(np.float32), u.astype(np.float32)
    g32 = fn(q32, u32, D, I, **kw)
    g64 = fn(q32.astype(np.float64), u32.astype(np.float64), D, I, **kw)
    assert g32.points.dtype == np.float32 and g64.points.dtype == np.float64
    _same_bits(g32.points, g64.points.astype(np.float32))
    _same_bits(g32.displacement, g64.displacement)
    _same_bits(g32.inverse_map, g64.inverse_map)
    # a float32 grid: its gradient in float32
    assert fn(q, u, D.astype(np.float32), I, **kw).displacement.dtype == np.float32
    # families: numpy stays numpy (a device grid included), a CPU tensor comes back on the CPU, a device tensor stays
    want = fn(q, u, D, I, **kw)
    gn = fn(q, u, torch.from_numpy(D).cuda(), I, **kw)
    assert all(isinstance(v, np.ndarray) for v in (gn.points, gn.displacement, gn.affine, gn.inverse_map))
    gc = fn(torch.from_numpy(q), torch.from_numpy(u), D, I, **kw)
    assert all(torch.is_tensor(v) and v.device.type == "cpu" for v in (gc.points, gc.displacement))
    gd = fn(torch.from_numpy(q).cuda(), torch.from_numpy(u).cuda(), D, I, **kw)
    assert all(torch.is_tensor(v) and v.is_cuda for v in (gd.points, gd.displacement, gd.affine, gd.inverse_map))
    for g in (gn, gc, gd):
        _same_bits(torch.as_tensor(g.points).cpu().numpy(), want.points)
        _same_bits(torch.as_tensor(g.displacement).cpu().numpy(), want.displacement)
        _same_bits(torch.as_tensor(g.inverse_map).cpu().numpy(), want.inverse_map)


def _library_call(u0):
    """edhip_deform_points_gradient itself (forward direction) on len(u0) samples of one point at (100, 0.5) -- sane:
    the limit is a control coordinate of 4e15 --, a prefiltered 4 x 4 grid on an 8 x 8 image, float64, the cotangent
    (u0[b], 0) for sample b: the gradient of the PREFILTERED grid, without the host layer's transposed filter (whose
    gain would take 4e307 past the largest double)."""
    import importlib
    api = importlib.import_module("elasticdeform_amd.deform_grid")
    from elasticdeform_amd import _lib
    nb = len(u0)
    P = torch.from_numpy(np.random.default_rng(11).random((2, 4, 4)) - 0.5).cuda().repeat(nb, 1, 1, 1)
    q = torch.tensor([[100.0, 0.5]], dtype=torch.float64).cuda().repeat(nb, 1, 1)
    u = torch.tensor([[[v, 0.0]] for v in u0], dtype=torch.float64).cuda()
    rows, dP = torch.full_like(q, 7.0), torch.full_like(P, 7.0)
    dK = torch.full((nb, 2, 3), 7.0, dtype=torch.float64).cuda()
    _lib.deform_points_gradient(0, nb, *api._desc_sample0(q), *api._desc_sample0(u), None, 0, *api._desc_sample0(P),
                                (8, 8), None, None, *api._desc_sample0(rows), *api._desc_sample0(dP),
                                *api._desc_sample0(dK), 0, api._stream(q.device))
    torch.cuda.synchronize()
    return rows.cpu().numpy(), dP.cpu().numpy(), dK.cpu().numpy()


def test_a_bound_that_overflows_poisons_both_sums_of_its_sample_only():
    """bP = 2 N max|u| = 8e307 is finite, bK = bP max(1, max|q|) = bP * 100 is not: this call's rule makes BOTH sums
    of the sample NaN; the point's own row J^T u is finite.  A second sample with the cotangent (1, 0) in the same
    call gives the bits of a call of its own."""
    rows, dP, dK = _library_call([4e307])
    assert np.isnan(dP).all() and np.isnan(dK).all() and np.isfinite(rows).all()
    rows2, dP2, dK2 = _library_call([4e307, 1.0])
    rows1, dP1, dK1 = _library_call([1.0])
    _same_bits(rows2[0], rows[0]), _same_bits(dP2[0], dP[0]), _same_bits(dK2[0], dK[0])
    _same_bits(rows2[1], rows1[0]), _same_bits(dP2[1], dP1[0]), _same_bits(dK2[1], dK1[0])
    assert np.isfinite(dP1).all() and abs(dP1[0, 0].sum() - 1.0) <= 1e-12 and not dP1[0, 1].any()
    assert np.array_equal(dK1[0], [[100.0, 0.5, 1.0], [0.0, 0.0, 0.0]])
