"""
Host tests that anchor the analytic gradient reference (oracle/dgrad_reference.py) before anything runs on a GPU.

1. dD and dK against central differences of the CPU oracle's float64 deform_grid, with the recipes of
   tests/test_displacement_gradient.py (_fd) and tests/test_affine_gradient.py (_fd_params, applied to the entries of
   the inverse map K): L = sum <dY, Y>, every entry perturbed by h = 1e-6 max(1, |value|), tolerance 1e-6 of
   max |want|.  (A perturbed K reaches the oracle as the affine whose inverse it is.)
2. The case table of tests/test_dgrad_routes.py through the reference alone: the fraction of coordinates outside the
   volume is between 0.05 and 0.95 in the mode cases, and on every case the float64 bound of the GPU comparison,
   c 2^-53 max S, is at most 1e-9 max |want| -- three orders under the finite-difference tolerance.
"""
import functools

import numpy as np
import pytest

import dgrad_cases as dc
from oracle import dgrad_reference as ref
from oracle import ed_oracle as orc

MODES = dc.MODES
TOL = 1e-6


def _loss(X, D, dY, kw):
    Y = orc.deform_grid(X, D, **kw)
    Ys, dYs = (Y, dY) if isinstance(Y, list) else ([Y], [dY])
    return sum(float(np.sum(y.astype(np.float64) * dy)) for y, dy in zip(Ys, dYs))


def _fd(X, D, dY, kw):
    g = np.zeros_like(D)
    for idx in np.ndindex(*D.shape):
        h = 1e-6 * max(1.0, abs(D[idx]))
        Dp, Dm = D.copy(), D.copy()
        Dp[idx] += h
        Dm[idx] -= h
        g[idx] = (_loss(X, Dp, dY, kw) - _loss(X, Dm, dY, kw)) / (2 * h)
    return g


def _fd_map(X, D, dY, kw):
    """central differences with respect to every entry of the inverse map K of the call"""
    n = D.shape[0]
    Xs = X if isinstance(X, list) else [X]
    axes, out_shapes = orc.prepare(Xs, D, kw["order"], kw["mode"], 0.0, kw.get("crop"), kw.get("axis"), None, None,
                                   None)[:2]
    K = orc._inverse_affine(kw.get("affine"), kw.get("rotate"), kw.get("zoom"), n, [out_shapes[0][d] for d in axes[0]])
    K = np.concatenate([np.eye(n), np.zeros((n, 1))], 1) if K is None else np.array(K, dtype=np.float64)
    bare = {k: v for k, v in kw.items() if k not in ("affine", "rotate", "zoom")}

    def loss(k):
        lin = np.linalg.inv(k[:, :n])                      # the affine whose inverse map is k
        return _loss(X, D, dY, dict(bare, affine=np.concatenate([lin, -lin @ k[:, n:]], 1)))

    g = np.zeros_like(K)
    for idx in np.ndindex(*K.shape):
        h = 1e-6 * max(1.0, abs(K[idx]))
        kp, km = K.copy(), K.copy()
        kp[idx] += h
        km[idx] -= h
        g[idx] = (loss(kp) - loss(km)) / (2 * h)
    return g


def _case(shape, ncp, sigma, seed, nin=1, channels=None):
    rng = np.random.default_rng(seed)
    n = len(shape)
    full = tuple(shape) + ((channels,) if channels else ())
    X = [rng.standard_normal(full) for _ in range(nin)]
    D = rng.standard_normal((n,) + tuple(ncp)) * sigma
    return (X if nin > 1 else X[0]), D, rng


def _check(X, D, kw, rng):
    Y = orc.deform_grid(X, D, **kw)
    dY = [rng.standard_normal(y.shape) for y in Y] if isinstance(Y, list) else rng.standard_normal(Y.shape)
    got = ref.reference(X, dY, D, **kw)
    for name, have, want in (("dD", got.dD, _fd(X, D, dY, kw)), ("dK", got.dK, _fd_map(X, D, dY, kw))):
        assert have.shape == want.shape and have.dtype == np.float64
        scale = np.abs(want).max()
        assert scale > 0
        err = np.abs(have - want).max()
        assert err <= TOL * scale, (name, err / scale, kw)
    return got


SHAPES = {1: ((40,), (5,), 1.5), 2: ((24, 30), (4, 5), 1.5), 3: ((9, 10, 8), (3, 4, 3), 1.0)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_orders_and_modes_against_finite_differences(n, order, mode):
    shape, ncp, sigma = SHAPES[n]
    X, D, rng = _case(shape, ncp, sigma, 100 * n + 10 * order + MODES.index(mode))
    _check(X, D, dict(order=order, mode=mode), rng)


def test_4d_against_finite_differences():
    X, D, rng = _case((6, 5, 6, 5), (3, 3, 3, 3), 0.8, 300)
    _check(X, D, dict(order=3, mode="mirror"), rng)


def test_crop_affine_rotate_zoom_prefilter():
    X, D, rng = _case((24, 30), (4, 5), 1.5, 400)
    A = np.array([[1.04, 0.05, 0.3], [-0.04, 0.97, -0.2]])
    _check(X, D, dict(order=3, mode="mirror", crop=(slice(3, 20), slice(5, 27)), affine=A), rng)
    _check(X, D, dict(order=3, mode="nearest", rotate=17.0, zoom=1.1), rng)
    _check(X, D, dict(order=3, mode="reflect", prefilter=False), rng)
    X3, D3, rng = _case((9, 10, 8), (3, 3, 3), 1.0, 401)
    A3 = np.array([[1.05, 0.05, 0.0, 0.3], [-0.04, 0.97, 0.03, -0.2], [0.02, 0.0, 1.02, 0.1]])
    _check(X3, D3, dict(order=2, mode="wrap", affine=A3, crop=(slice(1, 8), slice(2, 9), slice(0, 7))), rng)


def test_two_inputs_and_a_channel_axis():
    X, D, rng = _case((20, 22), (4, 4), 1.5, 501, nin=2)
    _check(X, D, dict(order=[3, 1], mode=["mirror", "nearest"]), rng)
    X, D, rng = _case((20, 22), (4, 4), 1.5, 500, channels=3)
    _check(X, D, dict(order=3, mode="mirror", axis=(0, 1)), rng)


@pytest.mark.parametrize("ncp", [(4, 1), (4, 2), (4, 3), (1, 5), (2, 5), (1, 1)])
def test_control_axes_of_one_to_three_points(ncp):
    # (every tap window of such an axis sticks out of the grid: several taps fold onto one control point)
    X, D, rng = _case((12, 30), ncp, 1.5, 600 + 10 * ncp[0] + ncp[1])
    _check(X, D, dict(order=3, mode="mirror"), rng)


def test_the_grid_coordinates_equal_the_point_restatement():
    # two routes to c(o): the separable matrices of `reference` and `coordinate`, the per-point tap loop
    D = np.random.default_rng(700).standard_normal((2, 4, 2)) * 2
    I, off = (13, 17), np.array([2.0, 3.0])
    K = np.array([[1.1, 0.15, -1.5], [-0.1, 0.9, 2.0]])
    o = np.indices((9, 12)).reshape(2, -1).T.astype(np.float64)
    want = ref.coordinate(o, D, I, off, K)
    B = [ref.control_matrix(m, D.shape[d + 1], I[d], off[d]) for d, m in enumerate((9, 12))]
    delta = np.einsum("hjk,aj,bk->abh", ref.prefiltered(D), B[0], B[1]).reshape(-1, 2)
    np.testing.assert_allclose(o @ K[:, :2].T + K[:, 2] + off + delta, want, rtol=0, atol=1e-12)


# ---- the GPU case table, through the reference alone ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _table_reference(name):
    case = next(c for c in dc.CASES if c["name"] == name)
    X, dY, D, kw = dc.make(case)
    up = (lambda a: a.astype(np.float64))
    if case.get("batch"):
        return case, [ref.reference(X[b], dY[b], D[b], **kw) for b in range(case["batch"])]
    if case.get("f32"):
        return case, [ref.reference(up(X), up(dY), D, **kw), ref.reference(X, dY, D, f32=True, **kw)]
    return case, [ref.reference(X, dY, D, **kw)]


def test_the_table_reaches_what_it_names():
    names = [c["name"] for c in dc.CASES]
    assert len(set(names)) == len(names)
    blocks, Ks = set(), set()
    for c in dc.CASES:
        L = (c["crop"][-1][1] - c["crop"][-1][0]) if c.get("crop") else c["shape"][-1]
        blocks.add((256 if L > 128 else (128 if L > 64 else 64), -(-L // 256)))
        Ks.add(len(c["shape"]) * c["ncp"][-1])
        assert len(c["shape"]) * c["ncp"][-1] <= 256
    assert {(128, 1), (256, 1), (256, 2), (256, 3)} <= blocks
    assert {32, 34, 66, 200, 255, 256} <= Ks
    assert {len(c["shape"]) for c in dc.CASES} == {1, 2, 3, 4, 5, 6, 7}


@pytest.mark.parametrize("name", [c["name"] for c in dc.F64_CASES])
def test_table_float64_conditions(name):
    case, results = _table_reference(name)
    for r in results:
        if case.get("modes_case"):
            assert 0.05 <= r.outside <= 0.95, r.outside
        c_d, c_k = dc.rounding_counts(case, r.cmax, r.dmax)
        for c, S, want in ((c_d, r.S_D, r.dD), (c_k, r.S_K, r.dK)):
            assert np.all(np.isfinite(want)) and np.abs(want).max() > 0
            assert c * dc.U * S.max() <= 1e-9 * np.abs(want).max(), (c, S.max() / np.abs(want).max())


@pytest.mark.parametrize("name", [c["name"] for c in dc.F32_CASES])
def test_table_float32_restatement(name):
    # the float32 restatement differs from the float64 reference by float32 rounding of the tap sum and no more:
    # (p + 1)^n additions and n + 1 products per tap, and the float32 prefilter of the volume (counted 3 per axis),
    # each 2^-24, relative to the tap-level scale
    case, (exact, single) = _table_reference(name)
    n, p = len(case["shape"]), case["order"]
    count = (p + 1) ** n + 4 * n + 2
    for got, want, S in ((single.dD, exact.dD, exact.S_D), (single.dK, exact.dK, exact.S_K)):
        err = np.abs(got - want)
        assert err.max() > 0
        assert np.all(err <= count * 2.0 ** -24 * S)
