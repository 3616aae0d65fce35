"""
GPU tests of deform_grid_inverse / deform_grid_inverse_batch (edhip_deform_inverse): an image resampled back through a
deformation, Z[p] = S_Y(q(p)) with r(q(p)) = p.

Expected values come from sources that share no code with the kernel:

* affine only (D = 0): r is affine, so q(p) = M (p - c - off) is affine too, and the expected Z is the CPU oracle's own
  gather (oracle.deform_raw) of the prefiltered Y with that map as its affine matrix;
* elastic fields: q comes from the existing deform_points kernel (verified here with the NumPy restatement of r from
  tests/test_points.py, restate(q) == p to 1e-8) and is sampled by scipy.ndimage.map_coordinates (mode 'mirror',
  orders 1-5) or by a small NumPy restatement of the gather (`np_gather` below; the other modes and order 0), which is
  itself checked against the oracle and against SciPy before use.

Tolerance.  Two solvers that both stop at |r(q) - p| <= tol differ by at most 2 tol |J^-1|.  With tol = 1e-10, a mild
field (|J^-1| <= 2, det J > 0.4) and Y in [0, 1], whose prefiltered interpolant has a slope of order 10 per voxel at
most, float64 results agree to 1e-8 absolute, float32 results to 1e-8 plus one float32 ulp of the value, integer
results exactly.  A voxel is left out of the comparison where the expected q lies within 1e-6 of a decision boundary,
where a 1e-9 difference in q may legitimately flip the branch: for order 0 and integer outputs a half-integer on any
axis (or a rounding tie of the value: for Y scaled to +-1000 two solvers' values differ by 4e-10 * 1e4 at most, the
margin is 1e-3), for 'constant' and for `valid` 0 or O_k - 1, for 'wrap' the fold points k (O_k - 1) of the mode.
Those sets have measure zero; the test asserts that the excluded share is below 1 % in every case.

The 2-D (sigma 3 on a control spacing of 4) and 3-D (sigma 1.5 on spacings of 2.3 to 4.3) fields are NOT mild: for
every seed of 1000 (2-D) / 100 (3-D) tried they fold (min det J < 0 on the lattice), and some voxels are not solved.
The cases stay, and the assumption of the bound is applied per voxel, which is what the bound is: a voxel with
det J(q) > 0.4 and |J(q)^-1|_inf <= 2 is held to 1e-8; elsewhere the same reasoning gives 1e-8 * |J(q)^-1|_inf / 2 and
that is what is asked there; an unsolved voxel must be cval exactly and not valid.  The "-mild" cases are the same
geometries with sigma scaled down until det J > 0.4 holds on the whole lattice, which is asserted, and every voxel of
them is held to 1e-8.
"""
import itertools
import math

import numpy as np
import pytest

from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402

TOL = 1e-8                 # float64 results, absolute
SOLVER_TOL = 1e-10
MAX_ITER = 32
EDGE = 1e-6                # thickness of a decision boundary in q
MODES = ["nearest", "wrap", "reflect", "mirror", "constant"]
ORDERS = [0, 1, 2, 3, 4, 5]
CVAL = 0.25

AFFINE3 = np.array([[1.05, 0.1, 0.0, -1.0], [-0.08, 0.95, 0.05, 0.5], [0.02, -0.04, 1.1, 1.5]])
CROP2 = (slice(2, 11), slice(3, 15))


# ---- the NumPy restatement of r (tests/test_points.py) and of the gather ----------------------------------------

def _prefiltered_grid(D):
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


def _cubic_weights(x):
    z = 1.0 - x
    w0 = z * z * z / 6.0
    w1 = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], axis=-1)


def restate(q, D, I, off=None, K=None):
    """r(q) for q of shape (N, n), vectorised over the points"""
    q = np.asarray(q, dtype=np.float64)
    n = D.shape[0]
    ncp = D.shape[1:]
    P = _prefiltered_grid(D)
    off = np.zeros(n) if off is None else np.asarray(off, dtype=np.float64)
    K = np.concatenate([np.eye(n), np.zeros((n, 1))], axis=1) if K is None else np.asarray(K, dtype=np.float64)
    idx, W = [], []
    for k in range(n):
        cp = (ncp[k] - 1) * (q[:, k] + off[k]) / (I[k] - 1)
        fl = np.floor(cp)
        W.append(_cubic_weights(cp - fl))
        idx.append(_mirror(fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], ncp[k]))
    delta = np.zeros((q.shape[0], n))
    for taps in itertools.product(range(4), repeat=n):
        w = np.ones(q.shape[0])
        for k in range(n):
            w = w * W[k][:, taps[k]]
        delta += P[(slice(None),) + tuple(idx[k][:, taps[k]] for k in range(n))].T * w[:, None]
    return q @ K[:, :n].T + K[:, n] + off + delta


def _bspline(x, order):
    """the centred cardinal B-spline of degree `order` at x (truncated powers)"""
    acc = np.zeros_like(x)
    for k in range(order + 2):
        acc += (-1) ** k * math.comb(order + 1, k) * np.maximum(x + (order + 1) / 2.0 - k, 0.0) ** order
    return acc / math.factorial(order)


def _map_legacy(c, n, mode):
    """the boundary map of a real coordinate, legacy SciPy semantics; NaN where 'constant' leaves the array"""
    c = np.array(c, dtype=np.float64)
    lo, hi = c < 0, c > n - 1
    if mode == "nearest":
        return np.clip(c, 0, n - 1)
    if mode == "constant":
        return np.where(lo | hi, np.nan, c)
    if mode == "wrap":
        period = n - 1
        below = c + period * (np.trunc(-c / period) + 1)
        above = c - period * np.trunc(c / period)
        return np.where(lo, below, np.where(hi, above, c))
    if mode == "mirror":
        period = 2 * n - 2
        m = np.mod(np.abs(c), period)
        return np.where(m > n - 1, period - m, m)
    period = 2 * n                                   # reflect: about -0.5 and n - 0.5, the legacy map unclipped
    below = np.where(c < -period, period * np.trunc(-c / period) + c, c)
    below = np.where(below < -n, below + period, -below - 1)
    above = c - period * np.trunc(c / period)
    above = np.where(above >= n, period - above - 1, above)
    return np.where(lo, below, np.where(hi, above, c))


def np_gather(Yf, q, order, mode, cval):
    """S_Y(q) in float64 for q of shape (N, n) on the (prefiltered) array Yf whose FIRST n axes are the deformed ones;
    the result has shape (N,) + the remaining axes"""
    n = q.shape[1]
    O = Yf.shape[:n]
    Yf = Yf.astype(np.float64)
    outside = np.zeros(q.shape[0], dtype=bool)
    idx, W = [], []
    for k in range(n):
        c = _map_legacy(q[:, k], O[k], mode)
        outside |= np.isnan(c)
        c = np.where(np.isnan(c), 0.0, c)
        start = (np.floor(c) if order & 1 else np.floor(c + 0.5)).astype(np.int64) - order // 2
        taps = start[:, None] + np.arange(order + 1)[None, :]
        W.append(_bspline(c[:, None] - taps, order) if order > 0 else np.ones_like(taps, dtype=np.float64))
        idx.append(_mirror(taps, O[k]))
    out = np.zeros((q.shape[0],) + Yf.shape[n:])
    for taps in itertools.product(range(order + 1), repeat=n):
        w = np.ones(q.shape[0])
        for k in range(n):
            w = w * W[k][:, taps[k]]
        vals = Yf[tuple(idx[k][:, taps[k]] for k in range(n))]
        out += vals * w.reshape((-1,) + (1,) * (vals.ndim - 1))
    out[outside] = cval
    return out


def store_rule(t, dtype):
    """the forward store of an fp64 value: the C cast for floats, round half away from zero and clamp for integers"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return t.astype(dtype)
    info = np.iinfo(dtype)
    r = np.where(t > 0, t + 0.5, t - 0.5) if info.min < 0 else np.where(t > 0, t + 0.5, 0.0)
    return np.trunc(np.clip(r, info.min, info.max)).astype(dtype)


def prefilter(Y, order, axes):
    """the reference's prefilter of an input along its deformed axes (the oracle's restatement of it)"""
    if order <= 1:
        return Y
    out = np.zeros_like(Y)
    src = Y
    for d in axes:
        orc.spline_filter1d(src, order, d, out)
        src = out
    return out


# ---- geometry helpers --------------------------------------------------------------------------------------------

def _offsets(crop, n):
    return np.zeros(n) if crop is None else np.array([float(s.start or 0) for s in crop])


def _out_shape(I, crop):
    return tuple(I) if crop is None else tuple((s.stop or i) - (s.start or 0) for s, i in zip(crop, I))


def _K(I, crop=None, affine=None, rotate=None, zoom=None):
    """the inverse map of the call, from the oracle's own restatement of the reference's matrix algebra"""
    if affine is None and rotate is None and zoom is None:
        return None
    return orc._inverse_affine(affine, rotate, zoom, len(I), list(_out_shape(I, crop)))


def _grid(seed, n, ncp, sigma, dtype=np.float64):
    D = np.random.default_rng(seed).standard_normal((n,) + tuple(ncp)) * sigma
    return np.round(D).astype(dtype) if np.dtype(dtype).kind == "i" else D.astype(dtype)


def _lattice(I):
    return np.stack(np.indices(I), axis=-1).reshape(-1, len(I)).astype(np.float64)


def _image(seed, shape, dtype=np.float64):
    """Y in [0, 1]; integer types: scaled to the type's range, capped at +-1000"""
    y = np.random.default_rng(seed).uniform(0.0, 1.0, size=shape)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return y.astype(dtype)
    info = np.iinfo(dtype)
    lo, hi = max(info.min, -1000), min(info.max, 1000)
    return np.round(lo + y * (hi - lo)).astype(dtype)


def boundary_mask(q, O, order, mode, integer_output):
    """True where q lies within EDGE of a decision boundary of the gather (see the head of the file)"""
    q = np.asarray(q)
    near = np.zeros(q.shape[0], dtype=bool)
    for k in range(q.shape[1]):
        if order == 0 or integer_output:
            near |= np.abs(q[:, k] - np.floor(q[:, k]) - 0.5) < EDGE
        if mode == "constant":
            near |= (np.abs(q[:, k]) < EDGE) | (np.abs(q[:, k] - (O[k] - 1)) < EDGE)
        if mode == "wrap":
            period = O[k] - 1
            near |= np.abs(q[:, k] - period * np.round(q[:, k] / period)) < EDGE
    return near


def valid_boundary_mask(q, O):
    near = np.zeros(q.shape[0], dtype=bool)
    for k in range(q.shape[1]):
        near |= (np.abs(q[:, k]) < EDGE) | (np.abs(q[:, k] - (O[k] - 1)) < EDGE)
    return near


def compare(got, want, want_fp64, q, O, order, mode, what, ok=None, slack=None, alts=None):
    """got == want within the tolerance of the dtype, away from the decision boundaries; prints the figures first.
    ok (all, if None): the solved voxels -- the others must hold cval; slack (1, if None): the per-voxel factor on the
    float tolerance, max(1, |J^-1| / 2); alts: expected arrays for q nudged to either side -- a voxel near a decision
    boundary is then not left out: it must equal one of them"""
    dtype = got.dtype
    integer = dtype.kind in "iub"
    npts = q.shape[0]
    ok = np.ones(npts, dtype=bool) if ok is None else ok
    unsolved = int((~ok).sum())
    slack = np.ones(npts) if slack is None else slack
    g_all = got.reshape(npts, -1)
    if not ok.all():
        assert (g_all[~ok] == store_rule(np.array([CVAL]), dtype)[0]).all()
    skip = boundary_mask(q, O, order, mode, integer) & ok
    tie = np.zeros(npts, dtype=bool)
    if integer and want_fp64 is not None:
        flat = want_fp64.reshape(npts, -1)
        tie = ok & (np.abs(flat - np.floor(flat) - 0.5) < 1e-3).any(axis=1)         # a rounding tie of the value
    if alts is not None:
        # an affine map sends lattice points EXACTLY onto boundaries (1.05 * 0 + 0.1 * 10 - 1.0 = 0, 1.05 * 10 - 1.0 =
        # 9.5: up to 9 % of the 3-D case's voxels): which side the rounding of q falls on is open, the value must be
        # that of one of the sides (an integer that is a rounding tie as well -- order 1 halfway between two voxels
        # -- may land on either neighbour)
        tol_alt = tie.astype(np.float64) if integer else np.full(npts, TOL + (1.2e-7 if dtype == np.float32 else 0.0))
        best = np.min([np.abs(g_all.astype(np.float64) - a.reshape(npts, -1).astype(np.float64)).max(axis=1)
                       for a in alts], axis=0)
        print("%s: %d voxels on a decision boundary, compared with every side: max |err| %.3g"
              % (what, skip.sum(), best[skip].max() if skip.any() else 0.0))
        scale = np.maximum(1.0, np.abs(want.reshape(npts, -1)).max(axis=1))
        assert (best[skip] <= (tol_alt * (1.0 if integer else scale))[skip]).all()
        ok = ok & ~skip
        tie = tie & ok
        skip = np.zeros(npts, dtype=bool)
    skip |= tie
    share = skip.mean()
    keep = ok & ~skip
    g = g_all[keep].astype(np.float64)
    w = want.reshape(npts, -1)[keep].astype(np.float64)
    err = np.abs(g - w)
    if integer:
        bound = np.zeros_like(err)
    elif dtype == np.float32:
        bound = TOL * slack[keep][:, None] + np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
    else:
        bound = TOL * slack[keep][:, None] + np.zeros_like(err)
    print("%s: max |err| %.3g (largest err / bound %.3g) over %d voxels, %d unsolved, excluded share %.4f"
          % (what, err.max() if err.size else 0.0, (err / np.maximum(bound, 1e-300)).max() if err.size and not integer
             else 0.0, keep.sum(), unsolved, share))
    assert share < 0.01
    assert not np.isnan(g_all).any()
    assert (err <= bound).all()


# ---- 1. affine only, against the oracle ------------------------------------------------------------------------

AFFINE_CASES = {
    "2d": dict(I=(13, 17), crop=CROP2, rotate=20.0, zoom=1.3),
    "3d": dict(I=(12, 14, 10), affine=AFFINE3),
}


def _affine_expected(name, order, mode, dtype):
    """(Y, the call's keyword arguments, the oracle's Z, q(p), O)"""
    c = dict(AFFINE_CASES[name])
    I = c.pop("I")
    n = len(I)
    crop = c.get("crop")
    O = _out_shape(I, crop)
    Y = _image(5 + n, O, dtype)
    K = _K(I, crop, c.get("affine"), c.get("rotate"), c.get("zoom"))
    off = _offsets(crop, n)
    M = np.linalg.inv(K[:, :n])
    inv = np.concatenate([M, (-M @ (K[:, n] + off))[:, None]], axis=1)       # q(p) = M (p - c - off)
    q = _lattice(I) @ M.T + inv[:, n]
    Yf = prefilter(Y, order, range(n))
    Zs = []
    # the map itself, and q moved by 1e-12 to every side of a boundary it may sit on
    for nudge in [np.zeros(n)] + [np.array(s) for s in itertools.product((1e-12, -1e-12), repeat=n)]:
        Z = np.zeros(I, dtype=Y.dtype)
        moved = inv.copy()
        moved[:, n] += nudge
        orc.deform_raw(0, [Yf], np.zeros((n,) + (3,) * n), None, [Z], [tuple(range(n))], [order],
                       [orc._MODE_CODES[mode]], [CVAL], moved)
        Zs.append(Z)
    return Y, c, Zs[0], q, O, Zs[1:]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(AFFINE_CASES))
def test_affine_only_equals_the_oracle_gather(name, order, mode):
    Y, kw, want, q, O, alts = _affine_expected(name, order, mode, np.float64)
    I = want.shape
    D = np.zeros((len(I),) + (3,) * len(I))
    got = ed.deform_grid_inverse(Y, D, I, order=order, mode=mode, cval=CVAL, tol=SOLVER_TOL, max_iter=MAX_ITER, **kw)
    assert got.shape == I and got.dtype == np.float64
    compare(got, want, None, q, O, order, mode, "%s order %d %s" % (name, order, mode), alts=alts)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.uint8])
@pytest.mark.parametrize("name", sorted(AFFINE_CASES))
def test_affine_only_other_dtypes(name, dtype, order, mode):
    Y, kw, want, q, O, alts = _affine_expected(name, order, mode, dtype)
    I = want.shape
    D = np.zeros((len(I),) + (3,) * len(I))
    got = ed.deform_grid_inverse(Y, D, I, order=order, mode=mode, cval=CVAL, tol=SOLVER_TOL, max_iter=MAX_ITER, **kw)
    assert got.shape == I and got.dtype == np.dtype(dtype)
    fp64 = None
    if np.dtype(dtype).kind in "iu":
        fp64 = np_gather(prefilter(Y, order, range(len(I))), q, order, mode, CVAL)
    compare(got, want, fp64, q, O, order, mode, "%s %s order %d %s" % (name, np.dtype(dtype).name, order, mode),
            alts=alts)


# ---- the NumPy gather is checked before it is used ---------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(AFFINE_CASES))
def test_the_numpy_gather_equals_the_oracle(name, order, mode):
    Y, _, want, q, O, alts = _affine_expected(name, order, mode, np.float64)
    got = np_gather(prefilter(Y, order, range(len(O))), q, order, mode, CVAL).reshape(want.shape)
    compare(got, want, None, q, O, order, mode, "np_gather %s order %d %s" % (name, order, mode), alts=alts)


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_the_numpy_gather_equals_scipy_for_mirror(order):
    import scipy.ndimage
    Y = _image(3, (9, 12))
    q = np.random.default_rng(4).uniform(-12.0, 24.0, size=(500, 2))
    want = scipy.ndimage.map_coordinates(Y, q.T, order=order, mode="mirror")
    got = np_gather(prefilter(Y, order, range(2)), q, order, "mirror", CVAL)
    assert np.abs(got - want).max() <= 1e-10


# ---- 2. elastic fields, against deform_points plus an independent sampler ----------------------------------------

ELASTIC = {
    "1d-affine": dict(I=(40,), ncp=(5,), sigma=2.0, seed=0, affine=np.array([[1.1, -1.5]]), mild=True),
    "2d-crop": dict(I=(13, 17), ncp=(4, 5), sigma=3.0, seed=91, crop=CROP2),
    "3d": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5, seed=88),
    "2d-crop-mild": dict(I=(13, 17), ncp=(4, 5), sigma=0.8, seed=91, crop=CROP2, mild=True),
    "3d-mild": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=0.25, seed=88, mild=True),
    # more than 7680 grid values: the control grid is read from global memory
    "2d-global-grid": dict(I=(70, 70), ncp=(62, 62), sigma=0.08, seed=1, mild=True),
}
_expected_q = {}


def _elastic(name):
    """(I, O, D, geometry keywords, q, ok, slack) with q, ok from deform_points, verified with the restatement;
    slack = max(1, |J(q)^-1|_inf / 2) per solved voxel.  Computed once per case."""
    c = dict(ELASTIC[name])
    I, ncp, sigma, seed, mild = c.pop("I"), c.pop("ncp"), c.pop("sigma"), c.pop("seed"), c.pop("mild", False)
    n = len(I)
    D = _grid(seed, n, ncp, sigma)
    crop = c.get("crop")
    O = _out_shape(I, crop)
    if name not in _expected_q:
        p = _lattice(I)
        q, ok = ed.deform_points(p, D, I, max_iter=MAX_ITER, tol=SOLVER_TOL, return_converged=True, **c)
        K = _K(I, crop, c.get("affine"))
        res = np.abs(restate(q[ok], D, I, _offsets(crop, n), K) - p[ok]).max()
        _, J = ed.deform_grid_coordinates(q[ok], D, I, jacobian=True, **c)
        det = np.linalg.det(J)
        slack = np.ones(p.shape[0])
        slack[ok] = np.maximum(1.0, np.abs(np.linalg.inv(J)).sum(axis=2).max(axis=1) / 2.0)
        print("%s: %d of %d solved, max |restate(q) - p| %.3g, min det J %.3g, largest slack %.3g, %d voxels with slack"
              % (name, ok.sum(), ok.size, res, det.min(), slack.max(), (slack > 1).sum()))
        assert res <= 1e-8
        if mild:                                                 # the mild field the tolerance assumes
            assert ok.all() and det.min() > 0.4 and (slack == 1.0).all()
        _expected_q[name] = (np.where(ok[:, None], q, 0.0), ok, slack)
    q, ok, slack = _expected_q[name]
    return I, O, D, c, q, ok, slack


def _sample(Y, q, order, mode):
    if mode == "mirror" and order >= 1:
        import scipy.ndimage
        return scipy.ndimage.map_coordinates(Y, q.T, order=order, mode="mirror")
    return np_gather(prefilter(Y, order, range(q.shape[1])), q, order, mode, CVAL)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["1d-affine", "2d-crop", "3d", "2d-crop-mild", "3d-mild"])
def test_elastic_field_equals_deform_points_plus_a_sampler(name, order, mode):
    I, O, D, kw, q, ok, slack = _elastic(name)
    Y = _image(7 + len(I), O)
    Z, valid = ed.deform_grid_inverse(Y, D, I, order=order, mode=mode, cval=CVAL, tol=SOLVER_TOL, max_iter=MAX_ITER,
                                      return_valid=True, **kw)
    assert Z.shape == I and Z.dtype == np.float64 and valid.shape == I and valid.dtype == np.uint8
    want = _sample(Y, q, order, mode).reshape(I)
    compare(Z, want, None, q, O, order, mode, "%s order %d %s" % (name, order, mode), ok, slack)
    # 3. valid == ok & (0 <= q <= O - 1)
    inside = ok & ((q >= 0) & (q <= np.array(O) - 1)).all(axis=1)
    keep = ~valid_boundary_mask(q, O) | ~ok
    print("valid: %d of %d voxels, %d compared" % (inside.sum(), inside.size, keep.sum()))
    assert keep.mean() > 0.99
    assert (valid.reshape(-1)[keep] == inside[keep]).all()


# ---- 3. unsolved voxels -----------------------------------------------------------------------------------------

def test_unsolved_voxels_take_cval_and_are_not_valid():
    """a strongly folding field (sigma = the control spacing): where deform_points does not solve, Z = cval in a mode
    that never produces cval by itself, valid = 0 and nothing is NaN"""
    I, ncp = (13, 17), (4, 5)
    D = _grid(3, 2, ncp, 4.0)
    Y = _image(9, I) + 1.0                                        # in [1, 2]: cval = 0.25 is not a value of Y
    q, ok = ed.deform_points(_lattice(I), D, I, max_iter=8, tol=SOLVER_TOL, return_converged=True)
    print("unsolved: %d of %d" % ((~ok).sum(), ok.size))
    assert 0 < (~ok).sum() < ok.size
    Z, valid = ed.deform_grid_inverse(Y, D, I, order=1, mode="nearest", cval=CVAL, max_iter=8, tol=SOLVER_TOL,
                                      return_valid=True)
    assert not np.isnan(Z).any()
    assert (Z.reshape(-1)[~ok] == CVAL).all() and (valid.reshape(-1)[~ok] == 0).all()
    assert (Z.reshape(-1)[ok] >= 1.0).all()
    Zi = ed.deform_grid_inverse(np.round(Y * 100).astype(np.int16), D, I, order=1, mode="nearest", cval=-7.4, max_iter=8,
                                tol=SOLVER_TOL)
    assert (Zi.reshape(-1)[~ok] == -7).all() and (Zi.reshape(-1)[ok] >= 100).all()


# ---- 4. layout ---------------------------------------------------------------------------------------------------

def _layout_case():
    I, O, D, kw, q, ok, slack = _elastic("2d-crop-mild")
    return I, O, D, kw, q


def test_step_axis_before_the_deformed_axes():
    I, O, D, kw, q = _layout_case()
    Y = _image(21, (2,) + O)
    Z = ed.deform_grid_inverse(Y, D, (2,) + I, order=3, mode="mirror", axis=(1, 2), tol=SOLVER_TOL, **kw)
    assert Z.shape == (2,) + I
    for ch in range(2):
        want = _sample(Y[ch], q, 3, "mirror").reshape(I)
        compare(Z[ch], want, None, q, O, 3, "mirror", "channel %d" % ch)


def test_step_axis_after_the_deformed_axes():
    I, O, D, kw, q = _layout_case()
    Y = _image(22, O + (3,))
    Z, valid = ed.deform_grid_inverse(Y, D, I + (3,), order=2, mode="reflect", cval=CVAL, axis=(0, 1), tol=SOLVER_TOL,
                                      return_valid=True, **kw)
    assert Z.shape == I + (3,) and valid.shape == I
    want = np_gather(prefilter(Y, 2, (0, 1)), q, 2, "reflect", CVAL).reshape(I + (3,))
    compare(Z, want, None, q, O, 2, "reflect", "steps last")


def test_non_contiguous_input():
    I, O, D, kw, q = _layout_case()
    Yt = _image(23, O[::-1])
    Y = Yt.T                                                     # a transposed view: shape O, strides reversed
    assert not Y.flags.c_contiguous
    Z = ed.deform_grid_inverse(Y, D, I, order=3, mode="mirror", tol=SOLVER_TOL, **kw)
    compare(Z, _sample(np.ascontiguousarray(Y), q, 3, "mirror").reshape(I), None, q, O, 3, "mirror", "transposed numpy")
    Zt = ed.deform_grid_inverse(torch.from_numpy(Yt).cuda().T, D, I, order=3, mode="mirror", tol=SOLVER_TOL, **kw)
    assert (Zt.cpu().numpy() == Z).all()


def test_list_of_two_inputs_with_their_own_order_and_mode():
    I, O, D, kw, q = _layout_case()
    Ya, Yb = _image(24, O), _image(25, O + (2,)).astype(np.float32)
    res = ed.deform_grid_inverse([Ya, Yb], D, [I, I + (2,)], order=[3, 1], mode=["mirror", "constant"],
                                 cval=[0.0, CVAL], axis=[(0, 1), (0, 1)], tol=SOLVER_TOL, return_valid=True, **kw)
    assert isinstance(res, list) and len(res) == 2
    (Za, va), (Zb, vb) = res
    assert (Za == ed.deform_grid_inverse(Ya, D, I, order=3, mode="mirror", tol=SOLVER_TOL, **kw)).all()
    assert (Zb == ed.deform_grid_inverse(Yb, D, I + (2,), order=1, mode="constant", cval=CVAL, axis=(0, 1),
                                         tol=SOLVER_TOL, **kw)).all()
    assert Zb.dtype == np.float32 and (va == vb).all()
    compare(Za, _sample(Ya, q, 3, "mirror").reshape(I), None, q, O, 3, "mirror", "list input 0")
    want = np_gather(Yb, q, 1, "constant", CVAL).reshape(I + (2,))
    compare(Zb, store_rule(want, np.float32), None, q, O, 1, "constant", "list input 1")


def test_prefilter_false_on_a_filtered_input_equals_prefilter_true():
    I, O, D, kw, q = _layout_case()
    Y = _image(26, O)
    Z = ed.deform_grid_inverse(Y, D, I, order=3, mode="mirror", tol=SOLVER_TOL, **kw)
    Zf = ed.deform_grid_inverse(prefilter(Y, 3, (0, 1)), D, I, order=3, mode="mirror", prefilter=False, tol=SOLVER_TOL,
                                **kw)
    assert (Z == Zf).all()


def test_numpy_in_numpy_out_tensor_in_tensor_out():
    I, O, D, kw, q = _layout_case()
    Y = _image(27, O)
    Z, valid = ed.deform_grid_inverse(Y, D, I, tol=SOLVER_TOL, return_valid=True, **kw)
    assert isinstance(Z, np.ndarray) and isinstance(valid, np.ndarray)
    Yt = torch.from_numpy(Y).cuda()
    Zt, vt = ed.deform_grid_inverse(Yt, torch.from_numpy(D).cuda(), I, tol=SOLVER_TOL, return_valid=True, **kw)
    assert torch.is_tensor(Zt) and Zt.device == Yt.device and vt.device == Yt.device and vt.dtype == torch.uint8
    assert (Zt.cpu().numpy() == Z).all() and (vt.cpu().numpy() == valid).all()


# ---- 5. batch ----------------------------------------------------------------------------------------------------

def test_batch_equals_single_calls_bit_for_bit():
    I, O, _, kw, _ = _layout_case()
    B = 3
    Ds = np.stack([_grid(40 + b, 2, (4, 5), 3.0) for b in range(B)])
    Ys = np.stack([_image(50 + b, O + (2,)) for b in range(B)]).astype(np.float32)
    args = dict(order=3, mode="constant", cval=CVAL, axis=(0, 1), tol=SOLVER_TOL, return_valid=True, **kw)
    Zb, vb = ed.deform_grid_inverse_batch(Ys, Ds, I + (2,), **args)
    assert Zb.shape == (B,) + I + (2,) and vb.shape == (B,) + I and vb.dtype == np.uint8
    for b in range(B):
        Z, v = ed.deform_grid_inverse(Ys[b], Ds[b], I + (2,), **args)
        assert (Zb[b] == Z).all() and (vb[b] == v).all()
    assert 0 < vb.sum() < vb.size


# ---- 6. the global-memory grid route ------------------------------------------------------------------------------

@pytest.mark.parametrize("order, mode", [(3, "mirror"), (1, "constant"), (0, "nearest")])
def test_global_memory_grid_route(order, mode):
    I, O, D, kw, q, ok, slack = _elastic("2d-global-grid")
    assert D.size > 7680
    Y = _image(31, O)
    Z, valid = ed.deform_grid_inverse(Y, D, I, order=order, mode=mode, cval=CVAL, tol=SOLVER_TOL, return_valid=True)
    compare(Z, _sample(Y, q, order, mode).reshape(I), None, q, O, order, mode, "global grid order %d %s" % (order, mode))
    inside = ok & ((q >= 0) & (q <= np.array(O) - 1)).all(axis=1)
    keep = ~valid_boundary_mask(q, O)
    assert (valid.reshape(-1)[keep] == inside[keep]).all()


# ---- 7. repeatability --------------------------------------------------------------------------------------------

def test_the_same_call_twice_gives_the_same_bits():
    I, O, D, kw, q, ok, slack = _elastic("3d")
    Y = _image(33, O).astype(np.float32)
    a = ed.deform_grid_inverse(Y, D, I, order=3, mode="mirror", return_valid=True)
    b = ed.deform_grid_inverse(Y, D, I, order=3, mode="mirror", return_valid=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
