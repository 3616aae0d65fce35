"""
GPU tests of the coordinate map at real positions and its inverse (elasticdeform_amd.deform_grid_coordinates,
deform_points, their batch forms; edhip_deform_points).

Expected values come from sources that share no code with the kernel:

* the oracle ramp: the CPU oracle deforms the coordinate ramp of axis h (numpy.indices(I)[h], float64) with order=1,
  mode='nearest' and returns clamp(r_h(o), 0, I_h - 1) at every integer o -- every voxel is compared;
* the refined lattice: the same oracle call on a ramp of extents I' = m (I - 1) + 1 with the same control grid gives
  delta_h(o' / m) = Y'[o'] - o'_h wherever 0 < Y' < I'_h - 1 (m = 3);
* a NumPy restatement of the formulas (`restate` below; scipy.ndimage.spline_filter1d(order=3, mode='mirror') as the
  prefilter), used at random real positions, for the Jacobian and to verify the inverse.

Tolerance for coordinates: 1e-10 absolute (coordinates and coefficients below 1e3; both sides are fp64 sums of at
most 4^n terms and the two CPU sources agree to 1.6e-14; a wrong tap, weight or offset shows at 1e-3 or more).
"""
import numpy as np
import pytest

from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402

TOL = 1e-10


# ---- the NumPy restatement (oracle/dgrad_reference.py, shared with the gradient tests) ----------------------------

from oracle.dgrad_reference import coordinate as restate  # noqa: E402


def restate_jacobian(q, D, I, off=None, K=None, h=1e-4):
    """central differences of the restatement: (N, n, n), J[:, a, l] = d r_a / d q_l"""
    n = D.shape[0]
    J = np.zeros((q.shape[0], n, n))
    for l in range(n):
        e = np.zeros(n)
        e[l] = h
        J[:, :, l] = (restate(q + e, D, I, off, K) - restate(q - e, D, I, off, K)) / (2 * h)
    return J


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


def _random_positions(seed, O, count):
    """real positions from one extent below 0 to one extent above O - 1 on every axis"""
    rng = np.random.default_rng(seed)
    O = np.asarray(O, dtype=np.float64)
    return rng.uniform(-O, 2 * O - 1, size=(count, len(O)))


AFFINE2 = np.array([[1.1, 0.15, -1.5], [-0.1, 0.9, 2.0]])
AFFINE3 = np.array([[1.05, 0.1, 0.0, -1.0], [-0.08, 0.95, 0.05, 0.5], [0.02, -0.04, 1.1, 1.5]])


# ---- 1. forward, integer lattice, against the oracle ramp ------------------------------------------------------

LATTICE = [((40,), (5,), None, 2.0), ((13, 17), (4, 5), (slice(2, 11), slice(3, 15)), 3.0),
           ((12, 14, 10), (4, 4, 5), None, 1.5)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int16])
@pytest.mark.parametrize("I, ncp, crop, sigma", LATTICE, ids=["1d", "2d-crop", "3d"])
def test_forward_integer_lattice_equals_the_oracle_ramp(I, ncp, crop, sigma, dtype):
    n = len(I)
    D = _grid(11 + n, n, ncp, sigma, dtype)
    O = _out_shape(I, crop)
    lattice = np.stack(np.indices(O), axis=-1)                   # integer positions, taken as float64
    r = ed.deform_grid_coordinates(lattice, D, I, crop=crop)
    assert r.shape == O + (n,) and r.dtype == np.float64
    for h in range(n):
        ramp = np.indices(I)[h].astype(np.float64)
        want = orc.deform_grid(ramp, D, order=1, mode="nearest", crop=crop)
        err = np.abs(np.clip(r[..., h], 0, I[h] - 1) - want).max()
        print("axis %d: max |err| %.3g" % (h, err))
        assert err <= TOL


# ---- 2. forward, fractional positions, against the refined lattice ---------------------------------------------

@pytest.mark.parametrize("I, ncp, sigma", [((13, 17), (4, 5), 3.0), ((12, 14, 10), (4, 4, 5), 1.5)], ids=["2d", "3d"])
def test_forward_fractional_positions_equal_the_refined_lattice(I, ncp, sigma):
    n, m = len(I), 3
    D = _grid(21 + n, n, ncp, sigma)
    If = tuple(m * (i - 1) + 1 for i in I)
    fine = np.stack(np.indices(If), axis=-1).astype(np.float64)
    q = fine / m
    r = ed.deform_grid_coordinates(q, D, I)
    compared = total = 0
    for h in range(n):
        Yf = orc.deform_grid(np.indices(If)[h].astype(np.float64), D, order=1, mode="nearest")
        # (a clamped voxel interpolates the ramp's last value with weights that sum to 1 - 1e-16: it can come out an
        # ulp or two inside the bound, so "strictly inside" is taken with a margin far above that and far below TOL's
        # meaning for the comparison)
        inside = (Yf > 1e-9) & (Yf < If[h] - 1 - 1e-9)
        want = Yf - fine[..., h]                                 # delta_h(o' / m)
        got = r[..., h] - q[..., h]
        err = np.abs(got - want)[inside].max()
        print("axis %d: max |err| %.3g over %d of %d" % (h, err, inside.sum(), inside.size))
        assert err <= TOL
        compared += int(inside.sum())
        total += inside.size
    assert compared >= 0.8 * total


# ---- 3. forward, random real positions, against the restatement -------------------------------------------------

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
    "2d-global-grid": dict(I=(70, 70), ncp=(64, 64), sigma=0.5),   # 2 x 64 x 64 = 8192 values: read from global memory
    "1d-short-grid": dict(I=(9,), ncp=(2,), sigma=1.0),            # two control points: every window is mirrored
}


def _case(name):
    c = dict(RANDOM[name])
    I, ncp, sigma = c.pop("I"), c.pop("ncp"), c.pop("sigma")
    D = _grid(31 + len(name), len(I), ncp, sigma)
    return I, D, c


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_forward_random_positions_equal_the_restatement(name):
    I, D, kw = _case(name)
    O = _out_shape(I, kw.get("crop"))
    q = _random_positions(5, O, 600)
    r = ed.deform_grid_coordinates(q, D, I, **kw)
    want = restate(q, D, I, _offsets(kw.get("crop"), len(I)), _K(I, **kw))
    err = np.abs(r - want).max()
    print("%s: max |err| %.3g" % (name, err))
    assert r.shape == q.shape and err <= TOL


@pytest.mark.parametrize("name", ["2d-crop", "3d-affine", "2d-global-grid"])
def test_float32_positions_round_once(name):
    """float32 positions: the float64 result of the same (float32-valued) positions, rounded once"""
    I, D, kw = _case(name)
    q32 = _random_positions(6, _out_shape(I, kw.get("crop")), 500).astype(np.float32)
    r32 = ed.deform_grid_coordinates(q32, D, I, **kw)
    r64 = ed.deform_grid_coordinates(q32.astype(np.float64), D, I, **kw)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    np.testing.assert_array_equal(r32, r64.astype(np.float32))
    p32, ok32 = ed.deform_points(r32, D, I, return_converged=True, **kw)
    p64, ok64 = ed.deform_points(r32.astype(np.float64), D, I, return_converged=True, **kw)
    assert p32.dtype == np.float32
    np.testing.assert_array_equal(ok32, ok64)
    np.testing.assert_array_equal(p32, p64.astype(np.float32))


# ---- 4. the Jacobian --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["1d", "2d", "3d", "4d-generic", "2d-crop", "3d-affine", "2d-rotate-zoom-crop",
                                  "2d-global-grid"])
def test_jacobian_equals_central_differences_of_the_restatement(name):
    I, D, kw = _case(name)
    O = _out_shape(I, kw.get("crop"))
    q = _random_positions(7, O, 300)
    r, J = ed.deform_grid_coordinates(q, D, I, jacobian=True, **kw)
    n = len(I)
    assert J.shape == (300, n, n) and J.dtype == np.float64
    np.testing.assert_array_equal(r, ed.deform_grid_coordinates(q, D, I, **kw))
    want = restate_jacobian(q, D, I, _offsets(kw.get("crop"), n), _K(I, **kw))
    err = np.abs(J - want).max()
    print("%s: max |J err| %.3g, |J|max %.3g" % (name, err, np.abs(want).max()))
    assert err <= 1e-6 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_jacobian_of_a_zero_grid(n):
    I = (6, 7, 8, 9)[:n]
    D = np.zeros((n,) + (3,) * n)
    q = _random_positions(8, I, 50)
    r, J = ed.deform_grid_coordinates(q, D, I, jacobian=True)
    assert np.abs(J - np.eye(n)).max() <= 1e-12 and np.abs(r - q).max() <= 1e-12
    if n in (2, 3):
        A = AFFINE2 if n == 2 else AFFINE3
        r, J = ed.deform_grid_coordinates(q, D, I, affine=A, jacobian=True)
        K = _K(I, affine=A)
        assert np.abs(J - K[:, :n]).max() <= 1e-12
        assert np.abs(r - (q @ K[:, :n].T + K[:, n])).max() <= 1e-10


# ---- 5. inverse, invertible fields ------------------------------------------------------------------------------

INVERTIBLE = {
    "2d": dict(I=(40, 52), ncp=(5, 5), sigma=2.0, seed=12),
    "2d-crop-affine": dict(I=(40, 52), ncp=(5, 5), sigma=2.0, seed=12, crop=(slice(4, 36), slice(6, 50)),
                           affine=AFFINE2),
    "3d": dict(I=(24, 28, 20), ncp=(4, 4, 4), sigma=0.5, seed=4),
    "3d-crop-affine": dict(I=(24, 28, 20), ncp=(4, 4, 4), sigma=0.5, seed=4,
                           crop=(slice(2, 22), slice(3, 27), slice(0, 18)), affine=AFFINE3),
}


@pytest.mark.parametrize("name", sorted(INVERTIBLE))
def test_inverse_on_invertible_fields(name):
    c = dict(INVERTIBLE[name])
    I, ncp, sigma, seed = c.pop("I"), c.pop("ncp"), c.pop("sigma"), c.pop("seed")
    n = len(I)
    D = np.random.default_rng(seed).standard_normal((n,) + ncp) * sigma
    O = _out_shape(I, c.get("crop"))
    off, K = _offsets(c.get("crop"), n), _K(I, **c)
    # the field does not fold: det J > 0.2 on a 12-per-axis lattice of the output (from the restatement)
    lat = np.stack(np.meshgrid(*[np.linspace(0, o - 1, 12) for o in O], indexing="ij"), axis=-1).reshape(-1, n)
    det = np.linalg.det(restate_jacobian(lat, D, I, off, K))
    print("%s: min det J %.3f" % (name, det.min()))
    assert det.min() > 0.2
    # source points that land inside the output: the images of random output positions, and a few anywhere in X
    rng = np.random.default_rng(9)
    q0 = rng.uniform(0, np.asarray(O, dtype=np.float64) - 1, size=(800, n))
    p = np.concatenate([restate(q0, D, I, off, K), rng.uniform(0, np.asarray(I) - 1.0, size=(200, n))])
    q, ok = ed.deform_points(p, D, I, return_converged=True, **c)
    assert ok.dtype == np.bool_ and ok.shape == (1000,) and q.shape == p.shape
    assert ok.all()
    res = np.abs(restate(q, D, I, off, K) - p).max()
    print("%s: max residual %.3g" % (name, res))
    assert res <= 1e-9
    back = ed.deform_grid_coordinates(q, D, I, **c)
    assert np.abs(back - p).max() <= 1e-9
    assert np.abs(q[:800] - q0).max() <= 1e-7               # det J > 0.2: the pre-image is the position it came from


# ---- 6. inverse, folding field ----------------------------------------------------------------------------------

def test_inverse_on_a_folding_field():
    I, n = (32, 32), 2
    D = np.random.default_rng(5).standard_normal((2, 5, 5)) * 6.0
    lat = np.stack(np.meshgrid(*[np.linspace(0, i - 1, 12) for i in I], indexing="ij"), axis=-1).reshape(-1, n)
    assert np.linalg.det(restate_jacobian(lat, D, I)).min() < 0        # it folds
    p = np.random.default_rng(10).uniform(0, 31, size=(1500, 2))
    q, ok = ed.deform_points(p, D, I, return_converged=True)
    assert ok.dtype == np.bool_ and ok.shape == (1500,)
    print("solved %d of %d" % (ok.sum(), ok.size))
    if ok.any():
        assert np.abs(restate(q[ok], D, I) - p[ok]).max() <= 1e-9
    assert np.isnan(q[~ok]).all() and np.isfinite(q[ok]).all()
    # without the mask: the same coordinates
    np.testing.assert_array_equal(ed.deform_points(p, D, I), q)
    # non-finite points are not solved; one step is not enough for a point away from its start
    bad = np.array([[np.nan, 3.0], [4.0, np.inf], [5.0, 6.0]])
    qb, okb = ed.deform_points(bad, D, I, return_converged=True)
    assert not okb[0] and not okb[1] and np.isnan(qb[:2]).all()
    q1, ok1 = ed.deform_points(p, D, I, max_iter=1, return_converged=True)
    assert ok1.sum() < ok.sum() and np.isnan(q1[~ok1]).all()
    assert np.abs(restate(q1[ok1], D, I) - p[ok1]).max() <= 1e-9 if ok1.any() else True


# ---- 7. a landmark, end to end ----------------------------------------------------------------------------------

def _blob(I, p, s=1.5):
    grids = np.indices(I).astype(np.float64)
    return np.exp(-sum((g - c) ** 2 for g, c in zip(grids, p)) / (2 * s * s))


@pytest.mark.parametrize("I, p, points, kw", [
    ((48, 56), (20.3, 30.6), 3, {}),
    ((48, 56), (25.2, 24.7), 3, dict(rotate=20, zoom=1.3)),
    ((48, 56), (22.4, 31.1), 3, dict(crop=(slice(5, 43), slice(8, 50)))),
    ((48, 56), (24.6, 27.3), 3, dict(rotate=20, zoom=1.3, crop=(slice(5, 43), slice(8, 50)))),
    ((24, 28, 20), (11.2, 14.7, 9.4), 3, {}),
    ((24, 28, 20), (12.3, 13.1, 10.2), 3, dict(crop=(slice(2, 22), slice(3, 25), slice(1, 19)))),
], ids=["2d", "2d-rotate-zoom", "2d-crop", "2d-rotate-zoom-crop", "3d", "3d-crop"])
def test_landmark_follows_the_image(I, p, points, kw):
    n = len(I)
    sigma = 0.2 * (min(I) - 1) / (points - 1)                    # relative strength sigma (points - 1) / (extent - 1) ~ 0.2
    D = np.random.default_rng(12).standard_normal((n,) + (points,) * n) * sigma
    X = _blob(I, p)
    Y = ed.deform_grid(X, D, order=3, mode="constant", **kw)
    q, ok = ed.deform_points(np.array(p), D, I, return_converged=True, **kw)
    assert q.shape == (n,) and ok.shape == () and bool(ok)
    peak = np.array(np.unravel_index(np.argmax(Y), Y.shape), dtype=np.float64)
    print("landmark %s -> %s, argmax %s" % (p, q, peak))
    assert Y.max() > 0.3                                         # the blob is inside the output
    assert np.abs(peak - q).max() <= 1.0


# ---- 8. contracts -----------------------------------------------------------------------------------------------

def _contract_case():
    I = (13, 17)
    D = _grid(41, 2, (4, 5), 1.5)
    q = _random_positions(13, I, 700)
    return I, D, q, dict(crop=(slice(1, 12), slice(2, 16)), affine=AFFINE2)


def test_batch_sample_equals_the_single_call():
    I, D, q, kw = _contract_case()
    Db = np.stack([D, -0.5 * D, _grid(42, 2, (4, 5), 1.0)])
    qb = np.stack([q, q[::-1], 0.5 * q])
    rb, Jb = ed.deform_grid_coordinates_batch(qb, Db, I, jacobian=True, **kw)
    pb, okb = ed.deform_points_batch(qb, Db, I, return_converged=True, **kw)
    assert rb.shape == (3, 700, 2) and Jb.shape == (3, 700, 2, 2) and okb.shape == (3, 700) and okb.dtype == np.bool_
    for b in range(3):
        r, J = ed.deform_grid_coordinates(qb[b], Db[b], I, jacobian=True, **kw)
        p, ok = ed.deform_points(qb[b], Db[b], I, return_converged=True, **kw)
        np.testing.assert_array_equal(rb[b], r)
        np.testing.assert_array_equal(Jb[b], J)
        np.testing.assert_array_equal(pb[b], p)
        np.testing.assert_array_equal(okb[b], ok)
    assert not np.array_equal(rb[0], rb[1][::-1])                # the grids are distinct
    np.testing.assert_array_equal(ed.deform_grid_coordinates_batch(qb, Db, I, **kw), rb)
    np.testing.assert_array_equal(ed.deform_points_batch(qb, Db, I, **kw), pb)


def test_slices_repeats_and_views_give_the_same_bits():
    I, D, q, kw = _contract_case()
    r, J = ed.deform_grid_coordinates(q, D, I, jacobian=True, **kw)
    p, ok = ed.deform_points(q, D, I, return_converged=True, **kw)
    # a slice of the points: the same rows
    rs, Js = ed.deform_grid_coordinates(q[300:437], D, I, jacobian=True, **kw)
    ps = ed.deform_points(q[300:437], D, I, **kw)
    np.testing.assert_array_equal(rs, r[300:437])
    np.testing.assert_array_equal(Js, J[300:437])
    np.testing.assert_array_equal(ps, p[300:437])
    # a second call
    np.testing.assert_array_equal(ed.deform_grid_coordinates(q, D, I, **kw), r)
    np.testing.assert_array_equal(ed.deform_points(q, D, I, **kw), p)
    # a transposed (non-contiguous) view, numpy and on the device
    qt = np.ascontiguousarray(q.T).T
    assert not qt.flags.c_contiguous
    np.testing.assert_array_equal(ed.deform_grid_coordinates(qt, D, I, **kw), r)
    np.testing.assert_array_equal(ed.deform_points(qt, D, I, **kw), p)
    tt = torch.from_numpy(np.ascontiguousarray(q.T)).cuda().t()
    assert not tt.is_contiguous()
    np.testing.assert_array_equal(ed.deform_grid_coordinates(tt, torch.from_numpy(D).cuda(), I, **kw).cpu().numpy(), r)
    np.testing.assert_array_equal(ed.deform_points(tt, torch.from_numpy(D).cuda(), I, **kw).cpu().numpy(), p)
    # leading dimensions are flattened and restored
    r3 = ed.deform_grid_coordinates(q.reshape(7, 100, 2), D, I, **kw)
    p3, ok3 = ed.deform_points(q.reshape(7, 100, 2), D, I, return_converged=True, **kw)
    np.testing.assert_array_equal(r3, r.reshape(7, 100, 2))
    np.testing.assert_array_equal(p3, p.reshape(7, 100, 2))
    np.testing.assert_array_equal(ok3, ok.reshape(7, 100))


def test_array_families_and_devices():
    I, D, q, kw = _contract_case()
    r = ed.deform_grid_coordinates(q, D, I, **kw)
    assert isinstance(r, np.ndarray)
    qt, Dt = torch.from_numpy(q).cuda(), torch.from_numpy(D).cuda()
    rt, Jt = etorch.deform_grid_coordinates(qt, Dt, I, jacobian=True, **kw)
    pt, okt = etorch.deform_points(qt, Dt, I, return_converged=True, **kw)
    for t in (rt, Jt, pt, okt):
        assert torch.is_tensor(t) and t.device == qt.device
    assert okt.dtype == torch.bool and Jt.dtype == torch.float64 and not rt.requires_grad
    np.testing.assert_array_equal(rt.cpu().numpy(), r)
    # numpy points with a device grid stay numpy; a CPU tensor comes back as a CPU tensor
    assert isinstance(ed.deform_grid_coordinates(q, Dt, I, **kw), np.ndarray)
    rc = ed.deform_grid_coordinates(torch.from_numpy(q), D, I, **kw)
    assert torch.is_tensor(rc) and rc.device.type == "cpu"
    np.testing.assert_array_equal(rc.numpy(), r)
    # the batch names are re-exported too
    assert etorch.deform_points_batch is ed.deform_points_batch
    assert etorch.deform_grid_coordinates_batch is ed.deform_grid_coordinates_batch


def test_no_points():
    I, D, q, kw = _contract_case()
    r, J = ed.deform_grid_coordinates(q[:0], D, I, jacobian=True, **kw)
    p, ok = ed.deform_points(q[:0], D, I, return_converged=True, **kw)
    assert r.shape == (0, 2) and J.shape == (0, 2, 2) and p.shape == (0, 2) and ok.shape == (0,)
    rb = ed.deform_grid_coordinates_batch(np.zeros((2, 0, 2)), np.stack([D, D]), I, **kw)
    assert rb.shape == (2, 0, 2)
    rt = ed.deform_grid_coordinates(torch.zeros((0, 2), dtype=torch.float32, device="cuda"), D, I, **kw)
    assert tuple(rt.shape) == (0, 2) and rt.dtype == torch.float32


def test_length_one_axis_gives_nan():
    D = np.zeros((2, 3, 3))
    qt = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    p, ok = ed.deform_points(qt, D, (1, 9), return_converged=True)
    assert p.device == qt.device and ok.device == qt.device and ok.dtype == torch.bool
    assert torch.isnan(p).all() and not ok.any()
    r, J = ed.deform_grid_coordinates(qt, D, (9, 1), jacobian=True)
    assert torch.isnan(r).all() and torch.isnan(J).all() and tuple(J.shape) == (4, 2, 2)


def test_more_points_than_one_launch_covers():
    """the grid-stride loop: more points than blocks x threads of one launch (2048 x 256); the last rows equal a
    call on those rows alone, the first ones the restatement"""
    I, D = (40,), _grid(43, 1, (5,), 2.0)
    N = 2048 * 256 + 1000
    q = torch.linspace(-5.0, 50.0, N, dtype=torch.float64, device="cuda").reshape(N, 1)
    Dt = torch.from_numpy(D).cuda()
    r = ed.deform_grid_coordinates(q, Dt, I)
    p = ed.deform_points(q, Dt, I)
    assert torch.equal(r[-1500:], ed.deform_grid_coordinates(q[-1500:], Dt, I))
    assert torch.equal(torch.nan_to_num(p[-1500:], nan=-1e30),
                       torch.nan_to_num(ed.deform_points(q[-1500:], Dt, I), nan=-1e30))
    pick = torch.cat([torch.arange(0, 2000, device="cuda"), torch.arange(N - 2000, N, device="cuda")])
    want = restate(q[pick].cpu().numpy(), D, I)
    assert np.abs(r[pick].cpu().numpy() - want).max() <= TOL


def test_capture_into_a_graph():
    """after one warm-up call, a forward and an inverse call captured in one graph on a side stream and replayed
    three times give the eager bits"""
    I, D, q, kw = _contract_case()
    qt, Dt = torch.from_numpy(q).cuda(), torch.from_numpy(D).cuda()
    r0, J0 = ed.deform_grid_coordinates(qt, Dt, I, jacobian=True, **kw)        # eager
    p0, ok0 = ed.deform_points(qt, Dt, I, return_converged=True, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the warm-up on the capture stream: the control grid's prefilter (not the points kernel) uses that stream's
        # workspace
        ed.deform_grid_coordinates(qt, Dt, I, jacobian=True, **kw)
        ed.deform_points(qt, Dt, I, return_converged=True, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        r, J = ed.deform_grid_coordinates(qt, Dt, I, jacobian=True, **kw)
        p, ok = ed.deform_points(qt, Dt, I, return_converged=True, **kw)
    for _ in range(3):
        r.zero_()
        p.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(r, r0) and torch.equal(J, J0) and torch.equal(ok, ok0)
        assert torch.equal(torch.nan_to_num(p, nan=-1e30), torch.nan_to_num(p0, nan=-1e30))
