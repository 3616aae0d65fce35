"""
GPU tests of the gradients of deform_grid_sample: deform_grid_sample_gradient (the adjoint in X),
deform_grid_sample_coordinate_gradient (g = dL/dr), deform_grid_sample_points_gradient (positions, displacement, inverse
map), their batch forms and autograd through elasticdeform_amd.torch.deform_grid_sample.

The reference is tests/sample_reference.py at the library's own coordinates r = ed.deform_grid_coordinates(q) (as in
test A of tests/test_sample.py: that call is held to its own reference in tests/test_points.py).

C. The adjoint in X against A^T dV, formed in long double from the reference's explicit matrix A.  The summation
   bound is that of tests/test_inverse_gradient.py: the kernel adds fl(dV[i] w_0 ... w_{n-1}) with a float atomic of the
   accumulator's type, so |got[j] - (A^T dV)[j]| <= gamma_m sum_i |A[i, j]| |dV[i]| with
   m = c_j (order + 1)^naxis + naxis + 1, c_j = #{i: A[i, j] != 0}, gamma_m = m eps / (1 - m eps), eps the accumulator's
   unit roundoff.  The reference's weights are SciPy's B-spline basis, the kernel's the closed forms of deform.c with
   "last weight = 1 - the others": for orders >= 2 each side's weight lies within 4 (order + 1) eps64 of the true one in
   ABSOLUTE terms (a few operations on values of at most 1; the last weight collects the others' errors), whatever the
   weight's size, so a product of naxis weights differs by naxis 8 (order + 1) eps64 at most and cell j by that times
   sum_i T[i, j] |dV[i]|, T[i, j] the number of taps of point i that land on cell j.  (Orders 0 and 1 have exact
   weights on both sides.)
   With the transposed prefilter the comparison is made behind it, with the bound carried through the entrywise
   absolute value of the transposed filter's matrix plus that filter's own recursion error, 8 L eps of the same
   carried sum per pass over an axis of L samples.
D. g against the reference with |err| <= 1e-10 S per element, S the same contraction with every term replaced by its
   absolute value (the convention of tests/test_points_gradient.py); the coordinates are asserted to be not within
   1e-6 of an integer, a half-integer, 0 or I_k - 1.  The point sums are checked against the reference g carried through
   the reference of tests/test_points_gradient.py (`adjoint`), under the same 1e-10 S.
"""
import numpy as np
import pytest

import sample_cases as sc
import sample_reference as sref
from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402
from test_points_gradient import adjoint as points_adjoint  # noqa: E402

EPS = {np.dtype("float64"): 2.0 ** -53, np.dtype("float32"): 2.0 ** -24}

exact_prefilter = pytest.fixture(autouse=True)(sc.exact_prefilter)


def _abs_transposed_filter(length, order):
    eye = np.eye(length)
    return np.abs(orc.spline_filter1d_grad(eye, np.zeros_like(eye), 0, order))


def _adjoint_bound(A, T, dV, shape, order, prefilter, eps):
    """the bound of C per cell of X (deformed axes only: shape = I), see the head of the file"""
    n = len(shape)
    c = (A != 0).sum(axis=0)
    m = (c * (order + 1) ** n + n + 1).astype(np.float64)
    s = np.abs(A).T @ np.abs(dV.astype(np.float64))
    bound = m * eps / (1.0 - m * eps) * s
    if order > 1:
        bound = bound + n * 8.0 * (order + 1) * 2.0 ** -53 * (T.T @ np.abs(dV.astype(np.float64)))
    bound, s = bound.reshape(shape), s.reshape(shape)
    if prefilter and order > 1:
        for d in range(n):
            F = _abs_transposed_filter(shape[d], order)
            bound = np.moveaxis(np.tensordot(F, bound, axes=([1], [d])), 0, d)
            s = np.moveaxis(np.tensordot(F, s, axes=([1], [d])), 0, d)
            bound = bound + 8.0 * shape[d] * eps * s
    return bound


# ---- C. the adjoint in X --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_adjoint_equals_the_transposed_matrix(name, order, dtype):
    I, D, kw, O = sc.case(name)
    n = len(I)
    q = sc.positions(3, O)
    r = ed.deform_grid_coordinates(q, D, I, **kw)
    dV = np.random.default_rng(13).standard_normal(len(q)).astype(dtype)
    for mode in sc.MODES:
        ref = sref.reference(np.zeros(I), r, range(n), order, mode, matrix=True)
        A = ref.A
        for prefilter in (False, True):
            got = ed.deform_grid_sample_gradient(dV, q, D, I, order=order, mode=mode, prefilter=prefilter, **kw)
            assert isinstance(got, np.ndarray) and got.shape == I and got.dtype == dtype
            want = sref.adjoint(A, dV[:, None], list(range(n)), I, order, prefilter)
            bound = _adjoint_bound(A, ref.T, dV, I, order, prefilter, EPS[np.dtype(dtype)])
            err = np.abs(got.astype(np.float64) - want)
            worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.any() else 0.0
            print("%s order %d %s %s prefilter %d: max |err| %.3g, largest share of the bound %.3g, max |want| %.3g"
                  % (name, order, np.dtype(dtype).name, mode, prefilter, err.max(), worst, np.abs(want).max()))
            assert np.abs(want).max() > 0
            assert (err <= bound).all()


def test_order_0_with_integer_cotangents_is_exact_and_repeatable():
    I, D, kw, O = sc.case("3d-affine")
    q = sc.positions(3, O)
    r = ed.deform_grid_coordinates(q, D, I, **kw)
    dV = np.random.default_rng(2).integers(-8, 9, size=len(q)).astype(np.float32)
    A = sref.reference(np.zeros(I), r, range(3), 0, "mirror", matrix=True).A
    keep = sref.boundary_distance(r, I, 0, "mirror") > sc.EDGE
    dV[~keep] = 0.0
    got = ed.deform_grid_sample_gradient(dV, q, D, I, order=0, mode="mirror", **kw)
    np.testing.assert_array_equal(got, (A.T @ dV.astype(np.float64)).reshape(I).astype(np.float32))
    np.testing.assert_array_equal(got, ed.deform_grid_sample_gradient(dV, q, D, I, order=0, mode="mirror", **kw))


# ---- D. g, and the sums over the points ---------------------------------------------------------------------------------

def _away_from_window_changes(r, I):
    I = np.asarray(I, dtype=np.float64)
    frac = np.abs(2 * r - np.round(2 * r)) / 2                  # integers and half-integers
    edge = np.minimum(np.abs(r), np.abs(r - (I - 1)))
    return (np.minimum(frac, edge) > sc.EDGE).all()


@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_g_equals_the_reference(name, order):
    I, D, kw, O = sc.case(name)
    n = len(I)
    q = sc.positions(6, O)
    r = ed.deform_grid_coordinates(q, D, I, **kw)
    assert _away_from_window_changes(r, I)
    X = sc.image(17 + n, I)
    dV = np.random.default_rng(14).standard_normal(len(q))
    for mode in sc.MODES:
        for prefilter in (True, False):
            g = ed.deform_grid_sample_coordinate_gradient(X, dV, q, D, order=order, mode=mode, prefilter=prefilter,
                                                          **kw)
            assert isinstance(g, np.ndarray) and g.shape == q.shape and g.dtype == np.float64
            ref = sref.reference(X, r, range(n), order, mode, prefilter=prefilter, dV=dV[:, None])
            err = np.abs(g - ref.g)
            share = float((err / np.maximum(1e-10 * ref.S_g, np.finfo(np.float64).tiny)).max()) if err.any() else 0.0
            print("%s order %d %s prefilter %d: max |err| %.3g, largest share of 1e-10 S %.3g"
                  % (name, order, mode, prefilter, err.max(), share))
            assert (err <= 1e-10 * ref.S_g).all()
            if order == 0:
                assert not g.any()
            if mode == "nearest":
                clamped = (r < 0) | (r > np.asarray(I, dtype=np.float64) - 1)
                assert not g[clamped].any()
            if mode == "constant":
                assert not g[ref.dead].any()


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_point_sums_equal_the_composed_references(name):
    I, D, kw, O = sc.case(name)
    n = len(I)
    q = sc.positions(6, O)
    r = ed.deform_grid_coordinates(q, D, I, **kw)
    assert _away_from_window_changes(r, I)
    X = sc.image(17 + n, I)
    dV = np.random.default_rng(15).standard_normal(len(q))
    for order, mode in ((1, "nearest"), (3, "mirror"), (3, "constant")):
        got = ed.deform_grid_sample_points_gradient(X, dV, q, D, order=order, mode=mode, **kw)
        assert isinstance(got, ed.PointsGradient) and got.points.shape == q.shape
        ref = sref.reference(X, r, range(n), order, mode, dV=dV[:, None])
        dD, dK = points_adjoint(q, ref.g, D, I, sc.offsets(kw.get("crop"), n))
        for h in range(n):
            s = ref.S_g[:, h].sum()
            err = np.abs(got.displacement[h] - dD[h]).max()
            print("%s order %d %s component %d: max |dD err| %.3g, S %.3g" % (name, order, mode, h, err, s))
            assert err <= 1e-10 * s
        bound = 1e-10 * ref.S_g.sum() * max(1.0, np.abs(q).max())
        errk = np.abs(got.inverse_map - dK).max()
        print("max |dK err| %.3g (bound %.3g)" % (errk, bound))
        assert errk <= bound
        # the rows: J^T g, the call deform_grid_coordinates_gradient makes of the library's own g
        g = ed.deform_grid_sample_coordinate_gradient(X, dV, q, D, order=order, mode=mode, **kw)
        direct = ed.deform_grid_coordinates_gradient(q, g, D, I, **kw)
        np.testing.assert_array_equal(got.points, direct.points)
        np.testing.assert_array_equal(got.displacement, direct.displacement)
        np.testing.assert_array_equal(got.inverse_map, direct.inverse_map)


def test_positions_that_are_not_sane_contribute_nothing():
    I, D, kw, O = sc.case("3d-affine")
    q = sc.positions(4, O)[:64]
    bad = np.arange(0, 64, 4)
    q[bad[0::3], 0] = np.nan
    q[bad[1::3], 2] = np.inf
    q[bad[2::3], 1] = 1e17
    good = np.setdiff1d(np.arange(64), bad)
    X = sc.image(5, I)
    dV = np.random.default_rng(1).standard_normal(64)
    for mode in ("mirror", "constant"):
        g = ed.deform_grid_sample_coordinate_gradient(X, dV, q, D, mode=mode, **kw)
        assert not g[bad].any()
        np.testing.assert_array_equal(g[good], ed.deform_grid_sample_coordinate_gradient(X, dV[good], q[good], D,
                                                                                         mode=mode, **kw))
        dX = ed.deform_grid_sample_gradient(dV.round(), q, D, I, order=0, mode=mode, **kw)
        np.testing.assert_array_equal(dX, ed.deform_grid_sample_gradient(dV[good].round(), q[good], D, I, order=0,
                                                                         mode=mode, **kw))


# ---- contracts ---------------------------------------------------------------------------------------------------------

def _contract_case(name="3d-affine"):
    I, D, kw, O = sc.case(name)
    q = sc.positions(8, O)
    return I, D, kw, q, sc.image(9, I), np.random.default_rng(10).standard_normal(len(q))


def _adjoint_check(got, dV, q, D, I, kw, order, mode):
    """got within the bound of C of the matrix at the library's coordinates"""
    r = ed.deform_grid_coordinates(q, D, I, **kw)
    ref = sref.reference(np.zeros(I), r, range(len(I)), order, mode, matrix=True)
    want = sref.adjoint(ref.A, dV[:, None], list(range(len(I))), I, order, True)
    assert (np.abs(got - want) <= _adjoint_bound(ref.A, ref.T, dV, I, order, True, EPS[np.dtype(got.dtype)])).all()


@pytest.mark.parametrize("name", ["2d-crop", "3d-affine", "2d-global-grid"])
def test_a_sample_of_a_batch_equals_the_single_call(name):
    I, D, kw, O = sc.case(name)
    B = 3
    rng = np.random.default_rng(12)
    Xs = rng.uniform(size=(B,) + I)
    Ds = np.stack([D * s for s in (1.0, 0.5, -0.7)])
    qs = np.stack([sc.positions(20 + b, O)[:257] for b in range(B)])
    dVs = rng.standard_normal((B, 257))
    g = ed.deform_grid_sample_coordinate_gradient_batch(Xs, dVs, qs, Ds, mode="mirror", **kw)
    pg = ed.deform_grid_sample_points_gradient_batch(Xs, dVs, qs, Ds, mode="mirror", **kw)
    dX = ed.deform_grid_sample_gradient_batch(dVs, qs, Ds, I, mode="mirror", **kw)
    assert g.shape == qs.shape and dX.shape == Xs.shape and pg.displacement.shape == Ds.shape
    dk = np.zeros((len(I), len(I) + 1))
    for b in range(B):
        np.testing.assert_array_equal(g[b], ed.deform_grid_sample_coordinate_gradient(Xs[b], dVs[b], qs[b], Ds[b],
                                                                                      mode="mirror", **kw))
        one = ed.deform_grid_sample_points_gradient(Xs[b], dVs[b], qs[b], Ds[b], mode="mirror", **kw)
        np.testing.assert_array_equal(pg.points[b], one.points)
        np.testing.assert_array_equal(pg.displacement[b], one.displacement)
        dk = dk + one.inverse_map
        _adjoint_check(dX[b], dVs[b], qs[b], Ds[b], I, kw, 3, "mirror")
    np.testing.assert_array_equal(pg.inverse_map, dk)


def test_repeats_slices_and_permutations():
    I, D, kw, q, X, dV = _contract_case()
    g = ed.deform_grid_sample_coordinate_gradient(X, dV, q, D, mode="reflect", **kw)
    np.testing.assert_array_equal(g, ed.deform_grid_sample_coordinate_gradient(X, dV, q, D, mode="reflect", **kw))
    np.testing.assert_array_equal(g[100:377], ed.deform_grid_sample_coordinate_gradient(X, dV[100:377], q[100:377], D,
                                                                                        mode="reflect", **kw))
    perm = np.random.default_rng(1).permutation(len(q))
    np.testing.assert_array_equal(g[perm], ed.deform_grid_sample_coordinate_gradient(X, dV[perm], q[perm], D,
                                                                                     mode="reflect", **kw))
    a = ed.deform_grid_sample_points_gradient(X, dV, q, D, mode="reflect", **kw)
    b = ed.deform_grid_sample_points_gradient(X, dV[perm], q[perm], D, mode="reflect", **kw)
    np.testing.assert_array_equal(a.displacement, b.displacement)
    np.testing.assert_array_equal(a.inverse_map, b.inverse_map)
    np.testing.assert_array_equal(a.points[perm], b.points)
    # dX: float atomics -- a repeat and a permutation agree within the bound of C
    for qq, vv in ((q, dV), (q[perm], dV[perm])):
        _adjoint_check(ed.deform_grid_sample_gradient(vv, qq, D, I, mode="reflect", **kw), dV, q, D, I, kw, 3, "reflect")


def test_channels_strides_and_a_list_of_inputs():
    I, D, kw, O = sc.case("2d-crop")
    q = sc.positions(8, O)
    rng = np.random.default_rng(3)
    X = rng.uniform(size=(2,) + I + (3,))
    dV = rng.standard_normal((2, 3, len(q)))
    g = ed.deform_grid_sample_coordinate_gradient(X, dV, q, D, mode="nearest", axis=(1, 2), **kw)
    dX = ed.deform_grid_sample_gradient(dV, q, D, X.shape, mode="nearest", axis=(1, 2), **kw)
    assert dX.shape == X.shape
    total = np.zeros(q.shape)
    for c in range(2):
        for d in range(3):
            total = total + ed.deform_grid_sample_coordinate_gradient(X[c, :, :, d], dV[c, d], q, D, mode="nearest",
                                                                      **kw)
            _adjoint_check(dX[c, :, :, d], dV[c, d], q, D, I, kw, 3, "nearest")
    scale = np.abs(total).max()
    assert np.abs(g - total).max() <= 1e-13 * scale             # (the same terms, the channels added in another order)
    # non-contiguous cotangent and positions
    wide = np.zeros((len(q), 5))
    wide[:, 1:4:2] = q
    np.testing.assert_array_equal(g, ed.deform_grid_sample_coordinate_gradient(
        X, np.moveaxis(np.ascontiguousarray(np.moveaxis(dV, -1, 0)), 0, -1), wide[:, 1:4:2], D, mode="nearest",
        axis=(1, 2), **kw))
    # a list: an order-3 image and an order-1 image; the rows add in input order
    Y = rng.uniform(size=I)
    dY = rng.standard_normal(len(q))
    both = ed.deform_grid_sample_coordinate_gradient([X[0, :, :, 0], Y], [dV[0, 0], dY], q, D, order=[3, 1],
                                                     mode=["nearest", "mirror"], **kw)
    parts = (ed.deform_grid_sample_coordinate_gradient(X[0, :, :, 0], dV[0, 0], q, D, order=3, mode="nearest", **kw)
             + ed.deform_grid_sample_coordinate_gradient(Y, dY, q, D, order=1, mode="mirror", **kw))
    np.testing.assert_array_equal(both, parts)
    dXs = ed.deform_grid_sample_gradient([dV[0, 0], dY], q, D, I, order=[3, 1], mode=["nearest", "mirror"], **kw)
    assert isinstance(dXs, list) and len(dXs) == 2
    _adjoint_check(dXs[1], dY, q, D, I, kw, 1, "mirror")


def test_array_families_float32_and_no_points():
    I, D, kw, q, X, dV = _contract_case()
    Xt, qt, Dt, Vt = (torch.from_numpy(a).cuda() for a in (X, q, D, dV))
    g = ed.deform_grid_sample_coordinate_gradient(X, dV, q, D, **kw)
    gt = ed.deform_grid_sample_coordinate_gradient(Xt, Vt, qt, Dt, **kw)
    assert torch.is_tensor(gt) and gt.is_cuda
    np.testing.assert_array_equal(g, gt.cpu().numpy())
    dXt = ed.deform_grid_sample_gradient(Vt.float(), qt, Dt, I, **kw)
    assert torch.is_tensor(dXt) and dXt.dtype == torch.float32 and tuple(dXt.shape) == I
    # float32 arrays are widened at the load: the rows of the same values in float64
    X32, V32 = X.astype(np.float32), dV.astype(np.float32)
    np.testing.assert_array_equal(
        ed.deform_grid_sample_coordinate_gradient(X32, V32, q, D, order=1, **kw),
        ed.deform_grid_sample_coordinate_gradient(X32.astype(np.float64), V32.astype(np.float64), q, D, order=1, **kw))
    assert ed.deform_grid_sample_coordinate_gradient(X, dV[:0], q[:0], D, **kw).shape == (0, 3)
    assert not ed.deform_grid_sample_gradient(dV[:0], q[:0], D, I, **kw).any()
    none = ed.deform_grid_sample_points_gradient(X, dV[:0], q[:0], D, **kw)
    assert none.points.shape == (0, 3) and not none.displacement.any() and not none.inverse_map.any()


def test_more_points_than_the_launch_covers():
    I, D, kw, O = sc.case("1d")
    N = 2048 * 256 + 77
    gen = torch.Generator(device="cuda").manual_seed(5)
    q = torch.rand((N, 1), generator=gen, device="cuda", dtype=torch.float64) * (O[0] + 3) - 2
    dV = torch.rand((N,), generator=gen, device="cuda", dtype=torch.float64) - 0.5
    X = torch.from_numpy(sc.image(2, I)).cuda()
    Dt = torch.from_numpy(D).cuda()
    g = ed.deform_grid_sample_coordinate_gradient(X, dV, q, Dt, mode="mirror")
    tail = slice(N - 1500, N)
    assert torch.equal(g[tail], ed.deform_grid_sample_coordinate_gradient(X, dV[tail], q[tail], Dt, mode="mirror"))
    # order 0, unit cotangents: every point adds 1 to one cell
    ones = torch.ones((N,), device="cuda", dtype=torch.float32)
    dX = ed.deform_grid_sample_gradient(ones, q, Dt, I, order=0, mode="mirror")
    assert float(dX.sum()) == N


def test_capture_into_a_graph():
    I, D, kw, q, X, dV = _contract_case()
    Xt, qt, Dt, Vt = (torch.from_numpy(a).cuda() for a in (X, q, D, dV))

    def run():
        return (ed.deform_grid_sample_coordinate_gradient(Xt, Vt, qt, Dt, mode="mirror", **kw),
                ed.deform_grid_sample_gradient(Vt, qt, Dt, I, mode="mirror", **kw),
                ed.deform_grid_sample_points_gradient(Xt, Vt, qt, Dt, mode="mirror", **kw))
    g0, _, pg0 = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                   # the filters and the point sums size that stream's workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g, dX, pg = run()
    I2, D2, kw2, O2 = sc.case("2d-crop")
    for _ in range(3):
        g.zero_()
        ed.deform_grid_sample_coordinate_gradient(sc.image(1, I2), np.ones(50), sc.positions(2, O2)[:50], D2, **kw2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g, g0) and torch.equal(pg.displacement, pg0.displacement)
        assert torch.equal(pg.inverse_map, pg0.inverse_map) and torch.equal(pg.points, pg0.points)
        _adjoint_check(dX.cpu().numpy(), dV, q, D, I, kw, 3, "mirror")


# ---- autograd --------------------------------------------------------------------------------------------------------

def test_autograd_gives_the_direct_calls():
    I, D, kw, q, X, dV = _contract_case()
    Xt = torch.from_numpy(X).cuda().requires_grad_()
    qt = torch.from_numpy(q).cuda().requires_grad_()
    Dt = torch.from_numpy(D).cuda().requires_grad_()
    At = torch.from_numpy(kw["affine"]).cuda().requires_grad_()
    Vt = torch.from_numpy(dV).cuda()
    V = etorch.deform_grid_sample(Xt, qt, Dt, mode="mirror", affine=At, displacement_grad=True, affine_grad=True)
    assert V.grad_fn is not None
    (V * Vt).sum().backward()
    # (device tensors in: the chain from dK to the affine runs where the autograd backward runs it)
    pg = ed.deform_grid_sample_points_gradient(Xt.detach(), Vt, qt.detach(), Dt.detach(), mode="mirror", **kw)
    assert torch.equal(qt.grad, pg.points) and torch.equal(Dt.grad, pg.displacement)
    np.testing.assert_array_equal(At.grad.cpu().numpy(), pg.affine.cpu().numpy())
    np.testing.assert_array_equal(pg.points.cpu().numpy(),
                                  ed.deform_grid_sample_points_gradient(X, dV, q, D, mode="mirror", **kw).points)
    _adjoint_check(Xt.grad.cpu().numpy(), dV, q, D, I, kw, 3, "mirror")
    # the switches: without them the displacement and the map get nothing
    Dt.grad = None
    V = etorch.deform_grid_sample(Xt, qt, Dt, mode="mirror", affine=At)
    V.sum().backward()
    assert Dt.grad is None
    # a list: each input's gradient flows
    Yt = torch.from_numpy(X[::-1].copy()).cuda().requires_grad_()
    a, b = etorch.deform_grid_sample([Xt.detach(), Yt], qt.detach(), Dt.detach(), order=[3, 1], mode="mirror", **kw)
    assert a.grad_fn is None or not a.requires_grad
    b.sum().backward()
    assert Yt.grad is not None and Yt.grad.abs().sum() > 0


def test_with_nothing_requiring_grad_nothing_changes():
    I, D, kw, q, X, dV = _contract_case()
    V = etorch.deform_grid_sample(X, q, D, mode="mirror", **kw)
    assert isinstance(V, np.ndarray)
    np.testing.assert_array_equal(V, ed.deform_grid_sample(X, q, D, mode="mirror", **kw))
    Xt, qt, Dt = (torch.from_numpy(a).cuda() for a in (X, q, D))
    Vt = etorch.deform_grid_sample(Xt, qt, Dt.requires_grad_(), mode="mirror", **kw)     # (no displacement_grad)
    assert Vt.grad_fn is None and not Vt.requires_grad
    np.testing.assert_array_equal(V, Vt.cpu().numpy())


@pytest.mark.parametrize("mode", ["mirror", "nearest"])
@pytest.mark.parametrize("order", [1, 3])
def test_gradcheck(order, mode):
    """float64 on (7, 8), 12 points kept away from the window changes of order 1 and from the clamp of 'nearest'.
    nondet_tol: dX comes from float atomics -- the bound of C for a unit cotangent, a row of A summing to 1 in absolute
    value at most 3 times over"""
    I = (7, 8)
    rng = np.random.default_rng(4)
    D = rng.standard_normal((2, 3, 3)) * 0.4
    X = torch.from_numpy(rng.uniform(size=I)).cuda().requires_grad_()
    q0 = rng.uniform(1.2, 4.8, size=(400, 2))
    r = ed.deform_grid_coordinates(q0, D, I)
    far = (np.abs(r - np.round(r)) > 0.05).all(1) & (r > 0.3).all(1) & (r < np.array(I) - 1.3).all(1)
    assert far.sum() >= 12
    q = torch.from_numpy(q0[far][:12]).cuda().requires_grad_()
    Dt = torch.from_numpy(D).cuda().requires_grad_()
    m = 12 * (order + 1) ** 2 + 3
    nondet = 3.0 * m * 2.0 ** -53 / (1.0 - m * 2.0 ** -53)

    def f(x, p, d):
        return etorch.deform_grid_sample(x, p, d, order=order, mode=mode, displacement_grad=True)
    assert torch.autograd.gradcheck(f, (X, q, Dt), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=nondet)
