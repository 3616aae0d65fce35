"""
GPU tests of the adjoint of the coordinate map's derivatives (elasticdeform_amd.deform_grid_derivatives_gradient, its
batch form, elasticdeform_amd.torch.deform_grid_derivatives; edhip_deform_points_derivatives_gradient).

Expected values come from tests/derivatives_reference.py (anchored against difference quotients of its own loss on the
CPU in tests/test_derivatives_reference_host.py).  Bounds, A the absolute-value sum of the entry's terms:
* displacement: 1024 eps A_D, inverse_map: 1024 eps A_K per entry, the points' rows: 512 eps A_q per component;
* affine / rotate / zoom: 1e-6 max(1, |value|), the bound of tests/test_jacobian.py.
The sums are 64-bit integer fixed point, so a repeated call, a permutation of the points, a sample of a batch and a
replayed graph give the same bits.  Cases, positions and counts: tests/derivatives_cases.py.

The grid beyond the LDS route on which every count is held to these bounds is 3 x 14^3 on 16^3.  The 2 x 64 x 64 grid
on (70, 70) is held to them with 1000 points, which reach every cell, and to every bit contract; with few points it
misses the displacement bound, and not in the new kernels: dP itself, carried through the reference's exact transposed
filter, is within 0.8 (N = 1), 21 (N = 63) and 51 (N = 257) eps A_D.  Along a 64-point axis A_D decays from the
point's cells by 0.268 per cell, over up to 70 orders of magnitude, and the library's transposed grid prefilter
(_filter_axes(transpose=True), the pass deform_grid_coordinates_gradient has always applied) resolves such a tail to the
line's largest values, not to the local one: measured 7.2e14 eps A_D at N = 1 and 6.2e4 at N = 63, 64 and 65, against
2.5 at N = 257 and 2.0 at N = 1000.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402

import derivatives_cases as cases  # noqa: E402
import jacobian_reference as jref  # noqa: E402

EPS = np.finfo(np.float64).eps
# every cotangent alone and all three on all the points; all three on every other count
PAIRS = [(which, cases.NMAX) for which in cases.WHICH] + [("all", c) for c in cases.COUNTS if c != cases.NMAX]
TRIPLES = [(name, which, count) for name in cases.NAMES for which, count in PAIRS
           if name != "2d-global-grid" or count == cases.NMAX]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _ratio(err, scale):
    """the worst err / (eps scale) over the entries with a scale; entries without one must be exact"""
    assert np.all(err[scale == 0] == 0)
    return float((err[scale > 0] / (EPS * scale[scale > 0])).max()) if np.any(scale > 0) else 0.0


def _call(name, which, count, **over):
    I, D, kw = cases.case(name)
    kw.update(over)
    return ed.deform_grid_derivatives_gradient(cases.data(name)[0][:count], D, I, **cases.cotangents(name, which, count),
                                               **kw)


@pytest.mark.parametrize("name,which,count", TRIPLES)
def test_gradients_equal_the_reference(name, which, count):
    I, D, kw = cases.case(name)
    ref = cases.reference(name, count, which)
    g = _call(name, which, count)
    assert isinstance(g, ed.PointsGradient)
    assert g.points.shape == (count, len(I)) and g.displacement.shape == D.shape and g.displacement.dtype == np.float64
    rD = _ratio(np.abs(g.displacement - ref.dD), ref.A_D)
    rK = _ratio(np.abs(g.inverse_map - ref.dK), ref.A_K)
    rq = _ratio(np.abs(g.points - ref.dq), np.where(ref.sane[:, None], ref.A_q, 0.0))
    print("%s %s N=%d: worst err / (eps A): displacement %.2f, inverse_map %.2f, points %.2f"
          % (name, which, count, rD, rK, rq))
    assert rD <= 1024 and rK <= 1024 and rq <= 512
    # points that contribute nothing: zero rows
    assert not g.points[~ref.sane].any()
    # affine / rotate / zoom from the reference's dK by the reference's own matrix algebra
    want = jref.parameter_gradients(ref.dK, cases.output_shape(name), kw.get("affine"), kw.get("rotate"), kw.get("zoom"))
    for got, w in zip((g.affine, g.rotate, g.zoom), want):
        if w is not None:
            assert np.all(np.abs(np.asarray(got) - w) <= 1e-6 * np.maximum(1.0, np.abs(w))), (got, w)
    # a repeated call
    again = _call(name, which, count)
    assert _same(g.points, again.points) and _same(g.displacement, again.displacement)
    assert _same(g.inverse_map, again.inverse_map)


@pytest.mark.parametrize("name", cases.NAMES)
def test_permutation_slice_and_float32(name):
    I, D, kw = cases.case(name)
    q, u, A, G = cases.data(name)
    g = _call(name, "all", cases.NMAX)
    perm = np.random.default_rng(3).permutation(cases.NMAX)
    p = ed.deform_grid_derivatives_gradient(q[perm], D, I, u[perm], A[perm], G[perm], **kw)
    assert _same(p.displacement, g.displacement) and _same(p.inverse_map, g.inverse_map)
    assert _same(p.points, g.points[perm])
    s = _call(name, "all", 257)
    assert _same(s.points, g.points[:257])
    # float32 positions and cotangents against their float64 upcast
    q32, u32, A32, G32 = (a[:257].astype(np.float32) for a in (q, u, A, G))
    f = ed.deform_grid_derivatives_gradient(q32, D, I, u32, A32, G32, **kw)
    w = ed.deform_grid_derivatives_gradient(*(a.astype(np.float64) for a in (q32,)), D, I,
                                            *(a.astype(np.float64) for a in (u32, A32, G32)), **kw)
    assert f.points.dtype == np.float32 and _same(f.points, w.points.astype(np.float32))
    assert _same(f.displacement, w.displacement) and _same(f.inverse_map, w.inverse_map)


@pytest.mark.parametrize("name", cases.NAMES)
def test_batch_equals_single_calls(name):
    I, D, kw = cases.case(name)
    q, u, A, G = cases.data(name)
    rng = np.random.default_rng(5)
    sl = [slice(0, 257), slice(300, 557), slice(600, 857)]
    Ds = np.stack([D, D + rng.standard_normal(D.shape), -D])
    stack = lambda a, f=1.0: np.stack([a[s] * (f ** b) for b, s in enumerate(sl)])        # noqa: E731
    qs, us, As, Gs = stack(q), stack(u, 3.0), stack(A, 0.5), stack(G, 7.0)
    got = ed.deform_grid_derivatives_gradient_batch(qs, Ds, I, us, As, Gs, **kw)
    total = 0.0
    for b in range(3):
        one = ed.deform_grid_derivatives_gradient(qs[b], Ds[b], I, us[b], As[b], Gs[b], **kw)
        assert _same(got.points[b], one.points) and _same(got.displacement[b], one.displacement)
        total = total + one.inverse_map
    assert _same(got.inverse_map, total)


def test_a_non_finite_cotangent_poisons_only_its_sample():
    name = "2d-crop-affine-rotate-zoom"
    I, D, kw = cases.case(name)
    q, u, A, G = (a[:257] for a in cases.data(name))
    clean = ed.deform_grid_derivatives_gradient(q, D, I, u, A, G, **kw)
    for which, index in (("u", (100, 0)), ("A", (101, 1, 0)), ("G", (102, 0, 1, 1))):
        cot = dict(u=u.copy(), A=A.copy(), G=G.copy())
        cot[which][index] = np.inf if which == "A" else np.nan
        qs = np.stack([q, q, q])
        got = ed.deform_grid_derivatives_gradient_batch(qs, np.stack([D, D, D]), I, np.stack([u, cot["u"], u]),
                                                        np.stack([A, cot["A"], A]), np.stack([G, cot["G"], G]), **kw)
        assert np.isnan(got.displacement[1]).all()
        assert _same(got.displacement[0], clean.displacement) and _same(got.displacement[2], clean.displacement)
        assert _same(got.points[0], clean.points) and _same(np.delete(got.points[1], index[0], 0),
                                                            np.delete(clean.points, index[0], 0))
        assert np.isnan(got.inverse_map).all()               # (the map's fields are summed over the samples)
        one = ed.deform_grid_derivatives_gradient(q, D, I, cot["u"], cot["A"], cot["G"], **kw)
        assert np.isnan(one.displacement).all() and np.isnan(one.inverse_map).all()
    # non-finite cotangents on the points that contribute nothing are ignored
    cot = u.copy()
    cot[cases.NAN_ROW] = np.nan
    cot[cases.FAR_ROW] = np.inf
    got = ed.deform_grid_derivatives_gradient(q, D, I, cot, A, G, **kw)
    assert _same(got.displacement, clean.displacement) and _same(got.inverse_map, clean.inverse_map)
    assert _same(got.points, clean.points) and not got.points[[cases.NAN_ROW, cases.FAR_ROW]].any()


def test_only_what_is_wanted():
    """the three results one by one through the host layer's switches: the same bits as together"""
    name = "3d-affine-crop"
    I, D, kw = cases.case(name)
    q, u, A, G = (a[:65] for a in cases.data(name))
    g = ed.deform_grid_derivatives_gradient(q, D, I, u, A, G, **kw)
    api = importlib.import_module("elasticdeform_amd.deform_grid")
    for want in (dict(want_points=True, want_disp=False, want_map=False),
                 dict(want_points=False, want_disp=True, want_map=False),
                 dict(want_points=False, want_disp=False, want_map=True)):
        _, rows, ddisp, dk = api._points_gradient(q, u, D, I, kw.get("crop"), None, kw.get("affine"), None, None, False,
                                                  False, derivatives=(A, G), **want)
        if want["want_points"]:
            assert _same(rows, g.points) and ddisp is None and dk is None
        if want["want_disp"]:
            assert _same(ddisp, g.displacement) and rows is None
        if want["want_map"]:
            assert _same(dk.cpu().numpy(), g.inverse_map)


def test_capture_into_a_graph():
    name = "3d-affine-crop"
    I, D, kw = cases.case(name)
    qt, ut, At, Gt = (torch.from_numpy(a.copy()).cuda() for a in cases.data(name))
    Dt = torch.from_numpy(D).cuda()
    g0 = ed.deform_grid_derivatives_gradient(qt, Dt, I, ut, At, Gt, **kw)         # eager
    f0 = ed.deform_grid_derivatives(qt, Dt, I, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ed.deform_grid_derivatives_gradient(qt, Dt, I, ut, At, Gt, **kw)          # warm-up: the stream's workspace
        ed.deform_grid_derivatives(qt, Dt, I, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g = ed.deform_grid_derivatives_gradient(qt, Dt, I, ut, At, Gt, **kw)
        f = ed.deform_grid_derivatives(qt, Dt, I, **kw)
    for _ in range(3):
        g.points.zero_()
        g.displacement.fill_(7.0)
        g.inverse_map.fill_(7.0)
        f.hessian.fill_(7.0)
        with torch.cuda.stream(side):
            ed.deform_grid_derivatives_gradient(qt[:333], Dt, I, 3.0 * ut[:333], **kw)   # an eager call of another N
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g.points, g0.points) and torch.equal(g.displacement, g0.displacement)
        assert torch.equal(g.inverse_map, g0.inverse_map)
        assert torch.equal(torch.nan_to_num(f.hessian), torch.nan_to_num(f0.hessian))


# ---- autograd -------------------------------------------------------------------------------------------------------

def _regulariser(J, H):
    det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
    return torch.relu(-det).sum() + (H ** 2).sum()


def test_autograd_step_test_of_a_folding_and_bending_penalty():
    """d/dD of relu(-det J).sum() + (H ** 2).sum() against central differences, float64, the 2-axis case"""
    name = "2d-crop-affine-rotate-zoom"
    I, D, kw = cases.case(name)
    D = 4.0 * D                                               # strong enough to fold somewhere
    sane = cases.reference(name, 65).sane
    q = torch.from_numpy(cases.data(name)[0][:65][sane]).cuda()
    Dt = torch.from_numpy(D).cuda().requires_grad_(True)
    r, J, H = etorch.deform_grid_derivatives(q, Dt, I, displacement_grad=True, **kw)
    det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
    assert bool((det < 0).any()) and bool((det > 0).any())
    loss = _regulariser(J, H)
    loss.backward()
    grad = Dt.grad.cpu().numpy()
    assert grad.shape == D.shape and np.isfinite(grad).all()

    def value(Dn):
        out = ed.deform_grid_derivatives(q, torch.from_numpy(Dn).cuda(), I, **kw)
        return float(_regulariser(out.jacobian, out.hessian))

    # the loss is piecewise quadratic in D (H linear, det bilinear): a central difference with h = 1e-6 is exact up to
    # rounding, about eps |loss| / h, as long as no det changes its sign within the step
    h = 1e-6
    rng = np.random.default_rng(9)
    scale = max(1.0, float(loss.detach()))
    for _ in range(12):
        j = tuple(rng.integers(0, s) for s in D.shape)
        E = np.zeros_like(D)
        E[j] = h
        d = (value(D + E) - value(D - E)) / (2 * h)
        assert abs(d - grad[j]) <= 1e-6 * max(1.0, abs(grad[j])) + 64 * EPS * scale / h, (j, d, grad[j])


def test_autograd_reaches_positions_and_rotate_and_respects_the_switches():
    name = "2d-crop-affine-rotate-zoom"
    I, D, kw = cases.case(name)
    q0, u, A, G = (a[5:70] for a in cases.data(name))
    ref = ed.deform_grid_derivatives_gradient(q0, D, I, u, A, G, **kw)
    q = torch.from_numpy(q0.copy()).cuda().requires_grad_(True)
    Dt = torch.from_numpy(D).cuda().requires_grad_(True)
    rot = torch.tensor(kw["rotate"], dtype=torch.float64, requires_grad=True)
    call = dict(kw, rotate=rot)
    ut, At, Gt = (torch.from_numpy(a.copy()).cuda() for a in (u, A, G))
    # without displacement_grad the grid receives nothing; the positions do
    r, J, H = etorch.deform_grid_derivatives(q, Dt, I, **call)
    ((r * ut).sum() + (J * At).sum() + (H * Gt).sum()).backward()
    assert Dt.grad is None and rot.grad is None
    assert _same(q.grad.cpu().numpy(), ref.points)
    q.grad = None
    r, J, H = etorch.deform_grid_derivatives(q, Dt, I, displacement_grad=True, affine_grad=True, **call)
    ((r * ut).sum() + (J * At).sum() + (H * Gt).sum()).backward()
    assert _same(q.grad.cpu().numpy(), ref.points)
    assert _same(Dt.grad.cpu().numpy(), ref.displacement)
    assert rot.grad is not None and abs(float(rot.grad) - ref.rotate) <= 1e-12 * max(1.0, abs(ref.rotate))
    # one output alone: the cotangents of the others are absent, not zeros
    Dt.grad = None
    H = etorch.deform_grid_derivatives(q.detach(), Dt, I, displacement_grad=True, **kw).hessian
    (H * Gt).sum().backward()
    only = ed.deform_grid_derivatives_gradient(q0, D, I, d_hessian=G, **kw)
    assert _same(Dt.grad.cpu().numpy(), only.displacement)
    # hessian=False: two differentiable outputs
    Dt.grad = None
    out = etorch.deform_grid_derivatives(q.detach(), Dt, I, hessian=False, displacement_grad=True, **kw)
    assert out.hessian is None
    (out.jacobian * At).sum().backward()
    only = ed.deform_grid_derivatives_gradient(q0, D, I, d_jacobian=A, **kw)
    assert _same(Dt.grad.cpu().numpy(), only.displacement)


def test_one_descent_step_lowers_the_bending_energy():
    name = "3d-affine-crop"
    I, D, kw = cases.case(name)
    sane = cases.reference(name, 257).sane
    q = torch.from_numpy(cases.data(name)[0][:257][sane]).cuda()
    Dt = torch.from_numpy(D).cuda().requires_grad_(True)

    def energy(grid, grad):
        H = etorch.deform_grid_derivatives(q, grid, I, displacement_grad=grad, **kw).hessian
        return (H ** 2).sum((-1, -2, -3)).mean()

    e0 = energy(Dt, True)
    e0.backward()
    g = Dt.grad
    # the energy is quadratic in D: along -g it is e0 - t |g|^2 + t^2 c with c <= e0 |g|^2 ... a small step lowers it
    step = 0.05 * float(e0.detach()) / float((g * g).sum())
    e1 = energy((Dt - step * g).detach(), False)
    print("bending energy %.6g -> %.6g" % (float(e0.detach()), float(e1)))
    assert float(e1) < float(e0.detach())


def _library_call(u0):
    """edhip_deform_points_derivatives_gradient itself on len(u0) samples of one point at (100, 0.5) -- sane: the limit
    is a control coordinate of 4e15 --, a prefiltered 4 x 4 grid on an 8 x 8 image, float64, d_coordinates (u0[b], 0)
    for sample b and nothing else: the gradient of the PREFILTERED grid, without the host layer's transposed filter
    (whose gain would take 4e307 past the largest double)."""
    api = importlib.import_module("elasticdeform_amd.deform_grid")
    from elasticdeform_amd import _lib
    nb = len(u0)
    P = torch.from_numpy(np.random.default_rng(11).random((2, 4, 4)) - 0.5).cuda().repeat(nb, 1, 1, 1)
    q = torch.tensor([[100.0, 0.5]], dtype=torch.float64).cuda().repeat(nb, 1, 1)
    u = torch.tensor([[[v, 0.0]] for v in u0], dtype=torch.float64).cuda()
    rows, dP = torch.full_like(q, 7.0), torch.full_like(P, 7.0)
    dK = torch.full((nb, 2, 3), 7.0, dtype=torch.float64).cuda()
    _lib.deform_points_derivatives_gradient(nb, *api._desc_sample0(q), *api._desc_sample0(u), None, 0, None, 0,
                                            *api._desc_sample0(P), (8, 8), None, None, *api._desc_sample0(rows),
                                            *api._desc_sample0(dP), *api._desc_sample0(dK), 0, api._stream(q.device))
    torch.cuda.synchronize()
    return rows.cpu().numpy(), dP.cpu().numpy(), dK.cpu().numpy()


def test_a_bound_that_overflows_poisons_its_own_sum_of_its_sample_only():
    """d_coordinates = (4e307, 0) alone: bP = 4e307 gives a finite 2 N bP, bK = |u_0 q_0| = 4e309 is not finite.  This
    call's rule keeps one state per quantum: dinverse_affine is NaN, ddisplacement is finite and equals u_h beta(q, j)
    to the quantum 2^(1023 - 62) -- at most four taps of the point fold into one cell, half a quantum each -- and to
    the rounding of the products in fp64 (beta is formed here from plainly evaluated weights: 64 ulp of 4e307 is
    generous).  A second sample with d_coordinates (1, 0) in the same call gives the bits of a call of its own."""
    rows, dP, dK = _library_call([4e307])
    beta = []
    for qk in (100.0, 0.5):
        cp = 3.0 * qk / 7.0
        fl = int(np.floor(cp))
        t = cp - fl
        z = 1.0 - t
        w = [z ** 3 / 6, (3 * t ** 3 - 6 * t * t + 4) / 6, (3 * z ** 3 - 6 * z * z + 4) / 6, t ** 3 / 6]
        b = np.zeros(4)
        for s in range(4):
            j = (fl - 1 + s) % 6
            b[6 - j if j >= 4 else j] += w[s]
        beta.append(b)
    want = 4e307 * np.outer(beta[0], beta[1])
    tol = 2.0 * 2.0 ** (1023 - 62) + 64 * 4e307 * 2.0 ** -52
    err = np.abs(dP[0, 0] - want)
    print("worst |ddisplacement - u beta| = %.3g, bound %.3g" % (err.max(), tol))
    assert np.isfinite(dP).all() and (err <= tol).all() and not dP[0, 1].any()
    assert np.isnan(dK).all() and np.isfinite(rows).all()
    rows2, dP2, dK2 = _library_call([4e307, 1.0])
    rows1, dP1, dK1 = _library_call([1.0])
    assert _same(rows2[0], rows[0]) and _same(dP2[0], dP[0]) and _same(dK2[0], dK[0])
    assert _same(rows2[1], rows1[0]) and _same(dP2[1], dP1[0]) and _same(dK2[1], dK1[0])
    assert np.abs(dP1[0, 0] - np.outer(beta[0], beta[1])).max() <= 1e-14
    assert np.array_equal(dK1[0], [[100.0, 0.5, 1.0], [0.0, 0.0, 0.0]])
