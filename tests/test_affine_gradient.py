"""
GPU tests of the gradient with respect to affine, rotate and zoom (elasticdeform_amd.deform_grid_affine_gradient,
edhip_deform_transform_gradient, elasticdeform_amd.torch.deform_grid(..., affine_grad=True)).

Expected values come from central differences of the CPU oracle's float64 deform_grid: L = sum <dY, Y>, every entry
of the user's affine (and rotate, zoom) perturbed by h = 1e-6 max(1, |value|).  Seeds and scales keep the voxels off
the forward's kinks within the step, as in tests/test_displacement_gradient.py.
"""
import numpy as np
import pytest

from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402
import importlib  # noqa: E402

_dg = importlib.import_module("elasticdeform_amd.deform_grid")      # (the module; the package exports the function)

MODES = ["constant", "nearest", "mirror", "reflect", "wrap"]


def _loss(X, D, dY, kw):
    Y = orc.deform_grid(X, D, **kw)
    Ys, dYs = (Y, dY) if isinstance(Y, list) else ([Y], [dY])
    return sum(float(np.sum(y.astype(np.float64) * dy)) for y, dy in zip(Ys, dYs))


def _fd_params(X, D, dY, kw):
    """central differences with respect to every entry of kw['affine'] (the identity (n, n+1) when None), then
    rotate, then zoom (when given) -> (affine gradient, rotate gradient, zoom gradient)"""
    n = D.shape[0]
    A = kw.get("affine")
    A0 = np.concatenate([np.eye(n), np.zeros((n, 1))], 1) if A is None else np.array(A, dtype=np.float64)
    gA = np.zeros_like(A0)
    for idx in np.ndindex(*A0.shape):
        if A0.shape[0] == n + 1 and idx[0] == n:
            continue
        h = 1e-6 * max(1.0, abs(A0[idx]))
        vals = []
        for s in (1, -1):
            a = A0.copy()
            a[idx] += s * h
            vals.append(_loss(X, D, dY, dict(kw, affine=a)))
        gA[idx] = (vals[0] - vals[1]) / (2 * h)
    out = [gA]
    for name in ("rotate", "zoom"):
        v = kw.get(name)
        if v is None:
            out.append(None)
            continue
        h = 1e-6 * max(1.0, abs(v))
        out.append((_loss(X, D, dY, dict(kw, **{name: v + h})) - _loss(X, D, dY, dict(kw, **{name: v - h}))) / (2 * h))
    return out


def _case(shape, ncp, sigma, seed, nin=1, channels=None, affine=True):
    rng = np.random.default_rng(seed)
    n = len(shape)
    full = tuple(shape) + ((channels,) if channels else ())
    X = [rng.standard_normal(full) for _ in range(nin)]
    D = rng.standard_normal((n,) + tuple(ncp)) * sigma
    A = None
    if affine:
        A = np.concatenate([np.eye(n) + 0.04 * rng.standard_normal((n, n)), 0.6 * rng.standard_normal((n, 1))], 1)
    return (X if nin > 1 else X[0]), D, A, rng


def _check(X, D, kw, rng, tol=1e-6):
    Y = orc.deform_grid(X, D, **kw)
    dY = [rng.standard_normal(y.shape) for y in Y] if isinstance(Y, list) else rng.standard_normal(Y.shape)
    wA, wr, wz = _fd_params(X, D, dY, kw)
    got = ed.deform_grid_affine_gradient(X, dY, D, **kw)
    assert isinstance(got.affine, np.ndarray) and got.affine.shape == wA.shape and got.affine.dtype == np.float64
    assert got.inverse_map.shape == (D.shape[0], D.shape[0] + 1)
    want = np.concatenate([wA.reshape(-1)] + [np.array([v]) for v in (wr, wz) if v is not None])
    have = np.concatenate([got.affine.reshape(-1)] + [np.array([v]) for v in (got.rotate, got.zoom) if v is not None])
    assert (got.rotate is None) == (wr is None) and (got.zoom is None) == (wz is None)
    scale = np.abs(want).max()
    assert scale > 0
    err = np.abs(have - want).max()
    assert err <= tol * scale, (err / scale, kw)
    return got


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_axes_against_finite_differences(n):
    shape, ncp = {1: ((40,), (5,)), 2: ((24, 30), (4, 5)), 3: ((12, 14, 10), (3, 4, 3)),
                  4: ((6, 5, 6, 5), (3, 3, 3, 3))}[n]
    X, D, A, rng = _case(shape, ncp, 1.0, 2000 + n)
    _check(X, D, dict(order=3, mode="mirror", affine=A), rng)


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode", MODES)
def test_2d_orders_and_modes(order, mode):
    X, D, A, rng = _case((24, 30), (4, 5), 1.2, 2100 + 10 * order + MODES.index(mode))
    _check(X, D, dict(order=order, mode=mode, affine=A), rng)


def test_crop_rotate_zoom_homogeneous_identity():
    X, D, A, rng = _case((24, 30), (4, 5), 1.2, 2200)
    crop = (slice(3, 20), slice(5, 27))
    _check(X, D, dict(order=3, mode="mirror", crop=crop, affine=A), rng)
    _check(X, D, dict(order=3, mode="nearest", rotate=17.0, zoom=1.1), rng)
    _check(X, D, dict(order=3, mode="mirror", rotate=-9.0, zoom=0.93, crop=crop), rng)
    _check(X, D, dict(order=3, mode="reflect", rotate=5.0, zoom=1.05, affine=A), rng)
    _check(X, D, dict(order=3, mode="mirror", affine=np.vstack([A, [0.0, 0.0, 1.0]])), rng)
    g = _check(X, D, dict(order=3, mode="mirror"), rng)               # affine=None: at the identity
    assert g.affine.shape == (2, 3) and g.rotate is None and g.zoom is None
    X3, D3, A3, rng = _case((12, 14, 10), (3, 3, 3), 1.0, 2201)
    _check(X3, D3, dict(order=3, mode="mirror", affine=A3, crop=(slice(1, 11), slice(2, 13), slice(0, 9))), rng)


def test_steps_inputs_prefilter_dense():
    X, D, A, rng = _case((20, 22), (4, 4), 1.2, 2300, channels=3)
    _check(X, D, dict(order=3, mode="mirror", axis=(0, 1), affine=A), rng)
    X, D, A, rng = _case((20, 22), (4, 4), 1.2, 2301, nin=2)
    _check(X, D, dict(order=[3, 1], mode=["mirror", "nearest"], affine=A), rng)
    X, D, A, rng = _case((20, 22), (4, 4), 1.2, 2302)
    _check(X, D, dict(order=3, mode="reflect", prefilter=False, affine=A), rng)
    X, D, A, rng = _case((16, 60), (4, 20), 0.5, 2303)
    _check(X, D, dict(order=3, mode="mirror", affine=A), rng)


def test_order_zero_is_exactly_zero():
    X, D, A, rng = _case((20, 22), (4, 4), 1.2, 2400)
    g = ed.deform_grid_affine_gradient(X, rng.standard_normal(X.shape), D, order=0, mode="mirror", affine=A,
                                       rotate=3.0, zoom=1.1)
    assert np.array_equal(g.affine, np.zeros_like(A)) and g.rotate == 0.0 and g.zoom == 0.0
    assert np.array_equal(g.inverse_map, np.zeros((2, 3)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_identity_translation_equals_summed_displacement_gradient():
    # B-spline weights sum to 1 and the prefilter keeps constants: a constant shift of D[h] is a translation of K
    rng = np.random.default_rng(2500)
    with torch.cuda.device(0):
        X = torch.rand((256, 256, 256), device="cuda", dtype=torch.float32)
        dY = torch.rand((256, 256, 256), device="cuda", dtype=torch.float32)
        D = _dev(rng.standard_normal((3, 5, 5, 5)) * 5)
        g = ed.deform_grid_affine_gradient(X, dY, D, order=3, mode="mirror")
        dD = ed.deform_grid_displacement_gradient(X, dY, D, order=3, mode="mirror")
        s = dD.reshape(3, -1).sum(1)
        tol = 1e-9 * dD.abs().reshape(3, -1).sum(1)
        assert torch.all((g.affine[:, -1] + s).abs() <= tol), (g.affine[:, -1], s)
        assert torch.all((g.inverse_map[:, -1] - s).abs() <= tol)


def test_float32_against_float64_forward_differences():
    rng = np.random.default_rng(2600)
    with torch.cuda.device(0):
        X = rng.standard_normal((128, 128, 128))
        dY = rng.standard_normal(X.shape)
        D = rng.standard_normal((3, 5, 5, 5)) * 3
        A = np.concatenate([np.eye(3) + 0.02 * rng.standard_normal((3, 3)), 0.5 * rng.standard_normal((3, 1))], 1)
        Xd, dYd, Dd = _dev(X), _dev(dY), _dev(D)
        g32 = ed.deform_grid_affine_gradient(Xd.float(), dYd.float(), Dd, order=3, mode="mirror", affine=A)

        def loss(a):
            return float(torch.sum(ed.deform_grid(Xd, Dd, order=3, mode="mirror", affine=a) * dYd))
        want = np.zeros_like(A)
        for idx in np.ndindex(*A.shape):
            h = 1e-5 * max(1.0, abs(A[idx]))
            ap, am = A.copy(), A.copy()
            ap[idx] += h
            am[idx] -= h
            want[idx] = (loss(ap) - loss(am)) / (2 * h)
        got = g32.affine.cpu().numpy()
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), (got, want)


def test_bit_reproducibility_batch_and_combined():
    rng = np.random.default_rng(2700)
    kw = dict(order=3, mode="mirror", affine=np.array([[1.02, 0.03, -0.01, 0.4], [-0.02, 0.98, 0.02, -0.3],
                                                       [0.01, -0.03, 1.01, 0.2]]))
    with torch.cuda.device(0):
        X = _dev(rng.standard_normal((3, 40, 36, 44)).astype(np.float32))
        D = _dev(rng.standard_normal((3, 3, 4, 4, 5)) * 3)
        dY = _dev(rng.standard_normal((3, 40, 36, 44)).astype(np.float32))
        # repeated calls
        a = ed.deform_grid_affine_gradient(X[0], dY[0], D[0], **kw)
        b = ed.deform_grid_affine_gradient(X[0], dY[0], D[0], **kw)
        assert torch.equal(a.affine, b.affine) and torch.equal(a.inverse_map, b.inverse_map)
        assert a.affine.dtype == torch.float64 and a.affine.device == X.device
        # the C ABI's batch samples = single calls (dK as the library wrote it), displacement part included
        _, ddb, dkb = _dg._transform_gradient_batch(X, dY, D, want_disp=True, want_map=True, **kw)
        singles = []
        for s in range(3):
            _, _, dds, dks = _dg._transform_gradient(X[s], dY[s], D[s], want_disp=True, want_map=True, **kw)
            assert torch.equal(dkb[s], dks) and torch.equal(ddb[s], dds)
            # the displacement part of a combined call = deform_grid_displacement_gradient
            assert torch.equal(dds, ed.deform_grid_displacement_gradient(X[s], dY[s], D[s], **kw))
            singles.append(ed.deform_grid_affine_gradient(X[s], dY[s], D[s], **kw))
        # the Python batch result = the sample-order fp64 sum of the single calls
        gb = ed.deform_grid_affine_gradient_batch(X, dY, D, **kw)
        for f in ("affine", "inverse_map"):
            want = getattr(singles[0], f)
            for r in singles[1:]:
                want = want + getattr(r, f)
            assert torch.equal(getattr(gb, f), want), f


def test_torch_gradcheck_single_and_batch():
    rng = np.random.default_rng(2800)
    with torch.cuda.device(0):
        X = _dev(rng.standard_normal((9, 11))).requires_grad_()
        D = _dev(rng.standard_normal((2, 3, 3)) * 0.8).requires_grad_()
        A = _dev(np.array([[1.03, 0.04, 0.3], [-0.05, 0.97, -0.2]])).requires_grad_()
        r = torch.tensor(7.0, dtype=torch.float64, device="cuda", requires_grad=True)
        z = torch.tensor(1.08, dtype=torch.float64, device="cuda", requires_grad=True)
        assert torch.autograd.gradcheck(
            lambda x, d, a, rr, zz: etorch.deform_grid(x, d, 3, "mirror", affine=a, rotate=rr, zoom=zz,
                                                       displacement_grad=True, affine_grad=True),
            (X, D, A, r, z), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=1e-12)
        X3 = _dev(rng.standard_normal((6, 7, 5))).requires_grad_()
        D3 = _dev(rng.standard_normal((3, 3, 3, 3)) * 0.6).requires_grad_()
        A3 = _dev(np.concatenate([np.eye(3) + 0.03 * rng.standard_normal((3, 3)),
                                  0.3 * rng.standard_normal((3, 1))], 1)).requires_grad_()
        assert torch.autograd.gradcheck(
            lambda x, d, a: etorch.deform_grid(x, d, 3, "mirror", 0.0, None, True, None, a, displacement_grad=True,
                                               affine_grad=True),
            (X3, D3, A3), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=1e-12)
        Xb = _dev(rng.standard_normal((2, 8, 9))).requires_grad_()
        Db = _dev(rng.standard_normal((2, 2, 3, 3)) * 0.8).requires_grad_()
        assert torch.autograd.gradcheck(
            lambda x, d, a, rr, zz: etorch.deform_grid_batch(x, d, order=3, mode="mirror", affine=a, rotate=rr,
                                                             zoom=zz, displacement_grad=True, affine_grad=True),
            (Xb, Db, A, r, z), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=1e-12)


def test_torch_default_leaves_affine_grad_none():
    rng = np.random.default_rng(2900)
    with torch.cuda.device(0):
        X = _dev(rng.standard_normal((16, 18))).requires_grad_()
        D = _dev(rng.standard_normal((2, 3, 3)))
        A = _dev(np.array([[1.0, 0.02, 0.3], [0.01, 1.0, -0.2]])).requires_grad_()
        etorch.deform_grid(X, D, order=3, mode="mirror", affine=A).sum().backward()
        assert X.grad is not None and A.grad is None
        # with the opt-in: in the parameter's dtype, on its device
        Ac = torch.tensor([[1.0, 0.02, 0.3], [0.01, 1.0, -0.2]], dtype=torch.float32, requires_grad=True)
        etorch.deform_grid(X, D, order=3, mode="mirror", affine=Ac, affine_grad=True).sum().backward()
        assert Ac.grad is not None and Ac.grad.dtype == torch.float32 and Ac.grad.device.type == "cpu"


def test_graph_capture_replay_matches_eager():
    rng = np.random.default_rng(3000)
    A = np.array([[1.02, 0.01, -0.02, 0.3], [0.0, 0.99, 0.01, -0.2], [0.02, 0.0, 1.01, 0.1]])
    with torch.cuda.device(0):
        X = _dev(rng.standard_normal((48, 48, 48)).astype(np.float32))
        dY = _dev(rng.standard_normal((48, 48, 48)).astype(np.float32))
        D = _dev(rng.standard_normal((3, 4, 4, 4)) * 2)

        def f():
            return ed.deform_grid_affine_gradient(X, dY, D, order=3, mode="mirror", affine=A)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                f()                              # warm the capture stream's workspace and the plan
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = f()
        for i in range(3):
            X.copy_(_dev(rng.standard_normal((48, 48, 48)).astype(np.float32)))
            D.copy_(_dev(rng.standard_normal((3, 4, 4, 4)) * 2))
            g.replay()
            torch.cuda.synchronize()
            want = f()
            assert torch.equal(out.affine, want.affine) and torch.equal(out.inverse_map, want.inverse_map), i


def _blobs(n, dims, rng, count=6, width=5.0):
    grids = np.meshgrid(*(np.arange(n),) * dims, indexing="ij")
    vol = np.zeros((n,) * dims)
    for _ in range(count):
        c = rng.uniform(0.3 * n, 0.7 * n, dims)
        vol += np.exp(-sum((g - ci) ** 2 for g, ci in zip(grids, c)) / (2 * width ** 2))
    return vol


def test_registration_3d_rotation_scale_translation():
    rng = np.random.default_rng(3100)
    n = 40
    with torch.cuda.device(0):
        X = _dev(_blobs(n, 3, rng).astype(np.float32))
        D = torch.zeros((3, 2, 2, 2), dtype=torch.float64, device="cuda")
        c = torch.full((3,), (n - 1) / 2.0, dtype=torch.float64, device="cuda")

        def affine(angle, scale, t):
            th = angle * (np.pi / 180.0)
            one, zero = torch.ones_like(th), torch.zeros_like(th)
            R = torch.stack([torch.stack([one, zero, zero]), torch.stack([zero, torch.cos(th), -torch.sin(th)]),
                             torch.stack([zero, torch.sin(th), torch.cos(th)])])
            M = scale * R
            return torch.cat([M, (c - M @ c + t)[:, None]], dim=1)

        truth = (torch.tensor(6.0, dtype=torch.float64, device="cuda"),
                 torch.tensor(1.05, dtype=torch.float64, device="cuda"),
                 torch.tensor([0.4, -0.3, 0.25], dtype=torch.float64, device="cuda"))
        Y = ed.deform_grid(X, D, order=3, mode="nearest", affine=affine(*truth).cpu().numpy())
        angle = torch.tensor(0.0, dtype=torch.float64, device="cuda", requires_grad=True)
        scale = torch.tensor(1.0, dtype=torch.float64, device="cuda", requires_grad=True)
        t = torch.zeros(3, dtype=torch.float64, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([{"params": [angle], "lr": 0.1}, {"params": [scale], "lr": 2e-3},
                                {"params": [t], "lr": 0.02}])
        # (Adam moves each parameter by about its lr per step: the schedule leaves room for the 6 degrees)
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.995)
        losses = []
        for _ in range(700):
            opt.zero_grad()
            out = etorch.deform_grid(X, D, order=3, mode="nearest", affine=affine(angle, scale, t), affine_grad=True)
            loss = ((out - Y) ** 2).sum()
            loss.backward()
            opt.step()
            sched.step()
            losses.append(float(loss.detach()))
        assert losses[-1] <= losses[0] / 100, (losses[0], losses[-1])
        assert abs(float(angle) - 6.0) <= 0.02 * 6.0, float(angle)
        assert abs(float(scale) - 1.05) <= 0.02 * 0.05, float(scale)
        assert torch.all((t - truth[2]).abs() <= 0.02 * truth[2].abs().max()), t


def test_registration_2d_rotate_zoom():
    rng = np.random.default_rng(3200)
    n = 96
    with torch.cuda.device(0):
        X = _dev(_blobs(n, 2, rng, count=8, width=6.0).astype(np.float32))
        D = torch.zeros((2, 2, 2), dtype=torch.float64, device="cuda")
        Y = ed.deform_grid(X, D, order=3, mode="nearest", rotate=12.0, zoom=1.15)
        rot = torch.tensor(0.0, dtype=torch.float64, device="cuda", requires_grad=True)
        zoom = torch.tensor(1.0, dtype=torch.float64, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([{"params": [rot], "lr": 0.2}, {"params": [zoom], "lr": 4e-3}])
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.99)
        for _ in range(400):
            opt.zero_grad()
            out = etorch.deform_grid(X, D, order=3, mode="nearest", rotate=rot, zoom=zoom, affine_grad=True)
            ((out - Y) ** 2).sum().backward()
            opt.step()
            sched.step()
        assert abs(float(rot) - 12.0) <= 0.2, float(rot)
        assert abs(float(zoom) - 1.15) <= 0.01, float(zoom)
