"""
GPU tests of the gradient with respect to the control-point displacement
(elasticdeform_amd.deform_grid_displacement_gradient, edhip_deform_displacement_gradient).

Expected values come from central differences of the CPU oracle's deform_grid (the restatement pinned to the
reference) in float64: L = sum <dY, Y>, every raw control coefficient perturbed by h = 1e-6 max(1, |D|).
Seeds and displacement scales are small enough that no voxel sits on a kink of the forward (order-1 integer
crossings, the borders of 'constant' / 'nearest', the folds of 'mirror' / 'reflect') within the step.
"""
import numpy as np
import pytest

from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402
from elasticdeform_amd import _lib  # noqa: E402

MODES = ["constant", "nearest", "mirror", "reflect", "wrap"]


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


def _case(shape, ncp, sigma, seed, nin=1, channels=None):
    rng = np.random.default_rng(seed)
    n = len(shape)
    full = tuple(shape) + ((channels,) if channels else ())
    X = [rng.standard_normal(full) for _ in range(nin)]
    D = rng.standard_normal((n,) + tuple(ncp)) * sigma
    return (X if nin > 1 else X[0]), D, rng


def _check(X, D, kw, rng, tol=1e-6):
    Y = orc.deform_grid(X, D, **kw)
    dY = [rng.standard_normal(y.shape) for y in Y] if isinstance(Y, list) else rng.standard_normal(Y.shape)
    want = _fd(X, D, dY, kw)
    got = ed.deform_grid_displacement_gradient(X, dY, D, **kw)
    assert isinstance(got, np.ndarray) and got.shape == D.shape and got.dtype == np.float64
    scale = np.abs(want).max()
    assert scale > 0
    err = np.abs(got - want).max()
    assert err <= tol * scale, (err / scale, kw)
    return got


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode", MODES)
def test_1d_against_finite_differences(order, mode):
    X, D, rng = _case((40,), (5,), 1.5, 10 * order + MODES.index(mode))
    _check(X, D, dict(order=order, mode=mode), rng)


@pytest.mark.parametrize("order", [1, 3, 5])
@pytest.mark.parametrize("mode", MODES)
def test_2d_against_finite_differences(order, mode):
    X, D, rng = _case((24, 30), (4, 5), 1.5, 100 + 10 * order + MODES.index(mode))
    _check(X, D, dict(order=order, mode=mode), rng)


@pytest.mark.parametrize("order,mode", [(1, "nearest"), (2, "mirror"), (3, "constant"), (4, "reflect"),
                                        (5, "wrap")])
def test_3d_against_finite_differences(order, mode):
    X, D, rng = _case((12, 14, 10), (3, 4, 3), 1.2, 200 + order)
    _check(X, D, dict(order=order, mode=mode), rng)


def test_4d_against_finite_differences():
    X, D, rng = _case((6, 5, 6, 5), (3, 3, 3, 3), 0.8, 300)
    _check(X, D, dict(order=3, mode="mirror"), rng)


def test_crop_affine_rotate_zoom():
    X, D, rng = _case((24, 30), (4, 5), 1.5, 400)
    _check(X, D, dict(order=3, mode="mirror", crop=(slice(3, 20), slice(5, 27))), rng)
    _check(X, D, dict(order=3, mode="nearest", rotate=17.0, zoom=1.1), rng)
    X3, D3, rng = _case((12, 14, 10), (3, 3, 3), 1.0, 401)
    A = np.array([[1.05, 0.05, 0.0, 0.3], [-0.04, 0.97, 0.03, -0.2], [0.02, 0.0, 1.02, 0.1]])
    _check(X3, D3, dict(order=3, mode="mirror", affine=A), rng)


def test_steps_inputs_prefilter_dense():
    # a channel step axis
    X, D, rng = _case((20, 22), (4, 4), 1.5, 500, channels=3)
    _check(X, D, dict(order=3, mode="mirror", axis=(0, 1)), rng)
    # two inputs with different order and mode
    X, D, rng = _case((20, 22), (4, 4), 1.5, 501, nin=2)
    _check(X, D, dict(order=[3, 1], mode=["mirror", "nearest"]), rng)
    # prefilter=False
    X, D, rng = _case((20, 22), (4, 4), 1.5, 502)
    _check(X, D, dict(order=3, mode="reflect", prefilter=False), rng)
    # a dense grid along the last axis (more than 13 points)
    X, D, rng = _case((16, 60), (4, 20), 0.6, 503)
    _check(X, D, dict(order=3, mode="mirror"), rng)


def test_order_zero_is_exactly_zero():
    X, D, rng = _case((20, 22), (4, 4), 1.5, 600)
    g = ed.deform_grid_displacement_gradient(X, rng.standard_normal(X.shape), D, order=0, mode="mirror")
    assert np.array_equal(g, np.zeros_like(D))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_float32_against_float64():
    rng = np.random.default_rng(700)
    X = rng.standard_normal((64, 64, 64))
    dY = rng.standard_normal(X.shape)
    D = rng.standard_normal((3, 5, 5, 5)) * 3
    g64 = ed.deform_grid_displacement_gradient(X, dY, D, order=3, mode="mirror")
    g32 = ed.deform_grid_displacement_gradient(X.astype(np.float32), dY.astype(np.float32), D, order=3,
                                               mode="mirror")
    assert np.linalg.norm(g32 - g64) <= 1e-4 * np.linalg.norm(g64)


def test_composition_float64():
    rng = np.random.default_rng(800)
    X1, X2 = rng.standard_normal((30, 34)), rng.standard_normal((30, 34))
    D = rng.standard_normal((2, 4, 5)) * 2
    d1, d2 = rng.standard_normal(X1.shape), rng.standard_normal(X1.shape)
    kw = dict(order=[3, 2], mode=["mirror", "reflect"])
    both = ed.deform_grid_displacement_gradient([X1, X2], [d1, d2], D, **kw)
    one = ed.deform_grid_displacement_gradient(X1, d1, D, order=3, mode="mirror")
    two = ed.deform_grid_displacement_gradient(X2, d2, D, order=2, mode="reflect")
    np.testing.assert_allclose(both, one + two, rtol=0, atol=1e-12 * np.abs(both).max())

    # a channel axis = the sum over channels
    Xc, dc = rng.standard_normal((30, 34, 3)), rng.standard_normal((30, 34, 3))
    allc = ed.deform_grid_displacement_gradient(Xc, dc, D, order=3, mode="mirror", axis=(0, 1))
    per = sum(ed.deform_grid_displacement_gradient(np.ascontiguousarray(Xc[..., c]), np.ascontiguousarray(dc[..., c]),
                                                   D, order=3, mode="mirror") for c in range(3))
    np.testing.assert_allclose(allc, per, rtol=0, atol=1e-12 * np.abs(allc).max())

    # a crop = the full call with dY zero outside the crop
    crop = (slice(4, 25), slice(6, 30))
    dcrop = rng.standard_normal((21, 24))
    got = ed.deform_grid_displacement_gradient(X1, dcrop, D, order=3, mode="mirror", crop=crop)
    dfull = np.zeros(X1.shape)
    dfull[crop] = dcrop
    full = ed.deform_grid_displacement_gradient(X1, dfull, D, order=3, mode="mirror")
    np.testing.assert_allclose(got, full, rtol=0, atol=1e-12 * np.abs(full).max())

    # the RAW result = the transposed grid filter of the prefiltered-grid result
    Df = orc._prefilter_displacement(D)
    with torch.cuda.device(0):
        Xt = _dev(orc.spline_filter1d(orc.spline_filter1d(X1, 3, 0), 3, 1))
        dYt, Dft = _dev(d1), _dev(Df)
        dP = torch.empty(D.shape, dtype=torch.float64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        _lib.deform_displacement_gradient([_lib.describe(Xt.data_ptr(), "float64", Xt.shape, [8 * v for v in Xt.stride()])],
                                          _lib.describe(Dft.data_ptr(), "float64", Dft.shape, [8 * v for v in Dft.stride()]),
                                          None, [_lib.describe(dYt.data_ptr(), "float64", dYt.shape, [8 * v for v in dYt.stride()])],
                                          [(0, 1)], [3], [3], [0.0], None,
                                          _lib.describe(dP.data_ptr(), "float64", dP.shape, [8 * v for v in dP.stride()]),
                                          0, s)
        torch.cuda.synchronize()
    dP = dP.cpu().numpy()
    for ax in (1, 2):
        out = np.zeros_like(dP)
        orc.spline_filter1d_grad(dP, out, ax, 3)
        dP = out
    np.testing.assert_allclose(one, dP, rtol=0, atol=1e-12 * np.abs(one).max())


def test_batch_equals_single_and_repeat_calls_are_bit_identical():
    rng = np.random.default_rng(900)
    with torch.cuda.device(0):
        X = _dev(rng.standard_normal((3, 40, 36, 44)).astype(np.float32))
        D = _dev(rng.standard_normal((3, 3, 4, 4, 5)) * 3)
        dY = _dev(rng.standard_normal((3, 40, 36, 44)).astype(np.float32))
        gb = ed.deform_grid_displacement_gradient_batch(X, dY, D, order=3, mode="mirror")
        for b in range(3):
            gs = ed.deform_grid_displacement_gradient(X[b], dY[b], D[b], order=3, mode="mirror")
            assert torch.equal(gb[b], gs)
        X = _dev(rng.standard_normal((128, 128, 128)).astype(np.float32))
        dY = _dev(rng.standard_normal((128, 128, 128)).astype(np.float32))
        D = _dev(rng.standard_normal((3, 5, 5, 5)) * 5)
        a = ed.deform_grid_displacement_gradient(X, dY, D, order=3, mode="mirror")
        b = ed.deform_grid_displacement_gradient(X, dY, D, order=3, mode="mirror")
        assert torch.equal(a, b) and a.dtype == torch.float64 and a.device == X.device


def test_torch_gradcheck_single_and_batch():
    # (nondet_tol: the X gradient's scatter adds with atomics in a varying order; the displacement gradient is
    # bit-reproducible, test_batch_equals_single_and_repeat_calls_are_bit_identical)
    rng = np.random.default_rng(1000)
    with torch.cuda.device(0):
        for shape, ncp in (((9, 11), (3, 3)), ((6, 7, 5), (3, 3, 3))):
            X = _dev(rng.standard_normal(shape)).requires_grad_()
            D = _dev(rng.standard_normal((len(shape),) + ncp) * 0.8).requires_grad_()
            assert torch.autograd.gradcheck(
                lambda x, d: etorch.deform_grid(x, d, order=3, mode="mirror", displacement_grad=True), (X, D),
                eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=1e-12)
        Xb = _dev(rng.standard_normal((2, 8, 9))).requires_grad_()
        Db = _dev(rng.standard_normal((2, 2, 3, 3)) * 0.8).requires_grad_()
        assert torch.autograd.gradcheck(
            lambda x, d: etorch.deform_grid_batch(x, d, order=3, mode="mirror", displacement_grad=True), (Xb, Db),
            eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=1e-12)


def test_torch_default_keeps_displacement_grad_none():
    rng = np.random.default_rng(1100)
    with torch.cuda.device(0):
        X = _dev(rng.standard_normal((16, 18))).requires_grad_()
        D = _dev(rng.standard_normal((2, 3, 3))).requires_grad_()
        etorch.deform_grid(X, D, order=3, mode="mirror").sum().backward()
        assert X.grad is not None and D.grad is None
        Xb = _dev(rng.standard_normal((2, 16, 18))).requires_grad_()
        Db = _dev(rng.standard_normal((2, 2, 3, 3))).requires_grad_()
        etorch.deform_grid_batch(Xb, Db, order=3, mode="mirror").sum().backward()
        assert Xb.grad is not None and Db.grad is None
        # with the opt-in: on the displacement's device, in its dtype
        Dc = torch.from_numpy(rng.standard_normal((2, 3, 3))).float().requires_grad_()
        etorch.deform_grid(X, Dc, order=3, mode="mirror", displacement_grad=True).sum().backward()
        assert Dc.grad is not None and Dc.grad.device.type == "cpu" and Dc.grad.dtype == torch.float32


def test_graph_capture_replay_matches_eager():
    rng = np.random.default_rng(1200)
    with torch.cuda.device(0):
        Xs = _dev(rng.standard_normal((20, 24, 28)).astype(np.float32))
        dYs = _dev(rng.standard_normal((20, 24, 28)).astype(np.float32))
        Ds = _dev(rng.standard_normal((3, 4, 4, 4)) * 2)
        Xo = _dev(rng.standard_normal((33, 30, 40)).astype(np.float32))
        dYo = _dev(rng.standard_normal((33, 30, 40)).astype(np.float32))
        Do = _dev(rng.standard_normal((3, 5, 4, 5)) * 2)

        def f():
            return ed.deform_grid_displacement_gradient(Xs, dYs, Ds, order=3, mode="mirror")

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                f()                              # warm the capture stream's workspace
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = f()
        for i in range(3):
            Xs.copy_(_dev(rng.standard_normal((20, 24, 28)).astype(np.float32)))
            Ds.copy_(_dev(rng.standard_normal((3, 4, 4, 4)) * 2))
            other = ed.deform_grid_displacement_gradient(Xo, dYo, Do, order=3, mode="mirror")
            g.replay()
            torch.cuda.synchronize()
            want = f()
            assert torch.equal(out, want), i
            assert torch.equal(other, ed.deform_grid_displacement_gradient(Xo, dYo, Do, order=3, mode="mirror"))


def test_cfg2_size_float32_against_float64():
    rng = np.random.default_rng(1300)
    with torch.cuda.device(0):
        X = torch.rand((256, 256, 256), device="cuda", dtype=torch.float32)
        dY = torch.rand((256, 256, 256), device="cuda", dtype=torch.float32)
        D = _dev(rng.standard_normal((3, 5, 5, 5)) * 5)
        g32 = ed.deform_grid_displacement_gradient(X, dY, D, order=3, mode="mirror")
        g64 = ed.deform_grid_displacement_gradient(X.double(), dY.double(), D, order=3, mode="mirror")
        assert torch.linalg.norm(g32 - g64) <= 1e-4 * torch.linalg.norm(g64)


def test_registration_end_to_end():
    torch.manual_seed(0)
    rng = np.random.default_rng(1400)
    with torch.cuda.device(0):
        n = 48
        z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
        vol = np.zeros((n, n, n))
        for _ in range(6):
            c = rng.uniform(12, 36, 3)
            vol += np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * 5.0 ** 2))
        X = _dev(vol.astype(np.float32))
        D_true = _dev(rng.standard_normal((3, 4, 4, 4)) * 1.5).float()
        Y = ed.deform_grid(X, D_true, order=3, mode="nearest")
        D = torch.zeros_like(D_true, requires_grad=True)
        opt = torch.optim.Adam([D], lr=0.1)
        losses = []
        for _ in range(200):
            opt.zero_grad()
            loss = ((etorch.deform_grid(X, D, order=3, mode="nearest", displacement_grad=True) - Y) ** 2).sum()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        assert losses[-1] <= losses[0] / 10, (losses[0], losses[-1])
