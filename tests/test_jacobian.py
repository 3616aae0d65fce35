"""
GPU tests of det J on the voxel lattice and of its gradients (elasticdeform_amd.deform_grid_jacobian,
deform_grid_jacobian_gradient, their batch forms, elasticdeform_amd.torch.deform_grid_jacobian; edhip_deform_jacobian,
edhip_deform_jacobian_gradient).

Expected values come from tests/jacobian_reference.py (NumPy on oracle/dgrad_reference.py, anchored against central
differences on the CPU in tests/test_jacobian_reference_host.py) and from numpy.linalg.det of the Jacobians that
deform_grid_coordinates returns on the voxel lattice (another kernel: a 4^n-tap sum per point).

Bounds:
* det: 512 eps B per voxel, B = prod_h (sum_l |K[h, l]| + 1.5 max|P[h]| sum_l s_l), which bounds every product in the
  determinant (sum_t |w'_t| <= 1.5); 512 exceeds the roundings of a 64-tap, 4-factor sum per entry plus the
  determinant's own.
* displacement / inverse_map: 1024 eps A, A the absolute-value sum of the entry's terms (the reference's A_D, A_K).
* affine / rotate / zoom: 1e-6 max(1, |value|), the central-difference bound of the reference's own check.
The shapes are the smallest at which the kernels can go wrong: odd sizes, crops, every tap folded, voxels on knots, a
row longer than two waves, a volume smaller than a tile, non-deformed axes, grids read from global memory, a last grid
axis beyond the row contraction.
"""
import functools
import math

import numpy as np
import pytest

from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402

import jacobian_reference as jref  # noqa: E402

EPS = np.finfo(np.float64).eps
AFFINE2 = np.array([[1.1, 0.15, -1.5], [-0.1, 0.9, 2.0]])
AFFINE3 = np.array([[1.05, 0.1, 0.0, -1.0], [-0.08, 0.95, 0.05, 0.5], [0.02, -0.04, 1.1, 1.5]])

CASES = {
    "1d": dict(X=(40,), ncp=(5,), sigma=2.0),
    "2d-crop": dict(X=(13, 17), ncp=(4, 5), sigma=3.0, crop=(slice(2, 11), slice(3, 15))),
    "3d": dict(X=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5),
    "3d-affine-crop": dict(X=(24, 28, 20), ncp=(4, 4, 4), sigma=0.5, crop=(slice(2, 22), slice(3, 27), slice(0, 18)),
                           affine=AFFINE3),
    "2d-rotate-zoom-crop": dict(X=(40, 52), ncp=(5, 5), sigma=2.0, rotate=20.0, zoom=1.3,
                                crop=(slice(4, 36), slice(6, 50))),
    "3d-two-points": dict(X=(9, 9, 9), ncp=(2, 2, 2), sigma=1.0),            # every tap folds
    "3d-knots": dict(X=(9, 9, 9), ncp=(5, 3, 2), sigma=1.0),                 # voxels on knots
    "3d-long-row": dict(X=(5, 6, 150), ncp=(3, 3, 7), sigma=1.0),            # longer than two waves, no multiple of 64
    "3d-tiny": dict(X=(2, 2, 2), ncp=(3, 3, 3), sigma=0.5),
    "3d-axis": dict(X=(3, 10, 12, 8), ncp=(3, 4, 3), sigma=1.0, axis=(1, 2, 3)),
    "2d-global-grid": dict(X=(70, 70), ncp=(64, 64), sigma=0.5),             # 8192 grid values, more than 7680
    "3d-global-grid": dict(X=(20, 18, 16), ncp=(16, 16, 11), sigma=0.5),     # 8448 grid values
}
# last grid axes whose n n ncp_x values do not fit the forward's row contraction (512): the forward's per-voxel route,
# and units of the gradient that reach a window of the control points only (several units a row)
CASES.update({
    "1d-per-voxel": dict(X=(700,), ncp=(600,), sigma=0.5),
    "2d-wide-grid": dict(X=(20, 300), ncp=(3, 129), sigma=0.5),              # 774 grid values, 516 a row
    "3d-wide-grid": dict(X=(6, 5, 130), ncp=(3, 3, 64), sigma=0.5, crop=(slice(0, 6), slice(1, 5), slice(2, 128))),
    "1d-dense-grid": dict(X=(12,), ncp=(40,), sigma=0.3),                    # more control points than voxels
})
NAMES = list(CASES)


def _case(name, dtype=np.float64):
    c = dict(CASES[name])
    X, ncp, sigma = c.pop("X"), c.pop("ncp"), c.pop("sigma")
    n = len(ncp)
    D = np.random.default_rng(100 + len(name) + 7 * n).standard_normal((n,) + ncp) * sigma
    D = np.round(D).astype(dtype) if np.dtype(dtype).kind == "i" else D.astype(dtype)
    return X, D, c


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(reference with gradients, the cotangent) of a case; computed once, never modified"""
    X, D, kw = _case(name)
    ref0 = jref.reference(D, X, **kw)
    g = np.random.default_rng(7).standard_normal(ref0.det.shape)
    ref = jref.reference(D, X, g, **kw)
    for a in (g, ref.det, ref.dD, ref.dK, ref.A_D, ref.A_K):
        a.setflags(write=False)
    return ref, g


def _bound(X, D, kw):
    """B for a grid of any dtype: P prefiltered in the grid's own dtype, as the library does"""
    n = D.shape[0]
    I, O, off, K = jref.geometry(X, D, **kw)
    P = orc._prefilter_displacement(np.ascontiguousarray(D)).astype(np.float64)
    s = sum((D.shape[k + 1] - 1) / (I[k] - 1) for k in range(n))
    return float(np.prod([np.abs(K[h, :n]).sum() + 1.5 * np.abs(P[h]).max() * s for h in range(n)])), O


# ---- values ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_det_equals_the_reference(name):
    X, D, kw = _case(name)
    ref = _reference(name)[0]
    det = ed.deform_grid_jacobian(D, X, **kw)
    assert isinstance(det, np.ndarray) and det.dtype == np.float64 and det.shape == ref.O
    err = np.abs(det - ref.det).max()
    print("%s: max |det err| %.3g = %.2f eps B, B %.3g, det in [%.3g, %.3g]"
          % (name, err, err / (EPS * ref.B), ref.B, ref.det.min(), ref.det.max()))
    assert err <= 512 * EPS * ref.B


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int16], ids=["float64", "float32", "int16"])
@pytest.mark.parametrize("name", NAMES)
def test_det_equals_the_determinant_of_the_coordinate_jacobian(name, dtype):
    X, D, kw = _case(name, dtype)
    B, O = _bound(X, D, kw)
    det = ed.deform_grid_jacobian(D, X, **kw)
    lattice = np.stack(np.indices(O), axis=-1).astype(np.float64)
    _, J = ed.deform_grid_coordinates(lattice, D, X, jacobian=True, **kw)
    want = np.linalg.det(J)
    assert det.shape == want.shape == tuple(O)
    err = np.abs(det - want).max()
    print("%s %s: max |det - det J| %.3g = %.2f eps B" % (name, np.dtype(dtype).name, err, err / (EPS * B)))
    assert err <= 512 * EPS * B


@pytest.mark.parametrize("name", ["1d", "2d-crop", "3d-affine-crop", "3d-long-row", "2d-global-grid", "1d-per-voxel"])
def test_float32_output_is_the_float64_output_rounded_once(name):
    X, D, kw = _case(name)
    det = ed.deform_grid_jacobian(D, X, **kw)
    for dtype in ("float32", np.float32):
        det32 = ed.deform_grid_jacobian(D, X, dtype=dtype, **kw)
        assert det32.dtype == np.float32
        np.testing.assert_array_equal(det32, det.astype(np.float32))
    np.testing.assert_array_equal(ed.deform_grid_jacobian(D, X, dtype="float64", **kw), det)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_a_zero_grid(n):
    X = (6, 7, 8)[:n]
    D = np.zeros((n,) + (3,) * n)
    assert np.abs(ed.deform_grid_jacobian(D, X) - 1.0).max() <= 1e-12
    if n > 1:
        A = AFFINE2 if n == 2 else AFFINE3
        K = orc._inverse_affine(A, None, None, n, list(X))
        det = ed.deform_grid_jacobian(D, X, affine=A)
        assert det.shape == X and np.abs(det - np.linalg.det(K[:, :n])).max() <= 1e-12


def test_the_folding_and_the_invertible_field():
    Df = np.random.default_rng(5).standard_normal((2, 5, 5)) * 6.0
    Dm = np.random.default_rng(12).standard_normal((2, 5, 5)) * 2.0
    assert jref.reference(Df, (32, 32)).det.min() < 0
    assert jref.reference(Dm, (40, 52)).det.min() > 0.2
    fold, mild = ed.deform_grid_jacobian(Df, (32, 32)), ed.deform_grid_jacobian(Dm, (40, 52))
    print("folding field: min det %.3f; invertible field: min det %.3f" % (fold.min(), mild.min()))
    assert fold.min() < 0
    assert mild.min() > 0.2


# ---- independence ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, crop", [
    ("1d", (slice(3, 38),)),
    ("2d-crop", (slice(2, 11), slice(3, 15))),
    ("3d", (slice(1, 9), slice(0, 14), slice(2, 7))),
    ("3d-long-row", (slice(1, 4), slice(2, 6), slice(7, 149))),
    ("3d-axis", (slice(0, 10), slice(5, 6), slice(1, 8))),
    ("3d-global-grid", (slice(3, 20), slice(0, 17), slice(5, 6))),          # a row of one voxel
    ("1d-per-voxel", (slice(100, 699),)),
])
def test_a_crop_gives_the_bits_of_the_whole_lattice(name, crop):
    X, D, kw = _case(name)
    kw.pop("crop", None)
    full = ed.deform_grid_jacobian(D, X, **kw)
    part = ed.deform_grid_jacobian(D, X, crop=crop, **kw)
    assert part.shape == full[crop].shape
    np.testing.assert_array_equal(part, full[crop])


@pytest.mark.parametrize("name", ["1d", "2d-rotate-zoom-crop", "3d-affine-crop", "3d-long-row", "2d-global-grid"])
def test_a_batch_equals_the_single_calls(name):
    X, D, kw = _case(name)
    rng = np.random.default_rng(3)
    Db = np.stack([D, -0.5 * D, rng.standard_normal(D.shape)])
    detb = ed.deform_grid_jacobian_batch(Db, X, **kw)
    gb = rng.standard_normal(detb.shape)
    rb = ed.deform_grid_jacobian_gradient_batch(gb, Db, X, **kw)
    assert isinstance(rb, ed.JacobianGradient) and rb.displacement.shape == Db.shape
    singles = []
    for b in range(3):
        np.testing.assert_array_equal(detb[b], ed.deform_grid_jacobian(Db[b], X, **kw))
        r = ed.deform_grid_jacobian_gradient(gb[b], Db[b], X, **kw)
        np.testing.assert_array_equal(rb.displacement[b], r.displacement)
        singles.append(r)
    assert not np.array_equal(detb[0], detb[1])
    for field in ("affine", "rotate", "zoom", "inverse_map"):
        got = getattr(rb, field)
        if getattr(singles[0], field) is None:
            assert got is None
            continue
        total = getattr(singles[0], field)
        for r in singles[1:]:
            total = total + getattr(r, field)
        np.testing.assert_array_equal(np.asarray(got), np.asarray(total))


def test_repeats_and_graph_replays_give_the_same_bits():
    """a second call, and three replays of a captured graph (forward and gradient on a side stream, after a warm-up
    there) interleaved with eager calls of another shape, give the bits of the first calls -- for both shapes"""
    X, D, kw = _case("3d-affine-crop")
    X2, D2, kw2 = _case("2d-crop")
    Dt, D2t = torch.from_numpy(D).cuda(), torch.from_numpy(D2).cuda()
    det0 = ed.deform_grid_jacobian(Dt, X, **kw)
    g = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(det0.shape))).cuda()
    r0 = ed.deform_grid_jacobian_gradient(g, Dt, X, **kw)
    other0 = ed.deform_grid_jacobian(D2t, X2, **kw2)
    g2 = torch.from_numpy(np.random.default_rng(6).standard_normal(tuple(other0.shape))).cuda()
    o0 = ed.deform_grid_jacobian_gradient(g2, D2t, X2, **kw2)
    assert torch.equal(ed.deform_grid_jacobian(Dt, X, **kw), det0)
    again = ed.deform_grid_jacobian_gradient(g, Dt, X, **kw)
    assert torch.equal(again.displacement, r0.displacement) and torch.equal(again.inverse_map, r0.inverse_map)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ed.deform_grid_jacobian(Dt, X, **kw)                       # the warm-up sizes the capture stream's workspace
        ed.deform_grid_jacobian_gradient(g, Dt, X, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        det = ed.deform_grid_jacobian(Dt, X, **kw)
        r = ed.deform_grid_jacobian_gradient(g, Dt, X, **kw)
    for _ in range(3):
        det.zero_()
        r.displacement.zero_()
        graph.replay()
        other = ed.deform_grid_jacobian(D2t, X2, **kw2)
        o = ed.deform_grid_jacobian_gradient(g2, D2t, X2, **kw2)
        torch.cuda.synchronize()
        assert torch.equal(det, det0) and torch.equal(r.displacement, r0.displacement)
        assert torch.equal(r.inverse_map, r0.inverse_map) and torch.equal(r.affine, r0.affine)
        assert torch.equal(other, other0) and torch.equal(o.displacement, o0.displacement)
        assert torch.equal(o.inverse_map, o0.inverse_map)


@pytest.mark.parametrize("name", ["2d-rotate-zoom-crop", "3d-long-row"])
def test_a_float32_cotangent_is_widened(name):
    X, D, kw = _case(name)
    g32 = _reference(name)[1].astype(np.float32)
    a = ed.deform_grid_jacobian_gradient(g32, D, X, **kw)
    b = ed.deform_grid_jacobian_gradient(g32.astype(np.float64), D, X, **kw)
    np.testing.assert_array_equal(a.displacement, b.displacement)
    np.testing.assert_array_equal(a.inverse_map, b.inverse_map)
    # a transposed (non-contiguous) cotangent: the same bits
    gt = np.ascontiguousarray(np.moveaxis(g32, 0, -1))
    c = ed.deform_grid_jacobian_gradient(np.moveaxis(gt, -1, 0), D, X, **kw)
    np.testing.assert_array_equal(c.displacement, a.displacement)


# ---- gradient -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_gradient_equals_the_reference(name):
    X, D, kw = _case(name)
    ref, g = _reference(name)
    n = D.shape[0]
    r = ed.deform_grid_jacobian_gradient(g, D, X, **kw)
    assert isinstance(r, ed.JacobianGradient)
    assert r.displacement.shape == D.shape and r.displacement.dtype == np.float64
    reached = ref.A_D > 0
    ratio = np.abs(r.displacement - ref.dD)[reached] / (EPS * ref.A_D[reached])
    print("%s: displacement worst %.2f eps A_D; max |dD| %.3g" % (name, ratio.max(initial=0.0), np.abs(ref.dD).max()))
    assert (np.abs(r.displacement - ref.dD) <= 1024 * EPS * ref.A_D).all()
    assert r.inverse_map.shape == (n, n + 1)
    assert (np.abs(r.inverse_map - ref.dK) <= 1024 * EPS * ref.A_K).all()
    assert not r.inverse_map[:, n].any()
    # without an affine map: the gradient at the identity, shape (n, n + 1)
    A = kw.get("affine", np.concatenate([np.eye(n), np.zeros((n, 1))], axis=1))
    d_aff, d_rot, d_zoom = jref.parameter_gradients(ref.dK, ref.O, A, kw.get("rotate"), kw.get("zoom"))
    assert r.affine.shape == d_aff.shape
    assert (np.abs(r.affine - d_aff) <= 1e-6 * np.maximum(1.0, np.abs(d_aff))).all()
    for got, want in ((r.rotate, d_rot), (r.zoom, d_zoom)):
        if want is None:
            assert got is None
        else:
            print("%s: got %.9g, reference %.9g" % (name, got, want))
            assert abs(got - want) <= 1e-6 * max(1.0, abs(want))


@pytest.mark.parametrize("name", ["2d-rotate-zoom-crop", "3d-affine-crop"])
def test_affine_parameters_together(name):
    """affine with rotate and zoom (2-D), and a homogeneous affine: against the reference's chain rule"""
    X, D, kw = _case(name)
    if len(X) == 2:
        kw["affine"] = np.concatenate([AFFINE2, [[0.0, 0.0, 1.0]]])
    ref0 = jref.reference(D, X, **kw)
    g = np.random.default_rng(11).standard_normal(ref0.det.shape)
    ref = jref.reference(D, X, g, **kw)
    r = ed.deform_grid_jacobian_gradient(g, D, X, **kw)
    A = kw["affine"]
    d_aff, d_rot, d_zoom = jref.parameter_gradients(ref.dK, ref.O, A[:len(X)], kw.get("rotate"), kw.get("zoom"))
    assert r.affine.shape == A.shape
    got = np.asarray(r.affine)[:len(X)]
    assert (np.abs(got - d_aff) <= 1e-6 * np.maximum(1.0, np.abs(d_aff))).all()
    if d_rot is not None:
        assert abs(r.rotate - d_rot) <= 1e-6 * max(1.0, abs(d_rot))
        assert abs(r.zoom - d_zoom) <= 1e-6 * max(1.0, abs(d_zoom))


@pytest.mark.parametrize("name", ["2d-crop", "3d-affine-crop", "3d-long-row", "3d-global-grid", "2d-wide-grid",
                                  "3d-wide-grid"])
def test_gradient_equals_step_one_differences_of_the_forward(name):
    """the two kernels against each other: det is affine in every single D[h, j], so the central difference with
    step 1 of L = sum g det, from two forward calls, is the gradient entry up to rounding"""
    X, D, kw = _case(name)
    ref, g = _reference(name)
    r = ed.deform_grid_jacobian_gradient(g, D, X, **kw)
    rng = np.random.default_rng(21)
    for _ in range(5):
        idx = tuple(int(rng.integers(0, s)) for s in D.shape)
        Dp, Dm = D.copy(), D.copy()
        Dp[idx] += 1.0
        Dm[idx] -= 1.0
        diff = ed.deform_grid_jacobian(Dp, X, **kw) - ed.deform_grid_jacobian(Dm, X, **kw)
        quotient = math.fsum((g * diff).reshape(-1)) / 2.0
        err = abs(quotient - r.displacement[idx])
        print("%s %s: quotient %.12g, gradient %.12g, %.2f eps A_D"
              % (name, idx, quotient, r.displacement[idx], err / (EPS * ref.A_D[idx])))
        assert err <= 1024 * EPS * ref.A_D[idx]


@pytest.mark.parametrize("name", ["1d-per-voxel", "3d-wide-grid"])
def test_backward_on_a_grid_beyond_the_row_contraction(name):
    """what the forward accepts, backward serves: the gradient has no limit on the last grid axis"""
    X, D, kw = _case(name)
    ref, g = _reference(name)
    Dt = torch.from_numpy(D).cuda().requires_grad_(True)
    det = etorch.deform_grid_jacobian(Dt, X, displacement_grad=True, **kw)
    (det * torch.from_numpy(np.array(g)).cuda()).sum().backward()
    assert (np.abs(Dt.grad.cpu().numpy() - ref.dD) <= 1024 * EPS * ref.A_D).all()


def test_result_dtypes_and_families():
    X, D, kw = _case("2d-crop")
    ref, g = _reference("2d-crop")
    r = ed.deform_grid_jacobian_gradient(g, D, X, **kw)
    r32 = ed.deform_grid_jacobian_gradient(g, D.astype(np.float32), X, **kw)
    assert r32.displacement.dtype == np.float32 and r32.inverse_map.dtype == np.float64
    Dt, gt = torch.from_numpy(D).cuda(), torch.from_numpy(np.array(g)).cuda()
    det = ed.deform_grid_jacobian(Dt, X, **kw)
    assert torch.is_tensor(det) and det.device == Dt.device and det.dtype == torch.float64
    rt = ed.deform_grid_jacobian_gradient(gt, Dt, X, **kw)
    for t in (rt.displacement, rt.affine, rt.inverse_map):
        assert torch.is_tensor(t) and t.device == Dt.device and t.dtype == torch.float64
    np.testing.assert_array_equal(rt.displacement.cpu().numpy(), r.displacement)
    np.testing.assert_array_equal(rt.inverse_map.cpu().numpy(), r.inverse_map)
    # a numpy cotangent with a device grid stays numpy; a CPU tensor comes back as a CPU tensor
    assert isinstance(ed.deform_grid_jacobian_gradient(g, Dt, X, **kw).displacement, np.ndarray)
    dc = ed.deform_grid_jacobian(torch.from_numpy(D), X, **kw)
    assert torch.is_tensor(dc) and dc.device.type == "cpu"
    np.testing.assert_array_equal(dc.numpy(), det.cpu().numpy())
    assert etorch.deform_grid_jacobian_batch is ed.deform_grid_jacobian_batch
    assert etorch.deform_grid_jacobian_gradient_batch is ed.deform_grid_jacobian_gradient_batch


def test_length_one_axis():
    Dt = torch.zeros((2, 3, 3), dtype=torch.float64, device="cuda")
    det = ed.deform_grid_jacobian(Dt, (1, 9))
    assert det.device == Dt.device and tuple(det.shape) == (1, 9) and bool(torch.isnan(det).all())
    r = ed.deform_grid_jacobian_gradient(torch.ones((9, 1), dtype=torch.float32, device="cuda"), Dt, (9, 1))
    assert r.displacement.device == Dt.device and not bool(r.displacement.any()) and not bool(r.inverse_map.any())


# ---- torch ----------------------------------------------------------------------------------------------------------

def _folding():
    return torch.from_numpy(np.random.default_rng(5).standard_normal((2, 5, 5)) * 6.0).cuda(), (32, 32)


def test_autograd_of_a_folding_penalty():
    D, X = _folding()
    D.requires_grad_(True)
    det = etorch.deform_grid_jacobian(D, X, displacement_grad=True)
    assert det.requires_grad and bool((det < 0).any())
    penalty = torch.relu(-det).sum()
    penalty.backward()
    want = ed.deform_grid_jacobian_gradient(-(det.detach() < 0).to(torch.float64), D.detach(), X).displacement
    assert D.grad.dtype == D.dtype and D.grad.device == D.device
    assert torch.equal(D.grad, want)
    assert bool(D.grad.abs().max() > 0)


def test_no_graph_without_the_switches():
    D, X = _folding()
    D.requires_grad_(True)
    A = torch.tensor(AFFINE2, requires_grad=True)
    det = etorch.deform_grid_jacobian(D, X, affine=A)
    assert not det.requires_grad and det.grad_fn is None
    np.testing.assert_array_equal(det.cpu().numpy(),
                                  ed.deform_grid_jacobian(D.detach().cpu().numpy(), X, affine=AFFINE2))
    # numpy stays numpy
    assert isinstance(etorch.deform_grid_jacobian(D.detach().cpu().numpy(), X), np.ndarray)
    # the displacement's switch alone does not reach the affine map, and the other way round
    det = etorch.deform_grid_jacobian(D, X, affine=A, displacement_grad=True)
    det.sum().backward()
    assert D.grad is not None and A.grad is None


def test_autograd_reaches_the_affine_map():
    D, X = _folding()
    A = torch.tensor(AFFINE2, dtype=torch.float32, requires_grad=True)          # a CPU tensor, float32
    rot = torch.tensor(12.0, dtype=torch.float64, device="cuda", requires_grad=True)
    det = etorch.deform_grid_jacobian(D, X, affine=A, rotate=rot, affine_grad=True)
    g = torch.from_numpy(np.random.default_rng(8).standard_normal(tuple(det.shape))).cuda()
    (det * g).sum().backward()
    want = ed.deform_grid_jacobian_gradient(g, D, X, affine=A.detach().double().numpy(), rotate=12.0)
    assert A.grad.dtype == torch.float32 and A.grad.device.type == "cpu" and A.grad.shape == A.shape
    assert torch.equal(A.grad, want.affine.cpu().to(torch.float32))
    assert rot.grad.dtype == torch.float64 and rot.grad.device == rot.device
    assert torch.equal(rot.grad, want.rotate.reshape(()))
    assert D.grad is None


def test_a_step_against_the_gradient_lowers_the_penalty():
    """the descent property, with no tuned number: halve a step along -D.grad, at most 20 times, until the penalty is
    lower than before"""
    D, X = _folding()
    D.requires_grad_(True)

    def penalty(d):
        return torch.relu(-etorch.deform_grid_jacobian(d, X, displacement_grad=True)).sum()

    first = penalty(D)
    first.backward()
    before = float(first.detach())
    step, lowered = 1.0, False
    for _ in range(20):
        after = float(penalty((D - step * D.grad).detach()))
        if after < before:
            lowered = True
            break
        step *= 0.5
    print("penalty %.6g -> %.6g at step %.3g" % (before, after, step))
    assert lowered
