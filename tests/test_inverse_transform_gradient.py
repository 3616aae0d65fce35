"""
GPU tests of deform_grid_inverse_displacement_gradient / deform_grid_inverse_affine_gradient, their batch forms
(edhip_deform_inverse_transform_gradient) and of autograd to the displacement and to affine / rotate / zoom through
deform_grid_inverse.

The reference is tests/inverse_tgrad_reference.py (NumPy / SciPy, anchored against central differences on the CPU in
tests/test_inverse_tgrad_reference_host.py), taken at the positions q that the tested deform_points solves on the
voxel lattice of X with the test's tol and max_iter: the same solver definition as the kernel's.

The assertion is |got - want| <= 2e-10 S per element, for dD and for dK (AffineGradient.inverse_map), S the
absolute-value scale of the same contraction (S_D, S_K of the reference).  Two parts:

* arithmetic, 1e-10 S: the convention of tests/test_points_gradient.py.  An fp64 or 2^-61-resolved sum errs below
  1e-13 of the scale; a wrong tap, fold or sign errs at 1e-3 of it.
* solver difference: two solvers that both stop at |r(q) - p| <= tol differ by at most 2 tol |J^-1|_inf in q
  (tests/test_inverse.py).  The tests pass tol = 1e-12 and the fields are mild (|J^-1|_inf <= 2): 4e-12.  Measured
  with this reference on the CPU (test_share_of_the_solver_difference): a shift of every q_h by +-4e-10 moves no
  element by more than 3.1e-10 S (2d-global-grid at order 3; 1d-affine 4.5e-11, 2d-crop-mild 3.5e-11, 3d-mild
  2.3e-11, 2d-rz 6.3e-11), so 4e-12 moves none by more than 3.1e-12 S: doubling the arithmetic bound leaves 30 times
  that.

The cases are the geometries tests/test_inverse.py asserts mild, with its seeds.  Asserted here on the reference side:
every voxel is solved (deform_points at tol = 1e-12), min det J is the table's, and no q_h lies within 1e-6 of an
integer, a half-integer, 0 or O_h - 1 (where the reference and the kernel could pick different windows or branches of
the boundary map).

A float32 reference is taken on the widened values: float32 dZ widened, and the float32 coefficients the kernel loads,
widened.  With prefilter=True and order > 1 those coefficients are the forward's own prefilter of the float32 Y (the
library's filter, tested on its own): on lines of 64 samples and more its float32 arithmetic is not the CPU oracle's,
and a reference on the oracle's coefficients differs from the kernel by the rounding of a float32 coefficient, 6e-8 S
(measured: 5.9e-8 S on 2d-global-grid, 70 x 70, order 3, against 5e-14 S at most on every other case), which has
nothing to do with the gradient.  float64 references prefilter with the oracle.
"""
import importlib
import functools

import numpy as np
import pytest

import inverse_tgrad_reference as itr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402
from elasticdeform_amd.deform_grid import _sum_in_order  # noqa: E402

MODES = ["nearest", "wrap", "reflect", "mirror", "constant"]
TOL = 1e-12
BOUND = 2e-10
SOLVE = dict(tol=TOL, max_iter=32)


@functools.lru_cache(maxsize=None)
def _solved(name):
    """(q, ok) of deform_points on the voxel lattice of X; the mild conditions asserted once per case"""
    I, O, D, kw, Y, dZ = itr.case(name)
    q, ok = ed.deform_points(itr.lattice(I), D, I, return_converged=True, **SOLVE, **kw)
    assert ok.all(), "%s: %d voxels not solved at tol %.0e" % (name, (~ok).sum(), TOL)
    _, _, _, off, K = itr.geometry(dZ, D, **kw)
    det = float(np.linalg.det(itr.jacobian(q, D, I, off, K)).min())
    print("%s: min det J %.3g" % (name, det))
    assert abs(det - itr.MIN_DET[name]) < 0.005
    for order in (1, 2):                                         # integers, half-integers; 0 and O - 1 in both
        assert not itr.near_boundary(q, O, order).any()
    q.setflags(write=False)
    return q, ok


def _check(got_D, got_K, r, what):
    for name, got, want, S in (("dD", got_D, r.dD, r.S_D), ("dK", got_K, r.dK, r.S_K)):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        share = float((err / np.maximum(S, np.finfo(np.float64).tiny)).max()) if err.any() else 0.0
        print("%s %s: max |got - want| %.3g, largest share of S %.3g, max |want| %.3g"
              % (what, name, float(err.max()), share, float(np.abs(want).max())))
        assert np.abs(want).max() > 0
        assert (err <= BOUND * S).all(), "%s %s" % (what, name)


def _forward_coefficients(Y, order):
    """the coefficients the forward (and the gradient) prefilter a float32 Y to, along every axis: the library's own"""
    api = importlib.import_module("elasticdeform_amd.deform_grid")
    t = torch.from_numpy(Y).cuda()
    with torch.cuda.device(t.device):
        return api._filter_axes(t, range(Y.ndim), order, False, t.device).cpu().numpy()


def _both(Y, dZ, D, **kw):
    dD = ed.deform_grid_inverse_displacement_gradient(Y, dZ, D, **kw)
    ag = ed.deform_grid_inverse_affine_gradient(Y, dZ, D, **kw)
    return dD, ag


# ---- 1. against the reference ------------------------------------------------------------------------------------

REFERENCE_CASES = ([(n, o, m, True) for n in ("2d-crop-mild", "2d-rz") for o in (1, 2, 3, 4, 5) for m in MODES]
                   + [(n, o, m, True) for n in ("1d-affine", "3d-mild", "2d-global-grid") for o in (1, 3) for m in MODES]
                   + [(n, 3, m, False) for n in itr.CASES for m in ("mirror", "constant")])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name, order, mode, prefilter", REFERENCE_CASES)
def test_gradients_equal_the_reference(name, order, mode, prefilter, dtype):
    I, O, D, kw, Y, dZ = itr.case(name)
    q, ok = _solved(name)
    Y, dZ = Y.astype(dtype), dZ.astype(dtype)
    if dtype == np.float32 and prefilter and order > 1:
        r = itr.reference(_forward_coefficients(Y, order), dZ, D, q, ok, order=order, mode=mode, prefilter=False, **kw)
    else:
        r = itr.reference(Y, dZ, D, q, ok, order=order, mode=mode, prefilter=prefilter, **kw)
    dD, ag = _both(Y, dZ, D, order=order, mode=mode, prefilter=prefilter, **SOLVE, **kw)
    assert isinstance(dD, np.ndarray) and dD.shape == D.shape and dD.dtype == np.float64
    assert ag.inverse_map.shape == (len(I), len(I) + 1)
    _check(dD, ag.inverse_map, r, "%s order %d %s prefilter %s %s" % (name, order, mode, prefilter,
                                                                       np.dtype(dtype).name))


# ---- 2. exact zeros ----------------------------------------------------------------------------------------------

def test_order_0_gives_exact_zeros():
    I, O, D, kw, Y, dZ = itr.case("2d-rz")
    dD, ag = _both(Y, dZ, D, order=0, mode="mirror", **SOLVE, **kw)
    assert dD.shape == D.shape and (dD == 0).all() and (ag.inverse_map == 0).all()
    assert ag.rotate == 0.0 and ag.zoom == 0.0
    # an order-0 input adds nothing to the other inputs' sum
    one = ed.deform_grid_inverse_displacement_gradient(Y, dZ, D, order=3, mode="mirror", **SOLVE, **kw)
    two = ed.deform_grid_inverse_displacement_gradient([Y, Y], [dZ, dZ], D, order=[3, 0], mode="mirror", **SOLVE, **kw)
    assert two.tobytes() == one.tobytes()


def test_the_library_writes_zeros_at_order_0():
    """the C entry itself at order 0: no per-voxel launch, clear and finish leave exact zeros in both results"""
    api = importlib.import_module("elasticdeform_amd.deform_grid")
    I, O, D, kw, Y, dZ = itr.case("2d-crop-mild")
    Yt, Zt, Dt = (torch.from_numpy(a).cuda() for a in (Y, dZ, D))
    dp = torch.full(D.shape, 7.0, dtype=torch.float64, device="cuda")
    dk = torch.full((2, 3), 7.0, dtype=torch.float64, device="cuda")
    api._lib.deform_inverse_transform_gradient(1, api._desc(Yt), 0, api._desc(Zt), 0, api._desc(Dt), 0, I, [2, 3],
                                               api._desc(dp), 0, api._desc(dk), 0, (0, 1), 0, 2, None, None, 32, 1e-9,
                                               0, api._stream(Yt.device))
    torch.cuda.synchronize()
    assert (dp == 0).all() and (dk == 0).all()


def test_a_deformed_axis_of_length_1_gives_zeros():
    D = np.random.default_rng(2).standard_normal((2, 3, 3))
    Y, dZ = np.ones((1, 9)), np.ones((1, 9))
    dD, ag = _both(Y, dZ, D, order=3)
    assert dD.shape == D.shape and (dD == 0).all() and (ag.inverse_map == 0).all()


# ---- 3. a folding field: voxels that are not solved, positions outside Y ------------------------------------------

FOLD_I = (13, 17)
FOLD_KW = dict(max_iter=8)


def _fold():
    D = np.random.default_rng(3).standard_normal((2, 4, 5)) * 4.0
    Y = np.random.default_rng(40).uniform(size=FOLD_I)
    dZ = np.random.default_rng(41).standard_normal(FOLD_I)
    return D, Y, dZ


def test_cotangent_on_unsolved_voxels_only_gives_exact_zeros():
    D, Y, dZ = _fold()
    _, ok = ed.deform_points(itr.lattice(FOLD_I), D, FOLD_I, return_converged=True, **FOLD_KW)
    unsolved = ~ok.reshape(FOLD_I)
    print("unsolved: %d of %d" % (unsolved.sum(), unsolved.size))
    assert 0 < unsolved.sum() < unsolved.size / 2
    for mode in ("nearest", "mirror", "constant"):
        dD, ag = _both(Y, np.where(unsolved, dZ, 0.0), D, order=3, mode=mode, **FOLD_KW)
        assert (dD == 0).all() and (ag.inverse_map == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_nothing_is_nan_on_a_folding_field(mode):
    D, Y, dZ = _fold()
    for order in (1, 3):
        dD, ag = _both(Y, dZ, D, order=order, mode=mode, **FOLD_KW)
        assert np.isfinite(dD).all() and np.isfinite(ag.inverse_map).all() and np.abs(dD).max() > 0


def test_constant_mode_cotangent_where_nothing_is_valid_gives_exact_zeros():
    D, Y, dZ = _fold()
    _, valid = ed.deform_grid_inverse(Y, D, FOLD_I, order=3, mode="constant", return_valid=True, **FOLD_KW)
    assert 0 < (valid == 0).sum() < valid.size
    dD, ag = _both(Y, np.where(valid == 0, dZ, 0.0), D, order=3, mode="constant", **FOLD_KW)
    assert (dD == 0).all() and (ag.inverse_map == 0).all()
    # (the same cotangent does reach the grid in a mode that extends Y)
    assert np.abs(ed.deform_grid_inverse_displacement_gradient(Y, np.where(valid == 0, dZ, 0.0), D, order=3,
                                                               mode="mirror", **FOLD_KW)).max() > 0


# ---- 4. the bit contracts ----------------------------------------------------------------------------------------

def _contract_case():
    I, O, D, kw, Y, dZ = itr.case("2d-crop-mild")
    return I, D, Y, dZ, dict(order=3, mode="mirror", **SOLVE, **kw)


def test_two_calls_give_equal_bits():
    for name in ("2d-crop-mild", "2d-global-grid", "3d-mild"):
        I, O, D, kw, Y, dZ = itr.case(name)
        a, b = (_both(Y, dZ, D, order=3, mode="mirror", **SOLVE, **kw) for _ in range(2))
        assert a[0].tobytes() == b[0].tobytes() and a[1].inverse_map.tobytes() == b[1].inverse_map.tobytes()


def test_a_sample_of_a_batch_equals_the_single_call():
    I, D, Y, dZ, kw = _contract_case()
    rng = np.random.default_rng(50)
    Ds = np.stack([D, -D, 0.5 * D])
    Ys = np.stack([Y, rng.uniform(size=Y.shape), Y[::-1].copy()])
    dZs = np.stack([dZ, rng.standard_normal(dZ.shape), dZ[:, ::-1].copy()])
    db = ed.deform_grid_inverse_displacement_gradient_batch(Ys, dZs, Ds, **kw)
    ab = ed.deform_grid_inverse_affine_gradient_batch(Ys, dZs, Ds, **kw)
    assert db.shape == Ds.shape
    singles = []
    for b in range(3):
        d, a = _both(Ys[b], dZs[b], Ds[b], **kw)
        assert db[b].tobytes() == d.tobytes()
        singles.append(a)
    # the parameters are shared: the batch result is the per-sample ones added in sample order
    for f in ("affine", "inverse_map"):
        assert getattr(ab, f).tobytes() == _sum_in_order([getattr(a, f) for a in singles]).tobytes()


def test_a_nan_cotangent_makes_that_sample_nan_and_no_other():
    I, D, Y, dZ, kw = _contract_case()
    Ds, Ys, dZs = np.stack([D, D, D]), np.stack([Y, Y, Y]), np.stack([dZ, dZ, dZ])
    dZs[1, 5, 6] = np.nan
    clean = ed.deform_grid_inverse_displacement_gradient(Y, dZ, D, **kw)
    db = ed.deform_grid_inverse_displacement_gradient_batch(Ys, dZs, Ds, **kw)
    assert np.isnan(db[1]).all() and db[0].tobytes() == clean.tobytes() and db[2].tobytes() == clean.tobytes()
    ag = ed.deform_grid_inverse_affine_gradient(Y, dZs[1], D, **kw)
    assert np.isnan(ag.inverse_map).all()


def test_capture_into_a_graph():
    I, D, Y, dZ, kw = _contract_case()
    Yt, Zt, Dt = (torch.from_numpy(a).cuda() for a in (Y, dZ, D))
    d0, a0 = _both(Yt, Zt, Dt, **kw)                                           # eager
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _both(Yt, Zt, Dt, **kw)                                                # warm-up: the stream's workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        d, a = _both(Yt, Zt, Dt, **kw)
    for _ in range(3):
        d.fill_(7.0)
        a.inverse_map.fill_(7.0)
        with torch.cuda.stream(side):
            ed.deform_grid_inverse_displacement_gradient(2.0 * Yt, Zt, Dt, **kw)   # an eager call in between
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(d, d0) and torch.equal(a.inverse_map, a0.inverse_map)


# ---- 5. layouts --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("front", [True, False])
def test_two_channels_on_3d(front):
    I, O, D, kw, Y, dZ = itr.case("3d-mild")
    q, ok = _solved("3d-mild")
    rng = np.random.default_rng(60)
    Ys = [Y, rng.uniform(size=O)]
    dZs = [dZ, rng.standard_normal(I)]
    Yc, dZc = np.stack(Ys, axis=0 if front else -1), np.stack(dZs, axis=0 if front else -1)
    axis = (1, 2, 3) if front else (0, 1, 2)
    r = itr.reference(Yc, dZc, D, q, ok, order=3, mode="mirror", axis=axis, **kw)
    dD, ag = _both(Yc, dZc, D, order=3, mode="mirror", axis=axis, **SOLVE, **kw)
    _check(dD, ag.inverse_map, r, "two channels %s" % ("in front" if front else "behind"))


def test_transposed_y_and_cotangent():
    I, D, Y, dZ, kw = _contract_case()
    kw = dict(kw, prefilter=False)                               # (so that the kernel itself reads the strides)
    want_D, want_A = _both(Y, dZ, D, **kw)
    Yt, dZt = np.ascontiguousarray(Y.T).T, np.ascontiguousarray(dZ.T).T
    assert not Yt.flags.c_contiguous and not dZt.flags.c_contiguous
    got_D, got_A = _both(Yt, dZt, D, **kw)
    assert got_D.tobytes() == want_D.tobytes() and got_A.inverse_map.tobytes() == want_A.inverse_map.tobytes()
    want1 = ed.deform_grid_inverse_displacement_gradient(Y, dZ, D, **dict(kw, order=1))
    got1 = ed.deform_grid_inverse_displacement_gradient(torch.from_numpy(np.ascontiguousarray(Y.T)).cuda().T,
                                                        torch.from_numpy(np.ascontiguousarray(dZ.T)).cuda().T,
                                                        torch.from_numpy(D).cuda(), **dict(kw, order=1))
    assert got1.cpu().numpy().tobytes() == want1.tobytes()


def test_list_inputs_equal_the_single_calls_added_in_input_order():
    I, O, D, geo, Y, dZ = itr.case("2d-crop-mild")
    rng = np.random.default_rng(61)
    Yb, dZb = rng.uniform(size=O + (2,)).astype(np.float32), rng.standard_normal(I + (2,)).astype(np.float32)
    kw = dict(SOLVE, **geo)
    d, a = _both([Y, Yb], [dZ, dZb], D, order=[3, 1], mode=["mirror", "constant"], axis=[(0, 1), (0, 1)], **kw)
    d0, a0 = _both(Y, dZ, D, order=3, mode="mirror", **kw)
    d1, a1 = _both(Yb, dZb, D, order=1, mode="constant", axis=(0, 1), **kw)
    assert d.tobytes() == (d0 + d1).tobytes()
    assert a.inverse_map.tobytes() == (a0.inverse_map + a1.inverse_map).tobytes()


def test_numpy_in_numpy_out_tensor_in_tensor_out():
    I, D, Y, dZ, kw = _contract_case()
    d, a = _both(Y, dZ, D, **kw)
    assert isinstance(d, np.ndarray) and isinstance(a.affine, np.ndarray) and isinstance(a.inverse_map, np.ndarray)
    Yt, Zt, Dt = (torch.from_numpy(x).cuda() for x in (Y, dZ, D))
    dt, at = _both(Yt, Zt, Dt, **kw)
    assert torch.is_tensor(dt) and dt.device == Zt.device and dt.dtype == torch.float64 and not dt.requires_grad
    assert torch.is_tensor(at.inverse_map) and at.inverse_map.device == Zt.device
    assert dt.cpu().numpy().tobytes() == d.tobytes() and at.inverse_map.cpu().numpy().tobytes() == a.inverse_map.tobytes()
    # the result's dtype is the displacement's own when that is floating
    d32 = ed.deform_grid_inverse_displacement_gradient(Yt, Zt, Dt.float(), **kw)
    assert d32.dtype == torch.float32
    # Y and dZ of different dtypes: both widened
    dm = ed.deform_grid_inverse_displacement_gradient(Y.astype(np.float32).astype(np.float64), dZ, D,
                                                      **dict(kw, prefilter=False))
    dw = ed.deform_grid_inverse_displacement_gradient(Y.astype(np.float32), dZ, D, **dict(kw, prefilter=False))
    assert dm.tobytes() == dw.tobytes()


def test_rotate_and_zoom_gradients_follow_the_inverse_map():
    """the chain rule to rotate / zoom is _affine_result's: checked against central differences of the call's own L"""
    I, O, D, kw, Y, dZ = itr.case("2d-rz")
    args = dict(order=3, mode="mirror", **SOLVE)

    def L(**p):
        Z = ed.deform_grid_inverse(Y, D, I, crop=kw["crop"], **args, **p)
        return float((Z * dZ).sum())
    ag = ed.deform_grid_inverse_affine_gradient(Y, dZ, D, **args, **kw)
    h = 1e-5
    fd_r = (L(rotate=20 + h, zoom=1.3) - L(rotate=20 - h, zoom=1.3)) / (2 * h)
    fd_z = (L(rotate=20, zoom=1.3 + h) - L(rotate=20, zoom=1.3 - h)) / (2 * h)
    print("rotate %.10g (central difference %.10g), zoom %.10g (%.10g)" % (ag.rotate, fd_r, ag.zoom, fd_z))
    assert abs(ag.rotate - fd_r) <= 1e-5 * abs(fd_r) and abs(ag.zoom - fd_z) <= 1e-5 * abs(fd_z)
    with pytest.raises(ValueError):
        ed.deform_grid_inverse_affine_gradient(Y, dZ, D, crop=kw["crop"], rotate=20, zoom=0, **args)


# ---- 6. autograd -------------------------------------------------------------------------------------------------

def _tensors(name):
    I, O, D, kw, Y, dZ = itr.case(name)
    return I, kw, torch.from_numpy(Y).cuda(), torch.from_numpy(dZ).cuda(), torch.from_numpy(D).cuda()


def test_displacement_and_parameter_grads_equal_the_direct_calls():
    I, kw, Y, dZ, D = _tensors("2d-rz")
    args = dict(order=3, mode="mirror", crop=kw["crop"], **SOLVE)
    D.requires_grad_()
    rot = torch.tensor(20.0, dtype=torch.float64, requires_grad=True)
    zoom = torch.tensor(1.3, dtype=torch.float32, device="cuda", requires_grad=True)
    Z = etorch.deform_grid_inverse(Y, D, I, rotate=rot, zoom=zoom, displacement_grad=True, affine_grad=True, **args)
    assert Z.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(Z, ed.deform_grid_inverse(Y, D, I, rotate=20.0, zoom=float(zoom.detach()), **args))
    Z.backward(dZ)
    zv = float(zoom.detach())
    want_D = ed.deform_grid_inverse_displacement_gradient(Y, dZ, D.detach(), rotate=20.0, zoom=zv, **args)
    want_A = ed.deform_grid_inverse_affine_gradient(Y, dZ, D.detach(), rotate=20.0, zoom=zv, **args)
    assert torch.equal(D.grad, want_D)
    assert rot.grad.device.type == "cpu" and float(rot.grad) == float(want_A.rotate)
    assert zoom.grad.dtype == torch.float32 and zoom.grad.is_cuda
    assert float(zoom.grad) == float(want_A.zoom.to(torch.float32))
    # an affine matrix
    I, kw, Y, dZ, D = _tensors("2d-crop-mild")
    A = torch.tensor([[1.02, 0.03, 0.1], [-0.02, 0.97, -0.2]], dtype=torch.float64, device="cuda", requires_grad=True)
    args = dict(order=3, mode="mirror", crop=kw["crop"], **SOLVE)
    Z = ed.deform_grid_inverse(Y, D, I, affine=A, affine_grad=True, **args)
    Z.backward(dZ)
    want_A = ed.deform_grid_inverse_affine_gradient(Y, dZ, D, affine=A.detach().cpu().numpy(), **args)
    assert A.grad.shape == A.shape and torch.equal(A.grad, want_A.affine)
    assert D.grad is None
    # the batch form: the parameters' gradients are summed over the samples
    Db = torch.stack([D, -D]).requires_grad_()
    A.grad = None
    Zb = ed.deform_grid_inverse_batch(torch.stack([Y, Y]), Db, I, affine=A, displacement_grad=True, affine_grad=True,
                                      **args)
    dZb = torch.stack([dZ, 2.0 * dZ])
    Zb.backward(dZb)
    wb = ed.deform_grid_inverse_displacement_gradient_batch(torch.stack([Y, Y]), dZb, Db.detach(),
                                                            affine=A.detach().cpu().numpy(), **args)
    ab = ed.deform_grid_inverse_affine_gradient_batch(torch.stack([Y, Y]), dZb, Db.detach(),
                                                      affine=A.detach().cpu().numpy(), **args)
    assert torch.equal(Db.grad, wb) and torch.equal(A.grad, ab.affine)


def test_gradcheck_displacement_and_affine():
    I, kw, Y, dZ, D = _tensors("2d-crop-mild")
    args = dict(order=3, mode="mirror", crop=kw["crop"], **SOLVE)
    D.requires_grad_()
    A = torch.tensor([[1.02, 0.03, 0.1], [-0.02, 0.97, -0.2]], dtype=torch.float64, device="cuda", requires_grad=True)

    def f(d):
        return ed.deform_grid_inverse(Y, d, I, displacement_grad=True, **args)

    def g(a):
        return ed.deform_grid_inverse(Y, D.detach(), I, affine=a, affine_grad=True, **args)

    assert torch.autograd.gradcheck(f, (D,), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(g, (A,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_with_both_switches_off_nothing_changes():
    I, kw, Y, dZ, D = _tensors("2d-crop-mild")
    args = dict(order=3, mode="mirror", crop=kw["crop"], **SOLVE)
    D.requires_grad_()
    Z = ed.deform_grid_inverse(Y, D, I, **args)
    assert Z.grad_fn is None and not Z.requires_grad
    with torch.no_grad():
        assert torch.equal(Z, ed.deform_grid_inverse(Y, D, I, **args))
    Yg = Y.clone().requires_grad_()
    Zg = ed.deform_grid_inverse(Yg, D, I, **args)
    assert torch.equal(Zg.detach(), Z)
    Zg.backward(dZ)
    assert D.grad is None and Yg.grad is not None
    assert etorch.deform_grid_inverse is ed.deform_grid_inverse


def test_all_three_gradients_at_once():
    """Y.grad is the image adjoint's own (float atomics: compared as tests/test_inverse_gradient.py compares it)"""
    I, kw, Y, dZ, D = _tensors("2d-crop-mild")
    args = dict(order=3, mode="mirror", crop=kw["crop"], **SOLVE)
    A = torch.tensor([[1.02, 0.03, 0.1], [-0.02, 0.97, -0.2]], dtype=torch.float64, requires_grad=True)
    Y.requires_grad_()
    D.requires_grad_()
    Z, valid = ed.deform_grid_inverse(Y, D, I, affine=A, return_valid=True, displacement_grad=True, affine_grad=True,
                                      **args)
    assert not valid.requires_grad
    Z.backward(dZ)
    An = A.detach().numpy()
    want_Y = ed.deform_grid_inverse_gradient(dZ, D.detach(), affine=An, **args)
    assert float((Y.grad - want_Y).abs().max()) <= 1e-11 * float(want_Y.abs().max())
    assert torch.equal(D.grad, ed.deform_grid_inverse_displacement_gradient(Y.detach(), dZ, D.detach(), affine=An,
                                                                            **args))
    want_A = ed.deform_grid_inverse_affine_gradient(Y.detach(), dZ, D.detach(), affine=An, **args)
    assert torch.equal(A.grad, want_A.affine.cpu())
