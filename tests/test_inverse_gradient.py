"""
GPU tests of deform_grid_inverse_gradient / deform_grid_inverse_gradient_batch (edhip_deform_inverse_gradient) and of
autograd through deform_grid_inverse.

The reference is the tested forward itself.  For fixed deformation arguments and cval = 0, Z = deform_grid_inverse(Y)
is linear in Y, so its matrix is read off the forward: A[p, j] is the result at source voxel p of the unit image j (one
batch call on the |Y| unit images, the grid repeated).  The gradient must be A^T dZ, formed here in extended precision.

The summation bound (tests 1, 4, 6, 7).  The kernel adds, per source voxel p and tap, the term
fl(dZ[p] w_0 ... w_{naxis-1}) into cell j with a float atomic of the accumulator's type:

* the term carries at most naxis roundings of the product in fp64 and one rounding to the accumulator's type:
  naxis + 1 roundings;
* m terms land on the cell, summed in an arrival order nobody fixes: m - 1 roundings on each term at most, whatever the
  order; m is at most (order + 1)^naxis per contributing voxel, c_j (order + 1)^naxis with c_j = #{p: A[p, j] != 0};
* B-spline weights are not negative, so the |terms| of one voxel on one cell add up to |A[p, j]| |dZ[p]|.

Hence |got[j] - (A^T dZ)[j]| <= gamma_n sum_p |A[p, j]| |dZ[p]| with n = c_j (order + 1)^naxis + naxis + 1,
gamma_n = n eps / (1 - n eps) and eps the unit roundoff of the accumulator (2^-53, 2^-24).  The reference adds little
to that: A^T dZ is formed in long double, and A itself carries the forward kernel's fp64 roundings only -- naxis - 1 per
product and f - 1 where f taps of one voxel fold onto the cell (orders >= 2 only, f <= 2^naxis).  With m <= c_j f both
fit under n, m + f + naxis - 3 <= c_j (order + 1)^naxis; at order 0 nothing is multiplied and A is exactly 0 / 1.  For a
float32 accumulator A's own error is 2^-29 of the bound.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402

MODES = ["nearest", "wrap", "reflect", "mirror", "constant"]
EPS = {np.dtype("float64"): 2.0 ** -53, np.dtype("float32"): 2.0 ** -24}
CVAL = 0.25


def _grid(seed, n, ncp, sigma):
    return np.random.default_rng(seed).standard_normal((n,) + tuple(ncp)) * sigma


# name -> (I, control grid, geometry keywords)
CASES = {
    "2d": ((13, 17), _grid(5, 2, (3, 3), 1.5), dict(crop=(slice(2, 11), slice(3, 15)), rotate=20, zoom=1.3)),
    "2d-b1": ((13, 17), _grid(9, 2, (3, 3), 1.5), dict(crop=(slice(2, 11), slice(3, 15)), rotate=20, zoom=1.3)),
    "3d": ((6, 7, 8), _grid(6, 3, (3, 3, 3), 0.5),
           dict(affine=np.array([[1.05, 0.1, 0.0, -0.5], [-0.08, 0.95, 0.05, 0.3], [0.02, -0.04, 1.1, -0.4]]))),
    # a strongly folding field (sigma = the control spacing) and a short iteration: some voxels are not solved
    "fold": ((13, 17), _grid(3, 2, (4, 5), 4.0), dict(max_iter=8)),
    "small": ((7, 8), _grid(8, 2, (3, 3), 0.6), dict()),
}


def _out_shape(name):
    I, _, kw = CASES[name]
    crop = kw.get("crop")
    return tuple(I) if crop is None else tuple((s.stop or i) - (s.start or 0) for s, i in zip(crop, I))


@functools.lru_cache(maxsize=None)
def _matrix(name, order, mode, prefilter=False):
    """A (|X|, |Y|) of deform_grid_inverse with cval = 0, from one batch call on the unit images; computed once"""
    I, D, kw = CASES[name]
    O = _out_shape(name)
    nY = int(np.prod(O))
    units = np.eye(nY).reshape((nY,) + O)
    Z = ed.deform_grid_inverse_batch(units, np.repeat(D[None], nY, axis=0), I, order=order, mode=mode, cval=0.0,
                                     prefilter=prefilter, **kw)
    assert Z.shape == (nY,) + I and Z.dtype == np.float64
    A = np.ascontiguousarray(Z.reshape(nY, -1).T)
    A.setflags(write=False)
    return A


def _cotangent(seed, shape, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


def _want(A, dZ):
    """A^T dZ in extended precision; dZ (|X|,) or (|X|, channels)"""
    return A.T.astype(np.longdouble) @ dZ.astype(np.longdouble)


def _bound(A, dZ, order, naxis):
    """gamma_n sum_p |A[p, j]| |dZ[p]| per cell (the head of the file)"""
    eps = EPS[np.dtype(dZ.dtype)]
    c = (A != 0).sum(axis=0)
    n = (c * (order + 1) ** naxis + naxis + 1).astype(np.float64)
    gamma = n * eps / (1.0 - n * eps)
    s = np.abs(A).T @ np.abs(dZ.astype(np.float64))
    return gamma.reshape((-1,) + (1,) * (s.ndim - 1)) * s


def _check_against_matrix(got, A, dZ, order, naxis, what):
    """got, dZ flattened over the deformed axes: (|Y|[, channels]) and (|X|[, channels])"""
    want, bound = _want(A, dZ), _bound(A, dZ, order, naxis)
    err = np.abs(got.astype(np.longdouble) - want)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.any() else 0.0
    print("%s: max |got - want| %.3g, largest share of the bound %.3g, max |want| %.3g"
          % (what, float(err.max()), worst, float(np.abs(want).max())))
    assert np.abs(want).max() > 0
    assert (err <= bound).all(), what


# ---- 1. the operator matrix from the tested forward --------------------------------------------------------------

MATRIX_CASES = [("2d", o, m) for o in range(6) for m in MODES] + [("3d", o, m) for o in (0, 1, 3) for m in MODES]


def test_every_voxel_of_the_mild_cases_is_solved():
    """the matrix rows of the mild cases are all there: in a mode that never gives cval a row sums to 1"""
    for name in ("2d", "3d", "2d-b1", "small"):
        A = _matrix(name, 1, "mirror")
        np.testing.assert_allclose(A.sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name, order, mode", MATRIX_CASES)
def test_gradient_equals_the_transposed_forward_matrix(name, order, mode, dtype):
    I, D, kw = CASES[name]
    A = _matrix(name, order, mode)
    dZ = _cotangent(11, I, dtype)
    got = ed.deform_grid_inverse_gradient(dZ, D, order=order, mode=mode, prefilter=False, **kw)
    assert isinstance(got, np.ndarray) and got.shape == _out_shape(name) and got.dtype == dtype
    _check_against_matrix(got.reshape(-1), A, dZ.reshape(-1), order, len(I), "%s order %d %s %s"
                          % (name, order, mode, np.dtype(dtype).name))


# ---- 2. with the transposed prefilter ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype, tol", [(np.float64, 1e-11), (np.float32, 1e-5)])
@pytest.mark.parametrize("name, order, mode", [("2d", o, m) for o in (2, 3, 4, 5) for m in MODES]
                         + [("3d", 3, m) for m in MODES])
def test_prefiltered_gradient_equals_the_transposed_forward_matrix(name, order, mode, dtype, tol):
    """A from the forward with prefilter=True: the transposed prefilter against the forward filter.  Tolerance: the
    project's stated one, 1e-11 of max |want| for float64 and 1e-5 for float32"""
    I, D, kw = CASES[name]
    A = _matrix(name, order, mode, True)
    dZ = _cotangent(12, I, dtype)
    got = ed.deform_grid_inverse_gradient(dZ, D, order=order, mode=mode, **kw)
    assert got.shape == _out_shape(name) and got.dtype == dtype
    want = _want(A, dZ.reshape(-1))
    err = float(np.abs(got.reshape(-1).astype(np.longdouble) - want).max())
    print("%s order %d %s %s: max err %.3g of max |want| %.3g" % (name, order, mode, np.dtype(dtype).name, err,
                                                                  float(np.abs(want).max())))
    assert err <= tol * float(np.abs(want).max())


# ---- 3. the exact case -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["2d", "3d"])
def test_order_0_with_integer_cotangents_is_exact(name, mode, dtype):
    """order 0: A is 0 / 1 and every sum of small integers is exact in any order -- the matrix result bit for bit, two
    calls and a batch sample alike"""
    I, D, kw = CASES[name]
    A = _matrix(name, 0, mode)
    assert set(np.unique(A)) <= {0.0, 1.0}
    dZ = np.random.default_rng(13).integers(-8, 9, size=I).astype(dtype)
    want = (A.T @ dZ.reshape(-1).astype(np.float64)).astype(dtype).reshape(_out_shape(name))
    args = dict(order=0, mode=mode, **kw)
    got = ed.deform_grid_inverse_gradient(dZ, D, **args)
    assert got.dtype == dtype and got.tobytes() == want.tobytes()
    assert ed.deform_grid_inverse_gradient(dZ, D, **args).tobytes() == got.tobytes()
    dZb = np.stack([dZ[::-1].copy(), dZ])
    gb = ed.deform_grid_inverse_gradient_batch(dZb, np.stack([D, D]), **args)
    assert gb.shape == (2,) + got.shape and gb[1].tobytes() == got.tobytes()
    assert gb[0].tobytes() == ed.deform_grid_inverse_gradient(dZb[0], D, **args).tobytes()


# ---- 4. a folding field: unsolved voxels -------------------------------------------------------------------------

def _unsolved():
    """the mask of the voxels the forward leaves unsolved: the image of ones in a mode that never gives cval"""
    I, D, kw = CASES["fold"]
    Z, valid = ed.deform_grid_inverse(np.ones(I), D, I, order=1, mode="nearest", cval=0.0, return_valid=True, **kw)
    unsolved = Z == 0.0
    assert (np.abs(Z[~unsolved] - 1.0) < 1e-12).all() and not valid[unsolved].any()
    print("unsolved: %d of %d" % (unsolved.sum(), unsolved.size))
    assert unsolved.sum() > 0, "the field should leave some voxels unsolved"
    assert unsolved.mean() < 0.5, "most voxels should be solved"
    return unsolved


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("mode", ["nearest", "mirror"])
def test_folding_field_matrix_check(order, mode):
    """where only the solved flag can zero a row: the rows of the unsolved voxels are empty, the rest as in test 1"""
    I, D, kw = CASES["fold"]
    unsolved = _unsolved().reshape(-1)
    A = _matrix("fold", order, mode)
    assert (A[unsolved] == 0).all() and (np.abs(A[~unsolved]).sum(axis=1) > 0.5).all()
    dZ = _cotangent(14, I)
    got = ed.deform_grid_inverse_gradient(dZ, D, order=order, mode=mode, prefilter=False, **kw)
    _check_against_matrix(got.reshape(-1), A, dZ.reshape(-1), order, 2, "fold order %d %s" % (order, mode))


@pytest.mark.parametrize("mode", ["nearest", "mirror", "constant"])
def test_cotangent_on_unsolved_voxels_only_gives_exact_zeros(mode):
    I, D, kw = CASES["fold"]
    unsolved = _unsolved()
    dZ = np.where(unsolved, _cotangent(15, I), 0.0)
    assert np.abs(dZ).sum() > 0
    for prefilter in (False, True):
        got = ed.deform_grid_inverse_gradient(dZ, D, order=3, mode=mode, prefilter=prefilter, **kw)
        assert (got == 0).all()


# ---- 5. the dot-product identity where the matrix is too big ------------------------------------------------------

def _dot_identity(I, D, order, mode, seed, channels=None, axis=None, **kw):
    """|<inverse(Y) - inverse(0), dZ> - <Y, dY>| <= 1e-11 sum |Z - Z0| |dZ| (prefilter=True, cval != 0)"""
    ch = () if channels is None else (channels,)
    rng = np.random.default_rng(seed)
    Y = rng.uniform(0.0, 1.0, size=tuple(I) + ch)
    dZ = rng.standard_normal(tuple(I) + ch)
    args = dict(order=order, mode=mode, axis=axis, **kw)
    Z = ed.deform_grid_inverse(Y, D, Y.shape, cval=CVAL, **args)
    Z0 = ed.deform_grid_inverse(np.zeros_like(Y), D, Y.shape, cval=CVAL, **args)
    dY = ed.deform_grid_inverse_gradient(dZ, D, **args)
    assert dY.shape == Y.shape
    lhs, rhs = float(((Z - Z0) * dZ).sum()), float((Y * dY).sum())
    scale = float((np.abs(Z - Z0) * np.abs(dZ)).sum())
    print("order %d %s: <Z - Z0, dZ> %.15g, <Y, dY> %.15g, difference %.3g of %.3g"
          % (order, mode, lhs, rhs, abs(lhs - rhs), scale))
    assert scale > 0 and abs(lhs - rhs) <= 1e-11 * scale


@pytest.mark.parametrize("mode", ["mirror", "constant"])
def test_dot_product_identity_3d_two_channels(mode):
    _dot_identity((12, 13, 14), _grid(16, 3, (4, 4, 5), 0.5), 3, mode, 17, channels=2, axis=(0, 1, 2))


# ---- 6. layouts --------------------------------------------------------------------------------------------------

def test_step_axis_before_the_deformed_axes():
    I, D, kw = CASES["2d"]
    A = _matrix("2d", 3, "mirror")
    dZ = _cotangent(18, (2,) + I)
    got = ed.deform_grid_inverse_gradient(dZ, D, order=3, mode="mirror", prefilter=False, axis=(1, 2), **kw)
    assert got.shape == (2,) + _out_shape("2d")
    _check_against_matrix(got.reshape(2, -1).T, A, dZ.reshape(2, -1).T, 3, 2, "steps first")


def test_step_axis_after_the_deformed_axes():
    I, D, kw = CASES["2d"]
    A = _matrix("2d", 2, "reflect")
    dZ = _cotangent(19, I + (3,))
    got = ed.deform_grid_inverse_gradient(dZ, D, order=2, mode="reflect", prefilter=False, axis=(0, 1), **kw)
    assert got.shape == _out_shape("2d") + (3,)
    _check_against_matrix(got.reshape(-1, 3), A, dZ.reshape(-1, 3), 2, 2, "steps last")


def test_non_contiguous_cotangent():
    I, D, kw = CASES["2d"]
    A = _matrix("2d", 3, "mirror")
    dZt = _cotangent(20, I[::-1])
    dZ = dZt.T                                                   # a transposed view: shape I, strides reversed
    assert not dZ.flags.c_contiguous
    got = ed.deform_grid_inverse_gradient(dZ, D, order=3, mode="mirror", prefilter=False, **kw)
    _check_against_matrix(got.reshape(-1), A, np.ascontiguousarray(dZ).reshape(-1), 3, 2, "transposed numpy")
    gt = ed.deform_grid_inverse_gradient(torch.from_numpy(dZt).cuda().T, D, order=3, mode="mirror", prefilter=False, **kw)
    _check_against_matrix(gt.cpu().numpy().reshape(-1), A, np.ascontiguousarray(dZ).reshape(-1), 3, 2,
                          "transposed tensor")


def test_list_of_two_inputs_with_their_own_order_and_mode():
    I, D, kw = CASES["2d"]
    dZa, dZb = _cotangent(21, I), _cotangent(22, I + (2,), np.float32)
    res = ed.deform_grid_inverse_gradient([dZa, dZb], D, order=[3, 1], mode=["mirror", "constant"], prefilter=False,
                                          axis=[(0, 1), (0, 1)], **kw)
    assert isinstance(res, list) and len(res) == 2
    assert res[0].dtype == np.float64 and res[1].dtype == np.float32 and res[1].shape == _out_shape("2d") + (2,)
    _check_against_matrix(res[0].reshape(-1), _matrix("2d", 3, "mirror"), dZa.reshape(-1), 3, 2, "list input 0")
    _check_against_matrix(res[1].reshape(-1, 2), _matrix("2d", 1, "constant"), dZb.reshape(-1, 2), 1, 2, "list input 1")


def test_numpy_in_numpy_out_tensor_in_tensor_out():
    I, D, kw = CASES["2d"]
    dZ = _cotangent(23, I)
    got = ed.deform_grid_inverse_gradient(dZ, D, **kw)
    assert isinstance(got, np.ndarray)
    dZt = torch.from_numpy(dZ).cuda()
    gt = ed.deform_grid_inverse_gradient(dZt, torch.from_numpy(D).cuda(), **kw)
    assert torch.is_tensor(gt) and gt.device == dZt.device and gt.dtype == torch.float64 and not gt.requires_grad
    np.testing.assert_allclose(gt.cpu().numpy(), got, rtol=0, atol=1e-11 * np.abs(got).max())
    gb = ed.deform_grid_inverse_gradient_batch(torch.stack([dZt, dZt]), torch.from_numpy(np.stack([D, D])).cuda(), **kw)
    assert torch.is_tensor(gb) and gb.device == dZt.device and tuple(gb.shape) == (2,) + _out_shape("2d")


@pytest.mark.parametrize("order, mode", [(3, "mirror"), (1, "constant")])
def test_global_memory_grid_route(order, mode):
    """more than 7680 grid values: the control grid is read from global memory"""
    D = _grid(1, 2, (62, 62), 0.08)
    assert D.size > 7680
    _dot_identity((70, 70), D, order, mode, 24)


# ---- 7. the batch form -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order, mode", [(3, "mirror"), (1, "constant")])
def test_batch_sample_agrees_with_the_single_call(order, mode):
    """the two differ in the order of the adds alone: by twice the sum's share gamma_{m-1} of the bound at most, which
    stays below gamma_n for orders >= 1 (n >= 2 m, the head of the file); each also meets the matrix of its own grid"""
    names = ["2d", "2d-b1"]
    I, _, kw = CASES["2d"]
    Ds = np.stack([CASES[name][1] for name in names])
    dZb = np.stack([_cotangent(30 + b, I) for b in range(2)])
    gb = ed.deform_grid_inverse_gradient_batch(dZb, Ds, order=order, mode=mode, prefilter=False, **kw)
    assert gb.shape == (2,) + _out_shape("2d")
    for b, name in enumerate(names):
        A = _matrix(name, order, mode)
        _check_against_matrix(gb[b].reshape(-1), A, dZb[b].reshape(-1), order, 2, "batch sample %d" % b)
        single = ed.deform_grid_inverse_gradient(dZb[b], Ds[b], order=order, mode=mode, prefilter=False, **kw)
        assert (np.abs(gb[b] - single).reshape(-1) <= _bound(A, dZb[b].reshape(-1), order, 2)).all()


# ---- 8. autograd through deform_grid_inverse ---------------------------------------------------------------------

@pytest.mark.parametrize("order", [1, 3])
def test_gradcheck(order):
    """linear in Y, so eps = 1e-3 is safe.  nondet_tol: the bound of test 1 for a unit cotangent -- a row of A sums to
    1, n <= |X| (order + 1)^2 + 3 -- times 3, the 1-norm of the transposed cubic prefilter over two axes (sqrt(3) each)"""
    I, D, kw = CASES["small"]
    n = I[0] * I[1] * (order + 1) ** 2 + 3
    eps = EPS[np.dtype("float64")]
    nondet = 3.0 * n * eps / (1.0 - n * eps)
    Dt = torch.from_numpy(D).cuda()
    Y = torch.from_numpy(np.random.default_rng(31).uniform(size=I)).cuda().requires_grad_()

    def f(y):
        return ed.deform_grid_inverse(y, Dt, I, order=order, mode="mirror")

    assert torch.autograd.gradcheck(f, (Y,), eps=1e-3, atol=1e-9, nondet_tol=nondet)


def _tensor_case(seed):
    I, D, kw = CASES["2d"]
    Y = torch.from_numpy(np.random.default_rng(seed).uniform(size=_out_shape("2d"))).cuda()
    return I, torch.from_numpy(D).cuda(), kw, Y


def test_grad_equals_the_gradient_call():
    I, Dt, kw, Y = _tensor_case(32)
    Y.requires_grad_()
    Z = ed.deform_grid_inverse(Y, Dt, I, order=3, mode="mirror", **kw)
    assert Z.grad_fn is not None and tuple(Z.shape) == I
    dZ = torch.from_numpy(_cotangent(33, I)).cuda()
    Z.backward(dZ)
    want = ed.deform_grid_inverse_gradient(dZ, Dt, order=3, mode="mirror", **kw)
    assert Y.grad.shape == Y.shape and Y.grad.dtype == Y.dtype
    assert float((Y.grad - want).abs().max()) <= 1e-11 * float(want.abs().max())
    # the batch form
    Yb = torch.stack([Y.detach(), Y.detach().flip(0)]).requires_grad_()
    Db = torch.stack([Dt, -Dt])
    Zb = ed.deform_grid_inverse_batch(Yb, Db, I, order=3, mode="mirror", **kw)
    dZb = torch.stack([dZ, dZ.flip(1)])
    Zb.backward(dZb)
    wb = ed.deform_grid_inverse_gradient_batch(dZb, Db, order=3, mode="mirror", **kw)
    assert float((Yb.grad - wb).abs().max()) <= 1e-11 * float(wb.abs().max())


def test_valid_is_not_differentiable():
    I, Dt, kw, Y = _tensor_case(34)
    Y.requires_grad_()
    back, valid = ed.deform_grid_inverse(Y, Dt, I, order=1, mode="constant", return_valid=True, **kw)
    assert back.requires_grad and not valid.requires_grad and valid.dtype == torch.uint8
    (back * valid).sum().backward()
    want = ed.deform_grid_inverse_gradient(valid.to(torch.float64), Dt, order=1, mode="constant", **kw)
    assert 0 < int(valid.sum()) and float(want.abs().max()) > 0
    assert float((Y.grad - want).abs().max()) <= 1e-11 * float(want.abs().max())


def test_list_input_with_one_y_requiring_grad():
    I, Dt, kw, Ya = _tensor_case(35)
    Ya.requires_grad_()
    Yb = torch.from_numpy(np.random.default_rng(36).uniform(size=_out_shape("2d") + (2,))).cuda().float()
    Za, Zb = ed.deform_grid_inverse([Ya, Yb], Dt, [I, I + (2,)], order=[3, 1], mode=["mirror", "constant"],
                                    axis=[(0, 1), (0, 1)], **kw)
    assert Za.grad_fn is not None and not Zb.requires_grad and Zb.dtype == torch.float32
    with torch.no_grad():
        plain = ed.deform_grid_inverse([Ya, Yb], Dt, [I, I + (2,)], order=[3, 1], mode=["mirror", "constant"],
                                       axis=[(0, 1), (0, 1)], **kw)
    assert torch.equal(Za.detach(), plain[0]) and torch.equal(Zb, plain[1])
    dZ = torch.from_numpy(_cotangent(37, I)).cuda()
    Za.backward(dZ)
    want = ed.deform_grid_inverse_gradient(dZ, Dt, order=3, mode="mirror", **kw)
    assert Yb.grad is None and float((Ya.grad - want).abs().max()) <= 1e-11 * float(want.abs().max())


def test_calls_that_need_no_gradient_are_unchanged():
    I, Dt, kw, Y = _tensor_case(38)
    Z = ed.deform_grid_inverse(Y, Dt, I, **kw)
    assert Z.grad_fn is None and not Z.requires_grad
    with torch.no_grad():
        Zn = ed.deform_grid_inverse(Y.clone().requires_grad_(), Dt, I, **kw)
    assert Zn.grad_fn is None and torch.equal(Zn, Z)
    Zi = ed.deform_grid_inverse((Y * 100).to(torch.int16), Dt, I, order=1, **kw)
    assert Zi.dtype == torch.int16 and not Zi.requires_grad
    Znp = ed.deform_grid_inverse(Y.cpu().numpy(), Dt.cpu().numpy(), I, **kw)
    assert isinstance(Znp, np.ndarray) and (Znp == Z.cpu().numpy()).all()
