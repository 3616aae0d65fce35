"""
GPU tests of the 1-, 2- and 4-axis kernels (elasticdeform_amd/csrc/deform_fast.hip) at every launch shape, against the
CPU oracle (oracle/ed_oracle.py, the fp64 C restatement) on the same inputs.

One table (tests/fast_cases.py), proven to reach its classes by tests/test_fast_cases_host.py from a NumPy restatement
of the launch arithmetic: the row kernel at 4, 8, 16 and 32 rows per block with partial last blocks, one to twelve
lane passes over E, both sides of kMaxE and kMaxE4, the butterfly and the rolled four-axis contraction, the 3-D calls
the tile path leaves to it; the 2-D LDS gradient with fitting, non-fitting, empty and partly dead blocks, non-finite
gradients, blocks with nothing to add, several steps, channels last below the Python layer's re-layout threshold
(in_stride[1] = 3 in the kernel), crops and an affine map; the 4-D LDS gradient with non-finite
gradients and with boxes that fit in float32 and not in float64.  The routes cannot be observed from outside, so the
host file proves the class and the mutation record below shows that the class bites.

Tolerances are those of tests/test_gpu_parity.py.  Forward: |got - want| <= eps (1 + |want|) on data in [0, 1),
eps = 1e-11 (float64) / 1e-5 (float32).  Gradient without the transposed prefilter and every float64 gradient:
eps (max(1, max |want|) + |want|).  float32 gradient with the prefilter: _f32_grad_check(flat=False) against the fp64
oracle on the upcast dY.  Non-finite dY: the finite mask equals the oracle's and the finite entries are within the
tolerance (prefilter=False: the transposed prefilter would spread the inf over whole lines).  Every test prints its
largest err / allowed.

test_fixed_point_resolution (G9): the float32 LDS gradient accumulates a block in int32 units of
unit = kW1^2 * 1.001 * sum |dY|_block / (2^31 - 2^10), every contribution rounded to the nearest unit.  Cells no tap of
the spike's block lands on keep the reference's local relative precision, max(2e-5, 4 x the oracle's own float32
figure).  Cells of that block beside the spike are within sum_b N_b 0.5 unit_b, the bound the issue states (N_b taps
of block b land on the cell, counted by the restatement; about 1e-3).  The (order + 1)^2 cells the spike itself lands
on cannot hold 1e6 to that in float32 and have a bound of their own: the same plus 12 * 2^-24 * sum |dY| over the taps
that land there -- the two weights within 2 * 2^-24 each (4), the three products of the contribution (3), the rounded
scale and its inverse (2), the conversion, the product with the inverse and one float atomic (3).

test_adjoint_identity: float64, prefilter=False, cval 0: |<dY, F(X)> - <G(dY), X>| <= 1e-11 sum |dY| max |X| ties
every gradient kernel to the forward row kernel without the oracle.

Found by this file: with the closed-form weights of the two LDS gradient kernels evaluated in float32 the order-5
gradient of an isolated pixel missed the float32 rule after the transposed prefilter (G5: 7.2e-7 against 6.2e-7
allowed, G9: 1.46 against 0.94 at scale 8.7e5; every other case passed).  A CPU restatement of the kernel's weights
gave the same figure (2.0e-7 on a largest cell of 0.2 before the prefilter, 9.1e-7 behind the fp64 prefilter) and
1.3e-8 / 8.2e-8 with the closed forms in double on the same float32 fraction, and 1.4e-7 with only the
two outer Horner forms w[1], w[4] (8e-7 off in float32, the others 6e-8 at most) and the last weight in double, which is
what the kernels now do at order 5 in float32 (weights_of_frac; orders 1 to 4 passed as they were and are unchanged);
G5 and G9 at order 5 are the regression cases (0.24 and 0.27 of the allowed error now).

Measured on the MI355X (largest err / allowed per class; 358 tests in 38 s, the slowest single test 0.87 s, R11 at
order 5):

    row kernel, forward     float64 0.13 (R4; R5a 0.11; the 3-D and 4-D cases 2e-4 to 1e-3), float32 0.016 (R14)
    row kernel, gradient    float64 0.17 (R5a, 1-D at nE = kMaxE; every other case at most 5e-3), float32 0.067 (R10b)
    across the boundaries   R5b and R6b (exact kernel) return the oracle's bits forward; gradient 5e-5 / 0.027
    2-D LDS, no prefilter   float64 3.1e-3 (G7), float32 0.070 (G2p); non-finite G4 / G6a / G6b: 1.5e-3 / 0.042
    2-D LDS, prefilter      float64 4.3e-3 (G7), float32 rule 0.46 (G5; G7 0.45, G3 0.40, G8 0.39; G6c 0.13)
    G9, float32             cells beside the spike 0.96 / 0.82 / 0.53 / 0.27 / 0.28 of the bound at orders 1 to 5 (order 1:
                            four taps per cell, each off by almost half a unit); the spike's own cells 0.78 * 2^-24 of
                            their sum |dY| at most, against the 12 allowed; far cells 3.2e-6 to 4.3e-6 locally
                            against the 2e-5 allowed (the oracle's own float32 figure: 2e-7 to 7e-7)
    4-D LDS                 float64 4.1e-4 (H2), float32 0.068 (H2); non-finite H1: 1.3e-4 / 0.059
    adjoint identity        1.3e-5 of the allowed 1e-11 sum |dY| max |X| at most (R11)

Mutation record.  One value-only change per branch of deform_fast.hip in a scratch copy of the library (no index,
extent or bound touched), this file run once per change; cases that fail, of 340:

    a wave's second row reuses the first row's E         75: every row case with more than 4 rows per block (R1, R2,
                                                          R3, R4, R6a, R8, R11), none with 4; the adjoint of R6a
    the row kernel's lane loop over E cut to one pass     63: R5a, R6a, R7, R9, R11, R12 (nE > 64) and no other
      (the later passes store zeros)
    the same in the 2-D LDS gradient                      11: R6a's gradients at orders 1 to 5 and its adjoint
    the rolled 4-D contraction drops a tap                 8: R9 and no other
    the 2-D no-fit path drops a tap's weight              62: G2, G2p, G3, G6a, G6b, R6a's gradient, five adjoints
    the 4-D no-fit path drops a tap's weight              16: H1, H2, R8, R10a, three adjoints
    the 2-D box not re-zeroed between steps               22: G6a, G6b and their adjoints, no other
    the 2-D `gtot == 0` skip inverted                    183: every 2-D LDS case
"""
import numpy as np
import pytest

import fast_cases as fc
from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
from test_gpu_parity import _f32_grad_check  # noqa: E402

EPS = {"float64": 1e-11, "float32": 1e-5}
EPS32 = float(np.finfo(np.float32).eps)
DTYPES = ("float64", "float32")


@pytest.fixture(autouse=True)
def _auto_arithmetic():
    prev = ed.set_arithmetic("auto")
    yield
    ed.set_arithmetic(prev)


def _ratio(got, want, eps, scale):
    """largest |got - want| / (eps (scale + |want|)) -- assert_allclose(rtol=eps, atol=eps * scale) as a figure"""
    assert got.shape == want.shape and got.dtype == want.dtype
    g, w = got.astype(np.float64), want.astype(np.float64)
    if g.size == 0:
        return 0.0
    return float((np.abs(g - w) / (eps * (scale + np.abs(w)))).max())


def _grad_scale(want):
    fin = np.isfinite(want)
    return max(1.0, float(np.abs(want[fin]).max())) if fin.any() else 1.0


def _nonfinite_ratio(got, want, eps):
    """non-finite dY: the same entries are finite, and those are within the tolerance"""
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    assert 0 < fin.sum() < fin.size
    return _ratio(got[fin], want[fin], eps, _grad_scale(want))


# ---- the row kernel ----------------------------------------------------------------------------------------------------

def _row_gradient_runs(case, order, dtype):
    """the gradient of a row case runs where the row kernel (or, across a boundary, its neighbour) serves it; R6 also
    through the 2-D LDS kernel, whose s_E is full there"""
    r = fc.route(case["deformed"], case["points"], order, True, dtype=dtype, batch=case["batch"] or 1)
    return r != "lds2" or case["id"] in ("R6a", "R6b")


@pytest.mark.parametrize("id,dtype,order", [(c["id"], dt, o) for c in fc.ROW_CASES if not c["batch"]
                                            for dt in c["dtypes"] for o in c["orders"]])
def test_row_kernel(id, dtype, order):
    case = fc.by_id(id)
    X, D, dY, kw = fc.make_row(case, dtype, order)
    eps = EPS[dtype]
    r_fwd = _ratio(ed.deform_grid(X, D, **kw), orc.deform_grid(X, D, **kw), eps, 1.0)
    r_grad = 0.0
    if _row_gradient_runs(case, order, dtype):
        want = orc.deform_grid_gradient(dY, D, X_shape=X.shape, **kw)
        got = ed.deform_grid_gradient(dY, D, X_shape=X.shape, **kw)
        r_grad = _ratio(got, want, eps, _grad_scale(want))
    print("FAST row %s %s o%d %s err/allowed fwd %.3g grad %.3g" % (id, dtype, order, kw["mode"], r_fwd, r_grad))
    assert r_fwd <= 1.0 and r_grad <= 1.0, (r_fwd, r_grad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_kernel_batch_behind_the_tile_launcher(dtype):
    """R14: tensors on the device, so that the library's own grid filter and clear run in front of the row kernel"""
    case = fc.by_id("R14")
    X, D, dY, kw = fc.make_row(case, dtype, 3)
    eps = EPS[dtype]
    with torch.cuda.device(0):
        Dd = torch.from_numpy(D).cuda()
        got = ed.deform_grid_batch(torch.from_numpy(X).cuda(), Dd, **kw).cpu().numpy()
        grad = ed.deform_grid_gradient_batch(torch.from_numpy(dY).cuda(), Dd, **kw).cpu().numpy()
    r_fwd = r_grad = 0.0
    for b in range(case["batch"]):
        r_fwd = max(r_fwd, _ratio(got[b], orc.deform_grid(X[b], D[b], **kw), eps, 1.0))
        want = orc.deform_grid_gradient(dY[b], D[b], **kw)
        r_grad = max(r_grad, _ratio(grad[b], want, eps, _grad_scale(want)))
    print("FAST row R14 %s o3 err/allowed fwd %.3g grad %.3g" % (dtype, r_fwd, r_grad))
    assert r_fwd <= 1.0 and r_grad <= 1.0, (r_fwd, r_grad)


# ---- the LDS gradients -------------------------------------------------------------------------------------------------

def _gradient_check(dY, D, kw, dtype, tag):
    """one product call and one oracle call (two for float32 with the prefilter); prints err / allowed, then asserts"""
    want = orc.deform_grid_gradient(dY, D, **kw)
    got = ed.deform_grid_gradient(dY, D, **kw)
    assert got.shape == want.shape and got.dtype == want.dtype
    if not np.isfinite(dY).all():
        r = _nonfinite_ratio(got, want, EPS[dtype])
    elif dtype == "float32" and kw["prefilter"] and kw["order"] > 1:
        truth = orc.deform_grid_gradient(dY.astype(np.float64), D, **kw)
        scale = max(1.0, float(np.abs(truth).max()))
        err_gpu, err_ref = float(np.abs(got - truth).max()), float(np.abs(want - truth).max())
        r = err_gpu / (4.0 * err_ref + 4.0 * EPS32 * scale)
        print("FAST %s err/allowed %.3g (float32 rule: err %.3g, oracle float32 %.3g, scale %.3g)"
              % (tag, r, err_gpu, err_ref, scale))
        _f32_grad_check(got, want, truth, flat=False)
        return r
    else:
        r = _ratio(got, want, EPS[dtype], _grad_scale(want))
    print("FAST %s err/allowed %.3g" % (tag, r))
    assert r <= 1.0, r
    return r


def _g_params():
    """(case, dtype, order, prefilter): the transposed prefilter where there is one (orders 2-5) and dY is finite (an
    inf would spread over whole lines)"""
    out = []
    for c in fc.G_CASES:
        finite = c.get("finite") or not (c.get("nonfinite") or c.get("layout"))
        for dt in DTYPES:
            for o in c["orders"]:
                out.append((c["id"], dt, o, False))
                if finite and o > 1:
                    out.append((c["id"], dt, o, True))
    return out


@pytest.mark.parametrize("id,dtype,order,prefilter", _g_params())
def test_lds2_gradient(id, dtype, order, prefilter):
    dY, D, kw, x_shape = fc.make_g(fc.by_id(id), dtype, order)
    assert bool(np.isfinite(dY).all()) or not prefilter
    _gradient_check(dY, D, dict(kw, prefilter=prefilter, X_shape=x_shape), dtype,
                    "lds2 %s %s o%d prefilter=%s" % (id, dtype, order, prefilter))


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_fixed_point_resolution(order):
    case = fc.by_id("G9")
    dY, D, kw, x_shape = fc.make_g(case, "float32", order)
    kw = dict(kw, prefilter=False)
    res = fc.g_geometry("G9", order)[5]
    bound, cover, mass = fc.fixed_point_bound(res, dY, order, x_shape)
    y, x = fc.g_spike(order)
    spike = next(i for i, b in enumerate(res["blocks"]) if b["index"] == (y // fc.kRows2, x // 64))
    near = cover[spike] > 0
    far = ~near
    assert 0.005 < near.mean() < 0.5 and far.sum() > near.sum()
    truth = orc.deform_grid_gradient(dY.astype(np.float64), D, **kw)
    want = orc.deform_grid_gradient(dY, D, **kw)
    got = ed.deform_grid_gradient(dY, D, **kw)
    assert got.dtype == np.float32
    local = float((np.abs(got[far] - truth[far]) / np.maximum(np.abs(truth[far]), 1e-4)).max())
    ref_local = float((np.abs(want[far] - truth[far]) / np.maximum(np.abs(truth[far]), 1e-4)).max())
    err = np.abs(got - truth)
    beside = near & (mass < 1.0)                     # the block's cells that the spike itself does not land on
    on = near & ~beside                              # the (order + 1)^2 cells it lands on
    assert on.sum() == (order + 1) ** 2 and beside.sum() > 20 * on.sum()
    r_beside = float((err[beside] / bound[beside]).max())
    r_on = float((err[on] / (bound[on] + 12.0 * 2.0 ** -24 * mass[on])).max())
    print("FAST lds2 G9 o%d far local %.3g (oracle float32 %.3g) beside the spike err/bound %.3g on its cells "
          "err/allowed %.3g (%.3g of 2^-24 mass)" % (order, local, ref_local, r_beside, r_on,
                                                     float((err[on] / (2.0 ** -24 * mass[on])).max())))
    assert local <= max(2e-5, 4.0 * ref_local), (local, ref_local)
    assert r_beside <= 1.0, r_beside
    assert r_on <= 1.0, r_on


@pytest.mark.parametrize("id,dtype,order", [(c["id"], dt, o) for c in fc.H_CASES for dt in DTYPES
                                            for o in c["orders"]])
def test_lds4_gradient(id, dtype, order):
    dY, D, kw = fc.make_h(fc.by_id(id), dtype, order)
    _gradient_check(dY, D, kw, dtype, "lds4 %s %s o%d" % (id, dtype, order))


# ---- the adjoint identity ------------------------------------------------------------------------------------------------

ADJOINT = [("R1", 0, "row, 2-D, rows 8"), ("R4", 0, "row, 2-D, rows 32"), ("R5a", 3, "row, 1-D, nE = kMaxE"),
           ("R8", 1, "row, 4-D, butterfly"), ("R9", 2, "row, 4-D, rolled"), ("R10b", 2, "row, 4-D beyond kMaxE4"),
           ("R11", 3, "row, 3-D direct"), ("R12", 2, "row, 3-D wide window"), ("R6a", 3, "lds2, s_E full"),
           ("G1", 3, "lds2, every block fits"), ("G2", 3, "lds2, dead and non-fitting blocks"),
           ("G2p", 5, "lds2, order 5, non-fitting"), ("G3", 2, "lds2, wrap seams"), ("G6a", 4, "lds2, two step axes"),
           ("G6b", 3, "lds2, channels last, in_stride[1] = 3"), ("G7", 3, "lds2, crop, rotate, zoom"), ("R10a", 3, "lds4, fits"),
           ("H2", 2, "lds4, float64 boxes that do not fit"), ("H2", 3, "lds4, float64 boxes that do not fit")]


@pytest.mark.parametrize("id,order,why", ADJOINT)
def test_adjoint_identity(id, order, why):
    case = fc.by_id(id)
    rng = np.random.default_rng(7000 + order)
    if id.startswith("R"):
        X, D, dY, kw = fc.make_row(case, "float64", order)
        x_shape = X.shape
    elif id.startswith("G"):
        dY, D, kw, x_shape = fc.make_g(case, "float64", order)
        dY = rng.random(dY.shape)                    # (finite, and no channel of zeros)
    else:
        dY, D, kw = fc.make_h(case, "float64", order)
        x_shape = dY.shape
    kw = dict(kw, prefilter=False, cval=0.0)
    X = rng.random(x_shape) - 0.25
    Y = ed.deform_grid(X, D, **kw)
    assert Y.shape == dY.shape
    G = ed.deform_grid_gradient(dY, D, X_shape=x_shape, **kw)
    lhs, rhs = float(np.sum(dY * Y)), float(np.sum(G * X))
    allowed = 1e-11 * float(np.abs(dY).sum()) * float(np.abs(X).max())
    print("FAST adjoint %s o%d (%s) err/allowed %.3g" % (id, order, why, abs(lhs - rhs) / allowed))
    assert abs(lhs - rhs) <= allowed, (lhs, rhs, allowed)
