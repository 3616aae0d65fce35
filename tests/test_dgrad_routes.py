"""
GPU tests of the displacement and affine gradient kernels (deform_dgrad.hip) at every launch shape, against the
analytic float64 reference oracle/dgrad_reference.py (anchored on the host by tests/test_dgrad_reference_host.py).

One table (tests/dgrad_cases.py); every case compares deform_grid_displacement_gradient with the reference's dD and
AffineGradient.inverse_map with its dK.  The batch cases go through the combined call (both results from one set of
launches), every sample against its own reference.

float64 tolerance:  |got - want| <= c 2^-53 S, S the reference's own sum with every term replaced by its absolute
value at tap level (S_D after the entrywise absolute value of the transposed grid filter, S_K for dK).  c counts, to
first order, the roundings on the longest path of one result (dgrad_cases.rounding_counts has every line):

    weights 12 n + products n + the tap sum (n (p + 2) in the separable 2- and 3-axis kernels, (p + 1)^n in the
    generic one) + steps and inputs
    + the band product and the running sum over the group's 64 / G voxels + the chunks + (block / 64) G partials
    + per contracted axis 22 + ceil(L_d / 64) + per grid axis of the transposed filter 9 + ncp_d
      (dK instead: two butterflies, the chunks, the waves, the lane loop of the store: about 30)
    + the reference's own weights, tap sum and matrix products, 4 p n + (p + 1)^n + 32 n
    + the conditioning of the coordinate: the kernel rounds c_h once at its magnitude (2 n + 2 times with an affine),
      once in the boundary fold, and sums the displacement along 4^(n-1) + 8 n + 4 roundings of size u dmax; that
      shift of m moves the weights by at most (4 + 2 (n - 1)) dm relative to the tap-level scale.  (The reference
      forms its coordinates with a 64-bit significand.)

For the table c is between 8.1e2 (dK, 7 axes) and 1.1e4 (the crop with an affine); the coordinate term is most of it
(a row of 300 voxels rounds c at 2^-44, 512 u).  The host file proves c 2^-53 max S <= 1e-9 max |want| for every case from the reference alone.
The float32 grid case returns dD in float32: one more rounding, 2^-24 |want|, on that result.

float32 volumes: the project's rule (tests/test_gpu_parity.py:_f32_grad_check) -- the kernel is no further from the
float64 reference than 4 times the float32 restatement of the same sum (tap sums in float32, fp64 after them) is,
plus 4 eps32 max |want|.

Measured on the MI355X (every test prints its figures): the largest float64 err / bound over the table is 0.032
(dD of 1d_K200_o4; most cases are between 1e-5 and 1e-3 -- the bound is a worst case, the roundings average out), and
0.78 for the float32 grid, all of it the float32 store.  The largest float32 err / allowed is 0.41 (dK of
float32_1d_o4), most are between 0.05 and 0.2.  With the row kernel's final sum short of its last wave 76 of the 95
cases fail, with the contraction's lane loop cut to one iteration the 5 cases whose contracted axis is longer than 64;
the finite-difference files pass under both.
"""
import functools
import importlib

import numpy as np
import pytest

import dgrad_cases as dc
from oracle import dgrad_reference as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402

_dg = importlib.import_module("elasticdeform_amd.deform_grid")      # (the module; the package exports the function)

EPS32 = float(np.finfo(np.float32).eps)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _up(a):
    return [v.astype(np.float64) for v in a] if isinstance(a, list) else a.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(case, inputs, references): one Result per sample; float32 cases: (float64 reference, float32 restatement)"""
    case = next(c for c in dc.CASES if c["name"] == name)
    X, dY, D, kw = dc.make(case)
    if case.get("batch"):
        refs = [ref.reference(X[b], dY[b], D[b], **kw) for b in range(case["batch"])]
    elif case.get("f32"):
        refs = [ref.reference(_up(X), _up(dY), D, **kw), ref.reference(X, dY, D, f32=True, **kw)]
    else:
        refs = [ref.reference(X, dY, D, **kw)]
    return case, (X, dY, D, kw), refs


def _ratio(err, bound):
    """largest err / bound; where the bound is zero (nothing contributes to that entry) the result must be exact"""
    live = bound > 0
    assert np.all(err[~live] == 0)
    return float((err[live] / bound[live]).max())


def _gpu(case, X, dY, D, kw):
    """[(dD, dK)] per sample from the product API, as float64 NumPy arrays (dD in the dtype the call returned)"""
    if case.get("batch"):
        with torch.cuda.device(0):
            _, dd, dk = _dg._transform_gradient_batch(_dev(X), _dev(dY), _dev(D), want_disp=True, want_map=True, **kw)
            dd, dk = dd.cpu().numpy(), dk.cpu().numpy()
        return [(dd[b], dk[b]) for b in range(case["batch"])]
    dd = ed.deform_grid_displacement_gradient(X, dY, D, **kw)
    g = ed.deform_grid_affine_gradient(X, dY, D, **kw)
    n = D.shape[0]
    assert isinstance(dd, np.ndarray) and dd.shape == D.shape and dd.dtype == D.dtype
    assert g.inverse_map.shape == (n, n + 1) and g.inverse_map.dtype == np.float64
    return [(dd, g.inverse_map)]


@pytest.mark.parametrize("name", [c["name"] for c in dc.F64_CASES])
def test_float64_against_the_analytic_reference(name):
    case, (X, dY, D, kw), refs = _reference(name)
    got = _gpu(case, X, dY, D, kw)
    assert len(got) == len(refs)
    worst = []
    for (dd, dk), r in zip(got, refs):
        c_d, c_k = dc.rounding_counts(case, r.cmax, r.dmax)
        bound_d = c_d * dc.U * r.S_D
        if case.get("grid32"):
            bound_d = bound_d + 2.0 ** -24 * np.abs(r.dD)           # the result is stored in the grid's float32
        bound_k = c_k * dc.U * r.S_K
        worst.append((_ratio(np.abs(dd.astype(np.float64) - r.dD), bound_d), _ratio(np.abs(dk - r.dK), bound_k)))
    print("DGRAD64 %s c %.0f %.0f err/bound dD %.3g dK %.3g" % (name, c_d, c_k, max(w[0] for w in worst),
                                                               max(w[1] for w in worst)))
    assert max(w[0] for w in worst) <= 1.0 and max(w[1] for w in worst) <= 1.0, worst


@pytest.mark.parametrize("name", [c["name"] for c in dc.F32_CASES])
def test_float32_volumes_against_the_analytic_reference(name):
    case, (X, dY, D, kw), (exact, single) = _reference(name)
    assert X.dtype == np.float32 and dY.dtype == np.float32
    (dd, dk), = _gpu(case, X, dY, D, kw)
    ratios = []
    for got, want, rest in ((dd, exact.dD, single.dD), (dk, exact.dK, single.dK)):
        err_gpu = float(np.abs(got - want).max())
        err_rest = float(np.abs(rest - want).max())
        allowed = 4.0 * err_rest + 4.0 * EPS32 * float(np.abs(want).max())
        ratios.append((err_gpu / allowed, err_gpu, err_rest))
    print("DGRAD32 %s err/allowed dD %.3g dK %.3g" % (name, ratios[0][0], ratios[1][0]))
    assert ratios[0][0] <= 1.0 and ratios[1][0] <= 1.0, ratios
