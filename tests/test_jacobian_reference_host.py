"""
CPU tests of tests/jacobian_reference.py, the NumPy reference the GPU tests of deform_grid_jacobian compare against:

* its J against central differences (h = 1e-4) of oracle.dgrad_reference.coordinate at the lattice positions, within
  1e-6 max(1, |J|max) -- the bound tests/test_points.py uses for the same differences;
* its dD and dK against central differences with step 1 of its own L = sum g det.  det is affine in every single
  D[h, j] and K[h, l] (each enters one row of J only), so the difference quotient is exact up to rounding: the bound
  is 1024 eps A, A the absolute-value sum of the entry's terms.  The quotient is summed voxel by voxel (math.fsum of
  g (det+ - det-) / 2), so that a voxel the entry does not reach contributes an exact zero;
* its rotate / zoom (and affine) gradients against central differences with step 1e-4 of L as a function of the
  parameter, within 1e-6 max(1, |value|).
"""
import math

import numpy as np
import pytest

from oracle import dgrad_reference as dref
from oracle import ed_oracle as orc

import jacobian_reference as jref

EPS = np.finfo(np.float64).eps
AFFINE2 = np.array([[1.1, 0.15, -1.5], [-0.1, 0.9, 2.0]])
AFFINE3 = np.array([[1.05, 0.1, 0.0, -1.0], [-0.08, 0.95, 0.05, 0.5], [0.02, -0.04, 1.1, 1.5]])

CASES = {
    "1d": dict(I=(40,), ncp=(5,), seed=1),
    "2d-crop": dict(I=(13, 17), ncp=(4, 5), seed=2, crop=(slice(2, 11), slice(3, 15))),
    "3d-affine": dict(I=(12, 14, 10), ncp=(4, 4, 5), seed=3, affine=AFFINE3),
    "3d-knots": dict(I=(9, 9, 9), ncp=(5, 3, 2), seed=4),
}


def _case(name, sigma=2.0):
    c = dict(CASES[name])
    I, ncp, seed = c.pop("I"), c.pop("ncp"), c.pop("seed")
    D = np.random.default_rng(seed).standard_normal((len(I),) + ncp) * sigma
    return I, D, c


def _cotangent(shape, seed=77):
    return np.random.default_rng(seed).standard_normal(shape)


@pytest.mark.parametrize("name", sorted(CASES))
def test_jacobian_equals_central_differences_of_the_coordinate_map(name):
    I, D, kw = _case(name)
    n = len(I)
    ref = jref.reference(D, I, **kw)
    _, O, off, K = jref.geometry(I, D, **kw)
    q = np.stack(np.indices(O), axis=-1).reshape(-1, n).astype(np.float64)
    h = 1e-4
    want = np.zeros((q.shape[0], n, n))
    for l in range(n):
        e = np.zeros(n)
        e[l] = h
        want[:, :, l] = (dref.coordinate(q + e, D, I, off, K) - dref.coordinate(q - e, D, I, off, K)) / (2 * h)
    err = np.abs(ref.J.reshape(-1, n, n) - want).max()
    print("%s: max |J err| %.3g, |J|max %.3g" % (name, err, np.abs(want).max()))
    assert err <= 1e-6 * max(1.0, np.abs(want).max())
    np.testing.assert_allclose(ref.det.reshape(-1), np.linalg.det(ref.J.reshape(-1, n, n)), rtol=0, atol=64 * EPS * ref.B)
    assert np.abs(ref.det).max() <= ref.B


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_equal_step_one_differences_of_the_loss(name):
    I, D, kw = _case(name)
    n = len(I)
    ref0 = jref.reference(D, I, **kw)
    g = _cotangent(ref0.det.shape)
    ref = jref.reference(D, I, g, **kw)
    assert ref.dK[:, n].tolist() == [0.0] * n
    worst = 0.0
    for idx in np.ndindex(*D.shape):
        Dp, Dm = D.copy(), D.copy()
        Dp[idx] += 1.0
        Dm[idx] -= 1.0
        diff = jref.reference(Dp, I, **kw).det - jref.reference(Dm, I, **kw).det
        quotient = math.fsum((g * diff).reshape(-1)) / 2.0
        err = abs(quotient - ref.dD[idx])
        worst = max(worst, err / (EPS * ref.A_D[idx]))
        assert err <= 1024 * EPS * ref.A_D[idx], (idx, quotient, ref.dD[idx], ref.A_D[idx])
    for h in range(n):
        for l in range(n):
            E = np.zeros_like(ref.K)
            E[h, l] = 1.0
            diff = jref.determinant(ref.S + (ref.K + E)[:, :n]) - jref.determinant(ref.S + (ref.K - E)[:, :n])
            quotient = math.fsum((g * diff).reshape(-1)) / 2.0
            err = abs(quotient - ref.dK[h, l])
            worst = max(worst, err / (EPS * ref.A_K[h, l]))
            assert err <= 1024 * EPS * ref.A_K[h, l], (h, l, quotient, ref.dK[h, l])
    print("%s: worst error %.1f eps A" % (name, worst))


PARAMS = {
    "rotate-zoom-crop": dict(I=(40, 52), ncp=(5, 5), crop=(slice(4, 36), slice(6, 50)), rotate=20.0, zoom=1.3),
    "rotate": dict(I=(13, 17), ncp=(4, 5), rotate=-35.0),
    "affine-rotate-zoom": dict(I=(13, 17), ncp=(4, 5), affine=AFFINE2, rotate=10.0, zoom=0.8),
    "affine3": dict(I=(12, 14, 10), ncp=(4, 4, 5), affine=AFFINE3),
}


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_parameter_gradients_equal_central_differences(name):
    c = dict(PARAMS[name])
    I, ncp = c.pop("I"), c.pop("ncp")
    n = len(I)
    D = np.random.default_rng(9).standard_normal((n,) + ncp) * 2.0
    ref0 = jref.reference(D, I, **c)
    g = _cotangent(ref0.det.shape)
    ref = jref.reference(D, I, g, **c)
    d_aff, d_rot, d_zoom = jref.parameter_gradients(ref.dK, ref.O, c.get("affine"), c.get("rotate"), c.get("zoom"))

    def L(**over):
        k = dict(c, **over)
        K = orc._inverse_affine(k.get("affine"), k.get("rotate"), k.get("zoom"), n, list(ref.O))
        return jref.loss(ref.S, K, g)

    h = 1e-4
    for key, got in (("rotate", d_rot), ("zoom", d_zoom)):
        if c.get(key) is None:
            assert got is None
            continue
        want = (L(**{key: c[key] + h}) - L(**{key: c[key] - h})) / (2 * h)
        print("%s: d %s %.9g, central difference %.9g" % (name, key, got, want))
        assert abs(got - want) <= 1e-6 * max(1.0, abs(want))
    if c.get("affine") is not None:
        A = np.asarray(c["affine"], dtype=np.float64)
        for idx in np.ndindex(*A.shape):
            Ap, Am = A.copy(), A.copy()
            Ap[idx] += h
            Am[idx] -= h
            want = (L(affine=Ap) - L(affine=Am)) / (2 * h)
            assert abs(d_aff[idx] - want) <= 1e-6 * max(1.0, abs(want)), (idx, d_aff[idx], want)


def test_the_folding_and_the_invertible_field():
    fold = jref.reference(np.random.default_rng(5).standard_normal((2, 5, 5)) * 6.0, (32, 32))
    mild = jref.reference(np.random.default_rng(12).standard_normal((2, 5, 5)) * 2.0, (40, 52))
    print("folding field: min det %.3f; invertible field: min det %.3f" % (fold.det.min(), mild.det.min()))
    assert fold.det.min() < 0
    assert mild.det.min() > 0.2
