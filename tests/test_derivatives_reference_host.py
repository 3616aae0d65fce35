"""
CPU tests of tests/derivatives_reference.py, the NumPy reference the GPU tests of deform_grid_derivatives compare
against:

* the three facts the adjoint's fixed-point quantum rests on: on [0, 1) sum_t |w_t| = 1, sum_t |w'_t| <= 1.5 and
  sum_t |w''_t| <= 4, the two maxima attained (x = 1/2 and x = 0);
* its r and J against oracle.dgrad_reference.coordinate and central differences of it;
* its H against central differences (h = 1e-4) of its own J, and its T against differences of its own H, at positions
  at least 2e-3 from a knot in control coordinates (the step stays inside the knot cell, where r is a polynomial).  The
  bound is the quotient's own error: truncation h^2 / 6 times the third derivative along the step -- of J[h, l] at most
  12 s^4 |P|max (sum |w'| sum |w'''| = 1.5 x 8), of H[h, l, m] at most 32 s^5 |P|max (sum |w''| sum |w'''| = 4 x 8), s the
  largest s_k -- plus rounding: each J (H) carries at most 72 eps A (64 taps, 8 operations a tap; A its absolute-value
  sum, at most |K|max + 1.5 s |P|max, resp. 4 s^2 |P|max) and moves by |H| (|T|) ulp(|q| + |off|) for the rounding of
  its position, both divided by h;
* the adjoint against d/d eps of L = sum u r + A J + G H for random u, A, G: L is linear in every D[h, j] and K[h, l],
  so a step-1 difference is exact up to rounding (1024 eps A_D and 1024 eps max(1, A_K), the bounds of the GPU tests;
  the points' terms that an entry does not reach cancel exactly, being the same numbers in both losses); the rows
  dq against central differences (h = 1e-5) in q, within 1e-6 max(1, A_q) (L is cubic in q inside a cell).
"""
import numpy as np
import pytest

from oracle import dgrad_reference as dref

import derivatives_reference as xref
import jacobian_reference as jref

EPS = np.finfo(np.float64).eps
AFFINE2 = np.array([[1.1, 0.15, -1.5], [-0.1, 0.9, 2.0], [0.0, 0.0, 1.0]])
AFFINE3 = np.array([[1.05, 0.1, 0.0, -1.0], [-0.08, 0.95, 0.05, 0.5], [0.02, -0.04, 1.1, 1.5]])

CASES = {
    "1d-two-points": dict(I=(9,), ncp=(2,), seed=1),
    "2d-crop-affine": dict(I=(13, 17), ncp=(4, 5), seed=2, crop=(slice(2, 11), slice(3, 15)), affine=AFFINE2),
    "2d-rotate-zoom": dict(I=(13, 17), ncp=(4, 5), seed=5, rotate=20.0, zoom=1.3),
    "3d-affine-crop": dict(I=(12, 14, 10), ncp=(4, 4, 5), seed=3, affine=AFFINE3,
                           crop=(slice(1, 11), slice(0, 12), slice(2, 9))),
}
NAMES = list(CASES)
N = 60


def _case(name):
    c = dict(CASES[name])
    I, ncp, seed = c.pop("I"), c.pop("ncp"), c.pop("seed")
    rng = np.random.default_rng(seed)
    n = len(I)
    D = rng.standard_normal((n,) + ncp) * 2.0
    _, _, off, _ = jref.geometry(I, D, **c)
    # positions inside and outside the image, each at least 1e-3 from a knot in control coordinates
    q = np.empty((N, n))
    for k in range(n):
        s = (ncp[k] - 1) / (I[k] - 1)
        cp = np.floor(rng.uniform(-3.0, ncp[k] + 2.0, N)) + rng.uniform(2e-3, 1.0 - 2e-3, N)
        q[:, k] = cp / s - off[k]
    u, A, G = rng.standard_normal((N, n)), rng.standard_normal((N, n, n)), rng.standard_normal((N, n, n, n))
    return I, D, c, q, u, A, G


def test_weight_sum_bounds():
    x = np.concatenate([np.linspace(0.0, 1.0, 100001)[:-1], [0.5, np.nextafter(1.0, 0.0)]])
    w = xref.weight_jet(x)
    s0, s1, s2 = (np.abs(w[a]).sum(-1) for a in range(3))
    assert np.all(w[0] >= 0) and np.abs(s0 - 1.0).max() <= 4 * EPS
    assert s1.max() <= 1.5 and s1.max() == 1.5
    assert s2.max() <= 4.0 and s2.max() == 4.0
    assert np.all(w[3] == np.array([-1.0, 3.0, -3.0, 1.0]))


@pytest.mark.parametrize("name", NAMES)
def test_coordinates_and_jacobian(name):
    I, D, kw, q, *_ = _case(name)
    ref = xref.reference(D, I, q, **kw)
    _, _, off, K = jref.geometry(I, D, **kw)
    r = dref.coordinate(q, D, I, off, K)
    assert np.abs(ref.r - r).max() <= 64 * EPS * max(1.0, np.abs(r).max())
    h = 1e-4
    for l in range(D.shape[0]):
        e = np.zeros(D.shape[0])
        e[l] = h
        d = (dref.coordinate(q + e, D, I, off, K) - dref.coordinate(q - e, D, I, off, K)) / (2 * h)
        assert np.abs(ref.J[:, :, l] - d).max() <= 1e-6 * max(1.0, np.abs(ref.J).max())


@pytest.mark.parametrize("name", NAMES)
def test_hessian_and_third_derivative_against_differences(name):
    I, D, kw, q, *_ = _case(name)
    n = D.shape[0]
    ref = xref.reference(D, I, q, **kw)
    assert ref.sane.all()
    assert np.array_equal(ref.H, np.swapaxes(ref.H, -1, -2))
    h = 1e-4
    _, _, off, K = jref.geometry(I, D, **kw)
    smax = max((D.shape[k + 1] - 1) / (I[k] - 1) for k in range(n))
    Pmax = np.abs(dref.prefiltered(D)).max()
    ulp = np.spacing((np.abs(q) + np.abs(off)).max())
    Hmax, Tmax = np.abs(ref.H).max(), np.abs(ref.T).max()
    tolH = h * h / 6 * 12 * smax ** 4 * Pmax + (72 * EPS * (np.abs(K).max() + 1.5 * smax * Pmax) + Hmax * ulp) / h
    tolT = h * h / 6 * 32 * smax ** 5 * Pmax + (72 * EPS * 4 * smax ** 2 * Pmax + Tmax * ulp) / h
    for p in range(n):
        e = np.zeros(n)
        e[p] = h
        plus, minus = xref.reference(D, I, q + e, **kw), xref.reference(D, I, q - e, **kw)
        dJ = (plus.J - minus.J) / (2 * h)
        dH = (plus.H - minus.H) / (2 * h)
        errH = np.abs(ref.H[..., p] - dJ).max()
        errT = np.abs(ref.T[..., p] - dH).max()
        print("%s axis %d: H err %.3g (bound %.3g, |H| %.3g), T err %.3g (bound %.3g, |T| %.3g)"
              % (name, p, errH, tolH, Hmax, errT, tolT, Tmax))
        assert errH <= tolH
        assert errT <= tolT


@pytest.mark.parametrize("which", ["u", "A", "G", "all"])
@pytest.mark.parametrize("name", NAMES)
def test_adjoint_against_differences_of_the_loss(name, which):
    I, D, kw, q, u, A, G = _case(name)
    n = D.shape[0]
    cot = dict(u=u if which in ("u", "all") else None, A=A if which in ("A", "all") else None,
               G=G if which in ("G", "all") else None)
    ref = xref.reference(D, I, q, **cot, **kw)
    L = lambda **over: xref.loss(xref.reference(over.pop("D", D), I, over.pop("q", q), **over, **kw), **cot)  # noqa: E731
    rng = np.random.default_rng(11)
    # D: a step of 1 on single entries (L is linear in each)
    for _ in range(8):
        j = tuple(rng.integers(0, s) for s in D.shape)
        E = np.zeros_like(D)
        E[j] = 1.0
        d = (L(D=D + E) - L(D=D - E)) / 2
        assert abs(d - ref.dD[j]) <= 1024 * EPS * ref.A_D[j], (j, d, ref.dD[j])
    # K likewise
    for h in range(n):
        for l in range(n + 1):
            E = np.zeros_like(ref.K)
            E[h, l] = 1.0
            d = (L(inverse_map=ref.K + E) - L(inverse_map=ref.K - E)) / 2
            assert abs(d - ref.dK[h, l]) <= 1024 * EPS * max(ref.A_K[h, l], 1.0), (h, l, d, ref.dK[h, l])
    # q: central differences, all points at once (a point's terms depend on that point alone)
    h = 1e-5
    for p in range(n):
        e = np.zeros(n)
        e[p] = h
        plus, minus = xref.reference(D, I, q + e, **kw), xref.reference(D, I, q - e, **kw)
        d = np.zeros(q.shape[0])
        for c, name_ in ((cot["u"], "r"), (cot["A"], "J"), (cot["G"], "H")):
            if c is not None:
                diff = (getattr(plus, name_) - getattr(minus, name_)) / (2 * h)
                d += (c * diff).reshape(q.shape[0], -1).sum(1)
        assert np.abs(d - ref.dq[:, p]).max() <= 1e-6 * max(1.0, ref.A_q.max())


def test_positions_that_are_not_sane():
    I, D, kw, q, u, A, G = _case("2d-crop-affine")
    q = q.copy()
    q[3, 0], q[5, 1], q[7, 0] = np.nan, np.inf, 1e17
    u = u.copy()
    u[3, 0] = np.nan
    ref = xref.reference(D, I, q, u=u, A=A, G=G, **kw)
    bad = np.array([3, 5, 7])
    assert not ref.sane[bad].any() and ref.sane.sum() == N - 3
    assert np.isnan(ref.r[bad]).all() and np.isnan(ref.H[bad]).all()
    assert np.all(ref.dq[bad] == 0) and np.isfinite(ref.dD).all() and np.isfinite(ref.dK).all()
    keep = np.delete(np.arange(N), bad)
    sub = xref.reference(D, I, q[keep], u=u[keep], A=A[keep], G=G[keep], **kw)
    assert np.allclose(sub.dD, ref.dD, rtol=0, atol=64 * EPS * ref.A_D.max())
