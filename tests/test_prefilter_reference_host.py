"""
CPU tests of tests/prefilter_reference.py, the NumPy reference the GPU tests of the prefilter passes compare against:

* forward() against scipy.ndimage.spline_filter1d(mode='mirror') and transpose() against the oracle's restatement of
  the reference's transposed filter (oracle.ed_oracle.spline_filter1d_grad), orders 2-5, within 1e-13 of the result's
  scale -- both recursions truncate their boundary sums at 1e-15, the dense inverse does not;
* adjointness <F x, y> = <x, F^T y>;
* windowed(): the window holds the filter of the window's own lines, the rest is untouched;
* tap_range() against the taps SciPy's map_coordinates actually uses (an impulse response), orders 0-5;
* the constant line and the alternating line, the two closed-form eigenvectors.
"""
import numpy as np
import pytest
import scipy.ndimage

from oracle import ed_oracle as orc

import prefilter_reference as pref

LENGTHS = (2, 3, 7, 64, 65, 97, 200, 576)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_forward_and_transpose_against_scipy_and_the_oracle(order):
    rng = np.random.default_rng(order)
    for n in LENGTHS:
        for shape, axis in (((n, 5), 0), ((3, n), 1), ((2, n, 3), 1)):
            x = rng.standard_normal(shape)
            want = scipy.ndimage.spline_filter1d(x, order=order, axis=axis, mode="mirror")
            got = pref.forward(x, order, axis)
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (n, shape)
            wt = np.zeros(shape)
            orc.spline_filter1d_grad(x, wt, axis, order)
            got = pref.transpose(x, order, axis)
            assert np.abs(got - wt).max() <= 1e-13 * np.abs(wt).max(), (n, shape)


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_adjointness(order):
    rng = np.random.default_rng(10 + order)
    for n in (64, 65, 97, 576, 2, 31):
        x, y = rng.standard_normal((n, 4)), rng.standard_normal((n, 4))
        a = np.sum(pref.forward(x, order, 0) * y)
        b = np.sum(x * pref.transpose(y, order, 0))
        scale = np.sum(np.abs(pref.forward(x, order, 0) * y))
        assert abs(a - b) <= 1e-13 * scale, (n, a, b)


def test_orders_below_two_are_the_identity():
    x = np.random.default_rng(0).standard_normal((5, 9))
    for order in (0, 1):
        np.testing.assert_array_equal(pref.forward(x, order, 1), x)
        np.testing.assert_array_equal(pref.transpose(x, order, 0), x)


@pytest.mark.parametrize("tr", [False, True])
def test_windowed_filters_the_window_as_its_own_array(tr):
    rng = np.random.default_rng(4)
    x = rng.standard_normal((9, 80, 70))
    window = ((2, 7), (5, 71), (0, 66))
    got = pref.windowed(x, window, (1, 2), 3, tr)
    sub = x[2:7, 5:71, 0:66].copy()
    for a in (1, 2):
        w = np.zeros_like(sub)
        if tr:
            orc.spline_filter1d_grad(sub, w, a, 3)
        else:
            w = scipy.ndimage.spline_filter1d(sub, order=3, axis=a, mode="mirror")
        sub = w
    assert np.abs(got[2:7, 5:71, 0:66] - sub).max() <= 1e-13 * np.abs(sub).max()
    mask = np.ones(x.shape, dtype=bool)
    mask[2:7, 5:71, 0:66] = False
    np.testing.assert_array_equal(got[mask], x[mask])
    # NaN outside the window stays outside
    y = np.full(x.shape, np.nan)
    y[2:7, 5:71, 0:66] = x[2:7, 5:71, 0:66]
    np.testing.assert_array_equal(pref.windowed(y, window, (1, 2), 3, tr)[2:7, 5:71, 0:66], got[2:7, 5:71, 0:66])


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4, 5])
def test_tap_range_against_the_taps_scipy_reads(order):
    """map_coordinates(prefilter=False) of unit impulses: the samples with a non-zero weight at coordinate c are inside
    tap_range(c) .. + order, and the outermost taps carry weight unless c sits where their weight vanishes"""
    n = 40
    eye = np.eye(n)
    rng = np.random.default_rng(order)
    cs = np.concatenate([rng.uniform(8.0, 30.0, 50), [12.0, 12.5, 13.0, 20.25, 20.75]])
    for c in cs:
        w = np.array([scipy.ndimage.map_coordinates(eye[j], [[c]], order=order, mode="mirror", prefilter=False)[0]
                      for j in range(n)])
        used = np.nonzero(np.abs(w) > 1e-14)[0]
        first = int(pref.tap_range(c, order))
        assert used.min() >= first and used.max() <= first + order, (c, used, first)
        frac = c - np.floor(c)
        if order > 0 and min(abs(frac), abs(frac - 0.5), abs(frac - 1.0)) > 0.05:      # 0.05^5 / 120 = 3e-9
            assert used.min() == first and used.max() == first + order, (c, used, first)
        assert abs(w.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_constant_and_alternating_lines(order):
    lam = pref.alternating_eigenvalue(order)
    assert abs(lam - 1.0 / sum(b * (-1) ** abs(k) for k, b in
                               [(k, pref.SAMPLES[order][abs(k)]) for k in range(-(len(pref.SAMPLES[order]) - 1),
                                                                                len(pref.SAMPLES[order]))])) < 1e-12 * lam
    for n in (64, 65, 97):
        one = np.ones((n, 2))
        alt = ((-1.0) ** np.arange(n))[:, None] * np.array([[1.0, -2.0]])
        assert np.abs(pref.forward(one, order, 0) - one).max() < 1e-13
        assert np.abs(pref.forward(alt, order, 0) - lam * alt).max() < 1e-12 * lam
        want = scipy.ndimage.spline_filter1d(alt, order=order, axis=0, mode="mirror")
        assert np.abs(want - lam * alt).max() < 1e-12 * lam
