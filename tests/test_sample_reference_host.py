"""
CPU tests that anchor tests/sample_reference.py, the NumPy reference of deform_grid_sample, on sources it shares no
code with: the CPU oracle's deform_grid on the integer lattice (orders 0 to 5, the five modes), scipy's map_coordinates
for mode='mirror', and central differences of the reference's own values for g.  No GPU is needed.
"""
import numpy as np
import pytest
import scipy.ndimage

import sample_reference as sref
from oracle import ed_oracle as orc
from oracle.dgrad_reference import MODES

GEOMETRIES = {
    "1d": dict(I=(40,), ncp=(5,), sigma=2.0, crop=None),
    "2d-crop": dict(I=(13, 17), ncp=(4, 5), sigma=3.0, crop=(slice(2, 11), slice(3, 15))),
    "3d": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5, crop=None),
}
EDGE = 1e-6


def _case(name):
    c = GEOMETRIES[name]
    n = len(c["I"])
    rng = np.random.default_rng(100 + n)
    D = rng.standard_normal((n,) + c["ncp"]) * c["sigma"]
    X = rng.uniform(0.0, 1.0, size=c["I"])
    crop = c["crop"]
    O = c["I"] if crop is None else tuple(s.stop - s.start for s in crop)
    off = np.zeros(n) if crop is None else np.array([float(s.start) for s in crop])
    return X, D, crop, O, off


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", range(6))
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_the_integer_lattice_equals_the_oracle(name, order, mode):
    X, D, crop, O, off = _case(name)
    n = X.ndim
    lattice = np.stack(np.indices(O), axis=-1).reshape(-1, n).astype(np.float64)
    r = sref.coordinate(lattice, D, X.shape, off)
    got = sref.reference(X, r, range(n), order, mode, cval=0.25).V[:, 0]
    want = orc.deform_grid(X, D, order=order, mode=mode, cval=0.25, crop=crop).reshape(-1)
    keep = sref.boundary_distance(r, X.shape, order, mode) > EDGE
    err = np.abs(got - want)[keep].max()
    print("%s order %d %s: max |err| %.3g, excluded %d of %d" % (name, order, mode, err, (~keep).sum(), keep.size))
    assert (~keep).mean() < 0.02
    assert err <= 1e-12


@pytest.mark.parametrize("order", range(1, 6))
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_mirror_equals_scipy_map_coordinates(name, order):
    X, D, crop, O, off = _case(name)
    n = X.ndim
    rng = np.random.default_rng(7)
    r = rng.uniform(-np.array(X.shape, float), 2.0 * np.array(X.shape) - 1, size=(400, n))
    got = sref.reference(X, r, range(n), order, "mirror").V[:, 0]
    want = scipy.ndimage.map_coordinates(X, r.T, order=order, mode="mirror")
    err = np.abs(got - want).max()
    print("%s order %d: max |err| %.3g" % (name, order, err))
    assert err <= 1e-12


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", range(1, 6))
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_g_equals_central_differences_of_the_value(name, order, mode):
    X, D, crop, O, off = _case(name)
    n = X.ndim
    I = np.array(X.shape, float)
    rng = np.random.default_rng(9)
    r = rng.uniform(-I, 2.0 * I - 1, size=(300, n))
    # away from every window change: integers and half-integers of the mapped coordinate, the array's ends, the folds
    m = sref.reference(X, r, range(n), order, mode).m.T
    frac = np.abs(m * 2 - np.round(m * 2)) / 2
    if mode in ("constant", "nearest"):                       # (outside, the value does not depend on that axis)
        frac = np.where((r < 0) | (r > I - 1), np.inf, frac)
    edge = np.minimum(np.abs(r), np.abs(r - (I - 1)))
    if mode == "wrap":
        edge = np.minimum(edge, np.abs(r / (I - 1) - np.round(r / (I - 1))) * (I - 1))
    far = (np.minimum(frac, edge) > 1e-3).all(1)
    r = r[far]
    assert len(r) >= 200
    dV = rng.standard_normal((len(r), 1))
    ref = sref.reference(X, r, range(n), order, mode, dV=dV)
    h = 1e-5
    for a in range(n):
        e = np.zeros(n)
        e[a] = h
        up = sref.reference(X, r + e, range(n), order, mode).V
        dn = sref.reference(X, r - e, range(n), order, mode).V
        want = (dV * (up - dn)).sum(-1) / (2 * h)
        scale = np.maximum(ref.S_g[:, a], 1.0)
        err = (np.abs(ref.g[:, a] - want) / scale).max()
        print("%s order %d %s axis %d: max rel err %.3g" % (name, order, mode, a, err))
        assert err <= 1e-6


def test_order_0_is_one_tap_at_the_nearest_sample():
    X = np.arange(7.0)
    r = np.array([[0.4], [0.6], [5.49], [2.0]])
    s = sref.reference(X, r, [0], 0, "nearest")
    np.testing.assert_array_equal(s.V[:, 0], [0.0, 1.0, 5.0, 2.0])
    assert s.inside.all()


def test_dead_points_take_cval_and_an_empty_row():
    X = np.random.default_rng(1).uniform(size=(6, 5))
    r = np.array([[np.nan, 1.0], [2.0, np.inf], [-0.5, 1.0], [2.5, 2.5]])
    s = sref.reference(X, r, [0, 1], 3, "constant", cval=7.0, matrix=True)
    np.testing.assert_array_equal(s.dead, [True, True, True, False])
    np.testing.assert_array_equal(s.inside, [False, False, False, True])
    np.testing.assert_array_equal(s.V[:3, 0], 7.0)
    assert not s.A[:3].any() and abs(s.A[3].sum() - 1.0) < 1e-12
    s = sref.reference(X, r, [0, 1], 3, "mirror", cval=7.0)
    np.testing.assert_array_equal(s.dead, [True, True, False, False])
