"""
What tests/test_sample.py and tests/test_sample_gradient.py share: the geometries of tests/test_points.py (small, and
every route of the front is among them), the images, the positions and the exclusion rule.  TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import sample_reference as sref
from oracle import ed_oracle as orc

AFFINE3 = np.array([[1.05, 0.1, 0.0, -1.0], [-0.08, 0.95, 0.05, 0.5], [0.02, -0.04, 1.1, 1.5]])
CROP2 = (slice(2, 11), slice(3, 15))

CASES = {
    "1d": dict(I=(40,), ncp=(5,), sigma=2.0),
    "2d-crop": dict(I=(13, 17), ncp=(4, 5), sigma=3.0, crop=CROP2),
    "3d": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5),
    "3d-affine": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5, affine=AFFINE3),
    "2d-rotate-zoom-crop": dict(I=(13, 17), ncp=(4, 5), sigma=3.0, crop=CROP2, rotate=20.0, zoom=1.3),
    "2d-global-grid": dict(I=(70, 70), ncp=(64, 64), sigma=0.5),   # 8192 grid values: the global-memory grid route
    "1d-short-grid": dict(I=(9,), ncp=(2,), sigma=1.0),            # two control points: every window is mirrored
}
NAMES = sorted(CASES)
MODES = ["constant", "nearest", "mirror", "reflect", "wrap"]
ORDERS = [0, 1, 2, 3, 4, 5]
CVAL = 0.25
EDGE = 1e-6


def out_shape(I, crop):
    return tuple(I) if crop is None else tuple((s.stop or i) - (s.start or 0) for s, i in zip(crop, I))


def offsets(crop, n):
    return np.zeros(n) if crop is None else np.array([float(s.start or 0) for s in crop])


def inverse_map(I, crop=None, affine=None, rotate=None, zoom=None):
    """the inverse map K of the call, from the oracle's restatement of the reference's matrix algebra"""
    if affine is None and rotate is None and zoom is None:
        return None
    return orc._inverse_affine(affine, rotate, zoom, len(I), list(out_shape(I, crop)))


def case(name):
    """(I, the control grid, the call's keyword arguments, O)"""
    c = dict(CASES[name])
    I, ncp, sigma = c.pop("I"), c.pop("ncp"), c.pop("sigma")
    D = np.random.default_rng(31 + len(name)).standard_normal((len(I),) + tuple(ncp)) * sigma
    return I, D, c, out_shape(I, c.get("crop"))


def image(seed, shape, dtype=np.float64):
    """X uniform in [0, 1]; integer types: scaled to the type's range, capped at +-1000"""
    x = np.random.default_rng(seed).uniform(0.0, 1.0, size=shape)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return x.astype(dtype)
    info = np.iinfo(dtype)
    lo, hi = max(info.min, -1000), min(info.max, 1000)
    return np.round(lo + x * (hi - lo)).astype(dtype)


def positions(seed, O):
    """500 positions uniform on [-2, O_k + 1] (mostly inside, a rim outside) and 100 on [-O_k, 2 O_k - 1] (several
    periods of mirror, reflect and wrap)"""
    rng = np.random.default_rng(seed)
    O = np.asarray(O, dtype=np.float64)
    return np.concatenate([rng.uniform(-2.0, O + 1, size=(500, len(O))), rng.uniform(-O, 2 * O - 1, size=(100, len(O)))])


def reference_coordinates(q, D, I, kw):
    """r(q) from the NumPy restatement (oracle.dgrad_reference.coordinate)"""
    return sref.coordinate(q, D, I, offsets(kw.get("crop"), len(I)), inverse_map(I, **kw))


def exact_prefilter():
    """(a generator for an autouse fixture) the library's reference-order spline prefilter for the test, whatever the
    line length: with the default arithmetic, float32 lines of 64 samples and more take the fast prefilter, whose
    coefficients differ from the reference's in the last float32 bits -- a property of the prefilter, not of the calls
    under test, that would otherwise sit on top of the float32 tolerance"""
    import importlib
    api = importlib.import_module("elasticdeform_amd.deform_grid")
    before = {v: k for k, v in api._ARITHMETIC.items()}[api._flags]
    api.set_arithmetic("exact")
    yield
    api.set_arithmetic(before)


def compare_values(got, ref, r, I, order, mode, tol, what):
    """got (N,) or (N, steps) equals the store rule of ref.V: float64 within tol, float32 within tol plus one float32
    ulp of the value, integers exactly -- away from the decision boundaries (EDGE in r); an integer whose fp64 value
    lies within 1e-3 of a rounding tie may be either neighbour.  Prints the figures first.  Returns the mask of the
    compared points."""
    dtype = got.dtype
    integer = dtype.kind in "iub"
    N = r.shape[0]
    skip = sref.boundary_distance(r, I, order, mode, integer) < EDGE
    keep = ~skip
    g = got.reshape(N, -1)[keep].astype(np.float64)
    w = sref.store(ref.V, dtype)[keep].astype(np.float64)
    err = np.abs(g - w)
    if integer:
        bound = (np.abs(ref.V - np.floor(ref.V) - 0.5) < 1e-3)[keep].astype(np.float64)
    elif dtype == np.float32:
        bound = tol + np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
    else:
        bound = np.full_like(err, tol)
    print("%s: max |err| %.3g over %d points, excluded share %.4f"
          % (what, err.max() if err.size else 0.0, keep.sum(), skip.mean()))
    assert skip.mean() < 0.02
    assert not np.isnan(g).any()
    assert (err <= bound).all()
    return keep
