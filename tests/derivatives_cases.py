"""
The cases the GPU tests of deform_grid_derivatives and of its adjoint share (tests/test_derivatives.py,
tests/test_derivatives_gradient.py): grids, extents, positions, cotangents and the NumPy reference of each, computed
once and never modified.  TEST INFRASTRUCTURE ONLY.

The shapes are the smallest at which the kernels can go wrong: a two-point grid (every tap folds), odd extents with a
crop, a homogeneous affine map, rotate and zoom, three axes, and grids of 2 x 64 x 64 = 8192 and 3 x 14^3 = 8232 values,
more than the 7680 that are staged in LDS.  Of the 1000 positions of a case the first two sit on the first and the last
knot exactly, the third on an inner knot where the extents allow an exact one, the fourth is NaN and the fifth lies
beyond a control coordinate of 4e15; the others are uniform over [-0.3 I, 1.3 I], so about a third lie outside the
image.  A test on N points takes the first N.
"""
import functools

import numpy as np

import derivatives_reference as xref
import jacobian_reference as jref

AFFINE2 = np.array([[1.1, 0.15, -1.5], [-0.1, 0.9, 2.0], [0.0, 0.0, 1.0]])
AFFINE3 = np.array([[1.05, 0.1, 0.0, -1.0], [-0.08, 0.95, 0.05, 0.5], [0.02, -0.04, 1.1, 1.5]])

CASES = {
    "1d-two-points": dict(I=(9,), ncp=(2,), sigma=1.0),
    "2d-crop-affine-rotate-zoom": dict(I=(13, 17), ncp=(4, 5), sigma=2.0, crop=(slice(2, 11), slice(3, 15)),
                                       affine=AFFINE2, rotate=20.0, zoom=1.3),
    "3d-affine-crop": dict(I=(12, 14, 10), ncp=(4, 4, 5), sigma=1.5, affine=AFFINE3,
                           crop=(slice(1, 11), slice(0, 12), slice(2, 9))),
    "2d-global-grid": dict(I=(70, 70), ncp=(64, 64), sigma=0.5),            # 8192 grid values, more than 7680
    "3d-global-grid": dict(I=(16, 16, 16), ncp=(14, 14, 14), sigma=0.5),    # 8232 grid values
}
NAMES = list(CASES)
COUNTS = (0, 1, 63, 64, 65, 257, 1000)
NMAX = 1000
NAN_ROW, FAR_ROW = 3, 4
WHICH = ("u", "A", "G", "all")


def case(name):
    """(I, D float64, the keyword arguments of the call)"""
    c = dict(CASES[name])
    I, ncp, sigma = c.pop("I"), c.pop("ncp"), c.pop("sigma")
    n = len(I)
    D = np.random.default_rng(200 + len(name) + 7 * n).standard_normal((n,) + ncp) * sigma
    return I, D, c


@functools.lru_cache(maxsize=None)
def data(name):
    """(q (1000, n), u, A, G) of a case, read-only"""
    I, D, kw = case(name)
    n = len(I)
    rng = np.random.default_rng(17 + len(name))
    _, _, off, _ = jref.geometry(I, D, **kw)
    q = np.stack([rng.uniform(-0.3 * I[k], 1.3 * I[k], NMAX) - off[k] for k in range(n)], axis=-1)
    for k in range(n):
        q[0, k] = -off[k]                                    # cp = 0
        q[1, k] = (I[k] - 1) - off[k]                        # cp = ncp - 1
        if (I[k] - 1) % (D.shape[k + 1] - 1) == 0:
            q[2, k] = (I[k] - 1) // (D.shape[k + 1] - 1) - off[k]       # cp = 1
    q[NAN_ROW, 0] = np.nan
    q[FAR_ROW, n - 1] = 1e17
    u, A, G = rng.standard_normal((NMAX, n)), rng.standard_normal((NMAX, n, n)), rng.standard_normal((NMAX, n, n, n))
    for a in (q, u, A, G):
        a.setflags(write=False)
    return q, u, A, G


def cotangents(name, which, count=NMAX):
    """dict(d_coordinates, d_jacobian, d_hessian) of the first `count` points: the ones `which` names, None otherwise"""
    _, u, A, G = data(name)
    return dict(d_coordinates=u[:count] if which in ("u", "all") else None,
                d_jacobian=A[:count] if which in ("A", "all") else None,
                d_hessian=G[:count] if which in ("G", "all") else None)


@functools.lru_cache(maxsize=None)
def reference(name, count=NMAX, which=None):
    """the reference on the first `count` points, with the gradients for the cotangents `which` names; read-only"""
    I, D, kw = case(name)
    q = data(name)[0][:count]
    c = cotangents(name, which, count) if which else {}
    ref = xref.reference(D, I, q, u=c.get("d_coordinates"), A=c.get("d_jacobian"), G=c.get("d_hessian"), **kw)
    for a in ref:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def output_shape(name):
    """the deformed extents of what deform_grid returns for the case (the centre of rotate / zoom)"""
    I, D, kw = case(name)
    return tuple(jref.geometry(I, D, **kw)[1])
