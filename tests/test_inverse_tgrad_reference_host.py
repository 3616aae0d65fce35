"""
Host tests that anchor the analytic reference of the gradients of deform_grid_inverse with respect to the deformation
(tests/inverse_tgrad_reference.py) before anything runs on a GPU.

1. The conditions the GPU comparison relies on, through the reference alone: with a NumPy Newton every voxel of the
   five cases solves at tol = 1e-12 in at most 5 steps, min det J is what the case table states, and no q_h lies
   within 1e-6 of an integer, a half-integer, 0 or O_h - 1.
2. dD and dK against central differences of L(D, K) = <dZ, map_coordinates(Y, q(D, K), mode='mirror')> with that
   Newton: h = 1e-5 on the four entries of D with the largest |dD|, h = 1e-6 on K[0, n], orders 1 and 3, 1e-5
   relative: h^2 times a third derivative of order 10, with a decade to spare.
3. The share of the solver difference in the GPU bound: every q_h shifted by +-4e-10 moves no element of dD or dK by
   more than the printed fraction of its scale S; by linearity 4e-12 (two solvers at tol = 1e-12, |J^-1|_inf <= 2)
   gives a hundredth of it.
"""
import functools

import numpy as np
import pytest
import scipy.ndimage

import inverse_tgrad_reference as itr
from oracle import dgrad_reference as dref

NAMES = list(itr.CASES)


@functools.lru_cache(maxsize=None)
def _solved(name):
    I, O, D, kw, Y, dZ = itr.case(name)
    _, I_, O_, off, K = itr.geometry(dZ, D, **kw)
    q, steps, res = itr.newton(itr.lattice(I), D, I, off, K)
    return q, steps, res, off, K


@pytest.mark.parametrize("name", NAMES)
def test_every_voxel_solves_and_none_sits_on_a_boundary(name):
    I, O, D, kw, Y, dZ = itr.case(name)
    q, steps, res, off, K = _solved(name)
    det = np.linalg.det(itr.jacobian(q, D, I, off, K))
    print("%s: %d steps, residual %.3g, min det J %.3g" % (name, steps, res, det.min()))
    assert steps <= 5 and res <= 1.0e-12
    assert abs(det.min() - itr.MIN_DET[name]) < 0.005
    for order in (1, 2):                                         # integers, then half-integers; 0 and O - 1 in both
        assert not itr.near_boundary(q, O, order).any()


def _loss(Y, dZ, D, I, off, K, order):
    q, _, res = itr.newton(itr.lattice(I), D, I, off, K)
    assert res <= 1e-12
    return float((dZ.reshape(-1) * scipy.ndimage.map_coordinates(Y, q.T, order=order, mode="mirror")).sum())


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("name", ["1d-affine", "2d-crop-mild", "2d-rz"])
def test_reference_equals_central_differences(name, order):
    I, O, D, kw, Y, dZ = itr.case(name)
    q, _, _, off, K = _solved(name)
    n = len(I)
    if order == 1:
        # a kink within reach of the finite-difference step: that voxel is left out of L
        kink = itr.near_boundary(q, O, 1, 1e-3).reshape(I)
        assert kink.mean() < 0.01
        dZ = np.where(kink, 0.0, dZ)
    r = itr.reference(Y, dZ, D, q, np.ones(q.shape[0], bool), order=order, mode="mirror", **kw)
    entries = [np.unravel_index(i, D.shape) for i in np.argsort(-np.abs(r.dD).reshape(-1))[:4]]
    for idx in entries:
        h = 1e-5
        Dp, Dm = D.copy(), D.copy()
        Dp[idx] += h
        Dm[idx] -= h
        fd = (_loss(Y, dZ, Dp, I, off, K, order) - _loss(Y, dZ, Dm, I, off, K, order)) / (2 * h)
        print("%s order %d dD%s: reference %.12g, central difference %.12g" % (name, order, idx, r.dD[idx], fd))
        assert abs(fd - r.dD[idx]) <= 1e-5 * abs(r.dD[idx])
    h = 1e-6
    Kp, Km = K.copy(), K.copy()
    Kp[0, n] += h
    Km[0, n] -= h
    fd = (_loss(Y, dZ, D, I, off, Kp, order) - _loss(Y, dZ, D, I, off, Km, order)) / (2 * h)
    print("%s order %d dK[0, n]: reference %.12g, central difference %.12g" % (name, order, r.dK[0, n], fd))
    assert abs(fd - r.dK[0, n]) <= 1e-5 * abs(r.dK[0, n])


@pytest.mark.parametrize("name", NAMES)
def test_share_of_the_solver_difference(name):
    """a shift of every q_h by +-4e-10 (random signs) moves dD and dK by the printed share of S; at 4e-12 a hundredth"""
    I, O, D, kw, Y, dZ = itr.case(name)
    q, _, _, off, K = _solved(name)
    ok = np.ones(q.shape[0], bool)
    worst = 0.0
    for order in (1, 3):
        r = itr.reference(Y, dZ, D, q, ok, order=order, mode="mirror", **kw)
        shift = 4e-10 * np.random.default_rng(3).choice([-1.0, 1.0], size=q.shape)
        s = itr.reference(Y, dZ, D, q + shift, ok, order=order, mode="mirror", **kw)
        share = max(float((np.abs(s.dD - r.dD) / r.S_D).max()), float((np.abs(s.dK - r.dK) / r.S_K).max()))
        print("%s order %d: a 4e-10 shift moves an element by %.3g S at most" % (name, order, share))
        worst = max(worst, share)
    assert worst * 1e-2 <= 1e-11
