"""
GPU tests of the coordinate map's derivatives at real positions (elasticdeform_amd.deform_grid_derivatives, its batch
form; edhip_deform_points_derivatives).

Expected values: r and J are the bits of deform_grid_coordinates(..., jacobian=True) (the same device code); H comes
from tests/derivatives_reference.py (NumPy on oracle/dgrad_reference.py, anchored against difference quotients on the
CPU in tests/test_derivatives_reference_host.py) within 512 eps A_H per element, A_H the absolute-value sum of the
element's 4^n terms: 512 exceeds the roundings of a 64-tap, 4-factor sum.  Cases, positions and counts:
tests/derivatives_cases.py.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402

import derivatives_cases as cases  # noqa: E402

EPS = np.finfo(np.float64).eps


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _full(name):
    """the call on all 1000 positions; computed once, never modified"""
    I, D, kw = cases.case(name)
    out = ed.deform_grid_derivatives(cases.data(name)[0], D, I, **kw)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("count", cases.COUNTS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_values_bits_and_slices(name, count):
    I, D, kw = cases.case(name)
    n = len(I)
    q = cases.data(name)[0][:count]
    ref = cases.reference(name, count)
    out = ed.deform_grid_derivatives(q, D, I, **kw)
    assert isinstance(out, ed.MapDerivatives)
    r, J, H = out
    assert isinstance(H, np.ndarray) and H.dtype == np.float64 and H.shape == (count, n, n, n)
    # r and J: the bits of deform_grid_coordinates, with and without the second-derivative sweep
    r0, J0 = ed.deform_grid_coordinates(q, D, I, jacobian=True, **kw)
    assert _same(r, r0) and _same(J, J0)
    r1, J1, H1 = ed.deform_grid_derivatives(q, D, I, hessian=False, **kw)
    assert H1 is None and _same(r1, r) and _same(J1, J)
    # symmetry, bit for bit
    assert _same(H, np.swapaxes(H, -1, -2))
    # positions that are not sane: NaN everywhere; the others: the reference
    bad = ~ref.sane
    assert np.isnan(r[bad]).all() and np.isnan(J[bad]).all() and np.isnan(H[bad]).all()
    assert np.isfinite(H[~bad]).all()
    if count > cases.FAR_ROW:
        assert bad[cases.NAN_ROW] and bad[cases.FAR_ROW] and bad.sum() == 2
    ratio = np.abs(H - ref.H)[~bad] / (EPS * ref.A_H[~bad])
    print("%s N=%d: worst |H err| / (eps A_H) = %.2f" % (name, count, ratio.max() if ratio.size else 0.0))
    assert np.all(np.abs(H - ref.H)[~bad] <= 512 * EPS * ref.A_H[~bad])
    # a slice of the points: the rows of the whole call
    for got, whole in zip(out, _full(name)):
        assert _same(got, whole[:count])
    # a repeated call
    for got, again in zip(out, ed.deform_grid_derivatives(q, D, I, **kw)):
        assert _same(got, again)


@pytest.mark.parametrize("name", cases.NAMES)
def test_batch_equals_single_calls(name):
    I, D, kw = cases.case(name)
    rng = np.random.default_rng(5)
    q = cases.data(name)[0]
    qs = np.stack([q[:257], q[300:557], q[600:857]])
    Ds = np.stack([D, D + rng.standard_normal(D.shape), -D])
    out = ed.deform_grid_derivatives_batch(qs, Ds, I, **kw)
    for b in range(3):
        for got, want in zip(out, ed.deform_grid_derivatives(qs[b], Ds[b], I, **kw)):
            assert _same(got[b], want)
    r, J, H = ed.deform_grid_derivatives_batch(qs, Ds, I, hessian=False, **kw)
    assert H is None and _same(r, out.coordinates) and _same(J, out.jacobian)


@pytest.mark.parametrize("name", cases.NAMES)
def test_float32_positions_and_array_families(name):
    I, D, kw = cases.case(name)
    q32 = cases.data(name)[0][:257].astype(np.float32)
    r, J, H = ed.deform_grid_derivatives(q32, D, I, **kw)
    r64, J64, H64 = ed.deform_grid_derivatives(q32.astype(np.float64), D, I, **kw)
    assert r.dtype == np.float32 and _same(r, r64.astype(np.float32)) and _same(J, J64) and _same(H, H64)
    # tensors stay on their device; leading dimensions are kept
    qt = torch.from_numpy(q32.astype(np.float64)[:256].reshape(4, 64, -1)).cuda()
    out = ed.deform_grid_derivatives(qt, torch.from_numpy(D).cuda(), I, **kw)
    n = len(I)
    assert all(torch.is_tensor(t) and t.is_cuda for t in out)
    assert tuple(out.hessian.shape) == (4, 64, n, n, n) and tuple(out.jacobian.shape) == (4, 64, n, n)
    assert _same(out.hessian.cpu().numpy().reshape(256, n, n, n), H64[:256])
    # the wrapper without anything that requires a gradient is the package's own call
    out = etorch.deform_grid_derivatives(q32, D, I, **kw)
    assert isinstance(out, ed.MapDerivatives) and isinstance(out.hessian, np.ndarray) and _same(out.hessian, H)


def test_strided_positions():
    """a strided view of the positions is read as it is"""
    I, D, kw = cases.case("3d-affine-crop")
    q = cases.data("3d-affine-crop")[0][:65]
    wide = torch.from_numpy(np.concatenate([q, q], axis=1)).cuda()
    Dt = torch.from_numpy(D).cuda()
    out = ed.deform_grid_derivatives(wide[:, :3], Dt, I, **kw)
    want = ed.deform_grid_derivatives(q, D, I, **kw)
    assert _same(out.hessian.cpu().numpy(), want.hessian) and _same(out.coordinates.cpu().numpy(), want.coordinates)
