"""The general rows of the z-walk forward route (csrc/deform_k1z.hip, k1z_gen_body): the boxes of the tiles on the x
faces, staged by rows with every 16-byte chunk clamped into its own source row and the misplaced and mirrored elements
put in place from LDS, and the work list the general workgroups deal among themselves (heavy strips first, a cursor per
XCD, counters and cursors cleared from call to call).  Shapes are the smallest at which that code can go wrong: arrays
narrower than a box row (both x faces in one tile, a boundary map that folds more than once), partial x tiles, wide row
pitches, volumes that are views of larger buffers, many more strips than workgroups, no general strip at all.
Everything under ``set_field_strength('strong')`` (the route then serves these small calls) against the oracle, with
the tolerance of tests/test_zwalk_route.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ed_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402

TOL = dict(rtol=1e-5, atol=3e-5)       # (tests/test_zwalk_route.py)
MODES = ["nearest", "wrap", "reflect", "mirror", "constant"]
PAD = 1e30                              # what lies beside a view's rows: one element of it in a box shows in the output


@pytest.fixture(autouse=True)
def strong_field():
    prev = ed.set_field_strength("strong")
    yield
    ed.set_field_strength(prev)


def _check(X, disp, msg="", **kw):
    np.testing.assert_allclose(ed.deform_grid(X, disp, **kw), orc.deform_grid(X, disp, **kw), err_msg=msg, **TOL)


@pytest.mark.parametrize("mode", MODES)
def test_narrow_arrays_every_mode_and_order(mode):
    """x extents 8, 9, 12, 17 and 24 (z and y of 16-24): one x tile that holds both faces, a box row wider than the
    array (the map folds more than once at 8 and 9), partial x tiles; orders 1-3 (order 2 reads the padding tap);
    displacements of a few voxels, so that boxes reach beyond both ends."""
    rng = np.random.default_rng(MODES.index(mode) + 40)
    for nx, nz, ny in ((8, 16, 24), (9, 24, 17), (12, 19, 16), (17, 16, 21), (24, 20, 18)):
        X = rng.random((nz, ny, nx)).astype(np.float32)
        for order in (1, 2, 3):
            disp = rng.standard_normal((3, 3, 4, 3)) * 2.5
            _check(X, disp, "x extent %d order %d" % (nx, order), order=order, mode=mode, cval=-0.5)


@pytest.mark.parametrize("nx", [8, 9, 12, 17, 24])
def test_narrow_arrays_crop_and_affine(nx):
    """A crop whose offsets are not multiples of 8 (the boxes' x origins take every residue mod 4) and an affine map
    (rotation and shear about the centre), on every narrow extent."""
    rng = np.random.default_rng(nx)
    X = rng.random((22, 23, nx)).astype(np.float32)
    disp = rng.standard_normal((3, 4, 4, 3)) * 2.0
    crop = (slice(3, 20), slice(5, 21), slice(min(3, nx - 6), nx - 1))
    aff = np.eye(3, 4)
    aff[:, :3] += rng.standard_normal((3, 3)) * 0.08
    aff[:, 3] = rng.standard_normal(3) * 1.5
    for order, mode in ((3, "mirror"), (2, "reflect"), (1, "constant")):
        _check(X, disp, "crop order %d" % order, order=order, mode=mode, cval=0.25, crop=crop)
        _check(X, disp, "affine order %d" % order, order=order, mode=mode, cval=0.25, affine=aff)


@pytest.mark.parametrize("stretch", [1.5, 2.2, 3.5])
def test_wide_pitches_at_the_x_faces(stretch):
    """24 x 24 x 40 under an affine map that stretches x by 1.5 / 2.2 / 3.5 and shears it along y by 0.8: a tile's
    8 x 8 outputs span 7 (stretch + 0.8) + 1 source columns, and with the 4-5 taps of a window its box rows hold
    ~21 / ~26 / ~35 elements -- the row pitches 24, 32 and 48 -- at the x faces, where the stretched coordinates fold
    back into the array."""
    rng = np.random.default_rng(int(stretch * 10))
    X = rng.random((24, 24, 40)).astype(np.float32)
    disp = rng.standard_normal((3, 3, 3, 4)) * 1.0
    aff = np.eye(3, 4)
    aff[2, 2] = stretch
    aff[2, 1] = 0.8
    for order, mode in ((3, "mirror"), (2, "wrap"), (3, "nearest"), (1, "reflect")):
        _check(X, disp, "order %d %s" % (order, mode), order=order, mode=mode, affine=aff)


@pytest.mark.parametrize("nx", [9, 17, 24])
def test_views_of_larger_buffers(nx):
    """The volume as a view with padded rows (elements of 1e30 before and behind every row) and as a view that starts
    at a non-zero offset of a larger buffer: a chunk that read beyond its own row would bring 1e30 into a box.  No
    prefilter, so the kernels read the views themselves."""
    rng = np.random.default_rng(nx + 100)
    shape = (18, 20, nx)
    X = rng.random(shape).astype(np.float32)
    disp = rng.standard_normal((3, 3, 3, 3)) * 2.5
    dd = torch.from_numpy(disp).cuda()
    padded = torch.full((shape[0], shape[1] + 2, nx + 11), PAD, dtype=torch.float32, device="cuda")
    rows = padded[:, 1:-1, 5:5 + nx]
    rows.copy_(torch.from_numpy(X))
    flat = torch.full((X.size + 1500,), PAD, dtype=torch.float32, device="cuda")
    inner = flat[777:777 + X.size].view(shape)
    inner.copy_(torch.from_numpy(X))
    assert not rows.is_contiguous() and rows.storage_offset() > 0 and inner.storage_offset() == 777
    for order, mode in ((3, "mirror"), (2, "reflect"), (1, "wrap"), (3, "constant")):
        kw = dict(order=order, mode=mode, cval=-1.0, prefilter=False)
        want = orc.deform_grid(X, disp, **kw)
        for name, view in (("padded rows", rows), ("offset", inner)):
            np.testing.assert_allclose(ed.deform_grid(view, dd, **kw).cpu().numpy(), want,
                                       err_msg="%s order %d %s" % (name, order, mode), **TOL)


def test_step_axes_and_batch():
    """Three channels on a step axis (the boxes are staged once per channel) and a batch of three volumes, narrow
    along x."""
    rng = np.random.default_rng(77)
    Xc = rng.random((3, 20, 18, 12)).astype(np.float32)
    disp = rng.standard_normal((3, 3, 3, 3)) * 2.0
    for order, mode in ((3, "mirror"), (2, "nearest")):
        _check(Xc, disp, "channels order %d" % order, order=order, mode=mode, axis=(1, 2, 3))
    B, shape = 3, (20, 18, 9)
    X = rng.random((B,) + shape).astype(np.float32)
    db = rng.standard_normal((B, 3, 3, 3, 3)) * 2.0
    got = ed.deform_grid_batch(torch.from_numpy(X).cuda(), torch.from_numpy(db).cuda(), order=3, mode="reflect")
    for b in range(B):
        np.testing.assert_allclose(got[b].cpu().numpy(), orc.deform_grid(X[b], db[b], order=3, mode="reflect"),
                                   err_msg="sample %d" % b, **TOL)


# ---- the work list ------------------------------------------------------------------------------------------------

def test_no_general_strip():
    """A crop well inside a 64^3 volume under a mild field: every tile is class A, list G is empty and the general
    workgroups leave at once."""
    rng = np.random.default_rng(8)
    X = rng.random((64, 64, 64)).astype(np.float32)
    disp = rng.standard_normal((3, 4, 4, 4)) * 0.5
    crop = (slice(16, 48), slice(16, 48), slice(16, 48))
    for order in (1, 3):
        _check(X, disp, "order %d" % order, order=order, mode="mirror", crop=crop)


@pytest.mark.parametrize("B", [64, 100])
def test_more_items_than_workgroups(B):
    """A batch of 24^3 volumes: every strip has general tiles.  64 volumes: 1152 strips, as many items as general
    workgroups; 100 volumes: 1800 items for the 1280 general workgroups a launch has at most."""
    rng = np.random.default_rng(B)
    X = rng.random((B, 24, 24, 24)).astype(np.float32)
    disp = rng.standard_normal((B, 3, 3, 3, 3)) * 2.0
    got = ed.deform_grid_batch(torch.from_numpy(X).cuda(), torch.from_numpy(disp).cuda(), order=3, mode="mirror").cpu().numpy()
    for b in range(B):
        np.testing.assert_allclose(got[b], orc.deform_grid(X[b], disp[b], order=3, mode="mirror"), err_msg="sample %d" % b, **TOL)


def test_alternating_shapes_on_one_stream():
    """Three calls, two shapes, no synchronisation between them: each call's counters and cursors were cleared by the
    call before it.  A stale count or cursor would skip strips or take entries of the other shape's list."""
    rng = np.random.default_rng(31)
    Xa, Xb = rng.random((24, 40, 17)).astype(np.float32), rng.random((56, 16, 48)).astype(np.float32)
    da, db = rng.standard_normal((3, 3, 3, 3)) * 2.0, rng.standard_normal((3, 4, 3, 4)) * 2.0
    Xad, Xbd, dad, dbd = (torch.from_numpy(a).cuda() for a in (Xa, Xb, da, db))
    kw = dict(order=3, mode="mirror")
    torch.cuda.synchronize()
    outs = [ed.deform_grid(Xad, dad, **kw), ed.deform_grid(Xbd, dbd, **kw), ed.deform_grid(Xad, dad, **kw),
            ed.deform_grid(Xbd, dbd, **kw), ed.deform_grid(Xbd, dbd, **kw)]
    torch.cuda.synchronize()
    wa, wb = orc.deform_grid(Xa, da, **kw), orc.deform_grid(Xb, db, **kw)
    for k, (o, w) in enumerate(zip(outs, (wa, wb, wa, wb, wb))):
        np.testing.assert_allclose(o.cpu().numpy(), w, err_msg="call %d" % k, **TOL)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]) and torch.equal(outs[3], outs[4])


def test_crop_identity_at_an_x_offset_of_3():
    """full[crop] == the cropped call, bit for bit, for a crop that starts at x = 3: the cropped call's tiles sit at
    other offsets in other boxes, staged by rows or by LDS-DMA as they lie, and gather the same values."""
    rng = np.random.default_rng(13)
    X = rng.random((24, 24, 24)).astype(np.float32)
    Xd = torch.from_numpy(X).cuda()
    crop = (slice(2, 18), slice(1, 17), slice(3, 21))
    for order, mode in ((3, "mirror"), (2, "reflect"), (1, "nearest")):
        dd = torch.from_numpy(rng.standard_normal((3, 3, 3, 3)) * 2.0).cuda()
        full = ed.deform_grid(Xd, dd, order=order, mode=mode)
        part = ed.deform_grid(Xd, dd, order=order, mode=mode, crop=crop)
        assert torch.equal(full[crop], part), (order, mode)
