"""
GPU tests of deform_grid_labels / deform_grid_labels_batch (run with `-m gpu` on the MI355X box), through the product
path: Python API -> ctypes -> edhip_deform_labels -> deform_vote.hip.

The expected value is the definition, computed with the CPU oracle class by class: with the classes being the distinct
values of L together with cval, in ascending order,
    s_c = oracle.deform_grid((L == c) as float64, D, order=1, mode, cval = 1.0 if c == cval else 0.0, ...)
and the label is the class with the largest s_c, updated with a strict `>` (so the smallest label wins a tie); the
weight is float32(best s_c).  Every comparison is bit equality.
"""
import numpy as np
import pytest

from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402

MODES = ["nearest", "wrap", "reflect", "mirror", "constant"]


def expected(L, D, cval=0, **kw):
    """(labels, best score, second best score) of the definition; the second best is -1 where there is one class"""
    classes = sorted(set(int(v) for v in np.unique(L)) | {int(cval)})
    lab = best = second = None
    for c in classes:
        s = orc.deform_grid((L == L.dtype.type(c)).astype(np.float64), D, order=1,
                            cval=1.0 if c == int(cval) else 0.0, **kw)
        if best is None:
            lab, best, second = np.full(s.shape, c, dtype=L.dtype), s.copy(), np.full(s.shape, -1.0)
            continue
        upd = s > best
        second = np.maximum(second, np.where(upd, best, s))
        lab[upd] = L.dtype.type(c)
        best = np.where(upd, s, best)
    return lab, best, second


def check(L, D, cval=0, **kw):
    """the call with return_weight against the definition; returns (labels, number of exactly tied voxels)"""
    want, best, second = expected(L, D, cval=cval, **kw)
    got, wt = ed.deform_grid_labels(L, D, cval=cval, return_weight=True, **kw)
    assert got.dtype == L.dtype and wt.dtype == np.float32 and got.shape == want.shape == wt.shape
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(wt, best.astype(np.float32))
    return got, int((best == second).sum())


def grids_and_affines(n, rng):
    """the grids and affines of test_label_kernel_ties_and_dtypes_bit_exact, reduced to n axes"""
    pts = {1: (4,), 2: (3, 4), 3: (3, 4, 3)}[n]
    grids = {
        "zero": np.zeros((n,) + (3,) * n),
        "half": np.full((n,) + pts, 0.5),
        "mhalf": np.full((n,) + (3,) * n, -1.5),
        "random": rng.standard_normal((n,) + (3,) * n) * 4,
    }
    half = np.concatenate([np.eye(n), np.full((n, 1), 0.5)], axis=1)
    shift = np.concatenate([np.eye(n), np.array([[-3.0], [2.0], [7.0]])[:n]], axis=1)
    return grids, {"none": None, "half": half, "shift": shift}


@pytest.mark.parametrize("mode", MODES)
def test_3d_every_mode_ties_included(mode):
    """(22, 27, 31) uint8, 5 labels, cval = 3: zero / constant / random grids with and without the half-voxel affine
    (every weight product 1/8: ties between equally frequent labels) and with a shift affine."""
    rng = np.random.default_rng(12)
    L = rng.integers(0, 5, (22, 27, 31)).astype(np.uint8)
    grids, affines = grids_and_affines(3, rng)
    ties = {}
    for gname, D in grids.items():
        for aname, aff in affines.items():
            _, ties[gname, aname] = check(L, D, cval=3, mode=mode, affine=aff)
    # the tie rule is exercised: the oracle's own best and second-best scores are equal somewhere
    assert ties["zero", "half"] > 0, ties


@pytest.mark.parametrize("mode", MODES)
def test_2d_and_1d(mode):
    rng = np.random.default_rng(13)
    L2 = rng.integers(0, 5, (37, 45)).astype(np.uint8)
    grids, affines = grids_and_affines(2, rng)
    ties = 0
    for D in grids.values():
        for aff in affines.values():
            ties += check(L2, D, cval=3, mode=mode, affine=aff)[1]
        ties += check(L2, D, cval=3, mode=mode, rotate=20, zoom=1.3)[1]
    assert ties > 0
    L1 = rng.integers(0, 5, (50,)).astype(np.uint8)
    grids, affines = grids_and_affines(1, rng)
    ties = 0
    for D in grids.values():
        for aff in affines.values():
            ties += check(L1, D, cval=3, mode=mode, affine=aff)[1]
    assert ties > 0


@pytest.mark.parametrize("dtype", [np.bool_, np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64,
                                   np.uint64])
def test_every_integer_dtype(dtype):
    """(9, 10, 11): 200 random labels (eight distinct labels in one cell), negative labels with a constructed tie
    between -3 and 2 that -3 wins, 2^53 and 2^53 + 1 as different classes of the 64-bit types."""
    rng = np.random.default_rng(14)
    dt = np.dtype(dtype)
    shape = (9, 10, 11)
    if dt.kind == "b":
        L = rng.integers(0, 2, shape).astype(dtype)
    elif dt.kind == "i":
        L = rng.integers(-100, 100, shape).astype(dtype)
    else:
        L = rng.integers(0, 200, shape).astype(dtype)
    low, high = (-3, 2) if dt.kind == "i" else (0, 1) if dt.kind == "b" else (2, 9)
    # the affine [I | 0.5] moves the image by half a voxel: output voxel o reads the cell o - 1 .. o with every weight
    # 1/8.  The cell of output voxel (3, 4, 5): four voxels of each label
    L[2:4, 3:5, 4:6] = np.array([low, high, high, low, high, low, low, high], dtype=dtype).reshape(2, 2, 2)
    big = 2 ** 53
    if dt.itemsize == 8:
        # the cell of output voxel (6, 6, 6): five voxels of 2^53 + 1 against three of 2^53 (one class of 8/8 if the
        # labels went through a double)
        L[5:7, 5:7, 5:7] = np.array([big + 1, big, big + 1, big + 1, big, big + 1, big, big + 1],
                                    dtype=dtype).reshape(2, 2, 2)
    if dt.kind != "b":
        cells = np.lib.stride_tricks.sliding_window_view(L, (2, 2, 2)).reshape(-1, 8)
        assert max(len(set(c.tolist())) for c in cells) == 8
    half = np.concatenate([np.eye(3), np.full((3, 1), 0.5)], axis=1)
    cval = low
    got, ties = check(L, np.zeros((3, 3, 3, 3)), cval=cval, mode="mirror", affine=half)
    assert ties > 0 and got[3, 4, 5] == low
    if dt.itemsize == 8:
        assert got[6, 6, 6] == big + 1 and (got == big).any()
    D = rng.standard_normal((3, 3, 3, 3)) * 2
    check(L, D, cval=cval, mode="constant")
    check(L, D, cval=cval, mode="wrap", affine=half)


def test_blocky_map_keeps_its_labels():
    """Nested cubes of labels 0 / 1 / 7 in 40^3: the vote never stores a value that is not in the map, where
    deform_grid(order=1) on the same map does -- and it differs from order 0."""
    rng = np.random.default_rng(15)
    L = np.zeros((40, 40, 40), dtype=np.uint8)
    L[8:32, 8:32, 8:32] = 1
    L[15:25, 15:25, 15:25] = 7
    D = rng.standard_normal((3, 3, 3, 3)) * 3
    got, _ = check(L, D, mode="nearest")
    assert set(np.unique(got).tolist()) <= {0, 1, 7}
    assert (got != ed.deform_grid(L, D, order=0, mode="nearest")).any()
    assert not set(np.unique(ed.deform_grid(L, D, order=1, mode="nearest")).tolist()) <= {0, 1, 7}


@pytest.mark.parametrize("mode", ["mirror", "constant"])
def test_crop_channel_axis_strides_and_lists(mode):
    """crop + channel axis + non-contiguous input, per-input lists of axis / mode / cval: a list gives a list"""
    rng = np.random.default_rng(16)
    V = rng.integers(-2, 4, (3, 40, 50, 36)).astype(np.int32).swapaxes(2, 3)      # (3, 40, 36, 50), strided
    L = rng.integers(0, 5, (44, 36, 50)).astype(np.uint8)[2:42]
    assert not V.flags.c_contiguous
    D = rng.standard_normal((3, 3, 3, 3)) * 3
    axis = [(1, 2, 3), (0, 1, 2)]
    crop = (slice(5, 30), slice(3, 33), slice(10, 45))
    modes, cvals = [mode, "nearest"], [-2, 4]
    res = ed.deform_grid_labels([V, L], D, mode=modes, cval=cvals, axis=axis, crop=crop, return_weight=True)
    assert isinstance(res, list) and len(res) == 2
    for i, X in enumerate((V, L)):
        want, best, _ = expected(X, D, cval=cvals[i], mode=modes[i], axis=axis[i], crop=crop)
        np.testing.assert_array_equal(res[i][0], want)
        np.testing.assert_array_equal(res[i][1], best.astype(np.float32))
    labels = ed.deform_grid_labels([V, L], D, mode=modes, cval=cvals, axis=axis, crop=crop)
    assert isinstance(labels, list)
    for (want, _), got in zip(res, labels):
        np.testing.assert_array_equal(got, want)


def test_control_grid_too_large_for_lds():
    """(2, 64, 64) = 8192 values, above the 7680 the kernel stages in LDS: the control grid is read from global memory"""
    rng = np.random.default_rng(17)
    L = rng.integers(0, 4, (40, 40)).astype(np.int16)
    D = rng.standard_normal((2, 64, 64))
    for mode in ("reflect", "constant"):
        check(L, D, cval=1, mode=mode)


def test_batch_equals_single_calls_and_the_definition():
    rng = np.random.default_rng(18)
    L = rng.integers(0, 5, (3, 20, 24, 28)).astype(np.uint8)
    D = rng.standard_normal((3, 3, 3, 3, 3)) * 3
    aff = np.eye(3, 4) + 0.03 * rng.standard_normal((3, 4))
    kw = dict(mode="reflect", cval=2, affine=aff)
    got, wt = ed.deform_grid_labels_batch(L, D, return_weight=True, **kw)
    assert got.shape == L.shape and got.dtype == L.dtype and wt.shape == L.shape and wt.dtype == np.float32
    np.testing.assert_array_equal(ed.deform_grid_labels_batch(L, D, **kw), got)
    for b in range(3):
        one, one_wt = ed.deform_grid_labels(L[b], D[b], return_weight=True, **kw)
        np.testing.assert_array_equal(got[b], one)
        np.testing.assert_array_equal(wt[b], one_wt)
        want, best, _ = expected(L[b], D[b], **kw)
        np.testing.assert_array_equal(got[b], want)
        np.testing.assert_array_equal(wt[b], best.astype(np.float32))


def test_determinism_families_and_hip_graph():
    """A repeated call and a call on device tensors give the bits of the numpy call; the call can be captured into a
    HIP graph (after a warm-up on the capture stream) and replayed on new data."""
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(19)
    shape = (30, 33, 35)

    def data():
        return rng.integers(0, 6, shape).astype(np.int32), rng.standard_normal((3, 4, 4, 4)) * 2.0

    L, D = data()
    kw = dict(mode="mirror", return_weight=True)
    first, first_wt = ed.deform_grid_labels(L, D, **kw)
    again, again_wt = ed.deform_grid_labels(L, D, **kw)
    np.testing.assert_array_equal(again, first)
    np.testing.assert_array_equal(again_wt, first_wt)
    Lt, Dt = torch.from_numpy(L).to(dev), torch.from_numpy(D).to(dev)
    yt, wt = ed.deform_grid_labels(Lt, Dt, **kw)
    assert yt.is_cuda and yt.dtype == torch.int32 and wt.is_cuda and wt.dtype == torch.float32
    np.testing.assert_array_equal(yt.cpu().numpy(), first)
    np.testing.assert_array_equal(wt.cpu().numpy(), first_wt)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):                          # warm-up on the capture stream
            ed.deform_grid_labels(Lt, Dt, **kw)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        y, w = ed.deform_grid_labels(Lt, Dt, **kw)
    for rep in range(2):
        L, D = data()
        Lt.copy_(torch.from_numpy(L))
        Dt.copy_(torch.from_numpy(D))
        g.replay()
        torch.cuda.synchronize()
        y_rep, w_rep = y.clone(), w.clone()
        y_eager, w_eager = ed.deform_grid_labels(Lt, Dt, **kw)
        assert torch.equal(y_rep, y_eager) and torch.equal(w_rep, w_eager), rep
        np.testing.assert_array_equal(y_rep.cpu().numpy(), ed.deform_grid_labels(L, D, mode="mirror"))


def test_length_one_deformed_axis():
    L = np.full((12, 1, 9), 5, dtype=np.uint16)
    D = np.random.default_rng(20).standard_normal((3, 3, 3, 3))
    for mode in ("nearest", "constant"):
        got, wt = ed.deform_grid_labels(L, D, mode=mode, cval=7, return_weight=True)
        assert got.dtype == np.uint16 and (got == 7).all() and wt.dtype == np.float32 and (wt == 1.0).all()
        np.testing.assert_array_equal(got, orc.deform_grid(L, D, order=1, mode=mode, cval=7.0))
    dev = torch.device("cuda", torch.cuda.current_device())
    got = ed.deform_grid_labels(torch.from_numpy(L.astype(np.int32)).to(dev), D, cval=-1)
    assert got.is_cuda and got.dtype == torch.int32 and bool((got == -1).all())
