"""
GPU tests of deform_grid_sample / deform_grid_sample_batch (edhip_deform_sample): the deformed image at real output
positions, V_i = S_X(r(q_i)).

Expected values come from tests/sample_reference.py (NumPy; anchored on the CPU oracle, on SciPy and on central
differences by tests/test_sample_reference_host.py), in two ways:

A. at the library's own coordinates, r = ed.deform_grid_coordinates(q): that call is tested against its own reference
   elsewhere (tests/test_points.py) and runs the device code the sample kernel runs, so the remainder is arithmetic
   only -- fp64 sums of at most 6^3 products of values below about 3: 1e-11 absolute for float64, one float32 ulp of
   the value on top for float32, integers exact;
B. end to end with no shared code: on the integer lattice of O against the CPU oracle's deform_grid.  Coordinates agree
   to 1e-10 (tests/test_points.py) and the interpolant of X in [0, 1] has a slope of about 10 per voxel at most: 1e-8
   absolute for float64, one float32 ulp on top for float32, integers exact.

A point is left out only where the expected r lies within 1e-6 of a decision boundary (half-integers for order 0 and
integer outputs; 0 and I_k - 1 for 'constant' and `inside`; the fold points of 'wrap'); the excluded share is asserted
to be below 2 %.  An integer output whose fp64 value lies within 1e-3 of a rounding tie is not left out (on a lattice of
40 voxels one such voxel is 2.5 %): it must be one of the two neighbours.
"""
import numpy as np
import pytest

import sample_cases as sc
import sample_reference as sref
from oracle import ed_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import elasticdeform_amd as ed  # noqa: E402
import elasticdeform_amd.torch as etorch  # noqa: E402

TOL_A = 1e-11
TOL_B = 1e-8
DTYPES = [np.float64, np.float32, np.int16]

exact_prefilter = pytest.fixture(autouse=True)(sc.exact_prefilter)


# ---- A. values against the reference at the library's own coordinates -------------------------------------------

@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_values_at_the_library_coordinates(name, order):
    I, D, kw, O = sc.case(name)
    n = len(I)
    q = sc.positions(3, O)
    r = ed.deform_grid_coordinates(q, D, I, **kw)
    for dtype in DTYPES:
        X = sc.image(17 + n, I, dtype)
        for mode in sc.MODES:
            for prefilter in (True, False):
                V, inside = ed.deform_grid_sample(X, q, D, order=order, mode=mode, cval=sc.CVAL, prefilter=prefilter,
                                                  return_inside=True, **kw)
                assert V.shape == (len(q),) and V.dtype == X.dtype and inside.dtype == np.bool_
                ref = sref.reference(X, r, range(n), order, mode, sc.CVAL, prefilter)
                keep = sc.compare_values(V, ref, r, I, order, mode, TOL_A, "%s order %d %s %s prefilter %d"
                                         % (name, order, np.dtype(dtype).name, mode, prefilter))
                np.testing.assert_array_equal(inside[keep], ref.inside[keep])


# ---- B. values end to end, on the integer lattice, against the oracle --------------------------------------------

@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_integer_lattice_equals_the_oracle(name, order):
    I, D, kw, O = sc.case(name)
    n = len(I)
    lattice = np.stack(np.indices(O), axis=-1).reshape(-1, n).astype(np.float64)
    r = sc.reference_coordinates(lattice, D, I, kw)
    for dtype in DTYPES:
        X = sc.image(17 + n, I, dtype)
        for mode in sc.MODES:
            want = orc.deform_grid(X, D, order=order, mode=mode, cval=sc.CVAL, **kw).reshape(-1)
            V = ed.deform_grid_sample(X, lattice, D, order=order, mode=mode, cval=sc.CVAL, **kw)
            # the oracle's stored voxels are compared; the fp64 reference value only places the rounding ties
            ref = sref.reference(X, r, range(n), order, mode, sc.CVAL)
            integer = np.dtype(dtype).kind in "iub"
            skip = sref.boundary_distance(r, I, order, mode, integer) < sc.EDGE
            err = np.abs(V.astype(np.float64) - want.astype(np.float64))[~skip]
            if integer:
                # (within 1e-3 of a rounding tie of the fp64 value either neighbour may be stored)
                bound = (np.abs(ref.V[:, 0] - np.floor(ref.V[:, 0]) - 0.5) < 1e-3)[~skip].astype(np.float64)
            else:
                bound = TOL_B + (np.spacing(np.abs(want[~skip]).astype(np.float32)).astype(np.float64)
                                 if dtype == np.float32 else 0.0)
            print("%s order %d %s %s: max |err| %.3g over %d voxels, excluded share %.4f"
                  % (name, order, np.dtype(dtype).name, mode, err.max(), (~skip).sum(), skip.mean()))
            assert skip.mean() < 0.02
            assert (err <= bound).all()


# ---- positions that are not finite or not sane -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["1d", "2d-crop", "3d-affine", "2d-global-grid"])
def test_positions_that_are_not_sane_give_cval_in_every_mode(name):
    I, D, kw, O = sc.case(name)
    n = len(I)
    q = sc.positions(4, O)[:64]
    bad = np.arange(0, 64, 4)
    q[bad[0::4], 0] = np.nan
    q[bad[1::4], n - 1] = np.inf
    q[bad[2::4], 0] = -np.inf
    q[bad[3::4], n - 1] = 1e17                                   # |control coordinate| > 4e15
    good = np.setdiff1d(np.arange(64), bad)
    for dtype in (np.float64, np.int16):
        X = sc.image(5, I, dtype)
        for mode in sc.MODES:
            for order in (0, 1, 3):
                V, inside = ed.deform_grid_sample(X, q, D, order=order, mode=mode, cval=7.0, return_inside=True, **kw)
                np.testing.assert_array_equal(V[bad], np.full(len(bad), 7, dtype=dtype))
                assert not inside[bad].any()
                clean = ed.deform_grid_sample(X, q[good], D, order=order, mode=mode, cval=7.0, **kw)
                np.testing.assert_array_equal(V[good], clean)


# ---- contracts -----------------------------------------------------------------------------------------------------

def _contract_case(name="3d-affine", dtype=np.float64):
    I, D, kw, O = sc.case(name)
    return I, D, kw, sc.positions(8, O), sc.image(9, I, dtype)


@pytest.mark.parametrize("name", ["2d-crop", "3d-affine", "2d-global-grid"])
def test_a_sample_of_a_batch_equals_the_single_call(name):
    I, D, kw, O = sc.case(name)
    B = 3
    rng = np.random.default_rng(12)
    Xs = rng.uniform(size=(B,) + I)
    Ds = np.stack([D * s for s in (1.0, 0.5, -0.7)])
    qs = np.stack([sc.positions(20 + b, O)[:257] for b in range(B)])
    V, inside = ed.deform_grid_sample_batch(Xs, qs, Ds, order=3, mode="mirror", return_inside=True, **kw)
    assert V.shape == (B, 257) and inside.shape == (B, 257)
    for b in range(B):
        v, i = ed.deform_grid_sample(Xs[b], qs[b], Ds[b], order=3, mode="mirror", return_inside=True, **kw)
        np.testing.assert_array_equal(V[b], v)
        np.testing.assert_array_equal(inside[b], i)


def test_repeats_slices_and_permutations_give_the_same_bits():
    I, D, kw, q, X = _contract_case()
    V = ed.deform_grid_sample(X, q, D, order=3, mode="reflect", **kw)
    np.testing.assert_array_equal(V, ed.deform_grid_sample(X, q, D, order=3, mode="reflect", **kw))
    np.testing.assert_array_equal(V[100:377], ed.deform_grid_sample(X, q[100:377], D, order=3, mode="reflect", **kw))
    perm = np.random.default_rng(1).permutation(len(q))
    np.testing.assert_array_equal(V[perm], ed.deform_grid_sample(X, q[perm], D, order=3, mode="reflect", **kw))
    # leading dimensions of the positions are carried through
    V2 = ed.deform_grid_sample(X, q.reshape(20, 30, 3), D, order=3, mode="reflect", **kw)
    np.testing.assert_array_equal(V2, V.reshape(20, 30))


def test_non_contiguous_and_transposed_inputs_and_positions():
    I, D, kw, q, X = _contract_case()
    V = ed.deform_grid_sample(X, q, D, order=2, mode="wrap", **kw)
    wide = np.zeros((len(q), 7))
    wide[:, 1:7:2] = q
    np.testing.assert_array_equal(V, ed.deform_grid_sample(X, wide[:, 1:7:2], D, order=2, mode="wrap", **kw))
    Xt = np.ascontiguousarray(X.transpose(2, 0, 1)).transpose(1, 2, 0)       # same values, other strides
    assert not Xt.flags.c_contiguous
    np.testing.assert_array_equal(V, ed.deform_grid_sample(Xt, q, D, order=2, mode="wrap", **kw))
    Xc = torch.from_numpy(np.repeat(X, 2, axis=2)).cuda()[:, :, ::2]          # a strided tensor on the device
    qc = torch.from_numpy(np.ascontiguousarray(q.T)).cuda().T
    got = ed.deform_grid_sample(Xc, qc, torch.from_numpy(D).cuda(), order=2, mode="wrap", **kw)
    np.testing.assert_array_equal(V, got.cpu().numpy())


def test_step_axes_before_and_after_the_deformed_axes():
    I, D, kw, O = sc.case("2d-crop")
    q = sc.positions(8, O)
    X = np.random.default_rng(3).uniform(size=(2,) + I + (3,))
    V = ed.deform_grid_sample(X, q, D, order=3, mode="nearest", axis=(1, 2), **kw)
    assert V.shape == (2, 3, len(q))
    for c in range(2):
        for d in range(3):
            np.testing.assert_array_equal(V[c, d], ed.deform_grid_sample(X[c, :, :, d], q, D, order=3, mode="nearest",
                                                                         **kw))
    first = ed.deform_grid_sample(X[:, :, :, 0], q.reshape(4, 150, 2), D, order=3, mode="nearest", axis=(1, 2), **kw)
    assert first.shape == (2, 4, 150)
    np.testing.assert_array_equal(first.reshape(2, -1), V[:, 0])
    last = ed.deform_grid_sample(np.moveaxis(X[:, :, :, 0], 0, -1), q, D, order=3, mode="nearest", axis=(0, 1), **kw)
    np.testing.assert_array_equal(last, V[:, 0])


def test_a_list_of_two_inputs_each_with_its_own_order_and_mode():
    I, D, kw, q, X = _contract_case()
    L = sc.image(10, I, np.uint8)
    out = ed.deform_grid_sample([X, L], q, D, order=[3, 0], mode=["mirror", "nearest"], cval=[0.0, 3.0], **kw)
    assert isinstance(out, list) and len(out) == 2 and out[1].dtype == np.uint8
    np.testing.assert_array_equal(out[0], ed.deform_grid_sample(X, q, D, order=3, mode="mirror", **kw))
    np.testing.assert_array_equal(out[1], ed.deform_grid_sample(L, q, D, order=0, mode="nearest", cval=3.0, **kw))
    pairs = ed.deform_grid_sample([X, L], q, D, order=[3, 0], mode=["mirror", "nearest"], return_inside=True, **kw)
    np.testing.assert_array_equal(pairs[0][1], pairs[1][1])


def test_numpy_in_numpy_out_and_tensor_in_tensor_out():
    I, D, kw, q, X = _contract_case(dtype=np.float32)
    V = ed.deform_grid_sample(X, q, D, **kw)
    assert isinstance(V, np.ndarray) and V.dtype == np.float32
    Vt, it = ed.deform_grid_sample(torch.from_numpy(X).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(D).cuda(),
                                   return_inside=True, **kw)
    assert torch.is_tensor(Vt) and Vt.is_cuda and Vt.dtype == torch.float32 and it.dtype == torch.bool
    np.testing.assert_array_equal(V, Vt.cpu().numpy())
    q32 = q.astype(np.float32)                                   # float32 positions are widened at the load
    np.testing.assert_array_equal(ed.deform_grid_sample(X, q32, D, **kw),
                                  ed.deform_grid_sample(X, q32.astype(np.float64), D, **kw))
    assert etorch.deform_grid_sample_batch is ed.deform_grid_sample_batch


def test_no_points():
    I, D, kw, q, X = _contract_case()
    V, inside = ed.deform_grid_sample(X, q[:0], D, return_inside=True, **kw)
    assert V.shape == (0,) and V.dtype == X.dtype and inside.shape == (0,)
    V = ed.deform_grid_sample(np.stack([X, X]), q[:0], D, axis=(1, 2, 3), **kw)
    assert V.shape == (2, 0)


def test_more_points_than_the_launch_covers():
    """N = 2048 * 256 + 77 points on the 1-D case: the grid-stride route"""
    I, D, kw, O = sc.case("1d")
    N = 2048 * 256 + 77
    gen = torch.Generator(device="cuda").manual_seed(5)
    q = (torch.rand((N, 1), generator=gen, device="cuda", dtype=torch.float64) * (O[0] + 3) - 2)
    X = torch.from_numpy(sc.image(2, I)).cuda()
    Dt = torch.from_numpy(D).cuda()
    V, inside = ed.deform_grid_sample(X, q, Dt, order=3, mode="mirror", return_inside=True)
    tail = slice(N - 1500, N)
    v, i = ed.deform_grid_sample(X, q[tail], Dt, order=3, mode="mirror", return_inside=True)
    assert torch.equal(V[tail], v) and torch.equal(inside[tail], i)
    pick = torch.cat([torch.arange(0, 300, device="cuda"), torch.arange(N - 300, N, device="cuda")])
    qp = q[pick].cpu().numpy()
    r = ed.deform_grid_coordinates(qp, D, I)
    ref = sref.reference(sc.image(2, I), r, [0], 3, "mirror")
    sc.compare_values(V[pick].cpu().numpy(), ref, r, I, 3, "mirror", TOL_A, "grid-stride")


def test_capture_into_a_graph():
    """after one warm-up call on the capture stream (the prefilters use that stream's workspace), the call captured in
    a graph and replayed three times, with an eager call of another shape in between, gives the eager bits"""
    I, D, kw, q, X = _contract_case()
    Xt, qt, Dt = torch.from_numpy(X).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(D).cuda()
    V0, in0 = ed.deform_grid_sample(Xt, qt, Dt, order=3, mode="mirror", return_inside=True, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ed.deform_grid_sample(Xt, qt, Dt, order=3, mode="mirror", return_inside=True, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        V, inside = ed.deform_grid_sample(Xt, qt, Dt, order=3, mode="mirror", return_inside=True, **kw)
    I2, D2, kw2, O2 = sc.case("2d-crop")
    for _ in range(3):
        V.zero_()
        ed.deform_grid_sample(sc.image(1, I2), sc.positions(2, O2)[:50], D2, **kw2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(V, V0) and torch.equal(inside, in0)
