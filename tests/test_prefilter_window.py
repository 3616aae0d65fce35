"""
The windowed prefilter passes (edhip_spline_filter_axes_window), called directly with hand-written windows.

The library's promise (include/edhip.h, TileGeo in spline_fast.hip): samples outside the window are neither read nor
written, lines inside it are filtered as lines of the window's length.  The host sizes tile, grid and LDS for the whole
array and the kernel shrinks its geometry on the device, so every case here makes the two differ somewhere.  One run
checks all three parts:

* the input holds NaN outside the window ("not read": a NaN that reaches the window's output is a read outside);
* the output starts as a sentinel bit pattern (a NaN with a payload) and is compared as integers outside the window
  ("not written"); in place, the input's own bits outside the window must survive;
* inside the window the result equals tests/prefilter_reference.windowed() (the fp64 chain on the contiguous copy of
  the window) within the tolerances of test_fast_prefilter_kernels: 2e-6 of the result's scale in float32, 1e-13 in
  float64.

Only valid windows are used -- what edhip_source_window guarantees: 0 <= w0 < w1 <= shape[d], at least 64 samples on a
filtered axis, and w0 / w1 of the last dimension on multiples of the vector width (4 float32 / 2 float64) whenever the
last extent is one (otherwise the launcher takes the scalar kernels and any window goes).

The windowed call is served by the whole-line tile kernels alone, so it also marks where they end: it accepts the
contiguous axis up to 1024 samples and a strided axis up to 576 and declines one sample beyond (the table in
tests/test_prefilter_routes.py) -- with nothing launched, which the dry pre-pass of a chain guarantees even when only
its last pass is outside the envelope.
"""
import importlib

import numpy as np
import pytest

import prefilter_reference as pref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from elasticdeform_amd import _lib  # noqa: E402

DTYPES = {"float32": (np.float32, np.int32, 0x7fc0dead, 4, 2e-6),
          "float64": (np.float64, np.int64, 0x7ff8dead0000beef, 2, 1e-13)}


def _env():
    dgm = importlib.import_module("elasticdeform_amd.deform_grid")
    dev = torch.device("cuda", torch.cuda.current_device())
    return dgm, dev, torch.cuda.current_stream(dev).cuda_stream


def _check_valid(shape, window, axes, vn):
    assert len(window) == len(shape)
    for d, (w0, w1) in enumerate(window):
        assert 0 <= w0 < w1 <= shape[d], (d, window)
    for a in axes:
        assert window[a][1] - window[a][0] >= 64, (a, window)
    if shape[-1] % vn == 0:
        assert window[-1][0] % vn == 0 and window[-1][1] % vn == 0, window


def _inputs(dtype, shape, window, seed):
    """(x with NaN outside the window, the same with zeros outside for the reference)"""
    ftype = DTYPES[dtype][0]
    rng = np.random.default_rng(seed)
    sl = pref.window_slices(window)
    x = np.full(shape, np.nan, dtype=ftype)
    x[sl] = rng.standard_normal(x[sl].shape).astype(ftype)
    return x


def _sentinel(dtype, shape, dev):
    _, itype, bits, _, _ = DTYPES[dtype]
    s = np.full(shape, bits, dtype=itype)
    return s, torch.from_numpy(s.view(DTYPES[dtype][0])).to(dev)


def _run(dtype, shape, window, axes, order, transpose, inplace, seed=0):
    """one windowed call; returns (status, result as numpy, bits the untouched part must still have)"""
    dgm, dev, stream = _env()
    ftype, itype, _, vn, tol = DTYPES[dtype]
    _check_valid(shape, window, axes, vn)
    x = _inputs(dtype, shape, window, seed)
    win = torch.tensor([w for pair in window for w in pair], dtype=torch.int32, device=dev)
    xd = torch.from_numpy(x).to(dev)
    if inplace:
        before, out = x.view(itype).copy(), xd
    else:
        before, out = _sentinel(dtype, shape, dev)
    st = _lib.spline_filter_axes_window(dgm._desc(xd), dgm._desc(out), list(axes), order, transpose, win.data_ptr(),
                                        _lib.FLAG_AUTO, stream)
    torch.cuda.synchronize(dev)
    if not inplace:      # the input of an out-of-place call is never written
        np.testing.assert_array_equal(xd.cpu().numpy().view(itype), x.view(itype))
    return st, out.cpu().numpy(), before, x


def _check(dtype, shape, window, axes, seed=0, orders=(2, 3)):
    ftype, itype, _, vn, tol = DTYPES[dtype]
    sl = pref.window_slices(window)
    outside = np.ones(shape, dtype=bool)
    outside[sl] = False
    for order in orders:
        for transpose in (False, True):
            want = None
            for inplace in (False, True):
                st, got, before, x = _run(dtype, shape, window, axes, order, transpose, inplace, seed)
                what = (dtype, shape, window, axes, order, transpose, inplace)
                assert st == 0, what
                if want is None:
                    want = pref.windowed(x, window, axes, order, transpose)[sl]
                # not written: every bit outside the window is what it was
                np.testing.assert_array_equal(got.view(itype)[outside], before[outside], err_msg=str(what))
                # not read: no NaN came in
                assert not np.isnan(got[sl]).any(), what
                scale = np.abs(want).max()
                err = np.abs(got[sl].astype(np.float64) - want).max()
                print("window %s: err %.3e of scale (bound %.1e)" % (what, err / scale, tol))
                assert err <= tol * scale, (what, err / scale)


# ---- geometries ------------------------------------------------------------------------------------------------------
# array of 320 samples along a STRIDED axis (host: 10 blocks, half-width columns), windows of 64, 65, 96, 97 and 288
# samples at the start, in the interior and at the end; the column window moves too (multiples of 4)
STRIDED_320 = [
    ((320, 40), ((0, 64), (0, 40)), (0,)),
    ((320, 40), ((100, 165), (4, 36)), (0,)),
    ((320, 40), ((224, 320), (8, 40)), (0,)),
    ((320, 40), ((223, 320), (0, 40)), (0,)),
    ((320, 40), ((16, 304), (12, 32)), (0,)),
    ((320, 40), ((0, 65), (20, 24)), (0,)),
    ((320, 40), ((256, 320), (0, 28)), (0,)),
    ((320, 40), ((120, 216), (0, 40)), (0,)),
    ((320, 40), ((0, 97), (4, 40)), (0,)),
    ((320, 40), ((32, 320), (0, 40)), (0,)),
]
# the same along the CONTIGUOUS axis; 65 and 97 on an array whose last extent (321) is no multiple of the vector width
CONTIG_320 = [
    ((24, 320), ((0, 24), (0, 64)), (1,)),
    ((24, 320), ((3, 20), (112, 208)), (1,)),
    ((24, 320), ((0, 24), (256, 320)), (1,)),
    ((24, 320), ((5, 24), (32, 320)), (1,)),
    ((24, 320), ((0, 11), (0, 288)), (1,)),
    ((24, 320), ((2, 3), (224, 320)), (1,)),
    ((24, 321), ((0, 24), (0, 65)), (1,)),
    ((24, 321), ((1, 23), (100, 197)), (1,)),
    ((24, 321), ((0, 24), (256, 321)), (1,)),
    ((24, 321), ((7, 8), (224, 321)), (1,)),
    ((24, 321), ((0, 24), (3, 291)), (1,)),
]
OTHER = [
    # an outer window of length 1 (both axis kinds)
    ((50, 128), ((7, 8), (0, 128)), (1,)),
    ((128, 80), ((0, 128), (36, 40)), (0,)),
    ((9, 128, 16), ((4, 5), (10, 100), (0, 16)), (1,)),
    # contiguous axis, tile height R = 32 (n = 128): 7 lines (below R), 45 lines (no multiple of it), 33 (one over)
    ((50, 128), ((3, 10), (0, 128)), (1,)),
    ((50, 128), ((3, 48), (32, 128)), (1,)),
    ((50, 128), ((17, 50), (0, 96)), (1,)),
    # ... R = 16 (n = 320: 10 blocks) and R = 8 (n = 600: 19 blocks): 5 / 19 / 9 lines
    ((40, 320), ((30, 35), (0, 320)), (1,)),
    ((40, 600), ((2, 21), (100, 500)), (1,)),
    ((40, 600), ((31, 40), (0, 600)), (1,)),
    # strided axis, full-width columns (C = 64 float32 / 32 float64): a column window that is no multiple of C,
    # one narrower than C / 2 although the array's 80 columns made the host pick the full width, one of exactly C + 4
    ((128, 80), ((0, 128), (4, 76)), (0,)),
    ((128, 80), ((10, 110), (8, 28)), (0,)),
    ((128, 80), ((60, 128), (12, 80)), (0,)),
    ((128, 200), ((0, 70), (64, 132)), (0,)),
    # half-width columns because the array itself has at most C / 2 of them
    ((100, 16), ((20, 90), (4, 12)), (0,)),
    # scalar kernels (last extent no multiple of the vector width): any column window
    ((128, 81), ((5, 128), (3, 70)), (0,)),
    ((130, 67), ((0, 65), (1, 2)), (0,)),
    # 3, 4 and 5 dimensions, every outer window narrower than its axis (the device's outer lengths, not the host's);
    # 5 dimensions with a contiguous line fill the kWinOuter = 4 outer lengths, 6 with a strided one do
    ((6, 10, 128), ((1, 5), (2, 7), (32, 128)), (2,)),
    ((6, 96, 24), ((1, 5), (10, 90), (4, 20)), (1,)),
    ((80, 7, 24), ((8, 72), (2, 6), (8, 24)), (0,)),
    ((3, 5, 70, 12), ((1, 3), (1, 4), (2, 68), (4, 12)), (2,)),
    ((3, 5, 6, 72), ((0, 2), (2, 5), (1, 4), (4, 72)), (3,)),
    ((72, 3, 5, 8), ((0, 66), (1, 3), (1, 5), (0, 4)), (0,)),
    ((2, 3, 64, 4, 8), ((1, 2), (1, 3), (0, 64), (1, 3), (4, 8)), (2,)),
    ((3, 3, 4, 5, 68), ((1, 3), (0, 2), (1, 4), (2, 5), (0, 64)), (4,)),
    ((2, 70, 3, 3, 9), ((0, 2), (3, 69), (1, 3), (0, 2), (2, 7)), (1,)),
    ((2, 2, 3, 66, 3, 8), ((1, 2), (0, 2), (1, 3), (1, 66), (0, 2), (4, 8)), (3,)),
]
# chains (first pass in -> out, the rest in place), as the forward and the gradient path run them
CHAINS = [
    ((72, 70, 80), ((4, 70), (3, 68), (8, 76)), (0, 1, 2)),
    ((72, 70, 81), ((0, 64), (6, 70), (5, 81)), (0, 1, 2)),
    ((3, 90, 100), ((1, 3), (10, 80), (20, 96)), (1, 2)),
    ((100, 90, 6), ((13, 78), (0, 90), (2, 6)), (0, 1)),
]


def _ids(cases):
    return ["%s-%s-ax%s" % ("x".join(map(str, s)), "_".join("%d:%d" % w for w in win), "".join(map(str, ax)))
            for s, win, ax in cases]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", STRIDED_320 + CONTIG_320, ids=_ids(STRIDED_320 + CONTIG_320))
def test_window_shorter_than_the_array_along_the_filtered_axis(case, dtype):
    """array 320 / 321, windows of 64, 65, 96, 97, 288 samples at the start, inside and at the end: the device's
    block count differs from the host's"""
    shape, window, axes = case
    _check(dtype, shape, window, axes, seed=1)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", OTHER, ids=_ids(OTHER))
def test_outer_and_column_windows(case, dtype):
    """outer windows of length 1, line counts below / across the tile height, column windows that are no multiple of
    the column width or narrower than half of it, arrays of 2 to 6 dimensions"""
    shape, window, axes = case
    _check(dtype, shape, window, axes, seed=2)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", CHAINS, ids=_ids(CHAINS))
def test_chains_over_several_axes(case, dtype):
    """every pass after the first runs in place in the output, whose samples outside the window are sentinel NaNs:
    a pass that reads or writes outside the window shows in either check"""
    shape, window, axes = case
    _check(dtype, shape, window, axes, seed=3)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_window_equal_to_the_array_gives_the_bits_of_the_plain_call(dtype):
    """same kernel, same geometry: bit for bit -- one pass of each axis kind, vector and scalar kernels, a chain"""
    dgm, dev, stream = _env()
    ftype, itype, _, vn, tol = DTYPES[dtype]
    rng = np.random.default_rng(5)
    for shape, axes in (((320, 40), (0,)), ((24, 320), (1,)), ((128, 81), (0,)), ((24, 321), (1,)), ((128, 80), (0,)),
                        ((100, 16), (0,)), ((40, 600), (1,)), ((3, 5, 70, 12), (2,)), ((72, 70, 80), (0, 1, 2))):
        x = rng.standard_normal(shape).astype(ftype)
        xd = torch.from_numpy(x).to(dev)
        win = torch.tensor([v for n in shape for v in (0, n)], dtype=torch.int32, device=dev)
        for order in (2, 3):
            for transpose in (False, True):
                plain = torch.empty_like(xd)
                _lib.spline_filter_axes(dgm._desc(xd), dgm._desc(plain), list(axes), order, transpose, _lib.FLAG_AUTO,
                                        stream)
                _, out = _sentinel(dtype, shape, dev)
                st = _lib.spline_filter_axes_window(dgm._desc(xd), dgm._desc(out), list(axes), order, transpose,
                                                    win.data_ptr(), _lib.FLAG_AUTO, stream)
                assert st == 0
                np.testing.assert_array_equal(out.cpu().numpy().view(itype), plain.cpu().numpy().view(itype),
                                              err_msg=str((shape, axes, order, transpose)))
                buf = xd.clone()
                st = _lib.spline_filter_axes_window(dgm._desc(buf), dgm._desc(buf), list(axes), order, transpose,
                                                    win.data_ptr(), _lib.FLAG_AUTO, stream)
                assert st == 0
                np.testing.assert_array_equal(buf.cpu().numpy().view(itype), plain.cpu().numpy().view(itype),
                                              err_msg=str((shape, axes, order, transpose, "in place")))


# ---- the envelope: what is outside it declines with nothing launched ---------------------------------------------

def _declines(dtype, shape, axes, order, window=None):
    dgm, dev, stream = _env()
    ftype, itype, _, vn, tol = DTYPES[dtype]
    x = np.random.default_rng(7).standard_normal(shape).astype(ftype)
    xd = torch.from_numpy(x).to(dev)
    window = window or tuple((0, n) for n in shape)
    win = torch.tensor([v for pair in window for v in pair], dtype=torch.int32, device=dev)
    for transpose in (False, True):
        before, out = _sentinel(dtype, shape, dev)
        st = _lib.spline_filter_axes_window(dgm._desc(xd), dgm._desc(out), list(axes), order, transpose,
                                            win.data_ptr(), _lib.FLAG_AUTO, stream)
        torch.cuda.synchronize(dev)
        assert st == _lib.ERR_UNSUPPORTED, (dtype, shape, axes, order, transpose, st)
        np.testing.assert_array_equal(out.cpu().numpy().view(itype), before,
                                      err_msg="a declined call wrote: %s" % str((dtype, shape, axes, order, transpose)))
        np.testing.assert_array_equal(xd.cpu().numpy(), x)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_declines_launch_nothing(dtype):
    # two poles
    for order in (4, 5):
        _declines(dtype, (128, 80), (0,), order)
        _declines(dtype, (24, 320), (1,), order)
        _declines(dtype, (72, 70, 80), (0, 1, 2), order)
    for order in (2, 3):
        # an array axis shorter than 64 (either axis kind)
        _declines(dtype, (48, 64), (0,), order)
        _declines(dtype, (64, 63), (1,), order)
        # a strided axis longer than the tile kernels take, a contiguous one
        _declines(dtype, (577, 16), (0,), order)
        _declines(dtype, (600, 16), (0,), order, window=((100, 200), (0, 16)))
        _declines(dtype, (8, 1025), (1,), order)
        # more outer axes than kWinOuter = 4: six dimensions around a contiguous line, seven around a strided one
        _declines(dtype, (2, 2, 2, 2, 3, 64), (5,), order)
        _declines(dtype, (2, 2, 2, 64, 2, 2, 4), (3,), order)
        # chains whose LAST pass is the unsupported one: the passes before it must not have run
        _declines(dtype, (80, 40, 72), (0, 2, 1), order)
        _declines(dtype, (64, 600, 8), (0, 1), order)
        _declines(dtype, (80, 72, 40), (0, 1, 2), order, window=((8, 72), (0, 64), (0, 40)))
        _declines(dtype, (2, 2, 2, 2, 66, 64), (4, 5), order)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_longest_lines_the_windowed_call_takes(dtype):
    """the last length on the tile kernels' side of each boundary: contiguous 1024 (R = 8, 8 * 32 blocks = kBlock),
    strided 576 (18 blocks, half-width columns in 80 KiB) -- whole and windowed; 1025 / 577 decline above"""
    _check(dtype, (12, 1024), ((0, 12), (0, 1024)), (1,), seed=8, orders=(3,))
    _check(dtype, (12, 1024), ((2, 11), (4, 1000)), (1,), seed=8, orders=(3,))
    _check(dtype, (576, 40), ((0, 576), (0, 40)), (0,), seed=9, orders=(3,))
    _check(dtype, (576, 40), ((1, 576), (8, 36)), (0,), seed=9, orders=(3,))
