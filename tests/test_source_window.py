"""
edhip_source_window against source coordinates computed independently (SciPy's map_coordinates on the raw control grid,
plus the affine part and the offset -- as test_source_box_kernel_vs_oracle_coordinates does for edhip_source_box) and
the tap rule of tests/prefilter_reference.tap_range.

The contract (include/edhip.h), per deformed axis of length n, and what is asserted for it:

* superset: every tap of every output voxel, clipped to the axis, plus `margin` samples of decay on either side, is
  inside [w0, w1) -- for 'nearest' / 'constant', and for the folding modes while no tap leaves the axis;
* folding modes ('wrap', 'reflect', 'mirror') whose taps leave the axis get (0, n): a folded tap can land anywhere.
  (While every tap stays inside the axis nothing folds, and the window is the clipped one: that is the case the
  crop-aware prefilter exists for in the default mode.)
* shape: 0 <= w0 < w1 <= n; non-deformed dimensions get (0, shape[d]); the last dimension's w0 / w1 are multiples of
  `align` or the axis end; a deformed axis keeps at least min(minlen, n) samples;
* not needlessly wide: inside the EDHIP_FLAG_FAST hull of edhip_source_box for the same call plus taps, margin,
  alignment rounding and 2 samples per side, unless it was grown to `minlen` ("return the whole array" fails this);
* pinned: the window is exactly the hull's tap window with ONE guard sample per side (the kernels' own coordinate
  arithmetic may round differently; elasticdeform_amd/_host.source_box states the same rule for the host), `margin`
  around it, `minlen`, `align`.  A window one sample narrower costs accuracy in the last bits near a crop's edge, one
  wider costs time; neither shows anywhere else.
"""
import importlib

import numpy as np
import pytest
import scipy.ndimage

import prefilter_reference as pref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from elasticdeform_amd import _lib  # noqa: E402
from elasticdeform_amd._host import MODE_CODES  # noqa: E402

A2 = np.array([[1.1, 0.05, -3.0], [-0.08, 0.9, 2.0]])
A3 = np.array([[1.1, 0.05, 0, -3.0], [0, 0.9, 0.1, 2.0], [0.02, 0, 1.0, 1.0]])

# name -> (input shape, deformed dimensions, control points, sigma, output box)
GEOMETRIES = {
    "2d": ((90, 130), (0, 1), (4, 5), 5.0, (20, 30)),
    "3d": ((90, 100, 80), (0, 1, 2), (4, 3, 5), 7.0, (20, 30, 25)),
    "3d-leading-channel": ((2, 70, 100, 84), (1, 2, 3), (3, 4, 3), 4.0, (10, 30, 24)),
    "2d-trailing-channel": ((80, 128, 4), (0, 1), (5, 4), 6.0, (28, 10)),
}
# (margin, align, minlen)
SETTINGS = [(0, 1, 1), (16, 1, 1), (32, 1, 1), (16, 2, 1), (16, 4, 1), (0, 4, 1), (32, 2, 1),
            (0, 1, 64), (16, 4, 64), (32, 2, 64), (16, 1, 64)]
CLIP = ("nearest", "constant")


def _coordinates(disp, in_len, out_len, off, aff):
    """exact raw source coordinates c_h(o), each of shape out_len, in float64"""
    n = len(in_len)
    o = np.stack(np.meshgrid(*[np.arange(m, dtype=np.float64) for m in out_len], indexing="ij"))
    cp = [(disp.shape[k + 1] - 1) * (o[k] + off[k]) / (in_len[k] - 1) for k in range(n)]
    cs = []
    for h in range(n):
        d = scipy.ndimage.map_coordinates(disp[h].astype(np.float64), cp, order=3, mode="mirror")
        base = o[h] if aff is None else sum(aff[h, l] * o[l] for l in range(n)) + aff[h, n]
        cs.append(base + off[h] + d)
    return cs


def _expected_from_hull(hull_lo, hull_hi, n, order, mode, margin, align, minlen, last):
    """the contract applied to the hull box (see the module docstring): the pinned window"""
    lo = int(hull_lo) - order // 2 - 1
    hi = int(hull_hi) + order - order // 2 + 1            # inclusive
    if lo < 0 or hi > n - 1:
        if mode in CLIP:
            clipped_lo, clipped_hi = lo < 0, hi > n - 1
            lo, hi = min(max(lo, 0), n - 1), max(min(hi, n - 1), 0)
            # taps that stick out are mirror-indexed: up to `order` samples inward of the edge
            if clipped_lo:
                hi = max(hi, min(order, n - 1))
            if clipped_hi:
                lo = min(lo, max(n - 1 - order, 0))
        else:
            lo, hi = 0, n - 1
    w0, w1 = max(lo - margin, 0), min(hi + 1 + margin, n)
    if w1 - w0 < minlen:
        w0 = max(min(w0, n - minlen), 0)
        w1 = min(w0 + minlen, n)
    if last and align > 1:
        w0 -= w0 % align
        w1 = min(-(-w1 // align) * align, n)
    return w0, w1


@pytest.mark.parametrize("grid_dtype", [np.float64, np.float32], ids=["f64grid", "f32grid"])
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_source_window_against_independent_coordinates(name, grid_dtype):
    dgm = importlib.import_module("elasticdeform_amd.deform_grid")
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev).cuda_stream
    shape, axis, points, sigma, out_len = GEOMETRIES[name]
    naxis, ndim = len(axis), len(shape)
    in_len = tuple(shape[a] for a in axis)
    rng = np.random.default_rng(sum(map(ord, name)))
    disp = (rng.standard_normal((naxis,) + points) * sigma).astype(grid_dtype)
    dd = torch.from_numpy(disp).to(dev)
    flags = _lib.FLAG_RAW_DISPLACEMENT | _lib.FLAG_FAST           # what _crop_windows passes
    win = torch.empty(2 * ndim, dtype=torch.int32, device=dev)
    crops = {"corner": tuple(0 for _ in in_len),
             "interior": tuple((n - m) // 2 + 3 for n, m in zip(in_len, out_len)),
             "far-faces": tuple(n - m for n, m in zip(in_len, out_len))}
    seen = {"clipped": 0, "free": 0, "folded": 0, "fold-free": 0, "minlen": 0}
    for cname, off in crops.items():
        for aff in (None, A2 if naxis == 2 else A3):
            cs = _coordinates(disp, in_len, out_len, off, aff)
            hull = _lib.source_box(dgm._desc(dd), in_len, out_len, off, aff, flags, stream)
            for h in range(naxis):      # (the hull contains the exact box: test_source_box_kernel_vs_oracle_coordinates)
                assert hull[h, 0] <= np.floor(cs[h].min()) and hull[h, 1] >= np.ceil(cs[h].max())
            for order in range(6):
                first = [pref.tap_range(c, order) for c in cs]
                tmin = [int(f.min()) for f in first]
                tmax = [int(f.max()) + order for f in first]
                for mode in ("nearest", "wrap", "reflect", "mirror", "constant"):
                    for margin, align, minlen in SETTINGS:
                        win.fill_(-7)
                        st = _lib.source_window(dgm._desc(dd), in_len, out_len, off, aff, shape, axis, order,
                                                MODE_CODES[mode], margin, align, minlen, flags, stream, win.data_ptr())
                        assert st == 0
                        w = win.cpu().numpy().reshape(ndim, 2)
                        what = (name, cname, aff is not None, order, mode, margin, align, minlen, w.tolist())
                        for d in range(ndim):
                            assert 0 <= w[d, 0] < w[d, 1] <= shape[d], what
                            if d not in axis:
                                assert tuple(w[d]) == (0, shape[d]), what
                        for h, d in enumerate(axis):
                            n = shape[d]
                            w0, w1 = int(w[d, 0]), int(w[d, 1])
                            last = d == ndim - 1
                            # shape of the result
                            assert w1 - w0 >= min(minlen, n), what
                            if last:
                                assert w0 % align == 0 and (w1 % align == 0 or w1 == n), what
                            sticks_out = tmin[h] < 0 or tmax[h] > n - 1
                            if mode in CLIP or not sticks_out:
                                # superset of every tap, clipped to the axis, plus the margin
                                lo, hi = min(max(tmin[h], 0), n - 1), max(min(tmax[h], n - 1), 0)
                                assert w0 <= max(0, lo - margin) and w1 >= min(n, hi + 1 + margin), (what, h, lo, hi)
                            else:
                                assert (w0, w1) == (0, n), (what, h)
                            # not needlessly wide: the hull, taps, margin, alignment, 2 samples per side
                            hl = int(hull[h, 0]) - 2 - order // 2
                            hh = int(hull[h, 1]) + 2 + order - order // 2
                            hull_out = hl < 0 or hh > n - 1
                            slack = align - 1 if last else 0
                            # (a window grown to minlen, then aligned, is at most minlen + 2 * slack wide)
                            if w1 - w0 > minlen + 2 * slack and not (mode not in CLIP and hull_out):
                                lo_b = min(max(hl, 0), n - 1)
                                hi_b = max(min(hh, n - 1), 0)
                                if hl < 0:
                                    hi_b = max(hi_b, min(order, n - 1))
                                if hh > n - 1:
                                    lo_b = min(lo_b, max(n - 1 - order, 0))
                                assert w0 >= max(0, lo_b - margin - slack), (what, h, hull[h].tolist())
                                assert w1 <= min(n, hi_b + 1 + margin + slack), (what, h, hull[h].tolist())
                            # pinned
                            want = _expected_from_hull(hull[h, 0], hull[h, 1], n, order, mode, margin, align, minlen, last)
                            assert (w0, w1) == want, (what, h, hull[h].tolist(), want)
                            if minlen == 1 and align == 1:
                                key = ("clipped" if sticks_out else "free") if mode in CLIP else \
                                    ("folded" if sticks_out else "fold-free")
                                seen[key] += 1
                            elif w1 - w0 == minlen:
                                seen["minlen"] += 1
    # the cases cover every branch of the contract
    assert all(v > 0 for v in seen.values()), seen
