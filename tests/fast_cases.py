"""
The case table of tests/test_fast_routes.py (GPU) and a NumPy restatement of the launch arithmetic of
elasticdeform_amd/csrc/deform_fast.hip; tests/test_fast_cases_host.py proves from the restatement alone that every
case is in the class it is listed for.  Not a test module.  Nothing is imported from the product: the constants below
are copies (the host file pins them to the source text), the coordinates come from oracle/dgrad_reference.py.

The three kernels and what decides their launch shape:

    row kernel (deform_fast_kernel)     rows per block 32 / 16 / 8 / 4 from the block count (`rows_per_block`),
                                        nE = naxis * ncp_x doubles of E per wave in lane passes of 64 (`nE`),
                                        the butterfly contraction for four axes with nE <= 64, a rolled loop beyond
    2-D gradient (deform_fast2_grad)    blocks of 16 x 64 pixels, a box of at most 6144 cells (`blocks2d`)
    4-D gradient (deform_fast4_grad)    tiles of 4^4 voxels, a box of 40 KiB: 10240 int32 or 5120 int64 cells
                                        (`tiles4d`), control grids of up to 6 points along x

`route` restates which of them (or the exact kernels, or the 3-D tile path) takes a call.
"""
import functools

import numpy as np

from oracle import dgrad_reference as ref

# ---- copies of the constants (pinned to the source by tests/test_fast_cases_host.py) ---------------------------------
kBlock = 256
kWaves = kBlock // 64
kRows = 32
kMaxE = 768
kRows2 = 16
kBoxCap2 = 6144
kT4A = kT4B = kT4C = kT4X = 4
kBoxBytes4 = 40 * 1024
kMaxE4 = 24
# the three direct conditions of deform_tile_supported (deform_tile.hip, ed_tile.h)
kT = 8
kOffQ = 3616
kWideStripTiles = 4
kWideMaxWin = 16
kTableBytes = 48 * 1024
# largest weight of a B-spline of orders 1-5 (the fixed-point scale of the LDS kernels)
kW1 = {1: 1.0, 2: 0.75, 3: 2.0 / 3.0, 4: 115.0 / 192.0, 5: 0.55}
kRange32 = 2.0 ** 31 - 2.0 ** 10
# deform_grid.py brings a channels-last input of this many elements or more to step-axes-first before the kernels see it
kRelayoutMinElements = 1 << 16

MODES = ("mirror", "constant", "wrap", "nearest", "reflect")


# ---- the launch arithmetic -------------------------------------------------------------------------------------------

def nE(naxis, ncp_x):
    return naxis * ncp_x


def rows_per_block(out_shape):
    """rows of the row kernel's block for an output of `out_shape` (deformed axes only)"""
    nrows = int(np.prod(out_shape[:-1], dtype=np.int64))
    xblocks = -(-out_shape[-1] // 64)
    rows = kRows
    while rows > kWaves and xblocks * (-(-nrows // rows)) < 1024:
        rows >>= 1
    return rows


def last_block_rows(out_shape):
    """live rows of the last row block"""
    nrows = int(np.prod(out_shape[:-1], dtype=np.int64))
    rows = rows_per_block(out_shape)
    return nrows - (-(-nrows // rows) - 1) * rows


def wide_grid(points):
    return kOffQ + 8 * (kT * kT * 4) * points[2] + 16 + 32768 > 64 * 1024


def wide_window(points, in_shape):
    r = (points[2] - 1) / (in_shape[2] - 1) if in_shape[2] > 1 else 0.0
    return int(np.floor(kWideStripTiles * kT * r)) + 6


def tile_declines(points, in_shape, order, dtype="float64", batch=1):
    """why the 3-D tile path leaves a call to the row kernel, or None (contiguous arrays; the three direct conditions of
    deform_tile_supported and launch_tile's refusal of a batch on a wide grid)"""
    if wide_grid(points):
        if order < 1:
            return "wide grid at order 0"
        wave = dtype == "float32" and order >= 4
        if not wave and wide_window(points, in_shape) > kWideMaxWin:
            return "strip window beyond kWideMaxWin"
    if 24 * points[1] * points[2] > kTableBytes:
        return "grid tables beyond 48 KiB"
    if wide_grid(points) and batch != 1:
        return "batch on a wide grid"
    return None


def route(out_shape, points, order, gradient, dtype="float64", batch=1, in_shape=None):
    """'row', 'lds2', 'lds4', 'exact' or 'tile': the kernel that takes a float call (launch_typed,
    deform_fast_supported, deform_tile_supported)"""
    n = len(out_shape)
    in_shape = out_shape if in_shape is None else in_shape
    if n < 1 or n > 4 or (n == 4 and order > 3):
        return "exact"
    if n == 4 and gradient and order == 3 and 4 * points[3] > kMaxE4:
        return "exact"
    if nE(n, points[-1]) > kMaxE:
        return "exact"
    if n == 3 and tile_declines(points, in_shape, order, dtype, batch) is None:
        return "tile"
    if n == 2 and order >= 1 and gradient:
        return "lds2"
    if n == 4 and 2 <= order <= 3 and gradient and 4 * points[3] <= kMaxE4:
        return "lds4"
    return "row"


# ---- the boxes of the LDS kernels ------------------------------------------------------------------------------------

def window_starts(D, in_shape, out_shape, order, mode, off=None, K=None):
    """(st, live): the first tap of every output voxel's window per axis, out_shape + (n,), unmapped tap-index space,
    and the voxels that scatter at all (dead: an axis outside under 'constant')"""
    n = len(out_shape)
    q = np.indices(out_shape).reshape(n, -1).T.astype(np.float64)
    c = ref.coordinate(q, D, in_shape, off, K)
    st = np.zeros(c.shape, dtype=np.int64)
    live = np.ones(c.shape[0], dtype=bool)
    for h in range(n):
        m, _, outside = ref.map_coordinate(c[:, h], in_shape[h], mode)
        if mode == "constant":
            live &= ~outside
        st[:, h] = (np.floor(m) if order & 1 else np.floor(m + 0.5)).astype(np.int64) - order // 2
    return st.reshape(tuple(out_shape) + (n,)), live.reshape(out_shape)


def _summary(blocks):
    return dict(blocks=blocks,
                fit=sum(1 for b in blocks if b["fits"]),
                nofit=sum(1 for b in blocks if b["live"] and not b["fits"]),
                empty=sum(1 for b in blocks if not b["live"]),
                partly_dead=sum(1 for b in blocks if 0 < b["live"] < b["voxels"]))


def _boxes(st, live, order, tile, fits):
    blocks = []
    shape = live.shape
    for idx in np.ndindex(*[-(-s // t) for s, t in zip(shape, tile)]):
        sl = tuple(slice(i * t, min((i + 1) * t, s)) for i, t, s in zip(idx, tile, shape))
        lv = live[sl]
        b = dict(index=idx, slices=sl, voxels=int(lv.size), live=int(lv.sum()), fits=False, lo=None, ext=None)
        if b["live"]:
            s = st[sl][lv]
            lo, hi = s.min(axis=0), s.max(axis=0) + order
            b["lo"], b["ext"] = tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1)
            b["fits"] = bool(fits(b["ext"]))
        blocks.append(b)
    return _summary(blocks)


def blocks2d(D, in_shape, out_shape, order, mode, off=None, K=None):
    """the box of every 16 x 64 block of deform_fast2_grad_kernel and the counts of fitting, non-fitting, empty and
    partly dead blocks"""
    st, live = window_starts(D, in_shape, out_shape, order, mode, off, K)
    res = _boxes(st, live, order, (kRows2, 64), lambda e: e[1] < 4096 and e[0] * (e[1] | 1) <= kBoxCap2)
    res["st"], res["live"] = st, live
    return res


def tiles4d(D, in_shape, out_shape, order, mode, cell_bytes, off=None, K=None):
    """the same for the 4^4 tiles of deform_fast4_grad_kernel; cell_bytes 4 (float32) or 8 (float64)"""
    st, live = window_starts(D, in_shape, out_shape, order, mode, off, K)
    cap = kBoxBytes4 // cell_bytes
    res = _boxes(st, live, order, (kT4A, kT4B, kT4C, kT4X),
                 lambda e: max(e) < 1024 and e[0] * e[1] * e[2] * (e[3] | 1) <= cap)
    res["st"], res["live"] = st, live
    return res


def fixed_point_bound(res, dY, order, in_shape):
    """(bound, cover, mass) per source cell of the 2-D LDS gradient without the transposed prefilter.
    bound: the fixed-point error in float32, the sum over the fitting blocks of N_b * 0.5 * unit_b with
    unit_b = kW1^2 * 1.001 * sum |dY|_block / (2^31 - 2^10) and N_b the number of the block's taps that land on the cell
    (every contribution is rounded to the nearest unit); cover[b] = N_b of block b (flat block order);
    mass: the sum of |dY| over all taps that land on the cell (each tap adds at most that times a weight <= 1)"""
    bound = np.zeros(in_shape)
    mass = np.zeros(in_shape)
    cover = []
    taps = np.arange(order + 1)
    for b in res["blocks"]:
        n_b = np.zeros(in_shape)
        if b["live"]:
            lv = res["live"][b["slices"]]
            s = res["st"][b["slices"]][lv]
            g = np.abs(dY[b["slices"]].astype(np.float64))
            ys = ref.mirror(s[:, 0, None] + taps[None, :], in_shape[0])[:, :, None]
            xs = ref.mirror(s[:, 1, None] + taps[None, :], in_shape[1])[:, None, :]
            np.add.at(n_b, (ys, xs), 1.0)
            np.add.at(mass, (ys, xs), g[lv][:, None, None])
            if b["fits"]:
                bound += n_b * 0.5 * (kW1[order] ** 2 * 1.001 * float(g.sum()) / kRange32)
        cover.append(n_b)
    return bound, cover, mass


# ---- the cases ---------------------------------------------------------------------------------------------------------

def grid(points, sigma=2.0, seed=0):
    return np.random.default_rng(seed).standard_normal((len(points),) + tuple(points)) * sigma


def _r(id, shape, points, why, orders=(0, 1, 2, 3, 4, 5), axis=None, seed=None, batch=0, dtypes=("float64", "float32")):
    deformed = tuple(shape) if axis is None else tuple(shape[a] for a in axis)
    return dict(id=id, shape=tuple(shape), deformed=deformed, points=tuple(points), why=why, orders=tuple(orders),
                axis=axis, sigma=2.0, seed=seed, batch=batch, dtypes=dtypes)


ROW_CASES = [
    _r("R1", (4099, 70), (3, 5), "rows 8, last block 3 rows, last x block 6 lanes"),
    _r("R2", (8200, 70), (3, 5), "rows 16, last block 8 rows"),
    _r("R3", (16389, 70), (3, 5), "rows 32, last block 5 rows", orders=(0, 3, 5)),
    _r("R4", (32768, 3), (3, 2), "rows 32, one x block, 3 live lanes"),
    _r("R5a", (200000,), (768,), "1-D, nE = kMaxE"),
    _r("R5b", (200000,), (769,), "1-D, nE = kMaxE + 1: the exact kernel"),
    _r("R6a", (600, 1100), (5, 384), "2-D, nE = 768: 12 lane passes, s_E full (also in the 2-D LDS gradient)"),
    _r("R6b", (600, 1100), (5, 385), "2-D, nE = 770: the exact kernel"),
    _r("R7", (3, 2051, 130), (3, 40), "2-D, nE = 80, a channel axis", axis=(1, 2)),
    _r("R8", (16, 16, 32, 5), (2, 3, 2, 2), "4-D, rows 8, butterfly contraction", orders=(0, 1, 2, 3)),
    _r("R9", (8, 8, 8, 70), (2, 2, 2, 17), "4-D, nE = 68: the rolled 64-tap contraction", orders=(0, 1, 2, 3)),
    _r("R10a", (9, 12, 10, 40), (3, 2, 3, 6), "4-D, 4 ncp_x = kMaxE4: the LDS gradient", orders=(2, 3)),
    _r("R10b", (9, 12, 10, 40), (3, 2, 3, 7), "4-D, beyond kMaxE4: row kernel at order 2, exact at order 3",
       orders=(2, 3)),
    _r("R11", (65, 64, 70), (3, 46, 46), "3-D direct (grid tables beyond 48 KiB), rows 8"),
    _r("R12", (40, 44, 70), (3, 4, 26), "3-D direct: strip window 17 > kWideMaxWin", orders=(1, 2, 3)),
    _r("R13", (40, 44, 70), (3, 4, 16), "3-D direct: wide grid at order 0", orders=(0,)),
    _r("R14", (40, 44, 70), (3, 4, 16), "3-D batch of 3 on a wide grid: the tile launcher declines", orders=(3,),
       batch=3),
]
for _i, _c in enumerate(ROW_CASES):
    if _c["seed"] is None:
        _c["seed"] = 100 + _i


def _g(id, why, sigma=25.0, mode="mirror", orders=(1, 2, 3, 4, 5), shape=(200, 300), points=(3, 3), **extra):
    return dict(id=id, why=why, sigma=sigma, mode=mode, orders=tuple(orders), shape=tuple(shape), points=tuple(points),
                seed=1, **extra)


G_CASES = [
    _g("G1", "every block fits (the README's geometry)"),
    _g("G2", "folding under constant: fitting, non-fitting, empty and partly dead blocks", sigma=150.0, mode="constant"),
    _g("G2p", "folding under nearest at order 5: a few blocks do not fit", sigma=60.0, mode="nearest", orders=(5,)),
    _g("G3", "wrap seams: the blocks on a seam do not fit", sigma=5.0, mode="wrap"),
    _g("G4", "one +inf and one NaN in dY, each in a fitting block", nonfinite=True),
    _g("G5", "dY zero except one pixel: gtot == 0 in every other block", single=True),
    _g("G6a", "two step axes (2, 3, H, W): the box re-zeroed per step; a zero channel and an inf", sigma=60.0,
       layout="steps"),
    _g("G6b", "channels last (100, 200, 3), 60000 elements: below the library's re-layout threshold, so the kernel itself "
       "sees in_stride[1] = 3; partial blocks, blocks without a box; a zero channel and an inf", sigma=150.0,
       shape=(100, 200), layout="last"),
    _g("G6c", "G6a with a finite dY (a zero channel): two step axes behind the transposed prefilter too", sigma=60.0,
       layout="steps", finite=True),
    _g("G7", "crop, rotate and zoom", crop=((7, 180), (13, 290)), rotate=20.0, zoom=1.3),
    _g("G8", "one row and one column beyond a block in each direction", shape=(33, 129), sigma=3.0),
    _g("G9", "dY of 1e-3 with one pixel at 1e6: the fixed-point resolution of the spike's block", spike=True,
       orders=(1, 2, 3, 4, 5)),
]

# four axes, LDS gradient: (9, 12, 10, 40), points (3, 2, 3, 4), seed 404.  H2's sigma was chosen with `tiles4d`: the
# first of 25, 20, 16, 12, 10, 8 at which tiles fit the 10240 int32 cells and not the 5120 int64 cells and both
# states hold at least 5 % of the tiles in float64 (the host file has the counts)
H_SHAPE, H_POINTS, H_SEED = (9, 12, 10, 40), (3, 2, 3, 4), 404
H_CASES = [
    dict(id="H1", why="one +inf and one NaN in dY", sigma=2.0, mode="mirror", orders=(2, 3), nonfinite=True),
    dict(id="H2", why="tiles whose box fits in float32 and not in float64", sigma=8.0, mode="mirror", orders=(2, 3)),
]


def by_id(id):
    return next(c for c in ROW_CASES + G_CASES + H_CASES if c["id"] == id)


def row_mode(case, order):
    """the boundary mode of a row-kernel case: every mode comes up over the orders"""
    return MODES[(order + ROW_CASES.index(case)) % len(MODES)]


def make_row(case, dtype, order):
    """(X, D, dY, kw) of a row-kernel case (with `batch` a leading axis on all three)"""
    rng = np.random.default_rng(case["seed"] + 1000)
    B = (case["batch"],) if case["batch"] else ()
    n = len(case["deformed"])
    X = rng.random(B + case["shape"]).astype(dtype)
    dY = rng.random(B + case["shape"]).astype(dtype)
    if case["batch"]:
        D = np.stack([grid(case["points"], case["sigma"], case["seed"] + b) for b in range(case["batch"])])
    else:
        D = grid(case["points"], case["sigma"], case["seed"])
    assert D.shape[len(B)] == n
    kw = dict(order=order, mode=row_mode(case, order), cval=0.5, prefilter=False)
    if case["axis"] is not None:
        kw["axis"] = case["axis"]
    return X, D, dY, kw


@functools.lru_cache(maxsize=None)
def g_geometry(id, order):
    """(D, in_shape, out_shape, off, K, blocks2d result) of a 2-D LDS case"""
    from oracle import ed_oracle as orc
    case = by_id(id)
    D = grid(case["points"], case["sigma"], case["seed"])
    in_shape = case["shape"]
    out_shape, off, K = in_shape, None, None
    if case.get("crop"):
        out_shape = tuple(b - a for a, b in case["crop"])
        off = [a for a, _ in case["crop"]]
    if case.get("rotate") is not None or case.get("zoom") is not None:
        K = orc._inverse_affine(None, case.get("rotate"), case.get("zoom"), 2, list(out_shape))
    return D, in_shape, out_shape, off, K, blocks2d(D, in_shape, out_shape, order, case["mode"], off, K)


def g_spike(order):
    """the pixel of G9's spike: the middle of block (6, 2), which fits at every order (host file)"""
    return (6 * kRows2 + 8, 2 * 64 + 32)


def make_g(case, dtype, order):
    """(dY, D, kw, X_shape) of a 2-D LDS case; dY has the output's shape"""
    rng = np.random.default_rng(2000 + order)
    D = grid(case["points"], case["sigma"], case["seed"])
    H, W = case["shape"]
    kw = dict(order=order, mode=case["mode"], cval=0.0)
    out = (H, W)
    if case.get("crop"):
        kw["crop"] = tuple(slice(a, b) for a, b in case["crop"])
        out = tuple(b - a for a, b in case["crop"])
    for k in ("rotate", "zoom"):
        if case.get(k) is not None:
            kw[k] = case[k]
    layout = case.get("layout")
    if layout == "steps":
        full, x_shape, kw["axis"] = (2, 3) + out, (2, 3, H, W), (2, 3)
    elif layout == "last":
        full, x_shape, kw["axis"] = out + (3,), (H, W, 3), (0, 1)
    else:
        full, x_shape = out, (H, W)
    dY = rng.random(full)
    if case.get("single"):
        dY[:] = 0.0
        dY[100, 170] = 0.75
    if case.get("spike"):
        dY = (dY + 0.5) * 1e-3
        dY[g_spike(order)] = 1e6
    dY = dY.astype(dtype)
    if case.get("nonfinite"):
        dY[40, 50] = np.inf                      # block (2, 0)
        dY[150, 200] = np.nan                    # block (9, 3)
    if layout == "steps":
        dY[0, 1] = 0.0
        if not case.get("finite"):
            dY[1, 2, 90, 140] = np.inf
    elif layout == "last":
        dY[:, :, 1] = 0.0
        dY[90, 140, 2] = np.inf
    return dY, D, kw, x_shape


def make_h(case, dtype, order):
    """(dY, D, kw) of a 4-D LDS case"""
    rng = np.random.default_rng(3000 + order)
    D = grid(H_POINTS, case["sigma"], H_SEED)
    dY = rng.random(H_SHAPE).astype(dtype)
    if case.get("nonfinite"):
        dY[3, 4, 5, 6] = np.inf
        dY[7, 2, 8, 33] = np.nan
    return dY, D, dict(order=order, mode=case["mode"], prefilter=False)
