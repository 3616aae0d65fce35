"""
Host tests of the case table of tests/test_fast_routes.py: from the NumPy restatement of the launch arithmetic
(tests/fast_cases.py) alone, every case is in the class it is listed for and every class has a case; and the
restatement's constants are the `constexpr` values of the source text, so that a change of kRows, kBoxCap2 or the tile
path's limits fails here and the table is looked at again.
"""
import os
import re

import numpy as np
import pytest

import fast_cases as fc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "elasticdeform_amd", "csrc")


def _case(id):
    c = fc.by_id(id)
    return c, c["deformed"], c["points"]


# ---- the row kernel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("id,rows,last,ne", [
    ("R1", 8, 3, 10), ("R2", 16, 8, 10), ("R3", 32, 5, 10), ("R4", 32, 32, 4), ("R5a", 32, 1, 768), ("R5b", 32, 1, 769),
    ("R6a", 8, 8, 768), ("R6b", 8, 8, 770), ("R7", 4, 3, 80), ("R8", 8, 8, 8), ("R9", 4, 4, 68), ("R10a", 4, 4, 24),
    ("R10b", 4, 4, 28), ("R11", 8, 8, 138), ("R12", 4, 4, 78), ("R13", 4, 4, 48), ("R14", 4, 4, 48)])
def test_rows_per_block_live_rows_and_nE(id, rows, last, ne):
    c, shape, points = _case(id)
    assert fc.rows_per_block(shape) == rows
    assert fc.last_block_rows(shape) == last
    assert fc.nE(len(shape), points[-1]) == ne


def test_lanes_of_the_last_x_block():
    assert fc.by_id("R1")["deformed"][-1] % 64 == 6                   # two x blocks, 6 live lanes in the last
    assert fc.by_id("R4")["deformed"][-1] == 3                        # one x block, 3 live lanes
    assert -(-fc.by_id("R6a")["points"][-1] * 2 // 64) == 12          # 12 passes of the lane loop over E


def _routes(id, dtype="float64"):
    c, shape, points = _case(id)
    return {(o, g): fc.route(shape, points, o, g, dtype=dtype, batch=c["batch"] or 1) for o in c["orders"]
            for g in (False, True)}


def test_routes_of_the_row_cases():
    # one and two axes: the row kernel forward, the gradient at order 0 (two axes) or every order (one axis)
    for id in ("R1", "R2", "R3", "R4", "R6a", "R7"):
        for (o, g), r in _routes(id).items():
            assert r == ("lds2" if g and o >= 1 else "row"), (id, o, g, r)
    assert set(_routes("R5a").values()) == {"row"}
    # the kMaxE boundary: 768 | 769 in 1-D, 384 | 385 in 2-D
    assert set(_routes("R5b").values()) == {"exact"} and set(_routes("R6b").values()) == {"exact"}
    assert fc.nE(1, 768) == fc.kMaxE == fc.nE(2, 384)
    # four axes: butterfly for nE <= 64, the rolled loop beyond; the LDS gradient for orders 2 / 3 up to kMaxE4
    assert _routes("R8") == {(0, False): "row", (0, True): "row", (1, False): "row", (1, True): "row",
                             (2, False): "row", (2, True): "lds4", (3, False): "row", (3, True): "lds4"}
    assert fc.nE(4, fc.by_id("R8")["points"][-1]) <= 64 < fc.nE(4, fc.by_id("R9")["points"][-1])
    r9 = _routes("R9")
    assert r9[(2, True)] == "row" and r9[(3, True)] == "exact" and all(r9[(o, False)] == "row" for o in range(4))
    assert r9[(0, True)] == r9[(1, True)] == "row"
    # both sides of kMaxE4
    assert 4 * fc.by_id("R10a")["points"][-1] == fc.kMaxE4 < 4 * fc.by_id("R10b")["points"][-1]
    assert _routes("R10a") == {(2, False): "row", (2, True): "lds4", (3, False): "row", (3, True): "lds4"}
    assert _routes("R10b") == {(2, False): "row", (2, True): "row", (3, False): "row", (3, True): "exact"}
    assert fc.route((9, 12, 10, 40), (3, 2, 3, 4), 4, False) == "exact"


def test_the_3d_cases_leave_the_tile_path_for_the_reason_they_name():
    for dtype in ("float64", "float32"):
        c, shape, points = _case("R11")
        assert 24 * points[1] * points[2] > fc.kTableBytes
        assert set(_routes("R11", dtype).values()) == {"row"}
        c, shape, points = _case("R12")
        assert fc.wide_grid(points) and fc.wide_window(points, shape) == 17 > fc.kWideMaxWin
        assert 24 * points[1] * points[2] <= fc.kTableBytes
        assert {fc.tile_declines(points, shape, o, dtype) for o in c["orders"]} == {"strip window beyond kWideMaxWin"}
        c, shape, points = _case("R13")
        assert fc.wide_grid(points) and fc.wide_window(points, shape) <= fc.kWideMaxWin
        assert fc.tile_declines(points, shape, 0, dtype) == "wide grid at order 0"
        assert fc.tile_declines(points, shape, 3, dtype) is None
        c, shape, points = _case("R14")
        assert fc.tile_declines(points, shape, 3, dtype, batch=1) is None
        assert fc.tile_declines(points, shape, 3, dtype, batch=c["batch"]) == "batch on a wide grid"
    # the narrow neighbours stay on the tile path
    assert not fc.wide_grid((3, 4, 14)) and fc.wide_grid((3, 4, 15))
    assert fc.route((40, 44, 70), (3, 4, 5), 3, True) == "tile"


def test_every_class_of_the_row_kernel_has_a_case():
    rows = {(len(c["deformed"]), fc.rows_per_block(c["deformed"])) for c in fc.ROW_CASES}
    assert {(2, 4), (2, 8), (2, 16), (2, 32), (4, 8), (4, 4), (3, 8), (3, 4), (1, 32)} <= rows
    partial = [c["id"] for c in fc.ROW_CASES if fc.last_block_rows(c["deformed"]) < fc.rows_per_block(c["deformed"])]
    assert {"R1", "R2", "R3"} <= set(partial)
    # a wave's second row (rows > kWaves) with a partial last block, in 2-D, 3-D and 4-D
    assert all(fc.rows_per_block(fc.by_id(i)["deformed"]) > fc.kWaves for i in ("R1", "R2", "R3", "R4", "R8", "R11"))
    passes = {len(c["deformed"]): 0 for c in fc.ROW_CASES}
    for c in fc.ROW_CASES:
        n = len(c["deformed"])
        if fc.nE(n, c["points"][-1]) <= fc.kMaxE:
            passes[n] = max(passes[n], -(-fc.nE(n, c["points"][-1]) // 64))
    assert passes[1] == 12 and passes[2] == 12 and passes[3] >= 2 and passes[4] == 2
    ids = {c["id"] for c in fc.ROW_CASES}
    assert len(ids) == len(fc.ROW_CASES) == 17
    assert all(set(c["dtypes"]) == {"float64", "float32"} for c in fc.ROW_CASES)


# ---- the 2-D LDS gradient ------------------------------------------------------------------------------------------------

def _counts(id, order):
    r = fc.g_geometry(id, order)[5]
    return r["fit"], r["nofit"], r["empty"], r["partly_dead"]


def test_block_counts_of_G1_to_G3():
    for order in range(1, 6):
        for id in ("G1", "G4", "G5", "G9"):
            assert _counts(id, order) == (65, 0, 0, 0)
        assert _counts("G7", order)[1:] == (0, 0, 0) and _counts("G8", order) == (9, 0, 0, 0)
    assert _counts("G2", 3) == (32, 13, 20, 30)
    assert _counts("G2p", 5) == (60, 5, 0, 0)
    assert _counts("G3", 3) == (55, 10, 0, 0)


@pytest.mark.parametrize("id", ["G2", "G2p", "G3"])
def test_mixed_cases_hold_both_states(id):
    for order in fc.by_id(id)["orders"]:
        fit, nofit, empty, partly = _counts(id, order)
        live = fit + nofit
        assert min(fit, nofit) >= 4 and min(fit, nofit) >= 0.05 * live, (order, fit, nofit)
        if id == "G2":
            assert empty >= 4 and partly >= 4, (order, empty, partly)
            # the `!any` early return next to live blocks
            assert live >= 4


def test_the_seams_of_G3_are_what_does_not_fit():
    D, in_shape, out_shape, off, K, r = fc.g_geometry("G3", 3)
    for b in r["blocks"]:
        if not b["fits"]:
            assert b["ext"][0] >= in_shape[0] - 20 or b["ext"][1] >= in_shape[1] - 20, b["ext"]


def test_the_marked_pixels_lie_in_fitting_blocks():
    for order in range(1, 6):
        r = fc.g_geometry("G4", order)[5]
        grid = {b["index"]: b for b in r["blocks"]}
        assert grid[(40 // 16, 50 // 64)]["fits"] and grid[(150 // 16, 200 // 64)]["fits"]
        y, x = fc.g_spike(order)
        assert grid[(y // 16, x // 64)]["fits"] and (y // 16, x // 64) == (6, 2)
        for id in ("G6a", "G6b", "G6c"):
            r = fc.g_geometry(id, order)[5]
            assert {b["index"]: b for b in r["blocks"]}[(90 // 16, 140 // 64)]["fits"]
            assert r["nofit"] >= 4                   # the step loop also runs in blocks without a box
    # G8: a block and one row, two blocks and one column
    assert fc.by_id("G8")["shape"] == (2 * fc.kRows2 + 1, 2 * 64 + 1)


def test_the_fixed_point_bound_counts_every_tap_once():
    D, in_shape, out_shape, off, K, r = fc.g_geometry("G9", 3)
    dY = np.ones(out_shape)
    bound, cover, mass = fc.fixed_point_bound(r, dY, 3, in_shape)
    assert sum(c.sum() for c in cover) == 16 * out_shape[0] * out_shape[1] == mass.sum()
    assert bound.max() > 0


# ---- the 4-D LDS gradient ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [2, 3])
def test_the_4d_cases(order):
    h1, h2 = fc.by_id("H1"), fc.by_id("H2")
    t = {}
    for case in (h1, h2):
        D = fc.grid(fc.H_POINTS, case["sigma"], fc.H_SEED)
        for cell in (4, 8):
            t[case["id"], cell] = fc.tiles4d(D, fc.H_SHAPE, fc.H_SHAPE, order, case["mode"], cell)
    assert 4 * fc.H_POINTS[-1] <= fc.kMaxE4 and fc.route(fc.H_SHAPE, fc.H_POINTS, order, True) == "lds4"
    # H1: the marked voxels lie in tiles that fit in both types
    for cell in (4, 8):
        tiles = {b["index"]: b for b in t["H1", cell]["blocks"]}
        assert tiles[(3 // 4, 4 // 4, 5 // 4, 6 // 4)]["fits"] and tiles[(7 // 4, 2 // 4, 8 // 4, 33 // 4)]["fits"]
    # H2: tiles that fit in float32 and not in float64, and both states well filled in float64
    a, b = t["H2", 4], t["H2", 8]
    only32 = sum(1 for x, y in zip(a["blocks"], b["blocks"]) if x["fits"] and not y["fits"])
    assert only32 >= 4
    live = b["fit"] + b["nofit"]
    assert min(b["fit"], b["nofit"]) >= 4 and min(b["fit"], b["nofit"]) >= 0.05 * live, (b["fit"], b["nofit"])
    assert min(a["fit"], a["nofit"]) >= 4
    # partial tiles on three axes of (9, 12, 10, 40)
    assert [s % 4 for s in fc.H_SHAPE] == [1, 0, 2, 0]


# ---- the source pin ------------------------------------------------------------------------------------------------------

def _int_expr(tokens, names):
    """value of an integer expression of literals, known names, + - * / << and parentheses (a small recursive-descent
    parser over a token list, consumed from the front); KeyError for a name that is not known"""
    def atom():
        t = tokens.pop(0)
        if t == "(":
            v = shift()
            assert tokens.pop(0) == ")"
            return v
        if t == "-":
            return -atom()
        return int(t) if t.isdigit() else names[t]

    def term():
        v = atom()
        while tokens and tokens[0] in "*/":
            op = tokens.pop(0)
            v = v * atom() if op == "*" else v // atom()
        return v

    def add():
        v = term()
        while tokens and tokens[0] in "+-":
            op = tokens.pop(0)
            v = v + term() if op == "+" else v - term()
        return v

    def shift():
        v = add()
        while tokens and tokens[0] == "<<":
            tokens.pop(0)
            v <<= add()
        return v

    v = shift()
    assert not tokens
    return v


def _constexpr(text, known=None):
    """every `constexpr int NAME = <integer arithmetic>;` of a source text, several names per statement included"""
    vals = dict(known or {})
    for stmt in re.findall(r"constexpr\s+int\s+([^;]+);", text):
        for name, expr in re.findall(r"(\w+)\s*=\s*([^,]+)", stmt):
            if re.fullmatch(r"[\w\s+\-*/()]+", expr):
                try:
                    vals[name] = _int_expr(re.findall(r"\w+|[-+*/()]", expr), vals)
                except KeyError:                   # (a name from elsewhere: not one of the pinned values)
                    pass
    return vals


def test_the_relayout_threshold_and_the_channels_last_case():
    # deform_grid.py permutes a channels-last input of RELAYOUT_MIN_ELEMENTS elements or more to step-axes-first before
    # any kernel sees it (orders >= 1): the channels-last case has to stay below that to reach the kernel as it is
    root = os.path.dirname(CSRC)
    text = open(os.path.join(root, "deform_grid.py")).read()
    m = re.search(r"^RELAYOUT_MIN_ELEMENTS\s*=\s*([\d\s<()*+-]+)$", text, re.M)
    assert m and _int_expr(re.findall(r"\d+|<<|[-+*()]", m.group(1)), {}) == fc.kRelayoutMinElements
    assert "int(numpy.prod(x.shape)) < RELAYOUT_MIN_ELEMENTS" in text
    case = fc.by_id("G6b")
    assert case["layout"] == "last"
    H, W = case["shape"]
    assert H * W * 3 < fc.kRelayoutMinElements           # in_stride[1] = 3 elements reaches the kernel
    assert H % fc.kRows2 and W % 64                      # partial blocks on both axes
    # G6a / G6c: the deformed axes are the trailing ones, no re-layout whatever the size
    assert fc.by_id("G6a")["layout"] == fc.by_id("G6c")["layout"] == "steps"
    assert fc.by_id("G6c").get("finite") and fc.by_id("G6c")["sigma"] == fc.by_id("G6a")["sigma"]


def test_the_constants_are_the_sources():
    fast = _constexpr(open(os.path.join(CSRC, "deform_fast.hip")).read())
    for name in ("kBlock", "kWaves", "kRows", "kMaxE", "kRows2", "kBoxCap2", "kT4A", "kT4B", "kT4C", "kT4X",
                 "kBoxBytes4", "kMaxE4"):
        assert fast[name] == getattr(fc, name), name
    tile_h = _constexpr(open(os.path.join(CSRC, "ed_tile.h")).read())
    assert tile_h["kT"] == fc.kT and tile_h["kOffQ"] == fc.kOffQ
    tile = open(os.path.join(CSRC, "ed_tile_host.h")).read()       # (the tile launcher's host arithmetic)
    wide = _constexpr(tile, tile_h)
    assert wide["kWideStripTiles"] == fc.kWideStripTiles and wide["kWideMaxWin"] == fc.kWideMaxWin
    assert "24 * (size_t)g.ncp[1] * (size_t)g.ncp[2] > 48 * 1024" in tile
    assert "kOffQ + q_bytes(g) + 16 + 32768 > (size_t)64 * 1024" in tile
    assert "8 * (size_t)(kT * kT * 4) * (size_t)g.ncp[2]" in tile
    # the largest weights of the fixed-point scale
    text = open(os.path.join(CSRC, "deform_fast.hip")).read()
    assert "ORDER == 1 ? 1.0 : ORDER == 2 ? 0.75 : ORDER == 3 ? 2.0 / 3.0" in text
    assert ": ORDER == 4 ? 115.0 / 192.0 : 0.55;" in text
    assert "4 * g.ncp[3] <= kMaxE4" in text and "4 * g.ncp[3] > 24" in text
    assert "xblocks * ((nrows + rows - 1) / rows) < 1024" in text
