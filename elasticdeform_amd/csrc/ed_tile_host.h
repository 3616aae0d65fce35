// ed_tile_host.h -- the host arithmetic of the tile launcher (deform_tile.hip), each fact stated once: the scratch
// layout, how a control grid of a given width is served, the addressing limits of the tile kernels and the strip
// lengths.  No HIP call and no kernel: tests/cxx/tile_launch_host_test.cpp checks it on the CPU.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "ed_params.h"
#include "ed_tile.h"

namespace ed {
namespace tile {

inline size_t pad64(size_t n) { return (n + 63) & ~(size_t)63; }

inline size_t q_bytes(const GridGeom& g) { return 8 * (size_t)(kT * kT * 4) * (size_t)g.ncp[2]; }
// near-tie list of the label kernel: up to 1M voxel ids (4 MiB), never more than the output has
inline size_t label_list_bytes(const GridGeom& g)
{
    int64_t nvox = 1;
    for (int k = 0; k < 3; ++k)
        nvox *= g.out_len[k];
    const int64_t cap = nvox < (1 << 20) ? nvox : (1 << 20);
    return (size_t)(cap + 32) * sizeof(int) + 64;
}

// ---- wide control grids ------------------------------------------------------------------------------------------
// the tile kernels keep a strip's 64 Q rows in LDS next to a 32 KiB box: up to this many control columns
inline bool wide_grid(const GridGeom& g) { return kOffQ + q_bytes(g) + 16 + 32768 > (size_t)64 * 1024; }
// wide grids: strips of kWideStripTiles tiles, the columns such a strip touches (conservative; <= kWideMaxWin or the
// row kernel of deform_fast.hip takes the call), at most kWideMaxStrips strips along x
constexpr int kWideStripTiles = 4;
constexpr int kWideMaxWin = 16;
constexpr int kWideMaxStrips = 256;
inline int wide_window(const GridGeom& g)
{
    const double r = g.in_len[2] > 1 ? (double)(g.ncp[2] - 1) / (double)(g.in_len[2] - 1) : 0.0;
    return (int)std::floor(kWideStripTiles * kT * r) + 6;
}
inline int64_t wide_strips(const GridGeom& g) { return (g.out_len[2] + kWideStripTiles * kT - 1) / (kWideStripTiles * kT); }

constexpr size_t kQTableMaxBytes = (size_t)512 << 20;       // the per-call Q table of one sample

// How the tile path serves a control grid of this width.  `win` and `strips` are the per-strip geometry of `g` whatever
// the answer (q_global_bytes sizes the table for it whenever the layout may be asked for).
enum class QTables {
    kWholeGrid,       // Q[o_z][o_y][ncp_x][4]: the strip's rows fit in LDS next to a box
    kPerStrip,        // Q[o_z][o_y][strip][win][4] (TileGeom::q_win): every kernel of the tile path reads it
    kWavePlain,       // whole-grid tables in global memory, read by the one-wave kernels of deform_wave.hip as they walk
    kNone,            // not by the tile path: the row kernel of deform_fast.hip (float) or the exact kernels take the call
};
struct WideTables {
    QTables kind = QTables::kWholeGrid;
    bool optional = false;      // kPerStrip by choice: the whole grid would fit
    int win = 0;
    int64_t strips = 0;
};
// f64: float64 volumes, otherwise float32 (integer volumes and label maps stay on whole-grid tables: wide_grid() alone
// decides for them); unit_x: unit stride along x on both sides.
//   wide grid      order 0 or a batch: none.  float32 orders 4 / 5 with unit_x: the one-wave kernels read their Q columns
//                  from global memory -- no LDS limit on the grid's width: plain tables, any window.  Otherwise per-strip
//                  tables, whose window and strip count have to fit.
//   narrower grid  whole-grid tables, but float64 volumes (round 5) take the per-strip layout also where the whole grid
//                  would still fit next to a box -- with 9 to 14 control columns the Q rows take 18-29 KB of LDS, the
//                  level-2 kernel is left with half a box of 8-byte cells and a rough deformation sends most tiles to the
//                  direct kernel (256^3, 13^3 grid, order 3 gradient: 8.0 ms, of which 6.8 in float64 global atomics;
//                  per-strip tables of 7 columns: see profiles/r05_bench_misc.txt).  Worth it when the window is
//                  narrower than the grid.
inline WideTables wide_tables(const GridGeom& g, bool f64, int order, bool unit_x, int nbatch)
{
    WideTables w;
    w.win = wide_window(g);
    w.strips = wide_strips(g);
    const bool fits = w.win <= kWideMaxWin && w.strips <= kWideMaxStrips;
    if (wide_grid(g)) {
        if (order < 1 || nbatch != 1)
            w.kind = QTables::kNone;
        else if (!f64 && order >= 4 && unit_x)
            w.kind = QTables::kWavePlain;
        else
            w.kind = fits ? QTables::kPerStrip : QTables::kNone;
    } else if (f64 && order >= 1 && nbatch == 1 && fits && w.win + 2 <= g.ncp[2] &&
               8.0 * (double)g.out_len[0] * (double)g.out_len[1] * 4.0 * (double)(w.strips * w.win) <= (double)kQTableMaxBytes) {
        w.kind = QTables::kPerStrip;
        w.optional = true;
    }
    return w;
}
// some float64 call of this geometry takes the per-strip layout although the whole grid would fit
inline bool wide_optional(const GridGeom& g) { return wide_tables(g, true, 1, false, 1).optional; }
// bytes of one sample's Q table; per_strip_allowed: the optional per-strip layout may be asked for (a wide grid is sized
// for it in any case, the one-wave kernels' plain tables included)
inline size_t q_global_bytes(const GridGeom& g, bool per_strip_allowed = false)
{
    size_t cols = (size_t)g.ncp[2];
    const WideTables w = wide_tables(g, per_strip_allowed, 1, false, 1);
    if (w.kind != QTables::kWholeGrid) {
        const size_t per_strip = (size_t)w.strips * (size_t)w.win;
        cols = per_strip > cols ? per_strip : cols;
    }
    return 8 * (size_t)g.out_len[0] * (size_t)g.out_len[1] * 4 * cols;
}

// ---- scratch -----------------------------------------------------------------------------------------------------
// The tile path's part of the stream's workspace, behind the kWorkspaceGridBytes of the control-grid head (byte offsets
// from there; every region 64-byte aligned):
//   spill list A | spill list B | x table | slack | Q of every sample | label list
// slack: the per-sample margins of K1's sampled boxes (TileGeom::slack), 32 bytes per sample.  The label list is there
// for every call so that the size does not depend on the element type.
struct TileScratch {
    size_t list_a, list_b, xt, slack, q, label;
    size_t q_stride;      // bytes between the Q tables of consecutive samples (q_global_bytes)
    size_t total;
};
inline size_t xt_only_bytes(const GridGeom& g) { return pad64(sizeof(AxTab) * (size_t)g.out_len[2]); }
inline TileScratch tile_scratch_layout(const GridGeom& g, int nbatch, bool per_strip_allowed)
{
    int64_t ntiles = 1;
    for (int k = 0; k < 3; ++k)
        ntiles *= (g.out_len[k] + kT - 1) / kT;
    const size_t list_bytes = pad64(sizeof(int) * ((size_t)ntiles * nbatch + 1));
    TileScratch l;
    l.list_a = 0;
    l.list_b = l.list_a + list_bytes;
    l.xt = l.list_b + list_bytes;
    l.slack = l.xt + xt_only_bytes(g);
    l.q = l.slack + pad64((size_t)nbatch * 32);
    l.q_stride = q_global_bytes(g, per_strip_allowed);
    l.label = l.q + pad64(l.q_stride * (size_t)nbatch);
    l.total = l.label + label_list_bytes(g);
    return l;
}

// The geometry buffer of the forward route of deform_k1z.hip (ed::GeoBuffer, its own allocation), size and layout:
//   counters (4 KiB, cleared at allocation) | ZGen (512) | z table | the per-tile arrays | step offsets | R per sample
// Per tile: its record (8 ints), a flag and a summary (1 + 1 per strip, at most one strip per tile), a slot in each of the
// two work lists dealt per XCD (entry k of XCD x at slot 8 k + x: 8 + 8 per strip, in case one XCD gets them all) and the
// records of its z halves (16).
constexpr size_t kK1zMaxSteps = 4096;
constexpr size_t kK1zRecInts = 8, kK1zMissedInts = 1, kK1zInfoInts = 1, kK1zListInts = 8, kK1zHalfInts = 16;
constexpr size_t kK1zTileBytes = sizeof(int) * (kK1zRecInts + kK1zMissedInts + kK1zInfoInts + 2 * kK1zListInts + kK1zHalfInts);
struct K1zGeoLayout {
    size_t zgen, zt, recs, missed, sinfo, list_g, list_f, recs_half, steps, r;   // byte offsets
    size_t r_stride;      // bytes between the R tables of consecutive samples
    size_t total;
};
inline K1zGeoLayout k1z_geo_layout(const GridGeom& g, int64_t ntiles, int nbatch)
{
    const size_t nt = (size_t)ntiles * (size_t)nbatch;
    K1zGeoLayout l;
    l.zgen = 4096;
    l.zt = l.zgen + 512;
    l.recs = l.zt + pad64(sizeof(AxTab) * (size_t)g.out_len[0]);
    l.missed = l.recs + nt * kK1zRecInts * sizeof(int);
    l.sinfo = l.missed + nt * kK1zMissedInts * sizeof(int);
    l.list_g = l.sinfo + nt * kK1zInfoInts * sizeof(int);
    l.list_f = l.list_g + nt * kK1zListInts * sizeof(int);
    l.recs_half = l.list_f + nt * kK1zListInts * sizeof(int);
    l.steps = l.recs + pad64(nt * kK1zTileBytes);
    l.r = l.steps + kK1zMaxSteps * 2 * sizeof(long long);
    l.r_stride = pad64(k1z_r_bytes(g));
    l.total = l.r + l.r_stride * (size_t)nbatch;
    return l;
}

// ---- addressing limits -------------------------------------------------------------------------------------------
// What every kernel that works from the per-call tables asks of a 3-axis call with elements of esz bytes: extents that
// leave tile and strip counts inside 30 bits, 32-bit element offsets inside a volume, the per-call Q table within
// 512 MiB; the tables kernel keeps 3 * ncp_y * ncp_x doubles in LDS.  need_divisible: the strides are not known to be
// multiples of esz (label maps of any dtype) and have to be.
inline bool tile_addressable(const GridGeom& g, const IOView& v, int64_t esz, bool need_divisible)
{
    int64_t in_span = 0, out_span = 0;
    for (int k = 0; k < 3; ++k) {
        if (g.in_len[k] >= 0x3fffffff || g.out_len[k] >= 0x3fffffff || g.ncp[k] > 1024)
            return false;
        if (need_divisible && (v.in_stride[k] % esz || v.out_stride[k] % esz))
            return false;
        const int64_t si = v.in_stride[k] / esz, so = v.out_stride[k] / esz;
        in_span += (si < 0 ? -si : si) * (g.in_len[k] - 1);
        out_span += (so < 0 ? -so : so) * (g.out_len[k] - 1);
    }
    for (int l = 0; need_divisible && l < v.nstep; ++l)
        if (v.in_step_stride[l] % esz || v.out_step_stride[l] % esz)
            return false;
    if (in_span >= 0x7fffffffLL || out_span >= 0x7fffffffLL)
        return false;
    return q_global_bytes(g) <= kQTableMaxBytes && !(24 * (size_t)g.ncp[1] * (size_t)g.ncp[2] > 48 * 1024);
}

// ---- strips ------------------------------------------------------------------------------------------------------
// strips of `st` tiles along one axis of `along` tiles, `across` tiles in the plane of the other two, nb samples
inline int64_t strip_count(int64_t nb, int64_t across, int along, int st) { return nb * across * ((along + st - 1) / st); }
// Strips of `start` tiles amortise a workgroup's prologue; small outputs (crops) take shorter ones, halved down to
// `floor`, until the launch has `enough` workgroups.
inline int shorten_strips(int start, int floor, int64_t enough, int64_t nb, int64_t across, int along)
{
    int st = start;
    while (st > floor && strip_count(nb, across, along, st) < enough)
        st >>= 1;
    return st;
}

}  // namespace tile
}  // namespace ed
