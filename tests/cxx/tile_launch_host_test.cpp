// Host-only check of the tile launcher's arithmetic (csrc/ed_tile_host.h): the scratch layout, how a control grid of a
// given width is served, the addressing limits and the strip lengths -- against the expressions the launcher used to
// carry in several copies, written out here literally (P_*).  No HIP call, no kernel: the header alone is included;
// link against libedhip.so for k1z_r_bytes and deform_tile_workspace_bytes.  Built and run by
// tests/test_tile_launch_host.py; the same program builds with -Xarch_host -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ed_tile_host.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
            return 1;                                                     \
        }                                                                 \
    } while (0)

using namespace ed;
using namespace ed::tile;

namespace {

GridGeom geom(int64_t i0, int64_t i1, int64_t i2, int64_t o0, int64_t o1, int64_t o2, int64_t c0, int64_t c1, int64_t c2)
{
    GridGeom g;
    memset(&g, 0, sizeof(g));
    g.naxis = 3;
    const int64_t in[3] = {i0, i1, i2}, out[3] = {o0, o1, o2}, ncp[3] = {c0, c1, c2};
    g.nvox = 1;
    for (int k = 0; k < 3; ++k) {
        g.in_len[k] = in[k];
        g.out_len[k] = out[k];
        g.ncp[k] = ncp[k];
        g.nvox *= out[k];
    }
    return g;
}
// a grid of ncp_x columns over in_x source and out_x output voxels along x (the other axes small)
GridGeom xgeom(int64_t ncp_x, int64_t in_x, int64_t out_x, int64_t o0 = 16, int64_t o1 = 16)
{
    return geom(16, 16, in_x, o0, o1, out_x, 4, 4, ncp_x);
}

// ---- the parent's expressions, literally ---------------------------------------------------------------------------
bool P_wide_grid(const GridGeom& g) { return kOffQ + 8 * (size_t)(kT * kT * 4) * (size_t)g.ncp[2] + 16 + 32768 > (size_t)64 * 1024; }
int P_window(const GridGeom& g)
{
    const double r = g.in_len[2] > 1 ? (double)(g.ncp[2] - 1) / (double)(g.in_len[2] - 1) : 0.0;
    return (int)std::floor(kWideStripTiles * kT * r) + 6;
}
int64_t P_strips(const GridGeom& g) { return (g.out_len[2] + kWideStripTiles * kT - 1) / (kWideStripTiles * kT); }
bool P_wide_optional(const GridGeom& g)
{
    if (P_wide_grid(g))
        return false;
    const int win = P_window(g);
    const int64_t strips = P_strips(g);
    if (win + 2 > g.ncp[2] || win > kWideMaxWin || strips > 256)
        return false;
    return 8.0 * (double)g.out_len[0] * (double)g.out_len[1] * 4.0 * (double)(strips * win) <= (double)((size_t)512 << 20);
}
size_t P_q_global_bytes(const GridGeom& g, bool wide_opt)
{
    size_t cols = (size_t)g.ncp[2];
    if (P_wide_grid(g) || (wide_opt && P_wide_optional(g))) {
        const size_t per_strip = (size_t)P_strips(g) * (size_t)P_window(g);
        cols = per_strip > cols ? per_strip : cols;
    }
    return 8 * (size_t)g.out_len[0] * (size_t)g.out_len[1] * 4 * cols;
}
size_t P_list_bytes(const GridGeom& g, int nb)
{
    int64_t ntiles = 1;
    for (int k = 0; k < 3; ++k)
        ntiles *= (g.out_len[k] + kT - 1) / kT;
    return (sizeof(int) * ((size_t)ntiles * nb + 1) + 63) & ~(size_t)63;
}
size_t P_xt_only_bytes(const GridGeom& g) { return (48 * (size_t)g.out_len[2] + 63) & ~(size_t)63; }
size_t P_xt_block_bytes(const GridGeom& g, int nb) { return P_xt_only_bytes(g) + (((size_t)nb * 32 + 63) & ~(size_t)63); }
size_t P_label_list_bytes(const GridGeom& g)
{
    const int64_t nvox = g.out_len[0] * g.out_len[1] * g.out_len[2];
    const int64_t cap = nvox < (1 << 20) ? nvox : (1 << 20);
    return (size_t)(cap + 32) * sizeof(int) + 64;
}
size_t P_workspace_bytes(const GridGeom& g, int nb, bool f64)
{
    const size_t q = P_q_global_bytes(g, f64 && nb == 1);
    if (q > ((size_t)512 << 20))
        return kWorkspaceGridBytes;
    return kWorkspaceGridBytes + 2 * P_list_bytes(g, nb) + P_xt_block_bytes(g, nb) + ((q * (size_t)nb + 63) & ~(size_t)63) +
           P_label_list_bytes(g);
}
// the wide-grid part of the parent's deform_tile_supported, with its Q-table bound
bool P_supported(const GridGeom& g, bool f32, int order, bool unit_x)
{
    if (P_wide_grid(g)) {
        if (order < 1)
            return false;
        const bool wave = f32 && order >= 4 && unit_x;
        if (!wave && (P_window(g) > kWideMaxWin || P_strips(g) > 256))
            return false;
    }
    return !(P_q_global_bytes(g, false) > ((size_t)512 << 20));
}
// the parent's launch_tile: 0 whole-grid tables, 1 per-strip, 2 plain tables on the one-wave kernels, 3 declined
int P_launch(const GridGeom& g, bool f32, int order, bool unit_x, int nb, bool* wide_opt_out)
{
    const bool wide_opt = !f32 && order >= 1 && nb == 1 && P_wide_optional(g);
    const bool wide = P_wide_grid(g) || wide_opt;
    const bool wide_wave = wide && f32 && order >= 4 && unit_x;
    *wide_opt_out = wide_opt;
    if (!wide)
        return 0;
    if (order < 1 || nb != 1)
        return 3;
    if (wide_wave)
        return 2;
    return P_window(g) > kWideMaxWin || P_strips(g) > 256 ? 3 : 1;
}
int kind_code(QTables k)
{
    return k == QTables::kWholeGrid ? 0 : k == QTables::kPerStrip ? 1 : k == QTables::kWavePlain ? 2 : 3;
}
// every question a caller can ask about g, against the parent
int same_as_parent(const GridGeom& g)
{
    CHECK(wide_grid(g) == P_wide_grid(g) && wide_window(g) == P_window(g) && wide_strips(g) == P_strips(g));
    CHECK(wide_optional(g) == P_wide_optional(g));
    CHECK(q_global_bytes(g, false) == P_q_global_bytes(g, false) && q_global_bytes(g, true) == P_q_global_bytes(g, true));
    for (int f32 = 0; f32 < 2; ++f32)
        for (int order = 0; order <= 5; ++order)
            for (int unit = 0; unit < 2; ++unit)
                for (int nb = 1; nb <= 3; nb += 2) {
                    bool p_opt = false;
                    const int p = P_launch(g, f32 != 0, order, unit != 0, nb, &p_opt);
                    const WideTables w = wide_tables(g, !f32, order, unit != 0, nb);
                    CHECK(kind_code(w.kind) == p && w.optional == p_opt);
                    CHECK(w.win == P_window(g) && w.strips == P_strips(g));
                    if (nb == 1)
                        CHECK((w.kind != QTables::kNone && q_global_bytes(g) <= kQTableMaxBytes) ==
                              P_supported(g, f32 != 0, order, unit != 0));
                }
    return 0;
}

int check_layout(const GridGeom& g)
{
    for (int nb = 1; nb <= 3; nb += 2)
        for (int allowed = 0; allowed < 2; ++allowed) {
            const TileScratch l = tile_scratch_layout(g, nb, allowed != 0);
            // the parent's carve, literally
            const size_t list_bytes = P_list_bytes(g, nb);
            const size_t q = P_q_global_bytes(g, allowed != 0);
            const size_t q_all = ((q * (size_t)nb) + 63) & ~(size_t)63;
            CHECK(l.list_a == 0 && l.list_b == list_bytes && l.xt == 2 * list_bytes);
            CHECK(l.slack == 2 * list_bytes + P_xt_only_bytes(g));
            CHECK(l.q == 2 * list_bytes + P_xt_block_bytes(g, nb) && l.q_stride == q);
            CHECK(l.label == 2 * list_bytes + P_xt_block_bytes(g, nb) + q_all);
            CHECK(l.total == 2 * list_bytes + P_xt_block_bytes(g, nb) + q_all + P_label_list_bytes(g));
            // aligned, in order, disjoint (each region holds what is kept there), ending at total
            const size_t off[7] = {l.list_a, l.list_b, l.xt, l.slack, l.q, l.label, l.total};
            int64_t ntiles = 1;
            for (int k = 0; k < 3; ++k)
                ntiles *= (g.out_len[k] + kT - 1) / kT;
            const size_t need[6] = {sizeof(int) * ((size_t)ntiles * nb + 1), sizeof(int) * ((size_t)ntiles * nb + 1),
                                    sizeof(AxTab) * (size_t)g.out_len[2], 32 * (size_t)nb, q * (size_t)nb,
                                    P_label_list_bytes(g)};
            for (int r = 0; r < 6; ++r) {
                CHECK(off[r] % 64 == 0);
                CHECK(off[r] + need[r] <= off[r + 1]);
            }
            CHECK(l.label + P_label_list_bytes(g) == l.total);
        }
    // the reservation edhip_deform makes up front: the parent's sum, and never less than what the launcher asks for,
    // whichever per_strip_allowed it passes for a call of this geometry
    for (int nb = 1; nb <= 3; nb += 2)
        for (int f64 = 0; f64 < 2; ++f64) {
            const size_t reserved = deform_tile_workspace_bytes(g, nb, f64 != 0);
            CHECK(reserved == P_workspace_bytes(g, nb, f64 != 0));
            for (int order = 0; order <= 5; ++order)
                for (int unit = 0; unit < 2; ++unit) {
                    const WideTables w = wide_tables(g, f64 != 0, order, unit != 0, nb);
                    if (w.kind == QTables::kNone)
                        continue;
                    CHECK(reserved >= kWorkspaceGridBytes + tile_scratch_layout(g, nb, w.optional).total);
                    CHECK(reserved >= kWorkspaceGridBytes + tile_scratch_layout(g, nb, false).total);     // (EDHIP_NO_WIDE64)
                }
        }
    return 0;
}

// the parent's three loops
int P_shorten(int start, int floor, int64_t enough, int64_t nb, int t0, int t1, int t2)
{
    int st = start;
    while (st > floor && (int64_t)nb * t0 * t1 * ((t2 + st - 1) / st) < enough)
        st >>= 1;
    return st;
}

}  // namespace

int main()
{
    // ---- thresholds, from the header's constants ---------------------------------------------------------------------
    int first_wide = 1;       // the first number of control columns whose 64 Q rows no longer fit next to a 32 KiB box
    while (!(kOffQ + 8 * (size_t)(kT * kT * 4) * (size_t)first_wide + 16 + 32768 > (size_t)64 * 1024))
        ++first_wide;
    CHECK(!wide_grid(xgeom(first_wide - 1, 256, 256)) && wide_grid(xgeom(first_wide, 256, 256)));
    const int64_t strip_vox = kWideStripTiles * kT;

    // ---- layout ----------------------------------------------------------------------------------------------------
    const int opt_cols = first_wide - 2;         // (a float64 volume's optional per-strip layout: window 7 of these columns)
    std::vector<GridGeom> table = {
        geom(40, 48, 70, 40, 48, 70, 4, 4, 5),                                   // whole-grid tables
        geom(64, 64, 256, 64, 64, 64, 5, 5, opt_cols),                           // wide-optional
        geom(64, 64, 256, 64, 64, 256, 5, 5, first_wide + 1),                    // wide
        geom(32, 32, 32, 1, 17, 33, 4, 4, 4),                                    // an output extent of 1
        geom(32, 32, 32, 1, 1, 1, 4, 4, 4),
        geom(64, 128, 128, 64, 128, 127, 4, 4, 6),                               // below 2^20 voxels
        geom(64, 128, 128, 64, 128, 128, 4, 4, 6),                               // 2^20: the label list's cap
        geom(64, 128, 128, 64, 128, 129, 4, 4, 6),                               // above
        geom(64, 128, 256, 64, 128, 129, 4, 4, opt_cols),                        // above, wide-optional
    };
    CHECK(wide_optional(table[1]) && !wide_grid(table[1]) && wide_grid(table[2]) && !wide_optional(table[0]));
    CHECK(label_list_bytes(table[5]) < label_list_bytes(table[6]) && label_list_bytes(table[6]) == label_list_bytes(table[7]));
    CHECK(label_list_bytes(table[6]) == ((size_t)(1 << 20) + 32) * sizeof(int) + 64);
    for (const GridGeom& g : table) {
        if (check_layout(g) || same_as_parent(g))
            return 1;
    }
    // (the optional layout is the larger one where it is taken: what "reserved >= used" rests on)
    CHECK(tile_scratch_layout(table[1], 1, true).total > tile_scratch_layout(table[1], 1, false).total);

    // ---- wide decision -----------------------------------------------------------------------------------------------
    const auto kind = [](const GridGeom& g, bool f64, int order, bool unit_x, int nb = 1) {
        return wide_tables(g, f64, order, unit_x, nb).kind;
    };
    {   // the column threshold
        const GridGeom below = xgeom(first_wide - 1, 256, 256), at = xgeom(first_wide, 256, 256);
        CHECK(kind(below, false, 3, true) == QTables::kWholeGrid && kind(at, false, 3, true) == QTables::kPerStrip);
        CHECK(kind(below, false, 0, true) == QTables::kWholeGrid && kind(at, false, 0, true) == QTables::kNone);
        CHECK(kind(at, false, 3, true, 3) == QTables::kNone && kind(at, false, 5, true, 3) == QTables::kNone);
        if (same_as_parent(below) || same_as_parent(at))
            return 1;
    }
    // window kWideMaxWin | + 1: 2 * strip_vox + 1 source voxels put half a column under a strip's voxel
    const int64_t in_w = 2 * strip_vox + 1;
    const GridGeom win_ok = xgeom(2 * (kWideMaxWin - 6) + 1, in_w, 64), win_over = xgeom(2 * (kWideMaxWin - 6) + 3, in_w, 64);
    {
        CHECK(wide_grid(win_ok) && wide_window(win_ok) == kWideMaxWin && wide_window(win_over) == kWideMaxWin + 1);
        CHECK(kind(win_ok, false, 3, true) == QTables::kPerStrip && kind(win_over, false, 3, true) == QTables::kNone);
        CHECK(kind(win_ok, true, 3, true) == QTables::kPerStrip && kind(win_over, true, 3, true) == QTables::kNone);
        if (same_as_parent(win_ok) || same_as_parent(win_over))
            return 1;
    }
    {   // strips kWideMaxStrips | + 1
        const GridGeom ok = xgeom(first_wide + 1, 8192, kWideMaxStrips * strip_vox), over = xgeom(first_wide + 1, 8192, kWideMaxStrips * strip_vox + 1);
        CHECK(wide_strips(ok) == kWideMaxStrips && wide_strips(over) == kWideMaxStrips + 1);
        CHECK(ok.out_len[2] == 8192 && over.out_len[2] == 8193);                // (with today's constants)
        CHECK(kind(ok, false, 2, false) == QTables::kPerStrip && kind(over, false, 2, false) == QTables::kNone);
        CHECK(kind(over, false, 4, true) == QTables::kWavePlain);
        if (same_as_parent(ok) || same_as_parent(over))
            return 1;
    }
    {   // the optional float64 layout: only where the window is narrower than the grid by two columns
        int cols = 2;
        while (wide_window(xgeom(cols, 256, 256)) + 2 > cols)
            ++cols;
        const GridGeom narrow = xgeom(cols - 1, 256, 256), enough = xgeom(cols, 256, 256);
        CHECK(cols < first_wide && wide_window(enough) + 2 == cols && wide_window(narrow) + 2 > cols - 1);
        CHECK(!wide_tables(narrow, true, 3, true, 1).optional && wide_tables(enough, true, 3, true, 1).optional);
        CHECK(kind(narrow, true, 3, true) == QTables::kWholeGrid && kind(enough, true, 3, true) == QTables::kPerStrip);
        CHECK(kind(enough, false, 3, true) == QTables::kWholeGrid);             // float32: whole-grid tables
        CHECK(kind(enough, true, 0, true) == QTables::kWholeGrid && kind(enough, true, 3, true, 3) == QTables::kWholeGrid);
        if (same_as_parent(narrow) || same_as_parent(enough))
            return 1;
        // ... and its 512 MiB bound: o_y rows of strips * win columns, 32 bytes each
        const int64_t per_row = 32 * wide_strips(enough) * wide_window(enough);
        const int64_t rows = (int64_t)(kQTableMaxBytes / (size_t)per_row);
        const GridGeom fits = xgeom(cols, 256, 256, 1, rows), beyond = xgeom(cols, 256, 256, 1, rows + 1);
        CHECK(wide_tables(fits, true, 3, true, 1).optional && !wide_tables(beyond, true, 3, true, 1).optional);
        CHECK(q_global_bytes(fits, true) <= kQTableMaxBytes && q_global_bytes(beyond, true) == q_global_bytes(beyond, false));
        if (same_as_parent(fits) || same_as_parent(beyond) || check_layout(fits) || check_layout(beyond))
            return 1;
    }
    {   // the 512 MiB bound of the whole-grid table, in the addressing limits both *_supported functions share
        const int64_t rows = (int64_t)(kQTableMaxBytes / (32 * 8)) / 2048;
        const GridGeom fits = geom(16, 16, 64, 2048, rows, 16, 4, 4, 8), beyond = geom(16, 16, 64, 2048, rows + 1, 16, 4, 4, 8);
        CHECK(q_global_bytes(fits) == kQTableMaxBytes && q_global_bytes(beyond) > kQTableMaxBytes);
        IOView v;
        memset(&v, 0, sizeof(v));
        for (int esz = 1; esz <= 8; esz *= 2) {
            for (const GridGeom* g : {&fits, &beyond}) {
                v.in_stride[2] = v.out_stride[2] = esz;
                v.in_stride[1] = g->in_len[2] * esz;
                v.in_stride[0] = g->in_len[1] * v.in_stride[1];
                v.out_stride[1] = g->out_len[2] * esz;
                v.out_stride[0] = g->out_len[1] * v.out_stride[1];
                CHECK(tile_addressable(*g, v, esz, esz < 4) == (g == &fits));
            }
            // a stride that is no multiple of the element: only where the caller asks
            v.in_stride[0] += 1;
            CHECK(tile_addressable(fits, v, esz, true) == (esz == 1));
        }
        // the tables kernel's grid in LDS: 3 * ncp_y * ncp_x doubles within 48 KiB
        v.in_stride[0] = 16 * 64;
        v.in_stride[1] = 64;
        v.in_stride[2] = v.out_stride[2] = 1;
        v.out_stride[1] = 16;
        v.out_stride[0] = 16 * 16;
        CHECK(tile_addressable(geom(16, 16, 64, 16, 16, 16, 4, 128, 16), v, 1, true));
        CHECK(!tile_addressable(geom(16, 16, 64, 16, 16, 16, 4, 128, 17), v, 1, true));
        CHECK(!tile_addressable(geom(16, 16, 64, 16, 16, 16, 1025, 4, 4), v, 1, true));
        if (same_as_parent(fits) || same_as_parent(beyond))
            return 1;
    }
    {   // orders 3 | 4, with and without unit stride along x: a window the per-strip layout holds, and one it does not
        CHECK(kind(win_ok, false, 3, true) == QTables::kPerStrip && kind(win_ok, false, 3, false) == QTables::kPerStrip);
        CHECK(kind(win_ok, false, 4, true) == QTables::kWavePlain && kind(win_ok, false, 4, false) == QTables::kPerStrip);
        CHECK(kind(win_over, false, 3, true) == QTables::kNone && kind(win_over, false, 3, false) == QTables::kNone);
        CHECK(kind(win_over, false, 4, true) == QTables::kWavePlain && kind(win_over, false, 4, false) == QTables::kNone);
        CHECK(kind(win_over, true, 4, true) == QTables::kNone && kind(win_ok, true, 4, true) == QTables::kPerStrip);
    }

    // ---- strips ------------------------------------------------------------------------------------------------------
    // 1024 workgroups (the x-strip kernels: forward from 4 down to 1, gradient from 8 down to 2)
    CHECK(shorten_strips(4, 1, 1024, 1, 1024, 4) == 4 && shorten_strips(4, 1, 1024, 1, 1023, 4) == 2);
    CHECK(shorten_strips(8, 2, 1024, 1, 1024, 8) == 8 && shorten_strips(8, 2, 1024, 1, 1023, 8) == 4);
    CHECK(shorten_strips(4, 1, 1024, 1, 1, 4) == 1 && shorten_strips(8, 2, 1024, 1, 1, 8) == 2);         // the floors
    CHECK(shorten_strips(4, 1, 1024, 1, 1, 1) == 1 && shorten_strips(8, 2, 1024, 1, 1, 1) == 2);
    // 8192 (the one-wave kernels)
    CHECK(shorten_strips(4, 1, 8192, 1, 8192, 4) == 4 && shorten_strips(4, 1, 8192, 1, 8191, 4) == 2);
    // batches enter the count
    CHECK(shorten_strips(4, 1, 1024, 3, 342, 4) == 4 && shorten_strips(4, 1, 1024, 1, 342, 4) == 1);
    CHECK(shorten_strips(4, 1, 1024, 3, 341, 4) == 2);
    CHECK(shorten_strips(4, 1, 8192, 2, 4096, 4) == 4 && shorten_strips(4, 1, 8192, 2, 4095, 4) == 2);
    for (int t0 = 1; t0 <= 40; t0 += 3)
        for (int t1 = 1; t1 <= 40; t1 += 7)
            for (int t2 = 1; t2 <= 33; ++t2)
                for (int nb = 1; nb <= 3; ++nb) {
                    const int64_t across = (int64_t)t0 * t1;
                    CHECK(shorten_strips(4, 1, 1024, nb, across, t2) == P_shorten(4, 1, 1024, nb, t0, t1, t2));
                    CHECK(shorten_strips(8, 2, 1024, nb, across, t2) == P_shorten(8, 2, 1024, nb, t0, t1, t2));
                    CHECK(shorten_strips(4, 1, 8192, nb, across, t2) == P_shorten(4, 1, 8192, nb, t0, t1, t2));
                    for (int st = 1; st <= 8; st <<= 1)
                        CHECK(strip_count(nb, across, t2, st) == (int64_t)nb * t0 * t1 * ((t2 + st - 1) / st));
                }
    // the z-walk's rule on the same counter: 256^3 keeps strips of 4 (8192 of them), 128^3 takes 2 (1024 -> 2048)
    CHECK(strip_count(1, 32 * 32, 32, 4) == 8192 && strip_count(1, 16 * 16, 16, 4) == 1024 && strip_count(1, 16 * 16, 16, 2) == 2048);

    // ---- the geometry buffer of the z-walk route (moved with the rest) -------------------------------------------------
    {
        const GridGeom g = geom(256, 256, 256, 256, 256, 256, 5, 5, 5);
        const K1zGeoLayout gl = k1z_geo_layout(g, 32 * 32 * 32, 1);
        CHECK(gl.r_stride == ((k1z_r_bytes(g) + 63) & ~(size_t)63) && gl.total == gl.r + gl.r_stride);
        CHECK(gl.zgen == 4096 && gl.recs % 64 == 0 && gl.steps % 64 == 0 && gl.recs_half + 32768 * 16 * sizeof(int) <= gl.steps);
    }
    std::printf("ok\n");
    return 0;
}
