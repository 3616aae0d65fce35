// ed_tile.h -- definitions shared by the LDS-tiled deform kernels: deform_tile.hip (general tile
// kernels, tables, spill levels, label kernel) and the float32 level-1 kernels (deform_hot.hip, deform_k1.hip,
// deform_k1z.hip, deform_wave.hip): argument blocks, the coordinate arithmetic, strips, the wave-level box reduction.
#pragma once

#include "ed_device.h"
#include "ed_params.h"
#include "ed_workspace.h"

namespace ed {
namespace tile {

constexpr int kT = 8;                 // tile edge
constexpr int kStrip = 8;             // tiles per strip (along x)
constexpr int kBlock = 256;

struct AxTab {
    double w[4];
    int idx[4];
};

// 16 bytes at 4-byte alignment: compiles to one global_load_dwordx4 (unaligned access is on)
struct __attribute__((packed, aligned(4))) F4u {
    float x, y, z, w;
};
static_assert(sizeof(AxTab) == 48, "AxTab layout");

// Compiler fence between two LDS reads: stops the backend's load/store optimizer from fusing
// neighbouring ds_read_b64 into ds_read2_b64.  Emits no instruction; s_waitcnt insertion is unaffected.
#define ED_NO_DS_MERGE() asm volatile("" ::: "memory")

// LDS carve (bytes)
constexpr int kOffTabX = 0;                               // [kStrip][8] AxTab
constexpr int kOffRed = kOffTabX + kStrip * kT * 48;      // int[3][8]: lo[3], hi[3], -, - (triple-buffered)
constexpr int kOffSum = kOffRed + 96;                     // float[2][4]: per-wave sum |dY| (K2)
constexpr int kOffHot = kOffSum + 32;                     // HotParams (uniform values kept out of SGPRs)
constexpr int kOffQ = kOffHot + 416;
static_assert(kOffQ % 16 == 0, "LDS carve alignment");

// Uniform per-call values the per-voxel code needs.  Kept in LDS and fetched with broadcast reads:
// as kernel arguments they would be hoisted into ~100 scalar registers, live across the whole tile
// loop, and the spill reloads (v_readlane) were a third of the kernel's VALU work.
struct HotParams {
    double offd[3];        // crop offset per axis
    double last[3];        // I_k - 1
    double period[3];      // boundary-map period for the input's mode, and its reciprocal
    double inv_period[3];
    double affine[12];     // inverse map, 3 x 4
    long long step_len[8];
    long long in_step_stride[8];
    long long out_step_stride[8];
    int nstep;
    int pad_;
    double slack[3];       // K1: margin of the sampled tile boxes (HotGeom::slack), per axis
};
static_assert(sizeof(HotParams) <= 416, "HotParams must fit its LDS slot");

__device__ __forceinline__ int mirror_i32(int idx, int len)
{
    if ((unsigned)idx < (unsigned)len)
        return idx;                       // in range: the common case
    if (len <= 1)
        return 0;
    if (idx < 0 && idx > -len)
        return -idx;                      // one reflection at the low end
    if (idx >= len && idx <= 2 * len - 2)
        return 2 * len - 2 - idx;         // one reflection at the high end
    const int period = 2 * len - 2;
    if (idx < 0) {
        idx = period * (-idx / period) + idx;
        idx = idx <= 1 - len ? idx + period : -idx;
    } else {
        idx -= period * (idx / period);
        if (idx >= len)
            idx = period - idx;
    }
    return idx;
}

// Wave-wide min / max / sum without touching LDS: four DPP steps fold each row of 16 lanes
// (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror), then the four row
// results meet in scalar registers.  All 64 lanes must be active.
#define ED_DPP_STEP(v, ctrl) __builtin_amdgcn_update_dpp((v), (v), (ctrl), 0xf, 0xf, false)
__device__ __forceinline__ int wave_min(int v)
{
    v = min(v, ED_DPP_STEP(v, 0xB1));
    v = min(v, ED_DPP_STEP(v, 0x4E));
    v = min(v, ED_DPP_STEP(v, 0x141));
    v = min(v, ED_DPP_STEP(v, 0x140));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int wave_max(int v)
{
    v = max(v, ED_DPP_STEP(v, 0xB1));
    v = max(v, ED_DPP_STEP(v, 0x4E));
    v = max(v, ED_DPP_STEP(v, 0x141));
    v = max(v, ED_DPP_STEP(v, 0x140));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ float wave_sum(float f)
{
    f += __int_as_float(ED_DPP_STEP(__float_as_int(f), 0xB1));
    f += __int_as_float(ED_DPP_STEP(__float_as_int(f), 0x4E));
    f += __int_as_float(ED_DPP_STEP(__float_as_int(f), 0x141));
    f += __int_as_float(ED_DPP_STEP(__float_as_int(f), 0x140));
    const int v = __float_as_int(f);
    return (__int_as_float(__builtin_amdgcn_readlane(v, 0)) +
            __int_as_float(__builtin_amdgcn_readlane(v, 16))) +
           (__int_as_float(__builtin_amdgcn_readlane(v, 32)) +
            __int_as_float(__builtin_amdgcn_readlane(v, 48)));
}

// Boundary map of a real coordinate for the fast kernels: the same piecewise map as deform.c:47-128
// (legacy SciPy semantics, same branch structure) with the trunc-divisions `(npy_intp)(c / period)`
// replaced by floor(c * (1 / period)) -- equal as real functions (every argument is positive
// there), different only in the last ulp of the product, which the fast path does not promise.
__device__ __forceinline__ double map_coordinate_fast(double c, int len, int mode, double period,
                                                      double inv_period)
{
    const double last = (double)(len - 1);
    if (c < 0) {
        switch (mode) {
        case EDHIP_MODE_MIRROR:
            if (len <= 1) {
                c = 0;
            } else {
                c = period * floor(-c * inv_period) + c;
                c = c <= -last ? c + period : -c;
            }
            break;
        case EDHIP_MODE_REFLECT:
            if (len <= 1) {
                c = 0;
            } else {
                if (c < -period)
                    c = period * floor(-c * inv_period) + c;
                c = c < (double)(-len) ? c + period : -c - 1;
            }
            break;
        case EDHIP_MODE_WRAP:
            if (len <= 1)
                c = 0;
            else
                c += period * (floor(-c * inv_period) + 1);
            break;
        case EDHIP_MODE_NEAREST: c = 0; break;
        default: c = -1; break;   // constant
        }
    } else if (c > last) {
        switch (mode) {
        case EDHIP_MODE_MIRROR:
            if (len <= 1) {
                c = 0;
            } else {
                c -= period * floor(c * inv_period);
                if (c >= (double)len)
                    c = period - c;
            }
            break;
        case EDHIP_MODE_REFLECT:
            if (len <= 1) {
                c = 0;
            } else {
                c -= period * floor(c * inv_period);
                if (c >= (double)len)
                    c = period - c - 1;
            }
            break;
        case EDHIP_MODE_WRAP:
            if (len <= 1)
                c = 0;
            else
                c -= period * floor(c * inv_period);
            break;
        case EDHIP_MODE_NEAREST: c = last; break;
        default: c = -1; break;   // constant
        }
    }
    return c;
}

// B-spline basis weights from the fractional offset, in the data's own width.  Same closed forms
// as deform.c:160-268 (last weight = 1 - sum of the others) with the divisions folded into
// constants.  x is c - floor(c) (odd orders) or c - floor(c + 0.5) (even orders).
// Every product-sum is written out as the fused multiply-add it is meant to be and the compiler's own
// contraction is switched off: the function is inlined into a dozen kernels, and left to itself the
// backend fused `0.75 - x * x` in some of them and not in others -- a voxel then got weights an ulp
// apart depending on the level that served its tile (order 2: 6 % of the voxels).
__device__ __forceinline__ float wt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double wt_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T, int ORDER>
__device__ __forceinline__ void weights_from_frac(T x, T* w)
{
#pragma clang fp contract(off)
    const T z = (T)1 - x;
    if (ORDER == 0) {
        w[0] = (T)1;
        return;
    }
    if (ORDER == 1) {
        w[0] = z;
    } else if (ORDER == 2) {
        w[1] = wt_fma(-x, x, (T)0.75);
        const T y = (T)0.5 - x;
        w[0] = ((T)0.5 * y) * y;
    } else if (ORDER == 3) {
        // all four cubic pieces in closed form (cheaper than "last = 1 - sum"; same polynomials)
        const T x2 = x * x, z2 = z * z;
        w[0] = (z2 * z) * (T)(1.0 / 6.0);
        w[3] = (x2 * x) * (T)(1.0 / 6.0);
        w[1] = wt_fma(x2, wt_fma(x, (T)0.5, (T)-1), (T)(2.0 / 3.0));
        w[2] = wt_fma(z2, wt_fma(z, (T)0.5, (T)-1), (T)(2.0 / 3.0));
        return;
    } else if (ORDER == 4) {
        T t = x * x;
        w[2] = wt_fma(t, wt_fma(t, (T)0.25, (T)-0.625), (T)(115.0 / 192.0));
        T y = (T)1 + x;
        w[1] = wt_fma(y, wt_fma(y, wt_fma(y * ((T)5 - y), (T)(1.0 / 6.0), (T)-1.25), (T)(5.0 / 24.0)), (T)(55.0 / 96.0));
        w[3] = wt_fma(z, wt_fma(z, wt_fma(z * ((T)5 - z), (T)(1.0 / 6.0), (T)-1.25), (T)(5.0 / 24.0)), (T)(55.0 / 96.0));
        y = (T)0.5 - x;
        t = y * y;
        w[0] = (t * t) * (T)(1.0 / 24.0);
    } else {
        T t = x * x;
        w[2] = wt_fma(t, wt_fma(t, wt_fma(-x, (T)(1.0 / 12.0), (T)0.25), (T)-0.5), (T)0.55);
        t = z * z;
        w[3] = wt_fma(t, wt_fma(t, wt_fma(-z, (T)(1.0 / 12.0), (T)0.25), (T)-0.5), (T)0.55);
        T y = x + (T)1;
        w[1] = wt_fma(y, wt_fma(y, wt_fma(y, wt_fma(y, wt_fma(y, (T)(1.0 / 24.0), (T)-0.375), (T)1.25), (T)-1.75), (T)0.625),
                      (T)0.425);
        const T zz = z + (T)1;
        w[4] = wt_fma(zz, wt_fma(zz, wt_fma(zz, wt_fma(zz, wt_fma(zz, (T)(1.0 / 24.0), (T)-0.375), (T)1.25), (T)-1.75), (T)0.625),
                      (T)0.425);
        y = (T)1 - x;
        t = y * y;
        w[0] = ((y * t) * t) * (T)(1.0 / 120.0);
    }
    T last = (T)1;
#pragma unroll
    for (int i = 0; i < ORDER; ++i)
        last -= w[i];
    w[ORDER] = last;
}

// ---- one axis of the source coordinate (deform.c:771-788) on the fast path -------------------------
// Every tile kernel (hot, general, direct) splits a coordinate into window start + fraction with
// these three functions, so a voxel gets bit-identical (start, frac) whichever kernel serves its
// tile -- the crop identity full[crop] == cropped (README.md:113) holds bit for bit across the spill
// levels.  Without an affine map the integer part (output index + crop offset, `b`) never meets the
// fp64 sum: floor(b + d) = b + floor(d).  Return value: the window start needs no boundary map
// (odd orders 0 <= floor(c) <= I-2; even orders 1 <= floor(c + 0.5) <= I-2).
template <int ORDER, typename T>
__device__ __forceinline__ bool coord_axis_fast(double d, int b, int in_len, int& ci, T& frac)
{
    const double fl = floor((ORDER & 1) ? d : d + 0.5);
    ci = (int)fl + b;
    frac = (T)(d - fl);
    const int lo = (ORDER & 1) ? 0 : 1;
    const int span = (ORDER & 1) ? in_len - 1 : in_len - 2;
    return (unsigned)(ci - lo) < (unsigned)max(span, 0);
}
// out-of-range axis: boundary map of the full coordinate c (deform.c:47-128, 782); returns true when
// the voxel maps to the constant
template <int ORDER, typename T>
__device__ __forceinline__ bool coord_axis_mapped(double c, int in_len, int mode, double period,
                                                  double inv_period, int& ci, T& frac)
{
    const double cc = map_coordinate_fast(c, in_len, mode, period, inv_period);
    const double fl = floor((ORDER & 1) ? cc : cc + 0.5);
    ci = (int)fl;
    frac = (T)(cc - fl);
    return !(cc > -1.0);
}
// General coordinates of one voxel (deform.c:771-824), the tail every level-1 kernel ends its displacement
// with: window start and fractions, with the boundary map for the axes along which the source point left the
// array.  `d` = the displacement, `b[h]` = output index + crop offset along axis h (no affine) or 0 (affine:
// the real base is in `P`).  in_len / mode / period / inv_period: pointers into whatever the kernel keeps them
// in (kernel arguments, LDS, constant memory), read where a branch needs them.  raw_start: the window start before range test and boundary map, which
// the fast tiles of the sampled-box kernels work with.  Returns true when the voxel maps to the constant.
template <int ORDER, bool AFFINE, typename T, typename IntP, typename DblP>
__device__ __forceinline__ bool tile_coords(IntP in_len, IntP mode, DblP period, DblP inv_period, const double (&d)[3],
                                            const int (&b)[3], const double (&P)[3], int* start, T* frac,
                                            int* raw_start = nullptr)
{
    int ci[3];
    bool inr[3];
#pragma unroll
    for (int h = 0; h < 3; ++h)
        inr[h] = coord_axis_fast<ORDER, T>(AFFINE ? P[h] + d[h] : d[h], AFFINE ? 0 : b[h], in_len[h], ci[h], frac[h]);
    if (raw_start) {
#pragma unroll
        for (int h = 0; h < 3; ++h)
            raw_start[h] = ci[h] - ORDER / 2;
    }
    bool cst = false;
    if (!(inr[0] && inr[1] && inr[2])) {
        // one divergent region: the axes along which the source point left the array
#pragma unroll
        for (int h = 0; h < 3; ++h) {
            if (!inr[h])
                cst = coord_axis_mapped<ORDER, T>(AFFINE ? P[h] + d[h] : (double)b[h] + d[h], in_len[h], *mode, period[h],
                                                  inv_period[h], ci[h], frac[h]) || cst;
        }
    }
#pragma unroll
    for (int h = 0; h < 3; ++h)
        start[h] = cst ? 0 : ci[h] - ORDER / 2;
    return cst;
}

// Displacement of one voxel (deform.c:693-758 after the contraction over z and y) from a row of Q laid out
// [control column][component padded to 4]: `off` = byte offsets of the four control columns, `w` = the cubic
// weights along x; ds_read_b128 (components 0, 1) + ds_read_b64 (2) per column.  ROFF: immediate byte offset.
template <int ROFF = 0>
__device__ __forceinline__ void qrow_disp(const char* qrow, const int (&off)[4], const double (&w)[4], double (&d)[3])
{
    double2 q01[4];
    double q2[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        q01[l] = *reinterpret_cast<const double2*>(qrow + off[l] + ROFF);
        q2[l] = *reinterpret_cast<const double*>(qrow + off[l] + ROFF + 16);
    }
    d[0] = w[0] * q01[0].x;
    d[1] = w[0] * q01[0].y;
    d[2] = w[0] * q2[0];
#pragma unroll
    for (int l = 1; l < 4; ++l) {
        d[0] = fma(w[l], q01[l].x, d[0]);
        d[1] = fma(w[l], q01[l].y, d[1]);
        d[2] = fma(w[l], q2[l], d[2]);
    }
}

// Bounding box of a wave's tap windows: min of lo[3], max of hi[3] with DPP only -- four row steps
// (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror) leave every lane with the result of
// its row of 16 (STEPS 4); row_bcast:15 / row_bcast:31 then carry the row results upwards so that lane 63
// holds the wave's (STEPS 6).  Hand-written: the compiler turns every __builtin_amdgcn_update_dpp step into
// copy + s_nop + v_mov_dpp + v_min (4 instructions instead of 1) and wraps single-lane atomics behind it in a
// wave-reduction loop -- together ~200 instructions per wave and tile, a quarter of K2's VALU work.  The six
// chains are interleaved, which also covers the DPP read-after-write hazard (2 wait states) without s_nop.
// All 64 lanes must be active.
#define ED_RED6(CTRL)                                      \
    "v_min_i32_dpp %0, %0, %0 " CTRL "\n\t"                \
    "v_min_i32_dpp %1, %1, %1 " CTRL "\n\t"                \
    "v_min_i32_dpp %2, %2, %2 " CTRL "\n\t"                \
    "v_max_i32_dpp %3, %3, %3 " CTRL "\n\t"                \
    "v_max_i32_dpp %4, %4, %4 " CTRL "\n\t"                \
    "v_max_i32_dpp %5, %5, %5 " CTRL "\n\t"
#define ED_RED6_ROWS                                                  \
    "s_nop 1\n\t"                                                     \
    ED_RED6("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")         \
    ED_RED6("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")         \
    ED_RED6("row_half_mirror row_mask:0xf bank_mask:0xf")             \
    ED_RED6("row_mirror row_mask:0xf bank_mask:0xf")
template <int STEPS>
__device__ __forceinline__ void box_reduce(int (&lo)[3], int (&hi)[3])
{
    static_assert(STEPS == 4 || STEPS == 6, "rows of 16 lanes, or the wave to lane 63");
    if constexpr (STEPS == 4)
        asm volatile(ED_RED6_ROWS
                     : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]));
    else
        asm volatile(ED_RED6_ROWS
                     ED_RED6("row_bcast:15 row_mask:0xa bank_mask:0xf")
                     ED_RED6("row_bcast:31 row_mask:0xc bank_mask:0xf")
                     : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]));
}
#undef ED_RED6_ROWS
#undef ED_RED6

struct TileGeom {
    int in_len[3];        // I_k (the tile kernels require extents < 2^30)
    int out_len[3];
    int tiles[3];         // number of tiles per axis
    int strips_x;         // strips per tile row
    int strip_tiles;      // tiles per strip (8, or 4 / 2 for small outputs)
    int nstrips;
    int ncpx;             // control points along x = stride of one component row of Q
    // Wide control grids (more columns than the 64 Q rows of a strip can hold in LDS next to a box): the tables
    // kernel writes Q per x-STRIP -- only the q_win columns a strip of q_strip_vox voxels touches, starting at
    // the strip's lowest column -- as Q[o_z][o_y][strip][q_win][4], and the x-table's column indices relative to
    // that start.  The level-1 kernels of deform_hot.hip then see a grid of q_win columns; nobody else reads the
    // tables of such a call (launch_tile runs it in self-serve form).  q_win == 0: the plain layout.
    int q_win, q_strip_vox, q_strips;
    int box_cap;          // elements per LDS copy
    int off_ov;           // LDS byte offset of the overlay region (box | D, P)
    int in_stride[3];     // element strides (the tile kernels require < 2^31 elements per volume)
    int out_stride[3];
    int mode;             // boundary mode of this input
    int has_affine;
    int off[3];           // crop offsets
    double period[3];     // boundary-map period of each axis for `mode`, and its reciprocal
    double inv_period[3];
    double affine[12];    // inverse map, 3 x 4
    int* spill;           // [0] = count, [1..] = tile ids that did not fit in LDS
    int* spill_next;      // the second level's spill list (its count is reset by the tables kernel)
    // level-1 spill feedback (ed_workspace.h, SpillHint): hint[0] = tiles of this call whose box does not fit
    // the standard level-1 box, hint[1] = this call's sequence number; the tables kernel of the next call
    // on the stream reports the pair to hint_host (pinned host memory) before it resets them
    int* hint;
    unsigned long long* hint_host;
    unsigned hint_seq;
    // EDHIP_FLAG_ZERO_GRADIENT: the tables kernel's blocks beyond out_len[0] clear this block (16-byte
    // aligned start, any length)
    char* zero_ptr;
    long long zero_bytes;
    int* label_list;      // label kernel: [0] = count, [1..cap] = linear ids of near-tie voxels (or nullptr)
    int label_cap;
    const int* worklist;  // second-level pass: [0] = count, [1..] = tile ids to process (else nullptr)
    // K1's sampled tile boxes (deform_k1.hip): block (0, sample) of the tables kernel leaves the margin they are
    // widened by, per component, in slack[sample * 4 + h] = clamp(slack_scale * max |D_f[h]|, 0.02, 0.75) voxels
    double* slack;
    double slack_scale;
    const double* q_global;   // [O_z][O_y][ncpx][4]: displacement contracted over z and y (component padded to 4)
    const AxTab* xt_global;   // [O_x]: cubic weights / control indices along x (x 4: Q element offsets)
    int dbg;              // ablation switches for profiling (EDHIP_TILE_DBG), 0 in production
    // batches of independent volumes with one control grid each (edhip_deform_batch): sample b of
    // nbatch lives at in + b * in_bstride, out + b * out_bstride (elements), its control grid at
    // disp + b * disp_bstride (bytes), its Q table at q_global + b * q_bstride (doubles); XT is shared.
    // Strip / tile ids carry the sample: id = sample * (strips | tiles per sample) + local id.
    int nbatch;
    int ntiles;           // tiles per sample
    long long in_bstride, out_bstride, q_bstride, disp_bstride;
};

// a run of at most strip_tiles tiles along x: what one workgroup of a level-1 kernel takes
struct Strip {
    int tz, ty, tx0, ntile;   // tile coordinates of the strip and number of tiles in it
    int sample;               // which volume of the batch
};

__device__ __forceinline__ bool strip_position(const TileGeom& tg, int work, Strip& sp)
{
    if (tg.worklist) {
        // second-level pass: one 8^3 tile per work item, taken from the first level's spill list
        if (work >= tg.worklist[0])
            return false;
        int t = tg.worklist[1 + work];
        sp.sample = t / tg.ntiles;
        t -= sp.sample * tg.ntiles;
        sp.tx0 = t % tg.tiles[2];
        t /= tg.tiles[2];
        sp.ty = t % tg.tiles[1];
        sp.tz = t / tg.tiles[1];
        sp.ntile = 1;
        return true;
    }
    if (work != (int)blockIdx.x)
        return false;        // first level: one strip per block
    // strips are dealt to the XCDs in contiguous chunks (block b runs on XCD b % 8): neighbouring
    // strips, whose source boxes overlap, share an L2
    const int b = blockIdx.x;
    const int total = tg.nstrips * tg.nbatch;
    const int per = (total + 7) >> 3;
    int s = (b & 7) * per + (b >> 3);
    if (s >= total)
        return false;
    sp.sample = s / tg.nstrips;
    s -= sp.sample * tg.nstrips;
    const int sx = s % tg.strips_x;
    s /= tg.strips_x;
    sp.ty = s % tg.tiles[1];
    sp.tz = s / tg.tiles[1];
    sp.tx0 = sx * tg.strip_tiles;
    sp.ntile = min(tg.strip_tiles, tg.tiles[2] - sp.tx0);
    return true;
}

// ---- the float32 benchmark kernels (deform_hot.hip) -------------------------------------------------
// Argument block of the hot kernels: 3 deformed axes, float32, unit stride along x on both sides.
// `vol` is the array with the INPUT's deformed extents (forward: the source volume, read; gradient:
// dX, accumulated into), `img` the one with the OUTPUT's extents (forward: written; gradient: dY).
// spill feedback of K2: a tile beyond the standard box counts 1, one beyond the LARGE box counts kHintHuge (the launcher
// reads "a tenth of the tiles beyond the large box" off the same counter: ed_workspace.h)
constexpr int kHintHuge = 64;
struct HotGeom {
    const float* vol_r;       // forward: source volume
    float* vol_w;             // gradient: dX
    const float* img_r;       // gradient: dY
    float* img_w;             // forward: destination
    const double* q;          // per-call tables (see tile_tables_kernel)
    const AxTab* xt;
    const double* slack;      // TileGeom::slack
    int* spill;               // tiles the LDS box cannot hold -> the general kernels
    int* hint;                // [0]: count of the tiles whose box exceeds small_cap elements (or nullptr)
    int small_cap;            // box_cap of the standard configuration (== box_cap unless the large boxes are in use)
    int large_cap;            // K2: box_cap of the large configuration -- a tile beyond it weighs kHintHuge in the count
    long long vol_bstride, img_bstride, q_bstride;      // elements between consecutive samples
    int in_len[3], out_len[3], off[3];
    int vol_sz, vol_sy;       // element strides of vol along z, y (x: 1)
    int img_sz, img_sy;
    int tiles[3];
    int strips_x, strip_tiles, nstrips, total_strips, ntiles;
    int ncpx, box_cap, off_box, mode, has_affine;
    int lds_grp;          // bytes of LDS per wave group (K2, two groups per workgroup)
    // tile bounding boxes handed from the forward to the gradient kernel: [tile][8] ints (lo x3,
    // hi x3, -, -), tile = sample * ntiles + (tz * tiles_y + ty) * tiles_x + tx.  K1 writes them when
    // the pointer is set; K2 reads them when `use_boxes` is set (see EDHIP_FLAG_USE_BOXES).
    int* boxes;
    int use_boxes;
    // self_serve: a geometry whose recent calls left (almost) no tile to the spill list (spill feedback,
    // ed_workspace.h) is launched without the level-2 / level-3 kernels behind it -- two launches that cost the
    // benchmark step 36 us for 2 tiles of 32768 -- and level 1 serves a tile whose box does not fit itself,
    // straight from / to global memory
    int self_serve;
    int io16;                     // IOView::out16: the output side (img_r / img_w) holds 16-bit floats
    int q_strips;                 // TileGeom::q_strips (1: the plain Q layout; ncpx then is the window width)
    unsigned long long* dbgbuf;   // EDHIP_EXPERIMENTS builds: per-workgroup timestamps (else unused)
    // integer fast path (wave_int_fwd_kernel): near-tie voxels for the exact re-evaluation,
    // [0] = count, [1 .. tie_cap] = linear output voxel ids; the constant of 'constant' mode in fp64
    int* tie_list;
    int tie_cap;
    double cvald;
    int dbg;                  // experiment switches (EDHIP_TILE_DBG), 0 in production
    float cval;
    int nstep;
    long long nsteps;
    long long step_len[8], vol_step[8], img_step[8];    // element strides of the step axes
    double period[3], inv_period[3], affine[12];
};

// One lane's share of filling HotParams in LDS, k = 0 .. 11.  The caller picks the twelve threads and places the
// barrier; HotParams::slack is K1's own.
__device__ __forceinline__ void fill_hot_params(HotParams* hp, const HotGeom& hg, int k)
{
    hp->affine[k] = hg.affine[k];
    if (k < 3) {
        hp->offd[k] = (double)hg.off[k];
        hp->last[k] = (double)(hg.in_len[k] - 1);
        hp->period[k] = hg.period[k];
        hp->inv_period[k] = hg.inv_period[k];
    }
    if (k < 8) {
        hp->step_len[k] = hg.step_len[k];
        hp->in_step_stride[k] = hg.vol_step[k];
        hp->out_step_stride[k] = hg.img_step[k];
    }
    if (k == 0)
        hp->nstep = hg.nstep;
}

// element offsets of step `ss` of the step axes (the axes that are not deformed) on the input and output side;
// I: long long or int64_t
template <typename I>
__device__ __forceinline__ void hot_step_offsets(const HotParams* hp, long long ss, I& vol_off, I& img_off)
{
    vol_off = 0;
    img_off = 0;
    I r = ss;
    const int nstep = hp->nstep;
    for (int l = 0; l < nstep; ++l) {
        const I len = hp->step_len[l];
        const I q = r / len;
        const I c = r - q * len;
        vol_off += hp->in_step_stride[l] * c;
        img_off += hp->out_step_stride[l] * c;
        r = q;
    }
}

// ---- block -> strip of the level-1 kernels ---------------------------------------------------------------------------
// Strips are dealt to the 8 XCDs in contiguous chunks (block b runs on XCD b % 8): neighbouring strips, whose
// source boxes overlap, share an L2.  `s` = the strip of block `b` out of `total`; false: no strip.  A grid of
// 8 * ceil(total / 8) blocks covers every strip once, and no block of a larger grid takes a second turn at one.
__host__ __device__ __forceinline__ bool strip_of_block(int b, int total, int& s)
{
    const int per = (total + 7) >> 3;
    s = (b & 7) * per + (b >> 3);
    if ((b >> 3) >= per || s >= total)
        return false;
    return true;
}
// strip id -> sample and tile coordinates; nstrips = strips per sample, strips_x = strips per tile row
__host__ __device__ __forceinline__ void strip_decode(Strip& sp, int s, int nstrips, int strips_x, int tiles_y, int tiles_x,
                                                      int strip_tiles)
{
    sp.sample = s / nstrips;
    s -= sp.sample * nstrips;
    const int sx = s % strips_x;
    s /= strips_x;
    sp.ty = s % tiles_y;
    sp.tz = s / tiles_y;
    sp.tx0 = sx * strip_tiles;
    sp.ntile = strip_tiles < tiles_x - sp.tx0 ? strip_tiles : tiles_x - sp.tx0;
}
__device__ __forceinline__ void strip_decode(const HotGeom& hg, Strip& sp, int s)
{
    strip_decode(sp, s, hg.nstrips, hg.strips_x, hg.tiles[1], hg.tiles[2], hg.strip_tiles);
}
__device__ __forceinline__ bool strip_of_block(const HotGeom& hg, Strip& sp, int b)
{
    int s;
    if (!strip_of_block(b, hg.total_strips, s))
        return false;
    strip_decode(hg, sp, s);
    return true;
}

// level-1 launch of K2 (deform_hot.hip: the gradient, orders 1-5); hipErrorNotSupported when (order, ...) has no
// instantiation
hipError_t launch_hot_grad_level1(const HotGeom& hg, int order, unsigned nblk, size_t lds, hipStream_t stream);
// level: 0 standard, 1 large (one workgroup per CU fewer and larger boxes, chosen from the spill feedback), 2 huge
// (gradient only: 64 KiB of cells, two workgroups per CU); 0: no useful box fits next to the Q rows
size_t hot_lds_bytes(bool gradient, int ncpx, int* box_cap, int* off_box, int level = 0);

// K1 of round 5 (deform_k1.hip): float32 forward, orders 1-3, sampled tile boxes; same argument block, strips of at
// most 4 tiles; hipErrorNotSupported (nothing launched) otherwise
size_t k1_lds_bytes(int ncpx, int* box_cap, int* off_box, bool large = false);
hipError_t launch_k1_level1(const HotGeom& hg, int order, unsigned nblk, size_t lds, hipStream_t stream);

// ---- K1 of round 6 (deform_k1z.hip): strips along z, displacement contracted over y and x ------------------------
// Second argument block of k1z_fwd_kernel / k1z_geo_kernel, next to HotGeom.
struct ZGeom {
    const double* r;          // [sample][O_y][O_x][ncp_z][4]: displacement contracted over y and x (component padded to 4)
    const AxTab* zt;          // [O_z]: cubic weights / control-plane byte offsets (x 32) along z
    int* recs;                // [sample * ntiles + tile][8]: tile records, written by the geometry kernel
    int* recs_half;           // [tile][2][8]: records of the z halves of the tiles whose whole box does not fit LDS
    int* missed;              // [sample * nstrips + strip]: a tile kernel saw a window outside its sampled box
    long long* steps;         // [nsteps][2]: element offsets (volume, image) of every index of the step axes
    int* sinfo;               // [sample * nstrips + strip]: 3 bits per tile of the strip (class, beyond the standard box)
    // work lists of strips: G = general tiles (geometry kernel), F = tiles that do not fit (geometry kernel) or a window
    // outside its sampled box (tile kernels).  List G is kept in two parts per XCD, heavy strips from the front and light
    // ones from the back.  ctl[parity][word][XCD] (zctl, deform_k1z.hip) = the counts of this call and the cursor the
    // general workgroups deal list G with; the geometry kernel clears the other parity's words for the next call on the
    // stream (the head of the geometry buffer, ed::GeoBuffer, is cleared when allocated)
    int* list_g;
    int* list_f;
    int* ctl;
    int parity;
    void* zgen;               // 512 bytes: the uniform values of the general paths (ZGen), written by the geometry kernel
    long long r_bstride;      // doubles between consecutive samples of r
    long long disp_bstride;   // bytes between the control grids of consecutive samples
    int ncpz;
    int order;
    int strip_tiles;          // tiles per strip (along z)
    int nstrips;              // strips per sample
    int total_strips;
    double slack_scale;       // margin of the sampled boxes = clamp(slack_scale * max |D_f[h]|, 0.02, 0.75)
    int* hint;                // spill feedback (TileGeom::hint): reset / reported by the geometry kernel, counted by K1
    unsigned long long* hint_host;
    unsigned hint_seq;
};
size_t k1z_lds_bytes(int* box_cap, bool large = false);
bool k1z_supported(const GridGeom& g);
size_t k1z_r_bytes(const GridGeom& g);
hipError_t launch_k1z_geo(const GridGeom& g, const HotGeom& hg, const ZGeom& zg, const GridPrefilter& gp, int nbatch,
                          hipStream_t stream);
hipError_t launch_k1z(const HotGeom& hg, const ZGeom& zg, int order, size_t lds, hipStream_t stream);

// one-wavefront-per-tile kernels (deform_wave.hip): same argument block; `strip_tiles`, `strips_x`,
// `nstrips`, `total_strips` describe the strips of the 64-thread workgroups, `box_cap` the floats /
// cells of LDS one wave owns
hipError_t launch_wave_level1(const HotGeom& hg, int order, bool gradient, unsigned nblk, size_t lds, int occ,
                              hipStream_t stream);
size_t wave_lds_bytes(bool gradient, int occ, int* box_cap);
// integer volumes (8- / 16-bit), orders 1-5, forward: fast coordinates, fp64 taps, near-tie voxels listed
// for the exact kernel; `dtype` is the edhip_dtype of input and output
hipError_t launch_wave_int(const HotGeom& hg, int order, int dtype, const void* vol, void* img, unsigned nblk,
                           size_t lds, hipStream_t stream);

}  // namespace tile
}  // namespace ed
