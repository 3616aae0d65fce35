// deform_jacobian.hip -- det J of the coordinate map on the voxel lattice, and its adjoint.
//
// Notation of deform_points.hip; o is an integer crop-local output position (n = 1..3 deformed axes, x the last one):
//   J[h,l](o) = K[h,l] + s_l sum_t P[h, m(t)] w'_l prod_{k != l} w_k,   s_l = (ncp_l - 1) / (I_l - 1),   det(o) = det J(o)
// On the lattice the tap weights of axis k depend on o_k only, so the axes other than x are contracted once per row:
//   R[c][h][j_x] = sum over the taps of the outer axes of P[h, ., j_x] times
//                  c = 0: prod_k w_k          (pairs with s_x w'_x: column l = n-1 of J)
//                  c = l+1: s_l w'_l prod_{k != l} w_k   (pairs with w_x: column l < n-1)
// n x n x ncp_x values a row (16-tap sums for 3 axes, 4-tap for 2, the grid itself for 1); every voxel of the row then
// does 4 x-taps for each of its n x n entries.
//
//   jacobian_kernel<N, LDS, true>    forward: a workgroup serves tiles of `tr` rows: R of the tile into LDS (the grid from
//                                    LDS -- stage_grid_lds, up to kPointsLdsValues values -- or from global memory),
//                                    then one thread per voxel: 4 taps per entry, det, one coalesced store.
//   jacobian_kernel<N, LDS, false>   forward when R does not fit its LDS share (n n ncp_x > kJacRowValues): eval_map of
//                                    ed_points.h per voxel, the full 4^n-tap sum.
// The route depends on the grid's shape only, and a voxel's weights on its global position o + off only: det does not
// depend on where in a row, tile, crop or batch the voxel sits.
//
// The adjoint, for g = dL/d det and C the cofactor matrix of J (d det / dJ = C, also where det = 0), G = g C:
//   dP[h,j]   = sum_o sum_l G[h,l](o) d_l beta_j(o),        dK[h,l<n] = sum_o G[h,l](o),        dK[h,n] = 0
// is the transposed chain, every sum in an order that depends on the shapes only (no atomics):
//   jacobian_grad_rows_kernel<N>     a unit = `xc` consecutive voxels of one row.  It reaches a window of w control
//                                    points along x only (reached_window: w <= min(ncp_x, ceil((xc - 1) s_x) + 5)), and
//                                    xc <= 256 is as large as n n w <= 512 and 2 xc w <= 2560 allow: any ncp_x is
//                                    served, a fine last axis by more units a row.  R of the row on the window (the
//                                    grid from LDS where it fits next to the rest, from global memory otherwise),
//                                    per voxel J, C and G into LDS next to the voxel's x weights folded onto the
//                                    window (b_x(v, j) and s_x b'_x(v, j), dense rows of odd stride); then a thread
//                                    per (segment of the unit, j_x) sums its voxels' n n entries -- G[h,n-1] s_x b'_x
//                                    (c = 0) and G[h,l] b_x (c = l+1) -- in registers, and the segments are added in
//                                    order: the transposed R on the window, n n w values, plus the n n plain sums of
//                                    G, into the unit's record of the workspace.  The contractions below find a
//                                    unit's window again from its index.
//   jacobian_grad_mid_kernel         3 axes: per z the sums over y (and the units of a row) against w_y / s_y w'_y.
//   jacobian_grad_finish_kernel<N>   the sums over the first axis against its weights: dP in the caller's layout, dK.
//                                    Both contractions sum an output's range in equal pieces (8 / 32 threads an
//                                    output), added in piece order through LDS.
// Workspace: per sample units x (n n wmax + n n) doubles (wmax: the bound of w, one more for rounding), for 3 axes
// plus O_z x (2 n ncp_y ncp_x + n n) doubles (jacobian_grad_scratch_bytes).
//
// fp64 throughout, default contraction.  The cooperative phases are blockDim-strided loops and every launch a
// grid-stride loop, so that the kernels also run as workgroups of one thread (tests/cxx/jacobian_host_test.cpp).
#include <cmath>
#include <cstring>

#include "ed_device.h"
#include "ed_exact_coord.h"
#include "ed_params.h"
#include "ed_points.h"

namespace ed {

namespace {

constexpr int kJacThreads = 256;
constexpr int kJacMaxBlocks = 2048;           // per sample; tiles / units beyond: grid-stride loop
constexpr int kJacRowValues = 512;            // doubles of LDS for R (the forward: of all rows of a tile)
constexpr int kJacChunk = 256;                // voxels of a unit of the gradient, at most
constexpr size_t kJacLdsBytes = 64 * 1024;    // a workgroup's LDS
constexpr int kJacDenseValues = 2560;        // doubles of LDS for a unit's folded x weights and their derivatives
constexpr int kJacPartValues = 2816;          // doubles of LDS for the partial sums of a unit's segments
constexpr int kJacMidGroup = 32;              // outputs a workgroup of the y contraction serves at a time (8 pieces each)
constexpr int kJacFinishGroup = 8;            // ... of the last contraction (32 pieces each)

struct JacArgs {
    PointsArgs p;                             // g (out_len: the crop), disp_bstride, scale; the rest unused
    char* det;                                // forward: det (written); gradient: g = dL/d det (read); float32 / float64
    int det_f32;
    int64_t det_stride[3], det_bstride;
    int64_t nrows;                            // prod out_len[0 .. n-2]
    int tr;                                   // forward: rows per tile
    int64_t ntiles;
    int xc, nch, nseg, seglen;                // gradient: voxels per unit, units per row, segments per unit, voxels per segment
    int wmax, wstride;                        // control points along x a unit reaches, at most; the odd stride of its dense rows
    int64_t units;                            // nrows * nch
    double* part;                             // units x (n n wmax + n n) per sample
    double* mid;                              // 3 axes: out_len[0] x (2 n ncp_y ncp_x + n n) per sample
    int64_t part_bstride, mid_bstride;        // doubles
    char* ddisp;                              // dP, the grid's shape, float32 / float64; nullptr: not wanted
    int ddisp_f32;
    int64_t ddisp_stride[4], ddisp_bstride;
    char* dK;                                 // float64 (n, n + 1); nullptr: not wanted
    int64_t dK_stride[2], dK_bstride;
};

__device__ __forceinline__ int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }

// weights, derivative weights (times s_k) and folded tap indices of lattice position o on axis k
__device__ __forceinline__ void axis_taps(const PointsArgs& a, int k, int64_t o, double (&w)[4], double (&dw)[4],
                                          int (&m)[4])
{
    const GridGeom& g = a.g;
    const double cp = (double)(g.ncp[k] - 1) * (double)(o + g.off[k]) / (double)(g.in_len[k] - 1);
    const int64_t start = window_start(cp, 3);
    spline_weights(cp, 3, w);
    spline_weight_derivatives(cp, 3, dw);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        m[t] = (int)mirror_index(start + t, g.ncp[k]);
        dw[t] *= a.scale[k];
    }
}

// the weight and the derivative weight with which position o of axis k falls onto control point j (folded taps added)
__device__ __forceinline__ void fold_weights(const PointsArgs& a, int k, int64_t o, int j, double& ws, double& dws)
{
    double w[4], dw[4];
    int m[4];
    axis_taps(a, k, o, w, dw, m);
    ws = dws = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        ws += m[t] == j ? w[t] : 0.0;
        dws += m[t] == j ? dw[t] : 0.0;
    }
}

// The control points of axis k that the positions first .. last reach: jlo .. jlo + w - 1.  The window starts of
// consecutive positions do not decrease, so the folded taps of the two ends bound everything between them once the
// axis has more than 5 points (a fold then lands next to the axis' end: -1 -> 1, ncp -> ncp - 2, ncp + 1 -> ncp - 3);
// shorter axes are taken whole.  w <= min(ncp, ceil((last - first) s_k) + 5).
__device__ __forceinline__ void reached_window(const PointsArgs& a, int k, int64_t first, int64_t last, int& jlo, int& w)
{
    const int ncp = (int)a.g.ncp[k];
    if (ncp <= 5) {
        jlo = 0;
        w = ncp;
        return;
    }
    double wt[4], dwt[4];
    int m0[4], m1[4];
    axis_taps(a, k, first, wt, dwt, m0);
    axis_taps(a, k, last, wt, dwt, m1);
    int lo = m0[0], hi = m0[0];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        lo = m0[t] < lo ? m0[t] : lo;
        lo = m1[t] < lo ? m1[t] : lo;
        hi = m0[t] > hi ? m0[t] : hi;
        hi = m1[t] > hi ? m1[t] : hi;
    }
    jlo = lo;
    w = hi - lo + 1;
}

// ... of unit `ch` of a row of the gradient: positions ch xc .. along axis k, the same for every row
__device__ __forceinline__ void unit_window(const JacArgs& a, int k, int64_t ch, int& jlo, int& w)
{
    const int64_t x0 = ch * a.xc;
    reached_window(a.p, k, x0, imin64(x0 + a.xc, a.p.g.out_len[k]) - 1, jlo, w);
}

// The contraction launches: a workgroup serves `group` outputs at a time and sums each over its range [0, n) in
// blockDim / group pieces -- thread (piece, output) -- that are then added in piece order.
struct Pieces {
    int group, npiece, out, piece;
};
__device__ __forceinline__ Pieces pieces_of(int group)
{
    Pieces p;
    p.group = (int)blockDim.x < group ? (int)blockDim.x : group;
    p.npiece = (int)blockDim.x / p.group;
    p.out = (int)threadIdx.x % p.group;
    p.piece = (int)threadIdx.x / p.group;
    return p;
}
__device__ __forceinline__ void piece_range(const Pieces& p, int64_t n, int64_t& lo, int64_t& hi)
{
    const int64_t len = (n + p.npiece - 1) / p.npiece;
    lo = imin64(p.piece * len, n);
    hi = p.piece < p.npiece ? imin64(lo + len, n) : lo;
}
// every thread of the workgroup calls it; the sum is returned to piece 0
__device__ __forceinline__ double combine(const Pieces& p, double acc, double* s_sum)
{
    __syncthreads();                          // the readers of the round before
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    double total = 0.0;
    if (p.piece == 0)
        for (int q = 0; q < p.npiece; ++q)
            total += s_sum[q * p.group + p.out];
    return total;
}

// outer coordinates o[0 .. N-2] of a row
template <int N>
__device__ __forceinline__ void decode_row(const GridGeom& g, int64_t row, int64_t (&o)[N])
{
#pragma unroll
    for (int k = N - 2; k >= 0; --k) {
        o[k] = row % g.out_len[k];
        row /= g.out_len[k];
    }
}

// R[c] (c = 0 .. N-1) at (h, j_x) of the row with outer coordinates o[0 .. N-2]
template <int N, typename Grid>
__device__ __forceinline__ void row_values(const PointsArgs& a, const Grid& grid, const int64_t (&ts)[N],
                                           const int64_t (&o)[N], int h, int jx, double (&R)[N])
{
    typedef typename Grid::Off Off;
    const Off ox = (Off)(jx * ts[N - 1]);
    if constexpr (N == 1) {
        R[0] = grid(h, ox);
    } else if constexpr (N == 2) {
        double w[4], dw[4];
        int m[4];
        axis_taps(a, 0, o[0], w, dw, m);
        R[0] = R[1] = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double p = grid(h, (Off)(m[t] * ts[0]) + ox);
            R[0] += w[t] * p;
            R[1] += dw[t] * p;
        }
    } else {
        double wz[4], dwz[4], wy[4], dwy[4];
        int mz[4], my[4];
        axis_taps(a, 0, o[0], wz, dwz, mz);
        axis_taps(a, 1, o[1], wy, dwy, my);
        R[0] = R[1] = R[2] = 0.0;
#pragma unroll
        for (int tz = 0; tz < 4; ++tz) {
            double sy = 0.0, sdy = 0.0;
#pragma unroll
            for (int ty = 0; ty < 4; ++ty) {
                const double p = grid(h, (Off)(mz[tz] * ts[0] + my[ty] * ts[1]) + ox);
                sy += wy[ty] * p;
                sdy += dwy[ty] * p;
            }
            R[0] += wz[tz] * sy;
            R[1] += dwz[tz] * sy;
            R[2] += wz[tz] * sdy;
        }
    }
}

// J of a voxel from its row's R (sR[(c N + h) len + j_x - jlo], j_x = jlo .. jlo + len - 1) and its x taps
template <int N>
__device__ __forceinline__ void voxel_jacobian(const GridGeom& g, const double* sR, int len, int jlo,
                                               const double (&w)[4], const double (&dw)[4], const int (&m)[4],
                                               double (&J)[N][N])
{
#pragma unroll
    for (int h = 0; h < N; ++h) {
#pragma unroll
        for (int l = 0; l < N; ++l) {
            const double* r = sR + ((l == N - 1 ? 0 : l + 1) * N + h) * len;
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc += r[m[t] - jlo] * (l == N - 1 ? dw[t] : w[t]);
            J[h][l] = acc + (g.has_affine ? g.affine[h * (N + 1) + l] : (h == l ? 1.0 : 0.0));
        }
    }
}

// det J and the cofactor matrix C (d det / dJ[h][l] = C[h][l])
template <int N>
__device__ __forceinline__ double det_cofactors(const double (&J)[N][N], double (&C)[N][N])
{
    if constexpr (N == 1) {
        C[0][0] = 1.0;
        return J[0][0];
    } else if constexpr (N == 2) {
        C[0][0] = J[1][1];
        C[0][1] = -J[1][0];
        C[1][0] = -J[0][1];
        C[1][1] = J[0][0];
        return J[0][0] * J[1][1] - J[0][1] * J[1][0];
    } else {
        C[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        C[0][1] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        C[0][2] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        C[1][0] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
        C[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
        C[1][2] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
        C[2][0] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
        C[2][1] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
        C[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        return J[0][0] * C[0][0] + J[0][1] * C[0][1] + J[0][2] * C[0][2];
    }
}

template <int N>
__device__ __forceinline__ char* det_address(const JacArgs& a, char* base, const int64_t (&o)[N])
{
    int64_t off = 0;
#pragma unroll
    for (int k = 0; k < N; ++k)
        off += o[k] * a.det_stride[k];
    return base + off;
}

// ---- forward -------------------------------------------------------------------------------------------------------
template <int N, bool LDS, bool ROWS>
__global__ __launch_bounds__(kJacThreads) void jacobian_kernel(JacArgs a)
{
    extern __shared__ double s_grid[];        // LDS: [the grid: N x ncp_0 x ... (LDS)] [R: tr x N x N x ncp_x (ROWS)]
    const int64_t b = blockIdx.y;
    a.p.g.disp += b * a.p.disp_bstride;
    const GridGeom& g = a.p.g;
    char* det = a.det + b * a.det_bstride;
    int64_t ts[N];
    int per = 0;
    if constexpr (LDS) {
        per = stage_grid_lds<N>(g, s_grid);
        __syncthreads();
        int64_t cs = 1;
#pragma unroll
        for (int k = N - 1; k >= 0; --k) {
            ts[k] = cs;
            cs *= g.ncp[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            ts[k] = g.disp_stride[k + 1];
    }
    const int64_t ox = g.out_len[N - 1];

    if constexpr (ROWS) {
        double* sR = s_grid + (LDS ? per * N : 0);
        const int ncpx = (int)g.ncp[N - 1];
        const int items = N * ncpx, rn = N * items;
        for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
            const int64_t row0 = tile * a.tr;
            const int nr = (int)imin64(a.tr, a.nrows - row0);
            __syncthreads();                  // the readers of the tile before
            for (int e = threadIdx.x; e < nr * items; e += blockDim.x) {
                const int r = e / items, i = e % items, h = i / ncpx, jx = i % ncpx;
                int64_t o[N];
                decode_row<N>(g, row0 + r, o);
                double R[N];
                if constexpr (LDS)
                    row_values<N>(a.p, LdsGrid{s_grid, per}, ts, o, h, jx, R);
                else
                    row_values<N>(a.p, GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, ts, o, h, jx, R);
#pragma unroll
                for (int c = 0; c < N; ++c)
                    sR[r * rn + (c * N + h) * ncpx + jx] = R[c];
            }
            __syncthreads();
            for (int64_t v = threadIdx.x; v < nr * ox; v += blockDim.x) {
                const int r = (int)(v / ox);
                int64_t o[N];
                decode_row<N>(g, row0 + r, o);
                o[N - 1] = v % ox;
                double w[4], dw[4], J[N][N], C[N][N];
                int m[4];
                axis_taps(a.p, N - 1, o[N - 1], w, dw, m);
                voxel_jacobian<N>(g, sR + r * rn, ncpx, 0, w, dw, m, J);
                const double d = det_cofactors<N>(J, C);
                char* dst = det_address<N>(a, det, o);
                if (a.det_f32)
                    *(float*)dst = (float)d;
                else
                    *(double*)dst = d;
            }
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.nvox;
             i += (int64_t)gridDim.x * blockDim.x) {
            int64_t o[N];
            int64_t rem = i;
#pragma unroll
            for (int k = N - 1; k >= 0; --k) {
                o[k] = rem % g.out_len[k];
                rem /= g.out_len[k];
            }
            double q[N], r[N], J[N][N], C[N][N];
#pragma unroll
            for (int k = 0; k < N; ++k)
                q[k] = (double)o[k];
            if constexpr (LDS)
                eval_map<N>(a.p, LdsGrid{s_grid, per}, ts, q, r, J);
            else
                eval_map<N>(a.p, GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, ts, q, r, J);
            const double d = det_cofactors<N>(J, C);
            char* dst = det_address<N>(a, det, o);
            if (a.det_f32)
                *(float*)dst = (float)d;
            else
                *(double*)dst = d;
        }
    }
}

// ---- gradient ------------------------------------------------------------------------------------------------------
// LDS of the row kernel, in doubles: R [N N wmax] | G [N N xc] | the folded x weights b_x(v, j) [xc wstride] | the
// folded s_x w'_x [xc wstride] | partial sums [nseg rv]: at most 512 + 2304 + 2560 + 2816 = 8192 (64 KiB).  wmax: the
// control points along x that a unit reaches, at most; wstride: wmax made odd (neighbouring voxels' rows on
// different banks).
__host__ __device__ inline size_t jac_grad_lds_doubles(int n, int wmax, int wstride, int xc, int nseg)
{
    const size_t rn = (size_t)n * n * wmax, rv = rn + (size_t)n * n;
    return rn + (size_t)n * n * xc + 2 * (size_t)xc * wstride + (size_t)nseg * rv;
}

template <int N, bool LDS>
__global__ __launch_bounds__(kJacThreads) void jacobian_grad_rows_kernel(JacArgs a)
{
    extern __shared__ double s_grid[];        // LDS: [the grid (LDS)] [what jac_grad_lds_doubles lists]
    const int64_t b = blockIdx.y;
    a.p.g.disp += b * a.p.disp_bstride;
    const GridGeom& g = a.p.g;
    const char* cot = a.det + b * a.det_bstride;
    double* part = a.part + b * a.part_bstride;
    const int wmax = a.wmax, wst = a.wstride;
    const int rn = N * N * wmax, rv = rn + N * N, xc = a.xc;   // a record: [(c N + h) wmax + j_x - jlo] [N N plain sums]
    int64_t ts[N];
    int per = 0;
    if constexpr (LDS) {
        per = stage_grid_lds<N>(g, s_grid);   // (the first unit's barrier covers it)
        int64_t cs = 1;
#pragma unroll
        for (int k = N - 1; k >= 0; --k) {
            ts[k] = cs;
            cs *= g.ncp[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            ts[k] = g.disp_stride[k + 1];
    }
    double* sR = s_grid + (LDS ? per * N : 0);
    double* sG = sR + rn;                     // [(h N + l) xc + v]
    double* sW = sG + N * N * xc;             // [v wst + j_x - jlo]
    double* sDW = sW + xc * wst;
    double* sPart = sDW + xc * wst;           // [seg rv + e]
    const int64_t ox = g.out_len[N - 1];

    for (int64_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const int64_t row = unit / a.nch, x0 = (unit % a.nch) * xc;
        const int nx = (int)imin64(xc, ox - x0);
        int64_t o[N];
        decode_row<N>(g, row, o);
        int jlo, wj;                          // the control points along x this unit reaches
        reached_window(a.p, N - 1, x0, x0 + nx - 1, jlo, wj);
        __syncthreads();                      // the readers of the unit before
        for (int e = threadIdx.x; e < N * wj; e += blockDim.x) {
            const int h = e / wj, jl = e % wj;
            double R[N];
            if constexpr (LDS)
                row_values<N>(a.p, LdsGrid{s_grid, per}, ts, o, h, jlo + jl, R);
            else
                row_values<N>(a.p, GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, ts, o, h, jlo + jl, R);
#pragma unroll
            for (int c = 0; c < N; ++c)
                sR[(c * N + h) * wmax + jl] = R[c];
        }
        __syncthreads();
        for (int v = threadIdx.x; v < nx; v += blockDim.x) {
            o[N - 1] = x0 + v;
            double w[4], dw[4], J[N][N], C[N][N];
            int m[4];
            axis_taps(a.p, N - 1, o[N - 1], w, dw, m);
            voxel_jacobian<N>(g, sR, wmax, jlo, w, dw, m, J);
            det_cofactors<N>(J, C);
            const char* src = det_address<N>(a, (char*)cot, o);
            const double gv = a.det_f32 ? (double)*(const float*)src : *(const double*)src;
#pragma unroll
            for (int h = 0; h < N; ++h)
#pragma unroll
                for (int l = 0; l < N; ++l)
                    sG[(h * N + l) * xc + v] = gv * C[h][l];
            // the voxel's row of the folded weights: its own wj cells, taps that fold onto one j added in tap order
            double* bw = sW + v * wst;
            double* bdw = sDW + v * wst;
            for (int j = 0; j < wj; ++j)
                bw[j] = bdw[j] = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                bw[m[t] - jlo] += w[t];
                bdw[m[t] - jlo] += dw[t];
            }
        }
        __syncthreads();
        // per (segment, j_x): the transposed x taps of all N N entries -- G[h][N-1] against s_x w'_x (c = 0), G[h][l]
        // against w_x (c = l + 1) -- and, with the window's first j_x, the plain sums of G
        for (int e = threadIdx.x; e < a.nseg * wj; e += blockDim.x) {
            const int seg = e / wj, jx = e % wj;
            const int v0 = seg * a.seglen, v1 = v0 + a.seglen < nx ? v0 + a.seglen : nx;
            double acc[N * N], plain[N * N];
#pragma unroll
            for (int k = 0; k < N * N; ++k)
                acc[k] = plain[k] = 0.0;
            for (int v = v0; v < v1; ++v) {
                const double ws = sW[v * wst + jx], dws = sDW[v * wst + jx];
#pragma unroll
                for (int k = 0; k < N * N; ++k) {
                    const double gk = sG[k * xc + v];
                    acc[k] += gk * (k % N == N - 1 ? dws : ws);
                    plain[k] += gk;
                }
            }
            double* dst = sPart + seg * rv;
#pragma unroll
            for (int k = 0; k < N * N; ++k) {
                const int h = k / N, l = k % N, c = l == N - 1 ? 0 : l + 1;
                dst[(c * N + h) * wmax + jx] = acc[k];
                if (jx == 0)
                    dst[rn + k] = plain[k];
            }
        }
        __syncthreads();
        // the segments in order, into the unit's record (cells beyond the unit's window stay unwritten and unread)
        for (int e = threadIdx.x; e < rv; e += blockDim.x) {
            if (e < rn && e % wmax >= wj)
                continue;
            double acc = 0.0;
            for (int seg = 0; seg < a.nseg; ++seg)
                acc += sPart[seg * rv + e];
            part[unit * rv + e] = acc;
        }
    }
}

// 3 axes: mid[z][c'][h][j_y][j_x], c' = 0: sum_y R^T[0] w_y + R^T[2] s_y w'_y (pairs with w_z), c' = 1: sum_y R^T[1] w_y
// (pairs with s_z w'_z); behind them the N N plain sums.  A (y, j_y) pair of weight zero is skipped.
__global__ __launch_bounds__(kJacThreads) void jacobian_grad_mid_kernel(JacArgs a)
{
    constexpr int N = 3;
    const int64_t b = blockIdx.y;
    const GridGeom& g = a.p.g;
    const double* part = a.part + b * a.part_bstride;
    double* mid = a.mid + b * a.mid_bstride;
    const int ncpx = (int)g.ncp[2], ncpy = (int)g.ncp[1];
    const int wmax = a.wmax, rn = N * N * wmax, rv = rn + N * N, m2 = N * ncpy * ncpx, uv = 2 * m2 + N * N;
    const int64_t oy = g.out_len[1], total = g.out_len[0] * uv;
    __shared__ double s_sum[kJacThreads];
    const Pieces p = pieces_of(kJacMidGroup);
    for (int64_t base = (int64_t)blockIdx.x * p.group; base < total; base += (int64_t)gridDim.x * p.group) {
        const int64_t i = base + p.out;
        double acc = 0.0;
        if (i < total) {
            const int64_t z = i / uv;
            const int u = (int)(i % uv);
            const double* rows = part + z * oy * a.nch * rv;
            int64_t lo, hi;
            if (u < 2 * m2) {
                const int cc = u / m2, r = u % m2, h = r / (ncpy * ncpx), jy = (r / ncpx) % ncpy, jx = r % ncpx;
                piece_range(p, oy, lo, hi);
                for (int ch = 0; ch < a.nch; ++ch) {
                    int jlo, wj;
                    unit_window(a, N - 1, ch, jlo, wj);
                    const int jl = jx - jlo;
                    if (jl < 0 || jl >= wj)
                        continue;             // the units of this piece of the rows do not reach j_x
                    for (int64_t y = lo; y < hi; ++y) {
                        double ws, dws;
                        fold_weights(a.p, 1, y, jy, ws, dws);
                        if (ws == 0.0 && dws == 0.0)
                            continue;
                        const double* row = rows + (y * a.nch + ch) * rv;
                        if (cc == 0)
                            acc += row[(0 * N + h) * wmax + jl] * ws + row[(2 * N + h) * wmax + jl] * dws;
                        else
                            acc += row[(1 * N + h) * wmax + jl] * ws;
                    }
                }
            } else {
                const int k = u - 2 * m2;
                piece_range(p, oy * a.nch, lo, hi);
                for (int64_t y = lo; y < hi; ++y)
                    acc += rows[y * rv + rn + k];
            }
        }
        acc = combine(p, acc, s_sum);
        if (p.piece == 0 && i < total)
            mid[i] = acc;
    }
}

// dP[h][j_0][rest] = sum over the first axis (and, for 2 axes, the units of a row) of in[.][0][h][rest] w_0 +
// in[.][1][h][rest] s_0 w'_0; for 1 axis the plain sum over the units.  dK[h][l < N] = the plain sums, dK[h][N] = 0.
template <int N>
__global__ __launch_bounds__(kJacThreads) void jacobian_grad_finish_kernel(JacArgs a)
{
    const int64_t b = blockIdx.y;
    const GridGeom& g = a.p.g;
    int64_t per = 1;
#pragma unroll
    for (int k = 0; k < N; ++k)
        per *= g.ncp[k];
    const int64_t inner = per / g.ncp[0], m = N * inner;
    const double* in = N == 3 ? a.mid + b * a.mid_bstride : a.part + b * a.part_bstride;
    const int64_t nouter = N == 1 ? 1 : g.out_len[0], ninner = N == 3 ? 1 : a.nch;
    // one record of `in`: 3 axes (mid) [c = 0: m] [c = 1: m] [N N plain sums]; 1 and 2 axes (a unit's)
    // [(c N + h) wmax + j_x - jlo] [N N plain sums]
    const int wmax = a.wmax, ncpx = (int)g.ncp[N - 1];
    const int64_t ex = N == 3 ? 2 * m : (int64_t)N * N * wmax, vs = ex + N * N;
    const int64_t nrec = g.nvox > 0 ? nouter * ninner : 0;
    const int64_t total = N * per + N * (N + 1);
    __shared__ double s_sum[kJacThreads];
    const Pieces p = pieces_of(kJacFinishGroup);
    for (int64_t base = (int64_t)blockIdx.x * p.group; base < total; base += (int64_t)gridDim.x * p.group) {
        const int64_t i = base + p.out;
        const bool grid_value = i < N * per;
        const bool wanted = i < total && (grid_value ? a.ddisp != nullptr : a.dK != nullptr);
        double acc = 0.0;
        int64_t lo, hi;
        if (wanted && grid_value) {
            const int64_t h = i / per, r = i % per, j0 = r / inner, rest = r % inner;
            if constexpr (N == 1) {
                piece_range(p, nrec, lo, hi);
                for (int64_t rec = lo; rec < hi; ++rec) {
                    int jlo, wj;
                    unit_window(a, 0, rec, jlo, wj);
                    const int jl = (int)r - jlo;
                    if (jl >= 0 && jl < wj)
                        acc += in[rec * vs + jl];
                }
            } else if constexpr (N == 2) {
                piece_range(p, nrec ? nouter : 0, lo, hi);
                for (int64_t ch = 0; ch < ninner; ++ch) {
                    int jlo, wj;
                    unit_window(a, 1, ch, jlo, wj);
                    const int jl = (int)(rest % ncpx) - jlo;
                    if (jl < 0 || jl >= wj)
                        continue;
                    for (int64_t o = lo; o < hi; ++o) {
                        double ws, dws;
                        fold_weights(a.p, 0, o, (int)j0, ws, dws);
                        if (ws == 0.0 && dws == 0.0)
                            continue;
                        const double* rec = in + (o * ninner + ch) * vs;
                        acc += rec[(0 * N + h) * wmax + jl] * ws + rec[(1 * N + h) * wmax + jl] * dws;
                    }
                }
            } else {
                piece_range(p, nrec ? nouter : 0, lo, hi);
                for (int64_t o = lo; o < hi; ++o) {
                    double ws, dws;
                    fold_weights(a.p, 0, o, (int)j0, ws, dws);
                    if (ws == 0.0 && dws == 0.0)
                        continue;
                    const double* rec = in + o * vs;
                    acc += rec[h * inner + rest] * ws + rec[m + h * inner + rest] * dws;
                }
            }
        } else if (wanted) {
            const int k = (int)(i - N * per), h = k / (N + 1), l = k % (N + 1);
            piece_range(p, l < N ? nrec : 0, lo, hi);
            for (int64_t rec = lo; rec < hi; ++rec)
                acc += in[rec * vs + ex + h * N + l];
        }
        acc = combine(p, acc, s_sum);
        if (p.piece != 0 || !wanted)
            continue;
        if (grid_value) {
            const int64_t h = i / per, r = i % per;
            int64_t off = h * a.ddisp_stride[0], rem = r;
#pragma unroll
            for (int k = N - 1; k >= 0; --k) {
                off += (rem % g.ncp[k]) * a.ddisp_stride[k + 1];
                rem /= g.ncp[k];
            }
            char* dst = a.ddisp + b * a.ddisp_bstride + off;
            if (a.ddisp_f32)
                *(float*)dst = (float)acc;
            else
                *(double*)dst = acc;
        } else {
            const int k = (int)(i - N * per), h = k / (N + 1), l = k % (N + 1);
            *(double*)(a.dK + b * a.dK_bstride + h * a.dK_stride[0] + l * a.dK_stride[1]) = acc;
        }
    }
}

// what both launchers fill alike; returns the number of control-grid values
int64_t fill_jac_args(JacArgs& a, const JacobianCall& c)
{
    memset(&a, 0, sizeof(a));
    const int n = c.g.naxis;
    const int64_t values = fill_points_args(a.p, c.g, c.disp_bstride, nullptr, 0, 0.0);
    a.det = c.det.ptr;
    a.det_f32 = c.det.dtype == EDHIP_F32;
    for (int k = 0; k < n; ++k)
        a.det_stride[k] = c.det.stride[k];
    a.det_bstride = c.det.bstride;
    a.nrows = 1;
    for (int k = 0; k + 1 < n; ++k)
        a.nrows *= c.g.out_len[k];
    return values;
}

inline unsigned blocks_for(int64_t work)
{
    return (unsigned)(work < 1 ? 1 : work < kJacMaxBlocks ? work : kJacMaxBlocks);
}

template <int N>
hipError_t launch_jacobian(JacArgs& a, int64_t values, int nbatch, hipStream_t stream)
{
    const GridGeom& g = a.p.g;
    const int64_t rn = (int64_t)N * N * g.ncp[N - 1], ox = g.out_len[N - 1];
    const size_t grid_lds = values <= kPointsLdsValues ? (size_t)values * sizeof(double) : 0;
    const dim3 block(kJacThreads);
    if (rn <= kJacRowValues) {
        // rows per tile: four voxels a thread (the row contraction keeps more of the workgroup busy), as far as R fits
        int64_t tr = 4 * kJacThreads / ox;
        tr = tr < 1 ? 1 : tr;
        tr = tr < kJacRowValues / rn ? tr : kJacRowValues / rn;
        tr = tr < a.nrows ? tr : a.nrows;
        a.tr = (int)tr;
        a.ntiles = (a.nrows + tr - 1) / tr;
        const dim3 grid(blocks_for(a.ntiles), (unsigned)nbatch);
        const size_t lds = grid_lds + (size_t)(tr * rn) * sizeof(double);
        if (grid_lds)
            hipLaunchKernelGGL((jacobian_kernel<N, true, true>), grid, block, lds, stream, a);
        else
            hipLaunchKernelGGL((jacobian_kernel<N, false, true>), grid, block, lds, stream, a);
    } else {
        const dim3 grid(blocks_for((g.nvox + kJacThreads - 1) / kJacThreads), (unsigned)nbatch);
        if (grid_lds)
            hipLaunchKernelGGL((jacobian_kernel<N, true, false>), grid, block, grid_lds, stream, a);
        else
            hipLaunchKernelGGL((jacobian_kernel<N, false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

// the shapes of the gradient's launches: voxels per unit, units per row, segments, and the control points along x a
// unit reaches at most
struct GradShape {
    int xc, nch, nseg, seglen, wmax, wstride;
};
GradShape grad_shape(const GridGeom& g)
{
    const int n = g.naxis;
    const int64_t ox = g.out_len[n - 1], ncpx = g.ncp[n - 1];
    const double sx = (double)(ncpx - 1) / (double)(g.in_len[n - 1] - 1);
    // reached_window's bound for xc consecutive voxels, one more for the rounding of the control coordinate
    auto width = [&](int64_t xc) {
        const int64_t w = (int64_t)std::ceil((double)(xc - 1) * sx) + 6;
        return w < ncpx ? w : ncpx;
    };
    // as many voxels as R and the folded weights of the unit have room for; one voxel (at most 6 points) always fits
    int64_t xc = ox < kJacChunk ? (ox < 1 ? 1 : ox) : kJacChunk;
    while (xc > 1 && (n * n * width(xc) > kJacRowValues || 2 * xc * (width(xc) | 1) > kJacDenseValues))
        --xc;
    GradShape s;
    s.xc = (int)xc;
    s.wmax = (int)width(xc);
    s.wstride = s.wmax | 1;
    s.nch = (int)((ox + xc - 1) / xc);
    s.nch = s.nch < 1 ? 1 : s.nch;
    // a thread per (segment, j_x): a workgroup's worth of them, as far as the partial sums fit
    const int64_t rv = n * n * s.wmax + n * n;
    int64_t segs = kJacThreads / s.wmax;
    segs = segs < kJacPartValues / rv ? segs : kJacPartValues / rv;
    segs = segs < xc ? segs : xc;
    segs = segs < 1 ? 1 : segs;
    s.seglen = (int)((xc + segs - 1) / segs);
    s.nseg = (int)((xc + s.seglen - 1) / s.seglen);
    return s;
}

template <int N>
hipError_t launch_jacobian_gradient(JacArgs& a, int nbatch, hipStream_t stream)
{
    const GridGeom& g = a.p.g;
    const dim3 block(kJacThreads);
    int64_t per = 1;
    for (int k = 0; k < N; ++k)
        per *= g.ncp[k];
    if (a.units > 0) {
        // the grid in LDS too where both fit the 64 KiB of a workgroup
        const size_t lds = jac_grad_lds_doubles(N, a.wmax, a.wstride, a.xc, a.nseg) * sizeof(double);
        const size_t grid_lds = (size_t)(N * per) * sizeof(double);
        const dim3 grid(blocks_for(a.units), (unsigned)nbatch);
        if (lds + grid_lds <= kJacLdsBytes)
            hipLaunchKernelGGL((jacobian_grad_rows_kernel<N, true>), grid, block, lds + grid_lds, stream, a);
        else
            hipLaunchKernelGGL((jacobian_grad_rows_kernel<N, false>), grid, block, lds, stream, a);
        if constexpr (N == 3) {
            const int64_t total = g.out_len[0] * (2 * N * g.ncp[1] * g.ncp[2] + N * N);
            hipLaunchKernelGGL(jacobian_grad_mid_kernel,
                               dim3(blocks_for((total + kJacMidGroup - 1) / kJacMidGroup), (unsigned)nbatch), block, 0,
                               stream, a);
        }
    }
    const int64_t total = N * per + N * (N + 1);
    hipLaunchKernelGGL((jacobian_grad_finish_kernel<N>),
                       dim3(blocks_for((total + kJacFinishGroup - 1) / kJacFinishGroup), (unsigned)nbatch), block, 0,
                       stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_deform_jacobian(const JacobianCall& c, hipStream_t stream)
{
    const int n = c.g.naxis;
    if (n < 1 || n > 3 || c.nbatch > 65535)
        return hipErrorNotSupported;
    if (c.g.nvox <= 0 || c.nbatch <= 0)
        return hipSuccess;                    // nothing to launch
    JacArgs a;
    const int64_t values = fill_jac_args(a, c);
    switch (n) {
    case 1: return launch_jacobian<1>(a, values, c.nbatch, stream);
    case 2: return launch_jacobian<2>(a, values, c.nbatch, stream);
    default: return launch_jacobian<3>(a, values, c.nbatch, stream);
    }
}

size_t jacobian_grad_scratch_bytes(const GridGeom& g, int nbatch)
{
    const int n = g.naxis;
    if (n < 1 || n > 3 || g.nvox <= 0)
        return 0;
    const GradShape s = grad_shape(g);
    int64_t rows = 1;
    for (int k = 0; k + 1 < n; ++k)
        rows *= g.out_len[k];
    size_t doubles = (size_t)rows * s.nch * (size_t)(n * n * s.wmax + n * n);
    if (n == 3)
        doubles += (size_t)g.out_len[0] * (size_t)(2 * n * g.ncp[1] * g.ncp[2] + n * n);
    return doubles * (size_t)nbatch * sizeof(double);
}

hipError_t launch_deform_jacobian_gradient(const JacobianCall& c, hipStream_t stream)
{
    const GridGeom& g = c.g;
    const int n = g.naxis;
    if (n < 1 || n > 3 || c.nbatch > 65535)
        return hipErrorNotSupported;
    if (c.nbatch <= 0 || (!c.ddisp.ptr && !c.dK.ptr))
        return hipSuccess;
    JacArgs a;
    fill_jac_args(a, c);
    if (g.nvox > 0) {
        const GradShape s = grad_shape(g);
        a.xc = s.xc, a.nch = s.nch, a.nseg = s.nseg, a.seglen = s.seglen, a.wmax = s.wmax, a.wstride = s.wstride;
        a.units = a.nrows * a.nch;
        a.part_bstride = a.units * (n * n * a.wmax + n * n);
        a.part = (double*)c.scratch;
        if (n == 3) {
            a.mid_bstride = g.out_len[0] * (2 * n * g.ncp[1] * g.ncp[2] + n * n);
            a.mid = a.part + a.part_bstride * c.nbatch;
        }
    }
    a.ddisp = c.ddisp.ptr;
    a.ddisp_f32 = c.ddisp.dtype == EDHIP_F32;
    for (int k = 0; k <= n; ++k)
        a.ddisp_stride[k] = c.ddisp.stride[k];
    a.ddisp_bstride = c.ddisp.bstride;
    a.dK = c.dK.ptr;
    a.dK_stride[0] = c.dK.stride[0];
    a.dK_stride[1] = c.dK.stride[1];
    a.dK_bstride = c.dK.bstride;
    switch (n) {
    case 1: return launch_jacobian_gradient<1>(a, c.nbatch, stream);
    case 2: return launch_jacobian_gradient<2>(a, c.nbatch, stream);
    default: return launch_jacobian_gradient<3>(a, c.nbatch, stream);
    }
}

}  // namespace ed
