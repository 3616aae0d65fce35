// ed_points_grad.h -- the fixed-point reduction behind every adjoint that sums per-point contributions into
// ddisplacement and dinverse_affine: deform_points_grad.hip (the adjoint of the coordinate map and of its inverse),
// deform_unwarp_tgrad.hip (an image resampled back through the deformation, with respect to the deformation) and
// deform_points_jet.hip (the adjoint of r, J and H).  ed_sample.h takes sane_position from here.
//
// The scheme, in four launches:
//   clear     heads and cells of every sample: zero.  Every call clears its own, so nothing is carried from one call
//             to the next and a captured graph replays self-contained.
//   prepare   the caller's kernel: per point its own row (dpoints) and whatever the scatter reads again; per sample
//             two bounds, the non-finite flag and the number of contributing points into the sample's head
//             (publish_head: wave reductions, then one integer atomic per wave and word; a max does not depend on
//             the order, and the bits of non-negative doubles order like the doubles).
//   scatter   the caller's kernel: per point and tap a coefficient c as llrint(c / quantum_P) added into 64-bit
//             integer cells (scatter_begin / scatter_end: LDS per workgroup for grids up to kPointsLdsValues values,
//             flushed with global integer atomics; global atomics directly beyond), the dK terms likewise with
//             quantum_K, reduced per wave first.
//   finish    per cell: cell * quantum into ddisplacement / dinverse_affine (NaN, or exact zeros, by the state).
// quantum = 2^(e - 62) with 2^e the smallest power of two >= the bound: no cell can overflow, and integer addition is
// associative, so the sums depend neither on the order in which the points arrive nor on how they are dealt to
// workgroups.  N below counts the points that contribute (so that points which contribute nothing do not change a bit
// of the sums).  Two rules turn a head into the two bounds (grad_quanta); they give different quanta, hence different
// bits, and both stay:
//   maxima (OWN = false)   the head holds max|u| and max|q|: bP = 2 N max|u|, bK = bP max(1, max|q|).  bP > 0 with a
//                          bK that is not finite: BOTH outputs are NaN.  deform_points_grad.hip and its callers.
//   own bounds (OWN = true) the head holds what one point can add to one cell of dP and of dK: bP = 2 N head[0],
//                          bK = 2 N head[1], each quantum with a state of its own: a bK that overflows makes
//                          dinverse_affine NaN and leaves ddisplacement finite.  deform_points_jet.hip.
// points_grad_clear and points_grad_finish are compiled once, in deform_points_grad.hip, and launched through
// launch_points_grad_clear / _finish (ed_params.h); launch_points_grad_reduce runs the points gradient's scatter and
// the finish for a caller that has written the rows itself.
//
// Scratch of one call, 64-bit words, in this order:
//   nbatch x kGradHead          per sample: bits of the two bounds (by the rule), the non-finite flag, the number of
//                               contributing rows
//   nbatch x cells_per          per sample: naxis (naxis + 1) cells of dK, then naxis prod ncp cells of dP
//   nbatch x rows x naxis       the u rows (doubles); not in deform_points_jet.hip, which reads its cotangents again
//   nbatch x rows x naxis       deform_unwarp_tgrad.hip only: the q rows (doubles); deform_points_grad.hip reads the
//                               positions from the caller's array
#pragma once

#include "ed_points.h"

namespace ed {

namespace {

// where the sums of one call go, and the cells they pass through
struct GradSums {
    char* dpts;                               // (npts, naxis) float32 / float64, or nullptr
    int dpts_f32;
    int64_t dpts_stride[2], dpts_bstride;
    char* ddisp;                              // the grid's shape, a floating dtype, or nullptr
    int ddisp_dtype;
    int64_t ddisp_stride[kMaxAxes + 1], ddisp_bstride;
    char* dK;                                 // float64 (naxis, naxis + 1), or nullptr
    int64_t dK_stride[2], dK_bstride;
    unsigned long long* head;                 // per sample kGradHead words
    unsigned long long* cells;                // per sample: naxis (naxis + 1) cells of dK, then `values` cells of dP
    int values;                               // naxis prod ncp when the dP cells (and the grid) fit LDS, else 0
    int64_t cells_per;                        // cells per sample: naxis (naxis + 1) + naxis prod ncp
};

struct PointsGradArgs {
    PointsArgs p;                             // p.pts: the positions q; p.g, p.scale: the geometry; the rest unused
    int inverse;
    const char* cot;                          // (npts, naxis) float32 / float64
    int cot_f32;
    int64_t cot_stride[2], cot_bstride;
    const unsigned char* status;              // inverse: uint8 (npts) or nullptr
    int64_t status_stride, status_bstride;
    GradSums o;                               // head: bits of max|u|, of max|q|, the flag, the count
    double* u;                                // per sample: (npts, naxis)
};

constexpr int kGradHead = 4;                  // 64-bit words per sample in front of the cells

// cells per sample: naxis (naxis + 1) + naxis prod ncp
inline int64_t points_grad_cells_per(const GridGeom& g)
{
    int64_t values = g.naxis;
    for (int k = 0; k < g.naxis; ++k)
        values *= g.ncp[k];
    return values + g.naxis * (g.naxis + 1);
}

// The output block of a call whose scratch begins with heads and cells; returns whether grid and cells fit LDS.
inline bool fill_grad_sums(GradSums& o, const BatchArray& dpts, const BatchArray& ddisp, const BatchArray& dK,
                           const GridGeom& g, char* scratch, int nbatch)
{
    unpack(dpts, o.dpts, o.dpts_stride, o.dpts_bstride);
    unpack(ddisp, o.ddisp, o.ddisp_stride, o.ddisp_bstride);
    unpack(dK, o.dK, o.dK_stride, o.dK_bstride);
    o.dpts_f32 = dpts.dtype == EDHIP_F32;
    o.ddisp_dtype = ddisp.dtype;
    o.cells_per = points_grad_cells_per(g);
    const int64_t values = o.cells_per - g.naxis * (g.naxis + 1);
    const bool lds = values <= kPointsLdsValues;
    o.values = lds ? (int)values : 0;
    o.head = (unsigned long long*)scratch;
    o.cells = o.head + (size_t)nbatch * kGradHead;
    return lds;
}

// the control coordinate of eval_map and whether the taps around it are exact integers
template <int N>
__device__ __forceinline__ bool sane_position(const PointsArgs& a, const double (&q)[N])
{
    bool sane = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double cpq = (double)(a.g.ncp[k] - 1) * (q[k] + (double)a.g.off[k]) / (double)(a.g.in_len[k] - 1);
        sane = sane && fabs(cpq) < kPointsMaxCoordinate;
    }
    return sane;
}

__device__ __forceinline__ double wave_max(double v)
{
    for (int m = warpSize / 2; m > 0; m >>= 1) {
        const double o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// a thread's two maxima, its non-finite flag and its count of contributing points into the sample's head: per wave
// first, then one integer atomic per wave and word
__device__ __forceinline__ void publish_head(unsigned long long* head, double max0, double max1, bool bad,
                                             unsigned long long count)
{
    max0 = wave_max(max0);
    max1 = wave_max(max1);
    const bool any_bad = __any(bad);
    for (int m = warpSize / 2; m > 0; m >>= 1)
        count += (unsigned long long)__shfl_xor((long long)count, m);
    if ((threadIdx.x & (warpSize - 1)) == 0) {
        if (max0 > 0.0)
            atomicMax(head + 0, (unsigned long long)__double_as_longlong(max0));
        if (max1 > 0.0)
            atomicMax(head + 1, (unsigned long long)__double_as_longlong(max1));
        if (any_bad)
            atomicMax(head + 2, 1ull);
        if (count)
            atomicAdd(head + 3, count);
    }
}

// the exponent e of the smallest power of two >= bound (bound > 0 and finite)
__device__ __forceinline__ int ceil_pow2_exponent(double bound)
{
    int ex;
    const double m = frexp(bound, &ex);       // bound = m 2^ex, 0.5 <= m < 1
    return m == 0.5 ? ex - 1 : ex;
}

__device__ __forceinline__ unsigned long long quantise(double c, int shift)
{
    return (unsigned long long)llrint(ldexp(c, shift));
}

// The two quanta of a sample as exponents (quantum = 2^(e - 62)), each with its state: 0 nothing to add (exact
// zeros), 1 e is set, -1 not representable (the bound overflows: NaN).  OWN: the rule (the head of this file).
template <bool OWN>
__device__ __forceinline__ void grad_quanta(const unsigned long long* head, int& eP, int& eK, int& sP, int& sK)
{
    const double h0 = __longlong_as_double((long long)head[0]);
    const double h1 = __longlong_as_double((long long)head[1]);
    const double bP = 2.0 * (double)head[3] * h0;
    const double bK = OWN ? 2.0 * (double)head[3] * h1 : bP * (h1 > 1.0 ? h1 : 1.0);
    sP = !(bP > 0.0) ? 0 : (isfinite(bP) ? 1 : -1);
    sK = !(bK > 0.0) ? 0 : (isfinite(bK) ? 1 : -1);
    if (!OWN)
        sP = sK = sP == 0 ? 0 : sK;           // one state for both (bK >= bP)
    eP = sP > 0 ? ceil_pow2_exponent(bP) : 0;
    eK = sK > 0 ? ceil_pow2_exponent(bK) : 0;
}

template <int N>
__device__ __forceinline__ void store_point_row(const GradSums& o, int64_t b, int64_t i, const double (&row)[N])
{
    char* dst = o.dpts + b * o.dpts_bstride + i * o.dpts_stride[0];
#pragma unroll
    for (int h = 0; h < N; ++h) {
        if (o.dpts_f32)
            *(float*)(dst + h * o.dpts_stride[1]) = (float)row[h];
        else
            *(double*)(dst + h * o.dpts_stride[1]) = row[h];
    }
}

// In front of a scatter kernel's point loop: the workgroup's LDS cells zeroed (LDS and wantP), the C-order strides
// of one component's cells; returns their number, prod ncp.
template <int N, bool LDS>
__device__ __forceinline__ int64_t scatter_begin(const GridGeom& g, const GradSums& o, bool wantP,
                                                 unsigned long long* s_cells, int64_t (&cstride)[N])
{
    if constexpr (LDS) {
        if (wantP) {
            for (int e = threadIdx.x; e < o.values; e += blockDim.x)
                s_cells[e] = 0ull;
            __syncthreads();
        }
    }
    int64_t per = 1;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
        cstride[k] = per;
        per *= g.ncp[k];
    }
    return per;
}

// Behind it: the thread's dK accumulators per wave first, then one atomic per wave and cell; the workgroup's LDS
// cells into the sample's.
template <int N, bool LDS>
__device__ __forceinline__ void scatter_end(const GradSums& o, bool wantP, bool wantK,
                                            const unsigned long long (&accK)[N * (N + 1)],
                                            const unsigned long long* s_cells, unsigned long long* cellsK)
{
    constexpr int NK = N * (N + 1);
    if (wantK) {
#pragma unroll
        for (int e = 0; e < NK; ++e) {
            unsigned long long v = accK[e];
            for (int m = warpSize / 2; m > 0; m >>= 1)
                v += (unsigned long long)__shfl_xor((long long)v, m);
            if ((threadIdx.x & (warpSize - 1)) == 0 && v != 0ull)
                atomicAdd(&cellsK[e], v);
        }
    }
    if constexpr (LDS) {
        if (wantP) {
            __syncthreads();
            for (int e = threadIdx.x; e < o.values; e += blockDim.x) {
                const unsigned long long v = s_cells[e];
                if (v != 0ull)
                    atomicAdd(&cellsK[NK + e], v);
            }
        }
    }
}

}  // namespace

}  // namespace ed
