// ed_points_grad.h -- what the kernels of deform_points_grad.hip (the adjoint of the coordinate map and of its inverse)
// and of deform_unwarp_tgrad.hip (the gradient of an image resampled back through the deformation, with respect to the
// deformation) share: the argument block of the fixed-point reduction, the layout of the call's scratch, and the two
// small device helpers both "prepare" kernels use.  The reduction's kernels (points_grad_clear, points_grad_scatter,
// points_grad_finish) are compiled once, in deform_points_grad.hip; launch_points_grad_clear / _reduce (ed_params.h)
// run them for a caller that has written the rows itself.
//
// Scratch of one call, 64-bit words, in this order:
//   nbatch x kGradHead          per sample: bits of max|u|, bits of max|q|, the non-finite flag, the number of
//                               contributing rows
//   nbatch x cells_per          per sample: naxis (naxis + 1) cells of dK, then naxis prod ncp cells of dP
//   nbatch x rows x naxis       the u rows (doubles)
//   nbatch x rows x naxis       deform_unwarp_tgrad.hip only: the q rows (doubles); deform_points_grad.hip reads the
//                               positions from the caller's array
// Heads and cells are cleared in front of every call (points_grad_clear); the rows are written in full by "prepare".
#pragma once

#include "ed_points.h"

namespace ed {

namespace {

struct PointsGradArgs {
    PointsArgs p;                             // p.pts: the positions q; p.g, p.scale: the geometry; the rest unused
    int inverse;
    const char* cot;                          // (npts, naxis) float32 / float64
    int cot_f32;
    int64_t cot_stride[2], cot_bstride;
    const unsigned char* status;              // inverse: uint8 (npts) or nullptr
    int64_t status_stride, status_bstride;
    char* dpts;                               // (npts, naxis) float32 / float64, or nullptr
    int dpts_f32;
    int64_t dpts_stride[2], dpts_bstride;
    char* ddisp;                              // the grid's shape, a floating dtype, or nullptr
    int ddisp_dtype;
    int64_t ddisp_stride[kMaxAxes + 1], ddisp_bstride;
    char* dK;                                 // float64 (naxis, naxis + 1), or nullptr
    int64_t dK_stride[2], dK_bstride;
    unsigned long long* head;                 // per sample: bits of max|u|, of max|q|, the non-finite flag, the
                                              // number of contributing points
    unsigned long long* cells;                // per sample: naxis (naxis + 1) cells of dK, then `values` cells of dP
    double* u;                                // per sample: (npts, naxis)
    int values;                               // naxis prod ncp when the dP cells (and the grid) fit LDS, else 0
    int64_t cells_per;                        // cells per sample: naxis (naxis + 1) + naxis prod ncp
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

}  // namespace

}  // namespace ed
