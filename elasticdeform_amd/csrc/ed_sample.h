// ed_sample.h -- the front the kernels of deform_sample.hip (the deformed image at real output positions) and of
// deform_sample_grad.hip (its gradients) share: the staging of the control grid, and per point the position, r(q) and
// the sane flag.  r(q) is eval_map of ed_points.h, the very code of points_kernel<N, LDS, false>; the taps are formed
// by form_taps of ed_unwarp.h on X with the extents I = GridGeom::in_len.
#pragma once

#include <cmath>
#include <cstring>

#include "ed_points_grad.h"
#include "ed_unwarp.h"

namespace ed {

namespace {

// where a point's taps go and come from (never written in the kernel: its step arrays are indexed at run time)
struct SampleView {
    IOView v;                                 // in: X of sample 0 (deformed extents I); out: V / dV, out_stride[0] per point
    int64_t in_bstride, out_bstride;
    unsigned char* inside;                    // forward: uint8 (npts), or nullptr
    int64_t inside_stride, inside_bstride;
};

// how the evaluator reaches the control grid, the same for every point of the thread
template <int N>
struct SampleFront {
    int64_t tstride[N];
    int per;
};

// this sample's control grid, staged in s_grid with LDS (every thread of the workgroup takes part in the barrier)
template <int N, bool LDS>
__device__ __forceinline__ void sample_front(PointsArgs& a, double* s_grid, SampleFront<N>& f)
{
    a.g.disp += (int64_t)blockIdx.y * a.disp_bstride;
    const GridGeom& g = a.g;
    f.per = 0;
    if constexpr (LDS) {
        f.per = stage_grid_lds<N>(g, s_grid);
        __syncthreads();
        int64_t cs = 1;
#pragma unroll
        for (int k = N - 1; k >= 0; --k) {
            f.tstride[k] = cs;
            cs *= g.ncp[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            f.tstride[k] = g.disp_stride[k + 1];
    }
}

// point i of sample b: r = r(q_i); false where the position is not finite or not sane_position, or r is not finite
// (the point then takes cval in every mode and contributes nothing to any gradient)
template <int N, bool LDS>
__device__ __forceinline__ bool sample_point(const PointsArgs& a, const double* s_grid, const SampleFront<N>& f,
                                             const int64_t b, const int64_t i, double (&r)[N])
{
    // (load_point's lines and, above, grid_tap_strides', kept inline: through the helpers of ed_points.h the two sample
    // kernels come out with another register allocation; DESIGN.md, "One copy of the reduction")
    const char* pts = a.pts + b * a.pts_bstride + i * a.pts_stride[0];
    double q[N], J[N][N];
#pragma unroll
    for (int h = 0; h < N; ++h) {
        const char* src = pts + h * a.pts_stride[1];
        q[h] = a.pts_f32 ? (double)*(const float*)src : *(const double*)src;
    }
    if constexpr (LDS)
        eval_map<N>(a, LdsGrid{s_grid, f.per}, f.tstride, q, r, J);
    else
        eval_map<N>(a, GlobalGrid{a.g.disp, a.g.disp_stride[0], a.g.disp_dtype}, f.tstride, q, r, J);
    bool ok = sane_position<N>(a, q);
#pragma unroll
    for (int h = 0; h < N; ++h)
        ok = ok && isfinite(r[h]);
    return ok;
}

// the checks both launchers make, and what they fill alike; hipSuccess with *launch false: nothing to launch
inline hipError_t fill_sample_args(const SampleCall& c, bool float_only, PointsArgs& a, SampleView& u, int64_t& values,
                                   bool* launch)
{
    const GridGeom& g = c.g;
    const int n = g.naxis;
    *launch = false;
    const bool floats = c.v.in_dtype == EDHIP_F32 || c.v.in_dtype == EDHIP_F64;
    if (n < 1 || n > 3 || c.nbatch > 65535 || c.v.in_dtype != c.v.out_dtype || c.v.in_dtype == EDHIP_F16 ||
        c.v.in_dtype == EDHIP_BF16 || (float_only && !floats) || c.v.order < 0 || c.v.order > 5)
        return hipErrorNotSupported;
    for (int k = 0; k < n; ++k)
        if (g.in_len[k] < 2)
            return hipErrorInvalidValue;
    if (c.nbatch <= 0 || c.npts <= 0 || c.v.nsteps <= 0)
        return hipSuccess;
    memset(&a, 0, sizeof(a));
    values = fill_points_args(a, g, c.disp_bstride, nullptr, 1, 1.0);
    unpack(c.pts, a.pts, a.pts_stride, a.pts_bstride);
    a.pts_f32 = c.pts.dtype == EDHIP_F32;
    a.npts = c.npts;
    memset(&u, 0, sizeof(u));
    u.v = c.v;
    u.in_bstride = c.in_bstride;
    u.out_bstride = c.out_bstride;
    unpack(c.inside, u.inside, u.inside_stride, u.inside_bstride);
    *launch = true;
    return hipSuccess;
}

}  // namespace

}  // namespace ed
