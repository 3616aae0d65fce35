// deform_points.hip -- the coordinate map of the deformation at arbitrary real positions, and its inverse.
//
// For a real, crop-local output position q (n deformed axes; P the prefiltered control grid, K the inverse map the
// image kernels apply, the identity without affine / rotate / zoom):
//   cp_k   = (ncp_k - 1) (q_k + off_k) / (I_k - 1)
//   d_h(q) = sum_{l in {0..3}^n} P[h, m(floor(cp) - 1 + l)] prod_k w_k[l_k]      (w: cubic weights, m: mirror tap map)
//   r_h(q) = sum_l K[h, l] q_l + K[h, n] + off_h + d_h(q)
//   J[h,l] = K[h, l] + (ncp_l - 1) / (I_l - 1) sum P[h, .] w'_l[.] prod_{k != l} w_k[.]
// At integer q, r is the coordinate of the image kernels before their boundary map (ed_exact_coord.h).  No boundary
// mode is applied: the mirror tap map extends the spline to every real q, r is C2 and J continuous.
//
//   points_kernel<N, LDS, false>   r(q), optionally J, for every point
//   points_kernel<N, LDS, true>    q with r(q) = p by a damped Newton iteration from q0 = M (p - off - K[:, n]):
//                                  step from the analytic J (adjugate for n <= 3, Gaussian elimination with partial
//                                  pivoting beyond), halved while the residual's max-norm does not decrease (at most
//                                  10 halvings), stop at |r(q) - p|_inf <= tol.  max_iter steps, an exhausted
//                                  backtrack, a singular J or a non-finite input: NaN in every component, status 0.
//
// One thread per point (grid-stride beyond the launch's range), blockIdx.y = sample, fp64 throughout; float32 points
// are widened at the load and float32 results rounded once at the store.  The control grid (any dtype, any strides)
// is staged in LDS as doubles when it has at most kPointsLdsValues values (stage_grid_lds) and read from global
// memory beyond.  No atomics and no cross-lane operations: a point's result depends on that point and the call's
// arguments only, so a sample of a batch, a slice of the points and a repeated call give the same bits.  The 1- to
// 3-axis instances keep everything in registers (the tap sum unrolled, but for the outermost of three tap loops);
// 4 to 7 axes run an odometer over the 4^n taps.
//
// eval_map, solve, invert_map and the grid readers live in ed_points.h: deform_points_grad.hip (the adjoint of both
// directions) and deform_unwarp.hip (the image resampled back through the deformation) share them.
#include <cmath>
#include <cstring>

#include "ed_device.h"
#include "ed_exact_coord.h"
#include "ed_params.h"
#include "ed_points.h"

namespace ed {

namespace {

template <int N, bool LDS, bool INVERSE>
__global__ __launch_bounds__(kPointsThreads) void points_kernel(PointsArgs a)
{
    extern __shared__ double s_grid[];        // LDS: [N][ncp_0]...[ncp_{N-1}]
    const int64_t b = blockIdx.y;
    a.g.disp += b * a.disp_bstride;           // this sample's control grid
    const GridGeom& g = a.g;
    // (the tap strides and, below, the position load stand inline, not as grid_tap_strides / load_point of ed_points.h:
    // through the helpers the 28 instances come out with another register allocation, <3, LDS, forward> with one wave
    // per SIMD fewer; DESIGN.md, "One copy of the reduction")
    int64_t tstride[N];
    int per = 0;
    if constexpr (LDS) {
        per = stage_grid_lds<N>(g, s_grid);
        __syncthreads();
        int64_t cs = 1;
#pragma unroll
        for (int k = N - 1; k >= 0; --k) {
            tstride[k] = cs;
            cs *= g.ncp[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            tstride[k] = g.disp_stride[k + 1];
    }
    const char* pts = a.pts + b * a.pts_bstride;
    char* res = a.res + b * a.res_bstride;

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts;
         i += (int64_t)gridDim.x * blockDim.x) {
        double p[N], out[N];
#pragma unroll
        for (int h = 0; h < N; ++h) {
            const char* src = pts + i * a.pts_stride[0] + h * a.pts_stride[1];
            p[h] = a.pts_f32 ? (double)*(const float*)src : *(const double*)src;
        }
        if constexpr (INVERSE) {
            bool ok;
            if constexpr (LDS)
                ok = invert_map<N>(a, LdsGrid{s_grid, per}, tstride, p, out);
            else
                ok = invert_map<N>(a, GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, tstride, p, out);
            if (!ok) {
#pragma unroll
                for (int h = 0; h < N; ++h)
                    out[h] = NAN;
            }
            if (a.status)
                a.status[b * a.status_bstride + i * a.status_stride] = ok ? 1 : 0;
        } else {
            double J[N][N];
            if constexpr (LDS)
                eval_map<N>(a, LdsGrid{s_grid, per}, tstride, p, out, J);
            else
                eval_map<N>(a, GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, tstride, p, out, J);
            if (a.jac) {
                char* dst = a.jac + b * a.jac_bstride + i * a.jac_stride[0];
#pragma unroll
                for (int h = 0; h < N; ++h)
#pragma unroll
                    for (int l = 0; l < N; ++l)
                        *(double*)(dst + h * a.jac_stride[1] + l * a.jac_stride[2]) = J[h][l];
            }
        }
#pragma unroll
        for (int h = 0; h < N; ++h) {
            char* dst = res + i * a.res_stride[0] + h * a.res_stride[1];
            if (a.res_f32)
                *(float*)dst = (float)out[h];
            else
                *(double*)dst = out[h];
        }
    }
}

template <int N>
hipError_t launch_points(const PointsArgs& a, bool inverse, int nbatch, size_t lds, hipStream_t stream)
{
    const dim3 grid = points_grid(a.npts, nbatch);
    const dim3 block(kPointsThreads);
    if (lds) {
        if (inverse)
            hipLaunchKernelGGL((points_kernel<N, true, true>), grid, block, lds, stream, a);
        else
            hipLaunchKernelGGL((points_kernel<N, true, false>), grid, block, lds, stream, a);
    } else {
        if (inverse)
            hipLaunchKernelGGL((points_kernel<N, false, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((points_kernel<N, false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}


}  // namespace

hipError_t launch_deform_points(const PointsCall& c, hipStream_t stream)
{
    const GridGeom& g = c.g;
    const int n = g.naxis;
    if (n < 1 || n > kMaxAxes || c.nbatch > 65535)
        return hipErrorNotSupported;
    if (c.npts <= 0 || c.nbatch <= 0)
        return hipSuccess;                    // nothing to launch
    PointsArgs a;
    memset(&a, 0, sizeof(a));
    const int64_t values = fill_points_args(a, g, c.disp_bstride, c.forward_linear, c.max_iter, c.tol);
    unpack(c.pts, a.pts, a.pts_stride, a.pts_bstride);
    unpack(c.res, a.res, a.res_stride, a.res_bstride);
    unpack(c.jac, a.jac, a.jac_stride, a.jac_bstride);
    unpack(c.status, a.status, a.status_stride, a.status_bstride);
    a.pts_f32 = c.pts.dtype == EDHIP_F32;
    a.res_f32 = c.res.dtype == EDHIP_F32;
    if (c.inverse)
        a.jac = nullptr;
    else
        a.status = nullptr;
    a.npts = c.npts;
    const size_t lds = values <= kPointsLdsValues ? (size_t)values * sizeof(double) : 0;
    switch (n) {
    case 1: return launch_points<1>(a, c.inverse, c.nbatch, lds, stream);
    case 2: return launch_points<2>(a, c.inverse, c.nbatch, lds, stream);
    case 3: return launch_points<3>(a, c.inverse, c.nbatch, lds, stream);
    case 4: return launch_points<4>(a, c.inverse, c.nbatch, lds, stream);
    case 5: return launch_points<5>(a, c.inverse, c.nbatch, lds, stream);
    case 6: return launch_points<6>(a, c.inverse, c.nbatch, lds, stream);
    default: return launch_points<7>(a, c.inverse, c.nbatch, lds, stream);
    }
}

}  // namespace ed
