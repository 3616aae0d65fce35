// deform_sample.hip -- the deformed image at arbitrary real output positions (edhip_deform_sample): what joins the image
// side (deform_grid) to the point side (deform_grid_coordinates).
//
// For a real, crop-local output position q of an edhip_deform call with the same control grid, crop offset and inverse
// map:
//   r(q)          what points_kernel<N, LDS, false> returns: the same eval_map (ed_points.h), fp64, no boundary map
//   V[i, step]  = S_X(r(q_i))[step]
// where S_X is the gather edhip_deform applies to its input at a source coordinate, on the array X with the deformed
// extents I: map_coordinate per axis, window_start, the mirror edge taps, spline_weights(order), the fp64 tap sum in the
// reference's tap order (no FMA) and store_forward -- the code deform_unwarp.hip runs on Y with the extents O
// (ed_unwarp.h: form_taps, tap_sum, gather_steps).  A 'constant' coordinate outside [0, I_k - 1] gives cval; a position
// that is not finite or not sane_position gives cval in EVERY mode.  inside[i] = 1 exactly when the position is sane
// and 0 <= r_k <= I_k - 1 on every axis.  At integer q this is the voxel deform_grid computes, to the rounding of the
// coordinate (the points code and the image kernels agree to 1e-10 there).
//
// One thread per point, 256 threads, blockIdx.y = sample; points past kPointsMaxBlocks * 256 are served by a
// grid-stride loop; the control grid is staged in LDS as doubles up to kPointsLdsValues values and read from global
// memory beyond (all as points_kernel).  A point runs two phases that share r[N] and the sane flag only: the eval_map
// phase, then the gather phase, which forms the taps and weights once and loops over the steps (channels).  The outer
// tap loops stay rolled, the innermost row of up to six taps is unrolled and loaded together, so every array is indexed
// with compile-time constants (nothing goes to scratch).  Whatever the coordinate, no load leaves X: tap indices are
// clamped to [0, I_k - 1].  No atomics, no workspace, no synchronisation beyond the staging barrier: a point's result
// depends on that point and the call's arguments alone, so a sample of a batch, a slice or a permutation of the points
// and a repeated call give the same bits, and the call can be captured into a graph.
#include "ed_sample.h"

namespace ed {

namespace {

template <int N, bool LDS>
__global__ __launch_bounds__(kPointsThreads) void sample_kernel(PointsArgs a, const SampleView u)
{
    extern __shared__ double s_grid[];        // LDS: [N][ncp_0]...[ncp_{N-1}]
    SampleFront<N> f;
    sample_front<N, LDS>(a, s_grid, f);
    const int64_t b = blockIdx.y;
    const IOView& v = u.v;
    const char* in_b = v.in + b * u.in_bstride;
    char* out_b = v.out + b * u.out_bstride;

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts;
         i += (int64_t)gridDim.x * blockDim.x) {
        // the eval_map phase
        double r[N];
        const bool sane = sample_point<N, LDS>(a, s_grid, f, b, i, r);
        // the gather phase
        double w[N][6];
        int64_t tap[N][6];                    // byte offsets of the taps on each deformed axis of X
        bool constant, inside;
        form_taps<N>(a.g.in_len, v, r, sane, w, tap, constant, inside);
        if (u.inside)
            u.inside[b * u.inside_bstride + i * u.inside_stride] = inside ? 1 : 0;
        gather_steps<N>(v, in_b, out_b + i * v.out_stride[0], tap, w, constant);
    }
}

template <int N>
hipError_t launch_sample(const PointsArgs& a, const SampleView& u, int64_t values, int nbatch, hipStream_t stream)
{
    const dim3 grid = points_grid(a.npts, nbatch);
    if (values <= kPointsLdsValues)
        hipLaunchKernelGGL((sample_kernel<N, true>), grid, dim3(kPointsThreads), (size_t)values * sizeof(double),
                           stream, a, u);
    else
        hipLaunchKernelGGL((sample_kernel<N, false>), grid, dim3(kPointsThreads), 0, stream, a, u);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_deform_sample(const SampleCall& c, hipStream_t stream)
{
    PointsArgs a;
    SampleView u;
    int64_t values = 0;
    bool launch;
    const hipError_t e = fill_sample_args(c, false, a, u, values, &launch);
    if (e != hipSuccess || !launch)
        return e;
    switch (c.g.naxis) {
    case 1: return launch_sample<1>(a, u, values, c.nbatch, stream);
    case 2: return launch_sample<2>(a, u, values, c.nbatch, stream);
    default: return launch_sample<3>(a, u, values, c.nbatch, stream);
    }
}

}  // namespace ed
