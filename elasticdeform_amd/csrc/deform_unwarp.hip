// deform_unwarp.hip -- an image carried back through the deformation (edhip_deform_inverse): the image-side
// counterpart of the inverse direction of deform_points.hip.
//
// deform_grid is a pull warp, Y[o] = X(r(o)).  For every integer source position p (extents I, the deformed extents
// of X) this kernel solves r(q) = p for the crop-local real position q in Y -- invert_map of ed_points.h, the very
// iteration of points_kernel<N, LDS, true>: same start, damped Newton step, halvings, tol and max_iter -- and stores
//   Z[p, step] = S_Y(q)[step]
// where S_Y is the gather deform_grid applies to its input at a source coordinate, on the array Y of deformed extents
// O: map_coordinate per axis, window_start, the mirror edge taps, spline_weights(order), the fp64 tap sum in the
// reference's tap order (lexicographic, last axis fastest; value, then * w_0, * w_1, * w_2, then added:
// deform.c:841-924 as deform_exact.hip restates it, no FMA) and store_forward.  A 'constant' coordinate outside
// [0, O_k - 1] gives cval; a voxel whose iteration does not solve gives cval in EVERY mode.  valid[p] = 1 exactly when
// q was solved and 0 <= q_k <= O_k - 1 on every axis: Z is interpolated from inside Y there.
//
// One thread per source voxel (the thread lattice is I = GridGeom::in_len; the array that is sampled and
// bounds-checked has the extents O = GridGeom::out_len), last deformed axis fastest, blockIdx.y = sample.  The thread
// runs in two phases that share q[N] and the solved flag only: the Newton phase (fp64, the control grid staged in LDS
// as doubles up to kPointsLdsValues values and read from global memory beyond), then the gather phase, which forms the
// taps and weights once and loops over the steps (channels) of its voxel.  The outer tap loops stay rolled and rotate
// their weights and offsets through scalars, the innermost row of up to six taps is unrolled and loaded together, so
// every array is indexed with compile-time constants (nothing goes to scratch).  Whatever the coordinate, no load
// leaves Y: tap indices are clamped to [0, O_k - 1] (no effect on a coordinate the boundary map produced).  No
// atomics, no workspace, no synchronisation beyond the staging barrier: a voxel's result depends on the call's
// arguments alone, so a sample of a batch and a repeated call give the same bits.
//
// The front of the kernel (staging, voxel index, Newton phase: solve_voxel) and the formation of the taps and weights
// (form_taps) and the tap sum (tap_sum) live in ed_unwarp.h: deform_unwarp_grad.hip, the adjoint in the image, and
// deform_unwarp_tgrad.hip, the gradient with respect to the deformation, run the same code.
#include <cstring>

#include "ed_unwarp.h"

namespace ed {

namespace {

// what the gather phase reads (never written in the kernel: its step arrays are indexed at run time)
struct UnwarpView {
    IOView v;                                 // in: Y of sample 0 (deformed extents O); out: Z (deformed extents I)
    int64_t in_bstride, out_bstride;
    unsigned char* valid;                     // uint8, deformed extents I, or nullptr
    int64_t valid_stride[3], valid_bstride;
    int64_t nsrc;                             // prod I_k: the work size
};

// The gather phase of source voxel o: S_Y(q) for every step, and valid.
template <int N>
__device__ __forceinline__ void resample(const GridGeom& g, const UnwarpView& u, const int64_t b,
                                         const int64_t (&o)[N], const double (&q)[N], const bool solved)
{
    // reference arithmetic (x86-64, no FMA): keep the products and sums separate
#pragma clang fp contract(off)
    const IOView& v = u.v;
    double w[N][6];
    int64_t tap[N][6];                        // byte offsets of the taps on each deformed axis of Y
    bool constant, inside;
    form_taps<N>(g.out_len, v, q, solved, w, tap, constant, inside);

    int64_t out_vox = 0;
#pragma unroll
    for (int k = 0; k < N; ++k)
        out_vox += v.out_stride[k] * o[k];
    if (u.valid) {
        int64_t voff = b * u.valid_bstride;
#pragma unroll
        for (int k = 0; k < N; ++k)
            voff += u.valid_stride[k] * o[k];
        u.valid[voff] = inside ? 1 : 0;
    }

    // every step (channel) of the voxel reuses q, the taps and the weights
    gather_steps<N>(v, v.in + b * u.in_bstride, v.out + b * u.out_bstride + out_vox, tap, w, constant);
}

template <int N, bool LDS>
__global__ __launch_bounds__(kUnwarpThreads) void unwarp_kernel(PointsArgs a, const UnwarpView u)
{
    extern __shared__ double s_grid[];        // LDS: [N][ncp_0]...[ncp_{N-1}]
    int64_t o[N];
    double q[N];
    bool solved;
    if (!solve_voxel<N, LDS>(a, s_grid, u.nsrc, o, q, solved))
        return;
    // the gather phase
    resample<N>(a.g, u, blockIdx.y, o, q, solved);
}

template <int N>
hipError_t launch_unwarp(const PointsArgs& a, const UnwarpView& u, int64_t values, int nbatch, hipStream_t stream)
{
    const int64_t nblk = (u.nsrc + kUnwarpThreads - 1) / kUnwarpThreads;
    if (nblk > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk, (unsigned)nbatch);
    if (values <= kPointsLdsValues)
        hipLaunchKernelGGL((unwarp_kernel<N, true>), grid, dim3(kUnwarpThreads), (size_t)values * sizeof(double),
                           stream, a, u);
    else
        hipLaunchKernelGGL((unwarp_kernel<N, false>), grid, dim3(kUnwarpThreads), 0, stream, a, u);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_deform_inverse(const InverseCall& c, hipStream_t stream)
{
    const GridGeom& g = c.g;
    const int n = g.naxis;
    if (n < 1 || n > 3 || c.nbatch > 65535 || c.v.in_dtype != c.v.out_dtype || c.v.in_dtype == EDHIP_F16 ||
        c.v.in_dtype == EDHIP_BF16 || c.v.order < 0 || c.v.order > 5)
        return hipErrorNotSupported;
    UnwarpView u;
    memset(&u, 0, sizeof(u));
    u.v = c.v;
    u.in_bstride = c.in_bstride;
    u.out_bstride = c.out_bstride;
    unpack(c.valid, u.valid, u.valid_stride, u.valid_bstride);
    u.nsrc = 1;
    for (int k = 0; k < n; ++k) {
        u.nsrc *= g.in_len[k];
        if (g.in_len[k] < 2 || g.out_len[k] < 1)
            return hipErrorInvalidValue;
    }
    if (c.nbatch <= 0 || u.nsrc <= 0 || c.v.nsteps <= 0)
        return hipSuccess;                    // nothing to launch
    PointsArgs a;
    memset(&a, 0, sizeof(a));
    const int64_t values = fill_points_args(a, g, c.disp_bstride, c.forward_linear, c.max_iter, c.tol);
    switch (n) {
    case 1: return launch_unwarp<1>(a, u, values, c.nbatch, stream);
    case 2: return launch_unwarp<2>(a, u, values, c.nbatch, stream);
    default: return launch_unwarp<3>(a, u, values, c.nbatch, stream);
    }
}

}  // namespace ed
