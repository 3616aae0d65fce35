// deform_unwarp_grad.hip -- the adjoint of deform_unwarp.hip with respect to the image (edhip_deform_inverse_gradient).
//
// For fixed deformation arguments and cval = 0 the forward is linear in Y: Z[p, s] = sum_j A[p, j] Y[j, s], the row
// A[p, :] holding the (order + 1)^N products of tap weights at q(p) (taps the mirror edge rule folds onto one cell add
// up), empty where p is not solved or where the mode is 'constant' and q(p) lies outside Y.  This kernel adds A^T dZ
// into dY: per source voxel p and step s, dZ[p, s] w_0 ... w_{N-1} into every tap cell of the voxel.
//
// Thread lattice, Newton phase and tap formation are the forward's own code (ed_unwarp.h: solve_voxel, form_taps): one
// thread per source voxel (extents I = GridGeom::in_len), last deformed axis fastest, 256 threads per workgroup,
// blockIdx.y = sample, the control grid in LDS up to kPointsLdsValues values.  The scatter phase loops over the steps
// of its voxel; the outer tap loops stay rolled and rotate weights and offsets through scalars, the innermost row of up
// to six taps is unrolled, so every array is indexed with compile-time constants (nothing goes to scratch).
//
// The adds are no-return device-scope float atomics in the accumulator's own type (float32 / float64; the products are
// formed in fp64 and rounded once to it), straight to global memory: a 3-D order-3 voxel adds 64 cells per step, far
// below what the solve costs until there are several channels, so there is no on-chip pre-reduction.  What the atomic
// rate depends on is the shape of a wave instruction: neighbouring lanes hold neighbouring p along the LAST deformed
// axis, a smooth map puts their q next to each other along that axis too, so with dY of unit last-axis stride one tap
// turn of a wave lands on a near-contiguous run of cells (one row segment, not 64 rows).  Keep this lane-to-voxel map.
//
// A voxel that is not solved, or 'constant' and outside, loads nothing and adds nothing.  Whatever the coordinate, no
// add leaves dY: form_taps clamps every tap index to [0, O_k - 1].  Which cell receives which product is fixed by the
// call's arguments; the ORDER in which the atomics arrive is not, so the last bits of a sum may differ between calls.
#include <cstring>

#include "ed_unwarp.h"

namespace ed {

namespace {

// what the scatter phase reads (never written in the kernel: its step arrays are indexed at run time)
struct UnwarpGradView {
    IOView v;                                 // in: dY of sample 0 (deformed extents O, added into); out: dZ (extents I, read)
    int64_t in_bstride, out_bstride;
    int64_t nsrc;                             // prod I_k: the work size
};

template <int N, bool LDS>
__global__ __launch_bounds__(kUnwarpThreads) void unwarp_grad_kernel(PointsArgs a, const UnwarpGradView u)
{
    extern __shared__ double s_grid[];        // LDS: [N][ncp_0]...[ncp_{N-1}]
    int64_t o[N];
    double q[N];
    bool solved;
    if (!solve_voxel<N, LDS>(a, s_grid, u.nsrc, o, q, solved))
        return;
    // the scatter phase
    const IOView& v = u.v;
    double w[N][6];
    int64_t tap[N][6];                        // byte offsets of the taps on each deformed axis of dY
    bool constant, inside;
    form_taps<N>(a.g.out_len, v, q, solved, w, tap, constant, inside);
    if (constant)
        return;                               // an empty row of A

    const int64_t b = blockIdx.y;
    int64_t out_vox = 0;
#pragma unroll
    for (int k = 0; k < N; ++k)
        out_vox += v.out_stride[k] * o[k];
    char* in_b = const_cast<char*>(v.in) + b * u.in_bstride;
    const char* out_b = v.out + b * u.out_bstride + out_vox;
    scatter_steps<N>(v, in_b, out_b, tap, w);
}

template <int N>
hipError_t launch_unwarp_grad(const PointsArgs& a, const UnwarpGradView& u, int64_t values, int nbatch,
                              hipStream_t stream)
{
    const int64_t nblk = (u.nsrc + kUnwarpThreads - 1) / kUnwarpThreads;
    if (nblk > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk, (unsigned)nbatch);
    if (values <= kPointsLdsValues)
        hipLaunchKernelGGL((unwarp_grad_kernel<N, true>), grid, dim3(kUnwarpThreads),
                           (size_t)values * sizeof(double), stream, a, u);
    else
        hipLaunchKernelGGL((unwarp_grad_kernel<N, false>), grid, dim3(kUnwarpThreads), 0, stream, a, u);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_deform_inverse_gradient(const InverseCall& c, hipStream_t stream)
{
    const GridGeom& g = c.g;
    const int n = g.naxis;
    if (n < 1 || n > 3 || c.nbatch > 65535 || c.v.in_dtype != c.v.out_dtype ||
        (c.v.in_dtype != EDHIP_F32 && c.v.in_dtype != EDHIP_F64) || c.v.order < 0 || c.v.order > 5)
        return hipErrorNotSupported;
    UnwarpGradView u;
    memset(&u, 0, sizeof(u));
    u.v = c.v;
    u.in_bstride = c.in_bstride;
    u.out_bstride = c.out_bstride;
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
    case 1: return launch_unwarp_grad<1>(a, u, values, c.nbatch, stream);
    case 2: return launch_unwarp_grad<2>(a, u, values, c.nbatch, stream);
    default: return launch_unwarp_grad<3>(a, u, values, c.nbatch, stream);
    }
}

}  // namespace ed
