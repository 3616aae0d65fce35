// deform_unwarp_tgrad.hip -- the gradient of deform_unwarp.hip with respect to the deformation: the prefiltered control
// grid P and the inverse map K (edhip_deform_inverse_transform_gradient).
//
// The forward is Z[p, step] = S_Y(q(p))[step] with r(q(p)) = p.  For L = sum_{p, step} dZ[p, step] Z[p, step], per
// source voxel p with solved q = q(p):
//   g_h(p) = sum_step dZ[p, step] m'_h sum_k C[k, step] w'_h(m_h, k_h) prod_{e != h} w_e(m_e, k_e)      dL/dq_h
// (C: the coefficients of Y, extents O; m_h = map_coordinate(q_h, O_h, mode), m'_h its slope; w, w' the tap weights
// and their derivatives on the window form_taps picks: the g_h of deform_dgrad.hip, on Y at q instead of on X at c(o)),
// and by the implicit function theorem at the solved q (r(q) = p holds for every P and K),
//   u(p) = -J(q)^-T g(p)                J = dr/dq (eval_map)
//   dP[h, j] = sum_p u_h(p) beta(q(p), j)     dK[h, l < n] = sum_p u_h(p) q_l(p)     dK[h, n] = sum_p u_h(p)
// which are the sums of deform_points_grad.hip for the inverse direction, with g in the place of the cotangent.
//
// unwarp_tgrad_prepare is the per-voxel part: the lattice, the Newton phase and the taps are the forward's own code
// (ed_unwarp.h: solve_voxel, form_taps, tap_sum), so q, the taps and the weights are the forward's bits.  One thread
// per source voxel (extents I), last deformed axis fastest, 256 threads, blockIdx.y = sample, the control grid in LDS
// up to kPointsLdsValues values.  After the solve the thread
//   * takes, one deformed axis h at a time, the forward's rolled tap sum over every step with row h of the weights
//     replaced by w'_h m'_h (N sums per step instead of one sum with both weight sets live: the register peak stays
//     the Newton phase's, and the N-fold loads hit L1 / L2), all in fp64 (float32 is widened at the load);
//   * evaluates J at q and solves J^T s = g, exactly as points_grad_prepare does for its inverse direction (a finite
//     right-hand side tells a singular J from a non-finite cotangent);
//   * stores u = -s and q as fp64 rows of the call's scratch (ed_points_grad.h), zeros for a voxel that contributes
//     nothing: not solved, 'constant' and outside Y (Z = cval there), a position that is not sane, a singular J;
//   * takes part in the wave reductions of the sample's head (publish_head): max|u|, max|q|, the non-finite flag, the
//     number of contributing voxels.  Lanes past the lattice take part with zeros: they do not return after
//     solve_voxel.
// points_grad_clear in front, points_grad_scatter and points_grad_finish behind (deform_points_grad.hip) turn the rows
// into dP and dK by the fixed-point reduction of ed_points_grad.h, its rule of the two maxima: the results do not depend
// on the order in which the voxels arrive -- a repeated call, a sample of a batch and a graph replay give the same bits.
// Where 'nearest' clamps an axis its slope is 0; at a window change (order 1 at integer q_h) the derivative is the
// one-sided one of spline_weight_derivatives.  Order 0 is piecewise constant: nothing but clear and finish runs, the
// results are zeros.
#include <cmath>
#include <cstring>

#include "ed_points_grad.h"
#include "ed_unwarp.h"

namespace ed {

namespace {

// what the gather phase reads and where the rows go (never written in the kernel)
struct UnwarpTgradView {
    IOView v;                                 // in: the coefficients of Y, sample 0 (extents O); out: dZ (extents I, read)
    int64_t in_bstride, out_bstride;
    int64_t nsrc;                             // prod I_k: the work size, and the rows per sample
    unsigned long long* head;                 // per sample kGradHead words
    double* u;                                // per sample (nsrc, N)
    double* q;                                // per sample (nsrc, N)
};

template <int N, bool LDS>
__global__ __launch_bounds__(kUnwarpThreads) void unwarp_tgrad_prepare(PointsArgs a, const UnwarpTgradView t)
{
    extern __shared__ double s_grid[];        // LDS: [N][ncp_0]...[ncp_{N-1}]
    int64_t o[N];
    double q[N];
    bool solved = false;
#pragma unroll
    for (int h = 0; h < N; ++h) {
        o[h] = 0;
        q[h] = 0.0;
    }
    // a lane past the lattice stays: it takes part in the wave reductions below, with zeros
    const bool live = solve_voxel<N, LDS>(a, s_grid, t.nsrc, o, q, solved);
    const IOView& v = t.v;
    const int64_t b = blockIdx.y;
    bool contributes = live && solved;
    double u[N];
#pragma unroll
    for (int h = 0; h < N; ++h)
        u[h] = 0.0;
    bool cfinite = true;

    if (contributes) {
        // the gather phase: g = dL/dq, one axis at a time
        double w[N][6];
        int64_t tap[N][6];                    // byte offsets of the taps on each deformed axis of Y
        bool constant, inside;
        form_taps<N>(a.g.out_len, v, q, true, w, tap, constant, inside);
        contributes = !constant && sane_position<N>(a, q);
        if (contributes) {
            int64_t out_vox = 0;
#pragma unroll
            for (int k = 0; k < N; ++k)
                out_vox += v.out_stride[k] * o[k];
            const char* in_b = v.in + b * t.in_bstride;
            const char* out_b = v.out + b * t.out_bstride + out_vox;
            double g[N];
            coordinate_gradient<N>(a.g.out_len, v, q, in_b, out_b, tap, w, g);
#pragma unroll
            for (int h = 0; h < N; ++h)
                cfinite = cfinite && isfinite(g[h]);
            // u = -J^-T g at the solved q (points_grad_prepare, inverse direction)
            int64_t tstride[N];
            int per = 0;
            if constexpr (LDS) {
                int64_t cs = 1;
#pragma unroll
                for (int k = N - 1; k >= 0; --k) {
                    tstride[k] = cs;
                    cs *= a.g.ncp[k];
                }
                per = (int)cs;
            } else {
#pragma unroll
                for (int k = 0; k < N; ++k)
                    tstride[k] = a.g.disp_stride[k + 1];
            }
            double r[N], J[N][N];
            if constexpr (LDS)
                eval_map<N>(a, LdsGrid{s_grid, per}, tstride, q, r, J);
            else
                eval_map<N>(a, GlobalGrid{a.g.disp, a.g.disp_stride[0], a.g.disp_dtype}, tstride, q, r, J);
            // A singular or non-finite J: the voxel contributes nothing; whether J is usable is asked with a finite
            // right-hand side, so that a non-finite cotangent is told apart from it
            double JT[N][N], rhs[N], s[N];
#pragma unroll
            for (int h = 0; h < N; ++h) {
                rhs[h] = cfinite ? g[h] : 1.0;
#pragma unroll
                for (int l = 0; l < N; ++l)
                    JT[h][l] = J[l][h];
            }
            contributes = solve<N>(JT, rhs, s);
#pragma unroll
            for (int h = 0; h < N; ++h)
                u[h] = cfinite ? -s[h] : NAN;
        }
    }

    double maxu = 0.0, maxq = 0.0;
    unsigned long long count = 0ull;          // contributing voxels
    bool bad = false;
    if (!contributes) {
#pragma unroll
        for (int h = 0; h < N; ++h)
            u[h] = q[h] = 0.0;
    } else if (!cfinite) {
        bad = true;
    } else {
        count = 1ull;
#pragma unroll
        for (int h = 0; h < N; ++h) {
            maxu = fabs(u[h]) > maxu ? fabs(u[h]) : maxu;
            maxq = fabs(q[h]) > maxq ? fabs(q[h]) : maxq;
        }
    }
    if (live) {
        const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x + b * t.nsrc) * N;
#pragma unroll
        for (int h = 0; h < N; ++h) {
            t.u[row + h] = u[h];
            t.q[row + h] = q[h];
        }
    }
    publish_head(t.head + b * kGradHead, maxu, maxq, bad, count);
}

template <int N>
hipError_t launch_unwarp_tgrad(const PointsArgs& a, const UnwarpTgradView& t, int64_t values, int nbatch,
                               hipStream_t stream)
{
    const int64_t nblk = (t.nsrc + kUnwarpThreads - 1) / kUnwarpThreads;
    if (nblk > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk, (unsigned)nbatch);
    if (values <= kPointsLdsValues)
        hipLaunchKernelGGL((unwarp_tgrad_prepare<N, true>), grid, dim3(kUnwarpThreads),
                           (size_t)values * sizeof(double), stream, a, t);
    else
        hipLaunchKernelGGL((unwarp_tgrad_prepare<N, false>), grid, dim3(kUnwarpThreads), 0, stream, a, t);
    return hipGetLastError();
}

int64_t lattice_size(const GridGeom& g)
{
    int64_t nsrc = 1;
    for (int k = 0; k < g.naxis; ++k)
        nsrc *= g.in_len[k];
    return nsrc;
}

}  // namespace

size_t inverse_tgrad_scratch_bytes(const GridGeom& g, int nbatch)
{
    return (size_t)nbatch * (size_t)(kGradHead + points_grad_cells_per(g) + 2 * lattice_size(g) * g.naxis) * 8;
}

hipError_t launch_deform_inverse_transform_gradient(const InverseCall& c, const BatchArray& ddisp, const BatchArray& dK,
                                                    char* scratch, hipStream_t stream)
{
    const GridGeom& g = c.g;
    const int n = g.naxis;
    if (n < 1 || n > 3 || c.nbatch > 65535 || c.v.in_dtype != c.v.out_dtype ||
        (c.v.in_dtype != EDHIP_F32 && c.v.in_dtype != EDHIP_F64) || c.v.order < 0 || c.v.order > 5)
        return hipErrorNotSupported;
    for (int k = 0; k < n; ++k)
        if (g.in_len[k] < 2 || g.out_len[k] < 1)
            return hipErrorInvalidValue;
    if (c.nbatch <= 0 || (!ddisp.ptr && !dK.ptr))
        return hipSuccess;                    // nothing to launch
    const int64_t nsrc = lattice_size(g);
    // order 0 (or no step at all): no row is written and none is read -- clear and finish leave exact zeros
    const bool rows = c.v.order > 0 && nsrc > 0 && c.v.nsteps > 0;

    UnwarpTgradView t;
    memset(&t, 0, sizeof(t));
    t.v = c.v;
    t.in_bstride = c.in_bstride;
    t.out_bstride = c.out_bstride;
    t.nsrc = nsrc;
    t.head = (unsigned long long*)scratch;
    t.u = (double*)(t.head + (size_t)c.nbatch * (size_t)(kGradHead + points_grad_cells_per(g)));
    t.q = t.u + (size_t)c.nbatch * (size_t)nsrc * n;

    // the reduction reads the rows as the points gradient reads its positions: q from `pos`, no status
    PointsGradCall p;
    memset(&p, 0, sizeof(p));
    p.g = g;
    p.inverse = 1;
    p.nbatch = c.nbatch;
    p.npts = rows ? nsrc : 0;
    p.disp_bstride = c.disp_bstride;
    p.pos.ptr = (char*)t.q;
    p.pos.dtype = EDHIP_F64;
    p.pos.stride[0] = (int64_t)n * 8;
    p.pos.stride[1] = 8;
    p.pos.bstride = nsrc * n * 8;
    p.ddisp = ddisp;
    p.dK = dK;
    p.scratch = scratch;

    hipError_t e = launch_points_grad_clear(g, c.nbatch, scratch, stream);
    if (e != hipSuccess)
        return e;
    if (rows) {
        PointsArgs a;
        memset(&a, 0, sizeof(a));
        const int64_t values = fill_points_args(a, g, c.disp_bstride, c.forward_linear, c.max_iter, c.tol);
        switch (n) {
        case 1: e = launch_unwarp_tgrad<1>(a, t, values, c.nbatch, stream); break;
        case 2: e = launch_unwarp_tgrad<2>(a, t, values, c.nbatch, stream); break;
        default: e = launch_unwarp_tgrad<3>(a, t, values, c.nbatch, stream); break;
        }
        if (e != hipSuccess)
            return e;
    }
    return launch_points_grad_reduce(p, stream);
}

}  // namespace ed
