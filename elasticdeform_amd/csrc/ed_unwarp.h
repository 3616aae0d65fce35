// ed_unwarp.h -- what the kernels of deform_unwarp.hip (an image resampled back through the deformation), of
// deform_unwarp_grad.hip (its adjoint in the image) and of deform_unwarp_tgrad.hip (its gradient with respect to the
// deformation) share: the thread lattice with its Newton phase, the formation of the tap offsets and weights at the
// solved position, and the forward's tap sum.  All three run this very code, so that the adjoint scatters to the
// cells, and with the weights, the forward gathers from, and the derivative is taken of the sum the forward forms.
// Notation: the head of deform_unwarp.hip.
#pragma once

#include "ed_device.h"
#include "ed_exact_coord.h"
#include "ed_params.h"
#include "ed_points.h"

namespace ed {

namespace {

constexpr int kUnwarpThreads = 256;

// spline_weights for a constant order; every order writes all six slots (zeros past the order), so that no store to
// w is ever indexed by the order at run time
template <int ORDER>
__device__ __forceinline__ void weights_of_order(double c, double (&w)[6])
{
    double tmp[ORDER + 1];
    spline_weights(c, ORDER, tmp);
#pragma unroll
    for (int l = 0; l < 6; ++l)
        w[l] = l <= ORDER ? tmp[l <= ORDER ? l : 0] : 0.0;
}
__device__ __forceinline__ void weights_by_order(double c, int order, double (&w)[6])
{
    switch (order) {
    case 1: weights_of_order<1>(c, w); break;
    case 2: weights_of_order<2>(c, w); break;
    case 3: weights_of_order<3>(c, w); break;
    case 4: weights_of_order<4>(c, w); break;
    case 5: weights_of_order<5>(c, w); break;
    default:                                  // order 0: one tap, no weight
#pragma unroll
        for (int l = 0; l < 6; ++l)
            w[l] = 0.0;
        break;
    }
}

// The taps of source voxel p at its solved position q, on the array of deformed extents g.out_len whose byte strides
// are v.in_stride: per axis the six byte offsets tap[h][.] and weights w[h][.] (a tap past the order repeats tap 0 with
// weight 0).  constant: the voxel takes no taps at all (not solved, or 'constant' and outside the array); inside:
// solved and 0 <= q_k <= O_k - 1 on every axis.
template <int N>
__device__ __forceinline__ void form_taps(const GridGeom& g, const IOView& v, const double (&q)[N], const bool solved,
                                          double (&w)[N][6], int64_t (&tap)[N][6], bool& constant, bool& inside)
{
    // reference arithmetic (x86-64, no FMA): keep the products and sums separate
#pragma clang fp contract(off)
    const int order = v.order;
    constant = !solved;
    inside = solved;
#pragma unroll
    for (int h = 0; h < N; ++h) {
        const int64_t len = g.out_len[h];
        const double qh = solved ? q[h] : 0.0;
        inside = inside && qh >= 0.0 && qh <= (double)(len - 1);
        // boundary map, window and weights as deform_exact.hip has them (deform.c:768-824)
        const double cc = map_coordinate(qh, len, v.mode);
        const bool in = cc > -1.0;
        constant = constant || !in;           // 'constant' outside the array (or a NaN coordinate): cval
        const double c = in ? cc : 0.0;       // (a voxel that takes cval forms taps inside the array and loads nothing)
        const int64_t start = window_start(c, order);
        // (a tap past the order repeats tap 0: the row loads below need no branch, and its value is never added)
        if (start < 0 || start + order >= len) {
            int64_t first = 0;
#pragma unroll
            for (int l = 0; l < 6; ++l) {
                int64_t idx = mirror_index(start + l, len);
                // no access leaves the array, whatever the coordinate (no effect on a coordinate the boundary map produced)
                idx = idx < 0 ? 0 : (idx > len - 1 ? len - 1 : idx);
                if (l == 0)
                    first = idx;
                tap[h][l] = (l <= order ? idx : first) * v.in_stride[h];
            }
        } else {
#pragma unroll
            for (int l = 0; l < 6; ++l)
                tap[h][l] = (l <= order ? start + l : start) * v.in_stride[h];
        }
        weights_by_order(c, order, w[h]);
    }
}

// The (order + 1)^N taps from deformed axis D on, added to t in the reference's order.  wo[k], k < D: the weight of
// the current tap on the outer axes.  S: the element type (its conversion to double is the plain C one).
template <typename S, int N, int D>
__device__ __forceinline__ void tap_rows(const char* base, int order, const int64_t (&tap)[N][6],
                                         const double (&w)[N][6], double (&wo)[N], double& t)
{
    // reference arithmetic (x86-64, no FMA): keep the products and sums separate
#pragma clang fp contract(off)
    if constexpr (D == N - 1) {
        S val[6];
#pragma unroll
        for (int l = 0; l < 6; ++l)           // (taps past the order repeat tap 0: no branch around a load)
            val[l] = *reinterpret_cast<const S*>(base + tap[D][l]);
#pragma unroll
        for (int l = 0; l < 6; ++l) {
            if (l <= order) {
                double coeff = (double)val[l];
                if (order > 0) {
#pragma unroll
                    for (int k = 0; k < D; ++k)
                        coeff *= wo[k];
                    coeff *= w[D][l];
                }
                t += coeff;
            }
        }
    } else {
        // rolled: the turn's weight and offset rotate through scalars (deform_points.hip: grid_taps)
        double w0 = w[D][0], w1 = w[D][1], w2 = w[D][2], w3 = w[D][3], w4 = w[D][4], w5 = w[D][5];
        int64_t o0 = tap[D][0], o1 = tap[D][1], o2 = tap[D][2], o3 = tap[D][3], o4 = tap[D][4], o5 = tap[D][5];
#pragma unroll 1
        for (int l = 0; l <= order; ++l) {
            wo[D] = w0;
            tap_rows<S, N, D + 1>(base + o0, order, tap, w, wo, t);
            const double wr = w0;
            const int64_t orot = o0;
            w0 = w1, w1 = w2, w2 = w3, w3 = w4, w4 = w5, w5 = wr;
            o0 = o1, o1 = o2, o2 = o3, o3 = o4, o4 = o5, o5 = orot;
        }
    }
}

template <typename S, int N>
__device__ __forceinline__ double tap_sum(const char* base, int order, const int64_t (&tap)[N][6],
                                          const double (&w)[N][6])
{
    double t = 0.0;
    double wo[N];
#pragma unroll
    for (int k = 0; k < N; ++k)
        wo[k] = 1.0;
    tap_rows<S, N, 0>(base, order, tap, w, wo, t);
    return t;
}

// The front of the kernels: this sample's control grid (staged in s_grid with LDS), the source voxel o of the thread
// (extents I, last deformed axis fastest) and the Newton phase, q with r(q) = o.  false: the thread is past the
// lattice (it has taken part in the staging barrier) and returns.
template <int N, bool LDS>
__device__ __forceinline__ bool solve_voxel(PointsArgs& a, double* s_grid, const int64_t nsrc, int64_t (&o)[N],
                                            double (&q)[N], bool& solved)
{
    a.g.disp += (int64_t)blockIdx.y * a.disp_bstride;     // this sample's control grid
    const GridGeom& g = a.g;
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
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= nsrc)
        return false;
    // source voxel index (extents I), last deformed axis fastest
    {
        int64_t r = tid;
#pragma unroll
        for (int k = N - 1; k >= 0; --k) {
            const int64_t d = r / g.in_len[k];
            o[k] = r - d * g.in_len[k];
            r = d;
        }
    }
    // the Newton phase: q with r(q) = p
    double p[N];
#pragma unroll
    for (int h = 0; h < N; ++h) {
        p[h] = (double)o[h];
        q[h] = 0.0;
    }
    if constexpr (LDS)
        solved = invert_map<N>(a, LdsGrid{s_grid, per}, tstride, p, q);
    else
        solved = invert_map<N>(a, GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, tstride, p, q);
    return true;
}

}  // namespace

}  // namespace ed
