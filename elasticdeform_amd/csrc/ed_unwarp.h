// ed_unwarp.h -- what the kernels of deform_unwarp.hip (an image resampled back through the deformation), of
// deform_unwarp_grad.hip (its adjoint in the image) and of deform_unwarp_tgrad.hip (its gradient with respect to the
// deformation) share: the thread lattice with its Newton phase, the formation of the tap offsets and weights at the
// solved position, the forward's tap sum over the steps (gather_steps), its transpose (scatter_rows, scatter_steps)
// and its derivative with respect to the position (coordinate_gradient).  All three run this very code, so that the
// adjoint scatters to the cells, and with the weights, the forward gathers from, and the derivative is taken of the
// sum the forward forms.  deform_sample.hip and deform_sample_grad.hip (the deformed image at real output positions,
// and its gradients) run the same taps, sums, transpose and derivative on X at r(q): form_taps takes the extents of
// the array it samples.  Notation: the head of deform_unwarp.hip.
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

// The taps at the real position q of the array of deformed extents ext whose byte strides are v.in_stride (the unwarp
// kernels: Y, ext = GridGeom::out_len, q the solved position of a source voxel; the sample kernels: X, ext =
// GridGeom::in_len, q = r(point)): per axis the six byte offsets tap[h][.] and weights w[h][.] (a tap past the order
// repeats tap 0 with weight 0).  constant: the position takes no taps at all (not solved, or 'constant' and outside the
// array); inside: solved and 0 <= q_k <= ext_k - 1 on every axis.
template <int N>
__device__ __forceinline__ void form_taps(const int64_t (&ext)[kMaxAxes], const IOView& v, const double (&q)[N],
                                          const bool solved, double (&w)[N][6], int64_t (&tap)[N][6], bool& constant,
                                          bool& inside)
{
    // reference arithmetic (x86-64, no FMA): keep the products and sums separate
#pragma clang fp contract(off)
    const int order = v.order;
    constant = !solved;
    inside = solved;
#pragma unroll
    for (int h = 0; h < N; ++h) {
        const int64_t len = ext[h];
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

// offsets of step ss (non-deformed axes, first step axis fastest, deform.c:828-838; the same for every thread)
__device__ __forceinline__ void step_offsets(const IOView& v, int64_t ss, int64_t& in_off, int64_t& out_off)
{
    in_off = out_off = 0;
    int64_t r = ss;
    for (int l = 0; l < v.nstep; ++l) {
        const int64_t d = r / v.step_len[l];
        const int64_t c = r - d * v.step_len[l];
        in_off += v.in_step_stride[l] * c;
        out_off += v.out_step_stride[l] * c;
        r = d;
    }
}

// The forward's gather of one position: for every step (channel) the tap sum on in_b -- cval for a `constant` position
// -- stored at out_b.  Every step reuses the taps and the weights.
template <int N>
__device__ __forceinline__ void gather_steps(const IOView& v, const char* in_b, char* out_b, const int64_t (&tap)[N][6],
                                             const double (&w)[N][6], const bool constant)
{
    const int order = v.order;
    for (int64_t ss = 0; ss < v.nsteps; ++ss) {
        int64_t in_off, out_off;
        step_offsets(v, ss, in_off, out_off);
        double t = v.cval;
        if (!constant) {
            const char* base = in_b + in_off;
            switch (v.in_dtype) {
            case EDHIP_BOOL:
            case EDHIP_U8: t = tap_sum<uint8_t, N>(base, order, tap, w); break;
            case EDHIP_I8: t = tap_sum<int8_t, N>(base, order, tap, w); break;
            case EDHIP_U16: t = tap_sum<uint16_t, N>(base, order, tap, w); break;
            case EDHIP_I16: t = tap_sum<int16_t, N>(base, order, tap, w); break;
            case EDHIP_U32: t = tap_sum<uint32_t, N>(base, order, tap, w); break;
            case EDHIP_I32: t = tap_sum<int32_t, N>(base, order, tap, w); break;
            case EDHIP_U64: t = tap_sum<uint64_t, N>(base, order, tap, w); break;
            case EDHIP_I64: t = tap_sum<int64_t, N>(base, order, tap, w); break;
            case EDHIP_F32: t = tap_sum<float, N>(base, order, tap, w); break;
            default: t = tap_sum<double, N>(base, order, tap, w); break;      // float64 (the launcher admits no other)
            }
        }
        store_forward(out_b + out_off, v.out_dtype, t);
    }
}

// ---- the adjoint in the sampled array: the transposed taps -----------------------------------------------------------
// dz w_0 ... w_{N-1} added to the (order + 1)^N tap cells from deformed axis D on.  wo[k], k < D: the weight of the
// current tap on the outer axes.
template <int N, int D>
__device__ __forceinline__ void scatter_rows(char* base, int order, bool f32, const int64_t (&tap)[N][6],
                                             const double (&w)[N][6], double (&wo)[N], const double dz)
{
    if constexpr (D == N - 1) {
#pragma unroll
        for (int l = 0; l < 6; ++l) {
            if (l <= order) {
                double coeff = dz;
                if (order > 0) {
#pragma unroll
                    for (int k = 0; k < D; ++k)
                        coeff *= wo[k];
                    coeff *= w[D][l];
                }
                if (f32)
                    unsafeAtomicAdd((float*)(base + tap[D][l]), (float)coeff);
                else
                    unsafeAtomicAdd((double*)(base + tap[D][l]), coeff);
            }
        }
    } else {
        // rolled: the turn's weight and offset rotate through scalars (tap_rows)
        double w0 = w[D][0], w1 = w[D][1], w2 = w[D][2], w3 = w[D][3], w4 = w[D][4], w5 = w[D][5];
        int64_t o0 = tap[D][0], o1 = tap[D][1], o2 = tap[D][2], o3 = tap[D][3], o4 = tap[D][4], o5 = tap[D][5];
#pragma unroll 1
        for (int l = 0; l <= order; ++l) {
            wo[D] = w0;
            scatter_rows<N, D + 1>(base + o0, order, f32, tap, w, wo, dz);
            const double wr = w0;
            const int64_t orot = o0;
            w0 = w1, w1 = w2, w2 = w3, w3 = w4, w4 = w5, w5 = wr;
            o0 = o1, o1 = o2, o2 = o3, o3 = o4, o4 = o5, o5 = orot;
        }
    }
}

// The adjoint of gather_steps for one position: for every step the cotangent at out_b (float32 / float64, v.in_dtype)
// times the tap weights, ADDED into the accumulator in_b of the same dtype.
template <int N>
__device__ __forceinline__ void scatter_steps(const IOView& v, char* in_b, const char* out_b,
                                              const int64_t (&tap)[N][6], const double (&w)[N][6])
{
    const bool f32 = v.in_dtype == EDHIP_F32;
    for (int64_t ss = 0; ss < v.nsteps; ++ss) {
        int64_t in_off, out_off;
        step_offsets(v, ss, in_off, out_off);
        const double dz = f32 ? (double)*reinterpret_cast<const float*>(out_b + out_off)
                              : *reinterpret_cast<const double*>(out_b + out_off);
        double wo[N];
#pragma unroll
        for (int k = 0; k < N; ++k)
            wo[k] = 1.0;
        scatter_rows<N, 0>(in_b + in_off, v.order, f32, tap, w, wo, dz);
    }
}

// ---- the derivative with respect to the position ---------------------------------------------------------------------
// spline_weight_derivatives for a constant order, all six slots written (weights_of_order's scheme)
template <int ORDER>
__device__ __forceinline__ void weight_derivatives_of_order(double c, double scale, double (&dw)[6])
{
    double tmp[ORDER + 1];
    spline_weight_derivatives(c, ORDER, tmp);
#pragma unroll
    for (int l = 0; l < 6; ++l)
        dw[l] = l <= ORDER ? tmp[l <= ORDER ? l : 0] * scale : 0.0;
}
__device__ __forceinline__ void weight_derivatives_by_order(double c, int order, double scale, double (&dw)[6])
{
    switch (order) {
    case 1: weight_derivatives_of_order<1>(c, scale, dw); break;
    case 2: weight_derivatives_of_order<2>(c, scale, dw); break;
    case 3: weight_derivatives_of_order<3>(c, scale, dw); break;
    case 4: weight_derivatives_of_order<4>(c, scale, dw); break;
    case 5: weight_derivatives_of_order<5>(c, scale, dw); break;
    default:                                  // order 0: the weight is constant
#pragma unroll
        for (int l = 0; l < 6; ++l)
            dw[l] = 0.0;
        break;
    }
}

// sum_step dZ[step] * (the forward's tap sum with the weights w) over every step of the position
template <int N>
__device__ __forceinline__ double step_sums(const IOView& v, const char* in_b, const char* out_b,
                                            const int64_t (&tap)[N][6], const double (&w)[N][6])
{
    const bool f32 = v.in_dtype == EDHIP_F32;
    double acc = 0.0;
    for (int64_t ss = 0; ss < v.nsteps; ++ss) {
        int64_t in_off, out_off;
        step_offsets(v, ss, in_off, out_off);
        double dz, t;
        if (f32) {
            dz = (double)*reinterpret_cast<const float*>(out_b + out_off);
            t = tap_sum<float, N>(in_b + in_off, v.order, tap, w);
        } else {
            dz = *reinterpret_cast<const double*>(out_b + out_off);
            t = tap_sum<double, N>(in_b + in_off, v.order, tap, w);
        }
        acc += dz * t;
    }
    return acc;
}

// g = dL/dq of a position that takes taps (not `constant`): one deformed axis h at a time the forward's rolled tap sum
// over every step with row h of the weights replaced by w'_h m'_h (N sums per step instead of one sum with both weight
// sets live: the register peak stays the front's, and the N-fold loads hit L1 / L2), all in fp64.  ext, q, tap and w
// are form_taps' arguments and results; w is left as it was.
template <int N>
__device__ __forceinline__ void coordinate_gradient(const int64_t (&ext)[kMaxAxes], const IOView& v,
                                                    const double (&q)[N], const char* in_b, const char* out_b,
                                                    const int64_t (&tap)[N][6], double (&w)[N][6], double (&g)[N])
{
#pragma unroll
    for (int h = 0; h < N; ++h) {
        double keep[6];
#pragma unroll
        for (int l = 0; l < 6; ++l)
            keep[l] = w[h][l];
        // (the coordinate form_taps took its window and weights at: not 'constant' outside, so it is m_h itself)
        const double m = map_coordinate(q[h], ext[h], v.mode);
        weight_derivatives_by_order(m, v.order, map_coordinate_slope(q[h], ext[h], v.mode), w[h]);
        g[h] = step_sums<N>(v, in_b, out_b, tap, w);
#pragma unroll
        for (int l = 0; l < 6; ++l)
            w[h][l] = keep[l];
    }
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
