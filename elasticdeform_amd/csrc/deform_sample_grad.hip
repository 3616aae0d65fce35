// deform_sample_grad.hip -- the gradients of deform_sample.hip (edhip_deform_sample_gradient): with respect to the image
// and with respect to the coordinate the image is sampled at.
//
// The forward is V[i, step] = S_X(r(q_i))[step].  For fixed positions and deformation and cval = 0 it is linear in X:
// V[i, s] = sum_j A[i, j] X[j, s], the row A[i, :] holding the (order + 1)^N products of tap weights at r(q_i) (taps
// the mirror edge rule folds onto one cell add up), empty where the position is not sane or where the mode is
// 'constant' and r lies outside X.  For L = sum_{i, step} dV[i, step] V[i, step] the kernel leaves, either or both:
//   dinput       A^T dV ADDED into the accumulator: per point and step, dV[i, s] w_0 ... w_{N-1} into every tap cell of
//                the point (scatter_rows of ed_unwarp.h: products in fp64, rounded once, no-return device-scope float
//                atomics in the accumulator's own type).  Which cell receives which product is fixed by the call's
//                arguments; the ORDER in which the atomics arrive is not, so the last bits of a sum may differ between
//                calls.  The caller zeroes the accumulator in front and applies the transposed prefilter behind.
//   dcoordinate  g_h(i) = sum_step dV[i, step] m'_h sum_k C[k, step] w'_h(m_h, k_h) prod_{e != h} w_e(m_e, k_e) = dL/dr_h
//                (C: the coefficients of X; m_h = map_coordinate(r_h, I_h, mode), m'_h its slope: 0 where 'nearest'
//                clamps; w' the one-sided derivative of the chosen window at a window change), one deformed axis at a
//                time with the forward's rolled tap sum (coordinate_gradient of ed_unwarp.h, the code of
//                unwarp_tgrad_prepare), stored as an fp64 row per point.  A row depends on its point alone: the same
//                bits on every call, for a sample of a batch and for any slice or permutation of the points.  Zeros
//                for a point that contributes nothing, and exact zeros at order 0.
// The gradients with respect to the positions, the control grid and the inverse map follow from g by
// edhip_deform_points_gradient(inverse = 0) with g as the cotangent: its 64-bit fixed-point sums are not restated here.
//
// The front (staging, grid-stride loop over the points, eval_map, the sane flag) and the taps are the forward's own
// code (ed_sample.h, ed_unwarp.h), so the adjoint scatters to the cells, and with the weights, the forward gathers
// from, and the derivative is taken of the sum the forward forms.  The two parts of a point run one after the other on
// the same registers: the taps are formed for the accumulator's strides, scattered, and formed again for the strides
// of X.  Whatever the coordinate, no add and no load leaves the arrays: form_taps clamps every tap index.
#include "ed_sample.h"

namespace ed {

namespace {

struct SampleGradView {
    SampleView s;                             // s.v.in: the coefficients of X, or nullptr; s.v.out: dV
    IOView acc;                               // acc.in: the accumulator (X's shape), or nullptr; acc.out: dV
    int64_t acc_bstride;
    char* dcoord;                             // float64 (npts, naxis), or nullptr
    int64_t dcoord_stride[2], dcoord_bstride;
};

template <int N, bool LDS>
__global__ __launch_bounds__(kPointsThreads) void sample_grad_kernel(PointsArgs a, const SampleGradView t)
{
    extern __shared__ double s_grid[];        // LDS: [N][ncp_0]...[ncp_{N-1}]
    SampleFront<N> f;
    sample_front<N, LDS>(a, s_grid, f);
    const int64_t b = blockIdx.y;
    const IOView& v = t.s.v;

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts;
         i += (int64_t)gridDim.x * blockDim.x) {
        double r[N];
        const bool sane = sample_point<N, LDS>(a, s_grid, f, b, i, r);
        const char* out_b = v.out + b * t.s.out_bstride + i * v.out_stride[0];
        double w[N][6];
        int64_t tap[N][6];
        bool constant, inside;
        if (t.acc.in && sane) {
            // the adjoint in X: the transposed taps on the accumulator's strides
            form_taps<N>(a.g.in_len, t.acc, r, true, w, tap, constant, inside);
            if (!constant)
                scatter_steps<N>(t.acc, const_cast<char*>(t.acc.in) + b * t.acc_bstride, out_b, tap, w);
        }
        if (t.dcoord) {
            double g[N];
#pragma unroll
            for (int h = 0; h < N; ++h)
                g[h] = 0.0;
            if (sane && v.order > 0) {
                form_taps<N>(a.g.in_len, v, r, true, w, tap, constant, inside);
                if (!constant)
                    coordinate_gradient<N>(a.g.in_len, v, r, v.in + b * t.s.in_bstride, out_b, tap, w, g);
            }
            char* dst = t.dcoord + b * t.dcoord_bstride + i * t.dcoord_stride[0];
#pragma unroll
            for (int h = 0; h < N; ++h)
                *(double*)(dst + h * t.dcoord_stride[1]) = g[h];
        }
    }
}

template <int N>
hipError_t launch_sample_grad(const PointsArgs& a, const SampleGradView& t, int64_t values, int nbatch,
                              hipStream_t stream)
{
    const dim3 grid = points_grid(a.npts, nbatch);
    if (values <= kPointsLdsValues)
        hipLaunchKernelGGL((sample_grad_kernel<N, true>), grid, dim3(kPointsThreads), (size_t)values * sizeof(double),
                           stream, a, t);
    else
        hipLaunchKernelGGL((sample_grad_kernel<N, false>), grid, dim3(kPointsThreads), 0, stream, a, t);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_deform_sample_gradient(const SampleCall& c, const IOView& acc, int64_t acc_bstride,
                                         const BatchArray& dcoord, hipStream_t stream)
{
    if ((!acc.in && !dcoord.ptr) || (dcoord.ptr && !c.v.in) || (acc.in && acc.in_dtype != c.v.out_dtype))
        return hipErrorInvalidValue;
    PointsArgs a;
    SampleGradView t;
    memset(&t, 0, sizeof(t));
    int64_t values = 0;
    bool launch;
    const hipError_t e = fill_sample_args(c, true, a, t.s, values, &launch);
    if (e != hipSuccess || !launch)
        return e;
    t.acc = acc;
    t.acc_bstride = acc_bstride;
    unpack(dcoord, t.dcoord, t.dcoord_stride, t.dcoord_bstride);
    switch (c.g.naxis) {
    case 1: return launch_sample_grad<1>(a, t, values, c.nbatch, stream);
    case 2: return launch_sample_grad<2>(a, t, values, c.nbatch, stream);
    default: return launch_sample_grad<3>(a, t, values, c.nbatch, stream);
    }
}

}  // namespace ed
