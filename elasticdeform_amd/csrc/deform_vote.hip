// deform_vote.hip -- label-aware linear resampling of label maps (edhip_deform_labels).
//
// For every output voxel the 2^n order-1 interpolation weights are summed per distinct label among the 2^n source
// voxels and the label with the largest sum is stored (on a tie the numerically smallest label); optionally the
// winning sum, rounded once to float32.  That is, class by class, the argmax over
//   s_c = deform_grid((L == c) as float64, order = 1, cval = 1.0 if c == cval else 0.0)
// without the one-hot volumes -- and bit for bit, ties included: a one-hot channel's reference value is the sum, in
// the reference's tap order (lexicographic, last axis fastest), of 1.0 * w_0 * ... * w_{n-1} over the taps that carry
// the label plus exact zeros, and this kernel forms the same products in the same axis order, adds the products of
// equal-label taps in the same tap order, and takes the coordinate from the reference-order evaluation
// (ed_exact_coord.h).  Compiled with -ffp-contract=off like deform_exact.hip.
//
// One thread per (output voxel, step), last deformed axis fastest, blockIdx.y = sample.  The prefiltered control grid
// is staged in LDS as doubles up to kPointsLdsValues values and read from global memory beyond.  The vote indexes its
// arrays with compile-time constants only (nothing goes to scratch): for tap i, total_i = sum_j [l_j == l_i] p_j with
// j in tap order -- 2^n x 2^n selects.  No workspace, no atomics, no synchronisation beyond the staging barrier: a
// voxel's result depends on the call's arguments alone.
#include <cstring>

#include "ed_device.h"
#include "ed_exact_coord.h"
#include "ed_params.h"

namespace ed {

namespace {

constexpr int kVoteThreads = 256;

struct VoteArgs {
    GridGeom g;                               // g.disp: the prefiltered grid of sample 0
    IOView v;                                 // in / out: the label maps of sample 0 (order and cval unused)
    int64_t in_bstride, out_bstride, disp_bstride, w_bstride;
    char* weight;                             // float32, the output's shape, or nullptr
    int64_t w_stride[3];
    int64_t w_step_stride[kMaxSteps];
    uint64_t cval_bits;                       // cval in the label type (two's complement, low bytes)
};

// the control grid as displacement3 reads it: doubles in LDS (stage_grid_lds: component-major, C order) or the
// caller's array
struct LdsTaps {
    typedef int Off;                          // tap offsets: elements of the LDS copy
    const double* s;
    int per;
    int stride[3];
    __device__ __forceinline__ double operator()(int h, int off) const { return s[h * per + off]; }
};
struct GlobalTaps {
    typedef int64_t Off;                      // bytes of the caller's array
    const char* base;
    int64_t hstride;
    int dtype;
    int64_t stride[3];
    __device__ __forceinline__ double operator()(int h, int64_t off) const
    {
        return load_as_double(base + h * hstride + off, dtype);
    }
};

// eval_displacement / eval_displacement_lds for three axes with the same values, products and order of the sums
// (value, then * w_0, * w_1, * w_2, then added; taps lexicographic, last axis fastest), hence the same bits -- but
// the outermost of the three tap loops stays rolled and the two inner ones are unrolled, so that no register array is
// indexed at run time.  The helpers' partly unrolled 64-tap loop indexes its weights and offsets with the loop
// counter, which puts them into scratch; unrolled completely, the compiler issues every grid read in front of the
// arithmetic and takes every register there is (deform_points.hip: grid_taps).  The turn's weight and offset rotate
// through scalars: a select on the loop counter is turned back into an indexed read.
template <typename Grid>
__device__ __forceinline__ void displacement3(const GridGeom& g, const Grid& grid, const int64_t* o, double* displ)
{
    // reference arithmetic (x86-64, no FMA): keep the products and sums separate
#pragma clang fp contract(off)
    double dw[3][4];
    typename Grid::Off dtap[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double cp = control_coordinate(g.ncp[k], o[k] + g.off[k], g.in_len[k]);
        const int64_t start = window_start(cp, 3);
        const bool edge = start < 0 || start + 3 >= g.ncp[k];
#pragma unroll
        for (int l = 0; l < 4; ++l)
            dtap[k][l] = (typename Grid::Off)((edge ? mirror_index(start + l, g.ncp[k]) : start + l) * grid.stride[k]);
        spline_weights(cp, 3, dw[k]);
    }
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        double acc = 0.0;
        double w0 = dw[0][0], w1 = dw[0][1], w2 = dw[0][2], w3 = dw[0][3];
        typename Grid::Off o0 = dtap[0][0], o1 = dtap[0][1], o2 = dtap[0][2], o3 = dtap[0][3];
#pragma unroll 1
        for (int t0 = 0; t0 < 4; ++t0) {
#pragma unroll
            for (int t1 = 0; t1 < 4; ++t1) {
#pragma unroll
                for (int t2 = 0; t2 < 4; ++t2) {
                    double coeff = grid(h, o0 + dtap[1][t1] + dtap[2][t2]);
                    coeff *= w0;
                    coeff *= dw[1][t1];
                    coeff *= dw[2][t2];
                    acc += coeff;
                }
            }
            const double wr = w0;
            const typename Grid::Off orot = o0;
            w0 = w1, w1 = w2, w2 = w3, w3 = wr;
            o0 = o1, o1 = o2, o2 = o3, o3 = orot;
        }
        displ[h] = acc;
    }
}

template <int N, typename S, bool LDS>
__global__ __launch_bounds__(kVoteThreads) void deform_vote_kernel(const VoteArgs a)
{
    // reference arithmetic (x86-64, no FMA): keep the products and sums separate
#pragma clang fp contract(off)
    extern __shared__ double sgrid[];         // LDS: [N][ncp_0]...[ncp_{N-1}]
    const int64_t b = blockIdx.y;
    // (a copy of the geometry alone: it is indexed with constants only and stays in registers, where a write into the
    // argument block would move all of it, the runtime-indexed step arrays included, into scratch)
    GridGeom g = a.g;
    g.disp += b * a.disp_bstride;             // this sample's control grid
    const IOView& v = a.v;
    int per = 0;
    if constexpr (LDS) {
        per = stage_grid_lds<N>(g, sgrid);
        __syncthreads();
    }
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= g.nvox * v.nsteps)
        return;
    int64_t kk, ss;
    if (v.steps_fastest) {
        kk = tid / v.nsteps;
        ss = tid - kk * v.nsteps;
    } else {
        ss = tid / g.nvox;
        kk = tid - ss * g.nvox;
    }
    // output voxel index, last deformed axis fastest
    int64_t o[N];
    {
        int64_t r = kk;
#pragma unroll
        for (int k = N - 1; k >= 0; --k) {
            const int64_t q = r / g.out_len[k];
            o[k] = r - q * g.out_len[k];
            r = q;
        }
    }
    double displ[N];
    if constexpr (N == 3) {
        if constexpr (LDS)
            displacement3(g, LdsTaps{sgrid, per, {(int)(g.ncp[1] * g.ncp[2]), (int)g.ncp[2], 1}}, o, displ);
        else
            displacement3(g, GlobalTaps{g.disp, g.disp_stride[0], g.disp_dtype,
                                        {g.disp_stride[1], g.disp_stride[2], g.disp_stride[3]}}, o, displ);
    } else if constexpr (LDS) {
        eval_displacement_lds<N>(g, sgrid, per, o, displ);
    } else {
        eval_displacement<N>(g, o, displ);
    }

    // source coordinate, boundary map, window and order-1 weights as deform_exact.hip has them (deform.c:768-824)
    double w[N][2];
    int64_t tap[N][2];                        // byte offsets of the two taps on each deformed input axis
    bool constant = false;
#pragma unroll
    for (int h = 0; h < N; ++h) {
        const double cc = map_coordinate(raw_coordinate<N>(g, o, h, displ[h]), g.in_len[h], v.mode);
        const bool inside = cc > -1.0;
        constant = constant || !inside;       // 'constant' outside the array (or a NaN coordinate): cval, weight 1
        const double c = inside ? cc : 0.0;   // (a voxel that takes cval still loads: from taps inside the array)
        const int64_t start = window_start(c, 1);
        const bool edge = start < 0 || start + 1 >= g.in_len[h];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            int64_t idx = edge ? mirror_index(start + l, g.in_len[h]) : start + l;
            // no load leaves the array, whatever the coordinate (no effect on a coordinate the boundary map produced)
            idx = idx < 0 ? 0 : (idx > g.in_len[h] - 1 ? g.in_len[h] - 1 : idx);
            tap[h][l] = idx * v.in_stride[h];
        }
        spline_weights(c, 1, w[h]);
    }

    // step (non-deformed axes) offsets, first step axis fastest
    int64_t in_off = 0, out_off = 0, w_off = 0;
    {
        int64_t r = ss;
        for (int l = 0; l < v.nstep; ++l) {
            const int64_t q = r / v.step_len[l];
            const int64_t c = r - q * v.step_len[l];
            in_off += v.in_step_stride[l] * c;
            out_off += v.out_step_stride[l] * c;
            w_off += a.w_step_stride[l] * c;
            r = q;
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        out_off += v.out_stride[k] * o[k];
        w_off += a.w_stride[k] * o[k];
    }

    // the 2^N taps, lexicographic, last axis fastest: label and weight product (1.0 * w_0 * ... * w_{N-1}, axis order)
    constexpr int T = 1 << N;
    const char* base = v.in + b * a.in_bstride + in_off;
    S lab[T];
    double p[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        int64_t offs = 0;
        double coeff = 1.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            offs += tap[k][(t >> (N - 1 - k)) & 1];
            coeff *= w[k][(t >> (N - 1 - k)) & 1];
        }
        lab[t] = *reinterpret_cast<const S*>(base + offs);
        p[t] = coeff;
    }
    // the vote: each tap's class total, summed in tap order; the largest wins, on equality the smaller label
    S best_lab = lab[0];
    double best = 0.0;
#pragma unroll
    for (int i = 0; i < T; ++i) {
        double total = 0.0;
#pragma unroll
        for (int j = 0; j < T; ++j)
            total += lab[j] == lab[i] ? p[j] : 0.0;
        const bool take = i == 0 || total > best || (total == best && lab[i] < best_lab);
        best = take ? total : best;
        best_lab = take ? lab[i] : best_lab;
    }
    if (constant) {
        best_lab = (S)a.cval_bits;
        best = 1.0;
    }
    *reinterpret_cast<S*>(v.out + b * a.out_bstride + out_off) = best_lab;
    if (a.weight)
        *reinterpret_cast<float*>(a.weight + b * a.w_bstride + w_off) = (float)best;
}

template <int N, typename S>
hipError_t launch_vote(const VoteArgs& a, int nbatch, hipStream_t stream)
{
    const int64_t total = a.g.nvox * a.v.nsteps;
    const int64_t nblk = (total + kVoteThreads - 1) / kVoteThreads;
    if (nblk > 0x7fffffffLL)
        return hipErrorInvalidValue;
    int64_t values = N;
    for (int k = 0; k < N; ++k)
        values *= a.g.ncp[k];
    const dim3 grid((unsigned)nblk, (unsigned)nbatch);
    if (values <= kPointsLdsValues)
        hipLaunchKernelGGL((deform_vote_kernel<N, S, true>), grid, dim3(kVoteThreads), (size_t)values * sizeof(double),
                           stream, a);
    else
        hipLaunchKernelGGL((deform_vote_kernel<N, S, false>), grid, dim3(kVoteThreads), 0, stream, a);
    return hipGetLastError();
}

template <int N>
hipError_t launch_vote_dtype(const VoteArgs& a, int nbatch, hipStream_t stream)
{
    switch (a.v.in_dtype) {
    case EDHIP_BOOL:
    case EDHIP_U8: return launch_vote<N, uint8_t>(a, nbatch, stream);
    case EDHIP_I8: return launch_vote<N, int8_t>(a, nbatch, stream);
    case EDHIP_U16: return launch_vote<N, uint16_t>(a, nbatch, stream);
    case EDHIP_I16: return launch_vote<N, int16_t>(a, nbatch, stream);
    case EDHIP_U32: return launch_vote<N, uint32_t>(a, nbatch, stream);
    case EDHIP_I32: return launch_vote<N, int32_t>(a, nbatch, stream);
    case EDHIP_U64: return launch_vote<N, uint64_t>(a, nbatch, stream);
    case EDHIP_I64: return launch_vote<N, int64_t>(a, nbatch, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_deform_labels(const LabelsCall& c, hipStream_t stream)
{
    const int n = c.g.naxis;
    if (n < 1 || n > 3 || c.nbatch > 65535 || c.v.in_dtype != c.v.out_dtype)
        return hipErrorNotSupported;
    if (c.nbatch <= 0 || c.g.nvox <= 0 || c.v.nsteps <= 0)
        return hipSuccess;                    // nothing to launch
    VoteArgs a;
    memset(&a, 0, sizeof(a));
    a.g = c.g;
    a.v = c.v;
    a.in_bstride = c.in_bstride;
    a.out_bstride = c.out_bstride;
    a.disp_bstride = c.disp_bstride;
    a.weight = c.weight;
    a.w_bstride = c.weight_bstride;
    for (int k = 0; k < n; ++k)
        a.w_stride[k] = c.weight_stride[k];
    for (int l = 0; l < c.v.nstep; ++l)
        a.w_step_stride[l] = c.weight_step_stride[l];
    a.cval_bits = c.cval_bits;
    switch (n) {
    case 1: return launch_vote_dtype<1>(a, c.nbatch, stream);
    case 2: return launch_vote_dtype<2>(a, c.nbatch, stream);
    default: return launch_vote_dtype<3>(a, c.nbatch, stream);
    }
}

}  // namespace ed
