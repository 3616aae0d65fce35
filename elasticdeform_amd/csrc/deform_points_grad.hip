// deform_points_grad.hip -- the adjoint of deform_points.hip: gradients through the coordinate map r(q) and through its
// inverse, with respect to the points, the prefiltered control grid P and the inverse map K.
//
// r_h(q) = sum_l K[h, l] q_l + K[h, n] + off_h + sum_j P[h, j] beta(q, j), beta(q, j) being the sum of the cubic
// tap-weight products whose mirrored tap index is j, is linear in P and K.  With u[i] = dL/dr(q_i):
//   dP[h, j] = sum_i u[i, h] beta(q_i, j)     dK[h, l < n] = sum_i u[i, h] q_i[l]     dK[h, n] = sum_i u[i, h]
//   dq_i = J_i^T u_i
// and for the inverse direction (q_i = r^-1(p_i), g_i = dL/dq_i), by the implicit function theorem at the solved q_i,
//   dp_i = J_i^-T g_i      and the sums above with u_i = -J_i^-T g_i.
#include <cmath>
#include <cstring>

#include "ed_device.h"
#include "ed_exact_coord.h"
#include "ed_params.h"
#include "ed_points.h"
#include "ed_points_grad.h"

namespace ed {

namespace {

// ---- the adjoint: gradients through r(q) and through its inverse ----------------------------------------------
//   points_grad_prepare   per point: u (forward: the cotangent; inverse: -J^-T g at the solved q) into scratch, the
//                         point's own row (forward: J^T u; inverse: J^-T g), and per sample max|u|, max|q| (one
//                         integer atomicMax per wave on the bits of the non-negative double) and the non-finite flag
//   points_grad_scatter   per point: the tap weights again, every u_h prod(w) as llrint(c / quantum_P) added into
//                         64-bit integer cells (LDS per workgroup for grids up to kPointsLdsValues values, flushed
//                         with global integer atomics; global atomics directly beyond), u_h and u_h q_l likewise with
//                         quantum_K, reduced per wave first
//   points_grad_finish    per cell: cell * quantum into ddisplacement / dinverse_affine
// quantum_P = 2^(e - 62) with 2^e the smallest power of two >= 2 N max|u|; quantum_K the same from
// N max|u| max(1, max|q|), N counting the points that contribute (so that points which contribute nothing do not
// change a bit of the sums): no cell can overflow, and integer addition is associative, so the sums depend neither on the
// order in which the points arrive nor on how they are dealt to workgroups.  points_grad_clear zeroes heads and cells
// in front of every call: nothing is carried from one call to the next.

// the exponent e of the smallest power of two >= bound (bound > 0 and finite)
__device__ __forceinline__ int ceil_pow2_exponent(double bound)
{
    int ex;
    const double m = frexp(bound, &ex);       // bound = m 2^ex, 0.5 <= m < 1
    return m == 0.5 ? ex - 1 : ex;
}

// the two quanta of a sample as exponents (quantum = 2^(e - 62)); false: nothing to add (max|u| = 0) or not
// representable (the bound overflows)
__device__ __forceinline__ bool grad_quanta(const unsigned long long* head, int& eP, int& eK)
{
    const double maxu = __longlong_as_double((long long)head[0]);
    const double maxq = __longlong_as_double((long long)head[1]);
    const double bP = 2.0 * (double)head[3] * maxu;
    const double bK = bP * (maxq > 1.0 ? maxq : 1.0);
    eP = eK = 0;
    if (!(bP > 0.0) || !isfinite(bK))
        return false;
    eP = ceil_pow2_exponent(bP);
    eK = ceil_pow2_exponent(bK);
    return true;
}

// heads and cells of every sample: zero (a kernel of the call's own, in stream order in front of the other three)
__global__ __launch_bounds__(kPointsThreads) void points_grad_clear(unsigned long long* words, int64_t count)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
        words[i] = 0ull;
}

template <int N, bool LDS>
__global__ __launch_bounds__(kPointsThreads) void points_grad_prepare(PointsGradArgs ga)
{
    extern __shared__ double s_grid[];
    const int64_t b = blockIdx.y;
    PointsArgs& a = ga.p;
    a.g.disp += b * a.disp_bstride;
    const GridGeom& g = a.g;
    const bool need_map = ga.inverse || ga.dpts;      // (the forward direction's sums need no J)
    int64_t tstride[N];
    int per = 0;
    if constexpr (LDS) {
        if (need_map) {
            per = stage_grid_lds<N>(g, s_grid);
            __syncthreads();
        }
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
    const char* cot = ga.cot + b * ga.cot_bstride;
    double* urow = ga.u + b * a.npts * N;
    double maxu = 0.0, maxq = 0.0;
    unsigned long long count = 0ull;          // contributing points
    bool bad = false;

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts;
         i += (int64_t)gridDim.x * blockDim.x) {
        double q[N], c[N], u[N], row[N];
        bool cfinite = true;
#pragma unroll
        for (int h = 0; h < N; ++h) {
            const char* src = pts + i * a.pts_stride[0] + h * a.pts_stride[1];
            q[h] = a.pts_f32 ? (double)*(const float*)src : *(const double*)src;
            const char* csrc = cot + i * ga.cot_stride[0] + h * ga.cot_stride[1];
            c[h] = ga.cot_f32 ? (double)*(const float*)csrc : *(const double*)csrc;
            cfinite = cfinite && isfinite(c[h]);
        }
        bool contributes = sane_position<N>(a, q);
        if (ga.inverse && ga.status)
            contributes = contributes && ga.status[b * ga.status_bstride + i * ga.status_stride] != 0;
        if (contributes && need_map) {
            double r[N], J[N][N];
            if constexpr (LDS)
                eval_map<N>(a, LdsGrid{s_grid, per}, tstride, q, r, J);
            else
                eval_map<N>(a, GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, tstride, q, r, J);
            if (ga.inverse) {
                // u = -J^-T g.  A singular or non-finite J: the point contributes nothing; whether J is usable is
                // asked with a finite right-hand side, so that a non-finite cotangent is told apart from it
                double JT[N][N], rhs[N], s[N];
#pragma unroll
                for (int h = 0; h < N; ++h) {
                    rhs[h] = cfinite ? c[h] : 1.0;
#pragma unroll
                    for (int l = 0; l < N; ++l)
                        JT[h][l] = J[l][h];
                }
                contributes = solve<N>(JT, rhs, s);
#pragma unroll
                for (int h = 0; h < N; ++h) {
                    row[h] = cfinite ? s[h] : NAN;
                    u[h] = -row[h];
                }
            } else {
#pragma unroll
                for (int l = 0; l < N; ++l) {
                    double acc = 0.0;
#pragma unroll
                    for (int h = 0; h < N; ++h)
                        acc += J[h][l] * c[h];
                    row[l] = acc;
                    u[l] = c[l];
                }
            }
        } else {
#pragma unroll
            for (int h = 0; h < N; ++h) {
                u[h] = c[h];
                row[h] = 0.0;
            }
        }
        if (!contributes) {
#pragma unroll
            for (int h = 0; h < N; ++h)
                u[h] = row[h] = 0.0;
        } else if (!cfinite) {
            bad = true;
        } else {
            ++count;
#pragma unroll
            for (int h = 0; h < N; ++h) {
                maxu = fabs(u[h]) > maxu ? fabs(u[h]) : maxu;
                maxq = fabs(q[h]) > maxq ? fabs(q[h]) : maxq;
            }
        }
#pragma unroll
        for (int h = 0; h < N; ++h)
            urow[i * N + h] = u[h];
        if (ga.dpts) {
            char* dst = ga.dpts + b * ga.dpts_bstride + i * ga.dpts_stride[0];
#pragma unroll
            for (int h = 0; h < N; ++h) {
                if (ga.dpts_f32)
                    *(float*)(dst + h * ga.dpts_stride[1]) = (float)row[h];
                else
                    *(double*)(dst + h * ga.dpts_stride[1]) = row[h];
            }
        }
    }
    // a max does not depend on the order: one integer atomicMax per wave on the bits of the non-negative doubles
    maxu = wave_max(maxu);
    maxq = wave_max(maxq);
    const bool any_bad = __any(bad);
    for (int m = warpSize / 2; m > 0; m >>= 1)
        count += (unsigned long long)__shfl_xor((long long)count, m);
    if ((threadIdx.x & (warpSize - 1)) == 0) {
        unsigned long long* head = ga.head + b * kGradHead;
        if (maxu > 0.0)
            atomicMax(head + 0, (unsigned long long)__double_as_longlong(maxu));
        if (maxq > 0.0)
            atomicMax(head + 1, (unsigned long long)__double_as_longlong(maxq));
        if (any_bad)
            atomicMax(head + 2, 1ull);
        if (count)
            atomicAdd(head + 3, count);
    }
}

__device__ __forceinline__ unsigned long long quantise(double c, int shift)
{
    return (unsigned long long)llrint(ldexp(c, shift));
}

template <int N, bool LDS>
__global__ __launch_bounds__(kPointsThreads) void points_grad_scatter(PointsGradArgs ga)
{
    extern __shared__ unsigned long long s_cells[];   // LDS: the dP cells of this workgroup
    const int64_t b = blockIdx.y;
    const PointsArgs& a = ga.p;
    const GridGeom& g = a.g;
    constexpr int NK = N * (N + 1);
    unsigned long long* cellsK = ga.cells + b * ga.cells_per;
    unsigned long long* cellsP = cellsK + NK;
    int eP, eK;
    const bool any = grad_quanta(ga.head + b * kGradHead, eP, eK);
    if (!any)
        return;                                       // (uniform over the workgroup)
    const bool wantP = ga.ddisp != nullptr, wantK = ga.dK != nullptr;
    if constexpr (LDS) {
        if (wantP) {
            for (int e = threadIdx.x; e < ga.values; e += blockDim.x)
                s_cells[e] = 0ull;
            __syncthreads();
        }
    }
    int64_t cstride[N];
    int64_t per = 1;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
        cstride[k] = per;
        per *= g.ncp[k];
    }
    const char* pts = a.pts + b * a.pts_bstride;
    const double* urow = ga.u + b * a.npts * N;
    unsigned long long accK[NK];
#pragma unroll
    for (int e = 0; e < NK; ++e)
        accK[e] = 0ull;

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts;
         i += (int64_t)gridDim.x * blockDim.x) {
        double q[N], u[N];
        bool zero = true, finite = true;
#pragma unroll
        for (int h = 0; h < N; ++h) {
            const char* src = pts + i * a.pts_stride[0] + h * a.pts_stride[1];
            q[h] = a.pts_f32 ? (double)*(const float*)src : *(const double*)src;
            u[h] = urow[i * N + h];
            zero = zero && u[h] == 0.0;
            finite = finite && isfinite(u[h]);
        }
        // a zero row adds nothing (a point that contributes nothing has one); a non-finite one has set the sample's
        // flag; a position that is not sane has no exact tap index
        if (zero || !finite || !sane_position<N>(a, q))
            continue;
        if (wantK) {
#pragma unroll
            for (int h = 0; h < N; ++h) {
#pragma unroll
                for (int l = 0; l < N; ++l)
                    accK[h * (N + 1) + l] += quantise(u[h] * q[l], 62 - eK);
                accK[h * (N + 1) + N] += quantise(u[h], 62 - eK);
            }
        }
        if (!wantP)
            continue;
        int64_t toff[N][4];
        double w[N][4];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double cp = (double)(g.ncp[k] - 1) * (q[k] + (double)g.off[k]) / (double)(g.in_len[k] - 1);
            const int64_t start = window_start(cp, 3);
            spline_weights(cp, 3, w[k]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                toff[k][t] = mirror_index(start + t, g.ncp[k]) * cstride[k];
        }
        auto add = [&](int64_t off, double prod) {
#pragma unroll
            for (int h = 0; h < N; ++h) {
                const unsigned long long v = quantise(u[h] * prod, 62 - eP);
                if constexpr (LDS)
                    atomicAdd(&s_cells[h * per + off], v);
                else
                    atomicAdd(&cellsP[h * per + off], v);
            }
        };
        if constexpr (N == 1) {
#pragma unroll
            for (int t0 = 0; t0 < 4; ++t0)
                add(toff[0][t0], w[0][t0]);
        } else if constexpr (N <= 3) {
            // the outermost tap loop stays rolled, its weight and offset rotating through scalars (grid_taps' scheme:
            // a select on the loop counter becomes an indexed read of a scratch array)
            double w0 = w[0][0], w1 = w[0][1], w2 = w[0][2], w3 = w[0][3];
            int64_t o0 = toff[0][0], o1 = toff[0][1], o2 = toff[0][2], o3 = toff[0][3];
#pragma unroll 1
            for (int t0 = 0; t0 < 4; ++t0) {
#pragma unroll
                for (int t1 = 0; t1 < 4; ++t1) {
                    if constexpr (N == 2) {
                        add(o0 + toff[1][t1], w0 * w[1][t1]);
                    } else {
#pragma unroll
                        for (int t2 = 0; t2 < 4; ++t2)
                            add(o0 + toff[1][t1] + toff[2][t2], w0 * w[1][t1] * w[N - 1][t2]);
                    }
                }
                const double wr = w0;
                const int64_t orot = o0;
                w0 = w1, w1 = w2, w2 = w3, w3 = wr;
                o0 = o1, o1 = o2, o2 = o3, o3 = orot;
            }
        } else {
            for (int tap = 0; tap < ipow4(N); ++tap) {
                int64_t off = 0;
                double prod = 1.0;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const int t = (tap >> (2 * (N - 1 - k))) & 3;
                    off += pick4(toff[k], t);
                    prod *= pick4(w[k], t);
                }
                add(off, prod);
            }
        }
    }
    if (wantK) {
        // per wave first, then one atomic per wave and cell
#pragma unroll
        for (int e = 0; e < NK; ++e) {
            unsigned long long v = accK[e];
            for (int m = warpSize / 2; m > 0; m >>= 1)
                v += (unsigned long long)__shfl_xor((long long)v, m);
            if ((threadIdx.x & (warpSize - 1)) == 0 && v != 0ull)
                atomicAdd(&cellsK[e], v);
        }
    }
    if constexpr (LDS) {
        if (wantP) {
            __syncthreads();
            for (int e = threadIdx.x; e < ga.values; e += blockDim.x) {
                const unsigned long long v = s_cells[e];
                if (v != 0ull)
                    atomicAdd(&cellsP[e], v);
            }
        }
    }
}

template <int N>
__global__ __launch_bounds__(kPointsThreads) void points_grad_finish(PointsGradArgs ga)
{
    const int64_t b = blockIdx.y;
    const GridGeom& g = ga.p.g;
    constexpr int NK = N * (N + 1);
    const unsigned long long* head = ga.head + b * kGradHead;
    const unsigned long long* cells = ga.cells + b * ga.cells_per;
    int eP, eK;
    const bool any = grad_quanta(head, eP, eK);
    const bool zero = __longlong_as_double((long long)head[0]) == 0.0;     // no contribution at all: exact zeros
    const bool nan = head[2] != 0ull || (!any && !zero);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ga.cells_per)
        return;
    if (e < NK) {
        if (!ga.dK)
            return;
        const double v = nan ? NAN : (any ? ldexp((double)(long long)cells[e], eK - 62) : 0.0);
        *(double*)(ga.dK + b * ga.dK_bstride + (e / (N + 1)) * ga.dK_stride[0] + (e % (N + 1)) * ga.dK_stride[1]) = v;
        return;
    }
    if (!ga.ddisp)
        return;
    const double v = nan ? NAN : (any ? ldexp((double)(long long)cells[e], eP - 62) : 0.0);
    int64_t r = e - NK;
    int64_t per = 1;
#pragma unroll
    for (int k = 0; k < N; ++k)
        per *= g.ncp[k];
    int64_t off = (r / per) * ga.ddisp_stride[0];
    r %= per;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        per /= g.ncp[k];
        off += (r / per) * ga.ddisp_stride[k + 1];
        r %= per;
    }
    store_cast(ga.ddisp + b * ga.ddisp_bstride + off, ga.ddisp_dtype, v);
}

// prepare (unless the caller has written the u rows and the heads itself), scatter and finish
template <int N>
hipError_t launch_points_grad(const PointsGradArgs& ga, int nbatch, bool lds, bool prepare, hipStream_t stream)
{
    const dim3 block(kPointsThreads);
    const int64_t npts = ga.p.npts;
    if (npts > 0) {
        const int64_t want = (npts + kPointsThreads - 1) / kPointsThreads;
        const dim3 grid((unsigned)(want < kPointsMaxBlocks ? want : kPointsMaxBlocks), (unsigned)nbatch);
        const size_t grid_lds = lds ? (size_t)ga.values * sizeof(double) : 0;
        hipError_t e = hipSuccess;
        if (prepare) {
            if (lds)
                hipLaunchKernelGGL((points_grad_prepare<N, true>), grid, block, grid_lds, stream, ga);
            else
                hipLaunchKernelGGL((points_grad_prepare<N, false>), grid, block, 0, stream, ga);
            e = hipGetLastError();
            if (e != hipSuccess)
                return e;
        }
        if (ga.ddisp || ga.dK) {
            if (lds)
                hipLaunchKernelGGL((points_grad_scatter<N, true>), grid, block,
                                   ga.ddisp ? (size_t)ga.values * sizeof(unsigned long long) : 0, stream, ga);
            else
                hipLaunchKernelGGL((points_grad_scatter<N, false>), grid, block, 0, stream, ga);
            e = hipGetLastError();
            if (e != hipSuccess)
                return e;
        }
    }
    if (ga.ddisp || ga.dK) {
        const dim3 grid((unsigned)((ga.cells_per + kPointsThreads - 1) / kPointsThreads), (unsigned)nbatch);
        hipLaunchKernelGGL((points_grad_finish<N>), grid, block, 0, stream, ga);
        return hipGetLastError();
    }
    return hipSuccess;
}

// the call as the kernels take it; returns whether grid and cells fit LDS
bool fill_points_grad_args(const PointsGradCall& c, PointsGradArgs& ga)
{
    const int n = c.g.naxis;
    memset(&ga, 0, sizeof(ga));
    PointsArgs& a = ga.p;
    const int64_t values = fill_points_args(a, c.g, c.disp_bstride, nullptr, 0, 0.0);
    unpack(c.pos, a.pts, a.pts_stride, a.pts_bstride);
    unpack(c.cot, ga.cot, ga.cot_stride, ga.cot_bstride);
    unpack(c.status, ga.status, ga.status_stride, ga.status_bstride);
    unpack(c.dpts, ga.dpts, ga.dpts_stride, ga.dpts_bstride);
    unpack(c.ddisp, ga.ddisp, ga.ddisp_stride, ga.ddisp_bstride);
    unpack(c.dK, ga.dK, ga.dK_stride, ga.dK_bstride);
    a.pts_f32 = c.pos.dtype == EDHIP_F32;
    ga.cot_f32 = c.cot.dtype == EDHIP_F32;
    ga.dpts_f32 = c.dpts.dtype == EDHIP_F32;
    ga.ddisp_dtype = c.ddisp.dtype;
    a.npts = c.npts;
    ga.inverse = c.inverse;
    if (!c.inverse)
        ga.status = nullptr;
    ga.cells_per = values + n * (n + 1);
    const bool lds = values <= kPointsLdsValues;
    ga.values = lds ? (int)values : 0;
    // scratch (ed_points_grad.h): [nbatch heads | nbatch x cells | nbatch x npts x naxis doubles]; heads and cells are
    // cleared by every call itself, so that nothing is carried from an earlier call (a captured graph replays
    // self-contained)
    ga.head = (unsigned long long*)c.scratch;
    ga.cells = ga.head + (size_t)c.nbatch * kGradHead;
    ga.u = (double*)(ga.cells + (size_t)c.nbatch * (size_t)ga.cells_per);
    return lds;
}

bool points_grad_call_ok(const PointsGradCall& c)
{
    return c.g.naxis >= 1 && c.g.naxis <= kMaxAxes && c.nbatch <= 65535;
}

hipError_t launch_points_grad_kernels(const PointsGradCall& c, bool prepare, hipStream_t stream)
{
    PointsGradArgs ga;
    const bool lds = fill_points_grad_args(c, ga);
    switch (c.g.naxis) {
    case 1: return launch_points_grad<1>(ga, c.nbatch, lds, prepare, stream);
    case 2: return launch_points_grad<2>(ga, c.nbatch, lds, prepare, stream);
    case 3: return launch_points_grad<3>(ga, c.nbatch, lds, prepare, stream);
    case 4: return launch_points_grad<4>(ga, c.nbatch, lds, prepare, stream);
    case 5: return launch_points_grad<5>(ga, c.nbatch, lds, prepare, stream);
    case 6: return launch_points_grad<6>(ga, c.nbatch, lds, prepare, stream);
    default: return launch_points_grad<7>(ga, c.nbatch, lds, prepare, stream);
    }
}

}  // namespace

size_t points_grad_scratch_bytes(const GridGeom& g, int nbatch, int64_t npts)
{
    return (size_t)nbatch * (size_t)(kGradHead + points_grad_cells_per(g) + npts * g.naxis) * 8;
}

hipError_t launch_points_grad_clear(const PointsGradCall& c, hipStream_t stream)
{
    if (!points_grad_call_ok(c))
        return hipErrorNotSupported;
    if (c.nbatch <= 0)
        return hipSuccess;
    const int64_t words = (int64_t)c.nbatch * (kGradHead + points_grad_cells_per(c.g));
    const int64_t blocks = (words + kPointsThreads - 1) / kPointsThreads;
    hipLaunchKernelGGL(points_grad_clear, dim3((unsigned)(blocks < kPointsMaxBlocks ? blocks : kPointsMaxBlocks)),
                       dim3(kPointsThreads), 0, stream, (unsigned long long*)c.scratch, words);
    return hipGetLastError();
}

hipError_t launch_points_grad_reduce(const PointsGradCall& c, hipStream_t stream)
{
    if (!points_grad_call_ok(c))
        return hipErrorNotSupported;
    if (c.nbatch <= 0)
        return hipSuccess;
    return launch_points_grad_kernels(c, false, stream);
}

hipError_t launch_deform_points_gradient(const PointsGradCall& c, hipStream_t stream)
{
    const hipError_t e = launch_points_grad_clear(c, stream);
    if (e != hipSuccess || c.nbatch <= 0)
        return e;
    return launch_points_grad_kernels(c, true, stream);
}

}  // namespace ed
