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
// The fixed-point reduction of ed_points_grad.h, with the bounds from two maxima (its rule OWN = false):
//   points_grad_clear     heads and cells of every sample: zero (this file compiles it for every caller)
//   points_grad_prepare   per point: u (forward: the cotangent; inverse: -J^-T g at the solved q) into scratch, the
//                         point's own row (forward: J^T u; inverse: J^-T g), and per sample max|u|, max|q|, the
//                         non-finite flag and the number of contributing points
//   points_grad_scatter   per point: the tap weights again, every u_h prod(w) with quantum_P, u_h and u_h q_l with
//                         quantum_K
//   points_grad_finish    per cell: cell * quantum into ddisplacement / dinverse_affine (this file compiles it for
//                         every caller, once per rule)

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
    const bool need_map = ga.inverse || ga.o.dpts;    // (the forward direction's sums need no J)
    int64_t tstride[N];
    int per = 0;
    if constexpr (LDS) {
        if (need_map) {
            per = stage_grid_lds<N>(g, s_grid);
            __syncthreads();
        }
    }
    grid_tap_strides<N, LDS>(g, tstride);
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
        load_point<N>(a, pts, i, q);
#pragma unroll
        for (int h = 0; h < N; ++h) {
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
        if (ga.o.dpts)
            store_point_row<N>(ga.o, b, i, row);
    }
    publish_head(ga.o.head + b * kGradHead, maxu, maxq, bad, count);
}

template <int N, bool LDS>
__global__ __launch_bounds__(kPointsThreads) void points_grad_scatter(PointsGradArgs ga)
{
    extern __shared__ unsigned long long s_cells[];   // LDS: the dP cells of this workgroup
    const int64_t b = blockIdx.y;
    const PointsArgs& a = ga.p;
    const GridGeom& g = a.g;
    constexpr int NK = N * (N + 1);
    unsigned long long* cellsK = ga.o.cells + b * ga.o.cells_per;
    unsigned long long* cellsP = cellsK + NK;
    int eP, eK, sP, sK;
    grad_quanta<false>(ga.o.head + b * kGradHead, eP, eK, sP, sK);
    if (sP <= 0)
        return;                                       // (uniform over the workgroup; one state for both quanta)
    const bool wantP = ga.o.ddisp != nullptr, wantK = ga.o.dK != nullptr;
    int64_t cstride[N];
    const int64_t per = scatter_begin<N, LDS>(g, ga.o, wantP, s_cells, cstride);
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
        load_point<N>(a, pts, i, q);
#pragma unroll
        for (int h = 0; h < N; ++h) {
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
    scatter_end<N, LDS>(ga.o, wantP, wantK, accK, s_cells, cellsK);
}

// OWN: the rule that turns the head into the two quanta (ed_points_grad.h)
template <int N, bool OWN>
__global__ __launch_bounds__(kPointsThreads) void points_grad_finish(GradSums o, GridGeom g)
{
    const int64_t b = blockIdx.y;
    constexpr int NK = N * (N + 1);
    const unsigned long long* head = o.head + b * kGradHead;
    const unsigned long long* cells = o.cells + b * o.cells_per;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= o.cells_per)
        return;
    const bool isK = e < NK;
    if (isK ? !o.dK : !o.ddisp)
        return;
    int eP, eK, sP, sK;
    grad_quanta<OWN>(head, eP, eK, sP, sK);
    const int state = isK ? sK : sP, ex = isK ? eK : eP;
    // a non-finite cotangent on a contributing point, or a bound that overflows: NaN; nothing to add: exact zeros
    const double v = (head[2] != 0ull || state < 0) ? NAN : (state > 0 ? ldexp((double)(long long)cells[e], ex - 62) : 0.0);
    if (isK) {
        *(double*)(o.dK + b * o.dK_bstride + (e / (N + 1)) * o.dK_stride[0] + (e % (N + 1)) * o.dK_stride[1]) = v;
        return;
    }
    int64_t r = e - NK;
    int64_t per = 1;
#pragma unroll
    for (int k = 0; k < N; ++k)
        per *= g.ncp[k];
    int64_t off = (r / per) * o.ddisp_stride[0];
    r %= per;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        per /= g.ncp[k];
        off += (r / per) * o.ddisp_stride[k + 1];
        r %= per;
    }
    store_cast(o.ddisp + b * o.ddisp_bstride + off, o.ddisp_dtype, v);
}

template <int N>
hipError_t launch_finish(const GradSums& o, const GridGeom& g, int nbatch, bool own_bounds, hipStream_t stream)
{
    const dim3 grid((unsigned)((o.cells_per + kPointsThreads - 1) / kPointsThreads), (unsigned)nbatch);
    if (own_bounds)
        hipLaunchKernelGGL((points_grad_finish<N, true>), grid, dim3(kPointsThreads), 0, stream, o, g);
    else
        hipLaunchKernelGGL((points_grad_finish<N, false>), grid, dim3(kPointsThreads), 0, stream, o, g);
    return hipGetLastError();
}

hipError_t finish_sums(const GradSums& o, const GridGeom& g, int nbatch, bool own_bounds, hipStream_t stream)
{
    if (!o.ddisp && !o.dK)
        return hipSuccess;
    switch (g.naxis) {
    case 1: return launch_finish<1>(o, g, nbatch, own_bounds, stream);
    case 2: return launch_finish<2>(o, g, nbatch, own_bounds, stream);
    case 3: return launch_finish<3>(o, g, nbatch, own_bounds, stream);
    case 4: return launch_finish<4>(o, g, nbatch, own_bounds, stream);
    case 5: return launch_finish<5>(o, g, nbatch, own_bounds, stream);
    case 6: return launch_finish<6>(o, g, nbatch, own_bounds, stream);
    default: return launch_finish<7>(o, g, nbatch, own_bounds, stream);
    }
}

// prepare (unless the caller has written the u rows and the heads itself), scatter and finish
template <int N>
hipError_t launch_points_grad(const PointsGradArgs& ga, int nbatch, bool lds, bool prepare, hipStream_t stream)
{
    const dim3 block(kPointsThreads);
    const GradSums& o = ga.o;
    if (ga.p.npts > 0) {
        const dim3 grid = points_grid(ga.p.npts, nbatch);
        const size_t grid_lds = lds ? (size_t)o.values * sizeof(double) : 0;
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
        if (o.ddisp || o.dK) {
            if (lds)
                hipLaunchKernelGGL((points_grad_scatter<N, true>), grid, block,
                                   o.ddisp ? (size_t)o.values * sizeof(unsigned long long) : 0, stream, ga);
            else
                hipLaunchKernelGGL((points_grad_scatter<N, false>), grid, block, 0, stream, ga);
            e = hipGetLastError();
            if (e != hipSuccess)
                return e;
        }
    }
    return finish_sums(o, ga.p.g, nbatch, false, stream);
}

bool points_grad_call_ok(const GridGeom& g, int nbatch)
{
    return g.naxis >= 1 && g.naxis <= kMaxAxes && nbatch <= 65535;
}

hipError_t launch_points_grad_kernels(const PointsGradCall& c, bool prepare, hipStream_t stream)
{
    PointsGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    PointsArgs& a = ga.p;
    fill_points_args(a, c.g, c.disp_bstride, nullptr, 0, 0.0);
    unpack(c.pos, a.pts, a.pts_stride, a.pts_bstride);
    unpack(c.cot, ga.cot, ga.cot_stride, ga.cot_bstride);
    unpack(c.status, ga.status, ga.status_stride, ga.status_bstride);
    a.pts_f32 = c.pos.dtype == EDHIP_F32;
    ga.cot_f32 = c.cot.dtype == EDHIP_F32;
    a.npts = c.npts;
    ga.inverse = c.inverse;
    if (!c.inverse)
        ga.status = nullptr;
    const bool lds = fill_grad_sums(ga.o, c.dpts, c.ddisp, c.dK, c.g, c.scratch, c.nbatch);
    ga.u = (double*)(ga.o.cells + (size_t)c.nbatch * (size_t)ga.o.cells_per);   // the u rows: behind heads and cells
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

hipError_t launch_points_grad_clear(const GridGeom& g, int nbatch, char* scratch, hipStream_t stream)
{
    if (!points_grad_call_ok(g, nbatch))
        return hipErrorNotSupported;
    if (nbatch <= 0)
        return hipSuccess;
    const int64_t words = (int64_t)nbatch * (kGradHead + points_grad_cells_per(g));
    hipLaunchKernelGGL(points_grad_clear, dim3(points_grid(words, 1).x), dim3(kPointsThreads), 0, stream,
                       (unsigned long long*)scratch, words);
    return hipGetLastError();
}

hipError_t launch_points_grad_finish(const GridGeom& g, int nbatch, const BatchArray& ddisp, const BatchArray& dK,
                                     char* scratch, bool own_bounds, hipStream_t stream)
{
    if (!points_grad_call_ok(g, nbatch))
        return hipErrorNotSupported;
    if (nbatch <= 0)
        return hipSuccess;
    GradSums o;
    memset(&o, 0, sizeof(o));
    fill_grad_sums(o, BatchArray{}, ddisp, dK, g, scratch, nbatch);
    return finish_sums(o, g, nbatch, own_bounds, stream);
}

hipError_t launch_points_grad_reduce(const PointsGradCall& c, hipStream_t stream)
{
    if (!points_grad_call_ok(c.g, c.nbatch))
        return hipErrorNotSupported;
    if (c.nbatch <= 0)
        return hipSuccess;
    return launch_points_grad_kernels(c, false, stream);
}

hipError_t launch_deform_points_gradient(const PointsGradCall& c, hipStream_t stream)
{
    const hipError_t e = launch_points_grad_clear(c.g, c.nbatch, c.scratch, stream);
    if (e != hipSuccess || c.nbatch <= 0)
        return e;
    return launch_points_grad_kernels(c, true, stream);
}

}  // namespace ed
