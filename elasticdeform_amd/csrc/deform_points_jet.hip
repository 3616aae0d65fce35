// deform_points_jet.hip -- the local differential structure of the coordinate map at arbitrary real positions: r(q),
// J = dr/dq and H = d^2r/dq dq, and the adjoint of the three with respect to the positions, the prefiltered control
// grid P and the inverse map K.
//
// In the notation of deform_points.hip (cp_k = (ncp_k - 1)(q_k + off_k)/(I_k - 1), s_k = (ncp_k - 1)/(I_k - 1), the
// four cubic taps of an axis starting at floor(cp_k) - 1 and folded by the mirror tap map m), with w^(a) the a-th
// derivative of the cubic weights in the knot cell of floor(cp) -- w'' = (1 - x, 3x - 2, 1 - 3x, x), w''' =
// (-1, 3, -3, 1) -- and a = (a_0 .. a_{n-1}) a multi-index:
//   S_h[a](q)     = sum_taps P[h, m(t)] prod_k s_k^{a_k} w_k^(a_k)[t_k]                       ("the jet sums")
//   r_h           = sum_l K[h, l] q_l + K[h, n] + off_h + S_h[0]
//   J[h, l]       = K[h, l] + S_h[e_l]         H[h, l, m] = S_h[e_l + e_m]         T[h, l, m, p] = S_h[e_l + e_m + e_p]
// H is symmetric in (l, m) and does not depend on K.
//
//   points_jet_kernel<N, LDS, HESS>   r and J from eval_map as deform_points.hip calls it (the same device code, the
//                                     same bits), H from jet_sums<N, 2, 2>: one sweep over the 4^n taps per component
//                                     with one accumulator per distinct second derivative (six for three axes).  One
//                                     thread per point, blockIdx.y = sample, no atomics, no cross-lane operations.
//
// The adjoint for the cotangents u = dL/dr, A = dL/dJ, G = dL/dH (any of them absent; G need not be symmetric), with
// beta(q, j) the folded tap-weight products of deform_points_grad.hip:
//   dP[h, j]   = sum_i ( u[i,h] beta(q_i, j) + sum_l A[i,h,l] d_l beta(q_i, j) + sum_lm G[i,h,l,m] d_l d_m beta(q_i, j) )
//   dK[h, l<n] = sum_i ( u[i,h] q_i[l] + A[i,h,l] )        dK[h, n] = sum_i u[i,h]
//   dq_i[p]    = sum_h u[i,h] J[h,p] + sum_hl A[i,h,l] H[h,l,p] + sum_hlm G[i,h,l,m] T[h,l,m,p]
// by the fixed-point reduction of ed_points_grad.h (the scheme, its bit contract and the clear and finish kernels
// are there and in deform_points_grad.hip), with the rule of own bounds (OWN = true):
//   points_jet_grad_prepare   per point the row dq (jet_sums<N, 1, 3>, or <N, 1, 2> without G); per sample the bounds
//                             bP = max_{i,h} |u_h| + 1.5 sum_l s_l |A_hl| + sum_lm c_lm s_l s_m |G_hlm| (c_ll = 4,
//                             c_lm = 2.25: sum_t |w_t| = 1, sum_t |w'_t| <= 1.5, sum_t |w''_t| <= 4 on [0, 1)), which
//                             bounds what one point adds to one cell however its taps fold, and
//                             bK = max_{i,h} max(|u_h|, max_l |u_h q_l| + |A_hl|); the non-finite flag; the number of
//                             contributing points
//   points_jet_grad_scatter   per point and tap the coefficient u_h W + sum_l A_hl d_l W + sum_lm G_hlm d_l d_m W with
//                             quantum_P, the dK terms with quantum_K
// The cotangents are read from the caller's arrays in both passes: the scratch holds heads and cells only.
#include <cmath>
#include <cstring>
#include <type_traits>

#include "ed_device.h"
#include "ed_exact_coord.h"
#include "ed_params.h"
#include "ed_points.h"
#include "ed_points_grad.h"
#include "ed_points_jet.h"

namespace ed {

namespace {

constexpr int kJetMaxAxes = 3;

struct JetArgs {
    PointsArgs p;                             // pts, res, jac, the geometry; status, minv, max_iter, tol unused
    char* hess;                               // (npts, naxis, naxis, naxis) float64, or nullptr
    int64_t hess_stride[4], hess_bstride;
};

struct JetGradArgs {
    PointsArgs p;                             // p.pts: the positions q; p.g, p.scale: the geometry; the rest unused
    const char* du;                           // (npts, naxis) float32 / float64, or nullptr
    const char* dA;                           // (npts, naxis, naxis), or nullptr
    const char* dG;                           // (npts, naxis, naxis, naxis), or nullptr
    int du_f32, dA_f32, dG_f32;
    int64_t du_stride[2], du_bstride;
    int64_t dA_stride[3], dA_bstride;
    int64_t dG_stride[4], dG_bstride;
    GradSums o;                               // head: bits of bP, of bK, the flag, the count
};

// four values that take turns at the front: what a rolled tap loop reads without indexing a register array
template <typename T>
struct Rot4 {
    T a, b, c, d;
    __device__ __forceinline__ void turn()
    {
        const T t = a;
        a = b, b = c, c = d, d = t;
    }
};

// Per axis the folded tap offsets (in units of tstride) and wj[k][a][t] = s_k^a w_k^(a)[t], a = 0 .. 3.  A position
// that is not finite, or too far out for the tap index to be an exact integer: eval_map's rule -- the taps of position
// 0 with NaN weights.
template <int N, typename Off>
__device__ __forceinline__ void jet_weights(const PointsArgs& a, const int64_t (&tstride)[N], const double (&q)[N],
                                            Off (&toff)[N][4], double (&wj)[N][4][4])
{
    const GridGeom& g = a.g;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double cpq = (double)(g.ncp[k] - 1) * (q[k] + (double)g.off[k]) / (double)(g.in_len[k] - 1);
        const bool sane = fabs(cpq) < kPointsMaxCoordinate;
        const double cp = sane ? cpq : 0.0;
        const int64_t start = window_start(cp, 3);
        spline_weights(cp, 3, wj[k][0]);
        spline_weight_derivatives(cp, 3, wj[k][1]);
        const double x = cp - floor(cp);
        wj[k][2][0] = 1.0 - x;
        wj[k][2][1] = 3.0 * x - 2.0;
        wj[k][2][2] = 1.0 - 3.0 * x;
        wj[k][2][3] = x;
        wj[k][3][0] = -1.0;
        wj[k][3][1] = 3.0;
        wj[k][3][2] = -3.0;
        wj[k][3][3] = 1.0;
        const double s1 = a.scale[k], s2 = s1 * s1, s3 = s2 * s1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            toff[k][t] = (Off)(mirror_index(start + t, g.ncp[k]) * tstride[k]);
            wj[k][0][t] = sane ? wj[k][0][t] : NAN;
            wj[k][1][t] = sane ? wj[k][1][t] * s1 : NAN;
            wj[k][2][t] = sane ? wj[k][2][t] * s2 : NAN;
            wj[k][3][t] = sane ? wj[k][3][t] * s3 : NAN;
        }
    }
}

// The jet sums S[a_0][a_1][a_2] of component h for every multi-index with LO <= |a| <= HI (a_k = 0 for k >= N), the
// other slots untouched: one separable sweep over the 4^N taps.  grid_taps' scheme for three axes: the outermost tap
// loop stays rolled, its weights and offset rotating through scalars; every index into S, into the partial sums and
// into wj is a constant after unrolling, so nothing is a runtime-indexed register array.
template <int N, int LO, int HI, typename Grid>
__device__ __forceinline__ void jet_sums(const Grid& grid, int h, const typename Grid::Off (&toff)[N][4],
                                         const double (&wj)[N][4][4], double (&S)[4][4][4])
{
    typedef typename Grid::Off Off;
#pragma unroll
    for (int a0 = 0; a0 <= HI; ++a0)
#pragma unroll
        for (int a1 = 0; a1 <= (N >= 2 ? HI : 0); ++a1)
#pragma unroll
            for (int a2 = 0; a2 <= (N >= 3 ? HI : 0); ++a2)
                if (a0 + a1 + a2 >= LO && a0 + a1 + a2 <= HI)
                    S[a0][a1][a2] = 0.0;
    if constexpr (N == 1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double c = grid(h, toff[0][t]);
#pragma unroll
            for (int a0 = LO; a0 <= HI; ++a0)
                S[a0][0][0] += c * wj[0][a0][t];
        }
    } else if constexpr (N == 2) {
#pragma unroll
        for (int t0 = 0; t0 < 4; ++t0) {
            double in[4];
#pragma unroll
            for (int a1 = 0; a1 <= HI; ++a1)
                in[a1] = 0.0;
#pragma unroll
            for (int t1 = 0; t1 < 4; ++t1) {
                const double c = grid(h, toff[0][t0] + toff[1][t1]);
#pragma unroll
                for (int a1 = 0; a1 <= HI; ++a1)
                    in[a1] += c * wj[1][a1][t1];
            }
#pragma unroll
            for (int a0 = 0; a0 <= HI; ++a0)
#pragma unroll
                for (int a1 = 0; a1 <= HI; ++a1)
                    if (a0 + a1 >= LO && a0 + a1 <= HI)
                        S[a0][a1][0] += wj[0][a0][t0] * in[a1];
        }
    } else {
        static_assert(N == 3, "the jet sums cover 1 to 3 axes");
        Rot4<double> wo[4];
#pragma unroll
        for (int a0 = 0; a0 <= HI; ++a0)
            wo[a0] = Rot4<double>{wj[0][a0][0], wj[0][a0][1], wj[0][a0][2], wj[0][a0][3]};
        Rot4<Off> oo{toff[0][0], toff[0][1], toff[0][2], toff[0][3]};
#pragma unroll 1
        for (int t0 = 0; t0 < 4; ++t0) {
            double mid[4][4];
#pragma unroll
            for (int a1 = 0; a1 <= HI; ++a1)
#pragma unroll
                for (int a2 = 0; a1 + a2 <= HI; ++a2)
                    mid[a1][a2] = 0.0;
#pragma unroll
            for (int t1 = 0; t1 < 4; ++t1) {
                double in[4];
#pragma unroll
                for (int a2 = 0; a2 <= HI; ++a2)
                    in[a2] = 0.0;
#pragma unroll
                for (int t2 = 0; t2 < 4; ++t2) {
                    const double c = grid(h, oo.a + toff[1][t1] + toff[2][t2]);
#pragma unroll
                    for (int a2 = 0; a2 <= HI; ++a2)
                        in[a2] += c * wj[2][a2][t2];
                }
#pragma unroll
                for (int a1 = 0; a1 <= HI; ++a1)
#pragma unroll
                    for (int a2 = 0; a1 + a2 <= HI; ++a2)
                        mid[a1][a2] += wj[1][a1][t1] * in[a2];
            }
#pragma unroll
            for (int a0 = 0; a0 <= HI; ++a0)
#pragma unroll
                for (int a1 = 0; a0 + a1 <= HI; ++a1)
#pragma unroll
                    for (int a2 = 0; a0 + a1 + a2 <= HI; ++a2)
                        if (a0 + a1 + a2 >= LO)
                            S[a0][a1][a2] += wo[a0].a * mid[a1][a2];
#pragma unroll
            for (int a0 = 0; a0 <= HI; ++a0)
                wo[a0].turn();
            oo.turn();
        }
    }
}

// S[e_l + e_m + e_p] for axes l, m, p; an axis of -1 adds nothing
__device__ __forceinline__ double jet_at(const double (&S)[4][4][4], int l, int m, int p)
{
    return S[(l == 0) + (m == 0) + (p == 0)][(l == 1) + (m == 1) + (p == 1)][(l == 2) + (m == 2) + (p == 2)];
}

// element (i0, i1, i2) of an optional float32 / float64 array (a stride that does not apply: times index 0)
__device__ __forceinline__ double load_cot(const char* base, int f32, int64_t off)
{
    if (!base)
        return 0.0;
    return f32 ? (double)*(const float*)(base + off) : *(const double*)(base + off);
}

// ---- forward: r, J, H -----------------------------------------------------------------------------------------------
template <int N, bool LDS, bool HESS>
__global__ __launch_bounds__(kPointsThreads) void points_jet_kernel(JetArgs ja)
{
    extern __shared__ double s_grid[];        // LDS: [N][ncp_0]...[ncp_{N-1}]
    const int64_t b = blockIdx.y;
    PointsArgs& a = ja.p;
    a.g.disp += b * a.disp_bstride;           // this sample's control grid
    const GridGeom& g = a.g;
    int64_t tstride[N];
    int per = 0;
    if constexpr (LDS) {
        per = stage_grid_lds<N>(g, s_grid);
        __syncthreads();
    }
    grid_tap_strides<N, LDS>(g, tstride);
    const char* pts = a.pts + b * a.pts_bstride;
    char* res = a.res + b * a.res_bstride;

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts;
         i += (int64_t)gridDim.x * blockDim.x) {
        double q[N], r[N], J[N][N];
        load_point<N>(a, pts, i, q);
        if constexpr (LDS)
            eval_map<N>(a, LdsGrid{s_grid, per}, tstride, q, r, J);
        else
            eval_map<N>(a, GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, tstride, q, r, J);
        if (a.jac) {
            char* dst = a.jac + b * a.jac_bstride + i * a.jac_stride[0];
#pragma unroll
            for (int h = 0; h < N; ++h)
#pragma unroll
                for (int l = 0; l < N; ++l)
                    *(double*)(dst + h * a.jac_stride[1] + l * a.jac_stride[2]) = J[h][l];
        }
#pragma unroll
        for (int h = 0; h < N; ++h) {
            char* dst = res + i * a.res_stride[0] + h * a.res_stride[1];
            if (a.res_f32)
                *(float*)dst = (float)r[h];
            else
                *(double*)dst = r[h];
        }
        if constexpr (HESS) {
            typedef typename std::conditional<LDS, LdsGrid, GlobalGrid>::type Grid;
            typename Grid::Off toff[N][4];
            double wj[N][4][4];
            jet_weights<N>(a, tstride, q, toff, wj);
            char* dst = ja.hess + b * ja.hess_bstride + i * ja.hess_stride[0];
#pragma unroll
            for (int h = 0; h < N; ++h) {
                double S[4][4][4];
                if constexpr (LDS)
                    jet_sums<N, 2, 2>(LdsGrid{s_grid, per}, h, toff, wj, S);
                else
                    jet_sums<N, 2, 2>(GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, h, toff, wj, S);
                // both halves of a symmetric pair are stored from one accumulator
#pragma unroll
                for (int l = 0; l < N; ++l)
#pragma unroll
                    for (int m = 0; m < N; ++m)
                        *(double*)(dst + h * ja.hess_stride[1] + l * ja.hess_stride[2] + m * ja.hess_stride[3]) =
                            jet_at(S, l, m, -1);
            }
        }
    }
}

template <int N>
hipError_t launch_points_jet(const JetArgs& ja, int nbatch, size_t lds, hipStream_t stream)
{
    const dim3 grid = points_grid(ja.p.npts, nbatch);
    const dim3 block(kPointsThreads);
    if (lds) {
        if (ja.hess)
            hipLaunchKernelGGL((points_jet_kernel<N, true, true>), grid, block, lds, stream, ja);
        else
            hipLaunchKernelGGL((points_jet_kernel<N, true, false>), grid, block, lds, stream, ja);
    } else {
        if (ja.hess)
            hipLaunchKernelGGL((points_jet_kernel<N, false, true>), grid, block, 0, stream, ja);
        else
            hipLaunchKernelGGL((points_jet_kernel<N, false, false>), grid, block, 0, stream, ja);
    }
    return hipGetLastError();
}

// ---- the adjoint ----------------------------------------------------------------------------------------------------

// the cotangents of component h of point i: u_h, A_h[l], G_h[l][m] (zeros for an absent array); false when one of
// them is not finite
template <int N>
__device__ __forceinline__ bool load_cotangents(const JetGradArgs& ga, int64_t b, int64_t i, int h, double& u,
                                                double (&A)[N], double (&G)[N][N])
{
    u = load_cot(ga.du, ga.du_f32, b * ga.du_bstride + i * ga.du_stride[0] + h * ga.du_stride[1]);
    bool finite = isfinite(u);
#pragma unroll
    for (int l = 0; l < N; ++l) {
        A[l] = load_cot(ga.dA, ga.dA_f32,
                        b * ga.dA_bstride + i * ga.dA_stride[0] + h * ga.dA_stride[1] + l * ga.dA_stride[2]);
        finite = finite && isfinite(A[l]);
#pragma unroll
        for (int m = 0; m < N; ++m) {
            G[l][m] = load_cot(ga.dG, ga.dG_f32, b * ga.dG_bstride + i * ga.dG_stride[0] + h * ga.dG_stride[1] +
                                                     l * ga.dG_stride[2] + m * ga.dG_stride[3]);
            finite = finite && isfinite(G[l][m]);
        }
    }
    return finite;
}

template <int N, bool LDS, bool THIRD>
__global__ __launch_bounds__(kPointsThreads) void points_jet_grad_prepare(JetGradArgs ga)
{
    extern __shared__ double s_grid[];
    typedef typename std::conditional<LDS, LdsGrid, GlobalGrid>::type Grid;
    const int64_t b = blockIdx.y;
    PointsArgs& a = ga.p;
    a.g.disp += b * a.disp_bstride;
    const GridGeom& g = a.g;
    int64_t tstride[N];
    int per = 0;
    if constexpr (LDS) {
        if (ga.o.dpts) {                      // (the sums need no derivative of the map)
            per = stage_grid_lds<N>(g, s_grid);
            __syncthreads();
        }
    }
    grid_tap_strides<N, LDS>(g, tstride);
    const char* pts = a.pts + b * a.pts_bstride;
    double maxP = 0.0, maxK = 0.0;
    unsigned long long count = 0ull;          // contributing points
    bool bad = false;

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts;
         i += (int64_t)gridDim.x * blockDim.x) {
        double q[N], row[N];
        load_point<N>(a, pts, i, q);
        const bool contributes = sane_position<N>(a, q);
        const bool sweep = contributes && ga.o.dpts;
        typename Grid::Off toff[N][4];
        double wj[N][4][4];
        if (sweep)
            jet_weights<N>(a, tstride, q, toff, wj);
        bool cfinite = true;
        double bP = 0.0, bK = 0.0;
#pragma unroll
        for (int p = 0; p < N; ++p)
            row[p] = 0.0;
#pragma unroll
        for (int h = 0; h < N; ++h) {
            double u, A[N], G[N][N];
            cfinite = load_cotangents<N>(ga, b, i, h, u, A, G) && cfinite;
            // what this component can add to one cell of dP and of dK
            double tP = fabs(u), tK = fabs(u);
#pragma unroll
            for (int l = 0; l < N; ++l) {
                tP += 1.5 * a.scale[l] * fabs(A[l]);
                const double k = fabs(u * q[l]) + fabs(A[l]);
                tK = k > tK ? k : tK;
#pragma unroll
                for (int m = 0; m < N; ++m)
                    tP += (l == m ? 4.0 : 2.25) * a.scale[l] * a.scale[m] * fabs(G[l][m]);
            }
            bP = tP > bP ? tP : bP;
            bK = tK > bK ? tK : bK;
            if (sweep) {
                double S[4][4][4];
                if constexpr (LDS)
                    jet_sums<N, 1, THIRD ? 3 : 2>(LdsGrid{s_grid, per}, h, toff, wj, S);
                else
                    jet_sums<N, 1, THIRD ? 3 : 2>(GlobalGrid{g.disp, g.disp_stride[0], g.disp_dtype}, h, toff, wj, S);
#pragma unroll
                for (int p = 0; p < N; ++p) {
                    const double Khp = g.has_affine ? g.affine[h * (N + 1) + p] : (h == p ? 1.0 : 0.0);
                    double acc = u * (Khp + jet_at(S, p, -1, -1));
#pragma unroll
                    for (int l = 0; l < N; ++l) {
                        acc += A[l] * jet_at(S, l, p, -1);
                        if constexpr (THIRD) {
#pragma unroll
                            for (int m = 0; m < N; ++m)
                                acc += G[l][m] * jet_at(S, l, m, p);
                        }
                    }
                    row[p] += acc;
                }
            }
        }
        if (contributes) {
            if (!cfinite) {
                bad = true;
            } else {
                ++count;
                maxP = bP > maxP ? bP : maxP;
                maxK = bK > maxK ? bK : maxK;
            }
        }
        if (ga.o.dpts)
            store_point_row<N>(ga.o, b, i, row);
    }
    publish_head(ga.o.head + b * kGradHead, maxP, maxK, bad, count);
}

template <int N, bool LDS>
__global__ __launch_bounds__(kPointsThreads) void points_jet_grad_scatter(JetGradArgs ga)
{
    extern __shared__ unsigned long long s_cells[];   // LDS: the dP cells of this workgroup
    const int64_t b = blockIdx.y;
    const PointsArgs& a = ga.p;
    const GridGeom& g = a.g;
    constexpr int NK = N * (N + 1);
    unsigned long long* cellsK = ga.o.cells + b * ga.o.cells_per;
    unsigned long long* cellsP = cellsK + NK;
    int eP, eK, sP, sK;
    grad_quanta<true>(ga.o.head + b * kGradHead, eP, eK, sP, sK);
    const bool wantP = sP > 0 && ga.o.ddisp != nullptr;
    const bool wantK = sK > 0 && ga.o.dK != nullptr;
    if (!wantP && !wantK)
        return;                                       // (uniform over the workgroup)
    int64_t cstride[N];
    const int64_t per = scatter_begin<N, LDS>(g, ga.o, wantP, s_cells, cstride);
    const char* pts = a.pts + b * a.pts_bstride;
    unsigned long long accK[NK];
#pragma unroll
    for (int e = 0; e < NK; ++e)
        accK[e] = 0ull;

    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts;
         i += (int64_t)gridDim.x * blockDim.x) {
        double q[N];
        load_point<N>(a, pts, i, q);
        bool finite = true;
#pragma unroll
        for (int h = 0; h < N; ++h) {
            double u, A[N], G[N][N];
            finite = load_cotangents<N>(ga, b, i, h, u, A, G) && finite;
        }
        // a non-finite cotangent has set the sample's flag; a position that is not sane has no exact tap index
        if (!finite || !sane_position<N>(a, q))
            continue;
        int64_t toff[N][4];
        double wj[N][4][4];
        if (wantP)
            jet_weights<N>(a, cstride, q, toff, wj);
#pragma unroll
        for (int h = 0; h < N; ++h) {
            double u, A[N], G[N][N];
            load_cotangents<N>(ga, b, i, h, u, A, G);
            if (wantK) {
#pragma unroll
                for (int l = 0; l < N; ++l)
                    accK[h * (N + 1) + l] += quantise(u * q[l] + A[l], 62 - eK);
                accK[h * (N + 1) + N] += quantise(u, 62 - eK);
            }
            if (!wantP)
                continue;
            auto add = [&](int64_t off, double c) {
                const unsigned long long v = quantise(c, 62 - eP);
                if constexpr (LDS)
                    atomicAdd(&s_cells[h * per + off], v);
                else
                    atomicAdd(&cellsP[h * per + off], v);
            };
            // the tap's coefficient u W + sum_l A_l d_l W + sum_lm G_lm d_l d_m W, factored axis by axis
            if constexpr (N == 1) {
#pragma unroll
                for (int t0 = 0; t0 < 4; ++t0)
                    add(toff[0][t0], u * wj[0][0][t0] + A[0] * wj[0][1][t0] + G[0][0] * wj[0][2][t0]);
            } else if constexpr (N == 2) {
                const double G01 = G[0][1] + G[1][0];
#pragma unroll
                for (int t0 = 0; t0 < 4; ++t0) {
                    const double w0 = wj[0][0][t0], d0 = wj[0][1][t0], D0 = wj[0][2][t0];
                    const double e0 = u * w0 + A[0] * d0 + G[0][0] * D0;
                    const double e1 = A[1] * w0 + G01 * d0;
                    const double e2 = G[1][1] * w0;
#pragma unroll
                    for (int t1 = 0; t1 < 4; ++t1)
                        add(toff[0][t0] + toff[1][t1], e0 * wj[1][0][t1] + e1 * wj[1][1][t1] + e2 * wj[1][2][t1]);
                }
            } else {
                const double G01 = G[0][1] + G[1][0], G02 = G[0][2] + G[N - 1][0], G12 = G[1][N - 1] + G[N - 1][1];
                const double G22 = G[N - 1][N - 1], A2 = A[N - 1];
                // the outermost tap loop stays rolled, its weights and offset rotating through scalars
                Rot4<double> w0{wj[0][0][0], wj[0][0][1], wj[0][0][2], wj[0][0][3]};
                Rot4<double> d0{wj[0][1][0], wj[0][1][1], wj[0][1][2], wj[0][1][3]};
                Rot4<double> D0{wj[0][2][0], wj[0][2][1], wj[0][2][2], wj[0][2][3]};
                Rot4<int64_t> o0{toff[0][0], toff[0][1], toff[0][2], toff[0][3]};
#pragma unroll 1
                for (int t0 = 0; t0 < 4; ++t0) {
                    const double e0 = u * w0.a + A[0] * d0.a + G[0][0] * D0.a;
                    const double e1 = A[1] * w0.a + G01 * d0.a;
                    const double e2 = G[1][1] * w0.a;
                    const double f0 = A2 * w0.a + G02 * d0.a;
                    const double f1 = G12 * w0.a;
                    const double g0 = G22 * w0.a;
#pragma unroll
                    for (int t1 = 0; t1 < 4; ++t1) {
                        const double w1 = wj[1][0][t1], d1 = wj[1][1][t1], D1 = wj[1][2][t1];
                        const double al = e0 * w1 + e1 * d1 + e2 * D1;
                        const double be = f0 * w1 + f1 * d1;
                        const double ga2 = g0 * w1;
#pragma unroll
                        for (int t2 = 0; t2 < 4; ++t2)
                            add(o0.a + toff[1][t1] + toff[N - 1][t2],
                                al * wj[N - 1][0][t2] + be * wj[N - 1][1][t2] + ga2 * wj[N - 1][2][t2]);
                    }
                    w0.turn(), d0.turn(), D0.turn(), o0.turn();
                }
            }
        }
    }
    scatter_end<N, LDS>(ga.o, wantP, wantK, accK, s_cells, cellsK);
}

// prepare and scatter over npts > 0 points
template <int N>
hipError_t launch_points_jet_grad(const JetGradArgs& ga, int nbatch, bool lds, hipStream_t stream)
{
    const dim3 block(kPointsThreads);
    const GradSums& o = ga.o;
    const dim3 grid = points_grid(ga.p.npts, nbatch);
    const size_t grid_lds = lds && o.dpts ? (size_t)o.values * sizeof(double) : 0;
    if (lds) {
        if (ga.dG)
            hipLaunchKernelGGL((points_jet_grad_prepare<N, true, true>), grid, block, grid_lds, stream, ga);
        else
            hipLaunchKernelGGL((points_jet_grad_prepare<N, true, false>), grid, block, grid_lds, stream, ga);
    } else {
        if (ga.dG)
            hipLaunchKernelGGL((points_jet_grad_prepare<N, false, true>), grid, block, 0, stream, ga);
        else
            hipLaunchKernelGGL((points_jet_grad_prepare<N, false, false>), grid, block, 0, stream, ga);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || (!o.ddisp && !o.dK))
        return e;
    if (lds)
        hipLaunchKernelGGL((points_jet_grad_scatter<N, true>), grid, block,
                           o.ddisp ? (size_t)o.values * sizeof(unsigned long long) : 0, stream, ga);
    else
        hipLaunchKernelGGL((points_jet_grad_scatter<N, false>), grid, block, 0, stream, ga);
    return hipGetLastError();
}

bool jet_call_ok(const GridGeom& g, int nbatch)
{
    return g.naxis >= 1 && g.naxis <= kJetMaxAxes && nbatch <= 65535;
}

}  // namespace

hipError_t launch_deform_points_derivatives(const PointsJetCall& c, hipStream_t stream)
{
    if (!jet_call_ok(c.g, c.nbatch))
        return hipErrorNotSupported;
    if (c.npts <= 0 || c.nbatch <= 0)
        return hipSuccess;                    // nothing to launch
    JetArgs ja;
    memset(&ja, 0, sizeof(ja));
    PointsArgs& a = ja.p;
    const int64_t values = fill_points_args(a, c.g, c.disp_bstride, nullptr, 0, 0.0);
    unpack(c.pts, a.pts, a.pts_stride, a.pts_bstride);
    unpack(c.res, a.res, a.res_stride, a.res_bstride);
    unpack(c.jac, a.jac, a.jac_stride, a.jac_bstride);
    unpack(c.hess, ja.hess, ja.hess_stride, ja.hess_bstride);
    a.pts_f32 = c.pts.dtype == EDHIP_F32;
    a.res_f32 = c.res.dtype == EDHIP_F32;
    a.npts = c.npts;
    const size_t lds = values <= kPointsLdsValues ? (size_t)values * sizeof(double) : 0;
    switch (c.g.naxis) {
    case 1: return launch_points_jet<1>(ja, c.nbatch, lds, stream);
    case 2: return launch_points_jet<2>(ja, c.nbatch, lds, stream);
    default: return launch_points_jet<3>(ja, c.nbatch, lds, stream);
    }
}

size_t points_jet_scratch_bytes(const GridGeom& g, int nbatch)
{
    return (size_t)nbatch * (size_t)(kGradHead + points_grad_cells_per(g)) * 8;
}

hipError_t launch_deform_points_derivatives_gradient(const PointsJetGradCall& c, hipStream_t stream)
{
    if (!jet_call_ok(c.g, c.nbatch))
        return hipErrorNotSupported;
    if (c.nbatch <= 0)
        return hipSuccess;
    JetGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    PointsArgs& a = ga.p;
    fill_points_args(a, c.g, c.disp_bstride, nullptr, 0, 0.0);
    unpack(c.pos, a.pts, a.pts_stride, a.pts_bstride);
    unpack(c.du, ga.du, ga.du_stride, ga.du_bstride);
    unpack(c.dA, ga.dA, ga.dA_stride, ga.dA_bstride);
    unpack(c.dG, ga.dG, ga.dG_stride, ga.dG_bstride);
    a.pts_f32 = c.pos.dtype == EDHIP_F32;
    ga.du_f32 = c.du.dtype == EDHIP_F32;
    ga.dA_f32 = c.dA.dtype == EDHIP_F32;
    ga.dG_f32 = c.dG.dtype == EDHIP_F32;
    a.npts = c.npts;
    const bool lds = fill_grad_sums(ga.o, c.dpts, c.ddisp, c.dK, c.g, c.scratch, c.nbatch);
    hipError_t e = launch_points_grad_clear(c.g, c.nbatch, c.scratch, stream);
    if (e != hipSuccess)
        return e;
    if (c.npts > 0) {
        switch (c.g.naxis) {
        case 1: e = launch_points_jet_grad<1>(ga, c.nbatch, lds, stream); break;
        case 2: e = launch_points_jet_grad<2>(ga, c.nbatch, lds, stream); break;
        default: e = launch_points_jet_grad<3>(ga, c.nbatch, lds, stream); break;
        }
        if (e != hipSuccess)
            return e;
    }
    return launch_points_grad_finish(c.g, c.nbatch, c.ddisp, c.dK, c.scratch, true, stream);
}

}  // namespace ed
