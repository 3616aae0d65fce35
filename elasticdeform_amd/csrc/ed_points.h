// ed_points.h -- what the kernels of deform_points.hip (the coordinate map at real positions and its inverse), of
// deform_points_grad.hip (their adjoint) and of deform_unwarp.hip / deform_unwarp_grad.hip (an image resampled back
// through the deformation, and the adjoint of that) share: the argument block, the launch shape, the control grid's
// readers, the position load and the tap strides, the separable tap sum, r(q) with its Jacobian, the n x n solve and
// the damped Newton inversion.  Notation: the head of deform_points.hip.
#pragma once

#include <cmath>

#include "ed_device.h"
#include "ed_exact_coord.h"
#include "ed_params.h"

namespace ed {

namespace {

constexpr int kPointsThreads = 256;
constexpr int kPointsMaxBlocks = 2048;        // per sample; points beyond blocks * threads: grid-stride loop
constexpr int kPointsMaxHalvings = 10;
constexpr double kPointsMaxCoordinate = 4e15; // |control coordinate| below 2^52: floor() and the tap index are exact

struct PointsArgs {
    GridGeom g;                               // g.disp: the prefiltered grid of sample 0; out_len / nvox unused
    int64_t disp_bstride;
    const char* pts;                          // (npts, naxis) float32 / float64
    int pts_f32;
    int64_t pts_stride[2], pts_bstride;
    char* res;                                // (npts, naxis) float32 / float64
    int res_f32;
    int64_t res_stride[2], res_bstride;
    char* jac;                                // forward: (npts, naxis, naxis) float64, or nullptr
    int64_t jac_stride[3], jac_bstride;
    unsigned char* status;                    // inverse: (npts) uint8, or nullptr
    int64_t status_stride, status_bstride;
    int64_t npts;
    double scale[kMaxAxes];                   // (ncp_k - 1) / (I_k - 1)
    double minv[kMaxAxes * kMaxAxes];         // inverse: M = (K[:, :n])^-1, row-major (identity without affine)
    int max_iter;
    double tol;
};

// ---- host: what the three launchers share ----------------------------------------------------------------------------
// The part of PointsArgs that every launcher fills alike: g, disp_bstride, scale, minv, max_iter, tol.  Returns the
// number of control-grid values, naxis prod ncp_k (up to kPointsLdsValues of them are staged in LDS).
inline int64_t fill_points_args(PointsArgs& a, const GridGeom& g, int64_t disp_bstride, const double* forward_linear,
                                int max_iter, double tol)
{
    const int n = g.naxis;
    a.g = g;
    a.disp_bstride = disp_bstride;
    a.max_iter = max_iter;
    a.tol = tol;
    int64_t values = n;
    for (int k = 0; k < n; ++k) {
        a.scale[k] = (double)(g.ncp[k] - 1) / (double)(g.in_len[k] - 1);
        values *= g.ncp[k];
        for (int l = 0; l < n; ++l)
            a.minv[k * n + l] = forward_linear ? forward_linear[k * n + l] : (k == l ? 1.0 : 0.0);
    }
    return values;
}

// a BatchArray into the (pointer, strides, batch stride) fields of a kernel argument block
template <typename P, int R>
inline void unpack(const BatchArray& s, P*& ptr, int64_t (&stride)[R], int64_t& bstride)
{
    ptr = (P*)s.ptr;
    for (int k = 0; k < R; ++k)
        stride[k] = s.stride[k];
    bstride = s.bstride;
}
template <typename P>
inline void unpack(const BatchArray& s, P*& ptr, int64_t& stride, int64_t& bstride)
{
    ptr = (P*)s.ptr;
    stride = s.stride[0];
    bstride = s.bstride;
}

// the launch shape of the per-point kernels: blocks of kPointsThreads over the points of one sample (a grid-stride
// loop beyond kPointsMaxBlocks of them), blockIdx.y = sample
inline dim3 points_grid(int64_t npts, int nbatch)
{
    const int64_t want = (npts + kPointsThreads - 1) / kPointsThreads;
    return dim3((unsigned)(want < kPointsMaxBlocks ? want : kPointsMaxBlocks), (unsigned)nbatch);
}

constexpr int ipow4(int e) { return e == 0 ? 1 : 4 * ipow4(e - 1); }

// a[t] for a runtime t without indexing a register array dynamically
template <typename T>
__device__ __forceinline__ T pick4(const T (&a)[4], int t)
{
    T r = a[0];
    r = t == 1 ? a[1] : r;
    r = t == 2 ? a[2] : r;
    r = t == 3 ? a[3] : r;
    return r;
}

// the control grid as the evaluator reads it: doubles in LDS (component-major, C order) or the caller's array
struct LdsGrid {
    typedef int Off;                          // tap offsets: elements of the LDS copy
    const double* s;
    int per;
    __device__ __forceinline__ double operator()(int h, int off) const { return s[h * per + off]; }
};
struct GlobalGrid {
    typedef int64_t Off;                      // bytes of the caller's array
    const char* base;
    int64_t hstride;
    int dtype;
    __device__ __forceinline__ double operator()(int h, int64_t off) const
    {
        return load_as_double(base + h * hstride + off, dtype);
    }
};

// point i of a sample's positions (`pts`: the sample's first row), widened to fp64
template <int N>
__device__ __forceinline__ void load_point(const PointsArgs& a, const char* pts, int64_t i, double (&q)[N])
{
#pragma unroll
    for (int h = 0; h < N; ++h) {
        const char* src = pts + i * a.pts_stride[0] + h * a.pts_stride[1];
        q[h] = a.pts_f32 ? (double)*(const float*)src : *(const double*)src;
    }
}

// tap strides of the evaluator: elements of the LDS copy (C order), or bytes of the caller's grid
template <int N, bool LDS>
__device__ __forceinline__ void grid_tap_strides(const GridGeom& g, int64_t (&tstride)[N])
{
    if constexpr (LDS) {
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
}

// Separable tap sum over grid axes D..N-1 (every loop unrolled but the outermost of three):
//   v     = sum_t C[t] prod_e w_e
//   dv[l] = sum_t C[t] dw_l prod_{e != l} w_e        (l >= D)
template <int N, int D, typename Grid>
__device__ __forceinline__ void grid_taps(const Grid& grid, int h, typename Grid::Off off,
                                          const typename Grid::Off (&toff)[N][4],
                                          const double (&w)[N][4], const double (&dw)[N][4], double& v,
                                          double (&dv)[N])
{
    if constexpr (D == N) {
        v = grid(h, off);
    } else {
        v = 0.0;
#pragma unroll
        for (int l = D; l < N; ++l)
            dv[l] = 0.0;
        if constexpr (N - D >= 3) {
            // the outermost tap loop of the 3-axis sum stays rolled: 16 grid reads per turn.  Unrolled too, the
            // compiler issues all 64 x 3 reads in front of the arithmetic and takes every register there is (256 + 122
            // accumulation registers, one wave per SIMD).  The turn's weights and offset rotate through scalars: a
            // select on the loop counter is turned back into an indexed read, which puts the arrays into scratch.
            double w0 = w[D][0], w1 = w[D][1], w2 = w[D][2], w3 = w[D][3];
            double d0 = dw[D][0], d1 = dw[D][1], d2 = dw[D][2], d3 = dw[D][3];
            typename Grid::Off o0 = toff[D][0], o1 = toff[D][1], o2 = toff[D][2], o3 = toff[D][3];
#pragma unroll 1
            for (int t = 0; t < 4; ++t) {
                double sv;
                double sdv[N];
                grid_taps<N, D + 1>(grid, h, off + o0, toff, w, dw, sv, sdv);
                v += w0 * sv;
                dv[D] += d0 * sv;
#pragma unroll
                for (int l = D + 1; l < N; ++l)
                    dv[l] += w0 * sdv[l];
                const double wr = w0, dr = d0;
                const typename Grid::Off orot = o0;
                w0 = w1, w1 = w2, w2 = w3, w3 = wr;
                d0 = d1, d1 = d2, d2 = d3, d3 = dr;
                o0 = o1, o1 = o2, o2 = o3, o3 = orot;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                double sv;
                double sdv[N];
                grid_taps<N, D + 1>(grid, h, off + toff[D][t], toff, w, dw, sv, sdv);
                v += w[D][t] * sv;
                dv[D] += dw[D][t] * sv;
#pragma unroll
                for (int l = D + 1; l < N; ++l)
                    dv[l] += w[D][t] * sdv[l];
            }
        }
    }
}

// r(q) and J(q).  tstride[k]: distance between neighbours along grid axis k in the units Grid takes (elements of the
// LDS copy, bytes of the caller's array).
template <int N, typename Grid>
__device__ __forceinline__ void eval_map(const PointsArgs& a, const Grid& grid, const int64_t (&tstride)[N],
                                         const double (&q)[N], double (&r)[N], double (&J)[N][N])
{
    const GridGeom& g = a.g;
    typename Grid::Off toff[N][4];
    double w[N][4], dw[N][4];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double cpq = (double)(g.ncp[k] - 1) * (q[k] + (double)g.off[k]) / (double)(g.in_len[k] - 1);
        // a position that is not finite, or too far out for the tap index to be an exact integer: the taps of
        // position 0 (inside the grid) with NaN weights, so that the result is NaN and nothing is read out of range
        const bool sane = fabs(cpq) < kPointsMaxCoordinate;
        const double cp = sane ? cpq : 0.0;
        const int64_t start = window_start(cp, 3);
        spline_weights(cp, 3, w[k]);
        spline_weight_derivatives(cp, 3, dw[k]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            toff[k][t] = (typename Grid::Off)(mirror_index(start + t, g.ncp[k]) * tstride[k]);
            w[k][t] = sane ? w[k][t] : NAN;
            dw[k][t] = sane ? dw[k][t] * a.scale[k] : NAN;
        }
    }
    double d[N];
    if constexpr (N <= 3) {
#pragma unroll
        for (int h = 0; h < N; ++h)
            grid_taps<N, 0>(grid, h, 0, toff, w, dw, d[h], J[h]);
    } else {
        // many axes (performance does not matter there): an odometer over the 4^N taps
#pragma unroll
        for (int h = 0; h < N; ++h) {
            d[h] = 0.0;
#pragma unroll
            for (int l = 0; l < N; ++l)
                J[h][l] = 0.0;
        }
        int t[N];
#pragma unroll
        for (int k = 0; k < N; ++k)
            t[k] = 0;
        for (int tap = 0; tap < ipow4(N); ++tap) {
            typename Grid::Off off = 0;
            double wv[N], dwv[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                off += pick4(toff[k], t[k]);
                wv[k] = pick4(w[k], t[k]);
                dwv[k] = pick4(dw[k], t[k]);
            }
            double prod = 1.0;
            double dprod[N];
#pragma unroll
            for (int k = 0; k < N; ++k)
                prod *= wv[k];
#pragma unroll
            for (int l = 0; l < N; ++l) {
                double p = dwv[l];
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (e != l)
                        p *= wv[e];
                dprod[l] = p;
            }
#pragma unroll
            for (int h = 0; h < N; ++h) {
                const double c = grid(h, off);
                d[h] += c * prod;
#pragma unroll
                for (int l = 0; l < N; ++l)
                    J[h][l] += c * dprod[l];
            }
            bool carry = true;
#pragma unroll
            for (int k = N - 1; k >= 0; --k) {
                if (carry) {
                    t[k] = t[k] < 3 ? t[k] + 1 : 0;
                    carry = t[k] == 0;
                }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < N; ++h) {
        double cc;
        if (g.has_affine) {
            cc = 0.0;
#pragma unroll
            for (int l = 0; l < N; ++l) {
                cc += g.affine[h * (N + 1) + l] * q[l];
                J[h][l] += g.affine[h * (N + 1) + l];
            }
            cc += g.affine[h * (N + 1) + N];
        } else {
            cc = q[h];
            J[h][h] += 1.0;
        }
        r[h] = cc + (double)g.off[h] + d[h];
    }
}

// s with J s = b; false when J is singular (or not finite)
template <int N>
__device__ __forceinline__ bool solve(const double (&J)[N][N], const double (&b)[N], double (&s)[N])
{
    if constexpr (N == 1) {
        s[0] = b[0] / J[0][0];
        return J[0][0] != 0.0 && isfinite(s[0]);
    } else if constexpr (N == 2) {
        const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        s[0] = (J[1][1] * b[0] - J[0][1] * b[1]) / det;
        s[1] = (J[0][0] * b[1] - J[1][0] * b[0]) / det;
        return det != 0.0 && isfinite(s[0]) && isfinite(s[1]);
    } else if constexpr (N == 3) {
        // adjugate: cofactors of J, expanded along the first row
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
        const double c10 = J[0][2] * J[2][1] - J[0][1] * J[2][2];
        const double c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0];
        const double c12 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
        const double c20 = J[0][1] * J[1][2] - J[0][2] * J[1][1];
        const double c21 = J[0][2] * J[1][0] - J[0][0] * J[1][2];
        const double c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        s[0] = (c00 * b[0] + c10 * b[1] + c20 * b[2]) / det;
        s[1] = (c01 * b[0] + c11 * b[1] + c21 * b[2]) / det;
        s[2] = (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det;
        return det != 0.0 && isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]);
    } else {
        // Gaussian elimination with partial pivoting on the augmented matrix
        double A[N][N + 1];
        for (int i = 0; i < N; ++i) {
            for (int j = 0; j < N; ++j)
                A[i][j] = J[i][j];
            A[i][N] = b[i];
        }
        for (int c = 0; c < N; ++c) {
            int piv = c;
            double best = fabs(A[c][c]);
            for (int i = c + 1; i < N; ++i) {
                const double v = fabs(A[i][c]);
                if (v > best) {
                    best = v;
                    piv = i;
                }
            }
            if (!(best > 0.0) || !isfinite(best))
                return false;
            if (piv != c) {
                for (int j = c; j <= N; ++j) {
                    const double tmp = A[c][j];
                    A[c][j] = A[piv][j];
                    A[piv][j] = tmp;
                }
            }
            for (int i = c + 1; i < N; ++i) {
                const double f = A[i][c] / A[c][c];
                for (int j = c; j <= N; ++j)
                    A[i][j] -= f * A[c][j];
            }
        }
        bool ok = true;
        for (int i = N - 1; i >= 0; --i) {
            double acc = A[i][N];
            for (int j = i + 1; j < N; ++j)
                acc -= A[i][j] * s[j];
            s[i] = acc / A[i][i];
            ok = ok && isfinite(s[i]);
        }
        return ok;
    }
}

template <int N>
__device__ __forceinline__ double max_norm_diff(const double (&r)[N], const double (&p)[N])
{
    double m = 0.0;
    bool bad = false;
#pragma unroll
    for (int h = 0; h < N; ++h) {
        const double e = fabs(r[h] - p[h]);
        bad = bad || !(e == e);
        m = e > m ? e : m;
    }
    return bad ? INFINITY : m;
}

// q with r(q) = p; false: no solution reached (see the head of deform_points.hip)
template <int N, typename Grid>
__device__ __forceinline__ bool invert_map(const PointsArgs& a, const Grid& grid, const int64_t (&tstride)[N],
                                           const double (&p)[N], double (&q)[N])
{
    const GridGeom& g = a.g;
    double b[N], s[N], trial[N];
    bool finite = true;
#pragma unroll
    for (int h = 0; h < N; ++h) {
        finite = finite && isfinite(p[h]);
        b[h] = p[h] - (double)g.off[h] - (g.has_affine ? g.affine[h * (N + 1) + N] : 0.0);
    }
    if (!finite)
        return false;
#pragma unroll
    for (int h = 0; h < N; ++h) {
        if (g.has_affine) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < N; ++l)
                acc += a.minv[h * N + l] * b[l];
            trial[h] = acc;
        } else {
            trial[h] = b[h];
        }
        s[h] = 0.0;
    }
    double res = INFINITY, lambda = 1.0;
    int steps = 0, halvings = 0;
    bool first = true;
    // one evaluation per turn: of the start, of a full Newton step, or of a halved one
    for (;;) {
        double r[N], J[N][N];
        eval_map<N>(a, grid, tstride, trial, r, J);
        const double rt = max_norm_diff<N>(r, p);
        if (rt < res) {
            // accepted (the start, or a step that lowers the residual)
#pragma unroll
            for (int h = 0; h < N; ++h)
                q[h] = trial[h];
            res = rt;
            if (res <= a.tol)
                return true;
            if (steps == a.max_iter)
                return false;
            double e[N];
#pragma unroll
            for (int h = 0; h < N; ++h)
                e[h] = r[h] - p[h];
            if (!solve<N>(J, e, s))
                return false;
            ++steps;
            lambda = 1.0;
            halvings = 0;
        } else {
            if (first || halvings == kPointsMaxHalvings)
                return false;             // a start that is not finite, or an exhausted backtrack
            ++halvings;
            lambda *= 0.5;
        }
        first = false;
#pragma unroll
        for (int h = 0; h < N; ++h)
            trial[h] = q[h] - lambda * s[h];
    }
}

}  // namespace

}  // namespace ed
