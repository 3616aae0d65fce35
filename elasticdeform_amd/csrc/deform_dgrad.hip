// deform_dgrad.hip -- gradient of the deformation with respect to the control-point displacement.
//
// For one call (the forward of deform.c:639-924, prefiltered grid P):
//   beta(o, j)  = prod_d b_d(o_d, j_d)       cubic weights of control point j at output voxel o (taps mirror-folded)
//   c_h(o)      = (A o)_h + s_h + sum_j P[h, j] beta(o, j)
//   m_h         = map_coordinate(c_h, L_h, mode_i)
//   g_h(o)      = sum_i sum_step dY_i[o, step] map'_h sum_k C_i[k, step] w'_h(m_h, k_h) prod_{e != h} w_e(m_e, k_e)
//   dP[h, j]    = sum_o g_h(o) beta(o, j)
// beta is separable and depends on o alone, so dP is a banded contraction of the g field, axis by axis:
//
//   dgrad_rows_kernel      one workgroup per output row (o_0 .. o_{n-2} fixed, o_{n-1} runs), blockIdx.y = sample.
//                          The row's displacement is Q[h, j_last] = sum_{j_0..j_{n-2}} P[h, j] prod_{d<n-1} b_d:
//                          a voxel's delta is then 4 taps of Q.  Per voxel g_h (fp64 coordinates and weights,
//                          tap sums in the volume's type, fp64 across steps and inputs), then g_h contracted
//                          with the row's band of b_{n-1} in LDS, in a fixed order -> part[b][row][h][j_last].
//   dgrad_contract_kernel  one launch per remaining axis, innermost first: [outer][L_d][inner] ->
//                          [outer][ncp_d][inner], one wavefront per output, the o_d sum in a fixed order.
//   dgrad_finish_kernel    [b][j_0..j_{n-2}][h][j_last] -> dP[b][h][j_0..j_{n-1}] in the destination's dtype.
//
// Gradient with respect to the inverse map K (n x (n+1)) the coordinate applies, c_h = sum_l K[h,l] o_l + K[h,n] + ...:
//   dK[h, l] = sum_o g_h(o) o_l        dK[h, n] = sum_o g_h(o)
// The row kernel (template flag AK) also leaves per row the moments S0_h = sum g_h and S1_h = sum g_h o_{n-1} along
// the row -> mom[b][row][h][2], built from the LDS copy of g (one xor butterfly per wave, the waves' sums in their
// own LDS slots chunk after chunk, the waves added in order at the end); then
//   dgrad_affine_reduce_kernel  256 rows per workgroup: dK[h, l < n-1] = o_l S0_h, dK[h, n-1] = S1_h, dK[h, n] = S0_h
//                               summed by a butterfly per wave and the waves in order -> one partial per workgroup
//   dgrad_affine_store_kernel   one wavefront per (output, sample): the partials in a fixed order -> dK (fp64)
//
// No atomics, no counters: every sum has one fixed order, so the result is the same bits from run to run, and a
// sample of a batch is the same bits as the single call.  No host synchronisation; the launches are capturable.
#include <cstring>

#include "ed_device.h"
#include "ed_params.h"

namespace ed {

namespace {

constexpr int kRowThreads = 256;          // largest row workgroup (the LDS arrays are sized for it)

struct RowArgs {
    GridGeom g;
    IOView v;
    double* part;                         // [nbatch][rows][K]; nullptr (AK kernels only): no displacement result
    int64_t rows;
    int K;                                // naxis * ncp_{naxis-1}
    int accumulate;                       // add to part (second and later inputs) instead of overwriting it
    int64_t in_bstride, out_bstride, disp_bstride;
    double* mom;                          // AK kernels: [nbatch][rows][naxis][2] row moments (S0_h, S1_h)
};

// sum over the 64 lanes of a wavefront by a fixed xor butterfly (every lane ends with the same bits)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        v += __shfl_xor(v, m, 64);
    return v;
}

// pick a[t] for a runtime t without indexing a register array dynamically
template <typename T, int M>
__device__ __forceinline__ T pick(const T (&a)[M], int t)
{
    T r = a[0];
#pragma unroll
    for (int i = 1; i < M; ++i)
        r = t == i ? a[i] : r;
    return r;
}

constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

// Separable tap sum over axes D..N-1 (order P, every loop unrolled):
//   v     = sum_k C[k] prod_e w_e
//   dv[h] = sum_k C[k] dw_h prod_{e != h} w_e        (h >= D)
template <typename T, int N, int P, int D>
__device__ __forceinline__ void tap_sep(const char* base, const int64_t (&koff)[N][P + 1], const T (&w)[N][P + 1],
                                        const T (&dw)[N][P + 1], T& v, T (&dv)[N])
{
    if constexpr (D == N) {
        v = *(const T*)base;
    } else {
        v = T(0);
#pragma unroll
        for (int h = D; h < N; ++h)
            dv[h] = T(0);
#pragma unroll
        for (int t = 0; t <= P; ++t) {
            T sv;
            T sdv[N];
            tap_sep<T, N, P, D + 1>(base + koff[D][t], koff, w, dw, sv, sdv);
            v += w[D][t] * sv;
            dv[D] += dw[D][t] * sv;
#pragma unroll
            for (int h = D + 1; h < N; ++h)
                dv[h] += w[D][t] * sdv[h];
        }
    }
}

__device__ __forceinline__ double load_dy(const char* p, int dt)
{
    return dt == EDHIP_F32 ? (double)*(const float*)p : *(const double*)p;
}

// flattened step index -> byte offsets into the input and into dY
__device__ __forceinline__ void step_offsets(const IOView& v, int64_t s, int64_t& ioff, int64_t& ooff)
{
    ioff = 0;
    ooff = 0;
#pragma unroll
    for (int k = 0; k < kMaxSteps; ++k) {
        if (k < v.nstep) {
            const int64_t i = s % v.step_len[k];
            s /= v.step_len[k];
            ioff += i * v.in_step_stride[k];
            ooff += i * v.out_step_stride[k];
        }
    }
}

// g[h] += sum_step dY[o, step] * slope_h * dv_h(step) for one input of order P
template <typename T, int N, int P>
__device__ __forceinline__ void voxel_taps(const RowArgs& a, const char* in, const char* dy, const double (&m)[N],
                           const double (&slope)[N], double (&g)[N])
{
    const IOView& v = a.v;
    if constexpr (N <= 3) {
        int64_t koff[N][P + 1];
        T w[N][P + 1], dw[N][P + 1];
#pragma unroll
        for (int d = 0; d < N; ++d) {
            double wd[P + 1], dwd[P + 1];
            spline_weights(m[d], P, wd);
            spline_weight_derivatives(m[d], P, dwd);
            const int64_t s = window_start(m[d], P);
#pragma unroll
            for (int t = 0; t <= P; ++t) {
                koff[d][t] = mirror_index(s + t, a.g.in_len[d]) * v.in_stride[d];
                w[d][t] = (T)wd[t];
                dw[d][t] = (T)(dwd[t] * slope[d]);
            }
        }
        for (int64_t s = 0; s < v.nsteps; ++s) {
            int64_t ioff, ooff;
            step_offsets(v, s, ioff, ooff);
            const double y = load_dy(dy + ooff, v.out_dtype);
            T val;
            T dv[N];
            tap_sep<T, N, P, 0>(in + ioff, koff, w, dw, val, dv);
#pragma unroll
            for (int h = 0; h < N; ++h)
                g[h] += y * (double)dv[h];
        }
    } else {
        // many axes (performance does not matter there): an odometer over the (P+1)^N taps that recomputes the
        // weights of each tap instead of keeping N x (P+1) of them in registers
        int64_t st[N];
#pragma unroll
        for (int d = 0; d < N; ++d)
            st[d] = window_start(m[d], P);
        for (int64_t s = 0; s < v.nsteps; ++s) {
            int64_t ioff, ooff;
            step_offsets(v, s, ioff, ooff);
            const double y = load_dy(dy + ooff, v.out_dtype);
            T dv[N];
            int t[N];
#pragma unroll
            for (int d = 0; d < N; ++d) {
                dv[d] = T(0);
                t[d] = 0;
            }
            for (int tap = 0; tap < ipow(P + 1, N); ++tap) {
                int64_t off = ioff;
                T wv[N], dwv[N];
#pragma unroll
                for (int d = 0; d < N; ++d) {
                    double wd[P + 1], dwd[P + 1];
                    spline_weights(m[d], P, wd);
                    spline_weight_derivatives(m[d], P, dwd);
                    off += mirror_index(st[d] + t[d], a.g.in_len[d]) * v.in_stride[d];
                    wv[d] = (T)pick(wd, t[d]);
                    dwv[d] = (T)(pick(dwd, t[d]) * slope[d]);
                }
                const T c = *(const T*)(in + off);
#pragma unroll
                for (int h = 0; h < N; ++h) {
                    T p = c * dwv[h];
#pragma unroll
                    for (int e = 0; e < N; ++e)
                        if (e != h)
                            p *= wv[e];
                    dv[h] += p;
                }
                bool carry = true;
#pragma unroll
                for (int d = N - 1; d >= 0; --d) {
                    if (carry) {
                        t[d] = t[d] < P ? t[d] + 1 : 0;
                        carry = t[d] == 0;
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < N; ++h)
                g[h] += y * (double)dv[h];
        }
    }
}

// sum_{j_0..j_{n-2}} P[base + j] prod_d b_d(o_d, j_d) over the row's 4^(n-1) grid taps (offsets and weights in LDS)
template <int N, typename Load>
__device__ __forceinline__ double row_coefficient(const char* base, const int64_t* ri, const double* rw, Load load)
{
    auto term = [&](int tap) {
        int64_t off = 0;
        double c = 1.0;
#pragma unroll
        for (int d = N - 2; d >= 0; --d) {
            off += ri[4 * d + (tap & 3)];
            c *= rw[4 * d + (tap & 3)];
            tap >>= 2;
        }
        return c * load(base + off);
    };
    double acc = 0.0;
    if constexpr (N <= 3) {
#pragma unroll
        for (int tap = 0; tap < ipow(4, N - 1); ++tap)
            acc += term(tap);
    } else {
        for (int tap = 0; tap < ipow(4, N - 1); ++tap)
            acc += term(tap);
    }
    return acc;
}

template <typename T, int N>
__device__ __forceinline__ void voxel_input(const RowArgs& a, const char* in, const char* dy, const double (&m)[N],
                                            const double (&slope)[N], double (&g)[N])
{
    switch (a.v.order) {
    case 1: voxel_taps<T, N, 1>(a, in, dy, m, slope, g); break;
    case 2: voxel_taps<T, N, 2>(a, in, dy, m, slope, g); break;
    case 3: voxel_taps<T, N, 3>(a, in, dy, m, slope, g); break;
    case 4: voxel_taps<T, N, 4>(a, in, dy, m, slope, g); break;
    case 5: voxel_taps<T, N, 5>(a, in, dy, m, slope, g); break;
    default: break;               // order 0: the weights do not depend on the coordinate
    }
}

// P > 0: one order and one volume type (T) per kernel -- the 2- and 3-axis kernels, each with the registers of its
// own tap loop; P == 0: every order and both types behind a runtime switch (1 and 4..7 axes)
// AK: also the row moments of g for the inverse map's gradient (a.mom); a.part may then be nullptr
template <int N, int P, typename T, bool AK>
__global__ __launch_bounds__(kRowThreads) void dgrad_rows_kernel(RowArgs a)
{
    __shared__ double s_q[kDgradMaxK];                    // the row's displacement coefficients Q[h][j_last]
    __shared__ double s_g[kMaxAxes * kRowThreads];        // g_h of the chunk's voxels; at the end: the wave partials
    __shared__ double s_bw[4 * kRowThreads];              // b_{n-1} weights of the chunk's voxels
    __shared__ int64_t s_st[kRowThreads];                 // their first control index (unfolded)
    __shared__ double s_mom[AK ? 2 * N * (kRowThreads / 64) : 1];   // AK: per wave, its moments summed over chunks
    const bool want_part = !AK || a.part != nullptr;
    const GridGeom& g = a.g;
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    const int64_t row = blockIdx.x;
    const int b = blockIdx.y;
    const char* disp = g.disp + (int64_t)b * a.disp_bstride;
    const char* in = a.v.in + (int64_t)b * a.in_bstride;
    const char* dyb = a.v.out + (int64_t)b * a.out_bstride;
    const int64_t nl = g.ncp[N - 1];
    const int K = a.K;

    int64_t o[N];
    {
        int64_t r = row;
#pragma unroll
        for (int d = N - 2; d >= 0; --d) {
            o[d] = r % g.out_len[d];
            r /= g.out_len[d];
        }
    }

    // ---- Q[h][j_last] = sum over the other grid axes of P[h, j] * prod_{d < n-1} b_d(o_d, j_d) ----
    // (the row's weights and grid offsets along axes 0..n-2 are the same for every thread: computed once, in LDS)
    __shared__ double s_rw[4 * kMaxAxes];
    __shared__ int64_t s_ri[4 * kMaxAxes];
    if (tid < N - 1) {
        const int d = tid;
        const double u = control_coordinate(g.ncp[d], o[d] + g.off[d], g.in_len[d]);
        const int64_t s = window_start(u, 3);
        double w[4];
        spline_weights(u, 3, w);
        for (int t = 0; t < 4; ++t) {
            s_rw[4 * d + t] = w[t];
            s_ri[4 * d + t] = mirror_index(s + t, g.ncp[d]) * g.disp_stride[d + 1];
        }
    }
    if constexpr (AK) {
        if (tid < 2 * N * ((nt + 63) >> 6))
            s_mom[tid] = 0.0;
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
        const int h = (int)(k / nl);
        const int64_t jl = k % nl;
        const char* base = disp + h * g.disp_stride[0] + jl * g.disp_stride[N];
        // (the dtype is decided once, outside the tap loop, so that the loads of a float grid go out together)
        auto any = [&](const char* p) { return load_as_double(p, g.disp_dtype); };
        if constexpr (N <= 3)
            s_q[k] = g.disp_dtype == EDHIP_F64   ? row_coefficient<N>(base, s_ri, s_rw, [](const char* p) { return *(const double*)p; })
                     : g.disp_dtype == EDHIP_F32 ? row_coefficient<N>(base, s_ri, s_rw, [](const char* p) { return (double)*(const float*)p; })
                                                 : row_coefficient<N>(base, s_ri, s_rw, any);
        else
            s_q[k] = row_coefficient<N>(base, s_ri, s_rw, any);
    }
    __syncthreads();

    // ---- owners of the band contraction: lane -> (h, j_last, voxel group of its wave) ----
    const int wave = tid >> 6, lane = tid & 63;
    const int nw = (nt + 63) >> 6;
    int G = 1;                            // voxel groups per wave (a power of two, G * K <= 64)
    while (G < 64 && 2 * G * K <= 64)
        G *= 2;
    const int gsize = 64 / G;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};

    const int64_t L = g.out_len[N - 1];
    for (int64_t c0 = 0; c0 < L; c0 += nt) {
        const int64_t ol = c0 + tid;
        double gv[N];
#pragma unroll
        for (int h = 0; h < N; ++h)
            gv[h] = 0.0;
        if (ol < L) {
            const double u = control_coordinate(nl, ol + g.off[N - 1], g.in_len[N - 1]);
            const int64_t s = window_start(u, 3);
            double bw[4];
            spline_weights(u, 3, bw);
            s_st[tid] = s;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                s_bw[4 * tid + t] = bw[t];
            o[N - 1] = ol;
            // coordinate: (A o)_h + s_h + delta_h, as deform.c:771-781 adds them
            double c[N];
#pragma unroll
            for (int h = 0; h < N; ++h) {
                double delta = 0.0;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    delta += s_q[h * nl + mirror_index(s + t, nl)] * bw[t];
                double cc;
                if (g.has_affine) {
                    cc = 0.0;
#pragma unroll
                    for (int l = 0; l < N; ++l)
                        cc += g.affine[h * (N + 1) + l] * (double)o[l];
                    cc += g.affine[h * (N + 1) + N];
                } else {
                    cc = (double)o[h];
                }
                c[h] = cc + (double)g.off[h] + delta;
            }
            double m[N], slope[N];
            bool inside = true;
#pragma unroll
            for (int h = 0; h < N; ++h) {
                m[h] = map_coordinate(c[h], g.in_len[h], a.v.mode);
                slope[h] = map_coordinate_slope(c[h], g.in_len[h], a.v.mode);
                inside = inside && m[h] > -1.0;         // 'constant' outside the axis: the voxel is cval
            }
            if (inside) {
                int64_t yoff = 0;
#pragma unroll
                for (int d = 0; d < N; ++d)
                    yoff += o[d] * a.v.out_stride[d];
                if constexpr (P > 0)
                    voxel_taps<T, N, P>(a, in, dyb + yoff, m, slope, gv);
                else if (a.v.in_dtype == EDHIP_F32)
                    voxel_input<float, N>(a, in, dyb + yoff, m, slope, gv);
                else
                    voxel_input<double, N>(a, in, dyb + yoff, m, slope, gv);
            }
        }
#pragma unroll
        for (int h = 0; h < N; ++h)
            s_g[h * kRowThreads + tid] = gv[h];
        __syncthreads();
        if constexpr (AK) {
            // the row moments from the LDS copy (a voxel past the row's end holds g = 0): S0_h = sum g_h,
            // S1_h = sum g_h o_{n-1} over the wave's 64 voxels, added to the wave's own slot in chunk order
            const double ol = (double)(c0 + tid);
#pragma unroll
            for (int h = 0; h < N; ++h) {
                const double gh = s_g[h * kRowThreads + tid];
                const double s0 = wave_sum(gh);
                const double s1 = wave_sum(gh * ol);
                if (lane == 0) {
                    s_mom[(wave * N + h) * 2] += s0;
                    s_mom[(wave * N + h) * 2 + 1] += s1;
                }
            }
        }
        // wave `wave` contracts its own 64 voxels: lane q -> (hj = q % K, group q / K), groups in ascending order
        const int64_t vend = L - c0 < (int64_t)nt ? L - c0 : (int64_t)nt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = lane + 64 * r;
            if (want_part && q < K * G) {
                const int hj = q % K, grp = q / K;
                const int h = hj / (int)nl;
                const int64_t j = hj % nl;
                const int v0 = wave * 64 + grp * gsize;
                const int v1 = (int)((int64_t)(v0 + gsize) < vend ? (int64_t)(v0 + gsize) : vend);
                double sum = 0.0;
                for (int vx = v0; vx < v1; ++vx) {
                    const int64_t s = s_st[vx];
                    const double gh = s_g[h * kRowThreads + vx];
                    if (s >= 0 && s + 3 < nl) {
                        const int64_t dj = j - s;
                        if (dj >= 0 && dj <= 3)
                            sum += s_bw[4 * vx + dj] * gh;
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            if (mirror_index(s + t, nl) == j)
                                sum += s_bw[4 * vx + t] * gh;
                    }
                }
                acc[r] += sum;
            }
        }
        __syncthreads();
    }

    if constexpr (AK) {
        // the waves' moments in wave order (their last additions are behind the chunk loop's final barrier)
        if (tid < 2 * N) {
            double sum = 0.0;
            for (int w = 0; w < nw; ++w)
                sum += s_mom[w * 2 * N + tid];
            double* dst = a.mom + ((int64_t)b * a.rows + row) * 2 * N + tid;
            *dst = a.accumulate ? *dst + sum : sum;
        }
        if (!want_part)
            return;
    }

    // ---- partials of the waves and groups, summed in a fixed order ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = lane + 64 * r;
        if (q < K * G)
            s_g[wave * K * G + q] = acc[r];
    }
    __syncthreads();
    for (int k = tid; k < K; k += nt) {
        double sum = 0.0;
        for (int w = 0; w < nw; ++w)
            for (int grp = 0; grp < G; ++grp)
                sum += s_g[w * K * G + grp * K + k];
        double* dst = a.part + ((int64_t)b * a.rows + row) * K + k;
        *dst = a.accumulate ? *dst + sum : sum;
    }
}

// [outer][L][inner] -> [outer][ncp][inner]: out[.., j, ..] = sum_o b(o, j) in[.., o, ..].  One wavefront per output:
// lane l sums o = l, l + 64, ... in ascending order, then the 64 partial sums are added in a fixed tree
// (same bits on every run).
struct ContractArgs {
    const double* in;
    double* out;
    int64_t nouter, L, ncp, inner;
    int64_t off, in_len;          // crop offset and input extent of this axis (control_coordinate)
};

__global__ __launch_bounds__(256) void dgrad_contract_kernel(ContractArgs c)
{
    __shared__ double s_red[256];
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const bool live = i < c.nouter * c.ncp * c.inner;
    double acc = 0.0;
    if (live) {
        const int64_t in_i = i % c.inner;
        const int64_t r = i / c.inner;
        const int64_t j = r % c.ncp;
        const int64_t outer = r / c.ncp;
        const double* src = c.in + outer * c.L * c.inner + in_i;
        for (int64_t o = lane; o < c.L; o += 64) {
            const double u = control_coordinate(c.ncp, o + c.off, c.in_len);
            const int64_t s = window_start(u, 3);
            if (s >= 0 && s + 3 < c.ncp && (j < s || j > s + 3))
                continue;
            double w[4];
            spline_weights(u, 3, w);
            double coef = 0.0;
            bool hit = false;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (mirror_index(s + t, c.ncp) == j) {
                    coef += w[t];
                    hit = true;
                }
            if (hit)
                acc += coef * src[o * c.inner];
        }
    }
    s_red[threadIdx.x] = acc;
    __syncthreads();
    const int base = threadIdx.x & ~63;
    for (int w = 32; w >= 1; w >>= 1) {
        if (lane < w)
            s_red[base + lane] += s_red[base + lane + w];
        __syncthreads();
    }
    if (live && lane == 0)
        c.out[i] = s_red[base];
}

// [b][j_0 .. j_{n-2}][h][j_{n-1}] (dense fp64) -> dst[b][h][j_0 .. j_{n-1}] in dst's dtype and strides
struct FinishArgs {
    const double* in;
    char* dst;
    int dst_dtype;
    int naxis;
    int64_t ncp[kMaxAxes];
    int64_t dst_stride[kMaxAxes + 1];
    int64_t dst_bstride;
    int64_t per_sample, nbatch;
};

__global__ __launch_bounds__(256) void dgrad_finish_kernel(FinishArgs f)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.per_sample * f.nbatch)
        return;
    const int64_t b = i / f.per_sample;
    int64_t r = i % f.per_sample;
    const int n = f.naxis;
    // source index (layout above), r = ((j_0 .. j_{n-2}) * n + h) * ncp_{n-1} + j_{n-1}
    const int64_t jl = r % f.ncp[n - 1];
    r /= f.ncp[n - 1];
    const int64_t h = r % n;
    r /= n;
    int64_t doff = h * f.dst_stride[0] + jl * f.dst_stride[n];
    for (int d = n - 2; d >= 0; --d) {
        doff += (r % f.ncp[d]) * f.dst_stride[d + 1];
        r /= f.ncp[d];
    }
    store_cast(f.dst + b * f.dst_bstride + doff, f.dst_dtype, f.in[i]);
}

// rows -> one partial of every dK entry per workgroup of kAffineRows rows: thread t takes row 256 * x + t, the
// entries are summed by a butterfly per wave, then the waves in order.  part[b][chunk][h][0..n].
constexpr int kAffineRows = 256;

struct AffineReduceArgs {
    const double* mom;            // [nbatch][rows][n][2]
    double* part;                 // [nbatch][nchunk][n][n+1]
    int64_t rows, nchunk;
    int64_t out_len[kMaxAxes];
};

template <int N>
__global__ __launch_bounds__(kAffineRows) void dgrad_affine_reduce_kernel(AffineReduceArgs r)
{
    constexpr int M = N * (N + 1);
    constexpr int NW = kAffineRows / 64;
    __shared__ double s_w[NW * M];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t chunk = blockIdx.x;
    const int64_t b = blockIdx.y;
    const int64_t row = chunk * kAffineRows + tid;
    double v[M];
#pragma unroll
    for (int k = 0; k < M; ++k)
        v[k] = 0.0;
    if (row < r.rows) {
        double o[N];
        int64_t q = row;
        o[N - 1] = 0.0;
#pragma unroll
        for (int d = N - 2; d >= 0; --d) {
            o[d] = (double)(q % r.out_len[d]);
            q /= r.out_len[d];
        }
        const double* m = r.mom + (b * r.rows + row) * 2 * N;
#pragma unroll
        for (int h = 0; h < N; ++h) {
            const double s0 = m[2 * h], s1 = m[2 * h + 1];
#pragma unroll
            for (int l = 0; l < N - 1; ++l)
                v[h * (N + 1) + l] = o[l] * s0;
            v[h * (N + 1) + N - 1] = s1;
            v[h * (N + 1) + N] = s0;
        }
    }
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0)
            s_w[wave * M + k] = s;
    }
    __syncthreads();
    if (tid < M) {
        double sum = 0.0;
        for (int w = 0; w < NW; ++w)
            sum += s_w[w * M + tid];
        r.part[(b * r.nchunk + chunk) * M + tid] = sum;
    }
}

// one wavefront per (dK entry, sample): lane l sums the partials l, l + 64, ... in order, then a butterfly
struct AffineStoreArgs {
    const double* part;           // [nbatch][nchunk][n][n+1]; nchunk == 0: nothing contributes, dK = 0
    int64_t nchunk;
    int naxis;
    char* dst;                    // float64 (n, n+1), any strides
    int64_t dst_stride[2];
    int64_t dst_bstride;
};

__global__ __launch_bounds__(64) void dgrad_affine_store_kernel(AffineStoreArgs s)
{
    const int lane = threadIdx.x;
    const int k = blockIdx.x;
    const int64_t b = blockIdx.y;
    const int M = s.naxis * (s.naxis + 1);
    double acc = 0.0;
    for (int64_t c = lane; c < s.nchunk; c += 64)
        acc += s.part[(b * s.nchunk + c) * M + k];
    acc = wave_sum(acc);
    if (lane == 0) {
        const int h = k / (s.naxis + 1), l = k % (s.naxis + 1);
        *(double*)(s.dst + b * s.dst_bstride + h * s.dst_stride[0] + l * s.dst_stride[1]) = acc;
    }
}

template <int N, int P, typename T, bool AK>
hipError_t launch_rows_one(const RowArgs& a, int block, int nbatch, hipStream_t stream)
{
    hipLaunchKernelGGL((dgrad_rows_kernel<N, P, T, AK>), dim3((unsigned)a.rows, (unsigned)nbatch), dim3(block), 0,
                       stream, a);
    return hipGetLastError();
}

template <int N, bool AK>
hipError_t launch_rows(const RowArgs& a, int block, int nbatch, hipStream_t stream)
{
    if constexpr (N == 2 || N == 3) {
        const bool f32 = a.v.in_dtype == EDHIP_F32;
        switch (a.v.order) {
        case 1: return f32 ? launch_rows_one<N, 1, float, AK>(a, block, nbatch, stream) : launch_rows_one<N, 1, double, AK>(a, block, nbatch, stream);
        case 2: return f32 ? launch_rows_one<N, 2, float, AK>(a, block, nbatch, stream) : launch_rows_one<N, 2, double, AK>(a, block, nbatch, stream);
        case 3: return f32 ? launch_rows_one<N, 3, float, AK>(a, block, nbatch, stream) : launch_rows_one<N, 3, double, AK>(a, block, nbatch, stream);
        case 4: return f32 ? launch_rows_one<N, 4, float, AK>(a, block, nbatch, stream) : launch_rows_one<N, 4, double, AK>(a, block, nbatch, stream);
        default: return f32 ? launch_rows_one<N, 5, float, AK>(a, block, nbatch, stream) : launch_rows_one<N, 5, double, AK>(a, block, nbatch, stream);
        }
    } else {
        return launch_rows_one<N, 0, double, AK>(a, block, nbatch, stream);
    }
}

template <int N>
hipError_t launch_rows_ak(const RowArgs& a, int block, int nbatch, hipStream_t stream)
{
    return a.mom ? launch_rows<N, true>(a, block, nbatch, stream) : launch_rows<N, false>(a, block, nbatch, stream);
}

template <int N>
hipError_t launch_affine_reduce(const AffineReduceArgs& r, int nbatch, hipStream_t stream)
{
    hipLaunchKernelGGL((dgrad_affine_reduce_kernel<N>), dim3((unsigned)r.nchunk, (unsigned)nbatch), dim3(kAffineRows),
                       0, stream, r);
    return hipGetLastError();
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int64_t affine_chunks(int64_t rows) { return (rows + kAffineRows - 1) / kAffineRows; }

// the inverse map's scratch: the row moments, then the reduce kernel's partials
size_t affine_scratch_bytes(const GridGeom& g, int nbatch, int64_t rows)
{
    const size_t n = (size_t)g.naxis;
    return align256((size_t)nbatch * (size_t)rows * n * 2 * 8) +
           align256((size_t)nbatch * (size_t)affine_chunks(rows) * n * (n + 1) * 8);
}

int64_t row_count(const GridGeom& g)
{
    int64_t rows = 1;
    for (int d = 0; d < g.naxis - 1; ++d)
        rows *= g.out_len[d];
    return rows;
}

// the two contraction buffers: the largest intermediate [b][o_0..o_{d-1}][j_d..j_{n-2}][K]
size_t stage_elems(const GridGeom& g, int nbatch, int d)
{
    size_t e = (size_t)nbatch * (size_t)g.naxis * (size_t)g.ncp[g.naxis - 1];
    for (int k = 0; k < g.naxis - 1; ++k)
        e *= (size_t)(k < d ? g.out_len[k] : g.ncp[k]);
    return e;
}

}  // namespace

bool dgrad_supported(const GridGeom& g)
{
    return g.naxis >= 1 && g.naxis <= kMaxAxes && (int64_t)g.naxis * g.ncp[g.naxis - 1] <= kDgradMaxK;
}

size_t dgrad_scratch_bytes(const GridGeom& g, int nbatch, bool dp, bool dk)
{
    // dP: part (d = n-1: every o_0..o_{n-2}) + the largest later stage, twice; dK: the row moments + partials
    size_t big = 0;
    for (int d = 0; d < g.naxis - 1; ++d)
        big = stage_elems(g, nbatch, d) > big ? stage_elems(g, nbatch, d) : big;
    big = stage_elems(g, nbatch, 0) > big ? stage_elems(g, nbatch, 0) : big;
    const size_t dp_bytes = dp ? align256(stage_elems(g, nbatch, g.naxis - 1) * 8) + 2 * align256(big * 8) : 0;
    return dp_bytes + (dk ? affine_scratch_bytes(g, nbatch, row_count(g)) : 0);
}

hipError_t launch_deform_dgrad(const DgradCall& c, hipStream_t stream)
{
    const GridGeom& g = c.g;
    const int n = g.naxis;
    if (!dgrad_supported(g) || (!c.dst && !c.dK))
        return hipErrorNotSupported;
    const bool want_dp = c.dst != nullptr, want_dk = c.dK != nullptr;
    const int K = n * (int)g.ncp[n - 1];
    const int64_t rows = row_count(g);
    // scratch: [part | buf0 | buf1] (dP wanted) [mom | affine partials] (dK wanted)
    size_t big = 0;
    for (int d = 0; d < n - 1; ++d)
        big = stage_elems(g, c.nbatch, d) > big ? stage_elems(g, c.nbatch, d) : big;
    big = stage_elems(g, c.nbatch, 0) > big ? stage_elems(g, c.nbatch, 0) : big;
    double* part = want_dp ? (double*)c.scratch : nullptr;
    double* buf[2] = {nullptr, nullptr};
    char* tail = c.scratch;
    if (want_dp) {
        buf[0] = (double*)(c.scratch + align256(stage_elems(g, c.nbatch, n - 1) * 8));
        buf[1] = (double*)((char*)buf[0] + align256(big * 8));
        tail = (char*)buf[1] + align256(big * 8);
    }
    double* mom = want_dk ? (double*)tail : nullptr;
    double* apart = want_dk ? (double*)(tail + align256((size_t)c.nbatch * (size_t)rows * (size_t)n * 2 * 8)) : nullptr;

    hipError_t e = hipSuccess;
    const int64_t L = g.out_len[n - 1];
    const int block = L > 128 ? 256 : (L > 64 ? 128 : 64);
    bool any = false;
    if (g.nvox > 0 && rows <= 0x7fffffff && c.nbatch <= 65535) {
        for (int i = 0; i < c.ninputs && e == hipSuccess; ++i) {
            const IOView& v = c.views[i];
            if (v.order < 1 || v.order > 5 || v.nsteps <= 0)
                continue;         // order 0 (and an empty step axis): the input contributes exactly zero
            RowArgs a;
            memset(&a, 0, sizeof(a));
            a.g = g;
            a.v = v;
            a.part = part;
            a.mom = mom;
            a.rows = rows;
            a.K = K;
            a.accumulate = any ? 1 : 0;
            a.in_bstride = c.in_bstride;
            a.out_bstride = c.out_bstride;
            a.disp_bstride = c.disp_bstride;
            switch (n) {
            case 1: e = launch_rows_ak<1>(a, block, c.nbatch, stream); break;
            case 2: e = launch_rows_ak<2>(a, block, c.nbatch, stream); break;
            case 3: e = launch_rows_ak<3>(a, block, c.nbatch, stream); break;
            case 4: e = launch_rows_ak<4>(a, block, c.nbatch, stream); break;
            case 5: e = launch_rows_ak<5>(a, block, c.nbatch, stream); break;
            case 6: e = launch_rows_ak<6>(a, block, c.nbatch, stream); break;
            default: e = launch_rows_ak<7>(a, block, c.nbatch, stream); break;
            }
            any = true;
        }
    } else if (g.nvox > 0) {
        return hipErrorNotSupported;
    }
    if (e != hipSuccess)
        return e;

    if (want_dk) {
        // dK: rows -> per-workgroup partials -> dK; nothing contributes: the store kernel writes exact zeros
        AffineReduceArgs r;
        memset(&r, 0, sizeof(r));
        r.mom = mom;
        r.part = apart;
        r.rows = rows;
        r.nchunk = any ? affine_chunks(rows) : 0;
        for (int d = 0; d < n; ++d)
            r.out_len[d] = g.out_len[d];
        if (any) {
            switch (n) {
            case 1: e = launch_affine_reduce<1>(r, c.nbatch, stream); break;
            case 2: e = launch_affine_reduce<2>(r, c.nbatch, stream); break;
            case 3: e = launch_affine_reduce<3>(r, c.nbatch, stream); break;
            case 4: e = launch_affine_reduce<4>(r, c.nbatch, stream); break;
            case 5: e = launch_affine_reduce<5>(r, c.nbatch, stream); break;
            case 6: e = launch_affine_reduce<6>(r, c.nbatch, stream); break;
            default: e = launch_affine_reduce<7>(r, c.nbatch, stream); break;
            }
            if (e != hipSuccess)
                return e;
        }
        AffineStoreArgs s;
        memset(&s, 0, sizeof(s));
        s.part = apart;
        s.nchunk = r.nchunk;
        s.naxis = n;
        s.dst = c.dK;
        s.dst_stride[0] = c.dK_stride[0];
        s.dst_stride[1] = c.dK_stride[1];
        s.dst_bstride = c.dK_bstride;
        hipLaunchKernelGGL(dgrad_affine_store_kernel, dim3((unsigned)(n * (n + 1)), (unsigned)c.nbatch), dim3(64), 0,
                           stream, s);
        e = hipGetLastError();
        if (e != hipSuccess || !want_dp)
            return e;
    }

    const double* cur = part;
    if (!any) {
        // nothing contributes (no output voxel, order 0, empty step axes): dP = 0
        const size_t bytes = stage_elems(g, c.nbatch, 0) * 8;
        e = hipMemsetAsync(buf[0], 0, bytes, stream);
        cur = buf[0];
    } else {
        // contract o_{n-2}, ..., o_0: [b][o_0..o_{d-1}][o_d][j_{d+1}..][K] -> [b][o_0..o_{d-1}][j_d][j_{d+1}..][K]
        int flip = 0;
        for (int d = n - 2; d >= 0 && e == hipSuccess; --d) {
            ContractArgs ca;
            ca.in = cur;
            ca.out = buf[flip];
            ca.nouter = c.nbatch;
            for (int k = 0; k < d; ++k)
                ca.nouter *= g.out_len[k];
            ca.L = g.out_len[d];
            ca.ncp = g.ncp[d];
            ca.inner = K;
            for (int k = d + 1; k < n - 1; ++k)
                ca.inner *= g.ncp[k];
            ca.off = g.off[d];
            ca.in_len = g.in_len[d];
            const int64_t total = ca.nouter * ca.ncp * ca.inner;          // outputs, four per workgroup
            hipLaunchKernelGGL(dgrad_contract_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, ca);
            e = hipGetLastError();
            cur = buf[flip];
            flip ^= 1;
        }
    }
    if (e != hipSuccess)
        return e;
    FinishArgs f;
    memset(&f, 0, sizeof(f));
    f.in = cur;
    f.dst = c.dst;
    f.dst_dtype = c.dst_dtype;
    f.naxis = n;
    f.per_sample = n;
    for (int d = 0; d < n; ++d) {
        f.ncp[d] = g.ncp[d];
        f.per_sample *= g.ncp[d];
    }
    for (int d = 0; d <= n; ++d)
        f.dst_stride[d] = c.dst_stride[d];
    f.dst_bstride = c.dst_bstride;
    f.nbatch = c.nbatch;
    const int64_t total = f.per_sample * f.nbatch;
    hipLaunchKernelGGL(dgrad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, f);
    return hipGetLastError();
}

}  // namespace ed
