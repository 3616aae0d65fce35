// Host-only run of the gradient kernels of csrc/deform_points_grad.hip (points_grad_prepare / _scatter / _finish) under
// AddressSanitizer and UndefinedBehaviorSanitizer: the device functions compiled as plain C++ against the stand-in
// runtime of tests/cxx/host_hip (one emulated thread per workgroup), fed the folded two-point grid, a grid whose cells
// live in global memory, non-finite and huge positions, non-finite cotangents, unsolved points and 1 to 5 axes.  Every
// array is a heap block of exactly the promised size, so a read or write beyond it is a report.  Also checked: the
// sums against what they must add up to (sum_j dP[h, j] = sum_i u[i, h], dK = u^T [q, 1]), exact bit equality after
// reversing the points, zero rows for points that contribute nothing, and a bound that overflows (NaN in both sums, in
// its own sample alone).
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
//       -Itests/cxx/host_hip -Ielasticdeform_amd/csrc -Iinclude tests/cxx/points_gradient_host_test.cpp -o t && ./t
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "deform_points_grad.hip"

namespace ed {
namespace {
double s_grid[kHostLdsBytes / 8];
unsigned long long s_cells[kHostLdsBytes / 8];
}  // namespace
}  // namespace ed

void host_lds_begin()
{
    // LDS is not cleared between workgroups and ends at the launch's size
    HOST_HIP_UNPOISON(ed::s_grid, kHostLdsBytes);
    HOST_HIP_UNPOISON(ed::s_cells, kHostLdsBytes);
    memset(ed::s_grid, 0xff, kHostLdsBytes);
    memset(ed::s_cells, 0xff, kHostLdsBytes);
    HOST_HIP_POISON((char*)ed::s_grid + host_lds_bytes, kHostLdsBytes - host_lds_bytes);
    HOST_HIP_POISON((char*)ed::s_cells + host_lds_bytes, kHostLdsBytes - host_lds_bytes);
}

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static double uniform(uint64_t& s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
}

template <typename T>
struct Block {                       // a heap block of exactly n elements
    T* p;
    size_t n;
    explicit Block(size_t n_) : p((T*)malloc(n_ * sizeof(T) + (n_ == 0))), n(n_) {}
    ~Block() { free(p); }
    T& operator[](size_t i) { return p[i]; }
};

struct Result {
    std::vector<double> rows, dP, dK;
};

// one call on `npts` points of `n` axes with `ncp` control points per axis; order: +1 as given, -1 reversed
static Result run(int n, int ncp, int64_t npts, int inverse, int nbatch, const std::vector<double>& q,
                  const std::vector<double>& c, const std::vector<unsigned char>& st, int order)
{
    using namespace ed;
    int64_t per = 1;
    for (int k = 0; k < n; ++k)
        per *= ncp;
    const int64_t values = n * per;
    Block<float> grid((size_t)nbatch * values);              // a float32 grid: converted at the load
    uint64_t seed = 7;
    for (size_t i = 0; i < grid.n; ++i)
        grid[i] = (float)(uniform(seed) - 0.5);
    Block<double> pos((size_t)nbatch * npts * n), cot((size_t)nbatch * npts * n), rows((size_t)nbatch * npts * n);
    Block<unsigned char> status((size_t)nbatch * npts);
    for (int b = 0; b < nbatch; ++b)
        for (int64_t i = 0; i < npts; ++i) {
            const int64_t src = order > 0 ? i : npts - 1 - i;
            for (int h = 0; h < n; ++h) {
                pos[(b * npts + i) * n + h] = q[src * n + h];
                cot[(b * npts + i) * n + h] = c[src * n + h] * (b + 1);
            }
            status[b * npts + i] = st[src];
        }
    Block<double> dP((size_t)nbatch * values), dK((size_t)nbatch * n * (n + 1));
    PointsGradCall call;
    memset(&call, 0, sizeof(call));
    GridGeom& g = call.g;
    g.naxis = n;
    g.has_affine = 1;
    g.disp_dtype = EDHIP_F32;
    g.disp = (const char*)grid.p;
    int64_t stride = 4;
    for (int k = n - 1; k >= 0; --k) {
        g.in_len[k] = g.out_len[k] = 9 + k;
        g.off[k] = k;
        g.ncp[k] = ncp;
        g.disp_stride[k + 1] = stride;
        stride *= ncp;
    }
    g.disp_stride[0] = stride;
    for (int h = 0; h < n; ++h)
        for (int l = 0; l <= n; ++l)
            g.affine[h * (n + 1) + l] = (h == l ? 1.0 : 0.0) + 0.05 * (h - l);
    call.inverse = inverse;
    call.nbatch = nbatch;
    call.npts = npts;
    call.disp_bstride = values * 4;
    call.pos.ptr = (char*)pos.p;
    call.cot.ptr = (char*)cot.p;
    call.dpts.ptr = (char*)rows.p;
    call.pos.dtype = call.cot.dtype = call.dpts.dtype = EDHIP_F64;
    call.pos.stride[0] = call.cot.stride[0] = call.dpts.stride[0] = n * 8;
    call.pos.stride[1] = call.cot.stride[1] = call.dpts.stride[1] = 8;
    call.pos.bstride = call.cot.bstride = call.dpts.bstride = npts * n * 8;
    call.status.ptr = inverse ? (char*)status.p : nullptr;
    call.status.stride[0] = 1;
    call.status.bstride = npts;
    call.ddisp.ptr = (char*)dP.p;
    call.ddisp.dtype = EDHIP_F64;
    call.ddisp.bstride = values * 8;
    stride = 8;
    for (int k = n; k >= 0; --k) {
        call.ddisp.stride[k] = stride;
        stride *= k > 0 ? ncp : 1;
    }
    call.dK.ptr = (char*)dK.p;
    call.dK.stride[0] = (n + 1) * 8;
    call.dK.stride[1] = 8;
    call.dK.bstride = n * (n + 1) * 8;
    Block<char> scratch(points_grad_scratch_bytes(g, nbatch, npts));
    memset(scratch.p, 0xff, scratch.n);                      // nothing may rely on what an earlier call left
    call.scratch = scratch.p;
    CHECK(launch_deform_points_gradient(call, nullptr) == hipSuccess);
    Result r;
    r.rows.assign(rows.p, rows.p + rows.n);
    r.dP.assign(dP.p, dP.p + dP.n);
    r.dK.assign(dK.p, dK.p + dK.n);
    return r;
}

static void one_case(int n, int ncp, int64_t npts, int inverse)
{
    uint64_t seed = 1000 * n + ncp + inverse;
    std::vector<double> q(npts * n), c(npts * n);
    std::vector<unsigned char> st(npts, 1);
    for (int64_t i = 0; i < npts; ++i)
        for (int h = 0; h < n; ++h) {
            q[i * n + h] = -12.0 + 36.0 * uniform(seed);
            c[i * n + h] = uniform(seed) - 0.5;
        }
    // points that contribute nothing: non-finite and huge positions (their cotangents non-finite too), and for the
    // inverse direction unsolved ones
    const double bad[4] = {NAN, INFINITY, 1e300, -INFINITY};
    std::vector<int64_t> dead;
    for (int j = 0; j < 4 && j < npts; ++j) {
        const int64_t i = (j * 7 + 3) % npts;
        q[i * n + (j % n)] = bad[j];
        c[i * n] = j & 1 ? NAN : 1.0;
        dead.push_back(i);
    }
    if (inverse && npts > 40) {
        st[40] = 0;
        c[40 * n] = INFINITY;
        dead.push_back(40);
    }
    const int nbatch = 2;
    const Result a = run(n, ncp, npts, inverse, nbatch, q, c, st, +1);
    const Result b = run(n, ncp, npts, inverse, nbatch, q, c, st, -1);
    CHECK(a.dP.size() == b.dP.size() && memcmp(a.dP.data(), b.dP.data(), a.dP.size() * 8) == 0);
    CHECK(memcmp(a.dK.data(), b.dK.data(), a.dK.size() * 8) == 0);
    for (int64_t i = 0; i < npts; ++i)
        CHECK(memcmp(&a.rows[i * n], &b.rows[(npts - 1 - i) * n], n * 8) == 0);
    for (int64_t i : dead)
        for (int h = 0; h < n; ++h)
            CHECK(a.rows[i * n + h] == 0.0);
    int64_t per = 1;
    for (int k = 0; k < n; ++k)
        per *= ncp;
    if (!inverse) {
        // u is the cotangent: sum_j dP[h, j] = sum_i u[i, h] = dK[h, n], dK[h, l] = sum_i u[i, h] q[i, l]
        for (int s = 0; s < nbatch; ++s)
            for (int h = 0; h < n; ++h) {
                double want = 0.0, scale = 0.0, got = 0.0;
                std::vector<double> wantK(n, 0.0);
                for (int64_t i = 0; i < npts; ++i) {
                    bool ok = true;
                    for (int64_t d : dead)
                        ok = ok && d != i;
                    if (!ok)
                        continue;
                    const double u = c[i * n + h] * (s + 1);
                    want += u;
                    scale += fabs(u);
                    for (int l = 0; l < n; ++l)
                        wantK[l] += u * q[i * n + l];
                }
                for (int64_t j = 0; j < per; ++j)
                    got += a.dP[(s * n + h) * per + j];
                CHECK(fabs(got - want) <= 1e-12 * scale);
                CHECK(fabs(a.dK[(s * n + h) * (n + 1) + n] - want) <= 1e-12 * scale);
                for (int l = 0; l < n; ++l)
                    CHECK(fabs(a.dK[(s * n + h) * (n + 1) + l] - wantK[l]) <= 1e-12 * scale * 24.0);
            }
    } else {
        for (double v : a.dP)
            CHECK(std::isfinite(v));
    }
    // one non-finite cotangent on a contributing point: every sum of the sample is NaN
    std::vector<double> c2 = c;
    c2[(npts / 2) * n] = NAN;
    bool contributing = true;
    for (int64_t d : dead)
        contributing = contributing && d != npts / 2;
    if (contributing && !inverse) {
        const Result x = run(n, ncp, npts, inverse, 1, q, c2, st, +1);
        for (double v : x.dP)
            CHECK(v != v);
        for (double v : x.dK)
            CHECK(v != v);
    }
    // no points: zeros
    const Result z = run(n, ncp, 0, inverse, 1, {}, {}, {}, +1);
    for (double v : z.dP)
        CHECK(v == 0.0);
    for (double v : z.dK)
        CHECK(v == 0.0);
}

// The bound rule of this call: bP = 2 N max|u| and bK = bP max(1, max|q|); bP > 0 with a bK that overflows makes
// BOTH outputs of the sample NaN.  One sample, two axes, a 4 x 4 grid on an 8 x 8 image, float64, one point at
// (100, 0.5) -- sane: the limit is a control coordinate of 4e15 -- with the cotangent (4e307, 0): bP = 8e307 is
// finite, bK = bP * 100 is not.  The point's own row J^T u stays finite.  In a batch the overflow poisons its own
// sample only: a second sample with the cotangent (1, 0) gives the bits of a call of its own.
struct Overflow {
    double rows[4], dP[64], dK[12];
};

static Overflow overflow_run(int nbatch, const double* cot_of_sample)
{
    using namespace ed;
    const int n = 2, ncp = 4, values = n * ncp * ncp;
    Block<double> grid((size_t)nbatch * values), pos((size_t)nbatch * n), cot((size_t)nbatch * n);
    Block<double> rows((size_t)nbatch * n), dP((size_t)nbatch * values), dK((size_t)nbatch * n * (n + 1));
    uint64_t seed = 11;
    for (int e = 0; e < values; ++e) {
        const double v = uniform(seed) - 0.5;
        for (int b = 0; b < nbatch; ++b)
            grid[b * values + e] = v;
    }
    for (int b = 0; b < nbatch; ++b) {
        pos[b * n] = 100.0, pos[b * n + 1] = 0.5;
        cot[b * n] = cot_of_sample[b], cot[b * n + 1] = 0.0;
    }
    PointsGradCall call;
    memset(&call, 0, sizeof(call));
    GridGeom& g = call.g;
    g.naxis = n;
    g.disp_dtype = EDHIP_F64;
    g.disp = (const char*)grid.p;
    for (int k = 0; k < n; ++k) {
        g.in_len[k] = g.out_len[k] = 8;
        g.ncp[k] = ncp;
    }
    g.disp_stride[0] = ncp * ncp * 8, g.disp_stride[1] = ncp * 8, g.disp_stride[2] = 8;
    call.nbatch = nbatch;
    call.npts = 1;
    call.disp_bstride = values * 8;
    call.pos.ptr = (char*)pos.p;
    call.cot.ptr = (char*)cot.p;
    call.dpts.ptr = (char*)rows.p;
    call.pos.dtype = call.cot.dtype = call.dpts.dtype = call.ddisp.dtype = EDHIP_F64;
    call.pos.stride[0] = call.cot.stride[0] = call.dpts.stride[0] = n * 8;
    call.pos.stride[1] = call.cot.stride[1] = call.dpts.stride[1] = 8;
    call.pos.bstride = call.cot.bstride = call.dpts.bstride = n * 8;
    call.ddisp.ptr = (char*)dP.p;
    call.ddisp.stride[0] = ncp * ncp * 8, call.ddisp.stride[1] = ncp * 8, call.ddisp.stride[2] = 8;
    call.ddisp.bstride = values * 8;
    call.dK.ptr = (char*)dK.p;
    call.dK.stride[0] = (n + 1) * 8, call.dK.stride[1] = 8;
    call.dK.bstride = n * (n + 1) * 8;
    Block<char> scratch(points_grad_scratch_bytes(g, nbatch, 1));
    memset(scratch.p, 0xff, scratch.n);
    call.scratch = scratch.p;
    CHECK(launch_deform_points_gradient(call, nullptr) == hipSuccess);
    Overflow r;
    memset(&r, 0, sizeof(r));
    memcpy(r.rows, rows.p, rows.n * 8);
    memcpy(r.dP, dP.p, dP.n * 8);
    memcpy(r.dK, dK.p, dK.n * 8);
    return r;
}

static void overflowing_bound()
{
    const double huge[2] = {4e307, 1.0}, one[1] = {1.0};
    const Overflow x = overflow_run(1, huge), both = overflow_run(2, huge), alone = overflow_run(1, one);
    for (int e = 0; e < 32; ++e)
        CHECK(x.dP[e] != x.dP[e]);
    for (int e = 0; e < 6; ++e)
        CHECK(x.dK[e] != x.dK[e]);
    CHECK(std::isfinite(x.rows[0]) && std::isfinite(x.rows[1]));
    // the batch: sample 0 as the single call, sample 1 the bits of its own call (finite, not all zero)
    CHECK(memcmp(both.dP, x.dP, 32 * 8) == 0 && memcmp(both.dK, x.dK, 6 * 8) == 0);
    CHECK(memcmp(both.rows, x.rows, 2 * 8) == 0);
    CHECK(memcmp(both.dP + 32, alone.dP, 32 * 8) == 0 && memcmp(both.dK + 6, alone.dK, 6 * 8) == 0);
    CHECK(memcmp(both.rows + 2, alone.rows, 2 * 8) == 0);
    double sum = 0.0;
    for (int e = 0; e < 32; ++e) {
        CHECK(std::isfinite(alone.dP[e]));
        sum += alone.dP[e];
    }
    CHECK(fabs(sum - 1.0) <= 1e-12);
    CHECK(alone.dK[0] == 100.0 && alone.dK[1] == 0.5 && alone.dK[2] == 1.0);
}

int main()
{
    overflowing_bound();
    for (int inverse = 0; inverse < 2; ++inverse) {
        for (int n = 1; n <= 5; ++n)
            one_case(n, 2, n <= 3 ? 700 : 60, inverse);      // the folded two-point grid: every window is mirrored
        one_case(1, 5, 300, inverse);
        one_case(2, 4, 300, inverse);
        one_case(3, 3, 300, inverse);
        one_case(2, 64, 300, inverse);                       // 2 x 64 x 64 = 8192 values: cells in global memory
    }
    printf(failures ? "%d checks failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
