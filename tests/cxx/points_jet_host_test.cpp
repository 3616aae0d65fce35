// Host-only run of the kernels of csrc/deform_points_jet.hip (points_jet_kernel, points_jet_grad_prepare / _scatter,
// with points_grad_clear / _finish of csrc/deform_points_grad.hip at their two ends) under AddressSanitizer and
// UndefinedBehaviorSanitizer: the device functions compiled as plain C++ against the stand-in runtime of tests/cxx/host_hip (one emulated thread per workgroup, dynamic LDS poisoned beyond the
// launch's size).  Every array is a heap block of exactly the promised size, so a read or write beyond it is a report.
// Cases, with 1, 2 and 3 axes each: the two-point grid (every tap folds), a grid read from global memory (more than
// kPointsLdsValues values), N = 1, a crop offset with an affine map, two samples; positions on knots, outside the
// image, not finite and beyond 4e15.  Checked in the program itself:
// H against a plain 4^n-tap evaluation written here, H's symmetry bit for bit, NaN rows for positions that are not sane,
// the forward without H against the forward with it (same bits), dP against step-1 differences of
// L = sum u r + A J + G H (exact up to rounding: L is linear in every grid value), dK against its plain sum, the rows dq
// against central differences of L away from the knots, zero rows for points that contribute nothing, NaN sums after a
// non-finite cotangent, zeros for N = 0, bit-equal results from two runs and for both samples, and a bound that
// overflows (NaN in dinverse_affine alone, and in its own sample alone).
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
//       -Itests/cxx/host_hip -Ielasticdeform_amd/csrc -Iinclude tests/cxx/points_jet_host_test.cpp -o t && ./t
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "deform_points_jet.hip"
#include "deform_points_grad.hip"                // points_grad_clear / _finish: the reduction's two ends live there

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

typedef std::vector<double> Vec;

struct Case {
    int n;
    int64_t ncp[3], I[3], off[3];
    bool affine;
};

static int64_t cells_of(const Case& c)
{
    int64_t per = 1;
    for (int k = 0; k < c.n; ++k)
        per *= c.ncp[k];
    return per;
}

static ed::GridGeom geometry(const Case& c, const double* grid)
{
    ed::GridGeom g;
    memset(&g, 0, sizeof(g));
    g.naxis = c.n;
    g.has_affine = c.affine;
    g.disp_dtype = EDHIP_F64;
    g.disp = (const char*)grid;
    int64_t stride = 8;
    for (int k = c.n - 1; k >= 0; --k) {
        g.in_len[k] = g.out_len[k] = c.I[k];
        g.off[k] = c.off[k];
        g.ncp[k] = c.ncp[k];
        g.disp_stride[k + 1] = stride;
        stride *= c.ncp[k];
    }
    g.disp_stride[0] = stride;
    for (int h = 0; h < c.n; ++h)
        for (int l = 0; l <= c.n; ++l)
            g.affine[h * (c.n + 1) + l] = (h == l ? 1.0 : 0.0) + 0.07 * (h - l) + (l == c.n ? 0.5 : 0.0);
    return g;
}

static ed::BatchArray rows_array(void* p, int rank, int n, int64_t npts)
{
    ed::BatchArray a;
    memset(&a, 0, sizeof(a));
    a.ptr = (char*)p;
    a.dtype = EDHIP_F64;
    int64_t stride = 8;
    for (int d = rank - 1; d >= 0; --d) {
        a.stride[d] = stride;
        stride *= d > 0 ? n : npts;
    }
    a.bstride = stride;
    return a;
}

struct Forward {
    Vec r, J, H;
};

// the forward on `nbatch` copies of the grid and of the points; the samples must agree bit for bit: sample 0 is returned
static Forward forward(const Case& c, const Vec& grid, const Vec& q, int64_t npts, bool hessian, int nbatch = 2)
{
    using namespace ed;
    const int n = c.n;
    const int64_t values = n * cells_of(c);
    Block<double> gr((size_t)nbatch * values), pts((size_t)nbatch * npts * n), res((size_t)nbatch * npts * n);
    Block<double> jac((size_t)nbatch * npts * n * n), hess(hessian ? (size_t)nbatch * npts * n * n * n : 0);
    for (int b = 0; b < nbatch; ++b) {
        memcpy(gr.p + b * values, grid.data(), values * 8);
        if (npts)
            memcpy(pts.p + b * npts * n, q.data(), npts * n * 8);
    }
    memset(res.p, 0xff, res.n * 8);
    memset(jac.p, 0xff, jac.n * 8);
    memset(hess.p, 0xff, hess.n * 8);
    PointsJetCall call;
    memset(&call, 0, sizeof(call));
    call.g = geometry(c, gr.p);
    call.nbatch = nbatch;
    call.npts = npts;
    call.disp_bstride = values * 8;
    call.pts = rows_array(pts.p, 2, n, npts);
    call.res = rows_array(res.p, 2, n, npts);
    call.jac = rows_array(jac.p, 3, n, npts);
    if (hessian)
        call.hess = rows_array(hess.p, 4, n, npts);
    CHECK(launch_deform_points_derivatives(call, nullptr) == hipSuccess);
    for (int b = 1; b < nbatch; ++b) {
        CHECK(memcmp(res.p, res.p + b * npts * n, npts * n * 8) == 0);
        CHECK(memcmp(jac.p, jac.p + b * npts * n * n, npts * n * n * 8) == 0);
        if (hessian)
            CHECK(memcmp(hess.p, hess.p + b * npts * n * n * n, npts * n * n * n * 8) == 0);
    }
    Forward f;
    f.r.assign(res.p, res.p + npts * n);
    f.J.assign(jac.p, jac.p + npts * n * n);
    if (hessian)
        f.H.assign(hess.p, hess.p + npts * n * n * n);
    return f;
}

struct Adjoint {
    Vec rows, dP, dK;
};

// the adjoint on two samples, the second with every cotangent doubled; an empty cotangent is not given
static Adjoint adjoint(const Case& c, const Vec& grid, const Vec& q, int64_t npts, const Vec& u, const Vec& A,
                       const Vec& G, int order = +1)
{
    using namespace ed;
    const int n = c.n, nbatch = 2;
    const int64_t values = n * cells_of(c);
    Block<double> gr((size_t)nbatch * values), pts((size_t)nbatch * npts * n), rows((size_t)nbatch * npts * n);
    Block<double> du(u.empty() ? 0 : (size_t)nbatch * npts * n), dA(A.empty() ? 0 : (size_t)nbatch * npts * n * n);
    Block<double> dG(G.empty() ? 0 : (size_t)nbatch * npts * n * n * n);
    Block<double> dP((size_t)nbatch * values), dK((size_t)nbatch * n * (n + 1));
    for (int b = 0; b < nbatch; ++b) {
        memcpy(gr.p + b * values, grid.data(), values * 8);
        for (int64_t i = 0; i < npts; ++i) {
            const int64_t src = order > 0 ? i : npts - 1 - i;
            memcpy(pts.p + (b * npts + i) * n, q.data() + src * n, n * 8);
            for (int e = 0; e < n && !u.empty(); ++e)
                du[(b * npts + i) * n + e] = u[src * n + e] * (b + 1);
            for (int e = 0; e < n * n && !A.empty(); ++e)
                dA[(b * npts + i) * n * n + e] = A[src * n * n + e] * (b + 1);
            for (int e = 0; e < n * n * n && !G.empty(); ++e)
                dG[(b * npts + i) * n * n * n + e] = G[src * n * n * n + e] * (b + 1);
        }
    }
    memset(rows.p, 0xff, rows.n * 8);
    memset(dP.p, 0xff, dP.n * 8);
    memset(dK.p, 0xff, dK.n * 8);
    PointsJetGradCall call;
    memset(&call, 0, sizeof(call));
    call.g = geometry(c, gr.p);
    call.nbatch = nbatch;
    call.npts = npts;
    call.disp_bstride = values * 8;
    call.pos = rows_array(pts.p, 2, n, npts);
    if (!u.empty())
        call.du = rows_array(du.p, 2, n, npts);
    if (!A.empty())
        call.dA = rows_array(dA.p, 3, n, npts);
    if (!G.empty())
        call.dG = rows_array(dG.p, 4, n, npts);
    call.dpts = rows_array(rows.p, 2, n, npts);
    call.ddisp.ptr = (char*)dP.p;
    call.ddisp.dtype = EDHIP_F64;
    call.ddisp.bstride = values * 8;
    int64_t stride = 8;
    for (int k = n; k >= 0; --k) {
        call.ddisp.stride[k] = stride;
        stride *= k > 0 ? c.ncp[k - 1] : 1;
    }
    call.dK.ptr = (char*)dK.p;
    call.dK.dtype = EDHIP_F64;
    call.dK.stride[0] = (n + 1) * 8;
    call.dK.stride[1] = 8;
    call.dK.bstride = n * (n + 1) * 8;
    Block<char> scratch(points_jet_scratch_bytes(call.g, nbatch));
    memset(scratch.p, 0xff, scratch.n);                      // nothing may rely on what an earlier call left
    call.scratch = scratch.p;
    CHECK(launch_deform_points_derivatives_gradient(call, nullptr) == hipSuccess);
    Adjoint r;
    r.rows.assign(rows.p, rows.p + rows.n);
    r.dP.assign(dP.p, dP.p + dP.n);
    r.dK.assign(dK.p, dK.p + dK.n);
    return r;
}

// ---- the plain evaluation: no code shared with the kernels ----------------------------------------------------------
static int64_t fold(int64_t i, int64_t n)
{
    if (n == 1)
        return 0;
    const int64_t period = 2 * n - 2;
    int64_t j = ((i % period) + period) % period;
    return j >= n ? period - j : j;
}

static void plain_hessian(const Case& c, const Vec& grid, const double* q, double* H)
{
    const int n = c.n;
    int64_t idx[3][4], per = cells_of(c);
    double w[3][3][4];
    for (int k = 0; k < n; ++k) {
        const double s = (double)(c.ncp[k] - 1) / (double)(c.I[k] - 1);
        const double cp = s * (q[k] + (double)c.off[k]);
        const double fl = floor(cp), x = cp - fl, z = 1.0 - x;
        const double w0[4] = {z * z * z / 6, (3 * x * x * x - 6 * x * x + 4) / 6, (3 * z * z * z - 6 * z * z + 4) / 6,
                              x * x * x / 6};
        const double w1[4] = {-z * z / 2, (3 * x * x - 4 * x) / 2, (-3 * x * x + 2 * x + 1) / 2, x * x / 2};
        const double w2[4] = {z, 3 * x - 2, 1 - 3 * x, x};
        for (int t = 0; t < 4; ++t) {
            idx[k][t] = fold((int64_t)fl - 1 + t, c.ncp[k]);
            w[k][0][t] = w0[t];
            w[k][1][t] = w1[t] * s;
            w[k][2][t] = w2[t] * s * s;
        }
    }
    int taps = 1;
    for (int k = 0; k < n; ++k)
        taps *= 4;
    for (int e = 0; e < n * n * n; ++e)
        H[e] = 0.0;
    for (int tap = 0; tap < taps; ++tap) {
        int t[3];
        int64_t cell = 0;
        for (int k = 0; k < n; ++k) {
            t[k] = (tap >> (2 * (n - 1 - k))) & 3;
            cell = cell * c.ncp[k] + idx[k][t[k]];
        }
        for (int l = 0; l < n; ++l)
            for (int m = 0; m < n; ++m) {
                double prod = 1.0;
                for (int k = 0; k < n; ++k)
                    prod *= w[k][(k == l) + (k == m)][t[k]];
                for (int h = 0; h < n; ++h)
                    H[(h * n + l) * n + m] += grid[h * per + cell] * prod;
            }
    }
}

// L = sum u r + A J + G H over the points that are sane, and the sum of the terms' absolute values
static double loss(const Case& c, const Vec& grid, const Vec& q, int64_t npts, const Vec& u, const Vec& A, const Vec& G,
                   const std::vector<char>& alive, double* scale = nullptr)
{
    const int n = c.n;
    const Forward f = forward(c, grid, q, npts, true, 1);
    double L = 0.0, S = 0.0;
    for (int64_t i = 0; i < npts; ++i) {
        if (!alive[i])
            continue;
        for (int e = 0; e < n && !u.empty(); ++e) {
            L += u[i * n + e] * f.r[i * n + e];
            S += fabs(u[i * n + e] * f.r[i * n + e]);
        }
        for (int e = 0; e < n * n && !A.empty(); ++e) {
            L += A[i * n * n + e] * f.J[i * n * n + e];
            S += fabs(A[i * n * n + e] * f.J[i * n * n + e]);
        }
        for (int e = 0; e < n * n * n && !G.empty(); ++e) {
            L += G[i * n * n * n + e] * f.H[i * n * n * n + e];
            S += fabs(G[i * n * n * n + e] * f.H[i * n * n * n + e]);
        }
    }
    if (scale)
        *scale = S;
    return L;
}

static void one_case(const Case& c, int64_t npts, int which)
{
    const int n = c.n;
    const int64_t per = cells_of(c), values = n * per;
    uint64_t seed = 1000 * n + c.ncp[0] + npts;
    Vec grid(values), q(npts * n), u(npts * n), A(npts * n * n), G(npts * n * n * n);
    for (double& v : grid)
        v = 3.0 * (uniform(seed) - 0.5);
    for (double& v : q)
        v = -8.0 + 40.0 * uniform(seed);
    for (double& v : u)
        v = uniform(seed) - 0.5;
    for (double& v : A)
        v = uniform(seed) - 0.5;
    for (double& v : G)
        v = uniform(seed) - 0.5;
    std::vector<char> alive(npts, 1);
    if (npts > 8) {
        // on knots exactly, and points that contribute nothing (their cotangents not finite either)
        for (int k = 0; k < n; ++k) {
            q[0 * n + k] = -(double)c.off[k];
            q[1 * n + k] = (double)(c.I[k] - 1) - (double)c.off[k];
        }
        const double bad[4] = {NAN, INFINITY, 1e300, -1e17};   // (the last: a control coordinate beyond 4e15)
        for (int j = 0; j < 4; ++j) {
            const int64_t i = 3 + j;
            q[i * n + (j % n)] = bad[j];
            u[i * n] = j & 1 ? NAN : 1.0;
            G[i * n * n * n] = INFINITY;
            alive[i] = 0;
        }
    }
    if (which == 1)
        A.clear(), G.clear();
    if (which == 2)
        u.clear(), G.clear();
    if (which == 3)
        u.clear(), A.clear();

    // ---- forward
    const Forward f = forward(c, grid, q, npts, true), f0 = forward(c, grid, q, npts, false);
    CHECK(f.r.size() == f0.r.size() && memcmp(f.r.data(), f0.r.data(), f.r.size() * 8) == 0);
    CHECK(memcmp(f.J.data(), f0.J.data(), f.J.size() * 8) == 0);
    for (int64_t i = 0; i < npts; ++i) {
        double H[27], Habs = 0.0;
        if (!alive[i]) {
            for (int e = 0; e < n * n * n; ++e)
                CHECK(f.H[i * n * n * n + e] != f.H[i * n * n * n + e]);
            for (int e = 0; e < n; ++e)
                CHECK(f.r[i * n + e] != f.r[i * n + e]);
            continue;
        }
        plain_hessian(c, grid, &q[i * n], H);
        for (int e = 0; e < n * n * n; ++e)
            Habs = fabs(H[e]) > Habs ? fabs(H[e]) : Habs;
        for (int h = 0; h < n; ++h)
            for (int l = 0; l < n; ++l)
                for (int m = 0; m < n; ++m) {
                    const double got = f.H[((i * n + h) * n + l) * n + m];
                    CHECK(fabs(got - H[(h * n + l) * n + m]) <= 1e-11 * (Habs + 1.0));
                    CHECK(memcmp(&got, &f.H[((i * n + h) * n + m) * n + l], 8) == 0);
                }
    }

    // ---- adjoint
    const Adjoint a = adjoint(c, grid, q, npts, u, A, G), b = adjoint(c, grid, q, npts, u, A, G);
    CHECK(memcmp(a.dP.data(), b.dP.data(), a.dP.size() * 8) == 0);
    CHECK(memcmp(a.dK.data(), b.dK.data(), a.dK.size() * 8) == 0);
    CHECK(memcmp(a.rows.data(), b.rows.data(), a.rows.size() * 8) == 0);
    const Adjoint r = adjoint(c, grid, q, npts, u, A, G, -1);            // the points reversed
    CHECK(memcmp(a.dP.data(), r.dP.data(), a.dP.size() * 8) == 0);
    CHECK(memcmp(a.dK.data(), r.dK.data(), a.dK.size() * 8) == 0);
    for (int64_t i = 0; i < npts; ++i)
        CHECK(memcmp(&a.rows[i * n], &r.rows[(npts - 1 - i) * n], n * 8) == 0);
    for (int64_t i = 0; i < npts; ++i)
        if (!alive[i])
            for (int h = 0; h < n; ++h)
                CHECK(a.rows[i * n + h] == 0.0);
    // the second sample has every cotangent doubled: every sum and row is twice the first's, exactly
    for (int64_t e = 0; e < values; ++e)
        CHECK(a.dP[values + e] == 2.0 * a.dP[e]);
    for (int e = 0; e < n * (n + 1); ++e)
        CHECK(a.dK[n * (n + 1) + e] == 2.0 * a.dK[e]);
    double scale = 0.0;
    const double L0 = loss(c, grid, q, npts, u, A, G, alive, &scale);
    // dP against L(P + e_hj) - L(P): a few cells of every component, the corners among them
    for (int h = 0; h < n; ++h)
        for (int pick = 0; pick < 6; ++pick) {
            const int64_t j = pick == 0 ? 0 : pick == 1 ? per - 1 : (int64_t)(uniform(seed) * per) % per;
            Vec moved = grid;
            moved[h * per + j] += 1.0;
            const double L1 = loss(c, moved, q, npts, u, A, G, alive);
            CHECK(fabs((L1 - L0) - a.dP[h * per + j]) <= 1e-10 * (scale + 1.0));
        }
    // dK against its plain sum
    for (int h = 0; h < n; ++h)
        for (int l = 0; l <= n; ++l) {
            double want = 0.0, sc = 0.0;
            for (int64_t i = 0; i < npts; ++i) {
                if (!alive[i])
                    continue;
                const double uu = u.empty() ? 0.0 : u[i * n + h];
                const double t = l < n ? uu * q[i * n + l] + (A.empty() ? 0.0 : A[(i * n + h) * n + l]) : uu;
                want += t;
                sc += fabs(t);
            }
            CHECK(fabs(a.dK[h * (n + 1) + l] - want) <= 1e-12 * (sc + 1e-300) * 64);
        }
    // the rows against central differences of L in q, for points well inside a knot cell
    const double step = 1e-4;
    for (int64_t i = 0; i < npts && i < 40; ++i) {
        bool inside = alive[i] != 0;
        for (int k = 0; k < n; ++k) {
            const double s = (double)(c.ncp[k] - 1) / (double)(c.I[k] - 1);
            const double cp = s * (q[i * n + k] + (double)c.off[k]), x = cp - floor(cp);
            inside = inside && x > 2 * step * s + 1e-6 && x < 1.0 - 2 * step * s - 1e-6;
        }
        if (!inside)
            continue;
        std::vector<char> only(npts, 0);
        only[i] = 1;
        for (int p = 0; p < n; ++p) {
            Vec qp = q, qm = q;
            qp[i * n + p] += step;
            qm[i * n + p] -= step;
            double sc = 0.0;
            const double d = (loss(c, grid, qp, npts, u, A, G, only, &sc) - loss(c, grid, qm, npts, u, A, G, only)) /
                             (2 * step);
            CHECK(fabs(d - a.rows[i * n + p]) <= 1e-6 * (sc + 1.0) * 10);
        }
    }
    // one non-finite cotangent on a contributing point: every sum of both samples is NaN (both carry it)
    if (npts > 8 || alive[0]) {
        Vec u2 = u, A2 = A, G2 = G;
        const int64_t i = npts > 8 ? npts / 2 + 4 : 0;
        if (!u2.empty())
            u2[i * n] = NAN;
        else if (!A2.empty())
            A2[i * n * n + n * n - 1] = INFINITY;
        else
            G2[i * n * n * n + n * n * n - 1] = NAN;
        const Adjoint x = adjoint(c, grid, q, npts, u2, A2, G2);
        for (double v : x.dP)
            CHECK(v != v);
        for (double v : x.dK)
            CHECK(v != v);
    }
}

static void no_points(const Case& c)
{
    const int64_t values = c.n * cells_of(c);
    uint64_t seed = 5;
    Vec grid(values);
    for (double& v : grid)
        v = uniform(seed);
    // (with no point there is no cotangent to read: the arrays are empty blocks)
    const Adjoint z = adjoint(c, grid, {}, 0, {}, {}, {});
    for (double v : z.dP)
        CHECK(v == 0.0);
    for (double v : z.dK)
        CHECK(v == 0.0);
    const Forward f = forward(c, grid, {}, 0, true);
    CHECK(f.r.empty() && f.H.empty());
}

// The bound rule of this call: the head holds bP and bK themselves and each quantum has its own state, so a bK that
// overflows makes dK NaN and leaves dP finite.  One sample, two axes, a 4 x 4 grid on an 8 x 8 image, float64, one
// point at (100, 0.5) -- sane: the limit is a control coordinate of 4e15 -- with u = (4e307, 0) and no A, no G:
// bP = 4e307 gives a finite 2 N bP, bK = |u_0 q_0| = 4e309 is not finite.  dP[h, j] is u_h beta(q, j) to the quantum
// 2^(1023 - 62) -- at most four taps of this point fold into one cell, half a quantum each -- and to the rounding of
// the products in fp64 (beta is formed here from plainly evaluated weights: 64 ulp of 4e307 is generous).  In a batch
// the overflow poisons its own sample only: a second sample with u = (1, 0) gives the bits of a call of its own.
static Adjoint overflow_run(int nbatch, const double* u0_of_sample)
{
    using namespace ed;
    const Case c = {2, {4, 4}, {8, 8}, {0, 0}, false};
    const int n = 2, values = 32;
    Block<double> gr((size_t)nbatch * values), pts((size_t)nbatch * n), du((size_t)nbatch * n), rows((size_t)nbatch * n);
    Block<double> dP((size_t)nbatch * values), dK((size_t)nbatch * n * (n + 1));
    uint64_t seed = 11;
    for (int e = 0; e < values; ++e) {
        const double v = uniform(seed) - 0.5;
        for (int b = 0; b < nbatch; ++b)
            gr[b * values + e] = v;
    }
    for (int b = 0; b < nbatch; ++b) {
        pts[b * n] = 100.0, pts[b * n + 1] = 0.5;
        du[b * n] = u0_of_sample[b], du[b * n + 1] = 0.0;
    }
    memset(rows.p, 0xff, rows.n * 8);
    memset(dP.p, 0xff, dP.n * 8);
    memset(dK.p, 0xff, dK.n * 8);
    PointsJetGradCall call;
    memset(&call, 0, sizeof(call));
    call.g = geometry(c, gr.p);
    call.nbatch = nbatch;
    call.npts = 1;
    call.disp_bstride = values * 8;
    call.pos = rows_array(pts.p, 2, n, 1);
    call.du = rows_array(du.p, 2, n, 1);
    call.dpts = rows_array(rows.p, 2, n, 1);
    call.ddisp.ptr = (char*)dP.p;
    call.ddisp.dtype = EDHIP_F64;
    call.ddisp.stride[0] = 16 * 8, call.ddisp.stride[1] = 4 * 8, call.ddisp.stride[2] = 8;
    call.ddisp.bstride = values * 8;
    call.dK.ptr = (char*)dK.p;
    call.dK.dtype = EDHIP_F64;
    call.dK.stride[0] = (n + 1) * 8, call.dK.stride[1] = 8;
    call.dK.bstride = n * (n + 1) * 8;
    Block<char> scratch(points_jet_scratch_bytes(call.g, nbatch));
    memset(scratch.p, 0xff, scratch.n);
    call.scratch = scratch.p;
    CHECK(launch_deform_points_derivatives_gradient(call, nullptr) == hipSuccess);
    Adjoint r;
    r.rows.assign(rows.p, rows.p + rows.n);
    r.dP.assign(dP.p, dP.p + dP.n);
    r.dK.assign(dK.p, dK.p + dK.n);
    return r;
}

static void overflowing_bound()
{
    const double huge[2] = {4e307, 1.0}, one[1] = {1.0};
    const Adjoint x = overflow_run(1, huge), both = overflow_run(2, huge), alone = overflow_run(1, one);
    // beta(q, j): the cubic weights of each axis at cp = 3 q / 7, folded onto the four control points
    double beta[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    const double q[2] = {100.0, 0.5};
    for (int k = 0; k < 2; ++k) {
        const double cp = 3.0 * q[k] / 7.0, fl = floor(cp), t = cp - fl, z = 1.0 - t;
        const double w[4] = {z * z * z / 6, (3 * t * t * t - 6 * t * t + 4) / 6, (3 * z * z * z - 6 * z * z + 4) / 6,
                             t * t * t / 6};
        for (int s = 0; s < 4; ++s)
            beta[k][fold((int64_t)fl - 1 + s, 4)] += w[s];
    }
    const double tol = 2.0 * ldexp(1.0, 1023 - 62) + 64.0 * ldexp(4e307, -52);
    for (int j0 = 0; j0 < 4; ++j0)
        for (int j1 = 0; j1 < 4; ++j1) {
            const double got = x.dP[j0 * 4 + j1];
            CHECK(std::isfinite(got) && fabs(got - 4e307 * (beta[0][j0] * beta[1][j1])) <= tol);
            CHECK(x.dP[16 + j0 * 4 + j1] == 0.0);
        }
    for (double v : x.dK)
        CHECK(v != v);
    CHECK(std::isfinite(x.rows[0]) && std::isfinite(x.rows[1]));
    // the batch: sample 0 as the single call, sample 1 the bits of its own call
    CHECK(memcmp(both.dP.data(), x.dP.data(), 32 * 8) == 0 && memcmp(both.dK.data(), x.dK.data(), 6 * 8) == 0);
    CHECK(memcmp(both.rows.data(), x.rows.data(), 2 * 8) == 0);
    CHECK(memcmp(both.dP.data() + 32, alone.dP.data(), 32 * 8) == 0);
    CHECK(memcmp(both.dK.data() + 6, alone.dK.data(), 6 * 8) == 0);
    CHECK(memcmp(both.rows.data() + 2, alone.rows.data(), 2 * 8) == 0);
    for (int e = 0; e < 16; ++e)
        CHECK(fabs(alone.dP[e] - beta[0][e / 4] * beta[1][e % 4]) <= 1e-14);
    CHECK(alone.dK[0] == 100.0 && alone.dK[1] == 0.5 && alone.dK[2] == 1.0);
}

int main()
{
    overflowing_bound();
    const Case two[3] = {{1, {2}, {9}, {0}, false}, {2, {2, 2}, {9, 11}, {1, 0}, true}, {3, {2, 2, 2}, {9, 7, 8}, {0, 2, 1}, true}};
    const Case mid[3] = {{1, {5}, {17}, {3}, true}, {2, {4, 5}, {13, 17}, {2, 3}, true}, {3, {4, 4, 5}, {12, 14, 10}, {1, 0, 2}, false}};
    // more than kPointsLdsValues = 7680 values: the grid is read from, and the cells live in, global memory
    const Case big[3] = {{1, {7700}, {9000}, {0}, false}, {2, {64, 64}, {70, 70}, {0, 0}, false}, {3, {14, 14, 14}, {16, 16, 16}, {0, 1, 0}, true}};
    for (int k = 0; k < 3; ++k) {
        for (int which = 0; which < 4; ++which) {
            one_case(two[k], 300, which);
            one_case(mid[k], 65, which);
        }
        one_case(mid[k], 1, 0);
        one_case(two[k], 1, 0);
        one_case(big[k], 40, 0);
        one_case(big[k], 1, 3);
        no_points(mid[k]);
        no_points(big[k]);
    }
    printf(failures ? "%d checks failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
