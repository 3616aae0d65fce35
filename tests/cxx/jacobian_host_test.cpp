// Host-only run of the kernels of csrc/deform_jacobian.hip (jacobian_kernel, jacobian_grad_rows / _mid / _finish) under
// AddressSanitizer and UndefinedBehaviorSanitizer: the device functions compiled as plain C++ against the stand-in
// runtime of tests/cxx/host_hip (one emulated thread per workgroup, dynamic LDS poisoned beyond the launch's size).
// Every array is a heap block of exactly the promised size, so a read or write beyond it is a report.  Cases: 1, 2 and
// 3 axes, the two-point grid (every tap folds), grids read from global memory, a row of one voxel, a last grid axis too
// long for the row contraction (the per-voxel route of the forward; units of the gradient that reach a window of the
// axis: 3 x 129, 3 x 3 x 64, 600 points, 40 points on 12 voxels), a crop with an affine map, two samples; and a sweep
// of axes for the window of control points a unit reaches (inside the axis, within the launch's room, holding every
// tap).  Checked:
// det against a plain 4^n-tap evaluation written here, det of a crop against the whole lattice (same bits),
// sum_j dP[h, j] = 0, dK against the plain sum of g C, entries of dP against central differences of L = sum g det
// with step 1 (exact up to rounding: det is affine in every grid value), bit-equal results from two runs.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
//       -Itests/cxx/host_hip -Ielasticdeform_amd/csrc -Iinclude tests/cxx/jacobian_host_test.cpp -o t && ./t
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "deform_jacobian.hip"

namespace ed {
namespace {
double s_grid[kHostLdsBytes / 8];
}  // namespace
}  // namespace ed

void host_lds_begin()
{
    // LDS is not cleared between workgroups and ends at the launch's size
    HOST_HIP_UNPOISON(ed::s_grid, kHostLdsBytes);
    memset(ed::s_grid, 0xff, kHostLdsBytes);
    HOST_HIP_POISON((char*)ed::s_grid + host_lds_bytes, kHostLdsBytes - host_lds_bytes);
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

struct Case {
    int n;
    int64_t I[3], ncp[3], off[3], O[3];
    bool affine;
    int nbatch;
};

static int64_t prod(const int64_t* v, int n)
{
    int64_t p = 1;
    for (int k = 0; k < n; ++k)
        p *= v[k];
    return p;
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
    g.nvox = 1;
    for (int k = c.n - 1; k >= 0; --k) {
        g.in_len[k] = c.I[k];
        g.out_len[k] = c.O[k];
        g.off[k] = c.off[k];
        g.ncp[k] = c.ncp[k];
        g.disp_stride[k + 1] = stride;
        stride *= c.ncp[k];
        g.nvox *= c.O[k];
    }
    g.disp_stride[0] = stride;
    for (int h = 0; h < c.n; ++h)
        for (int l = 0; l <= c.n; ++l)
            g.affine[h * (c.n + 1) + l] = (h == l ? 1.0 : 0.0) + 0.07 * (h - l) + 0.01 * l;
    return g;
}

// ---- the plain evaluation ------------------------------------------------------------------------------------------
static int64_t fold(int64_t i, int64_t len)
{
    if (len == 1)
        return 0;
    const int64_t period = 2 * len - 2;
    i %= period;
    if (i < 0)
        i += period;
    return i < len ? i : period - i;
}

static void plain_jacobian(const Case& c, const ed::GridGeom& g, const double* grid, const int64_t* o, double J[3][3])
{
    const int n = c.n;
    double w[3][4], dw[3][4];
    int64_t m[3][4];
    for (int k = 0; k < n; ++k) {
        const double s = (double)(c.ncp[k] - 1) / (double)(c.I[k] - 1);
        const double cp = (double)(c.ncp[k] - 1) * (double)(o[k] + c.off[k]) / (double)(c.I[k] - 1);
        const double fl = std::floor(cp), x = cp - fl, z = 1.0 - x;
        w[k][0] = z * z * z / 6.0;
        w[k][1] = (3.0 * x * x * x - 6.0 * x * x + 4.0) / 6.0;
        w[k][2] = (-3.0 * x * x * x + 3.0 * x * x + 3.0 * x + 1.0) / 6.0;
        w[k][3] = x * x * x / 6.0;
        dw[k][0] = -z * z / 2.0 * s;
        dw[k][1] = (3.0 * x * x - 4.0 * x) / 2.0 * s;
        dw[k][2] = (-3.0 * x * x + 2.0 * x + 1.0) / 2.0 * s;
        dw[k][3] = x * x / 2.0 * s;
        for (int t = 0; t < 4; ++t)
            m[k][t] = fold((int64_t)fl - 1 + t, c.ncp[k]);
    }
    const int64_t per = prod(c.ncp, n);
    for (int h = 0; h < n; ++h)
        for (int l = 0; l < n; ++l) {
            double acc = 0.0;
            const int taps = 1 << (2 * n);
            for (int t = 0; t < taps; ++t) {
                int64_t idx = 0;
                double wt = 1.0;
                for (int k = 0; k < n; ++k) {
                    const int tk = (t >> (2 * (n - 1 - k))) & 3;
                    idx = idx * c.ncp[k] + m[k][tk];
                    wt *= k == l ? dw[k][tk] : w[k][tk];
                }
                acc += grid[h * per + idx] * wt;
            }
            J[h][l] = acc + (c.affine ? g.affine[h * (n + 1) + l] : (h == l ? 1.0 : 0.0));
        }
}

static double plain_det(int n, const double J[3][3], double C[3][3])
{
    if (n == 1) {
        C[0][0] = 1.0;
        return J[0][0];
    }
    if (n == 2) {
        C[0][0] = J[1][1], C[0][1] = -J[1][0], C[1][0] = -J[0][1], C[1][1] = J[0][0];
        return J[0][0] * J[1][1] - J[0][1] * J[1][0];
    }
    for (int h = 0; h < 3; ++h)
        for (int l = 0; l < 3; ++l) {
            const int h1 = (h + 1) % 3, h2 = (h + 2) % 3, l1 = (l + 1) % 3, l2 = (l + 2) % 3;
            C[h][l] = J[h1][l1] * J[h2][l2] - J[h1][l2] * J[h2][l1];
        }
    return J[0][0] * C[0][0] + J[0][1] * C[0][1] + J[0][2] * C[0][2];
}

// ---- the kernels ---------------------------------------------------------------------------------------------------
static std::vector<double> run_forward(const Case& c, const double* grid)
{
    using namespace ed;
    const int64_t nvox = prod(c.O, c.n), values = c.n * prod(c.ncp, c.n);
    Block<double> det((size_t)c.nbatch * nvox);
    for (size_t i = 0; i < det.n; ++i)
        det[i] = -777.0;
    JacobianCall call;
    memset(&call, 0, sizeof(call));
    call.g = geometry(c, grid);
    call.nbatch = c.nbatch;
    call.disp_bstride = values * 8;
    call.det.ptr = (char*)det.p;
    call.det.dtype = EDHIP_F64;
    int64_t stride = 8;
    for (int k = c.n - 1; k >= 0; --k) {
        call.det.stride[k] = stride;
        stride *= c.O[k];
    }
    call.det.bstride = nvox * 8;
    CHECK(launch_deform_jacobian(call, nullptr) == hipSuccess);
    return std::vector<double>(det.p, det.p + det.n);
}

struct Grad {
    std::vector<double> dP, dK;
};

static Grad run_gradient(const Case& c, const double* grid, const double* cot)
{
    using namespace ed;
    const int n = c.n;
    const int64_t nvox = prod(c.O, n), values = n * prod(c.ncp, n);
    Block<double> gcot((size_t)c.nbatch * nvox), dP((size_t)c.nbatch * values), dK((size_t)c.nbatch * n * (n + 1));
    memcpy(gcot.p, cot, gcot.n * 8);
    JacobianCall call;
    memset(&call, 0, sizeof(call));
    call.g = geometry(c, grid);
    call.nbatch = c.nbatch;
    call.disp_bstride = values * 8;
    call.det.ptr = (char*)gcot.p;
    call.det.dtype = EDHIP_F64;
    int64_t stride = 8;
    for (int k = n - 1; k >= 0; --k) {
        call.det.stride[k] = stride;
        stride *= c.O[k];
    }
    call.det.bstride = nvox * 8;
    call.ddisp.ptr = (char*)dP.p;
    call.ddisp.dtype = EDHIP_F64;
    call.ddisp.bstride = values * 8;
    stride = 8;
    for (int k = n; k >= 1; --k) {
        call.ddisp.stride[k] = stride;
        stride *= c.ncp[k - 1];
    }
    call.ddisp.stride[0] = stride;
    call.dK.ptr = (char*)dK.p;
    call.dK.dtype = EDHIP_F64;
    call.dK.stride[0] = (n + 1) * 8;
    call.dK.stride[1] = 8;
    call.dK.bstride = n * (n + 1) * 8;
    Block<char> scratch(jacobian_grad_scratch_bytes(call.g, c.nbatch));
    memset(scratch.p, 0xff, scratch.n);                      // nothing may rely on what an earlier call left
    call.scratch = scratch.p;
    CHECK(launch_deform_jacobian_gradient(call, nullptr) == hipSuccess);
    Grad r;
    r.dP.assign(dP.p, dP.p + dP.n);
    r.dK.assign(dK.p, dK.p + dK.n);
    return r;
}

static void one_case(const Case& c, bool gradient)
{
    const int n = c.n;
    const int64_t nvox = prod(c.O, n), per = prod(c.ncp, n), values = n * per;
    uint64_t seed = 100 * n + c.ncp[n - 1];
    Block<double> grid((size_t)c.nbatch * values);
    for (size_t i = 0; i < grid.n; ++i)
        grid[i] = 4.0 * (uniform(seed) - 0.5);
    std::vector<double> cot((size_t)c.nbatch * nvox);
    for (double& v : cot)
        v = uniform(seed) - 0.5;

    const std::vector<double> det = run_forward(c, grid.p);
    const std::vector<double> again = run_forward(c, grid.p);
    CHECK(memcmp(det.data(), again.data(), det.size() * 8) == 0);
    std::vector<double> wantK((size_t)c.nbatch * n * n, 0.0), absK(wantK.size(), 0.0);
    double scale = 0.0;
    for (int b = 0; b < c.nbatch; ++b) {
        const ed::GridGeom g = geometry(c, grid.p + b * values);
        for (int64_t i = 0; i < nvox; ++i) {
            int64_t o[3] = {0, 0, 0}, rem = i;
            for (int k = n - 1; k >= 0; --k) {
                o[k] = rem % c.O[k];
                rem /= c.O[k];
            }
            double J[3][3], C[3][3];
            plain_jacobian(c, g, grid.p + b * values, o, J);
            const double want = plain_det(n, J, C);
            double bound = 1.0;
            for (int h = 0; h < n; ++h) {
                double row = 0.0;
                for (int l = 0; l < n; ++l)
                    row += std::fabs(J[h][l]);
                bound *= row > 1.0 ? row : 1.0;
            }
            scale = bound > scale ? bound : scale;
            CHECK(std::fabs(det[b * nvox + i] - want) <= 1e-12 * bound);
            for (int h = 0; h < n; ++h)
                for (int l = 0; l < n; ++l) {
                    wantK[(b * n + h) * n + l] += cot[b * nvox + i] * C[h][l];
                    absK[(b * n + h) * n + l] += std::fabs(cot[b * nvox + i] * C[h][l]);
                }
        }
    }
    // a crop of the lattice: the same bits (no affine map: with one, K acts on the crop-local index)
    if (!c.affine && c.O[n - 1] > 2) {
        Case crop = c;
        crop.off[n - 1] += 1;
        crop.O[n - 1] -= 2;
        if (n > 1 && c.O[0] > 1) {
            crop.off[0] += 1;
            crop.O[0] -= 1;
        }
        const std::vector<double> part = run_forward(crop, grid.p);
        const int64_t cvox = prod(crop.O, n);
        for (int b = 0; b < c.nbatch; ++b)
            for (int64_t i = 0; i < cvox; ++i) {
                int64_t rem = i, full = 0, mul = 1;
                for (int k = n - 1; k >= 0; --k) {
                    const int64_t ok = rem % crop.O[k] + crop.off[k] - c.off[k];
                    rem /= crop.O[k];
                    full += ok * mul;
                    mul *= c.O[k];
                }
                CHECK(memcmp(&part[b * cvox + i], &det[b * nvox + full], 8) == 0);
            }
    }
    if (!gradient)
        return;

    const Grad a = run_gradient(c, grid.p, cot.data());
    const Grad a2 = run_gradient(c, grid.p, cot.data());
    CHECK(memcmp(a.dP.data(), a2.dP.data(), a.dP.size() * 8) == 0);
    CHECK(memcmp(a.dK.data(), a2.dK.data(), a.dK.size() * 8) == 0);
    double gsum = 0.0;
    for (double v : cot)
        gsum += std::fabs(v);
    const double tol = 1e-12 * scale * gsum * 4.0;          // 4: a loose bound on s_l sum_t |w'_t| times the taps' sum
    for (int b = 0; b < c.nbatch; ++b)
        for (int h = 0; h < n; ++h) {
            double sum = 0.0;
            for (int64_t j = 0; j < per; ++j)
                sum += a.dP[(b * n + h) * per + j];
            CHECK(std::fabs(sum) <= tol);                    // the d beta sum to zero over j
            for (int l = 0; l < n; ++l)
                CHECK(std::fabs(a.dK[(b * n + h) * (n + 1) + l] - wantK[(b * n + h) * n + l]) <=
                      1e-12 * (absK[(b * n + h) * n + l] + 1.0));
            CHECK(a.dK[(b * n + h) * (n + 1) + n] == 0.0);
        }
    // central differences with step 1 of L = sum g det in 6 grid values: exact up to rounding
    for (int trial = 0; trial < 6; ++trial) {
        const size_t e = (size_t)(uniform(seed) * (double)grid.n) % grid.n;
        const double keep = grid[e];
        double L[2];
        for (int s = 0; s < 2; ++s) {
            grid[e] = keep + (s ? -1.0 : 1.0);
            const std::vector<double> d = run_forward(c, grid.p);
            L[s] = 0.0;
            for (size_t i = 0; i < d.size(); ++i)
                L[s] += cot[i] * d[i];
        }
        grid[e] = keep;
        CHECK(std::fabs((L[0] - L[1]) / 2.0 - a.dP[e]) <= tol * 16.0);
    }
}

// the window of control points a unit of the gradient reaches: inside the axis, no wider than the launch's room for
// it, and holding every folded tap of every voxel of the unit -- over a sweep of axes, extents and crops
static void window_bounds()
{
    using namespace ed;
    const int64_t ncps[] = {2, 3, 4, 5, 6, 7, 9, 33, 129, 600, 5000}, lens[] = {2, 3, 9, 50, 300, 1000};
    for (int64_t ncp : ncps)
        for (int64_t len : lens)
            for (int64_t off = 0; off < len; off += 1 + len / 3) {
                GridGeom g;
                memset(&g, 0, sizeof(g));
                g.naxis = 1;
                g.in_len[0] = len;
                g.out_len[0] = len - off;
                g.off[0] = off;
                g.ncp[0] = ncp;
                g.nvox = len - off;
                PointsArgs p;
                memset(&p, 0, sizeof(p));
                fill_points_args(p, g, 0, nullptr, 0, 0.0);
                const GradShape s = grad_shape(g);
                CHECK(s.xc >= 1 && s.wmax >= 1 && s.wmax <= 512 && 2 * s.xc * s.wstride <= kJacDenseValues);
                CHECK((int64_t)s.nch * s.xc >= g.out_len[0]);
                for (int64_t ch = 0; ch < s.nch; ++ch) {
                    const int64_t x0 = ch * s.xc, x1 = (x0 + s.xc < g.out_len[0] ? x0 + s.xc : g.out_len[0]) - 1;
                    int jlo, w;
                    reached_window(p, 0, x0, x1, jlo, w);
                    CHECK(jlo >= 0 && w >= 1 && jlo + w <= ncp && w <= s.wmax);
                    for (int64_t x = x0; x <= x1; ++x) {
                        double wt[4], dwt[4];
                        int m[4];
                        axis_taps(p, 0, x, wt, dwt, m);
                        for (int t = 0; t < 4; ++t)
                            CHECK(m[t] >= jlo && m[t] < jlo + w);
                    }
                }
            }
}

int main()
{
    const Case cases[] = {
        {1, {40}, {5}, {0}, {40}, false, 1},
        {1, {40}, {2}, {3}, {30}, true, 2},                          // the two-point grid: every tap folds
        {1, {700}, {600}, {0}, {700}, false, 1},                     // a last grid axis beyond the row contraction
        {2, {13, 17}, {4, 5}, {2, 3}, {9, 12}, false, 2},
        {2, {9, 9}, {2, 2}, {0, 0}, {9, 9}, true, 1},
        {2, {11, 1 + 1}, {3, 3}, {0, 1}, {11, 1}, false, 1},         // a row of one voxel
        {2, {70, 70}, {64, 64}, {0, 0}, {7, 70}, false, 1},          // 8192 values: the grid from global memory
        {3, {12, 14, 10}, {4, 4, 5}, {0, 0, 0}, {12, 14, 10}, false, 1},
        {3, {9, 9, 9}, {2, 2, 2}, {0, 0, 0}, {9, 9, 9}, false, 2},
        {3, {9, 9, 9}, {5, 3, 2}, {0, 0, 0}, {9, 9, 9}, true, 1},    // voxels on knots
        {3, {5, 6, 300}, {3, 3, 7}, {1, 1, 2}, {3, 4, 290}, true, 1},   // a row of two units
        {3, {2, 2, 2}, {3, 3, 3}, {0, 0, 0}, {2, 2, 2}, false, 1},
        {3, {6, 5, 4}, {16, 16, 11}, {0, 0, 0}, {6, 5, 4}, false, 1},   // 8448 values: global memory
        // last grid axes beyond the forward's row contraction: the gradient's units reach a window of them
        {2, {20, 300}, {3, 129}, {0, 0}, {20, 300}, false, 1},
        {3, {6, 5, 130}, {3, 3, 64}, {0, 1, 2}, {6, 4, 126}, true, 2},
        {1, {12}, {40}, {0}, {12}, false, 1},                           // more control points than voxels
    };
    for (const Case& c : cases)
        one_case(c, true);
    window_bounds();
    printf(failures ? "%d checks failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
