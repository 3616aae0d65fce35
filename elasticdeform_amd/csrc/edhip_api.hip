// edhip_api.hip -- the C ABI of include/edhip.h: argument validation (the checks of
// Py_DeformGrid_helper, _deform_grid.c:121-255, and Py_SplineFilter1D_grad, :71-81), kernel
// selection and stream-ordered launches.  No Python, NumPy or torch types.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ed_device.h"
#include "ed_params.h"
#include "ed_points_jet.h"
#include "ed_workspace.h"
#include "edhip.h"

namespace {

int fail(char* err, size_t errlen, int code, const char* fmt, ...)
{
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return code;
}

int hip_fail(char* err, size_t errlen, hipError_t e, const char* what)
{
    if (e == hipErrorOutOfMemory)
        return fail(err, errlen, EDHIP_ERR_MEMORY, "%s: out of device memory", what);
    return fail(err, errlen, EDHIP_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

bool dtype_ok(int dt) { return dt >= 0 && dt < EDHIP_NUM_DTYPES; }

int dtype_size(int dt)
{
    switch (dt) {
    case EDHIP_BOOL: case EDHIP_U8: case EDHIP_I8: return 1;
    case EDHIP_U16: case EDHIP_I16: case EDHIP_F16: case EDHIP_BF16: return 2;
    case EDHIP_U32: case EDHIP_I32: case EDHIP_F32: return 4;
    default: return 8;
    }
}

int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }

// ---- the checks the entry points share: each returns EDHIP_OK or the refusal, with its message in err --------------
int check_naxis(int naxis, char* err, size_t errlen)
{
    if (naxis < 1)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis list");
    if (naxis > ed::kMaxAxes)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED,
                    "more than %d deformed axes are not supported on the GPU", ed::kMaxAxes);
    return EDHIP_OK;
}

// the control grid: (naxis, ncp_0, ...), a known dtype, no empty axis; *points (if wanted): its number of values
int check_displacement(const edhip_array* d, int naxis, int64_t* points, char* err, size_t errlen)
{
    if (!d || d->ndim != naxis + 1 || d->shape[0] != naxis)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid displacement shape");
    if (!dtype_ok(d->dtype))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    int64_t total = 1;
    for (int k = 0; k <= naxis; ++k) {
        if (d->shape[k] <= 0)
            return fail(err, errlen, EDHIP_ERR_INVALID, "invalid displacement shape");
        total *= d->shape[k];
    }
    if (points)
        *points = total;
    return EDHIP_OK;
}

// ---- what the strided-batch calls on the prefiltered grid share (points, their gradient, labels, inverse) -----------
// the preamble: an empty message; a negative batch or a missing required argument is refused
int check_batch_call(int nbatch, bool required_given, char* err, size_t errlen)
{
    if (err && errlen)
        err[0] = 0;
    if (nbatch < 0 || !required_given)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid batch");
    return EDHIP_OK;
}

// the image-side calls: an axis list of 1 to 3 deformed axes
int check_axes_1_to_3(const char* entry, const int32_t* axis, int naxis, char* err, size_t errlen)
{
    if (!axis || naxis < 1)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis list");
    if (naxis > 3)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "%s takes 1 to 3 deformed axes", entry);
    return EDHIP_OK;
}

int check_prefiltered(const char* entry, uint32_t flags, char* err, size_t errlen)
{
    if (flags & EDHIP_FLAG_RAW_DISPLACEMENT)
        return fail(err, errlen, EDHIP_ERR_INVALID, "%s takes the prefiltered control grid", entry);
    return EDHIP_OK;
}

// blockIdx.y carries the sample
int check_batch_limit(const char* entry, int nbatch, char* err, size_t errlen)
{
    if (nbatch > 65535)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "%s: too many samples", entry);
    return EDHIP_OK;
}

// exactly this rank (at most EDHIP_MAX_DIMS) and these extents
bool has_shape(const edhip_array* a, int ndim, const int64_t* shape)
{
    bool same = a->ndim == ndim;
    for (int d = 0; same && d < ndim; ++d)
        same = a->shape[d] == shape[d];
    return same;
}

bool f32_or_f64(const edhip_array* a) { return a->dtype == EDHIP_F32 || a->dtype == EDHIP_F64; }

// an optional per-point array of rank `ndim`: (N, naxis, ...), float64 only or float32 / float64
int check_point_rows(const edhip_array* a, const char* name, int ndim, const int64_t* rows, bool f64_only, char* err,
                     size_t errlen)
{
    if (!a)
        return EDHIP_OK;
    if (!has_shape(a, ndim, rows))
        return fail(err, errlen, EDHIP_ERR_INVALID, "%s must have shape (N%s)", name,
                    ndim == 2 ? ", naxis" : ndim == 3 ? ", naxis, naxis" : ", naxis, naxis, naxis");
    if (f64_only ? a->dtype != EDHIP_F64 : !f32_or_f64(a))
        return fail(err, errlen, EDHIP_ERR_DTYPE, f64_only ? "%s must be float64" : "%s must be float32 or float64",
                    name);
    return EDHIP_OK;
}

// the dtype rules of ddisplacement, by entry
bool f32_or_f64_dtype(int dt) { return dt == EDHIP_F32 || dt == EDHIP_F64; }
bool floating_dtype(int dt) { return dt == EDHIP_F16 || dt == EDHIP_BF16 || f32_or_f64_dtype(dt); }
const char* const kFloatingDdisp = "ddisplacement must have a floating-point dtype";

// The two sums a gradient entry leaves, each optional: ddisplacement with the shape of the (checked) displacement and
// a dtype the entry takes -- `ddisp_dtype`, refused with `ddisp_dtype_message` --, dinverse_affine float64
// (naxis, naxis + 1).
int check_gradient_outputs(const edhip_array* ddisplacement, const edhip_array* displacement, bool (*ddisp_dtype)(int),
                           const char* ddisp_dtype_message, const edhip_array* dinverse_affine, int naxis, char* err,
                           size_t errlen)
{
    if (ddisplacement) {
        if (!has_shape(ddisplacement, displacement->ndim, displacement->shape))
            return fail(err, errlen, EDHIP_ERR_INVALID, "ddisplacement must have the shape of displacement");
        if (!ddisp_dtype(ddisplacement->dtype))
            return fail(err, errlen, EDHIP_ERR_DTYPE, "%s", ddisp_dtype_message);
    }
    if (dinverse_affine) {
        const int64_t map[2] = {naxis, naxis + 1};
        if (!has_shape(dinverse_affine, 2, map))
            return fail(err, errlen, EDHIP_ERR_INVALID, "dinverse_affine must have shape (naxis, naxis + 1)");
        if (dinverse_affine->dtype != EDHIP_F64)
            return fail(err, errlen, EDHIP_ERR_DTYPE, "dinverse_affine must be float64");
    }
    return EDHIP_OK;
}

// The tail of the point-gradient entries: `bytes` of the stream's workspace, behind its grid head, as the call's
// scratch; then the launch, reported as `what`.
template <typename Call>
int launch_with_scratch(Call& c, size_t bytes, hipError_t (*launch)(const Call&, hipStream_t), const char* what,
                        hipStream_t stream, char* err, size_t errlen)
{
    ed::StreamGuard guard(stream);
    hipError_t e = hipSuccess;
    char* ws = (char*)ed::workspace_reserve(stream, ed::kWorkspaceGridBytes + bytes, &e);
    if (!ws)
        return hip_fail(err, errlen, e, "scratch allocation");
    c.scratch = ws + ed::kWorkspaceGridBytes;
    e = launch(c, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, what);
    return EDHIP_OK;
}

// the optional solved-mask of the inverse direction: uint8 (npts)
int check_status(const edhip_array* status, bool inverse, int64_t npts, char* err, size_t errlen)
{
    if (!status)
        return EDHIP_OK;
    if (!inverse)
        return fail(err, errlen, EDHIP_ERR_INVALID, "the status belongs to the inverse direction");
    if (!has_shape(status, 1, &npts))
        return fail(err, errlen, EDHIP_ERR_INVALID, "status must have shape (N)");
    if (status->dtype != EDHIP_U8)
        return fail(err, errlen, EDHIP_ERR_DTYPE, "status must be uint8");
    return EDHIP_OK;
}

// the controls of the Newton iteration, and the inverse of the affine map's linear part it starts from
int check_iteration(int max_iter, double tol, const double* affine, const double* forward_linear, char* err,
                    size_t errlen)
{
    if (max_iter < 1)
        return fail(err, errlen, EDHIP_ERR_INVALID, "max_iter must be at least 1");
    if (!(tol > 0.0))
        return fail(err, errlen, EDHIP_ERR_INVALID, "tol must be positive");
    if (affine && !forward_linear)
        return fail(err, errlen, EDHIP_ERR_INVALID, "forward_linear is required with an affine map");
    return EDHIP_OK;
}

// sample 0's array and the byte distance between samples, as the launchers take them; nullptr: a zeroed struct
ed::BatchArray batch_array(const edhip_array* a, int64_t bstride)
{
    ed::BatchArray s;
    memset(&s, 0, sizeof(s));
    if (a) {
        s.ptr = (char*)a->data;
        s.dtype = a->dtype;
        for (int d = 0; d < a->ndim && d < EDHIP_MAX_DIMS; ++d)
            s.stride[d] = a->stride_bytes[d];
        s.bstride = bstride;
    }
    return s;
}

// the checks of _deform_grid.c:121-255 on the input/output pairs of edhip_deform and of its gradients (float_only:
// floating-point volumes only -- the derivative of an integer volume's rounded result is not defined)
int check_pairs(const edhip_array* inputs, const edhip_array* outputs, int ninputs, int naxis, const int32_t* axis,
                const int32_t* orders, const int32_t* modes, const double* cvals, bool float_only, char* err,
                size_t errlen)
{
    if (!inputs || !outputs || ninputs <= 0 || ninputs > EDHIP_MAX_INPUTS)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid number of inputs/outputs");
    if (!axis || !orders || !modes || !cvals)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis list");
    if (const int st = check_naxis(naxis, err, errlen))
        return st;
    for (int i = 0; i < ninputs; ++i) {
        const edhip_array& in = inputs[i];
        const edhip_array& out = outputs[i];
        if (in.ndim != out.ndim)
            return fail(err, errlen, EDHIP_ERR_INVALID, "input and output dimensions should match");
        if (in.ndim < 1 || in.ndim > EDHIP_MAX_DIMS)
            return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "arrays must have 1..%d dimensions",
                        EDHIP_MAX_DIMS);
        const bool floats = (in.dtype == EDHIP_F32 || in.dtype == EDHIP_F64) &&
                            (out.dtype == EDHIP_F32 || out.dtype == EDHIP_F64);
        if (!dtype_ok(in.dtype) || !dtype_ok(out.dtype) || (float_only && !floats))
            return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
        for (int j = 0; j < naxis; ++j) {
            const int a = axis[i * naxis + j];
            if (a < 0 || a >= in.ndim)
                return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis in axis list");
            if (in.shape[a] != inputs[0].shape[axis[j]])
                return fail(err, errlen, EDHIP_ERR_INVALID, "all inputs should have the same size");
            if (out.shape[a] != outputs[0].shape[axis[j]])
                return fail(err, errlen, EDHIP_ERR_INVALID, "all outputs should have the same size");
        }
        if (orders[i] < 0 || orders[i] > 5)
            return fail(err, errlen, EDHIP_ERR_INVALID, "spline order not supported");
        if (modes[i] < 0 || modes[i] > 4)
            return fail(err, errlen, EDHIP_ERR_INVALID, "boundary mode not supported");
    }
    return EDHIP_OK;
}

// deformed extents of an input and an output
void deformed_lengths(const edhip_array& in0, const edhip_array& out0, int naxis, const int32_t* axis,
                      int64_t* in_len, int64_t* out_len)
{
    for (int k = 0; k < naxis; ++k) {
        in_len[k] = in0.shape[axis[k]];
        out_len[k] = out0.shape[axis[k]];
    }
}

// sample b of a strided batch
edhip_array sample(const edhip_array& a, int b, int64_t bstride)
{
    edhip_array s = a;
    s.data = (char*)a.data + (int64_t)b * bstride;
    return s;
}

// Geometry shared by every input of a call (deform.c:381-391,439-451,771-776).  Host arithmetic only: nothing is
// launched or reserved; g.disp is the caller's grid (a raw one is staged by stage_raw_grid).
int fill_geometry(const edhip_array* displacement, const int64_t* in_len, const int64_t* out_len,
                  const int64_t* output_offset, int naxis, const double* affine, ed::GridGeom& g, char* err,
                  size_t errlen)
{
    memset(&g, 0, sizeof(g));
    g.naxis = naxis;
    g.has_affine = affine != nullptr;
    g.disp_dtype = displacement->dtype;
    g.disp = (const char*)displacement->data;
    g.nvox = 1;
    for (int k = 0; k < naxis; ++k) {
        g.in_len[k] = in_len[k];
        g.out_len[k] = out_len[k];
        g.off[k] = output_offset ? output_offset[k] : 0;
        g.ncp[k] = displacement->shape[k + 1];
        g.nvox *= g.out_len[k];
        if (g.out_len[k] > 0 && g.in_len[k] < 2)
            // the reference divides by (I_k - 1) (deform.c:643,655): undefined there, refused here
            return fail(err, errlen, EDHIP_ERR_INVALID,
                        "deformed axes must have at least 2 elements");
    }
    for (int k = 0; k <= naxis; ++k)
        g.disp_stride[k] = displacement->stride_bytes[k];
    if (affine)
        for (int k = 0; k < naxis * (naxis + 1); ++k)
            g.affine[k] = affine[k];
    return EDHIP_OK;
}

// A raw grid's order-3 prefilter that has not been enqueued yet (gp.total == 0: nothing to filter) and what the
// stream's stamp becomes once it is.
struct PendingGrid {
    ed::GridPrefilter gp;
    ed::GridStamp stamp;
};

// EDHIP_FLAG_RAW_DISPLACEMENT: the control grid is prefiltered into the head of the stream's workspace, where g.disp
// then points.  The filtered copy of this very grid may still be there (EDHIP_FLAG_GRID_STAYS and a matching stamp);
// otherwise the one-workgroup prefilter is launched here -- or, with `defer`, left to the caller (edhip_deform: the
// tables kernel of the tile path filters the grid inside its own launch).  f64_volumes: see deform_tile_workspace_bytes.
int stage_raw_grid(const edhip_array* displacement, uint32_t flags, hipStream_t stream, bool f64_volumes,
                   ed::GridGeom& g, PendingGrid* defer, char* err, size_t errlen)
{
    using namespace ed;
    const int naxis = g.naxis;
    int64_t total = 1;
    for (int k = 0; k <= naxis; ++k)
        total *= displacement->shape[k];
    if (total > 4096)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED,
                    "raw displacement grids are limited to 4096 points");
    // reserve everything this call can need now: a later, larger request would move the buffer
    // and lose the grid
    hipError_t e = hipSuccess;
    void* ws = workspace_reserve(stream, deform_tile_workspace_bytes(g, 1, f64_volumes), &e);
    if (!ws)
        return hip_fail(err, errlen, e, "scratch allocation");
    PendingGrid now;
    GridPrefilter& gp = now.gp;
    memset(&gp, 0, sizeof(gp));
    gp.in = (const char*)displacement->data;
    gp.out = (char*)ws;
    gp.dtype = displacement->dtype;
    gp.elem_size = dtype_size(displacement->dtype);
    gp.ndim = naxis + 1;
    gp.total = (int)total;
    gp.pole = -0.267949192431122706472553658494127633;      // order 3, SciPy's literal
    gp.gain = (1.0 - gp.pole) * (1.0 - 1.0 / gp.pole);
    int64_t stride = gp.elem_size;
    for (int k = naxis; k >= 0; --k) {
        gp.shape[k] = (int)displacement->shape[k];
        gp.stride_bytes[k] = displacement->stride_bytes[k];
        gp.pole_pow[k] = std::pow(gp.pole, (double)(gp.shape[k] - 1));
        g.disp_stride[k] = stride;
        stride *= gp.shape[k];
    }
    g.disp = (const char*)ws;
    now.stamp.raw = displacement->data;
    now.stamp.ws = ws;
    now.stamp.generation = workspace_generation(stream);
    now.stamp.dtype = displacement->dtype;
    now.stamp.ndim = naxis + 1;
    for (int k = 0; k <= naxis; ++k) {
        now.stamp.shape[k] = displacement->shape[k];
        now.stamp.stride[k] = displacement->stride_bytes[k];
    }
    GridStamp* stamp = grid_stamp(stream);
    if ((flags & EDHIP_FLAG_GRID_STAYS) && stamp->raw == now.stamp.raw && stamp->ws == now.stamp.ws &&
        stamp->generation == now.stamp.generation && stamp->dtype == now.stamp.dtype &&
        stamp->ndim == now.stamp.ndim && memcmp(stamp->shape, now.stamp.shape, sizeof(stamp->shape)) == 0 &&
        memcmp(stamp->stride, now.stamp.stride, sizeof(stamp->stride)) == 0)
        return EDHIP_OK;
    *stamp = GridStamp();
    if (defer) {
        *defer = now;
        return EDHIP_OK;
    }
    e = launch_grid_prefilter(gp, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "grid prefilter launch");
    *stamp = now.stamp;
    return EDHIP_OK;
}

// which kernels take one input/output pair of edhip_deform
enum Route { kRouteExact, kRouteFast, kRouteTile, kRouteLabel, kRouteInt };

Route pick_route(const ed::GridGeom& g, const ed::IOView& v, int in_dtype, int out_dtype, uint32_t flags,
                 int gradient)
{
    using namespace ed;
    if (flags & EDHIP_FLAG_EXACT)
        return kRouteExact;
    const bool floats = in_dtype == EDHIP_F32 || in_dtype == EDHIP_F64;
    if (((flags & EDHIP_FLAG_FAST) || (floats && out_dtype == in_dtype)) && deform_fast_supported(g, v, gradient))
        return deform_tile_supported(g, v, gradient != 0) ? kRouteTile : kRouteFast;
    // order-0 label maps of any dtype: bit-equal to the exact kernels, so AUTO takes it too
    if (!floats && deform_label_supported(g, v, gradient))
        return kRouteLabel;
    // 8- / 16-bit integer volumes, orders 1-5: bit-equal as well (near-tie voxels redone exactly)
    if (deform_int_supported(g, v, gradient))
        return kRouteInt;
    return kRouteExact;
}

// One input/output pair as the kernels see it: strides of the deformed axes, the non-deformed
// ("step") axes flattened (deform.c:399-436).
int make_view(const edhip_array& in, const edhip_array& out, int naxis, const int32_t* axis, int order,
              int mode, double cval, ed::IOView& v, char* err, size_t errlen)
{
    using namespace ed;
    memset(&v, 0, sizeof(v));
    v.in = (const char*)in.data;
    v.out = (char*)out.data;
    v.in_dtype = in.dtype;
    v.out_dtype = out.dtype;
    v.order = order;
    v.mode = mode;
    v.cval = cval;
    v.nsteps = 1;
    int64_t min_deform = INT64_MAX, min_step = INT64_MAX;
    for (int d = 0; d < in.ndim; ++d) {
        int k = -1;
        for (int j = 0; j < naxis; ++j)
            if (axis[j] == d)
                k = j;
        if (k >= 0) {
            v.in_stride[k] = in.stride_bytes[d];
            v.out_stride[k] = out.stride_bytes[d];
            if (out.shape[d] > 1 && iabs64(out.stride_bytes[d]) < min_deform)
                min_deform = iabs64(out.stride_bytes[d]);
        } else {
            if (in.shape[d] != out.shape[d])
                return fail(err, errlen, EDHIP_ERR_INVALID,
                            "non-deformed axes of input and output must have the same size");
            v.step_len[v.nstep] = in.shape[d];
            v.in_step_stride[v.nstep] = in.stride_bytes[d];
            v.out_step_stride[v.nstep] = out.stride_bytes[d];
            v.nsteps *= in.shape[d];
            if (out.shape[d] > 1 && iabs64(out.stride_bytes[d]) < min_step)
                min_step = iabs64(out.stride_bytes[d]);
            v.nstep++;
        }
    }
    v.steps_fastest = v.nstep > 0 && min_step < min_deform;
    return EDHIP_OK;
}

// descriptors of a batch that differ only in their base pointers, at a constant distance
bool uniform_batch(const edhip_array* a, int n, int64_t* stride)
{
    *stride = n > 1 ? (const char*)a[1].data - (const char*)a[0].data : 0;
    for (int b = 0; b < n; ++b) {
        if (a[b].dtype != a[0].dtype || a[b].ndim != a[0].ndim)
            return false;
        for (int d = 0; d < a[0].ndim; ++d)
            if (a[b].shape[d] != a[0].shape[d] || a[b].stride_bytes[d] != a[0].stride_bytes[d])
                return false;
        if ((const char*)a[b].data != (const char*)a[0].data + (int64_t)b * *stride)
            return false;
    }
    // the single-launch kernels address samples in elements: the distance must be a whole number of them
    const int64_t es = (a[0].dtype == EDHIP_F64 || a[0].dtype == EDHIP_I64 || a[0].dtype == EDHIP_U64) ? 8
                       : (a[0].dtype == EDHIP_F32 || a[0].dtype == EDHIP_I32 || a[0].dtype == EDHIP_U32) ? 4 : 1;
    if (*stride % es != 0)
        return false;
    return true;
}

}  // namespace

extern "C" {

#ifdef EDHIP_EXPERIMENTS
// marks a profiling build (make EXPERIMENTS=1): environment switches are live in it
int edhip_experiments_build = 1;
#endif

int edhip_version(void) { return EDHIP_VERSION; }

const char* edhip_status_string(int status)
{
    switch (status) {
    case EDHIP_OK: return "ok";
    case EDHIP_ERR_INVALID: return "invalid argument";
    case EDHIP_ERR_DTYPE: return "data type not supported";
    case EDHIP_ERR_MEMORY: return "out of memory";
    case EDHIP_ERR_DEVICE: return "HIP runtime error";
    case EDHIP_ERR_UNSUPPORTED: return "not supported by this build";
    default: return "unknown status";
    }
}

// the array's elements form one contiguous block (any axis order, no gaps, no overlap): its start and size
static bool dense_block(const edhip_array& a, char** ptr, long long* bytes)
{
    const long long esz = dtype_size(a.dtype);
    if (esz <= 0)
        return false;
    int order[EDHIP_MAX_DIMS], n = 0;
    long long total = esz;
    for (int d = 0; d < a.ndim; ++d) {
        if (a.shape[d] == 0) {
            *ptr = (char*)a.data;
            *bytes = 0;
            return true;
        }
        total *= a.shape[d];
        if (a.shape[d] > 1)
            order[n++] = d;
    }
    for (int i = 1; i < n; ++i)            // by ascending stride
        for (int j = i; j > 0 && a.stride_bytes[order[j]] < a.stride_bytes[order[j - 1]]; --j) {
            const int t = order[j];
            order[j] = order[j - 1];
            order[j - 1] = t;
        }
    long long expect = esz;
    for (int i = 0; i < n; ++i) {
        if (a.stride_bytes[order[i]] != expect)
            return false;
        expect *= a.shape[order[i]];
    }
    *ptr = (char*)a.data;
    *bytes = total;
    return true;
}

int edhip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return -1;
    return n;
}

int edhip_deform(int gradient, int ninputs, const edhip_array* inputs,
                 const edhip_array* displacement, const int64_t* output_offset,
                 const edhip_array* outputs, int naxis, const int32_t* axis, const int32_t* orders,
                 const int32_t* modes, const double* cvals, const double* affine, uint32_t flags,
                 void* hip_stream, char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    StreamGuard guard(stream);      // the stream's scratch is ours until every launch is enqueued
    if (err && errlen)
        err[0] = 0;
    if (int st = check_pairs(inputs, outputs, ninputs, naxis, axis, orders, modes, cvals, false, err, errlen))
        return st;
    if (int st = check_displacement(displacement, naxis, nullptr, err, errlen))
        return st;

    // EDHIP_FLAG_ZERO_GRADIENT: the dense blocks to clear (checked for every input before anything is enqueued)
    const bool zero = gradient && (flags & EDHIP_FLAG_ZERO_GRADIENT);
    char* zero_ptr[EDHIP_MAX_INPUTS];
    long long zero_bytes[EDHIP_MAX_INPUTS];
    if (zero) {
        for (int i = 0; i < ninputs; ++i)
            if (!dense_block(inputs[i], &zero_ptr[i], &zero_bytes[i]))
                return fail(err, errlen, EDHIP_ERR_INVALID, "EDHIP_FLAG_ZERO_GRADIENT needs dense gradient arrays");
    }
    // ---- shared geometry ------------------------------------------------------------------------
    GridGeom g;
    {
        int64_t in_len[kMaxAxes], out_len[kMaxAxes];
        deformed_lengths(inputs[0], outputs[0], naxis, axis, in_len, out_len);
        if (int st = fill_geometry(displacement, in_len, out_len, output_offset, naxis, affine, g, err, errlen))
            return st;
    }
    // Two facts about the call's progress, kept here and nowhere else:
    //   grid.gp.total > 0   the prefilter of a RAW_DISPLACEMENT grid is still to be enqueued.  The tables launch of the
    //                       tile / label / integer routes filters the grid itself where its LDS holds it; every other
    //                       launch gets the one-workgroup prefilter in front of it (grid_now).
    //   cleared[i]          the gradient block of input i has been cleared (ZERO_GRADIENT).  The spare workgroups of
    //                       grid_now clear block 0, those of the tile route's tables launch an aligned block i;
    //                       everything else is cleared by a memset in front of the scatter (clear_now).
    PendingGrid grid;
    memset(&grid.gp, 0, sizeof(grid.gp));
    bool cleared[EDHIP_MAX_INPUTS] = {};
    if (flags & EDHIP_FLAG_RAW_DISPLACEMENT) {
        bool f64_volumes = false;
        for (int i = 0; i < ninputs; ++i)
            f64_volumes = f64_volumes || inputs[i].dtype == EDHIP_F64;
        if (int st = stage_raw_grid(displacement, flags, stream, f64_volumes, g, &grid, err, errlen))
            return st;
    }
    auto grid_now = [&]() -> hipError_t {
        if (grid.gp.total <= 0)
            return hipSuccess;
        if (zero && zero_bytes[0] > 0 && !cleared[0] && ((uintptr_t)zero_ptr[0] & 15) == 0) {
            grid.gp.zero_ptr = zero_ptr[0];
            grid.gp.zero_bytes = zero_bytes[0];
            cleared[0] = true;
        }
        const hipError_t e = launch_grid_prefilter(grid.gp, stream);
        grid.gp.total = 0;
        if (e == hipSuccess)
            *grid_stamp(stream) = grid.stamp;
        return e;
    };
    auto clear_now = [&](int i) -> hipError_t {
        if (cleared[i])
            return hipSuccess;
        cleared[i] = true;
        return zero_bytes[i] > 0 ? hipMemsetAsync(zero_ptr[i], 0, (size_t)zero_bytes[i], stream) : hipSuccess;
    };
    if (g.nvox <= 0) {
        if (zero)
            for (int i = 0; i < ninputs; ++i)
                if (clear_now(i) != hipSuccess)
                    return fail(err, errlen, EDHIP_ERR_DEVICE, "clearing the gradient arrays failed");
        return EDHIP_OK;
    }

    // ---- one launch per input/output pair -----------------------------------------------------------
    for (int i = 0; i < ninputs; ++i) {
        const edhip_array& in = inputs[i];
        const edhip_array& out = outputs[i];
        IOView v;
        // float32 volume, 16-bit float on the output side (forward: narrowed at the store; gradient: dY widened at
        // the load), asked for with EDHIP_FLAG_FAST: the level-1 tile kernels take it, or nobody (EDHIP_ERR_UNSUPPORTED,
        // nothing launched; without the flag the exact kernels take the pair like any other).  The view pretends float32 with doubled output strides (IOView::out16).
        const int out16 = ((flags & EDHIP_FLAG_FAST) && !(flags & EDHIP_FLAG_EXACT) && in.dtype == EDHIP_F32)
                              ? (out.dtype == EDHIP_F16 ? 1 : (out.dtype == EDHIP_BF16 ? 2 : 0)) : 0;
        {
            edhip_array out32 = out;
            if (out16) {
                out32.dtype = EDHIP_F32;
                for (int d = 0; d < out.ndim; ++d)
                    out32.stride_bytes[d] = out.stride_bytes[d] * 2;
            }
            const int st = make_view(in, out16 ? out32 : out, naxis, axis + i * naxis, orders[i], modes[i], cvals[i], v,
                                     err, errlen);
            if (st != EDHIP_OK)
                return st;
            v.out16 = out16;
        }
        if (out16 && (v.nsteps <= 0 || ((uintptr_t)out.data & 3) || !deform_fast_supported(g, v, gradient) ||
                      !deform_tile_supported(g, v, gradient != 0)))
            return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "16-bit output next to a float32 volume: outside the tile kernels");
        if (v.nsteps <= 0) {
            if (zero && clear_now(i) != hipSuccess)
                return fail(err, errlen, EDHIP_ERR_DEVICE, "clearing the gradient arrays failed");
            continue;
        }

        const Route route = pick_route(g, v, in.dtype, out.dtype, flags, gradient);
        const bool tile = route == kRouteTile;
        DeformBatch db;
        db.nbatch = 1;
        db.in_bstride = db.out_bstride = db.disp_bstride = 0;
        if (tile) {
            // (several inputs share the geometry: the boxes are those of the last forward launch,
            // which is what a gradient call with the same inputs reads them for)
            db.box_mode = (!gradient && (flags & EDHIP_FLAG_KEEP_BOXES)) ? 1
                          : ((gradient && (flags & EDHIP_FLAG_USE_BOXES)) ? 2 : 0);
            db.disp_id = displacement->data;
            db.raw = (flags & EDHIP_FLAG_RAW_DISPLACEMENT) ? 1 : 0;
            db.strong = (flags & EDHIP_FLAG_STRONG_FIELD) ? 1 : 0;
        }
        // ---- in front of the launch: the grid filtered or handed to the tables launch, the block cleared or handed
        //      to it.  (The tables launch -- the label and integer routes run the tile path's -- filters a raw grid in
        //      LDS next to its plane slab: only where both fit.  A flat grid of 1342-1365 points would pass 64 KiB with
        //      the kernel's static LDS; such a grid gets the one-workgroup launch first.)
        if (route != kRouteExact && route != kRouteFast && grid.gp.total > 0 && !ed_env("EDHIP_GRIDPF_SEPARATE") &&
            8 * (3 * (size_t)g.ncp[1] * (size_t)g.ncp[2] + (size_t)grid.gp.total) <= 60 * 1024)
            db.gridpf = &grid.gp;
        hipError_t e = db.gridpf ? hipSuccess : grid_now();
        if (e != hipSuccess && tile)
            return fail(err, errlen, EDHIP_ERR_DEVICE, "grid prefilter launch");
        if (e == hipSuccess && zero && !cleared[i]) {
            // (the tile path clears a block inside its tables launch when its start is 16-byte aligned; a block it
            // cannot take is cleared HERE, in front of the scatter -- never behind a launch)
            if (tile && ((uintptr_t)zero_ptr[i] & 15) == 0) {
                db.zero_ptr = zero_ptr[i];
                db.zero_bytes = zero_bytes[i];
            } else {
                e = clear_now(i);
            }
        }
        // ---- the launch ---------------------------------------------------------------------------------------
        if (e != hipSuccess)
            ;
        else if (route == kRouteLabel || route == kRouteInt) {
            e = route == kRouteLabel ? launch_deform_label(g, v, stream, &db) : launch_deform_int(g, v, stream, &db);
            if (e == hipSuccess && db.gridpf && !db.gridpf_done)
                e = hipErrorUnknown;       // (cannot happen: every route of the label / integer paths starts with the tables launch)
        }
        else if (route == kRouteExact)
            e = launch_deform_exact(g, v, gradient != 0, stream);
        else if (tile)
            e = launch_deform_tile(g, v, gradient != 0, stream, &db);
        else
            e = launch_deform_fast(g, v, gradient != 0, stream);
        // ---- behind it: what the tables launch did on the way --------------------------------------------------
        if (db.gridpf_done) {
            grid.gp.total = 0;
            *grid_stamp(stream) = grid.stamp;
        }
        if (tile && e == hipErrorNotSupported) {
            (void)hipGetLastError();
            if (out16)
                return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "16-bit output next to a float32 volume: outside the level-1 tile kernels");
            // (a wide control grid the level-1 kernels declined -- batches, layouts: the row kernel takes the call, behind
            // a filtered grid and a cleared block.  A decline behind the tables launch has filtered the grid already;
            // the block is cleared here whether or not that launch did -- nothing has been added to it yet.)
            if (grid_now() != hipSuccess)
                return fail(err, errlen, EDHIP_ERR_DEVICE, "grid prefilter launch");
            if (zero && !cleared[i] && clear_now(i) != hipSuccess)
                return fail(err, errlen, EDHIP_ERR_DEVICE, "clearing the gradient arrays failed");
            e = launch_deform_fast(g, v, gradient != 0, stream);
        }
        if (db.zero_done)
            cleared[i] = true;
        else if (db.zero_ptr && (e == hipSuccess || e == hipErrorNotSupported)) {
            // (the tables launch -- which precedes every scatter of the tile path -- was not made, so nothing has
            // been added to the block yet)
            const hipError_t c2 = clear_now(i);
            if (e == hipSuccess)
                e = c2;
        }
        if (e != hipSuccess)
            return hip_fail(err, errlen, e, "deform kernel launch");
    }
    return EDHIP_OK;
}

int edhip_deform_batch(int gradient, int nbatch, const edhip_array* inputs,
                       const edhip_array* displacements, const int64_t* output_offset,
                       const edhip_array* outputs, int naxis, const int32_t* axis, int32_t order,
                       int32_t mode, double cval, const double* affine, uint32_t flags,
                       void* hip_stream, char* err, size_t errlen)
{
    if (err && errlen)
        err[0] = 0;
    if (nbatch < 0 || (nbatch > 0 && (!inputs || !displacements || !outputs)))
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid batch");
    if (nbatch == 0)
        return EDHIP_OK;          // nothing to do (and no descriptor to read)
    ed::StreamGuard guard((hipStream_t)hip_stream);
    if (gradient && (flags & EDHIP_FLAG_ZERO_GRADIENT)) {
        // batches: cleared up front, item by item (the single-launch path below shares one tables launch)
        for (int b = 0; b < nbatch; ++b) {
            char* zp = nullptr;
            long long zb = 0;
            if (!dense_block(inputs[b], &zp, &zb))
                return fail(err, errlen, EDHIP_ERR_INVALID, "EDHIP_FLAG_ZERO_GRADIENT needs dense gradient arrays");
            if (zb > 0 && hipMemsetAsync(zp, 0, (size_t)zb, (hipStream_t)hip_stream) != hipSuccess)
                return fail(err, errlen, EDHIP_ERR_DEVICE, "clearing the gradient arrays failed");
        }
        flags &= ~(uint32_t)EDHIP_FLAG_ZERO_GRADIENT;
    }
    // ---- one set of launches for the whole batch (the strip index of the tile kernels carries the
    //      sample): same-shaped float volumes at a constant distance, one prefiltered grid each ------
    {
        using namespace ed;
        DeformBatch db;
        db.nbatch = nbatch;
        db.box_mode = (!gradient && (flags & EDHIP_FLAG_KEEP_BOXES)) ? 1
                      : ((gradient && (flags & EDHIP_FLAG_USE_BOXES)) ? 2 : 0);
        db.disp_id = displacements[0].data;
        db.strong = (flags & EDHIP_FLAG_STRONG_FIELD) ? 1 : 0;
        const bool candidate = nbatch >= 2 && naxis == 3 && axis && !(flags & (EDHIP_FLAG_EXACT | EDHIP_FLAG_RAW_DISPLACEMENT)) &&
                               (inputs[0].dtype == EDHIP_F32 || inputs[0].dtype == EDHIP_F64) &&
                               outputs[0].dtype == inputs[0].dtype && inputs[0].ndim == outputs[0].ndim &&
                               inputs[0].ndim >= 3 && inputs[0].ndim <= EDHIP_MAX_DIMS &&
                               displacements[0].ndim == 4 && displacements[0].shape[0] == 3 &&
                               uniform_batch(inputs, nbatch, &db.in_bstride) &&
                               uniform_batch(outputs, nbatch, &db.out_bstride) &&
                               uniform_batch(displacements, nbatch, &db.disp_bstride);
        bool axes_ok = candidate && order >= 0 && order <= 5 && mode >= 0 && mode <= 4;
        for (int j = 0; axes_ok && j < naxis; ++j)
            axes_ok = axis[j] >= 0 && axis[j] < inputs[0].ndim && (j == 0 || axis[j] > axis[j - 1]);
        if (axes_ok) {
            hipStream_t stream = (hipStream_t)hip_stream;
            GridGeom g;
            int64_t in_len[kMaxAxes], out_len[kMaxAxes];
            bool shapes_ok = dtype_ok(displacements[0].dtype);
            deformed_lengths(inputs[0], outputs[0], naxis, axis, in_len, out_len);
            for (int k = 0; k < naxis; ++k)
                shapes_ok = shapes_ok && displacements[0].shape[k + 1] > 0 && in_len[k] >= 2;
            IOView v;
            if (shapes_ok &&
                fill_geometry(&displacements[0], in_len, out_len, output_offset, naxis, affine, g, nullptr, 0) == EDHIP_OK &&
                make_view(inputs[0], outputs[0], naxis, axis, order, mode, cval, v, nullptr, 0) == EDHIP_OK &&
                g.nvox > 0 && v.nsteps > 0 && deform_tile_supported(g, v, gradient != 0)) {
                const hipError_t e = launch_deform_tile(g, v, gradient != 0, stream, &db);
                if (e == hipSuccess)
                    return EDHIP_OK;
                if (e != hipErrorNotSupported)
                    return hip_fail(err, errlen, e, "deform kernel launch");
                (void)hipGetLastError();
            }
        }
    }
    // ---- otherwise: item by item (every shape, dtype and flag edhip_deform takes) ---------------------
    for (int b = 0; b < nbatch; ++b) {
        // stream order keeps item b + 1's control grid / tables (which reuse the workspace) behind
        // item b's kernels
        const int st = edhip_deform(gradient, 1, inputs + b, displacements + b, output_offset, outputs + b,
                                    naxis, axis, &order, &mode, &cval, affine, flags, hip_stream, err,
                                    errlen);
        if (st != EDHIP_OK)
            return st;
    }
    return EDHIP_OK;
}

int edhip_deform_batch_strided(int gradient, int nbatch, const edhip_array* input0,
                               int64_t input_batch_stride, const edhip_array* displacement0,
                               int64_t displacement_batch_stride, const int64_t* output_offset,
                               const edhip_array* output0, int64_t output_batch_stride, int naxis,
                               const int32_t* axis, int32_t order, int32_t mode, double cval,
                               const double* affine, uint32_t flags, void* hip_stream, char* err,
                               size_t errlen)
{
    if (err && errlen)
        err[0] = 0;
    if (nbatch < 0 || (nbatch > 0 && (!input0 || !displacement0 || !output0)))
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid batch");
    if (nbatch == 0)
        return EDHIP_OK;
    std::vector<edhip_array> all;
    try {
        all.resize(3 * (size_t)nbatch);
    } catch (...) {
        return fail(err, errlen, EDHIP_ERR_MEMORY, "out of host memory");
    }
    edhip_array* in = all.data();
    edhip_array* disp = in + nbatch;
    edhip_array* out = disp + nbatch;
    for (int b = 0; b < nbatch; ++b) {
        in[b] = sample(*input0, b, input_batch_stride);
        disp[b] = sample(*displacement0, b, displacement_batch_stride);
        out[b] = sample(*output0, b, output_batch_stride);
    }
    return edhip_deform_batch(gradient, nbatch, in, disp, output_offset, out, naxis, axis, order, mode, cval,
                              affine, flags, hip_stream, err, errlen);
}

int edhip_release_scratch(void)
{
    ed::workspace_release_all();
    return EDHIP_OK;
}

int edhip_profile_dominant(int enable)
{
    ed::tile_profile_enable(enable);
    return EDHIP_OK;
}

double edhip_profile_last_us(void) { return ed::tile_profile_last_us(); }

int edhip_source_box(const edhip_array* displacement, const int64_t* in_len, const int64_t* out_len,
                     const int64_t* output_offset, int naxis, const double* affine, uint32_t flags,
                     void* hip_stream, int64_t* box, char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    StreamGuard guard(stream);
    if (err && errlen)
        err[0] = 0;
    if (!in_len || !out_len || !box)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis list");
    if (int st = check_naxis(naxis, err, errlen))
        return st;
    if (int st = check_displacement(displacement, naxis, nullptr, err, errlen))
        return st;
    GridGeom g;
    if (int st = fill_geometry(displacement, in_len, out_len, output_offset, naxis, affine, g, err, errlen))
        return st;
    if (flags & EDHIP_FLAG_RAW_DISPLACEMENT)
        if (int st = stage_raw_grid(displacement, flags, stream, false, g, nullptr, err, errlen))
            return st;
    hipError_t e = hipSuccess;
    // the box lives in the last bytes of the workspace head (ed_workspace.h)
    char* ws = (char*)workspace_reserve(stream, deform_tile_workspace_bytes(g), &e);
    if (!ws)
        return hip_fail(err, errlen, e, "scratch allocation");
    int* dbox = (int*)(ws + kWorkspaceGridBytes - kWorkspaceBoxTail);
    e = launch_source_box(g, dbox, stream, (flags & EDHIP_FLAG_FAST) != 0);
    if (e == hipErrorNotSupported)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED,
                    "edhip_source_box: control grids are limited to 7680 values and 4 deformed axes");
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "source box launch");
    int hbox[2 * kMaxAxes];
    e = hipMemcpyAsync(hbox, dbox, sizeof(int) * 2 * naxis, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "source box read-back");
    for (int k = 0; k < 2 * naxis; ++k)
        box[k] = hbox[k];
    return EDHIP_OK;
}

// one filter pass; window: device-side window (only the whole-line tile kernels take one: EDHIP_ERR_UNSUPPORTED
// otherwise, nothing launched); dry: the checks of a windowed pass without its launch
static int filter1d_impl(const edhip_array* input, const edhip_array* output, int axis, int order,
                         int transpose, uint32_t flags, void* hip_stream, const int32_t* window, bool dry,
                         char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    StreamGuard guard(stream);
    if (err && errlen)
        err[0] = 0;
    if (!input || !output)
        return fail(err, errlen, EDHIP_ERR_INVALID, "missing array");
    if (order < 0 || order > 5)                                   // _deform_grid.c:71-74
        return fail(err, errlen, EDHIP_ERR_INVALID, "spline order not supported");
    if (input->ndim < 1 || input->ndim > EDHIP_MAX_DIMS || input->ndim != output->ndim)
        return fail(err, errlen, EDHIP_ERR_INVALID, "input and output dimensions should match");
    if (axis < 0)
        axis += input->ndim;                                      // _deform_grid.c:75-77
    if (axis < 0 || axis >= input->ndim)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis");
    if (!dtype_ok(input->dtype) || !dtype_ok(output->dtype))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    for (int d = 0; d < input->ndim; ++d)
        if (input->shape[d] != output->shape[d])
            return fail(err, errlen, EDHIP_ERR_INVALID, "input and output shapes should match");

    FilterParams p;
    memset(&p, 0, sizeof(p));
    p.in = (const char*)input->data;
    p.out = (char*)output->data;
    p.in_dtype = input->dtype;
    p.out_dtype = output->dtype;
    p.transpose = transpose != 0;
    p.len = input->shape[axis];
    p.in_axis_stride = input->stride_bytes[axis];
    p.out_axis_stride = output->stride_bytes[axis];
    p.nlines = 1;
    for (int d = 0; d < input->ndim; ++d) {
        if (d == axis)
            continue;
        p.outer_len[p.nouter] = input->shape[d];
        p.in_outer_stride[p.nouter] = input->stride_bytes[d];
        p.out_outer_stride[p.nouter] = output->stride_bytes[d];
        p.nlines *= input->shape[d];
        p.nouter++;
    }
    if (p.len <= 0 || p.nlines <= 0)
        return EDHIP_OK;

    // poles.  transpose: the sqrt() expressions of deform.c:1063-1084; forward: SciPy's correctly
    // rounded literals (they differ from the expressions by an ulp or so -- see oracle/ed_oracle.c)
    switch (order) {
    case 2:
        p.npoles = 1;
        p.pole[0] = p.transpose ? std::sqrt(8.0) - 3.0 : -0.171572875253809902396622551580603843;
        break;
    case 3:
        p.npoles = 1;
        p.pole[0] = p.transpose ? std::sqrt(3.0) - 2.0 : -0.267949192431122706472553658494127633;
        break;
    case 4:
        p.npoles = 2;
        if (p.transpose) {
            p.pole[0] = std::sqrt(664.0 - std::sqrt(438976.0)) + std::sqrt(304.0) - 19.0;
            p.pole[1] = std::sqrt(664.0 + std::sqrt(438976.0)) - std::sqrt(304.0) - 19.0;
        } else {
            p.pole[0] = -0.361341225900220177092212841325675255;
            p.pole[1] = -0.013725429297339121360331226939128204;
        }
        break;
    case 5:
        p.npoles = 2;
        if (p.transpose) {
            p.pole[0] = std::sqrt(67.5 - std::sqrt(4436.25)) + std::sqrt(26.25) - 6.5;
            p.pole[1] = std::sqrt(67.5 + std::sqrt(4436.25)) - std::sqrt(26.25) - 6.5;
        } else {
            p.pole[0] = -0.430575347099973791851434783493520110;
            p.pole[1] = -0.043096288203264653822712376822550182;
        }
        break;
    default: p.npoles = 0; break;
    }
    p.gain = 1.0;
    for (int h = 0; h < p.npoles; ++h) {
        p.gain *= (1.0 - p.pole[h]) * (1.0 - 1.0 / p.pole[h]);          // deform.c:1086-1088
        p.pole_pow[h] = std::pow(p.pole[h], (double)(p.len - 1));       // host libm, like the reference
        const int max = (int)std::ceil(std::log(1e-15) / std::log(std::fabs(p.pole[h])));
        p.trunc_branch[h] = max < p.len;                                // deform.c:1119,1134
    }

    // fast path for float32 / float64 unless the caller asks for the exact one; same operator, no
    // scratch, ~1e-16 relative to the sequential recursion (see spline_fast.hip)
    // (16-bit float storage on one side of a float32 pass: the whole-line tile kernels widen / narrow it on the way)
    const bool half_in = (input->dtype == EDHIP_F16 || input->dtype == EDHIP_BF16) && output->dtype == EDHIP_F32;
    const bool want_fast = !(flags & EDHIP_FLAG_EXACT) &&
                           (input->dtype == EDHIP_F32 || input->dtype == EDHIP_F64 || half_in);
    if (want_fast && p.npoles >= 1) {
        const hipError_t e = launch_spline_filter_fast(p, order, input->ndim, axis, input->shape,
                                                       input->stride_bytes, output->stride_bytes,
                                                       stream, window, dry);
        if (e == hipSuccess)
            return EDHIP_OK;
        if (e != hipErrorNotSupported)
            return hip_fail(err, errlen, e, "spline filter launch");
        (void)hipGetLastError();
    }
    if (window || dry)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "windowed prefilter: outside the whole-line tile kernels");
    // a float32 pass with 16-bit float storage on one side, asked for with EDHIP_FLAG_FAST: the tile kernels or nobody
    // (without the flag the exact kernel takes the pair like any other)
    const bool half_out = input->dtype == EDHIP_F32 && (output->dtype == EDHIP_F16 || output->dtype == EDHIP_BF16);
    if ((half_in || half_out) && (flags & EDHIP_FLAG_FAST) && !(flags & EDHIP_FLAG_EXACT))
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "16-bit storage next to a float32 pass: outside the whole-line tile kernels");

    const bool need_ws = p.npoles > 0 && p.len >= 2;
    if (need_ws) {
        // bound the fp64 scratch at 256 MiB; chunks of lines reuse it in stream order
        const int64_t budget = (int64_t)256 << 20;
        int64_t lines = budget / 8 / p.len;
        if (lines < 256)
            lines = 256;
        lines -= lines % 256;
        if (lines > p.nlines)
            lines = p.nlines;
        p.ws_lines = lines;
        hipError_t e = hipSuccess;
        void* ws = workspace_reserve(stream, kWorkspaceGridBytes + (size_t)lines * (size_t)p.len * 8, &e);
        if (!ws)
            return hip_fail(err, errlen, e, "scratch allocation");
        p.ws = (double*)((char*)ws + kWorkspaceGridBytes);
        e = launch_spline_filter(p, stream);
        if (e != hipSuccess)
            return hip_fail(err, errlen, e, "spline filter launch");
    } else {
        p.ws = nullptr;
        p.ws_lines = p.nlines;
        const hipError_t e = launch_spline_filter(p, stream);
        if (e != hipSuccess)
            return hip_fail(err, errlen, e, "spline filter launch");
    }
    return EDHIP_OK;
}

int edhip_spline_filter1d(const edhip_array* input, const edhip_array* output, int axis, int order,
                          int transpose, uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    return filter1d_impl(input, output, axis, order, transpose, flags, hip_stream, nullptr, false, err, errlen);
}

int edhip_spline_filter_axes_window(const edhip_array* input, const edhip_array* output, int naxes,
                                    const int32_t* axes, int order, int transpose, const int32_t* window,
                                    uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    if (err && errlen)
        err[0] = 0;
    if (naxes < 0 || (naxes > 0 && !axes) || !window)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis list / window");
    ed::StreamGuard guard((hipStream_t)hip_stream);
    // every pass must be one the tile kernels take, BEFORE the first one is launched
    for (int i = 0; i < naxes; ++i) {
        const int st = filter1d_impl(i == 0 ? input : output, output, axes[i], order, transpose, flags, hip_stream,
                                     window, true, err, errlen);
        if (st != EDHIP_OK)
            return st;
    }
    for (int i = 0; i < naxes; ++i) {
        const int st = filter1d_impl(i == 0 ? input : output, output, axes[i], order, transpose, flags, hip_stream,
                                     window, false, err, errlen);
        if (st != EDHIP_OK)
            return st;
    }
    return EDHIP_OK;
}

int edhip_source_window(const edhip_array* displacement, const int64_t* in_len, const int64_t* out_len,
                        const int64_t* output_offset, int naxis, const double* affine, int ndim,
                        const int64_t* shape, const int32_t* axis, int order, int mode, int margin, int align,
                        int minlen, uint32_t flags, void* hip_stream, int32_t* window, char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    StreamGuard guard(stream);
    if (err && errlen)
        err[0] = 0;
    if (!in_len || !out_len || !window || !shape || !axis || naxis < 1 || ndim < naxis || ndim > EDHIP_MAX_DIMS)
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis list");
    if (naxis > 4)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "edhip_source_window: up to 4 deformed axes");
    int64_t points = 0;
    if (int st = check_displacement(displacement, naxis, &points, err, errlen))
        return st;
    if (points > 7680)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "edhip_source_window: control grids are limited to 7680 values");
    SourceWindow sw{};
    sw.out = window;
    sw.ndim = ndim;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] <= 0 || shape[d] > 0x3fffffff)
            return fail(err, errlen, EDHIP_ERR_INVALID, "invalid shape");
        sw.shape[d] = (int)shape[d];
    }
    for (int k = 0; k < naxis; ++k) {
        if (axis[k] < 0 || axis[k] >= ndim || shape[axis[k]] != in_len[k])
            return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis list");
        sw.axis[k] = axis[k];
    }
    sw.order = order;
    sw.mode = mode;
    sw.margin = margin < 0 ? 0 : margin;
    sw.align = align < 1 ? 1 : align;
    sw.minlen = minlen < 1 ? 1 : minlen;
    GridGeom g;
    if (int st = fill_geometry(displacement, in_len, out_len, output_offset, naxis, affine, g, err, errlen))
        return st;
    if (flags & EDHIP_FLAG_RAW_DISPLACEMENT)
        if (int st = stage_raw_grid(displacement, flags, stream, false, g, nullptr, err, errlen))
            return st;
    hipError_t e = hipSuccess;
    char* ws = (char*)workspace_reserve(stream, deform_tile_workspace_bytes(g), &e);
    if (!ws)
        return hip_fail(err, errlen, e, "scratch allocation");
    int* dbox = (int*)(ws + kWorkspaceGridBytes - kWorkspaceBoxTail);
    e = launch_source_box(g, dbox, stream, true, &sw);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "source window launch");
    return EDHIP_OK;
}

int edhip_spline_filter_axes(const edhip_array* input, const edhip_array* output, int naxes,
                             const int32_t* axes, int order, int transpose, uint32_t flags,
                             void* hip_stream, char* err, size_t errlen)
{
    if (err && errlen)
        err[0] = 0;
    if (naxes < 0 || (naxes > 0 && !axes))
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis list");
    ed::StreamGuard guard((hipStream_t)hip_stream);
    const bool scratch_in = (flags & EDHIP_FLAG_SCRATCH_INPUT) && naxes > 1;
    if (naxes > 0 && input && output && input->dtype != output->dtype && (flags & EDHIP_FLAG_FAST) &&
        !(flags & EDHIP_FLAG_EXACT)) {
        // the one pass that converts (first of a widening chain, last of a narrowing one): can the tile kernels take
        // it?  Decided before anything is launched.
        const int i = (flags & EDHIP_FLAG_SCRATCH_INPUT) ? naxes - 1 : 0;
        const int st = filter1d_impl(input, output, axes[i], order, transpose, flags, hip_stream, nullptr, true, err, errlen);
        if (st != EDHIP_OK)
            return st;
    }
    for (int i = 0; i < naxes; ++i) {
        // the reference's loop (deform_grid.py:157-162, :279-284): input -> output, then in place;
        // EDHIP_FLAG_SCRATCH_INPUT: in place on the input, the last pass input -> output
        const edhip_array* src = scratch_in ? input : (i == 0 ? input : output);
        const edhip_array* dst = scratch_in ? (i == naxes - 1 ? output : input) : output;
        const int st = edhip_spline_filter1d(src, dst, axes[i], order, transpose, flags, hip_stream, err, errlen);
        if (st != EDHIP_OK)
            return st;
    }
    return EDHIP_OK;
}


// ---- gradient with respect to the control-point displacement and the inverse map (deform_dgrad.hip) ---------
// nbatch samples at constant byte distances (nbatch == 1: a single call); RAW_DISPLACEMENT batches arrive here
// one sample at a time.  ddisplacement / dinverse_affine: nullptr = not wanted (not both).
static int dgrad_impl(int ninputs, const edhip_array* inputs, const edhip_array* displacement,
                      const int64_t* output_offset, const edhip_array* doutputs, int naxis, const int32_t* axis,
                      const int32_t* orders, const int32_t* modes, const double* cvals, const double* affine,
                      const edhip_array* ddisplacement, const edhip_array* dinverse_affine, uint32_t flags,
                      hipStream_t stream, int nbatch, int64_t in_bstride, int64_t disp_bstride, int64_t dout_bstride,
                      int64_t ddisp_bstride, int64_t dinv_bstride, bool dry, char* err, size_t errlen)
{
    using namespace ed;
    // ---- the checks of edhip_deform, on floating-point volumes only ----------------------------------------------
    if (int st = check_pairs(inputs, doutputs, ninputs, naxis, axis, orders, modes, cvals, true, err, errlen))
        return st;
    int64_t points = 0;
    if (int st = check_displacement(displacement, naxis, &points, err, errlen))
        return st;
    if (!ddisplacement && !dinverse_affine)
        return fail(err, errlen, EDHIP_ERR_INVALID, "neither ddisplacement nor dinverse_affine is requested");
    if (int st = check_gradient_outputs(ddisplacement, displacement, dtype_ok, "data type not supported",
                                        dinverse_affine, naxis, err, errlen))
        return st;
    const bool raw = (flags & EDHIP_FLAG_RAW_DISPLACEMENT) != 0;
    if (raw && points > 4096)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "raw displacement grids are limited to 4096 points");
    IOView views[EDHIP_MAX_INPUTS];
    for (int i = 0; i < ninputs; ++i) {
        const int st = make_view(inputs[i], doutputs[i], naxis, axis + i * naxis, orders[i], modes[i], cvals[i],
                                 views[i], err, errlen);
        if (st != EDHIP_OK)
            return st;
    }
    int64_t in_len[kMaxAxes], out_len[kMaxAxes];
    deformed_lengths(inputs[0], doutputs[0], naxis, axis, in_len, out_len);
    GridGeom g;
    int st = fill_geometry(displacement, in_len, out_len, output_offset, naxis, affine, g, err, errlen);
    if (st != EDHIP_OK)
        return st;
    if (!dgrad_supported(g))
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED,
                    "displacement gradient: naxis * (control points along the last axis) is limited to %d",
                    kDgradMaxK);
    int64_t rows = 1;
    for (int k = 0; k < naxis - 1; ++k)
        rows *= out_len[k];
    if (nbatch > 65535 || rows > 0x7fffffff)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "displacement gradient: too many rows or samples");
    if (dry)
        return EDHIP_OK;

    // ---- scratch, reserved in one piece before anything is enqueued: [grid head | the transposed filter's line
    //      buffer | dense fp64 dD | partials] -- a later, larger request would move the buffer ----------------------
    const size_t grid_bytes = ((size_t)points * 8 + 255) & ~(size_t)255;
    size_t off = kWorkspaceGridBytes;
    const size_t dp_off = off + (raw ? grid_bytes : 0);
    const size_t sc_off = dp_off + (raw ? grid_bytes : 0);
    size_t need = sc_off + dgrad_scratch_bytes(g, nbatch, ddisplacement != nullptr, dinverse_affine != nullptr);
    if (raw && deform_tile_workspace_bytes(g, 1, false) > need)
        need = deform_tile_workspace_bytes(g, 1, false);
    hipError_t e = hipSuccess;
    char* ws = (char*)workspace_reserve(stream, need, &e);
    if (!ws)
        return hip_fail(err, errlen, e, "scratch allocation");
    if (raw) {
        // the library's order-3 mirror prefilter of the raw grid, into the workspace head (as edhip_deform does)
        st = stage_raw_grid(displacement, flags & ~(uint32_t)EDHIP_FLAG_GRID_STAYS, stream, false, g, nullptr, err,
                            errlen);
        if (st != EDHIP_OK)
            return st;
    }
    edhip_array dp;                   // dense fp64 dP of a RAW call, filtered in place below
    memset(&dp, 0, sizeof(dp));
    dp.data = ws + dp_off;
    dp.dtype = EDHIP_F64;
    dp.ndim = naxis + 1;
    for (int k = naxis, s = 8; k >= 0; --k) {
        dp.shape[k] = displacement->shape[k];
        dp.stride_bytes[k] = s;
        s *= (int)displacement->shape[k];
    }
    DgradCall c;
    memset(&c, 0, sizeof(c));
    c.g = g;
    c.ninputs = ninputs;
    c.views = views;
    c.nbatch = nbatch;
    c.in_bstride = in_bstride;
    c.out_bstride = dout_bstride;
    c.disp_bstride = disp_bstride;
    if (ddisplacement) {
        const edhip_array& dst = raw ? dp : *ddisplacement;
        c.dst = (char*)dst.data;
        c.dst_dtype = dst.dtype;
        c.dst_bstride = ddisp_bstride;
        for (int k = 0; k <= naxis; ++k)
            c.dst_stride[k] = dst.stride_bytes[k];
    }
    if (dinverse_affine) {
        c.dK = (char*)dinverse_affine->data;
        c.dK_stride[0] = dinverse_affine->stride_bytes[0];
        c.dK_stride[1] = dinverse_affine->stride_bytes[1];
        c.dK_bstride = dinv_bstride;
    }
    c.scratch = ws + sc_off;
    e = launch_deform_dgrad(c, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "displacement gradient launch");
    if (raw && ddisplacement) {
        // dD = (order-3 mirror prefilter)^T along the grid axes, in fp64, then one cast into the caller's array
        for (int k = 1; k <= naxis; ++k) {
            st = filter1d_impl(&dp, &dp, k, 3, 1, flags & EDHIP_FLAG_EXACT, stream, nullptr, false, err, errlen);
            if (st != EDHIP_OK)
                return st;
        }
        st = filter1d_impl(&dp, ddisplacement, 0, 0, 0, 0, stream, nullptr, false, err, errlen);
        if (st != EDHIP_OK)
            return st;
    }
    return EDHIP_OK;
}

// the two pairs of entry points: edhip_deform_displacement_gradient* = edhip_deform_transform_gradient* without
// the inverse map's result
static int transform_gradient_batch(int nbatch, const edhip_array* input0, int64_t input_batch_stride,
                                    const edhip_array* displacement0, int64_t displacement_batch_stride,
                                    const int64_t* output_offset, const edhip_array* doutput0,
                                    int64_t doutput_batch_stride, int naxis, const int32_t* axis, int32_t order,
                                    int32_t mode, double cval, const double* affine,
                                    const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                    const edhip_array* dinverse_affine0, int64_t dinverse_affine_batch_stride,
                                    uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (err && errlen)
        err[0] = 0;
    if (nbatch < 0 || (nbatch > 0 && (!input0 || !displacement0 || !doutput0)))
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid batch");
    if (!ddisplacement0 && !dinverse_affine0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "neither ddisplacement nor dinverse_affine is requested");
    if (nbatch == 0)
        return EDHIP_OK;
    ed::StreamGuard guard(stream);
    if (!(flags & EDHIP_FLAG_RAW_DISPLACEMENT))
        return dgrad_impl(1, input0, displacement0, output_offset, doutput0, naxis, axis, &order, &mode, &cval,
                          affine, ddisplacement0, dinverse_affine0, flags, stream, nbatch, input_batch_stride,
                          displacement_batch_stride, doutput_batch_stride, ddisplacement_batch_stride,
                          dinverse_affine_batch_stride, false, err, errlen);
    // raw grids: each sample's grid is prefiltered into the workspace head, so the samples go one after the other
    // (every argument is checked before the first launch)
    int st = dgrad_impl(1, input0, displacement0, output_offset, doutput0, naxis, axis, &order, &mode, &cval, affine,
                        ddisplacement0, dinverse_affine0, flags, stream, 1, 0, 0, 0, 0, 0, true, err, errlen);
    for (int b = 0; b < nbatch && st == EDHIP_OK; ++b) {
        const edhip_array in = sample(*input0, b, input_batch_stride);
        const edhip_array disp = sample(*displacement0, b, displacement_batch_stride);
        const edhip_array dout = sample(*doutput0, b, doutput_batch_stride);
        edhip_array ddisp, dinv;
        if (ddisplacement0)
            ddisp = sample(*ddisplacement0, b, ddisplacement_batch_stride);
        if (dinverse_affine0)
            dinv = sample(*dinverse_affine0, b, dinverse_affine_batch_stride);
        st = dgrad_impl(1, &in, &disp, output_offset, &dout, naxis, axis, &order, &mode, &cval, affine,
                        ddisplacement0 ? &ddisp : nullptr, dinverse_affine0 ? &dinv : nullptr, flags, stream, 1, 0, 0,
                        0, 0, 0, false, err, errlen);
    }
    return st;
}

int edhip_deform_transform_gradient(int ninputs, const edhip_array* inputs, const edhip_array* displacement,
                                    const int64_t* output_offset, const edhip_array* doutputs, int naxis,
                                    const int32_t* axis, const int32_t* orders, const int32_t* modes,
                                    const double* cvals, const double* affine, const edhip_array* ddisplacement,
                                    const edhip_array* dinverse_affine, uint32_t flags, void* hip_stream, char* err,
                                    size_t errlen)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    ed::StreamGuard guard(stream);
    if (err && errlen)
        err[0] = 0;
    return dgrad_impl(ninputs, inputs, displacement, output_offset, doutputs, naxis, axis, orders, modes, cvals,
                      affine, ddisplacement, dinverse_affine, flags, stream, 1, 0, 0, 0, 0, 0, false, err, errlen);
}

int edhip_deform_transform_gradient_batch_strided(
    int nbatch, const edhip_array* input0, int64_t input_batch_stride, const edhip_array* displacement0,
    int64_t displacement_batch_stride, const int64_t* output_offset, const edhip_array* doutput0,
    int64_t doutput_batch_stride, int naxis, const int32_t* axis, int32_t order, int32_t mode, double cval,
    const double* affine, const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
    const edhip_array* dinverse_affine0, int64_t dinverse_affine_batch_stride, uint32_t flags, void* hip_stream,
    char* err, size_t errlen)
{
    return transform_gradient_batch(nbatch, input0, input_batch_stride, displacement0, displacement_batch_stride,
                                    output_offset, doutput0, doutput_batch_stride, naxis, axis, order, mode, cval,
                                    affine, ddisplacement0, ddisplacement_batch_stride, dinverse_affine0,
                                    dinverse_affine_batch_stride, flags, hip_stream, err, errlen);
}

int edhip_deform_displacement_gradient(int ninputs, const edhip_array* inputs, const edhip_array* displacement,
                                       const int64_t* output_offset, const edhip_array* doutputs, int naxis,
                                       const int32_t* axis, const int32_t* orders, const int32_t* modes,
                                       const double* cvals, const double* affine, const edhip_array* ddisplacement,
                                       uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    if (err && errlen)
        err[0] = 0;
    if (!ddisplacement)
        return fail(err, errlen, EDHIP_ERR_INVALID, "ddisplacement must have the shape of displacement");
    return edhip_deform_transform_gradient(ninputs, inputs, displacement, output_offset, doutputs, naxis, axis, orders,
                                           modes, cvals, affine, ddisplacement, nullptr, flags, hip_stream, err,
                                           errlen);
}

int edhip_deform_displacement_gradient_batch_strided(
    int nbatch, const edhip_array* input0, int64_t input_batch_stride, const edhip_array* displacement0,
    int64_t displacement_batch_stride, const int64_t* output_offset, const edhip_array* doutput0,
    int64_t doutput_batch_stride, int naxis, const int32_t* axis, int32_t order, int32_t mode, double cval,
    const double* affine, const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride, uint32_t flags,
    void* hip_stream, char* err, size_t errlen)
{
    if (err && errlen)
        err[0] = 0;
    if (nbatch < 0 || (nbatch > 0 && !ddisplacement0))
        return fail(err, errlen, EDHIP_ERR_INVALID, "invalid batch");
    if (nbatch == 0)
        return EDHIP_OK;
    return transform_gradient_batch(nbatch, input0, input_batch_stride, displacement0, displacement_batch_stride,
                                    output_offset, doutput0, doutput_batch_stride, naxis, axis, order, mode, cval,
                                    affine, ddisplacement0, ddisplacement_batch_stride, nullptr, 0, flags, hip_stream,
                                    err, errlen);
}

// ---- the coordinate map at real positions and its inverse (deform_points.hip) ---------------------------------
int edhip_deform_points(int inverse, int nbatch, const edhip_array* points0, int64_t points_batch_stride,
                        const edhip_array* displacement0, int64_t displacement_batch_stride, const int64_t* in_len,
                        const int64_t* output_offset, int naxis, const double* affine, const double* forward_linear,
                        const edhip_array* result0, int64_t result_batch_stride, const edhip_array* jacobian0,
                        int64_t jacobian_batch_stride, const edhip_array* status0, int64_t status_batch_stride,
                        int max_iter, double tol, uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = check_batch_call(nbatch, points0 && displacement0 && result0 && in_len, err, errlen))
        return st;
    if (int st = check_naxis(naxis, err, errlen))
        return st;
    if (int st = check_prefiltered("edhip_deform_points", flags, err, errlen))
        return st;
    if (points0->ndim != 2 || points0->shape[1] != naxis || points0->shape[0] < 0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "points must have shape (N, naxis)");
    const int64_t npts = points0->shape[0];
    const int64_t rows[3] = {npts, naxis, naxis};            // (N, naxis) and (N, naxis, naxis)
    if (!has_shape(result0, 2, rows))
        return fail(err, errlen, EDHIP_ERR_INVALID, "result must have the shape of points");
    if (!f32_or_f64(points0) || !f32_or_f64(result0))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    if (jacobian0 && inverse)
        return fail(err, errlen, EDHIP_ERR_INVALID, "the jacobian belongs to the forward direction");
    if (int st = check_point_rows(jacobian0, "jacobian", 3, rows, true, err, errlen))
        return st;
    if (int st = check_status(status0, inverse != 0, npts, err, errlen))
        return st;
    if (inverse)
        if (int st = check_iteration(max_iter, tol, affine, forward_linear, err, errlen))
            return st;
    if (int st = check_displacement(displacement0, naxis, nullptr, err, errlen))
        return st;
    if (int st = check_batch_limit("edhip_deform_points", nbatch, err, errlen))
        return st;
    PointsCall c;
    memset(&c, 0, sizeof(c));
    if (int st = fill_geometry(displacement0, in_len, in_len, output_offset, naxis, affine, c.g, err, errlen))
        return st;
    if (nbatch == 0 || npts == 0)
        return EDHIP_OK;
    c.inverse = inverse != 0;
    c.nbatch = nbatch;
    c.npts = npts;
    c.disp_bstride = displacement_batch_stride;
    c.pts = batch_array(points0, points_batch_stride);
    c.res = batch_array(result0, result_batch_stride);
    c.jac = batch_array(jacobian0, jacobian_batch_stride);
    c.status = batch_array(status0, status_batch_stride);
    c.forward_linear = affine ? forward_linear : nullptr;
    c.max_iter = max_iter;
    c.tol = tol;
    const hipError_t e = launch_deform_points(c, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform points launch");
    return EDHIP_OK;
}

// ---- the adjoint of the coordinate map and of its inverse (deform_points_grad.hip) ---------------------------------
int edhip_deform_points_gradient(int inverse, int nbatch, const edhip_array* positions0,
                                 int64_t positions_batch_stride, const edhip_array* cotangent0,
                                 int64_t cotangent_batch_stride, const edhip_array* status0,
                                 int64_t status_batch_stride, const edhip_array* displacement0,
                                 int64_t displacement_batch_stride, const int64_t* in_len,
                                 const int64_t* output_offset, int naxis, const double* affine,
                                 const edhip_array* dpoints0, int64_t dpoints_batch_stride,
                                 const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                 const edhip_array* dinverse_affine0, int64_t dinverse_affine_batch_stride,
                                 uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = check_batch_call(nbatch, positions0 && cotangent0 && displacement0 && in_len, err, errlen))
        return st;
    if (int st = check_naxis(naxis, err, errlen))
        return st;
    if (int st = check_prefiltered("edhip_deform_points_gradient", flags, err, errlen))
        return st;
    if (!dpoints0 && !ddisplacement0 && !dinverse_affine0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "none of dpoints, ddisplacement and dinverse_affine is requested");
    if (positions0->ndim != 2 || positions0->shape[1] != naxis || positions0->shape[0] < 0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "positions must have shape (N, naxis)");
    const int64_t npts = positions0->shape[0];
    const int64_t rows[2] = {npts, naxis};
    if (!has_shape(cotangent0, 2, rows))
        return fail(err, errlen, EDHIP_ERR_INVALID, "cotangent must have the shape of positions");
    if (!f32_or_f64(positions0) || !f32_or_f64(cotangent0))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    if (int st = check_status(status0, inverse != 0, npts, err, errlen))
        return st;
    if (int st = check_displacement(displacement0, naxis, nullptr, err, errlen))
        return st;
    if (dpoints0) {
        if (!has_shape(dpoints0, 2, rows))
            return fail(err, errlen, EDHIP_ERR_INVALID, "dpoints must have the shape of positions");
        if (!f32_or_f64(dpoints0))
            return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    }
    if (int st = check_gradient_outputs(ddisplacement0, displacement0, floating_dtype, kFloatingDdisp,
                                        dinverse_affine0, naxis, err, errlen))
        return st;
    if (int st = check_batch_limit("edhip_deform_points_gradient", nbatch, err, errlen))
        return st;
    PointsGradCall c;
    memset(&c, 0, sizeof(c));
    if (int st = fill_geometry(displacement0, in_len, in_len, output_offset, naxis, affine, c.g, err, errlen))
        return st;
    if (nbatch == 0 || (npts == 0 && !ddisplacement0 && !dinverse_affine0))
        return EDHIP_OK;
    c.inverse = inverse != 0;
    c.nbatch = nbatch;
    c.npts = npts;
    c.disp_bstride = displacement_batch_stride;
    c.pos = batch_array(positions0, positions_batch_stride);
    c.cot = batch_array(cotangent0, cotangent_batch_stride);
    c.status = batch_array(status0, status_batch_stride);
    c.dpts = batch_array(dpoints0, dpoints_batch_stride);
    c.ddisp = batch_array(ddisplacement0, ddisplacement_batch_stride);
    c.dK = batch_array(dinverse_affine0, dinverse_affine_batch_stride);
    // heads, cells and the per-point u rows
    return launch_with_scratch(c, points_grad_scratch_bytes(c.g, nbatch, npts), launch_deform_points_gradient,
                               "deform points gradient launch", stream, err, errlen);
}

// ---- r, J = dr/dq and H = d^2r/dq dq at real positions, and their adjoint (deform_points_jet.hip) -------------------
namespace {

int check_axes_jet(const char* entry, int naxis, char* err, size_t errlen)
{
    if (int st = check_naxis(naxis, err, errlen))
        return st;
    if (naxis > 3)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "%s takes 1 to 3 deformed axes", entry);
    return EDHIP_OK;
}

}  // namespace

int edhip_deform_points_derivatives(int nbatch, const edhip_array* points0, int64_t points_batch_stride,
                                    const edhip_array* displacement0, int64_t displacement_batch_stride,
                                    const int64_t* in_len, const int64_t* output_offset, int naxis,
                                    const double* affine, const edhip_array* result0, int64_t result_batch_stride,
                                    const edhip_array* jacobian0, int64_t jacobian_batch_stride,
                                    const edhip_array* hessian0, int64_t hessian_batch_stride, uint32_t flags,
                                    void* hip_stream, char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = check_batch_call(nbatch, points0 && displacement0 && result0 && in_len, err, errlen))
        return st;
    if (int st = check_axes_jet("edhip_deform_points_derivatives", naxis, err, errlen))
        return st;
    if (int st = check_prefiltered("edhip_deform_points_derivatives", flags, err, errlen))
        return st;
    if (points0->ndim != 2 || points0->shape[1] != naxis || points0->shape[0] < 0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "points must have shape (N, naxis)");
    const int64_t npts = points0->shape[0];
    const int64_t rows[4] = {npts, naxis, naxis, naxis};
    if (!has_shape(result0, 2, rows))
        return fail(err, errlen, EDHIP_ERR_INVALID, "result must have the shape of points");
    if (!f32_or_f64(points0) || !f32_or_f64(result0))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    if (int st = check_point_rows(jacobian0, "jacobian", 3, rows, true, err, errlen))
        return st;
    if (int st = check_point_rows(hessian0, "hessian", 4, rows, true, err, errlen))
        return st;
    if (int st = check_displacement(displacement0, naxis, nullptr, err, errlen))
        return st;
    if (int st = check_batch_limit("edhip_deform_points_derivatives", nbatch, err, errlen))
        return st;
    PointsJetCall c;
    memset(&c, 0, sizeof(c));
    if (int st = fill_geometry(displacement0, in_len, in_len, output_offset, naxis, affine, c.g, err, errlen))
        return st;
    if (nbatch == 0 || npts == 0)
        return EDHIP_OK;
    c.nbatch = nbatch;
    c.npts = npts;
    c.disp_bstride = displacement_batch_stride;
    c.pts = batch_array(points0, points_batch_stride);
    c.res = batch_array(result0, result_batch_stride);
    c.jac = batch_array(jacobian0, jacobian_batch_stride);
    c.hess = batch_array(hessian0, hessian_batch_stride);
    const hipError_t e = launch_deform_points_derivatives(c, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform points derivatives launch");
    return EDHIP_OK;
}

int edhip_deform_points_derivatives_gradient(int nbatch, const edhip_array* positions0, int64_t positions_batch_stride,
                                             const edhip_array* dresult0, int64_t dresult_batch_stride,
                                             const edhip_array* djacobian0, int64_t djacobian_batch_stride,
                                             const edhip_array* dhessian0, int64_t dhessian_batch_stride,
                                             const edhip_array* displacement0, int64_t displacement_batch_stride,
                                             const int64_t* in_len, const int64_t* output_offset, int naxis,
                                             const double* affine, const edhip_array* dpoints0,
                                             int64_t dpoints_batch_stride, const edhip_array* ddisplacement0,
                                             int64_t ddisplacement_batch_stride, const edhip_array* dinverse_affine0,
                                             int64_t dinverse_affine_batch_stride, uint32_t flags, void* hip_stream,
                                             char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = check_batch_call(nbatch, positions0 && displacement0 && in_len, err, errlen))
        return st;
    if (int st = check_axes_jet("edhip_deform_points_derivatives_gradient", naxis, err, errlen))
        return st;
    if (int st = check_prefiltered("edhip_deform_points_derivatives_gradient", flags, err, errlen))
        return st;
    if (!dresult0 && !djacobian0 && !dhessian0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "none of dresult, djacobian and dhessian is given");
    if (!dpoints0 && !ddisplacement0 && !dinverse_affine0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "none of dpoints, ddisplacement and dinverse_affine is requested");
    if (positions0->ndim != 2 || positions0->shape[1] != naxis || positions0->shape[0] < 0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "positions must have shape (N, naxis)");
    const int64_t npts = positions0->shape[0];
    const int64_t rows[4] = {npts, naxis, naxis, naxis};
    if (!f32_or_f64(positions0))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    if (int st = check_point_rows(dresult0, "dresult", 2, rows, false, err, errlen))
        return st;
    if (int st = check_point_rows(djacobian0, "djacobian", 3, rows, false, err, errlen))
        return st;
    if (int st = check_point_rows(dhessian0, "dhessian", 4, rows, false, err, errlen))
        return st;
    if (int st = check_displacement(displacement0, naxis, nullptr, err, errlen))
        return st;
    if (int st = check_point_rows(dpoints0, "dpoints", 2, rows, false, err, errlen))
        return st;
    if (int st = check_gradient_outputs(ddisplacement0, displacement0, floating_dtype, kFloatingDdisp,
                                        dinverse_affine0, naxis, err, errlen))
        return st;
    if (int st = check_batch_limit("edhip_deform_points_derivatives_gradient", nbatch, err, errlen))
        return st;
    PointsJetGradCall c;
    memset(&c, 0, sizeof(c));
    if (int st = fill_geometry(displacement0, in_len, in_len, output_offset, naxis, affine, c.g, err, errlen))
        return st;
    if (nbatch == 0 || (npts == 0 && !ddisplacement0 && !dinverse_affine0))
        return EDHIP_OK;
    c.nbatch = nbatch;
    c.npts = npts;
    c.disp_bstride = displacement_batch_stride;
    c.pos = batch_array(positions0, positions_batch_stride);
    c.du = batch_array(dresult0, dresult_batch_stride);
    c.dA = batch_array(djacobian0, djacobian_batch_stride);
    c.dG = batch_array(dhessian0, dhessian_batch_stride);
    c.dpts = batch_array(dpoints0, dpoints_batch_stride);
    c.ddisp = batch_array(ddisplacement0, ddisplacement_batch_stride);
    c.dK = batch_array(dinverse_affine0, dinverse_affine_batch_stride);
    // heads and cells
    return launch_with_scratch(c, points_jet_scratch_bytes(c.g, nbatch), launch_deform_points_derivatives_gradient,
                               "deform points derivatives gradient launch", stream, err, errlen);
}

// ---- label-aware linear resampling of label maps (deform_vote.hip) --------------------------------------------
int edhip_deform_labels(int nbatch, const edhip_array* input0, int64_t input_batch_stride,
                        const edhip_array* displacement0, int64_t displacement_batch_stride,
                        const int64_t* output_offset, const edhip_array* output0, int64_t output_batch_stride,
                        const edhip_array* weight0, int64_t weight_batch_stride, int naxis, const int32_t* axis,
                        int32_t mode, double cval, const double* affine, uint32_t flags, void* hip_stream, char* err,
                        size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = check_batch_call(nbatch, input0 && displacement0 && output0, err, errlen))
        return st;
    if (int st = check_axes_1_to_3("edhip_deform_labels", axis, naxis, err, errlen))
        return st;
    if (int st = check_prefiltered("edhip_deform_labels", flags, err, errlen))
        return st;
    const edhip_array& in = *input0;
    const edhip_array& out = *output0;
    if (in.ndim != out.ndim)
        return fail(err, errlen, EDHIP_ERR_INVALID, "input and output dimensions should match");
    if (in.ndim < 1 || in.ndim > EDHIP_MAX_DIMS)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "arrays must have 1..%d dimensions", EDHIP_MAX_DIMS);
    if (in.dtype != out.dtype || in.dtype < EDHIP_BOOL || in.dtype > EDHIP_I64)
        return fail(err, errlen, EDHIP_ERR_INVALID,
                    "label maps must be integer or bool arrays, input and output of one dtype");
    for (int j = 0; j < naxis; ++j)
        if (axis[j] < 0 || axis[j] >= in.ndim || (j > 0 && axis[j] <= axis[j - 1]))
            return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis in axis list");
    if (mode < 0 || mode > 4)
        return fail(err, errlen, EDHIP_ERR_INVALID, "boundary mode not supported");
    if (int st = check_displacement(displacement0, naxis, nullptr, err, errlen))
        return st;
    if (weight0) {
        if (!has_shape(weight0, out.ndim, out.shape))
            return fail(err, errlen, EDHIP_ERR_INVALID, "weight must have the shape of the output");
        if (weight0->dtype != EDHIP_F32)
            return fail(err, errlen, EDHIP_ERR_DTYPE, "weight must be float32");
    }
    // cval as an element of the map's dtype: an integer value inside its range
    uint64_t cval_bits = 0;
    {
        double lo = 0.0, hi = 1.0;           // bool; hi is the largest value for the narrow types, 2^63 / 2^64 (excluded) for the wide ones
        bool hi_excluded = false;
        switch (in.dtype) {
        case EDHIP_U8: hi = 255.0; break;
        case EDHIP_I8: lo = -128.0; hi = 127.0; break;
        case EDHIP_U16: hi = 65535.0; break;
        case EDHIP_I16: lo = -32768.0; hi = 32767.0; break;
        case EDHIP_U32: hi = 4294967295.0; break;
        case EDHIP_I32: lo = -2147483648.0; hi = 2147483647.0; break;
        case EDHIP_U64: hi = 18446744073709551616.0; hi_excluded = true; break;
        case EDHIP_I64: lo = -9223372036854775808.0; hi = 9223372036854775808.0; hi_excluded = true; break;
        default: break;
        }
        if (!(cval >= lo) || !(hi_excluded ? cval < hi : cval <= hi) || cval != std::floor(cval))
            return fail(err, errlen, EDHIP_ERR_INVALID, "cval must be an integer value of the label map's dtype");
        cval_bits = lo < 0.0 ? (uint64_t)(int64_t)cval : (uint64_t)cval;
    }
    if (int st = check_batch_limit("edhip_deform_labels", nbatch, err, errlen))
        return st;
    LabelsCall c;
    memset(&c, 0, sizeof(c));
    {
        int64_t in_len[kMaxAxes], out_len[kMaxAxes];
        deformed_lengths(in, out, naxis, axis, in_len, out_len);
        if (int st = fill_geometry(displacement0, in_len, out_len, output_offset, naxis, affine, c.g, err, errlen))
            return st;
    }
    int st = make_view(in, out, naxis, axis, 1, mode, cval, c.v, err, errlen);
    if (st != EDHIP_OK)
        return st;
    if (weight0) {
        IOView wv;                            // the weight's strides, sorted like the output's
        st = make_view(in, *weight0, naxis, axis, 1, mode, cval, wv, err, errlen);
        if (st != EDHIP_OK)
            return st;
        c.weight = (char*)weight0->data;
        for (int k = 0; k < naxis; ++k)
            c.weight_stride[k] = wv.out_stride[k];
        for (int l = 0; l < wv.nstep; ++l)
            c.weight_step_stride[l] = wv.out_step_stride[l];
        c.weight_bstride = weight_batch_stride;
    }
    if (nbatch == 0 || c.g.nvox <= 0 || c.v.nsteps <= 0)
        return EDHIP_OK;
    c.nbatch = nbatch;
    c.in_bstride = input_batch_stride;
    c.out_bstride = output_batch_stride;
    c.disp_bstride = displacement_batch_stride;
    c.cval_bits = cval_bits;
    const hipError_t e = launch_deform_labels(c, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform labels launch");
    return EDHIP_OK;
}

// ---- an image carried back through the deformation (deform_unwarp.hip) and its adjoint (deform_unwarp_grad.hip) --
// What edhip_deform_inverse and edhip_deform_inverse_gradient check and fill alike.  sampled0: the array of deformed
// extents O (Y, or the accumulator dY); lattice0: the one of deformed extents in_len (Z, or the cotangent dZ), called
// `lattice_name` in the messages; valid0: the forward's (nullptr otherwise).  float_only: float32 / float64 arrays
// (the gradient); otherwise every dtype but the 16-bit floats.  *launch: there is something to launch.
static int fill_inverse_call(const char* entry, int nbatch, const edhip_array* sampled0, int64_t sampled_batch_stride,
                      const edhip_array* displacement0, int64_t displacement_batch_stride, const int64_t* in_len,
                      const int64_t* output_offset, const edhip_array* lattice0, const char* lattice_name,
                      int64_t lattice_batch_stride, const edhip_array* valid0, int64_t valid_batch_stride, int naxis,
                      const int32_t* axis, int32_t order, int32_t mode, double cval, const double* affine,
                      const double* forward_linear, int max_iter, double tol, uint32_t flags, bool float_only,
                      ed::InverseCall& c, bool* launch, char* err, size_t errlen)
{
    using namespace ed;
    *launch = false;
    if (int st = check_batch_call(nbatch, sampled0 && displacement0 && lattice0 && in_len, err, errlen))
        return st;
    if (int st = check_axes_1_to_3(entry, axis, naxis, err, errlen))
        return st;
    if (int st = check_prefiltered(entry, flags, err, errlen))
        return st;
    const edhip_array& in = *sampled0;
    const edhip_array& out = *lattice0;
    if (int st = check_pairs(sampled0, lattice0, 1, naxis, axis, &order, &mode, &cval, false, err, errlen))
        return st;
    for (int j = 1; j < naxis; ++j)
        if (axis[j] <= axis[j - 1])
            return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis in axis list");
    if (in.dtype != out.dtype)
        return fail(err, errlen, EDHIP_ERR_DTYPE, "input and output must have one dtype");
    if (float_only ? !f32_or_f64(&in) : (in.dtype == EDHIP_F16 || in.dtype == EDHIP_BF16))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    int64_t sampled_len[kMaxAxes];
    for (int k = 0; k < naxis; ++k) {
        sampled_len[k] = in.shape[axis[k]];
        if (out.shape[axis[k]] != in_len[k])
            return fail(err, errlen, EDHIP_ERR_INVALID, "the %s's deformed axes must have the extents in_len",
                        lattice_name);
        if (sampled_len[k] < 2)
            return fail(err, errlen, EDHIP_ERR_INVALID, "deformed axes must have at least 2 elements");
    }
    if (valid0) {
        if (!has_shape(valid0, naxis, in_len))
            return fail(err, errlen, EDHIP_ERR_INVALID, "valid must have the output's deformed shape");
        if (valid0->dtype != EDHIP_U8)
            return fail(err, errlen, EDHIP_ERR_DTYPE, "valid must be uint8");
    }
    if (int st = check_iteration(max_iter, tol, affine, forward_linear, err, errlen))
        return st;
    if (int st = check_displacement(displacement0, naxis, nullptr, err, errlen))
        return st;
    if (int st = check_batch_limit(entry, nbatch, err, errlen))
        return st;
    memset(&c, 0, sizeof(c));
    // the solve's geometry is the forward call's (extents in_len); the sampled array has its own extents
    if (int st = fill_geometry(displacement0, in_len, sampled_len, output_offset, naxis, affine, c.g, err, errlen))
        return st;
    if (int st = make_view(in, out, naxis, axis, order, mode, cval, c.v, err, errlen))
        return st;
    if (nbatch == 0 || c.v.nsteps <= 0)
        return EDHIP_OK;
    c.nbatch = nbatch;
    c.in_bstride = sampled_batch_stride;
    c.out_bstride = lattice_batch_stride;
    c.disp_bstride = displacement_batch_stride;
    c.valid = batch_array(valid0, valid_batch_stride);
    c.forward_linear = affine ? forward_linear : nullptr;
    c.max_iter = max_iter;
    c.tol = tol;
    *launch = true;
    return EDHIP_OK;
}

int edhip_deform_inverse(int nbatch, const edhip_array* input0, int64_t input_batch_stride,
                         const edhip_array* displacement0, int64_t displacement_batch_stride, const int64_t* in_len,
                         const int64_t* output_offset, const edhip_array* output0, int64_t output_batch_stride,
                         const edhip_array* valid0, int64_t valid_batch_stride, int naxis, const int32_t* axis,
                         int32_t order, int32_t mode, double cval, const double* affine, const double* forward_linear,
                         int max_iter, double tol, uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    ed::InverseCall c;
    bool launch;
    if (int st = fill_inverse_call("edhip_deform_inverse", nbatch, input0, input_batch_stride, displacement0,
                                   displacement_batch_stride, in_len, output_offset, output0, "output",
                                   output_batch_stride, valid0, valid_batch_stride, naxis, axis, order, mode, cval,
                                   affine, forward_linear, max_iter, tol, flags, false, c, &launch, err, errlen))
        return st;
    if (!launch)
        return EDHIP_OK;
    const hipError_t e = ed::launch_deform_inverse(c, (hipStream_t)hip_stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform inverse launch");
    return EDHIP_OK;
}

int edhip_deform_inverse_gradient(int nbatch, const edhip_array* cotangent0, int64_t cotangent_batch_stride,
                                  const edhip_array* displacement0, int64_t displacement_batch_stride,
                                  const int64_t* in_len, const int64_t* output_offset, const edhip_array* dinput0,
                                  int64_t dinput_batch_stride, int naxis, const int32_t* axis, int32_t order,
                                  int32_t mode, const double* affine, const double* forward_linear, int max_iter,
                                  double tol, uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    ed::InverseCall c;
    bool launch;
    if (int st = fill_inverse_call("edhip_deform_inverse_gradient", nbatch, dinput0, dinput_batch_stride,
                                   displacement0, displacement_batch_stride, in_len, output_offset, cotangent0,
                                   "cotangent", cotangent_batch_stride, nullptr, 0, naxis, axis, order, mode, 0.0,
                                   affine, forward_linear, max_iter, tol, flags, true, c, &launch, err, errlen))
        return st;
    if (!launch)
        return EDHIP_OK;
    const hipError_t e = ed::launch_deform_inverse_gradient(c, (hipStream_t)hip_stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform inverse gradient launch");
    return EDHIP_OK;
}

int edhip_deform_inverse_transform_gradient(int nbatch, const edhip_array* input0, int64_t input_batch_stride,
                                            const edhip_array* cotangent0, int64_t cotangent_batch_stride,
                                            const edhip_array* displacement0, int64_t displacement_batch_stride,
                                            const int64_t* in_len, const int64_t* output_offset,
                                            const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                            const edhip_array* dinverse_affine0, int64_t dinverse_affine_batch_stride,
                                            int naxis, const int32_t* axis, int32_t order, int32_t mode,
                                            const double* affine, const double* forward_linear, int max_iter,
                                            double tol, uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    InverseCall c;
    bool launch;
    if (int st = fill_inverse_call("edhip_deform_inverse_transform_gradient", nbatch, input0, input_batch_stride,
                                   displacement0, displacement_batch_stride, in_len, output_offset, cotangent0,
                                   "cotangent", cotangent_batch_stride, nullptr, 0, naxis, axis, order, mode, 0.0,
                                   affine, forward_linear, max_iter, tol, flags, true, c, &launch, err, errlen))
        return st;
    if (!ddisplacement0 && !dinverse_affine0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "neither ddisplacement nor dinverse_affine is requested");
    if (int st = check_gradient_outputs(ddisplacement0, displacement0, floating_dtype, kFloatingDdisp,
                                        dinverse_affine0, naxis, err, errlen))
        return st;
    if (!launch)
        return EDHIP_OK;
    // heads, cells and the per-voxel u and q rows: the stream's workspace, behind its grid head
    StreamGuard guard(stream);
    hipError_t e = hipSuccess;
    char* ws = (char*)workspace_reserve(stream, kWorkspaceGridBytes + inverse_tgrad_scratch_bytes(c.g, nbatch), &e);
    if (!ws)
        return hip_fail(err, errlen, e, "scratch allocation");
    e = launch_deform_inverse_transform_gradient(c, batch_array(ddisplacement0, ddisplacement_batch_stride),
                                                 batch_array(dinverse_affine0, dinverse_affine_batch_stride),
                                                 ws + kWorkspaceGridBytes, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform inverse transform gradient launch");
    return EDHIP_OK;
}

// ---- the deformed image at real output positions (deform_sample.hip) and its gradients (deform_sample_grad.hip) -----
// One X-shaped array `x` and one point-indexed array `p` (x's non-deformed axes, one axis of N points in the place of
// the first deformed axis) as the kernels see them: v.in / in_* from x, v.out / out_* from p, out_stride[0] per point.
static void make_sample_view(const edhip_array& x, const edhip_array& p, int naxis, const int32_t* axis, int order,
                             int mode, double cval, ed::IOView& v)
{
    memset(&v, 0, sizeof(v));
    v.in = (const char*)x.data;
    v.out = (char*)p.data;
    v.in_dtype = x.dtype;
    v.out_dtype = p.dtype;
    v.order = order;
    v.mode = mode;
    v.cval = cval;
    v.nsteps = 1;
    v.out_stride[0] = p.stride_bytes[axis[0]];
    for (int d = 0; d < x.ndim; ++d) {
        int k = -1;
        for (int j = 0; j < naxis; ++j)
            if (axis[j] == d)
                k = j;
        if (k >= 0) {
            v.in_stride[k] = x.stride_bytes[d];
        } else {
            v.step_len[v.nstep] = x.shape[d];
            v.in_step_stride[v.nstep] = x.stride_bytes[d];
            v.out_step_stride[v.nstep] = p.stride_bytes[v.nstep + (d > axis[0] ? 1 : 0)];
            v.nsteps *= x.shape[d];
            v.nstep++;
        }
    }
}

// What edhip_deform_sample and edhip_deform_sample_gradient check and fill alike.  x0: the array of X's shape the
// geometry is read from, called `x_name`; lattice0: output0 or cotangent0, called `lattice_name`.  float_only: float32 /
// float64 arrays (the gradient); otherwise every dtype but the 16-bit floats.
static int fill_sample_call(const char* entry, int nbatch, const edhip_array* x0, const char* x_name,
                            const edhip_array* points0, int64_t points_batch_stride, const edhip_array* displacement0,
                            int64_t displacement_batch_stride, const int64_t* in_len, const int64_t* output_offset,
                            const edhip_array* lattice0, const char* lattice_name, int64_t lattice_batch_stride,
                            int naxis, const int32_t* axis, int32_t order, int32_t mode, double cval,
                            const double* affine, uint32_t flags, bool float_only, ed::SampleCall& c, char* err,
                            size_t errlen)
{
    using namespace ed;
    if (int st = check_batch_call(nbatch, x0 && points0 && displacement0 && lattice0 && in_len, err, errlen))
        return st;
    if (int st = check_axes_1_to_3(entry, axis, naxis, err, errlen))
        return st;
    if (int st = check_prefiltered(entry, flags, err, errlen))
        return st;
    const edhip_array& x = *x0;
    const edhip_array& out = *lattice0;
    if (x.ndim < 1 || x.ndim > EDHIP_MAX_DIMS)
        return fail(err, errlen, EDHIP_ERR_UNSUPPORTED, "arrays must have 1..%d dimensions", EDHIP_MAX_DIMS);
    for (int j = 0; j < naxis; ++j)
        if (axis[j] < 0 || axis[j] >= x.ndim || (j > 0 && axis[j] <= axis[j - 1]))
            return fail(err, errlen, EDHIP_ERR_INVALID, "invalid axis in axis list");
    if (order < 0 || order > 5)
        return fail(err, errlen, EDHIP_ERR_INVALID, "spline order not supported");
    if (mode < 0 || mode > 4)
        return fail(err, errlen, EDHIP_ERR_INVALID, "boundary mode not supported");
    if (!dtype_ok(x.dtype) || (float_only ? !f32_or_f64(&x) : (x.dtype == EDHIP_F16 || x.dtype == EDHIP_BF16)))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "data type not supported");
    if (out.dtype != x.dtype)
        return fail(err, errlen, EDHIP_ERR_DTYPE, "%s and %s must have one dtype", x_name, lattice_name);
    for (int k = 0; k < naxis; ++k) {
        if (x.shape[axis[k]] != in_len[k])
            return fail(err, errlen, EDHIP_ERR_INVALID, "the %s's deformed axes must have the extents in_len", x_name);
        if (in_len[k] < 2)
            return fail(err, errlen, EDHIP_ERR_INVALID, "deformed axes must have at least 2 elements");
    }
    if (points0->ndim != 2 || points0->shape[1] != naxis || points0->shape[0] < 0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "points must have shape (N, naxis)");
    if (!f32_or_f64(points0))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "points must be float32 or float64");
    const int64_t npts = points0->shape[0];
    {
        // x's dimensions with the deformed axes replaced by one axis of N points at the place of the first
        int64_t want[EDHIP_MAX_DIMS];
        int nd = 0;
        for (int d = 0; d < x.ndim; ++d) {
            bool deformed = false;
            for (int j = 0; j < naxis; ++j)
                deformed = deformed || axis[j] == d;
            if (d == axis[0])
                want[nd++] = npts;
            else if (!deformed)
                want[nd++] = x.shape[d];
        }
        if (!has_shape(lattice0, nd, want))
            return fail(err, errlen, EDHIP_ERR_INVALID,
                        "%s must have the %s's non-deformed axes and one axis of N points", lattice_name, x_name);
    }
    if (int st = check_displacement(displacement0, naxis, nullptr, err, errlen))
        return st;
    if (int st = check_batch_limit(entry, nbatch, err, errlen))
        return st;
    memset(&c, 0, sizeof(c));
    if (int st = fill_geometry(displacement0, in_len, in_len, output_offset, naxis, affine, c.g, err, errlen))
        return st;
    make_sample_view(x, out, naxis, axis, order, mode, cval, c.v);
    c.nbatch = nbatch;
    c.npts = npts;
    c.out_bstride = lattice_batch_stride;
    c.disp_bstride = displacement_batch_stride;
    c.pts = batch_array(points0, points_batch_stride);
    return EDHIP_OK;
}

int edhip_deform_sample(int nbatch, const edhip_array* input0, int64_t input_batch_stride, const edhip_array* points0,
                        int64_t points_batch_stride, const edhip_array* displacement0,
                        int64_t displacement_batch_stride, const int64_t* in_len, const int64_t* output_offset,
                        const edhip_array* output0, int64_t output_batch_stride, const edhip_array* inside0,
                        int64_t inside_batch_stride, int naxis, const int32_t* axis, int32_t order, int32_t mode,
                        double cval, const double* affine, uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    ed::SampleCall c;
    if (int st = fill_sample_call("edhip_deform_sample", nbatch, input0, "input", points0, points_batch_stride,
                                  displacement0, displacement_batch_stride, in_len, output_offset, output0, "output",
                                  output_batch_stride, naxis, axis, order, mode, cval, affine, flags, false, c, err,
                                  errlen))
        return st;
    if (inside0) {
        if (!has_shape(inside0, 1, &c.npts))
            return fail(err, errlen, EDHIP_ERR_INVALID, "inside must have shape (N)");
        if (inside0->dtype != EDHIP_U8)
            return fail(err, errlen, EDHIP_ERR_DTYPE, "inside must be uint8");
    }
    if (nbatch == 0 || c.npts == 0 || c.v.nsteps <= 0)
        return EDHIP_OK;
    c.in_bstride = input_batch_stride;
    c.inside = batch_array(inside0, inside_batch_stride);
    const hipError_t e = ed::launch_deform_sample(c, (hipStream_t)hip_stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform sample launch");
    return EDHIP_OK;
}

int edhip_deform_sample_gradient(int nbatch, const edhip_array* input0, int64_t input_batch_stride,
                                 const edhip_array* cotangent0, int64_t cotangent_batch_stride,
                                 const edhip_array* points0, int64_t points_batch_stride,
                                 const edhip_array* displacement0, int64_t displacement_batch_stride,
                                 const int64_t* in_len, const int64_t* output_offset, const edhip_array* dinput0,
                                 int64_t dinput_batch_stride, const edhip_array* dcoordinate0,
                                 int64_t dcoordinate_batch_stride, int naxis, const int32_t* axis, int32_t order,
                                 int32_t mode, const double* affine, uint32_t flags, void* hip_stream, char* err,
                                 size_t errlen)
{
    using namespace ed;
    if (err && errlen)
        err[0] = 0;
    if (nbatch >= 0 && cotangent0 && points0 && displacement0 && in_len) {
        if (!dinput0 && !dcoordinate0)
            return fail(err, errlen, EDHIP_ERR_INVALID, "neither dinput nor dcoordinate is requested");
        if (dcoordinate0 && !input0)
            return fail(err, errlen, EDHIP_ERR_INVALID, "dcoordinate needs the input");
    }
    // the geometry is read from the input, or from the accumulator when there is no input
    const edhip_array* x0 = input0 ? input0 : dinput0;
    SampleCall c;
    if (int st = fill_sample_call("edhip_deform_sample_gradient", nbatch, x0, input0 ? "input" : "dinput", points0,
                                  points_batch_stride, displacement0, displacement_batch_stride, in_len, output_offset,
                                  cotangent0, "cotangent", cotangent_batch_stride, naxis, axis, order, mode, 0.0,
                                  affine, flags, true, c, err, errlen))
        return st;
    IOView acc;
    memset(&acc, 0, sizeof(acc));
    if (dinput0) {
        if (!has_shape(dinput0, x0->ndim, x0->shape))
            return fail(err, errlen, EDHIP_ERR_INVALID, "dinput must have the shape of the input");
        if (dinput0->dtype != cotangent0->dtype)
            return fail(err, errlen, EDHIP_ERR_DTYPE, "dinput and cotangent must have one dtype");
        make_sample_view(*dinput0, *cotangent0, naxis, axis, order, mode, 0.0, acc);
    }
    const int64_t rows[2] = {c.npts, naxis};
    if (int st = check_point_rows(dcoordinate0, "dcoordinate", 2, rows, true, err, errlen))
        return st;
    if (nbatch == 0 || c.npts == 0 || c.v.nsteps <= 0)
        return EDHIP_OK;
    if (!input0)
        c.v.in = nullptr;                     // (the view was read from the accumulator: only its shape counts)
    c.in_bstride = input_batch_stride;
    const hipError_t e = launch_deform_sample_gradient(c, acc, dinput_batch_stride,
                                                       batch_array(dcoordinate0, dcoordinate_batch_stride),
                                                       (hipStream_t)hip_stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform sample gradient launch");
    return EDHIP_OK;
}

// ---- det J of the coordinate map on the voxel lattice and its adjoint (deform_jacobian.hip) -------------------------
// What edhip_deform_jacobian and edhip_deform_jacobian_gradient check and fill alike.  lattice0: det (written) or ddet
// (read), called `name` in the messages; its own dimensions are the deformed axes.
static int fill_jacobian_call(const char* entry, int nbatch, const edhip_array* lattice0, const char* name,
                              int64_t lattice_batch_stride, const edhip_array* displacement0,
                              int64_t displacement_batch_stride, const int64_t* in_len, const int64_t* output_offset,
                              int naxis, const double* affine, const edhip_array* ddisplacement0,
                              const edhip_array* dinverse_affine0, bool gradient, uint32_t flags, ed::JacobianCall& c,
                              char* err, size_t errlen)
{
    static const int32_t lattice_axes[3] = {0, 1, 2};
    if (int st = check_batch_call(nbatch, lattice0 && displacement0 && in_len, err, errlen))
        return st;
    if (int st = check_axes_1_to_3(entry, lattice_axes, naxis, err, errlen))
        return st;
    if (int st = check_prefiltered(entry, flags, err, errlen))
        return st;
    if (gradient && !ddisplacement0 && !dinverse_affine0)
        return fail(err, errlen, EDHIP_ERR_INVALID, "none of ddisplacement and dinverse_affine is requested");
    if (lattice0->ndim != naxis)
        return fail(err, errlen, EDHIP_ERR_INVALID, "%s must have one dimension per deformed axis", name);
    if (!f32_or_f64(lattice0))
        return fail(err, errlen, EDHIP_ERR_DTYPE, "%s must be float32 or float64", name);
    if (int st = check_displacement(displacement0, naxis, nullptr, err, errlen))
        return st;
    if (int st = check_gradient_outputs(ddisplacement0, displacement0, f32_or_f64_dtype,
                                        "ddisplacement must be float32 or float64", dinverse_affine0, naxis, err, errlen))
        return st;
    if (int st = check_batch_limit(entry, nbatch, err, errlen))
        return st;
    memset(&c, 0, sizeof(c));
    if (int st = fill_geometry(displacement0, in_len, lattice0->shape, output_offset, naxis, affine, c.g, err, errlen))
        return st;
    c.nbatch = nbatch;
    c.disp_bstride = displacement_batch_stride;
    c.det = batch_array(lattice0, lattice_batch_stride);
    return EDHIP_OK;
}

int edhip_deform_jacobian(int nbatch, const edhip_array* displacement0, int64_t displacement_batch_stride,
                          const int64_t* in_len, const int64_t* output_offset, int naxis, const double* affine,
                          const edhip_array* det0, int64_t det_batch_stride, uint32_t flags, void* hip_stream,
                          char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    JacobianCall c;
    if (int st = fill_jacobian_call("edhip_deform_jacobian", nbatch, det0, "det", det_batch_stride, displacement0,
                                    displacement_batch_stride, in_len, output_offset, naxis, affine, nullptr, nullptr,
                                    false, flags, c, err, errlen))
        return st;
    if (nbatch == 0 || c.g.nvox <= 0)
        return EDHIP_OK;
    const hipError_t e = launch_deform_jacobian(c, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform jacobian launch");
    return EDHIP_OK;
}

int edhip_deform_jacobian_gradient(int nbatch, const edhip_array* ddet0, int64_t ddet_batch_stride,
                                   const edhip_array* displacement0, int64_t displacement_batch_stride,
                                   const int64_t* in_len, const int64_t* output_offset, int naxis, const double* affine,
                                   const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                   const edhip_array* dinverse_affine0, int64_t dinverse_affine_batch_stride,
                                   uint32_t flags, void* hip_stream, char* err, size_t errlen)
{
    using namespace ed;
    hipStream_t stream = (hipStream_t)hip_stream;
    JacobianCall c;
    if (int st = fill_jacobian_call("edhip_deform_jacobian_gradient", nbatch, ddet0, "ddet", ddet_batch_stride,
                                    displacement0, displacement_batch_stride, in_len, output_offset, naxis, affine,
                                    ddisplacement0, dinverse_affine0, true, flags, c, err, errlen))
        return st;
    if (nbatch == 0)
        return EDHIP_OK;
    c.ddisp = batch_array(ddisplacement0, ddisplacement_batch_stride);
    c.dK = batch_array(dinverse_affine0, dinverse_affine_batch_stride);
    // the per-unit and per-plane partial sums: the stream's workspace, behind its grid head
    StreamGuard guard(stream);
    hipError_t e = hipSuccess;
    char* ws = (char*)workspace_reserve(stream, kWorkspaceGridBytes + jacobian_grad_scratch_bytes(c.g, nbatch), &e);
    if (!ws)
        return hip_fail(err, errlen, e, "scratch allocation");
    c.scratch = ws + kWorkspaceGridBytes;
    e = launch_deform_jacobian_gradient(c, stream);
    if (e != hipSuccess)
        return hip_fail(err, errlen, e, "deform jacobian gradient launch");
    return EDHIP_OK;
}

}  // extern "C"
