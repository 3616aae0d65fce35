// ed_params.h -- kernel argument blocks (plain structs passed by value) and host-side launchers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edhip.h"

namespace ed {

constexpr int kMaxAxes = EDHIP_MAX_AXES;   // deformed axes on the GPU
constexpr int kMaxSteps = EDHIP_MAX_DIMS;  // non-deformed ("step") axes

// geometry shared by every input of one edhip_deform call: deform.c:381-391,439-451,771-776
struct GridGeom {
    int naxis;
    int has_affine;
    int disp_dtype;
    int pad_;
    int64_t in_len[kMaxAxes];     // I_k: deformed extents of inputs[0]          (deform.c:383)
    int64_t out_len[kMaxAxes];    // O_k: deformed extents of outputs[0]         (deform.c:384)
    int64_t off[kMaxAxes];        // crop offsets                                (deform.c:439-446)
    int64_t ncp[kMaxAxes];        // control points per axis                     (deform.c:449-451)
    const char* disp;             // prefiltered displacement grid
    int64_t disp_stride[kMaxAxes + 1];   // byte strides, [0] = component axis
    double affine[kMaxAxes * (kMaxAxes + 1)];   // inverse map, row-major naxis x (naxis+1)
    int64_t nvox;                 // prod O_k
};

// one input/output pair: deform.c:399-436,762-838
struct IOView {
    const char* in;               // forward: source; gradient: dX (accumulated into)
    char* out;                    // forward: destination; gradient: dY (read)
    int in_dtype, out_dtype;
    int order, mode;
    double cval;
    int64_t in_stride[kMaxAxes];  // byte strides of the deformed axes
    int64_t out_stride[kMaxAxes];
    int nstep;                    // number of non-deformed axes (ascending axis order)
    int steps_fastest;            // 1: flatten work as voxel*nsteps+step (step axes innermost in memory)
    int64_t nsteps;               // product of step extents
    int64_t step_len[kMaxSteps];
    int64_t in_step_stride[kMaxSteps];
    int64_t out_step_stride[kMaxSteps];
    // 16-bit float storage on the OUTPUT side of a float32 call (forward: the result is narrowed at the store;
    // gradient: dY is widened at the load): 1 half, 2 bfloat16.  out_dtype then reads EDHIP_F32 and every output
    // stride is twice its byte value, so that "stride / sizeof(float)" counts 16-bit elements.  Only the level-1
    // kernels of deform_hot.hip know about it (launch_tile declines every other route).
    int out16;
};

// launchers (defined in the .hip files, called from edhip_api.cpp); all enqueue on `stream` and
// return the hipError_t of the launch.
hipError_t launch_deform_exact(const GridGeom& g, const IOView& v, int gradient, hipStream_t stream);
// forward, 3 deformed axes, only the output voxels of a device-side list ([0] = count, [1 .. cap] =
// linear voxel ids; count > cap: every voxel): the near-tie voxels of the integer fast path
hipError_t launch_deform_exact_list(const GridGeom& g, const IOView& v, const int* list, int cap,
                                    hipStream_t stream);

// edhip_source_box: box[2h] = floor(min), box[2h+1] = ceil(max) of the raw (unmapped) source
// coordinate along axis h over every output voxel; `box` = 2 * naxis device ints
// conservative: the convex hull of the control coefficients (a superset of the exact box, O(grid points))
// sw (conservative only): also leave the FILTER window of one input on the device -- 2 * ndim ints (w0, w1) in
// the input's dimension order: the box widened by the tap window, the boundary mode's clipping, the filter's
// decay margin; last-axis rows on `align`-element boundaries; at least `minlen` samples along a deformed axis
struct SourceWindow {
    int32_t* out;                 // device, 2 * ndim ints (nullptr: none)
    int ndim;
    int shape[EDHIP_MAX_DIMS];
    int axis[kMaxAxes];           // array dimension of deformed axis h
    int order, mode, margin, align, minlen;
};
hipError_t launch_source_box(const GridGeom& g, int* box, hipStream_t stream, bool conservative = false,
                             const SourceWindow* sw = nullptr);

// fast path: returns hipErrorNotSupported (without launching) when the case is outside its
// envelope so that the caller can route it to the exact kernels instead.
hipError_t launch_deform_fast(const GridGeom& g, const IOView& v, int gradient, hipStream_t stream);
bool deform_fast_supported(const GridGeom& g, const IOView& v, int gradient);

// LDS-tiled forward kernel (3 deformed axes, order >= 2): the benchmark's hot kernel.
// A batch of independent volumes handled by ONE set of launches (edhip_deform_batch): sample b's
// arrays sit b * stride bytes after sample 0's; everything else (shapes, strides, order, mode, cval,
// crop, affine) is shared.  The strip / tile index of the kernels carries the sample.
struct GridPrefilter;
struct DeformBatch {
    int nbatch;
    int64_t in_bstride, out_bstride, disp_bstride;   // bytes
    int box_mode = 0;               // 1: EDHIP_FLAG_KEEP_BOXES (forward), 2: EDHIP_FLAG_USE_BOXES (gradient)
    const void* disp_id = nullptr;  // the caller's displacement pointer (identity of the control grid)
    int raw = 0;                    // EDHIP_FLAG_RAW_DISPLACEMENT was set
    int strong = 0;                 // EDHIP_FLAG_STRONG_FIELD was set
    // EDHIP_FLAG_ZERO_GRADIENT: the dense block to clear before the scatter; the tile path does it in its
    // tables launch and sets zero_done (left false: nothing has been launched that reads or adds to it)
    char* zero_ptr = nullptr;
    long long zero_bytes = 0;
    mutable bool zero_done = false;
    // EDHIP_FLAG_RAW_DISPLACEMENT, single volume: the control grid is still unfiltered -- the tables kernel of the tile
    // path filters it itself (every workgroup on its own LDS copy, workgroup 0 writes the filtered grid where
    // GridGeom::disp points) and sets gridpf_done; left false: nothing was launched, the caller filters it
    const GridPrefilter* gridpf = nullptr;
    mutable bool gridpf_done = false;
};
hipError_t launch_deform_tile(const GridGeom& g, const IOView& v, int gradient, hipStream_t stream,
                              const DeformBatch* batch = nullptr);
bool deform_tile_supported(const GridGeom& g, const IOView& v, int gradient);
size_t deform_tile_workspace_bytes(const GridGeom& g, int nbatch = 1, bool f64 = false);   // scratch the tile path will ask for (f64: a float64 volume is among the inputs)

// order-0 resampling of label maps (any dtype, 3 deformed axes, forward): bit-equal to the exact
// kernel (fast coordinates, exact re-evaluation of near-tie voxels), see deform_tile.hip
hipError_t launch_deform_label(const GridGeom& g, const IOView& v, hipStream_t stream, const DeformBatch* batch = nullptr);
bool deform_label_supported(const GridGeom& g, const IOView& v, int gradient);
// 8- / 16-bit integer volumes with spline orders 1-5 (forward): bit-equal to the exact kernel (fast
// coordinates and fp64 taps; voxels near a rounding tie or a coordinate boundary re-evaluated exactly)
hipError_t launch_deform_int(const GridGeom& g, const IOView& v, hipStream_t stream, const DeformBatch* batch = nullptr);
bool deform_int_supported(const GridGeom& g, const IOView& v, int gradient);
void tile_profile_enable(int enable);                    // edhip_profile_dominant
double tile_profile_last_us();                           // edhip_profile_last_us

struct FilterParams {
    const char* in;
    char* out;
    int in_dtype, out_dtype;
    int npoles;
    int transpose;
    double pole[2];
    double pole_pow[2];      // pole^(len-1), computed on the host with libm pow() like the reference
    int trunc_branch[2];     // transpose only: (int)ceil(log(1e-15)/log|p|) < len   (deform.c:1119,1134)
    double gain;
    int64_t len;             // extent along the filtered axis
    int64_t in_axis_stride, out_axis_stride;   // bytes
    int nouter;              // number of other axes
    int64_t nlines;
    int64_t outer_len[EDHIP_MAX_DIMS];
    int64_t in_outer_stride[EDHIP_MAX_DIMS];
    int64_t out_outer_stride[EDHIP_MAX_DIMS];
    double* ws;              // fp64 scratch for ws_lines lines, line-interleaved: ws[i * nl + j]
    int64_t ws_lines;        // lines per chunk
};

hipError_t launch_spline_filter(const FilterParams& p, hipStream_t stream);

// one-launch order-3 prefilter of a small control grid along every axis but the first
struct GridPrefilter {
    const char* in;
    char* out;               // contiguous, same dtype
    int dtype, elem_size;
    int ndim, total;
    int shape[kMaxAxes + 1];
    int64_t stride_bytes[kMaxAxes + 1];
    double pole, gain;
    double pole_pow[kMaxAxes + 1];   // pole^(shape[ax] - 1), host libm
    // EDHIP_FLAG_ZERO_GRADIENT: a dense, 16-byte-aligned block that workgroups 1 .. of the launch clear while
    // workgroup 0 filters the grid (the grid's recursion is one workgroup's latency: the rest of the chip is idle)
    char* zero_ptr;
    long long zero_bytes;
};
hipError_t launch_grid_prefilter(const GridPrefilter& p, hipStream_t stream);

// Gradient with respect to the prefiltered control grid (deform_dgrad.hip): dP[h, j] = sum_o g_h(o) beta(o, j).
// Row kernel (one workgroup per output row along the last deformed axis; blockIdx.y = sample) -> fp64 partials
// per (row, h, j_last) in `part`; one contraction launch per remaining deformed axis (fixed summation order, no
// atomics); a last launch writes dP with the layout / dtype of `dst`.  All scratch comes from the caller.
// With `dK` the same row pass also leaves per-row moments of g, reduced in a fixed order to dK[h, l] =
// d(sum <dY, Y>) / d(inverse map)[h, l] (float64, naxis x (naxis+1) per sample).  At least one of dst / dK.
struct DgradCall {
    GridGeom g;                   // g.disp: the prefiltered grid of sample 0
    int ninputs;
    const IOView* views;          // host array: v.in = C_i (read), v.out = dY_i (read); orders 1..5 only
    int nbatch;
    int64_t in_bstride, out_bstride, disp_bstride, dst_bstride;   // bytes between samples
    char* dst;                    // dP, shape (naxis, ncp_0, ...) per sample; nullptr: not wanted
    int dst_dtype;
    int64_t dst_stride[kMaxAxes + 1];
    char* dK;                     // float64 dK, shape (naxis, naxis+1) per sample; nullptr: not wanted
    int64_t dK_stride[2];
    int64_t dK_bstride;
    char* scratch;                // dgrad_scratch_bytes(g, nbatch, dst != nullptr, dK != nullptr) bytes of device scratch
};
constexpr int kDgradMaxK = 256;   // naxis * ncp_{naxis-1}: the row kernel's per-row band of the last grid axis
bool dgrad_supported(const GridGeom& g);
size_t dgrad_scratch_bytes(const GridGeom& g, int nbatch, bool dp = true, bool dk = false);
hipError_t launch_deform_dgrad(const DgradCall& c, hipStream_t stream);

// Sample 0 of an array of a strided batch, as the entry points hand it to the launchers below: sample b sits
// b * bstride bytes after it.  All zero (ptr == nullptr): the array was not given / is not wanted.
struct BatchArray {
    char* ptr;
    int dtype;
    int64_t stride[EDHIP_MAX_DIMS];   // bytes, in the array's own dimension order
    int64_t bstride;
};

// The coordinate map at arbitrary real positions and its inverse (deform_points.hip): one thread per point,
// blockIdx.y = sample, fp64; no scratch, no synchronisation.
struct PointsCall {
    GridGeom g;                   // g.disp: the prefiltered grid of sample 0; in_len >= 2 on every axis
    int inverse;                  // 0: r(q) (and J); 1: q with r(q) = p
    int nbatch;
    int64_t npts;
    int64_t disp_bstride;
    BatchArray pts;               // (npts, naxis), float32 / float64 (read)
    BatchArray res;               // (npts, naxis), float32 / float64
    BatchArray jac;               // forward: float64 (npts, naxis, naxis); not wanted otherwise
    BatchArray status;            // inverse: uint8 (npts), 1 = solved; not wanted otherwise
    const double* forward_linear; // inverse: host, M = (K[:, :naxis])^-1 row-major; nullptr: the identity
    int max_iter;
    double tol;
};
constexpr int kPointsLdsValues = 7680;   // control grids up to this many values are staged in LDS (60 KiB of doubles)
hipError_t launch_deform_points(const PointsCall& c, hipStream_t stream);

// The adjoint of the coordinate map and of its inverse (deform_points_grad.hip): for the cotangents of r(q) (forward) or of
// q = r^-1(p) (inverse, at the solved q) the per-point rows, the gradient with respect to the prefiltered grid and
// with respect to the inverse map K.  Sums are 64-bit integer fixed point (order-independent bits).  The call
// clears its scratch itself (a kernel of its own): [per sample 4 words | per sample naxis (naxis + 1) + values cells | per sample
// npts x naxis doubles], points_grad_scratch_bytes() bytes from the caller.
struct PointsGradCall {
    GridGeom g;                   // g.disp: the prefiltered grid of sample 0; in_len >= 2 on every axis
    int inverse;                  // 0: cot = dL/dr(q); 1: cot = dL/dq at the solved q
    int nbatch;
    int64_t npts;
    int64_t disp_bstride;
    BatchArray pos;               // (npts, naxis) float32 / float64: q (read)
    BatchArray cot;               // (npts, naxis) float32 / float64 (read)
    BatchArray status;            // inverse: uint8 (npts), 0 = not solved (contributes nothing; read); not given: all solved
    BatchArray dpts;              // (npts, naxis) float32 / float64
    BatchArray ddisp;             // the grid's shape, a floating dtype
    BatchArray dK;                // float64 (naxis, naxis + 1)
    char* scratch;
};
size_t points_grad_scratch_bytes(const GridGeom& g, int nbatch, int64_t npts);
hipError_t launch_deform_points_gradient(const PointsGradCall& c, hipStream_t stream);
// The ends of that call's fixed-point reduction for the other callers (ed_points_grad.h has the scheme and the
// scratch layout).  _clear zeroes the heads and cells at the front of `scratch`, in front of the caller's own kernels.
// _reduce, for a caller whose own kernel has written the u rows and the sample heads: the scatter and the finish,
// reading q from `pos` (no status: a row that contributes nothing is zero) and leaving `ddisp` / `dK`; `cot` and
// `dpts` play no part.  _finish, for a caller that has scattered into the cells itself: cell * quantum into `ddisp` /
// `dK` (nothing launched when neither is wanted); own_bounds: the heads hold the two bounds themselves, not max|u|
// and max|q|.
hipError_t launch_points_grad_clear(const GridGeom& g, int nbatch, char* scratch, hipStream_t stream);
hipError_t launch_points_grad_reduce(const PointsGradCall& c, hipStream_t stream);
hipError_t launch_points_grad_finish(const GridGeom& g, int nbatch, const BatchArray& ddisp, const BatchArray& dK,
                                     char* scratch, bool own_bounds, hipStream_t stream);

// Label-aware linear resampling of label maps (deform_vote.hip): per output voxel the order-1 weights are summed per
// distinct label among the 2^naxis source voxels, the label with the largest sum is stored (ties: the smallest label).
// One thread per (voxel, step), blockIdx.y = sample; no scratch, no synchronisation.  1 to 3 deformed axes, integer
// and bool maps (v.in_dtype == v.out_dtype); hipErrorNotSupported (nothing launched) otherwise.
struct LabelsCall {
    GridGeom g;                   // g.disp: the prefiltered grid of sample 0
    IOView v;                     // the label maps of sample 0: v.in read, v.out written; v.mode; order and cval unused
    int nbatch;
    int64_t in_bstride, out_bstride, disp_bstride;   // bytes between samples
    uint64_t cval_bits;           // cval as an element of the map's dtype (two's complement, in the low bytes)
    char* weight;                 // float32, the output's shape: the winning sum; nullptr: not wanted
    int64_t weight_stride[kMaxAxes];                 // byte strides of the deformed axes
    int64_t weight_step_stride[kMaxSteps];           // ... of the non-deformed axes, in the order of v.step_len
    int64_t weight_bstride;
};
hipError_t launch_deform_labels(const LabelsCall& c, hipStream_t stream);

// An image carried back through the deformation (deform_unwarp.hip): for every integer source position p (extents
// g.in_len) the q with r(q) = p, solved as launch_deform_points(inverse) solves it, and the forward gather of `v.in`
// (deformed extents g.out_len) at q, for every step of the voxel.  One thread per source voxel, blockIdx.y = sample; no
// scratch, no synchronisation.  1 to 3 deformed axes, v.in_dtype == v.out_dtype, no 16-bit floats;
// hipErrorNotSupported (nothing launched) otherwise.
struct InverseCall {
    GridGeom g;                   // g.disp: the prefiltered grid of sample 0; in_len = I (>= 2 each), out_len = O
    IOView v;                     // sample 0: v.in = Y (read, extents O), v.out = Z (written, extents I); order, mode, cval
                                  // (the gradient: v.in = dY, added into; v.out = dZ, read)
    int nbatch;
    int64_t in_bstride, out_bstride, disp_bstride;   // bytes between samples
    BatchArray valid;             // uint8, deformed extents I: 1 = solved and inside Y
    const double* forward_linear; // host, M = (K[:, :naxis])^-1 row-major; nullptr: the identity
    int max_iter;
    double tol;
};
hipError_t launch_deform_inverse(const InverseCall& c, hipStream_t stream);
// Its adjoint with respect to the image (deform_unwarp_grad.hip): the same solve and taps per source voxel, and
// v.out (dZ, read, extents I) times the tap weights ADDED into v.in (dY, extents O) with float atomics.  float32 /
// float64 only, v.in_dtype == v.out_dtype; v.cval and `valid` play no part.  One launch, no scratch.
hipError_t launch_deform_inverse_gradient(const InverseCall& c, hipStream_t stream);
// Its gradient with respect to the deformation (deform_unwarp_tgrad.hip): the same solve and taps per source voxel,
// v.in = the coefficients of Y (read, extents O), v.out = dZ (read, extents I), float32 / float64 of one dtype; per
// voxel u = -J^-T dL/dq and q as fp64 rows of `scratch`, reduced by the points gradient's fixed-point kernels into
// ddisp (the gradient of the PREFILTERED grid, the grid's shape, a floating dtype) and dK (float64 (naxis, naxis + 1));
// one of the two may be empty.  v.cval and `valid` play no part.  Four launches (order 0: two);
// inverse_tgrad_scratch_bytes() bytes of scratch from the caller: per sample 4 + naxis (naxis + 1) + naxis prod ncp
// words and 2 * naxis * 8 bytes per source voxel.
size_t inverse_tgrad_scratch_bytes(const GridGeom& g, int nbatch);
hipError_t launch_deform_inverse_transform_gradient(const InverseCall& c, const BatchArray& ddisp, const BatchArray& dK,
                                                    char* scratch, hipStream_t stream);

// The deformed image at real output positions (deform_sample.hip): per point q the coordinate r(q) of
// launch_deform_points (forward direction) and the forward gather of `v.in` (X, deformed extents g.in_len) at r, for
// every step.  One thread per point (grid-stride beyond kPointsMaxBlocks * 256), blockIdx.y = sample; no scratch, no
// atomics, no synchronisation.  1 to 3 deformed axes, v.in_dtype == v.out_dtype, no 16-bit floats;
// hipErrorNotSupported (nothing launched) otherwise.
struct SampleCall {
    GridGeom g;                   // g.disp: the prefiltered grid of sample 0; in_len = I (>= 2 each); out_len unused
    IOView v;                     // sample 0: v.in = X (read, extents I); v.out = V (written; out_stride[0]: the byte
                                  // stride of its point axis, the others unused); order, mode, cval
                                  // (the gradient: v.in = the coefficients of X, read, or nullptr; v.out = dV, read)
    int nbatch;
    int64_t npts;
    int64_t in_bstride, out_bstride, disp_bstride;   // bytes between samples
    BatchArray pts;               // (npts, naxis) float32 / float64 (read)
    BatchArray inside;            // uint8 (npts): 1 = a sane position with 0 <= r_k <= I_k - 1 on every axis
};
hipError_t launch_deform_sample(const SampleCall& c, hipStream_t stream);
// Its gradients (deform_sample_grad.hip), the same front and taps per point, either or both per call: `acc` (X's
// shape, float32 / float64, the cotangent's dtype) has A^T dV ADDED with float atomics; dcoord (float64 (npts, naxis))
// gets the row g = dL/dr of its point, which needs v.in, the coefficients of X in the cotangent's dtype.
hipError_t launch_deform_sample_gradient(const SampleCall& c, const IOView& acc, int64_t acc_bstride,
                                         const BatchArray& dcoord, hipStream_t stream);

// det J of the coordinate map on the voxel lattice and its adjoint (deform_jacobian.hip): rows along the last deformed
// axis, the other axes contracted once per row; blockIdx.y = sample, fp64, no atomics.  1 to 3 deformed axes;
// hipErrorNotSupported (nothing launched) otherwise.
struct JacobianCall {
    GridGeom g;                   // g.disp: the prefiltered grid of sample 0; in_len = I (>= 2 each), out_len = the crop
    int nbatch;
    int64_t disp_bstride;
    BatchArray det;               // deformed extents g.out_len, float32 / float64: det (written) / dL/d det (read)
    BatchArray ddisp;             // gradient: of the PREFILTERED grid, the grid's shape, float32 / float64; may be empty
    BatchArray dK;                // gradient: float64 (naxis, naxis + 1); may be empty
    char* scratch;                // gradient: jacobian_grad_scratch_bytes() bytes
};
hipError_t launch_deform_jacobian(const JacobianCall& c, hipStream_t stream);
// per sample rows * nch * (naxis^2 w + naxis^2) doubles -- a row is served in nch units of xc <= 256 voxels, each
// reaching at most w control points of the last axis (w <= min(ncp_last, ceil((xc - 1) s_last) + 6); xc as large as
// naxis^2 w <= 512 and xc w <= 1280 allow) --; 3 axes: plus O_0 * (2 naxis ncp_1 ncp_2 + naxis^2) doubles
size_t jacobian_grad_scratch_bytes(const GridGeom& g, int nbatch);
hipError_t launch_deform_jacobian_gradient(const JacobianCall& c, hipStream_t stream);

// first bytes of every per-stream workspace are reserved for the prefiltered control grid
constexpr size_t kWorkspaceGridBytes = 64 * 1024;

// fast path (orders 2/3, float32/float64, lines >= 64 samples, no scratch); hipErrorNotSupported
// (nothing launched) when the case is outside its envelope
// window: 2 ints (w0, w1) per array dimension in DEVICE memory (edhip_source_window) -- only the samples inside
// are read and written; hipErrorNotSupported (nothing launched) when the whole-line tile kernels cannot take it
hipError_t launch_spline_filter_fast(const FilterParams& p, int order, int ndim, int axis,
                                     const int64_t* shape, const int64_t* in_stride_bytes,
                                     const int64_t* out_stride_bytes, hipStream_t stream,
                                     const int* window = nullptr, bool dry = false);

}  // namespace ed
