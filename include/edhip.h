/*
 * edhip.h -- C ABI of the MI355X-native elastic grid deformation hot path.
 *
 * This is the drop-in boundary.  It replaces, one for one, the three entry points of the
 * reference's CPython extension `_deform_grid` (method table
 * /root/reference/elasticdeform/_deform_grid.c:306-311):
 *
 *   _deform_grid.deform_grid(...)          _deform_grid.c:296-299  -> edhip_deform(gradient=0, ...)
 *   _deform_grid.deform_grid_grad(...)     _deform_grid.c:301-304  -> edhip_deform(gradient=1, ...)
 *   _deform_grid.spline_filter1d_grad(...) _deform_grid.c:61-92    -> edhip_spline_filter1d(transpose=1)
 *   scipy.ndimage.spline_filter1d(...)     call sites deform_grid.py:160,168,271
 *                                                                  -> edhip_spline_filter1d(transpose=0)
 *
 * and its argument list mirrors the C core they all funnel into,
 *
 *   int DeformGrid(int gradient, int ninputs, PyArrayObject** inputs, PyArrayObject* displacement,
 *                  PyArrayObject* output_offset, PyArrayObject** outputs, int naxis, int* axis,
 *                  int* orders, int* modes, double* cvals, double* affine);      deform.h:15-16
 *   int NI_SplineFilter1DGrad(PyArrayObject*, int order, int axis, PyArrayObject*);  deform.h:18
 *
 * with `PyArrayObject*` replaced by the plain-old-data descriptor `edhip_array`
 * (pointer + dtype code + shape + byte strides == what PyArray_DATA / PyArray_TYPE /
 * PyArray_DIM / PyArray_STRIDE give the reference, deform.c:383-391,401,427-431).
 *
 * No Python, NumPy or torch type appears in any signature.  `data` pointers are DEVICE pointers
 * (HBM on the MI355X that owns `hip_stream`); the small parameter arrays (axis, orders, modes,
 * cvals, affine, output_offset) are HOST pointers, read before the call returns.
 *
 * Ownership: the caller allocates every array; the library borrows them for the duration of the
 * enqueued work and owns only a small scratch workspace per (device, stream), grown on demand.
 * Calls are asynchronous with respect to the host: work is enqueued on `hip_stream` and the
 * function returns; there is no implicit device synchronisation -- with one exception: when a call
 * needs MORE scratch than the stream's cached workspace holds, growing it waits for that stream once
 * (hipStreamSynchronize + hipFree + hipMalloc; not allowed under stream capture: warm the workspace
 * up with one call before capturing).  Requests above 320 MiB (the dense temporary of the float32
 * order-4/5 prefilter cascade on long lines, the fp64 line buffer of the exact filter on large
 * arrays) are stream-ordered allocations that are released when the call has enqueued its work.
 * Next to the workspace the library keeps, per (device, stream), 64 bytes of pinned host memory into
 * which the float32 tile kernels report how many of a call's tiles did not fit their standard LDS boxes
 * (written by the NEXT call's first kernel, read by the host without waiting): later calls of the same
 * geometry then start on larger boxes.  This changes speed only -- the forward result of a voxel is the
 * same bits whichever box size or tile level served it.  Apart from these mutex-guarded per-stream
 * caches the library keeps no mutable global state, so it is re-entrant and may be
 * called concurrently from several host threads on different streams / devices
 * (reference: single-threaded, GIL released for the whole call, deform.c:377-379).
 *
 * Error convention (reference: return 0 with a Python exception set, deform.c:1042,
 * _deform_grid.c:293): return EDHIP_OK (0) on success, otherwise a non-zero code and a
 * NUL-terminated message in `err` (if errlen > 0).  The host shim maps codes to the exception
 * classes the reference raises.
 */
#ifndef EDHIP_H
#define EDHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDHIP_VERSION 100        /* 0.1.0 */
#define EDHIP_MAX_DIMS 8         /* max ndim of any array (reference: NPY_MAXDIMS) */
#define EDHIP_MAX_AXES 7         /* max number of deformed axes: the control grid has naxis + 1 <= EDHIP_MAX_DIMS dims */
#define EDHIP_MAX_INPUTS 64

/* dtype codes: the 13 NumPy types the reference switches over (deform.c:716-741,863-887,
 * 907-919) collapse to 11 distinct machine types on LP64 (long == long long); two 16-bit floating
 * point storage types are an extension. */
enum edhip_dtype {
    EDHIP_BOOL = 0, /* npy_bool  (unsigned char; store is a plain C cast, deform.c:287-290,907) */
    EDHIP_U8 = 1,
    EDHIP_I8 = 2,
    EDHIP_U16 = 3,
    EDHIP_I16 = 4,
    EDHIP_U32 = 5,
    EDHIP_I32 = 6,
    EDHIP_U64 = 7,
    EDHIP_I64 = 8,
    EDHIP_F32 = 9,
    EDHIP_F64 = 10,
    /* reduced-precision storage -- NOT part of the reference's
     * contract, which rejects half precision with "data type not supported" (deform.c:742-747); the
     * host shim only hands these over when the caller opted in.  Arithmetic stays fp64 / fp32:
     * values are widened on load and rounded to nearest-even on store. */
    EDHIP_F16 = 11, /* IEEE binary16 */
    EDHIP_BF16 = 12, /* bfloat16 */
    EDHIP_NUM_DTYPES = 13
};

/* boundary modes, same integer codes as the reference (from_scipy.h:38-47,
 * deform_grid.py:440-454) */
enum edhip_mode {
    EDHIP_MODE_NEAREST = 0,
    EDHIP_MODE_WRAP = 1,
    EDHIP_MODE_REFLECT = 2,
    EDHIP_MODE_MIRROR = 3,
    EDHIP_MODE_CONSTANT = 4
};

/* return codes */
enum edhip_status {
    EDHIP_OK = 0,
    EDHIP_ERR_INVALID = 1,     /* shape / argument check failed   -> RuntimeError  (_deform_grid.c:121-255) */
    EDHIP_ERR_DTYPE = 2,       /* "data type not supported"       -> RuntimeError  (deform.c:744,891,922)   */
    EDHIP_ERR_MEMORY = 3,      /* scratch allocation failed       -> MemoryError   (deform.c:394-398 ...)   */
    EDHIP_ERR_DEVICE = 4,      /* a HIP call / kernel launch failed -> RuntimeError                         */
    EDHIP_ERR_UNSUPPORTED = 5  /* legal in the reference, outside this build's limits (more than 8 dims ...)   */
};

/* arithmetic selection for edhip_deform / edhip_spline_filter1d */
enum edhip_flags {
    EDHIP_FLAG_AUTO = 0,       /* float32 / float64 data -> fast path; integer and bool data -> bit-equal to the
                                  exact path (order-0 label maps and 8- / 16- / 32-bit integer volumes of orders 1-5: fast
                                  coordinates, near-tie voxels re-evaluated exactly; the rest: exact kernels) */
    EDHIP_FLAG_EXACT = 1,      /* fp64 arithmetic in the reference's own evaluation order (bit-comparable) */
    EDHIP_FLAG_FAST = 2,       /* fp64 coordinates, restructured (separable) sums, data-width tap accumulation
                                  (what AUTO selects for floating-point data).
                                  Given explicitly it also opens the pairs of a float32 array and a 16-bit float one
                                  (EDHIP_F16 / EDHIP_BF16; an extension -- the reference rejects float16, deform.c:742-747):
                                  float32 arithmetic with 16 bits in HBM on one side, converted inside the kernel that
                                  reads or writes it instead of by a cast pass --
                                    edhip_deform  inputs float32, outputs 16-bit: forward = the result is rounded to nearest
                                                  even at the store; gradient = dY is widened at the load (dX stays float32);
                                                  3 deformed axes, orders 1-3, unit stride along the last one;
                                    edhip_spline_filter_axes  16-bit input, float32 output: the first pass widens;
                                                  float32 input, 16-bit output with EDHIP_FLAG_SCRATCH_INPUT: the last pass
                                                  narrows; orders 2 / 3, lines of 64..256 samples, dense arrays.
                                  A pair outside those envelopes returns EDHIP_ERR_UNSUPPORTED
                                  (without the flag such pairs run on the exact kernels like any other dtype pair).
                                  edhip_deform decides per input: the control-grid prefilter of a RAW_DISPLACEMENT call
                                  (and the clear of a ZERO_GRADIENT call) has been enqueued by then, and with several
                                  inputs the kernels of the inputs in front of the declined one have run -- a caller
                                  that retries another way must treat every output of the call as unwritten and zero
                                  gradient accumulators again.  The filter entry points decline before any launch. */
    /* edhip_deform only: `displacement` is the RAW control grid; the library applies the order-3
     * mirror prefilter along every grid axis itself (what deform_grid.py:166-169,269-272 does with
     * SciPy before calling the C code), in one launch, with the same arithmetic and the same
     * per-axis rounding to the grid's dtype.  Grids of more than 4096 points are refused
     * (EDHIP_ERR_UNSUPPORTED): prefilter those with edhip_spline_filter1d. */
    EDHIP_FLAG_RAW_DISPLACEMENT = 4,
    /* edhip_deform / edhip_deform_batch*, forward (gradient = 0): also leave the bounding boxes of
     * the tiles' tap windows -- a by-product of the forward kernel -- in a small per-stream buffer
     * for the gradient call that follows (float32, 3 deformed axes: the tile kernels of
     * deform_hot.hip; ignored elsewhere). */
    EDHIP_FLAG_KEEP_BOXES = 8,
    /* gradient = 1: the caller promises that the displacement's CONTENTS and the geometry are those of
     * the last EDHIP_FLAG_KEEP_BOXES forward call on this stream (autograd: the backward of that
     * forward).  The library compares the arguments it can see (pointer, shape, strides, extents,
     * offsets, affine, order, mode); when they match the gradient kernel takes its tiles' boxes from
     * the buffer instead of computing every window twice.  The boxes are a HINT: a voxel whose window
     * does not lie in its tile's box is scattered straight to global memory, so a broken promise
     * costs time, never correctness. */
    EDHIP_FLAG_USE_BOXES = 16,
    /* gradient = 1: the library clears the gradient accumulators (`inputs`) itself before it scatters
     * into them -- the reference's numpy.zeros (deform_grid.py:243) -- so the caller may hand over
     * uninitialised memory.  The arrays must be dense (their elements one contiguous block, in any axis
     * order); float32 volumes on the tile kernels get the fill from spare workgroups of the per-call tables
     * launch (it overlaps that kernel instead of being a bandwidth-bound launch of its own), every other
     * route a hipMemsetAsync.  Without the flag the accumulators are added to as they are. */
    EDHIP_FLAG_ZERO_GRADIENT = 32,
    /* with EDHIP_FLAG_RAW_DISPLACEMENT: the caller promises that the raw control grid is, byte for byte, the one
     * of the previous RAW_DISPLACEMENT call on this stream (edhip_source_window followed by edhip_deform inside
     * one deform_grid call): when the library finds that call's filtered copy still in the stream's workspace
     * (same pointer, dtype, shape and strides, workspace not moved) it does not filter the grid again. */
    EDHIP_FLAG_GRID_STAYS = 64,
    /* edhip_spline_filter_axes: the caller hands `input` over as scratch -- every pass but the last runs in place on
     * it and the last one writes `output` (instead of: input -> output, then in place on the output).  With a
     * float32 input and an EDHIP_F16 / EDHIP_BF16 output the chain is computed in float32 and only its result is
     * rounded to 16 bits (the last pass narrows on its way out: 6 instead of 8 bytes per sample, and no cast pass). */
    EDHIP_FLAG_SCRATCH_INPUT = 128,
    /* edhip_deform / edhip_deform_batch*, forward, float32 volumes, 3 deformed axes, orders 1-3: a HINT that the
     * displacement field is strong (displacement gradient of ~0.15 per voxel and more: sigma >= 10 on a 5^3 grid over
     * 256^3, the reference README's own example).  The forward call then takes the z-walk route (csrc/deform_k1z.hip:
     * per-call geometry kernel, tiles split in halves, four row pitches) for EVERY geometry that route supports; without
     * the flag only single volumes whose z and y extents are multiples of 256 take it -- where it is measured faster
     * on mild fields too (profiles/r06_k1_route_sweep.txt) -- and everything else runs on the x-strip kernel
     * (csrc/deform_k1.hip), which is 5-50 % faster on mild fields and 5-35 % slower on strong ones.  The route is a
     * function of the call's arguments alone, never of earlier calls; the two routes agree to float32 rounding
     * (coordinates differ by ~1e-15), each is bit-reproducible. */
    EDHIP_FLAG_STRONG_FIELD = 256
};

/* strided N-d array in device memory: the POD stand-in for PyArrayObject* */
typedef struct edhip_array {
    void*   data;                          /* device pointer to element [0,...,0]          */
    int32_t dtype;                         /* enum edhip_dtype                              */
    int32_t ndim;                          /* 0 < ndim <= EDHIP_MAX_DIMS                    */
    int64_t shape[EDHIP_MAX_DIMS];         /* extents                                       */
    int64_t stride_bytes[EDHIP_MAX_DIMS];  /* byte strides (any sign, any order, may be 0)  */
} edhip_array;

/* library version (EDHIP_VERSION of the build) */
int edhip_version(void);

/* static string for a status code */
const char* edhip_status_string(int status);

/* number of visible HIP devices, or -1 if the HIP runtime cannot be initialised.  Lets a host
 * shim fail loudly before any compute call. */
int edhip_device_count(void);

/*
 * Forward deformation (gradient == 0) or its exact adjoint (gradient != 0).
 * Replaces DeformGrid (deform.c:340-1043) behind Py_DeformGrid_helper (_deform_grid.c:94-294).
 *
 *   inputs[ninputs]      forward: (prefiltered) source arrays, read.
 *                        gradient: dX arrays, accumulated into -- MUST be zero-filled on entry
 *                        (deform_grid.py:243).
 *   displacement         prefiltered control-point grid, shape (naxis, ncp_0, ..., ncp_{naxis-1}),
 *                        any dtype / strides (deform.c:388-391,715-741).
 *   output_offset        naxis crop offsets (host int64) or NULL (deform.c:439-446).
 *   outputs[ninputs]     forward: written.  gradient: dY arrays, read.
 *                        outputs[i].ndim == inputs[i].ndim; deformed extents of every output equal
 *                        those of outputs[0], of every input those of inputs[0]
 *                        (_deform_grid.c:137-175).
 *   axis                 host int32[ninputs * naxis], the deformed axes of each input, ascending.
 *   orders, modes, cvals host arrays of length ninputs: spline order 0..5, enum edhip_mode, cval.
 *   affine               host double[naxis * (naxis+1)], row-major INVERSE map output->source,
 *                        or NULL (deform.c:771-776; built by deform_grid.py:392-438).
 *   flags                enum edhip_flags.
 *   hip_stream           hipStream_t to enqueue on (NULL = the legacy default stream).
 *
 * Float gradients (fast arithmetic, 3 deformed axes): a tile of output voxels is accumulated in LDS
 * in fixed point, in a scale taken from the tile's sum of |dY|; one contribution is resolved to
 * wmax * sum|dY| / 2^31 of its tile (float32; 2^62 for float64) -- far below the float32 rounding of
 * the reference's own `+=` (deform.c:309-312) for data of one magnitude.  The bound is ABSOLUTE per
 * tile (8 x 8 x 16 output voxels): next to a dY value that is orders of magnitude above its
 * neighbours, the neighbours' contributions are rounded to that resolution (1e6 among 1e-3: the small
 * ones keep about 1e-4 absolute), where the reference's float `+=` keeps their relative precision in
 * cells the large value does not reach; other tiles are unaffected.  Non-finite dY values are added
 * with float atomics.  The order of the atomic additions is not reproducible from run to run
 * (about 1e-7 of the gradient's scale).  Integer gradients are bit-exact.
 */
int edhip_deform(int gradient, int ninputs,
                 const edhip_array* inputs,
                 const edhip_array* displacement,
                 const int64_t* output_offset,
                 const edhip_array* outputs,
                 int naxis, const int32_t* axis,
                 const int32_t* orders, const int32_t* modes, const double* cvals,
                 const double* affine,
                 uint32_t flags, void* hip_stream,
                 char* err, size_t errlen);

/*
 * A batch of independent volumes, each with its own control grid (per-sample augmentation:
 * SURVEY.md section 8(f) rank 2): item b is exactly
 *   edhip_deform(gradient, 1, &inputs[b], &displacements[b], output_offset, &outputs[b], naxis,
 *                axis, &order, &mode, &cval, affine, flags, hip_stream, ...)
 * -- same results, bit for bit.  `axis` (naxis entries), order, mode, cval, the crop offsets and
 * the affine map are shared by the batch.  Descriptors that differ only by a constant pointer
 * stride (see edhip_deform_batch_strided) take the single-launch path described there; anything
 * else is enqueued item by item.
 * The reference has no batched entry point; a host loop over its deform_grid is the equivalent.
 */
int edhip_deform_batch(int gradient, int nbatch,
                       const edhip_array* inputs,
                       const edhip_array* displacements,
                       const int64_t* output_offset,
                       const edhip_array* outputs,
                       int naxis, const int32_t* axis,
                       int32_t order, int32_t mode, double cval,
                       const double* affine,
                       uint32_t flags, void* hip_stream,
                       char* err, size_t errlen);

/*
 * The same batch described once: sample b's arrays are sample 0's moved by b * stride bytes (a
 * stacked tensor with a leading batch axis).  Spares the caller nbatch descriptors per array.
 * When the volumes are float32 / float64 with 3 deformed axes and the control grids are already
 * prefiltered (no EDHIP_FLAG_RAW_DISPLACEMENT), the whole batch is ONE set of launches: one tables
 * kernel producing the per-sample displacement tables, one tile launch whose strip index carries
 * the sample, one pair of spill passes -- bit-identical to nbatch edhip_deform calls.
 */
int edhip_deform_batch_strided(int gradient, int nbatch,
                               const edhip_array* input0, int64_t input_batch_stride,
                               const edhip_array* displacement0, int64_t displacement_batch_stride,
                               const int64_t* output_offset,
                               const edhip_array* output0, int64_t output_batch_stride,
                               int naxis, const int32_t* axis,
                               int32_t order, int32_t mode, double cval,
                               const double* affine,
                               uint32_t flags, void* hip_stream,
                               char* err, size_t errlen);

/*
 * Gradient of the deformation with respect to the control-point displacement (no counterpart in the
 * reference, whose wrappers drop this gradient).  Arguments as for edhip_deform(gradient = 0, ...), with
 *   inputs[ninputs]      the (prefiltered) source arrays C_i the forward read, read.  float32 / float64 only
 *                        (every other dtype: EDHIP_ERR_DTYPE before any launch).
 *   doutputs[ninputs]    dY_i, the gradient with respect to the forward's outputs, read; float32 / float64.
 *   ddisplacement        written: the shape of `displacement`, any dtype / strides (rounded once).
 * Without EDHIP_FLAG_RAW_DISPLACEMENT `displacement` is the prefiltered grid P and the result is
 *   dP[h, j] = d(sum_i <dY_i, Y_i>) / dP[h, j]
 *            = sum_o beta(o, j) sum_i sum_step dY_i[o, step] map'_h sum_k C_i[k, step] w'_h(m_h, k_h) prod_{e!=h} w_e(m_e, k_e)
 * (beta: the cubic weights of control point j at output voxel o; w': the derivative of the order-p weights of
 * deform.c:160-268; map': the slope of the boundary map's branch, deform.c:47-128 -- +1 inside and for 'wrap',
 * -1 on the folds of 'mirror' / 'reflect', 0 where 'nearest' clamps; a 'constant' voxel outside the volume
 * contributes nothing; at a kink, the one-sided derivative of the branch the forward takes).  With
 * EDHIP_FLAG_RAW_DISPLACEMENT `displacement` is the RAW grid D (at most 4096 points): the library applies the
 * order-3 mirror prefilter itself and returns dD = (prefilter)^T dP.  Order 0 gives exact zeros.
 * Arithmetic: fp64 coordinates and weights, tap sums in the volume's type, fp64 accumulation across voxels in a
 * fixed order (no atomics): the result is bit-reproducible from run to run.  No host synchronisation beyond the
 * workspace rule above; the call can be captured into a HIP graph once the stream's workspace is warm.
 * naxis * (control points along the last deformed axis) is limited to 256 (EDHIP_ERR_UNSUPPORTED beyond).
 */
int edhip_deform_displacement_gradient(int ninputs, const edhip_array* inputs,
                                       const edhip_array* displacement,
                                       const int64_t* output_offset,
                                       const edhip_array* doutputs,
                                       int naxis, const int32_t* axis,
                                       const int32_t* orders, const int32_t* modes, const double* cvals,
                                       const double* affine,
                                       const edhip_array* ddisplacement,
                                       uint32_t flags, void* hip_stream,
                                       char* err, size_t errlen);

/*
 * The same for a batch described once, as edhip_deform_batch_strided: sample b's input, control grid, dY and
 * result are sample 0's moved by b * stride bytes; axis / order / mode / cval / crop / affine are shared.
 * Sample b's result is bit-identical to edhip_deform_displacement_gradient on sample b alone.  Prefiltered
 * grids: one set of launches for the whole batch (the row kernel's grid carries the sample); RAW grids are
 * prefiltered and transposed sample by sample.
 */
int edhip_deform_displacement_gradient_batch_strided(int nbatch,
                                                     const edhip_array* input0, int64_t input_batch_stride,
                                                     const edhip_array* displacement0, int64_t displacement_batch_stride,
                                                     const int64_t* output_offset,
                                                     const edhip_array* doutput0, int64_t doutput_batch_stride,
                                                     int naxis, const int32_t* axis,
                                                     int32_t order, int32_t mode, double cval,
                                                     const double* affine,
                                                     const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                                     uint32_t flags, void* hip_stream,
                                                     char* err, size_t errlen);

/*
 * Gradient with respect to the displacement AND the inverse map.  Arguments as for
 * edhip_deform_displacement_gradient, with ddisplacement nullable and
 *   dinverse_affine      written (NULL: not wanted): float64 device array of shape naxis x (naxis+1), any strides,
 *                        dK[h, l] = d(sum_i <dY_i, Y_i>) / dK[h, l] for the map the coordinate applies,
 *                          c_h(o) = sum_l K[h, l] o_l + K[h, naxis] + offset_h + displacement_h(o)
 *                        (o: the crop-local output index, deform.c:771-781; K = `affine` as passed, the identity
 *                        when `affine` is NULL), i.e. dK[h, l < naxis] = sum_o g_h(o) o_l, dK[h, naxis] = sum_o g_h(o)
 *                        with g_h the per-voxel field of the displacement gradient above.
 * Both NULL: EDHIP_ERR_INVALID.  A wrong shape (EDHIP_ERR_INVALID) or dtype (EDHIP_ERR_DTYPE) of dinverse_affine is
 * refused before any launch.  When both are requested they come from one pass of the row kernel per input;
 * ddisplacement is then the same bits as edhip_deform_displacement_gradient's.  dK is summed in fp64 in a fixed
 * order (bit-reproducible, no atomics); order 0, empty step axes and no output voxels give exact zeros.
 */
int edhip_deform_transform_gradient(int ninputs, const edhip_array* inputs,
                                    const edhip_array* displacement,
                                    const int64_t* output_offset,
                                    const edhip_array* doutputs,
                                    int naxis, const int32_t* axis,
                                    const int32_t* orders, const int32_t* modes, const double* cvals,
                                    const double* affine,
                                    const edhip_array* ddisplacement,
                                    const edhip_array* dinverse_affine,
                                    uint32_t flags, void* hip_stream,
                                    char* err, size_t errlen);

/*
 * The same for a batch described once (edhip_deform_displacement_gradient_batch_strided): sample b's dK is written
 * dinverse_affine_batch_stride bytes after sample 0's and is bit-identical to edhip_deform_transform_gradient on
 * sample b alone.
 */
int edhip_deform_transform_gradient_batch_strided(int nbatch,
                                                  const edhip_array* input0, int64_t input_batch_stride,
                                                  const edhip_array* displacement0, int64_t displacement_batch_stride,
                                                  const int64_t* output_offset,
                                                  const edhip_array* doutput0, int64_t doutput_batch_stride,
                                                  int naxis, const int32_t* axis,
                                                  int32_t order, int32_t mode, double cval,
                                                  const double* affine,
                                                  const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                                  const edhip_array* dinverse_affine0,
                                                  int64_t dinverse_affine_batch_stride,
                                                  uint32_t flags, void* hip_stream,
                                                  char* err, size_t errlen);

/*
 * The coordinate map of a deformation at arbitrary real positions, and its inverse (no counterpart in the reference).
 * For a real, crop-local output position q of an edhip_deform call with this control grid, crop offset and inverse
 * map K (`affine`; the identity when NULL),
 *   cp_k   = (ncp_k - 1) (q_k + offset_k) / (in_len_k - 1)
 *   r_h(q) = sum_l K[h, l] q_l + K[h, naxis] + offset_h + sum_taps P[h, m(floor(cp) - 1 + t)] prod_k w_k[t_k]
 * (w: the cubic weights, m: the mirror tap map of deform.c:650-758): at integer q the source coordinate of
 * deform.c:771-781 BEFORE the boundary map.  No boundary mode is applied; the mirror tap map extends the spline to
 * every real q.
 *   inverse == 0         result[i] = r(points[i]); with `jacobian` also J[i, h, l] = d r_h / d q_l (analytic).
 *   inverse != 0         result[i] = q with r(q) = points[i] -- where a source position lands in the output -- by a
 *                        damped Newton iteration in fp64 from q0 = M (p - offset - K[:, naxis]): the step from the
 *                        analytic J, halved (at most 10 times) while the residual's max-norm does not decrease, until
 *                        |r(q) - p|_inf <= tol.  After max_iter steps, an exhausted backtrack, a singular J or a
 *                        non-finite point the result is NaN in every component and status[i] = 0; status[i] = 1 for a
 *                        solved point.  On a folded field a point may have several pre-images: the result is the one
 *                        this iteration reaches from q0 (deterministic).
 * The batch is described once, as for edhip_deform_batch_strided: sample b's points, control grid, result, jacobian
 * and status are sample 0's moved by b * stride bytes (nbatch = 1: a single call); everything else is shared.
 *   points0 / result0    (N, naxis), float32 or float64 each, any strides; the arithmetic is fp64, a float32 result is
 *                        rounded once at the store.  N = 0 launches nothing.
 *   displacement0        the PREFILTERED control grid (naxis, ncp_0, ...), any dtype / strides.
 *                        EDHIP_FLAG_RAW_DISPLACEMENT is refused (EDHIP_ERR_INVALID): the caller prefilters.
 *   in_len               host int64[naxis]: the deformed extents of the input (>= 2 each).
 *   output_offset        naxis crop offsets (host int64) or NULL;  affine: K, host double[naxis * (naxis+1)] or NULL.
 *   forward_linear       inverse only: M = (K[:, :naxis])^-1, host double[naxis * naxis] row-major; NULL with a NULL
 *                        affine (the identity).
 *   jacobian0            NULL, or (forward only) float64 (N, naxis, naxis), any strides.
 *   status0              NULL, or (inverse only) uint8 (N).
 *   max_iter, tol        inverse only: >= 1 and > 0.
 * Every shape and dtype check answers before any launch.  One launch, one thread per point, no atomics: a point's
 * result depends on that point and the call's arguments alone (a sample of a batch, a slice of the points and a
 * repeated call give the same bits).  The call enqueues on hip_stream, never synchronises and uses no workspace, so
 * it can be captured into a HIP graph.
 */
int edhip_deform_points(int inverse, int nbatch,
                        const edhip_array* points0, int64_t points_batch_stride,
                        const edhip_array* displacement0, int64_t displacement_batch_stride,
                        const int64_t* in_len,
                        const int64_t* output_offset,
                        int naxis,
                        const double* affine,
                        const double* forward_linear,
                        const edhip_array* result0, int64_t result_batch_stride,
                        const edhip_array* jacobian0, int64_t jacobian_batch_stride,
                        const edhip_array* status0, int64_t status_batch_stride,
                        int max_iter, double tol,
                        uint32_t flags, void* hip_stream,
                        char* err, size_t errlen);

/*
 * The adjoint of edhip_deform_points: gradients through the coordinate map and through its inverse (no counterpart in
 * the reference).  In the notation above, with beta(q, j) the sum of the cubic tap-weight products whose mirrored tap
 * index is j (beta >= 0, sum_j beta = 1; with few control points several taps of one point fold onto one j),
 *   r_h(q) = sum_l K[h, l] q_l + K[h, naxis] + offset_h + sum_j P[h, j] beta(q, j)
 * is linear in the prefiltered grid P and in K.
 *   inverse == 0   positions = q_i, cotangent u[i, :] = dL / d r(q_i):
 *                    dpoints[i, l]        = sum_h J[i, h, l] u[i, h]
 *                    ddisplacement[h, j]  = sum_i u[i, h] beta(q_i, j)                (= dL / dP)
 *                    dinverse_affine[h, l < naxis] = sum_i u[i, h] q_i[l],  [h, naxis] = sum_i u[i, h]
 *   inverse != 0   positions = the SOLVED q_i = r^-1(p_i) (the result of edhip_deform_points), cotangent
 *                  g[i, :] = dL / d q_i.  By the implicit function theorem at q_i:
 *                    dpoints[i, :] = J(q_i)^-T g[i, :]                                 (= dL / d p_i)
 *                    ddisplacement, dinverse_affine: the sums above with u[i, :] = -J(q_i)^-T g[i, :]
 * ddisplacement is the gradient with respect to the PREFILTERED grid; the caller applies the transposed prefilter.
 * Points that contribute nothing get a zero row of their own and their cotangent is ignored: (forward) a position
 * that is not finite or whose control coordinate exceeds 4e15; (inverse) status[i] == 0, a non-finite q, a singular or
 * non-finite J.
 *   positions0 / cotangent0 / dpoints0   (N, naxis), float32 or float64 each, any strides; fp64 arithmetic, a float32
 *                        row is rounded once at the store.  dpoints0 may be NULL.
 *   status0              NULL, or (inverse only, EDHIP_ERR_INVALID otherwise) uint8 (N).
 *   displacement0        the PREFILTERED control grid, as for edhip_deform_points; EDHIP_FLAG_RAW_DISPLACEMENT is
 *                        refused (EDHIP_ERR_INVALID).
 *   ddisplacement0       NULL, or the grid's shape in a floating-point dtype (EDHIP_ERR_INVALID / EDHIP_ERR_DTYPE).
 *   dinverse_affine0     NULL, or float64 (naxis, naxis + 1).  All three results NULL: EDHIP_ERR_INVALID.
 *   nbatch               at most 65535 (EDHIP_ERR_UNSUPPORTED); sample b's arrays are sample 0's moved by b * stride.
 * Every shape, dtype and flag check answers before any launch.  With N == 0 the requested ddisplacement /
 * dinverse_affine are written as zeros; with nbatch == 0 nothing is launched.
 * Resolution and bit contracts: the sums are accumulated in 64-bit integer fixed point.  Per sample, with N the number
 * of contributing points and max|u|, max|q| taken over them, one contribution to ddisplacement is rounded to a multiple of 2^(e-62), 2^e
 * being the smallest power of two >= 2 N max|u| -- it is resolved to 2^-61 of N max|u| -- and one contribution to
 * dinverse_affine likewise with N max|u| max(1, max|q|).  No cell can overflow, and integer addition is associative:
 * ddisplacement and dinverse_affine are the same bits on a repeated call, for a sample of a batch and the single call
 * on it, after ANY permutation of the points, and eager or replayed from a captured HIP graph.  A row of dpoints
 * depends on that point and the call's arguments alone.  One non-finite cotangent on a contributing point makes
 * every element of that sample's ddisplacement / dinverse_affine NaN (and no other sample's); max|u| = 0 gives exact
 * zeros.  Four launches -- the clearing of the call's scratch (the stream's workspace) and three kernels -- on hip_stream
 * without synchronising; nothing is carried from one call to the next, so a captured graph replays self-contained
 * (warm up once on the capture stream: the workspace is allocated on first use).
 */
int edhip_deform_points_gradient(int inverse, int nbatch,
                                 const edhip_array* positions0, int64_t positions_batch_stride,
                                 const edhip_array* cotangent0, int64_t cotangent_batch_stride,
                                 const edhip_array* status0, int64_t status_batch_stride,
                                 const edhip_array* displacement0, int64_t displacement_batch_stride,
                                 const int64_t* in_len,
                                 const int64_t* output_offset,
                                 int naxis,
                                 const double* affine,
                                 const edhip_array* dpoints0, int64_t dpoints_batch_stride,
                                 const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                 const edhip_array* dinverse_affine0, int64_t dinverse_affine_batch_stride,
                                 uint32_t flags, void* hip_stream,
                                 char* err, size_t errlen);

/*
 * The local differential structure of the coordinate map at arbitrary real positions (no counterpart in the
 * reference): r(q) as edhip_deform_points(inverse = 0) returns it, with its first and second derivatives.  In the
 * notation above, s_k = (ncp_k - 1) / (in_len_k - 1), w' and w'' = (1 - x, 3x - 2, 1 - 3x, x) the derivatives of the
 * cubic weights at the fraction x = cp - floor(cp):
 *   J[i, h, l]    = K[h, l] + sum_taps P[h, m(t)] s_l w'_l prod_{k != l} w_k                      (= d r_h / d q_l)
 *   H[i, h, l, m] = sum_taps P[h, m(t)] (l == m ? s_l^2 w''_l prod_{k != l} w_k
 *                                               : s_l s_m w'_l w'_m prod_{k != l, m} w_k)   (= d^2 r_h / d q_l d q_m)
 * H is symmetric in (l, m), bit for bit, and does not depend on K.  result0 and jacobian0 are the bits
 * edhip_deform_points writes (the same device code).  r is C2: H is continuous and piecewise linear, its derivative
 * jumps at the knots.
 *   points0 / result0    (N, naxis), float32 or float64 each, any strides.  N = 0 launches nothing.
 *   displacement0        the PREFILTERED control grid (naxis, ncp_0, ...), any dtype / strides;
 *                        EDHIP_FLAG_RAW_DISPLACEMENT is refused (EDHIP_ERR_INVALID).
 *   in_len, output_offset, affine   as for edhip_deform_points (in_len >= 2 each).
 *   naxis                1 to 3 (EDHIP_ERR_UNSUPPORTED beyond).
 *   jacobian0            NULL, or float64 (N, naxis, naxis), any strides.
 *   hessian0             NULL (the second-derivative sweep is skipped), or float64 (N, naxis, naxis, naxis).
 *   nbatch               at most 65535; the batch is described as for edhip_deform_points.
 * A position that is not finite, or whose control coordinate reaches 4e15, gives NaN in r, J and H; nothing is read out
 * of range.  Every shape and dtype check answers before any launch.  One launch, one thread per point, no atomics: a
 * point's result depends on that point and the call's arguments alone.  No workspace, no synchronisation: the call
 * can be captured into a HIP graph.
 */
int edhip_deform_points_derivatives(int nbatch,
                                    const edhip_array* points0, int64_t points_batch_stride,
                                    const edhip_array* displacement0, int64_t displacement_batch_stride,
                                    const int64_t* in_len,
                                    const int64_t* output_offset,
                                    int naxis,
                                    const double* affine,
                                    const edhip_array* result0, int64_t result_batch_stride,
                                    const edhip_array* jacobian0, int64_t jacobian_batch_stride,
                                    const edhip_array* hessian0, int64_t hessian_batch_stride,
                                    uint32_t flags, void* hip_stream,
                                    char* err, size_t errlen);

/*
 * The adjoint of edhip_deform_points_derivatives.  With the cotangents u[i, :] = dL / d r(q_i), A[i] = dL / d J(q_i),
 * G[i] = dL / d H(q_i) (any of them NULL; G need not be symmetric), beta(q, j) the folded tap-weight products of
 * edhip_deform_points_gradient and T[h, l, m, p] = d H[h, l, m] / d q_p (the cubic's third-derivative weights
 * (-1, 3, -3, 1) s^3 are constant per knot cell; the cell is that of floor(cp)):
 *   ddisplacement[h, j]  = sum_i ( u[i,h] beta(q_i, j) + sum_l A[i,h,l] d_l beta(q_i, j)
 *                                  + sum_lm G[i,h,l,m] d_l d_m beta(q_i, j) )                      (= dL / dP)
 *   dinverse_affine[h, l < naxis] = sum_i ( u[i,h] q_i[l] + A[i,h,l] ),   [h, naxis] = sum_i u[i,h]
 *   dpoints[i, p]        = sum_h u[i,h] J[h,p] + sum_hl A[i,h,l] H[h,l,p] + sum_hlm G[i,h,l,m] T[h,l,m,p]
 * ddisplacement is the gradient with respect to the PREFILTERED grid; the caller applies the transposed prefilter.
 * A position that is not finite or whose control coordinate reaches 4e15 contributes nothing: a zero row, its
 * cotangents ignored.
 *   positions0 / dpoints0   (N, naxis), float32 or float64 each, any strides.
 *   dresult0 / djacobian0 / dhessian0   NULL, or (N, naxis) / (N, naxis, naxis) / (N, naxis, naxis, naxis), float32
 *                        or float64 each.  All three NULL: EDHIP_ERR_INVALID.
 *   displacement0, in_len, output_offset, affine, naxis (1 to 3), nbatch (at most 65535): as for the forward call.
 *   dpoints0 / ddisplacement0 / dinverse_affine0   NULL or as for edhip_deform_points_gradient; all three NULL:
 *                        EDHIP_ERR_INVALID.
 * Every shape, dtype and flag check answers before any launch.  With N == 0 the requested ddisplacement /
 * dinverse_affine are written as zeros; with nbatch == 0 nothing is launched.
 * Resolution and bit contracts, those of edhip_deform_points_gradient: the sums are 64-bit integer fixed point.  Per
 * sample, over the N contributing points, bP = max_{i,h} |u_h| + 1.5 sum_l s_l |A_hl| + sum_lm c_lm s_l s_m |G_hlm|
 * (c_ll = 4, c_lm = 2.25) bounds what one point adds to one cell of ddisplacement, and bK = max_{i,h} max(|u_h|,
 * max_l |u_h q_l| + |A_hl|) what it adds to one of dinverse_affine; a contribution is rounded to a multiple of
 * 2^(e-62), 2^e the smallest power of two >= 2 N bP (2 N bK).  No cell can overflow and integer addition is
 * associative: the two sums are the same bits on a repeated call, for a sample of a batch and the single call on it,
 * after ANY permutation of the points, and eager or replayed from a captured HIP graph.  A row of dpoints depends on
 * that point and the call's arguments alone.  One non-finite cotangent on a contributing point makes every element of
 * that sample's ddisplacement / dinverse_affine NaN (and no other sample's).  Four launches -- the clearing of the
 * call's scratch (the stream's workspace) and three kernels -- on hip_stream without synchronising; nothing is carried
 * from one call to the next (warm up once on the capture stream: the workspace is allocated on first use).
 */
int edhip_deform_points_derivatives_gradient(int nbatch,
                                             const edhip_array* positions0, int64_t positions_batch_stride,
                                             const edhip_array* dresult0, int64_t dresult_batch_stride,
                                             const edhip_array* djacobian0, int64_t djacobian_batch_stride,
                                             const edhip_array* dhessian0, int64_t dhessian_batch_stride,
                                             const edhip_array* displacement0, int64_t displacement_batch_stride,
                                             const int64_t* in_len,
                                             const int64_t* output_offset,
                                             int naxis,
                                             const double* affine,
                                             const edhip_array* dpoints0, int64_t dpoints_batch_stride,
                                             const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                             const edhip_array* dinverse_affine0,
                                             int64_t dinverse_affine_batch_stride,
                                             uint32_t flags, void* hip_stream,
                                             char* err, size_t errlen);

/*
 * Label-aware linear resampling of label maps (no counterpart in the reference, whose order-1 interpolation of an
 * integer map interpolates the label NUMBERS).  For a label map L, with the classes being the distinct values of L
 * together with cval, the score of class c is the reference's own float64 order-1 result on the one-hot channel,
 *   s_c = DeformGrid((L == c) as float64, order = 1, mode, cval = 1.0 if c == cval else 0.0, same geometry),
 * and the result at output voxel o is the class with the largest s_c(o); ON A TIE THE NUMERICALLY SMALLEST LABEL
 * WINS.  `weight0`, when given, receives the winning score rounded once to float32: it lies in [2^-naxis, 1] and is
 * 1.0 where a 'constant' voxel outside the array takes cval.  The result equals that definition BIT FOR BIT, ties
 * included: per output voxel the 2^naxis order-1 weight products (1.0 * w_0 * ... * w_{naxis-1}, formed in axis order)
 * are added per distinct label among the 2^naxis source voxels in the reference's tap order (lexicographic, last axis
 * fastest; deform.c:843-901), the coordinate comes from the reference-order fp64 evaluation (deform.c:650-824, no
 * FMA), so every compared score has the bits of the one-hot channel's reference value.  One gather pass over the
 * integer map: no one-hot volumes, no prefilter of the map.
 * The batch is described once, as for edhip_deform_batch_strided: sample b's map, control grid, result and weight
 * are sample 0's moved by b * stride bytes (nbatch = 1: a single call); everything else is shared.
 *   input0 / output0     the label map and the result: one dtype, integer or bool (EDHIP_ERR_INVALID otherwise), any
 *                        strides; labels are compared as raw integers of their own width (int64 / uint64 values
 *                        beyond 2^53 stay distinct), signed or unsigned by dtype.
 *   displacement0        the PREFILTERED control grid (naxis, ncp_0, ...), any dtype / strides.
 *                        EDHIP_FLAG_RAW_DISPLACEMENT is refused (EDHIP_ERR_INVALID): the caller prefilters.
 *   weight0              NULL, or float32 with the output's shape (EDHIP_ERR_INVALID / EDHIP_ERR_DTYPE), any strides.
 *   naxis, axis          1 to 3 deformed axes (more: EDHIP_ERR_UNSUPPORTED), ascending; the other axes are carried
 *                        along as in edhip_deform.  A deformed axis of length < 2 is refused as edhip_deform refuses it.
 *   mode, cval           enum edhip_mode; cval must be an integer value the dtype can represent (EDHIP_ERR_INVALID).
 *   output_offset, affine  as for edhip_deform.
 * Every check answers before any launch.  One launch, one thread per (output voxel, step), no atomics: a voxel's
 * result depends on the call's arguments alone (a sample of a batch and a repeated call give the same bits).  The call
 * enqueues on hip_stream, never synchronises and uses no workspace, so it can be captured into a HIP graph.
 */
int edhip_deform_labels(int nbatch,
                        const edhip_array* input0, int64_t input_batch_stride,
                        const edhip_array* displacement0, int64_t displacement_batch_stride,
                        const int64_t* output_offset,
                        const edhip_array* output0, int64_t output_batch_stride,
                        const edhip_array* weight0, int64_t weight_batch_stride,
                        int naxis, const int32_t* axis,
                        int32_t mode, double cval,
                        const double* affine,
                        uint32_t flags, void* hip_stream,
                        char* err, size_t errlen);

/*
 * An image carried back through the deformation: the image-side counterpart of edhip_deform_points(inverse) (no
 * counterpart in the reference: the inverse of a B-spline field is not a B-spline field).  The forward call is a pull
 * warp, Y[o] = X(r(o)) with X of deformed extents in_len and Y of deformed extents O (in_len, or the crop's shape).
 * For every integer source position p in [0, in_len):
 *   q(p)        the solution of r(q) = p exactly as edhip_deform_points(inverse = 1) defines it: the same start
 *               q0 = M (p - offset - K[:, naxis]), damped Newton step, halvings, tol and max_iter; q is crop-local, a
 *               real position in Y.
 *   Z[p, step]  = S_Y(q(p))[step]: the gather edhip_deform applies to its input at a source coordinate, on the array
 *               input0 with extents O -- the boundary map of `mode` per axis, the (order + 1)-wide window with mirrored
 *               edge taps, the B-spline weights, the fp64 tap sum in the reference's tap order (deform.c:841-924, no
 *               FMA) and the per-dtype store (deform.c:292-306,906-919).  A 'constant' coordinate outside [0, O_k - 1]
 *               gives cval.  Where the iteration does not solve (edhip_deform_points: NaN, status 0), Z = cval in
 *               EVERY mode.
 *   valid[p]    1 exactly when q was solved and 0 <= q_k <= O_k - 1 on every axis (Z is interpolated from inside
 *               input0 there), else 0.
 * The solve happens once per voxel; every step (non-deformed position) of that voxel reuses q, the taps and weights.
 * The batch is described once, as for edhip_deform_batch_strided: sample b's input, control grid, output and valid
 * are sample 0's moved by b * stride bytes (nbatch = 1: a single call); everything else is shared.
 *   input0               Y: any dtype but the 16-bit floats (EDHIP_ERR_DTYPE), any strides; spline coefficients when
 *                        order > 1 (the caller prefilters, as for edhip_deform).  Deformed axes shorter than 2 are
 *                        refused (EDHIP_ERR_INVALID).
 *   displacement0        the PREFILTERED control grid (naxis, ncp_0, ...), any dtype / strides.
 *                        EDHIP_FLAG_RAW_DISPLACEMENT is refused (EDHIP_ERR_INVALID): the caller prefilters.
 *   in_len               host int64[naxis]: the deformed extents of X, hence of output0 (>= 2 each).
 *   output0              Z: input0's dtype (EDHIP_ERR_DTYPE) and non-deformed axes, deformed extents in_len
 *                        (EDHIP_ERR_INVALID), any strides.
 *   valid0               NULL, or uint8 with output0's deformed shape (in_len): EDHIP_ERR_INVALID / EDHIP_ERR_DTYPE.
 *   naxis, axis          1 to 3 deformed axes (more: EDHIP_ERR_UNSUPPORTED), ascending; the other axes are carried
 *                        along as in edhip_deform.
 *   order, mode, cval    0..5, enum edhip_mode, the constant: of the gather on input0.
 *   output_offset, affine  as for edhip_deform: the forward call's own.
 *   forward_linear       M = (K[:, :naxis])^-1, host double[naxis * naxis] row-major; NULL with a NULL affine.
 *   max_iter, tol        >= 1 and > 0 (EDHIP_ERR_INVALID).
 * Every shape, dtype and flag check answers before any launch.  One launch, one thread per source voxel, no atomics:
 * a voxel's result depends on the call's arguments alone (a sample of a batch and a repeated call give the same
 * bits).  The call enqueues on hip_stream, never synchronises and uses no workspace, so it can be captured into a
 * HIP graph.
 */
int edhip_deform_inverse(int nbatch,
                         const edhip_array* input0, int64_t input_batch_stride,
                         const edhip_array* displacement0, int64_t displacement_batch_stride,
                         const int64_t* in_len,
                         const int64_t* output_offset,
                         const edhip_array* output0, int64_t output_batch_stride,
                         const edhip_array* valid0, int64_t valid_batch_stride,
                         int naxis, const int32_t* axis,
                         int32_t order, int32_t mode, double cval,
                         const double* affine,
                         const double* forward_linear,
                         int max_iter, double tol,
                         uint32_t flags, void* hip_stream,
                         char* err, size_t errlen);

/*
 * The adjoint of edhip_deform_inverse with respect to its input (no counterpart in the reference).  For fixed
 * deformation arguments and cval = 0, Z = edhip_deform_inverse(Y) is linear in Y: Z[p, step] = sum_j A[p, j] Y[j, step],
 * the row A[p, :] holding the (order + 1)^naxis products of tap weights at q(p); taps that the mirror edge rule folds
 * onto one cell add up.  The row is empty where p is not solved, and where the mode is 'constant' and q(p) lies
 * outside Y.  This call ADDS A^T dZ into dinput0:
 *   dinput0[j, step] += sum_p A[p, j] cotangent0[p, step].
 * The caller zeroes dinput0 beforehand and, for order > 1, applies the transposed prefilter along the deformed axes
 * afterwards (edhip_spline_filter_axes with transpose) -- as it prefilters Y before edhip_deform_inverse.  cval plays
 * no part; the control grid and the affine map get theirs from edhip_deform_inverse_transform_gradient.  The solve (start, step, halvings, tol, max_iter)
 * and the taps and weights are those of edhip_deform_inverse: the same device code.
 * Arguments as for edhip_deform_inverse, except:
 *   cotangent0           dZ, read: float32 / float64 (anything else: EDHIP_ERR_DTYPE), deformed extents in_len
 *                        (EDHIP_ERR_INVALID), any strides.  Takes the place of output0.
 *   dinput0              the accumulator dY, added into: cotangent0's dtype (EDHIP_ERR_DTYPE) and non-deformed axes,
 *                        deformed extents O (>= 2 each: EDHIP_ERR_INVALID), any strides.  Takes the place of input0.
 *   (no valid0, no cval)
 * The products are formed in fp64 and rounded once to the accumulator's type; the adds are device-scope float atomics
 * in that type.  Which cell receives which product is fixed by the arguments, but the ORDER in which the adds arrive
 * is not: the last bits of a sum may differ from call to call, and between a sample of a batch and the single call
 * (the caveat of the float64 gradient of edhip_deform).  Sums of exactly representable terms (order 0 with integer
 * cotangents) are exact and reproducible.  No add leaves dinput0, whatever the coordinate.
 * Every shape, dtype and flag check answers before any launch.  One launch, one thread per source voxel.  The call
 * enqueues on hip_stream, never synchronises and uses no workspace, so it can be captured into a HIP graph.
 */
int edhip_deform_inverse_gradient(int nbatch,
                                  const edhip_array* cotangent0, int64_t cotangent_batch_stride,
                                  const edhip_array* displacement0, int64_t displacement_batch_stride,
                                  const int64_t* in_len,
                                  const int64_t* output_offset,
                                  const edhip_array* dinput0, int64_t dinput_batch_stride,
                                  int naxis, const int32_t* axis,
                                  int32_t order, int32_t mode,
                                  const double* affine,
                                  const double* forward_linear,
                                  int max_iter, double tol,
                                  uint32_t flags, void* hip_stream,
                                  char* err, size_t errlen);

/*
 * The gradient of edhip_deform_inverse with respect to the deformation: the prefiltered control grid P and the inverse
 * map K (no counterpart in the reference).  For L = sum_{p, step} cotangent0[p, step] Z[p, step] with
 * Z = edhip_deform_inverse(Y), per source voxel p with solved q = q(p), r(q) = p:
 *   g_h(p) = sum_step cotangent0[p, step] m'_h sum_k C[k, step] w'_h(m_h, k_h) prod_{e != h} w_e(m_e, k_e)
 * (C = input0, the coefficients of Y with deformed extents O; m_h = the boundary map of q_h on O_h and m'_h its slope;
 * w, w' the tap weights and their derivatives on the window edhip_deform_inverse samples: dL/dq), and by the implicit
 * function theorem at the solved q
 *   u(p) = -J(q)^-T g(p)                                     J = dr/dq
 *   ddisplacement0[h, j]       = sum_p u_h(p) beta(q(p), j)  (beta: the folded cubic tap-weight products)
 *   dinverse_affine0[h, l < n] = sum_p u_h(p) q_l(p)         dinverse_affine0[h, n] = sum_p u_h(p).
 * ddisplacement0 is the gradient of the PREFILTERED grid: the caller applies the transposed order-3 grid prefilter
 * (edhip_spline_filter_axes with transpose) for the gradient of the raw displacement.
 * A voxel contributes nothing where it is not solved, where the mode is 'constant' and q lies outside Y (Z = cval
 * there), and where J is singular.  Where 'nearest' clamps an axis that axis has slope 0.  At a window change (order 1
 * at integer q_h; orders >= 2 are C^1) the derivative is the one-sided one of the window the forward picks.  Order 0
 * is piecewise constant: both results are exact zeros.
 * Arguments as for edhip_deform_inverse, except:
 *   input0               the coefficients of Y, read: float32 / float64 (anything else: EDHIP_ERR_DTYPE), deformed
 *                        extents O (>= 2 each: EDHIP_ERR_INVALID), any strides.
 *   cotangent0           dZ, read: input0's dtype (EDHIP_ERR_DTYPE) and non-deformed axes, deformed extents in_len
 *                        (EDHIP_ERR_INVALID), any strides.  Takes the place of output0.
 *   ddisplacement0       NULL or displacement0's shape (EDHIP_ERR_INVALID), a floating dtype (EDHIP_ERR_DTYPE).
 *   dinverse_affine0     NULL or float64 (EDHIP_ERR_DTYPE) of shape (naxis, naxis + 1) (EDHIP_ERR_INVALID).
 *                        Both NULL: EDHIP_ERR_INVALID.
 *   (no valid0, no cval; EDHIP_FLAG_RAW_DISPLACEMENT is refused: EDHIP_ERR_INVALID)
 * All arithmetic is fp64 whatever the dtype (float32 is widened at the load).  The solve, the taps and the weights are
 * those of edhip_deform_inverse: the same device code.  The sums over the voxels are those of
 * edhip_deform_points_gradient -- 64-bit integer fixed point, one contribution resolved to 2^-61 of N max|u| -- and
 * keep its contracts: a repeated call gives the same bits; a sample of a batch gives the bits of the single call on it;
 * eager execution and the replay of a captured graph give the same bits; one non-finite cotangent (or coefficient) on
 * a contributing voxel makes that sample's results NaN and no other sample's; max|u| = 0 gives exact zeros.
 * Every shape, dtype and flag check answers before any launch.  Four launches (clear, the per-voxel kernel, scatter,
 * finish; order 0: clear and finish).  Workspace, from the stream's cached scratch: per sample
 * 4 + naxis (naxis + 1) + naxis prod ncp 64-bit words, plus 2 * naxis * 8 bytes per source voxel for the fp64 rows of u
 * and q -- 48 bytes per voxel with three deformed axes, about 100 MB for 128^3.  The call enqueues on hip_stream and
 * never synchronises; once a warm-up call has sized the workspace it can be captured into a HIP graph.
 */
int edhip_deform_inverse_transform_gradient(int nbatch,
                                            const edhip_array* input0, int64_t input_batch_stride,
                                            const edhip_array* cotangent0, int64_t cotangent_batch_stride,
                                            const edhip_array* displacement0, int64_t displacement_batch_stride,
                                            const int64_t* in_len,
                                            const int64_t* output_offset,
                                            const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                            const edhip_array* dinverse_affine0, int64_t dinverse_affine_batch_stride,
                                            int naxis, const int32_t* axis,
                                            int32_t order, int32_t mode,
                                            const double* affine,
                                            const double* forward_linear,
                                            int max_iter, double tol,
                                            uint32_t flags, void* hip_stream,
                                            char* err, size_t errlen);

/*
 * det J of the coordinate map on the voxel lattice (deform_jacobian.hip): for every integer crop-local output
 * position o of a strided batch, det0[o] = det J(o) with J the Jacobian edhip_deform_points returns at q = o,
 *   J[h,l](o) = K[h,l] + (ncp_l - 1) / (I_l - 1) sum_t P[h, m(t)] w'_l prod_{k != l} w_k.
 * No positions are read and no coordinates formed: the axes other than the last are contracted once per row of the
 * last deformed axis, every voxel then does 4 taps per entry of J.
 *   nbatch, displacement0, displacement_batch_stride, in_len, output_offset, naxis, affine
 *                        as for edhip_deform_points (the PREFILTERED grid; EDHIP_FLAG_RAW_DISPLACEMENT is refused);
 *                        naxis 1..3 (more: EDHIP_ERR_UNSUPPORTED); in_len >= 2 on every axis (EDHIP_ERR_INVALID).
 *   det0                 written: one dimension per deformed axis (EDHIP_ERR_INVALID) -- its extents are the crop
 *                        box's --, float32 / float64 (EDHIP_ERR_DTYPE), any strides.  fp64 arithmetic, a float32
 *                        value is rounded once.
 * det0[o] depends on o + output_offset and the call's arguments only: a crop gives the bits of the whole lattice at
 * those voxels, a sample of a batch the bits of the single call, a repeated call and a graph replay the same bits.
 * One launch, no workspace, no synchronisation; can be captured into a HIP graph.
 */
int edhip_deform_jacobian(int nbatch,
                          const edhip_array* displacement0, int64_t displacement_batch_stride,
                          const int64_t* in_len,
                          const int64_t* output_offset,
                          int naxis,
                          const double* affine,
                          const edhip_array* det0, int64_t det_batch_stride,
                          uint32_t flags, void* hip_stream,
                          char* err, size_t errlen);

/*
 * The adjoint of edhip_deform_jacobian: for L with ddet0 = dL / d det (the shape of det0, float32 / float64), and C(o)
 * the cofactor matrix of J(o) (d det / dJ = C, also where det = 0),
 *   ddisplacement0[h, j]     = sum_o ddet0[o] sum_l C[h,l](o) d_l beta_j(o)     (the gradient of the PREFILTERED grid)
 *   dinverse_affine0[h, l<n] = sum_o ddet0[o] C[h,l](o),    dinverse_affine0[h, n] = 0.
 *   ddisplacement0       NULL or displacement0's shape (EDHIP_ERR_INVALID), float32 / float64 (EDHIP_ERR_DTYPE).
 *   dinverse_affine0     NULL or float64 (EDHIP_ERR_DTYPE) of shape (naxis, naxis + 1) (EDHIP_ERR_INVALID).
 *                        Both NULL: EDHIP_ERR_INVALID.
 * Grids of any size are served: a row is cut into units of at most 256 voxels, each reaching a window of the last
 * axis' control points only, and a fine last axis takes more units a row.
 * Every sum runs in fp64 in an order fixed by the shapes, without atomics: per piece of a row over x, then over the
 * rows of a plane, then over the planes.  A repeated call, a graph replay and a sample of a batch give the bits of
 * the single call.  Two to three launches.  Workspace, from the stream's cached scratch: per sample
 * rows * nch * (naxis^2 w + naxis^2) doubles for nch units a row that reach at most w control points each (about
 * naxis^2 (ncp_last + 7 nch) doubles a row), with three axes plus O_0 * (2 naxis ncp_1 ncp_2 + naxis^2) doubles: for
 * 256^3, 27 MiB on a 5^3 grid, about 180 MB with 16 points along the last axis, 300 MB with 32, 520 MB with 64.  It
 * stays cached with the stream until edhip_release_scratch.  The call enqueues on hip_stream
 * and never synchronises; once a warm-up call has sized the workspace it can be captured into a HIP graph.
 */
int edhip_deform_jacobian_gradient(int nbatch,
                                   const edhip_array* ddet0, int64_t ddet_batch_stride,
                                   const edhip_array* displacement0, int64_t displacement_batch_stride,
                                   const int64_t* in_len,
                                   const int64_t* output_offset,
                                   int naxis,
                                   const double* affine,
                                   const edhip_array* ddisplacement0, int64_t ddisplacement_batch_stride,
                                   const edhip_array* dinverse_affine0, int64_t dinverse_affine_batch_stride,
                                   uint32_t flags, void* hip_stream,
                                   char* err, size_t errlen);

/*
 * The deformed image at arbitrary real output positions (deform_sample.hip; no counterpart in the reference): what
 * joins edhip_deform to edhip_deform_points.  q is a real, crop-local output position of an edhip_deform call with the
 * same control grid, crop offset and inverse map.
 *   r(q)          exactly what edhip_deform_points(inverse = 0) returns: the same device code, fp64, no boundary map.
 *   V[i, step]  = S_X(r(q_i))[step], S_X the gather edhip_deform applies to its input at a source coordinate, on the
 *                 array X = input0 with the deformed extents in_len (the code edhip_deform_inverse runs on Y):
 *                 map_coordinate of `mode` per axis, the (order + 1)-wide window with mirrored edge taps,
 *                 spline_weights, the fp64 tap sum in the reference's tap order with no FMA (deform.c:841-924) and the
 *                 per-dtype store.  A 'constant' coordinate outside [0, I_k - 1] gives cval.  A position that is not
 *                 finite, or so far out that |control coordinate| >= 4e15, gives cval in EVERY mode and contributes
 *                 nothing to any gradient.
 *   inside[i]     1 exactly when the position is sane and 0 <= r_k <= I_k - 1 on every axis, else 0.
 * At integer q this is the voxel edhip_deform computes, to the rounding of the coordinate: the points code and the
 * image kernels agree to about 1e-10 there, so the values are equal within that times the interpolant's slope, not
 * bit-equal.
 * The batch is described once: sample b's input, points, control grid, output and inside are sample 0's moved by
 * b * stride bytes (nbatch = 1: a single call); everything else is shared.
 *   input0               X: any dtype but the 16-bit floats (EDHIP_ERR_DTYPE), any strides; spline coefficients when
 *                        order > 1 (the caller prefilters, as for edhip_deform).
 *   points0              (N, naxis), float32 / float64 (EDHIP_ERR_DTYPE), any strides.
 *   displacement0        the PREFILTERED control grid (naxis, ncp_0, ...), any dtype / strides.
 *                        EDHIP_FLAG_RAW_DISPLACEMENT is refused (EDHIP_ERR_INVALID).
 *   in_len               host int64[naxis]: the deformed extents of input0 (>= 2 each: EDHIP_ERR_INVALID).
 *   output0              V: input0's dtype (EDHIP_ERR_DTYPE); input0's dimensions with the deformed axes replaced by
 *                        ONE axis of length N at the position of the first deformed axis (EDHIP_ERR_INVALID), any
 *                        strides.
 *   inside0              NULL, or uint8 (EDHIP_ERR_DTYPE) of shape (N) (EDHIP_ERR_INVALID).
 *   naxis, axis          1 to 3 deformed axes of input0 (more: EDHIP_ERR_UNSUPPORTED), ascending.
 *   order, mode, cval    0..5, enum edhip_mode, the constant.
 *   output_offset, affine  as for edhip_deform: the forward call's own.
 * nbatch <= 65535 (EDHIP_ERR_UNSUPPORTED).  N == 0 or nbatch == 0 launches nothing.  Every shape, dtype and flag check
 * answers before any launch.  One launch, one thread per point (a grid-stride loop beyond 2048 * 256 points a sample),
 * the control grid in LDS up to 7680 values; no atomics and no workspace: a point's result depends on that point and
 * the call's arguments alone (a sample of a batch, a slice or permutation of the points and a repeated call give the
 * same bits).  The call enqueues on hip_stream, never synchronises, never reads the environment and can be captured
 * into a HIP graph.
 */
int edhip_deform_sample(int nbatch,
                        const edhip_array* input0, int64_t input_batch_stride,
                        const edhip_array* points0, int64_t points_batch_stride,
                        const edhip_array* displacement0, int64_t displacement_batch_stride,
                        const int64_t* in_len,
                        const int64_t* output_offset,
                        const edhip_array* output0, int64_t output_batch_stride,
                        const edhip_array* inside0, int64_t inside_batch_stride,
                        int naxis, const int32_t* axis,
                        int32_t order, int32_t mode, double cval,
                        const double* affine,
                        uint32_t flags, void* hip_stream,
                        char* err, size_t errlen);

/*
 * The gradients of edhip_deform_sample (deform_sample_grad.hip) for L = sum_{i, step} cotangent0[i, step] V[i, step]:
 * the same front and the same taps per point, two optional results per call.
 *   dinput0       A^T dV ADDED into the accumulator, A the matrix of the call for fixed positions and deformation
 *                 (row i: the (order + 1)^naxis tap-weight products at r(q_i), folded taps added up; empty where the
 *                 position is not sane or the mode is 'constant' and r lies outside X).  Products in fp64, rounded
 *                 once, device-scope float atomics in the accumulator's type.  The caller zeroes dinput0 beforehand
 *                 and applies the transposed prefilter afterwards, as for edhip_deform_inverse_gradient; the caveat is
 *                 the same: the cells are fixed, the order in which the adds arrive is not.
 *   dcoordinate0  g_h(i) = sum_step cotangent0[i, step] m'_h sum_k C[k, step] w'_h prod_{e != h} w_e = dL/dr_h, a
 *                 plain store of an fp64 row per point (C = input0, the coefficients of X; m'_h the slope of the
 *                 boundary map: 0 where 'nearest' clamps; at a window change the one-sided derivative of the chosen
 *                 window; exact zeros at order 0 and for a point that contributes nothing).  Deterministic: a row
 *                 depends on its point alone.
 * The gradients with respect to the positions, the control grid and the inverse map are
 * edhip_deform_points_gradient(inverse = 0) with dcoordinate0 as the cotangent.
 * Arguments as for edhip_deform_sample, except:
 *   input0               NULL, or the coefficients of X: cotangent0's dtype (EDHIP_ERR_DTYPE).  Required with
 *                        dcoordinate0 (EDHIP_ERR_INVALID).  The shape of X is taken from it, or from dinput0.
 *   cotangent0           dV, read: float32 / float64 (EDHIP_ERR_DTYPE), the shape of output0 (EDHIP_ERR_INVALID).
 *   dinput0              NULL, or the accumulator: cotangent0's dtype (EDHIP_ERR_DTYPE), the shape of X.
 *   dcoordinate0         NULL, or float64 (EDHIP_ERR_DTYPE) of shape (N, naxis) (EDHIP_ERR_INVALID).
 *                        Both NULL: EDHIP_ERR_INVALID.
 *   (no inside0, no cval)
 * One launch, no workspace, no synchronisation; can be captured into a HIP graph.
 */
int edhip_deform_sample_gradient(int nbatch,
                                 const edhip_array* input0, int64_t input_batch_stride,
                                 const edhip_array* cotangent0, int64_t cotangent_batch_stride,
                                 const edhip_array* points0, int64_t points_batch_stride,
                                 const edhip_array* displacement0, int64_t displacement_batch_stride,
                                 const int64_t* in_len,
                                 const int64_t* output_offset,
                                 const edhip_array* dinput0, int64_t dinput_batch_stride,
                                 const edhip_array* dcoordinate0, int64_t dcoordinate_batch_stride,
                                 int naxis, const int32_t* axis,
                                 int32_t order, int32_t mode,
                                 const double* affine,
                                 uint32_t flags, void* hip_stream,
                                 char* err, size_t errlen);

/*
 * Frees the scratch workspaces the library caches per (device, stream): per-call tables, spill
 * lists, the fp64 line buffers of the exact prefilter and the dense temporary of the order-4/5
 * cascade (up to the size of the largest array filtered that way).  Waits for the owning devices to
 * go idle first.  Later calls allocate again on demand.  Must not run concurrently with other
 * calls into the library.
 */
int edhip_release_scratch(void);

/*
 * Measurement aid (bench.py): with profiling enabled, edhip_deform brackets the launch of its
 * dominant kernel -- the LDS-tiled forward / gradient kernel over all strips, without the tables
 * kernel and the spill passes -- with HIP events recorded on `hip_stream`.
 * edhip_profile_last_us() waits for the most recent such launch of the calling thread and returns
 * its duration in microseconds (-1 if there is none).  Off by default; no effect on results.
 */
int edhip_profile_dominant(int enable);
double edhip_profile_last_us(void);

/*
 * Bounding box of the source coordinates of a call: for every deformed axis h,
 *   box[2h]   = floor(min c_h),   box[2h+1] = ceil(max c_h)
 * over all output voxels, where c_h = affine(o)_h + offset_h + displacement_h(o) is the source
 * coordinate of deform.c:771-781 BEFORE the boundary map (values are clamped to +-1e9).  The
 * arguments have the meaning they have in edhip_deform; in_len / out_len (host int64[naxis]) are
 * the deformed extents of inputs[0] / outputs[0].  The box is returned to the host, so this call
 * SYNCHRONISES `hip_stream`.  Control grids of more than 7680 values (naxis * prod ncp) are
 * refused with EDHIP_ERR_UNSUPPORTED.  With EDHIP_FLAG_FAST the box is the conservative one of the
 * spline's convex hull -- [min, max] of the control coefficients that reach the output box, refined by up
 * to two levels of B-spline subdivision, plus the affine part at the box's corners: a superset of the exact
 * box (about 1.2x the displacement's true range for a random 5^3 grid; the unrefined hull is 9x), computed
 * from the control grid alone in microseconds, where the exact scan visits every output voxel.
 *
 * No counterpart in the reference.  It lets the host layer restrict the input prefilter
 * (deform_grid.py:155-164) to the part of a volume that a cropped output can reach.
 */
int edhip_source_box(const edhip_array* displacement,
                     const int64_t* in_len, const int64_t* out_len,
                     const int64_t* output_offset, int naxis, const double* affine,
                     uint32_t flags, void* hip_stream,
                     int64_t* box,
                     char* err, size_t errlen);

/*
 * One-dimensional B-spline prefilter along `axis`, mirror boundary.
 *   transpose == 0 : scipy.ndimage.spline_filter1d(input, order, axis, output, mode='mirror')
 *                    (call sites deform_grid.py:160,168,271)
 *   transpose != 0 : its exact adjoint, NI_SplineFilter1DGrad (deform.c:1049-1168)
 * input/output: same shape, any of the 11 dtypes each, may alias (in-place) -- the reference calls
 * it in place from the second axis on (deform_grid.py:158-161,280-283).  order 0/1: plain copy
 * with dtype conversion.  Arithmetic is fp64; the result is rounded to the output dtype once per
 * call, exactly like the reference's double line buffer (deform.c:1106-1162).
 */
int edhip_spline_filter1d(const edhip_array* input, const edhip_array* output,
                          int axis, int order, int transpose,
                          uint32_t flags, void* hip_stream,
                          char* err, size_t errlen);

/*
 * The filter chain of one array in one call: edhip_spline_filter1d along axes[0] from `input` into
 * `output`, then along axes[1..] in place in `output` -- the loop of deform_grid.py:157-162 (forward)
 * and :279-284 (transpose).  input may equal output (every pass in place).  One host call instead of
 * naxes (the per-call host overhead matters for small volumes).
 */
int edhip_spline_filter_axes(const edhip_array* input, const edhip_array* output,
                             int naxes, const int32_t* axes, int order, int transpose,
                             uint32_t flags, void* hip_stream,
                             char* err, size_t errlen);

/*
 * Crop-aware prefilter with the window kept ON THE DEVICE (no read-back, no stream synchronisation).
 * The reference prefilters every input whole before it deforms it (deform_grid.py:155-164) and runs the
 * transposed filter over the whole gradient afterwards (:277-286); with a crop only a box of the input is
 * ever read.  edhip_source_window computes, for ONE input of an edhip_deform call with these displacement /
 * crop / affine arguments, the index window [w0, w1) along each of the input's deformed axes outside which no
 * tap of the output can fall -- the range of the source coordinate (a superset: convex hull of the subdivided
 * control coefficients), the tap window of deform.c:783-813, the boundary mode's clipping or folding
 * (deform.c:47-128: 'nearest' / 'constant' clip, the folding modes keep the whole axis), `margin` samples of
 * filter decay on either side -- and writes 2 * ndim int32 (w0, w1) in the input's dimension order into
 * `window` (DEVICE memory; non-deformed dimensions get (0, shape[d])).  Rows of the last dimension start and
 * end on multiples of `align` elements; a deformed axis keeps at least `minlen` samples.
 * edhip_spline_filter_axes_window is edhip_spline_filter_axes restricted to that window: samples outside it
 * are neither read nor written, lines are filtered as lines of the window's length.  Whole-line tile kernels
 * only (float32 / float64, orders 2 / 3, lines of 64 .. 576 samples): EDHIP_ERR_UNSUPPORTED, with nothing
 * launched, when a pass is outside that envelope -- filter the whole array then.
 */
int edhip_source_window(const edhip_array* displacement, const int64_t* in_len, const int64_t* out_len,
                        const int64_t* output_offset /* naxis or NULL */, int naxis,
                        const double* inv_affine /* naxis*(naxis+1) or NULL */,
                        int ndim, const int64_t* shape /* ndim: the input's extents */,
                        const int32_t* axis /* naxis: the input's deformed dimensions */, int order, int mode,
                        int margin, int align, int minlen, uint32_t flags, void* hip_stream,
                        int32_t* window /* device, 2 * ndim */, char* err, size_t errlen);
int edhip_spline_filter_axes_window(const edhip_array* input, const edhip_array* output, int naxes,
                                    const int32_t* axes, int order, int transpose,
                                    const int32_t* window /* device, 2 * ndim */, uint32_t flags,
                                    void* hip_stream, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif /* EDHIP_H */
