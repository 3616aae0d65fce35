"""
ctypes binding of the C ABI (include/edhip.h) exported by elasticdeform_amd/libedhip.so -- the
hand-written HIP library for gfx950.  This is the Python side of the drop-in boundary: it plays
the role the CPython extension ``_deform_grid`` plays in the reference
(/root/reference/elasticdeform/_deform_grid.c:306-311).

There is NO CPU fallback: if the library is missing or no GPU is visible the product fails loudly.
"""
import ctypes
import os
import threading

import numpy

MAX_DIMS = 8
MAX_AXES = 7

FLAG_AUTO, FLAG_EXACT, FLAG_FAST = 0, 1, 2
FLAG_RAW_DISPLACEMENT = 4      # edhip_deform prefilters the control grid itself (<= 4096 points)
FLAG_GRID_STAYS = 64           # with RAW_DISPLACEMENT: the raw grid of the previous RAW call on the stream, unchanged
FLAG_SCRATCH_INPUT = 128       # edhip_spline_filter_axes: in place on the input, the last pass input -> output
FLAG_STRONG_FIELD = 256        # forward hint: a strong displacement field -> the z-walk route for every geometry it supports
ERR_UNSUPPORTED = 5             # EDHIP_ERR_UNSUPPORTED: legal, outside this build's limits (nothing was launched)
FLAG_KEEP_BOXES = 8            # forward: leave the tiles' bounding boxes for the gradient call that follows
FLAG_USE_BOXES = 16            # gradient: same displacement contents and geometry as that forward call
FLAG_ZERO_GRADIENT = 32        # gradient: the library clears the (dense) accumulators itself before scattering
RAW_DISPLACEMENT_MAX_POINTS = 4096

# enum edhip_dtype
DTYPE_CODES = {
    'bool': 0, 'uint8': 1, 'int8': 2, 'uint16': 3, 'int16': 4, 'uint32': 5, 'int32': 6,
    'uint64': 7, 'int64': 8, 'float32': 9, 'float64': 10,
    # reduced-precision storage: an extension the host layer only uses after an explicit opt-in
    # (the reference rejects half precision, deform.c:742-747)
    'float16': 11, 'bfloat16': 12,
}
REDUCED_DTYPES = ('float16', 'bfloat16')

# enum edhip_status -> the exception class the reference raises for that condition
_STATUS_EXC = {
    1: RuntimeError,   # EDHIP_ERR_INVALID      (PyErr_SetString(PyExc_RuntimeError, ...), _deform_grid.c:121-255)
    2: RuntimeError,   # EDHIP_ERR_DTYPE        ('data type not supported', deform.c:744,891,922)
    3: MemoryError,    # EDHIP_ERR_MEMORY       (PyErr_NoMemory, deform.c:394-398)
    4: RuntimeError,   # EDHIP_ERR_DEVICE
    5: RuntimeError,   # EDHIP_ERR_UNSUPPORTED
}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libedhip.so')

# every symbol include/edhip.h declares
EXPORTS = ('edhip_version', 'edhip_status_string', 'edhip_device_count', 'edhip_deform',
           'edhip_deform_batch', 'edhip_deform_batch_strided', 'edhip_source_box', 'edhip_spline_filter1d',
           'edhip_spline_filter_axes', 'edhip_source_window', 'edhip_spline_filter_axes_window',
           'edhip_release_scratch', 'edhip_profile_dominant',
           'edhip_profile_last_us', 'edhip_deform_displacement_gradient',
           'edhip_deform_displacement_gradient_batch_strided', 'edhip_deform_transform_gradient',
           'edhip_deform_transform_gradient_batch_strided', 'edhip_deform_points', 'edhip_deform_labels',
           'edhip_deform_points_gradient', 'edhip_deform_inverse', 'edhip_deform_inverse_gradient',
           'edhip_deform_inverse_transform_gradient', 'edhip_deform_jacobian', 'edhip_deform_jacobian_gradient',
           'edhip_deform_sample', 'edhip_deform_sample_gradient', 'edhip_deform_points_derivatives',
           'edhip_deform_points_derivatives_gradient')


class EdhipArray(ctypes.Structure):
    """struct edhip_array"""
    _fields_ = [('data', ctypes.c_void_p), ('dtype', ctypes.c_int32), ('ndim', ctypes.c_int32),
                ('shape', ctypes.c_int64 * MAX_DIMS), ('stride_bytes', ctypes.c_int64 * MAX_DIMS)]


_lib = None
_lock = threading.Lock()


def load():
    """Load libedhip.so (once).  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'elasticdeform_amd: %s not found -- build the HIP extension first '
                '(`make -C elasticdeform_amd/csrc` or `python -c "import __graft_entry__ as g; '
                'g.build()"`).  There is no CPU fallback.' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.edhip_version.restype = ctypes.c_int
        L.edhip_version.argtypes = []
        L.edhip_status_string.restype = ctypes.c_char_p
        L.edhip_status_string.argtypes = [ctypes.c_int]
        L.edhip_device_count.restype = ctypes.c_int
        L.edhip_device_count.argtypes = []
        L.edhip_deform.restype = ctypes.c_int
        L.edhip_deform.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.POINTER(EdhipArray),
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(EdhipArray), ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(ctypes.c_double), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p,
            ctypes.c_size_t]
        L.edhip_release_scratch.restype = ctypes.c_int
        L.edhip_release_scratch.argtypes = []
        L.edhip_deform_batch.restype = ctypes.c_int
        L.edhip_deform_batch.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.POINTER(EdhipArray),
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(EdhipArray), ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
            ctypes.POINTER(ctypes.c_double), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p,
            ctypes.c_size_t]
        L.edhip_deform_batch_strided.restype = ctypes.c_int
        L.edhip_deform_batch_strided.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
            ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_double),
            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_profile_dominant.restype = ctypes.c_int
        L.edhip_profile_dominant.argtypes = [ctypes.c_int]
        L.edhip_profile_last_us.restype = ctypes.c_double
        L.edhip_profile_last_us.argtypes = []
        L.edhip_source_box.restype = ctypes.c_int
        L.edhip_source_box.argtypes = [
            ctypes.POINTER(EdhipArray), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_double),
            ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_char_p,
            ctypes.c_size_t]
        L.edhip_spline_filter1d.restype = ctypes.c_int
        L.edhip_spline_filter1d.argtypes = [
            ctypes.POINTER(EdhipArray), ctypes.POINTER(EdhipArray), ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_spline_filter_axes.restype = ctypes.c_int
        L.edhip_spline_filter_axes.argtypes = [
            ctypes.POINTER(EdhipArray), ctypes.POINTER(EdhipArray), ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p,
            ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_source_window.restype = ctypes.c_int
        L.edhip_source_window.argtypes = [
            ctypes.POINTER(EdhipArray), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_spline_filter_axes_window.restype = ctypes.c_int
        L.edhip_spline_filter_axes_window.argtypes = [
            ctypes.POINTER(EdhipArray), ctypes.POINTER(EdhipArray), ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_displacement_gradient.restype = ctypes.c_int
        L.edhip_deform_displacement_gradient.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.POINTER(EdhipArray), ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(EdhipArray), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(EdhipArray), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_displacement_gradient_batch_strided.restype = ctypes.c_int
        L.edhip_deform_displacement_gradient_batch_strided.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_uint32,
            ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_transform_gradient.restype = ctypes.c_int
        L.edhip_deform_transform_gradient.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.POINTER(EdhipArray), ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(EdhipArray), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(EdhipArray), ctypes.POINTER(EdhipArray), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p,
            ctypes.c_size_t]
        L.edhip_deform_transform_gradient_batch_strided.restype = ctypes.c_int
        L.edhip_deform_transform_gradient_batch_strided.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_points.restype = ctypes.c_int
        L.edhip_deform_points.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.c_int, ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_points_gradient.restype = ctypes.c_int
        L.edhip_deform_points_gradient.argtypes = [
            ctypes.c_int, ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p,
            ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_points_derivatives.restype = ctypes.c_int
        L.edhip_deform_points_derivatives.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p,
            ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_points_derivatives_gradient.restype = ctypes.c_int
        L.edhip_deform_points_derivatives_gradient.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p,
            ctypes.c_size_t]
        L.edhip_deform_labels.restype = ctypes.c_int
        L.edhip_deform_labels.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_double,
            ctypes.POINTER(ctypes.c_double), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_inverse.restype = ctypes.c_int
        L.edhip_deform_inverse.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
            ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
            ctypes.c_int, ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_inverse_gradient.restype = ctypes.c_int
        L.edhip_deform_inverse_gradient.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double,
            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_inverse_transform_gradient.restype = ctypes.c_int
        L.edhip_deform_inverse_transform_gradient.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p,
            ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_jacobian.restype = ctypes.c_int
        L.edhip_deform_jacobian.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_jacobian_gradient.restype = ctypes.c_int
        L.edhip_deform_jacobian_gradient.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray),
            ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_sample.restype = ctypes.c_int
        L.edhip_deform_sample.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_int,
            ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
            ctypes.POINTER(ctypes.c_double), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.edhip_deform_sample_gradient.restype = ctypes.c_int
        L.edhip_deform_sample_gradient.argtypes = [
            ctypes.c_int, ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(EdhipArray), ctypes.c_int64,
            ctypes.POINTER(EdhipArray), ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
            ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p,
            ctypes.c_size_t]
        _lib = L
    return _lib


def raise_for_status(status, errbuf):
    if status == 0:
        return
    msg = errbuf.value.decode('utf-8', 'replace') if errbuf is not None else ''
    if not msg:
        msg = load().edhip_status_string(status).decode()
    raise _STATUS_EXC.get(status, RuntimeError)(msg)


_I64x8 = ctypes.c_int64 * MAX_DIMS


def describe(data_ptr, dtype_name, shape, strides_bytes):
    """Build a struct edhip_array from raw parts."""
    code = DTYPE_CODES.get(dtype_name)
    if code is None:
        # float16 / complex / ...: what the reference answers for them (deform.c:744,891)
        raise RuntimeError('data type not supported')
    nd = len(shape)
    if nd < 1 or nd > MAX_DIMS:
        raise RuntimeError('arrays must have 1..%d dimensions' % MAX_DIMS)
    return EdhipArray(data_ptr, code, nd, _I64x8(*shape), _I64x8(*strides_bytes))


class DeformArgs(object):
    """The host-side parameter arrays of one edhip_deform call (axis, orders, modes, cvals, crop
    offsets, inverse affine) converted to ctypes once; a cached Plan keeps them, so repeated calls
    with the same arguments skip the NumPy / ctypes conversions."""
    __slots__ = ("n", "naxis", "axis", "orders", "modes", "cvals", "off", "aff")

    def __init__(self, n, axis, orders, modes, cvals, output_offset, inverse_affine):
        axis = numpy.ascontiguousarray(numpy.asarray(axis, dtype=numpy.int32).reshape(n, -1))
        self.n = n
        self.naxis = int(axis.shape[1])
        self.axis = (ctypes.c_int32 * axis.size)(*[int(v) for v in axis.reshape(-1)])
        self.orders = (ctypes.c_int32 * n)(*[int(v) for v in orders])
        self.modes = (ctypes.c_int32 * n)(*[int(v) for v in modes])
        self.cvals = (ctypes.c_double * n)(*[float(v) for v in cvals])
        self.off = None
        if output_offset is not None:
            self.off = (ctypes.c_int64 * len(output_offset))(*[int(v) for v in output_offset])
        self.aff = None
        if inverse_affine is not None:
            flat = numpy.ascontiguousarray(inverse_affine, dtype=numpy.float64).reshape(-1)
            self.aff = (ctypes.c_double * flat.size)(*[float(v) for v in flat])


_errbuf = threading.local()


def _buf():
    b = getattr(_errbuf, "b", None)
    if b is None:
        b = _errbuf.b = ctypes.create_string_buffer(256)
    return b


def deform(gradient, in_descs, disp_desc, output_offset, out_descs, axis, orders, modes, cvals,
           inverse_affine, flags, stream, prepared=None, may_decline=False):
    """edhip_deform -- argument for argument `_deform_grid.deform_grid(_grad)` of the reference
    (_deform_grid.c:108-118) with descriptors in place of arrays, plus flags and the HIP stream.
    `prepared`: a DeformArgs built earlier from the same parameter arrays.  `may_decline`: return
    EDHIP_ERR_UNSUPPORTED (nothing launched) instead of raising; otherwise returns 0."""
    L = load()
    n = len(in_descs)
    a = prepared if prepared is not None else DeformArgs(n, axis, orders, modes, cvals, output_offset,
                                                         inverse_affine)
    ins = (EdhipArray * n)(*in_descs)
    outs = (EdhipArray * n)(*out_descs)
    buf = _buf()
    status = L.edhip_deform(1 if gradient else 0, n, ins, ctypes.byref(disp_desc), a.off, outs, a.naxis,
                            a.axis, a.orders, a.modes, a.cvals, a.aff, int(flags), stream, buf, 256)
    if status and not (may_decline and status == ERR_UNSUPPORTED):
        raise_for_status(status, buf)
    return status


_POINTER = {numpy.int32: ctypes.POINTER(ctypes.c_int32), numpy.int64: ctypes.POINTER(ctypes.c_int64),
            numpy.float64: ctypes.POINTER(ctypes.c_double)}


def _ptr(values, dtype):
    """(typed pointer to `values` as a flat host array of `dtype`, that array) -- (None, None) for None.  The caller
    holds on to the array until its library call has returned."""
    if values is None:
        return None, None
    arr = numpy.ascontiguousarray(values, dtype=dtype).reshape(-1)
    return arr.ctypes.data_as(_POINTER[dtype]), arr


def _offset_affine(output_offset, inverse_affine):
    """(int64 pointer to the crop offsets, double pointer to the inverse affine, the arrays behind them) -- None for
    an argument that is None.  The caller holds on to the third value until its library call has returned."""
    off, off_arr = _ptr(output_offset, numpy.int64)
    aff, aff_arr = _ptr(inverse_affine, numpy.float64)
    return off, aff, (off_arr, aff_arr)


def _call(entry, args, flags, stream):
    """entry(*args, flags, stream, the thread's error buffer, its size); raises what the status stands for"""
    buf = _buf()
    raise_for_status(entry(*args, int(flags), ctypes.c_void_p(stream), buf, 256), buf)


def deform_batch_strided(gradient, nbatch, in_desc, in_bstride, disp_desc, disp_bstride, output_offset,
                         out_desc, out_bstride, axis, order, mode, cval, inverse_affine, flags, stream):
    """edhip_deform_batch_strided: the batch described once -- sample 0's descriptors plus the byte
    distance between consecutive samples of each stacked array."""
    ax, axis = _ptr(axis, numpy.int32)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_batch_strided,
          (int(bool(gradient)), int(nbatch), *_pairs(in_desc, in_bstride, disp_desc, disp_bstride), off,
           *_pairs(out_desc, out_bstride), len(axis), ax, int(order), int(mode), float(cval), aff), flags, stream)


def _ref(desc):
    return ctypes.byref(desc) if desc is not None else None


def _pairs(*flat):
    """descriptor, byte stride, descriptor, byte stride, ... as the C side takes them: each descriptor by reference
    (None: not given / not wanted), each stride an int"""
    return [_ref(v) if i % 2 == 0 else int(v) for i, v in enumerate(flat)]


def _grid_gradient(entry, in_descs, disp_desc, output_offset, dout_descs, axis, orders, modes, cvals, inverse_affine,
                   results, flags, stream, prepared):
    """The list form of the two gradient entry points: `entry` is the C function, `results` its result descriptors
    (by reference), which follow the inverse affine in both signatures."""
    n = len(in_descs)
    a = prepared if prepared is not None else DeformArgs(n, axis, orders, modes, cvals, output_offset,
                                                         inverse_affine)
    ins = (EdhipArray * n)(*in_descs)
    outs = (EdhipArray * n)(*dout_descs)
    buf = _buf()
    status = entry(n, ins, ctypes.byref(disp_desc), a.off, outs, a.naxis, a.axis, a.orders, a.modes, a.cvals, a.aff,
                   *results, int(flags), stream, buf, 256)
    raise_for_status(status, buf)


def _grid_gradient_batch_strided(entry, nbatch, in_desc, in_bstride, disp_desc, disp_bstride, output_offset, dout_desc,
                                 dout_bstride, axis, order, mode, cval, inverse_affine, results, flags, stream):
    """The batch form of the two gradient entry points: `results` are descriptor, byte stride, ... as for _pairs."""
    ax, axis = _ptr(axis, numpy.int32)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(entry, (int(nbatch), *_pairs(in_desc, in_bstride, disp_desc, disp_bstride), off,
                  *_pairs(dout_desc, dout_bstride), len(axis), ax, int(order), int(mode), float(cval), aff,
                  *_pairs(*results)), flags, stream)


def deform_displacement_gradient(in_descs, disp_desc, output_offset, dout_descs, axis, orders, modes, cvals,
                                 inverse_affine, ddisp_desc, flags, stream, prepared=None):
    """edhip_deform_displacement_gradient: d(sum_i <dY_i, Y_i>) / d(displacement) into `ddisp_desc`.  `in_descs`
    are the (prefiltered) inputs the forward read, `dout_descs` the dY arrays; the other arguments as for
    deform()."""
    _grid_gradient(load().edhip_deform_displacement_gradient, in_descs, disp_desc, output_offset, dout_descs, axis,
                   orders, modes, cvals, inverse_affine, (ctypes.byref(ddisp_desc),), flags, stream, prepared)


def deform_displacement_gradient_batch_strided(nbatch, in_desc, in_bstride, disp_desc, disp_bstride, output_offset,
                                               dout_desc, dout_bstride, axis, order, mode, cval, inverse_affine,
                                               ddisp_desc, ddisp_bstride, flags, stream):
    """edhip_deform_displacement_gradient_batch_strided: sample 0's descriptors plus byte strides."""
    _grid_gradient_batch_strided(load().edhip_deform_displacement_gradient_batch_strided, nbatch, in_desc, in_bstride,
                                 disp_desc, disp_bstride, output_offset, dout_desc, dout_bstride, axis, order, mode,
                                 cval, inverse_affine, (ddisp_desc, ddisp_bstride), flags, stream)


def deform_transform_gradient(in_descs, disp_desc, output_offset, dout_descs, axis, orders, modes, cvals,
                              inverse_affine, ddisp_desc, dinv_desc, flags, stream, prepared=None):
    """edhip_deform_transform_gradient: d(sum_i <dY_i, Y_i>) / d(displacement) into `ddisp_desc` and / or
    d(...) / d(inverse map) into `dinv_desc` (float64, naxis x naxis+1); None = not wanted.  Otherwise as
    deform_displacement_gradient()."""
    _grid_gradient(load().edhip_deform_transform_gradient, in_descs, disp_desc, output_offset, dout_descs, axis,
                   orders, modes, cvals, inverse_affine, (_ref(ddisp_desc), _ref(dinv_desc)), flags, stream, prepared)


def deform_transform_gradient_batch_strided(nbatch, in_desc, in_bstride, disp_desc, disp_bstride, output_offset,
                                            dout_desc, dout_bstride, axis, order, mode, cval, inverse_affine,
                                            ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride, flags, stream):
    """edhip_deform_transform_gradient_batch_strided: sample 0's descriptors plus byte strides (None = not wanted)."""
    _grid_gradient_batch_strided(load().edhip_deform_transform_gradient_batch_strided, nbatch, in_desc, in_bstride,
                                 disp_desc, disp_bstride, output_offset, dout_desc, dout_bstride, axis, order, mode,
                                 cval, inverse_affine, (ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride), flags, stream)


def deform_points(inverse, nbatch, pts_desc, pts_bstride, disp_desc, disp_bstride, in_len, output_offset,
                  inverse_affine, forward_linear, res_desc, res_bstride, jac_desc, jac_bstride, status_desc,
                  status_bstride, max_iter, tol, flags, stream):
    """edhip_deform_points: the coordinate map r(q) at the points (inverse false; `jac_desc`: also its Jacobian) or
    the q with r(q) = point (inverse true; `status_desc`: 1 where solved).  Sample 0's descriptors plus byte strides;
    `disp_desc` is the PREFILTERED control grid; None = not wanted / not given."""
    lens, in_len = _ptr(in_len, numpy.int64)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    lin, _lin = _ptr(forward_linear, numpy.float64)
    _call(load().edhip_deform_points,
          (int(bool(inverse)), int(nbatch), *_pairs(pts_desc, pts_bstride, disp_desc, disp_bstride), lens, off,
           len(in_len), aff, lin, *_pairs(res_desc, res_bstride, jac_desc, jac_bstride, status_desc, status_bstride),
           int(max_iter), float(tol)), flags, stream)


def deform_points_gradient(inverse, nbatch, pos_desc, pos_bstride, cot_desc, cot_bstride, status_desc, status_bstride,
                           disp_desc, disp_bstride, in_len, output_offset, inverse_affine, dpts_desc, dpts_bstride,
                           ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride, flags, stream):
    """edhip_deform_points_gradient: the adjoint of deform_points().  `pos_desc`: the positions q (inverse true: the
    solved q), `cot_desc`: dL/dr (inverse true: dL/dq), `status_desc`: inverse only, 0 = not solved.  Results (None =
    not wanted): the per-point rows into `dpts_desc`, the gradient with respect to the PREFILTERED grid `disp_desc`
    into `ddisp_desc`, with respect to the inverse map into `dinv_desc` (float64, naxis x naxis+1).  Sample 0's
    descriptors plus byte strides."""
    lens, in_len = _ptr(in_len, numpy.int64)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_points_gradient,
          (int(bool(inverse)), int(nbatch), *_pairs(pos_desc, pos_bstride, cot_desc, cot_bstride, status_desc,
                                                    status_bstride, disp_desc, disp_bstride), lens, off, len(in_len),
           aff, *_pairs(dpts_desc, dpts_bstride, ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride)), flags, stream)


def deform_jacobian(nbatch, disp_desc, disp_bstride, in_len, output_offset, inverse_affine, det_desc, det_bstride, flags,
                    stream):
    """edhip_deform_jacobian: det J of the coordinate map at every voxel of the crop box into `det_desc` (float32 /
    float64, one dimension per deformed axis).  Sample 0's descriptors plus byte strides; `disp_desc` is the
    PREFILTERED control grid."""
    lens, in_len = _ptr(in_len, numpy.int64)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_jacobian,
          (int(nbatch), *_pairs(disp_desc, disp_bstride), lens, off, len(in_len), aff, *_pairs(det_desc, det_bstride)),
          flags, stream)


def deform_jacobian_gradient(nbatch, ddet_desc, ddet_bstride, disp_desc, disp_bstride, in_len, output_offset,
                             inverse_affine, ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride, flags, stream):
    """edhip_deform_jacobian_gradient: the adjoint of deform_jacobian() for the cotangent `ddet_desc`.  Results (None =
    not wanted): the gradient with respect to the PREFILTERED grid into `ddisp_desc`, with respect to the inverse map
    into `dinv_desc` (float64, naxis x naxis+1)."""
    lens, in_len = _ptr(in_len, numpy.int64)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_jacobian_gradient,
          (int(nbatch), *_pairs(ddet_desc, ddet_bstride, disp_desc, disp_bstride), lens, off, len(in_len), aff,
           *_pairs(ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride)), flags, stream)


def deform_points_derivatives(nbatch, pts_desc, pts_bstride, disp_desc, disp_bstride, in_len, output_offset,
                              inverse_affine, res_desc, res_bstride, jac_desc, jac_bstride, hess_desc, hess_bstride,
                              flags, stream):
    """edhip_deform_points_derivatives: r(q) at the points into `res_desc`, J = dr/dq into `jac_desc` (float64
    (N, naxis, naxis)) and H = d^2r/dq dq into `hess_desc` (float64 (N, naxis, naxis, naxis)); None = not wanted.
    Sample 0's descriptors plus byte strides; `disp_desc` is the PREFILTERED control grid; 1 to 3 deformed axes."""
    lens, in_len = _ptr(in_len, numpy.int64)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_points_derivatives,
          (int(nbatch), *_pairs(pts_desc, pts_bstride, disp_desc, disp_bstride), lens, off, len(in_len), aff,
           *_pairs(res_desc, res_bstride, jac_desc, jac_bstride, hess_desc, hess_bstride)), flags, stream)


def deform_points_derivatives_gradient(nbatch, pos_desc, pos_bstride, dres_desc, dres_bstride, djac_desc, djac_bstride,
                                       dhess_desc, dhess_bstride, disp_desc, disp_bstride, in_len, output_offset,
                                       inverse_affine, dpts_desc, dpts_bstride, ddisp_desc, ddisp_bstride, dinv_desc,
                                       dinv_bstride, flags, stream):
    """edhip_deform_points_derivatives_gradient: the adjoint of deform_points_derivatives() for the cotangents
    `dres_desc` = dL/dr, `djac_desc` = dL/dJ, `dhess_desc` = dL/dH (None = not given).  Results as for
    deform_points_gradient() (None = not wanted)."""
    lens, in_len = _ptr(in_len, numpy.int64)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_points_derivatives_gradient,
          (int(nbatch), *_pairs(pos_desc, pos_bstride, dres_desc, dres_bstride, djac_desc, djac_bstride, dhess_desc,
                                dhess_bstride, disp_desc, disp_bstride), lens, off, len(in_len), aff,
           *_pairs(dpts_desc, dpts_bstride, ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride)), flags, stream)


def deform_labels(nbatch, in_desc, in_bstride, disp_desc, disp_bstride, output_offset, out_desc, out_bstride,
                  weight_desc, weight_bstride, axis, mode, cval, inverse_affine, flags, stream):
    """edhip_deform_labels: label-aware linear resampling of an integer / bool label map into `out_desc` (the label
    with the largest sum of order-1 weights among the 2^naxis source voxels, ties to the smallest label) and, with
    `weight_desc` (float32, the output's shape; None = not wanted), the winning sum.  Sample 0's descriptors plus
    byte strides; `disp_desc` is the PREFILTERED control grid."""
    ax, axis = _ptr(axis, numpy.int32)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_labels,
          (int(nbatch), *_pairs(in_desc, in_bstride, disp_desc, disp_bstride), off,
           *_pairs(out_desc, out_bstride, weight_desc, weight_bstride), len(axis), ax, int(mode), float(cval), aff),
          flags, stream)


def deform_inverse(nbatch, in_desc, in_bstride, disp_desc, disp_bstride, in_len, output_offset, out_desc, out_bstride,
                   valid_desc, valid_bstride, axis, order, mode, cval, inverse_affine, forward_linear, max_iter, tol,
                   flags, stream):
    """edhip_deform_inverse: `in_desc` (the deformed image, spline coefficients for order > 1) resampled back into the
    source frame -- per source voxel the q with r(q) = voxel, solved as deform_points() solves it, and the forward
    gather of `in_desc` at q into `out_desc` (deformed extents `in_len`); `valid_desc` (uint8, shape `in_len`; None =
    not wanted): 1 where q was solved and lies inside `in_desc`.  Sample 0's descriptors plus byte strides; `disp_desc`
    is the PREFILTERED control grid."""
    lens, _lens = _ptr(in_len, numpy.int64)
    ax, axis = _ptr(axis, numpy.int32)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    lin, _lin = _ptr(forward_linear, numpy.float64)
    _call(load().edhip_deform_inverse,
          (int(nbatch), *_pairs(in_desc, in_bstride, disp_desc, disp_bstride), lens, off,
           *_pairs(out_desc, out_bstride, valid_desc, valid_bstride), len(axis), ax, int(order), int(mode),
           float(cval), aff, lin, int(max_iter), float(tol)), flags, stream)


def deform_inverse_gradient(nbatch, cot_desc, cot_bstride, disp_desc, disp_bstride, in_len, output_offset, din_desc,
                            din_bstride, axis, order, mode, inverse_affine, forward_linear, max_iter, tol, flags,
                            stream):
    """edhip_deform_inverse_gradient: the adjoint of deform_inverse() with respect to its input -- `cot_desc` (dZ,
    deformed extents `in_len`, float32 / float64) times the tap weights at the solved positions ADDED into `din_desc`
    (the accumulator, the input's shape, the same dtype) with float atomics.  The caller zeroes `din_desc` and applies
    the transposed prefilter afterwards.  Sample 0's descriptors plus byte strides; `disp_desc` is the PREFILTERED
    control grid."""
    lens, _lens = _ptr(in_len, numpy.int64)
    ax, axis = _ptr(axis, numpy.int32)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    lin, _lin = _ptr(forward_linear, numpy.float64)
    _call(load().edhip_deform_inverse_gradient,
          (int(nbatch), *_pairs(cot_desc, cot_bstride, disp_desc, disp_bstride), lens, off,
           *_pairs(din_desc, din_bstride), len(axis), ax, int(order), int(mode), aff, lin, int(max_iter),
           float(tol)), flags, stream)


def deform_inverse_transform_gradient(nbatch, in_desc, in_bstride, cot_desc, cot_bstride, disp_desc, disp_bstride, in_len,
                                      output_offset, ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride, axis, order,
                                      mode, inverse_affine, forward_linear, max_iter, tol, flags, stream):
    """edhip_deform_inverse_transform_gradient: the gradient of deform_inverse() with respect to the deformation --
    `in_desc` (the deformed image, spline coefficients for order > 1) and `cot_desc` (dZ, deformed extents `in_len`),
    float32 / float64 of one dtype; results (None = not wanted): the gradient of the PREFILTERED control grid into
    `ddisp_desc` (the caller applies the transposed grid prefilter), of the inverse map into `dinv_desc` (float64,
    naxis x naxis+1).  Sample 0's descriptors plus byte strides; `disp_desc` is the PREFILTERED control grid."""
    lens, _lens = _ptr(in_len, numpy.int64)
    ax, axis = _ptr(axis, numpy.int32)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    lin, _lin = _ptr(forward_linear, numpy.float64)
    _call(load().edhip_deform_inverse_transform_gradient,
          (int(nbatch), *_pairs(in_desc, in_bstride, cot_desc, cot_bstride, disp_desc, disp_bstride), lens, off,
           *_pairs(ddisp_desc, ddisp_bstride, dinv_desc, dinv_bstride), len(axis), ax, int(order), int(mode), aff, lin,
           int(max_iter), float(tol)), flags, stream)


def deform_sample(nbatch, in_desc, in_bstride, pts_desc, pts_bstride, disp_desc, disp_bstride, in_len, output_offset,
                  out_desc, out_bstride, inside_desc, inside_bstride, axis, order, mode, cval, inverse_affine, flags,
                  stream):
    """edhip_deform_sample: `in_desc` (the image, spline coefficients for order > 1; deformed extents `in_len`) gathered
    at r(q) for the positions q of `pts_desc` (N, naxis) into `out_desc` (the input's non-deformed axes, one axis of N
    points in the place of the first deformed axis); `inside_desc` (uint8 (N); None = not wanted): 1 where r lies inside
    the input.  Sample 0's descriptors plus byte strides; `disp_desc` is the PREFILTERED control grid."""
    lens, _lens = _ptr(in_len, numpy.int64)
    ax, axis = _ptr(axis, numpy.int32)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_sample,
          (int(nbatch), *_pairs(in_desc, in_bstride, pts_desc, pts_bstride, disp_desc, disp_bstride), lens, off,
           *_pairs(out_desc, out_bstride, inside_desc, inside_bstride), len(axis), ax, int(order), int(mode),
           float(cval), aff), flags, stream)


def deform_sample_gradient(nbatch, in_desc, in_bstride, cot_desc, cot_bstride, pts_desc, pts_bstride, disp_desc,
                           disp_bstride, in_len, output_offset, din_desc, din_bstride, dcoord_desc, dcoord_bstride, axis,
                           order, mode, inverse_affine, flags, stream):
    """edhip_deform_sample_gradient: for the cotangent `cot_desc` (the shape of deform_sample()'s output, float32 /
    float64) the adjoint in the image ADDED into `din_desc` (the accumulator, the image's shape, the cotangent's dtype;
    the caller zeroes it and applies the transposed prefilter afterwards) and / or dL/dr per point into `dcoord_desc`
    (float64 (N, naxis); needs `in_desc`, the image's coefficients in the cotangent's dtype).  None = not given / not
    wanted.  Sample 0's descriptors plus byte strides; `disp_desc` is the PREFILTERED control grid."""
    lens, _lens = _ptr(in_len, numpy.int64)
    ax, axis = _ptr(axis, numpy.int32)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    _call(load().edhip_deform_sample_gradient,
          (int(nbatch), *_pairs(in_desc, in_bstride, cot_desc, cot_bstride, pts_desc, pts_bstride, disp_desc,
                                disp_bstride), lens, off, *_pairs(din_desc, din_bstride, dcoord_desc, dcoord_bstride),
           len(axis), ax, int(order), int(mode), aff), flags, stream)


def source_box(disp_desc, in_len, out_len, output_offset, inverse_affine, flags, stream):
    """edhip_source_box -> int64 array (naxis, 2): floor(min) / ceil(max) of the unmapped source
    coordinate along every deformed axis.  Synchronises the stream."""
    L = load()
    in_len = numpy.ascontiguousarray(in_len, dtype=numpy.int64)
    out_len = numpy.ascontiguousarray(out_len, dtype=numpy.int64)
    naxis = len(in_len)
    p64 = ctypes.POINTER(ctypes.c_int64)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    box = numpy.zeros((naxis, 2), dtype=numpy.int64)
    buf = _buf()
    status = L.edhip_source_box(ctypes.byref(disp_desc), in_len.ctypes.data_as(p64),
                                out_len.ctypes.data_as(p64), off, naxis, aff, int(flags),
                                ctypes.c_void_p(stream), box.ctypes.data_as(p64), buf, 256)
    raise_for_status(status, buf)
    return box


def source_window(disp_desc, in_len, out_len, output_offset, inverse_affine, shape, axis, order, mode,
                  margin, align, minlen, flags, stream, window_ptr):
    """edhip_source_window: the filter window of one input, written to DEVICE memory at `window_ptr`
    (2 * len(shape) int32).  No synchronisation.  Returns the status (0, or EDHIP_ERR_UNSUPPORTED)."""
    L = load()
    in_len = numpy.ascontiguousarray(in_len, dtype=numpy.int64)
    out_len = numpy.ascontiguousarray(out_len, dtype=numpy.int64)
    shape = numpy.ascontiguousarray(shape, dtype=numpy.int64)
    naxis = len(in_len)
    p64 = ctypes.POINTER(ctypes.c_int64)
    off, aff, _keep = _offset_affine(output_offset, inverse_affine)
    buf = _buf()
    status = L.edhip_source_window(ctypes.byref(disp_desc), in_len.ctypes.data_as(p64),
                                   out_len.ctypes.data_as(p64), off, naxis, aff, len(shape),
                                   shape.ctypes.data_as(p64), (ctypes.c_int32 * naxis)(*[int(a) for a in axis]),
                                   int(order), int(mode), int(margin), int(align), int(minlen), int(flags),
                                   ctypes.c_void_p(stream), ctypes.c_void_p(window_ptr), buf, 256)
    if status and status != ERR_UNSUPPORTED:
        raise_for_status(status, buf)
    return status


def spline_filter_axes_window(in_desc, out_desc, axes, order, transpose, window_ptr, flags, stream):
    """edhip_spline_filter_axes_window; returns the status (0, or EDHIP_ERR_UNSUPPORTED with nothing launched)"""
    L = load()
    n = len(axes)
    buf = _buf()
    status = L.edhip_spline_filter_axes_window(ctypes.byref(in_desc), ctypes.byref(out_desc), n,
                                               (ctypes.c_int32 * n)(*axes), int(order), int(bool(transpose)),
                                               ctypes.c_void_p(window_ptr), int(flags), stream, buf, 256)
    if status and status != ERR_UNSUPPORTED:
        raise_for_status(status, buf)
    return status


def spline_filter1d(in_desc, out_desc, axis, order, transpose, flags, stream):
    """edhip_spline_filter1d"""
    L = load()
    buf = _buf()
    status = L.edhip_spline_filter1d(ctypes.byref(in_desc), ctypes.byref(out_desc), int(axis),
                                     int(order), int(bool(transpose)), int(flags), stream, buf, 256)
    if status:
        raise_for_status(status, buf)


def spline_filter_axes(in_desc, out_desc, axes, order, transpose, flags, stream, may_decline=False):
    """edhip_spline_filter_axes: the whole chain (first pass in -> out, the rest in place) in one call.
    `may_decline`: return EDHIP_ERR_UNSUPPORTED (nothing launched) instead of raising; otherwise returns 0."""
    L = load()
    n = len(axes)
    buf = _buf()
    status = L.edhip_spline_filter_axes(ctypes.byref(in_desc), ctypes.byref(out_desc), n,
                                        (ctypes.c_int32 * n)(*axes), int(order), int(bool(transpose)),
                                        int(flags), stream, buf, 256)
    if status and not (may_decline and status == ERR_UNSUPPORTED):
        raise_for_status(status, buf)
    return status


def release_scratch():
    """edhip_release_scratch: free the library's cached per-stream workspaces."""
    load().edhip_release_scratch()
