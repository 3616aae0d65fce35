"""
CPU tests that pin the C ABI's answers at the boundary: for a table of calls the exact (status, message) pair of every
refusal an entry point can give before it touches the device, the message that wins when two arguments are wrong, and
the "nothing to do" successes.  The raw ctypes functions are called with descriptors of memory that does not exist;
every case returns before any allocation or launch, so no GPU is needed.
"""
import ctypes
import os

import numpy as np
import pytest

from elasticdeform_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                                reason="libedhip.so not built (run __graft_entry__.build())")

OK, INVALID, DTYPE, UNSUPPORTED = 0, 1, 2, 5
RAW, FAST, ZERO = _lib.FLAG_RAW_DISPLACEMENT, _lib.FLAG_FAST, _lib.FLAG_ZERO_GRADIENT

M_NIN = "invalid number of inputs/outputs"
M_AXES = "invalid axis list"
M_NAXIS = "more than 7 deformed axes are not supported on the GPU"
M_NDIM = "input and output dimensions should match"
M_RANK = "arrays must have 1..8 dimensions"
M_DTYPE = "data type not supported"
M_AXIS = "invalid axis in axis list"
M_INS = "all inputs should have the same size"
M_OUTS = "all outputs should have the same size"
M_ORDER = "spline order not supported"
M_MODE = "boundary mode not supported"
M_DISP = "invalid displacement shape"
M_DENSE = "EDHIP_FLAG_ZERO_GRADIENT needs dense gradient arrays"
M_LEN2 = "deformed axes must have at least 2 elements"
M_RAWMAX = "raw displacement grids are limited to 4096 points"
M_STEP = "non-deformed axes of input and output must have the same size"
M_OUT16 = "16-bit output next to a float32 volume: outside the tile kernels"
M_BATCH = "invalid batch"
M_NEITHER = "neither ddisplacement nor dinverse_affine is requested"
M_DDISP = "ddisplacement must have the shape of displacement"
M_DINV = "dinverse_affine must have shape (naxis, naxis + 1)"
M_DINV64 = "dinverse_affine must be float64"
M_DGRADK = "displacement gradient: naxis * (control points along the last axis) is limited to 256"
M_DGRADN = "displacement gradient: too many rows or samples"
M_WINDOWED = "windowed prefilter: outside the whole-line tile kernels"


def A(shape, dtype="float32", ptr=0x1000):
    """descriptor of a C-contiguous array that does not exist"""
    a = np.empty(shape, dtype=dtype)
    return _lib.describe(ptr, a.dtype.name, a.shape, a.strides)


def H(ndim, shape=(), dtype=9, ptr=0x1000):
    """a hostile descriptor: any rank, any extents, any dtype code (strides of a dense float64 array, or 8)"""
    shape = tuple(shape) + (0,) * (8 - len(shape))
    strides = [8] * 8
    for d in range(min(ndim, 8) - 2, -1, -1):
        strides[d] = strides[d + 1] * max(1, shape[d + 1])
    return _lib.EdhipArray(ptr, dtype, ndim, (ctypes.c_int64 * 8)(*shape), (ctypes.c_int64 * 8)(*strides))


def arr(descs):
    return (_lib.EdhipArray * len(descs))(*descs) if descs is not None else None


def ref(d):
    return ctypes.byref(d) if d is not None else None


def i32(v):
    return (ctypes.c_int32 * len(v))(*v) if v is not None else None


def i64(v):
    return (ctypes.c_int64 * len(v))(*v) if v is not None else None


def f64(v):
    return (ctypes.c_double * len(v))(*v) if v is not None else None


def run(fn, *args):
    buf = ctypes.create_string_buffer(b"stale", 256)
    st = fn(*args, buf, 256)
    return st, buf.value.decode()


X, D2 = A((8, 9)), A((2, 3, 3), "float64")
X3, D3 = A((6, 8, 9)), A((3, 3, 3, 3), "float64")
BIGD = A((2, 50, 50), "float64")             # 5000 points: beyond a raw grid, within a window's 7680
_DEF = object()


def deform(ins=(X,), disp=D2, outs=_DEF, naxis=2, axis=_DEF, orders=_DEF, modes=_DEF, cvals=_DEF, off=None,
           aff=None, flags=0, grad=0, n=None):
    n = len(ins) if n is None else n
    k = max(n, 1)
    outs = ins if outs is _DEF else outs
    axis = list(range(max(naxis, 0))) * k if axis is _DEF else axis
    orders = [3] * k if orders is _DEF else orders
    modes = [4] * k if modes is _DEF else modes
    cvals = [0.0] * k if cvals is _DEF else cvals
    return run(_lib.load().edhip_deform, grad, n, arr(ins), ref(disp), i64(off), arr(outs), naxis, i32(axis),
               i32(orders), i32(modes), f64(cvals), f64(aff), flags, None)


def batch(nb=1, ins=_DEF, disps=_DEF, outs=_DEF, naxis=2, axis=(0, 1), order=3, mode=4, flags=0, grad=0):
    ins = [X] * max(nb, 1) if ins is _DEF else ins
    disps = [D2] * max(nb, 1) if disps is _DEF else disps
    outs = ins if outs is _DEF else outs
    return run(_lib.load().edhip_deform_batch, grad, nb, arr(ins), arr(disps), None, arr(outs), naxis, i32(axis),
               order, mode, 0.0, None, flags, None)


def strided(nb=1, inp=X, disp=D2, out=_DEF, naxis=2, axis=(0, 1), order=3, mode=4, flags=0, grad=0):
    out = inp if out is _DEF else out
    return run(_lib.load().edhip_deform_batch_strided, grad, nb, ref(inp), 1 << 12, ref(disp), 1 << 12, None, ref(out),
               1 << 12, naxis, i32(axis), order, mode, 0.0, None, flags, None)


def box(disp=D2, in_len=(8, 9), out_len=(8, 9), naxis=2, flags=0, res=(0,) * 16):
    return run(_lib.load().edhip_source_box, ref(disp), i64(in_len), i64(out_len), None, naxis, None, flags, None,
               i64(res))


def window(disp=D2, in_len=(8, 9), out_len=(8, 9), naxis=2, shape=(8, 9), axis=(0, 1), ndim=None, flags=0,
           win=0x2000):
    ndim = len(shape) if ndim is None else ndim
    return run(_lib.load().edhip_source_window, ref(disp), i64(in_len), i64(out_len), None, naxis, None, ndim,
               i64(shape), i32(axis), 3, 4, 0, 1, 1, flags, None, win)


def filt(inp=X, out=_DEF, axis=0, order=3, transpose=0, flags=0):
    out = inp if out is _DEF else out
    return run(_lib.load().edhip_spline_filter1d, ref(inp), ref(out), axis, order, transpose, flags, None)


def filt_axes(inp=X, out=_DEF, axes=(0, 1), naxes=None, order=3, flags=0):
    out = inp if out is _DEF else out
    naxes = len(axes) if naxes is None else naxes
    return run(_lib.load().edhip_spline_filter_axes, ref(inp), ref(out), naxes, i32(axes), order, 0, flags, None)


def filt_win(inp=X, out=_DEF, axes=(0, 1), naxes=None, order=3, win=0x2000, flags=0):
    out = inp if out is _DEF else out
    naxes = len(axes) if naxes is None else naxes
    return run(_lib.load().edhip_spline_filter_axes_window, ref(inp), ref(out), naxes, i32(axes), order, 0, win,
               flags, None)


def tgrad(ins=(X,), disp=D2, douts=_DEF, naxis=2, axis=_DEF, orders=_DEF, modes=_DEF, ddisp=_DEF, dinv=None,
          flags=0, n=None, only_displacement=False):
    n = len(ins) if n is None else n
    k = max(n, 1)
    douts = ins if douts is _DEF else douts
    axis = list(range(max(naxis, 0))) * k if axis is _DEF else axis
    orders = [3] * k if orders is _DEF else orders
    modes = [4] * k if modes is _DEF else modes
    ddisp = disp if ddisp is _DEF else ddisp
    L = _lib.load()
    head = (n, arr(ins), ref(disp), None, arr(douts), naxis, i32(axis), i32(orders), i32(modes), f64([0.0] * k), None)
    if only_displacement:
        return run(L.edhip_deform_displacement_gradient, *head, ref(ddisp), flags, None)
    return run(L.edhip_deform_transform_gradient, *head, ref(ddisp), ref(dinv), flags, None)


def tgrad_batch(nb=1, inp=X, disp=D2, dout=_DEF, naxis=2, axis=(0, 1), order=3, mode=4, ddisp=_DEF, dinv=None,
                flags=0, only_displacement=False):
    dout = inp if dout is _DEF else dout
    ddisp = disp if ddisp is _DEF else ddisp
    L = _lib.load()
    head = (nb, ref(inp), 1 << 12, ref(disp), 1 << 12, None, ref(dout), 1 << 12, naxis, i32(axis), order, mode, 0.0,
            None)
    if only_displacement:
        return run(L.edhip_deform_displacement_gradient_batch_strided, *head, ref(ddisp), 1 << 12, flags, None)
    return run(L.edhip_deform_transform_gradient_batch_strided, *head, ref(ddisp), 1 << 12, ref(dinv), 1 << 12, flags, None)


PTS = A((5, 2), "float64")


def points(inverse=0, nb=1, pts=PTS, disp=D2, in_len=(8, 9), naxis=2, aff=None, lin=None, res=_DEF, jac=None,
           status=None, max_iter=20, tol=1e-9, flags=0):
    res = pts if res is _DEF else res
    return run(_lib.load().edhip_deform_points, inverse, nb, ref(pts), 0, ref(disp), 0, i64(in_len), None, naxis,
               f64(aff), f64(lin), ref(res), 0, ref(jac), 0, ref(status), 0, max_iter, tol, flags, None)


L8 = A((8, 9), "uint8")


def labels(nb=1, inp=L8, disp=D2, out=_DEF, wt=None, naxis=2, axis=(0, 1), mode=0, cval=0.0, flags=0):
    out = inp if out is _DEF else out
    return run(_lib.load().edhip_deform_labels, nb, ref(inp), 0, ref(disp), 0, None, ref(out), 0, ref(wt), 0, naxis,
               i32(axis), mode, cval, None, flags, None)


def pgrad(inverse=0, nb=1, pos=PTS, cot=_DEF, status=None, disp=D2, in_len=(8, 9), naxis=2, dpts=_DEF, ddisp=_DEF,
          dinv=_DEF, flags=0):
    cot = pos if cot is _DEF else cot
    dpts = pos if dpts is _DEF else dpts
    ddisp = disp if ddisp is _DEF else ddisp
    dinv = DINV if dinv is _DEF else dinv
    return run(_lib.load().edhip_deform_points_gradient, inverse, nb, ref(pos), 0, ref(cot), 0, ref(status), 0,
               ref(disp), 0, i64(in_len), None, naxis, None, ref(dpts), 0, ref(ddisp), 0, ref(dinv), 0, flags, None)


Y2, Z2 = A((6, 7)), A((8, 9))


def inverse(nb=1, inp=Y2, disp=D2, in_len=(8, 9), out=Z2, valid=None, naxis=2, axis=(0, 1), order=3, mode=0, aff=None,
            lin=None, max_iter=20, tol=1e-9, flags=0):
    return run(_lib.load().edhip_deform_inverse, nb, ref(inp), 0, ref(disp), 0, i64(in_len), None, ref(out), 0,
               ref(valid), 0, naxis, i32(axis), order, mode, 0.0, f64(aff), f64(lin), max_iter, tol, flags, None)


AX8 = list(range(8))
X8 = A((2,) * 8)
D5 = A((5, 2, 2, 2, 2, 2), "float64")
DINV = A((2, 3), "float64")
NOT_DENSE = _lib.describe(0x1000, "float32", (8, 9), (80, 4))
ROWS = _lib.describe(0x1000, "float32", (1 << 32, 9), (36, 4))       # 2^32 output rows

CASES = [
    # ---- edhip_deform: one case per refusal ------------------------------------------------------------------
    ("deform-no-inputs", lambda: deform(ins=None, outs=None, n=1), (INVALID, M_NIN)),
    ("deform-zero-inputs", lambda: deform(n=0), (INVALID, M_NIN)),
    ("deform-too-many-inputs", lambda: deform(n=1 << 20), (INVALID, M_NIN)),
    ("deform-naxis-0", lambda: deform(naxis=0, axis=[0]), (INVALID, M_AXES)),
    ("deform-null-axis", lambda: deform(axis=None), (INVALID, M_AXES)),
    ("deform-null-cvals", lambda: deform(cvals=None), (INVALID, M_AXES)),
    ("deform-naxis-8", lambda: deform(ins=[X8], naxis=8, axis=AX8), (UNSUPPORTED, M_NAXIS)),
    ("deform-rank-mismatch", lambda: deform(outs=[A((8, 9, 1))]), (INVALID, M_NDIM)),
    ("deform-ndim-0", lambda: deform(ins=[H(0)]), (UNSUPPORTED, M_RANK)),
    ("deform-ndim-9", lambda: deform(ins=[H(9, (2,) * 8)]), (UNSUPPORTED, M_RANK)),
    ("deform-dtype-13", lambda: deform(ins=[H(2, (8, 9), 13)]), (DTYPE, M_DTYPE)),
    ("deform-dtype-negative", lambda: deform(outs=[H(2, (8, 9), -1)]), (DTYPE, M_DTYPE)),
    ("deform-axis-high", lambda: deform(axis=[0, 2]), (INVALID, M_AXIS)),
    ("deform-axis-negative", lambda: deform(axis=[-1, 1]), (INVALID, M_AXIS)),
    ("deform-inputs-differ", lambda: deform(ins=[X, A((8, 10))], outs=[X, X]), (INVALID, M_INS)),
    ("deform-outputs-differ", lambda: deform(ins=[X, X], outs=[X, A((8, 10))]), (INVALID, M_OUTS)),
    ("deform-order-6", lambda: deform(orders=[6]), (INVALID, M_ORDER)),
    ("deform-order-negative", lambda: deform(orders=[-1]), (INVALID, M_ORDER)),
    ("deform-mode-5", lambda: deform(modes=[5]), (INVALID, M_MODE)),
    ("deform-null-displacement", lambda: deform(disp=None), (INVALID, M_DISP)),
    ("deform-displacement-rank", lambda: deform(disp=A((2, 3), "float64")), (INVALID, M_DISP)),
    ("deform-displacement-components", lambda: deform(disp=A((3, 3, 3), "float64")), (INVALID, M_DISP)),
    ("deform-displacement-dtype", lambda: deform(disp=H(3, (2, 3, 3), 13)), (DTYPE, M_DTYPE)),
    ("deform-displacement-empty", lambda: deform(disp=A((2, 0, 3), "float64")), (INVALID, M_DISP)),
    ("deform-displacement-negative", lambda: deform(disp=H(3, (2, 3, -3), 10)), (INVALID, M_DISP)),
    ("deform-not-dense", lambda: deform(ins=[NOT_DENSE], grad=1, flags=ZERO), (INVALID, M_DENSE)),
    ("deform-length-1", lambda: deform(ins=[A((1, 9))], outs=[X]), (INVALID, M_LEN2)),
    ("deform-raw-5000", lambda: deform(disp=BIGD, flags=RAW), (UNSUPPORTED, M_RAWMAX)),
    ("deform-step-axes-differ", lambda: deform(ins=[A((4, 8, 9))], outs=[A((5, 8, 9))], axis=[1, 2]),
     (INVALID, M_STEP)),
    ("deform-out16-misaligned", lambda: deform(outs=[A((8, 9), "float16", 0x1002)], flags=FAST),
     (UNSUPPORTED, M_OUT16)),
    ("deform-out16-two-axes", lambda: deform(outs=[A((8, 9), "float16")], flags=FAST), (UNSUPPORTED, M_OUT16)),
    ("deform-out16-no-steps", lambda: deform(ins=[A((0, 8, 9))], outs=[A((0, 8, 9), "float16")], axis=[1, 2],
                                             flags=FAST), (UNSUPPORTED, M_OUT16)),
    # ---- edhip_deform: which message wins ----------------------------------------------------------------------
    ("deform-naxis-8+bad-displacement", lambda: deform(ins=[X8], naxis=8, axis=AX8, disp=A((2, 3), "float64")),
     (UNSUPPORTED, M_NAXIS)),
    ("deform-naxis-8+ndim-0", lambda: deform(ins=[H(0)], naxis=8, axis=AX8), (UNSUPPORTED, M_NAXIS)),
    ("deform-no-inputs+naxis-0", lambda: deform(n=0, naxis=0), (INVALID, M_NIN)),
    ("deform-rank-mismatch+ndim-9", lambda: deform(ins=[H(9, (2,) * 8)], outs=[X]), (INVALID, M_NDIM)),
    ("deform-axis+order", lambda: deform(axis=[0, 2], orders=[6]), (INVALID, M_AXIS)),
    ("deform-dtype+axis", lambda: deform(ins=[H(2, (8, 9), 13)], axis=[0, 2]), (DTYPE, M_DTYPE)),
    ("deform-order+mode", lambda: deform(orders=[6], modes=[5]), (INVALID, M_ORDER)),
    ("deform-second-axis+first-mode", lambda: deform(ins=[X, X], axis=[0, 1, 0, 2], modes=[5, 4]),
     (INVALID, M_MODE)),
    ("deform-mode+displacement", lambda: deform(modes=[5], disp=None), (INVALID, M_MODE)),
    ("deform-length-1+mode", lambda: deform(ins=[A((1, 9))], outs=[X], modes=[5]), (INVALID, M_MODE)),
    ("deform-displacement-shape+dtype", lambda: deform(disp=H(3, (3, 3, 3), 13)), (INVALID, M_DISP)),
    ("deform-displacement-dtype+empty", lambda: deform(disp=H(3, (2, 0, 3), 13)), (DTYPE, M_DTYPE)),
    ("deform-displacement+not-dense", lambda: deform(ins=[NOT_DENSE], disp=A((2, 0, 3), "float64"), grad=1,
                                                     flags=ZERO), (INVALID, M_DISP)),
    ("deform-not-dense+length-1", lambda: deform(ins=[_lib.describe(0x1000, "float32", (1, 9), (80, 8))], outs=[X],
                                                 grad=1, flags=ZERO), (INVALID, M_DENSE)),
    ("deform-length-1+raw-5000", lambda: deform(ins=[A((1, 9))], outs=[X], disp=BIGD, flags=RAW), (INVALID, M_LEN2)),
    ("deform-length-1+step-axes", lambda: deform(ins=[A((4, 1, 9))], outs=[A((5, 8, 9))], axis=[1, 2]),
     (INVALID, M_LEN2)),
    ("deform-step-axes+out16", lambda: deform(ins=[A((4, 8, 9))], outs=[A((5, 8, 9), "float16", 0x1002)],
                                              axis=[1, 2], flags=FAST), (INVALID, M_STEP)),
    ("deform-second-pair-step-axes", lambda: deform(ins=[A((0, 8, 9)), A((4, 8, 9))],
                                                    outs=[A((0, 8, 9)), A((5, 8, 9))], axis=[1, 2, 1, 2]),
     (INVALID, M_STEP)),
    # ---- edhip_deform: nothing to do -----------------------------------------------------------------------------
    ("deform-no-voxels", lambda: deform(outs=[A((0, 9))]), (OK, "")),
    ("deform-no-voxels-length-1", lambda: deform(ins=[A((1, 9))], outs=[A((0, 9))]), (OK, "")),
    ("deform-no-voxels+step-axes", lambda: deform(ins=[A((4, 8, 9))], outs=[A((5, 0, 9))], axis=[1, 2]), (OK, "")),
    ("deform-no-voxels-zero-gradient", lambda: deform(ins=[A((0, 9))], outs=[A((0, 9))], grad=1, flags=ZERO),
     (OK, "")),
    ("deform-no-steps", lambda: deform(ins=[A((0, 8, 9))], axis=[1, 2]), (OK, "")),
    ("deform-no-steps-zero-gradient", lambda: deform(ins=[A((0, 8, 9))], axis=[1, 2], grad=1, flags=ZERO),
     (OK, "")),
    # ---- edhip_deform_batch / edhip_deform_batch_strided ---------------------------------------------------------
    ("batch-negative", lambda: batch(nb=-1), (INVALID, M_BATCH)),
    ("batch-null-inputs", lambda: batch(ins=None, outs=None), (INVALID, M_BATCH)),
    ("batch-null-displacements", lambda: batch(disps=None), (INVALID, M_BATCH)),
    ("batch-empty", lambda: batch(nb=0, ins=None, disps=None, outs=None), (OK, "")),
    ("batch-not-dense", lambda: batch(ins=[NOT_DENSE], outs=[X], grad=1, flags=ZERO), (INVALID, M_DENSE)),
    ("batch-not-dense+order", lambda: batch(ins=[NOT_DENSE], outs=[X], grad=1, flags=ZERO, order=6),
     (INVALID, M_DENSE)),
    ("batch-order", lambda: batch(order=6), (INVALID, M_ORDER)),
    ("batch-null-axis", lambda: batch(axis=None), (INVALID, M_AXES)),
    ("batch-of-2-order", lambda: batch(nb=2, ins=[X3, A((6, 8, 9), ptr=0x2000)], disps=[D3, D3], naxis=3,
                                       axis=(0, 1, 2), order=6), (INVALID, M_ORDER)),
    ("batch-of-2-length-1", lambda: batch(nb=2, ins=[A((1, 8, 9)), A((1, 8, 9), ptr=0x2000)],
                                          outs=[X3, A((6, 8, 9), ptr=0x3000)], disps=[D3, D3], naxis=3,
                                          axis=(0, 1, 2)), (INVALID, M_LEN2)),
    ("batch-no-voxels", lambda: batch(nb=2, outs=[A((0, 9))] * 2), (OK, "")),
    ("strided-negative", lambda: strided(nb=-1), (INVALID, M_BATCH)),
    ("strided-null-output", lambda: strided(out=None), (INVALID, M_BATCH)),
    ("strided-empty", lambda: strided(nb=0, inp=None, disp=None, out=None), (OK, "")),
    ("strided-mode", lambda: strided(nb=3, mode=-1), (INVALID, M_MODE)),
    ("strided-naxis-8+displacement", lambda: strided(inp=X8, naxis=8, axis=AX8), (UNSUPPORTED, M_NAXIS)),
    ("strided-no-voxels", lambda: strided(nb=3, out=A((8, 0))), (OK, "")),
    # ---- edhip_source_box ------------------------------------------------------------------------------------------
    ("box-null-lengths", lambda: box(in_len=None), (INVALID, M_AXES)),
    ("box-null-result", lambda: box(res=None), (INVALID, M_AXES)),
    ("box-naxis-0", lambda: box(naxis=0), (INVALID, M_AXES)),
    ("box-naxis-8", lambda: box(naxis=8, in_len=(4,) * 8, out_len=(4,) * 8), (UNSUPPORTED, M_NAXIS)),
    ("box-null-displacement", lambda: box(disp=None), (INVALID, M_DISP)),
    ("box-displacement-components", lambda: box(disp=A((3, 3, 3), "float64")), (INVALID, M_DISP)),
    ("box-displacement-dtype", lambda: box(disp=H(3, (2, 3, 3), -2)), (DTYPE, M_DTYPE)),
    ("box-displacement-empty", lambda: box(disp=A((2, 3, 0), "float64")), (INVALID, M_DISP)),
    ("box-displacement-dtype+empty", lambda: box(disp=H(3, (2, 3, 0), 13)), (DTYPE, M_DTYPE)),
    ("box-length-1", lambda: box(in_len=(8, 1)), (INVALID, M_LEN2)),
    ("box-raw-5000", lambda: box(disp=BIGD, flags=RAW), (UNSUPPORTED, M_RAWMAX)),
    ("box-length-1+raw-5000", lambda: box(in_len=(1, 9), disp=BIGD, flags=RAW), (INVALID, M_LEN2)),
    # ---- edhip_source_window ---------------------------------------------------------------------------------------
    ("window-null-window", lambda: window(win=None), (INVALID, M_AXES)),
    ("window-null-shape", lambda: window(shape=None, ndim=2), (INVALID, M_AXES)),
    ("window-ndim-below-naxis", lambda: window(shape=(8,), axis=(0, 0)), (INVALID, M_AXES)),
    ("window-ndim-9", lambda: window(shape=(8, 9) + (1,) * 7), (INVALID, M_AXES)),
    ("window-naxis-5", lambda: window(disp=D5, naxis=5, in_len=(4,) * 5, out_len=(4,) * 5, shape=(4,) * 5,
                                      axis=range(5)), (UNSUPPORTED, "edhip_source_window: up to 4 deformed axes")),
    ("window-naxis-5+displacement", lambda: window(naxis=5, in_len=(4,) * 5, out_len=(4,) * 5, shape=(4,) * 5,
                                                   axis=range(5)),
     (UNSUPPORTED, "edhip_source_window: up to 4 deformed axes")),
    ("window-null-displacement", lambda: window(disp=None), (INVALID, M_DISP)),
    ("window-displacement-rank", lambda: window(disp=A((2, 3, 3, 3), "float64")), (INVALID, M_DISP)),
    ("window-displacement-dtype", lambda: window(disp=H(3, (2, 3, 3), 99)), (DTYPE, M_DTYPE)),
    ("window-displacement-negative", lambda: window(disp=H(3, (2, -3, 3), 10)), (INVALID, M_DISP)),
    ("window-7700-values", lambda: window(disp=A((2, 55, 70), "float64")),
     (UNSUPPORTED, "edhip_source_window: control grids are limited to 7680 values")),
    ("window-7700-values+shape", lambda: window(disp=A((2, 55, 70), "float64"), shape=(8, 0)),
     (UNSUPPORTED, "edhip_source_window: control grids are limited to 7680 values")),
    ("window-shape-0", lambda: window(shape=(8, 0)), (INVALID, "invalid shape")),
    ("window-shape-2^30", lambda: window(shape=(8, 1 << 30), in_len=(8, 1 << 30)), (INVALID, "invalid shape")),
    ("window-axis-high", lambda: window(axis=(0, 2)), (INVALID, M_AXES)),
    ("window-axis-length", lambda: window(in_len=(8, 10)), (INVALID, M_AXES)),
    ("window-length-1", lambda: window(shape=(8, 1), in_len=(8, 1)), (INVALID, M_LEN2)),
    ("window-raw-5000", lambda: window(disp=BIGD, flags=RAW), (UNSUPPORTED, M_RAWMAX)),
    # ---- the prefilter -----------------------------------------------------------------------------------------------
    ("filter-null-input", lambda: filt(inp=None, out=X), (INVALID, "missing array")),
    ("filter-null-output", lambda: filt(out=None), (INVALID, "missing array")),
    ("filter-order-6", lambda: filt(order=6), (INVALID, M_ORDER)),
    ("filter-null+order", lambda: filt(out=None, order=6), (INVALID, "missing array")),
    ("filter-ndim-0", lambda: filt(inp=H(0)), (INVALID, M_NDIM)),
    ("filter-ndim-9", lambda: filt(inp=H(9, (2,) * 8)), (INVALID, M_NDIM)),
    ("filter-rank-mismatch", lambda: filt(out=A((8, 9, 1))), (INVALID, M_NDIM)),
    ("filter-order+rank", lambda: filt(out=A((8, 9, 1)), order=-1), (INVALID, M_ORDER)),
    ("filter-axis-2", lambda: filt(axis=2), (INVALID, "invalid axis")),
    ("filter-axis-minus-3", lambda: filt(axis=-3), (INVALID, "invalid axis")),
    ("filter-dtype", lambda: filt(inp=H(2, (8, 9), 13)), (DTYPE, M_DTYPE)),
    ("filter-axis+dtype", lambda: filt(inp=H(2, (8, 9), 13), axis=2), (INVALID, "invalid axis")),
    ("filter-shapes", lambda: filt(out=A((8, 10))), (INVALID, "input and output shapes should match")),
    ("filter-dtype+shapes", lambda: filt(out=H(2, (8, 10), 13)), (DTYPE, M_DTYPE)),
    ("filter-no-samples", lambda: filt(inp=A((0, 9))), (OK, "")),
    ("filter-no-lines", lambda: filt(inp=A((8, 0)), axis=-2), (OK, "")),
    ("filter-half-order-1", lambda: filt(inp=A((8, 9), "float16"), out=X, order=1, flags=FAST),
     (UNSUPPORTED, "16-bit storage next to a float32 pass: outside the whole-line tile kernels")),
    ("axes-negative", lambda: filt_axes(naxes=-1), (INVALID, M_AXES)),
    ("axes-null", lambda: filt_axes(axes=None, naxes=2), (INVALID, M_AXES)),
    ("axes-none", lambda: filt_axes(inp=None, out=None, axes=None, naxes=0), (OK, "")),
    ("axes-null-input", lambda: filt_axes(inp=None, out=X), (INVALID, "missing array")),
    ("axes-second-axis", lambda: filt_axes(inp=A((0, 9)), axes=(0, 2)), (INVALID, "invalid axis")),
    ("axes-order", lambda: filt_axes(order=6), (INVALID, M_ORDER)),
    ("axes-converting-order-1", lambda: filt_axes(inp=A((8, 9), "float16"), out=X, order=1, flags=FAST),
     (UNSUPPORTED, M_WINDOWED)),
    ("axes-no-samples", lambda: filt_axes(inp=A((0, 9))), (OK, "")),
    ("axes-window-null-window", lambda: filt_win(win=None), (INVALID, "invalid axis list / window")),
    ("axes-window-null-axes", lambda: filt_win(axes=None, naxes=1), (INVALID, "invalid axis list / window")),
    ("axes-window-negative", lambda: filt_win(naxes=-1), (INVALID, "invalid axis list / window")),
    ("axes-window-none", lambda: filt_win(axes=None, naxes=0), (OK, "")),
    ("axes-window-integers", lambda: filt_win(inp=L8), (UNSUPPORTED, M_WINDOWED)),
    ("axes-window-order-1", lambda: filt_win(order=1), (UNSUPPORTED, M_WINDOWED)),
    ("axes-window-second-axis", lambda: filt_win(inp=A((0, 9)), axes=(0, 2)), (INVALID, "invalid axis")),
    ("axes-window-shapes", lambda: filt_win(out=A((8, 10))), (INVALID, "input and output shapes should match")),
    ("axes-window-no-samples", lambda: filt_win(inp=A((0, 9))), (OK, "")),
    # ---- the four gradient entry points ----------------------------------------------------------------------------
    ("tgrad-no-inputs", lambda: tgrad(n=0), (INVALID, M_NIN)),
    ("tgrad-naxis-0", lambda: tgrad(naxis=0, axis=[0]), (INVALID, M_AXES)),
    ("tgrad-naxis-8", lambda: tgrad(ins=[X8], naxis=8, axis=AX8), (UNSUPPORTED, M_NAXIS)),
    ("tgrad-naxis-8+neither", lambda: tgrad(ins=[X8], naxis=8, axis=AX8, ddisp=None), (UNSUPPORTED, M_NAXIS)),
    ("tgrad-rank-mismatch", lambda: tgrad(douts=[A((8, 9, 1))]), (INVALID, M_NDIM)),
    ("tgrad-ndim-0", lambda: tgrad(ins=[H(0)]), (UNSUPPORTED, M_RANK)),
    ("tgrad-ndim-9", lambda: tgrad(ins=[H(9, (2,) * 8)]), (UNSUPPORTED, M_RANK)),
    ("tgrad-integer-volume", lambda: tgrad(ins=[A((8, 9), "int16")]), (DTYPE, M_DTYPE)),
    ("tgrad-half-dy", lambda: tgrad(douts=[A((8, 9), "float16")]), (DTYPE, M_DTYPE)),
    ("tgrad-dtype-13", lambda: tgrad(ins=[H(2, (8, 9), 13)]), (DTYPE, M_DTYPE)),
    ("tgrad-integer-volume+axis", lambda: tgrad(ins=[A((8, 9), "int16")], axis=[0, 2]), (DTYPE, M_DTYPE)),
    ("tgrad-axis", lambda: tgrad(axis=[0, 2]), (INVALID, M_AXIS)),
    ("tgrad-axis+order", lambda: tgrad(axis=[0, 2], orders=[6]), (INVALID, M_AXIS)),
    ("tgrad-inputs-differ", lambda: tgrad(ins=[X, A((8, 10))], douts=[X, X]), (INVALID, M_INS)),
    ("tgrad-outputs-differ", lambda: tgrad(ins=[X, X], douts=[X, A((8, 10))]), (INVALID, M_OUTS)),
    ("tgrad-order", lambda: tgrad(orders=[6]), (INVALID, M_ORDER)),
    ("tgrad-mode", lambda: tgrad(modes=[5]), (INVALID, M_MODE)),
    ("tgrad-length-1+mode", lambda: tgrad(ins=[A((1, 9))], douts=[X], modes=[5]), (INVALID, M_MODE)),
    ("tgrad-null-displacement", lambda: tgrad(disp=None, ddisp=D2), (INVALID, M_DISP)),
    ("tgrad-displacement-components", lambda: tgrad(disp=A((3, 3, 3), "float64")), (INVALID, M_DISP)),
    ("tgrad-displacement-dtype", lambda: tgrad(disp=H(3, (2, 3, 3), 13), ddisp=D2), (DTYPE, M_DTYPE)),
    ("tgrad-displacement-empty", lambda: tgrad(disp=A((2, 3, 0), "float64")), (INVALID, M_DISP)),
    ("tgrad-displacement+neither", lambda: tgrad(disp=A((2, 3), "float64"), ddisp=None), (INVALID, M_DISP)),
    ("tgrad-neither", lambda: tgrad(ddisp=None), (INVALID, M_NEITHER)),
    ("tgrad-ddisp-rank", lambda: tgrad(ddisp=A((2, 3), "float64")), (INVALID, M_DDISP)),
    ("tgrad-ddisp-shape", lambda: tgrad(ddisp=A((2, 3, 4), "float64")), (INVALID, M_DDISP)),
    ("tgrad-ddisp-dtype", lambda: tgrad(ddisp=H(3, (2, 3, 3), 13)), (DTYPE, M_DTYPE)),
    ("tgrad-ddisp-shape+dtype", lambda: tgrad(ddisp=H(3, (2, 3, 4), 13)), (INVALID, M_DDISP)),
    ("tgrad-dinv-shape", lambda: tgrad(dinv=A((3, 2), "float64")), (INVALID, M_DINV)),
    ("tgrad-dinv-rank", lambda: tgrad(ddisp=None, dinv=A((6,), "float64")), (INVALID, M_DINV)),
    ("tgrad-dinv-float32", lambda: tgrad(ddisp=None, dinv=A((2, 3), "float32")), (DTYPE, M_DINV64)),
    ("tgrad-ddisp-shape+dinv-float32", lambda: tgrad(ddisp=A((2, 3, 4), "float64"), dinv=A((2, 3), "float32")),
     (INVALID, M_DDISP)),
    ("tgrad-dinv-float32+raw-5000", lambda: tgrad(disp=BIGD, dinv=A((2, 3), "float32"), flags=RAW),
     (DTYPE, M_DINV64)),
    ("tgrad-raw-5000", lambda: tgrad(disp=BIGD, flags=RAW), (UNSUPPORTED, M_RAWMAX)),
    ("tgrad-raw-5000+step-axes", lambda: tgrad(ins=[A((4, 8, 9))], douts=[A((5, 8, 9))], axis=[1, 2], disp=BIGD,
                                               flags=RAW), (UNSUPPORTED, M_RAWMAX)),
    ("tgrad-step-axes", lambda: tgrad(ins=[A((4, 8, 9))], douts=[A((5, 8, 9))], axis=[1, 2]), (INVALID, M_STEP)),
    ("tgrad-step-axes+length-1", lambda: tgrad(ins=[A((4, 1, 9))], douts=[A((5, 8, 9))], axis=[1, 2]),
     (INVALID, M_STEP)),
    ("tgrad-length-1", lambda: tgrad(ins=[A((1, 9))], douts=[X]), (INVALID, M_LEN2)),
    ("tgrad-length-1+wide-grid", lambda: tgrad(ins=[A((1, 9))], douts=[X], disp=A((2, 3, 129), "float64")),
     (INVALID, M_LEN2)),
    ("tgrad-wide-grid", lambda: tgrad(disp=A((2, 3, 129), "float64")), (UNSUPPORTED, M_DGRADK)),
    ("tgrad-wide-grid+rows", lambda: tgrad(douts=[ROWS], disp=A((2, 3, 129), "float64")),
     (UNSUPPORTED, M_DGRADK)),
    ("tgrad-rows", lambda: tgrad(douts=[ROWS]), (UNSUPPORTED, M_DGRADN)),
    ("dgrad-null-ddisp", lambda: tgrad(ddisp=None, only_displacement=True), (INVALID, M_DDISP)),
    ("dgrad-null-ddisp+no-inputs", lambda: tgrad(n=0, ddisp=None, only_displacement=True), (INVALID, M_DDISP)),
    ("dgrad-order", lambda: tgrad(orders=[6], only_displacement=True), (INVALID, M_ORDER)),
    ("dgrad-ddisp-shape", lambda: tgrad(ddisp=A((2, 4, 3), "float64"), only_displacement=True), (INVALID, M_DDISP)),
    ("tgrad-batch-negative", lambda: tgrad_batch(nb=-1), (INVALID, M_BATCH)),
    ("tgrad-batch-null-input", lambda: tgrad_batch(inp=None, dout=X), (INVALID, M_BATCH)),
    ("tgrad-batch-neither", lambda: tgrad_batch(ddisp=None), (INVALID, M_NEITHER)),
    ("tgrad-batch-empty-neither", lambda: tgrad_batch(nb=0, ddisp=None), (INVALID, M_NEITHER)),
    ("tgrad-batch-negative+neither", lambda: tgrad_batch(nb=-1, ddisp=None), (INVALID, M_BATCH)),
    ("tgrad-batch-empty", lambda: tgrad_batch(nb=0, inp=None, disp=None, dout=None, ddisp=D2), (OK, "")),
    ("tgrad-batch-order", lambda: tgrad_batch(nb=3, order=6), (INVALID, M_ORDER)),
    ("tgrad-batch-raw-order", lambda: tgrad_batch(nb=3, order=6, flags=RAW), (INVALID, M_ORDER)),
    ("tgrad-batch-raw-5000", lambda: tgrad_batch(nb=3, disp=BIGD, flags=RAW), (UNSUPPORTED, M_RAWMAX)),
    ("tgrad-batch-raw-length-1", lambda: tgrad_batch(nb=3, inp=A((1, 9)), dout=X, flags=RAW), (INVALID, M_LEN2)),
    ("tgrad-batch-65536", lambda: tgrad_batch(nb=65536), (UNSUPPORTED, M_DGRADN)),
    ("tgrad-batch-65536+wide-grid", lambda: tgrad_batch(nb=65536, disp=A((2, 3, 129), "float64")),
     (UNSUPPORTED, M_DGRADK)),
    ("tgrad-batch-dinv-float32", lambda: tgrad_batch(nb=2, dinv=A((2, 3), "float32")), (DTYPE, M_DINV64)),
    ("dgrad-batch-negative", lambda: tgrad_batch(nb=-1, only_displacement=True), (INVALID, M_BATCH)),
    ("dgrad-batch-null-ddisp", lambda: tgrad_batch(ddisp=None, only_displacement=True), (INVALID, M_BATCH)),
    ("dgrad-batch-empty", lambda: tgrad_batch(nb=0, ddisp=None, only_displacement=True), (OK, "")),
    ("dgrad-batch-null-input", lambda: tgrad_batch(inp=None, dout=X, only_displacement=True), (INVALID, M_BATCH)),
    ("dgrad-batch-ddisp-shape", lambda: tgrad_batch(nb=2, ddisp=A((2, 3, 4), "float64"), only_displacement=True),
     (INVALID, M_DDISP)),
    # ---- edhip_deform_points ---------------------------------------------------------------------------------------
    ("points-negative-batch", lambda: points(nb=-1), (INVALID, M_BATCH)),
    ("points-null-points", lambda: points(pts=None, res=PTS), (INVALID, M_BATCH)),
    ("points-null-displacement", lambda: points(disp=None), (INVALID, M_BATCH)),
    ("points-null-lengths", lambda: points(in_len=None), (INVALID, M_BATCH)),
    ("points-naxis-0", lambda: points(naxis=0), (INVALID, M_AXES)),
    ("points-naxis-8", lambda: points(naxis=8, in_len=(4,) * 8), (UNSUPPORTED, M_NAXIS)),
    ("points-naxis-8+displacement+raw", lambda: points(naxis=8, in_len=(4,) * 8, disp=A((2, 3), "float64"),
                                                       flags=RAW), (UNSUPPORTED, M_NAXIS)),
    ("points-raw", lambda: points(flags=RAW), (INVALID, "edhip_deform_points takes the prefiltered control grid")),
    ("points-raw+shape", lambda: points(flags=RAW, pts=A((5, 3), "float64")),
     (INVALID, "edhip_deform_points takes the prefiltered control grid")),
    ("points-shape", lambda: points(pts=A((5, 3), "float64")), (INVALID, "points must have shape (N, naxis)")),
    ("points-rank", lambda: points(pts=A((10,), "float64")), (INVALID, "points must have shape (N, naxis)")),
    ("points-negative-count", lambda: points(pts=H(2, (-1, 2), 10)), (INVALID, "points must have shape (N, naxis)")),
    ("points-result-shape", lambda: points(res=A((4, 2), "float64")), (INVALID, "result must have the shape of points")),
    ("points-dtype", lambda: points(pts=A((5, 2), "int32")), (DTYPE, M_DTYPE)),
    ("points-result-dtype", lambda: points(res=A((5, 2), "float16")), (DTYPE, M_DTYPE)),
    ("points-result-shape+dtype", lambda: points(res=A((4, 2), "int32")),
     (INVALID, "result must have the shape of points")),
    ("points-jacobian-inverse", lambda: points(inverse=1, jac=A((5, 2, 2), "float64")),
     (INVALID, "the jacobian belongs to the forward direction")),
    ("points-jacobian-shape", lambda: points(jac=A((5, 2, 3), "float64")),
     (INVALID, "jacobian must have shape (N, naxis, naxis)")),
    ("points-jacobian-float32", lambda: points(jac=A((5, 2, 2), "float32")), (DTYPE, "jacobian must be float64")),
    ("points-status-forward", lambda: points(status=A((5,), "uint8")),
     (INVALID, "the status belongs to the inverse direction")),
    ("points-status-shape", lambda: points(inverse=1, status=A((4,), "uint8")), (INVALID, "status must have shape (N)")),
    ("points-status-dtype", lambda: points(inverse=1, status=A((5,), "bool")), (DTYPE, "status must be uint8")),
    ("points-max-iter", lambda: points(inverse=1, max_iter=0), (INVALID, "max_iter must be at least 1")),
    ("points-tol", lambda: points(inverse=1, tol=0.0), (INVALID, "tol must be positive")),
    ("points-tol-nan", lambda: points(inverse=1, tol=float("nan")), (INVALID, "tol must be positive")),
    ("points-max-iter+tol", lambda: points(inverse=1, max_iter=0, tol=0.0), (INVALID, "max_iter must be at least 1")),
    ("points-forward-ignores-tol", lambda: points(max_iter=0, tol=0.0, nb=0), (OK, "")),
    ("points-affine-without-linear", lambda: points(inverse=1, aff=[1, 0, 0, 0, 1, 0]),
     (INVALID, "forward_linear is required with an affine map")),
    ("points-tol+displacement", lambda: points(inverse=1, tol=0.0, disp=A((2, 3), "float64")),
     (INVALID, "tol must be positive")),
    ("points-displacement-rank", lambda: points(disp=A((2, 3), "float64")), (INVALID, M_DISP)),
    ("points-displacement-components", lambda: points(disp=A((3, 3, 3), "float64")), (INVALID, M_DISP)),
    ("points-displacement-dtype", lambda: points(disp=H(3, (2, 3, 3), 13)), (DTYPE, M_DTYPE)),
    ("points-displacement-empty", lambda: points(disp=A((2, 0, 3), "float64")), (INVALID, M_DISP)),
    ("points-displacement+65536", lambda: points(nb=65536, disp=A((2, 0, 3), "float64")), (INVALID, M_DISP)),
    ("points-65536", lambda: points(nb=65536), (UNSUPPORTED, "edhip_deform_points: too many samples")),
    ("points-65536+length-1", lambda: points(nb=65536, in_len=(8, 1)),
     (UNSUPPORTED, "edhip_deform_points: too many samples")),
    ("points-length-1", lambda: points(in_len=(8, 1)), (INVALID, M_LEN2)),
    ("points-length-1-empty-batch", lambda: points(nb=0, in_len=(8, 1)), (INVALID, M_LEN2)),
    ("points-length-0-no-points", lambda: points(pts=A((0, 2), "float64"), in_len=(0, 9)), (OK, "")),
    ("points-empty-batch", lambda: points(nb=0), (OK, "")),
    ("points-no-points", lambda: points(pts=A((0, 2), "float64")), (OK, "")),
    ("points-no-points-inverse", lambda: points(inverse=1, pts=A((0, 2), "float32"), status=A((0,), "uint8")),
     (OK, "")),
    # ---- edhip_deform_labels ---------------------------------------------------------------------------------------
    ("labels-negative-batch", lambda: labels(nb=-1), (INVALID, M_BATCH)),
    ("labels-null-input", lambda: labels(inp=None, out=L8), (INVALID, M_BATCH)),
    ("labels-null-displacement", lambda: labels(disp=None), (INVALID, M_BATCH)),
    ("labels-null-axis", lambda: labels(axis=None), (INVALID, M_AXES)),
    ("labels-naxis-0", lambda: labels(naxis=0), (INVALID, M_AXES)),
    ("labels-naxis-4", lambda: labels(inp=A((3,) * 4, "uint8"), disp=A((4, 2, 2, 2, 2), "float64"), naxis=4,
                                      axis=(0, 1, 2, 3)),
     (UNSUPPORTED, "edhip_deform_labels takes 1 to 3 deformed axes")),
    ("labels-naxis-8+displacement+raw", lambda: labels(naxis=8, axis=AX8, flags=RAW),
     (UNSUPPORTED, "edhip_deform_labels takes 1 to 3 deformed axes")),
    ("labels-raw", lambda: labels(flags=RAW), (INVALID, "edhip_deform_labels takes the prefiltered control grid")),
    ("labels-raw+rank", lambda: labels(flags=RAW, out=A((8, 9, 1), "uint8")),
     (INVALID, "edhip_deform_labels takes the prefiltered control grid")),
    ("labels-rank-mismatch", lambda: labels(out=A((8, 9, 1), "uint8")), (INVALID, M_NDIM)),
    ("labels-ndim-0", lambda: labels(inp=H(0, (), 1)), (UNSUPPORTED, M_RANK)),
    ("labels-ndim-9", lambda: labels(inp=H(9, (2,) * 8, 1)), (UNSUPPORTED, M_RANK)),
    ("labels-float", lambda: labels(inp=X),
     (INVALID, "label maps must be integer or bool arrays, input and output of one dtype")),
    ("labels-two-dtypes", lambda: labels(out=A((8, 9), "int8")),
     (INVALID, "label maps must be integer or bool arrays, input and output of one dtype")),
    ("labels-dtype-negative", lambda: labels(inp=H(2, (8, 9), -1)),
     (INVALID, "label maps must be integer or bool arrays, input and output of one dtype")),
    ("labels-float+axis", lambda: labels(inp=X, axis=(0, 2)),
     (INVALID, "label maps must be integer or bool arrays, input and output of one dtype")),
    ("labels-axis-high", lambda: labels(axis=(0, 2)), (INVALID, M_AXIS)),
    ("labels-axis-unsorted", lambda: labels(axis=(1, 0)), (INVALID, M_AXIS)),
    ("labels-axis-repeated", lambda: labels(axis=(1, 1)), (INVALID, M_AXIS)),
    ("labels-axis+mode", lambda: labels(axis=(0, 2), mode=5), (INVALID, M_AXIS)),
    ("labels-mode", lambda: labels(mode=5), (INVALID, M_MODE)),
    ("labels-length-1+mode", lambda: labels(inp=A((8, 1), "uint8"), out=L8, mode=-1), (INVALID, M_MODE)),
    ("labels-mode+displacement", lambda: labels(mode=5, disp=A((2, 3), "float64")), (INVALID, M_MODE)),
    ("labels-displacement-rank", lambda: labels(disp=A((2, 3), "float64")), (INVALID, M_DISP)),
    ("labels-displacement-components", lambda: labels(disp=A((3, 3, 3), "float64")), (INVALID, M_DISP)),
    ("labels-displacement-dtype", lambda: labels(disp=H(3, (2, 3, 3), 13)), (DTYPE, M_DTYPE)),
    ("labels-displacement-empty", lambda: labels(disp=A((2, 3, 0), "float64")), (INVALID, M_DISP)),
    ("labels-displacement+weight", lambda: labels(disp=A((2, 3, 0), "float64"), wt=A((8, 8), "float32")),
     (INVALID, M_DISP)),
    ("labels-weight-shape", lambda: labels(wt=A((8, 8), "float32")),
     (INVALID, "weight must have the shape of the output")),
    ("labels-weight-rank", lambda: labels(wt=A((72,), "float32")),
     (INVALID, "weight must have the shape of the output")),
    ("labels-weight-float64", lambda: labels(wt=A((8, 9), "float64")), (DTYPE, "weight must be float32")),
    ("labels-weight+cval", lambda: labels(wt=A((8, 9), "float64"), cval=2.5), (DTYPE, "weight must be float32")),
    ("labels-cval-fraction", lambda: labels(cval=2.5),
     (INVALID, "cval must be an integer value of the label map's dtype")),
    ("labels-cval-256", lambda: labels(cval=256.0),
     (INVALID, "cval must be an integer value of the label map's dtype")),
    ("labels-cval-nan", lambda: labels(cval=float("nan")),
     (INVALID, "cval must be an integer value of the label map's dtype")),
    ("labels-cval-2^63", lambda: labels(inp=A((8, 9), "int64"), cval=2.0 ** 63),
     (INVALID, "cval must be an integer value of the label map's dtype")),
    ("labels-cval+65536", lambda: labels(cval=2.5, nb=65536),
     (INVALID, "cval must be an integer value of the label map's dtype")),
    ("labels-65536", lambda: labels(nb=65536), (UNSUPPORTED, "edhip_deform_labels: too many samples")),
    ("labels-65536+length-1", lambda: labels(nb=65536, inp=A((8, 1), "uint8"), out=L8),
     (UNSUPPORTED, "edhip_deform_labels: too many samples")),
    ("labels-length-1", lambda: labels(inp=A((8, 1), "uint8"), out=L8), (INVALID, M_LEN2)),
    ("labels-length-1-empty-batch", lambda: labels(nb=0, inp=A((8, 1), "uint8"), out=L8), (INVALID, M_LEN2)),
    ("labels-length-1+step-axes", lambda: labels(inp=A((4, 8, 1), "uint8"), out=A((5, 8, 9), "uint8"), axis=(1, 2)),
     (INVALID, M_LEN2)),
    ("labels-step-axes", lambda: labels(inp=A((4, 8, 9), "uint8"), out=A((5, 8, 9), "uint8"), axis=(1, 2)),
     (INVALID, M_STEP)),
    ("labels-step-axes-empty-batch", lambda: labels(nb=0, inp=A((4, 8, 9), "uint8"), out=A((5, 8, 9), "uint8"),
                                                    axis=(1, 2)), (INVALID, M_STEP)),
    ("labels-empty-batch", lambda: labels(nb=0), (OK, "")),
    ("labels-no-voxels", lambda: labels(out=A((0, 9), "uint8"), wt=A((0, 9), "float32")), (OK, "")),
    ("labels-no-voxels-length-1", lambda: labels(inp=A((1, 9), "uint8"), out=A((0, 9), "uint8")), (OK, "")),
    ("labels-no-steps", lambda: labels(inp=A((0, 8, 9), "uint8"), axis=(1, 2)), (OK, "")),
    ("labels-cval-extremes", lambda: labels(nb=0, inp=A((8, 9), "int64"), cval=-2.0 ** 63), (OK, "")),
    # ---- edhip_deform_points_gradient --------------------------------------------------------------------------------
    ("pgrad-negative-batch", lambda: pgrad(nb=-1), (INVALID, M_BATCH)),
    ("pgrad-null-positions", lambda: pgrad(pos=None, cot=PTS, dpts=PTS), (INVALID, M_BATCH)),
    ("pgrad-null-cotangent", lambda: pgrad(cot=None), (INVALID, M_BATCH)),
    ("pgrad-null-displacement", lambda: pgrad(disp=None, ddisp=D2), (INVALID, M_BATCH)),
    ("pgrad-null-lengths", lambda: pgrad(in_len=None), (INVALID, M_BATCH)),
    ("pgrad-null-cotangent+naxis-0", lambda: pgrad(cot=None, naxis=0), (INVALID, M_BATCH)),
    ("pgrad-naxis-0", lambda: pgrad(naxis=0), (INVALID, M_AXES)),
    ("pgrad-naxis-8", lambda: pgrad(naxis=8, in_len=(4,) * 8), (UNSUPPORTED, M_NAXIS)),
    ("pgrad-naxis-8+raw+none", lambda: pgrad(naxis=8, in_len=(4,) * 8, flags=RAW, dpts=None, ddisp=None, dinv=None),
     (UNSUPPORTED, M_NAXIS)),
    ("pgrad-raw", lambda: pgrad(flags=RAW),
     (INVALID, "edhip_deform_points_gradient takes the prefiltered control grid")),
    ("pgrad-raw+none", lambda: pgrad(flags=RAW, dpts=None, ddisp=None, dinv=None),
     (INVALID, "edhip_deform_points_gradient takes the prefiltered control grid")),
    ("pgrad-none", lambda: pgrad(dpts=None, ddisp=None, dinv=None),
     (INVALID, "none of dpoints, ddisplacement and dinverse_affine is requested")),
    ("pgrad-none+shape", lambda: pgrad(pos=A((5, 3), "float64"), dpts=None, ddisp=None, dinv=None),
     (INVALID, "none of dpoints, ddisplacement and dinverse_affine is requested")),
    ("pgrad-none-empty-batch", lambda: pgrad(nb=0, dpts=None, ddisp=None, dinv=None),
     (INVALID, "none of dpoints, ddisplacement and dinverse_affine is requested")),
    ("pgrad-shape", lambda: pgrad(pos=A((5, 3), "float64")), (INVALID, "positions must have shape (N, naxis)")),
    ("pgrad-rank", lambda: pgrad(pos=A((10,), "float64")), (INVALID, "positions must have shape (N, naxis)")),
    ("pgrad-rank-0", lambda: pgrad(pos=H(0)), (INVALID, "positions must have shape (N, naxis)")),
    ("pgrad-rank-9", lambda: pgrad(pos=H(9, (5, 2) + (1,) * 6, 10)), (INVALID, "positions must have shape (N, naxis)")),
    ("pgrad-negative-count", lambda: pgrad(pos=H(2, (-1, 2), 10)), (INVALID, "positions must have shape (N, naxis)")),
    ("pgrad-cotangent-shape", lambda: pgrad(cot=A((4, 2), "float64")),
     (INVALID, "cotangent must have the shape of positions")),
    ("pgrad-cotangent-rank", lambda: pgrad(cot=A((5, 2, 1), "float64")),
     (INVALID, "cotangent must have the shape of positions")),
    ("pgrad-cotangent-shape+dtype", lambda: pgrad(cot=A((4, 2), "int32")),
     (INVALID, "cotangent must have the shape of positions")),
    ("pgrad-dtype", lambda: pgrad(pos=A((5, 2), "int32"), cot=PTS, dpts=PTS), (DTYPE, M_DTYPE)),
    ("pgrad-cotangent-dtype", lambda: pgrad(cot=A((5, 2), "float16")), (DTYPE, M_DTYPE)),
    ("pgrad-dtype-13", lambda: pgrad(cot=H(2, (5, 2), 13)), (DTYPE, M_DTYPE)),
    ("pgrad-dtype+status-forward", lambda: pgrad(cot=A((5, 2), "float16"), status=A((5,), "uint8")),
     (DTYPE, M_DTYPE)),
    ("pgrad-status-forward", lambda: pgrad(status=A((5,), "uint8")),
     (INVALID, "the status belongs to the inverse direction")),
    ("pgrad-status-forward+shape", lambda: pgrad(status=A((4,), "bool")),
     (INVALID, "the status belongs to the inverse direction")),
    ("pgrad-status-shape", lambda: pgrad(inverse=1, status=A((4,), "uint8")), (INVALID, "status must have shape (N)")),
    ("pgrad-status-rank", lambda: pgrad(inverse=1, status=A((5, 1), "uint8")), (INVALID, "status must have shape (N)")),
    ("pgrad-status-dtype", lambda: pgrad(inverse=1, status=A((5,), "bool")), (DTYPE, "status must be uint8")),
    ("pgrad-status-shape+dtype", lambda: pgrad(inverse=1, status=A((4,), "bool")),
     (INVALID, "status must have shape (N)")),
    ("pgrad-status-dtype+displacement", lambda: pgrad(inverse=1, status=A((5,), "bool"), disp=A((2, 3), "float64"),
                                                      ddisp=None), (DTYPE, "status must be uint8")),
    ("pgrad-displacement-rank", lambda: pgrad(disp=A((2, 3), "float64"), ddisp=None), (INVALID, M_DISP)),
    ("pgrad-displacement-components", lambda: pgrad(disp=A((3, 3, 3), "float64")), (INVALID, M_DISP)),
    ("pgrad-displacement-dtype", lambda: pgrad(disp=H(3, (2, 3, 3), 13), ddisp=D2), (DTYPE, M_DTYPE)),
    ("pgrad-displacement-empty", lambda: pgrad(disp=A((2, 0, 3), "float64")), (INVALID, M_DISP)),
    ("pgrad-displacement-negative", lambda: pgrad(disp=H(3, (2, 3, -3), 10), ddisp=None), (INVALID, M_DISP)),
    ("pgrad-displacement+dpoints", lambda: pgrad(disp=A((2, 0, 3), "float64"), dpts=A((5, 3), "float64")),
     (INVALID, M_DISP)),
    ("pgrad-dpoints-shape", lambda: pgrad(dpts=A((5, 3), "float64")),
     (INVALID, "dpoints must have the shape of positions")),
    ("pgrad-dpoints-rank", lambda: pgrad(dpts=A((10,), "float64")),
     (INVALID, "dpoints must have the shape of positions")),
    ("pgrad-dpoints-dtype", lambda: pgrad(dpts=A((5, 2), "int64")), (DTYPE, M_DTYPE)),
    ("pgrad-dpoints-shape+dtype", lambda: pgrad(dpts=A((4, 2), "int64")),
     (INVALID, "dpoints must have the shape of positions")),
    ("pgrad-dpoints-dtype+ddisp-shape", lambda: pgrad(dpts=A((5, 2), "int64"), ddisp=A((2, 3, 4), "float64")),
     (DTYPE, M_DTYPE)),
    ("pgrad-ddisp-rank", lambda: pgrad(ddisp=A((2, 3), "float64")), (INVALID, M_DDISP)),
    ("pgrad-ddisp-rank-9", lambda: pgrad(ddisp=H(9, (2, 3, 3) + (1,) * 5, 10)), (INVALID, M_DDISP)),
    ("pgrad-ddisp-shape", lambda: pgrad(ddisp=A((2, 3, 4), "float64")), (INVALID, M_DDISP)),
    ("pgrad-ddisp-integer", lambda: pgrad(ddisp=A((2, 3, 3), "int32")),
     (DTYPE, "ddisplacement must have a floating-point dtype")),
    ("pgrad-ddisp-dtype-13", lambda: pgrad(ddisp=H(3, (2, 3, 3), 13)),
     (DTYPE, "ddisplacement must have a floating-point dtype")),
    ("pgrad-ddisp-shape+dtype", lambda: pgrad(ddisp=A((2, 3, 4), "int32")), (INVALID, M_DDISP)),
    ("pgrad-ddisp-dtype+dinv-shape", lambda: pgrad(ddisp=A((2, 3, 3), "int32"), dinv=A((3, 2), "float64")),
     (DTYPE, "ddisplacement must have a floating-point dtype")),
    ("pgrad-dinv-shape", lambda: pgrad(dinv=A((3, 2), "float64")), (INVALID, M_DINV)),
    ("pgrad-dinv-rank", lambda: pgrad(dinv=A((6,), "float64")), (INVALID, M_DINV)),
    ("pgrad-dinv-float32", lambda: pgrad(dinv=A((2, 3), "float32")), (DTYPE, M_DINV64)),
    ("pgrad-dinv-shape+float32", lambda: pgrad(dinv=A((3, 2), "float32")), (INVALID, M_DINV)),
    ("pgrad-dinv-float32+65536", lambda: pgrad(nb=65536, dinv=A((2, 3), "float32")), (DTYPE, M_DINV64)),
    ("pgrad-65536", lambda: pgrad(nb=65536), (UNSUPPORTED, "edhip_deform_points_gradient: too many samples")),
    ("pgrad-65536+length-1", lambda: pgrad(nb=65536, in_len=(8, 1)),
     (UNSUPPORTED, "edhip_deform_points_gradient: too many samples")),
    ("pgrad-length-1", lambda: pgrad(in_len=(8, 1)), (INVALID, M_LEN2)),
    ("pgrad-length-1-empty-batch", lambda: pgrad(nb=0, in_len=(8, 1)), (INVALID, M_LEN2)),
    ("pgrad-length-1-no-points", lambda: pgrad(pos=A((0, 2), "float64"), in_len=(1, 9), ddisp=None, dinv=None),
     (INVALID, M_LEN2)),
    ("pgrad-empty-batch", lambda: pgrad(nb=0), (OK, "")),
    ("pgrad-empty-batch-inverse", lambda: pgrad(inverse=1, nb=0, status=A((5,), "uint8")), (OK, "")),
    ("pgrad-empty-batch-no-points", lambda: pgrad(nb=0, pos=A((0, 2), "float32")), (OK, "")),
    ("pgrad-no-points-rows-only", lambda: pgrad(pos=A((0, 2), "float64"), ddisp=None, dinv=None), (OK, "")),
    ("pgrad-no-points-rows-only-inverse", lambda: pgrad(inverse=1, pos=A((0, 2), "float32"),
                                                        status=A((0,), "uint8"), ddisp=None, dinv=None), (OK, "")),
    # ---- edhip_deform_inverse ----------------------------------------------------------------------------------------
    ("inverse-negative-batch", lambda: inverse(nb=-1), (INVALID, M_BATCH)),
    ("inverse-null-input", lambda: inverse(inp=None), (INVALID, M_BATCH)),
    ("inverse-null-displacement", lambda: inverse(disp=None), (INVALID, M_BATCH)),
    ("inverse-null-output", lambda: inverse(out=None), (INVALID, M_BATCH)),
    ("inverse-null-lengths", lambda: inverse(in_len=None), (INVALID, M_BATCH)),
    ("inverse-null-lengths+null-axis", lambda: inverse(in_len=None, axis=None), (INVALID, M_BATCH)),
    ("inverse-null-axis", lambda: inverse(axis=None), (INVALID, M_AXES)),
    ("inverse-naxis-0", lambda: inverse(naxis=0), (INVALID, M_AXES)),
    ("inverse-naxis-4", lambda: inverse(inp=A((3,) * 4), out=A((3,) * 4), disp=A((4, 2, 2, 2, 2), "float64"),
                                        in_len=(3,) * 4, naxis=4, axis=(0, 1, 2, 3)),
     (UNSUPPORTED, "edhip_deform_inverse takes 1 to 3 deformed axes")),
    ("inverse-naxis-8+displacement+raw", lambda: inverse(naxis=8, axis=AX8, in_len=(4,) * 8, flags=RAW),
     (UNSUPPORTED, "edhip_deform_inverse takes 1 to 3 deformed axes")),
    ("inverse-raw", lambda: inverse(flags=RAW), (INVALID, "edhip_deform_inverse takes the prefiltered control grid")),
    ("inverse-raw+rank", lambda: inverse(flags=RAW, out=A((8, 9, 1))),
     (INVALID, "edhip_deform_inverse takes the prefiltered control grid")),
    ("inverse-rank-mismatch", lambda: inverse(out=A((8, 9, 1))), (INVALID, M_NDIM)),
    ("inverse-ndim-0", lambda: inverse(inp=H(0), out=H(0)), (UNSUPPORTED, M_RANK)),
    ("inverse-ndim-9", lambda: inverse(inp=H(9, (2,) * 8), out=H(9, (2,) * 8)), (UNSUPPORTED, M_RANK)),
    ("inverse-rank-mismatch+ndim-9", lambda: inverse(inp=H(9, (2,) * 8)), (INVALID, M_NDIM)),
    ("inverse-dtype-13", lambda: inverse(inp=H(2, (6, 7), 13)), (DTYPE, M_DTYPE)),
    ("inverse-dtype-negative", lambda: inverse(out=H(2, (8, 9), -1)), (DTYPE, M_DTYPE)),
    ("inverse-dtype+axis", lambda: inverse(inp=H(2, (6, 7), 13), axis=(0, 2)), (DTYPE, M_DTYPE)),
    ("inverse-axis-high", lambda: inverse(axis=(0, 2)), (INVALID, M_AXIS)),
    ("inverse-axis-negative", lambda: inverse(axis=(-1, 1)), (INVALID, M_AXIS)),
    ("inverse-axis+order", lambda: inverse(axis=(0, 2), order=6), (INVALID, M_AXIS)),
    ("inverse-order-6", lambda: inverse(order=6), (INVALID, M_ORDER)),
    ("inverse-order-negative", lambda: inverse(order=-1), (INVALID, M_ORDER)),
    ("inverse-order+mode", lambda: inverse(order=6, mode=5), (INVALID, M_ORDER)),
    ("inverse-mode", lambda: inverse(mode=5), (INVALID, M_MODE)),
    ("inverse-mode+unsorted", lambda: inverse(mode=5, axis=(1, 0)), (INVALID, M_MODE)),
    ("inverse-axis-unsorted", lambda: inverse(inp=A((7, 7)), out=A((9, 9)), in_len=(9, 9), axis=(1, 0)),
     (INVALID, M_AXIS)),
    ("inverse-axis-repeated", lambda: inverse(inp=A((7, 7)), out=A((9, 9)), in_len=(9, 9), axis=(1, 1)),
     (INVALID, M_AXIS)),
    ("inverse-unsorted+two-dtypes", lambda: inverse(out=A((8, 9), "float64"), axis=(1, 0)), (INVALID, M_AXIS)),
    ("inverse-two-dtypes", lambda: inverse(out=A((8, 9), "float64")),
     (DTYPE, "input and output must have one dtype")),
    ("inverse-two-dtypes+half", lambda: inverse(inp=A((6, 7), "float16")),
     (DTYPE, "input and output must have one dtype")),
    ("inverse-half", lambda: inverse(inp=A((6, 7), "float16"), out=A((8, 9), "float16")), (DTYPE, M_DTYPE)),
    ("inverse-bfloat16", lambda: inverse(inp=H(2, (6, 7), 12), out=H(2, (8, 9), 12)), (DTYPE, M_DTYPE)),
    ("inverse-half+extents", lambda: inverse(inp=A((6, 7), "float16"), out=A((8, 10), "float16")), (DTYPE, M_DTYPE)),
    ("inverse-extents", lambda: inverse(out=A((8, 10))),
     (INVALID, "the output's deformed axes must have the extents in_len")),
    ("inverse-extents-first-axis", lambda: inverse(out=A((7, 9))),
     (INVALID, "the output's deformed axes must have the extents in_len")),
    ("inverse-sampled-length-1", lambda: inverse(inp=A((6, 1))), (INVALID, M_LEN2)),
    ("inverse-sampled-length-0", lambda: inverse(inp=A((0, 7))), (INVALID, M_LEN2)),
    ("inverse-first-length-1+second-extents", lambda: inverse(inp=A((1, 7)), out=A((8, 10))), (INVALID, M_LEN2)),
    ("inverse-first-extents+second-length-1", lambda: inverse(inp=A((6, 1)), out=A((7, 9))),
     (INVALID, "the output's deformed axes must have the extents in_len")),
    ("inverse-extents+valid", lambda: inverse(out=A((8, 10)), valid=A((8, 8), "uint8")),
     (INVALID, "the output's deformed axes must have the extents in_len")),
    ("inverse-valid-shape", lambda: inverse(valid=A((8, 8), "uint8")),
     (INVALID, "valid must have the output's deformed shape")),
    ("inverse-valid-rank", lambda: inverse(valid=A((72,), "uint8")),
     (INVALID, "valid must have the output's deformed shape")),
    ("inverse-valid-rank-0", lambda: inverse(valid=H(0, (), 1)),
     (INVALID, "valid must have the output's deformed shape")),
    ("inverse-valid-rank-9", lambda: inverse(valid=H(9, (8, 9) + (1,) * 6, 1)),
     (INVALID, "valid must have the output's deformed shape")),
    ("inverse-valid-step-axes", lambda: inverse(inp=A((4, 6, 7)), out=A((4, 8, 9)), axis=(1, 2),
                                                valid=A((4, 8, 9), "uint8")),
     (INVALID, "valid must have the output's deformed shape")),
    ("inverse-valid-bool", lambda: inverse(valid=A((8, 9), "bool")), (DTYPE, "valid must be uint8")),
    ("inverse-valid-shape+dtype", lambda: inverse(valid=A((8, 8), "bool")),
     (INVALID, "valid must have the output's deformed shape")),
    ("inverse-valid-dtype+max-iter", lambda: inverse(valid=A((8, 9), "bool"), max_iter=0),
     (DTYPE, "valid must be uint8")),
    ("inverse-max-iter", lambda: inverse(max_iter=0), (INVALID, "max_iter must be at least 1")),
    ("inverse-tol", lambda: inverse(tol=0.0), (INVALID, "tol must be positive")),
    ("inverse-tol-nan", lambda: inverse(tol=float("nan")), (INVALID, "tol must be positive")),
    ("inverse-max-iter+tol", lambda: inverse(max_iter=0, tol=0.0), (INVALID, "max_iter must be at least 1")),
    ("inverse-affine-without-linear", lambda: inverse(aff=[1, 0, 0, 0, 1, 0]),
     (INVALID, "forward_linear is required with an affine map")),
    ("inverse-tol+affine-without-linear", lambda: inverse(tol=-1.0, aff=[1, 0, 0, 0, 1, 0]),
     (INVALID, "tol must be positive")),
    ("inverse-tol+displacement", lambda: inverse(tol=0.0, disp=A((2, 3), "float64")),
     (INVALID, "tol must be positive")),
    ("inverse-displacement-rank", lambda: inverse(disp=A((2, 3), "float64")), (INVALID, M_DISP)),
    ("inverse-displacement-components", lambda: inverse(disp=A((3, 3, 3), "float64")), (INVALID, M_DISP)),
    ("inverse-displacement-dtype", lambda: inverse(disp=H(3, (2, 3, 3), 13)), (DTYPE, M_DTYPE)),
    ("inverse-displacement-empty", lambda: inverse(disp=A((2, 3, 0), "float64")), (INVALID, M_DISP)),
    ("inverse-displacement+65536", lambda: inverse(nb=65536, disp=A((2, 0, 3), "float64")), (INVALID, M_DISP)),
    ("inverse-65536", lambda: inverse(nb=65536), (UNSUPPORTED, "edhip_deform_inverse: too many samples")),
    ("inverse-65536+length-1", lambda: inverse(nb=65536, out=A((8, 1)), in_len=(8, 1)),
     (UNSUPPORTED, "edhip_deform_inverse: too many samples")),
    ("inverse-length-1", lambda: inverse(out=A((8, 1)), in_len=(8, 1)), (INVALID, M_LEN2)),
    ("inverse-length-1-empty-batch", lambda: inverse(nb=0, out=A((8, 1)), in_len=(8, 1)), (INVALID, M_LEN2)),
    ("inverse-length-1+step-axes", lambda: inverse(inp=A((4, 6, 7)), out=A((5, 8, 1)), in_len=(8, 1), axis=(1, 2)),
     (INVALID, M_LEN2)),
    ("inverse-step-axes", lambda: inverse(inp=A((4, 6, 7)), out=A((5, 8, 9)), axis=(1, 2)), (INVALID, M_STEP)),
    ("inverse-step-axes-empty-batch", lambda: inverse(nb=0, inp=A((4, 6, 7)), out=A((5, 8, 9)), axis=(1, 2)),
     (INVALID, M_STEP)),
    ("inverse-empty-batch", lambda: inverse(nb=0), (OK, "")),
    ("inverse-empty-batch-valid-affine", lambda: inverse(nb=0, valid=A((8, 9), "uint8"), aff=[1, 0, 0, 0, 1, 0],
                                                         lin=[1, 0, 0, 1]), (OK, "")),
    ("inverse-no-steps", lambda: inverse(inp=A((0, 6, 7)), out=A((0, 8, 9)), axis=(1, 2)), (OK, "")),
    ("inverse-no-steps-valid", lambda: inverse(inp=A((6, 0, 7), "int16"), out=A((8, 0, 9), "int16"), axis=(0, 2),
                                               valid=A((8, 9), "uint8")), (OK, "")),
]


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name,call,want", CASES, ids=[c[0] for c in CASES])
def test_status_and_message(name, call, want):
    assert call() == want


def test_a_null_error_buffer_is_allowed():
    """err may be NULL (include/edhip.h): the status alone answers"""
    L = _lib.load()
    one = arr([X])
    assert L.edhip_deform(0, 1, one, ref(D2), None, one, 2, i32([0, 1]), i32([6]), i32([4]), f64([0.0]), None, 0,
                          None, None, 0) == INVALID
    assert L.edhip_spline_filter1d(ref(X), ref(X), 5, 3, 0, 0, None, None, 0) == INVALID
    assert L.edhip_deform_labels(1, ref(L8), 0, ref(D2), 0, None, ref(L8), 0, None, 0, 2, i32([0, 1]), 9, 0.0, None,
                                 0, None, None, 0) == INVALID
