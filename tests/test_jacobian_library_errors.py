"""
CPU tests that pin the answers of edhip_deform_jacobian and edhip_deform_jacobian_gradient at the boundary: the exact
(status, message) pair of every refusal before the device is touched, the message that wins when two arguments are
wrong, and the "nothing to do" successes.  The raw ctypes functions are called with descriptors of memory that does
not exist; every case returns before any allocation or launch, so no GPU is needed.
"""
import ctypes
import os

import numpy as np
import pytest

from elasticdeform_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                                reason="libedhip.so not built (run __graft_entry__.build())")

OK, INVALID, DTYPE, UNSUPPORTED = 0, 1, 2, 5
RAW = _lib.FLAG_RAW_DISPLACEMENT

M_BATCH = "invalid batch"
M_AXES = "invalid axis list"
M_DISP = "invalid displacement shape"
M_DTYPE = "data type not supported"
M_LEN2 = "deformed axes must have at least 2 elements"
M_NEITHER = "none of ddisplacement and dinverse_affine is requested"
M_DDISP = "ddisplacement must have the shape of displacement"
M_DDISP_DTYPE = "ddisplacement must be float32 or float64"
M_DINV = "dinverse_affine must have shape (naxis, naxis + 1)"
M_DINV64 = "dinverse_affine must be float64"
F = "edhip_deform_jacobian"
G = "edhip_deform_jacobian_gradient"


def A(shape, dtype="float64", ptr=0x1000):
    """descriptor of a C-contiguous array that does not exist"""
    a = np.empty(shape, dtype=dtype)
    return _lib.describe(ptr, a.dtype.name, a.shape, a.strides)


def H(ndim, shape=(), dtype=10, ptr=0x1000):
    """a hostile descriptor: any rank, any extents, any dtype code"""
    shape = tuple(shape) + (0,) * (8 - len(shape))
    return _lib.EdhipArray(ptr, dtype, ndim, (ctypes.c_int64 * 8)(*shape), (ctypes.c_int64 * 8)(*([8] * 8)))


def ref(d):
    return ctypes.byref(d) if d is not None else None


def i64(v):
    return (ctypes.c_int64 * len(v))(*v) if v is not None else None


def f64(v):
    return (ctypes.c_double * len(v))(*v) if v is not None else None


def run(fn, *args):
    buf = ctypes.create_string_buffer(b"stale", 256)
    st = fn(*args, buf, 256)
    return st, buf.value.decode()


D2, DET2, DINV2 = A((2, 3, 3)), A((8, 9)), A((2, 3))
D4 = A((4, 2, 2, 2, 2))
WIDE = A((2, 3, 129))                        # 2 * 2 * 129 = 516 values a row: beyond the forward's row contraction
_DEF = object()


def forward(nb=1, disp=D2, in_len=(8, 9), off=None, naxis=2, aff=None, det=DET2, flags=0):
    return run(_lib.load().edhip_deform_jacobian, nb, ref(disp), 0, i64(in_len), i64(off), naxis, f64(aff), ref(det), 0,
               flags, None)


def gradient(nb=1, ddet=DET2, disp=D2, in_len=(8, 9), off=None, naxis=2, aff=None, ddisp=_DEF, dinv=_DEF, flags=0):
    ddisp = disp if ddisp is _DEF else ddisp
    dinv = DINV2 if dinv is _DEF else dinv
    return run(_lib.load().edhip_deform_jacobian_gradient, nb, ref(ddet), 0, ref(disp), 0, i64(in_len), i64(off), naxis,
               f64(aff), ref(ddisp), 0, ref(dinv), 0, flags, None)


CASES = [
    # ---- edhip_deform_jacobian: one case per refusal, in the order of the checks --------------------------------
    ("forward-negative-batch", lambda: forward(nb=-1), (INVALID, M_BATCH)),
    ("forward-null-displacement", lambda: forward(disp=None), (INVALID, M_BATCH)),
    ("forward-null-det", lambda: forward(det=None), (INVALID, M_BATCH)),
    ("forward-null-lengths", lambda: forward(in_len=None), (INVALID, M_BATCH)),
    ("forward-naxis-0", lambda: forward(naxis=0), (INVALID, M_AXES)),
    ("forward-naxis-4", lambda: forward(naxis=4, disp=D4, in_len=(5,) * 4, det=A((5,) * 4)),
     (UNSUPPORTED, F + " takes 1 to 3 deformed axes")),
    ("forward-raw", lambda: forward(flags=RAW), (INVALID, F + " takes the prefiltered control grid")),
    ("forward-det-rank", lambda: forward(det=A((8, 9, 1))), (INVALID, "det must have one dimension per deformed axis")),
    ("forward-det-dtype", lambda: forward(det=A((8, 9), "float16")), (DTYPE, "det must be float32 or float64")),
    ("forward-det-integer", lambda: forward(det=A((8, 9), "int32")), (DTYPE, "det must be float32 or float64")),
    ("forward-displacement-rank", lambda: forward(disp=A((2, 3))), (INVALID, M_DISP)),
    ("forward-displacement-components", lambda: forward(disp=A((3, 3, 3))), (INVALID, M_DISP)),
    ("forward-displacement-dtype", lambda: forward(disp=H(3, (2, 3, 3), 13)), (DTYPE, M_DTYPE)),
    ("forward-displacement-empty", lambda: forward(disp=A((2, 0, 3))), (INVALID, M_DISP)),
    ("forward-65536", lambda: forward(nb=65536), (UNSUPPORTED, F + ": too many samples")),
    ("forward-length-1", lambda: forward(in_len=(8, 1)), (INVALID, M_LEN2)),
    # ---- which message wins ------------------------------------------------------------------------------------
    ("forward-negative-batch+naxis-4", lambda: forward(nb=-1, naxis=4), (INVALID, M_BATCH)),
    ("forward-naxis-8+raw+displacement", lambda: forward(naxis=8, flags=RAW, disp=A((2, 3))),
     (UNSUPPORTED, F + " takes 1 to 3 deformed axes")),
    ("forward-raw+det-rank", lambda: forward(flags=RAW, det=A((8,))), (INVALID, F + " takes the prefiltered control grid")),
    ("forward-det-rank+dtype", lambda: forward(det=A((8,), "int8")),
     (INVALID, "det must have one dimension per deformed axis")),
    ("forward-det-dtype+displacement", lambda: forward(det=A((8, 9), "uint8"), disp=A((2, 3))),
     (DTYPE, "det must be float32 or float64")),
    ("forward-displacement+65536", lambda: forward(nb=65536, disp=A((2, 0, 3))), (INVALID, M_DISP)),
    ("forward-65536+length-1", lambda: forward(nb=65536, in_len=(8, 1)), (UNSUPPORTED, F + ": too many samples")),
    # ---- nothing to do -------------------------------------------------------------------------------------------
    ("forward-length-1-empty-batch", lambda: forward(nb=0, in_len=(8, 1)), (INVALID, M_LEN2)),
    ("forward-empty-batch", lambda: forward(nb=0), (OK, "")),
    ("forward-no-voxels", lambda: forward(det=A((0, 9))), (OK, "")),
    ("forward-no-voxels-float32-affine", lambda: forward(det=A((8, 0), "float32"), aff=[1, 0, 0, 0, 1, 0], off=(1, 2)),
     (OK, "")),
    ("forward-length-0-no-voxels", lambda: forward(det=A((0, 9)), in_len=(0, 9)), (OK, "")),
    # ---- edhip_deform_jacobian_gradient --------------------------------------------------------------------------
    ("gradient-negative-batch", lambda: gradient(nb=-1), (INVALID, M_BATCH)),
    ("gradient-null-ddet", lambda: gradient(ddet=None), (INVALID, M_BATCH)),
    ("gradient-null-displacement", lambda: gradient(disp=None, ddisp=D2), (INVALID, M_BATCH)),
    ("gradient-null-lengths", lambda: gradient(in_len=None), (INVALID, M_BATCH)),
    ("gradient-naxis-0", lambda: gradient(naxis=0), (INVALID, M_AXES)),
    ("gradient-naxis-4", lambda: gradient(naxis=4, disp=D4, in_len=(5,) * 4, ddet=A((5,) * 4), dinv=A((4, 5))),
     (UNSUPPORTED, G + " takes 1 to 3 deformed axes")),
    ("gradient-raw", lambda: gradient(flags=RAW), (INVALID, G + " takes the prefiltered control grid")),
    ("gradient-neither", lambda: gradient(ddisp=None, dinv=None), (INVALID, M_NEITHER)),
    ("gradient-ddet-rank", lambda: gradient(ddet=A((8,))), (INVALID, "ddet must have one dimension per deformed axis")),
    ("gradient-ddet-dtype", lambda: gradient(ddet=A((8, 9), "float16")), (DTYPE, "ddet must be float32 or float64")),
    ("gradient-displacement-rank", lambda: gradient(disp=A((2, 3)), ddisp=D2), (INVALID, M_DISP)),
    ("gradient-displacement-dtype", lambda: gradient(disp=H(3, (2, 3, 3), -1), ddisp=D2), (DTYPE, M_DTYPE)),
    ("gradient-ddisp-rank", lambda: gradient(ddisp=A((2, 3))), (INVALID, M_DDISP)),
    ("gradient-ddisp-shape", lambda: gradient(ddisp=A((2, 3, 4))), (INVALID, M_DDISP)),
    ("gradient-ddisp-half", lambda: gradient(ddisp=A((2, 3, 3), "float16")), (DTYPE, M_DDISP_DTYPE)),
    ("gradient-ddisp-integer", lambda: gradient(ddisp=A((2, 3, 3), "int64")), (DTYPE, M_DDISP_DTYPE)),
    ("gradient-dinv-shape", lambda: gradient(dinv=A((3, 2))), (INVALID, M_DINV)),
    ("gradient-dinv-rank", lambda: gradient(ddisp=None, dinv=A((6,))), (INVALID, M_DINV)),
    ("gradient-dinv-float32", lambda: gradient(ddisp=None, dinv=A((2, 3), "float32")), (DTYPE, M_DINV64)),
    ("gradient-65536", lambda: gradient(nb=65536), (UNSUPPORTED, G + ": too many samples")),
    ("gradient-length-1", lambda: gradient(in_len=(1, 9)), (INVALID, M_LEN2)),
    # ---- which message wins ------------------------------------------------------------------------------------
    ("gradient-raw+neither", lambda: gradient(flags=RAW, ddisp=None, dinv=None),
     (INVALID, G + " takes the prefiltered control grid")),
    ("gradient-neither+ddet-rank", lambda: gradient(ddisp=None, dinv=None, ddet=A((8,))), (INVALID, M_NEITHER)),
    ("gradient-ddet-dtype+displacement", lambda: gradient(ddet=A((8, 9), "int16"), disp=A((2, 3)), ddisp=D2),
     (DTYPE, "ddet must be float32 or float64")),
    ("gradient-displacement+ddisp", lambda: gradient(disp=A((3, 3, 3)), ddisp=A((2, 3, 4))), (INVALID, M_DISP)),
    ("gradient-ddisp-shape+dtype", lambda: gradient(ddisp=A((2, 3, 4), "float16")), (INVALID, M_DDISP)),
    ("gradient-ddisp-shape+dinv-float32", lambda: gradient(ddisp=A((2, 3, 4)), dinv=A((2, 3), "float32")),
     (INVALID, M_DDISP)),
    ("gradient-dinv-float32+65536", lambda: gradient(nb=65536, dinv=A((2, 3), "float32")), (DTYPE, M_DINV64)),
    ("gradient-65536+length-1", lambda: gradient(nb=65536, in_len=(8, 1)), (UNSUPPORTED, G + ": too many samples")),
    # ---- nothing to do -------------------------------------------------------------------------------------------
    ("gradient-empty-batch", lambda: gradient(nb=0), (OK, "")),
    ("gradient-empty-batch-wide-grid", lambda: gradient(nb=0, disp=WIDE), (OK, "")),
    ("gradient-empty-batch-neither", lambda: gradient(nb=0, ddisp=None, dinv=None), (INVALID, M_NEITHER)),
]


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name,call,want", CASES, ids=[c[0] for c in CASES])
def test_status_and_message(name, call, want):
    assert call() == want


def test_a_null_error_buffer_is_allowed():
    L = _lib.load()
    assert L.edhip_deform_jacobian(1, ref(D2), 0, i64((8, 9)), None, 4, None, ref(DET2), 0, 0, None, None, 0) == UNSUPPORTED
    assert L.edhip_deform_jacobian_gradient(1, ref(DET2), 0, ref(D2), 0, i64((8, 9)), None, 2, None, None, 0, None, 0, 0,
                                            None, None, 0) == INVALID
