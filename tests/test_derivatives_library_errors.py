"""
CPU tests that pin the answers of edhip_deform_points_derivatives and edhip_deform_points_derivatives_gradient at the
boundary: the exact (status, message) pair of every refusal before the device is touched, the message that wins when
two arguments are wrong, and the "nothing to do" successes.  The raw ctypes functions are called with descriptors of
memory that does not exist; every case returns before any allocation or launch, so no GPU is needed.
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
M_POINTS = "points must have shape (N, naxis)"
M_POSITIONS = "positions must have shape (N, naxis)"
M_RESULT = "result must have the shape of points"
M_NO_COT = "none of dresult, djacobian and dhessian is given"
M_NO_RESULT = "none of dpoints, ddisplacement and dinverse_affine is requested"
M_DDISP = "ddisplacement must have the shape of displacement"
M_DDISP_DTYPE = "ddisplacement must have a floating-point dtype"
M_DINV = "dinverse_affine must have shape (naxis, naxis + 1)"
M_DINV64 = "dinverse_affine must be float64"
F = "edhip_deform_points_derivatives"
G = "edhip_deform_points_derivatives_gradient"


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


N = 5
D2 = A((2, 3, 3))
P2, J2, H2, DINV2 = A((N, 2)), A((N, 2, 2)), A((N, 2, 2, 2)), A((2, 3))
D4, P4 = A((4, 2, 2, 2, 2)), A((N, 4))
BIG = A((2, 64, 64))                          # 8192 values: read from global memory
_DEF = object()


def forward(nb=1, pts=P2, disp=D2, in_len=(8, 9), off=None, naxis=2, aff=None, res=P2, jac=J2, hess=H2, flags=0):
    return run(_lib.load().edhip_deform_points_derivatives, nb, ref(pts), 0, ref(disp), 0, i64(in_len), i64(off), naxis,
               f64(aff), ref(res), 0, ref(jac), 0, ref(hess), 0, flags, None)


def gradient(nb=1, pos=P2, du=P2, dj=J2, dh=H2, disp=D2, in_len=(8, 9), off=None, naxis=2, aff=None, dpts=P2,
             ddisp=_DEF, dinv=DINV2, flags=0):
    ddisp = disp if ddisp is _DEF else ddisp
    return run(_lib.load().edhip_deform_points_derivatives_gradient, nb, ref(pos), 0, ref(du), 0, ref(dj), 0, ref(dh), 0,
               ref(disp), 0, i64(in_len), i64(off), naxis, f64(aff), ref(dpts), 0, ref(ddisp), 0, ref(dinv), 0, flags,
               None)


CASES = [
    # ---- edhip_deform_points_derivatives: one case per refusal, in the order of the checks ------------------------
    ("forward-negative-batch", lambda: forward(nb=-1), (INVALID, M_BATCH)),
    ("forward-null-points", lambda: forward(pts=None), (INVALID, M_BATCH)),
    ("forward-null-displacement", lambda: forward(disp=None), (INVALID, M_BATCH)),
    ("forward-null-result", lambda: forward(res=None), (INVALID, M_BATCH)),
    ("forward-null-lengths", lambda: forward(in_len=None), (INVALID, M_BATCH)),
    ("forward-naxis-0", lambda: forward(naxis=0), (INVALID, M_AXES)),
    ("forward-naxis-4", lambda: forward(naxis=4, disp=D4, in_len=(5,) * 4, pts=P4, res=P4, jac=None, hess=None),
     (UNSUPPORTED, F + " takes 1 to 3 deformed axes")),
    ("forward-naxis-8", lambda: forward(naxis=8), (UNSUPPORTED, "more than 7 deformed axes are not supported on the GPU")),
    ("forward-raw", lambda: forward(flags=RAW), (INVALID, F + " takes the prefiltered control grid")),
    ("forward-points-rank", lambda: forward(pts=A((N,))), (INVALID, M_POINTS)),
    ("forward-points-columns", lambda: forward(pts=A((N, 3))), (INVALID, M_POINTS)),
    ("forward-result-shape", lambda: forward(res=A((N + 1, 2))), (INVALID, M_RESULT)),
    ("forward-points-dtype", lambda: forward(pts=A((N, 2), "float16")), (DTYPE, M_DTYPE)),
    ("forward-result-dtype", lambda: forward(res=A((N, 2), "int32")), (DTYPE, M_DTYPE)),
    ("forward-jacobian-shape", lambda: forward(jac=A((N, 2))), (INVALID, "jacobian must have shape (N, naxis, naxis)")),
    ("forward-jacobian-float32", lambda: forward(jac=A((N, 2, 2), "float32")), (DTYPE, "jacobian must be float64")),
    ("forward-hessian-shape", lambda: forward(hess=A((N, 2, 2))),
     (INVALID, "hessian must have shape (N, naxis, naxis, naxis)")),
    ("forward-hessian-extent", lambda: forward(hess=A((N, 2, 2, 3))),
     (INVALID, "hessian must have shape (N, naxis, naxis, naxis)")),
    ("forward-hessian-float32", lambda: forward(hess=A((N, 2, 2, 2), "float32")), (DTYPE, "hessian must be float64")),
    ("forward-displacement-rank", lambda: forward(disp=A((2, 3))), (INVALID, M_DISP)),
    ("forward-displacement-components", lambda: forward(disp=A((3, 3, 3))), (INVALID, M_DISP)),
    ("forward-displacement-dtype", lambda: forward(disp=H(3, (2, 3, 3), 13)), (DTYPE, M_DTYPE)),
    ("forward-displacement-empty", lambda: forward(disp=A((2, 0, 3))), (INVALID, M_DISP)),
    ("forward-65536", lambda: forward(nb=65536), (UNSUPPORTED, F + ": too many samples")),
    ("forward-length-1", lambda: forward(in_len=(8, 1)), (INVALID, M_LEN2)),
    # ---- which message wins ------------------------------------------------------------------------------------
    ("forward-negative-batch+naxis-4", lambda: forward(nb=-1, naxis=4), (INVALID, M_BATCH)),
    ("forward-naxis-4+raw", lambda: forward(naxis=4, flags=RAW), (UNSUPPORTED, F + " takes 1 to 3 deformed axes")),
    ("forward-raw+points", lambda: forward(flags=RAW, pts=A((N,))), (INVALID, F + " takes the prefiltered control grid")),
    ("forward-result-shape+dtype", lambda: forward(res=A((N, 3), "int8")), (INVALID, M_RESULT)),
    ("forward-hessian+displacement", lambda: forward(hess=A((N, 2, 2)), disp=A((2, 3))),
     (INVALID, "hessian must have shape (N, naxis, naxis, naxis)")),
    ("forward-displacement+65536", lambda: forward(nb=65536, disp=A((2, 0, 3))), (INVALID, M_DISP)),
    ("forward-65536+length-1", lambda: forward(nb=65536, in_len=(8, 1)), (UNSUPPORTED, F + ": too many samples")),
    # ---- nothing to do -------------------------------------------------------------------------------------------
    ("forward-length-1-empty-batch", lambda: forward(nb=0, in_len=(8, 1)), (INVALID, M_LEN2)),
    ("forward-empty-batch", lambda: forward(nb=0), (OK, "")),
    ("forward-no-points", lambda: forward(pts=A((0, 2)), res=A((0, 2)), jac=A((0, 2, 2)), hess=A((0, 2, 2, 2))),
     (OK, "")),
    ("forward-no-points-float32-no-hessian-global-grid",
     lambda: forward(pts=A((0, 2), "float32"), res=A((0, 2), "float32"), jac=None, hess=None, disp=BIG,
                     aff=[1, 0, 0, 0, 1, 0], off=(1, 2)), (OK, "")),
    # ---- edhip_deform_points_derivatives_gradient ----------------------------------------------------------------
    ("gradient-negative-batch", lambda: gradient(nb=-1), (INVALID, M_BATCH)),
    ("gradient-null-positions", lambda: gradient(pos=None), (INVALID, M_BATCH)),
    ("gradient-null-displacement", lambda: gradient(disp=None, ddisp=D2), (INVALID, M_BATCH)),
    ("gradient-null-lengths", lambda: gradient(in_len=None), (INVALID, M_BATCH)),
    ("gradient-naxis-0", lambda: gradient(naxis=0), (INVALID, M_AXES)),
    ("gradient-naxis-4", lambda: gradient(naxis=4, disp=D4, in_len=(5,) * 4, pos=P4, du=P4, dj=None, dh=None, dpts=P4,
                                          dinv=A((4, 5))), (UNSUPPORTED, G + " takes 1 to 3 deformed axes")),
    ("gradient-raw", lambda: gradient(flags=RAW), (INVALID, G + " takes the prefiltered control grid")),
    ("gradient-no-cotangent", lambda: gradient(du=None, dj=None, dh=None), (INVALID, M_NO_COT)),
    ("gradient-no-result", lambda: gradient(dpts=None, ddisp=None, dinv=None), (INVALID, M_NO_RESULT)),
    ("gradient-positions-shape", lambda: gradient(pos=A((N, 3))), (INVALID, M_POSITIONS)),
    ("gradient-positions-dtype", lambda: gradient(pos=A((N, 2), "int64")), (DTYPE, M_DTYPE)),
    ("gradient-dresult-shape", lambda: gradient(du=A((N + 1, 2))), (INVALID, "dresult must have shape (N, naxis)")),
    ("gradient-dresult-dtype", lambda: gradient(du=A((N, 2), "float16")),
     (DTYPE, "dresult must be float32 or float64")),
    ("gradient-djacobian-shape", lambda: gradient(dj=A((N, 2, 3))),
     (INVALID, "djacobian must have shape (N, naxis, naxis)")),
    ("gradient-djacobian-dtype", lambda: gradient(dj=A((N, 2, 2), "int32")),
     (DTYPE, "djacobian must be float32 or float64")),
    ("gradient-dhessian-shape", lambda: gradient(dh=A((N, 2, 2))),
     (INVALID, "dhessian must have shape (N, naxis, naxis, naxis)")),
    ("gradient-dhessian-dtype", lambda: gradient(dh=A((N, 2, 2, 2), "float16")),
     (DTYPE, "dhessian must be float32 or float64")),
    ("gradient-displacement-rank", lambda: gradient(disp=A((2, 3)), ddisp=D2), (INVALID, M_DISP)),
    ("gradient-displacement-dtype", lambda: gradient(disp=H(3, (2, 3, 3), -1), ddisp=D2), (DTYPE, M_DTYPE)),
    ("gradient-dpoints-shape", lambda: gradient(dpts=A((N, 1))), (INVALID, "dpoints must have shape (N, naxis)")),
    ("gradient-dpoints-dtype", lambda: gradient(dpts=A((N, 2), "int8")), (DTYPE, "dpoints must be float32 or float64")),
    ("gradient-ddisp-shape", lambda: gradient(ddisp=A((2, 3, 4))), (INVALID, M_DDISP)),
    ("gradient-ddisp-integer", lambda: gradient(ddisp=A((2, 3, 3), "int64")), (DTYPE, M_DDISP_DTYPE)),
    ("gradient-dinv-shape", lambda: gradient(dinv=A((3, 2))), (INVALID, M_DINV)),
    ("gradient-dinv-float32", lambda: gradient(dinv=A((2, 3), "float32")), (DTYPE, M_DINV64)),
    ("gradient-65536", lambda: gradient(nb=65536), (UNSUPPORTED, G + ": too many samples")),
    ("gradient-length-1", lambda: gradient(in_len=(1, 9)), (INVALID, M_LEN2)),
    # ---- which message wins ------------------------------------------------------------------------------------
    ("gradient-raw+no-cotangent", lambda: gradient(flags=RAW, du=None, dj=None, dh=None),
     (INVALID, G + " takes the prefiltered control grid")),
    ("gradient-no-cotangent+no-result", lambda: gradient(du=None, dj=None, dh=None, dpts=None, ddisp=None, dinv=None),
     (INVALID, M_NO_COT)),
    ("gradient-no-result+positions", lambda: gradient(dpts=None, ddisp=None, dinv=None, pos=A((N,))),
     (INVALID, M_NO_RESULT)),
    ("gradient-dhessian-dtype+displacement", lambda: gradient(dh=A((N, 2, 2, 2), "int16"), disp=A((2, 3)), ddisp=D2),
     (DTYPE, "dhessian must be float32 or float64")),
    ("gradient-displacement+ddisp", lambda: gradient(disp=A((3, 3, 3)), ddisp=A((2, 3, 4))), (INVALID, M_DISP)),
    ("gradient-ddisp-shape+dinv-float32", lambda: gradient(ddisp=A((2, 3, 4)), dinv=A((2, 3), "float32")),
     (INVALID, M_DDISP)),
    ("gradient-dinv-float32+65536", lambda: gradient(nb=65536, dinv=A((2, 3), "float32")), (DTYPE, M_DINV64)),
    ("gradient-65536+length-1", lambda: gradient(nb=65536, in_len=(8, 1)), (UNSUPPORTED, G + ": too many samples")),
    # ---- nothing to do -------------------------------------------------------------------------------------------
    ("gradient-empty-batch", lambda: gradient(nb=0), (OK, "")),
    ("gradient-empty-batch-float32-cotangents",
     lambda: gradient(nb=0, du=A((N, 2), "float32"), dj=None, dh=A((N, 2, 2, 2), "float32"), disp=BIG), (OK, "")),
    ("gradient-no-points-rows-only", lambda: gradient(pos=A((0, 2)), du=A((0, 2)), dj=None, dh=None, dpts=A((0, 2)),
                                                      ddisp=None, dinv=None), (OK, "")),
    ("gradient-empty-batch-no-result", lambda: gradient(nb=0, dpts=None, ddisp=None, dinv=None),
     (INVALID, M_NO_RESULT)),
]


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name,call,want", CASES, ids=[c[0] for c in CASES])
def test_status_and_message(name, call, want):
    assert call() == want


def test_a_null_error_buffer_is_allowed():
    L = _lib.load()
    assert L.edhip_deform_points_derivatives(1, ref(P2), 0, ref(D2), 0, i64((8, 9)), None, 4, None, ref(P2), 0, None, 0,
                                             None, 0, 0, None, None, 0) == UNSUPPORTED
    assert L.edhip_deform_points_derivatives_gradient(1, ref(P2), 0, None, 0, None, 0, None, 0, ref(D2), 0, i64((8, 9)),
                                                      None, 2, None, ref(P2), 0, None, 0, None, 0, 0, None, None,
                                                      0) == INVALID
