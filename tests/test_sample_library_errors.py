"""
CPU tests that pin the answers of edhip_deform_sample and edhip_deform_sample_gradient at the boundary: the exact
(status, message) pair of every refusal before the device is touched, one per check in the order of the checks, the
message that wins when two arguments are wrong, and the "nothing to do" successes.  The raw ctypes functions are called
with descriptors of memory that does not exist; every case returns before any launch, so no GPU is needed.
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
M_AXIS = "invalid axis in axis list"
M_DISP = "invalid displacement shape"
M_DTYPE = "data type not supported"
M_LEN2 = "deformed axes must have at least 2 elements"
M_POINTS = "points must have shape (N, naxis)"
M_POINTS_DTYPE = "points must be float32 or float64"
F = "edhip_deform_sample"
G = "edhip_deform_sample_gradient"


def A(shape, dtype="float64", ptr=0x1000):
    """descriptor of a C-contiguous array that does not exist"""
    a = np.empty(shape, dtype=dtype)
    return _lib.describe(ptr, a.dtype.name, a.shape, a.strides)


def ref(d):
    return ctypes.byref(d) if d is not None else None


def i64(v):
    return (ctypes.c_int64 * len(v))(*v) if v is not None else None


def i32(v):
    return (ctypes.c_int32 * len(v))(*v) if v is not None else None


def run(fn, *args):
    buf = ctypes.create_string_buffer(b"stale", 256)
    st = fn(*args, buf, 256)
    return st, buf.value.decode()


X2, P2, D2, V2, IN2, G2 = A((2, 8, 9)), A((5, 2)), A((2, 3, 3)), A((2, 5)), A((5,), "uint8"), A((5, 2))
_DEF = object()


def forward(nb=1, x=X2, pts=P2, disp=D2, in_len=(8, 9), off=None, out=V2, inside=None, naxis=2, axis=(1, 2), order=3,
            mode=0, flags=0):
    return run(_lib.load().edhip_deform_sample, nb, ref(x), 0, ref(pts), 0, ref(disp), 0, i64(in_len), i64(off),
               ref(out), 0, ref(inside), 0, naxis, i32(axis), order, mode, 0.0, None, flags, None)


def gradient(nb=1, x=X2, cot=V2, pts=P2, disp=D2, in_len=(8, 9), din=_DEF, dcoord=_DEF, naxis=2, axis=(1, 2), order=3,
             mode=0, flags=0):
    din = X2 if din is _DEF else din
    dcoord = G2 if dcoord is _DEF else dcoord
    return run(_lib.load().edhip_deform_sample_gradient, nb, ref(x), 0, ref(cot), 0, ref(pts), 0, ref(disp), 0,
               i64(in_len), None, ref(din), 0, ref(dcoord), 0, naxis, i32(axis), order, mode, None, flags, None)


M_OUT = "output must have the input's non-deformed axes and one axis of N points"
M_COT = "cotangent must have the input's non-deformed axes and one axis of N points"

CASES = [
    # ---- edhip_deform_sample: one case per refusal, in the order of the checks ------------------------------------
    ("forward-negative-batch", lambda: forward(nb=-1), (INVALID, M_BATCH)),
    ("forward-null-input", lambda: forward(x=None), (INVALID, M_BATCH)),
    ("forward-null-points", lambda: forward(pts=None), (INVALID, M_BATCH)),
    ("forward-null-displacement", lambda: forward(disp=None), (INVALID, M_BATCH)),
    ("forward-null-output", lambda: forward(out=None), (INVALID, M_BATCH)),
    ("forward-null-lengths", lambda: forward(in_len=None), (INVALID, M_BATCH)),
    ("forward-null-axis", lambda: forward(axis=None), (INVALID, M_AXES)),
    ("forward-naxis-0", lambda: forward(naxis=0), (INVALID, M_AXES)),
    ("forward-naxis-4", lambda: forward(naxis=4, axis=(0, 1, 2, 3)), (UNSUPPORTED, F + " takes 1 to 3 deformed axes")),
    ("forward-raw", lambda: forward(flags=RAW), (INVALID, F + " takes the prefiltered control grid")),
    ("forward-axis-out-of-range", lambda: forward(axis=(1, 3)), (INVALID, M_AXIS)),
    ("forward-axis-descending", lambda: forward(axis=(2, 1)), (INVALID, M_AXIS)),
    ("forward-order-6", lambda: forward(order=6), (INVALID, "spline order not supported")),
    ("forward-mode-5", lambda: forward(mode=5), (INVALID, "boundary mode not supported")),
    ("forward-half", lambda: forward(x=A((2, 8, 9), "float16"), out=A((2, 5), "float16")), (DTYPE, M_DTYPE)),
    ("forward-output-dtype", lambda: forward(out=A((2, 5), "float32")),
     (DTYPE, "input and output must have one dtype")),
    ("forward-lengths", lambda: forward(in_len=(8, 10)),
     (INVALID, "the input's deformed axes must have the extents in_len")),
    ("forward-length-1", lambda: forward(x=A((2, 8, 1)), in_len=(8, 1)), (INVALID, M_LEN2)),
    ("forward-points-rank", lambda: forward(pts=A((5, 2, 1))), (INVALID, M_POINTS)),
    ("forward-points-columns", lambda: forward(pts=A((5, 3))), (INVALID, M_POINTS)),
    ("forward-points-dtype", lambda: forward(pts=A((5, 2), "int32")), (DTYPE, M_POINTS_DTYPE)),
    ("forward-output-rank", lambda: forward(out=A((2, 5, 1))), (INVALID, M_OUT)),
    ("forward-output-points", lambda: forward(out=A((2, 6))), (INVALID, M_OUT)),
    ("forward-output-steps", lambda: forward(out=A((3, 5))), (INVALID, M_OUT)),
    ("forward-output-point-axis", lambda: forward(out=A((5, 2))), (INVALID, M_OUT)),
    ("forward-displacement-rank", lambda: forward(disp=A((2, 3))), (INVALID, M_DISP)),
    ("forward-displacement-empty", lambda: forward(disp=A((2, 0, 3))), (INVALID, M_DISP)),
    ("forward-65536", lambda: forward(nb=65536), (UNSUPPORTED, F + ": too many samples")),
    ("forward-inside-shape", lambda: forward(inside=A((6,), "uint8")), (INVALID, "inside must have shape (N)")),
    ("forward-inside-dtype", lambda: forward(inside=A((5,), "bool")), (DTYPE, "inside must be uint8")),
    # ---- which message wins -----------------------------------------------------------------------------------------
    ("forward-negative-batch+naxis-4", lambda: forward(nb=-1, naxis=4), (INVALID, M_BATCH)),
    ("forward-naxis-4+raw", lambda: forward(naxis=4, axis=(0, 1, 2, 3), flags=RAW),
     (UNSUPPORTED, F + " takes 1 to 3 deformed axes")),
    ("forward-raw+order-6", lambda: forward(flags=RAW, order=6), (INVALID, F + " takes the prefiltered control grid")),
    ("forward-order-6+half", lambda: forward(order=6, x=A((2, 8, 9), "float16")),
     (INVALID, "spline order not supported")),
    ("forward-points+output", lambda: forward(pts=A((5, 3)), out=A((2, 6))), (INVALID, M_POINTS)),
    ("forward-output+displacement", lambda: forward(out=A((2, 6)), disp=A((2, 3))), (INVALID, M_OUT)),
    ("forward-65536+inside", lambda: forward(nb=65536, inside=A((6,), "uint8")),
     (UNSUPPORTED, F + ": too many samples")),
    # ---- nothing to do ------------------------------------------------------------------------------------------------
    ("forward-empty-batch", lambda: forward(nb=0), (OK, "")),
    ("forward-no-points", lambda: forward(pts=A((0, 2)), out=A((2, 0)), inside=A((0,), "uint8")), (OK, "")),
    ("forward-no-steps", lambda: forward(x=A((0, 8, 9)), out=A((0, 5))), (OK, "")),
    ("forward-steps-last", lambda: forward(x=A((8, 9, 0)), out=A((5, 0)), axis=(0, 1)), (OK, "")),
    # ---- edhip_deform_sample_gradient -----------------------------------------------------------------------------------
    ("gradient-negative-batch", lambda: gradient(nb=-1), (INVALID, M_BATCH)),
    ("gradient-null-cotangent", lambda: gradient(cot=None), (INVALID, M_BATCH)),
    ("gradient-null-points", lambda: gradient(pts=None), (INVALID, M_BATCH)),
    ("gradient-null-displacement", lambda: gradient(disp=None), (INVALID, M_BATCH)),
    ("gradient-null-lengths", lambda: gradient(in_len=None), (INVALID, M_BATCH)),
    ("gradient-neither", lambda: gradient(din=None, dcoord=None),
     (INVALID, "neither dinput nor dcoordinate is requested")),
    ("gradient-dcoordinate-without-input", lambda: gradient(x=None), (INVALID, "dcoordinate needs the input")),
    ("gradient-naxis-4", lambda: gradient(naxis=4, axis=(0, 1, 2, 3)), (UNSUPPORTED, G + " takes 1 to 3 deformed axes")),
    ("gradient-raw", lambda: gradient(flags=RAW), (INVALID, G + " takes the prefiltered control grid")),
    ("gradient-axis", lambda: gradient(axis=(1, 1)), (INVALID, M_AXIS)),
    ("gradient-order-6", lambda: gradient(order=-1), (INVALID, "spline order not supported")),
    ("gradient-mode", lambda: gradient(mode=-1), (INVALID, "boundary mode not supported")),
    ("gradient-integer-input", lambda: gradient(x=A((2, 8, 9), "int16")), (DTYPE, M_DTYPE)),
    ("gradient-cotangent-dtype", lambda: gradient(cot=A((2, 5), "float32")),
     (DTYPE, "input and cotangent must have one dtype")),
    ("gradient-lengths", lambda: gradient(in_len=(9, 9)),
     (INVALID, "the input's deformed axes must have the extents in_len")),
    ("gradient-points", lambda: gradient(pts=A((5,))), (INVALID, M_POINTS)),
    ("gradient-points-dtype", lambda: gradient(pts=A((5, 2), "float16")), (DTYPE, M_POINTS_DTYPE)),
    ("gradient-cotangent-shape", lambda: gradient(cot=A((2, 4))), (INVALID, M_COT)),
    ("gradient-displacement", lambda: gradient(disp=A((3, 3, 3))), (INVALID, M_DISP)),
    ("gradient-65536", lambda: gradient(nb=65536), (UNSUPPORTED, G + ": too many samples")),
    ("gradient-dinput-shape", lambda: gradient(din=A((2, 8, 8))), (INVALID, "dinput must have the shape of the input")),
    ("gradient-dinput-dtype", lambda: gradient(din=A((2, 8, 9), "float32")),
     (DTYPE, "dinput and cotangent must have one dtype")),
    ("gradient-dcoordinate-shape", lambda: gradient(dcoord=A((5, 3))), (INVALID, "dcoordinate must have shape (N, naxis)")),
    ("gradient-dcoordinate-dtype", lambda: gradient(dcoord=A((5, 2), "float32")),
     (DTYPE, "dcoordinate must be float64")),
    ("gradient-dinput-only-wrong-cotangent", lambda: gradient(x=None, dcoord=None, cot=A((2, 5), "float32")),
     (DTYPE, "dinput and cotangent must have one dtype")),
    # ---- which message wins -----------------------------------------------------------------------------------------
    ("gradient-neither+raw", lambda: gradient(din=None, dcoord=None, flags=RAW),
     (INVALID, "neither dinput nor dcoordinate is requested")),
    ("gradient-raw+cotangent-shape", lambda: gradient(flags=RAW, cot=A((2, 4))),
     (INVALID, G + " takes the prefiltered control grid")),
    ("gradient-65536+dinput-shape", lambda: gradient(nb=65536, din=A((2, 8, 8))),
     (UNSUPPORTED, G + ": too many samples")),
    # ---- nothing to do ------------------------------------------------------------------------------------------------
    ("gradient-empty-batch", lambda: gradient(nb=0), (OK, "")),
    ("gradient-no-points", lambda: gradient(pts=A((0, 2)), cot=A((2, 0)), dcoord=A((0, 2))), (OK, "")),
    ("gradient-dinput-only", lambda: gradient(nb=0, x=None, dcoord=None), (OK, "")),
    ("gradient-dcoordinate-only", lambda: gradient(nb=0, din=None), (OK, "")),
]


def test_both_names_are_exported():
    assert "edhip_deform_sample" in _lib.EXPORTS and "edhip_deform_sample_gradient" in _lib.EXPORTS
    L = _lib.load()
    for name in _lib.EXPORTS:
        assert hasattr(L, name)


def test_the_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name,call,want", CASES, ids=[c[0] for c in CASES])
def test_status_and_message(name, call, want):
    assert call() == want


def test_a_null_error_buffer_is_allowed():
    L = _lib.load()
    assert L.edhip_deform_sample(1, ref(X2), 0, ref(P2), 0, ref(D2), 0, i64((8, 9)), None, ref(V2), 0, None, 0, 4,
                                 i32((0, 1, 2, 3)), 3, 0, 0.0, None, 0, None, None, 0) == UNSUPPORTED
    assert L.edhip_deform_sample_gradient(1, ref(X2), 0, ref(V2), 0, ref(P2), 0, ref(D2), 0, i64((8, 9)), None, None, 0,
                                          None, 0, 2, i32((1, 2)), 3, 0, None, 0, None, None, 0) == INVALID
