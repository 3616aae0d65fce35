"""
Public API: ``deform_random_grid``, ``deform_grid``, ``deform_grid_gradient`` -- drop-in for
``elasticdeform.deform_random_grid / deform_grid / deform_grid_gradient``
(/root/reference/elasticdeform/deform_grid.py:6-8, :52-53, :182-184): same names, positional
order, defaults, list-in => list-out, exception classes.

What differs is where the work happens: every array is (moved to) MI355X HBM and the whole
pipeline -- B-spline prefilter of the inputs and of the displacement grid, the per-voxel
deformation, and for the gradient the scatter-add plus the transposed prefilter -- runs as
hand-written HIP kernels behind the C ABI of include/edhip.h, enqueued on the current HIP stream
with no host synchronisation (one exception, documented in include/edhip.h: the first call on a
stream that needs more scratch than that stream's cached workspace holds waits for the stream once).

Limits that differ from the reference (status EDHIP_ERR_UNSUPPORTED / EDHIP_ERR_INVALID ->
RuntimeError): at most 8 array dimensions, hence at most 7 deformed axes (the control grid has one
dimension more; the reference takes whatever NumPy does, _deform_grid.c:158-175).  A deformed axis of length 1 gives what
the reference gives -- it divides by I - 1 = 0 there (deform.c:643), every coordinate is inf / NaN and maps to cval: the
output is cval everywhere, the gradient zero -- decided on the host (the C ABI itself refuses such an axis).

* numpy.ndarray in  -> numpy.ndarray out (one H2D and one D2H copy; the drop-in path)
* torch.Tensor in   -> torch.Tensor out on the same device (CUDA tensors never touch the host)

There is no CPU fallback: without a GPU or without the built library the call raises.
"""
import collections
import math
import os
import sys
import threading

import warnings

import numpy

from . import _fastlane
from . import _host
from . import _lib

_this = sys.modules[__name__]

_ARITHMETIC = {'auto': _lib.FLAG_AUTO, 'exact': _lib.FLAG_EXACT, 'fast': _lib.FLAG_FAST}
_flags = _ARITHMETIC.get(os.environ.get('EDHIP_ARITHMETIC', 'auto').lower(), _lib.FLAG_AUTO)


def set_arithmetic(kind):
    """Select the kernels' arithmetic: 'auto' (float32 / float64 volumes -> fast path, integer and
    bool volumes -> exact path), 'exact' (fp64 arithmetic in the reference's evaluation order for
    every dtype: float64 / float32 / integer outputs bit-comparable with the reference) or 'fast'
    (same as 'auto' today).  Returns the previous value."""
    global _flags
    if kind not in _ARITHMETIC:
        raise ValueError("arithmetic must be one of %s" % sorted(_ARITHMETIC))
    prev = [k for k, v in _ARITHMETIC.items() if v == _flags][0]
    _flags = _ARITHMETIC[kind]
    return prev


_reduced = os.environ.get('EDHIP_REDUCED_PRECISION', '') not in ('', '0')


def set_reduced_precision(enabled):
    """Opt in to reduced-precision I/O (off by default, where
    float16 input raises 'data type not supported' exactly like the reference, deform.c:742-747):

    * float16 / bfloat16 volumes (torch tensors; numpy float16): stored in 16 bits, computed in
      float32 -- prefilter, interpolation and the gradient's scatter all run on the widened values
      and only the final result is rounded (to nearest even) to the storage type.  Result =
      round_storage(float32 pipeline(widen(X))).
    * integer images with order > 1: the reference prefilters them INTO their integer dtype
      (deform_grid.py:158), which destroys the interpolation (off by up to 225 grey
      levels on uint8).  With the opt-in the prefilter and the interpolation run in float32 and the
      result is stored with the reference's own rounding / clamping rule (deform.c:292-306).  This
      deliberately DIFFERS from the reference for such images; order 0 / 1 are unaffected.

    With arithmetic 'exact' 16-bit volumes go through the fp64 kernels in their storage type
    (rounded after every filter axis, like every dtype there).  Returns the previous setting."""
    global _reduced
    prev = _reduced
    _reduced = bool(enabled)
    return prev


_strict_crop = os.environ.get('EDHIP_STRICT_CROP', '') not in ('', '0')


def set_crop_identity(strict):
    """The reference's crop guarantee, bit for bit (README.md:113 ``full[crop] == cropped``): with ``strict=True`` the
    spline prefilter of a cropped call always runs over the WHOLE input, exactly as in the uncropped call, so the
    cropped result equals the same region of the full result in every bit.  Off by default: large inputs with a small
    crop then prefilter only the part of the volume the crop can reach (plus a decay margin), which changes float32 /
    float64 results by ~1e-9 of the data's scale -- far inside every tolerance, but not identical bits -- and saves
    most of the prefilter (BASELINE cfg4: forward 263 -> 140 us).  Integer volumes and 'exact' arithmetic never use
    the window.  Returns the previous setting."""
    global _strict_crop
    prev = _strict_crop
    _strict_crop = bool(strict)
    return prev


_FIELD_STRENGTH = ('auto', 'strong')
_field_strength = os.environ.get('EDHIP_FIELD_STRENGTH', 'auto').lower()
if _field_strength not in _FIELD_STRENGTH:
    _field_strength = 'auto'


def set_field_strength(kind):
    """A performance hint for the forward kernels of float32 volumes with three deformed axes (results agree to float32
    rounding either way).  'strong' says the displacement fields are strong -- a displacement gradient of ~0.15 per voxel
    and more, e.g. sigma >= 10 on a 5^3 grid over 256^3, or the reference README's ``sigma=25, points=3`` on a 200 x 300
    image: the z-walk kernels (tiles split in halves, wide row pitches) then serve every geometry they support and are
    5-35 % faster on such fields; on mild fields they are 5-50 % slower than the default choice for small volumes and
    batches (profiles/r06_k1_route_sweep.txt).  'auto' (default) picks by the volume's shape alone.  The library never
    picks by looking at earlier calls: a call's bits depend on its arguments and on this setting only.  Returns the
    previous value."""
    global _field_strength
    if kind not in _FIELD_STRENGTH:
        raise ValueError("field strength must be one of %s" % list(_FIELD_STRENGTH))
    prev = _field_strength
    _field_strength = kind
    return prev


_tls = threading.local()
# deform_random_grid knows what the library cannot see without a host round trip: sigma and the control-point spacing.
# sigma * (points - 1) / (extent - 1) is the displacement gradient's scale; the z-walk kernels win from ~0.15
# (5 points: sigma 10 at 256^3 = 0.157: 128^3 +23 %, 192^3 +5 %, 256^3 +19 %, batches even; sigma 15: +20 ... +27 %; sigma 5:
# -7 ... -23 % -- profiles/r06_k1_route_sweep.txt, last table)
RANDOM_GRID_STRONG_FROM = 0.15


class _random_grid_hint(object):
    """Context of one deform_random_grid call: the forward call inside it carries EDHIP_FLAG_STRONG_FIELD when the
    drawn field is strong by construction.  A function of the call's own arguments (sigma, points, shape)."""

    def __init__(self, sigma, points, deform_shape):
        try:
            self.strong = any(abs(float(sigma)) * (int(p) - 1) >= RANDOM_GRID_STRONG_FROM * (int(n) - 1)
                              for p, n in zip(points, deform_shape) if int(n) > 1)
        except (TypeError, ValueError):
            self.strong = False

    def __enter__(self):
        self.prev = getattr(_tls, 'strong', False)
        _tls.strong = self.strong
        return self

    def __exit__(self, *exc):
        _tls.strong = self.prev
        return False


def _route_flags():
    return _lib.FLAG_STRONG_FIELD if (_field_strength == 'strong' or getattr(_tls, 'strong', False)) else 0


_GRAD_ACCUMULATION = ('fixed', 'float')
_grad_accumulation = os.environ.get('EDHIP_GRAD_ACCUMULATION', 'fixed').lower()
if _grad_accumulation not in _GRAD_ACCUMULATION:
    _grad_accumulation = 'fixed'


def set_gradient_accumulation(kind):
    """How ``deform_grid_gradient`` sums the taps of float32 / float64 gradients (deform.c:926-997 adds every tap
    into the output array in its own precision):

    * 'fixed' (default): the tile kernels accumulate in fixed-point LDS cells whose scale comes from the sum of |dY|
      over the tile (include/edhip.h).  Every contribution is resolved to ~1.4e-10 of its TILE's sum of |dY|: exact
      to float32 rounding for gradients of ordinary dynamic range, but one 1e6 outlier costs the other voxels of its
      8 x 8 x 16 tile ~1e-4 absolute.
    * 'float': every tap is added with a floating-point atomic in the array's own type, as the reference does -- the
      precision of a contribution is relative to the contribution itself, whatever its neighbours hold.  The scatter
      runs on the one-thread-per-voxel kernel with the reference's fp64 coordinate arithmetic (several times slower
      than the tile kernels); prefilter transposes are unchanged.

    Returns the previous setting."""
    global _grad_accumulation
    if kind not in _GRAD_ACCUMULATION:
        raise ValueError("gradient accumulation must be one of %s" % list(_GRAD_ACCUMULATION))
    prev = _grad_accumulation
    _grad_accumulation = kind
    return prev


def _torch():
    import torch
    return torch


_TORCH_NAMES = None


def _dtype_name(t):
    """torch dtype -> the NumPy-style name used by the C ABI table."""
    global _TORCH_NAMES
    if _TORCH_NAMES is None:
        torch = _torch()
        _TORCH_NAMES = {getattr(torch, n): n for n in _lib.DTYPE_CODES if hasattr(torch, n)}
    name = _TORCH_NAMES.get(t.dtype)
    if name is None or (name in _lib.REDUCED_DTYPES and not _reduced):
        raise RuntimeError('data type not supported')     # deform.c:744,891 (float16, complex ...)
    return name


def _device_for(arrays):
    """The GPU every array of this call lives on / is moved to.  Fails loudly without one."""
    torch = _torch()
    for a in arrays:
        if not isinstance(a, numpy.ndarray) and a.is_cuda:
            return a.device
    if not torch.cuda.is_available():
        raise RuntimeError('elasticdeform_amd needs a ROCm GPU (MI355X / gfx950): none is visible '
                           'and there is no CPU fallback.')
    return torch.device('cuda', torch.cuda.current_device())


def _to_device(x, device):
    """numpy / torch array -> tensor in HBM on `device`, keeping the logical strides when the
    bridge allows it (the reference accepts arbitrary strides, _deform_grid.c:12-15)."""
    torch = _torch()
    if isinstance(x, numpy.ndarray):
        if x.dtype.name not in _lib.DTYPE_CODES or (x.dtype.name in _lib.REDUCED_DTYPES and not _reduced):
            raise RuntimeError('data type not supported')
        if not x.dtype.isnative or not x.flags.aligned or any(s < 0 for s in x.strides) \
                or not x.flags.writeable:
            x = numpy.ascontiguousarray(x).astype(x.dtype.newbyteorder('='), copy=True)
        return torch.from_numpy(x).to(device)
    x = x.detach()
    if x.device != device:
        x = x.to(device)
    return x


def _from_device(t, like):
    """Give the result back in the caller's array family."""
    if isinstance(like, numpy.ndarray):
        return t.cpu().numpy()
    if like.device != t.device:
        return t.to(like.device)
    return t


def _constant_result(like, shape, cval):
    """An array of `shape` in the family, dtype and device of `like`, filled with the value the reference stores for
    a constant voxel (_host.stored_constant)."""
    shape = tuple(int(v) for v in shape)
    if isinstance(like, numpy.ndarray):
        name = like.dtype.name
        if name not in _lib.DTYPE_CODES or (name in _lib.REDUCED_DTYPES and not _reduced):
            raise RuntimeError('data type not supported')     # deform.c:744,891
        return numpy.full(shape, _host.stored_constant(cval, name), dtype=like.dtype)
    torch = _torch()
    return torch.full(shape, _host.stored_constant(cval, _dtype_name(like)), dtype=like.dtype, device=like.device)


_INT_RANGE = {'uint8': (0.0, 255.0), 'uint16': (0.0, 65535.0), 'uint32': (0.0, 4294967295.0),
              'int8': (-128.0, 127.0), 'int16': (-32768.0, 32767.0), 'int32': (-2147483648.0, 2147483647.0)}


def _widen(t, order, prefilter):
    """Reduced-precision opt-in: the float32 stand-in of a 16-bit float volume, or of an integer
    image that would lose its prefilter to integer rounding; None when `t` runs as it is."""
    if not _reduced or (_flags & _lib.FLAG_EXACT):
        return None
    name = _TORCH_NAMES.get(t.dtype) if _TORCH_NAMES else None
    if name is None:
        name = _dtype_name(t)
    if name in _lib.REDUCED_DTYPES or (name in _INT_RANGE and order > 1 and prefilter):
        return t.to(_torch().float32)
    return None


def _direct16(x, axes, order, prefilter, crop):
    """Reduced-precision opt-in, 16-bit float volume: can it stay in 16 bits in HBM?  (The float32 kernels then
    widen it where they read it and narrow where they write: the first prefilter pass, K1's store, K2's load of
    dY, the last transposed prefilter pass -- no cast passes, 16 instead of 44 bytes of casts + I/O per voxel
    around the float32 intermediates.)  This is only the host's guess from shapes; the library has the last word
    (EDHIP_ERR_UNSUPPORTED, nothing launched) and the caller then falls back to widening with a cast."""
    if not _reduced or (_flags & _lib.FLAG_EXACT) or crop is not None or not prefilter or order not in (2, 3):
        return False
    torch = _torch()
    if x.dtype not in (torch.float16, torch.bfloat16) or not x.is_contiguous() or len(axes) != 3 or x.dim() < 3:
        return False
    if tuple(axes) != tuple(range(x.dim() - 3, x.dim())) or int(x.shape[-1]) % 4:
        return False
    return all(64 <= int(x.shape[a]) <= 256 for a in axes)


def _narrow(t32, like):
    """float32 result -> the storage dtype of `like`: round to nearest even for 16-bit floats; the
    reference's store rule for integers (deform.c:292-306: round half away from zero, clamp)."""
    torch = _torch()
    name = _dtype_name(like)
    if name in _lib.REDUCED_DTYPES:
        return t32.to(like.dtype)
    lo, hi = _INT_RANGE[name]
    # in float64 like the reference (`t` is a double there): 0.49999997f + 0.5f rounds up to 1.0f in
    # float32 and would store 1 where the double rule stores 0
    t = t32.double()
    nan = torch.isnan(t)
    r = torch.where(t > 0, t + 0.5, t - 0.5) if lo < 0 else torch.where(t > 0, t + 0.5, torch.zeros_like(t))
    r = r.clamp_(lo, hi).trunc_()
    # NaN passes every comparison of the store rule and reaches the cast: x86-64's cvttsd2si gives the
    # "integer indefinite" 0x80...0, of which the narrow and the unsigned types keep the low bits (0)
    # -- what the exact kernels' store_forward produces
    r = torch.where(nan, torch.full_like(r, float(lo) if name in ('int32', 'int64') else 0.0), r)
    return r.to(like.dtype)


def _desc(t):
    es = t.element_size()
    return _lib.describe(t.data_ptr(), _dtype_name(t), t.shape, [s * es for s in t.stride()])


def _prepared(plan, n):
    """ctypes form of the plan's parameter arrays, built once per (cached) plan"""
    if plan.prepared is None:
        plan.prepared = _lib.DeformArgs(n, plan.axis, plan.order, plan.mode, plan.cval, plan.output_offset,
                                        plan.inverse_affine)
    return plan.prepared


def _desc_sample0(t):
    """Descriptor of sample 0 of a stacked tensor (B, ...) and the byte distance between samples."""
    es = t.element_size()
    return (_lib.describe(t.data_ptr(), _dtype_name(t), t.shape[1:], [s * es for s in t.stride()[1:]]),
            t.stride(0) * es)


def _stream(device):
    return _torch().cuda.current_stream(device).cuda_stream


# Forward -> gradient hand-over of the tile bounding boxes (EDHIP_FLAG_KEEP_BOXES / USE_BOXES): per
# (device, stream), the storage address and version counter of the displacement tensor of the last
# forward call.  The gradient call sets USE_BOXES when it is handed the same storage, unmodified
# (autograd's backward, or deform_grid_gradient after deform_grid in a training step).  This is a
# heuristic about CONTENTS only: the library checks every other argument itself and treats the boxes
# as a hint, so a tensor changed behind PyTorch's back (`.data`), or a new tensor that landed on a
# freed one's address, costs time and never correctness.
_box_owner = {}
_batch_grids = {}      # (device, stream) -> (identity of the displacement tensor, its filtered grids) of the last batch forward


def _box_id(displacement, df):
    torch = _torch()
    if torch.is_tensor(displacement) and displacement.is_cuda and df.data_ptr() == displacement.data_ptr():
        return (displacement.data_ptr(), displacement._version)
    return None


def _box_flag_forward(displacement, df, device, stream):
    """KEEP_BOXES for a forward call whose control grid is the caller's own device tensor."""
    ident = _box_id(displacement, df)
    _box_owner[(device.index, stream)] = ident
    _batch_grids[(device.index, stream)] = None        # (the stream's box buffer changes hands)
    return _lib.FLAG_KEEP_BOXES if ident is not None else 0


def _box_flag_gradient(displacement, df, device, stream):
    ident = _box_id(displacement, df)
    if ident is not None and _box_owner.get((device.index, stream)) == ident:
        return _lib.FLAG_USE_BOXES
    return 0


def _filter_axes(x, axes, order, transpose, device, overwrite=False, stream=None):
    """Chain of 1-D spline filters over `axes` -- the reference's loop at deform_grid.py:157-162
    (forward) / :279-284 (transpose).  The reference filters x -> x_f and then x_f in place; so does
    this chain for lines of up to 256 samples, and it ping-pongs between two buffers for longer ones
    (the caller's x is never written); the values are the same."""
    torch = _torch()
    axes = list(axes)
    if not axes:
        return x
    if stream is None:
        stream = _stream(device)
    # Lines that fit the whole-line tile kernels are filtered in place from the second pass on
    # (like the reference; one temporary instead of two keeps the step's working set smaller);
    # longer lines ping-pong, because in place the block-recompute kernels cannot split a line.
    inplace = all(int(x.shape[d]) <= 256 for d in axes)
    if overwrite and inplace:
        bufs = [x, None]            # x is the caller's own temporary (dX): every pass in place
    else:
        bufs = [torch.empty_like(x), torch.empty_like(x) if (len(axes) > 1 and not inplace) else None]
    if inplace:
        # one library call for the whole chain: x -> bufs[0], then in place
        _lib.spline_filter_axes(_desc(x), _desc(bufs[0]), axes, order, transpose, _flags, stream)
        return bufs[0]
    src = x
    for i, d in enumerate(axes):
        dst = bufs[i & 1]
        _lib.spline_filter1d(_desc(src), _desc(dst), d, order, transpose, _flags, stream)
        src = dst
    return src


# Crop-aware prefilter: with a crop only a box of each input is ever read, so only that
# box plus the filter's decay margin is filtered.  The window never leaves the device: edhip_source_window
# computes it from the control grid (one small launch, no read-back), the filter passes and the transposed
# passes of the gradient restrict themselves to it (edhip_spline_filter_axes_window), K1 / K2 work on full-size
# buffers whose samples outside the window are never touched.  The host only decides WHETHER to try, from what
# it knows without the device: the output box plus the margins, as a fraction of the input.
# (Until round 4 the box was read back to the host: the synchronisation exposed the launch latency of every
# kernel behind it, and BASELINE cfg4 -- 3 x 256^3 cropped to 64^3 -- never got a window.)
CROP_WINDOW_MIN_SAVING = 24e6        # voxels per filter pass, summed over the inputs: below, the window's own launches and
                                     # host calls (~30 us) eat what it saves (a 256^3 float32 pass is 25 us; profiles/r04_time_crop_window.txt)
CROP_WINDOW_MAX_FRACTION = 0.50      # (output box + margins) / input, upper bound known to the host
# decay margin (samples) after which a cut in a line is invisible in the data's own precision: |pole|^m below
# 1e-9 for float32 volumes (their filter runs in float32), below 1e-18 for float64
_WINDOW_MARGIN = {'float32': {2: 12, 3: 16}, 'float64': {2: 24, 3: 32}}
_WINDOW_MIN_LINE = 64                # the whole-line tile kernels' shortest line


def _crop_window_pays(plan, shapes, names, todo, in_len, out_len, disp_shape=None, contiguous=None):
    """What the host knows without the device: does the smallest possible window (output box + margins + taps, at
    least a tile kernel's shortest line) save enough filter work, summed over the inputs `todo`?  One rule for the
    general path (_crop_windows) and for the repeat-call lanes (_fastlane.Lane.window_pays), so that repeated
    identical calls take the same route and return the same bits."""
    def volume(i, lens):            # voxels of input i when its deformed axes have extents `lens`
        v = float(numpy.prod([int(d) for d in shapes[i]], dtype=numpy.float64))
        for a, l in zip(plan.axis[i], lens):
            v *= float(l) / float(shapes[i][a])
        return v

    def at_least(i):                # no window is smaller than the output box plus margins and taps
        m = _WINDOW_MARGIN[names[i]][int(plan.order[i])]
        return [min(n_in, max(n_out + 2 * m + int(plan.order[i]) + 3, _WINDOW_MIN_LINE))
                for n_in, n_out in zip(in_len, out_len)]
    if not todo or _strict_crop:
        return False
    if disp_shape is not None and (len(disp_shape) < 2 or len(disp_shape) > 5 or
                                   numpy.prod([int(d) for d in disp_shape]) > 7680):
        return False                # (control grid in LDS, up to 4 deformed axes: edhip_source_window)
    # inputs the window kernels take: contiguous, every deformed axis at least a tile kernel's shortest line
    todo = [i for i in todo if (contiguous is None or contiguous[i]) and
            all(int(shapes[i][a]) >= _WINDOW_MIN_LINE for a in plan.axis[i])]
    if not todo:
        return False
    full = sum(volume(i, in_len) for i in todo)
    least = sum(volume(i, at_least(i)) for i in todo)
    return not (full - least < CROP_WINDOW_MIN_SAVING or least > CROP_WINDOW_MAX_FRACTION * full)


def _crop_windows(plan, xs, disp_desc, dflag, crop, prefilter, device, stream, grid_stays=False):
    """Per input: a device tensor holding its filter window (2 ints per dimension, edhip_source_window), or
    None for 'filter the whole array'.  Floating-point volumes of orders 2 / 3 outside 'exact' arithmetic: the
    window's coefficients equal the whole-volume ones to below the data's rounding, not bit for bit."""
    n = len(xs)
    wins = [None] * n
    if crop is None or not prefilter or (_flags & _lib.FLAG_EXACT) or _strict_crop:
        return wins
    todo = [i for i in range(n) if int(plan.order[i]) in _WINDOW_MARGIN.get(_dtype_name(xs[i]), {})]
    if not todo:
        return wins
    ax0 = plan.axis[0]
    in_len = [int(xs[0].shape[a]) for a in ax0]
    out_len = [int(plan.output_shapes[0][a]) for a in ax0]
    # (one rule -- grid size, layout, shortest line, pay-off -- for this path and for the repeat-call lanes)
    if not _crop_window_pays(plan, [tuple(int(d) for d in x.shape) for x in xs], [_dtype_name(x) for x in xs], todo,
                             in_len, out_len, disp_shape=list(disp_desc.shape)[:disp_desc.ndim],
                             contiguous=[bool(x.is_contiguous()) for x in xs]):
        return wins
    torch = _torch()
    for i in todo:
        x = xs[i]
        if not x.is_contiguous() or any(int(x.shape[a]) < _WINDOW_MIN_LINE for a in plan.axis[i]):
            continue
        name = _dtype_name(x)
        vn = 4 if name == 'float32' else 2
        win = torch.empty(2 * x.dim(), dtype=torch.int32, device=device)
        st = _lib.source_window(disp_desc, in_len, out_len, plan.output_offset, plan.inverse_affine,
                                tuple(int(v) for v in x.shape), plan.axis[i], int(plan.order[i]), int(plan.mode[i]),
                                _WINDOW_MARGIN[name][int(plan.order[i])], vn if int(x.shape[-1]) % vn == 0 else 1,
                                _WINDOW_MIN_LINE,
                                _flags | dflag | _lib.FLAG_FAST | (_lib.FLAG_GRID_STAYS if (grid_stays and dflag) else 0),
                                stream, win.data_ptr())
        if st == 0:
            wins[i] = win
            grid_stays = True       # (the next input's window: same grid, just filtered by THIS call)
    return wins


def _prefilter_displacement(displacement, device):
    """Order-3 prefilter of the control grid along every grid axis (deform_grid.py:166-169,
    :269-272); the output keeps the displacement's dtype like numpy.zeros_like there.

    Returns (grid, extra_flags): small grids (the normal case) are handed over raw and filtered
    inside edhip_deform in a single launch (EDHIP_FLAG_RAW_DISPLACEMENT, same arithmetic and the
    same per-axis rounding); larger ones go through edhip_spline_filter1d axis by axis."""
    if displacement.ndim < 2:
        return displacement, 0
    if displacement.numel() <= _lib.RAW_DISPLACEMENT_MAX_POINTS:
        return displacement, _lib.FLAG_RAW_DISPLACEMENT
    return _filter_axes(displacement, range(1, displacement.ndim), 3, False, device), 0


def _lane_lookup(gradient, X, displacement, order, mode, cval, crop, prefilter, axis, X_shape,
                 affine, rotate, zoom):
    """(signature, lane) of a repeat call on device tensors (_fastlane.py); (None, None) for every
    call the lane does not serve; (sig, None) for a signature seen for the first time."""
    if _reduced or affine is not None or rotate is not None or zoom is not None or not _fastlane.enabled:
        return None, None
    if _strict_crop or (gradient and _grad_accumulation != 'fixed'):
        return None, None           # (the lanes are built for the default routes)
    sig = _fastlane.signature(gradient, X, displacement, order, mode, cval, crop, prefilter, axis,
                              X_shape, _flags | _route_flags())
    if sig is None:
        return None, None
    lane = _fastlane.lookup(sig)
    if lane is None:
        return sig, None
    if lane is False or lane.window_pays:
        return None, None
    return sig, lane


def _lane_build(sig, gradient, xs, dd, plan, prefilter, X_shape, crop):
    """After the general path has served `sig` once: prepare the repeat-call lane for it."""
    if dd.ndim < 2 or dd.numel() > _lib.RAW_DISPLACEMENT_MAX_POINTS:
        _fastlane.remember(sig, False)
        return
    try:
        lane = _fastlane.Lane(_this, gradient, xs, dd, plan, prefilter, X_shape, _flags | _route_flags(), crop)
    except Exception as exc:     # noqa: BLE001 -- whatever went wrong, the computed result must not be lost
        # the result of this call is already computed: a lane that cannot be built is no lane -- but say so once
        warnings.warn("elasticdeform_amd: no repeat-call lane for this signature (%s: %s)" % (type(exc).__name__, exc),
                      RuntimeWarning, stacklevel=3)
        lane = False
    _fastlane.remember(sig, lane)


# Layouts whose deformed axes are not the innermost ones (channel-last volumes: X is (D, H, W, C) with
# axis=(0, 1, 2)) miss every kernel that wants unit stride along the last deformed axis -- the LDS-DMA
# staging of the tile kernels, the integer fast path -- and run on the general kernels with one strided
# load per sample (96^3 x 4 float32, order 3: 0.39 ms against 0.15 ms channel-first).  Such inputs are
# brought to "step axes first" on the device (one transpose each way, ~4 passes over the array at HBM
# speed) and go through the same public function with the trailing axes as the deformed ones.  Values
# are those of the channel-first call on the same data.
RELAYOUT_MIN_ELEMENTS = 1 << 16


def _relayout_perms(plan, Xs):
    """Per input: the permutation that moves its non-deformed axes to the front, or None when the
    deformed axes already are the trailing ones (or the array is small).  None when no input needs one."""
    perms = []
    for x, ax, o in zip(Xs, plan.axis, plan.order):
        nd = len(x.shape)
        # (order 0 is one strided load per voxel either way: the two transposes would cost more than they save)
        if tuple(ax) == tuple(range(nd - len(ax), nd)) or int(o) < 1 or \
                int(numpy.prod(x.shape)) < RELAYOUT_MIN_ELEMENTS:
            perms.append(None)
        else:
            perms.append([a for a in range(nd) if a not in ax] + list(ax))
    return perms if any(p is not None for p in perms) else None


def _inverse_perm(p):
    inv = [0] * len(p)
    for i, a in enumerate(p):
        inv[a] = i
    return inv


def _relayout_detour(arrays, perms, plan, device, call):
    """The detour of deform_grid / deform_grid_gradient for `perms` (_relayout_perms): the arrays go to the device
    and are brought to "step axes first"; `call(arrays, axis)` is the public function itself on them, with the
    trailing axes as the deformed ones; its results come back in the caller's layout and array family."""
    with _torch().cuda.device(device):
        moved = [_to_device(x, device) for x in arrays]
        moved = [x.permute(p).contiguous() if p is not None else x for x, p in zip(moved, perms)]
        axis_p = [tuple(range(x.dim() - plan.naxis, x.dim())) if p is not None else tuple(ax)
                  for x, p, ax in zip(moved, perms, plan.axis)]
        outs = call(moved, axis_p)
        outs = [o.permute(_inverse_perm(p)).contiguous() if p is not None else o for o, p in zip(outs, perms)]
        return [_from_device(o, x) for o, x in zip(outs, arrays)]


def _deform_may_decline(gradient, ins, df, outs, plan, flags, stream, fast16, widen):
    """edhip_deform with `ins` / `outs` in the C ABI's roles (the gradient call: dX / dY).  `fast16`: 16-bit volumes
    stay in 16 bits (EDHIP_FLAG_FAST), which the library may decline with nothing launched; `widen()` then replaces
    the contents of the two lists by what the float32 route takes, and the call is repeated without the flag."""
    def call(extra, may_decline):
        return _lib.deform(gradient, [_desc(t) for t in ins], _desc(df), plan.output_offset,
                           [_desc(t) for t in outs], plan.axis, plan.order, plan.mode, plan.cval,
                           plan.inverse_affine, flags | extra, stream, prepared=_prepared(plan, len(ins)),
                           may_decline=may_decline)
    if call(_lib.FLAG_FAST if fast16 else 0, fast16) != 0:
        widen()
        call(0, False)


def deform_random_grid(X, sigma=25, points=3, order=3, mode='constant', cval=0.0,
                       crop=None, prefilter=True, axis=None,
                       affine=None, rotate=None, zoom=None):
    """
    Elastic deformation with a random square deformation grid (deform_grid.py:6-49): draws
    ``numpy.random.randn(ndim, *points) * sigma`` from NumPy's global RNG, exactly like the
    reference, and calls :func:`deform_grid`.
    """
    Xs = _host.normalize_inputs(X)
    axis, deform_shape = _host.normalize_axis_list(axis, Xs)
    if not isinstance(points, (list, tuple)):
        points = [points] * len(deform_shape)
    displacement = numpy.random.randn(len(deform_shape), *points) * sigma
    with _random_grid_hint(sigma, points, deform_shape):
        return deform_grid(X, displacement, order, mode, cval, crop, prefilter, axis,
                           affine, rotate, zoom)


def deform_grid(X, displacement, order=3, mode='constant', cval=0.0, crop=None, prefilter=True,
                axis=None, affine=None, rotate=None, zoom=None):
    """
    Elastic deformation with a deformation grid (deform_grid.py:52-179).

    X : array or list of arrays (numpy.ndarray or torch.Tensor); displacement : array of shape
    (naxis, n_0, ..., n_{naxis-1}); order 0..5, mode in {nearest, wrap, reflect, mirror,
    constant}, cval, crop (slices over the deformed axes), prefilter, axis, affine
    (naxis x naxis+1), rotate / zoom (2-D only) -- all with the reference's meaning, and order /
    mode / cval / axis may be per-input lists.  Returns the deformed array, or a list for a list.
    """
    sig, lane = _lane_lookup(False, X, displacement, order, mode, cval, crop, prefilter, axis, None,
                             affine, rotate, zoom)
    if lane is not None:
        return lane.run(_this, X, X if type(X) is list else (X,), displacement)
    Xs = _host.normalize_inputs(X)
    plan = _host.cached_plan(Xs, displacement, order, mode, cval, crop, axis, affine, rotate, zoom)

    torch = _torch()
    if _host.degenerate_axis([x.shape for x in Xs], plan.axis):
        # a deformed axis of length 1: every voxel maps to the constant, as in the reference (_host.degenerate_axis)
        res = [_constant_result(x, plan.output_shapes[i], plan.cval[i]) for i, x in enumerate(Xs)]
        return res if isinstance(X, list) else res[0]
    device = _device_for(list(Xs) + [displacement])
    perms = _relayout_perms(plan, Xs)
    if perms is not None:
        # (every argument has passed the reference's checks above, with the caller's own axes)
        res = _relayout_detour(Xs, perms, plan, device, lambda Xp, axis_p: deform_grid(
            Xp, _to_device(displacement, device), order, mode, cval, crop, prefilter, axis_p, affine, rotate, zoom))
        return res if isinstance(X, list) else res[0]
    with torch.cuda.device(device):
        stream = _stream(device)
        Xs_dev = [_to_device(x, device) for x in Xs]
        # reduced-precision opt-in: 16-bit float volumes (and integer images with order > 1) are
        # computed in float32 and narrowed at the end
        direct = [_direct16(x, plan.axis[i], int(plan.order[i]), prefilter, crop) for i, x in enumerate(Xs_dev)]
        wide = [None if direct[i] else _widen(x, int(plan.order[i]), prefilter) for i, x in enumerate(Xs_dev)]
        Xd = [w if w is not None else x for w, x in zip(wide, Xs_dev)]
        dd = _to_device(displacement, device)

        # the displacement is always prefiltered (deform_grid.py:166-169); the inputs along their
        # deformed axes (deform_grid.py:155-164): the whole array, or -- with a crop -- only the
        # window of it that the cropped output can reach
        df, dflag = _prefilter_displacement(dd, device)
        wins = _crop_windows(plan, Xd, _desc(df), dflag, crop, prefilter, device, stream)
        Xf = []
        for i, x in enumerate(Xd):
            xf = None
            if direct[i]:
                # 16-bit storage: the first filter pass widens, the chain continues in place in float32
                xf = torch.empty(x.shape, dtype=torch.float32, device=device)
                if _lib.spline_filter_axes(_desc(x), _desc(xf), list(plan.axis[i]), int(plan.order[i]), False,
                                           _flags | _lib.FLAG_FAST, stream, may_decline=True) != 0:
                    direct[i] = False
                    wide[i] = x = Xd[i] = x.to(torch.float32)
                    xf = None
            if xf is not None:
                pass
            elif not (prefilter and plan.order[i] > 1):
                xf = x
            elif wins[i] is not None:
                # a full-size buffer of which only the window is written -- and read: the kernels' taps stay
                # inside the source box, the box inside the window
                xf = torch.empty_like(x)
                if _lib.spline_filter_axes_window(_desc(x), _desc(xf), list(plan.axis[i]), int(plan.order[i]), False,
                                                  wins[i].data_ptr(), _flags, stream) != 0:
                    xf = None           # (outside the tile kernels' envelope: nothing was launched)
            if xf is None:
                xf = _filter_axes(x, plan.axis[i], int(plan.order[i]), False, device, stream=stream)
            Xf.append(xf)

        # every output element is written by the kernel (value or cval), so no zero fill is needed
        # (a 16-bit volume that stayed in 16 bits: K1 reads the float32 coefficients and narrows at its store)
        outs = [torch.empty(tuple(int(s) for s in shape), dtype=x.dtype, device=device)
                for shape, x in zip(plan.output_shapes, Xd)]

        bflag = _box_flag_forward(displacement, df, device, stream)
        if dflag and any(w is not None for w in wins):
            bflag |= _lib.FLAG_GRID_STAYS        # (edhip_source_window has just filtered this very grid on this stream)

        def widen():
            # the library declined the 16-bit stores: float32 outputs, narrowed by a cast like the other route
            outs[:] = [torch.empty(o.shape, dtype=torch.float32, device=device) if d else o
                       for o, d in zip(outs, direct)]
            wide[:] = [xf if d else w for xf, d, w in zip(Xf, direct, wide)]
        _deform_may_decline(False, Xf, df, outs, plan, _flags | dflag | bflag | _route_flags(), stream, any(direct),
                            widen)
        outs = [_narrow(o, xs) if w is not None else o for o, xs, w in zip(outs, Xs_dev, wide)]
        res = [_from_device(o, x) for o, x in zip(outs, Xs)]
        if sig is not None:
            _lane_build(sig, False, Xs_dev, dd, plan, prefilter, None, crop)
    return res if isinstance(X, list) else res[0]


def deform_grid_gradient(dY, displacement, order=3, mode='constant', cval=0.0, crop=None,
                         prefilter=True, axis=None, X_shape=None,
                         affine=None, rotate=None, zoom=None):
    """
    Gradient of :func:`deform_grid` with respect to its input (deform_grid.py:182-291): the exact
    adjoint, interpolation and prefilter included.  ``X_shape`` (tuple, or list of tuples) is
    required when ``crop`` is used.
    """
    sig, lane = _lane_lookup(True, dY, displacement, order, mode, cval, crop, prefilter, axis, X_shape,
                             affine, rotate, zoom)
    if lane is not None:
        return lane.run(_this, dY, dY if type(dY) is list else (dY,), displacement)
    dYs = _host.normalize_inputs(dY)

    if isinstance(X_shape, tuple):
        X_shape = [X_shape]
    elif X_shape is None:
        if crop is not None:
            raise ValueError("X_shape is required if the crop parameter is given.")
        X_shape = [tuple(dy.shape) for dy in dYs]

    # every argument check runs before anything touches the device, in the reference's order
    # (deform_grid.py:246-266): a bad displacement / order / crop raises what the reference raises
    plan = _host.cached_plan([_host.ShapeOnly(s) for s in X_shape], displacement, order, mode, cval, crop,
                             axis, affine, rotate, zoom)
    if [tuple(s) for s in plan.output_shapes] != [tuple(dy.shape) for dy in dYs]:
        raise ValueError("X_shape does not match output shape and cropping. "
                         "Expected output shape is %s, but %s given."
                         % (str(plan.output_shapes), str([tuple(dy.shape) for dy in dYs])))

    torch = _torch()
    if _host.degenerate_axis(X_shape, plan.axis):
        # (a deformed axis of length 1: no voxel contributes, the gradient is zero -- deform.c:928)
        res = [_constant_result(dy, tuple(int(v) for v in sh), 0.0) for dy, sh in zip(dYs, X_shape)]
        return res if isinstance(dY, list) else res[0]
    device = _device_for(list(dYs) + [displacement])
    perms = _relayout_perms(plan, [_host.ShapeOnly(sh) for sh in X_shape])
    if perms is not None:
        shape_p = [tuple(int(sh[a]) for a in p) if p is not None else tuple(sh) for sh, p in zip(X_shape, perms)]
        res = _relayout_detour(dYs, perms, plan, device, lambda dYp, axis_p: deform_grid_gradient(
            dYp, _to_device(displacement, device), order, mode, cval, crop, prefilter, axis_p, shape_p, affine, rotate,
            zoom))
        return res if isinstance(dY, list) else res[0]
    with torch.cuda.device(device):
        dY_dev = [_to_device(dy, device) for dy in dYs]
        # 16-bit dY that can stay in 16 bits (_direct16): K2 widens it where it reads it, the accumulators are float32
        direct = [_direct16(dy, plan.axis[i], int(plan.order[i]), prefilter, crop) and tuple(X_shape[i]) == tuple(dy.shape)
                  for i, dy in enumerate(dY_dev)]
        wide = [None if direct[i] else _widen(dy, int(plan.order[i]), prefilter) for i, dy in enumerate(dY_dev)]
        dYd = [w if w is not None else dy for w, dy in zip(wide, dY_dev)]
        # gradient accumulators start at zero (deform_grid.py:243): cleared by the library next to its
        # tables kernel (EDHIP_FLAG_ZERO_GRADIENT) instead of by a fill launch of their own
        dXs = [torch.empty(tuple(int(v) for v in s), dtype=torch.float32 if d else dy.dtype, device=device)
               for s, dy, d in zip(X_shape, dYd, direct)]

        dd = _to_device(displacement, device)
        df, dflag = _prefilter_displacement(dd, device)

        stream = _stream(device)
        gflags = _flags | dflag | _lib.FLAG_ZERO_GRADIENT | _box_flag_gradient(displacement, df, device, stream)
        if _grad_accumulation == 'float':
            # floating-point atomics in the array's own type (set_gradient_accumulation): the exact kernel's scatter
            gflags = (gflags & ~(_lib.FLAG_FAST | _lib.FLAG_AUTO)) | _lib.FLAG_EXACT

        def widen():
            # the library declined the 16-bit loads: widen dY with a cast, like the other route
            wide[:] = [dy.to(torch.float32) if d else w for dy, d, w in zip(dY_dev, direct, wide)]
            dYd[:] = [w if w is not None else dy for w, dy in zip(wide, dY_dev)]
            direct[:] = [False] * len(direct)
        _deform_may_decline(True, dXs, df, dYd, plan, gflags, stream, any(direct), widen)

        # gradient of the prefilter: its transpose along each deformed axis (deform_grid.py:276-286).
        # With a crop the scatter only touched a box of dX: the transposed filter runs on that box
        # plus its decay margin and the result replaces the box (the rest stays exactly zero, where
        # the whole-volume filter would leave values below 1e-18 of the gradient's scale).
        wins = _crop_windows(plan, dXs, _desc(df), dflag, crop, prefilter, device, stream, grid_stays=True)
        dXf = []
        for i, x in enumerate(dXs):
            if direct[i]:
                # the transposed chain in place in float32; its last pass narrows into the 16-bit result
                g16 = torch.empty(x.shape, dtype=dY_dev[i].dtype, device=device)
                if _lib.spline_filter_axes(_desc(x), _desc(g16), list(plan.axis[i]), int(plan.order[i]), True,
                                           _flags | _lib.FLAG_FAST | _lib.FLAG_SCRATCH_INPUT, stream,
                                           may_decline=True) == 0:
                    dXf.append(g16)
                    continue
                direct[i] = False
                wide[i] = x                 # (float32 chain below, narrowed by a cast)
            if not (prefilter and plan.order[i] > 1):
                dXf.append(x)
            elif wins[i] is not None and _lib.spline_filter_axes_window(
                    _desc(x), _desc(x), list(plan.axis[i]), int(plan.order[i]), True, wins[i].data_ptr(), _flags,
                    stream) == 0:
                dXf.append(x)           # in place, inside the window; the rest of dX stays exactly zero
            else:
                dXf.append(_filter_axes(x, plan.axis[i], int(plan.order[i]), True, device, overwrite=True,
                                        stream=stream))
        dXf = [_narrow(x, dy) if w is not None else x for x, dy, w in zip(dXf, dY_dev, wide)]
        res = [_from_device(x, dy) for x, dy in zip(dXf, dYs)]
        if sig is not None:
            _lane_build(sig, True, dY_dev, dd, plan, prefilter, X_shape, crop)
    return res if isinstance(dY, list) else res[0]


# ---- batches: one control grid per sample -----------------------

def _batch_plan(X, displacements, order, mode, cval, crop, axis, affine, rotate, zoom):
    """Normalise a batched call: X is (B, ...) -- sample b is X[b] -- and displacements is
    (B, naxis, n_0, ...).  `axis` counts the axes of ONE sample (like deform_grid's).  Returns the
    Plan of a single sample (shared by the whole batch).  The gradient call, which has no X, gives its shape
    (_host.ShapeOnly) after checking its dY itself."""
    if not isinstance(X, _host.ShapeOnly) and (not _host.is_array(X) or X.ndim < 2):
        raise Exception('X should be an array with a leading batch axis.')
    if not _host.is_array(displacements) or displacements.ndim < 3:
        raise Exception('displacements should be an array of shape (batch, naxis, n_0, ...).')
    assert displacements.shape[0] == X.shape[0], 'One displacement grid per sample is required.'
    assert not isinstance(order, (list, tuple)) and not isinstance(mode, (list, tuple)) and \
        not isinstance(cval, (list, tuple)), 'order, mode and cval are shared by the batch.'
    return _host.Plan([_host.ShapeOnly(X.shape[1:])], displacements[0], order, mode, cval, crop, axis, affine, rotate,
                      zoom)


def deform_grid_batch(X, displacements, order=3, mode='constant', cval=0.0, crop=None,
                      prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """
    :func:`deform_grid` over a batch with ONE CONTROL GRID PER SAMPLE: ``X`` has shape
    ``(B, ...)``, ``displacements`` ``(B, naxis, n_0, ..., n_{naxis-1})``; every other argument
    has the meaning it has for a single sample and is shared.  Returns ``(B, ...)``.

    Equivalent to ``stack([deform_grid(X[b], displacements[b], ...) for b in range(B)])`` --
    same results, bit for bit -- but the B samples are prefiltered together (the batch axis is just
    another outer axis of the filter passes) and deformed by ONE set of kernel launches
    (``edhip_deform_batch_strided``: the strip index of the tile kernels carries the sample), which
    removes the per-sample launches and host overhead that dominate for small volumes.  The reference has no batched entry point (one grid per call, deform_grid.py:52).
    """
    plan = _batch_plan(X, displacements, order, mode, cval, crop, axis, affine, rotate, zoom)
    torch = _torch()
    device = _device_for([X, displacements])
    with torch.cuda.device(device):
        Xd = _to_device(X, device)
        dd = _to_device(displacements, device)
        B = int(Xd.shape[0])
        ax = plan.axis[0]
        o = int(plan.order[0])
        Xf = Xd
        if prefilter and o > 1:
            Xf = _filter_axes(Xd, [a + 1 for a in ax], o, False, device)
        # all B control grids are prefiltered together (three launches for the batch; same values as
        # the per-call RAW_DISPLACEMENT path: a test pins that), then ONE library call and -- for
        # float volumes with 3 deformed axes -- one tables launch + one tile launch for all B samples
        df = _filter_axes(dd, range(2, dd.ndim), 3, False, device)
        out = torch.empty((B,) + tuple(int(v) for v in plan.output_shapes[0]), dtype=Xd.dtype, device=device)
        (xd, xs), (dd0, ds), (od, os_) = _desc_sample0(Xf), _desc_sample0(df), _desc_sample0(out)
        # the buffer of the filtered grids is kept for the gradient call of the same displacement
        # tensor: it takes this call's tile boxes (see _box_owner and deform_grid_gradient_batch)
        stream = _stream(device)
        ident = _box_id(displacements, dd)
        _batch_grids[(device.index, stream)] = (ident, df) if ident is not None else None
        _box_owner[(device.index, stream)] = None
        _lib.deform_batch_strided(False, B, xd, xs, dd0, ds, plan.output_offset, od, os_, ax, o,
                                  int(plan.mode[0]), float(plan.cval[0]), plan.inverse_affine,
                                  _flags | _route_flags() | (_lib.FLAG_KEEP_BOXES if ident is not None else 0), stream)
        return _from_device(out, X)


def deform_grid_gradient_batch(dY, displacements, order=3, mode='constant', cval=0.0, crop=None,
                               prefilter=True, axis=None, X_shape=None, affine=None, rotate=None,
                               zoom=None):
    """Gradient of :func:`deform_grid_batch` with respect to ``X``.  ``X_shape`` is the shape of
    ONE sample (required with a crop)."""
    if not _host.is_array(dY) or dY.ndim < 2:
        raise Exception('dY should be an array with a leading batch axis.')
    if X_shape is None:
        if crop is not None:
            raise ValueError("X_shape is required if the crop parameter is given.")
        X_shape = tuple(dY.shape[1:])
    plan = _batch_plan(_host.ShapeOnly((dY.shape[0],) + tuple(X_shape)), displacements, order, mode, cval, crop, axis,
                       affine, rotate, zoom)
    if tuple(plan.output_shapes[0]) != tuple(dY.shape[1:]):
        raise ValueError("X_shape does not match output shape and cropping. "
                         "Expected output shape is %s, but %s given."
                         % (str(plan.output_shapes[0]), str(tuple(dY.shape[1:]))))
    torch = _torch()
    device = _device_for([dY, displacements])
    with torch.cuda.device(device):
        dYd = _to_device(dY, device)
        dd = _to_device(displacements, device)
        B = int(dYd.shape[0])
        dX = torch.zeros((B,) + tuple(int(v) for v in X_shape), dtype=dYd.dtype, device=device)
        ax = plan.axis[0]
        o = int(plan.order[0])
        stream = _stream(device)
        kept = _batch_grids.get((device.index, stream))
        ident = _box_id(displacements, dd)
        bflag = 0
        # The control grids are ALWAYS prefiltered again (three small launches): storage address +
        # version counter say nothing certain about contents (a new tensor on a freed one's address, a
        # `.data` write).  Only the forward call's tile boxes are handed over -- the kernel treats
        # them as a hint it verifies per voxel -- and for that the fresh grids are written into the
        # forward call's buffer, whose address is the library's key for the boxes.
        df = _filter_axes(dd, range(2, dd.ndim), 3, False, device)
        if kept is not None and ident is not None and kept[0] == ident and kept[1].shape == df.shape \
                and kept[1].dtype == df.dtype:
            kept[1].copy_(df)
            df = kept[1]
            bflag = _lib.FLAG_USE_BOXES
        (xd, xs), (dd0, ds), (yd, ys) = _desc_sample0(dX), _desc_sample0(df), _desc_sample0(dYd)
        _lib.deform_batch_strided(True, B, xd, xs, dd0, ds, plan.output_offset, yd, ys, ax, o,
                                  int(plan.mode[0]), float(plan.cval[0]), plan.inverse_affine, _flags | bflag,
                                  stream)
        if prefilter and o > 1:
            dX = _filter_axes(dX, [a + 1 for a in ax], o, True, device, overwrite=True)
        return _from_device(dX, dY)


# ---- gradient with respect to the control-point displacement (no counterpart in the reference) ---------

_FLOAT_VOLUMES = ('float32', 'float64')


def _volume_dtype_name(a):
    return a.dtype.name if isinstance(a, numpy.ndarray) else str(a.dtype).replace('torch.', '')


def _check_float_volumes(arrays):
    """float32 / float64 volumes and dY only -- checked before anything touches the device."""
    for a in arrays:
        if _volume_dtype_name(a) not in _FLOAT_VOLUMES:
            raise RuntimeError('data type not supported')


def _dgrad_dtype(displacement):
    """The result's dtype: the displacement's own when it is floating, float64 otherwise."""
    torch = _torch()
    if isinstance(displacement, numpy.ndarray):
        return displacement.dtype if displacement.dtype.kind == 'f' else numpy.dtype('float64')
    return displacement.dtype if displacement.dtype.is_floating_point else torch.float64


def _dgrad_zeros(displacement, like):
    """Zeros of the displacement's shape and the result dtype, in the family / on the device of `like`."""
    dt = _dgrad_dtype(displacement)
    shape = tuple(int(v) for v in displacement.shape)
    if isinstance(like, numpy.ndarray):
        return numpy.zeros(shape, dtype=dt if isinstance(dt, numpy.dtype) else numpy.float64)
    torch = _torch()
    if isinstance(dt, numpy.dtype):
        dt = getattr(torch, dt.name)
    return torch.zeros(shape, dtype=dt, device=like.device)


def _result_tensor_dtype(displacement):
    torch = _torch()
    dt = _dgrad_dtype(displacement)
    return getattr(torch, dt.name) if isinstance(dt, numpy.dtype) else dt


def _transform_gradient_run(plan, Xs, axes, dYs, displacement, grid_axis, dk_shape, prefilter, zoom, want_disp,
                            want_map, call):
    """What _transform_gradient and _transform_gradient_batch share, so that a batch sample cannot differ from the
    single call: the checks, the prefilter of the inputs `Xs` along `axes`, the results' allocation, the control grid
    raw or filtered here (its grid axes start at `grid_axis`: 1, or 2 behind a batch axis), the ONE library call
    `call(Xf, dYd, df, dp, dk, flags, stream)` on device tensors (dp / dk: None = not wanted) and the transposed grid
    filter.  Returns (d displacement in the family of dYs[0] or None, dK of `dk_shape` or None)."""
    _check_float_volumes(list(Xs) + list(dYs))
    if want_map and zoom is not None and float(zoom) == 0:
        raise ValueError("zoom=0 means 'no zoom' (as in the reference): it has no gradient")
    torch = _torch()
    if _host.degenerate_axis([x.shape for x in Xs], axes):
        # (a deformed axis of length 1: every voxel is the constant, nothing depends on the grid or the map)
        dk = None
        if want_map:
            dk = torch.zeros(dk_shape, dtype=torch.float64, device=dYs[0].device if torch.is_tensor(dYs[0]) else 'cpu')
        return (_dgrad_zeros(displacement, dYs[0]) if want_disp else None), dk
    device = _device_for(list(dYs) + list(Xs) + [displacement])
    with torch.cuda.device(device):
        stream = _stream(device)
        Xf = []
        for i, x in enumerate(Xs):
            x = _to_device(x, device)
            if prefilter and plan.order[i] > 1:
                x = _filter_axes(x, axes[i], int(plan.order[i]), False, device, stream=stream)
            Xf.append(x)
        dYd = [_to_device(dy, device) for dy in dYs]
        dd = _to_device(displacement, device)
        dk = torch.empty(dk_shape, dtype=torch.float64, device=device) if want_map else None
        out = None
        if want_disp:
            out = torch.empty(tuple(int(v) for v in dd.shape), dtype=_result_tensor_dtype(displacement), device=device)
        grid_axes = range(grid_axis, dd.ndim)
        raw = math.prod(dd.shape[grid_axis - 1:]) <= _lib.RAW_DISPLACEMENT_MAX_POINTS     # (points per grid)
        # a large grid: prefiltered here, the gradient of the prefiltered grid transposed here (fp64 throughout)
        df = dd if raw else _filter_axes(dd, grid_axes, 3, False, device, stream=stream)
        dp = out if (raw or out is None) else torch.empty(out.shape, dtype=torch.float64, device=device)
        call(Xf, dYd, df, dp, dk, _flags | (_lib.FLAG_RAW_DISPLACEMENT if raw else 0), stream)
        if out is not None and not raw:
            dp = _filter_axes(dp, grid_axes, 3, True, device, overwrite=True, stream=stream)
            out.copy_(dp)
        return (_from_device(out, dYs[0]) if out is not None else None), dk


def _transform_gradient(X, dY, displacement, order=3, mode='constant', cval=0.0, crop=None, prefilter=True,
                        axis=None, affine=None, rotate=None, zoom=None, want_disp=True, want_map=False):
    """One library call for the gradients with respect to the displacement (`want_disp`) and to the inverse map
    (`want_map`).  Returns (plan, dYs, d displacement or None, dK or None): the displacement's result in the family
    of dY, dK a float64 tensor (naxis, naxis+1) on the device."""
    Xs = _host.normalize_inputs(X)
    dYs = _host.normalize_inputs(dY)
    plan = _host.cached_plan(Xs, displacement, order, mode, cval, crop, axis, affine, rotate, zoom)
    if len(dYs) != len(Xs) or [tuple(s) for s in plan.output_shapes] != [tuple(int(v) for v in dy.shape)
                                                                        for dy in dYs]:
        raise ValueError("dY does not match the output shape of deform_grid. Expected output shape is %s, "
                         "but %s given." % (str(plan.output_shapes), str([tuple(dy.shape) for dy in dYs])))

    def call(Xf, dYd, df, dp, dk, flags, stream):
        _lib.deform_transform_gradient([_desc(x) for x in Xf], _desc(df), plan.output_offset,
                                       [_desc(dy) for dy in dYd], plan.axis, plan.order, plan.mode, plan.cval,
                                       plan.inverse_affine, _desc(dp) if dp is not None else None,
                                       _desc(dk) if dk is not None else None, flags, stream,
                                       prepared=_prepared(plan, len(Xf)))
    n = plan.naxis
    ddisp, dk = _transform_gradient_run(plan, Xs, plan.axis, dYs, displacement, 1, (n, n + 1), prefilter, zoom,
                                        want_disp, want_map, call)
    return plan, dYs, ddisp, dk


def deform_grid_displacement_gradient(X, dY, displacement, order=3, mode='constant', cval=0.0, crop=None,
                                      prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """
    Gradient of :func:`deform_grid` with respect to the control-point ``displacement``: the array
    ``d(sum_i <dY_i, Y_i>) / d displacement`` where ``Y = deform_grid(X, displacement, ...)`` with the same
    arguments (the order-3 prefilter of the grid included).  ``X`` and ``dY`` are arrays or lists of arrays
    (float32 / float64), ``dY[i]`` of the shape of ``Y[i]``.  Returns an array of the displacement's shape, in its
    dtype when that is floating (float64 otherwise): numpy for a numpy ``dY``, otherwise a tensor on ``dY``'s
    device.  The sum over the volume runs in fp64 in a fixed order: repeated calls return the same bits.
    """
    return _transform_gradient(X, dY, displacement, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom,
                               True, False)[2]


def _transform_gradient_batch(X, dY, displacements, order=3, mode='constant', cval=0.0, crop=None, prefilter=True,
                              axis=None, affine=None, rotate=None, zoom=None, want_disp=True, want_map=False):
    """The batch form of _transform_gradient: (plan, d displacements or None, dK (B, naxis, naxis+1) or None)."""
    plan = _batch_plan(X, displacements, order, mode, cval, crop, axis, affine, rotate, zoom)
    if not _host.is_array(dY) or tuple(int(v) for v in dY.shape) != (int(X.shape[0]),) + tuple(plan.output_shapes[0]):
        raise ValueError("dY does not match the output shape of deform_grid_batch. Expected output shape is %s, "
                         "but %s given." % (str((int(X.shape[0]),) + tuple(plan.output_shapes[0])),
                                            str(tuple(dY.shape) if _host.is_array(dY) else dY)))
    B = int(X.shape[0])
    ax = plan.axis[0]

    def call(Xf, dYd, df, dp, dk, flags, stream):
        (xd, xs), (yd, ys), (gd, gs) = _desc_sample0(Xf[0]), _desc_sample0(dYd[0]), _desc_sample0(df)
        (pd, ps) = _desc_sample0(dp) if dp is not None else (None, 0)
        (kd, ks) = _desc_sample0(dk) if dk is not None else (None, 0)
        _lib.deform_transform_gradient_batch_strided(B, xd, xs, gd, gs, plan.output_offset, yd, ys, ax,
                                                     int(plan.order[0]), int(plan.mode[0]), float(plan.cval[0]),
                                                     plan.inverse_affine, pd, ps, kd, ks, flags, stream)
    n = plan.naxis
    # (the batch axis is just another outer axis of the stacked arrays: the deformed axes and the grid's move up by one)
    ddisp, dk = _transform_gradient_run(plan, [X], [[a + 1 for a in ax]], [dY], displacements, 2, (B, n, n + 1),
                                        prefilter, zoom, want_disp, want_map, call)
    return plan, ddisp, dk


def deform_grid_displacement_gradient_batch(X, dY, displacements, order=3, mode='constant', cval=0.0, crop=None,
                                            prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """:func:`deform_grid_displacement_gradient` over a batch, following :func:`deform_grid_batch`: ``X`` is
    ``(B, ...)``, ``dY`` the gradient of the batch's output, ``displacements`` ``(B, naxis, n_0, ...)``.  Returns
    ``(B, naxis, n_0, ...)``; sample ``b`` is the same bits as the single call on sample ``b``."""
    return _transform_gradient_batch(X, dY, displacements, order, mode, cval, crop, prefilter, axis, affine, rotate,
                                     zoom, True, False)[1]


# ---- gradient with respect to affine, rotate and zoom (no counterpart in the reference) -------------------------

AffineGradient = collections.namedtuple('AffineGradient', ['affine', 'rotate', 'zoom', 'inverse_map'])


def _affine_jacobian(plan, affine, rotate, zoom, device):
    """(J, shape of the affine gradient) of the plan -- J = d inverse_map / d(affine, rotate, zoom), formed once per
    plan on the host (_affine_grad.jacobian); with a device: J as a float64 tensor there, kept with the plan so that a
    repeated call (and a HIP graph capture after warm-up) copies nothing to the device."""
    if plan.affine_jacobian is None:
        from . import _affine_grad
        J, ashape = _affine_grad.jacobian(affine, rotate, zoom, plan.naxis,
                                          [plan.output_shapes[0][d] for d in plan.axis[0]])
        plan.affine_jacobian = (J, ashape, {})
    J, ashape, on_device = plan.affine_jacobian
    if device is None:
        return J, ashape
    key = str(device)
    if key not in on_device:
        on_device[key] = _torch().from_numpy(J).to(device)
    return on_device[key], ashape


def _affine_result(dk, plan, affine, rotate, zoom, numpy_out):
    """dK (naxis, naxis+1) -> AffineGradient: theta = J^T vec(dK), split into the affine (its own shape), rotate and
    zoom; numpy / floats when `numpy_out`, otherwise float64 tensors on dK's device."""
    torch = _torch()
    if numpy_out:
        g = dk.cpu().numpy() if torch.is_tensor(dk) else numpy.asarray(dk)
        J, ashape = _affine_jacobian(plan, affine, rotate, zoom, None)
        theta = numpy.dot(J.T, g.reshape(-1))
    else:
        g = dk
        J, ashape = _affine_jacobian(plan, affine, rotate, zoom, dk.device)
        theta = (J * g.reshape(-1, 1)).sum(0)
    na = int(numpy.prod(ashape))
    k = na
    rot = zm = None
    if rotate is not None:
        rot = float(theta[k]) if numpy_out else theta[k]
        k += 1
    if zoom is not None:
        zm = float(theta[k]) if numpy_out else theta[k]
    return AffineGradient(theta[:na].reshape(ashape), rot, zm, g)


def deform_grid_affine_gradient(X, dY, displacement, order=3, mode='constant', cval=0.0, crop=None, prefilter=True,
                                axis=None, affine=None, rotate=None, zoom=None):
    """
    Gradient of :func:`deform_grid` with respect to its affine part: ``L = sum_i <dY_i, Y_i>`` differentiated with
    respect to ``affine``, ``rotate`` and ``zoom``.  Arguments and checks as for
    :func:`deform_grid_displacement_gradient`.  Returns ``AffineGradient(affine, rotate, zoom, inverse_map)``:

    * ``affine``: dL / d affine in the shape given (the homogeneous 3 x 3 in 2-D included); with ``affine=None`` the
      gradient at the identity, shape (naxis, naxis+1).
    * ``rotate`` (per degree) / ``zoom``: when they are given, otherwise None (2-D only, as in the reference;
      ``zoom=0`` means "no zoom" there and raises ValueError here).
    * ``inverse_map``: dL / dK for the map K the kernels apply to the crop-local output index, c = K [o; 1] + offset
      + displacement (what a spatial transformer parameterises directly).

    numpy (floats for rotate / zoom) for a numpy ``dY``, otherwise float64 tensors on ``dY``'s device.  dK is summed
    in fp64 in a fixed order on the GPU (repeated calls return the same bits); the chain rule to the parameters is
    the Jacobian of a float64 restatement of the reference's matrix algebra.
    """
    plan, dYs, _, dk = _transform_gradient(X, dY, displacement, order, mode, cval, crop, prefilter, axis, affine,
                                           rotate, zoom, False, True)
    return _affine_result(dk, plan, affine, rotate, zoom, isinstance(dYs[0], numpy.ndarray))


def _sum_in_order(parts):
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total


def _affine_result_batch(dk, plan, affine, rotate, zoom, numpy_out):
    """per-sample AffineGradients of dK (B, naxis, naxis+1), summed over b = 0, 1, ... in that order"""
    per = [_affine_result(dk[b], plan, affine, rotate, zoom, numpy_out) for b in range(int(dk.shape[0]))]
    return AffineGradient(*[None if getattr(per[0], f) is None else _sum_in_order([getattr(r, f) for r in per])
                            for f in AffineGradient._fields])


def deform_grid_affine_gradient_batch(X, dY, displacements, order=3, mode='constant', cval=0.0, crop=None,
                                      prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """:func:`deform_grid_affine_gradient` over a batch (:func:`deform_grid_batch`: ``X`` ``(B, ...)``,
    ``displacements`` ``(B, naxis, n_0, ...)``).  ``affine`` / ``rotate`` / ``zoom`` are shared by the batch, so the
    result is the SUM over the samples: every field is each sample's value (the single call on that sample, same
    bits) added in fp64 in sample order, b = 0, 1, ..., B-1."""
    plan, _, dk = _transform_gradient_batch(X, dY, displacements, order, mode, cval, crop, prefilter, axis, affine,
                                            rotate, zoom, False, True)
    return _affine_result_batch(dk, plan, affine, rotate, zoom, isinstance(dY, numpy.ndarray))


# ---- the coordinate map at real positions and its inverse (no counterpart in the reference) ---------------------

_POINT_DTYPES = ('float32', 'float64')


def _as_points(points):
    """positions as a float32 / float64 array of the caller's family; integer arrays are taken as float64"""
    if not _host.is_array(points):
        points = numpy.asarray(points)
    if isinstance(points, numpy.ndarray):
        if points.dtype.kind in 'iub':
            return points.astype(numpy.float64)
        if points.dtype.name not in _POINT_DTYPES:
            raise RuntimeError('data type not supported')
        return points
    torch = _torch()
    if points.dtype in (torch.float32, torch.float64):
        return points.detach()
    if points.is_floating_point() or points.is_complex():
        raise RuntimeError('data type not supported')
    return points.detach().to(torch.float64)


def _fill(like, shape, value, dtype=None):
    """an array of `shape` filled with `value`, in the family and on the device of `like`; `like`'s dtype unless given"""
    shape = tuple(int(v) for v in shape)
    if isinstance(like, numpy.ndarray):
        return numpy.full(shape, value, dtype=like.dtype if dtype is None else dtype)
    torch = _torch()
    return torch.full(shape, value, dtype=like.dtype if dtype is None else getattr(torch, dtype), device=like.device)


def _check_iteration(max_iter, tol):
    if int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError("max_iter should be a positive integer.")
    if not float(tol) > 0.0:
        raise ValueError("tol should be positive.")


def _plan_of(arrays, batch, displacement, order, mode, cval, crop, axis, affine, rotate, zoom):
    """the Plan of deform_grid on `arrays` (or _host.ShapeOnly stand-ins): a list of inputs, or [the stacked batch]"""
    if batch:
        return _batch_plan(arrays[0], displacement, order, mode, cval, crop, axis, affine, rotate, zoom)
    return _host.cached_plan(arrays, displacement, order, mode, cval, crop, axis, affine, rotate, zoom)


def _shape_only(shape, nbatch=None):
    """[the stand-in of an array of `shape` -- of a stacked batch of `nbatch` of them --] for _plan_of"""
    return [_host.ShapeOnly(((int(nbatch),) if nbatch is not None else ()) + tuple(shape))]


def _grid_axes(dd, batch):
    return range(2 if batch else 1, dd.ndim)


def _prefiltered_grid(dd, batch, device, stream):
    """the control grid prefiltered like deform_grid's (order 3, mirror, rounded to its own dtype per axis)"""
    return _filter_axes(dd, _grid_axes(dd, batch), 3, False, device, stream=stream)


def _sample(t, batch):
    """(descriptor of t -- of sample 0 of a stacked t --, byte distance between samples); (None, 0) for None"""
    if t is None:
        return None, 0
    return _desc_sample0(t) if batch else (_desc(t), 0)


def _forward_linear(K, n):
    """M = (K[:, :n])^-1, where the Newton iteration starts; None without an affine map"""
    return numpy.linalg.inv(numpy.asarray(K, dtype=numpy.float64)[:, :n]) if K is not None else None


def _list_or_one(results, extras, paired, like):
    """a list in gives a list out; with `paired`, (result, extra) pairs"""
    out = list(zip(results, extras)) if paired else results
    return out if isinstance(like, list) else out[0]


def _points_plan(pts, X_shape, batch, displacement, crop, axis, affine, rotate, zoom):
    """(Plan of the image call on an array of X_shape, naxis, the leading dimensions of the points)"""
    _check_batch_points(pts, batch)
    plan = _plan_of(_shape_only(X_shape, pts.shape[0] if batch else None), batch, displacement, 3, 'constant', 0.0,
                    crop, axis, affine, rotate, zoom)
    return (plan,) + _points_of_plan(pts, plan)


def _check_batch_points(pts, batch):
    if batch and pts.ndim != 3:
        raise ValueError("points should have shape (batch, N, naxis).")


def _points_of_plan(pts, plan):
    """(naxis, the leading dimensions of the points), the points checked against the Plan's deformed axes"""
    n = plan.naxis
    if pts.ndim < 1 or int(pts.shape[-1]) != n:
        raise ValueError("The last dimension of the points should equal the number of deformed axes (%d), "
                         "but their shape is %s." % (n, str(tuple(pts.shape))))
    return n, tuple(int(v) for v in pts.shape[:-1])


def _points_map(points, displacement, X_shape, crop, axis, affine, rotate, zoom, inverse, jacobian, max_iter, tol,
                batch, hessian=None):
    """Both directions of the coordinate map, single call and batch.  Returns (coordinates, jacobian or None,
    converged or None) with the leading dimensions of `points`.  `hessian` given (forward direction only): the
    derivatives call, 1 to 3 deformed axes -- the third result is then H = d^2r/dq dq (float64) for True, None for
    False.  Every argument check runs before the device is touched: offsets, the inverse map K and the rotate / zoom
    centre are the image call's own (the same Plan)."""
    if X_shape is None:
        raise ValueError("X_shape is required: the shape of the array deform_grid deforms.")
    if inverse:
        _check_iteration(max_iter, tol)
    X_shape = tuple(int(v) for v in X_shape)
    pts = _as_points(points)
    plan, n, lead = _points_plan(pts, X_shape, batch, displacement, crop, axis, affine, rotate, zoom)
    if hessian is not None and n > 3:
        raise RuntimeError('deform_grid_derivatives takes 1 to 3 deformed axes')   # (the library's own limit)

    if any(int(d) == 1 for d in plan.deform_shape):
        # a deformed axis of length 1: the control coordinate divides by I - 1 = 0 (the image call maps every voxel
        # to cval there) -- no coordinate is defined and nothing converges
        return (_fill(pts, lead + (n,), float('nan')),
                _fill(pts, lead + (n, n), float('nan'), 'float64') if jacobian else None,
                _fill(pts, lead, False, 'bool') if inverse else
                _fill(pts, lead + (n, n, n), float('nan'), 'float64') if hessian else None)

    K = plan.inverse_affine
    M = _forward_linear(K, n) if inverse else None
    torch = _torch()
    device = _device_for([pts, displacement])
    with torch.cuda.device(device):
        stream = _stream(device)
        pd = _to_device(pts, device)
        if not batch:
            pd = pd.reshape(-1, n)
        df = _prefiltered_grid(_to_device(displacement, device), batch, device, stream)
        res = torch.empty(tuple(pd.shape), dtype=pd.dtype, device=device)
        jac = torch.empty(tuple(pd.shape) + (n,), dtype=torch.float64, device=device) if jacobian else None
        ok = torch.empty(tuple(pd.shape[:-1]), dtype=torch.uint8, device=device) if inverse else None
        if hessian is None:
            _lib.deform_points(inverse, lead[0] if batch else 1, *_sample(pd, batch), *_sample(df, batch),
                               plan.deform_shape, plan.output_offset, K, M, *_sample(res, batch), *_sample(jac, batch),
                               *_sample(ok, batch), int(max_iter), float(tol), 0, stream)
        else:
            hess = torch.empty(tuple(pd.shape) + (n, n), dtype=torch.float64, device=device) if hessian else None
            _lib.deform_points_derivatives(lead[0] if batch else 1, *_sample(pd, batch), *_sample(df, batch),
                                           plan.deform_shape, plan.output_offset, K, *_sample(res, batch),
                                           *_sample(jac, batch), *_sample(hess, batch), 0, stream)
        res = _from_device(res.reshape(lead + (n,)), pts)
        if jac is not None:
            jac = _from_device(jac.reshape(lead + (n, n)), pts)
        if ok is not None:
            ok = _from_device(ok.reshape(lead).to(torch.bool), pts)
        elif hessian:
            ok = _from_device(hess.reshape(lead + (n, n, n)), pts)
    return res, jac, ok


def deform_grid_coordinates(positions, displacement, X_shape, crop=None, axis=None, affine=None, rotate=None,
                            zoom=None, jacobian=False):
    """
    The coordinate map of :func:`deform_grid` at arbitrary real positions: for every crop-local output position
    ``q`` (``positions``, shape ``(..., naxis)``) the source coordinate ``r(q)`` at which
    ``deform_grid(X, displacement, crop=crop, axis=axis, affine=affine, rotate=rotate, zoom=zoom)`` samples ``X``
    for that output position -- ``Y[o] = X(r(o))`` at integer ``o``, before the boundary mode.  ``X_shape`` is the
    shape of ``X``; the other arguments are deform_grid's own, checked the same way.

    No boundary mode is applied: ``r`` is the unfolded map, defined for every real ``q`` (the control spline is
    extended by its mirror tap map) and twice continuously differentiable.  With ``jacobian=True`` the result is
    ``(r, J)`` with ``J[..., h, l] = d r_h / d q_l`` (float64, analytic); ``det J <= 0`` somewhere means the field
    folds there.

    float32 / float64 positions keep their dtype (the arithmetic is fp64, a float32 result is rounded once); integer
    positions are taken as float64.  numpy in gives numpy out, otherwise the result is a tensor on the positions'
    device.  A deformed axis of length 1 gives NaN.  No autograd flows through this call itself:
    :func:`deform_grid_coordinates_gradient` is its adjoint and ``elasticdeform_amd.torch.deform_grid_coordinates``
    the differentiable wrapper.
    """
    r, J, _ = _points_map(positions, displacement, X_shape, crop, axis, affine, rotate, zoom, False, jacobian, 1,
                          1.0, False)
    return (r, J) if jacobian else r


def deform_points(points, displacement, X_shape, crop=None, axis=None, affine=None, rotate=None, zoom=None,
                  max_iter=32, tol=1e-9, return_converged=False):
    """
    Where source points land in the output of
    ``deform_grid(X, displacement, crop=crop, axis=axis, affine=affine, rotate=rotate, zoom=zoom)``: for every point
    ``p`` in the coordinates of ``X`` (``points``, shape ``(..., naxis)``; ``X_shape`` is the shape of ``X``) the
    crop-local output position ``q`` with ``r(q) = p``, ``r`` being :func:`deform_grid_coordinates`.  This is what
    landmarks, keypoints, box corners and mesh vertices need: ``deform_grid`` is a pull warp, ``Y[o] = X(r(o))``, so
    a landmark at ``p`` in ``X`` shows up in ``Y`` at the ``o`` with ``r(o) = p``.

    Solved per point by a damped Newton iteration in fp64 from the affine part's own inverse, stopped at
    ``|r(q) - p|_inf <= tol`` (voxels).  A point that is not solved within ``max_iter`` steps -- or whose Jacobian is
    singular, or that is not finite -- is NaN in every component; ``return_converged=True`` also returns the bool
    mask of the solved points.  On a folding field a point can have several pre-images: the result is the one this
    iteration reaches from its start, the same on every call.  The result may lie outside the output array: the
    point is then not visible in ``Y``.

    dtypes, array families and the length-1 axis as for :func:`deform_grid_coordinates` (nothing converges there).
    No autograd flows through this call itself: :func:`deform_points_gradient` is its adjoint and
    ``elasticdeform_amd.torch.deform_points`` the differentiable wrapper.
    """
    q, _, ok = _points_map(points, displacement, X_shape, crop, axis, affine, rotate, zoom, True, False, max_iter,
                           tol, False)
    return (q, ok) if return_converged else q


def deform_grid_coordinates_batch(positions, displacements, X_shape, crop=None, axis=None, affine=None, rotate=None,
                                  zoom=None, jacobian=False):
    """:func:`deform_grid_coordinates` over a batch with one control grid per sample (:func:`deform_grid_batch`):
    ``positions`` ``(B, N, naxis)``, ``displacements`` ``(B, naxis, n_0, ...)``, ``X_shape`` the shape of ONE
    sample; everything else is shared.  One launch for the batch; sample b equals the single call, bit for bit."""
    r, J, _ = _points_map(positions, displacements, X_shape, crop, axis, affine, rotate, zoom, False, jacobian, 1,
                          1.0, True)
    return (r, J) if jacobian else r


def deform_points_batch(points, displacements, X_shape, crop=None, axis=None, affine=None, rotate=None, zoom=None,
                        max_iter=32, tol=1e-9, return_converged=False):
    """:func:`deform_points` over a batch with one control grid per sample: ``points`` ``(B, N, naxis)``,
    ``displacements`` ``(B, naxis, n_0, ...)``, ``X_shape`` the shape of ONE sample; everything else is shared.
    One launch for the batch; sample b equals the single call, bit for bit."""
    q, _, ok = _points_map(points, displacements, X_shape, crop, axis, affine, rotate, zoom, True, False, max_iter,
                           tol, True)
    return (q, ok) if return_converged else q


# ---- gradients through the coordinate map and its inverse -------------------------------------------------------

PointsGradient = collections.namedtuple('PointsGradient',
                                        ['points', 'displacement', 'affine', 'rotate', 'zoom', 'inverse_map'])


def _points_gradient(points, cotangent, displacement, X_shape, crop, axis, affine, rotate, zoom, inverse, batch,
                     want_points=True, want_disp=True, want_map=True, max_iter=32, tol=1e-9, positions=None,
                     converged=None, derivatives=None):
    """The adjoint of _points_map, single call and batch: ONE library call for whatever is wanted.  `cotangent` is
    dL/dr(q) for the positions q = `points` (forward direction) or dL/dq for q = r^-1(points) (inverse; solved here
    in float64 through _points_map unless `positions`, the solved q, and optionally its mask `converged` are given).
    `derivatives` = (dL/dJ or None, dL/dH or None) (forward direction only): the adjoint of the derivatives call, 1 to
    3 deformed axes; `cotangent` may then be None, but not all three.
    Returns (plan, d points or None, d displacement or None, dK or None): the first two in the family of `points`, dK
    a float64 tensor (naxis, naxis+1) -- (B, naxis, naxis+1) for a batch -- on the device.  Every argument check
    runs before the device or the library is touched."""
    if X_shape is None:
        raise ValueError("X_shape is required: the shape of the array deform_grid deforms.")
    if inverse and positions is None:
        _check_iteration(max_iter, tol)
    X_shape = tuple(int(v) for v in X_shape)
    pts = _as_points(points)
    if derivatives is not None and cotangent is None and derivatives[0] is None and derivatives[1] is None:
        raise ValueError("At least one of d_coordinates, d_jacobian and d_hessian should be given.")
    cot = _as_points(cotangent) if cotangent is not None else None
    plan, n, lead = _points_plan(pts, X_shape, batch, displacement, crop, axis, affine, rotate, zoom)
    if cot is not None and tuple(int(v) for v in cot.shape) != tuple(int(v) for v in pts.shape):
        raise ValueError("The cotangent should have the shape of the points, %s, but its shape is %s."
                         % (str(tuple(pts.shape)), str(tuple(cot.shape))))
    higher = []
    if derivatives is not None:
        if n > 3:
            raise RuntimeError('deform_grid_derivatives_gradient takes 1 to 3 deformed axes')   # (the library's limit)
        for name, value, tail in zip(('d_jacobian', 'd_hessian'), derivatives, ((n,), (n, n))):
            value = _as_points(value) if value is not None else None
            want = tuple(int(v) for v in pts.shape) + tail
            if value is not None and tuple(int(v) for v in value.shape) != want:
                raise ValueError("%s should have shape %s, but its shape is %s."
                                 % (name, str(want), str(tuple(value.shape))))
            higher.append(value)
    if positions is not None:
        positions = _as_points(positions)
        if tuple(int(v) for v in positions.shape) != tuple(int(v) for v in pts.shape):
            raise ValueError("positions should have the shape of the points, %s, but their shape is %s."
                             % (str(tuple(pts.shape)), str(tuple(positions.shape))))
    if want_map and zoom is not None and float(zoom) == 0:
        raise ValueError("zoom=0 means 'no zoom' (as in the reference): it has no gradient")
    dk_shape = ((lead[0],) if batch else ()) + (n, n + 1)
    torch = _torch()

    if any(int(d) == 1 for d in plan.deform_shape):
        # a deformed axis of length 1: no coordinate is defined there, nothing depends on anything
        dk = None
        if want_map:
            dk = torch.zeros(dk_shape, dtype=torch.float64, device=pts.device if torch.is_tensor(pts) else 'cpu')
        return (plan, _fill(pts, lead + (n,), 0.0) if want_points else None,
                _dgrad_zeros(displacement, pts) if want_disp else None, dk)

    device = _device_for([pts, displacement] + [c for c in [cot] + higher if c is not None])
    with torch.cuda.device(device):
        stream = _stream(device)
        pd = _to_device(pts, device)
        cd = _to_device(cot, device) if cot is not None else None
        dd = _to_device(displacement, device)
        ok = None
        if inverse:
            if positions is None:
                # solved in float64, so that float32 points give the float64 call's rows, rounded once
                qd, _, okb = _points_map(pd.to(torch.float64), dd, X_shape, crop, axis, affine, rotate, zoom, True,
                                         False, max_iter, tol, batch)
                ok = okb.to(torch.uint8)
            else:
                qd = _to_device(positions, device)
                if converged is not None:
                    ok = _to_device(converged, device).to(torch.uint8)
        else:
            qd = pd
        hd = [_to_device(c, device) if c is not None else None for c in higher]
        if not batch:
            qd = qd.reshape(-1, n)
            cd = cd.reshape(-1, n) if cd is not None else None
            hd = [c.reshape((-1,) + tuple(c.shape[len(lead):])) if c is not None else None for c in hd]
            ok = ok.reshape(-1) if ok is not None else None
        df = _prefiltered_grid(dd, batch, device, stream)
        rows = torch.empty(tuple(qd.shape), dtype=pd.dtype, device=device) if want_points else None
        dp = torch.empty(tuple(int(v) for v in dd.shape), dtype=torch.float64, device=device) if want_disp else None
        dk = torch.empty(dk_shape, dtype=torch.float64, device=device) if want_map else None
        if derivatives is None:
            _lib.deform_points_gradient(inverse, lead[0] if batch else 1, *_sample(qd, batch), *_sample(cd, batch),
                                        *_sample(ok, batch), *_sample(df, batch), plan.deform_shape,
                                        plan.output_offset, plan.inverse_affine, *_sample(rows, batch),
                                        *_sample(dp, batch), *_sample(dk, batch), 0, stream)
        else:
            _lib.deform_points_derivatives_gradient(lead[0] if batch else 1, *_sample(qd, batch), *_sample(cd, batch),
                                                    *_sample(hd[0], batch), *_sample(hd[1], batch),
                                                    *_sample(df, batch), plan.deform_shape, plan.output_offset,
                                                    plan.inverse_affine, *_sample(rows, batch), *_sample(dp, batch),
                                                    *_sample(dk, batch), 0, stream)
        out = None
        if dp is not None:
            # dD = (order-3 mirror prefilter)^T dP in fp64, rounded once to the result's dtype
            dp = _filter_axes(dp, _grid_axes(dd, batch), 3, True, device, overwrite=True, stream=stream)
            out = _from_device(dp.to(_result_tensor_dtype(displacement)), pts)
        if rows is not None:
            rows = _from_device(rows.reshape(lead + (n,)), pts)
    return plan, rows, out, dk


def _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, numpy_out, batch):
    result = _affine_result_batch if batch else _affine_result
    return PointsGradient(rows, ddisp, *result(dk, plan, affine, rotate, zoom, numpy_out))


def deform_grid_coordinates_gradient(positions, d_coordinates, displacement, X_shape, crop=None, axis=None,
                                     affine=None, rotate=None, zoom=None):
    """
    Gradient through :func:`deform_grid_coordinates`: for ``L`` with ``d_coordinates = dL / d r`` (the shape of
    ``positions``, float32 / float64) and ``r = deform_grid_coordinates(positions, displacement, X_shape, ...)``,
    returns ``PointsGradient(points, displacement, affine, rotate, zoom, inverse_map)``:

    * ``points``: dL / d positions, ``J^T d_coordinates`` per point, in the shape and dtype of the positions (fp64
      arithmetic, a float32 row is rounded once);
    * ``displacement``: dL / d displacement (the order-3 prefilter of the grid included), as
      :func:`deform_grid_displacement_gradient` returns it;
    * ``affine`` / ``rotate`` / ``zoom`` / ``inverse_map``: as in :class:`AffineGradient` (``zoom=0`` raises).

    A position that is not finite (or absurdly far out) contributes nothing: its row is zero and its cotangent is
    ignored.  One non-finite cotangent elsewhere makes ``displacement`` and the map's fields NaN.  The sums over the
    points are accumulated in 64-bit integer fixed point (one contribution resolved to 2^-61 of N max|d_coordinates|):
    they are the same bits on every call and after any permutation of the points.  numpy in gives numpy out,
    otherwise tensors on the positions' device.  A deformed axis of length 1 gives zeros.
    """
    plan, rows, ddisp, dk = _points_gradient(positions, d_coordinates, displacement, X_shape, crop, axis, affine,
                                             rotate, zoom, False, False)
    return _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, isinstance(rows, numpy.ndarray),
                                   False)


def deform_points_gradient(points, d_positions, displacement, X_shape, crop=None, axis=None, affine=None,
                           rotate=None, zoom=None, max_iter=32, tol=1e-9, positions=None):
    """
    Gradient through :func:`deform_points`: for ``L`` with ``d_positions = dL / d q`` (the shape of ``points``) and
    ``q = deform_points(points, displacement, X_shape, ...)``, by the implicit function theorem at the solved ``q``:
    ``points`` is ``J(q)^-T d_positions`` per point, ``displacement`` / ``affine`` / ``rotate`` / ``zoom`` /
    ``inverse_map`` the sums of :func:`deform_grid_coordinates_gradient` with ``-J(q)^-T d_positions`` in place of
    the cotangent.  This is what a landmark loss, a keypoint-consistency term or a fit to point correspondences
    differentiates.

    The inverse is solved here (in float64, with ``max_iter`` / ``tol``) unless ``positions``, the solved ``q``, is
    given.  Points that are not solved (NaN), or whose Jacobian is singular, contribute nothing: a zero row, their
    cotangent ignored.  Everything else as for :func:`deform_grid_coordinates_gradient`.
    """
    plan, rows, ddisp, dk = _points_gradient(points, d_positions, displacement, X_shape, crop, axis, affine, rotate,
                                             zoom, True, False, max_iter=max_iter, tol=tol, positions=positions)
    return _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, isinstance(rows, numpy.ndarray),
                                   False)


def deform_grid_coordinates_gradient_batch(positions, d_coordinates, displacements, X_shape, crop=None, axis=None,
                                           affine=None, rotate=None, zoom=None):
    """:func:`deform_grid_coordinates_gradient` over a batch with one control grid per sample: ``positions`` and
    ``d_coordinates`` ``(B, N, naxis)``, ``displacements`` ``(B, naxis, n_0, ...)``, ``X_shape`` the shape of ONE
    sample.  ``points`` and ``displacement`` are per sample, the same bits as the single call on that sample; the
    map's fields are the sum over the samples in sample order (:func:`deform_grid_affine_gradient_batch`)."""
    plan, rows, ddisp, dk = _points_gradient(positions, d_coordinates, displacements, X_shape, crop, axis, affine,
                                             rotate, zoom, False, True)
    return _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, isinstance(rows, numpy.ndarray),
                                   True)


def deform_points_gradient_batch(points, d_positions, displacements, X_shape, crop=None, axis=None, affine=None,
                                 rotate=None, zoom=None, max_iter=32, tol=1e-9, positions=None):
    """:func:`deform_points_gradient` over a batch with one control grid per sample; shapes and the summed fields
    as for :func:`deform_grid_coordinates_gradient_batch`."""
    plan, rows, ddisp, dk = _points_gradient(points, d_positions, displacements, X_shape, crop, axis, affine, rotate,
                                             zoom, True, True, max_iter=max_iter, tol=tol, positions=positions)
    return _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, isinstance(rows, numpy.ndarray),
                                   True)


# ---- r, J and H of the coordinate map at real positions, with gradients (no counterpart in the reference) ---------

MapDerivatives = collections.namedtuple('MapDerivatives', ['coordinates', 'jacobian', 'hessian'])


def deform_grid_derivatives(positions, displacement, X_shape, crop=None, axis=None, affine=None, rotate=None,
                            zoom=None, hessian=True):
    """
    The local differential structure of the coordinate map of :func:`deform_grid` at arbitrary real positions: for
    every crop-local output position ``q`` (``positions``, shape ``(..., naxis)``) returns
    ``MapDerivatives(coordinates, jacobian, hessian)`` with

    * ``coordinates``: ``r(q)``, exactly what :func:`deform_grid_coordinates` returns;
    * ``jacobian``: ``J[..., h, l] = d r_h / d q_l`` (float64), exactly its ``jacobian=True`` result;
    * ``hessian``: ``H[..., h, l, m] = d^2 r_h / d q_l d q_m`` (float64, shape ``(..., n, n, n)``), symmetric in its
      last two axes bit for bit and independent of affine / rotate / zoom; ``None`` with ``hessian=False`` (the
      second-derivative sweep is skipped).

    This is what a local regulariser evaluated at sampled positions needs: folding (``relu(-det J)``), ``log det``,
    volume preservation, rigidity (``|J^T J - I|^2``), diffusion (``|J - I|^2``) and the bending energy (``|H|^2``).
    ``r`` is twice continuously differentiable: ``H`` is continuous and piecewise linear in ``q``.

    1 to 3 deformed axes.  dtypes, array families and the other arguments as for :func:`deform_grid_coordinates`; a
    position that is not finite gives NaN in all three; a deformed axis of length 1 gives NaN.  No autograd flows
    through this call itself: :func:`deform_grid_derivatives_gradient` is its adjoint and
    ``elasticdeform_amd.torch.deform_grid_derivatives`` the differentiable wrapper.
    """
    return MapDerivatives(*_points_map(positions, displacement, X_shape, crop, axis, affine, rotate, zoom, False, True,
                                       1, 1.0, False, hessian=bool(hessian)))


def deform_grid_derivatives_batch(positions, displacements, X_shape, crop=None, axis=None, affine=None, rotate=None,
                                  zoom=None, hessian=True):
    """:func:`deform_grid_derivatives` over a batch with one control grid per sample: ``positions`` ``(B, N, naxis)``,
    ``displacements`` ``(B, naxis, n_0, ...)``, ``X_shape`` the shape of ONE sample; everything else is shared.  One
    launch for the batch; sample b equals the single call, bit for bit."""
    return MapDerivatives(*_points_map(positions, displacements, X_shape, crop, axis, affine, rotate, zoom, False,
                                       True, 1, 1.0, True, hessian=bool(hessian)))


def deform_grid_derivatives_gradient(positions, displacement, X_shape, d_coordinates=None, d_jacobian=None,
                                     d_hessian=None, crop=None, axis=None, affine=None, rotate=None, zoom=None):
    """
    Gradient through :func:`deform_grid_derivatives`: for ``L`` with ``d_coordinates = dL / d r`` (the shape of
    ``positions``), ``d_jacobian = dL / d J`` (``(..., n, n)``) and ``d_hessian = dL / d H`` (``(..., n, n, n)``; it
    need not be symmetric) -- float32 / float64, any of them ``None`` but not all -- returns the
    ``PointsGradient(points, displacement, affine, rotate, zoom, inverse_map)`` of
    :func:`deform_grid_coordinates_gradient`, in ONE library call:

    * ``points``: ``dL / d positions`` per point, ``J^T d_coordinates + H : d_jacobian + T : d_hessian`` with ``T``
      the derivative of ``H`` (constant within a knot cell of the control grid; at a knot, the cell of ``floor``);
    * ``displacement``: ``dL / d displacement``, the order-3 prefilter of the grid included;
    * ``affine`` / ``rotate`` / ``zoom`` / ``inverse_map``: as in :class:`AffineGradient` (``zoom=0`` raises);
      ``d_hessian`` does not reach them.

    Positions that are not finite contribute nothing (a zero row, their cotangents ignored); one non-finite cotangent
    elsewhere makes ``displacement`` and the map's fields NaN.  The sums over the points are 64-bit integer fixed
    point: the same bits on every call and after any permutation of the points.  1 to 3 deformed axes; numpy in
    gives numpy out, otherwise tensors on the positions' device.  A deformed axis of length 1 gives zeros.
    """
    plan, rows, ddisp, dk = _points_gradient(positions, d_coordinates, displacement, X_shape, crop, axis, affine,
                                             rotate, zoom, False, False, derivatives=(d_jacobian, d_hessian))
    return _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, isinstance(rows, numpy.ndarray),
                                   False)


def deform_grid_derivatives_gradient_batch(positions, displacements, X_shape, d_coordinates=None, d_jacobian=None,
                                           d_hessian=None, crop=None, axis=None, affine=None, rotate=None, zoom=None):
    """:func:`deform_grid_derivatives_gradient` over a batch with one control grid per sample: ``positions``
    ``(B, N, naxis)`` and the cotangents with that leading shape, ``displacements`` ``(B, naxis, n_0, ...)``,
    ``X_shape`` the shape of ONE sample.  ``points`` and ``displacement`` are per sample, the same bits as the single
    call on that sample; the map's fields are the sum over the samples in sample order."""
    plan, rows, ddisp, dk = _points_gradient(positions, d_coordinates, displacements, X_shape, crop, axis, affine,
                                             rotate, zoom, False, True, derivatives=(d_jacobian, d_hessian))
    return _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, isinstance(rows, numpy.ndarray),
                                   True)


# ---- det J of the coordinate map on the voxel lattice, with gradients (no counterpart in the reference) ----------

JacobianGradient = collections.namedtuple('JacobianGradient',
                                          ['displacement', 'affine', 'rotate', 'zoom', 'inverse_map'])

_DET_DTYPES = ('float32', 'float64')


def _jacobian_plan(displacement, X_shape, crop, axis, affine, rotate, zoom, batch):
    """(Plan of the image call on an array of X_shape, naxis, the shape of det: the deformed axes of the output --
    behind the batch axis for a batch)"""
    if X_shape is None:
        raise ValueError("X_shape is required: the shape of the array deform_grid deforms.")
    X_shape = tuple(int(v) for v in X_shape)
    nbatch = None
    if batch:
        nbatch = int(displacement.shape[0]) if _host.is_array(displacement) and displacement.ndim >= 1 else 0
    plan = _plan_of(_shape_only(X_shape, nbatch), batch, displacement, 3, 'constant', 0.0, crop, axis, affine, rotate,
                    zoom)
    n = plan.naxis
    if n > 3:
        raise ValueError("deform_grid_jacobian takes 1 to 3 deformed axes, not %d." % n)
    lattice = tuple(int(plan.output_shapes[0][d]) for d in plan.axis[0])
    return plan, n, ((nbatch,) if batch else ()) + lattice


def _jacobian_run(displacement, X_shape, crop, axis, affine, rotate, zoom, dtype, batch):
    """deform_grid_jacobian, single call and batch.  Every argument check runs before the device is touched."""
    if dtype is None:
        name = 'float64'
    elif isinstance(dtype, str):
        name = dtype
    else:
        try:
            name = numpy.dtype(dtype).name
        except TypeError:
            name = str(dtype).replace('torch.', '')      # a torch dtype: torch.float32 -> 'float32'
    if name not in _DET_DTYPES:
        raise ValueError("dtype should be 'float32' or 'float64' (or None: float64).")
    plan, n, shape = _jacobian_plan(displacement, X_shape, crop, axis, affine, rotate, zoom, batch)
    if any(int(d) == 1 for d in plan.deform_shape):
        # a deformed axis of length 1: no coordinate is defined there (deform_grid_coordinates gives NaN)
        return _fill(displacement, shape, float('nan'), name)
    torch = _torch()
    device = _device_for([displacement])
    with torch.cuda.device(device):
        stream = _stream(device)
        df = _prefiltered_grid(_to_device(displacement, device), batch, device, stream)
        det = torch.empty(shape, dtype=getattr(torch, name), device=device)
        if det.numel():
            _lib.deform_jacobian(shape[0] if batch else 1, *_sample(df, batch), plan.deform_shape, plan.output_offset,
                                 plan.inverse_affine, *_sample(det, batch), 0, stream)
        return _from_device(det, displacement)


def deform_grid_jacobian(displacement, X_shape, crop=None, axis=None, affine=None, rotate=None, zoom=None, dtype=None):
    """
    The Jacobian determinant of the coordinate map of :func:`deform_grid` at every output voxel: ``det[o] = det J(o)``
    for the ``J`` that ``deform_grid_coordinates(o, displacement, X_shape, ..., jacobian=True)`` returns at the integer
    crop-local position ``o``.  ``det <= 0`` somewhere means the field folds there; ``det`` is the local volume
    change of the map from the output to the source.  ``X_shape`` is the shape of the array ``deform_grid`` deforms;
    the other arguments are deform_grid's own, checked the same way.  1 to 3 deformed axes.

    The result has the shape of the deformed axes of what ``deform_grid`` returns for that call (crop applied), dtype
    float64 -- or float32 with ``dtype='float32'``: the arithmetic is fp64 and a float32 result is rounded once.  No
    positions are read and no coordinates formed: on the lattice the tap weights of an axis depend on that axis'
    index only, so the axes other than the last are contracted once per row.  A voxel's value depends on its
    position in the uncropped output and the call's arguments only: without affine / rotate / zoom a crop gives the
    bits of the whole lattice at those voxels.

    numpy in gives numpy out, otherwise a tensor on the displacement's device.  A deformed axis of length 1 gives
    NaN.  No autograd flows through this call itself: :func:`deform_grid_jacobian_gradient` is its adjoint and
    ``elasticdeform_amd.torch.deform_grid_jacobian`` the differentiable wrapper.
    """
    return _jacobian_run(displacement, X_shape, crop, axis, affine, rotate, zoom, dtype, False)


def deform_grid_jacobian_batch(displacements, X_shape, crop=None, axis=None, affine=None, rotate=None, zoom=None,
                               dtype=None):
    """:func:`deform_grid_jacobian` over a batch with one control grid per sample: ``displacements``
    ``(B, naxis, n_0, ...)``, ``X_shape`` the shape of ONE sample; everything else is shared.  The result is
    ``(B, ...)``.  One launch for the batch; sample b equals the single call, bit for bit."""
    return _jacobian_run(displacements, X_shape, crop, axis, affine, rotate, zoom, dtype, True)


def _jacobian_gradient(d_det, displacement, X_shape, crop, axis, affine, rotate, zoom, batch, want_disp=True,
                       want_map=True):
    """The adjoint of _jacobian_run: ONE library call for whatever is wanted.  Returns (plan, d displacement or None
    in the family of `d_det`, dK or None: a float64 tensor (naxis, naxis+1) -- (B, naxis, naxis+1) for a batch).
    Every argument check runs before the device or the library is touched."""
    plan, n, shape = _jacobian_plan(displacement, X_shape, crop, axis, affine, rotate, zoom, batch)
    if not _host.is_array(d_det):
        d_det = numpy.asarray(d_det)
    if _volume_dtype_name(d_det) not in _DET_DTYPES:
        raise ValueError("d_det should be float32 or float64, not %s." % _volume_dtype_name(d_det))
    if tuple(int(v) for v in d_det.shape) != shape:
        raise ValueError("d_det should have the shape of det, %s, but its shape is %s."
                         % (str(shape), str(tuple(d_det.shape))))
    if want_map and zoom is not None and float(zoom) == 0:
        raise ValueError("zoom=0 means 'no zoom' (as in the reference): it has no gradient")
    dk_shape = ((shape[0],) if batch else ()) + (n, n + 1)
    torch = _torch()
    if not isinstance(d_det, numpy.ndarray):
        d_det = d_det.detach()

    if any(int(d) == 1 for d in plan.deform_shape):
        # a deformed axis of length 1: det is NaN whatever the arguments, nothing depends on anything
        dk = None
        if want_map:
            dk = torch.zeros(dk_shape, dtype=torch.float64, device=d_det.device if torch.is_tensor(d_det) else 'cpu')
        return plan, _dgrad_zeros(displacement, d_det) if want_disp else None, dk

    device = _device_for([d_det, displacement])
    with torch.cuda.device(device):
        stream = _stream(device)
        gd = _to_device(d_det, device)
        dd = _to_device(displacement, device)
        df = _prefiltered_grid(dd, batch, device, stream)
        dp = torch.empty(tuple(int(v) for v in dd.shape), dtype=torch.float64, device=device) if want_disp else None
        dk = torch.empty(dk_shape, dtype=torch.float64, device=device) if want_map else None
        if want_disp or want_map:
            _lib.deform_jacobian_gradient(shape[0] if batch else 1, *_sample(gd, batch), *_sample(df, batch),
                                          plan.deform_shape, plan.output_offset, plan.inverse_affine,
                                          *_sample(dp, batch), *_sample(dk, batch), 0, stream)
        out = None
        if dp is not None:
            # dD = (order-3 mirror prefilter)^T dP in fp64, rounded once to the result's dtype
            dp = _filter_axes(dp, _grid_axes(dd, batch), 3, True, device, overwrite=True, stream=stream)
            out = _from_device(dp.to(_result_tensor_dtype(displacement)), d_det)
    return plan, out, dk


def deform_grid_jacobian_gradient(d_det, displacement, X_shape, crop=None, axis=None, affine=None, rotate=None,
                                  zoom=None):
    """
    Gradient through :func:`deform_grid_jacobian`: for ``L`` with ``d_det = dL / d det`` (the shape of ``det``,
    float32 / float64) returns ``JacobianGradient(displacement, affine, rotate, zoom, inverse_map)``:

    * ``displacement``: dL / d displacement (the order-3 prefilter of the grid included), as
      :func:`deform_grid_displacement_gradient` returns it;
    * ``affine`` / ``rotate`` / ``zoom`` / ``inverse_map``: as in :class:`AffineGradient` (``zoom=0`` raises).  The
      translation column of ``inverse_map`` is zero: det does not depend on it.

    With ``C(o)`` the cofactor matrix of ``J(o)`` (so that the derivative is right where ``det = 0`` too) this is
    ``dP[h, j] = sum_o d_det(o) sum_l C[h, l](o) d_l beta_j(o)`` and ``dK[h, l] = sum_o d_det(o) C[h, l](o)``, summed
    in fp64 as a chain of small contractions -- over x per row, over the rows, over the planes -- in an order that
    depends on the shapes only: no atomics, the same bits on every call.  A float32 ``d_det`` is widened at the load.
    numpy in gives numpy out, otherwise tensors on ``d_det``'s device.  A deformed axis of length 1 gives zeros.
    """
    plan, ddisp, dk = _jacobian_gradient(d_det, displacement, X_shape, crop, axis, affine, rotate, zoom, False)
    return JacobianGradient(ddisp, *_affine_result(dk, plan, affine, rotate, zoom, isinstance(ddisp, numpy.ndarray)))


def deform_grid_jacobian_gradient_batch(d_det, displacements, X_shape, crop=None, axis=None, affine=None, rotate=None,
                                        zoom=None):
    """:func:`deform_grid_jacobian_gradient` over a batch with one control grid per sample: ``d_det`` ``(B, ...)``,
    ``displacements`` ``(B, naxis, n_0, ...)``, ``X_shape`` the shape of ONE sample.  ``displacement`` is per sample,
    the same bits as the single call on that sample; the map's fields are the sum over the samples in sample order
    (:func:`deform_grid_affine_gradient_batch`).  One set of launches for the batch."""
    plan, ddisp, dk = _jacobian_gradient(d_det, displacements, X_shape, crop, axis, affine, rotate, zoom, True)
    return JacobianGradient(ddisp, *_affine_result_batch(dk, plan, affine, rotate, zoom,
                                                         isinstance(ddisp, numpy.ndarray)))


# ---- label-aware linear resampling of label maps (no counterpart in the reference) -------------------------------

_LABEL_RANGE = {'bool': (0, 1), 'uint8': (0, 2 ** 8 - 1), 'int8': (-2 ** 7, 2 ** 7 - 1), 'uint16': (0, 2 ** 16 - 1),
                'int16': (-2 ** 15, 2 ** 15 - 1), 'uint32': (0, 2 ** 32 - 1), 'int32': (-2 ** 31, 2 ** 31 - 1),
                'uint64': (0, 2 ** 64 - 1), 'int64': (-2 ** 63, 2 ** 63 - 1)}


def _label_cval(cval, name):
    """cval as a Python int: an integer value the label dtype can represent (and a float64 can carry to the library)"""
    try:
        value = int(cval)
        ok = value == cval and float(value) == value
    except (TypeError, ValueError, OverflowError):
        ok = False
    if ok:
        lo, hi = _LABEL_RANGE[name]
        ok = lo <= value <= hi
    if not ok:
        raise ValueError("cval should be an integer value that the label map's dtype (%s) can represent, "
                         "but %r given." % (name, cval))
    return value


def _labels_run(L, displacement, mode, cval, crop, axis, affine, rotate, zoom, return_weight, batch):
    """Both forms of deform_grid_labels.  Every argument check runs before the device is touched; offsets, the inverse
    map and the rotate / zoom centre are deform_grid's own for order 1 (the same Plan)."""
    Ls = [L] if batch else _host.normalize_inputs(L)
    plan = _plan_of(Ls, batch, displacement, 1, mode, cval, crop, axis, affine, rotate, zoom)
    shapes = [tuple(int(v) for v in x.shape[1 if batch else 0:]) for x in Ls]
    n = len(Ls)
    names = [_volume_dtype_name(x) for x in Ls]
    if any(name not in _LABEL_RANGE for name in names):
        raise RuntimeError('data type not supported')     # float, complex, 16-bit float: label maps are integer or bool
    cvals = [_label_cval(c, name) for c, name in zip(_host._per_input(cval, n, 'cval'), names)]
    if plan.naxis > 3:
        raise RuntimeError('deform_grid_labels takes 1 to 3 deformed axes')   # (the library's own limit)
    lead = (int(L.shape[0]),) if batch else ()
    out_shapes = [lead + tuple(int(v) for v in s) for s in plan.output_shapes]

    if _host.degenerate_axis(shapes, plan.axis):
        # a deformed axis of length 1: every voxel maps to the constant, as in deform_grid (_host.degenerate_axis)
        labels = [_fill(x, s, c) for x, s, c in zip(Ls, out_shapes, cvals)]
        weights = [_fill(x, s, 1.0, 'float32') for x, s in zip(Ls, out_shapes)]
    else:
        torch = _torch()
        device = _device_for(list(Ls) + [displacement])
        labels, weights = [], []
        with torch.cuda.device(device):
            stream = _stream(device)
            df = _prefiltered_grid(_to_device(displacement, device), batch, device, stream)
            for i, x in enumerate(Ls):
                xd = _to_device(x, device)
                out = torch.empty(out_shapes[i], dtype=xd.dtype, device=device)
                wt = torch.empty(out_shapes[i], dtype=torch.float32, device=device) if return_weight else None
                # one library call (one launch) per input
                _lib.deform_labels(lead[0] if batch else 1, *_sample(xd, batch), *_sample(df, batch),
                                   plan.output_offset, *_sample(out, batch), *_sample(wt, batch), plan.axis[i],
                                   int(plan.mode[i]), float(cvals[i]), plan.inverse_affine, 0, stream)
                labels.append(_from_device(out, x))
                weights.append(_from_device(wt, x) if wt is not None else None)
    return _list_or_one(labels, weights, return_weight, L)


def deform_grid_labels(L, displacement, mode='constant', cval=0, crop=None, axis=None, affine=None, rotate=None,
                       zoom=None, return_weight=False):
    """
    Label-aware linear resampling of a label map (a segmentation mask) under the deformation of :func:`deform_grid`:
    per output voxel, the ``2^naxis`` linear-interpolation weights are summed per distinct label among the
    ``2^naxis`` source voxels and the label with the largest sum is stored -- what deforming one float channel per
    class with ``order=1`` and taking the argmax computes, in one pass over the integer map and without the one-hot
    volumes.  No label number is ever interpolated: the result only holds values of ``L`` (and ``cval``), where
    ``deform_grid(L, order=1)`` puts label 5 halfway between labels 2 and 8, and its boundaries are smoother than
    those of ``order=0``.

    With the classes being the distinct values of ``L`` together with ``cval``, the score of class ``c`` is
    ``s_c = deform_grid((L == c).astype(float64), displacement, order=1, mode=mode, cval=1.0 if c == cval else 0.0,
    ...)`` and the result is the class with the largest score; **on a tie the numerically smallest label wins**.
    The result equals that definition bit for bit, ties included.  ``return_weight=True`` returns ``(labels, weight)``
    with the winning score rounded once to float32: in ``[2^-naxis, 1]``, a boundary-confidence map.

    ``L``: an integer or bool array, or a list of them (a list gives a list, of pairs with ``return_weight``; ``mode``,
    ``cval`` and ``axis`` may then be per-input lists as in deform_grid); 1 to 3 deformed axes.  ``cval`` must be an
    integer value the dtype can represent (ValueError otherwise); float, complex and 16-bit float inputs raise
    ``RuntimeError('data type not supported')``.  ``displacement``, ``mode``, ``crop``, ``axis``, ``affine``,
    ``rotate`` and ``zoom`` have deform_grid's meaning and checks.  A deformed axis of length 1 gives ``cval``
    everywhere with weight 1.0, as in deform_grid.  numpy in gives numpy out, tensors stay on their device.  No
    autograd flows through this call.
    """
    return _labels_run(L, displacement, mode, cval, crop, axis, affine, rotate, zoom, return_weight, False)


def deform_grid_labels_batch(L, displacements, mode='constant', cval=0, crop=None, axis=None, affine=None, rotate=None,
                             zoom=None, return_weight=False):
    """:func:`deform_grid_labels` over a batch with one control grid per sample (:func:`deform_grid_batch`): ``L``
    ``(B, ...)``, ``displacements`` ``(B, naxis, n_0, ...)``, ``axis`` counts the axes of ONE sample; everything else
    is shared.  One launch for the batch; sample b equals the single call on sample b, bit for bit."""
    return _labels_run(L, displacements, mode, cval, crop, axis, affine, rotate, zoom, return_weight, True)


# ---- an image carried back through the deformation (no counterpart in the reference) -----------------------------

def _inverse_shapes(X_shape, Ys, batch):
    """X_shape as one shape per input: a single shape serves every input, a list of shapes is per input"""
    if X_shape is None:
        raise ValueError("X_shape is required: the shape of the array deform_grid deforms.")
    per_input = isinstance(X_shape, list) and len(X_shape) > 0 and isinstance(X_shape[0], (tuple, list))
    if per_input and batch:
        raise ValueError("X_shape should be the shape of ONE sample.")
    shapes = [tuple(int(v) for v in s) for s in X_shape] if per_input else [tuple(int(v) for v in X_shape)] * len(Ys)
    assert len(shapes) == len(Ys), 'Number of X_shape parameters should be equal to number of inputs.'
    for s, y in zip(shapes, Ys):
        ndim = int(y.ndim) - (1 if batch else 0)
        if len(s) != ndim:
            raise ValueError("X_shape should have one extent per dimension of Y (%d), but %s given."
                             % (ndim, str(s)))
    return shapes


def _inverse_geometry(A, displacement, X_shape, order, mode, cval, crop, axis, affine, rotate, zoom, max_iter, tol, batch,
                      gradient):
    """The checks and the Plan every inverse call starts with, before the device is touched.  A: Y, or with `gradient`
    the cotangent dZ (it has the shape of X, so X_shape is not given).  Returns (the arrays of A, the shapes of X, the
    Plan of the forward call on arrays of those shapes, the shapes of Y that Plan gives, the leading batch extent as a
    tuple, the deformed extents of X, whether one of them is 1)."""
    _check_iteration(max_iter, tol)
    if batch and (not _host.is_array(A) or A.ndim < 2):
        raise Exception('%s should be an array with a leading batch axis.' % ('dZ' if gradient else 'Y'))
    As = [A] if batch else _host.normalize_inputs(A)
    a_shapes = [tuple(int(v) for v in a.shape[1 if batch else 0:]) for a in As]
    X_shapes = a_shapes if gradient else _inverse_shapes(X_shape, As, batch)
    stand_ins = _shape_only(X_shapes[0], A.shape[0]) if batch else [_host.ShapeOnly(s) for s in X_shapes]
    plan = _plan_of(stand_ins, batch, displacement, order, mode, cval, crop, axis, affine, rotate, zoom)
    y_shapes = [tuple(int(v) for v in s) for s in plan.output_shapes]
    if not gradient and y_shapes != a_shapes:
        raise ValueError("Y does not match X_shape and cropping. Expected shape of Y is %s, but %s given."
                         % (str(y_shapes), str(a_shapes)))
    if gradient:
        _check_float_volumes(As)                          # cotangent and accumulator share a float32 / float64 dtype
    elif any(name not in _lib.DTYPE_CODES or name in _lib.REDUCED_DTYPES for name in map(_volume_dtype_name, As)):
        raise RuntimeError('data type not supported')     # complex, 16-bit floats
    n = plan.naxis
    if n > 3:
        raise RuntimeError('deform_grid_inverse takes 1 to 3 deformed axes')   # (the library's own limit)
    lead = (int(A.shape[0]),) if batch else ()
    deformed = tuple(int(v) for v in plan.deform_shape)
    sampled = tuple(int(y_shapes[0][a]) for a in plan.axis[0])
    degenerate = any(v == 1 for v in deformed)
    if not degenerate and any(v < 2 for v in sampled):
        raise ValueError("deform_grid_inverse needs at least 2 elements along every deformed axis of Y, "
                         "but its deformed extents are %s." % str(sampled))
    return As, X_shapes, plan, y_shapes, lead, deformed, degenerate


def _inverse_host(A, displacement, X_shape, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom, max_iter,
                  tol, return_valid, batch, gradient):
    """The host path of deform_grid_inverse (A = Y) and of deform_grid_inverse_gradient (`gradient`: A = dZ, which has
    the shape of X, so X_shape is not given; the result has the shape of Y), single call and batch.  Every argument
    check runs before the device is touched; offsets, the inverse map K and the rotate / zoom centre are those of the
    forward call on an array of shape X_shape (the same Plan)."""
    As, X_shapes, plan, y_shapes, lead, deformed, degenerate = _inverse_geometry(
        A, displacement, X_shape, order, mode, cval, crop, axis, affine, rotate, zoom, max_iter, tol, batch, gradient)
    n = plan.naxis

    if degenerate:
        # a deformed axis of X of length 1: the forward call maps every voxel to the constant and no position is
        # defined (deform_points solves nothing there) -- cval everywhere, nothing valid, and nothing depends on Y
        if gradient:
            return _list_or_one([_fill(a, lead + s, 0.0) for a, s in zip(As, y_shapes)], None, False, A)
        Zs = [_constant_result(y, lead + s, c) for y, s, c in zip(As, X_shapes, plan.cval)]
        valids = [_fill(y, lead + deformed, 0, 'uint8') for y in As]
        return _list_or_one(Zs, valids, return_valid, A)

    K = plan.inverse_affine
    M = _forward_linear(K, n)
    torch = _torch()
    device = _device_for(list(As) + [displacement])
    results, valids = [], []
    with torch.cuda.device(device):
        stream = _stream(device)
        df = _prefiltered_grid(_to_device(displacement, device), batch, device, stream)
        for i, a in enumerate(As):
            ad = _to_device(a, device)
            o = int(plan.order[i])
            ax = plan.axis[i]
            # Y is prepared as deform_grid prepares its input: filtered along its deformed axes (deform_grid.py:155-164);
            # the gradient applies the transposed filter to its result
            filter_axes = ([d + 1 for d in ax] if batch else ax) if prefilter and o > 1 else []
            nb = lead[0] if batch else 1
            # one library call (one launch) per input: the solve is done again for each
            if gradient:
                acc = torch.zeros(lead + y_shapes[i], dtype=ad.dtype, device=device)
                _lib.deform_inverse_gradient(nb, *_sample(ad, batch), *_sample(df, batch), deformed,
                                             plan.output_offset, *_sample(acc, batch), ax, o, int(plan.mode[i]), K, M,
                                             int(max_iter), float(tol), 0, stream)
                acc = _filter_axes(acc, filter_axes, o, True, device, overwrite=True, stream=stream)
                results.append(_from_device(acc, a))
            else:
                yf = _filter_axes(ad, filter_axes, o, False, device, stream=stream)
                out = torch.empty(lead + X_shapes[i], dtype=ad.dtype, device=device)
                ok = torch.empty(lead + deformed, dtype=torch.uint8, device=device) if return_valid else None
                _lib.deform_inverse(nb, *_sample(yf, batch), *_sample(df, batch), deformed, plan.output_offset,
                                    *_sample(out, batch), *_sample(ok, batch), ax, o, int(plan.mode[i]),
                                    float(plan.cval[i]), K, M, int(max_iter), float(tol), 0, stream)
                results.append(_from_device(out, a))
                valids.append(_from_device(ok, a) if ok is not None else None)
    return _list_or_one(results, valids, return_valid and not gradient, A)


def _inverse_run(Y, displacement, X_shape, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom, max_iter, tol,
                 return_valid, batch, displacement_grad=False, affine_grad=False):
    """Both forms of deform_grid_inverse.  With grad mode on the call goes through an autograd Function of
    elasticdeform_amd.torch when a floating-point tensor Y requires grad, when `displacement_grad` is set and the
    displacement tensor requires grad, or when `affine_grad` is set and a tensor affine / rotate / zoom requires grad;
    the Function's forward comes back here with grad mode off: the plain path."""
    torch = sys.modules.get('torch')                      # (a tensor can only arrive with torch imported)
    if torch is not None and torch.is_grad_enabled():
        def needs(v):
            return torch.is_tensor(v) and v.is_floating_point() and v.requires_grad
        if (any(needs(y) for y in (Y if isinstance(Y, list) else [Y])) or (displacement_grad and needs(displacement))
                or (affine_grad and any(needs(v) for v in (affine, rotate, zoom)))):
            from . import torch as _autograd
            return _autograd._inverse_with_autograd(Y, displacement, X_shape, order, mode, cval, crop, prefilter, axis,
                                                    affine, rotate, zoom, max_iter, tol, return_valid, batch,
                                                    displacement_grad, affine_grad)
    return _inverse_host(Y, displacement, X_shape, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom,
                         max_iter, tol, return_valid, batch, False)


def deform_grid_inverse(Y, displacement, X_shape, order=3, mode='constant', cval=0.0, crop=None, prefilter=True,
                        axis=None, affine=None, rotate=None, zoom=None, max_iter=32, tol=1e-9, return_valid=False, *,
                        displacement_grad=False, affine_grad=False):
    """
    Resample an image back through a deformation: the image-side counterpart of :func:`deform_points`.  With
    ``Y = deform_grid(X, displacement, crop=crop, axis=axis, affine=affine, rotate=rotate, zoom=zoom)`` a pull warp,
    ``Y[o] = X(r(o))``, this call carries ``Y`` -- or anything that lives in its frame: a prediction made on the
    deformed image, the moving image of a fitted registration -- into the frame of ``X``.  ``X_shape`` is the shape of
    ``X``; the result ``Z`` has that shape and ``Y``'s dtype.  For every voxel ``p`` of ``X`` along the deformed axes:

    * ``q(p)`` solves ``r(q) = p`` exactly as :func:`deform_points` solves it (same start, damped Newton step, ``tol``
      and ``max_iter``); it is a real position in ``Y``;
    * ``Z[p] = Y(q(p))``, interpolated with the spline ``order``, boundary ``mode`` and ``cval`` the way ``deform_grid``
      interpolates its input at a source coordinate (orders 0-5, the five legacy modes; in fp64, stored with
      ``deform_grid``'s rounding rules for integer types).  With ``mode='constant'`` a position outside ``Y`` gives
      ``cval``;
    * where the iteration does not solve (``deform_points`` returns NaN there: a folding field, a singular Jacobian)
      ``Z = cval`` in every mode.

    ``return_valid=True`` returns ``(Z, valid)``: ``valid`` (uint8, the deformed extents of ``X``) is 1 exactly where
    ``q`` was solved and lies inside ``Y`` (``0 <= q_k <= O_k - 1``) -- where ``Z`` is interpolated from inside ``Y``
    and not extended by the boundary mode; average test-time-augmentation predictions over it.  The solve happens once
    per voxel: every channel (non-deformed position) reuses it.

    ``Y``: an array or a list of arrays (a list gives a list, of pairs with ``return_valid``; ``order``, ``mode``,
    ``cval`` and ``axis`` may then be per-input lists as in deform_grid, and ``X_shape`` a list of shapes); 1 to 3
    deformed axes; float32, float64, integer and bool arrays (16-bit floats raise
    ``RuntimeError('data type not supported')``).  ``prefilter=True`` filters ``Y`` along its deformed axes for
    ``order > 1``, as deform_grid prepares its input.  ``displacement``, ``crop``, ``axis``, ``affine``, ``rotate`` and
    ``zoom`` are the forward call's own, checked the same way; ``Y`` must have the shape that call returns.  A deformed
    axis of ``X`` of length 1 gives ``cval`` everywhere and nothing valid; every deformed axis of ``Y`` needs at least
    2 elements.  numpy in gives numpy out, tensors stay on their device.

    Autograd: with grad mode on, a floating-point tensor ``Y`` that requires grad gives a ``Z`` with a ``grad_fn``; its
    backward is :func:`deform_grid_inverse_gradient`, the exact adjoint in ``Y`` (float atomics: the last bits of
    ``Y.grad`` may differ between runs).  ``valid`` is not differentiable.  In a list, each ``Y`` that requires grad
    gets its gradient.  ``displacement_grad=True`` (keyword only, the switches of
    ``elasticdeform_amd.torch.deform_grid``): a displacement tensor that requires grad gets its gradient too
    (:func:`deform_grid_inverse_displacement_gradient`); ``affine_grad=True``: tensor ``affine`` / ``rotate`` /
    ``zoom`` that require grad get theirs (:func:`deform_grid_inverse_affine_gradient`); one library call per float
    input gives both, with reproducible bits.  With both switches off (the default) no gradient goes to them.  Every
    other call -- numpy arrays, integer tensors, tensors that do not require grad -- is untouched by this.
    """
    return _inverse_run(Y, displacement, X_shape, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom,
                        max_iter, tol, return_valid, False, displacement_grad, affine_grad)


def deform_grid_inverse_batch(Y, displacements, X_shape, order=3, mode='constant', cval=0.0, crop=None, prefilter=True,
                              axis=None, affine=None, rotate=None, zoom=None, max_iter=32, tol=1e-9,
                              return_valid=False, *, displacement_grad=False, affine_grad=False):
    """:func:`deform_grid_inverse` over a batch with one control grid per sample (:func:`deform_grid_batch`): ``Y``
    ``(B, ...)``, ``displacements`` ``(B, naxis, n_0, ...)``, ``X_shape`` the shape of ONE sample and ``axis`` counts
    the axes of one sample; everything else is shared.  One launch for the batch; sample b equals the single call on
    sample b, bit for bit (``Z`` and ``valid``).  ``displacement_grad`` / ``affine_grad`` as in
    :func:`deform_grid_inverse`; the parameters are shared, so their gradients are summed over the samples in sample
    order."""
    return _inverse_run(Y, displacements, X_shape, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom,
                        max_iter, tol, return_valid, True, displacement_grad, affine_grad)


def deform_grid_inverse_gradient(dZ, displacement, order=3, mode='constant', crop=None, prefilter=True, axis=None,
                                 affine=None, rotate=None, zoom=None, max_iter=32, tol=1e-9):
    """
    Gradient of :func:`deform_grid_inverse` with respect to ``Y``: for ``L`` with ``dZ = dL / dZ`` and
    ``Z = deform_grid_inverse(Y, displacement, X_shape, ...)``, returns ``dL / dY``.  ``dZ`` has the shape of ``X``
    (channels included; it takes the place of ``X_shape``), the result the shape of ``Y`` -- the shape the forward call
    returns for the crop -- and ``dZ``'s dtype.

    For fixed deformation arguments and ``cval = 0`` the call is linear in ``Y``: ``Z[p] = sum_j A[p, j] Yf[j]`` with
    ``Yf`` the prefiltered ``Y`` and the row ``A[p, :]`` the ``(order + 1)^naxis`` products of tap weights at ``q(p)``
    (taps that the mirror edge rule folds onto one cell add up).  The row is empty where ``p`` is not solved, and where
    ``mode='constant'`` and ``q(p)`` lies outside ``Y``.  The result is ``P^T A^T dZ``, ``P^T`` the transposed
    prefilter along the deformed axes (``order > 1`` and ``prefilter=True``): the exact adjoint, in the sense
    :func:`deform_grid_gradient` is for :func:`deform_grid`.  ``q(p)`` is solved again, exactly as the forward solves
    it (``max_iter``, ``tol``).  ``cval`` plays no part and ``valid`` is not differentiable.  The displacement and
    affine / rotate / zoom get their gradients from :func:`deform_grid_inverse_displacement_gradient` and
    :func:`deform_grid_inverse_affine_gradient`.

    ``dZ``: a float32 or float64 array, or a list of them (per-input ``order`` / ``mode`` / ``axis`` lists as in
    :func:`deform_grid_inverse`); everything else raises ``RuntimeError('data type not supported')``.  The products
    are formed in fp64 and added with float atomics in ``dZ``'s dtype: which cell receives what is fixed, but the
    order of the adds is not, so the last bits may differ between two calls, and between a batch sample and the
    single call (the caveat of ``set_gradient_accumulation('float')`` and of the float64 route of
    :func:`deform_grid_gradient`).  Sums of exactly representable terms -- order 0 with integer-valued ``dZ`` -- are
    exact and reproducible.  A deformed axis of ``X`` of length 1 gives zeros.  numpy in gives numpy out, tensors stay
    on their device.
    """
    return _inverse_host(dZ, displacement, None, order, mode, 0.0, crop, prefilter, axis, affine, rotate, zoom,
                         max_iter, tol, False, False, True)


def deform_grid_inverse_gradient_batch(dZ, displacements, order=3, mode='constant', crop=None, prefilter=True,
                                       axis=None, affine=None, rotate=None, zoom=None, max_iter=32, tol=1e-9):
    """:func:`deform_grid_inverse_gradient` over a batch with one control grid per sample
    (:func:`deform_grid_inverse_batch`): ``dZ`` ``(B, ...)``, ``displacements`` ``(B, naxis, n_0, ...)``, ``axis`` counts
    the axes of one sample; everything else is shared.  One launch for the batch; sample b equals the single call on
    sample b up to the order of the float adds."""
    return _inverse_host(dZ, displacements, None, order, mode, 0.0, crop, prefilter, axis, affine, rotate, zoom,
                         max_iter, tol, False, True, True)


# ---- the gradient of deform_grid_inverse with respect to the deformation -----------------------------------------

def _inverse_transform_gradient(Y, dZ, displacement, order, mode, crop, prefilter, axis, affine, rotate, zoom, max_iter,
                                tol, batch, want_disp=True, want_map=False):
    """The host path of the four deform_grid_inverse_*_gradient calls: ONE library call per input for whatever is
    wanted.  Returns (plan, d displacement or None, dK or None): the first in the family of dZ, dK a float64 tensor
    (naxis, naxis+1) -- (B, naxis, naxis+1) for a batch -- on the device.  dZ has the shape of X and takes the place of
    X_shape; the Plan, the offsets and the inverse map K are the forward call's own (_inverse_geometry), and Y must
    have the shape that call returns.  Every argument check runs before the device is touched."""
    dZs, _, plan, y_shapes, lead, deformed, degenerate = _inverse_geometry(
        dZ, displacement, None, order, mode, 0.0, crop, axis, affine, rotate, zoom, max_iter, tol, batch, True)
    if batch and (not _host.is_array(Y) or Y.ndim < 2):
        raise Exception('Y should be an array with a leading batch axis.')
    Ys = [Y] if batch else _host.normalize_inputs(Y)
    got = [tuple(int(v) for v in y.shape[1 if batch else 0:]) for y in Ys]
    if len(Ys) != len(dZs) or got != y_shapes or (batch and int(Y.shape[0]) != lead[0]):
        raise ValueError("Y does not match the shape of dZ and cropping. Expected shape of Y is %s, but %s given."
                         % (str(y_shapes), str(got)))
    _check_float_volumes(Ys)
    if want_map and zoom is not None and float(zoom) == 0:
        raise ValueError("zoom=0 means 'no zoom' (as in the reference): it has no gradient")
    n = plan.naxis
    dk_shape = lead + (n, n + 1)
    torch = _torch()
    # order 0 is piecewise constant in q: such an input adds nothing
    todo = [i for i in range(len(Ys)) if int(plan.order[i]) > 0]
    if degenerate or not todo:
        # (a deformed axis of X of length 1: no position is defined, nothing depends on the grid or the map)
        dk = None
        if want_map:
            dk = torch.zeros(dk_shape, dtype=torch.float64, device=dZs[0].device if torch.is_tensor(dZs[0]) else 'cpu')
        return plan, (_dgrad_zeros(displacement, dZs[0]) if want_disp else None), dk

    K = plan.inverse_affine
    M = _forward_linear(K, n)
    device = _device_for(list(dZs) + list(Ys) + [displacement])
    with torch.cuda.device(device):
        stream = _stream(device)
        dd = _to_device(displacement, device)
        df = _prefiltered_grid(dd, batch, device, stream)
        nb = lead[0] if batch else 1
        dp_sum = dk_sum = None
        for i in todo:
            yd, zd = _to_device(Ys[i], device), _to_device(dZs[i], device)
            if yd.dtype != zd.dtype:                      # (the arithmetic is fp64 whatever the dtype)
                yd, zd = yd.to(torch.float64), zd.to(torch.float64)
            o = int(plan.order[i])
            ax = plan.axis[i]
            # Y is prepared as the forward prepares it: filtered along its deformed axes
            filter_axes = ([d + 1 for d in ax] if batch else ax) if prefilter and o > 1 else []
            yf = _filter_axes(yd, filter_axes, o, False, device, stream=stream)
            dp = torch.empty(tuple(int(v) for v in dd.shape), dtype=torch.float64, device=device) if want_disp else None
            dk = torch.empty(dk_shape, dtype=torch.float64, device=device) if want_map else None
            _lib.deform_inverse_transform_gradient(nb, *_sample(yf, batch), *_sample(zd, batch), *_sample(df, batch),
                                                   deformed, plan.output_offset, *_sample(dp, batch),
                                                   *_sample(dk, batch), ax, o, int(plan.mode[i]), K, M, int(max_iter),
                                                   float(tol), 0, stream)
            if dp is not None:
                # dD = (order-3 mirror prefilter)^T dP in fp64; the inputs' results are added in input order
                dp = _filter_axes(dp, _grid_axes(dd, batch), 3, True, device, overwrite=True, stream=stream)
                dp_sum = dp if dp_sum is None else dp_sum + dp
            if dk is not None:
                dk_sum = dk if dk_sum is None else dk_sum + dk
        out = None
        if dp_sum is not None:
            out = _from_device(dp_sum.to(_result_tensor_dtype(displacement)), dZs[0])
    return plan, out, dk_sum


def deform_grid_inverse_displacement_gradient(Y, dZ, displacement, order=3, mode='constant', crop=None, prefilter=True,
                                              axis=None, affine=None, rotate=None, zoom=None, max_iter=32, tol=1e-9):
    """
    Gradient of :func:`deform_grid_inverse` with respect to the control-point ``displacement``: for ``L`` with
    ``dZ = dL / dZ`` and ``Z = deform_grid_inverse(Y, displacement, X_shape, ...)``, returns ``dL / d displacement``
    (the order-3 prefilter of the grid included).  This is what a loss taken in the source (fixed) frame needs: a
    registration similarity between ``deform_grid_inverse(moving, displacement, ...)`` and the fixed image, an
    inverse-consistency term, an augmentation judged after un-warping.

    ``Z[p] = S_Y(q(p))`` with ``r(q(p)) = p``.  The spatial derivative of the spline interpolant of ``Y`` at ``q``
    (through the boundary ``mode``; ``Y`` prefiltered as the forward prefilters it) gives ``g = dL / dq`` per voxel;
    the implicit function theorem at the solved ``q`` gives ``u = -J^-T g`` with ``J = dr / dq``, and
    ``dL / dP[h, j] = sum_p u_h(p) beta(q(p), j)`` for the prefiltered grid ``P`` -- the sums of
    :func:`deform_points_gradient`, with the positions and cotangents formed inside the kernel.  ``q(p)`` is solved
    again, exactly as the forward solves it (``max_iter``, ``tol``).

    ``Y`` and ``dZ``: float32 / float64 arrays or lists of them (``dZ[i]`` has the shape of ``X[i]``, channels included,
    and takes the place of ``X_shape``; ``Y[i]`` the shape the forward call returns for the crop; per-input ``order`` /
    ``mode`` / ``axis`` lists as in :func:`deform_grid_inverse`); everything else raises
    ``RuntimeError('data type not supported')``.  All arithmetic is fp64.  A voxel contributes nothing where it is not
    solved and where ``mode='constant'`` and ``q`` lies outside ``Y`` (``Z = cval`` there); where ``'nearest'`` clamps
    an axis that axis has slope 0; ``order=0`` is piecewise constant and gives zeros, as does a deformed axis of ``X``
    of length 1.  At order 1 the derivative at an integer ``q`` is the one-sided one of the window the forward picks;
    orders 2 and above are continuously differentiable.

    Returns an array of the displacement's shape, in its dtype when that is floating (float64 otherwise): numpy for a
    numpy ``dZ``, otherwise a tensor on ``dZ``'s device.  The sums over the voxels are accumulated in 64-bit integer
    fixed point: repeated calls return the same bits, and one non-finite ``dZ`` on a contributing voxel makes the
    result NaN.  With several inputs there is one library call per input, and the results are added in fp64 in input
    order.
    """
    return _inverse_transform_gradient(Y, dZ, displacement, order, mode, crop, prefilter, axis, affine, rotate, zoom,
                                       max_iter, tol, False, True, False)[1]


def deform_grid_inverse_displacement_gradient_batch(Y, dZ, displacements, order=3, mode='constant', crop=None,
                                                    prefilter=True, axis=None, affine=None, rotate=None, zoom=None,
                                                    max_iter=32, tol=1e-9):
    """:func:`deform_grid_inverse_displacement_gradient` over a batch with one control grid per sample
    (:func:`deform_grid_inverse_batch`): ``Y`` and ``dZ`` ``(B, ...)``, ``displacements`` ``(B, naxis, n_0, ...)``,
    ``axis`` counts the axes of one sample; everything else is shared.  Returns ``(B, naxis, n_0, ...)``; sample b is
    the same bits as the single call on sample b."""
    return _inverse_transform_gradient(Y, dZ, displacements, order, mode, crop, prefilter, axis, affine, rotate, zoom,
                                       max_iter, tol, True, True, False)[1]


def deform_grid_inverse_affine_gradient(Y, dZ, displacement, order=3, mode='constant', crop=None, prefilter=True,
                                        axis=None, affine=None, rotate=None, zoom=None, max_iter=32, tol=1e-9):
    """
    Gradient of :func:`deform_grid_inverse` with respect to the affine part of the deformation: ``L`` with
    ``dZ = dL / dZ`` differentiated with respect to ``affine``, ``rotate`` and ``zoom``.  Arguments, checks and
    arithmetic as for :func:`deform_grid_inverse_displacement_gradient`; with ``u`` as there,
    ``dL / dK[h, l] = sum_p u_h(p) q_l(p)`` and ``dL / dK[h, naxis] = sum_p u_h(p)`` for the inverse map ``K``.
    Returns ``AffineGradient(affine, rotate, zoom, inverse_map)`` as :func:`deform_grid_affine_gradient` does
    (``zoom=0`` raises ValueError): numpy (floats for rotate / zoom) for a numpy ``dZ``, otherwise float64 tensors on
    ``dZ``'s device.  Repeated calls return the same bits.
    """
    plan, _, dk = _inverse_transform_gradient(Y, dZ, displacement, order, mode, crop, prefilter, axis, affine, rotate,
                                              zoom, max_iter, tol, False, False, True)
    return _affine_result(dk, plan, affine, rotate, zoom, isinstance(_host.normalize_inputs(dZ)[0], numpy.ndarray))


def deform_grid_inverse_affine_gradient_batch(Y, dZ, displacements, order=3, mode='constant', crop=None, prefilter=True,
                                              axis=None, affine=None, rotate=None, zoom=None, max_iter=32, tol=1e-9):
    """:func:`deform_grid_inverse_affine_gradient` over a batch (:func:`deform_grid_inverse_batch`).  ``affine`` /
    ``rotate`` / ``zoom`` are shared by the batch, so the result is the SUM over the samples: every field is each
    sample's value (the single call on that sample, same bits) added in fp64 in sample order, b = 0, 1, ..., B-1."""
    plan, _, dk = _inverse_transform_gradient(Y, dZ, displacements, order, mode, crop, prefilter, axis, affine, rotate,
                                              zoom, max_iter, tol, True, False, True)
    return _affine_result_batch(dk, plan, affine, rotate, zoom, isinstance(dZ, numpy.ndarray))


# ---- the deformed image at real output positions (no counterpart in the reference) ---------------------------------

def _sample_shapes(X_shape, count):
    """X_shape as one shape per input: a single shape serves every input, a list of shapes is per input"""
    if X_shape is None:
        raise ValueError("X_shape is required: the shape of the array deform_grid deforms.")
    per_input = isinstance(X_shape, list) and len(X_shape) > 0 and isinstance(X_shape[0], (tuple, list))
    shapes = [tuple(int(v) for v in s) for s in X_shape] if per_input else [tuple(int(v) for v in X_shape)] * count
    assert len(shapes) == count, 'Number of X_shape parameters should be equal to number of inputs.'
    return shapes


def _sample_host(X, dV, positions, displacement, X_shape, order, mode, cval, crop, prefilter, axis, affine, rotate,
                 zoom, return_inside, batch, want):
    """The host path of deform_grid_sample (`want` 'value': X given), of deform_grid_sample_gradient ('input': dV and
    X_shape given, the result has the shape of X) and of deform_grid_sample_coordinate_gradient ('coordinate': X and dV
    given, the result is g = dL/dr summed over the inputs), single call and batch.  Every argument check runs before
    the device is touched; offsets, the inverse map K and the rotate / zoom centre are those of the image call on X
    (the same Plan), and `crop` only sets the offset and that centre, as in deform_grid_coordinates.  Returns
    (plan, result)."""
    lead_array = X if want != 'input' else dV
    if batch and (not _host.is_array(lead_array) or lead_array.ndim < 2):
        raise Exception('%s should be an array with a leading batch axis.' % ('X' if want != 'input' else 'dV'))
    Xs = None if want == 'input' else ([X] if batch else _host.normalize_inputs(X))
    dVs = None if want == 'value' else ([dV] if batch else _host.normalize_inputs(dV))
    count = len(Xs if Xs is not None else dVs)
    nb = int(lead_array.shape[0]) if batch else None
    if Xs is not None:
        X_shapes = [tuple(int(v) for v in x.shape[1 if batch else 0:]) for x in Xs]
    else:
        X_shapes = _sample_shapes(X_shape, count)
    pts = _as_points(positions)
    _check_batch_points(pts, batch)
    stand_ins = _shape_only(X_shapes[0], nb) if batch else [_host.ShapeOnly(s) for s in X_shapes]
    plan = _plan_of(stand_ins, batch, displacement, order, mode, cval, crop, axis, affine, rotate, zoom)
    n, lead = _points_of_plan(pts, plan)
    if batch and lead[0] != nb:
        raise ValueError("positions should have one set of points per sample (%d), but their shape is %s."
                         % (nb, str(tuple(pts.shape))))
    if n > 3:
        raise RuntimeError('deform_grid_sample takes 1 to 3 deformed axes')    # (the library's own limit)
    # the result of input i: its non-deformed axes in their order, then the leading dimensions of the positions
    steps = [tuple(v for d, v in enumerate(s) if d not in plan.axis[i]) for i, s in enumerate(X_shapes)]
    plead = lead[1:] if batch else lead
    v_shapes = [((nb,) if batch else ()) + st + plead for st in steps]
    if dVs is not None:
        if len(dVs) != count:
            raise ValueError("dV should have one array per input.")
        got = [tuple(int(v) for v in d.shape) for d in dVs]
        if got != v_shapes:
            raise ValueError("dV does not match X and the positions. Expected shape of dV is %s, but %s given."
                             % (str(v_shapes), str(got)))
        _check_float_volumes(dVs)
        if Xs is not None:
            _check_float_volumes(Xs)                          # (the derivative of an integer image's rounded value)
    elif any(name not in _lib.DTYPE_CODES or name in _lib.REDUCED_DTYPES for name in map(_volume_dtype_name, Xs)):
        raise RuntimeError('data type not supported')         # complex, 16-bit floats
    bl = (nb,) if batch else ()
    torch = _torch()

    if any(int(d) == 1 for d in plan.deform_shape):
        # a deformed axis of length 1: the image call maps every voxel to the constant and no coordinate is defined
        if want == 'value':
            Vs = [_constant_result(x, s, c) for x, s, c in zip(Xs, v_shapes, plan.cval)]
            ins = [_fill(pts, lead, False, 'bool')] * count
            return plan, _list_or_one(Vs, ins, return_inside, X)
        if want == 'input':
            return plan, _list_or_one([_fill(d, bl + s, 0.0) for d, s in zip(dVs, X_shapes)], None, False, dV)
        return plan, _fill(pts, lead + (n,), 0.0, 'float64')

    K = plan.inverse_affine
    deformed = tuple(int(v) for v in plan.deform_shape)
    device = _device_for([pts, displacement] + list(Xs if Xs is not None else dVs))
    results, insides, g_sum = [], [], None
    with torch.cuda.device(device):
        stream = _stream(device)
        pd = _to_device(pts, device)
        pd = pd if batch else pd.reshape(-1, n)
        npts = int(pd.shape[-2])
        df = _prefiltered_grid(_to_device(displacement, device), batch, device, stream)
        for i in range(count):
            o = int(plan.order[i])
            ax = plan.axis[i]
            filter_axes = ([d + 1 for d in ax] if batch else list(ax)) if prefilter and o > 1 else []
            point_axis = int(ax[0]) + (1 if batch else 0)     # where the library wants the points among V's dimensions
            flat = bl + steps[i] + (npts,)

            def lattice(t):
                return t.reshape(flat).movedim(-1, point_axis)
            xf = zd = None
            if Xs is not None:
                xd = _to_device(Xs[i], device)
            if dVs is not None:
                zd = _to_device(dVs[i], device)
            if want == 'coordinate' and xd.dtype != zd.dtype:  # (the arithmetic is fp64 whatever the dtype)
                xd, zd = xd.to(torch.float64), zd.to(torch.float64)
            if Xs is not None:
                # X is prepared as deform_grid prepares its input: filtered along its deformed axes
                xf = _filter_axes(xd, filter_axes, o, False, device, stream=stream)
            if want == 'value':
                out = torch.empty(flat, dtype=xd.dtype, device=device)
                ok = torch.empty(bl + (npts,), dtype=torch.uint8, device=device) if return_inside else None
                _lib.deform_sample(nb if batch else 1, *_sample(xf, batch), *_sample(pd, batch), *_sample(df, batch),
                                   deformed, plan.output_offset, *_sample(lattice(out), batch), *_sample(ok, batch),
                                   ax, o, int(plan.mode[i]), float(plan.cval[i]), K, 0, stream)
                results.append(_from_device(out.reshape(v_shapes[i]), Xs[i]))
                insides.append(_from_device(ok.reshape(lead).to(torch.bool), pts) if ok is not None else None)
            elif want == 'input':
                acc = torch.zeros(bl + X_shapes[i], dtype=zd.dtype, device=device)
                _lib.deform_sample_gradient(nb if batch else 1, None, 0, *_sample(lattice(zd), batch),
                                            *_sample(pd, batch), *_sample(df, batch), deformed, plan.output_offset,
                                            *_sample(acc, batch), None, 0, ax, o, int(plan.mode[i]), K, 0, stream)
                acc = _filter_axes(acc, filter_axes, o, True, device, overwrite=True, stream=stream)
                results.append(_from_device(acc, dVs[i]))
            elif o > 0:                                       # (order 0 is piecewise constant in r: it adds nothing)
                g = torch.empty(bl + (npts, n), dtype=torch.float64, device=device)
                _lib.deform_sample_gradient(nb if batch else 1, *_sample(xf, batch), *_sample(lattice(zd), batch),
                                            *_sample(pd, batch), *_sample(df, batch), deformed, plan.output_offset,
                                            None, 0, *_sample(g, batch), ax, o, int(plan.mode[i]), K, 0, stream)
                g_sum = g if g_sum is None else g_sum + g     # the inputs' rows are added in fp64 in input order
        if want == 'coordinate':
            if g_sum is None:
                g_sum = torch.zeros(bl + (npts, n), dtype=torch.float64, device=device)
            return plan, _from_device(g_sum.reshape(lead + (n,)), pts)
    if want == 'value':
        return plan, _list_or_one(results, insides, return_inside, X)
    return plan, _list_or_one(results, None, False, dV)


def _sample_run(X, positions, displacement, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom,
                return_inside, batch):
    return _sample_host(X, None, positions, displacement, None, order, mode, cval, crop, prefilter, axis, affine,
                        rotate, zoom, return_inside, batch, 'value')[1]


def deform_grid_sample(X, positions, displacement, order=3, mode='constant', cval=0.0, crop=None, prefilter=True,
                       axis=None, affine=None, rotate=None, zoom=None, return_inside=False):
    """
    The deformed image at arbitrary real output positions: ``V_i = X(r(q_i))``, the piece that joins the image side
    (:func:`deform_grid`) to the point side (:func:`deform_grid_coordinates`).  ``positions`` (shape ``(..., naxis)``)
    are real, crop-local output positions ``q`` of
    ``deform_grid(X, displacement, crop=crop, axis=axis, affine=affine, rotate=rotate, zoom=zoom)``:

    * ``r(q)`` is exactly what :func:`deform_grid_coordinates` returns (fp64, no boundary mode);
    * ``V = S_X(r(q))``, interpolated with the spline ``order``, boundary ``mode`` and ``cval`` the way ``deform_grid``
      interpolates its input at a source coordinate (orders 0-5, the five legacy modes; in fp64, stored with
      ``deform_grid``'s rounding rules for integer types).  With ``mode='constant'`` a coordinate outside ``X`` gives
      ``cval``;
    * a position that is not finite (or absurdly far out) gives ``cval`` in every mode.

    At integer ``q`` this is the voxel ``deform_grid`` computes, to the rounding of the coordinate (about 1e-10 voxels).
    A sampled registration metric, a read-out at landmarks or mesh vertices, sub-voxel patches and any sparse loss on a
    deformed image need this: a few thousand points cost a few thousand gathers, not a full-volume warp.

    The result has ``X``'s non-deformed axes in their order, followed by ``positions.shape[:-1]`` -- an input
    ``(C, z, y, x)`` with ``axis=(1, 2, 3)`` and ``(N, 3)`` positions gives ``(C, N)`` -- and ``X``'s dtype.
    ``return_inside=True`` returns ``(V, inside)``: ``inside`` (bool, ``positions.shape[:-1]``) is True exactly where
    the position is sane and ``0 <= r_k <= I_k - 1`` on every axis, where ``V`` is interpolated from inside ``X``;
    sampled metrics drop the other samples.

    ``X``: an array or a list of arrays that share the positions (a list gives a list, of pairs with
    ``return_inside``; ``order``, ``mode``, ``cval`` and ``axis`` may then be per-input lists as in
    :func:`deform_grid_inverse`: an image at order 3 and its label map at order 0); 1 to 3 deformed axes; float32,
    float64, integer and bool arrays (16-bit floats raise ``RuntimeError('data type not supported')``).
    ``prefilter=True`` filters ``X`` along its deformed axes for ``order > 1``, as deform_grid prepares its input.
    ``crop`` only sets the offset and the centre of ``rotate`` / ``zoom``, as in :func:`deform_grid_coordinates`.
    float32 / float64 positions; integer positions are taken as float64.  A deformed axis of length 1 gives ``cval``
    and nothing inside.  numpy in gives numpy out, tensors stay on their device.  One launch per input, one thread per
    point; the same bits for a repeated call, a slice or a permutation of the positions.  No autograd flows through
    this call itself: :func:`deform_grid_sample_gradient`, :func:`deform_grid_sample_coordinate_gradient` and
    :func:`deform_grid_sample_points_gradient` are its gradients and ``elasticdeform_amd.torch.deform_grid_sample``
    the differentiable wrapper.
    """
    return _sample_run(X, positions, displacement, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom,
                       return_inside, False)


def deform_grid_sample_batch(X, positions, displacements, order=3, mode='constant', cval=0.0, crop=None,
                             prefilter=True, axis=None, affine=None, rotate=None, zoom=None, return_inside=False):
    """:func:`deform_grid_sample` over a batch with one control grid per sample (:func:`deform_grid_batch`): ``X``
    ``(B, ...)``, ``positions`` ``(B, N, naxis)``, ``displacements`` ``(B, naxis, n_0, ...)``, ``axis`` counts the axes
    of one sample; everything else is shared.  The result is ``(B, non-deformed axes..., N)``.  One launch for the
    batch; sample b equals the single call on sample b, bit for bit."""
    return _sample_run(X, positions, displacements, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom,
                       return_inside, True)


def deform_grid_sample_gradient(dV, positions, displacement, X_shape, order=3, mode='constant', crop=None,
                                prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """
    Gradient of :func:`deform_grid_sample` with respect to ``X``: for ``L`` with ``dV = dL / dV`` (the shape of the
    forward's result, float32 / float64) returns ``dL / dX`` of shape ``X_shape`` in ``dV``'s dtype.  For fixed
    positions and deformation and ``cval = 0`` the call is linear in ``X``, ``V_i = sum_j A[i, j] Xf[j]`` with ``Xf``
    the prefiltered ``X`` and the row ``A[i, :]`` the ``(order + 1)^naxis`` tap-weight products at ``r(q_i)``; the row
    is empty where the position is not finite and where ``mode='constant'`` and ``r`` lies outside ``X``.  The result
    is ``P^T A^T dV`` (``P^T``: the transposed prefilter, ``order > 1`` and ``prefilter=True``): the exact adjoint.
    The products are formed in fp64 and added with float atomics in ``dV``'s dtype: which cell receives what is fixed,
    the order of the adds is not, so the last bits may differ between two calls (the caveat of
    :func:`deform_grid_inverse_gradient`); order 0 with integer-valued ``dV`` is exact and reproducible.  ``dV`` may be
    a list (``X_shape`` then one shape or a list of shapes; per-input ``order`` / ``mode`` / ``axis`` lists).
    """
    return _sample_host(None, dV, positions, displacement, X_shape, order, mode, 0.0, crop, prefilter, axis, affine,
                        rotate, zoom, False, False, 'input')[1]


def deform_grid_sample_gradient_batch(dV, positions, displacements, X_shape, order=3, mode='constant', crop=None,
                                      prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """:func:`deform_grid_sample_gradient` over a batch (:func:`deform_grid_sample_batch`): ``dV`` ``(B, ...)``,
    ``X_shape`` the shape of ONE sample; returns ``(B,) + X_shape``.  Sample b equals the single call on sample b up
    to the order of the float adds."""
    return _sample_host(None, dV, positions, displacements, X_shape, order, mode, 0.0, crop, prefilter, axis, affine,
                        rotate, zoom, False, True, 'input')[1]


def deform_grid_sample_coordinate_gradient(X, dV, positions, displacement, order=3, mode='constant', crop=None,
                                           prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """
    Gradient of :func:`deform_grid_sample` with respect to the coordinate the image is sampled at: ``g = dL / dr`` per
    point, with the shape of ``positions``, float64.  ``g_h = sum_step dV[step] m'_h sum_k C[k, step] w'_h prod_{e != h}
    w_e``: the spatial derivative of the spline interpolant of ``X`` at ``r(q)`` through the boundary ``mode`` (``X``
    prefiltered as the forward prefilters it).  Where ``'nearest'`` clamps an axis that component is 0; at order 1 the
    derivative at an integer coordinate is the one-sided one of the window the forward picks; ``order=0`` gives exact
    zeros, as do a position that is not finite and, with ``mode='constant'``, a coordinate outside ``X``.  ``X`` and
    ``dV``: float32 / float64 arrays or lists of them (the rows of a list's inputs are added in input order); integer
    images raise ``RuntimeError('data type not supported')``.  A row depends on its point alone: the same bits on
    every call, in a batch and after any permutation of the points.
    """
    return _sample_host(X, dV, positions, displacement, None, order, mode, 0.0, crop, prefilter, axis, affine, rotate,
                        zoom, False, False, 'coordinate')[1]


def deform_grid_sample_coordinate_gradient_batch(X, dV, positions, displacements, order=3, mode='constant', crop=None,
                                                 prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """:func:`deform_grid_sample_coordinate_gradient` over a batch (:func:`deform_grid_sample_batch`); returns
    ``(B, N, naxis)``, sample b the same bits as the single call on sample b."""
    return _sample_host(X, dV, positions, displacements, None, order, mode, 0.0, crop, prefilter, axis, affine, rotate,
                        zoom, False, True, 'coordinate')[1]


def _sample_points_gradient(X, dV, positions, displacement, order, mode, crop, prefilter, axis, affine, rotate, zoom,
                            batch, want_points=True, want_disp=True, want_map=True):
    """g = dL/dr, then the adjoint of the coordinate map with g as the cotangent (_points_gradient): the returns of
    _points_gradient.  The coordinate map is that of the first input (a list's inputs share their deformed extents)."""
    if want_map and zoom is not None and float(zoom) == 0:
        raise ValueError("zoom=0 means 'no zoom' (as in the reference): it has no gradient")
    plan, g = _sample_host(X, dV, positions, displacement, None, order, mode, 0.0, crop, prefilter, axis, affine,
                           rotate, zoom, False, batch, 'coordinate')
    first = X if batch else _host.normalize_inputs(X)[0]
    return _points_gradient(positions, g, displacement, tuple(int(v) for v in first.shape[1 if batch else 0:]), crop,
                            tuple(int(a) for a in plan.axis[0]), affine, rotate, zoom, False, batch,
                            want_points=want_points, want_disp=want_disp, want_map=want_map)


def deform_grid_sample_points_gradient(X, dV, positions, displacement, order=3, mode='constant', crop=None,
                                       prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """
    Gradient of :func:`deform_grid_sample` with respect to the positions and the deformation: returns
    ``PointsGradient(points, displacement, affine, rotate, zoom, inverse_map)`` as
    :func:`deform_grid_coordinates_gradient` does, for the cotangent ``g`` of
    :func:`deform_grid_sample_coordinate_gradient` -- ``points`` is ``J^T g`` per position, ``displacement`` the
    gradient of the control grid (its order-3 prefilter included), the other fields those of :class:`AffineGradient`.
    This is what a sampled registration metric differentiates.  The sums over the points are the 64-bit fixed-point
    sums of :func:`deform_grid_coordinates_gradient`: the same bits on every call and after any permutation of the
    points.
    """
    plan, rows, ddisp, dk = _sample_points_gradient(X, dV, positions, displacement, order, mode, crop, prefilter, axis,
                                                    affine, rotate, zoom, False)
    return _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, isinstance(rows, numpy.ndarray), False)


def deform_grid_sample_points_gradient_batch(X, dV, positions, displacements, order=3, mode='constant', crop=None,
                                             prefilter=True, axis=None, affine=None, rotate=None, zoom=None):
    """:func:`deform_grid_sample_points_gradient` over a batch (:func:`deform_grid_sample_batch`); shapes and the
    summed fields as for :func:`deform_grid_coordinates_gradient_batch`."""
    plan, rows, ddisp, dk = _sample_points_gradient(X, dV, positions, displacements, order, mode, crop, prefilter, axis,
                                                    affine, rotate, zoom, True)
    return _points_gradient_result(plan, rows, ddisp, dk, affine, rotate, zoom, isinstance(rows, numpy.ndarray), True)
