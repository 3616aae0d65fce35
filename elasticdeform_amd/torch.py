"""
PyTorch wrapper: ``elasticdeform_amd.torch.deform_grid(X, displacement, *args, **kwargs)`` --
drop-in for ``elasticdeform.torch.deform_grid`` (/root/reference/elasticdeform/torch.py:33-66).

Same autograd contract as the reference's ``ElasticDeform`` Function (torch.py:5-29): gradients
flow to the inputs ``X`` only (the displacement gets none), a list / tuple of inputs gives a
tuple of outputs.  With ``displacement_grad=True`` (keyword-only, an extension) the displacement gets its gradient
too (``elasticdeform_amd.deform_grid_displacement_gradient``); with ``affine_grad=True`` ``affine``, ``rotate`` and
``zoom`` as well (``elasticdeform_amd.deform_grid_affine_gradient``).  The difference is the one this build exists for: the reference copies every
tensor to the host, runs one CPU thread and copies back (torch.py:13-16,25-29); here CUDA tensors
stay in HBM and forward / backward are HIP kernels enqueued on the current stream.
"""
from __future__ import absolute_import

import torch

# the package re-exports the functions, and `deform_grid` the function shadows the submodule
from . import deform_grid as _deform_grid_fn
from . import deform_grid_gradient as _deform_grid_gradient_fn
from . import deform_grid_batch as _deform_grid_batch_fn
from . import deform_grid_gradient_batch as _deform_grid_gradient_batch_fn
from . import _host
# mapping positions through the deformation: the batch forms are the package's own (tensors stay on their device, no
# autograd); deform_grid_coordinates / deform_points below are differentiable wrappers of the single calls
from . import deform_grid_coordinates_batch, deform_points_batch  # noqa: F401
from . import deform_grid_coordinates as _deform_grid_coordinates_fn
from . import deform_points as _deform_points_fn
from . import deform_grid_derivatives_batch, deform_grid_derivatives_gradient  # noqa: F401
from . import deform_grid_derivatives_gradient_batch, MapDerivatives  # noqa: F401
from . import deform_grid_derivatives as _deform_grid_derivatives_fn
# label-aware linear resampling of label maps (integer tensors stay on their device; no autograd)
from . import deform_grid_labels, deform_grid_labels_batch  # noqa: F401
# an image resampled back through the deformation and its adjoint: the package's own names (tensors stay on their
# device).  A Y that requires grad makes deform_grid_inverse itself go through DeformGridInverse below.
from . import deform_grid_inverse, deform_grid_inverse_batch  # noqa: F401
from . import deform_grid_inverse_gradient, deform_grid_inverse_gradient_batch  # noqa: F401
# ... and its gradients with respect to the deformation; displacement_grad / affine_grad of deform_grid_inverse carry
# them through DeformGridInverseExtended below
from . import deform_grid_inverse_displacement_gradient, deform_grid_inverse_displacement_gradient_batch  # noqa: F401
from . import deform_grid_inverse_affine_gradient, deform_grid_inverse_affine_gradient_batch  # noqa: F401
# det J on the voxel lattice: the batch forms and the explicit gradient are the package's own (no autograd);
# deform_grid_jacobian below is the differentiable wrapper of the single call
from . import deform_grid_jacobian_batch, deform_grid_jacobian_gradient_batch  # noqa: F401
from . import deform_grid_jacobian_gradient  # noqa: F401
from . import deform_grid_jacobian as _deform_grid_jacobian_fn
import importlib  # noqa: E402

_api = importlib.import_module("elasticdeform_amd.deform_grid")      # (the module, not the function)


class ElasticDeform(torch.autograd.Function):
    """forward: deform_grid; backward: deform_grid_gradient (torch.py:5-29)."""

    @staticmethod
    def forward(ctx, displacement, deform_args, deform_kwargs, *xs):
        ctx.save_for_backward(displacement)
        ctx.deform_args = deform_args
        ctx.deform_kwargs = deform_kwargs
        ctx.x_shapes = [tuple(x.shape) for x in xs]
        ys = _deform_grid_fn([x.detach() for x in xs], displacement.detach(),
                             *deform_args, **deform_kwargs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        displacement, = ctx.saved_tensors
        dxs = _deform_grid_gradient_fn([dy.detach() for dy in dys], displacement.detach(),
                                       *ctx.deform_args, X_shape=ctx.x_shapes,
                                       **ctx.deform_kwargs)
        return (None, None, None) + tuple(dxs)


_AFFINE_ARGS = ('affine', 'rotate', 'zoom')
_AFFINE_POS = 6            # deform_grid(X, displacement, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom)


def _host_value(v):
    """a parameter as the forward's NumPy algebra takes it (tensors leave the graph here)"""
    if torch.is_tensor(v):
        v = v.detach().cpu()
        return float(v) if v.dim() == 0 else v.double().numpy()
    return v


def _param_grads(needs, params, grads):
    """the affine / rotate / zoom gradients for the autograd inputs that need one, in their dtype, on their device"""
    out = []
    for need, p, g in zip(needs, params, grads):
        if need and g is not None:
            out.append(torch.as_tensor(g, dtype=torch.float64).to(device=p.device, dtype=p.dtype).reshape(p.shape))
        else:
            out.append(None)
    return out


def _extended_forward(ctx, displacement, affine, rotate, zoom, deform_args, deform_kwargs, disp_grad, xs):
    """what both extended Functions keep for backward: X as well as the displacement, and affine / rotate / zoom both
    as given (they receive the gradients) and as host values (the keywords of every library call)"""
    ctx.save_for_backward(displacement, *xs)
    ctx.params = (affine, rotate, zoom)
    ctx.host = {k: _host_value(v) for k, v in zip(_AFFINE_ARGS, ctx.params) if v is not None}
    ctx.deform_args = deform_args
    ctx.deform_kwargs = deform_kwargs
    ctx.disp_grad = disp_grad


def _extended_backward(ctx, batch, dys):
    """backward of both extended Functions (inputs: displacement, affine, rotate, zoom, three non-tensors, X...):
    dX from deform_grid_gradient(_batch) when an X needs it; the displacement's and the parameters' gradients from ONE
    library call (deform_grid.py _transform_gradient(_batch)) when either is needed."""
    displacement, *xs = (t.detach() for t in ctx.saved_tensors)
    dys = [dy.detach() for dy in dys]
    x, dy = (xs[0], dys[0]) if batch else (xs, dys)
    kw = dict(ctx.deform_kwargs, **ctx.host)
    dxs = [None] * len(xs)
    if any(ctx.needs_input_grad[7:]):
        gradient = _deform_grid_gradient_batch_fn if batch else _deform_grid_gradient_fn
        dxs = gradient(dy, displacement, *ctx.deform_args, X_shape=ctx.x_shape, **kw)
        dxs = [dxs] if batch else dxs
    want_disp = ctx.disp_grad and ctx.needs_input_grad[0]
    want_map = any(ctx.needs_input_grad[1:4])
    ddisp = None
    grads = [None, None, None]
    if want_disp or want_map:
        transform = _api._transform_gradient_batch if batch else _api._transform_gradient
        plan, *_, ddisp, dk = transform(x, dy, displacement, *ctx.deform_args,
                                        **dict(kw, want_disp=want_disp, want_map=want_map))
        if ddisp is not None:
            ddisp = ddisp.to(device=displacement.device, dtype=displacement.dtype)
        if dk is not None:
            result = _api._affine_result_batch if batch else _api._affine_result
            r = result(dk, plan, ctx.host.get('affine'), ctx.host.get('rotate'), ctx.host.get('zoom'), False)
            grads = _param_grads(ctx.needs_input_grad[1:4], ctx.params, r[:3])
    return (ddisp,) + tuple(grads) + (None, None, None) + tuple(dxs)


class ElasticDeformExtended(torch.autograd.Function):
    """ElasticDeform with a gradient for the displacement (displacement_grad=True) and / or for affine / rotate / zoom
    (affine_grad=True, where they arrive as inputs of their own instead of inside the arguments): the forward keeps X."""

    @staticmethod
    def forward(ctx, displacement, affine, rotate, zoom, deform_args, deform_kwargs, disp_grad, *xs):
        _extended_forward(ctx, displacement, affine, rotate, zoom, deform_args, deform_kwargs, disp_grad, xs)
        ctx.x_shape = [tuple(x.shape) for x in xs]
        ys = _deform_grid_fn([x.detach() for x in xs], displacement.detach(), *deform_args, **ctx.host,
                             **deform_kwargs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        return _extended_backward(ctx, False, dys)


def _split_affine(args, kwargs):
    """(args without affine / rotate / zoom, kwargs without them, [affine, rotate, zoom]) -- by keyword or position"""
    args = list(args)
    params = []
    for k, name in enumerate(_AFFINE_ARGS):
        pos = _AFFINE_POS + k
        if name in kwargs:
            params.append(kwargs.pop(name))
        elif pos < len(args):
            params.append(args[pos])
        else:
            params.append(None)
    return tuple(args[:_AFFINE_POS]), kwargs, params


def deform_grid(X, displacement, *args, displacement_grad=False, affine_grad=False, **kwargs):
    """
    Elastic deformation with a deformation grid, wrapped for PyTorch with a custom gradient.

    X : torch.Tensor or list / tuple of torch.Tensors; displacement : tensor or array of control
    point displacements; remaining arguments as for ``elasticdeform_amd.deform_grid``.
    Returns a tensor, or a tuple of tensors for a list / tuple input (torch.py:56-66).
    displacement_grad : keyword only.  False (the default, the reference's contract): gradients flow to X
    only.  True: the displacement gets its gradient as well (on its device, in its dtype).
    affine_grad : keyword only.  True: ``affine``, ``rotate`` and ``zoom`` (by keyword or position) may be tensors
    and get their gradients (in their dtype, on their device); with displacement_grad as well, one library call
    gives both.  False (the default): they are taken as values, as in the reference.
    """
    if not isinstance(X, (list, tuple)):
        X_list = [X]
    else:
        X_list = X
    displacement = torch.as_tensor(displacement)
    if affine_grad:
        args, kwargs, (affine, rotate, zoom) = _split_affine(args, dict(kwargs))
        y = ElasticDeformExtended.apply(displacement, affine, rotate, zoom, args, kwargs, bool(displacement_grad),
                                        *X_list)
    elif displacement_grad:
        # (affine / rotate / zoom stay inside the arguments, as values)
        y = ElasticDeformExtended.apply(displacement, None, None, None, args, kwargs, True, *X_list)
    else:
        y = ElasticDeform.apply(displacement, args, kwargs, *X_list)
    if isinstance(X, (list, tuple)):
        return y
    else:
        return y[0]


def random_displacement(naxis, points=3, sigma=25, batch=None, device=None, dtype=torch.float64,
                        generator=None):
    """
    Random control-point displacements drawn ON THE DEVICE: ``randn(naxis, *points) * sigma``, the
    distribution of ``deform_random_grid`` (/root/reference/elasticdeform/deform_grid.py:42-48),
    from torch's device generator (Philox) instead of NumPy's host RNG -- no host round trip and
    no H2D copy per sample.  With ``batch=B`` the result has a leading batch axis: one grid per
    sample of a batch.
    """
    if not isinstance(points, (list, tuple)):
        points = [points] * naxis
    assert len(points) == naxis
    shape = (naxis,) + tuple(int(p) for p in points)
    if batch is not None:
        shape = (int(batch),) + shape
    return torch.randn(shape, device=device, dtype=dtype, generator=generator) * sigma


def _random_grid_hint(sigma, points, deform_shape):
    """deform_grid.py's hint for a grid drawn here (a strong field by construction -> the z-walk route)"""
    if not isinstance(points, (list, tuple)):
        points = [points] * len(deform_shape)
    return _api._random_grid_hint(sigma, points, deform_shape)


def deform_random_grid(X, sigma=25, points=3, order=3, mode='constant', cval=0.0, crop=None,
                       prefilter=True, axis=None, affine=None, rotate=None, zoom=None,
                       generator=None):
    """
    ``elasticdeform.deform_random_grid`` (deform_grid.py:6-49) for tensors that live on the GPU:
    same arguments and meaning, but the random grid is drawn on the device of ``X``
    (:func:`random_displacement`) and the result stays there, with the autograd contract of
    :func:`deform_grid`.  ``generator``: an optional ``torch.Generator`` of that device.
    """
    Xs = list(X) if isinstance(X, (list, tuple)) else [X]
    _, deform_shape = _host.normalize_axis_list(axis, Xs)
    displacement = random_displacement(len(deform_shape), points, sigma, device=Xs[0].device,
                                       generator=generator)
    with _random_grid_hint(sigma, points, deform_shape):
        return deform_grid(X, displacement, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom)


class ElasticDeformBatch(torch.autograd.Function):
    """deform_grid_batch / deform_grid_gradient_batch as an autograd pair: gradients flow to X."""

    @staticmethod
    def forward(ctx, x, displacements, deform_kwargs):
        ctx.save_for_backward(displacements)
        ctx.deform_kwargs = deform_kwargs
        ctx.x_shape = tuple(x.shape[1:])
        return _deform_grid_batch_fn(x.detach(), displacements.detach(), **deform_kwargs)

    @staticmethod
    def backward(ctx, dy):
        displacements, = ctx.saved_tensors
        dx = _deform_grid_gradient_batch_fn(dy.detach(), displacements.detach(), X_shape=ctx.x_shape,
                                            **ctx.deform_kwargs)
        return dx, None, None


class ElasticDeformBatchExtended(torch.autograd.Function):
    """ElasticDeformBatch with a gradient for the displacements (displacement_grad=True) and / or for the shared
    affine / rotate / zoom (affine_grad=True) -- summed over the samples; same inputs as ElasticDeformExtended."""

    @staticmethod
    def forward(ctx, displacements, affine, rotate, zoom, deform_args, deform_kwargs, disp_grad, x):
        _extended_forward(ctx, displacements, affine, rotate, zoom, deform_args, deform_kwargs, disp_grad, (x,))
        ctx.x_shape = tuple(x.shape[1:])
        return _deform_grid_batch_fn(x.detach(), displacements.detach(), **ctx.host, **deform_kwargs)

    @staticmethod
    def backward(ctx, dy):
        return _extended_backward(ctx, True, (dy,))


def deform_grid_batch(X, displacements, *, displacement_grad=False, affine_grad=False, **kwargs):
    """
    Batched :func:`deform_grid` with one control grid per sample: ``X`` is ``(B, ...)``,
    ``displacements`` is ``(B, naxis, n_0, ...)`` (e.g. from :func:`random_displacement` with
    ``batch=B``); keyword arguments as for ``elasticdeform_amd.deform_grid_batch``.  Differentiable
    with respect to ``X``; with ``displacement_grad=True`` with respect to the displacements as well; with
    ``affine_grad=True`` with respect to the shared ``affine`` / ``rotate`` / ``zoom`` keywords (tensors allowed).
    """
    displacements = torch.as_tensor(displacements, device=X.device)
    if affine_grad:
        kwargs = dict(kwargs)
        affine, rotate, zoom = (kwargs.pop(k, None) for k in _AFFINE_ARGS)
        return ElasticDeformBatchExtended.apply(displacements, affine, rotate, zoom, (), kwargs,
                                                bool(displacement_grad), X)
    if displacement_grad:
        return ElasticDeformBatchExtended.apply(displacements, None, None, None, (), kwargs, True, X)
    return ElasticDeformBatch.apply(X, displacements, kwargs)


def deform_random_grid_batch(X, sigma=25, points=3, axis=None, generator=None, **kwargs):
    """Per-sample random deformation of a batch ``X`` of shape ``(B, ...)``: draws ``B`` grids on
    the device and applies one to each sample (the augmentation step of a data loader, without a
    host round trip).  ``axis`` counts the axes of one sample."""
    _, deform_shape = _host.normalize_axis_list(axis, [X[0]])
    disp = random_displacement(len(deform_shape), points, sigma, batch=X.shape[0], device=X.device,
                               generator=generator)
    with _random_grid_hint(sigma, points, deform_shape):
        return deform_grid_batch(X, disp, axis=axis, **kwargs)


# ---- points through the deformation, with autograd ------------------------------------------------------------------

def _points_backward(ctx, inverse, cotangent, positions, converged, derivatives=None):
    """backward of the point Functions (inputs: points, displacement, affine, rotate, zoom, two non-tensors): ONE
    library call (deform_grid.py _points_gradient) for whatever needs a gradient; `derivatives`: the cotangents of J
    and H (either may be None, and then `cotangent` too) for the adjoint of the derivatives call"""
    pts, displacement = (t.detach() for t in ctx.saved_tensors[:2])
    want_points = ctx.needs_input_grad[0]
    want_disp = ctx.disp_grad and ctx.needs_input_grad[1]
    want_map = any(ctx.needs_input_grad[2:5])
    dpts = ddisp = None
    grads = [None, None, None]
    if want_points or want_disp or want_map:
        host = ctx.host
        plan, dpts, ddisp, dk = _api._points_gradient(
            pts, cotangent.detach() if cotangent is not None else None, displacement, ctx.x_shape, ctx.kw.get('crop'),
            ctx.kw.get('axis'), host.get('affine'), host.get('rotate'), host.get('zoom'), inverse, False,
            want_points=want_points, want_disp=want_disp, want_map=want_map, positions=positions, converged=converged,
            derivatives=derivatives)
        if ddisp is not None:
            ddisp = ddisp.to(device=displacement.device, dtype=displacement.dtype)
        if dk is not None:
            r = _api._affine_result(dk, plan, host.get('affine'), host.get('rotate'), host.get('zoom'), False)
            grads = _param_grads(ctx.needs_input_grad[2:5], ctx.params, r[:3])
    return (dpts, ddisp) + tuple(grads) + (None, None)


def _points_forward(ctx, pts, displacement, affine, rotate, zoom, kw, disp_grad):
    ctx.params = (affine, rotate, zoom)
    ctx.host = {k: _host_value(v) for k, v in zip(_AFFINE_ARGS, ctx.params) if v is not None}
    ctx.kw = kw
    ctx.x_shape = kw['X_shape']
    ctx.disp_grad = disp_grad
    return dict(crop=kw.get('crop'), axis=kw.get('axis'), **ctx.host)


class DeformGridCoordinates(torch.autograd.Function):
    """forward: deform_grid_coordinates (with its Jacobian); backward: deform_grid_coordinates_gradient"""

    @staticmethod
    def forward(ctx, pts, displacement, affine, rotate, zoom, kw, disp_grad):
        call = _points_forward(ctx, pts, displacement, affine, rotate, zoom, kw, disp_grad)
        ctx.save_for_backward(pts, displacement)
        r, J = _deform_grid_coordinates_fn(pts.detach(), displacement.detach(), kw['X_shape'], jacobian=True, **call)
        ctx.mark_non_differentiable(J)
        return r, J

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dr, _dJ):
        return _points_backward(ctx, False, dr, None, None)


class DeformPoints(torch.autograd.Function):
    """forward: deform_points, solved in float64 (q and the mask are kept); backward: deform_points_gradient at the
    kept q -- it never solves again"""

    @staticmethod
    def forward(ctx, pts, displacement, affine, rotate, zoom, kw, disp_grad):
        call = _points_forward(ctx, pts, displacement, affine, rotate, zoom, kw, disp_grad)
        q, ok = _deform_points_fn(pts.detach().to(torch.float64), displacement.detach(), kw['X_shape'],
                                  max_iter=kw['max_iter'], tol=kw['tol'], return_converged=True, **call)
        ctx.save_for_backward(pts, displacement, q, ok)
        ctx.mark_non_differentiable(ok)
        return q.to(pts.dtype), ok

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dq, _dok):
        q, ok = ctx.saved_tensors[2:]
        return _points_backward(ctx, True, dq, q, ok)


def _points_need_autograd(points, displacement, params, displacement_grad, affine_grad):
    def needs(v):
        return torch.is_tensor(v) and v.requires_grad
    return (needs(points) or (displacement_grad and needs(displacement))
            or (affine_grad and any(needs(v) for v in params)))


def deform_grid_coordinates(positions, displacement, X_shape, crop=None, axis=None, affine=None, rotate=None,
                            zoom=None, jacobian=False, *, displacement_grad=False, affine_grad=False):
    """
    ``elasticdeform_amd.deform_grid_coordinates`` with autograd: the gradient flows to ``positions`` whenever they
    require it, to ``displacement`` with ``displacement_grad=True`` and to tensor ``affine`` / ``rotate`` / ``zoom``
    with ``affine_grad=True`` (keyword-only, the switches of :func:`deform_grid`); the backward is ONE call of
    ``elasticdeform_amd.deform_grid_coordinates_gradient``'s kernels.  The Jacobian is not differentiable.  With
    nothing requiring a gradient the call is the package's own: same bits, same types, numpy stays numpy.
    """
    params = (affine, rotate, zoom)
    if not _points_need_autograd(positions, displacement, params, displacement_grad, affine_grad):
        host = [_host_value(v) for v in params]
        return _deform_grid_coordinates_fn(positions, displacement, X_shape, crop, axis, *host, jacobian=jacobian)
    positions = torch.as_tensor(positions)
    displacement = torch.as_tensor(displacement)
    if not affine_grad:
        params = tuple(_host_value(v) for v in params)
    r, J = DeformGridCoordinates.apply(positions, displacement, *params, dict(X_shape=X_shape, crop=crop, axis=axis),
                                       bool(displacement_grad))
    return (r, J) if jacobian else r


def deform_points(points, displacement, X_shape, crop=None, axis=None, affine=None, rotate=None, zoom=None,
                  max_iter=32, tol=1e-9, return_converged=False, *, displacement_grad=False, affine_grad=False):
    """
    ``elasticdeform_amd.deform_points`` with autograd (implicit function theorem at the solved position): the
    gradient flows to ``points`` whenever they require it, to ``displacement`` with ``displacement_grad=True`` and to
    tensor ``affine`` / ``rotate`` / ``zoom`` with ``affine_grad=True``.  The forward keeps the solved positions and
    the mask; the backward never solves again, and points that were not solved receive and contribute nothing.  The
    mask is not differentiable.  With nothing requiring a gradient the call is the package's own.
    """
    params = (affine, rotate, zoom)
    if not _points_need_autograd(points, displacement, params, displacement_grad, affine_grad):
        host = [_host_value(v) for v in params]
        return _deform_points_fn(points, displacement, X_shape, crop, axis, *host, max_iter=max_iter, tol=tol,
                                 return_converged=return_converged)
    points = torch.as_tensor(points)
    displacement = torch.as_tensor(displacement)
    if not affine_grad:
        params = tuple(_host_value(v) for v in params)
    q, ok = DeformPoints.apply(points, displacement, *params,
                               dict(X_shape=X_shape, crop=crop, axis=axis, max_iter=max_iter, tol=tol),
                               bool(displacement_grad))
    return (q, ok) if return_converged else q


# ---- r, J and H at real positions, with autograd ----------------------------------------------------------------------

class DeformGridDerivatives(torch.autograd.Function):
    """forward: deform_grid_derivatives; backward: ONE call of deform_grid_derivatives_gradient's kernels for whichever
    of r, J and H received a cotangent"""

    @staticmethod
    def forward(ctx, pts, displacement, affine, rotate, zoom, kw, disp_grad):
        call = _points_forward(ctx, pts, displacement, affine, rotate, zoom, kw, disp_grad)
        ctx.save_for_backward(pts, displacement)
        ctx.set_materialize_grads(False)
        r, J, H = _deform_grid_derivatives_fn(pts.detach(), displacement.detach(), kw['X_shape'],
                                              hessian=kw['hessian'], **call)
        return r, J, H

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dr, dJ, dH=None):
        if dr is None and dJ is None and dH is None:
            return (None,) * 7
        return _points_backward(ctx, False, dr, None, None,
                                derivatives=tuple(d.detach() if d is not None else None for d in (dJ, dH)))


def deform_grid_derivatives(positions, displacement, X_shape, crop=None, axis=None, affine=None, rotate=None,
                            zoom=None, hessian=True, *, displacement_grad=False, affine_grad=False):
    """
    ``elasticdeform_amd.deform_grid_derivatives`` with autograd: ``MapDerivatives(r, J, H)`` at the positions, all
    three differentiable -- the gradient flows to ``positions`` whenever they require it, to ``displacement`` with
    ``displacement_grad=True`` and to tensor ``affine`` / ``rotate`` / ``zoom`` with ``affine_grad=True`` (keyword-only,
    the switches of :func:`deform_grid_coordinates`); the backward is ONE call of
    ``elasticdeform_amd.deform_grid_derivatives_gradient``'s kernels for whichever of the three received a cotangent,
    and is differentiable once.  A sampled folding penalty and bending energy::

        r, J, H = deform_grid_derivatives(q, D, fixed.shape, displacement_grad=True)
        reg = relu(-det(J)).mean() + mu * (H ** 2).sum((-1, -2, -3)).mean()

    With nothing requiring a gradient the call is the package's own: same bits, same types, numpy stays numpy.
    """
    params = (affine, rotate, zoom)
    if not _points_need_autograd(positions, displacement, params, displacement_grad, affine_grad):
        host = [_host_value(v) for v in params]
        return _deform_grid_derivatives_fn(positions, displacement, X_shape, crop, axis, *host, hessian=hessian)
    positions = torch.as_tensor(positions)
    displacement = torch.as_tensor(displacement)
    if not affine_grad:
        params = tuple(_host_value(v) for v in params)
    return MapDerivatives(*DeformGridDerivatives.apply(
        positions, displacement, *params, dict(X_shape=X_shape, crop=crop, axis=axis, hessian=bool(hessian)),
        bool(displacement_grad)))


# ---- det J on the voxel lattice, with autograd ------------------------------------------------------------------------

class DeformGridJacobian(torch.autograd.Function):
    """forward: deform_grid_jacobian; backward: ONE call of deform_grid_jacobian_gradient's kernels for whatever needs
    a gradient (inputs: displacement, affine, rotate, zoom, two non-tensors)"""

    @staticmethod
    def forward(ctx, displacement, affine, rotate, zoom, kw, disp_grad):
        call = _points_forward(ctx, None, displacement, affine, rotate, zoom, kw, disp_grad)
        ctx.save_for_backward(displacement)
        return _deform_grid_jacobian_fn(displacement.detach(), kw['X_shape'], dtype=kw['dtype'], **call)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_det):
        displacement = ctx.saved_tensors[0].detach()
        want_disp = ctx.disp_grad and ctx.needs_input_grad[0]
        want_map = any(ctx.needs_input_grad[1:4])
        ddisp = None
        grads = [None, None, None]
        if want_disp or want_map:
            host = ctx.host
            plan, ddisp, dk = _api._jacobian_gradient(
                d_det.detach(), displacement, ctx.x_shape, ctx.kw.get('crop'), ctx.kw.get('axis'), host.get('affine'),
                host.get('rotate'), host.get('zoom'), False, want_disp=want_disp, want_map=want_map)
            if ddisp is not None:
                ddisp = ddisp.to(device=displacement.device, dtype=displacement.dtype)
            if dk is not None:
                r = _api._affine_result(dk, plan, host.get('affine'), host.get('rotate'), host.get('zoom'), False)
                grads = _param_grads(ctx.needs_input_grad[1:4], ctx.params, r[:3])
        return (ddisp,) + tuple(grads) + (None, None)


def deform_grid_jacobian(displacement, X_shape, crop=None, axis=None, affine=None, rotate=None, zoom=None, dtype=None, *,
                         displacement_grad=False, affine_grad=False):
    """
    ``elasticdeform_amd.deform_grid_jacobian`` with autograd: det J of the coordinate map at every output voxel, the
    gradient flowing to ``displacement`` with ``displacement_grad=True`` and to tensor ``affine`` / ``rotate`` /
    ``zoom`` with ``affine_grad=True`` (keyword-only, the switches of :func:`deform_grid_coordinates`), in their dtype
    and on their device; the backward is ONE call of ``elasticdeform_amd.deform_grid_jacobian_gradient``'s kernels.
    This is what a folding penalty (``relu(-det)``), a ``log det`` term or a volume-preservation term differentiates.
    With nothing requiring a gradient the call is the package's own: no graph is built, numpy stays numpy.
    """
    params = (affine, rotate, zoom)
    if not _points_need_autograd(None, displacement, params, displacement_grad, affine_grad):
        host = [_host_value(v) for v in params]
        return _deform_grid_jacobian_fn(displacement, X_shape, crop, axis, *host, dtype=dtype)
    displacement = torch.as_tensor(displacement)
    if not affine_grad:
        params = tuple(_host_value(v) for v in params)
    return DeformGridJacobian.apply(displacement, *params, dict(X_shape=X_shape, crop=crop, axis=axis, dtype=dtype),
                                    bool(displacement_grad))


# ---- an image carried back through the deformation, with autograd -----------------------------------------------------

def _per_input_subset(value, idx, n):
    """a per-input list of `n` arguments cut down to the inputs `idx`; a shared value stays as it is"""
    return [value[i] for i in idx] if isinstance(value, list) and len(value) == n else value


class DeformGridInverse(torch.autograd.Function):
    """forward: deform_grid_inverse(_batch), the plain path (grad mode is off in here); backward:
    deform_grid_inverse_gradient(_batch) on the cotangents of the Z whose Y needs a gradient.  Inputs: the
    displacement, the call's keywords, the batch flag, whether Y came as a list, then every Y; outputs: every Z, then
    every valid."""

    @staticmethod
    def forward(ctx, displacement, kw, batch, as_list, *ys):
        ctx.displacement = displacement.detach() if torch.is_tensor(displacement) else displacement
        ctx.kw, ctx.batch, ctx.n = kw, batch, len(ys)
        res = _api._inverse_run(list(ys) if as_list else ys[0], ctx.displacement, batch=batch, **kw)
        res = res if as_list else [res]
        zs, valids = (zip(*res) if kw['return_valid'] else (res, ()))
        needs = ctx.needs_input_grad[4:]
        ctx.mark_non_differentiable(*[t for t in valids if torch.is_tensor(t)],
                                    *[z for z, need in zip(zs, needs) if torch.is_tensor(z) and not need])
        return tuple(zs) + tuple(valids)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *douts):
        n, kw = ctx.n, ctx.kw
        idx = [i for i in range(n) if ctx.needs_input_grad[4 + i]]
        grads = [None] * n
        if idx:
            call = dict(crop=kw['crop'], prefilter=kw['prefilter'], affine=kw['affine'], rotate=kw['rotate'],
                        zoom=kw['zoom'], max_iter=kw['max_iter'], tol=kw['tol'])
            if ctx.batch:
                grads[0] = deform_grid_inverse_gradient_batch(douts[0].detach(), ctx.displacement, order=kw['order'],
                                                              mode=kw['mode'], axis=kw['axis'], **call)
            else:
                per_input = {k: _per_input_subset(kw[k], idx, n) for k in ('order', 'mode', 'axis')}
                for i, g in zip(idx, deform_grid_inverse_gradient([douts[i].detach() for i in idx], ctx.displacement,
                                                                  **per_input, **call)):
                    grads[i] = g
        return (None, None, None, None) + tuple(grads)


class DeformGridInverseExtended(torch.autograd.Function):
    """DeformGridInverse with a gradient for the displacement (displacement_grad=True) and / or for affine / rotate /
    zoom (affine_grad=True, where they arrive as inputs of their own instead of inside the keywords), modelled on
    ElasticDeformExtended: the forward keeps every Y.  Inputs: the displacement, affine, rotate, zoom, the call's other
    keywords, the batch flag, whether Y came as a list, displacement_grad, then every Y; outputs: every Z, then every
    valid.  backward: deform_grid_inverse_gradient(_batch) for the Y that need a gradient, and ONE call of
    deform_grid.py _inverse_transform_gradient for the displacement's and the parameters' gradients."""

    @staticmethod
    def forward(ctx, displacement, affine, rotate, zoom, kw, batch, as_list, disp_grad, *ys):
        ctx.params = (affine, rotate, zoom)
        ctx.host = {k: _host_value(v) for k, v in zip(_AFFINE_ARGS, ctx.params)}
        ctx.kw, ctx.batch, ctx.n, ctx.disp_grad = kw, batch, len(ys), disp_grad
        ctx.save_for_backward(displacement, *ys)
        res = _api._inverse_run([y.detach() for y in ys] if as_list else ys[0].detach(), displacement.detach(),
                                batch=batch, **kw, **ctx.host)
        res = res if as_list else [res]
        zs, valids = (zip(*res) if kw['return_valid'] else (res, ()))
        ctx.mark_non_differentiable(*valids, *[z for z in zs if not z.is_floating_point()])
        return tuple(zs) + tuple(valids)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *douts):
        n, kw, host = ctx.n, ctx.kw, ctx.host
        displacement, *ys = (t.detach() for t in ctx.saved_tensors)
        call = dict(crop=kw['crop'], prefilter=kw['prefilter'], max_iter=kw['max_iter'], tol=kw['tol'], **host)

        def subset(idx):
            return {k: _per_input_subset(kw[k], idx, n) for k in ('order', 'mode', 'axis')}
        grads = [None] * n
        idx = [i for i in range(n) if ctx.needs_input_grad[8 + i]]
        if idx:
            if ctx.batch:
                grads[0] = deform_grid_inverse_gradient_batch(douts[0].detach(), displacement, **subset(idx), **call)
            else:
                for i, g in zip(idx, deform_grid_inverse_gradient([douts[i].detach() for i in idx], displacement,
                                                                  **subset(idx), **call)):
                    grads[i] = g
        want_disp = ctx.disp_grad and ctx.needs_input_grad[0]
        want_map = any(ctx.needs_input_grad[1:4])
        ddisp = None
        pgrads = [None, None, None]
        idx = [i for i in range(n) if ys[i].is_floating_point()]
        if (want_disp or want_map) and idx:
            per = subset(idx)
            plan, ddisp, dk = _api._inverse_transform_gradient(
                ys[0] if ctx.batch else [ys[i] for i in idx], douts[0].detach() if ctx.batch else
                [douts[i].detach() for i in idx], displacement, per['order'], per['mode'], kw['crop'], kw['prefilter'],
                per['axis'], host['affine'], host['rotate'], host['zoom'], kw['max_iter'], kw['tol'], ctx.batch,
                want_disp, want_map)
            if ddisp is not None:
                ddisp = ddisp.to(device=displacement.device, dtype=displacement.dtype)
            if dk is not None:
                result = _api._affine_result_batch if ctx.batch else _api._affine_result
                r = result(dk, plan, host['affine'], host['rotate'], host['zoom'], False)
                pgrads = _param_grads(ctx.needs_input_grad[1:4], ctx.params, r[:3])
        return (ddisp,) + tuple(pgrads) + (None, None, None, None) + tuple(grads)


def _inverse_with_autograd(Y, displacement, X_shape, order, mode, cval, crop, prefilter, axis, affine, rotate, zoom,
                           max_iter, tol, return_valid, batch, displacement_grad=False, affine_grad=False):
    """deform_grid_inverse(_batch) through DeformGridInverse -- through DeformGridInverseExtended when the displacement
    or affine / rotate / zoom get a gradient -- (elasticdeform_amd.deform_grid._inverse_run sends the calls that need a
    gradient here); results in the plain call's form"""
    def needs(v):
        return torch.is_tensor(v) and v.requires_grad
    as_list = isinstance(Y, list)
    ys = Y if as_list else [Y]
    kw = dict(X_shape=X_shape, order=order, mode=mode, cval=cval, crop=crop, prefilter=prefilter, axis=axis,
              max_iter=max_iter, tol=tol, return_valid=return_valid)
    params = (affine, rotate, zoom)
    want_disp = bool(displacement_grad) and needs(displacement)
    want_map = bool(affine_grad) and any(needs(v) for v in params)
    if want_disp or want_map:
        if not want_map:
            params = tuple(_host_value(v) for v in params)
        ys = [torch.as_tensor(y) for y in ys]
        outs = DeformGridInverseExtended.apply(torch.as_tensor(displacement), *params, kw, batch, as_list, want_disp,
                                               *ys)
    else:
        outs = DeformGridInverse.apply(displacement, dict(kw, affine=affine, rotate=rotate, zoom=zoom), batch, as_list,
                                       *ys)
    res = list(zip(outs[:len(ys)], outs[len(ys):])) if return_valid else list(outs)
    return res if as_list else res[0]


# ---- the deformed image at real output positions, with autograd ------------------------------------------------------

from . import deform_grid_sample_batch, deform_grid_sample_gradient_batch  # noqa: F401,E402
from . import deform_grid_sample_coordinate_gradient_batch, deform_grid_sample_points_gradient_batch  # noqa: F401,E402
from . import deform_grid_sample_coordinate_gradient, deform_grid_sample_points_gradient  # noqa: F401,E402
from . import deform_grid_sample_gradient  # noqa: F401,E402
from . import deform_grid_sample as _deform_grid_sample_fn  # noqa: E402


class DeformGridSample(torch.autograd.Function):
    """forward: deform_grid_sample (with its inside mask); backward: deform_grid_sample_gradient for X, and g = dL/dr
    followed by ONE call of deform_grid_coordinates_gradient's kernels for the positions, the displacement and the
    parameters (inputs: X, positions, displacement, affine, rotate, zoom, two non-tensors)"""

    @staticmethod
    def forward(ctx, x, pts, displacement, affine, rotate, zoom, kw, disp_grad):
        call = _points_forward(ctx, pts, displacement, affine, rotate, zoom, kw, disp_grad)
        ctx.save_for_backward(x, pts, displacement)
        ctx.call = dict(call, order=kw['order'], mode=kw['mode'], prefilter=kw['prefilter'])
        v, inside = _deform_grid_sample_fn(x.detach(), pts.detach(), displacement.detach(), cval=kw['cval'],
                                           return_inside=True, **ctx.call)
        ctx.mark_non_differentiable(inside)
        return v, inside

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dv, _dinside):
        x, pts, displacement = (t.detach() for t in ctx.saved_tensors)
        dv = dv.detach()
        dx = dpts = ddisp = None
        grads = [None, None, None]
        if ctx.needs_input_grad[0]:
            dx = deform_grid_sample_gradient(dv, pts, displacement, tuple(x.shape), **ctx.call)
        want_points = ctx.needs_input_grad[1]
        want_disp = ctx.disp_grad and ctx.needs_input_grad[2]
        want_map = any(ctx.needs_input_grad[3:6])
        if want_points or want_disp or want_map:
            host = ctx.host
            c = ctx.call
            plan, dpts, ddisp, dk = _api._sample_points_gradient(
                x, dv, pts, displacement, c['order'], c['mode'], c['crop'], c['prefilter'], c['axis'],
                host.get('affine'), host.get('rotate'), host.get('zoom'), False, want_points=want_points,
                want_disp=want_disp, want_map=want_map)
            if ddisp is not None:
                ddisp = ddisp.to(device=displacement.device, dtype=displacement.dtype)
            if dk is not None:
                r = _api._affine_result(dk, plan, host.get('affine'), host.get('rotate'), host.get('zoom'), False)
                grads = _param_grads(ctx.needs_input_grad[3:6], ctx.params, r[:3])
        return (dx, dpts, ddisp) + tuple(grads) + (None, None)


def deform_grid_sample(X, positions, displacement, order=3, mode='constant', cval=0.0, crop=None, prefilter=True,
                       axis=None, affine=None, rotate=None, zoom=None, return_inside=False, *,
                       displacement_grad=False, affine_grad=False):
    """
    ``elasticdeform_amd.deform_grid_sample`` with autograd: the gradient flows to ``X`` (a floating-point tensor) and
    to ``positions`` whenever they require it, to ``displacement`` with ``displacement_grad=True`` and to tensor
    ``affine`` / ``rotate`` / ``zoom`` with ``affine_grad=True`` (keyword-only, the switches of
    :func:`deform_grid_coordinates`).  The backward is ``deform_grid_sample_gradient`` for ``X`` (float atomics: the
    last bits of ``X.grad`` may differ between runs) and ``deform_grid_sample_points_gradient`` for everything else
    (reproducible bits).  ``inside`` is not differentiable.  A list of inputs gives a list; each input's gradients are
    added by autograd.  With nothing requiring a gradient the call is the package's own: no graph is built, numpy
    stays numpy.
    """
    params = (affine, rotate, zoom)
    xs = X if isinstance(X, list) else [X]

    def needs(v):
        return torch.is_tensor(v) and v.is_floating_point() and v.requires_grad
    if not torch.is_grad_enabled() or not (any(needs(x) for x in xs) or _points_need_autograd(
            positions, displacement, params, displacement_grad, affine_grad)):
        host = [_host_value(v) for v in params]
        return _deform_grid_sample_fn(X, positions, displacement, order, mode, cval, crop, prefilter, axis, *host,
                                      return_inside=return_inside)
    positions = torch.as_tensor(positions)
    displacement = torch.as_tensor(displacement)
    if not affine_grad:
        params = tuple(_host_value(v) for v in params)
    n = len(xs)
    out = []
    for i, x in enumerate(xs):
        def one(v):
            return v[i] if isinstance(v, list) and len(v) == n else v
        x = torch.as_tensor(x)
        kw = dict(X_shape=tuple(x.shape), order=one(order), mode=one(mode), cval=one(cval), crop=crop,
                  prefilter=prefilter, axis=one(axis) if isinstance(axis, list) and axis and
                  isinstance(axis[0], (list, tuple)) else axis)
        v, inside = DeformGridSample.apply(x, positions, displacement, *params, kw, bool(displacement_grad))
        out.append((v, inside) if return_inside else v)
    return out if isinstance(X, list) else out[0]
