"""
The chain rule from the inverse map K -- the naxis x (naxis+1) matrix the kernels apply to the crop-local output
index, ``_host.Plan.inverse_affine`` -- back to the user's ``affine``, ``rotate`` and ``zoom``.

The forward keeps computing K with NumPy (``_host.inverse_of_affine``, ``_host.compose_rotation_zoom``).  This module
restates the same map in float64 torch ops and is used only for its derivatives: the Jacobian dK / d(parameters) is
formed once per plan on the host and applied to the library's dK on the result's device (no host round trip, so a
call on device tensors can be captured into a HIP graph once its plan has been seen).
"""
import math

import numpy
import torch


def _shift(c, sign):
    return torch.tensor([[1.0, 0.0, sign * c[0]], [0.0, 1.0, sign * c[1]], [0.0, 0.0, 1.0]], dtype=torch.float64)


class _AffineInverse(torch.autograd.Function):
    """[M | b] -> [M^-1 | -M^-1 b].  The value is LAPACK's through NumPy, as in _host.inverse_of_affine (torch's own
    inverse differs from it in the last bit); the derivative is the closed form dM^-1 = -M^-1 dM M^-1."""

    @staticmethod
    def forward(ctx, a):
        n = a.shape[0]
        an = a.detach().numpy()
        inv = numpy.zeros(an.shape, dtype='float64')
        inv[:, :-1] = numpy.linalg.inv(an[:, :-1])
        inv[:, -1] = -numpy.dot(inv[:, :-1], an[:, -1])
        out = torch.from_numpy(inv)
        ctx.save_for_backward(out)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        n = ctx.n
        minv_t = out[:, :n].t()
        t = out[:, n:]
        gm, gt = g[:, :n], g[:, n:]
        return torch.cat([-minv_t @ (gm @ minv_t + gt @ t.t()), -minv_t @ gt], dim=1)


class _RotationCosSin(torch.autograd.Function):
    """rotate (degrees) -> (cos, sin) of radians(-rotate), the values from NumPy as in _host.compose_rotation_zoom
    (torch's own cos / sin may differ from them in the last bit)."""

    @staticmethod
    def forward(ctx, rotate):
        th = numpy.radians(-float(rotate))
        ctx.cs = (float(numpy.cos(th)), float(numpy.sin(th)))
        return (torch.tensor(ctx.cs[0], dtype=torch.float64), torch.tensor(ctx.cs[1], dtype=torch.float64))

    @staticmethod
    def backward(ctx, gc, gs):
        c, s = ctx.cs
        # d th / d rotate = -pi / 180;  d cos = -sin d th,  d sin = cos d th
        return (gc * (-s) + gs * c) * (-math.pi / 180.0)


def inverse_map(affine, rotate, zoom, naxis, out_deform_shape):
    """K(affine, rotate, zoom) in float64 torch ops, the reference's factor order (deform_grid.py:382-438):
    ``[M^-1 | -M^-1 b]``, then T(c) Z R T(-c) from the left about the centre of the cropped output.  ``affine`` is an
    (naxis, naxis+1) or homogeneous 2-D (3, 3) tensor, or None (the identity); ``rotate`` / ``zoom`` are 0-d tensors or
    None.  Unlike the reference, the rotation factor is kept at ``rotate == 0``: it is the identity there (same K),
    and its derivative is not zero."""
    if affine is None:
        affine = torch.cat([torch.eye(naxis, dtype=torch.float64),
                            torch.zeros((naxis, 1), dtype=torch.float64)], dim=1)
    inv = _AffineInverse.apply(affine[:naxis, :])
    if rotate is None and zoom is None:
        return inv
    assert naxis == 2, 'Zoom and rotate is only implemented for 2D images.'
    centre = numpy.array(out_deform_shape) / 2 - 0.5
    m = _shift(centre, -1)
    if rotate is not None:
        c, s = _RotationCosSin.apply(rotate)
        zero, one = torch.zeros_like(c), torch.ones_like(c)
        m = torch.stack([torch.stack([c, -s, zero]), torch.stack([s, c, zero]), torch.stack([zero, zero, one])]) @ m
    if zoom is not None:
        scale = 1.0 / zoom
        zero, one = torch.zeros_like(scale), torch.ones_like(scale)
        m = torch.stack([torch.stack([scale, zero, zero]), torch.stack([zero, scale, zero]),
                         torch.stack([zero, zero, one])]) @ m
    m = _shift(centre, +1) @ m
    base = torch.cat([inv, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)], dim=0)
    return (m @ base)[:2, :]


def _as_f64(v):
    if v is None:
        return None
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    return torch.tensor(numpy.asarray(v, dtype=numpy.float64))


def jacobian(affine, rotate, zoom, naxis, out_deform_shape):
    """J[k, p] = d K.flat[k] / d theta_p at the given parameters, float64 numpy (naxis (naxis+1), P).  theta: the
    entries of ``affine`` in its own shape (the identity (naxis, naxis+1) when None), then ``rotate``, then ``zoom``
    (each only when given).  Returns (J, affine_shape)."""
    A = _as_f64(affine)
    if A is None:
        A = torch.cat([torch.eye(naxis, dtype=torch.float64), torch.zeros((naxis, 1), dtype=torch.float64)], dim=1)
    params = [A] + [p for p in (_as_f64(rotate), _as_f64(zoom)) if p is not None]
    has_rot, has_zoom = rotate is not None, zoom is not None

    def k_of(*p):
        it = iter(p[1:])
        r = next(it) if has_rot else None
        z = next(it) if has_zoom else None
        return inverse_map(p[0], r, z, naxis, out_deform_shape).reshape(-1)

    cols = torch.autograd.functional.jacobian(k_of, tuple(params))
    J = torch.cat([c.reshape(naxis * (naxis + 1), -1) for c in cols], dim=1)
    return J.numpy(), tuple(A.shape)
