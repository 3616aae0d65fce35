"""
elasticdeform_amd -- MI355X-native elastic grid deformation.

Drop-in for the hot path of gvtulder/elasticdeform: ``deform_random_grid``, ``deform_grid`` and
``deform_grid_gradient`` (reference: elasticdeform/__init__.py:1) with the same signatures, backed
by hand-written HIP kernels for gfx950 behind the C ABI in include/edhip.h.
``elasticdeform_amd.torch`` is the on-device PyTorch autograd wrapper (reference:
elasticdeform/torch.py).

    import elasticdeform_amd as elasticdeform
    Y = elasticdeform.deform_random_grid(X, sigma=25, points=3)

As in the reference, the function ``deform_grid`` shadows the submodule of the same name.
``deform_grid_batch`` / ``deform_grid_gradient_batch`` (no counterpart in the reference) take a
batch of samples with one control grid each.
``deform_grid_displacement_gradient`` / ``deform_grid_displacement_gradient_batch`` (no counterpart in the
reference either) differentiate with respect to the control-point displacement,
``deform_grid_affine_gradient`` / ``deform_grid_affine_gradient_batch`` with respect to affine, rotate and zoom.
``deform_grid_coordinates`` / ``deform_points`` (and their ``_batch`` forms) map positions through the deformation:
the coordinate map of ``deform_grid`` at real positions with its Jacobian, and where source points land in the output.
``deform_grid_coordinates_gradient`` / ``deform_points_gradient`` (and their ``_batch`` forms) are their adjoints: the
gradient of a loss on mapped points with respect to the points, the displacement and affine / rotate / zoom.
``deform_grid_labels`` / ``deform_grid_labels_batch`` resample label maps with linear weights and a per-label vote:
the argmax of the order-1 deformed one-hot channels without the one-hot volumes.
``deform_grid_inverse`` / ``deform_grid_inverse_batch`` resample an image back through the deformation, from the
deformed frame into the source frame: the image-side counterpart of ``deform_points``.
``deform_grid_inverse_gradient`` / ``deform_grid_inverse_gradient_batch`` are their adjoints with respect to the image;
a tensor that requires grad carries autograd through ``deform_grid_inverse``.
``deform_grid_inverse_displacement_gradient`` / ``deform_grid_inverse_affine_gradient`` (and their ``_batch`` forms)
differentiate ``deform_grid_inverse`` with respect to the control-point displacement and to affine, rotate and zoom:
what a loss taken in the source (fixed) frame needs; ``displacement_grad=True`` / ``affine_grad=True`` carry them through
autograd.
``deform_grid_jacobian`` / ``deform_grid_jacobian_batch`` give det J of the coordinate map at every output voxel (the
folding check of a fitted field, without a coordinate volume), ``deform_grid_jacobian_gradient`` /
``deform_grid_jacobian_gradient_batch`` its adjoint with respect to the displacement and to affine, rotate and zoom:
what a folding penalty, a log det or a volume-preservation term differentiates.
``deform_grid_sample`` / ``deform_grid_sample_batch`` give the deformed image at arbitrary real output positions,
``V_i = X(r(q_i))``, without deforming the volume: what a sampled registration metric, a read-out at landmarks or mesh
vertices and any sparse loss on a deformed image need.  ``deform_grid_sample_gradient`` (the adjoint in the image),
``deform_grid_sample_coordinate_gradient`` (``dL/dr`` per point) and ``deform_grid_sample_points_gradient`` (the
positions, the displacement and affine / rotate / zoom), with their ``_batch`` forms, are its gradients;
``elasticdeform_amd.torch.deform_grid_sample`` carries them through autograd.
``deform_grid_derivatives`` / ``deform_grid_derivatives_batch`` give the local differential structure of the coordinate
map at arbitrary real positions: ``r``, ``J = dr/dq`` and ``H = d^2r/dq dq`` (1 to 3 deformed axes);
``deform_grid_derivatives_gradient`` / ``deform_grid_derivatives_gradient_batch`` are the adjoint of all three with
respect to the positions, the displacement and affine / rotate / zoom, and
``elasticdeform_amd.torch.deform_grid_derivatives`` carries them through autograd: one call for every local
regulariser -- folding, log det, volume preservation, rigidity, diffusion, bending energy -- at sampled positions.
"""
from .deform_grid import (deform_grid, deform_grid_gradient, deform_random_grid,  # noqa: F401
                          deform_grid_batch, deform_grid_gradient_batch, set_arithmetic,
                          set_reduced_precision, set_crop_identity, set_gradient_accumulation,
                          set_field_strength, deform_grid_displacement_gradient,
                          deform_grid_displacement_gradient_batch, deform_grid_affine_gradient,
                          deform_grid_affine_gradient_batch, AffineGradient, deform_grid_coordinates,
                          deform_points, deform_grid_coordinates_batch, deform_points_batch,
                          deform_grid_labels, deform_grid_labels_batch, PointsGradient,
                          deform_grid_coordinates_gradient, deform_points_gradient,
                          deform_grid_coordinates_gradient_batch, deform_points_gradient_batch,
                          deform_grid_inverse, deform_grid_inverse_batch, deform_grid_inverse_gradient,
                          deform_grid_inverse_gradient_batch, deform_grid_inverse_displacement_gradient,
                          deform_grid_inverse_displacement_gradient_batch, deform_grid_inverse_affine_gradient,
                          deform_grid_inverse_affine_gradient_batch, JacobianGradient, deform_grid_jacobian,
                          deform_grid_jacobian_gradient, deform_grid_jacobian_batch,
                          deform_grid_jacobian_gradient_batch, deform_grid_sample, deform_grid_sample_batch,
                          deform_grid_sample_gradient, deform_grid_sample_gradient_batch,
                          deform_grid_sample_coordinate_gradient, deform_grid_sample_coordinate_gradient_batch,
                          deform_grid_sample_points_gradient, deform_grid_sample_points_gradient_batch,
                          MapDerivatives, deform_grid_derivatives, deform_grid_derivatives_batch,
                          deform_grid_derivatives_gradient, deform_grid_derivatives_gradient_batch)

from ._lib import release_scratch  # noqa: F401,E402  (frees the library's cached device scratch)

__version__ = '0.1.0'
