"""What a user does with a registration's displacement field: invert it, check a forward / backward pair against each
other, and ask where it folds.  The reference names the operation itself -- sitk.InvertDisplacementField at
platipy/imaging/visualisation/visualiser.py:1536 --; sitk.DisplacementFieldJacobianDeterminant is its standard companion.
Names and defaults are SimpleITK 2.3.1's [recalled, unverified here]; the rules are restated in include/platipy_amd.h.
SimpleITK parity is unpinned until tools/compare_with_sitk.py runs where SimpleITK exists."""
import torch

from .. import runtime
from ..image import Image, as_image
from ..transform import BSplineTransform, CompositeTransform, DisplacementFieldTransform, Transform


def _field_tensor(image, who):
    image = as_image(image)
    if not image.is_vector:
        raise ValueError(f"{who}: a planar vector Image [3, Z, Y, X] is expected, got a scalar image")
    t = image.tensor if image.tensor.dtype == torch.float32 else image.tensor.float()
    return image, t.contiguous()


def invert_displacement_field(field, maximum_number_of_iterations=10, max_error_tolerance_threshold=0.1,
                              mean_error_tolerance_threshold=0.001, enforce_boundary_condition=True, initial_estimate=None,
                              return_info=False):
    """sitk.InvertDisplacementField(field, maximumNumberOfIterations, maxErrorToleranceThreshold, meanErrorToleranceThreshold,
    enforceBoundaryCondition) [ITK-upstream, unverified here]: the fixed-point inverse v of the field u, p + v(p) + u(p + v(p)) = p,
    as a planar fp32 vector Image on the field's grid.  `initial_estimate` (a vector Image on the same grid) starts the
    iteration instead of zero.  return_info: -> (image, {"iterations", "max_error_norm", "mean_error_norm"}), the values of the
    last executed iteration, read back once; without it nothing is read back.  A scalar image, or an initial estimate on
    another grid, raises ValueError; a non-fp32 field is converted."""
    field, u = _field_tensor(field, "invert_displacement_field")
    v0 = None
    if initial_estimate is not None:
        initial_estimate, v0 = _field_tensor(initial_estimate, "invert_displacement_field: initial_estimate")
        if not initial_estimate.same_grid(field):
            raise ValueError("invert_displacement_field: the initial estimate is not on the field's grid")
        v0 = v0.to(u.device)
    ctx = runtime.context(field.device)
    out = torch.empty_like(u)
    info = ctx.invert_field(u, field.geom(), out, initial=v0, max_iterations=int(maximum_number_of_iterations),
                            max_tol=float(max_error_tolerance_threshold), mean_tol=float(mean_error_tolerance_threshold),
                            enforce_boundary=bool(enforce_boundary_condition), want_stats=bool(return_info))
    image = Image(out, field.spacing, field.origin, field.direction, True)
    return (image, info) if return_info else image


def displacement_field_jacobian_determinant(field, use_image_spacing=True, mask=None, return_stats=False):
    """sitk.DisplacementFieldJacobianDeterminant(field, useImageSpacing) [ITK-upstream, unverified here]: det(I + grad u) by
    central differences with a zero-flux border, as an fp32 scalar Image.  return_stats: -> (image, {"min", "max", "mean",
    "count", "count_nonpositive"}) over `mask`'s non-zero voxels (a scalar Image on the field's grid), or over the whole
    image; they come from the pass that writes the determinant.  count_nonpositive > 0: the field folds."""
    field, u = _field_tensor(field, "displacement_field_jacobian_determinant")
    m = None
    if mask is not None:
        mask = as_image(mask)
        if mask.is_vector or mask.GetSize() != field.GetSize():
            raise ValueError("displacement_field_jacobian_determinant: the mask is not a scalar image of the field's size")
        m = (mask.tensor if mask.tensor.dtype == torch.uint8 else (mask.tensor != 0).to(torch.uint8)).contiguous().to(u.device)
    ctx = runtime.context(field.device)
    out = torch.empty(field.shape, dtype=torch.float32, device=u.device)
    stats = ctx.jacobian_determinant(u, field.geom(), out, use_image_spacing=bool(use_image_spacing), mask=m,
                                     want_stats=bool(return_stats))
    image = Image(out, field.spacing, field.origin, field.direction, False)
    return (image, stats) if return_stats else image


def inverse_consistency_error(forward_field, inverse_field, return_image=False):
    """How far `inverse_field` is from inverting `forward_field`: {"max", "mean"} of the scaled residual norm
    |v(p) + u(p + v(p))| (components over the index axes' spacings, as the inversion measures it), by the kernel arm of one
    inversion iteration with nothing updated.  return_image: -> (dict, fp32 scalar Image of the norm)."""
    forward_field, u = _field_tensor(forward_field, "inverse_consistency_error")
    inverse_field, v = _field_tensor(inverse_field, "inverse_consistency_error")
    if not inverse_field.same_grid(forward_field):
        raise ValueError("inverse_consistency_error: the two fields are not on one grid")
    ctx = runtime.context(forward_field.device)
    norm = torch.empty(forward_field.shape, dtype=torch.float32, device=u.device) if return_image else None
    res = ctx.inverse_consistency(u, v.to(u.device), forward_field.geom(), norm_out=norm)
    if return_image:
        return res, Image(norm, forward_field.spacing, forward_field.origin, forward_field.direction, False)
    return res


def inverse_transform(transform, reference=None, **invert_kwargs):
    """The inverse of any transform apply_transform takes.  Identity and linear transforms: their GetInverse().  A
    DisplacementFieldTransform: DisplacementFieldTransform(invert_displacement_field(field, **invert_kwargs)) on the field's
    own grid.  A BSplineTransform: evaluated densely on `reference`, then inverted; without a reference it raises ValueError.
    A CompositeTransform: the members' inverses in the opposite order.  Transform.GetInverse() itself is unchanged (it raises
    TypeError for the members that are not linear)."""
    invert_kwargs.pop("return_info", None)
    if transform is None:
        return Transform()
    if isinstance(transform, CompositeTransform):
        return CompositeTransform([inverse_transform(t, reference, **invert_kwargs) for t in reversed(transform.flatten())])
    if isinstance(transform, BSplineTransform):
        if reference is None:
            raise ValueError("inverse_transform: a BSplineTransform needs a reference image to be evaluated on")
        reference = as_image(reference)
        dense = Image(transform.displacement_field(reference), reference.spacing, reference.origin, reference.direction, True)
        return DisplacementFieldTransform(invert_displacement_field(dense, **invert_kwargs))
    if isinstance(transform, DisplacementFieldTransform):
        return DisplacementFieldTransform(invert_displacement_field(transform.field, **invert_kwargs))
    return transform.GetInverse()
