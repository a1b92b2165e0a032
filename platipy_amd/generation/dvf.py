"""Drop-in for platipy/imaging/generation/dvf.py: the five synthetic deformation-field generators (shift, asymmetric
contract / extend, expand, radial bend), on torch tensors in HBM.

Every generator returns (deformed mask or image, DisplacementFieldTransform, dvf Image); the field is this project's planar
fp32 [3, Z, Y, X] vector Image (x, y, z components in mm), as demons returns it -- the reference's is sitkVectorFloat64.  No
volume leaves the device: constant and radial fields are torch broadcasts, masks are warped by pp_resample_u8, fields
smoothed by pp_recursive_gaussian_field_f32, structures grown by pp_binary_morph_ball_u8 and registered by the demons
kernels.  The reference's quirks are kept and marked G1-G6 below (SURVEY N1-N6 style).
"""
import logging

import numpy as np
import torch

from .. import runtime
from ..image import as_image
from ..label.utils import binary_dilate, binary_erode
from ..registration.deformable import fast_symmetric_forces_demons_registration
from ..registration.utils import apply_transform, convert_mask_to_reg_structure
from ..transform import DisplacementFieldTransform, sitkLinear, sitkNearestNeighbor

logger = logging.getLogger(__name__)


def _constant_field(mask_image, vector_zyx, sign):
    """dvf_arr = zeros(shape + (3,)) +- vector[::-1] (dvf.py:54-55, :114-115, :187-188).  G1: the vector is given in z, y, x
    order and the field's components are x, y, z."""
    comps = torch.tensor([sign * float(v) for v in vector_zyx[::-1]], dtype=torch.float32, device=mask_image.device)
    return comps.view(3, 1, 1, 1).expand((3,) + mask_image.shape).contiguous()


def _mask_field(field, keep):
    """sitk.Mask(dvf_template, mask): the vector where the mask is non-zero, 0 elsewhere."""
    return field * (keep != 0).to(field.dtype)


def _smooth_field(field, image, gaussian_smooth):
    """sitk.SmoothingRecursiveGaussian(dvf_template, gaussian_smooth) when np.any(gaussian_smooth) (dvf.py:69-74): sigma in
    mm, a scalar or (x, y, z) -- the recursive Gaussian demons uses for the same SimpleITK call, in place on `field`.  The
    kernel refuses axes shorter than four voxels, as ITK does; that error surfaces."""
    if np.any(gaussian_smooth):
        if not hasattr(gaussian_smooth, "__iter__"):
            gaussian_smooth = (gaussian_smooth,) * 3
        runtime.context(image.device).recursive_gaussian_field(field, image.geom(), [float(s) for s in gaussian_smooth])
    return field


def _warp_mask(mask_image, field):
    """-> (apply_transform(mask, DisplacementFieldTransform(field), 0, nearest neighbour), the transform, the field Image)"""
    dvf = mask_image.like(field, True)
    tfm = DisplacementFieldTransform(dvf)
    return apply_transform(mask_image, transform=tfm, default_value=0, interpolator=sitkNearestNeighbor), tfm, dvf


def generate_field_shift(mask_image, vector_shift=(10, 10, 10), gaussian_smooth=5):
    """Shifts (moves) a structure defined using a binary mask (reference dvf.py:29-81).

    vector_shift: (sup/inf, post/ant, left/right) in mm.  Returns (shifted mask, transform, dvf)."""
    mask_image = as_image(mask_image)
    field = _constant_field(mask_image, vector_shift, -1.0)                     # :54-55 (G1)
    mask_image_shift, _, _ = _warp_mask(mask_image, field)                      # :61-64, through the UNMASKED constant field
    # G2 (:66): the field lives on mask | shifted mask, and it is masked BEFORE it is smoothed
    field = _mask_field(field, (mask_image.tensor != 0) | (mask_image_shift.tensor != 0))
    field = _smooth_field(field, mask_image, gaussian_smooth)
    return _warp_mask(mask_image, field)                                        # :76-81: the mask through the SMOOTHED field


def generate_field_asymmetric_contract(mask_image, vector_asymmetric_contract=(10, 10, 10), gaussian_smooth=5, compute_real_dvf=False):
    """Contracts a structure using a specified vector (reference dvf.py:84-156): + vector inside the mask."""
    mask_image = as_image(mask_image)
    field = _mask_field(_constant_field(mask_image, vector_asymmetric_contract, 1.0), mask_image.tensor)     # :114-121
    mask_contract, _, _ = _warp_mask(mask_image, field)
    if compute_real_dvf:
        # G3 (:129-141): the "real" field is a demons registration of the two masks' registration structures (expansion 3 mm,
        # the contracted one as the fixed image), replacing the template altogether
        reg_struct = convert_mask_to_reg_structure(mask_image, expansion=3)
        reg_struct_def = convert_mask_to_reg_structure(mask_contract, expansion=3)
        _, _, dvf_template = fast_symmetric_forces_demons_registration(reg_struct_def, reg_struct, isotropic_resample=True,
                                                                       resolution_staging=[4, 2], iteration_staging=[20, 10])
        field = dvf_template.tensor
    field = _smooth_field(field, mask_image, gaussian_smooth)
    return _warp_mask(mask_image, field)


def generate_field_asymmetric_extend(mask_image, vector_asymmetric_extend=(10, 10, 10), gaussian_smooth=5):
    """Extends a structure using a specified vector (reference dvf.py:159-216): - vector inside the WARPED mask."""
    mask_image = as_image(mask_image)
    field = _constant_field(mask_image, vector_asymmetric_extend, -1.0)         # :187-188
    mask_extend, _, _ = _warp_mask(mask_image, field)
    field = _mask_field(field, mask_extend.tensor)                              # :200
    field = _smooth_field(field, mask_image, gaussian_smooth)
    return _warp_mask(mask_image, field)


def _expand_radii(mask, expand):
    """dvf.py:254-263 -> float (x, y, z) radii in voxels, signed.  G4: `expand` is z, y, x in mm; it is divided by the
    spacing reversed and then re-ordered to x, y, z; the kernels get np.abs(...).astype(int)."""
    if not hasattr(expand, "__iter__"):
        expand = (expand,) * 3
    expand = np.array(expand) / np.array(mask.GetSpacing()[::-1])
    return expand[::-1]


def _expand_mask(mask, expand):
    """The morphological intermediate of generate_field_expand (dvf.py:266-287): BinaryErode when every factor is <= 0,
    BinaryDilate when every factor is >= 0 (all zeros erode: the first test wins), otherwise dilate by the positive factors,
    then erode by the negative ones; ITK's ball, radii in voxels."""
    mask = as_image(mask)
    expand = _expand_radii(mask, expand)
    if np.all(expand <= 0):
        logger.info("All factors negative: shrinking only.")
        return binary_erode(mask, np.abs(expand).astype(int).tolist())
    if np.all(expand >= 0):
        logger.info("All factors positive: expansion only.")
        return binary_dilate(mask, np.abs(expand).astype(int).tolist())
    logger.info("Mixed factors: shrinking and expansion.")
    expansion_kernel = expand * (expand > 0)
    shrink_kernel = expand * (expand < 0)
    mask_expand = binary_dilate(mask, np.abs(expansion_kernel).astype(int).tolist())
    return binary_erode(mask_expand, np.abs(shrink_kernel).astype(int).tolist())


def _expand_structures(mask, bone_mask, expand, use_internal_deformation):
    """-> (fixed, moving) of generate_field_expand's registration (dvf.py:248-298): the expanded and the original structure,
    `bone_mask` ADDED to both (G5: a sum, so bone inside the structure counts 2), each converted to a registration structure
    when `use_internal_deformation`."""
    mask_original = mask + bone_mask if bone_mask is not False else mask
    mask_expand = _expand_mask(mask, expand)
    if bone_mask is not False:
        mask_expand = mask_expand + bone_mask
    if use_internal_deformation:
        return convert_mask_to_reg_structure(mask_expand), convert_mask_to_reg_structure(mask_original)
    return mask_expand, mask_original


def generate_field_expand(mask, bone_mask=False, expand=3, gaussian_smooth=5, use_internal_deformation=True):
    """Expands (or shrinks) a structure with a ball kernel and finds the field by registration (reference dvf.py:219-324).

    expand: (z, y, x) size of the kernel in mm, negative to shrink.  bone_mask: a mask of regions expected not to deform."""
    mask = as_image(mask)
    if bone_mask is not False:
        bone_mask = as_image(bone_mask)
    fixed, moving = _expand_structures(mask, bone_mask, expand, use_internal_deformation)
    _, _, dvf_template = fast_symmetric_forces_demons_registration(fixed, moving, isotropic_resample=True, resolution_staging=[4, 2],
                                                                   iteration_staging=[10, 10], ncores=8)            # :301-308
    field = _smooth_field(dvf_template.tensor, mask, gaussian_smooth)
    return _warp_mask(mask, field)


def generate_field_radial_bend(reference_image, body_mask, reference_point, axis_of_rotation=[0, 0, -1], scale=0.1,
                               mask_bend_from_reference_point=("z", "inf"), gaussian_smooth=5):
    """A synthetic field of radial bending about `reference_point` (reference dvf.py:327-415), e.g. a moving head.

    reference_point and axis_of_rotation are (z, y, x); mask_bend_from_reference_point = (axis, side) cuts the body mask on
    one side of the reference point, or False.  Returns (bent image, transform, dvf)."""
    reference_image, body_mask = as_image(reference_image), as_image(body_mask)
    body = body_mask.tensor != 0
    # the slices take the point as it is given (:364-379: whole numbers, anything else is a TypeError there and here); the
    # vectors are formed from its values as they are (:382), so without a cut the point may lie between voxels
    rz, ry, rx = reference_point
    if mask_bend_from_reference_point is not False:                             # Python slices as the reference has them
        body = body.clone()
        axis, side = mask_bend_from_reference_point[0], mask_bend_from_reference_point[1]
        if axis == "z":
            if side == "inf":
                body[:rz, :, :] = False
            elif side == "sup":
                body[rz:, :, :] = False
        if axis == "y":
            if side == "post":
                body[:, ry:, :] = False
            elif side == "ant":
                body[:, :ry, :] = False
        if axis == "x":
            if side == "left":
                body[:, :, rx:] = False
            elif side == "right":
                body[:, :, :rx] = False
    nz, ny, nx = reference_image.shape
    dev = reference_image.device
    field = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=dev)
    if scale is not False:
        # G6 (:381-394): cross((idx - ref)[::-1], axis[::-1]) * scale with idx - ref in VOXEL INDICES, not mm -- on an
        # anisotropic grid the bend is not a rotation in space.  fp64 index grids along each axis, broadcast; fp32 storage.
        n = np.array(axis_of_rotation, dtype=np.float64)
        n = n / np.linalg.norm(n)
        bx, by, bz = n[::-1]
        ax = (torch.arange(nx, dtype=torch.float64, device=dev) - rx).view(1, 1, nx)
        ay = (torch.arange(ny, dtype=torch.float64, device=dev) - ry).view(1, ny, 1)
        az = (torch.arange(nz, dtype=torch.float64, device=dev) - rz).view(nz, 1, 1)
        cross = (ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx)
        for c in range(3):
            field[c] = torch.where(body, (cross[c] * scale).expand(nz, ny, nx), torch.zeros((), dtype=torch.float64, device=dev)).float()
    field = _smooth_field(field, reference_image, gaussian_smooth)
    dvf = reference_image.like(field, True)
    tfm = DisplacementFieldTransform(dvf)
    bent = apply_transform(reference_image, transform=tfm, default_value=int(reference_image.tensor.min()), interpolator=sitkLinear)
    return bent, tfm, dvf
