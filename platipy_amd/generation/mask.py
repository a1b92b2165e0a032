"""Drop-in for platipy/imaging/generation/mask.py: extend_mask (:107-159), used by the structure-guided cardiac
pipeline (projects/cardiac/run.py:741-746, 826-831) -- a handful of slice copies on the device tensor --, get_bone_mask
(:21-47), which generate_random_augmentation needs, and get_external_mask (:50-104), the patient external contour the
synthetic-deformation walkthroughs start from: threshold, largest fully connected component, ball dilation, optional
closing and hole filling, then the convex hull image of every slice (pp_slice_convex_hull_u8 in place of the Python loop
over skimage's convex_hull_image).  The external mask of imaging/utils/lung.py (the closed outside-air component) is
another function: utils/lung.py's."""
import numpy as np
import torch

from ..image import as_image
from ..label.region import slice_convex_hull
from ..label.utils import binary_dilate, binary_fillhole, binary_morphological_closing, check_dilate_radius, largest_component


def _threshold_closed(t, lower, upper):
    """sitk.BinaryThreshold: lower <= v <= upper, both ends included, compared in double; a NaN is outside.  A float32
    tensor is compared with the bounds rounded inwards to float32, which decides every value as the double comparison
    does without a double copy of the volume."""
    lower, upper = float(lower), float(upper)
    if t.dtype == torch.float32 and not (np.isnan(lower) or np.isnan(upper)):
        with np.errstate(over="ignore"):
            lo, hi = np.float32(lower), np.float32(upper)
        if float(lo) < lower:
            lo = np.nextafter(lo, np.float32(np.inf))
        if float(hi) > upper:
            hi = np.nextafter(hi, np.float32(-np.inf))
        return ((t >= float(lo)) & (t <= float(hi))).to(torch.uint8)
    v = t.to(torch.float64)
    return ((v >= lower) & (v <= upper)).to(torch.uint8)


def get_bone_mask(image, lower_threshold=350, upper_threshold=3500, max_hole_size=5):
    """A binary mask of bones from a CT image (reference mask.py:21-47): sitk.BinaryThreshold on [lower, upper], both ends
    included, then sitk.BinaryMorphologicalClosing with the ball.  Quirk kept (:41-45): `max_hole_size` is documented as
    millimetres in z, y, x order but reaches the filter as a kernel radius in VOXELS, x, y, z; False closes nothing."""
    image = as_image(image)
    t = image.tensor
    bone_mask = image.like(((t >= lower_threshold) & (t <= upper_threshold)).to(torch.uint8))
    if max_hole_size is not False:
        if not hasattr(max_hole_size, "__iter__"):
            max_hole_size = (max_hole_size,) * 3
    return binary_morphological_closing(bone_mask, max_hole_size)


def get_external_mask(image, lower_threshold=-100, upper_threshold=2500, dilate=1, max_hole_size=False):
    """A binary mask of the patient external contour by slice-wise convex hulls (reference mask.py:50-104) -> uint8 Image on
    the input's grid.  The reference's order is kept: sitk.BinaryThreshold on [lower, upper] (:73-75) ->
    sitk.ConnectedComponent(mask, True) and RelabelComponent == 1, the largest FULLY connected component (:77-80) ->
    sitk.BinaryDilate with the ball (:82-85) -> with max_hole_size only, sitk.BinaryMorphologicalClosing and
    sitk.BinaryFillhole(fullyConnected=True) (:87-92) -> skimage's convex_hull_image of every slice (:94-99).  Quirks kept:
      E1 (:83-85, :88-91) `dilate` and `max_hole_size` are documented as millimetres in (z, y, x) order but reach SimpleITK
         as kernel radii in VOXELS, in (x, y, z) order; a scalar is repeated three times, False skips the step.
      E2 (:87) closing and hole filling run only when max_hole_size is given: the default leaves the cavities to the hull.
      E3 (:98) np.alen no longer exists under the reference's own locked numpy; the loop is over the slices.
    A radius above 15 voxels on an axis is refused by name (label.utils.check_dilate_radius).  A threshold that selects
    nothing gives an all-zero mask."""
    image = as_image(image)
    body_mask = largest_component(image.like(_threshold_closed(image.tensor, lower_threshold, upper_threshold)), fully_connected=True)
    if dilate is not False:
        if not hasattr(dilate, "__iter__"):
            dilate = (dilate,) * 3
        check_dilate_radius(dilate, "get_external_mask(dilate)")
        body_mask = binary_dilate(body_mask, dilate)                       # E1
    if max_hole_size is not False:                                         # E2
        if not hasattr(max_hole_size, "__iter__"):
            max_hole_size = (max_hole_size,) * 3
        check_dilate_radius(max_hole_size, "get_external_mask(max_hole_size)")
        body_mask = binary_morphological_closing(body_mask, max_hole_size)
        body_mask = binary_fillhole(body_mask, fully_connected=True)
    return slice_convex_hull(body_mask)                                    # E3


def extend_mask(mask, direction=("ax", "sup"), extension_mm=10, interior_mm_shape=10):
    """Extend a binary label a number of slices along the axial direction; the extended part takes the shape of
    the union (max) of `interior_mm_shape` worth of the label's end slices.  Only the "ax" axis is handled, as in
    the reference ("PROTOTYPE!", mask.py:110).  Python slice semantics are kept as the reference has them,
    including the empty slices its negative/inverted ranges produce."""
    mask = as_image(mask)
    t = mask.tensor
    vals = torch.unique(t[t > 0])
    if len(vals) > 2:
        cutoff = float(np.median(vals.cpu().numpy()))
        arr = ((t >= cutoff) & (t <= float(vals.max()))).to(torch.uint8)
    else:
        arr = t.clone()
    if direction[0] == "ax":
        occupied = torch.nonzero((arr != 0).flatten(1).any(dim=1)).flatten()
        if occupied.numel() == 0:
            raise ValueError("extend_mask: the mask is empty")   # the reference fails in np.min of an empty array
        inferior_slice, superior_slice = int(occupied.min()), int(occupied.max())
        n_slices_ext = int(extension_mm / mask.GetSpacing()[2])
        n_slices_est = int(interior_mm_shape / mask.GetSpacing()[2])

        def shape_of(lo, hi):
            sl = arr[lo:hi]
            if sl.shape[0] == 0:
                raise ValueError("extend_mask: no interior slices to take the shape from")   # np.max over an empty axis
            return sl.max(dim=0).values

        if direction[1] == "sup":
            max_index = min(arr.shape[0], superior_slice + 1 + n_slices_ext)
            for s_in in range(superior_slice + 1 - n_slices_est, max_index):
                arr[s_in] = shape_of(superior_slice - n_slices_est, superior_slice)
        if direction[1] == "inf":
            min_index = max(arr.shape[0], inferior_slice - n_slices_ext + n_slices_est)
            for s_in in range(min_index, inferior_slice):
                arr[s_in] = shape_of(inferior_slice + n_slices_est, inferior_slice)
    return mask.like(arr)
