"""Drop-in for platipy/imaging/generation/mask.py: extend_mask (:107-159), used by the structure-guided cardiac
pipeline (projects/cardiac/run.py:741-746, 826-831) -- a handful of slice copies on the device tensor -- and get_bone_mask
(:21-47), which generate_random_augmentation needs.  get_external_mask (per-slice convex hulls from scikit-image) has no
counterpart here; the external mask of imaging/utils/lung.py (the closed outside-air component) is utils/lung.py's."""
import numpy as np
import torch

from ..image import as_image
from ..label.utils import binary_morphological_closing


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
