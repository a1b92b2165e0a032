"""Drop-in for platipy/imaging/utils/lung.py: detect_holes (:18-62), get_external_mask (:65-85), get_lung_mask (:88-118)
and fill_holes (:121-152), on the device: the labelling, the per-label statistics and the morphology are HIP kernels
(csrc/pp_region.h, pp_morph.hip); one read-back of the label table per image.

The reference's quirks are kept and marked B1, B2 (the list continues in projects/bronchus.py)."""
import torch

from ..image import as_image
from ..label.region import connected_component, label_shape_statistics
from ..label.utils import binary_dilate, binary_morphological_closing


def detect_holes(img, lower_threshold=-10000, upper_threshold=-400):
    """Detect all (air) holes in the image -> (label_image, labels): the components of lower <= v <= upper numbered as
    sitk.ConnectedComponent numbers them, and a list of {"label", "phys_size", "elongation", "roundness", "perimeter",
    "flatness"} sorted by size, largest first.  `roundness` and `perimeter` are None (label_shape_statistics).

    B1 (lung.py:48): the list covers range(1, count) -- the LAST component is never listed.
    B2 (lung.py:60): sorted() is stable, equal sizes keep their label order."""
    img = as_image(img)
    t = img.tensor
    holes = img.like(((t >= lower_threshold) & (t <= upper_threshold)).to(torch.uint8))
    label_image, count = connected_component(holes)
    stats = label_shape_statistics(label_image, count)
    labels = []
    for region in range(1, count):      # B1
        st = stats[region]
        labels.append({"label": region, "phys_size": st["physical_size"], "elongation": st["elongation"], "roundness": st["roundness"],
                       "perimeter": st["perimeter"], "flatness": st["flatness"]})
    labels = sorted(labels, key=lambda i: i["phys_size"], reverse=True)      # B2
    return label_image, labels


def _label_equals(label_image, label):
    label_image = as_image(label_image)
    return label_image.like((label_image.tensor == int(label)).to(torch.uint8))


def get_external_mask(label_image, labels, kernel_radius=5):
    """The external mask: the largest listed hole (the air around the patient), closed with a ball of `kernel_radius`
    voxels (lung.py:77-85)."""
    return binary_morphological_closing(_label_equals(label_image, labels[0]["label"]), kernel_radius)


def get_lung_mask(label_image, labels, kernel_radius=2):
    """The lung mask: B2 -- the first entry AFTER index 0 of the size-sorted list whose flatness is <= 2, closed with a ball
    of `kernel_radius` voxels (lung.py:100-118).

    Deviation: when no entry satisfies the flatness test (or there is none after index 0) the reference runs off the end
    of the list with an IndexError -- its own `lung_idx > len(labels)` guard comes one step too late; here that is None."""
    lung_idx = 1
    while True:
        if lung_idx >= len(labels):
            return None
        if not labels[lung_idx]["flatness"] > 2:
            break
        lung_idx += 1
    return binary_morphological_closing(_label_equals(label_image, labels[lung_idx]["label"]), kernel_radius)


def fill_holes(img, label_image, external_mask, lung_mask, fill_value=50):
    """The image with all holes filled except the external and the lung holes (lung.py:135-152).  As in the reference the
    hole mask is BinaryThreshold(label_image, 1, int(img.max())) -- labels above the image's maximum are NOT holes -- minus
    the two masks in uint8 arithmetic, which wraps: only voxels that are exactly 1 afterwards are dilated (ball, 3 voxels)
    and filled.  An image whose maximum is below 1 has no holes to fill (the reference's threshold raises)."""
    img = as_image(img)
    label_image, external_mask, lung_mask = as_image(label_image), as_image(external_mask), as_image(lung_mask)
    top = int(img.tensor.max())
    lab = label_image.tensor
    mask = ((lab >= 1) & (lab <= top)).to(torch.uint8)
    mask = mask - external_mask.tensor.to(torch.uint8)      # (uint8: 0 - 1 wraps to 255, as sitk.Subtract does)
    mask = mask - lung_mask.tensor.to(torch.uint8)
    grown = binary_dilate(img.like((mask == 1).to(torch.uint8)), 3)
    out = img.tensor.clone()
    out[grown.tensor == 1] = fill_value
    return img.like(out)
