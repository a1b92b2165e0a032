"""Drop-in for the pieces of platipy/imaging/label/utils.py the pipelines use after fusion:
correct_volume_overlap (:23-58, element-wise tensor arithmetic on the GPU), plus the binary-mask SimpleITK calls
the pipelines make inline -- BinaryDilate / BinaryErode / BinaryMorphologicalClosing with the ball kernel and
"RelabelComponent(ConnectedComponent(x)) == 1" -- as HIP kernels (pp_morph.hip, pp_cc.hip), and get_com (:61-84) from the
per-slice moments kernel (pp_vessel.h)."""
import numpy as np
import torch

from .. import runtime
from ..image import as_image

_DILATE, _ERODE, _CLOSE = 0, 1, 2


def _u8(image):
    t = image.tensor
    return (t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)).contiguous()


MAX_DILATE_RADIUS = 15   # voxels per axis: what the valve / conduction-node definitions may ask binary_dilate for


def _radius3(image, radius):
    if not hasattr(radius, "__iter__"):
        radius = [radius] * 3
    radius = [int(r) for r in radius]
    if len(radius) != 3 or min(radius) < 0:
        raise ValueError(f"kernel radius must be three non-negative voxel counts, got {radius}")
    return radius


def check_dilate_radius(radius, who):
    """The geometric definitions dilate by a radius derived from mm and the spacing; above MAX_DILATE_RADIUS voxels on an axis
    that is refused by name (two smaller balls are not one large ball, so nothing is composed)."""
    if max(int(r) for r in radius) > MAX_DILATE_RADIUS:
        raise ValueError(f"{who}: dilation radius {tuple(int(r) for r in radius)} voxels exceeds the limit of {MAX_DILATE_RADIUS} "
                         "voxels per axis")


def _morph(mask, radius, op):
    mask = as_image(mask)
    radius = _radius3(mask, radius)
    src = _u8(mask)
    out = torch.empty_like(src)
    runtime.context(mask.device).binary_morph_ball(src, mask.GetSize(), radius, op, out)
    return mask.like(out)


def binary_dilate(mask, radius):
    """sitk.BinaryDilate(mask, radius): ball kernel, radius in voxels (x, y, z) (registration/utils.py:328-329)."""
    return _morph(mask, radius, _DILATE)


def binary_erode(mask, radius):
    """sitk.BinaryErode(mask, radius): ball kernel, the image boundary counts as foreground."""
    return _morph(mask, radius, _ERODE)


def binary_morphological_closing(mask, radius):
    """sitk.BinaryMorphologicalClosing(mask, radius), safe border (multiatlas/run.py:422, cardiac/run.py:1128)."""
    return _morph(mask, radius, _CLOSE)


def largest_component(mask, fully_connected=False):
    """sitk.RelabelComponent(sitk.ConnectedComponent(mask, fully_connected)) == 1 (multiatlas/run.py:421;
    generation/mask.py:77-80 with fully_connected): the largest component, the first in raster order on ties; an empty
    mask stays empty."""
    mask = as_image(mask)
    src = _u8(mask)
    out = torch.empty_like(src)
    ctx = runtime.context(mask.device)
    if fully_connected:
        ctx.fillhole_largest_component_conn(src, mask.GetSize(), out, fill_holes=False, keep_largest=True, fully_connected=True)
    else:
        ctx.fillhole_largest_component(src, mask.GetSize(), out, fill_holes=False)
    return mask.like(out)


def binary_fillhole(mask, fully_connected=False):
    """sitk.BinaryFillhole(mask, fullyConnected): background that is not connected to the image border becomes foreground.
    fully_connected is the connectivity of that BACKGROUND flood: with it a cavity that reaches the outside through a
    diagonal gap is not a hole (generation/mask.py:92)."""
    mask = as_image(mask)
    src = _u8(mask)
    out = torch.empty_like(src)
    runtime.context(mask.device).fillhole_largest_component_conn(src, mask.GetSize(), out, fill_holes=True, keep_largest=False,
                                                                fully_connected=bool(fully_connected))
    return mask.like(out)


def correct_volume_overlap(binary_label_dict, assign_overlap_to_largest=True):
    """Make the structures disjoint: rank them by volume (largest first by default) and give every voxel to the
    first structure in that order that contains it.  The reference does this by prime-encoding the labels
    (label/utils.py:44-56); the result is the same set arithmetic."""
    names = list(binary_label_dict.keys())
    labels = {k: as_image(v) for k, v in binary_label_dict.items()}
    vals = [int((labels[k].tensor != 0).sum()) for k in names]
    rank = np.argsort(vals)[::-1] if assign_overlap_to_largest else np.argsort(vals)
    ranked = [names[i] for i in rank]
    first = labels[ranked[0]]
    taken = torch.zeros(first.shape, dtype=torch.bool, device=first.device)
    out = {}
    for k in ranked:
        m = (labels[k].tensor != 0) & ~taken
        taken |= m
        out[k] = labels[k].like(m.to(torch.uint8))
    return out


def binary_encode_structure_list(structure_list):
    """Encode up to 32 binary labels into one integer image, structure k in bit k + 1 (reference label/utils.py:219-254).
    The reference casts to UInt32, which cannot hold bit 32; the tensor here is int64."""
    if len(structure_list) > 32:
        raise ValueError("You can only encode a maximum of 32 structures with this method!")
    first = as_image(structure_list[0])
    enc = torch.zeros(first.shape, dtype=torch.int64, device=first.device)
    for power, s_img in enumerate(structure_list):
        enc |= (as_image(s_img).tensor != 0).to(torch.int64) << (power + 1)
    return first.like(enc)


def binary_decode_image(binary_encoded_img):
    """Decode a binary-encoded label map into the list of non-empty structures (reference label/utils.py:257-288)."""
    img = as_image(binary_encoded_img)
    enc = img.tensor.to(torch.int64)
    out = []
    for power in range(32):
        s = (enc & (1 << (power + 1))) != 0
        if bool(s.any()):
            out.append(img.like(s.to(torch.uint8)))
    return out


def _weights_u8(image, who):
    """The label as the uint8 volume the moments kernel reads: its own values (the reference weights by value)."""
    t = image.tensor
    if t.dtype == torch.uint8:
        return t.contiguous()
    if t.dtype == torch.bool:
        return t.to(torch.uint8).contiguous()
    if t.dtype.is_floating_point or int(t.min()) < 0 or int(t.max()) > 255:
        raise TypeError(f"{who}: the label must hold integers 0 ... 255 (uint8), got {t.dtype}")
    return t.to(torch.uint8).contiguous()


def slice_moments(labels, scan_direction="z"):
    """int64 numpy array [len(labels), slices, 4] = {sum v, sum a v, sum b v, count(v != 0)} of every slice along
    `scan_direction` ("z": a = row (image y), b = column (image x); "x": a = array z, b = array y) of labels on one grid:
    the integer sums behind com_from_image_list (utils/vessel.py:33-167), exactly numpy's (pp_slice_moments_u8).  The
    reference's "y" falls through and crashes; here it is a ValueError."""
    axis = {"x": 0, "z": 2}.get(str(scan_direction).lower())
    if axis is None:
        raise ValueError(f"scan direction must be 'x' or 'z', got {scan_direction!r}")
    labels = [as_image(l) for l in labels]
    if len(labels) == 0:
        raise ValueError("slice_moments: no labels")
    size = labels[0].GetSize()
    if any(l.GetSize() != size for l in labels):
        raise ValueError("slice_moments: the labels must share one grid")
    masks = [_weights_u8(l, "slice_moments") for l in labels]
    ctx = runtime.context(labels[0].device)
    out = torch.empty((len(masks), size[axis], 4), dtype=torch.int64, device=labels[0].device)
    for k in range(0, len(masks), 64):     # the kernel takes 64 masks per launch
        ctx.slice_moments(masks[k:k + 64], size, axis, out[k:k + 64])
    return out.cpu().numpy()


def get_com(label, as_int=True, real_coords=False):
    """Centre of mass of a label (label/utils.py:61-84): scipy.ndimage.center_of_mass of the array, (z, y, x), from the exact
    integer moments in fp64; as_int truncates each component, real_coords returns the physical point (x, y, z) instead.
    An empty label gives NaN (int() of it raises, as in the reference)."""
    label = as_image(label)
    m = slice_moments([label], "z")[0]
    total = float(m[:, 0].sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        com = [np.float64(float((np.arange(m.shape[0], dtype=np.int64) * m[:, 0]).sum())) / total,
               np.float64(float(m[:, 1].sum())) / total, np.float64(float(m[:, 2].sum())) / total]
    if real_coords:
        d = np.asarray(label.direction, dtype=np.float64).reshape(3, 3)
        p = np.asarray(label.origin, dtype=np.float64) + d @ (np.asarray(label.spacing, dtype=np.float64) * np.array(com[::-1]))
        return tuple(float(v) for v in p)
    if as_int:
        return [int(i) for i in com]
    return tuple(float(c) for c in com)
