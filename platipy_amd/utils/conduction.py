"""Drop-in for platipy/imaging/utils/conduction.py:26-254: the geometric definitions of the sinoatrial and atrioventricular
nodes (after Loap et al. 2021), composed from the existing kernels.  The reference's 2-D steps (sitk images sliced with
[:, :, k]) run here on one-slice volumes: ball morphology with radius (e, e, 0) and the Maurer distance map of a volume with
size[2] == 1 are the 2-D filters.

Quirks of the reference that are kept:
  C1  geometric_atrioventricularnode has four erosion loops, but only the first can run: the other three start from
      `overlap = 0; while overlap > 0` (conduction.py:202-227) and are dead.  They are kept as no-ops.
  C2  that first loop erodes the LEFT VENTRICLE cumulatively by 1, 2, 3, ... voxels until it no longer touches the left atrium.
  C3  np.mean(..., dtype=int) of the four closest points truncates.
  C4  a minimum distance shared by several voxels goes to the first of them in raster order (np.where + argmin).
"""
import numpy as np
import torch

from ..generation.image import insert_sphere_image
from ..image import as_image
from ..label.iar import distance_map
from ..label.utils import binary_dilate, binary_erode, check_dilate_radius, get_com
from .crop import crop_to_roi, label_to_roi, paste


def _binary(label):
    label = as_image(label)
    return label.like((label.tensor != 0).to(torch.uint8))


def _first_slice(label):
    """np.min(np.where(arr)[0]): the most inferior slice that holds a voxel of the label."""
    z = torch.nonzero(label.tensor.flatten(1).any(dim=1))
    if z.numel() == 0:
        raise ValueError("the label is empty")
    return int(z[0])


def _slice_image(label, k):
    """label[:, :, k] as a one-slice volume at its physical position."""
    return crop_to_roi(label, (label.GetSize()[0], label.GetSize()[1], 1), (0, 0, int(k)))


def _first_minimum(distance, where):
    """(row, column) of the first voxel in raster order, among those where `where` is set, at which the 2-D tensor
    `distance` is smallest (np.where + argmin)."""
    if not bool(where.any()):
        raise ValueError("attempt to get argmin of an empty sequence")
    smallest = distance[where].min()
    loc = torch.nonzero(where & (distance == smallest))[0]
    return int(loc[0]), int(loc[1])


def get_closest_point_2d(reference_label, measurement_label):
    """The point (row, column) of `measurement_label` closest to `reference_label` (conduction.py:26-54): one-slice Images;
    the distance is the signed Maurer map of the reference, so points inside it count as closer than its border."""
    reference_label, measurement_label = as_image(reference_label), as_image(measurement_label)
    distancemap_2d = distance_map(reference_label, signed=True)
    return _first_minimum(distancemap_2d.tensor[0], measurement_label.tensor[0] != 0)


def geometric_sinoatrialnode(label_svc, label_ra, label_wholeheart, radius_mm=10):
    """Geometric definition of the sinoatrial node (conduction.py:57-148): a sphere on the most inferior slice of the
    (dilated) SVC, at the point at least 10 voxels inside the whole heart that is closest to where the SVC meets the right
    atrium."""
    label_svc, label_ra, label_wholeheart = _binary(label_svc), _binary(label_ra), _binary(label_wholeheart)
    template_img = 0 * label_wholeheart
    cb_size, cb_index = label_to_roi([label_svc, label_ra, label_wholeheart], expansion_mm=(20, 20, 20))
    label_svc = crop_to_roi(label_svc, cb_size, cb_index)
    label_ra = crop_to_roi(label_ra, cb_size, cb_index)
    label_wholeheart = crop_to_roi(label_wholeheart, cb_size, cb_index)
    inf_limit_svc = _first_slice(label_svc)
    overlap = 0
    dilate = 1
    dilate_ax = 0
    while overlap == 0:
        check_dilate_radius((dilate, dilate, dilate_ax), "geometric_sinoatrialnode")
        label_svc_dilate = binary_dilate(label_svc, (dilate, dilate, dilate_ax))
        label_overlap = label_ra.like(label_svc_dilate.tensor & label_ra.tensor)
        overlap = int(label_overlap.tensor[inf_limit_svc].sum())
        dilate += 1
        if dilate >= 3:
            inf_limit_svc = _first_slice(label_svc_dilate)
            dilate_ax += 1
    intersect_loc = get_com(label_overlap)
    intersect = torch.zeros_like(label_ra.tensor)
    intersect[inf_limit_svc, intersect_loc[1], intersect_loc[2]] = 1
    potential_san_region = binary_erode(label_wholeheart, (10, 10, 0))
    distancemap_san = distance_map(label_ra.like(intersect), signed=True)
    y, x = _first_minimum(distancemap_san.tensor[inf_limit_svc], potential_san_region.tensor[inf_limit_svc] != 0)     # C4
    label_san = insert_sphere_image(label_ra * 0, sp_radius=radius_mm, sp_centre=(inf_limit_svc, y, x))
    return paste(template_img, label_san, cb_index)


def geometric_atrioventricularnode(label_la, label_lv, label_ra, label_rv, radius_mm=10):
    """Geometric definition of the atrioventricular node (conduction.py:151-254): a sphere 1 cm above the most inferior slice
    of the left atrium, at the mean of the four points where each chamber comes closest to the one diagonally opposite."""
    label_la, label_lv, label_ra, label_rv = (_binary(l) for l in (label_la, label_lv, label_ra, label_rv))
    template_img = 0 * label_ra
    cb_size, cb_index = label_to_roi([label_la, label_lv, label_ra, label_rv], expansion_mm=(20, 20, 20))
    label_la = crop_to_roi(label_la, cb_size, cb_index)
    label_lv = crop_to_roi(label_lv, cb_size, cb_index)
    label_ra = crop_to_roi(label_ra, cb_size, cb_index)
    label_rv = crop_to_roi(label_rv, cb_size, cb_index)
    inf_limit_la = _first_slice(label_la)
    slice_loc = int(inf_limit_la + 10 / label_la.GetSpacing()[2])
    if slice_loc >= label_la.GetSize()[2]:
        raise IndexError(f"geometric_atrioventricularnode: slice {slice_loc} lies above the cropped volume")
    label_la_2d = _slice_image(label_la, slice_loc)
    label_lv_2d = _slice_image(label_lv, slice_loc)
    label_ra_2d = _slice_image(label_ra, slice_loc)
    label_rv_2d = _slice_image(label_rv, slice_loc)
    # C2: erode the left ventricle until it is clear of the left atrium
    overlap = 1
    erode = 1
    while overlap > 0:
        check_dilate_radius((erode, erode, 0), "geometric_atrioventricularnode")
        label_lv_2d = binary_erode(label_lv_2d, (erode, erode, 0))
        overlap = int((label_lv_2d.tensor & label_la_2d.tensor).sum())
        erode += 1
    # C1: the reference's three further loops (left atrium / right atrium, right atrium / right ventricle, right ventricle /
    # left ventricle) start from overlap = 0 and never run
    for _ in ("LEFT ATRIUM", "RIGHT ATRIUM", "RIGHT VENTRICLE"):
        overlap = 0
        while overlap > 0:
            pass
    y_la, x_la = get_closest_point_2d(label_rv_2d, label_la_2d)
    y_lv, x_lv = get_closest_point_2d(label_ra_2d, label_lv_2d)
    y_ra, x_ra = get_closest_point_2d(label_lv_2d, label_ra_2d)
    y_rv, x_rv = get_closest_point_2d(label_la_2d, label_rv_2d)
    x_location = np.mean((x_la, x_lv, x_ra, x_rv), dtype=int)      # C3
    y_location = np.mean((y_la, y_lv, y_ra, y_rv), dtype=int)
    label_avn = insert_sphere_image(label_ra * 0, sp_radius=radius_mm, sp_centre=(slice_loc, y_location, x_location))
    return paste(template_img, label_avn, cb_index)
