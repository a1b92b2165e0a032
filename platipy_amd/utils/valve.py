"""Drop-in for platipy/imaging/utils/valve.py:28-180: the geometric definitions of the four heart valves, composed step for
step from the kernels the build already has -- bounding box, crop and paste (utils/crop.py), ball morphology and the moments
behind get_com (label/utils.py), the inserted cylinder (generation/image.py) and nearest-neighbour rotation
(utils/geometry.py).  Labels are binary Images; every intermediate stays on the device."""
import numpy as np
import torch

from ..generation.image import insert_cylinder_image
from ..image import as_image
from ..label.utils import binary_dilate, binary_morphological_closing, check_dilate_radius, get_com
from ..transform import sitkNearestNeighbor
from .crop import crop_to_roi, label_to_roi, paste
from .geometry import rotate_image, vector_angle


def _binary(label):
    """The label as a 0 / 1 uint8 Image."""
    label = as_image(label)
    return label.like((label.tensor != 0).to(torch.uint8))


def generate_valve_from_great_vessel(label_great_vessel, label_ventricle, valve_thickness_mm=8):
    """Geometrically defined pulmonic / aortic valve (valve.py:28-82): the part of the great vessel within
    `valve_thickness_mm` (converted to voxels with the z spacing, truncated) of the ventricle, closed with a unit ball."""
    label_great_vessel, label_ventricle = _binary(label_great_vessel), _binary(label_ventricle)
    template_img = 0 * label_ventricle
    cb_size, cb_index = label_to_roi([label_great_vessel, label_ventricle], expansion_mm=(20, 20, 20))
    label_ventricle = crop_to_roi(label_ventricle, cb_size, cb_index)
    label_great_vessel = crop_to_roi(label_great_vessel, cb_size, cb_index)
    _, _, res_z = label_ventricle.GetSpacing()
    valve_thickness = int(valve_thickness_mm / res_z)
    check_dilate_radius((valve_thickness,) * 3, "generate_valve_from_great_vessel")
    label_ventricle_dilate = binary_dilate(label_ventricle, (valve_thickness,) * 3)
    overlap = label_great_vessel.tensor & label_ventricle_dilate.tensor
    mask = label_great_vessel.tensor | label_ventricle_dilate.tensor
    overlap = overlap * (mask != 0).to(torch.uint8)                       # sitk.Mask(overlap, mask)
    label_valve = binary_morphological_closing(label_ventricle.like(overlap), 1)
    return paste(template_img, label_valve, cb_index)


def generate_valve_using_cylinder(label_atrium, label_ventricle, radius_mm=15, height_mm=10):
    """Geometrically defined tricuspid / mitral valve (valve.py:85-180): a cylinder at the centre of mass of the region both
    dilated chambers share, turned so that its axis follows the line between the chambers' centres of mass.  The chambers
    are dilated by 1 mm, 2 mm, ... until they share more than 2000 mm^3."""
    label_atrium, label_ventricle = _binary(label_atrium), _binary(label_ventricle)
    template_img = 0 * label_ventricle
    cb_size, cb_index = label_to_roi([label_atrium, label_ventricle], expansion_mm=(20, 20, 20))
    label_atrium = crop_to_roi(label_atrium, cb_size, cb_index)
    label_ventricle = crop_to_roi(label_ventricle, cb_size, cb_index)
    dilation = 1
    overlap_vol = 0
    while overlap_vol <= 2000:
        dilation_img = [int(dilation / i) for i in label_ventricle.GetSpacing()]
        check_dilate_radius(dilation_img, "generate_valve_using_cylinder")
        overlap = label_ventricle.like(binary_dilate(label_atrium, dilation_img).tensor & binary_dilate(label_ventricle, dilation_img).tensor)
        overlap_vol = int(overlap.tensor.sum()) * np.prod(overlap.GetSpacing())
        dilation += 1
    valve_loc = get_com(overlap, as_int=True)
    valve_loc_real = get_com(overlap, real_coords=True)
    cylinder = insert_cylinder_image(0 * label_ventricle, radius_mm, height_mm, valve_loc[::-1])
    orientation_vector = np.array(get_com(label_ventricle, real_coords=True)) - np.array(get_com(label_atrium, real_coords=True))
    rotation_angle = vector_angle(orientation_vector, (0, 0, 1), smallest=False)
    rotation_axis = np.cross(orientation_vector, (0, 0, 1))
    label_valve = rotate_image(cylinder, rotation_centre=valve_loc_real, rotation_axis=rotation_axis,
                               rotation_angle_radians=rotation_angle, interpolation=sitkNearestNeighbor, default_value=0)
    return paste(template_img, label_valve, cb_index)
