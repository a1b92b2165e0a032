"""Drop-in for platipy/imaging/utils/geometry.py:19-79: vector_angle (host arithmetic) and rotate_image (a
VersorRigid3DTransform through the existing resampling kernels)."""
import numpy as np

from ..image import as_image
from ..registration.utils import apply_transform
from ..transform import VersorRigid3DTransform, sitkNearestNeighbor


def vector_angle(v1, v2, smallest=True):
    """The angle between two vectors in radians; with `smallest` the direction is ignored (geometry.py:19-39)."""
    v1 = np.array(v1)
    v2 = np.array(v2)
    v1_norm = v1 / np.linalg.norm(v1)
    v2_norm = v2 / np.linalg.norm(v2)
    dot_product = np.dot(v1_norm, v2_norm)
    if smallest:
        dot_product = np.abs(dot_product)
    return np.arccos(dot_product)


def rotate_image(img, rotation_centre=(0, 0, 0), rotation_axis=(1, 0, 0), rotation_angle_radians=0,
                 interpolation=sitkNearestNeighbor, default_value=0):
    """Rotate an image about `rotation_centre` (physical coordinates) and resample it into its own space
    (geometry.py:42-79): sitk.Resample(img, VersorRigid3DTransform, interpolation, default_value, img.GetPixelID()).
    A zero-length axis raises ValueError."""
    img = as_image(img)
    rotation_transform = VersorRigid3DTransform()
    rotation_transform.SetCenter(rotation_centre)
    rotation_transform.SetRotation(rotation_axis, rotation_angle_radians)
    return apply_transform(img, img, rotation_transform, default_value, interpolation)
