"""Drop-in for platipy/imaging/generation/image.py:19-137: spheres and cylinders drawn into an array or an Image, as
elementwise torch on the device the data lives on.  Every comparison is made in fp64 on the expressions the reference
writes, in its order, so the voxels set are the ones numpy sets.

The reference's conventions are kept, and they are not uniform:
  * insert_sphere reads `sp_centre` and a vector `sp_radius` in ARRAY order (axis 0 = image z, 1 = y, 2 = x);
  * insert_cylinder names the array axes x, y, z = np.indices(arr.shape) and then takes the radial distance from z (array
    axis 2, image x) with cyl_centre[0] / cyl_radius[0] and y (array axis 1) with cyl_centre[1] / cyl_radius[1], the height
    along its "x" (array axis 0, image z) with cyl_centre[2]: the centre is in IMAGE order (x, y, z) and the cylinder's axis
    is the image z axis;
  * both write into the array they are given (`arr_copy = arr[:]` is a view, not a copy) and return it.  The *_image
    functions work on a copy of the image's voxels, as sitk.GetArrayFromImage makes one.
"""
import numpy as np
import torch

from ..image import as_image


def _axis(n, axis, device):
    shape = [1, 1, 1]
    shape[axis] = n
    return torch.arange(n, dtype=torch.float64, device=device).reshape(shape)


def _as_tensor(arr):
    if isinstance(arr, np.ndarray):
        from .. import runtime

        return torch.from_numpy(arr).to(runtime.default_device()), True
    return arr, False


def _scalar(v, device):
    """A divisor as a 0-dim fp64 tensor ON THE DEVICE: torch divides a device tensor by a Python number by multiplying with its
    reciprocal, which is not numpy's correctly rounded quotient (it moves voxels that lie exactly on the surface)."""
    return torch.tensor(float(v), dtype=torch.float64, device=device)


def _sphere_mask(shape, device, radius, centre):
    x, y, z = (_axis(shape[k], k, device) for k in range(3))
    rx, ry, rz = (_scalar(r, device) for r in radius)
    return (((x - float(centre[0])) / rx) ** 2.0 + ((y - float(centre[1])) / ry) ** 2.0 + ((z - float(centre[2])) / rz) ** 2.0) <= 1


def _cylinder_mask(shape, device, radius, height, centre):
    x, y, z = (_axis(shape[k], k, device) for k in range(3))
    radial = (((z - float(centre[0])) / _scalar(radius[0], device)) ** 2 + ((y - float(centre[1])) / _scalar(radius[1], device)) ** 2) <= 1
    along = torch.abs((x - float(centre[2])) / _scalar(0.5 * float(height), device)) <= 1
    return radial & along


def insert_sphere(arr, sp_radius=4, sp_centre=(0, 0, 0)):
    """Set the voxels of `arr` (a torch tensor, or a numpy array) inside the ellipsoid to 1 (generation/image.py:19-48)."""
    t, was_numpy = _as_tensor(arr)
    if not hasattr(sp_radius, "__iter__"):
        sp_radius = [sp_radius] * 3
    t[_sphere_mask(tuple(t.shape), t.device, sp_radius, sp_centre)] = 1
    if was_numpy:
        arr[...] = t.cpu().numpy()
        return arr
    return t


def insert_cylinder(arr, cyl_radius=4, cyl_height=2, cyl_centre=(0, 0, 0)):
    """Set the voxels of `arr` inside the cylinder to 1; vertical extent +/- 0.5 * height (generation/image.py:51-79)."""
    t, was_numpy = _as_tensor(arr)
    if not hasattr(cyl_radius, "__iter__"):
        cyl_radius = [cyl_radius] * 2
    t[_cylinder_mask(tuple(t.shape), t.device, cyl_radius, cyl_height, cyl_centre)] = 1
    if was_numpy:
        arr[...] = t.cpu().numpy()
        return arr
    return t


def insert_sphere_image(image, sp_radius, sp_centre):
    """A sphere of `sp_radius` mm into a copy of `image` (generation/image.py:82-108); centre in array order (z, y, x)."""
    image = as_image(image)
    if not hasattr(sp_radius, "__iter__"):
        sp_radius = [sp_radius] * 3
    sp_radius_image = [i / j for i, j in zip(sp_radius, image.GetSpacing()[::-1])]
    return image.like(insert_sphere(image.tensor.clone(), sp_radius_image, sp_centre))


def insert_cylinder_image(image, cyl_radius=(5, 5), cyl_height=10, cyl_centre=(0, 0, 0)):
    """A cylinder along image z into a copy of `image`, sizes in mm, centre in image order (generation/image.py:111-137)."""
    image = as_image(image)
    if not hasattr(cyl_radius, "__iter__"):
        cyl_radius = [cyl_radius] * 2
    cyl_radius_image = [i / j for i, j in zip(cyl_radius, image.GetSpacing()[1::-1])]
    cyl_height_image = cyl_height / image.GetSpacing()[2]
    return image.like(insert_cylinder(image.tensor.clone(), cyl_radius_image, cyl_height_image, cyl_centre))
