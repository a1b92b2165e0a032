"""Drop-in for platipy/imaging/utils/vessel.py:33-436 (vessel splining) without VTK.

The two volume-sized steps are HIP kernels (csrc/pp_vessel.h): the per-slice moments of every atlas's propagated label
(pp_slice_moments_u8) and the voxelisation of a tube of fixed radius around the splined centreline (pp_tube_mask_u8).  The
arithmetic between them -- a few hundred centres of mass, one tridiagonal solve -- runs on the host in fp64.

DEVIATION.  The reference builds the tube with VTK (vtkParametricSpline, vtkTubeFilter with 50 sides,
vtkPolyDataToImageStencil with tolerance 0.5).  VTK is not a dependency here: tube_from_com_list returns the centreline
samples where the reference returns a vtkTubeFilter, and simpleitk_image_from_vtk_tube marks the voxels whose centre lies
within the radius of that polyline, with flat ends.  Parity with VTK's voxelisation is UNPINNED, like the rest of this
build's parity with SimpleITK.

Quirks of the reference that are kept:
  V1  a slice survives only if BOTH mean centre-of-mass components are finite and > 0 (vessel.py:97-98, :159-160): a vessel
      whose centre sits in row or column 0 of a slice loses that slice.
  V2  the centre of mass is truncated with int(), not rounded (:101, :163).
  V3  np.nanmean over the atlases, in list order; the "count" / "area" condition multiplies the mean by a boolean, so a
      failing slice becomes 0 (dropped by V1), and NaN * False stays NaN (dropped as not finite) (:74-91, :135-152).
  V4  the labels are weighted by their own value (a 0 / 255 mask weighs 255 in the "area" sum) (:60-63, :121-124).
  V5  an unknown scan direction ("y") falls through both branches and returns None, which crashes later; here it raises
      ValueError.  An invalid condition type raises ValueError for both directions (the z branch calls quit(), :154-155).
  V6  vessel_spline_generation forces the direction of the atlas labels to identity while it works and restores it
      (:389-434), and takes the first atlas's label as the reference grid.
"""
import logging
import warnings

import numpy as np
import torch

from .. import runtime
from ..image import as_image
from ..label.utils import slice_moments

logger = logging.getLogger(__name__)


class Tube(np.ndarray):
    """The centreline samples [n, 3] (mm, fp64) with the tube's `radius`: what stands in for the reference's vtkTubeFilter."""

    def __new__(cls, points, radius):
        obj = np.asarray(points, dtype=np.float64).reshape(-1, 3).view(cls)
        obj.radius = float(radius)
        return obj

    def __array_finalize__(self, obj):
        self.radius = getattr(obj, "radius", None)


def com_from_moments(moments, reference_image, condition_type="count", condition_value=0, scan_direction="z"):
    """com_from_image_list's host arithmetic on the int64 table [atlases, slices, 4] of label.utils.slice_moments (atlases in
    list order): the mean centre of mass per slice and the surviving points in physical space.  fp64 on exact integers, so
    every process that holds the same table computes the same bits."""
    scan = str(scan_direction).lower()
    if scan not in ("x", "z"):
        raise ValueError(f"scan direction must be 'x' or 'z', got {scan_direction!r}")
    cond = str(condition_type).lower()
    if cond not in ("area", "count"):
        raise ValueError("Invalid condition type, please select from 'area' or 'count'.")
    m = np.asarray(moments, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        weights = 1.0 * m[:, :, 0]
        com_a = 1.0 * m[:, :, 1] / weights
        com_b = 1.0 * m[:, :, 2] / weights
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        mean_a = np.nanmean(com_a, axis=0)
        mean_b = np.nanmean(com_b, axis=0)
        if cond == "area":
            keep = np.sum(m[:, :, 0], axis=0) > condition_value
        else:
            keep = np.sum(m[:, :, 3] > 0, axis=0) > condition_value
        mean_com = np.dstack((mean_a, mean_b))[0] * np.array((keep,) * 2).T
    reference_image = as_image(reference_image)
    d = np.asarray(reference_image.direction, dtype=np.float64).reshape(3, 3)
    sp = np.asarray(reference_image.spacing, dtype=np.float64)
    org = np.asarray(reference_image.origin, dtype=np.float64)
    point_array = []
    for index, com in enumerate(mean_com):
        if np.all(np.isfinite(com)) and np.all(com > 0):       # V1
            if scan == "x":
                idx = (index, int(com[1]), int(com[0]))         # V2; com = (array z, array y)
            else:
                idx = (int(com[1]), int(com[0]), index)         # com = (row = image y, column = image x)
            point_array.append(tuple(float(v) for v in org + d @ (sp * np.array(idx, dtype=np.float64))))
    return point_array


def com_from_image_list(sitk_image_list, condition_type="count", condition_value=0, scan_direction="z"):
    """Mean centre-of-mass positions of a list of labels, slice by slice along `scan_direction` ("x" sagittal, "z" axial), in
    physical space (vessel.py:33-167).  A slice counts when more than `condition_value` labels are present in it ("count") or
    their summed weight exceeds it ("area")."""
    images = [as_image(i) for i in sitk_image_list]
    if str(scan_direction).lower() not in ("x", "z"):
        raise ValueError(f"scan direction must be 'x' or 'z', got {scan_direction!r}")     # V5
    return com_from_moments(slice_moments(images, scan_direction), images[0], condition_type, condition_value, scan_direction)


def _clamped_cubic_spline(t, y, u):
    """The cubic spline through (t_i, y_i) with zero first derivative at both ends, at the parameters u (fp64, host)."""
    n = len(t)
    h = np.diff(t)
    A = np.zeros((n, n))
    rhs = np.zeros((n,) + y.shape[1:])
    slope = np.diff(y, axis=0) / h[:, None]
    A[0, 0], A[0, 1] = 2.0 * h[0], h[0]
    rhs[0] = 6.0 * slope[0]
    for i in range(1, n - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
        rhs[i] = 6.0 * (slope[i] - slope[i - 1])
    A[n - 1, n - 2], A[n - 1, n - 1] = h[n - 2], 2.0 * h[n - 2]
    rhs[n - 1] = -6.0 * slope[n - 2]
    M = np.linalg.solve(A, rhs)
    k = np.clip(np.searchsorted(t, u, side="right") - 1, 0, n - 2)
    hk = h[k][:, None]
    a = (t[k + 1] - u)[:, None]
    b = (u - t[k])[:, None]
    return (M[k] * a ** 3 + M[k + 1] * b ** 3) / (6.0 * hk) + (y[k] / hk - M[k] * hk / 6.0) * a + (y[k + 1] / hk - M[k + 1] * hk / 6.0) * b


def tube_from_com_list(com_list, radius):
    """The splined centreline of a tube through the points `com_list` (mm): a Tube, i.e. a (10 N + 1, 3) fp64 array of samples
    with the radius attached, where the reference returns a vtkTubeFilter (vessel.py:170-214) -- a stated deviation.

    The spline is cubic in each coordinate, parameterised by normalised cumulative chord length, with zero first derivative
    at both ends, sampled at 10 N + 1 uniform parameters (SetUResolution(10 N)).  These are the defaults of
    vtkParametricSpline / vtkCardinalSpline (ParameterizeByLength on, not closed, left / right constraint 1 with value 0) AS
    RECALLED FROM UPSTREAM, UNVERIFIED HERE: no VTK is available to check them against.  Consecutive duplicate points are
    dropped before the fit (their chord length is zero); fewer than two distinct points come back as they are."""
    pts = np.asarray(com_list, dtype=np.float64).reshape(-1, 3)
    if len(pts) > 1:
        keep = np.concatenate(([True], np.any(np.diff(pts, axis=0) != 0.0, axis=1)))
        pts = pts[keep]
    n = len(pts)
    if n < 2:
        return Tube(pts, radius)
    chord = np.sqrt((np.diff(pts, axis=0) ** 2).sum(axis=1))
    t = np.concatenate(([0.0], np.cumsum(chord)))
    t /= t[-1]
    t[-1] = 1.0
    u = np.arange(10 * n + 1, dtype=np.float64) / (10 * n)
    return Tube(_clamped_cubic_spline(t, pts, u), radius)


def simpleitk_image_from_vtk_tube(tube, sitk_reference_image):
    """Binary image (0 / 1, uint8) of the voxels of `sitk_reference_image`'s grid within tube.radius of the centreline `tube`
    (vessel.py:235-296; pp_tube_mask_u8, flat ends).  The grid's direction is taken as identity, as the reference's VTK
    image has none.  Fewer than two points: an empty mask and a warning."""
    ref = as_image(sitk_reference_image)
    out = torch.zeros(ref.shape, dtype=torch.uint8, device=ref.device)
    pts = np.asarray(tube, dtype=np.float64).reshape(-1, 3)
    if len(pts) < 2 or not np.any(np.diff(pts, axis=0) != 0.0):
        logger.warning("Fewer than two centreline points (%d): the vessel mask is empty", len(pts))
        return ref.like(out)
    runtime.context(ref.device).tube_mask(pts, ref.GetSize(), ref.GetSpacing(), ref.GetOrigin(), tube.radius, out)
    return ref.like(out)


def vessel_spline_generation(reference_image, atlas_set, vessel_name_list, vessel_radius_mm_dict, stop_condition_type_dict,
                             stop_condition_value_dict, scan_direction_dict, atlas_label="DIR"):
    """Generates a splined vessel from the atlases' propagated labels (vessel.py:336-436): atlas_set is
    {atlas_id: {atlas_label: {structure: Image}}}; returns {vessel name: binary Image}."""
    splined_vessels = {}
    if isinstance(vessel_name_list, str):
        vessel_name_list = [vessel_name_list]
    for vessel_name in vessel_name_list:
        initial_image_direction = as_image(reference_image).GetDirection()
        image_list = []
        for i in atlas_set.keys():
            try:
                image_list.append(as_image(atlas_set[i][atlas_label][vessel_name]))
            except (KeyError, TypeError):
                logger.warning("No match for ID=%s, label=%s, vessel=%s", i, atlas_label, vessel_name)
        if len(image_list) == 0:
            logger.warning("No structures found for vessel with name %s!", vessel_name)
            continue
        saved = [im.GetDirection() for im in image_list]
        for im in image_list:                                   # V6
            im.SetDirection((1, 0, 0, 0, 1, 0, 0, 0, 1))
        try:
            point_array = com_from_image_list(image_list, condition_type=stop_condition_type_dict[vessel_name],
                                              condition_value=stop_condition_value_dict[vessel_name],
                                              scan_direction=scan_direction_dict[vessel_name])
            tube = tube_from_com_list(point_array, radius=vessel_radius_mm_dict[vessel_name])
            reference_image = image_list[0]
            vessel_delineation = simpleitk_image_from_vtk_tube(tube, reference_image)
            vessel_delineation.SetDirection(initial_image_direction)
            splined_vessels[vessel_name] = vessel_delineation
        finally:
            for im, d in zip(image_list, saved):
                im.SetDirection(d)
    return splined_vessels
