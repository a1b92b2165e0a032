"""RTSTRUCT contours to binary masks on the GPU (platipy/dicom/io/rtstruct_to_nifti.py:54-217; csrc/pp_contour.h).

The reference loops over structures and contours, calls skimage.draw.polygon for each contour and XORs the result into a
slice.  Here the vertices of ALL structures are transformed to indices in one vectorised fp64 step on the host and all
structures and slices are filled by one call of pp_contour_fill_u8.  Reading DICOM files is not part of this module and
pydicom is never imported: `transform_point_set_from_dicom_struct` touches its dataset by attribute access only, so a
pydicom.Dataset works and so does a tree of types.SimpleNamespace; `rasterise_contours` takes plain arrays of points.

Parity with scikit-image and with the reference is UNPINNED: neither scikit-image nor SimpleITK is installed where this is
tested.  The tests hold the kernel byte for byte to a numpy fp64 restatement of the rule below, and that restatement to an
exact closed-polygon test on convex polygons and staircases.

What is kept of the reference, and what is not:
  R1   every vertex goes through TransformPhysicalPointToIndex: (direction diag(spacing))^-1 (point - origin) in fp64, every
       component rounded half up -- label.region.physical_point_to_index, vectorised.  Polygons have INTEGER vertices.
  R2   spacing_override[k] == 0 keeps component k, any other value replaces it (:117-125).  The reference writes the new
       spacing into the CALLER's image; here the caller's image is left alone (deviation) and only the returned masks carry
       the new spacing, as the reference's do.
  R3   a pixel is inside a contour by scikit-image's point_in_polygon [scikit-image upstream, _shared/geometry.pxd and
       draw/_draw.pyx, recalled, UNVERIFIED here].  With (u_i, v_i) = vertex - pixel, u along image y and v along image x
       (the reference passes x as r and y as c, and skimage tests (c, r)), walking the closed list with previous vertex 0 and
       current vertex 1: u1 == v1 == 0 -> in; (v1 > 0) != (v0 > 0) and (u1 v0 - u0 v1) / (v0 - v1) > 0 -> a right crossing;
       (v1 < 0) != (v0 < 0) and that quotient < 0 -> a left crossing; in when the right count is odd or the two parities
       differ.  For a simple polygon that is the closed polygon: interior, edges and vertices.
  R4   vertex indices are bounded at |index| <= 2^24 (ValueError beyond): every product of R3 then stays below 2^53, the
       reference's fp64 is exact, and the kernel decides the same signs in int64 without a division.
  R5   contours of one structure on one slice combine by XOR (:209): an inner contour cuts a hole, the same contour twice
       gives nothing.
  R6   a contour's slice is the rounded z of its FIRST vertex (:177); if any of its vertices rounds to another z the WHOLE
       structure is dropped and is absent from the output (:178-183, :211); a contour whose slice is outside [0, nz) is
       skipped alone (:190-200).
  R7   a structure is skipped when it has no entry in ROIContourSequence, no ContourSequence, an empty one, or a FIRST
       contour that is not CLOSED_PLANAR (:139-156); the type of the later contours is not looked at.
  R8   names are "_".join(ROIName.split()) (:135).
  R9   pixels are clipped to the true slice [0, nx) x [0, ny).  The reference passes shape = (ny, nx) to a call whose rows are
       x (:204-207): on a slice that is not square it truncates at the wrong extent or raises IndexError (deviation).
  R10  the reference's warning about the slice increment (:185-188) compares the x of the THIRD vertex, not a z; it is not
       reproduced.
  R11  fix_missing_data: one empty string in ContourData is repaired, x or y from the two neighbouring vertices of the
       closed contour, z from the other vertices.  The reference's own arithmetic there runs on an array of strings and its
       wrap-around for the last y reads past the end; this is the behaviour it describes, not its text.
"""
import logging

import numpy as np
import torch

from .. import _lib, runtime
from ..image import Image, as_image

logger = logging.getLogger(__name__)

__all__ = ["fix_missing_data", "rasterise_contours", "transform_point_set_from_dicom_struct"]


def fix_missing_data(contour_data):
    """ContourData (x0, y0, z0, x1, ...) with ONE missing value -- an empty string -- repaired (R11) -> float64 array.  A
    missing x or y becomes the mean of that component at the previous and the next vertex of the closed contour, a missing
    z the minimum of the other z.  Nothing missing: np.asarray(contour_data) as it is.  More than one value missing is
    not repaired and the data is returned unchanged (the conversion to numbers then fails, as in the reference)."""
    values = list(contour_data)
    missing = [i for i, v in enumerate(values) if isinstance(v, (str, bytes)) and len(v.strip()) == 0]
    if not missing:
        return np.asarray(contour_data)
    if len(missing) > 1:
        logger.debug("%d values missing in ContourData: not repaired", len(missing))
        return np.asarray(contour_data)
    k = missing[0]
    n = len(values)
    if n % 3 != 0:
        raise ValueError(f"fix_missing_data: ContourData of {n} values is not a list of (x, y, z)")
    values[k] = "nan"
    out = np.array(values, dtype=np.float64)
    if k % 3 == 2:
        out[k] = np.min(np.delete(out[2::3], k // 3)) if n > 3 else np.nan
    else:
        out[k] = 0.5 * (out[(k - 3) % n] + out[(k + 3) % n])
    if not np.isfinite(out[k]):
        raise ValueError("fix_missing_data: nothing to repair the missing value from")
    return out


def _override_spacing(spacing, spacing_override):
    if not spacing_override:
        return tuple(spacing)
    return tuple(float(spacing[k]) if spacing_override[k] == 0 else float(spacing_override[k]) for k in range(3))      # R2


def _points_to_index(points, spacing, origin, direction):
    """R1 for an [n, 3] array of physical points -> (int32 [n, 2] of (x, y), int64 [n] of z).  The three products of a
    component are summed left to right, as a plain loop would (component-major arrays: every pass is contiguous)."""
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    m = np.linalg.inv(d @ np.diag(np.asarray(spacing, dtype=np.float64)))
    rel = np.ascontiguousarray(points.T) - np.asarray(origin, dtype=np.float64)[:, None]
    xy = np.empty((points.shape[0], 2), dtype=np.int32)
    z = None
    for k in range(3):
        c = m[k, 0] * rel[0]
        c += m[k, 1] * rel[1]
        c += m[k, 2] * rel[2]
        c += 0.5
        np.floor(c, out=c)
        if c.size and not (np.abs(c).max() <= _lib.CONTOUR_MAX_INDEX):      # (also refuses NaN)
            raise ValueError("a contour vertex lies more than 2^24 voxels from the image origin (or is not finite)")      # R4
        if k < 2:
            xy[:, k] = c
        else:
            z = c.astype(np.int64)
    return xy, z


def _rasterise(reference_image, structures, spacing_override):
    """structures: (name, [points, ...]) pairs -> (uint8 tensor [S, Z, Y, X], names, spacing of the masks)."""
    ref = as_image(reference_image)
    spacing = _override_spacing(ref.GetSpacing(), spacing_override)
    nx, ny, nz = ref.GetSize()
    polys, owner = [], []
    structures = list(structures)
    for s, (_, contours) in enumerate(structures):
        for points in contours:
            p = np.asarray(points, dtype=np.float64)
            if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
                raise ValueError(f"a contour is an [n, 3] array of points with n >= 1, got shape {p.shape}")
            polys.append(p)
            owner.append(s)
    xy, zs = _points_to_index(np.concatenate(polys) if polys else np.zeros((0, 3)), spacing, ref.GetOrigin(), ref.GetDirection())
    count = np.array([len(p) for p in polys], dtype=np.int64)
    first = np.cumsum(count) - count
    owner = np.array(owner, dtype=np.int64)
    keep_structure = np.ones(len(structures), dtype=bool)
    if len(polys):
        z = zs[first]
        one_slice = (np.minimum.reduceat(zs, first) == z) & (np.maximum.reduceat(zs, first) == z)
        keep_structure[owner[~one_slice]] = False                            # R6: the whole structure
        rows = keep_structure[owner] & (z >= 0) & (z < nz)                   # R6: a contour outside the volume alone
    else:
        z, rows = first, np.zeros(0, dtype=bool)
    kept = np.flatnonzero(keep_structure)
    slot = np.cumsum(keep_structure) - 1
    table = np.zeros(int(rows.sum()), dtype=_lib.CONTOUR_DTYPE)
    table["first"], table["count"], table["structure"], table["z"] = first[rows], count[rows], slot[owner[rows]], z[rows]
    out = torch.empty((len(kept), nz, ny, nx), dtype=torch.uint8, device=ref.device)
    if len(kept):
        runtime.context(ref.device).contour_fill(xy, table, (nx, ny, nz), len(kept), out)
    return out, [structures[s][0] for s in kept], spacing


def rasterise_contours(reference_image, contours, spacing_override=None, as_dict=True):
    """Binary masks of closed planar contours on reference_image's grid.  contours: {name: [points, ...]}, every `points` an
    [n, 3] array (n >= 1) of physical points in mm, one closed contour.  -> {name: uint8 Image} in insertion order, or with
    as_dict=False (uint8 tensor [S, Z, Y, X], names).  All structures and slices are filled by one pp_contour_fill_u8 call.
    Semantics R1-R6, R9 of this module; a structure one of whose contours spans two slices is absent from the result (R6).
    The masks carry the spacing after spacing_override; reference_image itself is not changed (R2)."""
    ref = as_image(reference_image)
    out, names, spacing = _rasterise(ref, contours.items(), spacing_override)
    if not as_dict:
        return out, names
    return {name: Image(out[k], spacing, ref.GetOrigin(), ref.GetDirection()) for k, name in enumerate(names)}


def transform_point_set_from_dicom_struct(dicom_image, dicom_struct, spacing_override=None):
    """The reference's function (:105-217) -> (list of uint8 Images, list of names).  dicom_struct is read by attribute access
    only: StructureSetROISequence[*].ROIName / .ROINumber and ROIContourSequence[*].ReferencedROINumber /
    .ContourSequence[*].ContourGeometricType / .ContourData.  Structures are skipped by R7 and R6, named by R8."""
    ref = as_image(dicom_image)
    by_number = {cs.ReferencedROINumber: cs for cs in dicom_struct.ROIContourSequence}
    structures = []
    for roi in dicom_struct.StructureSetROISequence:
        name = "_".join(roi.ROIName.split())      # R8
        cs = by_number.get(roi.ROINumber)
        if cs is None:
            logger.debug("%s: no ROIContourSequence entry, skipped", name)
            continue
        sequence = getattr(cs, "ContourSequence", None)
        if sequence is None or len(sequence) == 0:
            logger.debug("%s: no contours, skipped", name)
            continue
        if sequence[0].ContourGeometricType != "CLOSED_PLANAR":
            logger.debug("%s: not a closed planar structure, skipped", name)
            continue
        structures.append((name, [np.array(fix_missing_data(c.ContourData), dtype=np.float64).reshape(-1, 3) for c in sequence]))
    out, names, spacing = _rasterise(ref, structures, spacing_override)
    return [Image(out[k], spacing, ref.GetOrigin(), ref.GetDirection()) for k in range(len(names))], names
