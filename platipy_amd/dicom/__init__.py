"""RTSTRUCT contours to binary masks on the GPU (platipy/dicom/io/rtstruct_to_nifti.py:54-217; csrc/pp_contour.h), and binary
masks back to RTSTRUCT contours (platipy/dicom/io/nifti_to_rtstruct.py; csrc/pp_contour_trace.h; T1-T7 below).

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

Masks to contours.  The reference (nifti_to_rtstruct.py, convert_nifti) hands each mask to rt-utils, which traces it slice by
slice with OpenCV's findContours on the host; neither is installed where this is tested and parity with them is UNPINNED.
Here ONE extraction of pp_contour_trace_u8 traces all structures and slices, by these rules, chosen so that R3's fill of the
result gives the masks back byte for byte.  The deliberate differences to rt-utils / OpenCV: every border pixel is a vertex
(approximate_contours is off by default), hole contours run through the hole's own pixels so that the XOR of R5 restores the
mask, and no pinholes are cut to join a hole to its outer contour.
  T1   per structure and slice; a pixel is (x, y), x to the right, y down; foreground is any non-zero value.  A foreground
       pixel has a CRACK on each side (N, E, S, W) whose 4-neighbour is background or outside the slice.  A crack is directed
       with its own pixel on its right as displayed: N heads east, E south, S west, W north.
  T2   foreground is 8-connected, background 4-connected.  At a crack's head corner, with AL / AR the pixels ahead-left /
       ahead-right (outside the slice = background): AL foreground -> the crack of AL (left turn); else AR foreground -> the
       crack of AR (straight on); else the next side of the same pixel (right turn).  Every crack has one successor and one
       predecessor: the cracks form disjoint cycles, the LOOPS.
  T3   a loop's LEADER is its crack with the smallest key (y, x, side), N < E < S < W.  A leader on side N: the outer border of
       an 8-connected component; on side S: the border of a hole (a 4-connected background component that does not reach
       the slice's edge).  (The test restatement decides this by the sign of the enclosed area instead.)
  T4   the SIDE PIXEL of a crack is its own pixel on an outer loop, the background pixel across the crack on a hole loop.
  T5   walking a loop from its leader, each maximal cyclic run of equal side pixels is one vertex; the first vertex is the run
       that holds the leader, even when that run began before it; outer borders run clockwise as displayed, holes the other
       way; a single pixel gives one vertex; consecutive vertices are 8-adjacent; no vertex is dropped.
  T6   contours are ordered by (structure, z, leader key); vertices are int32 (x, y), rows {first, count, structure, z} as
       pp_contour_fill_u8 takes them, and a parallel uint8 array flags the holes.
  T7   approximate_contours=True (rt-utils' CHAIN_APPROX_SIMPLE): from a contour of more than two vertices every vertex whose
       incoming step equals its outgoing step is dropped (cyclic neighbours, all decided on the full sequence) and the contour
       starts at the first kept vertex at or after the T5 start.  LOSSY on parts one pixel wide: the spur a b c b a becomes
       a c a and R3 no longer sees b, so the fill of the result may miss pixels of the mask.
  T8   ROIDisplayColor: the reference colours a structure by hash(name) % 256, which differs from run to run; here a fixed
       palette indexed by the structure's position, or the caller's colours (deviation).
"""
import logging

import numpy as np
import torch

from .. import _lib, runtime
from ..image import Image, as_image

logger = logging.getLogger(__name__)

__all__ = ["contours_to_dicom_struct", "extract_contours", "fix_missing_data", "rasterise_contours", "transform_point_set_from_dicom_struct"]


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


def extract_contours(masks, approximate_contours=False, as_physical=True):
    """Closed planar contours of binary masks, the inverse of rasterise_contours (T1-T7).  masks: {name: Image}, scalar images
    on ONE grid (ValueError otherwise), foreground = any non-zero voxel.  -> {name: [points, ...]} in insertion order, every
    `points` a float64 [n, 3] array of physical points in mm, origin + direction diag(spacing) (x, y, z), one closed contour;
    within a structure the contours keep the order of T6 (slice, then leader); a structure without foreground maps to [].
    as_physical=False -> (int32 vertices [n, 2] of (x, y), CONTOUR_DTYPE rows, uint8 hole flags, names): the tables
    Context.contour_fill takes.  All structures and slices are traced by one extraction of pp_contour_trace_u8; with
    approximate_contours=False rasterise_contours of the result on the same grid gives the masks back."""
    names = list(masks)
    images = [as_image(masks[n]) for n in names]
    for name, img in zip(names, images):
        if img.is_vector:
            raise ValueError(f"extract_contours: {name} is a vector image")
        if not img.same_grid(images[0]):
            raise ValueError(f"extract_contours: {name} is not on the grid of {names[0]}")
    if not names:
        empty = np.zeros((0, 2), np.int32), np.zeros(0, _lib.CONTOUR_DTYPE), np.zeros(0, np.uint8), []
        return {} if as_physical else empty
    ref = images[0]
    nx, ny, nz = ref.GetSize()
    stack = torch.stack([i.tensor if i.tensor.dtype == torch.uint8 else (i.tensor != 0).to(torch.uint8) for i in images]).contiguous()
    verts, rows, hole = runtime.context(ref.device).contour_trace(stack, (nx, ny, nz), len(names), approximate_contours)
    if not as_physical:
        return verts, rows, hole, names
    index = np.empty((verts.shape[0], 3), dtype=np.float64)
    index[:, :2] = verts
    index[:, 2] = np.repeat(rows["z"], rows["count"])
    m = np.asarray(ref.GetDirection(), dtype=np.float64).reshape(3, 3) @ np.diag(np.asarray(ref.GetSpacing(), dtype=np.float64))
    points = index @ m.T + np.asarray(ref.GetOrigin(), dtype=np.float64)
    out = {name: [] for name in names}
    for first, count, s, _ in rows.tolist():
        out[names[s]].append(points[first:first + count])
    return out


# ROIDisplayColor by position (T8)
PALETTE = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 128, 0), (128, 255, 0),
           (0, 255, 128), (0, 128, 255), (128, 0, 255), (255, 0, 128), (255, 128, 128), (128, 255, 128), (128, 128, 255), (192, 192, 192))


def contours_to_dicom_struct(contours, colours=None):
    """{name: [points [n, 3] in mm, ...]} (what extract_contours returns) -> a tree of types.SimpleNamespace with the attributes
    of an RTSTRUCT that transform_point_set_from_dicom_struct reads -- StructureSetROISequence[*].ROINumber / .ROIName and
    ROIContourSequence[*].ReferencedROINumber / .ContourSequence[*].ContourGeometricType ("CLOSED_PLANAR") / .ContourData
    (flat x0, y0, z0, x1, ...) -- plus NumberOfContourPoints and ROIDisplayColor.  ROI numbers count from 1 in insertion
    order.  colours: {name: (r, g, b)} or a sequence by position; otherwise PALETTE by position (T8).  A user with pydicom
    copies these fields into a Dataset; writing files is not part of this module."""
    from types import SimpleNamespace

    rois, sequence = [], []
    for k, (name, polys) in enumerate(contours.items()):
        if colours is None:
            colour = PALETTE[k % len(PALETTE)]
        else:
            colour = colours[name] if isinstance(colours, dict) else colours[k]
        items = []
        for points in polys:
            p = np.asarray(points, dtype=np.float64)
            if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
                raise ValueError(f"a contour is an [n, 3] array of points with n >= 1, got shape {p.shape}")
            items.append(SimpleNamespace(ContourGeometricType="CLOSED_PLANAR", NumberOfContourPoints=int(p.shape[0]),
                                         ContourData=p.ravel().tolist()))
        rois.append(SimpleNamespace(ROINumber=k + 1, ROIName=str(name)))
        sequence.append(SimpleNamespace(ReferencedROINumber=k + 1, ROIDisplayColor=[int(c) for c in colour], ContourSequence=items))
    return SimpleNamespace(StructureSetROISequence=rois, ROIContourSequence=sequence)
