"""Landmark-based quality assurance of a deformable registration: 3-D SIFT keypoints in two images, their matches, points
carried through a transform and the target registration error.  The reference's tool for this is the DIR QA service
(services/dirqa/service.py): crop both images to a contour's bounding box, clamp to an intensity window, `plastimatch sift`,
drop the matches outside the contour, return the two point lists.  `dir_qa` is that service without files, DataObjects or a
subprocess.

Neither plastimatch nor ITK's SIFT filter is available where this was written: parity with them is UNPINNED.  The semantics
are the numbered rules S1 ... S7 of csrc/pp_sift.h, THIS BUILD'S DECISIONS unless marked recalled, and the
rules of this file:

S2  scale space.  With `isotropic_voxel_size_mm` the image is first resampled by smooth_and_resample; otherwise the native grid
    is used.  sigma0_mm defaults to 1.6 max(spacing).  An octave holds intervals + 3 Gaussian images at
    sigma_o 2^(s / intervals), sigma_o = sigma0 2^octave.  The first image of octave 0 is discrete_gaussian(image, sigma0^2)
    (the input counts as unblurred); every other image of an octave is discrete_gaussian(first image,
    sigma_s^2 - sigma_o^2), variances in mm^2, maximum error BLUR_MAX_ERROR, kernel width blur_kernel_width(); the next
    octave starts from the image at 2 sigma_o taking every second voxel from index 0 (spacing doubled, origin kept).  Octaves
    stop early when an axis would drop below MIN_OCTAVE_AXIS voxels.
S8  points.  A keypoint's physical point is origin + direction (spacing_octave (index + offset)): the image's own frame.  The
    service's sign flip of two columns undoes plastimatch's output convention (LPS against RAS) and has no counterpart here.
S9  transform_points maps as the resampler maps, fixed-space point to moving-space point: a CompositeTransform applies its
    LAST member first (apply_transform's order), linear members in fp64 on the host, a displacement field through
    pp_transform_points_f64 (zero displacement outside the field), a B-spline through its dense evaluation on `reference`.
S10 dir_qa names a pair f"{name}_{i}", i = its number among the matches BEFORE the contour filter (the service names, then
    filters); a point is inside a contour when the voxel nearest to it (TransformPhysicalPointToIndex: round half away from
    the continuous index) on the cropped mask is non-zero.
"""
from dataclasses import dataclass

import numpy as np
import torch

from .. import runtime
from ..image import Image, as_image
from ..transform import BSplineTransform, CompositeTransform, DisplacementFieldTransform, Transform, sitkNearestNeighbor
from ..utils.crop import crop_to_roi, label_to_roi
from .utils import apply_transform, smooth_and_resample

DIRQA_SETTINGS_DEFAULTS = {
    "includePointsMode": "CONTOUR",  # "CONTOUR" or "BOUNDINGBOX"
    "intensityRange": [-1024, -200],  # Range: low to high
    "contrastThreshold": 0.03,  # Param for plastimatch
    "curvatureThreshold": 172.3,  # Param for plastimatch
}

DESCRIPTOR_LENGTH = 768
BLUR_MAX_ERROR = 0.01
MIN_OCTAVE_AXIS = 8
MAX_INTERVALS = 5             # SF_MAX_LEVELS - 3 of csrc/pp_sift.h
_FIRST_CAPACITY = 4096


@dataclass
class Keypoints:
    """points: float64 [n, 3] physical mm (x, y, z) in the image's frame; index: int32 [n, 3] (x, y, z) on the octave grid;
    octave, level: int32 [n]; sigma_mm, response: float64 [n]; offset: float64 [n, 3] (the Newton step, index units);
    descriptors: fp32 [n, 768] left on the device; count: the keypoints found (more than n when max_keypoints cut the list)."""
    points: np.ndarray
    index: np.ndarray
    octave: np.ndarray
    level: np.ndarray
    sigma_mm: np.ndarray
    response: np.ndarray
    offset: np.ndarray
    descriptors: torch.Tensor
    count: int

    def __len__(self):
        return int(self.points.shape[0])

    def take(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        sel = torch.as_tensor(rows, device=self.descriptors.device)
        return Keypoints(self.points[rows], self.index[rows], self.octave[rows], self.level[rows], self.sigma_mm[rows], self.response[rows],
                         self.offset[rows], self.descriptors.index_select(0, sel), len(rows))


@dataclass
class PointTable:
    """The content of one of the service's match files: names[i] and points[i] = (x, y, z) in mm."""
    names: list
    points: np.ndarray

    def __len__(self):
        return len(self.names)

    def rows(self):
        return [(n, float(p[0]), float(p[1]), float(p[2])) for n, p in zip(self.names, self.points)]


def blur_kernel_width(sigma_mm, spacing):
    """maximum_kernel_width for a blur of sigma_mm on `spacing`: room for five standard deviations on the finest axis."""
    return int(min(255, max(32, 2 * int(np.ceil(5.0 * float(sigma_mm) / min(spacing))) + 1)))


def scale_space(image, octaves=3, intervals=3, sigma0_mm=None):
    """S2 -> list of octaves, each a dict: stack (fp32 tensor [intervals + 3, Z, Y, X]), spacing, origin, direction, size
    (x, y, z), sigmas (mm, one per level), blurs ((variance mm^2, kernel width) per level, from the octave's first image)."""
    image = as_image(image)
    if image.is_vector:
        raise ValueError("sift: a scalar image is expected")
    intervals, octaves = int(intervals), int(octaves)
    if not 1 <= intervals <= MAX_INTERVALS or octaves < 1:
        raise ValueError(f"sift: intervals must be 1 ... {MAX_INTERVALS} and octaves at least 1")
    ctx = runtime.context(image.device)
    sigma0 = 1.6 * max(image.spacing) if sigma0_mm is None else float(sigma0_mm)
    if not sigma0 > 0.0:
        raise ValueError("sift: sigma0_mm must be positive")
    src = (image.tensor if image.tensor.dtype == torch.float32 else image.tensor.float()).contiguous()
    spacing = tuple(image.spacing)
    nlev = intervals + 3
    out, first = [], None
    for o in range(octaves):
        size = (int(src.shape[2]), int(src.shape[1]), int(src.shape[0]))
        sigma_o = sigma0 * 2.0 ** o
        sigmas = [sigma_o * 2.0 ** (s / intervals) for s in range(nlev)]
        stack = torch.empty((nlev,) + tuple(src.shape), dtype=torch.float32, device=src.device)
        blurs = []
        if o == 0:
            blurs.append((sigma_o ** 2, blur_kernel_width(sigma_o, spacing)))
            ctx.discrete_gaussian(src, stack[0], size, spacing, [blurs[0][0]] * 3, BLUR_MAX_ERROR, blurs[0][1], True)
        else:
            blurs.append((0.0, 0))
            stack[0].copy_(first)
        for s in range(1, nlev):
            var = sigmas[s] ** 2 - sigma_o ** 2
            width = blur_kernel_width(np.sqrt(var), spacing)
            blurs.append((var, width))
            ctx.discrete_gaussian(stack[0], stack[s], size, spacing, [var] * 3, BLUR_MAX_ERROR, width, True)
        out.append({"stack": stack, "spacing": spacing, "origin": tuple(image.origin), "direction": tuple(image.direction), "size": size,
                    "sigmas": sigmas, "blurs": blurs})
        nxt = tuple((n + 1) // 2 for n in size)
        if min(nxt) < MIN_OCTAVE_AXIS:
            break
        first = stack[intervals][::2, ::2, ::2].contiguous()
        src = first
        spacing = tuple(2.0 * s for s in spacing)
    return out


def _physical(index, origin, spacing, direction):
    D = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    return np.asarray(origin, dtype=np.float64)[None, :] + (np.asarray(index, dtype=np.float64) * np.asarray(spacing, dtype=np.float64)[None, :]) @ D.T


def _nearest_voxel(points, image):
    """TransformPhysicalPointToIndex for a list of points -> (int64 [n, 3] x, y, z, inside the buffer [n])."""
    D = np.asarray(image.direction, dtype=np.float64).reshape(3, 3) * np.asarray(image.spacing, dtype=np.float64)[None, :]
    c = np.linalg.solve(D, (np.asarray(points, dtype=np.float64).reshape(-1, 3) - np.asarray(image.origin, dtype=np.float64)).T).T
    idx = np.floor(c + 0.5).astype(np.int64)
    inside = np.all((idx >= 0) & (idx < np.asarray(image.GetSize())[None, :]), axis=1)
    return idx, inside


def points_in_mask(points, mask):
    """bool [n]: the voxel of `mask` nearest to each physical point is non-zero (outside the buffer: False)."""
    mask = as_image(mask)
    idx, inside = _nearest_voxel(points, mask)
    m = mask.numpy() != 0
    out = np.zeros(len(idx), dtype=bool)
    sel = np.flatnonzero(inside)
    out[sel] = m[idx[sel, 2], idx[sel, 1], idx[sel, 0]]
    return out


def sift_keypoints(image, mask=None, intensity_range=None, contrast_threshold=0.03, curvature_threshold=172.3, octaves=3, intervals=3,
                   sigma0_mm=None, isotropic_voxel_size_mm=None, max_keypoints=None):
    """3-D SIFT keypoints of a scalar image -> Keypoints, in ascending (octave, level, z, y, x) (S5).

    intensity_range (lo, hi): the window the contrast threshold is normalised by (S1), the image's minimum and maximum without
    one; the image is NOT clamped here.  mask: an Image; keypoints whose nearest mask voxel is zero are dropped.  max_keypoints:
    stop after that many (in the order above; .count still says how many there are).  The extremum search and the descriptors
    are pp_dog_extrema_f32 and pp_sift_describe_f32; the Gaussian images come from the existing discrete_gaussian passes."""
    image = as_image(image)
    if isotropic_voxel_size_mm:
        image = smooth_and_resample(image, isotropic_voxel_size_mm=float(isotropic_voxel_size_mm))
    ctx = runtime.context(image.device)
    src = (image.tensor if image.tensor.dtype == torch.float32 else image.tensor.float()).contiguous()
    if intensity_range is not None:
        lo, hi = float(intensity_range[0]), float(intensity_range[1])
    else:
        lo, hi = ctx.minmax(src, src.numel())
    if not hi > lo:
        raise ValueError("sift_keypoints: the intensity range is empty (a constant image has no keypoints to normalise)")
    limit = None if max_keypoints is None else max(int(max_keypoints), 0)
    parts, total = [], 0
    for o, octave in enumerate(scale_space(Image(src, image.spacing, image.origin, image.direction), octaves, intervals, sigma0_mm)):
        stack, size, nlev = octave["stack"], octave["size"], int(octave["stack"].shape[0])
        room = None if limit is None else max(limit - sum(len(p["index"]) for p in parts), 0)
        cap = _FIRST_CAPACITY if room is None else min(_FIRST_CAPACITY, room)
        count, index, values = ctx.dog_extrema(stack, size, nlev, hi - lo, contrast_threshold, curvature_threshold, cap)
        want = count if room is None else min(count, room)
        if want > len(index):       # (S5: the true count came back with the first rows; call again with room)
            count, index, values = ctx.dog_extrema(stack, size, nlev, hi - lo, contrast_threshold, curvature_threshold, want)
        total += count
        pts = _physical(index[:, :3].astype(np.float64) + values[:, :3], octave["origin"], octave["spacing"], octave["direction"])
        keep = np.ones(len(index), dtype=bool) if mask is None else points_in_mask(pts, mask)
        index, values, pts = index[keep], values[keep], pts[keep]
        desc = torch.empty((len(index), DESCRIPTOR_LENGTH), dtype=torch.float32, device=src.device)
        if len(index):
            ctx.sift_describe(stack, size, nlev, octave["spacing"], index, desc)
        parts.append({"index": index, "values": values, "points": pts, "octave": np.full(len(index), o, np.int32),
                      "sigma": np.asarray(octave["sigmas"], dtype=np.float64)[index[:, 3]], "desc": desc})
    cat = lambda k, empty: np.concatenate([p[k] for p in parts]) if parts else empty  # noqa: E731
    index, values = cat("index", np.zeros((0, 4), np.int32)), cat("values", np.zeros((0, 4)))
    desc = torch.cat([p["desc"] for p in parts]) if parts else torch.empty((0, DESCRIPTOR_LENGTH), dtype=torch.float32, device=src.device)
    return Keypoints(points=cat("points", np.zeros((0, 3))), index=np.ascontiguousarray(index[:, :3]), octave=cat("octave", np.zeros(0, np.int32)),
                     level=np.ascontiguousarray(index[:, 3]), sigma_mm=cat("sigma", np.zeros(0)), response=np.ascontiguousarray(values[:, 3]),
                     offset=np.ascontiguousarray(values[:, :3]), descriptors=desc, count=total)


def _nearest(ctx, a, b, pa, pb, radius):
    na, nb = int(a.shape[0]), int(b.shape[0])
    dev = a.device
    idx = torch.empty(na, dtype=torch.int32, device=dev)
    best, second = torch.empty(na, dtype=torch.float32, device=dev), torch.empty(na, dtype=torch.float32, device=dev)
    ctx.descriptor_match(a, na, b, nb, int(a.shape[1]), idx, best, second, pa, pb, 0.0 if radius is None else float(radius))
    ctx.sync()
    return idx.cpu().numpy(), best.cpu().numpy().astype(np.float64), second.cpu().numpy().astype(np.float64)


def match_keypoints(a, b, ratio=0.8, mutual=True, search_radius_mm=None):
    """Match two Keypoints lists by their descriptors (S7) -> (pairs int64 [m, 2] = rows of a and b, distances float64 [m, 2] =
    best and second-best squared distance of the row of a), rows of a ascending.  A row of a is accepted when
    best < ratio^2 second (compared in fp64 on the kernel's fp32 distances); `mutual` also requires the same of its partner
    towards it.  search_radius_mm: only keypoints of b within that distance (physical points) take part, and the reverse."""
    da, db = a.descriptors.contiguous(), b.descriptors.contiguous()
    if da.shape[0] == 0 or db.shape[0] == 0:
        return np.zeros((0, 2), np.int64), np.zeros((0, 2), np.float64)
    if da.shape[1] != db.shape[1] or da.device != db.device:
        raise ValueError("match_keypoints: the two descriptor tables differ in length or device")
    ctx = runtime.context(da.device)
    pa = pb = None
    if search_radius_mm is not None:
        pa = torch.from_numpy(np.ascontiguousarray(a.points, dtype=np.float64)).to(da.device)
        pb = torch.from_numpy(np.ascontiguousarray(b.points, dtype=np.float64)).to(da.device)
    ia, ba, sa = _nearest(ctx, da, db, pa, pb, search_radius_mm)
    ok = (ia >= 0) & (ba < float(ratio) ** 2 * sa)
    if mutual:
        ib, bb, sb = _nearest(ctx, db, da, pb, pa, search_radius_mm)
        okb = (ib >= 0) & (bb < float(ratio) ** 2 * sb)
        partner = np.where(ia >= 0, ia, 0)
        ok &= okb[partner] & (ib[partner] == np.arange(len(ia)))
    rows = np.flatnonzero(ok)
    return np.stack([rows, ia[rows].astype(np.int64)], axis=1).reshape(-1, 2), np.stack([ba[rows], sa[rows]], axis=1).reshape(-1, 2)


def transform_points(points, transform, reference=None):
    """Physical points [n, 3] through anything apply_transform takes (S9), fixed space to moving space -> float64 [n, 3].
    A BSplineTransform member needs `reference`, the grid it is evaluated on (as inverse_transform does); without one it
    raises ValueError."""
    p = np.array(points, dtype=np.float64).reshape(-1, 3)
    if transform is None:
        return p
    parts = transform.flatten() if isinstance(transform, CompositeTransform) else [transform]
    for part in reversed(parts):        # the LAST member is applied first
        if type(part) is Transform:
            continue
        if isinstance(part, BSplineTransform):
            if reference is None:
                raise ValueError("transform_points: a BSplineTransform needs a reference image to be evaluated on")
            ref = as_image(reference)
            part = DisplacementFieldTransform(Image(part.displacement_field(ref), ref.spacing, ref.origin, ref.direction, True))
        if isinstance(part, DisplacementFieldTransform):
            field = part.field
            f = (field.tensor if field.tensor.dtype == torch.float32 else field.tensor.float()).contiguous()
            if len(p):
                p = runtime.context(f.device).transform_points(f, field.geom(), p)
            continue
        A, off = part.matrix_offset()
        p = p @ np.asarray(A, dtype=np.float64).T + np.asarray(off, dtype=np.float64)[None, :]
    return p


def target_registration_error(points_fixed, points_moving, transform=None, reference=None):
    """|T(points_fixed) - points_moving| per pair in mm and {"mean", "median", "p95", "max", "n"} of them; transform=None is
    the error before registration.  No pairs: n = 0 and NaN statistics."""
    pf = np.asarray(points_fixed, dtype=np.float64).reshape(-1, 3)
    pm = np.asarray(points_moving, dtype=np.float64).reshape(-1, 3)
    if pf.shape != pm.shape:
        raise ValueError("target_registration_error: the two point lists differ in length")
    d = np.sqrt(((transform_points(pf, transform, reference) - pm) ** 2).sum(axis=1))
    if d.size == 0:
        return d, {"mean": float("nan"), "median": float("nan"), "p95": float("nan"), "max": float("nan"), "n": 0}
    return d, {"mean": float(d.mean()), "median": float(np.median(d)), "p95": float(np.percentile(d, 95)), "max": float(d.max()), "n": int(d.size)}


def _crop_to_contour(image, mask, lo, hi):
    """The service's crop_to_contour_bounding_box and clamp (service.py:34-62, 152-156) -> (cropped image, cropped mask)."""
    if not mask.same_grid(image):
        mask = apply_transform(mask, reference_image=image, default_value=0, interpolator=sitkNearestNeighbor)
    size, index = label_to_roi(mask)
    cropped, cmask = crop_to_roi(image, size, index), crop_to_roi(mask, size, index)
    t = cropped.tensor if cropped.tensor.dtype == torch.float32 else cropped.tensor.float()
    return cropped.like(t.clamp(lo, hi)), cmask


def dir_qa(primary, secondary, primary_contours, secondary_contours, settings=None):
    """The DIR QA service on Images: for every contour name present on both sides, SIFT landmark pairs of the two images
    inside that contour -> {name: (primary PointTable, secondary PointTable)}, rows paired.  settings: DIRQA_SETTINGS_DEFAULTS
    and the caller's overrides; "includePointsMode" "CONTOUR" drops a pair when either point's voxel is outside its mask (S10),
    "BOUNDINGBOX" keeps every pair.  Optional keys `octaves`, `intervals`, `ratio` go to sift_keypoints / match_keypoints."""
    s = dict(DIRQA_SETTINGS_DEFAULTS)
    s.update(settings or {})
    mode = s["includePointsMode"]
    if mode not in ("CONTOUR", "BOUNDINGBOX"):
        raise ValueError(f"dir_qa: includePointsMode must be CONTOUR or BOUNDINGBOX, got {mode!r}")
    lo, hi = (float(v) for v in s["intensityRange"])
    primary, secondary = as_image(primary), as_image(secondary)
    out = {}
    for name, pmask in primary_contours.items():
        if name not in secondary_contours:
            continue            # (service.py:125-129: no matching contour)
        sides = []
        for image, mask in ((primary, as_image(pmask)), (secondary, as_image(secondary_contours[name]))):
            cropped, cmask = _crop_to_contour(image, mask, lo, hi)
            kp = sift_keypoints(cropped, intensity_range=(lo, hi), contrast_threshold=s["contrastThreshold"],
                                curvature_threshold=s["curvatureThreshold"], octaves=s.get("octaves", 3), intervals=s.get("intervals", 3))
            sides.append((kp, cmask))
        (ka, ma), (kb, mb) = sides
        pairs, _ = match_keypoints(ka, kb, ratio=s.get("ratio", 0.8))
        pa, pb = ka.points[pairs[:, 0]], kb.points[pairs[:, 1]]
        names = [f"{name}_{i}" for i in range(len(pairs))]
        keep = np.ones(len(pairs), dtype=bool)
        if mode == "CONTOUR":
            keep = points_in_mask(pa, ma) & points_in_mask(pb, mb)
        names = [n for n, k in zip(names, keep) if k]
        out[name] = (PointTable(list(names), pa[keep]), PointTable(list(names), pb[keep]))
    return out
