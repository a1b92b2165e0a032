"""Drop-in for platipy/imaging/label/comparison.py: volume, surface-distance and added-path-length metrics of a pair
of labels, computed where the labels live.

Inputs are anything `as_image` accepts; non-zero = foreground; both labels must sit on one grid (ValueError otherwise).
Results are Python floats, dicts of floats and lists, as in the reference.

GPU (pp_compare.h, pp_dist.hip, pp_morph.hip): the overlap counts, the contours, the signed Maurer distance maps and ONE
fused pass per (label, distance map) pair that selects the samples, reads the map only there and returns count, fp64 sum and
sum of squares, min, max, the count of values <= tau and ITK's 128-bin histogram.  Host: the handful of divisions and square
roots that combine those numbers, written exactly as the reference combines them.

Synchronisations (device -> host reads) per call, none in between:
  compute_surface_metrics      1  (six result structs: two directions, two directed Hausdorff passes, two surface-DSC halves)
  compute_surface_dsc          1
  compute_volume_metrics       1  (three counts); compute_volume 1
  compute_apl / total / mean   1  (three per-slice count vectors)
  compute_metric_dsc / _sensitivity / _specificity   1, plus 2 for the bounding boxes of auto_crop=True
  compute_metric_masd / _hd    1, plus 2 for the bounding boxes and 1 for the emptiness test of auto_crop=True
A workspace that has to grow (the first call at a new size) allocates, which synchronises once more.

The reference's quirks are reproduced, not corrected; each is named where it happens:
  * `hausdorffDistance95` is np.percentile of the TWO directed maxima, not a percentile of the distances;
  * `sigmaSurfaceDistance` is not divided by the number of points (101.8 for a one-voxel shift of a 40-voxel cube);
  * `medianSurfaceDistance` is ITK's histogram median (the centre of one of 128 bins over the range of the WHOLE distance
    map), averaged over the two directions -- not the median of the distances;
  * the per-direction standard deviation is the sample one (n - 1): a one-voxel contour gives 0 / 0 = nan.
Voxels outside the image are "not a neighbour" for every contour / border rule here.  Whether ITK's filters agree on the image
boundary is pinned by nothing: `auto_crop=True` puts object voxels on the boundary by construction.
"""
import numpy as np
import torch

from .. import _lib, runtime
from ..image import as_image
from ..utils.crop import crop_to_roi, label_to_roi

VOLUME_KEYS = ("DSC", "volumeOverlap", "fractionOverlap", "truePositiveFraction", "trueNegativeFraction",
               "falsePositiveFraction", "falseNegativeFraction")
SURFACE_KEYS = ("hausdorffDistance", "hausdorffDistance95", "meanSurfaceDistance", "medianSurfaceDistance",
                "maximumSurfaceDistance", "sigmaSurfaceDistance", "surfaceDSC")
APL_KEYS = ("totalAPL", "meanAPL")
MAX_APL_RADIUS = 15      # pp_binary_morph_ball_u8's radius limit


def _u8(image):
    t = image.tensor
    return (t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)).contiguous()


def _pair(label_a, label_b):
    a, b = as_image(label_a), as_image(label_b)
    if a.is_vector or b.is_vector:
        raise ValueError("label comparison needs scalar labels")
    if not a.same_grid(b):
        raise ValueError(f"label comparison needs both labels on one grid: {a!r} vs {b!r}")
    return a, b


def _auto_crop(a, b):
    """The reference's auto_crop: both labels cut to the bounding box of their union (label_to_roi without expansion).
    Raises ValueError when both labels are empty (there is no box)."""
    ua, ub = _u8(a), _u8(b)
    size, index = label_to_roi([a.like(ua), b.like(ub)])
    return crop_to_roi(a.like(ua), size, index), crop_to_roi(b.like(ub), size, index)


def _counts(a, b):
    """|A|, |B|, |A and B|, N as Python ints."""
    ua, ub = _u8(a), _u8(b)
    n = ua.numel()
    na, nb, nab = runtime.context(a.device).overlap_counts(ua, ub, n)
    return int(na), int(nb), int(nab), int(n)


def compute_volume(label):
    """The volume in cubic centimetres: voxel count x prod(spacing) / 1000 (comparison.py:22-32; the reference sums the voxel
    VALUES, which is the count for a 0 / 1 label)."""
    label = as_image(label)
    na, _, _, _ = _counts(label, label)
    return float(na * np.prod(label.GetSpacing()) / 1000)


def _volume_metrics(na, nb, nab, n, spacing):
    na, nb, nab, n = (np.int64(v) for v in (na, nb, nab, n))
    union = na + nb - nab
    true_pos, true_neg = nab, n - union
    false_pos, false_neg = nb - nab, na - nab
    with np.errstate(divide="ignore", invalid="ignore"):     # a zero denominator gives nan / inf, as numpy does in the reference
        result = {
            "DSC": np.float64(2.0 * nab) / np.float64(na + nb),
            "volumeOverlap": nab * (np.prod(spacing) / 1000.0),
            "fractionOverlap": np.float64(nab) / np.float64(union),
            "truePositiveFraction": np.float64(true_pos) / np.float64(true_pos + false_neg),
            "trueNegativeFraction": np.float64(true_neg) / np.float64(true_neg + false_pos),
            "falsePositiveFraction": np.float64(false_pos) / np.float64(true_neg + false_pos),
            "falseNegativeFraction": np.float64(false_neg) / np.float64(true_pos + false_neg),
        }
    return {k: float(v) for k, v in result.items()}


def compute_volume_metrics(label_a, label_b):
    """DSC, volumeOverlap (cm^3), fractionOverlap, truePositiveFraction, trueNegativeFraction, falsePositiveFraction,
    falseNegativeFraction (comparison.py:144-191), from the four integer counts |A|, |B|, |A and B|, N in float64.  A zero
    denominator (an empty label, labels that fill the image) gives nan or inf, not an exception."""
    a, b = _pair(label_a, label_b)
    return _volume_metrics(*_counts(a, b), a.GetSpacing())


def _cropped_metric(label_a, label_b, auto_crop, key):
    a, b = _pair(label_a, label_b)
    if auto_crop:
        a, b = _auto_crop(a, b)
    return _volume_metrics(*_counts(a, b), a.GetSpacing())[key]


def compute_metric_dsc(label_a, label_b, auto_crop=True):
    """The Dice similarity coefficient 2 |A and B| / (|A| + |B|) (comparison.py:194-213)."""
    return _cropped_metric(label_a, label_b, auto_crop, "DSC")


def compute_metric_specificity(label_a, label_b, auto_crop=True):
    """TN / (TN + FP) with label_a the truth (comparison.py:216-242).  With auto_crop=True the true negatives are counted
    inside the bounding box of the union only, so the value differs from auto_crop=False: the reference's behaviour."""
    return _cropped_metric(label_a, label_b, auto_crop, "trueNegativeFraction")


def compute_metric_sensitivity(label_a, label_b, auto_crop=True):
    """TP / (TP + FN) with label_a the truth (comparison.py:245-270)."""
    return _cropped_metric(label_a, label_b, auto_crop, "truePositiveFraction")


class _SurfacePasses:
    """The fused statistics passes of one label pair, queued on the stream and read back once.  Each signed distance map is
    computed once and serves every pass that samples it; one fp32 volume of scratch is reused for all of them."""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.ua, self.ub = _u8(a), _u8(b)
        self.geom = a.geom()
        self.size = a.GetSize()
        self.n = self.ua.numel()
        self.device = self.ua.device
        self.ctx = runtime.context(a.device)
        self.names = []
        self.jobs = []
        self._dist = None

    def _map(self, mask):
        """The signed Maurer distance map of `mask` into the shared scratch volume (valid until the next _map)."""
        if self._dist is None:
            self._dist = torch.empty(self.ua.shape, dtype=torch.float32, device=self.device)
        self.ctx.distance_map(mask, self.geom, self._dist, signed=True, inside_positive=False)
        return self._dist

    def directions(self, hausdorff=True, stats=True):
        """For (la, lb) in ((a, b), (b, a)): |d(la)| on LabelContour(lb) -> 'stat_ab' / 'stat_ba' (with the histogram over the
        range of the whole |d(la)|), and max(d(la), 0) over every voxel of lb -> 'hd_ba' / 'hd_ab' (directed Hausdorff lb -> la)."""
        for la, lb, tag, rev in ((self.ua, self.ub, "ab", "ba"), (self.ub, self.ua, "ba", "ab")):
            d = self._map(la)
            if stats:
                rng = torch.empty(2, dtype=torch.float32, device=self.device)
                self.ctx.abs_range(d, self.n, rng)
                self._queue("stat_" + tag, lb, d, _lib.SURFACE_CONTOUR_ABS, 0.0, rng)
            if hausdorff:
                self._queue("hd_" + rev, lb, d, _lib.SURFACE_LABEL_POS, 0.0, None)

    def surface_dsc(self, tau):
        """BinaryContour (26-neighbour rule) of both labels, the signed map of each CONTOUR image, and the count of the other
        contour's voxels with map <= tau -> 'sdsc_b_near_a', 'sdsc_a_near_b'."""
        ca, cb = torch.empty_like(self.ua), torch.empty_like(self.ub)
        self.ctx.binary_contour(self.ua, self.size, ca, fully_connected=True)
        self.ctx.binary_contour(self.ub, self.size, cb, fully_connected=True)
        self._queue("sdsc_b_near_a", cb, self._map(ca), _lib.SURFACE_NONZERO, tau, None)
        self._queue("sdsc_a_near_b", ca, self._map(cb), _lib.SURFACE_NONZERO, tau, None)

    def _queue(self, name, select, dist, mode, tau, rng):
        self.names.append(name)
        self.jobs.append((select, mode, tau, rng))
        if not hasattr(self, "_out"):
            self._out = torch.zeros(8 * _lib.SURFACE_STATS_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        slot = self._out[(len(self.names) - 1) * _lib.SURFACE_STATS_DTYPE.itemsize:]
        self.ctx.surface_stats(select, dist, self.geom, mode, slot, tau=tau, device_range=rng)

    def read(self):
        """The one device -> host read: {name: numpy record of pp_surface_stats}."""
        raw = self._out.cpu().numpy()[: len(self.names) * _lib.SURFACE_STATS_DTYPE.itemsize].view(_lib.SURFACE_STATS_DTYPE)
        return {name: raw[k] for k, name in enumerate(self.names)}


def _direction_statistics(rec):
    """n, mean, max, sample standard deviation and histogram median of one direction, the way
    itk::LabelStatisticsImageFilter (behind sitk.LabelIntensityStatisticsImageFilter) derives them."""
    n = int(rec["count"])
    total, total_sq = np.float64(rec["sum"]), np.float64(rec["sum_sq"])
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = total / np.float64(n)
        std = np.sqrt((total_sq - total * total / np.float64(n)) / np.float64(n - 1))      # n = 1: 0 / 0 = nan
    if n == 0:
        return 0, np.float64(np.nan), np.float64(np.nan), np.float64(np.nan), np.float64(np.nan)
    return n, mean, np.float64(rec["max"]), std, histogram_median(rec["hist"], rec["range_lo"], rec["range_hi"])


def histogram_median(hist, lo, hi):
    """ITK's histogram median: the centre of the first of the 128 bins over [lo, hi] whose cumulative count reaches half the
    total."""
    hist = np.asarray(hist, dtype=np.int64)
    lo, hi = np.float64(lo), np.float64(hi)
    bins = hist.shape[0]
    cum = np.cumsum(hist)
    i = int(np.searchsorted(cum, cum[-1] / 2.0, side="left"))
    return lo + (i + 0.5) * (hi - lo) / bins


def _combine_surface(rec, with_dsc=True):
    """Exactly the reference's combination of the two directions (comparison.py:118-139)."""
    stats = [_direction_statistics(rec[k]) for k in ("stat_ab", "stat_ba")]
    if int(rec["hd_ab"]["count"]) == 0 or int(rec["hd_ba"]["count"]) == 0:
        # a label without a voxel has no distance map (ITK's filters refuse it); every distance is nan
        stats = [(s[0],) + (np.float64(np.nan),) * 4 for s in stats]
    num_points = [s[0] for s in stats]
    mean_sd_list, max_sd_list = [s[1] for s in stats], [s[2] for s in stats]
    std_sd_list, median_sd_list = [s[3] for s in stats], [s[4] for s in stats]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_surf_dist = np.dot(mean_sd_list, num_points) / np.sum(num_points)
        max_surf_dist = np.max(max_sd_list)
        hd_95 = np.percentile(max_sd_list, 95) if not np.any(np.isnan(max_sd_list)) else np.float64(np.nan)      # (sic)
        std_surf_dist = np.sqrt(np.dot(num_points, np.add(np.square(std_sd_list),
                                                          np.square(np.subtract(mean_sd_list, mean_surf_dist)))))    # (sic)
        median_surf_dist = np.mean(median_sd_list)
    result = {
        "hausdorffDistance": _hausdorff(rec),
        "hausdorffDistance95": float(hd_95),
        "meanSurfaceDistance": float(mean_surf_dist),
        "medianSurfaceDistance": float(median_surf_dist),
        "maximumSurfaceDistance": float(max_surf_dist),
        "sigmaSurfaceDistance": float(std_surf_dist),
    }
    if with_dsc:
        result["surfaceDSC"] = _surface_dsc(rec)
    return result, num_points


def _hausdorff(rec):
    """itk::HausdorffDistanceImageFilter: the larger of the two directed distances; nan when a label has no voxel."""
    if int(rec["hd_ab"]["count"]) == 0 or int(rec["hd_ba"]["count"]) == 0:
        return float("nan")
    return float(max(rec["hd_ab"]["max"], rec["hd_ba"]["max"]))


def _surface_dsc(rec):
    near = int(rec["sdsc_b_near_a"]["count_le_tau"]) + int(rec["sdsc_a_near_b"]["count_le_tau"])
    surface = int(rec["sdsc_b_near_a"]["count"]) + int(rec["sdsc_a_near_b"]["count"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(near) / np.float64(surface))


def compute_surface_dsc(label_a, label_b, tau=3.0):
    """Surface Dice (Nikolov et al. 2021; comparison.py:35-72): contours by BinaryContour with full (26-neighbour)
    connectivity, the signed Maurer map of each contour image, (|cb and d_a <= tau| + |ca and d_b <= tau|) / (|ca| + |cb|).
    Two empty labels give 0 / 0 = nan."""
    a, b = _pair(label_a, label_b)
    p = _SurfacePasses(a, b)
    p.surface_dsc(float(tau))
    return _surface_dsc(p.read())


def compute_surface_metrics(label_a, label_b, verbose=False):
    """hausdorffDistance, hausdorffDistance95, meanSurfaceDistance, medianSurfaceDistance, maximumSurfaceDistance,
    sigmaSurfaceDistance, surfaceDSC (tau = 3) of two labels, without cropping (comparison.py:75-141).  The reference's
    combination is kept to the letter, see the module docstring for what is odd about hausdorffDistance95,
    sigmaSurfaceDistance and medianSurfaceDistance.  An empty label gives nan for every distance."""
    a, b = _pair(label_a, label_b)
    p = _SurfacePasses(a, b)
    p.directions()
    p.surface_dsc(3.0)
    result, num_points = _combine_surface(p.read())
    if verbose:
        print("        Boundary points:  {0}  {1}".format(num_points[0], num_points[1]))
    return result


def _either_empty(a, b):
    na, nb, _, _ = _counts(a, b)
    return na == 0 or nb == 0


def compute_metric_masd(label_a, label_b, auto_crop=True):
    """The mean absolute surface distance: the point-weighted mean of the two directions' mean |distance map| on the other
    label's LabelContour (comparison.py:273-312); nan when either label is empty.  With auto_crop=True the labels are really
    cropped to the union's bounding box first, which puts object voxels on the image boundary; contour and border rules
    here treat outside-the-image as "not a neighbour", and no known answer pins ITK's behaviour there."""
    a, b = _pair(label_a, label_b)
    if auto_crop:
        a, b = _auto_crop(a, b)
        if _either_empty(a, b):
            return float("nan")
    p = _SurfacePasses(a, b)
    p.directions(hausdorff=True, stats=True)
    rec = p.read()
    if int(rec["hd_ab"]["count"]) == 0 or int(rec["hd_ba"]["count"]) == 0:
        return float("nan")
    stats = [_direction_statistics(rec[k]) for k in ("stat_ab", "stat_ba")]
    return float(np.dot([s[1] for s in stats], [s[0] for s in stats]) / np.sum([s[0] for s in stats]))


def compute_metric_hd(label_a, label_b, auto_crop=True):
    """The Hausdorff distance of itk::HausdorffDistanceImageFilter: the larger of the two directed distances, directed(A -> B)
    = max over ALL voxels of A of max(signed distance map of B, 0) (comparison.py:315-343); nan when either label is empty.
    The same remark on auto_crop=True and the image boundary as compute_metric_masd."""
    a, b = _pair(label_a, label_b)
    if auto_crop:
        a, b = _auto_crop(a, b)
        if _either_empty(a, b):
            return float("nan")
    p = _SurfacePasses(a, b)
    p.directions(hausdorff=True, stats=False)
    return _hausdorff(p.read())


def compute_apl(label_ref, label_test, distance_threshold_mm=3):
    """The added path length per z slice, in voxels (comparison.py:346-387): for every slice where at least one label has a
    voxel, the number of voxels of the reference's 2-D LabelContour that the test's 2-D LabelContour, dilated by the 2-D ITK
    ball of radius r = int(ceil(threshold / mean(spacing[:2]))) when the threshold is positive, does not cover.  Returns the
    list of the kept slices' counts in slice order.  r above 15, the limit of the dilation kernel, raises ValueError."""
    ref, test = _pair(label_ref, label_test)
    distance = int(np.ceil(distance_threshold_mm / np.mean(ref.GetSpacing()[:2])))
    if distance_threshold_mm > 0 and distance > MAX_APL_RADIUS:
        raise ValueError(f"compute_apl: the threshold is {distance} voxels in plane; the dilation kernel "
                         f"(pp_binary_morph_ball_u8) takes a radius of at most {MAX_APL_RADIUS}")
    ctx = runtime.context(ref.device)
    size = ref.GetSize()
    ur, ut = _u8(ref), _u8(test)
    ref_contour, test_contour = torch.empty_like(ur), torch.empty_like(ut)
    ctx.slice_contour(ur, size, ref_contour)
    ctx.slice_contour(ut, size, test_contour)
    if distance_threshold_mm > 0:
        dilated = torch.empty_like(ut)
        ctx.binary_morph_ball(test_contour, size, [distance, distance, 0], 0, dilated)
        test_contour = dilated
    counts = torch.zeros((3, size[2]), dtype=torch.int64, device=ur.device)
    ctx.slice_masked_count(ref_contour, test_contour, size, counts[0])
    ctx.slice_masked_count(ur, None, size, counts[1])
    ctx.slice_masked_count(ut, None, size, counts[2])
    added, in_ref, in_test = counts.cpu().numpy()
    return [int(added[z]) for z in range(size[2]) if in_ref[z] + in_test[z] != 0]


def compute_metric_total_apl(label_ref, label_test, distance_threshold_mm=3):
    """The total slice-wise added path length in mm (comparison.py:390-409): sum of compute_apl x mean(spacing[:2])."""
    apl = compute_apl(label_ref, label_test, distance_threshold_mm=distance_threshold_mm)
    return float(np.sum(apl) * np.mean(as_image(label_ref).GetSpacing()[:2]))


def compute_metric_mean_apl(label_ref, label_test, distance_threshold_mm=3):
    """The mean slice-wise added path length in mm (comparison.py:412-431); nan when no slice holds a voxel."""
    apl = compute_apl(label_ref, label_test, distance_threshold_mm=distance_threshold_mm)
    if not apl:
        return float("nan")
    return float(np.mean(apl) * np.mean(as_image(label_ref).GetSpacing()[:2]))


def compute_metrics(reference, test, metrics=VOLUME_KEYS + SURFACE_KEYS):
    """Score a dictionary of structures: {structure: label} x 2 (the shape run_segmentation returns) ->
    {structure: {metric: value}} for the structures both dictionaries hold, in `reference`'s order.

    NOT part of the reference's comparison.py: a convenience of this package.  `metrics` takes any key of
    compute_volume_metrics and compute_surface_metrics plus "totalAPL" and "meanAPL" (distance threshold 3 mm); nothing is
    cropped, so every value equals what the per-function call returns.  Per structure the counts are taken once, and each of
    the four distance maps (label a, label b, and their two contour images) once."""
    metrics = list(metrics)
    unknown = [m for m in metrics if m not in VOLUME_KEYS + SURFACE_KEYS + APL_KEYS]
    if unknown:
        raise ValueError(f"compute_metrics: unknown metrics {unknown}; known: {VOLUME_KEYS + SURFACE_KEYS + APL_KEYS}")
    out = {}
    for name, ref_label in reference.items():
        if name not in test:
            continue
        values = {}
        if any(m in VOLUME_KEYS for m in metrics):
            values.update(compute_volume_metrics(ref_label, test[name]))
        if any(m in SURFACE_KEYS for m in metrics):
            values.update(compute_surface_metrics(ref_label, test[name]))
        if "totalAPL" in metrics:
            values["totalAPL"] = compute_metric_total_apl(ref_label, test[name])
        if "meanAPL" in metrics:
            values["meanAPL"] = compute_metric_mean_apl(ref_label, test[name])
        out[name] = {m: values[m] for m in metrics}
    return out
