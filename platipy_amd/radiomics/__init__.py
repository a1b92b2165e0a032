"""Drop-in for the reference's radiomics service (services/radiomics/service.py, "PyRadiomics Extractor"): first-order and
texture features of an image inside each of its contour masks, one table row per contour -- without files, DataObjects or
the REST endpoint.

GPU (csrc/pp_radiomics.h, csrc/pp_dose.h), per structure, on the contiguous crop of its bounding box:
  count, sum, min, max     pp_dose_histogram_f32's statistics (a NaN inside the mask is refused there)
  percentiles              pp_masked_order_stats_f32 (the two order statistics np.percentile interpolates between)
  central moments          pp_masked_moments_f32 about the exact mean, and again over [P10, P90] for the robust MAD
  grey levels              pp_radiomics_discretise_f32 against np.arange's own edges
  glcm, gldm, ngtdm        pp_texture_neighbourhood_u16 (one pass over LDS tiles)
  glrlm                    pp_texture_runs_u16
Host: the feature formulas in fp64 numpy on those small integer tables (features.py).

pyradiomics is not installed where this was written, so parity with it is UNPINNED, like this build's parity with
SimpleITK: the semantics are recalled from pyradiomics 3.x and marked Q1 ... in the source.

Q1: low = min - (min mod binWidth) with Python's floor modulo.  Q2: edges = np.arange(low, max + 2 binWidth, binWidth); a
single edge e becomes [e - 0.5, e + 0.5].  Q3: level = np.digitize(v, edges), 1-based.  Q4: Ng is the largest level.
Q5 ... Q22: features.py.  Q23: getFeatureNames() lists a class's features by name (inspect.getmembers sorts), so the default
feature set and available_radiomics() are in sorted order; a caller's own list keeps the caller's order.
"""
import logging

import numpy as np
import torch

from .. import runtime
from ..image import as_image
from ..transform import sitkNearestNeighbor
from . import features as F

logger = logging.getLogger(__name__)

# service.py:42-55
RADIOMICS_SETTINGS = {
    "contours": [],  # If empty will extract radiomics for all contours
    "radiomics": {},  # If empty will extract all first order radiomics
    "pyradiomics_settings": {
        "binWidth": 25,
        "resampledPixelSpacing": None,
        "interpolator": "sitkNearestNeighbor",
        "verbose": True,
        "removeOutliers": 10000,
    },
    "resample_to_image": False,  # If true, mask will be resampled to spacing of image
    "append_histogram": False,  # If true, histogram will be appended to the end of each output row
    "histogram_bins": 256,  # Used only if append_histogram is true
}

# service.py:31-40
AVAILABLE_RADIOMICS = ("firstorder", "shape", "glcm", "glrlm", "glszm", "ngtdm", "gldm", "custom")
NOT_BUILT = {
    "shape": "the shape class needs a surface mesh of the mask (marching cubes), which this build does not have",
    "glszm": "the glszm class needs connected zones per grey level (a labelling pass per level), which this build does not have",
}
TEXTURE_CLASSES = ("glcm", "glrlm", "gldm", "ngtdm")
PERCENTILES = (10, 25, 50, 75, 90)


def available_radiomics():
    """{class: [feature names]} for the classes built here: the content of the service's /api/radiomics endpoint
    (service.py:239-248) without `shape` and `glszm` (Q23: sorted by name)."""
    return {rad: sorted(F.FEATURES[rad]) for rad in AVAILABLE_RADIOMICS if rad in F.FEATURES}


# --------------------------------------------------------------------------------------
# one structure


def _f32(t):
    return t if t.dtype == torch.float32 else t.to(torch.float32)


def _u8(mask):
    t = mask.tensor
    return t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)


class _Structure:
    """The crop of one mask's bounding box and everything counted on it, each table made once on demand."""

    def __init__(self, image, mask, name="mask"):
        image, mask = as_image(image), as_image(mask)
        if image.is_vector or mask.is_vector:
            raise ValueError("radiomics: image and mask must be scalar images")
        if not image.same_grid(mask):
            raise ValueError(f"radiomics: mask {name!r} does not lie on the image's grid (resample_to_image=True puts it there)")
        self.name = name
        self.voxel_volume = float(np.prod(image.GetSpacing()))
        m = _u8(mask).to(image.device).contiguous()
        self.ctx = runtime.context(image.device)
        box = self.ctx.bounding_box(m, mask.GetSize(), False)
        if box[0] > box[1]:
            raise ValueError(f"radiomics: mask {name!r} is empty")
        crop = (slice(box[4], box[5] + 1), slice(box[2], box[3] + 1), slice(box[0], box[1] + 1))
        self.origin_index = (box[0], box[2], box[4])
        self.image = _f32(image.tensor[crop]).contiguous()                       # (crop first: the conversion touches the box only)
        self.mask = m[crop].contiguous()
        self.size = (self.image.shape[2], self.image.shape[1], self.image.shape[0])
        self.n = self.image.numel()
        _, stats = self.ctx.dose_histogram(self.image, [self.mask], self.n, [0.0, 1.0])     # (ValueError for a NaN inside the mask)
        self.count, self.sum = int(stats["count"][0]), float(stats["dose_sum"][0])
        self.minimum, self.maximum = float(stats["dose_min"][0]), float(stats["dose_max"][0])
        if not (np.isfinite(self.minimum) and np.isfinite(self.maximum)):
            raise ValueError(f"radiomics: the image holds an infinity inside mask {name!r}")
        self._cache = {}

    def _once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def percentiles(self):
        def make():
            ranks = []
            for q in PERCENTILES:
                lo, hi, _ = F.percentile_rank(self.count, q)
                ranks += [lo, hi]
            v = self.ctx.masked_order_stats(self.image, self.mask, self.n, ranks)
            return {q: F.percentile_value(v[2 * k], v[2 * k + 1], F.percentile_rank(self.count, q)[2]) for k, q in enumerate(PERCENTILES)}
        return self._once("pct", make)

    def edges(self, bin_width):
        bw = float(bin_width)
        if not (np.isfinite(bw) and bw > 0.0):
            raise ValueError(f"radiomics: binWidth must be positive, got {bin_width!r}")
        low = self.minimum - (self.minimum % bw)                                   # Q1
        e = np.arange(low, self.maximum + 2.0 * bw, bw)                           # Q2
        if e.size == 1:
            e = np.array([e[0] - 0.5, e[0] + 0.5])
        return e

    def levels(self, bin_width):
        """(levels as an int16 tensor holding uint16 bits, Ng, voxels per level [Ng])."""
        def make():
            e = self.edges(bin_width)
            ng = int(np.digitize(np.float64(np.float32(self.maximum)), e))         # Q3, Q4
            lev = torch.empty(self.image.shape, dtype=torch.int16, device=self.image.device)
            self.ctx.radiomics_discretise(self.image, self.mask, self.n, e, lev)
            hist, _ = self.ctx.dose_histogram(self.image, [self.mask], self.n, e)
            return lev, ng, hist[0][:ng]
        return self._once(("levels", float(bin_width)), make)

    def neighbourhood(self, bin_width, wanted):
        """The tables of pp_texture_neighbourhood_u16 named in `wanted` ("glcm", "gldm", "ngtdm"), one call for those missing."""
        key = ("nb", float(bin_width))
        have = self._cache.setdefault(key, {})
        need = [w for w in wanted if w not in have]
        if need:
            lev, ng, _ = self.levels(bin_width)
            got = self.ctx.texture_neighbourhood(lev, self.size, ng, glcm="glcm" in need, gldm="gldm" in need, ngtdm="ngtdm" in need)
            for w in need:
                have[w] = (got["ngtdm_n"], got["ngtdm_s"]) if w == "ngtdm" else got[w]
        return have

    def runs(self, bin_width):
        def make():
            lev, ng, _ = self.levels(bin_width)
            return self.ctx.texture_runs(lev, self.size, ng)
        return self._once(("runs", float(bin_width)), make)

    def moments(self):
        """The sums about the exact mean: S|d|, S d^2, S d^3, S d^4, S v^2."""
        def make():
            _, m = self.ctx.masked_moments(self.image, self.mask, self.n, centre=self.sum / self.count)
            return m[1:]
        return self._once("moments", make)

    def robust(self):
        """(count, S|v - their mean|) over the values in [P10, P90] (Q11).  No value need lie there (two voxels 10 and 20:
        [11, 19]); then the count is 0 and the feature is the mean of an empty set, NaN."""
        def make():
            pct = self.percentiles()
            lo, hi = np.float64(pct[10]), np.float64(pct[90])
            rc, rs = self.ctx.masked_moments(self.image, self.mask, self.n, lo, hi, 0.0)
            if rc == 0:
                return 0, 0.0
            rc, rs = self.ctx.masked_moments(self.image, self.mask, self.n, lo, hi, rs[0] / rc)
            return rc, rs[1]
        return self._once("robust", make)

    def firstorder_stats(self, names, bin_width):
        """What F.firstorder needs for `names`, and no more: each part (F.FIRSTORDER_NEEDS) is made when a feature asks for
        it, so that Mean alone costs no percentile, moment or discretisation call (and meets none of their limits)."""
        s = {"count": self.count, "sum": self.sum, "minimum": self.minimum, "maximum": self.maximum, "voxel_volume": self.voxel_volume}
        parts = {"pct": self.percentiles, "m": self.moments, "robust": self.robust, "hist": lambda: self.levels(bin_width)[2]}
        for part, users in F.FIRSTORDER_NEEDS.items():
            if any(name in users for name in names):
                s[part] = parts[part]()
        return s

    def compute(self, rad, names, bin_width):
        if rad == "firstorder":
            return F.firstorder(names, self.firstorder_stats(names, bin_width))
        if rad == "custom":
            return F.custom(names, {"pct": self.percentiles()})
        present = np.flatnonzero(self.levels(bin_width)[2] > 0) + 1             # Q5
        if rad == "glcm":
            return F.glcm(names, self.neighbourhood(bin_width, ["glcm"])["glcm"], present)
        if rad == "glrlm":
            return F.glrlm(names, self.runs(bin_width), present, self.count)
        if rad == "gldm":
            return F.gldm(names, self.neighbourhood(bin_width, ["gldm"])["gldm"], present)
        if rad == "ngtdm":
            return F.ngtdm(names, *self.neighbourhood(bin_width, ["ngtdm"])["ngtdm"])
        raise KeyError(rad)


def texture_matrices(image, mask, bin_width=25, classes=TEXTURE_CLASSES):
    """The raw integer tables of one structure, as numpy int64 arrays on the crop of the mask's bounding box:
      "levels"  uint16 [z, y, x] of the crop, 0 outside the mask; "ng"; "origin_index" (x, y, z) of the crop in the image
      "glcm"    [13, ng, ng]  symmetric (P + P^T) counts per direction; directions: the offsets (dz, dy, dx) whose first
                non-zero component is positive, in lexicographic order ("directions")
      "glrlm"   [13, ng, max(crop size)]   runs of length column + 1
      "gldm"    [ng, 27]      voxels of a level by their number of same-level neighbours (dependence size = column + 1)
      "ngtdm_n", "ngtdm_s" [ng, 27]  voxels of a level by their number k of neighbours inside the mask, and the sum of
                |level k - sum of the neighbours' levels| over them (s_i = sum_k S[i][k] / k)
    Integer counts: two calls return the same bits."""
    unknown = [c for c in classes if c not in TEXTURE_CLASSES]
    if unknown:
        raise ValueError(f"texture_matrices: unknown classes {unknown} (of {TEXTURE_CLASSES})")
    s = _Structure(image, mask)
    lev, ng, _ = s.levels(bin_width)
    out = {"levels": lev.cpu().numpy().view(np.uint16), "ng": ng, "origin_index": s.origin_index,
           "directions": [(c // 9 - 1, (c // 3) % 3 - 1, c % 3 - 1) for c in range(14, 27)]}
    nb = s.neighbourhood(bin_width, [c for c in ("glcm", "gldm", "ngtdm") if c in classes])
    if "glcm" in classes:
        out["glcm"] = nb["glcm"] + nb["glcm"].transpose(0, 2, 1)
    if "gldm" in classes:
        out["gldm"] = nb["gldm"]
    if "ngtdm" in classes:
        out["ngtdm_n"], out["ngtdm_s"] = nb["ngtdm"]
    if "glrlm" in classes:
        out["glrlm"] = s.runs(bin_width)
    return out


def compute_histogram(image, mask, bins):
    """np.histogram of the image values inside the mask -> (counts, edges) (service.py:58-73), counted by
    pp_dose_histogram_f32.  bins: an int (numpy's equal bins between the minimum and the maximum inside the mask) or a
    sequence of edges.  The image is held as float32 (another dtype is converted first), and the result is np.histogram of
    that float32 array, edges included: for an int, numpy's own float32 edges (np.histogram_bin_edges needs only the
    minimum, the maximum and the dtype), against which numpy corrects its arithmetic bin guess, so a value's bin is
    the one its float32 edges bound; a sequence is returned as given and compared as doubles, as np.searchsorted does."""
    image, mask = as_image(image), as_image(mask)
    if image.GetSize() != mask.GetSize():
        raise ValueError("compute_histogram: image and mask differ in size")
    img = _f32(image.tensor).contiguous()
    m = _u8(mask).to(img.device).contiguous()
    ctx = runtime.context(img.device)
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool):
        if bins < 1:
            raise ValueError("`bins` must be positive, when an integer")
        _, stats = ctx.dose_histogram(img, [m], img.numel(), [0.0, 1.0])
        ends = [stats["dose_min"][0], stats["dose_max"][0]] if stats["count"][0] else []
        edges = np.histogram_bin_edges(np.asarray(ends, dtype=np.float32), int(bins))   # (ValueError for a range that is not finite)
    else:
        edges = np.asarray(bins)
        if edges.ndim != 1 or edges.size < 2:
            raise ValueError("`bins` must be an int or a 1-d sequence of at least two edges")
        if np.any(edges[:-1] > edges[1:]):
            raise ValueError("`bins` must increase monotonically, when an array")
    counts, _ = ctx.dose_histogram(img, [m], img.numel(), edges.astype(np.float64))
    return counts[0], edges


def extract_radiomics(image, masks, radiomics=None, pyradiomics_settings=None, resample_to_image=False, append_histogram=False,
                      histogram_bins=256, contours=None, as_frame=False):
    """The table of the "PyRadiomics Extractor" (service.py:76-236) for one image and its contour masks.

    masks: {name: Image}.  radiomics: {class: [feature names]}; empty or None = every non-deprecated first-order feature
    (service.py:95-97).  contours: names to keep, empty or None = all (:115).  An unknown class or feature is skipped with a
    warning (:155-157, :173-175); a class with an empty feature list is skipped (:167).  `shape` and `glszm` raise
    NotImplementedError.  pyradiomics_settings: `binWidth` is honoured; `verbose`, `removeOutliers` and `interpolator` are
    accepted and ignored (the feature classes ignore removeOutliers too); a non-None `resampledPixelSpacing` raises
    NotImplementedError.  resample_to_image=True puts a mask that lies on another grid onto the image's grid by nearest
    neighbour (apply_transform); otherwise such a mask is a ValueError.  An empty mask, or a NaN or infinity inside one, is
    a ValueError; a feature whose part cannot be made (Entropy on more than 65535 grey levels) is one too, and costs and
    limits only the requests that name it.  RobustMeanAbsoluteDeviation is NaN where no value lies in [P10, P90] (two voxels).
    append_histogram adds ("histogram", "0") ... columns: compute_histogram(image, mask, histogram_bins).

    -> {name: {(class, feature): float}} in the service's column order; as_frame=True: the pandas table the service writes, a
    ("", "Contour") column first, then the (class, feature) columns, one row per contour."""
    settings = dict(RADIOMICS_SETTINGS["pyradiomics_settings"])
    settings.update(pyradiomics_settings or {})
    if settings.get("resampledPixelSpacing") is not None:
        raise NotImplementedError("radiomics: resampling to `resampledPixelSpacing` is not built; resample the image and masks first")
    bin_width = settings.get("binWidth", 25)
    radiomics = dict(radiomics or {})
    if len(radiomics) == 0:
        radiomics = {"firstorder": sorted(F.FIRSTORDER)}                         # service.py:95-97, Q23
    plan = []
    for rad, names in radiomics.items():
        if rad not in AVAILABLE_RADIOMICS:
            logger.warning("Radiomic Class not found: %s", rad)
            continue
        if len(names) == 0:                                                      # service.py:167
            continue
        if rad in NOT_BUILT:
            raise NotImplementedError(f"radiomics class {rad!r}: {NOT_BUILT[rad]}")
        keep = []
        for name in names:
            if name in F.FEATURES[rad]:
                if name not in keep:
                    keep.append(name)
            else:
                logger.warning("Feature not found: %s", name)
        plan.append((rad, keep))
    image = as_image(image)
    result = {}
    for name, mask in masks.items():
        if contours and name not in contours:
            logger.debug("Skipping Contour: %s", name)
            continue
        mask = as_image(mask)
        if resample_to_image and not image.same_grid(mask):
            from ..registration.utils import apply_transform

            mask = apply_transform(mask, reference_image=image, default_value=0, interpolator=sitkNearestNeighbor)
        s = _Structure(image, mask, name)
        row = {}
        for rad, names in plan:
            if not names:
                continue
            for feature, value in s.compute(rad, names, bin_width).items():
                row[(rad, feature)] = value
        if append_histogram:
            counts, _ = compute_histogram(image, mask, histogram_bins)
            for k, c in enumerate(counts):
                row[("histogram", str(k))] = int(c)
        result[name] = row
    if not as_frame:
        return result
    import pandas as pd

    rows = [{("", "Contour"): name, **row} for name, row in result.items()]
    columns = [("", "Contour")] + [c for c in dict.fromkeys(k for row in result.values() for k in row)]
    return pd.DataFrame(rows, columns=pd.MultiIndex.from_tuples(columns)) if rows else pd.DataFrame()
