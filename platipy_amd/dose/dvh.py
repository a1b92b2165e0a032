"""Drop-in for platipy/imaging/dose/dvh.py: dose-volume histograms of structures, counted where the dose and the masks live.

GPU (pp_dose.h): ONE pass over the dose and all the masks (pp_dose_histogram_f32) leaves every structure's np.histogram
counts, voxel count, mask-value sum, dose sum, minimum and maximum; one read-back of a few kilobytes.  Host: the cumulative
sums, divisions and np.interp calls on those small tables, written as the reference combines them.

Deviations from the reference, each named where it happens:
  * the dose is held as float32, like every image here; the bin edges are float64 (np.arange / np.linspace of Python floats)
    and a dose value is compared with them as a double;
  * the mean is the exact sum of the float32 doses divided by the count in float64 -- numpy's mean of a float32 array is a
    float32 pairwise sum; the two agree to float32 precision, and this one equals the reference's value for a float64 dose;
  * a NaN dose inside a structure raises ValueError (numpy would quietly return a NaN mean);
  * masks are taken as uint8: a label of another type is converted with `!= 0`, so its cc counts voxels.
"""
import collections

import numpy as np
import torch

from .. import _lib, runtime
from ..image import as_image
from ..registration.utils import resample_image
from ..transform import sitkLinear

DvhTable = collections.namedtuple("DvhTable", ["labels", "bins", "counts", "cc", "mean", "min", "max"])


def _mask_u8(image):
    t = image.tensor
    return (t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)).contiguous()


def _dose_f32(image):
    t = image.tensor
    return (t if t.dtype == torch.float32 else t.to(torch.float32)).contiguous()


def _scalar(x, what):
    x = as_image(x)
    if x.is_vector:
        raise ValueError(f"{what} must be a scalar image")
    return x


def resample_dose(dose_grid, label):
    """sitk.Resample(dose_grid, label, sitk.Transform(), sitk.sitkLinear): the dose on the label's grid, float32."""
    return resample_image(_scalar(dose_grid, "the dose grid"), label, None, sitkLinear, 0.0)


def masked_histogram(dose, masks, edges):
    """np.histogram(dose[mask != 0], bins=edges) for every uint8 mask tensor, and the masks' statistics, in one kernel call
    per 64 masks -> (int64 counts [len(masks), len(edges) - 1], _lib.DOSE_STATS_DTYPE records)."""
    ctx = runtime.context(dose.device)
    hist, stats = [], []
    for k in range(0, len(masks), _lib.DOSE_MAX_LABELS):
        h, s = ctx.dose_histogram(dose, masks[k:k + _lib.DOSE_MAX_LABELS], dose.numel(), edges)
        hist.append(h)
        stats.append(s)
    return np.concatenate(hist), np.concatenate(stats)


def _outer_edges(lo, hi, bins):
    """np.histogram's edges for an integer `bins` over values spanning [lo, hi]: linspace in float64, an empty range widened
    by -/+ 0.5, no values at all taken as [0, 1]."""
    if not lo <= hi:
        lo, hi = 0.0, 1.0
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, bins + 1)


def calculate_dvh(dose_grid, label, bins=1001):
    """The dose-volume histogram of one structure -> (bin centres, values).

    bins: an int (numpy's rule: that many equal bins between the minimum and the maximum dose inside the structure) or a
    sequence of edges.  values: the fraction of the structure that receives at least the bin's dose -- the counts summed from
    the top down, divided by their maximum; when every count is zero the integer zeros come back as they are.  The dose is
    resampled onto the label (linear, default 0) only when the two differ in size, as in the reference."""
    label, dose_grid = _scalar(label, "the label"), _scalar(dose_grid, "the dose grid")
    if dose_grid.GetSize() != label.GetSize():
        dose_grid = resample_dose(dose_grid, label)
    dose, mask = _dose_f32(dose_grid), _mask_u8(label)
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool):
        if bins < 1:
            raise ValueError("`bins` must be positive, when an integer")
        _, stats = masked_histogram(dose, [mask], [0.0, 1.0])
        lo, hi = float(stats["dose_min"][0]), float(stats["dose_max"][0])
        if stats["count"][0] and not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"autodetected range of [{lo}, {hi}] is not finite")
        edges = _outer_edges(lo, hi, int(bins))
    else:
        edges = np.asarray(bins, dtype=np.float64)
        if edges.ndim != 1 or edges.size < 2:
            raise ValueError("`bins` must be an int or a 1-d sequence of at least two edges")
        if np.any(edges[:-1] > edges[1:]):
            raise ValueError("`bins` must increase monotonically, when an array")
    counts, _ = masked_histogram(dose, [mask], edges)
    centres = (edges[1:] + edges[:-1]) / 2.0
    values = np.cumsum(counts[0][::-1])[::-1]
    if np.all(values == 0):
        return centres, values
    return centres, values / values.max()


def dvh_table(dose_grid, labels, bin_width=0.1, max_dose=None):
    """The differential DVH of every structure as plain arrays -> DvhTable(labels, bins, counts, cc, mean, min, max).

    labels: dict name -> mask; every mask must have the size of the first.  The dose is resampled onto the first label's
    grid (linear, default 0).  Edges: np.arange(-bin_width / 2, max_dose + bin_width, bin_width) in float64 on the host;
    max_dose falsy = the maximum of the resampled dose (as a Python float).  bins = the bin centres rounded to 10 decimals;
    counts = int64 [len(labels), len(bins)]; cc = mask.sum() * prod(spacing / 10) (a 0 / 255 mask counts 255 per voxel, as in
    the reference); mean, min, max = of the dose inside each structure (NaN for an empty one), whether or not the histogram's
    range holds it.  One kernel call and one read-back per 64 structures."""
    names = list(labels.keys())
    if not names:
        raise ValueError("no labels")
    images = [_scalar(labels[k], f"label {k!r}") for k in names]
    dose_grid = resample_dose(dose_grid, images[0])
    for k, im in zip(names, images):
        if im.GetSize() != images[0].GetSize():
            raise ValueError(f"label {k!r} has size {im.GetSize()}, the first label {images[0].GetSize()}")
    dose = _dose_f32(dose_grid)
    masks = [_mask_u8(im).to(dose.device) for im in images]
    if not max_dose:
        max_dose = float(runtime.context(dose.device).minmax(dose, dose.numel())[1])
    edges = np.arange(-bin_width / 2, max_dose + bin_width, bin_width)
    counts, stats = masked_histogram(dose, masks, edges)
    centres = np.round(((edges[1:] + edges[:-1]) / 2.0).astype(float), decimals=10)
    cc = np.array([s * np.prod([a / 10 for a in im.GetSpacing()]) for s, im in zip(stats["mask_sum"], images)], dtype=np.float64)
    n = stats["count"]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = stats["dose_sum"] / n.astype(np.float64)
    empty = n == 0
    return DvhTable(names, centres, counts, cc, mean, np.where(empty, np.nan, stats["dose_min"]).astype(np.float32),
                    np.where(empty, np.nan, stats["dose_max"]).astype(np.float32))


def cumulative_values(counts):
    """calculate_dvh's values for one row of counts."""
    values = np.cumsum(counts[::-1])[::-1]
    if np.all(values == 0):
        return values
    return values / values.max()


def calculate_dvh_for_labels(dose_grid, labels, bin_width=0.1, max_dose=None):
    """The cumulative DVH of every structure -> pandas.DataFrame with the columns `label`, `cc`, `mean` and one float column
    per bin centre (rounded to 10 decimals).  A thin wrapper over dvh_table; an empty structure gets a NaN mean and zeros."""
    import pandas as pd

    table = dvh_table(dose_grid, labels, bin_width=bin_width, max_dose=max_dose)
    rows = []
    for i, name in enumerate(table.labels):
        rows.append({"label": name, "cc": table.cc[i], "mean": table.mean[i], **dict(zip(table.bins, cumulative_values(table.counts[i])))})
    return pd.DataFrame(rows)


def _curves(dvh, label):
    if label:
        dvh = dvh[dvh.label == label]
    bins = np.array([c for c in dvh.columns if isinstance(c, float)])
    return dvh, bins, np.array(dvh[bins])


def _as_list(x):
    return x if isinstance(x, list) else [x]


def calculate_d_x(dvh, x, label=None):
    """The dose that x percent of each structure receives (x a number or a list) from a calculate_dvh_for_labels frame ->
    DataFrame with `label` and one `D{x}` column per x.  np.interp of x / 100 on the reversed curve; 0 when the curve's first
    value equals the sum of the row (a structure that gets no dose); D100 is the last bin whose value is exactly 1.0."""
    import pandas as pd

    dvh, bins, values = _curves(dvh, label)
    rows = []
    for r in range(len(dvh)):
        row = {"label": dvh.iloc[r].label}
        for threshold in _as_list(x):
            value = np.interp(threshold / 100, values[r][::-1], bins[::-1])
            if values[r, 0] == np.sum(values[r]):
                value = 0
            if threshold == 100:     # np.interp answers the first bin there
                value = bins[values[r] == 1.0][-1]
            row[f"D{threshold}"] = value
        rows.append(row)
    return pd.DataFrame(rows)


def calculate_v_x(dvh, x, label=None):
    """The volume (cc) of each structure that receives at least x Gy (x a number or a list) -> DataFrame with `label` and one
    `V{x}` column per x (`V{int(x)}` for a whole x): np.interp on the curve times the structure's cc."""
    import pandas as pd

    dvh, bins, values = _curves(dvh, label)
    rows = []
    for r in range(len(dvh)):
        d = dvh.iloc[r]
        row = {"label": d.label}
        for threshold in _as_list(x):
            name = f"V{int(threshold)}" if threshold - int(threshold) == 0 else f"V{threshold}"
            row[name] = np.interp(threshold, bins, values[r]) * d.cc
        rows.append(row)
    return pd.DataFrame(rows)


def calculate_d_cc_x(dvh, x, label=None, index_cols=None):
    """The dose that x cc of each structure receives (x a number or a list) -> DataFrame with the index columns (default
    ["label"]) and one `D{x}cc` column per x: calculate_d_x at x / cc * 100 percent, at most 100, of the first row of each
    group of `index_cols`."""
    import pandas as pd

    index_cols = ["label"] if index_cols is None else index_cols
    if label:
        dvh = dvh[dvh.label == label]
    rows = []
    for key in dvh.groupby(index_cols).groups.keys():
        key = list(key) if isinstance(key, tuple) else [key]
        row, group = {}, dvh
        for col, value in zip(index_cols, key):
            row[col] = value
            group = group[group[col] == value]
        for threshold in _as_list(x):
            percent = min((threshold / group.cc.iloc[0]) * 100, 100)
            row[f"D{threshold}cc"] = calculate_d_x(group, percent)[f"D{percent}"].iloc[0]
        rows.append(row)
    return pd.DataFrame(rows)
