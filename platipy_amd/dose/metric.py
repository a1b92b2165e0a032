"""Drop-in for platipy/imaging/dose/metric.py: mean and maximum dose, the dose to a volume and the volume receiving a dose,
for structures on a dose grid.

Every function resamples the dose onto the label (linear, identity transform, default 0), as the reference does, and takes
the voxels with label > 0.  GPU (pp_dose.h): count, exact dose sum and maximum from pp_dose_histogram_f32; the two order
statistics np.percentile interpolates between from pp_masked_order_stats_f32 (a radix select: the masked doses are never
copied or sorted); the threshold counts of any number of structures and thresholds from one pp_masked_count_ge_f32 call.

The dose is float32.  The mean is the exact sum over the count in float64 (numpy's float32 pairwise mean agrees to float32
precision); percentiles are interpolated as numpy interpolates a float32 array; a Python-float threshold is rounded to float32
before it is compared, which is what numpy does with a float32 array.  A NaN dose inside a structure raises ValueError.
"""
import numpy as np
import torch

from .. import runtime
from .dvh import _dose_f32, _scalar, masked_histogram, resample_dose


def _mask_gt0(image):
    t = image.tensor
    return (t if t.dtype == torch.uint8 else (t > 0).to(torch.uint8)).contiguous()


def _on_label(dose_grid, label):
    """-> (float32 dose tensor on the label's grid, uint8 mask tensor, the label image)"""
    label = _scalar(label, "the label")
    dose = _dose_f32(resample_dose(dose_grid, label))
    return dose, _mask_gt0(label).to(dose.device), label


def _stats(dose, mask):
    return masked_histogram(dose, [mask], [0.0, 1.0])[1][0]


def calculate_d_mean(dose_grid, label):
    """The mean dose (Gy) inside the structure; NaN for an empty one."""
    dose, mask, _ = _on_label(dose_grid, label)
    s = _stats(dose, mask)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s["dose_sum"] / np.float64(s["count"])


def calculate_d_max(dose_grid, label):
    """The maximum dose (Gy) inside the structure, as the float32 it is stored as.  ValueError for an empty structure."""
    dose, mask, _ = _on_label(dose_grid, label)
    s = _stats(dose, mask)
    if s["count"] == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    return s["dose_max"]


def _percentile(dose, mask, count, q):
    """np.percentile(dose[mask > 0], q) with the default linear method, for a float32 array of `count` values: the virtual
    index (count - 1) * (q / 100) in float64, its two neighbouring order statistics, and numpy's two-sided interpolation with
    the weight rounded to float32."""
    if not 0 <= q <= 100:
        raise ValueError("Percentiles must be in the range [0, 100]")
    virtual = (count - 1) * np.true_divide(q, 100)
    below = int(np.floor(virtual))
    above = min(below + 1, count - 1)
    a, b = runtime.context(dose.device).masked_order_stats(dose, mask, dose.numel(), [below, above])
    t = np.float32(virtual - below)
    diff = b - a
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(b - diff * (np.float32(1) - t)) if t >= 0.5 else np.float32(a + diff * t)


def calculate_d_to_volume(dose_grid, label, volume, volume_in_cc=False):
    """The dose (Gy) that `volume` of the structure receives at least: np.percentile of the doses inside it at 100 - volume.
    volume: percent of the structure, or cc with volume_in_cc (converted as volume * 1000 / (voxels * prod(spacing)) * 100);
    more than the whole structure is taken as 100 %.  ValueError for an empty structure."""
    dose, mask, label = _on_label(dose_grid, label)
    count = int(_stats(dose, mask)["count"])
    if volume_in_cc:
        with np.errstate(divide="ignore"):
            volume = (volume * 1000 / (np.int64(count) * np.prod(label.GetSpacing()))) * 100
    if volume > 100:
        volume = 100
    if count == 0:
        raise ValueError("calculate_d_to_volume: the structure is empty")
    return _percentile(dose, mask, count, 100 - volume)


def _volumes_receiving(dose, masks, thresholds, voxel_cc, relative):
    """[len(masks), len(thresholds)] of calculate_v_receiving_dose's values: one kernel call per 64 masks.  The last threshold
    handed to the kernel is -inf, whose count is the number of voxels of the mask."""
    from .. import _lib

    ctx = runtime.context(dose.device)
    t = np.concatenate([np.asarray(thresholds, dtype=np.float64).astype(np.float32), np.float32([-np.inf])])
    counts = np.concatenate([ctx.masked_count_ge(dose, masks[k:k + _lib.DOSE_MAX_LABELS], dose.numel(), t)
                             for k in range(0, len(masks), _lib.DOSE_MAX_LABELS)])
    voxels = counts[:, -1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        percent = counts[:, :-1] / voxels * 100
    if relative:
        return percent
    return percent * (voxels * voxel_cc)


def calculate_v_receiving_dose(dose_grid, label, dose_threshold, relative=True):
    """The part of the structure that receives at least `dose_threshold` Gy, in percent of its voxels.

    relative=False returns what the reference returns: that PERCENTAGE multiplied by the structure's volume in cc -- one
    hundred times the volume in cc that receives the dose, not the volume itself.  Reproduced, not corrected."""
    dose, mask, label = _on_label(dose_grid, label)
    return _volumes_receiving(dose, [mask], [dose_threshold], np.prod(label.GetSpacing()) / 1000, relative)[0, 0]


def _as_list(x):
    return x if isinstance(x, list) else [x]


def calculate_d_to_volume_for_labels(dose_grid, labels, volume, volume_in_cc=False):
    """calculate_d_to_volume for every structure of the dict `labels` and every volume (a number or a list) -> DataFrame with
    `label` and one `D{volume}` (`D{volume}cc`) column per volume."""
    import pandas as pd

    rows = []
    for name in labels:
        row = {"label": name}
        for v in _as_list(volume):
            row[f"D{v}cc" if volume_in_cc else f"D{v}"] = calculate_d_to_volume(dose_grid, labels[name], v, volume_in_cc=volume_in_cc)
        rows.append(row)
    return pd.DataFrame(rows)


def calculate_v_receiving_dose_for_labels(dose_grid, labels, dose_threshold, relative=True):
    """calculate_v_receiving_dose for every structure of the dict `labels` and every threshold (a number or a list) ->
    DataFrame with `label` and one `V{threshold}` column per threshold (`V{int(threshold)}` for a whole one).  Structures that
    share one grid go through one resampling of the dose and one kernel call; others are taken one by one."""
    import pandas as pd

    thresholds = _as_list(dose_threshold)
    names = list(labels)
    images = [_scalar(labels[k], f"label {k!r}") for k in names]
    if images and all(im.same_grid(images[0]) for im in images):
        dose = _dose_f32(resample_dose(dose_grid, images[0]))
        masks = [_mask_gt0(im).to(dose.device) for im in images]
        values = _volumes_receiving(dose, masks, thresholds, np.prod(images[0].GetSpacing()) / 1000, relative)
    else:
        values = [[calculate_v_receiving_dose(dose_grid, im, t, relative) for t in thresholds] for im in images]
    rows = []
    for name, vals in zip(names, values):
        row = {"label": name}
        for t, v in zip(thresholds, vals):
            row[f"V{int(t)}" if t - int(t) == 0 else f"V{t}"] = v
        rows.append(row)
    return pd.DataFrame(rows)
