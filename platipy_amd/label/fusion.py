"""Drop-in for platipy/imaging/label/fusion.py: compute_weight_map (:56-202), combine_labels (:239-292),
combine_labels_staple (:205-236) and process_probability_image (:295-328) on volumes resident in HBM.

The reference's vote_type="patch_correlation" (:82-146) -- one scipy.stats.pearsonr call per voxel of the 3 mm resampled
image -- is compute_patch_correlation_weight_map (pp_patch_correlation_f32): both images through smooth_and_resample, the
window int(patch_window_mm / spacing) per axis, Pearson r of the two patches clipped to the image (the reference's zero
padding and mask of ones), exactly 0 where scipy gives NaN (a patch that is exactly constant), fp64 moments rounded to
fp32 once, then resample_image back onto the target grid and `correlation_function` (an Image in, an Image or a tensor
out).  weight_map_for_vote is the dispatcher the pipelines call: it sends that vote type there and every other one to
compute_weight_map.  compute_weight_map itself still refuses vote_type="patch_correlation" with NotImplementedError, and
mutual_information still raises it: tests/test_fusion.py and tests/test_staple.py pin both, so the new code sits beside
them -- histogram_mutual_information (:26-53) builds np.histogram2d's integer table on the GPU (pp_joint_histogram_f32,
also joint_histogram) and evaluates the reference's formula on the host in fp64.

STAPLE (`staple`, sitk.STAPLE / itk::STAPLEImageFilter, Warfield et al. 2004), as implemented by pp_staple_fuse.
With R raters, N voxels and D_ij = 1 iff fg - 1e-10 < v_ij < fg + 1e-10 (compared in double):
  1. W_i = (sum_j D_ij) / R;  g = (sum_i W_i / N) * confidence_weight, with sum_i W_i formed exactly as
     (sum of the popcounts) / R.  g is not updated afterwards.
  2. last_p_j = last_q_j = -10.
  3. for iter = 0, 1, ... while iter < maximum_iterations:
       M step  p_j = sum_i W_i D_ij / sum_i W_i,  q_j = sum_i (1 - W_i)(1 - D_ij) / sum_i (1 - W_i)  (both denominators summed)
       E step  a_i = prod_j (D_ij ? p_j : 1 - p_j),  b_i = prod_j (D_ij ? 1 - q_j : q_j)  (from 1.0, in rater order),
               W_i = g a_i / (g a_i + (1 - g) b_i)
       stop when |last_p_j - p_j| < 1e-14 and |last_q_j - q_j| < 1e-14 for every j, else last = current.
  4. elapsed_iterations = iter at the break (maximum_iterations if it never breaks); sensitivity = p, specificity = q.
Every quantity is a function of a voxel's rater bits, so the GPU packs them into one 64-bit key per voxel, runs the EM
loop over the compacted keys of the voxels some but not all raters mark, and adds the two uniform classes analytically
(hence at most 64 raters).  The sums are fixed-order trees: repeated runs are bit-identical.
Two deliberate deviations from ITK, both where ITK gives NaN or never stops:
  * degenerate input -- sum W or sum (1 - W) is 0 at the first M step (no rater marks anything, or every rater marks
    everything): EM is skipped, W = W_initial (all 0 or all 1), p = q = NaN, and a RuntimeWarning is issued.  ITK
    returns an all-NaN image.
  * a floating-point 2-cycle -- (p, q) equal, bit for bit, the iterate of two steps earlier -- also stops the loop.
    ITK would iterate forever.
combine_labels_staple binarises each label as sitk.BinaryThreshold(label, lowerThreshold=0.5) does, 0.5 <= v <= 255
(BinaryThreshold's default upper bound), compared in double as pp_binary_threshold_f32 compares; whether SimpleITK first
casts 0.5 to an integer pixel type is not pinned.
"""
import math
import warnings
from collections import namedtuple

import numpy as np
import torch

from .. import _lib, runtime
from ..image import Image, as_image

DEFAULT_VOTE_PARAMS = {
    "sigma": 2.0,
    "epsilon": 1e-5,
    "factor": 1e12,
    "gain": 6,
    "blockSize": 5,
    "normalise": False,
    "patch_window_mm": 25,
    "resampled_voxel_size_mm": 3,
    "correlation_function": lambda x: x + 1,
}


def _f32(image):
    t = image.tensor
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


def compute_weight_map(target_image, moving_image, vote_type="unweighted", vote_params=None):
    """Computes the weight map (reference fusion.py:56-202).  fp32 result on the target grid."""
    target_image, moving_image = as_image(target_image), as_image(moving_image)
    p = dict(DEFAULT_VOTE_PARAMS)
    if vote_params:
        p.update(vote_params)
    ctx = runtime.context(target_image.device)
    t, m = _f32(target_image), _f32(moving_image)   # :77-80 (quirk N1: everything in float32)
    n = t.numel()
    vt = vote_type.lower()

    if vt == "patch_correlation":
        raise NotImplementedError("compute_weight_map does not take vote_type='patch_correlation': call "
                                  "compute_patch_correlation_weight_map, or weight_map_for_vote as the pipelines do")
    if vt == "unweighted":
        weight = t * 0.0 + 1.0                                                      # :151-152
    elif vt == "global":
        ssd = ctx.sum_sq_diff(t, m, n)                                              # :154-161, fp64 sum (quirk N5)
        weight = t * 0.0 + (p["factor"] / ssd)
    elif vt == "local":
        weight = torch.empty_like(t)
        ctx.weight_map_local(t, m, target_image.GetSize(), target_image.spacing, p["sigma"], p["epsilon"], weight)  # :163-169
        weight = _normalise(weight, p["normalise"])                                 # :171-177
    elif vt == "block":
        bs = p["blockSize"]
        bs = (bs,) * 3 if isinstance(bs, int) else tuple(bs)                         # (x, y, z) radii of sitk.BoxMean
        weight = torch.empty_like(t)
        ctx.weight_map_block(t, m, target_image.GetSize(), bs, p["factor"], p["gain"], weight)   # :179-190
        weight = _normalise(weight, p["normalise"])
    else:
        raise ValueError(f"unknown vote_type {vote_type!r}")
    return target_image.like(weight.float().contiguous())


def weight_map_for_vote(target_image, moving_image, vote_type="unweighted", vote_params=None):
    """The reference's compute_weight_map with every vote type it has: "patch_correlation" goes to
    compute_patch_correlation_weight_map, anything else to compute_weight_map."""
    if vote_type.lower() == "patch_correlation":
        return compute_patch_correlation_weight_map(target_image, moving_image, vote_params)
    return compute_weight_map(target_image, moving_image, vote_type, vote_params)


def compute_patch_correlation_weight_map(target_image, moving_image, vote_params=None):
    """The reference's compute_weight_map(vote_type="patch_correlation") (fusion.py:82-146): both images cast to fp32 and
    resampled to isotropic voxels, local Pearson r, back to the target grid, then correlation_function (the reference's
    default adds 1: similar modalities; abs suits MR against CT).  vote_params overrides patch_window_mm (25),
    resampled_voxel_size_mm (3) and correlation_function of DEFAULT_VOTE_PARAMS.  fp32 result on the target grid."""
    from ..registration.utils import resample_image, smooth_and_resample

    target_image, moving_image = as_image(target_image), as_image(moving_image)
    p = dict(DEFAULT_VOTE_PARAMS)
    if vote_params:
        p.update(vote_params)
    ctx = runtime.context(target_image.device)
    target_image, moving_image = target_image.like(_f32(target_image)), moving_image.like(_f32(moving_image))   # :77-80
    voxel_size = p["resampled_voxel_size_mm"]
    target_res = smooth_and_resample(target_image, isotropic_voxel_size_mm=voxel_size)          # :87-88
    moving_res = smooth_and_resample(moving_image, isotropic_voxel_size_mm=voxel_size)
    if not target_res.same_grid(moving_res):
        raise ValueError(f"patch_correlation: the resampled images are on different grids ({target_res!r}, {moving_res!r})")
    window = [int(p["patch_window_mm"] / s) for s in target_res.GetSpacing()]                   # :97-98, (x, y, z) here
    if min(window) < 1:
        raise ValueError(f"patch_correlation: patch_window_mm={p['patch_window_mm']} is below the resampled spacing "
                         f"{target_res.GetSpacing()}")
    corr = torch.empty_like(target_res.tensor)
    ctx.patch_correlation(_f32(target_res), _f32(moving_res), target_res.GetSize(), window, corr)   # :100-132
    corr_image = resample_image(target_res.like(corr), target_image)                            # :138: linear, default 0
    weight = p["correlation_function"](corr_image)                                              # :144-146
    if isinstance(weight, Image):
        weight = weight.tensor
    if not torch.is_tensor(weight) or tuple(weight.shape) != tuple(target_image.tensor.shape):
        raise TypeError("correlation_function must return an Image or a tensor on the target grid")
    return target_image.like(weight.float().contiguous())


def _normalise(weight, normalise):
    if isinstance(normalise, bool):
        if normalise:
            weight = weight / weight.max()
    elif isinstance(normalise, Image):
        mask = normalise.tensor != 0
        weight = weight / weight[mask].max()
    return weight


def label_tensor(image):
    """An atlas label as the fusion kernels take it: uint8 / bool masks stay uint8 (one byte per voxel through HBM);
    anything else is weighted as sitk.Cast(label, sitkFloat32) weights it (reference fusion.py:269-272) -- a
    probabilistic label of 0.7 contributes 0.7 w, an int16 label of 256 contributes 256 w."""
    t = as_image(image).tensor
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype != torch.uint8:
        t = t.to(torch.float32)
    return t.contiguous()


def _accumulate(ctx, atlas_set, case_ids, label, s_name):
    """Left fold over the atlases, as functools.reduce over sitk images does (:263, :269-276)."""
    first = atlas_set[case_ids[0]][label]["Weight Map"]
    wsum = torch.zeros(first.shape, dtype=torch.float32, device=first.device)
    wlsum = torch.zeros_like(wsum)
    n = wsum.numel()
    for cid in case_ids:
        w = _f32(as_image(atlas_set[cid][label]["Weight Map"]))
        ctx.fuse_accumulate(w, label_tensor(atlas_set[cid][label][s_name]), wsum, wlsum, n)
    return first, wsum, wlsum


def finalize_probability(ctx, ref, wsum, wlsum, threshold=1e-4, smooth_sigma=1.0):
    """P = wlsum / guarded(wsum) -> DiscreteGaussian(sigma^2) -> RescaleIntensity(0,1) -> Threshold (:264-288)."""
    n = wsum.numel()
    prob = torch.empty_like(wsum)
    ctx.fuse_divide(wlsum, wsum, prob, n)
    var = smooth_sigma * smooth_sigma
    ctx.discrete_gaussian(prob, prob, ref.GetSize(), ref.spacing, (var, var, var), 0.01, 32, True)
    lo, hi = ctx.minmax(prob, n)
    # sitk.Threshold(lower=threshold, upper=1, outsideValue=0); a falsy threshold skips it (lower = -inf here)
    ctx.rescale_threshold(prob, n, lo, hi, threshold if threshold else -3.0e38)
    return ref.like(prob)


def combine_labels(atlas_set, structure_name, label="DIR", threshold=1e-4, smooth_sigma=1.0):
    """Combine labels using weight maps (reference fusion.py:239-292).
    atlas_set[case_id][label] is a dict holding "Weight Map" and one Image per structure."""
    case_id_list = list(atlas_set.keys())
    if isinstance(structure_name, str):
        structure_name_list = [structure_name]
    elif isinstance(structure_name, list):
        structure_name_list = structure_name
    else:
        raise TypeError("structure_name must be a str or a list of str")
    combined_label_dict = {}
    for s_name in structure_name_list:
        valid = [i for i in case_id_list if s_name in atlas_set[i][label].keys()]
        if not valid:
            raise KeyError(f"no atlas holds structure {s_name!r}")
        ref = as_image(atlas_set[valid[0]][label]["Weight Map"])
        ctx = runtime.context(ref.device)
        ref, wsum, wlsum = _accumulate(ctx, atlas_set, valid, label, s_name)
        combined_label_dict[s_name] = finalize_probability(ctx, as_image(ref), wsum, wlsum, threshold, smooth_sigma)
    return combined_label_dict


def process_probability_image(probability_image, threshold=0.5):
    """Generate a mask given a probability image (reference fusion.py:295-328): /max, BinaryThreshold(>= thr),
    BinaryFillhole, ConnectedComponent, keep the largest component, uint8 -- all on the GPU (union-find labelling,
    pp_fillhole_largest_component_u8)."""
    if not isinstance(probability_image, Image):
        probability_image = Image(torch.as_tensor(np.asarray(probability_image)).to(runtime.default_device()))
    ctx = runtime.context(probability_image.device)
    prob = _f32(probability_image)
    n = prob.numel()
    if threshold > 0 and n >= CROP_MIN_VOXELS:
        # A fused probability is zero outside the (smoothed) union of the atlas labels -- a few per cent of a 512 x 512 x 256
        # volume -- and every voxel that can pass a POSITIVE threshold lies in the box around its support.  On that box (one
        # voxel wider, so that its rim is background connected to the outside) the threshold, the fill-hole, the labelling and
        # the largest component are those of the whole volume: everything outside is background reaching the image border.
        from ..utils.crop import crop_to_roi

        size = probability_image.GetSize()
        box = ctx.bounding_box(prob, size, True)
        if box[0] <= box[1]:
            lo = [max(0, box[2 * k] - 1) for k in range(3)]
            ext = [min(size[k] - 1, box[2 * k + 1] + 1) - lo[k] + 1 for k in range(3)]
            if ext[0] * ext[1] * ext[2] <= n // 2:
                inner = _process_probability_image(crop_to_roi(probability_image.like(prob), ext, lo), threshold)
                out = torch.zeros(prob.shape, dtype=torch.uint8, device=prob.device)
                out[lo[2]:lo[2] + ext[2], lo[1]:lo[1] + ext[1], lo[0]:lo[0] + ext[0]] = inner.tensor
                return probability_image.like(out)
    return _process_probability_image(probability_image.like(prob), threshold)


CROP_MIN_VOXELS = 1 << 22


def _process_probability_image(probability_image, threshold):
    ctx = runtime.context(probability_image.device)
    prob = _f32(probability_image)
    n = prob.numel()
    _, hi = ctx.minmax(prob, n)
    binary = torch.empty(prob.shape, dtype=torch.uint8, device=prob.device)
    ctx.binary_threshold(prob, n, hi, threshold, binary)
    out = torch.empty_like(binary)
    ctx.fillhole_largest_component(binary, probability_image.GetSize(), out, fill_holes=True)
    return probability_image.like(out)


StapleResult = namedtuple("StapleResult", "image sensitivity specificity elapsed_iterations")


def _staple_inputs(labels):
    """Validated rater tensors: bool / uint8 as bytes, anything else through fp32 (as label_tensor reads labels)."""
    labels = [as_image(x) for x in labels]
    if not labels:
        raise ValueError("STAPLE needs at least one rater")
    if len(labels) > _lib.STAPLE_MAX_RATERS:
        raise ValueError(f"STAPLE takes at most {_lib.STAPLE_MAX_RATERS} raters, got {len(labels)}")
    ref = labels[0]
    for x in labels:
        if x.is_vector:
            raise ValueError("STAPLE labels are scalar images")
        if not ref.same_grid(x):
            raise ValueError("STAPLE labels must share one grid (size, spacing, origin, direction)")
        if x.device != ref.device:
            raise ValueError(f"STAPLE labels are on different devices ({ref.device}, {x.device})")
    is_float = any(x.tensor.dtype not in (torch.uint8, torch.bool) for x in labels)
    ts = [label_tensor(x) for x in labels]
    if is_float:
        ts = [t.to(torch.float32).contiguous() for t in ts]
    return ref, ts, is_float


def _staple_run(labels, foreground_test, foreground_value=1.0, confidence_weight=1.0, maximum_iterations=None, rescale=False,
                threshold_lower=-math.inf):
    ref, ts, is_float = _staple_inputs(labels)
    ctx = runtime.context(ref.device)
    out = torch.empty(ts[0].shape, dtype=torch.float64, device=ts[0].device)
    res = ctx.staple(ts, is_float, out.numel(), out, foreground_test, foreground_value, confidence_weight, maximum_iterations,
                     rescale, threshold_lower)
    if res.degenerate:
        warnings.warn("STAPLE: no rater marks any voxel, or every rater marks every voxel; returning the initial estimate "
                      "with NaN sensitivity and specificity", RuntimeWarning, stacklevel=3)
    r = len(ts)
    return StapleResult(ref.like(out), [res.sensitivity[j] for j in range(r)], [res.specificity[j] for j in range(r)],
                        int(res.elapsed_iterations))


def staple(labels, confidence_weight=1.0, foreground_value=1.0, maximum_iterations=None):
    """sitk.STAPLE(labels, confidenceWeight, foregroundValue, maximumIterations) on the GPU (see the module notes).
    labels: 1..64 Images on one grid and device.  maximum_iterations None = until convergence (ITK: 2^32 - 1).
    -> StapleResult(image = float64 W, sensitivity, specificity (lists of float, one per rater), elapsed_iterations)."""
    return _staple_run(labels, _lib.STAPLE_FOREGROUND, foreground_value, confidence_weight, maximum_iterations)


def combine_labels_staple(label_list_dict, threshold=1e-4):
    """Combine labels using STAPLE (reference fusion.py:205-236).  label_list_dict[atlas][structure] is a label Image;
    every atlas must hold every structure (KeyError otherwise).  Per structure: BinaryThreshold(lowerThreshold=0.5),
    STAPLE with its defaults, RescaleIntensity(0, 1) and, if `threshold`, Threshold(threshold, 1, outside 0) -- fused in
    the last pass.  -> {structure name (sorted, np.unique): float64 Image on the first atlas's grid}."""
    structure_name_list = [list(i.keys()) for i in label_list_dict.values()]
    structure_name_list = np.unique([item for sublist in structure_name_list for item in sublist])
    combined_label_dict = {}
    for structure_name in structure_name_list:
        labels = [label_list_dict[i][structure_name] for i in label_list_dict]
        combined_label_dict[structure_name] = _staple_run(labels, _lib.STAPLE_BINARY_THRESHOLD, rescale=True,
                                                          threshold_lower=threshold if threshold else -math.inf).image
    return combined_label_dict


def _flat_f32(x):
    """Image, tensor or ndarray -> flat float32 tensor on the device the kernels run on."""
    if isinstance(x, Image):
        x = x.tensor
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.device.type == "cpu":
        x = x.to(runtime.default_device())
    return x.reshape(-1).to(torch.float32).contiguous()


def _bin_counts(bins):
    """np.histogram2d's `bins` as (bins_a, bins_b): an int, or a pair of ints."""
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool):
        pair = (int(bins), int(bins))
    elif (isinstance(bins, (list, tuple)) and len(bins) == 2
          and all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) for b in bins)):
        pair = (int(bins[0]), int(bins[1]))
    else:
        raise NotImplementedError("mutual_information: `bins` given as edge arrays is not implemented; pass an int or a pair of ints")
    if min(pair) < 1:
        raise ValueError("mutual_information: `bins` must be positive")
    return pair


def joint_histogram(arr_a, arr_b, bins=64):
    """np.histogram2d(arr_a, arr_b, bins) -> (int64 counts [bins_a, bins_b], edges_a, edges_b), counted on the GPU.
    The samples are taken as float32 (what an Image holds) and binned as doubles against numpy's fp64 linspace edges, so
    the counts equal numpy's on the same values.  NaN or infinite samples raise ValueError, as numpy does."""
    bins_a, bins_b = _bin_counts(bins)
    a, b = _flat_f32(arr_a), _flat_f32(arr_b)
    if a.numel() != b.numel() or a.numel() == 0:
        raise ValueError("mutual_information: the arrays must hold the same, non-zero number of samples")
    if a.device != b.device:
        raise ValueError(f"mutual_information: the arrays are on different devices ({a.device}, {b.device})")
    hist, rng = runtime.context(a.device).joint_histogram(a, b, a.numel(), bins_a, bins_b)
    return hist, np.linspace(rng[0], rng[1], bins_a + 1), np.linspace(rng[2], rng[3], bins_b + 1)


def mutual_information(arr_a, arr_b, bins=64):
    raise NotImplementedError("mutual_information is not wired to the GPU path: call histogram_mutual_information")


def histogram_mutual_information(arr_a, arr_b, bins=64):
    """The reference's mutual_information (fusion.py:26-53), the histogram-based mutual information between two arrays:
    Images, tensors or ndarrays, flattened; bins an int or a pair of ints.  -> float.

    The joint histogram is counted on the GPU (joint_histogram); the value is the reference's formula, as written, in fp64
    on the host: np.histogram2d(density=True) divides the counts by the bin areas and the total, and the marginals are
    named by numpy axis, p_a = p_ab.sum(axis=0) and p_b = p_ab.sum(axis=1), so outer(p_a, p_b) pairs row i, column j with
    the marginals of column i and row j -- the transpose of the product of marginals.  That is kept: for a symmetric table
    it changes nothing, for an asymmetric one the value is the reference's, and for bins_a != bins_b the division cannot
    broadcast and raises ValueError as it does in the reference."""
    hist, edges_a, edges_b = joint_histogram(arr_a, arr_b, bins)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # np.histogramdd(density=True): counts / bin widths, axis by axis, then / total
        p_ab = hist.astype(np.float64)
        total = p_ab.sum()
        p_ab = p_ab / np.diff(edges_a).reshape(-1, 1)
        p_ab = p_ab / np.diff(edges_b).reshape(1, -1)
        p_ab /= total
        p_a = p_ab.sum(axis=0)
        p_b = p_ab.sum(axis=1)
        log_p = np.log(p_ab / np.outer(p_a, p_b))
    log_p[~np.isfinite(log_p)] = 0
    return (p_ab * log_p).sum()
