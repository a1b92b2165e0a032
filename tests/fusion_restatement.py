"""Plain numpy / fp64 restatements of the label-fusion arithmetic (the map and reduction kernels at the head of
platipy_amd/csrc/pp_fusion.hip), the references of tests/test_fusion_kernels.py.  One function per operation, written from
what SimpleITK's filters are documented to compute in the reference's compute_weight_map, combine_labels and
process_probability_image -- SquaredDifference, DiscreteGaussian, BoxMean, Pow, the image sums and products,
RescaleIntensity, Threshold, BinaryThreshold, MinimumMaximum -- not from the kernels.  The only project code used is the
library's Gaussian taps (host code, the same doubles in every build), so that `local_weight` compares the convolution and
not the operator; tests/test_smoothing_kernels.py holds the taps themselves to exact Bessel values.

All volumes are [Z][Y][X]; `size`, `spacing` and `radius` are (x, y, z) as the C ABI takes them.  Where the product may
legitimately round in two ways (a multiply-add that the compiler may or may not contract) the function returns both.
"""
import math
from fractions import Fraction

import numpy as np
from scipy.ndimage import correlate1d

from tests import smoothing_restatement as S

FLT_MAX = float(np.finfo(np.float32).max)


def squared_difference(t, m):
    """itk::SquaredDifferenceImageFilter on fp32 pixels: fp32 (t - m), then its fp32 square."""
    with np.errstate(over="ignore"):
        d = np.asarray(t, np.float32) - np.asarray(m, np.float32)
        return d * d


def gaussian_taps(lib, sigma, spacing):
    """The taps of sitk.DiscreteGaussian(image, sigma^2) per numpy axis (z, y, x): variance sigma^2 in physical units, image
    spacing on, maximum error 0.01, maximum kernel width 32; fp32 as the library stores them, widened to fp64."""
    from platipy_amd import _lib

    return {2 - a: np.float32(_lib.gauss_taps(sigma * sigma / (spacing[a] * spacing[a]), 0.01, 32, lib=lib)).astype(np.float64)
            for a in range(3)}


def local_weight(t, m, size, spacing, sigma, eps, lib=None):
    """vote_type "local": 1 / (G(squared difference) + eps) in fp64, G the fp64 FIR restatement (z, then y, then x, as
    DiscreteGaussian convolves).  -> (weight, raw = G(...), radii per numpy axis)."""
    sq = squared_difference(t, m).reshape(size[2], size[1], size[0])
    taps = gaussian_taps(lib, sigma, spacing)
    raw = S.fir_separable(sq, taps, (0, 1, 2))
    with np.errstate(divide="ignore"):
        return 1.0 / (raw + float(eps)), raw, [(taps[k].size - 1) // 2 for k in range(3)]


def box_mean(img, radius):
    """sitk.BoxMean: the fp64 mean over (2 rx + 1)(2 ry + 1)(2 rz + 1) voxels, edges replicated (ZeroFluxNeumann)."""
    out = np.asarray(img, np.float64)
    for a in range(3):                       # a = x, y, z -> numpy axis 2 - a
        w = 2 * int(radius[a]) + 1
        out = correlate1d(out, np.full(w, 1.0 / w), axis=2 - a, mode="nearest")
    return out


def block_weight(t, m, size, radius, factor, gain):
    """vote_type "block": factor * (1 / box mean of the squared difference) ^ |gain / 2|, as std::pow gives it: +inf where the
    mean is 0 and the power positive, factor where the power is 0.  -> (weight, mean), fp64."""
    sq = squared_difference(t, m).reshape(size[2], size[1], size[0])
    mean = box_mean(sq, radius)
    p = abs(gain / 2.0)
    with np.errstate(divide="ignore"):
        inv = np.where(mean == 0.0, np.inf, 1.0 / np.where(mean == 0.0, 1.0, mean))
        w = np.ones_like(mean) if p == 0.0 else inv ** p
    return float(factor) * w, mean


def ssd(a, b):
    """vote_type "global": the sum of the fp64 squared differences, math.fsum (exact sum, rounded once)."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return math.fsum((d * d).tolist())


def _round_to_f32_once(hi, lo):
    """float32 of the exact value hi + lo (fp64 hi, |lo| <= ulp(hi) / 2) with ONE rounding: hi is first replaced by the
    neighbour with an odd last bit on lo's side (round to odd), which 53 >= 24 + 2 bits make safe to round again."""
    hi = np.asarray(hi, np.float64)
    toward = np.where(lo > 0, np.inf, -np.inf)
    nb = np.nextafter(hi, toward)
    odd = (hi.view(np.int64) & 1) == 1
    return np.where((lo == 0) | odd | ~np.isfinite(hi), hi, nb).astype(np.float32)


def accumulate(w, label, wsum, wlsum):
    """One atlas of combine_labels' left fold on fp32 images: wsum + w, and wlsum + w * float32(label).
    -> (wsum', wlsum' with the product rounded to fp32 and then added, wlsum' as a fused multiply-add: w * l + acc exactly,
    rounded once).  wsum None -> wsum' None."""
    w = np.asarray(w, np.float32)
    lab = np.asarray(label).astype(np.float32)
    acc = np.asarray(wlsum, np.float32)
    two_step = acc + w * lab
    prod = w.astype(np.float64) * lab.astype(np.float64)             # exact: at most 48 significant bits
    a64 = acc.astype(np.float64)
    s = prod + a64                                                   # TwoSum: s + err is the exact sum
    bb = s - prod
    err = (prod - (s - bb)) + (a64 - bb)
    fused = _round_to_f32_once(s, err)
    return (None if wsum is None else np.asarray(wsum, np.float32) + w), two_step, fused


def divide(wl, ws):
    """wlsum / sitk.Mask(wsum, wsum == 0, maskingValue=1, outsideValue=1): the weight sum, 1 where it is 0; fp32 quotient."""
    ws = np.asarray(ws, np.float32)
    with np.errstate(all="ignore"):
        return np.asarray(wl, np.float32) / np.where(ws == 0, np.float32(1), ws)


def rescale_scale_shift(lo, hi):
    """itk::RescaleIntensityImageFilter to [0, 1], in double from the fp32 input range [lo, hi]: scale = 1 / (hi - lo); a
    constant non-zero image is divided by its value; a zero image gets scale 0; shift = 0 - lo * scale."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if lo != hi:
        scale = 1.0 / (hi - lo)
    elif hi != 0.0:
        scale = 1.0 / hi
    else:
        scale = 0.0
    return scale, 0.0 - lo * scale


def rescale_threshold(x, lo, hi, lower):
    """RescaleIntensity(0, 1) then Threshold(lower, upper = 1, outside 0) on fp32 pixels: x * scale + shift in double, clamped
    to [0, 1], rounded to fp32, 0 unless lower <= v <= 1.  -> (two roundings of x * scale + shift, one rounding)."""
    x = np.asarray(x, np.float32)
    scale, shift = rescale_scale_shift(lo, hi)
    x64 = x.astype(np.float64)
    plain = x64 * scale + shift
    if shift == 0.0 and (scale == 0.0 or math.frexp(scale)[0] == 0.5):
        fused = plain.copy()                 # a power-of-two scale and no shift: the product is exact either way
    else:
        fs, fh = Fraction(scale), Fraction(shift)
        fused = np.array([float(Fraction(float(v)) * fs + fh) if math.isfinite(v) else float(v) * scale + shift
                          for v in x64.ravel()], np.float64).reshape(x.shape)
    out = []
    for r in (plain, fused):
        v = np.clip(r, 0.0, 1.0).astype(np.float32)
        out.append(np.where((v < np.float32(lower)) | (v > np.float32(1)), np.float32(0), v).astype(np.float32))
    return out[0], out[1]


def binary_threshold(p, max_value, thr):
    """image / max (double quotient stored as the fp32 pixel), then BinaryThreshold(lowerThreshold = thr) -> uint8."""
    q = (np.asarray(p, np.float32).astype(np.float64) / float(max_value)).astype(np.float32)
    return (q.astype(np.float64) >= float(thr)).astype(np.uint8)


def minmax(x):
    """itk::MinimumMaximumImageCalculator on fp32: start at (+FLT_MAX, -FLT_MAX), replace the minimum on a strictly smaller
    pixel and the maximum on a strictly larger one.  A NaN compares false and never replaces; an all-NaN image returns the
    start pair; +inf can only become the maximum and -inf only the minimum (min over +inf alone stays FLT_MAX)."""
    v = np.asarray(x, np.float32).ravel()
    v = v[~np.isnan(v)]
    lo, hi = np.float32(FLT_MAX), np.float32(-FLT_MAX)
    if v.size:
        if v.min() < lo:
            lo = v.min()
        if v.max() > hi:
            hi = v.max()
    return float(lo), float(hi)
