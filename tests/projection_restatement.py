"""TEST ONLY: what pp_project_set reduces a ray to, restated in numpy on a volume that is ALREADY resampled (the samples
themselves are pp_resample_f32 / pp_resample_u8's, held to their own fp64 restatement in tests/test_resample_kernels.py),
and the one-slice geometry rule of platipy_amd.visualisation (P2).

  sum     the fp64 sum in index order (np.cumsum adds sequentially), rounded once to fp32
  mean    that sum / n
  std     sqrt(sum((v - mean)^2) / (n - 1)), fp64, index order; 0 / 0 = NaN for n = 1
  median  np.partition's element n // 2 (the upper median, no averaging; numpy sorts NaN last)
  min/max np.min / np.max (a NaN sample gives NaN)
"""
import numpy as np

KINDS = ("sum", "mean", "median", "std", "min", "max")


def np_axis(axis):
    """projection axis 0 = x, 1 = y, 2 = z of a [Z][Y][X] array"""
    return 2 - axis


def reduce64(vol, kind, axis):
    """sum / mean / std before the rounding to fp32 (float64 plane)"""
    ax = np_axis(axis)
    v = np.asarray(vol).astype(np.float64)
    n = v.shape[ax]
    with np.errstate(all="ignore"):
        s = np.take(np.cumsum(v, axis=ax), -1, axis=ax)
        if kind == "sum":
            return s
        mean = s / np.float64(n)
        if kind == "mean":
            return mean
        d = v - np.expand_dims(mean, ax)
        ss = np.take(np.cumsum(d * d, axis=ax), -1, axis=ax)
        return np.sqrt(ss / (np.float64(n) - 1.0))


def reduce(vol, kind, axis):
    """The fp32 plane pp_project_set writes for an fp32 volume of samples."""
    ax = np_axis(axis)
    vol = np.asarray(vol)
    n = vol.shape[ax]
    with np.errstate(all="ignore"):
        if kind == "min":
            return np.min(vol, axis=ax).astype(np.float32)
        if kind == "max":
            return np.max(vol, axis=ax).astype(np.float32)
        if kind == "median":
            return np.take(np.partition(vol.astype(np.float32), n // 2, axis=ax), n // 2, axis=ax)
        return reduce64(vol, kind, axis).astype(np.float32)


def label_max(vol, axis):
    return np.max(np.asarray(vol), axis=np_axis(axis))


def one_slice_geometry(size, spacing, origin, direction, axis):
    """-> (size, spacing, origin) of the projection as an image of the input's dimension: itk::ProjectionImageFilter as
    recalled (unpinned)."""
    size, spacing = list(size), [float(s) for s in spacing]
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    org = np.asarray(origin, dtype=np.float64) + d[:, axis] * ((size[axis] - 1) * spacing[axis] / 2.0)
    spacing[axis] *= size[axis]
    size[axis] = 1
    return tuple(size), tuple(spacing), tuple(org)
