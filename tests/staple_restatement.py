"""Numpy restatements of STAPLE (itk::STAPLEImageFilter, as platipy_amd.label.fusion's module notes state it) for the
tests of tests/test_staple.py.  Imports nothing from platipy_amd.

staple_voxels    -- the algorithm voxel by voxel, fp64 arrays over all N voxels
staple_patterns  -- the same EM on the histogram of the raters' bit patterns (np.unique of the 64-bit keys), cheap enough
                    for a 512 x 512 x 256 volume
Both return (W as an array shaped like the labels, p, q, elapsed_iterations, degenerate).
"""
import numpy as np

EPS = 1e-14


def foreground(label, mode="staple", foreground_value=1.0):
    """D: sitk.STAPLE's fg - 1e-10 < v < fg + 1e-10, or ("binary") sitk.BinaryThreshold(lower=0.5)'s 0.5 <= v <= 255, in double."""
    v = np.asarray(label).astype(np.float64)
    if mode == "binary":
        return (v >= 0.5) & (v <= 255.0)
    return (v > foreground_value - 1e-10) & (v < foreground_value + 1e-10)


def _weight(dbits, p, q, g):
    """W for rows of D (M x R bool): products from 1.0 in rater order."""
    a = np.ones(dbits.shape[0])
    b = np.ones(dbits.shape[0])
    for j in range(dbits.shape[1]):
        a = a * np.where(dbits[:, j], p[j], 1.0 - p[j])
        b = b * np.where(dbits[:, j], 1.0 - q[j], q[j])
    ga = g * a
    gb = (1.0 - g) * b
    return ga / (ga + gb)


def _em(dbits, counts, n, confidence_weight, maximum_iterations):
    """EM over rows of D with multiplicities `counts` (all 1 for the voxel restatement)."""
    r = dbits.shape[1]
    pc = dbits.sum(axis=1).astype(np.int64)
    w = pc / float(r)
    g = (float(np.sum(pc * counts)) / r) / n * confidence_weight
    cf = counts.astype(np.float64)
    last_p = np.full(r, -10.0)
    last_q = np.full(r, -10.0)
    prev2 = None
    p = q = np.full(r, np.nan)
    it = 0
    maximum_iterations = np.inf if maximum_iterations is None else maximum_iterations
    while it < maximum_iterations:
        sw = np.sum(cf * w)
        sw1 = np.sum(cf * (1.0 - w))
        if it == 0 and (sw == 0.0 or sw1 == 0.0):
            return w, np.full(r, np.nan), np.full(r, np.nan), 0, True
        p = np.array([np.sum(cf * w * dbits[:, j]) for j in range(r)]) / sw
        q = np.array([np.sum(cf * (1.0 - w) * ~dbits[:, j]) for j in range(r)]) / sw1
        w = _weight(dbits, p, q, g)
        converged = np.all(np.abs(last_p - p) < EPS) and np.all(np.abs(last_q - q) < EPS)
        cycle = prev2 is not None and it >= 2 and p.tobytes() == prev2[0].tobytes() and q.tobytes() == prev2[1].tobytes()
        if converged or cycle:
            break
        prev2 = (last_p, last_q)
        last_p, last_q = p, q
        it += 1
    return w, p, q, it, False


def _stack(labels, mode, foreground_value):
    return np.stack([foreground(x, mode, foreground_value).ravel() for x in labels], axis=1)


def staple_voxels(labels, confidence_weight=1.0, foreground_value=1.0, maximum_iterations=None, mode="staple"):
    d = _stack(labels, mode, foreground_value)
    w, p, q, it, deg = _em(d, np.ones(d.shape[0], dtype=np.int64), d.shape[0], confidence_weight, maximum_iterations)
    return w.reshape(np.shape(labels[0])), p, q, it, deg


def keys_of(labels, mode="staple", foreground_value=1.0):
    """One uint64 per voxel, rater j in bit j."""
    keys = np.zeros(np.size(labels[0]), dtype=np.uint64)
    for j, x in enumerate(labels):
        keys |= foreground(x, mode, foreground_value).ravel().astype(np.uint64) << np.uint64(j)
    return keys


def staple_patterns(labels, confidence_weight=1.0, foreground_value=1.0, maximum_iterations=None, mode="staple"):
    r = len(labels)
    keys = keys_of(labels, mode, foreground_value)
    uniq, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    d = ((uniq[:, None] >> np.arange(r, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    w, p, q, it, deg = _em(d, counts, keys.size, confidence_weight, maximum_iterations)
    return w[inverse.ravel()].reshape(np.shape(labels[0])), p, q, it, deg


def rescale_threshold(w, threshold=1e-4):
    """RescaleIntensity(w, 0, 1) (ITK's scale / shift rule, in double, clamped) then, if threshold, Threshold(threshold, 1, 0)."""
    lo, hi = float(np.min(w)), float(np.max(w))
    if lo != hi:
        scale = 1.0 / (hi - lo)
    elif hi != 0.0:
        scale = 1.0 / hi
    else:
        scale = 0.0
    shift = 0.0 - lo * scale
    r = np.clip(w * scale + shift, 0.0, 1.0)
    if threshold:
        r = np.where((r < threshold) | (r > 1.0), 0.0, r)
    return r


def raters_from_truth(shape, n_raters, seed, shift=2, flip=1e-4):
    """uint8 raters made from one smooth structure: an ellipsoid with a separable wobble, each rater shifted (up to
    `shift` voxels per axis) and eroded / dilated by a level offset, plus sparse random flips.  Mixed voxels are a few
    per cent of the volume."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = (np.arange(s, dtype=np.float32) for s in shape)
    out = []
    for _ in range(n_raters):
        dz, dy, dx = rng.integers(-shift, shift + 1, size=3)
        level = np.float32(1.0 + rng.uniform(-0.04, 0.04))
        fx = ((x - (nx / 2 + dx)) / (0.35 * nx)) ** 2 + 0.08 * np.sin(x / 7.0)
        fy = ((y - (ny / 2 + dy)) / (0.30 * ny)) ** 2 + 0.08 * np.sin(y / 5.0)
        fz = ((z - (nz / 2 + dz)) / (0.35 * nz)) ** 2 + 0.08 * np.sin(z / 6.0)
        lab = ((fz[:, None, None] + fy[None, :, None]) + fx[None, None, :]) < level
        n = lab.size
        idx = rng.integers(0, n, size=int(flip * n))
        flat = lab.reshape(-1)
        flat[idx] = ~flat[idx]
        out.append(lab.astype(np.uint8))
    return out
