"""TEST INFRASTRUCTURE: the logic of platipy/imaging/utils/lung.py and projects/bronchus/bronchus.py restated in numpy /
scipy, plus the four primitives it needs, written from the documented behaviour of the SimpleITK filters (SimpleITK is not
installed here, so parity with it is unpinned).  Arrays are [Z, Y, X]; geometry is (spacing, origin, direction) in x, y, z.

  labelling   scipy.ndimage.label, default (face) structure; first voxels are asserted to increase with the label, which is
              the order sitk.ConnectedComponent numbers in
  ITK ball    sum((d / (r + 0.5))^2) <= 1
  closing     safe border: pad by r, dilate, erode with border value 1, crop
  median      ndimage.median_filter(size = 2 r + 1, mode="nearest")"""
import math

import numpy as np
from scipy import ndimage

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def label(mask):
    lab, n = ndimage.label(np.asarray(mask) != 0)
    if n:
        flat = lab.ravel()
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        assert np.all(np.diff(first[1:]) > 0), "scipy's labels are not in raster order of first voxels"
    return lab.astype(np.int32), int(n)


def moments(labels, nlabels):
    """int64 [nlabels, 10]: count, sum x, y, z, xx, yy, zz, xy, xz, yz of labels 1 ... nlabels."""
    labels = np.asarray(labels)
    z, y, x = [a.astype(np.int64).ravel() for a in np.indices(labels.shape)]
    l = labels.ravel().astype(np.int64)
    keep = (l >= 1) & (l <= nlabels)
    out = np.zeros((nlabels, 10), dtype=np.int64)
    for k, v in enumerate((np.ones_like(x), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z)):
        np.add.at(out[:, k], l[keep] - 1, v[keep])
    return out


def covariance_matrix(row, spacing, direction):
    """The moment matrix of one label from its ten integer sums: exact-integer covariance, then spacing, the spacing^2 / 12
    term and the direction."""
    m = [int(v) for v in row]
    n = m[0]
    sp = np.asarray(spacing, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    idx = {(0, 0): 4, (1, 1): 5, (2, 2): 6, (0, 1): 7, (0, 2): 8, (1, 2): 9}
    cov = np.zeros((3, 3))
    for (i, j), s in idx.items():
        cov[i, j] = cov[j, i] = (n * m[s] - m[1 + i] * m[1 + j]) / (n * n)
    return d @ (cov * np.outer(sp, sp) + np.diag(sp * sp / 12.0)) @ d.T


def shape_statistics(labels, nlabels, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=IDENTITY):
    sp = np.asarray(spacing, dtype=np.float64)
    org = np.asarray(origin, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    out = {}
    for k, row in enumerate(moments(labels, nlabels)):
        n = int(row[0])
        st = {"count": n, "physical_size": n * float(sp[0] * sp[1] * sp[2])}
        out[k + 1] = st
        if n == 0:
            continue
        mean = np.array([int(row[1]) / n, int(row[2]) / n, int(row[3]) / n])
        st["centroid"] = tuple(org + d @ (sp * mean))
        lam = np.linalg.eigvalsh(covariance_matrix(row, spacing, direction))
        st["principal_moments"] = tuple(lam)
        st["elongation"] = math.sqrt(lam[2] / lam[1]) if lam[1] != 0 else 0.0
        st["flatness"] = math.sqrt(lam[1] / lam[0]) if lam[0] != 0 else 0.0
    return out


def physical_point_to_index(point, spacing, origin, direction):
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    m = np.linalg.inv(d @ np.diag(np.asarray(spacing, dtype=np.float64)))
    c = m @ (np.asarray(point, dtype=np.float64) - np.asarray(origin, dtype=np.float64))
    return [int(math.floor(v + 0.5)) for v in c]


def connected_threshold(img, seeds, lower, upper):
    """seeds: (x, y, z) indices inside the image."""
    v = np.asarray(img).astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (v >= lower) & (v <= upper)
    lab, _ = ndimage.label(inside)
    chosen = {int(lab[z, y, x]) for x, y, z in seeds} - {0}
    return np.isin(lab, sorted(chosen)).astype(np.uint8) if chosen else np.zeros(v.shape, np.uint8)


def itk_ball(radius):
    """radius (x, y, z) -> bool [2 rz + 1, 2 ry + 1, 2 rx + 1]"""
    rx, ry, rz = radius
    dz, dy, dx = np.meshgrid(np.arange(-rz, rz + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing="ij")
    return (dx / (rx + 0.5)) ** 2 + (dy / (ry + 0.5)) ** 2 + (dz / (rz + 0.5)) ** 2 <= 1.0


def dilate(mask, r):
    return ndimage.binary_dilation(np.asarray(mask) != 0, structure=itk_ball((r, r, r))).astype(np.uint8)


def closing(mask, r):
    p = np.pad(np.asarray(mask) != 0, r)
    se = itk_ball((r, r, r))
    p = ndimage.binary_erosion(ndimage.binary_dilation(p, structure=se), structure=se, border_value=1)
    return p[r:p.shape[0] - r, r:p.shape[1] - r, r:p.shape[2] - r].astype(np.uint8)


def median(mask, radius=(1, 1, 1)):
    rx, ry, rz = radius
    return ndimage.median_filter((np.asarray(mask) != 0).astype(np.uint8), size=(2 * rz + 1, 2 * ry + 1, 2 * rx + 1), mode="nearest")


# ---- imaging/utils/lung.py ---------------------------------------------------------------------------------------

def detect_holes(img, spacing, origin=(0.0, 0.0, 0.0), direction=IDENTITY, lower_threshold=-10000, upper_threshold=-400):
    holes = (img >= lower_threshold) & (img <= upper_threshold)
    lab, count = label(holes)
    st = shape_statistics(lab, count, spacing, origin, direction)
    labels = [{"label": r, "phys_size": st[r]["physical_size"], "elongation": st[r]["elongation"], "flatness": st[r]["flatness"]}
              for r in range(1, count)]
    return lab, sorted(labels, key=lambda i: i["phys_size"], reverse=True), count


def get_lung_mask(lab, labels, kernel_radius=2):
    lung_idx = 1
    while True:
        if lung_idx >= len(labels):
            return None
        if not labels[lung_idx]["flatness"] > 2:
            break
        lung_idx += 1
    return closing(lab == labels[lung_idx]["label"], kernel_radius)


# ---- imaging/projects/bronchus/bronchus.py -----------------------------------------------------------------------

DEFAULT_SETTINGS = {
    "fast_mode": True,
    "extend_from_carina_mm": 40,
    "minimum_tree_half_physical_size": 1000,
    "lung_mask_hu_values": [-750, -775, -800, -825, -850, -900, -700, -950, -650],
    "distance_from_supu_slice_values": [3, 10, 20],
    "expected_physical_size_range": [22000, 150000],
}


def generate_airway_mask(img, lung_mask, spacing, origin=(0.0, 0.0, 0.0), direction=IDENTITY, config=None):
    """-> (mask or None, info)"""
    cfg = config or DEFAULT_SETTINGS
    fast_mode = cfg["fast_mode"]
    size_range = cfg["expected_physical_size_range"]
    z_size = img.shape[0]
    sp = np.asarray(spacing, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    voxel = float(sp[0] * sp[1] * sp[2])
    extend = round(cfg["extend_from_carina_mm"] / spacing[2])
    lung_mask = (np.asarray(lung_mask) != 0).astype(np.uint8)
    processed = False
    best, best_size, best_hu, best_distance, best_seed = None, 0, 0, 0, None
    candidates, seed_regions = [], []
    grown = {}

    def grow(seed, hu):
        # ConnectedThreshold then BinaryDilate(2); pure in (region of the seed, hu), so each distinct region is grown once
        if hu not in grown:
            with np.errstate(invalid="ignore"):
                grown[hu] = (ndimage.label((img >= -2000) & (img <= hu))[0], {})
        lab, done = grown[hu]
        region = int(lab[seed[2], seed[1], seed[0]])
        if region not in done:
            done[region] = dilate(lab == region, 2) if region else np.zeros(img.shape, np.uint8)
        return done[region]

    for k in range(2):
        if processed and fast_mode:
            break
        if k == 1:
            lung_mask = median(lung_mask)
        for distance in cfg["distance_from_supu_slice_values"]:
            if processed and fast_mode:
                break
            lo, hi, _ = slice(z_size - distance - 10, z_size - distance).indices(z_size)
            max_elong, seed = 0, [0, 0, 0]
            if hi > lo:
                lab, count = label(lung_mask[lo:hi])
                slab_origin = np.asarray(origin, dtype=np.float64) + d @ (sp * np.array([0.0, 0.0, float(lo)]))
                for r, st in shape_statistics(lab, count, spacing, slab_origin, direction).items():
                    seed_regions.append((k, distance, r, st["elongation"], st["physical_size"]))
                    if st["elongation"] > max_elong and st["physical_size"] > 2000:
                        seed = physical_point_to_index(st["centroid"], spacing, origin, direction)
                        max_elong = st["elongation"]
            if lung_mask[seed[2], seed[1], seed[0]] == 0:
                continue
            for hu in cfg["lung_mask_hu_values"]:
                result = grow(tuple(seed), hu)
                voxels = int(result.sum())
                if voxels == 0:
                    candidates.append((k, distance, hu, -1, False))
                    continue
                size = int(voxels * voxel)
                passed = not (size > size_range[1] or size < size_range[0])
                candidates.append((k, distance, hu, size, passed))
                if passed:
                    processed = True
                if size > best_size and passed:
                    best, best_size, best_hu, best_distance, best_seed = result, size, hu, distance, list(seed)
    info = {"seed": best_seed, "lung_mask_hu": best_hu, "distance_from_sup_slice": best_distance, "physical_size": best_size,
            "carina_slice": -1, "extend_from_carina": extend, "candidates": candidates, "carina_sizes": None, "seed_regions": seed_regions}
    if best is None:
        return None, info
    carina = -1
    for idx in range(z_size - best_distance, 0, -1):
        cut = best.copy()
        cut[idx:z_size] = 0
        lab, count = label(cut)
        if count == 2:
            s0, s1 = int((lab == 1).sum() * voxel), int((lab == 2).sum() * voxel)
            if s0 > cfg["minimum_tree_half_physical_size"] and s1 > cfg["minimum_tree_half_physical_size"]:
                carina = idx
                info["carina_sizes"] = (s0, s1)
                break
    info["carina_slice"] = carina
    out = best.copy()
    if carina >= 0:
        out[carina + extend:z_size] = 0
    return out, info


def run_bronchus_segmentation(img, spacing, origin=(0.0, 0.0, 0.0), direction=IDENTITY, config=None):
    """-> (lung mask or None, bronchus mask or None, info)"""
    lab, labels, count = detect_holes(img, spacing, origin, direction)
    info = {"components": count, "listed": labels}
    lung = get_lung_mask(lab, labels)
    if lung is None:
        return None, None, info
    airway, ainfo = generate_airway_mask(img, lung, spacing, origin, direction, config)
    info.update(ainfo)
    return lung, airway, info


# ---- the phantom of the pipeline tests -----------------------------------------------------------------------------

def _capsule(shape, a, b, radius):
    """Voxels within `radius` of the segment a-b; points are (z, y, x) in voxel indices."""
    zz, yy, xx = np.indices(shape).astype(np.float64)
    p = np.stack([zz, yy, xx], axis=-1)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ab = b - a
    t = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return ((p - (a + t[..., None] * ab)) ** 2).sum(-1) <= radius * radius


def thorax_phantom(shape=(80, 96, 96), air_column=0):
    """Body 0 HU on -1000, two lungs at -800, an airway wall at -870 around a trachea lumen at -1000 that forks into two
    bronchi, and a gas bubble that is the last component in raster order.  Drawn in this order.  air_column = z: also an 8 x 8
    column of air from slice z to the top, inside the body and away from the trachea."""
    nz, ny, nx = shape
    zz, yy, xx = np.indices(shape).astype(np.float64)
    img = np.full(shape, -1000.0, dtype=np.float32)
    img[((xx - 47.5) / 40) ** 2 + ((yy - 47.5) / 30) ** 2 <= 1] = 0.0
    for sx in (-18, 18):
        img[((zz - 30) / 20) ** 2 + ((yy - 48) / 16) ** 2 + ((xx - (48 + sx)) / 12) ** 2 <= 1] = -800.0
    img[_capsule(shape, (42, 48, 48), (85, 48, 48), 3.6)] = -870.0
    img[_capsule(shape, (42, 48, 48), (85, 48, 48), 2.5)] = -1000.0
    for sx in (-16, 16):
        img[_capsule(shape, (42, 48, 48), (32, 48, 48 + sx), 1.6)] = -1000.0
    img[70:72, 30:32, 30:32] = -1000.0
    if air_column:
        img[air_column:, 60:68, 20:28] = -1000.0
    return img
