"""Plain fp64 numpy / scipy restatement of the cardiac geometry stages (vessel splining, shapes, valves, conduction nodes),
written from the reference's expressions and from the definitions in include/platipy_amd.h -- not from the kernels.

Volumes are [Z][Y][X] arrays; spacing, origin, sizes and points are (x, y, z)."""
import warnings

import numpy as np
from scipy import ndimage
from scipy.interpolate import CubicSpline


# --------------------------------------------------------------------------------------
# moments and centres of mass


def slice_moments(masks, scan):
    """int64 [n][slices][4] = {sum v, sum a v, sum b v, count(v != 0)}; z-scan a = row, b = column; x-scan a = array z, b = array y."""
    out = []
    for m in masks:
        v = np.asarray(m).astype(np.int64)
        nz, ny, nx = v.shape
        if scan == "z":
            a, b = np.mgrid[0:ny, 0:nx]
            out.append(np.stack([v.sum(axis=(1, 2)), (a * v).sum(axis=(1, 2)), (b * v).sum(axis=(1, 2)), (v != 0).sum(axis=(1, 2))], axis=1))
        else:
            a, b = np.mgrid[0:nz, 0:ny]
            out.append(np.stack([v.sum(axis=(0, 1)), (a[:, :, None] * v).sum(axis=(0, 1)), (b[:, :, None] * v).sum(axis=(0, 1)),
                                 (v != 0).sum(axis=(0, 1))], axis=1))
    return np.stack(out)


def com_from_array_list(arrays, spacing, origin, condition_type="count", condition_value=0, scan_direction="z"):
    """platipy/imaging/utils/vessel.py:33-167 on arrays, identity direction."""
    sp, org = np.asarray(spacing, dtype=np.float64), np.asarray(origin, dtype=np.float64)
    com_a_list, com_b_list, weight_list, count_list = [], [], [], []
    ref = np.asarray(arrays[0])
    axes = (1, 0) if scan_direction == "x" else (1, 2)
    if scan_direction == "x":
        a, b = np.mgrid[0:ref.shape[0]:1, 0:ref.shape[1]:1]
        a, b = a[:, :, np.newaxis], b[:, :, np.newaxis]
    else:
        a, b = np.mgrid[0:ref.shape[1]:1, 0:ref.shape[2]:1]
    with np.errstate(divide="ignore", invalid="ignore"):
        for arr in arrays:
            arr = np.asarray(arr)
            com_a = 1.0 * (a * arr).sum(axis=axes)
            com_b = 1.0 * (b * arr).sum(axis=axes)
            weights = np.sum(arr, axis=axes, dtype=np.int64)
            weight_list.append(weights)
            count_list.append(np.any(arr, axis=axes))
            com_a /= 1.0 * weights
            com_b /= 1.0 * weights
            com_a_list.append(com_a)
            com_b_list.append(com_b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        mean_a, mean_b = np.nanmean(com_a_list, axis=0), np.nanmean(com_b_list, axis=0)
        total = np.sum(weight_list, axis=0) if condition_type == "area" else np.sum(count_list, axis=0)
        mean_com = np.dstack((mean_a, mean_b))[0] * np.array((total > condition_value,) * 2).T
    points = []
    for index, com in enumerate(mean_com):
        if np.all(np.isfinite(com)) and np.all(com > 0):
            idx = (index, int(com[1]), int(com[0])) if scan_direction == "x" else (int(com[1]), int(com[0]), index)
            points.append(tuple(org + sp * np.array(idx, dtype=np.float64)))
    return points


# --------------------------------------------------------------------------------------
# centreline and tube


def centreline(points):
    """Clamped cubic spline (zero end derivatives) through the points over normalised cumulative chord length, at 10 N + 1
    uniform parameters."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.concatenate(([0.0], np.cumsum(np.sqrt((np.diff(p, axis=0) ** 2).sum(axis=1)))))
    t /= t[-1]
    t[-1] = 1.0
    u = np.arange(10 * len(p) + 1, dtype=np.float64) / (10 * len(p))
    return CubicSpline(t, p, axis=0, bc_type=((1, np.zeros(3)), (1, np.zeros(3))))(u)


def voxel_centres(shape, spacing, origin):
    z, y, x = np.indices(shape).astype(np.float64)
    return np.stack([origin[0] + x * spacing[0], origin[1] + y * spacing[1], origin[2] + z * spacing[2]], axis=-1)


def tube_distance(polyline, shape, spacing, origin):
    """[Z][Y][X] fp64: the smallest distance from each voxel centre to a segment of the polyline (clamped projection) among the
    segments that may mark it -- the first segment of non-zero length only where the unclamped parameter is >= 0, the last only
    where it is <= 1; +inf where none may.  A voxel is in the tube of radius r iff this is <= r."""
    pts = np.asarray(polyline, dtype=np.float64).reshape(-1, 3)
    segs = [(pts[k], pts[k + 1] - pts[k]) for k in range(len(pts) - 1) if np.any(pts[k + 1] != pts[k])]
    assert segs, "every segment has zero length"
    c = voxel_centres(shape, spacing, origin)
    best = np.full(shape, np.inf)
    for k, (a, d) in enumerate(segs):
        u = c - a
        dot = u @ d
        l2 = d @ d
        t = np.clip(dot / l2, 0.0, 1.0)
        q = u - t[..., None] * d
        dist = np.sqrt((q * q).sum(axis=-1))
        ok = np.ones(shape, bool)
        if k == 0:
            ok &= dot >= 0.0
        if k == len(segs) - 1:
            ok &= dot <= l2
        best = np.where(ok, np.minimum(best, dist), best)
    return best


# --------------------------------------------------------------------------------------
# shapes (platipy/imaging/generation/image.py:19-79)


def insert_sphere(arr, sp_radius=4, sp_centre=(0, 0, 0)):
    x, y, z = np.indices(arr.shape)
    if not hasattr(sp_radius, "__iter__"):
        sp_radius = [sp_radius] * 3
    rx, ry, rz = sp_radius
    with np.errstate(divide="ignore", invalid="ignore"):
        arr[((x - sp_centre[0]) / rx) ** 2.0 + ((y - sp_centre[1]) / ry) ** 2.0 + ((z - sp_centre[2]) / rz) ** 2.0 <= 1] = 1
    return arr


def insert_cylinder(arr, cyl_radius=4, cyl_height=2, cyl_centre=(0, 0, 0)):
    x, y, z = np.indices(arr.shape)
    if not hasattr(cyl_radius, "__iter__"):
        cyl_radius = [cyl_radius] * 2
    radial = (((z - cyl_centre[0]) / cyl_radius[0]) ** 2 + ((y - cyl_centre[1]) / cyl_radius[1]) ** 2) <= 1
    height = np.abs((x - cyl_centre[2]) / (0.5 * cyl_height)) <= 1
    arr[radial & height] = 1
    return arr


def insert_sphere_image(arr, spacing, sp_radius, sp_centre):
    if not hasattr(sp_radius, "__iter__"):
        sp_radius = [sp_radius] * 3
    return insert_sphere(arr.copy(), [i / j for i, j in zip(sp_radius, spacing[::-1])], sp_centre)


def insert_cylinder_image(arr, spacing, cyl_radius=(5, 5), cyl_height=10, cyl_centre=(0, 0, 0)):
    if not hasattr(cyl_radius, "__iter__"):
        cyl_radius = [cyl_radius] * 2
    return insert_cylinder(arr.copy(), [i / j for i, j in zip(cyl_radius, spacing[1::-1])], cyl_height / spacing[2], cyl_centre)


def versor_matrix(axis, angle):
    """Rodrigues' rotation matrix about `axis` by `angle` (what VersorRigid3DTransform.SetRotation describes)."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


# --------------------------------------------------------------------------------------
# valves and conduction nodes (platipy/imaging/utils/valve.py, conduction.py) on [Z][Y][X] 0 / 1 arrays with (x, y, z) spacing
# and origin, identity direction.  Morphology: scipy.ndimage with ITK's ball and border rules (oracle.binary_*_ball); the
# distance map: oracle.maurer_distance_map; resampling: tests/resample_restatement.py.


def _vol(arr, spacing, origin=(0.0, 0.0, 0.0)):
    from oracle import oracle as O

    return O.Vol(np.ascontiguousarray(arr, dtype=np.uint8), tuple(spacing), tuple(origin))


def dilate(arr, spacing, radius):
    from oracle import oracle as O

    return O.binary_dilate_ball(_vol(arr, spacing), radius).arr


def erode(arr, spacing, radius):
    from oracle import oracle as O

    return O.binary_erode_ball(_vol(arr, spacing), radius).arr


def closing(arr, spacing, radius):
    from oracle import oracle as O

    return O.binary_closing_ball(_vol(arr, spacing), radius).arr


def signed_distance(arr, spacing):
    from oracle import oracle as O

    return O.maurer_distance_map(_vol(arr, spacing), signed=True).arr


def label_to_roi(arr, spacing, expansion_mm):
    """utils/crop.py:24-60 -> (size, index), both (x, y, z)."""
    z, y, x = np.where(arr)
    index = np.array([x.min(), y.min(), z.min()])
    size = np.array([x.max(), y.max(), z.max()]) - index + 1
    expansion = (np.array(expansion_mm) / np.array(spacing)).astype(int)
    cb_index = np.max([index - expansion, np.array([0, 0, 0])], axis=0)
    cb_size = np.min([np.array(arr.shape[::-1]) - cb_index, size + 2 * expansion], axis=0)
    return [int(i) for i in cb_size], [int(i) for i in cb_index]


def crop(arr, size, index):
    return arr[index[2]:index[2] + size[2], index[1]:index[1] + size[1], index[0]:index[0] + size[0]].copy()


def paste(shape, arr, index):
    out = np.zeros(shape, np.uint8)
    out[index[2]:index[2] + arr.shape[0], index[1]:index[1] + arr.shape[1], index[0]:index[0] + arr.shape[2]] = arr
    return out


def com_real(arr, spacing, origin):
    return np.asarray(origin, dtype=np.float64) + np.asarray(spacing, dtype=np.float64) * np.asarray(ndimage.center_of_mass(arr))[::-1]


def valve_from_great_vessel(vessel, ventricle, spacing, valve_thickness_mm=8):
    shape = ventricle.shape
    size, index = label_to_roi((vessel + ventricle) > 0, spacing, (20, 20, 20))
    ventricle, vessel = crop(ventricle, size, index), crop(vessel, size, index)
    thickness = int(valve_thickness_mm / spacing[2])
    ventricle_dilate = dilate(ventricle, spacing, (thickness,) * 3)
    overlap = (vessel & ventricle_dilate) * ((vessel | ventricle_dilate) != 0)
    return paste(shape, closing(overlap, spacing, (1, 1, 1)), index)


def valve_using_cylinder(atrium, ventricle, spacing, origin, radius_mm=15, height_mm=10, info=None):
    from tests import resample_restatement as R

    shape = ventricle.shape
    size, index = label_to_roi((atrium + ventricle) > 0, spacing, (20, 20, 20))
    atrium, ventricle = crop(atrium, size, index), crop(ventricle, size, index)
    org = np.asarray(origin, dtype=np.float64) + np.asarray(spacing) * np.asarray(index)
    dilation, overlap_vol = 1, 0
    while overlap_vol <= 2000:
        r = [int(dilation / i) for i in spacing]
        overlap = dilate(atrium, spacing, r) & dilate(ventricle, spacing, r)
        overlap_vol = np.sum(overlap * np.prod(spacing))
        dilation += 1
    if info is not None:
        info["dilations"] = dilation - 1
    loc = [int(i) for i in ndimage.center_of_mass(overlap)]
    loc_real = com_real(overlap, spacing, org)
    cylinder = insert_cylinder_image(0 * ventricle, spacing, radius_mm, height_mm, loc[::-1])
    orientation = com_real(ventricle, spacing, org) - com_real(atrium, spacing, org)
    unit = orientation / np.linalg.norm(orientation)
    angle = np.arccos(np.dot(unit, (0.0, 0.0, 1.0)))
    axis = np.cross(orientation, (0, 0, 1))
    A = versor_matrix(axis, angle)
    g = R.Grid(size, spacing, org)
    valve = R.resample(cylinder, g, g, A, loc_real - A @ loc_real, interp="nearest", default=0, u8=True)["out"]
    return paste(shape, valve, index)


def closest_point_2d(reference, measurement, spacing):
    d = signed_distance(reference[None], spacing)[0]
    yloc, xloc = np.where(measurement)
    k = d[yloc, xloc].argmin()
    return yloc[k], xloc[k]


def sinoatrialnode(svc, ra, wholeheart, spacing, radius_mm=10, info=None):
    shape = wholeheart.shape
    size, index = label_to_roi((svc + ra + wholeheart) > 0, spacing, (20, 20, 20))
    svc, ra, wholeheart = crop(svc, size, index), crop(ra, size, index), crop(wholeheart, size, index)
    inf_limit = np.min(np.where(svc)[0])
    overlap, d, d_ax = 0, 1, 0
    while overlap == 0:
        svc_dilate = dilate(svc, spacing, (d, d, d_ax))
        label_overlap = svc_dilate & ra
        overlap = label_overlap[inf_limit].sum()
        d += 1
        if d >= 3:
            inf_limit = np.min(np.where(svc_dilate)[0])
            d_ax += 1
    if info is not None:
        info["dilations"] = d - 1
    loc = [int(i) for i in ndimage.center_of_mass(label_overlap)]
    intersect = ra * 0
    intersect[inf_limit, loc[1], loc[2]] = 1
    region = erode(wholeheart, spacing, (10, 10, 0))
    dmap = signed_distance(intersect, spacing)
    yloc, xloc = np.where(region[inf_limit])
    k = dmap[inf_limit, yloc, xloc].argmin()
    return paste(shape, insert_sphere_image(ra * 0, spacing, radius_mm, (inf_limit, yloc[k], xloc[k])), index)


def atrioventricularnode(la, lv, ra, rv, spacing, radius_mm=10, info=None):
    shape = ra.shape
    size, index = label_to_roi((la + lv + ra + rv) > 0, spacing, (20, 20, 20))
    la, lv, ra, rv = (crop(a, size, index) for a in (la, lv, ra, rv))
    slice_loc = int(np.min(np.where(la)[0]) + 10 / spacing[2])
    la2, lv2, ra2, rv2 = la[slice_loc], lv[slice_loc], ra[slice_loc], rv[slice_loc]
    overlap, e = 1, 1
    while overlap > 0:
        lv2 = erode(lv2[None], spacing, (e, e, 0))[0]
        overlap = (lv2 & la2).sum()
        e += 1
    if info is not None:
        info["erosions"] = e - 1
    y_la, x_la = closest_point_2d(rv2, la2, spacing)
    y_lv, x_lv = closest_point_2d(ra2, lv2, spacing)
    y_ra, x_ra = closest_point_2d(lv2, ra2, spacing)
    y_rv, x_rv = closest_point_2d(la2, rv2, spacing)
    x_loc = np.mean((x_la, x_lv, x_ra, x_rv), dtype=int)
    y_loc = np.mean((y_la, y_lv, y_ra, y_rv), dtype=int)
    return paste(shape, insert_sphere_image(ra * 0, spacing, radius_mm, (slice_loc, y_loc, x_loc)), index)
