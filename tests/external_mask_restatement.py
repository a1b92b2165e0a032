"""numpy / scipy restatement of get_external_mask (reference generation/mask.py:50-104) and of its three kernels' rules,
written independently of the kernels: nothing here looks at row extremes, runs or union-find.

Hull      all pixels' diamond points -> Andrew's monotone chain in Python integers -> every pixel centre against every
          hull edge with `>= 0` (a centre exactly on an edge or a vertex is inside).  Doubled coordinates keep it integral.
Labels    scipy.ndimage.label with the 3 x 3 x 3 structure, renumbered by first voxel in raster order.
Holes     scipy.ndimage.binary_fill_holes with the same structure (the BACKGROUND flood is 26-connected).
Ball      the rule of include/platipy_amd.h: offset d is in the element when sum_i (d_i / (radius_i + 0.5))^2 <= 1."""
import numpy as np
from scipy import ndimage

FULL = np.ones((3, 3, 3), dtype=bool)
FACES = ndimage.generate_binary_structure(3, 1)


# ---- hull ------------------------------------------------------------------------------------------------------------

def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_vertices(points):
    """Andrew's monotone chain over a list of integer (Y, X) tuples -> the hull's vertices, counter-clockwise in the (Y, X)
    plane, collinear points dropped.  Python integers throughout."""
    pts = sorted(set(points))
    if len(pts) <= 2:
        return pts
    lower = []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    upper = []
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def hull_slice(mask2d):
    """-> (uint8 hull image, number of pixel centres that lie exactly on the hull's boundary)."""
    m = np.asarray(mask2d) != 0
    out = np.zeros(m.shape, np.uint8)
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return out, 0
    pts = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        pts += [(2 * y - 1, 2 * x), (2 * y + 1, 2 * x), (2 * y, 2 * x - 1), (2 * y, 2 * x + 1)]
    v = hull_vertices(pts)                      # a diamond has area: at least 4 vertices, never degenerate
    cy, cx = np.indices(m.shape, dtype=np.int64)
    cy, cx = 2 * cy, 2 * cx
    inside = np.ones(m.shape, bool)
    on_edge = np.zeros(m.shape, bool)
    for k in range(len(v)):
        (ay, ax), (by, bx) = v[k], v[(k + 1) % len(v)]
        c = (by - ay) * (cx - ax) - (bx - ax) * (cy - ay)        # int64: |coordinates| < 2^18, products < 2^37
        inside &= c >= 0
        on_edge |= c == 0
    out[inside] = 1
    return out, int((inside & on_edge).sum())


def slice_convex_hull(mask):
    """[Z][Y][X] -> (hull volume, boundary centres over all slices)."""
    mask = np.asarray(mask)
    out = np.zeros(mask.shape, np.uint8)
    total = 0
    for z in range(mask.shape[0]):
        out[z], n = hull_slice(mask[z])
        total += n
    return out, total


# ---- labels, holes, morphology -----------------------------------------------------------------------------------------

def label(mask, fully_connected=False):
    """-> (int32 labels numbered in raster order of each component's first voxel, count)."""
    lab, n = ndimage.label(np.asarray(mask) != 0, structure=FULL if fully_connected else FACES)
    out = np.zeros(lab.shape, np.int32)
    if n:
        flat = lab.ravel()
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        order = np.argsort(first[1:], kind="stable")
        rank = np.zeros(n + 1, np.int32)
        rank[1 + order] = np.arange(1, n + 1, dtype=np.int32)
        out = rank[lab]
    return out.astype(np.int32), int(n)


def largest_component(mask, fully_connected=False):
    """RelabelComponent(ConnectedComponent(mask, fully_connected)) == 1: size descending, then first in raster order."""
    lab, n = label(mask, fully_connected)
    if n == 0:
        return np.zeros(lab.shape, np.uint8)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    return (lab == 1 + int(np.argmax(sizes))).astype(np.uint8)       # argmax: the first of equal sizes


def fill_holes(mask, fully_connected=False):
    return ndimage.binary_fill_holes(np.asarray(mask) != 0, structure=FULL if fully_connected else FACES).astype(np.uint8)


def itk_ball(radius):
    """radius (x, y, z) -> bool [2 rz + 1, 2 ry + 1, 2 rx + 1]"""
    rx, ry, rz = [int(r) for r in radius]
    dz, dy, dx = np.meshgrid(np.arange(-rz, rz + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing="ij")
    return (dx / (rx + 0.5)) ** 2 + (dy / (ry + 0.5)) ** 2 + (dz / (rz + 0.5)) ** 2 <= 1.0


def dilate(mask, radius):
    """Background outside the buffer."""
    return ndimage.binary_dilation(np.asarray(mask) != 0, structure=itk_ball(radius)).astype(np.uint8)


def closing(mask, radius):
    """Dilate then erode with a safe border: as if padded by the radius."""
    rx, ry, rz = [int(r) for r in radius]
    p = np.pad(np.asarray(mask) != 0, ((rz, rz), (ry, ry), (rx, rx)))
    se = itk_ball(radius)
    p = ndimage.binary_erosion(ndimage.binary_dilation(p, structure=se), structure=se, border_value=1)
    return p[rz:p.shape[0] - rz, ry:p.shape[1] - ry, rx:p.shape[2] - rx].astype(np.uint8)


# ---- the whole function ------------------------------------------------------------------------------------------------

def get_external_mask(img, lower_threshold=-100, upper_threshold=2500, dilate_radius=1, max_hole_size=False):
    """The reference's order.  `dilate_radius` / `max_hole_size`: False, a scalar (repeated) or three numbers that reach the
    filters as voxel radii in (x, y, z) order."""
    v = np.asarray(img).astype(np.float64)
    with np.errstate(invalid="ignore"):
        body = ((v >= lower_threshold) & (v <= upper_threshold)).astype(np.uint8)
    body = largest_component(body, fully_connected=True)
    if dilate_radius is not False:
        if not hasattr(dilate_radius, "__iter__"):
            dilate_radius = (dilate_radius,) * 3
        body = dilate(body, dilate_radius)
    if max_hole_size is not False:
        if not hasattr(max_hole_size, "__iter__"):
            max_hole_size = (max_hole_size,) * 3
        body = fill_holes(closing(body, max_hole_size), fully_connected=True)
    return slice_convex_hull(body)[0]


def head_phantom(shape=(14, 56, 48), seed=7):
    """A small CT-like head: an ellipsoid of tissue in air with two air cavities and a block of bone, a couch bar under the
    body that is joined to it only by a chain of voxels touching across edges, and bright specks in the air.
    [Z][Y][X] float32."""
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape).astype(np.float64)
    img = np.full(shape, -1000.0)
    body = ((x - nx / 2) / (0.30 * nx)) ** 2 + ((y - 0.42 * ny) / (0.30 * ny)) ** 2 + ((z - nz / 2) / (0.60 * nz)) ** 2 < 1
    img[body] = 40.0
    img[4:8, 20:26, 20:27] = -1000.0                                     # a closed cavity
    img[9:11, 18:22, 24:30] = -1000.0
    img[5:9, 30:34, 22:26] = 700.0                                       # bone
    img += rng.normal(0.0, 4.0, shape)
    # the couch: a bar two rows below the lowest body row, joined to it by a diagonal chain of single voxels
    ymax = int(np.nonzero(body.any(axis=(0, 2)))[0].max())
    zc = int(np.nonzero(body[:, ymax].any(axis=1))[0][0])
    xs = np.nonzero(body[zc, ymax])[0]
    x0 = int(xs.max())
    img[zc, ymax + 1, x0 + 1] = 300.0                                    # touches the body only across a corner / edge
    img[zc, ymax + 2, x0 + 2] = 300.0
    img[:, ymax + 3:ymax + 5, 4:nx - 4] = 300.0
    img[zc, ymax + 3, x0 + 3] = 300.0
    for _ in range(12):                                                  # specks in the air above the body
        img[rng.integers(0, nz), rng.integers(0, 4), rng.integers(0, nx)] = 500.0
    return img.astype(np.float32)
