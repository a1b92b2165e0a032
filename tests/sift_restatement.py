"""Restatement of the SIFT landmark rules S1 ... S7 in plain numpy, written from the rules and not from the
kernels of csrc/pp_sift.h: candidates by shifted comparisons of the whole difference stack, refinement with np.linalg.solve,
the descriptor with a vertex matrix and np.add.at, matching from the fp64 distance matrix, points by an fp64 trilinear sum of
eight weighted corners.  Every function that decides something also says which decisions lie within rounding of their
threshold ("marked"), so that a test can leave those out.

Arrays are [z, y, x]; a stack is [level, z, y, x]; keypoint rows are (x, y, z, level)."""
import numpy as np

PHI = (1.0 + np.sqrt(5.0)) / 2.0
SIGNS = [(1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0)]
# (x, y, z) components: (0, +-1, +-phi), (+-1, +-phi, 0), (+-phi, 0, +-1), signs (+,+), (+,-), (-,+), (-,-)
VERTICES = np.array([(0.0, a, b * PHI) for a, b in SIGNS] + [(a, b * PHI, 0.0) for a, b in SIGNS] + [(a * PHI, 0.0, b) for a, b in SIGNS])
NEAR = 1e-9


def dog(stack):
    stack = np.asarray(stack, np.float32)
    return stack[1:] - stack[:-1]          # one fp32 subtraction (S3)


def candidates(stack):
    """S3 -> int32 [n, 4] rows (x, y, z, level) in ascending (level, z, y, x)."""
    d = dog(stack)
    nl, nz, ny, nx = d.shape
    if nl < 3 or min(nz, ny, nx) < 3:
        return np.zeros((0, 4), np.int32)
    c = d[1:-1, 1:-1, 1:-1, 1:-1]
    gt, lt = np.ones(c.shape, bool), np.ones(c.shape, bool)
    for dl in (-1, 0, 1):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl == dz == dy == dx == 0:
                        continue
                    n = d[1 + dl:nl - 1 + dl, 1 + dz:nz - 1 + dz, 1 + dy:ny - 1 + dy, 1 + dx:nx - 1 + dx]
                    gt &= c > n
                    lt &= c < n
    l, z, y, x = np.nonzero(gt | lt)        # np.nonzero walks in C order: (level, z, y, x) ascending
    return np.stack([x + 1, y + 1, z + 1, l + 1], axis=1).astype(np.int32)


def refine(stack, cand, value_range, contrast_threshold, curvature_threshold):
    """S4 on the candidate rows -> dict: keep (bool), marked (bool: a test within NEAR of its threshold), offset [n, 3],
    response [n], and for the bound of the solve cond [n] (the condition number of H), raw [n] (the largest component of the
    step before the clamp) and gnorm [n] (the 1-norm of g)."""
    d = dog(stack).astype(np.float64)
    n = len(cand)
    keep, marked = np.zeros(n, bool), np.zeros(n, bool)
    offset, response, cond, raw, gnorm = np.zeros((n, 3)), np.zeros(n), np.ones(n), np.zeros(n), np.zeros(n)
    for k, (x, y, z, l) in enumerate(np.asarray(cand, np.int64)):
        v = d[l, z - 1:z + 2, y - 1:y + 2, x - 1:x + 2]          # v[dz + 1, dy + 1, dx + 1]
        c = v[1, 1, 1]
        g = 0.5 * np.array([v[1, 1, 2] - v[1, 1, 0], v[1, 2, 1] - v[1, 0, 1], v[2, 1, 1] - v[0, 1, 1]])
        hxx, hyy, hzz = v[1, 1, 2] - 2 * c + v[1, 1, 0], v[1, 2, 1] - 2 * c + v[1, 0, 1], v[2, 1, 1] - 2 * c + v[0, 1, 1]
        hxy = 0.25 * (v[1, 2, 2] - v[1, 0, 2] - v[1, 2, 0] + v[1, 0, 0])
        hxz = 0.25 * (v[2, 1, 2] - v[0, 1, 2] - v[2, 1, 0] + v[0, 1, 0])
        hyz = 0.25 * (v[2, 2, 1] - v[0, 2, 1] - v[2, 0, 1] + v[0, 0, 1])
        H = np.array([[hxx, hxy, hxz], [hxy, hyy, hyz], [hxz, hyz, hzz]])
        det = np.linalg.det(H)
        scale = np.abs(H).max() ** 3
        if not np.isfinite(det) or det == 0.0 or scale == 0.0:
            response[k] = c
            continue
        if abs(det) <= 1e-6 * scale:        # the solve itself is not trustworthy: leave the decision to nobody
            marked[k] = True
        cond[k] = np.linalg.cond(H)
        o = -np.linalg.solve(H, g)
        raw[k], gnorm[k] = np.abs(o).max(), np.abs(g).sum()
        o = np.clip(o, -0.5, 0.5)
        r = c + 0.5 * float(g @ o)
        offset[k], response[k] = o, r
        trace = hxx + hyy + hzz
        minors = (hyy * hzz - hyz * hyz) + (hxx * hzz - hxz * hxz) + (hxx * hyy - hxy * hxy)
        q_contrast, q_curv = abs(r) / value_range, trace ** 3 / det
        keep[k] = bool(q_contrast >= contrast_threshold and det * trace > 0 and minors > 0 and q_curv < curvature_threshold)
        m_scale = abs(hyy * hzz) + hyz * hyz + abs(hxx * hzz) + hxz * hxz + abs(hxx * hyy) + hxy * hxy
        marked[k] |= bool(abs(q_contrast - contrast_threshold) <= NEAR * abs(contrast_threshold)
                          or abs(q_curv - curvature_threshold) <= NEAR * abs(curvature_threshold)
                          or abs(minors) <= NEAR * m_scale or abs(trace) <= NEAR * (abs(hxx) + abs(hyy) + abs(hzz)))
    return {"keep": keep, "marked": marked, "offset": offset, "response": response, "cond": cond, "raw": raw, "gnorm": gnorm}


def descriptor(volume, spacing, kp):
    """S6 for one keypoint (x, y, z) on `volume` [z, y, x] fp32, spacing (x, y, z) -> (float32 [768], marked: a sample whose
    two largest dot products differ by less than 1e-12 relative without being equal: an exact tie -- a gradient with a zero
    component, as the replicated edge gives -- is decided by the rule itself, the lowest index)."""
    g = np.asarray(volume, np.float32)
    nz, ny, nx = g.shape
    o = np.arange(-8, 8)
    X, Y, Z = (np.clip(int(kp[0]) + o, 0, nx - 1), np.clip(int(kp[1]) + o, 0, ny - 1), np.clip(int(kp[2]) + o, 0, nz - 1))
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    up = lambda a, n: np.minimum(a + 1, n - 1)  # noqa: E731
    dn = lambda a: np.maximum(a - 1, 0)  # noqa: E731
    gx = (g[zz, yy, up(xx, nx)] - g[zz, yy, dn(xx)]).astype(np.float64) / (2.0 * spacing[0])
    gy = (g[zz, up(yy, ny), xx] - g[zz, dn(yy), xx]).astype(np.float64) / (2.0 * spacing[1])
    gz = (g[up(zz, nz), yy, xx] - g[dn(zz), yy, xx]).astype(np.float64) / (2.0 * spacing[2])
    grad = np.stack([gx, gy, gz], axis=-1)                      # [16, 16, 16, 3]
    mag = np.sqrt((grad ** 2).sum(-1))
    oz, oy, ox = np.meshgrid(o + 0.5, o + 0.5, o + 0.5, indexing="ij")
    weight = np.exp(-(ox ** 2 + oy ** 2 + oz ** 2) / 128.0)
    dots = grad @ VERTICES.T                                    # [16, 16, 16, 12]
    best = np.argmax(dots, axis=-1)                             # the first of equal maxima: the lowest index
    top2 = np.sort(dots, axis=-1)[..., -2:]
    live = mag > 0.0
    gap = top2[..., 1] - top2[..., 0]
    marked = bool(np.any(live & (gap > 0.0) & (gap < 1e-12 * np.abs(top2[..., 1]))))
    cz, cy, cx = np.meshgrid(np.arange(16) // 4, np.arange(16) // 4, np.arange(16) // 4, indexing="ij")
    hist = np.zeros(768)
    np.add.at(hist, (((cz * 4 + cy) * 4 + cx) * 12 + best)[live], (weight * mag)[live])
    norm = np.sqrt((hist ** 2).sum())
    if norm == 0.0:
        return np.zeros(768, np.float32), marked
    hist = np.minimum(hist / norm, 0.2)
    return (hist / np.sqrt((hist ** 2).sum())).astype(np.float32), marked


def distances(a, b):
    """fp64 squared distances [na, nb] of fp32 tables."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def distance_bound(a, b):
    """Bound [na, nb] on |fp32 running sum of fused (a - b)^2 terms - the fp64 distance|: each difference carries one fp32
    rounding (relative u on |a - b|, so 2 u + u^2 on its square) and each of the n additions one more on a partial sum that
    never exceeds the total: (n + 2) u (1 + u)^(n + 2) S <= 1.01 (n + 2) u S for n u < 0.005, u = 2^-24; S is the fp64 distance."""
    n = np.asarray(a).shape[1]
    return 1.01 * (n + 2) * 2.0 ** -24 * distances(a, b)


def nearest(a, b, points_a=None, points_b=None, radius=None):
    """S7 in fp64 -> (best_index [na], best [na], second [na]); the lowest index on a tie; inf where nothing takes part."""
    d = distances(a, b)
    if radius is not None:
        pa, pb = np.asarray(points_a, np.float64), np.asarray(points_b, np.float64)
        d = np.where(((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1) <= float(radius) ** 2, d, np.inf)
    idx = np.argmin(d, axis=1)
    best = d[np.arange(len(d)), idx]
    rest = d.copy()
    rest[np.arange(len(d)), idx] = np.inf
    second = rest.min(axis=1) if d.shape[1] > 1 else np.full(len(d), np.inf)
    idx = np.where(np.isfinite(best), idx, -1)
    return idx.astype(np.int32), best, second


def accepted(best, second, ratio):
    return best < ratio ** 2 * second


def match(a, b, ratio=0.8, mutual=True, points_a=None, points_b=None, radius=None, bound_rel=0.0):
    """-> (pairs int [m, 2], marked rows of a): accepted pairs by S7 in fp64; a row of a is marked when its decision (or its
    partner's reverse decision) lies within `bound_rel` (relative) of the ratio threshold or of a tie for the best row."""
    ia, ba, sa = nearest(a, b, points_a, points_b, radius)
    ok = accepted(ba, sa, ratio) & (ia >= 0)
    shaky = lambda bb, ss: np.isfinite(bb) & np.isfinite(ss) & (np.abs(bb - ratio ** 2 * ss) <= bound_rel * (bb + ratio ** 2 * ss))  # noqa: E731
    marked = shaky(ba, sa)
    if mutual:
        ib, bb, sb = nearest(b, a, points_b, points_a, radius)
        okb = accepted(bb, sb, ratio) & (ib >= 0)
        back = np.where(ia >= 0, ia, 0)
        marked |= shaky(bb, sb)[back] & (ia >= 0)
        ok &= okb[back] & (ib[back] == np.arange(len(ia)))
    rows = np.flatnonzero(ok)
    return np.stack([rows, ia[rows]], axis=1).astype(np.int64).reshape(-1, 2), marked


def physical_to_index(points, size, spacing, origin, direction):
    D = np.asarray(direction, np.float64).reshape(3, 3)
    M = D * np.asarray(spacing, np.float64)[None, :]
    return np.linalg.solve(M, (np.asarray(points, np.float64) - np.asarray(origin, np.float64)).T).T


def transform_points(field, size, spacing, origin, direction, points):
    """p + D(p), D trilinear in fp64 from the planar field [3, z, y, x]; zero outside [-0.5, n - 0.5); the upper corner
    clamped to the last voxel.  -> (points [n, 3], |field| bound per point for the tolerance)."""
    f = np.asarray(field, np.float64)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    c = physical_to_index(pts, size, spacing, origin, direction)
    out, scale = pts.copy(), np.zeros(len(pts))
    for k, ck in enumerate(c):
        if not all(-0.5 <= ck[a] < size[a] - 0.5 for a in range(3)):
            continue
        lo = [max(int(np.floor(v)), 0) for v in ck]
        w = [ck[a] - np.floor(ck[a]) if ck[a] >= 0 else 0.0 for a in range(3)]
        hi = [min(lo[a] + 1, size[a] - 1) for a in range(3)]
        disp = np.zeros(3)
        for (iz, wz) in ((lo[2], 1 - w[2]), (hi[2], w[2])):
            for (iy, wy) in ((lo[1], 1 - w[1]), (hi[1], w[1])):
                for (ix, wx) in ((lo[0], 1 - w[0]), (hi[0], w[0])):
                    disp += wz * wy * wx * f[:, iz, iy, ix]
                    scale[k] = max(scale[k], np.abs(f[:, iz, iy, ix]).max())
        out[k] = pts[k] + disp
    return out, scale
