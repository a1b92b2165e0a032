"""fp64 numpy restatement of the cubic B-spline transform, its dense evaluation and the similarity metrics with their
gradients over the control-point coefficients -- the yardstick tests/test_bspline.py holds the HIP kernels to.  Written
from the published definitions (uniform cubic B-spline basis; ITK's BSplineTransform conventions as DESIGN.md section 8
lists them, [ITK-upstream, unverified here]); imports nothing from platipy_amd."""
import numpy as np


def i2p(spacing, direction):
    return np.asarray(direction, dtype=np.float64).reshape(3, 3) * np.asarray(spacing, dtype=np.float64)[None, :]


def initializer(size, spacing, origin, direction, mesh):
    """sitk.BSplineTransformInitializer -> dict(mesh, domain_origin, domain_dimensions, direction, lattice_size, lattice_spacing,
    lattice_origin)."""
    size = np.asarray(size, dtype=np.float64)
    sp = np.asarray(spacing, dtype=np.float64)
    D = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    mesh = np.asarray(mesh, dtype=np.int64)
    domain_origin = np.asarray(origin, dtype=np.float64) + D @ (-0.5 * sp)
    dims = size * sp
    lsp = dims / mesh
    return {"mesh": mesh, "domain_origin": domain_origin, "domain_dimensions": dims, "direction": D, "lattice_size": mesh + 3,
            "lattice_spacing": lsp, "lattice_origin": domain_origin - D @ lsp}


def control_point_spacing_distance_to_number(size, spacing, grid_spacing):
    return (np.array(size) * np.array(spacing) / np.array(grid_spacing) + 0.5).astype(int)


def flat_parameters(coef):
    """[3, cz, cy, cx] -> ITK's flat order: x block, y block, z block, each x fastest."""
    return np.concatenate([coef[c].reshape(-1) for c in range(3)])


def basis(t):
    t = np.asarray(t, dtype=np.float64)
    return np.stack([(1 - t) ** 3 / 6.0, (3 * t ** 3 - 6 * t ** 2 + 4) / 6.0, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6.0, t ** 3 / 6.0], axis=-1)


def support(points, lat):
    """physical points [n, 3] -> (inside [n], base [n, 3] lattice index of the first supporting control point, w [n, 3, 4])."""
    u = (points - lat["lattice_origin"][None, :]) @ np.linalg.inv(i2p(lat["lattice_spacing"], lat["direction"])).T
    mesh = lat["mesh"][None, :].astype(np.float64)
    inside = np.all((u >= 1.0) & (u < mesh + 1.0), axis=1)
    fl = np.floor(np.where(inside[:, None], u, 1.0))
    return inside, fl.astype(np.int64) - 1, basis(np.where(inside[:, None], u - fl, 0.0))


def displacement(points, coef, lat):
    """D(p) for physical points [n, 3]; 0 outside the transform domain.  coef: [3, cz, cy, cx]."""
    inside, base, w = support(points, lat)
    coef = np.asarray(coef, dtype=np.float64)
    out = np.zeros((points.shape[0], 3))
    for k in range(4):
        for j in range(4):
            for i in range(4):
                ww = w[:, 0, i] * w[:, 1, j] * w[:, 2, k]
                out += ww[:, None] * coef[:, base[:, 2] + k, base[:, 1] + j, base[:, 0] + i].T
    out[~inside] = 0.0
    return out


def grid_points(size, spacing, origin, direction):
    """physical points of a grid, raster order (x fastest) [n, 3]"""
    nx, ny, nz = (int(s) for s in size)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1).astype(np.float64)
    return np.asarray(origin, dtype=np.float64)[None, :] + idx @ i2p(spacing, direction).T


def field(coef, lat, size, spacing, origin, direction):
    """planar displacement field [3, Z, Y, X] on a grid"""
    d = displacement(grid_points(size, spacing, origin, direction), coef, lat)
    return d.T.reshape(3, int(size[2]), int(size[1]), int(size[0]))


def _locate(c, n):
    ok = np.all((c >= -0.5) & (c < np.asarray(n, dtype=np.float64)[None, :] - 0.5), axis=1)
    fl = np.floor(np.where(ok[:, None], c, 0.0))
    return ok, fl.astype(np.int64), np.where(ok[:, None], c - fl, 0.0)


def _corners(vol, b, n):
    """the eight clamped corner values (ITK's linear interpolator: the lower index clamps at 0, the upper at n - 1, and the
    weight of an axis is 0 below index 0) -> (a [n, 2, 2, 2] indexed z y x, w [n, 3])"""
    lo = [np.maximum(b[:, a], 0) for a in range(3)]
    hi = [np.minimum(lo[a] + 1, n[a] - 1) for a in range(3)]
    a = np.empty((b.shape[0], 2, 2, 2))
    for kz, z in enumerate((lo[2], hi[2])):
        for ky, y in enumerate((lo[1], hi[1])):
            for kx, x in enumerate((lo[0], hi[0])):
                a[:, kz, ky, kx] = vol[z, y, x]
    return a


def _trilinear(a, w):
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    v00 = a[:, 0, 0, 0] + (a[:, 0, 0, 1] - a[:, 0, 0, 0]) * wx
    v10 = a[:, 0, 1, 0] + (a[:, 0, 1, 1] - a[:, 0, 1, 0]) * wx
    v01 = a[:, 1, 0, 0] + (a[:, 1, 0, 1] - a[:, 1, 0, 0]) * wx
    v11 = a[:, 1, 1, 0] + (a[:, 1, 1, 1] - a[:, 1, 1, 0]) * wx
    v0 = v00 + (v10 - v00) * wy
    v1 = v01 + (v11 - v01) * wy
    val = v0 + (v1 - v0) * wz
    gx0 = (a[:, 0, 0, 1] - a[:, 0, 0, 0]) + ((a[:, 0, 1, 1] - a[:, 0, 1, 0]) - (a[:, 0, 0, 1] - a[:, 0, 0, 0])) * wy
    gx1 = (a[:, 1, 0, 1] - a[:, 1, 0, 0]) + ((a[:, 1, 1, 1] - a[:, 1, 1, 0]) - (a[:, 1, 0, 1] - a[:, 1, 0, 0])) * wy
    gx = gx0 + (gx1 - gx0) * wz
    gy = (v10 - v00) + ((v11 - v01) - (v10 - v00)) * wz
    gz = v1 - v0
    return val, np.stack([gx, gy, gz], axis=1)


def metric(kind, fixed, fgeom, moving, mgeom, vgeom, stride, coef, lat, fixed_mask=None, moving_mask=None, jitter=None,
           moving_gradient=None):
    """kind: "mean_squares" | "correlation".  *geom: (size, spacing, origin, direction).  Samples: every stride-th voxel (raster
    order) of the virtual grid, plus jitter [nsamp, 3] in virtual-index units.  moving_gradient: [3, Z, Y, X] in moving-index
    units (linearly interpolated) or None (analytic gradient of the trilinear interpolant).
    -> (value, gradient [3 * ncp] in ITK's order, stats dict(valid, outside, masked, seen))."""
    fixed = np.asarray(fixed, dtype=np.float64)
    moving = np.asarray(moving, dtype=np.float64)
    vsize = [int(v) for v in vgeom[0]]
    nvirt = vsize[0] * vsize[1] * vsize[2]
    lin = np.arange(0, nvirt, int(stride), dtype=np.int64)
    v = np.stack([lin % vsize[0], (lin // vsize[0]) % vsize[1], lin // (vsize[0] * vsize[1])], axis=1).astype(np.float64)
    if jitter is not None:
        v = v + np.asarray(jitter, dtype=np.float64)[: v.shape[0]]
    p = np.asarray(vgeom[2], dtype=np.float64)[None, :] + v @ i2p(vgeom[1], vgeom[3]).T
    inside, base, w = support(p, lat)
    d = displacement(p, coef, lat)
    p2i_f = np.linalg.inv(i2p(fgeom[1], fgeom[3]))
    p2i_m = np.linalg.inv(i2p(mgeom[1], mgeom[3]))
    cf = (p - np.asarray(fgeom[2], dtype=np.float64)[None, :]) @ p2i_f.T
    cm = (p + d - np.asarray(mgeom[2], dtype=np.float64)[None, :]) @ p2i_m.T
    fn, mn = [int(s) for s in fgeom[0]], [int(s) for s in mgeom[0]]
    okf, bf, ff = _locate(cf, fn)
    okm, bm, fm = _locate(cm, mn)
    in_buffer = okf & okm
    masked = np.zeros_like(in_buffer)
    if fixed_mask is not None:
        q = np.floor(np.where(in_buffer[:, None], cf, 0.0) + 0.5).astype(np.int64)
        masked |= in_buffer & (np.asarray(fixed_mask)[q[:, 2], q[:, 1], q[:, 0]] == 0)
    if moving_mask is not None:
        q = np.floor(np.where(in_buffer[:, None], cm, 0.0) + 0.5).astype(np.int64)
        masked |= in_buffer & ~masked & (np.asarray(moving_mask)[q[:, 2], q[:, 1], q[:, 0]] == 0)
    valid = in_buffer & ~masked
    stats = {"valid": int(valid.sum()), "outside": int((~in_buffer).sum()), "masked": int(masked.sum()), "seen": int(v.shape[0])}

    sel = np.nonzero(valid)[0]
    wf = np.where(bf[sel] < 0, 0.0, ff[sel])
    wm = np.where(bm[sel] < 0, 0.0, fm[sel])
    f, _ = _trilinear(_corners(fixed, bf[sel], fn), wf)
    m, g_idx = _trilinear(_corners(moving, bm[sel], mn), wm)
    if moving_gradient is not None:
        mg = np.asarray(moving_gradient, dtype=np.float64)
        g_idx = np.stack([_trilinear(_corners(mg[r], bm[sel], mn), wm)[0] for r in range(3)], axis=1)
    g_phys = g_idx @ p2i_m          # d m / d c_r = sum_q g_idx[q] p2i_m[q, r]

    cz, cy, cx = (int(s) for s in np.asarray(coef).shape[1:])
    ncp = cx * cy * cz

    def scatter(weight):
        """sum over valid samples inside the domain of weight[:, r] * w_i w_j w_k -> [3 * ncp]"""
        out = np.zeros(3 * ncp)
        ins = inside[sel]
        b, ww, wt = base[sel][ins], w[sel][ins], weight[ins]
        for k in range(4):
            for j in range(4):
                for i in range(4):
                    cp = ((b[:, 2] + k) * cy + (b[:, 1] + j)) * cx + (b[:, 0] + i)
                    t = ww[:, 0, i] * ww[:, 1, j] * ww[:, 2, k]
                    for r in range(3):
                        out[r * ncp:(r + 1) * ncp] += np.bincount(cp, weights=wt[:, r] * t, minlength=ncp)
        return out

    n = float(sel.size)
    if n == 0:
        return float("nan"), np.zeros(3 * ncp), stats
    if kind == "mean_squares":
        diff = f - m
        return float((diff * diff).sum() / n), scatter((-2.0 * diff)[:, None] * g_phys) / n, stats
    fbar, mbar = f.mean(), m.mean()
    sff, smm, sfm = (f * f).sum() - n * fbar * fbar, (m * m).sum() - n * mbar * mbar, (f * m).sum() - n * fbar * mbar
    if sff <= 1e-300 or smm <= 1e-300:
        return 0.0, np.zeros(3 * ncp), stats
    G, FG, MG = scatter(g_phys), scatter(f[:, None] * g_phys), scatter(m[:, None] * g_phys)
    dsfm, dsmm = FG - fbar * G, 2.0 * (MG - mbar * G)
    grad = -(2.0 * sfm / (sff * smm) * dsfm - (sfm * sfm) / (sff * smm * smm) * dsmm)
    return float(-(sfm * sfm) / (sff * smm)), grad, stats


def blobs(shape, seed, n_blobs=10, noise=0.0):
    """smooth seeded sum of Gaussian blobs (+ noise) [Z, Y, X] float32"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol = np.zeros(shape)
    for _ in range(n_blobs):
        c = [rng.uniform(0.15, 0.85) * s for s in (nx, ny, nz)]
        r = [rng.uniform(0.10, 0.30) * s for s in (nx, ny, nz)]
        vol += rng.uniform(50, 200) * np.exp(-0.5 * (((xx - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((zz - c[2]) / r[2]) ** 2))
    if noise:
        vol += rng.normal(0, noise, size=shape)
    return vol.astype(np.float32)


def warp_linear(volume, geom, coef, lat, default=0.0, nearest=False):
    """volume on `geom` pulled back through the B-spline: out(p) = volume(p + D(p)), linear (or nearest) interpolation"""
    size, sp, org, D = geom
    p = grid_points(size, sp, org, D)
    q = p + displacement(p, coef, lat)
    c = (q - np.asarray(org, dtype=np.float64)[None, :]) @ np.linalg.inv(i2p(sp, D)).T
    n = [int(s) for s in size]
    ok, b, fr = _locate(c, n)
    out = np.full(p.shape[0], float(default))
    sel = np.nonzero(ok)[0]
    vol = np.asarray(volume, dtype=np.float64)
    if nearest:
        qn = np.floor(c[sel] + 0.5).astype(np.int64)
        out[sel] = vol[qn[:, 2], qn[:, 1], qn[:, 0]]
    else:
        out[sel] = _trilinear(_corners(vol, b[sel], n), np.where(b[sel] < 0, 0.0, fr[sel]))[0]
    return out.reshape(n[2], n[1], n[0])
