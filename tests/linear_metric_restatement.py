"""TEST INFRASTRUCTURE: an fp64 restatement of what the linear-registration metric kernels (pp_fusion.hip: pp_meansq_affine_f32,
pp_corr_moments_affine_f32, pp_metric_values_affine_f32, pp_mi_histogram_f32, pp_mi_gradient_f32) compute, with a first-order
error bound next to every number and the distance of the inputs from the nearest decision line.  It shares no code with
oracle/linear_oracle.py and gets there by another road: scipy's spline interpolator instead of eight gathered corners.

Definitions (include/platipy_amd.h, the comment above msq_args in pp_fusion.hip):
  sample e of the raster walk   lin = e * stride,  v = (lin % vx, (lin / vx) % vy, lin / (vx vy)) [+ jitter[e]]
  its two points                cf = Af v + bf,  cm = Am v + bm                                   (continuous indices x, y, z)
  inside                        -0.5 <= c < n - 0.5 on every axis; a mask is read at floor(c + 0.5)
  value                         the trilinear interpolant with edge replication in the half-voxel bands [-0.5, 0) and
                                [n - 1, n - 0.5): scipy.ndimage.map_coordinates(order=1, mode="nearest")
  interpolant gradient          along an axis the interpolant is linear inside the cell floor(c): the forward difference of that
                                cell, interpolated linearly along the other two axes -- map_coordinates of the forward-difference
                                image at (floor(c) on the axis, c on the others), mode="nearest".  Zero in the clamped band
                                [n - 1, n - 0.5) of the axis, where both corners are the last voxel.  In the lower band
                                [-0.5, 0) the cell is floor(c) = -1 and "nearest" hands back cell 0: the project's convention
                                (kernels, oracle/linear_oracle.py and the tests that pin them) continues the first cell's
                                slope to the border although the value is held constant there
  gradient image                map_coordinates(order=1, mode="nearest") of each of its three volumes

Error model (u = 2^-24): the kernels form every interpolated number in fp32 as three nested levels of a + (b - a) w with
w = (float)(c - floor(c)); everything after that -- differences, products, sums -- is fp64.  One level rounds four times:
the difference (u |b - a|, scaled by w afterwards), the weight (u w, times |b - a|), the product (u |b - a| w) and the sum
(u |result|); errors of a and b pass through as the convex combination (1 - w) ea + w eb.  So
      e(a + (b - a) w) <= (1 - w) ea + w eb + u (3 |b - a| w + |result|)
and a plain difference b - a of two interpolated numbers errs by ea + eb + u |b - a|.  A fused multiply-add rounds less.
`interp_bound` walks the kernel's own expression tree with these two rules on the eight corners of each sample; the corners are
gathered for the BOUND only (and for the footprint), never for a value.  The sums' bounds follow to first order plus the
second-order product terms, e.g. |d sum (f - m)^2| <= sum 2 |f - m| (ef + em) + (ef + em)^2, and the fp64 accumulation adds
n 2^-53 sum |term|.
"""
import numpy as np
from scipy.ndimage import map_coordinates

U24 = 2.0 ** -24
U53 = 2.0 ** -53


# --------------------------------------------------------------------------------------
# sample points


def lattice(vsize, stride, jitter=None):
    """-> v [n, 3] (x, y, z) float64: every stride-th voxel of the virtual grid in raster order, plus the jitter rows."""
    vx, vy, vz = (int(k) for k in vsize)
    nsamp = (vx * vy * vz + int(stride) - 1) // int(stride)
    lin = np.arange(nsamp, dtype=np.int64) * int(stride)
    v = np.empty((nsamp, 3))
    v[:, 0] = lin % vx
    v[:, 1] = (lin // vx) % vy
    v[:, 2] = lin // (vx * vy)
    if jitter is not None:
        v += np.asarray(jitter, dtype=np.float64)[:nsamp]
    return v


def points(A, b, v):
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    b = np.asarray(b, dtype=np.float64)
    return np.stack([A[r, 0] * v[:, 0] + A[r, 1] * v[:, 1] + A[r, 2] * v[:, 2] + b[r] for r in range(3)], axis=1)


def size_xyz(img):
    return np.array(img.shape[::-1], dtype=np.int64)        # (nx, ny, nz)


def inside(c, n):
    return np.all((c >= -0.5) & (c < n[None, :] - 0.5), axis=1)


def mask_at(mask, c):
    """The mask voxel floor(c + 0.5) of every point (clipped where the point is outside: the caller ignores those)."""
    n = size_xyz(mask)
    q = np.clip(np.floor(c + 0.5).astype(np.int64), 0, n[None, :] - 1)
    return np.asarray(mask)[q[:, 2], q[:, 1], q[:, 0]] != 0


# --------------------------------------------------------------------------------------
# values by scipy


def interp(img, c):
    """Trilinear value with edge replication at c [n, 3] (x, y, z)."""
    return map_coordinates(np.asarray(img, dtype=np.float64), [c[:, 2], c[:, 1], c[:, 0]], order=1, mode="nearest")


def interp_gradient(img, c):
    """Gradient of that interpolant, [n, 3] per index unit of x, y, z."""
    a = np.asarray(img, dtype=np.float64)
    n = size_xyz(a)
    out = np.zeros((len(c), 3))
    for r in range(3):                       # r = 0 (x) is array axis 2
        if n[r] < 2:
            continue
        d = np.diff(a, axis=2 - r)
        cc = c.copy()
        cell = np.floor(c[:, r])
        cc[:, r] = cell
        g = map_coordinates(d, [cc[:, 2], cc[:, 1], cc[:, 0]], order=1, mode="nearest")
        out[:, r] = np.where(c[:, r] < n[r] - 1.0, g, 0.0)
    return out


# --------------------------------------------------------------------------------------
# bounds by the kernel's expression tree


def _corners(img, c):
    """The eight corners the kernel reads, as a[dz][dy][dx], the three weights, and every voxel index it touches."""
    a = np.asarray(img, dtype=np.float64)
    n = size_xyz(a)
    fl = np.floor(c)
    b = fl.astype(np.int64)
    i0 = np.clip(b, 0, n[None, :] - 1)
    i1 = np.minimum(i0 + 1, n[None, :] - 1)
    w = np.where(b < 0, 0.0, c - fl)
    idx = (i0, i1)
    cor = [[[a[idx[dz][:, 2], idx[dy][:, 1], idx[dx][:, 0]] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    return cor, w, i0, i1


def _lerp(a, ea, b, eb, w):
    v = a + (b - a) * w
    return v, (1.0 - w) * ea + w * eb + U24 * (3.0 * np.abs(b - a) * w + np.abs(v))


def _sub(a, ea, b, eb):
    return b - a, ea + eb + U24 * np.abs(b - a)


def interp_bound(img, c, gradient=False):
    """-> e_value [n] (and e_gradient [n, 3]): bounds on the fp32 evaluation error of the kernel's value and interpolant gradient."""
    cor, w, _, _ = _corners(img, c)
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    z = np.zeros(len(c))
    row = {}
    for dz in (0, 1):
        for dy in (0, 1):
            row[dy, dz] = _lerp(cor[dz][dy][0], z, cor[dz][dy][1], z, wx)
    col = {dz: _lerp(*row[0, dz], *row[1, dz], wy) for dz in (0, 1)}
    val, e_val = _lerp(*col[0], *col[1], wz)
    if not gradient:
        return e_val
    eg = np.zeros((len(c), 3))
    dx = {(dy, dz): _sub(cor[dz][dy][0], z, cor[dz][dy][1], z) for dy in (0, 1) for dz in (0, 1)}
    gx = {dz: _lerp(*dx[0, dz], *dx[1, dz], wy) for dz in (0, 1)}
    eg[:, 0] = _lerp(*gx[0], *gx[1], wz)[1]
    dyv = {dz: _sub(*row[0, dz], *row[1, dz]) for dz in (0, 1)}
    eg[:, 1] = _lerp(*dyv[0], *dyv[1], wz)[1]
    eg[:, 2] = _sub(*col[0], *col[1])[1]
    return e_val, eg


def footprint(img_shape, c):
    """Flat voxel indices of every voxel the kernel may read for the points c (both x, y, z neighbours of the clamped cell)."""
    n = np.array(img_shape[::-1], dtype=np.int64)
    b = np.floor(c).astype(np.int64)
    i0 = np.clip(b, 0, n[None, :] - 1)
    i1 = np.minimum(i0 + 1, n[None, :] - 1)
    idx = (i0, i1)
    out = [(idx[dz][:, 2] * n[1] + idx[dy][:, 1]) * n[0] + idx[dx][:, 0] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    return np.unique(np.concatenate(out))


# --------------------------------------------------------------------------------------
# one side of a sample, the pair, the margin


def _line_distance(c):
    """Distance of every point from the nearest integer or half-integer on any axis (grid lines, mask rounding, borders)."""
    t = 2.0 * c
    return (np.abs(t - np.round(t)) / 2.0).min(axis=1)


def _robustness(c, n, mask):
    """How far a point is from being ACCEPTED by this image, 0 if it is: the distance beyond the border on the worst axis, or
    -- inside, under a zero mask voxel -- the distance to the nearest mask cell boundary."""
    out_lo, out_hi = np.maximum(-0.5 - c, 0.0), np.maximum(c - (n[None, :] - 0.5), 0.0)
    rho = np.maximum(out_lo, out_hi).max(axis=1)
    ins = inside(c, n)
    if mask is not None:
        t = c + 0.5
        cell = np.abs(t - np.round(t)).min(axis=1)
        rho = np.where(ins & ~mask_at(mask, c), cell, rho)
    return ins, rho


class Samples:
    """Everything per sample: v, validity, f / m values, the moving gradient, their error bounds, and the margin."""

    def __init__(self, fixed, moving, Af, bf, Am, bm, vsize, stride, fixed_mask=None, moving_mask=None, jitter=None,
                 moving_gradient=None):
        self.v = v = lattice(vsize, stride, jitter)
        self.cf = points(Af, bf, v)
        self.in_f, self.rho_f = _robustness(self.cf, size_xyz(fixed), fixed_mask)
        self.ok_f = self.in_f if fixed_mask is None else self.in_f & mask_at(fixed_mask, self.cf)
        self.f_all = interp(fixed, self.cf)
        self.ef_all = interp_bound(fixed, self.cf)
        nm = size_xyz(moving)
        self.cm = points(Am, bm, v)
        in_m, rho_m = _robustness(self.cm, nm, moving_mask)
        ok_m = in_m if moving_mask is None else in_m & mask_at(moving_mask, self.cm)
        self.ok = self.ok_f & ok_m
        ok = self.ok
        self.count = int(ok.sum())
        # margin: an accepted sample counts with its distance from the nearest line of either image; a rejected one with the
        # distance it would have to move to be accepted (it stays rejected under any smaller perturbation)
        d = np.minimum(_line_distance(self.cf), _line_distance(self.cm))
        contrib = np.where(ok, d, np.maximum(self.rho_f, rho_m))
        self.margin = float(contrib.min()) if len(contrib) else np.inf
        self._nm = nm
        self.vv = v[ok]
        self.f, self.ef = self.f_all[ok], self.ef_all[ok]
        cmo = self.cm[ok]
        self.cmo, self.cfo = cmo, self.cf[ok]
        self.m = interp(moving, cmo)
        if moving_gradient is None:
            self.em, self.eg = interp_bound(moving, cmo, gradient=True)
            self.g = interp_gradient(moving, cmo)
        else:
            self.em = interp_bound(moving, cmo)
            self.g = np.stack([interp(moving_gradient[r], cmo) for r in range(3)], axis=1)
            self.eg = np.stack([interp_bound(moving_gradient[r], cmo) for r in range(3)], axis=1)

    def margin_of(self, exact=()):
        """The margin of a case whose sides in `exact` ("f", "m") have dyadic coefficients: those coordinates are the same
        under any evaluation order, their ties are part of the test, and only the other side's lines count."""
        if set(exact) == {"f", "m"}:
            return np.inf
        if "f" in exact:
            d = _line_distance(self.cm)
            _, rho_m = _robustness(self.cm, self._nm, None)
            return float(np.where(self.ok, d, np.maximum(rho_m, d)).min())
        return self.margin

    def terms(self):
        """The twelve derivative carriers g_r v_q (row-major 9) and g_r (3) per sample, with bounds."""
        n = len(self.f)
        t = np.concatenate([(self.g[:, :, None] * self.vv[:, None, :]).reshape(n, 9), self.g], axis=1)
        et = np.concatenate([(self.eg[:, :, None] * np.abs(self.vv)[:, None, :]).reshape(n, 9), self.eg], axis=1)
        return t, et


def _acc(n, mag):
    return n * U53 * mag


def meansq(s):
    """-> (14 sums, 14 bounds): sum (f - m)^2, count, d/dAm (9), d/dbm (3) with term -2 (f - m) g_r (v_q | 1)."""
    d, ed = s.f - s.m, s.ef + s.em
    t, et = s.terms()
    out, bound = np.zeros(14), np.zeros(14)
    n = len(d)
    out[0], out[1] = (d * d).sum(), n
    bound[0] = (2.0 * np.abs(d) * ed + ed * ed).sum() + _acc(n, (d * d).sum())
    out[2:] = (-2.0 * d[:, None] * t).sum(0)
    bound[2:] = (2.0 * (np.abs(d)[:, None] * et + ed[:, None] * np.abs(t) + ed[:, None] * et)).sum(0) + _acc(n, 2.0 * np.abs(d[:, None] * t).sum(0))
    return out, bound


def corr(s):
    """-> (42 moments, 42 bounds): count, sum f, m, f^2, m^2, f m; sum t (12), sum f t (12), sum m t (12)."""
    f, m, ef, em = s.f, s.m, s.ef, s.em
    t, et = s.terms()
    n = len(f)
    out, bound = np.zeros(42), np.zeros(42)
    out[0:6] = [n, f.sum(), m.sum(), (f * f).sum(), (m * m).sum(), (f * m).sum()]
    bound[1:6] = [ef.sum(), em.sum(), (2 * np.abs(f) * ef + ef * ef).sum(), (2 * np.abs(m) * em + em * em).sum(),
                  (np.abs(f) * em + np.abs(m) * ef + ef * em).sum()]
    bound[1:6] += _acc(n, np.array([np.abs(f).sum(), np.abs(m).sum(), (f * f).sum(), (m * m).sum(), np.abs(f * m).sum()]))
    out[6:18], bound[6:18] = t.sum(0), et.sum(0) + _acc(n, np.abs(t).sum(0))
    for base, a, ea in ((18, f, ef), (30, m, em)):
        out[base:base + 12] = (a[:, None] * t).sum(0)
        bound[base:base + 12] = (np.abs(a)[:, None] * et + ea[:, None] * np.abs(t) + ea[:, None] * et).sum(0) + _acc(n, np.abs(a[:, None] * t).sum(0))
    return out, bound


def values(metric, s):
    """One row of pp_metric_values_affine_f32: [sum (f - m)^2, count, 0 ...] or the six raw moments, with bounds."""
    out, bound = np.zeros(6), np.zeros(6)
    if metric == 0:
        o, b = meansq(s)
        out[:2], bound[:2] = o[:2], b[:2]
    else:
        o, b = corr(s)
        out[:], bound[:] = o[:6], b[:6]
    return out, bound


def meansq_value(sums):
    return sums[0] / sums[1]


def corr_value(mom):
    n = mom[0]
    sfm, sff, smm = mom[5] - mom[1] * mom[2] / n, mom[3] - mom[1] ** 2 / n, mom[4] - mom[2] ** 2 / n
    return -(sfm * sfm) / (sff * smm)


def value_bound(value_fn, sums, bound):
    """First-order bound of a scalar function of the sums: sum_k |d value / d sums_k| bound_k, derivatives by central differences
    at a step far above fp64 noise and far below the sums' own scale."""
    sums, tot = np.asarray(sums, dtype=np.float64), 0.0
    for k in np.nonzero(bound)[0]:
        h = 1e-6 * max(abs(sums[k]), 1.0)
        p, q = sums.copy(), sums.copy()
        p[k] += h
        q[k] -= h
        tot += abs(value_fn(p) - value_fn(q)) / (2 * h) * bound[k]
    return 1.01 * tot


# --------------------------------------------------------------------------------------
# mutual information


def bspline3(u):
    a = np.abs(u)
    return np.where(a < 1.0, 2.0 / 3.0 - a * a + 0.5 * a ** 3, np.where(a < 2.0, (2.0 - a) ** 3 / 6.0, 0.0))


def bspline3_d1(u):
    a = np.abs(u)
    return np.sign(u) * np.where(a < 1.0, -2.0 * a + 1.5 * a * a, np.where(a < 2.0, -0.5 * (2.0 - a) ** 2, 0.0))


def bspline3_d2(u):
    a = np.abs(u)
    return np.where(a < 1.0, -2.0 + 3.0 * a, np.where(a < 2.0, 2.0 - a, 0.0))


class MiSamples:
    """Bin coordinates of the accepted samples, their error, and which samples sit so close to a bin decision that fp32 and
    fp64 interpolation may take different sides (`amb`): the hard decisions are the fixed bin (both kernels), the moving bin
    (joint histogram) and the moving half-bin (joint gradient)."""

    def __init__(self, s, bins):
        self.s, self.nb, self.kernel = s, int(bins["nbins"]), int(bins["kernel"])
        self.pad = 2 if self.kernel == 0 else 0
        lo, hi = self.pad, self.nb - 1 - self.pad
        # one more rounding: the kernel holds the interpolated value as a float before it divides in fp64 (included in ef / em)
        self.tf, self.etf = s.f / bins["f_bin"] - bins["f_norm_min"], s.ef / bins["f_bin"]
        self.tm, self.etm = s.m / bins["m_bin"] - bins["m_norm_min"], s.em / bins["m_bin"]
        self.fb = np.clip(np.floor(self.tf).astype(np.int64), lo, hi)
        self.mb = np.clip(np.floor(self.tm).astype(np.int64), lo, hi)
        near = lambda t, e, shift=0.0: np.abs((t - shift) - np.round(t - shift)) <= e      # noqa: E731
        self.amb_f = near(self.tf, self.etf)
        self.amb_m = near(self.tm, self.etm)
        self.amb_h = near(self.tm, self.etm, 0.5)
        d = [np.abs(self.tf - np.round(self.tf)) - self.etf]
        if self.kernel == 1:
            d += [np.abs(self.tm - np.round(self.tm)) - self.etm, np.abs(self.tm - 0.5 - np.round(self.tm - 0.5)) - self.etm]
        self.bin_margin = float(min(k.min() for k in d)) if len(s.f) else np.inf


def mi_histogram(s, bins):
    """-> (hist [nb, nb], count, bound [nb, nb]).  Joint: the bound is 0 except in the bins an ambiguous sample may enter or
    leave (one unit per such sample).  Mattes: each of the four weights moves by |B'| etm + etm^2 and is quantised to 2^-32
    (half a unit per weight: 2^-33); an ambiguous fixed bin allows the sample's whole weight in the rows around it."""
    q = MiSamples(s, bins)
    nb = q.nb
    hist, bound = np.zeros((nb, nb)), np.zeros((nb, nb))
    if q.kernel == 0:
        for d in (-1, 0, 1, 2):
            k = q.mb + d
            u = k - q.tm
            w = bspline3(u)
            np.add.at(hist, (q.fb, k), w)
            np.add.at(bound, (q.fb, k), np.abs(bspline3_d1(u)) * q.etm + q.etm ** 2 + 2.0 ** -33)
        for i in np.nonzero(q.amb_f)[0]:
            bound[max(q.fb[i] - 1, 0):q.fb[i] + 2, max(q.mb[i] - 2, 0):q.mb[i] + 4] += 1.0
    else:
        np.add.at(hist, (q.fb, q.mb), 1.0)
        for i in np.nonzero(q.amb_f | q.amb_m)[0]:
            bound[max(q.fb[i] - 1, 0):q.fb[i] + 2, max(q.mb[i] - 1, 0):q.mb[i] + 2] += 1.0
    return hist, float(len(s.f)), bound, q


def mi_gradient(s, bins, table):
    """-> (12 sums, 12 bounds): sum_s w_s g_s (v_q | 1); w from the score table (which the library rounds to fp32: u |table|)."""
    q = MiSamples(s, bins)
    tab = np.asarray(table, dtype=np.float64)
    tmax = np.abs(tab).max()
    n = len(s.f)
    w, ew = np.zeros(n), np.zeros(n)
    if q.kernel == 0:
        for d in (-1, 0, 1, 2):
            k = q.mb + d
            u = k - q.tm
            tk = tab[q.fb, k]
            w += bspline3_d1(u) * tk
            ew += (np.abs(bspline3_d2(u)) * q.etm + 1.5 * q.etm ** 2) * np.abs(tk) + np.abs(bspline3_d1(u)) * U24 * np.abs(tk)
        amb = q.amb_f
    else:
        k0 = np.clip(np.floor(q.tm - 0.5).astype(np.int64), 0, q.nb - 2)
        w = tab[q.fb, k0 + 1] - tab[q.fb, k0]
        ew = U24 * (np.abs(tab[q.fb, k0 + 1]) + np.abs(tab[q.fb, k0]))
        amb = q.amb_f | q.amb_h
    ew = np.where(amb, np.abs(w) + 2.0 * tmax, ew)          # another bin: any weight the table allows
    t, et = s.terms()
    out = (w[:, None] * t).sum(0)
    bound = (ew[:, None] * np.abs(t) + np.abs(w)[:, None] * et + ew[:, None] * et).sum(0) + _acc(n, np.abs(w[:, None] * t).sum(0))
    return out, bound, q
