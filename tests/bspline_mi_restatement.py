"""TEST INFRASTRUCTURE: an fp64 restatement of Mattes mutual information over a cubic B-spline transform -- what
pp_bspline_mi_histogram_f32, the host's score table and pp_bspline_mi_gradient_f32 compute -- with a first-order error bound
next to every number, following the convention of tests/linear_metric_restatement.py (LR) and importing nothing from
platipy_amd.

  sample set, mapped points      tests/bspline_restatement.py (R): support, displacement
  values, gradient, fp32 bounds  LR.interp, LR.interp_gradient, LR.interp_bound (bsp_locate / bsp_lerp8 are the expression
                                 trees of the linear kernels)
  bins, ambiguity, histogram     LR.MiSamples, LR.mi_histogram, fed with an object that carries .f .ef .m .em

Gradient of coefficient p = (r, k, j, i):  sum_s w_s (g_s . Md)_r B_s,  w_s = sum_q B3'(q - tm_s) table[fb_s][q],
B_s = w_i w_j w_k.  Bound per term, derived and not tuned:
  ew |t| + |w| et + ew et      t = (g . Md)_r B, et its fp32 interpolation error, ew as LR.mi_gradient's (the window's second
                               derivative times the bin coordinate's error, and u |table| for the fp32 table)
  5 * 2^-24 |term|             the kernel forms B in fp32 from three fp32-rounded weights with two multiplications
  n 2^-53 sum |term|           the fp64 sums
"""
import numpy as np

from tests import bspline_restatement as R
from tests import linear_metric_restatement as LR


class Samples:
    """The valid samples of one evaluation: .f .ef .m .em (what LR.MiSamples reads), the moving gradient carried to the
    coefficient axes (.gp, .egp [n, 3]), the support of those inside the transform domain, and the four counts."""

    def __init__(self, fixed, fgeom, moving, mgeom, vgeom, stride, coef, lat, fixed_mask=None, moving_mask=None, jitter=None,
                 moving_gradient=None):
        fixed, moving = np.asarray(fixed, dtype=np.float64), np.asarray(moving, dtype=np.float64)
        v = LR.lattice(vgeom[0], stride, jitter)
        p = np.asarray(vgeom[2], dtype=np.float64)[None, :] + v @ R.i2p(vgeom[1], vgeom[3]).T
        inside, base, w = R.support(p, lat)
        d = R.displacement(p, coef, lat)
        p2i_f, p2i_m = np.linalg.inv(R.i2p(fgeom[1], fgeom[3])), np.linalg.inv(R.i2p(mgeom[1], mgeom[3]))
        cf = (p - np.asarray(fgeom[2], dtype=np.float64)[None, :]) @ p2i_f.T
        cm = (p + d - np.asarray(mgeom[2], dtype=np.float64)[None, :]) @ p2i_m.T
        in_buffer = LR.inside(cf, LR.size_xyz(fixed)) & LR.inside(cm, LR.size_xyz(moving))
        masked = np.zeros_like(in_buffer)
        if fixed_mask is not None:
            masked |= in_buffer & ~LR.mask_at(fixed_mask, cf)
        if moving_mask is not None:
            masked |= in_buffer & ~masked & ~LR.mask_at(moving_mask, cm)
        ok = in_buffer & ~masked
        self.stats = {"valid": int(ok.sum()), "outside": int((~in_buffer).sum()), "masked": int(masked.sum()), "seen": int(len(v))}
        cfo, cmo = cf[ok], cm[ok]
        self.f, self.ef = LR.interp(fixed, cfo), LR.interp_bound(fixed, cfo)
        self.m = LR.interp(moving, cmo)
        if moving_gradient is None:
            self.em, eg = LR.interp_bound(moving, cmo, gradient=True)
            g = LR.interp_gradient(moving, cmo)
        else:
            mg = np.asarray(moving_gradient, dtype=np.float64)
            self.em = LR.interp_bound(moving, cmo)
            g = np.stack([LR.interp(mg[r], cmo) for r in range(3)], axis=1)
            eg = np.stack([LR.interp_bound(mg[r], cmo) for r in range(3)], axis=1)
        self.gp, self.egp = g @ p2i_m, eg @ np.abs(p2i_m)        # d m / d c_r = sum_q g[q] p2i_m[q, r]
        self.inside, self.base, self.w = inside[ok], base[ok], w[ok]
        self.lattice_shape = tuple(int(s) for s in np.asarray(coef).shape[1:])      # (cz, cy, cx)


def bins(nbins, fixed, moving, fixed_mask=None, moving_mask=None):
    """PP_MI_MATTES bins of a level: width (max - min) / (nbins - 4), normalised minimum min / width - 2, the range taken
    inside the mask when one is given."""
    def rng(img, mask):
        a = np.asarray(img, dtype=np.float64)
        a = a[np.asarray(mask) != 0] if mask is not None and np.any(mask) else a
        return float(a.min()), float(a.max())

    (flo, fhi), (mlo, mhi) = rng(fixed, fixed_mask), rng(moving, moving_mask)
    fb, mb = (fhi - flo) / (nbins - 4), (mhi - mlo) / (nbins - 4)
    return {"nbins": int(nbins), "kernel": 0, "f_bin": fb, "f_norm_min": flo / fb - 2, "m_bin": mb, "m_norm_min": mlo / mb - 2}


def histogram(s, b):
    """-> (hist, bound, MiSamples): LR.mi_histogram; MiSamples.amb_f lists the ambiguous samples."""
    hist, _, bound, q = LR.mi_histogram(s, b)
    return hist, bound, q


def value_and_table(hist, count, m_bin):
    """negative mutual information of P = hist / sum (eps 1e-16) and table = log(P / PM) / (N m_bin)"""
    eps = 1e-16
    P = hist / hist.sum()
    PF, PM = P.sum(1)[:, None], P.sum(0)[None, :]
    ok = (P > eps) & (PF > eps) & (PM > eps)
    Ps = np.where(ok, P, 1.0)
    value = -float(np.where(ok, Ps * np.log(Ps / np.where(ok, PF * PM, 1.0)), 0.0).sum())
    table = np.where(ok, np.log(Ps / np.where(ok, PM * np.ones_like(P), 1.0)), 0.0) / (count * m_bin)
    return value, table


def value_bound(hist, bound):
    """First-order bound of the value for a histogram within `bound` of `hist`: d value / d hist_ij = -(log r_ij + value) / S with
    r = P / (PF PM), S = sum hist.  A bin at or below eps contributes nothing on either side of it and at most
    eps |log eps| <= 37 eps once it crosses: 40 / S per unit covers both."""
    eps = 1e-16
    S = hist.sum()
    P = hist / S
    PF, PM = P.sum(1)[:, None], P.sum(0)[None, :]
    ok = (P > eps) & (PF > eps) & (PM > eps)
    value = value_and_table(hist, S, 1.0)[0]
    slope = np.where(ok, np.abs(np.log(np.where(ok, P, 1.0) / np.where(ok, PF * PM, 1.0)) + value), 40.0) / S
    return 1.01 * float((slope * bound).sum()) + 1e-15


def gradient(s, b, table):
    """-> (gradient [3 ncp] in ITK's order, bound [3 ncp], MiSamples)"""
    q = LR.MiSamples(s, b)
    tab = np.asarray(table, dtype=np.float64)
    tmax = np.abs(tab).max()
    n = len(s.f)
    w, ew = np.zeros(n), np.zeros(n)
    for d in (-1, 0, 1, 2):
        k = q.mb + d
        u = k - q.tm
        tk = tab[q.fb, k]
        w += LR.bspline3_d1(u) * tk
        ew += (np.abs(LR.bspline3_d2(u)) * q.etm + 1.5 * q.etm ** 2) * np.abs(tk) + np.abs(LR.bspline3_d1(u)) * LR.U24 * np.abs(tk)
    ew = np.where(q.amb_f, np.abs(w) + 2.0 * tmax, ew)          # another fixed bin: any weight the table allows
    cz, cy, cx = s.lattice_shape
    ncp = cx * cy * cz
    ins = s.inside
    base, ww = s.base[ins], s.w[ins]
    w, ew, gp, egp = w[ins], ew[ins], s.gp[ins], s.egp[ins]
    out, bound, mag = np.zeros(3 * ncp), np.zeros(3 * ncp), np.zeros(3 * ncp)
    for k in range(4):
        for j in range(4):
            for i in range(4):
                cp = ((base[:, 2] + k) * cy + (base[:, 1] + j)) * cx + (base[:, 0] + i)
                B = ww[:, 0, i] * ww[:, 1, j] * ww[:, 2, k]
                for r in range(3):
                    t, et = gp[:, r] * B, egp[:, r] * B
                    term = w * t
                    e = ew * np.abs(t) + np.abs(w) * et + ew * et + 5.0 * LR.U24 * np.abs(term)
                    sl = slice(r * ncp, (r + 1) * ncp)
                    out[sl] += np.bincount(cp, weights=term, minlength=ncp)
                    bound[sl] += np.bincount(cp, weights=e, minlength=ncp)
                    mag[sl] += np.bincount(cp, weights=np.abs(term), minlength=ncp)
    return out, bound + len(w) * LR.U53 * mag, q


def outside_support(s):
    """[3 ncp] bool: coefficients no valid sample inside the domain touches"""
    cz, cy, cx = s.lattice_shape
    ncp = cx * cy * cz
    hit = np.zeros(ncp, dtype=bool)
    base = s.base[s.inside]
    for k in range(4):
        for j in range(4):
            for i in range(4):
                hit[((base[:, 2] + k) * cy + (base[:, 1] + j)) * cx + (base[:, 0] + i)] = True
    return np.tile(~hit, 3)


def metric(fixed, fgeom, moving, mgeom, vgeom, stride, coef, lat, nbins, fixed_mask=None, moving_mask=None, jitter=None, moving_gradient=None,
           bins_of=None):
    """-> (value, gradient, stats): the whole evaluation, for the optimiser and the central differences.  bins_of: the bins
    (fixed across a level) or None to take them from these images."""
    s = Samples(fixed, fgeom, moving, mgeom, vgeom, stride, coef, lat, fixed_mask, moving_mask, jitter, moving_gradient)
    b = bins_of if bins_of is not None else bins(nbins, fixed, moving, fixed_mask, moving_mask)
    hist, _, _ = histogram(s, b)
    value, table = value_and_table(hist, float(s.stats["valid"]), b["m_bin"])
    g, _, _ = gradient(s, b, table)
    return value, g, s.stats
