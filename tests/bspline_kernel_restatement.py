"""TEST INFRASTRUCTURE: an fp64 restatement of mean squares and correlation over a cubic B-spline transform -- what
pp_bspline_metric_f32 computes -- with a first-order error bound next to every number, built on the sample set of
tests/bspline_mi_restatement.py (RM.Samples: .f .ef .m .em .gp .egp .inside .base .w and the four counts) and following the
convention of tests/linear_metric_restatement.py (LR).  Imports nothing from platipy_amd.  Also the grids the geometry tests
sample on (shrunk by ITK's rule, grown, refined), stated here and not taken from the product.

n = the number of valid samples; B_s = w_i w_j w_k of sample s for control point (i, j, k); d = f - m, ed = ef + em;
u = 2^-24.  Only valid samples inside the transform domain reach a gradient; every valid sample reaches the scalars.

Mean squares.  value = sum d^2 / n, bound [sum (2 |d| ed + ed^2) + n 2^-53 sum d^2] / n.  Gradient of coefficient p = (r, k, j, i):
sum_s term_s, term = -2 d gp_r B / n.  Bound per term, derived and not tuned:
  2 [ed |gp_r| + |d| egp_r + ed egp_r] B / n   f, m and the moving gradient are interpolated in fp32 (LR.interp_bound); the
                                               differences and products after them are fp64
  5 u |term|                                   the kernel forms B in fp32 from three fp32-rounded weights with two multiplications
  n 2^-53 sum |term|                           the fp64 sums (rows, slabs, cells: n additions at the most on the way to one entry)
  4 * 2^-149 |term / B|                        where B leaves fp32's normal range the 5 u above no longer hold: a weight below
                                               2^-126 is rounded to a multiple of 2^-149 and so is each of the two products
                                               (`underflow_floor`).  A sample whose voxel centre lies ON a cell face has a
                                               weight t^3 / 6 with t = 0 or one rounding of the coordinate, 1e-16: 0 on one
                                               side, 1e-49 on the other.  At most 1e-44 of the gradient's scale

Correlation.  The kernel adds three rows G, FG, MG = sum (1 | f | m) gp_r B and the moments S = sum f, m, f^2, m^2, f m, then
  out_p = -(a (FG - fbar G) - b 2 (MG - mbar G)),  a = 2 sfm / (sff smm),  b = sfm^2 / (sff smm^2),
  sff = S_ff - n fbar^2, smm = S_mm - n mbar^2, sfm = S_fm - n fbar mbar,  value = -sfm^2 / (sff smm).
Bounds of the sums, term by term with t = gp_r B, et = egp_r B:
  G    et + 5 u |t|                                          + n 2^-53 sum |t|
  FG   |f| et + ef |t| + ef et + 5 u |f t|                   + n 2^-53 sum |f t|          (MG alike with m, em)
  S    ef | em | 2 |f| ef + ef^2 | 2 |m| em + em^2 | |f| em + |m| ef + ef em, each + n 2^-53 sum |term|   (LR.corr's)
They are carried through the formula to first order, as RM.value_bound carries the histogram's: out_p is linear in its three
sums (d out / d FG = -a, d out / d MG = 2 b, d out / d G = a fbar - 2 b mbar), and the derivatives with respect to the five
moments are central differences at a step far above fp64 noise and far below the moments' own scale (LR.value_bound's way).
1.01 covers the second-order terms (the sums are good to 1e-6 of themselves or better).
"""
import numpy as np

from tests import linear_metric_restatement as LR


# ---- grids ---------------------------------------------------------------------------------------------------------------


def shrunk(geom, factor):
    """itk::ShrinkImageFilter's output grid: size floor(n / f), spacing f times, the same physical centre."""
    size, sp, org, D = geom
    n, f = np.asarray(size, dtype=np.float64), np.broadcast_to(np.asarray(factor, dtype=np.float64), (3,))
    D = np.asarray(D, dtype=np.float64).reshape(3, 3)
    out_n = np.floor(n / f)
    out_sp = np.asarray(sp, dtype=np.float64) * f
    centre = np.asarray(org, dtype=np.float64) + D @ (np.asarray(sp, dtype=np.float64) * (n - 1.0) / 2.0)
    return tuple(int(k) for k in out_n), tuple(out_sp), tuple(centre - D @ (out_sp * (out_n - 1.0) / 2.0)), D


def grown(geom, pad):
    """the grid with `pad` more voxels on every side"""
    size, sp, org, D = geom
    D = np.asarray(D, dtype=np.float64).reshape(3, 3)
    return tuple(int(k) + 2 * pad for k in size), tuple(sp), tuple(np.asarray(org, dtype=np.float64) - D @ (pad * np.asarray(sp, dtype=np.float64))), D


def refined(geom):
    """half the spacing, twice the voxels, the origin a quarter of a (coarse) voxel earlier: the same box"""
    size, sp, org, D = geom
    D = np.asarray(D, dtype=np.float64).reshape(3, 3)
    sp = np.asarray(sp, dtype=np.float64)
    return tuple(2 * int(k) for k in size), tuple(0.5 * sp), tuple(np.asarray(org, dtype=np.float64) - D @ (0.25 * sp)), D


# ---- the two metrics -----------------------------------------------------------------------------------------------------


def _scatter(s, weight, unit=False):
    """sum over the valid samples inside the domain of weight[:, r] * w_i w_j w_k -> [3 * ncp] (ITK's parameter order); unit: B = 1"""
    cz, cy, cx = s.lattice_shape
    ncp = cx * cy * cz
    ins = s.inside
    base, ww, wt = s.base[ins], s.w[ins], weight[ins]
    out = np.zeros(3 * ncp)
    for k in range(4):
        for j in range(4):
            for i in range(4):
                cp = ((base[:, 2] + k) * cy + (base[:, 1] + j)) * cx + (base[:, 0] + i)
                B = 1.0 if unit else ww[:, 0, i] * ww[:, 1, j] * ww[:, 2, k]
                for r in range(3):
                    out[r * ncp:(r + 1) * ncp] += np.bincount(cp, weights=wt[:, r] * B, minlength=ncp)
    return out


def underflow_floor(s, magnitude):
    """[3 ncp]: 4 * 2^-149 times the sum of magnitude[:, r] (a bound of |term / B|) over the samples that reach a coefficient"""
    return 4.0 * 2.0 ** -149 * _scatter(s, magnitude, unit=True)


def mean_squares(s):
    """RM.Samples -> (value, gradient [3 ncp], value_bound, bound [3 ncp])"""
    n = len(s.f)
    d, ed = s.f - s.m, s.ef + s.em
    value = float((d * d).sum() / n)
    value_bound = float(((2.0 * np.abs(d) * ed + ed * ed).sum() + n * LR.U53 * (d * d).sum()) / n)
    term = (-2.0 * d)[:, None] * s.gp / n
    e = 2.0 * (ed[:, None] * np.abs(s.gp) + np.abs(d)[:, None] * s.egp + ed[:, None] * s.egp) / n + 5.0 * LR.U24 * np.abs(term)
    ninside = int(s.inside.sum())
    floor = underflow_floor(s, 2.0 * (np.abs(d) + ed)[:, None] * (np.abs(s.gp) + s.egp) / n)
    return value, _scatter(s, term), value_bound, _scatter(s, e) + ninside * LR.U53 * _scatter(s, np.abs(term)) + floor


def _corr_gradient(G, FG, MG, S, n):
    """k_bsp_gather<1>'s formula.  S = sum f, m, f^2, m^2, f m"""
    fbar, mbar = S[0] / n, S[1] / n
    sff, smm, sfm = S[2] - n * fbar * fbar, S[3] - n * mbar * mbar, S[4] - n * fbar * mbar
    return -(2.0 * sfm / (sff * smm) * (FG - fbar * G) - (sfm * sfm) / (sff * smm * smm) * 2.0 * (MG - mbar * G))


def correlation(s):
    """RM.Samples -> (value, gradient [3 ncp], value_bound, bound [3 ncp]); the variances must not vanish"""
    f, m, ef, em = s.f, s.m, s.ef, s.em
    n = len(f)
    ninside = int(s.inside.sum())
    S = np.array([f.sum(), m.sum(), (f * f).sum(), (m * m).sum(), (f * m).sum()])
    eS = np.array([ef.sum(), em.sum(), (2 * np.abs(f) * ef + ef * ef).sum(), (2 * np.abs(m) * em + em * em).sum(),
                   (np.abs(f) * em + np.abs(m) * ef + ef * em).sum()])
    eS += n * LR.U53 * np.array([np.abs(f).sum(), np.abs(m).sum(), (f * f).sum(), (m * m).sum(), np.abs(f * m).sum()])
    t, et = s.gp, s.egp
    G = _scatter(s, t)
    eG = _scatter(s, et + 5.0 * LR.U24 * np.abs(t)) + ninside * LR.U53 * _scatter(s, np.abs(t)) + underflow_floor(s, np.abs(t) + et)
    sums, esums = [G], [eG]
    for a, ea in ((f, ef), (m, em)):
        at = a[:, None] * t
        sums.append(_scatter(s, at))
        esums.append(_scatter(s, np.abs(a)[:, None] * et + ea[:, None] * np.abs(t) + ea[:, None] * et + 5.0 * LR.U24 * np.abs(at))
                     + ninside * LR.U53 * _scatter(s, np.abs(at)) + underflow_floor(s, (np.abs(a) + ea)[:, None] * (np.abs(t) + et)))
    G, FG, MG = sums
    eG, eFG, eMG = esums
    fbar, mbar = S[0] / n, S[1] / n
    sff, smm, sfm = S[2] - n * fbar * fbar, S[3] - n * mbar * mbar, S[4] - n * fbar * mbar
    assert sff > 0 and smm > 0
    a, b = 2.0 * sfm / (sff * smm), (sfm * sfm) / (sff * smm * smm)
    gradient = _corr_gradient(G, FG, MG, S, n)
    bound = np.abs(a) * eFG + np.abs(2.0 * b) * eMG + np.abs(a * fbar - 2.0 * b * mbar) * eG
    for k in range(5):
        h = 1e-6 * max(abs(S[k]), 1.0)
        p, q = S.copy(), S.copy()
        p[k] += h
        q[k] -= h
        bound = bound + np.abs(_corr_gradient(G, FG, MG, p, n) - _corr_gradient(G, FG, MG, q, n)) / (2 * h) * eS[k]
    mom, emom = np.concatenate([[n], S]), np.concatenate([[0.0], eS])
    return float(LR.corr_value(mom)), gradient, float(LR.value_bound(LR.corr_value, mom, emom)), 1.01 * bound


def metric(kind, s):
    return mean_squares(s) if kind == "mean_squares" else correlation(s)
