"""The feature formulas of pyradiomics' firstorder, glcm, glrlm, gldm and ngtdm classes, in fp64 numpy on the small tables the
kernels of csrc/pp_radiomics.h return (a few hundred KB at most).  Nothing here touches a voxel.

pyradiomics is not installed where this was written: the semantics are RECALLED from pyradiomics 3.x and marked Q1 ... where
they are decided (DESIGN.md 4.16 lists them); parity with pyradiomics is unpinned.

Shared conventions.  Grey levels that hold no voxel are dropped from a table before its features (Q5); a row keeps its
level's own value i.  Ng is the largest level (Q4).  Q6: eps = 2.2e-16 inside every log2.
"""
import numpy as np

EPS = 2.2e-16

FIRSTORDER = ("Energy", "TotalEnergy", "Entropy", "Minimum", "10Percentile", "90Percentile", "Maximum", "Mean", "Median",
              "InterquartileRange", "Range", "MeanAbsoluteDeviation", "RobustMeanAbsoluteDeviation", "RootMeanSquared", "Skewness",
              "Kurtosis", "Variance", "Uniformity")
GLCM = ("Autocorrelation", "JointAverage", "ClusterProminence", "ClusterShade", "ClusterTendency", "Contrast", "Correlation",
        "DifferenceAverage", "DifferenceEntropy", "DifferenceVariance", "JointEnergy", "JointEntropy", "Imc1", "Imc2", "Idm", "Idmn", "Id",
        "Idn", "InverseVariance", "MaximumProbability", "SumAverage", "SumEntropy", "SumSquares", "MCC")
GLRLM = ("ShortRunEmphasis", "LongRunEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized", "RunLengthNonUniformity",
         "RunLengthNonUniformityNormalized", "RunPercentage", "GrayLevelVariance", "RunVariance", "RunEntropy", "LowGrayLevelRunEmphasis",
         "HighGrayLevelRunEmphasis", "ShortRunLowGrayLevelEmphasis", "ShortRunHighGrayLevelEmphasis", "LongRunLowGrayLevelEmphasis",
         "LongRunHighGrayLevelEmphasis")
GLDM = ("SmallDependenceEmphasis", "LargeDependenceEmphasis", "GrayLevelNonUniformity", "DependenceNonUniformity",
        "DependenceNonUniformityNormalized", "GrayLevelVariance", "DependenceVariance", "DependenceEntropy", "LowGrayLevelEmphasis",
        "HighGrayLevelEmphasis", "SmallDependenceLowGrayLevelEmphasis", "SmallDependenceHighGrayLevelEmphasis",
        "LargeDependenceLowGrayLevelEmphasis", "LargeDependenceHighGrayLevelEmphasis")
NGTDM = ("Coarseness", "Contrast", "Busyness", "Complexity", "Strength")
CUSTOM = ("25Percentile", "75Percentile")

# The parts of firstorder()'s input beyond count, sum, minimum, maximum and voxel_volume, and the features that read each:
# a part is made only when one of them is asked for.
FIRSTORDER_NEEDS = {
    "pct": ("10Percentile", "90Percentile", "Median", "InterquartileRange"),
    "m": ("Energy", "TotalEnergy", "MeanAbsoluteDeviation", "RootMeanSquared", "Skewness", "Kurtosis", "Variance"),
    "robust": ("RobustMeanAbsoluteDeviation",),
    "hist": ("Entropy", "Uniformity"),
}

FEATURES = {"firstorder": FIRSTORDER, "glcm": GLCM, "glrlm": GLRLM, "gldm": GLDM, "ngtdm": NGTDM, "custom": CUSTOM}


def _entropy(p):
    return float(-np.sum(p * np.log2(p + EPS)))


def percentile_rank(n, q):
    """np.percentile's linear rule on n sorted values -> (lower index, upper index, weight of the upper one)."""
    virtual = (n - 1) * (q / 100.0)
    lo = int(np.floor(virtual))
    return lo, min(lo + 1, n - 1), virtual - lo


def percentile_value(a, b, t):
    """numpy's lerp between the two order statistics, in fp64."""
    a, b = float(a), float(b)
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


def firstorder(names, s):
    """s: count, sum (exact), minimum, maximum, pct {q: value}, m (the sums about the mean: S|d|, S d^2, S d^3, S d^4, S v^2),
    robust (count, S|v - their mean|) over the values in [P10, P90], hist (voxels per grey level), voxel_volume; pct, m,
    robust and hist only where `names` holds a feature that reads them (FIRSTORDER_NEEDS).  No value need lie in
    [P10, P90]: then the robust MAD is the mean of an empty set, NaN.
    Q7: voxelArrayShift = 0.  Q8: Entropy and Uniformity use the discretised histogram.  Q9: Kurtosis is not the excess.
    Q10: percentiles by np.percentile's linear rule.  Q11: the robust MAD is taken over the values in [P10, P90] about their
    own mean.  Q12: TotalEnergy = Energy x voxel volume."""
    n = float(s["count"])
    mean = s["sum"] / n
    if "m" in s:
        sabs, m2, m3, m4, energy = (float(x) for x in s["m"])
        m2, m3, m4 = m2 / n, m3 / n, m4 / n
    if "hist" in s:
        p = s["hist"][s["hist"] > 0].astype(np.float64)
        p = p / p.sum()
    out = {}
    for name in names:
        if name == "Energy":
            v = energy
        elif name == "TotalEnergy":
            v = energy * s["voxel_volume"]
        elif name == "Entropy":
            v = _entropy(p)
        elif name == "Minimum":
            v = s["minimum"]
        elif name == "Maximum":
            v = s["maximum"]
        elif name == "10Percentile":
            v = s["pct"][10]
        elif name == "90Percentile":
            v = s["pct"][90]
        elif name == "Mean":
            v = mean
        elif name == "Median":
            v = s["pct"][50]
        elif name == "InterquartileRange":
            v = s["pct"][75] - s["pct"][25]
        elif name == "Range":
            v = s["maximum"] - s["minimum"]
        elif name == "MeanAbsoluteDeviation":
            v = sabs / n
        elif name == "RobustMeanAbsoluteDeviation":
            v = s["robust"][1] / s["robust"][0] if s["robust"][0] else np.nan
        elif name == "RootMeanSquared":
            v = np.sqrt(energy / n)
        elif name == "Skewness":
            v = 0.0 if m2 == 0.0 else m3 / m2 ** 1.5
        elif name == "Kurtosis":
            v = 0.0 if m2 == 0.0 else m4 / m2 ** 2
        elif name == "Variance":
            v = m2
        elif name == "Uniformity":
            v = float(np.sum(p * p))
        else:
            raise KeyError(name)
        out[name] = float(v)
    return out


def custom(names, s):
    return {name: float(s["pct"][int(name[:2])]) for name in names}


def _nanmean(rows, names):
    """Features are computed per direction and averaged with nanmean (Q15, Q18)."""
    out = {}
    for name in names:
        v = np.array([r[name] for r in rows], dtype=np.float64)
        v = v[~np.isnan(v)]
        out[name] = float(v.mean()) if v.size else float("nan")
    return out


def _glcm_direction(P, lv, ng):
    """One direction's symmetric counts (empty levels dropped) -> every feature.  lv: the levels of the rows."""
    P = P / P.sum()
    i, j = lv[:, None], lv[None, :]
    px, py = P.sum(1), P.sum(0)
    ux, uy = float((i * P).sum()), float((j * P).sum())
    k_add, k_sub = (i + j).astype(np.int64), np.abs(i - j).astype(np.int64)
    p_add = np.bincount(k_add.ravel(), weights=P.ravel(), minlength=2 * ng + 1)[2:]
    p_sub = np.bincount(k_sub.ravel(), weights=P.ravel(), minlength=ng)
    ka, ks = np.arange(2, 2 * ng + 1, dtype=np.float64), np.arange(0, ng, dtype=np.float64)
    hxy = _entropy(P)
    hx, hy = _entropy(px), _entropy(py)
    pxpy = px[:, None] * py[None, :]
    hxy1 = float(-np.sum(P * np.log2(pxpy + EPS)))
    hxy2 = float(-np.sum(pxpy * np.log2(pxpy + EPS)))
    sigx, sigy = np.sqrt(float((P * (i - ux) ** 2).sum())), np.sqrt(float((P * (j - uy) ** 2).sum()))
    f = {}
    f["Autocorrelation"] = float((P * i * j).sum())
    f["JointAverage"] = ux
    f["ClusterProminence"] = float((P * (i + j - ux - uy) ** 4).sum())
    f["ClusterShade"] = float((P * (i + j - ux - uy) ** 3).sum())
    f["ClusterTendency"] = float((P * (i + j - ux - uy) ** 2).sum())
    f["Contrast"] = float((P * (i - j) ** 2).sum())
    f["Correlation"] = 1.0 if sigx * sigy == 0.0 else float((P * (i - ux) * (j - uy)).sum()) / (sigx * sigy)     # a flat region: 1
    da = float((ks * p_sub).sum())
    f["DifferenceAverage"] = da
    f["DifferenceEntropy"] = _entropy(p_sub)
    f["DifferenceVariance"] = float(((ks - da) ** 2 * p_sub).sum())
    f["JointEnergy"] = float((P * P).sum())
    f["JointEntropy"] = hxy
    f["Imc1"] = 0.0 if max(hx, hy) == 0.0 else (hxy - hxy1) / max(hx, hy)
    f["Imc2"] = 0.0 if hxy > hxy2 else float(np.sqrt(1.0 - np.exp(-2.0 * (hxy2 - hxy))))
    f["Idm"] = float((p_sub / (1.0 + ks ** 2)).sum())
    f["Idmn"] = float((p_sub / (1.0 + ks ** 2 / ng ** 2)).sum())
    f["Id"] = float((p_sub / (1.0 + ks)).sum())
    f["Idn"] = float((p_sub / (1.0 + ks / ng)).sum())
    f["InverseVariance"] = float((p_sub[1:] / ks[1:] ** 2).sum())
    f["MaximumProbability"] = float(P.max())
    f["SumAverage"] = float((ka * p_add).sum())
    f["SumEntropy"] = _entropy(p_add)
    f["SumSquares"] = float((P * (i - ux) ** 2).sum())
    if lv.size == 1:
        f["MCC"] = 1.0
    else:
        Q = (P / (px[:, None] + EPS)) @ (P / (py[None, :] + EPS)).T       # Q[i, j] = sum_k P[i, k] P[j, k] / (px[i] py[k])
        ev = np.sort(np.linalg.eigvals(Q).real)
        f["MCC"] = float(np.sqrt(max(ev[-2], 0.0)))
    return f


def glcm(names, forward, levels_present):
    """forward: int64 [13, Ng, Ng], the forward neighbour counts.  Q13: distance 1, 13 directions, symmetric (P + P^T), both
    voxels inside the mask.  Q14: each direction is normalised by its own sum.  Q15: features per direction, nanmean;
    a direction without a pair is left out."""
    ng = forward.shape[1]
    keep = np.asarray(levels_present, dtype=np.int64) - 1
    lv = (keep + 1).astype(np.float64)
    rows = []
    for d in range(forward.shape[0]):
        P = (forward[d] + forward[d].T)[np.ix_(keep, keep)].astype(np.float64)
        if P.sum() > 0:
            rows.append(_glcm_direction(P, lv, ng))
    if not rows:
        return {name: float("nan") for name in names}
    return _nanmean(rows, names)


def _emphasis_table(P, lv, jv):
    """The features the run-length and the dependence matrix share.  P [levels, sizes] counts, jv: the sizes of the columns."""
    i2, j2 = (lv ** 2)[:, None], (jv ** 2)[None, :]
    pg, pj = P.sum(1), P.sum(0)
    n = P.sum()
    p = P / n
    ug, uj = float((pg / n * lv).sum()), float((pj / n * jv).sum())
    return {
        "small": float((pj / jv ** 2).sum() / n), "large": float((pj * jv ** 2).sum() / n),
        "gln": float((pg ** 2).sum() / n), "glnn": float((pg ** 2).sum() / n ** 2),
        "sn": float((pj ** 2).sum() / n), "snn": float((pj ** 2).sum() / n ** 2),
        "glv": float((pg / n * (lv - ug) ** 2).sum()), "sv": float((pj / n * (jv - uj) ** 2).sum()),
        "entropy": _entropy(p), "low": float((pg / lv ** 2).sum() / n), "high": float((pg * lv ** 2).sum() / n),
        "small_low": float((P / (i2 * j2)).sum() / n), "small_high": float((P * i2 / j2).sum() / n),
        "large_low": float((P * j2 / i2).sum() / n), "large_high": float((P * i2 * j2).sum() / n),
    }


def glrlm(names, runs, levels_present, nvoxels):
    """runs: int64 [13, Ng, Nr].  Q16: maximal runs along the 13 directions inside the mask.  Q17: empty run-length columns
    are dropped (they add nothing to any sum).  Q18: features per direction, averaged."""
    keep = np.asarray(levels_present, dtype=np.int64) - 1
    lv = (keep + 1).astype(np.float64)
    rows = []
    for d in range(runs.shape[0]):
        P = runs[d][keep].astype(np.float64)
        cols = np.flatnonzero(P.sum(0) > 0)
        if cols.size == 0:
            continue
        e = _emphasis_table(P[:, cols], lv, (cols + 1).astype(np.float64))
        rows.append({
            "ShortRunEmphasis": e["small"], "LongRunEmphasis": e["large"], "GrayLevelNonUniformity": e["gln"],
            "GrayLevelNonUniformityNormalized": e["glnn"], "RunLengthNonUniformity": e["sn"], "RunLengthNonUniformityNormalized": e["snn"],
            "RunPercentage": float(P.sum() / nvoxels), "GrayLevelVariance": e["glv"], "RunVariance": e["sv"], "RunEntropy": e["entropy"],
            "LowGrayLevelRunEmphasis": e["low"], "HighGrayLevelRunEmphasis": e["high"], "ShortRunLowGrayLevelEmphasis": e["small_low"],
            "ShortRunHighGrayLevelEmphasis": e["small_high"], "LongRunLowGrayLevelEmphasis": e["large_low"],
            "LongRunHighGrayLevelEmphasis": e["large_high"]})
    return _nanmean(rows, names)


def gldm(names, table, levels_present):
    """table: int64 [Ng, 27].  Q19: 26 neighbours, alpha = 0 (a neighbour depends when it has the same level).  Q20: column j
    holds the voxels with j - 1 dependent neighbours, i.e. the dependence size is that number plus 1."""
    keep = np.asarray(levels_present, dtype=np.int64) - 1
    P = table[keep].astype(np.float64)
    cols = np.flatnonzero(P.sum(0) > 0)
    e = _emphasis_table(P[:, cols], (keep + 1).astype(np.float64), (cols + 1).astype(np.float64))
    f = {"SmallDependenceEmphasis": e["small"], "LargeDependenceEmphasis": e["large"], "GrayLevelNonUniformity": e["gln"],
         "DependenceNonUniformity": e["sn"], "DependenceNonUniformityNormalized": e["snn"], "GrayLevelVariance": e["glv"],
         "DependenceVariance": e["sv"], "DependenceEntropy": e["entropy"], "LowGrayLevelEmphasis": e["low"], "HighGrayLevelEmphasis": e["high"],
         "SmallDependenceLowGrayLevelEmphasis": e["small_low"], "SmallDependenceHighGrayLevelEmphasis": e["small_high"],
         "LargeDependenceLowGrayLevelEmphasis": e["large_low"], "LargeDependenceHighGrayLevelEmphasis": e["large_high"]}
    return {name: f[name] for name in names}


def ngtdm_columns(n_table, s_table):
    """The integer tables -> (levels, p_i, n_i, s_i) for the levels that hold a voxel.  Q21: 26 neighbours inside the mask.
    Q22: a voxel with no neighbour inside the mask counts for p_i but not for n_i and s_i.  s_i = sum_k S[i][k] / k in fp64,
    the k ascending."""
    total = n_table.sum(1)
    keep = np.flatnonzero(total > 0)
    k = np.arange(1, n_table.shape[1], dtype=np.float64)
    s = np.zeros(keep.size, dtype=np.float64)
    for c in range(k.size):                      # a fixed order of the 26 terms
        s += s_table[keep, c + 1].astype(np.float64) / k[c]
    n = n_table[keep, 1:].sum(1).astype(np.float64)
    p = total[keep].astype(np.float64) / float(total.sum())
    return (keep + 1).astype(np.float64), p, n, s


def ngtdm(names, n_table, s_table):
    lv, p, n, s = ngtdm_columns(n_table, s_table)
    nvp, ngp = float(n.sum()), lv.size
    pi, pj = p[:, None], p[None, :]
    ii, jj = lv[:, None], lv[None, :]
    ps = float((p * s).sum())
    f = {}
    f["Coarseness"] = 1.0e6 if ps == 0.0 else 1.0 / ps
    f["Contrast"] = 0.0 if ngp == 1 or nvp == 0.0 else float((pi * pj * (ii - jj) ** 2).sum()) / (ngp * (ngp - 1)) * float(s.sum()) / nvp
    den = float(np.abs(ii * pi - jj * pj).sum())
    f["Busyness"] = 0.0 if den == 0.0 else ps / den
    f["Complexity"] = float("nan") if nvp == 0.0 else float((np.abs(ii - jj) * (pi * s[:, None] + pj * s[None, :]) / (pi + pj)).sum()) / nvp
    ssum = float(s.sum())
    f["Strength"] = 0.0 if ssum == 0.0 else float(((pi + pj) * (ii - jj) ** 2).sum()) / ssum
    return {name: f[name] for name in names}
