"""TEST ONLY: the arithmetic of the reference's imaging/dose/dvh.py and metric.py restated on host arrays with plain numpy
(np.histogram, np.percentile, np.interp), for tests/test_dose.py.  Arrays are [Z, Y, X]; spacing is (x, y, z) in mm.

Where the package deviates from numpy on a float32 dose it says so (platipy_amd/dose/dvh.py): the histogram compares the
dose as a double with float64 edges and the mean is a float64 sum, so the restatement casts the masked float32 values to
float64 for those two -- the reference's own arithmetic when its dose image is float64.  `mean_f32` is numpy's mean of the
float32 values as they are."""
import numpy as np


def masked(dose, mask):
    return dose[np.where(mask)]


def histogram(dose, mask, edges):
    return np.histogram(masked(dose, mask).astype(np.float64), bins=edges)[0]


def dvh(dose, mask, bins=1001):
    counts, edges = np.histogram(masked(dose, mask).astype(np.float64), bins=bins)
    centres = (edges[1:] + edges[:-1]) / 2.0
    values = np.cumsum(counts[::-1])[::-1]
    if np.all(values == 0):
        return centres, values
    return centres, values / values.max()


def dvh_edges(dose, bin_width=0.1, max_dose=None):
    if not max_dose:
        max_dose = float(dose.max())
    return np.arange(-bin_width / 2, max_dose + bin_width, bin_width)


def dvh_rows(dose, masks, spacing, bin_width=0.1, max_dose=None):
    """calculate_dvh_for_labels as a list of dicts (what the DataFrame is built from); masks: dict name -> array."""
    edges = dvh_edges(dose, bin_width, max_dose)
    rows = []
    for name, mask in masks.items():
        cc = mask.sum() * np.prod([a / 10 for a in spacing])
        centres, values = dvh(dose, mask, edges)
        centres = np.round(centres.astype(float), decimals=10)
        inside = dose[mask > 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = inside.astype(np.float64).mean() if inside.size else np.nan
            mean_f32 = inside.mean() if inside.size else np.nan
        rows.append({"label": name, "cc": cc, "mean": mean, "mean_f32": mean_f32, "bins": centres, "values": values})
    return rows


def frame(rows):
    import pandas as pd

    return pd.DataFrame([{"label": r["label"], "cc": r["cc"], "mean": r["mean"], **dict(zip(r["bins"], r["values"]))} for r in rows])


def _curves(df):
    bins = np.array([b for b in df.columns if isinstance(b, float)])
    return bins, np.array(df[bins])


def d_x(df, x):
    """-> {label: {f"D{x}": value}}"""
    bins, values = _curves(df)
    out = {}
    for idx in range(len(df)):
        m = {}
        for threshold in (x if isinstance(x, list) else [x]):
            value = np.interp(threshold / 100, values[idx][::-1], bins[::-1])
            if values[idx, 0] == np.sum(values[idx]):
                value = 0
            if threshold == 100:
                value = bins[np.where(values[idx] == 1.0)[0]][-1]
            m[f"D{threshold}"] = value
        out[df.iloc[idx].label] = m
    return out


def v_x(df, x):
    bins, values = _curves(df)
    out = {}
    for idx in range(len(df)):
        m = {}
        for threshold in (x if isinstance(x, list) else [x]):
            name = f"V{threshold}"
            if threshold - int(threshold) == 0:
                name = f"V{int(threshold)}"
            m[name] = np.interp(threshold, bins, values[idx]) * df.iloc[idx].cc
        out[df.iloc[idx].label] = m
    return out


def d_cc_x(df, x):
    out = {}
    for idx in range(len(df)):
        row = df.iloc[[idx]]
        m = {}
        for threshold in (x if isinstance(x, list) else [x]):
            cc_at = min((threshold / row.cc.iloc[0]) * 100, 100)
            m[f"D{threshold}cc"] = d_x(row, cc_at)[row.iloc[0].label][f"D{cc_at}"]
        out[row.iloc[0].label] = m
    return out


def d_to_volume(dose, mask, spacing, volume, volume_in_cc=False):
    if volume_in_cc:
        volume = (volume * 1000 / ((mask > 0).sum() * np.prod(spacing))) * 100
    if volume > 100:
        volume = 100
    return np.percentile(dose[mask > 0], 100 - volume)


def v_receiving_dose(dose, mask, spacing, threshold, relative=True):
    inside = dose[mask > 0]
    n = (mask > 0).sum()
    rel = (inside >= threshold).sum() / n * 100
    if relative:
        return rel
    return rel * (n * np.prod(spacing) / 1000)
