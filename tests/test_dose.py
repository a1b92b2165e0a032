"""pa.dose (dose-volume histograms and dose metrics) and its kernels -- pp_dose_histogram_f32, pp_masked_order_stats_f32,
pp_masked_count_ge_f32 -- against the numpy restatement of the reference's arithmetic (tests/dose_restatement.py).

Inputs: a 14 x 23 x 29 volume (9338 voxels: the 16-byte mask loads get a tail) with a dose on a 0.05 Gy grid, so that nearly
every voxel sits on or beside an edge of the 0.1 Gy histogram, a few negative voxels and a few exactly on a top edge.

Limits stated by the library and checked here: at most 64 labels per call, at most 2^20 bins.

Tolerances
  histogram counts, voxel counts, mask-value sums, threshold counts: EQUAL numpy's.
  min, max, order statistics: bit-equal.
  dose sum: |kernel - numpy fp64 sum| <= count * 2^-52 * sum on a non-negative dose, the reordering bound of an fp64 sum of
      non-negative terms (the kernel's sum is exact and rounded once).
  mean: that bound against the fp64 mean; rtol 2^-20 against numpy's own fp32 pairwise mean (fewer than 10^4 terms).
  cumulative values: rtol 1e-15 (integer counts, one fp64 division); cc rtol 1e-12; D_x / V_x / D_cc rtol 1e-12 (the same fp64
      host arithmetic on equal tables).
  dose to volume: 4 fp32 ulp of the larger neighbouring order statistic."""
import functools

import numpy as np
import pytest

from platipy_amd import _lib
from tests import dose_restatement as R

SHAPE = (14, 23, 29)            # [Z][Y][X]
SPACING = (0.9, 1.1, 2.5)       # (x, y, z) mm
N = int(np.prod(SHAPE))
MAX_LABELS, MAX_BINS = 64, 1 << 20
assert (_lib.DOSE_MAX_LABELS, _lib.DOSE_MAX_BINS) == (MAX_LABELS, MAX_BINS)


def ellipsoid(centre, radii):
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in SHAPE], indexing="ij")
    return ((((xx - centre[0]) / radii[0]) ** 2 + ((yy - centre[1]) / radii[1]) ** 2 + ((zz - centre[2]) / radii[2]) ** 2) <= 1)


@functools.lru_cache(maxsize=None)
def dose_array():
    rng = np.random.default_rng(2024)
    d = (rng.integers(0, 1400, SHAPE) * 0.05).astype(np.float32)
    flat = d.reshape(-1)
    where = rng.choice(N, size=24, replace=False)
    flat[where[:6]] = np.float32([-0.35, -1.0, -0.05, -12.5, -0.1, -3.3])                  # below the first edge
    flat[where[6:10]] = np.float32(69.95)                                                     # the maximum (set, not drawn)
    flat[where[10:14]] = np.float32(np.arange(-0.05, 69.95 + 0.1, 0.1)[-1])                   # beside the 0.1 Gy top edge
    flat[where[14:18]] = np.float32(64.0)                                                     # exactly on the top edge of EDGES["exact"]
    flat[where[18:22]] = np.float32(np.arange(-0.05, 50 + 0.1, 0.1)[-1])                      # beside the top edge of max_dose=50
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def mask_arrays():
    """33 masks: 0 and 1 overlap, 2 is empty, 3 is valued 255, 4 is the whole volume, the rest random ellipsoids."""
    rng = np.random.default_rng(7)
    masks = [ellipsoid((12, 10, 6), (8, 6.5, 4.2)).astype(np.uint8), ellipsoid((15, 12, 7), (6, 7, 4)).astype(np.uint8),
             np.zeros(SHAPE, np.uint8), (ellipsoid((20, 8, 8), (5, 5, 3)) * 255).astype(np.uint8), np.ones(SHAPE, np.uint8)]
    while len(masks) < 33:
        c = [rng.uniform(3, s - 3) for s in SHAPE[::-1]]
        r = [rng.uniform(1.5, 0.3 * s) for s in SHAPE[::-1]]
        masks.append(ellipsoid(c, r).astype(np.uint8))
    assert (masks[0] & masks[1]).any() and masks[3].max() == 255
    for m in masks:
        m.setflags(write=False)
    return tuple(masks)


@functools.lru_cache(maxsize=None)
def edge_set(name):
    top = float(dose_array().max())
    return {"w0.1": np.arange(-0.1 / 2, top + 0.1, 0.1),                 # 700 bins: per-workgroup LDS tables
            "w0.001": np.arange(-0.001 / 2, top + 0.001, 0.001),         # ~70 000 bins: one label's bins do not fit LDS
            "max50": np.arange(-0.1 / 2, 50 + 0.1, 0.1),                 # more than a quarter of the voxels above the top edge
            "exact": np.linspace(0.0, 64.0, 129)}[name]                  # every edge a float32; 64.0 voxels sit ON the top edge


@functools.lru_cache(maxsize=None)
def expected_counts(name):
    d, e = dose_array(), edge_set(name)
    return np.stack([R.histogram(d, m, e) for m in mask_arrays()])


def run_histogram(backend, dose, masks, edges):
    dev = [backend.dev(m) for m in masks]
    return backend.ctx.dose_histogram(backend.dev(dose), dev, dose.size, edges)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------
# pp_dose_histogram_f32


@pytest.mark.parametrize("nlabels", [1, 9, 33])
@pytest.mark.parametrize("edges", ["w0.1", "w0.001", "max50", "exact"])
def test_histogram_equals_numpy(backend, edges, nlabels):
    d, masks, e = dose_array(), mask_arrays()[:nlabels], edge_set(edges)
    want = expected_counts(edges)[:nlabels]
    got, stats = run_histogram(backend, d, masks, e)
    assert got.dtype == np.int64 and got.shape == (nlabels, e.size - 1)
    dropped = [int(np.count_nonzero(m)) - int(w.sum()) for m, w in zip(masks, want)]
    print(edges, nlabels, "bins", e.size - 1, "voxels dropped per label", dropped[:5])
    if edges == "w0.001":
        assert e.size - 1 > 12288, "this case is meant to leave the LDS path"
    if edges == "max50" and nlabels > 4:
        assert dropped[4] > N // 4
    if edges == "exact" and nlabels > 4:
        assert want[4][-1] >= 4 and dropped[4] > 0           # the voxels ON the top edge are counted, those above it dropped
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(stats["count"], [np.count_nonzero(m) for m in masks])


def test_histogram_statistics(backend):
    d, masks = dose_array(), mask_arrays()
    _, stats = run_histogram(backend, d, masks, edge_set("w0.1"))
    assert stats.dtype == _lib.DOSE_STATS_DTYPE
    for k, m in enumerate(masks):
        inside = d[m != 0]
        assert stats["count"][k] == inside.size and stats["mask_sum"][k] == int(m.sum(dtype=np.int64))
        if inside.size:
            assert bits(stats["dose_min"][k]) == bits(inside.min()) and bits(stats["dose_max"][k]) == bits(inside.max())
        else:
            assert stats["dose_sum"][k] == 0.0 and stats["dose_min"][k] == np.inf and stats["dose_max"][k] == -np.inf
    assert stats["mask_sum"][3] == 255 * stats["count"][3] and stats["dose_min"][4] < 0
    # the sum on a dose without the negative voxels: the reordering bound of non-negative terms
    pos = np.where(d < 0, np.float32(0.25), d)
    _, stats = run_histogram(backend, pos, masks, edge_set("w0.1"))
    for k, m in enumerate(masks):
        want = pos[m != 0].astype(np.float64).sum()
        err = abs(stats["dose_sum"][k] - want)
        if k < 5:
            print("label", k, "count", stats["count"][k], "sum", stats["dose_sum"][k], "|err|", err, "bound", stats["count"][k] * 2.0 ** -52 * want)
        assert err <= stats["count"][k] * 2.0 ** -52 * want


def test_histogram_dose_sum_is_exact(backend):
    """Terms 2^60 apart, subnormals, signs that cancel and infinities: the limbs hold the exact sum."""
    d = np.zeros(SHAPE, np.float32).reshape(-1)
    d[:8] = np.float32([2.0 ** 100, 1.0, -2.0 ** 100, 2.0 ** -140, 3.5, -1.0, 2.0 ** -149, -0.0])
    d[20:23] = np.float32([np.inf, 1.0, 2.0])
    d[40:42] = np.float32([np.inf, -np.inf])
    d[60:62] = np.float32([np.finfo(np.float32).max, np.finfo(np.float32).max])
    masks = [np.zeros(N, np.uint8) for _ in range(4)]
    masks[0][:8], masks[1][20:23], masks[2][40:42], masks[3][60:62] = 1, 1, 1, 1
    _, stats = run_histogram(backend, d, masks, [0.0, 1.0])
    assert stats["dose_sum"][0] == 3.5 + 2.0 ** -140 + 2.0 ** -149 and stats["dose_sum"][1] == np.inf
    assert np.isnan(stats["dose_sum"][2]) and stats["dose_sum"][3] == 2.0 * float(np.finfo(np.float32).max)
    assert bits(stats["dose_min"][0]) == bits(-2.0 ** 100) and stats["dose_max"][2] == np.inf


def test_histogram_rerun_is_bit_identical(backend):
    d, masks = dose_array(), mask_arrays()
    a, b = run_histogram(backend, d, masks, edge_set("w0.1")), run_histogram(backend, d, masks, edge_set("w0.1"))
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_histogram_masks_off_the_16_byte_grid(backend):
    """Masks that start one byte into an allocation take the byte-wise path: the same counts and statistics."""
    d, masks, e = dose_array(), mask_arrays()[:9], edge_set("w0.1")
    dev_d = backend.dev(d)
    shifted = [backend.dev(np.concatenate([[7], m.reshape(-1)]).astype(np.uint8))[1:] for m in masks]
    assert all(_lib.ptr(s) % 16 == 1 for s in shifted)
    got, stats = backend.ctx.dose_histogram(dev_d, shifted, N, e)
    want, want_stats = backend.ctx.dose_histogram(dev_d, [backend.dev(m) for m in masks], N, e)
    assert np.array_equal(got, expected_counts("w0.1")[:9]) and np.array_equal(got, want)
    assert stats.tobytes() == want_stats.tobytes()


def test_histogram_nan(backend):
    d, masks, e = dose_array().copy(), mask_arrays()[:4], edge_set("w0.1")       # (without the whole-volume mask)
    union = np.zeros(SHAPE, bool)
    for m in masks:
        union |= m != 0
    outside, inside = np.argwhere(~union)[5], np.argwhere(masks[1] != 0)[3]
    d[tuple(outside)] = np.nan
    got, _ = run_histogram(backend, d, masks, e)
    assert np.array_equal(got, expected_counts("w0.1")[:4])
    d[tuple(inside)] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        run_histogram(backend, d, masks, e)


def test_histogram_limits(backend):
    d = dose_array()
    m = mask_arrays()[0]
    dev_d, dev_m = backend.dev(d), backend.dev(m)
    with pytest.raises(ValueError):
        backend.ctx.dose_histogram(dev_d, [dev_m] * (MAX_LABELS + 1), N, [0.0, 1.0])
    got, _ = backend.ctx.dose_histogram(dev_d, [dev_m] * MAX_LABELS, N, [0.0, 35.0, 70.0])
    assert np.array_equal(got, np.tile(R.histogram(d, m, [0.0, 35.0, 70.0]), (MAX_LABELS, 1)))
    with pytest.raises(ValueError):
        backend.ctx.dose_histogram(dev_d, [dev_m], N, np.linspace(0.0, 70.0, MAX_BINS + 2))
    wide = np.linspace(0.0, 70.0, MAX_BINS + 1)
    got, _ = backend.ctx.dose_histogram(dev_d, [dev_m], N, wide)
    assert np.array_equal(got[0], R.histogram(d, m, wide))
    for bad in ([0.0], [1.0, 0.5, 2.0], [0.0, np.nan], []):
        with pytest.raises(ValueError):
            backend.ctx.dose_histogram(dev_d, [dev_m], N, bad)
    with pytest.raises(ValueError):
        backend.ctx.dose_histogram(dev_d, [], N, [0.0, 1.0])


def test_histogram_uneven_edges(backend):
    """Edges the arithmetic guess is far off for (the bisection), a repeated edge and an open top bin."""
    d, masks = dose_array(), mask_arrays()[:9]
    e = np.array([-20.0, -0.05, 0.0, 0.05, 0.05, 1.0, 1.05, 10.0, 33.3, np.float32(33.35), 60.0, 69.0, np.inf])
    got, _ = run_histogram(backend, d, masks, e)
    assert np.array_equal(got, np.stack([R.histogram(d, m, e) for m in masks]))


# --------------------------------------------------------------------------------------
# pp_masked_order_stats_f32


def order_stats(backend, d, m, ranks):
    return backend.ctx.masked_order_stats(backend.dev(d), backend.dev(m), d.size, ranks)


def test_order_statistics(backend):
    d, m = dose_array(), mask_arrays()[0]
    inside = d[m != 0]
    n = inside.size
    assert 700 < n < 1100
    ranks = [0, 1, n // 2, n - 2, n - 1]
    got = order_stats(backend, d, m, ranks)
    assert got.dtype == np.float32
    assert np.array_equal(bits(got), bits(np.partition(inside, ranks)[ranks]))
    # more than eight ranks, unordered and repeated
    many = [n - 1, 5, 5, 17, n // 3, 0, 2 * n // 3, 99, 100, 101, n - 1]
    assert np.array_equal(bits(order_stats(backend, d, m, many)), bits(np.sort(inside)[many]))
    for bad in (n, -1):
        with pytest.raises(ValueError):
            order_stats(backend, d, m, [0, bad])


def test_order_statistics_small_and_constant_masks(backend):
    d = dose_array()
    one, two = np.zeros(SHAPE, np.uint8), np.zeros(SHAPE, np.uint8)
    one[5, 7, 11] = 1
    two[3, 2, 1], two[13, 22, 28] = 1, 255
    assert bits(order_stats(backend, d, one, [0]))[0] == bits(d[5, 7, 11])
    assert np.array_equal(bits(order_stats(backend, d, two, [0, 1])), bits(np.sort(d[two != 0])))
    with pytest.raises(ValueError):
        order_stats(backend, d, one, [1])
    with pytest.raises(ValueError):
        order_stats(backend, d, np.zeros(SHAPE, np.uint8), [0])
    m = mask_arrays()[1]
    flat = np.full(SHAPE, np.float32(17.35))
    n = int(np.count_nonzero(m))
    assert np.array_equal(bits(order_stats(backend, flat, m, [0, n // 2, n - 1])), bits([17.35] * 3))
    nan = d.copy()
    nan[tuple(np.argwhere(m != 0)[9])] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        order_stats(backend, nan, m, [0])
    nan = d.copy()
    nan[tuple(np.argwhere(m == 0)[9])] = np.nan
    assert bits(order_stats(backend, nan, m, [3]))[0] == bits(np.sort(d[m != 0])[3])


def test_order_statistics_signed_values(backend):
    """Negative values, subnormals and -0.0 (no +0.0: numpy does not order the two zeros, the key puts -0.0 first)."""
    rng = np.random.default_rng(99)
    d = rng.normal(0.0, 3.0, SHAPE).astype(np.float32)
    m = mask_arrays()[0]
    idx = np.argwhere(m != 0)
    for k in range(0, 40):
        d[tuple(idx[k])] = np.float32(-0.0)
    d[tuple(idx[40])], d[tuple(idx[41])], d[tuple(idx[42])] = np.float32(-1e-42), np.float32(1e-42), np.float32(-np.inf)
    inside = d[m != 0]
    assert not np.any((inside == 0) & ~np.signbit(inside))
    n = inside.size
    srt = np.sort(inside)
    zero_at = int(np.searchsorted(srt, 0.0))                   # a rank that lands on -0.0
    assert np.signbit(srt[zero_at]) and srt[zero_at] == 0
    ranks = [0, 1, n // 2, n - 2, n - 1, zero_at, zero_at - 1, zero_at + 40]
    assert np.array_equal(bits(order_stats(backend, d, m, ranks)), bits(np.partition(inside, sorted(set(ranks)))[ranks]))


# --------------------------------------------------------------------------------------
# pp_masked_count_ge_f32


def test_count_ge(backend):
    d, masks = dose_array(), mask_arrays()[:9]
    assert np.any(d == np.float32(3.3)) and float(np.float32(3.3)) != 3.3
    thresholds = [3.3, 0, 25.05, float(d.max()), float(d.max()) + 1.0, -5.0, 3.3, 64.0]
    got = backend.ctx.masked_count_ge(backend.dev(d), [backend.dev(m) for m in masks], N, thresholds)
    want = np.array([[(d[m != 0] >= np.float32(t)).sum() for t in thresholds] for m in masks])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # a float32 array against the Python float is the float32 comparison; against the float64 it is not
    assert np.array_equal(want[:, 0], [(d[m != 0] >= 3.3).sum() for m in masks])
    assert want[4, 0] != (d.astype(np.float64) >= 3.3).sum()
    assert np.all(got[:, 4] == 0) and np.all(got[2] == 0)
    with pytest.raises(ValueError):
        backend.ctx.masked_count_ge(backend.dev(d), [backend.dev(masks[0])], N, [1.0, np.nan])


# --------------------------------------------------------------------------------------
# pa.dose


def images(pa, n=9):
    dose = pa.image_from_array(dose_array().copy(), SPACING)
    names = [f"S{k}" for k in range(n)]
    arrays = dict(zip(names, mask_arrays()[:n]))
    return dose, {k: pa.image_from_array(v.copy(), SPACING) for k, v in arrays.items()}, arrays


@pytest.mark.parametrize("kwargs", [{}, {"bin_width": 0.25}, {"max_dose": 50}, {"bin_width": 0.001, "max_dose": 20.0}], ids=str)
def test_dvh_table(host_api, kwargs):
    pa = host_api
    dose, labels, arrays = images(pa)
    table = pa.dose.dvh_table(dose, labels, **kwargs)
    rows = R.dvh_rows(dose_array(), arrays, SPACING, **kwargs)
    assert table.labels == list(arrays) and table.counts.dtype == np.int64
    for i, row in enumerate(rows):
        assert np.array_equal(table.bins, row["bins"])
        np.testing.assert_allclose(pa.dose.dvh.cumulative_values(table.counts[i]), row["values"], rtol=1e-15, atol=0)
        np.testing.assert_allclose(table.cc[i], row["cc"], rtol=1e-12)
        inside = dose_array()[arrays[row["label"]] != 0]
        if inside.size == 0:
            assert np.isnan(table.mean[i]) and np.isnan(table.min[i]) and np.isnan(table.max[i]) and not table.counts[i].any()
            continue
        assert bits(table.min[i]) == bits(inside.min()) and bits(table.max[i]) == bits(inside.max())
        # (negative voxels: the bound is taken on the sum of magnitudes)
        bound = inside.size * 2.0 ** -52 * np.abs(inside.astype(np.float64)).sum() / inside.size
        print(row["label"], "mean", table.mean[i], "- fp64", table.mean[i] - row["mean"], "- fp32", table.mean[i] - row["mean_f32"])
        assert abs(table.mean[i] - row["mean"]) <= bound
        np.testing.assert_allclose(table.mean[i], row["mean_f32"], rtol=2.0 ** -20, atol=0)
    assert table.cc[3] == 255 * np.count_nonzero(arrays["S3"]) * np.prod(SPACING) / 1000


def test_dvh_for_labels_frame(host_api):
    pytest.importorskip("pandas")
    pa = host_api
    dose, labels, arrays = images(pa)
    df = pa.dose.calculate_dvh_for_labels(dose, labels)
    want = R.frame(R.dvh_rows(dose_array(), arrays, SPACING))
    assert list(df.columns[:3]) == ["label", "cc", "mean"] and list(df.columns) == list(want.columns)
    assert all(isinstance(c, float) for c in df.columns[3:]) and list(df.label) == list(arrays)
    np.testing.assert_allclose(df[df.columns[3:]].to_numpy(dtype=float), want[want.columns[3:]].to_numpy(dtype=float), rtol=1e-15, atol=0)
    np.testing.assert_allclose(df.cc.to_numpy(), want.cc.to_numpy(), rtol=1e-12)
    np.testing.assert_allclose(df["mean"].to_numpy(), want["mean"].to_numpy(), rtol=1e-14, equal_nan=True)
    assert np.isnan(df["mean"][2]) and not df[df.columns[3:]].iloc[2].any()
    # a later label of another size
    labels["other"] = pa.image_from_array(np.ones((4, 5, 6), np.uint8), SPACING)
    with pytest.raises(ValueError):
        pa.dose.calculate_dvh_for_labels(dose, labels)


def test_dvh_resamples_the_dose(host_api):
    """A dose grid of another size and spacing than the labels: the restatement fed resample_image's output."""
    from platipy_amd.registration.utils import resample_image

    pa = host_api
    _, labels, arrays = images(pa, 5)
    rng = np.random.default_rng(3)
    coarse = pa.image_from_array((rng.integers(0, 1400, (10, 17, 20)) * 0.05).astype(np.float32), (1.4, 1.6, 3.3), (-1.0, 0.5, 1.0))
    first = labels["S0"]
    on_labels = resample_image(coarse, first, None, pa.sitkLinear, 0.0)
    assert on_labels.same_grid(first) and 0 < np.count_nonzero(on_labels.numpy() == 0) < N     # part of the label grid is outside
    table = pa.dose.dvh_table(coarse, labels)
    rows = R.dvh_rows(on_labels.numpy(), arrays, SPACING)
    for i, row in enumerate(rows):
        assert np.array_equal(table.bins, row["bins"])
        assert np.array_equal(pa.dose.dvh.cumulative_values(table.counts[i]), row["values"])
    centres, values = pa.dose.calculate_dvh(coarse, first, bins=50)
    want_c, want_v = R.dvh(on_labels.numpy(), arrays["S0"], 50)
    assert np.array_equal(centres, want_c) and np.array_equal(values, want_v)
    np.testing.assert_allclose(pa.dose.calculate_d_mean(coarse, first), on_labels.numpy()[arrays["S0"] != 0].astype(np.float64).mean(), rtol=1e-14)


@pytest.mark.parametrize("bins", [1001, 37, "edges", "top"], ids=str)
def test_calculate_dvh(host_api, bins):
    pa = host_api
    dose, labels, arrays = images(pa, 5)
    kwargs = {"bins": {"edges": [0.0, 0.05, 1.0, 10.0, 33.3, 50.0, 60.0], "top": np.linspace(0.0, 64.0, 129)}.get(bins, bins)}
    if bins == 1001:
        kwargs = {}                                # the default
    for name in ("S0", "S2", "S3", "S4"):          # S2 is empty: integer zeros, unnormalised
        centres, values = pa.dose.calculate_dvh(dose, labels[name], **kwargs)
        want_c, want_v = R.dvh(dose_array(), arrays[name], kwargs.get("bins", 1001))
        assert np.array_equal(centres, want_c)
        assert values.dtype == want_v.dtype
        np.testing.assert_allclose(values, want_v, rtol=1e-15, atol=0)
    const = pa.image_from_array(np.full(SHAPE, np.float32(2.5)), SPACING)
    centres, values = pa.dose.calculate_dvh(const, labels["S0"], bins=10)         # min == max: the range is widened by 0.5
    want_c, want_v = R.dvh(np.full(SHAPE, np.float32(2.5)), arrays["S0"], 10)
    assert np.array_equal(centres, want_c) and np.array_equal(values, want_v)


def test_dvh_metrics_from_the_frame(host_api):
    pytest.importorskip("pandas")
    pa = host_api
    dose, labels, arrays = images(pa)
    del labels["S2"]                                  # (D100 of an empty structure has no bin with value 1: IndexError in the reference too)
    df = pa.dose.calculate_dvh_for_labels(dose, labels)
    want_df = R.frame(R.dvh_rows(dose_array(), {k: v for k, v in arrays.items() if k != "S2"}, SPACING))

    def check(got, want):
        assert list(got.label) == list(want)
        for _, row in got.iterrows():
            assert list(row.index[1:]) == list(want[row.label])
            for col, value in want[row.label].items():
                np.testing.assert_allclose(row[col], value, rtol=1e-12, atol=0, err_msg=f"{row.label} {col}")

    check(pa.dose.calculate_d_x(df, 95), R.d_x(want_df, 95))
    check(pa.dose.calculate_d_x(df, 100), R.d_x(want_df, 100))
    check(pa.dose.calculate_d_x(df, [2, 50, 99.5, 100]), R.d_x(want_df, [2, 50, 99.5, 100]))
    got = pa.dose.calculate_v_x(df, [20, 35.5, 0, 70.0])
    assert list(got.columns) == ["label", "V20", "V35.5", "V0", "V70"]
    check(got, R.v_x(want_df, [20, 35.5, 0, 70.0]))
    check(pa.dose.calculate_v_x(df, 40), R.v_x(want_df, 40))
    big = float(df.cc.max()) * 3                       # more cc than any structure holds: clamped to 100 %
    check(pa.dose.calculate_d_cc_x(df, [0.01, 0.1, big]), R.d_cc_x(want_df, [0.01, 0.1, big]))
    one = pa.dose.calculate_d_x(df, 50, label="S1")
    assert list(one.label) == ["S1"] and one["D50"][0] == R.d_x(want_df, 50)["S1"]["D50"]
    df["plan"] = ["a"] * len(df)
    got = pa.dose.calculate_d_cc_x(df, 0.1, index_cols=["plan", "label"])
    assert list(got.columns) == ["plan", "label", "D0.1cc"] and set(got.plan) == {"a"}
    want = R.d_cc_x(want_df, 0.1)
    for _, row in got.iterrows():
        np.testing.assert_allclose(row["D0.1cc"], want[row.label]["D0.1cc"], rtol=1e-12)
    # a structure that receives no dose: D_x is 0
    cold = pa.dose.calculate_dvh_for_labels(pa.image_from_array(np.zeros(SHAPE, np.float32), SPACING), {"S0": labels["S0"]}, max_dose=10)
    assert pa.dose.calculate_d_x(cold, 50)["D50"][0] == 0


def test_metrics(host_api):
    pa = host_api
    dose, labels, arrays = images(pa, 5)
    d = dose_array()
    for name in ("S0", "S1", "S3", "S4"):
        m, lab = arrays[name], labels[name]
        inside = d[m > 0]
        srt = np.sort(inside)
        for volume in (0.5, 2, 37.3, 95, 100, 150):
            got, want = pa.dose.calculate_d_to_volume(dose, lab, volume), R.d_to_volume(d, m, SPACING, volume)
            virtual = (inside.size - 1) * ((100 - min(volume, 100)) / 100)
            upper = srt[min(int(np.floor(virtual)) + 1, inside.size - 1)]
            assert isinstance(got, np.float32) and isinstance(want, np.float32)
            assert abs(float(got) - float(want)) <= 4 * float(np.spacing(np.abs(upper))), (name, volume, got, want)
        for cc in (0.005, 0.1, 1e4):
            got, want = pa.dose.calculate_d_to_volume(dose, lab, cc, volume_in_cc=True), R.d_to_volume(d, m, SPACING, cc, True)
            assert abs(float(got) - float(want)) <= 4 * float(np.spacing(srt[-1])), (name, cc, got, want)
        assert bits(pa.dose.calculate_d_max(dose, lab)) == bits(inside.max())
        mean = pa.dose.calculate_d_mean(dose, lab)
        assert abs(mean - inside.astype(np.float64).mean()) <= 2.0 ** -52 * np.abs(inside.astype(np.float64)).sum()
        np.testing.assert_allclose(mean, inside.mean(), rtol=2.0 ** -20)
        for threshold in (3.3, 0, 25, 69.95, 80.0):
            for relative in (True, False):
                np.testing.assert_allclose(pa.dose.calculate_v_receiving_dose(dose, lab, threshold, relative),
                                           R.v_receiving_dose(d, m, SPACING, threshold, relative), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        pa.dose.calculate_d_to_volume(dose, labels["S2"], 50)
    with pytest.raises(ValueError):
        pa.dose.calculate_d_max(dose, labels["S2"])
    assert np.isnan(pa.dose.calculate_d_mean(dose, labels["S2"]))


def test_metrics_for_labels(host_api):
    pytest.importorskip("pandas")
    pa = host_api
    dose, labels, arrays = images(pa)
    d = dose_array()
    del labels["S2"]
    got = pa.dose.calculate_v_receiving_dose_for_labels(dose, labels, [20, 3.3, 65.0])
    assert list(got.columns) == ["label", "V20", "V3.3", "V65"] and list(got.label) == list(labels)
    for relative in (True, False):
        got = pa.dose.calculate_v_receiving_dose_for_labels(dose, labels, [20, 3.3, 65.0], relative)
        for _, row in got.iterrows():
            for col, t in (("V20", 20), ("V3.3", 3.3), ("V65", 65.0)):
                np.testing.assert_allclose(row[col], R.v_receiving_dose(d, arrays[row.label], SPACING, t, relative), rtol=1e-12, atol=0)
    assert list(pa.dose.calculate_v_receiving_dose_for_labels(dose, labels, 20).columns) == ["label", "V20"]
    got = pa.dose.calculate_d_to_volume_for_labels(dose, labels, [2, 95])
    assert list(got.columns) == ["label", "D2", "D95"]
    for _, row in got.iterrows():
        for col, v in (("D2", 2), ("D95", 95)):
            want = R.d_to_volume(d, arrays[row.label], SPACING, v)
            assert abs(float(row[col]) - float(want)) <= 4 * float(np.spacing(d[arrays[row.label] > 0].max()))
    assert list(pa.dose.calculate_d_to_volume_for_labels(dose, labels, 0.1, volume_in_cc=True).columns) == ["label", "D0.1cc"]


def test_dvh_of_a_warped_dose_and_structure(host_api):
    """Dose and mask warped with the same DisplacementFieldTransform through apply_transform, then the DVH of the pair."""
    from tests.helpers import random_dvf

    pa = host_api
    dose, labels, _ = images(pa, 2)
    tfm = pa.DisplacementFieldTransform(pa.image_from_array(random_dvf(SHAPE, SPACING, seed=11, max_mm=3.0), SPACING, is_vector=True))
    warped_dose = pa.registration.apply_transform(dose, dose, tfm, default_value=0, interpolator=pa.sitkLinear)
    warped = {k: pa.registration.apply_transform(v, dose, tfm, default_value=0, interpolator=pa.sitkNearestNeighbor) for k, v in labels.items()}
    wd, wm = warped_dose.numpy(), {k: v.numpy() for k, v in warped.items()}
    assert wd.dtype == np.float32 and wm["S0"].dtype == np.uint8 and wm["S0"].any() and not np.array_equal(wm["S0"], mask_arrays()[0])
    table = pa.dose.dvh_table(warped_dose, warped)
    for i, row in enumerate(R.dvh_rows(wd, wm, SPACING)):
        assert np.array_equal(table.bins, row["bins"])
        np.testing.assert_allclose(pa.dose.dvh.cumulative_values(table.counts[i]), row["values"], rtol=1e-15, atol=0)
        np.testing.assert_allclose(table.cc[i], row["cc"], rtol=1e-12)
        np.testing.assert_allclose(table.mean[i], row["mean"], rtol=1e-14)
