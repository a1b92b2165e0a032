"""platipy_amd.label.comparison: the reference's recorded SimpleITK answers (tests/golden/comparison_known_answers.json),
the numpy / scipy restatement (tests/comparison_restatement.py) on inputs that are not cubes, auto_crop, edge cases,
determinism, the new C-ABI entry points, and one full-size run on the GPU.

Tolerances: the known answers carry the reference test's own (np.allclose defaults).  Against the restatement, everything
derived from integer counts is EQUAL; distances are held to rtol 2e-6 / atol 2e-5, what the project holds distance_map to
(the fp32 map's sums of squared spacings round differently from scipy's fp64 EDT); the histogram median is a step function
of the distances and is compared, to 1e-6 relative, with the restatement's rule applied to the product's own distance map."""
import json
import os

import numpy as np
import pytest

from tests import comparison_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
KNOWN = json.load(open(os.path.join(HERE, "golden", "comparison_known_answers.json")))
SPACING = (0.9, 1.1, 2.5)
RTOL, ATOL = 2e-6, 2e-5
DISTANCE_KEYS = ("hausdorffDistance", "hausdorffDistance95", "meanSurfaceDistance", "maximumSurfaceDistance", "sigmaSurfaceDistance")


def img(pa, arr, spacing=SPACING, origin=(0.0, 0.0, 0.0)):
    return pa.image_from_array(np.ascontiguousarray(arr), spacing=spacing, origin=origin)


def same(x, y):
    """Equal as floats, nan == nan and inf == inf included."""
    return np.array_equal(np.float64(x), np.float64(y), equal_nan=True)


def close(x, y):
    return bool(np.isclose(x, y, rtol=RTOL, atol=ATOL, equal_nan=True))


def known_boxes():
    shape = tuple(KNOWN["size"])[::-1]
    return shape, tuple(KNOWN["spacing"]), R.box(shape, *KNOWN["box_a"])


def expected_median(pa, a, b, spacing):
    """The histogram rule applied to the distance maps pa.label.distance_map returns."""
    med = []
    for la, lb in ((a, b), (b, a)):
        d = np.abs(pa.label.distance_map(img(pa, la, spacing), signed=True).numpy())
        c = R.contour6(lb)
        med.append(R.histogram_median(d[c], d.min(), d.max()))
    return float(np.mean(med))


def check_surface_metrics(pa, a, b, spacing=SPACING):
    got = pa.label.comparison.compute_surface_metrics(img(pa, a, spacing), img(pa, b, spacing))
    want, _ = R.compute_surface_metrics(a, b, spacing)
    assert set(got) == set(want)
    assert all(type(v) is float for v in got.values())
    print({k: (got[k], want[k]) for k in got})
    assert got["surfaceDSC"] == want["surfaceDSC"]
    for k in DISTANCE_KEYS:
        assert close(got[k], want[k]), (k, got[k], want[k])
    med = expected_median(pa, a, b, spacing)
    assert abs(got["medianSurfaceDistance"] - med) <= 1e-6 * abs(med), (got["medianSurfaceDistance"], med)
    return got


# --------------------------------------------------------------------------------------
# 1. known answers


def test_known_answers_restatement():
    shape, spacing, a = known_boxes()
    for bb, want in zip(KNOWN["boxes_b"], KNOWN["surface_dsc"]):
        got = R.compute_surface_dsc(a, R.box(shape, *bb), spacing)
        assert got == 1.0 if want == 1.0 else np.allclose(got, want), (bb, got, want)
    for case in KNOWN["surface_metrics"]:
        got, _ = R.compute_surface_metrics(a, R.box(shape, *case["box_b"]), spacing)
        for k, want in case.items():
            if k != "box_b":
                assert np.allclose(got[k], want), (k, got[k], want)


def test_known_answers_surface_dsc(host_api):
    pa = host_api
    shape, spacing, a = known_boxes()
    for bb, want in zip(KNOWN["boxes_b"], KNOWN["surface_dsc"]):
        got = pa.label.comparison.compute_surface_dsc(img(pa, a, spacing), img(pa, R.box(shape, *bb), spacing))
        assert type(got) is float
        print(bb, got, want)
        if want == 1.0:
            assert got == 1.0
        else:
            assert np.allclose(got, want), (bb, got, want)


def test_known_answers_surface_metrics(host_api):
    pa = host_api
    shape, spacing, a = known_boxes()
    for case in KNOWN["surface_metrics"]:
        got = pa.label.comparison.compute_surface_metrics(img(pa, a, spacing), img(pa, R.box(shape, *case["box_b"]), spacing))
        print(case["box_b"], got)
        for k, want in case.items():
            if k != "box_b":
                assert np.allclose(got[k], want), (k, got[k], want)
    assert got["surfaceDSC"] != 1.0


# --------------------------------------------------------------------------------------
# 2. against the restatement


def pairs():
    e1 = (R.ellipsoid((11, 29, 37), (5, 14, 18), (3.5, 9, 12)), R.ellipsoid((11, 29, 37), (6, 12, 20), (3, 10, 10)))
    blobs = R.blob_pair((23, 31, 29), seed=7)
    edge = (R.ellipsoid((11, 29, 37), (2, 5, 30), (4, 8, 9)), R.ellipsoid((11, 29, 37), (4, 8, 27), (3, 6, 8)))      # touches z = 0, y = 0, x = 36
    return {"ellipsoids": e1, "blobs": blobs, "boundary": edge}


@pytest.mark.parametrize("name", ["ellipsoids", "blobs", "boundary"])
def test_surface_metrics_against_restatement(host_api, name):
    a, b = pairs()[name]
    assert a.any() and b.any() and (a & b).any() and (a != b).any()
    check_surface_metrics(host_api, a, b)


def test_surface_metrics_against_restatement_96(host_api):
    a = R.ellipsoid((96, 97, 99), (48, 50, 47), (20, 31, 26))
    b = R.ellipsoid((96, 97, 99), (50, 47, 50), (23, 27, 28))
    check_surface_metrics(host_api, a, b)


@pytest.mark.parametrize("name", ["ellipsoids", "blobs", "boundary"])
def test_integer_metrics_against_restatement(host_api, name):
    pa = host_api
    C = pa.label.comparison
    a, b = pairs()[name]
    ia, ib = img(pa, a), img(pa, b)
    got, want = C.compute_volume_metrics(ia, ib), R.compute_volume_metrics(a, b, SPACING)
    assert list(got) == ["DSC", "volumeOverlap", "fractionOverlap", "truePositiveFraction", "trueNegativeFraction",
                         "falsePositiveFraction", "falseNegativeFraction"]
    for k in want:
        assert type(got[k]) is float and same(got[k], want[k]), (k, got[k], want[k])
    assert C.compute_volume(ia) == R.compute_volume(a, SPACING)
    for tau in (3.0, 1.0, 0.0, 4.7):
        assert C.compute_surface_dsc(ia, ib, tau=tau) == R.compute_surface_dsc(a, b, SPACING, tau=tau), tau
    for thr in (3, 0, 1.5, 7):
        got_apl, want_apl = C.compute_apl(ia, ib, distance_threshold_mm=thr), R.compute_apl(a, b, SPACING, thr)
        assert isinstance(got_apl, list) and got_apl == want_apl, (thr, got_apl, want_apl)
        assert C.compute_metric_total_apl(ia, ib, thr) == float(np.sum(want_apl) * np.mean(SPACING[:2]))
        assert C.compute_metric_mean_apl(ia, ib, thr) == float(np.mean(want_apl) * np.mean(SPACING[:2]))


@pytest.mark.parametrize("dtype", [np.uint8, bool, np.float32])
def test_label_dtypes(host_api, dtype):
    pa = host_api
    C = pa.label.comparison
    a, b = pairs()["ellipsoids"]
    scale = 0.25 if dtype is np.float32 else 1          # non-zero = foreground, whatever the value
    ia, ib = img(pa, (a * scale).astype(dtype)), img(pa, (b * 3 * scale).astype(dtype))
    want = R.compute_volume_metrics(a, b, SPACING)
    got = C.compute_volume_metrics(ia, ib)
    assert all(same(got[k], want[k]) for k in want)
    assert C.compute_surface_dsc(ia, ib) == R.compute_surface_dsc(a, b, SPACING)
    assert C.compute_apl(ia, ib) == R.compute_apl(a, b, SPACING)
    assert close(C.compute_metric_hd(ia, ib, auto_crop=False), R.hausdorff(a, b, SPACING))


# --------------------------------------------------------------------------------------
# 3. auto_crop


@pytest.mark.parametrize("name", ["ellipsoids", "blobs", "boundary"])
def test_auto_crop_against_cropped_restatement(host_api, name):
    pa = host_api
    C = pa.label.comparison
    a, b = pairs()[name]
    ca, cb = R.crop_to_union(a, b)
    ia, ib = img(pa, a), img(pa, b)
    vc, vf = R.compute_volume_metrics(ca, cb, SPACING), R.compute_volume_metrics(a, b, SPACING)
    assert same(C.compute_metric_dsc(ia, ib), vc["DSC"]) and same(C.compute_metric_dsc(ia, ib, auto_crop=False), vf["DSC"])
    assert same(C.compute_metric_sensitivity(ia, ib), vc["truePositiveFraction"])
    assert same(C.compute_metric_specificity(ia, ib), vc["trueNegativeFraction"])
    assert same(C.compute_metric_specificity(ia, ib, auto_crop=False), vf["trueNegativeFraction"])
    for crop, (xa, xb) in ((True, (ca, cb)), (False, (a, b))):
        hd, masd = C.compute_metric_hd(ia, ib, auto_crop=crop), C.compute_metric_masd(ia, ib, auto_crop=crop)
        print(crop, hd, R.hausdorff(xa, xb, SPACING), masd, R.compute_metric_masd(xa, xb, SPACING))
        assert type(hd) is float and type(masd) is float
        assert close(hd, R.hausdorff(xa, xb, SPACING))
        assert close(masd, R.compute_metric_masd(xa, xb, SPACING))


def test_auto_crop_changes_specificity_and_masd(host_api):
    pa = host_api
    C = pa.label.comparison
    # two small overlapping boxes in a large empty volume: most true negatives lie outside the union's bounding box
    a, b = np.zeros((20, 24, 28), np.uint8), np.zeros((20, 24, 28), np.uint8)
    a[5:12, 6:14, 7:15] = 1
    b[7:14, 8:16, 9:17] = 1
    ia, ib = img(pa, a), img(pa, b)
    s_crop, s_full = C.compute_metric_specificity(ia, ib), C.compute_metric_specificity(ia, ib, auto_crop=False)
    ca, cb = R.crop_to_union(a, b)
    assert same(s_crop, R.compute_volume_metrics(ca, cb, SPACING)["trueNegativeFraction"])
    assert same(s_full, R.compute_volume_metrics(a, b, SPACING)["trueNegativeFraction"])
    assert s_crop < s_full
    # the crop puts a's face on the box boundary, where its voxels stop being border voxels: the restatement on the really
    # cropped arrays says what MASD must then be, and it is not the uncropped value
    m_crop, m_full = R.compute_metric_masd(ca, cb, SPACING), R.compute_metric_masd(a, b, SPACING)
    assert abs(m_crop - m_full) > 1e-3
    assert close(C.compute_metric_masd(ia, ib), m_crop) and close(C.compute_metric_masd(ia, ib, auto_crop=False), m_full)


# --------------------------------------------------------------------------------------
# 4. edges


def test_empty_label(host_api):
    pa = host_api
    C = pa.label.comparison
    a, _ = pairs()["ellipsoids"]
    z = np.zeros_like(a)
    ia, iz = img(pa, a), img(pa, z)
    for x, y in ((ia, iz), (iz, ia)):
        for crop in (True, False):
            assert np.isnan(C.compute_metric_masd(x, y, auto_crop=crop))
            assert np.isnan(C.compute_metric_hd(x, y, auto_crop=crop))
    got, want = C.compute_volume_metrics(ia, iz), R.compute_volume_metrics(a, z, SPACING)
    assert all(same(got[k], want[k]) for k in want)
    assert got["DSC"] == 0.0 and got["truePositiveFraction"] == 0.0
    got = C.compute_volume_metrics(iz, ia)
    assert np.isnan(got["truePositiveFraction"]) and np.isnan(got["falseNegativeFraction"])       # 0 / 0
    got = C.compute_volume_metrics(iz, iz)
    assert np.isnan(got["DSC"]) and np.isnan(got["fractionOverlap"]) and got["trueNegativeFraction"] == 1.0
    got, want = C.compute_volume_metrics(img(pa, np.ones_like(a)), iz), R.compute_volume_metrics(np.ones_like(a), z, SPACING)
    assert all(same(got[k], want[k]) for k in want) and np.isnan(got["trueNegativeFraction"])      # no negatives at all: 0 / 0
    sm = C.compute_surface_metrics(ia, iz)
    assert all(np.isnan(sm[k]) for k in DISTANCE_KEYS + ("medianSurfaceDistance",))
    assert sm["surfaceDSC"] == 0.0
    assert C.compute_volume(iz) == 0.0
    assert C.compute_apl(iz, iz) == [] and np.isnan(C.compute_metric_mean_apl(iz, iz)) and C.compute_metric_total_apl(iz, iz) == 0.0


def test_identical_labels(host_api):
    pa = host_api
    C = pa.label.comparison
    a, _ = pairs()["blobs"]
    ia, ib = img(pa, a), img(pa, a.copy())
    assert C.compute_metric_dsc(ia, ib) == 1.0 and C.compute_metric_hd(ia, ib) == 0.0 and C.compute_metric_masd(ia, ib) == 0.0
    assert C.compute_surface_dsc(ia, ib) == 1.0
    apl = C.compute_apl(ia, ib)
    assert len(apl) == int((a.sum(axis=(1, 2)) > 0).sum()) and all(v == 0 for v in apl)
    sm = C.compute_surface_metrics(ia, ib)
    assert sm["hausdorffDistance"] == 0.0 and sm["meanSurfaceDistance"] == 0.0 and sm["sigmaSurfaceDistance"] == 0.0
    assert sm["surfaceDSC"] == 1.0


def test_disjoint_labels(host_api):
    pa = host_api
    C = pa.label.comparison
    a = R.ellipsoid((11, 29, 37), (5, 8, 8), (3, 5, 6))
    b = R.ellipsoid((11, 29, 37), (5, 20, 28), (4, 6, 7))
    assert not (a & b).any()
    assert C.compute_metric_dsc(img(pa, a), img(pa, b)) == 0.0
    check_surface_metrics(pa, a, b)
    assert C.compute_apl(img(pa, a), img(pa, b)) == R.compute_apl(a, b, SPACING)


def test_single_voxel_labels(host_api):
    """A one-voxel label has a one-voxel contour: the sample standard deviation is (v^2 - v^2 / 1) / 0 = 0 / 0 = nan in fp64
    (v^2 of an fp32 value is exact), so sigmaSurfaceDistance is nan -- what the restatement's arithmetic gives."""
    pa = host_api
    C = pa.label.comparison
    a, b = np.zeros((9, 11, 13), np.uint8), np.zeros((9, 11, 13), np.uint8)
    a[4, 5, 6] = 1
    b[6, 2, 9] = 1
    got = C.compute_surface_metrics(img(pa, a), img(pa, b))
    want, n = R.compute_surface_metrics(a, b, SPACING)
    assert n == [1, 1] and np.isnan(want["sigmaSurfaceDistance"]) and np.isnan(got["sigmaSurfaceDistance"])
    dist = float(np.float32(np.sqrt(np.float32((3 * 0.9) ** 2 + (3 * 1.1) ** 2 + (2 * 2.5) ** 2))))
    for k in ("hausdorffDistance", "meanSurfaceDistance", "maximumSurfaceDistance"):
        assert close(got[k], want[k]) and close(got[k], dist), (k, got[k], want[k], dist)
    assert got["surfaceDSC"] == want["surfaceDSC"] == 0.0
    assert close(C.compute_metric_masd(img(pa, a), img(pa, b)), dist)


def test_argument_errors(host_api):
    pa = host_api
    C = pa.label.comparison
    a, b = pairs()["ellipsoids"]
    ia = img(pa, a)
    for other in (img(pa, b, spacing=(1.0, 1.1, 2.5)), img(pa, b, origin=(1.0, 0.0, 0.0)), img(pa, b[:, :, :-1])):
        for fn in (C.compute_volume_metrics, C.compute_surface_metrics, C.compute_surface_dsc, C.compute_metric_dsc, C.compute_metric_hd,
                   C.compute_metric_masd, C.compute_apl):
            with pytest.raises(ValueError):
                fn(ia, other)
    # 16 voxels in plane: above the dilation kernel's radius limit of 15
    with pytest.raises(ValueError, match="15"):
        C.compute_apl(ia, img(pa, b), distance_threshold_mm=15.5)
    assert C.compute_apl(ia, img(pa, b), distance_threshold_mm=15.0) == R.compute_apl(a, b, SPACING, 15.0)
    with pytest.raises(ValueError):
        C.compute_metrics({"s": ia}, {"s": img(pa, b)}, metrics=["DSC", "nonsense"])


def test_apl_slice_with_one_label(host_api):
    pa = host_api
    C = pa.label.comparison
    a, b = np.zeros((8, 20, 22), np.uint8), np.zeros((8, 20, 22), np.uint8)
    a[1:5, 4:15, 5:16] = 1          # slices 1..4
    b[3:7, 5:14, 4:18] = 1          # slices 3..6: 1, 2 hold the reference only, 5, 6 the test only, 0 and 7 nothing
    for thr in (3, 0):
        got, want = C.compute_apl(img(pa, a), img(pa, b), thr), R.compute_apl(a, b, SPACING, thr)
        assert got == want and len(got) == 6
        assert got[0] == got[1] == int(R.contour4_slices(a)[1].sum()) and got[4] == got[5] == 0


# --------------------------------------------------------------------------------------
# 5. determinism, compute_metrics


def bits(d):
    return {k: np.float64(v).tobytes() for k, v in d.items()}


def test_reruns_are_bit_identical(host_api):
    pa = host_api
    C = pa.label.comparison
    a, b = pairs()["blobs"]
    ia, ib = img(pa, a), img(pa, b)
    first = (bits(C.compute_surface_metrics(ia, ib)), bits(C.compute_volume_metrics(ia, ib)),
             np.float64(C.compute_metric_masd(ia, ib)).tobytes(), np.float64(C.compute_metric_hd(ia, ib)).tobytes(), C.compute_apl(ia, ib))
    C.compute_surface_metrics(ib, ia)       # other work on the same context in between
    again = (bits(C.compute_surface_metrics(ia, ib)), bits(C.compute_volume_metrics(ia, ib)),
             np.float64(C.compute_metric_masd(ia, ib)).tobytes(), np.float64(C.compute_metric_hd(ia, ib)).tobytes(), C.compute_apl(ia, ib))
    assert first == again


def test_compute_metrics_equals_the_single_calls(host_api):
    pa = host_api
    C = pa.label.comparison
    p = pairs()
    ref = {k: img(pa, v[0]) for k, v in p.items()}
    tst = {k: img(pa, v[1]) for k, v in p.items() if k != "boundary"}
    tst["extra"] = tst["blobs"]
    got = C.compute_metrics(ref, tst)
    assert list(got) == ["ellipsoids", "blobs"]
    for k in got:
        want = dict(C.compute_volume_metrics(ref[k], tst[k]))
        want.update(C.compute_surface_metrics(ref[k], tst[k]))
        assert list(got[k]) == list(C.VOLUME_KEYS + C.SURFACE_KEYS)
        assert bits(got[k]) == bits(want)
    few = C.compute_metrics(ref, tst, metrics=["DSC", "totalAPL", "meanAPL", "hausdorffDistance"])
    for k in few:
        assert few[k] == {"DSC": C.compute_metric_dsc(ref[k], tst[k], auto_crop=False), "totalAPL": C.compute_metric_total_apl(ref[k], tst[k]),
                          "meanAPL": C.compute_metric_mean_apl(ref[k], tst[k]),
                          "hausdorffDistance": C.compute_surface_metrics(ref[k], tst[k])["hausdorffDistance"]}


# --------------------------------------------------------------------------------------
# 6. the C ABI


def abi_volume(seed=3, shape=(7, 13, 19)):
    """A label, a signed "distance map" of random values, and the volume's size: 1729 voxels, a multiple of nothing."""
    rng = np.random.default_rng(seed)
    sel = (R.blob_pair(shape, seed, sigma=1.5)[0] * rng.integers(1, 255, size=shape)).astype(np.uint8)
    dist = rng.normal(scale=4.0, size=shape).astype(np.float32)
    return sel, dist, (shape[2], shape[1], shape[0])


@pytest.mark.parametrize("misalign", [0, 1])
def test_abi_surface_stats(backend, misalign):
    from platipy_amd import _lib

    be = backend
    sel, dist, size = abi_volume()
    n = sel.size
    assert n % 16 != 0 and sel.any()
    geom = _lib.make_geom(size, SPACING)
    dsel_all = be.dev(np.concatenate([np.zeros(misalign, np.uint8), sel.ravel()]))     # misalign = 1: the byte path
    dsel = dsel_all[misalign:]
    ddist = be.dev(dist)
    rng = be.empty((2,), np.float32)
    be.ctx.abs_range(ddist, n, rng)
    lo, hi = be.host(rng)
    assert lo == np.abs(dist).min() and hi == np.abs(dist).max()
    out = be.empty((_lib.SURFACE_STATS_DTYPE.itemsize,), np.uint8)
    tau = 1.25
    samples = {
        _lib.SURFACE_CONTOUR_ABS: np.abs(dist)[R.contour6(sel)],
        _lib.SURFACE_LABEL_POS: np.maximum(dist, 0)[sel != 0],
        _lib.SURFACE_NONZERO: dist[sel != 0],
    }
    for mode, v in samples.items():
        for use_range in (True, False):
            be.ctx.surface_stats(dsel, ddist, geom, mode, out, tau=tau, device_range=rng if use_range else None)
            rec = be.host(out).view(_lib.SURFACE_STATS_DTYPE)[0]
            v64 = v.astype(np.float64)
            assert rec["count"] == v.size > 0
            assert rec["count_le_tau"] == int((v64 <= tau).sum())
            assert rec["min"] == v.min() and rec["max"] == v.max()
            assert np.isclose(rec["sum"], v64.sum(), rtol=1e-12, atol=1e-12) and np.isclose(rec["sum_sq"], (v64 * v64).sum(), rtol=1e-12)
            if use_range:
                assert rec["range_lo"] == lo and rec["range_hi"] == hi
                x = (v64 - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * 128.0
                want = np.bincount(np.where(x >= 127, 127, np.maximum(x, 0).astype(np.int64)), minlength=128)
                assert rec["hist"].sum() == rec["count"] and np.array_equal(rec["hist"], want)
            else:
                assert rec["hist"].sum() == 0 and rec["range_lo"] == 0.0 and rec["range_hi"] == 0.0
    # an empty selection
    be.ctx.surface_stats(be.dev(np.zeros_like(sel)), ddist, geom, _lib.SURFACE_CONTOUR_ABS, out, device_range=rng)
    rec = be.host(out).view(_lib.SURFACE_STATS_DTYPE)[0]
    assert rec["count"] == 0 and rec["sum"] == 0.0 and rec["hist"].sum() == 0


@pytest.mark.parametrize("misalign", [0, 1])
def test_abi_counts_and_contours(backend, misalign):
    be = backend
    a, _, size = abi_volume(seed=5)
    b, _, _ = abi_volume(seed=6)
    n = a.size
    da = be.dev(np.concatenate([np.zeros(misalign, np.uint8), a.ravel()]))[misalign:]
    db = be.dev(np.concatenate([np.zeros(misalign, np.uint8), b.ravel()]))[misalign:]
    assert be.ctx.overlap_counts(da, db, n) == (int((a != 0).sum()), int((b != 0).sum()), int(((a != 0) & (b != 0)).sum()))
    out = be.empty((n,), np.uint8)
    be.ctx.binary_contour(da, size, out, fully_connected=True)
    assert np.array_equal(be.host(out).reshape(a.shape) != 0, R.border26(a))
    be.ctx.binary_contour(da, size, out, fully_connected=False)
    assert np.array_equal(be.host(out).reshape(a.shape) != 0, R.contour6(a))
    be.ctx.slice_contour(da, size, out)
    assert np.array_equal(be.host(out).reshape(a.shape) != 0, R.contour4_slices(a))
    per = be.empty((8 * size[2],), np.uint8)
    be.ctx.slice_masked_count(da, db, size, per)
    assert np.array_equal(be.host(per).view(np.int64), ((a != 0) & (b == 0)).sum(axis=(1, 2)))
    be.ctx.slice_masked_count(da, None, size, per)
    assert np.array_equal(be.host(per).view(np.int64), (a != 0).sum(axis=(1, 2)))


def test_abi_slice_count_word_path(backend):
    """Slices of a multiple of 4 voxels take the 4-byte loads; many chunks per slice."""
    be = backend
    rng = np.random.default_rng(11)
    a = (rng.random((3, 52, 60)) < 0.3).astype(np.uint8) * 7
    b = (rng.random((3, 52, 60)) < 0.5).astype(np.uint8)
    per = be.empty((8 * 3,), np.uint8)
    be.ctx.slice_masked_count(be.dev(a), be.dev(b), (60, 52, 3), per)
    assert np.array_equal(be.host(per).view(np.int64), ((a != 0) & (b == 0)).sum(axis=(1, 2)))


# --------------------------------------------------------------------------------------
# 7. full size, on the card


@pytest.mark.gpu
def test_full_size_512x512x256(gpu_backend):
    import platipy_amd as pa

    C = pa.label.comparison
    shape, sub, at = (256, 512, 512), (80, 150, 170), (90, 180, 160)
    ea = R.ellipsoid(sub, (38, 74, 84), (30, 60, 70))
    eb = R.ellipsoid(sub, (41, 79, 80), (30, 60, 70))
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    sl = tuple(slice(o, o + s) for o, s in zip(at, sub))
    a[sl], b[sl] = ea, eb
    ia, ib = img(pa, a), img(pa, b)
    # integer results against numpy on the whole volume
    fa, fb = a != 0, b != 0
    na, nb, nab, n = int(fa.sum()), int(fb.sum()), int((fa & fb).sum()), a.size
    vm = C.compute_volume_metrics(ia, ib)
    assert vm["DSC"] == 2.0 * nab / (na + nb)
    assert vm["fractionOverlap"] == nab / (na + nb - nab)
    assert vm["trueNegativeFraction"] == (n - (na + nb - nab)) / (n - (na + nb - nab) + nb - nab)
    assert vm["truePositiveFraction"] == nab / na
    assert C.compute_volume(ia) == float(na * np.prod(SPACING) / 1000)
    # the ellipsoids sit well inside `sub`: every border voxel and every sample lies in it, so distances, surface DSC and
    # the added path length of the whole volume equal the restatement's on the box (the histogram's range does not: the
    # median is left to the smaller cases)
    got = C.compute_surface_metrics(ia, ib)
    want, _ = R.compute_surface_metrics(ea, eb, SPACING)
    print({k: (got[k], want[k]) for k in got})
    assert got["surfaceDSC"] == want["surfaceDSC"]
    for k in DISTANCE_KEYS:
        assert close(got[k], want[k]), (k, got[k], want[k])
    assert close(C.compute_metric_masd(ia, ib, auto_crop=False), R.compute_metric_masd(ea, eb, SPACING))
    assert close(C.compute_metric_hd(ia, ib, auto_crop=False), R.hausdorff(ea, eb, SPACING))
    ca, cb = R.crop_to_union(ea, eb)
    assert close(C.compute_metric_masd(ia, ib), R.compute_metric_masd(ca, cb, SPACING))
    assert close(C.compute_metric_hd(ia, ib), R.hausdorff(ca, cb, SPACING))
    assert C.compute_apl(ia, ib) == R.compute_apl(ea, eb, SPACING)
