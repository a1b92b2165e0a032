"""pa.radiomics: the kernels of csrc/pp_radiomics.h against the brute-force restatement (tests/radiomics_restatement.py), and
the drop-in interface of the radiomics service.

Tables.  Discretised levels and the four integer tables are held to the restatement with np.array_equal on every input of
CASES: a 5 x 5 x 1 image with a known answer; noise on 9 x 17 x 33 and on 19 x 21 x 37 (more than one 32 x 8 x 8 tile on
every axis) under random masks, one touching all six faces, one a single voxel; a constant image (Ng = 1); a negative minimum
that is no multiple of binWidth; values exactly on bin edges; Ng on both sides of every LDS threshold of the header (25 | 26:
one GLCM direction group | two; 78 | 79: the run table; 90 | 91: the GLCM; 101 | 102: the 26-neighbour tables) and Ng = 320 on
the global path; 70-voxel constant lines along x, y and the body diagonal (runs across tile seams); a checkerboard mask; a
crop that starts one element into a larger buffer (no 16-byte alignment).  Two calls return the same bits.

Features.  Each side computes a feature as a sum of at most T terms (T = 26 x voxels inside the mask bounds the pairs, the
runs and the voxels of every table) followed by a few operations.  A term takes at most 8 roundings (u = 2^-53) and a sum of
T terms adds at most T u times the sum of the terms' magnitudes, on either side, whatever the order.  The inputs are skewed
(exponential noise) so that no feature is a near-cancellation: the sum of the magnitudes stays within a factor 4 of the value
(third powers about the mean included).  Hence |got - want| <= 2 (T + 8) 4 u |want| =: FEATURE_RTOL(T) |want|, no
measured figure enters.  Imc1, Imc2 and MCC have no direct form on a list of pairs: they are checked only through the
matrix route (range and known special cases).
"""
import ctypes as C
import functools
import logging

import numpy as np
import pytest

from platipy_amd import _lib
from tests import memory_state_cases as M
from tests import radiomics_restatement as RR

U = 2.0 ** -53


def feature_rtol(terms):
    return 2.0 * (terms + 8) * 4.0 * U


# --------------------------------------------------------------------------------------
# inputs


def _noise(shape, seed, scale=60.0):
    return (np.random.default_rng(seed).exponential(scale, size=shape) - 20.0).astype(np.float32)


def _levels_image(shape, ng, seed):
    """Integer values 0 ... ng - 1, each present: binWidth 1 gives exactly ng levels."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, ng, size=shape)
    a.reshape(-1)[rng.permutation(a.size)[:ng]] = np.arange(ng)
    return a.astype(np.float32)


def _line(shape, axis_steps):
    m = np.zeros(shape, np.uint8)
    for k in range(70):
        m[1 + k * axis_steps[0] if axis_steps[0] else 1, 1 + k * axis_steps[1] if axis_steps[1] else 1,
          1 + k * axis_steps[2] if axis_steps[2] else 1] = 1
    return m


@functools.lru_cache(maxsize=None)
def case_input(name):
    """-> (image float32 [z, y, x], mask uint8, binWidth)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "known-5x5":
        img = np.array([[1, 2, 5, 2, 3], [3, 2, 1, 3, 1], [1, 3, 5, 5, 2], [1, 1, 1, 1, 2], [1, 2, 4, 3, 5]], np.float32)[None]
        return img, np.ones(img.shape, np.uint8), 1.0
    if name == "noise-9x17x33":
        return _noise((9, 17, 33), 1), (rng.random((9, 17, 33)) < 0.6).astype(np.uint8), 25.0
    if name == "noise-19x21x37-faces":
        m = (rng.random((19, 21, 37)) < 0.5).astype(np.uint8)
        m[0, 3, 4] = m[18, 5, 6] = m[7, 0, 8] = m[9, 20, 10] = m[11, 12, 0] = m[13, 14, 36] = 1
        return _noise((19, 21, 37), 2), m, 25.0
    if name == "single-voxel":
        m = np.zeros((9, 17, 33), np.uint8)
        m[4, 9, 17] = 1
        return _noise((9, 17, 33), 3), m, 25.0
    if name == "constant":
        return np.full((5, 9, 35), 7.25, np.float32), (rng.random((5, 9, 35)) < 0.7).astype(np.uint8), 25.0
    if name == "negative-minimum":
        img = _noise((6, 11, 34), 4)
        img.reshape(-1)[5] = -37.5
        m = (rng.random(img.shape) < 0.6).astype(np.uint8)
        m.reshape(-1)[5] = 1
        return img, m, 25.0
    if name == "on-edges":
        return (25.0 * rng.integers(-3, 6, size=(6, 11, 34))).astype(np.float32), (rng.random((6, 11, 34)) < 0.8).astype(np.uint8), 25.0
    if name.startswith("ng-"):
        ng = int(name[3:])
        return _levels_image((7, 9, 35), ng, ng), np.ones((7, 9, 35), np.uint8), 1.0
    if name.startswith("line-"):
        shape, steps = {"x": ((3, 3, 72), (0, 0, 1)), "y": ((3, 72, 3), (0, 1, 0)), "diagonal": ((72, 72, 72), (1, 1, 1))}[name[5:]]
        return np.full(shape, 3.0, np.float32), _line(shape, steps), 25.0
    if name == "checkerboard":
        from tests.helpers import checkerboard
        return _noise((9, 10, 35), 6), checkerboard((9, 10, 35)), 25.0
    raise KeyError(name)


NG_CASES = ["ng-25", "ng-26", "ng-78", "ng-79", "ng-90", "ng-91", "ng-101", "ng-102", "ng-320"]
CASES = ["known-5x5", "noise-9x17x33", "noise-19x21x37-faces", "single-voxel", "constant", "negative-minimum", "on-edges"] + NG_CASES + [
    "line-x", "line-y", "line-diagonal", "checkerboard"]


@functools.lru_cache(maxsize=None)
def reference_tables(name):
    img, mask, bw = case_input(name)
    lev, ng = RR.discretise(img, mask, bw)
    n, s = RR.ngtdm(lev, ng)
    return {"levels": lev, "ng": ng, "glcm": RR.glcm_symmetric(lev, ng), "gldm": RR.gldm(lev, ng), "ngtdm_n": n, "ngtdm_s": s,
            "glrlm": RR.glrlm(lev, ng)}


# --------------------------------------------------------------------------------------
# the raw calls, every output taken from the leg (garbage-filled)


def leg_of(be):
    return M.Leg(be, be.ctx, 0xFF, 0xA5, 0xFF)


def _offset_copy(leg, a, offset):
    """`a` on the backend, starting `offset` elements into a larger buffer."""
    flat = np.concatenate([np.zeros(offset, a.dtype), a.reshape(-1), np.zeros(3, a.dtype)])
    buf = leg.dev(flat)
    leg._keep.append(buf)
    return buf[offset:offset + a.size]


def discretise(leg, img, mask, edges, offset=0):
    n = img.size
    lev = leg.empty(2 * (n + 8), np.uint8)
    out = lev[2 * offset:2 * offset + 2 * n]
    e = np.ascontiguousarray(edges, np.float64)
    rc = leg.lib.pp_radiomics_discretise_f32(leg.ctx.h, _lib.ptr(_offset_copy(leg, img, offset)), _lib.ptr(_offset_copy(leg, mask, offset)), n,
                                             M.hptr(e), e.size, _lib.ptr(out))
    leg._keep.append(lev)
    return rc, out


def run_tables(leg, img, mask, bw, offset=0):
    """-> dict of the levels and the four tables (the GLCM symmetric) through the C ABI."""
    e = RR.bin_edges(img[mask != 0], bw)
    rc, lev = discretise(leg, img, mask, e, offset)
    assert rc == 0, leg.ctx.lib.pp_last_error(leg.ctx.h)
    levels = leg.host(lev).view(np.uint16).reshape(img.shape)
    ng = int(np.digitize(float(img[mask != 0].max()), e))
    size = (C.c_int * 3)(*M.size_of(img.shape))
    glcm, gldm = leg.hempty((13, ng, ng), np.int64), leg.hempty((ng, 27), np.int64)
    nn, ns = leg.hempty((ng, 27), np.int64), leg.hempty((ng, 27), np.int64)
    p = lambda a: M.hptr(a, C.c_int64)  # noqa: E731
    assert leg.lib.pp_texture_neighbourhood_u16(leg.ctx.h, _lib.ptr(lev), size, ng, p(glcm), p(gldm), p(nn), p(ns)) == 0
    nr = max(img.shape)
    glrlm = leg.hempty((13, ng, nr), np.int64)
    assert leg.lib.pp_texture_runs_u16(leg.ctx.h, _lib.ptr(lev), size, ng, nr, p(glrlm)) == 0
    return {"levels": levels, "ng": np.array([ng]), "glcm": glcm + glcm.transpose(0, 2, 1), "gldm": gldm, "ngtdm_n": nn, "ngtdm_s": ns,
            "glrlm": glrlm}


def assert_tables(got, want, what):
    assert int(got["ng"][0]) == want["ng"], what
    for k in ("levels", "glcm", "gldm", "ngtdm_n", "ngtdm_s", "glrlm"):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


KNOWN_GLCM_X = [[6, 4, 3, 0, 0], [4, 0, 2, 1, 3], [3, 2, 0, 1, 2], [0, 1, 1, 0, 0], [0, 3, 2, 0, 2]]


def test_known_answer_of_the_restatement():
    """The committed known answer: the symmetric GLCM of the 5 x 5 image along x, by brute force."""
    ref = reference_tables("known-5x5")
    assert ref["ng"] == 5 and RR.DIRECTIONS[0] == (0, 0, 1)
    assert ref["glcm"][0].tolist() == KNOWN_GLCM_X


@pytest.mark.parametrize("name", CASES)
def test_tables_equal_the_restatement(backend, name):
    img, mask, bw = case_input(name)
    got = run_tables(leg_of(backend), img, mask, bw)
    assert_tables(got, reference_tables(name), name)
    if name == "known-5x5":
        assert got["glcm"][0].tolist() == KNOWN_GLCM_X
    if name == "checkerboard":        # no face neighbour is inside the mask: every run along an axis has length 1
        for d in (0, 2, 8):
            assert got["glrlm"][d][:, 1:].sum() == 0 and got["glrlm"][d][:, 0].sum() == int(mask.sum())
    if name.startswith("line-"):
        d = {"line-x": 0, "line-y": 2, "line-diagonal": 12}[name]
        assert got["glrlm"][d][0, 69] == 1 and got["glrlm"][d].sum() == 1


@pytest.mark.parametrize("name", ["noise-9x17x33", "ng-91"])
def test_unaligned_crop_and_rerun(backend, name):
    """The same tables from buffers that start one element into a larger allocation (the image 4 bytes, the mask 1 byte past
    a 16-byte boundary: the scalar path), and the same bits from a second call."""
    img, mask, bw = case_input(name)
    leg = leg_of(backend)
    a = run_tables(leg, img, mask, bw, offset=1)
    assert_tables(a, reference_tables(name), name + " unaligned")
    b = run_tables(leg, img, mask, bw)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# --------------------------------------------------------------------------------------
# moments


@pytest.mark.parametrize("name,offset", [("noise-19x21x37-faces", 0), ("noise-9x17x33", 1), ("single-voxel", 0)])
def test_moments_against_fp64(backend, name, offset):
    """Every sum within (n + 8) u sum|terms| of the exactly rounded sum (math.fsum) of fp64 terms on the fp32 values: n
    additions of either order lose at most n u sum|terms|, a term (up to a fourth power of a rounded difference) at most 8 u of
    itself.  The count is exact, and a second call returns the same bits."""
    import math

    img, mask, _ = case_input(name)
    leg = leg_of(backend)
    v = img[mask != 0].astype(np.float64)
    p10, p90 = np.percentile(v, 10), np.percentile(v, 90)
    for lo, hi, c in ((-np.inf, np.inf, float(v.mean())), (p10, p90, 3.5), (1e9, 2e9, 0.0)):
        sel = v[(v >= lo) & (v <= hi)]
        d = sel - c
        want = [d, np.abs(d), d ** 2, d ** 3, d ** 4, sel ** 2]
        outs = []
        for _ in range(2):
            count, sums = C.c_int64(-1), leg.hempty(6, np.float64)
            rc = leg.lib.pp_masked_moments_f32(leg.ctx.h, _lib.ptr(_offset_copy(leg, img, offset)), _lib.ptr(_offset_copy(leg, mask, offset)),
                                               img.size, lo, hi, c, C.byref(count), M.hptr(sums))
            assert rc == 0 and count.value == sel.size
            outs.append(sums.copy())
        assert outs[0].tobytes() == outs[1].tobytes()
        for k, terms in enumerate(want):
            bound = (sel.size + 8) * U * math.fsum(np.abs(terms).tolist())
            err = abs(outs[0][k] - math.fsum(terms.tolist()))
            print(f"{name} moment {k}: error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (name, k, err, bound)


# --------------------------------------------------------------------------------------
# errors


def test_errors(backend):
    leg = leg_of(backend)
    img, mask, bw = case_input("noise-9x17x33")
    e = RR.bin_edges(img[mask != 0], bw)
    bad = img.copy()
    inside, outside = np.flatnonzero(mask.reshape(-1) != 0)[7], np.flatnonzero(mask.reshape(-1) == 0)[7]
    bad.reshape(-1)[outside] = np.nan
    rc, lev = discretise(leg, bad, mask, e)                       # a NaN outside the mask is never looked at
    assert rc == 0 and np.array_equal(leg.host(lev).view(np.uint16).reshape(img.shape), reference_tables("noise-9x17x33")["levels"])
    for poison in (np.nan, np.inf, float(e[-1])):                 # NaN, infinity, a value not below the last edge
        bad = img.copy()
        bad.reshape(-1)[inside] = poison
        assert discretise(leg, bad, mask, e)[0] == _lib.ERR_ARG
    assert discretise(leg, img, mask, np.arange(0.0, 65537.0))[0] == _lib.ERR_SIZE          # 65536 levels
    assert discretise(leg, img, mask, [0.0, 1.0, 1.0])[0] == _lib.ERR_ARG                    # edges that do not increase
    rc, lev = discretise(leg, img, mask, e)
    assert rc == 0
    size = (C.c_int * 3)(*M.size_of(img.shape))
    one = leg.hempty((13, 4, 4), np.int64)
    p = M.hptr(one, C.c_int64)
    assert leg.lib.pp_texture_neighbourhood_u16(leg.ctx.h, _lib.ptr(lev), size, _lib.TEXTURE_MAX_NG + 1, p, None, None, None) == _lib.ERR_SIZE
    assert leg.lib.pp_texture_runs_u16(leg.ctx.h, _lib.ptr(lev), size, _lib.TEXTURE_MAX_NG + 1, 33, p) == _lib.ERR_SIZE
    assert leg.lib.pp_texture_neighbourhood_u16(leg.ctx.h, _lib.ptr(lev), size, 2, p, None, None, None) == _lib.ERR_ARG     # levels above Ng
    assert leg.lib.pp_texture_runs_u16(leg.ctx.h, _lib.ptr(lev), size, 2, 33, p) == _lib.ERR_ARG
    assert leg.lib.pp_texture_runs_u16(leg.ctx.h, _lib.ptr(lev), size, 4, 32, p) == _lib.ERR_ARG                            # Nr is not the longest axis
    assert leg.lib.pp_texture_neighbourhood_u16(leg.ctx.h, _lib.ptr(lev), size, 4, None, None, None, None) == _lib.ERR_ARG


# --------------------------------------------------------------------------------------
# the public interface


def images(pa, name, spacing=(0.9, 1.1, 2.5), origin=(3.0, -2.0, 5.0)):
    img, mask, bw = case_input(name)
    return pa.image_from_array(img.copy(), spacing, origin), pa.image_from_array(mask.copy(), spacing, origin), bw


def _all_features(pa):
    return {rad: list(names) for rad, names in pa.radiomics.features.FEATURES.items()}


def check_features(got, want, rad, terms, what):
    rtol = feature_rtol(terms)
    for name, w in want.items():
        g = got[(rad, name)]
        if np.isnan(w):
            assert np.isnan(g), (what, rad, name, g)
            continue
        err = abs(g - w)
        print(f"{what} {rad}.{name}: {g!r} want {w!r}, relative error {err / max(abs(w), 1e-300):.2e}, bound {rtol:.2e}")
        assert err <= rtol * abs(w), (what, rad, name, g, w, err / max(abs(w), 1e-300), rtol)


@pytest.mark.parametrize("name", ["noise-19x21x37-faces", "noise-9x17x33", "ng-26"])
def test_features_against_the_direct_restatement(host_api, name):
    pa = host_api
    image, mask, bw = images(pa, name)
    img, m, _ = case_input(name)
    got = pa.radiomics.extract_radiomics(image, {"s": mask}, radiomics=_all_features(pa), pyradiomics_settings={"binWidth": bw})["s"]
    lev, ng = RR.discretise(img, m, bw)
    terms = 26 * int(np.count_nonzero(m))
    check_features(got, RR.firstorder(img, m, bw, 0.9 * 1.1 * 2.5), "firstorder", terms, name)
    check_features(got, {"25Percentile": np.percentile(img[m != 0].astype(np.float64), 25),
                         "75Percentile": np.percentile(img[m != 0].astype(np.float64), 75)}, "custom", terms, name)
    check_features(got, RR.glcm_features(lev, ng), "glcm", terms, name)
    check_features(got, RR.glrlm_features(lev), "glrlm", terms, name)
    check_features(got, RR.gldm_features(lev), "gldm", terms, name)
    check_features(got, RR.ngtdm_features(lev), "ngtdm", terms, name)
    # the matrix route only: ranges
    assert got[("glcm", "Imc1")] <= 0.0 and 0.0 <= got[("glcm", "Imc2")] <= 1.0 and 0.0 <= got[("glcm", "MCC")] <= 1.0 + 1e-9
    assert set(got) == {(rad, f) for rad, names in _all_features(pa).items() for f in names}


def test_special_cases(host_api):
    """Ng = 1 and a single voxel: the documented values of the degenerate branches."""
    pa = host_api
    image, mask, bw = images(pa, "constant")
    got = pa.radiomics.extract_radiomics(image, {"c": mask}, radiomics=_all_features(pa))["c"]
    assert got[("firstorder", "Variance")] == 0.0 and got[("firstorder", "Skewness")] == 0.0 and got[("firstorder", "Kurtosis")] == 0.0
    assert got[("firstorder", "Mean")] == 7.25 and got[("firstorder", "Uniformity")] == 1.0
    assert got[("glcm", "Correlation")] == 1.0 and got[("glcm", "MCC")] == 1.0 and got[("glcm", "Contrast")] == 0.0
    assert got[("ngtdm", "Coarseness")] == 1.0e6 and got[("ngtdm", "Contrast")] == 0.0 and got[("gldm", "GrayLevelVariance")] == 0.0
    image, mask, bw = images(pa, "single-voxel")
    got = pa.radiomics.extract_radiomics(image, {"v": mask}, radiomics=_all_features(pa))["v"]
    assert np.isnan(got[("glcm", "Contrast")])                   # no direction has a pair
    assert got[("glrlm", "RunPercentage")] == 1.0 and got[("gldm", "SmallDependenceEmphasis")] == 1.0
    assert got[("firstorder", "Minimum")] == got[("firstorder", "Maximum")] == got[("firstorder", "Median")]


def test_texture_matrices(host_api):
    pa = host_api
    image, mask, bw = images(pa, "noise-19x21x37-faces")
    ref = reference_tables("noise-19x21x37-faces")
    got = pa.radiomics.texture_matrices(image, mask, bw)
    assert got["ng"] == ref["ng"] and got["directions"] == RR.DIRECTIONS and got["origin_index"] == (0, 0, 0)
    for k in ("levels", "glcm", "gldm", "ngtdm_n", "ngtdm_s", "glrlm"):
        assert np.array_equal(got[k], ref[k]), k
    again = pa.radiomics.texture_matrices(image, mask, bw)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in ("levels", "glcm", "gldm", "ngtdm_n", "ngtdm_s", "glrlm"))
    # a structure whose bounding box starts at an odd x inside a larger image: the tables of the crop
    img, m, _ = case_input("noise-9x17x33")
    big, bigm = np.full((12, 20, 40), -500.0, np.float32), np.zeros((12, 20, 40), np.uint8)
    m = m.copy()
    m[0, 0, 0] = m[8, 16, 32] = 1
    big[2:11, 1:18, 3:36], bigm[2:11, 1:18, 3:36] = img, m
    got = pa.radiomics.texture_matrices(pa.image_from_array(big), pa.image_from_array(bigm), 25.0, classes=("glcm", "glrlm"))
    lev, ng = RR.discretise(img, m, 25.0)
    assert got["origin_index"] == (3, 1, 2) and np.array_equal(got["levels"], lev) and set(got) >= {"glcm", "glrlm"} and "gldm" not in got
    assert np.array_equal(got["glcm"], RR.glcm_symmetric(lev, ng)) and np.array_equal(got["glrlm"], RR.glrlm(lev, ng))
    with pytest.raises(ValueError):
        pa.radiomics.texture_matrices(image, mask, bw, classes=("glszm",))


def test_interface(host_api, caplog):
    pa = host_api
    R = pa.radiomics
    assert R.RADIOMICS_SETTINGS == {"contours": [], "radiomics": {}, "pyradiomics_settings": {
        "binWidth": 25, "resampledPixelSpacing": None, "interpolator": "sitkNearestNeighbor", "verbose": True, "removeOutliers": 10000},
        "resample_to_image": False, "append_histogram": False, "histogram_bins": 256}
    avail = R.available_radiomics()
    assert {k: len(v) for k, v in avail.items()} == {"firstorder": 18, "glcm": 24, "glrlm": 16, "ngtdm": 5, "gldm": 14, "custom": 2}
    image, mask, bw = images(pa, "noise-9x17x33")
    img, m, _ = case_input("noise-9x17x33")
    other = (np.random.default_rng(9).random(img.shape) < 0.3).astype(np.uint8)
    masks = {"a": mask, "b": pa.image_from_array(other, image.GetSpacing(), image.GetOrigin())}
    # the default set: every first-order feature, for every contour
    got = R.extract_radiomics(image, masks)
    assert list(got) == ["a", "b"] and list(got["a"]) == [("firstorder", f) for f in avail["firstorder"]]
    assert got["a"][("firstorder", "Mean")] == pytest.approx(float(img[m != 0].astype(np.float64).mean()), rel=1e-12)
    # the contour filter, unknown names skipped with a warning, an empty class skipped, the caller's column order
    with caplog.at_level(logging.WARNING):
        got = R.extract_radiomics(image, masks, contours=["b"], radiomics={"glcm": ["Contrast", "NoSuchFeature", "Id"], "nonsense": ["x"],
                                                                          "gldm": [], "custom": ["75Percentile"]})
    assert list(got) == ["b"] and list(got["b"]) == [("glcm", "Contrast"), ("glcm", "Id"), ("custom", "75Percentile")]
    assert "Feature not found: NoSuchFeature" in caplog.text and "Radiomic Class not found: nonsense" in caplog.text
    # the table
    frame = R.extract_radiomics(image, masks, radiomics={"firstorder": ["Mean", "Energy"], "ngtdm": ["Busyness"]}, as_frame=True)
    assert list(frame.columns) == [("", "Contour"), ("firstorder", "Mean"), ("firstorder", "Energy"), ("ngtdm", "Busyness")]
    assert list(frame[("", "Contour")]) == ["a", "b"] and frame.shape == (2, 4)
    # the histogram
    counts, edges = R.compute_histogram(image, mask, 16)
    want_c, want_e = np.histogram(img[np.where(m)], bins=16)                         # (of the float32 values: float32 edges)
    assert np.array_equal(counts, want_c) and np.array_equal(edges, want_e) and edges.dtype == want_e.dtype == np.float32
    counts, edges = R.compute_histogram(image, mask, [-10.0, 0.0, 40.0, 1000.0])
    want = np.histogram(img[np.where(m)], bins=[-10.0, 0.0, 40.0, 1000.0])
    assert np.array_equal(counts, want[0]) and np.array_equal(edges, want[1]) and edges.dtype == want[1].dtype
    got = R.extract_radiomics(image, {"a": mask}, radiomics={"firstorder": ["Mean"]}, append_histogram=True, histogram_bins=16)["a"]
    assert list(got)[0] == ("firstorder", "Mean") and [got[("histogram", str(k))] for k in range(16)] == want_c.tolist() and len(got) == 17
    # binWidth is honoured, the ignored settings are accepted
    wide = R.extract_radiomics(image, {"a": mask}, radiomics={"firstorder": ["Entropy"]},
                               pyradiomics_settings={"binWidth": 100, "verbose": False, "removeOutliers": 3, "interpolator": "sitkBSpline"})
    assert wide["a"][("firstorder", "Entropy")] < R.extract_radiomics(image, {"a": mask}, radiomics={"firstorder": ["Entropy"]})["a"][
        ("firstorder", "Entropy")]
    # what is not built
    for kw in (dict(radiomics={"shape": ["Sphericity"]}), dict(radiomics={"glszm": ["ZoneEntropy"]}),
               dict(pyradiomics_settings={"resampledPixelSpacing": [1, 1, 1]})):
        with pytest.raises(NotImplementedError):
            R.extract_radiomics(image, {"a": mask}, **kw)


def test_few_voxel_masks(host_api):
    """Two voxels 10 and 20: [P10, P90] = [11, 19] holds no value, so the robust MAD is the mean of an empty set (NaN) and
    every other feature is the plain one; with 15 between them it is that one value's deviation from itself."""
    pa = host_api
    R = pa.radiomics
    img = np.full((3, 4, 5), -7.0, np.float32)
    m = np.zeros((3, 4, 5), np.uint8)
    img[1, 1, 1], img[1, 2, 3] = 10.0, 20.0
    m[1, 1, 1] = m[1, 2, 3] = 1
    got = R.extract_radiomics(pa.image_from_array(img), {"two": pa.image_from_array(m)})["two"]
    assert len(got) == 18 and np.isnan(got.pop(("firstorder", "RobustMeanAbsoluteDeviation")))
    want = {"Mean": 15.0, "Median": 15.0, "Minimum": 10.0, "Maximum": 20.0, "Range": 10.0, "10Percentile": 11.0, "90Percentile": 19.0,
            "InterquartileRange": 5.0, "MeanAbsoluteDeviation": 5.0, "Variance": 25.0, "Energy": 500.0, "TotalEnergy": 500.0,
            "RootMeanSquared": np.sqrt(250.0), "Skewness": 0.0, "Kurtosis": 1.0, "Entropy": 0.0, "Uniformity": 1.0}
    assert set(got) == {("firstorder", k) for k in want}
    for k, w in want.items():                                    # (small integers: every sum is exact; Entropy holds eps inside its log2)
        assert got[("firstorder", k)] == pytest.approx(w, rel=1e-15, abs=1e-15), k
    # a request that does not need the robust sums does not meet them
    assert R.extract_radiomics(pa.image_from_array(img), {"two": pa.image_from_array(m)}, radiomics={"firstorder": ["Mean"]}) == {
        "two": {("firstorder", "Mean"): 15.0}}
    img[2, 0, 0], m[2, 0, 0] = 15.0, 1
    got = R.extract_radiomics(pa.image_from_array(img), {"three": pa.image_from_array(m)},
                              radiomics={"firstorder": ["RobustMeanAbsoluteDeviation", "MeanAbsoluteDeviation"]})["three"]
    assert got == {("firstorder", "RobustMeanAbsoluteDeviation"): 0.0, ("firstorder", "MeanAbsoluteDeviation"): pytest.approx(10.0 / 3.0, rel=1e-15)}


def test_parts_on_demand_and_empty_classes(host_api):
    """Each part of the first-order input is made only for a feature that reads it: on a range of 4e6 at binWidth 25
    (160001 levels, above the cap of 65535) only Entropy and Uniformity are refused.  A class with an empty feature list
    is skipped, `shape` and `glszm` included."""
    pa = host_api
    R = pa.radiomics
    img = np.linspace(-2.0e6, 2.0e6, 2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5)
    image, mask = pa.image_from_array(img), pa.image_from_array(np.ones(img.shape, np.uint8))
    v = img.astype(np.float64).ravel()
    names = ["Mean", "Median", "Variance", "Range", "RobustMeanAbsoluteDeviation", "90Percentile"]
    got = R.extract_radiomics(image, {"a": mask}, radiomics={"firstorder": names, "custom": ["25Percentile"]})["a"]
    inner = v[(v >= np.percentile(v, 10)) & (v <= np.percentile(v, 90))]
    want = {"Mean": v.mean(), "Median": np.median(v), "Variance": v.var(), "Range": v.max() - v.min(),
            "RobustMeanAbsoluteDeviation": np.abs(inner - inner.mean()).mean(), "90Percentile": np.percentile(v, 90)}
    assert list(got) == [("firstorder", k) for k in names] + [("custom", "25Percentile")]
    for k, w in want.items():                                    # (30 terms in fp64; the symmetric values' mean is 0 up to their rounding)
        assert got[("firstorder", k)] == pytest.approx(w, rel=30 * 2.0 ** -52, abs=30 * 2.0e6 * 2.0 ** -52), k
    for name in ("Entropy", "Uniformity"):
        with pytest.raises(ValueError, match="levels"):
            R.extract_radiomics(image, {"a": mask}, radiomics={"firstorder": [name]})
    got = R.extract_radiomics(image, {"a": mask}, radiomics={"shape": [], "glszm": [], "glcm": [], "firstorder": ["Minimum"]})
    assert got == {"a": {("firstorder", "Minimum"): -2.0e6}}


def test_histogram_is_numpys_on_its_own_edges(host_api):
    """np.histogram of a float32 array makes float32 edges and corrects its bin guess against them: values on those edges and
    one float32 step to either side land where numpy puts them; a constant mask and an empty one take numpy's ranges."""
    pa = host_api
    R = pa.radiomics
    rng = np.random.default_rng(31)
    img = rng.normal(0.0, 60.0, (6, 11, 23)).astype(np.float32)
    m = (rng.random(img.shape) < 0.7).astype(np.uint8)
    inside = np.flatnonzero(m.ravel())
    for bins in (37, 256):
        e = np.histogram_bin_edges(img.ravel()[inside], bins)
        assert e.dtype == np.float32
        near = np.concatenate([e[1:-1], np.nextafter(e[1:-1], np.float32(np.inf)), np.nextafter(e[1:-1], np.float32(-np.inf))])
        a = img.copy().ravel()
        keep = [int(np.argmin(a[inside])), int(np.argmax(a[inside]))]      # the range, and so the edges, stay
        spots = np.setdiff1d(np.arange(inside.size), keep)[:near.size]
        a[inside[spots]] = near[:spots.size]
        a = a.reshape(img.shape)
        counts, edges = R.compute_histogram(pa.image_from_array(a), pa.image_from_array(m), bins)
        want_c, want_e = np.histogram(a[np.where(m)], bins=bins)
        assert np.array_equal(want_e, e) and np.array_equal(edges, want_e) and edges.dtype == np.float32
        assert np.array_equal(counts, want_c), np.flatnonzero(counts != want_c)
    flat = np.full(img.shape, 3.25, np.float32)
    for mask in (m, np.zeros_like(m)):
        counts, edges = R.compute_histogram(pa.image_from_array(flat), pa.image_from_array(mask), 8)
        want_c, want_e = np.histogram(flat[np.where(mask)], bins=8)
        assert np.array_equal(counts, want_c) and np.array_equal(edges, want_e) and edges.dtype == want_e.dtype


def test_interface_errors_and_resampling(host_api):
    pa = host_api
    R = pa.radiomics
    image, mask, bw = images(pa, "noise-9x17x33")
    img, m, _ = case_input("noise-9x17x33")
    with pytest.raises(ValueError, match="empty"):
        R.extract_radiomics(image, {"e": pa.image_from_array(np.zeros_like(m), image.GetSpacing(), image.GetOrigin())})
    for poison in (np.nan, np.inf):
        bad = img.copy()
        bad[m != 0] = np.where(np.arange(int(m.sum())) == 5, poison, bad[m != 0])
        with pytest.raises(ValueError):
            R.extract_radiomics(pa.image_from_array(bad, image.GetSpacing(), image.GetOrigin()), {"a": mask})
    ok = img.copy()
    ok[m == 0] = np.nan                                          # NaN only outside the mask is fine
    got = R.extract_radiomics(pa.image_from_array(ok, image.GetSpacing(), image.GetOrigin()), {"a": mask}, radiomics={"glcm": ["Contrast"]})
    assert got == R.extract_radiomics(image, {"a": mask}, radiomics={"glcm": ["Contrast"]})
    # a mask on another grid: the same voxels at half the spacing along x (every voxel doubled), origin moved to match
    sx, sy, sz = image.GetSpacing()
    fine = pa.image_from_array(np.repeat(m, 2, axis=2), (sx / 2, sy, sz), (image.GetOrigin()[0] - sx / 4, image.GetOrigin()[1], image.GetOrigin()[2]))
    with pytest.raises(ValueError, match="grid"):
        R.extract_radiomics(image, {"a": fine})
    got = R.extract_radiomics(image, {"a": fine}, radiomics={"glrlm": ["RunEntropy"], "firstorder": ["Mean"]}, resample_to_image=True)
    assert got == R.extract_radiomics(image, {"a": mask}, radiomics={"glrlm": ["RunEntropy"], "firstorder": ["Mean"]})
