"""The linear-registration metric kernels (pp_fusion.hip: k_metric_grad, k_metric_values_lanes, k_mi_histogram,
k_mi_gradient + k_sum14_final, k_fixed_samples) against the fp64 restatement of
tests/linear_metric_restatement.py, on every path of their dispatch ("Linear metric, which lattice enters
which kernel").  tests/test_linear.py ties them to a reference at one lattice of 158 samples -- one block, one ticket group,
one fold trip; here every case is the smallest lattice that reaches another path.

The dispatch forest (NT = 256 threads a block, n = samples of the lattice):
  value + gradient   k_metric_grad<MODE, GI>, min(ceil(n / 256), 512) blocks, a thread holds
                     G = 4 samples in flight (2 for correlation and for the packed gradient image), so a second grid-stride
                     trip starts above 512 * 256 * G samples; two-level ticket (block b counts in group b % 8, the last of a group
                     on the top counter); the last block folds floor(256 / NACC) * 16 rows a trip (288 mean squares, 96
                     correlation); 64-bit lattice arithmetic from 2^31 virtual voxels.
  value probes       k_metric_values_lanes, 16 sample slots a block, spt = samples per thread
                     (a multiple of 4) so that at most 128 blocks (n < 20000) or 1024 blocks run; folds 128 (mean squares) /
                     32 (correlation) rows a trip; walk<FAST, MASKED>: FAST with the level's fixed-sample cache and 32-bit
                     offsets (moving nx >= 2), else the plain form.
  mutual information k_mi_histogram, k_mi_gradient + k_sum14_final: at most 512 blocks, one sample a thread and trip.
  fixed-sample cache k_fixed_samples, inside pp_linear_optimize_f32 only.

Bounds.  Counts are exact.  Every sum is held to the `bound` the restatement returns next to it, derived there from
per-sample bounds and never tuned: the kernels interpolate in fp32 (three nested levels of a + (b - a) w, four roundings a level:
e <= (1 - w) ea + w eb + 2^-24 (3 |b - a| w + |result|), walked over the kernel's own expression tree for the value, each
gradient component and the gradient image) and do everything else in fp64 (n 2^-53 of the absolute sum).  The bound is a
worst case -- all errors aligned -- so the measured error sits one to two orders below it; one dropped or doubled sample
among the thousands of a case moves a sum by ~1 / count, three orders above the bound.  Mattes histogram: |B'| em / m_bin +
2^-33 per weight; joint histogram: exact, except that a sample whose bin coordinate lies within its own error of a bin edge may
sit in the neighbouring bin (the restatement lists those; none in the small cases); MI gradient: |B''| em / m_bin |table| plus the
fp32 rounding of the table.  Cross-kernel agreements (candidate 0 against the gradient-bearing call, packed against planar):
the same per-sample terms added in another order, 1e-12 of the largest sum of the call.

Inputs.  Images are 100 * standard_normal fp32: rough, every corner matters.  A generic case has non-round coefficients and
asserts margin >= 1e-9 before it calls a kernel: two correct fp64 evaluation orders of c = A v + b (with or without fused
multiply-add) differ by ~1e-13 at |c| < 100, so no decision -- inside, cell, mask voxel -- can differ between the two sides.
A dyadic case (coefficients multiples of 2^-10) is exact under any order: ties are part of the test.

The measured maxima go to record_stats("linear_metric"), absolute and as a fraction of the bound.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from platipy_amd import _lib
from tests import linear_metric_restatement as LR
from tests.helpers import record_stats

_STATS = {}
MARGIN = 1e-9
# a fixed matrix of non-round digits with a dominant diagonal
R = np.array([[1.03917, 0.04713, -0.02189], [-0.03571, 0.97243, 0.05127], [0.01873, -0.04419, 1.01631]])


def _fit(size, vsize, lo, hi):
    """Diagonal map of lattice index 0 .. v - 1 onto [-0.5 - lo, n - 0.5 + hi] per axis (lo, hi: non-round overhang in voxels)."""
    size, vsize = np.asarray(size, dtype=np.float64), np.asarray(vsize, dtype=np.float64)
    return np.diag((size + lo + hi) / np.maximum(vsize - 1.0, 1.0)), -0.5 - np.asarray(lo, dtype=np.float64) * np.ones(3)


def _generic(fshape, mshape, vsize, stride, seed, flo=0.83719, fhi=(0.91357, 0.87431, -0.73129), mlo=0.77431, mhi=(0.68823, 0.79153, -0.81347)):
    """A generic case: the lattice overhangs both images on every side but the upper z side, where it ends inside them -- the
    LAST samples of the raster walk (the ragged tail of the last block, the rows of the second fold trip) are accepted ones."""
    fhi, mhi = np.asarray(fhi), np.asarray(mhi)
    Af, bf = _fit(fshape[::-1], vsize, flo, fhi)
    Sm, bm = _fit(mshape[::-1], vsize, mlo, mhi)
    return dict(fshape=fshape, mshape=mshape, vsize=vsize, stride=stride, Af=Af, bf=bf, Am=R @ Sm, bm=bm + np.array([0.31337, -0.27183, 0.16180]),
                seed=seed, exact=())


FS, MS = (10, 12, 14), (11, 12, 13)


def _cases():
    c = {}
    I = np.eye(3)
    c["band"] = dict(fshape=(6, 7, 9), mshape=(5, 8, 7), vsize=(21, 17, 15), stride=1, Af=0.5 * I, bf=np.full(3, -0.5), Am=0.47 * I + 1e-3 * R,
                     bm=np.array([-0.5 + 1.0371e-4, -0.5 + 1.2943e-4, -0.5 + 0.8317e-4]), seed=1, exact=("f",))
    c["ties"] = dict(fshape=FS, mshape=MS, vsize=(30, 26, 22), stride=1, Af=0.5 * I, bf=np.full(3, -0.5), Am=0.25 * I, bm=np.full(3, -0.5),
                     seed=2, exact=("f", "m"))
    nx1 = _generic((6, 7, 9), (5, 8, 1), (19, 16, 13), 1, 3)
    nx1["Am"][0, :] = 0.0
    nx1["bm"][0] = 0.13173
    c["nx1"] = nx1
    flat = _generic((1, 1, 9), (1, 1, 7), (19, 1, 1), 1, 4)
    flat["bf"][1:], flat["bm"][1:] = [0.12347, -0.21731], [0.20513, 0.11937]
    c["flat"] = flat
    col = _generic(FS, MS, (1, 1, 777), 1, 5)
    col["Af"] = np.zeros((3, 3))
    col["Af"][:, 2] = np.array([14.0, 12.0, 10.0]) * 1.13719 / 776.0            # a diagonal walk through the volume
    col["Am"] = R @ np.diag([13.0 / 14.0, 1.0, 11.0 / 10.0]) @ col["Af"]
    c["column"] = col
    svx = _generic(FS, MS, (16, 41, 29), 16, 6)
    svx["bf"][0], svx["bm"][0] = 3.41273, 5.73119                               # every sample has lattice x = 0
    c["stride_vx"] = svx
    c["ragged"] = _generic(FS, MS, (23, 13, 9), 1, 7)
    c["virtual64"] = _generic(FS, MS, (2053, 2039, 521), 700001, 8)
    c["lanes8"] = _generic(FS, MS, (29, 23, 19), 1, 9)
    c["fold_corr"] = _generic(FS, MS, (37, 31, 23), 1, 10)
    c["fold_msq"] = _generic(FS, MS, (53, 47, 31), 1, 11)
    c["strided"] = _generic(FS, MS, (113, 89, 53), 1, 12)
    return c


CASES = _cases()
ALL = list(CASES)
SOME = ["band", "ragged", "fold_corr"]
SAMPLES = {"band": 5355, "ties": 17160, "nx1": 3952, "flat": 19, "column": 777, "stride_vx": 1189, "ragged": 2691, "virtual64": 3116,
           "lanes8": 12673, "fold_corr": 26381, "fold_msq": 77221, "strided": 533021}


@functools.lru_cache(maxsize=None)
def data(key):
    """Images and masks of a case (read-only, shared by every test of the case)."""
    c = CASES[key]
    rng = np.random.default_rng(1000 + c["seed"])
    F = (100 * rng.standard_normal(c["fshape"])).astype(np.float32)
    M = (100 * rng.standard_normal(c["mshape"])).astype(np.float32)
    fm = (rng.random(c["fshape"]) > 0.3).astype(np.uint8)
    mm = (rng.random(c["mshape"]) > 0.3).astype(np.uint8)
    GI = (100 * rng.standard_normal((3,) + c["mshape"])).astype(np.float32)
    nsamp = SAMPLES[key]
    jit = (rng.standard_normal((nsamp, 3)) / 3.0).astype(np.float32)
    for a in (F, M, fm, mm, GI, jit):
        a.setflags(write=False)
    v = c["vsize"]
    assert (v[0] * v[1] * v[2] + c["stride"] - 1) // c["stride"] == nsamp
    return F, M, fm, mm, GI, jit


def size_of(shape):
    return (shape[2], shape[1], shape[0])


@functools.lru_cache(maxsize=None)
def reference(key, masks="fm", jitter=False, gimg=False, cand=0):
    """Restatement of a case (candidate 0 = the case's own map), computed once."""
    c = CASES[key]
    F, M, fm, mm, GI, jit = data(key)
    Am, bm = candidates(key)[cand]
    s = LR.Samples(F, M, c["Af"], c["bf"], Am, bm, c["vsize"], c["stride"], fm if "f" in masks else None, mm if "m" in masks else None,
                   jit if jitter else None, GI if gimg else None)
    m = s.margin if jitter else s.margin_of(c["exact"])          # (jitter makes every coordinate generic)
    assert m >= MARGIN, (key, cand, m)
    return s


@functools.lru_cache(maxsize=None)
def candidates(key):
    """Sixteen candidate maps: 0 the case's own, 2 without any overlap, the rest perturbed by non-round amounts (a dyadic case
    by multiples of 2^-10, so that it stays exact)."""
    c = CASES[key]
    rng = np.random.default_rng(2000 + c["seed"])
    out = []
    for k in range(16):
        dA, db = 0.004 * rng.standard_normal((3, 3)), 0.3 * rng.standard_normal(3)
        if set(c["exact"]) == {"f", "m"}:
            dA, db = np.round(dA * 1024) / 1024, np.round(db * 1024) / 1024
        if k == 0:
            dA, db = 0.0, 0.0
        Am, bm = c["Am"] + dA, c["bm"] + db
        if k == 2:
            bm = c["bm"] + 512.0
        if np.all(c["Am"][0] == 0.0):
            Am[0, :] = 0.0
        out.append((Am, bm))
    return out


def call_args(be, key, masks="fm"):
    c = CASES[key]
    F, M, fm, mm, _, _ = data(key)
    return dict(fixed=be.dev(F), fsize=size_of(c["fshape"]), moving=be.dev(M), msize=size_of(c["mshape"]), Af=c["Af"].ravel(), bf=c["bf"],
                vsize=c["vsize"], stride=c["stride"], fixed_mask=be.dev(fm) if "f" in masks else None,
                moving_mask=be.dev(mm) if "m" in masks else None)


def note(be, key, path, got, want, bound):
    err = np.abs(np.asarray(got) - want)
    frac = float(np.max(err / np.where(bound > 0, bound, np.inf))) if np.any(bound > 0) else 0.0
    _STATS[f"{be.name}:{key}:{path}"] = {"max_abs_error": float(err.max()), "error_over_bound": frac,
                                         "error_over_largest_sum": float(err.max() / max(np.abs(want).max(), 1e-300))}
    record_stats("linear_metric", _STATS)


def within(got, want, bound, what):
    got = np.asarray(got)
    assert np.isfinite(got).all(), what
    bad = ~(np.abs(got - want) <= bound)
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5], bound[bad][:5])


def grad_calls(be, a, Am, bm):
    """Both gradient-bearing entry points -> {fn: sums}; the second call bit-equal."""
    out = {}
    for name in ("meansq_affine", "corr_moments_affine"):
        fn = getattr(be.ctx, name)
        r = np.array(fn(a["fixed"], a["fsize"], a["moving"], a["msize"], a["Af"], a["bf"], np.asarray(Am).ravel(), bm, a["vsize"], a["stride"],
                        fixed_mask=a["fixed_mask"], moving_mask=a["moving_mask"]))
        again = np.array(fn(a["fixed"], a["fsize"], a["moving"], a["msize"], a["Af"], a["bf"], np.asarray(Am).ravel(), bm, a["vsize"],
                            a["stride"], fixed_mask=a["fixed_mask"], moving_mask=a["moving_mask"]))
        assert np.array_equal(r, again), name
        out[name] = r
    return out


def check_grad(be, key, path, got, s):
    for name, r in got.items():
        want, bound = LR.meansq(s) if name == "meansq_affine" else LR.corr(s)
        cnt = 1 if name == "meansq_affine" else 0
        assert r[cnt] == want[cnt] == s.count, (key, path, name, r[cnt], want[cnt])
        note(be, key, f"{path}:{name}", r, want, bound)
        within(r, want, bound, (key, path, name))


# --------------------------------------------------------------------------------------
# the restatement itself (CPU only)


def test_restatement_reproduces_multilinear_polynomials_in_closed_form():
    """On F = a + b x + c y + d z + e x y + f x z + g y z + h x y z the trilinear interpolant IS the polynomial in the interior,
    so value, gradient and every sum have closed forms over the interior samples."""
    z, y, x = np.meshgrid(np.arange(9.0), np.arange(11.0), np.arange(13.0), indexing="ij")

    def poly(k, x, y, z):
        return k[0] + k[1] * x + k[2] * y + k[3] * z + k[4] * x * y + k[5] * x * z + k[6] * y * z + k[7] * x * y * z

    def dpoly(k, x, y, z):
        return np.stack([k[1] + k[4] * y + k[5] * z + k[7] * y * z, k[2] + k[4] * x + k[6] * z + k[7] * x * z,
                         k[3] + k[5] * x + k[6] * y + k[7] * x * y], axis=1)

    kf = np.array([3.1, -0.7, 0.45, 1.3, 0.021, -0.013, 0.034, 0.0017])
    km = np.array([-1.9, 0.55, -0.38, 0.9, -0.017, 0.026, 0.011, -0.0023])
    F, M = poly(kf, x, y, z), poly(km, x, y, z)
    # interior: every sample inside [0, n - 1] of both images
    Af, bf = np.diag([0.43719, 0.51357, 0.38823]), np.array([0.7137, 0.2291, 0.6113])
    Am, bm = R @ np.diag([0.41, 0.47, 0.36]), np.array([1.3137, 0.9291, 0.8113])
    vsize, stride = (17, 13, 11), 3
    s = LR.Samples(F, M, Af, bf, Am, bm, vsize, stride)
    v = LR.lattice(vsize, stride)
    cf, cm = v @ Af.T + bf, v @ Am.T + bm
    assert s.count == len(v) and cf.min() > 0 and cm.min() > 0 and np.all(cf < [12, 10, 8]) and np.all(cm < [12, 10, 8])
    f, m, g = poly(kf, *cf.T), poly(km, *cm.T), dpoly(km, *cm.T)
    t = np.concatenate([(g[:, :, None] * v[:, None, :]).reshape(len(v), 9), g], axis=1)
    want_sq = np.concatenate([[((f - m) ** 2).sum(), len(v)], (-2 * (f - m)[:, None] * t).sum(0)])
    want_co = np.concatenate([[len(v), f.sum(), m.sum(), (f * f).sum(), (m * m).sum(), (f * m).sum()], t.sum(0), (f[:, None] * t).sum(0),
                              (m[:, None] * t).sum(0)])
    np.testing.assert_allclose(LR.meansq(s)[0], want_sq, rtol=1e-10, atol=1e-10 * np.abs(want_sq).max())
    np.testing.assert_allclose(LR.corr(s)[0], want_co, rtol=1e-10, atol=1e-10 * np.abs(want_co).max())
    np.testing.assert_allclose(LR.values(0, s)[0][:2], want_sq[:2], rtol=1e-10)
    np.testing.assert_allclose(LR.values(1, s)[0], want_co[:6], rtol=1e-10)
    # the bands: the value is the edge voxel's; the gradient along the axis is zero in the upper band and the first cell's slope
    # (for this polynomial: the derivative at the clamped point) in the lower one; across the axis it is the clamped point's
    edge = np.array([[-0.3, 4.2, 3.1], [12.4, 4.2, 3.1], [5.5, -0.5, 3.1], [5.5, 4.2, 8.25]])
    clamped = np.clip(edge, 0, [12, 10, 8])
    np.testing.assert_allclose(LR.interp(F, edge), poly(kf, *clamped.T), rtol=1e-12)
    ge, gc = LR.interp_gradient(F, edge), dpoly(kf, *clamped.T)
    for i, (axis, upper) in enumerate(((0, False), (0, True), (1, False), (2, True))):
        if upper:
            assert ge[i, axis] == 0.0
            gc[i, axis] = 0.0
        np.testing.assert_allclose(ge[i], gc[i], rtol=1e-10)


@pytest.mark.parametrize("key", ["ragged", "stride_vx", "virtual64"])
def test_restatement_agrees_with_the_oracle(key):
    """Second opinion: oracle/linear_oracle.py gathers eight corners, the restatement asks scipy's spline interpolator; 1e-11 of
    the largest sum of the call, counts equal -- plain, with jitter and with a gradient image, both masks.  Each of the three
    cases has accepted samples in both half-voxel bands of the moving image."""
    from oracle import linear_oracle as O

    c = CASES[key]
    F, M, fm, mm, GI, jit = data(key)
    for kw, okw in ((dict(), dict()), (dict(jitter=True), dict(jitter=jit)), (dict(gimg=True), dict(moving_gradient=GI))):
        s = reference(key, **kw)
        nm = LR.size_xyz(M)
        assert (s.cmo < 0).any() and (s.cmo >= nm - 1).any()
        for mine, theirs, cnt in ((LR.meansq, O.meansq_affine, 1), (LR.corr, O.corr_moments_affine, 0)):
            got = mine(s)[0]
            want = theirs(F, M, c["Af"], c["bf"], c["Am"], c["bm"], c["vsize"], c["stride"], fm, mm, **okw)
            assert got[cnt] == want[cnt] > 50
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-11 * np.abs(want).max())
    bins = mi_bins(key, 0, 50)[1]
    s = reference(key)
    hist, count, _, q = LR.mi_histogram(s, bins)
    oh, oc = O.mi_histogram(F, M, c["Af"], c["bf"], c["Am"], c["bm"], c["vsize"], c["stride"], bins, fm, mm)
    assert count == oc
    # The oracle rounds the interpolated values to fp32 first.  Per bin: every sample that touches the bin moves its weight by at
    # most the B-spline's slope (|B'| <= 2/3 < 1) times the rounding of its bin coordinate, 2^-24 |m| / m_bin, plus the square
    # of that; no fixed bin may flip (no sample within 2^-24 |f| / f_bin of a bin edge: asserted).
    assert (np.abs(q.tf - np.round(q.tf)) > 2.0 ** -24 * np.abs(s.f) / bins["f_bin"]).all()
    shift = 2.0 ** -24 * np.abs(s.m) / bins["m_bin"]
    per_bin = np.zeros_like(hist)
    for d in (-1, 0, 1, 2):
        np.add.at(per_bin, (q.fb, q.mb + d), shift + shift ** 2)
    assert (np.abs(hist - oh) <= per_bin).all(), np.abs(hist - oh).max()


# --------------------------------------------------------------------------------------
# value + gradient


@pytest.mark.parametrize("key", ALL)
def test_gradient_kernels(backend, key):
    """pp_meansq_affine_f32 / pp_corr_moments_affine_f32, both masks: counts equal, every sum within its bound, the second
    call bit-equal."""
    s = reference(key)
    assert s.count > (4 if key == "flat" else 50) and s.count < 0.8 * SAMPLES[key]
    a = call_args(backend, key)
    check_grad(backend, key, "grad", grad_calls(backend, a, CASES[key]["Am"], CASES[key]["bm"]), s)


@pytest.mark.parametrize("key", SOME)
@pytest.mark.parametrize("masks", ["", "f", "m"])
def test_mask_combinations(backend, key, masks):
    s, both = reference(key, masks=masks), reference(key)
    assert s.count > both.count
    a = call_args(backend, key, masks)
    check_grad(backend, key, "masks=" + (masks or "none"), grad_calls(backend, a, CASES[key]["Am"], CASES[key]["bm"]), s)
    for metric in (0, 1):
        Am, bm = candidates(key)[1]
        r = backend.ctx.metric_values_affine(metric, a["fixed"], a["fsize"], a["moving"], a["msize"], a["Af"], a["bf"], [CASES[key]["Am"], Am],
                                             [CASES[key]["bm"], bm], a["vsize"], a["stride"], fixed_mask=a["fixed_mask"], moving_mask=a["moving_mask"])
        for row, sc in ((0, s), (1, reference(key, masks=masks, cand=1))):
            want, bound = LR.values(metric, sc)
            assert r[row, 1 - metric] == sc.count
            within(r[row], want, bound, (key, masks, metric, row))


@pytest.mark.parametrize("key", SOME)
def test_gradient_image(backend, monkeypatch, key):
    """The filtered-gradient-image paths (k_metric_grad<., 1> planar, <., 2> packed), both masks."""
    c = CASES[key]
    F, M, fm, mm, GI, _ = data(key)
    s = reference(key, gimg=True)
    a = call_args(backend, key)
    plain = grad_calls(backend, a, c["Am"], c["bm"])
    dgi = backend.dev(GI)
    packed = backend.dev(np.ascontiguousarray(np.concatenate([np.moveaxis(GI, 0, -1), M[..., None]], axis=-1)))
    try:
        backend.ctx.set_moving_gradient(dgi, a["msize"], packed=packed)
        monkeypatch.setenv("PP_METRIC_GRAD_PLANAR", "1")
        planar = grad_calls(backend, a, c["Am"], c["bm"])
        monkeypatch.delenv("PP_METRIC_GRAD_PLANAR", raising=False)
        pack = grad_calls(backend, a, c["Am"], c["bm"])
    finally:
        backend.ctx.set_moving_gradient(None)
    check_grad(backend, key, "gimg:planar", planar, s)
    check_grad(backend, key, "gimg:packed", pack, s)
    for k in planar:
        np.testing.assert_allclose(pack[k], planar[k], rtol=0, atol=1e-12 * np.abs(planar[k]).max())
        nval = 2 if k == "meansq_affine" else 6
        np.testing.assert_allclose(planar[k][:nval], plain[k][:nval], rtol=0, atol=1e-12 * np.abs(plain[k][:nval]).max())
        assert np.abs(planar[k][nval:] - plain[k][nval:]).max() > 1e-2 * np.abs(plain[k][nval:]).max()
    after = grad_calls(backend, a, c["Am"], c["bm"])
    for k in plain:
        assert np.array_equal(after[k], plain[k])


@pytest.mark.parametrize("key", SOME)
def test_sample_jitter(backend, key):
    """Every entry point at lattice index + jitter (a seeded N(0, 1/3) array, taken as given); without the array, the plain bits."""
    c = CASES[key]
    jit = data(key)[5]
    s = reference(key, jitter=True)
    a = call_args(backend, key)
    plain = grad_calls(backend, a, c["Am"], c["bm"])
    dj = backend.dev(jit)
    try:
        backend.ctx.set_sample_jitter(dj)
        got = grad_calls(backend, a, c["Am"], c["bm"])
        check_grad(backend, key, "jitter", got, s)
        for metric in (0, 1):
            r = backend.ctx.metric_values_affine(metric, a["fixed"], a["fsize"], a["moving"], a["msize"], a["Af"], a["bf"], [c["Am"]], [c["bm"]],
                                                 a["vsize"], a["stride"], fixed_mask=a["fixed_mask"], moving_mask=a["moving_mask"])
            want, bound = LR.values(metric, s)
            assert r[0, 1 - metric] == s.count
            within(r[0], want, bound, (key, "jitter", metric))
        for kernel, nbins in ((0, 50), (1, 20)):
            b, bd = mi_bins(key, kernel, nbins)
            hist, count = backend.ctx.mi_histogram(a["fixed"], a["fsize"], a["moving"], a["msize"], a["Af"], a["bf"], c["Am"].ravel(), c["bm"],
                                                   a["vsize"], a["stride"], b, fixed_mask=a["fixed_mask"], moving_mask=a["moving_mask"])
            want, wcount, bound, _ = LR.mi_histogram(s, bd)
            assert count == wcount
            within(hist, want, bound, (key, "jitter", "mi", kernel))
    finally:
        backend.ctx.set_sample_jitter(None)
    assert got["meansq_affine"][1] != plain["meansq_affine"][1] or got["meansq_affine"][0] != plain["meansq_affine"][0]
    after = grad_calls(backend, a, c["Am"], c["bm"])
    for k in plain:
        assert np.array_equal(after[k], plain[k])


# --------------------------------------------------------------------------------------
# value probes


NCAND = (1, 3, 4, 5, 8, 9, 16)


def _probe_params():
    """(backend, case); the emulator's leg of `strided` walks 533021 samples x 16 candidates thread by thread: marked slow."""
    emu = [pytest.param("emu", k, id=f"emu-{k}", marks=[pytest.mark.slow] if k == "strided" else []) for k in ALL]
    return emu + [pytest.param("gpu", k, id=f"gpu-{k}", marks=pytest.mark.gpu) for k in ALL]


@pytest.mark.parametrize("backend,key", _probe_params(), indirect=["backend"])
def test_value_probes(backend, key):
    """pp_metric_values_affine_f32, both metrics, 1 .. 16 candidates (one or two mailbox writers): counts equal, values
    within bound, candidate 0 = the gradient-bearing call, candidate 2 (no overlap) exactly zero, and a candidate's bits
    independent of its companions."""
    c = CASES[key]
    cand = candidates(key)
    a = call_args(backend, key)
    grad = grad_calls(backend, a, c["Am"], c["bm"])
    ncs = (3, 16) if key == "strided" else NCAND
    refs = {k: reference(key, cand=k) for k in range(16) if k != 2}
    assert len({refs[k].count for k in refs}) > (2 if key == "flat" else 8)                 # the perturbations move samples across borders and mask voxels

    def run(metric, maps):
        return backend.ctx.metric_values_affine(metric, a["fixed"], a["fsize"], a["moving"], a["msize"], a["Af"], a["bf"], [m[0] for m in maps],
                                                [m[1] for m in maps], a["vsize"], a["stride"], fixed_mask=a["fixed_mask"],
                                                moving_mask=a["moving_mask"])

    for metric in (0, 1):
        cnt, nv = 1 - metric, 2 if metric == 0 else 6
        first = grad["meansq_affine"][:2] if metric == 0 else grad["corr_moments_affine"][:6]
        rows = {}
        for n in ncs:
            r = run(metric, cand[:n])
            assert r.shape == (n, 6) and np.isfinite(r).all()
            for k in range(n):
                if k == 2:
                    assert np.array_equal(r[k], np.zeros(6)), (key, metric, n, r[k])
                    continue
                want, bound = LR.values(metric, refs[k])
                assert r[k, cnt] == refs[k].count, (key, metric, n, k, r[k, cnt], refs[k].count)
                within(r[k], want, bound, (key, metric, n, k))
                assert np.array_equal(r[k, nv:], np.zeros(6 - nv))
                if k in rows:     # the same candidate in a smaller batch: the lane kernel's layout does not depend on the batch
                    assert np.array_equal(r[k], rows[k]), (key, metric, n, k)
                rows[k] = r[k]
            np.testing.assert_allclose(r[0, :nv], first, rtol=0, atol=1e-12 * np.abs(first).max())
            assert r[0, cnt] == first[cnt]
            assert np.array_equal(run(metric, cand[:n]), r)
            if n in (3, 5, 16):     # other companions in the other slots: the same bits
                other = list(cand[:n])
                keep = 1 if n == 3 else 4
                swapped = [other[keep] if i == keep else cand[(i + 7) % 16] for i in range(n)]
                assert np.array_equal(run(metric, swapped)[keep], r[keep]), (key, metric, n)
        big = ncs[-1]
        want, bound = LR.values(metric, refs[0])
        note(backend, key, f"values:metric={metric}", run(metric, cand[:big])[0], want, bound)


# --------------------------------------------------------------------------------------
# mutual information


def mi_bins(key, kernel, nbins):
    F, M = data(key)[:2]
    b = _lib.MiBins()
    b.nbins, b.kernel = nbins, kernel
    pad = 2 if kernel == 0 else 0
    # non-round bin widths; the range leaves the tails to the clamped end bins
    b.f_bin = 1.00371 * (float(F.max()) - float(F.min())) / max(nbins - 2 * pad, 1)
    b.m_bin = 0.99173 * (float(M.max()) - float(M.min())) / max(nbins - 2 * pad, 1)
    b.f_norm_min = float(F.min()) / b.f_bin - pad - 0.01337
    b.m_norm_min = float(M.min()) / b.m_bin - pad + 0.02113
    return b, dict(nbins=nbins, kernel=kernel, f_bin=b.f_bin, f_norm_min=b.f_norm_min, m_bin=b.m_bin, m_norm_min=b.m_norm_min)


@pytest.mark.parametrize("kernel,nbins", [(0, 5), (0, 50), (0, 64), (1, 2), (1, 20), (1, 64)])
@pytest.mark.parametrize("key", ["band", "ragged", "fold_corr", "strided"])
def test_mi_kernels(backend, key, kernel, nbins):
    """pp_mi_histogram_f32 / pp_mi_gradient_f32 with both masks at the bin limits: equal count, histogram mass = count, the joint
    histogram exactly equal (but for listed samples on a bin edge), Mattes bins and the gradient within bound, twice the same
    bits."""
    c = CASES[key]
    s = reference(key)
    a = call_args(backend, key)
    b, bd = mi_bins(key, kernel, nbins)
    args = (a["fixed"], a["fsize"], a["moving"], a["msize"], a["Af"], a["bf"], c["Am"].ravel(), c["bm"], a["vsize"], a["stride"], b)
    kw = dict(fixed_mask=a["fixed_mask"], moving_mask=a["moving_mask"])
    hist, count = backend.ctx.mi_histogram(*args, **kw)
    want, wcount, bound, q = LR.mi_histogram(s, bd)
    assert count == wcount == s.count
    np.testing.assert_allclose(hist.sum(), count, rtol=1e-9)
    namb = int((q.amb_f | q.amb_m).sum()) if kernel == 1 else int(q.amb_f.sum())
    if key != "strided":
        # the MI part of the precondition: no sample's bin coordinate lies within its own interpolation error of a bin edge
        # (bin_margin = smallest distance minus that error, in bins), so every hard decision is the same on both sides ...
        assert q.bin_margin > 0 and namb == 0, (key, kernel, nbins, q.bin_margin)
        if kernel == 1:
            assert np.array_equal(hist, want)             # ... and the joint histogram is exactly equal
    else:
        # 172700 accepted samples with an error of ~5e-6 bins each: a few on a bin edge are expected under any digits.  They
        # are listed, capped, and only the bins around each may differ, by one unit (`bound` is 0 elsewhere: exact there)
        assert namb <= 1 + s.count // 20000, (key, kernel, nbins, namb)
        if kernel == 1:
            assert np.array_equal(hist[bound == 0], want[bound == 0])
    within(hist, want, bound, (key, kernel, nbins, "histogram"))
    note(backend, key, f"mi_histogram:kernel={kernel}:bins={nbins}", hist, want, bound)
    again, _ = backend.ctx.mi_histogram(*args, **kw)
    assert np.array_equal(hist, again)
    table = np.random.default_rng(5).normal(size=(nbins, nbins))
    g = backend.ctx.mi_gradient(*args, table, **kw)
    wg, gbound, _ = LR.mi_gradient(s, bd, table)
    within(g, wg, gbound, (key, kernel, nbins, "gradient"))
    note(backend, key, f"mi_gradient:kernel={kernel}:bins={nbins}", g, wg, gbound)
    assert np.array_equal(backend.ctx.mi_gradient(*args, table, **kw), g)


# --------------------------------------------------------------------------------------
# Inf / NaN under rejected samples


@pytest.mark.parametrize("key", SOME)
def test_inf_nan_under_rejected_samples(backend, monkeypatch, key):
    """A NaN slab and an Inf slab in both images and the gradient image, under mask voxels that reject every sample whose
    corners could touch them, and NaN at voxel 0 where clamped outside samples gather: every output finite and bit-equal to
    the run on clean images."""
    c = CASES[key]
    F, M, _, _, GI, _ = data(key)
    rng = np.random.default_rng(77)

    def poison(img_shape):
        nz, ny, nx = img_shape
        bad = np.zeros(img_shape, bool)
        bad[nz // 2, 1:ny - 1, nx // 3] = True                       # a NaN slab ...
        inf = np.zeros(img_shape, bool)
        inf[1:nz - 1, ny // 2 + 1, 2 * nx // 3] = True               # ... and an Inf slab
        bad[0, 0, 0] = True
        mask = (rng.random(img_shape) > 0.3)
        from scipy.ndimage import binary_dilation
        mask &= ~binary_dilation(bad | inf, structure=np.ones((3, 3, 3), bool), iterations=2)
        return bad, inf, mask.astype(np.uint8)

    fbad, finf, fm = poison(c["fshape"])
    mbad, minf, mm = poison(c["mshape"])
    s = LR.Samples(F, M, c["Af"], c["bf"], c["Am"], c["bm"], c["vsize"], c["stride"], fm, mm)
    assert s.count > 50
    # no accepted sample of any candidate reads a poisoned voxel
    cand = candidates(key)[:5]
    for Am, bm in cand:
        sc = LR.Samples(F, M, c["Af"], c["bf"], Am, bm, c["vsize"], c["stride"], fm, mm)
        assert not (fbad | finf).ravel()[LR.footprint(c["fshape"], sc.cfo)].any()
        assert not (mbad | minf).ravel()[LR.footprint(c["mshape"], sc.cmo)].any()
    Fp, Mp, GIp = F.copy(), M.copy(), GI.copy()
    Fp[fbad], Fp[finf] = np.nan, np.inf
    Mp[mbad], Mp[minf] = np.nan, -np.inf
    GIp[:, mbad], GIp[:, minf] = np.nan, np.inf

    def run(F_, M_, GI_):
        a = dict(call_args(backend, key), fixed=backend.dev(F_), moving=backend.dev(M_), fixed_mask=backend.dev(fm), moving_mask=backend.dev(mm))
        out = [grad_calls(backend, a, c["Am"], c["bm"])]
        dgi = backend.dev(GI_)
        packed = backend.dev(np.ascontiguousarray(np.concatenate([np.moveaxis(GI_, 0, -1), M_[..., None]], axis=-1)))
        try:
            backend.ctx.set_moving_gradient(dgi, a["msize"], packed=packed)
            out.append(grad_calls(backend, a, c["Am"], c["bm"]))
            monkeypatch.setenv("PP_METRIC_GRAD_PLANAR", "1")
            out.append(grad_calls(backend, a, c["Am"], c["bm"]))
        finally:
            monkeypatch.delenv("PP_METRIC_GRAD_PLANAR", raising=False)
            backend.ctx.set_moving_gradient(None)
        probes = {}
        for metric in (0, 1):
            probes[metric] = backend.ctx.metric_values_affine(metric, a["fixed"], a["fsize"], a["moving"], a["msize"], a["Af"], a["bf"],
                                                              [m[0] for m in cand], [m[1] for m in cand], a["vsize"], a["stride"],
                                                              fixed_mask=a["fixed_mask"], moving_mask=a["moving_mask"])
        return out, probes

    (clean, clean_p), (dirty, dirty_p) = run(F, M, GI), run(Fp, Mp, GIp)
    check_grad(backend, key, "poison-masks", clean[0], s)
    for cl, di in zip(clean, dirty):
        for k in cl:
            assert np.isfinite(di[k]).all(), k
            assert np.array_equal(di[k], cl[k]), k
    for k in clean_p:
        assert np.isfinite(dirty_p[k]).all() and np.array_equal(dirty_p[k], clean_p[k]), k


# --------------------------------------------------------------------------------------
# the cached (FAST) paths: inside pp_linear_optimize_f32 only


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("key", ["band", "ragged", "lanes8"])
def test_cached_paths_against_the_restatement(backend, monkeypatch, key, metric, jitter):
    """One gradient-descent iteration of the translation model on unit geometry: history[0] is the metric at the start through
    k_metric_grad reading the fixed-sample cache; with PP_LINREG_RETURN_BEST stats.value is the metric at the returned point,
    through walk<FAST, MASKED> of the lane kernel when the step was taken.  Both against the restatement at those
    parameters, and bit-equal to the run without the cache."""
    c = CASES[key]
    F, M, fm, mm, _, jit = data(key)
    init = c["Am"] @ np.linalg.inv(c["Af"])              # moving index = init (fixed-side physical point + t) + offset
    off = c["bm"] - init @ c["bf"]
    lv = _lib.LinregLevel()
    lv.model, lv.metric, lv.optimizer, lv.iterations = _lib.MODEL_TRANSLATION, metric, _lib.OPT_GD, 1
    lv.vsize[:] = list(c["vsize"])
    lv.stride, lv.speculation, lv.flags = c["stride"], 4, _lib.LINREG_RETURN_BEST
    lv.v_i2p[:] = c["Af"].ravel().tolist()
    lv.v_origin[:] = c["bf"].tolist()
    lv.f_p2i[:] = np.eye(3).ravel().tolist()
    lv.m_p2i[:] = np.eye(3).ravel().tolist()
    lv.f_origin[:] = [0.0, 0.0, 0.0]
    lv.m_origin[:] = [0.0, 0.0, 0.0]
    lv.init_matrix[:] = init.ravel().tolist()
    lv.init_offset[:] = off.tolist()
    lv.center[:] = [0.0, 0.0, 0.0]
    lv.v_min_spacing = 0.00571
    a = call_args(backend, key)
    dj = backend.dev(jit) if jitter else None

    def value_at(p):
        Am, bm = init @ c["Af"], init @ (c["bf"] + p) + off
        s = LR.Samples(F, M, c["Af"], c["bf"], Am, bm, c["vsize"], c["stride"], fm, mm, jit if jitter else None)
        assert (s.margin if jitter else s.margin_of(c["exact"])) >= MARGIN
        sums, bound = LR.meansq(s) if metric == 0 else LR.corr(s)
        fn = LR.meansq_value if metric == 0 else LR.corr_value
        return fn(sums), LR.value_bound(fn, sums, bound)

    # On noise images a descent step of fixed length may land on a worse value, and RETURN_BEST then hands back the start with
    # the gradient kernel's number: further starts are tried until one step is kept.  Every start is checked in full.
    kept = False
    for p0 in (np.array([0.01373, -0.02117, 0.00931]), np.array([-0.13719, 0.09343, 0.05171]), np.array([0.21373, 0.17117, -0.11931])):
        out = {}
        try:
            backend.ctx.set_sample_jitter(dj)
            for nocache in ("1", None):
                if nocache:
                    monkeypatch.setenv("PP_NO_FIXED_SAMPLES", nocache)
                else:
                    monkeypatch.delenv("PP_NO_FIXED_SAMPLES", raising=False)
                p, st, hist = backend.ctx.linear_optimize(a["fixed"], a["fsize"], a["moving"], a["msize"], lv, p0, a["fixed_mask"],
                                                          a["moving_mask"], history=1)
                out[nocache] = (np.array(p), st.value, hist[0], st.iterations)
        finally:
            backend.ctx.set_sample_jitter(None)
        p, value, h0, its = out[None]
        assert its == 1 and np.array_equal(out["1"][0], p) and out["1"][1] == value and out["1"][2] == h0
        want0, b0 = value_at(p0)
        assert abs(h0 - want0) <= b0, (h0, want0, b0)
        want1, b1 = value_at(p)
        assert abs(value - want1) <= b1, (value, want1, b1)
        _STATS[f"{backend.name}:{key}:cached:metric={metric}:jitter={jitter}"] = {
            "start_error_over_bound": abs(h0 - want0) / b0, "end_error_over_bound": abs(value - want1) / b1}
        record_stats("linear_metric", _STATS)
        if not np.array_equal(p, p0):                     # the step was kept: stats.value came from the lane kernel
            kept = True
            break
        assert value == h0
    assert kept


@pytest.mark.parametrize("itk_sampling", [False, True])
@pytest.mark.parametrize("metric", ["mean_squares", "correlation"])
def test_fixed_sample_cache_with_a_moving_mask_does_not_change_the_optimisation(backend, monkeypatch, metric, itk_sampling):
    """test_linear.py's cache test passes only a fixed mask; with moving_structure the probes run walk<FAST, MASKED>."""
    import torch

    import platipy_amd as pa
    from platipy_amd import runtime
    from tests.test_linear import _rigid_pair

    if backend.name == "emu":
        monkeypatch.setattr(runtime, "context", lambda device=None: backend.ctx)
        monkeypatch.setattr(runtime, "default_device", lambda: torch.device("cpu"))
    shape, spacing, origin = (16, 20, 24), (1.5, 1.5, 2.5), (-30.0, -20.0, 10.0)
    fix, mov, _ = _rigid_pair(pa, shape, spacing, origin, angle=0.05, shift=(1.5, -1.0, 1.0))
    m = np.zeros(shape, np.uint8)
    m[2:14, 3:17, 4:20] = 1
    m2 = np.zeros(shape, np.uint8)
    m2[1:15, 2:18, 3:21] = 1
    out = {}
    for off in ("1", None):
        if off:
            monkeypatch.setenv("PP_NO_FIXED_SAMPLES", off)
        else:
            monkeypatch.delenv("PP_NO_FIXED_SAMPLES", raising=False)
        _, tfm = pa.registration.linear_registration(
            pa.image_from_array(fix, spacing, origin), pa.image_from_array(mov, spacing, origin), reg_method="affine", metric=metric,
            optimiser="gradient_descent_line_search", shrink_factors=[2, 1], smooth_sigmas=[0, 0], sampling_rate=0.5, number_of_iterations=5,
            fixed_structure=pa.image_from_array(m, spacing, origin), moving_structure=pa.image_from_array(m2, spacing, origin),
            itk_sampling=itk_sampling)
        out[off] = np.asarray(tfm.transforms[1].GetParameters())
    assert np.abs(out[None] - np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.0])).max() > 1e-3
    np.testing.assert_array_equal(out["1"], out[None])


# --------------------------------------------------------------------------------------
# refusals (a too-short jitter array and a gradient image of another size: tests/test_linear.py)


def test_refusals_leave_the_outputs_alone(backend):
    key = "flat"
    c = CASES[key]
    a = call_args(backend, key, masks="")
    lib, h, ptr = backend.lib, backend.ctx.h, _lib.ptr
    dp = C.POINTER(C.c_double)
    i3, dn = _lib._i3, _lib._dn
    Am = np.ascontiguousarray(np.tile(c["Am"].ravel(), (17, 1)))
    bm = np.ascontiguousarray(np.tile(c["bm"], (17, 1)))
    SENTINEL = -12345.678

    def values(ncand, vsize, stride):
        res = np.full((17, 6), SENTINEL)
        rc = lib.pp_metric_values_affine_f32(h, 0, ptr(a["fixed"]), i3(a["fsize"]), ptr(a["moving"]), i3(a["msize"]), dn(a["Af"], 9), dn(a["bf"], 3),
                                             ncand, Am.ctypes.data_as(dp), bm.ctypes.data_as(dp), i3(vsize), stride, None, None, res.ctypes.data_as(dp))
        return rc, res

    def grad(fn, vsize, stride):
        res = np.full(42, SENTINEL)
        rc = fn(h, ptr(a["fixed"]), i3(a["fsize"]), ptr(a["moving"]), i3(a["msize"]), dn(a["Af"], 9), dn(a["bf"], 3), dn(c["Am"].ravel(), 9),
                dn(c["bm"], 3), i3(vsize), stride, None, None, res.ctypes.data_as(dp))
        return rc, res

    def hist(kernel, nbins, vsize=c["vsize"], stride=1):
        b = _lib.MiBins()
        b.nbins, b.kernel, b.f_bin, b.m_bin, b.f_norm_min, b.m_norm_min = nbins, kernel, 10.0, 10.0, -30.0, -30.0
        res, count = np.full(65 * 65, SENTINEL), C.c_double(SENTINEL)
        rc = lib.pp_mi_histogram_f32(h, ptr(a["fixed"]), i3(a["fsize"]), ptr(a["moving"]), i3(a["msize"]), dn(a["Af"], 9), dn(a["bf"], 3),
                                     dn(c["Am"].ravel(), 9), dn(c["bm"], 3), i3(vsize), stride, None, None, C.byref(b), res.ctypes.data_as(dp),
                                     C.byref(count))
        return rc, np.append(res, count.value)

    refused = [values(0, c["vsize"], 1), values(17, c["vsize"], 1), values(3, c["vsize"], 0), values(3, (19, 0, 1), 1),
               grad(lib.pp_meansq_affine_f32, c["vsize"], 0), grad(lib.pp_corr_moments_affine_f32, (0, 1, 1), 1),
               hist(_lib.MI_MATTES, 4), hist(_lib.MI_MATTES, 65), hist(_lib.MI_JOINT, 1), hist(_lib.MI_JOINT, 65), hist(_lib.MI_JOINT, 20, stride=0)]
    for rc, res in refused:
        assert rc != 0 and np.all(res == SENTINEL), (rc, res[:6])
    # ... and the context still works
    rc, res = values(16, c["vsize"], 1)
    assert rc == 0 and res[0, 1] == LR.Samples(*data(key)[:2], c["Af"], c["bf"], c["Am"], c["bm"], c["vsize"], 1).count and np.all(res[16] == SENTINEL)
    rc, res = hist(_lib.MI_MATTES, 5)
    assert rc == 0 and res[-1] == values(1, c["vsize"], 1)[1][0, 1]
