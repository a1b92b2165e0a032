"""Mattes mutual information over a cubic B-spline transform: the two kernels (pp_bspline_mi_histogram_f32,
pp_bspline_mi_gradient_f32), the host's value and score table between them, and bspline_registration(metric="mattes_mi"),
held to the fp64 restatement in tests/bspline_mi_restatement.py with its derived bounds (parity with ITK itself is unpinned:
DESIGN.md section 8)."""
import ctypes as C

import numpy as np
import pytest

from platipy_amd import _lib
from tests import bspline_mi_restatement as RM
from tests import bspline_restatement as R

SIZE, SPACING, ORIGIN = (33, 27, 20), (0.9, 1.1, 2.5), (320.0, -52.0, 60.0)
EYE = (1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0)
FLIP = (-1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0)
MOVING = ((31, 29, 22), (1.0, 1.0, 2.3), (318.5, -53.0, 58.0), np.eye(3))
MESH_A, MESH_B, MESH_C = (3, 2, 2), (1, 1, 1), (11, 9, 11)      # A, B: cut into 16 z slabs; C: 1089 cells, none cut, narrower than the margin
_SHARED = {}


def _inputs():
    """images, masks, jitter and gradient image shared by the kernel tests (built once, never written to)"""
    if "fixed" not in _SHARED:
        # Seed 61, and no case at stride 1 without jitter: a lattice that visits the image's brightest or darkest voxel puts a sample
        # exactly on the first or last bin edge, which the restatement lists as ambiguous (the clamp makes either side the same
        # bin, but the list does not know); the condition on that list is asserted before any kernel runs (_check_ambiguity)
        fixed = R.blobs(SIZE[::-1], 61, noise=3.0)
        moving = (260.0 - 0.8 * R.blobs(MOVING[0][::-1], 22, noise=3.0)).astype(np.float32)       # another "modality": inverted, rescaled
        nz, ny, nx = SIZE[::-1]
        zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        fmask = ((((xx - 16) / 14.0) ** 2 + ((yy - 13) / 11.0) ** 2 + ((zz - 10) / 8.5) ** 2) < 1).astype(np.uint8)
        mmask = np.ones(MOVING[0][::-1], dtype=np.uint8)
        mmask[:, :, 24:] = 0
        mmask[:4] = 0
        grad = np.stack([np.gradient(moving.astype(np.float64), axis=a) for a in (2, 1, 0)]).astype(np.float32)
        packed = np.ascontiguousarray(np.concatenate([np.moveaxis(grad, 0, -1), moving[..., None]], axis=-1))
        rng = np.random.default_rng(24)      # (23 leaves one sample of case A-jit-30 within 2e-6 of a fixed-bin edge)
        jitter = {s: (rng.standard_normal(((np.prod(SIZE) + s - 1) // s, 3)) / 3.0).astype(np.float32) for s in (1, 2)}
        _SHARED.update(fixed=fixed, moving=moving, fmask=fmask, mmask=mmask, grad=grad, packed=packed, jitter=jitter)
    return _SHARED


CASES = {
    # mesh, stride, jitter, gradient source (None: analytic, "planar", "packed"), masks, bins, flipped direction
    "A-jit-30": (MESH_A, 1, True, None, False, 30, False),
    "A-s2-jit-packed-masks-30": (MESH_A, 2, True, "packed", True, 30, False),
    "B-jit-masks-5": (MESH_B, 1, True, None, True, 5, False),
    "A-s2-jit-planar-masks-64": (MESH_A, 2, True, "planar", True, 64, False),
    "A-s2-packed-flipped-30": (MESH_A, 2, False, "packed", False, 30, True),
    "B-s2-planar-64": (MESH_B, 2, False, "planar", False, 64, False),
    "C-jit-masks-30": (MESH_C, 1, True, None, True, 30, False),
}
CASE_IDS = list(CASES)


def _case(name):
    """geometry, inputs and the restatement of a case (computed once, shared by the tests, never written to)"""
    key = ("case", name)
    if key not in _SHARED:
        mesh, stride, jitter, source, masks, nbins, flipped = CASES[name]
        d = _inputs()
        direction = FLIP if flipped else EYE
        origin = (ORIGIN[0] + (SIZE[0] - 1) * SPACING[0], ORIGIN[1], ORIGIN[2]) if flipped else ORIGIN
        lat = R.initializer(SIZE, SPACING, origin, direction, mesh)
        cx, cy, cz = (int(s) for s in lat["lattice_size"])
        coef = np.random.default_rng(31).normal(0, 1.5, size=(3, cz, cy, cx)).astype(np.float32)
        fg = (SIZE, SPACING, origin, np.reshape(direction, (3, 3)))
        jit = d["jitter"][stride] if jitter else None
        fm, mm = (d["fmask"], d["mmask"]) if masks else (None, None)
        s = RM.Samples(d["fixed"], fg, d["moving"], MOVING, fg, stride, coef, lat, fm, mm, jit, d["grad"] if source else None)
        b = RM.bins(nbins, d["fixed"], d["moving"], fm, mm)
        hist, hbound, q = RM.histogram(s, b)
        table = np.random.default_rng(47).normal(0, 1.0, size=(nbins, nbins))        # any table: pass 2 is linear in it
        _SHARED[key] = dict(mesh=mesh, stride=stride, source=source, nbins=nbins, direction=direction, origin=origin, lat=lat, coef=coef,
                            fg=fg, jit=jit, fm=fm, mm=mm, s=s, b=b, hist=hist, hbound=hbound, amb=int(q.amb_f.sum()), table=table)
    return _SHARED[key]


def _mibins(b, kernel=_lib.MI_MATTES):
    m = _lib.MiBins()
    m.nbins, m.kernel, m.f_bin, m.f_norm_min, m.m_bin, m.m_norm_min = b["nbins"], kernel, b["f_bin"], b["f_norm_min"], b["m_bin"], b["m_norm_min"]
    return m


def _lat_geom(lat):
    return _lib.make_geom(lat["lattice_size"], lat["lattice_spacing"], lat["lattice_origin"], lat["direction"].ravel())


class _Installed:
    """the case's buffers on the backend, its jitter and gradient source installed on the context for the `with` block"""

    def __init__(self, backend, c):
        d = _inputs()
        self.ctx, self.c = backend.ctx, c
        dev = lambda a: None if a is None else backend.dev(a)        # noqa: E731
        self.keep = [dev(d["fixed"]), dev(d["moving"]), dev(c["coef"]), dev(c["fm"]), dev(c["mm"]), dev(c["jit"]), dev(d["grad"]), dev(d["packed"])]
        geom = _lib.make_geom(SIZE, SPACING, c["origin"], c["direction"])
        self.args = (self.keep[0], geom, self.keep[1], _lib.make_geom(*MOVING[:3], MOVING[3].ravel()), geom, c["stride"], self.keep[2],
                     _lat_geom(c["lat"]), _mibins(c["b"]))
        self.kw = dict(fixed_mask=self.keep[3], moving_mask=self.keep[4], jitter_bound=0.0 if c["jit"] is None else float(np.abs(c["jit"]).max()))

    def __enter__(self):
        if self.c["jit"] is not None:
            self.ctx.set_sample_jitter(self.keep[5])
        if self.c["source"] == "packed":
            self.ctx.set_moving_gradient(self.keep[6], packed=self.keep[7])
        elif self.c["source"] == "planar":
            self.ctx.set_moving_gradient(self.keep[6])
        return self

    def __exit__(self, *exc):
        self.ctx.set_sample_jitter(None)
        self.ctx.set_moving_gradient(None)


def _check_ambiguity(c):
    """the restatement alone: so few samples sit on a fixed-bin edge that the unit allowance around them says nothing about the rest"""
    valid = c["s"].stats["valid"]
    assert valid > 1000
    assert c["amb"] <= 1 + valid // 20000
    if c["s"].stats["seen"] < 20000:
        assert c["amb"] == 0


# ---- 1. pass 1 -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", CASE_IDS)
def test_histogram_kernel_against_restatement(backend, name):
    c = _case(name)
    _check_ambiguity(c)
    want = c["s"].stats
    with _Installed(backend, c) as k:
        h1, s1 = backend.ctx.bspline_mi_histogram(*k.args, **k.kw)
        h2, s2 = backend.ctx.bspline_mi_histogram(*k.args, **k.kw)
    assert np.array_equal(h1, h2) and s1 == s2                                      # bit-identical between calls
    assert s1 == {k_: float(v) for k_, v in want.items()}
    assert want["seen"] == (np.prod(SIZE) + c["stride"] - 1) // c["stride"]
    assert want["outside"] > 0                                                      # samples leave the moving buffer
    if c["fm"] is not None:
        assert want["masked"] > 0
    np.testing.assert_allclose(h1.sum(), want["valid"], rtol=1e-9)                  # the four weights of a sample sum to one
    excess = np.abs(h1 - c["hist"]) - c["hbound"]
    print(f"{name}: valid {want['valid']}, max |hist - want| = {np.abs(h1 - c['hist']).max():.3e}, max bound {c['hbound'].max():.3e}, "
          f"worst excess {excess.max():.3e}")
    assert np.all(excess <= 0.0)


# ---- 2. pass 2 -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", CASE_IDS)
def test_gradient_kernel_against_restatement(backend, name):
    c = _case(name)
    _check_ambiguity(c)
    want, bound, _ = RM.gradient(c["s"], c["b"], c["table"])
    with _Installed(backend, c) as k:
        g1, s1 = backend.ctx.bspline_mi_gradient(*k.args, c["table"], **k.kw)
        g2, s2 = backend.ctx.bspline_mi_gradient(*k.args, c["table"], **k.kw)
    assert np.array_equal(g1, g2) and s1 == s2
    assert s1 == {k_: float(v) for k_, v in c["s"].stats.items()}
    excess = np.abs(g1 - want) - bound
    print(f"{name}: max |g| = {np.abs(want).max():.3e}, max |g - want| = {np.abs(g1 - want).max():.3e}, max bound {bound.max():.3e}, "
          f"worst excess {excess.max():.3e}")
    assert np.abs(want).max() > 0
    assert np.all(excess <= 0.0)
    untouched = RM.outside_support(c["s"])
    if c["mesh"] == MESH_C:
        assert untouched.any()                                                      # the masks leave whole supports of the fine mesh without a sample
    assert np.all(g1[untouched] == 0.0)


# ---- 3. value and gradient together ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", CASE_IDS)
def test_metric_object_value_and_gradient(host_api, name):
    import torch

    from platipy_amd import runtime
    from platipy_amd.registration.bspline import _BSplineMetric

    pa = host_api
    c, d = _case(name), _inputs()
    _check_ambiguity(c)
    f_img = pa.Image(d["fixed"], SPACING, c["origin"], c["direction"])
    m_img = pa.Image(d["moving"], *MOVING[1:3], MOVING[3].ravel())
    dev = f_img.tensor.device
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    fm = None if c["fm"] is None else pa.Image(c["fm"], SPACING, c["origin"], c["direction"])
    mm = None if c["mm"] is None else pa.Image(c["mm"], *MOVING[1:3], MOVING[3].ravel())
    t = pa.bspline_transform_initializer(f_img, c["mesh"])
    t.SetParameters(R.flat_parameters(c["coef"]))
    ctx = runtime.context(dev)
    x = R.flat_parameters(c["coef"]).astype(np.float64)
    keep = [None if c["jit"] is None else on(c["jit"]), on(d["grad"]), on(d["packed"])]
    try:
        if c["jit"] is not None:
            ctx.set_sample_jitter(keep[0])
        if c["source"]:
            ctx.set_moving_gradient(keep[1], packed=keep[2] if c["source"] == "packed" else None)
        jb = 0.0 if c["jit"] is None else float(np.abs(c["jit"]).max())
        ms = _BSplineMetric(ctx, None, f_img, m_img, f_img.geom(), c["stride"], t, fm, mm, jb, mi_bins=c["nbins"])
        for k_ in ("f_bin", "f_norm_min", "m_bin", "m_norm_min"):                   # the level's bins: the range inside the masks
            assert getattr(ms.bins, k_) == c["b"][k_]
        alone = ms.value(x)                                                         # histogram pass only
        assert ms.last is None and ms.evaluations == 1
        v, g = ms.value_and_gradient(x)
        assert v == alone                                                           # bit for bit
        assert ms.value(x) == v and ms.evaluations == 2                             # ... and cached
        ms2 = _BSplineMetric(ctx, None, f_img, m_img, f_img.geom(), c["stride"], t, fm, mm, jb, mi_bins=c["nbins"])
        assert ms2.value_and_gradient(x)[0] == v and ms2.value(x) == v
        hist, _ = ctx.bspline_mi_histogram(ms.ft, ms.fg, ms.mt, ms.mg, ms.vg, ms.stride, ms.coefficients(x), ms.lg, ms.bins, ms.fmask, ms.mmask, jb)
    finally:
        ctx.set_sample_jitter(None)
        ctx.set_moving_gradient(None)
    b = c["b"]
    want_v, _ = RM.value_and_table(c["hist"], float(c["s"].stats["valid"]), b["m_bin"])
    vb = RM.value_bound(c["hist"], c["hbound"])
    print(f"{name}: value {v:.12g} / {want_v:.12g}, bound {vb:.3e}")
    assert abs(v - want_v) <= vb
    # the gradient pass ran on the table of the KERNEL's histogram (held to its bound above and in test 1): restate it from there
    _, table = RM.value_and_table(hist, float(c["s"].stats["valid"]), b["m_bin"])
    want_g, gbound, _ = RM.gradient(c["s"], b, table)
    excess = np.abs(g - want_g) - gbound
    print(f"{name}: max |g| = {np.abs(want_g).max():.3e}, max |g - want| = {np.abs(g - want_g).max():.3e}, worst excess {excess.max():.3e}")
    assert np.all(excess <= 0.0)
    assert np.abs(want_g).max() > 0 or c["nbins"] == 5       # 5 bins leave ONE fixed bin: P = PM, the value and the table are 0


# ---- 4. the yardstick ----------------------------------------------------------------------------------------------------


def test_restated_gradient_against_central_differences():
    """CPU only: checks the yardstick, not the product."""
    d = _inputs()
    lat = R.initializer(SIZE, SPACING, ORIGIN, EYE, MESH_A)
    cx, cy, cz = (int(s) for s in lat["lattice_size"])
    coef = np.random.default_rng(31).normal(0, 1.5, size=(3, cz, cy, cx))
    fg = (SIZE, SPACING, ORIGIN, np.eye(3))
    b = RM.bins(30, d["fixed"], d["moving"], d["fmask"], d["mmask"])
    args = (d["fixed"], fg, d["moving"], MOVING, fg, 2)
    kw = dict(nbins=30, fixed_mask=d["fmask"], moving_mask=d["mmask"], jitter=d["jitter"][2], bins_of=b)
    _, g, _ = RM.metric(*args, coef, lat, **kw)
    big = np.nonzero(np.abs(g) > 1e-2 * np.abs(g).max())[0]
    h = 1e-4
    for p in np.random.default_rng(41).choice(big, size=10, replace=False):
        plus, minus = coef.copy().reshape(-1), coef.copy().reshape(-1)
        plus[p] += h
        minus[p] -= h
        vp = RM.metric(*args, plus.reshape(coef.shape), lat, **kw)[0]
        vm = RM.metric(*args, minus.reshape(coef.shape), lat, **kw)[0]
        np.testing.assert_allclose((vp - vm) / (2 * h), g[p], rtol=1e-5)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------


def test_refusals_leave_the_outputs_alone(backend):
    c, d = _case("A-s2-jit-packed-masks-30"), _inputs()
    lib, h, ptr = backend.lib, backend.ctx.h, _lib.ptr
    dp = C.POINTER(C.c_double)
    SENTINEL = -12345.678
    geom = _lib.make_geom(SIZE, SPACING, ORIGIN, EYE)
    mgeom = _lib.make_geom(*MOVING[:3], MOVING[3].ravel())
    keep = [backend.dev(d["fixed"]), backend.dev(d["moving"]), backend.dev(c["coef"]), backend.dev(4.0 * c["jit"])]       # jitter up to 5 voxels
    ncoef = c["coef"].size
    table = np.ascontiguousarray(c["table"])

    def both(nbins=30, kernel=_lib.MI_MATTES, lat=c["lat"], jitter_bound=float(np.abs(4.0 * c["jit"]).max()), moving_geom=mgeom, stride=2):
        b = _mibins(dict(c["b"], nbins=nbins), kernel)
        out = []
        hist, st = np.full(65 * 65, SENTINEL), np.full(4, SENTINEL)
        rc = lib.pp_bspline_mi_histogram_f32(h, ptr(keep[0]), C.byref(geom), ptr(keep[1]), C.byref(moving_geom), C.byref(geom), stride, None, None,
                                             ptr(keep[2]), C.byref(_lat_geom(lat)), jitter_bound, C.byref(b), hist.ctypes.data_as(dp),
                                             st.ctypes.data_as(dp))
        out.append((rc, np.concatenate([hist, st])))
        tab = np.zeros(65 * 65)
        tab[:table.size] = table.ravel()
        grad, st = np.full(ncoef, SENTINEL), np.full(4, SENTINEL)
        rc = lib.pp_bspline_mi_gradient_f32(h, ptr(keep[0]), C.byref(geom), ptr(keep[1]), C.byref(moving_geom), C.byref(geom), stride, None, None,
                                            ptr(keep[2]), C.byref(_lat_geom(lat)), jitter_bound, C.byref(b), tab.ctypes.data_as(dp),
                                            st.ctypes.data_as(dp), grad.ctypes.data_as(dp))
        out.append((rc, np.concatenate([grad, st])))
        return out

    flipped = R.initializer(SIZE, SPACING, ORIGIN, FLIP, MESH_A)
    far = _lib.make_geom(MOVING[0], MOVING[1], (5000.0, 0.0, 0.0), MOVING[3].ravel())
    try:
        backend.ctx.set_sample_jitter(keep[3])
        refused = {"4 bins": both(nbins=4), "65 bins": both(nbins=65), "joint kernel": both(kernel=_lib.MI_JOINT), "stride 0": both(stride=0),
                   "direction": both(lat=flipped), "jitter beyond its bound": both(jitter_bound=0.5), "negative bound": both(jitter_bound=-1.0),
                   "no overlap": both(moving_geom=far)}
        for what, pair in refused.items():
            for rc, res in pair:
                assert rc != 0 and np.all(res == SENTINEL), (what, rc)
        assert [rc for rc, _ in refused["direction"]] == [_lib.ERR_DIRECTION] * 2
        assert [rc for rc, _ in refused["no overlap"]] == [_lib.ERR_NO_OVERLAP] * 2
        for rc, res in both():          # ... and the context still works
            assert rc == 0 and not np.any(res[-4:] == SENTINEL) and res[-1] == (np.prod(SIZE) + 1) // 2
    finally:
        backend.ctx.set_sample_jitter(None)
    lat = c["lat"]
    for fn, extra in ((backend.ctx.bspline_mi_histogram, ()), (backend.ctx.bspline_mi_gradient, (table,))):
        with pytest.raises(ValueError):     # a mask of another size never reaches the kernel
            fn(keep[0], geom, keep[1], mgeom, geom, 1, keep[2], _lat_geom(lat), _mibins(c["b"]), *extra, fixed_mask=backend.dev(d["mmask"]))


# ---- 6. end to end -------------------------------------------------------------------------------------------------------


def _mi_pair():
    """test_bspline's pair (geometry, label, known B-spline of at most 3 mm) with a fine texture on the fixed image and the moving
    image as another modality would show it: inverted and rescaled.  Without the texture the smooth blobs leave 20 unregularised
    L-BFGS-B iterations free to raise the mutual information by pushing border samples out of the moving buffer (coefficients of
    20 mm, Dice 0.50 against 0.82 before -- in the product and in the restated optimiser alike); the voxels the pull-back cannot
    reach get the image's mean."""
    if "e2e" not in _SHARED:
        from scipy.ndimage import gaussian_filter

        from tests.test_bspline import E2E_SIZE, E2E_SPACING, _e2e_pair

        _, label, _, moving_label, geom = _e2e_pair()
        shape = E2E_SIZE[::-1]
        texture = gaussian_filter(np.random.default_rng(53).normal(0, 60.0, size=shape), 1.0)
        fixed = (gaussian_filter(R.blobs(shape, 51).astype(np.float64), 1.0) + texture).astype(np.float32)
        lat = R.initializer(E2E_SIZE, E2E_SPACING, (0, 0, 0), np.eye(3), (2, 2, 2))
        rng = np.random.default_rng(52)      # the coefficients _e2e_pair moved its label with
        true = np.stack([rng.uniform(1.5, 3.0, size=(5, 5, 5)), rng.uniform(-3.0, -1.0, size=(5, 5, 5)), rng.uniform(-3.0, 3.0, size=(5, 5, 5))])
        moving = (300.0 - 1.2 * R.warp_linear(fixed, geom, true, lat, default=float(fixed.mean()))).astype(np.float32)
        _SHARED["e2e"] = (fixed, label, moving, moving_label, geom)
    return _SHARED["e2e"]


def test_registration_against_restated_optimiser(host_api):
    from scipy.optimize import fmin_l_bfgs_b

    from tests.helpers import dice
    from tests.test_bspline import E2E_SIZE, E2E_SPACING

    pa = host_api
    fixed, label, moving, moving_label, geom = _mi_pair()
    f_img, m_img = pa.Image(fixed, E2E_SPACING), pa.Image(moving, E2E_SPACING)
    kw = dict(resolution_staging=[1], smooth_sigmas=[0], grid_scale_factors=[1], initial_grid_spacing=24, sampling_rate=1.0, itk_sampling=False,
              optimiser="lbfgsb", number_of_iterations=20)
    out, t = pa.registration.bspline_registration(f_img, m_img, metric="mattes_mi", **kw)
    mesh = tuple(R.control_point_spacing_distance_to_number(E2E_SIZE, E2E_SPACING, 24))
    assert tuple(t.GetTransformDomainMeshSize()) == mesh
    lat = R.initializer(E2E_SIZE, E2E_SPACING, (0, 0, 0), np.eye(3), mesh)
    shape = (3,) + tuple(int(s) for s in lat["lattice_size"][::-1])
    b = RM.bins(30, fixed, moving)

    def fun(x):
        v, g, _ = RM.metric(fixed, geom, moving, geom, geom, 1, x.reshape(shape), lat, 30, bins_of=b)
        return v, g

    x0 = np.zeros(int(np.prod(shape)))
    want_first = fun(x0)[0]
    x, _, _ = fmin_l_bfgs_b(fun, x0, m=5, factr=1e7, pgtol=1e-5, maxiter=20, maxfun=1024)
    want_final = fun(x)[0]
    first, last = t.level_values[0]
    print(f"end to end: initial {first:.6f} / {want_first:.6f}, product final {last:.6f}, restated optimiser final {want_final:.6f}")
    np.testing.assert_allclose(first, want_first, rtol=1e-5)
    assert last < first
    assert first - last >= 0.90 * (want_first - want_final)      # the value is negative: the 10 % apply to the decrease
    apply = lambda tr: pa.registration.apply_transform(pa.Image(moving_label, E2E_SPACING), f_img, tr, 0, pa.sitkNearestNeighbor).numpy()      # noqa: E731
    before, after = dice(moving_label, label), dice(apply(t), label)
    _, t_ms = pa.registration.bspline_registration(f_img, m_img, metric="mean_squares", **kw)
    after_ms = dice(apply(t_ms), label)
    print(f"Dice before {before:.4f}, mattes_mi {after:.4f}, mean_squares {after_ms:.4f}")
    assert after > before
    assert after_ms < after                                       # mean squares cannot register an inverted image


def test_registration_three_levels(host_api):
    from tests.test_bspline import E2E_SPACING

    pa = host_api
    fixed, _, moving, _, _ = _mi_pair()
    _, t = pa.registration.bspline_registration(pa.Image(fixed, E2E_SPACING), pa.Image(moving, E2E_SPACING), metric="mattes_mi",
                                                initial_grid_spacing=24)
    assert len(t.level_values) == 3
    for first, last in t.level_values:
        assert np.isfinite(first) and last <= first


# ---- 7. signature --------------------------------------------------------------------------------------------------------


def test_signature(host_api):
    pa = host_api
    img = pa.Image(R.blobs((8, 9, 10), 1), (2.0, 2.0, 2.0))
    reg = pa.registration.bspline_registration
    _, t = reg(img, img, metric="mattes_mi", resolution_staging=[1], smooth_sigmas=[0], grid_scale_factors=[1], initial_grid_spacing=12,
               sampling_rate=1.0, itk_sampling=False, optimiser="lbfgsb", number_of_iterations=1, number_of_histogram_bins_mi=8)
    assert len(t.level_values) == 1
    for nbins in (4, 65):
        with pytest.raises(ValueError, match="5..64"):
            reg(img, img, metric="mattes_mi", number_of_histogram_bins_mi=nbins)
    reg(img, img, metric="mean_squares", number_of_histogram_bins_mi=4, resolution_staging=[1], smooth_sigmas=[0], grid_scale_factors=[1],
        initial_grid_spacing=12, number_of_iterations=1)      # ignored for the other metrics, as before
    with pytest.raises(NotImplementedError, match="mattes_mi"):
        reg(img, img, metric="mutual_information")
