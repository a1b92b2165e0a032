"""The B-spline kernels of platipy_amd/csrc/pp_bspline.h at the geometries bspline_registration hands them, held to fp64
restatements with derived bounds:

  1. the bounded restatement of mean squares and correlation (tests/bspline_kernel_restatement.py, RK) against the
     unbounded one of tests/bspline_restatement.py -- CPU only;
  2. all four entry points (pp_bspline_metric_f32 with both metrics, pp_bspline_mi_histogram_f32, pp_bspline_mi_gradient_f32)
     over virtual grids that are not the fixed image's (shrunk by ITK's rule, grown, refined), long strides, every kind of
     z-slab split (bsp_metric_prepare: nsplit = min(16, ceil(1024 / cells)) below 1024 cells, else 1), cells narrower than the
     stride or than a voxel, empty slabs, and jitter wider than a cell;
  3. single-sample probes on a dyadic geometry: a mask leaves one voxel, so a sample sent to the wrong cell or weighted for
     the wrong control point changes WHICH entries are non-zero, whatever the tolerance;
  4. the field kernels (k_bsp_tables, k_bsp_field<true / false>) with voxel centres exactly on the domain's edges, on a grid
     turned by 90 degrees, around the switch between the table path and the per-voxel path, and at tiny grids;
  5. the refusals of pp_bspline_metric_f32, which leave value, stats and gradient as the caller had them.

Out of scope: the grid-stride loop of k_bsp_field is only entered above 2^28 voxels (its grid is capped at 2^20 workgroups of
256 threads); an output of 3 GB is no test for this suite.
"""
import ctypes as C

import numpy as np
import pytest

from platipy_amd import _lib
from tests import bspline_kernel_restatement as RK
from tests import bspline_mi_restatement as RM
from tests import bspline_restatement as R
from tests import test_bspline as TB
from tests import test_bspline_mi as TM

SIZE, SPACING, ORIGIN, MOVING = TB.SIZE, TB.SPACING, TB.ORIGIN, TB.MOVING
EYE, FLIP = TB.EYE, TB.FLIP
_SHARED = {}


def _geom(g):
    return _lib.make_geom(g[0], g[1], g[2], np.ravel(g[3]))


def _lat_geom(lat):
    return _lib.make_geom(lat["lattice_size"], lat["lattice_spacing"], lat["lattice_origin"], lat["direction"].ravel())


def _coef(lat, seed, sigma):
    cx, cy, cz = (int(s) for s in lat["lattice_size"])
    return np.random.default_rng(seed).normal(0, sigma, size=(3, cz, cy, cx)).astype(np.float32)


def _mibins(b):
    m = _lib.MiBins()
    m.nbins, m.kernel, m.f_bin, m.f_norm_min, m.m_bin, m.m_norm_min = b["nbins"], _lib.MI_MATTES, b["f_bin"], b["f_norm_min"], b["m_bin"], b["m_norm_min"]
    return m


class _Call:
    """the buffers of one evaluation on the backend and the three entry points on them; jitter and gradient source are
    installed on the context for the length of a call"""

    def __init__(self, backend, fixed, fgeom, moving, mgeom, vgeom, stride, coef, lat, fmask=None, mmask=None, jitter=None, source=None,
                 grad=None, packed=None):
        dev = lambda a: None if a is None else backend.dev(a)        # noqa: E731
        self.ctx, self.source = backend.ctx, source
        self.fixed, self.moving, self.coef, self.jit = dev(fixed), dev(moving), dev(coef), dev(jitter)
        self.fmask, self.mmask = dev(fmask), dev(mmask)
        self.grad, self.packed = (dev(grad), dev(packed)) if source else (None, None)
        self.args = (self.fixed, _geom(fgeom), self.moving, _geom(mgeom), _geom(vgeom), int(stride), self.coef, _lat_geom(lat))
        self.jitter_bound = 0.0 if jitter is None else float(np.abs(jitter).max())

    def set_fixed_mask(self, backend, fmask):
        self.fmask = backend.dev(fmask)

    def _run(self, fn):
        try:
            if self.jit is not None:
                self.ctx.set_sample_jitter(self.jit)
            if self.source == "packed":
                self.ctx.set_moving_gradient(self.grad, packed=self.packed)
            elif self.source == "planar":
                self.ctx.set_moving_gradient(self.grad)
            return fn()
        finally:
            self.ctx.set_sample_jitter(None)
            self.ctx.set_moving_gradient(None)

    def metric(self, kind):
        code = _lib.BSPLINE_MEAN_SQUARES if kind == "mean_squares" else _lib.BSPLINE_CORRELATION
        return self._run(lambda: self.ctx.bspline_metric(code, *self.args, self.fmask, self.mmask, self.jitter_bound))

    def histogram(self, b):
        return self._run(lambda: self.ctx.bspline_mi_histogram(*self.args, _mibins(b), self.fmask, self.mmask, self.jitter_bound))

    def gradient(self, b, table):
        return self._run(lambda: self.ctx.bspline_mi_gradient(*self.args, _mibins(b), table, self.fmask, self.mmask, self.jitter_bound))


def _mi_gradient(s, b, table):
    """RM.gradient, its bound completed where the weight product leaves fp32's normal range (RK.underflow_floor; a sample's
    score derivative is at most 4 max|B3'| max|table| = 8 / 3 max|table|)"""
    want, bound, q = RM.gradient(s, b, table)
    return want, bound + RK.underflow_floor(s, 8.0 / 3.0 * np.abs(table).max() * (np.abs(s.gp) + s.egp)), q


def _report(entry, name, err, bound, scale):
    """prints the worst err / bound and how tight the bound is; -> nothing.  A zero bound admits a zero error only."""
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"RATIO {entry} {name}: worst err / bound = {ratio:.3f}, bound.max() / scale = {bound.max() / scale:.3e}, max err = {err.max():.3e}")


# ---- 1. the yardstick ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("metric,mesh,stride,jitter,packed,masks", TB.CASES)
def test_bounded_restatement_against_the_unbounded_one(metric, mesh, stride, jitter, packed, masks):
    """CPU only: checks the yardstick, not the product.  RK goes through scipy's interpolator (RM.Samples), R.metric through
    eight gathered corners."""
    d = TB._metric_inputs()
    lat = TB._lattice(mesh)
    coef = TB._coef(lat, 31, 1.5)
    fg = (SIZE, SPACING, ORIGIN, np.eye(3))
    jit = d["jitter"][stride] if jitter else None
    fm, mm = (d["fmask"], d["mmask"]) if masks else (None, None)
    grad = d["grad"] if packed else None
    want_v, want_g, want_s = R.metric(metric, d["fixed"], fg, d["moving"], MOVING, fg, stride, coef, lat, fm, mm, jit, grad)
    s = RM.Samples(d["fixed"], fg, d["moving"], MOVING, fg, stride, coef, lat, fm, mm, jit, grad)
    value, g, value_bound, bound = RK.metric(metric, s)
    assert s.stats == want_s
    gmax = np.abs(want_g).max()
    assert np.abs(g - want_g).max() <= 1e-12 * gmax
    assert abs(value - want_v) <= 1e-12 * abs(want_v)
    assert 0 < value_bound < np.inf
    assert np.all(bound >= 0) and bound.max() <= 2e-4 * gmax      # tighter than the atol of 1e-3 max|g| the old test allows


# ---- 2. geometry matrix --------------------------------------------------------------------------------------------------

MESH_A, MESH_C = (3, 2, 2), (11, 9, 11)
GEOMETRY = {
    # mesh, virtual grid (a function of the fixed grid), stride, nsplit it reaches, then: jitter, masks, gradient source, bins, flipped
    "A-shrink2-s3": dict(mesh=MESH_A, grid=lambda g: RK.shrunk(g, 2), vsize=(16, 13, 10), stride=3, nsplit=16, bins=30),
    "A-shrink2-s3-flipped-packed": dict(mesh=MESH_A, grid=lambda g: RK.shrunk(g, 2), vsize=(16, 13, 10), stride=3, nsplit=16, bins=64, flipped=True,
                                        source="packed"),
    "A-shrink221-s10-planar": dict(mesh=MESH_A, grid=lambda g: RK.shrunk(g, (2, 2, 1)), vsize=(16, 13, 20), stride=10, nsplit=16, bins=30,
                                   source="planar"),
    "888-s7": dict(mesh=(8, 8, 8), grid=None, stride=7, nsplit=2, bins=64),
    "888-s7-masks-packed": dict(mesh=(8, 8, 8), grid=None, stride=7, nsplit=2, bins=30, masks=True, source="packed"),
    "777-shrink3-s1": dict(mesh=(7, 7, 7), grid=lambda g: RK.shrunk(g, 3), vsize=(11, 9, 6), stride=1, nsplit=3, bins=5),
    "555-s10": dict(mesh=(5, 5, 5), grid=None, stride=10, nsplit=9, bins=30),
    "555-s10-masks-planar": dict(mesh=(5, 5, 5), grid=None, stride=10, nsplit=9, bins=64, masks=True, source="planar"),
    "C-s7": dict(mesh=MESH_C, grid=None, stride=7, nsplit=1, bins=30),
    "A25-s3": dict(mesh=(3, 2, 25), grid=None, stride=3, nsplit=7, bins=64),
    "A25-s3-masks": dict(mesh=(3, 2, 25), grid=None, stride=3, nsplit=7, bins=30, masks=True),
    "A-grown-s5": dict(mesh=MESH_A, grid=lambda g: RK.grown(g, 3), vsize=(39, 33, 26), stride=5, nsplit=16, bins=30),
    "C-grown-s2-packed": dict(mesh=MESH_C, grid=lambda g: RK.grown(g, 3), vsize=(39, 33, 26), stride=2, nsplit=1, bins=5, source="packed",
                              mi_fixed_seed=63),      # stride 2 on this grid visits the brightest voxel of test_bspline_mi's fixed image: a bin edge
    "555-fine-s9": dict(mesh=(5, 5, 5), grid=RK.refined, vsize=(66, 54, 40), stride=9, nsplit=9, bins=30),
    "C-s1-jit": dict(mesh=MESH_C, grid=None, stride=1, nsplit=1, bins=30, jitter=True),
    "A-s10-jit": dict(mesh=MESH_A, grid=None, stride=10, nsplit=16, bins=30, jitter=True),
    "555-s3-jit-planar": dict(mesh=(5, 5, 5), grid=None, stride=3, nsplit=9, bins=30, jitter=True, source="planar"),
}
GEOMETRY_IDS = list(GEOMETRY)
JITTER = 3.7        # voxels, uniform: margin ceil(3.7) + 1 = 5, wider than a cell of MESH_C


def _geometry_case(name):
    """geometry and inputs of a case and its sample sets on the two image pairs (test_bspline's for mean squares and
    correlation, test_bspline_mi's for the two mutual-information passes): computed once, shared, never written to"""
    key = ("geometry", name)
    if key not in _SHARED:
        spec = GEOMETRY[name]
        flipped = spec.get("flipped", False)
        direction = FLIP if flipped else EYE
        origin = (ORIGIN[0] + (SIZE[0] - 1) * SPACING[0], ORIGIN[1], ORIGIN[2]) if flipped else ORIGIN
        fg = (SIZE, SPACING, origin, np.reshape(direction, (3, 3)))
        lat = R.initializer(SIZE, SPACING, origin, direction, spec["mesh"])
        coef = _coef(lat, 31, 1.5)
        vg = fg if spec["grid"] is None else spec["grid"](fg)
        assert tuple(vg[0]) == tuple(spec.get("vsize", SIZE))
        ncells = int(np.prod(spec["mesh"]))
        assert spec["nsplit"] == (min(16, -(-1024 // ncells)) if ncells < 1024 else 1)
        stride = spec["stride"]
        nsamp = -(-int(np.prod(vg[0])) // stride)
        jit = None
        if spec.get("jitter"):
            jit = np.random.default_rng(71).uniform(-JITTER, JITTER, size=(nsamp, 3)).astype(np.float32)
        c = dict(spec=spec, fg=fg, vg=vg, lat=lat, coef=coef, stride=stride, nsamp=nsamp, jit=jit, source=spec.get("source"))
        mi = TM._inputs()
        if "mi_fixed_seed" in spec:
            mi = dict(mi, fixed=R.blobs(SIZE[::-1], spec["mi_fixed_seed"], noise=3.0))
        for pair, d in (("ms", TB._metric_inputs()), ("mi", mi)):
            fm, mm = (d["fmask"], d["mmask"]) if spec.get("masks") else (None, None)
            s = RM.Samples(d["fixed"], fg, d["moving"], MOVING, vg, stride, coef, lat, fm, mm, jit, d["grad"] if c["source"] else None)
            c[pair] = dict(d=d, fm=fm, mm=mm, s=s)
        m = c["mi"]
        m["b"] = RM.bins(spec["bins"], m["d"]["fixed"], m["d"]["moving"], m["fm"], m["mm"])
        m["hist"], m["hbound"], q = RM.histogram(m["s"], m["b"])
        m["amb"] = int(q.amb_f.sum())
        m["table"] = np.random.default_rng(47).normal(0, 1.0, size=(spec["bins"], spec["bins"]))      # any table: pass 2 is linear in it
        _SHARED[key] = c
    return _SHARED[key]


def _call(backend, c, pair):
    p = c[pair]
    d = p["d"]
    return _Call(backend, d["fixed"], c["fg"], d["moving"], MOVING, c["vg"], c["stride"], c["coef"], c["lat"], p["fm"], p["mm"], c["jit"],
                 c["source"], d["grad"], d["packed"])


def _check_samples(c, pair):
    """conditions on the restatement alone, before any kernel runs"""
    st = c[pair]["s"].stats
    assert st["seen"] == c["nsamp"]
    assert st["valid"] >= 300
    assert st["outside"] > 0
    if c["spec"].get("masks"):
        assert st["masked"] > 0
    if pair == "mi":        # test_bspline_mi._check_ambiguity's rule without its floor of 1000 valid samples
        assert c["mi"]["amb"] <= 1 + st["valid"] // 20000
        if st["seen"] < 20000:
            assert c["mi"]["amb"] == 0


def _as_floats(stats):
    return {k: float(v) for k, v in stats.items()}


@pytest.mark.parametrize("metric", ["mean_squares", "correlation"])
@pytest.mark.parametrize("name", GEOMETRY_IDS)
def test_metric_kernel_geometries(backend, name, metric):
    c = _geometry_case(name)
    _check_samples(c, "ms")
    s = c["ms"]["s"]
    want_v, want_g, vbound, bound = RK.metric(metric, s)
    gmax = np.abs(want_g).max()
    assert gmax > 0 and bound.max() <= 2e-4 * gmax
    k = _call(backend, c, "ms")
    v1, g1, s1 = k.metric(metric)
    v2, g2, s2 = k.metric(metric)
    assert v1 == v2 and np.array_equal(g1, g2) and s1 == s2                       # bit-identical between calls
    assert s1 == _as_floats(s.stats)
    err = np.abs(g1 - want_g)
    _report(metric, name, err, bound, gmax)
    print(f"value {v1:.12g} / {want_v:.12g}, |difference| / bound = {abs(v1 - want_v) / vbound:.3f}")
    assert np.all(err <= bound)
    assert abs(v1 - want_v) <= vbound
    assert np.all(g1[RM.outside_support(s)] == 0.0)


@pytest.mark.parametrize("name", GEOMETRY_IDS)
def test_mi_histogram_kernel_geometries(backend, name):
    c = _geometry_case(name)
    _check_samples(c, "mi")
    m = c["mi"]
    k = _call(backend, c, "mi")
    h1, s1 = k.histogram(m["b"])
    h2, s2 = k.histogram(m["b"])
    assert np.array_equal(h1, h2) and s1 == s2
    assert s1 == _as_floats(m["s"].stats)
    np.testing.assert_allclose(h1.sum(), m["s"].stats["valid"], rtol=1e-9)        # the four weights of a sample sum to one
    err = np.abs(h1 - m["hist"])
    _report("mi_histogram", name, err, m["hbound"], 1.0)
    assert np.all(err <= m["hbound"])


@pytest.mark.parametrize("name", GEOMETRY_IDS)
def test_mi_gradient_kernel_geometries(backend, name):
    c = _geometry_case(name)
    _check_samples(c, "mi")
    m = c["mi"]
    want, bound, _ = _mi_gradient(m["s"], m["b"], m["table"])
    gmax = np.abs(want).max()
    assert gmax > 0 and bound.max() <= 2e-4 * gmax
    k = _call(backend, c, "mi")
    g1, s1 = k.gradient(m["b"], m["table"])
    g2, s2 = k.gradient(m["b"], m["table"])
    assert np.array_equal(g1, g2) and s1 == s2
    assert s1 == _as_floats(m["s"].stats)
    err = np.abs(g1 - want)
    _report("mi_gradient", name, err, bound, gmax)
    assert np.all(err <= bound)
    assert np.all(g1[RM.outside_support(m["s"])] == 0.0)


# ---- 3. single-sample probes ---------------------------------------------------------------------------------------------

P_SIZE = (16, 8, 12)
P_FG = (P_SIZE, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), np.eye(3))
P_MG = (tuple(n + 8 for n in P_SIZE), (1.0, 1.0, 1.0), (-4.0, -4.0, -4.0), np.eye(3))
P_MESHES = [(4, 2, 3), (1, 1, 1)]       # cells of 4 voxels with their faces between voxels (x = 3|4, 7|8, 11|12; y = 3|4; z = 3|4, 7|8); one cell


def _probe_images():
    """small-integer ramps: the interpolation is good to a few ulp of ~250 and f - m is far from 0"""
    if "probe" not in _SHARED:
        zz, yy, xx = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in P_SIZE[::-1]), indexing="ij")
        fixed = (3 * xx - 2 * yy - 5 * zz).astype(np.float32)
        zz, yy, xx = np.meshgrid(*(np.arange(n, dtype=np.float64) - 4.0 for n in P_MG[0][::-1]), indexing="ij")
        moving = (100 + 2 * xx + 3 * yy - 4 * zz + 0.25 * xx * yy).astype(np.float32)
        _SHARED["probe"] = (fixed, moving)
    return _SHARED["probe"]


def _probe_voxels(stride):
    """the two corners; both voxels next to every interior cell face of mesh (4, 2, 3) on each axis; every z of a column (each
    z slab of a cell's box holds one z at this size) -- those the stride visits, the other two coordinates moved until it does
    and until the voxel's intensity, an integer, is no edge of the 26 inner fixed bins (RM.bins with 30)"""
    nx, ny, nz = P_SIZE
    fixed = _probe_images()[0].astype(np.float64)
    width = (fixed.max() - fixed.min()) / 26.0

    def visited(x, y, z):
        tf = (fixed[z, y, x] - fixed.min()) / width
        return ((z * ny + y) * nx + x) % stride == 0 and abs(tf - round(tf)) > 1e-3

    want = [(0, 0, 0), (nx - 1, ny - 1, nz - 1)]
    out = [v for v in want if visited(*v)]
    rng = np.random.default_rng(5)
    for axis, values in ((0, (3, 4, 7, 8, 11, 12)), (1, (3, 4)), (2, tuple(range(nz)))):
        for val in values:
            for _ in range(64):
                v = [int(rng.integers(0, n)) for n in P_SIZE]
                v[axis] = val
                if visited(*v):
                    out.append(tuple(v))
                    break
            else:
                raise AssertionError("no visited voxel")
    return out


def _support_pattern(s):
    return ~RM.outside_support(s)


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("mesh", P_MESHES)
def test_single_sample_probes(backend, mesh, stride):
    fixed, moving = _probe_images()
    lat = R.initializer(*P_FG[:3], EYE, mesh)
    coef = _coef(lat, 83, 0.7)
    b = RM.bins(30, fixed, moving)
    table = np.random.default_rng(47).normal(0, 1.0, size=(30, 30))
    k = _Call(backend, fixed, P_FG, moving, P_MG, P_FG, stride, coef, lat, fmask=np.zeros(P_SIZE[::-1], dtype=np.uint8))
    probes = _probe_voxels(stride)
    assert len(probes) >= 20
    worst = {"mean_squares": 0.0, "mi_gradient": 0.0}
    for x, y, z in probes:
        fmask = np.zeros(P_SIZE[::-1], dtype=np.uint8)
        fmask[z, y, x] = 1
        s = RM.Samples(fixed, P_FG, moving, P_MG, P_FG, stride, coef, lat, fmask)
        assert s.stats["valid"] == 1 and s.stats["outside"] == 0 and s.inside.all()      # no probe leaves the moving buffer
        assert abs(s.f[0] - s.m[0]) > 20
        pattern = _support_pattern(s)
        assert pattern.sum() == 192
        k.set_fixed_mask(backend, fmask)
        # mean squares: the entries that are not zero, then their values
        _, want, _, _ = RK.mean_squares(s)
        assert np.all(want[pattern] != 0.0)
        v, g, st = k.metric("mean_squares")
        assert st == _as_floats(s.stats), (x, y, z)
        assert np.array_equal(g != 0.0, pattern), (x, y, z)
        gmax = np.abs(want).max()
        worst["mean_squares"] = max(worst["mean_squares"], np.abs(g - want).max() / gmax)
        assert np.abs(g - want).max() <= 1e-5 * gmax, (x, y, z)
        # pass 2 of mutual information
        want, bound, q = _mi_gradient(s, b, table)
        assert not q.amb_f.any() and np.all(want[pattern] != 0.0)
        g, st = k.gradient(b, table)
        assert st == _as_floats(s.stats), (x, y, z)
        assert np.array_equal(g != 0.0, pattern), (x, y, z)
        err = np.abs(g - want)
        worst["mi_gradient"] = max(worst["mi_gradient"], (err[pattern] / bound[pattern]).max())
        assert np.all(err <= bound), (x, y, z)
    print(f"RATIO probes mesh {mesh} stride {stride}: {len(probes)} probes, mean squares worst err / max|g| = {worst['mean_squares']:.3e}, "
          f"mi_gradient worst err / bound = {worst['mi_gradient']:.3f}")


@pytest.mark.parametrize("stride", [1, 3])
def test_three_sample_probes_correlation(backend, stride):
    """correlation needs a variance: each probe is joined by two voxels of other cells whose intensities are well apart"""
    mesh = P_MESHES[0]
    fixed, moving = _probe_images()
    lat = R.initializer(*P_FG[:3], EYE, mesh)
    coef = _coef(lat, 83, 0.7)
    k = _Call(backend, fixed, P_FG, moving, P_MG, P_FG, stride, coef, lat, fmask=np.zeros(P_SIZE[::-1], dtype=np.uint8))
    nx, ny, nz = P_SIZE
    visited = [(x, y, z) for z in range(nz) for y in range(ny) for x in range(nx) if ((z * ny + y) * nx + x) % stride == 0]
    cell = lambda v: (v[0] // 4, v[1] // 4, v[2] // 4)        # noqa: E731
    rng = np.random.default_rng(6)
    worst, disjoint = 0.0, 0
    for p in _probe_voxels(stride):
        trio = [p]
        for _ in range(1000):
            v = visited[int(rng.integers(0, len(visited)))]
            if all(cell(v) != cell(t) and abs(float(fixed[v[2], v[1], v[0]]) - float(fixed[t[2], t[1], t[0]])) >= 10 for t in trio):
                trio.append(v)
                if len(trio) == 3:
                    break
        assert len(trio) == 3
        fmask = np.zeros(P_SIZE[::-1], dtype=np.uint8)
        for x, y, z in trio:
            fmask[z, y, x] = 1
        s = RM.Samples(fixed, P_FG, moving, P_MG, P_FG, stride, coef, lat, fmask)
        assert s.stats["valid"] == 3 and s.inside.all()
        pattern = _support_pattern(s)
        want_v, want, vbound, bound = RK.correlation(s)
        assert np.all(want[pattern] != 0.0)
        if pattern.sum() == 3 * 192:
            disjoint += 1
        k.set_fixed_mask(backend, fmask)
        v, g, st = k.metric("correlation")
        assert st == _as_floats(s.stats), trio
        assert np.array_equal(g != 0.0, pattern), trio
        err = np.abs(g - want)
        worst = max(worst, (err[pattern] / bound[pattern]).max())
        assert np.all(err <= bound), trio
        assert abs(v - want_v) <= vbound, trio
    print(f"RATIO probes correlation stride {stride}: worst err / bound = {worst:.3f}, {disjoint} trios with disjoint supports")


# ---- 4. field kernel edges -----------------------------------------------------------------------------------------------

F_MESH = (4, 2, 3)      # domain [-0.5, 15.5) x [-0.5, 7.5) x [-0.5, 11.5), lattice spacing 4: every coordinate below is exact in fp64


def _field(backend, coef, lat, grid):
    out = backend.empty((3, grid[0][2], grid[0][1], grid[0][0]))
    backend.ctx.bspline_field(backend.dev(coef), _lat_geom(lat), _geom(grid), out)
    return backend.host(out)


def _field_checks(backend, lat, grid, want_outside=True):
    """the field of random coefficients against the restatement on `grid`: the same inside set, exact zeros outside, 1e-5
    max|c| inside (the bound derived in test_bspline.test_field_kernel_against_restatement); constants within 4 ulp"""
    coef = _coef(lat, 11, 3.0)
    inside, _, _ = R.support(R.grid_points(*grid), lat)
    inside = inside.reshape(grid[0][2], grid[0][1], grid[0][0])
    assert inside.any()
    if want_outside:
        assert (~inside).any()
    got = _field(backend, coef, lat, grid)
    want = R.field(coef, lat, *grid)
    assert np.array_equal(np.any(got != 0.0, axis=0), inside)         # (a displacement of exactly 0 inside would need three zero sums)
    assert np.all(got[:, ~inside] == 0.0)
    err = np.abs(got - want).max()
    print(f"field: max |kernel - restatement| = {err:.3e}, max|c| = {np.abs(coef).max():.3f}, {int(inside.sum())} of {inside.size} inside")
    assert err <= 1e-5 * np.abs(coef).max()
    const = np.empty_like(coef)
    vals = np.array([2.71828, -13.5, 0.3], dtype=np.float32)
    const[:] = vals[:, None, None, None]
    got_c = _field(backend, const, lat, grid)
    for r in range(3):
        assert np.abs(got_c[r][inside] - vals[r]).max() <= 4 * np.spacing(np.abs(vals[r]))      # partition of unity
        assert np.all(got_c[r][~inside] == 0.0)
    return inside


def _edge_counts(inside, axes_xyz):
    """the inside set along each grid axis is one run: -> its (first, last + 1) per axis, x y z"""
    out = []
    for a in axes_xyz:
        line = inside.any(axis=tuple(k for k in range(3) if k != 2 - a))
        idx = np.nonzero(line)[0]
        assert np.array_equal(np.arange(idx[0], idx[-1] + 1), idx)
        out.append((int(idx[0]), int(idx[-1]) + 1))
    return out


def test_field_grid_on_the_domain_edges(backend):
    """spacing 0.5 from -1.5: centres fall exactly on both edges of the domain; inside at u == 1, outside at u == mesh + 1"""
    lat = R.initializer(*P_FG[:3], EYE, F_MESH)
    grid = ((37, 21, 29), (0.5, 0.5, 0.5), (-1.5, -1.5, -1.5), np.eye(3))
    inside = _field_checks(backend, lat, grid)
    # index 2 is -0.5 (inside); 15.5, 7.5, 11.5 are indices 34, 18, 26 (outside)
    assert _edge_counts(inside, (0, 1, 2)) == [(2, 34), (2, 18), (2, 26)]


def test_field_rotated_grid_on_the_domain_edges(backend):
    """the same grid turned by 90 degrees about z: the per-voxel path with exact coordinates.  Grid axis 0 runs along +y from
    -1.5, grid axis 1 along -x from 16.5."""
    lat = R.initializer(*P_FG[:3], EYE, F_MESH)
    grid = ((21, 37, 29), (0.5, 0.5, 0.5), (16.5, -1.5, -1.5), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]))
    inside = _field_checks(backend, lat, grid)
    # along -x: 16.5 - 0.5 j is 15.5 (outside) at j = 2 and -0.5 (inside) at j = 34
    assert _edge_counts(inside, (0, 1, 2)) == [(2, 18), (3, 35), (2, 26)]


@pytest.mark.parametrize("tilt", [1e-13, 3e-12, 1e-6])
def test_field_around_the_table_switch(backend, tilt):
    """off <= 1e-12 * diag chooses the table path: a tilt below it, just above it and far above it all agree with the
    restatement of the tilted grid.  The origin keeps every centre off the domain's edges, where the table path (which drops
    the tilt) and the restatement legitimately differ."""
    lat = R.initializer(*P_FG[:3], EYE, F_MESH)
    c, s = np.cos(tilt), np.sin(tilt)
    grid = ((37, 21, 29), (0.5, 0.5, 0.5), (-1.37, -1.41, -1.33), np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]))
    u = (R.grid_points(*grid) - lat["lattice_origin"][None, :]) @ np.linalg.inv(R.i2p(lat["lattice_spacing"], lat["direction"])).T
    edge = np.minimum(np.abs(u - 1.0), np.abs(u - (np.asarray(F_MESH, dtype=np.float64)[None, :] + 1.0))).min()
    assert edge >= 1e-6
    _field_checks(backend, lat, grid)


@pytest.mark.parametrize("size", [(255, 1, 1), (1, 256, 1), (1, 1, 257), (5, 3, 1)])
def test_field_small_grids(backend, size):
    """voxel counts around one workgroup of 256 threads, on a lattice of 4 x 8 x 5"""
    lat = R.initializer(*P_FG[:3], EYE, (1, 5, 2))
    assert tuple(int(k) for k in lat["lattice_size"]) == (4, 8, 5)
    # the long axis runs from 1.3 before the domain to beyond its far end; the others start inside it
    extent = (16.0, 8.0, 12.0)
    spacing = tuple((extent[a] + 3.0) / size[a] if size[a] > 5 else 1.7 for a in range(3))
    origin = tuple(-1.3 if size[a] > 1 else 2.2 for a in range(3))
    _field_checks(backend, lat, (size, spacing, origin, np.eye(3)))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------


def test_metric_refusals_leave_the_outputs_alone(backend):
    d = TB._metric_inputs()
    lib, h, ptr = backend.lib, backend.ctx.h, _lib.ptr
    dp = C.POINTER(C.c_double)
    SENTINEL = -12345.678
    lat = TB._lattice(MESH_A)
    coef = TB._coef(lat, 31, 1.5)
    geom = _lib.make_geom(SIZE, SPACING, ORIGIN, EYE)
    mgeom = _lib.make_geom(*MOVING[:3], MOVING[3].ravel())
    nsamp = int(np.prod(SIZE))
    jitter = np.zeros((nsamp, 3), dtype=np.float32)
    jitter[(10 * SIZE[1] + 13) * SIZE[0] + 8, 0] = 6.0        # voxel (8, 13, 10) of cell 0 (x < 10.5) lands in cell 1, whose box starts at x = 9
    keep = [backend.dev(d["fixed"]), backend.dev(d["moving"]), backend.dev(coef), backend.dev(jitter), backend.dev(jitter[:nsamp - 1].copy())]
    ncoef = coef.size

    def call(metric=_lib.BSPLINE_MEAN_SQUARES, lattice=lat, jitter_bound=6.0, moving_geom=mgeom, virt=geom, stride=1):
        value, st, grad = C.c_double(SENTINEL), np.full(4, SENTINEL), np.full(ncoef, SENTINEL)
        rc = lib.pp_bspline_metric_f32(h, metric, ptr(keep[0]), C.byref(geom), ptr(keep[1]), C.byref(moving_geom), C.byref(virt), stride, None, None,
                                       ptr(keep[2]), C.byref(_lat_geom(lattice)), jitter_bound, C.byref(value), st.ctypes.data_as(dp),
                                       grad.ctypes.data_as(dp))
        return rc, np.concatenate([[value.value], st, grad])

    flipped = R.initializer(SIZE, SPACING, ORIGIN, FLIP, MESH_A)
    thin = dict(lat, lattice_size=np.array([6, 3, 5]))
    far = _lib.make_geom(MOVING[0], MOVING[1], (5000.0, 0.0, 0.0), MOVING[3].ravel())
    turned = _lib.make_geom(SIZE, SPACING, ORIGIN, FLIP)
    try:
        backend.ctx.set_sample_jitter(keep[3])
        before = {m: call(metric=m) for m in (_lib.BSPLINE_MEAN_SQUARES, _lib.BSPLINE_CORRELATION)}
        for rc, res in before.values():
            assert rc == 0 and not np.any(res == SENTINEL) and res[4] == nsamp
        refused = {}
        for m in (_lib.BSPLINE_MEAN_SQUARES, _lib.BSPLINE_CORRELATION):
            refused.update({
                ("jitter beyond its bound", m): call(metric=m, jitter_bound=0.5), ("no overlap", m): call(metric=m, moving_geom=far),
                ("stride 0", m): call(metric=m, stride=0), ("negative bound", m): call(metric=m, jitter_bound=-1.0),
                ("infinite bound", m): call(metric=m, jitter_bound=float("inf")), ("3 control points", m): call(metric=m, lattice=thin),
                ("flipped lattice", m): call(metric=m, lattice=flipped), ("virtual direction", m): call(metric=m, virt=turned)})
        refused[("metric code", 2)] = call(metric=2)
        refused[("metric code", -1)] = call(metric=-1)
        backend.ctx.set_sample_jitter(keep[4])
        refused[("short jitter", 0)] = call()
        backend.ctx.set_sample_jitter(keep[3])
        for what, (rc, res) in refused.items():
            assert rc != 0 and np.all(res == SENTINEL), (what, rc)
        for m in (_lib.BSPLINE_MEAN_SQUARES, _lib.BSPLINE_CORRELATION):
            assert refused[("jitter beyond its bound", m)][0] == _lib.ERR_ARG
            assert refused[("no overlap", m)][0] == _lib.ERR_NO_OVERLAP
            assert refused[("flipped lattice", m)][0] == refused[("virtual direction", m)][0] == _lib.ERR_DIRECTION
            rc, res = call(metric=m)        # ... and the context still works, to the bit
            assert rc == 0 and np.array_equal(res, before[m][1])
    finally:
        backend.ctx.set_sample_jitter(None)
