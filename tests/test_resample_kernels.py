"""The resampling kernels (pp_resample.hip, pp_warp_sample.h, pp_internal.h) against the definition-level fp64 restatement
tests/resample_restatement.py: exact border decisions on dyadic geometry, oblique and flipped grids at the kernel,
uint8 linear interpolation, hostile displacements, the two halves of the cubic B-spline apart, and one banded launch.

Decisions (inside / outside, nearest-neighbour picks, uint8 truncation) are compared at EVERY voxel; the only voxels ever
set aside are those whose fp64 reference coordinate lies within the kernel's own coordinate rounding of a decision
boundary, their share is asserted (it is 0 on every dyadic case) and the figures observed are written beside the
assertions.  Value bounds are derived, not tuned:

  fp64-coordinate kernels (k_resample*, k_resample_field*):   tol = 24 * 2^-24 * M
      three nested lerps a + (b - a) w of three fp32 roundings each on magnitudes <= 2 M, plus the fp32 rounding of the
      three weights (M = max |corner|)
  fp32-coordinate kernels (warp, compose):                    tol += 2^-22 * sum_a |d_a / s_a| * R
      the rounding of (float)(1 / s) and of the product d * (1 / s), times the local range R = max - min of the corners;
      compose adds 2^-24 |total + sample| for its final fp32 add.
"""
import numpy as np
import pytest

from platipy_amd import _lib
from tests import resample_restatement as R
from tests.helpers import (EPS6, border_probe_fields, border_targets, direction_cases, hostile_displacements, random_dvf,
                           record_stats, rot_xyz)

U24, U22 = 2.0 ** -24, 2.0 ** -22
LIN, NEAR, BSP = _lib.INTERP_LINEAR, _lib.INTERP_NEAREST, _lib.INTERP_BSPLINE
_WORST = {}     # group -> largest observed |error| / bound, kept by record_stats for the record


def _note(group, ratio):
    _WORST[group] = max(_WORST.get(group, 0.0), float(ratio))
    record_stats("resample_kernels_error_over_bound", _WORST)


def geom_of(g):
    return _lib.make_geom(g.size, g.spacing, g.origin, g.direction.ravel())


def grid_of(shape, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None):
    return R.Grid(shape[::-1], spacing, origin, direction)


def switch(monkeypatch, name, on):
    if on:
        monkeypatch.setenv(name, "1")
    else:
        monkeypatch.delenv(name, raising=False)


def run_warp(be, mov, f, g, edge):
    out = be.empty(g.shape)
    be.ctx.warp(be.dev(mov), be.dev(f), geom_of(g), edge, out)
    return be.host(out).copy()


def run_compose(be, total, it, g):
    d = be.dev(total)
    be.ctx.compose_field(d, be.dev(it), geom_of(g))
    return be.host(d).copy()


def run_resample(be, vol, gin, gout, interp, default, A=None, t=None, field=None):
    u8 = vol.dtype == np.uint8
    out = be.empty(gout.shape, np.uint8 if u8 else np.float32)
    be.ctx.resample(be.dev(vol), geom_of(gin), geom_of(gout), out, affine_A=None if A is None else np.asarray(A).ravel(),
                    affine_t=t, field=None if field is None else be.dev(field), interp=interp, default_value=default, u8=u8)
    return be.host(out).copy()


def run_resample_field(be, f, gin, gout):
    out = be.empty((3,) + gout.shape)
    be.ctx.resample_field(be.dev(f), geom_of(gin), geom_of(gout), out)
    return be.host(out).copy()


def tol_fp64(M):
    return 24.0 * U24 * M


def tol_fp32(M, Rng, field, spacing):
    dv = sum(np.abs(np.asarray(field[a], dtype=np.float64) / spacing[a]) for a in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return 24.0 * U24 * M + U22 * np.where(np.isfinite(dv), dv, 0.0) * Rng


def near_boundary(c, size, width, ties):
    """Voxels whose reference coordinate lies within `width` ([..., 3] or scalar) of -0.5 or n - 0.5 -- and, for `ties`, of any
    k + 0.5 -- on some axis: the kernel's own coordinate rounding may decide them either way."""
    w = np.broadcast_to(width, c.shape)
    hit = np.zeros(c.shape[:-1], bool)
    for a in range(3):
        ca = c[..., a]
        if ties:
            d = np.abs(ca - 0.5 - np.round(ca - 0.5))       # distance to the nearest half-integer
            hit |= (d < w[..., a]) & (ca > -1.0) & (ca < size[a])
        else:
            hit |= (np.abs(ca + 0.5) < w[..., a]) | (np.abs(ca - (size[a] - 0.5)) < w[..., a])
    return hit


def check_linear(group, got, ref, tol, keep=None, default=None):
    """Inside / outside equal to the reference at every kept voxel, values within the bound inside, the default exactly outside."""
    keep = np.ones(ref["inside"].shape, bool) if keep is None else keep
    ins = ref["inside"]
    if default is not None:
        got_out = got == np.float32(default)
        bad = keep & (got_out == ins)
        assert not bad.any(), (group, "inside/outside differs", np.argwhere(bad)[:5], ref["c"][bad][:5])
    sel = keep & ins
    err = np.abs(got.astype(np.float64) - ref["out"])[sel]
    t = np.broadcast_to(tol, ins.shape)[sel]
    if err.size:
        ratio = float((err / np.maximum(t, 1e-300)).max())
        _note(group, ratio)
        assert (err <= t).all(), (group, "error / bound", ratio, np.argwhere(keep & ins)[np.argmax(err / np.maximum(t, 1e-300))])


# --------------------------------------------------------------------------------------
# 1. exact border decisions on dyadic geometry (fp32 and fp64 coordinates are the same numbers)

BORDER_SHAPES = [(5, 6, 9), (4, 8, 12), (3, 4, 2), (6, 5, 1), (1, 1, 7), (1, 9, 1), (1, 1, 1)]
EDGE = -4096.0      # never a voxel value nor a lerp of voxel values: every image here stays within +-1000


def border_case(shape):
    k = BORDER_SHAPES.index(shape)
    sp = [(0.5, 2.0, 4.0), (1.0, 0.5, 2.0), (4.0, 1.0, 0.5)][k % 3]
    g = grid_of(shape, sp, (3.015625, -7.5, 11.25 + k))
    rng = np.random.default_rng(100 + k)
    img = np.clip(rng.normal(0.0, 400.0, shape), -1000.0, 1000.0).astype(np.float32)
    lab = rng.integers(0, 256, shape).astype(np.uint8)
    return g, img, lab, border_probe_fields(shape, sp, 200 + k)


def test_border_probes_reach_every_target():
    """The generator itself: on every shape, every (axis, target) pair occurs, exactly (the field is dyadic)."""
    for shape in BORDER_SHAPES:
        g, _, _, fields = border_case(shape)
        cs = np.concatenate([R.continuous_index(g, g, field=f).reshape(-1, 3) for f in fields])
        for a in range(3):
            assert set(border_targets(g.size[a])) <= set(cs[:, a].tolist()), (shape, a)
        ins = np.concatenate([R.inside_buffer(R.continuous_index(g, g, field=f), g.size).ravel() for f in fields])
        assert ins.any() and not ins.all()


@pytest.mark.parametrize("legacy", [False, True], ids=["sl", "legacy"])
@pytest.mark.parametrize("shape", BORDER_SHAPES)
def test_border_warp(backend, monkeypatch, shape, legacy):
    switch(monkeypatch, "PP_WARP_LEGACY", legacy)
    g, img, _, fields = border_case(shape)
    for f in fields:
        ref = R.resample(img, g, g, field=f, default=EDGE)
        got = run_warp(backend, img, f, g, EDGE)
        check_linear("1 border warp", got, ref, tol_fp32(ref["M"], ref["R"], f, g.spacing), default=EDGE)


@pytest.mark.parametrize("shape", BORDER_SHAPES)
def test_border_compose(backend, shape):
    g, _, _, fields = border_case(shape)
    rng = np.random.default_rng(7)
    it = rng.uniform(5.0, 20.0, (3,) + shape).astype(np.float32)     # > 0: the sampled term is 0 only outside
    for f in fields:
        ref = R.compose(f, it, g)
        got = run_compose(backend, f, it, g)
        moved = got != f
        for k in range(3):
            assert np.array_equal(moved[k], ref["inside"]), (shape, k, np.argwhere(moved[k] != ref["inside"])[:5])
        tol = tol_fp32(ref["M"], ref["R"], f, g.spacing) + U24 * np.abs(ref["out"])
        err = np.abs(got - ref["out"])
        _note("1 border compose", (err / np.maximum(tol, 1e-300)).max())
        assert (err <= tol).all(), (err / np.maximum(tol, 1e-300)).max()


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
@pytest.mark.parametrize("shape", BORDER_SHAPES)
def test_border_resample_through_field(backend, monkeypatch, shape, generic):
    switch(monkeypatch, "PP_RESAMPLE_GENERIC", generic)
    g, img, lab, fields = border_case(shape)
    for f in fields:
        ref = R.resample(img, g, g, field=f, default=EDGE)
        check_linear("1 border resample", run_resample(backend, img, g, g, LIN, EDGE, field=f), ref, tol_fp64(ref["M"]), default=EDGE)
        want = R.resample(img, g, g, field=f, interp="nearest", default=EDGE)["out"]
        np.testing.assert_array_equal(run_resample(backend, img, g, g, NEAR, EDGE, field=f), want)
        # uint8 labels: the default 300 clamps to 255; a label may be 255 too, so the whole volume is compared, bit for bit
        want = R.resample(lab, g, g, field=f, interp="nearest", default=300, u8=True)["out"]
        np.testing.assert_array_equal(run_resample(backend, lab, g, g, NEAR, 300, field=f), want)


@pytest.mark.parametrize("generic", [False, True], ids=["march", "generic"])
@pytest.mark.parametrize("shape", BORDER_SHAPES)
def test_border_resample_field_between_grids(backend, monkeypatch, shape, generic):
    """Seven output grids at half the input's spacing whose first sample sits at -0.5 (+- 2^-6 on one axis): along every
    axis the samples step through -0.5, 0, 0.5, ... n - 1, n - 0.5 (each also 2^-6 early and late)."""
    switch(monkeypatch, "PP_RESAMPLE_GENERIC", generic)
    g, _, _, _ = border_case(shape)
    rng = np.random.default_rng(11)
    f = rng.uniform(5.0, 20.0, (3,) + shape).astype(np.float32)      # > 0: 0 only outside
    shifts = [(0.0, 0.0, 0.0)] + [tuple(s * EPS6 if a == b else 0.0 for b in range(3)) for a in range(3) for s in (-1.0, 1.0)]
    seen = [set(), set(), set()]
    for d in shifts:
        org = g.origin + (np.asarray(d) - 0.5) * g.spacing
        gout = R.Grid([2 * n + 2 for n in g.size], g.spacing / 2.0, org)
        ref = R.resample_field(f, g, gout)
        got = run_resample_field(backend, f, g, gout)
        for k in range(3):
            assert np.array_equal(got[k] != 0.0, ref["inside"]), (shape, d, k)
        err, tol = np.abs(got - ref["out"]), tol_fp64(ref["M"])
        _note("1 border resample_field", (err / tol).max())
        assert (err <= tol).all(), (shape, d, (err / tol).max())
        for a in range(3):
            seen[a] |= set(ref["c"][..., a].ravel().tolist())
    for a in range(3):
        assert set(border_targets(g.size[a])) <= seen[a]


# --------------------------------------------------------------------------------------
# 2. oblique and flipped grids at the kernel

DIRS = direction_cases()
OB_IN_SHAPE, OB_OUT_SHAPE = (9, 11, 14), (8, 13, 10)
OB_A = rot_xyz(4.0, -3.0, 6.0) @ np.array([[1.05, 0.02, 0.0], [0.0, 0.97, -0.015], [0.01, 0.0, 1.02]])


def oblique_case(din, dout):
    gin = grid_of(OB_IN_SHAPE, (0.83, 1.27, 1.9), (-31.7, 12.3, 105.1), DIRS[din])
    ctr = gin.index_to_physical((np.asarray(gin.size) - 1) / 2.0)
    sp_out = np.array([1.6, 1.2, 2.6])      # inside shares 40 .. 58 % over the 100 cases
    org = ctr - DIRS[dout] @ (sp_out * (np.asarray(OB_OUT_SHAPE[::-1]) - 1) / 2.0) + np.array([0.3719, -0.2137, 0.4541])
    gout = grid_of(OB_OUT_SHAPE, sp_out, org, DIRS[dout])
    t = ctr - OB_A @ ctr + np.array([0.6, -0.4, 0.3])
    seed = 31 * list(DIRS).index(din) + list(DIRS).index(dout)
    rng = np.random.default_rng(seed)
    field = (random_dvf(OB_OUT_SHAPE, sp_out, seed=seed, max_mm=2.5) + rng.normal(0.0, 0.4, (3,) + OB_OUT_SHAPE)).astype(np.float32)
    return gin, gout, OB_A, t, field


def oblique_images():
    rng = np.random.default_rng(5)
    img = np.clip(rng.normal(0.0, 400.0, OB_IN_SHAPE), -1000.0, 1000.0).astype(np.float32)
    lab = rng.choice(np.array([0, 255, 1, 17, 128, 254], np.uint8), OB_IN_SHAPE, p=[0.2, 0.2, 0.15, 0.15, 0.15, 0.15])
    lab[2:6, 3:8, 4:10] = 200      # constant blocks: all eight corners equal somewhere, at 200, 0 and 255
    lab[6:9, 0:4, 0:5] = 0
    lab[0:3, 7:11, 9:14] = 255
    return img, lab


OB_MODES = ["none", "affine", "field", "affine+field"]
U8_DEFAULTS = {"none": -5.0, "affine": 300.0, "field": 7.4, "affine+field": 300.0}


@pytest.mark.parametrize("dout", list(DIRS))
@pytest.mark.parametrize("din", list(DIRS))
def test_oblique_resample(backend, din, dout):
    gin, gout, A, t, field = oblique_case(din, dout)
    img, lab = oblique_images()
    for mode in OB_MODES:
        kw = dict(A=A if "affine" in mode else None, t=t if "affine" in mode else None, field=field if "field" in mode else None)
        ref = R.resample(img, gin, gout, default=EDGE, **kw)
        share = ref["inside"].mean()
        assert 0.2 <= share <= 0.8, (din, dout, mode, share)
        # fp64 coordinates on both sides: only voxels within 1e-9 of a boundary are set aside (measured: none on any of the 100 cases)
        edge_band = near_boundary(ref["c"], gin.size, 1e-9, ties=False)
        tie_band = near_boundary(ref["c"], gin.size, 1e-9, ties=True)
        assert edge_band.mean() <= 0.005 and tie_band.mean() <= 0.005
        got = run_resample(backend, img, gin, gout, LIN, EDGE, **kw)
        check_linear("2 oblique resample f32", got, ref, tol_fp64(ref["M"]), keep=~edge_band, default=EDGE)
        for vol, dflt in ((img, EDGE), (lab, U8_DEFAULTS[mode])):
            want = R.resample(vol, gin, gout, interp="nearest", default=dflt, u8=vol.dtype == np.uint8, **kw)["out"]
            got = run_resample(backend, vol, gin, gout, NEAR, dflt, **kw)
            np.testing.assert_array_equal(got[~tie_band], want[~tie_band])
        # uint8 linear: clamp, then truncate; exact where the eight corners agree, elsewhere unless the reference sits within
        # the fp32 bound of an integer (share set aside, measured on the reference alone: at most 0.68 % over the 100 cases -- mostly lerps
        # between equal corners on two axes, whose fp64 value is an integer up to rounding; cap 1 %)
        r8 = R.resample(lab, gin, gout, default=U8_DEFAULTS[mode], u8=True, **kw)
        got = run_resample(backend, lab, gin, gout, LIN, U8_DEFAULTS[mode], **kw)
        shaky = r8["inside"] & (r8["R"] > 0) & (np.abs(r8["ref"] - np.round(r8["ref"])) < tol_fp64(r8["M"]))
        assert shaky.mean() <= 0.01, shaky.mean()
        keep = ~(shaky | edge_band)
        np.testing.assert_array_equal(got[keep], r8["out"][keep])
        assert (r8["inside"] & (r8["R"] == 0)).any() and (got[~r8["inside"]] == np.uint8(np.clip(U8_DEFAULTS[mode], 0, 255))).all()


@pytest.mark.parametrize("dout", list(DIRS))
@pytest.mark.parametrize("din", list(DIRS))
def test_oblique_resample_field(backend, din, dout):
    gin, gout, _, _, _ = oblique_case(din, dout)
    rng = np.random.default_rng(3)
    f = (rng.uniform(5.0, 20.0, (3,) + OB_IN_SHAPE) * rng.choice([-1.0, 1.0], (3, 1, 1, 1))).astype(np.float32)
    ref = R.resample_field(f, gin, gout)
    assert 0.2 <= ref["inside"].mean() <= 0.8
    band = near_boundary(ref["c"], gin.size, 1e-9, ties=False)
    assert band.mean() <= 0.005
    got = run_resample_field(backend, f, gin, gout)
    for k in range(3):
        assert np.array_equal((got[k] != 0.0)[~band], ref["inside"][~band]), (din, dout, k)
    err, tol = np.abs(got - ref["out"])[:, ~band], tol_fp64(ref["M"])[:, ~band]
    _note("2 oblique resample_field", (err / tol).max())
    assert (err <= tol).all(), (err / tol).max()


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("direction", list(DIRS))
def test_transform_to_field(backend, direction, with_add):
    """k_affine_displacement: (A - I) p + t in fp64, rounded once to fp32 (2^-24 |D|), then one fp32 add of `add_field`
    (2^-24 |D + add|); 2^-23 max |D| leaves the fp64 products their own rounding."""
    g = grid_of((6, 9, 11), (0.83, 1.27, 1.9), (-31.7, 12.3, 105.1), DIRS[direction])
    A = rot_xyz(-8.0, 5.0, 12.0) @ np.array([[1.1, 0.03, 0.0], [0.0, 0.93, 0.02], [-0.01, 0.0, 1.04]])
    t = np.array([12.5, -7.25, 3.1])
    add = np.random.default_rng(9).normal(0.0, 30.0, (3,) + g.shape).astype(np.float32) if with_add else None
    plain, want = R.affine_displacement(g, A, t, add)
    out = backend.empty((3,) + g.shape)
    backend.ctx.transform_to_field(geom_of(g), A, t, None if add is None else backend.dev(add), out)
    got = backend.host(out)
    tol = 2.0 ** -23 * np.abs(plain).max() + (U24 * np.abs(want) if with_add else 0.0)
    err = np.abs(got - want)
    _note("2 transform_to_field", (err / tol).max())
    assert (err <= tol).all(), (err / tol).max()
    assert np.abs(plain).max() > 10.0


# --------------------------------------------------------------------------------------
# 3. random, non-dyadic same-grid cases: the fp32-coordinate kernels with their coordinate rounding set aside

RANDOM_GRIDS = [((7, 10, 13), (0.9, 1.1, 2.5), (320.0, -52.0, 60.0), 41), ((6, 9, 16), (1.3, 0.7, 1.0), (-3.0, 8.5, 0.25), 42)]


def random_case(shape, spacing, origin, seed):
    g = grid_of(shape, spacing, origin)
    rng = np.random.default_rng(seed)
    img = np.clip(rng.normal(0.0, 400.0, shape), -1000.0, 1000.0).astype(np.float32)
    f = (random_dvf(shape, spacing, seed=seed, max_mm=5.0) + rng.normal(0.0, 0.5, (3,) + shape)).astype(np.float32)
    f[:, :, :2, :] *= 3.0      # push some rows out of the buffer
    return g, img, f


def fp32_band(c, f, g, ties=False):
    width = np.stack([U22 * np.abs(f[a].astype(np.float64) / g.spacing[a]) + 1e-9 for a in range(3)], axis=-1)
    return near_boundary(c, g.size, width, ties)


def test_random_cases_set_aside_under_half_a_percent():
    """The seeds: on the reference alone, the share of voxels within coordinate rounding of a boundary (measured: 0 on both)."""
    for grid in RANDOM_GRIDS:
        g, img, f = random_case(*grid)
        ref = R.resample(img, g, g, field=f, default=EDGE)
        assert fp32_band(ref["c"], f, g).mean() <= 0.005
        assert 0.02 < (~ref["inside"]).mean() < 0.6


@pytest.mark.parametrize("legacy", [False, True], ids=["sl", "legacy"])
@pytest.mark.parametrize("grid", RANDOM_GRIDS, ids=["vec1", "vec4"])
def test_random_warp_and_compose(backend, monkeypatch, grid, legacy):
    switch(monkeypatch, "PP_WARP_LEGACY", legacy)
    g, img, f = random_case(*grid)
    ref = R.resample(img, g, g, field=f, default=EDGE)
    band = fp32_band(ref["c"], f, g)
    assert band.mean() <= 0.005
    check_linear("3 random warp", run_warp(backend, img, f, g, EDGE), ref, tol_fp32(ref["M"], ref["R"], f, g.spacing), keep=~band, default=EDGE)
    if legacy:
        return
    it = (np.random.default_rng(1).uniform(5.0, 20.0, (3,) + g.shape)).astype(np.float32)
    rc = R.compose(f, it, g)
    got = run_compose(backend, f, it, g)
    for k in range(3):
        assert np.array_equal((got[k] != f[k])[~band], rc["inside"][~band])
    tol = tol_fp32(rc["M"], rc["R"], f, g.spacing) + U24 * np.abs(rc["out"])
    err = np.abs(got - rc["out"])[:, ~band]
    _note("3 random compose", (err / tol[:, ~band]).max())
    assert (err <= tol[:, ~band]).all(), (err / tol[:, ~band]).max()


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
def test_random_axis_aligned_resample(backend, monkeypatch, affine, generic):
    """k_resample_axis (with and without its 3 x 3) and k_resample between two different axis-aligned grids through a field."""
    switch(monkeypatch, "PP_RESAMPLE_GENERIC", generic)
    gin, img, _ = random_case(*RANDOM_GRIDS[0])
    gout = grid_of((8, 9, 15), (1.05, 1.3, 2.1), (319.0, -53.0, 59.0))
    f = (random_dvf(gout.shape, gout.spacing, seed=8, max_mm=4.0)).astype(np.float32)
    ctr = gin.index_to_physical((np.asarray(gin.size) - 1) / 2.0)
    kw = dict(A=OB_A, t=ctr - OB_A @ ctr) if affine else {}
    ref = R.resample(img, gin, gout, field=f, default=EDGE, **kw)
    edge_band = near_boundary(ref["c"], gin.size, 1e-9, ties=False)
    tie_band = near_boundary(ref["c"], gin.size, 1e-9, ties=True)
    assert edge_band.mean() <= 0.005 and tie_band.mean() <= 0.005 and 0.1 < ref["inside"].mean() < 0.9
    check_linear("3 random resample", run_resample(backend, img, gin, gout, LIN, EDGE, field=f, **kw), ref, tol_fp64(ref["M"]),
                 keep=~edge_band, default=EDGE)
    want = R.resample(img, gin, gout, field=f, interp="nearest", default=EDGE, **kw)["out"]
    got = run_resample(backend, img, gin, gout, NEAR, EDGE, field=f, **kw)
    np.testing.assert_array_equal(got[~tie_band], want[~tie_band])


# --------------------------------------------------------------------------------------
# 4. degenerate and hostile displacements: NaN, Inf and absurd values are "outside", and disturb no other voxel

def hostile_case(shape):
    g, img, lab, _ = border_case(shape)
    rng = np.random.default_rng(17)
    clean = rng.uniform(-1.5, 1.5, (3,) + shape).astype(np.float32) * np.asarray(g.spacing, np.float32)[:, None, None, None]
    f = clean.copy()
    N = img.size
    hit = np.zeros(shape, bool)
    k = 0
    for a in range(3):
        for v in hostile_displacements(g.spacing[a]):
            i = (7 * k + 3) % N
            f[a].reshape(-1)[i] = v
            hit.reshape(-1)[i] = True
            k += 1
    return g, img, lab, clean, f, hit


@pytest.mark.parametrize("legacy", [False, True], ids=["sl", "legacy"])
@pytest.mark.parametrize("shape", [(5, 6, 9), (4, 8, 12), (6, 5, 1)])
def test_hostile_displacements_warp_and_compose(backend, monkeypatch, shape, legacy):
    switch(monkeypatch, "PP_WARP_LEGACY", legacy)
    g, img, _, clean, f, hit = hostile_case(shape)
    assert not R.inside_buffer(R.continuous_index(g, g, field=f), g.size)[hit].any()      # by definition, not by the kernel's rule
    base, got = run_warp(backend, img, clean, g, EDGE), run_warp(backend, img, f, g, EDGE)
    assert (got[hit] == np.float32(EDGE)).all()
    np.testing.assert_array_equal(got[~hit], base[~hit])
    assert (base[hit] != np.float32(EDGE)).any()
    if legacy:
        return
    it = np.random.default_rng(1).uniform(5.0, 20.0, (3,) + shape).astype(np.float32)
    base, got = run_compose(backend, clean, it, g), run_compose(backend, f, it, g)
    np.testing.assert_array_equal(got[:, hit], f[:, hit])          # total + 0, NaN and Inf included
    np.testing.assert_array_equal(got[:, ~hit], base[:, ~hit])


@pytest.mark.parametrize("generic", [False, True], ids=["fast", "generic"])
@pytest.mark.parametrize("shape", [(5, 6, 9), (6, 5, 1)])
def test_hostile_displacements_resample(backend, monkeypatch, shape, generic):
    switch(monkeypatch, "PP_RESAMPLE_GENERIC", generic)
    g, img, lab, clean, f, hit = hostile_case(shape)
    for vol, dflt in ((img, EDGE), (lab, 300.0)):
        for interp in (LIN, NEAR):
            base = run_resample(backend, vol, g, g, interp, dflt, field=clean)
            got = run_resample(backend, vol, g, g, interp, dflt, field=f)
            assert (got[hit] == (np.uint8(255) if vol.dtype == np.uint8 else np.float32(dflt))).all()
            np.testing.assert_array_equal(got[~hit], base[~hit])


# --------------------------------------------------------------------------------------
# 5. cubic B-spline: the prefilter and the evaluation, each against scipy on its own

PREFILTER_LENGTHS = [1, 2, 3, 4, 17, 18, 19, 20, 41]


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["z", "y", "x"])
@pytest.mark.parametrize("length", PREFILTER_LENGTHS)
def test_bspline_prefilter(backend, length, axis):
    shape = [3, 4, 5]
    shape[axis] = length
    vol = np.random.default_rng(1000 + 10 * length + axis).normal(0.0, 1000.0, shape).astype(np.float32)
    want = R.bspline_prefilter(vol)
    # The reference's own sensitivity to fp32 storage between the passes, times 4 for the kernel's second fp32 store inside
    # each pass (the causal sweep is stored, then the anti-causal sweep).  Measured over the 27 cases: bounds of 1.0e-3 ..
    # 8.8e-3 on coefficients of order 6000 (the filter's gain); the kernel's largest error is 0.50 of its bound.
    bound = 4.0 * np.abs(R.bspline_prefilter_fp32_storage(vol) - want).max()
    assert bound > 0.0
    size = tuple(shape[::-1])
    out = backend.empty(tuple(shape))
    backend.ctx.bspline_prefilter(backend.dev(vol), size, out)
    sep = backend.host(out).copy()
    buf = backend.dev(vol)
    backend.ctx.bspline_prefilter(buf, size, buf)
    np.testing.assert_array_equal(backend.host(buf), sep)           # in place == out of place, bit for bit
    err = np.abs(sep - want).max()
    _note("5 prefilter", err / bound)
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("shape", [(6, 7, 9), (1, 5, 2)])
def test_bspline_evaluation(backend, shape):
    sp = (0.5, 2.0, 1.0)
    g = grid_of(shape, sp, (3.015625, -7.5, 11.25))
    coef = np.random.default_rng(77).normal(0.0, 1000.0, shape).astype(np.float32)
    mirrored_twice = False
    for f in border_probe_fields(shape, sp, 300):
        c = R.continuous_index(g, g, field=f)
        ins = R.inside_buffer(c, g.size)
        want = R.bspline_evaluate(coef, np.where(ins[..., None], c, 0.0))
        got = run_resample(backend, coef, g, g, BSP, EDGE, field=f)
        assert np.array_equal(got == np.float32(EDGE), ~ins)
        err, bound = np.abs(got - want)[ins], 4.0 * U24 * np.abs(coef).max()
        _note("5 evaluation", err.max() / bound)
        assert (err <= bound).all(), (err.max(), bound)
        for a in range(3):
            n = g.size[a]
            lo = np.floor(c[..., a][ins]) - 1
            if n >= 2 and ((lo < -(n - 1)) | (lo + 3 > 2 * (n - 1))).any():
                mirrored_twice = True
    assert mirrored_twice == (min(s for s in shape if s > 1) <= 2)   # (1, 5, 2): the 4-wide support wraps the period on x


def test_bspline_u8_raises(backend):
    g = grid_of((3, 4, 5))
    lab = np.zeros(g.shape, np.uint8)
    with pytest.raises(_lib.PlatipyAmdError):
        run_resample(backend, lab, g, g, BSP, 0.0)


# --------------------------------------------------------------------------------------
# 6. one banded launch: 65 tiles of 64 x 4 per plane, 9 per XCD with 7 left over

def test_banded_launch_against_the_definition(backend):
    shape, sp = (2, 260, 12), (0.9, 1.1, 2.5)
    g = grid_of(shape, sp, (4.0, -2.0, 1.5))
    rng = np.random.default_rng(61)
    img = np.clip(rng.normal(0.0, 400.0, shape), -1000.0, 1000.0).astype(np.float32)
    f = (random_dvf(shape, sp, seed=62, max_mm=4.0) + rng.normal(0.0, 0.5, (3,) + shape)).astype(np.float32)
    ref = R.resample(img, g, g, field=f, default=EDGE)
    band = near_boundary(ref["c"], g.size, 1e-9, ties=False)
    assert band.mean() <= 0.005 and 0.05 < (~ref["inside"]).mean() < 0.8
    check_linear("6 banded resample", run_resample(backend, img, g, g, LIN, EDGE, field=f), ref, tol_fp64(ref["M"]), keep=~band, default=EDGE)
    band = fp32_band(ref["c"], f, g)
    assert band.mean() <= 0.005
    check_linear("6 banded warp", run_warp(backend, img, f, g, EDGE), ref, tol_fp32(ref["M"], ref["R"], f, g.spacing), keep=~band, default=EDGE)
