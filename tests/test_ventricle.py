"""The left-ventricle 17-segment model -- pp_polar_sectors_u8, pp_resample_bits_u32 (csrc/pp_ventricle.h), GetInverse,
principal_axes_from_moments and utils/ventricle.py -- against tests/ventricle_restatement.py, the reference's arithmetic in
fp64 numpy / scipy.

Bounds (none is tuned):
  * bits, counts, bit planes and the 17 masks: np.array_equal.  An fp64 atan2 may differ by an ulp between libraries, so
    every comparison of sectors first asserts ON THE NUMPY SIDE that each voxel's distance to a sector boundary and to
    radius_min is either exactly 0 or above 1e-9 (exact ties are axis-aligned voxels, whose atan2 is 0, +-pi / 2 or pi in
    every library); the whole function also asserts that no nearest-neighbour resample has an inside index within 1e-9 of a
    half-integer (the rotation parameters come from exact integer moments and agree to ~1e-12 between the two sides, which
    moves an index by ~1e-10 at these coordinates);
  * info scalars: 1e-9; integer limits and counts: equal;
  * GetInverse, principal_axes_from_moments: 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

from tests import resample_restatement as R
from tests import ventricle_restatement as V

PI = np.pi
CW, ANY = V.CW, V.ANY_AREA


def size_of(shape):
    return (shape[2], shape[1], shape[0])


# --------------------------------------------------------------------------------------
# pp_polar_sectors_u8

SIX = [(lab, 0, lo, hi) for lab, (lo, hi) in zip((8, 9, 10, 11, 12, 7), V.SIXTHS)]
FOUR = [(1, 0, 5 * PI / 4, 7 * PI / 4), (32, CW, 1 * PI / 4, 7 * PI / 4), (15, 0, 1 * PI / 4, 3 * PI / 4), (16, 0, 3 * PI / 4, 5 * PI / 4)]
WHOLE = [(17, 0, -np.inf, np.inf)]
RULES = SIX + FOUR + WHOLE + [(17, ANY, -np.inf, np.inf)]      # 0-5, 6-9, 10, 11


def slice_table(shape):
    """One entry per slice, cycling through: six sectors about an integer centre with theta0 = 0 (exact ties, V5); four sectors
    (labels 1 and 32, a clockwise rule) with theta0 in (pi, 2 pi); skipped; the whole slice; six sectors with radius_min = 3 and
    theta0 in (pi, 2 pi) about a centre outside the image, so that V4 leaves voxels without a segment (the angle stays
    negative after the single + 2 pi; only a clockwise rule would take it); the whole slice, exempt from the area test; four
    sectors about a fractional centre."""
    nz, ny, nx = shape
    kinds = [(float(ny // 2), float(nx // 2), 0.0, 0.0, 0, 6), (ny / 2 + 0.37, nx / 2 - 0.21, 4.0, 0.0, 6, 4), (0.0, 0.0, 0.0, 0.0, 0, 0),
             (0.0, 0.0, 0.0, 0.0, 10, 1), (-2.25, nx + 1.5, 4.0, 3.0, 0, 6), (0.0, 0.0, 0.0, 0.0, 11, 1), (ny / 3 + 0.13, nx / 3 + 0.29, -0.7, 3.0, 6, 4)]
    return [kinds[z % len(kinds)] for z in range(nz)]


def run_polar(backend, mask, slices, rules, area, min_area, offset=0):
    shape = mask.shape
    if offset:
        buf = backend.dev(np.concatenate([np.zeros(offset, np.uint8), mask.ravel()]))
        dmask = buf[offset:]
    else:
        dmask = backend.dev(mask)
    bits = backend.dev(np.full(shape, 0x5a5a5a5a, np.uint32).view(np.int32))
    counts = backend.dev(np.full((shape[0], 32), -7, np.int64))
    backend.ctx.polar_sectors(dmask, size_of(shape), slices, rules, area, min_area, bits, counts)
    return backend.host(bits).view(np.uint32), backend.host(counts)


def equality_threshold(counts, area):
    """min_area that puts one (slice, label) pair exactly on the threshold (kept) and another one count below (dropped), or
    None when no two pairs differ by one voxel."""
    present = set(int(c) for c in counts.ravel() if c > 1)
    for c in sorted(present):
        if c - 1 in present:
            return c * area
    return None


def check_polar(backend, mask, offset=0, need_threshold=False, min_area=None):
    shape = mask.shape
    slices, area = slice_table(shape), 0.5
    if min_area is None:
        _, plain = V.polar_sectors(mask, slices, RULES, area, 0.0)
        min_area = equality_threshold(plain, area)
        assert min_area is not None or not need_threshold
        if min_area is None:
            min_area = float(np.median(plain[plain > 0])) * area if (plain > 0).any() else 1.0
    gaps = {}
    want_bits, want_counts = V.polar_sectors(mask, slices, RULES, area, min_area, gaps)
    assert gaps["angle"] > 1e-9 and gaps["radius"] > 1e-9, gaps      # no voxel is decided by the last bits of atan2 / sqrt
    got_bits, got_counts = run_polar(backend, mask, slices, RULES, area, min_area, offset)
    print(f"polar {shape} offset {offset}: min_area {min_area}, gaps {gaps}, voxels {int((want_bits != 0).sum())}")
    assert np.array_equal(got_counts, want_counts), np.argwhere(got_counts != want_counts)[:5]
    assert np.array_equal(got_bits, want_bits), np.argwhere(got_bits != want_bits)[:5]
    again_bits, again_counts = run_polar(backend, mask, slices, RULES, area, min_area, offset)
    assert np.array_equal(again_bits, got_bits) and np.array_equal(again_counts, got_counts)
    return want_bits, want_counts, min_area, area


POLAR_SHAPES = [(5, 9, 37), (1, 7, 19), (6, 5, 1), (3, 4, 1040), (7, 16, 48)]


@pytest.mark.parametrize("shape", POLAR_SHAPES, ids=str)
def test_polar_sectors_random_mask(backend, shape):
    rng = np.random.default_rng(11)
    mask = ((rng.random(shape) < 0.3) * rng.integers(1, 256, shape)).astype(np.uint8)
    check_polar(backend, mask)


@pytest.mark.parametrize("shape", POLAR_SHAPES, ids=str)
def test_polar_sectors_full_and_empty_masks(backend, shape):
    big = shape in ((5, 9, 37), (7, 16, 48), (3, 4, 1040))
    bits, counts, min_area, area = check_polar(backend, np.ones(shape, np.uint8), need_threshold=big)
    if big:
        kept = [(z, l) for z, l in np.argwhere(counts * area == min_area) if (bits[z] >> np.uint32(l) & np.uint32(1)).any()]
        dropped = [(z, l) for z, l in np.argwhere((counts > 0) & (counts * area < min_area)) if not (bits[z] >> np.uint32(l) & np.uint32(1)).any()]
        assert kept and dropped                                    # equality keeps, one voxel fewer drops
        bits, _, _, _ = check_polar(backend, np.ones(shape, np.uint8), min_area=0.0)
        two = np.array([bin(int(v)).count("1") for v in bits[0].ravel()]) >= 2
        assert two.any()                                           # V5: a voxel on a boundary carries two bits
        if shape[0] > 4:                                           # V4: theta0 in (pi, 2 pi) leaves voxels without a segment
            assert (bits[4] == 0).any() and (bits[4] != 0).any()
    got, cnt, _, _ = check_polar(backend, np.zeros(shape, np.uint8))
    assert not got.any() and not cnt.any()


def test_polar_sectors_unaligned_mask(backend):
    rng = np.random.default_rng(12)
    shape = (7, 16, 48)
    mask = (rng.random(shape) < 0.3).astype(np.uint8)
    a = check_polar(backend, mask, offset=3)
    b = check_polar(backend, mask)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_polar_sectors_exempt_rule_survives_the_area_test(backend):
    mask = np.ones((2, 3, 5), np.uint8)
    slices = [(0.0, 0.0, 0.0, 0.0, 0, 1), (0.0, 0.0, 0.0, 0.0, 1, 1)]
    rules = [(17, 0, -np.inf, np.inf), (17, ANY, -np.inf, np.inf)]
    bits, counts = run_polar(backend, mask, slices, rules, 1.0, 1000.0)
    assert not bits[0].any() and (bits[1] == 1 << 16).all() and counts[0, 16] == 15 and counts[1, 16] == 15


def test_polar_sectors_bad_arguments_leave_the_outputs_alone(backend):
    shape = (2, 3, 4)
    mask = backend.dev(np.ones(shape, np.uint8))
    bits = backend.dev(np.full(shape, 77, np.int32))
    counts = backend.dev(np.full((2, 32), -7, np.int64))
    ok = [(1.0, 1.0, 0.0, 0.0, 0, 1)] * 2
    cases = [(ok, [(0, 0, 0.0, 1.0)]), (ok, [(33, 0, 0.0, 1.0)]), ([(1.0, 1.0, 0.0, 0.0, 1, 1)] * 2, [(1, 0, 0.0, 1.0)]),
             ([(1.0, 1.0, 0.0, 0.0, 0, 2)] * 2, [(1, 0, 0.0, 1.0)]), ([(1.0, 1.0, 0.0, 0.0, -1, 1)] * 2, [(1, 0, 0.0, 1.0)]),
             (ok, [(1, 4, 0.0, 1.0)])]
    for slices, rules in cases:
        with pytest.raises(ValueError):
            backend.ctx.polar_sectors(mask, size_of(shape), slices, rules, 1.0, 0.0, bits, counts)
    rules = [(1, 0, 0.0, 1.0)]
    for m, b, c in ((None, bits, counts), (mask, None, counts), (mask, bits, None)):
        with pytest.raises(ValueError):
            backend.ctx.polar_sectors(m, size_of(shape), ok, rules, 1.0, 0.0, b, c)
    with pytest.raises(ValueError):
        backend.ctx.polar_sectors(mask, (4, 3, 0), [], rules, 1.0, 0.0, bits, counts)
    with pytest.raises(ValueError):
        backend.ctx.polar_sectors(mask, size_of(shape), ok[:1], rules, 1.0, 0.0, bits, counts)      # one entry per slice
    # the error code itself, through the C ABI
    from platipy_amd import _lib

    st = np.array(ok, dtype=_lib.POLAR_SLICE_DTYPE)
    rt = np.array([(0, 0, 0.0, 1.0)], dtype=_lib.POLAR_RULE_DTYPE)
    rc = backend.lib.pp_polar_sectors_u8(backend.ctx.h, _lib.ptr(mask), (ctypes.c_int * 3)(4, 3, 2), st.ctypes.data, rt.ctypes.data, 1, 1.0, 0.0,
                                         _lib.ptr(bits), _lib.ptr(counts))
    assert rc == _lib.ERR_ARG
    assert (backend.host(bits) == 77).all() and (backend.host(counts) == -7).all()


# --------------------------------------------------------------------------------------
# pp_resample_bits_u32


def rigid(axis, angle, centre, shift=(0.0, 0.0, 0.0)):
    from tests.cardiac_geometry_restatement import versor_matrix

    A = versor_matrix(axis, angle)
    c = np.asarray(centre, dtype=np.float64)
    return A, c - A @ c + np.asarray(shift, dtype=np.float64)


@pytest.mark.parametrize("nbits", [1, 17, 32])
@pytest.mark.parametrize("case", ["oblique", "partly-outside", "oblique-grid"])
@pytest.mark.parametrize("shape", [(6, 10, 21), (4, 9, 37)], ids=str)
def test_resample_bits(backend, shape, case, nbits):
    from platipy_amd import _lib
    from tests.helpers import rot_xyz

    rng = np.random.default_rng(21)
    vol = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    spacing, origin = (1.25, 1.1, 1.8), (-7.5, 4.0, 30.0)
    size = size_of(shape)
    centre = np.asarray(origin) + np.asarray(spacing) * (np.asarray(size) - 1) / 2.0
    direction = rot_xyz(10.0, -20.0, 30.0) if case == "oblique-grid" else np.eye(3)
    gin = R.Grid(size, spacing, origin)
    gout = R.Grid(size, spacing, origin, direction)
    A, t = rigid((1, 2, 3), 0.4, centre, (0.0, 0.0, 0.0) if case != "partly-outside" else (9.3, -4.1, 2.7))
    lgin = _lib.make_geom(size, spacing, origin)
    lgout = _lib.make_geom(size, spacing, origin, direction.ravel())
    out = backend.dev(np.full((nbits,) + shape, 9, np.uint8))
    backend.ctx.resample_bits(backend.dev(vol.view(np.int32)), lgin, lgout, nbits, out, affine_A=A.ravel(), affine_t=t)
    got = backend.host(out)
    inside_any = False
    for k in range(nbits):
        plane = ((vol >> np.uint32(k)) & np.uint32(1)).astype(np.uint8)
        want = R.resample(plane, gin, gout, A, t, interp="nearest", default=0, u8=True)
        frac = want["c"][want["inside"]]
        assert frac.size == 0 or np.abs(frac - np.floor(frac) - 0.5).min() > 1e-9      # no index sits on a rounding tie
        inside_any |= bool(want["inside"].any())
        assert case != "partly-outside" or (not want["inside"].all() and want["inside"].any())
        assert np.array_equal(got[k], want["out"]), (k, np.argwhere(got[k] != want["out"])[:5])
        one = backend.dev(np.full(shape, 9, np.uint8))
        backend.ctx.resample(backend.dev(plane), lgin, lgout, one, affine_A=A.ravel(), affine_t=t, interp=_lib.INTERP_NEAREST, default_value=0.0,
                             u8=True)
        assert np.array_equal(got[k], backend.host(one)), k
    assert inside_any


def test_resample_bits_without_a_transform(backend):
    """affine_A=None on two axis-aligned grids of different size, spacing and origin: the arm without a linear transform; part of
    the output grid lies outside the input."""
    from platipy_amd import _lib

    rng = np.random.default_rng(22)
    shape_in, shape_out = (6, 10, 21), (5, 13, 18)
    vol = rng.integers(0, 2 ** 32, shape_in, dtype=np.uint64).astype(np.uint32)
    sp_in, org_in, sp_out, org_out = (1.25, 1.1, 1.8), (-7.5, 4.0, 30.0), (1.7, 0.9, 2.1), (-9.1, 5.3, 28.9)
    gin, gout = R.Grid(size_of(shape_in), sp_in, org_in), R.Grid(size_of(shape_out), sp_out, org_out)
    lgin, lgout = _lib.make_geom(size_of(shape_in), sp_in, org_in), _lib.make_geom(size_of(shape_out), sp_out, org_out)
    out = backend.dev(np.full((32,) + shape_out, 9, np.uint8))
    backend.ctx.resample_bits(backend.dev(vol.view(np.int32)), lgin, lgout, 32, out)
    got = backend.host(out)
    for k in range(32):
        plane = ((vol >> np.uint32(k)) & np.uint32(1)).astype(np.uint8)
        want = R.resample(plane, gin, gout, interp="nearest", default=0, u8=True)
        frac = want["c"][want["inside"]]
        assert np.abs(frac - np.floor(frac) - 0.5).min() > 1e-9 and want["inside"].any() and not want["inside"].all()
        assert np.array_equal(got[k], want["out"]), k
        one = backend.dev(np.full(shape_out, 9, np.uint8))
        backend.ctx.resample(backend.dev(plane), lgin, lgout, one, interp=_lib.INTERP_NEAREST, default_value=0.0, u8=True)
        assert np.array_equal(got[k], backend.host(one)), k


@pytest.mark.parametrize("case", ["oblique", "partly-outside"])
def test_resample_bits_equals_apply_transform(host_api, case):
    """Every plane against the public seam: apply_transform (nearest neighbour, default 0) of that bit as a uint8 Image."""
    pa = host_api
    rng = np.random.default_rng(23)
    shape, spacing, origin = (4, 9, 37), (1.25, 1.1, 1.8), (-7.5, 4.0, 30.0)
    vol = rng.integers(0, 2 ** 17, shape, dtype=np.int64).astype(np.int32)
    size = size_of(shape)
    t = pa.VersorRigid3DTransform()
    t.SetCenter(np.asarray(origin) + np.asarray(spacing) * (np.asarray(size) - 1) / 2.0)
    t.SetRotation((1, 2, 3), 0.4)
    if case == "partly-outside":
        p = np.array(t.GetParameters())
        p[3:] = (9.3, -4.1, 2.7)
        t.SetParameters(p)
    A, off = t.matrix_offset()
    image = pa.image_from_array(vol, spacing, origin)
    planes = torch.full((17,) + shape, 9, dtype=torch.uint8, device=image.device)
    pa.runtime.context(image.device).resample_bits(image.tensor, image.geom(), image.geom(), 17, planes, affine_A=A.ravel(), affine_t=off)
    some = False
    for k in range(17):
        bit = pa.image_from_array(((vol >> k) & 1).astype(np.uint8), spacing, origin)
        want = pa.registration.apply_transform(bit, bit, t, 0, pa.sitkNearestNeighbor).numpy()
        some |= bool(want.any())
        assert np.array_equal(planes[k].cpu().numpy(), want), k
    assert some


def test_resample_bits_refuses_bad_arguments(backend):
    from platipy_amd import _lib

    g = _lib.make_geom((4, 3, 2))
    vol, out = backend.dev(np.zeros((2, 3, 4), np.int32)), backend.dev(np.full((1, 2, 3, 4), 9, np.uint8))
    for nbits in (0, 33, -1):
        with pytest.raises(ValueError):
            backend.ctx.resample_bits(vol, g, g, nbits, out)
    with pytest.raises(ValueError):
        backend.ctx.resample_bits(None, g, g, 1, out)
    with pytest.raises(ValueError):
        backend.ctx.resample_bits(vol, g, g, 1, None)
    assert (backend.host(out) == 9).all()


# --------------------------------------------------------------------------------------
# GetInverse, principal_axes_from_moments


def test_get_inverse():
    from platipy_amd import transform as T

    def versor(axis, angle, centre, translation):
        t = T.VersorRigid3DTransform()
        t.SetCenter(centre)
        t.SetRotation(axis, angle)
        p = np.array(t.GetParameters())
        p[3:] = translation
        t.SetParameters(p)
        return t

    one = versor((1, 2, 3), 0.7, (10.0, -20.0, 30.0), (1.5, -2.5, 3.5))
    three = T.CompositeTransform([one, versor((0, 1, 1), -1.1, (3.0, 4.0, 5.0), (0.0, 0.0, 0.0)),
                                  T.AffineTransform(np.diag([1.1, 0.9, 1.3]), (4.0, 5.0, 6.0), (1.0, 2.0, 3.0))])
    for t in (one, three):
        inv = t.GetInverse()
        for both in (T.CompositeTransform([inv, t]), T.CompositeTransform([t, inv])):
            A, off = both.matrix_offset()
            assert np.abs(A - np.eye(3)).max() <= 1e-12 and np.abs(off).max() <= 1e-12
    assert np.allclose(one.GetInverse().GetCenter(), one.GetCenter())
    assert isinstance(T.Transform().GetInverse(), T.Transform)
    with pytest.raises(ValueError):
        T.AffineTransform(np.zeros((3, 3))).GetInverse()
    field = type("F", (T.Transform,), {"is_linear": lambda self: False})()
    with pytest.raises(TypeError):
        T.CompositeTransform([one, field]).GetInverse()
    with pytest.raises(TypeError):
        field.GetInverse()
    zero = torch.zeros((3, 2, 3, 4), dtype=torch.float32)
    from platipy_amd.image import Image

    with pytest.raises(TypeError):      # the classes that derive from Transform without overriding it
        T.DisplacementFieldTransform(Image(zero, is_vector=True)).GetInverse()
    with pytest.raises(TypeError):
        T.BSplineTransform((2, 2, 2), coefficients=torch.zeros((3, 5, 5, 5), dtype=torch.float32)).GetInverse()


def test_principal_axes_from_moments(host_api):
    pa = host_api
    shape, spacing = (30, 36, 40), (1.25, 1.1, 1.8)
    z, y, x = np.indices(shape).astype(np.float64)
    p = np.stack([x * spacing[0], y * spacing[1], z * spacing[2]], axis=-1) - np.array([25.0, 20.0, 27.0])
    from tests.helpers import rot_xyz

    q = p @ rot_xyz(20.0, -35.0, 50.0)
    arr = (((q[..., 0] / 20.0) ** 2 + (q[..., 1] / 9.0) ** 2 + (q[..., 2] / 14.0) ** 2) <= 1).astype(np.uint8)
    want_lam, want_axes = V.principal_axes(arr, spacing)
    moments = pa.label.label_moments(pa.image_from_array(arr.astype(np.int32), spacing), 1)
    lam, axes = pa.label.principal_axes_from_moments(moments[0], spacing)
    print("principal moments:", want_lam, "difference", np.abs(lam - want_lam).max())
    assert np.abs(lam - want_lam).max() <= 1e-12
    assert want_lam[0] < 0.7 * want_lam[1] < 0.7 * want_lam[2]      # well separated: the eigenvectors are well conditioned
    for k in range(3):
        s = np.sign(np.dot(axes[k], want_axes[k]))
        assert np.abs(axes[k] - s * want_axes[k]).max() <= 1e-12
    assert abs(np.linalg.norm(axes[0]) - 1) < 1e-14
    with pytest.raises(ValueError):
        pa.label.principal_axes_from_moments(np.zeros(10, np.int64), spacing)


# --------------------------------------------------------------------------------------
# the whole function

NAMES = ("Ventricle_L", "Atrium_L", "Ventricle_R", "Heart")
KEYS = [f"Ventricle_L_Segment{k}" for k in range(1, 18)]


def heart_phantom(shape=(60, 80, 84), spacing=(1.25, 1.1, 1.8), scale=1.0):
    """Tilted ellipsoid chambers ([Z][Y][X] uint8): the long axis l leans 25 degrees away from -z."""
    sp = np.asarray(spacing, dtype=np.float64)
    z, y, x = np.indices(shape).astype(np.float64)
    p = np.stack([x * sp[0], y * sp[1], z * sp[2]], axis=-1)
    c = 0.5 * np.asarray(size_of(shape), dtype=np.float64) * sp
    s25, c25 = np.sin(np.radians(25.0)), np.cos(np.radians(25.0))
    l = np.array([0.8 * s25, 0.6 * s25, -c25])
    l /= np.linalg.norm(l)
    u = np.cross(l, (0.0, 1.0, 0.0))
    u /= np.linalg.norm(u)
    v = np.cross(l, u)
    lv_c = c + 4.0 * scale * l

    def ellipsoid(centre, semi):
        d = p - centre
        return ((d @ u) / (semi[0] * scale)) ** 2 + ((d @ v) / (semi[1] * scale)) ** 2 + ((d @ l) / (semi[2] * scale)) ** 2 <= 1

    along = (p - lv_c) @ l
    heart = (((p - c) / (np.array([44.0, 44.0, 54.0]) * scale)) ** 2).sum(axis=-1) <= 1
    lv = ellipsoid(lv_c, (24, 24, 38)) & (along >= -14 * scale)
    la = ellipsoid(lv_c - 25 * scale * l, (16, 16, 11)) & (along < -14 * scale)
    rv = ellipsoid(lv_c + 24 * scale * u + 2 * scale * l, (16, 24, 40)) & ~lv & ~la & (along >= -14 * scale)
    return {n: a.astype(np.uint8) for n, a in zip(NAMES, (lv, la, rv, heart))}


ORIGIN = (0.0, 0.0, 0.0)
SPACING = (1.25, 1.1, 1.8)
_WANT = {}


def restated(key, arrays, spacing, **kw):
    """The restatement, computed once per case and left unchanged."""
    if key not in _WANT:
        info = {}
        segs = V.left_ventricle_segments(*[arrays[n] for n in NAMES], spacing, ORIGIN, info=info, **kw)
        for s in segs:
            s.setflags(write=False)
        _WANT[key] = (segs, info)
    return _WANT[key]


def images(pa, arrays, spacing, names=NAMES):
    return {k: pa.image_from_array(arrays[n], spacing, ORIGIN) for k, n in zip(names, NAMES)}


def check_preconditions(info):
    assert info["angle_gap"] > 1e-9 and info["radius_gap"] > 1e-9 and info["half_gap"] > 1e-9, info


def test_left_ventricle_segments_against_the_restatement(host_api):
    pa = host_api
    arrays = heart_phantom()
    want, winfo = restated("full", arrays, SPACING)
    # 1. preconditions, on the restatement alone
    check_preconditions(winfo)
    print("restatement:", {k: winfo[k] for k in ("rotation_angles", "inf_limit_lv", "apical_extent", "mid_extent", "basal_extent", "theta_0",
                                                  "theta_0_apical", "angle_gap", "angle_ties", "radius_gap", "half_gap", "suppressed")})
    assert winfo["inf_limit_lv"] < winfo["apical_extent"] < winfo["mid_extent"] < winfo["basal_extent"]
    assert len(winfo["rotation_angles"]) >= 3 and winfo["suppressed"] >= 1 and winfo["angle_ties"] >= 1
    assert all(w.sum() > 100 for w in want)
    assert (np.sum([w != 0 for w in want], axis=0) >= 2).any()      # V5: voxels in two segments
    src = images(pa, arrays, SPACING)
    before = {k: v.numpy().copy() for k, v in src.items()}
    info = {}
    got = pa.utils.generate_left_ventricle_segments(src, info=info)
    # 2. the scalars
    for k in ("rotation_angles", "rotation_centres", "rotation_axes", "theta_0", "theta_0_apical"):
        assert np.abs(np.asarray(info[k]) - np.asarray(winfo[k])).max() <= 1e-9, k
    for k in ("inf_limit_lv", "apical_extent", "mid_extent", "basal_extent", "slice_origins"):
        assert info[k] == winfo[k], k
    assert np.array_equal(info["counts"], winfo["counts"])
    # 3. the masks
    assert list(got) == KEYS
    for k, w in zip(KEYS, want):
        g = got[k]
        assert g.GetSize() == src["Heart"].GetSize() and g.GetSpacing() == src["Heart"].GetSpacing() and g.tensor.dtype == torch.uint8
        assert np.array_equal(g.numpy(), w), (k, int(g.numpy().sum()), int(w.sum()))
    # 4. a second call, and the inputs
    again = pa.utils.generate_left_ventricle_segments(src)
    assert all(np.array_equal(again[k].numpy(), got[k].numpy()) for k in KEYS)
    assert all(np.array_equal(src[k].numpy(), before[k]) for k in src)


SMALL_SHAPE = (40, 56, 56)
SMALL_KW = {"optimiser_tol_degrees": 2}      # the two-thirds phantom settles at 1.56 degrees per trip: stop there, after three rotations


def small_phantom():
    return heart_phantom(SMALL_SHAPE, SPACING, 2.0 / 3.0)


@pytest.mark.parametrize("kw", [{"hole_fill_mm": 0}, {"min_area_mm2": 0}, {"min_area_mm2": 150}], ids=["no-closing", "no-area-test", "area-150"])
def test_left_ventricle_segments_options(host_api, kw):
    pa = host_api
    arrays = small_phantom()
    kw = dict(kw, **SMALL_KW)
    want, winfo = restated(("small", tuple(sorted(kw.items()))), arrays, SPACING, **kw)
    check_preconditions(winfo)
    assert len(winfo["rotation_angles"]) == 3
    if kw.get("min_area_mm2") == 0:
        other, oinfo = restated(("small", tuple(sorted(dict(kw, min_area_mm2=150).items()))), arrays, SPACING, **dict(kw, min_area_mm2=150))
        assert winfo["suppressed"] == 0 and oinfo["suppressed"] >= 1 and any(not np.array_equal(a, b) for a, b in zip(want, other))
    if kw.get("hole_fill_mm") == 0:
        other, _ = restated(("small", tuple(sorted(dict(kw, hole_fill_mm=3).items()))), arrays, SPACING, **dict(kw, hole_fill_mm=3))
        assert any(not np.array_equal(a, b) for a, b in zip(want, other))      # the closing does change the result
    # other names through the label_* arguments
    src = images(pa, arrays, SPACING, ("lv", "la", "rv", "wh"))
    before = {k: v.numpy().copy() for k, v in src.items()}
    got = pa.utils.generate_left_ventricle_segments(src, "lv", "la", "rv", "wh", **kw)
    assert list(got) == KEYS
    for k, w in zip(KEYS, want):
        assert np.array_equal(got[k].numpy(), w), k
    assert all(np.array_equal(src[k].numpy(), before[k]) for k in src)


def test_left_ventricle_segments_refuses_large_radii_by_name(host_api):
    pa = host_api
    arrays = heart_phantom((12, 16, 16), (0.5, 0.5, 0.5), 0.1)
    with pytest.raises(ValueError, match="generate_left_ventricle_segments.*limit of 15 voxels"):
        pa.utils.generate_left_ventricle_segments(images(pa, arrays, (0.5, 0.5, 0.5)))


def test_left_ventricle_segments_missing_right_ventricle(host_api):
    """V9.  The rotations depend on LV, LA and the heart only, so the restatement's inverse transform tells which input voxels
    land in the apical slices of the aligned frame; the RV is removed there (and two slices beyond)."""
    pa = host_api
    from tests import cardiac_geometry_restatement as G

    arrays = dict(small_phantom())
    _, binfo = restated(("small", tuple(sorted(dict(SMALL_KW, hole_fill_mm=0).items()))), arrays, SPACING, hole_fill_mm=0, **SMALL_KW)
    A, t = binfo["inverse"]                     # a point of the input image -> the same point in the aligned frame
    size, index = G.label_to_roi(arrays["Heart"] > 0, SPACING, (30, 30, 60))
    org = np.asarray(ORIGIN) + np.asarray(SPACING) * np.asarray(index)
    grid = R.Grid(size, SPACING, org)
    p = grid.index_to_physical(grid.indices())
    aligned_z = ((p @ A.T + t) - org)[..., 2] / SPACING[2]
    cut = G.paste(arrays["Heart"].shape, (aligned_z < binfo["apical_extent"] + 2).astype(np.uint8), index).astype(bool)
    rv = arrays["Ventricle_R"].copy()
    rv[cut] = 0
    assert rv.any() and rv.sum() < arrays["Ventricle_R"].sum()
    src = images(pa, arrays, SPACING)
    src["Ventricle_R"] = pa.image_from_array(rv, SPACING, ORIGIN)
    with pytest.raises(ValueError, match="right ventricle is absent from slice"):
        pa.utils.generate_left_ventricle_segments(src, **SMALL_KW)
