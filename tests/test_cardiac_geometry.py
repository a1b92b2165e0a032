"""The cardiac geometry stages -- vessel splining (pp_slice_moments_u8, pp_tube_mask_u8, utils/vessel.py), shapes
(generation/image.py), rotate_image (utils/geometry.py) -- against tests/cardiac_geometry_restatement.py, the reference's
arithmetic in fp64 numpy / scipy.

Bounds (none is tuned):
  * moments, masks, shapes, nearest-neighbour rotation: np.array_equal;
  * the tube: the brute-force fp64 distance of the definition; the test first asserts that NO voxel of the reference lies
    within 1e-6 mm of the radius (fp64 rounding of a distance of a few hundred mm is ~1e-13 mm), then demands equality
    everywhere;
  * get_com: 1e-12 (two fp64 roundings of exact integer sums), exact with as_int;
  * the spline: 1e-10 mm against scipy.interpolate.CubicSpline with clamped ends;
  * linear rotation: 24 * 2^-24 * max|image| (tests/test_resample_kernels.py's bound for the fp64-coordinate kernels).
"""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import cardiac_geometry_restatement as G
from tests import resample_restatement as R

SHAPE, SPACING, ORIGIN = (24, 32, 40), (1.0, 1.2, 2.5), (-20.0, 13.5, 100.25)      # the grid of tests/test_generation.py
NN, LINEAR = 1, 2


def p(i, j, k, spacing=SPACING, origin=ORIGIN):
    return (origin[0] + i * spacing[0], origin[1] + j * spacing[1], origin[2] + k * spacing[2])


def size_of(shape):
    return (shape[2], shape[1], shape[0])


def sphere01(shape=SHAPE):
    z, y, x = np.indices(shape).astype(np.float64)
    c = [(s - 1) / 2.0 + 0.3 for s in shape]
    r = [max(s / 3.0, 1.0) for s in shape]
    return ((((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2) <= 1).astype(np.uint8)


def box255(shape=SHAPE):
    m = np.zeros(shape, np.uint8)
    m[0:max(shape[0] // 3, 1), 0:max(shape[1] // 2, 1), 0:max(shape[2] // 4, 1)] = 255      # touches index 0 on every axis
    return m


def three_masks(shape=SHAPE):
    return [sphere01(shape), box255(shape), np.zeros(shape, np.uint8)]


# --------------------------------------------------------------------------------------
# pp_slice_moments_u8


def run_moments(backend, masks, axis, offset=0):
    shape = masks[0].shape
    if offset:      # masks that start `offset` bytes into their allocation: the unaligned path
        bufs = [backend.dev(np.concatenate([np.zeros(offset, np.uint8), m.ravel()])) for m in masks]
        dev = [b[offset:] for b in bufs]
    else:
        dev = [backend.dev(m) for m in masks]
    nslices = size_of(shape)[axis]
    out = backend.dev(np.full((len(masks), nslices, 4), -7, np.int64))
    backend.ctx.slice_moments(dev, size_of(shape), axis, out)
    return backend.host(out)


@pytest.mark.parametrize("scan", ["z", "x"])
@pytest.mark.parametrize("shape", [SHAPE, (5, 9, 37), (1, 7, 19), (6, 5, 1), (3, 4, 1040)], ids=str)
def test_slice_moments(backend, shape, scan):
    masks = three_masks(shape)
    want = G.slice_moments(masks, scan)
    got = run_moments(backend, masks, 0 if scan == "x" else 2)
    assert np.array_equal(got, want)
    assert np.array_equal(run_moments(backend, masks, 0 if scan == "x" else 2), got)      # a rerun gives the same bits


@pytest.mark.parametrize("scan", ["z", "x"])
def test_slice_moments_unaligned_masks_and_random_values(backend, scan):
    rng = np.random.default_rng(5)
    shape = (7, 16, 48)     # nx % 16 == 0: only the pointers keep the 16-byte loads away
    masks = [(rng.integers(0, 256, shape) * (rng.random(shape) < 0.3)).astype(np.uint8) for _ in range(4)]
    want = G.slice_moments(masks, scan)
    assert np.array_equal(run_moments(backend, masks, 0 if scan == "x" else 2, offset=3), want)
    assert np.array_equal(run_moments(backend, masks, 0 if scan == "x" else 2), want)


def test_slice_moments_refuses_other_axes_and_counts(backend):
    m = backend.dev(sphere01((4, 5, 6)))
    out = backend.dev(np.zeros((1, 6, 4), np.int64))
    for axis in (1, 3, -1):
        with pytest.raises(ValueError):
            backend.ctx.slice_moments([m], (6, 5, 4), axis, out)
    with pytest.raises(ValueError):
        backend.ctx.slice_moments([m] * 65, (6, 5, 4), 2, out)
    with pytest.raises(ValueError):
        backend.ctx.slice_moments([], (6, 5, 4), 2, out)


def test_get_com(host_api):
    pa = host_api
    for arr in (sphere01(), box255(), sphere01((5, 9, 37)) * 3):
        img = pa.image_from_array(arr, SPACING, ORIGIN)
        want = ndimage.center_of_mass(arr)
        got = pa.label.utils.get_com(img, as_int=False)
        assert np.allclose(got, want, rtol=0, atol=1e-12)
        assert pa.label.utils.get_com(img) == [int(i) for i in want]
        real = pa.label.utils.get_com(img, real_coords=True)
        assert np.allclose(real, np.asarray(ORIGIN) + np.asarray(SPACING) * np.asarray(want[::-1]), rtol=0, atol=1e-10)
    with pytest.raises(ValueError):
        pa.label.utils.slice_moments([pa.image_from_array(sphere01(), SPACING, ORIGIN)], "y")


# --------------------------------------------------------------------------------------
# pp_tube_mask_u8

LINES = {
    "z-run": [p(6 + 0.31 * k + 0.4 * (k % 3), 9 + 0.17 * k * k / 4, k) for k in range(3, 21)],
    "x-run": [p(i, 20 - 0.21 * i + 0.3 * (i % 2), 5 + 0.33 * i) for i in range(2, 37, 2)],
    "through": [p(-3.3, 4.2, 2.1), p(8.7, 10.4, 9.6), p(22.2, 30.9, 14.3), p(44.1, 35.5, 26.2)],
    "two": [p(5.2, 6.1, 4.3), p(30.4, 25.3, 19.8)],
}
RADII = [2.0, 3.7, 0.45]


def run_tube(backend, polyline, shape, spacing, origin, radius):
    out = backend.dev(np.full(shape, 9, np.uint8))
    backend.ctx.tube_mask(np.asarray(polyline, dtype=np.float64), size_of(shape), spacing, origin, radius, out)
    return backend.host(out)


def check_tube(backend, polyline, radius, shape=SHAPE, spacing=SPACING, origin=ORIGIN, at_least=1):
    dist = G.tube_distance(polyline, shape, spacing, origin)
    assert not np.any(np.abs(dist - radius) <= 1e-6), "the reference has a near-tie voxel: the case decides nothing"
    want = (dist <= radius).astype(np.uint8)
    assert want.sum() >= at_least
    got = run_tube(backend, polyline, shape, spacing, origin, radius)
    assert np.array_equal(got, want), (int(got.sum()), int(want.sum()), np.argwhere(got != want)[:5])
    assert np.array_equal(run_tube(backend, polyline, shape, spacing, origin, radius), got)
    return want


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("line", sorted(LINES))
def test_tube_mask_splined_centrelines(backend, line, radius):
    check_tube(backend, G.centreline(LINES[line]), radius, at_least=10)


def test_tube_mask_duplicated_points(backend):
    a, b, c = p(5.2, 6.1, 4.3), p(18.4, 15.3, 9.8), p(30.4, 25.3, 19.8)
    plain = check_tube(backend, [a, b, c], 2.0)
    assert np.array_equal(check_tube(backend, [a, b, b, c], 2.0), plain)
    assert np.array_equal(check_tube(backend, [a, a, b, c, c], 2.0), plain)      # the flat ends move to the segments that remain
    for bad in ([a, a], [a, a, a], [a]):
        with pytest.raises(ValueError):
            run_tube(backend, bad, SHAPE, SPACING, ORIGIN, 2.0)


def test_tube_mask_more_segments_than_one_chunk(backend):
    """1500 segments, all of them within reach of the same bricks: the LDS list (512 entries) is used and restarted."""
    t = np.linspace(0.0, 1.0, 1501)[:, None]
    a, b = np.array(p(9.3, 9.4, 2.2)), np.array(p(14.1, 13.2, 3.1))
    line = a + t * (b - a) + 0.05 * np.stack([np.sin(40 * t[:, 0]), np.cos(31 * t[:, 0]), np.sin(17 * t[:, 0])], axis=1)
    check_tube(backend, line, 2.0, at_least=10)


@pytest.mark.parametrize("shape", [(6, 19, 37), (9, 18, 48), (5, 16, 16), (3, 7, 5)], ids=str)
def test_tube_mask_odd_volumes(backend, shape):
    """Sizes that are no multiple of the 16 x 16 x 4 brick: nx % 4 != 0 (byte stores), nx % 16 == 0 (16-byte rows of empty
    bricks), and a volume smaller than one brick."""
    nz, ny, nx = shape
    line = [p(0.6, 0.7, 0.2), p(nx * 0.55, ny * 0.35, nz * 0.6), p(nx - 1.3, ny - 1.6, nz - 1.2)]
    check_tube(backend, line, 1.7, shape=shape)


def test_tube_mask_flat_ends(backend):
    line = [p(10, 16, 12), p(20, 16, 12)]
    want = check_tube(backend, line, 2.0)
    assert want[12, 16, 10] == 1 and want[12, 16, 20] == 1 and want[12, 16, 15] == 1
    assert want[12, 16, 9] == 0 and want[12, 16, 21] == 0      # 1 mm behind the first / beyond the last point: no cap
    assert want[12, 17, 10] == 1 and want[12, 17, 9] == 0


# --------------------------------------------------------------------------------------
# utils/vessel.py


@pytest.mark.parametrize("line", sorted(LINES))
def test_spline_against_scipy(host_api, line):
    pa = host_api
    tube = pa.utils.vessel.tube_from_com_list(LINES[line], 2.0)
    want = G.centreline(LINES[line])
    assert tube.shape == (10 * len(LINES[line]) + 1, 3) and tube.dtype == np.float64 and tube.radius == 2.0
    assert np.abs(np.asarray(tube) - want).max() <= 1e-10
    assert np.abs(np.asarray(tube)[[0, -1]] - np.asarray(LINES[line])[[0, -1]]).max() <= 1e-10      # it interpolates its end points


def vessel_atlases(n=4, shape=SHAPE, values=(1, 1, 255, 1)):
    """n propagated labels of one thin vessel running along z and drifting in x / y, each atlas shifted a little."""
    out = []
    for a in range(n):
        m = np.zeros(shape, np.uint8)
        for k in range(2 + a % 2, shape[0] - 3 - a):
            y, x = int(6 + 0.8 * k + a), int(8 + 0.5 * k + (a % 3))
            m[k, y:y + 2, x:x + 3] = values[a % len(values)]
        out.append(m)
    return out


@pytest.mark.parametrize("scan,cond,value", [("z", "count", 0), ("z", "count", 2), ("z", "area", 600), ("x", "count", 1), ("x", "area", 0)])
def test_com_from_image_list(host_api, scan, cond, value):
    pa = host_api
    arrays = vessel_atlases()
    arrays[1][5, 0, 0:3] = 1      # V1: a slice whose centre of mass sits in row 0 ...
    arrays[1][5, 1:, :] = 0
    images = [pa.image_from_array(a, SPACING, ORIGIN) for a in arrays]
    want = G.com_from_array_list(arrays, SPACING, ORIGIN, cond, value, scan)
    got = pa.utils.vessel.com_from_image_list(images, cond, value, scan)
    assert len(want) >= 3
    assert np.array_equal(np.asarray(got), np.asarray(want))


def test_com_from_image_list_errors(host_api):
    pa = host_api
    images = [pa.image_from_array(a, SPACING, ORIGIN) for a in vessel_atlases(2)]
    with pytest.raises(ValueError):
        pa.utils.vessel.com_from_image_list(images, "count", 0, "y")
    with pytest.raises(ValueError):
        pa.utils.vessel.com_from_image_list(images, "volume", 0, "z")


def test_vessel_spline_generation(host_api, caplog):
    pa = host_api
    arrays = vessel_atlases()
    direction = (0, 1, 0, -1, 0, 0, 0, 0, 1)
    atlas_set = {f"a{k}": {"DIR": {"LAD": pa.Image(torch.from_numpy(a).to(pa.runtime.default_device()), SPACING, ORIGIN, direction),
                                   "EMPTY": pa.image_from_array(np.zeros(SHAPE, np.uint8), SPACING, ORIGIN)}} for k, a in enumerate(arrays)}
    ref = atlas_set["a0"]["DIR"]["LAD"]
    names = ["LAD", "EMPTY", "MISSING"]
    out = pa.utils.vessel.vessel_spline_generation(ref, atlas_set, names, {n: 2.0 for n in names}, {n: "count" for n in names},
                                                   {n: 1 for n in names}, {n: "z" for n in names})
    assert sorted(out) == ["EMPTY", "LAD"]
    points = G.com_from_array_list(arrays, SPACING, ORIGIN, "count", 1, "z")
    dist = G.tube_distance(G.centreline(points), SHAPE, SPACING, ORIGIN)
    assert not np.any(np.abs(dist - 2.0) <= 1e-6)
    assert np.array_equal(out["LAD"].numpy(), (dist <= 2.0).astype(np.uint8)) and out["LAD"].numpy().sum() > 50
    assert out["LAD"].GetDirection() == direction and ref.GetDirection() == direction      # V6: forced to identity, then restored
    assert out["EMPTY"].numpy().sum() == 0                                                  # fewer than two points: empty, a warning
    assert any("Fewer than two" in r.message for r in caplog.records)


# --------------------------------------------------------------------------------------
# generation/image.py


@pytest.mark.parametrize("radius,centre", [(4, (10, 12, 20)), ((3, 5.5, 7.25), (11.5, 0, 39)), (2.5, (-1, 31, 3.2))])
def test_insert_sphere(host_api, radius, centre):
    pa = host_api
    base = box255() // 255 * 3
    got = pa.generation.image.insert_sphere(torch.from_numpy(base.copy()).to(pa.runtime.default_device()), radius, centre)
    assert np.array_equal(got.cpu().numpy(), G.insert_sphere(base.copy(), radius, centre))
    img = pa.image_from_array(base, SPACING, ORIGIN)
    got = pa.generation.image.insert_sphere_image(img, radius, centre)
    assert np.array_equal(got.numpy(), G.insert_sphere_image(base, SPACING, radius, centre))
    assert np.array_equal(img.numpy(), base)      # the image itself is not written to


@pytest.mark.parametrize("radius,height,centre", [(4, 2, (20, 12, 10)), ((3, 5.5), 7, (39, 0, 11.5)), (2.5, 5, (3.2, 31, -1))])
def test_insert_cylinder(host_api, radius, height, centre):
    pa = host_api
    base = box255() // 255 * 3
    t = torch.from_numpy(base.copy()).to(pa.runtime.default_device())
    got = pa.generation.image.insert_cylinder(t, radius, height, centre)
    want = G.insert_cylinder(base.copy(), radius, height, centre)
    assert np.array_equal(got.cpu().numpy(), want) and want.sum() != base.sum()
    assert np.array_equal(t.cpu().numpy(), want)      # written in place, as the reference's arr[:] view is
    img = pa.image_from_array(base, SPACING, ORIGIN)
    got = pa.generation.image.insert_cylinder_image(img, radius, height, centre)
    assert np.array_equal(got.numpy(), G.insert_cylinder_image(base, SPACING, radius, height, centre))


# --------------------------------------------------------------------------------------
# utils/geometry.py

ROT_SHAPE, ROT_SPACING, ROT_ORIGIN = (10, 21, 25), (1.5, 1.5, 2.5), (-7.5, 4.0, 30.0)


def rotated(arr, centre, axis, angle, interp, default, u8):
    A = G.versor_matrix(axis, angle)
    c = np.asarray(centre, dtype=np.float64)
    g = R.Grid(size_of(ROT_SHAPE), ROT_SPACING, ROT_ORIGIN)
    return R.resample(arr, g, g, A, c - A @ c, interp=interp, default=default, u8=u8)


def test_vector_angle_and_zero_axis(host_api):
    pa = host_api
    assert abs(pa.utils.geometry.vector_angle((1, 0, 0), (0, 2, 0)) - np.pi / 2) < 1e-15
    assert abs(pa.utils.geometry.vector_angle((1, 0, 0), (-1, 1, 0)) - np.pi / 4) < 1e-15
    assert abs(pa.utils.geometry.vector_angle((1, 0, 0), (-1, 1, 0), smallest=False) - 3 * np.pi / 4) < 1e-15
    img = pa.image_from_array(np.zeros(ROT_SHAPE, np.uint8), ROT_SPACING, ROT_ORIGIN)
    with pytest.raises(ValueError):
        pa.utils.geometry.rotate_image(img, rotation_axis=(0, 0, 0), rotation_angle_radians=1.0)


def test_rotate_image_quarter_turn_is_a_permutation(host_api):
    pa = host_api
    rng = np.random.default_rng(2)
    arr = (rng.random(ROT_SHAPE) < 0.4).astype(np.uint8)
    centre = (ROT_ORIGIN[0] + 12 * 1.5, ROT_ORIGIN[1] + 10 * 1.5, ROT_ORIGIN[2] + 4 * 2.5)      # voxel (12, 10, 4)
    img = pa.image_from_array(arr, ROT_SPACING, ROT_ORIGIN)
    got = pa.utils.geometry.rotate_image(img, centre, (0, 0, 1), np.pi / 2).numpy()
    want = rotated(arr, centre, (0, 0, 1), np.pi / 2, "nearest", 0, True)["out"]
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # out(x, y) = in(cx - (y - cy), cy + (x - cx)): every output voxel whose source is inside the image is a copy of it
    z, y, x = np.indices(ROT_SHAPE)
    sx, sy = 12 - (y - 10), 10 + (x - 12)
    ok = (sx >= 0) & (sx < ROT_SHAPE[2]) & (sy >= 0) & (sy < ROT_SHAPE[1])
    assert np.array_equal(got[ok], arr[z[ok], sy[ok], sx[ok]]) and not got[~ok].any()


def test_rotate_image_oblique(host_api):
    pa = host_api
    rng = np.random.default_rng(3)
    arr = ndimage.gaussian_filter(rng.normal(0, 100, ROT_SHAPE), 1.5).astype(np.float32)
    mask = (arr > 5).astype(np.uint8)
    centre, axis, angle = (10.3, 19.1, 41.7), (1, 2, 3), 0.7
    got = pa.utils.geometry.rotate_image(pa.image_from_array(mask, ROT_SPACING, ROT_ORIGIN), centre, axis, angle).numpy()
    assert np.array_equal(got, rotated(mask, centre, axis, angle, "nearest", 0, True)["out"]) and got.sum() > 100
    got = pa.utils.geometry.rotate_image(pa.image_from_array(arr, ROT_SPACING, ROT_ORIGIN), centre, axis, angle, LINEAR, -3).numpy()
    want = rotated(arr, centre, axis, angle, "linear", -3.0, False)
    assert np.abs(got - want["out"]).max() <= 24 * 2.0 ** -24 * np.abs(arr).max()
    assert np.array_equal(got == -3, ~want["inside"]) or np.abs(got[~want["inside"]] + 3).max() == 0


# --------------------------------------------------------------------------------------
# utils/valve.py, utils/conduction.py

HEART_SHAPE, HEART_SPACING, HEART_ORIGIN = (48, 64, 64), (1.5, 1.5, 2.5), (-48.0, -40.0, 12.5)
CHAMBERS = ("LEFTVENTRICLE", "RIGHTVENTRICLE", "LEFTATRIUM", "RIGHTATRIUM", "ASCENDINGAORTA", "PULMONARYARTERY", "SVC", "WHOLEHEART")


def heart_phantom(shift=(0, 0, 0), shape=HEART_SHAPE):
    """Ellipsoid chambers and cylindrical great vessels ([Z][Y][X] uint8, 0 / 1), placed so that every loop of the geometric
    definitions runs more than once: atria and ventricles start apart or barely overlapping (the cylinder valves dilate
    several times), the SVC stands clear of the right atrium (the sinoatrial loop dilates in plane, then axially), and the
    left ventricle overlaps the left atrium on the atrioventricular slice (its erosion loop runs three times).
    `shift` (x, y, z voxels) moves everything, e.g. against the border of the image."""
    z, y, x = np.indices(shape).astype(np.float64)
    x, y, z = x - shift[0], y - shift[1], z - shift[2]

    def ellipsoid(c, r):
        return ((((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2) <= 1).astype(np.uint8)

    def cylinder(c, r, z0, z1):
        return ((((x - c[0]) ** 2 + (y - c[1]) ** 2) <= r * r) & (z >= z0) & (z <= z1)).astype(np.uint8)

    out = {"LEFTVENTRICLE": ellipsoid((40, 36, 18), (11, 11, 13)), "RIGHTVENTRICLE": ellipsoid((24, 28, 18), (8, 8, 10)),
           "LEFTATRIUM": ellipsoid((40, 48, 31), (8, 8, 7)), "RIGHTATRIUM": ellipsoid((24, 38, 27), (7, 7, 7)),
           "ASCENDINGAORTA": cylinder((40, 32), 4, 27, 44), "PULMONARYARTERY": cylinder((24, 24), 4, 26, 44),
           "SVC": cylinder((13, 48), 3, 31, 44), "WHOLEHEART": ellipsoid((32, 38, 25), (27, 25, 23))}
    return out


HEARTS = {"centred": ((0, 0, 0), HEART_SPACING), "border": ((14, -12, -6), HEART_SPACING), "anisotropic": ((0, 0, 0), (1.0, 1.7, 3.0))}


@pytest.fixture(scope="module", params=sorted(HEARTS))
def heart(request):
    shift, spacing = HEARTS[request.param]
    return request.param, heart_phantom(shift), spacing


def heart_images(pa, arrays, spacing):
    return {k: pa.image_from_array(v, spacing, HEART_ORIGIN) for k, v in arrays.items()}


@pytest.mark.parametrize("vessel,ventricle", [("ASCENDINGAORTA", "LEFTVENTRICLE"), ("PULMONARYARTERY", "RIGHTVENTRICLE")])
def test_valve_from_great_vessel(host_api, heart, vessel, ventricle):
    pa = host_api
    name, arrays, spacing = heart
    images = heart_images(pa, arrays, spacing)
    want = G.valve_from_great_vessel(arrays[vessel], arrays[ventricle], spacing, 10)
    got = pa.utils.valve.generate_valve_from_great_vessel(images[vessel], images[ventricle], 10).numpy()
    assert want.sum() > 20 and np.array_equal(got, want)


@pytest.mark.parametrize("atrium,ventricle", [("LEFTATRIUM", "LEFTVENTRICLE"), ("RIGHTATRIUM", "RIGHTVENTRICLE")])
def test_valve_using_cylinder(host_api, heart, atrium, ventricle):
    pa = host_api
    name, arrays, spacing = heart
    images = heart_images(pa, arrays, spacing)
    info = {}
    want = G.valve_using_cylinder(arrays[atrium], arrays[ventricle], spacing, HEART_ORIGIN, 15, 10, info)
    assert info["dilations"] > 1      # the loop ran more than once
    got = pa.utils.valve.generate_valve_using_cylinder(images[atrium], images[ventricle], 15, 10).numpy()
    assert want.sum() > 100 and np.array_equal(got, want)


def test_sinoatrialnode(host_api, heart):
    pa = host_api
    name, arrays, spacing = heart
    images = heart_images(pa, arrays, spacing)
    info = {}
    want = G.sinoatrialnode(arrays["SVC"], arrays["RIGHTATRIUM"], arrays["WHOLEHEART"], spacing, 10, info)
    assert info["dilations"] > 2      # in plane first, then axially too
    got = pa.utils.conduction.geometric_sinoatrialnode(images["SVC"], images["RIGHTATRIUM"], images["WHOLEHEART"], 10).numpy()
    assert want.sum() > 100 and np.array_equal(got, want)


def test_atrioventricularnode(host_api, heart):
    pa = host_api
    name, arrays, spacing = heart
    images = heart_images(pa, arrays, spacing)
    info = {}
    args = ("LEFTATRIUM", "LEFTVENTRICLE", "RIGHTATRIUM", "RIGHTVENTRICLE")
    want = G.atrioventricularnode(*[arrays[k] for k in args], spacing, 10, info)
    assert info["erosions"] > 1
    got = pa.utils.conduction.geometric_atrioventricularnode(*[images[k] for k in args], 10).numpy()
    assert want.sum() > 100 and np.array_equal(got, want)


def test_one_slice_volumes(host_api):
    """The 2-D steps: ball morphology with radius (e, e, 0) and the Maurer map on volumes with size[2] == 1, and the first
    minimum in raster order."""
    pa = host_api
    arrays = heart_phantom()
    a = arrays["LEFTVENTRICLE"][18:19]
    b = arrays["RIGHTVENTRICLE"][18:19]
    img = pa.image_from_array(a, HEART_SPACING, HEART_ORIGIN)
    for e in (1, 2, 5):
        assert np.array_equal(pa.label.binary_erode(img, (e, e, 0)).numpy(), G.erode(a, HEART_SPACING, (e, e, 0)))
        assert np.array_equal(pa.label.binary_dilate(img, (e, e, 0)).numpy(), G.dilate(a, HEART_SPACING, (e, e, 0)))
    d = pa.label.distance_map(img, signed=True).numpy()
    assert np.abs(d - G.signed_distance(a, HEART_SPACING)).max() <= 1e-4
    got = pa.utils.conduction.get_closest_point_2d(img, pa.image_from_array(b, HEART_SPACING, HEART_ORIGIN))
    assert got == tuple(int(v) for v in G.closest_point_2d(a[0], b[0], HEART_SPACING))
    # a tie: two voxels at the same distance from a single reference voxel -- the first in raster order wins
    ref = np.zeros((1, 9, 9), np.uint8)
    ref[0, 4, 4] = 1
    meas = np.zeros((1, 9, 9), np.uint8)
    meas[0, 4, 7] = meas[0, 7, 4] = meas[0, 1, 4] = 1
    iso = (1.0, 1.0, 2.0)
    assert pa.utils.conduction.get_closest_point_2d(pa.image_from_array(ref, iso), pa.image_from_array(meas, iso)) == (1, 4)


def test_dilation_limit_is_named(host_api):
    pa = host_api
    images = heart_images(pa, heart_phantom(), HEART_SPACING)
    with pytest.raises(ValueError, match="limit of 15 voxels"):
        pa.utils.valve.generate_valve_from_great_vessel(images["ASCENDINGAORTA"], images["LEFTVENTRICLE"], 50)


# --------------------------------------------------------------------------------------
# the pipeline: run_cardiac_segmentation(..., geometry_stages=True)

VESSELS = ["LANTDESCARTERY", "LCIRCUMFLEXARTERY", "LCORONARYARTERY", "RCORONARYARTERY"]
NEW_KEYS = VESSELS + ["Valve_Mitral", "Valve_Tricuspid", "Valve_Aortic", "Valve_Pulmonic", "CN_Sinoatrial", "CN_Atrioventricular"]


def pipeline_subject(shift):
    """One synthetic subject: the phantom's chambers, four thin vessels (three along z, the left coronary along x) and a
    CT-like image made of them."""
    labels = heart_phantom(shift)
    z, y, x = np.indices(HEART_SHAPE)
    x, y, z = x - shift[0], y - shift[1], z - shift[2]
    labels["LANTDESCARTERY"] = ((np.abs(x - (30 + 0.4 * z)) <= 1) & (np.abs(y - (22 + 0.3 * z)) <= 1) & (z >= 8) & (z <= 30)).astype(np.uint8)
    labels["LCIRCUMFLEXARTERY"] = ((np.abs(x - (48 - 0.2 * z)) <= 1) & (np.abs(y - (40 + 0.2 * z)) <= 1) & (z >= 10) & (z <= 28)).astype(np.uint8)
    labels["RCORONARYARTERY"] = ((np.abs(x - (16 + 0.1 * z)) <= 1) & (np.abs(y - (30 + 0.3 * z)) <= 1) & (z >= 9) & (z <= 29)).astype(np.uint8)
    labels["LCORONARYARTERY"] = ((np.abs(z - (30 - 0.15 * x)) <= 1) & (np.abs(y - (26 + 0.2 * x)) <= 1) & (x >= 22) & (x <= 44)).astype(np.uint8)
    ct = np.where(labels["WHOLEHEART"] != 0, 0.0, -1000.0)
    for k, name in enumerate(CHAMBERS[:-1]):
        ct[labels[name] != 0] = 40.0 + 30.0 * k
    return ct.astype(np.float32), labels


def pipeline_case(pa, ids=("01", "02")):
    """-> (target image, atlases in memory, settings): the reference's default settings with the atlas list, the structure
    list and -- as tests/test_cardiac.py does for the CPU suite -- shorter registration schedules replaced."""
    shifts = {"01": (1, 0, 0), "02": (0, 1, 1), "03": (-1, 0, 0)}
    atlases = {}
    for cid in ids:
        ct, labels = pipeline_subject(shifts[cid])
        atlases[cid] = {"CT Image": pa.image_from_array(ct, HEART_SPACING, HEART_ORIGIN),
                        **{k: pa.image_from_array(v, HEART_SPACING, HEART_ORIGIN) for k, v in labels.items()}}
    ct, _ = pipeline_subject((0, 0, 0))
    s = __import__("copy").deepcopy(pa.projects.cardiac.CARDIAC_SETTINGS_DEFAULTS)
    s["atlas_settings"]["atlas_id_list"] = list(ids)
    s["atlas_settings"]["atlas_structure_list"] = list(CHAMBERS) + VESSELS
    s["linear_registration_settings"].update({"shrink_factors": [4, 2], "number_of_iterations": 15})
    s["auto_crop_target_image_settings"]["expansion_mm"] = [12, 12, 20]
    s["deformable_registration_settings"].update({"resolution_staging": [8, 4], "iteration_staging": [5, 5], "default_value": -1000})
    s["vessel_spline_settings"]["stop_condition_value_dict"] = {v: 0 for v in VESSELS}      # two atlases: one is enough
    return pa.image_from_array(ct, HEART_SPACING, HEART_ORIGIN), atlases, s


_PIPELINE_RUNS = {}


def run_pipelines(kind):
    """The pipeline three times on one case, and the stage functions applied by hand to the first run's atlas set; computed
    once per backend ("emu": the CPU emulation, "gpu")."""
    import copy

    import platipy_amd as pa

    if kind in _PIPELINE_RUNS:
        return _PIPELINE_RUNS[kind]
    patch = pytest.MonkeyPatch()
    try:
        if kind == "emu":
            from tests.helpers import install_emu_runtime

            install_emu_runtime(lambda obj, name, value: patch.setattr(obj, name, value, raising=False))
        run = pa.projects.cardiac.run_cardiac_segmentation
        target, atlases, settings = pipeline_case(pa)
        out = {"settings": settings, "target": target}
        s = copy.deepcopy(settings)
        s["return_as_cropped"] = True
        s["postprocessing_settings"]["run_postprocessing"] = False
        out["cropped"] = run(target, settings=s, atlases=atlases, geometry_stages=True, return_atlas_set=True)
        out["centrelines"] = {k: v.copy() for k, v in run.last_vessel_centrelines.items()}
        s["postprocessing_settings"]["run_postprocessing"] = True
        out["cropped_postprocessed"] = run(target, settings=s, atlases=atlases, geometry_stages=True)
        out["default"] = run(target, settings=settings, atlases=atlases, geometry_stages=True)
        results, _, atlas_set = out["cropped"]
        kept = {k: v for k, v in atlas_set.items() if v.get("DIR")}
        out["vessels_by_hand"] = pa.utils.vessel.vessel_spline_generation(results["CROP_IMAGE"], kept, **settings["vessel_spline_settings"])
        fused = {k: v for k, v in results.items() if k in CHAMBERS}
        out["geometry_by_hand"] = pa.projects.multiatlas.geometric_definitions(fused, settings["geometric_segmentation_settings"])
    finally:
        patch.undo()
    _PIPELINE_RUNS[kind] = out
    return out


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def pipeline_runs(request):
    if request.param == "gpu":
        request.getfixturevalue("gpu_backend")
    return run_pipelines(request.param)


def test_pipeline_returns_the_ten_new_keys(pipeline_runs):
    results, prob = pipeline_runs["default"]
    target = pipeline_runs["target"]
    assert set(NEW_KEYS) <= set(results) and set(CHAMBERS) <= set(results)
    for k in NEW_KEYS:
        assert results[k].GetSize() == target.GetSize() and int((results[k].tensor != 0).sum()) > 0, k
    for v in VESSELS:      # every atlas's propagated vessel, one bit per kept atlas
        assert prob[v].GetSize() == target.GetSize() and len(__import__("platipy_amd").label.binary_decode_image(prob[v])) == 2


def test_pipeline_stages_equal_the_functions_applied_by_hand(pipeline_runs):
    results, prob, _ = pipeline_runs["cropped"]
    for v in VESSELS:
        assert np.array_equal(results[v].numpy(), pipeline_runs["vessels_by_hand"][v].numpy()), v
        assert results[v].numpy().sum() > 20
    for k, want in pipeline_runs["geometry_by_hand"].items():
        assert np.array_equal(results[k].numpy(), want.numpy()), k


def test_pipeline_step7_runs_before_postprocessing(pipeline_runs):
    plain, _, _ = pipeline_runs["cropped"]
    post, _ = pipeline_runs["cropped_postprocessed"]
    for k in NEW_KEYS[4:]:
        assert np.array_equal(post[k].numpy(), plain[k].numpy()), k
    assert any(not np.array_equal(post[k].numpy(), plain[k].numpy()) for k in CHAMBERS)      # post-processing did change its inputs


def test_pipeline_keeps_the_guard_without_the_keyword(pipeline_runs):
    import platipy_amd as pa

    with pytest.raises(NotImplementedError, match="vessel"):
        pa.projects.cardiac.run_cardiac_segmentation(pipeline_runs["target"], settings=pipeline_runs["settings"])


def _geometry_worker(rank, world, port, out_dir):
    import os

    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world)})
    import torch.distributed as dist

    import platipy_amd as pa
    from tests.helpers import install_emu_runtime

    install_emu_runtime()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        target, atlases, settings = pipeline_case(pa)
        ids = settings["atlas_settings"]["atlas_id_list"]
        mine = {k: v for k, v in atlases.items() if k in ids[rank::world]}
        run = pa.projects.cardiac.run_cardiac_segmentation
        results, _ = run(target, settings=settings, atlases=mine, geometry_stages=True)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **{f"line_{k}": v for k, v in run.last_vessel_centrelines.items()},
                 **{f"mask_{k}": results[k].numpy() for k in VESSELS})
        try:
            run(target, settings=settings, atlases=mine, geometry_stages=True, fusion_collective="reduce")
            refused = False
        except NotImplementedError:
            refused = True
        assert refused
    finally:
        dist.destroy_process_group()


@pytest.mark.slow
def test_pipeline_two_ranks_gloo_same_centreline_bits(tmp_path):
    """World size 2 over gloo on the CPU emulation: each rank computes the moments of its own atlas, the tables are
    gathered, and both ranks draw the centreline world size 1 draws -- bit for bit."""
    import os

    pipeline_runs = run_pipelines("emu")

    import torch.multiprocessing as mp

    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_geometry_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    for v in VESSELS:
        want = pipeline_runs["centrelines"][v]
        assert want.shape[0] > 20
        assert np.array_equal(r0[f"line_{v}"], want) and np.array_equal(r1[f"line_{v}"], want), v
        assert np.array_equal(r0[f"mask_{v}"], r1[f"mask_{v}"])
