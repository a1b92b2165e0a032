"""pp_project_set (platipy_amd/csrc/pp_project.h) and platipy_amd.visualisation: rotated projections of an image and its labels.

The kernel's contract is that of pp_resample_set: for every view, every sample along a ray is, bit for bit, the voxel
pp_resample_f32 / pp_resample_u8 write for that member, transform and output index with gout = gin -- those are held to their
fp64 restatement in tests/test_resample_kernels.py.  So every member is resampled alone with ctx.resample, reduced in numpy
with tests/projection_restatement.py (sequential fp64 sums, np.partition's element n // 2, np.min / np.max) and compared with
np.array_equal: min, max, median, sum and every label plane always; mean and std too, because the build's fp64 division and
square root are correctly rounded (DESIGN 4.15 says which case holds).

NaN: min, max, sum, mean and std return NaN when a sample is NaN; the median sorts every NaN last (numpy's rule) and is NaN only
when more than (n - 1) / 2 samples are (test_nan_and_infinities).

The median select has no staging chunk, so the ray lengths around a chunk are the issue's 63, 64, 65 and 129 (and 15, 16, 17,
33 around the walk's tile of 16 samples)."""
import ctypes as C

import numpy as np
import pytest

from platipy_amd import _lib
from platipy_amd.transform import VersorRigid3DTransform
from tests import projection_restatement as PR
from tests.helpers import EPS6, rot_xyz

LIN, NEAR, BSP = _lib.INTERP_LINEAR, _lib.INTERP_NEAREST, _lib.INTERP_BSPLINE
DEFAULT = -777.25      # never a voxel value nor a lerp of voxel values: every image here stays within +-500
KINDS = PR.KINDS
ROT = rot_xyz(20.0, -35.0, 50.0)
IDENTITY_VIEW = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])


class Grid:
    def __init__(self, shape, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None):
        self.shape = tuple(shape)
        self.size = tuple(shape[::-1])
        self.spacing, self.origin = tuple(spacing), tuple(origin)
        self.direction = np.eye(3) if direction is None else np.asarray(direction, dtype=np.float64)

    def geom(self):
        return _lib.make_geom(self.size, self.spacing, self.origin, self.direction.ravel())

    def centre(self):
        return np.asarray(self.origin) + self.direction @ (np.asarray(self.spacing) * (np.asarray(self.size) - 1) / 2.0)


def grid_named(name, shape):
    if name == "unit":
        return Grid(shape)
    return Grid(shape, (0.9, 1.1, 2.5), (-31.7, 12.3, 105.1), ROT if name == "oblique" else None)


def rotation_view(grid, axis, angle, shift=(0.0, 0.0, 0.0)):
    """12 doubles (A row-major, t) of the rotation about the grid's centre, as VersorRigid3DTransform gives it."""
    tfm = VersorRigid3DTransform()
    tfm.SetCenter(grid.centre())
    tfm.SetRotation(axis, angle)
    A, t = tfm.matrix_offset()
    return np.concatenate([A.ravel(), t + np.asarray(shift)])


def standard_views(grid):
    """0.3 and 2.9 about an oblique axis, pi / 2 about each axis: five distinct transforms"""
    return np.stack([rotation_view(grid, (1.0, 2.0, 3.0), 0.3), rotation_view(grid, (1.0, 2.0, 3.0), 2.9),
                     rotation_view(grid, (1, 0, 0), np.pi / 2), rotation_view(grid, (0, 1, 0), np.pi / 2),
                     rotation_view(grid, (0, 0, 1), np.pi / 2)])


def volumes(shape, nlabels, seed):
    """An image within +-500 and labels whose every voxel is >= 1: a 0 in a label plane can only come from defaults."""
    rng = np.random.default_rng(seed)
    img = np.clip(rng.normal(0.0, 200.0, shape), -500.0, 500.0).astype(np.float32)
    labs = [rng.integers(1, 256, shape).astype(np.uint8) for _ in range(nlabels)]
    return img, labs


def plane_shape(shape, axis):
    nz, ny, nx = shape
    return {0: (nz, ny), 1: (nz, nx), 2: (ny, nx)}[axis]


def label_interps(n, linterp):
    return [linterp] * n if np.isscalar(linterp) else list(linterp)


def run_fused(be, img, labs, grid, axis, views, kind="max", interp=LIN, linterp=NEAR, default=DEFAULT):
    """-> (fp32 [V, rows, cols] or None, [uint8 [V, rows, cols], ...]) of ONE pp_project_set call"""
    views = np.atleast_2d(views)
    shape = (len(views),) + plane_shape(grid.shape, axis)
    io = None if img is None else be.empty(shape)
    los = [be.empty(shape, np.uint8) for _ in labs]
    be.ctx.project_set(grid.geom(), axis, views, image=None if img is None else be.dev(img), image_out=io,
                       kind=_lib.PROJECT_KINDS[kind], interp=interp, default_value=default, labels=[be.dev(lab) for lab in labs],
                       labels_out=los, label_interp=label_interps(len(labs), linterp))
    return (None if img is None else be.host(io).copy()), [be.host(lo).copy() for lo in los]


def resample_members(be, img, labs, grid, views, interp=LIN, linterp=NEAR, default=DEFAULT):
    """Every member through every view alone: -> ([volume per view] or None, [[volume per view] per label])"""
    g = grid.geom()

    def one(vol, v, interp_, default_):
        u8 = vol.dtype == np.uint8
        out = be.empty(grid.shape, np.uint8 if u8 else np.float32)
        be.ctx.resample(be.dev(vol), g, g, out, affine_A=v[:9], affine_t=v[9:], interp=interp_, default_value=default_, u8=u8)
        return be.host(out).copy()

    views = np.atleast_2d(views)
    li = label_interps(len(labs), linterp)
    return (None if img is None else [one(img, v, interp, default) for v in views]), [[one(lab, v, i, 0.0) for v in views] for lab, i in zip(labs, li)]


def assert_plane(got, volume, kind, axis, what=""):
    """One fp32 plane against the restated reduction of the member's resampled volume, bit for bit (NaN equal to NaN)."""
    want = PR.reduce(volume, kind, axis)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want, equal_nan=True):
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).ravel())
        raise AssertionError(f"{what} {kind} axis {axis}: {bad.size} of {got.size} pixels differ, first {bad[:4].tolist()}: "
                             f"{got.ravel()[bad[:4]]} instead of {want.ravel()[bad[:4]]}")


def assert_fused_equals_members(be, img, labs, grid, axis, views, kinds=KINDS, interp=LIN, linterp=NEAR, default=DEFAULT, what=""):
    """All `kinds` of the fused call against the members, which are resampled once.  -> the members' volumes"""
    vi, vl = resample_members(be, img, labs, grid, views, interp, linterp, default)
    for kind in (kinds if img is not None else ("max",)):
        gi, gl = run_fused(be, img, labs, grid, axis, views, kind, interp, linterp, default)
        assert (gi is None) == (img is None) and len(gl) == len(labs)
        for v in range(len(np.atleast_2d(views))):
            if img is not None:
                assert_plane(gi[v], vi[v], kind, axis, f"{what} view {v}")
            for k in range(len(labs)):
                np.testing.assert_array_equal(gl[k][v], PR.label_max(vl[k][v], axis), err_msg=f"{what} view {v} label {k}")
    return vi, vl


# --------------------------------------------------------------------------------------
# the kernel against its members


@pytest.mark.parametrize("interp", [LIN, NEAR], ids=["lin", "near"])
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("gname", ["aligned", "oblique"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (9, 17, 33)], ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_members(backend, shape, gname, axis, interp):
    """Six kinds, five views in one call, three labels (nearest, linear, nearest) on an anisotropic grid, axis-aligned and
    with oblique direction cosines."""
    grid = grid_named(gname, shape)
    img, labs = volumes(shape, 3, 11 + shape[2])
    vi, vl = assert_fused_equals_members(backend, img, labs, grid, axis, standard_views(grid), interp=interp, linterp=[NEAR, LIN, NEAR],
                                         what=f"{shape} {gname}")
    outside = np.stack(vi) == np.float32(DEFAULT)
    assert 0.02 < outside.mean() < 0.98, outside.mean()      # the case is one: rays leave the volume and come back


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_views_equal_their_single_view_calls(backend, axis):
    shape = (9, 17, 33)
    grid = grid_named("oblique", shape)
    img, labs = volumes(shape, 2, 5)
    views = standard_views(grid)
    for kind in ("median", "std"):
        gi, gl = run_fused(backend, img, labs, grid, axis, views, kind)
        for v, view in enumerate(views):
            si, sl = run_fused(backend, img, labs, grid, axis, view, kind)
            np.testing.assert_array_equal(gi[v], si[0])
            for a, b in zip(gl, sl):
                np.testing.assert_array_equal(a[v], b[0])
        assert not np.array_equal(gi[0], gi[1])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_angle_zero_is_the_plain_axis_reduction(backend, axis):
    """A rotation by 0 about the centre of a unit grid maps every index onto itself: the fused result is the reduction of the
    input along the axis."""
    shape = (9, 17, 33)
    grid = grid_named("unit", shape)
    img, labs = volumes(shape, 2, 3)
    view = rotation_view(grid, (1, 0, 0), 0.0)
    np.testing.assert_array_equal(view, IDENTITY_VIEW)
    for interp in (LIN, NEAR):
        for kind in KINDS:
            gi, gl = run_fused(backend, img, labs, grid, axis, view, kind, interp, [NEAR, LIN])
            assert_plane(gi[0], img, kind, axis, "angle 0")
            for lab, g in zip(labs, gl):
                np.testing.assert_array_equal(g[0], PR.label_max(lab, axis))


RAY_LENGTHS = [1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 129]


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("n", RAY_LENGTHS)
def test_ray_lengths(backend, n, axis):
    """Rays of 1 (std is 0 / 0), 2 and 3 samples -- the median of even and odd counts, n / 2 against (n - 1) / 2 -- and the
    lengths around 16 (the walk's tile), 2 * 16 + 1, 64 and 2 * 64 + 1; the other two sizes are 4 and 5."""
    size = [4, 5]
    size.insert(axis, n)
    shape = tuple(size[::-1])
    grid = grid_named("aligned", shape)
    img, labs = volumes(shape, 1, 100 + n)
    views = np.stack([rotation_view(grid, (0, 0, 1), 0.0), rotation_view(grid, (1.0, 2.0, 3.0), 0.05)])
    vi, _ = assert_fused_equals_members(backend, img, labs, grid, axis, views, interp=LIN, what=f"n = {n}")
    if n == 1:
        gi, _ = run_fused(backend, img, labs, grid, axis, views, "std")
        assert np.isnan(gi).all()
    if n == 2:      # the upper median of two samples is their maximum
        gi, _ = run_fused(backend, img, labs, grid, axis, views[0], "median")
        np.testing.assert_array_equal(gi[0], np.max(vi[0], axis=PR.np_axis(axis)))


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", [(6, 7, 1), (6, 1, 9)], ids=["nx1", "ny1"])
def test_single_column_and_single_row_inputs(backend, shape, axis):
    grid = grid_named("aligned", shape)
    img, labs = volumes(shape, 2, 40)
    # (small turns and a shift: a single column leaves its own grid at any larger angle)
    views = np.stack([rotation_view(grid, (0, 0, 1), 0.0), rotation_view(grid, (1.0, 2.0, 3.0), 0.02, (0.2, -0.3, 0.4)),
                      rotation_view(grid, (1, 0, 0), 0.3) if shape[2] == 1 else rotation_view(grid, (0, 1, 0), 0.3)])
    vi, _ = assert_fused_equals_members(backend, img, labs, grid, axis, views, linterp=[LIN, NEAR], what=str(shape))
    assert 0.0 < (np.stack(vi) != np.float32(DEFAULT)).mean()


def test_whole_rays_outside_reduce_the_default(backend):
    """A slab of 3 x 21 x 21 turned by pi / 2 about x: projected along x, the pixels whose y lies beyond the turned slab see n
    defaults, and the default takes part in every reduction."""
    shape, axis = (3, 21, 21), 0
    grid = grid_named("unit", shape)
    img, labs = volumes(shape, 1, 8)
    view = rotation_view(grid, (1, 0, 0), np.pi / 2)
    vi, _ = assert_fused_equals_members(backend, img, labs, grid, axis, view, what="slab")
    empty = (vi[0] == np.float32(DEFAULT)).all(axis=2)          # [nz][ny]: every sample of the ray is the default
    assert 0.5 < empty.mean() < 1.0
    n = shape[2]
    for kind in KINDS:
        gi, gl = run_fused(backend, img, labs, grid, axis, view, kind)
        want = PR.reduce(np.full((1, 1, n), DEFAULT, np.float32), kind, axis)[0, 0]
        assert (gi[0][empty] == want).all(), kind
        assert want == {"sum": np.float32(n * DEFAULT), "std": 0.0}.get(kind, np.float32(DEFAULT))
        assert not gl[0][0][empty].any() and gl[0][0][~empty].all()


@pytest.mark.parametrize("interp", [LIN, NEAR], ids=["lin", "near"])
@pytest.mark.parametrize("shape", [(5, 6, 9), (6, 5, 1), (1, 9, 4)], ids=lambda s: "x".join(map(str, s)))
def test_exact_borders_and_ties(backend, shape, interp):
    """Unit spacing, origin 0, translations by exact multiples of 2^-6 (tests/helpers.py: EPS6, the offsets of
    border_targets): the samples of a view lie exactly on -0.5 and n - 0.5 (the first inside, the second outside), on every
    nearest-neighbour tie k + 0.5 and 2^-6 either side of them."""
    grid = grid_named("unit", shape)
    img, labs = volumes(shape, 2, 23)
    offsets = [-0.5 - EPS6, -0.5, -0.5 + EPS6, -EPS6, 0.5 - EPS6, 0.5, 0.5 + EPS6]
    shifts = [np.eye(3)[a] * o for a in range(3) for o in offsets] + [np.full(3, o) for o in offsets]
    views = np.stack([np.concatenate([np.eye(3).ravel(), s]) for s in shifts])
    z, y, x = np.indices(shape)
    for axis in range(3):
        assert_fused_equals_members(backend, img, labs, grid, axis, views, kinds=("sum", "median", "min"), interp=interp,
                                    linterp=[NEAR, LIN], what="ties")
        # ... and, for nearest neighbour, against the definition: inside is [-0.5, n - 0.5), ties round half up
        gi, gl = run_fused(backend, img, labs, grid, axis, views, "sum", NEAR, NEAR)
        some_inside = some_outside = False
        for v, s in enumerate(shifts):
            c = [x + s[0], y + s[1], z + s[2]]
            inside = np.ones(shape, bool)
            for a in range(3):
                inside &= (c[a] >= -0.5) & (c[a] < grid.size[a] - 0.5)
            q = [np.clip(np.floor(c[a] + 0.5).astype(np.int64), 0, grid.size[a] - 1) for a in range(3)]
            assert_plane(gi[v], np.where(inside, img[q[2], q[1], q[0]], np.float32(DEFAULT)), "sum", axis, f"shift {s}")
            np.testing.assert_array_equal(gl[0][v], PR.label_max(np.where(inside, labs[0][q[2], q[1], q[0]], 0), axis))
            some_inside, some_outside = some_inside or inside.any(), some_outside or not inside.all()
        assert some_inside and some_outside


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("members", [(True, 0), (True, 1), (True, 2), (True, 4), (True, 5), (True, 8), (True, 9), (True, 15), (True, 16), (False, 1),
                                     (False, 2), (False, 5), (False, 15), (False, 16)],
                         ids=lambda m: f"{'img' if m[0] else 'noimg'}-{m[1]}")
def test_label_counts_and_absent_image(backend, members, axis):
    """Label counts on either side of the kernel's label capacities (0, 4, 8, 16) -- 0, 1, 2, 15, 16 as the issue lists them, and
    4, 5, 8, 9 -- with and without the image, on the axis-0 patch shape and the other."""
    with_image, nlabels = members
    shape = (5, 9, 35)
    grid = grid_named("oblique", shape)
    img, labs = volumes(shape, nlabels, 17 + nlabels)
    views = standard_views(grid)[:2]
    assert_fused_equals_members(backend, img if with_image else None, labs, grid, axis, views, kinds=("mean", "max"),
                                linterp=[NEAR if k % 3 else LIN for k in range(nlabels)], what=f"{members}")


def test_median_of_equal_samples_and_duplicates(backend):
    """Identity view of a unit grid, nearest neighbour: the samples are the voxels.  Rays along x with all-equal samples, with
    duplicates around the middle, and the even count whose (n - 1) / 2 and n / 2 elements differ."""
    rays5 = [[7, 7, 7, 7, 7], [1, 2, 2, 2, 3], [3, 2, 2, 2, 1], [2, 9, 2, 9, 2], [9, 2, 9, 2, 9], [-1, -1, 0, 0, 5], [5, 4, 3, 2, 1],
             [-0.0, 0.0, -0.0, 0.0, 1]]
    want5 = [7, 2, 2, 2, 9, 0, 3, 0]
    rays4 = [[4, 4, 4, 4], [1, 2, 3, 4], [4, 3, 2, 1], [1, 2, 2, 3], [2, 2, 3, 3], [3, 3, 2, 2], [-5, -6, -7, -8], [1, 1, 1, 2]]
    want4 = [4, 3, 3, 2, 3, 3, -6, 1]
    for rays, want in ((rays5, want5), (rays4, want4)):
        vol = np.asarray(rays, np.float32).reshape(2, 4, len(rays[0]))
        gi, _ = run_fused(backend, vol, [], grid_named("unit", vol.shape), 0, IDENTITY_VIEW, "median", NEAR)
        np.testing.assert_array_equal(gi[0].ravel(), np.asarray(want, np.float32))
        assert_plane(gi[0], vol, "median", 0)
        for axis in (1, 2):     # the same rays along y and z
            t = np.ascontiguousarray(np.moveaxis(vol, 2, PR.np_axis(axis)))
            gi, _ = run_fused(backend, t, [], grid_named("unit", t.shape), axis, IDENTITY_VIEW, "median", NEAR)
            assert_plane(gi[0], t, "median", axis)
            np.testing.assert_array_equal(np.sort(gi[0].ravel()), np.sort(np.asarray(want, np.float32)))


def test_nan_and_infinities(backend):
    """min, max, sum, mean, std: NaN when a sample is NaN.  median: NaN sorts last whatever its sign, so one NaN among five
    samples leaves a finite median and three make it NaN.  Infinities are ordinary ordered values for min, max and median."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    neg_nan = np.frombuffer(np.uint32(0xffc00001).tobytes(), np.float32)[0]
    rays = np.array([[1, nan, 3, 2, 5], [neg_nan, 4, 1, 9, 2], [nan, 1, neg_nan, 2, nan], [nan, nan, nan, nan, nan], [inf, 1, -inf, 2, 3],
                     [inf, inf, inf, 1, 2], [-inf, -inf, -inf, 1, 2], [1, 2, 3, 4, 5]], np.float32)
    vol = rays.reshape(2, 4, 5)
    grid = grid_named("unit", vol.shape)
    got = {kind: run_fused(backend, vol, [], grid, 0, IDENTITY_VIEW, kind, NEAR)[0][0] for kind in KINDS}
    for kind in KINDS:
        assert_plane(got[kind], vol, kind, 0, "nan")
    has_nan = np.isnan(rays).any(axis=1)
    for kind in ("min", "max", "sum", "mean", "std"):
        assert np.isnan(got[kind].ravel()[has_nan[:4].nonzero()[0]]).all(), kind
    np.testing.assert_array_equal(got["median"].ravel(), np.array([3, 4, nan, nan, 2, inf, -inf, 3], np.float32))
    np.testing.assert_array_equal(got["min"].ravel()[4:], np.array([-inf, 1, -inf, 1], np.float32))
    np.testing.assert_array_equal(got["max"].ravel()[4:], np.array([inf, inf, 2, 5], np.float32))
    # through the linear interpolator and a rotation the fused samples are still the members'
    assert_fused_equals_members(backend, vol, [], grid, 1, standard_views(grid)[:1], what="nan, rotated")


def test_two_runs_return_identical_bits(backend):
    shape = (9, 17, 33)
    grid = grid_named("oblique", shape)
    img, labs = volumes(shape, 16, 3)
    for axis, kind in ((0, "std"), (1, "median"), (2, "mean")):
        a = run_fused(backend, img, labs, grid, axis, standard_views(grid), kind, linterp=LIN)
        b = run_fused(backend, img, labs, grid, axis, standard_views(grid), kind, linterp=LIN)
        assert a[0].tobytes() == b[0].tobytes()
        for x, y in zip(a[1], b[1]):
            assert x.tobytes() == y.tobytes()


def test_bad_arguments_are_errors_and_touch_nothing(backend):
    shape, axis = (4, 5, 6), 1
    grid = grid_named("aligned", shape)
    img, labs = volumes(shape, 17, 1)
    g = grid.geom()
    pshape = (1,) + plane_shape(shape, axis)
    d_img, d_labs = backend.dev(img), [backend.dev(lab) for lab in labs]
    io = backend.garbage(pshape, np.float32, 7.5)
    los = [backend.garbage(pshape, np.uint8, 0x5A) for _ in labs]
    views = (C.c_double * 12)(*IDENTITY_VIEW)
    table = lambda bufs: (C.c_void_p * max(len(bufs), 1))(*[_lib.ptr(b) for b in bufs])     # noqa: E731
    ints = lambda vals: (C.c_int * max(len(vals), 1))(*vals)     # noqa: E731

    def call(axis=axis, views=views, nviews=1, image=d_img, kind=_lib.PROJECT_MAX, interp=LIN, image_out=io, labels=d_labs[:2],
             linterp=(NEAR, NEAR), nlabels=None, labels_out=None):
        labels_out = los[:len(labels)] if labels_out is None else labels_out
        return backend.lib.pp_project_set(backend.ctx.h, C.byref(g), axis, views, nviews, _lib.ptr(image), kind, interp, DEFAULT,
                                          _lib.ptr(image_out), table(labels), ints(list(linterp)), len(labels) if nlabels is None else nlabels,
                                          table(labels_out))

    arg = [dict(axis=-1), dict(axis=3), dict(kind=-1), dict(kind=6), dict(interp=0), dict(interp=4), dict(linterp=(NEAR, 7)),
           dict(labels=d_labs, linterp=[NEAR] * 17), dict(nlabels=-1), dict(image=None, image_out=None, labels=[], linterp=[]),
           dict(nviews=0), dict(nviews=-3), dict(views=None), dict(image_out=None), dict(image_out=d_img),
           dict(labels_out=[d_labs[0], los[1]]), dict(labels_out=[d_labs[1], los[1]]), dict(labels_out=[los[0], los[0]]),
           dict(labels_out=[los[0], d_img])]
    for kw in arg:
        assert call(**kw) == _lib.ERR_ARG, kw
    for kw in (dict(interp=BSP), dict(linterp=(NEAR, BSP)), dict(image=None, image_out=None, linterp=(BSP, NEAR))):
        assert call(**kw) == _lib.ERR_UNSUPPORTED, kw
    assert (backend.host(io) == np.float32(7.5)).all()
    for lo in los:
        assert (backend.host(lo) == 0x5A).all()
    np.testing.assert_array_equal(backend.host(d_img), img)
    # the wrapper raises with the code, and the context still works
    with pytest.raises(_lib.PlatipyAmdError) as e:
        run_fused(backend, img, labs, grid, axis, IDENTITY_VIEW)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.PlatipyAmdError) as e:
        run_fused(backend, img, labs[:1], grid, axis, IDENTITY_VIEW, interp=BSP)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    assert call() == 0
    assert_fused_equals_members(backend, img, labs[:2], grid, axis, IDENTITY_VIEW, kinds=("max",))


# --------------------------------------------------------------------------------------
# the Python layer


def _image(pa, arr, grid):
    return pa.Image(np.ascontiguousarray(arr), grid.spacing, grid.origin, tuple(grid.direction.ravel()))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_project_onto_arbitrary_plane_is_rotate_then_reduce(host_api, axis):
    pa = host_api
    from platipy_amd.utils.geometry import rotate_image

    shape = (9, 17, 33)
    grid = grid_named("oblique", shape)
    img, _ = volumes(shape, 0, 77)
    image = _image(pa, img, grid)
    rotated = rotate_image(image, grid.centre(), (1.0, 2.0, 3.0), 0.3, pa.sitkLinear, DEFAULT).numpy()
    assert 0.02 < (rotated == np.float32(DEFAULT)).mean() < 0.98
    for kind in KINDS:
        got = pa.visualisation.project_onto_arbitrary_plane(image, kind, axis, [1.0, 2.0, 3.0], 0.3, DEFAULT, pa.sitkLinear)
        size, spacing, origin = PR.one_slice_geometry(grid.size, grid.spacing, grid.origin, grid.direction, axis)
        assert got.GetSize() == size and got.tensor.dtype == image.tensor.dtype
        np.testing.assert_allclose(got.GetSpacing(), spacing, rtol=1e-15)
        np.testing.assert_allclose(got.GetOrigin(), origin, rtol=1e-15)
        assert got.GetDirection() == image.GetDirection()
        assert_plane(got.numpy().squeeze(PR.np_axis(axis)), rotated, kind, axis, "python layer")
    # the defaults are the reference's: mean, axis 0, about x, angle 0, -1000, linear (a unit grid: angle 0 samples the voxels)
    plain = pa.visualisation.project_onto_arbitrary_plane(_image(pa, img, grid_named("unit", shape)))
    np.testing.assert_array_equal(plain.numpy().squeeze(2), PR.reduce(img, "mean", 0))


def test_projection_names_dtypes_and_uint8(host_api):
    pa = host_api
    from platipy_amd.utils.geometry import rotate_image

    shape = (9, 17, 33)
    grid = grid_named("aligned", shape)
    img, labs = volumes(shape, 1, 78)
    image = _image(pa, img, grid)
    with pytest.raises(KeyError):
        pa.visualisation.project_onto_arbitrary_plane(image, "mode")
    with pytest.raises(KeyError):
        pa.visualisation.project_set(image, [], [0.1], "average")
    # an int16-valued image goes through fp32 and comes back as int16: the fp32 result, truncated (P3)
    i16 = _image(pa, np.round(img).astype(np.int16), grid)
    for kind in ("mean", "max", "std"):
        got = pa.visualisation.project_onto_arbitrary_plane(i16, kind, 1, [0, 0, 1], 0.4, -1000)
        ref = pa.visualisation.project_onto_arbitrary_plane(_image(pa, np.round(img).astype(np.float32), grid), kind, 1, [0, 0, 1], 0.4, -1000)
        assert got.tensor.dtype == i16.tensor.dtype and got.GetSize() == ref.GetSize()
        np.testing.assert_array_equal(got.numpy(), np.trunc(ref.numpy()).astype(np.int16))
    # a uint8 image: "max" through the label path, the other kinds through rotate_image and the reduction (P4)
    u8 = _image(pa, labs[0], grid)
    for interp in (pa.sitkNearestNeighbor, pa.sitkLinear):
        rotated = rotate_image(u8, grid.centre(), (0, 0, 1), 0.4, interp, 0).numpy()
        for kind in ("max", "mean", "median"):
            got = pa.visualisation.project_onto_arbitrary_plane(u8, kind, 2, [0, 0, 1], 0.4, -1000, interp)
            assert got.numpy().dtype == np.uint8
            np.testing.assert_array_equal(got.numpy()[0], np.trunc(PR.reduce(rotated.astype(np.float32), kind, 2)).astype(np.uint8))


def test_project_set_equals_member_calls(host_api):
    """17 labels (two groups of the kernel's 16) and, in a second call, a label on another grid (the member-by-member path):
    every plane equals its own project_onto_arbitrary_plane call, bit for bit."""
    pa = host_api
    V = pa.visualisation
    shape = (9, 17, 33)
    grid = grid_named("aligned", shape)
    img, labs = volumes(shape, 17, 79)
    image, labels = _image(pa, img, grid), [_image(pa, lab, grid) for lab in labs]
    angles, rax = [0.0, 0.3, 2.9], (1.0, 2.0, 3.0)
    other = Grid((7, 11, 13), (1.3, 0.8, 2.0), (-20.0, 10.0, 100.0))
    stray = _image(pa, volumes(other.shape, 1, 80)[1][0], other)
    for kind, labels_ in (("median", labels), ("mean", labels[:2] + [stray])):
        for near in (True, False):
            li = pa.sitkNearestNeighbor if near else pa.sitkLinear
            gi, gl = V.project_set(image, labels_, angles, kind, 1, rax, DEFAULT, pa.sitkLinear, li)
            assert tuple(gi.shape) == (3, 9, 33) and len(gl) == len(labels_)
            for a, angle in enumerate(angles):
                one = V.project_onto_arbitrary_plane(image, kind, 1, rax, angle, DEFAULT, pa.sitkLinear)
                np.testing.assert_array_equal(gi[a].cpu().numpy(), one.numpy()[:, 0, :])
                for lab, g in zip(labels_, gl):
                    one = V.project_onto_arbitrary_plane(lab, "max", 1, rax, angle, 0, li)
                    assert g.dtype == one.tensor.dtype
                    np.testing.assert_array_equal(g[a].cpu().numpy(), one.numpy()[:, 0, :])
    # labels only, image only, nothing
    gi, gl = V.project_set(None, labels[:2], angles, label_interpolation=pa.sitkNearestNeighbor)
    assert gi is None and len(gl) == 2 and gl[0].any()
    gi, gl = V.project_set(image, [], angles)
    assert gl == [] and tuple(gi.shape) == (3, 9, 17)
    assert V.project_set(None, [], angles) == (None, [])
    gi, gl = V.project_set(image, labels[:2], [], projection_axis=2)        # no angle: empty stacks, one per member
    assert tuple(gi.shape) == (0, 17, 33) and gi.dtype == image.tensor.dtype and [tuple(g.shape) for g in gl] == [(0, 17, 33)] * 2


def test_linear_interpolation_erases_a_small_rotated_mask(host_api):
    """P6, the reference's default: linear interpolation of a 0 / 1 mask, truncated to uint8, keeps a sample only where all the
    corners it weighs are foreground -- the mask loses a voxel on every side.  A 2 x 2 x 2 cube turned by 0.5 rad is (nearly)
    gone from its projection; nearest neighbour keeps it."""
    pa = host_api
    shape = (12, 12, 12)
    cube = np.zeros(shape, np.uint8)
    cube[5:7, 5:7, 5:7] = 1
    mask = _image(pa, cube, Grid(shape))
    _, (lin,) = pa.visualisation.project_set(None, [mask], [0.5], rotation_axis=(1.0, 2.0, 3.0))
    _, (near,) = pa.visualisation.project_set(None, [mask], [0.5], rotation_axis=(1.0, 2.0, 3.0), label_interpolation=pa.sitkNearestNeighbor)
    lin, near = lin.cpu().numpy()[0], near.cpu().numpy()[0]
    assert near.sum() >= 4 and lin.sum() <= 1, (lin.sum(), near.sum())
    assert not (lin & ~near).any()


def test_comparison_colormix(host_api):
    import colorsys

    import torch

    pa = host_api
    rng = np.random.default_rng(5)
    a = rng.uniform(-400.0, 400.0, (5, 7))
    b = rng.uniform(-400.0, 400.0, (5, 7))
    b[1, :] = a[1, :]                       # a == b
    a[2, :3], b[2, :3] = 900.0, -900.0      # outside the window, a > b
    a[3, :3], b[3, :3] = -600.0, 700.0      # outside the window, a < b
    a[4, 0], b[4, 0] = 300.0, 800.0         # both clip to the window's top: equal after clipping
    assert (a > b).any() and (a == b).any() and (a < b).any()
    window, rot = (-250, 500), 0.35
    want = np.zeros((5, 7, 3))
    for i in range(5):
        for j in range(7):
            na, nb = [(min(max(v, window[0]), window[0] + window[1]) - window[0]) / window[1] for v in (a[i, j], b[i, j])]
            want[i, j] = colorsys.hsv_to_rgb(rot if na > nb else 0.5 + rot, abs(na - nb), (na + nb) / 2)
    V = pa.visualisation
    got = V.generate_comparison_colormix([torch.from_numpy(a), torch.from_numpy(b)])
    assert tuple(got.shape) == (1, 5, 7, 3)          # P7: arr_slice=None indexes with None
    assert np.abs(got[0].cpu().numpy() - want).max() <= 1e-6
    got = V.generate_comparison_colormix([torch.from_numpy(a), torch.from_numpy(b)], (slice(None), slice(None)))
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-6
    vols = [pa.Image(np.ascontiguousarray(np.stack([x, x + 1.0]).astype(np.float32))) for x in (a, b)]
    got = V.generate_comparison_colormix(vols, (0, slice(None), slice(None)))
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-6
    with pytest.raises(ValueError):
        V.generate_comparison_colormix(vols)                              # 3-D without arr_slice
    with pytest.raises(ValueError):
        V.generate_comparison_colormix([torch.zeros(2, 3, 4), torch.zeros(2, 3, 4)])
    with pytest.raises(ValueError):
        V.generate_comparison_colormix([torch.zeros(3, 4)] * 3)           # not two
    with pytest.raises(ValueError):
        V.generate_comparison_colormix([torch.zeros(3, 4)])
