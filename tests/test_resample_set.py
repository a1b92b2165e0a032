"""pp_resample_set (platipy_amd/csrc/pp_resample_set.h): an image and up to 16 label volumes through one transform in one
gather.  Its contract is equality, bit for bit, with pp_resample_f32 / pp_resample_u8 called for each member alone -- those
are held to the fp64 restatement in tests/test_resample_kernels.py -- so every comparison here is np.array_equal against
ctx.resample, on the shapes where a fused kernel can go wrong: an output grid that is no multiple of a block edge, input
and output grids that differ, the axis-aligned arm with and without its 3 x 3, the general (oblique) arm, single-column
and single-plane inputs, samples exactly on the buffer's ends and on nearest-neighbour ties, every label count that
changes the unrolled loop's trip count, and the banded launch."""
import ctypes as C

import numpy as np
import pytest

from platipy_amd import _lib
from tests import resample_restatement as R
from tests.helpers import border_probe_fields, random_dvf, rot_xyz

LIN, NEAR, BSP = _lib.INTERP_LINEAR, _lib.INTERP_NEAREST, _lib.INTERP_BSPLINE
DEFAULT = -777.25      # never a voxel value nor a lerp of voxel values: every image here stays within +-500
OUT_SHAPE = (11, 19, 37)        # 37 x 19 x 11: no multiple of 64 x 4 (nor of any other block shape)


def grid_of(shape, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None):
    return R.Grid(shape[::-1], spacing, origin, direction)


def geom_of(g):
    return _lib.make_geom(g.size, g.spacing, g.origin, g.direction.ravel())


def volumes(shape, nlabels, seed):
    """An image within +-500 and labels whose every voxel is >= 1: a 0 in an output can only be the default."""
    rng = np.random.default_rng(seed)
    img = np.clip(rng.normal(0.0, 200.0, shape), -500.0, 500.0).astype(np.float32)
    labs = [rng.integers(1, 256, shape).astype(np.uint8) for _ in range(nlabels)]
    return img, labs


def run_set(be, img, labs, gin, gout, interp=LIN, default=DEFAULT, A=None, t=None, field=None):
    io = None if img is None else be.empty(gout.shape)
    los = [be.empty(gout.shape, np.uint8) for _ in labs]
    be.ctx.resample_set(geom_of(gin), geom_of(gout), image=None if img is None else be.dev(img), image_out=io,
                        labels=[be.dev(lab) for lab in labs], labels_out=los, affine_A=None if A is None else np.asarray(A).ravel(),
                        affine_t=t, field=None if field is None else be.dev(field), interp=interp, default_value=default)
    return (None if img is None else be.host(io).copy()), [be.host(lo).copy() for lo in los]


def run_members(be, img, labs, gin, gout, interp=LIN, default=DEFAULT, A=None, t=None, field=None):
    def one(vol, interp_, default_):
        u8 = vol.dtype == np.uint8
        out = be.empty(gout.shape, np.uint8 if u8 else np.float32)
        be.ctx.resample(be.dev(vol), geom_of(gin), geom_of(gout), out, affine_A=None if A is None else np.asarray(A).ravel(), affine_t=t,
                        field=None if field is None else be.dev(field), interp=interp_, default_value=default_, u8=u8)
        return be.host(out).copy()

    return (None if img is None else one(img, interp, default)), [one(lab, NEAR, 0.0) for lab in labs]


def assert_same(got, want):
    assert (got[0] is None) == (want[0] is None) and len(got[1]) == len(want[1])
    if want[0] is not None:
        np.testing.assert_array_equal(got[0], want[0])
    for a, b in zip(got[1], want[1]):
        np.testing.assert_array_equal(a, b)


# --------------------------------------------------------------------------------------
# geometries: name -> (gin, gout, A, t, field or None)

IN_SHAPE = (9, 14, 23)
ROT = rot_xyz(20.0, -35.0, 50.0)
AFF = rot_xyz(4.0, -3.0, 6.0) @ np.array([[1.05, 0.02, 0.0], [0.0, 0.97, -0.015], [0.01, 0.0, 1.02]])


def geometry(name):
    direction = ROT if name.startswith("oblique") else None
    in_shape = {"nx1": (6, 7, 1), "nz1": (1, 7, 9)}.get(name, IN_SHAPE)
    gin = grid_of(in_shape, (0.9, 1.1, 2.5), (-31.7, 12.3, 105.1), direction)
    ctr = gin.index_to_physical((np.asarray(gin.size) - 1) / 2.0)
    # the output grid is centred on the input's and a little larger than it on every axis a volume has extent on
    ext_in = np.asarray(gin.size) * np.asarray(gin.spacing)
    # (a single column / plane: a twentieth of its spacing, so that the field decides which samples stay within it)
    sp = np.where(np.asarray(gin.size) > 1, 1.15 * ext_in / np.asarray(OUT_SHAPE[::-1]), 0.05 * np.asarray(gin.spacing))
    org = ctr - (ROT if direction is not None else np.eye(3)) @ (sp * (np.asarray(OUT_SHAPE[::-1]) - 1) / 2.0) + np.array([0.3719, -0.2137, 0.4541])
    gout = grid_of(OUT_SHAPE, sp, org, direction if name == "oblique_both" else None)
    A = t = None
    if "affine" in name:
        A, t = AFF, ctr - AFF @ ctr + np.array([0.6, -0.4, 0.3])
    field = None
    if not name.endswith("nofield"):
        # about +-3 input voxels on every axis: part of the output leaves the input
        f = random_dvf(OUT_SHAPE, sp, seed=len(name), max_mm=1.0)
        f = f / np.abs(f).max() * 3.0 * np.asarray(gin.spacing, np.float32)[:, None, None, None]
        field = np.ascontiguousarray(f, dtype=np.float32)
    return gin, gout, A, t, field


GEOMETRIES = ["aligned", "aligned_nofield", "affine", "affine_nofield", "oblique", "oblique_both", "oblique_nofield", "nx1", "nz1"]
MEMBERS = [(LIN, 0), (LIN, 1), (LIN, 3), (LIN, 16), (NEAR, 0), (NEAR, 3), (NEAR, 16), (None, 1), (None, 3), (None, 16)]


@pytest.mark.parametrize("members", MEMBERS, ids=lambda m: f"{ {LIN: 'lin', NEAR: 'near', None: 'noimg'}[m[0]] }-{m[1]}")
@pytest.mark.parametrize("name", GEOMETRIES)
def test_set_equals_members(backend, name, members):
    interp, nlabels = members
    gin, gout, A, t, field = geometry(name)
    img, labs = volumes(gin.shape, nlabels, 17 + nlabels)
    if interp is None:
        img = None
    kw = dict(interp=interp or LIN, A=A, t=t, field=field)
    got = run_set(backend, img, labs, gin, gout, **kw)
    want = run_members(backend, img, labs, gin, gout, **kw)
    assert_same(got, want)
    # the case is one: part of the output is outside the input, part inside; the image default is DEFAULT, the labels' 0
    outside = (got[0] == np.float32(DEFAULT)) if img is not None else (got[1][0] == 0)
    assert 0.02 < outside.mean() < 0.98, outside.mean()
    for lo in got[1]:
        np.testing.assert_array_equal(lo == 0, outside)


@pytest.mark.parametrize("name", ["aligned", "affine", "nx1"])
def test_both_arms_answer_alike(backend, monkeypatch, name):
    """The axis-aligned arm and the general arm (forced by PP_RESAMPLE_GENERIC) on the same axis-aligned case."""
    gin, gout, A, t, field = geometry(name)
    img, labs = volumes(gin.shape, 3, 5)
    fast = run_set(backend, img, labs, gin, gout, A=A, t=t, field=field)
    monkeypatch.setenv("PP_RESAMPLE_GENERIC", "1")
    assert_same(run_set(backend, img, labs, gin, gout, A=A, t=t, field=field), fast)
    assert_same(run_members(backend, img, labs, gin, gout, A=A, t=t, field=field), fast)


@pytest.mark.parametrize("interp", [LIN, NEAR], ids=["lin", "near"])
@pytest.mark.parametrize("shape", [(5, 6, 9), (6, 5, 1), (1, 9, 4)])
def test_exact_borders_and_ties(backend, shape, interp):
    """Unit spacing, origin 0, fields of exact multiples of 2^-7 (tests/helpers.py:border_probe_fields): samples exactly on
    -0.5 and n - 0.5 (the first inside, the second outside), on every nearest-neighbour tie k + 0.5 and 2^-6 either side."""
    g = grid_of(shape)
    img, labs = volumes(shape, 3, 23)
    for f in border_probe_fields(shape, (1.0, 1.0, 1.0), 300 + shape[2]):
        got = run_set(backend, img, labs, g, g, interp=interp, field=f)
        assert_same(got, run_members(backend, img, labs, g, g, interp=interp, field=f))
        c = R.continuous_index(g, g, field=f)
        inside = R.inside_buffer(c, g.size)          # by definition: [-0.5, n - 0.5) on every axis
        assert inside.any() and not inside.all()
        np.testing.assert_array_equal(got[0] != np.float32(DEFAULT), inside)
        q = np.floor(c + 0.5).astype(np.int64)       # ties round half up
        for lab, lo in zip(labs, got[1]):
            want = np.where(inside, lab[np.clip(q[..., 2], 0, shape[0] - 1), np.clip(q[..., 1], 0, shape[1] - 1), np.clip(q[..., 0], 0, shape[2] - 1)], 0)
            np.testing.assert_array_equal(lo, want)


def test_banded_launch(backend):
    """65 tiles of 64 x 4 per plane: the XCD-banded block order k_resample_axis uses for a linear image through a field."""
    shape = (2, 260, 12)
    g = grid_of(shape, (0.9, 1.1, 2.5), (4.0, -2.0, 1.5))
    img, labs = volumes(shape, 3, 61)
    f = (random_dvf(shape, g.spacing, seed=62, max_mm=4.0)).astype(np.float32)
    got = run_set(backend, img, labs, g, g, field=f)
    assert_same(got, run_members(backend, img, labs, g, g, field=f))
    assert 0.02 < (got[0] == np.float32(DEFAULT)).mean() < 0.9


def test_two_calls_return_identical_bits(backend):
    gin, gout, A, t, field = geometry("affine")
    img, labs = volumes(gin.shape, 16, 3)
    assert_same(run_set(backend, img, labs, gin, gout, A=A, t=t, field=field), run_set(backend, img, labs, gin, gout, A=A, t=t, field=field))


def test_bad_counts_and_interpolators_are_errors(backend):
    gin, gout, _, _, _ = geometry("aligned_nofield")
    img, labs = volumes(gin.shape, 17, 1)
    with pytest.raises(_lib.PlatipyAmdError) as e:
        run_set(backend, img, labs, gin, gout)
    assert e.value.code == _lib.ERR_ARG
    # a negative count, at the C entry itself: an error code, nothing launched, nothing read
    one_in, one_out = backend.dev(labs[0]), backend.empty(gout.shape, np.uint8)
    tin, tout = (C.c_void_p * 1)(_lib.ptr(one_in)), (C.c_void_p * 1)(_lib.ptr(one_out))
    rc = backend.lib.pp_resample_set(backend.ctx.h, C.byref(geom_of(gin)), C.byref(geom_of(gout)), None, None, None, None, LIN, 0.0, None,
                                     tin, -1, tout)
    assert rc == _lib.ERR_ARG
    assert not backend.host(one_out).any()
    with pytest.raises(_lib.PlatipyAmdError) as e:       # neither an image nor a label
        run_set(backend, None, [], gin, gout)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.PlatipyAmdError) as e:       # declined, for the Python layer to go member by member
        run_set(backend, img, labs[:2], gin, gout, interp=BSP)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.PlatipyAmdError):            # an output that is its input
        backend.ctx.resample_set(geom_of(gin), geom_of(gin), labels=[one_in], labels_out=[one_in])
    assert_same(run_set(backend, img, labs[:1], gin, gout), run_members(backend, img, labs[:1], gin, gout))     # the context still works
