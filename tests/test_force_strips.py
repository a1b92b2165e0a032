"""Kernel A's strip fetch (pp_demons_fused2.h, STRIPS): the MASK instances of k_fused2_force_smooth up to radius 2 bring the
(warped, fixed) image pair on chip as 16-byte strips over the whole image tile, double-buffered in LDS, instead of 4-byte
loads per owned voxel plus a border ring.  Only the way the bytes arrive changed, so the displacement field must equal,
bit for bit, what the untouched restatements of the same iteration compute:

  * generation 1 of the fused kernels (PP_FUSED_GEN=1) -- held bit-equal to generation 2 by
    test_kernels.py::test_fused_demons_generations_agree and ::test_fused_kernels_on_interior_tiles;
  * generation 2's branchy instances (PP_FUSED_MASK=0), which keep the per-voxel fetch -- held bit-equal to the MASK instances
    by test_kernels.py::test_fused_demons_padded_rows_do_not_change_the_field and ::test_fused_demons_pair_mix_visits_every_tile_once;
    they group the statistics like the MASK instances do, so the metric / RMS history is compared exactly;
  * the staged schedule (DEMONS_STAGED).  No existing test holds it BIT-equal to the fused kernels (tests/test_fullsize.py
    compares the two to 1e-3 mm), but on these inputs it is: the assertion is the bit comparison.

Shapes: the smallest at which a strip fetch can go wrong (tile remainders in x and y, rows shorter than a tile, fewer planes
than the z window, the 32 x 32 remainder column, padded rows), and one radius-3 case, which keeps the per-voxel fetch.
The moving image is the fixed one moved two voxels towards the high faces, so the warp leaves it there from the second
iteration on: sentinel values (FLT_MAX) then sit in the tile's halo, its border ring and the out-of-volume strips.
"""
import numpy as np
import pytest

from platipy_amd import _lib
from tests.helpers import phantom

# (nz, ny, nx), switches on top of PP_FUSED_MASK=1, sigma_u (voxels)
CASES = {
    "tile+remainder 70x38x12": ((12, 38, 70), {"PP_FUSED_TILE": "0", "PP_FUSED_PITCH": "1"}, 1.0),
    "nx%4==0, not 64k 100x20x9": ((9, 20, 100), {"PP_FUSED_TILE": "0"}, 1.0),
    "below one tile 36x18x7": ((7, 18, 36), {"PP_FUSED_TILE": "0"}, 1.0),
    "32x32 tiles 36x18x7": ((7, 18, 36), {"PP_FUSED_TILE": "1"}, 1.0),
    "nz < 2R+2 72x22x4": ((4, 22, 72), {"PP_FUSED_TILE": "0"}, 1.0),
    "mixed shapes 96x40x10": ((10, 40, 96), {"PP_FUSED_MIX": "1"}, 1.0),
    "odd nx, padded rows 67x21x9": ((9, 21, 67), {"PP_FUSED_TILE": "0", "PP_FUSED_PITCH": "1"}, 1.0),
    "radius 1 44x20x6": ((6, 20, 44), {"PP_FUSED_TILE": "0"}, 0.5),
    "radius 3 keeps the old fetch 72x20x9": ((9, 20, 72), {"PP_FUSED_TILE": "0"}, 1.7),
}
ITERS = 4
SWITCHES = ("PP_FUSED_MASK", "PP_FUSED_GEN", "PP_FUSED_TILE", "PP_FUSED_MIX", "PP_FUSED_PITCH")


def _pair(shape):
    fix = phantom(shape, seed=70)
    mov = np.pad(phantom(shape, seed=70, noise=0), ((2, 0), (2, 0), (2, 0)), mode="edge")[: shape[0], : shape[1], : shape[2]]
    mov = (mov + np.random.default_rng(71).normal(0, 3, size=shape)).astype(np.float32)
    return fix, np.ascontiguousarray(mov)


def _run(backend, monkeypatch, fix, mov, shape, sigma_u, variant, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    p = backend.ctx.default_demons_params()
    p.iterations, p.smooth_update, p.smooth_displacement, p.max_rms_error, p.variant = ITERS, 1, 1, 0.0, variant
    p.sigma_d_vox[:] = [1.5, 1.5, 1.5]
    p.sigma_u_vox[:] = [sigma_u] * 3
    g = _lib.make_geom((shape[2], shape[1], shape[0]), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    backend.ctx.profile_enable(True)
    try:
        backend.ctx.profile_read()
        f = backend.empty((3,) + shape)
        st = backend.ctx.demons_execute(backend.dev(fix), backend.dev(mov), g, p, f)
        field = backend.host(f).copy()
        names = {k for k, v in backend.ctx.profile_read().items() if v[0] > 0}
    finally:
        backend.ctx.profile_enable(False)
    return field, backend.ctx.demons_history(), (st.n_pixels, st.elapsed_iterations), names


@pytest.mark.parametrize("case", list(CASES))
def test_strip_fetch_leaves_the_field_bit_identical(backend, case, monkeypatch):
    shape, env, sigma_u = CASES[case]
    fix, mov = _pair(shape)
    strips = _run(backend, monkeypatch, fix, mov, shape, sigma_u, _lib.DEMONS_FUSED, dict(env, PP_FUSED_MASK="1"))
    assert "k_fused2_force_smooth" in strips[3] and "k_fused2_add_smooth_warp" in strips[3], strips[3]
    assert strips[2][1] == ITERS and len(strips[1]) == ITERS
    # the warp left the moving image: sentinel voxels were live in the later iterations (they are not counted)
    assert strips[2][0] < fix.size, "no sentinel voxel reached kernel A"
    assert np.abs(strips[0]).max() > 0.1

    branchy = _run(backend, monkeypatch, fix, mov, shape, sigma_u, _lib.DEMONS_FUSED, dict(env, PP_FUSED_MASK="0"))
    gen1 = _run(backend, monkeypatch, fix, mov, shape, sigma_u, _lib.DEMONS_FUSED,
                {k: v for k, v in env.items() if k == "PP_FUSED_TILE"} | {"PP_FUSED_GEN": "1"})
    staged = _run(backend, monkeypatch, fix, mov, shape, sigma_u, _lib.DEMONS_STAGED, {})
    assert "k_fused2_force_smooth" in branchy[3] and "k_fused_force_smooth" in gen1[3] and "k_demons_force" in staged[3]
    for name, other in (("branchy generation 2", branchy), ("generation 1", gen1), ("staged", staged)):
        diff = strips[0].view(np.int32) != other[0].view(np.int32)
        print(f"{case}: {name}: {int(diff.sum())} of {diff.size} field words differ, history {other[1]}")
    print(f"{case}: strips history {strips[1]}, counted {strips[2][0]} of {fix.size}")
    for name, other in (("branchy generation 2", branchy), ("generation 1", gen1), ("staged", staged)):
        np.testing.assert_array_equal(strips[0].view(np.int32), other[0].view(np.int32), err_msg=name)
        assert strips[2] == other[2], name
    assert strips[1] == branchy[1]      # the same per-thread sums in the same order
    # generation 1 and the staged schedule group the fp32 partial sums of the statistics differently
    np.testing.assert_allclose(np.array(strips[1]), np.array(gen1[1]), rtol=1e-6)
    np.testing.assert_allclose(np.array(strips[1]), np.array(staged[1]), rtol=1e-6)
