"""Cubic B-spline transform, its two kernels (pp_bspline_field_f32, pp_bspline_metric_f32), lattice refinement and
pa.registration.bspline_registration, held to the fp64 numpy restatement in tests/bspline_restatement.py (parity with ITK
itself is unpinned: DESIGN.md section 8)."""
import inspect

import numpy as np
import pytest
import torch

from platipy_amd import _lib
from tests import bspline_restatement as R

SIZE, SPACING, ORIGIN = (33, 27, 20), (0.9, 1.1, 2.5), (320.0, -52.0, 60.0)
EYE = (1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0)
FLIP = (-1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0)
MESH_A, MESH_B = (3, 2, 2), (1, 1, 1)


def _lattice(mesh, direction=EYE):
    return R.initializer(SIZE, SPACING, ORIGIN, direction, mesh)


def _lat_geom(lat):
    return _lib.make_geom(lat["lattice_size"], lat["lattice_spacing"], lat["lattice_origin"], lat["direction"].ravel())


def _coef(lat, seed, sigma):
    cx, cy, cz = (int(s) for s in lat["lattice_size"])
    return np.random.default_rng(seed).normal(0, sigma, size=(3, cz, cy, cx)).astype(np.float32)


def _field(backend, coef, lat, grid):
    out = backend.empty((3, grid[0][2], grid[0][1], grid[0][0]))
    backend.ctx.bspline_field(backend.dev(coef), _lat_geom(lat), _lib.make_geom(*grid[:3], np.ravel(grid[3])), out)
    return backend.host(out)


# ---- 1. initialiser and parameters --------------------------------------------------------------------------------------


@pytest.mark.parametrize("direction", [EYE, FLIP])
def test_initializer_and_parameter_order(host_api, direction):
    pa = host_api
    img = pa.Image(np.zeros(SIZE[::-1], dtype=np.float32), SPACING, ORIGIN, direction)
    t = pa.bspline_transform_initializer(img, MESH_A)
    want = _lattice(MESH_A, direction)
    assert t.GetOrder() == 3
    assert tuple(t.GetTransformDomainMeshSize()) == MESH_A
    np.testing.assert_allclose(t.GetTransformDomainOrigin(), want["domain_origin"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(t.GetTransformDomainPhysicalDimensions(), want["domain_dimensions"], rtol=1e-15)
    np.testing.assert_allclose(np.reshape(t.GetTransformDomainDirection(), (3, 3)), want["direction"], rtol=0, atol=0)
    images = t.GetCoefficientImages()
    assert len(images) == 3 and tuple(images[0].GetSize()) == tuple(want["lattice_size"]) == (6, 5, 5)
    np.testing.assert_allclose(images[0].GetSpacing(), want["lattice_spacing"], rtol=1e-15)
    np.testing.assert_allclose(images[0].GetOrigin(), want["lattice_origin"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.reshape(images[0].GetDirection(), (3, 3)), want["direction"], rtol=0, atol=0)
    assert t.GetNumberOfParameters() == len(t.GetParameters()) == 450
    assert all(v == 0.0 for v in t.GetParameters())
    coef = _coef(want, 3, 3.0)
    t.SetParameters(R.flat_parameters(coef))
    np.testing.assert_array_equal(np.asarray(t.GetParameters(), dtype=np.float32), R.flat_parameters(coef))
    for c, im in enumerate(t.GetCoefficientImages()):
        np.testing.assert_array_equal(im.numpy(), coef[c])
    with pytest.raises(ValueError):
        t.SetParameters(np.zeros(449))


def test_control_point_spacing_distance_to_number(host_api):
    pa = host_api
    img = pa.Image(np.zeros(SIZE[::-1], dtype=np.float32), SPACING, ORIGIN)
    for spacing in (10, 24, 64, [8, 16, 30], 7.5):
        got = pa.registration.control_point_spacing_distance_to_number(img, spacing)
        want = R.control_point_spacing_distance_to_number(SIZE, SPACING, spacing)
        assert got.dtype.kind == "i" and np.array_equal(got, want)


# ---- 2. kernel A ---------------------------------------------------------------------------------------------------------


def _grids(direction=EYE):
    D = np.reshape(direction, (3, 3))
    own = (SIZE, SPACING, ORIGIN, D)
    sp = tuple(0.7 * s for s in SPACING)
    big = (tuple(int(np.ceil(n / 0.7)) + 8 for n in SIZE), sp, tuple(np.asarray(ORIGIN) - D @ (4.0 * np.asarray(sp))), D)
    return own, big


@pytest.mark.parametrize("case", ["own", "larger", "flipped", "oblique"])
def test_field_kernel_against_restatement(backend, case):
    direction = FLIP if case == "flipped" else EYE
    lat = _lattice(MESH_A, direction)
    coef = _coef(lat, 11, 3.0)
    own, big = _grids(direction)
    grid = {"own": own, "larger": big, "flipped": big, "oblique": big}[case]
    if case == "oblique":     # the grid turned by 20 degrees about z against the lattice: the per-voxel weight path
        c, s = np.cos(np.radians(20.0)), np.sin(np.radians(20.0))
        grid = (big[0], big[1], big[2], np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]))
    if case == "flipped":     # ... and the lattice flipped against an unflipped grid
        grid = (big[0], big[1], tuple(np.asarray(ORIGIN) - np.array([(SIZE[0] - 1) * SPACING[0], 0.0, 0.0]) - 4.0 * np.asarray(big[1])),
                np.eye(3))
    got = _field(backend, coef, lat, grid)
    want = R.field(coef, lat, *grid)
    # a 64-term convex combination of |c| <= max|c|: 66 x 2^-24 = 3.9e-6 max|c| if formed in fp32, the rest of 1e-5 max|c| for the
    # fp32 rounding of a fractional lattice coordinate; the kernel forms it in fp64 and rounds once, so it sits far inside
    err = np.abs(got - want).max()
    print(f"{case}: max |kernel - restatement| = {err:.3e} mm, max|c| = {np.abs(coef).max():.3f}")
    assert err <= 1e-5 * np.abs(coef).max()
    inside, _, _ = R.support(R.grid_points(*grid), lat)
    inside = inside.reshape(got.shape[1:])
    assert inside.sum() > 1000
    if case != "own":
        assert (~inside).sum() > 0
    assert np.all(got[:, ~inside] == 0.0)
    # exact properties
    zero = _field(backend, np.zeros_like(coef), lat, grid)
    assert np.all(zero == 0.0)
    const = np.empty_like(coef)
    vals = np.array([2.71828, -13.5, 0.3], dtype=np.float32)
    const[:] = vals[:, None, None, None]
    got_c = _field(backend, const, lat, grid)
    for r in range(3):
        ulp = np.spacing(np.abs(vals[r]))
        assert np.abs(got_c[r][inside] - vals[r]).max() <= 4 * ulp      # partition of unity
        assert np.all(got_c[r][~inside] == 0.0)


# ---- 3. plumbing ---------------------------------------------------------------------------------------------------------


def _transform(pa, mesh, seed, sigma, direction=EYE):
    img = pa.Image(np.zeros(SIZE[::-1], dtype=np.float32), SPACING, ORIGIN, direction)
    t = pa.bspline_transform_initializer(img, mesh)
    lat = _lattice(mesh, direction)
    coef = _coef(lat, seed, sigma)
    t.SetParameters(R.flat_parameters(coef))
    return t, coef, lat


def test_apply_transform_and_composites(host_api):
    pa = host_api
    t, coef, lat = _transform(pa, MESH_A, 5, 3.0)
    vol = R.blobs(SIZE[::-1], 1, noise=2.0)
    img = pa.Image(vol, SPACING, ORIGIN)
    mask = pa.Image((vol > 80).astype(np.uint8), SPACING, ORIGIN)
    field = pa.registration.transform_to_displacement_field(t, img)
    np.testing.assert_array_equal(field.numpy(), t.displacement_field(img).cpu().numpy())
    err = np.abs(field.numpy() - R.field(coef, lat, SIZE, SPACING, ORIGIN, np.eye(3))).max()
    assert err <= 1e-5 * np.abs(coef).max()
    as_field = pa.DisplacementFieldTransform(field)
    apply = pa.registration.apply_transform
    a = apply(mask, transform=t, interpolator=pa.sitkNearestNeighbor)
    b = apply(mask, transform=as_field, interpolator=pa.sitkNearestNeighbor)
    assert a.tensor.dtype == torch.uint8 and torch.equal(a.tensor, b.tensor) and 0 < int(a.tensor.sum()) != int(mask.tensor.sum())
    a = apply(img, transform=t, interpolator=pa.sitkLinear, default_value=-7)
    b = apply(img, transform=as_field, interpolator=pa.sitkLinear, default_value=-7)
    assert torch.equal(a.tensor, b.tensor)
    affine = pa.AffineTransform(np.array([[1.02, 0.03, 0], [-0.03, 0.98, 0], [0, 0, 1.0]]), (1.5, -2.0, 0.5), (330.0, -40.0, 80.0))
    for order in ("affine_first", "bspline_first"):
        members = (lambda x: [affine, x]) if order == "affine_first" else (lambda x: [x, affine])
        a = apply(img, transform=pa.CompositeTransform(members(t)), interpolator=pa.sitkLinear)
        b = apply(img, transform=pa.CompositeTransform(members(as_field)), interpolator=pa.sitkLinear)
        assert torch.equal(a.tensor, b.tensor)
        assert not torch.equal(a.tensor, apply(img, transform=affine, interpolator=pa.sitkLinear).tensor)


# ---- 4. kernel B ---------------------------------------------------------------------------------------------------------

MOVING = ((31, 29, 22), (1.0, 1.0, 2.3), (318.5, -53.0, 58.0), np.eye(3))
_SHARED = {}


def _metric_inputs():
    """images, masks, jitter and gradient image shared by the kernel B tests (built once, never written to)"""
    if "fixed" not in _SHARED:
        fixed = R.blobs(SIZE[::-1], 21, noise=3.0)
        moving = R.blobs(MOVING[0][::-1], 22, noise=3.0)
        nz, ny, nx = SIZE[::-1]
        zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        fmask = ((((xx - 16) / 14.0) ** 2 + ((yy - 13) / 11.0) ** 2 + ((zz - 10) / 8.5) ** 2) < 1).astype(np.uint8)
        mmask = np.ones(MOVING[0][::-1], dtype=np.uint8)
        mmask[:, :, 24:] = 0
        mmask[:4] = 0
        grad = np.stack([np.gradient(moving.astype(np.float64), axis=a) for a in (2, 1, 0)]).astype(np.float32)
        packed = np.ascontiguousarray(np.concatenate([np.moveaxis(grad, 0, -1), moving[..., None]], axis=-1))
        rng = np.random.default_rng(23)
        jitter = {s: (rng.standard_normal(((np.prod(SIZE) + s - 1) // s, 3)) / 3.0).astype(np.float32) for s in (1, 2)}
        _SHARED.update(fixed=fixed, moving=moving, fmask=fmask, mmask=mmask, grad=grad, packed=packed, jitter=jitter)
    return _SHARED


CASES = [
    # metric, mesh, stride, jitter, gradient source (None: analytic, "planar": gradient image, "packed": image + float4 companion), masks
    ("mean_squares", MESH_A, 1, False, None, False),
    ("mean_squares", MESH_A, 2, True, "packed", True),
    ("mean_squares", MESH_B, 1, True, None, True),
    ("mean_squares", MESH_A, 2, True, "planar", True),
    ("correlation", MESH_A, 2, False, "packed", False),
    ("correlation", MESH_B, 1, True, None, True),
    ("correlation", MESH_A, 1, True, "packed", True),
    ("correlation", MESH_A, 2, True, "planar", False),
]


@pytest.mark.parametrize("metric,mesh,stride,jitter,packed,masks", CASES)
def test_metric_kernel_against_restatement(backend, metric, mesh, stride, jitter, packed, masks):
    d = _metric_inputs()
    direction = FLIP if (mesh == MESH_A and stride == 2 and metric == "correlation" and packed == "packed") else EYE       # one flipped-direction case
    D = np.reshape(direction, (3, 3))
    lat = _lattice(mesh, direction)
    coef = _coef(lat, 31, 1.5)
    origin = ORIGIN if direction == EYE else (ORIGIN[0] + (SIZE[0] - 1) * SPACING[0], ORIGIN[1], ORIGIN[2])
    if direction != EYE:
        lat = R.initializer(SIZE, SPACING, origin, direction, mesh)
    fg = (SIZE, SPACING, origin, D)
    jit = d["jitter"][stride] if jitter else None
    fm, mm = (d["fmask"], d["mmask"]) if masks else (None, None)
    want_v, want_g, want_s = R.metric(metric, d["fixed"], fg, d["moving"], MOVING, fg, stride, coef, lat, fm, mm, jit,
                                      d["grad"] if packed else None)
    ctx = backend.ctx
    keep = [backend.dev(d["fixed"]), backend.dev(d["moving"]), backend.dev(coef), None if fm is None else backend.dev(fm),
            None if mm is None else backend.dev(mm), None if jit is None else backend.dev(jit), backend.dev(d["grad"]), backend.dev(d["packed"])]
    geom = _lib.make_geom(SIZE, SPACING, origin, direction)
    try:
        if jit is not None:
            ctx.set_sample_jitter(keep[5])
        if packed == "packed":
            ctx.set_moving_gradient(keep[6], packed=keep[7])
        elif packed == "planar":
            ctx.set_moving_gradient(keep[6])
        args = (_lib.BSPLINE_MEAN_SQUARES if metric == "mean_squares" else _lib.BSPLINE_CORRELATION, keep[0], geom, keep[1],
                _lib.make_geom(*MOVING[:3], MOVING[3].ravel()), geom, stride, keep[2], _lat_geom(lat), keep[3], keep[4],
                0.0 if jit is None else float(np.abs(jit).max()))
        v1, g1, s1 = ctx.bspline_metric(*args)
        v2, g2, s2 = ctx.bspline_metric(*args)
    finally:
        ctx.set_sample_jitter(None)
        ctx.set_moving_gradient(None)
    assert v1 == v2 and np.array_equal(g1, g2) and s1 == s2                       # bit-identical between calls
    assert s1["valid"] == want_s["valid"] and s1["outside"] == want_s["outside"] and s1["masked"] == want_s["masked"]
    assert s1["seen"] == want_s["seen"] == (np.prod(SIZE) + stride - 1) // stride
    assert want_s["outside"] > 0                                                    # samples leave the moving buffer
    if masks:
        assert want_s["masked"] > 0
    gmax = np.abs(want_g).max()
    print(f"value {v1:.9g} / {want_v:.9g}; max |g - want| = {np.abs(g1 - want_g).max():.3e}, max |g| = {gmax:.3e}, valid {s1['valid']}")
    assert gmax > 0
    np.testing.assert_allclose(v1, want_v, rtol=1e-5)
    if metric == "mean_squares":
        np.testing.assert_allclose(g1, want_g, rtol=2e-4, atol=1e-3 * gmax)
    else:
        np.testing.assert_allclose(g1, want_g, rtol=3e-4, atol=1e-3 * gmax)


@pytest.mark.parametrize("metric", ["mean_squares", "correlation"])
def test_restated_gradient_against_central_differences(metric):
    """CPU only: checks the yardstick, not the product."""
    d = _metric_inputs()
    lat = _lattice(MESH_A)
    coef = _coef(lat, 31, 1.5).astype(np.float64)
    fg = (SIZE, SPACING, ORIGIN, np.eye(3))
    jit = d["jitter"][2]
    _, g, _ = R.metric(metric, d["fixed"], fg, d["moving"], MOVING, fg, 2, coef, lat, d["fmask"], None, jit)
    rng = np.random.default_rng(41)
    # control points whose gradient is not negligible (an entry 1e-6 of the largest cannot be held to rtol 1e-5 by differences)
    big = np.nonzero(np.abs(g) > 1e-2 * np.abs(g).max())[0]
    h = 1e-4
    for p in rng.choice(big, size=10, replace=False):
        plus, minus = coef.copy().reshape(-1), coef.copy().reshape(-1)
        plus[p] += h
        minus[p] -= h
        vp = R.metric(metric, d["fixed"], fg, d["moving"], MOVING, fg, 2, plus.reshape(coef.shape), lat, d["fmask"], None, jit)[0]
        vm = R.metric(metric, d["fixed"], fg, d["moving"], MOVING, fg, 2, minus.reshape(coef.shape), lat, d["fmask"], None, jit)[0]
        np.testing.assert_allclose((vp - vm) / (2 * h), g[p], rtol=1e-5)


# ---- 5. refinement -------------------------------------------------------------------------------------------------------


def test_refinement_keeps_the_deformation(host_api):
    pa = host_api
    t, coef, lat = _transform(pa, MESH_A, 7, 3.0)
    fine = pa.registration.refine_bspline(t, [2 * m for m in MESH_A])
    assert tuple(fine.GetTransformDomainMeshSize()) == (6, 4, 4)
    assert fine.GetTransformDomainOrigin() == t.GetTransformDomainOrigin()
    img = pa.Image(np.zeros(SIZE[::-1], dtype=np.float32), SPACING, ORIGIN)
    before, after = t.displacement_field(img).cpu().numpy(), fine.displacement_field(img).cpu().numpy()
    diff = np.abs(before - after).max(axis=0)
    # voxels at least two fine cells from the domain border
    cell = np.asarray(SIZE, dtype=np.float64) / np.array([6, 4, 4])       # fine cell in voxels
    zz, yy, xx = np.meshgrid(*(np.arange(n) for n in SIZE[::-1]), indexing="ij")
    interior = np.ones(diff.shape, dtype=bool)
    for idx, n, c in ((xx, SIZE[0], cell[0]), (yy, SIZE[1], cell[1]), (zz, SIZE[2], cell[2])):
        interior &= (idx + 0.5 >= 2 * c) & (n - 0.5 - idx >= 2 * c)
    # With mesh A x 2 = (6, 4, 4) no voxel centre lies two fine cells from BOTH z borders (20 voxels, 5 per cell), so the
    # interior bound is asserted on the whole domain instead, which includes it: refine_bspline pads the lattice before the
    # prefilter, leaving 0.268^12 = 1.4e-7 of max|c| ~ 12 mm from the mirror rule plus fp32 rounding of the coefficients.
    border = diff[~interior].max() if (~interior).any() else 0.0
    print(f"refinement: max {diff.max():.3e} mm over the domain, {border:.3e} mm within two fine cells of the border, "
          f"max|c| {np.abs(coef).max():.2f}")
    assert diff.max() <= 1e-4
    assert np.all(np.isfinite(after)) and border < np.abs(coef).max()


# ---- 6. end to end -------------------------------------------------------------------------------------------------------

E2E_SIZE, E2E_SPACING = (48, 40, 32), (1.5, 1.5, 2.0)


def _e2e_pair():
    if "e2e" not in _SHARED:
        from scipy.ndimage import gaussian_filter

        shape = E2E_SIZE[::-1]
        fixed = gaussian_filter(R.blobs(shape, 51).astype(np.float64), 1.0).astype(np.float32)
        zz, yy, xx = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
        label = ((((xx - 22) / 9.0) ** 2 + ((yy - 21) / 8.0) ** 2 + ((zz - 15) / 7.0) ** 2) < 1).astype(np.uint8)
        lat = R.initializer(E2E_SIZE, E2E_SPACING, (0, 0, 0), np.eye(3), (2, 2, 2))
        rng = np.random.default_rng(52)      # |coefficient| <= 3 mm bounds the displacement; x and y keep a sign so the label moves
        true = np.stack([rng.uniform(1.5, 3.0, size=(5, 5, 5)), rng.uniform(-3.0, -1.0, size=(5, 5, 5)), rng.uniform(-3.0, 3.0, size=(5, 5, 5))])
        geom = (E2E_SIZE, E2E_SPACING, (0.0, 0.0, 0.0), np.eye(3))
        moving = R.warp_linear(fixed, geom, true, lat).astype(np.float32)
        moving_label = R.warp_linear(label, geom, true, lat, nearest=True).astype(np.uint8)
        _SHARED["e2e"] = (fixed, label, moving, moving_label, geom)
    return _SHARED["e2e"]


def test_registration_against_restated_optimiser(host_api):
    from scipy.optimize import fmin_l_bfgs_b

    from tests.helpers import dice

    pa = host_api
    fixed, label, moving, moving_label, geom = _e2e_pair()
    f_img, m_img = pa.Image(fixed, E2E_SPACING), pa.Image(moving, E2E_SPACING)
    out, t = pa.registration.bspline_registration(f_img, m_img, resolution_staging=[1], smooth_sigmas=[0], grid_scale_factors=[1],
                                                  initial_grid_spacing=24, sampling_rate=1.0, itk_sampling=False, optimiser="lbfgsb",
                                                  number_of_iterations=20, metric="mean_squares")
    mesh = tuple(R.control_point_spacing_distance_to_number(E2E_SIZE, E2E_SPACING, 24))
    assert tuple(t.GetTransformDomainMeshSize()) == mesh
    lat = R.initializer(E2E_SIZE, E2E_SPACING, (0, 0, 0), np.eye(3), mesh)
    shape = (3,) + tuple(int(s) for s in lat["lattice_size"][::-1])

    def fun(x):
        v, g, _ = R.metric("mean_squares", fixed, geom, moving, geom, geom, 1, x.reshape(shape), lat)
        return v, g

    x, _, _ = fmin_l_bfgs_b(fun, np.zeros(int(np.prod(shape))), m=5, factr=1e7, pgtol=1e-5, maxiter=20, maxfun=1024)
    want_final = fun(x)[0]
    first, last = t.level_values[0]
    print(f"end to end: initial {first:.6f}, product final {last:.6f}, restated optimiser final {want_final:.6f}")
    np.testing.assert_allclose(first, fun(np.zeros(int(np.prod(shape))))[0], rtol=1e-5)
    assert last <= 1.10 * want_final
    assert last < first
    moved = pa.registration.apply_transform(pa.Image(moving_label, E2E_SPACING), f_img, t, 0, pa.sitkNearestNeighbor)
    assert dice(moved.numpy(), label) >= dice(moving_label, label)
    assert out.tensor.dtype == torch.float32 and tuple(out.GetSize()) == E2E_SIZE


def test_registration_staging(host_api):
    pa = host_api
    fixed, _, moving, _, _ = _e2e_pair()
    f_img, m_img = pa.Image(fixed, E2E_SPACING), pa.Image(np.round(moving).astype(np.int16), E2E_SPACING)
    out, t = pa.registration.bspline_registration(f_img, m_img, resolution_staging=[2, 1], smooth_sigmas=[1, 0], grid_scale_factors=[1, 2],
                                                  initial_grid_spacing=24, sampling_rate=0.5, itk_sampling=True, number_of_iterations=6)
    mesh = R.control_point_spacing_distance_to_number(E2E_SIZE, E2E_SPACING, 24)
    assert tuple(t.GetTransformDomainMeshSize()) == tuple(2 * mesh)
    assert t.level_values[-1][1] < t.level_values[-1][0]
    assert out.tensor.dtype == torch.int16 and out.same_grid(f_img)


# ---- 7. surface ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("structures", [False, True])
def test_registration_isotropic_resample(host_api, structures):
    """isotropic_resample puts both images on new grids; the structures stay where the caller drew them and must reach the kernel
    on the grids it indexes (ITK's masks live in physical space)."""
    pa = host_api
    fixed, label, moving, moving_label, _ = _e2e_pair()
    f_img, m_img = pa.Image(fixed, E2E_SPACING), pa.Image(moving, E2E_SPACING)
    kw = {}
    if structures:
        body = np.ones_like(label)
        body[:, :, :6] = 0
        kw = {"fixed_structure": pa.Image(body, E2E_SPACING), "moving_structure": pa.Image(np.ones_like(label), E2E_SPACING)}
    out, t = pa.registration.bspline_registration(f_img, m_img, resolution_staging=[2], smooth_sigmas=[0], grid_scale_factors=[1],
                                                  initial_grid_spacing=24, sampling_rate=0.5, itk_sampling=False, optimiser="lbfgsb",
                                                  number_of_iterations=5, isotropic_resample=True, initial_isotropic_size=2, **kw)
    assert out.same_grid(f_img) and out.tensor.dtype == torch.float32
    first, last = t.level_values[0]
    assert np.isfinite(last) and last < first
    # the transform domain is the resampled fixed image's box
    iso = pa.registration.smooth_and_resample(f_img, isotropic_voxel_size_mm=2)
    np.testing.assert_allclose(t.GetTransformDomainPhysicalDimensions(), np.asarray(iso.GetSize()) * np.asarray(iso.GetSpacing()), rtol=1e-12)
    if structures:      # the mask took samples away: the two runs do not start from the same value
        _, t0 = pa.registration.bspline_registration(f_img, m_img, resolution_staging=[2], smooth_sigmas=[0], grid_scale_factors=[1],
                                                     initial_grid_spacing=24, sampling_rate=0.5, itk_sampling=False, optimiser="lbfgsb",
                                                     number_of_iterations=1, isotropic_resample=True, initial_isotropic_size=2)
        assert t0.level_values[0][0] != first


def test_structures_may_be_none(host_api):
    pa = host_api
    fixed, _, moving, _, _ = _e2e_pair()
    f_img, m_img = pa.Image(fixed, E2E_SPACING), pa.Image(moving, E2E_SPACING)
    _, t = pa.registration.bspline_registration(f_img, m_img, fixed_structure=None, moving_structure=None, resolution_staging=[4],
                                                smooth_sigmas=[0], grid_scale_factors=[1], initial_grid_spacing=36, sampling_rate=1.0,
                                                itk_sampling=False, optimiser="lbfgsb", number_of_iterations=1)
    assert len(t.level_values) == 1


def test_binding_refuses_a_mask_of_another_size(backend):
    """... instead of letting the kernel read past its end"""
    d = _metric_inputs()
    lat = _lattice(MESH_A)
    geom = _lib.make_geom(SIZE, SPACING, ORIGIN, EYE)
    with pytest.raises(ValueError):
        backend.ctx.bspline_metric(_lib.BSPLINE_MEAN_SQUARES, backend.dev(d["fixed"]), geom, backend.dev(d["moving"]),
                                   _lib.make_geom(*MOVING[:3], MOVING[3].ravel()), geom, 1, backend.dev(_coef(lat, 1, 1.0)), _lat_geom(lat),
                                   fixed_mask=backend.dev(d["mmask"]))


def test_signature_and_refusals(host_api):
    pa = host_api
    want = {"fixed_image": inspect.Parameter.empty, "moving_image": inspect.Parameter.empty, "fixed_structure": False,
            "moving_structure": False, "resolution_staging": [8, 4, 2], "smooth_sigmas": [4, 2, 1], "sampling_rate": 0.1,
            "optimiser": "LBFGS", "metric": "mean_squares", "initial_grid_spacing": 64, "grid_scale_factors": [1, 2, 4],
            "interp_order": 3, "default_value": -1000, "number_of_iterations": 20, "isotropic_resample": False,
            "initial_isotropic_size": 1, "number_of_histogram_bins_mi": 30, "verbose": False, "ncores": 8, "itk_sampling": True}
    got = {k: p.default for k, p in inspect.signature(pa.registration.bspline_registration).parameters.items()}
    assert list(got) == list(want) and got == want
    assert pa.sitkBSpline == 3
    img = pa.Image(R.blobs((8, 9, 10), 1), (2.0, 2.0, 2.0))
    reg = pa.registration.bspline_registration
    for kw in ({"metric": "mutual_information"}, {"metric": "demons"}, {"optimiser": "cgls"}):
        with pytest.raises(NotImplementedError):
            reg(img, img, **kw)
    for kw in ({"metric": "sum_of_squares"}, {"optimiser": "adam"}):
        with pytest.raises(ValueError):
            reg(img, img, **kw)


def test_metric_refuses_a_lattice_direction_other_than_the_fixed_images(backend):
    d = _metric_inputs()
    lat = _lattice(MESH_A, FLIP)
    geom = _lib.make_geom(SIZE, SPACING, ORIGIN, EYE)
    with pytest.raises(_lib.PlatipyAmdError) as e:
        backend.ctx.bspline_metric(_lib.BSPLINE_MEAN_SQUARES, backend.dev(d["fixed"]), geom, backend.dev(d["moving"]),
                                   _lib.make_geom(*MOVING[:3], MOVING[3].ravel()), geom, 1, backend.dev(_coef(lat, 1, 1.0)), _lat_geom(lat))
    assert e.value.code == _lib.ERR_DIRECTION == -7
