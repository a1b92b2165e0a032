"""pp_invert_field_f32 / pp_inverse_consistency_f32 against the fp64 restatement (tests/field_inverse_restatement.py).

The bound of the comparison (inversion_bound in the restatement module), derived, never fitted to what the kernel returns.
Errors are measured in the norm the filter itself uses, e(x) = |(v_kernel(x) - v_ref(x)) / spacing|_2 (voxels); E_k bounds
max_x e(x) at the start of iteration k, E_1 = 0 (both sides start from the same fp32 numbers).  eps32 = 2^-24.

 * Warped point.  Its index displacement is diag(1 / spacing) Dir^T v; an error e in v moves it by at most sigma e, sigma the
   2-norm of diag(1 / spacing) Dir^T diag(spacing) (1 on axis-aligned grids).  The kernel forms it from nine fp32
   coefficients, three products and two sums per axis -- at most 6 eps32 W per axis, W the largest index displacement --,
   and splits it into floor and fraction with one more rounding of at most eps32: pos = sqrt(3) (6 eps32 W + eps32).
   dc_k = sigma E_k + pos must stay below the restatement's distance of every warped point from a +-0.5 plane (asserted), so
   both sides take the same inside / outside decision everywhere.
 * Sample.  Linear interpolation moves by at most L per unit of index displacement, L = the Frobenius norm of the three
   longest neighbour differences of u / spacing, one per axis (lipschitz_scaled, measured on the input).  Each of the seven lerps a + (b - a) w
   rounds three times on values of at most 2 U, 2 U and U: 5 eps32 U, three levels deep = 15 eps32 U per component, plus one
   rounding of the sum v + sample: 17 eps32 Us + eps32 Vs with Us, Vs the scaled norms of max |u| and of the estimate.
   Residual error: e_r <= (1 + L sigma) E_k + d_r,  d_r = L pos + 17 eps32 Us + eps32 Vs.  M and the mean are 1-Lipschitz
   in the residual (norm and max), so they carry e_r plus the norm's own 6 eps32 M.
 * Update.  v' = v + eps P(r), r = -(v + a), P the projection onto the ball of radius eps M: r -> r min(1, eps M / |r|).
   P is firmly non-expansive, so with the sample a and the radius held fixed v -> v - eps P(v + a) is non-expansive for
   eps <= 1: the old error passes through at most unchanged.  The sample's change enters through P with factor eps
   (eps (L sigma E_k + d_r)), the radius' change with factor eps (P is 1-Lipschitz in its radius) times eps e_M, and the
   update's own roundings (the norm twice, the quotient, three products, the sum) are d_u = eps32 (12 eps M + 5 M + 2 Vs):
       E_{k+1} <= (1 + eps L sigma) E_k + eps d_r + eps^2 e_M + d_u,   e_M <= (1 + L sigma) E_k + d_r + 6 eps32 M,
   i.e. (1 + eps L') E_k + delta with L' = L sigma + eps (1 + L sigma).  The boundary rule only sets both sides to 0.
   The factor is about 2.6 per iteration on the prototype field (L = 1.8, a field that folds): after ten iterations the
   bound is five orders of magnitude above fp32's resolution, and the kernel is expected to use a small fraction of it.
W, Vs and M come from the restatement's own history with 1 % + 1 voxel of slack.  The worst observed fraction of the bound
is recorded by record_stats (field_inverse_bound) and quoted in DESIGN 4.12."""
import ctypes as C

import numpy as np
import pytest

from platipy_amd import _lib
from tests import field_inverse_restatement as R
from tests.helpers import record_stats

# (nx, ny, nz): general small; crosses a 64-wide block with nx % 4 != 0; aligned; single-voxel axes; smallest volume
SHAPES = [(33, 18, 9), (70, 9, 5), (64, 8, 4), (1, 7, 6), (5, 1, 4), (6, 5, 1), (2, 2, 2)]
GEOMS = R.geometries()
_WORST = {"fraction": 0.0}


def zyx(size):
    return (size[2], size[1], size[0])


MAX_LIPSCHITZ = 1.85       # of the 33 x 18 x 9 prototype field (1.80); smaller grids get the amplitude that keeps them no rougher


def make_field(size, spacing, scale=1.0, seed=0):
    """The windowed sinusoid (3, 2, 4 mm), at most 0.3 voxel of displacement on axes too short to hold more, scaled down
    where the grid is so small that the field would be rougher than the prototype (an input property: the error
    recurrence's growth factor is 1 + eps L, and a bound that outgrows the buffer margin proves nothing)."""
    amp = [a * scale for a in (3.0, 2.0, 4.0)]
    for d in range(3):          # (exact for the axis-aligned geometries, a fair limit for the rotated one)
        if size[d] <= 2:
            amp[d] = min(amp[d], 0.3 * spacing[d])
    u = R.windowed_sinusoid(zyx(size), spacing, tuple(amp), seed)
    L = R.lipschitz_scaled(u, spacing)
    return u if L <= MAX_LIPSCHITZ else (u * np.float32(MAX_LIPSCHITZ / L * 0.999)).astype(np.float32)


def scaled_error(a, b, spacing):
    sp = np.asarray(spacing, dtype=np.float64).reshape(3, 1, 1, 1)
    return float(np.sqrt((((np.asarray(a, dtype=np.float64) - b) / sp) ** 2).sum(0)).max())


def run_invert(be, u, geom, iterations, max_tol=0.0, mean_tol=0.0, boundary=True, initial=None, want_stats=True):
    size = tuple(geom.size)
    out = be.dev(np.full((3,) + zyx(size), 7.0, np.float32))        # (whatever was there must be overwritten)
    info = be.ctx.invert_field(be.dev(u), geom, out, initial=None if initial is None else be.dev(initial), max_iterations=iterations,
                               max_tol=max_tol, mean_tol=mean_tol, enforce_boundary=boundary, want_stats=want_stats)
    return be.host(out).copy(), info


def note_fraction(err, bound):
    _WORST["fraction"] = max(_WORST["fraction"], err / bound)
    record_stats("field_inverse_bound", {"worst_fraction_of_bound": _WORST["fraction"]})


# --------------------------------------------------------------------------------------
# restatement self-checks (CPU only)


def test_restatement_constant_field_gives_minus_0_5625():
    c = np.zeros((3, 5, 6, 7), np.float32)
    c[0], c[1], c[2] = 1.0, -2.0, 0.5
    v, hist = R.invert(c, (1.0, 1.0, 1.0), maximum_number_of_iterations=1, enforce_boundary_condition=False)
    assert len(hist) == 1
    np.testing.assert_allclose(v, -0.5625 * c, rtol=0, atol=1e-15)


def test_restatement_max_error_falls_monotonically():
    sp = (0.9, 0.9, 2.5)
    u = make_field((33, 18, 9), sp)
    _, hist = R.invert(u, sp, max_error_tolerance_threshold=0.0, mean_error_tolerance_threshold=0.0)
    M = [h["M"] for h in hist]
    assert len(M) == 10 and all(b < a for a, b in zip(M, M[1:])), M
    assert 1.5 < M[0] < 3.0 and M[-1] < 0.3, M


# --------------------------------------------------------------------------------------
# kernel against restatement at fixed iteration counts


@pytest.mark.parametrize("gname", list(GEOMS))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_restatement_at_fixed_iterations(backend, size, gname):
    spacing, origin, direction = GEOMS[gname]
    geom = _lib.make_geom(size, spacing, origin, direction.ravel())
    u = make_field(size, spacing)
    v0 = (-0.5 * u).astype(np.float32)
    for boundary in (True, False):
        for initial in (None, v0):
            ref, hist = R.invert(u, spacing, direction, 10, 0.0, 0.0, boundary, initial)
            assert len(hist) == 10
            assert min(h["margin"] for h in hist) >= 1e-3, "a warped point of the test field sits on a buffer plane"
            for iterations in (1, 2, 10):
                b = R.inversion_bound(u, spacing, direction, hist, iterations)
                assert max(b["dc"]) < min(h["margin"] for h in hist[:iterations])      # the derivation's precondition
                got, info = run_invert(backend, u, geom, iterations, boundary=boundary, initial=initial)
                err = scaled_error(got, hist[iterations - 1]["v"], spacing)
                print(f"{size} {gname} boundary={boundary} initial={initial is not None} k={iterations}: err {err:.3e} bound {b['E']:.3e}")
                assert err <= b["E"], (err, b["E"])
                note_fraction(err, b["E"])
                assert info["iterations"] == iterations
                h = hist[iterations - 1]
                assert abs(info["max_error_norm"] - h["M"]) <= b["e_r"][-1]
                assert abs(info["mean_error_norm"] - h["mean"]) <= b["e_r"][-1] + 2.0 ** -25


def test_constant_field_kernel(backend):
    size = (7, 6, 5)
    c = np.zeros((3,) + zyx(size), np.float32)
    c[0], c[1], c[2] = 1.0, -2.0, 0.5
    got, info = run_invert(backend, c, _lib.make_geom(size), 1, boundary=False)
    np.testing.assert_allclose(got, -0.5625 * c, rtol=0, atol=4 * 2.0 ** -24)
    assert info["iterations"] == 1


def test_zero_iterations_returns_the_initial_estimate(backend):
    size = (6, 5, 4)
    u = make_field(size, (1.0, 1.0, 1.0))
    got, info = run_invert(backend, u, _lib.make_geom(size), 0, initial=u)
    assert np.array_equal(got, u) and info["iterations"] == 0 and np.isinf(info["max_error_norm"])
    got, _ = run_invert(backend, u, _lib.make_geom(size), 0)
    assert not got.any()


# --------------------------------------------------------------------------------------
# outside rule


def outside_probe(size, spacing, direction, seed):
    """(u, v0): an estimate that throws voxel i, by i % 9, at least 0.25 voxel beyond each of the six faces (0 ... 5), into the
    [-0.5, 0) band of one axis (6), into the [n - 1, n - 0.5) band (7), or somewhere inside (8); u is a windowed sinusoid plus
    a large constant, so that the two arms of a decision give results that differ by tens of voxels."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = zyx(size)
    n = (nx, ny, nz)
    z, y, x = np.indices((nz, ny, nx))
    idx = np.stack([x, y, z]).astype(np.float64)
    lin = (z * ny + y) * nx + x
    group = lin % 9
    target = np.stack([rng.uniform(0.0, n[a] - 1.0, size=x.shape) for a in range(3)])
    axis = (lin // 9) % 3
    for a in range(3):
        beyond = rng.uniform(0.25, 1.25, size=x.shape)
        target[a] = np.where(group == 2 * a, -0.5 - beyond, target[a])
        target[a] = np.where(group == 2 * a + 1, n[a] - 0.5 + beyond, target[a])
        target[a] = np.where((group == 6) & (axis == a), rng.uniform(-0.45, -0.05, size=x.shape), target[a])
        target[a] = np.where((group == 7) & (axis == a), n[a] - 1.0 + rng.uniform(0.05, 0.45, size=x.shape), target[a])
    dv = (target - idx) * np.asarray(spacing).reshape(3, 1, 1, 1)
    v0 = np.einsum("rc,czyx->rzyx", np.asarray(direction, dtype=np.float64), dv).astype(np.float32)
    u = R.windowed_sinusoid((nz, ny, nx), spacing, seed=seed) + np.array([60.0, -50.0, 80.0], np.float32).reshape(3, 1, 1, 1)
    return u.astype(np.float32), v0, group


@pytest.mark.parametrize("gname", ["identity", "rot20"])
def test_outside_rule(backend, gname):
    size = (33, 18, 9)
    spacing, origin, direction = GEOMS[gname]
    geom = _lib.make_geom(size, spacing, origin, direction.ravel())
    u, v0, group = outside_probe(size, spacing, direction, 5)
    res = R.residual(u, v0, spacing, direction)
    assert res["margin"] >= 1e-3
    ins = res["inside"]
    assert not ins[group < 6].any() and ins[group >= 6].all()       # the probe does what it says
    ref, hist = R.invert(u, spacing, direction, 1, 0.0, 0.0, False, v0)
    b = R.inversion_bound(u, spacing, direction, hist, 1)
    assert b["dc"][0] < res["margin"]
    # the decision of every voxel, read off the norm image: the two arms differ by |u / spacing| >= 30 voxels
    norm = backend.dev(np.zeros(zyx(size), np.float32))
    st = backend.ctx.inverse_consistency(backend.dev(u), backend.dev(v0), geom, norm_out=norm)
    s = backend.host(norm).astype(np.float64)
    sp = np.asarray(spacing).reshape(3, 1, 1, 1)
    s_out = np.sqrt(((v0.astype(np.float64) / sp) ** 2).sum(0))
    s_in_or_ref = res["s"]
    kernel_inside = np.where(ins, np.abs(s - s_in_or_ref) <= b["e_r"][0], np.abs(s - s_out) > b["e_r"][0])
    assert np.array_equal(kernel_inside, ins), int((kernel_inside != ins).sum())
    assert np.abs(s - res["s"]).max() <= b["e_r"][0]
    assert abs(st["max"] - res["M"]) <= b["e_r"][0] and abs(st["mean"] - res["mean"]) <= b["e_r"][0] + 2.0 ** -25
    got, _ = run_invert(backend, u, geom, 1, boundary=False, initial=v0)
    err = scaled_error(got, ref, spacing)
    assert err <= b["E"], (err, b["E"])
    note_fraction(err, b["E"])


# --------------------------------------------------------------------------------------
# stopping


STOP_CASES = {
    # name: (amplitude scale, max iterations, iterations the restatement runs, the rule that decides)
    "mean_rule": (0.8, 10, 8, "mean"),
    "max_rule": (0.1, 10, 2, "max"),
    "out_of_iterations": (1.0, 5, 5, None),
}


@pytest.mark.parametrize("case", list(STOP_CASES))
def test_stopping(backend, case):
    scale, max_iter, expect, rule = STOP_CASES[case]
    size, spacing = (33, 18, 9), (0.9, 0.9, 2.5)
    max_tol, mean_tol = 0.1, 0.001
    u = make_field(size, spacing, scale)
    _, full = R.invert(u, spacing, np.eye(3), max_iter, 0.0, 0.0)
    ref, hist = R.invert(u, spacing, np.eye(3), max_iter, max_tol, mean_tol)
    assert len(hist) == expect
    # from the restatement alone: every iteration that continues clears BOTH thresholds by 10 %, the one that stops misses
    # the deciding threshold by 10 %
    for h in full[:expect - 1] if rule else full[:expect]:
        assert h["M"] >= 1.1 * max_tol and h["mean"] >= 1.1 * mean_tol
    last = full[expect - 1]
    if rule == "mean":
        assert last["mean"] <= 0.9 * mean_tol and last["M"] >= 1.1 * max_tol
    elif rule == "max":
        assert last["M"] <= 0.9 * max_tol and last["mean"] >= 1.1 * mean_tol
    b = R.inversion_bound(u, spacing, np.eye(3), full, expect)
    geom = _lib.make_geom(size, spacing)
    got, info = run_invert(backend, u, geom, max_iter, max_tol, mean_tol)
    assert info["iterations"] == expect
    assert abs(info["max_error_norm"] - last["M"]) <= b["e_r"][-1]
    assert abs(info["mean_error_norm"] - last["mean"]) <= b["e_r"][-1] + 2.0 ** -25
    err = scaled_error(got, ref, spacing)
    assert err <= b["E"], (err, b["E"])
    note_fraction(err, b["E"])
    # the same field without a read-back: only enqueued, the same bits
    quiet, none = run_invert(backend, u, geom, max_iter, max_tol, mean_tol, want_stats=False)
    assert none is None and np.array_equal(quiet, got)


# --------------------------------------------------------------------------------------
# determinism, arguments


def test_two_calls_return_the_same_bits(backend):
    size, (spacing, origin, direction) = (70, 9, 5), GEOMS["rot20"]
    geom = _lib.make_geom(size, spacing, origin, direction.ravel())
    u = make_field(size, spacing)
    a, ia = run_invert(backend, u, geom, 6)
    b, ib = run_invert(backend, u, geom, 6)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ia == ib
    ca = backend.ctx.inverse_consistency(backend.dev(u), backend.dev(a), geom)
    cb = backend.ctx.inverse_consistency(backend.dev(u), backend.dev(a), geom)
    assert ca == cb


def test_null_aliased_and_oversized_arguments(backend):
    lib, h = backend.lib, backend.ctx.h
    size = (6, 5, 4)
    geom = _lib.make_geom(size)
    u = backend.dev(np.zeros((3,) + zyx(size), np.float32))
    v = backend.dev(np.zeros((3,) + zyx(size), np.float32))
    s = backend.dev(np.zeros(zyx(size), np.float32))
    p = _lib.ptr
    st, js = _lib.InvertStats(), _lib.JacobianStats()
    g = C.byref(geom)
    inv = lambda *a: lib.pp_invert_field_f32(h, *a)      # noqa: E731
    assert inv(None, g, None, 3, 0.0, 0.0, 1, p(v), None) == _lib.ERR_ARG
    assert inv(p(u), g, None, 3, 0.0, 0.0, 1, None, None) == _lib.ERR_ARG
    assert inv(p(u), g, None, 3, 0.0, 0.0, 1, p(u), None) == _lib.ERR_ARG
    assert inv(p(u), g, p(v), 3, 0.0, 0.0, 1, p(v), None) == _lib.ERR_ARG
    assert inv(p(u), None, None, 3, 0.0, 0.0, 1, p(v), None) == _lib.ERR_ARG
    assert inv(p(u), g, None, -1, 0.0, 0.0, 1, p(v), None) == _lib.ERR_ARG
    assert inv(p(u), g, None, _lib.INVERT_MAX_ITERATIONS + 1, 0.0, 0.0, 1, p(v), None) == _lib.ERR_ARG
    assert inv(p(u), g, None, 3, float("nan"), 0.0, 1, p(v), None) == _lib.ERR_ARG
    ice = lambda *a: lib.pp_inverse_consistency_f32(h, *a)      # noqa: E731
    assert ice(None, p(v), g, None, C.byref(st)) == _lib.ERR_ARG
    assert ice(p(u), None, g, None, C.byref(st)) == _lib.ERR_ARG
    assert ice(p(u), p(v), g, None, None) == _lib.ERR_ARG
    assert ice(p(u), p(v), g, p(u), C.byref(st)) == _lib.ERR_ARG
    jac = lambda *a: lib.pp_jacobian_determinant_f32(h, *a)      # noqa: E731
    assert jac(None, g, 1, None, p(s), None) == _lib.ERR_ARG
    assert jac(p(u), g, 1, None, None, None) == _lib.ERR_ARG
    assert jac(p(u), g, 1, None, p(u), None) == _lib.ERR_ARG
    assert jac(p(u), None, 1, None, p(s), None) == _lib.ERR_ARG
    # fields of 2^32 bytes and more, or an axis beyond a grid dimension, are refused before anything is launched
    for big in ((2048, 2048, 128), (65536, 2, 2)):
        gb = C.byref(_lib.make_geom(big))
        assert inv(p(u), gb, None, 3, 0.0, 0.0, 1, p(v), None) == _lib.ERR_SIZE
        assert ice(p(u), p(v), gb, None, C.byref(st)) == _lib.ERR_SIZE
        assert jac(p(u), gb, 1, None, p(s), C.byref(js)) == _lib.ERR_SIZE
    # the binding turns a refusal into ValueError
    with pytest.raises(ValueError):
        backend.ctx.invert_field(u, geom, u)


def test_python_interface_arguments(host_api):
    import torch

    pa = host_api
    from platipy_amd.registration import invert_displacement_field, inverse_consistency_error

    size, spacing = (9, 8, 7), (1.0, 1.2, 2.5)
    dev = pa.runtime.default_device()
    u = make_field(size, spacing, 0.5)
    field = pa.Image(torch.from_numpy(u).to(dev), spacing, (1.0, 2.0, 3.0))
    with pytest.raises(ValueError):
        invert_displacement_field(pa.Image(torch.zeros(zyx(size), device=dev), spacing))
    with pytest.raises(ValueError):
        invert_displacement_field(field, initial_estimate=pa.Image(torch.from_numpy(u).to(dev), spacing, (0.0, 0.0, 0.0)))
    with pytest.raises(ValueError):
        inverse_consistency_error(field, pa.Image(torch.from_numpy(u).to(dev), spacing, (0.0, 0.0, 0.0)))
    inv32, info = invert_displacement_field(field, 4, 0.0, 0.0, return_info=True)
    assert inv32.is_vector and inv32.tensor.dtype == torch.float32 and inv32.same_grid(field)
    assert set(info) == {"iterations", "max_error_norm", "mean_error_norm"} and info["iterations"] == 4
    inv64 = invert_displacement_field(pa.Image(torch.from_numpy(u.astype(np.float64)).to(dev), spacing, (1.0, 2.0, 3.0)), 4, 0.0, 0.0)
    assert inv64.tensor.dtype == torch.float32 and torch.equal(inv64.tensor, inv32.tensor)      # an fp64 field is converted
    warm = invert_displacement_field(field, 2, 0.0, 0.0, initial_estimate=inv32)
    res, img = inverse_consistency_error(field, warm, return_image=True)
    assert not img.is_vector and img.shape == zyx(size) and abs(float(img.tensor.max()) - res["max"]) == 0.0
    assert res["max"] < info["max_error_norm"]


# --------------------------------------------------------------------------------------
# inverse consistency


def test_inverse_consistency_is_the_next_iterations_residual(backend):
    size, (spacing, origin, direction) = (33, 18, 9), GEOMS["rot20"]
    geom = _lib.make_geom(size, spacing, origin, direction.ravel())
    u = make_field(size, spacing)
    _, hist = R.invert(u, spacing, direction, 4, 0.0, 0.0)
    b = R.inversion_bound(u, spacing, direction, hist, 4)
    # u against an arbitrary estimate: the restatement's residual norms
    v = (-0.7 * u).astype(np.float32)
    res = R.residual(u, v, spacing, direction)
    norm = backend.dev(np.zeros(zyx(size), np.float32))
    st = backend.ctx.inverse_consistency(backend.dev(u), backend.dev(v), geom, norm_out=norm)
    assert np.abs(backend.host(norm) - res["s"]).max() <= b["e_r"][0]
    assert abs(st["max"] - res["M"]) <= b["e_r"][0] and abs(st["mean"] - res["mean"]) <= b["e_r"][0] + 2.0 ** -25
    # v = invert(u) with k iterations: M and mean of the restatement's iteration k + 1
    k = 3
    got, _ = run_invert(backend, u, geom, k)
    st = backend.ctx.inverse_consistency(backend.dev(u), backend.dev(got), geom)
    assert abs(st["max"] - hist[k]["M"]) <= b["e_r"][k]
    assert abs(st["mean"] - hist[k]["mean"]) <= b["e_r"][k] + 2.0 ** -25
