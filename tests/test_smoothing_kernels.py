"""The Gaussian smoothing kernels (pp_fir.hip, pp_iir.hip) against the fp64 restatements of tests/smoothing_restatement.py, on
every path of the two dispatch forests ("Smoothing, which shape enters which kernel"): each FIR kernel -- not
only k_conv_axis at the end of a chain of bit-equality tests -- and each IIR kernel is tied to a reference directly, at the
shapes where it takes another path: axes of one voxel, radii beyond the axis, a second march segment, rows beyond one
wavefront and beyond the LDS row, pointers off 16-byte alignment, in-place calls, listed rows, both sides of the
single-sweep threshold.

Bounds are derived, not tuned; the measured maxima go to record_stats("smoothing_fir" / "smoothing_iir").

  FIR   atol = 2^-24 * max|in| * sum_axes (2 r_axis + 2)
        The reference convolves with the library's own fp32 taps, so only the arithmetic differs.  A chain of fmaf over 2r + 1
        non-negative weights that sum to 1 errs by at most (2r + 1) u max|v| (u = 2^-24, every partial sum is bounded by
        max|v|); storing the pass adds one rounding, u max|v|; a later pass has gain <= 1, so earlier errors pass through
        undamped at worst and the three bounds add.
  IIR   per pass  |got - want| <= 2 ulp32(G max|in|),  G = impulse_gain of that pass (the L1 norm of its response)
        The restatement follows the kernel operation for operation in fp64, so the two differ only where fp64 noise (the
        order of a sum, a contracted multiply-add, the single sweep's 3e-13 warm-up) crosses an fp32 rounding boundary: of
        the causal half (one ulp of a value <= G max|in|, the two halves having disjoint supports) and then of the sum
        (another).  For a chain the per-pass bounds add, each multiplied by the gains of the passes after it.
        The number of values that differ AT ALL is capped at 1 + N / 1000 -- the project's own (diff > 0).mean() < 1e-3 of
        test_recursive_gaussian_single_sweep_equals_two_sweeps; a crossing needs ~1e-8 per value.
"""
import functools

import numpy as np
import pytest

from platipy_amd import _lib
from tests import smoothing_restatement as S
from tests.helpers import record_stats

U24 = 2.0 ** -24
_FIR_STATS, _IIR_STATS = {}, {}


def size_of(shape):
    return (shape[2], shape[1], shape[0])


def switch(monkeypatch, env):
    for name in ("PP_FIR_LEGACY", "PP_FIR_MARCH_SP", "PP_GAUSS3", "PP_RG_SEG_V1", "PP_RG_TWO_SWEEP"):
        if env and name in env:
            monkeypatch.setenv(name, env[name])
        else:
            monkeypatch.delenv(name, raising=False)


def offset_view(be, a):
    """`a` on the backend in a buffer whose first voxel is NOT 16-byte aligned: a view one float into a larger allocation
    (two floats where the allocation itself sits 12 bytes past a 16-byte boundary)."""
    flat = be.empty((a.size + 2,), np.uint8 if a.dtype == np.uint8 else np.float32)
    off = 1 if (_lib.ptr(flat) + 4) % 16 else 2
    v = flat[off:off + a.size].reshape(a.shape)
    v[...] = be.dev(a)
    assert _lib.ptr(v) % 16 != 0 and _lib.ptr(v) % 4 == 0
    return v


# --------------------------------------------------------------------------------------
# taps: the library's Gaussian operator against exact Bessel values (CPU only)


@pytest.mark.parametrize("max_width", [5, 32, 64, 127])
@pytest.mark.parametrize("max_error", [0.1, 0.01, 0.001])
def test_gauss_taps_against_exact_bessel(emu_backend, max_error, max_width):
    """ITK's recipe evaluates e^-v I_k(v) with the Abramowitz-Stegun polynomial fits (9.8.1-9.8.4, stated accuracy 2e-7) and a
    downward recurrence; scipy.special.ive is exact to double rounding.  Same length, values within 2e-7, for variances
    0.05 .. 110.  (Beyond that the recipe drifts -- 9.4e-7 at variance 150, 5.7e-4 at 400 -- and the reference implementation
    drifts with it: a property of the ITK operator, DESIGN.md 4.2, not asserted.)"""
    worst = 0.0
    for var in (0.05, 0.1, 0.3, 0.5, 1.0, 2.25, 4.0, 9.0, 12.0, 16.0, 30.0, 64.0, 110.0):
        got = np.asarray(_lib.gauss_taps(var, max_error, max_width, lib=emu_backend.lib))
        want = S.gaussian_operator_bessel(var, max_error, max_width)
        assert got.size == want.size, (var, got.size, want.size)
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.abs(got - want).max() <= 2e-7, (var, np.abs(got - want).max())
        assert abs(got.sum() - 1.0) < 1e-14 and np.array_equal(got, got[::-1])
    print("largest |tap - exact|", worst)      # measured: 1.5e-7


# --------------------------------------------------------------------------------------
# FIR: discrete_gaussian (fresh / unaligned / in place / listed rows) and smooth_field

V_SMALL, V_R8, V_MID, V_MIDX, V_R32 = (0.3, 1.0, 4.0), (9.0, 9.0, 9.0), (30.0, 64.0, 110.0), (110.0, 30.0, 64.0), (150.0, 150.0, 150.0)
UNIT = (1.0, 1.0, 1.0)
# id -> (shape (nz, ny, nx), variance (x, y, z), max_kernel_width, spacing, use_image_spacing); radii at max_error 0.01:
# variance 0.3 / 1 / 4 / 9 / 12 / 30 / 64 / 110 / 150 -> 2 / 3 / 5 / 8 / 9 / 14 / 21 / 27 / 32, variance 200 at width 127 -> 36
FIR_CASES = {
    # axes of one voxel, radii beyond the axis, nx % 4 != 0
    "row8-small": ((1, 1, 8), V_SMALL, 64, UNIT, False),
    "row8-fused": ((1, 1, 8), (0.3, 0.3, 0.3), 64, UNIT, False),          # k_gauss3_zyx on a single row
    "3x1x12-mid": ((3, 1, 12), V_MID, 64, UNIT, False),
    "3x1x12-r36": ((3, 1, 12), (200.0,) * 3, 127, UNIT, False),           # beyond radius 32: k_conv_x4, k_conv_axis<., 4>
    "1x37x4-r8": ((1, 37, 4), V_R8, 64, UNIT, False),
    "4x4x4-r32": ((4, 4, 4), V_R32, 64, UNIT, False),
    "5x7x9-small": ((5, 7, 9), V_SMALL, 64, UNIT, False),
    "5x7x9-mid": ((5, 7, 9), V_MID, 64, UNIT, False),
    "5x7x9-r36": ((5, 7, 9), (200.0,) * 3, 127, UNIT, False),             # k_conv_axis<., 1> on dense input
    "5x7x9-spacing": ((5, 7, 9), (4.0, 4.0, 4.0), 64, (0.9, 1.1, 2.5), True),
    # a row longer than 4096 (k_fir_x_row's fallback), x radius 27 and 14
    "4104-midx": ((2, 3, 4104), V_MIDX, 64, UNIT, False),
    "4104-mid": ((2, 3, 4104), V_MID, 64, UNIT, False),
    # a second segment of k_fir_march<RB, 4>, RB 2 / 4 / 8, in y and in z (the x radius of 5 keeps the fused kernel out)
    "march2-y": ((4, 41, 8), (4.0, 0.3, 1.0), 64, UNIT, False),
    "march2-z": ((41, 4, 8), (4.0, 1.0, 0.3), 64, UNIT, False),
    "march4-y": ((4, 73, 8), (4.0, 1.0, 0.3), 64, UNIT, False),
    "march4-z": ((73, 4, 8), (4.0, 0.3, 1.0), 64, UNIT, False),
    "march8-y": ((4, 137, 8), V_R8, 64, UNIT, False),
    "march8-z": ((137, 4, 8), V_R8, 64, UNIT, False),
    # ... and of the scalar-column form k_fir_march<8, 1>
    "march8s-y": ((4, 137, 9), V_R8, 64, UNIT, False),
    "march8s-z": ((137, 4, 9), V_R8, 64, UNIT, False),
    # a second segment of k_fir_march_sp: len >= 8 (2 r + 1) at r = 9
    "marchsp-y": ((3, 160, 4), (12.0,) * 3, 64, UNIT, False),
    "marchsp-z": ((160, 3, 4), (12.0,) * 3, 64, UNIT, False),
    # x rows longer than one wavefront's 256 voxels
    "260-r8": ((2, 3, 260), V_R8, 64, UNIT, False),
    "260-midx": ((2, 3, 260), V_MIDX, 64, UNIT, False),
    "260-r32": ((2, 3, 260), V_R32, 64, UNIT, False),
    # the fused kernel with tiles overhanging in x and y
    "fused-small": ((18, 20, 72), (0.3, 1.0, 1.0), 64, UNIT, False),
    "fused-spacing": ((18, 20, 72), (1.0, 1.0, 1.0), 64, (0.9, 1.1, 2.5), True),
}
FIR_FORMS = ("fresh", "unaligned", "inplace", "rows")
FIR_SWITCHED = ("fused-small", "marchsp-y", "260-midx")
FIR_SWITCHES = {"legacy": {"PP_FIR_LEGACY": "1"}, "march_sp0": {"PP_FIR_MARCH_SP": "0"}, "gauss3_0": {"PP_GAUSS3": "0"}}


def fir_image(shape, seed):
    return (1000.0 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def fir_taps(lib, variance_xyz, max_error, max_width, spacing, use_spacing):
    """The library's own fp32 taps per numpy axis (z, y, x), widened to fp64, and their radii."""
    taps = {}
    for a in range(3):
        var = variance_xyz[a] / (spacing[a] * spacing[a]) if use_spacing else variance_xyz[a]
        taps[2 - a] = np.float32(_lib.gauss_taps(var, max_error, max_width, lib=lib)).astype(np.float64)
    return taps, [(taps[k].size - 1) // 2 for k in range(3)]


_FIR_REF = {}


def fir_reference(lib, name):
    """(image, fp64 reference, atol) of a case: computed once, shared by every form, switch and backend (the taps are host
    code, the same doubles in every build)."""
    if name not in _FIR_REF:
        shape, var, mkw, spacing, use = FIR_CASES[name]
        img = fir_image(shape, 1000 + sorted(FIR_CASES).index(name))
        taps, radii = fir_taps(lib, var, 0.01, mkw, spacing, use)
        ref = S.fir_separable(img, taps, (0, 1, 2))                  # DiscreteGaussian convolves z, then y, then x
        ref.setflags(write=False)
        _FIR_REF[name] = (img, ref, U24 * float(np.abs(img).max()) * sum(2 * r + 2 for r in radii), radii)
    return _FIR_REF[name]


def need_rows(n):
    need = np.zeros(n, np.uint8)
    need[[0, n // 2, n - 1]] = 1
    return need


def run_discrete_gaussian(be, name, form):
    shape, var, mkw, spacing, use = FIR_CASES[name]
    img = fir_reference(be.lib, name)[0]
    size = size_of(shape)
    keep = np.ones(shape, bool)
    if form == "fresh":
        src, dst = be.dev(img), be.empty(shape)
    elif form == "unaligned":
        src, dst = offset_view(be, img), offset_view(be, np.zeros(shape, np.float32))
    elif form == "inplace":
        src = dst = be.dev(img)
    if form == "rows":
        ny_need, nz_need = need_rows(shape[1]), need_rows(shape[0])
        keep = (nz_need[:, None, None] & ny_need[None, :, None]).astype(bool) & keep
        src, dst = be.dev(img), be.empty(shape)
        be.ctx.discrete_gaussian_rows(src, dst, size, spacing, var, be.dev(ny_need), be.dev(nz_need), 0.01, mkw, use)
    else:
        be.ctx.discrete_gaussian(src, dst, size, spacing, var, 0.01, mkw, use)
    return np.array(be.host(dst), dtype=np.float64), keep


def check_fir(be, key, got, ref, atol, keep):
    err = float(np.abs(got - ref)[keep].max())
    _FIR_STATS[be.name + ":" + key] = {"max_abs_error": err, "atol": atol, "error_over_bound": err / atol}
    record_stats("smoothing_fir", _FIR_STATS)
    print(key, "max |error|", err, "bound", atol)
    assert np.isfinite(got[keep]).all() and err <= atol, (key, err, atol, np.argwhere(keep & ~(np.abs(got - ref) <= atol))[:5])


@pytest.mark.parametrize("form", FIR_FORMS)
@pytest.mark.parametrize("name", list(FIR_CASES))
def test_discrete_gaussian_against_fp64(backend, name, form, monkeypatch):
    switch(monkeypatch, None)
    _, ref, atol, _ = fir_reference(backend.lib, name)
    got, keep = run_discrete_gaussian(backend, name, form)
    check_fir(backend, f"{name}/{form}", got, ref, atol, keep)


@pytest.mark.parametrize("form", FIR_FORMS)
@pytest.mark.parametrize("sw", list(FIR_SWITCHES))
@pytest.mark.parametrize("name", FIR_SWITCHED)
def test_discrete_gaussian_variants_against_fp64(backend, name, sw, form, monkeypatch):
    """PP_FIR_LEGACY=1 (k_conv_axis / k_conv_x4 everywhere), PP_FIR_MARCH_SP=0 (no k_fir_march_sp / k_fir_x_row) and PP_GAUSS3=0
    (three launches instead of the fused kernel): every variant against the reference itself, not only against its sibling."""
    switch(monkeypatch, FIR_SWITCHES[sw])
    _, ref, atol, _ = fir_reference(backend.lib, name)
    got, keep = run_discrete_gaussian(backend, name, form)
    check_fir(backend, f"{name}/{form}/{sw}", got, ref, atol, keep)


_FIELD_REF = {}


def field_reference(lib, name):
    """smooth_field on the case's shape: three different components, sigma = sqrt(variance) in voxels, max_error 0.1, width 30."""
    if name not in _FIELD_REF:
        shape, var, _, spacing, use = FIR_CASES[name]
        sig = [np.sqrt(var[a]) / (spacing[a] if use else 1.0) for a in range(3)]
        f = np.stack([fir_image(shape, 2000 + 3 * sorted(FIR_CASES).index(name) + c) for c in range(3)])
        taps, radii = fir_taps(lib, [s * s for s in sig], 0.1, 30, UNIT, False)
        ref = np.stack([S.fir_separable(f[c], taps, (2, 1, 0)) for c in range(3)])      # SmoothDisplacementField: x, y, z
        ref.setflags(write=False)
        _FIELD_REF[name] = (f, sig, ref, U24 * float(np.abs(f).max()) * sum(2 * r + 2 for r in radii))
    return _FIELD_REF[name]


@pytest.mark.parametrize("name", list(FIR_CASES))
def test_smooth_field_against_fp64(backend, name, monkeypatch):
    switch(monkeypatch, None)
    f, sig, ref, atol = field_reference(backend.lib, name)
    d = backend.dev(f)
    backend.ctx.smooth_field(d, size_of(FIR_CASES[name][0]), sig, 0.1, 30)
    check_fir(backend, f"{name}/field", np.array(backend.host(d), dtype=np.float64), ref, atol, np.ones(ref.shape, bool))


@pytest.mark.parametrize("sw", ["legacy", "march_sp0"])
@pytest.mark.parametrize("name", FIR_SWITCHED)
def test_smooth_field_variants_against_fp64(backend, name, sw, monkeypatch):
    switch(monkeypatch, FIR_SWITCHES[sw])
    f, sig, ref, atol = field_reference(backend.lib, name)
    d = backend.dev(f)
    backend.ctx.smooth_field(d, size_of(FIR_CASES[name][0]), sig, 0.1, 30)
    check_fir(backend, f"{name}/field/{sw}", np.array(backend.host(d), dtype=np.float64), ref, atol, np.ones(ref.shape, bool))


# --------------------------------------------------------------------------------------
# IIR: recursive_gaussian_pass (order 0 and 1), recursive_gaussian, recursive_gaussian_field

IIR_SHAPES = [(4, 4, 4), (5, 33, 31), (33, 4, 64), (65, 32, 97), (4, 97, 5), (97, 5, 36)]
IIR_SPACINGS = [(1.0, 1.0, 1.0), (0.8, 1.3, 2.5)]
IIR_S = [0.3, 1.0, 1.54, 1.56, 4.0]          # sigma in voxels: 1.54 takes the single sweep, 1.56 the two-sweep kernels
PASS_KINDS = [(0, False), (1, False), (1, True)]     # (order, normalize_across_scale)


def ulp32(v):
    return float(np.spacing(np.float32(v)))


def iir_image(shape, seed, ncomp=None):
    full = (ncomp,) + tuple(shape) if ncomp else shape
    return (100.0 * np.random.default_rng(seed).standard_normal(full)).astype(np.float32)


def pass_scale(sigma, spacing, order, nas):
    return ((sigma if nas else 1.0) * (-1.0 if spacing < 0 else 1.0)) if order == 1 else 1.0


@functools.lru_cache(maxsize=None)
def pass_reference(shape, spacing, sigma, lib_axis, order, nas, seed):
    img = iir_image(shape, seed)
    sp = spacing[lib_axis]
    scale = pass_scale(sigma, sp, order, nas)
    want = S.deriche_pass(img, 2 - lib_axis, sigma, sp, order, scale)
    want.setflags(write=False)
    return img, want, 2.0 * ulp32(S.impulse_gain(sigma, sp, order, scale) * float(np.abs(img).max()))


@functools.lru_cache(maxsize=None)
def chain_reference(shape, spacing, sigma, seed, ncomp):
    """z, then x, then y (SmoothingRecursiveGaussian's order), every pass stored as fp32; the bound of the chain."""
    f = iir_image(shape, seed, ncomp)
    want = f if ncomp else f[None]
    m = float(np.abs(f).max())
    gains = [S.impulse_gain(sigma[a], spacing[a]) for a in (2, 0, 1)]
    bound = 0.0
    for p, a in enumerate((2, 0, 1)):
        want = np.stack([S.deriche_pass(c, 2 - a, sigma[a], spacing[a]) for c in want])
        bound += 2.0 * ulp32(float(np.prod(gains[:p + 1])) * m) * float(np.prod(gains[p + 1:]))
    want = want if ncomp else want[0]
    want.setflags(write=False)
    return f, want, bound


def check_iir(be, key, got, want, bound):
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    err, flips = float(diff.max()), int((diff > 0).sum())
    _IIR_STATS[be.name + ":" + key] = {"max_abs_error": err, "bound": bound, "flips": flips, "values": int(diff.size)}
    record_stats("smoothing_iir", _IIR_STATS)
    print(key, "max |error|", err, "bound", bound, "flips", flips, "of", diff.size)
    assert np.isfinite(got).all() and err <= bound, (key, err, bound, np.argwhere(~(diff <= bound))[:5])
    assert flips <= 1 + diff.size // 1000, (key, flips, diff.size)


def run_pass(be, img, shape, spacing, lib_axis, sigma, order, nas, unaligned=False):
    src = offset_view(be, img) if unaligned else be.dev(img)
    dst = offset_view(be, np.zeros(shape, np.float32)) if unaligned else be.empty(shape)
    be.ctx.recursive_gaussian_pass(src, dst, _lib.make_geom(size_of(shape), spacing), lib_axis, sigma, order, nas)
    return np.array(be.host(dst))


@pytest.mark.parametrize("s", IIR_S)
@pytest.mark.parametrize("spacing", IIR_SPACINGS)
@pytest.mark.parametrize("shape", IIR_SHAPES)
def test_recursive_gaussian_pass_against_fp64(backend, shape, spacing, s, monkeypatch):
    """One directional pass on each axis: the Gaussian, and its first derivative with NormalizeAcrossScale off and on."""
    switch(monkeypatch, None)
    for a in range(3):
        sigma = s * spacing[a]
        for order, nas in PASS_KINDS:
            img, want, bound = pass_reference(shape, spacing, sigma, a, order, nas, 31)
            got = run_pass(backend, img, shape, spacing, a, sigma, order, nas)
            check_iir(backend, f"pass/{shape}/{spacing}/s{s}/axis{a}/order{order}/nas{int(nas)}", got, want, bound)


@pytest.mark.parametrize("lib_axis", [0, 1, 2])
def test_recursive_gaussian_first_order_negative_spacing(backend, lib_axis, monkeypatch):
    """A negative spacing on the pass axis: ITK filters with its magnitude and negates the first-order response (the zero
    order ignores the sign).  Both sides of the single-sweep threshold."""
    switch(monkeypatch, None)
    shape = (5, 33, 31)
    spacing = [0.8, 1.3, 2.5]
    spacing[lib_axis] = -spacing[lib_axis]
    spacing = tuple(spacing)
    for s in (1.0, 4.0):
        sigma = s * abs(spacing[lib_axis])
        for order, nas in PASS_KINDS:
            img, want, bound = pass_reference(shape, spacing, sigma, lib_axis, order, nas, 32)
            got = run_pass(backend, img, shape, spacing, lib_axis, sigma, order, nas)
            check_iir(backend, f"pass-negative/s{s}/axis{lib_axis}/order{order}/nas{int(nas)}", got, want, bound)
            if order == 1:      # ... and it IS the negated response of the positive spacing
                pos = tuple(abs(v) for v in spacing)
                flipped = pass_reference(shape, pos, sigma, lib_axis, order, nas, 32)[1]
                assert np.array_equal(want, -flipped)
    # only the pass axis may carry the sign, and never a zero
    img = iir_image(shape, 32)
    for bad in ([-v for v in spacing], [0.0 if a == lib_axis else abs(v) for a, v in enumerate(spacing)]):
        with pytest.raises(_lib.PlatipyAmdError):
            backend.ctx.recursive_gaussian_pass(backend.dev(img), backend.empty(shape), _lib.make_geom(size_of(shape), bad), lib_axis, 1.0, 1, False)


def chain_sigmas():
    out = [(sp, tuple(s * v for v in sp)) for sp in IIR_SPACINGS for s in IIR_S]
    out.append(((0.6, 1.0, 2.0), (1.2, 1.2, 1.2)))      # 2.0 / 1.2 / 0.6 voxels: x two sweeps, y and z the single sweep, in one call
    return out


def run_chain(be, f, shape, spacing, sigma, ncomp, unaligned=False):
    g = _lib.make_geom(size_of(shape), spacing)
    if ncomp:
        d = offset_view(be, f) if unaligned else be.dev(f)
        be.ctx.recursive_gaussian_field(d, g, sigma)
        return np.array(be.host(d))
    src = offset_view(be, f) if unaligned else be.dev(f)
    dst = offset_view(be, np.zeros(shape, np.float32)) if unaligned else be.empty(shape)
    be.ctx.recursive_gaussian(src, dst, g, sigma)
    return np.array(be.host(dst))


@pytest.mark.parametrize("spacing_sigma", chain_sigmas(), ids=lambda v: "sp%g-%g-%g_sig%g-%g-%g" % (v[0] + v[1]))
@pytest.mark.parametrize("shape", IIR_SHAPES)
def test_recursive_gaussian_chain_against_fp64(backend, shape, spacing_sigma, monkeypatch):
    """recursive_gaussian (scalar, src -> dst) and recursive_gaussian_field (three components in place; an odd voxel count puts
    components 1 and 2 off 16-byte alignment)."""
    switch(monkeypatch, None)
    spacing, sigma = spacing_sigma
    for ncomp in (0, 3):
        f, want, bound = chain_reference(shape, spacing, sigma, 41, ncomp)
        got = run_chain(backend, f, shape, spacing, sigma, ncomp)
        check_iir(backend, f"chain/{shape}/{spacing}/{sigma}/comp{ncomp}", got, want, bound)


@pytest.mark.parametrize("s", [1.0, 4.0])
def test_recursive_gaussian_unaligned_views(backend, s, monkeypatch):
    """Rows of whole 16-byte quads (nx = 64) at pointers that are not 16-byte aligned: k_rg_x_seg<false> and k_rg_x<false> by
    alignment alone, and the strided kernels through offset bases."""
    switch(monkeypatch, None)
    shape, spacing = (33, 4, 64), (0.8, 1.3, 2.5)
    for a in range(3):
        for order, nas in PASS_KINDS[:2]:
            sigma = s * spacing[a]
            img, want, bound = pass_reference(shape, spacing, sigma, a, order, nas, 31)
            got = run_pass(backend, img, shape, spacing, a, sigma, order, nas, unaligned=True)
            check_iir(backend, f"unaligned-pass/s{s}/axis{a}/order{order}", got, want, bound)
    sigma = tuple(s * v for v in spacing)
    for ncomp in (0, 3):
        f, want, bound = chain_reference(shape, spacing, sigma, 41, ncomp)
        got = run_chain(backend, f, shape, spacing, sigma, ncomp, unaligned=True)
        check_iir(backend, f"unaligned-chain/s{s}/comp{ncomp}", got, want, bound)


@pytest.mark.parametrize("sw", [{"PP_RG_SEG_V1": "1"}, {"PP_RG_TWO_SWEEP": "1"}], ids=["seg_v1", "two_sweep"])
@pytest.mark.parametrize("s", [0.3, 1.54])
def test_recursive_gaussian_variants_against_fp64(backend, s, sw, monkeypatch):
    """k_rg_strided_seg (the fallback for components of 2^32 bytes and more, PP_RG_SEG_V1) and the two-sweep kernels at a sigma
    the single sweep would take (PP_RG_TWO_SWEEP), on the largest volume."""
    switch(monkeypatch, sw)
    shape, spacing = (65, 32, 97), (0.8, 1.3, 2.5)
    key = "+".join(sw)
    for a in range(3):
        for order, nas in PASS_KINDS[:2]:
            sigma = s * spacing[a]
            img, want, bound = pass_reference(shape, spacing, sigma, a, order, nas, 31)
            got = run_pass(backend, img, shape, spacing, a, sigma, order, nas)
            check_iir(backend, f"{key}/pass/s{s}/axis{a}/order{order}", got, want, bound)
    sigma = tuple(s * v for v in spacing)
    f, want, bound = chain_reference(shape, spacing, sigma, 41, 3)
    got = run_chain(backend, f, shape, spacing, sigma, 3)
    check_iir(backend, f"{key}/chain/s{s}", got, want, bound)
