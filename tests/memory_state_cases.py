"""The case table of tests/test_memory_state.py: one case (or a few) per C-ABI entry point that writes device memory or reserves
scratch.  A case is a plain function run(leg) that makes the call with every OUTPUT buffer taken from the leg (leg.empty /
leg.hempty / leg.hstruct: zeros on the base leg, garbage on the others) and returns {name: numpy array} of everything the call
defines, and a check(leg, outs) that holds the base leg to the operation's reference with the bound of the operation's own test.

Contracts: every output of every case is `written` (each element defined by the call) unless the case lists it in
`accumulates` -- pp_fuse_accumulate_u8 / _f32 (wsum, wlsum) and the running total of pp_compose_field_f32, the in/out
arguments of include/platipy_amd.h; those start from defined values on every leg.  In-place filters (pp_smooth_field_f32,
pp_recursive_gaussian_field_f32, pp_rescale_threshold_f32) read what they overwrite: their buffer is an input.

Inputs, references and bounds come from the operation's existing test module (named next to each case) or from the
restatement modules; nothing here sets a tolerance of its own.
"""
import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

from platipy_amd import _lib
from tests.helpers import host_garbage

FLT_MAX = float(np.finfo(np.float32).max)


# --------------------------------------------------------------------------------------
# a leg: the backend with a context of its own and output buffers pre-filled per leg


class Leg:
    """What a case sees of a backend: `ctx` is the leg's context, `empty` hands out OUTPUT buffers holding the leg's fill
    (float pattern for float types, integer pattern for the others; an int is a byte value, a float an element value)."""

    def __init__(self, be, ctx, fpat, ipat, spat):
        self.be, self.ctx, self.lib, self.name = be, ctx, be.lib, be.name
        self.fpat, self.ipat, self.spat = fpat, ipat, spat
        self._keep = []

    def _pattern(self, dtype):
        return self.fpat if np.dtype(dtype).kind == "f" else self.ipat

    def dev(self, a, align=None):
        """`align`: the alignment in bytes that include/platipy_amd.h requires of this buffer.  Whole allocations have it; the
        offset views of tests/buffer_views.py keep it."""
        return self.be.dev(a if a.flags.writeable else a.copy())       # (the shared, read-only inputs of other test modules)

    def p(self, a, align=None):
        """The address of `a` on the backend, for a raw call; the buffer lives as long as the leg."""
        self._keep.append(self.dev(a))
        return _lib.ptr(self._keep[-1])

    def host(self, h):
        self.ctx.sync()
        return np.array(h.cpu().numpy() if hasattr(h, "cpu") else h)

    def empty(self, shape, dtype=np.float32, align=None):
        return self.be.garbage(shape, dtype, self._pattern(dtype))

    def hempty(self, shape, dtype=np.float64):
        """A HOST output array (statistics, histograms, counts)."""
        return host_garbage(shape, dtype, self._pattern(dtype))

    def hstruct(self, ctype):
        """A host output struct, every byte holding the leg's struct pattern."""
        s = ctype()
        C.memset(C.byref(s), self.spat, C.sizeof(s))
        return s


def fields(s, skip=("reserved",), **cut):
    """A ctypes struct as {field: array}; `reserved` members are not outputs; cut[name] = n keeps the first n of an array."""
    out = {}
    for name, _ in s._fields_:
        if name in skip:
            continue
        v = np.array(getattr(s, name))
        out[name] = v[:cut[name]] if name in cut else v
    return out


def hptr(a, ctype=C.c_double):
    return a.ctypes.data_as(C.POINTER(ctype))


def size_of(shape):
    return (shape[2], shape[1], shape[0])


@dataclass
class Case:
    id: str
    fns: tuple                  # the entry points this case covers
    run: object                 # run(leg) -> {name: array}
    check: object               # check(leg, outs): the base leg against the reference
    nvox: int                   # voxels (or samples) of the case: the dirtier works on as many
    scratch: bool = True        # the call reserves context scratch
    accumulates: tuple = ()     # outputs with an in/out contract
    family: str = ""            # the dirtier comes from ANOTHER family
    bad: object = None          # bad(leg) -> status of the case's own call with a NULL input (else a generic PP_ERR_ARG call)
    setters: tuple = ()         # pp_linear_set_* entry points in force during the call


CASES = []


def case(id, fns, nvox, check, **kw):
    def deco(run):
        CASES.append(Case(id=id, fns=tuple(fns) if not isinstance(fns, str) else (fns,), run=run, check=check, nvox=int(nvox), **kw))
        return run
    return deco


@functools.lru_cache(maxsize=None)
def T(name):
    """tests.test_<name>: the operation's own test module (inputs, references, bounds)."""
    import importlib

    return importlib.import_module("tests.test_" + name)


# ======================================================================================
# Gaussian smoothing (tests/test_smoothing_kernels.py: FIR_CASES, IIR_SHAPES; bounds check_fir / check_iir)

FIR_NAMES = ["5x7x9-mid", "march8s-y", "fused-small"]       # nx % 4 != 0 twice, more than one tile in x


def _fir(name, form):
    S = T("smoothing_kernels")
    shape = S.FIR_CASES[name][0]

    def run(leg):
        got, keep = S.run_discrete_gaussian(leg, name, form)
        return {"out": got[keep]}

    def check(leg, outs):
        _, ref, atol, _ = S.fir_reference(leg.lib, name)
        keep = np.ones(shape, bool)
        if form == "rows":
            keep = (S.need_rows(shape[0])[:, None, None] & S.need_rows(shape[1])[None, :, None]).astype(bool) & keep
        full = np.zeros(shape)
        full[keep] = outs["out"]
        S.check_fir(leg, f"memory-state/{name}/{form}", full, ref, atol, keep)      # test_discrete_gaussian_against_fp64

    fn = "pp_discrete_gaussian_rows_f32" if form == "rows" else "pp_discrete_gaussian_f32"
    # (the fused three-axis kernel of a dense small-radius call keeps its planes in LDS: no scratch)
    case(f"fir-{form}-{name}", fn, np.prod(shape), check, family="smooth", scratch=not (name == "fused-small" and form == "fresh"))(run)


for _n in FIR_NAMES:
    _fir(_n, "fresh")
for _n in ("5x7x9-mid", "fused-small"):
    _fir(_n, "rows")


def _smooth_field(name):
    S = T("smoothing_kernels")
    shape = S.FIR_CASES[name][0]

    def run(leg):
        f, sig, _, _ = S.field_reference(leg.lib, name)
        d = leg.dev(f)
        leg.ctx.smooth_field(d, size_of(shape), sig, 0.1, 30)
        return {"field": leg.host(d)}

    def check(leg, outs):
        _, _, ref, atol = S.field_reference(leg.lib, name)
        S.check_fir(leg, f"memory-state/{name}/field", outs["field"].astype(np.float64), ref, atol, np.ones(ref.shape, bool))   # test_smooth_field_against_fp64

    case(f"smooth-field-{name}", "pp_smooth_field_f32", 3 * np.prod(shape), check, family="smooth")(run)


for _n in ("5x7x9-mid", "fused-small"):
    _smooth_field(_n)

IIR_CASES = [((5, 33, 31), (0.8, 1.3, 2.5)), ((33, 4, 64), (1.0, 1.0, 1.0))]


def _iir_pass(shape, spacing):
    S = T("smoothing_kernels")
    combos = [(a, s, order, nas) for a in range(3) for s in (1.0, 4.0) for order, nas in ((0, False), (1, True))]

    def run(leg):
        out = {}
        for a, s, order, nas in combos:
            img = S.pass_reference(shape, spacing, s * spacing[a], a, order, nas, 31)[0]
            out[f"axis{a}-s{s}-order{order}"] = S.run_pass(leg, img, shape, spacing, a, s * spacing[a], order, nas)
        return out

    def check(leg, outs):
        for a, s, order, nas in combos:
            _, want, bound = S.pass_reference(shape, spacing, s * spacing[a], a, order, nas, 31)
            S.check_iir(leg, f"memory-state/pass/{shape}/axis{a}/s{s}/order{order}", outs[f"axis{a}-s{s}-order{order}"], want, bound)  # test_recursive_gaussian_pass_against_fp64

    case(f"iir-pass-{'x'.join(map(str, shape))}", "pp_recursive_gaussian_pass_f32", np.prod(shape), check, family="smooth", scratch=False)(run)


def _iir_chain(shape, spacing):
    S = T("smoothing_kernels")
    sigmas = [tuple(s * v for v in spacing) for s in (1.0, 4.0)]

    for ncomp, fn in ((0, "pp_recursive_gaussian_f32"), (3, "pp_recursive_gaussian_field_f32")):
        def run(leg, ncomp=ncomp):
            return {f"sigma{k}": S.run_chain(leg, S.chain_reference(shape, spacing, sg, 41, ncomp)[0], shape, spacing, sg, ncomp)
                    for k, sg in enumerate(sigmas)}

        def check(leg, outs, ncomp=ncomp):
            for k, sg in enumerate(sigmas):
                _, want, bound = S.chain_reference(shape, spacing, sg, 41, ncomp)
                S.check_iir(leg, f"memory-state/chain/{shape}/{sg}/comp{ncomp}", outs[f"sigma{k}"], want, bound)   # test_recursive_gaussian_chain_against_fp64

        case(f"iir-{'field' if ncomp else 'scalar'}-{'x'.join(map(str, shape))}", fn, max(ncomp, 1) * np.prod(shape), check, family="smooth")(run)


for _shape, _sp in IIR_CASES:
    _iir_pass(_shape, _sp)
    _iir_chain(_shape, _sp)


# ======================================================================================
# warp / resample (tests/test_resample_kernels.py: the oblique grids, part of every output outside the input)


def _oblique(din, dout):
    K = T("resample_kernels")
    R = K.R
    gin, gout, A, t, fld = K.oblique_case(din, dout)
    img, lab = K.oblique_images()
    kw = dict(A=A, t=t, field=fld)
    EDGE = K.EDGE

    def run(leg):
        return {"f32-linear": K.run_resample(leg, img, gin, gout, K.LIN, EDGE, **kw),
                "f32-nearest": K.run_resample(leg, img, gin, gout, K.NEAR, EDGE, **kw),
                "u8-nearest": K.run_resample(leg, lab, gin, gout, K.NEAR, 300.0, **kw),
                "u8-linear": K.run_resample(leg, lab, gin, gout, K.LIN, 300.0, **kw)}

    def check(leg, outs):      # test_oblique_resample
        ref = R.resample(img, gin, gout, default=EDGE, **kw)
        assert 0.2 <= ref["inside"].mean() <= 0.8            # the default-value path writes
        edge_band = K.near_boundary(ref["c"], gin.size, 1e-9, ties=False)
        tie_band = K.near_boundary(ref["c"], gin.size, 1e-9, ties=True)
        K.check_linear("memory-state oblique", outs["f32-linear"], ref, K.tol_fp64(ref["M"]), keep=~edge_band, default=EDGE)
        want = R.resample(img, gin, gout, interp="nearest", default=EDGE, **kw)["out"]
        np.testing.assert_array_equal(outs["f32-nearest"][~tie_band], want[~tie_band])
        want = R.resample(lab, gin, gout, interp="nearest", default=300.0, u8=True, **kw)["out"]
        np.testing.assert_array_equal(outs["u8-nearest"][~tie_band], want[~tie_band])
        r8 = R.resample(lab, gin, gout, default=300.0, u8=True, **kw)
        shaky = r8["inside"] & (r8["R"] > 0) & (np.abs(r8["ref"] - np.round(r8["ref"])) < K.tol_fp64(r8["M"]))
        keep = ~(shaky | edge_band)
        np.testing.assert_array_equal(outs["u8-linear"][keep], r8["out"][keep])

    case(f"resample-oblique-{din}-{dout}", ("pp_resample_f32", "pp_resample_u8"), np.prod(K.OB_OUT_SHAPE), check, family="resample", scratch=False)(run)

    def run_field(leg):
        rng = np.random.default_rng(3)
        f = (rng.uniform(5.0, 20.0, (3,) + K.OB_IN_SHAPE) * rng.choice([-1.0, 1.0], (3, 1, 1, 1))).astype(np.float32)
        return {"out": K.run_resample_field(leg, f, gin, gout)}

    def check_field(leg, outs):     # test_oblique_resample_field
        rng = np.random.default_rng(3)
        f = (rng.uniform(5.0, 20.0, (3,) + K.OB_IN_SHAPE) * rng.choice([-1.0, 1.0], (3, 1, 1, 1))).astype(np.float32)
        ref = R.resample_field(f, gin, gout)
        band = K.near_boundary(ref["c"], gin.size, 1e-9, ties=False)
        got = outs["out"]
        for k in range(3):
            assert np.array_equal((got[k] != 0.0)[~band], ref["inside"][~band])
        err, tol = np.abs(got - ref["out"])[:, ~band], K.tol_fp64(ref["M"])[:, ~band]
        assert (err <= tol).all(), (err / tol).max()
        assert 0.2 <= ref["inside"].mean() <= 0.8

    case(f"resample-field-oblique-{din}-{dout}", "pp_resample_field_f32", 3 * np.prod(K.OB_OUT_SHAPE), check_field, family="resample", scratch=False)(run_field)


_oblique("rot", "rotflip")
_oblique("perm", "rot")


def _warp_compose(k):
    K = T("resample_kernels")
    R = K.R
    g, img, f = K.random_case(*K.RANDOM_GRIDS[k])
    it = (np.random.default_rng(1).uniform(5.0, 20.0, (3,) + g.shape)).astype(np.float32)

    def run(leg):
        return {"out": K.run_warp(leg, img, f, g, K.EDGE)}

    def check(leg, outs):       # test_random_warp_and_compose
        ref = R.resample(img, g, g, field=f, default=K.EDGE)
        band = K.fp32_band(ref["c"], f, g)
        assert 0.02 < (~ref["inside"]).mean() < 0.6
        K.check_linear("memory-state warp", outs["out"], ref, K.tol_fp32(ref["M"], ref["R"], f, g.spacing), keep=~band, default=K.EDGE)

    case(f"warp-{k}", "pp_warp_f32", np.prod(g.shape), check, family="resample", scratch=False)(run)

    def run_c(leg):
        return {"total": K.run_compose(leg, f, it, g)}       # the running total: in/out, starts from the defined field f

    def check_c(leg, outs):
        rc = R.compose(f, it, g)
        band = K.fp32_band(rc["c"], f, g)
        got = outs["total"]
        for c in range(3):
            assert np.array_equal((got[c] != f[c])[~band], rc["inside"][~band])
        tol = K.tol_fp32(rc["M"], rc["R"], f, g.spacing) + K.U24 * np.abs(rc["out"])
        err = np.abs(got - rc["out"])[:, ~band]
        assert (err <= tol[:, ~band]).all()

    case(f"compose-{k}", "pp_compose_field_f32", 3 * np.prod(g.shape), check_c, family="resample", scratch=False, accumulates=("total",))(run_c)


_warp_compose(0)
_warp_compose(1)


def _transform_to_field(direction, with_add):
    K = T("resample_kernels")
    g = K.grid_of((6, 9, 11), (0.83, 1.27, 1.9), (-31.7, 12.3, 105.1), K.DIRS[direction])
    A = K.rot_xyz(-8.0, 5.0, 12.0) @ np.array([[1.1, 0.03, 0.0], [0.0, 0.93, 0.02], [-0.01, 0.0, 1.04]])
    t = np.array([12.5, -7.25, 3.1])
    add = np.random.default_rng(9).normal(0.0, 30.0, (3,) + g.shape).astype(np.float32) if with_add else None

    def run(leg):
        out = leg.empty((3,) + g.shape)
        leg.ctx.transform_to_field(K.geom_of(g), A, t, None if add is None else leg.dev(add), out)
        return {"out": leg.host(out)}

    def check(leg, outs):       # test_transform_to_field
        plain, want = K.R.affine_displacement(g, A, t, add)
        tol = 2.0 ** -23 * np.abs(plain).max() + (K.U24 * np.abs(want) if with_add else 0.0)
        assert (np.abs(outs["out"] - want) <= tol).all()

    case(f"transform-to-field-{direction}-{'add' if with_add else 'plain'}", "pp_transform_to_field_f32", 3 * np.prod(g.shape), check,
         family="resample", scratch=False)(run)


_transform_to_field("rot", False)
_transform_to_field("rotflip", True)


def _prefilter(shape):
    K = T("resample_kernels")
    vol = np.random.default_rng(1000 + shape[2]).normal(0.0, 1000.0, shape).astype(np.float32)

    def run(leg):
        out = leg.empty(shape)
        leg.ctx.bspline_prefilter(leg.dev(vol), size_of(shape), out)
        return {"out": leg.host(out)}

    def check(leg, outs):       # test_bspline_prefilter
        want = K.R.bspline_prefilter(vol)
        bound = 4.0 * np.abs(K.R.bspline_prefilter_fp32_storage(vol) - want).max()
        assert np.abs(outs["out"] - want).max() <= bound

    case(f"bspline-prefilter-{'x'.join(map(str, shape))}", "pp_bspline_prefilter_f32", np.prod(shape), check, family="resample", scratch=False)(run)


_prefilter((3, 4, 41))
_prefilter((19, 4, 5))


def _resample_set(name):
    RS = T("resample_set")
    K = T("resample_kernels")
    gin, gout, A, t, fld = RS.geometry(name)
    kw = dict(A=A, t=t, field=fld)
    img, labs = RS.volumes(gin.shape, 3, 20)

    def run(leg):
        got_img, got_labs = RS.run_set(leg, img, labs, gin, gout, **kw)
        res = {"image": got_img}
        res.update({f"label{k}": o for k, o in enumerate(got_labs)})
        return res

    def check(leg, outs):
        # test_set_equals_members: every output is pp_resample_f32 / _u8 of that member alone, bit for bit ...
        want = RS.run_members(leg, img, labs, gin, gout, **kw)
        RS.assert_same((outs["image"], [outs[f"label{k}"] for k in range(len(labs))]), want)
        # ... and the members are the restatement's (test_oblique_resample's bounds)
        ref = K.R.resample(img, gin, gout, default=RS.DEFAULT, **kw)
        assert 0.02 < (~ref["inside"]).mean() < 0.98
        edge_band = K.near_boundary(ref["c"], gin.size, 1e-9, ties=False)
        tie_band = K.near_boundary(ref["c"], gin.size, 1e-9, ties=True)
        K.check_linear("memory-state resample_set", outs["image"], ref, K.tol_fp64(ref["M"]), keep=~edge_band, default=RS.DEFAULT)
        for k, lab in enumerate(labs):
            w = K.R.resample(lab, gin, gout, interp="nearest", default=0.0, u8=True, **kw)["out"]
            np.testing.assert_array_equal(outs[f"label{k}"][~tie_band], w[~tie_band])

    case(f"resample-set-{name}", "pp_resample_set", np.prod(gout.shape), check, family="resample", scratch=False)(run)


_resample_set("oblique_both")
_resample_set("affine")


# ======================================================================================
# demons (tests/test_kernels.py: GRIDS[0], ODD, MIXED[0]; test_demons_force_single_sweep, test_demons_execute,
# test_demons_early_halt, test_demons_edge_cases)


def _demons_grids():
    Kt = T("kernels")
    return {"grid0": Kt.GRIDS[0], "odd": Kt.ODD, "mixed0": Kt.MIXED[0]}


@functools.lru_cache(maxsize=None)
def _force_inputs(gname):
    Kt = T("kernels")
    shape, spacing, origin = _demons_grids()[gname]
    from tests.helpers import phantom, smooth_noise
    fix = phantom(shape, seed=30)
    warped = (phantom(shape, seed=30, noise=0) + 40.0 * smooth_noise(shape, 31).astype(np.float32)).copy()
    warped[:, :, :3] = FLT_MAX          # crunched border
    warped[4:6, 5:9, 10:14] = FLT_MAX   # interior hole: voxels that are not live, their update is 0
    warped[2, 3, 20] = fix[2, 3, 20]    # |speed| below the intensity threshold
    want, wst = Kt.O.esm_update(Kt.O.Vol(fix, spacing, origin), Kt.O.Vol(warped, spacing, origin))
    return fix, warped, want, wst


def _demons_force(gname, variant):
    Kt = T("kernels")
    shape, spacing, origin = _demons_grids()[gname]

    def call(leg, fixed, warped, upd, st):
        p = Kt._demons_params(leg.ctx, 1, spacing, variant)
        return leg.lib.pp_demons_force_f32(leg.ctx.h, _lib.ptr(fixed), _lib.ptr(warped), C.byref(Kt.geom_of(shape, spacing, origin)), C.byref(p),
                                           _lib.ptr(upd), C.byref(st))

    def run(leg):
        fix, warped, _, _ = _force_inputs(gname)
        upd, st = leg.empty((3,) + shape), leg.hstruct(_lib.DemonsStats)
        assert call(leg, leg.dev(fix), leg.dev(warped), upd, st) == 0
        # a single sweep defines metric, rms_change, the two sums and the pixel count; elapsed_iterations / halted belong to Execute
        return {"update": leg.host(upd), **fields(st, skip=("elapsed_iterations", "halted"))}

    def check(leg, outs):       # test_demons_force_single_sweep
        _, _, want, wst = _force_inputs(gname)
        np.testing.assert_allclose(outs["update"], want, rtol=2e-5, atol=2e-6)
        assert outs["n_pixels"] == wst.n_pixels
        np.testing.assert_allclose(outs["metric"], wst.metric, rtol=1e-6)
        np.testing.assert_allclose(outs["rms_change"], wst.rms_change, rtol=1e-5)
        assert (outs["update"][:, 4:6, 5:9, 10:14] == 0).all()

    def bad(leg):
        fix, warped, _, _ = _force_inputs(gname)
        return call(leg, None, leg.dev(warped), leg.empty((3,) + shape), leg.hstruct(_lib.DemonsStats))

    case(f"demons-force-{gname}-{'staged' if variant == _lib.DEMONS_STAGED else 'fused'}", "pp_demons_force_f32", 3 * np.prod(shape), check,
         family="demons", bad=bad)(run)


@functools.lru_cache(maxsize=None)
def _execute_inputs(gname, mode):
    """(fixed, moving, iterations, max_rms, oracle field, oracle stats)."""
    Kt = T("kernels")
    O = Kt.O
    from tests.helpers import phantom, random_dvf, smooth_noise
    shape, spacing, origin = _demons_grids()[gname]
    if mode == "halt":          # the threshold of test_demons_early_halt: between the oracle's second and third RMS change
        fix = phantom(shape, seed=50, noise=0)
        mov = fix + np.float32(0.5) * smooth_noise(shape, 51).astype(np.float32)
        rms = [Kt._oracle_execute(fix, mov, spacing, origin, n, 0.0)[1].rms_change for n in (2, 3)]
        thr = 0.5 * (rms[0] + rms[1])
        want, wst = Kt._oracle_execute(fix, mov, spacing, origin, 8, thr)
        assert 1 < wst.elapsed_iterations < 8
        return fix, mov, 8, thr, want, wst
    fix = phantom(shape, seed=40)
    dv = random_dvf(shape, spacing, seed=41, max_mm=2.5)
    mov = O.warp_image(O.Vol(fix, spacing, origin), dv.astype(np.float64), edge_value=-1000.0).arr
    mov = (mov + np.random.default_rng(42).normal(0, 5, size=shape)).astype(np.float32)
    iters = {"zero": 0, "3": 3, "4": 4}[mode]
    want, wst = Kt._oracle_execute(fix, mov, spacing, origin, iters, 0.0) if iters else (np.zeros((3,) + shape), None)
    return fix, mov, iters, 0.0, want, wst


def _demons_execute(gname, variant, mode):
    Kt = T("kernels")
    shape, spacing, origin = _demons_grids()[gname]

    def call(leg, fixed, moving, fld, st):
        _, _, iters, thr, _, _ = _execute_inputs(gname, mode)
        p = Kt._demons_params(leg.ctx, iters, spacing, variant, max_rms=thr)
        return leg.lib.pp_demons_execute_f32(leg.ctx.h, _lib.ptr(fixed), _lib.ptr(moving), C.byref(Kt.geom_of(shape, spacing, origin)), C.byref(p),
                                             _lib.ptr(fld), C.byref(st))

    def run(leg):
        fix, mov = _execute_inputs(gname, mode)[:2]
        # (PP_DEMONS_FUSED wants the field on 16 bytes, include/platipy_amd.h; the staged variant takes any)
        fld, st = leg.empty((3,) + shape, align=16 if variant == _lib.DEMONS_FUSED else None), leg.hstruct(_lib.DemonsStats)
        assert call(leg, leg.dev(fix), leg.dev(mov), fld, st) == 0
        out = {"field": leg.host(fld), **fields(st)}
        metric, rms = leg.hempty(16), leg.hempty(16)         # pp_demons_history: what an iteration observer reads
        n = leg.lib.pp_demons_history(leg.ctx.h, hptr(metric), hptr(rms), 16)
        out.update(history_n=np.array(n), history_metric=metric[:n].copy(), history_rms=rms[:n].copy())
        return out

    def check(leg, outs):
        _, _, iters, thr, want, wst = _execute_inputs(gname, mode)
        if mode == "zero":      # test_demons_edge_cases: the field is zero and nothing was counted
            assert outs["elapsed_iterations"] == 0 and not outs["field"].any() and outs["history_n"] == 0
            return
        assert outs["elapsed_iterations"] == wst.elapsed_iterations == outs["history_n"]
        if mode == "halt":      # test_demons_early_halt
            assert outs["halted"] == 1
            np.testing.assert_allclose(outs["field"], want, rtol=0, atol=1e-3)
            return
        # test_demons_execute: its bounds are stated for 4 iterations of this phantom; 3 iterations accumulate no more
        err = np.abs(outs["field"] - want)
        assert err.max() <= 2e-3 and np.sqrt((err ** 2).mean()) <= 5e-5, (err.max(), np.sqrt((err ** 2).mean()))
        np.testing.assert_allclose(outs["metric"], wst.metric, rtol=1e-4)
        np.testing.assert_allclose(outs["rms_change"], wst.rms_change, rtol=1e-4)
        assert outs["history_metric"][-1] == outs["metric"] and outs["history_rms"][-1] == outs["rms_change"]
        assert np.abs(want).max() > 0.2

    def bad(leg):
        fix = _execute_inputs(gname, mode)[0]
        return call(leg, leg.dev(fix), None, leg.empty((3,) + shape), leg.hstruct(_lib.DemonsStats))

    vname = "staged" if variant == _lib.DEMONS_STAGED else "fused"
    case(f"demons-execute-{gname}-{vname}-{mode}", ("pp_demons_execute_f32", "pp_demons_history"), 3 * np.prod(shape), check, family="demons",
         bad=bad)(run)


for _g in ("grid0", "odd", "mixed0"):
    for _v in (_lib.DEMONS_STAGED, _lib.DEMONS_FUSED):
        _demons_force(_g, _v)
        for _m in ("3", "4"):
            _demons_execute(_g, _v, _m)
for _v in (_lib.DEMONS_STAGED, _lib.DEMONS_FUSED):
    _demons_execute("grid0", _v, "halt")
    _demons_execute("odd", _v, "zero")


# ======================================================================================
# label fusion arithmetic (tests/test_fusion_kernels.py: n = 1027 -- a block of quads, then a three-voxel tail -- and the
# volumes of VOLUMES)

N_FLAT = 1027


def _fusion_flat():
    F = T("fusion_kernels")
    R = F.R

    def check_divide(leg, outs):        # test_fuse_divide
        F.assert_same_bits(outs["out"], R.divide(*F.divide_inputs(N_FLAT)), "divide")

    @case("fuse-divide", "pp_fuse_divide_f32", N_FLAT, check_divide, family="fusion", scratch=False)
    def run_divide(leg):
        wl, ws = F.divide_inputs(N_FLAT)
        out = leg.empty(N_FLAT)
        leg.ctx.fuse_divide(leg.dev(wl), leg.dev(ws), out, N_FLAT)
        return {"out": leg.host(out)}

    mx = float(np.float32(0.9))

    def check_threshold(leg, outs):     # test_binary_threshold
        F.assert_same_bits(outs["out"], R.binary_threshold(F.threshold_inputs(N_FLAT), mx, 0.5), "binary_threshold")

    @case("binary-threshold", "pp_binary_threshold_f32", N_FLAT, check_threshold, family="fusion", scratch=False)
    def run_threshold(leg):
        out = leg.empty(N_FLAT, np.uint8)
        leg.ctx.binary_threshold(leg.dev(F.threshold_inputs(N_FLAT)), N_FLAT, mx, 0.5, out)
        return {"out": leg.host(out)}

    for kind, fn in (("u8_full", "pp_fuse_accumulate_u8"), ("f32", "pp_fuse_accumulate_f32")):
        def check_acc(leg, outs, kind=kind):        # test_fuse_accumulate
            ws, labs = F.accumulate_inputs(N_FLAT, kind)
            want_wsum, plain, fused = F.accumulate_reference(ws, labs, True)
            F.assert_one_of(outs["wlsum"], plain, fused, ("wlsum", kind))
            F.assert_same_bits(outs["wsum"], want_wsum, ("wsum", kind))

        def run_acc(leg, kind=kind):
            ws, labs = F.accumulate_inputs(N_FLAT, kind)
            # in/out accumulators: they start from the defined value 0 on every leg, as their contract says
            wsum, wlsum = leg.dev(np.zeros(N_FLAT, np.float32)), leg.dev(np.zeros(N_FLAT, np.float32))
            for w, lab in zip(ws, labs):
                leg.ctx.fuse_accumulate(leg.dev(w), leg.dev(lab), wsum, wlsum, N_FLAT)
            return {"wsum": leg.host(wsum), "wlsum": leg.host(wlsum)}

        case(f"fuse-accumulate-{kind}", fn, N_FLAT, check_acc, family="fusion", scratch=False, accumulates=("wsum", "wlsum"))(run_acc)

    def check_rescale(leg, outs):       # test_rescale_threshold
        x, lo, hi, lower = F.rescale_inputs(N_FLAT)
        F.assert_one_of(outs["data"], *R.rescale_threshold(x, lo, hi, lower), "rescale")

    @case("rescale-threshold", "pp_rescale_threshold_f32", N_FLAT, check_rescale, family="fusion", scratch=False)
    def run_rescale(leg):
        x, lo, hi, lower = F.rescale_inputs(N_FLAT)
        d = leg.dev(x)
        leg.ctx.rescale_threshold(d, N_FLAT, lo, hi, lower)
        return {"data": leg.host(d)}

    def _ab(n):
        r = F.rng_for(n, 11)
        return (100.0 * r.standard_normal(n)).astype(np.float32), (100.0 * r.standard_normal(n)).astype(np.float32)

    for n in (N_FLAT, 70001):           # one block row; 274 blocks: a second row of k_sum_final
        def check_ssd(leg, outs, n=n):  # test_sum_sq_diff
            a, b = _ab(n)
            want = R.ssd(a, b)
            assert abs(outs["ssd"] - want) / want <= F.ssd_bound(n)

        def run_ssd(leg, n=n):
            a, b = _ab(n)
            r = leg.hempty(1)
            assert leg.lib.pp_sum_sq_diff_f32(leg.ctx.h, leg.p(a), leg.p(b), n, hptr(r)) == 0
            return {"ssd": r}

        case(f"sum-sq-diff-{n}", "pp_sum_sq_diff_f32", n, check_ssd, family="reduce")(run_ssd)

        def check_minmax(leg, outs, n=n):       # test_minmax_planted_extrema
            base = F.rng_for(n, 13).uniform(-1.0, 1.0, n).astype(np.float32)
            F.minmax_equal((outs["min"][0], outs["max"][0]), R.minmax(base))

        def run_minmax(leg, n=n):
            base = F.rng_for(n, 13).uniform(-1.0, 1.0, n).astype(np.float32)
            lo, hi = leg.hempty(1, np.float32), leg.hempty(1, np.float32)
            assert leg.lib.pp_minmax_f32(leg.ctx.h, leg.p(base), n, hptr(lo, C.c_float), hptr(hi, C.c_float)) == 0
            return {"min": lo, "max": hi}

        case(f"minmax-{n}", "pp_minmax_f32", n, check_minmax, family="reduce")(run_minmax)


_fusion_flat()


def _weight_maps(shape):
    F = T("fusion_kernels")
    R = F.R
    spacing = F.VOLUMES[shape]
    sigma, eps = 2.0, 1e-5

    def check_local(leg, outs):         # test_weight_map_local
        t, m = F.volume_pair(shape)
        want, bound = _local_bound(leg)
        assert (np.abs(outs["weight"].astype(np.float64) - want) <= bound).all()

    def _local_bound(leg):
        t, m = F.volume_pair(shape)
        raw, b_fir = F.local_reference(leg.lib, shape, sigma)
        want = 1.0 / (raw + np.float64(np.float32(eps)))
        return want, b_fir / (raw + np.float64(np.float32(eps))) ** 2 + 3 * F.U24 * want

    @case(f"weight-map-local-{'x'.join(map(str, shape))}", "pp_weight_map_local_f32", np.prod(shape), check_local, family="fusion")
    def run_local(leg):
        t, m = F.volume_pair(shape)
        w = leg.empty(shape)
        leg.ctx.weight_map_local(leg.dev(t), leg.dev(m), size_of(shape), spacing, sigma, eps, w)
        return {"weight": leg.host(w)}

    radius, factor, gain = (2, 1, 0), 1e4, 2

    def check_block(leg, outs):         # test_weight_map_block
        from scipy.ndimage import maximum_filter

        t, m = F.volume_pair(shape)
        sq = R.squared_difference(t, m).astype(np.float64)
        box_max = maximum_filter(sq, size=tuple(2 * radius[2 - k] + 1 for k in range(3)), mode="nearest")
        b_box = F.U24 * box_max * sum(2 * r + 3 for r in radius)
        got = outs["weight"].astype(np.float64)
        want, mean = R.block_weight(t, m, size_of(shape), radius, factor, gain)
        zero = mean == 0.0
        assert np.array_equal(got[zero], want[zero])
        p = abs(gain / 2.0)
        low = F.power_of_inverse(mean + b_box, p, factor)
        high = F.power_of_inverse(np.maximum(mean - b_box, 0.0), p, factor)
        ok = (got >= low - F.POWF_ULP * F.ulp32(low)) & (got <= high + F.POWF_ULP * F.ulp32(high))
        assert ok.all() and not np.isnan(got).any()

    @case(f"weight-map-block-{'x'.join(map(str, shape))}", "pp_weight_map_block_f32", np.prod(shape), check_block, family="fusion")
    def run_block(leg):
        t, m = F.volume_pair(shape)
        w = leg.empty(shape)
        leg.ctx.weight_map_block(leg.dev(t), leg.dev(m), size_of(shape), radius, factor, gain, w)
        return {"weight": leg.host(w)}


_weight_maps((9, 14, 23))
_weight_maps((6, 10, 70))


# ======================================================================================
# mask family (shapes of tests/test_bronchus.py; references of tests/test_mask_kernels.py, tests/test_bronchus.py,
# tests/comparison_restatement.py, tests/external_mask_restatement.py).  Integer results: exact.

MASK_SHAPES = [(5, 9, 37), (3, 4, 1040), (1, 7, 19), (6, 5, 1)]


def _sid(shape):
    return "x".join(map(str, shape))


def _mask(shape, density=0.5, salt=0):
    from tests.helpers import bernoulli
    return bernoulli(shape, density, seed=11 + shape[2] + salt)


def _mask_family(shape):
    MK, BR = T("mask_kernels"), T("bronchus")
    from tests import comparison_restatement as CR
    from tests import external_mask_restatement as XR
    n, sid, size = int(np.prod(shape)), _sid(shape), size_of(shape)
    m = _mask(shape)
    kw = dict(family="mask")

    def dev_out(fn_name, *args, dtype=np.uint8, **kws):
        """run(leg) of an operation whose only output is one volume `out` (the last argument of the Context method)."""
        def run(leg):
            out = leg.empty(shape, dtype)
            getattr(leg.ctx, fn_name)(*[leg.dev(a) if isinstance(a, np.ndarray) else a for a in args], out, **kws)
            return {"out": leg.host(out)}
        return run

    def exact(want):
        def check(leg, outs):
            np.testing.assert_array_equal(outs["out"], want() if callable(want) else want)
        return check

    # fillhole / largest component: both settings, with the host count (test_mask_kernels.check_cc)
    def run_cc(leg):
        out = {}
        for fill in (True, False):
            o, cnt = leg.empty(shape, np.uint8), leg.hempty(1, np.int64)
            assert leg.lib.pp_fillhole_largest_component_u8(leg.ctx.h, leg.p(m), _lib._i3(size), int(fill), _lib.ptr(o),
                                                            hptr(cnt, C.c_int64)) == 0
            out[f"out-fill{int(fill)}"], out[f"count-fill{int(fill)}"] = leg.host(o), cnt
        return out

    def check_cc(leg, outs):
        for fill in (True, False):
            want, count = MK.cc_reference(m, fill)
            np.testing.assert_array_equal(outs[f"out-fill{int(fill)}"], want)
            assert outs[f"count-fill{int(fill)}"][0] == count

    case(f"fillhole-largest-{sid}", "pp_fillhole_largest_component_u8", n, check_cc, **kw)(run_cc)

    def run_cc_conn(leg):       # 26-connectivity: largest component alone, hole filling alone (tests/test_external_mask.py)
        out = {}
        for name, fill, keep in (("largest26", 0, 1), ("fill26", 1, 0)):
            o, cnt = leg.empty(shape, np.uint8), leg.hempty(1, np.int64)
            assert leg.lib.pp_fillhole_largest_component_conn_u8(leg.ctx.h, leg.p(m), _lib._i3(size), fill, keep, 1, _lib.ptr(o),
                                                                 hptr(cnt, C.c_int64) if keep else None) == 0
            out[name] = leg.host(o)
            if keep:
                out[name + "-count"] = cnt
        return out

    def check_cc_conn(leg, outs):
        want = XR.largest_component(m, True)
        np.testing.assert_array_equal(outs["largest26"], want)
        assert outs["largest26-count"][0] == int(want.sum())
        np.testing.assert_array_equal(outs["fill26"], XR.fill_holes(m, True))

    case(f"fillhole-largest-conn-{sid}", "pp_fillhole_largest_component_conn_u8", n, check_cc_conn, **kw)(run_cc_conn)

    # morphology: the three operations (test_mask_kernels.check_morph: the oracle's scipy restatement)
    radius = (2, 1, 1)

    def run_morph(leg):
        return {f"op{op}": MK.run_morph(leg, m, radius, op) for op in (MK.DILATE, MK.ERODE, MK.CLOSE)}

    def check_morph(leg, outs):
        vol = MK.O.Vol(m, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
        for op in (MK.DILATE, MK.ERODE, MK.CLOSE):
            np.testing.assert_array_equal(outs[f"op{op}"], MK.MORPH_REF[op](vol, radius).arr)

    case(f"morph-ball-{sid}", "pp_binary_morph_ball_u8", n, check_morph, **kw)(run_morph)

    # distance map: unsigned, signed, inside-positive (test_mask_kernels.check_distance)
    spacing = (0.9, 1.1, 2.5)
    dm = _mask(shape, 0.7, 1)

    def run_dist(leg):
        g = _lib.make_geom(size, spacing, (3.0, -7.0, 11.0))
        out = {}
        for signed, pos in ((False, False), (True, False), (True, True)):
            o = leg.empty(shape)
            leg.ctx.distance_map(leg.dev(dm), g, o, signed=signed, inside_positive=pos)
            out[f"signed{int(signed)}-pos{int(pos)}"] = leg.host(o)
        return out

    def check_dist(leg, outs):
        d, border = MK.distance_reference(dm, spacing)
        obj = dm != 0
        for signed, pos in ((False, False), (True, False), (True, True)):
            want = d if not signed else np.where(obj != pos, -d, d)
            got = outs[f"signed{int(signed)}-pos{int(pos)}"]
            np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-5)
            assert (got[border] == 0.0).all()
            np.testing.assert_array_equal(np.sign(got), np.sign(want))

    case(f"distance-map-{sid}", "pp_distance_map_f32", n, check_dist, **kw)(run_dist)

    # contours: face rule, 26-neighbourhood rule, per-slice rule (test_mask_kernels.test_label_contour, tests/test_comparison.py)
    case(f"label-contour-{sid}", "pp_label_contour_u8", n, exact(lambda: MK.contour_reference(m)), scratch=False, **kw)(
        dev_out("label_contour", m, size))

    def run_bc(leg):
        out = {}
        for full in (True, False):
            o = leg.empty(shape, np.uint8)
            leg.ctx.binary_contour(leg.dev(m), size, o, fully_connected=full)
            out[f"full{int(full)}"] = leg.host(o)
        return out

    def check_bc(leg, outs):
        np.testing.assert_array_equal(outs["full1"], CR.border26(m).astype(np.uint8))
        np.testing.assert_array_equal(outs["full0"], CR.contour6(m).astype(np.uint8))

    case(f"binary-contour-{sid}", "pp_binary_contour_u8", n, check_bc, scratch=False, **kw)(run_bc)
    case(f"slice-contour-{sid}", "pp_slice_contour_u8", n, exact(lambda: CR.contour4_slices(m).astype(np.uint8)), scratch=False, **kw)(
        dev_out("slice_contour", m, size))

    # connected components, both entry points, with the host count (tests/test_bronchus.py::test_labels_equal_scipy)
    def run_labels(leg):
        out = {}
        for name, call in (("face", lambda lab, cnt: leg.lib.pp_connected_components_u8(leg.ctx.h, leg.p(m), _lib._i3(size), _lib.ptr(lab), hptr(cnt, C.c_int))),
                           ("full", lambda lab, cnt: leg.lib.pp_connected_components_conn_u8(leg.ctx.h, leg.p(m), _lib._i3(size), 1, _lib.ptr(lab), hptr(cnt, C.c_int)))):
            lab, cnt = leg.empty(shape, np.int32), leg.hempty(1, np.int32)
            assert call(lab, cnt) == 0
            out[name], out[name + "-count"] = leg.host(lab), cnt
        return out

    def check_labels(leg, outs):
        want, nlab = BR.R.label(m)
        assert outs["face-count"][0] == nlab and np.array_equal(outs["face"], want)
        want, nlab = XR.label(m, True)
        assert outs["full-count"][0] == nlab and np.array_equal(outs["full"], want)

    case(f"connected-components-{sid}", ("pp_connected_components_u8", "pp_connected_components_conn_u8"), n, check_labels, **kw)(run_labels)

    # label moments (test_moments_equal_integer_sums): more labels asked for than present -> zero rows
    lab, nlab = BR.R.label(_mask(shape, 0.45, 3))

    def run_moments(leg):
        out = leg.empty((nlab + 7, 10), np.int64)
        leg.ctx.label_moments(leg.dev(lab), size, nlab + 7, out)
        return {"out": leg.host(out)}

    case(f"label-moments-{sid}", "pp_label_moments_i32", n, exact(lambda: BR.R.moments(lab, nlab + 7)), scratch=False, **kw)(run_moments)

    # connected threshold (test_region_growing_equals_scipy)
    img = np.random.default_rng(21 + shape[2]).integers(0, 5, size=shape).astype(np.float32)
    seeds = [BR.first_voxel_with(img, 1.0), BR.first_voxel_with(img, 3.0)]

    def run_grow(leg):
        out, vox = leg.empty(shape, np.uint8), leg.hempty(1, np.int64)
        s = np.ascontiguousarray(seeds, dtype=np.int32)
        assert leg.lib.pp_connected_threshold_f32(leg.ctx.h, leg.p(img), _lib._i3(size), 1.0, 3.0, hptr(s, C.c_int), len(seeds),
                                                  _lib.ptr(out), hptr(vox, C.c_int64)) == 0
        return {"out": leg.host(out), "voxels": vox}

    def check_grow(leg, outs):
        want = BR.R.connected_threshold(img, seeds, 1.0, 3.0)
        assert np.array_equal(outs["out"], want) and outs["voxels"][0] == int(want.sum())

    case(f"connected-threshold-{sid}", "pp_connected_threshold_f32", n, check_grow, **kw)(run_grow)

    # binary median (test_median_equals_scipy)
    mr = (2, 1, 0)
    case(f"binary-median-{sid}", "pp_binary_median_u8", n, exact(lambda: BR.R.median(m, mr)), scratch=False, **kw)(
        dev_out("binary_median", m * 200, size, mr))

    # per-slice convex hull (tests/test_external_mask.py; tests/external_mask_restatement.py)
    hm = _mask(shape, 0.08, 5)
    case(f"slice-convex-hull-{sid}", "pp_slice_convex_hull_u8", n, exact(lambda: XR.slice_convex_hull(hm)[0]), **kw)(
        dev_out("slice_convex_hull", hm, size))

    # bounding box, uint8 and float (test_mask_kernels.box_reference)
    bm = np.zeros(shape, np.uint8)
    bm[shape[0] // 2:, shape[1] // 3:, shape[2] // 4:max(shape[2] - 2, shape[2] // 4 + 1)] = m[shape[0] // 2:, shape[1] // 3:, shape[2] // 4:max(shape[2] - 2, shape[2] // 4 + 1)]

    def run_box(leg):
        out = {}
        for name, vol, dt in (("u8", bm, 0), ("f32", bm.astype(np.float32) * 0.25, 1)):
            box = leg.hempty(6, np.int32)
            assert leg.lib.pp_bounding_box(leg.ctx.h, leg.p(vol), dt, _lib._i3(size), hptr(box, C.c_int)) == 0
            out[name] = box
        return out

    def check_box(leg, outs):
        want = MK.box_reference(bm)
        assert list(outs["u8"]) == list(want) and list(outs["f32"]) == list(want), (outs, want)

    case(f"bounding-box-{sid}", "pp_bounding_box", n, check_box, **kw)(run_box)


for _shape in MASK_SHAPES:
    _mask_family(_shape)


def _mask_family_2(shape):
    """Slice moments, tube mask, polar sectors, resample_bits, contour fill / trace on the same shapes."""
    from tests import cardiac_geometry_restatement as G
    from tests import contour_restatement as CF
    from tests import contour_trace_restatement as CT
    from tests import resample_restatement as RR
    from tests import ventricle_restatement as V
    CG, VT, CO = T("cardiac_geometry"), T("ventricle"), T("contours")
    n, sid, size = int(np.prod(shape)), _sid(shape), size_of(shape)
    nz, ny, nx = shape
    kw = dict(family="mask")
    rng = np.random.default_rng(500 + nx)

    # slice moments, both scan axes, three masks of values 1 / 255 / random (tests/test_cardiac_geometry.py::test_slice_moments)
    masks = [_mask(shape, 0.4, 7), (_mask(shape, 0.3, 8) * 255).astype(np.uint8), rng.integers(0, 256, shape).astype(np.uint8)]

    def run_sm(leg):
        out = {}
        for scan, axis in (("z", 2), ("x", 0)):
            o = leg.empty((len(masks), size[axis], 4), np.int64)
            leg.ctx.slice_moments([leg.dev(x) for x in masks], size, axis, o)
            out[scan] = leg.host(o)
        return out

    def check_sm(leg, outs):
        for scan in ("z", "x"):
            np.testing.assert_array_equal(outs[scan], G.slice_moments(masks, scan))

    case(f"slice-moments-{sid}", "pp_slice_moments_u8", n, check_sm, scratch=False, **kw)(run_sm)

    # tube mask (test_tube_mask_odd_volumes: a polyline through the volume, radius 1.7)
    spacing, origin = CG.SPACING, CG.ORIGIN
    line = [CG.p(0.6, 0.7, 0.2), CG.p(nx * 0.55, ny * 0.35, nz * 0.6), CG.p(nx - 1.3, ny - 1.6, nz - 1.2)]

    def run_tube(leg):
        out = leg.empty(shape, np.uint8)
        leg.ctx.tube_mask(np.asarray(line, dtype=np.float64), size, spacing, origin, 1.7, out)
        return {"out": leg.host(out)}

    def check_tube(leg, outs):
        dist = G.tube_distance(line, shape, spacing, origin)
        assert not np.any(np.abs(dist - 1.7) <= 1e-6)
        want = (dist <= 1.7).astype(np.uint8)
        assert want.sum() >= 1 and np.array_equal(outs["out"], want)

    case(f"tube-mask-{sid}", "pp_tube_mask_u8", n, check_tube, **kw)(run_tube)

    # polar sectors (tests/test_ventricle.py::check_polar: the slice table with a skipped slice, the area test at min_area)
    pm = _mask(shape, 0.6, 9)
    slices, area = VT.slice_table(shape), 0.5

    @functools.lru_cache(maxsize=None)
    def polar_want():
        _, plain = V.polar_sectors(pm, slices, VT.RULES, area, 0.0)
        min_area = VT.equality_threshold(plain, area)
        if min_area is None:
            min_area = float(np.median(plain[plain > 0])) * area if (plain > 0).any() else 1.0
        gaps = {}
        bits, counts = V.polar_sectors(pm, slices, VT.RULES, area, min_area, gaps)
        assert gaps["angle"] > 1e-9 and gaps["radius"] > 1e-9
        return bits, counts, min_area

    def run_polar(leg):
        bits, counts = leg.empty(shape, np.uint32), leg.empty((nz, 32), np.int64)
        leg.ctx.polar_sectors(leg.dev(pm), size, slices, VT.RULES, area, polar_want()[2], bits, counts)
        return {"bits": leg.host(bits).view(np.uint32), "counts": leg.host(counts)}

    def check_polar(leg, outs):
        bits, counts, _ = polar_want()
        assert np.array_equal(outs["counts"], counts) and np.array_equal(outs["bits"], bits)

    case(f"polar-sectors-{sid}", "pp_polar_sectors_u8", n, check_polar, **kw)(run_polar)

    # resample_bits (tests/test_ventricle.py::test_resample_bits, the partly-outside rigid map)
    vol = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    sp2, org2, nbits = (1.25, 1.1, 1.8), (-7.5, 4.0, 30.0), 17
    centre = np.asarray(org2) + np.asarray(sp2) * (np.asarray(size) - 1) / 2.0
    A, t = VT.rigid((1, 2, 3), 0.4, centre, tuple(0.3137 * s * v for s, v in zip(sp2, size)))

    def run_bits(leg):
        out = leg.empty((nbits,) + shape, np.uint8)
        g = _lib.make_geom(size, sp2, org2)
        leg.ctx.resample_bits(leg.dev(vol.view(np.int32)), g, g, nbits, out, affine_A=A.ravel(), affine_t=t)
        return {"out": leg.host(out)}

    def check_bits(leg, outs):
        g = RR.Grid(size, sp2, org2)
        inside = False
        for k in range(nbits):
            plane = ((vol >> np.uint32(k)) & np.uint32(1)).astype(np.uint8)
            want = RR.resample(plane, g, g, A, t, interp="nearest", default=0, u8=True)
            frac = want["c"][want["inside"]]
            assert frac.size == 0 or np.abs(frac - np.floor(frac) - 0.5).min() > 1e-9
            inside |= bool(want["inside"].any())
            assert not want["inside"].all()                  # the default-value path writes
            assert np.array_equal(outs["out"][k], want["out"]), k
        assert inside

    case(f"resample-bits-{sid}", "pp_resample_bits_u32", n, check_bits, scratch=False, **kw)(run_bits)

    # contour fill (tests/test_contours.py::test_random_polygons): 3 structures, polygons over every border
    polys = [(k % 3, z, pts) for k, (_, z, pts) in enumerate(CO.random_polygons(ny, nx, nz, 24, seed=1000 * ny + nx + nz))]
    verts, rows = CO.tables(polys)

    def run_fill(leg):
        out = leg.empty((3, nz, ny, nx), np.uint8)
        leg.ctx.contour_fill(verts, rows, size, 3, out)
        return {"out": leg.host(out)}

    def check_fill(leg, outs):
        want = CF.fill(verts, rows, size, 3)
        assert np.array_equal(outs["out"], want) and int(want.sum()) >= 1

    case(f"contour-fill-{sid}", "pp_contour_fill_u8", n, check_fill, **kw)(run_fill)

    # contour trace: the count call and the fill call, full and approximate (tests/test_contour_trace.py::test_equals_restatement)
    tm = np.stack([_mask(shape, d, 20 + k) * (255 if k else 1) for k, d in enumerate((0.3, 0.7))]).astype(np.uint8)

    def run_trace(leg):
        out = {}
        for approx in (0, 1):
            dm = leg.dev(tm)
            counts = leg.hempty(3, np.int64)
            assert leg.lib.pp_contour_trace_u8(leg.ctx.h, _lib.ptr(dm), _lib._i3(size), 2, approx, None, 0, None, None, 0, hptr(counts, C.c_int64)) == 0
            out[f"counts-{approx}"] = counts.copy()
            nv, nc = int(counts[1]), int(counts[2])
            v, r, h = leg.hempty((nv, 2), np.int32), leg.hempty(nc, _lib.CONTOUR_DTYPE), leg.hempty(nc, np.uint8)
            counts2 = leg.hempty(3, np.int64)
            assert leg.lib.pp_contour_trace_u8(leg.ctx.h, _lib.ptr(dm), _lib._i3(size), 2, approx, v.ctypes.data, nv, r.ctypes.data, h.ctypes.data, nc,
                                               hptr(counts2, C.c_int64)) == 0
            out.update({f"vertices-{approx}": v, f"rows-{approx}": r.view(np.int32), f"hole-{approx}": h, f"counts2-{approx}": counts2})
        return out

    def check_trace(leg, outs):
        for approx in (0, 1):
            wv, wr, wh = CT.trace(tm, bool(approx))
            assert [tuple(x) for x in outs[f"rows-{approx}"].reshape(-1, 4).tolist()] == wr
            assert np.array_equal(outs[f"vertices-{approx}"], wv) and np.array_equal(outs[f"hole-{approx}"], wh)
            assert list(outs[f"counts-{approx}"][1:]) == [len(wv), len(wr)] and np.array_equal(outs[f"counts-{approx}"], outs[f"counts2-{approx}"])

    case(f"contour-trace-{sid}", "pp_contour_trace_u8", n, check_trace, **kw)(run_trace)


for _shape in MASK_SHAPES:
    _mask_family_2(_shape)


# ======================================================================================
# reductions: label comparison, dose, patch correlation, joint histogram, STAPLE


def _compare():
    from tests import comparison_restatement as CR
    RE = T("reduction_edges")
    kw = dict(family="reduce")

    for n in (1027, 70001):
        rng = np.random.default_rng(n)
        a, b = (rng.random(n) < 0.4).astype(np.uint8) * 255, (rng.random(n) < 0.6).astype(np.uint8)

        def run_ov(leg, a=a, b=b, n=n):
            c = leg.hempty(3, np.int64)
            assert leg.lib.pp_overlap_counts_u8(leg.ctx.h, leg.p(a), leg.p(b), n, hptr(c, C.c_int64)) == 0
            return {"counts": c}

        def check_ov(leg, outs, a=a, b=b):      # tests/test_comparison.py::test_integer_metrics_against_restatement: exact counts
            assert list(outs["counts"]) == [int((a != 0).sum()), int((b != 0).sum()), int(((a != 0) & (b != 0)).sum())]

        case(f"overlap-counts-{n}", "pp_overlap_counts_u8", n, check_ov, **kw)(run_ov)

    for n in (257, 65537):
        x = next(iter(RE._planted(n, seed=n)))[0]

        def run_ar(leg, x=x, n=n):
            r = leg.empty((2,), np.float32)
            leg.ctx.abs_range(leg.dev(x), n, r)
            return {"range": leg.host(r)}

        def check_ar(leg, outs, x=x):           # test_abs_range_sizes
            assert tuple(outs["range"]) == (np.abs(x).min(), np.abs(x).max())

        case(f"abs-range-{n}", "pp_abs_range_f32", n, check_ar, **kw)(run_ar)

    for shape in ((5, 9, 37), (3, 4, 1040)):
        n, size = int(np.prod(shape)), size_of(shape)
        rng = np.random.default_rng(41 + shape[2])
        dist = rng.normal(scale=4.0, size=shape).astype(np.float32)
        sel = (_mask(shape, 0.6, 30) * rng.integers(1, 4, shape)).astype(np.uint8)
        tau = 1.25

        def samples(mode, sel=sel, dist=dist):
            if mode == _lib.SURFACE_CONTOUR_ABS:
                return np.abs(dist[CR.contour6(sel)])
            if mode == _lib.SURFACE_LABEL_POS:
                return np.maximum(dist[sel != 0], np.float32(0))
            return dist[sel != 0]

        def run_ss(leg, shape=shape, size=size, n=n, sel=sel, dist=dist):
            geom = _lib.make_geom(size, (0.9, 1.1, 2.5))
            dsel, ddist = leg.dev(sel), leg.dev(dist)
            drange = leg.empty((2,), np.float32)
            leg.ctx.abs_range(ddist, n, drange)
            out = {}
            for mode in (0, 1, 2):
                for ranged in (True, False):
                    rec = leg.empty((_lib.SURFACE_STATS_DTYPE.itemsize,), np.uint8, align=8)
                    leg.ctx.surface_stats(dsel, ddist, geom, mode, rec, tau=tau, device_range=drange if ranged else None)
                    out[f"mode{mode}-range{int(ranged)}"] = leg.host(rec)
            return out

        def check_ss(leg, outs, dist=dist, samples=samples):     # tests/test_reduction_edges.py::test_surface_stats_257_blocks
            lo, hi = np.float64(np.abs(dist).min()), np.float64(np.abs(dist).max())
            for mode in (0, 1, 2):
                v = samples(mode)
                v64 = v.astype(np.float64)
                assert v.size > 20
                for ranged in (True, False):
                    rec = outs[f"mode{mode}-range{int(ranged)}"].view(_lib.SURFACE_STATS_DTYPE)[0]
                    assert rec["count"] == v.size and rec["count_le_tau"] == int((v64 <= tau).sum())
                    assert rec["min"] == v.min() and rec["max"] == v.max()
                    assert np.isclose(rec["sum"], v64.sum(), rtol=1e-12, atol=1e-12) and np.isclose(rec["sum_sq"], (v64 * v64).sum(), rtol=1e-12)
                    if ranged:
                        x = (v64 - lo) / (hi - lo) * 128.0
                        want = np.bincount(np.where(x >= 127, 127, np.maximum(x, 0).astype(np.int64)), minlength=128)
                        assert np.array_equal(rec["hist"], want) and (rec["range_lo"], rec["range_hi"]) == (np.float32(lo), np.float32(hi))
                    else:
                        assert (rec["range_lo"], rec["range_hi"]) == (0.0, 0.0)

        case(f"surface-stats-{_sid(shape)}", "pp_surface_stats_f32", n, check_ss, **kw)(run_ss)

        a, b = _mask(shape, 0.5, 31), _mask(shape, 0.5, 32) * 255

        def run_smc(leg, shape=shape, size=size, a=a, b=b):
            out = {}
            for name, nb in (("masked", b), ("plain", None)):
                o = leg.empty((shape[0],), np.int64, align=8)
                leg.ctx.slice_masked_count(leg.dev(a), None if nb is None else leg.dev(nb), size, o)
                out[name] = leg.host(o)
            return out

        def check_smc(leg, outs, a=a, b=b):     # tests/test_comparison.py (added path length): exact counts per slice
            assert np.array_equal(outs["masked"], ((a != 0) & (b == 0)).sum(axis=(1, 2)))
            assert np.array_equal(outs["plain"], (a != 0).sum(axis=(1, 2)))

        case(f"slice-masked-count-{_sid(shape)}", "pp_slice_masked_count_u8", n, check_smc, scratch=False, **kw)(run_smc)


_compare()


def _dose():
    import math

    D = T("dose")
    kw = dict(family="reduce")
    d, masks = D.dose_array(), D.mask_arrays()[:9]

    for edges in ("w0.1", "w0.001"):            # per-workgroup LDS tables; global integer atomics
        e = D.edge_set(edges)

        def run_h(leg, e=e):
            nb = e.size - 1
            hist, stats = leg.hempty((len(masks), nb), np.int64), leg.hempty(len(masks) * _lib.DOSE_STATS_DTYPE.itemsize, np.uint8)
            dev = [leg.dev(m) for m in masks]
            ptrs = (C.c_void_p * len(masks))(*[_lib.ptr(x) for x in dev])
            ee = np.ascontiguousarray(e, dtype=np.float64)
            assert leg.lib.pp_dose_histogram_f32(leg.ctx.h, leg.p(d), ptrs, len(masks), d.size, hptr(ee), nb, hptr(hist, C.c_int64), stats.ctypes.data) == 0
            st = stats.view(_lib.DOSE_STATS_DTYPE)
            return {"hist": hist, **{k: np.ascontiguousarray(st[k]) for k in st.dtype.names}}       # (field by field: the records have padding)

        def check_h(leg, outs, edges=edges):    # test_histogram_equals_numpy, test_histogram_statistics, test_histogram_dose_sum_is_exact
            assert np.array_equal(outs["hist"], D.expected_counts(edges)[:len(masks)])
            for k, m in enumerate(masks):
                inside = d[m != 0]
                assert outs["count"][k] == inside.size and outs["mask_sum"][k] == int(m.sum(dtype=np.int64))
                if inside.size:
                    assert outs["dose_min"][k] == inside.min() and outs["dose_max"][k] == inside.max()
                    assert outs["dose_sum"][k] == math.fsum(inside.astype(np.float64).tolist())
                else:
                    assert outs["dose_sum"][k] == 0.0 and outs["dose_min"][k] == np.inf and outs["dose_max"][k] == -np.inf

        case(f"dose-histogram-{edges}", "pp_dose_histogram_f32", d.size, check_h, **kw)(run_h)

    m0 = masks[0]
    nin = int(np.count_nonzero(m0))
    ranks = [0, 1, nin // 2, nin - 2, nin - 1]

    def run_os(leg):
        out = leg.hempty(len(ranks), np.float32)
        rk = np.asarray(ranks, np.int64)
        assert leg.lib.pp_masked_order_stats_f32(leg.ctx.h, leg.p(d), leg.p(m0), d.size, hptr(rk, C.c_int64), len(ranks), hptr(out, C.c_float)) == 0
        return {"out": out}

    def check_os(leg, outs):                    # test_order_statistics
        inside = d[m0 != 0]
        assert np.array_equal(D.bits(outs["out"]), D.bits(np.partition(inside, ranks)[ranks]))

    case("masked-order-stats", "pp_masked_order_stats_f32", d.size, check_os, **kw)(run_os)

    thresholds = [3.3, 0, 25.05, float(d.max()), float(d.max()) + 1.0, -5.0, 3.3, 64.0]

    def run_ge(leg):
        counts = leg.hempty((len(masks), len(thresholds)), np.int64)
        dev = [leg.dev(m) for m in masks]
        ptrs = (C.c_void_p * len(masks))(*[_lib.ptr(x) for x in dev])
        th = np.asarray(thresholds, np.float32)
        assert leg.lib.pp_masked_count_ge_f32(leg.ctx.h, leg.p(d), ptrs, len(masks), d.size, hptr(th, C.c_float), len(thresholds),
                                              hptr(counts, C.c_int64)) == 0
        return {"counts": counts}

    def check_ge(leg, outs):                    # test_count_ge
        want = np.array([[(d[m != 0] >= np.float32(t)).sum() for t in thresholds] for m in masks])
        assert np.array_equal(outs["counts"], want)

    case("masked-count-ge", "pp_masked_count_ge_f32", d.size, check_ge, **kw)(run_ge)


_dose()


def _patch_and_histograms():
    P = T("patch_correlation")
    kw = dict(family="reduce")
    t, m = P.kernel_pair()

    for window in ((3, 5, 4), (16, 5, 3), (17, 3, 3)):        # the two LDS tiles, and patches read from global memory
        def run_pc(leg, window=window):
            out = leg.empty(t.shape)
            leg.ctx.patch_correlation(leg.dev(t), leg.dev(m), t.shape[::-1], window, out)
            return {"corr": leg.host(out)}

        def check_pc(leg, outs, window=window):     # test_kernel_against_restatement
            want = P.R.patch_correlation(t, m, window[::-1])
            got = outs["corr"]
            zero = want == 0
            assert zero.sum() > 0 and np.all(got[zero] == 0.0) and np.all(np.abs(got) <= 1.0)
            np.testing.assert_allclose(got, want, rtol=0, atol=P.ULP)

        case(f"patch-correlation-{'x'.join(map(str, window))}", "pp_patch_correlation_f32", t.size, check_pc, scratch=False, **kw)(run_pc)

    a, b = P.mi_pairs()["noise"]
    for bins in (64, 130):                      # the LDS table; global integer atomics
        def run_jh(leg, bins=bins):
            hist, rng = leg.hempty((bins, bins), np.int64), leg.hempty(4)
            assert leg.lib.pp_joint_histogram_f32(leg.ctx.h, leg.p(a), leg.p(b), a.size, bins, bins, hptr(hist, C.c_int64), hptr(rng)) == 0
            return {"hist": hist, "range": rng}

        def check_jh(leg, outs, bins=bins):     # test_joint_histogram_kernel_beyond_the_lds_table
            want, ea, eb = P.R.joint_histogram(a, b, bins)
            assert np.array_equal(outs["hist"], want) and tuple(outs["range"]) == (ea[0], ea[-1], eb[0], eb[-1])

        case(f"joint-histogram-{bins}", "pp_joint_histogram_f32", a.size, check_jh, **kw)(run_jh)


_patch_and_histograms()


def _staple():
    from tests import staple_restatement as SR
    ST = T("staple")
    kw = dict(family="reduce")
    shape = ST.SHAPE
    n = int(np.prod(shape))
    _, raters = ST._raters(shape, 5, 3)

    for dtype, rescale in (("uint8", False), ("float32", True)):
        labels = ST._as_dtype(raters, dtype, 4)

        def run(leg, labels=labels, dtype=dtype, rescale=rescale):
            w, res = leg.empty((n,), np.float64), leg.hstruct(_lib.StapleResult)
            prm = _lib.StapleParams(_lib.STAPLE_FOREGROUND, int(rescale), 1.0, 1.0, (1 << 64) - 1, 1e-4 if rescale else float("-inf"))
            dev = [leg.dev(x) for x in labels]
            ptrs = (C.c_void_p * len(dev))(*[_lib.ptr(x) for x in dev])
            assert leg.lib.pp_staple_fuse(leg.ctx.h, ptrs, int(dtype == "float32"), len(dev), n, C.byref(prm), _lib.ptr(w), C.byref(res)) == 0
            return {"w": leg.host(w), **fields(res, sensitivity=len(dev), specificity=len(dev))}

        def check(leg, outs, labels=labels, rescale=rescale):       # tests/test_staple.py::_check, tests/test_reduction_edges.py::test_staple_rescale_257_blocks
            w, p, q, it, degenerate = SR.staple_patterns(labels)
            want = SR.rescale_threshold(w, 1e-4) if rescale else w
            assert not degenerate and not outs["degenerate"] and abs(int(outs["elapsed_iterations"]) - it) <= 3
            np.testing.assert_allclose(outs["w"], want.ravel(), rtol=0, atol=1e-7)
            np.testing.assert_allclose(outs["sensitivity"], p, rtol=0, atol=1e-12)
            np.testing.assert_allclose(outs["specificity"], q, rtol=0, atol=1e-12)
            keys = SR.keys_of(labels)
            assert (outs["n_zero"], outs["n_one"]) == ((keys == 0).sum(), (keys == (1 << len(labels)) - 1).sum())
            assert outs["n_mixed"] == n - outs["n_zero"] - outs["n_one"]

        case(f"staple-{dtype}{'-rescale' if rescale else ''}", "pp_staple_fuse", n, check, **kw)(run)


_staple()


# ======================================================================================
# linear-registration metrics (tests/test_linear_metric_kernels.py: the lattices `ragged` -- a ragged last block -- and
# `column`; every sum within the restatement's own bound, counts exact)


def _linear_metrics(key, setter=None):
    LM = T("linear_metric_kernels")
    LR = LM.LR
    c = LM.CASES[key]
    kw = dict(family="reduce")
    tag = f"{key}{'-' + setter if setter else ''}"
    setters = {None: (), "jitter": ("pp_linear_set_sample_jitter",),
               "gimg": ("pp_linear_set_moving_gradient", "pp_linear_set_moving_gradient_packed")}[setter]

    def ref(cand=0):
        return LM.reference(key, jitter=setter == "jitter", gimg=setter == "gimg", cand=cand)

    class installed:
        """The case's jitter array or gradient image in force on the leg's context for the `with` block."""

        def __init__(self, leg):
            self.leg = leg

        def __enter__(self):
            F, M, _, _, GI, jit = LM.data(key)
            leg = self.leg
            if setter == "jitter":
                self.keep = leg.dev(jit)
                leg.ctx.set_sample_jitter(self.keep)
            elif setter == "gimg":
                self.keep = (leg.dev(GI), leg.dev(np.ascontiguousarray(np.concatenate([np.moveaxis(GI, 0, -1), M[..., None]], axis=-1)), align=16))
                leg.ctx.set_moving_gradient(self.keep[0], LM.size_of(c["mshape"]), packed=self.keep[1])
            return LM.call_args(leg, key)

        def __exit__(self, *exc):
            self.leg.ctx.set_sample_jitter(None)
            self.leg.ctx.set_moving_gradient(None)

    def head(leg, a):
        return (leg.ctx.h, _lib.ptr(a["fixed"]), _lib._i3(a["fsize"]), _lib.ptr(a["moving"]), _lib._i3(a["msize"]), _lib._dn(a["Af"], 9), _lib._dn(a["bf"], 3))

    def tail(a):
        return (_lib._i3(a["vsize"]), int(a["stride"]), _lib.ptr(a["fixed_mask"]), _lib.ptr(a["moving_mask"]))

    def run_grad(leg):
        out = {}
        with installed(leg) as a:
            for name, nres in (("meansq", 14), ("corr_moments", 42)):
                res = leg.hempty(nres)
                fn = getattr(leg.lib, f"pp_{name}_affine_f32")
                assert fn(*head(leg, a), _lib._dn(c["Am"].ravel(), 9), _lib._dn(c["bm"], 3), *tail(a), hptr(res)) == 0
                out[name] = res
        return out

    def check_grad(leg, outs):      # test_gradient_kernels / test_sample_jitter / test_gradient_image
        LM.check_grad(leg, key, "memory-state:" + tag, {"meansq_affine": outs["meansq"], "corr_moments_affine": outs["corr_moments"]}, ref())

    def bad_grad(leg):
        a = LM.call_args(leg, key)
        res = leg.hempty(14)
        return leg.lib.pp_meansq_affine_f32(leg.ctx.h, None, *head(leg, a)[2:], _lib._dn(c["Am"].ravel(), 9), _lib._dn(c["bm"], 3), *tail(a), hptr(res))

    case(f"metric-gradient-{tag}", ("pp_meansq_affine_f32", "pp_corr_moments_affine_f32"), LM.SAMPLES[key], check_grad, bad=bad_grad,
         setters=setters, **kw)(run_grad)
    if setter == "gimg":
        return

    ncands = (5, 16)                # one mailbox writer, two

    def run_values(leg):
        out = {}
        cand = LM.candidates(key)
        with installed(leg) as a:
            for metric in (0, 1):
                for n in ncands:
                    am = np.ascontiguousarray(np.asarray([m[0] for m in cand[:n]], dtype=np.float64).reshape(n, 9))
                    bm = np.ascontiguousarray(np.asarray([m[1] for m in cand[:n]], dtype=np.float64).reshape(n, 3))
                    res = leg.hempty((n, 6))
                    assert leg.lib.pp_metric_values_affine_f32(leg.ctx.h, metric, *head(leg, a)[1:], n, hptr(am), hptr(bm), *tail(a), hptr(res)) == 0
                    out[f"metric{metric}-n{n}"] = res
        return out

    def check_values(leg, outs):    # test_value_probes
        for metric in (0, 1):
            for n in ncands:
                r = outs[f"metric{metric}-n{n}"]
                for k in range(n):
                    if k == 2:
                        assert np.array_equal(r[k], np.zeros(6))
                        continue
                    s = ref(k)
                    want, bound = LR.values(metric, s)
                    assert r[k, 1 - metric] == s.count
                    LM.within(r[k], want, bound, (key, metric, n, k))

    case(f"metric-values-{tag}", "pp_metric_values_affine_f32", LM.SAMPLES[key], check_values, setters=setters, **kw)(run_values)

    kinds = ((0, 50), (1, 20))

    def run_mi(leg):
        out = {}
        with installed(leg) as a:
            for kernel, nbins in kinds:
                b, _ = LM.mi_bins(key, kernel, nbins)
                hist, count = leg.hempty((nbins, nbins)), leg.hempty(1)
                mid = (_lib._dn(c["Am"].ravel(), 9), _lib._dn(c["bm"], 3), *tail(a), C.byref(b))
                assert leg.lib.pp_mi_histogram_f32(*head(leg, a), *mid, hptr(hist), hptr(count)) == 0
                table = np.ascontiguousarray(np.random.default_rng(5).normal(size=(nbins, nbins)))
                g = leg.hempty(12)
                assert leg.lib.pp_mi_gradient_f32(*head(leg, a), *mid, hptr(table), hptr(g)) == 0
                out.update({f"hist-k{kernel}": hist, f"count-k{kernel}": count, f"gradient-k{kernel}": g})
        return out

    def check_mi(leg, outs):        # test_mi_kernels
        s = ref()
        for kernel, nbins in kinds:
            _, bd = LM.mi_bins(key, kernel, nbins)
            want, wcount, bound, q = LR.mi_histogram(s, bd)
            assert outs[f"count-k{kernel}"][0] == wcount == s.count
            assert q.bin_margin > 0
            if kernel == 1:
                assert np.array_equal(outs[f"hist-k{kernel}"], want)
            LM.within(outs[f"hist-k{kernel}"], want, bound, (key, kernel, "histogram"))
            table = np.random.default_rng(5).normal(size=(nbins, nbins))
            wg, gbound, _ = LR.mi_gradient(s, bd, table)
            LM.within(outs[f"gradient-k{kernel}"], wg, gbound, (key, kernel, "gradient"))

    case(f"metric-mi-{tag}", ("pp_mi_histogram_f32", "pp_mi_gradient_f32"), LM.SAMPLES[key], check_mi, setters=setters, **kw)(run_mi)


_linear_metrics("ragged")
_linear_metrics("column")
_linear_metrics("ragged", "jitter")
_linear_metrics("ragged", "gimg")


def _linear_optimize(metric):
    """Three line-search iterations of the translation model on the 158-sample lattice of tests/test_linear.py
    (test_meansq_kernel_matches_numpy_and_finite_differences), the level laid out as in
    tests/test_linear_metric_kernels.py::test_cached_paths_against_the_restatement, whose two checks are made: history[0] is the
    metric at the start, stats.value (PP_LINREG_RETURN_BEST) the metric at the returned point, each within the restatement's bound."""
    from tests.helpers import phantom
    LM = T("linear_metric_kernels")
    LR = LM.LR
    F, M = phantom((10, 14, 18), seed=300, noise=0), phantom((12, 13, 17), seed=301, noise=0)
    Af, bf = 2.0 * np.eye(3), np.array([0.5, 0.5, 0.5])
    Am = np.array([[1.9137, 0.1071, 0.0031], [-0.0813, 2.0519, 0.0207], [0.0109, 0.0043, 2.3011]])
    bm = np.array([0.7123, -0.4057, 0.9131])
    vsize, stride, iters = (9, 7, 5), 2, 3
    init = Am @ np.linalg.inv(Af)
    off = bm - init @ bf
    p0 = np.array([0.01373, -0.02117, 0.00931])

    def level():
        lv = _lib.LinregLevel()
        lv.model, lv.metric, lv.optimizer, lv.iterations = _lib.MODEL_TRANSLATION, metric, _lib.OPT_GD_LINE_SEARCH, iters
        lv.vsize[:] = list(vsize)
        lv.stride, lv.speculation, lv.flags = stride, 4, _lib.LINREG_RETURN_BEST
        lv.v_i2p[:], lv.v_origin[:] = Af.ravel().tolist(), bf.tolist()
        lv.f_p2i[:], lv.m_p2i[:] = np.eye(3).ravel().tolist(), np.eye(3).ravel().tolist()
        lv.f_origin[:], lv.m_origin[:] = [0.0] * 3, [0.0] * 3
        lv.init_matrix[:], lv.init_offset[:] = init.ravel().tolist(), off.tolist()
        lv.center[:] = [0.0] * 3
        lv.v_min_spacing = 0.00571
        return lv

    def call(leg, fixed):
        params = np.array(p0)                       # host in/out: the start point is an input
        st, hist = leg.hstruct(_lib.LinregStats), leg.hempty(iters)
        lv = level()
        rc = leg.lib.pp_linear_optimize_f32(leg.ctx.h, fixed, _lib._i3((18, 14, 10)), leg.p(M), _lib._i3((17, 13, 12)), None, None, C.byref(lv),
                                            hptr(params), C.byref(st), hptr(hist), iters)
        return rc, params, st, hist

    def run(leg):
        rc, params, st, hist = call(leg, leg.p(F))
        assert rc == 0
        n = int(st.iterations)
        return {"params": params, "history": hist[:n].copy(), **fields(st)}

    def value_at(p):
        s = LR.Samples(F, M, Af, bf, init @ Af, init @ (bf + p) + off, vsize, stride)
        assert s.margin_of(("f",)) >= LM.MARGIN and s.count > 50      # (the fixed side is dyadic: exact under any evaluation order)
        sums, bound = LR.meansq(s) if metric == 0 else LR.corr(s)
        fn = LR.meansq_value if metric == 0 else LR.corr_value
        return fn(sums), LR.value_bound(fn, sums, bound)

    def check(leg, outs):
        assert 1 <= outs["iterations"] <= iters and outs["evaluations"] > outs["iterations"]
        want0, b0 = value_at(p0)
        assert abs(outs["history"][0] - want0) <= b0
        want1, b1 = value_at(outs["params"])
        assert abs(outs["value"] - want1) <= b1
        assert outs["value"] <= outs["history"][0] and not np.array_equal(outs["params"], p0)      # a step was kept: the lane kernel's number

    def bad(leg):
        return call(leg, None)[0]

    case(f"linear-optimize-{'meansq' if metric == 0 else 'corr'}", "pp_linear_optimize_f32", 158, check, bad=bad, family="reduce")(run)


_linear_optimize(0)
_linear_optimize(1)


# ======================================================================================
# cubic B-spline transform (tests/test_bspline.py, tests/test_bspline_mi.py)


def _bspline_field(name):
    B = T("bspline")
    direction = B.EYE
    lat = B._lattice(B.MESH_A, direction)
    coef = B._coef(lat, 11, 3.0)
    own, big = B._grids(direction)
    grid = big
    if name == "oblique":
        cs, sn = np.cos(np.radians(20.0)), np.sin(np.radians(20.0))
        grid = (big[0], big[1], big[2], np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]]))

    def run(leg):
        return {"out": B._field(leg, coef, lat, grid)}

    def check(leg, outs):           # test_field_kernel_against_restatement
        want = B.R.field(coef, lat, *grid)
        assert np.abs(outs["out"] - want).max() <= 1e-5 * np.abs(coef).max()
        inside, _, _ = B.R.support(B.R.grid_points(*grid), lat)
        inside = inside.reshape(outs["out"].shape[1:])
        assert inside.sum() > 1000 and (~inside).sum() > 0 and np.all(outs["out"][:, ~inside] == 0.0)     # exactly 0 outside the domain

    # (a grid turned against the lattice takes the per-voxel weight path: no weight tables in the scratch)
    case(f"bspline-field-{name}", "pp_bspline_field_f32", 3 * np.prod(grid[0]), check, family="bspline", scratch=name != "oblique")(run)


_bspline_field("larger")
_bspline_field("oblique")


def _bspline_metric(k):
    B = T("bspline")
    metric, mesh, stride, jitter, source, masks = B.CASES[k]
    lat = B._lattice(mesh, B.EYE)
    coef = B._coef(lat, 31, 1.5)
    fg = (B.SIZE, B.SPACING, B.ORIGIN, np.eye(3))

    def parts():
        d = B._metric_inputs()
        jit = d["jitter"][stride] if jitter else None
        fm, mm = (d["fmask"], d["mmask"]) if masks else (None, None)
        return d, jit, fm, mm

    def run(leg):
        d, jit, fm, mm = parts()
        ctx = leg.ctx
        dev = lambda a, **kw: None if a is None else leg.dev(a, **kw)        # noqa: E731
        keep = [dev(d["fixed"]), dev(d["moving"]), dev(coef), dev(fm), dev(mm), dev(jit), dev(d["grad"]), dev(d["packed"], align=16)]
        geom, mgeom, lgeom = _lib.make_geom(B.SIZE, B.SPACING, B.ORIGIN, B.EYE), _lib.make_geom(*B.MOVING[:3], B.MOVING[3].ravel()), B._lat_geom(lat)
        value, st, grad = leg.hempty(1), leg.hempty(4), leg.hempty(coef.size)
        try:
            if jit is not None:
                ctx.set_sample_jitter(keep[5])
            if source == "packed":
                ctx.set_moving_gradient(keep[6], packed=keep[7])
            elif source == "planar":
                ctx.set_moving_gradient(keep[6])
            rc = leg.lib.pp_bspline_metric_f32(ctx.h, _lib.BSPLINE_MEAN_SQUARES if metric == "mean_squares" else _lib.BSPLINE_CORRELATION,
                                               _lib.ptr(keep[0]), C.byref(geom), _lib.ptr(keep[1]), C.byref(mgeom), C.byref(geom), stride,
                                               _lib.ptr(keep[3]), _lib.ptr(keep[4]), _lib.ptr(keep[2]), C.byref(lgeom),
                                               0.0 if jit is None else float(np.abs(jit).max()), hptr(value), hptr(st), hptr(grad))
        finally:
            ctx.set_sample_jitter(None)
            ctx.set_moving_gradient(None)
        assert rc == 0
        return {"value": value, "stats": st, "gradient": grad}

    def check(leg, outs):           # test_metric_kernel_against_restatement
        d, jit, fm, mm = parts()
        want_v, want_g, want_s = B.R.metric(metric, d["fixed"], fg, d["moving"], B.MOVING, fg, stride, coef, lat, fm, mm, jit,
                                            d["grad"] if source else None)
        assert list(outs["stats"]) == [want_s["valid"], want_s["outside"], want_s["masked"], want_s["seen"]]
        gmax = np.abs(want_g).max()
        np.testing.assert_allclose(outs["value"][0], want_v, rtol=1e-5)
        np.testing.assert_allclose(outs["gradient"], want_g, rtol=2e-4 if metric == "mean_squares" else 3e-4, atol=1e-3 * gmax)

    setters = (("pp_linear_set_sample_jitter",) if jitter else ()) + \
        ({"packed": ("pp_linear_set_moving_gradient", "pp_linear_set_moving_gradient_packed"), "planar": ("pp_linear_set_moving_gradient",), None: ()}[source])
    case(f"bspline-metric-{metric}-{k}", "pp_bspline_metric_f32", np.prod(B.SIZE) // stride, check, family="bspline", setters=setters)(run)


_bspline_metric(1)      # mean squares, stride 2, jitter, packed gradient image, masks
_bspline_metric(5)      # correlation, the coarse mesh, stride 1, jitter, masks


def _bspline_mi(name):
    BM = T("bspline_mi")
    RM = BM.RM

    def run(leg):
        c = BM._case(name)
        nb = c["nbins"]
        inst = BM._Installed(leg, c)
        inst.keep[7] = leg.dev(BM._inputs()["packed"], align=16)       # (the header wants the packed image on 16 bytes)
        with inst as k:
            fixed, geom, moving, mgeom, vgeom, stride, coefd, lgeom, bins = k.args
            head = (leg.ctx.h, _lib.ptr(fixed), C.byref(geom), _lib.ptr(moving), C.byref(mgeom), C.byref(vgeom), int(stride), _lib.ptr(k.kw["fixed_mask"]),
                    _lib.ptr(k.kw["moving_mask"]), _lib.ptr(coefd), C.byref(lgeom), float(k.kw["jitter_bound"]), C.byref(bins))
            hist, st1 = leg.hempty((nb, nb)), leg.hempty(4)
            assert leg.lib.pp_bspline_mi_histogram_f32(*head, hptr(hist), hptr(st1)) == 0
            table = np.ascontiguousarray(c["table"], dtype=np.float64)
            st2, grad = leg.hempty(4), leg.hempty(c["coef"].size)
            assert leg.lib.pp_bspline_mi_gradient_f32(*head, hptr(table), hptr(st2), hptr(grad)) == 0
        return {"hist": hist, "hist-stats": st1, "gradient": grad, "gradient-stats": st2}

    def check(leg, outs):           # test_histogram_kernel_against_restatement, test_gradient_kernel_against_restatement
        c = BM._case(name)
        BM._check_ambiguity(c)
        want = c["s"].stats
        for key in ("hist-stats", "gradient-stats"):
            assert list(outs[key]) == [float(want[k]) for k in ("valid", "outside", "masked", "seen")]
        assert np.all(np.abs(outs["hist"] - c["hist"]) - c["hbound"] <= 0.0)
        wg, bound, _ = RM.gradient(c["s"], c["b"], c["table"])
        assert np.all(np.abs(outs["gradient"] - wg) - bound <= 0.0)
        assert np.all(outs["gradient"][RM.outside_support(c["s"])] == 0.0)

    mesh, stride, jitter, source, masks, nbins, flipped = BM.CASES[name]
    setters = (("pp_linear_set_sample_jitter",) if jitter else ()) + \
        ({"packed": ("pp_linear_set_moving_gradient", "pp_linear_set_moving_gradient_packed"), "planar": ("pp_linear_set_moving_gradient",), None: ()}[source])
    case(f"bspline-mi-{name}", ("pp_bspline_mi_histogram_f32", "pp_bspline_mi_gradient_f32"), np.prod(BM.SIZE) // stride, check, family="bspline",
         setters=setters)(run)


_bspline_mi("A-s2-jit-packed-masks-30")
_bspline_mi("C-jit-masks-30")


# ======================================================================================
# field tools (tests/test_field_inverse.py, tests/test_field_jacobian.py: sizes (33, 18, 9) and (5, 1, 4))


def _field_tools(size):
    FI, FJ = T("field_inverse"), T("field_jacobian")
    R = FI.R
    spacing, origin, direction = FI.GEOMS["rot20"]
    shape = FI.zyx(size)
    sid = "x".join(map(str, size))
    n = 3 * int(np.prod(size))
    u = FI.make_field(size, spacing)
    v0 = (-0.5 * u).astype(np.float32)

    def geom():
        return _lib.make_geom(size, spacing, origin, direction.ravel())

    for iterations in (0, 3):
        def call(leg, fld, out, st, iterations=iterations):
            g = geom()
            return leg.lib.pp_invert_field_f32(leg.ctx.h, fld, C.byref(g), leg.p(v0), iterations, 0.0, 0.0, 1, _lib.ptr(out), C.byref(st))

        def run(leg, call=call):
            out, st = leg.empty((3,) + shape), leg.hstruct(_lib.InvertStats)
            assert call(leg, leg.p(u), out, st) == 0
            return {"inverse": leg.host(out), **fields(st)}

        def check(leg, outs, iterations=iterations):
            if iterations == 0:     # test_zero_iterations_returns_the_initial_estimate
                assert np.array_equal(outs["inverse"], v0) and outs["iterations"] == 0 and np.isinf(outs["max_error_norm"]) and np.isinf(outs["mean_error_norm"])
                return
            # test_kernel_matches_restatement_at_fixed_iterations
            ref, hist = R.invert(u, spacing, direction, 10, 0.0, 0.0, True, v0)
            b = R.inversion_bound(u, spacing, direction, hist, iterations)
            assert max(b["dc"]) < min(h["margin"] for h in hist[:iterations])
            assert FI.scaled_error(outs["inverse"], hist[iterations - 1]["v"], spacing) <= b["E"]
            h = hist[iterations - 1]
            assert outs["iterations"] == iterations
            assert abs(outs["max_error_norm"] - h["M"]) <= b["e_r"][-1] and abs(outs["mean_error_norm"] - h["mean"]) <= b["e_r"][-1] + 2.0 ** -25

        def bad(leg, call=call):
            return call(leg, None, leg.empty((3,) + shape), leg.hstruct(_lib.InvertStats))

        case(f"invert-field-{sid}-{iterations}", "pp_invert_field_f32", n, check, bad=bad, family="field")(run)

    v = (-0.7 * u).astype(np.float32)

    def run_ic(leg):
        norm, st = leg.empty(shape), leg.hstruct(_lib.InvertStats)
        g = geom()
        assert leg.lib.pp_inverse_consistency_f32(leg.ctx.h, leg.p(u), leg.p(v), C.byref(g), _lib.ptr(norm), C.byref(st)) == 0
        return {"norm": leg.host(norm), **fields(st)}

    def check_ic(leg, outs):        # test_inverse_consistency_is_the_next_iterations_residual
        _, hist = R.invert(u, spacing, direction, 4, 0.0, 0.0)
        b = R.inversion_bound(u, spacing, direction, hist, 4)
        res = R.residual(u, v, spacing, direction)
        assert np.abs(outs["norm"] - res["s"]).max() <= b["e_r"][0] and outs["iterations"] == 1
        assert abs(outs["max_error_norm"] - res["M"]) <= b["e_r"][0] and abs(outs["mean_error_norm"] - res["mean"]) <= b["e_r"][0] + 2.0 ** -25

    case(f"inverse-consistency-{sid}", "pp_inverse_consistency_f32", n, check_ic, family="field")(run_ic)

    ju = (4.0 * R.windowed_sinusoid(shape, FJ.SPACING, seed=3)).astype(np.float32)
    rng = np.random.default_rng(4)
    mask = (rng.random(shape) < 0.4).astype(np.uint8) * rng.integers(1, 255, shape).astype(np.uint8)

    def run_j(leg):
        out = {}
        g = _lib.make_geom(size, FJ.SPACING, (1.0, -2.0, 3.0))
        for name, m in (("all", None), ("masked", mask)):
            det, st = leg.empty(shape), leg.hstruct(_lib.JacobianStats)
            assert leg.lib.pp_jacobian_determinant_f32(leg.ctx.h, leg.p(ju), C.byref(g), 1, None if m is None else leg.p(m), _lib.ptr(det), C.byref(st)) == 0
            out[name + "-det"] = leg.host(det)
            out.update({f"{name}-{k}": x for k, x in fields(st).items()})
        return out

    def check_j(leg, outs):         # test_smooth_field_matches_restatement (the bound), test_statistics
        ref = R.jacobian_determinant(ju, FJ.SPACING, True)
        bound = FJ.jacobian_bound(np.abs(ju).max(), 1.0 / min(FJ.SPACING), FJ.entries_max(ju, FJ.SPACING, True), False)
        for name, m in (("all", None), ("masked", mask)):
            got = outs[name + "-det"]
            assert np.abs(got - ref).max() <= bound
            sel = got[m > 0] if m is not None else got.ravel()
            assert outs[f"{name}-count"] == sel.size and outs[f"{name}-count_nonpositive"] == int((sel <= 0).sum())
            assert outs[f"{name}-min"] == float(sel.min()) and outs[f"{name}-max"] == float(sel.max())
            mean = float(sel.astype(np.float64).sum() / sel.size)
            assert abs(outs[f"{name}-mean"] - mean) <= 2.0 ** -25 + sel.size * 2.0 ** -53 * float(np.abs(sel).max())

    case(f"jacobian-determinant-{sid}", "pp_jacobian_determinant_f32", n, check_j, family="field")(run_j)


_field_tools((33, 18, 9))
_field_tools((5, 1, 4))
