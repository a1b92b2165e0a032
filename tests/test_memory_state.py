"""Every C-ABI operation on dirty outputs, dirty scratch and a used context (the case table: tests/memory_state_cases.py).

The kernel tests elsewhere hand the library zero-filled outputs and, mostly, a context whose scratch they never look at; the
product allocates with torch.empty and reuses one context for everything.  A kernel that skips an output voxel whose correct
value is 0, reads scratch it did not write, or leaves a counter behind passes there and fails here.  Every case runs four legs:

  base      fresh context, outputs pre-filled with zeros, no switch: held to the case's reference (its own test's bound)
  garbage A fresh context under PP_POISON_WS=1 (the GROWTH arm of pp_reserve, poisoned as a whole), outputs filled with 0xFF
            bytes (NaN) for float types and 0xA5 bytes for integer types, host arrays and statistics structs included
  garbage B the context of leg A without the switch (the REUSE arm) after a dirtier -- unrelated operations of another family on
            as many voxels, whose scratch is at least as large -- left real data, counters and tables in the scratch; outputs
            filled with +1e30 / 0x5A bytes, so that a skipped element that happened to equal pattern A cannot hide twice
  used      the session context of the `backend` fixture, whatever ran on it before, directly after a call that returned
            PP_ERR_ARG; outputs filled as in leg A

Legs A, B and used must equal base BIT FOR BIT, outputs and returned statistics: include/platipy_amd.h, DESIGN.md or the
operation's own rerun test promise identical bits for every operation in the table (integer atomics and fixed-order folds), so
REFERENCE_BOUND_ONLY below is empty and must stay so for any operation whose tests assert identical bits.

The CPU emulation runs the blocks of a launch one after another: it vouches for stores and for scratch that is read before it
is written, not for tickets, last-block folds or the mailbox; only the gpu legs see those.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from platipy_amd import _lib
from tests import memory_state_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "platipy_amd.h")

# Operations held to their reference bound on every leg instead of to the bits of the base leg, each with the sentence that
# says why no promise of identical reruns exists.  Empty: every operation of the table carries such a promise.
REFERENCE_BOUND_ONLY = {}

# Entry points that neither write device memory nor reserve scratch.
EXEMPT = {
    "pp_abi_version": "returns a constant",
    "pp_reload_switches": "re-reads the environment into the host-side switch snapshot",
    "pp_create": "allocates the context; every leg creates or reuses one",
    "pp_destroy": "frees the context; every fresh-context leg ends with it",
    "pp_last_error": "returns the context's host-side message",
    "pp_set_stream": "waits for the old stream, then stores the new handle (tests/test_stream_order.py holds it to that)",
    "pp_sync": "waits for the stream; every leg calls it before reading back",
    "pp_workspace_bytes": "returns a host-side size; the garbage-A leg reads it",
    "pp_profile_enable": "host-side switch of the event brackets",
    "pp_profile_read": "reads HIP event timings into a host array",
    "pp_gauss_taps": "host arithmetic only",
    "pp_demons_default_params": "fills a host struct with constants",
    "pp_demons_history": "copies the device ring to host arrays; covered as an OUTPUT of the demons-execute cases",
    "pp_linear_num_parameters": "returns a constant per model",
    "pp_linear_set_sample_jitter": "stores a caller-owned pointer; in force in the linear-metric jitter case",
    "pp_linear_set_moving_gradient": "stores a caller-owned pointer; in force in the gradient-image case",
    "pp_linear_set_moving_gradient_packed": "stores a caller-owned pointer; in force in the gradient-image case",
}
SETTERS = ("pp_linear_set_sample_jitter", "pp_linear_set_moving_gradient", "pp_linear_set_moving_gradient_packed")

FILL_BASE = (0, 0, 0)                   # (float pattern, integer pattern, struct byte): an int is a BYTE value
FILL_A = (0xFF, 0xA5, 0xFF)
FILL_B = (1.0e30, 0x5A, 0x5A)


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", text)))


def test_every_entry_point_is_a_case_or_exempt_for_a_reason():
    covered = {fn for c in M.CASES for fn in c.fns}
    declared = set(declared_symbols())
    assert len(declared) >= 80
    assert covered <= declared, covered - declared
    assert set(EXEMPT) <= declared, set(EXEMPT) - declared
    assert all(isinstance(r, str) and len(r) > 10 for r in EXEMPT.values())
    allowed = {"pp_abi_version", "pp_reload_switches", "pp_create", "pp_destroy", "pp_last_error", "pp_set_stream", "pp_sync",
               "pp_workspace_bytes", "pp_profile_enable", "pp_profile_read", "pp_gauss_taps", "pp_demons_default_params",
               "pp_demons_history", "pp_linear_num_parameters"} | set(SETTERS)
    assert set(EXEMPT) <= allowed, f"may not be exempt: {sorted(set(EXEMPT) - allowed)}"
    assert not (covered & set(EXEMPT)) or (covered & set(EXEMPT)) <= {"pp_demons_history"}
    missing = declared - covered - set(EXEMPT)
    assert not missing, f"neither a case nor exempt: {sorted(missing)}"
    in_force = {s for c in M.CASES for s in c.setters}
    assert in_force == set(SETTERS), set(SETTERS) - in_force
    assert not (set(REFERENCE_BOUND_ONLY) - covered)
    ids = [c.id for c in M.CASES]
    assert len(ids) == len(set(ids))


# --------------------------------------------------------------------------------------
# the legs


def fresh_context(be):
    if be.name == "gpu":
        return _lib.Context(0, be.torch.cuda.current_stream().cuda_stream, lib=be.lib)
    return _lib.Context(0, 0, lib=be.lib)


def dirty(be, ctx, case, need_bytes):
    """Unrelated work of another family on the context, on as many voxels as the case has (more, while its scratch is
    smaller than the case's): a distance map and a dose histogram -- a transposed volume, scan tables and integer counters in
    the scratch -- or, for the mask and reduction families, a recursive Gaussian and a field inversion -- float volumes and
    the residual reduction's partials."""
    n = max(case.nvox, 512)
    rng = np.random.default_rng(case.nvox)
    for _ in range(8):
        nz = max(int(round((n / 6.0) ** (1.0 / 3.0))), 2)
        shape = (nz, 2 * nz + 1, 3 * nz + 2)
        size = (shape[2], shape[1], shape[0])
        if case.family in ("mask", "reduce"):
            f = be.dev((50.0 * rng.standard_normal((3,) + shape)).astype(np.float32))
            ctx.recursive_gaussian_field(f, _lib.make_geom(size, (0.8, 1.3, 2.5)), (2.0, 2.0, 3.0))
            ctx.invert_field(f, _lib.make_geom(size), be.garbage((3,) + shape, np.float32, 3.0), max_iterations=2, want_stats=True)
        else:
            m = be.dev((rng.random(shape) < 0.4).astype(np.uint8))
            ctx.distance_map(m, _lib.make_geom(size, (0.9, 1.1, 2.5)), be.garbage(shape, np.float32, 7.0), signed=True)
            ctx.dose_histogram(be.dev((60.0 * rng.random(shape)).astype(np.float32)), [m], int(np.prod(shape)), np.linspace(0.0, 61.0, 300))
        ctx.sync()
        if ctx.workspace_bytes() >= need_bytes:
            return
        n *= 2
    raise AssertionError("the dirtier's scratch stays smaller than the case's")


def refused_call(leg, case):
    """A call that returns PP_ERR_ARG on the leg's context: the case's own with a NULL input where it names one."""
    if case.bad is not None:
        rc = case.bad(leg)
    else:
        r = C.c_double(0.0)
        rc = leg.lib.pp_sum_sq_diff_f32(leg.ctx.h, None, None, 8, C.byref(r))
    assert rc == _lib.ERR_ARG, rc


def assert_same_bits(got, base, what):
    assert sorted(got) == sorted(base), (what, sorted(got), sorted(base))
    for name in base:
        g, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(base[name])
        assert g.shape == b.shape and g.dtype == b.dtype, (what, name, g.shape, b.shape, g.dtype, b.dtype)
        if g.tobytes() != b.tobytes():
            gv, bv = g.reshape(-1).view(np.uint8).reshape(g.size, -1), b.reshape(-1).view(np.uint8).reshape(b.size, -1)
            bad = np.flatnonzero((gv != bv).any(axis=1))
            raise AssertionError(f"{what}: output `{name}` differs from the base leg in {bad.size} of {g.size} elements, first at "
                                 f"{bad[:5].tolist()}: {g.reshape(-1)[bad[:5]]} instead of {b.reshape(-1)[bad[:5]]}")


def hold(case, leg, outs, base, what):
    if set(case.fns) & set(REFERENCE_BOUND_ONLY):
        case.check(leg, outs)
    else:
        assert_same_bits(outs, base, f"{case.id} [{leg.name}] {what}")


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.id)
def test_memory_state(backend, monkeypatch, case):
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    ctx = fresh_context(backend)
    try:
        leg = M.Leg(backend, ctx, *FILL_BASE)
        base = case.run(leg)
        case.check(leg, base)
    finally:
        ctx.close()
    ctx = fresh_context(backend)
    try:
        monkeypatch.setenv("PP_POISON_WS", "1")
        leg = M.Leg(backend, ctx, *FILL_A)
        outs = case.run(leg)
        ctx.sync()
        ws = ctx.workspace_bytes()
        assert (ws > 0) == case.scratch, (case.id, ws)       # the growth arm was taken (and poisoned), or there is no scratch
        hold(case, leg, outs, base, "garbage A (poisoned growth arm, 0xFF / 0xA5 outputs)")
        monkeypatch.delenv("PP_POISON_WS")
        dirty(backend, ctx, case, ws)
        before = ctx.workspace_bytes()
        leg = M.Leg(backend, ctx, *FILL_B)
        outs = case.run(leg)
        ctx.sync()
        assert ctx.workspace_bytes() == before, "leg B was meant to take the reuse arm"
        hold(case, leg, outs, base, "garbage B (reuse arm after a dirtier, 1e30 / 0x5A outputs)")
    finally:
        ctx.close()
    leg = M.Leg(backend, backend.ctx, *FILL_A)
    refused_call(leg, case)
    outs = case.run(leg)
    hold(case, leg, outs, base, "used context, after a refused call")


# --------------------------------------------------------------------------------------
# the Python layer: every torch.empty / empty_like / new_empty buffer holds garbage, the scratch is poisoned


def _garbage_allocators(monkeypatch):
    """torch.empty, torch.empty_like and Tensor.new_empty return tensors filled with NaN (float types), 113 (integer types) or
    True (bool), on every device -- what tools/poison_check.py does for CUDA tensors."""
    import torch

    def filled(t):
        if t.is_floating_point() or t.is_complex():
            t.fill_(float("nan"))
        elif t.dtype == torch.bool:
            t.fill_(True)
        else:
            t.fill_(113)
        return t

    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: filled(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: filled(empty_like(*a, **k)))
    monkeypatch.setattr(torch.Tensor, "new_empty", lambda self, *a, **k: filled(new_empty(self, *a, **k)))


# Every builder takes `images`: an object whose image_from_array(array, spacing, origin) makes the INPUT images (None: the
# package's own, a plain upload).  tests/test_buffer_views.py passes one that puts every input into an offset view.


def _path_demons(pa, images=None):
    from tests.helpers import phantom, random_dvf
    from oracle import oracle as O
    shape, spacing = (12, 20, 72), (1.0, 1.0, 1.0)
    fix = phantom(shape, seed=40)
    dv = random_dvf(shape, spacing, seed=41, max_mm=2.5)
    mov = O.warp_image(O.Vol(fix, spacing, (0.0, 0.0, 0.0)), dv.astype(np.float64), edge_value=-1000.0).arr.astype(np.float32)
    mk = (images or pa).image_from_array
    f, m = mk(fix, spacing), mk(mov, spacing)

    def run():
        img, _, dvf = pa.registration.fast_symmetric_forces_demons_registration(f, m, resolution_staging=[2, 1], iteration_staging=[4, 3])
        return [img.numpy(), dvf.numpy()]
    return run


def _path_linear(pa, images=None):
    from tests.test_linear import _rigid_pair
    shape, spacing, origin = (16, 20, 24), (1.5, 1.5, 2.5), (-30.0, -20.0, 10.0)
    fix, mov, _ = _rigid_pair(pa, shape, spacing, origin, angle=0.05, shift=(1.5, -1.0, 1.0))
    mk = (images or pa).image_from_array
    f, m = mk(fix, spacing, origin), mk(mov, spacing, origin)

    def run():
        img, tfm = pa.registration.linear_registration(f, m, reg_method="affine", optimiser="gradient_descent_line_search", shrink_factors=[2, 1],
                                                       smooth_sigmas=[1, 0], sampling_rate=0.5, number_of_iterations=4)
        return [img.numpy(), np.asarray(tfm.transforms[1].GetParameters())]
    return run


def _path_combine_labels(pa, images=None):
    from tests.helpers import phantom, smooth_noise
    from tests.test_kernels import GRIDS
    shape, spacing, origin = GRIDS[0]
    mk = (images or pa).image_from_array
    tgt = mk(phantom(shape, seed=70), spacing, origin)
    atl = [mk(phantom(shape, seed=70, noise=0) + 30 * smooth_noise(shape, 71 + i).astype(np.float32), spacing, origin) for i in range(3)]
    labels = [mk((smooth_noise(shape, 80 + i, cells=4) > 0.1).astype(np.uint8), spacing, origin) for i in range(3)]

    def run():
        aset = {str(i): {"DIR": {"Weight Map": pa.label.compute_weight_map(tgt, atl[i], vote_type="local"), "S": labels[i]}} for i in range(3)}
        return [aset[str(i)]["DIR"]["Weight Map"].numpy() for i in range(3)] + [pa.label.fusion.combine_labels(aset, "S")["S"].numpy()]
    return run


def _path_surface_metrics(pa, images=None):
    from tests import comparison_restatement as CR
    a, b = CR.blob_pair((20, 24, 28), 3)
    mk = (images or pa).image_from_array
    ia, ib = mk(a.astype(np.uint8), (0.9, 1.1, 2.5)), mk(b.astype(np.uint8), (0.9, 1.1, 2.5))

    def run():
        got = pa.label.comparison.compute_surface_metrics(ia, ib)
        return [np.array([got[k] for k in sorted(got)])]
    return run


def _path_dvh(pa, images=None):
    from tests.test_dose import images as dose_images
    dose, labels, _ = dose_images(images or pa)

    def run():
        t = pa.dose.dvh_table(dose, labels)
        return [np.asarray(t.counts), np.asarray(t.cc), np.asarray(t.mean)[np.isfinite(t.mean)], np.asarray(t.min)[np.isfinite(t.min)],
                np.asarray(t.max)[np.isfinite(t.max)]]
    return run


def _path_invert_field(pa, images=None):
    import torch
    from tests.test_field_inverse import make_field
    size, spacing = (33, 18, 9), (0.9, 0.9, 2.5)
    if images is None:
        field = pa.Image(torch.from_numpy(make_field(size, spacing)).to(pa.runtime.default_device()), spacing, (1.0, 2.0, 3.0))
    else:
        field = images.image_from_array(make_field(size, spacing), spacing, (1.0, 2.0, 3.0))

    def run():
        from platipy_amd.registration import invert_displacement_field
        inv, info = invert_displacement_field(field, 4, 0.0, 0.0, return_info=True)
        return [inv.numpy(), np.array([info["iterations"], info["max_error_norm"], info["mean_error_norm"]])]
    return run


def _path_external_mask(pa, images=None):
    from tests.external_mask_restatement import head_phantom
    image = (images or pa).image_from_array(head_phantom().copy(), (0.9, 1.1, 2.5))

    def run():
        return [pa.generation.get_external_mask(image, max_hole_size=3).numpy()]
    return run


def _path_bspline(pa, images=None):
    from tests.test_bspline import E2E_SPACING, _e2e_pair
    fixed, _, moving, _, _ = _e2e_pair()
    f, m = (pa.Image(fixed, E2E_SPACING), pa.Image(moving, E2E_SPACING)) if images is None else \
        (images.image_from_array(fixed, E2E_SPACING), images.image_from_array(moving, E2E_SPACING))

    def run():
        out, t = pa.registration.bspline_registration(f, m, resolution_staging=[1], smooth_sigmas=[0], grid_scale_factors=[1], initial_grid_spacing=24,
                                                      sampling_rate=1.0, itk_sampling=False, optimiser="lbfgsb", number_of_iterations=4,
                                                      metric="mean_squares")
        return [out.numpy(), np.asarray(t.level_values[0])]
    return run


PYTHON_PATHS = {"demons": _path_demons, "linear_registration": _path_linear, "combine_labels": _path_combine_labels,
                "compute_surface_metrics": _path_surface_metrics, "dvh_table": _path_dvh, "invert_field": _path_invert_field,
                "get_external_mask": _path_external_mask, "bspline_registration": _path_bspline}


@pytest.mark.parametrize("path", list(PYTHON_PATHS))
def test_python_layer_on_garbage_allocations(host_api, monkeypatch, path):
    """The public path once plain and once with garbage-filled allocations and a poisoned scratch: bit-identical, no NaN.  The
    inputs are made before the allocators are patched, so they are ordinary."""
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    run = PYTHON_PATHS[path](host_api)
    plain = [np.array(x) for x in run()]
    _garbage_allocators(monkeypatch)
    monkeypatch.setenv("PP_POISON_WS", "1")
    dirty_run = [np.array(x) for x in run()]
    assert len(plain) == len(dirty_run)
    for k, (a, b) in enumerate(zip(plain, dirty_run)):
        assert a.shape == b.shape and a.dtype == b.dtype, (path, k)
        assert not (a.dtype.kind == "f" and (np.isnan(a).any() or np.isnan(b).any())), (path, k, "NaN in the result")
        assert a.tobytes() == b.tobytes(), (path, k, int((a != b).sum()), "elements differ under garbage allocations")
