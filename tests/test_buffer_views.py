"""Every C-ABI operation of the case table (tests/memory_state_cases.py) on canaried offset views (tests/buffer_views.py).

Everywhere else in the suite a buffer is a whole, fresh allocation: it starts on a 256-byte boundary and allocator slack
follows it.  The product also passes views -- one component of a field, one level of a pyramid stack -- where an element
stored past the end lands in the neighbour, and where the host-side predicates that pick a kernel arm from the pointers'
residues mod 4, 8 and 16 take the other arm.  Every case runs a base leg (plain M.Leg, zero-filled whole allocations, held to
the case's reference) and five legs of views (shifts in whole elements):

  leg     inputs                          outputs
  bands   0                               0          (canaries only)
  in      1                               0
  out     0                               1
  all     3                               2
  quad    4 for uint8, 2 for all others   the same   (uint8 on 4 mod 16: between the two predicates of the byte kernels;
                                                      the others on 8 mod 16)

Each leg asserts, in this order: the call succeeded; every canary byte of every buffer is intact; no input buffer changed
(IN_OUT below excepted); the case's own reference and bound hold; the outputs equal the base leg bit for bit
(GROUPING_FOLLOWS_ALIGNMENT below excepted).  No tolerance is set here.

The CPU emulation runs the blocks of a launch in order and has no buffer-resource accesses: it vouches for the host-side
predicates, the refusals and plain out-of-range indices, not for what wide or hardware-clamped accesses do on an unaligned
base; only the gpu legs see those.
"""
import ctypes as C
import re

import numpy as np
import pytest

from platipy_amd import _lib
from tests import buffer_views as V
from tests import memory_state_cases as M
from tests.test_memory_state import FILL_A, FILL_BASE, HEADER, assert_same_bits, fresh_context

# Entry points whose header text declares a buffer in/out, with that text.  A changed input is accepted only for these, and
# only when its final bytes are one of the outputs the case returns (it IS the result), never for their read-only inputs.
IN_OUT = {
    "pp_smooth_field_f32": "in place on a planar 3-vector field",
    "pp_recursive_gaussian_field_f32": "in place on a planar field",
    "pp_rescale_threshold_f32": "(label/fusion.py:282-288), in place.",
    "pp_compose_field_f32": "total(x) += iter(x + total(x)), 0 outside; both on grid g.",
    "pp_fuse_accumulate_u8": "wsum += w (if wsum != NULL); wlsum += w * label.",
    "pp_fuse_accumulate_f32": "the same with a float label",
}

# Entry points whose floating-point SUMS may differ from the aligned run's in the last bits: launch geometry and per-thread
# grouping follow a `vec` predicate on the pointer.  Integer and mask outputs are never excused.  {entry point: (reason, the
# record members held to the case's reference bound instead of to bits)}
GROUPING_FOLLOWS_ALIGNMENT = {
    "pp_surface_stats_f32": ("platipy_amd/csrc/pp_compare.h:296-297: vec = select on 16 bytes picks (n + 15) / 16 work items, and at :161-170 a "
                             "thread then sums 16 consecutive voxels instead of one per step, so the fp64 partial sums are grouped differently; "
                             "include/platipy_amd.h says so at pp_surface_stats_f32", ("sum", "sum_sq")),
}

# Alignment the header requires of a buffer: {entry point: (argument, bytes)}; the case table passes align= for each.
REQUIRED_ALIGNMENT = {"pp_surface_stats_f32": ("out", 8), "pp_slice_masked_count_u8": ("per_slice", 8),
                      "pp_linear_set_moving_gradient_packed": ("packed", 16), "pp_demons_execute_f32": ("field", 16)}

SEEN = {}       # (backend, case id) -> {leg: [(role, shift in bytes, address mod 16)]}


def header_text():
    text = open(HEADER).read()
    return re.sub(r"\s+", " ", re.sub(r"^\s*/?\*+ ?", "", text, flags=re.M))


def test_the_tables_quote_the_header():
    text = header_text()
    allowed = {"pp_smooth_field_f32", "pp_recursive_gaussian_field_f32", "pp_rescale_threshold_f32", "pp_compose_field_f32",
               "pp_fuse_accumulate_u8", "pp_fuse_accumulate_f32"}
    assert set(IN_OUT) <= allowed, set(IN_OUT) - allowed
    for fn, sentence in IN_OUT.items():
        assert re.sub(r"\s+", " ", sentence) in text, (fn, sentence)
    covered = {fn for c in M.CASES for fn in c.fns} | {s for c in M.CASES for s in c.setters}
    assert set(IN_OUT) <= covered and set(GROUPING_FOLLOWS_ALIGNMENT) <= covered and set(REQUIRED_ALIGNMENT) <= covered
    assert len(GROUPING_FOLLOWS_ALIGNMENT) < 5
    assert "a select that starts elsewhere may differ from an aligned one's in the last bits" in text
    assert "PP_DEMONS_FUSED needs `field` on a 16-byte boundary" in text and "PP_DEMONS_AUTO takes the staged variant" in text
    assert "out (DEVICE, 8-byte aligned)" in text and "size[2] x int64, 8-byte aligned" in text and "(gx, gy, gz, m) per voxel, 16-byte aligned" in text


# --------------------------------------------------------------------------------------
# one case, all its legs


def grouped_bits(case, outs, base, what):
    """The bit comparison of an entry of GROUPING_FOLLOWS_ALIGNMENT: every member of the record but the excused sums."""
    excused = {m for fn in case.fns if fn in GROUPING_FOLLOWS_ALIGNMENT for m in GROUPING_FOLLOWS_ALIGNMENT[fn][1]}
    assert case.fns == ("pp_surface_stats_f32",), case.fns
    dt = _lib.SURFACE_STATS_DTYPE
    assert sorted(outs) == sorted(base)
    for name in base:
        g, b = outs[name].view(dt)[0], base[name].view(dt)[0]
        for member in dt.names:
            if member not in excused:
                assert np.asarray(g[member]).tobytes() == np.asarray(b[member]).tobytes(), (what, name, member, g[member], b[member])


def hold_views(case, leg, outs, base):
    """The assertions of one view leg after case.run(leg) returned `outs`, in the order of the module docstring."""
    what = f"{case.id} [{leg.name}, leg {leg.leg}]"
    bad = V.check_bands(leg)
    assert not bad, V.bands_message(what, bad)
    results = {np.ascontiguousarray(o).tobytes() for o in outs.values()}
    in_out = bool(set(case.fns) & set(IN_OUT))
    for v in V.inputs_changed(leg):
        assert in_out and v.data_bytes() in results, f"{what}: an input buffer changed ({v.describe()}) that no header sentence declares in/out"
    case.check(leg, outs)
    if set(case.fns) & set(GROUPING_FOLLOWS_ALIGNMENT):
        grouped_bits(case, outs, base, what)
    else:
        assert_same_bits(outs, base, what)


def run_legs(be, case, new_context, seen=None):
    ctx = new_context(be)
    try:
        leg = M.Leg(be, ctx, *FILL_BASE)
        base = case.run(leg)
        case.check(leg, base)
    finally:
        ctx.close()
    for name in V.LEGS:
        ctx = new_context(be)
        try:
            leg = V.ViewLeg(be, ctx, *FILL_A, leg=name)
            outs = case.run(leg)
            assert leg.views, f"{case.id} [{name}]: the case made no device buffer through the leg: it ran vacuously"
            if seen is not None:
                seen[name] = [(v.role, v.shift, v.address % 16) for v in leg.views]
            hold_views(case, leg, outs, base)
        finally:
            ctx.close()


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.id)
def test_buffer_views(backend, monkeypatch, case):
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    seen = SEEN.setdefault((backend.name, case.id), {})
    run_legs(backend, case, fresh_context, seen)


def test_no_case_runs_vacuously(emu_backend, monkeypatch):
    """Every case hands out at least one view on every leg, every view sits on the residue its leg means, and the table as a
    whole reaches 4, 8 and 12 mod 16 for inputs and 4 and 8 for outputs (their shifts are one and two elements).  (Cases that test_buffer_views did not run in this session
    are run here.)"""
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    reached = {"input": set(), "output": set()}
    for case in M.CASES:
        seen = SEEN.get(("emu", case.id)) or SEEN.get(("gpu", case.id))
        if not seen or set(seen) != set(V.LEGS):
            seen = {}
            run_legs(emu_backend, case, fresh_context, seen)
        for name in V.LEGS:
            assert seen[name], (case.id, name)
            for role, shift, residue in seen[name]:
                assert residue == shift % 16, (case.id, name, role, shift, residue)
                reached[role].add(residue)
            if name == "bands":
                assert all(r == 0 for _, _, r in seen[name]), (case.id, seen[name])
        for name in ("all", "quad"):
            assert any(r != 0 for _, _, r in seen[name]), f"{case.id} [{name}]: every buffer stayed on 16 bytes"
    assert reached["input"] >= {0, 4, 8, 12} and reached["output"] >= {0, 4, 8}, reached


# --------------------------------------------------------------------------------------
# the plumbing, held without a GPU: a fake operation in numpy with a planted fault must be caught by the matching assertion


class _FakeCtx:
    def sync(self):
        pass

    def close(self):
        pass


class _FakeBackend:
    name, lib, ctx = "emu", None, _FakeCtx()

    def dev(self, a):
        return np.ascontiguousarray(a).copy()

    def garbage(self, shape, dtype, pattern):
        return M.host_garbage(shape, dtype, pattern)


_X = np.arange(1.0, 38.0, dtype=np.float32)
_X[17] = 0.0            # (the unwritten element's right value is the base leg's fill: only the garbage-filled legs can tell)


def _fake_case(fault):
    """out = 2 x in plain numpy, through the leg's buffers, with one planted fault on the view legs."""
    def run(leg):
        x, out = leg.dev(_X), leg.empty(_X.shape)
        keep = out[17].copy()
        out[...] = 2.0 * x
        if not isinstance(leg, V.ViewLeg):
            return {"out": leg.host(out)}
        vin, vout = leg.views[-2], leg.views[-1]
        end = vout.off + vout.nbytes
        if fault == "one element past the output":
            vout.alloc[end:end + 4] = 0
        elif fault == "one element in front of the output":
            vout.alloc[vout.off - 4:vout.off] = 0
        elif fault == "4095 bytes past the output":
            vout.alloc[end + 4094] = 0
        elif fault == "one input byte altered":
            vin.alloc[vin.off + 5] ^= 1
        elif fault == "one output element unwritten":
            out[17] = keep
        elif fault == "the sum follows the alignment" and vin.shift:
            out[3] = np.nextafter(out[3], np.float32(1e9))
        return {"out": leg.host(out)}

    def check(leg, outs):
        np.testing.assert_allclose(outs["out"], 2.0 * _X, rtol=1e-6)

    return M.Case(id="fake-" + fault.replace(" ", "-"), fns=("pp_fake",), run=run, check=check, nvox=_X.size)


FAULTS = {"one element past the output": r"0 in front .*, 4 behind \(first at \[0, 1, 2, 3\] bytes past the end",
          "one element in front of the output": r"4 in front \(first at \[-4, -3, -2, -1\] bytes from the data\), 0 behind",
          "4095 bytes past the output": r"first at \[4094\] bytes past the end",
          "one input byte altered": "an input buffer changed",
          "one output element unwritten": "Not equal to tolerance|nan",
          "the sum follows the alignment": "differs from the base leg in 1 of 37 elements"}


def test_clean_fake_operation_passes_every_leg():
    seen = {}
    run_legs(_FakeBackend(), _fake_case("none"), lambda be: _FakeCtx(), seen)
    assert set(seen) == set(V.LEGS) and all(len(v) == 2 for v in seen.values())
    assert seen["all"] == [("input", 12, 12), ("output", 8, 8)] and seen["quad"] == [("input", 8, 8), ("output", 8, 8)]
    assert seen["in"] == [("input", 4, 4), ("output", 0, 0)] and seen["out"] == [("input", 0, 0), ("output", 4, 4)]


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_caught(fault):
    with pytest.raises(AssertionError, match=FAULTS[fault]):
        run_legs(_FakeBackend(), _fake_case(fault), lambda be: _FakeCtx())


def test_view_layout_and_required_alignment():
    """The layout of one view: base on 256 bytes, 4096 canary bytes on either side, the shift rounded up to align=."""
    leg = V.ViewLeg(_FakeBackend(), _FakeCtx(), *FILL_A, leg="all")
    a = leg.dev(np.arange(5, dtype=np.uint8))
    b = leg.empty((3,), np.int64)
    c = leg.empty((7,), np.uint8, align=8)
    d = leg.dev(np.zeros((2, 4), np.float32), align=16)
    va, vb, vc, vd = leg.views
    assert [v.shift for v in leg.views] == [3, 16, 8, 16] and [_lib.ptr(x) % 16 for x in (a, b, c, d)] == [3, 0, 8, 0]
    for v in leg.views:
        alloc = v.read_alloc()
        assert (v.address - v.shift) % 256 == 0 and v.off - v.shift >= V.BAND and alloc.size - (v.off + v.nbytes) >= V.BAND
        assert (alloc[:v.off] == V.CANARY).all() and (alloc[v.off + v.nbytes:] == V.CANARY).all()
    assert bytes(vc.data_bytes()) == bytes([0xA5]) * 7 and np.isnan(leg.empty((2,), np.float32)).all()
    assert V.shift_bytes("quad", "input", np.uint8) == 4 and V.shift_bytes("quad", "output", np.float32) == 8
    assert V.shift_bytes("out", "output", np.uint8, align=8) == 8 and V.shift_bytes("bands", "output", np.uint8, align=8) == 0
    assert not V.check_bands(leg) and not V.inputs_changed(leg) and V.outputs_untouched(leg)


# --------------------------------------------------------------------------------------
# the alignment requirements of the header: refused with PP_ERR_ARG, nothing touched, the context stays usable


def _legs(be, ctx, in_bytes=0, out_bytes=0):
    return (V.ViewLeg(be, ctx, *FILL_A, leg="aligned", shifts={"input": 0, "output": 0}),
            V.ViewLeg(be, ctx, *FILL_A, leg="off", shifts={"input": in_bytes, "output": out_bytes}))


def _refused(leg_off, legs, rc, names):
    assert rc == _lib.ERR_ARG, rc
    msg = leg_off.lib.pp_last_error(leg_off.ctx.h).decode()
    assert names in msg and "aligned" in msg, msg
    assert V.outputs_untouched(leg_off), "a refused call wrote to its output"
    for leg in legs:
        bad = V.check_bands(leg)
        assert not bad, V.bands_message("refused call", bad)
        assert not V.inputs_changed(leg)


@pytest.mark.parametrize("off", [1, 4])
def test_surface_stats_refuses_an_unaligned_record(backend, off):
    shape = (5, 9, 37)
    rng = np.random.default_rng(78)
    dist = rng.normal(scale=4.0, size=shape).astype(np.float32)
    sel = (rng.random(shape) < 0.6).astype(np.uint8)
    geom = _lib.make_geom(M.size_of(shape), (0.9, 1.1, 2.5))
    nbytes = _lib.SURFACE_STATS_DTYPE.itemsize
    ctx = fresh_context(backend)
    try:
        ok, bad = _legs(backend, ctx, out_bytes=off)
        dsel, ddist = ok.dev(sel), ok.dev(dist)
        rec = ok.empty((nbytes,), np.uint8)
        ctx.surface_stats(dsel, ddist, geom, _lib.SURFACE_LABEL_POS, rec, tau=1.25)
        base = ok.host(rec)
        assert base.view(_lib.SURFACE_STATS_DTYPE)[0]["count"] == int(sel.sum())
        rec_off = bad.empty((nbytes,), np.uint8)
        assert _lib.ptr(rec_off) % 8 == off
        rc = backend.lib.pp_surface_stats_f32(ctx.h, _lib.ptr(dsel), _lib.ptr(ddist), C.byref(geom), _lib.SURFACE_LABEL_POS, 1.25, None, _lib.ptr(rec_off))
        _refused(bad, (ok, bad), rc, "out")
        again = ok.empty((nbytes,), np.uint8)
        ctx.surface_stats(dsel, ddist, geom, _lib.SURFACE_LABEL_POS, again, tau=1.25)
        assert ok.host(again).tobytes() == base.tobytes()
        assert not V.check_bands(ok)
    finally:
        ctx.close()


def test_slice_masked_count_refuses_unaligned_counts(backend):
    shape = (5, 9, 37)
    a = (np.random.default_rng(79).random(shape) < 0.5).astype(np.uint8)
    ctx = fresh_context(backend)
    try:
        ok, bad = _legs(backend, ctx, out_bytes=4)
        da = ok.dev(a)
        out = ok.empty((shape[0],), np.int64)
        ctx.slice_masked_count(da, None, M.size_of(shape), out)
        base = ok.host(out)
        assert np.array_equal(base, (a != 0).sum(axis=(1, 2)))
        out_off = bad.empty((8 * shape[0],), np.uint8)          # int64 counts, one 4-byte word off
        assert _lib.ptr(out_off) % 8 == 4
        rc = backend.lib.pp_slice_masked_count_u8(ctx.h, _lib.ptr(da), None, _lib._i3(M.size_of(shape)), _lib.ptr(out_off))
        _refused(bad, (ok, bad), rc, "per_slice")
        again = ok.empty((shape[0],), np.int64)
        ctx.slice_masked_count(da, None, M.size_of(shape), again)
        assert ok.host(again).tobytes() == base.tobytes()
        assert not V.check_bands(ok)
    finally:
        ctx.close()


def test_packed_gradient_image_refuses_an_unaligned_image(backend):
    LM = M.T("linear_metric_kernels")
    key = "ragged"
    c = LM.CASES[key]
    _, Mv, _, _, GI, _ = LM.data(key)
    packed = np.ascontiguousarray(np.concatenate([np.moveaxis(GI, 0, -1), Mv[..., None]], axis=-1))
    ctx = fresh_context(backend)
    try:
        ok, bad = _legs(backend, ctx, in_bytes=4)
        a = LM.call_args(ok, key)
        dgi, dpk = ok.dev(GI), ok.dev(packed)
        try:
            ctx.set_moving_gradient(dgi, a["msize"], packed=dpk)
            base = LM.grad_calls(ok, a, c["Am"], c["bm"])
            ctx.set_moving_gradient(dgi, a["msize"])
            planar = LM.grad_calls(ok, a, c["Am"], c["bm"])
            dpk_off = bad.dev(packed)
            assert _lib.ptr(dpk_off) % 16 == 4
            rc = backend.lib.pp_linear_set_moving_gradient_packed(ctx.h, _lib.ptr(dpk_off))
            _refused(bad, (ok, bad), rc, "packed")
            after = LM.grad_calls(ok, a, c["Am"], c["bm"])      # the refusal installed nothing: the planar image is in force
            ctx.set_moving_gradient(dgi, a["msize"], packed=dpk)
            again = LM.grad_calls(ok, a, c["Am"], c["bm"])
        finally:
            ctx.set_moving_gradient(None)
        for k in base:
            assert after[k].tobytes() == planar[k].tobytes() and again[k].tobytes() == base[k].tobytes(), k
        assert not V.check_bands(ok) and not V.inputs_changed(ok)
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------
# fused demons: the field wants 16 bytes, the images nothing beyond their own 4


def _demons_pair(grid):
    Kt = M.T("kernels")
    from tests.helpers import phantom, random_dvf
    shape, spacing, origin = grid
    fix = phantom(shape, seed=40)
    dv = random_dvf(shape, spacing, seed=41, max_mm=2.5)
    mov = Kt.O.warp_image(Kt.O.Vol(fix, spacing, origin), dv.astype(np.float64), edge_value=-1000.0).arr.astype(np.float32)
    return fix, mov


def _execute(leg, grid, fix, mov, variant, iters=3):
    """-> (status, the field's buffer, statistics as a dict)"""
    Kt = M.T("kernels")
    shape, spacing, origin = grid
    p = Kt._demons_params(leg.ctx, iters, spacing, variant, max_rms=0.0)
    fld, st = leg.empty((3,) + shape), leg.hstruct(_lib.DemonsStats)
    rc = leg.lib.pp_demons_execute_f32(leg.ctx.h, _lib.ptr(leg.dev(fix)), _lib.ptr(leg.dev(mov)), C.byref(Kt.geom_of(shape, spacing, origin)),
                                       C.byref(p), _lib.ptr(fld), C.byref(st))
    return rc, fld, M.fields(st)


def _clean(what, *legs):
    for leg in legs:
        bad = V.check_bands(leg)
        assert not bad, V.bands_message(what, bad)
        changed = V.inputs_changed(leg)
        assert not changed, (what, [v.describe() for v in changed])


def test_fused_demons_refuses_a_field_off_16_bytes(backend, monkeypatch):
    Kt = M.T("kernels")
    grid = Kt.GRIDS[1]
    fix, mov = _demons_pair(grid)
    ctx = fresh_context(backend)
    try:
        ok, bad = _legs(backend, ctx, out_bytes=4)
        rc, fld, _ = _execute(bad, grid, fix, mov, _lib.DEMONS_FUSED)
        assert rc == _lib.ERR_UNSUPPORTED, rc
        msg = backend.lib.pp_last_error(ctx.h).decode()
        assert "fused demons needs field on a 16-byte boundary (got an address at 4 mod 16)" in msg and "radii" not in msg, msg
        assert V.outputs_untouched(bad), "the refused call wrote to the field"
        _clean("refused fused demons", bad)
        # a smoother that is off is still told apart
        p = Kt._demons_params(ctx, 3, grid[1], _lib.DEMONS_FUSED, max_rms=0.0)
        p.smooth_update = 0
        f2 = ok.empty((3,) + grid[0])
        rc = backend.lib.pp_demons_execute_f32(ctx.h, _lib.ptr(ok.dev(fix)), _lib.ptr(ok.dev(mov)), C.byref(Kt.geom_of(*grid)), C.byref(p), _lib.ptr(f2), None)
        assert rc == _lib.ERR_UNSUPPORTED and "both smoothers on" in backend.lib.pp_last_error(ctx.h).decode()
        assert V.outputs_untouched(ok)
        rc, f3, _ = _execute(ok, grid, fix, mov, _lib.DEMONS_FUSED)     # and the context goes on
        assert rc == 0 and np.abs(ok.host(f3)).max() > 0.1
        _clean("fused demons after the refusals", ok)
    finally:
        ctx.close()


@pytest.mark.parametrize("gname", ["grid1", "odd"])
def test_auto_demons_takes_the_staged_variant_for_a_field_off_16_bytes(backend, gname):
    Kt = M.T("kernels")
    grid = {"grid1": Kt.GRIDS[1], "odd": Kt.ODD}[gname]
    fix, mov = _demons_pair(grid)
    ctx = fresh_context(backend)
    try:
        ok, off = _legs(backend, ctx, out_bytes=4)
        rc, fld, st = _execute(ok, grid, fix, mov, _lib.DEMONS_STAGED)
        assert rc == 0
        staged = {"field": ok.host(fld), **st}
        ctx.profile_enable(True)
        rc, fld, st = _execute(ok, grid, fix, mov, _lib.DEMONS_AUTO)
        assert rc == 0 and "k_warp_same_grid" not in ctx.profile_read()        # (aligned: AUTO is the fused variant here)
        rc, fld, st = _execute(off, grid, fix, mov, _lib.DEMONS_AUTO)
        assert rc == 0 and _lib.ptr(fld) % 16 == 4
        names = {k for k, v in ctx.profile_read().items() if v[0] > 0}
        assert "k_warp_same_grid" in names and not any(k.startswith(("k_fused", "k_cube")) for k in names), names
        ctx.profile_enable(False)
        assert_same_bits({"field": off.host(fld), **st}, staged, f"AUTO with the field at 4 mod 16 against STAGED on aligned buffers ({gname})")
        _clean("auto demons", ok, off)
    finally:
        ctx.close()


SWITCHES = [("PP_FUSED_MASK", "0"), ("PP_FUSED_MASK", "1"), ("PP_FUSED_CUBE", "0"), ("PP_FUSED_CUBE", "1")]


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: f"{s[0][3:]}={s[1]}")
@pytest.mark.parametrize("gname", ["grid1", "odd"])
def test_fused_demons_takes_images_at_any_element(backend, monkeypatch, gname, switch):
    """PP_DEMONS_FUSED with an aligned field and fixed / moving 1, 2 and 3 elements into a larger buffer: the aligned fused
    bits, field and statistics, on grid1 (nx % 4 == 0: the caller's pointers reach the strip and pair loads directly) and on
    the odd grid, with the branchy and the MASK instances and with the marching kernels and the bricks."""
    Kt = M.T("kernels")
    grid = {"grid1": Kt.GRIDS[1], "odd": Kt.ODD}[gname]
    fix, mov = _demons_pair(grid)
    monkeypatch.setenv(*switch)
    ctx = fresh_context(backend)
    try:
        ctx.profile_enable(True)
        ok = V.ViewLeg(backend, ctx, *FILL_A, leg="aligned", shifts={"input": 0, "output": 0})
        rc, fld, st = _execute(ok, grid, fix, mov, _lib.DEMONS_FUSED)
        assert rc == 0
        base = {"field": ok.host(fld), **st}
        names = {k for k, v in ctx.profile_read().items() if v[0] > 0}
        assert any(k.startswith("k_cube") for k in names) == (switch == ("PP_FUSED_CUBE", "1")), names      # both grids allow the bricks
        assert np.abs(base["field"]).max() > 0.1
        _clean(f"fused demons ({gname}, aligned)", ok)
        for k in (1, 2, 3):
            leg = V.ViewLeg(backend, ctx, *FILL_A, leg=f"images+{k}", shifts={"input": 4 * k, "output": 0})
            rc, fld, st = _execute(leg, grid, fix, mov, _lib.DEMONS_FUSED)
            assert rc == 0, backend.lib.pp_last_error(ctx.h)
            assert {v.address % 16 for v in leg.views if v.role == "input"} == {4 * k}
            _clean(f"fused demons ({gname}, fixed and moving {k} elements in)", leg)
            assert_same_bits({"field": leg.host(fld), **st}, base, f"fused demons ({gname}, {switch}), fixed and moving {k} elements in")
            assert {k for k, v in ctx.profile_read().items() if v[0] > 0} == names
    finally:
        ctx.profile_enable(False)
        ctx.close()


# --------------------------------------------------------------------------------------
# the Python layer: every input image a one-element-shifted view inside a canaried allocation


class _ViewImages:
    """The hook of tests/test_memory_state.py's _path_* builders: how an input array becomes an Image.  Every array goes
    into a canaried allocation of the runtime's device, one element in, and the Image is made of that view."""

    def __init__(self, pa):
        import torch
        self.pa, self.torch, self.device = pa, torch, pa.runtime.default_device()
        self.made = []      # (alloc, off, nbytes, original bytes, address, tensor)

    def tensor(self, arr):
        t = self.torch
        arr = np.ascontiguousarray(arr)
        raw = arr.reshape(-1).view(np.uint8)
        shift = arr.dtype.itemsize
        alloc = t.full((256 + 2 * V.BAND + shift + raw.size,), V.CANARY, dtype=t.uint8, device=self.device)
        off = (-alloc.data_ptr()) % 256 + V.BAND + shift
        alloc[off:off + raw.size].copy_(t.from_numpy(raw.copy()))
        view = alloc[off:off + raw.size].view(t.from_numpy(arr[:0].reshape(-1)).dtype).reshape(arr.shape)
        assert view.data_ptr() == alloc.data_ptr() + off and view.data_ptr() % 16 == shift % 16 and view.is_contiguous()
        self.made.append((alloc, off, raw.size, raw.tobytes(), view.data_ptr(), view))
        return view

    def image_from_array(self, arr, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
        return self.pa.Image(self.tensor(arr), spacing, origin, is_vector=np.ndim(arr) == 4)

    def check(self, path):
        for alloc, off, n, orig, _, _ in self.made:
            a = alloc.cpu().numpy()
            assert (a[:off] == V.CANARY).all() and (a[off + n:] == V.CANARY).all(), (path, "bytes around an input image were overwritten")
            assert a[off:off + n].tobytes() == orig, (path, "an input image changed")


# Paths whose inputs do NOT reach the library as the view itself (the API copies them on the way in), with the place.  For
# these the run still has to give the plain bits with intact canaries, but it is no evidence about unaligned pointers.
COPIED_ON_THE_WAY_IN = {
    "get_external_mask": "platipy_amd/generation/mask.py:59: the thresholds are a torch expression on image.tensor; the library's first call "
                         "(the largest component) gets that expression's result, a fresh allocation",
}

# Results of a path that are arithmetic on the sums GROUPING_FOLLOWS_ALIGNMENT excuses: held to the path's own reference and
# bound (tests/test_comparison.py::check_surface_metrics) instead of to the plain run's bits.  Everything else: bits.
DERIVED_FROM_GROUPED_SUMS = {"compute_surface_metrics": ("meanSurfaceDistance", "sigmaSurfaceDistance")}


def _surface_metrics_by_reference(shifted):
    """-> the positions in the path's result vector that are excused, after holding them to the restatement"""
    from tests import comparison_restatement as CR
    TC = M.T("comparison")
    a, b = CR.blob_pair((20, 24, 28), 3)            # the images of test_memory_state._path_surface_metrics
    want, _ = CR.compute_surface_metrics(a, b, (0.9, 1.1, 2.5))
    keys = sorted(want)
    assert len(keys) == shifted[0].size
    where = [keys.index(k) for k in DERIVED_FROM_GROUPED_SUMS["compute_surface_metrics"]]
    for i in where:
        assert keys[i] in TC.DISTANCE_KEYS and TC.close(shifted[0][i], want[keys[i]]), (keys[i], shifted[0][i], want[keys[i]])
    return where


def _python_paths():
    from tests.test_memory_state import PYTHON_PATHS
    return PYTHON_PATHS


@pytest.mark.parametrize("path", list(_python_paths()))
def test_python_layer_on_offset_views(host_api, monkeypatch, path):
    """The public path once on ordinary images and once with every input image one element into a canaried allocation:
    identical bits, canaries intact, inputs unchanged -- and at the C ABI the library was handed the view's own address (the
    binding's ptr() is watched), so the run is evidence about the kernels and not about a copy."""
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    build = _python_paths()[path]
    plain = [np.array(x) for x in build(host_api)()]
    hook = _ViewImages(host_api)
    run = build(host_api, images=hook)
    assert hook.made, (path, "the builder made no input through the hook")
    passed = set()
    real_ptr = _lib.ptr

    def watching_ptr(x):
        p = real_ptr(x)
        passed.add(p)
        return p

    monkeypatch.setattr(_lib, "ptr", watching_ptr)
    shifted = [np.array(x) for x in run()]
    monkeypatch.setattr(_lib, "ptr", real_ptr)
    assert len(plain) == len(shifted)
    if path in DERIVED_FROM_GROUPED_SUMS:
        assert len(plain) == 1
        for i in _surface_metrics_by_reference(shifted):
            shifted[0][i] = plain[0][i]
    for k, (a, b) in enumerate(zip(plain, shifted)):
        assert a.shape == b.shape and a.dtype == b.dtype, (path, k)
        assert a.tobytes() == b.tobytes(), (path, k, int((a != b).sum()), "elements differ when the inputs are offset views")
    hook.check(path)
    for _, _, _, _, address, view in hook.made:
        assert view.data_ptr() == address
    reached = [m[4] in passed for m in hook.made]
    if path in COPIED_ON_THE_WAY_IN:
        assert not all(reached), (path, "every input reaches the library as the view: drop the path from COPIED_ON_THE_WAY_IN")
    else:
        assert all(reached), (path, reached, "an input image was copied before it reached the C ABI")
