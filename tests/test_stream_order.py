"""Every C-ABI operation, and the public Python paths, on a delayed non-blocking side stream (plumbing: tests/stream_order.py).

The kernel tests elsewhere run on torch's current stream, which in the test process is the legacy default stream; the product
runs every atlas chain on a non-blocking stream of its own (runtime.context, projects/multiatlas.py::_map_atlases).  On the
default stream a launch, memset or copy that goes to stream 0 instead of the context's stream, a host read that does not wait
for the context's stream, and a cached tensor published before its upload finished are all still ordered, by accident.  Here a
device spin of SPIN_MS milliseconds is queued in front of every call (a proxy library object does it), so that such a mistake
gives other bits every time instead of once in many runs.  Every case of tests/memory_state_cases.py runs three legs:

  base          as in tests/test_memory_state.py: fresh context on the default stream, held to the case's reference
  delayed       fresh context on a fresh side stream, the spin on THAT stream: the call's device work sits behind it, so
                whatever the library issued to another stream, and any host read that does not wait, comes too early
  busy default  the same, the spin on the LEGACY DEFAULT stream: whatever the library sent there by mistake comes too late
                while the side stream goes ahead (a first-in-chain zero fill or table upload, which the delayed leg cannot see)

The two side legs must equal the base leg BIT FOR BIT, outputs and returned statistics (the promise REFERENCE_BOUND_ONLY of
tests/test_memory_state.py records: it is empty).  Each side leg runs its case twice, on the fresh context and again after
another family's work went over the scratch (side_leg says why: a growing scratch waits for the stream).  Each side stream first passes a positive control on a buffer of the test's
own (stream_order.independent) when it is chosen, and again in front of every leg that uses it: streams that share a hardware
queue are serialised and would show nothing, and then the test fails and says so.  PP_POISON_WS stays unset: a stale read is meant to meet old data, not 0xFF bytes used as indices.

The CPU emulation has no streams; the unmarked tests here hold the plumbing (proxy, dealing, tables) and pp_set_stream's status.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from platipy_amd import _lib
from tests import memory_state_cases as M
from tests import stream_order as SO
from tests import test_memory_projection  # noqa: F401  (puts the projection cases into M.CASES)
from tests.test_memory_state import EXEMPT, FILL_A, FILL_BASE, PYTHON_PATHS, REFERENCE_BOUND_ONLY, assert_same_bits, dirty, fresh_context

CASES = list(M.CASES)
BY_ID = {c.id: c for c in CASES}
NO_SPIN = frozenset(set(EXEMPT) - {"pp_demons_history"})       # host-only entry points: nothing of theirs could be delayed
WORKERS = 3                                                     # with the default stream: the four hardware queues of a process

# Cases whose side legs deviate from the base leg and whose cause could not be read from the code: id -> the evidence.  Such a
# case is still held to its reference on every leg.  At most three, none from the demons, smooth and resample families.
DEVIATES = {}

_BASE = {}          # (backend, case id) -> outputs of the base leg (checked against the reference once)
_SCRATCH = {}       # (backend, case id) -> bytes of scratch the base leg's context ended with
_RIG = []


class Rig:
    """The spin and the controlled side streams, made once per module."""

    def __init__(self, be):
        self.spin = SO.Spin(be.torch)
        self.streams = SO.SideStreams(be.torch, self.spin)


def rig_of(be):
    if not _RIG:
        _RIG.append(Rig(be))
    return _RIG[0]


def base_of(be, case):
    if (be.name, case.id) not in _BASE:
        ctx = fresh_context(be)
        try:
            leg = M.Leg(be, ctx, *FILL_BASE)
            outs = case.run(leg)
            case.check(leg, outs)
            _SCRATCH[be.name, case.id] = ctx.workspace_bytes()
        finally:
            ctx.close()
        _BASE[be.name, case.id] = outs
    return _BASE[be.name, case.id]


def side_context(be, spin, side, late):
    """(proxy, context): a fresh context bound to `side` whose every call is preceded by the spin on `late` (while the proxy is
    `armed`)."""
    proxy = SO.SpinProxy(be.lib, lambda: spin.on(late), NO_SPIN)
    return proxy, _lib.Context(0, side.cuda_stream, lib=proxy)


def grow_scratch(be, ctx, need_bytes):
    """A distance map (17 bytes of scratch per voxel) large enough to leave the context with `need_bytes` of scratch."""
    if need_bytes <= 0:
        return
    nz = max(int(np.ceil((need_bytes / 17.0 / 6.0) ** (1.0 / 3.0))) + 1, 2)
    shape = (nz, 2 * nz, 3 * nz)
    m = be.dev((np.random.default_rng(nz).random(shape) < 0.4).astype(np.uint8))
    ctx.distance_map(m, _lib.make_geom(M.size_of(shape)), be.garbage(shape, np.float32, 7.0), signed=True)
    ctx.sync()
    assert ctx.workspace_bytes() >= need_bytes, (ctx.workspace_bytes(), need_bytes)


def scribble(be, ctx):
    """A distance map over (nearly) all the scratch the context has, without growing it: other data where the last call left its own."""
    have = ctx.workspace_bytes()
    nz = int((have / 18.0 / 6.0) ** (1.0 / 3.0)) - 1
    if nz < 2:
        return
    shape = (nz, 2 * nz, 3 * nz)
    m = be.dev((np.random.default_rng(nz).random(shape) < 0.4).astype(np.uint8))
    ctx.distance_map(m, _lib.make_geom(M.size_of(shape)), be.garbage(shape, np.float32, 7.0), signed=True)
    ctx.sync()
    assert ctx.workspace_bytes() == have, (ctx.workspace_bytes(), have)


def side_leg(be, spin, side, late, cases, passes=1, scratch=0):
    """The cases, one after the other, inside `with torch.cuda.stream(side)` on one fresh context that was first left with
    `scratch` bytes of scratch: uploads, output buffers (filled with 0xFF / 0xA5 bytes on that stream) and read-backs are on the
    side stream too.  -> {case id: [outputs of every pass]}, proxy.

    passes=2 runs each case a second time after the dirtier of tests/test_memory_state.py (unrelated work of another family,
    not delayed) went over the context.  A context's FIRST call at a size grows its scratch, and pp_reserve waits for the
    context's stream before it does (the staging buffer and the mailbox are allocated once, too): the wait lets the spin run
    out before anything is launched, so on a fresh context a mis-ordering shows only behind the first allocation.  The second
    pass allocates nothing, every launch of it is queued behind the spin -- and what a link that runs early or late then
    finds in the scratch is the dirtier's data, not the first pass's own (equal) values."""
    torch = be.torch
    out = {}
    with torch.cuda.stream(side):
        proxy, ctx = side_context(be, spin, side, late)
        try:
            proxy.armed = False
            grow_scratch(be, ctx, scratch)
            for case in cases:
                proxy.forwarded.clear()
                out[case.id] = []
                for k in range(passes):
                    if k:
                        proxy.armed = False
                        dirty(be, ctx, case, ctx.workspace_bytes())
                    proxy.armed = True
                    leg = M.Leg(be, ctx, *FILL_A)
                    leg.lib = proxy
                    out[case.id].append(case.run(leg))
                    ctx.sync()
                missing = (set(case.fns) | set(case.setters)) - proxy.forwarded
                assert not missing, f"{case.id}: the proxy never saw {sorted(missing)}: the case reached the library around it"
        finally:
            ctx.close()
    return out, proxy


def hold(be, case, outs, what):
    if case.id in DEVIATES or set(case.fns) & set(REFERENCE_BOUND_ONLY):
        case.check(M.Leg(be, be.ctx, *FILL_BASE), outs)
    else:
        assert_same_bits(outs, _BASE[be.name, case.id], f"{case.id} [{what}]")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_stream_legs(gpu_backend, monkeypatch, case):
    """Measured on an MI355X: the spin takes 4.99 ms, the first three streams tried pass the control (the fourth shares the default
    stream's queue and fails it both ways round); with the final fold of pp_sum_sq_diff_f32 launched on stream 0 both side legs of
    the two sum-sq-diff cases fail (delayed on the second pass, busy default on both)."""
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    be, torch = gpu_backend, gpu_backend.torch
    rig = rig_of(be)
    base_of(be, case)
    torch.cuda.synchronize()
    side = rig.streams.get(1)[0]
    for what, late in (("delayed: the spin on the context's own stream", side),
                       ("busy default: the spin on the legacy default stream", torch.cuda.default_stream())):
        rig.streams.control(side, "side" if late is side else "default")
        outs, proxy = side_leg(be, rig.spin, side, late, [case], passes=2)
        torch.cuda.synchronize()
        assert proxy.spins >= 2 * len(set(case.fns) - NO_SPIN)
        hold(be, case, outs[case.id][0], what + ", first pass (the fresh context allocates)")
        hold(be, case, outs[case.id][1], what + ", second pass (after the dirtier, nothing is allocated)")


@pytest.mark.gpu
def test_neighbours_on_three_streams(gpu_backend, monkeypatch):
    """The whole table once, dealt by family to three worker threads (the pattern of _map_atlases: a `ready` event, the worker's
    stream waits for it, the work runs under that stream), each with its own controlled side stream, its own fresh context and
    the delayed proxy, so that the device work of the three overlaps: every output equals the base leg's bits.  One pass, on
    contexts that arrive with the largest scratch of the table (a growth waits for the stream: see side_leg)."""
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    be, torch = gpu_backend, gpu_backend.torch
    rig = rig_of(be)
    for case in CASES:
        base_of(be, case)
    torch.cuda.synchronize()
    streams = rig.streams.get(WORKERS)
    for st in streams:
        rig.streams.control(st, "side")
    hands = SO.deal(CASES, WORKERS)
    scratch = max(_SCRATCH[be.name, c.id] for c in CASES)
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream())

    def work(k):
        torch.cuda.set_device(0)
        s = streams[k]
        s.wait_event(ready)
        outs, _ = side_leg(be, rig.spin, s, s, hands[k], scratch=scratch)
        s.synchronize()
        return outs

    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        futures = [ex.submit(work, k) for k in range(WORKERS)]
        results = [f.result() for f in futures]
    torch.cuda.synchronize()
    assert sorted(i for r in results for i in r) == sorted(BY_ID)
    for k, r in enumerate(results):
        for cid, outs in r.items():
            hold(be, BY_ID[cid], outs[0], f"neighbours, worker {k}")


# --------------------------------------------------------------------------------------
# the Python layer: runtime.context() of the side stream is a context built on the proxy

_PLAIN = {}         # path -> (run, results of the plain run on the default stream)


def plain_of(pa, torch, path):
    if path not in _PLAIN:
        run = PYTHON_PATHS[path](pa)
        res = [np.array(x) for x in run()]
        torch.cuda.synchronize()
        _PLAIN[path] = (run, res)
    return _PLAIN[path]


def python_leg(be, spin, side, late, run):
    """The path twice under `side` with the proxy's context behind runtime.context(): on the fresh context, and again after a
    distance map (not delayed) went over the scratch the first run left (why: see side_leg).  -> the results of both."""
    from platipy_amd import runtime

    torch = be.torch
    idx = torch.cuda.current_device()
    key = (idx, side.cuda_stream)
    proxy = SO.SpinProxy(_lib.dll(), lambda: spin.on(late), NO_SPIN)
    with torch.cuda.stream(side):
        ctx = _lib.Context(idx, side.cuda_stream, lib=proxy)
        with runtime._LOCK:
            before = runtime._CTX.pop(key, None)
            runtime._CTX[key] = ctx
        try:
            assert runtime.context() is ctx
            res = [[np.array(x) for x in run()]]
            proxy.armed = False
            scribble(be, ctx)
            proxy.armed = True
            res.append([np.array(x) for x in run()])
            side.synchronize()
        finally:
            with runtime._LOCK:
                runtime._CTX.pop(key, None)
                if before is not None:
                    runtime._CTX[key] = before
            ctx.close()
    assert proxy.spins > 0, "the path never reached the library through the side stream's context"
    return res


def same_results(path, what, got, plain):
    assert len(got) == len(plain), (path, what)
    for k, (a, b) in enumerate(zip(plain, got)):
        assert a.shape == b.shape and a.dtype == b.dtype, (path, what, k)
        assert not (a.dtype.kind == "f" and (np.isnan(a).any() or np.isnan(b).any())), (path, what, k, "NaN in the result")
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(np.ravel(a != b))
            raise AssertionError(f"{path} [{what}]: result {k} differs from the plain run in {bad.size} of {a.size} elements, first at "
                                 f"{bad[:5].tolist()}: {np.ravel(b)[bad[:5]]} instead of {np.ravel(a)[bad[:5]]}")


def release_caches(torch):
    from platipy_amd.registration.linear import release_cached_jitter
    from platipy_amd.registration.utils import release_cached_masks

    torch.cuda.synchronize()
    release_cached_masks()
    release_cached_jitter()


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PYTHON_PATHS))
def test_python_layer_on_a_side_stream(gpu_backend, monkeypatch, path):
    """The public path plain on the default stream, then under a side stream: first with the spin on the default stream and the
    device caches warm from the plain run (the HIT arm: the cached tensor was uploaded on another stream), then with the spin on
    the side stream after the caches were dropped (the MISS arm: the entry is uploaded on the side stream).  Each leg runs the
    path twice (python_leg).  Bit-identical."""
    import platipy_amd as pa

    monkeypatch.delenv("PP_POISON_WS", raising=False)
    torch = gpu_backend.torch
    rig = rig_of(gpu_backend)
    run, plain = plain_of(pa, torch, path)
    side = rig.streams.get(1)[0]
    try:
        # (the plain result may come from the module's cache and every test here drops the device caches when it ends: the
        # hit arm needs entries uploaded on the default stream NOW)
        same_results(path, "plain run again, warming the caches", [np.array(x) for x in run()], plain)
        torch.cuda.synchronize()
        rig.streams.control(side, "default")
        got = python_leg(gpu_backend, rig.spin, side, torch.cuda.default_stream(), run)
        same_results(path, "busy default, warm caches, first run", got[0], plain)
        same_results(path, "busy default, warm caches, second run", got[1], plain)
        release_caches(torch)
        rig.streams.control(side, "side")
        got = python_leg(gpu_backend, rig.spin, side, side, run)
        same_results(path, "delayed, caches dropped, first run", got[0], plain)
        same_results(path, "delayed, second run", got[1], plain)
    finally:
        release_caches(torch)      # (nothing allocated on the side stream stays in a cache)


NEIGHBOUR_PATHS = ("demons", "linear_registration", "combine_labels")


@pytest.mark.gpu
def test_python_layer_neighbours(gpu_backend, monkeypatch):
    """Three different public paths at once on three threads, each under its own controlled side stream with the delayed
    proxy behind runtime.context(): each equals its plain run bit for bit.  No repetition and no retry; as in every Python leg a
    thread runs its path twice (python_leg: on the fresh context, and after a distance map went over its scratch)."""
    import platipy_amd as pa

    monkeypatch.delenv("PP_POISON_WS", raising=False)
    torch = gpu_backend.torch
    rig = rig_of(gpu_backend)
    plain = {p: plain_of(pa, torch, p) for p in NEIGHBOUR_PATHS}
    streams = rig.streams.get(WORKERS)
    for st in streams:
        rig.streams.control(st, "side")
    release_caches(torch)
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream())

    def work(k):
        torch.cuda.set_device(0)
        s = streams[k]
        s.wait_event(ready)
        return python_leg(gpu_backend, rig.spin, s, s, plain[NEIGHBOUR_PATHS[k]][0])

    try:
        with ThreadPoolExecutor(max_workers=WORKERS) as ex:
            futures = [ex.submit(work, k) for k in range(WORKERS)]
            results = [f.result() for f in futures]
        for p, got in zip(NEIGHBOUR_PATHS, results):
            same_results(p, "neighbours, first run", got[0], plain[p][1])
            same_results(p, "neighbours, second run", got[1], plain[p][1])
    finally:
        release_caches(torch)


# --------------------------------------------------------------------------------------
# pp_set_stream with work in flight

SET_STREAM_SHAPE = (14, 29, 44)
SET_STREAM_NEXT = "sum-sq-diff-70001"       # another family (reduce), scratch smaller than the distance map's: the reuse arm


def _distance_inputs():
    mask = (np.random.default_rng(5).random(SET_STREAM_SHAPE) < 0.4).astype(np.uint8)
    return mask, _lib.make_geom(M.size_of(SET_STREAM_SHAPE), (0.9, 1.1, 2.5))


def test_set_stream_waits_for_the_old_stream(backend, monkeypatch):
    """A context's scratch, tickets and mailbox are shared by everything it queued, so pp_set_stream waits for the old stream
    before it binds the new one (include/platipy_amd.h).  No timing: on a context that has its scratch already, a 20 ms spin and
    a distance map (five volumes of scratch) are queued on stream A -- A.query() is false --, set_stream(B) follows at once, and
    when it returns A.query() is true; a reduction on B and the distance map then both equal the bits of a plain run.  The
    emulation has no streams: the status and a working context."""
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    be = backend
    mask, geom = _distance_inputs()
    nxt = BY_ID[SET_STREAM_NEXT]
    ctx = fresh_context(be)
    try:
        out = be.garbage(SET_STREAM_SHAPE, np.float32, 0)
        ctx.distance_map(be.dev(mask), geom, out, signed=True)
        ctx.sync()
        want = {"distance": np.array(be.host(out))}
    finally:
        ctx.close()
    want_next = base_of(be, nxt) if be.name == "gpu" else None
    if be.name == "emu":
        ctx = fresh_context(be)
        try:
            leg = M.Leg(be, ctx, *FILL_BASE)
            want_next = nxt.run(leg)
            nxt.check(leg, want_next)
            out = be.garbage(SET_STREAM_SHAPE, np.float32, 0xFF)
            ctx.distance_map(be.dev(mask), geom, out, signed=True)
            assert be.lib.pp_set_stream(ctx.h, C.c_void_p(0x10)) == _lib.PP_OK      # (a handle the emulation never follows)
            assert be.lib.pp_set_stream(ctx.h, C.c_void_p(0x10)) == _lib.PP_OK
            got_next = nxt.run(M.Leg(be, ctx, *FILL_A))
            ctx.set_stream(0)
            got = {"distance": np.array(out)}
            assert be.lib.pp_set_stream(None, None) == _lib.ERR_ARG
        finally:
            ctx.close()
        assert_same_bits(got, want, "distance map around set_stream")
        assert_same_bits(got_next, want_next, "a reduction after set_stream")
        return
    torch = be.torch
    rig = rig_of(be)
    a, b = rig.streams.get(2)
    torch.cuda.synchronize()
    ctx = _lib.Context(0, a.cuda_stream, lib=be.lib)
    try:
        with torch.cuda.stream(a):
            m, out = be.dev(mask), be.garbage(SET_STREAM_SHAPE, np.float32, 0xFF)
            # the context's first call at a size grows the scratch, and pp_reserve waits for the stream before it does: that
            # wait would let the spin run out before a kernel is launched.  So the distance map and the reduction run once
            # without a spin (scratch, staging buffer and tickets exist from then on) ...
            ctx.distance_map(m, geom, out, signed=True)
            nxt.run(M.Leg(be, ctx, *FILL_A))
            out.fill_(float("nan"))
            a.synchronize()
            have = ctx.workspace_bytes()
            # ... and the second distance map, which allocates nothing, really sits behind 20 ms of spin when it returns
            rig.spin.on(a, scale=4)
            ctx.distance_map(m, geom, out, signed=True)
            grown = ctx.workspace_bytes() != have
            queued = not a.query()
        ctx.set_stream(b.cuda_stream)
        drained = a.query()
        with torch.cuda.stream(b):
            got_next = nxt.run(M.Leg(be, ctx, *FILL_A))
            b.synchronize()
        a.synchronize()
        got = {"distance": out.cpu().numpy()}
        grown = grown or ctx.workspace_bytes() != have
    finally:
        torch.cuda.synchronize()
        ctx.close()
    assert not grown, "the calls around set_stream were meant to allocate nothing"
    assert queued, "the spin and the distance map were meant to be in flight on the old stream when set_stream was called"
    assert drained, "pp_set_stream returned while the old stream still held the context's work"
    assert_same_bits(got_next, want_next, "a reduction on the new stream")
    assert_same_bits(got, want, "the distance map queued on the old stream")


# --------------------------------------------------------------------------------------
# the plumbing, without a GPU


class FakeLib:
    """Records what reaches it; every pp_* function returns (name, arguments) -- pp_create and pp_sync a status."""

    version = 7

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        if not name.startswith("pp_"):
            raise AttributeError(name)

        def fn(*args, **kwargs):
            self.log.append(("call", name))
            if name == "pp_create":
                args[2]._obj.value = 0x1234
            return _lib.PP_OK if name in ("pp_create", "pp_sync", "pp_set_stream") else (name, args, kwargs)
        return fn


def test_no_spin_names_are_the_host_only_entry_points():
    assert NO_SPIN == set(EXEMPT) - {"pp_demons_history"} and "pp_demons_history" in EXEMPT
    assert NO_SPIN < set(_lib.EXPORTED_SYMBOLS)
    assert len(set(_lib.EXPORTED_SYMBOLS) - NO_SPIN) >= 64
    assert not REFERENCE_BOUND_ONLY


def test_proxy_forwards_spins_and_records():
    log = []
    proxy = SO.SpinProxy(FakeLib(log), lambda: log.append(("spin",)), NO_SPIN)
    for name in _lib.EXPORTED_SYMBOLS:
        if name in ("pp_create", "pp_sync", "pp_set_stream"):
            continue
        del log[:]
        assert getattr(proxy, name)(1, "two", k=3.0) == (name, (1, "two"), {"k": 3.0})
        assert log == ([("call", name)] if name in NO_SPIN else [("spin",), ("call", name)]), name      # the spin comes FIRST
    assert getattr(proxy, "pp_warp_f32") is getattr(proxy, "pp_warp_f32")
    assert proxy.forwarded == set(_lib.EXPORTED_SYMBOLS) - {"pp_create", "pp_sync", "pp_set_stream"}
    assert proxy.spins == len(proxy.forwarded - NO_SPIN)
    assert proxy.version == 7                       # not a pp_* name: the library's own attribute
    with pytest.raises(AttributeError):
        proxy.no_such_thing


def test_proxy_serves_as_the_library_of_a_context():
    log = []
    proxy = SO.SpinProxy(FakeLib(log), lambda: log.append(("spin",)), NO_SPIN)
    ctx = _lib.Context(0, 0, lib=proxy)
    assert ctx.lib is proxy and ctx.h.value == 0x1234
    ctx.sync()
    ctx.set_stream(0)
    assert ctx.workspace_bytes()[0] == "pp_workspace_bytes"
    ctx.h = None                                    # (nothing to destroy)
    assert log == [("call", "pp_create"), ("call", "pp_sync"), ("call", "pp_set_stream"), ("call", "pp_workspace_bytes")]
    assert proxy.spins == 0 and proxy.forwarded == {"pp_create", "pp_sync", "pp_set_stream", "pp_workspace_bytes"}


@pytest.mark.parametrize("cid", ["fuse-divide", "sum-sq-diff-1027", "demons-execute-odd-fused-3"])
def test_cases_run_through_the_proxy_on_the_emulation(emu_backend, monkeypatch, cid):
    """What the gpu legs do, less the streams: Context(lib=proxy), leg.lib = proxy, raw calls and methods alike pass through it,
    with the bits of a run around it."""
    monkeypatch.delenv("PP_POISON_WS", raising=False)
    be, case = emu_backend, BY_ID[cid]
    spun = []
    proxy = SO.SpinProxy(be.lib, lambda: spun.append(1), NO_SPIN)
    ctx = _lib.Context(0, 0, lib=proxy)
    try:
        leg = M.Leg(be, ctx, *FILL_A)
        leg.lib = proxy
        outs = case.run(leg)
    finally:
        ctx.close()
    assert set(case.fns) | set(case.setters) <= proxy.forwarded
    assert {"pp_create", "pp_destroy"} <= proxy.forwarded
    assert len(spun) == proxy.spins >= len(set(case.fns) - NO_SPIN)
    ctx = fresh_context(be)
    try:
        plain = case.run(M.Leg(be, ctx, *FILL_BASE))
    finally:
        ctx.close()
    assert_same_bits(outs, plain, f"{cid} through the proxy")


def test_deal_mixes_the_families():
    hands = SO.deal(CASES, WORKERS)
    assert sorted(c.id for h in hands for c in h) == sorted(BY_ID)
    sizes = {}
    for c in CASES:
        sizes[c.family] = sizes.get(c.family, 0) + 1
    assert {"mask", "reduce", "demons", "smooth", "resample"} <= set(sizes)
    for h in hands:
        held = {c.family for c in h}
        assert {f for f, n in sizes.items() if n >= WORKERS} <= held
        assert max(len(x) for x in hands) - len(h) <= 1


def test_deviates_table_is_within_its_limits():
    assert len(DEVIATES) <= 3 and set(DEVIATES) <= set(BY_ID)
    assert not [i for i in DEVIATES if BY_ID[i].family in ("demons", "smooth", "resample")]
    assert all(isinstance(s, str) and len(s) > 40 for s in DEVIATES.values())
