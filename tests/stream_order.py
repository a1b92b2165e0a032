"""Plumbing of tests/test_stream_order.py: a proxy library object that queues a device spin in front of every C-ABI call, the
spin itself, the positive control that proves two streams are independent, and the choice of side streams.

The proxy and the dealing of cases need no GPU (tests/test_stream_order.py checks them against a fake library); everything
that touches torch.cuda imports it when called.
"""
import threading

SPIN_MS = 5.0                   # the delay in front of every call; the control, not the library, says whether it is long enough
STREAM_TRIES = 4                # streams are given hardware queues in turn and a process has four of them


class SpinProxy:
    """Stands where a ctypes library stands (`_lib.Context(lib=...)`, `leg.lib`, `_lib.gauss_taps(lib=...)`): every `pp_*`
    attribute is a callable that first calls `spin()` -- unless the name is in `no_spin`, the host-only entry points -- and
    then forwards to the real function, arguments and return value untouched.  `forwarded` holds the names it passed on,
    `spins` how often it queued a delay; while `armed` is false it only forwards (a test's own preparations on the context).
    Anything that is not a `pp_*` name is the real library's attribute."""

    def __init__(self, lib, spin, no_spin=()):
        self._lib, self._spin, self._no_spin = lib, spin, frozenset(no_spin)
        self.forwarded, self.spins, self.armed = set(), 0, True

    def __getattr__(self, name):                # (only names not found the ordinary way: the wrappers below are cached)
        real = getattr(self._lib, name)
        if not name.startswith("pp_"):
            return real
        delay = name not in self._no_spin

        def call(*args, **kwargs):
            if delay and self.armed:
                self._spin()
                self.spins += 1
            self.forwarded.add(name)
            return real(*args, **kwargs)

        call.__name__ = name
        self.__dict__[name] = call
        return call


def deal(cases, hands):
    """The cases dealt round-robin BY FAMILY into `hands` lists: ordered by family (the table's order within one), then card
    k goes to hand k % hands, so that every hand holds a share of every family with at least `hands` cases."""
    order = sorted(range(len(cases)), key=lambda i: (cases[i].family, i))
    return [[cases[i] for i in order[h::hands]] for h in range(hands)]


class Spin:
    """A device-side delay of about `ms` milliseconds that can be queued on any stream.  torch.cuda._sleep counts device
    clock cycles; one pair of events turns its unit into milliseconds.  Should it not scale (a second measurement at the
    computed count misses `ms` by more than a factor of two), the delay is a chain of fills of a 64 MiB buffer instead."""

    def __init__(self, torch, ms=SPIN_MS):
        self.torch, self.ms, self.cycles, self.fills, self._buf = torch, float(ms), None, None, None
        probe = 20_000_000
        torch.cuda._sleep(1000)                 # (loads the kernel)
        per_ms = probe / max(self._time(lambda: torch.cuda._sleep(probe)), 1e-6)
        cycles = int(per_ms * self.ms)
        self.measured_ms = self._time(lambda: torch.cuda._sleep(cycles))
        if 0.5 * self.ms <= self.measured_ms <= 2.0 * self.ms:
            self.cycles = cycles
            return
        self._buf = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        one = self._time(lambda: [self._buf.fill_(k) for k in range(16)]) / 16.0
        self.fills = max(int(self.ms / max(one, 1e-6)) + 1, 1)
        self.measured_ms = self._time(self._queue)

    def _time(self, queue):
        torch = self.torch
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        queue()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def _queue(self, scale=1):
        if self.cycles is not None:
            self.torch.cuda._sleep(self.cycles * scale)
        else:
            for k in range(self.fills * scale):
                self._buf.fill_(k & 1)

    def on(self, stream, scale=1):
        """Queue the delay (`scale` times as long) on `stream`; returns at once."""
        with self.torch.cuda.stream(stream):
            self._queue(scale)


def independent(torch, spin, side, late):
    """The positive control, a benign value race on a buffer of the test's own: the `late` stream ("side" or "default") gets the
    spin and then x.fill_(1), the other one y = x.clone().  Streams that run independently give y == 0 everywhere; streams that
    share a hardware queue are serialised and give 1 -- and so does a spin that is too short to hide the clone behind."""
    default = torch.cuda.default_stream()
    x = torch.zeros(4096, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    first, second = (side, default) if late == "side" else (default, side)
    spin.on(first)
    with torch.cuda.stream(first):
        x.fill_(1)
    with torch.cuda.stream(second):
        y = x.clone()
    first.synchronize()
    second.synchronize()
    torch.cuda.synchronize()
    return bool((y == 0).all().item())


class SideStreams:
    """Fresh non-blocking streams, each of which passed BOTH controls against the legacy default stream.  A stream that fails
    one is dropped (kept alive, so that the next one is another) and replaced, STREAM_TRIES times per stream asked for; if none
    shows independence the caller's test FAILS: nothing could be seen on serialised streams, and that is no library error."""

    def __init__(self, torch, spin):
        self.torch, self.spin, self.good, self.dropped, self._lock = torch, spin, [], [], threading.Lock()

    def get(self, n=1):
        with self._lock:
            tries = 0
            while len(self.good) < n and tries < STREAM_TRIES * n:
                tries += 1
                s = self.torch.cuda.Stream()
                assert s.cuda_stream != 0
                if independent(self.torch, self.spin, s, "side") and independent(self.torch, self.spin, s, "default"):
                    self.good.append(s)
                else:
                    self.dropped.append(s)
            if len(self.good) < n:
                raise AssertionError(
                    f"the positive control found {len(self.good)} of {n} side streams that run independently of the default stream "
                    f"({len(self.dropped)} tried and dropped, spin {self.spin.measured_ms:.2f} ms): the streams of this process are "
                    "serialised (shared hardware queues), so a mis-ordered launch could not be seen.  This is not an error of the library.")
            return self.good[:n]

    def control(self, stream, late):
        """The control of one leg, in front of it: `stream` was chosen by get() and the queues of a live stream do not change,
        but whether the spin still hides the other stream's work is looked at every time."""
        if not independent(self.torch, self.spin, stream, late):
            raise AssertionError(
                f"the positive control (spin on the {late} stream, {self.spin.measured_ms:.2f} ms) no longer shows this side stream to "
                "run independently of the default stream: the streams are serialised, or the spin is too short, so a mis-ordered "
                "launch could not be seen.  This is not an error of the library.")
