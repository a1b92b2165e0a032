"""Plumbing of tests/test_buffer_views.py: every device buffer of a case as a contiguous view inside a larger allocation.

A whole, fresh allocation starts on a 256-byte boundary and is followed by allocator slack, so a kernel that stores a quad
past the last voxel, or that takes a vector arm its base pointer does not allow, goes unnoticed.  Here every buffer is

    [allocation base, rounded up to 256 bytes] [4096 canary bytes] [shift: k whole elements of canary] [data] [4096 canary bytes]

with every byte of the allocation outside the data holding CANARY.  k is given per leg and per role (input: made by dev / p,
output: made by empty).  Shifts are whole elements -- exactly the addresses a sliced contiguous tensor can have; sub-element
misalignment and non-contiguous strides are out of scope.  A buffer created with align=A (a requirement the header states)
has its shift rounded up to a multiple of A bytes.
"""
import numpy as np

from platipy_amd import _lib
from tests import memory_state_cases as M

CANARY = 0xC3
BAND = 4096

# leg -> (input shift, output shift) in elements; None: the `quad` rule below
LEGS = {"bands": (0, 0), "in": (1, 0), "out": (0, 1), "all": (3, 2), "quad": None}


def shift_elements(leg, role, dtype):
    """The shift in whole elements.  quad: uint8 buffers land on 4 but not 16 bytes (the arm between the two predicates of
    the byte kernels), all others on 8 mod 16 where their element size allows."""
    if LEGS[leg] is None:
        return 4 if np.dtype(dtype) == np.uint8 else 2
    return LEGS[leg][0 if role == "input" else 1]


def shift_bytes(leg, role, dtype, align=None):
    b = shift_elements(leg, role, dtype) * np.dtype(dtype).itemsize
    if align and b % align:
        b += align - b % align
    return b


class View:
    """One buffer: `arr` is what the case sees, `alloc` the uint8 allocation around it, `off` the data's byte offset in it."""

    def __init__(self, arr, alloc, off, nbytes, role, shape, dtype, shift, orig):
        self.arr, self.alloc, self.off, self.nbytes, self.role = arr, alloc, off, nbytes, role
        self.shape, self.dtype, self.shift, self.orig = tuple(shape), np.dtype(dtype), shift, orig

    @property
    def address(self):
        return _lib.ptr(self.arr)

    def describe(self):
        return f"{self.role} buffer {self.shape} {self.dtype.name} at {self.address % 16} mod 16"

    def read_alloc(self):
        a = self.alloc
        return np.array(a.cpu().numpy() if hasattr(a, "cpu") else a)

    def data_bytes(self):
        return self.read_alloc()[self.off:self.off + self.nbytes].tobytes()


class ViewLeg(M.Leg):
    """M.Leg whose dev, p and empty hand out canaried offset views of the leg's backend."""

    def __init__(self, be, ctx, fpat, ipat, spat, leg="bands", shifts=None):
        super().__init__(be, ctx, fpat, ipat, spat)
        self.leg = leg
        self.shifts = shifts            # {role: bytes} instead of the leg's rule (the explicit tests)
        self.views = []

    # -- the allocation ----------------------------------------------------------------
    def _torch_dtype(self, dt):
        t = self.be.torch
        if dt.name == "uint32":         # as GpuBackend.garbage: no unsigned 32-bit tensors, the same bytes
            return t.int32
        return t.from_numpy(np.empty(0, dt)).dtype

    def _view(self, shape, dtype, role, fill, align=None):
        dt = np.dtype(dtype)
        shape = (shape,) if np.isscalar(shape) else tuple(int(s) for s in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        shift = self.shifts[role] if self.shifts is not None else shift_bytes(self.leg, role, dt, align)
        total = 256 + BAND + shift + nbytes + BAND
        if self.name == "gpu":
            alloc = self.be.torch.full((total,), CANARY, dtype=self.be.torch.uint8, device="cuda")
            base = alloc.data_ptr()
        else:
            alloc = np.full(total, CANARY, np.uint8)
            base = alloc.ctypes.data
        off = (-base) % 256 + BAND + shift
        fill = np.ascontiguousarray(fill).reshape(-1).view(np.uint8)
        assert fill.size == nbytes, (fill.size, nbytes)
        if self.name == "gpu":
            if nbytes:
                alloc[off:off + nbytes].copy_(self.be.torch.from_numpy(fill.copy()))
            arr = alloc[off:off + nbytes].view(self._torch_dtype(dt)).reshape(shape)
        else:
            alloc[off:off + nbytes] = fill
            arr = alloc[off:off + nbytes].view(dt).reshape(shape)
        v = View(arr, alloc, off, nbytes, role, shape, dt, shift, fill.tobytes())
        assert (base + off) % 256 == shift % 256 and v.address == base + off, (base, off, v.address)
        assert v.address % 16 == shift % 16, f"{v.describe()}: meant {shift % 16} mod 16"
        assert not align or v.address % align == 0, v.describe()
        self.views.append(v)
        return arr

    # -- what a case calls ---------------------------------------------------------------
    def dev(self, a, align=None):
        a = np.ascontiguousarray(a)
        return self._view(a.shape, a.dtype, "input", a, align)

    def p(self, a, align=None):
        self._keep.append(self.dev(a, align))
        return _lib.ptr(self._keep[-1])

    def empty(self, shape, dtype=np.float32, align=None):
        fill = M.host_garbage(shape, dtype, self._pattern(dtype))
        return self._view(fill.shape, dtype, "output", fill, align)


def check_bands(leg):
    """[(view, offsets)] for every buffer of the leg with changed canary bytes.  Offsets are relative to the data: negative in
    front of the first byte, from nbytes on behind the last."""
    if hasattr(leg.ctx, "sync"):
        leg.ctx.sync()
    bad = []
    for v in leg.views:
        a = v.read_alloc()
        keep = np.ones(a.size, bool)
        keep[v.off:v.off + v.nbytes] = False
        hit = np.flatnonzero(keep & (a != CANARY))
        if hit.size:
            bad.append((v, (hit - v.off).tolist()))
    return bad


def inputs_changed(leg):
    """The input views whose bytes are no longer the ones they were made with."""
    if hasattr(leg.ctx, "sync"):
        leg.ctx.sync()
    return [v for v in leg.views if v.role == "input" and v.data_bytes() != v.orig]


def outputs_untouched(leg):
    """True when every output view still holds its fill (a refused call)."""
    return all(v.data_bytes() == v.orig for v in leg.views if v.role == "output")


def bands_message(what, bad):
    lines = [f"{what}: bytes outside the buffer were overwritten"]
    for v, offs in bad:
        front = [o for o in offs if o < 0]
        rear = [o - v.nbytes for o in offs if o >= 0]
        lines.append(f"  {v.describe()}: {len(front)} in front (first at {front[-5:]} bytes from the data), "
                     f"{len(rear)} behind (first at {rear[:5]} bytes past the end)")
    return "\n".join(lines)
