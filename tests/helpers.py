"""Shared test plumbing: two ways to reach the kernels behind the C ABI, and synthetic volumes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from platipy_amd import _lib  # noqa: E402


class EmuBackend:
    """TEST ONLY: the kernel sources compiled for the CPU (tests/emu); buffers are numpy arrays."""

    name = "emu"

    def __init__(self):
        from tests.emu.build_emu import build

        self.lib = _lib.load(build())
        self.ctx = _lib.Context(0, 0, lib=self.lib)

    def dev(self, a):
        return np.ascontiguousarray(a).copy()

    def host(self, h):
        return np.asarray(h)

    def empty(self, shape, dtype=np.float32):
        return np.zeros(shape, dtype=dtype)

    def garbage(self, shape, dtype, pattern):
        return host_garbage(shape, dtype, pattern)


def host_garbage(shape, dtype, pattern):
    """A numpy buffer that holds what a call must overwrite.  pattern: an int 0 .. 255 puts it into every BYTE (0xFF is a NaN
    in every float type), a float into every ELEMENT."""
    dt = np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    if isinstance(pattern, (int, np.integer)):
        n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        return np.full(n, int(pattern), np.uint8).view(dt).reshape(shape)
    return np.full(shape, pattern, dtype=dt)


class GpuBackend:
    """The real libplatipy_hip.so on cuda:0; buffers are torch tensors."""

    name = "gpu"

    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need a GPU"
        self.torch = torch
        self.lib = _lib.dll()
        self.ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream, lib=self.lib)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def host(self, h):
        self.ctx.sync()
        return h.cpu().numpy()

    def empty(self, shape, dtype=np.float32):
        tdt = {np.float32: self.torch.float32, np.uint8: self.torch.uint8}[dtype]
        return self.torch.zeros(tuple(shape), dtype=tdt, device="cuda")

    def garbage(self, shape, dtype, pattern):
        """host_garbage on the device.  torch has no unsigned 32-bit tensors here: a uint32 buffer comes back as int32 (the
        same bytes; view it as uint32 on the host)."""
        t = self.torch
        dt = np.dtype(dtype)
        tdt = {"float32": t.float32, "float64": t.float64, "uint8": t.uint8, "int32": t.int32, "uint32": t.int32, "int64": t.int64}[dt.name]
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        if isinstance(pattern, (int, np.integer)):
            n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
            return t.full((n,), int(pattern), dtype=t.uint8, device="cuda").view(tdt).reshape(shape)
        return t.full(shape, pattern, dtype=tdt, device="cuda")


# --------------------------------------------------------------------------------------
# synthetic data (SURVEY 8d recipe, scaled down)


def smooth_noise(shape, seed, cells=6):
    """Smooth random scalar field: coarse N(0,1) noise, trilinearly up-sampled."""
    from scipy.ndimage import zoom

    rng = np.random.default_rng(seed)
    coarse = rng.normal(size=(cells, cells, cells))
    z = [s / cells for s in shape]
    out = zoom(coarse, z, order=1, mode="nearest", grid_mode=False)
    out = out[: shape[0], : shape[1], : shape[2]]
    pad = [(0, shape[i] - out.shape[i]) for i in range(3)]
    return np.pad(out, pad, mode="edge")


def phantom(shape, seed=1234, n_blobs=8, noise=5.0):
    """CT-like volume: -1000 background, 0 HU ellipsoid body, ellipsoidal organs, blur, noise."""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol = np.full(shape, -1000.0)
    body = ((xx - nx / 2) / (0.42 * nx)) ** 2 + ((yy - ny / 2) / (0.40 * ny)) ** 2 + ((zz - nz / 2) / (0.46 * nz)) ** 2 < 1
    vol[body] = 0.0
    for _ in range(n_blobs):
        c = [rng.uniform(0.25, 0.75) * s for s in (nx, ny, nz)]
        r = [rng.uniform(0.06, 0.2) * s for s in (nx, ny, nz)]
        val = rng.uniform(-200, 400)
        m = ((xx - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((zz - c[2]) / r[2]) ** 2 < 1
        vol[m & body] = val
    vol = gaussian_filter(vol, 1.5)
    if noise:
        vol = vol + np.random.default_rng(seed + 1).normal(0, noise, size=shape)
    return vol.astype(np.float32)


def random_dvf(shape, spacing, seed, max_mm=4.0, cells=5):
    f = np.stack([smooth_noise(shape, seed + c, cells) for c in range(3)])
    f *= max_mm / np.sqrt((f ** 2).sum(0)).max()
    return f.astype(np.float32)


def dice(a, b):
    a = a > 0
    b = b > 0
    return 2.0 * (a & b).sum() / max(1, a.sum() + b.sum())


def install_emu_runtime(setattr_fn=None):
    """TEST PLUMBING: point platipy_amd's context lookup at the CPU-emulated kernels (tensors stay on the host).
    linear_registration evaluates the metric thousands of times; emulating each 256-thread reduction launch
    thread-by-thread is too slow for the CPU suite, so here (only) the metric evaluation is the oracle's vectorised
    restatement -- the kernel itself is compared with it in tests/test_linear.py::test_meansq_kernel_*.
    `setattr_fn(obj, name, value)` defaults to plain setattr (used by spawned worker processes)."""
    import torch

    from oracle import linear_oracle
    from platipy_amd import runtime

    be = EmuBackend()
    sa = setattr_fn or setattr
    sa(runtime, "context", lambda device=None: be.ctx)
    sa(runtime, "default_device", lambda: torch.device("cpu"))

    def jit():      # the jitter array the host code set on the context (linear_registration(itk_sampling=True)), or None
        t = getattr(be.ctx, "_sample_jitter", None)
        return None if t is None else (t.numpy() if hasattr(t, "numpy") else np.asarray(t))

    def mgrad():    # ... and the filtered gradient image, or None
        t = getattr(be.ctx, "_moving_gradient", None)
        return None if t is None else (t.numpy() if hasattr(t, "numpy") else np.asarray(t))

    def fake_meansq(fixed, fsize, moving, msize, Af, bf, Am, bm, vsize, stride, fixed_mask=None, moving_mask=None):
        tn = lambda t: None if t is None else t.numpy()  # noqa: E731
        return list(linear_oracle.meansq_affine(fixed.numpy(), moving.numpy(), Af, bf, Am, bm, vsize, stride, tn(fixed_mask),
                                                tn(moving_mask), jitter=jit(), moving_gradient=mgrad()))

    def fake_corr(fixed, fsize, moving, msize, Af, bf, Am, bm, vsize, stride, fixed_mask=None, moving_mask=None):
        tn = lambda t: None if t is None else t.numpy()  # noqa: E731
        return list(linear_oracle.corr_moments_affine(fixed.numpy(), moving.numpy(), Af, bf, Am, bm, vsize, stride, tn(fixed_mask),
                                                      tn(moving_mask), jitter=jit(), moving_gradient=mgrad()))

    def fake_values(metric, fixed, fsize, moving, msize, Af, bf, Ams, bms, vsize, stride, fixed_mask=None, moving_mask=None):
        out = np.zeros((len(Ams), 6))
        for c, (Am, bm) in enumerate(zip(Ams, bms)):
            r = (fake_meansq if metric == 0 else fake_corr)(fixed, fsize, moving, msize, Af, bf, np.asarray(Am).ravel(), bm, vsize, stride,
                                                            fixed_mask, moving_mask)
            out[c, :2 if metric == 0 else 6] = r[:2 if metric == 0 else 6]
        return out

    from platipy_amd.registration import linear as _linear

    sa(_linear, "NATIVE_OPTIMISER", False)        # the native loop would run every probe through the emulated kernels
    sa(_linear, "LINE_SEARCH_SPECULATION", 1)     # sequential probes: the numpy stand-in gains nothing from batching
    sa(be.ctx, "metric_values_affine", fake_values)
    sa(be.ctx, "meansq_affine", fake_meansq)
    sa(be.ctx, "corr_moments_affine", fake_corr)
    return be


def sphere_case(i, shape=(30, 64, 64)):
    """The reference's synthetic cardiac case i (platipy/imaging/tests/test_cardiac.py:43-71) at half size:
    a -1000 volume holding a sphere of value 1, its mask, a small sub-structure, slightly different spacing."""
    nz, ny, nx = shape
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    m = (zz - (nz // 2 + i)) ** 2 + (yy - (ny // 2 + i)) ** 2 + (xx - nx // 2) ** 2 <= (nx * 25 // 128) ** 2
    sub = (zz - (nz // 2 + i)) ** 2 + (yy - (ny // 2 - 2 + i)) ** 2 + (xx - (nx // 2 - 2)) ** 2 <= (nx * 5 // 128 + 1) ** 2
    ct = np.where(m, 1.0, -1000.0).astype(np.float32)
    return ct, m.astype(np.uint8), sub.astype(np.uint8), (0.9 + i * 0.01, 0.9 + i * 0.01, 2.5 + i * 0.01)


def record_stats(name, stats):
    """Keep a test's MEASURED error statistics: one JSON per test under
    $PP_STATS_DIR (default gpurun_out/parity_stats/, which gpurun merges back); the builder commits the collected
    file under profiles/.  Never fails a test."""
    import json

    d = os.environ.get("PP_STATS_DIR", os.path.join(ROOT, "gpurun_out", "parity_stats"))
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".json"), "w") as fh:
            json.dump(stats, fh, indent=1, sort_keys=True, default=float)
    except OSError:
        pass


# --------------------------------------------------------------------------------------
# adversarial binary volumes for the mask post-processing kernels (tests/test_mask_kernels.py); all [Z][Y][X] uint8


def serpentine(shape):
    """A one-voxel-wide snake: full x-rows at every other y, joined by single voxels at alternating x ends; the same
    pattern on every other z, the planes joined by single voxels alternately at the pattern's end and at its start.  One
    face-connected component whose last voxel is (rows x nx) voxels along the path from voxel 0."""
    nz, ny, nx = shape
    plane = np.zeros((ny, nx), np.uint8)
    plane[0::2, :] = 1
    for k, y in enumerate(range(1, ny - 1, 2)):
        plane[y, nx - 1 if k % 2 == 0 else 0] = 1
    last_row = (ny - 1) // 2 * 2
    end = (last_row, 0 if (last_row // 2) % 2 else nx - 1)     # where the path that starts at (0, 0) leaves the plane
    m = np.zeros(shape, np.uint8)
    m[0::2] = plane
    for k, z in enumerate(range(1, nz - 1, 2)):
        y, x = end if k % 2 == 0 else (0, 0)
        m[z, y, x] = 1
    return m


def checkerboard(shape):
    zz, yy, xx = np.indices(shape)
    return ((zz + yy + xx) % 2 == 0).astype(np.uint8)


def nested_shells(shape=(13, 14, 15), opening=None):
    """A hollow box (walls one voxel thick, one voxel inside the volume) holding a hollow box holding a solid.
    opening: None, or 'face' / 'edge' / 'corner': one wall voxel removed so that the outer cavity touches the outside
    across a face (no longer a hole), or only across an edge / a corner (still a hole under face connectivity)."""
    m = np.zeros(shape, np.uint8)
    for k, v in ((1, 1), (2, 0), (4, 1), (5, 0), (6, 1)):
        m[k:shape[0] - k, k:shape[1] - k, k:shape[2] - k] = v
    if opening == "face":
        m[1, shape[1] // 2, shape[2] // 2] = 0
    elif opening == "edge":
        m[1, 1, shape[2] // 2] = 0
    elif opening == "corner":
        m[1, 1, 1] = 0
    return m


def bernoulli(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def random_runs(shape, seed, lo=1, hi=5):
    """Every x-row alternates foreground and background runs of random length lo..hi, starting with either value."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    m = np.zeros((nz * ny, nx), np.uint8)
    for r in range(nz * ny):
        lens = rng.integers(lo, hi + 1, size=nx // lo + 1)
        vals = (np.arange(lens.size) + rng.integers(0, 2)) % 2
        m[r] = np.repeat(vals, lens)[:nx]
    return m.reshape(shape)


def boundary_rows(nx, rows, seed, span=8, pass_len=512):
    """[rows][nx] rows whose runs straddle the multiples of `span` and of `pass_len` in every way: one run over the whole
    row; period-3 and period-11 runs; random runs of 1..20; a run that starts in the first pass and ends in the last (the
    passes between hold no run start); runs of exactly span and pass_len voxels that start one voxel before / on / after
    each pass boundary; a single last voxel."""
    rng = np.random.default_rng(seed)
    x = np.arange(nx)
    pats = [np.ones(nx, np.uint8), ((x // 3) % 2).astype(np.uint8), (((x + 5) // 11) % 2 == 0).astype(np.uint8),
            random_runs((1, 1, nx), seed, 1, 20)[0, 0]]
    long_run = np.zeros(nx, np.uint8)
    long_run[min(3, nx - 1):max(nx - 2, 1)] = 1
    pats.append(long_run)
    edges = np.zeros(nx, np.uint8)
    for k, b in enumerate(range(pass_len, nx + pass_len, pass_len)):
        s = b - 1 + k % 3                      # one before, on, one after the boundary
        edges[s:s + span] = 1
        edges[max(b - pass_len // 2, 0):max(b - pass_len // 2 + 1, 0)] = 1
    pats.append(edges)
    last = np.zeros(nx, np.uint8)
    last[nx - 1] = 1
    pats.append(last)
    pats.append(1 - edges)
    out = np.stack([pats[(r + int(rng.integers(0, len(pats)))) % len(pats)] if r >= len(pats) else pats[r] for r in range(rows)])
    return out


# --------------------------------------------------------------------------------------
# geometry and displacement generators for the resampling kernels (tests/test_resample_kernels.py)

EPS6 = 2.0 ** -6


def rot_xyz(ax_deg, ay_deg, az_deg):
    """Proper rotation Rz Ry Rx (degrees about x, y, z)."""
    ax, ay, az = np.radians([ax_deg, ay_deg, az_deg])
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return rz @ ry @ rx


def direction_cases():
    """name -> 3 x 3 direction cosines: identity, a flip of x, the axis permutation (y, z, x) with one sign flipped, a
    proper rotation by 20 / -35 / 50 degrees about x / y / z, and that rotation times a flip (determinant -1)."""
    rot = rot_xyz(20.0, -35.0, 50.0)
    perm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])    # index x -> physical y, y -> -z, z -> x
    return {"identity": np.eye(3), "flipx": np.diag([-1.0, 1.0, 1.0]), "perm": perm, "rot": rot,
            "rotflip": rot @ np.diag([1.0, -1.0, 1.0])}


def border_targets(n):
    """The continuous indices on an axis of n voxels at which a border decision is taken, each with its two neighbours at
    2^-6: the buffer test's ends -0.5 and n - 0.5, the first and last index, and every nearest-neighbour tie k + 0.5."""
    t = [-0.5 - EPS6, -0.5, -0.5 + EPS6, -EPS6, 0.0]
    for k in range(max(n - 1, 1)):
        t += [k + 0.5 - EPS6, k + 0.5, k + 0.5 + EPS6]
    t += [n - 1 - EPS6, n - 1.0, n - 1 + EPS6, n - 0.5 - EPS6, n - 0.5, n - 0.5 + EPS6]
    return t


def border_probe_fields(shape, spacing, seed):
    """Displacement fields [3][Z][Y][X] (physical units, fp32, every value a multiple of 2^-7) on a grid of `shape` with dyadic
    `spacing` that put the samples of a same-grid gather exactly on border_targets: voxel i of pass p probes axis (i + p N) % 3
    with the next target of that axis while the other two axes land on multiples of 2^-6 inside [0, n - 1]; every fourth
    probe puts ALL three axes on a target (corners of the decision).  Consecutive voxels of a row probe different targets,
    so every row longer than the list holds all of them; shorter volumes get as many passes as it takes for every
    (axis, target) pair to occur."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    n = (nx, ny, nz)
    N = nx * ny * nz
    tg = [border_targets(k) for k in n]
    need = 3 * max(len(t) for t in tg)
    passes = max(1, -(-need // N))
    z, y, x = np.indices(shape)
    idx = (x, y, z)
    lin = (z * ny + y) * nx + x
    out = []
    for p in range(passes):
        q = lin + p * N
        axis = q % 3
        c = []
        for a in range(3):
            benign = rng.integers(0, (n[a] - 1) * 64 + 1, size=shape) / 64.0
            probe = np.asarray(tg[a])[(q // 3 + (a * 5)) % len(tg[a])]
            c.append(np.where((axis == a) | (q % 4 == 3), probe, benign))
        f = np.stack([(c[a] - idx[a]) * spacing[a] for a in range(3)])
        assert np.array_equal(f, f.astype(np.float32).astype(np.float64))
        out.append(f.astype(np.float32))
    return out


def hostile_displacements(spacing_axis):
    """Physical displacements no volume survives: NaN, +-Inf, +-1e30, +-3e6 voxels, +-(2^23 + 1) voxels."""
    s = float(spacing_axis)
    vox = [3.0e6, -3.0e6, 2.0 ** 23 + 1, -(2.0 ** 23 + 1)]
    return np.array([np.nan, np.inf, -np.inf, 1e30, -1e30] + [v * s for v in vox], dtype=np.float32)
