"""Masks to RTSTRUCT contours -- pp_contour_trace_u8 (csrc/pp_contour_trace.h) and platipy_amd.dicom.extract_contours --
against tests/contour_trace_restatement.py (T1-T7 walked sequentially in plain Python, holes decided by the sign of the
enclosed area) and against the round trip through pp_contour_fill_u8, which rests on neither.

Bounds: none.  Everything is integer; every comparison is np.array_equal or equality of lists.  Physical points are held to
their slice's plane to 1e-9 mm: |coordinate| < 1e3 mm here, three fp64 products and sums give an error below 1e-12 mm.

A case's extraction is made once per backend and shared by the tests that look at it."""
import ctypes as C

import numpy as np
import pytest
import torch

from platipy_amd import _lib
from tests import contour_restatement as F
from tests import contour_trace_restatement as T

DENSITIES = (0.1, 0.3, 0.5, 0.7, 0.9)


# --------------------------------------------------------------------------------------
# masks, all uint8 [S][Z][Y][X]


def noise(ny, nx, seed):
    """3 structures x 4 slices: structure 1 and slice 2 are empty, the others cycle through the five densities."""
    rng = np.random.default_rng(seed)
    m = np.zeros((3, 4, ny, nx), np.uint8)
    k = 0
    for s in (0, 2):
        for z in (0, 1, 3):
            m[s, z] = (rng.random((ny, nx)) < DENSITIES[k % 5]) * (1 if k % 2 else 255)      # any non-zero byte is foreground
            k += 1
    return m


def spiral(n):
    """A square spiral one pixel wide, arms two pixels apart, from the corner inwards: one loop around all of it."""
    m = np.zeros((n, n), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    while True:
        moved = False
        while True:
            ax, ay, bx, by = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if not (0 <= ax < n and 0 <= ay < n) or m[ay, ax] or (0 <= bx < n and 0 <= by < n and m[by, bx]):
                break
            x, y, moved = ax, ay, True
            m[y, x] = 1
        if not moved:
            return m
        dx, dy = -dy, dx


def specials():
    ny, nx = 9, 11
    yy, xx = np.indices((ny, nx))
    rings = np.zeros((ny, nx), np.uint8)
    rings[0:9, 1:10] = 1
    rings[1:8, 2:9] = 0
    rings[2:7, 3:8] = 1
    rings[3:6, 4:7] = 0
    rings[4, 5] = 1
    diag = ((xx == yy) | (xx + yy == 10)).astype(np.uint8)                    # two diagonal chains that cross
    chain = ((xx - yy) % 4 == 0).astype(np.uint8)                             # parallel diagonal chains into every edge
    frame = np.ones((ny, nx), np.uint8)
    frame[1:-1, 1:-1] = 0
    cross = ((xx == 5) | (yy == 4)).astype(np.uint8)                          # touches all four edges, one pixel wide
    planes = [((yy + xx) % 2 == 0), ((yy + xx) % 2 == 1), np.ones((ny, nx)), np.zeros((ny, nx)), rings, diag, chain, frame, cross]
    return np.stack([np.asarray(p, np.uint8) for p in planes])[:, None]      # 9 structures x 1 slice


def long_loops():
    sp = spiral(96)
    inner = np.ones((98, 98), np.uint8)
    inner[1:-1, 1:-1] = 1 - sp      # the spiral as background inside a filled square: one long hole loop
    outer = np.zeros((98, 98), np.uint8)
    outer[1:-1, 1:-1] = sp
    return np.stack([outer, inner])[:, None]


CASES = {f"noise-{ny}x{nx}": (lambda ny=ny, nx=nx: noise(ny, nx, 100 * ny + nx)) for ny in range(1, 15) for nx in range(1, 15)}
CASES["specials-9x11"] = specials
CASES["zeros"] = lambda: np.zeros((2, 3, 5, 7), np.uint8)
CASES["noise-35x67"] = lambda: noise(35, 67, 7)
CASES["noise-3x200"] = lambda: noise(3, 200, 8)
CASES["runs-35x67"] = lambda: np.repeat(np.repeat(noise(7, 14, 9), 5, axis=2), 5, axis=3)[:, :, :, :67]      # thick blobs
CASES["spirals-98"] = long_loops
SMALL = [k for k in CASES if k.startswith("noise-") and k not in ("noise-35x67", "noise-3x200")]
GROUPS = {f"noise-ny{ny}": [k for k in SMALL if k.startswith(f"noise-{ny}x")] for ny in range(1, 15)}
GROUPS.update({k: [k] for k in CASES if k not in SMALL})

_masks, _traced, _wanted = {}, {}, {}


def masks_of(case):
    if case not in _masks:
        _masks[case] = np.ascontiguousarray(CASES[case]())
    return _masks[case]


def traced(backend, case, approximate):
    key = (backend.name, case, approximate)
    if key not in _traced:
        m = masks_of(case)
        s, nz, ny, nx = m.shape
        _traced[key] = backend.ctx.contour_trace(backend.dev(m), (nx, ny, nz), s, approximate, with_cracks=True)
    return _traced[key]


def wanted(case, approximate):
    if (case, approximate) not in _wanted:
        _wanted[(case, approximate)] = T.trace(masks_of(case), approximate)
    return _wanted[(case, approximate)]


def fill(backend, verts, rows, shape):
    s, nz, ny, nx = shape
    out = backend.dev(np.full(shape, 0xFF, np.uint8))
    backend.ctx.contour_fill(verts, rows, (nx, ny, nz), s, out)
    return backend.host(out)


def binary(m):
    return (m != 0).astype(np.uint8)


# --------------------------------------------------------------------------------------
# 1. the restatement


@pytest.mark.parametrize("approximate", [False, True], ids=["full", "approximate"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_equals_restatement(backend, group, approximate):
    for case in GROUPS[group]:
        verts, rows, hole, _ = traced(backend, case, approximate)
        wv, wr, wh = wanted(case, approximate)
        assert verts.dtype == np.int32 and rows.dtype == _lib.CONTOUR_DTYPE and hole.dtype == np.uint8
        assert [tuple(r) for r in rows.tolist()] == wr, case
        assert np.array_equal(verts, wv), case
        assert np.array_equal(hole, wh), case


def test_cases_decide_something(backend):
    """The long loops are long: one loop of more than 2^11 cracks (more than 10 doubling rounds, many workgroups) as an
    outer border, and one as a hole; the specials hold holes inside holes."""
    verts, rows, hole, cracks = traced(backend, "spirals-98", False)
    assert [tuple(r)[2:] for r in rows.tolist()] == [(0, 0), (1, 0), (1, 0)] and hole.tolist() == [0, 0, 1]
    assert rows["count"][0] > 2048 and rows["count"][2] > 2048 and cracks > 3 * 2048
    _, rows, hole, _ = traced(backend, "specials-9x11", False)
    assert hole[rows["structure"] == 4].tolist() == [0, 1, 0, 1, 0]      # ring, its hole, ring, its hole, the centre pixel
    assert traced(backend, "zeros", False)[3] == 0 and len(traced(backend, "zeros", False)[1]) == 0


# --------------------------------------------------------------------------------------
# 2. the round trip


@pytest.mark.parametrize("group", list(GROUPS))
def test_round_trip(backend, group):
    for case in GROUPS[group]:
        m = masks_of(case)
        verts, rows, _, _ = traced(backend, case, False)
        assert np.array_equal(fill(backend, verts, rows, m.shape), binary(m)), case
        s, nz, ny, nx = m.shape
        assert np.array_equal(F.fill(verts, rows.tolist(), (nx, ny, nz), s), binary(m)), case


# --------------------------------------------------------------------------------------
# 3. topology


@pytest.mark.parametrize("group", list(GROUPS))
def test_topology(backend, group):
    from scipy import ndimage

    for case in GROUPS[group]:
        m = masks_of(case)
        _, rows, hole, _ = traced(backend, case, False)
        for s in range(m.shape[0]):
            for z in range(m.shape[1]):
                here = (rows["structure"] == s) & (rows["z"] == z)
                _, components = ndimage.label(m[s, z] != 0, structure=np.ones((3, 3)))
                _, background = ndimage.label(np.pad(m[s, z], 1) == 0)      # 4-connected
                assert int((hole[here] == 0).sum()) == components, (case, s, z)
                assert int((hole[here] == 1).sum()) == background - 1, (case, s, z)


# --------------------------------------------------------------------------------------
# 4. determinism


@pytest.mark.parametrize("case", ["noise-35x67", "spirals-98"])
def test_two_calls_give_the_same_bytes(backend, case):
    m = masks_of(case)
    s, nz, ny, nx = m.shape
    for approximate in (False, True):
        a = backend.ctx.contour_trace(backend.dev(m), (nx, ny, nz), s, approximate)
        b = traced(backend, case, approximate)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# --------------------------------------------------------------------------------------
# 5. approximate contours


def on_segment(p, a, b):
    cross = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
    return cross == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


@pytest.mark.parametrize("group", list(GROUPS))
def test_approximate_drops_only_collinear_vertices(backend, group):
    dropped = 0
    for case in GROUPS[group]:
        fv, fr, fh, _ = traced(backend, case, False)
        av, ar, ah, _ = traced(backend, case, True)
        assert len(fr) == len(ar) and np.array_equal(fh, ah)
        assert np.array_equal(fr["structure"], ar["structure"]) and np.array_equal(fr["z"], ar["z"])
        for (f0, fn, _, _), (a0, an, _, _) in zip(fr.tolist(), ar.tolist()):
            full, kept = [tuple(v) for v in fv[f0:f0 + fn].tolist()], [tuple(v) for v in av[a0:a0 + an].tolist()]
            at, j = [], 0
            for k, v in enumerate(full):      # the kept vertices, in order, inside the full contour
                if j < len(kept) and v == kept[j]:
                    at.append(k)
                    j += 1
            assert j == len(kept), (case, full, kept)
            if fn <= 2:
                assert kept == full
            for k, v in enumerate(full):
                if k in at:
                    continue
                before = max([i for i in range(len(at)) if at[i] < k], default=len(at) - 1)      # cyclic neighbours
                assert on_segment(v, kept[before], kept[(before + 1) % len(kept)]), (case, full, kept, k)
                dropped += 1
    print(group, "dropped vertices:", dropped)


def thick_slices():
    """300 seeded 24 x 28 slices of box-dilated seeds; kept: those where, padded by 2, the mask and its complement are their
    own 2 x 2 openings (no part of either is one pixel wide)."""
    from scipy import ndimage

    rng = np.random.default_rng(2024)
    box = np.ones((2, 2))
    kept = []
    for _ in range(300):
        seeds = rng.random((24, 28)) < rng.choice([0.004, 0.008, 0.015])
        m = ndimage.binary_dilation(seeds, structure=np.ones((int(rng.integers(2, 5)), int(rng.integers(2, 5)))))
        p = np.pad(m, 2)
        if np.array_equal(ndimage.binary_opening(p, structure=box), p) and np.array_equal(ndimage.binary_opening(~p, structure=box), ~p):
            kept.append(m.astype(np.uint8))
    return kept


def test_approximate_round_trip_on_thick_masks(backend):
    kept = thick_slices()
    print("thick slices kept:", len(kept), "of 300")
    assert len(kept) >= 100, "the filter rejects too much to decide anything"
    m = np.stack(kept)[None]
    assert m.any(axis=(2, 3)).sum() > 50
    verts, rows, _ = backend.ctx.contour_trace(backend.dev(m), (28, 24, len(kept)), 1, True)
    full_verts, full_rows, _ = backend.ctx.contour_trace(backend.dev(m), (28, 24, len(kept)), 1, False)
    assert len(verts) < len(full_verts), "nothing was dropped"
    assert np.array_equal(fill(backend, verts, rows, m.shape), m)
    assert np.array_equal(fill(backend, full_verts, full_rows, m.shape), m)


# --------------------------------------------------------------------------------------
# 6. platipy_amd.dicom

SPACING, ORIGIN = (0.9, 1.1, 2.5), (-120.5, 33.25, 60.0)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def oblique():
    from tests.helpers import rot_xyz

    return tuple(rot_xyz(7.0, -4.0, 25.0).ravel().tolist())


def host_masks(pa, direction):
    nz, ny, nx = 9, 21, 23
    zz, yy, xx = np.indices((nz, ny, nx))
    r2 = (zz - 4) ** 2 * 4 + (yy - 10) ** 2 + (xx - 11) ** 2
    shell = ((r2 <= 81) & (r2 > 16)).astype(np.uint8)      # a sphere with an inner void
    speckle = (np.random.default_rng(5).random((nz, ny, nx)) < 0.4).astype(np.uint8)
    arrays = {"Shell": shell, "Nothing": np.zeros((nz, ny, nx), np.uint8), "Speckle": speckle}
    return {k: pa.image_from_array(v, SPACING, ORIGIN, direction) for k, v in arrays.items()}, arrays


@pytest.mark.parametrize("direction", ["identity", "oblique"])
def test_extract_contours(host_api, direction):
    pa = host_api
    d = IDENTITY if direction == "identity" else oblique()
    images, arrays = host_masks(pa, d)
    ref = images["Shell"]
    contours = pa.dicom.extract_contours(images)
    assert list(contours) == ["Shell", "Nothing", "Speckle"] and contours["Nothing"] == []
    assert all(p.dtype == np.float64 and p.ndim == 2 and p.shape[1] == 3 for polys in contours.values() for p in polys)
    back = pa.dicom.rasterise_contours(ref, contours)
    assert list(back) == list(arrays)
    for name, a in arrays.items():
        assert np.array_equal(back[name].numpy(), a), name
        assert back[name].same_grid(ref.like(back[name].tensor))
    # every point on its slice's plane; the tables behind the points
    verts, rows, hole, names = pa.dicom.extract_contours(images, as_physical=False)
    assert names == list(arrays) and verts.dtype == np.int32 and rows.dtype == _lib.CONTOUR_DTYPE and hole.dtype == np.uint8
    assert hole.sum() > 0 and set(rows["structure"].tolist()) == {0, 2}
    normal = np.asarray(d, dtype=np.float64).reshape(3, 3)[:, 2]
    flat = [p for name in names for p in contours[name]]
    assert len(flat) == len(rows)
    worst = 0.0
    for p, (first, count, s, z) in zip(flat, rows.tolist()):
        assert p.shape[0] == count
        worst = max(worst, float(np.abs((p - np.asarray(ORIGIN)) @ normal - z * SPACING[2]).max()))
        want = np.asarray(ORIGIN) + (np.asarray(d).reshape(3, 3) @ (np.array([[x, y, z] for x, y in verts[first:first + count].tolist()],
                                                                             dtype=np.float64) * np.asarray(SPACING)).T).T
        assert np.abs(p - want).max() < 1e-9
    print("largest distance from the slice plane (mm):", worst)
    assert worst <= 1e-9
    # through the RTSTRUCT tree and back
    ds = pa.dicom.contours_to_dicom_struct(contours)
    assert [r.ROIName for r in ds.StructureSetROISequence] == list(arrays) and [r.ROINumber for r in ds.StructureSetROISequence] == [1, 2, 3]
    shell = ds.ROIContourSequence[0]
    assert shell.ReferencedROINumber == 1 and shell.ROIDisplayColor == list(pa.dicom.PALETTE[0])
    assert all(c.ContourGeometricType == "CLOSED_PLANAR" and len(c.ContourData) == 3 * c.NumberOfContourPoints for c in shell.ContourSequence)
    assert ds.ROIContourSequence[1].ContourSequence == []
    images2, names2 = pa.dicom.transform_point_set_from_dicom_struct(ref, ds)
    assert names2 == ["Shell", "Speckle"]      # (a structure without contours is skipped by the reader, R7)
    assert np.array_equal(images2[0].numpy(), arrays["Shell"]) and np.array_equal(images2[1].numpy(), arrays["Speckle"])
    custom = pa.dicom.contours_to_dicom_struct(contours, colours={"Shell": (1, 2, 3), "Nothing": (4, 5, 6), "Speckle": (7, 8, 9)})
    assert custom.ROIContourSequence[2].ROIDisplayColor == [7, 8, 9]


def test_extract_contours_approximate_and_dtypes(host_api):
    pa = host_api
    images, arrays = host_masks(pa, IDENTITY)
    full = pa.dicom.extract_contours(images)
    approx = pa.dicom.extract_contours(images, approximate_contours=True)
    assert len(full["Shell"]) == len(approx["Shell"]) and sum(map(len, approx["Shell"])) < sum(map(len, full["Shell"]))
    as_float = {"Shell": images["Shell"].like(images["Shell"].tensor.to(torch.float32) * 0.25)}      # any non-zero voxel is foreground
    again = pa.dicom.extract_contours(as_float)
    assert all(np.array_equal(a, b) for a, b in zip(again["Shell"], full["Shell"])) and len(again["Shell"]) == len(full["Shell"])
    assert pa.dicom.extract_contours({}) == {}


# --------------------------------------------------------------------------------------
# 7. refusals


def test_host_refusals(host_api):
    pa = host_api
    images, _ = host_masks(pa, IDENTITY)
    other = pa.image_from_array(np.zeros((9, 21, 23), np.uint8), (0.9, 1.1, 3.0), ORIGIN, IDENTITY)
    with pytest.raises(ValueError):
        pa.dicom.extract_contours({"Shell": images["Shell"], "other": other})
    smaller = pa.image_from_array(np.zeros((9, 21, 22), np.uint8), SPACING, ORIGIN, IDENTITY)
    with pytest.raises(ValueError):
        pa.dicom.extract_contours({"Shell": images["Shell"], "smaller": smaller})
    vector = pa.image_from_array(np.zeros((3, 9, 21, 23), np.float32), SPACING, ORIGIN, IDENTITY, is_vector=True)
    with pytest.raises(ValueError):
        pa.dicom.extract_contours({"vector": vector})


def test_abi_refusals(backend):
    m = masks_of("noise-35x67")
    s, nz, ny, nx = m.shape
    dm = backend.dev(m)
    lib, h, size = backend.ctx.lib, backend.ctx.h, (C.c_int * 3)(nx, ny, nz)
    counts = (C.c_int64 * 3)()

    def call(masks=_lib.ptr(dm), size=size, nstructures=s, vertices=None, nverts=0, contours=None, hole=None, ncontours=0, counts=counts):
        return lib.pp_contour_trace_u8(h, masks, size, nstructures, 0, vertices, nverts, contours, hole, ncontours, counts)

    assert call() == _lib.PP_OK
    cracks, nv, nc = (int(c) for c in counts)
    assert (nv, nc) == (len(traced(backend, "noise-35x67", False)[0]), len(traced(backend, "noise-35x67", False)[1])) and cracks >= nv
    verts, rows, hole = np.full((nv + 1, 2), -7, np.int32), np.zeros(nc + 1, _lib.CONTOUR_DTYPE), np.full(nc + 1, 9, np.uint8)
    pv, pr, ph = verts.ctypes.data, rows.ctypes.data, hole.ctypes.data
    assert call(masks=None) == _lib.ERR_ARG and call(size=None) == _lib.ERR_ARG and call(counts=None) == _lib.ERR_ARG
    assert call(nstructures=0) == _lib.ERR_ARG and call(nstructures=-1) == _lib.ERR_ARG
    assert call(size=(C.c_int * 3)(nx, 0, nz)) == _lib.ERR_ARG
    assert call(vertices=None, nverts=nv, contours=pr, hole=ph, ncontours=nc) == _lib.ERR_ARG      # a NULL table
    assert call(vertices=pv, nverts=nv, contours=None, hole=ph, ncontours=nc) == _lib.ERR_ARG
    assert call(vertices=pv, nverts=nv, contours=pr, hole=None, ncontours=nc) == _lib.ERR_ARG
    assert call(vertices=pv, nverts=-1, contours=pr, hole=ph, ncontours=nc) == _lib.ERR_ARG
    for bad_v, bad_c in ((nv - 1, nc), (nv + 1, nc), (nv, nc - 1), (nv, nc + 1)):                   # mis-sized tables
        counts[1] = counts[2] = -1
        assert call(vertices=pv, nverts=bad_v, contours=pr, hole=ph, ncontours=bad_c) == _lib.ERR_ARG
        assert (int(counts[1]), int(counts[2])) == (nv, nc)
    assert (verts == -7).all() and (hole == 9).all()      # nothing was written by a refused call
    assert call(vertices=pv, nverts=nv, contours=pr, hole=ph, ncontours=nc) == _lib.PP_OK          # a fill call on its own
    want = traced(backend, "noise-35x67", False)
    assert np.array_equal(verts[:nv], want[0]) and np.array_equal(rows[:nc], want[1]) and np.array_equal(hole[:nc], want[2])
    assert (verts[nv] == -7).all() and hole[nc] == 9
    with pytest.raises(ValueError):
        backend.ctx.contour_trace(dm, (nx, ny, nz), s + 1)
    with pytest.raises(ValueError):
        backend.ctx.contour_trace(dm, (nx, ny, nz), 0)
