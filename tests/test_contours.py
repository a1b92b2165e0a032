"""RTSTRUCT contours to masks -- pp_contour_fill_u8 (csrc/pp_contour.h) and platipy_amd.dicom -- against
tests/contour_restatement.py: the point-in-polygon rule in numpy fp64 with its division kept, XOR per contour, the skip rules
in plain Python.

Bounds: none.  Vertices are integers within +-2^24, so every product and sum of the rule is an integer below 2^53 and the
fp64 restatement is exact; the kernel decides the same signs in int64.  Every comparison is np.array_equal, byte for byte,
and every output buffer is filled with 0xFF before the call, which has to define all of it.

The rule itself is recalled from scikit-image, which is not installed here.  test_closed_set_* therefore hold the kernel AND
the restatement to a test that does not rest on it: on convex polygons and on staircases the result must be the closed
polygon, decided by exact integer cross products / closed columns."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from platipy_amd import _lib
from tests import contour_restatement as C

CHUNK = _lib.CONTOUR_CHUNK      # edges staged into LDS per pass
SLICES = [(1, 1), (7, 19), (13, 13), (5, 37), (3, 1040)]      # (ny, nx): shorter than a 16-byte store, no multiple of 16, odd
#                                                               ny nx (slices off 16-byte alignment), wider than one tile


def tables(polys):
    """polys: (structure, z, [(x, y), ...]) -> (vertices [n, 2], contour rows)."""
    verts, rows = [], []
    for s, z, pts in polys:
        rows.append((len(verts), len(pts), s, z))
        verts += [(int(x), int(y)) for x, y in pts]
    return np.array(verts, dtype=np.int64).reshape(-1, 2), rows


def run_fill(backend, verts, rows, size, nstructures):
    nx, ny, nz = size
    out = backend.dev(np.full((nstructures, nz, ny, nx), 0xFF, np.uint8))
    backend.ctx.contour_fill(verts, rows, size, nstructures, out)
    return backend.host(out)


def check(backend, polys, size, nstructures, at_least=0):
    verts, rows = tables(polys)
    want = C.fill(verts, rows, size, nstructures)
    got = run_fill(backend, verts, rows, size, nstructures)
    assert np.array_equal(got, want), (int(got.sum()), int(want.sum()), np.argwhere(got != want)[:5])
    assert int(want.sum()) >= at_least, "the case decides nothing"
    return want


def random_polygons(ny, nx, nz, count, seed):
    """3 ... 12 integer vertices from [-4, n + 4): they reach over every border; every eighth polygon lies wholly outside."""
    rng = np.random.default_rng(seed)
    polys = []
    for k in range(count):
        n = int(rng.integers(3, 13))
        xs, ys = rng.integers(-4, nx + 4, n), rng.integers(-4, ny + 4, n)
        if k % 8 == 7:
            xs, ys = (rng.integers(-4, 0, n), ys) if k % 16 == 7 else (xs, rng.integers(ny, ny + 4, n))
        polys.append((k, k % nz, list(zip(xs.tolist(), ys.tolist()))))
    return polys


@pytest.mark.parametrize("nz", [1, 3])
@pytest.mark.parametrize("slice_", SLICES, ids=str)
def test_random_polygons(backend, slice_, nz):
    ny, nx = slice_
    polys = random_polygons(ny, nx, nz, 60, seed=1000 * ny + nx + nz)
    check(backend, polys, (nx, ny, nz), 60, at_least=1)


def test_two_calls_give_the_same_bytes(backend):
    polys = random_polygons(5, 37, 3, 60, seed=77)
    verts, rows = tables(polys)
    a = run_fill(backend, verts, rows, (37, 5, 3), 60)
    b = run_fill(backend, verts, rows, (37, 5, 3), 60)
    assert np.array_equal(a, b)


DEGENERATE = {
    "one vertex": [(5, 5)],
    "one vertex outside": [(-2, 3)],
    "two vertices": [(2, 3), (9, 8)],
    "two vertices, axis-aligned": [(2, 6), (11, 6)],
    "all equal": [(4, 6)] * 4,
    "repeated consecutive": [(2, 2), (2, 2), (9, 2), (9, 9), (9, 9), (9, 9), (2, 9)],
    "collinear": [(1, 1), (4, 4), (8, 8), (11, 11)],
    "collinear on an edge": [(1, 1), (6, 1), (11, 1), (11, 11), (6, 6)],
    "spur": [(2, 2), (9, 2), (9, 9), (12, 12), (9, 9), (2, 9)],
    "spur along an edge": [(2, 2), (12, 2), (9, 2), (9, 9), (2, 9)],
    "bow-tie": [(2, 2), (10, 10), (10, 2), (2, 10)],
    "bow-tie, even": [(1, 1), (11, 12), (11, 1), (1, 12)],
    "rectangle": [(3, 2), (10, 2), (10, 8), (3, 8)],
    "rectangle, reversed": [(3, 8), (10, 8), (10, 2), (3, 2)],
    "rectangle over the border": [(-3, -2), (15, -2), (15, 4), (-3, 4)],
    "slope 1/2": [(0, 0), (12, 6), (0, 6)],
    "slope 3/1": [(1, 0), (5, 12), (1, 12)],
    "slope 1/1": [(0, 0), (12, 12), (12, 0)],
    "slope 2/3": [(0, 0), (12, 8), (0, 8)],
    "slope 1/2, reversed": [(0, 6), (12, 6), (0, 0)],
    "slope -3/1": [(5, 0), (1, 12), (9, 12)],
    "slope -2/3": [(12, 0), (0, 8), (12, 8)],
}


@pytest.mark.parametrize("slice_", [(13, 13), (7, 19)], ids=str)
def test_degenerate_polygons(backend, slice_):
    ny, nx = slice_
    polys = [(k, k % 3, pts) for k, pts in enumerate(DEGENERATE.values())]
    want = check(backend, polys, (nx, ny, 3), len(polys), at_least=100)
    names = list(DEGENERATE)
    assert want[names.index("one vertex")].sum() == 1 and want[names.index("one vertex outside")].sum() == 0
    assert want[names.index("all equal")].sum() == 1


def circle(n, cx, cy, r):
    t = 2.0 * np.pi * np.arange(n) / n
    return list(zip(np.floor(cx + r * np.cos(t) + 0.5).astype(int).tolist(), np.floor(cy + r * np.sin(t) + 0.5).astype(int).tolist()))


@pytest.mark.parametrize("n", [CHUNK + 1, 2 * CHUNK + 3])
def test_more_vertices_than_one_chunk(backend, n):
    """A circle of 31 pixels radius rounded to integers on a 70 x 90 slice: it spans two tiles in x and two in y, so the
    edge list is staged in two or three passes AND culled differently by each tile."""
    want = check(backend, [(0, 0, circle(n, 45.3, 34.6, 31.0)), (1, 1, circle(n, 40.0, 30.0, 3.0))], (90, 70, 2), 2, at_least=2500)
    assert want[0, 0, 35, 45] == 1 and want[0, 0, 0, 0] == 0 and want[0, 1].sum() == 0


def test_xor_of_contours_on_one_slice(backend):
    outer, inner, core = circle(48, 20, 18, 15), circle(32, 21, 18, 8), circle(16, 20, 17, 3)
    rng = np.random.default_rng(3)
    many = []
    for _ in range(40):
        x, y, w, h = (int(v) for v in (rng.integers(-2, 36), rng.integers(-2, 32), rng.integers(1, 14), rng.integers(1, 14)))
        many.append((3, 1, [(x, y), (x + w, y), (x + w // 2, y + h)] if rng.random() < 0.5 else [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]))
    polys = [(0, 0, outer), (0, 0, inner),                      # a ring
             (1, 1, outer), (1, 1, list(outer)),                # the same contour twice: nothing
             (2, 0, outer), (2, 0, inner), (2, 0, core),        # three nested
             (2, 1, core)] + many                               # 40 contours on one slice of one structure
    want = check(backend, polys, (40, 36, 2), 4, at_least=500)
    assert want[0, 0, 18, 20] == 0 and want[0, 0, 18, 33] == 1      # the hole and the ring
    assert want[1].sum() == 0
    assert want[2, 0, 17, 20] == 1 and want[2, 0, 18, 27] == 0 and want[2, 0, 18, 33] == 1
    assert np.array_equal(want[2, 0], want[0, 0] ^ want[2, 1])


def test_many_jobs_and_structures_without_contours(backend):
    """5 structures x 3 slices with different boxes in one call, between two structures that have no contour at all."""
    rng = np.random.default_rng(11)
    polys = []
    for s in (0, 1, 3, 4, 6):
        for z in range(3):
            cx, cy, r = rng.uniform(2, 60), rng.uniform(2, 30), rng.uniform(1.5, 14)
            polys.append((s, z, circle(int(rng.integers(5, 40)), cx, cy, r)))
    want = check(backend, polys, (67, 33, 3), 7, at_least=500)
    assert want[2].sum() == 0 and want[5].sum() == 0
    assert all(want[s, z].sum() > 0 for s in (0, 1, 3, 4, 6) for z in range(3))


def test_no_contours_gives_all_zeros(backend):
    got = run_fill(backend, np.zeros((0, 2), np.int64), [], (19, 7, 3), 2)
    assert got.shape == (2, 3, 7, 19) and not got.any()


def test_vertex_bound(backend):
    """+-2^24 is accepted and decided exactly; 2^24 + 1 is refused by the C call, which leaves `out` alone."""
    big = 1 << 24
    polys = [(0, 0, [(-big, -big), (big, -big), (big, big), (-big, big)]),
             (1, 0, [(-big, 3), (big, 5), (7, big)]),
             (2, 0, [(-big, -big), (big, big), (big, big - 1)]),      # a sliver along the main diagonal
             (3, 0, [(6, -big), (6, big), (big, 2)])]
    want = check(backend, polys, (19, 7, 1), 4, at_least=19 * 7)
    assert want[0].all()
    for bad in (big + 1, -big - 1):
        verts, rows = tables([(0, 0, [(0, 0), (bad, 3), (4, 5)])])
        out = backend.dev(np.full((1, 1, 7, 19), 0xFF, np.uint8))
        with pytest.raises(ValueError):
            backend.ctx.contour_fill(verts, rows, (19, 7, 1), 1, out)
        assert (backend.host(out) == 0xFF).all()
    with pytest.raises(ValueError):      # (does not fit the table's int32 at all)
        backend.ctx.contour_fill(np.array([[0, 0], [1 << 40, 3], [4, 5]]), [(0, 3, 0, 0)], (19, 7, 1), 1, out)


def test_refused_tables(backend):
    verts, _ = tables([(0, 0, [(0, 0), (5, 3), (4, 5)])])
    out = backend.dev(np.full((2, 1, 7, 19), 0xFF, np.uint8))
    for rows in ([(0, 4, 0, 0)], [(1, 3, 0, 0)], [(-1, 2, 0, 0)], [(0, 0, 0, 0)], [(0, 3, 2, 0)], [(0, 3, -1, 0)], [(0, 3, 0, 1)],
                 [(0, 3, 0, -1)]):
        with pytest.raises(ValueError):
            backend.ctx.contour_fill(verts, rows, (19, 7, 1), 2, out)
    for size, nstructures in (((19, 7, 0), 2), ((19, 7, 1), 0), ((19, 7, 1), 3)):
        with pytest.raises(ValueError):
            backend.ctx.contour_fill(verts, [(0, 3, 0, 0)], size, nstructures, out)
    assert (backend.host(out) == 0xFF).all()


# --------------------------------------------------------------------------------------
# the independent test


def convex_family(count, seed):
    rng = np.random.default_rng(seed)
    hulls = []
    while len(hulls) < count:
        h = C.convex_hull(rng.integers(2, 14, size=(int(rng.integers(3, 10)), 2)).tolist())      # points in a 12 x 12 box
        if len(h) >= 3:
            hulls.append(h if len(hulls) % 2 else h[::-1])      # both orientations
    return hulls


def staircase_family(count, seed):
    rng = np.random.default_rng(seed)
    return [C.staircase(rng.integers(1, 9, int(rng.integers(2, 9))).tolist(), int(rng.integers(1, 5)), int(rng.integers(1, 5)))
            for _ in range(count)]


def test_closed_set_restatement():
    """The restatement itself against the exact closed-set test (no kernel): if this fails the restatement has a slip."""
    for h in convex_family(100, 5):
        assert np.array_equal(C.polygon_mask([p[0] for p in h], [p[1] for p in h], 16, 16), C.closed_convex_mask(h, 16, 16)), h
    for verts, cols in staircase_family(50, 6):
        assert np.array_equal(C.polygon_mask([p[0] for p in verts], [p[1] for p in verts], 16, 16), C.closed_columns_mask(cols, 16, 16)), verts


def test_closed_set_kernel(backend):
    hulls, stairs = convex_family(100, 5), staircase_family(50, 6)
    polys = [(k, 0, h) for k, h in enumerate(hulls)] + [(100 + k, 0, v) for k, (v, _) in enumerate(stairs)]
    verts, rows = tables(polys)
    got = run_fill(backend, verts, rows, (16, 16, 1), 150)
    for k, h in enumerate(hulls):
        assert np.array_equal(got[k, 0], C.closed_convex_mask(h, 16, 16)), h
    for k, (_, cols) in enumerate(stairs):
        assert np.array_equal(got[100 + k, 0], C.closed_columns_mask(cols, 16, 16)), cols


# --------------------------------------------------------------------------------------
# platipy_amd.dicom

CARDIAC = ((0.9, 0.9, 2.5), (320.0, -52.0, 60.0))      # spacing and origin of the reference's cardiac fixture
ROT90Z = (0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def oblique():
    from tests.helpers import rot_xyz

    return tuple(rot_xyz(7.0, -4.0, 25.0).ravel().tolist())


def to_physical(index_points, spacing, origin, direction):
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    return np.asarray(origin) + (d @ (np.asarray(index_points, dtype=np.float64) * np.asarray(spacing)).T).T


def blank(pa, size, spacing, origin, direction):
    nx, ny, nz = size
    return pa.image_from_array(np.zeros((nz, ny, nx), np.float32), spacing, origin, direction)


def sample_structures(size, spacing, origin, direction, seed):
    """Three structures whose vertices sit at fractional continuous indices (never within 0.05 of a tie): a ring over three
    slices, a blob that reaches over the border and has one contour below slice 0 and one at nz, and a structure one of
    whose contours is tilted over two slices."""
    nx, ny, nz = size
    rng = np.random.default_rng(seed)

    def poly(n, cx, cy, r, z, tilt=0.0):
        t = 2.0 * np.pi * np.arange(n) / n
        x, y = cx + r * np.cos(t), cy + r * np.sin(t)
        x, y = np.floor(x) + rng.uniform(-0.45, 0.45, n), np.floor(y) + rng.uniform(-0.45, 0.45, n)
        return to_physical(np.stack([x, y, z + rng.uniform(-0.3, 0.3, n) + tilt * np.arange(n)], axis=1), spacing, origin, direction)

    ring = [poly(24, nx * 0.5, ny * 0.5, ny * 0.4, z) for z in (1, 2, 3)] + [poly(12, nx * 0.5, ny * 0.5, ny * 0.2, z) for z in (1, 2, 3)]
    blob = [poly(9, nx * 0.9, ny * 0.2, ny * 0.3, z) for z in (-1, 0, nz - 1, nz)]
    tilted = [poly(8, 5, 5, 3, 1), poly(8, 6, 5, 3, 2, tilt=0.2)]
    return [("ring", ring), ("blob", blob), ("tilted", tilted)]


@pytest.mark.parametrize("direction", ["identity", "rot90z", "oblique"])
def test_rasterise_contours_transform(host_api, direction):
    pa = host_api
    d = {"identity": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), "rot90z": ROT90Z, "oblique": oblique()}[direction]
    size = (31, 22, 5)
    ref = blank(pa, size, *CARDIAC, d)
    structures = sample_structures(size, *CARDIAC, d, seed=21)
    want, names, _ = C.rasterise(size, *CARDIAC, d, structures)
    assert names == ["ring", "blob"] and all(m.sum() > 20 for m in want)
    got = pa.dicom.rasterise_contours(ref, dict(structures))
    assert list(got) == names
    for name, m in zip(names, want):
        img = got[name]
        assert img.tensor.dtype == torch.uint8 and img.GetSize() == size
        assert img.GetSpacing() == ref.GetSpacing() and img.GetOrigin() == ref.GetOrigin() and img.GetDirection() == ref.GetDirection()
        assert np.array_equal(img.numpy(), m), name
    stack, names2 = pa.dicom.rasterise_contours(ref, dict(structures), as_dict=False)
    assert names2 == names and tuple(stack.shape) == (2, 5, 22, 31) and np.array_equal(stack.cpu().numpy(), np.stack(want))


def test_half_indices_round_up(host_api):
    """Dyadic geometry, so the continuous indices are exact: 1.5 -> 2, 5.5 -> 6, 4.5 -> 5, -0.5 -> 0, -1.5 -> -1, z 0.5 -> 1."""
    pa = host_api
    spacing, origin = (0.5, 2.0, 4.0), (-8.0, 4.0, 16.0)
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    ref = blank(pa, (9, 8, 3), spacing, origin, ident)
    rect = to_physical([(1.5, 1.5, 0.5), (5.5, 1.5, 0.5), (5.5, 4.5, 0.5), (1.5, 4.5, 0.5)], spacing, origin, ident)
    corner = to_physical([(-1.5, -1.5, 1.5), (-0.5, -1.5, 1.5), (-0.5, -0.5, 1.5), (-1.5, -0.5, 1.5)], spacing, origin, ident)
    got = pa.dicom.rasterise_contours(ref, {"rect": [rect], "corner": [corner]})
    want = np.zeros((3, 8, 9), np.uint8)
    want[1, 2:6, 2:7] = 1
    assert np.array_equal(got["rect"].numpy(), want)
    want = np.zeros((3, 8, 9), np.uint8)
    want[2, 0, 0] = 1      # the square (-1, -1) ... (0, 0): only its corner (0, 0) is a pixel
    assert np.array_equal(got["corner"].numpy(), want)
    masks, _, _ = C.rasterise((9, 8, 3), spacing, origin, ident, [("rect", [rect]), ("corner", [corner])])
    assert np.array_equal(got["rect"].numpy(), masks[0]) and np.array_equal(got["corner"].numpy(), masks[1])


def test_spacing_override(host_api):
    pa = host_api
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    size = (20, 17, 6)
    ref = blank(pa, size, *CARDIAC, ident)
    override = (0, 0, 3.0)
    spacing = (0.9, 0.9, 3.0)
    structures = [(n, c) for n, c in sample_structures(size, spacing, CARDIAC[1], ident, seed=4) if n != "tilted"]
    want, names, used = C.rasterise(size, *CARDIAC, ident, structures, spacing_override=override)
    assert used == spacing
    plain, plain_names, _ = C.rasterise(size, *CARDIAC, ident, structures)
    assert plain_names != names or not all(np.array_equal(a, b) for a, b in zip(want, plain)), "the override decides nothing"
    got = pa.dicom.rasterise_contours(ref, dict(structures), spacing_override=override)
    assert list(got) == names
    for name, m in zip(names, want):
        assert np.array_equal(got[name].numpy(), m)
        assert got[name].GetSpacing() == spacing
    assert ref.GetSpacing() == CARDIAC[0]      # the caller's image is left alone


def dataset(size, spacing, origin, direction):
    """An RTSTRUCT as a tree of SimpleNamespace that meets every skip rule."""
    st = dict(sample_structures(size, spacing, origin, direction, seed=8))

    def contours(polys, kind="CLOSED_PLANAR"):
        return [NS(ContourGeometricType=kind, ContourData=[float(v) for v in p.ravel()]) for p in polys]

    rois = [NS(ROIName="Heart", ROINumber=1), NS(ROIName="no entry", ROINumber=2), NS(ROIName="no sequence", ROINumber=3),
            NS(ROIName="empty sequence", ROINumber=4), NS(ROIName="open first", ROINumber=5), NS(ROIName="two slices", ROINumber=6),
            NS(ROIName="  Left \t Lung  (L) ", ROINumber=9), NS(ROIName="open later", ROINumber=7)]
    open_later = contours(st["ring"][:1]) + contours(st["ring"][3:4], "OPEN_PLANAR")
    seq = [NS(ReferencedROINumber=9, ContourSequence=contours(st["blob"])),
           NS(ReferencedROINumber=1, ContourSequence=contours(st["ring"])),
           NS(ReferencedROINumber=3),
           NS(ReferencedROINumber=4, ContourSequence=[]),
           NS(ReferencedROINumber=5, ContourSequence=contours(st["ring"][:1], "OPEN_PLANAR") + contours(st["ring"][1:2])),
           NS(ReferencedROINumber=6, ContourSequence=contours(st["tilted"])),
           NS(ReferencedROINumber=7, ContourSequence=open_later)]
    return NS(StructureSetROISequence=rois, ROIContourSequence=seq)


def test_transform_point_set_from_dicom_struct(host_api):
    pa = host_api
    d = oblique()
    size = (31, 22, 5)
    ref = blank(pa, size, *CARDIAC, d)
    ds = dataset(size, *CARDIAC, d)
    structures = C.structures_of_dataset(ds)
    assert [n for n, _ in structures] == ["Heart", "two_slices", "Left_Lung_(L)", "open_later"]
    want, names, _ = C.rasterise(size, *CARDIAC, d, structures)
    assert names == ["Heart", "Left_Lung_(L)", "open_later"]      # "two slices" is absent as a whole
    images, got_names = pa.dicom.transform_point_set_from_dicom_struct(ref, ds)
    assert isinstance(images, list) and got_names == names
    for img, m in zip(images, want):
        assert img.tensor.dtype == torch.uint8 and img.same_grid(ref.like(img.tensor))
        assert np.array_equal(img.numpy(), m) and m.sum() > 0
    # the blob's contours below slice 0 and at nz are skipped alone: it equals the blob without them
    blob = dict(sample_structures(size, *CARDIAC, d, seed=8))["blob"]
    alone, _, _ = C.rasterise(size, *CARDIAC, d, [("b", blob[1:3])])
    assert np.array_equal(images[1].numpy(), alone[0])
    # the override reaches the function too, and leaves the image alone
    images3, names3 = pa.dicom.transform_point_set_from_dicom_struct(ref, ds, spacing_override=(0, 0, 1.25))
    want3, wnames3, used = C.rasterise(size, *CARDIAC, d, structures, spacing_override=(0, 0, 1.25))
    assert names3 == wnames3 and all(np.array_equal(i.numpy(), m) for i, m in zip(images3, want3))
    assert all(i.GetSpacing() == used for i in images3) and ref.GetSpacing() == CARDIAC[0]


def test_dataset_with_a_missing_value(host_api):
    pa = host_api
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    size = (12, 11, 3)
    ref = blank(pa, size, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), ident)
    data = [2.0, 2.0, 1.0, 9.0, 2.0, 1.0, 9.0, 8.0, 1.0, 2.0, 8.0, 1.0]
    holed = list(data)
    holed[5] = ""       # a z: the minimum of the others
    ds = NS(StructureSetROISequence=[NS(ROIName="box", ROINumber=1)],
            ROIContourSequence=[NS(ReferencedROINumber=1, ContourSequence=[NS(ContourGeometricType="CLOSED_PLANAR", ContourData=holed)])])
    images, names = pa.dicom.transform_point_set_from_dicom_struct(ref, ds)
    want = np.zeros((3, 11, 12), np.uint8)
    want[1, 2:9, 2:10] = 1
    assert names == ["box"] and np.array_equal(images[0].numpy(), want)


def test_fix_missing_data(host_api):
    pa = host_api
    data = [1.0, 10.0, 5.0, 3.0, 12.0, 5.0, 7.0, 16.0, 4.5, 2.0, 11.0, 5.0]      # four vertices

    def fixed(k):
        holed = [str(v) for v in data]
        holed[k] = ""
        out = pa.dicom.fix_missing_data(holed)
        assert out.dtype == np.float64 and out.shape == (12,)
        assert np.array_equal(np.delete(out, k), np.delete(np.array(data), k))
        return out[k]

    # x and y: the mean of the neighbouring vertices of the CLOSED contour
    assert fixed(0) == 0.5 * (2.0 + 3.0) and fixed(3) == 0.5 * (1.0 + 7.0) and fixed(9) == 0.5 * (7.0 + 1.0)
    assert fixed(1) == 0.5 * (11.0 + 12.0) and fixed(4) == 0.5 * (10.0 + 16.0) and fixed(10) == 0.5 * (16.0 + 10.0)
    # z: the minimum of the other vertices' z
    assert fixed(2) == 4.5 and fixed(5) == 4.5 and fixed(8) == 5.0 and fixed(11) == 4.5
    assert np.array_equal(pa.dicom.fix_missing_data(data), np.array(data))      # nothing missing
    two = [str(v) for v in data]
    two[0] = two[4] = ""
    assert list(pa.dicom.fix_missing_data(two)) == two      # not repaired


def test_refusals(host_api):
    pa = host_api
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    ref = blank(pa, (12, 11, 3), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), ident)
    with pytest.raises(ValueError):
        pa.dicom.rasterise_contours(ref, {"far": [np.array([[1.0, 1.0, 1.0], [2.0 ** 24 + 1, 3.0, 1.0], [4.0, 5.0, 1.0]])]})
    with pytest.raises(ValueError):
        pa.dicom.rasterise_contours(ref, {"nan": [np.array([[1.0, np.nan, 1.0]])]})
    with pytest.raises(ValueError):
        pa.dicom.rasterise_contours(ref, {"empty": [np.zeros((0, 3))]})
    assert pa.dicom.rasterise_contours(ref, {}) == {}
    stack, names = pa.dicom.rasterise_contours(ref, {}, as_dict=False)
    assert tuple(stack.shape) == (0, 3, 11, 12) and names == []
    got = pa.dicom.rasterise_contours(ref, {"none": []})      # a structure without contours: kept, all zero
    assert list(got) == ["none"] and not got["none"].numpy().any()


def test_sphere_end_to_end(host_api):
    """A sphere of 10 voxels radius cut into per-slice circles of 64 vertices, rasterised, against insert_sphere_image.  The
    bound is the restatement's own Dice on the same polygons, minus nothing."""
    pa = host_api
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    size, spacing, origin = (32, 32, 32), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    ref = blank(pa, size, spacing, origin, ident)
    sphere = pa.generation.insert_sphere_image(ref, 10, (16, 16, 16))
    sphere = sphere.like((sphere.tensor != 0).to(torch.uint8))
    t = 2.0 * np.pi * np.arange(64) / 64
    polys = []
    for z in range(6, 27):
        r = np.sqrt(100.0 - (z - 16.0) ** 2)
        polys.append(np.stack([16.0 + r * np.cos(t), 16.0 + r * np.sin(t), np.full(64, float(z))], axis=1))
    want, _, _ = C.rasterise(size, spacing, origin, ident, [("sphere", polys)])
    truth = sphere.numpy() != 0
    na, nb, nab = int(truth.sum()), int(want[0].sum()), int((truth & (want[0] != 0)).sum())
    bound = np.float64(2.0 * nab) / np.float64(na + nb)
    assert bound > 0.9, "the polygons do not describe the sphere"
    got = pa.dicom.rasterise_contours(ref, {"sphere": polys})
    dsc = pa.label.comparison.compute_metric_dsc(sphere, got["sphere"])
    print("Dice", dsc, "bound", float(bound))
    assert dsc >= bound
    dose = ref.like(torch.full((32, 32, 32), 2.0, dtype=torch.float32, device=ref.device))
    dvh = pa.dose.calculate_dvh_for_labels(dose, got)
    assert list(dvh.label) == ["sphere"] and abs(float(dvh.cc[0]) - nb / 1000.0) < 1e-9
