"""The mask post-processing kernels (pp_cc.hip, pp_dist.hip, pp_morph.hip) on adversarial shapes.

test_kernels.py holds each of them to the oracle on smooth blobs; here the inputs are the ones on which a wrong
run-start rule, a dropped carry, a wrong tie-break or an off-by-one in the parabola envelope shows: snakes, checkerboards,
nested shells, Bernoulli noise, rows that straddle the scan passes, single border voxels, radii up to the table's end.

References: scipy.ndimage with face connectivity, and -- for volumes of at most BRUTE_MAX voxels -- brute-force fp64
restatements written below (a BFS flood fill; the minimum over all border voxels of the spacing-weighted distance), so
that the small cases do not rest on scipy alone.  Every case compares every voxel.  Masks and counts are bit-exact;
distances carry test_distance_map_and_contour's tolerance (rtol 2e-6, atol 2e-5), are exactly 0.0 on border voxels and
have the exact sign everywhere.
"""
from collections import deque

import numpy as np
import pytest
from scipy import ndimage

from oracle import oracle as O
from platipy_amd import _lib
from tests.helpers import bernoulli, boundary_rows, checkerboard, nested_shells, random_runs, serpentine

BRUTE_MAX = 4096
NO_BORDER = np.float32(1.0e9)      # sqrtf of the kernel's "no border voxel" squared distance (1e18f); see DESIGN.md


def size_of(shape):
    return (shape[2], shape[1], shape[0])


# --------------------------------------------------------------------------------------
# connected components and hole filling

def _neighbours6(shape, z, y, x):
    if z > 0:
        yield z - 1, y, x
    if y > 0:
        yield z, y - 1, x
    if x > 0:
        yield z, y, x - 1
    if x + 1 < shape[2]:
        yield z, y, x + 1
    if y + 1 < shape[1]:
        yield z, y + 1, x
    if z + 1 < shape[0]:
        yield z + 1, y, x


def bfs_label(b):
    """Face-connected components of the True voxels by plain BFS, numbered from 1 in raster order of their first voxel."""
    lab = np.zeros(b.shape, np.int64)
    n = 0
    for start in zip(*np.nonzero(b)):              # np.nonzero walks in raster order
        if lab[start]:
            continue
        n += 1
        lab[start] = n
        todo = deque([start])
        while todo:
            p = todo.popleft()
            for q in _neighbours6(b.shape, *p):
                if b[q] and not lab[q]:
                    lab[q] = n
                    todo.append(q)
    return lab, n


def bfs_fill_holes(b):
    """b plus the background components that own no voxel on the volume's border."""
    lab, n = bfs_label(~b)
    edge = np.ones(b.shape, bool)
    edge[1:-1, 1:-1, 1:-1] = False
    open_ids = np.unique(lab[edge & ~b])
    return b | ((lab > 0) & ~np.isin(lab, open_ids))


def _first_largest(lab):
    """(mask of the largest component, its size); ties go to the component whose first voxel comes first in raster order
    -- computed from the voxel indices, not from the labeller's numbering.  No component: (all zeros, 0)."""
    ids, first, counts = np.unique(lab.ravel(), return_index=True, return_counts=True)
    keep = ids > 0
    if not keep.any():
        return np.zeros(lab.shape, np.uint8), 0
    ids, first, counts = ids[keep], first[keep], counts[keep]
    best = counts == counts.max()
    return (lab == ids[best][np.argmin(first[best])]).astype(np.uint8), int(counts.max())


def cc_reference(m, fill):
    b = m.astype(bool)
    if fill:
        b = ndimage.binary_fill_holes(b)
    want, count = _first_largest(ndimage.label(b)[0])
    if m.size <= BRUTE_MAX:
        bb = bfs_fill_holes(m.astype(bool)) if fill else m.astype(bool)
        np.testing.assert_array_equal(bb, b, err_msg="BFS and scipy disagree on the filled mask")
        want2, count2 = _first_largest(bfs_label(bb)[0])
        np.testing.assert_array_equal(want2, want, err_msg="BFS and scipy disagree on the largest component")
        assert count2 == count
    return want, count


def run_cc(backend, m, fill):
    out = backend.empty(m.shape, np.uint8)
    cnt = backend.ctx.fillhole_largest_component(backend.dev(m), size_of(m.shape), out, fill_holes=fill, want_count=True)
    return backend.host(out).copy(), cnt


def check_cc(backend, m, label=""):
    """Both fill_holes settings of one mask against the references, every voxel and the count; -> the two outputs."""
    m = np.ascontiguousarray(m, dtype=np.uint8)
    got = {}
    for fill in (True, False):
        want, count = cc_reference(m, fill)
        out, cnt = run_cc(backend, m, fill)
        np.testing.assert_array_equal(out, want, err_msg=f"{label} fill_holes={fill}")
        assert cnt == count, (label, fill, cnt, count)
        got[fill] = (out, cnt)
    return got


CC_SHAPE = (39, 47, 64)     # 117k voxels: 459 blocks of 256, 1833 rows (some wavefronts of the last block have no row)


def test_cc_serpentine_and_its_complement(backend):
    m = serpentine(CC_SHAPE)
    assert ndimage.label(m)[1] == 1 and int(m.sum()) > 30000        # one component, ~900 rows and joints long
    got = check_cc(backend, m, "serpentine")
    assert got[False][1] == int(m.sum())
    check_cc(backend, 1 - m, "serpentine complement")
    small = serpentine((5, 7, 9))                                   # the BFS reference's size
    check_cc(backend, small, "small serpentine")
    check_cc(backend, 1 - small, "small serpentine complement")


@pytest.mark.parametrize("shape", [(39, 47, 63), (5, 6, 7), (4, 4, 4)])
def test_cc_checkerboard(backend, shape):
    """n/2 one-voxel components, all tied: voxel 0's wins.  Filled, every interior background voxel is a hole."""
    m = checkerboard(shape)
    got = check_cc(backend, m, f"checkerboard {shape}")
    first = np.zeros(shape, np.uint8)
    first[0, 0, 0] = 1
    np.testing.assert_array_equal(got[False][0], first)
    assert got[False][1] == 1
    inv = 1 - m                                                  # voxel 0 is background: the winner is voxel 1
    got = check_cc(backend, inv, f"inverse checkerboard {shape}")
    assert got[False][0].ravel()[1] == 1 and got[False][1] == 1


@pytest.mark.parametrize("opening", [None, "face", "edge", "corner"])
def test_cc_nested_shells(backend, opening):
    m = nested_shells(opening=opening)
    got = check_cc(backend, m, f"shells {opening}")
    outer = (m.shape[0] - 2) * (m.shape[1] - 2) * (m.shape[2] - 2)
    if opening == "face":       # the outer cavity drains through the channel: the one-voxel outer wall is the largest
        inside = (m.shape[0] - 4) * (m.shape[1] - 4) * (m.shape[2] - 4)
        assert got[True][1] == got[False][1] == outer - inside - 1
    else:                       # a hole: everything inside the outer wall fills (minus the removed wall voxel)
        assert got[True][1] == outer - (0 if opening is None else 1)


def test_cc_diagonal_contact(backend):
    """Blocks that touch only across an edge or a corner stay separate components."""
    m = np.zeros((7, 9, 12), np.uint8)
    m[0:2, 0:3, 0:3] = 1          # 18 voxels
    m[2:4, 3:6, 3:6] = 1          # touches the first at a corner only: 18 voxels, later in raster order
    m[4:6, 3:6, 6:9] = 1          # touches the second across an edge (z and x differ): 18 voxels
    got = check_cc(backend, m, "diagonal")
    want = np.zeros_like(m)
    want[0:2, 0:3, 0:3] = 1
    np.testing.assert_array_equal(got[False][0], want)
    assert got[False][1] == 18
    m[5, 5, 9] = 1                # the third grows by a face neighbour and wins
    got = check_cc(backend, m, "diagonal, third larger")
    assert got[False][1] == 19 and got[False][0][5, 5, 9] == 1 and got[False][0][:4].sum() == 0


@pytest.mark.parametrize("density", [0.25, 0.31, 0.5, 0.7])
def test_cc_bernoulli(backend, density):
    """0.31 is near the site-percolation threshold of the cubic lattice: many mid-sized components."""
    check_cc(backend, bernoulli(CC_SHAPE, density, seed=int(density * 100)), f"bernoulli {density}")
    check_cc(backend, bernoulli((9, 14, 17), density, seed=7), f"small bernoulli {density}")


@pytest.mark.parametrize("seed", [11, 12])
def test_cc_random_runs(backend, seed):
    """Runs of 1..5 voxels per row: runs of adjacent rows overlap in single voxels, under a run that starts to the left
    as often as to the right (k_cc_merge's `start || upper-left differs` rule)."""
    check_cc(backend, random_runs(CC_SHAPE, seed), "runs 1..5")
    check_cc(backend, random_runs((8, 9, 33), seed), "small runs 1..5")


def test_cc_run_start_rule_by_hand(backend):
    """The two ways a run can meet the row above in a single voxel, in y and in z, alone in the volume."""
    for axis in (1, 0):
        for upper, lower in [((2, 6), (5, 9)), ((5, 9), (2, 6)), ((2, 9), (4, 6)), ((4, 6), (2, 9))]:
            m = np.zeros((3, 3, 12), np.uint8)
            a, b = [1, 1, slice(*upper)], [1, 1, slice(*lower)]
            a[axis], b[axis] = 0, 1
            m[tuple(a)] = 1
            m[tuple(b)] = 1
            got = check_cc(backend, m, f"axis {axis} {upper} {lower}")
            assert got[False][1] == int(m.sum())
            check_cc(backend, 1 - m, f"complement axis {axis} {upper} {lower}")


def test_cc_ties(backend):
    # two components: the raster-first one (smaller z) has the larger x and y
    m = np.zeros((4, 8, 12), np.uint8)
    m[0, 6, 8:11] = 1
    m[1, 1, 1:4] = 1
    got = check_cc(backend, m, "tie z")
    assert got[False][0][0, 6, 9] == 1 and got[False][0][1].sum() == 0
    # same plane: the raster-first one (smaller y) has the larger x
    m = np.zeros((3, 8, 12), np.uint8)
    m[1, 2, 9:12] = 1
    m[1, 5, 0:3] = 1
    got = check_cc(backend, m, "tie y")
    assert got[False][0][1, 2, 10] == 1 and got[False][0][1, 5].sum() == 0
    # three tied L-shapes whose ROOTS (first voxels) order differently from their smallest x, plus smaller ones
    m = np.zeros((5, 9, 14), np.uint8)
    m[1, 1, 10], m[1, 2, 8:11] = 1, 1        # root (1, 1, 10); smallest x 8
    m[1, 6, 0:4] = 1                         # root (1, 6, 0)
    m[3, 0, 5:7], m[3, 1, 5:7] = 1, 1        # root (3, 0, 5)
    m[0, 8, 12:14] = 1                       # smaller, earlier
    m[4, 8, 0:3] = 1                         # smaller, later
    got = check_cc(backend, m, "three-way tie")
    assert got[False][1] == 4 and got[False][0][1, 1, 10] == 1 and got[False][0].sum() == 4
    # tied components far apart: their roots fall to different blocks of the arg-max and to its final fold
    m = np.zeros(CC_SHAPE, np.uint8)
    m[30, 40, 1:6] = 1
    m[8, 45, 50:55] = 1                      # raster-first (z = 8)
    m[20, 3, 20:25] = 1
    m[38, 0, 0:4] = 1
    got = check_cc(backend, m, "far ties")
    assert got[False][1] == 5 and got[False][0][8, 45, 52] == 1 and got[False][0].sum() == 5


def test_cc_tie_inside_one_argmax_thread(backend):
    """k_cc_argmax runs at most 2048 blocks of 256 threads: only above 524288 voxels does one thread meet two roots and
    resolve their tie itself -- the one path here that needs a volume this large (nearly all background)."""
    shape = (3, 342, 512)
    assert shape[0] * shape[1] * shape[2] > 2048 * 256
    m = np.zeros(shape, np.uint8)
    flat = m.reshape(-1)
    flat[5] = flat[5 + 2048 * 256] = 1       # same thread, equal size
    flat[300:302] = flat[300 + 2048 * 256:302 + 2048 * 256] = 1
    want, count = _first_largest(ndimage.label(m)[0])
    out, cnt = run_cc(backend, m, False)
    np.testing.assert_array_equal(out, want)
    assert cnt == count == 2 and out.reshape(-1)[300] == 1


ROW_NX = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1025]


def _row_case(nx, pass_len):
    return boundary_rows(nx, 9, seed=nx, pass_len=pass_len).reshape(3, 3, nx)     # 9 rows: the third wavefront group has 1


@pytest.mark.parametrize("nx", ROW_NX)
def test_cc_row_lengths(backend, nx):
    """Rows around the multiples of the 8-voxel lane span and of the 512-voxel pass of k_cc_rows_wave."""
    m = _row_case(nx, 512)
    check_cc(backend, m, f"nx {nx}")
    check_cc(backend, 1 - m, f"nx {nx} complement")
    check_cc(backend, m[:1, :1], f"nx {nx}, one row")
    check_cc(backend, m[:, ::-1][:, :, ::-1].copy(), f"nx {nx} mirrored")


@pytest.mark.parametrize("nx", ROW_NX + [2049, 4100])
def test_cc_rows_with_run_boundaries_at_2048(backend, nx):
    """The same row lengths and two rows of several passes (2049, 4100) with the run boundaries placed around multiples of
    2048 voxels, and the complement of the 512-voxel cases."""
    for m in (_row_case(nx, 2048), 1 - _row_case(nx, 512)):
        check_cc(backend, m, f"nx {nx}")


def test_cc_degenerate_volumes(backend):
    for shape in [(1, 1, 1), (3, 4, 5), (1, 6, 9), (1, 1, 300), (7, 1, 1)]:
        ones, zeros = np.ones(shape, np.uint8), np.zeros(shape, np.uint8)
        got = check_cc(backend, ones, f"ones {shape}")
        assert got[True][1] == got[False][1] == ones.size
        got = check_cc(backend, zeros, f"zeros {shape}")           # no component: the input comes back, count 0
        assert got[True][1] == got[False][1] == 0
        one = zeros.copy()
        one.reshape(-1)[one.size // 2] = 1
        got = check_cc(backend, one, f"one voxel {shape}")
        assert got[False][1] == 1
    # nz = 1 (2-D): every voxel lies on the volume's border (z = 0), so no background is enclosed and nothing fills --
    # scipy's answer too for a 3-D volume one voxel thick (its outside reaches every voxel from above and below)
    ring = np.zeros((1, 9, 11), np.uint8)
    ring[0, 2:7, 2:9] = 1
    ring[0, 3:6, 3:8] = 0
    ring[0, 4, 5] = 1
    got = check_cc(backend, ring, "2-D ring")
    assert got[True][1] == 20 and got[False][1] == 20
    check_cc(backend, bernoulli((1, 40, 50), 0.55, 3), "2-D bernoulli")


@pytest.mark.parametrize("volume", ["serpentine", "bernoulli"])
def test_cc_repeat_calls_are_bit_identical(backend, volume):
    m = serpentine(CC_SHAPE) if volume == "serpentine" else bernoulli(CC_SHAPE, 0.31, seed=31)
    for fill in (True, False):
        a, ca = run_cc(backend, m, fill)
        b, cb = run_cc(backend, m, fill)
        np.testing.assert_array_equal(a, b)
        assert ca == cb


# --------------------------------------------------------------------------------------
# distance map and contour

def border26(mask):
    """Object voxels with a background voxel among their 26 neighbours inside the volume (the Maurer filter's zero set)."""
    obj = mask != 0
    p = np.pad(obj, 1, mode="constant", constant_values=True)        # outside the volume: never background
    near_bg = np.zeros(obj.shape, bool)
    nz, ny, nx = obj.shape
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                near_bg |= ~p[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    return obj & near_bg


def brute_edt(border, spacing):
    """fp64 minimum over all border voxels of the spacing-weighted distance (spacing is x, y, z)."""
    sp = np.array(spacing[::-1], np.float64)
    pts = np.argwhere(border).astype(np.float64) * sp
    vox = np.argwhere(np.ones(border.shape, bool)).astype(np.float64) * sp
    out = np.empty(len(vox))
    for s in range(0, len(vox), 512):
        d = vox[s:s + 512, None, :] - pts[None, :, :]
        out[s:s + 512] = np.sqrt((d * d).sum(-1)).min(1)
    return out.reshape(border.shape)


def distance_reference(mask, spacing):
    """(unsigned fp64 distance to the nearest border voxel, border mask); NO_BORDER everywhere without a border voxel."""
    border = border26(mask)
    if not border.any():
        return np.full(mask.shape, np.float64(NO_BORDER)), border
    d = ndimage.distance_transform_edt(~border, sampling=spacing[::-1])
    if mask.size <= BRUTE_MAX:
        np.testing.assert_allclose(brute_edt(border, spacing), d, rtol=1e-12, atol=1e-12, err_msg="brute force and scipy disagree")
    return d, border


def check_distance(backend, mask, spacing, label=""):
    """unsigned, signed and signed inside-positive maps of one mask at the ABI, every voxel."""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    d, border = distance_reference(mask, spacing)
    g = _lib.make_geom(size_of(mask.shape), spacing, (3.0, -7.0, 11.0))
    obj = mask != 0
    dm = backend.dev(mask)
    for signed, inside_positive in ((False, False), (True, False), (True, True)):
        want = d if not signed else np.where(obj != inside_positive, -d, d)
        out = backend.empty(mask.shape)
        backend.ctx.distance_map(dm, g, out, signed=signed, inside_positive=inside_positive)
        got = backend.host(out)
        tag = f"{label} {mask.shape} {spacing} signed={signed} inside_positive={inside_positive}"
        assert np.isfinite(got).all(), tag
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-5, err_msg=tag)
        assert (got[border] == 0.0).all(), tag
        np.testing.assert_array_equal(np.sign(got), np.sign(want), err_msg=tag)       # (also: non-zero off the border)


def _points(shape, pts):
    m = np.zeros(shape, np.uint8)
    for p in pts:
        m[p] = 1
    return m


def border_configurations(shape=(9, 10, 12)):
    nz, ny, nx = shape
    yield "corner voxel", _points(shape, [(0, 0, 0)])
    yield "far corner voxel", _points(shape, [(nz - 1, ny - 1, nx - 1)])
    yield "opposite corners", _points(shape, [(0, 0, 0), (nz - 1, ny - 1, nx - 1)])
    yield "other opposite corners", _points(shape, [(0, ny - 1, 0), (nz - 1, 0, nx - 1)])
    for ax in range(3):
        sl = [slice(None)] * 3
        sl[ax] = shape[ax] // 2
        plane = np.zeros(shape, np.uint8)
        plane[tuple(sl)] = 1
        yield f"plane across axis {ax}", plane
        line = np.zeros(shape, np.uint8)
        sl = [shape[0] // 3, shape[1] // 2, shape[2] - 2]
        sl[ax] = slice(None)
        line[tuple(sl)] = 1
        yield f"line along axis {ax}", line
    yield "one background voxel", 1 - _points(shape, [(nz // 2, ny // 3, nx - 3)])
    yield "one background voxel in a corner", 1 - _points(shape, [(0, 0, nx - 1)])
    # whole (x, y) columns and whole y-lines without a border voxel next to ones that hold some
    yield "z line and x line", _points(shape, [(slice(None), 0, 0), (nz - 2, ny - 2, slice(None))])
    yield "half a plane", _points(shape, [(2, slice(0, ny // 2), slice(nx // 2, None))])
    block = np.zeros(shape, np.uint8)
    block[1:-1, 2:-1, 3:-2] = 1                                   # a solid with an interior, off centre
    yield "block", block
    yield "block touching every face", np.pad(np.zeros((nz - 4, ny - 4, nx - 4), np.uint8), 2, constant_values=1)


BORDER_CONFIGURATIONS = dict(border_configurations())


@pytest.mark.parametrize("name", list(BORDER_CONFIGURATIONS))
def test_distance_border_configurations(backend, name):
    for spacing in [(1.0, 1.0, 1.0), (0.7, 1.3, 2.1)]:
        check_distance(backend, BORDER_CONFIGURATIONS[name], spacing, name)


ANISO = [((0.3, 1.0, 5.0), 2), ((5.0, 0.3, 1.0), 1), ((1.0, 5.0, 0.3), 0)]     # (spacing x y z, the fine axis of [Z][Y][X])


@pytest.mark.parametrize("kind", ["voxels", "solids"])
@pytest.mark.parametrize("spacing,fine", ANISO)
def test_distance_anisotropy(backend, spacing, fine, kind):
    """The long axis is the fine one: the nearest border voxel is often dozens of voxels along it although one a voxel or
    two across is in the volume; symmetric pairs make equidistant candidates."""
    shape = [5, 8, 5]
    shape[fine] = 90
    other = [a for a in range(3) if a != fine]

    def at(f, a, b):
        p = [0, 0, 0]
        p[fine], p[other[0]], p[other[1]] = f, a, b
        return tuple(p)

    if kind == "voxels":
        # isolated voxels (each is its own border): far along the fine axis, and pairs equidistant from the voxels between
        check_distance(backend, _points(shape, [at(0, 0, 0), at(89, 4, 4)]), spacing, "two far voxels")
        check_distance(backend, _points(shape, [at(10, 2, 2), at(70, 2, 2)]), spacing, "equidistant along the fine axis")
        check_distance(backend, _points(shape, [at(45, 0, 2), at(45, 4, 2), at(45, 2, 0), at(45, 2, 4)]), spacing, "equidistant across")
        check_distance(backend, _points(shape, [at(3, 1, 1), at(20, 3, 0), at(21, 0, 4), at(60, 2, 2), at(88, 4, 0)]), spacing, "scattered")
        return
    # a 3 x 3 bar along the fine axis: its core is interior; the nearest border is across, not along
    bar = np.zeros(shape, np.uint8)
    sl = [slice(1, 4)] * 3
    sl[fine] = slice(20, 75)
    bar[tuple(sl)] = 1
    check_distance(backend, bar, spacing, "bar")
    check_distance(backend, 1 - bar, spacing, "bar complement")
    check_distance(backend, bernoulli(tuple(shape), 0.02, 5), spacing, "sparse bernoulli")


@pytest.mark.parametrize("ny", [1, 2, 31, 32, 33, 65])
@pytest.mark.parametrize("nz", [1, 2])
def test_distance_transpose_tile_edges(backend, nz, ny):
    """nx and ny around the 32 x 32 tile of the x <-> y transpose."""
    spacing = (0.8, 1.25, 2.0)
    for nx in (1, 2, 31, 32, 33, 65):
        shape = (nz, ny, nx)
        m = bernoulli(shape, 0.03, seed=nx * 100 + ny)
        m[nz - 1, ny - 1, nx - 1] = 1
        m[0, 0, 0] = 0 if m.size > 1 else 1
        m[0, ny // 2:ny // 2 + 4, nx // 3:nx // 3 + 5] = 1           # a block with an interior when ny, nx allow
        check_distance(backend, m, spacing, "tile edges")


def test_distance_more_slices_than_transpose_blocks(backend):
    """nz = 1030 > the 1024-block cap of the transpose grid's z; fine spacing along z, so that distances of hundreds of
    voxels are sums along z."""
    shape = (1030, 3, 5)
    m = _points(shape, [(0, 0, 0), (1029, 2, 4), (1026, 1, 2), (700, 0, 3)])
    check_distance(backend, m, (1.0, 5.0, 0.3), "tall")
    m = np.ones(shape, np.uint8)
    m[1027, 1, 1] = 0
    m[3, 2, 4] = 0
    check_distance(backend, m, (0.9, 1.1, 2.5), "tall, mostly object")


def test_distance_without_a_border_voxel(backend):
    """An empty mask and an all-ones mask have no border voxel; ITK and scipy give no usable reference.  The kernel
    returns sqrtf(1e18f) = 1e9 (finite) at every voxel, with the sign of the voxel's side ("No border voxel")."""
    for shape in [(4, 6, 9), (1, 1, 1), (2, 33, 65)]:
        g = _lib.make_geom(size_of(shape), (0.9, 1.1, 2.5), (0.0, 0.0, 0.0))
        for value in (0, 1):
            m = np.full(shape, value, np.uint8)
            for signed, inside_positive in ((False, False), (True, False), (True, True)):
                out = backend.empty(shape)
                backend.ctx.distance_map(backend.dev(m), g, out, signed=signed, inside_positive=inside_positive)
                got = backend.host(out)
                sign = 1.0 if not signed else (1.0 if bool(value) == inside_positive else -1.0)
                assert np.isfinite(got).all()
                np.testing.assert_array_equal(got, np.full(shape, sign * NO_BORDER, np.float32))
            check_distance(backend, m, (0.9, 1.1, 2.5), "no border")


def contour_reference(mask):
    """Object voxels with a face neighbour of another value; voxels outside the volume are no neighbours."""
    obj = mask != 0
    cross = ndimage.generate_binary_structure(3, 1)
    want = obj & ~ndimage.binary_erosion(obj, structure=cross, border_value=1)
    np.testing.assert_array_equal(want.astype(np.uint8), O.label_contour(O.Vol(mask, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))).arr)
    return want.astype(np.uint8)


def test_label_contour(backend):
    solid = np.ones((9, 10, 12), np.uint8)
    dented = solid.copy()
    dented[0, 0, 0] = dented[4, 5, 6] = dented[8, 9, 5] = dented[3, 0, 11] = 0
    cases = [checkerboard((9, 12, 13)), 1 - checkerboard((9, 12, 13)), checkerboard(CC_SHAPE)]
    cases += [nested_shells(opening=o) for o in (None, "face", "edge", "corner")]
    cases += [solid, dented, np.zeros((3, 4, 5), np.uint8), np.ones((1, 1, 1), np.uint8), bernoulli((1, 33, 70), 0.5, 2),
              bernoulli((30, 1, 1), 0.5, 2), bernoulli(CC_SHAPE, 0.6, 9)]
    for m in cases:
        out = backend.empty(m.shape, np.uint8)
        backend.ctx.label_contour(backend.dev(m), size_of(m.shape), out)
        np.testing.assert_array_equal(backend.host(out), contour_reference(m))
    out = backend.empty(solid.shape, np.uint8)
    backend.ctx.label_contour(backend.dev(solid), size_of(solid.shape), out)
    assert backend.host(out).sum() == 0                               # the whole volume: no voxel differs from a neighbour


# --------------------------------------------------------------------------------------
# ball morphology

DILATE, ERODE, CLOSE = 0, 1, 2
MORPH_REF = {DILATE: O.binary_dilate_ball, ERODE: O.binary_erode_ball, CLOSE: O.binary_closing_ball}


def run_morph(backend, m, radius, op):
    out = backend.empty(m.shape, np.uint8)
    backend.ctx.binary_morph_ball(backend.dev(m), size_of(m.shape), radius, op, out)
    return backend.host(out).copy()


def brute_morph(m, radius, op):
    """The three operations from their definitions, voxel by voxel (tiny volumes): dilation stamps the element on every
    foreground voxel, into a grid padded by the radius; erosion keeps a voxel whose whole element window is foreground,
    the outside counting as foreground; closing erodes the PADDED dilation back onto the original grid (safe border)."""
    rx, ry, rz = radius
    el = O.ball_element(radius)
    obj = m != 0
    nz, ny, nx = m.shape

    def dilate_padded(a):
        out = np.zeros((nz + 2 * rz, ny + 2 * ry, nx + 2 * rx), bool)
        for z, y, x in np.argwhere(a):
            out[z:z + 2 * rz + 1, y:y + 2 * ry + 1, x:x + 2 * rx + 1] |= el
        return out

    def erode_padded(p):        # p: the grid padded by the radius -> the original grid
        out = np.zeros(m.shape, bool)
        for z, y, x in np.ndindex(*m.shape):
            out[z, y, x] = p[z:z + 2 * rz + 1, y:y + 2 * ry + 1, x:x + 2 * rx + 1][el].all()
        return out

    if op == DILATE:
        return dilate_padded(obj)[rz:rz + nz, ry:ry + ny, rx:rx + nx].astype(np.uint8)
    if op == ERODE:
        return erode_padded(np.pad(obj, [(rz, rz), (ry, ry), (rx, rx)], constant_values=True)).astype(np.uint8)
    return erode_padded(dilate_padded(obj)).astype(np.uint8)


MORPH_BRUTE_MAX = 256


def check_morph(backend, m, radius, ops=(DILATE, ERODE, CLOSE), label="", scipy_ops=(DILATE, ERODE, CLOSE)):
    """scipy_ops: the ops also held to scipy (the oracle); tiny volumes are held to brute_morph as well."""
    vol = O.Vol(np.ascontiguousarray(m, dtype=np.uint8), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert m.size <= MORPH_BRUTE_MAX or set(ops) <= set(scipy_ops)
    got = {}
    for op in ops:
        got[op] = run_morph(backend, vol.arr, radius, op)
        if op in scipy_ops:
            np.testing.assert_array_equal(got[op], MORPH_REF[op](vol, radius).arr, err_msg=f"{label} radius {radius} op {op}")
        if m.size <= MORPH_BRUTE_MAX:
            np.testing.assert_array_equal(got[op], brute_morph(vol.arr, radius, op), err_msg=f"{label} radius {radius} op {op} (brute)")
    return got


@pytest.mark.parametrize("radius", [(r, r, r) for r in range(16)] + [(15, 0, 1), (0, 15, 0), (1, 2, 15), (15, 15, 0)])
def test_morph_dilated_voxel_is_the_ball(backend, radius):
    """Dilating one voxel stamps the element: make_ball and the table's indexing, apart from the scan."""
    rx, ry, rz = radius
    shape = (2 * rz + 3, 2 * ry + 3, 2 * rx + 3)
    m = np.zeros(shape, np.uint8)
    m[rz + 1, ry + 1, rx + 1] = 1
    want = np.zeros(shape, np.uint8)
    want[1:-1, 1:-1, 1:-1] = O.ball_element(radius)
    np.testing.assert_array_equal(run_morph(backend, m, radius, DILATE), want)
    # eroding the complement removes exactly the same voxels (the element is symmetric)
    np.testing.assert_array_equal(run_morph(backend, 1 - m, radius, ERODE), 1 - want)


def test_morph_ball_element_by_hand():
    """The element the tests above stamp, restated with exact rational arithmetic: d in the ball iff
    sum_i (2 d_i)^2 / (2 r_i + 1)^2 <= 1."""
    from fractions import Fraction

    for radius in [(0, 0, 0), (1, 1, 1), (2, 3, 1), (5, 5, 5), (15, 0, 1), (15, 15, 15)]:
        rx, ry, rz = radius
        e = O.ball_element(radius)
        assert e.shape == (2 * rz + 1, 2 * ry + 1, 2 * rx + 1)
        for z in range(-rz, rz + 1):
            for y in range(-ry, ry + 1):
                for x in range(-rx, rx + 1):
                    s = Fraction(4 * x * x, (2 * rx + 1) ** 2) + Fraction(4 * y * y, (2 * ry + 1) ** 2) + Fraction(4 * z * z, (2 * rz + 1) ** 2)
                    # no lattice point lies ON the surface: 4 (x^2 b^2 c^2 + ...) is even, (a b c)^2 with a = 2 r + 1 odd;
                    # off it |s - 1| >= 31^-6, far above fp64 rounding -- so `<= 1` and `< 1` select the same element
                    assert s != 1
                    assert bool(e[z + rz, y + ry, x + rx]) == (s < 1), (radius, x, y, z)


@pytest.mark.parametrize("radius", [(15, 15, 15), (15, 1, 0), (0, 7, 15)])
def test_morph_radius_larger_than_the_volume(backend, radius):
    """All three ops.  scipy needs half a minute for one closing with the 31^3 element on the padded grid: there the
    brute-force restatement is the reference, and scipy for the dilation and the erosion of one mask."""
    shape = (5, 6, 7)
    big = radius == (15, 15, 15)
    check_morph(backend, bernoulli(shape, 0.3, 4), radius, label="bernoulli", scipy_ops=(DILATE, ERODE) if big else (DILATE, ERODE, CLOSE))
    for label, m in [("one voxel", _points(shape, [(2, 3, 3)])), ("one hole", 1 - _points(shape, [(0, 5, 6)])),
                     ("sparse", bernoulli(shape, 0.03, 9)), ("dense", bernoulli(shape, 0.97, 9)),
                     ("1x1x1", np.ones((1, 1, 1), np.uint8)), ("1x1x1 empty", np.zeros((1, 1, 1), np.uint8))]:
        check_morph(backend, m, radius, label=label, scipy_ops=() if big else (DILATE, ERODE, CLOSE))


@pytest.mark.parametrize("radius", [(1, 1, 1), (3, 2, 1), (4, 4, 4), (0, 0, 2)])
def test_morph_objects_on_the_faces(backend, radius):
    shape = (9, 11, 13)
    ones, zeros = np.ones(shape, np.uint8), np.zeros(shape, np.uint8)
    got = check_morph(backend, ones, radius, label="ones")
    np.testing.assert_array_equal(got[ERODE], ones)               # the boundary counts as foreground
    got = check_morph(backend, zeros, radius, label="zeros")
    np.testing.assert_array_equal(got[DILATE], zeros)
    for corner in [(0, 0, 0), (8, 10, 12), (0, 10, 0), (8, 0, 12)]:
        m = zeros.copy()
        sl = tuple(slice(0, 4) if c == 0 else slice(s - 4, s) for c, s in zip(corner, shape))
        m[sl] = 1
        m[corner] = 0                                            # a notch in the very corner
        m[4, 5, 6] = 1
        got = check_morph(backend, m, radius, label=f"corner {corner}")
        assert (got[CLOSE] >= m).all()                           # closing is extensive, at the border too (safe border)
    faces = np.pad(np.zeros((5, 7, 9), np.uint8), 2, constant_values=1)      # a shell on all six faces
    check_morph(backend, faces, radius, label="six faces")
    check_morph(backend, 1 - faces, radius, label="inside of six faces")


@pytest.mark.parametrize("radius", [(3, 2, 1), (1, 1, 1), (2, 5, 3)])
def test_morph_duality(backend, radius):
    """erode(m) = 1 - dilate(1 - m) further than the radius from the buffer's edge (at the edge the two ops assume
    opposite outsides); both equal scipy over the whole volume."""
    shape = (50, 70, 60)
    rx, ry, rz = radius
    n_el = int(O.ball_element(radius).sum())
    m = bernoulli(shape, 0.5 ** (1.0 / n_el), seed=rx + 10 * ry)     # about half of the interior survives the erosion
    er = check_morph(backend, m, radius, ops=(ERODE,))[ERODE]
    di = check_morph(backend, 1 - m, radius, ops=(DILATE,))[DILATE]
    inner = (slice(rz + 1, shape[0] - rz - 1), slice(ry + 1, shape[1] - ry - 1), slice(rx + 1, shape[2] - rx - 1))
    np.testing.assert_array_equal(er[inner], 1 - di[inner])
    assert 0.2 < er[inner].mean() < 0.8


def test_morph_refuses_radii_outside_the_table(backend):
    m = backend.dev(np.zeros((4, 5, 6), np.uint8))
    out = backend.empty((4, 5, 6), np.uint8)
    for radius in [(16, 1, 1), (1, 16, 1), (1, 1, 16), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (16, 16, 16)]:
        for op in (DILATE, ERODE, CLOSE):
            with pytest.raises(_lib.PlatipyAmdError):
                backend.ctx.binary_morph_ball(m, (6, 5, 4), radius, op, out)
    backend.ctx.binary_morph_ball(m, (6, 5, 4), (15, 15, 15), DILATE, out)      # the table's last radius is accepted


# --------------------------------------------------------------------------------------
# bounding box

def box_reference(a):
    zz, yy, xx = np.nonzero(a > 0)
    return [int(v) for v in (xx.min(), xx.max(), yy.min(), yy.max(), zz.min(), zz.max())]


def run_box(backend, a):
    return backend.ctx.bounding_box(backend.dev(a), size_of(a.shape), a.dtype == np.float32)


def is_empty_box(box):
    return box[0] > box[1] and box[2] > box[3] and box[4] > box[5]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_bounding_box_edges(backend, dtype):
    # 16900 rows of 3 voxels: more than 4096 blocks x 4 rows cover in one step
    shape = (130, 130, 3)
    assert shape[0] * shape[1] > 4096 * 4
    a = np.zeros(shape, dtype)
    assert is_empty_box(run_box(backend, a))
    a[129, 129, 2] = 1                                  # the very last voxel, in a row only the second step reaches
    assert run_box(backend, a) == [2, 2, 129, 129, 129, 129]
    a[126, 5, 0] = 2                                    # row 16385: second step too
    assert run_box(backend, a) == box_reference(a)
    a[0, 0, 0] = 1
    assert run_box(backend, a) == [0, 2, 0, 129, 0, 129]
    a[:] = 0
    a[0, 0, 0] = 1                                      # index 0 alone
    assert run_box(backend, a) == [0, 0, 0, 0, 0, 0]
    a = (np.random.default_rng(3).random(shape) > 0.999).astype(dtype)
    assert run_box(backend, a) == box_reference(a)
    # nx = 1
    a = np.zeros((5, 7, 1), dtype)
    assert is_empty_box(run_box(backend, a))
    a[4, 6, 0] = 1
    assert run_box(backend, a) == [0, 0, 6, 6, 4, 4]
    a[1, 2, 0] = 1
    assert run_box(backend, a) == [0, 0, 2, 6, 1, 4]
    a = np.ones((1, 1, 1), dtype)
    assert run_box(backend, a) == [0, 0, 0, 0, 0, 0]
    # rows longer than a wavefront's 64-voxel step, last and first voxel of the row
    a = np.zeros((2, 3, 131), dtype)
    a[1, 2, 130] = a[0, 1, 64] = 1
    assert run_box(backend, a) == [64, 130, 1, 2, 0, 1]


def test_bounding_box_float_values_that_are_not_positive(backend):
    """Negatives, -0.0, NaN and -inf are not > 0."""
    shape = (4, 9, 70)
    rng = np.random.default_rng(6)
    a = -rng.random(shape).astype(np.float32)
    a[rng.random(shape) < 0.3] = -0.0
    a[rng.random(shape) < 0.3] = np.nan
    a[rng.random(shape) < 0.1] = 0.0
    a[0, 0, 0], a[3, 8, 69] = np.nan, -np.inf
    assert is_empty_box(run_box(backend, a))
    a[2, 5, 66] = np.float32(1e-40)                     # the smallest things that are: a subnormal ...
    assert run_box(backend, a) == [66, 66, 5, 5, 2, 2]
    a[1, 7, 3] = np.inf                                 # ... and +inf
    assert run_box(backend, a) == [3, 66, 5, 7, 1, 2]
    assert run_box(backend, a) == box_reference(a)
