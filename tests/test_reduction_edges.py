"""The block reductions behind the C ABI (pp_block_tree, pp_block_range_store, k_range_fold, the arg-max pair of
pp_cc.hip; platipy_amd/csrc/pp_reduce.h) at the sizes where a fold can go wrong: one element, one thread short of / over a
block, 257 blocks (a one-block fold of the partials takes its second strided trip above NT = 256 blocks) and one element
past the launcher's grid cap (the partial kernel's second grid-stride trip).

Every expectation is exact against numpy or scipy -- min / max, integer counts, arg-max -- except the fp64 sums of
pp_surface_stats_f32 and STAPLE's rates, which carry the bounds of tests/test_comparison.py::test_abi_surface_stats
(rtol 1e-12) and tests/test_staple.py::_check (atol 1e-12; the image: atol 1e-7)."""
import numpy as np
import pytest
from scipy import ndimage

from platipy_amd import _lib
from tests import bronchus_restatement as BR
from tests import staple_restatement as SR
from tests.test_mask_kernels import _first_largest, run_cc, size_of

NT = 256
GRID_CAP = 2048          # blocks of the partial kernels of pp_abs_range_f32, pp_fillhole_largest_component_u8, k_rg_select


# --------------------------------------------------------------------------------------
# pp_abs_range_f32: k_abs_range_partial + k_range_fold<float>

def _planted(n, seed):
    """(array, position of the largest |value|, position of the smallest) for every pairing of the positions 0, n - 1 and
    65536 (the first element of block 256) that n allows.  Magnitudes lie in [1, 2) with random signs; the planted values
    are negative, so a reduction without the fabsf returns them as minima."""
    rng = np.random.default_rng(seed)
    base = (rng.uniform(1.0, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    pos = sorted({0, n - 1} | ({65536} if n > 65536 else set()))
    for k, hi_at in enumerate(pos):
        lo_at = pos[(k + 1) % len(pos)]
        x = base.copy()
        x[lo_at] = -0.125
        x[hi_at] = -8.0          # (n == 1: the one element is both)
        yield x, hi_at, lo_at


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537, GRID_CAP * NT + 1])
def test_abs_range_sizes(backend, n):
    be = backend
    for x, hi_at, lo_at in _planted(n, seed=n):
        rng = be.empty((2,), np.float32)
        be.ctx.abs_range(be.dev(x), n, rng)
        lo, hi = be.host(rng)
        want = np.abs(x)
        assert (lo, hi) == (want.min(), want.max()), (n, hi_at, lo_at)
        assert hi == 8.0 and lo == (0.125 if n > 1 else 8.0)


# --------------------------------------------------------------------------------------
# pp_surface_stats_f32, PP_SURFACE_NONZERO: 257 blocks on the 16-byte arm, all samples in the last block

def test_surface_stats_257_blocks(backend):
    be = backend
    shape = (1, 1025, 1024)                       # [Z][Y][X], flat: 16 * 65600 voxels
    n = shape[0] * shape[1] * shape[2]
    assert n % 16 == 0 and n // 16 > NT * NT      # more than 256 blocks of 16-voxel lanes
    rng = np.random.default_rng(41)
    dist = rng.normal(scale=4.0, size=shape).astype(np.float32)
    sel = np.zeros(n, np.uint8)
    sel[n - 4096:] = rng.integers(0, 3, size=4096).astype(np.uint8) * 100      # about two thirds of the last 4096, nothing else
    sel[n - 1] = 7
    dist.reshape(-1)[0] = 1000.0                  # not selected: must not show
    sel = sel.reshape(shape)
    dsel, ddist = be.dev(sel), be.dev(dist)
    assert _lib.ptr(dsel) % 16 == 0               # the 16-byte arm
    geom = _lib.make_geom(size_of(shape), (0.9, 1.1, 2.5))
    drange = be.empty((2,), np.float32)
    be.ctx.abs_range(ddist, n, drange)
    lo, hi = be.host(drange)
    assert lo == np.abs(dist).min() and hi == 1000.0
    out = be.empty((_lib.SURFACE_STATS_DTYPE.itemsize,), np.uint8)
    tau = 1.25
    be.ctx.surface_stats(dsel, ddist, geom, _lib.SURFACE_NONZERO, out, tau=tau, device_range=drange)
    rec = be.host(out).view(_lib.SURFACE_STATS_DTYPE)[0]
    v = dist[sel != 0]
    v64 = v.astype(np.float64)
    assert 2000 < v.size < 4096
    assert rec["count"] == v.size
    assert rec["count_le_tau"] == int((v64 <= tau).sum())
    assert rec["min"] == v.min() and rec["max"] == v.max()
    assert np.isclose(rec["sum"], v64.sum(), rtol=1e-12, atol=1e-12) and np.isclose(rec["sum_sq"], (v64 * v64).sum(), rtol=1e-12)
    x = (v64 - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * 128.0
    want = np.bincount(np.where(x >= 127, 127, np.maximum(x, 0).astype(np.int64)), minlength=128)
    assert rec["hist"].sum() == rec["count"] and np.array_equal(rec["hist"], want)


# --------------------------------------------------------------------------------------
# pp_staple_fuse with rescale: k_staple_wminmax + k_range_fold<double> over more than 256 blocks of mixed keys

STAPLE_ITERATIONS = 3


@pytest.mark.parametrize("agree", [1, 0])
def test_staple_rescale_257_blocks(backend, agree):
    """Two raters that disagree on 65536 + 300 voxels (257 blocks of mixed keys) and agree -- both `agree` -- on 1500 more.
    Rater 0 alone marks the mixed voxels, except the last 200 of them, which rater 1 alone marks: that key, and with it one
    end of W's range over the mixed keys, exists only in block 256, which the fold reaches on its second trip.  The other
    uniform class is absent, so that end of the range comes from the fold alone (agree = 1: the minimum, 0: the maximum, or
    the other way round -- the two cases mirror each other)."""
    be = backend
    nm, na = NT * NT + 300, 1500
    n = nm + na
    rng = np.random.default_rng(5)
    mixed = np.ones(n, bool)
    mixed[rng.choice(NT * NT, size=na, replace=False)] = False          # the agreeing voxels sit among the first blocks
    at = np.flatnonzero(mixed)
    assert at.size == nm and at[NT * NT] > NT * NT
    r0 = np.full(n, agree, np.uint8)
    r1 = np.full(n, agree, np.uint8)
    r0[at[:nm - 200]], r1[at[:nm - 200]] = 1, 0
    r0[at[nm - 200:]], r1[at[nm - 200:]] = 0, 1
    labels = [r0, r1]
    w, p, q, it, degenerate = SR.staple_patterns(labels, maximum_iterations=STAPLE_ITERATIONS)
    assert it == STAPLE_ITERATIONS and not degenerate
    w_mixed = w[at]
    assert w_mixed[-1] != w_mixed[0] and w_mixed[-1] in (w.min(), w.max())   # block 256 holds one end of the range
    want = SR.rescale_threshold(w, 0)
    runs = []
    for _ in range(2):
        out = be.dev(np.full(n, -1.0, np.float64))
        res = be.ctx.staple([be.dev(x) for x in labels], False, n, out, _lib.STAPLE_FOREGROUND, maximum_iterations=STAPLE_ITERATIONS,
                            rescale=True)
        got = be.host(out).copy()
        assert res.n_mixed == nm and not res.degenerate and res.elapsed_iterations == STAPLE_ITERATIONS
        assert got.min() == 0.0 and got.max() == 1.0
        np.testing.assert_allclose([res.sensitivity[0], res.sensitivity[1]], p, rtol=0, atol=1e-12)
        np.testing.assert_allclose([res.specificity[0], res.specificity[1]], q, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-7)
        runs.append((got.tobytes(), bytes(res)))
    assert runs[0] == runs[1]


# --------------------------------------------------------------------------------------
# pp_fillhole_largest_component_u8: k_cc_argmax + k_cc_argmax_final over more than 256 blocks

CC_SHAPE = (40, 41, 41)          # 67240 voxels: 263 blocks of the arg-max


def _check_largest(be, m):
    want, count = _first_largest(ndimage.label(m)[0])
    out, cnt = run_cc(be, m, False)
    np.testing.assert_array_equal(out, want)
    assert cnt == count
    return out, cnt


def test_largest_component_tie_across_the_fold(backend):
    """Two components of 6 voxels: the root of the one that must win lies in block 1, the other's in block 257 -- both are
    folded by thread 1 of the final kernel, the loser on its second trip -- and smaller ones in blocks 0, 256 and 262."""
    m = np.zeros(CC_SHAPE, np.uint8)
    assert m.size > NT * NT
    flat = m.reshape(-1)
    win, lose = NT + 10, 257 * NT + 2
    assert (win % 41) + 6 <= 41 and (lose % 41) + 6 <= 41            # each run stays inside one x-row
    flat[win:win + 6] = 1
    flat[lose:lose + 6] = 1
    flat[3:6] = 1
    flat[256 * NT + 1:256 * NT + 5] = 1
    flat[m.size - 5:] = 1
    out, cnt = _check_largest(backend, m)
    assert cnt == 6 and out.reshape(-1)[win] == 1 and out.sum() == 6


def test_largest_component_in_the_last_256_voxels(backend):
    m = np.zeros(CC_SHAPE, np.uint8)
    m.reshape(-1)[m.size - 7:m.size - 2] = 1
    out, cnt = _check_largest(backend, m)
    assert cnt == 5 and out.sum() == 5


# --------------------------------------------------------------------------------------
# pp_connected_threshold_f32: the voxel count of k_rg_select (block tree, then one integer atomic per block)

@pytest.mark.parametrize("shape", [(1, 1, 257), (2, 513, 512)])
def test_region_growing_voxel_count(backend, shape):
    """One row of 257 voxels (two blocks, the second with one voxel), all of it grown; and a volume just larger than the
    2048-block grid of k_rg_select, so that every thread of the first 1024 rows' worth adds voxels of two grid-stride trips,
    with holes that the count must leave out."""
    be = backend
    n = shape[0] * shape[1] * shape[2]
    assert n == 257 or n > GRID_CAP * NT
    img = np.full(shape, 2.0, np.float32)
    if n > 257:
        img.reshape(-1)[np.random.default_rng(n).choice(n, size=n // 50, replace=False)] = 9.0     # holes in the region
        img.reshape(-1)[[0, n - 1]] = 2.0
    seeds = [[0, 0, 0]]
    want = BR.connected_threshold(img, seeds, 1.0, 3.0)
    assert want.reshape(-1)[n - 1] == 1 and (int(want.sum()) == 257 if n == 257 else n // 2 < int(want.sum()) < n)
    out = be.dev(np.full(shape, 7, np.uint8))
    vox = be.ctx.connected_threshold(be.dev(img), size_of(shape), 1.0, 3.0, seeds, out)
    assert vox == int(want.sum())
    assert np.array_equal(be.host(out), want)
