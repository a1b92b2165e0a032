"""The label-fusion map and reduction kernels at the head of pp_fusion.hip (k_map4<Op> with its seven functors, k_ssd_partial /
k_sum_final, k_minmax_partial / k_range_fold<float>) at the C ABI against the numpy / fp64 restatements of
tests/fusion_restatement.py, on every arm ("Fusion arithmetic, which call enters which arm of k_map4"):

  sizes       N_EDGE: n < 4, n % 4 = 0 .. 3, one voxel either side of a block (256) and of a block of 16-byte quads (1024);
              N_STRIDE = 2048 * 256 * 4 + 4 * 256 * 3 + 3: a second grid-stride trip of the vector arm (cap 2048 blocks x 256
              lanes x 4 voxels), a three-voxel tail, and a fifth trip of the scalar arm and of both reductions (cap 2048 x 256).
  alignment   every pointer 16-byte aligned, and each pointer of the call moved off 16 bytes in turn (uint8 arrays by 1, 2 and
              3 bytes): the results are bit-identical to each other and to the reference.  Unaligned 16-byte global accesses do
              not fault on this hardware, so these cases do not test the alignment predicate; they pin the arithmetic and the
              indexing of the scalar arm (vec == 0), which the product enters with rows of a stacked buffer whenever the
              voxel count is not a multiple of 4 (projects/multiatlas.py, buf[1 + k]).
  canaries    four elements before and after every view the call may write are checked unchanged.

Bounds (u = 2^-24; derived, not tuned; the measured maxima go to record_stats("fusion_kernels")):

  op_fuse_divide, op_binary_threshold, wsum      bit-exact: no contractible expression, fp32 / and fp64 / correctly rounded.
  op_sqdiff   has no entry point of its own.  Through pp_weight_map_block_f32 with radius 0 (the box mean is fmaf(1, v, 0) = v)
              it is seen through factor * powf(1 / sq, p): held to the powf bound below against the bit-exact numpy square.
  wlsum       a * b + c may be contracted: every element equals the fold with the product rounded first, or the fold of fused
              multiply-adds (w * l + acc exactly, one rounding).  With labels 0 / 1 the two coincide: bit-exact.
  op_rescale_threshold   x * scale + shift in double may be contracted: every element equals one of the two evaluations; random
              inputs keep the rescaled value 2^-20 from `lower`, the exact sets are exact either way.
  pp_sum_sq_diff_f32     relative error against math.fsum <= (k + 8 + ceil(nb / 256) + 8 + 2) 2^-53, nb = min(ceil(n / 256), 2048)
              blocks, k = ceil(n / (256 nb)) terms a thread: k serial additions, the 8 levels of pp_block_sum3's tree over 256
              threads, ceil(nb / 256) serial additions and 8 tree levels of k_sum_final, one rounding each for d and d * d (the
              reference rounds them too; a contracted d * d + s does not).  All terms are non-negative, so the relative errors
              add and no cancellation enters.  a == b gives exactly 0.
  pp_minmax_f32          exact (==) against ITK's rule; repeated calls of both reductions are bit-identical.
  pp_weight_map_local_f32   |got - want| <= B_fir / (raw + eps)^2 + 3 u want, B_fir = u max|sq| sum_axes (2 r_axis + 2): the FIR
              bound of tests/test_smoothing_kernels.py on the squared-difference image, through d(1 / x) = dx / x^2; 3 u for
              the fp32 eps, the add and the divide.  t == m gives 1 / eps exactly as fp32 computes it.
  pp_weight_map_block_f32   f(mean + B) - POWF_ULP ulp32 <= got <= f(mean - B) + POWF_ULP ulp32, f(x) = factor x^-p,
              p = |gain / 2| -- to first order |got - want| <= want p B / mean + POWF_ULP ulp32(want); f is monotone, so the
              interval is that bound without its dropped second-order term.  B = u max_box|sq| sum_axes (2 r_axis + 3): the FIR
              derivation with taps 1 / (2 r + 1) -- every value a pass sums lies under the voxel's box, hence the maximum over
              the box -- and one more u per axis because the kernel's fp32 tap is the exact tap times (1 + d), |d| <= u.
              Where every voxel under the box has t == m the mean is exactly 0 on both sides and the weight is exactly
              +inf (p > 0) or factor (p = 0).
              POWF_ULP: 1 / x, powf and the multiply.  With no documented accuracy of the device powf to cite, it is
              the largest distance measured on an MI355X on inputs whose box mean is exact (radius 0), plus 1, and may not
              exceed 8: test_block_weight_powf_distance measures it again on every run and asserts it.  For
              comparison: 1 / x errs by u relative, p <= 2 doubles it (<= 2 ulp), a powf good to 1 ulp and the multiply's half
              ulp would give 3.5; the card measures 2.71, the CPU build 2.35.
"""
import itertools

import numpy as np
import pytest

from platipy_amd import _lib
from tests import fusion_restatement as R
from tests.helpers import record_stats

U24 = 2.0 ** -24
N_EDGE = [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 1027]
N_STRIDE = 2048 * 256 * 4 + 4 * 256 * 3 + 3
N_MATRIX = [7, 1027]
PAD = 4
CANARY = {np.dtype(np.float32): np.float32(-7.25e33), np.dtype(np.uint8): np.uint8(0xA5)}
POWF_ULP = 3.75         # measured on the card: 2.711 ulp (profiles/fusion_kernels.json), plus 1, rounded up to a quarter
_STATS = {}


def note(be, op, **figures):
    """Keep the largest value of every figure per operation and backend."""
    slot = _STATS.setdefault(be.name + ":" + op, {})
    for k, v in figures.items():
        slot[k] = max(float(v), slot.get(k, float("-inf")))
    record_stats("fusion_kernels", _STATS)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Placed:
    """`a` on the backend inside a larger allocation: its first element `off` bytes past a 16-byte boundary, PAD canary
    elements either side (the offset_view of tests/test_smoothing_kernels.py, with canaries and byte offsets)."""

    def __init__(self, be, a, off=0):
        a = np.ascontiguousarray(a)
        self.n, self.shape, self.dtype = a.size, a.shape, a.dtype
        self.flat = be.empty((a.size + 2 * PAD + 32,), np.uint8 if a.dtype == np.uint8 else np.float32)
        self.flat[...] = CANARY[a.dtype].item()
        s = PAD
        while (_lib.ptr(self.flat) + s * a.dtype.itemsize) % 16 != off:
            s += 1
        self.s = s
        self.v = self.flat[s:s + a.size]
        self.v[...] = be.dev(a.ravel())
        assert _lib.ptr(self.v) % 16 == off

    def result(self, be):
        h = np.asarray(be.host(self.flat))
        c = CANARY[self.dtype]
        assert (h[self.s - PAD:self.s] == c).all() and (h[self.s + self.n:self.s + self.n + PAD] == c).all(), "canary overwritten"
        return h[self.s:self.s + self.n].reshape(self.shape).copy()


def offsets_matrix(roles):
    """{}: every pointer aligned; then each pointer moved in turn.  roles: name -> "f" (float32: 4 bytes) or "b" (uint8: 1, 2, 3)."""
    yield {}
    for name, kind in roles.items():
        for off in ((4,) if kind == "f" else (1, 2, 3)):
            yield {name: off}


def sizes_and_offsets(roles):
    """(n, offsets) of every case of a flat operation: N_EDGE aligned, the matrix at N_MATRIX, N_STRIDE aligned and once with
    its first pointer off (the scalar arm's grid-stride loop)."""
    out = [(n, {}) for n in N_EDGE if n not in N_MATRIX]
    out += [(n, o) for n in N_MATRIX for o in offsets_matrix(roles)]
    first = next(iter(roles))
    return out + [(N_STRIDE, {}), (N_STRIDE, {first: 4})]


def case_id(v):
    n, o = v
    return str(n) + "".join(f"-{k}+{b}" for k, b in o.items())


def rng_for(n, salt):
    return np.random.default_rng(1000003 * salt + n)


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, (what, bad[:5], np.asarray(got).ravel()[bad[:5]], np.asarray(want).ravel()[bad[:5]])


def assert_one_of(got, cand_a, cand_b, what):
    ok = (bits(got) == bits(cand_a)) | (bits(got) == bits(cand_b))
    bad = np.flatnonzero(~ok.ravel())
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], cand_a.ravel()[bad[:5]], cand_b.ravel()[bad[:5]])
    return int((bits(got) != bits(cand_a)).sum())


_ALIGNED = {}


def same_as_aligned(key, offs, got):
    """The aligned call of a case runs first (offsets_matrix yields it first); every offset call must reproduce its bits."""
    if not offs:
        _ALIGNED[key] = [g.copy() for g in got]
    elif key in _ALIGNED:
        for g, a in zip(got, _ALIGNED[key]):
            assert_same_bits(g, a, ("offset call differs from the aligned call", key, offs))


# --------------------------------------------------------------------------------------
# the restatement itself, by hand (CPU only)


def test_squared_difference_and_ssd_by_hand():
    t, m = np.float32([3.0, -1.5, 1e20, 0.1]), np.float32([1.0, 2.5, -1e20, 0.1])
    assert R.squared_difference(t, m).tolist() == [4.0, 16.0, np.inf, 0.0]        # (2e20)^2 overflows fp32
    assert R.ssd(t[:2], m[:2]) == 20.0
    assert R.ssd(t, m) == (2.0 * float(np.float32(1e20))) ** 2                    # fp64 squares: finite; 20 is below half an ulp
    # 2^54 + 1 + 1 + 1: a running fp64 sum stays at 2^54 (ulp 4), the exact sum 2^54 + 3 rounds to 2^54 + 4
    assert R.ssd(np.float32([2.0 ** 27, 1.0, 1.0, 1.0]), np.zeros(4, np.float32)) == 2.0 ** 54 + 4.0


def test_local_weight_by_hand(emu_backend):
    """Three voxels in a row, sigma 0.5: every tap written out against the clamped index; the y and z passes of a one-voxel
    axis multiply by the sum of the taps."""
    t, m = np.float32([1.0, 3.0, 0.0]), np.float32([0.0, 1.0, 2.0])
    sq = [1.0, 4.0, 4.0]
    w, raw, radii = R.local_weight(t, m, (3, 1, 1), (1.0, 1.0, 1.0), 0.5, 0.5, lib=emu_backend.lib)
    taps = np.float32(_lib.gauss_taps(0.25, 0.01, 32, lib=emu_backend.lib)).astype(np.float64)
    r = (taps.size - 1) // 2
    assert r >= 1 and radii == [r, r, r]
    row = [sum(taps[k + r] * sq[min(max(i + k, 0), 2)] for k in range(-r, r + 1)) for i in range(3)]
    want_raw = np.array(row) * taps.sum() ** 2
    np.testing.assert_allclose(raw.ravel(), want_raw, rtol=1e-14)
    np.testing.assert_allclose(w.ravel(), 1.0 / (want_raw + 0.5), rtol=1e-14)


def test_block_weight_by_hand():
    """Four voxels in a row, x radius 1: means (1+1+4)/3, (1+4+0)/3, (4+0+0)/3, (0+0+0)/3 with replicated edges."""
    t, m = np.float32([1.0, 3.0, 5.0, 7.0]), np.float32([0.0, 1.0, 5.0, 7.0])     # squared differences 1, 4, 0, 0
    w, mean = R.block_weight(t, m, (4, 1, 1), (1, 0, 0), 10.0, -4)
    np.testing.assert_allclose(mean.ravel(), [2.0, 5.0 / 3.0, 4.0 / 3.0, 0.0], rtol=1e-15)
    np.testing.assert_allclose(w.ravel()[:3], [10.0 / 4.0, 10.0 * 9.0 / 25.0, 10.0 * 9.0 / 16.0], rtol=1e-15)
    assert w.ravel()[3] == np.inf
    w0, _ = R.block_weight(t, m, (4, 1, 1), (1, 0, 0), 10.0, 0)
    assert w0.ravel().tolist() == [10.0, 10.0, 10.0, 10.0]                         # pow(x, 0) = 1, also at x = inf
    w1, _ = R.block_weight(t, m, (4, 1, 1), (0, 0, 0), 1.0, 1)                     # radius 0: 1 / sqrt(sq)
    assert w1.ravel().tolist() == [1.0, 0.5, np.inf, np.inf]
    # a y radius beyond the axis: two rows, every box of radius 3 holds the voxel's own row 3 or 4 times out of 7
    sq = np.float32([[[1.0], [8.0]]])
    np.testing.assert_allclose(R.box_mean(sq, (0, 3, 0)).ravel(), [(4 * 1 + 3 * 8) / 7.0, (3 * 1 + 4 * 8) / 7.0], rtol=1e-15)


def test_accumulate_and_divide_by_hand():
    one = np.float32(1.0)
    ws, two_step, fused = R.accumulate(np.float32([0.25]), np.uint8([1]), np.float32([0.5]), np.float32([1.0]))
    assert ws.tolist() == [0.75] and two_step.tolist() == [1.25] and fused.tolist() == [1.25]
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: the fp32 product is a tie and rounds to 1 + 2^-11; fused, the 2^-24 reaches the sum
    w, lab, acc = np.float32([1.0 + 2.0 ** -12]), np.float32([1.0 + 2.0 ** -12]), np.float32([-1.0])
    _, two_step, fused = R.accumulate(w, lab, None, acc)
    assert two_step.tolist() == [2.0 ** -11] and fused.tolist() == [2.0 ** -11 + 2.0 ** -24]
    # (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46 onto 2^24 + 2 (ulp 2): the exact sum lies just below the midpoint 2^24 + 3 and rounds
    # down; an fp64 sum would land ON the midpoint and go up to the even neighbour, as the rounded product 1 does
    w, lab, acc = np.float32([1.0 + 2.0 ** -23]), np.float32([1.0 - 2.0 ** -23]), np.float32([2.0 ** 24 + 2.0])
    _, two_step, fused = R.accumulate(w, lab, None, acc)
    assert fused.tolist() == [2.0 ** 24 + 2.0] and two_step.tolist() == [2.0 ** 24 + 4.0]
    # uint8 labels are cast to float; wsum None stays None
    ws, a, b = R.accumulate(np.float32([0.5, 0.25]), np.uint8([255, 0]), None, np.float32([1.0, 1.0]))
    assert ws is None and a.tolist() == [128.5, 1.0] and b.tolist() == [128.5, 1.0]
    assert R.divide(np.float32([1.0, 3.0, -2.0]), np.float32([3.0, 0.0, -0.0])).tolist() == [float(one / np.float32(3.0)), 3.0, -2.0]


def test_rescale_and_thresholds_by_hand():
    assert R.rescale_scale_shift(0.0, 4.0) == (0.25, 0.0)
    assert R.rescale_scale_shift(2.0, 2.0) == (0.5, -1.0)                          # a constant image: divided by its value
    assert R.rescale_scale_shift(0.0, 0.0) == (0.0, 0.0)
    x = np.float32([0.0, 1.0, 4.0, 8.0, -1.0, 0.5])
    a, b = R.rescale_threshold(x, 0.0, 4.0, 0.25)
    assert a.tolist() == [0.0, 0.25, 1.0, 1.0, 0.0, 0.0] and b.tolist() == a.tolist()
    a, _ = R.rescale_threshold(x, 0.0, 4.0, -3.0e38)
    assert a.tolist() == [0.0, 0.25, 1.0, 1.0, 0.0, 0.125]
    # a constant image of 2.5: scale fl(0.4) = 0.4 + 2^-52 / 10, shift -fl(2.5 fl(0.4)) = -1.  2.5 fl(0.4) - 1 is 0 when the
    # product is rounded first and 2^-54 when it is not
    a, b = R.rescale_threshold(np.float32([2.5, 5.0]), 2.5, 2.5, -3.0e38)
    assert a.tolist() == [0.0, 1.0] and b[0] == np.float32(2.0 ** -54) and b[1] == 1.0
    assert R.binary_threshold(np.float32([0.0, 1.0, 2.0, 4.0]), 4.0, 0.5).tolist() == [0, 0, 1, 1]
    third = np.float32(1.0) / np.float32(3.0)
    assert R.binary_threshold([third], 1.0, float(third)).tolist() == [1]
    assert R.binary_threshold([third], 1.0, float(third) + 1e-9).tolist() == [0]


def test_minmax_by_hand():
    fmax = float(np.finfo(np.float32).max)
    assert R.minmax(np.float32([3.0, -2.0, 7.0])) == (-2.0, 7.0)
    assert R.minmax(np.float32([np.nan, -2.0, np.nan, -5.0])) == (-5.0, -2.0)
    assert R.minmax(np.float32([np.nan, np.nan])) == (fmax, -fmax)
    assert R.minmax(np.float32([np.inf, 1.0, -np.inf])) == (-np.inf, np.inf)
    assert R.minmax(np.float32([np.inf, np.inf])) == (fmax, np.inf)                # +inf is not < FLT_MAX
    assert R.minmax(np.float32([-0.0, 0.0])) == (0.0, 0.0)


# --------------------------------------------------------------------------------------
# k_map4<op_fuse_divide>, <op_binary_threshold>, <op_fuse_accumulate<.>>, <op_rescale_threshold>, <op_sqdiff>: flat sizes


def divide_inputs(n):
    r = rng_for(n, 1)
    wl = (r.uniform(0.0, 50.0, n) * r.choice([1.0, 1e-20, 1e20], n)).astype(np.float32)
    ws = (r.uniform(0.5, 80.0, n) * r.choice([1.0, 1e-9, 1e9], n)).astype(np.float32)
    ws[r.random(n) < 0.2] = 0.0
    ws[r.random(n) < 0.05] = -0.0
    if n > 4:
        ws[n - 1] = 0.0
        ws[n - 3] = 3.0
    return wl, ws


@pytest.mark.parametrize("case", sizes_and_offsets({"wl": "f", "ws": "f", "out": "f"}), ids=case_id)
def test_fuse_divide(backend, case):
    """wlsum / (wsum, 1 where it is 0), zeros of both signs among the sums and in the last element."""
    n, offs = case
    wl, ws = divide_inputs(n)
    a, b = Placed(backend, wl, offs.get("wl", 0)), Placed(backend, ws, offs.get("ws", 0))
    o = Placed(backend, np.full(n, 123.0, np.float32), offs.get("out", 0))
    backend.ctx.fuse_divide(a.v, b.v, o.v, n)
    got = o.result(backend)
    assert_same_bits(got, R.divide(wl, ws), ("divide", n, offs))
    same_as_aligned((backend.name, "divide", n), offs, [got])
    note(backend, "fuse_divide", mismatches=0, largest_n=n)


def threshold_inputs(n):
    r = rng_for(n, 2)
    p = r.uniform(0.0, 0.9, n).astype(np.float32)
    p[r.random(n) < 0.1] = np.float32(0.45)          # exactly threshold * max: >= keeps it
    p[r.random(n) < 0.1] = np.nextafter(np.float32(0.45), np.float32(0))
    p[0] = 0.9
    if n > 1:
        p[n - 1] = 0.45
    return p


@pytest.mark.parametrize("case", sizes_and_offsets({"prob": "f", "out": "b"}), ids=case_id)
def test_binary_threshold(backend, case):
    n, offs = case
    p = threshold_inputs(n)
    a = Placed(backend, p, offs.get("prob", 0))
    o = Placed(backend, np.full(n, 7, np.uint8), offs.get("out", 0))
    mx = float(np.float32(0.9))
    backend.ctx.binary_threshold(a.v, n, mx, 0.5, o.v)
    got = o.result(backend)
    want = R.binary_threshold(p, mx, 0.5)
    assert 0 < want.sum() < n or n < 8
    assert_same_bits(got, want, ("binary_threshold", n, offs))
    same_as_aligned((backend.name, "threshold", n), offs, [got])
    note(backend, "binary_threshold", mismatches=0, largest_n=n)


LABEL_KINDS = ("u8_binary", "u8_full", "f32")


def accumulate_inputs(n, kind):
    r = rng_for(n, 3 + LABEL_KINDS.index(kind))
    ws = [(r.uniform(0.01, 100.0, n) * r.choice([1.0, 1e-3, 1e3], n)).astype(np.float32) for _ in range(3)]
    if kind == "u8_binary":
        labs = [r.integers(0, 2, n).astype(np.uint8) for _ in range(3)]
    elif kind == "u8_full":
        labs = [r.integers(0, 256, n).astype(np.uint8) for _ in range(3)]
    else:
        labs = [r.uniform(0.0, 1.0, n).astype(np.float32) for _ in range(3)]
    for lab in labs:
        lab[n - 1] = 1
    return ws, labs


def accumulate_reference(ws, labs, with_wsum):
    n = ws[0].size
    wsum = np.zeros(n, np.float32) if with_wsum else None
    plain, fused = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for w, lab in zip(ws, labs):
        s, plain, _ = R.accumulate(w, lab, wsum, plain)
        _, _, fused = R.accumulate(w, lab, None, fused)
        wsum = s
    return wsum, plain, fused


def accumulate_cases():
    roles = {"w": "f", "label": "b", "wsum": "f", "wlsum": "f"}
    out = []
    for kind in LABEL_KINDS:
        roles["label"] = "f" if kind == "f32" else "b"
        for n, o in sizes_and_offsets(roles):
            for with_wsum in (True, False):
                if "wsum" in o and not with_wsum:
                    continue
                if n == N_STRIDE and (kind == "u8_full" or (not with_wsum and o)):
                    continue
                out.append((kind, n, o, with_wsum))
    return out


@pytest.mark.parametrize("case", accumulate_cases(), ids=lambda c: f"{c[0]}-{case_id(c[1:3])}-{'wsum' if c[3] else 'nowsum'}")
def test_fuse_accumulate(backend, case):
    """Three atlases folded into the same sums, as combine_labels does; wsum = NULL is the product's shared-weight-sum path
    for every structure but the first."""
    kind, n, offs, with_wsum = case
    ws, labs = accumulate_inputs(n, kind)
    wsum = Placed(backend, np.zeros(n, np.float32), offs.get("wsum", 0)) if with_wsum else None
    wlsum = Placed(backend, np.zeros(n, np.float32), offs.get("wlsum", 0))
    for w, lab in zip(ws, labs):
        a, b = Placed(backend, w, offs.get("w", 0)), Placed(backend, lab, offs.get("label", 0))
        backend.ctx.fuse_accumulate(a.v, b.v, None if wsum is None else wsum.v, wlsum.v, n)
        assert_same_bits(a.result(backend), w, "weight overwritten")
        assert_same_bits(b.result(backend), lab, "label overwritten")
    want_wsum, plain, fused = accumulate_reference(ws, labs, with_wsum)
    got = wlsum.result(backend)
    if kind == "u8_binary":
        assert_same_bits(plain, fused, "the two candidates must coincide for labels 0 / 1")
    contracted = assert_one_of(got, plain, fused, ("wlsum", kind, n, offs, with_wsum))
    outs = [got]
    if with_wsum:
        outs.append(wsum.result(backend))
        assert_same_bits(outs[1], want_wsum, ("wsum", kind, n, offs))
    same_as_aligned((backend.name, "accumulate", kind, n, with_wsum), offs, outs)
    note(backend, "fuse_accumulate_" + kind, elements_equal_to_the_fused_candidate_only=contracted,
         candidates_differ=int((bits(plain) != bits(fused)).sum()), largest_n=n)


def rescale_inputs(n):
    """Random data in and around [lo, hi] = [-0.3, 1.7], lower 1e-4; values whose rescaled image comes within 2^-20 of `lower`
    are replaced by hi."""
    r = rng_for(n, 7)
    lo, hi, lower = np.float32(-0.3), np.float32(1.7), 1e-4
    x = r.uniform(-0.5, 1.9, n).astype(np.float32)
    x[r.random(n) < 0.1] = lo
    x[r.random(n) < 0.1] = hi
    scale, shift = R.rescale_scale_shift(lo, hi)
    x[np.abs(x.astype(np.float64) * scale + shift - lower) < 2.0 ** -20] = hi
    x[n - 1] = hi
    return x, float(lo), float(hi), lower


@pytest.mark.parametrize("case", sizes_and_offsets({"data": "f"}), ids=case_id)
def test_rescale_threshold(backend, case):
    n, offs = case
    if n == N_STRIDE:       # multiples of 2^-8 in [-1, 8) on [0, 4]: a power-of-two scale, exact either way, values ON `lower` and ON 1
        x = (rng_for(n, 8).integers(-256, 2048, n) / 256.0).astype(np.float32)
        x[n - 1], x[n - 2], x[n - 3] = 4.0, 1.0, 0.5
        lo, hi, lower = 0.0, 4.0, 0.25
    else:
        x, lo, hi, lower = rescale_inputs(n)
    d = Placed(backend, x, offs.get("data", 0))
    backend.ctx.rescale_threshold(d.v, n, lo, hi, lower)
    got = d.result(backend)
    plain, fused = R.rescale_threshold(x, lo, hi, lower)
    contracted = assert_one_of(got, plain, fused, ("rescale", n, offs))
    same_as_aligned((backend.name, "rescale", n), offs, [got])
    note(backend, "rescale_threshold", elements_equal_to_the_fused_candidate_only=contracted,
         candidates_differ=int((bits(plain) != bits(fused)).sum()), largest_n=n)


@pytest.mark.parametrize("off", [0, 4])
def test_rescale_threshold_exact_and_degenerate(backend, off):
    """Values exactly on `lower` and exactly 1 stay; both degenerate branches of RescaleIntensity; the -3.0e38 lower bound the
    host passes for a falsy threshold."""
    one, four = np.float32(1.0), np.float32(4.0)
    exact = np.float32([0.0, np.nextafter(one, np.float32(0)), 1.0, np.nextafter(one, np.float32(2)), 4.0, np.nextafter(four, np.float32(8)),
                        -1.0, 8.0])
    sets = [(exact, 0.0, 4.0, 0.25, np.float32([0.0, 0.0, 0.25, np.nextafter(one, np.float32(2)) * np.float32(0.25), 1.0, 1.0, 0.0, 1.0])),
            (exact, 0.0, 4.0, -3.0e38, None),
            (np.float32([2.5, 0.0, 5.0, 1.25, 2.5, 3.75, 7.0]), 2.5, 2.5, 1e-4, None),        # in_min == in_max != 0: x / 2.5 - 1
            (np.float32([2.5, 0.0, 5.0, 1.25, 2.5, 3.75, 7.0]), 2.5, 2.5, -3.0e38, None),
            (np.float32([0.0, 1.0, -1.0, 3.0e38, 0.5]), 0.0, 0.0, 1e-4, np.zeros(5, np.float32)),   # in_min == in_max == 0: scale 0
            (np.float32([0.0, 1.0, -1.0, 3.0e38, 0.5]), 0.0, 0.0, -3.0e38, np.zeros(5, np.float32)),
            (rescale_inputs(1027)[0], -0.3, 1.7, -3.0e38, None)]
    for x, lo, hi, lower, by_hand in sets:
        d = Placed(backend, x, off)
        backend.ctx.rescale_threshold(d.v, x.size, lo, hi, lower)
        got = d.result(backend)
        plain, fused = R.rescale_threshold(x, lo, hi, lower)
        if by_hand is not None:
            assert_same_bits(plain, by_hand, "restatement")
            assert_same_bits(fused, by_hand, "restatement")
        assert_one_of(got, plain, fused, ("rescale", lo, hi, lower, off))
    want = R.rescale_threshold(np.float32([5.0]), 2.5, 2.5, 1e-4)[0]
    assert want[0] == 1.0                    # the constant-image branch divides by the value: 5 / 2.5 - 1


def ulp_distance(got, want64):
    want32 = np.asarray(want64).astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want32)).astype(np.float64)


@pytest.mark.parametrize("case", sizes_and_offsets({"t": "f", "m": "f", "w": "f"}), ids=case_id)
def test_sqdiff_through_block_weight(backend, case):
    """op_sqdiff on flat sizes: a volume of (n, 1, 1) voxels, box radius 0 (the mean is the voxel itself), gain 2, factor 1:
    the weight is powf(1 / (t - m)^2, 1)."""
    n, offs = case
    r = rng_for(n, 9)
    t, m = (100.0 * r.standard_normal(n)).astype(np.float32), (100.0 * r.standard_normal(n)).astype(np.float32)
    a, b = Placed(backend, t, offs.get("t", 0)), Placed(backend, m, offs.get("m", 0))
    o = Placed(backend, np.full(n, 5.0, np.float32), offs.get("w", 0))
    backend.ctx.weight_map_block(a.v, b.v, (n, 1, 1), (0, 0, 0), 1.0, 2.0, o.v)
    got = o.result(backend)
    want = 1.0 / R.squared_difference(t, m).astype(np.float64)
    dist = ulp_distance(got, want)
    assert dist.max() <= POWF_ULP, ("sqdiff", n, offs, dist.max(), int(dist.argmax()))
    same_as_aligned((backend.name, "sqdiff", n), offs, [got])
    note(backend, "sqdiff_through_block_weight", max_ulp=dist.max(), bound_ulp=POWF_ULP, largest_n=n)


# --------------------------------------------------------------------------------------
# pp_sum_sq_diff_f32


def ssd_bound(n):
    nb = min(-(-n // 256), 2048)
    k = -(-n // (nb * 256))
    return (k + 8 + -(-nb // 256) + 8 + 2) * 2.0 ** -53


@pytest.mark.parametrize("scale", [100.0, 1e18], ids=["normal", "1e18"])
@pytest.mark.parametrize("n", N_EDGE + [N_STRIDE])
def test_sum_sq_diff(backend, n, scale):
    r = rng_for(n, 11)
    a, b = (scale * r.standard_normal(n)).astype(np.float32), (scale * r.standard_normal(n)).astype(np.float32)
    want = R.ssd(a, b)
    da, db = backend.dev(a), backend.dev(b)
    got = backend.ctx.sum_sq_diff(da, db, n)
    rel = abs(got - want) / want
    note(backend, "sum_sq_diff", max_rel_error=rel, error_over_bound=rel / ssd_bound(n), largest_n=n)
    print("ssd", n, scale, "relative error", rel, "bound", ssd_bound(n))
    assert rel <= ssd_bound(n), (n, got, want, rel, ssd_bound(n))
    assert backend.ctx.sum_sq_diff(da, da, n) == 0.0
    if n in N_MATRIX or n == N_STRIDE:       # offset views: the same bits
        for oa, ob in ((4, 0), (0, 4)):
            pa_, pb_ = Placed(backend, a, oa), Placed(backend, b, ob)
            assert backend.ctx.sum_sq_diff(pa_.v, pb_.v, n) == got


# --------------------------------------------------------------------------------------
# pp_minmax_f32


def minmax_equal(got, want):
    assert got[0] == want[0] and got[1] == want[1], (got, want)


@pytest.mark.parametrize("n", [1, 2, 7, 257, 1027, N_STRIDE])
def test_minmax_planted_extrema(backend, n):
    """The minimum and the maximum planted, each in turn, at index 0, n - 1, either side of a block boundary, either side of
    the grid-stride wrap (2048 x 256) and in the last element of the last block (block 2047's fourth trip)."""
    base = rng_for(n, 13).uniform(-1.0, 1.0, n).astype(np.float32)
    pos = sorted({p for p in (0, n - 1, 255, 256, 511, 512, 2048 * 256 - 1, 2048 * 256, 4 * 2048 * 256 - 1, 4 * 2048 * 256) if 0 <= p < n})
    d = backend.dev(base)
    minmax_equal(backend.ctx.minmax(d, n), R.minmax(base))
    for k, p in enumerate(pos):
        q = pos[(k + 1) % len(pos)]
        host = base.copy()
        host[q] = 3.0
        host[p] = -2.0                         # (one position: the minimum wins, the maximum stays a random value)
        d[q] = 3.0
        d[p] = -2.0
        minmax_equal(backend.ctx.minmax(d, n), R.minmax(host))
        d[q], d[p] = float(base[q]), float(base[p])
    pl = Placed(backend, base, 4)
    minmax_equal(backend.ctx.minmax(pl.v, n), R.minmax(base))
    note(backend, "minmax", mismatches=0, largest_n=n)


@pytest.mark.parametrize("n", [5, 1027])
def test_minmax_edge_values(backend, n):
    """NaN among finite values, all NaN, +inf and -inf, zeros of both signs, constant arrays of either sign."""
    r = rng_for(n, 14)
    base = r.uniform(-4.0, -1.0, n).astype(np.float32)          # all negative: a maximum that starts at 0 would show
    fmax = float(np.finfo(np.float32).max)
    arrays = {"negative": base, "positive": -base}
    x = base.copy()
    x[r.random(n) < 0.3] = np.nan
    x[0] = x[n - 1] = np.nan
    x[n // 2] = -2.5
    arrays["nan_sprinkled"] = x
    arrays["all_nan"] = np.full(n, np.nan, np.float32)
    for name, v in (("plus_inf", np.inf), ("minus_inf", -np.inf)):
        x = base.copy()
        x[n - 1] = v
        arrays[name] = x
    x = base.copy()
    x[0], x[n - 1] = np.inf, -np.inf
    arrays["both_inf"] = x
    z = np.zeros(n, np.float32)
    z[::2] = -0.0
    arrays["zeros"] = z
    arrays["constant"] = np.full(n, -7.5, np.float32)
    arrays["constant_fmax"] = np.full(n, -fmax, np.float32)
    for name, x in arrays.items():
        got, want = backend.ctx.minmax(backend.dev(x), n), R.minmax(x)
        assert got[0] == want[0] and got[1] == want[1], (name, got, want)
    assert R.minmax(arrays["all_nan"]) == (fmax, -fmax)


def test_reductions_repeat_bit_identically(backend):
    """Three calls of each reduction on N_STRIDE, with the other reduction and an operation with a larger workspace (the box
    mean's two volumes) between them, so that the partials buffer holds foreign bytes before every call."""
    n = N_STRIDE
    r = rng_for(n, 15)
    a, b = backend.dev((100.0 * r.standard_normal(n)).astype(np.float32)), backend.dev((100.0 * r.standard_normal(n)).astype(np.float32))
    shape = (6, 10, 70)
    t, m = backend.dev(r.standard_normal(shape).astype(np.float32)), backend.dev(r.standard_normal(shape).astype(np.float32))
    w = backend.empty(shape)
    sums, ranges = [], []
    for _ in range(3):
        sums.append(backend.ctx.sum_sq_diff(a, b, n))
        backend.ctx.minmax(b, n)
        backend.ctx.weight_map_block(t, m, (70, 10, 6), (2, 1, 0), 1.0, 2.0, w)
        ranges.append(backend.ctx.minmax(a, n))
        backend.ctx.sum_sq_diff(b, b, n)
        backend.ctx.weight_map_block(t, m, (70, 10, 6), (1, 1, 1), 1.0, 1.0, w)
    assert len({np.float64(s).tobytes() for s in sums}) == 1, sums
    assert len({np.float32(v).tobytes() for v in ranges}) == 1, ranges


# --------------------------------------------------------------------------------------
# pp_weight_map_local_f32, pp_weight_map_block_f32: volumes

VOLUMES = {(5, 6, 7): (0.9, 1.1, 2.5), (9, 14, 23): (0.9, 1.1, 2.5), (1, 1, 9): (1.0, 1.0, 1.0), (3, 1, 1): (1.0, 1.0, 1.0),
           (1, 1, 1): (1.0, 1.0, 1.0), (6, 10, 70): (1.0, 1.0, 1.0)}        # shape (nz, ny, nx) -> spacing (x, y, z)
ZERO_BLOCK_SHAPE = (9, 14, 23)
RADII = [(0, 0, 0), (1, 1, 1), (2, 1, 0), (5, 9, 4)]
_VOL = {}


def size_of(shape):
    return (shape[2], shape[1], shape[0])


def volume_pair(shape):
    """(t, m): 100 N(0, 1) each; in ZERO_BLOCK_SHAPE a block of 7 x 5 x 4 voxels (x, y, z) where t == m, which holds a whole
    box of radius (1, 1, 1) and of (2, 1, 0)."""
    if shape not in _VOL:
        r = np.random.default_rng(77 + int(np.prod(shape)))
        t, m = (100.0 * r.standard_normal(shape)).astype(np.float32), (100.0 * r.standard_normal(shape)).astype(np.float32)
        if shape == ZERO_BLOCK_SHAPE:
            m[2:6, 3:8, 4:11] = t[2:6, 3:8, 4:11]
        t.setflags(write=False)
        m.setflags(write=False)
        _VOL[shape] = (t, m)
    return _VOL[shape]


_LOCAL_REF = {}


def local_reference(lib, shape, sigma):
    key = (shape, sigma)
    if key not in _LOCAL_REF:
        t, m = volume_pair(shape)
        _, raw, radii = R.local_weight(t, m, size_of(shape), VOLUMES[shape], sigma, 0.0, lib=lib)
        raw.setflags(write=False)
        b_fir = U24 * float(R.squared_difference(t, m).max()) * sum(2 * r + 2 for r in radii)
        _LOCAL_REF[key] = (raw, b_fir)
    return _LOCAL_REF[key]


@pytest.mark.parametrize("form", ["fresh", "offset"])
@pytest.mark.parametrize("eps", [1e-5, 1.0])
@pytest.mark.parametrize("sigma", [0.5, 2.0])
@pytest.mark.parametrize("shape", list(VOLUMES), ids=lambda s: "x".join(map(str, s)))
def test_weight_map_local(backend, shape, sigma, eps, form):
    t, m = volume_pair(shape)
    raw, b_fir = local_reference(backend.lib, shape, sigma)
    want = 1.0 / (raw + eps)
    off = 4 if form == "offset" else 0
    a, b, o = Placed(backend, t, off), Placed(backend, m, off), Placed(backend, np.full(shape, 9.0, np.float32), off)
    backend.ctx.weight_map_local(a.v, b.v, size_of(shape), VOLUMES[shape], sigma, eps, o.v)
    got = o.result(backend).astype(np.float64)
    assert_same_bits(a.result(backend), t, "target overwritten")
    assert_same_bits(b.result(backend), m, "moving overwritten")
    bound = b_fir / (raw + eps) ** 2 + 3 * U24 * want
    ratio = float((np.abs(got - want) / bound).max())
    note(backend, "weight_map_local", error_over_bound=ratio, max_rel_error=float((np.abs(got - want) / want).max()))
    print("local", shape, sigma, eps, form, "error / bound", ratio)
    assert np.isfinite(got).all() and ratio <= 1.0, (shape, sigma, eps, form, ratio)


@pytest.mark.parametrize("eps", [1e-5, 1.0])
def test_weight_map_local_identical_images(backend, eps):
    """t == m: the squared difference and its Gaussian are exactly 0, every weight is 1 / eps as fp32 computes it."""
    shape = (5, 6, 7)
    t, _ = volume_pair(shape)
    o = Placed(backend, np.full(shape, 9.0, np.float32), 0)
    backend.ctx.weight_map_local(backend.dev(t), backend.dev(t), size_of(shape), VOLUMES[shape], 2.0, eps, o.v)
    want = np.float32(1.0) / (np.float32(0.0) + np.float32(eps))
    assert_same_bits(o.result(backend), np.full(shape, want, np.float32), "1 / eps")


def test_block_weight_powf_distance(backend):
    """The powf part of the block-weight bound, measured where the box mean is exact: radius 0, squared differences from 1e-4
    to 1e8 (differences of 0.01 .. 1e4), every gain and factor of the tests.  Distance = |got - fp64 restatement| in ulps of
    the fp32 result: 1 / x, powf and the multiply."""
    n = 4099
    r = rng_for(n, 17)
    t = (10.0 ** r.uniform(-2.0, 4.0, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    m = np.zeros(n, np.float32)
    worst = 0.0
    for gain, factor in itertools.product([0, 1, 2, -4], [1.0, 1e4]):
        w = backend.empty((n,))
        backend.ctx.weight_map_block(backend.dev(t), backend.dev(m), (n, 1, 1), (0, 0, 0), factor, gain, w)
        want, mean = R.block_weight(t, m, (n, 1, 1), (0, 0, 0), factor, gain)
        assert np.array_equal(mean.ravel(), R.squared_difference(t, m).astype(np.float64))
        got = np.asarray(backend.host(w))
        if gain == 0:
            assert_same_bits(got, np.full(n, factor, np.float32), "powf(x, 0) must be 1")
        worst = max(worst, float(ulp_distance(got, want.ravel()).max()))
    note(backend, "block_weight_powf", measured_max_ulp=worst, bound_used_ulp=POWF_ULP)
    print("powf distance", worst, "ulp; bound", POWF_ULP)
    assert POWF_ULP <= 8.0 and worst <= POWF_ULP, worst


def power_of_inverse(mean, p, factor):
    """factor * (1 / mean)^p in fp64, as std::pow gives it at mean == 0: +inf for p > 0, factor for p == 0."""
    with np.errstate(divide="ignore"):
        inv = np.where(mean == 0.0, np.inf, 1.0 / np.where(mean == 0.0, 1.0, mean))
    return factor * (np.ones_like(mean) if p == 0.0 else inv ** p)


def ulp32(v):
    v32 = np.asarray(v).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v32), np.spacing(np.abs(v32)), 0.0).astype(np.float64)


@pytest.mark.parametrize("form", ["fresh", "offset"])
@pytest.mark.parametrize("radius", RADII, ids=lambda r: "r%d-%d-%d" % r)
@pytest.mark.parametrize("shape", list(VOLUMES), ids=lambda s: "x".join(map(str, s)))
def test_weight_map_block(backend, shape, radius, form):
    """Box radii 0, inside the volume and beyond every axis of the small ones; gain 0 (the weight is `factor`), 1, 2 and -4; in
    ZERO_BLOCK_SHAPE a box whose mean is exactly 0: +inf for a positive power, `factor` for gain 0."""
    from scipy.ndimage import maximum_filter

    t, m = volume_pair(shape)
    sq = R.squared_difference(t, m).astype(np.float64)
    box_max = maximum_filter(sq, size=tuple(2 * radius[2 - k] + 1 for k in range(3)), mode="nearest")
    b_box = U24 * box_max * sum(2 * r + 3 for r in radius)
    off = 4 if form == "offset" else 0
    a, b = Placed(backend, t, off), Placed(backend, m, off)
    for gain, factor in itertools.product([0, 1, 2, -4], [1.0, 1e4]):
        o = Placed(backend, np.full(shape, 9.0, np.float32), off)
        backend.ctx.weight_map_block(a.v, b.v, size_of(shape), radius, factor, gain, o.v)
        got = o.result(backend).astype(np.float64)
        want, mean = R.block_weight(t, m, size_of(shape), radius, factor, gain)
        zero = mean == 0.0
        if shape == ZERO_BLOCK_SHAPE and radius != (5, 9, 4):
            assert zero.any() and (box_max[zero] == 0.0).all()
            assert (want[zero] == (factor if gain == 0 else np.inf)).all()
        assert np.array_equal(got[zero], want[zero]), (shape, radius, gain, factor, got[zero][:4], want[zero][:4])
        p = abs(gain / 2.0)
        low = power_of_inverse(mean + b_box, p, factor)
        high = power_of_inverse(np.maximum(mean - b_box, 0.0), p, factor)
        ok = (got >= low - POWF_ULP * ulp32(low)) & (got <= high + POWF_ULP * ulp32(high))
        dist = float(ulp_distance(got[~zero].astype(np.float32), want[~zero]).max()) if (~zero).any() else 0.0
        note(backend, "weight_map_block", max_ulp_from_restatement=dist,
             largest_relative_box_bound=float((b_box[~zero] / mean[~zero]).max(initial=0.0)))
        assert ok.all() and not np.isnan(got).any(), (shape, radius, gain, factor, form, np.argwhere(~ok)[:4], got[~ok][:4], want[~ok][:4])
    assert_same_bits(a.result(backend), t, "target overwritten")
    assert_same_bits(b.result(backend), m, "moving overwritten")


# --------------------------------------------------------------------------------------
# argument errors


def test_argument_errors_leave_outputs_untouched(backend):
    """NULL pointers, n == 0 for the range, an empty volume, a box radius of -1 and of 128 (PP_MAX_RADIUS is 127): an error
    through _chk, and not one byte of an output written.  (pp_weight_map_block_f32 used to launch the squared difference into
    `weight` BEFORE it looked at the radii, so a refused radius left the output overwritten; the check now comes first.)"""
    ctx, n, shape = backend.ctx, 12, (2, 2, 3)
    f = Placed(backend, np.arange(n, dtype=np.float32) + 1, 0)
    g = Placed(backend, np.arange(n, dtype=np.float32) + 2, 0)
    lab = Placed(backend, np.ones(n, np.uint8), 0)
    out = Placed(backend, np.full(n, 9.0, np.float32), 0)
    out2 = Placed(backend, np.full(n, 8.0, np.float32), 0)
    out8 = Placed(backend, np.full(n, 7, np.uint8), 0)
    size, sp = size_of(shape), (1.0, 1.0, 1.0)
    calls = [lambda: ctx.weight_map_local(None, g.v, size, sp, 2.0, 1e-5, out.v),
             lambda: ctx.weight_map_local(f.v, None, size, sp, 2.0, 1e-5, out.v),
             lambda: ctx.weight_map_local(f.v, g.v, size, sp, 2.0, 1e-5, None),
             lambda: ctx.weight_map_local(f.v, g.v, (0, 2, 3), sp, 2.0, 1e-5, out.v),
             lambda: ctx.weight_map_block(None, g.v, size, (1, 1, 1), 1.0, 2.0, out.v),
             lambda: ctx.weight_map_block(f.v, None, size, (1, 1, 1), 1.0, 2.0, out.v),
             lambda: ctx.weight_map_block(f.v, g.v, size, (1, 1, 1), 1.0, 2.0, None),
             lambda: ctx.weight_map_block(f.v, g.v, (3, 0, 2), (1, 1, 1), 1.0, 2.0, out.v),
             lambda: ctx.weight_map_block(f.v, g.v, size, (1, -1, 1), 1.0, 2.0, out.v),
             lambda: ctx.weight_map_block(f.v, g.v, size, (1, 1, 128), 1.0, 2.0, out.v),
             lambda: ctx.sum_sq_diff(None, g.v, n), lambda: ctx.sum_sq_diff(f.v, None, n),
             lambda: ctx.fuse_accumulate(None, lab.v, out.v, out2.v, n), lambda: ctx.fuse_accumulate(f.v, None, out.v, out2.v, n),
             lambda: ctx.fuse_accumulate(f.v, lab.v, out.v, None, n),
             lambda: ctx.fuse_divide(None, g.v, out.v, n), lambda: ctx.fuse_divide(f.v, None, out.v, n), lambda: ctx.fuse_divide(f.v, g.v, None, n),
             lambda: ctx.minmax(None, n), lambda: ctx.minmax(f.v, 0),
             lambda: ctx.rescale_threshold(None, n, 0.0, 1.0, 1e-4),
             lambda: ctx.binary_threshold(None, n, 1.0, 0.5, out8.v), lambda: ctx.binary_threshold(f.v, n, 1.0, 0.5, None)]
    for k, call in enumerate(calls):
        with pytest.raises(_lib.PlatipyAmdError):
            call()
        assert (out.result(backend) == 9.0).all() and (out2.result(backend) == 8.0).all() and (out8.result(backend) == 7).all(), k
