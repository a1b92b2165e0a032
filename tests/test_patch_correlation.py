"""The patch-correlation weight map (compute_patch_correlation_weight_map, and weight_map_for_vote as the pipelines call it),
histogram_mutual_information and Image arithmetic against the numpy / scipy
restatement of the reference's arithmetic (tests/patch_correlation_restatement.py).

Tolerances
  kernel vs restatement, identical fp32 inputs: atol 2^-23, rtol 0 -- one fp32 ulp at |r| = 1.  The kernel rounds to fp32
      once; its fp64 moments over at most 4096 terms contribute ~1e-12.  Where scipy gives NaN (the reference's 0) the
      kernel's value is exactly 0.0.
  compute_weight_map end to end and through combine_labels: atol 3e-6, what the linear-resample and fusion parity tests
      hold fp32 kernels to against the fp64 oracle (tests/test_kernels.py, tests/test_fusion.py).
  joint histogram: counts EQUAL np.histogram2d's; mutual information rtol 1e-12 (fp64 on the same integers)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import patch_correlation_restatement as R
from tests.helpers import phantom

ULP = 2.0 ** -23
SHAPE = (14, 23, 29)                                   # [Z][Y][X]
WINDOWS = [(8, 8, 8), (3, 5, 4), (1, 1, 7), (16, 5, 3)]   # (x, y, z) voxels


@functools.lru_cache(maxsize=None)
def kernel_pair():
    """Noisy CT-like target, the moving image one voxel off with its own noise; a slab that is exactly constant in both
    images and a slab that is constant in the moving image only."""
    base = phantom(SHAPE, seed=31, noise=0).astype(np.float64)
    t = (base + np.random.default_rng(32).normal(0, 5.0, SHAPE)).astype(np.float32)
    m = (np.roll(base, 1, axis=2) + np.random.default_rng(33).normal(0, 5.0, SHAPE)).astype(np.float32)
    t[:, 0:9, 0:10] = -1000.0
    m[:, 0:9, 0:10] = -1000.0
    m[:, 14:23, 18:29] = 37.5
    return t, m


def run_kernel(backend, t, m, window):
    out = backend.empty(t.shape)
    backend.ctx.patch_correlation(backend.dev(t), backend.dev(m), t.shape[::-1], window, out)
    return np.array(backend.host(out))


@pytest.mark.parametrize("window", WINDOWS + [(17, 3, 3)], ids=lambda w: "x".join(map(str, w)))
def test_kernel_against_restatement(backend, window):
    """Windows of up to 8 and up to 16 voxels (the two LDS tiles) and one beyond (patches read from global memory)."""
    t, m = kernel_pair()
    want = R.patch_correlation(t, m, window[::-1])
    got = run_kernel(backend, t, m, window)
    assert got.dtype == np.float32 and got.shape == SHAPE
    zero = want == 0
    err = np.abs(got.astype(np.float64) - want)
    print(window, "max |err|", err.max(), "constant patches", int(zero.sum()), "of", want.size, "range", want.min(), want.max())
    assert zero.sum() > 0, "the constant-patch branch is not exercised"
    assert np.all(got[zero] == 0.0)
    assert np.all(np.abs(got) <= 1.0)
    np.testing.assert_allclose(got, want, rtol=0, atol=ULP)
    assert np.array_equal(got, run_kernel(backend, t, m, window)), "a rerun differs"


@pytest.mark.parametrize("window", [(2, 2, 2), (1, 2, 2), (1, 1, 1)], ids=lambda w: "x".join(map(str, w)))
def test_rejected_windows(backend, window):
    """Some patch would hold a single voxel, where scipy.stats.pearsonr raises."""
    t, m = kernel_pair()
    with pytest.raises(ValueError):
        run_kernel(backend, t, m, window)
    with pytest.raises(ValueError):
        R.patch_correlation(t[:4, :4, :4], m[:4, :4, :4], window[::-1])


# --------------------------------------------------------------------------------------
# compute_weight_map

E_SHAPE, E_SPACING, E_ORIGIN = (20, 44, 52), (0.9, 1.1, 2.5), (12.0, -30.0, 7.5)


@functools.lru_cache(maxsize=None)
def e2e_pair(seed=41):
    base = phantom(E_SHAPE, seed=40, noise=0).astype(np.float64)
    t = (base + np.random.default_rng(seed).normal(0, 5.0, E_SHAPE)).astype(np.float32)
    m = (np.roll(base, (1, -1), axis=(1, 2)) + np.random.default_rng(seed + 1).normal(0, 5.0, E_SHAPE)).astype(np.float32)
    return t, m


def expected_weight_map(pa, t, m, params):
    """The restatement fed the package's own smooth_and_resample outputs of the images cast to fp32."""
    p = {"patch_window_mm": 25, "resampled_voxel_size_mm": 3, "correlation_function": lambda x: x + 1}
    p.update(params)
    res = [pa.registration.smooth_and_resample(pa.image_from_array(a.astype(np.float32), E_SPACING, E_ORIGIN),
                                               isotropic_voxel_size_mm=p["resampled_voxel_size_mm"]) for a in (t, m)]
    assert res[0].tensor.dtype == torch.float32 and res[0].same_grid(res[1])
    return R.weight_map(res[0].numpy(), res[1].numpy(), res[0].GetSpacing(), res[0].GetOrigin(), E_SHAPE, E_SPACING, E_ORIGIN,
                        p["patch_window_mm"], p["correlation_function"])


@pytest.mark.parametrize("case", ["default", "window12_voxel4_abs", "int16"])
def test_compute_weight_map_patch_correlation(host_api, case):
    pa = host_api
    t, m = e2e_pair()
    params = {}
    if case == "window12_voxel4_abs":
        params = {"patch_window_mm": 12, "resampled_voxel_size_mm": 4, "correlation_function": abs}
    if case == "int16":
        t, m = np.round(t).astype(np.int16), np.round(m).astype(np.int16)
    target, moving = pa.image_from_array(t, E_SPACING, E_ORIGIN), pa.image_from_array(m, E_SPACING, E_ORIGIN)
    got = pa.label.fusion.weight_map_for_vote(target, moving, vote_type="patch_correlation", vote_params=params or None)
    assert got.tensor.dtype == torch.float32
    assert got.GetSize() == target.GetSize() and got.GetSpacing() == target.GetSpacing() and got.GetOrigin() == target.GetOrigin()
    assert got.GetDirection() == target.GetDirection()
    want = expected_weight_map(pa, t, m, params)
    err = np.abs(got.numpy().astype(np.float64) - want)
    print(case, "max |err|", err.max(), "range", want.min(), want.max())
    assert want.max() - want.min() > 0.2
    np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=3e-6)
    again = pa.label.fusion.weight_map_for_vote(target, moving, vote_type="PATCH_CORRELATION", vote_params=params or None)
    assert np.array_equal(got.numpy(), again.numpy()), "a rerun differs"


def test_compute_weight_map_patch_correlation_arguments(host_api):
    pa = host_api
    t, m = e2e_pair()
    target, moving = pa.image_from_array(t, E_SPACING, E_ORIGIN), pa.image_from_array(m, E_SPACING, E_ORIGIN)
    # a callable that returns a tensor is accepted as well
    a = pa.label.compute_patch_correlation_weight_map(target, moving, {"correlation_function": lambda x: x.tensor + 1})
    b = pa.label.compute_patch_correlation_weight_map(target, moving)
    assert np.array_equal(a.numpy(), b.numpy())
    # the resampled grids differ
    other = pa.image_from_array(m[:, :, :40].copy(), E_SPACING, E_ORIGIN)
    with pytest.raises(ValueError):
        pa.label.compute_patch_correlation_weight_map(target, other)
    # int(6 / 3.x) = 1 voxel per axis: every patch is a single voxel
    with pytest.raises(ValueError):
        pa.label.compute_patch_correlation_weight_map(target, moving, {"patch_window_mm": 6})
    # every other vote type goes through the dispatcher unchanged
    for vote in ("unweighted", "block"):
        assert np.array_equal(pa.label.fusion.weight_map_for_vote(target, moving, vote).numpy(),
                              pa.label.compute_weight_map(target, moving, vote).numpy())
    d = pa.label.fusion.DEFAULT_VOTE_PARAMS
    assert d["patch_window_mm"] == 25 and d["resampled_voxel_size_mm"] == 3
    assert np.array_equal(d["correlation_function"](pa.image_from_array(t)).numpy(), t + 1)


def test_combine_labels_with_patch_correlation_weights(host_api):
    pa = host_api
    t, _ = e2e_pair()
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in E_SHAPE], indexing="ij")
    aset_g, aset_o = {}, {}
    for k, seed in enumerate((41, 51)):
        m = e2e_pair(seed)[1]
        lab = ((((xx - 26 - 2 * k) / 11.0) ** 2 + ((yy - 22 + k) / 9.0) ** 2 + ((zz - 10) / 5.0) ** 2) <= 1).astype(np.uint8)
        w = pa.label.fusion.weight_map_for_vote(pa.image_from_array(t, E_SPACING, E_ORIGIN), pa.image_from_array(m, E_SPACING, E_ORIGIN),
                                                vote_type="patch_correlation")
        aset_g[f"{k}"] = {"DIR": {"Weight Map": w, "HEART": pa.image_from_array(lab, E_SPACING, E_ORIGIN)}}
        aset_o[f"{k}"] = {"DIR": {"Weight Map": O.Vol(expected_weight_map(pa, t, m, {}), E_SPACING, E_ORIGIN),
                                  "HEART": O.Vol(lab, E_SPACING, E_ORIGIN)}}
    got = pa.label.combine_labels(aset_g, "HEART")["HEART"].numpy()
    want = O.combine_labels(aset_o, "HEART")["HEART"].arr
    print("max |err|", np.abs(got.astype(np.float64) - want).max())
    assert got.max() == 1.0 and 0.01 < (got > 0.5).mean() < 0.5
    np.testing.assert_allclose(got, want, rtol=0, atol=3e-6)


# --------------------------------------------------------------------------------------
# Image arithmetic


def test_image_operators(host_api):
    pa = host_api
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=(4, 5, 6)).astype(np.float32), rng.uniform(1, 2, size=(4, 5, 6)).astype(np.float32)
    sp, org = (0.5, 0.75, 2.0), (1.0, -2.0, 3.0)
    ia, ib = pa.image_from_array(a, sp, org), pa.image_from_array(b, sp, org)
    cases = {
        "add": (ia + ib, a + b), "add_s": (ia + 1, a + 1), "radd": (1.5 + ia, 1.5 + a),
        "sub": (ia - ib, a - b), "sub_s": (ia - 2, a - 2), "rsub": (2 - ia, 2 - a),
        "mul": (ia * ib, a * b), "mul_s": (ia * 3.0, a * 3.0), "rmul": (3.0 * ia, 3.0 * a),
        "div": (ia / ib, a / b), "div_s": (ia / 4, a / 4), "rdiv": (1 / ib, 1 / b),
        "pow": (ib ** 2, b ** 2), "pow_i": (ib ** ia, b ** a), "rpow": (2.0 ** ia, np.float32(2.0) ** a),
        "neg": (-ia, -a), "abs": (abs(ia), np.abs(a)),
    }
    for name, (got, want) in cases.items():
        assert isinstance(got, pa.Image), name
        assert got.same_grid(ia) and got.tensor.dtype == torch.float32, name
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=0, err_msg=name)
    assert np.array_equal(ia.numpy(), a), "an operator changed its operand"
    assert (pa.image_from_array(np.ones((2, 2, 2), np.int16)) + 1).tensor.dtype == torch.int16
    for other in (pa.image_from_array(b, (0.5, 0.75, 2.5), org), pa.image_from_array(b, sp, (0.0, 0.0, 0.0)),
                  pa.image_from_array(b[:, :, :5].copy(), sp, org)):
        with pytest.raises(ValueError):
            ia + other
        with pytest.raises(ValueError):
            ia / other
    with pytest.raises(TypeError):
        ia + "1"


# --------------------------------------------------------------------------------------
# mutual information


@functools.lru_cache(maxsize=None)
def mi_pairs():
    rng = np.random.default_rng(77)
    n = 9973                                            # not a multiple of the 256-thread block
    x = rng.normal(size=n)
    noise = (x.astype(np.float32) * 40 - 1000, (0.6 * x + 0.8 * rng.normal(size=n)).astype(np.float32) * 25 + 30)
    # integers 0..128: with 64 bins every even value sits exactly on an edge, with 20 bins every multiple of 32
    ia = rng.integers(0, 129, size=(7, 31, 41))
    ib = np.clip(ia + rng.integers(-20, 21, size=ia.shape), 0, 128)
    ia.flat[:2], ib.flat[:2] = (0, 128), (128, 0)
    const = (np.full(n, 3.25, np.float32), noise[1])
    return {"noise": noise, "integers": (ia.astype(np.float32), ib.astype(np.float32)), "constant": const}


@pytest.mark.parametrize("bins", [64, 20, (16, 40)], ids=str)
@pytest.mark.parametrize("name", ["noise", "integers", "constant"])
def test_joint_histogram_equals_numpy(host_api, name, bins):
    pa = host_api
    a, b = mi_pairs()[name]
    want, ea, eb = R.joint_histogram(a, b, bins)
    got, ga, gb = pa.label.fusion.joint_histogram(a, b, bins)
    assert got.dtype == np.int64 and got.shape == want.shape and got.sum() == a.size
    assert np.array_equal(ga, ea) and np.array_equal(gb, eb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_joint_histogram_kernel_beyond_the_lds_table(backend):
    """130 x 130 bins do not fit the 128 x 128 LDS table: global integer atomics, the same counts."""
    a, b = mi_pairs()["noise"]
    got, rng = backend.ctx.joint_histogram(backend.dev(a), backend.dev(b), a.size, 130, 130)
    want, ea, eb = R.joint_histogram(a, b, 130)
    assert np.array_equal(got, want)
    assert rng == (ea[0], ea[-1], eb[0], eb[-1])


@pytest.mark.parametrize("bins", [64, 20], ids=str)
@pytest.mark.parametrize("name", ["noise", "integers", "constant"])
def test_mutual_information(host_api, name, bins):
    pa = host_api
    a, b = mi_pairs()[name]
    want = R.mutual_information(a, b, bins)
    got = pa.label.fusion.histogram_mutual_information(a, b, bins)
    print(name, bins, got, want)
    assert isinstance(got, float) and np.isfinite(got)
    if name != "constant":
        assert want != 0.0          # (a density, not a probability, goes into the logarithm: the scale depends on the units)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    if bins == 64:
        assert pa.label.fusion.histogram_mutual_information(a, b) == got                  # the default
        img = [pa.image_from_array(v.reshape(-1, 1, 1)) for v in (a, b)]         # Images and tensors are flattened alike
        assert pa.label.fusion.histogram_mutual_information(img[0], img[1]) == got
        assert pa.label.fusion.histogram_mutual_information(img[0].tensor, torch.from_numpy(np.ascontiguousarray(b))) == got


def test_mutual_information_arguments(host_api):
    pa = host_api
    a, b = mi_pairs()["noise"]
    with pytest.raises(NotImplementedError):
        pa.label.fusion.histogram_mutual_information(a, b, bins=np.linspace(-1200, 200, 33))
    with pytest.raises(NotImplementedError):
        pa.label.fusion.histogram_mutual_information(a, b, bins=[np.linspace(-1200, 200, 33), 16])
    for bad in (np.nan, np.inf):
        c = a.copy()
        c[17] = bad
        with pytest.raises(ValueError):
            pa.label.fusion.histogram_mutual_information(c, b)
        with pytest.raises(ValueError):
            pa.label.fusion.histogram_mutual_information(b, c, bins=20)
        with pytest.raises(ValueError):
            R.mutual_information(c, b)
    # bins_a != bins_b: the reference's outer(p_a, p_b) has the transposed shape and its division cannot broadcast
    with pytest.raises(ValueError):
        R.mutual_information(a, b, (16, 40))
    with pytest.raises(ValueError):
        pa.label.fusion.histogram_mutual_information(a, b, (16, 40))
