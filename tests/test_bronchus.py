"""Airway and lung segmentation: the four region kernels (csrc/pp_region.h) against numpy / scipy on the CPU stand-in and
on the GPU, and the lung / bronchus pipeline against the restatement of the reference's logic
(tests/bronchus_restatement.py) on a thorax phantom."""
import functools

import numpy as np
import pytest

from platipy_amd import _lib
from tests import bronchus_restatement as R
from tests.helpers import bernoulli, checkerboard, rot_xyz

SHAPES = [(24, 32, 40), (5, 9, 37), (1, 7, 19), (6, 5, 1), (3, 4, 1040)]      # base, odd widths, one slice, one column, row carry


def size_of(shape):
    return (shape[2], shape[1], shape[0])


def run_labels(be, mask):
    lab = be.dev(np.zeros(mask.shape, np.int32))
    count = be.ctx.connected_components(be.dev(mask), size_of(mask.shape), lab)
    return be.host(lab), count


def run_moments(be, labels_dev, shape, nlabels):
    out = be.dev(np.full((nlabels, 10), -1, np.int64))
    be.ctx.label_moments(labels_dev, size_of(shape), nlabels, out)
    return be.host(out)


def u_shape():
    """Two arms that start at z = 0 and join only in the last slice: the second arm's first voxel gets the first arm's
    label only through the highest z."""
    m = np.zeros((6, 7, 9), np.uint8)
    m[:, 1, 1] = 1
    m[:, 5, 7] = 1
    m[5, 1:6, 1] = 1
    m[5, 5, 1:8] = 1
    return m


# ---- labels ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", [0.3, 0.6])
@pytest.mark.parametrize("shape", SHAPES)
def test_labels_equal_scipy(backend, shape, density):
    mask = bernoulli(shape, density, seed=11 + shape[2])
    want, n = R.label(mask)
    got, count = run_labels(backend, mask)
    assert count == n
    assert np.array_equal(got, want)


def test_labels_checkerboard_scan_crosses_blocks(backend):
    mask = checkerboard((9, 33, 300))
    want, n = R.label(mask)
    assert n > 40000
    got, count = run_labels(backend, mask)
    assert count == n and np.array_equal(got, want)


def test_labels_u_empty_full_and_rerun(backend):
    m = u_shape()
    got, count = run_labels(backend, m)
    want, n = R.label(m)
    assert n == 1 and count == 1 and np.array_equal(got, want)
    empty, c0 = run_labels(backend, np.zeros((5, 9, 37), np.uint8))
    assert c0 == 0 and not empty.any()
    full, c1 = run_labels(backend, np.full((5, 9, 37), 255, np.uint8))
    assert c1 == 1 and np.all(full == 1)
    mask = bernoulli((24, 32, 40), 0.45, seed=5)
    a, ca = run_labels(backend, mask)
    b, cb = run_labels(backend, mask)
    assert ca == cb and np.array_equal(a, b)


# ---- moments ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_moments_equal_integer_sums(backend, shape):
    lab, n = R.label(bernoulli(shape, 0.45, seed=3 + shape[2]))
    dev = backend.dev(lab)
    assert np.array_equal(run_moments(backend, dev, shape, n), R.moments(lab, n))
    # more labels asked for than present: zero rows; fewer: the labels above are ignored
    assert np.array_equal(run_moments(backend, dev, shape, n + 7), R.moments(lab, n + 7))
    few = max(n // 2, 1)
    assert np.array_equal(run_moments(backend, dev, shape, few), R.moments(lab, few))
    again = run_moments(backend, dev, shape, n)
    assert np.array_equal(again, R.moments(lab, n))


def test_moments_offset_pointer_and_negative_labels(backend):
    shape = (5, 9, 37)
    lab, n = R.label(bernoulli(shape, 0.4, seed=8))
    lab[0, 0, :5] = -3                                            # not a label
    buf = backend.dev(np.concatenate([np.zeros(1, np.int32), lab.ravel()]))
    assert np.array_equal(run_moments(backend, buf[1:], shape, n), R.moments(lab, n))


def test_moments_one_dominant_label(backend):
    shape = (24, 32, 40)
    lab = np.ones(shape, np.int32)
    lab[3, 4, 5:9] = 2
    lab[20:22, 30, 38:] = 3
    lab[23, 31, 39] = 0
    assert (lab == 1).mean() > 0.99
    assert np.array_equal(run_moments(backend, backend.dev(lab), shape, 3), R.moments(lab, 3))


# ---- region growing --------------------------------------------------------------------------------------------

def run_grow(be, img, lower, upper, seeds):
    out = be.dev(np.full(img.shape, 7, np.uint8))
    vox = be.ctx.connected_threshold(be.dev(img), size_of(img.shape), lower, upper, seeds, out)
    return be.host(out), vox


def first_voxel_with(img, value, skip=0):
    z, y, x = [a[skip] for a in np.nonzero(img == value)]
    return [int(x), int(y), int(z)]


@pytest.mark.parametrize("shape", SHAPES)
def test_region_growing_equals_scipy(backend, shape):
    img = np.random.default_rng(21 + shape[2]).integers(0, 5, size=shape).astype(np.float32)
    lower, upper = 1.0, 3.0
    lab, _ = R.label((img >= lower) & (img <= upper))
    on_lower, on_upper, outside = first_voxel_with(img, 1.0), first_voxel_with(img, 3.0), first_voxel_with(img, 4.0)
    # a seed exactly on `lower`, one exactly on `upper`, both ends included
    for seeds in ([on_lower], [on_upper], [on_lower, on_upper]):
        got, vox = run_grow(backend, img, lower, upper, seeds)
        want = R.connected_threshold(img, seeds, lower, upper)
        assert want[seeds[0][2], seeds[0][1], seeds[0][0]] == 1
        assert np.array_equal(got, want) and vox == int(want.sum())
    # a seed outside the interval contributes nothing
    got, vox = run_grow(backend, img, lower, upper, [outside])
    assert vox == 0 and not got.any()
    got, vox = run_grow(backend, img, lower, upper, [outside, on_upper])
    assert np.array_equal(got, R.connected_threshold(img, [on_upper], lower, upper))
    # two seeds in one component
    zs, ys, xs = np.nonzero(lab == lab[on_lower[2], on_lower[1], on_lower[0]])
    pair = [on_lower, [int(xs[-1]), int(ys[-1]), int(zs[-1])]]
    got, vox = run_grow(backend, img, lower, upper, pair)
    assert np.array_equal(got, R.connected_threshold(img, [on_lower], lower, upper))


def test_region_growing_two_components_and_nan_plane(backend):
    img = np.full((5, 9, 37), 2.0, np.float32)
    img[:, 4, :] = np.nan                                       # a NaN plane separates y < 4 from y > 4
    a, b = [3, 1, 2], [30, 7, 4]
    got, vox = run_grow(backend, img, 0.0, 5.0, [a])
    want = np.zeros(img.shape, np.uint8)
    want[:, :4, :] = 1
    assert np.array_equal(got, want) and vox == int(want.sum())
    got, vox = run_grow(backend, img, 0.0, 5.0, [a, b])
    want[:, 5:, :] = 1
    assert np.array_equal(got, want) and vox == int(want.sum())
    got, vox = run_grow(backend, img, 0.0, 5.0, [[5, 4, 2]])   # a seed on a NaN
    assert vox == 0 and not got.any()
    got, vox = run_grow(backend, img, float("nan"), 5.0, [a])  # a NaN bound: nothing joins
    assert vox == 0 and not got.any()


@pytest.mark.parametrize("seed", [[37, 0, 0], [0, 9, 0], [0, 0, 5], [-1, 0, 0]])
def test_region_growing_seed_outside_the_buffer(backend, seed):
    img = np.zeros((5, 9, 37), np.float32)
    with pytest.raises(IndexError) as e:
        run_grow(backend, img, -1.0, 1.0, [[1, 1, 1], seed])
    assert e.value.code == _lib.ERR_INVALID


# ---- median ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [(1, 1, 1), (2, 1, 0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_median_equals_scipy(backend, shape, radius):
    masks = [bernoulli(shape, 0.5, seed=31 + shape[2])]
    frame = bernoulli(shape, 0.5, seed=32 + shape[2])          # foreground on every face, edge and corner
    frame[[0, -1], :, :] = 1
    frame[:, [0, -1], :] = 1
    frame[:, :, [0, -1]] = 1
    masks.append(frame)
    masks.append(1 - frame)
    for m in masks:
        out = backend.dev(np.full(shape, 9, np.uint8))
        backend.ctx.binary_median(backend.dev(m * 200), size_of(shape), radius, out)
        assert np.array_equal(backend.host(out), R.median(m, radius))


# ---- shape statistics ------------------------------------------------------------------------------------------

def stat_fixture():
    lab = np.zeros((24, 32, 40), np.int32)
    lab[2:11, 3:8, 4:7] = 1                                     # box 3 x 5 x 9 (x, y, z)
    lab[13:24, 20:22, 30:32] = 2                                # box 2 x 2 x 11
    zz, yy, xx = np.indices(lab.shape)
    lab[(zz - 12) ** 2 + (yy - 16) ** 2 + (xx - 20) ** 2 <= 36] = 3
    return lab


@pytest.mark.parametrize("direction", ["identity", "oblique"])
def test_label_shape_statistics(host_api, direction):
    pa = host_api
    lab = stat_fixture()
    spacing, origin = (1.0, 1.2, 2.5), (-20.0, 13.5, 100.25)
    d = tuple((np.eye(3) if direction == "identity" else rot_xyz(20.0, -35.0, 50.0)).ravel())
    want = R.shape_statistics(lab, 4, spacing, origin, d)
    for k in (1, 2, 3):       # the bound below rests on this separation: an eigenvalue moves by ~1e-16 |M|
        lam = want[k]["principal_moments"]
        assert lam[0] >= 1e-3 * lam[2]
    got = pa.label.label_shape_statistics(pa.image_from_array(lab, spacing, origin, d), 4)
    assert sorted(got) == [1, 2, 3, 4]
    assert got[4]["count"] == 0 and got[4]["centroid"] is None and got[4]["physical_size"] == 0.0
    for k in (1, 2, 3):
        assert got[k]["roundness"] is None and got[k]["perimeter"] is None
        assert got[k]["count"] == want[k]["count"] == int((lab == k).sum())
        assert got[k]["physical_size"] == want[k]["physical_size"]
        scale = np.abs(want[k]["centroid"]).max()
        assert np.abs(np.subtract(got[k]["centroid"], want[k]["centroid"])).max() <= 1e-12 * scale
        for key in ("elongation", "flatness"):
            assert abs(got[k][key] - want[k][key]) <= 1e-10 * want[k][key], (k, key, got[k][key], want[k][key])
    # the default label count is the largest label present
    assert sorted(pa.label.label_shape_statistics(pa.image_from_array(lab, spacing, origin, d))) == [1, 2, 3]
    # known answers: a box of a x b x c voxels has second moments (a^2, b^2, c^2) spacing^2 / 12
    lam = np.sort(np.array([3 * 1.0, 5 * 1.2, 9 * 2.5]) ** 2 / 12.0)
    assert np.allclose(got[1]["principal_moments"], lam, rtol=1e-12)
    assert abs(got[1]["elongation"] - (9 * 2.5) / (5 * 1.2)) < 1e-12 and abs(got[1]["flatness"] - (5 * 1.2) / 3.0) < 1e-12


def test_python_wrappers(host_api):
    pa = host_api
    mask = bernoulli((5, 9, 37), 0.5, seed=77)
    img = pa.image_from_array(mask, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0))
    lab, count = pa.label.connected_component(img)
    want, n = R.label(mask)
    assert count == n and str(lab.tensor.dtype) == "torch.int32" and np.array_equal(lab.numpy(), want)
    assert lab.GetSpacing() == img.GetSpacing() and lab.GetOrigin() == img.GetOrigin()
    assert np.array_equal(pa.label.binary_median(img, 1).numpy(), R.median(mask))
    ct = np.random.default_rng(4).integers(-3, 3, size=mask.shape).astype(np.int16)
    seed = [int(v) for v in np.argwhere(ct == 0)[0][::-1]]
    got = pa.registration.connected_threshold(pa.image_from_array(ct), [seed], -1, 1)
    assert str(got.tensor.dtype) == "torch.uint8" and np.array_equal(got.numpy(), R.connected_threshold(ct, [seed], -1, 1))
    with pytest.raises(IndexError):
        pa.registration.connected_threshold(pa.image_from_array(ct), [[0, 0, 99]], -1, 1)


# ---- pipeline --------------------------------------------------------------------------------------------------

SPACING = (3.0, 3.0, 3.0)


@functools.lru_cache(maxsize=None)
def restated(air_column=0, fast_mode=True, size_range=(22000, 150000), hu_values=None, distances=None):
    img = R.thorax_phantom(air_column=air_column)
    cfg = dict(R.DEFAULT_SETTINGS, fast_mode=fast_mode, expected_physical_size_range=list(size_range))
    if hu_values:
        cfg.update(lung_mask_hu_values=list(hu_values), distance_from_supu_slice_values=list(distances))
    lung, airway, info = R.run_bronchus_segmentation(img, SPACING, config=cfg)
    for a in (img, lung, airway):
        if a is not None:
            a.setflags(write=False)
    return img, lung, airway, info


def settings_for(pa, **changes):
    s = dict(pa.projects.bronchus.BRONCHUS_SETTINGS_DEFAULTS)
    s["algorithmSettings"] = dict(pa.projects.bronchus.default_settings, **changes)
    return s


def check_against_restatement(pa, res, lung, airway, info):
    got = pa.projects.bronchus.run_bronchus_segmentation.last_info
    assert str(res["Auto_Lung"].tensor.dtype) == "torch.uint8"
    assert np.array_equal(res["Auto_Lung"].numpy(), lung)
    for key in ("seed", "lung_mask_hu", "distance_from_sup_slice", "physical_size", "carina_slice", "extend_from_carina"):
        assert got[key] == info[key], (key, got[key], info[key])
    assert [tuple(c) for c in got["candidates"]] == [tuple(c) for c in info["candidates"]]
    if airway is None:
        assert "Auto_Bronchus" not in res
    else:
        assert str(res["Auto_Bronchus"].tensor.dtype) == "torch.uint8"
        assert res["Auto_Bronchus"].numpy().shape == airway.shape
        assert np.array_equal(res["Auto_Bronchus"].numpy(), airway)


def test_restatement_on_the_phantom():
    """The numbers the phantom was designed for, with the margins that keep every decision away from its threshold."""
    img, lung, airway, info = restated()
    assert info["components"] == 3 and len(info["listed"]) == 2
    flat = [l["flatness"] for l in info["listed"]]
    assert np.allclose(flat, [1.385, 1.562], atol=1e-3) and all(abs(f - 2) >= 0.2 for f in flat)
    assert all(abs(size - 2000) >= 500 for k, d, r, elong, size in info["seed_regions"])
    assert info["seed"] == [48, 48, 72] and info["distance_from_sup_slice"] == 3
    sizes = {hu: size for k, d, hu, size, ok in info["candidates"]}
    assert [sizes[h] for h in (-750, -775, -800, -700, -650)] == [1431405] * 5
    assert sizes[-825] == sizes[-850] == 150903 and sizes[-900] == sizes[-950] == 121176
    assert [ok for k, d, hu, size, ok in info["candidates"]] == [False] * 5 + [True, False, True, False]
    assert info["lung_mask_hu"] == -900 and info["physical_size"] == 121176       # B7: the tie keeps -900
    for s in sizes.values():
        assert abs(s - 22000) >= 500 and abs(s - 150000) >= 500
    assert info["carina_slice"] == 38 and info["extend_from_carina"] == 13
    assert all(abs(s - 1000) >= 500 for s in info["carina_sizes"])
    assert int(airway.sum()) == 2487


def test_pipeline_default_settings(host_api):
    pa = host_api
    img, lung, airway, info = restated()
    res = pa.projects.run_bronchus_segmentation(pa.image_from_array(img.copy(), SPACING))
    assert sorted(res) == ["Auto_Bronchus", "Auto_Lung"]
    assert res["Auto_Bronchus"].GetSpacing() == SPACING
    check_against_restatement(pa, res, lung, airway, info)


def test_pipeline_all_candidates(host_api):
    """fast_mode off: every k, distance and HU value runs, so the median branch and the distances 10 and 20 are covered."""
    pa = host_api
    img, lung, airway, info = restated(fast_mode=False)
    assert len(info["candidates"]) == 2 * 3 * 9
    res = pa.projects.run_bronchus_segmentation(pa.image_from_array(img.copy(), SPACING), settings_for(pa, fast_mode=False))
    check_against_restatement(pa, res, lung, airway, info)


@pytest.mark.parametrize("air_column", [55, 38])
def test_pipeline_extra_air_feature(host_api, air_column):
    """An 8 x 8 air column through the top slices, inside the body and away from the trachea: isolated (from z = 55), or
    reaching down into the left lung (from z = 38), where it is a second region of the seed slab.  Whatever the restatement
    does, the build does."""
    pa = host_api
    img, lung, airway, info = restated(air_column=air_column)
    res = pa.projects.run_bronchus_segmentation(pa.image_from_array(img.copy(), SPACING))
    check_against_restatement(pa, res, lung, airway, info)


def test_pipeline_nothing_passes(host_api):
    pa = host_api
    img, lung, airway, info = restated(size_range=(1, 2), hu_values=(-750, -900), distances=(3, 10))      # (a short list: all of it runs twice)
    assert airway is None and len(info["candidates"]) == 2 * 2 * 2
    image = pa.image_from_array(img.copy(), SPACING)
    settings = settings_for(pa, expected_physical_size_range=[1, 2], lung_mask_hu_values=[-750, -900], distance_from_supu_slice_values=[3, 10])
    assert pa.projects.bronchus.generate_airway_mask(None, image, pa.image_from_array(lung.copy(), SPACING), settings["algorithmSettings"]) is None
    res = pa.projects.run_bronchus_segmentation(image, settings)
    assert sorted(res) == ["Auto_Lung"]
    check_against_restatement(pa, res, lung, airway, info)


def test_pipeline_all_tissue_image(host_api):
    pa = host_api
    with pytest.raises(ValueError):
        pa.projects.run_bronchus_segmentation(pa.image_from_array(np.zeros((12, 16, 16), np.float32), SPACING))


def test_pipeline_oblique_direction_and_origin(host_api):
    pa = host_api
    img, lung, airway, info = restated()
    direction, origin = tuple(rot_xyz(20.0, -35.0, 50.0).ravel()), (-120.5, 33.25, 410.0)
    lung_o, airway_o, info_o = R.run_bronchus_segmentation(img, SPACING, origin, direction)
    assert np.array_equal(lung_o, lung) and np.array_equal(airway_o, airway)
    settings = dict(pa.projects.BRONCHUS_SETTINGS_DEFAULTS, outputLungName="Lung", outputBronchusName="Tree")
    res = pa.projects.run_bronchus_segmentation(pa.image_from_array(img.copy(), SPACING, origin, direction), settings)
    assert sorted(res) == ["Lung", "Tree"]
    assert res["Tree"].GetDirection() == direction and res["Tree"].GetOrigin() == origin
    check_against_restatement(pa, {"Auto_Lung": res["Lung"], "Auto_Bronchus": res["Tree"]}, lung_o, airway_o, info_o)


def test_lung_helpers(host_api):
    """detect_holes (B1: the bubble, last in raster order, is not listed), get_external_mask and fill_holes."""
    pa = host_api
    img, lung, airway, info = restated()
    image = pa.image_from_array(img.copy(), SPACING)
    label_image, labels = pa.utils.lung.detect_holes(image)
    lab, want_labels, count = R.detect_holes(img, SPACING)
    assert np.array_equal(label_image.numpy(), lab)
    assert [l["label"] for l in labels] == [l["label"] for l in want_labels] == [1, 2]
    assert all(l["roundness"] is None and l["perimeter"] is None for l in labels)
    external = pa.utils.lung.get_external_mask(label_image, labels)
    assert np.array_equal(external.numpy(), R.closing(lab == 1, 5))
    lung_mask = pa.utils.lung.get_lung_mask(label_image, labels)
    filled = pa.utils.lung.fill_holes(image, label_image, external, lung_mask)
    assert np.array_equal(filled.numpy(), img)                   # the image's maximum is 0: no label counts as a hole
    warm = img + 1.5                                               # maximum 1: label 1 (the outside air) minus the external mask
    m = ((lab >= 1) & (lab <= 1)).astype(np.uint8) - external.numpy() - lung
    want = warm.copy()
    want[R.ndimage.binary_dilation(m == 1, structure=R.itk_ball((3, 3, 3)))] = 50
    got = pa.utils.lung.fill_holes(pa.image_from_array(warm, SPACING), label_image, external, lung_mask)
    assert np.array_equal(got.numpy(), want)
    f = pa.projects.bronchus.fast_mask(lung_mask, 10, 20)
    assert str(f.tensor.dtype) == "torch.float64" and not f.numpy()[10:20].any() and np.array_equal(f.numpy()[20:], lung[20:])
