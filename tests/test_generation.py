"""platipy_amd/generation (dvf.py, augment.py, mask.get_bone_mask) and registration.apply_transform_to_set against
tests/generation_restatement.py -- the reference's arithmetic in fp64 numpy over the CPU oracle -- and, where the contract is
"the same as the member-by-member calls", against those calls, bit for bit.

Bounds (none is tuned):
  * unsmoothed fields of whole-voxel vectors, masks, morphology: np.array_equal;
  * smoothed fields: atol = 3e-6 * (|v|_max / 5 mm) -- what tests/test_kernels.py::test_recursive_gaussian_field grants
    pp_recursive_gaussian_field_f32 against the oracle on a field of 5 mm amplitude, scaled by this field's amplitude;
  * masks after smoothing: equal to the oracle's nearest-neighbour resampling THROUGH THE RETURNED fp32 FIELD (the same
    numbers on both sides, so no tie allowance);
  * the bent image: 24 * 2^-24 * M per voxel, M = the largest corner magnitude of that voxel's trilinear sample
    (tests/test_resample_kernels.py's bound for the fp64-coordinate kernels).
"""
import random

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import generation_restatement as G
from tests import resample_restatement as R

SHAPE, SPACING, ORIGIN = (24, 32, 40), (1.0, 1.2, 2.5), (-20.0, 13.5, 100.25)
NN, LINEAR, BSPLINE = 1, 2, 3


def sphere(centre_zyx, radius_mm, shape=SHAPE):
    z, y, x = np.indices(shape).astype(np.float64)
    d2 = ((z - centre_zyx[0]) * SPACING[2]) ** 2 + ((y - centre_zyx[1]) * SPACING[1]) ** 2 + ((x - centre_zyx[2]) * SPACING[0]) ** 2
    return (d2 <= radius_mm ** 2).astype(np.uint8)


def box(lo, hi, shape=SHAPE):
    m = np.zeros(shape, np.uint8)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    return m


def ct_like(seed=4, shape=SHAPE):
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape).astype(np.float64)
    img = -1000.0 + 1100.0 * np.exp(-(((z - 12) / 9.0) ** 2 + ((y - 16) / 11.0) ** 2 + ((x - 20) / 14.0) ** 2)) + rng.normal(0.0, 5.0, shape)
    return img.astype(np.float32)


def image(pa, arr):
    return pa.image_from_array(arr, SPACING, ORIGIN)


def vol(arr):
    return O.Vol(arr, SPACING, ORIGIN)


def host(img):
    return img.tensor.detach().cpu().numpy()


@pytest.fixture(scope="module")
def masks():
    return {"sphere": sphere((12, 16, 20), 9.0), "box": box((8, 10, 12), (15, 20, 24))}


GENERATORS = {"shift": ("generate_field_shift", G.field_shift, -1.0), "contract": ("generate_field_asymmetric_contract", G.field_asymmetric_contract, 1.0),
              "extend": ("generate_field_asymmetric_extend", G.field_asymmetric_extend, -1.0)}
WHOLE = (2.5, -2.4, 3.0)        # z, y, x in mm: 1, -2 and 3 voxels


@pytest.mark.parametrize("shape_name", ["sphere", "box"])
@pytest.mark.parametrize("kind", list(GENERATORS))
def test_whole_voxel_vectors_unsmoothed(host_api, masks, kind, shape_name):
    pa = host_api
    name, restate, sign = GENERATORS[kind]
    m = masks[shape_name]
    out, tfm, dvf = getattr(pa.generation, name)(image(pa, m), WHOLE, 0)
    keep, f_ref, m_ref = restate(vol(m), WHOLE, 0)
    f = host(dvf)
    assert f.dtype == np.float32 and f.shape == (3,) + SHAPE and dvf.is_vector
    for c, v in enumerate(WHOLE[::-1]):     # x, y, z components
        np.testing.assert_array_equal(f[c], np.where(keep, np.float32(sign * v), np.float32(0.0)))
    np.testing.assert_array_equal(f, f_ref.astype(np.float32))
    np.testing.assert_array_equal(host(out), m_ref)
    assert tfm.GetDisplacementField() is dvf and host(out).dtype == np.uint8 and out.same_grid(dvf)
    moved = np.zeros_like(m)        # the mask moved by (1, -2, 3) voxels, nothing wrapping round
    moved[1:, :-2, 3:] = m[:-1, 2:, :-3]
    if kind == "shift":
        np.testing.assert_array_equal(host(out), moved)
        np.testing.assert_array_equal(keep, (m | moved) != 0)
    elif kind == "extend":
        np.testing.assert_array_equal(keep, moved != 0)
    else:
        np.testing.assert_array_equal(keep, m != 0)


@pytest.mark.parametrize("smooth", [5, (2, 3, 4)], ids=["scalar5", "xyz234"])
@pytest.mark.parametrize("kind", list(GENERATORS))
def test_smoothed_fields(host_api, masks, kind, smooth):
    pa = host_api
    name, restate, _ = GENERATORS[kind]
    m, v = masks["sphere"], (5.0, -7.0, 10.0)
    out, tfm, dvf = getattr(pa.generation, name)(image(pa, m), v, smooth)
    _, f_ref, _ = restate(vol(m), v, smooth)
    f = host(dvf)
    atol = 3e-6 * (max(abs(c) for c in v) / 5.0)
    err = np.abs(f - f_ref).max()
    print(f"{kind} smooth={smooth}: max |field - restatement| = {err:.3e} (bound {atol:.3e})")
    assert err <= atol, (err, atol)
    assert np.abs(f).max() > 1.0 and tfm.GetDisplacementField() is dvf
    np.testing.assert_array_equal(host(out), G.warp_mask(vol(m), f).arr)


def test_contract_real_dvf(host_api, masks):
    """compute_real_dvf=True (dvf.py:129-141): the template is replaced by the registration of the two masks' registration
    structures (expansion 3), the contracted one as the fixed image, [4, 2] / [20, 10] -- public calls held to the oracle
    elsewhere, so the field must equal their composition bit for bit."""
    pa = host_api
    from platipy_amd import runtime

    m, v = masks["sphere"], (5.0, -4.8, 6.0)        # 2, -4 and 6 voxels: the contracted mask has no nearest-neighbour ties
    mask = image(pa, m)
    out, tfm, dvf = pa.generation.generate_field_asymmetric_contract(mask, v, 5, compute_real_dvf=True)
    _, _, contracted = G.field_asymmetric_contract(vol(m), v, 0)
    assert 0 < contracted.sum() and not np.array_equal(contracted, m)
    reg = pa.registration.convert_mask_to_reg_structure(mask, expansion=3)
    reg_def = pa.registration.convert_mask_to_reg_structure(image(pa, contracted), expansion=3)
    _, _, raw = pa.registration.fast_symmetric_forces_demons_registration(reg_def, reg, isotropic_resample=True, resolution_staging=[4, 2],
                                                                           iteration_staging=[20, 10])
    want = raw.tensor.clone()
    runtime.context(want.device).recursive_gaussian_field(want, mask.geom(), [5.0, 5.0, 5.0])
    np.testing.assert_array_equal(host(dvf), want.cpu().numpy())
    assert tfm.GetDisplacementField() is dvf and host(dvf).any()
    np.testing.assert_array_equal(host(out), G.warp_mask(vol(m), host(dvf)).arr)
    # without smoothing the registration's field is returned as it is, not the template
    _, _, unsmoothed = pa.generation.generate_field_asymmetric_contract(mask, v, 0, compute_real_dvf=True)
    np.testing.assert_array_equal(host(unsmoothed), host(raw))


BEND_CUTS = [("z", "inf"), ("z", "sup"), ("y", "post"), ("y", "ant"), ("x", "left"), ("x", "right"), False]


@pytest.fixture(scope="module")
def bend_case():
    body = 1 - box((9, 12, 15), (13, 18, 22))       # the whole volume, so that the bend pushes border voxels out, less a hole
    return ct_like(), body, (11, 15, 19), [0.3, -0.5, 1.0]


@pytest.mark.parametrize("cut", BEND_CUTS, ids=lambda c: "-".join(c) if c else "nocut")
def test_radial_bend_unsmoothed(host_api, bend_case, cut):
    pa = host_api
    ct, body, ref, axis = bend_case
    _, tfm, dvf = pa.generation.generate_field_radial_bend(image(pa, ct), image(pa, body), ref, axis, 0.1, cut, 0)
    want, cut_mask = G.field_radial_bend(SHAPE, body, ref, axis, 0.1, cut)
    f = host(dvf)
    np.testing.assert_allclose(f, want, rtol=1e-6, atol=0.0)
    np.testing.assert_array_equal((f != 0).any(axis=0) & ~cut_mask, False)      # zero outside the cut mask
    assert (f != 0).any() and tfm.GetDisplacementField() is dvf
    if cut is not False:
        assert cut_mask.sum() < (body != 0).sum()


def test_radial_bend_fractional_reference_point(host_api, bend_case):
    """Without a cut the reference point is only subtracted (dvf.py:382), so it may lie between voxels and is not truncated;
    with a cut it is a slice bound, and a fraction is the TypeError it is in the reference."""
    pa = host_api
    ct, body, _, axis = bend_case
    ref = (10.5, 15.25, 18.75)
    _, _, dvf = pa.generation.generate_field_radial_bend(image(pa, ct), image(pa, body), ref, axis, 0.1, False, 0)
    want, _ = G.field_radial_bend(SHAPE, body, ref, axis, 0.1, False)
    truncated, _ = G.field_radial_bend(SHAPE, body, (10, 15, 18), axis, 0.1, False)
    np.testing.assert_allclose(host(dvf), want, rtol=1e-6, atol=0.0)
    assert np.abs(want - truncated).max() > 0.01
    with pytest.raises(TypeError):
        pa.generation.generate_field_radial_bend(image(pa, ct), image(pa, body), ref, axis, 0.1, ("z", "inf"), 0)


def test_radial_bend_scale_false_and_defaults(host_api, bend_case):
    pa = host_api
    ct, body, ref, _ = bend_case
    bent, _, dvf = pa.generation.generate_field_radial_bend(image(pa, ct), image(pa, body), ref, scale=False, gaussian_smooth=0)
    assert not host(dvf).any()
    # the zero field resamples every voxel onto itself, up to the rounding of ((s i + o) - o) / s and of the lerps
    np.testing.assert_allclose(host(bent), ct, rtol=0.0, atol=24.0 * 2.0 ** -24 * np.abs(ct).max())


def test_radial_bend_smoothed_and_image(host_api, bend_case):
    pa = host_api
    ct, body, ref, axis = bend_case
    bent, _, dvf = pa.generation.generate_field_radial_bend(image(pa, ct), image(pa, body), ref, axis, 0.1, ("z", "inf"), 5)
    raw, _ = G.field_radial_bend(SHAPE, body, ref, axis, 0.1, ("z", "inf"))
    f_ref = G.smooth(vol(ct), raw, 5)
    f = host(dvf)
    atol = 3e-6 * (np.abs(raw).max() / 5.0)
    err = np.abs(f - f_ref).max()
    print(f"radial bend: max |field - restatement| = {err:.3e} (bound {atol:.3e}), amplitude {np.abs(raw).max():.3f}")
    assert err <= atol, (err, atol)
    default = int(ct.min())
    want = G.warp_image_linear(vol(ct), f, default).arr
    g = R.Grid(SHAPE[::-1], SPACING, ORIGIN)
    ref_ = R.resample(ct, g, g, field=f, default=default)
    tol = np.where(ref_["inside"], 24.0 * 2.0 ** -24 * ref_["M"], 0.0)
    got = host(bent)
    ratio = (np.abs(got.astype(np.float64) - want) / np.maximum(tol, 1e-300))[ref_["inside"]].max()
    print(f"radial bend: image error / bound = {ratio:.3f}")
    assert (np.abs(got.astype(np.float64) - want) <= tol).all(), ratio
    assert got.dtype == np.float32 and 0 < (~ref_["inside"]).sum() and (got[~ref_["inside"]] == default).all()


# --------------------------------------------------------------------------------------
# expand

EXPAND = {"positive": (3, 3, 3), "negative": (-3, -3, -3), "mixed": (-3, 3, 3)}


@pytest.fixture(scope="module")
def bone():
    return box((4, 20, 6), (20, 24, 30))


@pytest.mark.parametrize("sign", list(EXPAND))
def test_expand_morphology(host_api, masks, sign):
    pa = host_api
    from platipy_amd.generation import dvf as D

    m = masks["sphere"]
    want, radii = G.expand_mask(vol(m), EXPAND[sign])
    np.testing.assert_array_equal(host(D._expand_mask(image(pa, m), EXPAND[sign])), want)
    # (z, y, x) mm / (2.5, 1.2, 1.0) -> (x, y, z) voxels 3, 2, 1
    assert radii == {"positive": [[3, 2, 1], [0, 0, 0]], "negative": [[0, 0, 0], [3, 2, 1]], "mixed": [[3, 2, 0], [0, 0, 1]]}[sign]
    assert (want.sum() > m.sum()) if sign == "positive" else (want.sum() < m.sum()) if sign == "negative" else True
    np.testing.assert_array_equal(host(D._expand_mask(image(pa, m), 0)), m)         # all zero: the erosion arm, radius 0


@pytest.mark.parametrize("internal", [True, False], ids=["regstruct", "binary"])
@pytest.mark.parametrize("with_bone", [False, True], ids=["nobone", "bone"])
@pytest.mark.parametrize("sign", list(EXPAND))
def test_expand_field(host_api, masks, bone, sign, with_bone, internal):
    pa = host_api
    from platipy_amd import runtime
    from platipy_amd.generation import dvf as D

    m = masks["sphere"]
    mask = image(pa, m)
    bone_mask = image(pa, bone) if with_bone else False
    out, tfm, dvf = pa.generation.generate_field_expand(mask, bone_mask, EXPAND[sign], 5, internal)
    # the structures that were registered: morphology by the oracle, + bone, (the registration structure of both)
    fixed, moving = D._expand_structures(mask, bone_mask, EXPAND[sign], internal)
    grown, _ = G.expand_mask(vol(m), EXPAND[sign])
    if internal:
        want_f = pa.registration.convert_mask_to_reg_structure(image(pa, grown + bone if with_bone else grown))
        want_m = pa.registration.convert_mask_to_reg_structure(image(pa, m + bone if with_bone else m))
    else:
        want_f, want_m = image(pa, grown + bone if with_bone else grown), image(pa, m + bone if with_bone else m)
    np.testing.assert_array_equal(host(fixed), host(want_f))
    np.testing.assert_array_equal(host(moving), host(want_m))
    # the field: the recursive Gaussian of what the public registration call returns for those two structures
    _, _, raw = pa.registration.fast_symmetric_forces_demons_registration(fixed, moving, isotropic_resample=True, resolution_staging=[4, 2],
                                                                           iteration_staging=[10, 10])
    want = raw.tensor.clone()
    runtime.context(want.device).recursive_gaussian_field(want, mask.geom(), [5.0, 5.0, 5.0])
    np.testing.assert_array_equal(host(dvf), want.cpu().numpy())
    assert tfm.GetDisplacementField() is dvf and host(dvf).any()
    np.testing.assert_array_equal(host(out), G.warp_mask(vol(m), host(dvf)).arr)
    n_in, n_out = int(m.sum()), int(host(out).sum())
    print(f"expand {sign} bone={with_bone} internal={internal}: {n_in} -> {n_out} voxels")
    if sign == "positive":
        assert n_out > n_in
    elif sign == "negative":
        assert n_out < n_in


def test_contract_augment_quirk(host_api, masks):
    pa = host_api
    from platipy_amd.generation import dvf as D

    mask = image(pa, masks["sphere"])
    aug = pa.generation.ContractAugment(mask, vector_contract=(10, 10, 10))
    assert aug.contract == [-10, -8, -4]        # int(-10 / 1.0), int(-10 / 1.2), int(-10 / 2.5): z, y, x mm over x, y, z spacing
    # ... and generate_field_expand divides by the spacing again: (-10 / 2.5, -8 / 1.2, -4 / 1.0) as z, y, x -> x, y, z radii
    assert np.abs(D._expand_radii(mask, aug.contract)).astype(int).tolist() == [4, 6, 4]
    assert G.expand_mask(vol(masks["sphere"]), aug.contract)[1] == [[0, 0, 0], [4, 6, 4]]


def test_get_bone_mask(host_api):
    pa = host_api
    rng = np.random.default_rng(12)
    ct = ct_like(5)
    ct[box((6, 8, 10), (18, 22, 30)) != 0] = 900.0
    holes = rng.random(SHAPE) < 0.15
    ct[holes] = 100.0                       # below the window: holes for the closing to fill
    ct[2, 3, 4], ct[2, 3, 5], ct[2, 3, 6] = 350.0, 3500.0, 3500.5       # both ends of the window are inside it
    for size in (5, (1, 2, 1), False):
        got = host(pa.generation.get_bone_mask(image(pa, ct), max_hole_size=size))
        np.testing.assert_array_equal(got, G.bone_mask(vol(ct), max_hole_size=size if size is not False else 0))
    plain = host(pa.generation.get_bone_mask(image(pa, ct), max_hole_size=False))
    assert plain[2, 3, 4] == 1 and plain[2, 3, 5] == 1 and plain[2, 3, 6] == 0 and got.dtype == np.uint8


# --------------------------------------------------------------------------------------
# augmentation

@pytest.mark.parametrize("count", [2, 3])
def test_apply_augmentation(host_api, masks, count):
    pa = host_api
    gen = pa.generation
    ct = image(pa, ct_like())
    ms = [image(pa, masks["sphere"]), image(pa, masks["box"])]
    augs = [gen.ShiftAugment(ms[0], (2.5, -3.0, 4.0), 3), gen.ShiftAugment(ms[1], (-5.0, 2.0, 1.0), (2, 3, 4)),
            gen.ExpandAugment(ms[0], (3, 3, 3), 4)][:count]
    img_d, masks_d, dvf = gen.apply_augmentation(ct, augs, ms)
    parts = [a.augment() for a in augs]
    total = parts[0][1].tensor.clone()
    for _, field in parts[1:]:
        total = total + field.tensor
    np.testing.assert_array_equal(host(dvf), total.cpu().numpy())
    for (tfm, field), again in zip(parts, [a.augment() for a in augs]):      # the members' own fields were not added into
        np.testing.assert_array_equal(host(field), host(again[1]))
    composite = pa.CompositeTransform([tfm for tfm, _ in parts])
    want = pa.registration.apply_transform(ct, transform=composite, default_value=int(host(ct).min()), interpolator=LINEAR)
    np.testing.assert_array_equal(host(img_d), host(want))
    assert len(masks_d) == 2 and not np.array_equal(host(img_d), host(ct))
    for m, md in zip(ms, masks_d):
        np.testing.assert_array_equal(host(md), host(pa.registration.apply_transform(m, transform=composite, default_value=0, interpolator=NN)))
        assert md.tensor.dtype == torch.uint8
    # without masks: (image, dvf); a single augmentation need not be in a list
    two = gen.apply_augmentation(ct, augs[0])
    assert len(two) == 2
    np.testing.assert_array_equal(host(two[1]), host(parts[0][1]))
    np.testing.assert_array_equal(host(two[0]), host(pa.registration.apply_transform(ct, transform=parts[0][0], default_value=int(host(ct).min()),
                                                                                     interpolator=LINEAR)))


def test_apply_augmentation_type_errors(host_api, masks):
    pa = host_api
    gen = pa.generation
    m = image(pa, masks["sphere"])
    apply, shift = gen.apply_augmentation, gen.ShiftAugment(m)      # outside the blocks: a missing name is not the error meant
    with pytest.raises(AttributeError, match=r"^image should be a platipy_amd\.Image$"):
        apply(masks["sphere"], shift)
    with pytest.raises(AttributeError, match=r"^Each augmentation must be of type DeformableAugment$"):
        apply(m, [shift, "shift"])
    with pytest.raises(AttributeError, match=r"^augmentation must be a DeformableAugment or an iterable"):
        apply(m, 3)


def test_generate_random_augmentation_is_seeded(host_api, masks):
    pa = host_api
    gen = pa.generation
    ct = image(pa, ct_like())
    ms = [image(pa, masks["sphere"]), image(pa, masks["box"]), image(pa, sphere((10, 14, 22), 6.0)), image(pa, box((3, 4, 5), (9, 12, 20)))]

    def draw():
        random.seed(7)
        order = list(ms)
        augs = gen.generate_random_augmentation(ct, order)
        described = []
        for a in augs:
            args = {k: v for k, v in vars(a).items() if k not in ("mask", "bone_mask")}
            described.append((type(a).__name__, ms.index(a.mask), args, None if getattr(a, "bone_mask", False) is False else host(a.bone_mask).sum()))
        return described

    first, second = draw(), draw()
    assert first == second and len(first) == len(ms)
    assert sorted(d[1] for d in first) == [0, 1, 2, 3]
    for name, _, args, bone_voxels in first:
        assert name in ("ShiftAugment", "ContractAugment", "ExpandAugment") and 3 <= args["gaussian_smooth"] <= 5
        assert (bone_voxels is None) == (name == "ShiftAugment")


# --------------------------------------------------------------------------------------
# apply_transform_to_set: every path returns what the member-by-member calls return

def member_calls(pa, img, labels, reference, transform, default, interp):
    at = pa.registration.apply_transform
    return (None if img is None else at(img, reference, transform, default, interp)), [at(lab, reference, transform, 0, NN) for lab in labels]


def assert_set_equal(got, want):
    assert (got[0] is None) == (want[0] is None) and len(got[1]) == len(want[1])
    for a, b in zip(([got[0]] if got[0] is not None else []) + got[1], ([want[0]] if want[0] is not None else []) + want[1]):
        assert a.tensor.dtype == b.tensor.dtype and a.same_grid(b)
        np.testing.assert_array_equal(host(a), host(b))


@pytest.fixture
def set_case(host_api, masks):
    pa = host_api
    ct = image(pa, ct_like())
    labels = [image(pa, masks["sphere"]), image(pa, masks["box"] * 7)]
    rng = np.random.default_rng(2)
    field = pa.Image(torch.from_numpy((rng.normal(0.0, 3.0, (3,) + SHAPE)).astype(np.float32)).to(ct.device), SPACING, ORIGIN, is_vector=True)
    affine = pa.AffineTransform(np.array([[1.02, 0.03, 0.0], [-0.02, 0.98, 0.01], [0.0, 0.02, 1.01]]), (1.5, -2.0, 0.5), (0.0, 30.0, 130.0))
    transform = pa.CompositeTransform([affine, pa.DisplacementFieldTransform(field)])
    reference = pa.Image(torch.zeros((20, 30, 36), dtype=torch.float32, device=ct.device), (1.1, 1.3, 2.9), (-19.0, 14.0, 101.0))
    return pa, ct, labels, reference, transform


@pytest.mark.parametrize("case", ["fused", "fused_nearest", "fused_no_reference", "labels_only", "image_only", "float64_image", "bspline",
                                  "other_grid", "int16_label", "uint8_image", "twenty_labels"])
def test_apply_transform_to_set(set_case, case, monkeypatch):
    pa, ct, labels, reference, transform = set_case
    interp, img = LINEAR, ct
    if case == "fused_nearest":
        interp = NN
    elif case == "fused_no_reference":
        reference = None
    elif case == "labels_only":
        img = None
    elif case == "image_only":
        labels = []
    elif case == "float64_image":
        img = ct.astype(torch.float64)
    elif case == "bspline":
        interp = BSPLINE
    elif case == "other_grid":
        other = pa.Image(labels[1].tensor[:, :, :-3].contiguous(), SPACING, (ORIGIN[0] + 1.0, ORIGIN[1], ORIGIN[2]))
        labels = [labels[0], other]
    elif case == "int16_label":
        labels = [labels[0], labels[1].astype(torch.int16)]
    elif case == "uint8_image":
        img = labels[1]
    elif case == "twenty_labels":
        labels = [pa.Image(torch.roll(labels[k % 2].tensor, k, dims=2) * (k + 1), SPACING, ORIGIN) for k in range(20)]
    calls = []
    from platipy_amd import _lib

    real = _lib.Context.resample_set
    monkeypatch.setattr(_lib.Context, "resample_set", lambda self, *a, **k: (calls.append(len(k["labels"])), real(self, *a, **k))[1])
    got = pa.registration.apply_transform_to_set(img, labels, reference, transform, -1000, interp)
    assert calls == {"fused": [2], "fused_nearest": [2], "fused_no_reference": [2], "labels_only": [2], "image_only": [0], "float64_image": [2],
                     "twenty_labels": [16, 4]}.get(case, []), calls
    assert_set_equal(got, member_calls(pa, img, labels, reference, transform, -1000, interp))
    assert all((g.tensor != 0).any() for g in got[1]) and (got[0] is None or (got[0].tensor == (0 if case == "uint8_image" else -1000)).any())


def test_apply_transform_to_set_of_nothing(host_api):
    assert host_api.registration.apply_transform_to_set(None, []) == (None, [])
