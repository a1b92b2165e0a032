"""inverse_transform: the inverse of whatever apply_transform takes, checked by the round trip
transform_to_displacement_field(CompositeTransform([T, inverse_transform(T)]), reference) = T(T^-1(p)) - p.

For a field member u with inverse estimate v that round trip is c = v + u_lin(. + v), the composition the inversion itself
measures, so it is compared -- voxel by voxel on the box at least 3 voxels from every face, nothing excluded -- with the
fp64 restatement's own residual for the same member fields and iteration count.  The allowance on top of it, in the scaled
norm |. / spacing|_2 (voxels), is derived, not fitted:
 * e_r[K] of tests/test_field_inverse.py's recurrence (inversion_bound): the error of the kernel's K-iteration inverse
   carried through one more composition, the composition's own fp32 roundings included;
 * where linear members surround the fields (T = A o F), the inverse field is sampled off its grid points, which adds
   the interpolation's roundings 17 eps32 Vs, and four more fp32 images are formed along the chain (A^-1's displacement,
   two compositions, A's displacement), each rounding a displacement of at most Dmax once or twice and each seen through
   the two interpolations that follow it: 8 eps32 Dmax (1 + L_u)(1 + L_v).  Linear maps act on points in fp64.
The restatement also asserts that every intermediate point of the box stays at least 0.5 voxel inside every member's buffer."""
import numpy as np
import pytest

from tests import field_inverse_restatement as R

SIZE, SPACING, ORIGIN = (33, 20, 12), (0.9, 1.1, 2.5), (-12.0, 7.5, 30.0)
K = 6
EPS32 = 2.0 ** -24
BOX = (slice(3, -3), slice(3, -3), slice(3, -3))


def zyx(size):
    return (size[2], size[1], size[0])


def grid_points():
    z, y, x = np.indices(zyx(SIZE)).astype(np.float64)
    return np.stack([ORIGIN[0] + x * SPACING[0], ORIGIN[1] + y * SPACING[1], ORIGIN[2] + z * SPACING[2]])


def sample(field, pts):
    """A field on the reference grid at physical points -> (values [3, ...], the smallest distance inside the buffer's
    [0, n - 1] box, negative when a point is closer than 0.5 voxel to a buffer face)."""
    c = [(pts[a] - ORIGIN[a]) / SPACING[a] for a in range(3)]
    depth = min(float(np.minimum(c[a], SIZE[a] - 1 - c[a])[BOX].min()) for a in range(3))
    cc = [np.clip(c[a], 0.0, SIZE[a] - 1.0) for a in range(3)]
    return np.stack([R.linear_sample(field[d].astype(np.float64), cc[0], cc[1], cc[2]) for d in range(3)]), depth


def scaled(d):
    return np.sqrt(((d / np.asarray(SPACING).reshape(3, 1, 1, 1)) ** 2).sum(0))


def small_affine(pa):
    a = np.radians(2.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    centre = [ORIGIN[i] + 0.5 * (SIZE[i] - 1) * SPACING[i] for i in range(3)]
    return pa.AffineTransform(rot, (1.2, -1.5, 3.0), centre)        # <= 1.5 voxels of translation, 2 degrees


def field_image(pa, u):
    import torch

    return pa.Image(torch.from_numpy(u).to(pa.runtime.default_device()), SPACING, ORIGIN)


def reference_image(pa):
    import torch

    return pa.Image(torch.zeros(zyx(SIZE), dtype=torch.float32, device=pa.runtime.default_device()), SPACING, ORIGIN)


def round_trip(pa, T, reference, **kw):
    from platipy_amd.registration import inverse_transform, transform_to_displacement_field

    Tinv = inverse_transform(T, reference, maximum_number_of_iterations=K, max_error_tolerance_threshold=0.0,
                             mean_error_tolerance_threshold=0.0, **kw)
    D = transform_to_displacement_field(pa.CompositeTransform([T, Tinv]), reference)
    return Tinv, D.numpy().astype(np.float64)


def report_dice(pa, T, Tinv, reference, name):
    """A label through T and back through the inverse: reported, not asserted -- no reference number exists for it."""
    import torch

    from platipy_amd.registration import apply_transform
    from tests.helpers import dice

    z, y, x = np.indices(zyx(SIZE))
    ball = (((x - 16) / 9.0) ** 2 + ((y - 10) / 6.0) ** 2 + ((z - 6) / 3.5) ** 2 <= 1.0).astype(np.uint8)
    label = pa.Image(torch.from_numpy(ball).to(pa.runtime.default_device()), SPACING, ORIGIN)
    there = apply_transform(label, reference, T)
    back = apply_transform(there, reference, Tinv)
    print(f"label round trip through {name}: Dice {dice(back.numpy(), ball):.4f}")


def test_identity_and_linear_members(host_api):
    pa = host_api
    from platipy_amd.registration import inverse_transform

    ref = reference_image(pa)
    ident = inverse_transform(pa.Transform())
    assert type(ident) is pa.Transform and type(inverse_transform(None)) is pa.Transform
    _, D = round_trip(pa, pa.Transform(), ref)
    assert not D.any()
    A = small_affine(pa)
    Ainv, D = round_trip(pa, A, ref)
    assert isinstance(Ainv, pa.AffineTransform)
    # (A A^-1 - I) p in fp64 on positions below 100 mm: a few dozen roundings of 2^-53 x 100
    assert np.abs(D).max() <= 1e-11
    B = pa.AffineTransform(np.diag([1.05, 0.97, 1.0]), (0.5, 0.0, -1.0))
    comp = pa.CompositeTransform([A, B])
    got, want = inverse_transform(comp), comp.GetInverse()
    assert all(np.array_equal(g, w) for g, w in zip(got.matrix_offset(), want.matrix_offset()))
    _, D = round_trip(pa, comp, ref)
    assert np.abs(D).max() <= 1e-11
    # GetInverse itself is unchanged: a member that is not linear still raises there
    F = pa.DisplacementFieldTransform(field_image(pa, R.windowed_sinusoid(zyx(SIZE), SPACING, (1.0, 1.0, 1.0))))
    with pytest.raises(TypeError):
        F.GetInverse()
    with pytest.raises(TypeError):
        pa.CompositeTransform([A, F]).GetInverse()


def check_field_round_trip(u, D, chain_affine=None):
    """D = T(T^-1(p)) - p of the product against the restatement for the member field u (and the affine (A, off) around
    it: T = A o F)."""
    v, hist = R.invert(u, SPACING, np.eye(3), K + 1, 0.0, 0.0)
    v = hist[K - 1]["v"]
    b = R.inversion_bound(u, SPACING, np.eye(3), hist, K + 1)
    p = grid_points()
    if chain_affine is None:
        q, lin = p, np.eye(3)
    else:
        lin, off = chain_affine
        q = np.einsum("rc,czyx->rzyx", np.linalg.inv(lin), p - off.reshape(3, 1, 1, 1))
    vq, d0 = sample(v, q)
    uq, d1 = sample(u, q + vq)
    c = vq + uq
    _, d2 = sample(u, q + c)        # (where T's own field would be read next: the end point is inside too)
    assert min(d0, d1, d2) >= 0.0, "an intermediate point of the box leaves a member's buffer by more than allowed"
    ref_s = scaled(c)
    extra = 0.0
    if chain_affine is not None:
        Vs = float(scaled(v).max())
        Dmax = float(max(scaled(q - p).max(), scaled(q + vq - p).max(), scaled(q + c - p).max()))
        extra = 17.0 * EPS32 * Vs + 8.0 * EPS32 * Dmax * (1.0 + b["L"]) * (1.0 + R.lipschitz_scaled(v, SPACING))
    S = np.diag(1.0 / np.asarray(SPACING)) @ lin @ np.diag(SPACING)
    gain = float(np.linalg.norm(S, 2))
    got_s = scaled(D)
    bound = b["e_r"][K] + extra
    excess = (got_s - gain * (ref_s + bound))[BOX].max()
    print(f"round trip: max {got_s[BOX].max():.3e} voxel, restatement {ref_s[BOX].max():.3e}, allowance {bound:.3e}, worst margin {excess:.3e}")
    assert excess <= 0.0
    return v


def test_displacement_field(host_api):
    pa = host_api
    ref = reference_image(pa)
    u = R.windowed_sinusoid(zyx(SIZE), SPACING, (1.8, 1.2, 2.4), seed=1)
    T = pa.DisplacementFieldTransform(field_image(pa, u))
    Tinv, D = round_trip(pa, T, ref)
    assert isinstance(Tinv, pa.DisplacementFieldTransform) and Tinv.field.same_grid(T.field)
    v = check_field_round_trip(u, D)
    # the inverse itself, against the restatement's
    b = R.inversion_bound(u, SPACING, np.eye(3), R.invert(u, SPACING, np.eye(3), K, 0.0, 0.0)[1], K)
    assert scaled(Tinv.field.numpy().astype(np.float64) - v).max() <= b["E"]
    report_dice(pa, T, Tinv, ref, "a displacement field")


def test_affine_then_field_chain(host_api):
    """Composite([affine, field]): what linear_registration + demons produce (the field is applied first)."""
    pa = host_api
    ref = reference_image(pa)
    u = R.windowed_sinusoid(zyx(SIZE), SPACING, (1.8, 1.2, 2.4), seed=2)
    A = small_affine(pa)
    T = pa.CompositeTransform([A, pa.DisplacementFieldTransform(field_image(pa, u))])
    Tinv, D = round_trip(pa, T, ref)
    parts = Tinv.flatten()
    assert isinstance(parts[0], pa.DisplacementFieldTransform) and isinstance(parts[1], pa.AffineTransform) and len(parts) == 2
    check_field_round_trip(u, D, chain_affine=A.matrix_offset())
    report_dice(pa, T, Tinv, ref, "affine o field")


def test_bspline_needs_and_uses_a_reference(host_api):
    import torch

    pa = host_api
    from platipy_amd.registration import inverse_transform

    ref = reference_image(pa)
    T = pa.bspline_transform_initializer(ref, (4, 3, 2))
    g = torch.Generator().manual_seed(7)
    T.coefficients = (1.5 * (torch.rand(tuple(T.coefficients.shape), generator=g) - 0.5)).float().to(T.coefficients.device)
    with pytest.raises(ValueError):
        inverse_transform(T)
    with pytest.raises(ValueError):
        inverse_transform(pa.CompositeTransform([small_affine(pa), T]))
    Tinv, D = round_trip(pa, T, ref)
    assert isinstance(Tinv, pa.DisplacementFieldTransform) and Tinv.field.same_grid(ref)
    u = T.displacement_field(ref).cpu().numpy()          # the member field both sides use: the dense evaluation on the reference
    check_field_round_trip(u, D)
    report_dice(pa, T, Tinv, ref, "a B-spline")
