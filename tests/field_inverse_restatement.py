"""numpy fp64 restatement of the displacement-field inversion, its residual and the Jacobian determinant
(itk::InvertDisplacementFieldImageFilter / itk::DisplacementFieldJacobianDeterminantFilter of ITK 5.3 as recalled
[ITK-upstream, unverified here]).  Written from the rule in include/platipy_amd.h, not from the kernels.

Fields are planar [3, Z, Y, X] arrays of physical components (x, y, z); spacing is (sx, sy, sz); direction is 3 x 3."""
import numpy as np


def index_displacement(v, spacing, direction):
    """Physical displacement -> continuous-index displacement, diag(1 / spacing) Dir^T v, as [3 (x, y, z), Z, Y, X]."""
    M = np.diag(1.0 / np.asarray(spacing, dtype=np.float64)) @ np.asarray(direction, dtype=np.float64).reshape(3, 3).T
    return np.einsum("ac,czyx->azyx", M, np.asarray(v, dtype=np.float64))


def inside_buffer(c, n):
    """itk::ImageFunction::IsInsideBuffer on one axis: [-0.5, n - 0.5)."""
    return (c >= -0.5) & (c < n - 0.5)


def plane_margin(c, n):
    """Distance of the continuous indices from the nearer of the two +-0.5-voxel buffer planes of an axis."""
    return np.minimum(np.abs(c + 0.5), np.abs(c - (n - 0.5)))


def linear_sample(vol, cx, cy, cz):
    """itk::LinearInterpolateImageFunction on points known to be inside the buffer: base = floor(c); below index 0 the
    weight is 0 on index 0, on the last index the upper neighbour is the index itself."""
    nz, ny, nx = vol.shape
    out = None

    def axis(c, n):
        b = np.floor(c)
        f = c - b
        b = b.astype(np.int64)
        w = np.where(b < 0, 0.0, f)
        i0 = np.clip(b, 0, n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        return i0, i1, w

    x0, x1, wx = axis(cx, nx)
    y0, y1, wy = axis(cy, ny)
    z0, z1, wz = axis(cz, nz)
    for zi, wzk in ((z0, 1.0 - wz), (z1, wz)):
        for yi, wyk in ((y0, 1.0 - wy), (y1, wy)):
            for xi, wxk in ((x0, 1.0 - wx), (x1, wx)):
                term = vol[zi, yi, xi] * (wzk * wyk * wxk)
                out = term if out is None else out + term
    return out


def residual(u, v, spacing, direction=np.eye(3)):
    """One composition of the estimate v with the field u -> dict(r [3, Z, Y, X] = -(v + u_lin(p + v)) or -v outside,
    s [Z, Y, X] the scaled norm, inside [Z, Y, X] bool, margin: the smallest distance of any warped point from a +-0.5 plane,
    M, mean)."""
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    _, nz, ny, nx = u.shape
    z, y, x = np.indices((nz, ny, nx)).astype(np.float64)
    dv = index_displacement(v, spacing, direction)
    cx, cy, cz = x + dv[0], y + dv[1], z + dv[2]
    ins = inside_buffer(cx, nx) & inside_buffer(cy, ny) & inside_buffer(cz, nz)
    margin = float(min(plane_margin(cx, nx).min(), plane_margin(cy, ny).min(), plane_margin(cz, nz).min()))
    # (outside points are clipped only so that the gather stays defined; their samples are discarded)
    ccx, ccy, ccz = np.clip(cx, -0.5, nx - 0.5), np.clip(cy, -0.5, ny - 0.5), np.clip(cz, -0.5, nz - 0.5)
    c = v.copy()
    for d in range(3):
        c[d] += np.where(ins, linear_sample(u[d], ccx, ccy, ccz), 0.0)
    r = -c
    sp = np.asarray(spacing, dtype=np.float64).reshape(3, 1, 1, 1)
    s = np.sqrt(((r / sp) ** 2).sum(0))
    return {"r": r, "s": s, "inside": ins, "margin": margin, "M": float(s.max()), "mean": float(s.sum() / s.size),
            "index_displacement": float(np.abs(dv).max())}


def border_mask(shape):
    nz, ny, nx = shape
    z, y, x = np.indices(shape)
    return (x == 0) | (x == nx - 1) | (y == 0) | (y == ny - 1) | (z == 0) | (z == nz - 1)


def invert(u, spacing, direction=np.eye(3), maximum_number_of_iterations=10, max_error_tolerance_threshold=0.1,
           mean_error_tolerance_threshold=0.001, enforce_boundary_condition=True, initial_estimate=None):
    """-> (v, history): history[k - 1] = dict(M, mean, margin, inside, index_displacement, v_norm, v) of iteration k; v is the
    estimate AFTER the iteration, the others are taken at its composition."""
    u = np.asarray(u, dtype=np.float64)
    v = np.zeros_like(u) if initial_estimate is None else np.asarray(initial_estimate, dtype=np.float64).copy()
    sp = np.asarray(spacing, dtype=np.float64).reshape(3, 1, 1, 1)
    border = border_mask(u.shape[1:])
    M, mean, k, history = np.inf, np.inf, 0, []
    while k < maximum_number_of_iterations and M > max_error_tolerance_threshold and mean > mean_error_tolerance_threshold:
        k += 1
        res = residual(u, v, spacing, direction)
        r, s, M, mean = res["r"], res["s"], res["M"], res["mean"]
        eps = 0.75 if k == 1 else 0.5
        clip = s > eps * M
        scale = np.where(clip, eps * M / np.where(clip, s, 1.0), 1.0)
        history.append({"M": M, "mean": mean, "margin": res["margin"], "inside": res["inside"],
                        "index_displacement": res["index_displacement"], "v_norm": float(np.sqrt(((v / sp) ** 2).sum(0)).max())})
        v = v + eps * (r * scale)
        if enforce_boundary_condition:
            v[:, border] = 0.0
        history[-1]["v"] = v.copy()
    return v, history


def jacobian_determinant(u, spacing, use_image_spacing=True):
    """det(I + J), J[i][j] = 0.5 w_i (u_j(x + e_i) - u_j(x - e_i)), neighbours outside the buffer replaced by the voxel."""
    u = np.asarray(u, dtype=np.float64)
    w = 1.0 / np.asarray(spacing, dtype=np.float64) if use_image_spacing else np.ones(3)
    J = np.zeros((3, 3) + u.shape[1:])
    for i, ax in enumerate((2, 1, 0)):          # index axis x, y, z -> array axis
        pad = [(0, 0)] * 3
        pad[ax] = (1, 1)
        for j in range(3):
            e = np.pad(u[j], pad, mode="edge")
            hi = np.take(e, np.arange(2, e.shape[ax]), axis=ax)
            lo = np.take(e, np.arange(0, e.shape[ax] - 2), axis=ax)
            J[i, j] = 0.5 * w[i] * (hi - lo)
    for i in range(3):
        J[i, i] += 1.0
    return (J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) - J[0, 1] * (J[1, 0] * J[2, 2] - J[1, 2] * J[2, 0])
            + J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))


# --------------------------------------------------------------------------------------
# inputs


def windowed_sinusoid(shape, spacing, amplitude=(3.0, 2.0, 4.0), seed=0):
    """A smooth field [3, Z, Y, X] (mm, fp32) that vanishes at the border: one sinusoid per component under sin^2 windows.
    An axis of length 1 or 2 has no window (the window would leave nothing)."""
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape).astype(np.float64)

    def win(i, n):
        return np.sin(np.pi * i / (n - 1)) ** 2 if n > 2 else np.ones_like(i)

    w = win(x, nx) * win(y, ny) * win(z, nz)
    out = []
    for d in range(3):
        ph = rng.uniform(0, 2 * np.pi, 3)
        fx, fy, fz = (1.0 + d % 2) * 2 * np.pi / max(nx, 2), 2 * np.pi / max(ny, 2), 2 * np.pi / max(nz, 2)
        out.append(amplitude[d] * w * np.sin(fx * x + ph[0]) * np.cos(fy * y + ph[1]) * np.cos(fz * z + ph[2]))
    return np.stack(out).astype(np.float32)


def geometries():
    """name -> (spacing, origin, direction 3 x 3)"""
    a = np.radians(20.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return {"identity": ((0.9, 0.9, 2.5), (0.0, 0.0, 0.0), np.eye(3)),
            "origin": ((1.0, 1.2, 2.5), (-40.5, 12.25, 100.0), np.eye(3)),
            "flip": ((0.9, 0.9, 2.5), (3.0, -2.0, 1.0), np.diag([-1.0, -1.0, 1.0])),
            "rot20": ((0.9, 1.1, 2.5), (5.0, 6.0, -7.0), rz)}


# --------------------------------------------------------------------------------------
# the fp32 error bound of the inversion kernel (derived in tests/test_field_inverse.py's docstring)

EPS32 = 2.0 ** -24


def lipschitz_scaled(u, spacing):
    """L with |u_lin(c + d) / spacing - u_lin(c) / spacing|_2 <= L |d|_2: inside a cell the interpolant's derivative along index
    axis a is a convex combination of the cell's four edge differences along a, so column a of its Jacobian is no longer than
    the longest scaled neighbour difference along a, and the Jacobian's 2-norm is at most the Frobenius norm of those three
    lengths."""
    u = np.asarray(u, dtype=np.float64) / np.asarray(spacing, dtype=np.float64).reshape(3, 1, 1, 1)
    tot = 0.0
    for ax in (1, 2, 3):
        if u.shape[ax] > 1:
            tot += (np.diff(u, axis=ax) ** 2).sum(0).max()
    return float(np.sqrt(tot))


def inversion_bound(u, spacing, direction, history, iterations):
    """-> dict(E: bound on max_x |(v_kernel - v_ref) / spacing|_2 after `iterations` iterations, e_r: per-iteration bound on
    the residual's error (and so on M and the mean), dc: per-iteration bound on a warped point's index error)."""
    sp = np.asarray(spacing, dtype=np.float64)
    D = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    sigma = float(np.linalg.norm(np.diag(1.0 / sp) @ D.T @ np.diag(sp), 2))
    L = lipschitz_scaled(u, spacing)
    Us = float(np.sqrt(sum((np.abs(np.asarray(u[d], dtype=np.float64)).max() / sp[d]) ** 2 for d in range(3))))
    E, e_r, dc = 0.0, [], []
    for k in range(1, iterations + 1):
        h = history[min(k, len(history)) - 1]
        W, Vs, M = 1.01 * h["index_displacement"] + 1.0, 1.01 * h["v_norm"] + 1.0, 1.01 * h["M"] + 1.0
        eps = 0.75 if k == 1 else 0.5
        pos = np.sqrt(3.0) * (6.0 * EPS32 * W + EPS32)
        d_r = L * pos + 17.0 * EPS32 * Us + EPS32 * Vs
        d_u = EPS32 * (12.0 * eps * M + 5.0 * M + 2.0 * Vs)
        dc.append(sigma * E + pos)
        er = (1.0 + L * sigma) * E + d_r
        e_r.append(er + 6.0 * EPS32 * M)
        E = (1.0 + eps * L * sigma) * E + eps * d_r + eps * eps * e_r[-1] + d_u
    return {"E": E, "e_r": e_r, "dc": dc, "L": L, "sigma": sigma}
