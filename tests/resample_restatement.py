"""Plain fp64 numpy restatement of the resampling family (platipy_amd/csrc/pp_resample.hip), written from the definitions
of the ITK filters it stands in for -- not from the kernels, and independent of oracle/.

Conventions: a grid is a `Grid(size, spacing, origin, direction)` with size, spacing and origin in (x, y, z) order and a
3 x 3 direction matrix; volumes are [Z][Y][X] arrays, vector fields [3][Z][Y][X] with component 0 along physical x.

  index -> physical on the output grid      p = origin + Dir diag(spacing) idx
  linear transform (optional)               q = A p + t
  displacement field (optional)             q += D(idx), the physical displacement stored at the output voxel
  physical -> continuous index, input grid  c = diag(1 / spacing) inv(Dir) (q - origin)

A sample is inside the input buffer iff -0.5 <= c < n - 0.5 on every axis (itk::ImageFunction::IsInsideBuffer).  Nearest
neighbour picks floor(c + 0.5); linear is the trilinear interpolant at clip(c, 0, n - 1) (ITK's clamped interpolator:
the outer half voxel repeats the border value); a uint8 output is trunc(clip(v, 0, 255)).
"""
import numpy as np
from scipy import ndimage


class Grid:
    def __init__(self, size, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=None):
        self.size = tuple(int(s) for s in size)                      # (nx, ny, nz)
        self.spacing = np.asarray(spacing, dtype=np.float64)
        self.origin = np.asarray(origin, dtype=np.float64)
        self.direction = np.eye(3) if direction is None else np.asarray(direction, dtype=np.float64).reshape(3, 3)

    @property
    def shape(self):                                                 # [Z][Y][X]
        return self.size[::-1]

    def indices(self):
        """[Z][Y][X][3] integer indices (x, y, z) of every voxel, as fp64."""
        z, y, x = np.indices(self.shape)
        return np.stack([x, y, z], axis=-1).astype(np.float64)

    def index_to_physical(self, idx):
        return self.origin + idx @ (self.direction @ np.diag(self.spacing)).T

    def physical_to_index(self, p):
        return (p - self.origin) @ (np.diag(1.0 / self.spacing) @ np.linalg.inv(self.direction)).T


def continuous_index(gin, gout, A=None, t=None, field=None):
    """[Z][Y][X][3] continuous index (x, y, z) on `gin` of every voxel of `gout`."""
    q = gout.index_to_physical(gout.indices())
    if A is not None:
        q = q @ np.asarray(A, dtype=np.float64).reshape(3, 3).T + (0.0 if t is None else np.asarray(t, dtype=np.float64))
    if field is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            q = q + np.moveaxis(np.asarray(field, dtype=np.float64), 0, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        return gin.physical_to_index(q)


def inside_buffer(c, size):
    n = np.asarray(size, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.all((c >= -0.5) & (c < n - 0.5), axis=-1)         # NaN compares false: outside


def _corner_axes(c, size):
    """Per axis: lower index, upper index (repeated on the last voxel) and the weight of the upper one, at clip(c, 0, n - 1)."""
    out = []
    for a in range(3):
        n = size[a]
        cc = np.clip(np.where(np.isfinite(c[..., a]), c[..., a], 0.0), 0.0, n - 1.0)
        i0 = np.minimum(np.floor(cc).astype(np.int64), n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        out.append((i0, i1, cc - i0))
    return out


def linear_sample(vol, c):
    """Trilinear value of the [Z][Y][X] volume at clip(c, 0, n - 1) plus, over the eight corners, max |value| (M) and
    max - min (R).  No inside test here."""
    v = np.asarray(vol, dtype=np.float64)
    size = v.shape[::-1]
    (x0, x1, wx), (y0, y1, wy), (z0, z1, wz) = _corner_axes(c, size)
    corners = np.stack([v[zz, yy, xx] for zz in (z0, z1) for yy in (y0, y1) for xx in (x0, x1)])   # x fastest
    # a + (b - a) w along x, then y, then z, in fp64: exact where the corners of a lerp agree (a weighted sum of eight equal
    # corners is not -- its weights need not add up to exactly 1 -- and a uint8 output truncates)
    vx = [corners[k] + (corners[k + 1] - corners[k]) * wx for k in (0, 2, 4, 6)]
    vy = [vx[k] + (vx[k + 1] - vx[k]) * wy for k in (0, 2)]
    val = vy[0] + (vy[1] - vy[0]) * wz
    return val, np.abs(corners).max(0), corners.max(0) - corners.min(0)


def nearest_sample(vol, c, size):
    """Voxel floor(c + 0.5), indices clipped into the buffer (the caller applies the inside test)."""
    idx = []
    for a in range(3):
        ca = np.where(np.isfinite(c[..., a]), c[..., a], 0.0)
        idx.append(np.clip(np.floor(ca + 0.5), 0, size[a] - 1).astype(np.int64))
    return np.asarray(vol)[idx[2], idx[1], idx[0]]


def cast_u8(v):
    return np.trunc(np.clip(v, 0.0, 255.0)).astype(np.uint8)


def resample(vol, gin, gout, A=None, t=None, field=None, interp="linear", default=0.0, u8=False):
    """-> dict(out, inside, c, M, R, ref): `out` in the output type, `ref` the fp64 value before any cast (linear only)."""
    c = continuous_index(gin, gout, A, t, field)
    ins = inside_buffer(c, gin.size)
    res = {"c": c, "inside": ins}
    dflt = float(np.clip(default, 0.0, 255.0)) if u8 else float(default)
    if interp == "nearest":
        picked = nearest_sample(vol, c, gin.size)
        dv = np.uint8(dflt) if u8 else np.float32(dflt)
        res["out"] = np.where(ins, picked, dv).astype(np.uint8 if u8 else np.float32)
        return res
    val, M, R = linear_sample(vol, c)
    res.update(M=M, R=R, ref=val)
    if u8:
        res["out"] = np.where(ins, cast_u8(val), np.uint8(dflt)).astype(np.uint8)
    else:
        res["out"] = np.where(ins, val, dflt)                      # fp64: the test applies the bound
    return res


def resample_field(f, gin, gout, through=None):
    """The vector field `f` on `gin` sampled per component (linear, 0 outside) at the voxels of `gout` -- moved by the
    field `through` on `gout` when given.  -> dict(out [3][Z][Y][X] fp64, inside, c, M, R) with M, R over the components."""
    c = continuous_index(gin, gout, field=through)
    ins = inside_buffer(c, gin.size)
    parts = [linear_sample(f[k], c) for k in range(3)]
    out = np.stack([np.where(ins, p[0], 0.0) for p in parts])
    return {"out": out, "inside": ins, "c": c, "M": np.stack([p[1] for p in parts]), "R": np.stack([p[2] for p in parts])}


def compose(total, it, grid):
    """total + iter(x + total(x)), the sampled term 0 outside.  -> dict(out, sample, inside, c, M, R)."""
    r = resample_field(it, grid, grid, through=total)
    with np.errstate(invalid="ignore", over="ignore"):
        r["sample"] = r["out"]
        r["out"] = np.asarray(total, dtype=np.float64) + r["sample"]
    return r


def affine_displacement(grid, A, t, add=None):
    """(A - I) p + t (+ add) at every voxel of `grid` (sitk.TransformToDisplacementField of a linear transform).
    -> (field [3][Z][Y][X] fp64 WITHOUT `add`, field with `add`)."""
    p = grid.index_to_physical(grid.indices())
    d = p @ (np.asarray(A, dtype=np.float64).reshape(3, 3) - np.eye(3)).T + np.asarray(t, dtype=np.float64)
    d = np.moveaxis(d, -1, 0)
    return d, (d if add is None else d + np.asarray(add, dtype=np.float64))


# --------------------------------------------------------------------------------------
# cubic B-spline: prefilter and evaluation, apart

def bspline_prefilter(vol):
    return ndimage.spline_filter(np.asarray(vol, dtype=np.float64), order=3, mode="mirror", output=np.float64)


def bspline_prefilter_fp32_storage(vol):
    """The same filter with the volume rounded to fp32 after each axis pass (x, then y, then z): how far fp32 storage
    alone moves the result -- the yardstick of the prefilter test's tolerance."""
    v = np.asarray(vol, dtype=np.float64)
    for axis in (2, 1, 0):
        v = ndimage.spline_filter1d(v, order=3, axis=axis, mode="mirror", output=np.float64).astype(np.float32).astype(np.float64)
    return v


def bspline_evaluate(coef, c):
    """Cubic B-spline with mirror boundaries (period 2 n - 2) on the coefficient volume [Z][Y][X] at the continuous
    indices c[..., (x, y, z)].  An axis of length 1 is constant along itself (every mirrored index is 0 and the four
    weights sum to 1), so it is dropped by hand instead of being handed to scipy."""
    co = np.asarray(coef, dtype=np.float64)
    keep = [ax for ax in range(3) if co.shape[ax] > 1]               # array axes (z, y, x)
    flat = c.reshape(-1, 3)
    if not keep:
        return np.full(c.shape[:-1], co.reshape(-1)[0])
    coords = np.stack([flat[:, 2 - ax] for ax in keep])
    vals = ndimage.map_coordinates(co.reshape([co.shape[ax] for ax in keep]), coords, order=3, mode="mirror", prefilter=False)
    return vals.reshape(c.shape[:-1])
