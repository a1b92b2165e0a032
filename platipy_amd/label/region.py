"""Region primitives on the GPU (csrc/pp_region.h): the SimpleITK calls the bronchus pipeline makes in host loops --
sitk.ConnectedComponent, sitk.LabelShapeStatisticsImageFilter, sitk.ConnectedThreshold and sitk.Median on a mask
(platipy/imaging/utils/lung.py:41-56, projects/bronchus/bronchus.py:194-196, 214-229, 259-262, 331-339).  Parity with
SimpleITK itself is UNPINNED: it is not installed where this is tested; the tests hold these to a numpy / scipy
restatement of the documented behaviour."""
import math

import numpy as np
import torch

from .. import runtime
from ..image import as_image
from .utils import _radius3, _u8


def connected_component(mask, fully_connected=False):
    """sitk.ConnectedComponent(mask, fullyConnected) -> (int32 label Image, count): 0 on the background, the components
    1 ... count in raster order of their first voxel.  Face connectivity by default (pp_connected_components_u8); with
    fully_connected voxels that touch by an edge or a corner are joined too (pp_connected_components_conn_u8)."""
    mask = as_image(mask)
    src = _u8(mask)
    labels = torch.empty(src.shape, dtype=torch.int32, device=src.device)
    ctx = runtime.context(mask.device)
    if fully_connected:
        count = ctx.connected_components_conn(src, mask.GetSize(), labels, fully_connected=True)
    else:
        count = ctx.connected_components(src, mask.GetSize(), labels)
    return mask.like(labels), count


def slice_convex_hull(mask):
    """skimage.morphology.convex_hull_image of every z-slice of a binary mask -> uint8 Image on the mask's grid: 1 where the
    pixel centre lies in the closed convex hull of the slice's pixel diamonds (pp_slice_convex_hull_u8, exact integers)."""
    mask = as_image(mask)
    src = _u8(mask)
    out = torch.empty_like(src)
    runtime.context(mask.device).slice_convex_hull(src, mask.GetSize(), out)
    return mask.like(out)


def label_moments(label_image, nlabels):
    """int64 numpy array [nlabels, 10] = {count, sum x, y, z, xx, yy, zz, xy, xz, yz} over the voxel indices of labels
    1 ... nlabels (pp_label_moments_i32; one pass, one read-back)."""
    label_image = as_image(label_image)
    t = label_image.tensor
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    t = t.contiguous()
    nlabels = int(nlabels)
    if nlabels <= 0:
        return np.zeros((0, 10), dtype=np.int64)
    out = torch.empty((nlabels, 10), dtype=torch.int64, device=t.device)
    runtime.context(label_image.device).label_moments(t, label_image.GetSize(), nlabels, out)
    return out.cpu().numpy()


def physical_point_to_index(image, point):
    """itk::ImageBase::TransformPhysicalPointToIndex: (direction diag(spacing))^-1 (point - origin), every component rounded
    half up [ITK-upstream Math::RoundHalfIntegerUp, unverified here]."""
    d = np.asarray(image.GetDirection(), dtype=np.float64).reshape(3, 3)
    m = np.linalg.inv(d @ np.diag(np.asarray(image.GetSpacing(), dtype=np.float64)))
    c = m @ (np.asarray(point, dtype=np.float64) - np.asarray(image.GetOrigin(), dtype=np.float64))
    return [int(math.floor(v + 0.5)) for v in c]


def shape_statistics_from_moments(moments, spacing, origin, direction):
    """The attributes of sitk.LabelShapeStatisticsImageFilter that follow from the ten integer sums of one label ->
    {label: dict}.  Recalled from ITK upstream (itk::ShapeLabelMapFilter) and UNVERIFIED here: the moment matrix is the
    covariance of the voxel centres in physical space plus spacing_i^2 / 12 on the diagonal (a voxel is a box, not a point),
    rotated by the direction cosines; principal moments are its eigenvalues in ascending order, elongation =
    sqrt(l2 / l1), flatness = sqrt(l1 / l0), a ratio being 0 when its denominator is 0.  The covariance is formed from the
    int64 sums in exact Python integer arithmetic, N sum(ab) - sum(a) sum(b), and only then converted to float.  `roundness`
    and `perimeter` need ITK's intercept-based perimeter estimator, which is not built: the keys are present, the values
    None.  A label without voxels has count 0 and None for everything that divides by it."""
    sp = np.asarray(spacing, dtype=np.float64)
    org = np.asarray(origin, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    voxel = float(sp[0] * sp[1] * sp[2])
    pairs = {(0, 0): 4, (1, 1): 5, (2, 2): 6, (0, 1): 7, (0, 2): 8, (1, 2): 9}
    out = {}
    for k, row in enumerate(np.asarray(moments)):
        m = [int(v) for v in row]
        n = m[0]
        st = {"label": k + 1, "count": n, "physical_size": n * voxel, "centroid": None, "principal_moments": None, "elongation": None,
              "flatness": None, "roundness": None, "perimeter": None}
        out[k + 1] = st
        if n == 0:
            continue
        mean = np.array([m[1] / n, m[2] / n, m[3] / n], dtype=np.float64)
        st["centroid"] = tuple(float(v) for v in org + d @ (sp * mean))
        cov = np.zeros((3, 3), dtype=np.float64)
        for (i, j), s in pairs.items():
            cov[i, j] = cov[j, i] = (n * m[s] - m[1 + i] * m[1 + j]) / (n * n)      # exact integers, one rounding
        cov = cov * np.outer(sp, sp) + np.diag(sp * sp / 12.0)
        lam = np.linalg.eigvalsh(d @ cov @ d.T)
        st["principal_moments"] = tuple(float(v) for v in lam)
        st["elongation"] = float(np.sqrt(lam[2] / lam[1])) if lam[1] != 0 else 0.0
        st["flatness"] = float(np.sqrt(lam[1] / lam[0])) if lam[0] != 0 else 0.0
    return out


def principal_axes_from_moments(moments, spacing, direction=(1, 0, 0, 0, 1, 0, 0, 0, 1)):
    """(principal moments, principal axes) of ONE label from its ten integer sums (a row of label_moments): what
    sitk.LabelShapeStatisticsImageFilter's GetPrincipalMoments / GetPrincipalAxes report.  The matrix is the one of
    shape_statistics_from_moments -- the covariance of the voxel centres in physical space plus spacing_i^2 / 12 on the
    diagonal, rotated by the direction cosines, formed from the int64 sums in exact integer arithmetic --, decomposed with
    np.linalg.eigh: moments ascending, axes a 3 x 3 array whose ROW k is the unit eigenvector of moment k.  That ITK orders
    the rows like this (ascending moments, so row 0 is the SHORT axis) is recalled from upstream and UNVERIFIED here, and so
    is the sign of each row: ITK only fixes the sign of the last row so that the matrix is a proper rotation, an
    eigenvector's own sign is the eigen-solver's.  A label without voxels raises ValueError."""
    m = [int(v) for v in np.asarray(moments).reshape(-1)]
    if len(m) != 10:
        raise ValueError("principal_axes_from_moments: ten sums {count, x, y, z, xx, yy, zz, xy, xz, yz} expected")
    n = m[0]
    if n == 0:
        raise ValueError("principal_axes_from_moments: the label has no voxels")
    sp = np.asarray(spacing, dtype=np.float64)
    d = np.asarray(direction, dtype=np.float64).reshape(3, 3)
    pairs = {(0, 0): 4, (1, 1): 5, (2, 2): 6, (0, 1): 7, (0, 2): 8, (1, 2): 9}
    cov = np.zeros((3, 3), dtype=np.float64)
    for (i, j), s in pairs.items():
        cov[i, j] = cov[j, i] = (n * m[s] - m[1 + i] * m[1 + j]) / (n * n)      # exact integers, one rounding
    cov = cov * np.outer(sp, sp) + np.diag(sp * sp / 12.0)
    lam, vec = np.linalg.eigh(d @ cov @ d.T)
    return lam, np.ascontiguousarray(vec.T)


def label_shape_statistics(label_image, nlabels=None):
    """sitk.LabelShapeStatisticsImageFilter().Execute(label_image) -> {label: {"count", "physical_size", "centroid" (physical,
    x y z), "principal_moments" (ascending), "elongation", "flatness", "roundness": None, "perimeter": None}} for the labels
    1 ... nlabels (default: the largest label present).  See shape_statistics_from_moments for what is recalled from ITK and
    not verified, and for the two attributes that are out of scope."""
    label_image = as_image(label_image)
    if nlabels is None:
        nlabels = int(label_image.tensor.max()) if label_image.tensor.numel() else 0
    return shape_statistics_from_moments(label_moments(label_image, max(int(nlabels), 0)), label_image.GetSpacing(), label_image.GetOrigin(),
                                         label_image.GetDirection())


def connected_threshold(image, seed_list, lower, upper, return_count=False):
    """sitk.ConnectedThreshold(image, seedList=seed_list, lower=lower, upper=upper): the uint8 mask of the voxels
    face-connected to a seed (index x, y, z) through values in [lower, upper], both ends included; the image is compared as
    float32 (pp_connected_threshold_f32).  A seed outside the image raises IndexError."""
    image = as_image(image)
    t = image.tensor
    src = (t if t.dtype == torch.float32 else t.to(torch.float32)).contiguous()
    out = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    seeds = np.asarray(seed_list, dtype=np.int64).reshape(-1, 3)
    voxels = runtime.context(image.device).connected_threshold(src, image.GetSize(), lower, upper, seeds, out)
    res = image.like(out)
    return (res, voxels) if return_count else res


def binary_median(mask, radius=1):
    """sitk.Median(mask, radius) of a binary mask: 1 where more than half of the window is foreground, the window clamped at
    the image edge; radius in voxels (x, y, z), at most 2 per axis (pp_binary_median_u8)."""
    mask = as_image(mask)
    radius = _radius3(mask, radius)
    src = _u8(mask)
    out = torch.empty_like(src)
    runtime.context(mask.device).binary_median(src, mask.GetSize(), radius, out)
    return mask.like(out)
