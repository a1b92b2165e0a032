"""The volume computations of platipy/imaging/visualisation/utils.py: project_onto_arbitrary_plane (:305-368) and
generate_comparison_colormix (:260-302).  The plotting half of that package (ImageVisualiser, matplotlib) stays out of scope.

project_onto_arbitrary_plane rotates a volume about its centre, resamples it onto its own grid and reduces it along an axis.
ImageVisualiser(projection=...) calls it for the image and, with "max", for every contour and scalar overlay; a rotating
maximum-intensity projection is one call per angle.  Here every angle, the image and its labels go through ONE launch of
pp_project_set (csrc/pp_project.h): a thread walks a ray of the rotated grid and reduces the samples as it takes them, so the
rotated volume is never written.  Every sample is, bit for bit, the voxel apply_transform / rotate_image would have produced,
and every other path below reduces through the same kernel, so a result never depends on which path ran.

Quirks and deviations (P1-P7):
  P1  Image is 3-D only: the result is a ONE-SLICE Image (size 1 on the projection axis), not the 2-D slice the reference
      cuts out of it.  result.tensor.squeeze(...) / result.numpy()[...] is the reference's array.
  P2  The slice's geometry is what itk::ProjectionImageFilter gives an output of the input's dimension, AS RECALLED
      (unpinned): spacing on the projection axis = spacing * size, origin moved by (size - 1) * spacing / 2 along that
      axis's direction column; everything else kept.
  P3  Integer images other than uint8 are sampled and reduced in fp32 and cast ONCE, after the reduction (cast_tensor:
      truncation); the reference resamples into the integer type first (sitk.Resample(..., image.GetPixelID())) and lets the
      projection filter choose its output type.  Which pixel type SimpleITK gives MeanProjection / StandardDeviationProjection
      of an integer image is unpinned; here the result has the input's dtype.
  P4  A uint8 image is resampled as uint8 (clamp, then truncate: pp_resample_u8), as the reference does; "max" goes through
      the kernel's label path, the other kinds rotate first and reduce the uint8 volume through the kernel.
  P5  The default value takes part in the reduction (the reference's behaviour: a mean over a ray that leaves the volume is
      pulled towards default_value).
  P6  project_set's label_interpolation defaults to sitkLinear because the reference's resample_interpolation does, and the
      visualiser passes its contours through it unchanged.  Linear interpolation of a 0 / 1 mask followed by the uint8
      cast's truncation keeps a sample only where every corner it weighs is foreground: a rotated mask loses a voxel on every
      side, and a thin or small structure (a contour, a 2 x 2 x 2 cube) is erased almost entirely.  That is the reference's
      behaviour; sitkNearestNeighbor is the useful choice.
  P7  generate_comparison_colormix: with arr_slice=None a 2-D input is indexed with None, which adds a leading axis (the
      reference's `__getitem__(None)`); a list of two inputs of different kinds raises ValueError where the reference fails
      with an unbound local.  Hue, saturation and value are computed in float64.
"""
import numpy as np
import torch

from .. import _lib, runtime
from ..image import Image, as_image, cast_tensor
from ..registration.utils import _check_interp, _split_transform, resample_image
from ..transform import VersorRigid3DTransform, sitkLinear

_UNIT_VIEW = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])


def _rotation_about_centre(image, rotation_axis, rotation_angle):
    """The reference's transform (:339-347): a VersorRigid3DTransform about the physical point of continuous index
    (size - 1) / 2."""
    size = np.asarray(image.GetSize(), dtype=np.float64)
    direction = np.asarray(image.GetDirection(), dtype=np.float64).reshape(3, 3)
    centre = np.asarray(image.GetOrigin(), dtype=np.float64) + direction @ (np.asarray(image.GetSpacing(), dtype=np.float64) * (size - 1.0) / 2.0)
    tfm = VersorRigid3DTransform()
    tfm.SetCenter(centre)
    tfm.SetRotation(rotation_axis, rotation_angle)
    return tfm


def _views(image, rotation_axis, rotation_angles):
    """[A, 12] doubles for pp_project_set and the transforms they came from, split as apply_transform splits them."""
    tfms = [_rotation_about_centre(image, rotation_axis, a) for a in rotation_angles]
    rows = []
    for tfm in tfms:
        A, t, _ = _split_transform(tfm, image)
        rows.append(np.concatenate([np.asarray(A, dtype=np.float64).ravel(), np.asarray(t, dtype=np.float64).ravel()]))
    return np.stack(rows), tfms


def _plane_shape(shape, axis):
    nz, ny, nx = shape
    return {0: (nz, ny), 1: (nz, nx), 2: (ny, nx)}[axis]


def _check_axis(projection_axis):
    if projection_axis not in (0, 1, 2):
        raise KeyError(projection_axis)      # (the reference's image_slice[projection_axis])
    return int(projection_axis)


def _reduce_volume(tensor, kind, axis):
    """The kernel's reduction of a volume that is already rotated: an identity view of a unit grid, nearest neighbour -- each
    sample is the voxel itself -- so the fallback paths add and select in the order the fused path does."""
    src = (tensor if tensor.dtype == torch.float32 else tensor.float()).contiguous()
    nz, ny, nx = src.shape
    out = torch.empty((1,) + _plane_shape(src.shape, axis), dtype=torch.float32, device=src.device)
    runtime.context(src.device).project_set(_lib.make_geom((nx, ny, nz)), axis, _UNIT_VIEW, image=src, image_out=out, kind=kind,
                                            interp=_lib.INTERP_NEAREST, default_value=0.0)
    return out[0]


def _member_image(image, tfm, kind, axis, default_value, interpolator):
    """One image, one view, member by member: resample_image (what rotate_image runs), then the reduction."""
    rotated = resample_image(image, image, tfm, interpolator, default_value).tensor
    if rotated.dtype == torch.uint8 and kind == _lib.PROJECT_MAX:
        return rotated.amax(dim=2 - axis).float()
    return _reduce_volume(rotated, kind, axis)


def _member_label(label, tfm, axis, interpolator):
    rotated = resample_image(label, label, tfm, interpolator, 0).tensor
    return cast_tensor(rotated.amax(dim=2 - axis), torch.uint8)


def project_set(image, labels, rotation_angles, projection_name="max", projection_axis=0, rotation_axis=(1, 0, 0), default_value=-1000,
                resample_interpolation=sitkLinear, label_interpolation=sitkLinear):
    """project_onto_arbitrary_plane for every angle of `rotation_angles` (radians), for `image` with `projection_name` and
    for every label of `labels` with "max" (the visualiser's contour path) -> (fp32 tensor [A, rows, cols] or None,
    [uint8 tensor [A, rows, cols], ...]); rows x cols are the two remaining axes in array order ([nz, ny], [nz, nx], [ny, nx]
    for axis 0, 1, 2).  `image` may be None and `labels` empty; without angles the stacks are empty ([0, rows, cols]).

    When the members share one grid, the labels are uint8, the image is not, and the interpolators are nearest or linear, all
    angles, the image and all labels go through ONE pp_project_set call (more than 16 labels: in groups of 16).  Anything
    else -- sitkBSpline, members on different grids, a uint8 image, labels of another type -- goes member by member and angle
    by angle through resample_image and the same reduction, so a result never depends on which path ran.

    label_interpolation defaults to sitkLinear as the reference's resample_interpolation does; linear interpolation and the
    uint8 cast's truncation take a voxel off every side of a rotated 0 / 1 mask and erase thin structures almost entirely
    (P6).  sitkNearestNeighbor is the useful choice for contours."""
    kind = _lib.PROJECT_KINDS[projection_name]
    axis = _check_axis(projection_axis)
    image = as_image(image) if image is not None else None
    labels = [as_image(lab) for lab in labels]
    interp, linterp = _check_interp(resample_interpolation), _check_interp(label_interpolation)
    angles = [float(a) for a in rotation_angles]
    members = ([image] if image is not None else []) + labels
    if not members:
        return None, []
    if not angles:      # no view: empty stacks, still one per member
        def none_of(member, dtype):
            return torch.empty((0,) + _plane_shape(member.shape, axis), dtype=dtype, device=member.device)
        return (None if image is None else none_of(image, torch.float32)), [none_of(lab, torch.uint8) for lab in labels]
    first = members[0]
    fused = (all(m.same_grid(first) and m.device == first.device for m in members)
             and all(lab.tensor.dtype == torch.uint8 for lab in labels)
             and (image is None or (image.tensor.dtype != torch.uint8 and interp != _lib.INTERP_BSPLINE))
             and (not labels or linterp != _lib.INTERP_BSPLINE))
    if fused:
        try:
            return _project_fused(image, labels, angles, kind, axis, rotation_axis, default_value, interp, linterp)
        except _lib.PlatipyAmdError as e:
            if getattr(e, "code", None) != _lib.ERR_UNSUPPORTED:
                raise
    image_out = None
    if image is not None:
        tfms = [_rotation_about_centre(image, rotation_axis, a) for a in angles]
        image_out = torch.stack([_member_image(image, tfm, kind, axis, default_value, resample_interpolation) for tfm in tfms])
    labels_out = []
    for lab in labels:
        tfms = [_rotation_about_centre(lab, rotation_axis, a) for a in angles]
        labels_out.append(torch.stack([_member_label(lab, tfm, axis, label_interpolation) for tfm in tfms]))
    return image_out, labels_out


def _project_fused(image, labels, angles, kind, axis, rotation_axis, default_value, interp, linterp):
    first = image if image is not None else labels[0]
    ctx = runtime.context(first.device)
    views, _ = _views(first, rotation_axis, angles)
    shape = (len(angles),) + _plane_shape(first.shape, axis)
    src = out = None
    if image is not None:
        src = (image.tensor if image.tensor.dtype == torch.float32 else image.tensor.float()).contiguous()
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    outs = [torch.empty(shape, dtype=torch.uint8, device=first.device) for _ in labels]
    step = _lib.PROJECT_MAX_LABELS
    for k in range(0, max(len(labels), 1), step):
        with_image = image is not None and k == 0
        ctx.project_set(first.geom(), axis, views, image=src if with_image else None, image_out=out if with_image else None, kind=kind,
                        interp=interp, default_value=float(default_value), labels=[lab.tensor for lab in labels[k:k + step]],
                        labels_out=outs[k:k + step], label_interp=linterp)
    return out, outs


def _one_slice(image, plane, axis):
    """P1, P2: the plane as a one-slice Image of `image`'s dtype."""
    size, spacing = image.GetSize(), list(image.GetSpacing())
    direction = np.asarray(image.GetDirection(), dtype=np.float64).reshape(3, 3)
    origin = np.asarray(image.GetOrigin(), dtype=np.float64) + direction[:, axis] * ((size[axis] - 1) * spacing[axis] / 2.0)
    spacing[axis] = spacing[axis] * size[axis]
    return Image(cast_tensor(plane.unsqueeze(2 - axis), image.tensor.dtype), spacing, origin, image.GetDirection(), False)


def project_onto_arbitrary_plane(image, projection_name="mean", projection_axis=0, rotation_axis=[1, 0, 0], rotation_angle=0,
                                 default_value=-1000, resample_interpolation=sitkLinear):
    """Rotate `image` about its centre by `rotation_angle` radians about `rotation_axis`, resample it onto its own grid and
    reduce it along `projection_axis` (0 = x, 1 = y, 2 = z) with "sum", "mean", "median", "std", "min" or "max" (reference
    visualisation/utils.py:305-368; an unknown name raises KeyError as there).  Returns a one-slice Image of the input's
    dtype (P1-P3).  Samples outside the volume are `default_value` and take part in the reduction (P5)."""
    kind = _lib.PROJECT_KINDS[projection_name]
    axis = _check_axis(projection_axis)
    image = as_image(image)
    _check_interp(resample_interpolation)
    if image.tensor.dtype == torch.uint8 and kind == _lib.PROJECT_MAX:
        # P4: the kernel's label path samples and casts as pp_resample_u8 does (default_value clamped into 0 ... 255 there; 0 here
        # unless the caller's default is one, which only the member path can honour)
        if float(default_value) <= 0.0:
            _, planes = project_set(None, [image], [rotation_angle], "max", axis, rotation_axis, 0, sitkLinear, resample_interpolation)
            return _one_slice(image, planes[0][0], axis)
        tfm = _rotation_about_centre(image, rotation_axis, rotation_angle)
        return _one_slice(image, _member_image(image, tfm, kind, axis, default_value, resample_interpolation), axis)
    plane, _ = project_set(image, [], [rotation_angle], projection_name, axis, rotation_axis, default_value, resample_interpolation)
    return _one_slice(image, plane[0], axis)


def _hsv_to_rgb(h, s, v):
    """The standard sextant formula (skimage.color.hsv2rgb's), elementwise."""
    h6 = h * 6.0
    hi = torch.floor(h6)
    f = h6 - hi
    p = v * (1.0 - s)
    q = v * (1.0 - f * s)
    t = v * (1.0 - (1.0 - f) * s)
    sextant = hi.to(torch.int64) % 6
    r = torch.stack([v, q, p, p, t, v], dim=-1)
    g = torch.stack([t, v, v, q, p, p], dim=-1)
    b = torch.stack([p, p, t, v, v, q], dim=-1)
    idx = sextant.unsqueeze(-1)
    return torch.stack([torch.gather(c, -1, idx).squeeze(-1) for c in (r, g, b)], dim=-1)


def generate_comparison_colormix(image_list, arr_slice=None, window=(-250, 500), color_rotation=0.35):
    """Two images as one RGB image (reference visualisation/utils.py:260-302): each is windowed to [0, 1] over
    [window[0], window[0] + window[1]]; the hue is color_rotation where the first is brighter and 0.5 + color_rotation where
    it is not, the saturation their absolute difference, the value their mean; HSV -> RGB.  `image_list`: two Images (3-D, so
    `arr_slice` is required) or two tensors; the result is a float64 tensor [..., 3] on the inputs' device.  ValueError for
    anything but two inputs of one kind, and for 3-D inputs without `arr_slice`, as in the reference (P7)."""
    if len(image_list) != 2:
        raise ValueError("'image_list' must be a list of two Image or torch.Tensor.")
    if all(isinstance(im, Image) for im in image_list):
        if arr_slice is None:
            raise ValueError("Images cannot be 3D unless 'arr_slice' is specified.")
        arrays = [im.tensor[arr_slice] for im in image_list]
    elif all(isinstance(im, torch.Tensor) for im in image_list):
        if any(im.dim() >= 3 for im in image_list) and arr_slice is None:
            raise ValueError("Images cannot be 3D unless 'arr_slice' is specified.")
        arrays = [im[arr_slice] for im in image_list]
    else:
        raise ValueError("'image_list' must be a list of two Image or torch.Tensor.")
    lo, width = float(window[0]), float(window[1])
    a, b = [(torch.clamp(x.double(), lo, lo + width) - lo) / width for x in arrays]
    first_brighter = (a > b).double()
    hue = color_rotation * first_brighter + (0.5 + color_rotation) * (1.0 - first_brighter)
    return _hsv_to_rgb(hue, torch.abs(a - b), (a + b) / 2.0)
