"""Drop-in for platipy/imaging/utils/ventricle.py:75-684: the 17 segments of the left ventricle from the chamber labels
the cardiac pipeline returns.  The heart is turned so that its long axis (mitral valve -> apex) lies along z, the
myocardium is cut into apical, mid and basal thirds, every slice is divided into angular sectors about its own centre, and
the sectors are turned back into image space.

Everything volume-sized stays on the device: the five labels go through one pp_resample_set call per rotation, apex,
centres of mass and slice limits come from the per-slice moments kernel, the whole segment assignment -- the reference's
Python loop over slices with 4 or 6 `extract` calls each (:408-644; `extract` itself, :30-72, is subsumed by the kernel and
not exported) -- is ONE pp_polar_sectors_u8 call, and the way back -- 17 resamples there -- is ONE pp_resample_bits_u32 call.
Parity with SimpleITK is UNPINNED (it is not installed where this is tested; tests/ventricle_restatement.py restates the
reference's arithmetic in fp64 numpy / scipy), and so are ITK's ordering and sign of the principal axes
(label/region.py: principal_axes_from_moments).

The reference's quirks are kept:
  V1  the reference takes the FIRST row of GetPrincipalAxes -- with ascending moments the SHORT axis --, flips it by the sign
      of its third component and reverses it ([::-1]) before use;
  V2  the rotation angles are vector_angle(..., smallest=True): the direction of the axis is ignored;
  V3  integer (as_int) centres of mass for the slice origins and for the z of the mitral valve;
  V4  a negative angle gets 2 pi added ONCE, so an angle below -2 pi stays negative: its voxel belongs to no segment of
      the mid and basal thirds (apically, to the clockwise segment 14);
  V5  both ends of every sector are inclusive: a voxel on a boundary belongs to two segments;
  V6  the basal sectors start at a radius of 15 VOXELS, not mm;
  V7  a sector's area is its voxel count times the in-plane spacing product; below min_area_mm2 (default 50) it is dropped
      from its slice.  Segment 17 (the myocardium below the blood pool) is never put to that test;
  V8  (deviation) an apical or mid slice without myocardium makes the reference raise through int(NaN); here it is skipped,
      as the reference skips empty basal slices;
  V9  an LV or RV missing from a slice that theta_0 / theta_0_apical need raises ValueError naming the slice (the
      reference's int(NaN) / min() of nothing); a zero rotation axis -- the heart already aligned -- raises as rotate_image
      does."""
import numpy as np
import torch

from .. import _lib, runtime
from ..image import as_image
from ..label.region import label_moments, principal_axes_from_moments
from ..label.utils import binary_dilate, binary_erode, binary_morphological_closing, check_dilate_radius, get_com, slice_moments
from ..registration.utils import _split_transform, apply_transform_to_set
from ..transform import CompositeTransform, VersorRigid3DTransform, sitkNearestNeighbor
from .crop import crop_to_roi, label_to_roi, paste
from .geometry import vector_angle
from .valve import generate_valve_using_cylinder

PI = np.pi
# (label, clockwise, angle_min, angle_max) with the reference's own expressions for the angles (:436-476, :500-552, :579-644)
APICAL_RULES = [(13, False, 5 * PI / 4, 7 * PI / 4), (14, True, 1 * PI / 4, 7 * PI / 4), (15, False, 1 * PI / 4, 3 * PI / 4),
                (16, False, 3 * PI / 4, 5 * PI / 4)]
_SIXTHS = [(0, PI / 3), (1 * PI / 3, 2 * PI / 3), (2 * PI / 3, 3 * PI / 3), (3 * PI / 3, 4 * PI / 3), (4 * PI / 3, 5 * PI / 3), (5 * PI / 3, 2 * PI)]
MID_RULES = [(label, False, lo, hi) for label, (lo, hi) in zip((8, 9, 10, 11, 12, 7), _SIXTHS)]
BASAL_RULES = [(label, False, lo, hi) for label, (lo, hi) in zip((2, 3, 4, 5, 6, 1), _SIXTHS)]
BASAL_RADIUS_MIN = 15      # V6: voxels


def _binary(label):
    label = as_image(label)
    return label.like((label.tensor != 0).to(torch.uint8))


def _rotation(centre, axis, angle):
    t = VersorRigid3DTransform()
    t.SetCenter(centre)
    t.SetRotation(axis, angle)        # ValueError for a zero axis (V9)
    return t


def _slice_com_int(moments, z, what):
    """get_com(label[:, :, z]) of the reference: (y, x), each truncated (V3).  An empty slice raises (V9)."""
    if z < 0 or z >= moments.shape[0] or moments[z, 0] == 0:
        raise ValueError(f"generate_left_ventricle_segments: {what} is absent from slice {int(z)}")
    total = float(moments[z, 0])
    return [int(np.float64(float(moments[z, 1])) / total), int(np.float64(float(moments[z, 2])) / total)]


def generate_left_ventricle_segments(contours, label_left_ventricle="Ventricle_L", label_left_atrium="Atrium_L",
                                     label_right_ventricle="Ventricle_R", label_heart="Heart", myocardium_thickness_mm=10,
                                     hole_fill_mm=3, optimiser_tol_degrees=1, optimiser_max_iter=10, min_area_mm2=50, verbose=False,
                                     info=None):
    """{"Ventricle_L_Segment1" ... "Ventricle_L_Segment17": uint8 Image on the input grid} from the binary labels of the left
    ventricle, left atrium, right ventricle and whole heart in `contours` (ventricle.py:75-684).  `info`, when a dict,
    receives rotation_angles / rotation_centres / rotation_axes (one entry per rotation, the initial one first), inf_limit_lv,
    apical_extent, mid_extent, basal_extent, theta_0, theta_0_apical, slice_origins ({slice: (y, x)}) and counts (int64
    [slices][32], voxels per slice and segment before the area test).  The inputs are not modified."""
    def say(*a):
        if verbose:
            print(*a)

    who = "generate_left_ventricle_segments"
    say("Beginning LV segmentation algorithm.")
    names = [label_left_ventricle, label_left_atrium, label_right_ventricle, label_heart]
    template = as_image(contours[label_heart])
    work = [_binary(contours[s]) for s in names]
    LV, LA, RV, HEART, MV = range(5)
    erode_img = [int(myocardium_thickness_mm / i) for i in work[LV].GetSpacing()]
    hole_fill_img = [int(hole_fill_mm / i) for i in work[HEART].GetSpacing()]
    check_dilate_radius(erode_img, who + " (myocardium_thickness_mm)")      # (before any work is done)
    check_dilate_radius(hole_fill_img, who + " (hole_fill_mm)")
    work.append(generate_valve_using_cylinder(work[LA], work[LV], radius_mm=15, height_mm=10))

    # Module 1: crop, initial alignment to the cardiac axis
    cb_size, cb_index = label_to_roi(work[HEART], expansion_mm=(30, 30, 60))
    work = [crop_to_roi(w, cb_size, cb_index) for w in work]
    say("Module 1: Cropping and initial alignment.")
    label_orient = work[LV].like(work[LV].tensor | work[LA].tensor)
    _, axes = principal_axes_from_moments(label_moments(label_orient.like(label_orient.tensor.to(torch.int32)), 1)[0],
                                          label_orient.GetSpacing(), label_orient.GetDirection())
    cardiac_axis = axes[0]                                     # V1
    if cardiac_axis[2] < 0:
        cardiac_axis = -1 * cardiac_axis
    rotation_angle = vector_angle(cardiac_axis[::-1], (0, 0, 1))        # V2
    rotation_axis = np.cross(cardiac_axis[::-1], (0, 0, 1))
    rotation_centre = get_com(label_orient, real_coords=True)
    transforms, angles, centres, rot_axes = [], [], [], []

    def rotate(centre, axis, angle):
        say("    Rotation axis:   ", axis, "\n    Rotation angle:  ", angle, "\n    Rotation centre: ", centre)
        t = _rotation(centre, axis, angle)
        transforms.append(t)
        angles.append(float(angle))
        centres.append(tuple(float(v) for v in centre))
        rot_axes.append(tuple(float(v) for v in axis))
        return apply_transform_to_set(None, work, None, t, 0, sitkNearestNeighbor)[1]     # the five labels in one gather

    work = rotate(rotation_centre, rotation_axis, rotation_angle)

    # Module 2: refine the alignment to the mitral valve -> apex axis
    say("Module 2: LV orientation alignment.")
    tol = optimiser_tol_degrees * np.pi / 180
    n = 0
    while n < optimiser_max_iter and np.abs(rotation_angle) > tol:
        n += 1
        m = slice_moments([work[LV]], "z")[0]
        filled = np.nonzero(m[:, 3])[0]
        if filled.size == 0:
            raise ValueError(f"{who}: the left ventricle left the cropped volume during alignment")
        apex_z = int(filled[0])
        apex = np.array([float(m[apex_z, 2]) / float(m[apex_z, 3]), float(m[apex_z, 1]) / float(m[apex_z, 3]), float(apex_z)])
        mv_com = np.array(get_com(work[MV], real_coords=True))
        lv = work[LV]
        d = np.asarray(lv.GetDirection(), dtype=np.float64).reshape(3, 3)
        apex_img = np.asarray(lv.GetOrigin(), dtype=np.float64) + d @ (np.asarray(lv.GetSpacing(), dtype=np.float64) * apex)
        lv_axis = apex_img - mv_com
        rotation_axis = np.cross(lv_axis, (0, 0, 1))
        rotation_angle = vector_angle(lv_axis, (0, 0, 1))
        say("    N:               ", n, "\n    LV apex:         ", apex_img, "\n    MV COM:          ", mv_com)
        work = rotate(0.5 * (mv_com + apex_img), rotation_axis, rotation_angle)

    # Module 3: the myocardium and the limits of its thirds
    say("Module 3: Myocardium generation.")
    lv_inner = binary_erode(work[LV], erode_img)
    myo_mask = binary_dilate(lv_inner, erode_img)
    lv_myo = work[LV].like((work[LV].tensor - lv_inner.tensor) * (myo_mask.tensor != 0).to(torch.uint8))
    mom = slice_moments([work[LV], work[RV], lv_myo, lv_inner], "z")
    m_lv, m_rv, m_myo, m_inner = mom[0], mom[1], mom[2], mom[3]
    filled = np.nonzero(m_inner[:, 3])[0]
    if filled.size == 0:
        raise ValueError(f"{who}: nothing of the left ventricle is left after eroding by {tuple(erode_img)} voxels")
    inf_limit_lv = int(filled[0])
    com_mv = get_com(work[MV])[0]                             # V3
    dc = int((com_mv - inf_limit_lv) / 3)
    apical_extent, mid_extent, basal_extent = inf_limit_lv + dc, inf_limit_lv + 2 * dc, com_mv
    say("  Apex (long axis) slice:      ", inf_limit_lv, "\n  Apical section extent slice: ", apical_extent,
        "\n  Mid section extent slice:    ", mid_extent, "\n  Basal section extent slice:  ", basal_extent)

    # Module 4: the two reference angles on the host (fp64 numpy), then every slice's sectors in one launch
    say("Module 4: Segment generation.")
    nz = lv_myo.shape[0]
    theta_rv_insertion = []
    lo = max(mid_extent, 0)
    rv_basal = work[RV].tensor[lo:max(mid_extent + 5, lo)].cpu().numpy()        # only these five slices are read back
    for z in range(mid_extent, mid_extent + 5):
        lv_com = _slice_com_int(m_lv, z, "the left ventricle")
        _slice_com_int(m_rv, z, "the right ventricle")
        loc_y, loc_x = np.where(rv_basal[z - lo])
        theta_rv = np.arctan2(lv_com[0] - loc_y, loc_x - lv_com[1])
        theta_rv[theta_rv < 0] += 2 * np.pi
        theta_rv_insertion.append(theta_rv.min())
    theta_0 = float(np.median(theta_rv_insertion))
    if apical_extent <= inf_limit_lv:
        raise ValueError(f"{who}: the left ventricle has no apical slices (slices {inf_limit_lv} ... {basal_extent})")
    lv_com_apical = np.mean([_slice_com_int(m_lv, z, "the left ventricle") for z in range(inf_limit_lv, apical_extent)], axis=0)
    rv_com_apical = np.mean([_slice_com_int(m_rv, z, "the right ventricle") for z in range(inf_limit_lv, apical_extent)], axis=0)
    theta_0_apical = float(np.arctan2(lv_com_apical[0] - rv_com_apical[0], rv_com_apical[1] - lv_com_apical[1]))
    say("  RV insertion angle (basal section): ", theta_0, "\n Apical LV-RV COM angle: ", theta_0_apical)

    rules, first = [], {}
    for key, rs in (("apical", APICAL_RULES), ("mid", MID_RULES), ("basal", BASAL_RULES)):
        first[key] = (len(rules), len(rs))
        rules += [(label, _lib.POLAR_CW if cw else 0, a0, a1) for label, cw, a0, a1 in rs]
    first["apex"] = (len(rules), 1)
    rules.append((17, _lib.POLAR_ANY_AREA, -np.inf, np.inf))                   # V7: segment 17 is not put to the area test
    slices, origins = [], {}
    for z in range(nz):
        if inf_limit_lv <= z < apical_extent:
            key, t0, rmin = "apical", theta_0_apical, 0.0
        elif apical_extent <= z < mid_extent:
            key, t0, rmin = "mid", theta_0, 0.0
        elif mid_extent <= z < basal_extent:
            key, t0, rmin = "basal", theta_0, float(BASAL_RADIUS_MIN)
        elif z < inf_limit_lv:
            slices.append((0.0, 0.0, 0.0, 0.0) + first["apex"])
            continue
        else:
            key = None
        if key is None or m_myo[z, 3] == 0:                                    # V8
            slices.append((0.0, 0.0, 0.0, 0.0, 0, 0))
            continue
        y_0, x_0 = _slice_com_int(m_myo, z, "the myocardium")                  # V3
        origins[z] = (y_0, x_0)
        slices.append((float(y_0), float(x_0), t0, rmin) + first[key])
    sp = lv_myo.GetSpacing()
    ctx = runtime.context(lv_myo.device)
    bits = torch.empty(lv_myo.shape, dtype=torch.int32, device=lv_myo.device)      # (uint32 words; torch has no arithmetic on them)
    counts = torch.empty((nz, 32), dtype=torch.int64, device=lv_myo.device)
    ctx.polar_sectors(lv_myo.tensor, lv_myo.GetSize(), slices, rules, float(np.prod(sp[:2])), float(min_area_mm2), bits, counts)

    # Module 5: back into image space
    say("  Module 5: Re-orientation.")
    inverse = CompositeTransform(transforms).GetInverse()
    A, off, _ = _split_transform(inverse, lv_myo)
    planes = torch.empty((17,) + lv_myo.shape, dtype=torch.uint8, device=lv_myo.device)
    ctx.resample_bits(bits, lv_myo.geom(), lv_myo.geom(), 17, planes, affine_A=A.ravel(), affine_t=off)
    zero = template.like(torch.zeros(template.shape, dtype=torch.uint8, device=template.device))
    out = {}
    for k in range(17):
        seg = lv_myo.like(planes[k])
        if hole_fill_mm > 0:
            seg = binary_morphological_closing(seg, hole_fill_img)
        out[f"Ventricle_L_Segment{k + 1}"] = paste(zero, seg, cb_index)
    if info is not None:
        info.update(rotation_angles=angles, rotation_centres=centres, rotation_axes=rot_axes, inf_limit_lv=inf_limit_lv,
                    apical_extent=apical_extent, mid_extent=mid_extent, basal_extent=basal_extent, theta_0=theta_0,
                    theta_0_apical=theta_0_apical, slice_origins=origins, counts=counts.cpu().numpy())
    say("Complete!")
    return out
