"""Drop-in for platipy/imaging/projects/bronchus/{bronchus,run}.py (run_bronchus_segmentation): lung and proximal
bronchial tree of a thoracic CT, on the device.  Every voxel-level step is a HIP kernel behind the C ABI -- the labelling,
the per-label statistics, the nine region grows, the dilations, the median (csrc/pp_region.h, pp_morph.hip) -- and the host
reads back a label table or a count per decision, never a volume.

The reference's quirks are kept (B1, B2 live in utils/lung.py):
  B3 (bronchus.py:203-212)  the seed slab is z_size - d - 10 : z_size - d with Python's slice semantics (clamped, a
                            negative start counts from the top).
  B4 (:219-229)             of the slab's components with physical size > 2000 the seed region is the one of strictly
                            greatest elongation (the first one on ties).
  B5 (:227-229, :220)       the seed is the region's centroid mapped to an index of the FULL image, rounded half up;
                            [0, 0, 0] when no region qualifies.
  B6 (:189, :200)           the fast_mode breaks sit at the two outer loops only: once a seed is found all HU values run.
  B7 (:278, :312)           sizes are truncated with int(); the best candidate is the strictly largest passing size, so
                            the first of equal sizes stays.
  B8 (:326-347, :159)       the carina search runs range(z_size - best_distance, 0, -1), wants exactly two components,
                            both int(size) > the minimum, and crops at carina + round(extend_mm / z_spacing).
Deviations: get_lung_mask returns None where the reference raises IndexError, and run_bronchus_segmentation turns that into
a ValueError; generate_airway_mask returns None where the reference dies in fast_mask(None), and run_bronchus_segmentation
then returns the lung alone, which is what its `if not bronchus_mask` branch intends.  Nothing is written to `dest`;
get_distance (it reads files) is not provided.  Parity with SimpleITK itself is UNPINNED (label/region.py)."""
import logging

import numpy as np
import torch

from .. import runtime
from ..image import as_image
from ..label.region import binary_median, connected_component, connected_threshold, label_shape_statistics, physical_point_to_index
from ..label.utils import binary_dilate
from ..utils.lung import detect_holes, get_lung_mask

logger = logging.getLogger(__name__)


def fast_mask(img, start, end):
    """The image with slices start:end set to 0 (bronchus.py:38-56); as in the reference the result is float64."""
    img = as_image(img)
    t = img.tensor.to(torch.float64).clone()
    t[start:end] = 0
    return img.like(t)


def generate_lung_mask(img):
    """The initial airway mask, lungs included (bronchus.py:107-124): detect_holes, then get_lung_mask.  None when no hole
    passes the flatness test."""
    label_image, labels = detect_holes(img)
    return get_lung_mask(label_image, labels)


default_settings = {
    "fast_mode": True,
    "extend_from_carina_mm": 40,
    "minimum_tree_half_physical_size": 1000,
    "lung_mask_hu_values": [-750, -775, -800, -825, -850, -900, -700, -950, -650],
    "distance_from_supu_slice_values": [3, 10, 20],
    "expected_physical_size_range": [22000, 150000],
}


def _slab_image(img, tensor, z0):
    """`tensor` = slices z0 ... of an image on img's grid, with the origin sitk's slicing gives it."""
    d = np.asarray(img.GetDirection(), dtype=np.float64).reshape(3, 3)
    sp = np.asarray(img.GetSpacing(), dtype=np.float64)
    origin = np.asarray(img.GetOrigin(), dtype=np.float64) + d @ (sp * np.array([0.0, 0.0, float(z0)]))
    return type(img)(tensor, img.GetSpacing(), tuple(origin), img.GetDirection())


def _carina_slice(best_result, start, minimum_size, voxel):
    """B8 on the device: for idx = start ... 1 label the z-prefix mask[0:idx] -- contiguous, so labelled in place -- of the
    airway's bounding box (component count and sizes do not change under cropping) and stop at the first idx with exactly two
    components, both int(size) > minimum_size.  -> idx or -1."""
    ctx = runtime.context(best_result.device)
    box = ctx.bounding_box(best_result.tensor, best_result.GetSize(), False)
    if box[0] > box[1]:
        return -1
    crop = best_result.tensor[box[4]:box[5] + 1, box[2]:box[3] + 1, box[0]:box[1] + 1].contiguous()
    labels = torch.empty(crop.shape, dtype=torch.int32, device=crop.device)
    nz, ny, nx = crop.shape
    done = None
    for idx_slice in range(start, 0, -1):
        m = min(idx_slice, box[5] + 1) - box[4]
        if m <= 0:
            break               # the cut mask is empty from here down: no slice can have two components
        if m == done:
            continue            # the same prefix as the slice above, which did not pass
        done = m
        if ctx.connected_components(crop, (nx, ny, m), labels) != 2:
            continue
        st = label_shape_statistics(best_result.like(labels[:m]), 2)
        if int(st[1]["count"] * voxel) > minimum_size and int(st[2]["count"] * voxel) > minimum_size:
            return idx_slice
    return -1


def generate_airway_mask(dest, img, lung_mask, config_dict=None):
    """The final bronchus segmentation (bronchus.py:137-355) -> uint8 mask on img's grid, or None when no candidate's size is
    inside expected_physical_size_range.  `dest` is accepted and ignored: no file is written.  What was decided -- "seed",
    "lung_mask_hu", "distance_from_sup_slice", "physical_size", "carina_slice", "extend_from_carina", "candidates" -- is logged
    and kept in generate_airway_mask.last_info."""
    if not config_dict:
        config_dict = default_settings
    img, lung_mask = as_image(img), as_image(lung_mask)
    fast_mode = config_dict["fast_mode"]
    extend_from_carina_mm = config_dict["extend_from_carina_mm"]
    lung_mask_hu_values = config_dict["lung_mask_hu_values"]
    minimum_tree_half_physical_size = config_dict["minimum_tree_half_physical_size"]
    distance_from_supu_slice_values = config_dict["distance_from_supu_slice_values"]
    expected_physical_size_range = config_dict["expected_physical_size_range"]

    z_size = img.GetDepth()
    spacing = img.GetSpacing()
    z_spacing = spacing[2]
    voxel = float(np.prod(np.asarray(spacing, dtype=np.float64)))
    extend_from_carina = round(extend_from_carina_mm / z_spacing)
    ct = img.like(img.tensor.to(torch.float32))
    if lung_mask.tensor.dtype != torch.uint8:
        lung_mask = lung_mask.like((lung_mask.tensor != 0).to(torch.uint8))

    processed_correctly = False
    best_result = None
    best_result_sim = 0
    best_lung_mask_hu = 0
    best_distance_from_sup_slice = 0
    best_seed = None
    candidates = []

    for k in range(2):
        if processed_correctly and fast_mode:       # B6
            break
        if k == 1:
            lung_mask = binary_median(lung_mask, 1)     # smoothing the lung mask affects all tests below
        for distance_from_sup_slice in distance_from_supu_slice_values:
            if processed_correctly and fast_mode:   # B6
                break
            lo, hi, _ = slice(z_size - distance_from_sup_slice - 10, z_size - distance_from_sup_slice).indices(z_size)    # B3
            max_elong = 0
            airway_open = [0, 0, 0]                 # B5
            if hi > lo:
                connected, count = connected_component(_slab_image(img, lung_mask.tensor[lo:hi], lo))
                for label, st in label_shape_statistics(connected, count).items():
                    if st["elongation"] > max_elong and st["physical_size"] > 2000:     # B4
                        centre = physical_point_to_index(img, st["centroid"])           # B5
                        max_elong = st["elongation"]
                        airway_open = [int(centre[0]), int(centre[1]), int(centre[2])]
            if int(lung_mask.tensor[airway_open[2], airway_open[1], airway_open[0]]) == 0:
                logger.info("error locating trachea centroid at distance %d (additional air features on this slice?)", distance_from_sup_slice)
                continue
            for lung_mask_hu in lung_mask_hu_values:
                result = connected_threshold(ct, [airway_open], -2000, lung_mask_hu)
                result = binary_dilate(result, 2)
                voxels = int(result.tensor.sum(dtype=torch.int64))
                if voxels == 0:
                    candidates.append((k, distance_from_sup_slice, lung_mask_hu, -1, False))
                    continue
                airway_mask_physical_size = int(voxels * voxel)     # B7
                passed = expected_physical_size_range[0] <= airway_mask_physical_size <= expected_physical_size_range[1]
                candidates.append((k, distance_from_sup_slice, lung_mask_hu, airway_mask_physical_size, passed))
                logger.info("airway mask k=%d distance=%d HU=%s size=%d %s", k, distance_from_sup_slice, lung_mask_hu, airway_mask_physical_size,
                            "passed" if passed else "failed")
                if passed:
                    processed_correctly = True
                if airway_mask_physical_size > best_result_sim and passed:      # B7
                    best_result_sim = airway_mask_physical_size
                    best_result = result
                    best_lung_mask_hu = lung_mask_hu
                    best_distance_from_sup_slice = distance_from_sup_slice
                    best_seed = list(airway_open)

    info = {"seed": best_seed, "lung_mask_hu": best_lung_mask_hu, "distance_from_sup_slice": best_distance_from_sup_slice,
            "physical_size": best_result_sim, "carina_slice": -1, "extend_from_carina": extend_from_carina, "candidates": candidates}
    generate_airway_mask.last_info = info
    if best_result is None:
        logger.error("unable to process correctly: no airway candidate inside %s", expected_physical_size_range)
        return None

    corina_slice = _carina_slice(best_result, z_size - best_distance_from_sup_slice, minimum_tree_half_physical_size, voxel)     # B8
    info["carina_slice"] = corina_slice
    out = best_result.tensor.clone()
    if corina_slice >= 0:
        logger.info("cropping from slice %d + %d slices", corina_slice, extend_from_carina)
        out[corina_slice + extend_from_carina:z_size] = 0
    logger.info("selected lung mask HU %s, seed %s, distance %d", best_lung_mask_hu, best_seed, best_distance_from_sup_slice)
    return img.like(out)


generate_airway_mask.last_info = None

BRONCHUS_SETTINGS_DEFAULTS = {
    "outputBronchusName": "Auto_Bronchus",
    "outputLungName": "Auto_Lung",
    "algorithmSettings": default_settings,
}


def run_bronchus_segmentation(input_image, settings=BRONCHUS_SETTINGS_DEFAULTS):
    """Runs the proximal bronchial tree segmentation (bronchus/run.py:33-66) -> {settings["outputLungName"]: lung mask,
    settings["outputBronchusName"]: bronchus mask}, uint8 on the input grid; the bronchus entry is missing when no airway
    candidate passes.  ValueError when the image holds no lung (see the module docstring).  The decisions of the airway search
    are kept in run_bronchus_segmentation.last_info."""
    input_image = as_image(input_image)
    results = {}
    run_bronchus_segmentation.last_info = None
    lung_mask = generate_lung_mask(input_image)
    if lung_mask is None:
        raise ValueError("run_bronchus_segmentation: no air region of the image passes the lung test (flatness <= 2)")
    results[settings["outputLungName"]] = lung_mask
    bronchus_mask = generate_airway_mask(None, input_image, lung_mask, config_dict=settings["algorithmSettings"])
    run_bronchus_segmentation.last_info = generate_airway_mask.last_info
    if bronchus_mask is None:
        logger.error("Unable to generate bronchus mask")
        return results
    results[settings["outputBronchusName"]] = bronchus_mask
    return results


run_bronchus_segmentation.last_info = None
