from .fusion import combine_labels, combine_labels_staple, compute_patch_correlation_weight_map, compute_weight_map, process_probability_image, staple  # noqa: F401
from .iar import distance_map, evaluate_distance_to_reference, label_contour, run_iar  # noqa: F401
from . import comparison, region, utils  # noqa: F401
from .region import (  # noqa: F401
    binary_median, connected_component, label_moments, label_shape_statistics, principal_axes_from_moments, slice_convex_hull)
from .utils import (  # noqa: F401
    binary_decode_image, binary_dilate, binary_encode_structure_list, binary_erode, binary_fillhole, binary_morphological_closing,
    correct_volume_overlap, get_com, largest_component)
