from .deformable import fast_symmetric_forces_demons_registration, multiscale_demons, HipDemonsFilter  # noqa: F401
from .bspline import bspline_registration, refine_bspline  # noqa: F401
from .linear import linear_registration  # noqa: F401
from .utils import (  # noqa: F401
    apply_deformable_transform,
    apply_linear_transform,
    apply_transform,
    apply_transform_to_set,
    convert_mask_to_distance_map,
    control_point_spacing_distance_to_number,
    convert_mask_to_reg_structure,
    smooth_and_resample,
    transform_to_displacement_field,
)
from .field import (  # noqa: F401
    displacement_field_jacobian_determinant,
    inverse_consistency_error,
    inverse_transform,
    invert_displacement_field,
)
from ..label.region import connected_threshold  # noqa: E402,F401  (sitk.ConnectedThreshold: a region-growing segmentation filter)
from .qa import (  # noqa: E402,F401
    DIRQA_SETTINGS_DEFAULTS,
    Keypoints,
    PointTable,
    dir_qa,
    match_keypoints,
    sift_keypoints,
    target_registration_error,
    transform_points,
)
