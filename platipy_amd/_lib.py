"""ctypes binding of the C ABI in include/platipy_amd.h (libplatipy_hip.so, gfx950).

The product path has no CPU fallback: if the shared library is missing or fails to load, every
operation raises.  `Context` methods take raw device addresses (ints); `ptr()` extracts one from
a torch tensor.  The same binding class is pointed at the CPU-emulated build of the identical
kernel sources by the test-suite only (tests/emu), never by the package itself.
"""
import ctypes as C

import numpy as np
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libplatipy_hip.so")

PP_OK = 0
INTERP_NEAREST = 1
INTERP_LINEAR = 2
INTERP_BSPLINE = 3
DEMONS_AUTO, DEMONS_STAGED, DEMONS_FUSED = 0, 1, 2
ABI_VERSION = 6
HISTORY_CAPACITY = 4096     # PP_DEMONS_HISTORY_CAPACITY: iterations of one Execute whose metric / RMS change the device ring keeps


class Geom(C.Structure):
    _fields_ = [("size", C.c_int * 3), ("spacing", C.c_double * 3), ("origin", C.c_double * 3),
                ("direction", C.c_double * 9)]


class MiBins(C.Structure):
    """pp_mi_bins"""
    _fields_ = [("nbins", C.c_int), ("kernel", C.c_int), ("f_bin", C.c_double), ("f_norm_min", C.c_double), ("m_bin", C.c_double),
                ("m_norm_min", C.c_double)]


MI_MATTES, MI_JOINT = 0, 1


class LinregLevel(C.Structure):     # pp_linreg_level
    _fields_ = [("model", C.c_int), ("metric", C.c_int), ("optimizer", C.c_int), ("iterations", C.c_int), ("vsize", C.c_int * 3),
                ("stride", C.c_int), ("speculation", C.c_int), ("flags", C.c_int),
                ("v_i2p", C.c_double * 9), ("v_origin", C.c_double * 3), ("f_p2i", C.c_double * 9), ("f_origin", C.c_double * 3),
                ("m_p2i", C.c_double * 9), ("m_origin", C.c_double * 3), ("init_matrix", C.c_double * 9),
                ("init_offset", C.c_double * 3), ("center", C.c_double * 3), ("v_min_spacing", C.c_double)]


class LinregStats(C.Structure):     # pp_linreg_stats
    _fields_ = [("iterations", C.c_int), ("evaluations", C.c_int), ("stop", C.c_int), ("reserved", C.c_int), ("value", C.c_double),
                ("learning_rate", C.c_double)]


ERR_ARG, ERR_SIZE = -1, -5
ERR_UNSUPPORTED = -4
RESAMPLE_SET_MAX_LABELS = 16    # PP_RESAMPLE_SET_MAX_LABELS
PROJECT_MAX_LABELS = 16         # PP_PROJECT_MAX_LABELS
PROJECT_SUM, PROJECT_MEAN, PROJECT_MEDIAN, PROJECT_STD, PROJECT_MIN, PROJECT_MAX = range(6)     # PP_PROJECT_*
PROJECT_KINDS = {"sum": PROJECT_SUM, "mean": PROJECT_MEAN, "median": PROJECT_MEDIAN, "std": PROJECT_STD, "min": PROJECT_MIN,
                 "max": PROJECT_MAX}
ERR_NO_OVERLAP = -6
ERR_DIRECTION = -7
ERR_INVALID = -8        # PP_ERR_INVALID: a seed outside the buffer
BSPLINE_MEAN_SQUARES, BSPLINE_CORRELATION = 0, 1
MODEL_TRANSLATION, MODEL_VERSOR_RIGID, MODEL_SIMILARITY, MODEL_SCALE, MODEL_AFFINE, MODEL_EULER, MODEL_SCALE_VERSOR, MODEL_SCALE_SKEW_VERSOR = range(8)
OPT_GD, OPT_GD_LINE_SEARCH = 0, 1
LINREG_RETURN_BEST = 1


class DemonsParams(C.Structure):
    _fields_ = [
        ("iterations", C.c_int),
        ("sigma_d_vox", C.c_double * 3),
        ("sigma_u_vox", C.c_double * 3),
        ("smooth_displacement", C.c_int),
        ("smooth_update", C.c_int),
        ("max_rms_error", C.c_double),
        ("max_step_length", C.c_double),
        ("intensity_threshold", C.c_double),
        ("denominator_threshold", C.c_double),
        ("max_error", C.c_double),
        ("max_kernel_width", C.c_int),
        ("variant", C.c_int),
    ]


class DemonsStats(C.Structure):
    _fields_ = [
        ("metric", C.c_double),
        ("rms_change", C.c_double),
        ("sum_sq_diff", C.c_double),
        ("sum_sq_change", C.c_double),
        ("n_pixels", C.c_int64),
        ("elapsed_iterations", C.c_int),
        ("halted", C.c_int),
    ]


class ProfileEntry(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int), ("total_ms", C.c_double)]


STAPLE_MAX_RATERS = 64
STAPLE_FOREGROUND, STAPLE_BINARY_THRESHOLD = 0, 1


class StapleParams(C.Structure):    # pp_staple_params
    _fields_ = [("foreground_test", C.c_int), ("rescale", C.c_int), ("foreground_value", C.c_double),
                ("confidence_weight", C.c_double), ("maximum_iterations", C.c_uint64), ("threshold_lower", C.c_double)]


class StapleResult(C.Structure):    # pp_staple_result
    _fields_ = [("sensitivity", C.c_double * STAPLE_MAX_RATERS), ("specificity", C.c_double * STAPLE_MAX_RATERS),
                ("elapsed_iterations", C.c_uint64), ("n_zero", C.c_int64), ("n_one", C.c_int64), ("n_mixed", C.c_int64),
                ("degenerate", C.c_int), ("reserved", C.c_int)]


SURFACE_CONTOUR_ABS, SURFACE_LABEL_POS, SURFACE_NONZERO = 0, 1, 2
SURFACE_BINS = 128
# pp_surface_stats as a numpy record (the struct lives in device memory; the host views the bytes it reads back)
SURFACE_STATS_DTYPE = np.dtype([("count", "<i8"), ("count_le_tau", "<i8"), ("sum", "<f8"), ("sum_sq", "<f8"), ("min", "<f4"),
                                ("max", "<f4"), ("range_lo", "<f4"), ("range_hi", "<f4"), ("hist", "<i8", (SURFACE_BINS,))])


# pp_contour, and the two constants of pp_contour_fill_u8: edges staged per pass (PP_CONTOUR_CHUNK), the vertex bound
CONTOUR_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("structure", "<i4"), ("z", "<i4")])
CONTOUR_CHUNK, CONTOUR_MAX_INDEX = 256, 1 << 24

DOSE_MAX_LABELS, DOSE_MAX_BINS, ORDER_STATS_MAX_RANKS = 64, 1 << 20, 8
TEXTURE_MAX_NG, TEXTURE_LDS_WORDS, DISCRETISE_MAX_LEVELS = 1024, 8192, 65535     # TX_MAX_NG, TX_LDS_WORDS, RD_MAX_LEVELS of csrc/pp_radiomics.h
# pp_dose_stats as a numpy record
DOSE_STATS_DTYPE = np.dtype([("count", "<i8"), ("mask_sum", "<i8"), ("dose_sum", "<f8"), ("dose_min", "<f4"), ("dose_max", "<f4")])


class InvertStats(C.Structure):      # pp_invert_stats
    _fields_ = [("iterations", C.c_int), ("reserved", C.c_int), ("max_error_norm", C.c_double), ("mean_error_norm", C.c_double)]


class JacobianStats(C.Structure):    # pp_jacobian_stats
    _fields_ = [("min", C.c_double), ("max", C.c_double), ("mean", C.c_double), ("count", C.c_int64), ("count_nonpositive", C.c_int64)]


INVERT_MAX_ITERATIONS = 256

POLAR_CW, POLAR_ANY_AREA = 1, 2      # PP_POLAR_CW, PP_POLAR_ANY_AREA
# pp_polar_slice / pp_polar_rule as numpy records (host tables of pp_polar_sectors_u8)
POLAR_SLICE_DTYPE = np.dtype([("cy", "<f8"), ("cx", "<f8"), ("theta0", "<f8"), ("radius_min", "<f8"), ("first_rule", "<i4"), ("nrules", "<i4")])
POLAR_RULE_DTYPE = np.dtype([("label", "<i4"), ("flags", "<i4"), ("angle_min", "<f8"), ("angle_max", "<f8")])


class PlatipyAmdError(RuntimeError):
    pass


_P = C.c_void_p
_SIGNATURES = {
    "pp_abi_version": (C.c_int, []),
    "pp_create": (C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    "pp_destroy": (None, [_P]),
    "pp_last_error": (C.c_char_p, [_P]),
    "pp_set_stream": (C.c_int, [_P, _P]),
    "pp_sync": (C.c_int, [_P]),
    "pp_workspace_bytes": (C.c_size_t, [_P]),
    "pp_profile_enable": (C.c_int, [_P, C.c_int]),
    "pp_profile_read": (C.c_int, [_P, C.POINTER(ProfileEntry), C.c_int]),
    "pp_gauss_taps": (C.c_int, [C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int]),
    "pp_demons_default_params": (None, [C.POINTER(DemonsParams)]),
    "pp_discrete_gaussian_f32": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.c_double, C.c_int, C.c_int]),
    "pp_discrete_gaussian_rows_f32": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.c_double, C.c_int, C.c_int, _P, _P]),
    "pp_smooth_field_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_double, C.c_int]),
    "pp_recursive_gaussian_field_f32": (C.c_int, [_P, _P, C.POINTER(Geom), C.POINTER(C.c_double)]),
    "pp_recursive_gaussian_f32": (C.c_int, [_P, _P, _P, C.POINTER(Geom), C.POINTER(C.c_double)]),
    "pp_warp_f32": (C.c_int, [_P, _P, _P, C.POINTER(Geom), C.c_float, _P]),
    "pp_resample_f32": (C.c_int, [_P, _P, C.POINTER(Geom), C.POINTER(Geom), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  _P, C.c_int, C.c_double, _P]),
    "pp_resample_u8": (C.c_int, [_P, _P, C.POINTER(Geom), C.POINTER(Geom), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 _P, C.c_int, C.c_double, _P]),
    "pp_resample_set": (C.c_int, [_P, C.POINTER(Geom), C.POINTER(Geom), C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _P, C.c_int,
                                  C.c_double, _P, C.POINTER(_P), C.c_int, C.POINTER(_P)]),
    "pp_project_set": (C.c_int, [_P, C.POINTER(Geom), C.c_int, C.POINTER(C.c_double), C.c_int, _P, C.c_int, C.c_int, C.c_double, _P,
                                 C.POINTER(_P), C.POINTER(C.c_int), C.c_int, C.POINTER(_P)]),
    "pp_resample_field_f32": (C.c_int, [_P, _P, C.POINTER(Geom), C.POINTER(Geom), _P]),
    "pp_bspline_prefilter_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P]),
    "pp_compose_field_f32": (C.c_int, [_P, _P, _P, C.POINTER(Geom)]),
    "pp_transform_to_field_f32": (C.c_int, [_P, C.POINTER(Geom), C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _P]),
    "pp_demons_force_f32": (C.c_int, [_P, _P, _P, C.POINTER(Geom), C.POINTER(DemonsParams), _P, C.POINTER(DemonsStats)]),
    "pp_demons_execute_f32": (C.c_int, [_P, _P, _P, C.POINTER(Geom), C.POINTER(DemonsParams), _P, C.POINTER(DemonsStats)]),
    "pp_demons_history": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]),
    "pp_weight_map_local_f32": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_double, C.c_double, _P]),
    "pp_weight_map_block_f32": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_double, C.c_double, _P]),
    "pp_sum_sq_diff_f32": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_double)]),
    "pp_fuse_accumulate_u8": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t]),
    "pp_fuse_accumulate_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t]),
    "pp_fuse_divide_f32": (C.c_int, [_P, _P, _P, _P, C.c_size_t]),
    "pp_minmax_f32": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pp_rescale_threshold_f32": (C.c_int, [_P, _P, C.c_size_t, C.c_float, C.c_float, C.c_float]),
    "pp_binary_threshold_f32": (C.c_int, [_P, _P, C.c_size_t, C.c_double, C.c_double, _P]),
    "pp_fillhole_largest_component_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, _P, C.POINTER(C.c_int64)]),
    "pp_fillhole_largest_component_conn_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_int64)]),
    "pp_binary_morph_ball_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, _P]),
    "pp_bounding_box": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pp_staple_fuse": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_size_t, C.POINTER(StapleParams), _P,
                                 C.POINTER(StapleResult)]),
    "pp_patch_correlation_f32": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "pp_joint_histogram_f32": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "pp_dose_histogram_f32": (C.c_int, [_P, _P, C.POINTER(_P), C.c_int, C.c_size_t, C.POINTER(C.c_double), C.c_int,
                                        C.POINTER(C.c_int64), _P]),
    "pp_masked_order_stats_f32": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_float)]),
    "pp_masked_count_ge_f32": (C.c_int, [_P, _P, C.POINTER(_P), C.c_int, C.c_size_t, C.POINTER(C.c_float), C.c_int,
                                         C.POINTER(C.c_int64)]),
    "pp_masked_moments_f32": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64),
                                        C.POINTER(C.c_double)]),
    "pp_radiomics_discretise_f32": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_double), C.c_int, _P]),
    "pp_texture_neighbourhood_u16": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                               C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pp_texture_runs_u16": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "pp_dog_extrema_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pp_sift_describe_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, _P]),
    "pp_descriptor_match_f32": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, C.c_double, _P, _P, _P]),
    "pp_transform_points_f64": (C.c_int, [_P, _P, C.POINTER(Geom), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]),
    "pp_label_contour_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P]),
    "pp_distance_map_f32": (C.c_int, [_P, _P, C.POINTER(Geom), C.c_int, C.c_int, _P]),
    "pp_overlap_counts_u8": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_int64)]),
    "pp_binary_contour_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, _P]),
    "pp_slice_contour_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P]),
    "pp_abs_range_f32": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "pp_surface_stats_f32": (C.c_int, [_P, _P, _P, C.POINTER(Geom), C.c_int, C.c_double, _P, _P]),
    "pp_slice_masked_count_u8": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int), _P]),
    "pp_meansq_affine_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int), C.c_int, _P, _P, C.POINTER(C.c_double)]),
    "pp_corr_moments_affine_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_int), C.c_int, _P, _P, C.POINTER(C.c_double)]),
    "pp_metric_values_affine_f32": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int), _P, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                              C.POINTER(C.c_int), C.c_int, _P, _P, C.POINTER(C.c_double)]),
    "pp_linear_set_sample_jitter": (C.c_int, [_P, _P, C.c_size_t]),
    "pp_linear_set_moving_gradient": (C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    "pp_linear_set_moving_gradient_packed": (C.c_int, [_P, _P]),
    "pp_recursive_gaussian_pass_f32": (C.c_int, [_P, _P, _P, C.POINTER(Geom), C.c_int, C.c_double, C.c_int, C.c_int]),
    "pp_mi_histogram_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, _P, _P, C.POINTER(MiBins),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pp_mi_gradient_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, _P, _P, C.POINTER(MiBins),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pp_linear_num_parameters": (C.c_int, [C.c_int]),
    "pp_reload_switches": (None, []),
    "pp_linear_optimize_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P, C.POINTER(C.c_int), _P, _P, C.POINTER(LinregLevel),
                                         C.POINTER(C.c_double), C.POINTER(LinregStats), C.POINTER(C.c_double), C.c_int]),
    "pp_bspline_field_f32": (C.c_int, [_P, _P, C.POINTER(Geom), C.POINTER(Geom), _P]),
    "pp_bspline_metric_f32": (C.c_int, [_P, C.c_int, _P, C.POINTER(Geom), _P, C.POINTER(Geom), C.POINTER(Geom), C.c_int, _P, _P, _P,
                                        C.POINTER(Geom), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]),
    "pp_bspline_mi_histogram_f32": (C.c_int, [_P, _P, C.POINTER(Geom), _P, C.POINTER(Geom), C.POINTER(Geom), C.c_int, _P, _P, _P,
                                              C.POINTER(Geom), C.c_double, C.POINTER(MiBins), C.POINTER(C.c_double),
                                              C.POINTER(C.c_double)]),
    "pp_bspline_mi_gradient_f32": (C.c_int, [_P, _P, C.POINTER(Geom), _P, C.POINTER(Geom), C.POINTER(Geom), C.c_int, _P, _P, _P,
                                             C.POINTER(Geom), C.c_double, C.POINTER(MiBins), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pp_slice_moments_u8": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(C.c_int), C.c_int, _P]),
    "pp_tube_mask_u8": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.c_double, _P]),
    "pp_contour_fill_u8": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.POINTER(C.c_int), C.c_int, _P]),
    "pp_contour_trace_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_int64)]),
    "pp_connected_components_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P, C.POINTER(C.c_int)]),
    "pp_connected_components_conn_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, _P, C.POINTER(C.c_int)]),
    "pp_slice_convex_hull_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P]),
    "pp_label_moments_i32": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_int, _P]),
    "pp_connected_threshold_f32": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.c_double, C.c_double, C.POINTER(C.c_int), C.c_int, _P,
                                             C.POINTER(C.c_int64)]),
    "pp_binary_median_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "pp_polar_sectors_u8": (C.c_int, [_P, _P, C.POINTER(C.c_int), _P, _P, C.c_int, C.c_double, C.c_double, _P, _P]),
    "pp_resample_bits_u32": (C.c_int, [_P, _P, C.POINTER(Geom), C.POINTER(Geom), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, _P]),
    "pp_invert_field_f32": (C.c_int, [_P, _P, C.POINTER(Geom), _P, C.c_int, C.c_double, C.c_double, C.c_int, _P, C.POINTER(InvertStats)]),
    "pp_inverse_consistency_f32": (C.c_int, [_P, _P, _P, C.POINTER(Geom), _P, C.POINTER(InvertStats)]),
    "pp_jacobian_determinant_f32": (C.c_int, [_P, _P, C.POINTER(Geom), C.c_int, _P, _P, C.POINTER(JacobianStats)]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load(path=None):
    """dlopen the C-ABI library and declare every entry point.  Raises if it is absent."""
    path = path or DEFAULT_LIB
    if not os.path.exists(path):
        raise PlatipyAmdError(
            f"{path} not found: build it with `python -m platipy_amd._build` (needs hipcc). "
            "platipy_amd has no CPU fallback.")
    try:
        dll = C.CDLL(path)
    except OSError as e:  # e.g. libamdhip64 missing
        raise PlatipyAmdError(f"cannot load {path}: {e}") from e
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(dll, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    if dll.pp_abi_version() != ABI_VERSION:
        raise PlatipyAmdError(f"{path}: ABI version {dll.pp_abi_version()} != {ABI_VERSION}")
    _LOADED.append(dll)
    return dll


_LOADED = []


def reload_switches():
    """pp_reload_switches() on every library this process loaded: the PP_* measurement switches are read from the environment
    once; tests and A/B tools that flip one inside a process call this afterwards (not while kernels are being launched from
    another thread)."""
    for d in _LOADED:
        d.pp_reload_switches()


_DLL = None


def dll():
    global _DLL
    if _DLL is None:
        _DLL = load()
    return _DLL


def ptr(x):
    """Device (or, in the emulated test build, host) address of a tensor/array, or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return x.ctypes.data  # numpy (test builds only)


def make_geom(size, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), direction=(1, 0, 0, 0, 1, 0, 0, 0, 1)):
    g = Geom()
    g.size[:] = [int(s) for s in size]
    g.spacing[:] = [float(s) for s in spacing]
    g.origin[:] = [float(s) for s in origin]
    g.direction[:] = [float(s) for s in direction]
    return g


def _i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _dn(v, n):
    if v is None:
        return None
    return (C.c_double * n)(*[float(x) for x in v])


def _nbytes(buf):
    """Bytes of a tensor / array, or None for a bare address (nothing to check)."""
    if buf is None or isinstance(buf, int):
        return None
    return buf.numel() * buf.element_size() if hasattr(buf, "numel") else buf.nbytes


def _check_volume(who, size, **buffers):
    """The library gets bare pointers: a buffer that does not have its geometry's size would be read or written past its
    end.  buffers: name=(buffer, bytes per voxel)."""
    if len(size) != 3 or min(int(s) for s in size) <= 0:
        raise ValueError(f"{who}: size must be three positive voxel counts, got {tuple(size)}")
    n = int(size[0]) * int(size[1]) * int(size[2])
    for name, (buf, width) in buffers.items():
        have = _nbytes(buf)
        if have is not None and have != width * n:
            raise ValueError(f"{who}: `{name}` does not have the size of its geometry ({have} bytes for {tuple(size)})")


def gauss_taps(variance, max_error, max_kernel_width, lib=None):
    lib = lib or dll()
    buf = (C.c_double * 1024)()
    r = lib.pp_gauss_taps(float(variance), float(max_error), int(max_kernel_width), buf, 1024)
    if r < 0:
        raise PlatipyAmdError(f"pp_gauss_taps failed ({r})")
    return [buf[i] for i in range(2 * r + 1)]


class Context:
    """One pp_ctx: a (device, stream) pair plus its scratch memory."""

    def __init__(self, device=0, stream=0, lib=None):
        self.lib = lib or dll()
        h = _P()
        rc = self.lib.pp_create(int(device), _P(stream or None), C.byref(h))
        if rc != PP_OK:
            raise PlatipyAmdError(f"pp_create(device={device}) failed ({rc})")
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.lib.pp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != PP_OK:
            msg = self.lib.pp_last_error(self.h)
            raise PlatipyAmdError(f"{what} failed ({rc}): {msg.decode(errors='replace') if msg else ''}")

    def set_stream(self, stream):
        self._chk(self.lib.pp_set_stream(self.h, _P(stream or None)), "pp_set_stream")

    def sync(self):
        self._chk(self.lib.pp_sync(self.h), "pp_sync")

    def workspace_bytes(self):
        return self.lib.pp_workspace_bytes(self.h)

    def profile_enable(self, on=True, every=1):
        """Per-launch HIP events around the demons kernels; `every` = k > 1 brackets every k-th launch of each kernel."""
        self._chk(self.lib.pp_profile_enable(self.h, (max(1, int(every)) if on else 0)), "pp_profile_enable")

    def profile_read(self):
        """{kernel name: (launches, total ms)} since the last read (synchronises the stream)."""
        buf = (ProfileEntry * 32)()
        n = self.lib.pp_profile_read(self.h, buf, 32)
        if n < 0:
            self._chk(n, "pp_profile_read")
        return {buf[i].name.decode(): (buf[i].launches, buf[i].total_ms) for i in range(n)}

    def default_demons_params(self):
        p = DemonsParams()
        self.lib.pp_demons_default_params(C.byref(p))
        return p

    # -- FIR / IIR ------------------------------------------------------------------
    def discrete_gaussian(self, src, dst, size, spacing, variance, max_error=0.01, max_kernel_width=32, use_spacing=True):
        self._chk(self.lib.pp_discrete_gaussian_f32(self.h, ptr(src), ptr(dst), _i3(size), _d3(spacing), _d3(variance),
                                                    float(max_error), int(max_kernel_width), int(bool(use_spacing))),
                  "pp_discrete_gaussian_f32")

    def discrete_gaussian_rows(self, src, dst, size, spacing, variance, need_y, need_z, max_error=0.01, max_kernel_width=32,
                               use_spacing=True):
        """DiscreteGaussian valid only at rows (y, z) with need_y[y] and need_z[z] (uint8 device masks)."""
        self._chk(self.lib.pp_discrete_gaussian_rows_f32(self.h, ptr(src), ptr(dst), _i3(size), _d3(spacing), _d3(variance),
                                                         float(max_error), int(max_kernel_width), int(bool(use_spacing)), ptr(need_y),
                                                         ptr(need_z)), "pp_discrete_gaussian_rows_f32")

    def smooth_field(self, field, size, sigma_vox, max_error=0.1, max_kernel_width=30):
        self._chk(self.lib.pp_smooth_field_f32(self.h, ptr(field), _i3(size), _d3(sigma_vox), float(max_error),
                                               int(max_kernel_width)), "pp_smooth_field_f32")

    def recursive_gaussian_field(self, field, geom, sigma):
        self._chk(self.lib.pp_recursive_gaussian_field_f32(self.h, ptr(field), C.byref(geom), _d3(sigma)),
                  "pp_recursive_gaussian_field_f32")

    def recursive_gaussian(self, src, dst, geom, sigma):
        self._chk(self.lib.pp_recursive_gaussian_f32(self.h, ptr(src), ptr(dst), C.byref(geom), _d3(sigma)),
                  "pp_recursive_gaussian_f32")

    # -- warp / resample ------------------------------------------------------------
    def warp(self, moving, field, geom, edge_value, out):
        self._chk(self.lib.pp_warp_f32(self.h, ptr(moving), ptr(field), C.byref(geom), float(edge_value), ptr(out)),
                  "pp_warp_f32")

    def resample(self, src, gin, gout, out, affine_A=None, affine_t=None, field=None, interp=INTERP_LINEAR,
                 default_value=0.0, u8=False):
        fn = self.lib.pp_resample_u8 if u8 else self.lib.pp_resample_f32
        self._chk(fn(self.h, ptr(src), C.byref(gin), C.byref(gout), _dn(affine_A, 9), _dn(affine_t, 3), ptr(field),
                     int(interp), float(default_value), ptr(out)), "pp_resample")

    def resample_set(self, gin, gout, image=None, image_out=None, labels=(), labels_out=(), affine_A=None, affine_t=None, field=None,
                     interp=INTERP_LINEAR, default_value=0.0):
        """pp_resample_set: the fp32 `image` (or None) and the uint8 `labels` (at most RESAMPLE_SET_MAX_LABELS), all on `gin`,
        through one transform onto `gout` in one gather; every output is what `resample` gives for that member alone.  Raises
        PlatipyAmdError with .code (ERR_UNSUPPORTED for an interpolator the entry declines, ERR_ARG for a bad count)."""
        if len(labels) != len(labels_out):
            raise ValueError("resample_set: one output per label")
        n = len(labels)
        tin = (_P * max(n, 1))(*[ptr(x) for x in labels])
        tout = (_P * max(n, 1))(*[ptr(x) for x in labels_out])
        rc = self.lib.pp_resample_set(self.h, C.byref(gin), C.byref(gout), _dn(affine_A, 9), _dn(affine_t, 3), ptr(field), ptr(image),
                                      int(interp), float(default_value), ptr(image_out), tin, n, tout)
        if rc:
            msg = self.lib.pp_last_error(self.h)
            err = PlatipyAmdError(f"pp_resample_set failed ({rc}): {msg.decode(errors='replace') if msg else ''}")
            err.code = rc
            raise err

    def project_set(self, geom, axis, views, image=None, image_out=None, kind=PROJECT_MAX, interp=INTERP_LINEAR, default_value=0.0,
                    labels=(), labels_out=(), label_interp=INTERP_NEAREST):
        """pp_project_set: the fp32 `image` (or None) and the uint8 `labels` (at most PROJECT_MAX_LABELS), all on `geom`,
        through every transform of `views` ([nviews, 12]: row-major A, then t, of q = A p + t) and reduced along `axis`
        (0 = x, 1 = y, 2 = z) in one launch: the image with `kind` (PROJECT_*) into image_out [nviews, rows, cols] fp32, every
        label with max into labels_out[l] [nviews, rows, cols] uint8.  label_interp: one interpolator for all labels or one
        per label.  Raises PlatipyAmdError with .code (ERR_UNSUPPORTED for sitkBSpline, ERR_ARG for a bad argument).
        Waits for the stream while the views are uploaded; the kernel is only enqueued."""
        if len(labels) != len(labels_out):
            raise ValueError("project_set: one output per label")
        n = len(labels)
        v = np.ascontiguousarray(views, dtype=np.float64).reshape(-1)
        if v.size % 12:
            raise ValueError("project_set: `views` holds 12 doubles per view")
        li = [int(label_interp)] * n if np.isscalar(label_interp) else [int(i) for i in label_interp]
        if len(li) != n:
            raise ValueError("project_set: one interpolator per label")
        tin = (_P * max(n, 1))(*[ptr(x) for x in labels])
        tout = (_P * max(n, 1))(*[ptr(x) for x in labels_out])
        tli = (C.c_int * max(n, 1))(*li)
        rc = self.lib.pp_project_set(self.h, C.byref(geom), int(axis), v.ctypes.data_as(C.POINTER(C.c_double)), v.size // 12, ptr(image),
                                     int(kind), int(interp), float(default_value), ptr(image_out), tin, tli, n, tout)
        if rc:
            msg = self.lib.pp_last_error(self.h)
            err = PlatipyAmdError(f"pp_project_set failed ({rc}): {msg.decode(errors='replace') if msg else ''}")
            err.code = rc
            raise err

    def bspline_prefilter(self, src, size, out):
        """B-spline (order 3) coefficients of a fp32 volume (`out` may be `src`)."""
        self._chk(self.lib.pp_bspline_prefilter_f32(self.h, ptr(src), _i3(size), ptr(out)), "pp_bspline_prefilter_f32")

    def resample_field(self, src, gin, gout, out):
        self._chk(self.lib.pp_resample_field_f32(self.h, ptr(src), C.byref(gin), C.byref(gout), ptr(out)),
                  "pp_resample_field_f32")

    def transform_to_field(self, geom, A, t, add_field, out):
        """out = (A - I) p + t (+ add_field) on the grid `geom` (sitk.TransformToDisplacementField for a linear map)."""
        a = (C.c_double * 9)(*[float(v) for v in np.asarray(A, dtype=np.float64).ravel()])
        tt = (C.c_double * 3)(*[float(v) for v in np.asarray(t, dtype=np.float64).ravel()])
        self._chk(self.lib.pp_transform_to_field_f32(self.h, C.byref(geom), a, tt, ptr(add_field) if add_field is not None else None,
                                                     ptr(out)), "pp_transform_to_field_f32")

    def bspline_field(self, coefficients, lattice_geom, grid_geom, out):
        """Displacement field [3, Z, Y, X] of a cubic B-spline transform (coefficients [3, cz, cy, cx] on `lattice_geom`) on the
        grid `grid_geom`; exactly 0 outside the transform domain (pp_bspline_field_f32)."""
        self._chk(self.lib.pp_bspline_field_f32(self.h, ptr(coefficients), C.byref(lattice_geom), C.byref(grid_geom), ptr(out)),
                  "pp_bspline_field_f32")

    @staticmethod
    def _bspline_buffer_check(name, fixed, fixed_geom, moving, moving_geom, fixed_mask, moving_mask, coefficients, lattice_geom):
        """-> the number of coefficients.  The library gets bare pointers: a buffer that does not have its geometry's size would
        be read past its end."""
        for what, buf, g, width in (("fixed", fixed, fixed_geom, 4), ("moving", moving, moving_geom, 4), ("fixed_mask", fixed_mask, fixed_geom, 1),
                                    ("moving_mask", moving_mask, moving_geom, 1), ("coefficients", coefficients, lattice_geom, 12)):
            have = None if buf is None or isinstance(buf, int) else (buf.numel() * buf.element_size() if hasattr(buf, "numel") else buf.nbytes)
            if have is not None and have != width * int(g.size[0]) * int(g.size[1]) * int(g.size[2]):
                raise ValueError(f"{name}: `{what}` does not have the size of its geometry")
        return 3 * int(lattice_geom.size[0]) * int(lattice_geom.size[1]) * int(lattice_geom.size[2])

    def _bspline_raise(self, name, rc):
        msg = self.lib.pp_last_error(self.h)
        err = PlatipyAmdError(f"{name} failed ({rc}): {msg.decode(errors='replace') if msg else ''}")
        err.code = rc
        raise err

    def bspline_mi_histogram(self, fixed, fixed_geom, moving, moving_geom, virtual_geom, stride, coefficients, lattice_geom, bins,
                             fixed_mask=None, moving_mask=None, jitter_bound=0.0):
        """pp_bspline_mi_histogram_f32 -> (hist [nbins, nbins] float64, row = fixed bin; stats dict).  Raises PlatipyAmdError with
        .code (ERR_DIRECTION, ERR_NO_OVERLAP, ...)."""
        self._bspline_buffer_check("bspline_mi_histogram", fixed, fixed_geom, moving, moving_geom, fixed_mask, moving_mask, coefficients,
                                   lattice_geom)
        if not 1 <= int(bins.nbins) <= 64:      # the output array is sized from it
            raise ValueError("bspline_mi_histogram: 5..64 bins")
        hist = np.zeros((int(bins.nbins), int(bins.nbins)), dtype=np.float64)
        st = (C.c_double * 4)()
        rc = self.lib.pp_bspline_mi_histogram_f32(self.h, ptr(fixed), C.byref(fixed_geom), ptr(moving), C.byref(moving_geom),
                                                  C.byref(virtual_geom), int(stride), ptr(fixed_mask), ptr(moving_mask), ptr(coefficients),
                                                  C.byref(lattice_geom), float(jitter_bound), C.byref(bins),
                                                  hist.ctypes.data_as(C.POINTER(C.c_double)), st)
        if rc:
            self._bspline_raise("pp_bspline_mi_histogram_f32", rc)
        return hist, {"valid": st[0], "outside": st[1], "masked": st[2], "seen": st[3]}

    def bspline_mi_gradient(self, fixed, fixed_geom, moving, moving_geom, virtual_geom, stride, coefficients, lattice_geom, bins, table,
                            fixed_mask=None, moving_mask=None, jitter_bound=0.0):
        """pp_bspline_mi_gradient_f32 with the score `table` [nbins, nbins] -> (float64 gradient [3 cx cy cz] in ITK's parameter
        order, stats dict)."""
        n = self._bspline_buffer_check("bspline_mi_gradient", fixed, fixed_geom, moving, moving_geom, fixed_mask, moving_mask, coefficients,
                                       lattice_geom)
        tab = np.ascontiguousarray(table, dtype=np.float64)
        if tab.size != int(bins.nbins) ** 2:
            raise ValueError("bspline_mi_gradient: `table` is not nbins x nbins")
        grad = np.zeros(n, dtype=np.float64)
        st = (C.c_double * 4)()
        rc = self.lib.pp_bspline_mi_gradient_f32(self.h, ptr(fixed), C.byref(fixed_geom), ptr(moving), C.byref(moving_geom),
                                                 C.byref(virtual_geom), int(stride), ptr(fixed_mask), ptr(moving_mask), ptr(coefficients),
                                                 C.byref(lattice_geom), float(jitter_bound), C.byref(bins),
                                                 tab.ctypes.data_as(C.POINTER(C.c_double)), st, grad.ctypes.data_as(C.POINTER(C.c_double)))
        if rc:
            self._bspline_raise("pp_bspline_mi_gradient_f32", rc)
        return grad, {"valid": st[0], "outside": st[1], "masked": st[2], "seen": st[3]}

    def bspline_metric(self, metric, fixed, fixed_geom, moving, moving_geom, virtual_geom, stride, coefficients, lattice_geom,
                       fixed_mask=None, moving_mask=None, jitter_bound=0.0):
        """pp_bspline_metric_f32 -> (value, float64 gradient [3 cx cy cz] in ITK's parameter order, stats dict).  Raises
        PlatipyAmdError with .code (ERR_DIRECTION, ERR_NO_OVERLAP, ...)."""
        n = self._bspline_buffer_check("bspline_metric", fixed, fixed_geom, moving, moving_geom, fixed_mask, moving_mask, coefficients,
                                       lattice_geom)
        grad = np.zeros(n, dtype=np.float64)
        value = C.c_double()
        st = (C.c_double * 4)()
        rc = self.lib.pp_bspline_metric_f32(self.h, int(metric), ptr(fixed), C.byref(fixed_geom), ptr(moving), C.byref(moving_geom),
                                            C.byref(virtual_geom), int(stride), ptr(fixed_mask), ptr(moving_mask), ptr(coefficients),
                                            C.byref(lattice_geom), float(jitter_bound), C.byref(value), st,
                                            grad.ctypes.data_as(C.POINTER(C.c_double)))
        if rc:
            msg = self.lib.pp_last_error(self.h)
            err = PlatipyAmdError(f"pp_bspline_metric_f32 failed ({rc}): {msg.decode(errors='replace') if msg else ''}")
            err.code = rc
            raise err
        return value.value, grad, {"valid": st[0], "outside": st[1], "masked": st[2], "seen": st[3]}

    def compose_field(self, total, it, geom):
        self._chk(self.lib.pp_compose_field_f32(self.h, ptr(total), ptr(it), C.byref(geom)), "pp_compose_field_f32")

    # -- demons ---------------------------------------------------------------------
    def demons_force(self, fixed, warped, geom, params, update, want_stats=True):
        st = DemonsStats()
        self._chk(self.lib.pp_demons_force_f32(self.h, ptr(fixed), ptr(warped), C.byref(geom), C.byref(params), ptr(update),
                                               C.byref(st) if want_stats else None), "pp_demons_force_f32")
        return st if want_stats else None

    def demons_execute(self, fixed, moving, geom, params, field, want_stats=True):
        st = DemonsStats()
        self._chk(self.lib.pp_demons_execute_f32(self.h, ptr(fixed), ptr(moving), C.byref(geom), C.byref(params), ptr(field),
                                                 C.byref(st) if want_stats else None), "pp_demons_execute_f32")
        return st if want_stats else None

    def demons_history(self, cap=4096):
        """-> [(metric, rms_change)] per iteration of the last demons_execute on this context (an sitkIterationEvent
        observer's view of the filter, deformable.py:260-264)."""
        m, r = (C.c_double * cap)(), (C.c_double * cap)()
        n = self.lib.pp_demons_history(self.h, m, r, cap)
        self._chk(n if n < 0 else 0, "pp_demons_history")
        kept = min(n, cap, HISTORY_CAPACITY)
        if n > kept:
            import warnings

            warnings.warn(f"demons_history: {n} iterations ran, the device ring keeps the first {HISTORY_CAPACITY}; "
                          f"{n - kept} later iterations have no recorded metric / RMS change", RuntimeWarning)
        self.last_history_iterations = n     # iterations that ran (may exceed the number of entries)
        return [(m[k], r[k]) for k in range(kept)]

    # -- fusion ---------------------------------------------------------------------
    def weight_map_local(self, target, moving, size, spacing, sigma, epsilon, out):
        self._chk(self.lib.pp_weight_map_local_f32(self.h, ptr(target), ptr(moving), _i3(size), _d3(spacing), float(sigma),
                                                   float(epsilon), ptr(out)), "pp_weight_map_local_f32")

    def weight_map_block(self, target, moving, size, radius, factor, gain, weight):
        self._chk(self.lib.pp_weight_map_block_f32(self.h, ptr(target), ptr(moving), _i3(size), _i3(radius), float(factor), float(gain),
                                                   ptr(weight)), "pp_weight_map_block_f32")

    def sum_sq_diff(self, a, b, n):
        r = C.c_double()
        self._chk(self.lib.pp_sum_sq_diff_f32(self.h, ptr(a), ptr(b), int(n), C.byref(r)), "pp_sum_sq_diff_f32")
        return r.value

    def fuse_accumulate(self, weight, label, wsum, wlsum, n):
        """wsum += w; wlsum += w * label.  `label` is uint8 (masks) or float32 (probabilistic labels)."""
        if getattr(label, "dtype", None) is not None and str(label.dtype).endswith("float32"):
            self._chk(self.lib.pp_fuse_accumulate_f32(self.h, ptr(weight), ptr(label), ptr(wsum), ptr(wlsum), int(n)),
                      "pp_fuse_accumulate_f32")
        else:
            self._chk(self.lib.pp_fuse_accumulate_u8(self.h, ptr(weight), ptr(label), ptr(wsum), ptr(wlsum), int(n)),
                      "pp_fuse_accumulate_u8")

    def fuse_divide(self, wlsum, wsum, out, n):
        self._chk(self.lib.pp_fuse_divide_f32(self.h, ptr(wlsum), ptr(wsum), ptr(out), int(n)), "pp_fuse_divide_f32")

    def minmax(self, src, n):
        lo, hi = C.c_float(), C.c_float()
        self._chk(self.lib.pp_minmax_f32(self.h, ptr(src), int(n), C.byref(lo), C.byref(hi)), "pp_minmax_f32")
        return lo.value, hi.value

    def rescale_threshold(self, data, n, in_min, in_max, lower):
        self._chk(self.lib.pp_rescale_threshold_f32(self.h, ptr(data), int(n), float(in_min), float(in_max), float(lower)),
                  "pp_rescale_threshold_f32")

    def binary_threshold(self, prob, n, max_value, threshold, out):
        self._chk(self.lib.pp_binary_threshold_f32(self.h, ptr(prob), int(n), float(max_value), float(threshold), ptr(out)),
                  "pp_binary_threshold_f32")

    def fillhole_largest_component(self, mask, size, out, fill_holes=True, want_count=False):
        n = C.c_int64(0)
        self._chk(self.lib.pp_fillhole_largest_component_u8(self.h, ptr(mask), _i3(size), int(bool(fill_holes)), ptr(out),
                                                            C.byref(n) if want_count else None), "pp_fillhole_largest_component_u8")
        return n.value if want_count else None

    def binary_morph_ball(self, mask, size, radius, op, out):
        """op: 0 dilate, 1 erode, 2 closing (safe border); ITK ball of `radius` voxels (x, y, z)."""
        self._chk(self.lib.pp_binary_morph_ball_u8(self.h, ptr(mask), _i3(size), _i3(radius), int(op), ptr(out)),
                  "pp_binary_morph_ball_u8")

    def bounding_box(self, data, size, is_float):
        """-> [xmin, xmax, ymin, ymax, zmin, zmax] of the voxels > 0 (xmin > xmax when there are none)."""
        box = (C.c_int * 6)()
        self._chk(self.lib.pp_bounding_box(self.h, ptr(data), 1 if is_float else 0, _i3(size), box), "pp_bounding_box")
        return [box[i] for i in range(6)]

    def staple(self, labels, is_float, n, out, foreground_test, foreground_value=1.0, confidence_weight=1.0,
               maximum_iterations=None, rescale=False, threshold_lower=float("-inf")):
        """pp_staple_fuse over `labels` (uint8, or float32 when is_float) -> StapleResult; W (fp64) into `out`.
        maximum_iterations None = until convergence."""
        prm = StapleParams(int(foreground_test), int(bool(rescale)), float(foreground_value), float(confidence_weight),
                           (1 << 64) - 1 if maximum_iterations is None else int(maximum_iterations), float(threshold_lower))
        ptrs = (_P * len(labels))(*[ptr(x) for x in labels])
        res = StapleResult()
        self._chk(self.lib.pp_staple_fuse(self.h, ptrs, 1 if is_float else 0, len(labels), int(n), C.byref(prm), ptr(out),
                                          C.byref(res)), "pp_staple_fuse")
        return res

    def patch_correlation(self, target, moving, size, window, out):
        """pp_patch_correlation_f32: per-voxel Pearson r over a `window` (x, y, z voxels) clipped to the image.  ValueError
        for a window that leaves a single voxel in a patch (every axis <= 2)."""
        rc = self.lib.pp_patch_correlation_f32(self.h, ptr(target), ptr(moving), _i3(size), _i3(window), ptr(out))
        if rc == ERR_SIZE:
            msg = self.lib.pp_last_error(self.h)
            raise ValueError(msg.decode(errors="replace") if msg else "pp_patch_correlation_f32: unsupported window or volume size")
        self._chk(rc, "pp_patch_correlation_f32")

    def joint_histogram(self, a, b, n, bins_a, bins_b):
        """pp_joint_histogram_f32 -> (int64 counts [bins_a, bins_b], (amin, amax, bmin, bmax)): np.histogram2d's table and
        outer edges (synchronises).  ValueError for NaN / infinite samples or an argument the library rejects."""
        hist = np.zeros((int(bins_a), int(bins_b)), dtype=np.int64)
        rng = (C.c_double * 4)()
        rc = self.lib.pp_joint_histogram_f32(self.h, ptr(a), ptr(b), int(n), int(bins_a), int(bins_b),
                                             hist.ctypes.data_as(C.POINTER(C.c_int64)), rng)
        if rc == ERR_ARG:
            msg = self.lib.pp_last_error(self.h)
            raise ValueError(msg.decode(errors="replace") if msg else "pp_joint_histogram_f32: bad argument")
        self._chk(rc, "pp_joint_histogram_f32")
        return hist, tuple(rng)

    # -- dose ---------------------------------------------------------------------
    def _chk_value(self, rc, what):
        """ValueError for an argument the library refuses (PP_ERR_ARG, PP_ERR_SIZE), PlatipyAmdError for anything else."""
        if rc in (ERR_ARG, ERR_SIZE):
            msg = self.lib.pp_last_error(self.h)
            raise ValueError(msg.decode(errors="replace") if msg else f"{what}: bad argument")
        self._chk(rc, what)

    def dose_histogram(self, dose, labels, n, edges):
        """pp_dose_histogram_f32 over the uint8 masks `labels` -> (int64 counts [len(labels), len(edges) - 1], a
        DOSE_STATS_DTYPE record per label): np.histogram(dose[mask != 0], bins=edges) and count, mask-value sum, dose sum,
        min and max of each mask (synchronises).  ValueError for a NaN dose inside a mask, more than DOSE_MAX_LABELS labels or
        DOSE_MAX_BINS bins, edges that decrease."""
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        nbins = max(int(e.size) - 1, 0)
        hist = np.zeros((len(labels), nbins), dtype=np.int64)
        stats = np.zeros(len(labels), dtype=DOSE_STATS_DTYPE)
        ptrs = (_P * max(len(labels), 1))(*[ptr(x) for x in labels])
        rc = self.lib.pp_dose_histogram_f32(self.h, ptr(dose), ptrs, len(labels), int(n), e.ctypes.data_as(C.POINTER(C.c_double)), nbins,
                                            hist.ctypes.data_as(C.POINTER(C.c_int64)), stats.ctypes.data)
        self._chk_value(rc, "pp_dose_histogram_f32")
        return hist, stats

    def masked_order_stats(self, dose, label, n, ranks):
        """pp_masked_order_stats_f32 -> float32 array: the ranks[j]-th smallest (0-based) dose inside the uint8 mask, any
        number of ranks (eight per call).  ValueError for an empty mask, a rank >= its count, a NaN inside it."""
        ranks = [int(r) for r in ranks]
        out = np.zeros(len(ranks), dtype=np.float32)
        for k in range(0, len(ranks), ORDER_STATS_MAX_RANKS):
            part = ranks[k:k + ORDER_STATS_MAX_RANKS]
            res = (C.c_float * len(part))()
            rc = self.lib.pp_masked_order_stats_f32(self.h, ptr(dose), ptr(label), int(n), (C.c_int64 * len(part))(*part), len(part), res)
            self._chk_value(rc, "pp_masked_order_stats_f32")
            out[k:k + len(part)] = np.frombuffer(res, dtype=np.float32)
        return out

    def masked_count_ge(self, dose, labels, n, thresholds):
        """pp_masked_count_ge_f32 -> int64 [len(labels), len(thresholds)]: voxels of each uint8 mask with dose >= threshold,
        the thresholds rounded to float32 and compared as float32 (synchronises)."""
        t = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
        counts = np.zeros((len(labels), int(t.size)), dtype=np.int64)
        ptrs = (_P * max(len(labels), 1))(*[ptr(x) for x in labels])
        rc = self.lib.pp_masked_count_ge_f32(self.h, ptr(dose), ptrs, len(labels), int(n), t.ctypes.data_as(C.POINTER(C.c_float)),
                                             int(t.size), counts.ctypes.data_as(C.POINTER(C.c_int64)))
        self._chk_value(rc, "pp_masked_count_ge_f32")
        return counts

    # -- radiomics ----------------------------------------------------------------
    def masked_moments(self, image, mask, n, lo=-np.inf, hi=np.inf, centre=0.0):
        """pp_masked_moments_f32 -> (count, float64 [6]): over the voxels of the uint8 mask with lo <= v <= hi, the sums of
        v - c, |v - c|, (v - c)^2, (v - c)^3, (v - c)^4 and v^2 in fp64, bit-identical from call to call (synchronises)."""
        count = C.c_int64(0)
        sums = np.zeros(6, dtype=np.float64)
        rc = self.lib.pp_masked_moments_f32(self.h, ptr(image), ptr(mask), int(n), float(lo), float(hi), float(centre), C.byref(count),
                                            sums.ctypes.data_as(C.POINTER(C.c_double)))
        self._chk_value(rc, "pp_masked_moments_f32")
        return int(count.value), sums

    def radiomics_discretise(self, image, mask, n, edges, levels):
        """pp_radiomics_discretise_f32: levels (uint16 device memory, n voxels; torch has no uint16 arithmetic, an int16 tensor
        serves) = np.digitize(image, edges) inside the uint8 mask, 0 outside.  ValueError for a NaN, an infinity or a value
        outside the edges inside the mask, and for more than 65535 levels."""
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        have = _nbytes(levels)
        if have is not None and have != 2 * int(n):
            raise ValueError(f"pp_radiomics_discretise_f32: `levels` holds {have} bytes for {n} voxels")
        rc = self.lib.pp_radiomics_discretise_f32(self.h, ptr(image), ptr(mask), int(n), e.ctypes.data_as(C.POINTER(C.c_double)), int(e.size),
                                                  ptr(levels))
        self._chk_value(rc, "pp_radiomics_discretise_f32")

    def texture_neighbourhood(self, levels, size, ng, glcm=True, gldm=True, ngtdm=True):
        """pp_texture_neighbourhood_u16 -> dict of int64 arrays: "glcm" [13, ng, ng] (forward counts; the symmetric matrix is
        g + g.transpose(0, 2, 1)), "gldm" [ng, 27], "ngtdm_n" and "ngtdm_s" [ng, 27], those asked for (synchronises).
        ValueError for ng outside 1 ... TEXTURE_MAX_NG or a level above ng."""
        _check_volume("pp_texture_neighbourhood_u16", size, levels=(levels, 2))
        ng = int(ng)
        ok = 1 <= ng <= TEXTURE_MAX_NG          # (a refused call allocates nothing)
        out = {}
        if glcm:
            out["glcm"] = np.zeros((13, ng, ng) if ok else (0,), dtype=np.int64)
        if gldm:
            out["gldm"] = np.zeros((ng, 27) if ok else (0,), dtype=np.int64)
        if ngtdm:
            out["ngtdm_n"] = np.zeros((ng, 27) if ok else (0,), dtype=np.int64)
            out["ngtdm_s"] = np.zeros((ng, 27) if ok else (0,), dtype=np.int64)
        p = lambda k: out[k].ctypes.data_as(C.POINTER(C.c_int64)) if k in out else None  # noqa: E731
        rc = self.lib.pp_texture_neighbourhood_u16(self.h, ptr(levels), _i3(size), ng, p("glcm"), p("gldm"), p("ngtdm_n"), p("ngtdm_s"))
        self._chk_value(rc, "pp_texture_neighbourhood_u16")
        return out

    def texture_runs(self, levels, size, ng):
        """pp_texture_runs_u16 -> int64 [13, ng, max(size)]: the run-length table of every direction (synchronises)."""
        _check_volume("pp_texture_runs_u16", size, levels=(levels, 2))
        ng, nr = int(ng), max(int(s) for s in size)
        out = np.zeros((13, ng, nr) if 1 <= ng <= TEXTURE_MAX_NG else (0,), dtype=np.int64)
        rc = self.lib.pp_texture_runs_u16(self.h, ptr(levels), _i3(size), ng, nr, out.ctypes.data_as(C.POINTER(C.c_int64)))
        self._chk_value(rc, "pp_texture_runs_u16")
        return out

    # -- SIFT landmarks (DIR QA) --------------------------------------------------------
    def dog_extrema(self, gauss, size, nlevels, value_range, contrast_threshold, curvature_threshold, capacity, candidates_only=False):
        """pp_dog_extrema_f32 over one octave's stack of `nlevels` Gaussian volumes -> (count, int32 [rows, 4] = x, y, z, level,
        float64 [rows, 4] = offset x, y, z, response) with rows = min(count, capacity), in ascending (level, z, y, x)
        (synchronises)."""
        _check_volume("pp_dog_extrema_f32", (int(size[0]), int(size[1]), int(size[2]) * int(nlevels)), gauss=(gauss, 4))
        capacity = max(int(capacity), 0)
        index, values, count = np.zeros((capacity, 4), np.int32), np.zeros((capacity, 4), np.float64), C.c_int64(0)
        rc = self.lib.pp_dog_extrema_f32(self.h, ptr(gauss), _i3(size), int(nlevels), float(value_range), float(contrast_threshold),
                                         float(curvature_threshold), int(bool(candidates_only)), capacity,
                                         index.ctypes.data_as(C.POINTER(C.c_int32)), values.ctypes.data_as(C.POINTER(C.c_double)),
                                         C.byref(count))
        self._chk_value(rc, "pp_dog_extrema_f32")
        rows = min(int(count.value), capacity)
        return int(count.value), index[:rows], values[:rows]

    def sift_describe(self, gauss, size, nlevels, spacing, keypoints, descriptors):
        """pp_sift_describe_f32: descriptors (fp32 device memory [n, 768]) of the keypoints (int32 [n, 4] = x, y, z, level, a
        host array) on the stack `gauss` (synchronises)."""
        _check_volume("pp_sift_describe_f32", (int(size[0]), int(size[1]), int(size[2]) * int(nlevels)), gauss=(gauss, 4))
        kp = np.ascontiguousarray(keypoints, dtype=np.int32).reshape(-1, 4)
        have = _nbytes(descriptors)
        if have is not None and have != kp.shape[0] * 768 * 4:
            raise ValueError(f"pp_sift_describe_f32: `descriptors` holds {have} bytes for {kp.shape[0]} keypoints")
        rc = self.lib.pp_sift_describe_f32(self.h, ptr(gauss), _i3(size), int(nlevels), _d3(spacing), kp.ctypes.data_as(C.POINTER(C.c_int32)),
                                           int(kp.shape[0]), ptr(descriptors))
        self._chk_value(rc, "pp_sift_describe_f32")

    def descriptor_match(self, a, na, b, nb, length, best_index, best, second, points_a=None, points_b=None, radius=0.0):
        """pp_descriptor_match_f32: for every row of a [na, length] the nearest row of b [nb, length] (int32 device memory
        `best_index`) and the two smallest squared distances (fp32 device memory `best`, `second`); with fp64 device point lists
        only rows of b within `radius` take part.  Nothing is read back."""
        for what, buf, want in (("a", a, na * length * 4), ("b", b, nb * length * 4), ("best_index", best_index, na * 4), ("best", best, na * 4),
                                ("second", second, na * 4), ("points_a", points_a, na * 24), ("points_b", points_b, nb * 24)):
            have = None if buf is None else _nbytes(buf)
            if have is not None and have != int(want):
                raise ValueError(f"pp_descriptor_match_f32: `{what}` holds {have} bytes, {int(want)} expected")
        rc = self.lib.pp_descriptor_match_f32(self.h, ptr(a), int(na), ptr(b), int(nb), int(length), ptr(points_a), ptr(points_b), float(radius),
                                              ptr(best_index), ptr(best), ptr(second))
        self._chk_value(rc, "pp_descriptor_match_f32")

    def transform_points(self, field, geom, points):
        """pp_transform_points_f64 -> float64 [n, 3]: p + D(p) for physical points through the planar fp32 field [3, Z, Y, X] on
        `geom`; zero displacement outside the field (synchronises)."""
        _check_volume("pp_transform_points_f64", (int(geom.size[0]), int(geom.size[1]), int(geom.size[2]) * 3), field=(field, 4))
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        out = np.zeros_like(p)
        rc = self.lib.pp_transform_points_f64(self.h, ptr(field), C.byref(geom), p.ctypes.data_as(C.POINTER(C.c_double)), int(p.shape[0]),
                                              out.ctypes.data_as(C.POINTER(C.c_double)))
        self._chk_value(rc, "pp_transform_points_f64")
        return out

    # -- vessel splining ------------------------------------------------------------
    def slice_moments(self, masks, size, axis, out):
        """pp_slice_moments_u8: out (int64 device memory [len(masks)][size[axis]][4]) = {sum v, sum a v, sum b v, count} of every
        slice along `axis` (0 = x, 2 = z) of the uint8 volumes `masks`; nothing is read back.  ValueError for another axis or
        a mask count / size the library refuses."""
        ptrs = (_P * max(len(masks), 1))(*[ptr(x) for x in masks])
        self._chk_value(self.lib.pp_slice_moments_u8(self.h, ptrs, len(masks), _i3(size), int(axis), ptr(out)), "pp_slice_moments_u8")

    def tube_mask(self, points, size, spacing, origin, radius, out):
        """pp_tube_mask_u8: out (uint8 [Z][Y][X]) = 1 within `radius` mm of the polyline `points` ([n, 3] host doubles, mm), flat
        ends.  ValueError for fewer than two points or a polyline of zero length."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self._chk_value(self.lib.pp_tube_mask_u8(self.h, p.ctypes.data_as(C.POINTER(C.c_double)), int(p.shape[0]), _i3(size), _d3(spacing),
                                                 _d3(origin), float(radius), ptr(out)), "pp_tube_mask_u8")

    # -- RTSTRUCT contours -------------------------------------------------------------
    def contour_fill(self, vertices, contours, size, nstructures, out):
        """pp_contour_fill_u8: out (uint8 [nstructures][Z][Y][X], every byte written) = the XOR of the closed polygons of each
        (structure, slice).  vertices: [n, 2] int32 (x, y) pixel indices on the host; contours: (first, count, structure, z)
        rows (or a CONTOUR_DTYPE array).  ValueError for a vertex beyond +-2^24, a contour outside the vertex table, a
        structure or slice out of range, a buffer that does not hold nstructures volumes.  Synchronises."""
        if isinstance(vertices, np.ndarray) and vertices.dtype == np.int32:
            v = np.ascontiguousarray(vertices).reshape(-1, 2)
        else:
            v = np.ascontiguousarray(vertices, dtype=np.int64).reshape(-1, 2)
            if v.size and int(np.abs(v).max()) > 0x7fffffff:     # (the cast to int32 would wrap it; the library refuses the rest)
                raise ValueError(f"contour_fill: a vertex index beyond +-2^24 ({int(np.abs(v).max())})")
            v = v.astype(np.int32)
        ct = contours if isinstance(contours, np.ndarray) and contours.dtype == CONTOUR_DTYPE else \
            np.array([tuple(int(x) for x in c) for c in contours], dtype=CONTOUR_DTYPE)
        ct = np.ascontiguousarray(ct).reshape(-1)
        _check_volume("contour_fill", size)
        have = _nbytes(out)
        if have is not None and have != int(nstructures) * int(size[0]) * int(size[1]) * int(size[2]):
            raise ValueError(f"contour_fill: `out` does not hold {nstructures} volumes of {tuple(size)} ({have} bytes)")
        self._chk_value(self.lib.pp_contour_fill_u8(self.h, v.ctypes.data if v.size else None, int(v.shape[0]),
                                                    ct.ctypes.data if ct.size else None, int(ct.size), _i3(size), int(nstructures), ptr(out)),
                        "pp_contour_fill_u8")

    def contour_trace(self, masks, size, nstructures, approximate=False, with_cracks=False):
        """pp_contour_trace_u8: the closed contours of the uint8 masks [nstructures][Z][Y][X] (device memory, foreground = any
        non-zero byte) -> (vertices int32 [n, 2] of (x, y), CONTOUR_DTYPE rows, hole flags uint8), all host arrays, the rows
        ordered by (structure, z, leader) -- what contour_fill takes.  One count call and one fill call of the library: the
        extraction runs once (two read-backs), the second call copies.  with_cracks=True appends the crack count.
        ValueError for a buffer that does not hold nstructures volumes, nstructures < 1, more than 2^31 - 1 cracks.
        Synchronises."""
        _check_volume("contour_trace", size)
        have = _nbytes(masks)
        if int(nstructures) < 1:
            raise ValueError("contour_trace: at least one structure")
        if have is not None and have != int(nstructures) * int(size[0]) * int(size[1]) * int(size[2]):
            raise ValueError(f"contour_trace: `masks` does not hold {nstructures} volumes of {tuple(size)} ({have} bytes)")
        counts = (C.c_int64 * 3)()
        self._chk_value(self.lib.pp_contour_trace_u8(self.h, ptr(masks), _i3(size), int(nstructures), int(bool(approximate)), None, 0,
                                                     None, None, 0, counts), "pp_contour_trace_u8")
        nv, nc = int(counts[1]), int(counts[2])
        verts, rows, hole = np.empty((nv, 2), dtype=np.int32), np.empty(nc, dtype=CONTOUR_DTYPE), np.empty(nc, dtype=np.uint8)
        if nc:
            self._chk_value(self.lib.pp_contour_trace_u8(self.h, ptr(masks), _i3(size), int(nstructures), int(bool(approximate)),
                                                         verts.ctypes.data, nv, rows.ctypes.data, hole.ctypes.data, nc, counts),
                            "pp_contour_trace_u8")
        return (verts, rows, hole, int(counts[0])) if with_cracks else (verts, rows, hole)

    # -- region primitives ------------------------------------------------------------
    def connected_components(self, mask, size, labels, want_count=True):
        """pp_connected_components_u8: labels (int32) = sitk.ConnectedComponent of the uint8 mask, face connectivity, numbered
        in raster order of first voxels -> the number of components (synchronises), or None without want_count."""
        n = C.c_int(0)
        self._chk_value(self.lib.pp_connected_components_u8(self.h, ptr(mask), _i3(size), ptr(labels), C.byref(n) if want_count else None),
                        "pp_connected_components_u8")
        return n.value if want_count else None

    def connected_components_conn(self, mask, size, labels, fully_connected=False, want_count=True):
        """pp_connected_components_conn_u8: connected_components with a choice of connectivity (fully_connected: 26 neighbours)
        -> the number of components (synchronises), or None without want_count."""
        _check_volume("connected_components_conn", size, mask=(mask, 1), labels=(labels, 4))
        n = C.c_int(0)
        self._chk_value(self.lib.pp_connected_components_conn_u8(self.h, ptr(mask), _i3(size), int(bool(fully_connected)), ptr(labels),
                                                                 C.byref(n) if want_count else None), "pp_connected_components_conn_u8")
        return n.value if want_count else None

    def fillhole_largest_component_conn(self, mask, size, out, fill_holes=True, keep_largest=True, fully_connected=False, want_count=False):
        """pp_fillhole_largest_component_conn_u8: hole filling and / or the largest component with a choice of connectivity ->
        the kept component's voxels with want_count (synchronises), else None."""
        _check_volume("fillhole_largest_component_conn", size, mask=(mask, 1), out=(out, 1))
        n = C.c_int64(0)
        self._chk_value(self.lib.pp_fillhole_largest_component_conn_u8(self.h, ptr(mask), _i3(size), int(bool(fill_holes)), int(bool(keep_largest)),
                                                                       int(bool(fully_connected)), ptr(out), C.byref(n) if want_count else None),
                        "pp_fillhole_largest_component_conn_u8")
        return n.value if want_count else None

    def slice_convex_hull(self, mask, size, out):
        """pp_slice_convex_hull_u8: out (uint8 [Z][Y][X]) = the convex hull image of every z-slice of the uint8 mask (`out` may
        be `mask`).  ValueError for an axis longer than 65535 or a buffer that does not have the size of the volume."""
        _check_volume("slice_convex_hull", size, mask=(mask, 1), out=(out, 1))
        self._chk_value(self.lib.pp_slice_convex_hull_u8(self.h, ptr(mask), _i3(size), ptr(out)), "pp_slice_convex_hull_u8")

    def label_moments(self, labels, size, nlabels, out):
        """pp_label_moments_i32: out (int64 device memory [nlabels][10]) = {count, sum x, y, z, xx, yy, zz, xy, xz, yz} over the
        voxel indices of labels 1 ... nlabels of the int32 volume; nothing is read back."""
        self._chk_value(self.lib.pp_label_moments_i32(self.h, ptr(labels), _i3(size), int(nlabels), ptr(out)), "pp_label_moments_i32")

    def connected_threshold(self, image, size, lower, upper, seeds, out):
        """pp_connected_threshold_f32: out (uint8) = sitk.ConnectedThreshold of the float32 volume from `seeds` ([n, 3] indices
        x, y, z) -> voxels in the region (synchronises).  IndexError for a seed outside the buffer."""
        s = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
        vox = C.c_int64(0)
        rc = self.lib.pp_connected_threshold_f32(self.h, ptr(image), _i3(size), float(lower), float(upper),
                                                 s.ctypes.data_as(C.POINTER(C.c_int)), int(s.shape[0]), ptr(out), C.byref(vox))
        if rc == ERR_INVALID:
            msg = self.lib.pp_last_error(self.h)
            err = IndexError(msg.decode(errors="replace") if msg else "pp_connected_threshold_f32: seed outside the buffer")
            err.code = rc
            raise err
        self._chk_value(rc, "pp_connected_threshold_f32")
        return vox.value

    def binary_median(self, mask, size, radius, out):
        """pp_binary_median_u8: out = 1 where more than half of the (2 r + 1)^3 window (edge-replicated) of the uint8 mask is
        non-zero; radius (x, y, z) in 0 ... 2."""
        self._chk_value(self.lib.pp_binary_median_u8(self.h, ptr(mask), _i3(size), _i3(radius), ptr(out)), "pp_binary_median_u8")

    # -- left-ventricle segments ------------------------------------------------------
    def polar_sectors(self, mask, size, slices, rules, area, min_area_mm2, bits, counts):
        """pp_polar_sectors_u8: bits (uint32 [Z][Y][X]) and counts (int64 [Z][32], both device memory) from the uint8 `mask`.
        slices: one (cy, cx, theta0, radius_min, first_rule, nrules) per z-slice (or a POLAR_SLICE_DTYPE array), nrules 0 =
        skipped; rules: (label 1 ... 32, flags POLAR_CW | POLAR_ANY_AREA, angle_min, angle_max) (or a POLAR_RULE_DTYPE array).
        ValueError for a table that does not have one entry per slice and for whatever the library refuses (a label outside
        1 ... 32, a rule range outside the table, a NULL buffer, an empty volume); the outputs are then untouched."""
        st = slices if isinstance(slices, np.ndarray) and slices.dtype == POLAR_SLICE_DTYPE else np.array([tuple(v) for v in slices], dtype=POLAR_SLICE_DTYPE)
        rt = rules if isinstance(rules, np.ndarray) and rules.dtype == POLAR_RULE_DTYPE else np.array([tuple(v) for v in rules], dtype=POLAR_RULE_DTYPE)
        st, rt = np.ascontiguousarray(st).reshape(-1), np.ascontiguousarray(rt).reshape(-1)
        if len(size) != 3 or st.size != max(int(size[2]), 0):
            raise ValueError(f"polar_sectors: {st.size} slice entries for a volume of size {tuple(size)}")
        self._chk_value(self.lib.pp_polar_sectors_u8(self.h, ptr(mask), _i3(size), st.ctypes.data if st.size else None,
                                                     rt.ctypes.data if rt.size else None, int(rt.size), float(area), float(min_area_mm2),
                                                     ptr(bits), ptr(counts)), "pp_polar_sectors_u8")

    def resample_bits(self, src, gin, gout, nbits, out, affine_A=None, affine_t=None):
        """pp_resample_bits_u32: out (uint8 [nbits][Z][Y][X] on gout) plane k = bit k of the uint32 volume `src` (on gin) picked by
        nearest neighbour through q = A p + t, 0 outside; plane k equals `resample(..., interp=INTERP_NEAREST, u8=True)` of that
        bit.  ValueError for nbits outside 1 ... 32, a NULL buffer or a geometry the library refuses."""
        if affine_A is None and affine_t is not None:
            raise ValueError("resample_bits: a translation needs its matrix (pass the identity)")
        self._chk_value(self.lib.pp_resample_bits_u32(self.h, ptr(src), C.byref(gin), C.byref(gout), _dn(affine_A, 9), _dn(affine_t, 3),
                                                      int(nbits), ptr(out)), "pp_resample_bits_u32")

    # -- displacement-field inverse / Jacobian ----------------------------------------
    def invert_field(self, field, geom, out, initial=None, max_iterations=10, max_tol=0.1, mean_tol=0.001, enforce_boundary=True,
                     want_stats=False):
        """pp_invert_field_f32: out (planar fp32 [3, Z, Y, X]) = the iterative inverse of `field` on `geom`, from `initial` or 0.
        want_stats: -> {"iterations", "max_error_norm", "mean_error_norm"} of the last executed iteration (synchronises);
        otherwise None and the call only enqueues work.  ValueError for what the library refuses as an argument."""
        _check_volume("invert_field", geom.size, field=(field, 12), out=(out, 12), initial=(initial, 12))
        st = InvertStats()
        self._chk_value(self.lib.pp_invert_field_f32(self.h, ptr(field), C.byref(geom), ptr(initial), int(max_iterations), float(max_tol),
                                                     float(mean_tol), int(bool(enforce_boundary)), ptr(out),
                                                     C.byref(st) if want_stats else None), "pp_invert_field_f32")
        if not want_stats:
            return None
        return {"iterations": int(st.iterations), "max_error_norm": float(st.max_error_norm), "mean_error_norm": float(st.mean_error_norm)}

    def inverse_consistency(self, field, inverse, geom, norm_out=None):
        """pp_inverse_consistency_f32 -> {"max", "mean"} of the scaled residual norm of `inverse` against `field`; norm_out (fp32
        [Z, Y, X]) receives the norm image when given.  Synchronises."""
        _check_volume("inverse_consistency", geom.size, field=(field, 12), inverse=(inverse, 12), norm_out=(norm_out, 4))
        st = InvertStats()
        self._chk_value(self.lib.pp_inverse_consistency_f32(self.h, ptr(field), ptr(inverse), C.byref(geom), ptr(norm_out), C.byref(st)),
                        "pp_inverse_consistency_f32")
        return {"max": float(st.max_error_norm), "mean": float(st.mean_error_norm)}

    def jacobian_determinant(self, field, geom, out, use_image_spacing=True, mask=None, want_stats=False):
        """pp_jacobian_determinant_f32: out (fp32 [Z, Y, X], or None with want_stats) = det(I + grad u).  want_stats: ->
        {"min", "max", "mean", "count", "count_nonpositive"} over `mask` (uint8) or the whole image, from the same pass
        (synchronises); otherwise None."""
        _check_volume("jacobian_determinant", geom.size, field=(field, 12), out=(out, 4), mask=(mask, 1))
        st = JacobianStats()
        self._chk_value(self.lib.pp_jacobian_determinant_f32(self.h, ptr(field), C.byref(geom), int(bool(use_image_spacing)), ptr(mask),
                                                             ptr(out), C.byref(st) if want_stats else None), "pp_jacobian_determinant_f32")
        if not want_stats:
            return None
        return {"min": float(st.min), "max": float(st.max), "mean": float(st.mean), "count": int(st.count),
                "count_nonpositive": int(st.count_nonpositive)}

    def label_contour(self, mask, size, out):
        self._chk(self.lib.pp_label_contour_u8(self.h, ptr(mask), _i3(size), ptr(out)), "pp_label_contour_u8")

    def distance_map(self, mask, geom, out, signed=False, inside_positive=False):
        self._chk(self.lib.pp_distance_map_f32(self.h, ptr(mask), C.byref(geom), int(bool(signed)), int(bool(inside_positive)),
                                               ptr(out)), "pp_distance_map_f32")

    # -- label comparison ----------------------------------------------------------
    def overlap_counts(self, a, b, n):
        """-> (|A|, |B|, |A and B|) of two uint8 masks, non-zero = foreground (synchronises)."""
        c = (C.c_int64 * 3)()
        self._chk(self.lib.pp_overlap_counts_u8(self.h, ptr(a), ptr(b), int(n), c), "pp_overlap_counts_u8")
        return c[0], c[1], c[2]

    def binary_contour(self, mask, size, out, fully_connected=True):
        self._chk(self.lib.pp_binary_contour_u8(self.h, ptr(mask), _i3(size), int(bool(fully_connected)), ptr(out)),
                  "pp_binary_contour_u8")

    def slice_contour(self, mask, size, out):
        self._chk(self.lib.pp_slice_contour_u8(self.h, ptr(mask), _i3(size), ptr(out)), "pp_slice_contour_u8")

    def abs_range(self, src, n, device_range):
        """min / max of |src| into `device_range` (2 floats in device memory); nothing is read back."""
        self._chk(self.lib.pp_abs_range_f32(self.h, ptr(src), int(n), ptr(device_range)), "pp_abs_range_f32")

    def surface_stats(self, select, dist, geom, mode, out, tau=0.0, device_range=None):
        """pp_surface_stats_f32 into `out`: SURFACE_STATS_DTYPE.itemsize bytes of device memory, 8-byte aligned (an address or
        a buffer); nothing is read back."""
        self._chk(self.lib.pp_surface_stats_f32(self.h, ptr(select), ptr(dist), C.byref(geom), int(mode), float(tau),
                                                ptr(device_range), ptr(out)), "pp_surface_stats_f32")

    def slice_masked_count(self, a, not_b, size, per_slice):
        """per_slice[z] (int64, device memory) = voxels of slice z with a != 0 and not_b == 0 (not_b None: with a != 0)."""
        self._chk(self.lib.pp_slice_masked_count_u8(self.h, ptr(a), ptr(not_b), _i3(size), ptr(per_slice)),
                  "pp_slice_masked_count_u8")

    def meansq_affine(self, fixed, fsize, moving, msize, Af, bf, Am, bm, vsize, stride, fixed_mask=None, moving_mask=None):
        """-> (sum sq diff, count, dAm[9], dbm[3]) as a list of 14 floats."""
        res = (C.c_double * 14)()
        self._chk(self.lib.pp_meansq_affine_f32(self.h, ptr(fixed), _i3(fsize), ptr(moving), _i3(msize), _dn(Af, 9), _dn(bf, 3),
                                                _dn(Am, 9), _dn(bm, 3), _i3(vsize), int(stride), ptr(fixed_mask),
                                                ptr(moving_mask), res), "pp_meansq_affine_f32")
        return [res[i] for i in range(14)]

    def metric_values_affine(self, metric, fixed, fsize, moving, msize, Af, bf, Ams, bms, vsize, stride, fixed_mask=None,
                             moving_mask=None):
        """Values only for len(Ams) <= 16 candidate maps in one launch -> array [ncand, 6] (pp_metric_values_affine_f32)."""
        import numpy as np

        k = len(Ams)
        am = np.ascontiguousarray(np.asarray(Ams, dtype=np.float64).reshape(k, 9))
        bm = np.ascontiguousarray(np.asarray(bms, dtype=np.float64).reshape(k, 3))
        res = np.zeros((k, 6), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.pp_metric_values_affine_f32(self.h, int(metric), ptr(fixed), _i3(fsize), ptr(moving), _i3(msize), _dn(Af, 9),
                                                       _dn(bf, 3), k, am.ctypes.data_as(dp), bm.ctypes.data_as(dp), _i3(vsize),
                                                       int(stride), ptr(fixed_mask), ptr(moving_mask), res.ctypes.data_as(dp)),
                  "pp_metric_values_affine_f32")
        return res

    def set_sample_jitter(self, jitter):
        """ITK's per-sample jitter for the metric entry points (pp_linear_set_sample_jitter): a contiguous float32 device
        tensor [nsamples, 3] in virtual-index units, kept alive by this context until replaced; None restores the lattice."""
        if jitter is None:
            self._chk(self.lib.pp_linear_set_sample_jitter(self.h, None, 0), "pp_linear_set_sample_jitter")
        else:
            shape, dtype = tuple(jitter.shape), str(jitter.dtype).replace("torch.", "")
            contiguous = jitter.is_contiguous() if hasattr(jitter, "is_contiguous") else jitter.flags["C_CONTIGUOUS"]
            if len(shape) != 2 or shape[1] != 3 or dtype != "float32" or not contiguous:
                raise ValueError("set_sample_jitter: a contiguous float32 array [nsamples, 3]")
            self._chk(self.lib.pp_linear_set_sample_jitter(self.h, ptr(jitter), int(jitter.shape[0])), "pp_linear_set_sample_jitter")
        self._sample_jitter = jitter

    def set_moving_gradient(self, gradient, msize=None, packed=None):
        """ITK's filtered gradient image for the gradient-bearing metric entry points (pp_linear_set_moving_gradient): a
        contiguous float32 device tensor [3, Z, Y, X] in moving-index units, kept alive by this context until replaced; None
        restores the interpolant's analytic gradient.  `packed`: optionally the same image with the intensity, float32
        [Z, Y, X, 4] = (gx, gy, gz, m) (pp_linear_set_moving_gradient_packed)."""
        self._moving_gradient_packed = None
        if gradient is None:
            self._chk(self.lib.pp_linear_set_moving_gradient(self.h, None, None), "pp_linear_set_moving_gradient")
        else:
            shape = tuple(gradient.shape)
            if len(shape) != 4 or shape[0] != 3 or str(gradient.dtype).replace("torch.", "") != "float32":
                raise ValueError("set_moving_gradient: a float32 array [3, Z, Y, X]")
            size = msize if msize is not None else (shape[3], shape[2], shape[1])
            self._chk(self.lib.pp_linear_set_moving_gradient(self.h, ptr(gradient), _i3(size)), "pp_linear_set_moving_gradient")
            if packed is not None:
                if tuple(packed.shape) != shape[1:] + (4,) or str(packed.dtype).replace("torch.", "") != "float32":
                    raise ValueError("set_moving_gradient: `packed` must be a float32 array [Z, Y, X, 4]")
                self._chk(self.lib.pp_linear_set_moving_gradient_packed(self.h, ptr(packed)), "pp_linear_set_moving_gradient_packed")
                self._moving_gradient_packed = packed
        self._moving_gradient = gradient

    def recursive_gaussian_pass(self, src, dst, geom, axis, sigma, order=0, normalize_across_scale=False):
        """One directional pass of itk::RecursiveGaussianImageFilter (pp_recursive_gaussian_pass_f32): order 0 / 1 along `axis`."""
        self._chk(self.lib.pp_recursive_gaussian_pass_f32(self.h, ptr(src), ptr(dst), C.byref(geom), int(axis), float(sigma), int(order),
                                                          int(bool(normalize_across_scale))), "pp_recursive_gaussian_pass_f32")

    def linear_optimize(self, fixed, fsize, moving, msize, level, params, fixed_mask=None, moving_mask=None, history=0):
        """One level of linear_registration's optimisation in the library (pp_linear_optimize_f32).
        -> (params list, LinregStats, history list).  Raises PlatipyAmdError; .code == ERR_NO_OVERLAP when the images
        do not overlap at the start."""
        n = self.lib.pp_linear_num_parameters(int(level.model))
        p = (C.c_double * n)(*[float(v) for v in params])
        st = LinregStats()
        hist = (C.c_double * max(1, int(history)))()
        rc = self.lib.pp_linear_optimize_f32(self.h, ptr(fixed), _i3(fsize), ptr(moving), _i3(msize), ptr(fixed_mask), ptr(moving_mask),
                                             C.byref(level), p, C.byref(st), hist, int(history))
        if rc:
            msg = self.lib.pp_last_error(self.h)
            err = PlatipyAmdError(f"pp_linear_optimize_f32 failed ({rc}): {msg.decode(errors='replace') if msg else ''}")
            err.code = rc
            raise err
        return [p[i] for i in range(n)], st, [hist[i] for i in range(min(int(history), st.iterations))]

    def mi_histogram(self, fixed, fsize, moving, msize, Af, bf, Am, bm, vsize, stride, bins, fixed_mask=None, moving_mask=None):
        """Joint intensity histogram of the valid sample pairs -> (hist [nbins, nbins] float64, row = fixed bin; count)."""
        hist = np.zeros((bins.nbins, bins.nbins), dtype=np.float64)
        count = C.c_double()
        self._chk(self.lib.pp_mi_histogram_f32(self.h, ptr(fixed), _i3(fsize), ptr(moving), _i3(msize), _dn(Af, 9), _dn(bf, 3), _dn(Am, 9),
                                               _dn(bm, 3), _i3(vsize), int(stride), ptr(fixed_mask), ptr(moving_mask), C.byref(bins),
                                               hist.ctypes.data_as(C.POINTER(C.c_double)), C.byref(count)), "pp_mi_histogram_f32")
        return hist, count.value

    def mi_gradient(self, fixed, fsize, moving, msize, Af, bf, Am, bm, vsize, stride, bins, table, fixed_mask=None, moving_mask=None):
        """sum_s w_s g_s (v_q | 1) with w_s from the score `table` [nbins, nbins] -> 12 floats (d/dAm row-major 9, d/dbm 3)."""
        tab = np.ascontiguousarray(table, dtype=np.float64)
        res = (C.c_double * 12)()
        self._chk(self.lib.pp_mi_gradient_f32(self.h, ptr(fixed), _i3(fsize), ptr(moving), _i3(msize), _dn(Af, 9), _dn(bf, 3), _dn(Am, 9),
                                              _dn(bm, 3), _i3(vsize), int(stride), ptr(fixed_mask), ptr(moving_mask), C.byref(bins),
                                              tab.ctypes.data_as(C.POINTER(C.c_double)), res), "pp_mi_gradient_f32")
        return np.array([res[i] for i in range(12)])

    def corr_moments_affine(self, fixed, fsize, moving, msize, Af, bf, Am, bm, vsize, stride, fixed_mask=None, moving_mask=None):
        """-> the 42 raw moments of pp_corr_moments_affine_f32."""
        res = (C.c_double * 42)()
        self._chk(self.lib.pp_corr_moments_affine_f32(self.h, ptr(fixed), _i3(fsize), ptr(moving), _i3(msize), _dn(Af, 9), _dn(bf, 3),
                                                      _dn(Am, 9), _dn(bm, 3), _i3(vsize), int(stride), ptr(fixed_mask),
                                                      ptr(moving_mask), res), "pp_corr_moments_affine_f32")
        return [res[i] for i in range(42)]
