/*
 * include/platipy_amd.h -- C ABI of libplatipy_hip.so (gfx950 / MI355X).
 *
 * The reference (pyplati/platipy) has no C/FFI boundary on this path: its L2 Python functions
 * call SimpleITK (SWIG -> ITK C++) directly.  This header is therefore the boundary a
 * maintainer would bind *instead of* those SimpleITK calls; every entry point names the
 * reference call site (file:line under the reference tree) whose SimpleITK call it replaces.
 * platipy_amd/_lib.py is the ctypes binding; INTEGRATION.md shows the reference-side stub.
 *
 * Rules of the ABI
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - All volume pointers are caller-owned DEVICE pointers (e.g. torch tensor data_ptr());
 *    the library never frees or retains them past the call.  Scratch memory belongs to the
 *    ctx and grows on demand (hipMalloc only when a call needs more than any earlier one).
 *  - Every call enqueues on the ctx's stream and returns; pp_sync() waits.  The one
 *    exception is a call given a non-NULL host `stats` pointer, which synchronises the
 *    stream before returning so the statistics are valid.
 *  - Return value: PP_OK (0) or a negative pp_status; pp_last_error(ctx) describes the last
 *    failure.  Nothing throws across the ABI and nothing calls exit().
 *  - One ctx per (device, stream); no global state, so N ctxs can drive N GPUs/streams.
 *
 * Layout: scalar volumes are [Z][Y][X] (x fastest), size = {nx, ny, nz}.  Displacement
 * fields are planar fp32, [3][Z][Y][X]; plane c holds the c-th physical (mm) component.
 */
#ifndef PLATIPY_AMD_H
#define PLATIPY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_ABI_VERSION 6

typedef enum {
  PP_OK = 0,
  PP_ERR_ARG = -1,         /* NULL / inconsistent argument                       */
  PP_ERR_HIP = -2,         /* a HIP runtime call or kernel launch failed          */
  PP_ERR_ALLOC = -3,       /* workspace allocation failed                         */
  PP_ERR_UNSUPPORTED = -4, /* valid request this build does not implement         */
  PP_ERR_SIZE = -5,        /* volume too small / too large for the operation      */
  PP_ERR_NO_OVERLAP = -6,  /* linear registration: no valid sample point at start */
  PP_ERR_DIRECTION = -7,   /* B-spline metric: lattice / virtual / fixed direction cosines differ */
  PP_ERR_INVALID = -8      /* a value that points outside the data it refers to (a seed outside the buffer) */
} pp_status;

enum { PP_INTERP_NEAREST = 1, PP_INTERP_LINEAR = 2, PP_INTERP_BSPLINE = 3 }; /* = sitk.sitkNearestNeighbor / sitkLinear / sitkBSpline */
enum { PP_MORPH_DILATE = 0, PP_MORPH_ERODE = 1, PP_MORPH_CLOSE = 2 };
enum { PP_DTYPE_U8 = 0, PP_DTYPE_F32 = 1 };

enum { PP_DEMONS_AUTO = 0, PP_DEMONS_STAGED = 1, PP_DEMONS_FUSED = 2 };

typedef struct pp_ctx pp_ctx;

typedef struct {
  int size[3];         /* nx, ny, nz */
  double spacing[3];   /* mm         */
  double origin[3];    /* mm         */
  double direction[9]; /* row-major  */
} pp_geom;

/* Parameters of sitk.FastSymmetricForcesDemonsRegistrationFilter as the reference
 * configures it (registration/deformable.py:244-257); pp_demons_default_params() fills
 * SimpleITK 2.3.1's defaults. */
typedef struct {
  int iterations;               /* SetNumberOfIterations (deformable.py:144)              */
  double sigma_d_vox[3];        /* SetStandardDeviations, voxels (deformable.py:253-257)  */
  double sigma_u_vox[3];        /* UpdateFieldStandardDeviations, voxels (default 1.0)    */
  int smooth_displacement;      /* SetSmoothDisplacementField (deformable.py:249)         */
  int smooth_update;            /* SetSmoothUpdateField (deformable.py:248)               */
  double max_rms_error;         /* MaximumRMSError, 0.02; <= 0 disables the early halt    */
  double max_step_length;       /* MaximumUpdateStepLength, 0.5                           */
  double intensity_threshold;   /* IntensityDifferenceThreshold, 0.001                    */
  double denominator_threshold; /* ESM m_DenominatorThreshold, 1e-9                       */
  double max_error;             /* GaussianOperator MaximumError, 0.1                     */
  int max_kernel_width;         /* GaussianOperator MaximumKernelWidth, 30                */
  int variant;                  /* PP_DEMONS_AUTO | _STAGED | _FUSED                      */
} pp_demons_params;

typedef struct {
  double metric;         /* GetMetric(): mean squared intensity difference            */
  double rms_change;     /* GetRMSChange(): sqrt(mean |update|^2), raw update         */
  double sum_sq_diff;
  double sum_sq_change;
  int64_t n_pixels;
  int elapsed_iterations; /* GetElapsedIterations()                                   */
  int halted;             /* 1 if the RMS rule stopped the loop early                 */
} pp_demons_stats;

/* ---- context --------------------------------------------------------------------- */
int pp_abi_version(void);
/* The PP_* measurement / debugging switches are read from the process environment ONCE, when the library
 * first needs one; launch paths never call getenv.  pp_reload_switches() takes the snapshot again -- for tests and A/B tools
 * that flip a switch inside one process; not while another thread is inside the library.  (No reference counterpart.) */
void pp_reload_switches(void);
int pp_create(int device, void* hip_stream, pp_ctx** out);
void pp_destroy(pp_ctx* ctx);
const char* pp_last_error(const pp_ctx* ctx);
/* Every operation is asynchronous on the context's stream; the context's scratch, ticket counters and mailbox are shared by
 * all of them.  pp_set_stream therefore WAITS (hipStreamSynchronize) for everything the context has queued on its current
 * stream before it binds the new one, so work on the new stream never meets scratch that work on the old one still uses;
 * setting the stream the context already has is free.  Results already queued keep their meaning: they are complete when
 * the call returns.  The stream bound so far must therefore still be ALIVE when pp_set_stream is called: rebind first,
 * destroy the old stream afterwards (a destroyed handle makes the wait fail with PP_ERR_HIP, or worse).  (No reference
 * counterpart.) */
int pp_set_stream(pp_ctx* ctx, void* hip_stream);
int pp_sync(pp_ctx* ctx);
size_t pp_workspace_bytes(const pp_ctx* ctx);

/* Optional per-kernel timing with HIP events recorded on the ctx stream around every kernel
 * launch of the demons loop (bench.py's roofline figures).  Off by default: when off no event
 * is created or recorded.  `on` = 1 brackets every launch, `on` = k > 1 every k-th launch of each
 * kernel (a pair of events costs the stream ~7 us); `launches` counts the bracketed ones.
 * pp_profile_read synchronises, returns the number of distinct kernels (<= cap entries written)
 * and resets the accumulators. */
typedef struct {
  char name[48];
  int launches;
  double total_ms;
} pp_profile_entry;
int pp_profile_enable(pp_ctx* ctx, int on);
int pp_profile_read(pp_ctx* ctx, pp_profile_entry* out, int cap);

/* ---- host helpers ---------------------------------------------------------------- */
/* itk::GaussianOperator coefficients (every FIR below uses them).  taps gets 2r+1 values,
 * returns r or a negative pp_status. */
int pp_gauss_taps(double variance, double max_error, int max_kernel_width, double* taps, int cap);
void pp_demons_default_params(pp_demons_params* p);

/* ---- Gaussian FIR ------------------------------------------------------------------ */
/* sitk.DiscreteGaussian(image, variance, maximumKernelWidth, maximumError=0.01,
 * useImageSpacing=True): registration/utils.py:226, label/fusion.py:168,279. */
int pp_discrete_gaussian_f32(pp_ctx* ctx, const float* in, float* out, const int size[3],
                             const double spacing[3], const double variance[3], double max_error,
                             int max_kernel_width, int use_image_spacing);
/* The same filter when only rows (y, z) with need_y[y] && need_z[z] (device uint8 masks of ny / nz entries) of the
 * result will be read -- the pyramid's blur is followed by a resample onto a coarser grid (registration/utils.py:226,
 * :257-267).  Values that are produced equal the dense filter's bit for bit; other entries of out are unspecified. */
int pp_discrete_gaussian_rows_f32(pp_ctx* ctx, const float* in, float* out, const int size[3],
                                  const double spacing[3], const double variance[3], double max_error,
                                  int max_kernel_width, int use_image_spacing, const uint8_t* need_y,
                                  const uint8_t* need_z);
/* PDEDeformableRegistrationFilter::SmoothDisplacementField / SmoothUpdateField, in place on
 * a planar 3-vector field; sigma in voxels (deformable.py:248-257). */
int pp_smooth_field_f32(pp_ctx* ctx, float* field, const int size[3], const double sigma_vox[3],
                        double max_error, int max_kernel_width);

/* ---- recursive (IIR) Gaussian ------------------------------------------------------ */
/* sitk.SmoothingRecursiveGaussian(dvf_total, sigma) (deformable.py:157-158), in place on a
 * planar field; sigma in the units ITK reads them in (mm). */
int pp_recursive_gaussian_field_f32(pp_ctx* ctx, float* field, const pp_geom* g,
                                    const double sigma[3]);
int pp_recursive_gaussian_f32(pp_ctx* ctx, const float* in, float* out, const pp_geom* g,
                              const double sigma[3]);

/* ONE directional pass of itk::RecursiveGaussianImageFilter over a scalar volume (in != out): order 0 the Gaussian, order 1 its
 * first derivative along `axis` per VOXEL (a unit ramp answers 1; times sigma when normalize_across_scale, as ITK's
 * NormalizeAcrossScale).  The spacing of `axis` may be negative: the filter uses its magnitude and the first-order response takes
 * its sign, as ITK's does (every other spacing must be positive).  The building block of itk::GradientRecursiveGaussianImageFilter -- derivative along one axis, then
 * Gaussians along the others -- which itk::ImageToImageMetricv4 runs over the moving image (sigma = its largest spacing) inside
 * registration.Execute (registration/linear.py:238) as the metric's default gradient source; the host chains the passes
 * (platipy_amd/registration/linear.py, itk_sampling=True). */
int pp_recursive_gaussian_pass_f32(pp_ctx* ctx, const float* in, float* out, const pp_geom* g, int axis, double sigma, int order,
                                   int normalize_across_scale);

/* ---- warp / resample --------------------------------------------------------------- */
/* out(x) = moving(x + D(x)), moving/field/out on one grid: itk::WarpImageFilter inside the
 * demons loop (edge = FLT_MAX sentinel) and sitk.Resample(m_image, tfm_total, interp)
 * (deformable.py:140, edge 0) / the final warp (deformable.py:281-301). */
int pp_warp_f32(pp_ctx* ctx, const float* moving, const float* field, const pp_geom* g,
                float edge_value, float* out);
/* sitk.ResampleImageFilter (registration/utils.py:176-190, :257-267): out grid gout, input
 * grid gin, transform q = A p + t (NULL = identity) followed by q += D(p) for a field D
 * sampled on gout (NULL = none).  Coordinates are computed in fp64. */
int pp_resample_f32(pp_ctx* ctx, const float* in, const pp_geom* gin, const pp_geom* gout,
                    const double* affine_A, const double* affine_t, const float* field,
                    int interp, double default_value, float* out);
int pp_resample_u8(pp_ctx* ctx, const uint8_t* in, const pp_geom* gin, const pp_geom* gout,
                   const double* affine_A, const double* affine_t, const float* field,
                   int interp, double default_value, uint8_t* out);
/* One fp32 image and nlabels uint8 label volumes, all on the grid gin, through ONE transform onto gout in one gather: what
 * apply_augmentation (generation/augment.py:65-78) and the atlas propagation (multiatlas/run.py:280-298) do with 1 + M
 * apply_transform calls.  The field is read, the point mapped, the inside test taken and the sample addresses formed once
 * per output voxel.  image (may be NULL: labels only) is sampled with image_interp = PP_INTERP_NEAREST or PP_INTERP_LINEAR,
 * image_default outside, into image_out; labels[l] (HOST array of nlabels device pointers, 0 ... 16) nearest neighbour,
 * 0 outside, into labels_out[l].  Every output equals, bit for bit, what pp_resample_f32 / pp_resample_u8 return for that
 * member alone.  PP_INTERP_BSPLINE: PP_ERR_UNSUPPORTED (callers go member by member); more than 16 labels, a negative
 * count, nothing to resample or an output that aliases its input: PP_ERR_ARG. */
#define PP_RESAMPLE_SET_MAX_LABELS 16
int pp_resample_set(pp_ctx* ctx, const pp_geom* gin, const pp_geom* gout, const double* affine_A, const double* affine_t,
                    const float* field, const float* image, int image_interp, double image_default, float* image_out,
                    const uint8_t* const* labels, int nlabels, uint8_t* const* labels_out);
/* project_onto_arbitrary_plane (visualisation/utils.py:305-368: sitk.Resample through a rotation about the volume's centre,
 * then sitk.{Sum,Mean,Median,StandardDeviation,Minimum,Maximum}Projection along an axis) for nviews transforms, one fp32
 * image and nlabels uint8 label volumes, all on the grid g, in ONE launch.  views: HOST, nviews x 12 doubles, per view the
 * row-major 3 x 3 A and then t of q = A p + t.  axis: 0 = x, 1 = y, 2 = z.  Outputs (DEVICE) are [nviews][rows][cols] with
 * the two remaining axes ordered as sitk.GetArrayFromImage orders them: axis 0 -> [nz][ny], 1 -> [nz][nx], 2 -> [ny][nx].
 * image (may be NULL: labels only) is sampled with image_interp (PP_INTERP_NEAREST or PP_INTERP_LINEAR), image_default
 * outside, and reduced with `kind` into image_out (fp32); labels[l] (HOST array of nlabels device pointers, 0 ... 16) with
 * label_interp[l] (HOST), 0 outside, reduced with max into labels_out[l] (uint8).  Every sample along a ray is, bit for bit,
 * the voxel pp_resample_f32 / pp_resample_u8 write for that member, transform and output index with gout = gin = g (the
 * default takes part in the reduction, as in the reference).  Reductions [ITK's accumulators as recalled, UNPINNED]: min, max;
 * sum = the fp64 sum in index order, mean = sum / n, std = sqrt(sum((v - mean)^2) / (n - 1)) in fp64 in index order (NaN for
 * n = 1), each rounded once to fp32; median = the element at index n / 2 of the sorted samples (std::nth_element: the upper
 * median, no averaging).  NaN samples: min, max, sum, mean and std return NaN; the median sorts every NaN last (numpy's rule),
 * so it is NaN only when more than (n - 1) / 2 samples are.  Nothing is atomic: reruns are bit-identical.  The median is a
 * radix select that re-samples the ray (nine walks, no staging chunk, no scratch that grows with the volume).
 * PP_INTERP_BSPLINE (image or label): PP_ERR_UNSUPPORTED (callers rotate member by member).  A bad axis or kind, an unknown
 * interpolator, more than 16 labels or a negative count, nothing to project, nviews < 1, a NULL table or volume, an output
 * that is an input or another output: PP_ERR_ARG.  More than 65535 output rows or views: PP_ERR_SIZE.  No error touches an
 * output.  Scratch: 304 bytes per view.  Waits for the stream once, after queueing the copy of the views (host memory of the
 * call); the kernel itself is only enqueued. */
#define PP_PROJECT_MAX_LABELS 16
enum { PP_PROJECT_SUM = 0, PP_PROJECT_MEAN = 1, PP_PROJECT_MEDIAN = 2, PP_PROJECT_STD = 3, PP_PROJECT_MIN = 4, PP_PROJECT_MAX = 5 };
int pp_project_set(pp_ctx* ctx, const pp_geom* g, int axis, const double* views, int nviews, const float* image, int kind,
                   int image_interp, double image_default, float* image_out, const uint8_t* const* labels, const int* label_interp,
                   int nlabels, uint8_t* const* labels_out);
/* itk::BSplineDecompositionImageFilter (spline order 3): samples -> B-spline coefficients, mirror boundaries; `out` may be
 * `in`.  pp_resample_f32 with interp = PP_INTERP_BSPLINE expects this coefficient volume as its input
 * (itk::BSplineInterpolateImageFunction: any sitk interpolator may reach registration/utils.py:176-190). */
int pp_bspline_prefilter_f32(pp_ctx* ctx, const float* in, const int size[3], float* out);
/* sitk.Resample on the vector field itself (deformable.py:130,137,185): linear, default 0. */
int pp_resample_field_f32(pp_ctx* ctx, const float* in, const pp_geom* gin, const pp_geom* gout,
                          float* out);
/* sitk.TransformToDisplacementField(initial_transform, sitkVectorFloat64, fixed grid) (deformable.py:101-108) for a
 * linear transform q = A p + t (fp64 coordinates): out(idx) = (A - I) p(idx) + t, plus `add_field` (planar, on the
 * same grid, may be NULL) -- the displacement part of a composite whose last member is a displacement field. */
int pp_transform_to_field_f32(pp_ctx* ctx, const pp_geom* g, const double* affine_A, const double* affine_t,
                              const float* add_field, float* out);
/* dvf_total + sitk.Resample(dvf_iter, DisplacementFieldTransform(dvf_total))
 * (deformable.py:154): total(x) += iter(x + total(x)), 0 outside; both on grid g. */
int pp_compose_field_f32(pp_ctx* ctx, float* total, const float* iter, const pp_geom* g);

/* ---- demons ------------------------------------------------------------------------ */
/* One itk::ESMDemonsRegistrationFunction::ComputeUpdate sweep (symmetric gradient) over
 * the grid: update = planar field.  stats may be NULL. */
int pp_demons_force_f32(pp_ctx* ctx, const float* fixed, const float* warped, const pp_geom* g,
                        const pp_demons_params* p, float* update, pp_demons_stats* stats);
/* registration_algorithm.Execute(f_image, m_image) (deformable.py:149): the whole inner
 * loop on device, field starting from zero.  stats may be NULL (then fully asynchronous).
 * Alignment: fixed and moving need no more than their natural 4 bytes under either variant (a view that starts at any
 * element of a larger buffer gives the bits of an aligned one).  PP_DEMONS_FUSED needs `field` on a 16-byte boundary (its
 * kernels store the field as 8- and 16-byte vectors): otherwise PP_ERR_UNSUPPORTED, "fused demons needs field on a
 * 16-byte boundary", before anything is launched; the same status with its own message says that a smoother is off or a
 * kernel radius is above 5.  PP_DEMONS_AUTO takes the staged variant in each of these cases, which accepts any 4-byte
 * aligned field; PP_DEMONS_STAGED never looks at the alignment. */
int pp_demons_execute_f32(pp_ctx* ctx, const float* fixed, const float* moving, const pp_geom* g,
                          const pp_demons_params* p, float* field, pp_demons_stats* stats);
/* What an sitkIterationEvent observer of the filter reads after every iteration -- registration_method.AddCommand(
 * sitk.sitkIterationEvent, ...) printing GetElapsedIterations() / GetMetric() (deformable.py:260-264,
 * registration/utils.py:36-41).  The loop runs on the device without host round trips, so the per-iteration values are kept
 * in a device ring by the kernel that closes each iteration and read back here: entry k = GetMetric() / GetRMSChange() after
 * iteration k + 1 of the LAST pp_demons_execute_f32 on this ctx.  Returns the number of iterations that ran, or a negative
 * pp_status; entries written: min(that, cap, PP_DEMONS_HISTORY_CAPACITY = 4096 -- the ring keeps the first 4096 iterations of an
 * Execute, a return value above it says the later ones were not recorded).  Synchronises the stream. */
#define PP_DEMONS_HISTORY_CAPACITY 4096
int pp_demons_history(pp_ctx* ctx, double* metric, double* rms_change, int cap);

/* ---- label fusion ------------------------------------------------------------------ */
/* compute_weight_map(vote_type="local") (label/fusion.py:148-169):
 * w = 1 / (DiscreteGaussian((T - M)^2, sigma^2) + epsilon). */
int pp_weight_map_local_f32(pp_ctx* ctx, const float* target, const float* moving,
                            const int size[3], const double spacing[3], double sigma,
                            double epsilon, float* weight);
/* compute_weight_map(vote_type="block") (label/fusion.py:179-190):
 * w = factor * BoxMean((T - M)^2, radius)^(-|gain / 2|), box mean with ZeroFluxNeumann edges; radius in voxels (x, y, z). */
int pp_weight_map_block_f32(pp_ctx* ctx, const float* target, const float* moving, const int size[3],
                            const int radius[3], double factor, double gain, float* weight);
/* sum of squared differences (vote_type="global", label/fusion.py:154-161), fp64 on host. */
int pp_sum_sq_diff_f32(pp_ctx* ctx, const float* a, const float* b, size_t n, double* result);
/* combine_labels accumulation (label/fusion.py:263,269-276), one atlas at a time:
 * wsum += w (if wsum != NULL);  wlsum += w * label. */
int pp_fuse_accumulate_u8(pp_ctx* ctx, const float* weight, const uint8_t* label, float* wsum,
                          float* wlsum, size_t n);
/* the same with a float label (probabilistic atlas labels: the reference casts every label to sitkFloat32 before
 * weighting, label/fusion.py:269-272, so values other than 0/1 are weighted as they are) */
int pp_fuse_accumulate_f32(pp_ctx* ctx, const float* weight, const float* label, float* wsum,
                           float* wlsum, size_t n);
/* P = wlsum / (wsum == 0 ? 1 : wsum)  (label/fusion.py:264-276) */
int pp_fuse_divide_f32(pp_ctx* ctx, const float* wlsum, const float* wsum, float* out, size_t n);
/* global min / max (RescaleIntensity, label/fusion.py:282; process_probability_image :305) */
int pp_minmax_f32(pp_ctx* ctx, const float* in, size_t n, float* min_out, float* max_out);
/* RescaleIntensity(0,1) given (min,max) then Threshold(lower, upper=1, outside=0)
 * (label/fusion.py:282-288), in place. */
int pp_rescale_threshold_f32(pp_ctx* ctx, float* data, size_t n, float in_min, float in_max,
                             float lower);
/* BinaryThreshold(prob / max_value >= threshold) -> uint8 (label/fusion.py:305-308) */
int pp_binary_threshold_f32(pp_ctx* ctx, const float* prob, size_t n, double max_value,
                            double threshold, uint8_t* out);

/* BinaryFillhole -> ConnectedComponent -> keep the largest component (label/fusion.py:310-328), face
 * connectivity.  `in`/`out` are uint8 masks (non-zero = foreground); fill_holes = 0 skips the hole filling.
 * If there is no foreground the (filled) input comes back, as the reference returns its binary image.
 * component_voxels (host, may be NULL) receives the size of the kept component; non-NULL synchronises. */
int pp_fillhole_largest_component_u8(pp_ctx* ctx, const uint8_t* in, const int size[3], int fill_holes,
                                     uint8_t* out, int64_t* component_voxels);
/* The same two steps with a choice of connectivity, each optional (generation/mask.py:77-80, "RelabelComponent(
 * ConnectedComponent(mask, True)) == 1", and :92, BinaryFillhole(fullyConnected=True)).  fully_connected = 0: faces, as
 * above; 1: two voxels are neighbours when they differ by at most 1 on every axis.  fill_holes: background components that
 * do not reach the volume border become foreground; with fully_connected = 1 the BACKGROUND flood from the border is
 * 26-connected, so a cavity that leaks through a diagonal gap is not a hole [recalled from ITK's GrayscaleFillhole,
 * unverified here; scipy's binary_fill_holes with a 3 x 3 x 3 structure states the same].  keep_largest: the largest
 * foreground component, size descending then first in raster order [sitk.RelabelComponent's order as recalled]; no
 * foreground: the (filled) input comes back.  fill_holes = keep_largest = 0 is PP_ERR_ARG; with fully_connected = 0 and
 * keep_largest = 1 the result is pp_fillhole_largest_component_u8's, bit for bit.  component_voxels needs keep_largest.
 * `out` must not alias `in`. */
int pp_fillhole_largest_component_conn_u8(pp_ctx* ctx, const uint8_t* in, const int size[3], int fill_holes, int keep_largest,
                                          int fully_connected, uint8_t* out, int64_t* component_voxels);

/* sitk.BinaryDilate / BinaryErode / BinaryMorphologicalClosing(mask, radius) with SimpleITK's defaults
 * (registration/utils.py:328-329; projects/multiatlas/run.py:421-423, projects/cardiac/run.py:1127-1129):
 * kernel = ITK ball, offset d in the element when sum_i (d_i / (radius_i + 0.5))^2 <= 1; dilation sees background
 * and erosion foreground outside the buffer; PP_MORPH_CLOSE = dilate then erode with a safe border (as if padded
 * by the radius).  Masks are 0 / non-zero in, 0 / 1 out; radius in voxels per axis (x, y, z), each <= 15. */
int pp_binary_morph_ball_u8(pp_ctx* ctx, const uint8_t* in, const int size[3], const int radius[3], int op,
                            uint8_t* out);

/* Bounding box of the voxels > 0 (label_to_roi, utils/crop.py:24-60): box (host) = {xmin, xmax, ymin, ymax, zmin,
 * zmax}; an empty volume gives xmin > xmax.  dtype = PP_DTYPE_U8 or PP_DTYPE_F32.  Synchronises. */
int pp_bounding_box(pp_ctx* ctx, const void* data, int dtype, const int size[3], int box[6]);

/* ---- STAPLE ------------------------------------------------------------------------ */
#define PP_STAPLE_MAX_RATERS 64
enum { PP_STAPLE_FOREGROUND = 0, PP_STAPLE_BINARY_THRESHOLD = 1 };
typedef struct {
  int foreground_test;          /* PP_STAPLE_FOREGROUND: fg - 1e-10 < v < fg + 1e-10 (sitk.STAPLE's own test);
                                   PP_STAPLE_BINARY_THRESHOLD: 0.5 <= v <= 255 (sitk.BinaryThreshold(lowerThreshold=0.5)
                                   first, label/fusion.py:218); both compared in double                        */
  int rescale;                  /* 1: RescaleIntensity(W, 0, 1), then values outside [threshold_lower, 1] -> 0  */
  double foreground_value;
  double confidence_weight;
  uint64_t maximum_iterations;  /* UINT64_MAX: until convergence                                                */
  double threshold_lower;       /* with rescale; -inf skips the threshold                                       */
} pp_staple_params;
typedef struct {
  double sensitivity[PP_STAPLE_MAX_RATERS];   /* p_j of the last M step (NaN when degenerate)                   */
  double specificity[PP_STAPLE_MAX_RATERS];   /* q_j                                                            */
  uint64_t elapsed_iterations;
  int64_t n_zero, n_one, n_mixed;             /* voxels no rater / every rater / some raters mark                */
  int degenerate;                             /* no rater marks anything or every rater marks everything: W is the
                                                 initial estimate (all 0 or all 1), no EM step ran                */
  int reserved;
} pp_staple_result;
/* sitk.STAPLE(labels, confidence_weight, foreground_value) (label/fusion.py:223; itk::STAPLEImageFilter's EM with ITK's
 * 1e-14 stopping test, plus a stop on a floating-point 2-cycle of (p, q)).  labels: host array of `nraters` (1..64)
 * device pointers to n voxels each, dtype PP_DTYPE_U8 or PP_DTYPE_F32.  w: n fp64 voxels out.  Synchronises. */
int pp_staple_fuse(pp_ctx* ctx, const void* const* labels, int dtype, int nraters, size_t n,
                   const pp_staple_params* params, double* w, pp_staple_result* result);

/* ---- patch correlation and mutual information -------------------------------------- */
/* The per-voxel scipy.stats.pearsonr loop of compute_weight_map(vote_type="patch_correlation") (label/fusion.py:94-132)
 * as one pass.  For output voxel i the patch spans, per axis with window w, the input indices i - (w - 1) / 2 ... i + w / 2
 * (integer division) that lie inside the image -- the reference's zero padding plus its mask of ones: padded voxels are
 * left out, not counted as zeros.  corr = Pearson r of the two patches, clipped to [-1, 1] as scipy clips it, and exactly 0
 * where scipy returns NaN: where either patch is exactly constant (every voxel equal to the patch's first in-image voxel;
 * no variance threshold).  The moments are accumulated in fp64 on values shifted by each patch's first in-image voxel
 * (CT patches have means near -1000 and a small spread), in raster order of the patch: a rerun gives the same bits.  The
 * result is rounded to fp32 once.
 * window = {x, y, z} voxels, each >= 1.  When every axis has w <= 2 some patch holds a single voxel, where pearsonr
 * raises: PP_ERR_SIZE.  Windows of up to 8 and up to 16 voxels per axis run from an LDS tile of both images (one
 * workgroup per 8 x 8 x 4 outputs); a larger window takes a slower path that reads the patches from global memory and
 * gives the same values.  corr must not alias an input. */
int pp_patch_correlation_f32(pp_ctx* ctx, const float* target, const float* moving, const int size[3], const int window[3],
                             float* corr);
/* np.histogram2d(a, b, bins=(bins_a, bins_b)) behind mutual_information (label/fusion.py:26-53): hist (HOST, bins_a x bins_b
 * int64, row = bin of a) holds exactly numpy's counts for the float32 samples taken as doubles.  Per array the edges are
 * numpy's linspace(min, max, bins + 1) in fp64 (min == max widened by -/+ 0.5); a sample's bin is the one
 * searchsorted(edges, v, side="right") - 1 picks -- an arithmetic guess corrected against the fp64 edge table -- and the
 * top edge is closed.  range (HOST, out) = the outer edges {amin, amax, bmin, bmax} after that widening.  Integer counts:
 * per-workgroup LDS tables while bins_a * bins_b <= 16384 (128 x 128), global integer atomics beyond; a rerun gives the
 * same counts.  A NaN or infinite sample is an error (PP_ERR_ARG), as numpy raises.  Synchronises. */
int pp_joint_histogram_f32(pp_ctx* ctx, const float* a, const float* b, size_t n, int bins_a, int bins_b, int64_t* hist,
                           double range[4]);

/* ---- dose-volume histograms and dose metrics --------------------------------------- */
typedef struct {
  int64_t count;     /* voxels with label != 0                                                              */
  int64_t mask_sum;  /* sum of the label's own values there (a 0 / 255 mask counts 255 per voxel)           */
  double dose_sum;   /* the exact sum of the fp32 doses there, rounded to fp64 once                         */
  float dose_min;    /* +inf / -inf for an empty label                                                      */
  float dose_max;
} pp_dose_stats;
/* np.histogram(dose[label_l != 0], bins=edges) for l = 0 ... nlabels - 1 in one pass over the volume (imaging/dose/dvh.py),
 * and each label's statistics.  labels: host array of nlabels (1 ... 64) device pointers to n uint8 voxels each, non-zero =
 * inside.  edges: nbins + 1 (nbins 1 ... 2^20) HOST doubles that do not decrease; the last one may be +inf.  hist (HOST,
 * int64 [nlabels][nbins]): a voxel is counted in the bin with edges[k] <= v < edges[k + 1], the last bin closed on the
 * right, values outside the edges dropped, the fp32 dose compared as a double -- exactly numpy's counts.  stats (HOST,
 * nlabels records, or NULL) covers every voxel of a label, including those the histogram dropped.  More labels or bins than
 * that, or 2^31 voxels or more: PP_ERR_SIZE.  A NaN dose inside any label is an error (PP_ERR_ARG; numpy would return a NaN
 * mean); NaNs outside every label are never looked at.  Only integer atomics are used (the dose sum is accumulated exactly,
 * as a 288-bit integer): a rerun gives the same bits.  Per-workgroup LDS tables for as many labels at a time as fit 12288
 * counters (at most 16; one launch per group of labels), global integer atomics when nbins > 12288.  Synchronises. */
int pp_dose_histogram_f32(pp_ctx* ctx, const float* dose, const uint8_t* const* labels, int nlabels, size_t n,
                          const double* edges, int nbins, int64_t* hist, pp_dose_stats* stats);
/* out[j] (HOST) = the ranks[j]-th smallest (0-based) dose among the voxels with label != 0, bit for bit the fp32 value
 * np.partition puts there (-0.0 sorts below +0.0), for 1 ... 8 ranks: a radix select in three counting passes of 11 + 11 + 10
 * bits over the order-preserving integer image of the value; nothing is sorted or copied.  An empty label, a rank outside
 * [0, count) or a NaN inside the label: PP_ERR_ARG.  Synchronises. */
int pp_masked_order_stats_f32(pp_ctx* ctx, const float* dose, const uint8_t* label, size_t n, const int64_t* ranks,
                              int nranks, float* out);
/* counts[l][j] (HOST, int64 [nlabels][nthresholds]) = voxels of label l with dose >= thresholds[j], compared in fp32, for
 * every pair in one pass (pp_dose_histogram_f32 over the sorted thresholds with an open top bin).  nthresholds 1 ... 2^20;
 * a NaN threshold, or a NaN dose inside a label: PP_ERR_ARG.  Synchronises. */
int pp_masked_count_ge_f32(pp_ctx* ctx, const float* dose, const uint8_t* const* labels, int nlabels, size_t n,
                           const float* thresholds, int nthresholds, int64_t* counts);

/* ---- radiomics: first-order moments and texture tables ------------------------------ */
/* The counting behind the "PyRadiomics Extractor" (services/radiomics/service.py:76-236; the classes of :31-40 that it runs
 * at :152-177), for ONE structure on the contiguous crop of its bounding box; the feature formulas are host code
 * (platipy_amd/radiomics/features.py).  Count, sum, minimum and maximum come from pp_dose_histogram_f32 (which is also
 * compute_histogram, service.py:58-73) and percentiles from pp_masked_order_stats_f32.  Parity with pyradiomics is unpinned:
 * it is not installed where this was written (DESIGN 4.16 lists the semantics Q1 ... as recalled).
 *
 * *count (HOST) = the voxels with mask != 0 and lo <= v <= hi (lo, hi may be -inf / +inf; a NaN voxel is never inside), and
 * sums[6] (HOST) = S(v - c), S|v - c|, S(v - c)^2, S(v - c)^3, S(v - c)^4 and S v^2 over them, c = centre, every term and sum
 * in fp64.  The reduction has a fixed order for a given n (no floating-point atomics): two calls return the same bits,
 * whatever the alignment of the buffers.  2^31 voxels or more: PP_ERR_SIZE.  Synchronises. */
int pp_masked_moments_f32(pp_ctx* ctx, const float* image, const uint8_t* mask, size_t n, double lo, double hi, double centre,
                          int64_t* count, double sums[6]);
/* levels[i] (DEVICE, uint16, every voxel written) = np.digitize(image[i], edges) where mask[i] != 0, else 0: pyradiomics'
 * binning (imageoperations.binImage, behind every texture class of service.py:161).  edges: nedges >= 2 finite, strictly
 * increasing HOST doubles (the caller's np.arange, so a level is decided against numpy's own edges; the fp32 value is
 * compared as a double).  A voxel inside the mask that is NaN, infinite, below edges[0] or not below the last edge:
 * PP_ERR_ARG (levels are written all the same).  More than 65535 levels (nedges - 1), or 2^31 voxels or more: PP_ERR_SIZE.
 * 16-byte image loads where image is 16-byte, mask 4-byte and levels 8-byte aligned.  Synchronises. */
int pp_radiomics_discretise_f32(pp_ctx* ctx, const float* image, const uint8_t* mask, size_t n, const double* edges, int nedges,
                                uint16_t* levels);
/* The tables of the glcm, gldm and ngtdm classes (service.py:34-38) from a level volume (size = {x, y, z}, 0 = outside the
 * mask, levels 1 ... ng) in one pass over 32 x 8 x 8 tiles held in LDS with a one-voxel halo.  Outputs are HOST int64 and may
 * each be NULL (ngtdm_n and ngtdm_s go together):
 *   glcm    [13][ng][ng]  [d][i - 1][j - 1] = voxels of level i whose neighbour at +direction d has level j, both inside the
 *                         mask; directions: the offsets (dz, dy, dx) whose first non-zero component is positive, in
 *                         lexicographic order.  The symmetric matrix is glcm[d] + glcm[d]^T.
 *   gldm    [ng][27]      [i - 1][k] = voxels of level i with k of their 26 neighbours at the same level
 *   ngtdm_n [ng][27]      [i - 1][k] = voxels of level i with k of their 26 neighbours inside the mask
 *   ngtdm_s [ng][27]      [i - 1][k] = over those voxels, the sum of |i k - sum of the neighbours' levels|
 * Counts are kept in per-workgroup LDS tables of 8192 counters and flushed with 64-bit integer atomics: the GLCM in 1 ... 13
 * direction groups while 13 / groups x ng^2 fits (ng <= 90), the others while 81 ng fits (ng <= 101); beyond that, 64-bit
 * global integer atomics.  Integer sums only: a rerun gives the same bits.  ng 1 ... 1024, above that or 2^31 voxels or more:
 * PP_ERR_SIZE; a voxel whose level exceeds ng: PP_ERR_ARG (it is never used as an index).  Synchronises. */
int pp_texture_neighbourhood_u16(pp_ctx* ctx, const uint16_t* levels, const int size[3], int ng, int64_t* glcm, int64_t* gldm,
                                 int64_t* ngtdm_n, int64_t* ngtdm_s);
/* The table of the glrlm class (service.py:35): glrlm (HOST int64 [13][ng][nr], nr = the longest box axis, anything else is
 * PP_ERR_ARG) [d][i - 1][r - 1] = maximal runs of r voxels of level i along direction d (the 13 of
 * pp_texture_neighbourhood_u16).  A voxel starts a run when its predecessor is outside the box, outside the mask or of
 * another level; its thread walks the run.  Integer atomics only (LDS counters for runs of up to 8 voxels while ng <= 78): a
 * rerun gives the same bits.  Limits and errors as pp_texture_neighbourhood_u16.  Synchronises. */
int pp_texture_runs_u16(pp_ctx* ctx, const uint16_t* levels, const int size[3], int ng, int nr, int64_t* glrlm);

/* ---- SIFT landmarks for deformable-registration QA ---------------------------------- */
/* The hot paths behind the reference's DIR QA service (services/dirqa/service.py:60-140 runs `plastimatch sift` on two
 * cropped, windowed images and keeps the matches inside a contour).  Neither plastimatch nor ITK's SIFT filter is available
 * where this was written: parity with them is UNPINNED and the semantics are this build's own rules S1 ... S7 (stated in
 * csrc/pp_sift.h and DESIGN 4.17, restated in numpy by tests/sift_restatement.py).  All four promise identical bits on a rerun.
 *
 * gauss: DEVICE, one octave's nlevels = intervals + 3 (4 ... 8) Gaussian volumes of size = {x, y, z}, one after another.
 * D_l = G_{l+1} - G_l (one fp32 subtraction, never written).  A voxel of a level 1 <= l <= nlevels - 3, at least one voxel
 * from every face, is a candidate when D_l is strictly greater, or strictly smaller, than its 80 neighbours (S3); it is
 * refined and tested in fp64 (S4: one clamped Newton step, |response| / range >= contrast_threshold, definite Hessian,
 * trace^3 / det < curvature_threshold).  candidates_only != 0 skips S4 (offset 0, response = D; range and thresholds unused).
 * Outputs are HOST: *count = the kept keypoints, and the first min(count, capacity) of them in ascending (level, z, y, x)
 * (S5): index[k] = {x, y, z, level}, values[k] = {offset x, y, z, response}; rows beyond are untouched.  An axis shorter
 * than 3: count 0, nothing launched.  A range that is not positive and finite, a NaN threshold, nlevels outside 4 ... 8:
 * PP_ERR_ARG; 2^31 voxels or more: PP_ERR_SIZE.  Synchronises. */
int pp_dog_extrema_f32(pp_ctx* ctx, const float* gauss, const int size[3], int nlevels, double range, double contrast_threshold,
                       double curvature_threshold, int candidates_only, int capacity, int32_t* index, double* values, int64_t* count);
/* descriptors (DEVICE fp32 [n][768], every entry written) of n keypoints (HOST int32 [n][4] = {x, y, z, level}, level = the
 * Gaussian volume of `gauss` to describe on): the gradient-orientation histogram of S6 -- 16^3 voxels about the keypoint
 * (edge replicate), 4^3 cells x 12 icosahedron-vertex bins, Gaussian window, fp64 sums in a fixed order, L2-normalise, clip at
 * 0.2, normalise again.  Not rotation invariant.  spacing = {x, y, z} mm.  A keypoint outside the stack: PP_ERR_ARG before
 * anything is launched.  Synchronises (the keypoints are staged from the caller's array). */
int pp_sift_describe_f32(pp_ctx* ctx, const float* gauss, const int size[3], int nlevels, const double spacing[3],
                         const int32_t* keypoints, int n, float* descriptors);
/* For every row i of a (DEVICE fp32 [na][length]): best_index[i] (DEVICE int32) = the row of b (DEVICE fp32 [nb][length]) at
 * the smallest squared L2 distance (fp32, components in ascending order, one fused multiply-add each), the lowest index on a
 * tie; best[i], second[i] (DEVICE fp32) = the smallest and second-smallest distance (S7).  With points_a / points_b (DEVICE
 * fp64 [n][3], both or neither) only rows of b within `radius` of row i's point take part.  No row takes part: -1, +inf,
 * +inf; one: second = +inf.  Any length >= 1.  The rows of b are split over workgroups and the partial results folded in a fixed
 * order (context scratch: 12 bytes per row of a and segment); the result does not depend on the split.  No synchronisation. */
int pp_descriptor_match_f32(pp_ctx* ctx, const float* a, int na, const float* b, int nb, int length, const double* points_a,
                            const double* points_b, double radius, int32_t* best_index, float* best, float* second);
/* out[k] (HOST fp64 [n][3]) = points[k] + D(points[k]) for physical points (HOST fp64 [n][3]) and a planar fp32 displacement
 * field (DEVICE [3][nz][ny][nx], mm) with geometry g: the continuous index of pp_resample_f32's own map, fp64 trilinear
 * interpolation with ITK's clamped upper corner; a point outside [-0.5, n - 0.5) on any axis moves by zero, as
 * itk::DisplacementFieldTransform leaves it [ITK-upstream, unverified here].  Synchronises. */
int pp_transform_points_f64(pp_ctx* ctx, const float* field, const pp_geom* g, const double* points, int n, double* out);

/* ---- iterative atlas removal ------------------------------------------------------- */
/* sitk.LabelContour(mask) with face connectivity (label/projection.py:85): object voxels that have a face
 * neighbour of a different value. */
int pp_label_contour_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], uint8_t* out);
/* sitk.SignedMaurerDistanceMap(mask, squaredDistance=False, useImageSpacing=True) (label/projection.py:80-82,
 * registration/utils.py:288-293): exact Euclidean distance (mm) to the nearest border voxel of the object
 * (object voxel with background in its 26-neighbourhood), 0 on the border; want_signed = 0 gives the absolute
 * map, otherwise inside is negative unless inside_positive. */
int pp_distance_map_f32(pp_ctx* ctx, const uint8_t* mask, const pp_geom* g, int want_signed,
                        int inside_positive, float* out);

/* ---- label comparison -------------------------------------------------------------- */
/* The three counts every volume metric is made of (label/comparison.py:157-180, :211-213): counts (host, 3 x int64) =
 * |A|, |B|, |A and B| over n voxels, non-zero = foreground, one streaming pass over both masks.  Synchronises. */
int pp_overlap_counts_u8(pp_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, int64_t counts[3]);
/* sitk.BinaryContourImageFilter, FullyConnectedOn (label/comparison.py:51-54): object voxels with a background voxel in
 * their 26-neighbourhood -- the border rule of pp_distance_map_f32; fully_connected = 0 gives the face rule of
 * pp_label_contour_u8.  Voxels outside the image are not neighbours. */
int pp_binary_contour_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], int fully_connected, uint8_t* out);
/* sitk.LabelContour(label[:, :, i]) for every slice i at once (label/comparison.py:373-374): object voxels with a
 * background voxel among their four in-plane face neighbours. */
int pp_slice_contour_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], uint8_t* out);
/* min and max of |in| over n voxels into device_range (DEVICE, 2 floats): the range of sitk.Abs(SignedMaurerDistanceMap)
 * that itk::LabelStatisticsImageFilter's histogram spans (label/comparison.py:99-106).  No read-back, no synchronisation. */
int pp_abs_range_f32(pp_ctx* ctx, const float* in, size_t n, float* device_range);
/* sitk.LabelIntensityStatisticsImageFilter over a distance map, fused with the selection of its samples
 * (label/comparison.py:99-113; :64-65; itk::DirectedHausdorffDistanceImageFilter behind :89-91).  `select` is a label on
 * the grid g, `dist` a distance map on it, read only where a sample sits:
 *   PP_SURFACE_CONTOUR_ABS   samples = sitk.LabelContour(select) (face rule, evaluated on the fly), value = |dist|
 *   PP_SURFACE_LABEL_POS     samples = every voxel of select, value = max(dist, 0)      (directed Hausdorff)
 *   PP_SURFACE_NONZERO       samples = every non-zero voxel of select, value = dist     (select is a ready contour)
 * out (DEVICE, 8-byte aligned): count, fp64 sum and sum of squares, min, max, the count of values <= tau and, when
 * device_range (DEVICE, 2 floats {lo, hi}, e.g. from pp_abs_range_f32) is not NULL, ITK's 128-bin histogram of the values
 * over [lo, hi]: bin = min(int((v - lo) / (hi - lo) * 128), 127) in fp64.  Sums run in a fixed order and the bins are
 * integers: a rerun ON THE SAME BUFFERS gives the same bits.  The order follows the alignment of `select`: on a 16-byte
 * boundary a thread sums 16 consecutive voxels (and the grid is sized for that), elsewhere one voxel per step, so
 * `sum` and `sum_sq` of a select that starts elsewhere may differ from an aligned one's in the last bits (fp64 rounding of
 * the same samples); every other member does not depend on it.  No read-back, no synchronisation. */
enum { PP_SURFACE_CONTOUR_ABS = 0, PP_SURFACE_LABEL_POS = 1, PP_SURFACE_NONZERO = 2 };
#define PP_SURFACE_BINS 128
typedef struct pp_surface_stats {
  int64_t count;
  int64_t count_le_tau;
  double sum, sum_sq;
  float min, max;                  /* FLT_MAX, -FLT_MAX when count == 0 */
  float range_lo, range_hi;        /* the histogram's range (0, 0 without device_range) */
  int64_t hist[PP_SURFACE_BINS];
} pp_surface_stats;
int pp_surface_stats_f32(pp_ctx* ctx, const uint8_t* select, const float* dist, const pp_geom* g, int mode, double tau,
                         const float* device_range, pp_surface_stats* out);
/* Per z slice, the number of voxels with a != 0 and not_b == 0 (not_b may be NULL: the count of a): sitk.MaskNegated +
 * sum per slice, and the "both slices empty" test (label/comparison.py:367-385).  per_slice: DEVICE, size[2] x int64, 8-byte
 * aligned (PP_ERR_ARG otherwise); a and not_b at any address, the counts do not depend on it.
 * No read-back, no synchronisation. */
int pp_slice_masked_count_u8(pp_ctx* ctx, const uint8_t* a, const uint8_t* not_b, const int size[3], int64_t* per_slice);

/* ---- linear registration ----------------------------------------------------------- */
/* One evaluation of the mean-squares metric (itk::MeanSquaresImageToImageMetricv4, selected at
 * registration/linear.py:141-148, evaluated inside registration.Execute at :238) and its gradient
 * with respect to an affine map in INDEX space.  Sample points: every `stride`-th voxel, raster
 * order, of a virtual grid vsize (REGULAR sampling, linear.py:152-153).  For virtual index v:
 * f = trilinear(fixed, Af v + bf), m = trilinear(moving, Am v + bm); samples leaving either buffer or
 * rejected by a mask (nearest voxel == 0) are skipped.  result (host, 14 doubles):
 * [0] sum (f-m)^2, [1] count, [2..10] d/dAm (row-major), [11..13] d/dbm.  Synchronises. */
int pp_meansq_affine_f32(pp_ctx* ctx, const float* fixed, const int fsize[3], const float* moving,
                         const int msize[3], const double Af[9], const double bf[3],
                         const double Am[9], const double bm[3], const int vsize[3], int stride,
                         const uint8_t* fixed_mask, const uint8_t* moving_mask, double* result);

/* The same sampling for the correlation metric (itk::CorrelationImageToImageMetricv4, linear.py:142-143): raw
 * moments from which value and gradient of -corr^2 follow on the host.  result (host, 42 doubles):
 * [0] count [1] sum f [2] sum m [3] sum f^2 [4] sum m^2 [5] sum f m, then three blocks of 12 (d/dAm row-major 9,
 * d/dbm 3): [6..17] sum g, [18..29] sum f g, [30..41] sum m g, with g the interpolant-gradient terms g_r v_q / g_r. */
int pp_corr_moments_affine_f32(pp_ctx* ctx, const float* fixed, const int fsize[3], const float* moving,
                               const int msize[3], const double Af[9], const double bf[3],
                               const double Am[9], const double bm[3], const int vsize[3], int stride,
                               const uint8_t* fixed_mask, const uint8_t* moving_mask, double* result);

/* Line-search evaluations (ITK GradientDescentLineSearchOptimizerv4::GoldenSectionSearch inside
 * registration.Execute, registration/linear.py:238): metric VALUES only, for `ncand` (1..16) candidate moving
 * maps Am[c][9], bm[c][3] in one launch -- the host speculates the next levels of the search tree.  Sampling,
 * validity and interpolation exactly as pp_meansq_affine_f32 / pp_corr_moments_affine_f32.  result (host,
 * ncand x 6 doubles): metric 0 -> [sum (f-m)^2, count, -, -, -, -]; metric 1 -> [count, sum f, sum m, sum f^2,
 * sum m^2, sum f m].  A candidate's numbers do not depend on the others in the call.  Synchronises. */
int pp_metric_values_affine_f32(pp_ctx* ctx, int metric, const float* fixed, const int fsize[3],
                                const float* moving, const int msize[3], const double Af[9],
                                const double bf[3], int ncand, const double* Am, const double* bm,
                                const int vsize[3], int stride, const uint8_t* fixed_mask,
                                const uint8_t* moving_mask, double* result);

/* ITK's sample-point jitter for every metric entry point of this section (registration.SetMetricSamplingPercentage(rate,
 * seed=42) + SetMetricSamplingStrategy(REGULAR), registration/linear.py:151-152): itk::ImageRegistrationMethodv4 perturbs each
 * REGULAR sample point by a seeded normal variate times a third of the virtual spacing per axis.  `jitter` (device, caller-owned,
 * must stay valid until replaced): 3 floats per sample of the raster walk, in VIRTUAL-INDEX units, added to the sample's lattice
 * index before the fixed and moving maps are applied; `nsamples` its length in samples (>= the lattice's sample count of every
 * later call, else that call fails).  NULL / 0 restores the plain lattice (the default).  The host draws the variates
 * (platipy_amd/registration/linear.py, itk_sampling=True). */
int pp_linear_set_sample_jitter(pp_ctx* ctx, const float* jitter, size_t nsamples);

/* ITK's moving-image gradient source for the gradient-bearing metric entry points of this section (pp_meansq_affine_f32,
 * pp_corr_moments_affine_f32, pp_mi_gradient_f32, pp_linear_optimize_f32): itk::ImageToImageMetricv4 (inside
 * registration.Execute, registration/linear.py:238) by default does not differentiate the intensity interpolant but LINEARLY
 * interpolates a gradient image it computes once per level with itk::GradientRecursiveGaussianImageFilter (sigma = the moving
 * image's largest spacing).  `gradient` (device, caller-owned, valid until replaced): that image as three volumes
 * [3][Z][Y][X] of the moving image's size `msize`, converted to moving-INDEX units (d intensity / d index); NULL restores the
 * interpolant's analytic gradient (the default).  Built by the host from pp_recursive_gaussian_pass_f32. */
int pp_linear_set_moving_gradient(pp_ctx* ctx, const float* gradient, const int msize[3]);
/* Optional companion of the image above for the value + gradient kernel (pp_meansq_affine_f32 / pp_corr_moments_affine_f32 and
 * through them pp_linear_optimize_f32): the SAME gradient image packed with the moving image's intensity, [Z][Y][X][4] =
 * (gx, gy, gz, m) per voxel, 16-byte aligned (device, caller-owned, valid until replaced).  With ITK's jittered sample points
 * every sample has its own rows; one 16-byte element per corner is 8 gathers and ~0.25 KB of cache sectors a sample where the
 * planar images cost 32 and ~1 KB.  Results are bit-identical.  Call after pp_linear_set_moving_gradient (which clears it);
 * NULL removes it.  (No reference counterpart: a layout of this build.) */
int pp_linear_set_moving_gradient_packed(pp_ctx* ctx, const float* packed);

/* Mutual-information metrics (SetMetricAsMattesMutualInformation / SetMetricAsJointHistogramMutualInformation,
 * registration/linear.py:145-148) over the same sample lattice: pass 1 returns the joint intensity histogram of the valid
 * sample pairs (row = fixed bin; 64-bit fixed-point accumulation, independent of scheduling) and their count; the caller
 * turns it into PDFs, the value and a per-bin score table; pass 2 returns sum_s w_s g_s v_q / sum_s w_s g_s in the
 * d/dAm (9), d/dbm (3) layout of pp_meansq_affine_f32 with w_s = sum_k dkernel_k(s) table[f_bin(s)][k].
 * bin coordinate of an intensity = value / *_bin - *_norm_min.  PP_MI_MATTES: fixed nearest bin, moving cubic B-spline
 * over 4 bins, both clamped to [2, nbins - 3] (itk::MattesMutualInformationImageToImageMetricv4); PP_MI_JOINT: nearest
 * bins, the score differenced between the two neighbouring moving-bin centres. */
enum { PP_MI_MATTES = 0, PP_MI_JOINT = 1 };
typedef struct pp_mi_bins {
  int nbins;                 /* <= 64 */
  int kernel;                /* PP_MI_* */
  double f_bin, f_norm_min;  /* fixed:  bin width, normalised minimum */
  double m_bin, m_norm_min;  /* moving */
} pp_mi_bins;
int pp_mi_histogram_f32(pp_ctx* ctx, const float* fixed, const int fsize[3], const float* moving, const int msize[3],
                        const double Af[9], const double bf[3], const double Am[9], const double bm[3],
                        const int vsize[3], int stride, const uint8_t* fixed_mask, const uint8_t* moving_mask,
                        const pp_mi_bins* bins, double* hist, double* count);
int pp_mi_gradient_f32(pp_ctx* ctx, const float* fixed, const int fsize[3], const float* moving, const int msize[3],
                       const double Af[9], const double bf[3], const double Am[9], const double bm[3],
                       const int vsize[3], int stride, const uint8_t* fixed_mask, const uint8_t* moving_mask,
                       const pp_mi_bins* bins, const double* table, double* result);

/* One resolution level of linear_registration's optimisation (what registration.Execute does inside a level,
 * registration/linear.py:129-238): ITK v4 gradient descent (optionally with the golden-section line search) on
 * the mean-squares or correlation metric above, parameter scales from physical shift, learning rate estimated
 * once, convergence window 10 / 1e-6, best point kept.  Host logic in the library, metric on the GPU. */
enum { PP_MODEL_TRANSLATION = 0, PP_MODEL_VERSOR_RIGID = 1, PP_MODEL_SIMILARITY = 2, PP_MODEL_SCALE = 3,
       PP_MODEL_AFFINE = 4, PP_MODEL_EULER = 5, PP_MODEL_SCALE_VERSOR = 6,
       PP_MODEL_SCALE_SKEW_VERSOR = 7 };                 /* sitk parameter layouts; 3/6/7/3/12/6/9/15 parameters */
enum { PP_OPT_GD = 0, PP_OPT_GD_LINE_SEARCH = 1 };
enum { PP_LINREG_RETURN_BEST = 1 };
enum { PP_LINREG_STOP_ITERATIONS = 0, PP_LINREG_STOP_CONVERGED = 1, PP_LINREG_STOP_NO_OVERLAP = 2 };
typedef struct pp_linreg_level {
  int model;              /* PP_MODEL_*: q = A(params) (p - center) + center + t(params)            */
  int metric;             /* 0 mean squares, 1 correlation                                            */
  int optimizer;          /* PP_OPT_*                                                                 */
  int iterations;         /* numberOfIterations                                                       */
  int vsize[3];           /* virtual (shrunk fixed) domain                                            */
  int stride;             /* REGULAR sampling: every stride-th voxel of it                            */
  int speculation;        /* golden-section tree levels probed per launch, 1..4 (1 = sequential)      */
  int flags;              /* PP_LINREG_RETURN_BEST or 0 (ITK / SimpleITK default: the level's last point) */
  double v_i2p[9], v_origin[3]; /* virtual index -> physical: p = v_i2p idx + v_origin               */
  double f_p2i[9], f_origin[3]; /* fixed  physical -> index:  idx = f_p2i (p - f_origin)             */
  double m_p2i[9], m_origin[3]; /* moving physical -> index                                           */
  double init_matrix[9], init_offset[3]; /* the centring transform composed in front: q = M p + o    */
  double center[3];       /* fixed centre of rotation of the optimised transform                      */
  double v_min_spacing;   /* m_MaximumStepSizeInPhysicalUnits of the learning-rate estimate: the smallest virtual
                             spacing OF THE FIRST LEVEL (ITK assigns the default once per optimiser)     */
} pp_linreg_level;
typedef struct pp_linreg_stats {
  int iterations;         /* optimiser iterations taken            */
  int evaluations;        /* metric evaluations (probes included)  */
  int stop;               /* PP_LINREG_STOP_*                      */
  int reserved;
  double value;           /* optimiser's GetMetricValue(): the last evaluation (with RETURN_BEST: at the returned point) */
  double learning_rate;   /* last learning rate                    */
} pp_linreg_stats;
int pp_linear_num_parameters(int model);
/* params (host, in/out): pp_linear_num_parameters(model) doubles.  history (host, may be NULL): metric value
 * per iteration, up to history_capacity.  PP_ERR_NO_OVERLAP when no sample point is valid at the start. */
int pp_linear_optimize_f32(pp_ctx* ctx, const float* fixed, const int fsize[3], const float* moving,
                           const int msize[3], const uint8_t* fixed_mask, const uint8_t* moving_mask,
                           const pp_linreg_level* level, double* params, pp_linreg_stats* stats,
                           double* history, int history_capacity);

/* ---- cubic B-spline transform (sitk.BSplineTransform, order 3) ---------------------------------------------------
 * The coefficient lattice is a planar fp32 device array [3][cz][cy][cx] (x, y, z displacement in mm) with its own
 * geometry `lattice`: size = mesh + 3 per axis, spacing = domain length / mesh, origin one lattice spacing before the
 * domain origin, direction = the domain's.  A physical point p with continuous lattice index u is inside the transform
 * domain when 1 <= u < mesh + 1 on every axis; there T(p) = p + sum w_i w_j w_k c_ijk over its 4 x 4 x 4 support, and
 * T(p) = p everywhere else (itk::BSplineTransform::InsideValidRegion) [ITK-upstream, unverified here]. */

/* Dense evaluation: out = planar displacement field [3][Z][Y][X] of the transform on the grid `grid`
 * (sitk.TransformToDisplacementField for a B-spline; what apply_transform needs, reference registration/utils.py:176).
 * The grid may differ from the lattice in size, spacing, origin and direction; voxels outside the domain get exactly 0. */
int pp_bspline_field_f32(pp_ctx* ctx, const float* coefficients, const pp_geom* lattice, const pp_geom* grid, float* out);

enum { PP_BSPLINE_MEAN_SQUARES = 0, PP_BSPLINE_CORRELATION = 1 };
/* stats[] of pp_bspline_metric_f32 */
enum { PP_BSPLINE_STAT_VALID = 0, PP_BSPLINE_STAT_OUTSIDE = 1, PP_BSPLINE_STAT_MASKED = 2, PP_BSPLINE_STAT_SEEN = 3 };
/* Similarity metric of `fixed` and `moving` under the B-spline and its gradient with respect to all 3 cx cy cz
 * coefficients, ITK's flat parameter order (what registration_method.Execute evaluates per iteration at reference
 * deformable.py:513 with the metrics set at deformable.py:533 and before).  Samples are every `stride`-th voxel (raster
 * order) of the grid `virt`, moved by the jitter installed with pp_linear_set_sample_jitter when there is one; the
 * moving gradient comes from the image installed with pp_linear_set_moving_gradient(_packed), else from the
 * trilinear interpolant; masks are uint8 volumes of the fixed / moving size or NULL.  Value and sign conventions are
 * those of pp_meansq_affine_f32 (sum of squares / count) and pp_corr_moments_affine_f32 combined (-corr^2).
 *   jitter_bound: an upper bound of |jitter| in virtual voxels, any axis (0 without jitter); a sample that moves
 *                 further is reported as PP_ERR_ARG, never dropped silently.
 *   value, stats[4] (valid samples, samples outside the fixed or moving buffer, samples rejected by a mask, samples
 *   visited), gradient[3 cx cy cz]: HOST memory.  No valid sample: PP_ERR_NO_OVERLAP.
 * The direction cosines of `lattice`, `virt` and `fixed_geom` must agree (the initialiser takes them from the fixed
 * image): PP_ERR_DIRECTION otherwise, before anything is launched.  Two calls on the same inputs return identical bits.
 * A refusal (PP_ERR_ARG, PP_ERR_DIRECTION, a sample beyond jitter_bound, PP_ERR_NO_OVERLAP) leaves value, stats and gradient
 * untouched.  Synchronises. */
int pp_bspline_metric_f32(pp_ctx* ctx, int metric, const float* fixed, const pp_geom* fixed_geom, const float* moving,
                          const pp_geom* moving_geom, const pp_geom* virt, int stride, const uint8_t* fixed_mask,
                          const uint8_t* moving_mask, const float* coefficients, const pp_geom* lattice,
                          double jitter_bound, double* value, double* stats, double* gradient);

/* Mattes mutual information over the B-spline (SetMetricAsMattesMutualInformation(numberOfHistogramBins) at reference
 * deformable.py:482-485), in two passes as pp_mi_histogram_f32 / pp_mi_gradient_f32 are for the affine case.  Samples, their
 * validity, jitter, masks, the moving-gradient source, jitter_bound, the direction rule and stats[4] are exactly those of
 * pp_bspline_metric_f32; `bins` must be PP_MI_MATTES with 5..64 bins (PP_ERR_ARG otherwise).
 * Pass 1: hist[nbins * nbins] (HOST, row = fixed bin) = the joint histogram of the valid samples, fixed intensity in its
 * nearest bin, moving intensity spread over 4 bins by the cubic B-spline, every weight accumulated in 64-bit fixed point
 * (2^-32 units) with integer atomics: two calls return identical bits.  The caller turns it into the value and a score
 * table (platipy_amd/registration/_mattes.py).  A refusal (PP_ERR_ARG, PP_ERR_DIRECTION, a sample beyond jitter_bound,
 * PP_ERR_NO_OVERLAP) leaves hist and stats untouched.  Synchronises. */
int pp_bspline_mi_histogram_f32(pp_ctx* ctx, const float* fixed, const pp_geom* fixed_geom, const float* moving,
                                const pp_geom* moving_geom, const pp_geom* virt, int stride, const uint8_t* fixed_mask,
                                const uint8_t* moving_mask, const float* coefficients, const pp_geom* lattice,
                                double jitter_bound, const pp_mi_bins* bins, double* hist, double* stats);
/* Pass 2 (reference deformable.py:482-485, the derivative ITK's metric hands to the optimiser at :513): gradient[3 cx cy cz]
 * (HOST, ITK's flat parameter order), for coefficient p = (r, k, j, i)
 *   sum_s [ sum_{q = mb_s - 1 .. mb_s + 2} B3'(q - tm_s) table[fb_s][q] ] (g_s . Md)_r w_i w_j w_k
 * over the valid samples inside the transform domain whose 4 x 4 x 4 support holds the control point.  table[nbins * nbins]
 * (HOST, fp64; held as fp32 on the device) already carries 1 / (N m_bin): no further normalisation.  No floating-point
 * atomics: two calls return identical bits.  A refusal leaves stats and gradient untouched.  Synchronises. */
int pp_bspline_mi_gradient_f32(pp_ctx* ctx, const float* fixed, const pp_geom* fixed_geom, const float* moving,
                               const pp_geom* moving_geom, const pp_geom* virt, int stride, const uint8_t* fixed_mask,
                               const uint8_t* moving_mask, const float* coefficients, const pp_geom* lattice,
                               double jitter_bound, const pp_mi_bins* bins, const double* table, double* stats,
                               double* gradient);

/* ---- vessel splining --------------------------------------------------------------- */
/* The per-slice sums behind com_from_image_list (imaging/utils/vessel.py:33-167) and get_com (label/utils.py:61-84), for
 * every atlas's propagated label in one pass.  masks: HOST array of nmasks (1 ... 64) device pointers to uint8 volumes of
 * `size` (x, y, z).  axis: the scan axis, 0 (x, sagittal, vessel.py:46-105) or 2 (z, axial, :107-167); anything else is
 * PP_ERR_ARG (the reference's "y" falls through and crashes).  out (DEVICE, int64 [nmasks][size[axis]][4]) =
 * {sum v, sum a v, sum b v, count(v != 0)} of each slice, v the voxel's own value (the reference weights by value: a 0 / 255
 * mask weighs 255) and a, b the two in-slice array indices in the reference's order: z-scan row (image y) then column
 * (image x), vessel.py:116-122; x-scan array z then array y, :55-61.  Integer arithmetic and integer atomics only: the
 * table equals numpy's integer sums and a rerun gives the same bits.  The x-scan reads rows, never columns: the lanes of a
 * wavefront lie along x, 16 bytes each where the masks are 16-byte aligned and size[0] % 16 == 0.  An axis longer than
 * 65535 or 2^31 voxels or more: PP_ERR_SIZE.  No read-back, no synchronisation. */
int pp_slice_moments_u8(pp_ctx* ctx, const uint8_t* const* masks, int nmasks, const int size[3], int axis, int64_t* out);
/* The voxels within `radius` (mm) of a polyline: what vtkTubeFilter + vtkPolyDataToImageStencil make of the splined
 * centreline at imaging/utils/vessel.py:170-296 -- a deviation, VTK is not used and parity with its voxelisation (50-sided
 * tube, stencil tolerance 0.5) is UNPINNED.  points: HOST, npoints (>= 2) x 3 doubles in mm; the grid has identity
 * direction (the reference forces it at vessel.py:406-407).  out[z][y][x] = 1 iff for some segment k the distance from the
 * voxel centre origin + index * spacing to its closest point on the segment is <= radius, else 0; the ends are flat, as
 * vtkTubeFilter does not cap: on the first segment only points whose unclamped projection parameter is >= 0 count, on the
 * last only those with <= 1.  Segments of zero length are skipped (first and last then mean the first and last that remain);
 * if none remains: PP_ERR_ARG.  Decided in fp64.  One workgroup per brick of 16 x 16 x 4 voxels culls the segment list
 * against the brick's bounding sphere into LDS, in chunks, for any npoints.  Reruns are bit-identical.  Synchronises. */
int pp_tube_mask_u8(pp_ctx* ctx, const double* points, int npoints, const int size[3], const double spacing[3],
                    const double origin[3], double radius, uint8_t* out);

/* ---- RTSTRUCT contours -------------------------------------------------------------- */
/* Closed planar contours to binary masks: what the loop of skimage.draw.polygon calls and XORs does at
 * dicom/io/rtstruct_to_nifti.py:105-217, for all structures and all slices in ONE call.  vertices: HOST, nverts x 2 int32
 * (x, y) pixel indices, already rounded (the reference rounds them too, :172-180), each within +-2^24.  contours: HOST,
 * ncontours entries {first, count, structure, z}: the vertices first ... first + count - 1 (count >= 1) are one closed
 * polygon on slice z (0 ... size[2] - 1) of structure `structure` (0 ... nstructures - 1).  out: DEVICE, uint8
 * [nstructures][size[2]][size[1]][size[0]]; the call defines EVERY byte of it (1 inside, 0 elsewhere), the caller does not
 * clear it.  A pixel is inside a contour by scikit-image's point_in_polygon (the closed polygon for simple polygons: interior,
 * edges and vertices; recalled from upstream, UNVERIFIED here, parity with scikit-image UNPINNED), evaluated in exact
 * integers: no division, no floating point.  Contours of one structure on one slice combine by XOR (:209), so an inner contour
 * cuts a hole and the same contour twice gives nothing.  Pixels are clipped to the true slice [0, size[0]) x [0, size[1]) -- a
 * deviation: the reference passes shape = (ny, nx) to a call whose rows are x.  No contours at all is valid (all zeros).
 * One workgroup per 64 x 64 tile of a (structure, slice)'s bounding box, edges staged into LDS PP_CONTOUR_CHUNK at a time,
 * any count works; the rest of `out` is one memset on the same stream.  Nothing is atomic: reruns are bit-identical.
 * PP_ERR_ARG for a NULL table, a negative count, nstructures < 1, an empty volume, a contour outside the vertex table, a
 * structure or slice out of range, a vertex beyond +-2^24 (`out` is then untouched); an axis longer than 2^24: PP_ERR_SIZE.
 * Synchronises (the tables are host memory of the call). */
#define PP_CONTOUR_CHUNK 256
typedef struct {
  int32_t first, count; /* vertices of the contour */
  int32_t structure, z; /* the mask and the slice it is XORed into */
} pp_contour;
int pp_contour_fill_u8(pp_ctx* ctx, const int32_t* vertices, int nverts, const pp_contour* contours, int ncontours,
                       const int size[3], int nstructures, uint8_t* out);
/* Binary masks to closed planar contours, the inverse of pp_contour_fill_u8 and the volume-sized step of
 * dicom/io/nifti_to_rtstruct.py (convert_nifti, which hands every mask to rt-utils and OpenCV on the host), for all structures
 * and all slices in ONE extraction.  masks: DEVICE, uint8 [nstructures][size[2]][size[1]][size[0]], foreground = any non-zero
 * byte.  The rule (T1-T7 of platipy_amd/dicom, csrc/pp_contour_trace.h): the boundary of a slice is cut into directed cracks
 * (pixel sides with the foreground on their right as displayed), 8-connected foreground, linked into loops; a loop's leader is
 * its crack with the smallest (y, x, side); a leader on a north side is an outer border (clockwise as displayed), on a south
 * side a hole (the other way round).  A contour's vertices are the pixels the loop runs through -- its own foreground pixels
 * for an outer border, the hole's own background pixels for a hole -- every border pixel once per visit, starting at the
 * leader's pixel; with approximate != 0 a vertex whose incoming and outgoing steps are equal is dropped (lossy on parts one
 * pixel wide).  Contours are ordered by (structure, z, leader).  With approximate == 0, pp_contour_fill_u8 of the result gives
 * `masks` back byte for byte (as 0 / 1).  Parity with rt-utils / OpenCV is UNPINNED (neither is installed where this is
 * tested).
 *   Call shape: a COUNT call (vertices == contours == hole == NULL, nverts == ncontours == 0) runs the extraction, leaves the
 * tables in the context's scratch and writes counts = {cracks, vertices, contours} (HOST).  A FILL call (vertices: HOST,
 * nverts x 2 int32 (x, y); contours: HOST, ncontours rows {first, count, structure, z}; hole: HOST, ncontours bytes, 1 for a
 * hole) with exactly those counts copies them out.  A fill call that directly follows the count call of the same arguments on
 * the same context -- no other library call on it in between, `masks` unchanged -- only copies; any other fill call runs the
 * extraction first.  An extraction makes two host read-backs ({cracks, cracks of the largest slice}; {vertices, contours}).
 * Integer arithmetic only, one integer atomicMax, every output word written by one thread: reruns are bit-identical.  No
 * workgroup waits for another: every pointer-doubling round is its own launch, ceil(log2(cracks of the largest slice)) + 1
 * rounds for the leaders and as many for the ranking.  Scratch: one int per row and 64-pixel block, about 50 bytes per crack.
 * PP_ERR_ARG for a NULL argument, a NULL table beside a non-zero count, a negative count, table counts that are not the
 * extraction's (counts is still written), nstructures < 1, an empty volume, more than 2^31 - 1 cracks; an axis longer than
 * 2^24 or more than 2^31 - 1 rows: PP_ERR_SIZE.  Synchronises. */
int pp_contour_trace_u8(pp_ctx* ctx, const uint8_t* masks, const int size[3], int nstructures, int approximate,
                        int32_t* vertices, int nverts, pp_contour* contours, uint8_t* hole, int ncontours, int64_t counts[3]);

/* ---- region primitives (airway and lung segmentation) ------------------------------- */
/* sitk.ConnectedComponent(mask) with face connectivity (imaging/utils/lung.py:41-42, projects/bronchus/bronchus.py:214 and
 * :331-333): labels (DEVICE, int32, `size` voxels) = 0 on background (mask == 0), and 1 ... N on the components, numbered in
 * raster order of their first voxel -- the order ITK numbers them in [ITK-upstream, unverified here; SimpleITK is absent].
 * The labelling is the union-find of pp_fillhole_largest_component_u8 (a component's root is its first voxel); the roots
 * are then ranked by a reduce-then-scan over the volume in separate launches, no block waits for another.  count (HOST, may
 * be NULL) receives N (GetObjectCount); non-NULL synchronises.  2^31 voxels or more: PP_ERR_SIZE.  Reruns are
 * bit-identical. */
int pp_connected_components_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], int32_t* labels, int* count);
/* sitk.ConnectedComponent(mask, fullyConnected) (generation/mask.py:77).  fully_connected = 0 is
 * pp_connected_components_u8, bit for bit; with 1 two foreground voxels are joined when they differ by at most 1 on every
 * axis (13 backward neighbours).  Numbering stays 1 ... N in raster order of each component's first voxel.  The run-based
 * merge generalises: runs of the four backward rows (dy, dz) = (-1, 0), (0, -1), (-1, -1), (+1, -1) join when their
 * x-extents overlap after one of them is widened by 1, still tried only where a run starts (and at a run's last voxel, for
 * the run that starts one past it). */
int pp_connected_components_conn_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], int fully_connected, int32_t* labels,
                                    int* count);
/* The sums sitk.LabelShapeStatisticsImageFilter derives size, centroid and principal moments from (lung.py:46-56,
 * bronchus.py:221-229, :336-339), for every label in one pass.  labels: DEVICE int32 volume (4-byte aligned); out: DEVICE
 * int64 [nlabels][10] = {count, sum x, sum y, sum z, sum xx, sum yy, sum zz, sum xy, sum xz, sum yz} over the voxel indices of
 * label l in row l - 1.  Label 0, negative labels and labels above nlabels are ignored; a label that does not occur gives
 * zeros.  Exact integer sums (modulo 2^64) by 64-bit integer atomics, equal labels combined inside the block first; reruns
 * are bit-identical.  2^31 voxels or more: PP_ERR_SIZE.  No read-back, no synchronisation. */
int pp_label_moments_i32(pp_ctx* ctx, const int32_t* labels, const int size[3], int nlabels, int64_t* out);
/* sitk.ConnectedThreshold(image, seedList, lower, upper) (bronchus.py:259-262): out (DEVICE uint8) = 1 on every voxel that
 * is face-connected to a seed through voxels with lower <= v <= upper -- both ends included, compared in double, a NaN
 * never joins -- and 0 elsewhere.  seeds: HOST, nseeds x 3 indices (x, y, z); a seed whose own voxel is outside the interval
 * contributes nothing, a seed outside the buffer is PP_ERR_INVALID (ITK raises).  Threshold, the labelling of
 * pp_connected_components_u8, then the components of the seeds' roots.  voxels (HOST, may be NULL): the size of the region.
 * 2^31 voxels or more: PP_ERR_SIZE.  Reruns are bit-identical.  Synchronises. */
int pp_connected_threshold_f32(pp_ctx* ctx, const float* image, const int size[3], double lower, double upper, const int* seeds,
                               int nseeds, uint8_t* out, int64_t* voxels);
/* sitk.Median(mask, radius) on a 0 / non-zero mask (bronchus.py:194-196): out = 1 iff more than half of the
 * (2 rx + 1)(2 ry + 1)(2 rz + 1) window is non-zero, the window clamped to the volume (edge replication, ITK's zero-flux
 * Neumann condition).  radius (x, y, z) in 0 ... 2, anything else PP_ERR_ARG; `out` must not alias `in`.  From an LDS tile
 * with halo. */
int pp_binary_median_u8(pp_ctx* ctx, const uint8_t* in, const int size[3], const int radius[3], uint8_t* out);

/* ---- per-slice convex hull (patient external contour) ----------------------------------- */
/* skimage.morphology.convex_hull_image of every z-slice (generation/mask.py:94-99, a Python loop over the slices).  mask,
 * out: DEVICE uint8 [Z][Y][X].  For each slice let S be its non-zero pixels (y, x) and P the union over S of the four points
 * (y +- 1/2, x), (y, x +- 1/2) -- skimage's offset_coordinates=True diamond.  out[z][y][x] = 1 iff the pixel centre (y, x)
 * lies in the CLOSED convex hull of P: a centre exactly on a hull edge or vertex is inside.  Everything else is 0, every
 * voxel is written, an empty slice gives zeros.  Exact: doubled integer coordinates and int64 cross products, no floating
 * point takes part in any decision.  [The rule agrees with scikit-image 0.18.3 on the recorded masks of
 * tests/golden/slice_convex_hull_skimage_0.18.3.npz; that 0.21.0, which the reference locks, treats boundary centres the
 * same way is recalled, not verified.]  Row extents, then one workgroup per slice builds the left and right chains and
 * every row's closed interval, then a fill; `out` may be `mask` itself (in place), any other overlap is not allowed.  An
 * axis longer than 65535: PP_ERR_SIZE, nothing is launched.  No atomics on global memory, no block waits for another:
 * reruns are bit-identical. */
int pp_slice_convex_hull_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], uint8_t* out);

/* ---- left-ventricle 17-segment model (imaging/utils/ventricle.py) -------------------- */
/* The segment assignment of generate_left_ventricle_segments (ventricle.py:408-644: a Python loop over slices with 4 or 6
 * `extract` calls each, :30-72) for every slice at once.  mask: DEVICE uint8 [Z][Y][X], non-zero = inside.  slices: HOST,
 * one pp_polar_slice per z-slice; nrules == 0 skips the slice (its bits are written as 0, its counts stay 0).  rules: HOST,
 * nrules_total pp_polar_rule; slice z uses rules[first_rule ... first_rule + nrules).  For every mask voxel (y, x) of a
 * slice, in fp64, one rounding per operation, in this order:
 *     dy = y - cy, dx = x - cx;  theta = -atan2(dy, dx) - theta0;  if (theta < 0) theta += 2 pi  (ONCE: the angle may stay
 *     negative, and then matches no sector with angle_min >= 0, only a PP_POLAR_CW one);  r = sqrt(dy * dy + dx * dx)
 * A rule matches when r >= radius_min and -- PP_POLAR_CW set -- theta <= angle_min || theta >= angle_max, otherwise
 * theta >= angle_min && theta <= angle_max; both ends are inclusive, so a voxel on a boundary matches two rules.
 * angle_min = -inf, angle_max = +inf is "the whole slice".  counts (DEVICE, int64 [Z][32]): the voxels of slice z that match
 * a rule of label l, in [z][l - 1], before any suppression (a voxel counts once per label however many rules of that label
 * it matches).  A (slice, label) pair with (double)count * area < min_area_mm2 is suppressed as a whole (ventricle.py:67-70;
 * equality keeps it) unless a rule of that label on that slice carries PP_POLAR_ANY_AREA (the reference's segment 17 is
 * never put to the area test, :325-327).  bits (DEVICE, uint32 [Z][Y][X]): bit l - 1 set for every surviving match, 0
 * elsewhere; every voxel is written.  Two launches on the context's stream -- count, then write, which reads the counts
 * on the device; integer atomics only, so a rerun gives the same bits.  Labels outside 1 ... 32, a rule range outside the
 * table, unknown flags, NaN angles or areas, a centre that is not finite: PP_ERR_ARG before anything is written; an axis
 * longer than 65535: PP_ERR_SIZE.  The fp64 atan2 is the device library's: a voxel within an ulp of a sector boundary may
 * fall on either side of it compared with another libm.  Synchronises (the tables are host memory of the call). */
enum { PP_POLAR_CW = 1, PP_POLAR_ANY_AREA = 2 };
typedef struct pp_polar_slice {
  double cy, cx;      /* the slice's centre: row (y), column (x) */
  double theta0;      /* subtracted from every angle */
  double radius_min;  /* voxels */
  int first_rule, nrules;
} pp_polar_slice;
typedef struct pp_polar_rule {
  int label;          /* 1 ... 32 */
  int flags;          /* PP_POLAR_CW | PP_POLAR_ANY_AREA */
  double angle_min, angle_max;
} pp_polar_rule;
int pp_polar_sectors_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], const pp_polar_slice* slices, const pp_polar_rule* rules,
                        int nrules_total, double area, double min_area_mm2, uint32_t* bits, int64_t* counts);
/* The way back into image space (ventricle.py:660-666, 17 sitk.Resample calls): nearest-neighbour resample of the uint32 bit
 * image `in` on `gin` through the LINEAR transform q = A p + t (NULL: identity) onto `gout`, unpacked: out (DEVICE uint8
 * [nbits][Z][Y][X] on gout) plane k = bit k of the picked voxel, 0 outside the buffer.  Coordinates, inside test and
 * rounding are pp_resample_u8's nearest-neighbour path (the same device functions), so plane k equals pp_resample_u8 of
 * bit k as a uint8 volume, default 0.  nbits in 1 ... 32.  One read of the source, nbits byte planes written. */
int pp_resample_bits_u32(pp_ctx* ctx, const uint32_t* in, const pp_geom* gin, const pp_geom* gout, const double* affine_A,
                         const double* affine_t, int nbits, uint8_t* out);

/* ---- inverse of a displacement field, inverse consistency, Jacobian determinant ---------- */
/* All three: field pointers are DEVICE planar fp32 [3][Z][Y][X] on `geom`, any direction cosines.  A field of 2^32 bytes or
 * more, or an axis longer than 65535: PP_ERR_SIZE, nothing is launched.  Reductions use integer atomics only: two calls on
 * the same inputs return the same bits, images and statistics.  Scratch comes from the ctx workspace. */
typedef struct pp_invert_stats {
  int iterations;          /* iterations executed                                                        */
  int reserved;
  double max_error_norm;   /* max and mean over the voxels of the scaled residual norm, last executed iteration */
  double mean_error_norm;  /* (+inf, +inf when no iteration ran)                                           */
} pp_invert_stats;
/* sitk.InvertDisplacementField(field, maximumNumberOfIterations, maxErrorToleranceThreshold, meanErrorToleranceThreshold,
 * enforceBoundaryCondition) -- the operation the reference names at visualisation/visualiser.py:1536
 * [itk::InvertDisplacementFieldImageFilter, ITK 5.3 as recalled: ITK-upstream, unverified here].  u = field, v = the
 * estimate (initial, or 0 when NULL).  Iteration k = 1, 2, ...: c = v + u_lin(p + v) where the warped point's continuous
 * index idx + diag(1 / spacing) Dir^T v lies in [-0.5, n - 0.5) on every axis (linear interpolation clamped at the edge
 * cells), c = v elsewhere; r = -c; s = sqrt(sum_d (r_d / spacing_d)^2) -- physical components over index-axis spacings,
 * no direction cosines: ITK's quirk --; M = max s, mean = sum s / N; eps = 0.75 in iteration 1 and 0.5 afterwards; where
 * s > eps M, r *= eps M / s; v += eps r; with enforce_boundary, v = 0 on every voxel with an index 0 or n - 1.  The loop
 * runs while k <= max_iterations and M > max_tol and mean > mean_tol, both of iteration k - 1 (+inf before the first): the
 * iteration whose error trips a threshold still applies its own update.  One launch per iteration; the stop test runs on
 * the device and later launches return at once.  max_iterations in 0 ... 256.  inverse_out must alias neither input.
 * stats (HOST, may be NULL): non-NULL synchronises; otherwise the call only enqueues work. */
int pp_invert_field_f32(pp_ctx* ctx, const float* field, const pp_geom* geom, const float* initial, int max_iterations,
                        double max_tol, double mean_tol, int enforce_boundary, float* inverse_out, pp_invert_stats* stats);
/* The residual of a forward / backward pair: iteration 1's c, r, s, M and mean of pp_invert_field_f32 with v = inverse
 * and nothing updated (the same kernel arm; visualiser.py:1536 is where the reference inverts a field).  norm_out (DEVICE
 * fp32 [Z][Y][X], may be NULL) = s.  stats (HOST, required): iterations = 1, max_error_norm = M, mean_error_norm = mean.
 * Synchronises. */
int pp_inverse_consistency_f32(pp_ctx* ctx, const float* field, const float* inverse, const pp_geom* geom, float* norm_out,
                               pp_invert_stats* stats);
typedef struct pp_jacobian_stats {
  double min, max, mean;       /* over the mask's non-zero voxels, or every voxel; NaN when there is none */
  int64_t count;               /* voxels taken                                                            */
  int64_t count_nonpositive;   /* of them, det <= 0 (or NaN): where the field folds                       */
} pp_jacobian_stats;
/* sitk.DisplacementFieldJacobianDeterminant(field, useImageSpacing), the companion of the inversion above
 * (visualiser.py:1536) [itk::DisplacementFieldJacobianDeterminantFilter: ITK-upstream, unverified here]:
 * J[i][j] = 0.5 w_i (u_j(x + e_i) - u_j(x - e_i)) + delta_ij with w_i = 1 / spacing_i (use_image_spacing) or 1, a neighbour
 * outside the buffer being the voxel itself (zero-flux Neumann: a border derivative is half the one-sided difference, an
 * axis of length 1 contributes 0); direction cosines are not applied.  det_out (DEVICE fp32 [Z][Y][X], may be NULL when
 * stats is given) = det J in fp32.  mask (DEVICE uint8, may be NULL) restricts the statistics, never the image.  stats
 * (HOST, may be NULL) come from the same pass: min / max exact, mean from a 2^-24 fixed-point sum, counts exact; non-NULL
 * synchronises, otherwise the call only enqueues work. */
int pp_jacobian_determinant_f32(pp_ctx* ctx, const float* field, const pp_geom* geom, int use_image_spacing, const uint8_t* mask,
                                float* det_out, pp_jacobian_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* PLATIPY_AMD_H */
