"""Drop-in for platipy/imaging/registration/deformable.py:309-547 (bspline_registration).

What the reference hands to sitk.ImageRegistrationMethod with a sitk.BSplineTransform as the optimised transform is rebuilt
around the dense evaluation of the transform (pp_bspline_field_f32) and the similarity metric with its gradient over all
3 cx cy cz control-point coefficients (pp_bspline_metric_f32 for mean squares and correlation; pp_bspline_mi_histogram_f32 and
pp_bspline_mi_gradient_f32 for Mattes mutual information: one workgroup per B-spline cell, no floating-point atomics,
bit-identical between calls).  Levels (shrink factors, smoothing in physical units, REGULAR sampling
with ITK's seeded jitter, the filtered moving-gradient image) are the linear module's; the optimisers run on the host over
the flat parameter vector, as they do in ITK.

ITK rules assumed [ITK-upstream, unverified here: no SimpleITK on any machine this was built on; DESIGN.md section 8]:
  * sitk.BSplineTransformInitializer: transform domain = the fixed image's physical box (continuous index -0.5 .. size - 0.5),
    the image's direction, lattice = mesh + 3 control points per axis, zero coefficients;
  * SetInitialTransformAsBSpline(scaleFactors): level l optimises a lattice of initial mesh x scaleFactors[l] cells, the
    coefficients carried over by itk::BSplineTransformParametersAdaptor (refine_bspline below);
  * a point outside the transform domain maps to itself and contributes no gradient;
  * parameter scales are uniform (every coefficient is a displacement in mm); the gradient-descent learning rate is estimated
    once per level so that the first step's largest shift over the virtual grid is one voxel of the FIRST level's virtual grid.

Deliberate deviations:
  * optimiser "lbfgs" (ITK's LBFGS2 = libLBFGS) is scipy's L-BFGS-B WITHOUT bounds, maxcor = 6 (hessianApproximateAccuracy),
    at most 40 line-search evaluations per iteration (lineSearchMaximumEvaluations), ended by
    |g| / max(1, |x|) <= 1e-2 (solutionAccuracy) or by the iteration count.  scipy's line search is More-Thuente with
    strong-Wolfe conditions as libLBFGS's default is, but with its own constants (ftol 1e-3, gtol 0.9 against libLBFGS's
    1e-4 and lineSearchAccuracy 0.01); the delta-convergence test (tolerance 0.01 over a distance of 0 = off) is not restated;
  * optimiser "lbfgsb" is scipy's fmin_l_bfgs_b as the linear module calls it (m = 5, factr = 1e7, pgtol = 1e-5,
    maxfun = 1024, no bounds), ITK's being the same Fortran code behind another wrapper;
  * Mattes mutual information (the reference's metric="mutual_information", deformable.py:482-485) is spelled
    metric="mattes_mi", as linear_registration spells the same ITK metric; the reference's spelling keeps raising
    NotImplementedError, with a message that names "mattes_mi" -- the arrangement the project already has for
    vote_type="patch_correlation" and fusion.mutual_information.  number_of_histogram_bins_mi must lie in 5..64.  The histogram
    is accumulated in 64-bit fixed point (units of 2^-32 per weight), the bins' intensity range is that of each level's
    smoothed image inside its structure when one is given;
  * "cgls" and the metric "demons" raise NotImplementedError (see bspline_registration);
  * fixed_structure / moving_structure on another grid than their image (always so with isotropic_resample) are resampled onto
    it, nearest neighbour; None means "no mask" as False does;
  * a level whose trial point leaves the overlap reports a large value with a zero gradient to the quasi-Newton optimisers
    (ITK's metric would warn and return its maximum).
"""
import numpy as np
import torch

from .. import _lib, runtime
from ..image import as_image, cast_tensor
from ..transform import BSplineTransform, bspline_transform_initializer, sitkBSpline, sitkNearestNeighbor
from . import _mattes
from . import linear as _linear
from .utils import apply_transform, control_point_spacing_distance_to_number, discrete_gaussian, smooth_and_resample

_METRICS = {"mean_squares": _lib.BSPLINE_MEAN_SQUARES, "correlation": _lib.BSPLINE_CORRELATION, "mattes_mi": None}
_OPTIMISERS = ("lbfgsb", "lbfgs", "cgls", "gradient_descent", "gradient_descent_line_search")
REFINE_PADDING = 12     # control points added on every side of the fine lattice before the prefilter (refine_bspline)


def _basis(t):
    t2, t3, o = t * t, t * t * t, 1.0 - t
    return np.stack([o * o * o / 6.0, (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0, (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0, t3 / 6.0], axis=-1)


def _refine_matrix(n_coarse, mesh_coarse, mesh_fine, pad):
    """[n_fine + 2 pad, n_coarse] fp64: the coarse spline (coefficients beyond its lattice taken as zero) evaluated at the
    positions of the fine lattice's control points, `pad` further ones on either side."""
    n_fine = mesh_fine + 3
    k = np.arange(-pad, n_fine + pad, dtype=np.float64)
    u = 1.0 + (k - 1.0) * (mesh_coarse / float(mesh_fine))      # continuous coarse-lattice index of fine control point k
    fl = np.floor(u)
    w = _basis(u - fl)
    W = np.zeros((k.size, n_coarse))
    for q in range(4):
        idx = fl.astype(np.int64) - 1 + q
        ok = (idx >= 0) & (idx < n_coarse)
        W[np.nonzero(ok)[0], idx[ok]] += w[ok, q]
    return W


def refine_bspline(transform, mesh_size):
    """The same deformation on a lattice of `mesh_size` cells, as itk::BSplineTransformParametersAdaptor carries a transform from
    one level to the next [ITK-upstream, unverified here]: the coarse spline is evaluated at the fine lattice's control-point
    positions (torch, three small matrix products), and pp_bspline_prefilter_f32 turns those samples into coefficients.

    The prefilter's boundary rule is a mirror about the first and the last sample, which the exact fine coefficients do not
    obey; the difference decays by 2 - sqrt(3) = 0.268 per control point from either end.  Run on the bare lattice it would
    leave about 7 % of the coefficient amplitude as an error two cells inside the domain.  The samples are therefore taken
    on the fine lattice grown by REFINE_PADDING control points on every side -- the coarse spline continued with zero
    coefficients, still one cubic spline on the coarse knots and so exactly representable on the fine ones -- and the result
    is cropped: what the mirror rule leaves on the lattice proper is below 0.268^12 = 1.4e-7 of the amplitude, outermost cells
    included."""
    mesh_size = tuple(int(m) for m in mesh_size)
    if mesh_size == tuple(transform.mesh_size):
        return transform
    dev = transform.coefficients.device
    ctx = runtime.context(dev)
    pad = REFINE_PADDING
    coarse = transform.coefficients.double()
    Wx, Wy, Wz = (torch.from_numpy(_refine_matrix(transform.mesh_size[a] + 3, transform.mesh_size[a], mesh_size[a], pad)).to(dev)
                  for a in range(3))
    samples = torch.einsum("kz,jy,ix,czyx->ckji", Wz, Wy, Wx, coarse).float().contiguous()
    size = (samples.shape[3], samples.shape[2], samples.shape[1])
    fine = torch.empty_like(samples)
    for c in range(3):
        ctx.bspline_prefilter(samples[c], size, fine[c])
    fine = fine[:, pad:samples.shape[1] - pad, pad:samples.shape[2] - pad, pad:samples.shape[3] - pad].contiguous()
    return BSplineTransform(mesh_size, transform.domain_origin, transform.domain_dimensions, transform.domain_direction, coefficients=fine)


class _BSplineMetric:
    """value / gradient of one level's similarity metric over the flat coefficient vector: pp_bspline_metric_f32, or -- with
    `mi_bins`, the number of histogram bins of "mattes_mi" -- pp_bspline_mi_histogram_f32, the host's score table
    (_mattes.value_and_table) and pp_bspline_mi_gradient_f32.  A value alone costs the histogram pass only."""

    def __init__(self, ctx, metric, fixed, moving, virtual, stride, transform, fixed_mask, moving_mask, jitter_bound, mi_bins=None):
        self.ctx, self.metric = ctx, metric
        self.ft = (fixed.tensor if fixed.tensor.dtype == torch.float32 else fixed.tensor.float()).contiguous()
        self.mt = (moving.tensor if moving.tensor.dtype == torch.float32 else moving.tensor.float()).contiguous()
        self.fg, self.mg, self.vg = fixed.geom(), moving.geom(), virtual
        self.stride = int(stride)
        self.transform = transform
        self.lg = transform.lattice_geom()
        self.shape = tuple(transform.coefficients.shape)
        self.device = transform.coefficients.device
        self.fmask = None if fixed_mask is None else fixed_mask.tensor.to(torch.uint8).contiguous()
        self.mmask = None if moving_mask is None else moving_mask.tensor.to(torch.uint8).contiguous()
        if self.fmask is not None and tuple(self.fmask.shape) != tuple(self.ft.shape):
            raise ValueError("bspline metric: the fixed mask must be on the fixed image's grid")
        if self.mmask is not None and tuple(self.mmask.shape) != tuple(self.mt.shape):
            raise ValueError("bspline metric: the moving mask must be on the moving image's grid")
        self.jitter_bound = float(jitter_bound)
        self.evaluations = 0
        self.last = None
        self.bins = None
        self.last_hist = None       # mutual information: (x, value, score table) of the last histogram pass
        if mi_bins is not None:
            # the range of the level's smoothed images, inside their masks when there are any (as linear_registration's levels)
            self.bins = _mattes.make_bins(int(mi_bins), _lib.MI_MATTES, _mattes.intensity_range(ctx, self.ft, self.fmask),
                                          _mattes.intensity_range(ctx, self.mt, self.mmask))

    def coefficients(self, x):
        return torch.from_numpy(np.asarray(x, dtype=np.float32).reshape(self.shape)).to(self.device).contiguous()

    def value_and_gradient(self, x):
        """-> (value, float64 gradient); RuntimeError when no sample is valid.  The last evaluation is kept: the optimisers ask for
        the value at the point they have just evaluated (start of a level, end of a level, a line search's accepted probe)."""
        if self.last is not None and np.array_equal(self.last[0], x):
            return self.last[1], self.last[2]
        self.evaluations += 1
        try:
            if self.bins is not None:
                v, table = self._mi_value_and_table(x)
                g, _ = self.ctx.bspline_mi_gradient(self.ft, self.fg, self.mt, self.mg, self.vg, self.stride, self.coefficients(x), self.lg,
                                                    self.bins, table, self.fmask, self.mmask, self.jitter_bound)
            else:
                v, g, _ = self.ctx.bspline_metric(self.metric, self.ft, self.fg, self.mt, self.mg, self.vg, self.stride, self.coefficients(x),
                                                  self.lg, self.fmask, self.mmask, self.jitter_bound)
        except _lib.PlatipyAmdError as e:
            if getattr(e, "code", None) == _lib.ERR_NO_OVERLAP:
                raise RuntimeError("bspline registration: no valid sample points (images do not overlap)") from e
            raise
        self.last = (np.array(x, dtype=np.float64), v, g)
        return v, g

    def _mi_value_and_table(self, x):
        """The histogram pass at x (kept: the gradient pass at the same point reuses it) -> (value, score table)."""
        if self.last_hist is None or not np.array_equal(self.last_hist[0], x):
            hist, stats = self.ctx.bspline_mi_histogram(self.ft, self.fg, self.mt, self.mg, self.vg, self.stride, self.coefficients(x), self.lg,
                                                        self.bins, self.fmask, self.mmask, self.jitter_bound)
            self.last_hist = (np.array(x, dtype=np.float64),) + _mattes.value_and_table("mattes_mi", hist, stats["valid"], self.bins.m_bin)
        return self.last_hist[1], self.last_hist[2]

    def value(self, x):
        if self.bins is None or (self.last is not None and np.array_equal(self.last[0], x)):
            return self.value_and_gradient(x)[0]
        if self.last_hist is None or not np.array_equal(self.last_hist[0], x):
            self.evaluations += 1
        try:
            return self._mi_value_and_table(x)[0]
        except _lib.PlatipyAmdError as e:
            if getattr(e, "code", None) == _lib.ERR_NO_OVERLAP:
                raise RuntimeError("bspline registration: no valid sample points (images do not overlap)") from e
            raise

    def values(self, xs):
        out = []
        for x in xs:
            try:
                out.append(self.value(x))
            except RuntimeError:
                out.append(float("inf"))
        return out

    def step_scale(self, x, step):
        """Largest shift (mm) over the virtual grid that adding `step` to the coefficients causes: the transform is linear in
        its coefficients, so that is the largest norm of the step's own displacement field."""
        size = (int(self.vg.size[0]), int(self.vg.size[1]), int(self.vg.size[2]))
        field = torch.empty((3, size[2], size[1], size[0]), dtype=torch.float32, device=self.device)
        self.ctx.bspline_field(self.coefficients(step), self.lg, self.vg, field)
        return float(torch.sqrt((field.double() ** 2).sum(0)).max())


def _structure_on(structure, image):
    """`structure` (False or None: no mask) as a uint8 Image on `image`'s grid."""
    if structure is False or structure is None:
        return None
    structure = as_image(structure)
    if structure.is_vector:
        raise ValueError("bspline_registration: a structure is a scalar image")
    structure = structure.like((structure.tensor != 0).to(torch.uint8))
    if not structure.same_grid(image):
        structure = apply_transform(structure, image, None, 0, sitkNearestNeighbor)
    return structure


class _Converged(Exception):
    pass


def _lbfgs(ms, x0, number_of_iterations, verbose):
    """ITK's LBFGS2 settings on scipy's L-BFGS-B without bounds (module docstring, deliberate deviations)."""
    from scipy.optimize import minimize

    state = {"it": 0, "x": np.array(x0, dtype=np.float64)}
    start = ms.value(x0)

    def fun(x):
        try:
            v, g = ms.value_and_gradient(x)
        except RuntimeError:
            return 10.0 * abs(start) + 1.0, np.zeros_like(x)
        return v, g

    def callback(xk):
        state["it"] += 1
        state["x"] = np.array(xk, dtype=np.float64)
        lx, lv, lg = ms.last
        if verbose:
            print("{0:3} = {1:10.5f}".format(state["it"], lv))
        if np.array_equal(lx, xk) and np.linalg.norm(lg) / max(1.0, np.linalg.norm(xk)) <= 1e-2:      # solutionAccuracy
            raise _Converged

    try:
        res = minimize(fun, np.array(x0, dtype=np.float64), jac=True, method="L-BFGS-B", callback=callback,
                       options={"maxcor": 6, "maxls": 40, "maxiter": int(number_of_iterations), "ftol": 0.0, "gtol": 0.0,
                                "maxfun": 41 * int(number_of_iterations) + 1})
        x = res.x
    except _Converged:
        x = state["x"]
    return x


def bspline_registration(
    fixed_image,
    moving_image,
    fixed_structure=False,
    moving_structure=False,
    resolution_staging=[8, 4, 2],
    smooth_sigmas=[4, 2, 1],
    sampling_rate=0.1,
    optimiser="LBFGS",
    metric="mean_squares",
    initial_grid_spacing=64,
    grid_scale_factors=[1, 2, 4],
    interp_order=sitkBSpline,
    default_value=-1000,
    number_of_iterations=20,
    isotropic_resample=False,
    initial_isotropic_size=1,
    number_of_histogram_bins_mi=30,
    verbose=False,
    ncores=8,
    itk_sampling=True,
):
    """B-spline (free-form deformation) registration (reference registration/deformable.py:309-547).

    -> (registered_image, BSplineTransform).  Arguments and defaults are the reference's; metric: "mean_squares", "correlation" or
    "mattes_mi" (Mattes mutual information with number_of_histogram_bins_mi bins, 5..64 -- the reference's "mutual_information",
    spelled as linear_registration spells it; the reference's spelling raises NotImplementedError and says so); `ncores` is accepted and ignored (the
    work runs on the GPU); `itk_sampling` as in linear_registration: True moves every sample point by ITK's seeded jitter and
    takes the moving gradient from ITK's filtered gradient image, False samples on the lattice with the analytic gradient of
    the trilinear interpolant.  The returned transform carries `.level_values`: the (first, last) metric value of each level."""
    opt = str(optimiser).lower()
    if metric == "mutual_information":
        raise NotImplementedError('bspline_registration: Mattes mutual information over a B-spline transform is metric="mattes_mi" '
                                  "(the spelling linear_registration uses for the same ITK metric)")
    if metric == "demons":
        raise NotImplementedError("bspline_registration: ITK's demons metric (v4) accepts displacement-field transforms only and so "
                                  "rejects a B-spline transform [ITK-upstream, unverified here]")
    if metric not in _METRICS:
        raise ValueError(f"bspline_registration: unknown metric {metric!r}")
    if opt not in _OPTIMISERS:
        raise ValueError(f"bspline_registration: unknown optimiser {optimiser!r}")
    if opt == "cgls":
        raise NotImplementedError("bspline_registration: the conjugate-gradient line-search optimiser (cgls) is not built yet")
    mi_bins = None
    if metric == "mattes_mi":
        mi_bins = int(number_of_histogram_bins_mi)
        if not 5 <= mi_bins <= 64:
            raise ValueError(f"bspline_registration: number_of_histogram_bins_mi must be in 5..64 (2 padding bins on either side, at most "
                             f"64 x 64 bins in the kernels' LDS table), got {number_of_histogram_bins_mi}")
    levels = len(resolution_staging)
    if len(smooth_sigmas) != levels or len(grid_scale_factors) != levels:
        raise ValueError("bspline_registration: resolution_staging, smooth_sigmas and grid_scale_factors need one entry per level")
    if isinstance(sampling_rate, (list, tuple, np.ndarray)):
        rates = [float(r) for r in sampling_rate]
        if len(rates) != levels:
            raise ValueError("bspline_registration: a per-level sampling_rate needs one entry per level")
    else:
        rates = [float(sampling_rate)] * levels

    fixed_image = as_image(fixed_image)
    moving_image = as_image(moving_image)
    moving_image_type = moving_image.tensor.dtype
    fixed_image = fixed_image.astype(torch.float32)
    moving_image = moving_image.astype(torch.float32)
    fixed_image_original = fixed_image
    if isotropic_resample:
        fixed_image = smooth_and_resample(fixed_image, isotropic_voxel_size_mm=initial_isotropic_size)
        moving_image = smooth_and_resample(moving_image, isotropic_voxel_size_mm=initial_isotropic_size)
    # ITK's masks live in physical space; the kernel indexes a mask with its image's strides.  A structure on another grid than
    # the image the kernel gets (isotropic_resample, or simply a label drawn elsewhere) is resampled onto it, nearest neighbour.
    fixed_mask = _structure_on(fixed_structure, fixed_image)
    moving_mask = _structure_on(moving_structure, moving_image)

    ctx = runtime.context(fixed_image.device)
    initial_mesh = [max(1, int(i)) for i in control_point_spacing_distance_to_number(fixed_image, initial_grid_spacing)]
    if verbose:
        print(f"Initial grid size: {initial_mesh}")
    transform = bspline_transform_initializer(fixed_image, initial_mesh, device=fixed_image.device)

    jitter = _linear._JitterSource(42, fixed_image.device) if itk_sampling else None
    max_step = None
    level_values = []
    try:
        for level, (shrink, sigma, scale, rate) in enumerate(zip(resolution_staging, smooth_sigmas, grid_scale_factors, rates)):
            f_l = discrete_gaussian(fixed_image, sigma * sigma) if sigma > 0 else fixed_image
            m_l = discrete_gaussian(moving_image, sigma * sigma) if sigma > 0 else moving_image
            vsize, vspacing, vorigin, vdir = _linear._shrink_geometry(fixed_image, shrink)
            virtual = _lib.make_geom(vsize, vspacing, vorigin, vdir.ravel())
            stride = int(np.ceil(1.0 / rate)) if rate < 1.0 else 1
            if max_step is None:
                max_step = float(np.min(vspacing))
            transform = refine_bspline(transform, [m * int(scale) for m in initial_mesh])
            jitter_bound = 0.0
            if jitter is not None:
                jit = jitter.level([int(v) for v in vsize], stride, vspacing, vdir)
                ctx.set_sample_jitter(jit)
                jitter_bound = float(jit.abs().max())
                grad = _linear.itk_moving_gradient(ctx, m_l)
                packed = None       # (gradient, intensity) as one 16-byte element per corner where the lattice is large enough to pay
                if grad.is_cuda and int(np.prod(vsize)) / stride >= _linear.PACKED_GRADIENT_MIN_SAMPLES:      # for the copy, as linear.py
                    packed = torch.stack((grad[0], grad[1], grad[2], m_l.tensor.float()), dim=-1)
                ctx.set_moving_gradient(grad, packed=packed)
            ms = _BSplineMetric(ctx, _METRICS[metric], f_l, m_l, virtual, stride, transform, fixed_mask, moving_mask, jitter_bound,
                                mi_bins=mi_bins)
            x = np.asarray(transform.coefficients.detach().reshape(-1).cpu().numpy(), dtype=np.float64)
            first = ms.value(x)
            if verbose:
                print(f"level {level}: shrink {shrink}, sigma {sigma}, mesh {transform.mesh_size}, {x.size} parameters, start {first:.6f}")
            if opt == "lbfgsb":
                from scipy.optimize import fmin_l_bfgs_b

                def fun(p):
                    try:
                        v, g = ms.value_and_gradient(p)
                    except RuntimeError:
                        return 10.0 * abs(first) + 1.0, np.zeros_like(p)
                    if verbose:
                        print("{0:3} = {1:10.5f}".format(ms.evaluations, v))
                    return v, g

                x, _, _ = fmin_l_bfgs_b(fun, x, m=5, factr=1e7, pgtol=1e-5, maxiter=number_of_iterations, maxfun=1024)
            elif opt == "lbfgs":
                x = _lbfgs(ms, x, number_of_iterations, verbose)
            else:
                x = _linear.gradient_descent_level(ms.value_and_gradient, ms.values, ms.value, lambda p, step: p + step, np.ones_like(x),
                                                   ms.step_scale, x, opt, number_of_iterations, max_step, verbose)
            last = ms.value(x)
            level_values.append((first, last))
            transform = BSplineTransform(transform.mesh_size, transform.domain_origin, transform.domain_dimensions,
                                         transform.domain_direction, coefficients=ms.coefficients(x))
    finally:
        if jitter is not None:
            ctx.set_sample_jitter(None)
            ctx.set_moving_gradient(None)
            jitter.close()
    transform.level_values = level_values

    registered_image = apply_transform(input_image=moving_image, reference_image=fixed_image_original, transform=transform,
                                       default_value=default_value, interpolator=interp_order)
    registered_image = registered_image.like(cast_tensor(registered_image.tensor, moving_image_type))
    return registered_image, transform
