"""Host arithmetic of the mutual-information metrics, shared by linear_registration (pp_mi_histogram_f32 / pp_mi_gradient_f32)
and bspline_registration (pp_bspline_mi_histogram_f32 / pp_bspline_mi_gradient_f32): the intensity range and the bins of a
level, and what turns a joint histogram of at most 64 x 64 numbers into the metric value and the per-bin score table of the
gradient pass."""
import numpy as np
import torch

MI_PADDING = 2


def intensity_range(ctx, image, mask):
    """(min, max) of `image` INSIDE `mask` when one is given (both ITK v4 MI metrics' Initialize() walk the image and skip
    points outside the mask); an empty mask leaves the whole image."""
    if mask is not None:
        inside = mask != 0
        if bool(inside.any()):
            inf = torch.tensor(float("inf"), dtype=image.dtype, device=image.device)
            return float(torch.where(inside, image, inf).min()), float(torch.where(inside, image, -inf).max())
    return ctx.minmax(image, image.numel())


def make_bins(nbins, kernel, fixed_range, moving_range):
    """pp_mi_bins by itk::MattesMutualInformation...::Initialize: bin = (max - min) / (bins - 2 padding), normalised
    min = min / bin - padding."""
    from .._lib import MiBins

    (f_lo, f_hi), (m_lo, m_hi) = fixed_range, moving_range
    b = MiBins()
    b.nbins, b.kernel = int(nbins), int(kernel)
    b.f_bin = max((f_hi - f_lo) / (nbins - 2 * MI_PADDING), 1e-30)
    b.m_bin = max((m_hi - m_lo) / (nbins - 2 * MI_PADDING), 1e-30)
    b.f_norm_min = f_lo / b.f_bin - MI_PADDING
    b.m_norm_min = m_lo / b.m_bin - MI_PADDING
    return b


def value_and_table(metric, hist, count, m_bin, lib=None, smoothing_variance=None):
    """Joint histogram -> (negative mutual information, per-bin score table for the gradient pass).  metric: "mattes_mi" or
    "joint_hist_mi" (which smooths the PDF with ITK's Gaussian of `smoothing_variance`, taps from the loaded library `lib`)."""
    eps = 1e-16
    if metric == "mattes_mi":
        P = hist / hist.sum()
    else:
        from scipy.ndimage import correlate1d

        from .._lib import gauss_taps

        taps = np.asarray(gauss_taps(smoothing_variance, 0.01, 32, lib=lib))   # ITK's DiscreteGaussian on the PDF image
        P = correlate1d(correlate1d(hist / count, taps, axis=0, mode="nearest"), taps, axis=1, mode="nearest")
    PF, PM = P.sum(1), P.sum(0)
    ok = (P > eps) & (PF[:, None] > eps) & (PM[None, :] > eps)
    safe = np.where(ok, P, 1.0)
    value = -float((np.where(ok, P * np.log(safe / np.where(ok, PF[:, None] * PM[None, :], 1.0)), 0.0)).sum())
    ratio = np.where(ok, np.log(safe / np.where(ok, np.broadcast_to(PM[None, :], P.shape), 1.0)), 0.0)
    # Mattes: d value / d mu = sum_s sum_k B3'(k - u_s) table[f_s][k] (grad M . dT/dmu), table = log(P / PM) / (N bin)
    # joint:  d value / d mu = -(1/N) sum_s d/dm [log P - log PM](f_s, m_s) (grad M . dT/dmu), differenced between bin centres
    scale = 1.0 / (count * m_bin)
    table = ratio * scale if metric == "mattes_mi" else -ratio * scale
    return value, table
