"""fp64 restatements of the two Gaussian smoothers (numpy / scipy only, no project code), the references of
tests/test_smoothing_kernels.py.

FIR  itk::DiscreteGaussianImageFilter and the demons field smoothers: a separable correlation with the taps of
     itk::GaussianOperator, ZeroFluxNeumann (edge-value) boundaries, one axis after the other.  `fir_separable` takes the
     taps as given (the tests hand it the library's own fp32 taps, so that what is compared is the convolution);
     `gaussian_operator_bessel` builds the operator from the exact scaled Bessel functions scipy.special.ive.
IIR  itk::RecursiveGaussianImageFilter: Deriche's fourth-order recursion, a causal and an anti-causal sweep per line with
     edge-value extension, the line filtered in fp64 and the result stored as fp32.

All arrays are [Z][Y][X]; `axis` arguments are numpy axes of that array.
"""
import numpy as np
from scipy.ndimage import correlate1d
from scipy.special import ive


# --------------------------------------------------------------------------------------
# FIR


def fir_separable(img, taps_by_axis, order):
    """correlate1d(mode="nearest") in fp64 along the numpy axes of `order`, in that order; taps_by_axis[axis] are that axis's taps."""
    out = np.asarray(img, dtype=np.float64)
    for axis in order:
        out = correlate1d(out, np.asarray(taps_by_axis[axis], dtype=np.float64), axis=axis, mode="nearest")
    return out


def gaussian_operator_bessel(var, max_error, max_width):
    """itk::GaussianOperator::GenerateCoefficients with exact Bessel values: e^-var I_k(var) from the centre outwards (the
    centre and its neighbour always) until the covered mass reaches 1 - max_error, no further mass can be gained, or the half
    kernel holds max_width + 1 coefficients; then normalised.  Returns the 2 r + 1 taps."""
    half = [float(ive(0, var)), float(ive(1, var))]
    mass = half[0] + 2.0 * half[1]
    k = 2
    while mass < 1.0 - max_error:
        half.append(float(ive(k, var)))
        mass += 2.0 * half[k]
        if half[k] < mass * np.finfo(np.float64).eps or len(half) > max_width:
            break
        k += 1
    h = np.asarray(half) / mass
    return np.concatenate([h[:0:-1], h])


# --------------------------------------------------------------------------------------
# IIR


def deriche_coefficients(sigma, spacing, order=0, scale=1.0):
    """itk::RecursiveGaussianImageFilter::SetUp: the causal (N), anti-causal (M) and recursive (D) coefficients for sigma in
    physical units on an axis of `spacing` (its sign does not enter here).  order 0: the Gaussian, unit DC gain; order 1:
    its first derivative per voxel times `scale`, antisymmetric.  kn / km are the steady-state gains of the two halves for a
    constant line, which is what the edge-value extension starts each sweep from."""
    sd = sigma / abs(spacing)
    W1, L1, W2, L2 = 0.6681, -1.3932, 2.0787, -1.3732
    if order == 0:
        A1, B1, A2, B2 = 1.3530, 1.8151, -0.3531, 0.0902
    else:
        A1, B1, A2, B2 = -0.6724, -3.4327, 0.6724, 0.6100
    c1, c2, s1, s2 = np.cos(W1 / sd), np.cos(W2 / sd), np.sin(W1 / sd), np.sin(W2 / sd)
    e1, e2 = np.exp(L1 / sd), np.exp(L2 / sd)
    d4 = e1 * e1 * e2 * e2
    d3 = -2 * c1 * e1 * e2 * e2 + -2 * c2 * e2 * e1 * e1
    d2 = 4 * c2 * c1 * e1 * e2 + e1 * e1 + e2 * e2
    d1 = -2 * (e2 * c2 + e1 * c1)
    SD = 1.0 + d1 + d2 + d3 + d4
    DD = d1 + 2 * d2 + 3 * d3 + 4 * d4
    n0 = A1 + A2
    n1 = e2 * (B2 * s2 - (A2 + 2 * A1) * c2) + e1 * (B1 * s1 - (A1 + 2 * A2) * c1)
    n2 = 2 * e1 * e2 * ((A1 + A2) * c2 * c1 - (B1 * c2 * s1 + B2 * c1 * s2)) + A2 * e1 * e1 + A1 * e2 * e2
    n3 = e2 * e1 * e1 * (B2 * s2 - A2 * c2) + e1 * e2 * e2 * (B1 * s1 - A1 * c1)
    SN = n0 + n1 + n2 + n3
    DN = n1 + 2 * n2 + 3 * n3
    if order == 0:
        norm = 1.0 / (2 * SN / SD - n0)
    else:
        norm = scale / (2 * (SN * DD - DN * SD) / (SD * SD))
    n0, n1, n2, n3 = n0 * norm, n1 * norm, n2 * norm, n3 * norm
    sgn = 1.0 if order == 0 else -1.0
    m1, m2, m3, m4 = sgn * (n1 - d1 * n0), sgn * (n2 - d2 * n0), sgn * (n3 - d3 * n0), sgn * (-d4 * n0)
    return dict(n=(n0, n1, n2, n3), d=(d1, d2, d3, d4), m=(m1, m2, m3, m4), kn=(n0 + n1 + n2 + n3) / SD, km=(m1 + m2 + m3 + m4) / SD)


def deriche_pass(a, axis, sigma, spacing, order=0, scale=1.0, store_fp32=True):
    """One directional pass over every line of `a` along `axis`.  Both sweeps run in fp64 from the steady state of the line's
    edge value; the causal half is rounded to fp32 before the sum and the sum is rounded to fp32 (store_fp32=False keeps
    everything in fp64: the filter itself, for impulse_gain)."""
    k = deriche_coefficients(sigma, spacing, order, scale)
    (n0, n1, n2, n3), (d1, d2, d3, d4), (m1, m2, m3, m4) = k["n"], k["d"], k["m"]
    x = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    n = x.shape[0]
    causal = np.empty_like(x)
    x1 = x2 = x3 = x[0]
    y1 = y2 = y3 = y4 = x[0] * k["kn"]
    for i in range(n):
        y = (n0 * x[i] + n1 * x1 + n2 * x2 + n3 * x3) - (d1 * y1 + d2 * y2 + d3 * y3 + d4 * y4)
        x3, x2, x1 = x2, x1, x[i]
        y4, y3, y2, y1 = y3, y2, y1, y
        causal[i] = y
    if store_fp32:
        causal = causal.astype(np.float32).astype(np.float64)
    out = np.empty_like(x)
    x1 = x2 = x3 = x4 = x[n - 1]
    y1 = y2 = y3 = y4 = x[n - 1] * k["km"]
    for i in range(n - 1, -1, -1):
        y = (m1 * x1 + m2 * x2 + m3 * x3 + m4 * x4) - (d1 * y1 + d2 * y2 + d3 * y3 + d4 * y4)
        x4, x3, x2, x1 = x3, x2, x1, x[i]
        y4, y3, y2, y1 = y3, y2, y1, y
        out[i] = causal[i] + y
    out = np.moveaxis(out, 0, axis)
    return np.ascontiguousarray(out.astype(np.float32) if store_fp32 else out)


def impulse_gain(sigma, spacing, order=0, scale=1.0):
    """L1 norm of the pass's response to a unit impulse in the middle of a line of 257 voxels: max |out| <= gain * max |in|."""
    line = np.zeros(257)
    line[128] = 1.0
    return float(np.abs(deriche_pass(line, 0, sigma, spacing, order, scale, store_fp32=False)).sum())
