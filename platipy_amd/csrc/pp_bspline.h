// platipy_amd/csrc/pp_bspline.h -- cubic B-spline transform on the GPU: dense evaluation and the similarity metric with its
// gradient over all control-point coefficients (pp_bspline_field_f32, pp_bspline_metric_f32; Mattes mutual information in two
// passes: pp_bspline_mi_histogram_f32, pp_bspline_mi_gradient_f32).  Included at the end of pp_linear.hip.
//
// Replaces what sitk.ImageRegistrationMethod does per iteration with a sitk.BSplineTransform as its optimised transform
// (platipy/imaging/registration/deformable.py:309-547) and what sitk.Resample / TransformToDisplacementField do with one
// [ITK-upstream, restated; parity unpinned -- DESIGN.md section 8].
//
// Conventions.  The lattice is a planar fp32 array [3][cz][cy][cx] with its own pp_geom; a point with continuous lattice index
// u is inside the transform domain when 1 <= u < mesh + 1 on every axis (mesh = lattice size - 3), its cell is floor(u) - 1 and
// its 4 x 4 x 4 support starts at lattice index floor(u) - 1.  Outside the domain the transform is the identity.
//
// Kernel A (k_bsp_field): one thread per output voxel, 64 x 3 coefficient reads from a lattice of kilobytes (L1 / L2 resident),
// 12 bytes written.  DESIGNED AGAINST THE WRITE BOUND: 12 B/voxel of compulsory stores; the products run in fp64 (192 FMAs per
// voxel: 13 GFLOP at 512 x 512 x 256, about 0.2 ms at the card's vector fp64 rate, the same order as the 0.2 ms the 805 MB of
// stores need), so that constant coefficients come back exact to the last fp32 bit.  When the lattice axes are the grid's axes
// (any spacing, origin, axis flip) the weights of an axis depend on the index along that axis alone: a first kernel writes four
// weights and a support base per index (k_bsp_tables, nx + ny + nz entries) and the voxel kernel reads three entries.
//
// Kernel B (k_bsp_metric): ONE WORKGROUP PER B-SPLINE CELL (times a few z-slabs of the cell when the mesh has fewer cells than
// the card has room for).  Every sample of a cell shares its 64 control points, so the 192 (mean squares) or 576 (correlation)
// gradient sums of the cell live in REGISTERS of 192 threads and nothing is scattered: the workgroup stages 256 samples at a
// time in LDS (3 gradient terms in fp64, 12 axis weights, f, m, a status word: 24 KB), then thread (component r, control point
// i j k) walks the staged samples IN SLOT ORDER and adds g_r w_i w_j w_k in fp64, ten further threads add the scalar moments
// the same way.  A sample belongs to the cell of its JITTERED position; a workgroup therefore scans its cell's voxel box grown
// by the jitter bound and drops what it does not own, so the support is always exactly the cell's 4 x 4 x 4 and ITK's unbounded
// normal jitter needs no wider window.  Per cell one row of fp64 partial sums goes to the workspace (1.6 KB / 4.7 KB); a gather
// kernel adds, for every coefficient, the rows of the <= 64 cells that cover it in a fixed order and applies the metric's
// normalisation (k_bsp_gather).  No floating-point atomics anywhere and no dependence on the order in which workgroups run: two
// calls return the same bits.  DESIGNED AGAINST LDS BANDWIDTH: the staged walk reads 4 LDS words per fp64 FMA, 768 lane-reads per
// sample, about 24 cycles per sample and CU -- 67 M samples in under 3 ms on 256 CUs; the image gathers (8 corners, 32 or 128 B
// per sample) stay below that.  THESE FIGURES ARE A MODEL, NOT A MEASUREMENT, and they count owned samples only: every
// workgroup also stages the candidates of its margin (ceil(jitter bound) + 1 voxels on every side, 3 with ITK's jitter) and drops
// them after the ownership test, so on a shrunk level whose cells are ~8 voxels wide about five candidates go through the staging
// loop and its two barriers per owned sample; without jitter the margin is 1.
// MEASURED (MI355X, 512 x 512 x 256): kernel A 1.8 - 1.9 ms (430 GB/s, a ninth of its bound: the fp64 sum and
// its 192 cached loads per voxel are the cost); kernel B 34 - 48 ms per evaluation at 67 M samples, 12 - 16x the model above.  LDS per workgroup is 24 KB of the CU's 160 KB, so occupancy is set by the 256 threads, not by LDS.
//
// Mattes mutual information (reference deformable.py:482-485) scans the same rows twice.  Pass 1 (k_bsp_mi_hist) bins every valid
// sample into a 64-bit fixed-point LDS histogram with integer atomics, a bounded grid walking the rows; pass 2 is MODE 2 of kernel
// B with the host's score table in LDS.  Both evaluate a sample through bsp_sample, as modes 0 and 1 do.  MEASURED (MI355X, 512 x
// 512 x 256, 30 bins, mesh 8 x 8 x 4 / 32 x 32 x 16, rate 1.0): pass 1 5.0 / 6.0 ms, pass 2 47.5 / 34.3 ms beside 46.1 / 33.1 ms for mean squares.
#pragma once

#include "pp_reduce.h"

namespace {

constexpr int BSP_NT = 256;
constexpr int BSP_NSCAL = 10;   // count, sum f, sum m, sum f^2, sum m^2, sum f m, sum (f - m)^2, outside, masked, seen
enum { BSP_VALID = 1, BSP_GRAD = 2, BSP_OUTSIDE = 4, BSP_MASKED = 8, BSP_SEEN = 16 };

// uniform cubic B-spline basis at fraction t in [0, 1): weights of control points floor(u) - 1 .. floor(u) + 2
__host__ __device__ inline void bsp_weights(double t, double w[4]) {
  const double t2 = t * t, t3 = t2 * t, o = 1.0 - t;
  w[0] = o * o * o / 6.0;
  w[1] = (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0;
  w[2] = (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0;
  w[3] = t3 / 6.0;
}

// one axis of itk::BSplineTransform::InsideValidRegion + the support: false outside [1, mesh + 1)
__device__ inline bool bsp_axis(double u, int mesh, int& base, double w[4]) {
  if (!(u >= 1.0 && u < mesh + 1.0)) return false;
  const double fl = floor(u);
  base = (int)fl - 1;
  bsp_weights(u - fl, w);
  return true;
}

struct bsp_field_args {
  double A[9], b[3];   // grid index -> continuous lattice index
  int n[3];            // grid size
  int lat[3];          // lattice size
};

__global__ void __launch_bounds__(BSP_NT) k_bsp_tables(bsp_field_args a, int* __restrict__ tb, double* __restrict__ tw) {
  const int i = blockIdx.x * BSP_NT + threadIdx.x;
  if (i >= a.n[0] + a.n[1] + a.n[2]) return;
  const int axis = i < a.n[0] ? 0 : (i < a.n[0] + a.n[1] ? 1 : 2);
  const int idx = i - (axis == 0 ? 0 : (axis == 1 ? a.n[0] : a.n[0] + a.n[1]));
  const double u = a.A[axis * 3 + axis] * idx + a.b[axis];
  int base = -1;
  double w[4] = {0.0, 0.0, 0.0, 0.0};
  if (!bsp_axis(u, a.lat[axis] - 3, base, w)) base = -1;
  tb[i] = base;
  for (int k = 0; k < 4; ++k) tw[4 * (size_t)i + k] = w[k];
}

template <bool ALIGNED>
__global__ void __launch_bounds__(BSP_NT) k_bsp_field(const float* __restrict__ C, bsp_field_args a, const int* __restrict__ tb,
                                                      const double* __restrict__ tw, float* __restrict__ out) {
  const size_t n = (size_t)a.n[0] * a.n[1] * a.n[2];
  const size_t ncp = (size_t)a.lat[0] * a.lat[1] * a.lat[2];
  for (size_t v = (size_t)blockIdx.x * BSP_NT + threadIdx.x; v < n; v += (size_t)gridDim.x * BSP_NT) {
    const int x = (int)(v % a.n[0]), y = (int)((v / a.n[0]) % a.n[1]), z = (int)(v / ((size_t)a.n[0] * a.n[1]));
    int bx = -1, by = -1, bz = -1;
    double wx[4], wy[4], wz[4];
    bool in;
    if (ALIGNED) {
      bx = tb[x];
      by = tb[a.n[0] + y];
      bz = tb[a.n[0] + a.n[1] + z];
      in = bx >= 0 && by >= 0 && bz >= 0;
      if (in)
        for (int k = 0; k < 4; ++k) {
          wx[k] = tw[4 * (size_t)x + k];
          wy[k] = tw[4 * (size_t)(a.n[0] + y) + k];
          wz[k] = tw[4 * (size_t)(a.n[0] + a.n[1] + z) + k];
        }
    } else {
      double u[3];
      for (int r = 0; r < 3; ++r) u[r] = a.A[r * 3 + 0] * x + a.A[r * 3 + 1] * y + a.A[r * 3 + 2] * z + a.b[r];
      in = bsp_axis(u[0], a.lat[0] - 3, bx, wx);
      in = bsp_axis(u[1], a.lat[1] - 3, by, wy) && in;
      in = bsp_axis(u[2], a.lat[2] - 3, bz, wz) && in;
    }
    double d[3] = {0.0, 0.0, 0.0};
    if (in) {
      for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 4; ++j) {
          const double wyz = wy[j] * wz[k];
          const float* row = C + ((size_t)(bz + k) * a.lat[1] + (by + j)) * a.lat[0] + bx;
          for (int r = 0; r < 3; ++r) {
            const float* rr = row + r * ncp;
            const double t = wx[0] * (double)rr[0] + wx[1] * (double)rr[1] + wx[2] * (double)rr[2] + wx[3] * (double)rr[3];
            d[r] += wyz * t;
          }
        }
    }
    out[v] = (float)d[0];
    out[n + v] = (float)d[1];
    out[2 * n + v] = (float)d[2];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// metric

struct bsp_metric_args {
  double Af[9], bf[3];   // virtual index -> fixed index
  double Am[9], bm[3];   // virtual index -> moving index (identity transform)
  double Md[9];          // physical displacement (mm) -> moving index units; also d m / d c_r = sum_q g_idx[q] Md[q][r]
  double Au[3], bu[3];   // virtual index -> continuous lattice index, per axis (the directions agree)
  int vsize[3], stride;
  int lat[3], mesh[3];
  int margin, nsplit;
  const float* jit;      // as msq_args of pp_fusion.hip
  const float* grad;
  const float4* grad4;
};

__device__ __forceinline__ bool bsp_locate(const double c[3], const pp_dims& n, int b[3], float f[3]) {
  if (!(c[0] >= -0.5 && c[0] < n.nx - 0.5 && c[1] >= -0.5 && c[1] < n.ny - 0.5 && c[2] >= -0.5 && c[2] < n.nz - 0.5)) return false;
  for (int k = 0; k < 3; ++k) {
    const double fl = floor(c[k]);
    b[k] = (int)fl;
    f[k] = (float)(c[k] - fl);
  }
  return true;
}

// the nested lerps of pp_trilinear over eight corner values, x fastest
__device__ __forceinline__ float bsp_lerp8(const float a[8], float wx, float wy, float wz) {
  const float v00 = a[0] + (a[1] - a[0]) * wx, v10 = a[2] + (a[3] - a[2]) * wx;
  const float v01 = a[4] + (a[5] - a[4]) * wx, v11 = a[6] + (a[7] - a[6]) * wx;
  const float v0 = v00 + (v10 - v00) * wy, v1 = v01 + (v11 - v01) * wy;
  return v0 + (v1 - v0) * wz;
}

// voxel range [lo, hi] along one axis that can hold samples of cell `c` (jitter within `margin` voxels included)
__device__ __forceinline__ void bsp_cell_range(double Au, double bu, int c, int mesh, int n, int margin, int& lo, int& hi) {
  const double l = ceil((c + 1.0 - bu) / Au), h = ceil((c + 2.0 - bu) / Au);
  lo = c == 0 ? 0 : (l - margin < 0.0 ? 0 : (l - margin > n ? n : (int)(l - margin)));
  hi = c == mesh - 1 ? n - 1 : (h - 1.0 + margin > n - 1.0 ? n - 1 : (h - 1.0 + margin < -1.0 ? -1 : (int)(h - 1.0 + margin)));
}

// Mattes bins of the two mutual-information passes (pp_mi_bins, PP_MI_MATTES) and, for pass 2, the score table
struct bsp_mi_args {
  int nbins;
  double f_bin, f_norm_min, m_bin, m_norm_min;
  const float* table;   // device, [nbins * nbins] fp32, row = fixed bin (pass 2 only)
};

// What one workgroup scans for row `row` = (cell, z slab): the cell, its voxel box grown by the jitter margin and cut to the
// slab, and the number of candidate samples (items) in it.
struct bsp_box {
  int ci, cj, ck;
  int xlo, xhi, ylo, zlo, by, kmax;
  long long items;
};

__device__ __forceinline__ bsp_box bsp_row_box(const bsp_metric_args& a, int row) {
  bsp_box b;
  const int cell = row / a.nsplit, split = row % a.nsplit;
  b.ci = cell % a.mesh[0], b.cj = (cell / a.mesh[0]) % a.mesh[1], b.ck = cell / (a.mesh[0] * a.mesh[1]);
  int yhi, zlo, zhi;
  bsp_cell_range(a.Au[0], a.bu[0], b.ci, a.mesh[0], a.vsize[0], a.margin, b.xlo, b.xhi);
  bsp_cell_range(a.Au[1], a.bu[1], b.cj, a.mesh[1], a.vsize[1], a.margin, b.ylo, yhi);
  bsp_cell_range(a.Au[2], a.bu[2], b.ck, a.mesh[2], a.vsize[2], a.margin, zlo, zhi);
  {   // this row's z slab of the box
    const int len = zhi - zlo + 1 > 0 ? (zhi - zlo + 1 + a.nsplit - 1) / a.nsplit : 0;
    const int z0 = zlo + split * len, z1 = z0 + len - 1;
    zlo = z0;
    zhi = z1 < zhi ? z1 : zhi;
  }
  b.zlo = zlo;
  const int bx = b.xhi - b.xlo + 1, bz = zhi - zlo + 1;
  b.by = yhi - b.ylo + 1;
  b.kmax = bx > 0 ? (bx + a.stride - 1) / a.stride : 0;
  b.items = (bx > 0 && b.by > 0 && bz > 0) ? (long long)b.kmax * b.by * bz : 0;
  return b;
}

// Candidate `item` of a box -> its voxel and its index `e` in the raster walk of the sampling lattice; false where the row of
// the box holds fewer samples than kmax.
__device__ __forceinline__ bool bsp_box_item(const bsp_metric_args& a, const bsp_box& b, long long item, int& x, int& y, int& z, size_t& e) {
  const long long row = item / b.kmax;
  const int k = (int)(item % b.kmax);
  y = b.ylo + (int)(row % b.by), z = b.zlo + (int)(row / b.by);
  const size_t lin0 = ((size_t)z * a.vsize[1] + y) * a.vsize[0] + b.xlo;
  const int skip = (int)((a.stride - lin0 % a.stride) % a.stride);
  const long long xl = (long long)b.xlo + skip + (long long)k * a.stride;
  if (xl > b.xhi) return false;
  x = (int)xl;
  e = (lin0 + (size_t)(x - b.xlo)) / a.stride;
  return true;
}

// One candidate sample, for every kernel that scans cell by cell (k_bsp_metric<0 / 1 / 2>, k_bsp_mi_hist): jitter, ownership by the
// jittered position, displacement from the cell's 192 coefficients in LDS (`s_c`), the two buffer tests, the masks, the two
// intensities and -- GRAD -- the moving gradient from the packed image, the planar image or the interpolant, carried to the
// coefficient's axes (gp[r] = (g . Md)_r).  -> status bits (0: the sample belongs to another cell); w[12] = the axis weights of
// a sample inside the transform domain (left untouched otherwise: the caller zeroes them).  Without GRAD the moving intensity
// is read from the image itself whatever gradient source is installed (the packed image holds the same numbers).
template <bool GRAD>
__device__ __forceinline__ int bsp_sample(const float* __restrict__ F, const pp_dims& df, const float* __restrict__ M, const pp_dims& dm,
                                          const uint8_t* __restrict__ fmask, const uint8_t* __restrict__ mmask, const float* s_c,
                                          const bsp_metric_args& a, const bsp_box& b, int x, int y, int z, size_t e, float& fval, float& mval,
                                          double gp[3], float w[12]) {
  double v[3] = {(double)x, (double)y, (double)z};
  if (a.jit) {
    v[0] += (double)a.jit[3 * e + 0];
    v[1] += (double)a.jit[3 * e + 1];
    v[2] += (double)a.jit[3 * e + 2];
  }
  double s[3];
  int own[3];
  bool inside = true;
  for (int q = 0; q < 3; ++q) {
    s[q] = a.Au[q] * v[q] + a.bu[q] - 1.0;
    own[q] = s[q] >= 0.0 ? (s[q] < a.mesh[q] ? (int)s[q] : a.mesh[q] - 1) : 0;
    inside = inside && s[q] >= 0.0 && s[q] < a.mesh[q];
  }
  if (!(own[0] == b.ci && own[1] == b.cj && own[2] == b.ck)) return 0;
  int code = BSP_SEEN;
  double d[3] = {0.0, 0.0, 0.0};
  if (inside) {
    double wx[4], wy[4], wz[4];
    bsp_weights(s[0] - own[0], wx);
    bsp_weights(s[1] - own[1], wy);
    bsp_weights(s[2] - own[2], wz);
    for (int q = 0; q < 4; ++q) {
      w[q] = (float)wx[q];
      w[4 + q] = (float)wy[q];
      w[8 + q] = (float)wz[q];
    }
    for (int kk = 0; kk < 4; ++kk)
      for (int jj = 0; jj < 4; ++jj) {
        const double wyz = wy[jj] * wz[kk];
        const float* c0 = s_c + kk * 16 + jj * 4;
        for (int r = 0; r < 3; ++r)
          d[r] += wyz * (wx[0] * (double)c0[r * 64 + 0] + wx[1] * (double)c0[r * 64 + 1] + wx[2] * (double)c0[r * 64 + 2] +
                         wx[3] * (double)c0[r * 64 + 3]);
      }
  }
  double cf[3], cm[3];
  for (int r = 0; r < 3; ++r) {
    cf[r] = a.Af[r * 3 + 0] * v[0] + a.Af[r * 3 + 1] * v[1] + a.Af[r * 3 + 2] * v[2] + a.bf[r];
    cm[r] = a.Am[r * 3 + 0] * v[0] + a.Am[r * 3 + 1] * v[1] + a.Am[r * 3 + 2] * v[2] + a.bm[r] +
            (a.Md[r * 3 + 0] * d[0] + a.Md[r * 3 + 1] * d[1] + a.Md[r * 3 + 2] * d[2]);
  }
  int bf_[3], bm_[3];
  float ff[3], fm[3];
  if (!bsp_locate(cf, df, bf_, ff) || !bsp_locate(cm, dm, bm_, fm)) return code | BSP_OUTSIDE;
  bool masked = false;
  if (fmask) {
    const int qx = (int)floor(cf[0] + 0.5), qy = (int)floor(cf[1] + 0.5), qz = (int)floor(cf[2] + 0.5);
    masked = !fmask[((size_t)qz * df.ny + qy) * df.nx + qx];
  }
  if (!masked && mmask) {
    const int qx = (int)floor(cm[0] + 0.5), qy = (int)floor(cm[1] + 0.5), qz = (int)floor(cm[2] + 0.5);
    masked = !mmask[((size_t)qz * dm.ny + qy) * dm.nx + qx];
  }
  if (masked) return code | BSP_MASKED;
  code |= BSP_VALID | (inside ? BSP_GRAD : 0);
  fval = pp_trilinear(F, df.nx, df.ny, df.nz, bf_[0], ff[0], bf_[1], ff[1], bf_[2], ff[2]);
  int x0, x1, y0, y1, z0, z1;
  float ux, uy, uz;
  pp_axis_setup(bm_[0], fm[0], dm.nx, x0, x1, ux);
  pp_axis_setup(bm_[1], fm[1], dm.ny, y0, y1, uy);
  pp_axis_setup(bm_[2], fm[2], dm.nz, z0, z1, uz);
  const size_t sy = dm.nx, sz = (size_t)dm.nx * dm.ny;
  const size_t o[8] = {z0 * sz + y0 * sy + x0, z0 * sz + y0 * sy + x1, z0 * sz + y1 * sy + x0, z0 * sz + y1 * sy + x1,
                       z1 * sz + y0 * sy + x0, z1 * sz + y0 * sy + x1, z1 * sz + y1 * sy + x0, z1 * sz + y1 * sy + x1};
  float am[8], gi[3] = {0.0f, 0.0f, 0.0f};
  if (GRAD && a.grad4) {   // (uniform) gradient and intensity of a corner in one 16-byte element
    float c4[4][8];
    for (int q = 0; q < 8; ++q) {
      const float4 p = a.grad4[o[q]];
      c4[0][q] = p.x, c4[1][q] = p.y, c4[2][q] = p.z, c4[3][q] = p.w;
    }
    for (int r = 0; r < 3; ++r) gi[r] = bsp_lerp8(c4[r], ux, uy, uz);
    for (int q = 0; q < 8; ++q) am[q] = c4[3][q];
  } else {
    for (int q = 0; q < 8; ++q) am[q] = M[o[q]];
    if (GRAD && a.grad) {
      const size_t N = sz * dm.nz;
      for (int r = 0; r < 3; ++r) {
        float ag[8];
        for (int q = 0; q < 8; ++q) ag[q] = a.grad[r * N + o[q]];
        gi[r] = bsp_lerp8(ag, ux, uy, uz);
      }
    } else if (GRAD) {   // gradient of the trilinear interpolant, per moving voxel (as k_metric_grad)
      const float v00 = am[0] + (am[1] - am[0]) * ux, v10 = am[2] + (am[3] - am[2]) * ux;
      const float v01 = am[4] + (am[5] - am[4]) * ux, v11 = am[6] + (am[7] - am[6]) * ux;
      const float v0 = v00 + (v10 - v00) * uy, v1 = v01 + (v11 - v01) * uy;
      const float gx0 = (am[1] - am[0]) + ((am[3] - am[2]) - (am[1] - am[0])) * uy;
      const float gx1 = (am[5] - am[4]) + ((am[7] - am[6]) - (am[5] - am[4])) * uy;
      gi[0] = gx0 + (gx1 - gx0) * uz;
      gi[1] = (v10 - v00) + ((v11 - v01) - (v10 - v00)) * uz;
      gi[2] = v1 - v0;
    }
  }
  mval = bsp_lerp8(am, ux, uy, uz);
  if (GRAD)
    for (int r = 0; r < 3; ++r)
      gp[r] = (double)gi[0] * a.Md[0 * 3 + r] + (double)gi[1] * a.Md[1 * 3 + r] + (double)gi[2] * a.Md[2 * 3 + r];
  return code;
}

// the score derivative of a sample for pass 2 of the Mattes metric: sum_{q = mb - 1 .. mb + 2} B3'(q - tm) table[fb][q]
__device__ __forceinline__ double bsp_mi_bracket(const bsp_mi_args& mi, const float* tab, float fval, float mval) {
  double tf, tm;
  const int fb = mi_bin((double)fval, mi.f_bin, mi.f_norm_min, 2, mi.nbins - 3, tf);
  const int mb = mi_bin((double)mval, mi.m_bin, mi.m_norm_min, 2, mi.nbins - 3, tm);
  double w = 0.0;
  for (int k = mb - 1; k <= mb + 2; ++k) w += mi_bspline3_deriv((double)k - tm) * (double)tab[fb * mi.nbins + k];
  return w;
}

// MODE 0: mean squares (row = 192 sums of -2 (f - m) g_r w + scalars).  MODE 1: correlation (192 sums each of g_r w, f g_r w, m g_r w).
// MODE 2: pass 2 of Mattes mutual information (192 sums of bracket_s g_r w, bsp_mi_bracket).  Its score table is staged in LDS
// as fp32, as k_mi_gradient holds it: 16 KB next to the 24 KB of sample staging, 40 KB per workgroup and so still four
// workgroups per CU (160 KB); modes 0 and 1 declare one element.
template <int MODE>
__global__ void __launch_bounds__(BSP_NT) k_bsp_metric(const float* __restrict__ F, pp_dims df, const float* __restrict__ M, pp_dims dm,
                                                       const uint8_t* __restrict__ fmask, const uint8_t* __restrict__ mmask,
                                                       const float* __restrict__ C, bsp_metric_args a, bsp_mi_args mi,
                                                       double* __restrict__ partial) {
  constexpr int NG = MODE == 1 ? 576 : 192;
  constexpr int ROW = NG + BSP_NSCAL;
  __shared__ float s_c[192];
  __shared__ double s_g[3 * BSP_NT];
  __shared__ float s_w[12 * BSP_NT];
  __shared__ double s_f[BSP_NT];
  __shared__ double s_m[BSP_NT];
  __shared__ int s_code[BSP_NT];
  __shared__ float s_tab[MODE == 2 ? MI_MAX_BINS * MI_MAX_BINS : 1];

  const int t = threadIdx.x;
  const bsp_box b = bsp_row_box(a, (int)blockIdx.x);
  const size_t ncp = (size_t)a.lat[0] * a.lat[1] * a.lat[2];
  if (t < 192) {
    const int r = t >> 6, cp = t & 63;
    s_c[t] = C[r * ncp + ((size_t)(b.ck + (cp >> 4)) * a.lat[1] + (b.cj + ((cp >> 2) & 3))) * a.lat[0] + b.ci + (cp & 3)];
  }
  if (MODE == 2)
    for (int i = t; i < mi.nbins * mi.nbins; i += BSP_NT) s_tab[i] = mi.table[i];

  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  __syncthreads();
  for (long long first = 0; first < b.items; first += BSP_NT) {
    // ---- phase 1: one candidate sample per thread, staged in slot t
    int code = 0;
    double fd = 0.0, md = 0.0, g[3] = {0.0, 0.0, 0.0};
    float w[12];
    for (int k = 0; k < 12; ++k) w[k] = 0.0f;
    const long long item = first + t;
    int x, y, z;
    size_t e;
    if (item < b.items && bsp_box_item(a, b, item, x, y, z, e)) {
      float fval = 0.0f, mval = 0.0f;
      double gp[3] = {0.0, 0.0, 0.0};
      code = bsp_sample<true>(F, df, M, dm, fmask, mmask, s_c, a, b, x, y, z, e, fval, mval, gp, w);
      if (code & BSP_VALID) {
        fd = fval;
        md = mval;
        const double scale = MODE == 0 ? -2.0 * (fd - md) : (MODE == 1 ? 1.0 : bsp_mi_bracket(mi, s_tab, fval, mval));
        for (int r = 0; r < 3; ++r) g[r] = scale * gp[r];
      }
    }
    s_code[t] = code;
    s_f[t] = fd;
    s_m[t] = md;
    for (int r = 0; r < 3; ++r) s_g[r * BSP_NT + t] = g[r];
    for (int k = 0; k < 12; ++k) s_w[k * BSP_NT + t] = w[k];
    __syncthreads();
    // ---- phase 2: thread (r, i j k) adds its term of every staged sample, in slot order
    if (t < 192) {
      const int r = t >> 6, cp = t & 63;
      const float* pwx = s_w + (cp & 3) * BSP_NT;
      const float* pwy = s_w + (4 + ((cp >> 2) & 3)) * BSP_NT;
      const float* pwz = s_w + (8 + (cp >> 4)) * BSP_NT;
      const double* pg = s_g + r * BSP_NT;
      for (int s = 0; s < BSP_NT; ++s) {
        if (!(s_code[s] & BSP_GRAD)) continue;
        const double term = pg[s] * (double)(pwx[s] * pwy[s] * pwz[s]);
        acc0 += term;
        if (MODE == 1) {
          acc1 += s_f[s] * term;
          acc2 += s_m[s] * term;
        }
      }
    } else if (t < 192 + BSP_NSCAL) {
      const int q = t - 192;
      for (int s = 0; s < BSP_NT; ++s) {
        const int c = s_code[s];
        if (!c) continue;
        const double f = s_f[s], m = s_m[s];
        double add = 0.0;
        if (c & BSP_VALID) {
          switch (q) {
            case 0: add = 1.0; break;
            case 1: add = f; break;
            case 2: add = m; break;
            case 3: add = f * f; break;
            case 4: add = m * m; break;
            case 5: add = f * m; break;
            case 6: add = (f - m) * (f - m); break;
            default: break;
          }
        }
        if (q == 7 && (c & BSP_OUTSIDE)) add = 1.0;
        if (q == 8 && (c & BSP_MASKED)) add = 1.0;
        if (q == 9) add = 1.0;
        acc0 += add;
      }
    }
    __syncthreads();
  }
  double* row = partial + (size_t)blockIdx.x * ROW;
  if (t < 192) {
    row[t] = acc0;
    if (MODE == 1) {
      row[192 + t] = acc1;
      row[384 + t] = acc2;
    }
  } else if (t < 192 + BSP_NSCAL) {
    row[NG + (t - 192)] = acc0;
  }
}

// Pass 1 of Mattes mutual information over the B-spline: the joint histogram of the valid samples.  The same rows (cell, z
// slab) as k_bsp_metric, scanned the same way, but by a BOUNDED grid: workgroup g takes rows g, g + grid, ... and keeps ONE LDS
// table in 64-bit fixed point (2^-32 units, integer atomics: the sum is associative, so two calls return the same bits whatever
// the scheduling) which it flushes once, non-empty bins only -- a table per row would send up to 16 384 x nbins^2 atomics of a
// 32 x 32 x 16 mesh to the same few thousand addresses.  No staging and no second phase: a thread bins its own sample.  The four
// counts (valid, outside, masked, seen) are kept in registers and follow the table.  LDS: 32 KB + the 192 coefficients.
constexpr int BSP_MI_GRID = 1024;   // four workgroups per CU on 256 CUs, twice k_mi_histogram's 512: A MODEL, NOT A MEASUREMENT
__global__ void __launch_bounds__(BSP_NT) k_bsp_mi_hist(const float* __restrict__ F, pp_dims df, const float* __restrict__ M, pp_dims dm,
                                                        const uint8_t* __restrict__ fmask, const uint8_t* __restrict__ mmask,
                                                        const float* __restrict__ C, bsp_metric_args a, bsp_mi_args mi, int nrows,
                                                        unsigned long long* __restrict__ hist /* [nbins^2 + 4], last 4 = the counts */) {
  __shared__ float s_c[192];
  __shared__ unsigned long long s_h[MI_MAX_BINS * MI_MAX_BINS + 4];
  const int t = threadIdx.x;
  const int nb2 = mi.nbins * mi.nbins;
  for (int i = t; i < nb2 + 4; i += BSP_NT) s_h[i] = 0ull;
  const size_t ncp = (size_t)a.lat[0] * a.lat[1] * a.lat[2];
  unsigned long long cnt[4] = {0ull, 0ull, 0ull, 0ull};
  for (int row = (int)blockIdx.x; row < nrows; row += (int)gridDim.x) {
    const bsp_box b = bsp_row_box(a, row);
    __syncthreads();   // the table is zero; nobody reads the previous cell's coefficients any more
    if (t < 192) {
      const int r = t >> 6, cp = t & 63;
      s_c[t] = C[r * ncp + ((size_t)(b.ck + (cp >> 4)) * a.lat[1] + (b.cj + ((cp >> 2) & 3))) * a.lat[0] + b.ci + (cp & 3)];
    }
    __syncthreads();
    for (long long item = t; item < b.items; item += BSP_NT) {
      int x, y, z;
      size_t e;
      if (!bsp_box_item(a, b, item, x, y, z, e)) continue;
      float fval = 0.0f, mval = 0.0f, w[12];
      double gp[3];
      const int code = bsp_sample<false>(F, df, M, dm, fmask, mmask, s_c, a, b, x, y, z, e, fval, mval, gp, w);
      if (!code) continue;
      cnt[3] += 1ull;
      if (code & BSP_OUTSIDE) cnt[1] += 1ull;
      if (code & BSP_MASKED) cnt[2] += 1ull;
      if (!(code & BSP_VALID)) continue;
      cnt[0] += 1ull;
      double tf, tm;
      const int fb = mi_bin((double)fval, mi.f_bin, mi.f_norm_min, 2, mi.nbins - 3, tf);
      const int mb = mi_bin((double)mval, mi.m_bin, mi.m_norm_min, 2, mi.nbins - 3, tm);
      for (int k = mb - 1; k <= mb + 2; ++k)
        atomicAdd(&s_h[fb * mi.nbins + k], (unsigned long long)(mi_bspline3((double)k - tm) * 4294967296.0 + 0.5));
    }
  }
  for (int q = 0; q < 4; ++q)
    if (cnt[q]) atomicAdd(&s_h[nb2 + q], cnt[q]);
  __syncthreads();
  for (int i = t; i < nb2 + 4; i += BSP_NT)
    if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

// the ten scalar moments of all rows, one fixed tree
__global__ void __launch_bounds__(BSP_NT) k_bsp_scalars(const double* __restrict__ partial, int nrows, int row, int off,
                                                        double* __restrict__ out) {
  __shared__ double red[BSP_NSCAL * BSP_NT];
  double acc[BSP_NSCAL];
  for (int q = 0; q < BSP_NSCAL; ++q) acc[q] = 0.0;
  for (int i = threadIdx.x; i < nrows; i += BSP_NT)
    for (int q = 0; q < BSP_NSCAL; ++q) acc[q] += partial[(size_t)i * row + off + q];
  for (int q = 0; q < BSP_NSCAL; ++q) red[q * BSP_NT + threadIdx.x] = acc[q];
  pp_block_tree<BSP_NT>((int)threadIdx.x, [&](int a, int b) {
    for (int q = 0; q < BSP_NSCAL; ++q) red[q * BSP_NT + a] += red[q * BSP_NT + b];
  });
  if ((int)threadIdx.x < BSP_NSCAL) out[threadIdx.x] = red[threadIdx.x * BSP_NT];
}

// gradient[p] for coefficient p = (r, k, j, i): the rows of the cells (and slabs) that cover control point (i, j, k), added in a
// fixed order, then the metric's normalisation from the scalar moments (MODE 2, mutual information: none)
template <int MODE>
__global__ void __launch_bounds__(BSP_NT) k_bsp_gather(const double* __restrict__ partial, const double* __restrict__ scal,
                                                       bsp_metric_args a, double* __restrict__ gradient) {
  constexpr int NG = MODE == 1 ? 576 : 192;
  constexpr int ROW = NG + BSP_NSCAL;
  const size_t ncp = (size_t)a.lat[0] * a.lat[1] * a.lat[2];
  const size_t p = (size_t)blockIdx.x * BSP_NT + threadIdx.x;
  if (p >= 3 * ncp) return;
  const int r = (int)(p / ncp);
  const size_t q = p % ncp;
  const int i = (int)(q % a.lat[0]), j = (int)((q / a.lat[0]) % a.lat[1]), k = (int)(q / ((size_t)a.lat[0] * a.lat[1]));
  double G = 0.0, FG = 0.0, MG = 0.0;
  for (int lk = 0; lk < 4; ++lk) {
    const int ck = k - lk;
    if (ck < 0 || ck >= a.mesh[2]) continue;
    for (int lj = 0; lj < 4; ++lj) {
      const int cj = j - lj;
      if (cj < 0 || cj >= a.mesh[1]) continue;
      for (int li = 0; li < 4; ++li) {
        const int ci = i - li;
        if (ci < 0 || ci >= a.mesh[0]) continue;
        const size_t cell = ((size_t)ck * a.mesh[1] + cj) * a.mesh[0] + ci;
        const int slot = r * 64 + lk * 16 + lj * 4 + li;
        for (int sp = 0; sp < a.nsplit; ++sp) {
          const double* row = partial + (cell * a.nsplit + sp) * ROW;
          G += row[slot];
          if (MODE == 1) {
            FG += row[192 + slot];
            MG += row[384 + slot];
          }
        }
      }
    }
  }
  const double cnt = scal[0];
  double out = 0.0;
  if (cnt > 0.0) {
    if (MODE == 0) {
      out = G / cnt;
    } else if (MODE == 2) {
      out = G;   // 1 / (N m_bin) is in the score table
    } else {
      const double fbar = scal[1] / cnt, mbar = scal[2] / cnt;
      const double sff = scal[3] - cnt * fbar * fbar, smm = scal[4] - cnt * mbar * mbar, sfm = scal[5] - cnt * fbar * mbar;
      if (sff > 1e-300 && smm > 1e-300) {
        const double dsfm = FG - fbar * G, dsmm = 2.0 * (MG - mbar * G);
        out = -(2.0 * sfm / (sff * smm) * dsfm - (sfm * sfm) / (sff * smm * smm) * dsmm);
      }
    }
  }
  gradient[p] = out;
}

int bsp_lattice_check(pp_ctx* ctx, const pp_geom* lattice, const char* what) {
  const int rc = pp_geom_check(ctx, lattice, what);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k)
    if (lattice->size[k] < 4) return pp_fail(ctx, PP_ERR_ARG, "%s: a cubic B-spline lattice has at least 4 control points per axis", what);
  return PP_OK;
}

bool bsp_same_direction(const pp_geom* a, const pp_geom* b) {
  for (int k = 0; k < 9; ++k)
    if (!(std::fabs(a->direction[k] - b->direction[k]) <= 1e-9)) return false;
  return true;
}

}  // namespace

extern "C" int pp_bspline_field_f32(pp_ctx* ctx, const float* coefficients, const pp_geom* lattice, const pp_geom* grid, float* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, coefficients && out, "pp_bspline_field_f32: NULL argument");
  int rc = bsp_lattice_check(ctx, lattice, "pp_bspline_field_f32 lattice");
  if (rc) return rc;
  rc = pp_geom_check(ctx, grid, "pp_bspline_field_f32 grid");
  if (rc) return rc;
  pp_index_map m;
  pp_make_index_map(lattice, grid, nullptr, nullptr, &m);
  bsp_field_args a;
  double diag = 0.0, off = 0.0;
  for (int k = 0; k < 9; ++k) {
    a.A[k] = m.A[k];
    if (k % 4 == 0) diag = std::fmax(diag, std::fabs(m.A[k]));
    else off = std::fmax(off, std::fabs(m.A[k]));
  }
  for (int k = 0; k < 3; ++k) {
    a.b[k] = m.b[k];
    a.n[k] = grid->size[k];
    a.lat[k] = lattice->size[k];
  }
  // lattice axes = grid axes (any spacing, origin, flip): an off-diagonal term below 1e-12 of the diagonal moves the far
  // corner of a 2^11-voxel axis by 2e-9 of a cell
  const bool aligned = off <= 1e-12 * diag;
  const size_t n = pp_nvox(grid->size);
  const int ntab = grid->size[0] + grid->size[1] + grid->size[2];
  int* tb = nullptr;
  double* tw = nullptr;
  if (aligned) {
    rc = pp_reserve(ctx, pp_align_up((size_t)ntab * sizeof(int), 256) + pp_align_up((size_t)ntab * 4 * sizeof(double), 256));
    if (rc) return rc;
    pp_carver cv{ctx->ws, 0};
    tb = cv.take<int>(ntab);
    tw = cv.take<double>((size_t)ntab * 4);
    hipLaunchKernelGGL(k_bsp_tables, dim3((ntab + BSP_NT - 1) / BSP_NT), dim3(BSP_NT), 0, ctx->stream, a, tb, tw);
    PP_LAUNCH_CHECK(ctx, "k_bsp_tables");
  }
  const unsigned nb = (unsigned)std::min<size_t>((n + BSP_NT - 1) / BSP_NT, 1u << 20);
  pp_prof_scope prof(ctx, "bspline_field");
  if (aligned)
    hipLaunchKernelGGL((k_bsp_field<true>), dim3(nb), dim3(BSP_NT), 0, ctx->stream, coefficients, a, (const int*)tb, (const double*)tw, out);
  else
    hipLaunchKernelGGL((k_bsp_field<false>), dim3(nb), dim3(BSP_NT), 0, ctx->stream, coefficients, a, (const int*)tb, (const double*)tw, out);
  PP_LAUNCH_CHECK(ctx, "k_bsp_field");
  return PP_OK;
}

namespace {

// What the three metric entry points check and set up alike, before anything is launched: the geometries, the directions, the
// index maps, the jitter and gradient sources of the context, the z-slab split.  `what`: the entry point's name for messages.
int bsp_metric_prepare(pp_ctx* ctx, const char* what, const pp_geom* fixed_geom, const pp_geom* moving_geom, const pp_geom* virt, int stride,
                       const pp_geom* lattice, double jitter_bound, bsp_metric_args& a, size_t& nsamp, size_t& nrows) {
  if (!(stride >= 1)) return pp_fail(ctx, PP_ERR_ARG, "%s: stride must be at least 1", what);
  if (!(jitter_bound >= 0.0 && jitter_bound < 1.0e6))
    return pp_fail(ctx, PP_ERR_ARG, "%s: jitter_bound must be a finite, non-negative number of voxels", what);
  char name[96];
  snprintf(name, sizeof(name), "%s lattice", what);
  int rc = bsp_lattice_check(ctx, lattice, name);
  if (rc) return rc;
  snprintf(name, sizeof(name), "%s fixed", what);
  if ((rc = pp_geom_check(ctx, fixed_geom, name)) != PP_OK) return rc;
  snprintf(name, sizeof(name), "%s moving", what);
  if ((rc = pp_geom_check(ctx, moving_geom, name)) != PP_OK) return rc;
  snprintf(name, sizeof(name), "%s virtual", what);
  if ((rc = pp_geom_check(ctx, virt, name)) != PP_OK) return rc;
  if (!bsp_same_direction(lattice, fixed_geom) || !bsp_same_direction(lattice, virt))
    return pp_fail(ctx, PP_ERR_DIRECTION, "%s: the lattice, the virtual grid and the fixed image must share their direction cosines", what);

  pp_index_map mf, mm, mu;
  pp_make_index_map(fixed_geom, virt, nullptr, nullptr, &mf);
  pp_make_index_map(moving_geom, virt, nullptr, nullptr, &mm);
  pp_make_index_map(lattice, virt, nullptr, nullptr, &mu);
  for (int k = 0; k < 9; ++k) a.Af[k] = mf.A[k], a.Am[k] = mm.A[k], a.Md[k] = mm.Md[k];
  for (int k = 0; k < 3; ++k) {
    a.bf[k] = mf.b[k];
    a.bm[k] = mm.b[k];
    a.Au[k] = mu.A[k * 3 + k];
    a.bu[k] = mu.b[k];
    a.vsize[k] = virt->size[k];
    a.lat[k] = lattice->size[k];
    a.mesh[k] = lattice->size[k] - 3;
    if (!(a.Au[k] > 0.0)) return pp_fail(ctx, PP_ERR_DIRECTION, "%s: lattice axis %d does not run along the virtual grid's", what, k);
  }
  for (int k = 0; k < 9; ++k)
    if (k % 4 != 0 && std::fabs(mu.A[k]) > 1e-9 * a.Au[k / 3])
      return pp_fail(ctx, PP_ERR_DIRECTION, "%s: the lattice is oblique to the virtual grid", what);
  a.stride = stride;
  a.margin = (int)std::ceil(jitter_bound) + 1;   // + 1: the box edges are divisions, the ownership test a multiplication
  const size_t nvirt = pp_nvox(virt->size);
  nsamp = (nvirt + stride - 1) / stride;
  a.jit = nullptr;
  if (ctx->jitter) {
    PP_REQUIRE(ctx, ctx->jitter_samples >= nsamp, "metric: the sample-jitter array set by pp_linear_set_sample_jitter is shorter than the sampling lattice");
    a.jit = ctx->jitter;
  }
  a.grad = nullptr;
  a.grad4 = nullptr;
  if (ctx->mgrad) {
    PP_REQUIRE(ctx, ctx->mgrad_size[0] == moving_geom->size[0] && ctx->mgrad_size[1] == moving_geom->size[1] && ctx->mgrad_size[2] == moving_geom->size[2],
               "metric: the gradient image set by pp_linear_set_moving_gradient does not have the moving image's size");
    a.grad = ctx->mgrad;
    if (ctx->mgrad4) a.grad4 = reinterpret_cast<const float4*>(ctx->mgrad4);
  }
  const size_t ncells = (size_t)a.mesh[0] * a.mesh[1] * a.mesh[2];
  // enough workgroups for the card: a mesh of few cells is cut into z slabs (at most 16; the count is a function of the mesh
  // alone, so the summation order -- and with it every bit of the result -- is too)
  int nsplit = 1;
  if (ncells < 1024) nsplit = (int)std::min<size_t>(16, (1024 + ncells - 1) / ncells);
  a.nsplit = nsplit;
  nrows = ncells * nsplit;
  if (!(nrows < (size_t)1 << 30)) return pp_fail(ctx, PP_ERR_ARG, "%s: mesh too fine", what);
  return PP_OK;
}

// The bins of the two mutual-information passes: Mattes only, 5..64 bins, positive widths.
int bsp_mi_bins_check(pp_ctx* ctx, const char* what, const pp_mi_bins* bins, bsp_mi_args& mi) {
  if (bins->kernel != PP_MI_MATTES) return pp_fail(ctx, PP_ERR_ARG, "%s: the Parzen kernel must be PP_MI_MATTES", what);
  if (!(bins->nbins >= 5 && bins->nbins <= MI_MAX_BINS)) return pp_fail(ctx, PP_ERR_ARG, "%s: 5..64 bins, got %d", what, bins->nbins);
  if (!(bins->f_bin > 0.0 && bins->m_bin > 0.0)) return pp_fail(ctx, PP_ERR_ARG, "%s: bin widths must be positive", what);
  mi.nbins = bins->nbins;
  mi.f_bin = bins->f_bin, mi.f_norm_min = bins->f_norm_min;
  mi.m_bin = bins->m_bin, mi.m_norm_min = bins->m_norm_min;
  mi.table = nullptr;
  return PP_OK;
}

// rows -> scalar moments (read back into s) and the device gradient.  mode as k_bsp_metric's MODE.
int bsp_gather(pp_ctx* ctx, int mode, const bsp_metric_args& a, const double* partial, size_t nrows, double* scal, double* dgrad, size_t ncp,
               double s[BSP_NSCAL]) {
  const int ROW = (mode == 1 ? 576 : 192) + BSP_NSCAL;
  {
    pp_prof_scope prof(ctx, "bspline_gather");
    hipLaunchKernelGGL(k_bsp_scalars, dim3(1), dim3(BSP_NT), 0, ctx->stream, partial, (int)nrows, ROW, ROW - BSP_NSCAL, scal);
    PP_LAUNCH_CHECK(ctx, "k_bsp_scalars");
    const unsigned gb = (unsigned)((3 * ncp + BSP_NT - 1) / BSP_NT);
    if (mode == 0)
      hipLaunchKernelGGL((k_bsp_gather<0>), dim3(gb), dim3(BSP_NT), 0, ctx->stream, partial, (const double*)scal, a, dgrad);
    else if (mode == 1)
      hipLaunchKernelGGL((k_bsp_gather<1>), dim3(gb), dim3(BSP_NT), 0, ctx->stream, partial, (const double*)scal, a, dgrad);
    else
      hipLaunchKernelGGL((k_bsp_gather<2>), dim3(gb), dim3(BSP_NT), 0, ctx->stream, partial, (const double*)scal, a, dgrad);
    PP_LAUNCH_CHECK(ctx, "k_bsp_gather");
  }
  return pp_read_back(ctx, scal, s, BSP_NSCAL * sizeof(double));
}

}  // namespace

extern "C" int pp_bspline_metric_f32(pp_ctx* ctx, int metric, const float* fixed, const pp_geom* fixed_geom, const float* moving,
                                     const pp_geom* moving_geom, const pp_geom* virt, int stride, const uint8_t* fixed_mask,
                                     const uint8_t* moving_mask, const float* coefficients, const pp_geom* lattice, double jitter_bound,
                                     double* value, double* stats, double* gradient) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, fixed && moving && coefficients && value && gradient, "pp_bspline_metric_f32: NULL argument");
  PP_REQUIRE(ctx, metric == PP_BSPLINE_MEAN_SQUARES || metric == PP_BSPLINE_CORRELATION,
             "pp_bspline_metric_f32: metric must be 0 (mean squares) or 1 (correlation)");
  bsp_metric_args a;
  size_t nsamp = 0, nrows = 0;
  int rc = bsp_metric_prepare(ctx, "pp_bspline_metric_f32", fixed_geom, moving_geom, virt, stride, lattice, jitter_bound, a, nsamp, nrows);
  if (rc) return rc;
  const size_t ncp = pp_nvox(lattice->size);
  const int ROW = (metric == 0 ? 192 : 576) + BSP_NSCAL;
  rc = pp_reserve(ctx, pp_align_up(nrows * ROW * sizeof(double), 256) + 256 + pp_align_up(3 * ncp * sizeof(double), 256));
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  double* partial = cv.take<double>(nrows * ROW);
  double* scal = cv.take<double>(BSP_NSCAL);
  double* dgrad = cv.take<double>(3 * ncp);
  const pp_dims df{fixed_geom->size[0], fixed_geom->size[1], fixed_geom->size[2]};
  const pp_dims dm{moving_geom->size[0], moving_geom->size[1], moving_geom->size[2]};
  const bsp_mi_args no_mi{0, 0.0, 0.0, 0.0, 0.0, nullptr};
  {
    pp_prof_scope prof(ctx, "bspline_metric");
    if (metric == 0)
      hipLaunchKernelGGL((k_bsp_metric<0>), dim3((unsigned)nrows), dim3(BSP_NT), 0, ctx->stream, fixed, df, moving, dm, fixed_mask, moving_mask,
                         coefficients, a, no_mi, partial);
    else
      hipLaunchKernelGGL((k_bsp_metric<1>), dim3((unsigned)nrows), dim3(BSP_NT), 0, ctx->stream, fixed, df, moving, dm, fixed_mask, moving_mask,
                         coefficients, a, no_mi, partial);
    PP_LAUNCH_CHECK(ctx, "k_bsp_metric");
  }
  double s[BSP_NSCAL];
  rc = bsp_gather(ctx, metric, a, partial, nrows, scal, dgrad, ncp, s);
  if (rc) return rc;
  if (s[9] != (double)nsamp)   // (a refusal leaves value, stats and gradient as they were)
    return pp_fail(ctx, PP_ERR_ARG, "pp_bspline_metric_f32: %.0f of %zu samples visited -- a sample's jitter exceeds jitter_bound = %g voxels",
                   s[9], nsamp, jitter_bound);
  const double cnt = s[0];
  if (cnt <= 0.0) return pp_fail(ctx, PP_ERR_NO_OVERLAP, "pp_bspline_metric_f32: no valid sample points");
  PP_HIP(ctx, hipMemcpyAsync(gradient, dgrad, 3 * ncp * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) stats[0] = s[0], stats[1] = s[7], stats[2] = s[8], stats[3] = s[9];
  if (metric == 0) {
    *value = s[6] / cnt;
  } else {
    const double fbar = s[1] / cnt, mbar = s[2] / cnt;
    const double sff = s[3] - cnt * fbar * fbar, smm = s[4] - cnt * mbar * mbar, sfm = s[5] - cnt * fbar * mbar;
    *value = (sff <= 1e-300 || smm <= 1e-300) ? 0.0 : -(sfm * sfm) / (sff * smm);
  }
  return PP_OK;
}

extern "C" int pp_bspline_mi_histogram_f32(pp_ctx* ctx, const float* fixed, const pp_geom* fixed_geom, const float* moving,
                                           const pp_geom* moving_geom, const pp_geom* virt, int stride, const uint8_t* fixed_mask,
                                           const uint8_t* moving_mask, const float* coefficients, const pp_geom* lattice, double jitter_bound,
                                           const pp_mi_bins* bins, double* hist, double* stats) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, fixed && moving && coefficients && bins && hist, "pp_bspline_mi_histogram_f32: NULL argument");
  bsp_mi_args mi;
  int rc = bsp_mi_bins_check(ctx, "pp_bspline_mi_histogram_f32", bins, mi);
  if (rc) return rc;
  bsp_metric_args a;
  size_t nsamp = 0, nrows = 0;
  rc = bsp_metric_prepare(ctx, "pp_bspline_mi_histogram_f32", fixed_geom, moving_geom, virt, stride, lattice, jitter_bound, a, nsamp, nrows);
  if (rc) return rc;
  const int nb2 = mi.nbins * mi.nbins;
  rc = pp_reserve(ctx, pp_align_up((size_t)(nb2 + 4) * sizeof(unsigned long long), 256));
  if (rc) return rc;
  unsigned long long* dh = reinterpret_cast<unsigned long long*>(ctx->ws);
  PP_HIP(ctx, hipMemsetAsync(dh, 0, (size_t)(nb2 + 4) * sizeof(unsigned long long), ctx->stream));
  const pp_dims df{fixed_geom->size[0], fixed_geom->size[1], fixed_geom->size[2]};
  const pp_dims dm{moving_geom->size[0], moving_geom->size[1], moving_geom->size[2]};
  {
    pp_prof_scope prof(ctx, "bspline_mi_histogram");
    const unsigned nb = (unsigned)std::min<size_t>(nrows, (size_t)BSP_MI_GRID);
    hipLaunchKernelGGL(k_bsp_mi_hist, dim3(nb), dim3(BSP_NT), 0, ctx->stream, fixed, df, moving, dm, fixed_mask, moving_mask, coefficients, a, mi,
                       (int)nrows, dh);
    PP_LAUNCH_CHECK(ctx, "k_bsp_mi_hist");
  }
  std::vector<unsigned long long> h((size_t)nb2 + 4);
  PP_HIP(ctx, hipMemcpyAsync(h.data(), dh, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (h[nb2 + 3] != (unsigned long long)nsamp)   // (a refusal leaves hist and stats as they were)
    return pp_fail(ctx, PP_ERR_ARG, "pp_bspline_mi_histogram_f32: %llu of %zu samples visited -- a sample's jitter exceeds jitter_bound = %g voxels",
                   h[nb2 + 3], nsamp, jitter_bound);
  if (h[nb2] == 0ull) return pp_fail(ctx, PP_ERR_NO_OVERLAP, "pp_bspline_mi_histogram_f32: no valid sample points");
  for (int i = 0; i < nb2; ++i) hist[i] = (double)h[i] / 4294967296.0;
  if (stats)
    for (int q = 0; q < 4; ++q) stats[q] = (double)h[nb2 + q];
  return PP_OK;
}

extern "C" int pp_bspline_mi_gradient_f32(pp_ctx* ctx, const float* fixed, const pp_geom* fixed_geom, const float* moving,
                                          const pp_geom* moving_geom, const pp_geom* virt, int stride, const uint8_t* fixed_mask,
                                          const uint8_t* moving_mask, const float* coefficients, const pp_geom* lattice, double jitter_bound,
                                          const pp_mi_bins* bins, const double* table, double* stats, double* gradient) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, fixed && moving && coefficients && bins && table && gradient, "pp_bspline_mi_gradient_f32: NULL argument");
  bsp_mi_args mi;
  int rc = bsp_mi_bins_check(ctx, "pp_bspline_mi_gradient_f32", bins, mi);
  if (rc) return rc;
  bsp_metric_args a;
  size_t nsamp = 0, nrows = 0;
  rc = bsp_metric_prepare(ctx, "pp_bspline_mi_gradient_f32", fixed_geom, moving_geom, virt, stride, lattice, jitter_bound, a, nsamp, nrows);
  if (rc) return rc;
  const size_t ncp = pp_nvox(lattice->size);
  const int ROW = 192 + BSP_NSCAL;
  const int nb2 = mi.nbins * mi.nbins;
  rc = pp_reserve(ctx, pp_align_up(nrows * ROW * sizeof(double), 256) + 256 + pp_align_up(3 * ncp * sizeof(double), 256) +
                           pp_align_up((size_t)nb2 * sizeof(float), 256));
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  double* partial = cv.take<double>(nrows * ROW);
  double* scal = cv.take<double>(BSP_NSCAL);
  double* dgrad = cv.take<double>(3 * ncp);
  float* dtab = cv.take<float>((size_t)nb2);
  std::vector<float> ht((size_t)nb2);
  for (int i = 0; i < nb2; ++i) ht[i] = (float)table[i];
  PP_HIP(ctx, hipMemcpyAsync(dtab, ht.data(), (size_t)nb2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // ht is a local: the copy must have left it
  mi.table = dtab;
  const pp_dims df{fixed_geom->size[0], fixed_geom->size[1], fixed_geom->size[2]};
  const pp_dims dm{moving_geom->size[0], moving_geom->size[1], moving_geom->size[2]};
  {
    pp_prof_scope prof(ctx, "bspline_mi_gradient");
    hipLaunchKernelGGL((k_bsp_metric<2>), dim3((unsigned)nrows), dim3(BSP_NT), 0, ctx->stream, fixed, df, moving, dm, fixed_mask, moving_mask,
                       coefficients, a, mi, partial);
    PP_LAUNCH_CHECK(ctx, "k_bsp_metric");
  }
  double s[BSP_NSCAL];
  rc = bsp_gather(ctx, 2, a, partial, nrows, scal, dgrad, ncp, s);
  if (rc) return rc;
  if (s[9] != (double)nsamp)   // (a refusal leaves stats and gradient as they were)
    return pp_fail(ctx, PP_ERR_ARG, "pp_bspline_mi_gradient_f32: %.0f of %zu samples visited -- a sample's jitter exceeds jitter_bound = %g voxels",
                   s[9], nsamp, jitter_bound);
  if (s[0] <= 0.0) return pp_fail(ctx, PP_ERR_NO_OVERLAP, "pp_bspline_mi_gradient_f32: no valid sample points");
  if (stats) stats[0] = s[0], stats[1] = s[7], stats[2] = s[8], stats[3] = s[9];
  PP_HIP(ctx, hipMemcpyAsync(gradient, dgrad, 3 * ncp * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PP_OK;
}
