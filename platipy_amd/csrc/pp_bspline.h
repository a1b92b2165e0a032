// platipy_amd/csrc/pp_bspline.h -- cubic B-spline transform on the GPU: dense evaluation and the similarity metric with its
// gradient over all control-point coefficients (pp_bspline_field_f32, pp_bspline_metric_f32).  Included at the end of pp_linear.hip.
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
#pragma once

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

// MODE 0: mean squares (row = 192 sums of -2 (f - m) g_r w + scalars).  MODE 1: correlation (192 sums each of g_r w, f g_r w, m g_r w).
template <int MODE>
__global__ void __launch_bounds__(BSP_NT) k_bsp_metric(const float* __restrict__ F, pp_dims df, const float* __restrict__ M, pp_dims dm,
                                                       const uint8_t* __restrict__ fmask, const uint8_t* __restrict__ mmask,
                                                       const float* __restrict__ C, bsp_metric_args a, double* __restrict__ partial) {
  constexpr int NG = MODE == 0 ? 192 : 576;
  constexpr int ROW = NG + BSP_NSCAL;
  __shared__ float s_c[192];
  __shared__ double s_g[3 * BSP_NT];
  __shared__ float s_w[12 * BSP_NT];
  __shared__ double s_f[BSP_NT];
  __shared__ double s_m[BSP_NT];
  __shared__ int s_code[BSP_NT];

  const int t = threadIdx.x;
  const int cell = blockIdx.x / a.nsplit, split = blockIdx.x % a.nsplit;
  const int ci = cell % a.mesh[0], cj = (cell / a.mesh[0]) % a.mesh[1], ck = cell / (a.mesh[0] * a.mesh[1]);
  const size_t ncp = (size_t)a.lat[0] * a.lat[1] * a.lat[2];
  if (t < 192) {
    const int r = t >> 6, cp = t & 63;
    s_c[t] = C[r * ncp + ((size_t)(ck + (cp >> 4)) * a.lat[1] + (cj + ((cp >> 2) & 3))) * a.lat[0] + ci + (cp & 3)];
  }
  int xlo, xhi, ylo, yhi, zlo, zhi;
  bsp_cell_range(a.Au[0], a.bu[0], ci, a.mesh[0], a.vsize[0], a.margin, xlo, xhi);
  bsp_cell_range(a.Au[1], a.bu[1], cj, a.mesh[1], a.vsize[1], a.margin, ylo, yhi);
  bsp_cell_range(a.Au[2], a.bu[2], ck, a.mesh[2], a.vsize[2], a.margin, zlo, zhi);
  {   // this workgroup's z slab of the box
    const int len = zhi - zlo + 1 > 0 ? (zhi - zlo + 1 + a.nsplit - 1) / a.nsplit : 0;
    const int z0 = zlo + split * len, z1 = z0 + len - 1;
    zlo = z0;
    zhi = z1 < zhi ? z1 : zhi;
  }
  const int bx = xhi - xlo + 1, by = yhi - ylo + 1, bz = zhi - zlo + 1;
  const int kmax = bx > 0 ? (bx + a.stride - 1) / a.stride : 0;
  const long long items = (bx > 0 && by > 0 && bz > 0) ? (long long)kmax * by * bz : 0;

  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  __syncthreads();
  for (long long first = 0; first < items; first += BSP_NT) {
    // ---- phase 1: one candidate sample per thread, staged in slot t
    int code = 0;
    double fd = 0.0, md = 0.0, g[3] = {0.0, 0.0, 0.0};
    float w[12];
    for (int k = 0; k < 12; ++k) w[k] = 0.0f;
    const long long item = first + t;
    if (item < items) {
      const long long row = item / kmax;
      const int k = (int)(item % kmax);
      const int y = ylo + (int)(row % by), z = zlo + (int)(row / by);
      const size_t lin0 = ((size_t)z * a.vsize[1] + y) * a.vsize[0] + xlo;
      const int skip = (int)((a.stride - lin0 % a.stride) % a.stride);
      const long long xl = (long long)xlo + skip + (long long)k * a.stride;
      if (xl <= xhi) {
        const int x = (int)xl;
        const size_t e = (lin0 + (size_t)(x - xlo)) / a.stride;
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
        if (own[0] == ci && own[1] == cj && own[2] == ck) {
          code = BSP_SEEN;
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
          bool masked = false;
          if (!bsp_locate(cf, df, bf_, ff) || !bsp_locate(cm, dm, bm_, fm)) {
            code |= BSP_OUTSIDE;
          } else {
            if (fmask) {
              const int qx = (int)floor(cf[0] + 0.5), qy = (int)floor(cf[1] + 0.5), qz = (int)floor(cf[2] + 0.5);
              masked = !fmask[((size_t)qz * df.ny + qy) * df.nx + qx];
            }
            if (!masked && mmask) {
              const int qx = (int)floor(cm[0] + 0.5), qy = (int)floor(cm[1] + 0.5), qz = (int)floor(cm[2] + 0.5);
              masked = !mmask[((size_t)qz * dm.ny + qy) * dm.nx + qx];
            }
            if (masked) {
              code |= BSP_MASKED;
            } else {
              code |= BSP_VALID | (inside ? BSP_GRAD : 0);
              const float fval = pp_trilinear(F, df.nx, df.ny, df.nz, bf_[0], ff[0], bf_[1], ff[1], bf_[2], ff[2]);
              int x0, x1, y0, y1, z0, z1;
              float ux, uy, uz;
              pp_axis_setup(bm_[0], fm[0], dm.nx, x0, x1, ux);
              pp_axis_setup(bm_[1], fm[1], dm.ny, y0, y1, uy);
              pp_axis_setup(bm_[2], fm[2], dm.nz, z0, z1, uz);
              const size_t sy = dm.nx, sz = (size_t)dm.nx * dm.ny;
              const size_t o[8] = {z0 * sz + y0 * sy + x0, z0 * sz + y0 * sy + x1, z0 * sz + y1 * sy + x0, z0 * sz + y1 * sy + x1,
                                   z1 * sz + y0 * sy + x0, z1 * sz + y0 * sy + x1, z1 * sz + y1 * sy + x0, z1 * sz + y1 * sy + x1};
              float am[8], gi[3];
              if (a.grad4) {   // (uniform) gradient and intensity of a corner in one 16-byte element
                float c4[4][8];
                for (int q = 0; q < 8; ++q) {
                  const float4 p = a.grad4[o[q]];
                  c4[0][q] = p.x, c4[1][q] = p.y, c4[2][q] = p.z, c4[3][q] = p.w;
                }
                for (int r = 0; r < 3; ++r) gi[r] = bsp_lerp8(c4[r], ux, uy, uz);
                for (int q = 0; q < 8; ++q) am[q] = c4[3][q];
              } else {
                for (int q = 0; q < 8; ++q) am[q] = M[o[q]];
                if (a.grad) {
                  const size_t N = sz * dm.nz;
                  for (int r = 0; r < 3; ++r) {
                    float ag[8];
                    for (int q = 0; q < 8; ++q) ag[q] = a.grad[r * N + o[q]];
                    gi[r] = bsp_lerp8(ag, ux, uy, uz);
                  }
                } else {   // gradient of the trilinear interpolant, per moving voxel (as k_metric_affine)
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
              const float mval = bsp_lerp8(am, ux, uy, uz);
              fd = fval;
              md = mval;
              const double scale = MODE == 0 ? -2.0 * (fd - md) : 1.0;
              for (int r = 0; r < 3; ++r)
                g[r] = scale * ((double)gi[0] * a.Md[0 * 3 + r] + (double)gi[1] * a.Md[1 * 3 + r] + (double)gi[2] * a.Md[2 * 3 + r]);
            }
          }
        }
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

// the ten scalar moments of all rows, one fixed tree
__global__ void __launch_bounds__(BSP_NT) k_bsp_scalars(const double* __restrict__ partial, int nrows, int row, int off,
                                                        double* __restrict__ out) {
  __shared__ double red[BSP_NSCAL * BSP_NT];
  double acc[BSP_NSCAL];
  for (int q = 0; q < BSP_NSCAL; ++q) acc[q] = 0.0;
  for (int i = threadIdx.x; i < nrows; i += BSP_NT)
    for (int q = 0; q < BSP_NSCAL; ++q) acc[q] += partial[(size_t)i * row + off + q];
  for (int q = 0; q < BSP_NSCAL; ++q) red[q * BSP_NT + threadIdx.x] = acc[q];
  __syncthreads();
  for (int s = BSP_NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int q = 0; q < BSP_NSCAL; ++q) red[q * BSP_NT + threadIdx.x] += red[q * BSP_NT + threadIdx.x + s];
    __syncthreads();
  }
  if ((int)threadIdx.x < BSP_NSCAL) out[threadIdx.x] = red[threadIdx.x * BSP_NT];
}

// gradient[p] for coefficient p = (r, k, j, i): the rows of the cells (and slabs) that cover control point (i, j, k), added in a
// fixed order, then the metric's normalisation from the scalar moments
template <int MODE>
__global__ void __launch_bounds__(BSP_NT) k_bsp_gather(const double* __restrict__ partial, const double* __restrict__ scal,
                                                       bsp_metric_args a, double* __restrict__ gradient) {
  constexpr int NG = MODE == 0 ? 192 : 576;
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

extern "C" int pp_bspline_metric_f32(pp_ctx* ctx, int metric, const float* fixed, const pp_geom* fixed_geom, const float* moving,
                                     const pp_geom* moving_geom, const pp_geom* virt, int stride, const uint8_t* fixed_mask,
                                     const uint8_t* moving_mask, const float* coefficients, const pp_geom* lattice, double jitter_bound,
                                     double* value, double* stats, double* gradient) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, fixed && moving && coefficients && value && gradient, "pp_bspline_metric_f32: NULL argument");
  PP_REQUIRE(ctx, metric == PP_BSPLINE_MEAN_SQUARES || metric == PP_BSPLINE_CORRELATION,
             "pp_bspline_metric_f32: metric must be 0 (mean squares) or 1 (correlation)");
  PP_REQUIRE(ctx, stride >= 1, "pp_bspline_metric_f32: stride must be at least 1");
  PP_REQUIRE(ctx, jitter_bound >= 0.0 && jitter_bound < 1.0e6, "pp_bspline_metric_f32: jitter_bound must be a finite, non-negative number of voxels");
  int rc = bsp_lattice_check(ctx, lattice, "pp_bspline_metric_f32 lattice");
  if (rc) return rc;
  if ((rc = pp_geom_check(ctx, fixed_geom, "pp_bspline_metric_f32 fixed")) != PP_OK) return rc;
  if ((rc = pp_geom_check(ctx, moving_geom, "pp_bspline_metric_f32 moving")) != PP_OK) return rc;
  if ((rc = pp_geom_check(ctx, virt, "pp_bspline_metric_f32 virtual")) != PP_OK) return rc;
  if (!bsp_same_direction(lattice, fixed_geom) || !bsp_same_direction(lattice, virt))
    return pp_fail(ctx, PP_ERR_DIRECTION,
                   "pp_bspline_metric_f32: the lattice, the virtual grid and the fixed image must share their direction cosines");

  bsp_metric_args a;
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
    if (!(a.Au[k] > 0.0)) return pp_fail(ctx, PP_ERR_DIRECTION, "pp_bspline_metric_f32: lattice axis %d does not run along the virtual grid's", k);
  }
  for (int k = 0; k < 9; ++k)
    if (k % 4 != 0 && std::fabs(mu.A[k]) > 1e-9 * a.Au[k / 3])
      return pp_fail(ctx, PP_ERR_DIRECTION, "pp_bspline_metric_f32: the lattice is oblique to the virtual grid");
  a.stride = stride;
  a.margin = (int)std::ceil(jitter_bound) + 1;   // + 1: the box edges are divisions, the ownership test a multiplication
  const size_t nvirt = pp_nvox(virt->size);
  const size_t nsamp = (nvirt + stride - 1) / stride;
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
  const size_t ncp = pp_nvox(lattice->size);
  // enough workgroups for the card: a mesh of few cells is cut into z slabs (at most 16; the count is a function of the mesh
  // alone, so the summation order -- and with it every bit of the result -- is too)
  int nsplit = 1;
  if (ncells < 1024) nsplit = (int)std::min<size_t>(16, (1024 + ncells - 1) / ncells);
  a.nsplit = nsplit;
  const int ROW = (metric == 0 ? 192 : 576) + BSP_NSCAL;
  const size_t nrows = ncells * nsplit;
  PP_REQUIRE(ctx, nrows < (size_t)1 << 30, "pp_bspline_metric_f32: mesh too fine");
  rc = pp_reserve(ctx, pp_align_up(nrows * ROW * sizeof(double), 256) + 256 + pp_align_up(3 * ncp * sizeof(double), 256));
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  double* partial = cv.take<double>(nrows * ROW);
  double* scal = cv.take<double>(BSP_NSCAL);
  double* dgrad = cv.take<double>(3 * ncp);
  const pp_dims df{fixed_geom->size[0], fixed_geom->size[1], fixed_geom->size[2]};
  const pp_dims dm{moving_geom->size[0], moving_geom->size[1], moving_geom->size[2]};
  {
    pp_prof_scope prof(ctx, "bspline_metric");
    if (metric == 0)
      hipLaunchKernelGGL((k_bsp_metric<0>), dim3((unsigned)nrows), dim3(BSP_NT), 0, ctx->stream, fixed, df, moving, dm, fixed_mask, moving_mask,
                         coefficients, a, partial);
    else
      hipLaunchKernelGGL((k_bsp_metric<1>), dim3((unsigned)nrows), dim3(BSP_NT), 0, ctx->stream, fixed, df, moving, dm, fixed_mask, moving_mask,
                         coefficients, a, partial);
    PP_LAUNCH_CHECK(ctx, "k_bsp_metric");
  }
  {
    pp_prof_scope prof(ctx, "bspline_gather");
    hipLaunchKernelGGL(k_bsp_scalars, dim3(1), dim3(BSP_NT), 0, ctx->stream, (const double*)partial, (int)nrows, ROW, ROW - BSP_NSCAL, scal);
    PP_LAUNCH_CHECK(ctx, "k_bsp_scalars");
    const unsigned gb = (unsigned)((3 * ncp + BSP_NT - 1) / BSP_NT);
    if (metric == 0)
      hipLaunchKernelGGL((k_bsp_gather<0>), dim3(gb), dim3(BSP_NT), 0, ctx->stream, (const double*)partial, (const double*)scal, a, dgrad);
    else
      hipLaunchKernelGGL((k_bsp_gather<1>), dim3(gb), dim3(BSP_NT), 0, ctx->stream, (const double*)partial, (const double*)scal, a, dgrad);
    PP_LAUNCH_CHECK(ctx, "k_bsp_gather");
  }
  double s[BSP_NSCAL];
  rc = pp_read_back(ctx, scal, s, sizeof(s));
  if (rc) return rc;
  PP_HIP(ctx, hipMemcpyAsync(gradient, dgrad, 3 * ncp * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) stats[0] = s[0], stats[1] = s[7], stats[2] = s[8], stats[3] = s[9];
  if (s[9] != (double)nsamp)
    return pp_fail(ctx, PP_ERR_ARG, "pp_bspline_metric_f32: %.0f of %zu samples visited -- a sample's jitter exceeds jitter_bound = %g voxels",
                   s[9], nsamp, jitter_bound);
  const double cnt = s[0];
  if (cnt <= 0.0) return pp_fail(ctx, PP_ERR_NO_OVERLAP, "pp_bspline_metric_f32: no valid sample points");
  if (metric == 0) {
    *value = s[6] / cnt;
  } else {
    const double fbar = s[1] / cnt, mbar = s[2] / cnt;
    const double sff = s[3] - cnt * fbar * fbar, smm = s[4] - cnt * mbar * mbar, sfm = s[5] - cnt * fbar * mbar;
    *value = (sff <= 1e-300 || smm <= 1e-300) ? 0.0 : -(sfm * sfm) / (sff * smm);
  }
  return PP_OK;
}
