// platipy_amd/csrc/pp_field_inverse.h -- what a user does with a registration's displacement field: its inverse
// (sitk.InvertDisplacementField, the operation the reference names at visualisation/visualiser.py:1536), the residual of a
// forward / backward pair, and the Jacobian determinant (sitk.DisplacementFieldJacobianDeterminant).  #included at the end of
// pp_resample.hip: it uses that file's NT, grid3_for, band_for / pp_band_block and the sampling helpers of pp_internal.h.
//
// Inversion [ITK-upstream, unverified here: itk::InvertDisplacementFieldImageFilter of ITK 5.3 as recalled].  u is the
// input, v the estimate.  Iteration k = 1, 2, ...:
//     c(x) = v(x) + u_lin(p + v(x)) where the warped point is inside u's buffer, v(x) otherwise (pp_inside1 / pp_trilinear);
//     r = -c;  s(x) = sqrt(sum_d (r_d / spacing_d)^2)  (index-axis spacings on physical components: ITK's quirk);
//     M = max s, mean = sum s / N;  eps = 0.75 (k = 1) or 0.5;  if s > eps M: r *= eps M / s;  v += eps r;
//     v = 0 on the border voxels when the boundary condition is enforced.
// The loop runs while k <= max_iterations and M > max_tol and mean > mean_tol, both taken from iteration k - 1.
//
// One launch per iteration and no host read in between.  u never changes and the update of voxel x needs only v(x), r(x)
// and the global M, so launch k first applies the pending update of iteration k - 1 (M_{k-1} read from device memory),
// then gathers u at x + v(x), stores r_k and reduces M_k and sum s_k.  r is kept in scratch between launches: 12 B read v +
// 12 B read r + 12 B write v + 12 B write r + 12 B compulsory gather of u = 60 B per voxel and iteration, one gather.  (The
// alternative recomputes r_{k-1} with a second gather: 48 B, twice the gather instructions -- and the sibling
// k_compose_same_grid is bound by its gather instructions, not by bytes.)  The stop test runs on the device: row k of
// the per-iteration table stays at -1 until launch k has run, launch k returns at once when row k - 1 is -1 or its values
// are within the thresholds.  The update of the last executed iteration is applied by k_invert_apply, which also posts the
// result.  Reductions are integers only -- M by atomicMax on the bit pattern of a non-negative float, the sum in 2^-24
// fixed point by 64-bit integer adds -- so two calls return the same bits.  What the reduction costs decided the launch
// shape (512 x 512 x 256, ms per iteration inside a ten-iteration call, profiles/field_inverse_bench.json): one voxel per
// thread with every 64 x 4 block adding to ONE max and ONE sum ran at 3.27; the blocks spread over 16 accumulators 256 B
// apart (and the max posted only where it improved on what the block read there), 2.65; each block walking FI_ZC = 8
// consecutive planes of its tile before it reduces in LDS and posts once, 1.19; the same without the read in front of the
// max, 1.07 (3.8 TB/s of the 60 B; 1.09 with it in another run, so the read bought nothing and is gone -- in front of the
// Jacobian's min / max it cost 0.4 ms).
//
// Jacobian determinant [ITK-upstream, unverified here: itk::DisplacementFieldJacobianDeterminantFilter].
//     J[i][j] = 0.5 w_i (u_j(x + e_i) - u_j(x - e_i)) + delta_ij,  w_i = 1 / spacing_i or 1;  a neighbour outside the buffer
//     is the voxel itself (zero-flux Neumann); direction cosines are not applied.
// One pass: a 32 x 8 tile of (x, y) columns marches a chunk of planes with the +-z neighbours in a register window and the
// +-x / +-y neighbours in an LDS tile with a one-voxel halo, every load from clamped coordinates so that the tile IS the
// Neumann extension.  12 B read + 4 B written per voxel.  min / max by integer atomics on order-preserving keys, the sum in
// 2^-24 fixed point, the counts in 64-bit integers: the statistics are bit-reproducible too.
#pragma once

#include "pp_reduce.h"

namespace {

constexpr int FI_MAX_ITERATIONS = 256;           // rows of the per-iteration table
constexpr int FI_SLOTS = 16;                     // accumulators per iteration, 256 B apart (one address would serialise every block's atomics)
constexpr int FI_ZC = 8;                         // planes a block of the iteration kernel walks before it posts its max and sum
constexpr double FI_FIXED_ONE = 16777216.0;      // 2^24: one unit of the fixed-point sums
constexpr double FI_FIXED_MAX = 1.0e18;          // a single term is clamped: eight of them stay below 2^63

// device control block of one inversion: header, then FI_SLOTS accumulators per iteration (row 0 unused)
struct fi_slot {
  unsigned long long sum;           // 2^-24 fixed point
  int mbits;                        // bit pattern of a non-negative float; -1: no block has posted here
  int pad[61];
};
struct fi_ctl {
  int last;                         // last executed iteration
  int last_mbits;                   // its M (bit pattern) and sum, posted by k_invert_apply
  unsigned long long last_sum;
  int pad[60];
  fi_slot slot[FI_MAX_ITERATIONS + 1][FI_SLOTS];
};
static_assert(sizeof(fi_slot) == 256, "one accumulator per 256 bytes");

// M (bit pattern, -1 when the iteration has not run) and the sum of iteration k
__device__ __forceinline__ int fi_fold(const fi_ctl* ctl, int k, unsigned long long& sum) {
  int mb = -1;
  sum = 0ull;
  for (int j = 0; j < FI_SLOTS; ++j) {
    const int m = ctl->slot[k][j].mbits;
    mb = m > mb ? m : mb;
    sum += ctl->slot[k][j].sum;
  }
  return mb;
}

struct fi_scale {
  float m[9];      // physical displacement -> continuous-index displacement: diag(1 / spacing) Dir^T
  float isx, isy, isz;
};

__device__ __forceinline__ unsigned long long fi_to_fixed(float s) {
  const double t = fmin((double)s * FI_FIXED_ONE + 0.5, FI_FIXED_MAX);   // (fmin drops a NaN)
  return (unsigned long long)t;
}
__device__ __forceinline__ float fi_scaled_norm(float rx, float ry, float rz, const fi_scale& sc) {
  const float ax = rx * sc.isx, ay = ry * sc.isy, az = rz * sc.isz;
  return sqrtf(ax * ax + ay * ay + az * az);
}
// v += eps r', r' = r shortened to eps M where its scaled norm is longer; then the boundary rule
__device__ __forceinline__ void fi_update(float& vx, float& vy, float& vz, float rx, float ry, float rz, const fi_scale& sc, float eps,
                                          float M, bool border) {
  const float s = fi_scaled_norm(rx, ry, rz, sc);
  const float lim = eps * M;
  if (s > lim) {
    const float f = lim / s;
    rx *= f; ry *= f; rz *= f;
  }
  vx += eps * rx; vy += eps * ry; vz += eps * rz;
  if (border) vx = vy = vz = 0.0f;
}

// Block-wide max of non-negative float bit patterns and sum of 64-bit integers; every thread of the block must call it.
__device__ __forceinline__ void fi_block_reduce(int& mx, unsigned long long& sm, int* smx, unsigned long long* ssm) {
  const int t = threadIdx.y * blockDim.x + threadIdx.x;
  smx[t] = mx;
  ssm[t] = sm;
  pp_block_tree<NT>(t, [=](int a, int b) {
    smx[a] = smx[a] > smx[b] ? smx[a] : smx[b];
    ssm[a] += ssm[b];
  });
  mx = smx[0];
  sm = ssm[0];
}

// Iteration k.  r == NULL: nothing is kept (the residual of a forward / backward pair); norm_out: s per voxel, or NULL.
template <bool PAIRS>
__global__ void __launch_bounds__(NT) k_invert_iter(const float* __restrict__ u, float* __restrict__ v, float* __restrict__ r,
                                                    float* __restrict__ norm_out, pp_dims d, fi_scale sc, int k, double max_tol,
                                                    double mean_tol, int enforce, fi_ctl* __restrict__ ctl, pp_band B) {
  __shared__ int smx[NT];
  __shared__ unsigned long long ssm[NT];
  const size_t N = (size_t)d.nx * d.ny * d.nz;
  float Mprev = 0.0f;
  if (k > 1) {   // the stop test, on the values of launch k - 1 (the same decision in every thread of the launch)
    unsigned long long sum_prev;
    const int mb = fi_fold(ctl, k - 1, sum_prev);
    if (mb < 0) return;
    Mprev = __builtin_bit_cast(float, mb);
    const double mean = (double)sum_prev / FI_FIXED_ONE / (double)N;
    if (!((double)Mprev > max_tol && mean > mean_tol)) return;
  }
  unsigned bx_, by_, bz_;
  if (!pp_band_block(B, bx_, by_, bz_)) return;
  const int x = bx_ * blockDim.x + threadIdx.x, y = by_ * blockDim.y + threadIdx.y;
  const int z0 = bz_ * FI_ZC, z1 = z0 + FI_ZC < d.nz ? z0 + FI_ZC : d.nz;
  int mx = 0;
  unsigned long long sm = 0ull;
  if (x < d.nx && y < d.ny) for (int z = z0; z < z1; ++z) {
    const size_t i = ((size_t)z * d.ny + y) * d.nx + x;
    float vx = v[i], vy = v[N + i], vz = v[2 * N + i];
    if (k > 1) {
      const bool border = enforce && (x == 0 || x == d.nx - 1 || y == 0 || y == d.ny - 1 || z == 0 || z == d.nz - 1);
      fi_update(vx, vy, vz, r[i], r[N + i], r[2 * N + i], sc, k == 2 ? 0.75f : 0.5f, Mprev, border);
      v[i] = vx; v[N + i] = vy; v[2 * N + i] = vz;
    }
    int bx, by, bz;
    float fx, fy, fz;
    pp_split(x, sc.m[0] * vx + sc.m[1] * vy + sc.m[2] * vz, bx, fx);
    pp_split(y, sc.m[3] * vx + sc.m[4] * vy + sc.m[5] * vz, by, fy);
    pp_split(z, sc.m[6] * vx + sc.m[7] * vy + sc.m[8] * vz, bz, fz);
    float cx = vx, cy = vy, cz = vz;
    if (pp_inside1(bx, fx, d.nx) && pp_inside1(by, fy, d.ny) && pp_inside1(bz, fz, d.nz)) {
      if (PAIRS) {
        cx += pp_trilinear_pairs(u, d.nx, d.ny, d.nz, bx, fx, by, fy, bz, fz);
        cy += pp_trilinear_pairs(u + N, d.nx, d.ny, d.nz, bx, fx, by, fy, bz, fz);
        cz += pp_trilinear_pairs(u + 2 * N, d.nx, d.ny, d.nz, bx, fx, by, fy, bz, fz);
      } else {
        cx += pp_trilinear(u, d.nx, d.ny, d.nz, bx, fx, by, fy, bz, fz);
        cy += pp_trilinear(u + N, d.nx, d.ny, d.nz, bx, fx, by, fy, bz, fz);
        cz += pp_trilinear(u + 2 * N, d.nx, d.ny, d.nz, bx, fx, by, fy, bz, fz);
      }
    }
    const float rx = -cx, ry = -cy, rz = -cz;
    float s = fi_scaled_norm(rx, ry, rz, sc);
    if (!(s == s)) s = INFINITY;   // a NaN residual never passes for "converged"
    if (r) {
      r[i] = rx; r[N + i] = ry; r[2 * N + i] = rz;
    }
    if (norm_out) norm_out[i] = s;
    const int sb = __builtin_bit_cast(int, s);
    mx = sb > mx ? sb : mx;
    sm += fi_to_fixed(s);
  }
  fi_block_reduce(mx, sm, smx, ssm);
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    // (mbits is -1 before the launch: the first block's M replaces it, being >= 0)
    fi_slot* slot = &ctl->slot[k][(blockIdx.x + blockIdx.y + blockIdx.z) % FI_SLOTS];
    atomicMax(&slot->mbits, mx);
    atomicAdd(&slot->sum, sm);
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) ctl->last = k;
  }
}

// The pending update of the last executed iteration, and its values into the header.
__global__ void __launch_bounds__(NT) k_invert_apply(float* __restrict__ v, const float* __restrict__ r, pp_dims d, fi_scale sc,
                                                     int enforce, fi_ctl* __restrict__ ctl) {
  const int last = ctl->last;
  if (last < 1) return;
  unsigned long long sum_last;
  const int mb = fi_fold(ctl, last, sum_last);
  if (threadIdx.x == 0 && threadIdx.y == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
    ctl->last_mbits = mb;
    ctl->last_sum = sum_last;
  }
  const size_t N = (size_t)d.nx * d.ny * d.nz;
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y, z = blockIdx.z;
  if (x < d.nx && y < d.ny) {
    const size_t i = ((size_t)z * d.ny + y) * d.nx + x;
    float vx = v[i], vy = v[N + i], vz = v[2 * N + i];
    const bool border = enforce && (x == 0 || x == d.nx - 1 || y == 0 || y == d.ny - 1 || z == 0 || z == d.nz - 1);
    fi_update(vx, vy, vz, r[i], r[N + i], r[2 * N + i], sc, last == 1 ? 0.75f : 0.5f, __builtin_bit_cast(float, mb), border);
    v[i] = vx; v[N + i] = vy; v[2 * N + i] = vz;
  }
}

// the header of a launch sequence that ends without an update (pp_inverse_consistency_f32)
__global__ void k_invert_post(fi_ctl* ctl) {
  const int last = ctl->last;
  if (last < 1) return;
  unsigned long long sum_last;
  ctl->last_mbits = fi_fold(ctl, last, sum_last);
  ctl->last_sum = sum_last;
}

// All three entry points take fields below 2^32 bytes with no axis longer than 65535 (a grid dimension of the apply launch).
int fi_check(pp_ctx* ctx, const pp_geom* g, const char* who, pp_dims* d, fi_scale* sc) {
  int rc = pp_geom_check(ctx, g, "grid");
  if (rc) return rc;
  const size_t N = pp_nvox(g->size);
  if (N * 12u >= ((size_t)1 << 32) || g->size[0] > 65535 || g->size[1] > 65535 || g->size[2] > 65535)
    return pp_fail(ctx, PP_ERR_SIZE, "%s: fields of 2^32 bytes and more, or with an axis longer than 65535, are not taken", who);
  *d = pp_dims{g->size[0], g->size[1], g->size[2]};
  if (sc) {
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) sc->m[a * 3 + c] = (float)(g->direction[c * 3 + a] / g->spacing[a]);
    sc->isx = (float)(1.0 / g->spacing[0]);
    sc->isy = (float)(1.0 / g->spacing[1]);
    sc->isz = (float)(1.0 / g->spacing[2]);
  }
  return PP_OK;
}

int fi_launch_iter(pp_ctx* ctx, const float* u, float* v, float* r, float* norm_out, const pp_dims& d, const fi_scale& sc, int k,
                   double max_tol, double mean_tol, int enforce, fi_ctl* ctl) {
  // 64 x 4 blocks, as the composition's (pp_compose_field_f32), each on FI_ZC consecutive planes of its tile
  const pp_grid3 g3 = grid3_for(d.nx, d.ny, (d.nz + FI_ZC - 1) / FI_ZC, 64u);
  dim3 launch;
  const pp_band B = band_for(g3, &launch);
  if (d.nx >= 2)
    hipLaunchKernelGGL(k_invert_iter<true>, launch, g3.block, 0, ctx->stream, u, v, r, norm_out, d, sc, k, max_tol, mean_tol, enforce, ctl, B);
  else
    hipLaunchKernelGGL(k_invert_iter<false>, launch, g3.block, 0, ctx->stream, u, v, r, norm_out, d, sc, k, max_tol, mean_tol, enforce, ctl, B);
  PP_LAUNCH_CHECK(ctx, "k_invert_iter");
  return PP_OK;
}

__global__ void __launch_bounds__(NT) k_invert_init(fi_ctl* ctl, int rows) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i == 0) {
    ctl->last = ctl->last_mbits = 0;
    ctl->last_sum = 0ull;
  }
  if (i < rows * FI_SLOTS) {
    fi_slot* s = &ctl->slot[0][0] + i;
    s->sum = 0ull;
    s->mbits = -1;
  }
}

// rows 0 ... iterations of the table cleared
int fi_init_ctl(pp_ctx* ctx, fi_ctl* ctl, int iterations) {
  const int rows = iterations + 1;
  hipLaunchKernelGGL(k_invert_init, dim3((unsigned)((rows * FI_SLOTS + NT - 1) / NT)), dim3(NT), 0, ctx->stream, ctl, rows);
  PP_LAUNCH_CHECK(ctx, "k_invert_init");
  return PP_OK;
}

int fi_read_stats(pp_ctx* ctx, const fi_ctl* ctl, size_t N, pp_invert_stats* stats) {
  struct {
    int last, mbits;
    unsigned long long sum;
  } h;
  int rc = pp_read_back(ctx, ctl, &h, sizeof(h));
  if (rc) return rc;
  stats->iterations = h.last;
  stats->reserved = 0;
  if (h.last < 1) {
    stats->max_error_norm = stats->mean_error_norm = INFINITY;
  } else {
    stats->max_error_norm = (double)__builtin_bit_cast(float, h.mbits);
    stats->mean_error_norm = (double)h.sum / FI_FIXED_ONE / (double)N;
  }
  return PP_OK;
}

// ---------------------------------------------------------------------------------------
// Jacobian determinant

constexpr int FJ_TX = 32, FJ_TY = 8, FJ_ZC = 32;   // tile of columns, planes per block
constexpr int FJ_PITCH = FJ_TX + 3;                // tile row: halo, 32, halo (+1: rows on different banks)

struct fj_acc {          // device accumulators of one call
  int min_key, max_key;  // order-preserving keys of the floats
  unsigned long long sum;   // 2^-24 fixed point, two's complement
  unsigned long long count, nonpositive;
};

__device__ __forceinline__ int fj_key(float f) {   // a < b  <=>  key(a) < key(b) as signed integers
  const int b = __builtin_bit_cast(int, f);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__host__ __device__ inline float fj_unkey(int k) {
  return __builtin_bit_cast(float, k >= 0 ? k : k ^ 0x7fffffff);
}

__global__ void k_jacobian_init(fj_acc* a) {
  a->min_key = 0x7fffffff;
  a->max_key = (int)0x80000000;
  a->sum = a->count = a->nonpositive = 0ull;
}

template <bool STATS>
__global__ void __launch_bounds__(NT) k_jacobian_det(const float* __restrict__ u, const uint8_t* __restrict__ mask, float* __restrict__ out,
                                                     pp_dims d, float wx, float wy, float wz, fj_acc* __restrict__ acc) {
  __shared__ float tile[3][FJ_TY + 2][FJ_PITCH];
  __shared__ int s_min[NT], s_max[NT];
  __shared__ unsigned long long s_sum[NT], s_cnt[NT], s_np[NT];
  const int tx = threadIdx.x, ty = threadIdx.y, t = ty * FJ_TX + tx;
  const int x = blockIdx.x * FJ_TX + tx, y = blockIdx.y * FJ_TY + ty;
  const bool live = x < d.nx && y < d.ny;
  const int xc = x < d.nx ? x : d.nx - 1, yc = y < d.ny ? y : d.ny - 1;   // every load from clamped coordinates
  const size_t plane = (size_t)d.nx * d.ny, N = plane * d.nz;
  const size_t col = (size_t)yc * d.nx + xc;
  // halo entry of this thread (t < 80): rows above / below the tile (32 each), columns left / right of it (8 each)
  int hx = 0, hy = 0, hr = 0, hc = 0;
  const bool halo = t < 2 * FJ_TX + 2 * FJ_TY;
  if (halo) {
    if (t < FJ_TX) { hr = 0; hc = t + 1; hx = blockIdx.x * FJ_TX + t; hy = blockIdx.y * FJ_TY - 1; }
    else if (t < 2 * FJ_TX) { hr = FJ_TY + 1; hc = t - FJ_TX + 1; hx = blockIdx.x * FJ_TX + t - FJ_TX; hy = blockIdx.y * FJ_TY + FJ_TY; }
    else if (t < 2 * FJ_TX + FJ_TY) { hr = t - 2 * FJ_TX + 1; hc = 0; hx = blockIdx.x * FJ_TX - 1; hy = blockIdx.y * FJ_TY + t - 2 * FJ_TX; }
    else { hr = t - 2 * FJ_TX - FJ_TY + 1; hc = FJ_TX + 1; hx = blockIdx.x * FJ_TX + FJ_TX; hy = blockIdx.y * FJ_TY + t - 2 * FJ_TX - FJ_TY; }
    hx = pp_clampi(hx, 0, d.nx - 1);
    hy = pp_clampi(hy, 0, d.ny - 1);
  }
  const size_t hcol = (size_t)hy * d.nx + hx;
  const int z0 = blockIdx.z * FJ_ZC, z1 = z0 + FJ_ZC < d.nz ? z0 + FJ_ZC : d.nz;
  float prev[3], cur[3], next[3];
  {
    const size_t zp = (size_t)(z0 > 0 ? z0 - 1 : 0) * plane, zc = (size_t)z0 * plane;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      prev[c] = u[c * N + zp + col];
      cur[c] = u[c * N + zc + col];
    }
  }
  float lmin = INFINITY, lmax = -INFINITY;
  long long lsum = 0;
  unsigned long long lcnt = 0ull, lnp = 0ull;
  for (int z = z0; z < z1; ++z) {
    const size_t zo = (size_t)z * plane, zn = (size_t)(z + 1 < d.nz ? z + 1 : d.nz - 1) * plane;
    __syncthreads();   // the previous plane's tile has been read
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      next[c] = u[c * N + zn + col];
      tile[c][ty + 1][tx + 1] = cur[c];
      if (halo) tile[c][hr][hc] = u[c * N + zo + hcol];
    }
    __syncthreads();
    if (live) {
      float J[3][3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        J[0][c] = 0.5f * wx * (tile[c][ty + 1][tx + 2] - tile[c][ty + 1][tx]);
        J[1][c] = 0.5f * wy * (tile[c][ty + 2][tx + 1] - tile[c][ty][tx + 1]);
        J[2][c] = 0.5f * wz * (next[c] - prev[c]);
      }
      J[0][0] += 1.0f; J[1][1] += 1.0f; J[2][2] += 1.0f;
      const float det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                        J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
      const size_t i = zo + (size_t)y * d.nx + x;
      if (out) out[i] = det;
      if (STATS && (!mask || mask[i])) {
        lmin = fminf(lmin, det);
        lmax = fmaxf(lmax, det);
        const double f = fmax(fmin((double)det * FI_FIXED_ONE, 2.7e11 * FI_FIXED_ONE), -2.7e11 * FI_FIXED_ONE);   // (a NaN becomes a bound)
        lsum += (long long)(f < 0.0 ? f - 0.5 : f + 0.5);
        ++lcnt;
        if (!(det > 0.0f)) ++lnp;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      prev[c] = cur[c];
      cur[c] = next[c];
    }
  }
  if (STATS) {
    s_min[t] = fj_key(lmin);
    s_max[t] = fj_key(lmax);
    s_sum[t] = (unsigned long long)lsum;
    s_cnt[t] = lcnt;
    s_np[t] = lnp;
    pp_block_tree<NT>(t, [&](int a, int b) {
      s_min[a] = s_min[a] < s_min[b] ? s_min[a] : s_min[b];
      s_max[a] = s_max[a] > s_max[b] ? s_max[a] : s_max[b];
      s_sum[a] += s_sum[b];
      s_cnt[a] += s_cnt[b];
      s_np[a] += s_np[b];
    });
    if (t == 0 && s_cnt[0]) {
      atomicMin(&acc->min_key, s_min[0]);
      atomicMax(&acc->max_key, s_max[0]);
      atomicAdd(&acc->sum, s_sum[0]);
      atomicAdd(&acc->count, s_cnt[0]);
      atomicAdd(&acc->nonpositive, s_np[0]);
    }
  }
}

}  // namespace

extern "C" {

int pp_invert_field_f32(pp_ctx* ctx, const float* field, const pp_geom* geom, const float* initial, int max_iterations, double max_tol,
                        double mean_tol, int enforce_boundary, float* inverse_out, pp_invert_stats* stats) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, field && inverse_out && field != inverse_out && initial != inverse_out, "pp_invert_field_f32: NULL or aliased field");
  PP_REQUIRE(ctx, max_iterations >= 0 && max_iterations <= FI_MAX_ITERATIONS, "pp_invert_field_f32: 0 ... 256 iterations");
  PP_REQUIRE(ctx, max_tol == max_tol && mean_tol == mean_tol, "pp_invert_field_f32: a threshold is NaN");
  pp_dims d;
  fi_scale sc;
  int rc = fi_check(ctx, geom, "pp_invert_field_f32", &d, &sc);
  if (rc) return rc;
  const size_t N = pp_nvox(geom->size);
  rc = pp_reserve(ctx, pp_align_up(3 * N * sizeof(float), 256) + pp_align_up(sizeof(fi_ctl), 256));
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  float* r = cv.take<float>(3 * N);
  fi_ctl* ctl = cv.take<fi_ctl>(1);
  rc = fi_init_ctl(ctx, ctl, max_iterations);
  if (rc) return rc;
  if (initial)
    PP_HIP(ctx, hipMemcpyAsync(inverse_out, initial, 3 * N * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  else
    PP_HIP(ctx, hipMemsetAsync(inverse_out, 0, 3 * N * sizeof(float), ctx->stream));
  for (int k = 1; k <= max_iterations; ++k) {
    rc = fi_launch_iter(ctx, field, inverse_out, r, nullptr, d, sc, k, max_tol, mean_tol, enforce_boundary != 0, ctl);
    if (rc) return rc;
  }
  if (max_iterations > 0) {
    const pp_grid3 g3 = grid3_for(d.nx, d.ny, d.nz, 64u);
    hipLaunchKernelGGL(k_invert_apply, g3.grid, g3.block, 0, ctx->stream, inverse_out, r, d, sc, enforce_boundary != 0, ctl);
    PP_LAUNCH_CHECK(ctx, "k_invert_apply");
  }
  return stats ? fi_read_stats(ctx, ctl, N, stats) : PP_OK;
}

int pp_inverse_consistency_f32(pp_ctx* ctx, const float* field, const float* inverse, const pp_geom* geom, float* norm_out,
                               pp_invert_stats* stats) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, field && inverse && stats, "pp_inverse_consistency_f32: NULL argument");
  PP_REQUIRE(ctx, norm_out != field && norm_out != inverse, "pp_inverse_consistency_f32: the norm image aliases a field");
  pp_dims d;
  fi_scale sc;
  int rc = fi_check(ctx, geom, "pp_inverse_consistency_f32", &d, &sc);
  if (rc) return rc;
  rc = pp_reserve(ctx, pp_align_up(sizeof(fi_ctl), 256));
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  fi_ctl* ctl = cv.take<fi_ctl>(1);
  rc = fi_init_ctl(ctx, ctl, 1);
  if (rc) return rc;
  // iteration 1's arm with nothing kept: it reads the estimate and never writes it
  rc = fi_launch_iter(ctx, field, const_cast<float*>(inverse), nullptr, norm_out, d, sc, 1, 0.0, 0.0, 0, ctl);
  if (rc) return rc;
  hipLaunchKernelGGL(k_invert_post, dim3(1), dim3(1), 0, ctx->stream, ctl);
  PP_LAUNCH_CHECK(ctx, "k_invert_post");
  return fi_read_stats(ctx, ctl, pp_nvox(geom->size), stats);
}

int pp_jacobian_determinant_f32(pp_ctx* ctx, const float* field, const pp_geom* geom, int use_image_spacing, const uint8_t* mask,
                                float* det_out, pp_jacobian_stats* stats) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, field && (det_out || stats), "pp_jacobian_determinant_f32: NULL field, or nothing to compute");
  PP_REQUIRE(ctx, det_out != field && (!det_out || (const void*)det_out != (const void*)mask),
             "pp_jacobian_determinant_f32: the output aliases an input");
  pp_dims d;
  int rc = fi_check(ctx, geom, "pp_jacobian_determinant_f32", &d, nullptr);
  if (rc) return rc;
  const float wx = use_image_spacing ? (float)(1.0 / geom->spacing[0]) : 1.0f;
  const float wy = use_image_spacing ? (float)(1.0 / geom->spacing[1]) : 1.0f;
  const float wz = use_image_spacing ? (float)(1.0 / geom->spacing[2]) : 1.0f;
  const dim3 grid((unsigned)((d.nx + FJ_TX - 1) / FJ_TX), (unsigned)((d.ny + FJ_TY - 1) / FJ_TY), (unsigned)((d.nz + FJ_ZC - 1) / FJ_ZC));
  const dim3 block(FJ_TX, FJ_TY, 1);
  if (!stats) {
    hipLaunchKernelGGL(k_jacobian_det<false>, grid, block, 0, ctx->stream, field, mask, det_out, d, wx, wy, wz, (fj_acc*)nullptr);
    PP_LAUNCH_CHECK(ctx, "k_jacobian_det");
    return PP_OK;
  }
  rc = pp_reserve(ctx, 256);
  if (rc) return rc;
  fj_acc* acc = reinterpret_cast<fj_acc*>(ctx->ws);
  hipLaunchKernelGGL(k_jacobian_init, dim3(1), dim3(1), 0, ctx->stream, acc);
  PP_LAUNCH_CHECK(ctx, "k_jacobian_init");
  hipLaunchKernelGGL(k_jacobian_det<true>, grid, block, 0, ctx->stream, field, mask, det_out, d, wx, wy, wz, acc);
  PP_LAUNCH_CHECK(ctx, "k_jacobian_det");
  fj_acc h;
  rc = pp_read_back(ctx, acc, &h, sizeof(h));
  if (rc) return rc;
  stats->count = (int64_t)h.count;
  stats->count_nonpositive = (int64_t)h.nonpositive;
  if (h.count == 0) {
    stats->min = stats->max = stats->mean = NAN;
  } else {
    stats->min = (double)fj_unkey(h.min_key);
    stats->max = (double)fj_unkey(h.max_key);
    stats->mean = (double)(long long)h.sum / FI_FIXED_ONE / (double)h.count;
  }
  return PP_OK;
}

}  // extern "C"
