// platipy_amd/csrc/pp_compare.h -- label comparison metrics: the device side of platipy/imaging/label/comparison.py.
// #included at the end of pp_dist.hip (it uses that file's NT, grid_for, k_border26 and k_contour6).
//
// The reference scores a pair of labels with SimpleITK filters over whole volumes: overlap counts on host arrays,
// LabelContour / BinaryContour volumes, Abs(SignedMaurerDistanceMap) volumes, LabelIntensityStatistics over them.  Here the
// distance maps come from pp_distance_map_f32 and everything that reads them is one pass:
//   overlap counts   |A|, |B|, |A and B|: 16-byte loads of both masks, integer counts, one 64-bit add per block
//   abs range        min / max of |dist| (block partials, then one block), left in device memory for the next pass
//   surface stats    streams the SELECT label 16 voxels a load, skips empty groups, decides "is a sample" on the fly (the
//                    face-contour rule needs no contour volume) and reads the distance map only at the samples: count, sum,
//                    sum of squares, min, max, count <= tau and ITK's 128-bin histogram (the median's source)
//   slice counts     per z slice |a and not b| for the added path length
// Every floating-point sum is a fixed tree (thread, block tree in LDS, block partials folded by one block in block order);
// counts and histogram bins are integers (LDS per block, then one integer atomic per non-empty bin).  No float atomics: a
// rerun gives the same bits.
#pragma once

#include "pp_reduce.h"

namespace {

constexpr int CMP_BINS = PP_SURFACE_BINS;

struct alignas(16) cmp_u32x4 {
  unsigned x, y, z, w;
};

// bit 7 of every byte of w that is not zero
__device__ __forceinline__ unsigned cmp_nonzero_bytes(unsigned w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }

// counts[0..2] += |A|, |B|, |A and B| (non-zero = foreground).  16 voxels a lane and load when `vec`, the tail by bytes.
__global__ void __launch_bounds__(NT) k_overlap_counts(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t n, int vec,
                                                       unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long red[3][NT];
  unsigned long long ca = 0, cb = 0, cab = 0;
  const size_t n16 = vec ? n / 16 : 0;
  for (size_t g = (size_t)blockIdx.x * NT + threadIdx.x; g < n16; g += (size_t)gridDim.x * NT) {
    const cmp_u32x4 wa = reinterpret_cast<const cmp_u32x4*>(a)[g];
    const cmp_u32x4 wb = reinterpret_cast<const cmp_u32x4*>(b)[g];
    const unsigned ma[4] = {cmp_nonzero_bytes(wa.x), cmp_nonzero_bytes(wa.y), cmp_nonzero_bytes(wa.z), cmp_nonzero_bytes(wa.w)};
    const unsigned mb[4] = {cmp_nonzero_bytes(wb.x), cmp_nonzero_bytes(wb.y), cmp_nonzero_bytes(wb.z), cmp_nonzero_bytes(wb.w)};
    for (int k = 0; k < 4; ++k) {
      ca += (unsigned)__builtin_popcount(ma[k]);
      cb += (unsigned)__builtin_popcount(mb[k]);
      cab += (unsigned)__builtin_popcount(ma[k] & mb[k]);
    }
  }
  for (size_t i = n16 * 16 + (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const bool fa = a[i] != 0, fb = b[i] != 0;
    ca += fa;
    cb += fb;
    cab += fa && fb;
  }
  const int t = threadIdx.x;
  red[0][t] = ca;
  red[1][t] = cb;
  red[2][t] = cab;
  pp_block_tree<NT>(t, [&](int a, int b) {
    for (int f = 0; f < 3; ++f) red[f][a] += red[f][b];
  });
  if (t < 3 && red[t][0]) atomicAdd(&counts[t], red[t][0]);
}

// sitk.LabelContour of every z slice taken as a 2-D image: object voxels with a background voxel among their four
// in-plane face neighbours; voxels outside the image are not neighbours.
__global__ void __launch_bounds__(NT) k_contour4(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, pp_dims d) {
  const size_t n = (size_t)d.nx * d.ny * d.nz;
  const size_t sy = d.nx;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    uint8_t c = 0;
    if (mask[i]) {
      const int x = (int)(i % d.nx), y = (int)((i / d.nx) % d.ny);
      c = (x > 0 && !mask[i - 1]) || (x < d.nx - 1 && !mask[i + 1]) || (y > 0 && !mask[i - sy]) || (y < d.ny - 1 && !mask[i + sy]);
    }
    out[i] = c;
  }
}

// min / max of |in|: partials[2 b] = min, [2 b + 1] = max of block b
__global__ void __launch_bounds__(NT) k_abs_range_partial(const float* __restrict__ in, size_t n, float* __restrict__ partials) {
  float lo = FLT_MAX, hi = -FLT_MAX;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const float v = fabsf(in[i]);
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  pp_block_range_store<NT>(lo, hi, partials + 2 * (size_t)blockIdx.x);
}

// what one thread, one block (partials[b]) or the whole pass knows about its samples
struct surf_acc {
  unsigned long long count, cle;
  double sum, sumsq;
  float lo, hi;
};

__device__ __forceinline__ void surf_merge(surf_acc& a, const surf_acc& b) {
  a.count += b.count;
  a.cle += b.cle;
  a.sum += b.sum;
  a.sumsq += b.sumsq;
  a.lo = fminf(a.lo, b.lo);
  a.hi = fmaxf(a.hi, b.hi);
}

// the histogram's range and the tau test, in fp64 like ITK's histogram and the reference's `dist <= tau`
struct surf_bins {
  double lo, width, tau;   // width = hi - lo; <= 0: every value falls into bin 0
  int on;
};

// k_contour6's rule for one voxel of the label
__device__ __forceinline__ bool surf_on_face_contour(const uint8_t* __restrict__ m, size_t i, const pp_dims& d) {
  const size_t sy = d.nx, sz = (size_t)d.nx * d.ny;
  const int x = (int)(i % d.nx), y = (int)((i / d.nx) % d.ny), z = (int)(i / sz);
  return (x > 0 && !m[i - 1]) || (x < d.nx - 1 && !m[i + 1]) || (y > 0 && !m[i - sy]) || (y < d.ny - 1 && !m[i + sy]) ||
         (z > 0 && !m[i - sz]) || (z < d.nz - 1 && !m[i + sz]);
}

// voxel i of the label is non-zero: is it a sample, and with which value
template <int MODE>
__device__ __forceinline__ void surf_visit(const uint8_t* __restrict__ select, const float* __restrict__ dist, size_t i, const pp_dims& d,
                                           const surf_bins& hb, surf_acc& acc, unsigned* shist) {
  if (MODE == PP_SURFACE_CONTOUR_ABS && !surf_on_face_contour(select, i, d)) return;
  float v = dist[i];
  if (MODE == PP_SURFACE_CONTOUR_ABS) v = fabsf(v);
  if (MODE == PP_SURFACE_LABEL_POS) v = fmaxf(v, 0.0f);
  const double dv = (double)v;
  acc.count += 1;
  acc.cle += dv <= hb.tau;
  acc.sum += dv;
  acc.sumsq += dv * dv;
  acc.lo = fminf(acc.lo, v);
  acc.hi = fmaxf(acc.hi, v);
  if (hb.on) {
    int bin = 0;
    if (hb.width > 0.0) {
      const double x = (dv - hb.lo) / hb.width * (double)CMP_BINS;
      bin = x >= (double)(CMP_BINS - 1) ? CMP_BINS - 1 : (x > 0.0 ? (int)x : 0);
    }
    atomicAdd(&shist[bin], 1u);
  }
}

template <int MODE>
__global__ void __launch_bounds__(NT) k_surface_stats(const uint8_t* __restrict__ select, const float* __restrict__ dist, pp_dims d, int vec,
                                                      double tau, const float* __restrict__ range, surf_acc* __restrict__ partials,
                                                      unsigned long long* __restrict__ hist) {
  __shared__ unsigned shist[CMP_BINS];
  __shared__ surf_acc sm[NT];
  const int t = threadIdx.x;
  surf_bins hb;
  hb.on = range != nullptr;
  hb.lo = hb.on ? (double)range[0] : 0.0;
  hb.width = hb.on ? (double)range[1] - (double)range[0] : 0.0;
  hb.tau = tau;
  if (t < CMP_BINS) shist[t] = 0u;
  __syncthreads();
  surf_acc acc{0ull, 0ull, 0.0, 0.0, FLT_MAX, -FLT_MAX};
  const size_t n = (size_t)d.nx * d.ny * d.nz;
  const size_t n16 = vec ? n / 16 : 0;
  for (size_t g = (size_t)blockIdx.x * NT + t; g < n16; g += (size_t)gridDim.x * NT) {
    const cmp_u32x4 w = reinterpret_cast<const cmp_u32x4*>(select)[g];
    if ((w.x | w.y | w.z | w.w) == 0u) continue;
    const unsigned word[4] = {w.x, w.y, w.z, w.w};
    for (int k = 0; k < 16; ++k)
      if ((word[k >> 2] >> (8 * (k & 3))) & 0xffu) surf_visit<MODE>(select, dist, g * 16 + k, d, hb, acc, shist);
  }
  for (size_t i = n16 * 16 + (size_t)blockIdx.x * NT + t; i < n; i += (size_t)gridDim.x * NT)
    if (select[i]) surf_visit<MODE>(select, dist, i, d, hb, acc, shist);
  sm[t] = acc;
  pp_block_tree<NT>(t, [&](int a, int b) { surf_merge(sm[a], sm[b]); });
  if (t == 0) partials[blockIdx.x] = sm[0];
  if (hb.on && t < CMP_BINS && shist[t]) atomicAdd(&hist[t], (unsigned long long)shist[t]);
}

// One block: thread t folds the partials of blocks t, t + NT, ... in that order, then the block tree.
__global__ void __launch_bounds__(NT) k_surface_final(const surf_acc* __restrict__ partials, int nb, const float* __restrict__ range,
                                                      pp_surface_stats* __restrict__ out) {
  __shared__ surf_acc sm[NT];
  const int t = threadIdx.x;
  surf_acc acc{0ull, 0ull, 0.0, 0.0, FLT_MAX, -FLT_MAX};
  for (int b = t; b < nb; b += NT) surf_merge(acc, partials[b]);
  sm[t] = acc;
  pp_block_tree<NT>(t, [&](int a, int b) { surf_merge(sm[a], sm[b]); });
  if (t == 0) {
    out->count = (int64_t)sm[0].count;
    out->count_le_tau = (int64_t)sm[0].cle;
    out->sum = sm[0].sum;
    out->sum_sq = sm[0].sumsq;
    out->min = sm[0].lo;
    out->max = sm[0].hi;
    out->range_lo = range ? range[0] : 0.0f;
    out->range_hi = range ? range[1] : 0.0f;
  }
}

// Block (z, c) counts part c of slice z: per_slice[z] += |a != 0 and not_b == 0|.  4 voxels a lane and load when `vec`.
__global__ void __launch_bounds__(NT) k_slice_masked_count(const uint8_t* __restrict__ a, const uint8_t* __restrict__ not_b, size_t slice,
                                                           int chunks, size_t per, int vec, unsigned long long* __restrict__ per_slice) {
  __shared__ unsigned red[NT];
  const size_t z = blockIdx.x / (unsigned)chunks, c = blockIdx.x % (unsigned)chunks;
  const size_t begin = c * per, end = begin + per < slice ? begin + per : slice;   // per is a multiple of 4
  const uint8_t* pa = a + z * slice;
  const uint8_t* pb = not_b ? not_b + z * slice : nullptr;
  unsigned cnt = 0;
  const int t = threadIdx.x;
  for (size_t i = begin + 4 * (size_t)t; i < end; i += 4 * (size_t)NT) {
    if (vec && i + 4 <= end) {
      const unsigned ma = cmp_nonzero_bytes(*reinterpret_cast<const unsigned*>(pa + i));
      const unsigned mb = pb ? cmp_nonzero_bytes(*reinterpret_cast<const unsigned*>(pb + i)) : 0u;
      cnt += (unsigned)__builtin_popcount(ma & ~mb);
    } else {
      for (size_t e = i; e < end && e < i + 4; ++e) cnt += pa[e] != 0 && !(pb && pb[e] != 0);
    }
  }
  red[t] = cnt;
  pp_block_tree<NT>(t, [&](int a, int b) { red[a] += red[b]; });
  if (t == 0 && red[0]) atomicAdd(&per_slice[z], (unsigned long long)red[0]);
}

bool cmp_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

extern "C" {

int pp_overlap_counts_u8(pp_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, int64_t counts[3]) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, a && b && counts && n > 0, "pp_overlap_counts_u8: NULL or empty argument");
  int rc = pp_reserve(ctx, 256);
  if (rc) return rc;
  unsigned long long* dcounts = reinterpret_cast<unsigned long long*>(ctx->ws);
  PP_HIP(ctx, hipMemsetAsync(dcounts, 0, 3 * sizeof(unsigned long long), ctx->stream));
  const int vec = cmp_aligned(a, 16) && cmp_aligned(b, 16);
  hipLaunchKernelGGL(k_overlap_counts, dim3(grid_for(vec ? (n + 15) / 16 : n, 2048u)), dim3(NT), 0, ctx->stream, a, b, n, vec, dcounts);
  PP_LAUNCH_CHECK(ctx, "k_overlap_counts");
  return pp_read_back(ctx, dcounts, counts, 3 * sizeof(int64_t));
}

int pp_binary_contour_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], int fully_connected, uint8_t* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, mask && size && out && mask != out, "pp_binary_contour_u8: NULL or aliased argument");
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_binary_contour_u8: empty volume");
  const pp_dims d{size[0], size[1], size[2]};
  if (fully_connected) {
    hipLaunchKernelGGL(k_border26, dim3(grid_for(pp_nvox(size))), dim3(NT), 0, ctx->stream, mask, out, d);
    PP_LAUNCH_CHECK(ctx, "k_border26");
  } else {
    hipLaunchKernelGGL(k_contour6, dim3(grid_for(pp_nvox(size))), dim3(NT), 0, ctx->stream, mask, out, d);
    PP_LAUNCH_CHECK(ctx, "k_contour6");
  }
  return PP_OK;
}

int pp_slice_contour_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], uint8_t* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, mask && size && out && mask != out, "pp_slice_contour_u8: NULL or aliased argument");
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_slice_contour_u8: empty volume");
  const pp_dims d{size[0], size[1], size[2]};
  hipLaunchKernelGGL(k_contour4, dim3(grid_for(pp_nvox(size))), dim3(NT), 0, ctx->stream, mask, out, d);
  PP_LAUNCH_CHECK(ctx, "k_contour4");
  return PP_OK;
}

int pp_abs_range_f32(pp_ctx* ctx, const float* in, size_t n, float* device_range) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, in && device_range && n > 0, "pp_abs_range_f32: NULL or empty argument");
  const unsigned nb = grid_for(n, 2048u);
  int rc = pp_reserve(ctx, pp_align_up(2 * (size_t)nb * sizeof(float), 256));
  if (rc) return rc;
  float* partials = reinterpret_cast<float*>(ctx->ws);
  hipLaunchKernelGGL(k_abs_range_partial, dim3(nb), dim3(NT), 0, ctx->stream, in, n, partials);
  PP_LAUNCH_CHECK(ctx, "k_abs_range_partial");
  hipLaunchKernelGGL((k_range_fold<NT, float>), dim3(1), dim3(NT), 0, ctx->stream, (const float*)partials, (int)nb, device_range);
  PP_LAUNCH_CHECK(ctx, "k_range_fold");
  return PP_OK;
}

int pp_surface_stats_f32(pp_ctx* ctx, const uint8_t* select, const float* dist, const pp_geom* g, int mode, double tau,
                         const float* device_range, pp_surface_stats* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, select && dist && out, "pp_surface_stats_f32: NULL argument");
  PP_REQUIRE(ctx, cmp_aligned(out, 8), "pp_surface_stats_f32: out must be 8-byte aligned");
  PP_REQUIRE(ctx, mode == PP_SURFACE_CONTOUR_ABS || mode == PP_SURFACE_LABEL_POS || mode == PP_SURFACE_NONZERO,
             "pp_surface_stats_f32: unknown mode");
  int rc = pp_geom_check(ctx, g, "grid");
  if (rc) return rc;
  const pp_dims d{g->size[0], g->size[1], g->size[2]};
  const size_t n = pp_nvox(g->size);
  const int vec = cmp_aligned(select, 16);
  const unsigned nb = grid_for(vec ? (n + 15) / 16 : n, 2048u);
  rc = pp_reserve(ctx, pp_align_up((size_t)nb * sizeof(surf_acc), 256));
  if (rc) return rc;
  surf_acc* partials = reinterpret_cast<surf_acc*>(ctx->ws);
  PP_HIP(ctx, hipMemsetAsync(out, 0, sizeof(pp_surface_stats), ctx->stream));
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(out->hist);
  if (mode == PP_SURFACE_CONTOUR_ABS)
    hipLaunchKernelGGL(k_surface_stats<PP_SURFACE_CONTOUR_ABS>, dim3(nb), dim3(NT), 0, ctx->stream, select, dist, d, vec, tau, device_range,
                       partials, hist);
  else if (mode == PP_SURFACE_LABEL_POS)
    hipLaunchKernelGGL(k_surface_stats<PP_SURFACE_LABEL_POS>, dim3(nb), dim3(NT), 0, ctx->stream, select, dist, d, vec, tau, device_range,
                       partials, hist);
  else
    hipLaunchKernelGGL(k_surface_stats<PP_SURFACE_NONZERO>, dim3(nb), dim3(NT), 0, ctx->stream, select, dist, d, vec, tau, device_range,
                       partials, hist);
  PP_LAUNCH_CHECK(ctx, "k_surface_stats");
  hipLaunchKernelGGL(k_surface_final, dim3(1), dim3(NT), 0, ctx->stream, (const surf_acc*)partials, (int)nb, device_range, out);
  PP_LAUNCH_CHECK(ctx, "k_surface_final");
  return PP_OK;
}

int pp_slice_masked_count_u8(pp_ctx* ctx, const uint8_t* a, const uint8_t* not_b, const int size[3], int64_t* per_slice) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, a && size && per_slice, "pp_slice_masked_count_u8: NULL argument");
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_slice_masked_count_u8: empty volume");
  PP_REQUIRE(ctx, cmp_aligned(per_slice, 8), "pp_slice_masked_count_u8: per_slice must be 8-byte aligned");
  const size_t slice = (size_t)size[0] * size[1];
  const size_t nz = (size_t)size[2];
  // enough blocks to fill the chip when there are few slices; a block covers at least 4 NT voxels, 4 per lane
  size_t chunks = (2048 + nz - 1) / nz;
  const size_t most = (slice + 4 * (size_t)NT - 1) / (4 * (size_t)NT);
  if (chunks > most) chunks = most;
  const size_t per = ((slice + chunks - 1) / chunks + 3) / 4 * 4;
  chunks = (slice + per - 1) / per;
  PP_REQUIRE(ctx, nz * chunks <= 0x7fffffffu, "pp_slice_masked_count_u8: too many slices");
  const int vec = slice % 4 == 0 && cmp_aligned(a, 4) && (!not_b || cmp_aligned(not_b, 4));
  PP_HIP(ctx, hipMemsetAsync(per_slice, 0, nz * sizeof(int64_t), ctx->stream));
  hipLaunchKernelGGL(k_slice_masked_count, dim3((unsigned)(nz * chunks)), dim3(NT), 0, ctx->stream, a, not_b, slice, (int)chunks, per, vec,
                     reinterpret_cast<unsigned long long*>(per_slice));
  PP_LAUNCH_CHECK(ctx, "k_slice_masked_count");
  return PP_OK;
}

}  // extern "C"
