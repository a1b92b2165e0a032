// platipy_amd/csrc/pp_staple.h -- STAPLE label fusion: sitk.STAPLE (itk::STAPLEImageFilter) as label/fusion.py:223 calls it.
// #included at the end of pp_fusion.hip (it uses that file's NT and grid_for).
//
// The raters' foreground bits of a voxel form one 64-bit key (rater j in bit j), and every quantity of the EM loop is a
// function of the key: W(key) from the rater-ordered products, and the 2R+2 sums of the M step as sums over keys.  Voxels
// that no rater marks (key 0) or every rater marks (key `all`) are counted and enter the sums analytically, so each
// iteration reads only the compacted keys of the mixed voxels -- a few per cent of a real volume:
//   pack     R labels -> keys[n] + per-block counts {all-zero, all-one, mixed, popcount}
//   scan     one block: exclusive scan of the per-block mixed counts + totals
//   compact  the mixed keys, in voxel order (per-block offsets + a wavefront ballot inside each tile)
//   em       per iteration: W(key) from the previous (p, q) -> block partials of the 2R+2 sums -> k_staple_fold, read back
//   write    W(key) per voxel (optionally RescaleIntensity(0, 1) + Threshold), fp64
// Every sum is a fixed tree (block partials, then one block folding them in order): repeated runs are bit-identical, which
// the 1e-14 stopping test needs.  No float atomics.
#pragma once

#include "pp_reduce.h"

namespace {

constexpr int ST_MAX_R = PP_STAPLE_MAX_RATERS;

struct staple_inputs {
  const void* p[ST_MAX_R];
};

// the foreground test of one label value, compared in double: sitk.STAPLE's fg - 1e-10 < v < fg + 1e-10, or
// sitk.BinaryThreshold(lowerThreshold = 0.5)'s 0.5 <= v <= 255 (combine_labels_staple binarises first)
struct staple_test {
  double lo, hi;
  int inclusive;
};
__device__ __forceinline__ bool st_fg(double v, const staple_test& t) {
  return t.inclusive ? (v >= t.lo && v <= t.hi) : (v > t.lo && v < t.hi);
}

// the E step's model: W(key) = g a / (g a + (1 - g) b), a = prod_j (D_j ? p_j : 1 - p_j), b = prod_j (D_j ? 1 - q_j : q_j)
// in rater order; `first` = the initial estimate popcount / R.
struct staple_model {
  double p[ST_MAX_R], q[ST_MAX_R];
  double g;
  int R;
  int first;
};

// (host and device: the host evaluates the two uniform classes with the same operations; the separate statements keep
// the compiler from contracting them into an fma)
__host__ __device__ inline double st_weight(unsigned long long key, const staple_model& m) {
  if (m.first) return (double)__builtin_popcountll(key) / (double)m.R;
  double a = 1.0, b = 1.0;
  for (int j = 0; j < m.R; ++j) {
    const bool d = (key >> j) & 1ull;
    a *= d ? m.p[j] : 1.0 - m.p[j];
    b *= d ? 1.0 - m.q[j] : m.q[j];
  }
  const double ga = m.g * a;
  const double gb = (1.0 - m.g) * b;
  const double den = ga + gb;
  return ga / den;
}

__device__ __forceinline__ void st_load4(const uint8_t* p, double x[4]) {
  const uchar4 u = *reinterpret_cast<const uchar4*>(p);
  x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w;
}
__device__ __forceinline__ void st_load4(const float* p, double x[4]) {
  const float4 f = *reinterpret_cast<const float4*>(p);
  x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
}

// Block b owns voxels [b * chunk, min(n, (b + 1) * chunk)); chunk is a multiple of 4 * NT.  A lane packs 4 consecutive
// voxels (one 4- or 16-byte load per rater when `vec`).  counts[4 b + {0, 1, 2, 3}] = all-zero, all-one, mixed, popcount.
template <typename T>
__global__ void __launch_bounds__(NT) k_staple_pack(staple_inputs in, int R, size_t n, size_t chunk, int vec, staple_test ft,
                                                    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long red[4][NT];
  const size_t begin = (size_t)blockIdx.x * chunk;
  const size_t end = begin + chunk < n ? begin + chunk : n;
  const unsigned long long all = R == 64 ? ~0ull : (1ull << R) - 1ull;
  unsigned long long c0 = 0, c1 = 0, cm = 0, pc = 0;
  for (size_t v = begin + 4 * (size_t)threadIdx.x; v < end; v += 4 * (size_t)NT) {
    const bool full = vec && v + 4 <= end;
    unsigned long long k[4] = {0ull, 0ull, 0ull, 0ull};
    for (int j = 0; j < R; ++j) {
      const T* lab = static_cast<const T*>(in.p[j]);
      double x[4];
      if (full) {
        st_load4(lab + v, x);
      } else {
        for (int e = 0; e < 4; ++e) x[e] = v + e < end ? (double)lab[v + e] : 0.0;
      }
      for (int e = 0; e < 4; ++e)
        if (st_fg(x[e], ft)) k[e] |= 1ull << j;
    }
    for (int e = 0; e < 4; ++e) {
      if (v + e >= end) break;
      keys[v + e] = k[e];
      c0 += k[e] == 0ull;
      c1 += k[e] == all;
      cm += k[e] != 0ull && k[e] != all;
      pc += (unsigned long long)__builtin_popcountll(k[e]);
    }
  }
  const int t = threadIdx.x;
  red[0][t] = c0; red[1][t] = c1; red[2][t] = cm; red[3][t] = pc;
  pp_block_tree<NT>(t, [&](int a, int b) {
    for (int f = 0; f < 4; ++f) red[f][a] += red[f][b];
  });
  if (t < 4) counts[4 * (size_t)blockIdx.x + t] = red[t][0];
}

// One block: offsets[b] = mixed voxels of blocks [0, b); totals = the four counts over all blocks.
__global__ void __launch_bounds__(NT) k_staple_scan(const unsigned long long* __restrict__ counts, int nb,
                                                    unsigned long long* __restrict__ offsets, unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long sc[2][4][NT];
  const int t = threadIdx.x;
  const int per = (nb + NT - 1) / NT;
  const int b0 = t * per, b1 = b0 + per < nb ? b0 + per : nb;
  unsigned long long loc[4] = {0ull, 0ull, 0ull, 0ull};
  for (int b = b0; b < b1; ++b)
    for (int f = 0; f < 4; ++f) loc[f] += counts[4 * (size_t)b + f];
  for (int f = 0; f < 4; ++f) sc[0][f][t] = loc[f];
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < NT; d <<= 1) {   // inclusive Hillis-Steele scan, double-buffered
    for (int f = 0; f < 4; ++f) sc[cur ^ 1][f][t] = sc[cur][f][t] + (t >= d ? sc[cur][f][t - d] : 0ull);
    cur ^= 1;
    __syncthreads();
  }
  unsigned long long off = sc[cur][2][t] - loc[2];
  for (int b = b0; b < b1; ++b) {
    offsets[b] = off;
    off += counts[4 * (size_t)b + 2];
  }
  if (t < 4) totals[t] = sc[cur][t][NT - 1];
}

// The mixed keys of block b's voxels, in voxel order, from offsets[b] on.
__global__ void __launch_bounds__(NT) k_staple_compact(const unsigned long long* __restrict__ keys, size_t n, size_t chunk,
                                                       unsigned long long all, const unsigned long long* __restrict__ offsets,
                                                       unsigned long long* __restrict__ mixed) {
  __shared__ unsigned wcount[NT / 64];
  const size_t begin = (size_t)blockIdx.x * chunk;
  const size_t end = begin + chunk < n ? begin + chunk : n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long base = offsets[blockIdx.x];
  for (size_t t0 = begin; t0 < end; t0 += NT) {
    const size_t i = t0 + threadIdx.x;
    unsigned long long k = 0ull;
    bool m = false;
    if (i < end) {
      k = keys[i];
      m = k != 0ull && k != all;
    }
    const unsigned long long ballot = __ballot(m);
    const unsigned before = (unsigned)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[wave] = (unsigned)__builtin_popcountll(ballot);
    __syncthreads();
    unsigned woff = 0, tile = 0;
    for (int w = 0; w < NT / 64; ++w) {
      if (w < wave) woff += wcount[w];
      tile += wcount[w];
    }
    if (m) mixed[base + woff + before] = k;
    base += tile;
    __syncthreads();
  }
}

// One M step over the mixed keys: block partials of the S = 2R + 2 sums {sum W, sum (1 - W), A_j = sum W D_j,
// B_j = sum (1 - W)(1 - D_j)}.  A tile's (key, W) pairs go to LDS; then thread t owns sum s = t % S for the tile entries
// e = t / S (mod G = NT / S), and the G group partials are folded in group order -- no per-thread arrays of 2R doubles.
__global__ void __launch_bounds__(NT) k_staple_em(const unsigned long long* __restrict__ mixed, size_t m, staple_model md,
                                                  double* __restrict__ partials) {
  __shared__ unsigned long long skey[NT];
  __shared__ double sw[NT];
  __shared__ double red[NT];
  const int R = md.R, S = 2 * R + 2, G = NT / S;
  const int t = threadIdx.x;
  const int s = t % S, grp = t / S;
  const bool active = grp < G;
  // sum s adds (useW ? W : 1 - W) for the keys with (key & sel) == want
  const int j = s < 2 ? 0 : (s < 2 + R ? s - 2 : s - 2 - R);
  const unsigned long long sel = s < 2 ? 0ull : (1ull << j);
  const unsigned long long want = s < 2 + R ? sel : 0ull;
  const bool useW = s == 0 || (s >= 2 && s < 2 + R);
  double acc = 0.0;
  for (size_t base = (size_t)blockIdx.x * NT; base < m; base += (size_t)gridDim.x * NT) {
    const size_t i = base + t;
    const int cnt = m - base < (size_t)NT ? (int)(m - base) : NT;
    if (i < m) {
      const unsigned long long k = mixed[i];
      skey[t] = k;
      sw[t] = st_weight(k, md);
    }
    __syncthreads();
    if (active) {
      for (int e = grp; e < cnt; e += G) {
        const double w = sw[e];
        const double v = useW ? w : 1.0 - w;
        acc += (skey[e] & sel) == want ? v : 0.0;
      }
    }
    __syncthreads();
  }
  red[t] = active ? acc : 0.0;
  __syncthreads();
  if (t < S) {
    double v = 0.0;
    for (int g = 0; g < G; ++g) v += red[g * S + t];
    partials[(size_t)blockIdx.x * S + t] = v;
  }
}

// The EM partials folded, all S sums at once: sum s's blocks are split into C = ST_FOLD_NT / S contiguous runs, thread
// s + S c adds run c in block order, then thread s adds the C run sums in run order (a fixed order: bit-identical reruns).
constexpr int ST_FOLD_NT = 1024;
__global__ void __launch_bounds__(ST_FOLD_NT) k_staple_fold(const double* __restrict__ partials, int nb, int S, double* __restrict__ result) {
  __shared__ double run[ST_FOLD_NT];
  const int t = threadIdx.x, C = ST_FOLD_NT / S, s = t % S, c = t / S;
  double v = 0.0;
  if (c < C) {
    const int per = (nb + C - 1) / C, b0 = c * per, b1 = b0 + per < nb ? b0 + per : nb;
    for (int b = b0; b < b1; ++b) v += partials[(size_t)b * S + s];
  }
  run[t] = v;
  __syncthreads();
  if (t < S) {
    double r = 0.0;
    for (int k = 0; k < C; ++k) r += run[k * S + t];
    result[t] = r;
  }
}

// min / max of W over the mixed keys: partials[2 b] = min, [2 b + 1] = max (+-inf for a block without keys)
__global__ void __launch_bounds__(NT) k_staple_wminmax(const unsigned long long* __restrict__ mixed, size_t m, staple_model md,
                                                       double* __restrict__ partials) {
  double lo = INFINITY, hi = -INFINITY;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < m; i += (size_t)gridDim.x * NT) {
    const double w = st_weight(mixed[i], md);
    lo = fmin(lo, w);
    hi = fmax(hi, w);
  }
  pp_block_range_store<NT>(lo, hi, partials + 2 * (size_t)blockIdx.x);
}

// W per voxel from its key; with `rescale`: RescaleIntensity(0, 1) (x * scale + shift, clamped) then Threshold(lower, 1, 0).
struct st_write {
  staple_model md;
  int rescale;
  double scale, shift, lower;
  __device__ __forceinline__ double f(unsigned long long key) const {
    double w = st_weight(key, md);
    if (rescale) {
      const double xs = w * scale;
      double r = xs + shift;
      r = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
      w = (r < lower || r > 1.0) ? 0.0 : r;
    }
    return w;
  }
};
struct alignas(16) st_u64x2 {
  unsigned long long a, b;
};
struct alignas(16) st_f64x2 {
  double a, b;
};
// two voxels per lane (16-byte accesses) when `vec`, the odd voxel by block 0
__global__ void __launch_bounds__(NT) k_staple_write(const unsigned long long* __restrict__ keys, size_t n, int vec, st_write op,
                                                     double* __restrict__ out) {
  const size_t n2 = vec ? n / 2 : 0;
  for (size_t g = (size_t)blockIdx.x * NT + threadIdx.x; g < n2; g += (size_t)gridDim.x * NT) {
    const st_u64x2 k = reinterpret_cast<const st_u64x2*>(keys)[g];
    reinterpret_cast<st_f64x2*>(out)[g] = st_f64x2{op.f(k.a), op.f(k.b)};
  }
  for (size_t i = n2 * 2 + (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) out[i] = op.f(keys[i]);
}

bool st_same_bits(const double* a, const double* b, int n) { return memcmp(a, b, (size_t)n * sizeof(double)) == 0; }

}  // namespace

extern "C" int pp_staple_fuse(pp_ctx* ctx, const void* const* labels, int dtype, int nraters, size_t n,
                              const pp_staple_params* prm, double* w, pp_staple_result* res) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, labels && prm && w && res, "pp_staple_fuse: NULL argument");
  PP_REQUIRE(ctx, nraters >= 1 && nraters <= ST_MAX_R, "pp_staple_fuse: nraters must be 1..PP_STAPLE_MAX_RATERS");
  PP_REQUIRE(ctx, n > 0, "pp_staple_fuse: empty volume");
  PP_REQUIRE(ctx, dtype == PP_DTYPE_U8 || dtype == PP_DTYPE_F32, "pp_staple_fuse: dtype must be PP_DTYPE_U8 or PP_DTYPE_F32");
  PP_REQUIRE(ctx, prm->foreground_test == PP_STAPLE_FOREGROUND || prm->foreground_test == PP_STAPLE_BINARY_THRESHOLD,
             "pp_staple_fuse: unknown foreground_test");
  const int R = nraters;
  staple_inputs in{};
  const uintptr_t align = dtype == PP_DTYPE_U8 ? 4 : 16;
  int vec = 1;
  for (int j = 0; j < R; ++j) {
    PP_REQUIRE(ctx, labels[j], "pp_staple_fuse: NULL label");
    in.p[j] = labels[j];
    if (reinterpret_cast<uintptr_t>(labels[j]) % align) vec = 0;
  }
  staple_test ft;
  if (prm->foreground_test == PP_STAPLE_FOREGROUND) {
    ft.lo = prm->foreground_value - 1e-10;
    ft.hi = prm->foreground_value + 1e-10;
    ft.inclusive = 0;
  } else {
    ft.lo = 0.5;
    ft.hi = 255.0;
    ft.inclusive = 1;
  }
  const unsigned long long all = R == 64 ? ~0ull : (1ull << R) - 1ull;
  const int S = 2 * R + 2;

  // grid of the pack / compact passes: chunks of whole 4 * NT tiles
  const size_t tile = 4 * (size_t)NT;
  size_t nbp = (n + tile - 1) / tile;
  if (nbp > 2048) nbp = 2048;
  const size_t chunk = ((n + nbp - 1) / nbp + tile - 1) / tile * tile;
  nbp = (n + chunk - 1) / chunk;
  const unsigned nbe = grid_for(n, 1024u);   // EM / min-max grid: an upper bound (the mixed count is not known yet)

  const size_t bytes = 2 * pp_align_up(n * sizeof(unsigned long long), 256) + pp_align_up(nbp * 4 * 8, 256) +
                       pp_align_up(nbp * 8, 256) + 256 + pp_align_up(((size_t)nbe * S + S) * 8, 256) +
                       pp_align_up((2 * (size_t)nbe + 2) * 8, 256);
  int rc = pp_reserve(ctx, bytes);
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  unsigned long long* keys = cv.take<unsigned long long>(n);
  unsigned long long* mixed = cv.take<unsigned long long>(n);
  unsigned long long* counts = cv.take<unsigned long long>(nbp * 4);
  unsigned long long* offsets = cv.take<unsigned long long>(nbp);
  unsigned long long* totals = cv.take<unsigned long long>(4);
  double* em_part = cv.take<double>((size_t)nbe * S + S);
  double* mm_part = cv.take<double>(2 * (size_t)nbe + 2);

  {
    pp_prof_scope ps(ctx, "k_staple_pack");
    if (dtype == PP_DTYPE_U8)
      hipLaunchKernelGGL(k_staple_pack<uint8_t>, dim3((unsigned)nbp), dim3(NT), 0, ctx->stream, in, R, n, chunk, vec, ft, keys, counts);
    else
      hipLaunchKernelGGL(k_staple_pack<float>, dim3((unsigned)nbp), dim3(NT), 0, ctx->stream, in, R, n, chunk, vec, ft, keys, counts);
    PP_LAUNCH_CHECK(ctx, "k_staple_pack");
  }
  {
    pp_prof_scope ps(ctx, "k_staple_scan+compact");
    hipLaunchKernelGGL(k_staple_scan, dim3(1), dim3(NT), 0, ctx->stream, (const unsigned long long*)counts, (int)nbp, offsets, totals);
    PP_LAUNCH_CHECK(ctx, "k_staple_scan");
    hipLaunchKernelGGL(k_staple_compact, dim3((unsigned)nbp), dim3(NT), 0, ctx->stream, (const unsigned long long*)keys, n, chunk, all,
                       (const unsigned long long*)offsets, mixed);
    PP_LAUNCH_CHECK(ctx, "k_staple_compact");
  }
  unsigned long long tot[4];
  rc = pp_read_back(ctx, totals, tot, sizeof(tot));
  if (rc) return rc;
  const unsigned long long n0 = tot[0], n1 = tot[1], nm = tot[2], pcsum = tot[3];
  PP_REQUIRE(ctx, n0 + n1 + nm == n, "pp_staple_fuse: voxel classes do not add up (internal error)");
  const unsigned nbm = grid_for(nm, 1024u);   // (4 blocks per CU; also bounds the serial runs of k_staple_fold)

  staple_model md{};
  md.R = R;
  md.first = 1;
  // W_initial = popcount / R;  g = (sum_i W_i / N) * confidence_weight with sum_i W_i = (exact sum of popcounts) / R
  md.g = ((double)pcsum / (double)R) / (double)n * prm->confidence_weight;

  double p[ST_MAX_R], q[ST_MAX_R], last_p[ST_MAX_R], last_q[ST_MAX_R], prev2_p[ST_MAX_R], prev2_q[ST_MAX_R];
  for (int k = 0; k < R; ++k) last_p[k] = last_q[k] = -10.0;
  for (int k = 0; k < R; ++k) p[k] = q[k] = NAN;
  int degenerate = 0;
  unsigned long long it = 0;
  double sums[2 * ST_MAX_R + 2];
  while (it < prm->maximum_iterations) {
    if (nm > 0) {
      pp_prof_scope ps(ctx, "k_staple_em");
      hipLaunchKernelGGL(k_staple_em, dim3(nbm), dim3(NT), 0, ctx->stream, (const unsigned long long*)mixed, (size_t)nm, md, em_part);
      PP_LAUNCH_CHECK(ctx, "k_staple_em");
      hipLaunchKernelGGL(k_staple_fold, dim3(1), dim3(ST_FOLD_NT), 0, ctx->stream, (const double*)em_part, (int)nbm, S, em_part + (size_t)nbm * S);
      PP_LAUNCH_CHECK(ctx, "k_staple_fold");
      rc = pp_read_back(ctx, em_part + (size_t)nbm * S, sums, (size_t)S * sizeof(double));
      if (rc) return rc;
    } else {
      for (int s = 0; s < S; ++s) sums[s] = 0.0;
    }
    // the uniform classes: key 0 adds W0 / 1 - W0 / nothing / 1 - W0, key `all` adds W1 / 1 - W1 / W1 / nothing
    const double w0 = st_weight(0ull, md), w1 = st_weight(all, md);
    const double c0 = (double)n0, c1 = (double)n1;
    const double t0 = c0 * w0, t1 = c1 * w1, u0 = c0 * (1.0 - w0), u1 = c1 * (1.0 - w1);
    const double sw = sums[0] + t0 + t1;
    const double sw1 = sums[1] + u0 + u1;
    if (it == 0 && (sw == 0.0 || sw1 == 0.0)) {   // no rater marks anything, or every rater marks everything
      degenerate = 1;
      break;
    }
    for (int k = 0; k < R; ++k) {
      p[k] = (sums[2 + k] + t1) / sw;
      q[k] = (sums[2 + R + k] + u0) / sw1;
    }
    bool converged = true;
    for (int k = 0; k < R; ++k)
      if (!(fabs(last_p[k] - p[k]) < 1e-14 && fabs(last_q[k] - q[k]) < 1e-14)) converged = false;
    const bool cycle = it >= 2 && st_same_bits(p, prev2_p, R) && st_same_bits(q, prev2_q, R);
    md.first = 0;   // E step: the next W comes from this (p, q)
    for (int k = 0; k < R; ++k) {
      md.p[k] = p[k];
      md.q[k] = q[k];
    }
    if (converged || cycle) break;
    memcpy(prev2_p, last_p, sizeof(double) * R);
    memcpy(prev2_q, last_q, sizeof(double) * R);
    memcpy(last_p, p, sizeof(double) * R);
    memcpy(last_q, q, sizeof(double) * R);
    ++it;
  }
  if (degenerate) {
    md.first = 1;
    for (int k = 0; k < R; ++k) p[k] = q[k] = NAN;
  }

  double scale = 1.0, shift = 0.0;
  if (prm->rescale) {
    // RescaleIntensity(W, 0, 1): min / max over the classes that occur
    double lo = INFINITY, hi = -INFINITY;
    if (nm > 0) {
      hipLaunchKernelGGL(k_staple_wminmax, dim3(nbm), dim3(NT), 0, ctx->stream, (const unsigned long long*)mixed, (size_t)nm, md, mm_part);
      PP_LAUNCH_CHECK(ctx, "k_staple_wminmax");
      hipLaunchKernelGGL((k_range_fold<NT, double>), dim3(1), dim3(NT), 0, ctx->stream, (const double*)mm_part, (int)nbm, mm_part + 2 * (size_t)nbm);
      PP_LAUNCH_CHECK(ctx, "k_range_fold");
      double mm[2];
      rc = pp_read_back(ctx, mm_part + 2 * (size_t)nbm, mm, sizeof(mm));
      if (rc) return rc;
      lo = mm[0];
      hi = mm[1];
    }
    if (n0 > 0) {
      const double w0 = st_weight(0ull, md);
      lo = fmin(lo, w0);
      hi = fmax(hi, w0);
    }
    if (n1 > 0) {
      const double w1 = st_weight(all, md);
      lo = fmin(lo, w1);
      hi = fmax(hi, w1);
    }
    // itk::RescaleIntensityImageFilter::BeforeThreadedGenerateData, output range [0, 1]
    if (lo != hi) scale = 1.0 / (hi - lo);
    else if (hi != 0.0) scale = 1.0 / hi;
    else scale = 0.0;
    shift = 0.0 - lo * scale;
  }
  {
    pp_prof_scope ps(ctx, "k_staple_write");
    const int vec = reinterpret_cast<uintptr_t>(w) % 16 == 0;
    const st_write op{md, prm->rescale, scale, shift, prm->threshold_lower};
    hipLaunchKernelGGL(k_staple_write, dim3(grid_for(vec ? (n + 1) / 2 : n, 2048u)), dim3(NT), 0, ctx->stream, (const unsigned long long*)keys,
                       n, vec, op, w);
    PP_LAUNCH_CHECK(ctx, "k_staple_write");
  }

  memset(res, 0, sizeof(*res));
  for (int k = 0; k < R; ++k) {
    res->sensitivity[k] = p[k];
    res->specificity[k] = q[k];
  }
  res->elapsed_iterations = degenerate ? 0 : it;
  res->n_zero = (int64_t)n0;
  res->n_one = (int64_t)n1;
  res->n_mixed = (int64_t)nm;
  res->degenerate = degenerate;
  return PP_OK;
}
