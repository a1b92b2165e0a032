// platipy_amd/csrc/pp_dose.h -- the numpy pieces of platipy/imaging/dose/: the per-structure np.histogram of dvh.py and the
// mean / max / np.percentile / threshold counts of metric.py, for every structure in one pass over the volume.  #included at
// the end of pp_fusion.hip (it uses that file's NT and grid_for).
//
// Histogram and statistics.  A thread takes 16 consecutive voxels: one 16-byte load per mask, all of them OR-ed.  Most
// voxels belong to no structure, and a strip whose mask bytes are all zero ends there: its dose is never requested, no edge
// is looked up and no atomic issued.  In a strip that holds a structure the thread visits the marked voxels one by one (the
// dose value and the mask bytes come from the cache lines the strip just touched): bin = the one np.histogram picks --
// an arithmetic guess corrected against the fp64 edge table, the fp32 dose compared as a double, the top edge closed,
// values outside the edges dropped -- counted in a per-workgroup LDS table, one table per label of the launch.  Labels are
// processed DH_GROUP at a time, fewer when their tables do not fit DH_LDS_WORDS counters (one launch per group); when a
// single label's bins do not fit, the counts go to global memory with 64-bit integer atomics.
//
// Every atomic is an integer atomic, so a rerun gives the same bits -- including the dose SUM: an fp32 value is
// m * 2^(s - 149) with a 24-bit integer m and 0 <= s <= 253, and the kernel adds m << (s % 32) into two of nine 64-bit
// limbs (limb j weighs 2^(32 j - 149)).  The limbs hold the exact sum of every finite fp32 dose of the structure; the host
// rounds it to fp64 once.  Minimum and maximum travel as the order-preserving signed-integer image of the fp32 bits.
//
// Order statistics.  The k-th smallest dose of one structure by radix select on the order-preserving 32-bit key: three
// counting passes over 11 + 11 + 10 bits with LDS counters, up to eight ranks side by side (a pass counts, for each distinct
// prefix the ranks have reached, the next digit of the voxels that carry that prefix).  Nothing is sorted or compacted.
#pragma once

#include <algorithm>
#include <climits>

namespace {

constexpr int DH_GROUP = 16;          // labels of one launch
constexpr int DH_LDS_WORDS = 12288;   // 32-bit bin counters of one workgroup: 48 KB
constexpr int DH_MAX_LABELS = 64;
constexpr int DH_MAX_BINS = 1 << 20;
constexpr int DH_LIMBS = 9;           // 9 x 32 bits span 2^-149 ... 2^139 > FLT_MAX * 2^24
constexpr int DH_STAT = 4 + DH_LIMBS;   // 64-bit slots: count, sum of mask values, +inf, -inf, limbs

struct dh_rec {   // one label's statistics in device memory
  unsigned long long s[DH_STAT];
  int min_key, max_key;
};

struct dh_args {
  const uint8_t* lab[DH_GROUP];
  int nl;          // labels of this launch
  int nbins;
  int use_lds;     // nl * nbins <= DH_LDS_WORDS
  int vec;         // every mask is 16-byte aligned
  double e0, scale;   // the arithmetic guess: bin ~ (v - e0) * scale
};

// fp32 bits <-> a signed integer with the same order (-0.0 sorts below +0.0)
__host__ __device__ __forceinline__ int dh_key(float v) {
  const unsigned b = __builtin_bit_cast(unsigned, v);
  return (int)(b & 0x80000000u ? b ^ 0x7fffffffu : b);
}
inline float dh_unkey(int k) {
  const unsigned b = (unsigned)k;
  return __builtin_bit_cast(float, b & 0x80000000u ? b ^ 0x7fffffffu : b);
}

// np.histogram(v, bins=e): the largest k with e[k] <= v, the last bin closed on the right; -1 outside [e[0], e[nbins]]
__device__ __forceinline__ int dh_bin(double v, const double* __restrict__ e, int nbins, double e0, double scale) {
  if (!(v >= e[0]) || !(v <= e[nbins])) return -1;
  const double g = (v - e0) * scale;
  int k = g >= (double)(nbins - 1) ? nbins - 1 : (g > 0.0 ? (int)g : 0);   // (a NaN guess, from infinite edges, gives 0)
  if (v >= e[k]) {
    if (k == nbins - 1 || v < e[k + 1]) return k;
    if (k + 2 > nbins - 1 || v < e[k + 2]) return k + 1;
  } else if (k > 0 && v >= e[k - 1]) {
    return k - 1;
  }
  // the guess is off by more than one (edges that are not evenly spaced): bisect, e[lo] <= v and (hi == nbins or v < e[hi])
  int lo = 0, hi = nbins;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (v >= e[mid]) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One voxel that may belong to structures of this launch.
__device__ __forceinline__ void dh_voxel(const float* __restrict__ dose, const dh_args& a, size_t i, const double* __restrict__ edges,
                                         unsigned* sh_hist, unsigned long long (*sh_stat)[DH_STAT], int (*sh_mm)[2],
                                         unsigned long long* __restrict__ hist, unsigned& bad) {
  float v = 0.0f;
  int k = -2, sk = 0;   // -2: dose not looked at yet
  for (int g = 0; g < a.nl; ++g) {
    const unsigned m = a.lab[g][i];
    if (!m) continue;
    if (k == -2) {
      v = dose[i];
      if (!(v == v)) {
        ++bad;
        return;
      }
      k = dh_bin((double)v, edges, a.nbins, a.e0, a.scale);
      sk = dh_key(v);
    }
    if (k >= 0) {
      if (a.use_lds) atomicAdd(&sh_hist[g * a.nbins + k], 1u);
      else atomicAdd(&hist[(size_t)g * a.nbins + k], 1ull);
    }
    atomicAdd(&sh_stat[g][0], 1ull);
    atomicAdd(&sh_stat[g][1], (unsigned long long)m);
    if (sk < sh_mm[g][0]) atomicMin(&sh_mm[g][0], sk);
    if (sk > sh_mm[g][1]) atomicMax(&sh_mm[g][1], sk);
    const unsigned bits = __builtin_bit_cast(unsigned, v);
    const unsigned eb = (bits >> 23) & 0xffu;
    const bool neg = (bits >> 31) != 0u;
    if (eb == 0xffu) {
      atomicAdd(&sh_stat[g][neg ? 3 : 2], 1ull);
    } else {
      const unsigned long long man = (bits & 0x7fffffu) | (eb ? 0x800000u : 0u);
      const unsigned s = eb ? eb - 1u : 0u;             // v = man * 2^(s - 149)
      const unsigned long long wide = man << (s & 31u);
      const unsigned long long lo = wide & 0xffffffffull, hi = wide >> 32;
      if (lo) atomicAdd(&sh_stat[g][4 + (s >> 5)], neg ? 0ull - lo : lo);   // (two's complement: a signed 64-bit sum)
      if (hi) atomicAdd(&sh_stat[g][5 + (s >> 5)], neg ? 0ull - hi : hi);
    }
  }
}

// hist[g][k] += voxels of label g in bin k; rec[g] += the label's statistics; *nan_count += voxels of any label whose dose is
// NaN.  n < 2^31.
__global__ void __launch_bounds__(NT) k_dose_hist(const float* __restrict__ dose, dh_args a, size_t n, const double* __restrict__ edges,
                                                  unsigned long long* __restrict__ hist, dh_rec* __restrict__ rec,
                                                  unsigned long long* __restrict__ nan_count) {
  __shared__ unsigned sh_hist[DH_LDS_WORDS];
  __shared__ unsigned long long sh_stat[DH_GROUP][DH_STAT];
  __shared__ int sh_mm[DH_GROUP][2];
  const int t = threadIdx.x;
  const int words = a.use_lds ? a.nl * a.nbins : 0;
  for (int i = t; i < words; i += NT) sh_hist[i] = 0u;
  for (int i = t; i < DH_GROUP * DH_STAT; i += NT) sh_stat[i / DH_STAT][i % DH_STAT] = 0ull;
  if (t < DH_GROUP) {
    sh_mm[t][0] = INT_MAX;
    sh_mm[t][1] = INT_MIN;
  }
  __syncthreads();
  unsigned bad = 0;
  const size_t n16 = a.vec ? n / 16 : 0;
  for (size_t c = (size_t)blockIdx.x * NT + t; c < n16; c += (size_t)gridDim.x * NT) {
    unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
    for (int g = 0; g < DH_GROUP; ++g)
      if (g < a.nl) {
        const int4 m = reinterpret_cast<const int4*>(a.lab[g])[c];
        lo |= (unsigned long long)(unsigned)m.x | ((unsigned long long)(unsigned)m.y << 32);
        hi |= (unsigned long long)(unsigned)m.z | ((unsigned long long)(unsigned)m.w << 32);
      }
    if (!(lo | hi)) continue;
    for (int j = 0; j < 16; ++j)
      if ((((j < 8 ? lo : hi) >> (8 * (j & 7))) & 0xffull) != 0ull) dh_voxel(dose, a, c * 16 + j, edges, sh_hist, sh_stat, sh_mm, hist, bad);
  }
  // the n % 16 tail, or everything when a mask is not 16-byte aligned
  for (size_t i = n16 * 16 + (size_t)blockIdx.x * NT + t; i < n; i += (size_t)gridDim.x * NT)
    dh_voxel(dose, a, i, edges, sh_hist, sh_stat, sh_mm, hist, bad);
  if (bad) atomicAdd(nan_count, (unsigned long long)bad);
  __syncthreads();
  for (int i = t; i < words; i += NT)
    if (sh_hist[i]) atomicAdd(&hist[i], (unsigned long long)sh_hist[i]);
  for (int i = t; i < a.nl * DH_STAT; i += NT) {
    const unsigned long long s = sh_stat[i / DH_STAT][i % DH_STAT];
    if (s) atomicAdd(&rec[i / DH_STAT].s[i % DH_STAT], s);
  }
  if (t < a.nl && sh_mm[t][0] <= sh_mm[t][1]) {
    atomicMin(&rec[t].min_key, sh_mm[t][0]);
    atomicMax(&rec[t].max_key, sh_mm[t][1]);
  }
}

// The exact value of sum_j (int64) limb[j] * 2^(32 j - 149), rounded to fp64: each limb is split into two halves that a
// double holds exactly, and the 18 terms are added without error (Shewchuk's growing expansion) before one final sum.
double dh_limbs_to_double(const unsigned long long* limb) {
  double part[2 * DH_LIMBS + 2];
  int np = 0;
  for (int j = 0; j < DH_LIMBS; ++j) {
    const long long sv = (long long)limb[j];
    const long long hi = sv >> 32, lo = sv - hi * 4294967296ll;   // sv = hi * 2^32 + lo, 0 <= lo < 2^32
    const double term[2] = {ldexp((double)hi, 32 * j + 32 - 149), ldexp((double)lo, 32 * j - 149)};
    for (int q = 0; q < 2; ++q) {
      volatile double x = term[q];
      int kept = 0;
      for (int p = 0; p < np; ++p) {
        volatile double y = part[p];
        if (fabs(x) < fabs(y)) {
          const double tmp = x;
          x = y;
          y = tmp;
        }
        volatile double sum = x + y;
        volatile double back = sum - x;
        const double err = y - back;
        if (err != 0.0) part[kept++] = err;
        x = sum;
      }
      part[kept++] = x;
      np = kept;
    }
  }
  double total = 0.0;
  for (int p = np - 1; p >= 0; --p) total += part[p];   // the partials do not overlap: largest first
  return total;
}

// The histogram and the statistics of every label; hist on the HOST.  edges: nbins + 1 host doubles, checked by the caller.
int dh_run(pp_ctx* ctx, const char* who, const float* dose, const uint8_t* const* labels, int nlabels, size_t n, const double* edges,
           int nbins, int64_t* hist, pp_dose_stats* stats) {
  const size_t cells = (size_t)nlabels * nbins;
  const size_t hist_bytes = pp_align_up((cells + 1) * sizeof(unsigned long long), 256);   // (+ the NaN counter)
  const size_t rec_bytes = pp_align_up((size_t)nlabels * sizeof(dh_rec), 256);
  int rc = pp_reserve(ctx, hist_bytes + rec_bytes + pp_align_up(((size_t)nbins + 1) * sizeof(double), 256));
  if (rc) return rc;
  unsigned long long* dh = reinterpret_cast<unsigned long long*>(ctx->ws);
  dh_rec* dr = reinterpret_cast<dh_rec*>(ctx->ws + hist_bytes);
  double* de = reinterpret_cast<double*>(ctx->ws + hist_bytes + rec_bytes);
  std::vector<dh_rec> recs((size_t)nlabels);
  for (auto& r : recs) {
    memset(&r, 0, sizeof(r));
    r.min_key = INT_MAX;
    r.max_key = INT_MIN;
  }
  PP_HIP(ctx, hipMemsetAsync(dh, 0, (cells + 1) * sizeof(unsigned long long), ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(dr, recs.data(), recs.size() * sizeof(dh_rec), hipMemcpyHostToDevice, ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(de, edges, ((size_t)nbins + 1) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const double width = edges[nbins] - edges[0];
  int per = DH_LDS_WORDS / nbins;
  const int use_lds = per >= 1;
  if (per > DH_GROUP || !use_lds) per = DH_GROUP;
  for (int g0 = 0; g0 < nlabels; g0 += per) {
    dh_args a;
    a.nl = nlabels - g0 < per ? nlabels - g0 : per;
    a.nbins = nbins;
    a.use_lds = use_lds;
    a.vec = 1;
    for (int g = 0; g < DH_GROUP; ++g) {
      a.lab[g] = g < a.nl ? labels[g0 + g] : nullptr;
      if (reinterpret_cast<uintptr_t>(a.lab[g]) % 16) a.vec = 0;
    }
    a.e0 = edges[0];
    a.scale = width > 0.0 && width <= DBL_MAX ? (double)nbins / width : 0.0;
    hipLaunchKernelGGL(k_dose_hist, dim3(grid_for(a.vec ? (n + 15) / 16 : n, 1024u)), dim3(NT), 0, ctx->stream, dose, a, n,
                       (const double*)de, dh + (size_t)g0 * nbins, dr + g0, dh + cells);
    PP_LAUNCH_CHECK(ctx, "k_dose_hist");
  }
  unsigned long long bad = 0;
  PP_HIP(ctx, hipMemcpyAsync(hist, dh, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(&bad, dh + cells, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(recs.data(), dr, recs.size() * sizeof(dh_rec), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (bad) return pp_fail(ctx, PP_ERR_ARG, "%s: %llu voxels inside a mask hold a NaN dose", who, bad);
  if (stats)
    for (int l = 0; l < nlabels; ++l) {
      const dh_rec& r = recs[(size_t)l];
      pp_dose_stats& s = stats[l];
      s.count = (int64_t)r.s[0];
      s.mask_sum = (int64_t)r.s[1];
      if (r.s[2] && r.s[3]) s.dose_sum = (double)NAN;
      else if (r.s[2] || r.s[3]) s.dose_sum = r.s[2] ? (double)INFINITY : -(double)INFINITY;
      else s.dose_sum = dh_limbs_to_double(r.s + 4);
      s.dose_min = r.s[0] ? dh_unkey(r.min_key) : INFINITY;
      s.dose_max = r.s[0] ? dh_unkey(r.max_key) : -INFINITY;
    }
  return PP_OK;
}

int dh_check_labels(pp_ctx* ctx, const char* who, const uint8_t* const* labels, int nlabels, size_t n) {
  if (nlabels < 1 || nlabels > DH_MAX_LABELS) return pp_fail(ctx, PP_ERR_SIZE, "%s: %d labels (1 ... %d)", who, nlabels, DH_MAX_LABELS);
  if (n >= 0x7fffffffu) return pp_fail(ctx, PP_ERR_SIZE, "%s: volume of 2^31 voxels or more", who);
  for (int l = 0; l < nlabels; ++l)
    if (!labels[l]) return pp_fail(ctx, PP_ERR_ARG, "%s: NULL label", who);
  return PP_OK;
}

// ---------------------------------------------------------------------------------------
// order statistics

constexpr int OS_RANKS = 8;
constexpr int OS_DIGIT = 2048;   // counters per prefix: 11 bits (the last pass uses 1024 of them)

struct os_args {
  unsigned prefix[OS_RANKS];   // distinct
  int np;
  int match_shift;   // a voxel belongs to prefix p when key >> match_shift == prefix[p]; 32: every voxel, np = 1
  int bin_shift;
  unsigned bin_mask;
  int vec;
};

__device__ __forceinline__ void os_voxel(const float* __restrict__ dose, size_t i, const os_args& a, unsigned* sh, unsigned& bad) {
  const float v = dose[i];
  if (!(v == v)) {
    ++bad;
    return;
  }
  const unsigned key = (unsigned)dh_key(v) ^ 0x80000000u;   // unsigned order
  const unsigned digit = (key >> a.bin_shift) & a.bin_mask;
  if (a.match_shift >= 32) {
    atomicAdd(&sh[digit], 1u);
    return;
  }
  const unsigned pre = key >> a.match_shift;
  for (int p = 0; p < a.np; ++p)
    if (pre == a.prefix[p]) {
      atomicAdd(&sh[p * OS_DIGIT + digit], 1u);
      return;
    }
}

// table[p][digit] += voxels of the mask whose key carries prefix p; *nan_count += NaN voxels of the mask.  n < 2^31.
__global__ void __launch_bounds__(NT) k_masked_radix_count(const float* __restrict__ dose, const uint8_t* __restrict__ label, size_t n,
                                                           os_args a, unsigned long long* __restrict__ table,
                                                           unsigned long long* __restrict__ nan_count) {
  __shared__ unsigned sh[OS_RANKS * OS_DIGIT];
  const int t = threadIdx.x;
  for (int i = t; i < a.np * OS_DIGIT; i += NT) sh[i] = 0u;
  __syncthreads();
  unsigned bad = 0;
  const size_t n16 = a.vec ? n / 16 : 0;
  for (size_t c = (size_t)blockIdx.x * NT + t; c < n16; c += (size_t)gridDim.x * NT) {
    const int4 m = reinterpret_cast<const int4*>(label)[c];
    const unsigned long long lo = (unsigned long long)(unsigned)m.x | ((unsigned long long)(unsigned)m.y << 32);
    const unsigned long long hi = (unsigned long long)(unsigned)m.z | ((unsigned long long)(unsigned)m.w << 32);
    if (!(lo | hi)) continue;
    for (int j = 0; j < 16; ++j)
      if ((((j < 8 ? lo : hi) >> (8 * (j & 7))) & 0xffull) != 0ull) os_voxel(dose, c * 16 + j, a, sh, bad);
  }
  for (size_t i = n16 * 16 + (size_t)blockIdx.x * NT + t; i < n; i += (size_t)gridDim.x * NT)
    if (label[i]) os_voxel(dose, i, a, sh, bad);
  if (bad) atomicAdd(nan_count, (unsigned long long)bad);
  __syncthreads();
  for (int i = t; i < a.np * OS_DIGIT; i += NT)
    if (sh[i]) atomicAdd(&table[i], (unsigned long long)sh[i]);
}

}  // namespace

extern "C" {

int pp_dose_histogram_f32(pp_ctx* ctx, const float* dose, const uint8_t* const* labels, int nlabels, size_t n, const double* edges,
                          int nbins, int64_t* hist, pp_dose_stats* stats) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, dose && labels && edges && hist && n > 0, "pp_dose_histogram_f32: NULL or empty argument");
  if (nbins < 1 || nbins > DH_MAX_BINS) return pp_fail(ctx, PP_ERR_SIZE, "pp_dose_histogram_f32: %d bins (1 ... 2^20)", nbins);
  int rc = dh_check_labels(ctx, "pp_dose_histogram_f32", labels, nlabels, n);
  if (rc) return rc;
  for (int k = 0; k <= nbins; ++k) {
    PP_REQUIRE(ctx, edges[k] == edges[k], "pp_dose_histogram_f32: an edge is NaN");
    PP_REQUIRE(ctx, k == 0 || edges[k] >= edges[k - 1], "pp_dose_histogram_f32: the edges must not decrease");
  }
  return dh_run(ctx, "pp_dose_histogram_f32", dose, labels, nlabels, n, edges, nbins, hist, stats);
}

int pp_masked_count_ge_f32(pp_ctx* ctx, const float* dose, const uint8_t* const* labels, int nlabels, size_t n, const float* thresholds,
                           int nthresholds, int64_t* counts) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, dose && labels && thresholds && counts && n > 0, "pp_masked_count_ge_f32: NULL or empty argument");
  if (nthresholds < 1 || nthresholds > DH_MAX_BINS)
    return pp_fail(ctx, PP_ERR_SIZE, "pp_masked_count_ge_f32: %d thresholds (1 ... 2^20)", nthresholds);
  int rc = dh_check_labels(ctx, "pp_masked_count_ge_f32", labels, nlabels, n);
  if (rc) return rc;
  // the distinct thresholds, ascending, are the edges of a histogram whose top bin is open: v >= t <=> bin(v) >= index of t
  std::vector<double> edges;
  for (int j = 0; j < nthresholds; ++j) {
    PP_REQUIRE(ctx, thresholds[j] == thresholds[j], "pp_masked_count_ge_f32: a threshold is NaN");
    edges.push_back((double)thresholds[j]);
  }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  const int nb = (int)edges.size();
  edges.push_back((double)INFINITY);
  std::vector<int64_t> hist((size_t)nlabels * nb);
  rc = dh_run(ctx, "pp_masked_count_ge_f32", dose, labels, nlabels, n, edges.data(), nb, hist.data(), nullptr);
  if (rc) return rc;
  for (int l = 0; l < nlabels; ++l) {
    int64_t* h = hist.data() + (size_t)l * nb;
    for (int k = nb - 2; k >= 0; --k) h[k] += h[k + 1];   // h[k] = voxels at or above edge k
    for (int j = 0; j < nthresholds; ++j) {
      const int k = (int)(std::lower_bound(edges.begin(), edges.begin() + nb, (double)thresholds[j]) - edges.begin());
      counts[(size_t)l * nthresholds + j] = h[k];
    }
  }
  return PP_OK;
}

int pp_masked_order_stats_f32(pp_ctx* ctx, const float* dose, const uint8_t* label, size_t n, const int64_t* ranks, int nranks,
                              float* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, dose && label && ranks && out && n > 0, "pp_masked_order_stats_f32: NULL or empty argument");
  PP_REQUIRE(ctx, nranks >= 1 && nranks <= OS_RANKS, "pp_masked_order_stats_f32: 1 ... 8 ranks per call");
  if (n >= 0x7fffffffu) return pp_fail(ctx, PP_ERR_SIZE, "pp_masked_order_stats_f32: volume of 2^31 voxels or more");
  const size_t cells = (size_t)OS_RANKS * OS_DIGIT;
  int rc = pp_reserve(ctx, pp_align_up((cells + 1) * sizeof(unsigned long long), 256));
  if (rc) return rc;
  unsigned long long* dt = reinterpret_cast<unsigned long long*>(ctx->ws);
  std::vector<unsigned long long> table(cells + 1);
  unsigned prefix[OS_RANKS];            // per rank: the key bits found so far
  int64_t left[OS_RANKS];               // per rank: its rank among the voxels that carry its prefix
  for (int j = 0; j < nranks; ++j) prefix[j] = 0u, left[j] = ranks[j];
  const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
  for (int pass = 0; pass < 3; ++pass) {
    os_args a;
    a.np = 0;
    int slot[OS_RANKS];
    if (pass == 0) {
      a.np = 1;
      a.prefix[0] = 0u;
      for (int j = 0; j < nranks; ++j) slot[j] = 0;
    } else {
      for (int j = 0; j < nranks; ++j) {
        int p = 0;
        while (p < a.np && a.prefix[p] != prefix[j]) ++p;
        if (p == a.np) a.prefix[a.np++] = prefix[j];
        slot[j] = p;
      }
    }
    a.match_shift = pass == 0 ? 32 : shifts[pass - 1];
    a.bin_shift = shifts[pass];
    a.bin_mask = (1u << widths[pass]) - 1u;
    a.vec = reinterpret_cast<uintptr_t>(label) % 16 == 0;
    PP_HIP(ctx, hipMemsetAsync(dt, 0, (cells + 1) * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_masked_radix_count, dim3(grid_for(a.vec ? (n + 15) / 16 : n, 1024u)), dim3(NT), 0, ctx->stream, dose, label, n, a,
                       dt, dt + cells);
    PP_LAUNCH_CHECK(ctx, "k_masked_radix_count");
    PP_HIP(ctx, hipMemcpyAsync(table.data(), dt, (cells + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (pass == 0) {
      if (table[cells]) return pp_fail(ctx, PP_ERR_ARG, "pp_masked_order_stats_f32: %llu voxels inside the mask hold a NaN dose", table[cells]);
      unsigned long long count = 0;
      for (int d = 0; d < OS_DIGIT; ++d) count += table[(size_t)d];
      PP_REQUIRE(ctx, count > 0, "pp_masked_order_stats_f32: the mask is empty");
      for (int j = 0; j < nranks; ++j)
        if (ranks[j] < 0 || (unsigned long long)ranks[j] >= count)
          return pp_fail(ctx, PP_ERR_ARG, "pp_masked_order_stats_f32: rank %lld of a mask of %llu voxels", (long long)ranks[j], count);
    }
    for (int j = 0; j < nranks; ++j) {
      const unsigned long long* row = table.data() + (size_t)slot[j] * OS_DIGIT;
      unsigned d = 0;
      while (d < a.bin_mask && (unsigned long long)left[j] >= row[d]) left[j] -= (int64_t)row[d++];
      PP_REQUIRE(ctx, (unsigned long long)left[j] < row[d], "pp_masked_order_stats_f32: digit counts do not add up (internal error)");
      prefix[j] = (prefix[j] << widths[pass]) | d;
    }
  }
  for (int j = 0; j < nranks; ++j) out[j] = dh_unkey((int)(prefix[j] ^ 0x80000000u));
  return PP_OK;
}

}  // extern "C"
