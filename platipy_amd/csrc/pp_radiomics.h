// platipy_amd/csrc/pp_radiomics.h -- the counting behind pyradiomics' first-order and texture classes as the radiomics service
// runs them (services/radiomics/service.py:152-177), for ONE structure on the contiguous crop of its bounding box.  #included
// at the end of pp_fusion.hip (it uses that file's NT and grid_for, and pp_block_tree of pp_reduce.h).
//
// Moments (pp_masked_moments_f32).  Seven fp64 sums over the voxels with mask != 0 and lo <= v <= hi.  Thread g of the grid
// takes the strips of four voxels g, g + G, g + 2 G, ... in that order, the block folds its threads with pp_block_tree and a
// single block folds the block partials (thread t takes blocks t, t + NT, ...): a fixed order for a given n, no
// floating-point atomic, so two calls return the same bits whatever the alignment of the buffers (the 16-byte load of an
// aligned strip changes the access, not the order).
//
// Discretisation (pp_radiomics_discretise_f32).  level = np.digitize(v, edges): an arithmetic guess corrected against the
// fp64 edge table (the host's np.arange, so the edges are numpy's own bits), the fp32 value compared as a double.  A thread
// takes four voxels: one 16-byte image load, one 4-byte mask load, one 8-byte store where the three pointers allow it.
// Every voxel of the output is written, 0 outside the mask.
//
// Neighbourhood tables (pp_texture_neighbourhood_u16).  A workgroup of 256 threads walks tiles of 32 x 8 x 8 voxels; each
// tile is read once with a one-voxel halo into LDS (34 x 10 x 10 levels of 2 bytes: 6800 bytes), and every thread visits
// eight voxels of it.  blockIdx.y is the ROLE of the workgroup:
//   roles 0 ... groups - 1   the GLCM of `per` consecutive directions (13 = the offsets (dz, dy, dx) whose first non-zero
//                            component is positive, in lexicographic order): the forward neighbour counted once,
//                            glcm[d][i - 1][j - 1] += 1; the caller forms P + P^T;
//   the last role            the 26-neighbour tables: gldm[i - 1][dependents], ngtdm_n[i - 1][k] and
//                            ngtdm_s[i - 1][k] += |i k - sum of the neighbours' levels|, k = neighbours inside the mask.
// THE LDS RULE.  A role counts in a per-workgroup table of TX_LDS_WORDS = 8192 32-bit counters (32 KB; with the tile 39 KB, so
// four workgroups share a CU's 160 KB) and flushes the non-zero ones with 64-bit integer atomics once, after its last tile.
// The GLCM takes the smallest number of direction groups among 1, 2, 3, 4, 5, 7 and 13 whose `per` x Ng^2 counters fit: one
// group up to Ng = 25, thirteen up to Ng = 90; above that one role counts all 13 directions with 64-bit global atomics.  The
// 26-neighbour tables take 81 Ng counters: LDS up to Ng = 101, global atomics above.  A workgroup visits at most 256 tiles, so
// that no 32-bit counter can wrap (the largest, a sum of |i k - sum|, stays below 2^19 x 26 x 101 < 2^32).
// Ng <= TX_MAX_NG = 1024 (a GLCM of 13 x 2^20 counters, 109 MB); PP_ERR_SIZE above.
//
// Runs (pp_texture_runs_u16).  A voxel starts a run along d when its predecessor at -d is outside the box, 0 or another
// level; the starting thread walks forward (at most the longest box axis) and adds one count to glrlm[d][i - 1][length - 1].
// Runs of up to RL_LDS_LEN = 8 voxels are counted in the workgroup's LDS table while 13 x Ng x 8 <= 8192 (Ng <= 78), longer
// ones and larger Ng with global 64-bit atomics.
//
// Every table is a sum of integers: a rerun gives the same bits.  A level above Ng is never used as an index: the call
// counts such voxels and fails with PP_ERR_ARG.
#pragma once

#include <algorithm>

namespace {

constexpr int TX_LDS_WORDS = 8192;
constexpr int TX_MAX_NG = 1024;
constexpr int TX_DIRS = 13;
constexpr int TX_COLS = 27;               // 0 ... 26 neighbours
constexpr int TX_TX = 32, TX_TY = 8, TX_TZ = 8;
constexpr int TX_HX = TX_TX + 2, TX_HY = TX_TY + 2, TX_HZ = TX_TZ + 2;
constexpr int TX_MAX_TILES_PER_BLOCK = 256;
constexpr int RL_LDS_LEN = 8;
constexpr int RD_MAX_LEVELS = 65535;
constexpr int MM_SUMS = 7;                // count, S(v-c), S|v-c|, S(v-c)^2, S(v-c)^3, S(v-c)^4, S v^2

// ---------------------------------------------------------------------------------------
// moments

__device__ __forceinline__ void mm_add(double* s, float v, unsigned m, double lo, double hi, double c) {
  const double x = (double)v;
  if (!m || !(x >= lo) || !(x <= hi)) return;
  const double d = x - c, d2 = d * d;
  s[0] += 1.0;
  s[1] += d;
  s[2] += fabs(d);
  s[3] += d2;
  s[4] += d2 * d;
  s[5] += d2 * d2;
  s[6] += x * x;
}

// partial[b][MM_SUMS] = the sums of block b's strips
__global__ void __launch_bounds__(NT) k_masked_moments(const float* __restrict__ img, const uint8_t* __restrict__ mask, size_t n, double lo,
                                                       double hi, double c, int vec, double* __restrict__ partial) {
  __shared__ double sh[MM_SUMS][NT];
  const int t = threadIdx.x;
  double s[MM_SUMS];
#pragma unroll
  for (int k = 0; k < MM_SUMS; ++k) s[k] = 0.0;
  const size_t strips = (n + 3) / 4;
  for (size_t g = (size_t)blockIdx.x * NT + t; g < strips; g += (size_t)gridDim.x * NT) {
    const size_t i0 = g * 4;
    if (vec && i0 + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(img + i0);
      const unsigned m = *reinterpret_cast<const unsigned*>(mask + i0);
      if (!m) continue;
      mm_add(s, v.x, m & 0xffu, lo, hi, c);
      mm_add(s, v.y, m & 0xff00u, lo, hi, c);
      mm_add(s, v.z, m & 0xff0000u, lo, hi, c);
      mm_add(s, v.w, m & 0xff000000u, lo, hi, c);
    } else {
      for (size_t i = i0; i < i0 + 4 && i < n; ++i)
        if (mask[i]) mm_add(s, img[i], 1u, lo, hi, c);
    }
  }
#pragma unroll
  for (int k = 0; k < MM_SUMS; ++k) sh[k][t] = s[k];
  pp_block_tree<NT>(t, [&](int a, int b) {
#pragma unroll
    for (int k = 0; k < MM_SUMS; ++k) sh[k][a] += sh[k][b];
  });
  if (t < MM_SUMS) partial[(size_t)blockIdx.x * MM_SUMS + t] = sh[t][0];
}

// one block: out[k] = the partials of blocks 0 ... nb - 1, thread t folding blocks t, t + NT, ... first
__global__ void __launch_bounds__(NT) k_masked_moments_fold(const double* __restrict__ partial, int nb, double* __restrict__ out) {
  __shared__ double sh[MM_SUMS][NT];
  const int t = threadIdx.x;
  double s[MM_SUMS];
#pragma unroll
  for (int k = 0; k < MM_SUMS; ++k) s[k] = 0.0;
  for (int b = t; b < nb; b += NT)
#pragma unroll
    for (int k = 0; k < MM_SUMS; ++k) s[k] += partial[(size_t)b * MM_SUMS + k];
#pragma unroll
  for (int k = 0; k < MM_SUMS; ++k) sh[k][t] = s[k];
  pp_block_tree<NT>(t, [&](int a, int b) {
#pragma unroll
    for (int k = 0; k < MM_SUMS; ++k) sh[k][a] += sh[k][b];
  });
  if (t < MM_SUMS) out[t] = sh[t][0];
}

// ---------------------------------------------------------------------------------------
// discretisation

// np.digitize(v, e) for increasing e[0 ... ne - 1], 1 ... ne - 1; 0 when v is NaN, below e[0] or not below e[ne - 1]
__device__ __forceinline__ unsigned rd_level(double v, const double* __restrict__ e, int ne, double e0, double scale) {
  if (!(v >= e[0]) || !(v < e[ne - 1])) return 0u;
  const double g = (v - e0) * scale;
  int k = g >= (double)(ne - 2) ? ne - 2 : (g > 0.0 ? (int)g : 0);
  if (v >= e[k]) {
    if (v < e[k + 1]) return (unsigned)(k + 1);
    if (k + 2 <= ne - 1 && v < e[k + 2]) return (unsigned)(k + 2);
  } else if (k > 0 && v >= e[k - 1]) {
    return (unsigned)k;
  }
  int lo = 0, hi = ne - 1;   // e[lo] <= v < e[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (v >= e[mid]) lo = mid;
    else hi = mid;
  }
  return (unsigned)(lo + 1);
}

__global__ void __launch_bounds__(NT) k_rd_discretise(const float* __restrict__ img, const uint8_t* __restrict__ mask, size_t n,
                                                      const double* __restrict__ e, int ne, double e0, double scale, int vec,
                                                      uint16_t* __restrict__ out, unsigned long long* __restrict__ bad_count) {
  unsigned bad = 0;
  const size_t strips = (n + 3) / 4;
  for (size_t g = (size_t)blockIdx.x * NT + threadIdx.x; g < strips; g += (size_t)gridDim.x * NT) {
    const size_t i0 = g * 4;
    if (vec && i0 + 4 <= n) {
      const unsigned m = *reinterpret_cast<const unsigned*>(mask + i0);
      unsigned long long packed = 0ull;
      if (m) {
        const float4 v = *reinterpret_cast<const float4*>(img + i0);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((m >> (8 * j)) & 0xffu) {
            const unsigned l = rd_level((double)vv[j], e, ne, e0, scale);
            if (!l) ++bad;
            packed |= (unsigned long long)l << (16 * j);
          }
      }
      *reinterpret_cast<unsigned long long*>(out + i0) = packed;
    } else {
      for (size_t i = i0; i < i0 + 4 && i < n; ++i) {
        unsigned l = 0u;
        if (mask[i]) {
          l = rd_level((double)img[i], e, ne, e0, scale);
          if (!l) ++bad;
        }
        out[i] = (uint16_t)l;
      }
    }
  }
  if (bad) atomicAdd(bad_count, (unsigned long long)bad);
}

// ---------------------------------------------------------------------------------------
// the neighbourhood tables

struct tx_args {
  int nx, ny, nz, ng;
  int tiles_x, tiles_y, tiles_z;
  int groups, per;      // GLCM roles and the directions of each; groups == 0: no GLCM
  int glcm_lds;         // per * ng * ng <= TX_LDS_WORDS
  int small;            // the 26-neighbour role exists
  int small_lds;        // 3 * TX_COLS * ng <= TX_LDS_WORDS
  int want_gldm, want_ngtdm;
};

// direction d = 0 ... 12 -> the d-th offset (dz, dy, dx) after (0, 0, 0) in lexicographic order
__host__ __device__ __forceinline__ void tx_dir(int d, int& dz, int& dy, int& dx) {
  const int c = 14 + d;
  dz = c / 9 - 1;
  dy = (c / 3) % 3 - 1;
  dx = c % 3 - 1;
}

__global__ void __launch_bounds__(NT) k_texture_neighbourhood(const uint16_t* __restrict__ lev, tx_args a, unsigned long long* __restrict__ glcm,
                                                              unsigned long long* __restrict__ gldm, unsigned long long* __restrict__ ng_n,
                                                              unsigned long long* __restrict__ ng_s, unsigned long long* __restrict__ bad_count) {
  __shared__ unsigned table[TX_LDS_WORDS];
  __shared__ uint16_t tile[TX_HZ * TX_HY * TX_HX];
  const int t = threadIdx.x;
  const int role = blockIdx.y;
  const bool is_glcm = role < a.groups;
  const int d0 = is_glcm ? role * a.per : 0;
  const int d1 = is_glcm ? (d0 + a.per < TX_DIRS ? d0 + a.per : TX_DIRS) : 0;
  const int ng = a.ng;
  const bool lds = is_glcm ? a.glcm_lds != 0 : a.small_lds != 0;
  const int words = !lds ? 0 : (is_glcm ? (d1 - d0) * ng * ng : 3 * TX_COLS * ng);
  for (int i = t; i < words; i += NT) table[i] = 0u;
  unsigned bad = 0;
  const int tiles = a.tiles_x * a.tiles_y * a.tiles_z;
  const int tx = t & (TX_TX - 1), ty = t >> 5;   // 32 x 8 threads, each walks the tile's 8 planes
  for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const int x0 = (tl % a.tiles_x) * TX_TX, y0 = ((tl / a.tiles_x) % a.tiles_y) * TX_TY, z0 = (tl / (a.tiles_x * a.tiles_y)) * TX_TZ;
    __syncthreads();   // the previous tile is done with (and the table is zeroed)
    for (int i = t; i < TX_HZ * TX_HY * TX_HX; i += NT) {
      const int hx = i % TX_HX, hy = (i / TX_HX) % TX_HY, hz = i / (TX_HX * TX_HY);
      const int x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
      uint16_t l = 0;
      if (x >= 0 && x < a.nx && y >= 0 && y < a.ny && z >= 0 && z < a.nz) l = lev[((size_t)z * a.ny + y) * a.nx + x];
      tile[i] = l;
    }
    __syncthreads();
    for (int tz = 0; tz < TX_TZ; ++tz) {
      const int centre = ((tz + 1) * TX_HY + ty + 1) * TX_HX + tx + 1;
      const int li = tile[centre];
      if (!li) continue;     // outside the mask (or the box: the halo holds 0 there)
      if (li > ng) {
        ++bad;
        continue;
      }
      if (is_glcm) {
        for (int d = d0; d < d1; ++d) {
          int dz, dy, dx;
          tx_dir(d, dz, dy, dx);
          const int lj = tile[centre + (dz * TX_HY + dy) * TX_HX + dx];
          if (!lj || lj > ng) continue;   // (a level above ng is counted as bad where it is the centre)
          const int cell = (li - 1) * ng + (lj - 1);
          if (lds) atomicAdd(&table[(d - d0) * ng * ng + cell], 1u);
          else atomicAdd(&glcm[(size_t)d * ng * ng + cell], 1ull);
        }
      } else {
        int k = 0, dep = 0, sum = 0;
        for (int c = 0; c < 27; ++c) {
          if (c == 13) continue;
          const int lj = tile[centre + ((c / 9 - 1) * TX_HY + (c / 3) % 3 - 1) * TX_HX + c % 3 - 1];
          if (!lj) continue;
          ++k;
          sum += lj;
          dep += lj == li;
        }
        const int dev = li * k - sum;
        const unsigned adev = (unsigned)(dev < 0 ? -dev : dev);
        const int row = (li - 1) * TX_COLS;
        if (lds) {
          if (a.want_gldm) atomicAdd(&table[row + dep], 1u);
          if (a.want_ngtdm) {
            atomicAdd(&table[TX_COLS * ng + row + k], 1u);
            if (adev) atomicAdd(&table[2 * TX_COLS * ng + row + k], adev);
          }
        } else {
          if (a.want_gldm) atomicAdd(&gldm[row + dep], 1ull);
          if (a.want_ngtdm) {
            atomicAdd(&ng_n[row + k], 1ull);
            if (adev) atomicAdd(&ng_s[row + k], (unsigned long long)adev);
          }
        }
      }
    }
  }
  if (bad && (role == 0)) atomicAdd(bad_count, (unsigned long long)bad);
  __syncthreads();
  if (!lds) return;
  if (is_glcm) {
    unsigned long long* dst = glcm + (size_t)d0 * ng * ng;
    for (int i = t; i < words; i += NT)
      if (table[i]) atomicAdd(&dst[i], (unsigned long long)table[i]);
  } else {
    const int rows = TX_COLS * ng;
    for (int i = t; i < rows; i += NT) {
      if (a.want_gldm && table[i]) atomicAdd(&gldm[i], (unsigned long long)table[i]);
      if (a.want_ngtdm) {
        if (table[rows + i]) atomicAdd(&ng_n[i], (unsigned long long)table[rows + i]);
        if (table[2 * rows + i]) atomicAdd(&ng_s[i], (unsigned long long)table[2 * rows + i]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// runs

__global__ void __launch_bounds__(NT) k_texture_runs(const uint16_t* __restrict__ lev, int nx, int ny, int nz, int ng, int nr, int lds,
                                                     unsigned long long* __restrict__ glrlm, unsigned long long* __restrict__ bad_count) {
  __shared__ unsigned table[TX_LDS_WORDS];
  const int t = threadIdx.x;
  const int words = lds ? TX_DIRS * ng * RL_LDS_LEN : 0;
  for (int i = t; i < words; i += NT) table[i] = 0u;
  __syncthreads();
  unsigned bad = 0;
  const size_t n = (size_t)nx * ny * nz;
  for (size_t i = (size_t)blockIdx.x * NT + t; i < n; i += (size_t)gridDim.x * NT) {
    const int li = lev[i];
    if (!li) continue;
    if (li > ng) {
      ++bad;
      continue;
    }
    const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((size_t)nx * ny));
    for (int d = 0; d < TX_DIRS; ++d) {
      int dz, dy, dx;
      tx_dir(d, dz, dy, dx);
      const long long step = ((long long)dz * ny + dy) * nx + dx;
      const int px = x - dx, py = y - dy, pz = z - dz;
      if (px >= 0 && px < nx && py >= 0 && py < ny && pz >= 0 && lev[(long long)i - step] == li) continue;   // inside a run
      int len = 1;
      int qx = x + dx, qy = y + dy, qz = z + dz;
      long long q = (long long)i + step;
      while (len < nr && qx >= 0 && qx < nx && qy >= 0 && qy < ny && qz < nz && lev[q] == li) {
        ++len;
        qx += dx;
        qy += dy;
        qz += dz;
        q += step;
      }
      if (lds && len <= RL_LDS_LEN) atomicAdd(&table[(d * ng + li - 1) * RL_LDS_LEN + len - 1], 1u);
      else atomicAdd(&glrlm[((size_t)d * ng + li - 1) * nr + len - 1], 1ull);
    }
  }
  if (bad) atomicAdd(bad_count, (unsigned long long)bad);
  __syncthreads();
  for (int i = t; i < words; i += NT)
    if (table[i]) atomicAdd(&glrlm[(size_t)(i / RL_LDS_LEN) * nr + i % RL_LDS_LEN], (unsigned long long)table[i]);
}

int tx_check_box(pp_ctx* ctx, const char* who, const int size[3], int ng) {
  if (size[0] < 1 || size[1] < 1 || size[2] < 1) return pp_fail(ctx, PP_ERR_ARG, "%s: empty box", who);
  if (pp_nvox(size) >= 0x7fffffffu) return pp_fail(ctx, PP_ERR_SIZE, "%s: box of 2^31 voxels or more", who);
  if (ng < 1) return pp_fail(ctx, PP_ERR_ARG, "%s: Ng = %d", who, ng);
  if (ng > TX_MAX_NG) return pp_fail(ctx, PP_ERR_SIZE, "%s: Ng = %d (1 ... %d)", who, ng, TX_MAX_NG);
  return PP_OK;
}

}  // namespace

extern "C" {

int pp_masked_moments_f32(pp_ctx* ctx, const float* image, const uint8_t* mask, size_t n, double lo, double hi, double centre,
                          int64_t* count, double sums[6]) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, image && mask && count && sums && n > 0, "pp_masked_moments_f32: NULL or empty argument");
  PP_REQUIRE(ctx, lo == lo && hi == hi && centre - centre == 0.0, "pp_masked_moments_f32: NaN bound or a centre that is not finite");
  if (n >= 0x7fffffffu) return pp_fail(ctx, PP_ERR_SIZE, "pp_masked_moments_f32: volume of 2^31 voxels or more");
  const int nb = (int)grid_for((n + 3) / 4, 1024u);
  int rc = pp_reserve(ctx, pp_align_up((size_t)nb * MM_SUMS * sizeof(double), 256) + 256);
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  double* partial = cv.take<double>((size_t)nb * MM_SUMS);
  double* out = cv.take<double>(MM_SUMS);
  const int vec = reinterpret_cast<uintptr_t>(image) % 16 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0;
  hipLaunchKernelGGL(k_masked_moments, dim3(nb), dim3(NT), 0, ctx->stream, image, mask, n, lo, hi, centre, vec, partial);
  PP_LAUNCH_CHECK(ctx, "k_masked_moments");
  hipLaunchKernelGGL(k_masked_moments_fold, dim3(1), dim3(NT), 0, ctx->stream, (const double*)partial, nb, out);
  PP_LAUNCH_CHECK(ctx, "k_masked_moments_fold");
  double host[MM_SUMS];
  rc = pp_read_back(ctx, out, host, sizeof(host));
  if (rc) return rc;
  *count = (int64_t)host[0];
  for (int k = 0; k < 6; ++k) sums[k] = host[k + 1];
  return PP_OK;
}

int pp_radiomics_discretise_f32(pp_ctx* ctx, const float* image, const uint8_t* mask, size_t n, const double* edges, int nedges,
                                uint16_t* levels) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, image && mask && edges && levels && n > 0, "pp_radiomics_discretise_f32: NULL or empty argument");
  PP_REQUIRE(ctx, nedges >= 2, "pp_radiomics_discretise_f32: fewer than two edges");
  if (nedges - 1 > RD_MAX_LEVELS) return pp_fail(ctx, PP_ERR_SIZE, "pp_radiomics_discretise_f32: %d levels (1 ... 65535)", nedges - 1);
  if (n >= 0x7fffffffu) return pp_fail(ctx, PP_ERR_SIZE, "pp_radiomics_discretise_f32: volume of 2^31 voxels or more");
  for (int k = 0; k < nedges; ++k) {
    PP_REQUIRE(ctx, edges[k] - edges[k] == 0.0, "pp_radiomics_discretise_f32: an edge is not finite");
    PP_REQUIRE(ctx, k == 0 || edges[k] > edges[k - 1], "pp_radiomics_discretise_f32: the edges must increase");
  }
  int rc = pp_reserve(ctx, pp_align_up((size_t)nedges * sizeof(double), 256) + 256);
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  double* de = cv.take<double>((size_t)nedges);
  unsigned long long* dbad = cv.take<unsigned long long>(1);
  PP_HIP(ctx, hipMemcpyAsync(de, edges, (size_t)nedges * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PP_HIP(ctx, hipMemsetAsync(dbad, 0, sizeof(unsigned long long), ctx->stream));
  const double width = edges[nedges - 1] - edges[0];
  const double scale = width > 0.0 && width <= DBL_MAX ? (double)(nedges - 1) / width : 0.0;
  const int vec = reinterpret_cast<uintptr_t>(image) % 16 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(levels) % 8 == 0;
  hipLaunchKernelGGL(k_rd_discretise, dim3(grid_for((n + 3) / 4, 4096u)), dim3(NT), 0, ctx->stream, image, mask, n, (const double*)de, nedges,
                     edges[0], scale, vec, levels, dbad);
  PP_LAUNCH_CHECK(ctx, "k_rd_discretise");
  unsigned long long bad = 0;
  rc = pp_read_back(ctx, dbad, &bad, sizeof(bad));
  if (rc) return rc;
  if (bad)
    return pp_fail(ctx, PP_ERR_ARG, "pp_radiomics_discretise_f32: %llu voxels inside the mask are NaN, infinite or outside the edges", bad);
  return PP_OK;
}

int pp_texture_neighbourhood_u16(pp_ctx* ctx, const uint16_t* levels, const int size[3], int ng, int64_t* glcm, int64_t* gldm,
                                 int64_t* ngtdm_n, int64_t* ngtdm_s) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, levels && size, "pp_texture_neighbourhood_u16: NULL argument");
  PP_REQUIRE(ctx, glcm || gldm || ngtdm_n, "pp_texture_neighbourhood_u16: no table asked for");
  PP_REQUIRE(ctx, (ngtdm_n != nullptr) == (ngtdm_s != nullptr), "pp_texture_neighbourhood_u16: ngtdm_n and ngtdm_s go together");
  int rc = tx_check_box(ctx, "pp_texture_neighbourhood_u16", size, ng);
  if (rc) return rc;
  tx_args a;
  a.nx = size[0], a.ny = size[1], a.nz = size[2], a.ng = ng;
  a.tiles_x = (a.nx + TX_TX - 1) / TX_TX, a.tiles_y = (a.ny + TX_TY - 1) / TX_TY, a.tiles_z = (a.nz + TX_TZ - 1) / TX_TZ;
  const size_t cells = (size_t)ng * ng, rows = (size_t)TX_COLS * ng;
  a.groups = 0, a.per = TX_DIRS, a.glcm_lds = 0;
  if (glcm) {
    a.groups = 1;
    const int per_of[7] = {13, 7, 5, 4, 3, 2, 1};
    for (int k = 0; k < 7; ++k)
      if ((size_t)per_of[k] * cells <= (size_t)TX_LDS_WORDS) {
        a.per = per_of[k], a.groups = (TX_DIRS + a.per - 1) / a.per, a.glcm_lds = 1;
        break;
      }
  }
  a.small = gldm || ngtdm_n;
  a.small_lds = 3 * rows <= (size_t)TX_LDS_WORDS;
  a.want_gldm = gldm != nullptr, a.want_ngtdm = ngtdm_n != nullptr;
  const size_t n_glcm = glcm ? TX_DIRS * cells : 0, n_small = a.small ? 3 * rows : 0;
  rc = pp_reserve(ctx, pp_align_up((1 + n_glcm + n_small) * sizeof(unsigned long long), 256));
  if (rc) return rc;
  unsigned long long* dbad = reinterpret_cast<unsigned long long*>(ctx->ws);
  unsigned long long* dglcm = dbad + 1;
  unsigned long long* dsmall = dglcm + n_glcm;
  PP_HIP(ctx, hipMemsetAsync(dbad, 0, (1 + n_glcm + n_small) * sizeof(unsigned long long), ctx->stream));
  const long long tiles = (long long)a.tiles_x * a.tiles_y * a.tiles_z;
  long long blocks = tiles < 1024 ? tiles : 1024;
  if (blocks * TX_MAX_TILES_PER_BLOCK < tiles) blocks = (tiles + TX_MAX_TILES_PER_BLOCK - 1) / TX_MAX_TILES_PER_BLOCK;
  hipLaunchKernelGGL(k_texture_neighbourhood, dim3((unsigned)blocks, (unsigned)(a.groups + a.small)), dim3(NT), 0, ctx->stream, levels, a, dglcm,
                     dsmall, dsmall + rows, dsmall + 2 * rows, dbad);
  PP_LAUNCH_CHECK(ctx, "k_texture_neighbourhood");
  unsigned long long bad = 0;
  PP_HIP(ctx, hipMemcpyAsync(&bad, dbad, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (bad) return pp_fail(ctx, PP_ERR_ARG, "pp_texture_neighbourhood_u16: %llu voxels hold a level above Ng = %d", bad, ng);
  if (glcm) PP_HIP(ctx, hipMemcpyAsync(glcm, dglcm, n_glcm * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  if (gldm) PP_HIP(ctx, hipMemcpyAsync(gldm, dsmall, rows * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  if (ngtdm_n) {
    PP_HIP(ctx, hipMemcpyAsync(ngtdm_n, dsmall + rows, rows * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    PP_HIP(ctx, hipMemcpyAsync(ngtdm_s, dsmall + 2 * rows, rows * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  }
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PP_OK;
}

int pp_texture_runs_u16(pp_ctx* ctx, const uint16_t* levels, const int size[3], int ng, int nr, int64_t* glrlm) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, levels && size && glrlm, "pp_texture_runs_u16: NULL argument");
  int rc = tx_check_box(ctx, "pp_texture_runs_u16", size, ng);
  if (rc) return rc;
  const int longest = std::max(size[0], std::max(size[1], size[2]));
  PP_REQUIRE(ctx, nr == longest, "pp_texture_runs_u16: Nr must be the longest box axis");
  const size_t cells = (size_t)TX_DIRS * ng * nr;
  rc = pp_reserve(ctx, pp_align_up((1 + cells) * sizeof(unsigned long long), 256));
  if (rc) return rc;
  unsigned long long* dbad = reinterpret_cast<unsigned long long*>(ctx->ws);
  unsigned long long* dt = dbad + 1;
  PP_HIP(ctx, hipMemsetAsync(dbad, 0, (1 + cells) * sizeof(unsigned long long), ctx->stream));
  const int lds = (size_t)TX_DIRS * ng * RL_LDS_LEN <= (size_t)TX_LDS_WORDS && nr >= RL_LDS_LEN;
  hipLaunchKernelGGL(k_texture_runs, dim3(grid_for(pp_nvox(size), 1024u)), dim3(NT), 0, ctx->stream, levels, size[0], size[1], size[2], ng, nr,
                     lds, dt, dbad);
  PP_LAUNCH_CHECK(ctx, "k_texture_runs");
  unsigned long long bad = 0;
  PP_HIP(ctx, hipMemcpyAsync(&bad, dbad, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (bad) return pp_fail(ctx, PP_ERR_ARG, "pp_texture_runs_u16: %llu voxels hold a level above Ng = %d", bad, ng);
  PP_HIP(ctx, hipMemcpyAsync(glrlm, dt, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PP_OK;
}

}  // extern "C"
