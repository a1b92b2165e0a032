// platipy_amd/csrc/pp_region.h -- region primitives on top of the union-find labelling of pp_cc.hip (included at its end):
// a label image numbered as sitk.ConnectedComponent numbers it, exact per-label moments (what LabelShapeStatistics is
// computed from), seeded region growing (sitk.ConnectedThreshold) and the binary median.  They replace the host ITK calls
// of the bronchus pipeline (platipy/imaging/utils/lung.py:33-62, projects/bronchus/bronchus.py:194-196, 214-221, 259-262,
// 331-339).  Integer atomics only: every result is independent of the order in which blocks run.
#include <vector>

#include "pp_reduce.h"

namespace {

constexpr int RG_E = 16;                 // voxels per thread of the scan and moment kernels
constexpr int RG_CHUNK = NT * RG_E;      // voxels per block pass

// A component's root is its first voxel in raster order (cc_unite keeps the smaller index), so ranking the roots in index
// order IS ITK's numbering.  Reduce-then-scan in three launches: roots per chunk, an exclusive scan of the chunk counts by
// one block, then every chunk ranks its own roots from its offset.  No block ever waits for another.
__device__ __forceinline__ int rg_is_root(const uint8_t* mask, const int* L, size_t i) { return mask[i] != 0 && L[i] == (int)i; }

__global__ void __launch_bounds__(NT) k_rg_root_count(const uint8_t* __restrict__ mask, const int* __restrict__ L, size_t n, size_t nchunks,
                                                      int* __restrict__ chunk_count) {
  __shared__ int s[NT];
  for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const size_t i0 = c * RG_CHUNK + (size_t)threadIdx.x * RG_E;
    int cnt = 0;
    for (int e = 0; e < RG_E; ++e)
      if (i0 + e < n) cnt += rg_is_root(mask, L, i0 + e);
    s[threadIdx.x] = cnt;
    pp_block_tree<NT>((int)threadIdx.x, [&](int a, int b) { s[a] += s[b]; });
    if (threadIdx.x == 0) chunk_count[c] = s[0];
    __syncthreads();
  }
}

// One block: chunk_count -> its exclusive scan, in place; total[0] = the number of roots.
__global__ void __launch_bounds__(NT) k_rg_scan_chunks(int* __restrict__ chunk_count, size_t nchunks, int* __restrict__ total) {
  __shared__ int s[NT];
  int carry = 0;
  for (size_t t0 = 0; t0 < nchunks; t0 += NT) {
    const size_t k = t0 + threadIdx.x;
    const int v = k < nchunks ? chunk_count[k] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
      const int t = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += t;
      __syncthreads();
    }
    if (k < nchunks) chunk_count[k] = carry + s[threadIdx.x] - v;
    const int tile = s[NT - 1];
    __syncthreads();
    carry += tile;
  }
  if (threadIdx.x == 0) total[0] = carry;
}

// rank[root] = 1 + the number of roots before it.  Only roots are written; nothing else of `rank` is ever read.
__global__ void __launch_bounds__(NT) k_rg_rank_roots(const uint8_t* __restrict__ mask, const int* __restrict__ L, size_t n, size_t nchunks,
                                                      const int* __restrict__ chunk_offset, int* __restrict__ rank) {
  __shared__ int s[NT];
  for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const size_t i0 = c * RG_CHUNK + (size_t)threadIdx.x * RG_E;
    unsigned flags = 0;
    int cnt = 0;
    for (int e = 0; e < RG_E; ++e)
      if (i0 + e < n && rg_is_root(mask, L, i0 + e)) {
        flags |= 1u << e;
        ++cnt;
      }
    s[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
      const int t = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += t;
      __syncthreads();
    }
    int r = chunk_offset[c] + s[threadIdx.x] - cnt;
    for (int e = 0; e < RG_E; ++e)
      if (flags & (1u << e)) rank[i0 + e] = ++r;
    __syncthreads();
  }
}

// In place: a foreground voxel's root index becomes its root's rank, background becomes 0.
__global__ void __launch_bounds__(NT) k_rg_relabel(const uint8_t* __restrict__ mask, int* __restrict__ L, const int* __restrict__ rank, size_t n) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) L[i] = mask[i] ? rank[L[i]] : 0;
}

// Per-label moments.  A thread walks RG_E consecutive voxels (linear order; a run ends where the label changes or the row
// does) and keeps ten sums for the label it is in, the run's sum of x and of x^2 in closed form.  When it leaves a label it
// hands the sums to the block's LDS table -- LM_SLOTS labels per block pass, a label's slot is label % LM_SLOTS and goes to
// the largest label that asks for it in a claiming sweep before the walk -- and only labels that lost their slot go to global
// memory directly.  The table is flushed with one 64-bit atomic per non-zero entry, so the outside air of a CT costs ten
// atomics per 4096 voxels, not ten per run.  All arithmetic is modulo 2^64: exact whenever the true sums fit in int64.
constexpr int LM_SLOTS = 64;

__global__ void __launch_bounds__(NT) k_label_moments(const int* __restrict__ lab, pp_dims d, size_t n, size_t nchunks, int nlabels,
                                                      unsigned long long* __restrict__ out) {
  typedef unsigned long long u64;
  __shared__ int tag[LM_SLOTS];
  __shared__ u64 acc[LM_SLOTS * 10];
  for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    for (int k = threadIdx.x; k < LM_SLOTS; k += NT) tag[k] = 0;
    for (int k = threadIdx.x; k < LM_SLOTS * 10; k += NT) acc[k] = 0;
    __syncthreads();
    const size_t i0 = c * RG_CHUNK + (size_t)threadIdx.x * RG_E;
    int v[RG_E];
    int prev = 0;
#pragma unroll
    for (int e = 0; e < RG_E; ++e) {
      const int l = i0 + e < n ? lab[i0 + e] : 0;
      v[e] = (l >= 1 && l <= nlabels) ? l : 0;
      if (v[e] && v[e] != prev) atomicMax(&tag[v[e] & (LM_SLOTS - 1)], v[e]);
      prev = v[e];
    }
    __syncthreads();
    if (i0 < n) {
      const unsigned row = (unsigned)i0 / (unsigned)d.nx;   // (n < 2^31)
      int x = (int)((unsigned)i0 - row * (unsigned)d.nx), y = (int)(row % (unsigned)d.ny), z = (int)(row / (unsigned)d.ny);
      int cl = 0, rs = 0, rl = 0, ry = 0, rz = 0;     // label in force; open run: start x, length, its row
      u64 a[10];
#pragma unroll
      for (int k = 0; k < 10; ++k) a[k] = 0;
      auto close_run = [&]() {
        if (rl > 0 && cl) {
          const u64 len = (u64)rl, x0 = (u64)rs, uy = (u64)ry, uz = (u64)rz;
          const u64 tri = len * (len - 1) / 2;                         // sum of 0 .. len-1
          const u64 sq = (len - 1) * len * (2 * len - 1) / 6;          // sum of squares of 0 .. len-1
          const u64 sx = len * x0 + tri;
          a[0] += len;
          a[1] += sx;
          a[2] += len * uy;
          a[3] += len * uz;
          a[4] += len * x0 * x0 + 2 * x0 * tri + sq;
          a[5] += len * uy * uy;
          a[6] += len * uz * uz;
          a[7] += sx * uy;
          a[8] += sx * uz;
          a[9] += len * uy * uz;
        }
        rl = 0;
      };
      auto flush = [&]() {
        if (cl) {
          const int slot = cl & (LM_SLOTS - 1);
          u64* dst = tag[slot] == cl ? &acc[slot * 10] : &out[(size_t)(cl - 1) * 10];
#pragma unroll
          for (int k = 0; k < 10; ++k)
            if (a[k]) atomicAdd(&dst[k], a[k]);
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) a[k] = 0;
      };
#pragma unroll
      for (int e = 0; e < RG_E; ++e) {
        if (i0 + e < n) {
          if (v[e] != cl) {
            close_run();
            flush();
            cl = v[e];
          } else if (x == 0) {
            close_run();
          }
          if (rl == 0) {
            rs = x;
            ry = y;
            rz = z;
          }
          ++rl;
          if (++x == d.nx) {
            x = 0;
            if (++y == d.ny) {
              y = 0;
              ++z;
            }
          }
        }
      }
      close_run();
      flush();
    }
    __syncthreads();
    for (int k = threadIdx.x; k < LM_SLOTS * 10; k += NT) {
      const int t = tag[k / 10];
      if (t && acc[k]) atomicAdd(&out[(size_t)(t - 1) * 10 + k % 10], acc[k]);
    }
    __syncthreads();
  }
}

// lower <= v <= upper in double; a NaN (voxel or bound) compares false.
__global__ void __launch_bounds__(NT) k_rg_threshold(const float* __restrict__ image, size_t n, double lower, double upper, uint8_t* __restrict__ mask) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const double v = (double)image[i];
    mask[i] = (v >= lower && v <= upper) ? (uint8_t)1 : (uint8_t)0;
  }
}

// The seeds' roots (-1 for a seed on a voxel outside the interval), read before anything is marked ...
__global__ void __launch_bounds__(NT) k_rg_seed_roots(const int* __restrict__ seed, int nseeds, const uint8_t* __restrict__ mask,
                                                      const int* __restrict__ L, int* __restrict__ roots) {
  for (int j = blockIdx.x * NT + threadIdx.x; j < nseeds; j += gridDim.x * NT) roots[j] = mask[seed[j]] ? L[seed[j]] : -1;
}

// ... then marked in the label array itself: a selected root points at -1.  (Seeds that share a root store the same value.)
__global__ void __launch_bounds__(NT) k_rg_mark_roots(const int* __restrict__ roots, int nseeds, int* __restrict__ L) {
  for (int j = blockIdx.x * NT + threadIdx.x; j < nseeds; j += gridDim.x * NT)
    if (roots[j] >= 0) L[roots[j]] = -1;
}

__global__ void __launch_bounds__(NT) k_rg_select(const uint8_t* __restrict__ mask, const int* __restrict__ L, uint8_t* __restrict__ out, size_t n,
                                                  unsigned long long* __restrict__ voxels) {
  __shared__ int s[NT];
  int cnt = 0;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    bool in = false;
    if (mask[i]) {
      const int r = L[i];
      in = r < 0 || L[r] < 0;
    }
    out[i] = in ? (uint8_t)1 : (uint8_t)0;
    cnt += in;
  }
  s[threadIdx.x] = cnt;
  pp_block_tree<NT>((int)threadIdx.x, [&](int a, int b) { s[a] += s[b]; });
  if (threadIdx.x == 0 && s[0]) atomicAdd(voxels, (unsigned long long)s[0]);
}

// Binary median: a block computes a MD_TX x MD_TY x MD_TZ brick from an LDS tile of the brick plus its halo, the halo
// clamped to the volume (edge replication, itk::ZeroFluxNeumannBoundaryCondition).
constexpr int MD_TX = 32, MD_TY = 8, MD_TZ = 4, MD_R = 2;
constexpr int MD_LX = MD_TX + 2 * MD_R, MD_LY = MD_TY + 2 * MD_R, MD_LZ = MD_TZ + 2 * MD_R;

__global__ void __launch_bounds__(NT) k_binary_median(const uint8_t* __restrict__ in, pp_dims d, int rx, int ry, int rz, uint8_t* __restrict__ out) {
  __shared__ uint8_t tile[MD_LZ * MD_LY * MD_LX];
  const int bx = (int)blockIdx.x * MD_TX, by = (int)blockIdx.y * MD_TY, bz = (int)blockIdx.z * MD_TZ;
  const int lx = MD_TX + 2 * rx, ly = MD_TY + 2 * ry, lz = MD_TZ + 2 * rz;
  for (int k = threadIdx.x; k < lx * ly * lz; k += NT) {
    const int tx = k % lx, ty = (k / lx) % ly, tz = k / (lx * ly);
    const int gx = pp_clampi(bx + tx - rx, 0, d.nx - 1), gy = pp_clampi(by + ty - ry, 0, d.ny - 1), gz = pp_clampi(bz + tz - rz, 0, d.nz - 1);
    tile[(tz * MD_LY + ty) * MD_LX + tx] = in[((size_t)gz * d.ny + gy) * d.nx + gx] != 0 ? (uint8_t)1 : (uint8_t)0;
  }
  __syncthreads();
  const int tx = (int)threadIdx.x % MD_TX, ty = (int)threadIdx.x / MD_TX;
  const int x = bx + tx, y = by + ty;
  const int half = (2 * rx + 1) * (2 * ry + 1) * (2 * rz + 1) / 2;
  for (int tz = 0; tz < MD_TZ; ++tz) {
    const int z = bz + tz;
    if (x >= d.nx || y >= d.ny || z >= d.nz) continue;
    int ones = 0;
    for (int dz = 0; dz <= 2 * rz; ++dz)
      for (int dy = 0; dy <= 2 * ry; ++dy) {
        const uint8_t* row = &tile[((tz + dz) * MD_LY + ty + dy) * MD_LX + tx];
        for (int dx = 0; dx <= 2 * rx; ++dx) ones += row[dx];
      }
    out[((size_t)z * d.ny + y) * d.nx + x] = ones > half ? (uint8_t)1 : (uint8_t)0;
  }
}

int rg_volume_args(pp_ctx* ctx, const int* size, const char* who, size_t* n) {
  if (!(size[0] > 0 && size[1] > 0 && size[2] > 0)) return pp_fail(ctx, PP_ERR_ARG, "%s: empty volume", who);
  *n = pp_nvox(size);
  if (!(*n < 2147483647u)) return pp_fail(ctx, PP_ERR_SIZE, "%s: 2^31 voxels or more", who);
  return PP_OK;
}

int rg_connected_components(pp_ctx* ctx, const uint8_t* mask, const int size[3], int full, int32_t* labels, int* count) {
  PP_REQUIRE(ctx, mask && size && labels, "pp_connected_components_u8: NULL argument");
  size_t n = 0;
  int rc = rg_volume_args(ctx, size, "pp_connected_components_u8", &n);
  if (rc) return rc;
  const pp_dims d{size[0], size[1], size[2]};
  const size_t nchunks = (n + RG_CHUNK - 1) / RG_CHUNK;
  rc = pp_reserve(ctx, pp_align_up(n * sizeof(int), 256) + pp_align_up((nchunks + 1) * sizeof(int), 256));
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  int* rank = cv.take<int>(n);
  int* chunk = cv.take<int>(nchunks + 1);
  int* total = chunk + nchunks;
  int* L = reinterpret_cast<int*>(labels);
  rc = cc_label(ctx, mask, L, d, n, 1, full);
  if (rc) return rc;
  const dim3 gc((unsigned)(nchunks < 16384 ? nchunks : 16384)), b(NT);
  hipLaunchKernelGGL(k_rg_root_count, gc, b, 0, ctx->stream, mask, (const int*)L, n, nchunks, chunk);
  PP_LAUNCH_CHECK(ctx, "k_rg_root_count");
  hipLaunchKernelGGL(k_rg_scan_chunks, dim3(1), b, 0, ctx->stream, chunk, nchunks, total);
  PP_LAUNCH_CHECK(ctx, "k_rg_scan_chunks");
  hipLaunchKernelGGL(k_rg_rank_roots, gc, b, 0, ctx->stream, mask, (const int*)L, n, nchunks, (const int*)chunk, rank);
  PP_LAUNCH_CHECK(ctx, "k_rg_rank_roots");
  hipLaunchKernelGGL(k_rg_relabel, dim3(grid_for(n)), b, 0, ctx->stream, mask, L, (const int*)rank, n);
  PP_LAUNCH_CHECK(ctx, "k_rg_relabel");
  if (count) {
    int h = 0;
    rc = pp_read_back(ctx, total, &h, sizeof(h));
    if (rc) return rc;
    *count = h;
  }
  return PP_OK;
}

}  // namespace

extern "C" {

int pp_connected_components_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], int32_t* labels, int* count) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  return rg_connected_components(ctx, mask, size, 0, labels, count);
}

int pp_connected_components_conn_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], int fully_connected, int32_t* labels, int* count) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  return rg_connected_components(ctx, mask, size, fully_connected != 0, labels, count);
}

int pp_label_moments_i32(pp_ctx* ctx, const int32_t* labels, const int size[3], int nlabels, int64_t* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, labels && size && nlabels >= 0 && (out || nlabels == 0), "pp_label_moments_i32: NULL argument or negative label count");
  size_t n = 0;
  int rc = rg_volume_args(ctx, size, "pp_label_moments_i32", &n);
  if (rc) return rc;
  if (nlabels == 0) return PP_OK;
  const pp_dims d{size[0], size[1], size[2]};
  const size_t nchunks = (n + RG_CHUNK - 1) / RG_CHUNK;
  unsigned long long* dout = reinterpret_cast<unsigned long long*>(out);
  PP_HIP(ctx, hipMemsetAsync(dout, 0, (size_t)nlabels * 10 * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_label_moments, dim3((unsigned)(nchunks < 16384 ? nchunks : 16384)), dim3(NT), 0, ctx->stream,
                     reinterpret_cast<const int*>(labels), d, n, nchunks, nlabels, dout);
  PP_LAUNCH_CHECK(ctx, "k_label_moments");
  return PP_OK;
}

int pp_connected_threshold_f32(pp_ctx* ctx, const float* image, const int size[3], double lower, double upper, const int* seeds,
                               int nseeds, uint8_t* out, int64_t* voxels) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, image && size && out && nseeds >= 0 && (seeds || nseeds == 0), "pp_connected_threshold_f32: NULL argument or negative seed count");
  size_t n = 0;
  int rc = rg_volume_args(ctx, size, "pp_connected_threshold_f32", &n);
  if (rc) return rc;
  std::vector<int> lin((size_t)nseeds);
  for (int j = 0; j < nseeds; ++j) {
    const int x = seeds[3 * j], y = seeds[3 * j + 1], z = seeds[3 * j + 2];
    if (x < 0 || y < 0 || z < 0 || x >= size[0] || y >= size[1] || z >= size[2])
      return pp_fail(ctx, PP_ERR_INVALID, "pp_connected_threshold_f32: seed %d (%d, %d, %d) is outside the buffer", j, x, y, z);
    lin[(size_t)j] = (int)(((size_t)z * size[1] + y) * size[0] + x);
  }
  const pp_dims d{size[0], size[1], size[2]};
  const size_t ns = nseeds > 0 ? (size_t)nseeds : 1;
  rc = pp_reserve(ctx, pp_align_up(n * sizeof(int), 256) + pp_align_up(n, 256) + 2 * pp_align_up(ns * sizeof(int), 256) + 256);
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  int* L = cv.take<int>(n);
  uint8_t* mask = cv.take<uint8_t>(n);
  int* dseed = cv.take<int>(ns);
  int* roots = cv.take<int>(ns);
  unsigned long long* dvox = cv.take<unsigned long long>(1);
  const dim3 g(grid_for(n)), b(NT);
  PP_HIP(ctx, hipMemsetAsync(dvox, 0, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_rg_threshold, g, b, 0, ctx->stream, image, n, lower, upper, mask);
  PP_LAUNCH_CHECK(ctx, "k_rg_threshold");
  rc = cc_label(ctx, mask, L, d, n, 1);
  if (rc) return rc;
  if (nseeds > 0) {
    PP_HIP(ctx, hipMemcpyAsync(dseed, lin.data(), (size_t)nseeds * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const dim3 gs(grid_for((size_t)nseeds, 1024u));
    hipLaunchKernelGGL(k_rg_seed_roots, gs, b, 0, ctx->stream, (const int*)dseed, nseeds, (const uint8_t*)mask, (const int*)L, roots);
    PP_LAUNCH_CHECK(ctx, "k_rg_seed_roots");
    hipLaunchKernelGGL(k_rg_mark_roots, gs, b, 0, ctx->stream, (const int*)roots, nseeds, L);
    PP_LAUNCH_CHECK(ctx, "k_rg_mark_roots");
  }
  hipLaunchKernelGGL(k_rg_select, dim3(grid_for(n, 2048u)), b, 0, ctx->stream, (const uint8_t*)mask, (const int*)L, out, n, dvox);
  PP_LAUNCH_CHECK(ctx, "k_rg_select");
  unsigned long long h = 0;
  rc = pp_read_back(ctx, dvox, &h, sizeof(h));   // (also: the seed list above is host memory of this call)
  if (rc) return rc;
  if (voxels) *voxels = (int64_t)h;
  return PP_OK;
}

int pp_binary_median_u8(pp_ctx* ctx, const uint8_t* in, const int size[3], const int radius[3], uint8_t* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, in && size && radius && out && in != out, "pp_binary_median_u8: NULL or aliased argument");
  size_t n = 0;
  int rc = rg_volume_args(ctx, size, "pp_binary_median_u8", &n);
  if (rc) return rc;
  for (int a = 0; a < 3; ++a) PP_REQUIRE(ctx, radius[a] >= 0 && radius[a] <= MD_R, "pp_binary_median_u8: radius outside [0, 2]");
  const pp_dims d{size[0], size[1], size[2]};
  const dim3 grid((unsigned)((d.nx + MD_TX - 1) / MD_TX), (unsigned)((d.ny + MD_TY - 1) / MD_TY), (unsigned)((d.nz + MD_TZ - 1) / MD_TZ));
  if (grid.y > 65535u || grid.z > 65535u) return pp_fail(ctx, PP_ERR_SIZE, "pp_binary_median_u8: volume too large");
  hipLaunchKernelGGL(k_binary_median, grid, dim3(NT), 0, ctx->stream, in, d, radius[0], radius[1], radius[2], out);
  PP_LAUNCH_CHECK(ctx, "k_binary_median");
  return PP_OK;
}

}  // extern "C"
