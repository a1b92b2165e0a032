// platipy_amd/csrc/pp_patch_corr.h -- the two numpy / scipy pieces of platipy/imaging/label/fusion.py: the local Pearson
// correlation of compute_weight_map(vote_type="patch_correlation") (:94-132) and the joint histogram behind
// mutual_information (:26-53).  #included at the end of pp_fusion.hip (it uses that file's NT and grid_for, and calls
// pp_minmax_f32).
//
// Patch correlation.  The reference pads both arrays and a mask of ones, cuts one window per voxel and calls
// scipy.stats.pearsonr on the unmasked values; here one workgroup owns 8 x 8 x 4 output voxels, stages that brick plus the
// window's halo of BOTH images in LDS (19 KB for a window of 8, 79 KB for 16) and every thread walks its own window in
// raster order.  The moments n, Sx, Sy, Sxx, Syy, Sxy are fp64 sums of values shifted by the patch's first in-image voxel:
// the shift removes the -1000 HU offset before anything is squared, the difference of two floats is exact in fp64, and
// the order is fixed, so a rerun gives the same bits.  "Constant patch" (scipy's NaN, the reference's 0) is the exact
// all-equal test scipy makes, carried along the same walk.
//
// Joint histogram.  Edges are numpy's linspace in fp64, built on the host; a thread guesses the bin arithmetically and
// walks the guess onto the bin np.searchsorted(side="right") picks.  Counts are integers: LDS per workgroup, then one
// 64-bit integer atomic per non-empty bin.
#pragma once

namespace {

// ---------------------------------------------------------------------------------------
// local Pearson correlation

constexpr int PC_BX = 8, PC_BY = 8, PC_BZ = 4;   // outputs of one workgroup, one per thread
static_assert(PC_BX * PC_BY * PC_BZ == NT, "one output voxel per thread");

struct pc_args {
  pp_dims d;
  int wx, wy, wz;      // window
  int lx, ly, lz;      // (w - 1) / 2: voxels in front of the centre
  int bxn, byn;        // bricks along x and y
};

struct pc_box {
  int x0, x1, y0, y1, z0, z1;   // the patch, clipped to the image (inclusive)
};

__device__ __forceinline__ pc_box pc_patch(const pc_args& a, int x, int y, int z) {
  pc_box b;
  b.x0 = x - a.lx < 0 ? 0 : x - a.lx;
  b.y0 = y - a.ly < 0 ? 0 : y - a.ly;
  b.z0 = z - a.lz < 0 ? 0 : z - a.lz;
  b.x1 = x + a.wx / 2 > a.d.nx - 1 ? a.d.nx - 1 : x + a.wx / 2;
  b.y1 = y + a.wy / 2 > a.d.ny - 1 ? a.d.ny - 1 : y + a.wy / 2;
  b.z1 = z + a.wz / 2 > a.d.nz - 1 ? a.d.nz - 1 : z + a.wz / 2;
  return b;
}

// One patch.  Voxel (x, y, z) of the two images is rt / rm[z * sz + y * sy + x - back] (global memory, or an LDS tile whose
// first element is image voxel `back`).
__device__ __forceinline__ float pc_pearson(const float* __restrict__ rt, const float* __restrict__ rm, int sy, int sz, int back,
                                            const pc_box& b) {
  const float t0 = rt[b.z0 * sz + b.y0 * sy + b.x0 - back], m0 = rm[b.z0 * sz + b.y0 * sy + b.x0 - back];
  const double dt0 = (double)t0, dm0 = (double)m0;
  bool const_t = true, const_m = true;
  double sx = 0.0, sy_ = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
  for (int z = b.z0; z <= b.z1; ++z)
    for (int y = b.y0; y <= b.y1; ++y) {
      const int row = z * sz + y * sy - back;
      for (int x = b.x0; x <= b.x1; ++x) {
        const float tv = rt[row + x], mv = rm[row + x];
        const_t = const_t && tv == t0;
        const_m = const_m && mv == m0;
        const double dt = (double)tv - dt0, dm = (double)mv - dm0;
        sx += dt;
        sy_ += dm;
        sxx += dt * dt;
        syy += dm * dm;
        sxy += dt * dm;
      }
    }
  if (const_t || const_m) return 0.0f;   // scipy: (x == x[0]).all() -> NaN; the reference: NaN -> 0
  const double n = (double)(b.x1 - b.x0 + 1) * (double)(b.y1 - b.y0 + 1) * (double)(b.z1 - b.z0 + 1);
  const double vx = sxx - sx * sx / n, vy = syy - sy_ * sy_ / n, cov = sxy - sx * sy_ / n;
  const double den = sqrt(vx) * sqrt(vy);
  double r = den > 0.0 ? cov / den : 0.0;
  if (!(r == r)) r = 0.0;                // non-finite input: NaN in scipy too
  r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
  return (float)r;
}

// Windows of up to WMAX voxels per axis from an LDS tile.  Block b owns the brick (b % bxn, (b / bxn) % byn, b / (bxn byn)).
template <int WMAX>
__global__ void __launch_bounds__(NT) k_patch_corr_tile(const float* __restrict__ target, const float* __restrict__ moving, pc_args a,
                                                        float* __restrict__ corr) {
  constexpr int TX = PC_BX + WMAX - 1, TY = PC_BY + WMAX - 1, TZ = PC_BZ + WMAX - 1;
  __shared__ float st[TZ * TY * TX];
  __shared__ float sm[TZ * TY * TX];
  const int t = threadIdx.x;
  const int bx = (int)(blockIdx.x % (unsigned)a.bxn), by = (int)((blockIdx.x / (unsigned)a.bxn) % (unsigned)a.byn),
            bz = (int)(blockIdx.x / ((unsigned)a.bxn * (unsigned)a.byn));
  // tile voxel (0, 0, 0) is image voxel (ox, oy, oz); the part of the tile this window reaches is ex x ey x ez
  const int ox = bx * PC_BX - a.lx, oy = by * PC_BY - a.ly, oz = bz * PC_BZ - a.lz;
  const int ex = PC_BX + a.wx - 1, ey = PC_BY + a.wy - 1, ez = PC_BZ + a.wz - 1;
  const size_t gsy = (size_t)a.d.nx, gsz = (size_t)a.d.nx * a.d.ny;
  for (int i = t; i < ex * ey * ez; i += NT) {
    const int tx = i % ex, ty = (i / ex) % ey, tz = i / (ex * ey);
    const int gx = ox + tx, gy = oy + ty, gz = oz + tz;
    const bool in = gx >= 0 && gx < a.d.nx && gy >= 0 && gy < a.d.ny && gz >= 0 && gz < a.d.nz;
    const size_t g = in ? (size_t)gz * gsz + (size_t)gy * gsy + (size_t)gx : 0;
    st[(tz * TY + ty) * TX + tx] = in ? target[g] : 0.0f;   // (never read: a patch is clipped to the image)
    sm[(tz * TY + ty) * TX + tx] = in ? moving[g] : 0.0f;
  }
  __syncthreads();
  const int x = bx * PC_BX + (t % PC_BX), y = by * PC_BY + ((t / PC_BX) % PC_BY), z = bz * PC_BZ + t / (PC_BX * PC_BY);
  if (x >= a.d.nx || y >= a.d.ny || z >= a.d.nz) return;
  const pc_box b = pc_patch(a, x, y, z);
  corr[(size_t)z * gsz + (size_t)y * gsy + (size_t)x] = pc_pearson(st, sm, TX, TY * TX, (oz * TY + oy) * TX + ox, b);
}

// Any window, patches read from global memory (the volume must have fewer than 2^31 voxels).
__global__ void __launch_bounds__(NT) k_patch_corr_global(const float* __restrict__ target, const float* __restrict__ moving, pc_args a,
                                                          float* __restrict__ corr) {
  const size_t n = (size_t)a.d.nx * a.d.ny * a.d.nz;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const int x = (int)(i % a.d.nx), y = (int)((i / a.d.nx) % a.d.ny), z = (int)(i / ((size_t)a.d.nx * a.d.ny));
    corr[i] = pc_pearson(target, moving, a.d.nx, a.d.nx * a.d.ny, 0, pc_patch(a, x, y, z));
  }
}

// ---------------------------------------------------------------------------------------
// joint histogram

constexpr int JH_LDS_BINS = 16384;   // 128 x 128 counters of 4 bytes: 64 KB of LDS

struct jh_axis {
  double lo, scale;   // the arithmetic guess: bin ~ (v - lo) * scale
  int bins;
};

// np.searchsorted(e, v, side="right") - 1 for lo <= v <= hi, the top edge closed: the bin with e[k] <= v < e[k + 1]
__device__ __forceinline__ int jh_bin(double v, const double* __restrict__ e, const jh_axis& ax) {
  const double g = (v - ax.lo) * ax.scale;
  int k = g >= (double)(ax.bins - 1) ? ax.bins - 1 : (g > 0.0 ? (int)g : 0);
  while (k > 0 && v < e[k]) --k;
  while (k < ax.bins - 1 && v >= e[k + 1]) ++k;
  return k;
}

// hist[ia * bins_b + ib] += 1 per sample; hist[bins_a * bins_b] += the samples holding a NaN.  edges = bins_a + 1 edges of
// a, then bins_b + 1 edges of b.
__global__ void __launch_bounds__(NT) k_joint_histogram(const float* __restrict__ a, const float* __restrict__ b, size_t n, jh_axis aa, jh_axis ab,
                                                        const double* __restrict__ edges, int use_lds, unsigned long long* __restrict__ hist) {
  __shared__ unsigned sh[JH_LDS_BINS];
  const int nb2 = aa.bins * ab.bins;
  const int t = threadIdx.x;
  if (use_lds) {
    for (int i = t; i < nb2; i += NT) sh[i] = 0u;
    __syncthreads();
  }
  const double* ea = edges;
  const double* eb = edges + aa.bins + 1;
  unsigned bad = 0;
  for (size_t i = (size_t)blockIdx.x * NT + t; i < n; i += (size_t)gridDim.x * NT) {
    const float va = a[i], vb = b[i];
    if (!(va == va) || !(vb == vb)) {
      ++bad;
      continue;
    }
    const int k = jh_bin((double)va, ea, aa) * ab.bins + jh_bin((double)vb, eb, ab);
    if (use_lds) atomicAdd(&sh[k], 1u);
    else atomicAdd(&hist[k], 1ull);
  }
  if (bad) atomicAdd(&hist[nb2], (unsigned long long)bad);
  if (use_lds) {
    __syncthreads();
    for (int i = t; i < nb2; i += NT)
      if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
  }
}

// numpy.linspace(lo, hi, bins + 1) in fp64: i * step + lo as a rounded product and a rounded sum, the last edge = hi
void jh_linspace(double lo, double hi, int bins, double* e) {
  const double delta = hi - lo, step = delta / (double)bins;
  for (int i = 0; i <= bins; ++i) {
    volatile double p = step != 0.0 ? (double)i * step : (double)i / (double)bins * delta;   // (volatile: never fused into the sum)
    e[i] = p + lo;
  }
  e[bins] = hi;
}

}  // namespace

extern "C" {

int pp_patch_correlation_f32(pp_ctx* ctx, const float* target, const float* moving, const int size[3], const int window[3], float* corr) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, target && moving && size && window && corr, "pp_patch_correlation_f32: NULL argument");
  PP_REQUIRE(ctx, corr != target && corr != moving, "pp_patch_correlation_f32: corr aliases an input");
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_patch_correlation_f32: empty volume");
  PP_REQUIRE(ctx, window[0] >= 1 && window[1] >= 1 && window[2] >= 1, "pp_patch_correlation_f32: a window is at least 1 voxel per axis");
  if (window[0] <= 2 && window[1] <= 2 && window[2] <= 2)
    return pp_fail(ctx, PP_ERR_SIZE, "pp_patch_correlation_f32: window %d x %d x %d leaves a single voxel in a corner patch (pearsonr needs 2)",
                   window[0], window[1], window[2]);
  if (pp_nvox(size) >= 0x7fffffffu) return pp_fail(ctx, PP_ERR_SIZE, "pp_patch_correlation_f32: volume of 2^31 voxels or more");
  pc_args a;
  a.d = pp_dims{size[0], size[1], size[2]};
  a.wx = window[0], a.wy = window[1], a.wz = window[2];
  a.lx = (a.wx - 1) / 2, a.ly = (a.wy - 1) / 2, a.lz = (a.wz - 1) / 2;
  a.bxn = (size[0] + PC_BX - 1) / PC_BX, a.byn = (size[1] + PC_BY - 1) / PC_BY;
  const size_t bricks = (size_t)a.bxn * a.byn * (size_t)((size[2] + PC_BZ - 1) / PC_BZ);
  const int wmax = a.wx > a.wy ? (a.wx > a.wz ? a.wx : a.wz) : (a.wy > a.wz ? a.wy : a.wz);
  if (wmax <= 8) {
    hipLaunchKernelGGL(k_patch_corr_tile<8>, dim3((unsigned)bricks), dim3(NT), 0, ctx->stream, target, moving, a, corr);
    PP_LAUNCH_CHECK(ctx, "k_patch_corr_tile<8>");
  } else if (wmax <= 16) {
    hipLaunchKernelGGL(k_patch_corr_tile<16>, dim3((unsigned)bricks), dim3(NT), 0, ctx->stream, target, moving, a, corr);
    PP_LAUNCH_CHECK(ctx, "k_patch_corr_tile<16>");
  } else {
    hipLaunchKernelGGL(k_patch_corr_global, dim3(grid_for(pp_nvox(size))), dim3(NT), 0, ctx->stream, target, moving, a, corr);
    PP_LAUNCH_CHECK(ctx, "k_patch_corr_global");
  }
  return PP_OK;
}

int pp_joint_histogram_f32(pp_ctx* ctx, const float* a, const float* b, size_t n, int bins_a, int bins_b, int64_t* hist, double range[4]) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, a && b && hist && range && n > 0, "pp_joint_histogram_f32: NULL or empty argument");
  PP_REQUIRE(ctx, bins_a >= 1 && bins_b >= 1 && (size_t)bins_a * (size_t)bins_b <= ((size_t)1 << 24),
             "pp_joint_histogram_f32: 1 <= bins, bins_a * bins_b <= 2^24");
  float lo[2], hi[2];
  int rc = pp_minmax_f32(ctx, a, n, &lo[0], &hi[0]);
  if (!rc) rc = pp_minmax_f32(ctx, b, n, &lo[1], &hi[1]);
  if (rc) return rc;
  const int bins[2] = {bins_a, bins_b};
  std::vector<double> edges((size_t)bins_a + bins_b + 2);
  jh_axis ax[2];
  double* e = edges.data();
  for (int k = 0; k < 2; ++k) {
    // (min / max skip NaNs: an all-NaN array leaves lo > hi here, and the kernel counts every NaN it meets)
    if (!(fabsf(lo[k]) <= FLT_MAX) || !(fabsf(hi[k]) <= FLT_MAX))
      return pp_fail(ctx, PP_ERR_ARG, "pp_joint_histogram_f32: non-finite value in array %c", k ? 'b' : 'a');
    double l = (double)lo[k], h = (double)hi[k];
    if (l >= h) l -= 0.5, h += 0.5;      // numpy's _get_outer_edges
    jh_linspace(l, h, bins[k], e);
    ax[k] = jh_axis{l, (double)bins[k] / (h - l), bins[k]};
    range[2 * k] = l;
    range[2 * k + 1] = h;
    e += bins[k] + 1;
  }
  const size_t nb2 = (size_t)bins_a * bins_b;
  const unsigned nb = grid_for(n, 256u);
  PP_REQUIRE(ctx, n / nb < 0xffffffffu, "pp_joint_histogram_f32: too many samples");     // a block's 32-bit counters
  const size_t hist_bytes = pp_align_up((nb2 + 1) * sizeof(unsigned long long), 256);
  rc = pp_reserve(ctx, hist_bytes + pp_align_up(edges.size() * sizeof(double), 256));
  if (rc) return rc;
  unsigned long long* dh = reinterpret_cast<unsigned long long*>(ctx->ws);
  double* de = reinterpret_cast<double*>(ctx->ws + hist_bytes);
  PP_HIP(ctx, hipMemsetAsync(dh, 0, (nb2 + 1) * sizeof(unsigned long long), ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(de, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_joint_histogram, dim3(nb), dim3(NT), 0, ctx->stream, a, b, n, ax[0], ax[1], (const double*)de,
                     nb2 <= (size_t)JH_LDS_BINS ? 1 : 0, dh);
  PP_LAUNCH_CHECK(ctx, "k_joint_histogram");
  unsigned long long bad = 0;
  PP_HIP(ctx, hipMemcpyAsync(hist, dh, nb2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(&bad, dh + nb2, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (bad) return pp_fail(ctx, PP_ERR_ARG, "pp_joint_histogram_f32: %llu samples hold a NaN", bad);
  return PP_OK;
}

}  // extern "C"
