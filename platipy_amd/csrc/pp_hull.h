// platipy_amd/csrc/pp_hull.h -- the convex hull image of every z-slice of a binary volume (included at the end of pp_cc.hip).
//
// Replaces the Python loop of skimage.morphology.convex_hull_image calls at the end of get_external_mask
// (platipy/imaging/generation/mask.py:94-99).  Exact: integers only, no floating point takes part in any decision.
//
// Definition (include/platipy_amd.h): with S the non-zero pixels (y, x) of a slice and P the four diamond points
// (y +- 1/2, x), (y, x +- 1/2) of every pixel of S, out = 1 iff the pixel centre lies in the CLOSED convex hull of P.
// Everything is kept in doubled coordinates Y = 2 y, X = 2 x, so P is integer: (2y +- 1, 2x), (2y, 2x +- 1).
//
// Three launches, no block waits for another, no atomics on global memory:
//   extents  one wavefront per row reads it in 16-byte strips and leaves (first, last) non-zero x.  Only these two pixels
//            of a row can put points on the hull: the diamond points of the pixels between them lie on segments between
//            the extremes' points.
//   chain    one workgroup per slice.  The slice of the hull at height Y is the interval [L(Y), R(Y)], L the lower convex
//            envelope of Y -> (smallest X of a point of P at Y) and R the upper envelope of the largest.  Every Y from
//            2 ymin - 1 to 2 ymax + 1 has at most one candidate per side, so the envelope is one monotone-chain scan over an
//            array indexed by Y -- the left side by one thread, the right side by a thread of another wavefront, the stack
//            in place over the candidates already consumed (in LDS up to HULL_LDS_ROWS rows, in the context's scratch memory
//            beyond).  Then every row finds the chain edge that spans 2 y by bisection and takes the closed integer interval
//            [ceil(L / 2), floor(R / 2)] by exact 64-bit division.
//   fill     out = 1 on [xl, xr] of every row, 0 elsewhere, in 16-byte stores.
// 16-byte accesses need a 16-byte aligned pointer and nx % 16 == 0; otherwise the same code moves bytes.
// The extents are complete before the first byte of `out` is written, so `out` may be `mask` itself.

namespace {

constexpr int HULL_MAX_DIM = 65535;
constexpr int HULL_LDS_ROWS = 1024;                 // rows of a slice whose chains are built in LDS
constexpr int HULL_LDS_N = 2 * HULL_LDS_ROWS + 1;   // candidates per side: Y = 2 y - 1 ... 2 y + 1 of every row
constexpr int HULL_NONE = 0x7fffffff;
constexpr int HULL_WPB = NT / 64;                   // rows a block of the extents kernel has in flight

// Bytes p[0 ... 15] as four little-endian words; with !vec only p[0 ... valid - 1] are touched, the rest are 0.
__device__ __forceinline__ void hull_load16(const uint8_t* __restrict__ p, int valid, bool vec, unsigned w[4]) {
  if (vec) {
    const int4 v = *reinterpret_cast<const int4*>(p);
    w[0] = (unsigned)v.x;
    w[1] = (unsigned)v.y;
    w[2] = (unsigned)v.z;
    w[3] = (unsigned)v.w;
  } else {
    w[0] = w[1] = w[2] = w[3] = 0u;
    for (int j = 0; j < valid; ++j) w[j >> 2] |= (unsigned)p[j] << (8 * (j & 3));
  }
}

// bit 8 k + 7 set where byte k of w is non-zero
__device__ __forceinline__ unsigned hull_nonzero_bytes(unsigned w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }

// ext[2 row] = first, ext[2 row + 1] = last non-zero x of the row; (nx, -1) for an empty row.
__global__ void __launch_bounds__(NT) k_hull_extents(const uint8_t* __restrict__ mask, pp_dims d, int vec, int* __restrict__ ext) {
  __shared__ int s_lo[HULL_WPB], s_hi[HULL_WPB];
  const size_t rows = (size_t)d.ny * d.nz;
  const int lane = (int)threadIdx.x & 63, wib = (int)threadIdx.x >> 6;
  const int nstrips = (d.nx + 15) / 16;
  if (lane == 0) {
    s_lo[wib] = d.nx;
    s_hi[wib] = -1;
  }
  for (size_t row0 = (size_t)blockIdx.x * HULL_WPB; row0 < rows; row0 += (size_t)gridDim.x * HULL_WPB) {   // (block-uniform)
    const size_t row = row0 + wib;
    __syncthreads();
    if (row < rows) {
      const uint8_t* __restrict__ m = mask + row * d.nx;
      int lo = d.nx, hi = -1;
      for (int s = lane; s < nstrips; s += 64) {
        const int x0 = s * 16;
        unsigned w[4];
        hull_load16(m + x0, d.nx - x0 < 16 ? d.nx - x0 : 16, vec != 0, w);
        if (!(w[0] | w[1] | w[2] | w[3])) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned b = hull_nonzero_bytes(w[q]);
          if (b) {
            const int first = x0 + 4 * q + (__builtin_ctz(b) >> 3), last = x0 + 4 * q + ((31 - __builtin_clz(b)) >> 3);
            if (first < lo) lo = first;
            if (last > hi) hi = last;
          }
        }
      }
      if (hi >= 0) {
        atomicMin(&s_lo[wib], lo);
        atomicMax(&s_hi[wib], hi);
      }
    }
    __syncthreads();
    if (lane == 0 && row < rows) {
      ext[2 * row] = s_lo[wib];
      ext[2 * row + 1] = s_hi[wib];
      s_lo[wib] = d.nx;
      s_hi[wib] = -1;
    }
  }
}

// Lower convex envelope of the points (i, cx[i]), cx[i] != HULL_NONE, i = 0 ... n - 1: the vertices come back in
// (sy[k], cx[k]), k < the count returned.  The stack overwrites candidates already read (k <= i at every store).
__device__ int hull_lower_envelope(int* cx, int* sy, int n) {
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const int X = cx[i];
    if (X == HULL_NONE) continue;
    while (k >= 2) {
      const long long ay = sy[k - 2], ax = cx[k - 2], by = sy[k - 1], bx = cx[k - 1];
      // b is on or above the segment a -> c: it is no vertex of the lower envelope
      if ((bx - ax) * ((long long)i - ay) >= ((long long)X - ax) * (by - ay)) --k;
      else break;
    }
    sy[k] = i;
    cx[k] = X;
    ++k;
  }
  return k;
}

__device__ __forceinline__ long long hull_floor_div(long long a, long long b) {   // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// The envelope's value at index yi as the fraction num / den (den > 0): the edge j, j + 1 with sy[j] <= yi <= sy[j + 1].
__device__ __forceinline__ void hull_envelope_at(const int* cx, const int* sy, int k, int yi, long long* num, long long* den) {
  int lo = 0, hi = k - 1;              // sy[lo] <= yi < sy[hi] or yi == sy[k - 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (sy[mid] <= yi) lo = mid;
    else hi = mid;
  }
  const long long y0 = sy[lo], x0 = cx[lo], y1 = sy[hi], x1 = cx[hi];
  *den = y1 - y0;
  *num = x0 * (y1 - y0) + (x1 - x0) * ((long long)yi - y0);
}

// ext (first, last non-zero x per row) -> the hull's closed interval (xl, xr) per row, in place; xl > xr: nothing.
// Index i of a slice's candidate arrays is the doubled row coordinate Y = i - 1 (row y owns i = 2 y, 2 y + 1, 2 y + 2).
__global__ void __launch_bounds__(NT) k_hull_chain(int* ext, pp_dims d, int* scratch) {
  __shared__ int lds[4 * HULL_LDS_N];
  __shared__ int s_count[2];
  const int n = 2 * d.ny + 1;
  int* base = scratch ? scratch + (size_t)blockIdx.x * 4 * n : lds;
  int *lx = base, *ly = base + n, *rx = base + 2 * n, *ry = base + 3 * n;
  for (int z = blockIdx.x; z < d.nz; z += gridDim.x) {
    int* e = ext + (size_t)z * d.ny * 2;
    for (int i = threadIdx.x; i < n; i += NT) {
      int l = HULL_NONE, r = HULL_NONE;                 // the right side is mirrored (-X): one envelope routine serves both
      if (i & 1) {
        const int y = i >> 1;
        if (e[2 * y + 1] >= 0) {
          l = 2 * e[2 * y] - 1;
          r = -(2 * e[2 * y + 1] + 1);
        }
      } else {
        for (int y = (i >> 1) - 1; y <= (i >> 1); ++y)
          if (y >= 0 && y < d.ny && e[2 * y + 1] >= 0) {
            const int a = 2 * e[2 * y], b = -2 * e[2 * y + 1];
            if (a < l) l = a;
            if (b < r) r = b;
          }
      }
      lx[i] = l;
      rx[i] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_count[0] = hull_lower_envelope(lx, ly, n);
    if (threadIdx.x == 64) s_count[1] = hull_lower_envelope(rx, ry, n);
    __syncthreads();
    const int kl = s_count[0], kr = s_count[1];        // both 0 (empty slice) or both >= 3, with the same first and last index
    for (int y = threadIdx.x; y < d.ny; y += NT) {
      int xl = 1, xr = 0;
      const int yi = 2 * y + 1;
      if (kl >= 2 && kr >= 2 && yi >= ly[0] && yi <= ly[kl - 1]) {
        long long num, den;
        hull_envelope_at(lx, ly, kl, yi, &num, &den);
        long long v = -hull_floor_div(-num, 2 * den);    // ceil(L / 2)
        xl = v < 0 ? 0 : (int)v;
        hull_envelope_at(rx, ry, kr, yi, &num, &den);
        v = hull_floor_div(-num, 2 * den);               // floor(R / 2), R = -num / den
        xr = v > d.nx - 1 ? d.nx - 1 : (int)v;
      }
      e[2 * y] = xl;
      e[2 * y + 1] = xr;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(NT) k_hull_fill(const int* __restrict__ xlr, pp_dims d, int vec, uint8_t* __restrict__ out) {
  const unsigned nstrips = (unsigned)(d.nx + 15) / 16u;
  const size_t total = (size_t)d.ny * d.nz * nstrips;
  for (size_t c = (size_t)blockIdx.x * NT + threadIdx.x; c < total; c += (size_t)gridDim.x * NT) {
    const size_t row = c / nstrips;
    const int x0 = (int)(c - row * nstrips) * 16;
    const int xl = xlr[2 * row], xr = xlr[2 * row + 1];
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (xr >= x0 && xl <= x0 + 15) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (x0 + j >= xl && x0 + j <= xr) w[j >> 2] |= 1u << (8 * (j & 3));
    }
    uint8_t* o = out + row * d.nx + x0;
    if (vec) {
      int4 v;
      v.x = (int)w[0];
      v.y = (int)w[1];
      v.z = (int)w[2];
      v.w = (int)w[3];
      *reinterpret_cast<int4*>(o) = v;
    } else {
      const int valid = d.nx - x0 < 16 ? d.nx - x0 : 16;
      for (int j = 0; j < valid; ++j) o[j] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
  }
}

}  // namespace

extern "C" int pp_slice_convex_hull_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], uint8_t* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, mask && size && out, "pp_slice_convex_hull_u8: NULL argument");
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_slice_convex_hull_u8: empty volume");
  for (int a = 0; a < 3; ++a)
    if (size[a] > HULL_MAX_DIM) return pp_fail(ctx, PP_ERR_SIZE, "pp_slice_convex_hull_u8: an axis longer than %d", HULL_MAX_DIM);
  const pp_dims d{size[0], size[1], size[2]};
  const size_t rows = (size_t)d.ny * d.nz;
  // chains of tall slices live in scratch memory: 4 arrays of 2 ny + 1 per block, at most 64 MiB of them
  const bool in_lds = d.ny <= HULL_LDS_ROWS;
  const size_t per_block = 4 * (2 * (size_t)d.ny + 1) * sizeof(int);
  size_t chain_blocks = (size_t)d.nz;
  if (!in_lds && chain_blocks * per_block > ((size_t)64 << 20)) chain_blocks = ((size_t)64 << 20) / per_block;   // >= 32
  int rc = pp_reserve(ctx, pp_align_up(rows * 2 * sizeof(int), 256) + (in_lds ? 0 : pp_align_up(chain_blocks * per_block, 256)));
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  int* ext = cv.take<int>(rows * 2);
  int* scratch = in_lds ? nullptr : cv.take<int>(chain_blocks * per_block / sizeof(int));
  const int vec_in = (reinterpret_cast<uintptr_t>(mask) % 16 == 0 && d.nx % 16 == 0) ? 1 : 0;
  const int vec_out = (reinterpret_cast<uintptr_t>(out) % 16 == 0 && d.nx % 16 == 0) ? 1 : 0;
  const size_t nbr = (rows + HULL_WPB - 1) / HULL_WPB;
  hipLaunchKernelGGL(k_hull_extents, dim3((unsigned)(nbr < 16384 ? nbr : 16384)), dim3(NT), 0, ctx->stream, mask, d, vec_in, ext);
  PP_LAUNCH_CHECK(ctx, "k_hull_extents");
  hipLaunchKernelGGL(k_hull_chain, dim3((unsigned)chain_blocks), dim3(NT), 0, ctx->stream, ext, d, scratch);
  PP_LAUNCH_CHECK(ctx, "k_hull_chain");
  const size_t strips = rows * (size_t)((d.nx + 15) / 16);
  hipLaunchKernelGGL(k_hull_fill, dim3(grid_for(strips)), dim3(NT), 0, ctx->stream, (const int*)ext, d, vec_out, out);
  PP_LAUNCH_CHECK(ctx, "k_hull_fill");
  return PP_OK;
}
