// platipy_amd/csrc/pp_vessel.h -- the two volume-sized steps of platipy/imaging/utils/vessel.py: the per-slice moments behind
// com_from_image_list (:33-167; also get_com, label/utils.py:61-84) and the voxelisation of a tube of fixed radius around a
// centreline (what vtkTubeFilter + vtkPolyDataToImageStencil do at :170-296).  #included at the end of pp_fusion.hip (it uses
// that file's NT).
//
// Slice moments.  out[m][s] = {sum v, sum a v, sum b v, count(v != 0)} over slice s of mask m, v the voxel's own value, all
// in integers: 32-bit partial sums in registers, 64-bit integer atomics in LDS, then 64-bit integer atomics in global
// memory -- sums of integers do not depend on their order, so the table equals numpy's and a rerun gives the same bits.
//   z-scan  a slice is ny nx contiguous bytes: a thread takes 16-byte strips of it, skips the strips that are all zero (most
//           of a propagated label) and walks (row, column) along the others; a block reduces its four sums in LDS.
//   x-scan  slice s is the column x = s, a stride-nx read.  Instead the lanes of a wavefront lie ALONG x -- lane l loads the
//           16 bytes x = 16 l ... 16 l + 15 of a row, so a wavefront reads 1 KB of consecutive memory (the rows that follow when nx
//           < 1024) -- and every thread keeps the 4 x 16 partial sums of its sixteen x-slices in registers while it walks down
//           XS_ROWS rows.  Threads that share x (the other rows of the block) meet in an LDS table laid out [sum][x] so that
//           neighbouring lanes hit neighbouring banks; one global atomic per non-zero entry and block.
//           32-bit partials: XS_ROWS * 255 * 65535 < 2^32 (every axis <= 65535 is checked).
// 16-byte loads need a 16-byte aligned mask and nx % 16 == 0 (z-scan: nx ny % 16 == 0); otherwise the same code assembles
// the strip from single bytes, zero beyond the row's end.
//
// Tube mask.  A voxel is inside when, for some segment k of the polyline, the distance from its centre to the closest
// point of the segment is <= radius; the two ends are flat (vtkTubeFilter does not cap): on the first segment only points
// whose unclamped projection parameter is >= 0 count, on the last only <= 1.  Decided in fp64.
// Brute force is voxels x segments (67 M x 5 000 at the workload's size), so a workgroup owns a BRICK of 16 x 16 x 4 voxels
// and first finds the segments that can reach it: thread t tests segment base + t against the sphere around the brick's
// voxel centres (distance to the clamped segment <= radius + brick radius, in fp64 with a relative and an absolute
// slack, so it can only keep too many) and appends the survivors to a list in LDS; then each thread runs its four voxels
// over that list only.  When the list could overflow (TB_CAP - NT entries held) the voxels are run over what is there and the
// list restarts: any number of segments works, nothing is truncated; the result is an OR, so neither the order of the list
// nor the chunking changes a bit.  Bricks outside the polyline's bounding box grown by the radius skip the scan.
//   Why 16 x 16 x 4 and 256 threads: CT grids here are 2 - 3 times coarser in z than in plane, so this brick is close to a
//   cube in mm and its bounding sphere (12.4 mm at 1 x 1 x 2.5) is the smallest of the 1024-voxel shapes with 16-byte rows
//   (32 x 8 x 4: 17.2 mm, 64 x 4 x 4: 32.5 mm) -- the sphere's radius is what the cull pays for.  A row of the brick is one
//   16-byte store, what an empty brick is written with (64 lanes, one per row); a wavefront of a brick near the tube owns one
//   z-layer and writes 4 bytes per lane, 16 consecutive bytes per four lanes.  The list holds whole segments (64 B each,
//   read back as LDS broadcasts, no global traffic in the voxel loop): TB_CAP = 512 -> 32 KB per workgroup, five workgroups
//   = 20 wavefronts per CU beside the 160 KB of LDS, more than the fp64 loop's registers allow anyway.
#pragma once

#include <vector>

namespace {

// ---------------------------------------------------------------------------------------
// slice moments

constexpr int SM_MAX_MASKS = 64;
constexpr int SM_MAX_DIM = 65535;   // 32-bit partial sums of the x-scan; grid.y
constexpr int XS_ROWS = 64;         // rows a thread of the x-scan walks
constexpr int XS_TX = 64;           // 16-byte strips of one row a block covers at most

struct sm_args {
  const uint8_t* m[SM_MAX_MASKS];
};

// Bytes p[0 ... 15] as four little-endian words; with !vec only p[0 ... valid - 1] are touched, the rest are 0.
__device__ __forceinline__ void sm_load16(const uint8_t* __restrict__ p, int valid, bool vec, unsigned w[4]) {
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

// out[mask][z][4] += the moments of slice z = blockIdx.x of mask blockIdx.z (part blockIdx.y of it); a = row (y), b = column (x).
__global__ void __launch_bounds__(NT) k_slice_moments_z(sm_args a, int nx, int ny, int vec, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh[4];
  const int t = threadIdx.x;
  if (t < 4) sh[t] = 0ull;
  __syncthreads();
  const size_t slice = (size_t)nx * ny;
  const uint8_t* __restrict__ src = a.m[blockIdx.z] + (size_t)blockIdx.x * slice;
  const size_t nstrips = (slice + 15) / 16;
  unsigned long long s0 = 0ull, s1 = 0ull, s2 = 0ull, s3 = 0ull;
  for (size_t c = (size_t)blockIdx.y * NT + t; c < nstrips; c += (size_t)gridDim.y * NT) {
    const size_t i0 = c * 16;
    const int valid = slice - i0 < 16 ? (int)(slice - i0) : 16;
    unsigned w[4];
    sm_load16(src + i0, valid, vec != 0, w);
    if (!(w[0] | w[1] | w[2] | w[3])) continue;
    unsigned y = (unsigned)(i0 / (size_t)nx), x = (unsigned)(i0 % (size_t)nx);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned v = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
      s0 += v;
      s1 += (unsigned long long)(y * v);   // y, x < 2^16 (checked), v < 2^8
      s2 += (unsigned long long)(x * v);
      s3 += v ? 1u : 0u;
      if (++x == (unsigned)nx) x = 0u, ++y;
    }
  }
  if (s3) {
    atomicAdd(&sh[0], s0);
    atomicAdd(&sh[1], s1);
    atomicAdd(&sh[2], s2);
    atomicAdd(&sh[3], s3);
  }
  __syncthreads();
  if (t < 4 && sh[t]) atomicAdd(&out[((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 4 + t], sh[t]);
}

// out[mask][x][4] += the moments of the rows blockIdx.x * rows_per_block ... (strips blockIdx.y * tx_count ...) of mask blockIdx.z; a = array z, b = array y.
// tx_count (a power of two <= XS_TX) lanes lie along x, NT / tx_count rows are in flight at once.
__global__ void __launch_bounds__(NT) k_slice_moments_x(sm_args a, int nx, int ny, int nz, int vec, int tx_count,
                                                        unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh[4 * 16 * XS_TX];   // [sum][x within the strip][strip]: 32 KB
  const int t = threadIdx.x;
  const int tx = t & (tx_count - 1), ty = t / tx_count, ty_count = NT / tx_count;
  for (int i = t; i < 4 * 16 * XS_TX; i += NT) sh[i] = 0ull;
  __syncthreads();
  const int x0 = (blockIdx.y * tx_count + tx) * 16;
  const unsigned rows = (unsigned)ny * (unsigned)nz;   // < 2^31 (checked)
  const uint8_t* __restrict__ src = a.m[blockIdx.z];
  if (x0 < nx) {
    const int valid = nx - x0 < 16 ? nx - x0 : 16;
    unsigned sv[16], sz[16], sy[16], sc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) sv[j] = sz[j] = sy[j] = sc[j] = 0u;
    const unsigned r0 = blockIdx.x * (unsigned)(ty_count * XS_ROWS) + ty;
    unsigned any = 0u;
    for (int k = 0; k < XS_ROWS; ++k) {
      const unsigned r = r0 + (unsigned)(k * ty_count);
      if (r >= rows) break;
      unsigned w[4];
      sm_load16(src + (size_t)r * nx + x0, valid, vec != 0, w);
      if (!(w[0] | w[1] | w[2] | w[3])) continue;
      any = 1u;
      const unsigned z = r / (unsigned)ny, y = r % (unsigned)ny;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned v = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        sv[j] += v;
        sz[j] += z * v;
        sy[j] += y * v;
        sc[j] += v ? 1u : 0u;
      }
    }
    if (any) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (sc[j]) {
          atomicAdd(&sh[(0 * 16 + j) * XS_TX + tx], (unsigned long long)sv[j]);
          atomicAdd(&sh[(1 * 16 + j) * XS_TX + tx], (unsigned long long)sz[j]);
          atomicAdd(&sh[(2 * 16 + j) * XS_TX + tx], (unsigned long long)sy[j]);
          atomicAdd(&sh[(3 * 16 + j) * XS_TX + tx], (unsigned long long)sc[j]);
        }
    }
  }
  __syncthreads();
  for (int i = t; i < 4 * 16 * tx_count; i += NT) {
    const int ltx = i & (tx_count - 1), j = (i / tx_count) & 15, q = i / (tx_count * 16);
    const unsigned long long s = sh[(q * 16 + j) * XS_TX + ltx];
    const int x = (blockIdx.y * tx_count + ltx) * 16 + j;
    if (s && x < nx) atomicAdd(&out[((size_t)blockIdx.z * nx + x) * 4 + q], s);
  }
}

// ---------------------------------------------------------------------------------------
// tube mask

constexpr int TB_BX = 16, TB_BY = 16, TB_BZ = 4;   // the brick (voxels); TB_BX * TB_BY * TB_BZ = 4 NT
constexpr int TB_CAP = 512;                        // segments of the LDS list

struct alignas(16) tb_seg {   // 64 B
  double a[3];     // first point (mm)
  double d[3];     // second - first
  double l2;       // |d|^2 > 0
  unsigned flags;  // 1: the polyline's first segment (projection parameter >= 0 only), 2: its last (<= 1 only)
  unsigned pad;
};

struct tb_args {
  int nx, ny, nz, nseg;
  double sp[3], org[3];
  double radius, r2;
  double slack;            // absolute slack of the cull (mm)
  double lo[3], hi[3];     // the polyline's bounding box grown by radius + slack
  int vec16, vec4;         // out and nx allow aligned 16- / 4-byte stores
};

// squared distance from p to the closest point of segment s; dot = (p - a) . d
__device__ __forceinline__ double tb_dist2(const tb_seg& s, double px, double py, double pz, double& dot) {
  const double ux = px - s.a[0], uy = py - s.a[1], uz = pz - s.a[2];
  dot = ux * s.d[0] + uy * s.d[1] + uz * s.d[2];
  double tt = dot / s.l2;
  tt = tt < 0.0 ? 0.0 : (tt > 1.0 ? 1.0 : tt);
  const double qx = ux - tt * s.d[0], qy = uy - tt * s.d[1], qz = uz - tt * s.d[2];
  return qx * qx + qy * qy + qz * qz;
}

// OR into `marks` (bit j = voxel j of the thread's four) every voxel within the radius of one of list[0 ... n); bits of
// `done` are voxels that need no test (marked already, or outside the volume).
__device__ __forceinline__ void tb_voxels(const tb_seg* list, int n, const double cx[4], double cy, double cz, double r2, unsigned& marks,
                                          unsigned outside) {
  for (int i = 0; i < n; ++i) {
    if ((marks | outside) == 0xfu) return;
    const tb_seg s = list[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((marks | outside) >> j & 1u) continue;
      double dot;
      const double d2 = tb_dist2(s, cx[j], cy, cz, dot);
      const bool ends = (!(s.flags & 1u) || dot >= 0.0) && (!(s.flags & 2u) || dot <= s.l2);
      if (ends && d2 <= r2) marks |= 1u << j;
    }
  }
}

__global__ void __launch_bounds__(NT) k_tube_mask(const tb_seg* __restrict__ segs, tb_args a, uint8_t* __restrict__ out) {
  __shared__ tb_seg sh_seg[TB_CAP];
  __shared__ int sh_n;
  const int t = threadIdx.x;
  const int bx0 = blockIdx.x * TB_BX, by0 = blockIdx.y * TB_BY, bz0 = blockIdx.z * TB_BZ;
  // the brick's voxel centres inside the volume: an axis-aligned box
  const int bx1 = (bx0 + TB_BX < a.nx ? bx0 + TB_BX : a.nx) - 1, by1 = (by0 + TB_BY < a.ny ? by0 + TB_BY : a.ny) - 1;
  const int bz1 = (bz0 + TB_BZ < a.nz ? bz0 + TB_BZ : a.nz) - 1;
  const double lo[3] = {a.org[0] + bx0 * a.sp[0], a.org[1] + by0 * a.sp[1], a.org[2] + bz0 * a.sp[2]};
  const double hi[3] = {a.org[0] + bx1 * a.sp[0], a.org[1] + by1 * a.sp[1], a.org[2] + bz1 * a.sp[2]};
  const bool near = lo[0] <= a.hi[0] && hi[0] >= a.lo[0] && lo[1] <= a.hi[1] && hi[1] >= a.lo[1] && lo[2] <= a.hi[2] && hi[2] >= a.lo[2];
  if (!near) {   // (the same decision in every thread of the block)
    if (a.vec16) {   // nx % 16 == 0: the brick is whole in x and every row of it is one aligned 16-byte store
      if (t < TB_BY * TB_BZ) {
        const int y = by0 + (t & (TB_BY - 1)), z = bz0 + t / TB_BY;
        int4 zero;
        zero.x = zero.y = zero.z = zero.w = 0;
        if (y < a.ny && z < a.nz) *reinterpret_cast<int4*>(out + ((size_t)z * a.ny + y) * a.nx + bx0) = zero;
      }
      return;
    }
  }
  const int x = bx0 + 4 * (t & 3), y = by0 + ((t >> 2) & (TB_BY - 1)), z = bz0 + (t >> 6);
  unsigned marks = 0u;
  if (near) {
    unsigned outside = 0u;
    for (int j = 0; j < 4; ++j)
      if (x + j >= a.nx || y >= a.ny || z >= a.nz) outside |= 1u << j;
    double cx[4];
    for (int j = 0; j < 4; ++j) cx[j] = a.org[0] + (x + j) * a.sp[0];
    const double cy = a.org[1] + y * a.sp[1], cz = a.org[2] + z * a.sp[2];
    // bounding sphere of the box; a segment further from its centre than radius + sphere radius reaches no voxel of the brick
    const double mx = 0.5 * (lo[0] + hi[0]), my = 0.5 * (lo[1] + hi[1]), mz = 0.5 * (lo[2] + hi[2]);
    const double ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
    const double reach = (a.radius + 0.5 * sqrt(ex * ex + ey * ey + ez * ez)) * (1.0 + 1e-9) + a.slack;
    const double reach2 = reach * reach;
    if (t == 0) sh_n = 0;
    for (int base = 0; base < a.nseg; base += NT) {
      __syncthreads();
      const int n = sh_n;
      __syncthreads();
      if (n > TB_CAP - NT) {   // the next NT candidates might not fit: use the list and start it again
        tb_voxels(sh_seg, n, cx, cy, cz, a.r2, marks, outside);
        __syncthreads();
        if (t == 0) sh_n = 0;
        __syncthreads();
      }
      const int k = base + t;
      if (k < a.nseg) {
        const tb_seg s = segs[k];
        double dot;
        if (tb_dist2(s, mx, my, mz, dot) <= reach2) sh_seg[atomicAdd(&sh_n, 1)] = s;
      }
    }
    __syncthreads();
    tb_voxels(sh_seg, sh_n, cx, cy, cz, a.r2, marks, outside);
  }
  if (y >= a.ny || z >= a.nz || x >= a.nx) return;
  uint8_t* __restrict__ row = out + ((size_t)z * a.ny + y) * a.nx + x;
  if (a.vec4) {   // nx % 4 == 0: the four voxels are inside together
    *reinterpret_cast<unsigned*>(row) = (marks & 1u) | ((marks >> 1 & 1u) << 8) | ((marks >> 2 & 1u) << 16) | ((marks >> 3 & 1u) << 24);
  } else {
    for (int j = 0; j < 4 && x + j < a.nx; ++j) row[j] = (uint8_t)(marks >> j & 1u);
  }
}

}  // namespace

extern "C" {

int pp_slice_moments_u8(pp_ctx* ctx, const uint8_t* const* masks, int nmasks, const int size[3], int axis, int64_t* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, masks && size && out, "pp_slice_moments_u8: NULL argument");
  PP_REQUIRE(ctx, axis == 0 || axis == 2, "pp_slice_moments_u8: the scan axis is 0 (x) or 2 (z)");
  if (nmasks < 1 || nmasks > SM_MAX_MASKS) return pp_fail(ctx, PP_ERR_ARG, "pp_slice_moments_u8: %d masks (1 ... %d)", nmasks, SM_MAX_MASKS);
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_slice_moments_u8: empty volume");
  if (size[0] > SM_MAX_DIM || size[1] > SM_MAX_DIM || size[2] > SM_MAX_DIM || pp_nvox(size) >= 0x7fffffffu)
    return pp_fail(ctx, PP_ERR_SIZE, "pp_slice_moments_u8: an axis longer than %d or a volume of 2^31 voxels or more", SM_MAX_DIM);
  const int nx = size[0], ny = size[1], nz = size[2];
  sm_args a;
  bool aligned = true;
  for (int m = 0; m < SM_MAX_MASKS; ++m) {
    a.m[m] = m < nmasks ? masks[m] : nullptr;
    if (m < nmasks && !masks[m]) return pp_fail(ctx, PP_ERR_ARG, "pp_slice_moments_u8: NULL mask");
    if (reinterpret_cast<uintptr_t>(a.m[m]) % 16) aligned = false;
  }
  const int nslices = axis == 0 ? nx : nz;
  unsigned long long* dout = reinterpret_cast<unsigned long long*>(out);
  PP_HIP(ctx, hipMemsetAsync(dout, 0, (size_t)nmasks * nslices * 4 * sizeof(unsigned long long), ctx->stream));
  if (axis == 2) {
    const size_t slice = (size_t)nx * ny;
    const size_t strips = (slice + 15) / 16;
    const unsigned parts = (unsigned)std::min<size_t>((strips + (size_t)NT * 8 - 1) / ((size_t)NT * 8), 64);   // 8 strips per thread
    hipLaunchKernelGGL(k_slice_moments_z, dim3((unsigned)nz, parts, (unsigned)nmasks), dim3(NT), 0, ctx->stream, a, nx, ny,
                       (int)(aligned && slice % 16 == 0), dout);
    PP_LAUNCH_CHECK(ctx, "k_slice_moments_z");
  } else {
    const int strips = (nx + 15) / 16;
    int tx = 1;
    while (tx < strips && tx < XS_TX) tx *= 2;
    const int rows_per_block = NT / tx * XS_ROWS;
    const unsigned gy = (unsigned)(((size_t)ny * nz + rows_per_block - 1) / rows_per_block);
    hipLaunchKernelGGL(k_slice_moments_x, dim3(gy, (unsigned)((strips + tx - 1) / tx), (unsigned)nmasks), dim3(NT), 0, ctx->stream, a, nx, ny,
                       nz, (int)(aligned && nx % 16 == 0), tx, dout);
    PP_LAUNCH_CHECK(ctx, "k_slice_moments_x");
  }
  return PP_OK;
}

int pp_tube_mask_u8(pp_ctx* ctx, const double* points, int npoints, const int size[3], const double spacing[3], const double origin[3],
                    double radius, uint8_t* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, points && size && spacing && origin && out, "pp_tube_mask_u8: NULL argument");
  PP_REQUIRE(ctx, npoints >= 2, "pp_tube_mask_u8: a polyline has at least two points");
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_tube_mask_u8: empty volume");
  PP_REQUIRE(ctx, radius >= 0.0 && radius <= DBL_MAX, "pp_tube_mask_u8: the radius must be finite and not negative");
  if ((size[2] + TB_BZ - 1) / TB_BZ > 65535 || (size[1] + TB_BY - 1) / TB_BY > 65535)
    return pp_fail(ctx, PP_ERR_SIZE, "pp_tube_mask_u8: volume too large");
  tb_args a;
  a.nx = size[0], a.ny = size[1], a.nz = size[2];
  double scale = 1.0;
  for (int c = 0; c < 3; ++c) {
    PP_REQUIRE(ctx, spacing[c] > 0.0 && spacing[c] <= DBL_MAX && fabs(origin[c]) <= DBL_MAX, "pp_tube_mask_u8: spacing must be positive, origin finite");
    a.sp[c] = spacing[c];
    a.org[c] = origin[c];
    a.lo[c] = DBL_MAX;
    a.hi[c] = -DBL_MAX;
    scale = std::max(scale, std::max(fabs(origin[c]), fabs(origin[c] + (size[c] - 1) * spacing[c])));
  }
  for (int i = 0; i < 3 * npoints; ++i) {
    PP_REQUIRE(ctx, fabs(points[i]) <= DBL_MAX, "pp_tube_mask_u8: a point is not finite");
    scale = std::max(scale, fabs(points[i]));
  }
  // the segments of non-zero length; the flat ends belong to the first and the last of THOSE
  std::vector<tb_seg> segs;
  segs.reserve((size_t)npoints - 1);
  for (int k = 0; k + 1 < npoints; ++k) {
    tb_seg s;
    s.l2 = 0.0;
    for (int c = 0; c < 3; ++c) {
      s.a[c] = points[3 * k + c];
      s.d[c] = points[3 * k + 3 + c] - s.a[c];
      s.l2 += s.d[c] * s.d[c];
    }
    s.flags = s.pad = 0u;
    if (!(s.l2 > 0.0)) continue;
    PP_REQUIRE(ctx, s.l2 <= DBL_MAX, "pp_tube_mask_u8: a segment is too long");
    segs.push_back(s);
    for (int c = 0; c < 3; ++c) {
      a.lo[c] = std::min(a.lo[c], std::min(s.a[c], s.a[c] + s.d[c]));
      a.hi[c] = std::max(a.hi[c], std::max(s.a[c], s.a[c] + s.d[c]));
    }
  }
  PP_REQUIRE(ctx, !segs.empty(), "pp_tube_mask_u8: every segment of the polyline has zero length");
  segs.front().flags |= 1u;
  segs.back().flags |= 2u;
  a.nseg = (int)segs.size();
  a.radius = radius;
  a.r2 = radius * radius;
  a.slack = 1e-9 * scale;
  for (int c = 0; c < 3; ++c) {
    a.lo[c] -= radius * (1.0 + 1e-9) + a.slack;
    a.hi[c] += radius * (1.0 + 1e-9) + a.slack;
  }
  const bool aligned16 = reinterpret_cast<uintptr_t>(out) % 16 == 0, aligned4 = reinterpret_cast<uintptr_t>(out) % 4 == 0;
  a.vec16 = aligned16 && a.nx % 16 == 0;
  a.vec4 = aligned4 && a.nx % 4 == 0;
  int rc = pp_reserve(ctx, pp_align_up(segs.size() * sizeof(tb_seg), 256));
  if (rc) return rc;
  tb_seg* dsegs = reinterpret_cast<tb_seg*>(ctx->ws);
  PP_HIP(ctx, hipMemcpyAsync(dsegs, segs.data(), segs.size() * sizeof(tb_seg), hipMemcpyHostToDevice, ctx->stream));
  const dim3 grid((unsigned)((a.nx + TB_BX - 1) / TB_BX), (unsigned)((a.ny + TB_BY - 1) / TB_BY), (unsigned)((a.nz + TB_BZ - 1) / TB_BZ));
  hipLaunchKernelGGL(k_tube_mask, grid, dim3(NT), 0, ctx->stream, (const tb_seg*)dsegs, a, out);
  PP_LAUNCH_CHECK(ctx, "k_tube_mask");
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the segment list above is host memory of this call)
  return PP_OK;
}

}  // extern "C"
