// platipy_amd/csrc/pp_ventricle.h -- the two volume-sized steps of platipy/imaging/utils/ventricle.py: the assignment of
// the myocardium's voxels to the 17 segments (the per-slice np.where / extract loop at :408-644) and the way back into image
// space (17 sitk.Resample calls at :660-666).  #included at the end of pp_resample.hip: it uses that file's NT, pp_map_point,
// rs_affine / rs_axis, rs_inside and fill_xform.
//
// Polar sectors.  A slice of the mask is ny nx contiguous bytes: a thread takes 16-byte strips of it (one 16-byte load where
// the mask is 16-byte aligned and nx ny % 16 == 0, single bytes otherwise), skips the arithmetic of the strips that are all
// zero -- the myocardium is a shell in a cropped box, most strips are -- and walks (row, column) along the others.  A voxel's
// angle and radius about its slice's centre are formed in fp64, one rounding per operation (no contraction), in the order the
// reference writes them; every rule of the slice is then two or three comparisons.
//   count  a thread keeps the bit set of the run of voxels it is in and hands (bit set, run length) to 32 counters in LDS
//          when the set changes -- neighbours along a row nearly always lie in the same sector --; a block adds its non-zero
//          counters to counts[z][32] with 64-bit integer atomics.  Integers only: the table does not depend on the order.
//   write  a second launch on the same stream reads counts[z][32] on the device, forms the slice's mask of surviving labels
//          once per block and writes every strip of `bits`, the empty ones included, as four 16-byte stores (bits 16-byte
//          aligned and nx ny % 4 == 0; single words otherwise, and for the last strip of a slice when it is short).
// The slice and rule tables are host memory of the call: they are copied into the context's scratch and the call
// synchronises before it returns, as pp_tube_mask_u8 does for its segment list.
//
// Resample bits.  One thread per output voxel maps its point as pp_resample_u8 would for a uint8 volume on these grids --
// the same arm: rs_axis / rs_affine on two axis-aligned grids, pp_map_point otherwise --, takes rs_inside and
// floor(c + 0.5) as its nearest-neighbour arms do, loads ONE 32-bit word and stores bit k of it into plane k: a wavefront
// writes 64 consecutive bytes per plane.
#pragma once

#include <algorithm>
#include <vector>

namespace {

constexpr int PS_MAX_DIM = 65535;   // grid.x = slices
constexpr double PS_TWO_PI = 6.283185307179586476925286766559;

// bytes p[0 ... 15] as four little-endian words; with !vec only p[0 ... valid - 1] are touched, the rest are 0
__device__ __forceinline__ void ps_load16(const uint8_t* __restrict__ p, int valid, bool vec, unsigned w[4]) {
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

// the labels (bit label - 1) whose rules voxel (y, x) of a slice matches
__device__ __forceinline__ unsigned ps_voxel_bits(const pp_polar_slice& s, const pp_polar_rule* __restrict__ rules, unsigned y, unsigned x) {
#pragma clang fp contract(off)
  const double dy = (double)y - s.cy, dx = (double)x - s.cx;
  double theta = -atan2(dy, dx) - s.theta0;
  if (theta < 0.0) theta = theta + PS_TWO_PI;   // once: an angle below -2 pi stays negative (only a clockwise rule takes it)
  const double yy = dy * dy, xx = dx * dx;
  const double r = sqrt(yy + xx);
  unsigned bits = 0u;
  if (r >= s.radius_min) {
    for (int k = 0; k < s.nrules; ++k) {
      const pp_polar_rule q = rules[s.first_rule + k];
      const bool in = (q.flags & PP_POLAR_CW) ? (theta <= q.angle_min || theta >= q.angle_max) : (theta >= q.angle_min && theta <= q.angle_max);
      if (in) bits |= 1u << (q.label - 1);
    }
  }
  return bits;
}

// slice blockIdx.x, part blockIdx.y of its strips.  !WRITE: counts[z][32] += voxels per label.  WRITE: bits = the labels of
// every voxel whose (slice, label) count times `area` reaches `min_area` (or whose rule is exempt from that test).
template <bool WRITE>
__global__ void __launch_bounds__(NT) k_polar_sectors(const uint8_t* __restrict__ mask, int nx, int ny, int vec, int svec,
                                                      const pp_polar_slice* __restrict__ slices, const pp_polar_rule* __restrict__ rules,
                                                      double area, double min_area, unsigned long long* __restrict__ counts,
                                                      unsigned* __restrict__ bits) {
  __shared__ unsigned sh[32];
  const int t = threadIdx.x;
  const unsigned z = blockIdx.x;
  const pp_polar_slice s = slices[z];
  if (!WRITE && s.nrules == 0) return;   // (the same decision in every thread of the block)
  const size_t slice = (size_t)nx * ny;
  const size_t nstrips = (slice + 15) / 16;
  unsigned keep = 0u;
  if (WRITE) {
    if (s.nrules != 0) {
      if (t < 32) {
        const unsigned long long c = counts[(size_t)z * 32 + t];
        sh[t] = ((double)c * area < min_area) ? 0u : (1u << t);
      }
      __syncthreads();
      for (int k = 0; k < 32; ++k) keep |= sh[k];
      for (int k = 0; k < s.nrules; ++k) {
        const pp_polar_rule q = rules[s.first_rule + k];
        if (q.flags & PP_POLAR_ANY_AREA) keep |= 1u << (q.label - 1);
      }
    }
  } else {
    if (t < 32) sh[t] = 0u;
    __syncthreads();
  }
  const uint8_t* __restrict__ src = mask + (size_t)z * slice;
  unsigned cur = 0u, run = 0u;   // count: the bit set of the open run and its length
  for (size_t c = (size_t)blockIdx.y * NT + t; c < nstrips; c += (size_t)gridDim.y * NT) {
    const size_t i0 = c * 16;
    const int valid = slice - i0 < 16 ? (int)(slice - i0) : 16;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (s.nrules != 0) ps_load16(src + i0, valid, vec != 0, w);
    const bool empty = !(w[0] | w[1] | w[2] | w[3]);
    if (!WRITE && empty) continue;
    unsigned y = (unsigned)(i0 / (size_t)nx), x = (unsigned)(i0 % (size_t)nx);
    unsigned* __restrict__ dst = WRITE ? bits + (size_t)z * slice + i0 : nullptr;
    // four voxels at a time (not unrolled: one copy of the fp64 atan2 per voxel of the four, not sixteen)
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      const unsigned wq = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
      unsigned v[4] = {0u, 0u, 0u, 0u};
      if (wq) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if ((wq >> (8 * j)) & 0xffu) v[j] = ps_voxel_bits(s, rules, y, x);
          if (++x == (unsigned)nx) x = 0u, ++y;
        }
      } else {   // (x stays below nx: it advances by at most 4 per row wrap)
        x += 4u;
        while (x >= (unsigned)nx) x -= (unsigned)nx, ++y;
      }
      if (WRITE) {
        if (svec && valid >= 4 * q + 4) {
          int4 o;
          o.x = (int)(v[0] & keep);
          o.y = (int)(v[1] & keep);
          o.z = (int)(v[2] & keep);
          o.w = (int)(v[3] & keep);
          *reinterpret_cast<int4*>(dst + 4 * q) = o;
        } else {
          for (int j = 0; j < 4 && 4 * q + j < valid; ++j) dst[4 * q + j] = v[j] & keep;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (v[j] == cur) {
            ++run;
          } else {
            for (unsigned b = cur; b; b &= b - 1u) atomicAdd(&sh[__builtin_ctz(b)], run);
            cur = v[j];
            run = 1u;
          }
        }
      }
    }
  }
  if (!WRITE) {
    for (unsigned b = cur; b; b &= b - 1u) atomicAdd(&sh[__builtin_ctz(b)], run);
    __syncthreads();
    if (t < 32 && sh[t]) atomicAdd(&counts[(size_t)z * 32 + t], (unsigned long long)sh[t]);
  }
}

// ARM 0: any direction cosines (pp_map_point); 1: both grids axis-aligned; 2: axis-aligned with a linear transform between
template <int ARM>
__global__ void __launch_bounds__(NT) k_resample_bits(const unsigned* __restrict__ in, pp_dims din, pp_dims dout, pp_xform X, rs_axes XA,
                                                      int nbits, uint8_t* __restrict__ out) {
  const size_t N = (size_t)dout.nx * dout.ny * dout.nz;
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y, z = blockIdx.z;
  if (x >= dout.nx || y >= dout.ny) return;
  const size_t i = ((size_t)z * dout.ny + y) * dout.nx + x;
  double c[3];
  if (ARM == 0) {
    pp_map_point(X, x, y, z, 0.0, 0.0, 0.0, c);
  } else if (ARM == 2) {
    rs_affine<false>(XA, x, y, z, 0.0, 0.0, 0.0, c);
  } else {
    c[0] = rs_axis<false>(XA, 0, x, 0.0);
    c[1] = rs_axis<false>(XA, 1, y, 0.0);
    c[2] = rs_axis<false>(XA, 2, z, 0.0);
  }
  unsigned v = 0u;
  if (ARM == 0 ? pp_inside_d(c, din) : rs_inside(c, din)) {
    const int qx = (int)floor(c[0] + 0.5), qy = (int)floor(c[1] + 0.5), qz = (int)floor(c[2] + 0.5);
    v = in[((size_t)qz * din.ny + qy) * din.nx + qx];
  }
  for (int k = 0; k < nbits; ++k) out[(size_t)k * N + i] = (uint8_t)((v >> k) & 1u);
}

}  // namespace

extern "C" {

int pp_polar_sectors_u8(pp_ctx* ctx, const uint8_t* mask, const int size[3], const pp_polar_slice* slices, const pp_polar_rule* rules,
                        int nrules, double area, double min_area_mm2, uint32_t* bits, int64_t* counts) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, mask && size && slices && bits && counts, "pp_polar_sectors_u8: NULL argument");
  PP_REQUIRE(ctx, nrules >= 0 && (rules || nrules == 0), "pp_polar_sectors_u8: NULL rule table or negative rule count");
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_polar_sectors_u8: empty volume");
  if (size[0] > PS_MAX_DIM || size[1] > PS_MAX_DIM || size[2] > PS_MAX_DIM)
    return pp_fail(ctx, PP_ERR_SIZE, "pp_polar_sectors_u8: an axis longer than %d", PS_MAX_DIM);
  PP_REQUIRE(ctx, area == area && min_area_mm2 == min_area_mm2, "pp_polar_sectors_u8: the areas must not be NaN");
  const int nx = size[0], ny = size[1], nz = size[2];
  for (int k = 0; k < nrules; ++k) {
    if (rules[k].label < 1 || rules[k].label > 32)
      return pp_fail(ctx, PP_ERR_ARG, "pp_polar_sectors_u8: rule %d has label %d (1 ... 32)", k, rules[k].label);
    if ((rules[k].flags & ~(PP_POLAR_CW | PP_POLAR_ANY_AREA)) || rules[k].angle_min != rules[k].angle_min || rules[k].angle_max != rules[k].angle_max)
      return pp_fail(ctx, PP_ERR_ARG, "pp_polar_sectors_u8: rule %d has unknown flags or a NaN angle", k);
  }
  for (int z = 0; z < nz; ++z) {
    const pp_polar_slice& s = slices[z];
    if (s.nrules < 0 || (s.nrules > 0 && (s.first_rule < 0 || s.first_rule > nrules - s.nrules)))
      return pp_fail(ctx, PP_ERR_ARG, "pp_polar_sectors_u8: slice %d uses rules %d ... %d of %d", z, s.first_rule, s.first_rule + s.nrules - 1, nrules);
    if (s.nrules > 0 && !(fabs(s.cy) <= DBL_MAX && fabs(s.cx) <= DBL_MAX && fabs(s.theta0) <= DBL_MAX && s.radius_min == s.radius_min))
      return pp_fail(ctx, PP_ERR_ARG, "pp_polar_sectors_u8: slice %d has a centre or an angle that is not finite", z);
  }
  const size_t slice = (size_t)nx * ny;
  const size_t sbytes = pp_align_up((size_t)nz * sizeof(pp_polar_slice), 256), rbytes = pp_align_up((size_t)(nrules > 0 ? nrules : 1) * sizeof(pp_polar_rule), 256);
  int rc = pp_reserve(ctx, sbytes + rbytes);
  if (rc) return rc;
  pp_polar_slice* dslices = reinterpret_cast<pp_polar_slice*>(ctx->ws);
  pp_polar_rule* drules = reinterpret_cast<pp_polar_rule*>(ctx->ws + sbytes);
  PP_HIP(ctx, hipMemcpyAsync(dslices, slices, (size_t)nz * sizeof(pp_polar_slice), hipMemcpyHostToDevice, ctx->stream));
  if (nrules > 0) PP_HIP(ctx, hipMemcpyAsync(drules, rules, (size_t)nrules * sizeof(pp_polar_rule), hipMemcpyHostToDevice, ctx->stream));
  unsigned long long* dcounts = reinterpret_cast<unsigned long long*>(counts);
  PP_HIP(ctx, hipMemsetAsync(dcounts, 0, (size_t)nz * 32 * sizeof(unsigned long long), ctx->stream));
  const size_t strips = (slice + 15) / 16;
  const unsigned parts = (unsigned)std::min<size_t>((strips + (size_t)NT * 4 - 1) / ((size_t)NT * 4), 64);   // 4 strips per thread
  const int vec = reinterpret_cast<uintptr_t>(mask) % 16 == 0 && slice % 16 == 0;
  const int svec = reinterpret_cast<uintptr_t>(bits) % 16 == 0 && slice % 4 == 0;
  const dim3 grid((unsigned)nz, parts);
  hipLaunchKernelGGL(k_polar_sectors<false>, grid, dim3(NT), 0, ctx->stream, mask, nx, ny, vec, svec, (const pp_polar_slice*)dslices,
                     (const pp_polar_rule*)drules, area, min_area_mm2, dcounts, reinterpret_cast<unsigned*>(bits));
  PP_LAUNCH_CHECK(ctx, "k_polar_sectors<count>");
  hipLaunchKernelGGL(k_polar_sectors<true>, grid, dim3(NT), 0, ctx->stream, mask, nx, ny, vec, svec, (const pp_polar_slice*)dslices,
                     (const pp_polar_rule*)drules, area, min_area_mm2, dcounts, reinterpret_cast<unsigned*>(bits));
  PP_LAUNCH_CHECK(ctx, "k_polar_sectors<write>");
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the two tables above are host memory of this call)
  return PP_OK;
}

int pp_resample_bits_u32(pp_ctx* ctx, const uint32_t* in, const pp_geom* gin, const pp_geom* gout, const double* affine_A,
                         const double* affine_t, int nbits, uint8_t* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, in && out, "pp_resample_bits_u32: NULL volume");
  PP_REQUIRE(ctx, (const void*)in != (const void*)out, "pp_resample_bits_u32: in-place is not supported");
  PP_REQUIRE(ctx, nbits >= 1 && nbits <= 32, "pp_resample_bits_u32: 1 ... 32 bit planes");
  int rc = pp_geom_check(ctx, gin, "input");
  if (rc) return rc;
  rc = pp_geom_check(ctx, gout, "output");
  if (rc) return rc;
  pp_xform X;
  fill_xform(gin, gout, affine_A, affine_t, &X);
  const pp_dims din{gin->size[0], gin->size[1], gin->size[2]};
  const pp_dims dout{gout->size[0], gout->size[1], gout->size[2]};
  const pp_grid3 g3 = grid3_for(dout.nx, dout.ny, dout.nz);
  if (g3.grid.y > 65535u || g3.grid.z > 65535u) return pp_fail(ctx, PP_ERR_SIZE, "pp_resample_bits_u32: volume too large");
  const rs_axes XA = rs_axes_of(X);
  unsigned* src = const_cast<unsigned*>(reinterpret_cast<const unsigned*>(in));
  // the arm pp_resample_u8 takes for a uint8 volume on these grids (resample_any)
  if (X.axis && rs_small(din, 1) && rs_small(dout, 1) && !rs_generic_forced()) {
    if (X.has_affine)
      hipLaunchKernelGGL(k_resample_bits<2>, g3.grid, g3.block, 0, ctx->stream, (const unsigned*)src, din, dout, X, XA, nbits, out);
    else
      hipLaunchKernelGGL(k_resample_bits<1>, g3.grid, g3.block, 0, ctx->stream, (const unsigned*)src, din, dout, X, XA, nbits, out);
  } else {
    hipLaunchKernelGGL(k_resample_bits<0>, g3.grid, g3.block, 0, ctx->stream, (const unsigned*)src, din, dout, X, XA, nbits, out);
  }
  PP_LAUNCH_CHECK(ctx, "k_resample_bits");
  return PP_OK;
}

}  // extern "C"
