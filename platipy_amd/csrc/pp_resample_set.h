// platipy_amd/csrc/pp_resample_set.h -- one image and up to 16 label volumes through ONE transform in ONE gather.
//
// Included by pp_resample.hip inside its anonymous namespace, below the kernels it is built from.  apply_augmentation
// (reference generation/augment.py:65-78) and the pipelines' atlas propagation (multiatlas/run.py:280-298) warp an image
// and M structures on one grid through the same transform: 1 + M calls of k_resample(_axis) read the 12 B / voxel field and
// redo the fp64 index -> physical -> index mapping 1 + M times.  Here a thread reads the field, maps its point, takes the
// inside decision and forms the nearest-neighbour offset and the trilinear corners once, then loads from every member and
// stores every output: (12) + 4 + M bytes read and 4 + M written per voxel instead of (1 + M) 12 + 4 + M.
//
// Every member's result is bit for bit what pp_resample_f32 / pp_resample_u8 give for it alone: the point goes through the
// same pp_map_point / rs_axis / rs_affine, the decision through rs_inside, the image through rs_corners + rs_sample (axis
// arm) or pp_trilinear(_pairs) (general arm) and pp_cast_out, nearest neighbour through floor(c + 0.5).  What differs is
// control flow only: a point outside the buffer is sampled at index (0, 0, 0) and its result replaced by the default, so a
// thread's 1 + M gathers are straight-line code, all in flight together, rather than M + 1 divergent branches.
//
// The label pointers travel by value in the kernel arguments (rs_set_labels, 256 bytes; no table to upload).  Launch
// geometry is k_resample_axis': grid3_for, banded where that kernel is (a linear image through a field).
#pragma once

constexpr int RS_SET_MAX = PP_RESAMPLE_SET_MAX_LABELS;
constexpr int RS_SET_NO_IMAGE = 0;   // IMG template argument: 0, PP_INTERP_NEAREST or PP_INTERP_LINEAR

struct rs_set_labels {
  const uint8_t* in[RS_SET_MAX];
  uint8_t* out[RS_SET_MAX];
};

// the point, or (0, 0, 0) where it is outside (NaN included): every address formed from it is inside the volume
__device__ __forceinline__ void rs_set_safe(const double c[3], bool ok, double s[3]) {
  s[0] = ok ? c[0] : 0.0;
  s[1] = ok ? c[1] : 0.0;
  s[2] = ok ? c[2] : 0.0;
}

// every label's voxel at element offset q, then every output at element offset i (loads first: the label volumes and
// the outputs are not known to be distinct to the compiler, and a store between two loads would order them)
template <typename OFF>
__device__ __forceinline__ void rs_set_labels_gather(const rs_set_labels& L, int nlabels, bool ok, OFF q, OFF i) {
  uint8_t v[RS_SET_MAX];
#pragma unroll
  for (int l = 0; l < RS_SET_MAX; ++l)
    if (l < nlabels) v[l] = L.in[l][q];
#pragma unroll
  for (int l = 0; l < RS_SET_MAX; ++l)
    if (l < nlabels) L.out[l][i] = ok ? v[l] : (uint8_t)0;
}

// k_resample_axis for the set: both grids axis-aligned, every volume below 2^32 bytes
template <int IMG, bool HASFIELD, bool WIDE, bool AFFINE>
__global__ void __launch_bounds__(NT) k_resample_set_axis(const float* __restrict__ image, pp_dims din, const float* __restrict__ field,
                                                          float* __restrict__ image_out, pp_dims dout, rs_axes X, float default_value,
                                                          rs_set_labels L, int nlabels, pp_band B) {
  unsigned bx_, by_, bz_;
  if (!pp_band_block(B, bx_, by_, bz_)) return;
  const int x = bx_ * blockDim.x + threadIdx.x, y = by_ * blockDim.y + threadIdx.y, z = bz_;
  if (x >= dout.nx || y >= dout.ny) return;
  const unsigned N4 = (unsigned)dout.nx * (unsigned)dout.ny * (unsigned)dout.nz * 4u;
  const unsigned i = ((unsigned)z * (unsigned)dout.ny + (unsigned)y) * (unsigned)dout.nx + (unsigned)x;
  double ddx = 0.0, ddy = 0.0, ddz = 0.0;
  if (HASFIELD) {
    ddx = (double)rs_ld(field, i * 4u);
    ddy = (double)rs_ld(field, N4 + i * 4u);
    ddz = (double)rs_ld(field, 2u * N4 + i * 4u);
  }
  double c[3], s[3];
  if (AFFINE) {
    rs_affine<HASFIELD>(X, x, y, z, ddx, ddy, ddz, c);
  } else {
    c[0] = rs_axis<HASFIELD>(X, 0, x, ddx);
    c[1] = rs_axis<HASFIELD>(X, 1, y, ddy);
    c[2] = rs_axis<HASFIELD>(X, 2, z, ddz);
  }
  const bool ok = rs_inside(c, din);
  rs_set_safe(c, ok, s);
  const int qx = (int)floor(s[0] + 0.5), qy = (int)floor(s[1] + 0.5), qz = (int)floor(s[2] + 0.5);
  const unsigned q = ((unsigned)qz * (unsigned)din.ny + (unsigned)qy) * (unsigned)din.nx + (unsigned)qx;
  float res = 0.0f;
  if (IMG == PP_INTERP_NEAREST) {
    res = rs_ld(image, q * 4u);
  } else if (IMG == PP_INTERP_LINEAR) {
    const double flx = floor(s[0]), fly = floor(s[1]), flz = floor(s[2]);
    rs_corner a;
    rs_corners(din, (int)flx, (float)(s[0] - flx), (int)fly, (float)(s[1] - fly), (int)flz, (float)(s[2] - flz), a);
    res = pp_cast_out<float>(rs_sample<WIDE>(image, a));
  }
  rs_set_labels_gather<unsigned>(L, nlabels, ok, q, i);
  if (IMG != RS_SET_NO_IMAGE) rs_st(image_out, i * 4u, ok ? res : default_value);
}

// k_resample for the set: any direction cosines, any size
template <int IMG, bool HASFIELD>
__global__ void __launch_bounds__(NT) k_resample_set(const float* __restrict__ image, pp_dims din, const float* __restrict__ field,
                                                     float* __restrict__ image_out, pp_dims dout, pp_xform X, float default_value,
                                                     rs_set_labels L, int nlabels) {
  const size_t N = (size_t)dout.nx * dout.ny * dout.nz;
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y, z = blockIdx.z;
  if (x >= dout.nx || y >= dout.ny) return;
  const size_t i = ((size_t)z * dout.ny + y) * dout.nx + x;
  double ddx = 0.0, ddy = 0.0, ddz = 0.0;
  if (HASFIELD) {
    ddx = (double)field[i];
    ddy = (double)field[N + i];
    ddz = (double)field[2 * N + i];
  }
  double c[3], s[3];
  pp_map_point(X, x, y, z, ddx, ddy, ddz, c);
  const bool ok = rs_inside(c, din);
  rs_set_safe(c, ok, s);
  const int qx = (int)floor(s[0] + 0.5), qy = (int)floor(s[1] + 0.5), qz = (int)floor(s[2] + 0.5);
  const size_t q = ((size_t)qz * din.ny + qy) * din.nx + qx;
  float res = 0.0f;
  if (IMG == PP_INTERP_NEAREST) {
    res = image[q];
  } else if (IMG == PP_INTERP_LINEAR) {
    const double flx = floor(s[0]), fly = floor(s[1]), flz = floor(s[2]);
    res = pp_cast_out<float>(din.nx >= 2 ? pp_trilinear_pairs(image, din.nx, din.ny, din.nz, (int)flx, (float)(s[0] - flx), (int)fly,
                                                              (float)(s[1] - fly), (int)flz, (float)(s[2] - flz))
                                         : pp_trilinear(image, din.nx, din.ny, din.nz, (int)flx, (float)(s[0] - flx), (int)fly,
                                                        (float)(s[1] - fly), (int)flz, (float)(s[2] - flz)));
  }
  rs_set_labels_gather<size_t>(L, nlabels, ok, q, i);
  if (IMG != RS_SET_NO_IMAGE) image_out[i] = ok ? res : default_value;
}

// The arm is chosen as resample_any chooses it for a fp32 member (the two arms give the same bits: tests/test_kernels.py,
// tests/test_resample_set.py).
int resample_set_launch(pp_ctx* ctx, const pp_geom* gin, const pp_geom* gout, const double* A, const double* t, const float* field,
                        const float* image, int interp, double default_value, float* image_out, const rs_set_labels& L, int nlabels) {
  pp_xform X;
  fill_xform(gin, gout, A, t, &X);
  const pp_dims din{gin->size[0], gin->size[1], gin->size[2]};
  const pp_dims dout{gout->size[0], gout->size[1], gout->size[2]};
  const pp_grid3 g3 = grid3_for(dout.nx, dout.ny, dout.nz);
  const int img = image ? interp : RS_SET_NO_IMAGE;
  const float dv = (float)default_value;
  if (X.axis && rs_small(din, 4) && rs_small(dout, field ? 12 : 4) && !rs_generic_forced()) {
    const rs_axes XA = rs_axes_of(X);
    dim3 launch;
    const pp_band B = band_for(g3, &launch, field != nullptr && img == PP_INTERP_LINEAR);
#define PP_RSS3(I, F, W, AF) hipLaunchKernelGGL((k_resample_set_axis<I, F, W, AF>), launch, g3.block, 0, ctx->stream, image, din, field, \
                                                image_out, dout, XA, dv, L, nlabels, B)
#define PP_RSS2(I, F, W) do { if (X.has_affine) PP_RSS3(I, F, W, true); else PP_RSS3(I, F, W, false); } while (0)
#define PP_RSS(I, W) do { if (field) PP_RSS2(I, true, W); else PP_RSS2(I, false, W); } while (0)
    if (img == RS_SET_NO_IMAGE) PP_RSS(RS_SET_NO_IMAGE, true);
    else if (img == PP_INTERP_NEAREST) PP_RSS(PP_INTERP_NEAREST, true);
    else if (din.nx >= 2) PP_RSS(PP_INTERP_LINEAR, true);
    else PP_RSS(PP_INTERP_LINEAR, false);
#undef PP_RSS
#undef PP_RSS2
#undef PP_RSS3
    PP_LAUNCH_CHECK(ctx, "k_resample_set_axis");
    return PP_OK;
  }
#define PP_RSG2(I, F) hipLaunchKernelGGL((k_resample_set<I, F>), g3.grid, g3.block, 0, ctx->stream, image, din, field, image_out, dout, X, \
                                         dv, L, nlabels)
#define PP_RSG(I) do { if (field) PP_RSG2(I, true); else PP_RSG2(I, false); } while (0)
  if (img == RS_SET_NO_IMAGE) PP_RSG(RS_SET_NO_IMAGE);
  else if (img == PP_INTERP_NEAREST) PP_RSG(PP_INTERP_NEAREST);
  else PP_RSG(PP_INTERP_LINEAR);
#undef PP_RSG
#undef PP_RSG2
  PP_LAUNCH_CHECK(ctx, "k_resample_set");
  return PP_OK;
}
