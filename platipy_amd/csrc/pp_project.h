// platipy_amd/csrc/pp_project.h -- rotated volume projections: project_onto_arbitrary_plane (reference
// visualisation/utils.py:305-368) for every view, the image and its contours in ONE launch.
//
// #included at the end of pp_resample.hip: it uses that file's pp_xform / fill_xform / pp_map_point / pp_inside_d /
// pp_cast_out and the trilinear samplers of pp_internal.h.  The reference rotates the volume about its centre, resamples
// it onto its own grid (sitk.Resample) and reduces the result along an axis (sitk.*Projection); composed from this
// library's pieces that is pp_resample_f32 + a reduction: 4 B read, 4 B written, 4 B read again per voxel and view for one
// plane of output.  Here a thread owns a RAY -- one output pixel of one view -- and walks the ray's samples in index order:
// every sample is the voxel pp_resample_f32 / pp_resample_u8 would have written for that member, transform and output
// index with gout = gin, bit for bit (pp_map_point per sample in fp64, never an incremental step; pp_inside_d; the same
// nearest / trilinear functions; pp_cast_out; the default outside, which takes part in the reduction as it does in the
// reference).  The point is mapped and the inside test taken once per sample for the image and all labels.  Compulsory
// traffic per voxel and view: 4 B of image + 1 B per label read; one fp32 plane + one uint8 plane per label written.
//
// Threads to rays.  A block is one wavefront of PJ_RAYS = 64 rays whose pixels are neighbours along the output's fastest
// axis, so the stores coalesce.  A lane does NOT walk its own ray through memory: turned by pi / 2, 64 lanes would sit on 64
// rows of the input, touch one cache line per lane and member every step and want each line again for the next 32 (fp32)
// or 128 (uint8) steps -- 64 lines per member held in L1 by every wavefront of the CU at once.  Instead the wavefront takes
// a tile of 64 rays x PJ_TS = 16 samples at a time: in the sampling phase every step gathers one compact PATCH of the
// tile, 16 steps for the tile, and parks the samples in LDS; after a barrier lane r consumes row r of the tile in index
// order.  Same samples, same order of reduction.  The patch is chosen per projection axis so that at zero rotation its
// lanes read neighbouring addresses:
//   * axis 0 (rays along x): 4 rays x 16 consecutive samples a step -- four row segments of 64 B;
//   * axis 1 (rays along y) and axis 2 (rays along z): 16 consecutive rays (x) x 4 samples a step -- four row segments of 64 B.
// Whatever the rotation a step touches a 16 x 4 patch of the input and the next step of the same rays the patch beside it.
// LDS: 64 x 17 floats + 64 x 20 bytes per label (NLCAP = 0, 4, 8 or 16 labels: 4.3 / 9.4 / 14.5 / 24.8 KB a block).
//
// Reductions [ITK-upstream, UNPINNED: itk::ProjectionImageFilter's accumulators as recalled; SimpleITK is absent].
//   min, max  of the samples; a NaN sample makes the result NaN (numpy's rule, the restatement's; ITK's comparisons would
//             skip it).
//   sum       the fp64 sum of the samples in index order; mean: that sum / n; both rounded once to fp32.
//   std       sqrt(sum((v - mean)^2) / (n - 1)): a second walk of the ray, fp64, index order; n = 1 gives 0 / 0 = NaN.
//   median    the element at index n / 2 of the sorted samples (std::nth_element: the upper median, no averaging), NaN
//             sorted last whatever its sign bit (numpy's rule); the result is a canonical quiet NaN then.
//   labels    max.
// Nothing is atomic and every output word is written by one thread: reruns are bit-identical.
//
// The median is the one reduction that needs a ray's samples together.  It is a radix SELECT that re-samples the ray: the
// samples' order-preserving 32-bit keys are narrowed four bits a walk, eight walks after the first, each counting the 16
// digits below the prefix fixed so far in registers.  There is NO staging chunk: nothing is kept between walks but the
// prefix and the remaining rank, so it is exact for any ray length the entry accepts (below 2^31) and reserves no scratch
// that grows with the volume; a median costs nine walks where a max costs one.  (Staging C samples per ray in LDS would
// save walks only for rays of at most C samples -- 64 rays x 512 samples are 128 KB -- and sorting a staged chunk does not
// give the rank of an element among the samples outside it.)
//
// The views (fill_xform of each q = A p + t) are uploaded into the context's scratch -- nviews x 304 bytes -- and the
// call waits for the stream once that copy is queued, because they are host memory of this call; the kernel is enqueued.
#pragma once

#include <vector>

namespace {

constexpr int PJ_MAX = PP_PROJECT_MAX_LABELS;
constexpr int PJ_RAYS = 64;            // rays per block: one wavefront
constexpr int PJ_TS = 16;              // samples per ray and tile
constexpr int PJ_IS = PJ_TS + 1;       // ... row stride of the image tile (floats) and
constexpr int PJ_LS = PJ_TS + 4;       // ... of a label tile (bytes: 5 words), both odd in words: lane r reads row r without conflicts

struct pj_args {
  pp_dims d;
  int axis, n, rows, cols;      // n: samples per ray; the output planes are [rows][cols]
  int kind, img_interp, nlabels, any_linear;   // any_linear: some label is interpolated linearly
  float default_value;
  const float* image;           // NULL: labels only
  float* image_out;
  const uint8_t* lin[PJ_MAX];   // padded with lin[0] beyond nlabels: every entry up to the kernel's NLCAP can be read
  uint8_t* lout[PJ_MAX];
  int linterp[PJ_MAX];
  const pp_xform* views;        // device, one per view
};

// The sample of every member at output index (x, y, z): what k_resample<T, INTERP, false> writes there.  As in
// pp_resample_set.h only the control flow differs: a point outside the buffer (NaN included) is sampled at index (0, 0, 0)
// and its results replaced by the defaults, and every label's nearest-neighbour voxel is loaded whether the label wants it
// or not (lin[] is padded with valid pointers up to NLCAP), so that the gathers of a sample are straight-line code, all in
// flight together.  LABELS = false: the image alone.
template <int NLCAP, bool LABELS>
__device__ __forceinline__ void pj_sample(const pj_args& P, const pp_xform& X, int x, int y, int z, float& v, uint8_t* lab) {
  double c[3];
  pp_map_point(X, x, y, z, 0.0, 0.0, 0.0, c);
  const bool ok = pp_inside_d(c, P.d);
  const double s0 = ok ? c[0] : 0.0, s1 = ok ? c[1] : 0.0, s2 = ok ? c[2] : 0.0;
  const int qx = (int)floor(s0 + 0.5), qy = (int)floor(s1 + 0.5), qz = (int)floor(s2 + 0.5);
  const size_t q = ((size_t)qz * P.d.ny + qy) * P.d.nx + qx;
  const double flx = floor(s0), fly = floor(s1), flz = floor(s2);
  const int bx = (int)flx, by = (int)fly, bz = (int)flz;
  const float fx = (float)(s0 - flx), fy = (float)(s1 - fly), fz = (float)(s2 - flz);
  const bool wide = P.d.nx >= 2;
  float r = 0.0f;
  if (P.img_interp == PP_INTERP_NEAREST)
    r = P.image[q];
  else if (P.img_interp == PP_INTERP_LINEAR)
    r = pp_cast_out<float>(wide ? pp_trilinear_pairs(P.image, P.d.nx, P.d.ny, P.d.nz, bx, fx, by, fy, bz, fz)
                                : pp_trilinear(P.image, P.d.nx, P.d.ny, P.d.nz, bx, fx, by, fy, bz, fz));
  v = ok ? r : P.default_value;
  if (LABELS) {
    uint8_t nn[NLCAP ? NLCAP : 1];
#pragma unroll
    for (int l = 0; l < NLCAP; ++l) nn[l] = P.lin[l][q];
    if (P.any_linear) {     // (uniform, and rare: the labels that are interpolated linearly)
#pragma unroll
      for (int l = 0; l < NLCAP; ++l)
        if (P.linterp[l] == PP_INTERP_LINEAR)
          nn[l] = pp_cast_out<uint8_t>(wide ? pp_trilinear_pairs(P.lin[l], P.d.nx, P.d.ny, P.d.nz, bx, fx, by, fy, bz, fz)
                                            : pp_trilinear(P.lin[l], P.d.nx, P.d.ny, P.d.nz, bx, fx, by, fy, bz, fz));
    }
#pragma unroll
    for (int l = 0; l < NLCAP; ++l) lab[l] = ok ? nn[l] : (uint8_t)0;
  }
}

// f(v, lab) for every sample of this thread's ray (col, row) in index order.  The wavefront samples a tile of PJ_RAYS rays x
// PJ_TS samples in PJ_TS steps of one compact patch each (see the head of this file), parks the samples in LDS, and lane r
// consumes row r of the tile.  Every thread of the block must call it (barriers), whether its ray exists or not.
template <bool AX0, int NLCAP, bool LABELS, typename F>
__device__ __forceinline__ void pj_walk(const pj_args& P, const pp_xform& X, int col, int row, float* timg, uint8_t* tlab, F&& f) {
  constexpr int NL1 = NLCAP ? NLCAP : 1;
  const int lane = (int)threadIdx.x, c0 = (int)blockIdx.x * PJ_RAYS;
  for (int k0 = 0; k0 < P.n; k0 += PJ_TS) {
#pragma unroll 4
    for (int i = 0; i < PJ_TS; ++i) {
      // axis 0: 4 rays x 16 samples a step (the samples run along x); axes 1, 2: 16 rays x 4 samples (the rays do)
      const int r = AX0 ? i * (PJ_RAYS / PJ_TS) + lane / PJ_TS : (i / 4) * 16 + lane % 16;
      const int s = AX0 ? lane % PJ_TS : (i % 4) * 4 + lane / 16;
      const int k = k0 + s, c = c0 + r;
      if (k < P.n && c < P.cols) {
        float v;
        uint8_t lab[NL1];
        if (AX0) pj_sample<NLCAP, LABELS>(P, X, k, c, row, v, lab);
        else if (P.axis == 1) pj_sample<NLCAP, LABELS>(P, X, c, k, row, v, lab);
        else pj_sample<NLCAP, LABELS>(P, X, c, row, k, v, lab);
        timg[r * PJ_IS + s] = v;
        if (LABELS) {
#pragma unroll
          for (int l = 0; l < NLCAP; ++l) tlab[(l * PJ_RAYS + r) * PJ_LS + s] = lab[l];
        }
      }
    }
    __syncthreads();
    if (col < P.cols) {
      const int m = P.n - k0 < PJ_TS ? P.n - k0 : PJ_TS;
#pragma unroll 4
      for (int s = 0; s < m; ++s) {
        uint8_t lab[NL1];
        if (LABELS) {
#pragma unroll
          for (int l = 0; l < NLCAP; ++l) lab[l] = tlab[(l * PJ_RAYS + lane) * PJ_LS + s];
        }
        f(timg[lane * PJ_IS + s], lab);
      }
    }
    __syncthreads();
  }
}

// order-preserving key of a sample: a < b <=> key(a) < key(b); every NaN is the largest key
__device__ __forceinline__ unsigned pj_key(float v) {
  const unsigned b = __builtin_bit_cast(unsigned, v);
  if (v != v) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float pj_unkey(unsigned k) {
  if (k == 0xffffffffu) return __builtin_bit_cast(float, 0x7fc00000u);
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// one more squared deviation, each operation rounded on its own
__device__ __forceinline__ double pj_add_sq(double s, float v, double mean) {
#pragma clang fp contract(off)
  const double dv = (double)v - mean;
  const double sq = dv * dv;
  return s + sq;
}

template <bool AX0, int NLCAP>
__global__ void __launch_bounds__(PJ_RAYS) k_project(pj_args P) {
  constexpr int NL1 = NLCAP ? NLCAP : 1;
  __shared__ float timg[PJ_RAYS * PJ_IS];
  __shared__ uint8_t tlab[NLCAP ? NLCAP * PJ_RAYS * PJ_LS : 4];
  const pp_xform X = P.views[blockIdx.z];
  const int col = (int)blockIdx.x * PJ_RAYS + (int)threadIdx.x, row = (int)blockIdx.y;
  const bool live = col < P.cols;
  const size_t o = ((size_t)blockIdx.z * P.rows + row) * P.cols + col;
  const bool img = P.image != nullptr;

  // the first walk: every member; min, max and the ordered sum together (one of them is the result for four of the kinds)
  float mn = INFINITY, mx = -INFINITY;
  double sum = 0.0;
  uint8_t lmx[NL1];
#pragma unroll
  for (int l = 0; l < NL1; ++l) lmx[l] = 0;
  pj_walk<AX0, NLCAP, (NLCAP > 0)>(P, X, col, row, timg, tlab, [&](float v, const uint8_t* lab) {
    mn = (v < mn || v != v) ? v : mn;
    mx = (v > mx || v != v) ? v : mx;
    sum = sum + (double)v;
#pragma unroll
    for (int l = 0; l < NLCAP; ++l) lmx[l] = lab[l] > lmx[l] ? lab[l] : lmx[l];
  });
  if (live) {
#pragma unroll
    for (int l = 0; l < NLCAP; ++l)
      if (l < P.nlabels) P.lout[l][o] = lmx[l];
  }
  if (!img) return;     // (uniform: no barrier is left waiting)

  const double n = (double)P.n;
  float res;
  if (P.kind == PP_PROJECT_SUM) {
    res = (float)sum;
  } else if (P.kind == PP_PROJECT_MEAN) {
    res = (float)(sum / n);
  } else if (P.kind == PP_PROJECT_MIN) {
    res = mn;
  } else if (P.kind == PP_PROJECT_MAX) {
    res = mx;
  } else if (P.kind == PP_PROJECT_STD) {
    const double mean = sum / n;
    double ss = 0.0;
    pj_walk<AX0, NLCAP, false>(P, X, col, row, timg, tlab, [&](float v, const uint8_t*) { ss = pj_add_sq(ss, v, mean); });
    res = (float)sqrt(ss / (n - 1.0));
  } else {   // PP_PROJECT_MEDIAN: the key of rank n / 2, four bits a walk
    unsigned long long prefix = 0;
    unsigned rank = (unsigned)P.n / 2u;
    for (int shift = 28; shift >= 0; shift -= 4) {
      unsigned cnt[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) cnt[j] = 0;
      pj_walk<AX0, NLCAP, false>(P, X, col, row, timg, tlab, [&](float v, const uint8_t*) {
        const unsigned long long key = pj_key(v);
        const unsigned digit = (unsigned)(key >> shift) & 15u;
        const bool mine = (key >> (shift + 4)) == prefix;
#pragma unroll
        for (int j = 0; j < 16; ++j) cnt[j] += (mine && digit == (unsigned)j) ? 1u : 0u;
      });
      unsigned digit = 15;
      bool found = false;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (!found) {
          if (rank < cnt[j]) {
            digit = (unsigned)j;
            found = true;
          } else {
            rank -= cnt[j];
          }
        }
      }
      prefix = (prefix << 4) | digit;
    }
    res = pj_unkey((unsigned)prefix);
  }
  if (live) P.image_out[o] = res;
}

}  // namespace

extern "C" {

int pp_project_set(pp_ctx* ctx, const pp_geom* g, int axis, const double* views, int nviews, const float* image, int kind,
                   int image_interp, double image_default, float* image_out, const uint8_t* const* labels, const int* label_interp,
                   int nlabels, uint8_t* const* labels_out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, axis >= 0 && axis <= 2, "pp_project_set: the projection axis is 0, 1 or 2");
  PP_REQUIRE(ctx, nviews >= 1 && views, "pp_project_set: at least one view");
  PP_REQUIRE(ctx, nlabels >= 0 && nlabels <= PP_PROJECT_MAX_LABELS, "pp_project_set: 0 ... 16 label volumes per call");
  PP_REQUIRE(ctx, image || nlabels > 0, "pp_project_set: neither an image nor a label");
  PP_REQUIRE(ctx, !image || image_out, "pp_project_set: NULL image output");
  PP_REQUIRE(ctx, !image || (kind >= PP_PROJECT_SUM && kind <= PP_PROJECT_MAX), "pp_project_set: unknown projection kind");
  PP_REQUIRE(ctx, nlabels == 0 || (labels && labels_out && label_interp), "pp_project_set: NULL label table");
  PP_REQUIRE(ctx, !image || (image_interp >= PP_INTERP_NEAREST && image_interp <= PP_INTERP_BSPLINE), "pp_project_set: unknown interpolator");
  for (int l = 0; l < nlabels; ++l) {
    PP_REQUIRE(ctx, labels[l] && labels_out[l], "pp_project_set: NULL label volume");
    PP_REQUIRE(ctx, label_interp[l] >= PP_INTERP_NEAREST && label_interp[l] <= PP_INTERP_BSPLINE, "pp_project_set: unknown interpolator");
  }
  // no output is an input or another output
  const void* ins[PJ_MAX + 1];
  const void* outs[PJ_MAX + 1];
  int nin = 0, nout = 0;
  if (image) {
    ins[nin++] = image;
    outs[nout++] = image_out;
  }
  for (int l = 0; l < nlabels; ++l) {
    ins[nin++] = labels[l];
    outs[nout++] = labels_out[l];
  }
  for (int a = 0; a < nout; ++a) {
    for (int b = 0; b < nin; ++b) PP_REQUIRE(ctx, outs[a] != ins[b], "pp_project_set: an output aliases an input");
    for (int b = 0; b < a; ++b) PP_REQUIRE(ctx, outs[a] != outs[b], "pp_project_set: two outputs are one buffer");
  }
  bool spline = image && image_interp == PP_INTERP_BSPLINE;
  for (int l = 0; l < nlabels; ++l) spline = spline || label_interp[l] == PP_INTERP_BSPLINE;
  if (spline) return pp_fail(ctx, PP_ERR_UNSUPPORTED, "pp_project_set: interpolators are nearest or linear; rotate with pp_resample_f32");
  int rc = pp_geom_check(ctx, g, "grid");
  if (rc) return rc;

  pj_args P;
  P.d = pp_dims{g->size[0], g->size[1], g->size[2]};
  P.axis = axis;
  P.n = g->size[axis];
  P.rows = axis == 2 ? g->size[1] : g->size[2];
  P.cols = axis == 0 ? g->size[1] : g->size[0];
  P.kind = kind;
  P.img_interp = image ? image_interp : 0;
  P.nlabels = nlabels;
  P.default_value = (float)image_default;
  P.image = image;
  P.image_out = image_out;
  P.any_linear = 0;
  for (int l = 0; l < PJ_MAX; ++l) {
    P.lin[l] = l < nlabels ? labels[l] : (nlabels > 0 ? labels[0] : nullptr);
    P.lout[l] = l < nlabels ? labels_out[l] : nullptr;
    P.linterp[l] = l < nlabels ? label_interp[l] : 0;
    if (P.linterp[l] == PP_INTERP_LINEAR) P.any_linear = 1;
  }
  if (P.rows > 65535 || nviews > 65535) return pp_fail(ctx, PP_ERR_SIZE, "pp_project_set: more than 65535 output rows or views");

  rc = pp_reserve(ctx, (size_t)nviews * sizeof(pp_xform));
  if (rc) return rc;
  std::vector<pp_xform> host((size_t)nviews);
  for (int v = 0; v < nviews; ++v) fill_xform(g, g, views + (size_t)v * 12, views + (size_t)v * 12 + 9, &host[(size_t)v]);
  pp_xform* dviews = reinterpret_cast<pp_xform*>(ctx->ws);
  PP_HIP(ctx, hipMemcpyAsync(dviews, host.data(), host.size() * sizeof(pp_xform), hipMemcpyHostToDevice, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (`host` is memory of this call: no return below leaves the copy queued)
  P.views = dviews;

  const dim3 grid((unsigned)((P.cols + PJ_RAYS - 1) / PJ_RAYS), (unsigned)P.rows, (unsigned)nviews), block(PJ_RAYS);
  {
    pp_prof_scope prof_(ctx, "k_project");
#define PP_PJ(AX0) do { \
      if (nlabels == 0) hipLaunchKernelGGL((k_project<AX0, 0>), grid, block, 0, ctx->stream, P); \
      else if (nlabels <= 4) hipLaunchKernelGGL((k_project<AX0, 4>), grid, block, 0, ctx->stream, P); \
      else if (nlabels <= 8) hipLaunchKernelGGL((k_project<AX0, 8>), grid, block, 0, ctx->stream, P); \
      else hipLaunchKernelGGL((k_project<AX0, PJ_MAX>), grid, block, 0, ctx->stream, P); \
    } while (0)
    if (axis == 0) PP_PJ(true);
    else PP_PJ(false);
#undef PP_PJ
  }
  PP_LAUNCH_CHECK(ctx, "k_project");
  return PP_OK;
}

}  // extern "C"
