// platipy_amd/csrc/pp_sift.h -- 3-D SIFT landmarks for deformable-registration QA (the reference's services/dirqa/service.py
// runs `plastimatch sift` and matches the two keypoint lists): the scale-space extremum search, the windowed gradient
// descriptor, the all-pairs nearest-neighbour search and a displacement field applied to a list of points.  #included at the
// end of pp_fusion.hip (it uses that file's NT and grid_for, and pp_block_tree of pp_reduce.h).
//
// Neither plastimatch nor ITK's SIFT filter is available where this was written: parity with them is UNPINNED.  The rules
// S1 ... S7 below are THIS BUILD'S DECISIONS unless marked "recalled"; tests/sift_restatement.py restates
// them in numpy.
//
// S1  normalisation   the contrast threshold applies to |response| / range, range = hi - lo of the caller's intensity window
//                     (the image's min / max without one); the caller passes `range`.
// S2  scale space     built by the caller (platipy_amd/registration/qa.py) from the existing Gaussian passes: an octave is
//                     a stack of nlevels = intervals + 3 volumes G_0 ... G_{nlevels-1} on one grid.
// S3  candidates      D_l = G_{l+1} - G_l, ONE fp32 subtraction.  A voxel of an interior level 1 <= l <= nlevels - 3, at
//                     least one voxel from every face, is a candidate when D_l there is STRICTLY greater than all 80
//                     neighbours (26 on its level, 27 on each adjacent level) or strictly smaller than all of them.  A
//                     plateau, or a NaN among the 81 values, yields nothing.
// S4  refinement      on candidates only, in fp64, in index units: g and H of D_l by central differences
//                     (g_x = (D(x+1) - D(x-1)) / 2, H_xx = D(x+1) - 2 D + D(x-1), H_xy = (D(+,+) - D(+,-) - D(-,+) + D(-,-)) / 4),
//                     one Newton step o = -H^-1 g by the adjugate, each component clamped to [-0.5, 0.5],
//                     response = D + 0.5 g.o.  Kept when |response| / range >= contrast_threshold, H is definite
//                     (determinant and trace of the same sign, sum of the principal 2 x 2 minors positive) and
//                     trace^3 / det < curvature_threshold.  A zero or non-finite determinant rejects.
//                     [recalled, unverified: 172.3 ~ (r + 2)^3 / r at r = 10, Lowe's edge ratio carried to three dimensions]
// S5  order           keypoints come out in ascending (level, z, y, x); with more than `capacity` the first `capacity`
//                     rows in that order are returned together with the true count.
// S6  descriptor      NOT rotation invariant (DIR QA pairs are already roughly aligned).  On the Gaussian image of the
//                     keypoint's level: the 16 x 16 x 16 voxels at offsets -8 ... 7 about the keypoint's voxel, indices
//                     clamped to the grid (edge replicate); gradient component = (double)(G[i+1] - G[i-1]) / (2 spacing), the
//                     difference ONE fp32 subtraction of the clamped neighbours; weight = w[oz] w[oy] w[ox],
//                     w[o] = exp(-(o + 0.5)^2 / 128) (the caller's fp64 table); the sample adds weight x |gradient| to the
//                     orientation bin, of the 12 icosahedron vertices (0, +-1, +-phi), (+-1, +-phi, 0), (+-phi, 0, +-1), in
//                     that order with signs (+,+), (+,-), (-,+), (-,-), whose dot product with the gradient is largest, the
//                     lowest index on a tie; a zero (or NaN) gradient adds nothing.  4 x 4 x 4 cells of 4 x 4 x 4 samples x
//                     12 bins = 768 fp64 sums, entry (cell_z 16 + cell_y 4 + cell_x) 12 + bin, each accumulated over z, y, x
//                     of its cell in that order.  Then: L2-normalise, clip at 0.2, normalise again, store fp32.  An
//                     all-zero histogram stays all zero.
// S7  matching        distance = sum over k ascending of (a_k - b_k)^2 in fp32, each term one fused multiply-add.  Per row
//                     of A: best and second-best distance over the rows of B that take part and the best row, the lowest
//                     index on a tie (so a duplicated best row gives second == best); nothing takes part: index -1, both
//                     +inf; one row: second = +inf.  With a gate, row j takes part when |pa_i - pb_j|^2 <= radius^2 (fp64).
//                     Acceptance (best < ratio^2 second, mutual) is the caller's, on these numbers.
//
// Extremum pass (pp_dog_extrema_f32).  The difference images are never written.  A workgroup of 256 threads owns a column of
// 32 x 8 voxels and walks SF_ZC planes; per step every Gaussian level of plane z + 1 is read once (with a one-voxel halo
// in x and y) and its differences go to a ring of three LDS planes per DoG level (34 x 10 voxels each), so the compulsory
// traffic, nlevels x 4 bytes per voxel, is read once apart from the halo.  A thread tests its voxel against its own plane first
// (most voxels stop there).  Kept voxels are FLAGGED, one bit per voxel and interior level (a wavefront ballot: two 32-bit
// words per wavefront, levels x voxels / 8 bytes in all); the list is then compacted in key order by count, scan, write:
// k_dog_count sums the bits of 4096 words per block, one block scans the block sums, k_dog_write ranks the bits of its words
// and writes row `rank` after refining the keypoint again from global memory (the same device function that decided to
// keep it).  No floating-point atomic, no arrival order: reruns are bit-identical.
//
// Describe pass (pp_sift_describe_f32).  One wavefront per keypoint, one lane per cell, twelve fp64 sums in registers, no
// atomics; the two norms are xor-butterfly wave reductions (every lane adds the same pairs: one fixed order).
//
// Match (pp_descriptor_match_f32).  A workgroup takes 64 rows of A and a segment of B's tiles of 64 rows, both staged through
// LDS in chunks of 32 components; a thread holds a 4 x 4 register tile of distances (eight LDS reads per sixteen
// multiply-adds), keeps per row the running best / second of its columns (ascending), and one thread per row merges the 16
// partial results in ascending column group.  B is split into as many segments as it takes to fill the device; a second
// kernel folds the segments' partial results in ascending segment order.  Every fold is in a fixed order and the merge rule
// prefers the lower index on equal distances, so the result does not depend on the split.  Any descriptor length.
//
// Points (pp_transform_points_f64).  q = p + D(p): the continuous index c = A p + b of pp_make_index_map (the map
// pp_resample_f32 uses, from a unit grid whose index IS the physical point), fp64 trilinear interpolation of the fp32 field
// with ITK's clamped upper corner; outside [-0.5, n - 0.5) on any axis (or NaN) the displacement is zero.
#pragma once

namespace {

constexpr int SF_TX = 32, SF_TY = 8, SF_ZC = 16;
constexpr int SF_PITCH = SF_TX + 3;
constexpr int SF_MAX_LEVELS = 8;          // Gaussian volumes of an octave: intervals + 3
constexpr int SF_SCAN_WORDS = 16;         // flag words a thread of the count / write kernels takes
constexpr int SF_DESC = 768, SF_BINS = 12, SF_WIN = 16;
constexpr int SM_ROWS = 64, SM_COLS = 64, SM_K = 32;

struct sf_tests {
  double range, contrast, curvature;
  int candidates_only;
};

struct sf_fit {
  double o[3], response;
  int keep;
};

// S4 on voxel (x, y, z) of DoG level l (all 27 neighbours inside the grid)
__device__ inline sf_fit sf_refine(const float* __restrict__ g, pp_dims d, int l, int x, int y, int z, const sf_tests& t) {
  const size_t N = (size_t)d.nx * d.ny * d.nz;
  const float* lo = g + (size_t)l * N;
  const float* hi = lo + N;
  auto D = [&](int dx, int dy, int dz) -> double {
    const size_t i = ((size_t)(z + dz) * d.ny + (size_t)(y + dy)) * d.nx + (size_t)(x + dx);
    return (double)(hi[i] - lo[i]);
  };
  sf_fit f;
  const double c = D(0, 0, 0);
  f.o[0] = f.o[1] = f.o[2] = 0.0;
  f.response = c;
  f.keep = 1;
  if (t.candidates_only) return f;
  const double xp = D(1, 0, 0), xm = D(-1, 0, 0), yp = D(0, 1, 0), ym = D(0, -1, 0), zp = D(0, 0, 1), zm = D(0, 0, -1);
  const double gx = 0.5 * (xp - xm), gy = 0.5 * (yp - ym), gz = 0.5 * (zp - zm);
  const double hxx = xp - 2.0 * c + xm, hyy = yp - 2.0 * c + ym, hzz = zp - 2.0 * c + zm;
  const double hxy = 0.25 * (D(1, 1, 0) - D(1, -1, 0) - D(-1, 1, 0) + D(-1, -1, 0));
  const double hxz = 0.25 * (D(1, 0, 1) - D(1, 0, -1) - D(-1, 0, 1) + D(-1, 0, -1));
  const double hyz = 0.25 * (D(0, 1, 1) - D(0, 1, -1) - D(0, -1, 1) + D(0, -1, -1));
  const double c00 = hyy * hzz - hyz * hyz, c01 = hxz * hyz - hxy * hzz, c02 = hxy * hyz - hxz * hyy;
  const double c11 = hxx * hzz - hxz * hxz, c12 = hxy * hxz - hxx * hyz, c22 = hxx * hyy - hxy * hxy;
  const double det = hxx * c00 + hxy * c01 + hxz * c02;
  if (!(det != 0.0) || !(det - det == 0.0)) {
    f.keep = 0;
    return f;
  }
  const double o[3] = {-(c00 * gx + c01 * gy + c02 * gz) / det, -(c01 * gx + c11 * gy + c12 * gz) / det,
                       -(c02 * gx + c12 * gy + c22 * gz) / det};
#pragma unroll
  for (int k = 0; k < 3; ++k) f.o[k] = o[k] < -0.5 ? -0.5 : (o[k] > 0.5 ? 0.5 : o[k]);
  f.response = c + 0.5 * (gx * f.o[0] + gy * f.o[1] + gz * f.o[2]);
  const double trace = hxx + hyy + hzz, minors = c00 + c11 + c22;
  const bool contrast = fabs(f.response) / t.range >= t.contrast;
  const bool definite = ((det > 0.0 && trace > 0.0) || (det < 0.0 && trace < 0.0)) && minors > 0.0;
  const bool round_enough = trace * trace * trace / det < t.curvature;
  f.keep = contrast && definite && round_enough;
  return f;
}

// words[((l - 1) nz + z) ny + y][xw] |= bit (x & 31) for every kept voxel; `words` starts zeroed
__global__ void __launch_bounds__(NT) k_dog_flags(const float* __restrict__ g, pp_dims d, int nlev, sf_tests t, unsigned* __restrict__ words,
                                                  int xw) {
  __shared__ float tile[3][SF_MAX_LEVELS - 1][SF_TY + 2][SF_PITCH];
  const int tid = threadIdx.x, tx = tid & (SF_TX - 1), ty = tid / SF_TX;
  const int x0 = blockIdx.x * SF_TX, y0 = blockIdx.y * SF_TY;
  const int x = x0 + tx, y = y0 + ty;
  const int ndog = nlev - 1;
  const size_t plane = (size_t)d.nx * d.ny, N = plane * d.nz;
  const int z0 = blockIdx.z * SF_ZC, z1 = z0 + SF_ZC < d.nz ? z0 + SF_ZC : d.nz;
  auto load_plane = [&](int z) {   // the differences of plane z (clamped) into ring slot (z + 3) % 3
    const int slot = (z + 3) % 3;
    const size_t zo = (size_t)pp_clampi(z, 0, d.nz - 1) * plane;
    for (int e = tid; e < (SF_TY + 2) * (SF_TX + 2); e += NT) {
      const int r = e / (SF_TX + 2), c = e % (SF_TX + 2);
      const size_t i = zo + (size_t)pp_clampi(y0 + r - 1, 0, d.ny - 1) * d.nx + (size_t)pp_clampi(x0 + c - 1, 0, d.nx - 1);
      float below = g[i];
      for (int l = 0; l < ndog; ++l) {
        const float above = g[(size_t)(l + 1) * N + i];
        tile[slot][l][r][c] = above - below;
        below = above;
      }
    }
  };
  load_plane(z0 - 1);
  load_plane(z0);
  const bool inside_xy = x >= 1 && x <= d.nx - 2 && y >= 1 && y <= d.ny - 2;
  for (int z = z0; z < z1; ++z) {
    __syncthreads();   // plane z - 2 has been read
    load_plane(z + 1);
    __syncthreads();
    const int sc = (z + 3) % 3, sp = (z + 2) % 3, sn = (z + 4) % 3;
    const bool inside = inside_xy && z >= 1 && z <= d.nz - 2;
    for (int l = 1; l <= ndog - 2; ++l) {
      int keep = 0;
      if (inside) {
        const float v = tile[sc][l][ty + 1][tx + 1];
        bool gt = true, lt = true;
        // own plane of the own level first, then the other eight 3 x 3 groups
        const int ls[3] = {l, l - 1, l + 1}, ss[3] = {sc, sp, sn};
        for (int a = 0; a < 3 && (gt || lt); ++a)
          for (int b = 0; b < 3 && (gt || lt); ++b) {
            const bool own = a == 0 && b == 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) {
                if (own && dy == 1 && dx == 1) continue;
                const float n = tile[ss[b]][ls[a]][ty + dy][tx + dx];
                gt = gt && v > n;
                lt = lt && v < n;
              }
          }
        if (gt || lt) keep = t.candidates_only ? 1 : sf_refine(g, d, l, x, y, z, t).keep;
      }
      const unsigned long long ballot = __ballot(keep);
      const unsigned word = (unsigned)(ballot >> (32 * ((tid >> 5) & 1)));
      if (tx == 0 && y < d.ny && word) words[(((size_t)(l - 1) * d.nz + z) * d.ny + y) * xw + blockIdx.x] = word;
    }
  }
}

// partial[b] = set bits of words [b CH, (b + 1) CH), CH = NT * SF_SCAN_WORDS
__global__ void __launch_bounds__(NT) k_dog_count(const unsigned* __restrict__ words, size_t W, int* __restrict__ partial) {
  __shared__ int sh[NT];
  const int t = threadIdx.x;
  const size_t w0 = ((size_t)blockIdx.x * NT + t) * SF_SCAN_WORDS;
  int s = 0;
  for (int k = 0; k < SF_SCAN_WORDS; ++k)
    if (w0 + k < W) s += __builtin_popcount(words[w0 + k]);
  sh[t] = s;
  pp_block_tree<NT>(t, [&](int a, int b) { sh[a] += sh[b]; });
  if (t == 0) partial[blockIdx.x] = sh[0];
}

// one block: partial[0 ... nb) -> its exclusive prefix sums in place, partial[nb] = the total
__global__ void __launch_bounds__(NT) k_dog_scan(int* __restrict__ partial, int nb) {
  __shared__ int sh[NT];
  const int t = threadIdx.x;
  const int per = (nb + NT - 1) / NT;
  const int b0 = t * per < nb ? t * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
  int s = 0;
  for (int b = b0; b < b1; ++b) s += partial[b];
  sh[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < NT; ++k) {
      const int v = sh[k];
      sh[k] = run;
      run += v;
    }
    partial[nb] = run;
  }
  __syncthreads();
  int run = sh[t];
  for (int b = b0; b < b1; ++b) {
    const int v = partial[b];
    partial[b] = run;
    run += v;
  }
}

// row `rank` of the outputs for every set bit of rank < cap, ranks in word order then bit order = (level, z, y, x)
__global__ void __launch_bounds__(NT) k_dog_write(const float* __restrict__ g, pp_dims d, sf_tests t, const unsigned* __restrict__ words, size_t W,
                                                  int xw, const int* __restrict__ offsets, int cap, int* __restrict__ out_index,
                                                  double* __restrict__ out_values) {
  __shared__ int sh[NT];
  const int tid = threadIdx.x;
  const size_t w0 = ((size_t)blockIdx.x * NT + tid) * SF_SCAN_WORDS;
  int s = 0;
  for (int k = 0; k < SF_SCAN_WORDS; ++k)
    if (w0 + k < W) s += __builtin_popcount(words[w0 + k]);
  sh[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = offsets[blockIdx.x];
    for (int k = 0; k < NT; ++k) {
      const int v = sh[k];
      sh[k] = run;
      run += v;
    }
  }
  __syncthreads();
  int rank = sh[tid];
  if (!s) return;
  for (int k = 0; k < SF_SCAN_WORDS && rank < cap; ++k) {
    if (w0 + k >= W) break;
    unsigned word = words[w0 + k];
    if (!word) continue;
    size_t r = w0 + k;
    const int xi = (int)(r % xw);
    r /= xw;
    const int y = (int)(r % d.ny);
    r /= d.ny;
    const int z = (int)(r % d.nz), l = (int)(r / d.nz) + 1;
    while (word && rank < cap) {
      const int bit = __builtin_ctz(word);
      word &= word - 1;
      const int x = xi * 32 + bit;
      const sf_fit f = sf_refine(g, d, l, x, y, z, t);
      out_index[4 * (size_t)rank + 0] = x;
      out_index[4 * (size_t)rank + 1] = y;
      out_index[4 * (size_t)rank + 2] = z;
      out_index[4 * (size_t)rank + 3] = l;
      out_values[4 * (size_t)rank + 0] = f.o[0];
      out_values[4 * (size_t)rank + 1] = f.o[1];
      out_values[4 * (size_t)rank + 2] = f.o[2];
      out_values[4 * (size_t)rank + 3] = f.response;
      ++rank;
    }
  }
}

// ---------------------------------------------------------------------------------------
// descriptor

struct sf_window {
  double w[SF_WIN];       // exp(-(o + 0.5)^2 / 128), o = -8 ... 7
  double two_s[3];        // 2 x spacing of x, y, z
  double phi;
};

__device__ __forceinline__ double sf_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ void __launch_bounds__(NT) k_sift_describe(const float* __restrict__ g, pp_dims d, const int* __restrict__ kp, int n, sf_window win,
                                                      float* __restrict__ desc) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int k_raw = blockIdx.x * (NT / 64) + (tid >> 6);
  const bool live = k_raw < n;
  const int k = live ? k_raw : n - 1;   // (a spare wavefront repeats the last keypoint and stores nothing)
  const int kx = kp[4 * k + 0], ky = kp[4 * k + 1], kz = kp[4 * k + 2], kl = kp[4 * k + 3];
  const size_t plane = (size_t)d.nx * d.ny;
  const float* G = g + (size_t)kl * plane * d.nz;
  const int cx = lane & 3, cy = (lane >> 2) & 3, cz = lane >> 4;
  double h[SF_BINS];
#pragma unroll
  for (int b = 0; b < SF_BINS; ++b) h[b] = 0.0;
  for (int sz = 0; sz < 4; ++sz) {
    const int oz = cz * 4 + sz, Z = pp_clampi(kz + oz - 8, 0, d.nz - 1);
    const int Zm = Z > 0 ? Z - 1 : 0, Zp = Z < d.nz - 1 ? Z + 1 : d.nz - 1;
    for (int sy = 0; sy < 4; ++sy) {
      const int oy = cy * 4 + sy, Y = pp_clampi(ky + oy - 8, 0, d.ny - 1);
      const int Ym = Y > 0 ? Y - 1 : 0, Yp = Y < d.ny - 1 ? Y + 1 : d.ny - 1;
      const double wzy = win.w[oz] * win.w[oy];
      for (int sx = 0; sx < 4; ++sx) {
        const int ox = cx * 4 + sx, X = pp_clampi(kx + ox - 8, 0, d.nx - 1);
        const int Xm = X > 0 ? X - 1 : 0, Xp = X < d.nx - 1 ? X + 1 : d.nx - 1;
        const size_t row = (size_t)Z * plane + (size_t)Y * d.nx;
        const double gx = (double)(G[row + Xp] - G[row + Xm]) / win.two_s[0];
        const double gy = (double)(G[(size_t)Z * plane + (size_t)Yp * d.nx + X] - G[(size_t)Z * plane + (size_t)Ym * d.nx + X]) / win.two_s[1];
        const double gz = (double)(G[(size_t)Zp * plane + (size_t)Y * d.nx + X] - G[(size_t)Zm * plane + (size_t)Y * d.nx + X]) / win.two_s[2];
        const double mag = sqrt(gx * gx + gy * gy + gz * gz);
        if (!(mag > 0.0)) continue;
        const double py = gy * win.phi, pz = gz * win.phi, px = gx * win.phi;
        const double dots[SF_BINS] = {gy + pz, gy - pz, -gy + pz, -gy - pz, gx + py, gx - py, -gx + py, -gx - py,
                                      px + gz, px - gz, -px + gz, -px - gz};
        int best = 0;
        double top = dots[0];
#pragma unroll
        for (int b = 1; b < SF_BINS; ++b)
          if (dots[b] > top) {
            top = dots[b];
            best = b;
          }
        const double add = wzy * win.w[ox] * mag;
#pragma unroll
        for (int b = 0; b < SF_BINS; ++b) h[b] += b == best ? add : 0.0;
      }
    }
  }
  double s = 0.0;
#pragma unroll
  for (int b = 0; b < SF_BINS; ++b) s += h[b] * h[b];
  s = sf_wave_sum(s);
  const double n1 = sqrt(s);
  double s2 = 0.0;
#pragma unroll
  for (int b = 0; b < SF_BINS; ++b) {
    double v = s > 0.0 ? h[b] / n1 : 0.0;
    v = v > 0.2 ? 0.2 : v;
    h[b] = v;
    s2 += v * v;
  }
  s2 = sf_wave_sum(s2);
  const double n2 = sqrt(s2);
  if (!live) return;
  float* out = desc + (size_t)k * SF_DESC + (size_t)lane * SF_BINS;
#pragma unroll
  for (int b = 0; b < SF_BINS; ++b) out[b] = s2 > 0.0 ? (float)(h[b] / n2) : 0.0f;
}

// ---------------------------------------------------------------------------------------
// match

// fold candidate (b2, s2, i2) into (b, s, i): the two smallest of the union, the lower index on equal best
__device__ __forceinline__ void sm_merge(float& b, float& s, int& i, float b2, float s2, int i2) {
  if (i2 < 0) return;
  if (i < 0 || b2 < b || (b2 == b && i2 < i)) {
    const float old = b;
    const bool had = i >= 0;
    b = b2;
    i = i2;
    s = had ? fminf(old, s2) : s2;
  } else {
    s = fminf(s, b2);
  }
}

// Workgroup (x, y): rows [64 x, 64 x + 64) of A against segment y of B, tiles [y tiles_per_seg, (y + 1) tiles_per_seg) of 64 rows.
// Thread (ti, tj) holds the 4 x 4 distances of rows ti + 16 p and columns tj + 16 q of the tile; per row it keeps the running
// best / second of its columns (ascending), thread (ti, 0) merges the sixteen in ascending tj and writes the segment's partial
// result to part_*[y][row].
__global__ void __launch_bounds__(NT) k_descriptor_match(const float* __restrict__ A, int na, const float* __restrict__ B, int nb, int len,
                                                         const double* __restrict__ pa, const double* __restrict__ pb, double r2,
                                                         int tiles_per_seg, int* __restrict__ part_index, float* __restrict__ part_best,
                                                         float* __restrict__ part_second) {
  __shared__ float As[SM_ROWS][SM_K + 1];
  __shared__ float Bs[SM_COLS][SM_K + 1];
  __shared__ float mb[SM_ROWS][16], ms[SM_ROWS][16];
  __shared__ int mi[SM_ROWS][16];
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
  const int a0 = blockIdx.x * SM_ROWS;
  double p[4][3];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = a0 + ti + 16 * r;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[r][k] = pa && row < na ? pa[3 * (size_t)row + k] : 0.0;
  }
  float rb[4], rs[4];
  int ri[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rb[r] = INFINITY, rs[r] = INFINITY, ri[r] = -1;
  const int tile0 = blockIdx.y * tiles_per_seg;
  for (int tile = tile0; tile < tile0 + tiles_per_seg; ++tile) {
    const int b0 = tile * SM_COLS;
    if (b0 >= nb) break;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[r][q] = 0.0f;
    for (int k0 = 0; k0 < len; k0 += SM_K) {
      __syncthreads();
      for (int e = t; e < SM_ROWS * SM_K; e += NT) {
        const int r = e / SM_K, c = e % SM_K;
        As[r][c] = (a0 + r < na && k0 + c < len) ? A[(size_t)(a0 + r) * len + k0 + c] : 0.0f;
        Bs[r][c] = (b0 + r < nb && k0 + c < len) ? B[(size_t)(b0 + r) * len + k0 + c] : 0.0f;
      }
      __syncthreads();
#pragma unroll 4
      for (int c = 0; c < SM_K; ++c) {
        float av[4], bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = As[ti + 16 * r][c], bv[r] = Bs[tj + 16 * r][c];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float df = av[r] - bv[q];
            acc[r][q] = __fmaf_rn(df, df, acc[r][q]);
          }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (a0 + ti + 16 * r >= na) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = b0 + tj + 16 * q;
        if (j >= nb) continue;
        if (pb) {
          const double dx = p[r][0] - pb[3 * (size_t)j + 0], dy = p[r][1] - pb[3 * (size_t)j + 1], dz = p[r][2] - pb[3 * (size_t)j + 2];
          if (!(dx * dx + dy * dy + dz * dz <= r2)) continue;
        }
        const float dist = acc[r][q];
        if (dist < rb[r]) {
          rs[r] = rb[r];
          rb[r] = dist;
          ri[r] = j;
        } else if (dist < rs[r]) {
          rs[r] = dist;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mb[ti + 16 * r][tj] = rb[r];
    ms[ti + 16 * r][tj] = rs[r];
    mi[ti + 16 * r][tj] = ri[r];
  }
  __syncthreads();
  if (t < SM_ROWS && a0 + t < na) {
    float bb = INFINITY, ss = INFINITY;
    int ii = -1;
    for (int c = 0; c < 16; ++c) sm_merge(bb, ss, ii, mb[t][c], ms[t][c], mi[t][c]);
    const size_t o = (size_t)blockIdx.y * na + a0 + t;
    part_index[o] = ii;
    part_best[o] = bb;
    part_second[o] = ss;
  }
}

// row i: the segments' partial results folded in ascending segment order
__global__ void __launch_bounds__(NT) k_descriptor_match_fold(const int* __restrict__ part_index, const float* __restrict__ part_best,
                                                              const float* __restrict__ part_second, int na, int segments,
                                                              int* __restrict__ best_index, float* __restrict__ best, float* __restrict__ second) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= na) return;
  float bb = INFINITY, ss = INFINITY;
  int ii = -1;
  for (int s = 0; s < segments; ++s) {
    const size_t o = (size_t)s * na + i;
    sm_merge(bb, ss, ii, part_best[o], part_second[o], part_index[o]);
  }
  best_index[i] = ii;
  best[i] = bb;
  second[i] = ss;
}

// ---------------------------------------------------------------------------------------
// points

__global__ void __launch_bounds__(NT) k_transform_points(const float* __restrict__ field, pp_dims d, pp_index_map m, const double* __restrict__ pts,
                                                         int n, double* __restrict__ out) {
  const int k = blockIdx.x * NT + threadIdx.x;
  if (k >= n) return;
  const double p[3] = {pts[3 * (size_t)k + 0], pts[3 * (size_t)k + 1], pts[3 * (size_t)k + 2]};
  const int size[3] = {d.nx, d.ny, d.nz};
  int i0[3], i1[3];
  double w[3];
  bool inside = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double c = m.A[3 * r + 0] * p[0] + m.A[3 * r + 1] * p[1] + m.A[3 * r + 2] * p[2] + m.b[r];
    if (!(c >= -0.5 && c < (double)size[r] - 0.5)) {
      inside = false;
      i0[r] = i1[r] = 0;
      w[r] = 0.0;
      continue;
    }
    const double fl = floor(c);
    const int b = (int)fl;
    i0[r] = b < 0 ? 0 : b;
    i1[r] = i0[r] + 1 > size[r] - 1 ? size[r] - 1 : i0[r] + 1;
    w[r] = b < 0 ? 0.0 : c - fl;
  }
  double q[3] = {p[0], p[1], p[2]};
  if (inside) {
    const size_t sy = (size_t)d.nx, sz = (size_t)d.nx * d.ny, N = sz * d.nz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* u = field + (size_t)c * N;
      const double a000 = u[i0[2] * sz + i0[1] * sy + i0[0]], a100 = u[i0[2] * sz + i0[1] * sy + i1[0]];
      const double a010 = u[i0[2] * sz + i1[1] * sy + i0[0]], a110 = u[i0[2] * sz + i1[1] * sy + i1[0]];
      const double a001 = u[i1[2] * sz + i0[1] * sy + i0[0]], a101 = u[i1[2] * sz + i0[1] * sy + i1[0]];
      const double a011 = u[i1[2] * sz + i1[1] * sy + i0[0]], a111 = u[i1[2] * sz + i1[1] * sy + i1[0]];
      const double v00 = a000 + (a100 - a000) * w[0], v10 = a010 + (a110 - a010) * w[0];
      const double v01 = a001 + (a101 - a001) * w[0], v11 = a011 + (a111 - a011) * w[0];
      const double v0 = v00 + (v10 - v00) * w[1], v1 = v01 + (v11 - v01) * w[1];
      q[c] = p[c] + (v0 + (v1 - v0) * w[2]);
    }
  }
  out[3 * (size_t)k + 0] = q[0];
  out[3 * (size_t)k + 1] = q[1];
  out[3 * (size_t)k + 2] = q[2];
}

int sf_check_stack(pp_ctx* ctx, const char* who, const int size[3], int nlevels) {
  if (size[0] < 1 || size[1] < 1 || size[2] < 1) return pp_fail(ctx, PP_ERR_ARG, "%s: empty volume", who);
  if (pp_nvox(size) >= 0x7fffffffu) return pp_fail(ctx, PP_ERR_SIZE, "%s: volume of 2^31 voxels or more", who);
  if (nlevels < 4 || nlevels > SF_MAX_LEVELS) return pp_fail(ctx, PP_ERR_ARG, "%s: %d Gaussian levels (4 ... %d)", who, nlevels, SF_MAX_LEVELS);
  return PP_OK;
}

}  // namespace

extern "C" {

int pp_dog_extrema_f32(pp_ctx* ctx, const float* gauss, const int size[3], int nlevels, double range, double contrast_threshold,
                       double curvature_threshold, int candidates_only, int capacity, int32_t* index, double* values, int64_t* count) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, gauss && size && count, "pp_dog_extrema_f32: NULL argument");
  PP_REQUIRE(ctx, capacity >= 0 && (capacity == 0 || (index && values)), "pp_dog_extrema_f32: negative capacity, or rows without arrays");
  int rc = sf_check_stack(ctx, "pp_dog_extrema_f32", size, nlevels);
  if (rc) return rc;
  PP_REQUIRE(ctx, candidates_only || (range > 0.0 && range - range == 0.0), "pp_dog_extrema_f32: the intensity range must be positive and finite");
  PP_REQUIRE(ctx, candidates_only || (contrast_threshold == contrast_threshold && curvature_threshold == curvature_threshold),
             "pp_dog_extrema_f32: NaN threshold");
  *count = 0;
  if (size[0] < 3 || size[1] < 3 || size[2] < 3) return PP_OK;   // no voxel is one voxel from every face
  const pp_dims d{size[0], size[1], size[2]};
  const int xw = (d.nx + 31) / 32, intervals = nlevels - 3;
  const size_t W = (size_t)intervals * d.nz * d.ny * xw;
  const size_t chunk = (size_t)NT * SF_SCAN_WORDS;
  const int nb = (int)((W + chunk - 1) / chunk);
  const size_t b_words = pp_align_up(W * sizeof(unsigned), 256), b_part = pp_align_up(((size_t)nb + 1) * sizeof(int), 256);
  const size_t b_idx = pp_align_up((size_t)capacity * 4 * sizeof(int), 256), b_val = pp_align_up((size_t)capacity * 4 * sizeof(double), 256);
  rc = pp_reserve(ctx, b_words + b_part + b_idx + b_val + 256);
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  unsigned* words = cv.take<unsigned>(W);
  int* partial = cv.take<int>((size_t)nb + 1);
  int* d_idx = cv.take<int>((size_t)capacity * 4 + 1);
  double* d_val = cv.take<double>((size_t)capacity * 4 + 1);
  const sf_tests t{range, contrast_threshold, curvature_threshold, candidates_only != 0};
  PP_HIP(ctx, hipMemsetAsync(words, 0, W * sizeof(unsigned), ctx->stream));
  const dim3 grid((unsigned)xw, (unsigned)((d.ny + SF_TY - 1) / SF_TY), (unsigned)((d.nz + SF_ZC - 1) / SF_ZC));
  if (grid.y > 65535u || grid.z > 65535u) return pp_fail(ctx, PP_ERR_SIZE, "pp_dog_extrema_f32: an axis too long for the launch grid");
  hipLaunchKernelGGL(k_dog_flags, grid, dim3(NT), 0, ctx->stream, gauss, d, nlevels, t, words, xw);
  PP_LAUNCH_CHECK(ctx, "k_dog_flags");
  hipLaunchKernelGGL(k_dog_count, dim3((unsigned)nb), dim3(NT), 0, ctx->stream, (const unsigned*)words, W, partial);
  PP_LAUNCH_CHECK(ctx, "k_dog_count");
  hipLaunchKernelGGL(k_dog_scan, dim3(1), dim3(NT), 0, ctx->stream, partial, nb);
  PP_LAUNCH_CHECK(ctx, "k_dog_scan");
  int total = 0;
  rc = pp_read_back(ctx, partial + nb, &total, sizeof(total));
  if (rc) return rc;
  *count = total;
  const int rows = total < capacity ? total : capacity;
  if (rows == 0) return PP_OK;
  hipLaunchKernelGGL(k_dog_write, dim3((unsigned)nb), dim3(NT), 0, ctx->stream, gauss, d, t, (const unsigned*)words, W, xw, (const int*)partial,
                     capacity, d_idx, d_val);
  PP_LAUNCH_CHECK(ctx, "k_dog_write");
  PP_HIP(ctx, hipMemcpyAsync(index, d_idx, (size_t)rows * 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(values, d_val, (size_t)rows * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PP_OK;
}

int pp_sift_describe_f32(pp_ctx* ctx, const float* gauss, const int size[3], int nlevels, const double spacing[3], const int32_t* keypoints,
                         int n, float* descriptors) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, gauss && size && spacing && n >= 0 && (n == 0 || (keypoints && descriptors)), "pp_sift_describe_f32: NULL argument or negative count");
  int rc = sf_check_stack(ctx, "pp_sift_describe_f32", size, nlevels);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k)
    PP_REQUIRE(ctx, spacing[k] > 0.0 && spacing[k] - spacing[k] == 0.0, "pp_sift_describe_f32: the spacing must be positive and finite");
  for (int k = 0; k < n; ++k) {
    const int32_t* p = keypoints + 4 * (size_t)k;
    PP_REQUIRE(ctx, p[0] >= 0 && p[0] < size[0] && p[1] >= 0 && p[1] < size[1] && p[2] >= 0 && p[2] < size[2] && p[3] >= 0 && p[3] < nlevels,
               "pp_sift_describe_f32: a keypoint lies outside the stack");
  }
  if (n == 0) return PP_OK;
  rc = pp_reserve(ctx, pp_align_up((size_t)n * 4 * sizeof(int), 256));
  if (rc) return rc;
  int* dkp = reinterpret_cast<int*>(ctx->ws);
  PP_HIP(ctx, hipMemcpyAsync(dkp, keypoints, (size_t)n * 4 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  sf_window win;
  for (int o = 0; o < SF_WIN; ++o) win.w[o] = exp(-((double)(o - 8) + 0.5) * ((double)(o - 8) + 0.5) / 128.0);
  for (int k = 0; k < 3; ++k) win.two_s[k] = 2.0 * spacing[k];
  win.phi = (1.0 + sqrt(5.0)) / 2.0;
  const pp_dims d{size[0], size[1], size[2]};
  const int per = NT / 64;
  hipLaunchKernelGGL(k_sift_describe, dim3((unsigned)((n + per - 1) / per)), dim3(NT), 0, ctx->stream, gauss, d, (const int*)dkp, n, win, descriptors);
  PP_LAUNCH_CHECK(ctx, "k_sift_describe");
  // (the keypoints were staged from pageable memory: the caller may reuse its array once this returns)
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PP_OK;
}

int pp_descriptor_match_f32(pp_ctx* ctx, const float* a, int na, const float* b, int nb, int length, const double* points_a,
                            const double* points_b, double radius, int32_t* best_index, float* best, float* second) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, a && b && best_index && best && second, "pp_descriptor_match_f32: NULL argument");
  PP_REQUIRE(ctx, na >= 1 && nb >= 1 && length >= 1, "pp_descriptor_match_f32: empty table");
  PP_REQUIRE(ctx, (points_a != nullptr) == (points_b != nullptr), "pp_descriptor_match_f32: the two point lists go together");
  PP_REQUIRE(ctx, !points_a || radius >= 0.0, "pp_descriptor_match_f32: the search radius must not be negative or NaN");
  if ((double)na * length >= 2147483647.0 * 64.0 || (double)nb * length >= 2147483647.0 * 64.0)
    return pp_fail(ctx, PP_ERR_SIZE, "pp_descriptor_match_f32: table too large");
  // enough workgroups to fill the device: the tiles of B are split into segments, each with its own partial result
  const int row_blocks = (na + SM_ROWS - 1) / SM_ROWS, tiles = (nb + SM_COLS - 1) / SM_COLS;
  int segments = (1024 + row_blocks - 1) / row_blocks;
  segments = segments < 1 ? 1 : (segments > tiles ? tiles : segments);
  if (segments > 65535) segments = 65535;
  const int tiles_per_seg = (tiles + segments - 1) / segments;
  segments = (tiles + tiles_per_seg - 1) / tiles_per_seg;
  const size_t cells = (size_t)segments * na;
  int rc = pp_reserve(ctx, 3 * pp_align_up(cells * sizeof(float), 256));
  if (rc) return rc;
  pp_carver cv{ctx->ws, 0};
  int* part_index = cv.take<int>(cells);
  float* part_best = cv.take<float>(cells);
  float* part_second = cv.take<float>(cells);
  hipLaunchKernelGGL(k_descriptor_match, dim3((unsigned)row_blocks, (unsigned)segments), dim3(NT), 0, ctx->stream, a, na, b, nb, length, points_a,
                     points_b, radius * radius, tiles_per_seg, part_index, part_best, part_second);
  PP_LAUNCH_CHECK(ctx, "k_descriptor_match");
  hipLaunchKernelGGL(k_descriptor_match_fold, dim3((unsigned)((na + NT - 1) / NT)), dim3(NT), 0, ctx->stream, (const int*)part_index,
                     (const float*)part_best, (const float*)part_second, na, segments, best_index, best, second);
  PP_LAUNCH_CHECK(ctx, "k_descriptor_match_fold");
  return PP_OK;
}

int pp_transform_points_f64(pp_ctx* ctx, const float* field, const pp_geom* g, const double* points, int n, double* out) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, field && n >= 0 && (n == 0 || (points && out)), "pp_transform_points_f64: NULL argument or negative count");
  int rc = pp_geom_check(ctx, g, "field");
  if (rc) return rc;
  if (n == 0) return PP_OK;
  pp_geom unit;
  for (int k = 0; k < 3; ++k) unit.size[k] = 1, unit.spacing[k] = 1.0, unit.origin[k] = 0.0;
  for (int k = 0; k < 9; ++k) unit.direction[k] = k % 4 == 0 ? 1.0 : 0.0;
  pp_index_map m;
  pp_make_index_map(g, &unit, nullptr, nullptr, &m);   // continuous field index = A p + b for a physical point p
  const size_t bytes = pp_align_up((size_t)n * 3 * sizeof(double), 256);
  rc = pp_reserve(ctx, 2 * bytes);
  if (rc) return rc;
  double* din = reinterpret_cast<double*>(ctx->ws);
  double* dout = reinterpret_cast<double*>(ctx->ws + bytes);
  PP_HIP(ctx, hipMemcpyAsync(din, points, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const pp_dims d{g->size[0], g->size[1], g->size[2]};
  hipLaunchKernelGGL(k_transform_points, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, ctx->stream, field, d, m, (const double*)din, n, dout);
  PP_LAUNCH_CHECK(ctx, "k_transform_points");
  PP_HIP(ctx, hipMemcpyAsync(out, dout, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PP_OK;
}

}  // extern "C"
