// platipy_amd/csrc/pp_contour_trace.h -- binary masks to closed planar contours: the volume-sized step of
// platipy/dicom/io/nifti_to_rtstruct.py (convert_nifti), where the reference hands every mask to rt-utils, which traces it
// slice by slice with OpenCV on the host.  The inverse of pp_contour.h: filling the contours traced here gives the masks back
// byte for byte.  #included at the end of pp_fusion.hip, after pp_contour.h (it uses pp_fusion.hip's NT and grid_for and
// pp_contour.h's CT_MAX_INDEX).
//
// The rule (dicom/__init__.py T1-T7).  Per structure and slice; pixel (x, y), x to the right, y down; foreground is any
// non-zero byte.  A foreground pixel has a CRACK on each side (N, E, S, W) whose 4-neighbour is background or outside.
//   T1  a crack is directed with its own pixel on its right as displayed: N heads east, E south, S west, W north.
//   T2  successor at the head corner, AL / AR the pixels ahead-left / ahead-right: AL foreground -> the crack of AL (left turn,
//       side - 1); else AR foreground -> the crack of AR (straight, same side); else the next side of the same pixel (right
//       turn).  Foreground is 8-connected.  Every crack has one successor and one predecessor: disjoint cycles, the LOOPS.
//   T3  a loop's LEADER is its crack with the smallest key (y, x, side).  Leader on N: an outer border; on S: a hole.
//   T4  side pixel: the crack's own pixel on an outer loop, the background pixel across the crack on a hole loop.
//   T5  walking from the leader, every maximal cyclic run of equal side pixels is one vertex; the first vertex is the run
//       that holds the leader.
//   T6  contours are ordered by (structure, z, leader key); rows {first, count, structure, z} as pp_contour_fill_u8 takes them.
//   T7  approximate: a vertex whose incoming step equals its outgoing step is dropped (decided on the full sequence); the
//       contour starts at the first kept vertex at or after the T5 start.
//
// Scheme.  Cracks get dense ids in key order (structure, z, y, x, side), so "smallest key" is "smallest id" and the contour
// order of T6 is the id order of the leaders.
//   1  k_tr_stream<false>  the only pass that has to touch every byte (with pass 3): a thread owns 16 pixels of a row, walks
//      TR_ROWS rows down keeping the row above, its own and the row below as 18-bit words in registers (one 16-byte load per
//      new row), and four neighbouring lanes add their crack counts into one entry of the TABLE, one per row and 64-pixel
//      block -- the one volume-proportional scratch array, 1/16 int per pixel.
//   2  reduce-then-scan of the table in three launches (chunk sums, one block scans them, every chunk scans itself); a fourth
//      takes the largest slice's crack count.  READ-BACK 1: {cracks, cracks of the largest slice}; it sizes all that follows.
//   3  k_tr_stream<true>   the same walk writes each crack's (row, x, side) at its id.
//   4  k_tr_succ           successor by T2 from the 2 x 2 pixels at the head; a neighbour's id is one table read plus popcounts
//      over at most 63 pixels of three rows (tr_crack_id); predecessor by scatter (every crack is written exactly once).
//   5  leader = minimum id of the loop by pointer doubling, ceil(log2(cracks of the largest slice)) + 1 rounds, each round its
//      own launch from one pair of arrays into another.  No workgroup ever waits for another and nothing spins on a flag.
//   6  k_tr_weights        1 on the crack that starts a T5 run (and, T7, whose vertex is kept), and the loop is cut at its
//      leader; the same number of doubling rounds over the predecessor links ranks the list: every crack learns how many
//      vertices its loop has emitted up to and including it.
//   7  k_tr_loops at the leaders, a two-array exclusive scan over the crack ids (vertex offsets, contour numbers), READ-BACK 2:
//      {vertices, contours}, then k_tr_scatter writes vertices, rows and hole flags.
// Two host read-backs per extraction.  The only atomic is an integer atomicMax (pass 2); every output word is written by
// exactly one thread, so reruns are bit-identical.  Scratch: the table, and about 50 bytes per crack.
#pragma once

#include <algorithm>

namespace {

constexpr int TR_ROWS = 8;            // rows a thread of the streaming pass walks down
constexpr int TR_E = 16;              // elements per thread of the scan kernels
constexpr int TR_CHUNK = NT * TR_E;   // elements per block of the scan kernels
typedef unsigned long long tr_u64;

struct tr_desc {
  int row;   // (structure * nz + z) * ny + y
  int xs;    // x * 4 + side, sides N = 0, E = 1, S = 2, W = 3
};

// non-zero bytes of a word -> one bit each
__device__ __forceinline__ unsigned tr_nz4(unsigned w) {
  const unsigned t = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
  return (((t >> 7) * 0x01020408u) >> 24) & 0xfu;
}

// Pixels x0 - 1 ... x0 + 16 of a row as bits 0 ... 17 (outside the row: 0).  One 16-byte load where the address allows it.
__device__ __forceinline__ unsigned tr_bits18(const uint8_t* __restrict__ row, int x0, int nx) {
  const uint8_t* __restrict__ p = row + x0;
  unsigned f = 0u;
  if (x0 + 16 <= nx && reinterpret_cast<uintptr_t>(p) % 16 == 0) {
    const int4 w = *reinterpret_cast<const int4*>(p);
    f = tr_nz4((unsigned)w.x) | tr_nz4((unsigned)w.y) << 4 | tr_nz4((unsigned)w.z) << 8 | tr_nz4((unsigned)w.w) << 12;
  } else {
    const int n = nx - x0 < 16 ? nx - x0 : 16;
    for (int j = 0; j < n; ++j) f |= (unsigned)(p[j] != 0) << j;
  }
  f <<= 1;
  if (x0 > 0 && p[-1] != 0) f |= 1u;
  if (x0 + 16 < nx && p[16] != 0) f |= 1u << 17;
  return f;
}

// Pixels xb ... xb + 63 of a row as bits (outside the row: 0).
__device__ __forceinline__ tr_u64 tr_bits64(const uint8_t* __restrict__ row, int xb, int nx) {
  const uint8_t* __restrict__ p = row + xb;
  const int n = nx - xb < 64 ? nx - xb : 64;
  tr_u64 f = 0ull;
  if (n == 64 && reinterpret_cast<uintptr_t>(p) % 8 == 0) {
    const tr_u64* __restrict__ q = reinterpret_cast<const tr_u64*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const tr_u64 w = q[k];
      f |= (tr_u64)(tr_nz4((unsigned)w) | tr_nz4((unsigned)(w >> 32)) << 4) << (8 * k);
    }
  } else {
    for (int j = 0; j < n; ++j) f |= (tr_u64)(p[j] != 0) << j;
  }
  return f;
}

// Passes 1 and 3.  A work item is (slice, group of TR_ROWS rows, 64-pixel block); its four threads are neighbouring lanes.
// EMIT = false: table[row * nb + block] = the block's cracks.  EMIT = true: table holds the exclusive scan; desc[id] is written.
template <bool EMIT>
__global__ void __launch_bounds__(NT) k_tr_stream(const uint8_t* __restrict__ masks, int nx, int ny, int nb, int ngy, size_t nitems,
                                                  int* __restrict__ table, tr_desc* __restrict__ desc) {
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  const size_t item = t >> 2;
  const int strip = (int)(t & 3), q0 = (int)(threadIdx.x & 63u) & ~3;
  const bool live = item < nitems;
  int b = 0, g = 0;
  size_t slice = 0;
  if (live) {
    b = (int)(item % (size_t)nb);
    const size_t r = item / (size_t)nb;
    g = (int)(r % (size_t)ngy);
    slice = r / (size_t)ngy;
  }
  const int x0 = b * 64 + strip * 16, y0 = g * TR_ROWS;
  const bool has = live && x0 < nx;
  const uint8_t* __restrict__ base = masks + slice * (size_t)ny * nx;
  unsigned up = has && y0 > 0 ? tr_bits18(base + (size_t)(y0 - 1) * nx, x0, nx) : 0u;
  unsigned mid = has ? tr_bits18(base + (size_t)y0 * nx, x0, nx) : 0u;
  for (int r = 0; r < TR_ROWS; ++r) {   // (every lane of the wavefront runs all rounds: the exchanges below need them)
    const int y = y0 + r;
    const bool rowok = has && y < ny;
    const unsigned down = rowok && y + 1 < ny ? tr_bits18(base + (size_t)(y + 1) * nx, x0, nx) : 0u;
    const unsigned f = rowok ? (mid >> 1) & 0xffffu : 0u;
    const unsigned cn = f & ~(up >> 1), ce = f & ~(mid >> 2), cs = f & ~(down >> 1), cw = f & ~mid;
    const int cnt = __builtin_popcount(cn) + __builtin_popcount(ce) + __builtin_popcount(cs) + __builtin_popcount(cw);
    const int c0 = __shfl(cnt, q0), c1 = __shfl(cnt, q0 + 1), c2 = __shfl(cnt, q0 + 2), c3 = __shfl(cnt, q0 + 3);
    if (live && y < ny) {
      const size_t grow = slice * (size_t)ny + y;
      if (!EMIT) {
        if (strip == 0) table[grow * nb + b] = c0 + c1 + c2 + c3;
      } else if (cnt) {
        int id = table[grow * nb + b] + (strip > 0 ? c0 : 0) + (strip > 1 ? c1 : 0) + (strip > 2 ? c2 : 0);
        unsigned any = cn | ce | cs | cw;
        while (any) {
          const int j = __builtin_ctz(any);
          any &= any - 1u;
          const int xs = (x0 + j) << 2;
          if (cn >> j & 1u) desc[id++] = tr_desc{(int)grow, xs};
          if (ce >> j & 1u) desc[id++] = tr_desc{(int)grow, xs | 1};
          if (cs >> j & 1u) desc[id++] = tr_desc{(int)grow, xs | 2};
          if (cw >> j & 1u) desc[id++] = tr_desc{(int)grow, xs | 3};
        }
      }
    }
    up = mid;
    mid = down;
  }
}

// In-place exclusive scan of one or two int arrays (b may be NULL), reduce-then-scan: sums[2 c], sums[2 c + 1] of chunk c ...
__global__ void __launch_bounds__(NT) k_tr_chunk_sums(const int* __restrict__ a, const int* __restrict__ b, size_t n, tr_u64* __restrict__ sums) {
  __shared__ tr_u64 sa[NT], sb[NT];
  const size_t i0 = (size_t)blockIdx.x * TR_CHUNK + (size_t)threadIdx.x * TR_E;
  tr_u64 va = 0, vb = 0;
  for (int e = 0; e < TR_E; ++e)
    if (i0 + e < n) {
      va += (tr_u64)(unsigned)a[i0 + e];
      if (b) vb += (tr_u64)(unsigned)b[i0 + e];
    }
  sa[threadIdx.x] = va, sb[threadIdx.x] = vb;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sa[threadIdx.x] += sa[threadIdx.x + s], sb[threadIdx.x] += sb[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[2 * (size_t)blockIdx.x] = sa[0], sums[2 * (size_t)blockIdx.x + 1] = sb[0];
}

// ... one block turns the chunk sums into their exclusive scan, totals[0 ... 1] = the grand totals ...
__global__ void __launch_bounds__(NT) k_tr_scan_chunks(tr_u64* __restrict__ sums, size_t nchunks, tr_u64* __restrict__ totals) {
  __shared__ tr_u64 sa[NT], sb[NT];
  tr_u64 ca = 0, cb = 0;
  for (size_t t0 = 0; t0 < nchunks; t0 += NT) {
    const size_t k = t0 + threadIdx.x;
    const tr_u64 va = k < nchunks ? sums[2 * k] : 0, vb = k < nchunks ? sums[2 * k + 1] : 0;
    sa[threadIdx.x] = va, sb[threadIdx.x] = vb;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
      const tr_u64 ta = (int)threadIdx.x >= off ? sa[threadIdx.x - off] : 0, tb = (int)threadIdx.x >= off ? sb[threadIdx.x - off] : 0;
      __syncthreads();
      sa[threadIdx.x] += ta, sb[threadIdx.x] += tb;
      __syncthreads();
    }
    if (k < nchunks) sums[2 * k] = ca + sa[threadIdx.x] - va, sums[2 * k + 1] = cb + sb[threadIdx.x] - vb;
    const tr_u64 ta = sa[NT - 1], tb = sb[NT - 1];
    __syncthreads();
    ca += ta, cb += tb;
  }
  if (threadIdx.x == 0) totals[0] = ca, totals[1] = cb;
}

// ... and every chunk scans itself from its offset.  (Entries are non-negative; a total beyond int32 is refused by the host
// before anything reads the wrapped values.)
__global__ void __launch_bounds__(NT) k_tr_scan_apply(int* __restrict__ a, int* __restrict__ b, size_t n, const tr_u64* __restrict__ sums) {
  __shared__ int sa[NT], sb[NT];
  const size_t i0 = (size_t)blockIdx.x * TR_CHUNK + (size_t)threadIdx.x * TR_E;
  int va[TR_E], vb[TR_E];
  int ta = 0, tb = 0;
#pragma unroll
  for (int e = 0; e < TR_E; ++e) {
    va[e] = i0 + e < n ? a[i0 + e] : 0;
    vb[e] = b && i0 + e < n ? b[i0 + e] : 0;
    ta += va[e], tb += vb[e];
  }
  sa[threadIdx.x] = ta, sb[threadIdx.x] = tb;
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {
    const int ua = (int)threadIdx.x >= off ? sa[threadIdx.x - off] : 0, ub = (int)threadIdx.x >= off ? sb[threadIdx.x - off] : 0;
    __syncthreads();
    sa[threadIdx.x] += ua, sb[threadIdx.x] += ub;
    __syncthreads();
  }
  int ra = (int)(unsigned)sums[2 * (size_t)blockIdx.x] + sa[threadIdx.x] - ta;
  int rb = (int)(unsigned)sums[2 * (size_t)blockIdx.x + 1] + sb[threadIdx.x] - tb;
#pragma unroll
  for (int e = 0; e < TR_E; ++e)
    if (i0 + e < n) {
      a[i0 + e] = ra, ra += va[e];
      if (b) b[i0 + e] = rb, rb += vb[e];
    }
}

// Cracks of the largest slice, from the scanned table (per entries of it to a slice).
__global__ void __launch_bounds__(NT) k_tr_slice_max(const int* __restrict__ table, size_t nslices, size_t per, const tr_u64* __restrict__ totals,
                                                     int* __restrict__ out) {
  for (size_t s = (size_t)blockIdx.x * NT + threadIdx.x; s < nslices; s += (size_t)gridDim.x * NT) {
    const int lo = table[s * per], hi = s + 1 < nslices ? table[(s + 1) * per] : (int)(unsigned)totals[0];
    if (hi > lo) atomicMax(out, hi - lo);
  }
}

// The id of crack (x, y, side) of the row `row` (its pixel is foreground and has that crack): the table entry of its block plus
// the cracks of the pixels before it in the block, plus its own sides before `side`.
__device__ __forceinline__ int tr_crack_id(const uint8_t* __restrict__ masks, const int* __restrict__ table, int nx, int ny, int nb, size_t row,
                                           int y, int x, int side) {
  const int b = x >> 6, xb = b << 6, p = x & 63;
  const uint8_t* __restrict__ r = masks + row * (size_t)nx;
  const tr_u64 f = tr_bits64(r, xb, nx);
  const tr_u64 u = y > 0 ? tr_bits64(r - nx, xb, nx) : 0ull, d = y + 1 < ny ? tr_bits64(r + nx, xb, nx) : 0ull;
  const tr_u64 left = xb > 0 && r[xb - 1] != 0 ? 1ull : 0ull, right = xb + 64 < nx && r[xb + 64] != 0 ? 1ull << 63 : 0ull;
  const tr_u64 cn = f & ~u, cs = f & ~d, cw = f & ~(f << 1 | left), ce = f & ~(f >> 1 | right);
  const tr_u64 below = (1ull << p) - 1ull;
  int id = table[row * nb + b] + __builtin_popcountll(cn & below) + __builtin_popcountll(ce & below) + __builtin_popcountll(cs & below) +
           __builtin_popcountll(cw & below);
  if (side > 0) id += (int)(cn >> p & 1ull);
  if (side > 1) id += (int)(ce >> p & 1ull);
  if (side > 2) id += (int)(cs >> p & 1ull);
  return id;
}

// Pass 4 (T2).
__global__ void __launch_bounds__(NT) k_tr_succ(const uint8_t* __restrict__ masks, const int* __restrict__ table, const tr_desc* __restrict__ desc,
                                                size_t ncr, int nx, int ny, int nb, int* __restrict__ succ, int* __restrict__ pred) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < ncr; i += (size_t)gridDim.x * NT) {
    const tr_desc d = desc[i];
    const int x = d.xs >> 2, side = d.xs & 3, y = d.row % ny;
    const uint8_t* __restrict__ r = masks + (size_t)d.row * nx;
    const int dx = side == 0 ? 1 : side == 2 ? -1 : 0, dy = side == 1 ? 1 : side == 3 ? -1 : 0;   // the heading (T1)
    const int arx = x + dx, ary = y + dy, alx = arx + dy, aly = ary - dx;                          // left of (dx, dy) is (dy, -dx)
    auto fg = [&](int px, int py) { return px >= 0 && px < nx && py >= 0 && py < ny && r[(ptrdiff_t)(py - y) * nx + px] != 0; };
    int s;
    if (fg(alx, aly))
      s = tr_crack_id(masks, table, nx, ny, nb, (size_t)(d.row + (aly - y)), aly, alx, (side + 3) & 3);
    else if (fg(arx, ary))
      s = tr_crack_id(masks, table, nx, ny, nb, (size_t)(d.row + (ary - y)), ary, arx, side);
    else if (side < 3)
      s = (int)i + 1;                                                 // the pixel's next side is its next crack
    else
      s = (int)i - 1 - (fg(x + 1, y) ? 0 : 1) - (fg(x, y + 1) ? 0 : 1);   // W -> N of the same pixel: past its S and E cracks
    succ[i] = s;
    pred[s] = (int)i;
  }
}

// Pass 5: m = the minimum over, nxt = the crack after, twice as many cracks as before (m_in NULL: the crack itself).
__global__ void __launch_bounds__(NT) k_tr_min_round(const int* __restrict__ m_in, const int* __restrict__ n_in, int* __restrict__ m_out,
                                                     int* __restrict__ n_out, size_t ncr) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < ncr; i += (size_t)gridDim.x * NT) {
    const int j = n_in[i];
    const int a = m_in ? m_in[i] : (int)i, b = m_in ? m_in[j] : j;
    m_out[i] = a < b ? a : b;
    n_out[i] = n_in[j];
  }
}

// T4: the side pixel of a crack as (x, row).
__device__ __forceinline__ void tr_pix(const tr_desc d, bool hole, int& px, int& prow) {
  const int side = d.xs & 3;
  px = d.xs >> 2, prow = d.row;
  if (hole) {
    px += side == 1 ? 1 : side == 3 ? -1 : 0;
    prow += side == 2 ? 1 : side == 0 ? -1 : 0;
  }
}

// Pass 6: the weight of every crack (T5, T7) and the list cut at the leader.
__global__ void __launch_bounds__(NT) k_tr_weights(const tr_desc* __restrict__ desc, const int* __restrict__ lead, const int* __restrict__ succ,
                                                   const int* __restrict__ pred, int approximate, size_t ncr, int* __restrict__ val,
                                                   int* __restrict__ link) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < ncr; i += (size_t)gridDim.x * NT) {
    const int l = lead[i], p = pred[i];
    const bool hole = (desc[l].xs & 3) == 2;   // T3
    int cx, cr, px, pr;
    tr_pix(desc[i], hole, cx, cr);
    tr_pix(desc[p], hole, px, pr);
    int w = cx != px || cr != pr;              // a run starts here
    if (w && approximate) {
      int c = (int)i, qx = cx, qr = cr;        // the next vertex: a run has at most four cracks
      for (int k = 0; k < 4; ++k) {
        c = succ[c];
        tr_pix(desc[c], hole, qx, qr);
        if (qx != cx || qr != cr) break;
      }
      w = (cx - px != qx - cx) || (cr - pr != qr - cr);
    }
    val[i] = w;
    link[i] = (int)i == l ? -1 : p;
  }
}

__global__ void __launch_bounds__(NT) k_tr_rank_round(const int* __restrict__ v_in, const int* __restrict__ l_in, int* __restrict__ v_out,
                                                      int* __restrict__ l_out, size_t ncr) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < ncr; i += (size_t)gridDim.x * NT) {
    const int l = l_in[i];
    v_out[i] = l < 0 ? v_in[i] : v_in[i] + v_in[l];
    l_out[i] = l < 0 ? -1 : l_in[l];
  }
}

// Pass 7a.  rank = the inclusive weighted rank from the leader.  At a leader: the loop's vertex count, a 1 to number it by, and
// whether its vertices are stored rotated: the run that holds the leader started before it (on the far side of the cut) and
// its vertex is kept, so that vertex -- the last by rank -- is the contour's first.
__global__ void __launch_bounds__(NT) k_tr_loops(const tr_desc* __restrict__ desc, const int* __restrict__ lead, const int* __restrict__ pred,
                                                 const int* __restrict__ rank, size_t ncr, int* __restrict__ nvert, int* __restrict__ isleader,
                                                 uint8_t* __restrict__ rotated) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < ncr; i += (size_t)gridDim.x * NT) {
    if (lead[i] != (int)i) {
      nvert[i] = 0, isleader[i] = 0;
      continue;
    }
    const int n = rank[pred[i]];
    const bool hole = (desc[i].xs & 3) == 2;
    int rot = 0;
    if (n > 0 && rank[i] == 0) {
      int c = (int)i;
      bool found = false;
      for (int k = 0; k < 4 && !found; ++k) {
        const int p = pred[c];
        int cx, cr, px, pr;
        tr_pix(desc[c], hole, cx, cr);
        tr_pix(desc[p], hole, px, pr);
        if (cx != px || cr != pr) found = true;
        else c = p;
      }
      if (found && c != (int)i) rot = rank[c] - rank[pred[c]] == 1;
    }
    nvert[i] = n > 0 ? n : 1;   // (one run all around: a single pixel, one vertex)
    isleader[i] = 1;
    rotated[i] = (uint8_t)rot;
  }
}

// Pass 7b.  first / number: the exclusive scans of k_tr_loops' two arrays.
__global__ void __launch_bounds__(NT) k_tr_scatter(const tr_desc* __restrict__ desc, const int* __restrict__ lead, const int* __restrict__ pred,
                                                   const int* __restrict__ rank, const int* __restrict__ first, const int* __restrict__ number,
                                                   const uint8_t* __restrict__ rotated, size_t ncr, int ny, int nz, int* __restrict__ verts,
                                                   pp_contour* __restrict__ rows, uint8_t* __restrict__ holes) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < ncr; i += (size_t)gridDim.x * NT) {
    const int l = lead[i];
    const bool hole = (desc[l].xs & 3) == 2;
    const int n = rank[pred[l]], f = first[l];
    int px, prow;
    tr_pix(desc[i], hole, px, prow);
    if ((int)i == l) {
      const int k = number[l], slice = desc[l].row / ny;
      pp_contour c;
      c.first = f, c.count = n > 0 ? n : 1, c.structure = slice / nz, c.z = slice % nz;
      rows[k] = c;
      holes[k] = hole ? (uint8_t)1 : (uint8_t)0;
      if (n == 0) verts[2 * (size_t)f] = px, verts[2 * (size_t)f + 1] = prow % ny;
    }
    const int w = (int)i == l ? rank[i] : rank[i] - rank[pred[i]];
    if (w) {
      const int slot = rotated[l] ? rank[i] % n : rank[i] - 1;
      verts[2 * ((size_t)f + slot)] = px, verts[2 * ((size_t)f + slot) + 1] = prow % ny;
    }
  }
}

struct tr_plan {
  int nx, ny, nz, nb, ngy;
  size_t nslices, rows, entries, nitems, chunks1;
  // phase 1 scratch
  tr_u64* totals;   // {cracks, -, largest slice (an int), -}
  int* table;
  tr_u64* sums1;
};

int tr_phase1(pp_ctx* ctx, const uint8_t* masks, const tr_plan& p) {
  const dim3 b(NT);
  PP_HIP(ctx, hipMemsetAsync(p.totals, 0, 4 * sizeof(tr_u64), ctx->stream));
  {
    pp_prof_scope ps(ctx, "k_tr_stream_count");
    hipLaunchKernelGGL(k_tr_stream<false>, dim3((unsigned)((p.nitems * 4 + NT - 1) / NT)), b, 0, ctx->stream, masks, p.nx, p.ny, p.nb, p.ngy,
                       p.nitems, p.table, (tr_desc*)nullptr);
    PP_LAUNCH_CHECK(ctx, "k_tr_stream<false>");
  }
  pp_prof_scope ps(ctx, "tr_table_scan");
  hipLaunchKernelGGL(k_tr_chunk_sums, dim3((unsigned)p.chunks1), b, 0, ctx->stream, (const int*)p.table, (const int*)nullptr, p.entries, p.sums1);
  PP_LAUNCH_CHECK(ctx, "k_tr_chunk_sums");
  hipLaunchKernelGGL(k_tr_scan_chunks, dim3(1), b, 0, ctx->stream, p.sums1, p.chunks1, p.totals);
  PP_LAUNCH_CHECK(ctx, "k_tr_scan_chunks");
  hipLaunchKernelGGL(k_tr_scan_apply, dim3((unsigned)p.chunks1), b, 0, ctx->stream, p.table, (int*)nullptr, p.entries, (const tr_u64*)p.sums1);
  PP_LAUNCH_CHECK(ctx, "k_tr_scan_apply");
  hipLaunchKernelGGL(k_tr_slice_max, dim3(grid_for(p.nslices, 1024u)), b, 0, ctx->stream, (const int*)p.table, p.nslices, (size_t)p.ny * p.nb,
                     (const tr_u64*)p.totals, reinterpret_cast<int*>(p.totals + 2));
  PP_LAUNCH_CHECK(ctx, "k_tr_slice_max");
  return PP_OK;
}

// The whole extraction; the three tables stay in the context's scratch (ctx->trace says where).
int tr_run(pp_ctx* ctx, const uint8_t* masks, const int size[3], int nstructures, int approximate) {
  ctx->trace.valid = 0;
  tr_plan p;
  p.nx = size[0], p.ny = size[1], p.nz = size[2];
  p.nb = (p.nx + 63) / 64, p.ngy = (p.ny + TR_ROWS - 1) / TR_ROWS;
  p.nslices = (size_t)nstructures * p.nz;
  p.rows = p.nslices * p.ny;
  if (p.rows > 0x7fffffffu) return pp_fail(ctx, PP_ERR_SIZE, "pp_contour_trace_u8: more than 2^31 - 1 rows");
  p.entries = p.rows * p.nb;
  p.nitems = p.nslices * p.ngy * p.nb;
  p.chunks1 = (p.entries + TR_CHUNK - 1) / TR_CHUNK;
  if (p.nitems * 4 > 0xffffffffull) return pp_fail(ctx, PP_ERR_SIZE, "pp_contour_trace_u8: more than 2^32 threads in the streaming pass");
  const size_t need1 = 256 + pp_align_up(p.entries * sizeof(int), 256) + pp_align_up(p.chunks1 * 2 * sizeof(tr_u64), 256);
  int rc = pp_reserve(ctx, need1);
  if (rc) return rc;
  auto carve1 = [&](pp_carver& cv) {
    p.totals = cv.take<tr_u64>(4);
    p.table = cv.take<int>(p.entries);
    p.sums1 = cv.take<tr_u64>(p.chunks1 * 2);
  };
  pp_carver cv{ctx->ws, 0};
  carve1(cv);
  rc = tr_phase1(ctx, masks, p);
  if (rc) return rc;
  tr_u64 h[4];
  rc = pp_read_back(ctx, p.totals, h, sizeof(h));   // read-back 1
  if (rc) return rc;
  if (h[0] > 0x7fffffffull) return pp_fail(ctx, PP_ERR_ARG, "pp_contour_trace_u8: more than 2^31 - 1 cracks (%llu)", h[0]);
  const size_t ncr = (size_t)h[0];
  const int largest = (int)(unsigned)h[2];
  ctx->trace.cracks = (long long)ncr, ctx->trace.verts = 0, ctx->trace.contours = 0;
  if (ncr == 0) {
    ctx->trace.valid = 1;
    return PP_OK;
  }
  int rounds = 0;
  while (((long long)1 << rounds) < (long long)largest) ++rounds;
  rounds += 1;   // ceil(log2(cracks of the largest slice)) + 1: no loop is longer than its slice's cracks
  const size_t chunks2 = (ncr + TR_CHUNK - 1) / TR_CHUNK, maxloops = ncr / 4 + 1;
  const size_t need = need1 + pp_align_up(ncr * sizeof(tr_desc), 256) + 7 * pp_align_up(ncr * sizeof(int), 256) + pp_align_up(ncr, 256) +
                      pp_align_up(chunks2 * 2 * sizeof(tr_u64), 256) + 256 + pp_align_up(ncr * 2 * sizeof(int), 256) +
                      pp_align_up(maxloops * sizeof(pp_contour), 256) + pp_align_up(maxloops, 256);
  if (need > ctx->ws_bytes) {   // the scratch moves when it grows (the first call at a size): count again, without a read-back
    rc = pp_reserve(ctx, need);
    if (rc) return rc;
    cv = pp_carver{ctx->ws, 0};
    carve1(cv);
    rc = tr_phase1(ctx, masks, p);
    if (rc) return rc;
  }
  tr_desc* desc = cv.take<tr_desc>(ncr);
  int* arr[7];
  for (int k = 0; k < 7; ++k) arr[k] = cv.take<int>(ncr);
  uint8_t* rotated = cv.take<uint8_t>(ncr);
  tr_u64* sums2 = cv.take<tr_u64>(chunks2 * 2);
  tr_u64* totals2 = cv.take<tr_u64>(2);
  const size_t off_verts = cv.off;
  int* verts = cv.take<int>(ncr * 2);
  const size_t off_rows = cv.off;
  pp_contour* rows = cv.take<pp_contour>(maxloops);
  const size_t off_holes = cv.off;
  uint8_t* holes = cv.take<uint8_t>(maxloops);
  const dim3 b(NT), g(grid_for(ncr, 16384u));
  {
    pp_prof_scope ps(ctx, "k_tr_stream_emit");
    hipLaunchKernelGGL(k_tr_stream<true>, dim3((unsigned)((p.nitems * 4 + NT - 1) / NT)), b, 0, ctx->stream, masks, p.nx, p.ny, p.nb, p.ngy,
                       p.nitems, p.table, desc);
    PP_LAUNCH_CHECK(ctx, "k_tr_stream<true>");
  }
  int *succ = arr[0], *pred = arr[1];
  {
    pp_prof_scope ps(ctx, "k_tr_succ");
    hipLaunchKernelGGL(k_tr_succ, g, b, 0, ctx->stream, masks, (const int*)p.table, (const tr_desc*)desc, ncr, p.nx, p.ny, p.nb, succ, pred);
    PP_LAUNCH_CHECK(ctx, "k_tr_succ");
  }
  const int *mi = nullptr, *ni = succ;
  int *mo = arr[2], *no = arr[3], *mo2 = arr[4], *no2 = arr[5];
  {
    pp_prof_scope ps(ctx, "tr_leader_rounds");
    for (int k = 0; k < rounds; ++k) {
      hipLaunchKernelGGL(k_tr_min_round, g, b, 0, ctx->stream, mi, ni, mo, no, ncr);
      PP_LAUNCH_CHECK(ctx, "k_tr_min_round");
      mi = mo, ni = no;
      std::swap(mo, mo2), std::swap(no, no2);
    }
  }
  const int* lead = mi;
  // free now: (mo, no), the array behind ni, arr[6]
  const int *vi = mo, *li = no;
  int *vo = const_cast<int*>(ni), *lo = arr[6], *vo2 = mo, *lo2 = no;
  {
    pp_prof_scope ps(ctx, "tr_rank_rounds");
    hipLaunchKernelGGL(k_tr_weights, g, b, 0, ctx->stream, (const tr_desc*)desc, lead, (const int*)succ, (const int*)pred, approximate != 0, ncr, mo, no);
    PP_LAUNCH_CHECK(ctx, "k_tr_weights");
    for (int k = 0; k < rounds; ++k) {
      hipLaunchKernelGGL(k_tr_rank_round, g, b, 0, ctx->stream, vi, li, vo, lo, ncr);
      PP_LAUNCH_CHECK(ctx, "k_tr_rank_round");
      vi = vo, li = lo;
      std::swap(vo, vo2), std::swap(lo, lo2);
    }
  }
  const int* rank = vi;
  int *nvert = succ, *number = vo;   // (the successors are no longer needed; vo is the pair not holding the ranks)
  {
    pp_prof_scope ps(ctx, "tr_output");
    hipLaunchKernelGGL(k_tr_loops, g, b, 0, ctx->stream, (const tr_desc*)desc, lead, (const int*)pred, rank, ncr, nvert, number, rotated);
    PP_LAUNCH_CHECK(ctx, "k_tr_loops");
    hipLaunchKernelGGL(k_tr_chunk_sums, dim3((unsigned)chunks2), b, 0, ctx->stream, (const int*)nvert, (const int*)number, ncr, sums2);
    PP_LAUNCH_CHECK(ctx, "k_tr_chunk_sums");
    hipLaunchKernelGGL(k_tr_scan_chunks, dim3(1), b, 0, ctx->stream, sums2, chunks2, totals2);
    PP_LAUNCH_CHECK(ctx, "k_tr_scan_chunks");
    hipLaunchKernelGGL(k_tr_scan_apply, dim3((unsigned)chunks2), b, 0, ctx->stream, nvert, number, ncr, (const tr_u64*)sums2);
    PP_LAUNCH_CHECK(ctx, "k_tr_scan_apply");
    hipLaunchKernelGGL(k_tr_scatter, g, b, 0, ctx->stream, (const tr_desc*)desc, lead, (const int*)pred, rank, (const int*)nvert, (const int*)number,
                       (const uint8_t*)rotated, ncr, p.ny, p.nz, verts, rows, holes);
    PP_LAUNCH_CHECK(ctx, "k_tr_scatter");
  }
  tr_u64 t2[2];
  rc = pp_read_back(ctx, totals2, t2, sizeof(t2));   // read-back 2
  if (rc) return rc;
  ctx->trace.verts = (long long)t2[0], ctx->trace.contours = (long long)t2[1];
  ctx->trace.off_verts = off_verts, ctx->trace.off_rows = off_rows, ctx->trace.off_holes = off_holes;
  ctx->trace.valid = 1;
  return PP_OK;
}

}  // namespace

extern "C" {

int pp_contour_trace_u8(pp_ctx* ctx, const uint8_t* masks, const int size[3], int nstructures, int approximate, int32_t* vertices,
                        int nverts, pp_contour* contours, uint8_t* hole, int ncontours, int64_t counts[3]) {
  if (!ctx) return PP_ERR_ARG;
  pp_device_guard dev_guard_(ctx);
  PP_REQUIRE(ctx, masks && size && counts, "pp_contour_trace_u8: NULL argument");
  PP_REQUIRE(ctx, nstructures >= 1, "pp_contour_trace_u8: at least one structure");
  PP_REQUIRE(ctx, size[0] > 0 && size[1] > 0 && size[2] > 0, "pp_contour_trace_u8: empty volume");
  PP_REQUIRE(ctx, nverts >= 0 && ncontours >= 0, "pp_contour_trace_u8: a negative count");
  PP_REQUIRE(ctx, (vertices || nverts == 0) && ((contours && hole) || ncontours == 0), "pp_contour_trace_u8: NULL table");
  if (size[0] > CT_MAX_INDEX || size[1] > CT_MAX_INDEX || size[2] > CT_MAX_INDEX)
    return pp_fail(ctx, PP_ERR_SIZE, "pp_contour_trace_u8: an axis longer than 2^24");
  const bool fill = vertices || contours || hole || nverts || ncontours;
  const bool kept = ctx->trace.valid && ctx->trace.masks == masks && ctx->trace.size[0] == size[0] && ctx->trace.size[1] == size[1] &&
                    ctx->trace.size[2] == size[2] && ctx->trace.nstructures == nstructures && ctx->trace.approximate == (approximate != 0);
  if (!(fill && kept)) {   // a fill call right after its count call finds the tables still in the scratch
    const int rc = tr_run(ctx, masks, size, nstructures, approximate);
    if (rc) return rc;
    ctx->trace.masks = masks, ctx->trace.nstructures = nstructures, ctx->trace.approximate = approximate != 0;
    for (int a = 0; a < 3; ++a) ctx->trace.size[a] = size[a];
  }
  counts[0] = ctx->trace.cracks, counts[1] = ctx->trace.verts, counts[2] = ctx->trace.contours;
  if (!fill) return PP_OK;
  ctx->trace.valid = 0;   // (a result is fetched once)
  if (nverts != counts[1] || ncontours != counts[2])
    return pp_fail(ctx, PP_ERR_ARG, "pp_contour_trace_u8: tables for %d vertices and %d contours, the masks have %lld and %lld", nverts, ncontours,
                   (long long)counts[1], (long long)counts[2]);
  if (ncontours == 0) return PP_OK;
  pp_prof_scope ps(ctx, "tr_copy_out");
  PP_HIP(ctx, hipMemcpyAsync(vertices, ctx->ws + ctx->trace.off_verts, (size_t)nverts * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(contours, ctx->ws + ctx->trace.off_rows, (size_t)ncontours * sizeof(pp_contour), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipMemcpyAsync(hole, ctx->ws + ctx->trace.off_holes, (size_t)ncontours, hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PP_OK;
}

}  // extern "C"
