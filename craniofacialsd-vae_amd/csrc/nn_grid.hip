// Exact nearest neighbour over a uniform grid (gfx950): the search of
// chamfer.hip for DENSE point sets.  Same result, bit for bit -- distance and
// index, lowest index among bit-equal distances -- at a cost that follows the
// points near a query instead of all of them.
//
// Build (cfsd_nn_grid_build).  Every batch element gets a grid of gx x gy x gz
// cells over its own bounding box.  Stage CELLS: one workgroup per element
// reduces the box and writes the header (lo, cell size h, inverse cell size
// inv, extent), a second launch writes every point's cell id
//     c_a = min(trunc(fl(fl(p_a - lo_a) * inv_a)), g_a - 1),  id = (c_z gy + c_y) gx + c_x.
// The caller sorts the ids (stable; any order inside a cell gives the same
// query results, see below).  Stage GROUP: cell_start[c] = the first sorted
// position whose id is >= c (a binary search per cell), and the points in
// sorted order as 16-byte records (x, y, z, original index), so that a lane
// fetches a point with one global_load_dwordx4.  Nothing is read back.
// An axis whose extent is not in [1e-30, 1e30] (zero: planar, collinear,
// coincident or single points; or not finite) gets inv = h = 0: every point
// lies in cell 0 of it and the query treats it as one cell wide.
//
// Query (nn_points_grid_k).  One lane owns one query.  It locates its cell c
// (clamped into the grid) and visits the cells of the box [c - k, c + k],
// k = 0, 1, ..., shell by shell; cells along x are contiguous in the record
// list, so a row of a shell is one cell_start pair and one run of records.
// Every visited point is evaluated with nn_dist (nn_dist.h, the brute-force
// kernel's own sequence) and the best is the lexicographic minimum of
// (dist2 bits, original index): independent of the visiting order.
//
// The stopping rule and its margin.  u = 2^-24.  After shell k an unvisited
// point p lies in a cell beyond one of the (at most six) faces of the visited
// box that are not on the grid's boundary.  Take the +x face, cells >= i:
//   c_x >= i  =>  fl(t inv) >= i with t = fl(p - lo) = (p - lo)(1 + d1), so
//   (p - lo)(1 + d1)(1 + d2) inv >= i;  inv = (g / ext)(1 + d3) and
//   h = (ext / g)(1 + d4) give  p - lo >= i h (1 - u)^4 >= fl(i h)(1 - 5.01 u).
//   (-x face, cells < i <= g - 1, not reached by the clamp: p - lo <
//   fl(i h)(1 + 5.01 u) the same way.  ext in [1e-30, 1e30] and g <= 128 keep
//   inv, h and i h away from overflow and underflow.)
// The query holds s = fl(q - lo) = (q - lo)(1 + d6) and G = fl(fl(i h) - s).
// The true gap along x is  (p - lo) - (q - lo) >= fl(i h) - s
// - 5.01 u fl(i h) - 1.01 u |s| >= G - 6.03 u (ext + |s|), using fl(i h) <=
// ext (1 + 2u) and u G <= 1.01 u (ext + |s|).  With the slack
//   e = fl(2^-20 fl(ext + |s|)) >= 15.9 u (ext + |s|)
// L = max(fl(G - e), 0) <= G - 14.8 u (ext + |s|) <= the true |p_x - q_x|.
// The computed distance of that pair, d = nn_dist(q, p), loses at most one
// rounding per difference, product and sum (all terms non-negative, no
// cancellation): d >= |p - q|^2 (1 - 5.01 u) >= L^2 (1 - 5.01 u), while
//   bound = fl(fl(L L) (1 - 2^-20)) <= L^2 (1 + u)^2 (1 - 16 u) <= L^2 (1 - 13.9 u) <= d.
// (bound < 1e-30 is taken as 0: the products above stay in the normal range.)
// The same holds with L^2 replaced by the sum of the squared gaps of two or
// three axes (one more rounding per sum: (1 + u)^4 (1 - 16 u) <= 1 - 11.9 u),
// which is how a row of cells, and the cells at a row's ends, are skipped
// INSIDE a shell once nothing in them can win or tie (grid_cell_gap,
// grid_beyond): the walk reads the cells of a sphere around the query, not
// of the cube that holds it.
// So with kMargin = 2^-20 in both places every unvisited point has d >= the
// smallest bound over the open faces, and the lane stops only when
//   best < bound   (STRICT),
// i.e. when every unvisited point is strictly farther in computed bits: a
// point at exactly the bound with a lower index is never skipped.  A face on
// the grid's boundary has nothing beyond it; with no open face everything was
// visited.  A NaN anywhere makes the comparison false, so the lane walks on:
// the shell loop is bounded by max(gx, gy, gz), at which the box covers the
// grid whatever c is, and terminates for any input.
//
// Per-lane loads and occupancy.  Lanes of a wave diverge (each walks its own
// rows), so the kernel is latency bound: it keeps four independent 16-byte
// record loads in flight per lane (indices past the run clamped to its last
// record; re-evaluating a record cannot change a lexicographic minimum) and
// uses no LDS and no barrier, so that the other waves of a SIMD cover a
// wave's load latency: 256-thread workgroups, 103 VGPRs, 4 waves per SIMD
// (the per-axis state of the pruning costs the registers; forcing 6 or 8
// waves spills).
#include <math.h>

#include "cfsd_common.h"
#include "nn_dist.h"

namespace cfsd {

constexpr int kGridMax = CFSD_NN_GRID_MAX;  // cells per axis
constexpr int kGridHdr = CFSD_NN_GRID_HDR;  // floats per header: lo, h, inv, ext as four xyz0
constexpr float kMargin = 0x1p-20f;         // derived above
constexpr float kExtMin = 1e-30f, kExtMax = 1e30f;
constexpr int kGridBlock = 256;
constexpr int kHdrBlock = 1024;

struct GridLayout {
  size_t rec, hdr, start, ids, total;  // byte offsets into the grid buffer
  long ncell;
};

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// Byte layout of a grid buffer (cfsd.h): a function of the shapes alone.
static GridLayout grid_layout(int br, int p, int gx, int gy, int gz) {
  GridLayout l;
  l.ncell = (long)gx * gy * gz;
  l.rec = 0;
  l.hdr = (size_t)br * p * 16;
  l.start = l.hdr + (size_t)br * kGridHdr * 4;
  l.ids = l.start + align16((size_t)br * (l.ncell + 1) * 4);
  l.total = l.ids + align16((size_t)br * p * 4);
  return l;
}

// Cell of coordinate v along one axis: NaN and anything outside the box land
// inside [0, g - 1] (fmaxf / fminf return their non-NaN operand).
__device__ __forceinline__ int grid_cell(float s, float inv, int g) {
#pragma clang fp contract(off)
  return (int)fminf(fmaxf(s * inv, 0.f), (float)(g - 1));
}

// One workgroup per batch element: bounding box -> header.
__global__ __launch_bounds__(kHdrBlock) void grid_header_k(const float* __restrict__ r, float* __restrict__ hdr, int p,
                                                           int gx, int gy, int gz) {
  __shared__ float red[6][kHdrBlock / 64];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const float* rp = r + (long)b * p * 3;
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int j = tid; j < p; j += kHdrBlock) {
    float c[3];
    ld_row<3>(rp + (long)j * 3, c);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = fminf(v[a], c[a]);
      v[3 + a] = fmaxf(v[3 + a], c[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    for (int o = 32; o > 0; o >>= 1) {
      const float w = __shfl_xor(v[a], o);
      v[a] = a < 3 ? fminf(v[a], w) : fmaxf(v[a], w);
    }
    if ((tid & 63) == 0) red[a][tid >> 6] = v[a];
  }
  __syncthreads();
  if (tid < 3) {
#pragma clang fp contract(off)
    float lo = INFINITY, hi = -INFINITY;
    for (int w = 0; w < kHdrBlock / 64; ++w) {
      lo = fminf(lo, red[tid][w]);
      hi = fmaxf(hi, red[3 + tid][w]);
    }
    const float g = (float)(tid == 0 ? gx : tid == 1 ? gy : gz);
    float ext = hi - lo;
    const bool ok = ext >= kExtMin && ext <= kExtMax;  // false for NaN too
    if (!ok) ext = 0.f;
    float* h = hdr + (long)b * kGridHdr;
    h[tid] = lo;
    h[4 + tid] = ok ? ext / g : 0.f;
    h[8 + tid] = ok ? g / ext : 0.f;
    h[12 + tid] = ext;
  } else if (tid < 7) {
    hdr[(long)b * kGridHdr + (tid - 3) * 4 + 3] = 0.f;
  }
}

// One thread per point (b, j): its cell id.
__global__ __launch_bounds__(kGridBlock) void grid_cells_k(const float* __restrict__ r, const float* __restrict__ hdr,
                                                           int* __restrict__ ids, int p, long total, int gx, int gy,
                                                           int gz) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * kGridBlock + threadIdx.x;
  if (t >= total) return;
  const int b = (int)(t / p);
  const float* h = hdr + (long)b * kGridHdr;
  float c[3];
  ld_row<3>(r + t * 3, c);
  const int cx = grid_cell(c[0] - h[0], h[8], gx);
  const int cy = grid_cell(c[1] - h[1], h[9], gy);
  const int cz = grid_cell(c[2] - h[2], h[10], gz);
  ids[t] = (cz * gy + cy) * gx + cx;
}

// After the sort.  Thread (b, e): e < p writes record e of element b (the
// point order[b, e], clamped into range); e <= ncell writes cell_start[b, e],
// the first sorted position whose id is >= e.
__global__ __launch_bounds__(kGridBlock) void grid_group_k(const float* __restrict__ r,
                                                           const int* __restrict__ sorted_ids,
                                                           const int64_t* __restrict__ order,
                                                           f32x4* __restrict__ rec, int* __restrict__ start, int p,
                                                           int ncell, int per) {
  const int b = (int)blockIdx.y;
  const int e = (int)blockIdx.x * kGridBlock + (int)threadIdx.x;
  if (e >= per) return;
  if (e < p) {
    const long j = min(max((long)order[(long)b * p + e], 0L), (long)p - 1);
    float c[3];
    ld_row<3>(r + ((long)b * p + j) * 3, c);
    rec[(long)b * p + e] = (f32x4){c[0], c[1], c[2], __int_as_float((int)j)};
  }
  if (e <= ncell) {
    const int* s = sorted_ids + (long)b * p;
    int lo = 0, hi = p;  // first position with s[pos] >= e
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s[mid] < e) lo = mid + 1;
      else hi = mid;
    }
    start[(long)b * (ncell + 1) + e] = lo;
  }
}

struct GridBest {
  float d;
  int j;
};

// Lexicographic minimum of (dist2, original index).
__device__ __forceinline__ void grid_take(GridBest& best, float qx, float qy, float qz, f32x4 rc) {
  const float d = nn_dist<float>(qx, qy, qz, rc.x, rc.y, rc.z);
  const int j = __float_as_int(rc.w);
  if (d < best.d || (d == best.d && j < best.j)) {
    best.d = d;
    best.j = j;
  }
}

// The records [a, b) of one run, four loads in flight.
__device__ __forceinline__ void grid_run(GridBest& best, int& cnt, const f32x4* __restrict__ rec, int a, int b, int p,
                                         float qx, float qy, float qz) {
  a = min(max(a, 0), p);
  b = min(max(b, a), p);
  const int last = b - 1;
  for (int e = a; e < b; e += 4) {
    const f32x4 r0 = rec[e], r1 = rec[min(e + 1, last)], r2 = rec[min(e + 2, last)], r3 = rec[min(e + 3, last)];
    grid_take(best, qx, qy, qz, r0);
    grid_take(best, qx, qy, qz, r1);
    grid_take(best, qx, qy, qz, r2);
    grid_take(best, qx, qy, qz, r3);
    cnt += min(4, b - e);
  }
}

// Lower bound on the distance along one axis to anything beyond the open
// faces of [c - k, c + k] (L of the derivation at the top); +inf without one.
// fmaxf(NaN, 0) = 0: a gap that is not a number bounds nothing.
__device__ __forceinline__ float grid_axis_bound(float s, float h, float slack, int c, int k, int ne, bool& open) {
#pragma clang fp contract(off)
  float m = INFINITY;
  if (c - k > 0) {
    open = true;
    const float face = (float)(c - k) * h;
    const float gap = s - face;
    m = fmaxf(gap - slack, 0.f);
  }
  if (c + k < ne - 1) {
    open = true;
    const float face = (float)(c + k + 1) * h;
    const float gap = face - s;
    m = fminf(m, fmaxf(gap - slack, 0.f));
  }
  return m;
}

// Lower bound on |p_a - q_a| over the points of cell t of one axis, c the
// query's cell: L of the derivation with the face between t and c (cells > c:
// claim A with i = t; cells < c: claim B with i = t + 1 <= c); 0 for t = c.
__device__ __forceinline__ float grid_cell_gap(float s, float h, float slack, int c, int t) {
#pragma clang fp contract(off)
  if (t == c) return 0.f;
  const float face = (float)(t > c ? t : t + 1) * h;
  const float gap = t > c ? face - s : s - face;
  return fmaxf(gap - slack, 0.f);
}

// True when `best` is STRICTLY below the computed distance of every point
// whose per-axis gaps have squares summing to l2 (at most three terms): the
// bound of the derivation, fl(l2 (1 - 2^-20)) <= l2 (1 + u)^4 (1 - 16 u) <= d.
__device__ __forceinline__ bool grid_beyond(float best, float l2) {
#pragma clang fp contract(off)
  const float bound = l2 * (1.f - kMargin);
  return bound >= 1e-30f && best < bound;  // false for NaN
}

// Block (b, qb): queries [qb * 256, +256) of batch b against the grid of
// batch b (or the single shared one: g_bs = 0, like q_bs = 0).  Query i writes
// its result at position q_perm[i] (i itself without q_perm) of row b.
__global__ __launch_bounds__(kGridBlock) void nn_points_grid_k(
    const float* __restrict__ q, const float* __restrict__ hdr, const int* __restrict__ start,
    const f32x4* __restrict__ rec, const int* __restrict__ q_perm, float* __restrict__ dist2, int* __restrict__ idx,
    int* __restrict__ count, int n, int p, long q_bs, int g_shared, int gx, int gy, int gz, int ncell, int qblocks) {
#pragma clang fp contract(off)
  const int blk = (int)blockIdx.x;
  const int b = blk / qblocks, qb = blk - b * qblocks;
  const int i = qb * kGridBlock + (int)threadIdx.x;
  if (i >= n) return;
  const long gb = g_shared ? 0 : b;
  const float* h = hdr + gb * kGridHdr;
  const int* cs = start + gb * ((long)ncell + 1);
  const f32x4* rc = rec + gb * p;
  const f32x4 lo = ld4(h), hh = ld4(h + 4), inv = ld4(h + 8), ext = ld4(h + 12);
  float qv[3];
  ld_row<3>(q + (long)b * q_bs + (long)i * 3, qv);
  const float qx = qv[0], qy = qv[1], qz = qv[2];
  const float sx = qx - lo.x, sy = qy - lo.y, sz = qz - lo.z;
  // an axis without extent is one cell wide
  const int nex = inv.x > 0.f ? gx : 1, ney = inv.y > 0.f ? gy : 1, nez = inv.z > 0.f ? gz : 1;
  const int cx = grid_cell(sx, inv.x, nex), cy = grid_cell(sy, inv.y, ney), cz = grid_cell(sz, inv.z, nez);
  const float ex = kMargin * (ext.x + fabsf(sx)), ey = kMargin * (ext.y + fabsf(sy)),
              ez = kMargin * (ext.z + fabsf(sz));
  GridBest best = {INFINITY, 0};
  int cnt = 0;
  const int kmax = max(gx, max(gy, gz));
  for (int k = 0; k < kmax; ++k) {
    const int x0 = max(cx - k, 0), x1 = min(cx + k, nex - 1);
    const int y0 = max(cy - k, 0), y1 = min(cy + k, ney - 1);
    const int z0 = max(cz - k, 0), z1 = min(cz + k, nez - 1);
    for (int z = z0; z <= z1; ++z) {
      const bool zface = z == cz - k || z == cz + k;
      const float lz = grid_cell_gap(sz, hh.z, ez, cz, z), lz2 = lz * lz;
      for (int y = y0; y <= y1; ++y) {
        const float ly = grid_cell_gap(sy, hh.y, ey, cy, y), l2 = ly * ly + lz2;
        if (grid_beyond(best.d, l2)) continue;  // nothing in this row can win or tie
        const int row = (z * gy + y) * gx;
        int ra[2] = {0, 0}, rb[2] = {0, 0};  // the row's runs of records
        if (zface || y == cy - k || y == cy + k) {  // a row new in this shell: one run, ends trimmed
          int xa = x0, xb = x1;
          for (; xa < cx; ++xa) {
            const float lx = grid_cell_gap(sx, hh.x, ex, cx, xa);
            if (!grid_beyond(best.d, l2 + lx * lx)) break;
          }
          for (; xb > cx; --xb) {
            const float lx = grid_cell_gap(sx, hh.x, ex, cx, xb);
            if (!grid_beyond(best.d, l2 + lx * lx)) break;
          }
          ra[0] = cs[row + xa];
          rb[0] = cs[row + xb + 1];
        } else {  // a row seen before: its two end cells
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int x = t ? cx + k : cx - k;
            if (x < 0 || x > nex - 1) continue;
            const float lx = grid_cell_gap(sx, hh.x, ex, cx, x);
            if (grid_beyond(best.d, l2 + lx * lx)) continue;
            ra[t] = cs[row + x];
            rb[t] = cs[row + x + 1];
          }
        }
#pragma unroll 1
        for (int t = 0; t < 2; ++t) grid_run(best, cnt, rc, ra[t], rb[t], p, qx, qy, qz);
      }
    }
    bool open = false;
    float m = grid_axis_bound(sx, hh.x, ex, cx, k, nex, open);
    const float my = grid_axis_bound(sy, hh.y, ey, cy, k, ney, open);
    const float mz = grid_axis_bound(sz, hh.z, ez, cz, k, nez, open);
    if (!open) break;  // the box covers the grid
    m = fminf(m, fminf(my, mz));
    if (grid_beyond(best.d, m * m)) break;
  }
  const long o = (long)b * n + (q_perm ? min(max(q_perm[i], 0), n - 1) : i);
  dist2[o] = best.d;
  idx[o] = best.j;
  if (count) count[o] = cnt;
}

static int grid_check(const char* what, int br, int p, int gx, int gy, int gz) {
  if (br <= 0 || p <= 0 || br > 65535)
    return set_error(CFSD_EINVAL, "%s: bad sizes br=%d p=%d (1 <= br <= 65535, p >= 1)", what, br, p);
  if (gx < 1 || gy < 1 || gz < 1 || gx > kGridMax || gy > kGridMax || gz > kGridMax)
    return set_error(CFSD_EINVAL, "%s: cells (%d, %d, %d) outside 1..%d", what, gx, gy, gz, kGridMax);
  if ((long)br * p * 4 >= (1L << 31) || (long)br * ((long)gx * gy * gz + 1) >= (1L << 31))
    return set_error(CFSD_EINVAL, "%s: br x points x 4 or br x cells >= 2^31 (32-bit indices)", what);
  return CFSD_OK;
}

}  // namespace cfsd

using namespace cfsd;

extern "C" size_t cfsd_nn_grid_build_workspace(int br, int p, int gx, int gy, int gz) {
  if (br <= 0 || br > 65535 || p <= 0) return 0;
  if (gx < 1 || gy < 1 || gz < 1 || gx > kGridMax || gy > kGridMax || gz > kGridMax) return 0;
  if ((long)br * p * 4 >= (1L << 31) || (long)br * ((long)gx * gy * gz + 1) >= (1L << 31)) return 0;
  return grid_layout(br, p, gx, gy, gz).total;
}

extern "C" int cfsd_nn_grid_build(const float* r, void* grid, size_t grid_bytes, int stage, const int32_t* sorted_ids,
                                  const int64_t* order, int br, int p, int gx, int gy, int gz, void* stream) {
  if (!r || !grid) return set_error(CFSD_EINVAL, "nn_grid_build: null pointer");
  if (int rc = grid_check("nn_grid_build", br, p, gx, gy, gz)) return rc;
  const GridLayout l = grid_layout(br, p, gx, gy, gz);
  if (grid_bytes < l.total)
    return set_error(CFSD_EWORKSPACE, "nn_grid_build: grid buffer %zu < %zu bytes", grid_bytes, l.total);
  if ((uintptr_t)grid & 15) return set_error(CFSD_EINVAL, "nn_grid_build: the grid buffer must be 16-byte aligned");
  char* base = (char*)grid;
  float* hdr = (float*)(base + l.hdr);
  const hipStream_t st = (hipStream_t)stream;
  const long total = (long)br * p;
  if (stage == CFSD_NN_GRID_CELLS) {
    hipLaunchKernelGGL(grid_header_k, dim3((unsigned)br), dim3(kHdrBlock), 0, st, r, hdr, p, gx, gy, gz);
    hipLaunchKernelGGL(grid_cells_k, dim3((unsigned)((total + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, st,
                       r, (const float*)hdr, (int*)(base + l.ids), p, total, gx, gy, gz);
    return launch_status("nn_grid_build");
  }
  if (stage != CFSD_NN_GRID_GROUP) return set_error(CFSD_EINVAL, "nn_grid_build: stage %d", stage);
  if (!sorted_ids || !order) return set_error(CFSD_EINVAL, "nn_grid_build: the group stage needs the sorted ids");
  const long per = l.ncell + 1 > p ? l.ncell + 1 : p;
  hipLaunchKernelGGL(grid_group_k, dim3((unsigned)((per + kGridBlock - 1) / kGridBlock), (unsigned)br),
                     dim3(kGridBlock), 0, st, r, sorted_ids, order, (f32x4*)(base + l.rec), (int*)(base + l.start), p,
                     (int)l.ncell, (int)per);
  return launch_status("nn_grid_build");
}

extern "C" int cfsd_nn_points_grid(const float* q, const void* grid, size_t grid_bytes, const int32_t* q_perm,
                                   float* dist2, int32_t* idx, int32_t* count, int batch, int bq, int br, int n,
                                   int p, int gx, int gy, int gz, void* stream) {
  if (!q || !grid || !dist2 || !idx) return set_error(CFSD_EINVAL, "nn_points_grid: null pointer");
  if (batch <= 0 || n <= 0)
    return set_error(CFSD_EINVAL, "nn_points_grid: bad sizes batch=%d n=%d (both must be >= 1)", batch, n);
  if ((bq != 1 && bq != batch) || (br != 1 && br != batch))
    return set_error(CFSD_EINVAL, "nn_points_grid: operand batches %d and %d must each be 1 or %d", bq, br, batch);
  if (int rc = grid_check("nn_points_grid", br, p, gx, gy, gz)) return rc;
  if ((long)batch * n * 3 >= (1L << 31))
    return set_error(CFSD_EINVAL, "nn_points_grid: batch x points x 3 >= 2^31 (32-bit indices)");
  const GridLayout l = grid_layout(br, p, gx, gy, gz);
  if (grid_bytes < l.total)
    return set_error(CFSD_EWORKSPACE, "nn_points_grid: grid buffer %zu < %zu bytes", grid_bytes, l.total);
  if ((uintptr_t)grid & 15) return set_error(CFSD_EINVAL, "nn_points_grid: the grid buffer must be 16-byte aligned");
  const int qblocks = (n + kGridBlock - 1) / kGridBlock;
  const long blocks = (long)batch * qblocks;
  if (blocks >= (1L << 31)) return set_error(CFSD_EINVAL, "nn_points_grid: too many workgroups");
  const char* base = (const char*)grid;
  hipLaunchKernelGGL(nn_points_grid_k, dim3((unsigned)blocks), dim3(kGridBlock), 0, (hipStream_t)stream, q,
                     (const float*)(base + l.hdr), (const int*)(base + l.start), (const f32x4*)(base + l.rec), q_perm,
                     dist2, idx, count, n, p, bq == 1 ? 0L : (long)n * 3, br == 1 ? 1 : 0, gx, gy, gz, (int)l.ncell,
                     qblocks);
  return launch_status("nn_points_grid");
}
