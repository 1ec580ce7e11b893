// t-SNE of the latent space (gfx950): scikit-learn 1.7.2's TSNE with
// method='barnes_hut' at angle = 0 -- kNN-sparse input affinities, EXACT
// repulsion, two output dimensions (degrees_of_freedom = 1) -- the second
// branch of the reference's plot_embeddings (test.py:1177-1180).
//
// Five kernels.  Two run once per fit:
//   knn_rows_k     brute-force k nearest rows in difference form, the k best of
//                  every row kept as a sorted list of (d2, index) keys in LDS;
//   affinities_k   _binary_search_perplexity (sklearn/manifold/_utils.pyx), one
//                  wave per row, the search in float64.
// Three run per gradient-descent step (_kl_divergence_bh + _gradient_descent,
// sklearn/manifold/_t_sne.py), in this order, with no host synchronisation:
//   repulsion_k    the N^2 term: column tiles of y staged in LDS, two rows per
//                  thread in registers, the column range split over S
//                  workgroups per row block -> partials [S][n][3];
//   attract_fold_k the CSR term, one wave per row (the whole workgroup for a
//                  long row), and the fold of the S partials in ascending order;
//   update_k       Z, the gradient, the gains / momentum rule and, on request,
//                  the KL divergence and the gradient norm.
// No atomics anywhere: every sum has one fixed order that depends on the
// sizes alone (n, the row lengths, the split count), so two calls give the
// same bits.  include/cfsd.h states the arithmetic of each entry point.
#include <float.h>
#include <math.h>

#include "cfsd_common.h"

namespace cfsd {

constexpr int kMaxK = CFSD_TSNE_MAX_K;
constexpr int kKnnRows = CFSD_TSNE_KNN_ROWS;  // query rows per workgroup: 4 waves x 4 rows
constexpr int kKnnCols = CFSD_TSNE_KNN_COLS;  // candidate rows per tile: one per lane
constexpr int kKnnDims = CFSD_TSNE_KNN_DIMS;  // coordinates per staged chunk
constexpr int kKnnQ = kKnnRows / 4;           // query rows per wave
constexpr int kKnnPitch = kKnnDims + 1;       // odd pitch: lane l reads bank (l + c) % 64
constexpr unsigned long long kNoKey = ~0ull;
static_assert(kKnnCols == 64 && kKnnRows % 4 == 0 && kMaxK % 64 == 0, "knn_rows_k's lane mapping");

// Insert `key` into the ascending list L[0..k) of one wave (the last entry
// falls out).  Lane l owns the positions l, l + 64, ...: every lane reads its
// entries and their left neighbours, then every lane writes.  The LDS
// executes one wave's instructions in order, so all reads precede all writes.
__device__ __forceinline__ void knn_insert(volatile unsigned long long* L, int k, int lane,
                                           unsigned long long key) {
  unsigned long long own[kMaxK / 64], left[kMaxK / 64];
#pragma unroll
  for (int t = 0; t < kMaxK / 64; ++t) {
    const int p = lane + 64 * t;
    if (p < k) {
      own[t] = L[p];
      left[t] = p ? L[p - 1] : 0ull;
    }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int t = 0; t < kMaxK / 64; ++t) {
    const int p = lane + 64 * t;
    if (p < k && own[t] > key) L[p] = left[t] < key ? key : left[t];
  }
  __builtin_amdgcn_wave_barrier();
}

// Workgroup b owns the query rows [16 b, 16 b + 16), wave w four of them.  The
// candidate rows are walked in ascending tiles of 64 (lane l: row j0 + l), each
// tile's coordinates in ascending chunks of 64 staged in LDS; a query
// coordinate is wave-uniform and read straight from memory.  Per pair, for
// c = 0 .. d - 1 from acc = +0,
//   t = fl(z[i, c] - z[j, c]),  e = (z[i, c] - z[j, c]) - t exactly (TwoSum),
//   acc <- fma(t, t, fma(2 e, t, acc))
// (contraction off: nothing else is fused): two roundings of the sum per
// coordinate and a dropped e^2, so d2 is within d 2^-23 of the exact
// distance for every d -- the plain fl(t)^2 form is not for d = 1 (1.5 2^-23:
// the subtraction's rounding counts twice).  The key of a candidate is
// (bits of d2) << 32 | j -- d2 >= +0, so keys order as (d2, j) -- and a
// candidate enters the row's list when its key is below the list's last one.
__global__ void __launch_bounds__(256) knn_rows_k(const float* __restrict__ z, int32_t* __restrict__ idx,
                                                  float* __restrict__ d2, int n, int d, int k) {
#pragma clang fp contract(off)
  __shared__ float tile[kKnnCols * kKnnPitch];
  __shared__ unsigned long long list[kKnnRows][kMaxK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = (int)blockIdx.x * kKnnRows + wave * kKnnQ;
  const float* zq[kKnnQ];
#pragma unroll
  for (int q = 0; q < kKnnQ; ++q) {
    zq[q] = z + (size_t)min(row0 + q, n - 1) * d;
    for (int p = lane; p < k; p += 64) list[wave * kKnnQ + q][p] = kNoKey;
  }
  for (int j0 = 0; j0 < n; j0 += kKnnCols) {
    float acc[kKnnQ];
#pragma unroll
    for (int q = 0; q < kKnnQ; ++q) acc[q] = 0.f;
    for (int c0 = 0; c0 < d; c0 += kKnnDims) {
      __syncthreads();  // the previous chunk has been consumed
#pragma unroll 4
      for (int e = tid; e < kKnnCols * kKnnDims; e += 256) {
        const int col = e / kKnnDims, cc = e % kKnnDims;
        const int j = j0 + col, c = c0 + cc;
        tile[col * kKnnPitch + cc] = (j < n && c < d) ? z[(size_t)j * d + c] : 0.f;
      }
      __syncthreads();
      const int cend = min(kKnnDims, d - c0);
#pragma unroll 8
      for (int cc = 0; cc < cend; ++cc) {
        const float zj = tile[lane * kKnnPitch + cc];
#pragma unroll
        for (int q = 0; q < kKnnQ; ++q) {
          const float a = zq[q][c0 + cc], nb = -zj;
          const float t = a + nb, bb = t - a;
          const float e = (a - (t - bb)) + (nb - bb);  // TwoSum: a - zj == t + e exactly
          acc[q] = fmaf(t, t, fmaf(e + e, t, acc[q]));
        }
      }
    }
    const int j = j0 + lane;
#pragma unroll
    for (int q = 0; q < kKnnQ; ++q) {
      const int i = row0 + q;
      if (i >= n) break;  // wave-uniform
      volatile unsigned long long* L = list[wave * kKnnQ + q];
      const unsigned long long key =
          (j < n && j != i) ? ((unsigned long long)__float_as_uint(acc[q]) << 32) | (unsigned)j : kNoKey;
      unsigned long long last = L[k - 1];
      unsigned long long todo = __ballot(key < last);
      while (todo) {  // ascending lanes = ascending j
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)key, src);
        const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(key >> 32), src);
        const unsigned long long cand = ((unsigned long long)hi << 32) | lo;
        if (cand < last) {
          knn_insert(L, k, lane, cand);
          last = L[k - 1];
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kKnnQ; ++q) {
    const int i = row0 + q;
    if (i >= n) break;
    for (int p = lane; p < k; p += 64) {  // k <= n - 1: every entry is a real key
      const unsigned long long key = list[wave * kKnnQ + q][p];
      idx[i * k + p] = (int32_t)(unsigned)key;
      d2[i * k + p] = __uint_as_float((unsigned)(key >> 32));
    }
  }
}

// Sum over the wave in a fixed butterfly (xor 32, 16, ..., 1): every lane
// ends with the same bits (a + b == b + a).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
  return v;
}

// _binary_search_perplexity, one wave per row: lane l holds the neighbours l,
// l + 64, ... (at most kMaxK / 64).  Every lane sees the same sums, so the
// search's branches are wave-uniform.
__global__ void __launch_bounds__(256) affinities_k(const float* __restrict__ d2, float* __restrict__ p_cond,
                                                    float* __restrict__ beta_out, int n, int k,
                                                    double desired_entropy) {
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (row >= n) return;
  constexpr int T = kMaxK / 64;
  double dist[T], e[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int j = lane + 64 * t;
    dist[t] = j < k ? (double)d2[row * k + j] : 0.0;
    e[t] = 0.0;
  }
  const double tiny = (double)1e-8f, tol = (double)1e-5f;  // _utils.pyx declares both as C floats
  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, used = 1.0, sum = 1.0;
  for (int step = 0; step < 100; ++step) {
    double s = 0.0, sd = 0.0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      e[t] = lane + 64 * t < k ? exp(-dist[t] * beta) : 0.0;
      s += e[t];
      sd += dist[t] * e[t];
    }
    s = wave_sum(s);
    sd = wave_sum(sd);
    if (s == 0.0) s = tiny;
    sum = s;
    used = beta;
    const double diff = log(s) + beta * (sd / s) - desired_entropy;
    if (fabs(diff) <= tol) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int j = lane + 64 * t;
    if (j < k) p_cond[row * k + j] = (float)(e[t] / sum);
  }
  if (lane == 0) beta_out[row] = (float)used;
}

// ---------------------------------------------------------------- the iteration
constexpr int kRepThreads = 256;
constexpr int kRepRows = CFSD_TSNE_ROWS;  // rows per workgroup: two per thread
constexpr int kRepTile = CFSD_TSNE_TILE;  // columns per LDS stage
constexpr int kMaxSplits = CFSD_TSNE_MAX_SPLITS;
constexpr int kLongRow = CFSD_TSNE_LONG_ROW;
constexpr int kAttThreads = 1024, kAttRows = CFSD_TSNE_ATT_ROWS;
constexpr int kUpdThreads = 1024;
static_assert(kRepRows == 2 * kRepThreads && kRepTile <= kRepThreads && kRepTile % 2 == 0, "repulsion_k's mapping");
static_assert(kAttRows * 64 == kAttThreads && kLongRow % 64 == 0, "attract_fold_k's mapping");

struct Rep {
  float x, y, z;
};

// One (row, column) pair: q = 1 / (1 + |yi - yj|^2) (v_rcp_f32, 1 ulp), the
// force q^2 (yi - yj) and q itself.  CAREFUL: the pair counts only when `ok`.
template <bool CAREFUL>
__device__ __forceinline__ void rep_pair(float2 yi, float cx, float cy, bool ok, Rep& a) {
  const float dx = yi.x - cx, dy = yi.y - cy;
  float q = __builtin_amdgcn_rcpf(1.f + fmaf(dx, dx, dy * dy));
  if (CAREFUL) q = ok ? q : 0.f;
  const float q2 = q * q;
  a.x = fmaf(q2, dx, a.x);
  a.y = fmaf(q2, dy, a.y);
  a.z += q;
}

template <bool CAREFUL>
__device__ __forceinline__ void rep_tile(const float2* ty, float2 y0, float2 y1, int i0, int i1, int jb, int n,
                                         Rep& a0, Rep& a1) {
#pragma unroll 8
  for (int jj = 0; jj < kRepTile; jj += 2) {
    const f32x4 c = *reinterpret_cast<const f32x4*>(&ty[jj]);  // two columns, the same address in every lane
    const int j = jb + jj;
    rep_pair<CAREFUL>(y0, c.x, c.y, j != i0 && j < n, a0);
    rep_pair<CAREFUL>(y1, c.x, c.y, j != i1 && j < n, a1);
    rep_pair<CAREFUL>(y0, c.z, c.w, j + 1 != i0 && j + 1 < n, a0);
    rep_pair<CAREFUL>(y1, c.z, c.w, j + 1 != i1 && j + 1 < n, a1);
  }
}

// grid (row blocks, S).  Thread t of row block b owns the rows 512 b + t and
// 512 b + 256 + t; split s walks the column tiles [s tps, (s + 1) tps) in
// ascending order.  Per row and tile the 128 columns are added in ascending j
// onto +0, the tile's three sums are then added onto the split's: two levels,
// so a row's error does not grow with n / 128 the way one running sum would.
// The next tile's columns are fetched into a register while this one is used.
__global__ void __launch_bounds__(kRepThreads) repulsion_k(const float2* __restrict__ y, float* __restrict__ part,
                                                           int n, int n_tiles, int tiles_per_split) {
  __shared__ __attribute__((aligned(16))) float2 ty[kRepTile];
  const int tid = threadIdx.x;
  const int r0 = (int)blockIdx.x * kRepRows;
  const int i0 = r0 + tid, i1 = i0 + kRepThreads;
  const int t0 = (int)blockIdx.y * tiles_per_split, t1 = min(n_tiles, t0 + tiles_per_split);
  const float2 zero = make_float2(0.f, 0.f);
  const float2 y0 = i0 < n ? y[i0] : zero, y1 = i1 < n ? y[i1] : zero;
  Rep s0 = {0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f};
  float2 next = zero;
  if (tid < kRepTile && t0 < t1) {
    const int j = t0 * kRepTile + tid;
    next = j < n ? y[j] : zero;
  }
  for (int t = t0; t < t1; ++t) {
    __syncthreads();  // the previous tile has been consumed
    if (tid < kRepTile) ty[tid] = next;
    __syncthreads();
    if (tid < kRepTile && t + 1 < t1) {
      const int j = (t + 1) * kRepTile + tid;
      next = j < n ? y[j] : zero;
    }
    const int jb = t * kRepTile;
    Rep a0 = {0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f};
    // a tile that holds one of this block's own rows, or runs past n, checks every pair
    if (jb + kRepTile > n || (jb < r0 + kRepRows && jb + kRepTile > r0))
      rep_tile<true>(ty, y0, y1, i0, i1, jb, n, a0, a1);
    else
      rep_tile<false>(ty, y0, y1, i0, i1, jb, n, a0, a1);
    s0.x += a0.x, s0.y += a0.y, s0.z += a0.z;
    s1.x += a1.x, s1.y += a1.y, s1.z += a1.z;
  }
  float* out = part + (size_t)blockIdx.y * n * 3;
  if (i0 < n) out[i0 * 3 + 0] = s0.x, out[i0 * 3 + 1] = s0.y, out[i0 * 3 + 2] = s0.z;
  if (i1 < n) out[i1 * 3 + 0] = s1.x, out[i1 * 3 + 1] = s1.y, out[i1 * 3 + 2] = s1.z;
}

// The step's scratch: forces [n][4] = (attr_x, attr_y, rep_x, rep_y), then per
// attract_fold_k workgroup three float64 partials (sum zrow, sum p log(p/q),
// sum p), then the repulsion partials [S][n][3].
struct StepWs {
  float* forces;
  double* zpart;
  float* part;
  size_t bytes;
};
__host__ __device__ inline int att_blocks(int n) { return (n + kAttRows - 1) / kAttRows; }
inline StepWs step_ws(void* ws, int n, int splits) {
  StepWs w;
  char* p = (char*)ws;
  w.forces = (float*)p;
  size_t off = (size_t)n * 4 * sizeof(float);
  w.zpart = (double*)(p + off);
  off += (size_t)att_blocks(n) * 3 * sizeof(double);
  w.part = (float*)(p + off);
  off += (size_t)splits * n * 3 * sizeof(float);
  w.bytes = off;
  return w;
}

struct Att {
  float x, y;
  double kl, sp;
};

// Entries first, first + stride, ... of one CSR row, in ascending order.
__device__ __forceinline__ Att att_entries(const float2* __restrict__ y, const int32_t* __restrict__ col,
                                           const float* __restrict__ val, float2 yi, int begin, int end,
                                           int first, int stride, int n, bool want_error) {
  Att a = {0.f, 0.f, 0.0, 0.0};
#pragma unroll 4
  for (int e = begin + first; e < end; e += stride) {
    const int c = min(max(col[e], 0), n - 1);
    const float p = val[e];
    const float2 yj = y[c];
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float pq = p * __builtin_amdgcn_rcpf(1.f + fmaf(dx, dx, dy * dy));
    a.x = fmaf(pq, dx, a.x);
    a.y = fmaf(pq, dy, a.y);
    if (want_error && p > 0.f) {  // -log q = log1p(|yi - yj|^2), in float64: finite for every finite y
      const double dd = (double)dx * (double)dx + (double)dy * (double)dy;
      a.kl += (double)p * (log((double)p) + log1p(dd));
      a.sp += (double)p;
    }
  }
  return a;
}
__device__ __forceinline__ Att att_wave(Att a, bool want_error) {
  a.x = wave_sum(a.x);
  a.y = wave_sum(a.y);
  if (want_error) a.kl = wave_sum(a.kl), a.sp = wave_sum(a.sp);
  return a;
}

// Workgroup b owns the rows [16 b, 16 b + 16), wave w the row 16 b + w.  A row
// of at most CFSD_TSNE_LONG_ROW entries: lane l adds its entries l, l + 64, ...
// in ascending order onto 0, the 64 sums meet in the butterfly.  A longer
// row: thread t of the whole workgroup adds t, t + 1024, ..., each wave folds
// its 64 sums in the butterfly, and the 16 wave sums are added in ascending
// wave order.  Thread r < 16 then folds row 16 b + r's S repulsion partials in
// ascending s, and thread 0 adds the 16 rows' zrow (and, on request, their KL
// terms) in ascending row order in float64.
__global__ void __launch_bounds__(kAttThreads) attract_fold_k(const float2* __restrict__ y,
                                                              const int32_t* __restrict__ row_ptr,
                                                              const int32_t* __restrict__ col,
                                                              const float* __restrict__ val,
                                                              const float* __restrict__ part,
                                                              float* __restrict__ forces, double* __restrict__ zpart,
                                                              int n, int nnz, int splits, float exaggeration,
                                                              int want_error) {
  __shared__ Att rows[kAttRows];
  __shared__ Att waves[kAttRows];
  __shared__ double zrow[kAttRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = (int)blockIdx.x * kAttRows;
  const bool err = want_error != 0;
  {
    const int i = r0 + wave;
    if (i < n) {
      const int begin = min(max(row_ptr[i], 0), nnz), end = min(max(row_ptr[i + 1], begin), nnz);
      if (end - begin <= kLongRow) {
        const Att a = att_wave(att_entries(y, col, val, y[i], begin, end, lane, 64, n, err), err);
        if (lane == 0) rows[wave] = a;
      }
    }
  }
  for (int r = 0; r < kAttRows; ++r) {  // the long rows, by the whole workgroup (block-uniform branch)
    const int i = r0 + r;
    if (i >= n) break;
    const int begin = min(max(row_ptr[i], 0), nnz), end = min(max(row_ptr[i + 1], begin), nnz);
    if (end - begin <= kLongRow) continue;
    const Att a = att_wave(att_entries(y, col, val, y[i], begin, end, tid, kAttThreads, n, err), err);
    if (lane == 0) waves[wave] = a;
    __syncthreads();
    if (tid == 0) {
      Att s = waves[0];
      for (int w = 1; w < kAttRows; ++w) s.x += waves[w].x, s.y += waves[w].y, s.kl += waves[w].kl, s.sp += waves[w].sp;
      rows[r] = s;
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid < kAttRows) {
    const int i = r0 + tid;
    double zr = 0.0;
    if (i < n) {
      float rx = 0.f, ry = 0.f, rz = 0.f;
      for (int s = 0; s < splits; ++s) {
        const float* p = part + ((size_t)s * n + i) * 3;
        rx += p[0], ry += p[1], rz += p[2];
      }
      st4(forces + (size_t)i * 4, (f32x4){exaggeration * rows[tid].x, exaggeration * rows[tid].y, rx, ry});
      zr = (double)rz;
    }
    zrow[tid] = zr;
  }
  __syncthreads();
  if (tid == 0) {
    double z = 0.0, kl = 0.0, sp = 0.0;
    for (int r = 0; r < kAttRows && r0 + r < n; ++r) {
      z += zrow[r];
      if (err) kl += rows[r].kl, sp += rows[r].sp;
    }
    zpart[blockIdx.x * 3 + 0] = z;
    zpart[blockIdx.x * 3 + 1] = kl;
    zpart[blockIdx.x * 3 + 2] = sp;
  }
}

// Sum of one double per thread over the 1024-thread workgroup: a halving tree
// in LDS (sh[t] += sh[t + w], w = 512, ..., 1); every thread gets the total.
__device__ __forceinline__ double block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = kUpdThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}
// Entry `which` of the nb workgroup partials: thread t adds b = t, t + 1024, ...
// in ascending order, then the tree.
__device__ __forceinline__ double partial_sum(const double* __restrict__ zpart, int nb, int which, double* sh) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += kUpdThreads) s += zpart[b * 3 + which];
  return block_sum(s, sh);
}

// Grid-stride over the points with 1024 threads per workgroup; every
// workgroup forms Z itself from the partials, in the same order.  With
// want_error the grid is ONE workgroup, which also reduces the KL terms and
// the squared norm of gains * grad (float64: per thread in ascending point
// order, then the tree) -- the per-point arithmetic is the same code, so y,
// update, gains and grad do not depend on the flag.
__global__ void __launch_bounds__(kUpdThreads) update_k(float2* __restrict__ y, float2* __restrict__ update,
                                                        float2* __restrict__ gains, float2* __restrict__ grad,
                                                        float* __restrict__ result, const float* __restrict__ forces,
                                                        const double* __restrict__ zpart, int n, float exaggeration,
                                                        float momentum, float lr, int want_error) {
#pragma clang fp contract(off)
  __shared__ double sh[kUpdThreads];
  const int nb = att_blocks(n);
  const double z = fmax(partial_sum(zpart, nb, 0, sh), DBL_EPSILON);  // _barnes_hut_tsne.pyx: sQ = max(sQ, eps)
  const float inv_z = (float)(1.0 / z);
  double norm2 = 0.0;
  for (int i = (int)(blockIdx.x * kUpdThreads + threadIdx.x); i < n; i += (int)(gridDim.x * kUpdThreads)) {
    const f32x4 f = ld4(forces + (size_t)i * 4);
    const float g[2] = {4.f * (f.x - f.z * inv_z), 4.f * (f.y - f.w * inv_z)};
    const float2 u0 = update[i], k0 = gains[i], p0 = y[i];
    const float uo[2] = {u0.x, u0.y}, ko[2] = {k0.x, k0.y};
    float un[2], kn[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float k1 = uo[c] * g[c] < 0.f ? ko[c] + 0.2f : ko[c] * 0.8f;
      kn[c] = fmaxf(k1, 0.01f);
      const float gg = kn[c] * g[c];
      un[c] = momentum * uo[c] - lr * gg;
      norm2 += (double)gg * (double)gg;
    }
    grad[i] = make_float2(g[0], g[1]);
    gains[i] = make_float2(kn[0], kn[1]);
    update[i] = make_float2(un[0], un[1]);
    y[i] = make_float2(p0.x + un[0], p0.y + un[1]);
  }
  if (want_error) {  // gridDim.x == 1
    const double kl = partial_sum(zpart, nb, 1, sh), sp = partial_sum(zpart, nb, 2, sh);
    norm2 = block_sum(norm2, sh);
    if (threadIdx.x == 0) {
      const double a = (double)exaggeration;
      result[0] = (float)(a * (kl + sp * (log(a) + log(z))));
      result[1] = (float)sqrt(norm2);
    }
  }
}

static int auto_splits(int n) {
  const int row_blocks = (n + kRepRows - 1) / kRepRows, n_tiles = (n + kRepTile - 1) / kRepTile;
  int s = (2048 + row_blocks - 1) / row_blocks;  // ~8 workgroups of 256 threads per CU
  s = s < n_tiles ? s : n_tiles;
  return s < kMaxSplits ? s : kMaxSplits;
}

}  // namespace cfsd

using namespace cfsd;

static int knn_check(const char* what, int n, int d, int k) {
  if (n < 2) return set_error(CFSD_EINVAL, "%s: n=%d, at least 2 rows", what, n);
  if (k < 1 || k > n - 1 || k > kMaxK)
    return set_error(CFSD_EINVAL, "%s: k=%d outside 1..min(n - 1 = %d, %d)", what, k, n - 1, kMaxK);
  if (d < 1 || d > CFSD_TSNE_MAX_D) return set_error(CFSD_EINVAL, "%s: d=%d outside 1..%d", what, d, CFSD_TSNE_MAX_D);
  if ((long)n * k >= (1L << 31)) return set_error(CFSD_EINVAL, "%s: n x k >= 2^31", what);
  return CFSD_OK;
}

extern "C" size_t cfsd_knn_rows_workspace(int n, int d, int k) {
  (void)n, (void)d, (void)k;
  return 0;  // the k best of a row live in LDS
}

extern "C" int cfsd_knn_rows(const float* z, int32_t* idx, float* d2, void* workspace, size_t workspace_bytes, int n,
                             int d, int k, void* stream) {
  (void)workspace, (void)workspace_bytes;
  if (!z || !idx || !d2) return set_error(CFSD_EINVAL, "knn_rows: null pointer");
  if (int rc = knn_check("knn_rows", n, d, k)) return rc;
  hipLaunchKernelGGL(knn_rows_k, dim3((unsigned)((n + kKnnRows - 1) / kKnnRows)), dim3(256), 0, (hipStream_t)stream, z,
                     idx, d2, n, d, k);
  return launch_status("knn_rows");
}

extern "C" int cfsd_tsne_affinities(const float* d2, float* p_cond, float* beta, int n, int k, float perplexity,
                                    void* stream) {
  if (!d2 || !p_cond || !beta) return set_error(CFSD_EINVAL, "tsne_affinities: null pointer");
  if (int rc = knn_check("tsne_affinities", n, 1, k)) return rc;
  if (!(perplexity > 0.f) || !(perplexity < INFINITY))
    return set_error(CFSD_EINVAL, "tsne_affinities: perplexity %g is not a positive number", (double)perplexity);
  hipLaunchKernelGGL(affinities_k, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d2, p_cond, beta,
                     n, k, log((double)perplexity));
  return launch_status("tsne_affinities");
}

static int step_check(const char* what, int n, int nnz, int& splits) {
  if (n < 2 || n > CFSD_TSNE_MAX_N) return set_error(CFSD_EINVAL, "%s: n=%d outside 2..%d", what, n, CFSD_TSNE_MAX_N);
  if (nnz < 0) return set_error(CFSD_EINVAL, "%s: nnz=%d", what, nnz);
  if (splits < 0 || splits > kMaxSplits)
    return set_error(CFSD_EINVAL, "%s: splits=%d outside 0..%d", what, splits, kMaxSplits);
  if (splits == 0) splits = auto_splits(n);
  return CFSD_OK;
}

extern "C" int cfsd_tsne_splits(int n) { return n < 2 ? 1 : auto_splits(n); }

extern "C" size_t cfsd_tsne_step_workspace(int n, int splits) {
  if (n < 2 || n > CFSD_TSNE_MAX_N || splits < 0 || splits > kMaxSplits) return 0;
  return step_ws(nullptr, n, splits ? splits : auto_splits(n)).bytes;
}

extern "C" int cfsd_tsne_forces(const float* y, const int32_t* row_ptr, const int32_t* col, const float* val,
                                void* workspace, size_t workspace_bytes, int n, int nnz, int splits,
                                float exaggeration, int want_error, void* stream) {
  if (!y || !row_ptr || !workspace || (nnz > 0 && (!col || !val)))
    return set_error(CFSD_EINVAL, "tsne_forces: null pointer");
  if (int rc = step_check("tsne_forces", n, nnz, splits)) return rc;
  if (!(exaggeration > 0.f)) return set_error(CFSD_EINVAL, "tsne_forces: exaggeration %g <= 0", (double)exaggeration);
  const StepWs w = step_ws(workspace, n, splits);
  if (workspace_bytes < w.bytes)
    return set_error(CFSD_EWORKSPACE, "tsne_forces: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  const int n_tiles = (n + kRepTile - 1) / kRepTile;
  hipLaunchKernelGGL(repulsion_k, dim3((unsigned)((n + kRepRows - 1) / kRepRows), (unsigned)splits), dim3(kRepThreads),
                     0, (hipStream_t)stream, (const float2*)y, w.part, n, n_tiles, (n_tiles + splits - 1) / splits);
  if (int rc = launch_status("tsne_forces (repulsion)")) return rc;
  hipLaunchKernelGGL(attract_fold_k, dim3((unsigned)att_blocks(n)), dim3(kAttThreads), 0, (hipStream_t)stream,
                     (const float2*)y, row_ptr, col, val, w.part, w.forces, w.zpart, n, nnz, splits, exaggeration,
                     want_error);
  return launch_status("tsne_forces (attraction)");
}

extern "C" int cfsd_tsne_update(float* y, float* update, float* gains, float* grad, float* result,
                                const void* workspace, size_t workspace_bytes, int n, int splits, float exaggeration,
                                float momentum, float learning_rate, int want_error, void* stream) {
  if (!y || !update || !gains || !grad || !workspace || (want_error && !result))
    return set_error(CFSD_EINVAL, "tsne_update: null pointer");
  if (int rc = step_check("tsne_update", n, 0, splits)) return rc;
  if (!(exaggeration > 0.f)) return set_error(CFSD_EINVAL, "tsne_update: exaggeration %g <= 0", (double)exaggeration);
  const StepWs w = step_ws(const_cast<void*>(workspace), n, splits);
  if (workspace_bytes < w.bytes)
    return set_error(CFSD_EWORKSPACE, "tsne_update: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  const unsigned grid = want_error ? 1u : (unsigned)((n + kUpdThreads - 1) / kUpdThreads);
  hipLaunchKernelGGL(update_k, dim3(grid), dim3(kUpdThreads), 0, (hipStream_t)stream, (float2*)y, (float2*)update,
                     (float2*)gains, (float2*)grad, result, w.forces, w.zpart, n, exaggeration, momentum,
                     learning_rate, want_error);
  return launch_status("tsne_update");
}
