// General-shape SpiralConv (fp32, batch-major): forward, data gradient and
// weight gradient for ANY spiral length and channel pair inside the limits of
// cfsd.h (CFSD_GEN_MAX_SEQ, CFSD_GEN_MAX_CH).  The specialised kernels of
// spiral_conv.hip are template instances of a short shape list; these take
// the shape as run-time arguments, so a configuration with another spiral
// length or channel width trains at all.  They are not tuned to the
// specialised kernels' level (DESIGN "General-shape SpiralConv").
//
// Every contraction runs on v_mfma_f32_32x32x2_f32, one 32 x 32 output tile
// (or two side by side) per wave, operands straight from global memory:
//
//   forward   y[m, o]   = sum_k G[m, k] w[o, k]      A = gathered x, B = w^T
//   dx        dx[m', c] = sum_{s, o} T[m', s, o] w[o, s cin + c]
//                                                   A = T = the dpre rows of
//                                                   list (u, s) added up, B = w
//   dW | db   dw[o, k]  = sum_m dpre[m, o] [G | 1][m, k]
//                                                   A = dpre^T, B = [G | 1]
//
// Padding.  The k index of an MFMA step only has to be the SAME for both
// operands, so each step takes whichever k suit the loads: the lane half h
// (lane >> 5) covers 4 consecutive channels (16-B loads, channel counts that
// are multiples of 4) or 1 channel.  A k past the end of its spiral slot (cin
// or cout not a multiple of the step), a row past the last row and a column
// past the last column feed 0.0f from a CLAMPED address: nothing is read
// outside x, idx, w or dpre, and fma(0, 0, c) == c leaves the sums exact.
// Stores are masked.  All sums have a fixed order; there are no atomics.
#include <type_traits>

#include "cfsd_common.h"
#include "conv_dispatch.h"

namespace cfsd {
namespace gen {

constexpr int kWaves = 4;  // waves per workgroup (one tile each; conv_dx<SPLIT>: one tile for all four)

__device__ __forceinline__ f32x4 zero4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// ---------------------------------------------------------------- forward
// Wave = 32 output rows m = b*rows + r  x  NT column tiles of 32 outputs.
// VEC: cin % 4 == 0 and 16-B aligned x / w (one 16-B load feeds 4 k-steps).
template <bool VEC, int NT>
__global__ __launch_bounds__(64 * kWaves) void conv_fwd(const float* __restrict__ x, const int* __restrict__ idx,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int vsrc, int rows, int seq, int cin,
                                                        int cout, long M, int act) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const long tile = (long)blockIdx.x * kWaves + wave;
  if (tile * 32 >= M) return;  // wave-uniform
  const int K = seq * cin;
  const long m = tile * 32 + i;
  const int mc = (int)(m < M ? m : M - 1);  // clamped: rows past M are computed and not stored
  const int b = mc / rows, r = mc - b * rows;
  const float* xb = x + (long)b * vsrc * cin;
  const int* ir = idx + (long)r * seq;
  const float* wr[NT];
  bool cv[NT];
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = (blockIdx.y * NT + t) * 32 + i;
    cv[t] = col < cout;
    wr[t] = w + (long)(cv[t] ? col : 0) * K;
    acc[t] = zero16();
  }
  for (int s = 0; s < seq; ++s) {
    const float* xr = xb + (long)ir[s] * cin;
    const int ko = s * cin;
    if constexpr (VEC) {
      for (int c0 = 0; c0 < cin; c0 += 8) {
        const int c = c0 + 4 * h;
        const bool in = c < cin;
        const int cc = in ? c : 0;
        const f32x4 a = in ? ld4(xr + cc) : zero4();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 bw = (in && cv[t]) ? ld4(wr[t] + ko + cc) : zero4();
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[t] = mfma32(a[j], bw[j], acc[t]);
        }
      }
    } else {
      for (int c0 = 0; c0 < cin; c0 += 2) {
        const int c = c0 + h;
        const bool in = c < cin;
        const int cc = in ? c : 0;
        const float a = in ? xr[cc] : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float bw = (in && cv[t]) ? wr[t][ko + cc] : 0.f;
          acc[t] = mfma32(a, bw, acc[t]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = (blockIdx.y * NT + t) * 32 + i;
    if (col >= cout) continue;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const long row = tile * 32 + acc_row(q, lane);
      if (row >= M) continue;
      const float v = acc[t][q] + bv;
      y[row * cout + col] = act == CFSD_ACT_ELU ? elu_f(v) : v;
    }
  }
}

// ---------------------------------------------------------------- data gradient
// Wave = 32 source rows m = b*vsrc + u  x  NT column tiles of 32 input
// channels; the contraction index is (slot s, output channel o):
//   dx[m, c] = sum_{s, o} T[m, s, o] w[o, s cin + c],
//   T[m, s, o] = sum_{e in list(u, s)} dpre[b, r_e, o]   (e ascending)
// so the MFMA count does not depend on the list lengths: the lane's row adds
// the dpre rows of its list on the VALU (an empty list: T = 0, and
// fma(0, w, acc) == acc, so a vertex in no spiral keeps an exact 0) and the
// slot's weights are the B operand of every row.  The first kHead entries of
// a list are loaded one slot ahead and their dpre rows fetched together;
// longer lists finish in a per-lane loop.  VEC: cout % 4 == 0 and 16-B
// aligned dpre.
constexpr int kHead = 4;
struct DxList {
  int p0, len, r[kHead];
};
__device__ __forceinline__ DxList dx_list(const int* __restrict__ pk, const int* __restrict__ inv_row, int s,
                                          bool mv) {
  DxList L;
  L.p0 = pk[s];
  L.len = mv ? pk[s + 1] - L.p0 : 0;
#pragma unroll
  for (int j = 0; j < kHead; ++j) L.r[j] = j < L.len ? inv_row[L.p0 + j] : 0;
  return L;
}

// SPLIT (few-row layers: fewer row tiles than fill the chip): the four waves of
// a workgroup share ONE tile and take every fourth slot each, so a wave's
// dependent chain of gathers is a quarter as long; their accumulators are
// added through LDS in wave order (fixed, like every other sum here).
template <bool VEC, int NT, bool SPLIT>
__global__ __launch_bounds__(64 * kWaves) void conv_dx(const float* __restrict__ dpre,
                                                       const int* __restrict__ inv_ptr,
                                                       const int* __restrict__ inv_row, const float* __restrict__ w,
                                                       const float* __restrict__ elu_y, float* __restrict__ dx,
                                                       int vsrc, int rows, int seq, int cin, int cout, long M) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const long tile = SPLIT ? (long)blockIdx.x : (long)blockIdx.x * kWaves + wave;
  if (!SPLIT && tile * 32 >= M) return;  // wave-uniform (SPLIT: the grid is the tile count, and a barrier follows)
  const int K = seq * cin;
  const long m = tile * 32 + i;
  const bool mv = m < M;
  const int mc = (int)(mv ? m : M - 1);
  const int b = mc / vsrc, u = mc - b * vsrc;
  const float* dpb = dpre + (long)b * rows * cout;
  const int* pk = inv_ptr + (long)u * seq;
  int ccol[NT];
  bool cv[NT];
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = (blockIdx.y * NT + t) * 32 + i;
    cv[t] = col < cin;
    ccol[t] = cv[t] ? col : 0;
    acc[t] = zero16();
  }
  constexpr int STEP = VEC ? 8 : 2, W = VEC ? 4 : 1;  // channels per MFMA run, per lane half
  constexpr int S0 = SPLIT ? kWaves : 1;  // slot stride of this wave
  const int s_first = SPLIT ? wave : 0;
  DxList nxt = dx_list(pk, inv_row, s_first < seq ? s_first : 0, mv);
  for (int s = s_first; s < seq; s += S0) {
    const DxList cur = nxt;
    nxt = dx_list(pk, inv_row, s + S0 < seq ? s + S0 : s, mv);  // (past the end: this slot again, in bounds, unused)
    const float* ws = w + s * cin;
    // T of one run of channels: the head's rows in flight together, then the rest of the list
    auto list_sum = [&](int o0, float (&a)[W], bool& in, int& oc) {
      const int o = o0 + W * h;
      in = o < cout;
      oc = in ? o : 0;
#pragma unroll
      for (int j = 0; j < W; ++j) a[j] = 0.f;
      if (!in) return;
#pragma unroll
      for (int e = 0; e < kHead; ++e) {
        if (e < cur.len) {
          const float* dr = dpb + (long)cur.r[e] * cout + oc;
          if constexpr (VEC) {
            const f32x4 d = ld4(dr);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += d[j];
          } else {
            a[0] += dr[0];
          }
        }
      }
      for (int e = kHead; e < cur.len; ++e) {  // per lane: lists longer than the head
        const float* dr = dpb + (long)inv_row[cur.p0 + e] * cout + oc;
        if constexpr (VEC) {
          const f32x4 d = ld4(dr);
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] += d[j];
        } else {
          a[0] += dr[0];
        }
      }
    };
    auto contract = [&](const float (&a)[W], bool in, int oc) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const float bw = (in && cv[t]) ? ws[(long)(oc + j) * K + ccol[t]] : 0.f;
          acc[t] = mfma32(a[j], bw, acc[t]);
        }
      }
    };
    // two runs per trip: both runs' gathers are issued before the first MFMA waits for them
    for (int o0 = 0; o0 < cout; o0 += 2 * STEP) {
      float a0[W], a1[W];
      bool in0, in1 = false;
      int oc0, oc1 = 0;
      const bool two = o0 + STEP < cout;  // wave-uniform
      list_sum(o0, a0, in0, oc0);
      if (two) list_sum(o0 + STEP, a1, in1, oc1);
      contract(a0, in0, oc0);
      if (two) contract(a1, in1, oc1);
    }
  }
  if constexpr (SPLIT) {
    __shared__ float red[kWaves - 1][NT][16][64];
    if (wave > 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) red[wave - 1][t][q][lane] = acc[t][q];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int v = 0; v < kWaves - 1; ++v)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] += red[v][t][q][lane];
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = (blockIdx.y * NT + t) * 32 + i;
    if (col >= cin) continue;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const long row = tile * 32 + acc_row(q, lane);
      if (row >= M) continue;
      const float g = elu_y ? elu_grad_from_out(elu_y[row * cin + col]) : 1.f;
      dx[row * cin + col] = g * acc[t][q];
    }
  }
}

// ---------------------------------------------------------------- weight gradient
// Stage 1.  The output [cout] x [K + 1] (column K: the bias gradient, whose B
// operand is 1) is cut into 32 x 32 tiles and the M = batch*rows rows into
// n_slabs chunks of `chunk` rows; a wave owns one (chunk, tile) and sums its
// rows two per MFMA step, in ascending row order.  Slab p holds the chunk's
// partial [cout*K | cout] like dw | db.  Stage 2 (slab_sum) adds the slabs of
// one element in a fixed order.
__global__ __launch_bounds__(64 * kWaves) void conv_dw(const float* __restrict__ x, const int* __restrict__ idx,
                                                       const float* __restrict__ dpre, float* __restrict__ slabs,
                                                       int vsrc, int rows, int seq, int cin, int cout, long M,
                                                       int chunk, int n_ot, int n_tiles, long n_tasks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const long task = (long)blockIdx.x * kWaves + wave;
  if (task >= n_tasks) return;  // wave-uniform
  const int K = seq * cin;
  const int slab = (int)(task / n_tiles), tile = (int)(task - (long)slab * n_tiles);
  const int kt = tile / n_ot, ot = tile - kt * n_ot;
  // A: this lane's output channel; B: this lane's column of [G | 1]
  const int o = ot * 32 + i;
  const bool ov = o < cout;
  const int oc = ov ? o : 0;
  const int kc = kt * 32 + i;
  const bool gv = kc < K, one = kc == K;
  const int ks = gv ? kc / cin : 0, kch = gv ? kc - ks * cin : 0;
  const long m0 = (long)slab * chunk, m1 = m0 + chunk < M ? m0 + chunk : M;
  int bb = (int)((m0 + h) / rows), r = (int)((m0 + h) - (long)bb * rows);
  f32x16 acc = zero16();
  constexpr int U = 4;  // steps whose loads are issued together
  for (long base = m0; base < m1; base += 2 * U) {  // wave-uniform trip count
    float a[U], bw[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const long mm = base + 2 * q + h;
      const bool v = mm < m1;
      const int rc = v ? r : 0, bc = v ? bb : 0;
      a[q] = (v && ov) ? dpre[(v ? mm : 0) * cout + oc] : 0.f;
      bw[q] = (v && one) ? 1.f : 0.f;
      if (v && gv) bw[q] = x[((long)bc * vsrc + idx[(long)rc * seq + ks]) * cin + kch];
      r += 2;  // r < rows before: at most two wraps (rows == 1)
      if (r >= rows) r -= rows, ++bb;
      if (r >= rows) r -= rows, ++bb;
    }
#pragma unroll
    for (int q = 0; q < U; ++q) acc = mfma32(a[q], bw[q], acc);
  }
  float* out = slabs + (long)slab * ((long)cout * K + cout);
  if (kc <= K) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int oo = ot * 32 + acc_row(q, lane);
      if (oo >= cout) continue;
      if (kc < K) out[(long)oo * K + kc] = acc[q];
      else out[(long)cout * K + oo] = acc[q];
    }
  }
}

// Stage 2: element e of [dw | db] = the sum of its n_slabs partials, 16 waves
// taking every 16th slab each, their sums added in wave order.
__global__ __launch_bounds__(1024) void slab_sum(const float* __restrict__ slabs, int n_slabs, long n_el,
                                                 float* __restrict__ dw, long n_dw, float* __restrict__ db) {
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long e = (long)blockIdx.x * 64 + lane;
  const bool valid = e < n_el;
  if (!valid) e = n_el - 1;
  float sum = 0.f;
#pragma unroll 4
  for (int p = wv; p < n_slabs; p += 16) sum += slabs[(long)p * n_el + e];
  part[wv][lane] = sum;
  __syncthreads();
  if (wv == 0 && valid) {
    float t = part[0][lane];
#pragma unroll
    for (int q = 1; q < 16; ++q) t += part[q][lane];
    if (e < n_dw) dw[e] = t;
    else db[e - n_dw] = t;
  }
}

// Launch geometry of the weight gradient, shared by the workspace query, the
// launch and the reduce: constants only, so all three always agree.
struct DwGeom {
  int n_ot, n_tiles, chunk, n_slabs;
  long n_el;
};
static DwGeom dw_geom(int batch, int rows, int seq, int cin, int cout) {
  DwGeom g;
  const long M = (long)batch * rows, K = (long)seq * cin;
  g.n_ot = (cout + 31) / 32;
  g.n_tiles = g.n_ot * (int)((K + 1 + 31) / 32);
  g.n_el = (long)cout * K + cout;
  // ~4k waves over the chip, chunks of at least 64 rows, at most 256 slabs
  long want = (4096 + g.n_tiles - 1) / g.n_tiles;
  want = want > 256 ? 256 : want;
  const long most = (M + 63) / 64;
  want = want > most ? most : want;
  long chunk = ((M + want - 1) / want + 1) / 2 * 2;  // even: a step takes two rows
  g.chunk = (int)chunk;
  g.n_slabs = (int)((M + chunk - 1) / chunk);
  return g;
}

}  // namespace gen
}  // namespace cfsd

using namespace cfsd;

// ============================================================== C ABI
static int gen_check(const char* who, const void* a, const void* b, const void* c, const void* d, int batch, int vsrc,
                     int rows, int seq, int cin, int cout) {
  if (!a || !b || !c || !d) return set_error(CFSD_EINVAL, "%s: null pointer", who);
  if (batch <= 0 || vsrc <= 0 || rows <= 0 || seq <= 0 || cin <= 0 || cout <= 0)
    return set_error(CFSD_EINVAL, "%s: non-positive size (batch=%d vsrc=%d rows=%d seq=%d cin=%d cout=%d)", who,
                     batch, vsrc, rows, seq, cin, cout);
  if (seq > CFSD_GEN_MAX_SEQ || cin > CFSD_GEN_MAX_CH || cout > CFSD_GEN_MAX_CH)
    return set_error(CFSD_EINVAL, "%s: seq %d / channels %d -> %d above the limits (seq <= %d, channels <= %d)", who,
                     seq, cin, cout, CFSD_GEN_MAX_SEQ, CFSD_GEN_MAX_CH);
  if (batch > kMaxBatch) return set_error(CFSD_EINVAL, "%s: batch %d too large", who, batch);
  const long v = vsrc > rows ? vsrc : rows, c_max = cin > cout ? cin : cout;
  if ((long)batch * v >= (1L << 31)) return set_error(CFSD_EINVAL, "%s: batch x vertices >= 2^31 (32-bit row indices)", who);
  if ((long)batch * v * c_max >= (1L << 31) || (long)rows * seq >= (1L << 31) || (long)vsrc * seq >= (1L << 31))
    return set_error(CFSD_EINVAL, "%s: a tensor has >= 2^31 elements (32-bit offsets)", who);
  return CFSD_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

constexpr long kTwoTilesFrom = 2048;  // row tiles from which a wave takes two column tiles
template <typename F>
static int gen_for_variant(bool vec, int n_col, long row_tiles, F&& f) {
  // Two column tiles per wave (one gather feeds both) once there is more than one AND the row
  // tiles alone fill the chip (1024 SIMDs); below that a wave per column tile halves each wave's
  // dependent chain, which is what a few-row layer's time is made of.
  const bool two = n_col > 32 && row_tiles >= kTwoTilesFrom;
  if (vec) return two ? f(std::true_type{}, Int<2>{}) : f(std::true_type{}, Int<1>{});
  return two ? f(std::false_type{}, Int<2>{}) : f(std::false_type{}, Int<1>{});
}

extern "C" int cfsd_spiral_conv_gen_fwd(const float* x, const int32_t* idx, const float* w, const float* bias,
                                        float* y, int batch, int vsrc, int rows, int seq, int cin, int cout, int act,
                                        void* stream) {
  int rc = gen_check("spiral_conv_gen_fwd", x, idx, w, y, batch, vsrc, rows, seq, cin, cout);
  if (rc) return rc;
  if (act != CFSD_ACT_NONE && act != CFSD_ACT_ELU) return set_error(CFSD_EINVAL, "spiral_conv_gen_fwd: bad act %d", act);
  const long M = (long)batch * rows;
  const bool vec = cin % 4 == 0 && aligned16(x) && aligned16(w);
  const unsigned gx = (unsigned)(((M + 31) / 32 + gen::kWaves - 1) / gen::kWaves);
  return gen_for_variant(vec, cout, (M + 31) / 32, [&](auto v, auto nt) {
    constexpr int NT = decltype(nt)::value;
    const dim3 grid(gx, (unsigned)((cout + 32 * NT - 1) / (32 * NT)));
    hipLaunchKernelGGL((gen::conv_fwd<decltype(v)::value, NT>), grid, dim3(64 * gen::kWaves), 0, (hipStream_t)stream,
                       x, idx, w, bias, y, vsrc, rows, seq, cin, cout, M, act);
    return launch_status("spiral_conv_gen_fwd");
  });
}

extern "C" int cfsd_spiral_conv_gen_bwd_data(const float* dpre, const int32_t* inv_ptr, const int32_t* inv_row,
                                             const float* w, const float* elu_y, float* dx, int batch, int vsrc,
                                             int rows, int seq, int cin, int cout, void* stream) {
  int rc = gen_check("spiral_conv_gen_bwd_data", dpre, inv_ptr, inv_row, w, batch, vsrc, rows, seq, cin, cout);
  if (rc) return rc;
  if (!dx) return set_error(CFSD_EINVAL, "spiral_conv_gen_bwd_data: null dx");
  const long M = (long)batch * vsrc;
  const bool vec = cout % 4 == 0 && aligned16(dpre);
  const long row_tiles = (M + 31) / 32;
  return gen_for_variant(vec, cin, row_tiles, [&](auto v, auto nt) {
    constexpr int NT = decltype(nt)::value;
    constexpr bool V = decltype(v)::value;
    const unsigned gy = (unsigned)((cin + 32 * NT - 1) / (32 * NT));
    if constexpr (NT == 1) {
      if (row_tiles < kTwoTilesFrom) {  // few rows: one tile per workgroup, the slots split over its waves
        hipLaunchKernelGGL((gen::conv_dx<V, 1, true>), dim3((unsigned)row_tiles, gy), dim3(64 * gen::kWaves), 0,
                           (hipStream_t)stream, dpre, inv_ptr, inv_row, w, elu_y, dx, vsrc, rows, seq, cin, cout, M);
        return launch_status("spiral_conv_gen_bwd_data");
      }
    }
    const dim3 grid((unsigned)((row_tiles + gen::kWaves - 1) / gen::kWaves), gy);
    hipLaunchKernelGGL((gen::conv_dx<V, NT, false>), grid, dim3(64 * gen::kWaves), 0, (hipStream_t)stream, dpre,
                       inv_ptr, inv_row, w, elu_y, dx, vsrc, rows, seq, cin, cout, M);
    return launch_status("spiral_conv_gen_bwd_data");
  });
}

static bool gen_sizes_ok(int batch, int rows, int seq, int cin, int cout) {
  return batch > 0 && batch <= kMaxBatch && rows > 0 && seq > 0 && cin > 0 && cout > 0 && seq <= CFSD_GEN_MAX_SEQ &&
         cin <= CFSD_GEN_MAX_CH && cout <= CFSD_GEN_MAX_CH && (long)batch * rows < (1L << 31);
}

extern "C" size_t cfsd_spiral_conv_gen_bwd_weight_workspace(int batch, int rows, int seq, int cin, int cout) {
  if (!gen_sizes_ok(batch, rows, seq, cin, cout)) return 0;
  const gen::DwGeom g = gen::dw_geom(batch, rows, seq, cin, cout);
  return (size_t)g.n_slabs * (size_t)g.n_el * sizeof(float);
}

static int gen_dw_reduce(const gen::DwGeom& g, const float* workspace, float* dw, float* db, int seq, int cin,
                         int cout, hipStream_t st) {
  hipLaunchKernelGGL(gen::slab_sum, dim3((unsigned)((g.n_el + 63) / 64)), dim3(1024), 0, st, workspace, g.n_slabs,
                     g.n_el, dw, (long)cout * seq * cin, db);
  return launch_status("spiral_conv_gen_dw_reduce");
}

static int gen_check_ws(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
  if (!workspace) return set_error(CFSD_EINVAL, "%s: null workspace", who);
  if (workspace_bytes < need) return set_error(CFSD_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
  return CFSD_OK;
}

extern "C" int cfsd_spiral_conv_gen_bwd_weight(const float* x, const int32_t* idx, const float* dpre, float* dw,
                                               float* db, float* workspace, size_t workspace_bytes, int batch,
                                               int vsrc, int rows, int seq, int cin, int cout, void* stream) {
  const char* who = "spiral_conv_gen_bwd_weight";
  int rc = gen_check(who, x, idx, dpre, dpre, batch, vsrc, rows, seq, cin, cout);
  if (rc) return rc;
  if ((dw == nullptr) != (db == nullptr))
    return set_error(CFSD_EINVAL, "%s: dw and db must both be set (or both NULL: deferred)", who);
  if ((rc = gen_check_ws(who, workspace, workspace_bytes,
                         cfsd_spiral_conv_gen_bwd_weight_workspace(batch, rows, seq, cin, cout))))
    return rc;
  const gen::DwGeom g = gen::dw_geom(batch, rows, seq, cin, cout);
  const long n_tasks = (long)g.n_slabs * g.n_tiles;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gen::conv_dw, dim3((unsigned)((n_tasks + gen::kWaves - 1) / gen::kWaves)), dim3(64 * gen::kWaves),
                     0, st, x, idx, dpre, workspace, vsrc, rows, seq, cin, cout, (long)batch * rows, g.chunk, g.n_ot,
                     g.n_tiles, n_tasks);
  if ((rc = launch_status(who))) return rc;
  if (!dw) return CFSD_OK;  // deferred: cfsd_spiral_conv_gen_dw_reduce sums the slabs later
  return gen_dw_reduce(g, workspace, dw, db, seq, cin, cout, st);
}

extern "C" int cfsd_spiral_conv_gen_dw_reduce(const float* workspace, size_t workspace_bytes, float* dw, float* db,
                                              int batch, int rows, int seq, int cin, int cout, void* stream) {
  const char* who = "spiral_conv_gen_dw_reduce";
  if (!dw || !db) return set_error(CFSD_EINVAL, "%s: null dw / db", who);
  if (!gen_sizes_ok(batch, rows, seq, cin, cout)) return set_error(CFSD_EINVAL, "%s: sizes non-positive or above the limits", who);
  const int rc = gen_check_ws(who, workspace, workspace_bytes,
                              cfsd_spiral_conv_gen_bwd_weight_workspace(batch, rows, seq, cin, cout));
  if (rc) return rc;
  return gen_dw_reduce(gen::dw_geom(batch, rows, seq, cin, cout), workspace, dw, db, seq, cin, cout,
                       (hipStream_t)stream);
}
