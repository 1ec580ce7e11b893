// Chamfer distance of the latent fitting loop (gfx950): batched brute-force
// nearest neighbour and the gradient with respect to the generated points.
//
// Reference: Tester.fit_mesh (test.py:404-405, 427-429) scores the decoded
// heads against an unregistered scan with pytorch3d.loss.chamfer_distance,
// which has no ROCm build.  Semantics restated here: per query the squared
// distance to, and the index of, its nearest reference point; the loss sums
// both directions; only the generated side receives a gradient.
//
// Layout of the search.  A lane owns kNnQpt queries in registers.  The
// reference points are walked in chunks of kNnTile; every address of a chunk
// is wave-uniform (block index and loop counter only), so the coordinates
// arrive through the scalar data cache and are SGPR operands of the VALU ops:
// no LDS, no barrier, nothing to pad -- a partial last chunk is a plain
// per-point loop over the points that exist, so no padding value can win.
// The distance is the difference form (q - r)^2 summed over x, y, z; the
// lane's two queries share packed fp32 instructions (3 sub, 1 mul, 2 fma per
// two pairs).  The arg-min is kept per CHUNK (min3 over its 16 distances,
// one compare + two selects per chunk) and resolved to a point by re-scanning
// the winning chunk at the end: about 3.7 VALU per pair.  Ascending order
// with a strict '<' keeps the lowest index among bit-equal distances.  To
// fill the machine when there are few queries the reference range is cut
// into segments (one workgroup each); the per-segment winners are merged in
// ascending segment order by a second launch.  Every pair's
// distance is the same instruction sequence whatever the cut, so results do
// not depend on the grid.
#include <math.h>

#include "cfsd_common.h"
#include "nn_dist.h"

namespace cfsd {

constexpr int kNnTile = CFSD_NN_TILE;  // reference points per chunk (48 SGPRs)
constexpr int kNnQpt = 2;              // queries per lane
constexpr int kNnBlock = 256;
constexpr int kNnQpb = kNnBlock * kNnQpt;  // queries per workgroup
constexpr int kNnMinSeg = 128;             // least reference points worth a segment
constexpr long kNnTargetBlocks = 8192;     // 32 workgroups per CU: short blocks, small tail

struct NnSplit {
  int nseg, seg_len;
};

// The cut of [0, p) into segments: a function of the shapes alone.
static NnSplit nn_split(int batch, int n, int p) {
  const long qblocks = (long)batch * ((n + kNnQpb - 1) / kNnQpb);
  long want = (kNnTargetBlocks + qblocks - 1) / qblocks;
  const long most = p / kNnMinSeg > 1 ? p / kNnMinSeg : 1;
  if (want > most) want = most;
  if (want > 64) want = 64;
  if (want < 1) want = 1;
  int len = (int)((p + want - 1) / want);
  len = (len + kNnTile - 1) / kNnTile * kNnTile;
  NnSplit s;
  s.seg_len = len;
  s.nseg = (p + len - 1) / len;  // every segment holds at least one point
  return s;
}

// Squared distances of the lane's two queries to one reference point: nn_dist
// (nn_dist.h, shared with the grid search).  One fixed rounding sequence
// (mul, fma, fma) wherever a pair is evaluated -- full chunk, tail loop or the
// closing re-scan -- so the same pair always gives the same bits.  The two
// queries ride in the halves of packed fp32 operands.

// Block (b, s, qb): queries [qb * kNnQpb, +kNnQpb) of batch b against the
// reference points [s * seg_len, min(p, (s + 1) * seg_len)) of batch b (or of
// the single shared batch: q_bs / r_bs = 0 broadcasts).  Writes the segment's
// winner of query (b, i) to dist2 / idx[(s * batch + b) * n + i].
//
// The main loop keeps, per query, the smallest distance and the CHUNK it was
// first reached in (min3 over the chunk's 16 distances, one compare + two
// selects per chunk instead of per pair); the index inside that chunk is
// found afterwards by re-evaluating its <= 16 pairs: the first one whose
// distance is bit-equal to the minimum.  First chunk by strict '<', first
// point inside it: the lowest index among equal distances.
__global__ __launch_bounds__(kNnBlock) void nn_points_k(const float* __restrict__ q, const float* __restrict__ r,
                                                        float* __restrict__ dist2, int* __restrict__ idx, int batch,
                                                        int n, int p, long q_bs, long r_bs, int qblocks, int nseg,
                                                        int seg_len) {
  static_assert(kNnQpt == 2, "a lane's two queries share packed operands");
  const int blk = (int)blockIdx.x;
  const int qb = blk % qblocks, bs = blk / qblocks;
  const int s = bs % nseg, b = bs / nseg;
  const float* qp = q + (long)b * q_bs;
  const float* rp = r + (long)b * r_bs;
  const int j0 = s * seg_len, j1 = min(p, j0 + seg_len);
  const int i0 = min(qb * kNnQpb + (int)threadIdx.x, n - 1);  // clamped lanes: loads only
  const int i1 = min(qb * kNnQpb + kNnBlock + (int)threadIdx.x, n - 1);
  const f32x2 qx = {qp[(long)i0 * 3 + 0], qp[(long)i1 * 3 + 0]};
  const f32x2 qy = {qp[(long)i0 * 3 + 1], qp[(long)i1 * 3 + 1]};
  const f32x2 qz = {qp[(long)i0 * 3 + 2], qp[(long)i1 * 3 + 2]};
  float best[kNnQpt] = {INFINITY, INFINITY};
  int bj[kNnQpt] = {j0, j0};  // start of the winning chunk; in range even if nothing compares below +inf (NaN)
  int j = j0;
  for (; j + kNnTile <= j1; j += kNnTile) {
    const float* c = rp + (long)j * 3;
    float rr[3 * kNnTile];
#pragma unroll
    for (int k = 0; k < 3 * kNnTile; ++k) rr[k] = c[k];
    f32x2 d[kNnTile];
#pragma unroll
    for (int t = 0; t < kNnTile; ++t) d[t] = nn_dist(qx, qy, qz, rr[3 * t], rr[3 * t + 1], rr[3 * t + 2]);
#pragma unroll
    for (int u = 0; u < kNnQpt; ++u) {
      float m = d[0][u];
#pragma unroll
      for (int t = 1; t + 1 < kNnTile; t += 2) m = fminf(fminf(m, d[t][u]), d[t + 1][u]);
      m = fminf(m, d[kNnTile - 1][u]);
      if (m < best[u]) {
        best[u] = m;
        bj[u] = j;
      }
    }
  }
  for (; j < j1; ++j) {  // partial last chunk: only the points that exist
    const float* c = rp + (long)j * 3;
    const f32x2 d = nn_dist(qx, qy, qz, c[0], c[1], c[2]);
#pragma unroll
    for (int u = 0; u < kNnQpt; ++u) {
      if (d[u] < best[u]) {
        best[u] = d[u];
        bj[u] = j;  // its own start: the re-scan matches at once
      }
    }
  }
  // the index inside the winning chunk (per-lane addresses, clamped to the segment)
  int bi[kNnQpt] = {bj[0], bj[1]};
  bool open[kNnQpt] = {true, true};
  for (int t = 0; t < kNnTile; ++t) {
    const int ja = min(bj[0] + t, j1 - 1), jb = min(bj[1] + t, j1 - 1);
    const float* ca = rp + (long)ja * 3;
    const float* cb = rp + (long)jb * 3;
    const float da = nn_dist(qx, qy, qz, ca[0], ca[1], ca[2])[0];
    const float db = nn_dist(qx, qy, qz, cb[0], cb[1], cb[2])[1];
    if (open[0] && da == best[0]) {
      bi[0] = ja;
      open[0] = false;
    }
    if (open[1] && db == best[1]) {
      bi[1] = jb;
      open[1] = false;
    }
  }
#pragma unroll
  for (int u = 0; u < kNnQpt; ++u) {
    const int i = qb * kNnQpb + u * kNnBlock + (int)threadIdx.x;
    if (i < n) {
      const long o = ((long)s * batch + b) * n + i;
      dist2[o] = best[u];
      idx[o] = bi[u];
    }
  }
}

// Merge of the per-segment winners, ascending segment = ascending index, so
// the strict '<' keeps the lowest index among equal distances.
__global__ __launch_bounds__(256) void nn_merge_k(const float* __restrict__ seg_d, const int* __restrict__ seg_i,
                                                  float* __restrict__ dist2, int* __restrict__ idx, long total,
                                                  int nseg) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  float best = seg_d[t];
  int bi = seg_i[t];
  for (int s = 1; s < nseg; ++s) {
    const float d = seg_d[s * total + t];
    if (d < best) {
      best = d;
      bi = seg_i[s * total + t];
    }
  }
  dist2[t] = best;
  idx[t] = bi;
}

// One thread per generated point (b, i):
//   gx = wx[b] * 2 (x_i - y[idx_xy[b,i]]) + wy[b] * sum_{e in segment (b,i)} 2 (x_i - y[seg_j[b,e]])
// The segment lists the targets whose nearest generated point is i, ascending
// (a stable sort of idx_yx), and is summed in that order by this one thread:
// no atomics.  Indices read from memory are clamped into range (never fault).
__global__ __launch_bounds__(256) void chamfer_bwd_k(const float* __restrict__ x, const float* __restrict__ y,
                                                     const int* __restrict__ idx_xy, const int* __restrict__ seg_ptr,
                                                     const int* __restrict__ seg_j, const float* __restrict__ wx,
                                                     const float* __restrict__ wy, float* __restrict__ gx, int n,
                                                     int p, long y_bs, long total) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int b = (int)(t / n), i = (int)(t - (long)b * n);
  const float* yb = y + (long)b * y_bs;
  const float x0 = x[t * 3], x1 = x[t * 3 + 1], x2 = x[t * 3 + 2];
  const int k = min(max(idx_xy[t], 0), p - 1);
  const float a = wx[b], c = wy[b];
  float g0 = a * (2.f * (x0 - yb[(long)k * 3]));
  float g1 = a * (2.f * (x1 - yb[(long)k * 3 + 1]));
  float g2 = a * (2.f * (x2 - yb[(long)k * 3 + 2]));
  const int* sp = seg_ptr + (long)b * (n + 1) + i;
  const int e0 = min(max(sp[0], 0), p), e1 = min(max(sp[1], 0), p);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int e = e0; e < e1; ++e) {
    const int j = min(max(seg_j[(long)b * p + e], 0), p - 1);
    s0 += 2.f * (x0 - yb[(long)j * 3]);
    s1 += 2.f * (x1 - yb[(long)j * 3 + 1]);
    s2 += 2.f * (x2 - yb[(long)j * 3 + 2]);
  }
  gx[t * 3] = g0 + c * s0;
  gx[t * 3 + 1] = g1 + c * s1;
  gx[t * 3 + 2] = g2 + c * s2;
}

static int nn_check_sizes(const char* what, int batch, int bq, int br, int n, int p) {
  if (batch <= 0 || n <= 0 || p <= 0)
    return set_error(CFSD_EINVAL, "%s: bad sizes batch=%d n=%d p=%d (all must be >= 1)", what, batch, n, p);
  if ((bq != 1 && bq != batch) || (br != 1 && br != batch))
    return set_error(CFSD_EINVAL, "%s: operand batches %d and %d must each be 1 or %d", what, bq, br, batch);
  if ((long)batch * n * 3 >= (1L << 31) || (long)batch * p * 3 >= (1L << 31))
    return set_error(CFSD_EINVAL, "%s: batch x points x 3 >= 2^31 (32-bit indices)", what);
  return CFSD_OK;
}

}  // namespace cfsd

using namespace cfsd;

extern "C" size_t cfsd_nn_points_workspace(int batch, int n, int p) {
  if (batch <= 0 || n <= 0 || p <= 0 || (long)batch * n * 3 >= (1L << 31) || (long)batch * p * 3 >= (1L << 31))
    return 0;
  const NnSplit sp = nn_split(batch, n, p);
  return sp.nseg > 1 ? (size_t)sp.nseg * batch * n * 8 : 0;
}

extern "C" int cfsd_nn_points(const float* q, const float* r, float* dist2, int32_t* idx, void* workspace,
                              size_t workspace_bytes, int batch, int bq, int br, int n, int p, void* stream) {
  if (!q || !r || !dist2 || !idx) return set_error(CFSD_EINVAL, "nn_points: null pointer");
  if (int rc = nn_check_sizes("nn_points", batch, bq, br, n, p)) return rc;
  const NnSplit sp = nn_split(batch, n, p);
  const long total = (long)batch * n;
  const size_t need = sp.nseg > 1 ? (size_t)sp.nseg * total * 8 : 0;
  if (need && (!workspace || workspace_bytes < need))
    return set_error(CFSD_EWORKSPACE, "nn_points: workspace %zu < %zu bytes", workspace_bytes, need);
  const int qblocks = (n + kNnQpb - 1) / kNnQpb;
  const long blocks = (long)batch * sp.nseg * qblocks;
  if (blocks >= (1L << 31)) return set_error(CFSD_EINVAL, "nn_points: too many workgroups");
  float* seg_d = need ? (float*)workspace : dist2;
  int* seg_i = need ? (int*)((float*)workspace + (size_t)sp.nseg * total) : idx;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nn_points_k, dim3((unsigned)blocks), dim3(kNnBlock), 0, st, q, r, seg_d, seg_i, batch, n, p,
                     bq == 1 ? 0L : (long)n * 3, br == 1 ? 0L : (long)p * 3, qblocks, sp.nseg, sp.seg_len);
  if (need)
    hipLaunchKernelGGL(nn_merge_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, seg_d, seg_i, dist2, idx,
                       total, sp.nseg);
  return launch_status("nn_points");
}

extern "C" int cfsd_chamfer_bwd(const float* x, const float* y, const int32_t* idx_xy, const int32_t* seg_ptr,
                                const int32_t* seg_j, const float* wx, const float* wy, float* gx, int batch, int by,
                                int n, int p, void* stream) {
  if (!x || !y || !idx_xy || !seg_ptr || !seg_j || !wx || !wy || !gx)
    return set_error(CFSD_EINVAL, "chamfer_bwd: null pointer");
  if (int rc = nn_check_sizes("chamfer_bwd", batch, batch, by, n, p)) return rc;
  const long total = (long)batch * n;
  hipLaunchKernelGGL(chamfer_bwd_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y,
                     idx_xy, seg_ptr, seg_j, wx, wy, gx, n, p, by == 1 ? 0L : (long)p * 3, total);
  return launch_status("chamfer_bwd");
}
