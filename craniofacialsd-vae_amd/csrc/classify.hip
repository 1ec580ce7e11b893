// Classifiers on the latent code (gfx950): per-class statistics and
// discriminant scores for LDA / QDA, and the MLP classifier's forward pass and
// fused train step.
//
// Reference: ModelManager.train_and_validate_classifiers
// (model_manager.py:448-504) fits scikit-learn's LinearDiscriminantAnalysis /
// QuadraticDiscriminantAnalysis and trains MLPClassifier (model.py:191-203:
// Linear + ReLU after EVERY layer) with CrossEntropyLoss(weight) and Adam in
// batches of `batch_size` latents (mlp_classifier_epoch, :428-446).
//
// Every reduction runs in an order fixed by the shapes alone (no atomics, no
// grid-wide barrier; dependent phases are separate launches), so two runs
// give the same bits.
//
// Statistics.  Rows are cut into R slices (a function of n); a workgroup
// walks its slice in chunks of 64 rows: one wave ballots the chunk's labels,
// the rows of the workgroup's class are compacted IN ASCENDING ORDER and
// staged (centred in the second pass) through LDS, and each thread adds them
// to the output elements it owns.  The slice partials are merged in
// ascending slice order by a second launch.  Sums of the mean pass are
// compensated (Kahan), so a mean is within an ulp or two of the exact one.
//
// Scores.  A workgroup owns 64 rows, staged once; per class the whitening
// matrix passes through LDS in panels of 32 columns, thread (row, q) forms
// the projections of columns q, q + 4, ... and the four partial squared norms
// of a row are added in ascending q.
//
// MLP.  A layer is a wave per output neuron: lanes stride the input width
// (coalesced weight rows), all rows of the tile share each weight, a xor
// butterfly sums the lanes.  The train step's first launch is ONE workgroup
// (forward, weighted cross-entropy, activation gradients; layer inputs x_l
// and output gradients dy_l left in the workspace), the second covers the
// parameters: each thread forms its element's gradient (<= 16 terms,
// ascending row) and applies Adam in place.  The same two launches serve as a
// head of the VAE step (cfsd_mlp_head_step, mlp_training_type: end2end,
// model_manager.py:295-318): rows strided through the step's latent codes,
// labels gathered through its batch indices, the backward continued one layer
// into the latent gradient, the parameters' gradient scaled by the loss weight.
#include <math.h>

#include "cfsd_common.h"

namespace cfsd {

constexpr int kClsMaxD = CFSD_CLS_MAX_D;
constexpr int kClsMaxC = CFSD_CLS_MAX_CLASSES;
constexpr int kStatRows = 64;         // rows per staged chunk: one wave ballots their labels
constexpr int kStatThreads = 256;
constexpr int kStatSliceRows = 2048;  // least rows worth a slice of their own
constexpr int kStatMaxSlices = 16;

static int stat_slices(int n) {
  const int r = (n + kStatSliceRows - 1) / kStatSliceRows;
  return r < 1 ? 1 : (r > kStatMaxSlices ? kStatMaxSlices : r);
}
// rows of the d x d scatter one workgroup owns (one output element per thread)
static int stat_tile_rows(int d) {
  const int ta = kStatThreads / d;
  return ta < 1 ? 1 : (ta > d ? d : ta);
}
static size_t stat_workspace_floats(int n, int d, int c) {
  const size_t r = (size_t)stat_slices(n);
  return r * c * d * d + r * c * d + r * c;
}

__device__ __forceinline__ void kahan_add(float& sum, float& comp, float x) {
  const float y = x - comp, t = sum + y;
  comp = (t - sum) - y;
  sum = t;
}

// Stages the rows of class c among [i0, min(i0 + 64, i1)), ascending, as
// xs[k * d + j] = z[row_k, col0 + j] - centre[j] (centre may be NULL).
// Returns their number.  The caller puts a barrier between its last read of
// xs and the next call.
__device__ __forceinline__ int stage_class_rows(const float* __restrict__ z, const int* __restrict__ label,
                                                const float* __restrict__ centre, int ld, int col0, int d, int c,
                                                int i0, int i1, int* sel, int* cnt, float* xs) {
  if (threadIdx.x < 64) {
    const int i = i0 + (int)threadIdx.x;
    const bool in = i < i1 && label[i] == c;
    const unsigned long long m = __ballot(in);
    if (in) sel[__popcll(m & ((1ull << threadIdx.x) - 1ull))] = i;
    if (threadIdx.x == 0) *cnt = __popcll(m);
  }
  __syncthreads();
  const int kn = *cnt;
  for (int e = threadIdx.x; e < kn * d; e += blockDim.x) {
    const int k = e / d, j = e - k * d;
    xs[e] = z[(long)sel[k] * ld + col0 + j] - (centre ? centre[j] : 0.f);
  }
  __syncthreads();
  return kn;
}

// Block (c, s): column sums and the count of class c over slice s.
__global__ __launch_bounds__(kStatThreads) void class_sum_k(const float* __restrict__ z,
                                                            const int* __restrict__ label, float* __restrict__ psum,
                                                            int* __restrict__ pcount, int n, int ld, int col0, int d,
                                                            int n_classes, int slice_rows) {
  __shared__ int sel[kStatRows];
  __shared__ int cnt;
  __shared__ float xs[kStatRows * kClsMaxD];
  const int c = blockIdx.x, s = blockIdx.y, j = threadIdx.x;
  const int r0 = min(n, s * slice_rows), r1 = min(n, r0 + slice_rows);
  float sum = 0.f, comp = 0.f;
  int total = 0;
  for (int i0 = r0; i0 < r1; i0 += kStatRows) {
    const int kn = stage_class_rows(z, label, nullptr, ld, col0, d, c, i0, r1, sel, &cnt, xs);
    total += kn;
    if (j < d)
      for (int k = 0; k < kn; ++k) kahan_add(sum, comp, xs[k * d + j]);
    __syncthreads();
  }
  if (j < d) psum[((long)s * n_classes + c) * d + j] = sum;
  if (j == 0) pcount[s * n_classes + c] = total;
}

__global__ __launch_bounds__(256) void class_mean_k(const float* __restrict__ psum, const int* __restrict__ pcount,
                                                    int* __restrict__ count, float* __restrict__ mean, int n_classes,
                                                    int d, int slices) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_classes * d) return;
  const int c = t / d;
  int nc = 0;
  float sum = 0.f, comp = 0.f;
  for (int s = 0; s < slices; ++s) {
    nc += pcount[s * n_classes + c];
    kahan_add(sum, comp, psum[(long)s * n_classes * d + t]);
  }
  mean[t] = nc > 0 ? sum / (float)nc : 0.f;
  if (t - c * d == 0) count[c] = nc;
}

// Block (tile, c, s): rows [tile * ta, +ta) of class c's centred scatter over slice s.
__global__ __launch_bounds__(kStatThreads) void class_scatter_k(const float* __restrict__ z,
                                                                const int* __restrict__ label,
                                                                const float* __restrict__ mean,
                                                                float* __restrict__ pscatter, int n, int ld, int col0,
                                                                int d, int n_classes, int slice_rows, int ta) {
  __shared__ int sel[kStatRows];
  __shared__ int cnt;
  __shared__ float xs[kStatRows * kClsMaxD];
  const int c = blockIdx.y, s = blockIdx.z, a0 = blockIdx.x * ta;
  const int na = min(ta, d - a0);
  const bool own = (int)threadIdx.x < na * d;
  const int a = own ? a0 + (int)threadIdx.x / d : 0, b = own ? (int)threadIdx.x % d : 0;
  const int r0 = min(n, s * slice_rows), r1 = min(n, r0 + slice_rows);
  float acc = 0.f;
  for (int i0 = r0; i0 < r1; i0 += kStatRows) {
    const int kn = stage_class_rows(z, label, mean + (long)c * d, ld, col0, d, c, i0, r1, sel, &cnt, xs);
    if (own)
      for (int k = 0; k < kn; ++k) acc = fmaf(xs[k * d + a], xs[k * d + b], acc);
    __syncthreads();
  }
  if (own) pscatter[(((long)s * n_classes + c) * d + a) * d + b] = acc;
}

__global__ __launch_bounds__(256) void class_scatter_merge_k(const float* __restrict__ pscatter,
                                                             float* __restrict__ scatter, long total, int slices) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  float sum = pscatter[t];
  for (int s = 1; s < slices; ++s) sum += pscatter[s * total + t];
  scatter[t] = sum;
}

// ------------------------------------------------------------ scores
constexpr int kDsRows = 64;
constexpr int kDsThreads = 256;
constexpr int kDsPanel = 32;  // whitening columns per LDS panel
constexpr int kDsCpt = kDsPanel / (kDsThreads / kDsRows);  // panel columns per thread

__global__ __launch_bounds__(kDsThreads) void discriminant_k(const float* __restrict__ z,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ whiten,
                                                             const float* __restrict__ offset,
                                                             float* __restrict__ maha2, float* __restrict__ scores,
                                                             int* __restrict__ pred, int n, int ld, int col0, int d,
                                                             int n_classes, int n_whiten) {
  __shared__ float xs[kDsRows * (kClsMaxD + 1)];  // row stride d | 1: odd, conflict-free down a column
  __shared__ float wp[kClsMaxD * kDsPanel];
  __shared__ float mc[kClsMaxD];
  __shared__ float part[kDsThreads];
  const int r = threadIdx.x & (kDsRows - 1), q = threadIdx.x / kDsRows;
  const long i0 = (long)blockIdx.x * kDsRows;
  const int rows = (int)min((long)kDsRows, n - i0);
  const int xld = d | 1;
  for (int e = threadIdx.x; e < kDsRows * d; e += kDsThreads) {
    const int k = e / d, j = e - k * d;
    xs[k * xld + j] = k < rows ? z[(i0 + k) * ld + col0 + j] : 0.f;
  }
  float best = -INFINITY;
  int bi = 0;
  for (int c = 0; c < n_classes; ++c) {
    const float* W = whiten + (n_whiten == 1 ? 0L : (long)c * d * d);
    __syncthreads();  // the previous class's mc / part are consumed; xs is staged
    if ((int)threadIdx.x < d) mc[threadIdx.x] = mean[(long)c * d + threadIdx.x];
    float m2 = 0.f;
    for (int k0 = 0; k0 < d; k0 += kDsPanel) {
      const int kw = min(kDsPanel, d - k0);
      __syncthreads();  // the previous panel is consumed; mc is visible
      for (int e = threadIdx.x; e < d * kDsPanel; e += kDsThreads) {
        const int j = e / kDsPanel, kk = e - j * kDsPanel;
        wp[e] = kk < kw ? W[(long)j * d + k0 + kk] : 0.f;
      }
      __syncthreads();
      float y[kDsCpt];
#pragma unroll
      for (int u = 0; u < kDsCpt; ++u) y[u] = 0.f;
      for (int j = 0; j < d; ++j) {
        const float x = xs[r * xld + j] - mc[j];
#pragma unroll
        for (int u = 0; u < kDsCpt; ++u) y[u] = fmaf(x, wp[j * kDsPanel + q + (kDsThreads / kDsRows) * u], y[u]);
      }
#pragma unroll
      for (int u = 0; u < kDsCpt; ++u) m2 = fmaf(y[u], y[u], m2);
    }
    part[threadIdx.x] = m2;
    __syncthreads();
    if (q == 0) {
      float t = part[r];
#pragma unroll
      for (int g = 1; g < kDsThreads / kDsRows; ++g) t += part[g * kDsRows + r];
      const float sc = fmaf(-0.5f, t, offset[c]);
      if (r < rows) {
        if (maha2) maha2[(i0 + r) * n_classes + c] = t;
        if (scores) scores[(i0 + r) * n_classes + c] = sc;
      }
      if (sc > best) {  // strict: the lowest class wins a tie
        best = sc;
        bi = c;
      }
    }
  }
  if (q == 0 && r < rows && pred) pred[i0 + r] = bi;
}

// ------------------------------------------------------------ MLP
constexpr int kMlpMaxLayers = CFSD_MLP_MAX_LAYERS;
constexpr int kMlpMaxWidth = CFSD_MLP_MAX_WIDTH;
constexpr int kMlpMaxBs = CFSD_MLP_MAX_BS;
constexpr int kMlpFwdThreads = 512;
constexpr int kMlpStepThreads = 1024;
constexpr size_t kMlpLdsMax = 159 * 1024;

// Layer l maps dims[l] -> dims[l + 1]; its W [dims[l+1], dims[l]] starts at
// woff[l] of the flat parameters and is followed by its bias (state_dict order).
struct MlpDesc {
  int n_layers, total, maxw;
  int dims[kMlpMaxLayers + 1];
  int woff[kMlpMaxLayers + 1];
};

static int mlp_describe(const char* what, const int* dims, int n_layers, MlpDesc& D) {
  if (!dims) return set_error(CFSD_EINVAL, "%s: null dims", what);
  if (n_layers < 1 || n_layers > kMlpMaxLayers)
    return set_error(CFSD_EINVAL, "%s: %d layers (1..%d supported)", what, n_layers, kMlpMaxLayers);
  D.n_layers = n_layers;
  D.maxw = 0;
  long off = 0;
  for (int l = 0; l <= n_layers; ++l) {
    if (dims[l] < 1 || dims[l] > kMlpMaxWidth)
      return set_error(CFSD_EINVAL, "%s: width %d of layer %d (1..%d supported)", what, dims[l], l, kMlpMaxWidth);
    D.dims[l] = dims[l];
    D.maxw = dims[l] > D.maxw ? dims[l] : D.maxw;
    D.woff[l] = (int)off;
    if (l < n_layers) off += (long)dims[l + 1] * dims[l] + dims[l + 1];
  }
  for (int l = n_layers + 1; l <= kMlpMaxLayers; ++l) D.dims[l] = 0, D.woff[l] = (int)off;
  D.total = (int)off;
  return CFSD_OK;
}

// workspace of a step, in floats per batch row: x_l (l < L) then dy_l (l < L)
__host__ __device__ inline int mlp_x_off(const MlpDesc& D, int l) {
  int o = 0;
  for (int m = 0; m < l; ++m) o += D.dims[m];
  return o;
}
__host__ __device__ inline int mlp_dy_off(const MlpDesc& D, int l) {
  int o = 0;
  for (int m = 0; m < D.n_layers; ++m) o += D.dims[m];
  for (int m = 0; m < l; ++m) o += D.dims[m + 1];
  return o;
}

// xout[i, o] = relu(b[o] + sum_k W[o, k] xin[i, k]) for the RB rows of an LDS
// tile (row stride ldx): a wave per output neuron, lanes over k.  A wave
// works on NU neurons at a time so that NU weight rows are in flight
// together (one row per trip is a memory latency per neuron); every neuron's
// own sum keeps one order (ascending k per lane, then the butterfly).
template <int RB>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ W, const float* __restrict__ b, const float* xin,
                                          float* xout, int n_in, int n_out, int ldx) {
  constexpr int NU = RB <= 4 ? 4 : (RB <= 8 ? 2 : 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int o0 = wave * NU; o0 < n_out; o0 += nw * NU) {
    const float* w[NU];
    float bias[NU];  // loaded with the weights: a load after the butterfly is a memory latency per neuron
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int o = min(o0 + u, n_out - 1);  // clamped: loads only
      w[u] = W + (long)o * n_in;
      bias[u] = b[o];
    }
    float acc[NU][RB];
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[u][i] = 0.f;
#pragma unroll 2
    for (int k = lane; k < n_in; k += 64) {
      float wk[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) wk[u] = w[u][k];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const float x = xin[i * ldx + k];
#pragma unroll
        for (int u = 0; u < NU; ++u) acc[u][i] = fmaf(wk[u], x, acc[u][i]);
      }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < RB; ++i) {
#pragma unroll
        for (int off = 32; off; off >>= 1) acc[u][i] += __shfl_xor(acc[u][i], off);
        if (lane == i) v = acc[u][i];
      }
      if (lane < RB && o0 + u < n_out) xout[lane * ldx + o0 + u] = fmaxf(v + bias[u], 0.f);
    }
  }
}

// rows [i0, i0 + rows) of z [*, n0] into an LDS tile of RB rows, the rest zero
template <int RB>
__device__ __forceinline__ void mlp_load_rows(const float* __restrict__ z, long i0, int rows, int n0, float* x,
                                              int ldx) {
  for (int e = threadIdx.x; e < RB * n0; e += blockDim.x) {
    const int i = e / n0, k = e - i * n0;
    x[i * ldx + k] = i < rows ? z[(i0 + i) * n0 + k] : 0.f;
  }
}

template <int RB>
__global__ __launch_bounds__(kMlpFwdThreads) void mlp_fwd_k(MlpDesc D, const float* __restrict__ z,
                                                            const float* __restrict__ params,
                                                            float* __restrict__ logits, int* __restrict__ pred,
                                                            int n) {
  extern __shared__ float mlp_lds[];
  const int ldx = D.maxw;
  float* A = mlp_lds;
  float* B = mlp_lds + RB * ldx;
  const long i0 = (long)blockIdx.x * RB;
  const int rows = (int)min((long)RB, n - i0);
  mlp_load_rows<RB>(z, i0, rows, D.dims[0], A, ldx);
  __syncthreads();
  for (int l = 0; l < D.n_layers; ++l) {
    const float* W = params + D.woff[l];
    mlp_layer<RB>(W, W + (long)D.dims[l + 1] * D.dims[l], A, B, D.dims[l], D.dims[l + 1], ldx);
    __syncthreads();
    float* t = A;
    A = B;
    B = t;
  }
  const int C = D.dims[D.n_layers];
  for (int e = threadIdx.x; e < rows * C; e += blockDim.x) {
    const int i = e / C, c = e - i * C;
    logits[(i0 + i) * C + c] = A[i * ldx + c];
  }
  if (pred && (int)threadIdx.x < rows) {
    const float* o = A + threadIdx.x * ldx;
    int bi = 0;
    for (int c = 1; c < C; ++c)
      if (o[c] > o[bi]) bi = c;
    pred[i0 + threadIdx.x] = bi;
  }
}

// What the head step (cfsd_mlp_head_step) adds to a step's first launch: rows
// strided through z, labels looked up through the step's batch indices, and
// (train) the gradient w.r.t. the input rows added to dlat.
struct MlpHead {
  const int* batch_idx;    // [bs] rows of label_table
  const int* label_table;  // [n_labels] class indices
  float* dlat;             // row i at dlat + i * dlat_stride; the first dims[0] columns gain w_cls * dz_i
  long z_stride, dlat_stride;
  int n_labels;
  float w_cls;
};

// First launch of a step, ONE workgroup: forward of bs rows, loss / accuracy
// into acc[3], and (train) the activation gradients.  HEAD = false
// (cfsd_mlp_train_steps): rows [row_base, +bs) of z [*, dims[0]], labelled by
// row number.  HEAD = true (cfsd_mlp_head_step): row i at z + i * H.z_stride,
// labelled label_table[batch_idx[i]], and the backward continues through
// layer 0 into H.dlat.
template <int RB, bool HEAD>
__device__ __forceinline__ void mlp_step_body(const MlpDesc& D, const float* __restrict__ z,
                                              const int* __restrict__ label, const float* __restrict__ cw,
                                              const float* __restrict__ params, float* __restrict__ ws,
                                              float* __restrict__ acc, int* __restrict__ step, long row_base, int bs,
                                              int train, const MlpHead& H) {
  extern __shared__ float mlp_lds[];
  __shared__ float s_li[kMlpMaxBs], s_wi[kMlpMaxBs], s_lse[kMlpMaxBs];
  __shared__ int s_y[kMlpMaxBs], s_ok[kMlpMaxBs];
  __shared__ float s_wsum;
  const int ldx = D.maxw, L = D.n_layers;
  // two activation tiles; the backward pass keeps dy in one and up to 16
  // waves x 64 columns of partial sums per row in the other
  float* A = mlp_lds;
  float* B = mlp_lds + RB * (train ? kMlpMaxWidth : ldx);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if constexpr (HEAD) {
    const int n0 = D.dims[0];
    for (int e = threadIdx.x; e < RB * n0; e += blockDim.x) {
      const int i = e / n0, k = e - i * n0;
      A[i * ldx + k] = i < bs ? z[i * H.z_stride + k] : 0.f;
    }
  } else {
    mlp_load_rows<RB>(z, row_base, bs, D.dims[0], A, ldx);
  }
  __syncthreads();
  for (int l = 0; l < L; ++l) {
    const int n_in = D.dims[l], n_out = D.dims[l + 1];
    if (train) {  // x_l, the layer's input, for the weight gradient and the ReLU mask
      float* xl = ws + (long)bs * mlp_x_off(D, l);
      for (int e = threadIdx.x; e < bs * n_in; e += blockDim.x) {
        const int i = e / n_in, k = e - i * n_in;
        xl[e] = A[i * ldx + k];
      }
    }
    const float* W = params + D.woff[l];
    mlp_layer<RB>(W, W + (long)n_out * n_in, A, B, n_in, n_out, ldx);
    __syncthreads();
    float* t = A;
    A = B;
    B = t;
  }
  // A: the logits o [bs, C] (after the last ReLU).  Wave i takes row i.
  const int C = D.dims[L];
  if (wave < bs) {
    const float* o = A + wave * ldx;
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < C; c += 64)
      if (o[c] > m) {
        m = o[c];
        am = c;
      }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const float om = __shfl_xor(m, off);
      const int oa = __shfl_xor(am, off);
      if (om > m || (om == m && oa < am)) {
        m = om;
        am = oa;
      }
    }
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(o[c] - m);
#pragma unroll
    for (int off = 32; off; off >>= 1) se += __shfl_xor(se, off);
    if (lane == 0) {
      int y;
      if constexpr (HEAD)
        y = H.label_table[min(max(H.batch_idx[wave], 0), H.n_labels - 1)];
      else
        y = label[row_base + wave];
      y = min(max(y, 0), C - 1);
      const float lse = m + logf(se);
      s_y[wave] = y;
      s_lse[wave] = lse;
      s_li[wave] = lse - o[y];
      s_wi[wave] = cw[y];
      s_ok[wave] = am == y;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float wsum = 0.f, num = 0.f;
    int ok = 0;
    for (int i = 0; i < bs; ++i) {
      wsum += s_wi[i];
      num = fmaf(s_wi[i], s_li[i], num);
      ok += s_ok[i];
    }
    s_wsum = wsum;
    acc[0] += num / wsum;
    acc[1] += 100.f * (float)ok / (float)bs;
    acc[2] += 1.f;
    if (train) *step += 1;
  }
  if (!train) return;
  __syncthreads();
  {  // dy_{L-1}: d loss / d (pre-ReLU logits), in place
    float* dy = ws + (long)bs * mlp_dy_off(D, L - 1);
    const float wsum = s_wsum;
    for (int e = threadIdx.x; e < bs * C; e += blockDim.x) {
      const int i = e / C, c = e - i * C;
      const float o = A[i * ldx + c];
      const float p = expf(o - s_lse[i]);
      const float g = o > 0.f ? (s_wi[i] / wsum) * (p - (c == s_y[i] ? 1.f : 0.f)) : 0.f;
      A[i * ldx + c] = g;
      dy[e] = g;
    }
  }
  __syncthreads();
  // dy_{l-1} = (dy_l W_l) * [x_l > 0].  Wave (tile, g): input columns
  // [64 tile, +64), output neurons g, g + G, ...; the G partials of a column
  // are added in ascending g.  HEAD: one layer further, dz = dy_0 W_0 (no
  // mask: the input is z), added to dlat by the thread that owns the element.
  for (int l = L - 1; l >= (HEAD ? 0 : 1); --l) {
    const int n_in = D.dims[l], n_out = D.dims[l + 1];
    const int tiles = (n_in + 63) / 64, G = nw / tiles, pld = tiles * 64;
    const int tile = wave % tiles, g = wave / tiles, k = tile * 64 + lane;
    if (g < G) {
      const float* W = params + D.woff[l];
      float a[RB];
#pragma unroll
      for (int i = 0; i < RB; ++i) a[i] = 0.f;
      if (k < n_in) {
        // UB weight rows are loaded before the first of them is used (left to
        // the compiler, every trip waited out its own load); the sum keeps
        // ascending o
        constexpr int UB = RB <= 8 ? 8 : 4;
        int o = g;
        for (; o + (UB - 1) * G < n_out; o += UB * G) {
          float wv[UB];
#pragma unroll
          for (int t = 0; t < UB; ++t) wv[t] = W[(long)(o + t * G) * n_in + k];
#pragma unroll
          for (int t = 0; t < UB; ++t)
#pragma unroll
            for (int i = 0; i < RB; ++i) a[i] = fmaf(A[i * ldx + o + t * G], wv[t], a[i]);
        }
        for (; o < n_out; o += G) {
          const float w = W[(long)o * n_in + k];
#pragma unroll
          for (int i = 0; i < RB; ++i) a[i] = fmaf(A[i * ldx + o], w, a[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < RB; ++i) B[(g * RB + i) * pld + k] = a[i];
    }
    __syncthreads();
    if (HEAD && l == 0) {
      for (int e = threadIdx.x; e < bs * n_in; e += blockDim.x) {
        const int i = e / n_in, kk = e - i * n_in;
        float s = B[i * pld + kk];
        for (int gg = 1; gg < G; ++gg) s += B[(gg * RB + i) * pld + kk];
        float* d = H.dlat + i * H.dlat_stride + kk;
        *d = fmaf(H.w_cls, s, *d);
      }
      return;
    }
    const float* xl = ws + (long)bs * mlp_x_off(D, l);
    float* dy = ws + (long)bs * mlp_dy_off(D, l - 1);
    for (int e = threadIdx.x; e < bs * n_in; e += blockDim.x) {
      const int i = e / n_in, kk = e - i * n_in;
      float s = B[i * pld + kk];
      for (int gg = 1; gg < G; ++gg) s += B[(gg * RB + i) * pld + kk];
      const float v = xl[e] > 0.f ? s : 0.f;
      A[i * ldx + kk] = v;
      dy[e] = v;
    }
    __syncthreads();
  }
}

template <int RB>
__global__ __launch_bounds__(kMlpStepThreads) void mlp_step_k(MlpDesc D, const float* __restrict__ z,
                                                              const int* __restrict__ label,
                                                              const float* __restrict__ cw,
                                                              const float* __restrict__ params, float* __restrict__ ws,
                                                              float* __restrict__ acc, int* __restrict__ step,
                                                              long row_base, int bs, int train) {
  mlp_step_body<RB, false>(D, z, label, cw, params, ws, acc, step, row_base, bs, train, MlpHead{});
}

template <int RB>
__global__ __launch_bounds__(kMlpStepThreads) void mlp_head_k(MlpDesc D, const float* __restrict__ z,
                                                              const float* __restrict__ cw,
                                                              const float* __restrict__ params, float* __restrict__ ws,
                                                              float* __restrict__ acc, int* __restrict__ step, int bs,
                                                              int train, MlpHead H) {
  mlp_step_body<RB, true>(D, z, nullptr, cw, params, ws, acc, step, 0, bs, train, H);
}

// Second launch of a step: one thread per parameter.  HEAD: the gradient is
// that of w_cls * loss (gscale = w_cls), and without moments (m == NULL) it is
// only written out (the data-parallel step: Adam follows the all-reduce).
template <bool HEAD>
__global__ __launch_bounds__(256) void mlp_adam_k(MlpDesc D, float* __restrict__ params, float* __restrict__ m,
                                                  float* __restrict__ v, const float* __restrict__ ws,
                                                  const int* __restrict__ step, float* __restrict__ dw_out, int bs,
                                                  float lr, float b1, float b2, float eps, float wd, float gscale) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= D.total) return;
  int l = 0;
  while (l + 1 < D.n_layers && e >= D.woff[l + 1]) ++l;
  const int n_in = D.dims[l], n_out = D.dims[l + 1], local = e - D.woff[l];
  const float* dy = ws + (long)bs * mlp_dy_off(D, l);
  float g = 0.f;
  if (local < n_out * n_in) {
    const int o = local / n_in, k = local - o * n_in;
    const float* x = ws + (long)bs * mlp_x_off(D, l);
    for (int i = 0; i < bs; ++i) g = fmaf(dy[i * n_out + o], x[i * n_in + k], g);
  } else {
    const int o = local - n_out * n_in;
    for (int i = 0; i < bs; ++i) g += dy[i * n_out + o];
  }
  if constexpr (HEAD) g *= gscale;
  if (dw_out) dw_out[e] = g;
  if (HEAD && !m) return;
  const int t = *step;
  const float bc1 = 1.f - powf(b1, (float)t);
  const float sqrt_bc2 = sqrtf(1.f - powf(b2, (float)t));
  adam_elem(params[e], g, m[e], v[e], b1, b2, eps, wd, lr / bc1, sqrt_bc2);
}

static int mlp_rows_tile(int rows) { return rows <= 4 ? 4 : (rows <= 8 ? 8 : 16); }

static int mlp_raise_lds(const char* what, const void* kernel, size_t lds) {
  if (lds > kMlpLdsMax) return set_error(CFSD_EINVAL, "%s: needs %zu B of LDS (> %zu)", what, lds, kMlpLdsMax);
  // (static LDS of the kernel counts against the default 64 KB too)
  if (lds + 1024 > 64 * 1024 &&
      hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return set_error(CFSD_EINVAL, "%s: cannot raise the dynamic LDS limit", what);
  return CFSD_OK;
}

static int stats_check(const char* what, int n, int ld, int col0, int d, int c) {
  if (d < 1 || d > kClsMaxD || c < 1 || c > kClsMaxC)
    return set_error(CFSD_EINVAL, "%s: d=%d classes=%d (supported: d <= %d, classes <= %d)", what, d, c, kClsMaxD,
                     kClsMaxC);
  if (n < 1 || col0 < 0 || ld < col0 + d)
    return set_error(CFSD_EINVAL, "%s: bad sizes n=%d ld=%d col0=%d d=%d", what, n, ld, col0, d);
  return CFSD_OK;
}

}  // namespace cfsd

using namespace cfsd;

extern "C" size_t cfsd_class_stats_workspace(int n, int d, int n_classes) {
  if (n < 1 || d < 1 || d > kClsMaxD || n_classes < 1 || n_classes > kClsMaxC) return 0;
  return stat_workspace_floats(n, d, n_classes) * 4;
}

extern "C" int cfsd_class_stats(const float* z, const int32_t* label, int32_t* count, float* mean, float* scatter,
                                void* workspace, size_t workspace_bytes, int n, int ld, int col0, int d,
                                int n_classes, void* stream) {
  if (int rc = stats_check("class_stats", n, ld, col0, d, n_classes)) return rc;
  if (!z || !label || !count || !mean || !scatter || !workspace)
    return set_error(CFSD_EINVAL, "class_stats: null pointer");
  const size_t need = stat_workspace_floats(n, d, n_classes) * 4;
  if (workspace_bytes < need)
    return set_error(CFSD_EINVAL, "class_stats: workspace %zu < %zu bytes", workspace_bytes, need);
  const int R = stat_slices(n), slice_rows = (n + R - 1) / R, ta = stat_tile_rows(d);
  float* pscatter = (float*)workspace;
  float* psum = pscatter + (size_t)R * n_classes * d * d;
  int* pcount = (int*)(psum + (size_t)R * n_classes * d);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(class_sum_k, dim3(n_classes, R), dim3(kStatThreads), 0, st, z, label, psum, pcount, n, ld, col0,
                     d, n_classes, slice_rows);
  hipLaunchKernelGGL(class_mean_k, dim3((n_classes * d + 255) / 256), dim3(256), 0, st, psum, pcount, count, mean,
                     n_classes, d, R);
  hipLaunchKernelGGL(class_scatter_k, dim3((d + ta - 1) / ta, n_classes, R), dim3(kStatThreads), 0, st, z, label,
                     mean, pscatter, n, ld, col0, d, n_classes, slice_rows, ta);
  const long total = (long)n_classes * d * d;
  hipLaunchKernelGGL(class_scatter_merge_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pscatter,
                     scatter, total, R);
  return launch_status("class_stats");
}

extern "C" int cfsd_discriminant_scores(const float* z, const float* mean, const float* whiten, const float* offset,
                                        float* maha2, float* scores, int32_t* pred, int n, int ld, int col0, int d,
                                        int n_classes, int n_whiten, void* stream) {
  if (int rc = stats_check("discriminant_scores", n, ld, col0, d, n_classes)) return rc;
  if (n_whiten != 1 && n_whiten != n_classes)
    return set_error(CFSD_EINVAL, "discriminant_scores: %d whitening matrices (1 or %d)", n_whiten, n_classes);
  if (!z || !mean || !whiten || !offset) return set_error(CFSD_EINVAL, "discriminant_scores: null pointer");
  hipLaunchKernelGGL(discriminant_k, dim3((unsigned)((n + kDsRows - 1) / kDsRows)), dim3(kDsThreads), 0,
                     (hipStream_t)stream, z, mean, whiten, offset, maha2, scores, pred, n, ld, col0, d, n_classes,
                     n_whiten);
  return launch_status("discriminant_scores");
}

template <int RB>
static int mlp_fwd_launch(const MlpDesc& D, const float* z, const float* params, float* logits, int32_t* pred, int n,
                          hipStream_t st) {
  const size_t lds = (size_t)2 * RB * D.maxw * 4;
  if (int rc = mlp_raise_lds("mlp_fwd", (const void*)mlp_fwd_k<RB>, lds)) return rc;
  hipLaunchKernelGGL(mlp_fwd_k<RB>, dim3((unsigned)((n + RB - 1) / RB)), dim3(kMlpFwdThreads), lds, st, D, z, params,
                     logits, pred, n);
  return launch_status("mlp_fwd");
}

extern "C" int cfsd_mlp_fwd(const float* z, const float* params, float* logits, int32_t* pred, const int* dims,
                            int n_layers, int n, void* stream) {
  MlpDesc D;
  if (int rc = mlp_describe("mlp_fwd", dims, n_layers, D)) return rc;
  if (n < 1) return set_error(CFSD_EINVAL, "mlp_fwd: n=%d", n);
  if (!z || !params || !logits) return set_error(CFSD_EINVAL, "mlp_fwd: null pointer");
  const hipStream_t st = (hipStream_t)stream;
  switch (mlp_rows_tile(n)) {
    case 4: return mlp_fwd_launch<4>(D, z, params, logits, pred, n, st);
    case 8: return mlp_fwd_launch<8>(D, z, params, logits, pred, n, st);
    default: return mlp_fwd_launch<16>(D, z, params, logits, pred, n, st);
  }
}

extern "C" size_t cfsd_mlp_workspace(const int* dims, int n_layers, int bs) {
  MlpDesc D;
  if (!dims || n_layers < 1 || n_layers > kMlpMaxLayers || bs < 1 || bs > kMlpMaxBs) return 0;
  if (mlp_describe("mlp_workspace", dims, n_layers, D)) return 0;
  return (size_t)bs * mlp_dy_off(D, n_layers) * 4;
}

template <int RB>
static int mlp_steps_launch(const MlpDesc& D, const float* z, const int32_t* label, const float* cw, float* params,
                            float* m, float* v, int32_t* step, float* acc, float* ws, float* dw_out, long row0,
                            int bs, int n_steps, int train, float lr, float b1, float b2, float eps, float wd,
                            hipStream_t st) {
  const size_t lds = (size_t)2 * RB * (train ? kMlpMaxWidth : D.maxw) * 4;
  if (int rc = mlp_raise_lds("mlp_train_steps", (const void*)mlp_step_k<RB>, lds)) return rc;
  for (int t = 0; t < n_steps; ++t) {
    hipLaunchKernelGGL(mlp_step_k<RB>, dim3(1), dim3(kMlpStepThreads), lds, st, D, z, label, cw, params, ws, acc,
                       step, row0 + (long)t * bs, bs, train);
    if (train)
      hipLaunchKernelGGL(mlp_adam_k<false>, dim3((D.total + 255) / 256), dim3(256), 0, st, D, params, m, v, ws, step,
                         dw_out, bs, lr, b1, b2, eps, wd, 1.f);
  }
  return launch_status("mlp_train_steps");
}

extern "C" int cfsd_mlp_train_steps(const float* z, const int32_t* label, const float* class_weight, float* params,
                                    float* m, float* v, int32_t* step, float* acc, void* workspace,
                                    size_t workspace_bytes, float* dw_out, const int* dims, int n_layers, int n_rows,
                                    int row0, int bs, int n_steps, int train, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, void* stream) {
  MlpDesc D;
  if (int rc = mlp_describe("mlp_train_steps", dims, n_layers, D)) return rc;
  if (bs < 1 || bs > kMlpMaxBs) return set_error(CFSD_EINVAL, "mlp_train_steps: batch %d (1..%d)", bs, kMlpMaxBs);
  if (n_steps < 0 || row0 < 0 || (long)row0 + (long)n_steps * bs > n_rows)
    return set_error(CFSD_EINVAL, "mlp_train_steps: rows [%d, +%d x %d) outside [0, %d)", row0, n_steps, bs, n_rows);
  if (!z || !label || !class_weight || !params || !acc || (train && (!m || !v || !step)))
    return set_error(CFSD_EINVAL, "mlp_train_steps: null pointer");
  const size_t need = (size_t)bs * mlp_dy_off(D, n_layers) * 4;
  if (train && (!workspace || workspace_bytes < need))
    return set_error(CFSD_EINVAL, "mlp_train_steps: workspace %zu < %zu bytes", workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
#define CFSD_MLP_STEPS(RB)                                                                                         \
  return mlp_steps_launch<RB>(D, z, label, class_weight, params, m, v, step, acc, (float*)workspace, dw_out, row0, \
                              bs, n_steps, train ? 1 : 0, lr, beta1, beta2, eps, weight_decay, st)
  switch (mlp_rows_tile(bs)) {
    case 4: CFSD_MLP_STEPS(4);
    case 8: CFSD_MLP_STEPS(8);
    default: CFSD_MLP_STEPS(16);
  }
#undef CFSD_MLP_STEPS
}

template <int RB>
static int mlp_head_launch(const MlpDesc& D, const float* z, const float* cw, float* params, float* m, float* v,
                           int32_t* step, float* acc, float* ws, float* dw_out, const MlpHead& H, int bs, int train,
                           float lr, float b1, float b2, float eps, float wd, hipStream_t st) {
  const size_t lds = (size_t)2 * RB * (train ? kMlpMaxWidth : D.maxw) * 4;
  // the limit is raised once per instantiation and device (to the train
  // step's size, the larger one: the attribute belongs to the current device's
  // function), so nothing but launches is issued when a step is recorded
  constexpr int kMaxDevices = 64;
  static bool raised[kMaxDevices] = {};
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return set_error(CFSD_EINVAL, "mlp_head_step: no current device");
  const bool known = device >= 0 && device < kMaxDevices;
  if (!known || !raised[device]) {
    if (int rc = mlp_raise_lds("mlp_head_step", (const void*)mlp_head_k<RB>, (size_t)2 * RB * kMlpMaxWidth * 4))
      return rc;
    if (known) raised[device] = true;
  }
  hipLaunchKernelGGL(mlp_head_k<RB>, dim3(1), dim3(kMlpStepThreads), lds, st, D, z, cw, params, ws, acc, step, bs,
                     train, H);
  if (train)
    hipLaunchKernelGGL(mlp_adam_k<true>, dim3((D.total + 255) / 256), dim3(256), 0, st, D, params, m, v, ws, step,
                       dw_out, bs, lr, b1, b2, eps, wd, H.w_cls);
  return launch_status("mlp_head_step");
}

extern "C" int cfsd_mlp_head_step(const float* z, int ld_z, int row_stride, const int32_t* batch_idx,
                                  const int32_t* label_table, int n_labels, const float* class_weight,
                                  float* params, float* m, float* v, int32_t* step, float* acc, void* workspace,
                                  size_t workspace_bytes, float* dw_out, float* dlat, int ld_dlat, float w_cls,
                                  const int* dims, int n_layers, int bs, int train, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, void* stream) {
  MlpDesc D;
  if (int rc = mlp_describe("mlp_head_step", dims, n_layers, D)) return rc;
  if (bs < 1 || bs > kMlpMaxBs) return set_error(CFSD_EINVAL, "mlp_head_step: batch %d (1..%d)", bs, kMlpMaxBs);
  if (row_stride < 1 || ld_z < D.dims[0] || n_labels < 1)
    return set_error(CFSD_EINVAL, "mlp_head_step: bad sizes row_stride=%d ld_z=%d (width %d) n_labels=%d",
                     row_stride, ld_z, D.dims[0], n_labels);
  if (!z || !batch_idx || !label_table || !class_weight || !params || !acc)
    return set_error(CFSD_EINVAL, "mlp_head_step: null pointer");
  if (train) {
    if (!step || !dlat || (!m != !v) || (!m && !dw_out))
      return set_error(CFSD_EINVAL, "mlp_head_step: a train step needs step, dlat and either m and v or dw_out");
    if (ld_dlat < D.dims[0]) return set_error(CFSD_EINVAL, "mlp_head_step: ld_dlat %d < width %d", ld_dlat, D.dims[0]);
    const size_t need = (size_t)bs * mlp_dy_off(D, n_layers) * 4;
    if (!workspace || workspace_bytes < need)
      return set_error(CFSD_EINVAL, "mlp_head_step: workspace %zu < %zu bytes", workspace_bytes, need);
  }
  MlpHead H;
  H.batch_idx = batch_idx;
  H.label_table = label_table;
  H.dlat = dlat;
  H.z_stride = (long)row_stride * ld_z;
  H.dlat_stride = (long)row_stride * ld_dlat;
  H.n_labels = n_labels;
  H.w_cls = w_cls;
  const hipStream_t st = (hipStream_t)stream;
#define CFSD_MLP_HEAD(RB)                                                                                       \
  return mlp_head_launch<RB>(D, z, class_weight, params, m, v, step, acc, (float*)workspace, dw_out, H, bs,     \
                             train ? 1 : 0, lr, beta1, beta2, eps, weight_decay, st)
  switch (mlp_rows_tile(bs)) {
    case 4: CFSD_MLP_HEAD(4);
    case 8: CFSD_MLP_HEAD(8);
    default: CFSD_MLP_HEAD(16);
  }
#undef CFSD_MLP_HEAD
}
