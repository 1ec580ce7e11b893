// Surgical planning in latent space (gfx950): the crossings of a patient's
// path to the healthy distribution, the latent tables of the planned
// procedures and the raw quantities of the pre- / post-operative metrics.
//
// Reference: Tester.interpolate_syndrome_to_normal (test.py:652-748) evaluates
// scipy's multivariate_normal.logpdf on every one of the 5000 points of a
// torch.linspace from the patient to the healthy mean and takes the first
// point inside the 3, 2 and 1 sigma shells; evaluate_pre_post_pair
// (test.py:972-1088) calls scipy.spatial.distance per pair and region.
//
// Here the crossing comes from a closed form: the grid runs along the segment
// from z to the mean, on which the Mahalanobis distance to the mean shrinks
// linearly, maha(i) = maha (1 - i / (steps - 1)), so the first point within
// `level` is i0 = ceil((steps - 1)(1 - level / maha)).  The grid itself is
// fp32 (torch.linspace's two-sided formula), so the ACTUAL grid points i0 - 1,
// i0, i0 + 1 are evaluated and the lowest one inside the level wins.
//
// One 128-thread workgroup per row (patient; patient x group; pair x window).
// Operands are fp32, every product and sum is float64: thread k owns column k
// of the whitened vector (ascending j), the squared norms meet in a fixed
// halving tree over 128 slots.  No atomics; a row's result depends on nothing
// but that row, and two calls give the same bits.
#include <math.h>

#include "cfsd_common.h"

namespace cfsd {

constexpr int kPlanThreads = CFSD_CLS_MAX_D;  // one thread per column of the widest window
constexpr int kPlanMaxLevels = CFSD_PLAN_MAX_LEVELS;
constexpr int kPlanMaxWindows = CFSD_PLAN_MAX_WINDOWS;
static_assert(kPlanThreads == 128, "the reduction tree below is written for 128 slots");

struct PlanLevels {
  float v[kPlanMaxLevels];
};

struct PairWindows {
  int32_t w[kPlanMaxWindows][4];  // col0, d, mean offset, whiten offset
};

// Point i of torch.linspace(s, e, steps) (RangeFactories.cpp: the step in the
// tensor's type, the first half counted from s, the second back from e).
// steps - 1 and i are below 2^24: their conversions are exact.
__device__ __forceinline__ float grid_point(float s, float e, int i, int steps) {
#pragma clang fp contract(off)
  const float step = (e - s) / (float)(steps - 1);
  return i < steps / 2 ? s + step * (float)i : e - step * (float)(steps - 1 - i);
}

// Sum of the 128 slots of `part` (every thread has written its own), the same
// tree for every call: part[t] += part[t + w], w = 64, ..., 1.  Ends with a
// barrier after which part may be written again.
__device__ __forceinline__ double tree_sum(double* part) {
  __syncthreads();
  for (int w = kPlanThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  const double s = part[0];
  __syncthreads();
  return s;
}

// |x W|^2 of the d-vector x (LDS, float64) under W [d, d] (global, fp32).
__device__ __forceinline__ double maha2_of(const double* x, const float* __restrict__ W, int d, double* part) {
  const int k = threadIdx.x;
  double y = 0.0;
  if (k < d)
    for (int j = 0; j < d; ++j) y += x[j] * (double)W[(long)j * d + k];
  part[k] = y * y;
  return tree_sum(part);
}

__global__ __launch_bounds__(kPlanThreads) void plan_targets_k(const float* __restrict__ z,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ whiten, PlanLevels levels,
                                                               float* __restrict__ maha, int32_t* __restrict__ index,
                                                               float* __restrict__ targets, int ld, int col0, int d,
                                                               int S, int steps) {
  __shared__ double x[kPlanThreads];
  __shared__ double part[kPlanThreads];
  const long p = blockIdx.x;
  const int j = threadIdx.x;
  const bool own = j < d;
  const float s = own ? z[p * ld + col0 + j] : 0.f;
  const float e = own ? mean[j] : 0.f;
  x[j] = (double)s - (double)e;
  __syncthreads();
  const double m0 = sqrt(maha2_of(x, whiten, d, part));
  if (j == 0) maha[p] = (float)m0;
  float* trow = targets + p * (long)(S + 1) * d;
  for (int k = 0; k < S; ++k) {
    const double level = (double)levels.v[k];
    // m0 == 0 gives -inf, a patient inside the level a value <= 0: both clamp to 0
    const double c = ceil((double)(steps - 1) * (1.0 - level / m0));
    const int i0 = c > 0.0 ? (c < (double)(steps - 1) ? (int)c : steps - 1) : 0;
    int found = min(i0 + 1, steps - 1);  // (the last grid point is the mean: always inside)
    for (int t = 1; t >= -1; --t) {      // i0 + 1, i0, i0 - 1: the lowest one inside wins
      const int i = i0 + t;
      if (i < 0 || i > steps - 1) continue;  // (uniform over the workgroup)
      x[j] = own ? (double)grid_point(s, e, i, steps) - (double)e : 0.0;
      __syncthreads();
      const double m2 = maha2_of(x, whiten, d, part);
      if (m2 <= level * level) found = i;
    }
    if (j == 0) index[p * S + k] = found;
    if (own) trow[(long)k * d + j] = grid_point(s, e, found, steps);
  }
  if (own) trow[(long)S * d + j] = e;
}

// Workgroup (patient, group); thread j owns column j of all F rows.
__global__ __launch_bounds__(kPlanThreads) void plan_tables_k(const float* __restrict__ z,
                                                              const float* __restrict__ targets,
                                                              const uint8_t* __restrict__ mask,
                                                              float* __restrict__ tables, float* __restrict__ dist,
                                                              int L, int S, int P, int n_first) {
  __shared__ double part[kPlanThreads];
  const int G = 1 + P, F = n_first + S;
  const long p = blockIdx.x / (unsigned)G;
  const int g = (int)(blockIdx.x - (unsigned long)p * G);
  const int j = threadIdx.x;
  const bool own = j < L;
  const bool moved = own && (g == 0 || mask[(long)(g - 1) * L + j] != 0);
  const float* trow = targets + p * (long)(S + 1) * L;
  const float zj = own ? z[p * L + j] : 0.f;
  const float t0 = own ? trow[j] : 0.f;
  const float healthy = own ? trow[(long)S * L + j] : 0.f;
  float* out = tables + ((long)p * G + g) * F * L;
  float last = zj;  // row n_first - 1
  for (int r = 0; r < n_first; ++r) {
    last = moved && n_first > 1 ? grid_point(zj, t0, r, n_first) : zj;  // (linspace of one step is its start)
    if (own) out[(long)r * L + j] = last;
  }
  for (int t = 0; t <= S; ++t) {
    float v = last;
    if (t > 0) {
      v = moved ? trow[(long)t * L + j] : zj;
      if (own) out[(long)(n_first - 1 + t) * L + j] = v;
    }
    const double diff = own ? (double)v - (double)healthy : 0.0;
    part[j] = diff * diff;
    const double sum = tree_sum(part);
    if (j == 0) dist[((long)p * G + g) * (S + 1) + t] = (float)(sum / (double)L);
  }
}

// Workgroup (pair, window).
__global__ __launch_bounds__(kPlanThreads) void pair_metrics_k(const float* __restrict__ z_pre,
                                                               const float* __restrict__ z_post, PairWindows win,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ whiten,
                                                               float* __restrict__ raw, int L, int W) {
  __shared__ double xa[kPlanThreads], xb[kPlanThreads], xd[kPlanThreads];
  __shared__ double part[kPlanThreads];
  const long p = blockIdx.x / (unsigned)W;
  const int w = (int)(blockIdx.x - (unsigned long)p * W);
  const int col0 = win.w[w][0], d = win.w[w][1];
  const float* mu = mean + win.w[w][2];
  const float* Wh = whiten + win.w[w][3];
  const int j = threadIdx.x;
  const bool own = j < d;
  const double a = own ? (double)z_pre[p * L + col0 + j] : 0.0;
  const double b = own ? (double)z_post[p * L + col0 + j] : 0.0;
  const double m = own ? (double)mu[j] : 0.0;
  const double da = a - m, db = b - m, dd = b - a;  // (exact: differences of fp32 values)
  xa[j] = da;
  xb[j] = db;
  xd[j] = dd;
  __syncthreads();
  double ya = 0.0, yb = 0.0, yd = 0.0;
  if (own)
    for (int i = 0; i < d; ++i) {
      const double wv = (double)Wh[(long)i * d + j];
      ya += xa[i] * wv;
      yb += xb[i] * wv;
      yd += xd[i] * wv;
    }
  double sums[7];
  const double terms[7] = {ya * ya, yb * yb, da * da, db * db, dd * -da, yd * yd, dd * dd};
  for (int q = 0; q < 7; ++q) {
    part[j] = terms[q];
    sums[q] = tree_sum(part);
  }
  if (j == 0) {
    float* o = raw + ((long)p * W + w) * 6;
    o[0] = (float)sqrt(sums[0]);
    o[1] = (float)sqrt(sums[1]);
    o[2] = (float)sqrt(sums[2]);
    o[3] = (float)sqrt(sums[3]);
    // (post - pre) . (mean - pre) over the two lengths: 0 / 0 = NaN for a zero vector, as numpy gives
    o[4] = (float)(sums[4] / (sqrt(sums[6]) * sqrt(sums[2])));
    o[5] = (float)sqrt(sums[5]);
  }
}

}  // namespace cfsd

using namespace cfsd;

extern "C" int cfsd_plan_targets(const float* z, const float* mean, const float* whiten, const float* levels,
                                 float* maha, int32_t* index, float* targets, int n, int ld, int col0, int d,
                                 int n_levels, int steps, void* stream) {
  if (!z || !mean || !whiten || !levels || !maha || !index || !targets)
    return set_error(CFSD_EINVAL, "plan_targets: null pointer");
  if (d < 1 || d > kPlanThreads) return set_error(CFSD_EINVAL, "plan_targets: d=%d (1..%d supported)", d, kPlanThreads);
  if (n < 1 || col0 < 0 || ld < col0 + d)
    return set_error(CFSD_EINVAL, "plan_targets: bad sizes n=%d ld=%d col0=%d d=%d", n, ld, col0, d);
  if (n_levels < 1 || n_levels > kPlanMaxLevels)
    return set_error(CFSD_EINVAL, "plan_targets: %d levels (1..%d supported)", n_levels, kPlanMaxLevels);
  if (steps < 2 || steps > CFSD_PLAN_MAX_STEPS)
    return set_error(CFSD_EINVAL, "plan_targets: steps=%d (2..%d supported)", steps, CFSD_PLAN_MAX_STEPS);
  if ((long)n * ld >= (1L << 31) || (long)n * (n_levels + 1) * d >= (1L << 31))
    return set_error(CFSD_EINVAL, "plan_targets: n x ld or n x (levels + 1) x d >= 2^31");
  PlanLevels lv;
  for (int k = 0; k < kPlanMaxLevels; ++k) lv.v[k] = 0.f;
  for (int k = 0; k < n_levels; ++k) {
    const float v = levels[k];
    if (!(v > 0.f) || !isfinite(v) || (k > 0 && !(v < levels[k - 1])))
      return set_error(CFSD_EINVAL, "plan_targets: levels must be positive, finite and descending (level %d = %g)", k,
                       (double)v);
    lv.v[k] = v;
  }
  hipLaunchKernelGGL(plan_targets_k, dim3((unsigned)n), dim3(kPlanThreads), 0, (hipStream_t)stream, z, mean, whiten,
                     lv, maha, index, targets, ld, col0, d, n_levels, steps);
  return launch_status("plan_targets");
}

extern "C" int cfsd_plan_tables(const float* z, const float* targets, const uint8_t* mask, float* tables,
                                float* dist, int n, int latent, int n_levels, int n_procedures, int n_first,
                                void* stream) {
  if (!z || !targets || !tables || !dist || (n_procedures > 0 && !mask))
    return set_error(CFSD_EINVAL, "plan_tables: null pointer");
  if (latent < 1 || latent > kPlanThreads)
    return set_error(CFSD_EINVAL, "plan_tables: latent=%d (1..%d supported)", latent, kPlanThreads);
  if (n < 1 || n_procedures < 0) return set_error(CFSD_EINVAL, "plan_tables: bad sizes n=%d procedures=%d", n, n_procedures);
  if (n_levels < 1 || n_levels > kPlanMaxLevels)
    return set_error(CFSD_EINVAL, "plan_tables: %d levels (1..%d supported)", n_levels, kPlanMaxLevels);
  if (n_first < 1 || n_first > CFSD_PLAN_MAX_FIRST)
    return set_error(CFSD_EINVAL, "plan_tables: n_first=%d (1..%d supported)", n_first, CFSD_PLAN_MAX_FIRST);
  const long groups = (long)n * (1 + (long)n_procedures);
  if (groups >= (1L << 31) || groups * (n_first + n_levels) * latent >= (1L << 31) ||
      ((long)n_procedures + 1) * latent >= (1L << 31))
    return set_error(CFSD_EINVAL, "plan_tables: n x (1 + procedures) x frames x latent >= 2^31");
  hipLaunchKernelGGL(plan_tables_k, dim3((unsigned)groups), dim3(kPlanThreads), 0, (hipStream_t)stream, z, targets,
                     mask, tables, dist, latent, n_levels, n_procedures, n_first);
  return launch_status("plan_tables");
}

extern "C" int cfsd_pair_metrics(const float* z_pre, const float* z_post, const int32_t* windows, const float* mean,
                                 const float* whiten, float* raw, int n, int latent, int n_windows, int mean_floats,
                                 int whiten_floats, void* stream) {
  if (!z_pre || !z_post || !windows || !mean || !whiten || !raw)
    return set_error(CFSD_EINVAL, "pair_metrics: null pointer");
  if (n < 1 || latent < 1 || mean_floats < 1 || whiten_floats < 1)
    return set_error(CFSD_EINVAL, "pair_metrics: bad sizes n=%d latent=%d mean=%d whiten=%d", n, latent, mean_floats,
                     whiten_floats);
  if (n_windows < 1 || n_windows > kPlanMaxWindows)
    return set_error(CFSD_EINVAL, "pair_metrics: %d windows (1..%d supported)", n_windows, kPlanMaxWindows);
  if ((long)n * latent >= (1L << 31) || (long)n * n_windows * 6 >= (1L << 31))
    return set_error(CFSD_EINVAL, "pair_metrics: n x latent or n x windows x 6 >= 2^31");
  PairWindows pw;
  for (int w = 0; w < kPlanMaxWindows; ++w) {
    const bool in = w < n_windows;
    for (int q = 0; q < 4; ++q) pw.w[w][q] = in ? windows[w * 4 + q] : (q == 1 ? 1 : 0);
    if (!in) continue;
    const long col0 = pw.w[w][0], d = pw.w[w][1], mo = pw.w[w][2], wo = pw.w[w][3];
    if (d < 1 || d > kPlanThreads || col0 < 0 || col0 + d > latent)
      return set_error(CFSD_EINVAL, "pair_metrics: window %d: columns [%ld, %ld) outside [0, %d) or wider than %d", w,
                       col0, col0 + d, latent, kPlanThreads);
    if (mo < 0 || mo + d > mean_floats || wo < 0 || wo + d * d > whiten_floats)
      return set_error(CFSD_EINVAL, "pair_metrics: window %d: offsets %ld / %ld past the packed mean (%d) or whiten (%d)",
                       w, mo, wo, mean_floats, whiten_floats);
  }
  hipLaunchKernelGGL(pair_metrics_k, dim3((unsigned)((long)n * n_windows)), dim3(kPlanThreads), 0, (hipStream_t)stream,
                     z_pre, z_post, pw, mean, whiten, raw, latent, n_windows);
  return launch_status("pair_metrics");
}
