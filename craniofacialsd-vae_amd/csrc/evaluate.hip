// Evaluation of a trained model (gfx950): the two device reductions of a
// latent traversal (Tester.latent_traversals, test.py:128-229).
//
// Reference: per latent variable the reference decodes n_steps heads, expands
// the first one to the batch, calls compute_vertex_errors
// (model_manager.py:395-400) on the pair (test.py:157-158) and, for the plot,
// averages the last step's distances over each feature region's vertex list
// through fancy indexing and pandas on the host (test.py:208-215).
//
// Here both stay on the device.  group_vertex_errors_k is vertex_errors_k
// (pool_swap.hip) with the ground truth read in place from frame 0 of the
// thread's own group: the same operations in the same order, so the result is
// bit-equal to cfsd_vertex_errors on an expanded copy that is never made.
// region_means_k is one 256-thread workgroup per (row, region): a strided
// partial sum per thread, a fixed LDS tree, one division.  Plain fp32, no
// atomics; neither result depends on the launch geometry or on the other rows
// of the call.
#include <math.h>

#include "cfsd_common.h"

namespace cfsd {

// One thread per (frame, vertex).  total = groups * n * nv; total * 3 < 2^31
// (checked at the ABI), so every index fits an int.
__global__ void group_vertex_errors_k(const float* __restrict__ frames, const float* __restrict__ mean,
                                      const float* __restrict__ std, float* __restrict__ err, int n, int nv,
                                      long total, float to_mm) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int frame = (int)(t / nv);
  const int v = (int)(t - (long)frame * nv);
  const long t0 = (long)(frame - frame % n) * nv + v;  // the same vertex of the group's frame 0
  float a[3], g[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a[q] = frames[t * 3 + q];
    g[q] = frames[t0 * 3 + q];
  }
  if (mean) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float s = std[v * 3 + q], m = mean[v * 3 + q];
      a[q] = a[q] * s + m;
      g[q] = g[q] * s + m;
    }
  }
  const float d0 = a[0] - g[0], d1 = a[1] - g[1], d2 = a[2] - g[2];
  err[t] = sqrtf(d0 * d0 + d1 * d1 + d2 * d2) * to_mm;
}

constexpr int kRmMaxRegions = CFSD_RM_MAX_REGIONS;
constexpr int kRmThreads = CFSD_RM_THREADS;

// The CSR's row pointer travels by value: the entry point has checked it.
struct RegionPtr {
  int32_t p[kRmMaxRegions + 1];
};

// Workgroup w = row * n_regions + region.  Thread t adds the list entries t,
// t + 256, ... in ascending order (ceil(len / 256) additions at the most, the
// first onto 0), the 256 partials meet in a halving tree (8 additions), the
// total is divided by len.
__global__ void __launch_bounds__(kRmThreads) region_means_k(const float* __restrict__ values, RegionPtr rp,
                                                             const int32_t* __restrict__ idx,
                                                             float* __restrict__ out, int nv, int n_regions) {
  __shared__ float part[kRmThreads];
  const int b = (int)(blockIdx.x / (unsigned)n_regions);
  const int r = (int)(blockIdx.x - (unsigned)b * (unsigned)n_regions);
  const int start = rp.p[r];
  const int len = rp.p[r + 1] - start;
  const float* row = values + (long)b * nv;
  const int32_t* list = idx + start;
  float acc = 0.f;
  for (int j = threadIdx.x; j < len; j += kRmThreads) acc += row[list[j]];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kRmThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = part[0] / (float)len;
}

}  // namespace cfsd

using namespace cfsd;

extern "C" int cfsd_group_vertex_errors(const float* frames, const float* mean, const float* std, float* err,
                                        int groups, int n, int nv, float to_mm, void* stream) {
  if (!frames || !err) return set_error(CFSD_EINVAL, "group_vertex_errors: null pointer");
  if (!mean != !std) return set_error(CFSD_EINVAL, "group_vertex_errors: mean and std go together");
  if (groups <= 0 || n <= 0 || nv <= 0)
    return set_error(CFSD_EINVAL, "group_vertex_errors: bad sizes (groups=%d n=%d nv=%d)", groups, n, nv);
  const long total = (long)groups * n * nv;
  if ((long)groups * n >= (1L << 31) || total * 3 >= (1L << 31))
    return set_error(CFSD_EINVAL, "group_vertex_errors: groups x n x nv x 3 >= 2^31");
  hipLaunchKernelGGL(group_vertex_errors_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, frames, mean, std, err, n, nv, total, to_mm);
  return launch_status("group_vertex_errors");
}

extern "C" int cfsd_region_means(const float* values, const int32_t* region_ptr, const int32_t* region_idx,
                                 float* out, int rows, int nv, int n_regions, void* stream) {
  if (!values || !region_ptr || !region_idx || !out) return set_error(CFSD_EINVAL, "region_means: null pointer");
  if (rows <= 0 || nv <= 0 || n_regions <= 0)
    return set_error(CFSD_EINVAL, "region_means: bad sizes (rows=%d nv=%d n_regions=%d)", rows, nv, n_regions);
  if (n_regions > kRmMaxRegions)
    return set_error(CFSD_EINVAL, "region_means: %d regions, at most %d", n_regions, kRmMaxRegions);
  if ((long)rows * nv >= (1L << 31) || (long)rows * n_regions >= (1L << 31))
    return set_error(CFSD_EINVAL, "region_means: rows x nv or rows x n_regions >= 2^31");
  RegionPtr rp;
  if (region_ptr[0] != 0) return set_error(CFSD_EINVAL, "region_means: region_ptr[0]=%d, expected 0", region_ptr[0]);
  for (int r = 0; r < n_regions; ++r) {
    if (region_ptr[r + 1] < region_ptr[r])
      return set_error(CFSD_EINVAL, "region_means: region_ptr decreases at region %d", r);
    if (region_ptr[r + 1] == region_ptr[r]) return set_error(CFSD_EINVAL, "region_means: region %d is empty", r);
  }
  for (int r = 0; r <= n_regions; ++r) rp.p[r] = region_ptr[r];
  for (int r = n_regions + 1; r <= kRmMaxRegions; ++r) rp.p[r] = region_ptr[n_regions];
  hipLaunchKernelGGL(region_means_k, dim3((unsigned)rows * (unsigned)n_regions), dim3(kRmThreads), 0,
                     (hipStream_t)stream, values, rp, region_idx, out, nv, n_regions);
  return launch_status("region_means");
}
