// The embedding figures (gfx950): batched Gaussian kernel density estimates,
// iso-level bands shaded into an image, and anti-aliased point / line /
// triangle overlays.
//
// Reference: Tester.plot_embeddings / plot_embeddings_per_region
// (test.py:1161-1321) call seaborn's kdeplot, which evaluates scipy's
// gaussian_kde on a 200 x 200 grid per class and hands matplotlib the iso-levels
// to fill; _render_embed_save_z_interpolations (test.py:750-833) and
// _project_pre_post_pair (test.py:1090-1136) scatter points and arrows on those
// figures.  Here the densities, the bands and the markers are drawn on the
// device.
//
// No atomics.  A grid node, a pixel of an image, belongs to one thread, which
// walks its points / layers / primitives in the order given: the same input
// gives the same bits.  Small descriptor tables (sets, panels, layers) are HOST
// arrays: the entry checks them and passes them to the kernel by value, a few
// per launch, so what the kernel indexes with is what was checked.  The
// primitive table can be long and lives on the device; its host copy is what is
// checked, and the kernel clamps every index it reads from the device copy.
#include <math.h>

#include "cfsd_common.h"

namespace cfsd {

constexpr int kFigThreads = 256;
constexpr int kKdeChunk = CFSD_KDE_CHUNK;
constexpr int kKdeSetsPerLaunch = 32;  // 32 x 8 doubles + 33 ints of kernel arguments
constexpr int kShadeMaxPanels = CFSD_SHADE_MAX_PANELS;
constexpr int kShadeMaxLevels = CFSD_SHADE_MAX_LEVELS;
constexpr int kShadeLayersPerLaunch = 12;  // 12 x 24 + 16 x 8 doubles of kernel arguments (< 4 KiB)
constexpr int kPanelDoubles = CFSD_SHADE_PANEL_DOUBLES;
constexpr int kLayerDoubles = CFSD_SHADE_LAYER_DOUBLES;
constexpr int kPrimRound = CFSD_PRIM_ROUND;
constexpr int kPrimFloats = CFSD_PRIM_FLOATS;
constexpr int kTileW = 32, kTileH = 8;  // pixels of one workgroup: rows of 128 B
constexpr float kCullSlack = 1.f / 64.f;  // pixels added to a primitive's cull box
static_assert(kPrimRound == kFigThreads, "a round stages one primitive per thread");
static_assert(kTileW * kTileH == kFigThreads, "one thread per pixel of a tile");
static_assert(kPanelDoubles == 8 && kLayerDoubles == 24 && kPrimFloats == 16, "table rows as laid out below");

// ---------------------------------------------------------------- kde2d
struct KdeSets {
  int32_t ptr[kKdeSetsPerLaunch + 1];
  double p[kKdeSetsPerLaunch][8];  // L00, L10, L11, scale, lo0, step0, lo1, step1
};

// One thread per grid node; the set's points pass through LDS kKdeChunk at a
// time and every thread adds them in point order.
__global__ __launch_bounds__(kFigThreads) void kde2d_k(const double* __restrict__ points, KdeSets sets,
                                                       double* __restrict__ density, int G) {
  __shared__ double pts[kKdeChunk][2];
  const int s = blockIdx.y;
  const int node = blockIdx.x * kFigThreads + threadIdx.x;
  const bool active = node < G * G;
  const int i = node / G, j = node - i * G;
  const double l00 = sets.p[s][0], l10 = sets.p[s][1], l11 = sets.p[s][2], scale = sets.p[s][3];
  double g0, g1;
  {
#pragma clang fp contract(off)
    g0 = sets.p[s][4] + (double)i * sets.p[s][5];
    g1 = sets.p[s][6] + (double)j * sets.p[s][7];
  }
  const int begin = sets.ptr[s], end = sets.ptr[s + 1];
  double acc = 0.0;
  for (int c0 = begin; c0 < end; c0 += kKdeChunk) {
    const int n = min(kKdeChunk, end - c0);
    __syncthreads();  // the previous chunk has been read
    for (int e = threadIdx.x; e < 2 * n; e += kFigThreads) (&pts[0][0])[e] = points[2 * (long)c0 + e];
    __syncthreads();
    if (active)
      for (int k = 0; k < n; ++k) {
        const double d0 = g0 - pts[k][0], d1 = g1 - pts[k][1];
        const double u0 = l00 * d0 + l10 * d1, u1 = l11 * d1;
        acc += exp(-0.5 * (u0 * u0 + u1 * u1));
      }
  }
  if (active) density[((long)s * G + i) * G + j] = scale * acc;
}

// ---------------------------------------------------------------- density_shade
struct ShadeArgs {
  double panel[kShadeMaxPanels][kPanelDoubles];       // px0, py0, pw, ph, xlo, xhi, ylo, yhi
  double layer[kShadeLayersPerLaunch][kLayerDoubles];  // see cfsd.h
};

// Band of the pixel (x, y) of panel P under layer L: float64, nothing fused, the
// operations in the order cfsd.h states (a host restatement gives the same bits).
__device__ __forceinline__ int band_at(const double* P, const double* L, const double* __restrict__ grids, int x,
                                       int y) {
#pragma clang fp contract(off)
  const double tx = ((double)x + 0.5 - P[0]) / P[2], ty = ((double)y + 0.5 - P[1]) / P[3];
  const double dx = P[4] + tx * (P[5] - P[4]), dy = P[7] - ty * (P[7] - P[6]);
  const int g0 = (int)L[2], g1 = (int)L[3];
  const double u = (dx - L[4]) / L[5], v = (dy - L[6]) / L[7];
  double d = 0.0;
  if (u >= 0.0 && u <= (double)(g0 - 1) && v >= 0.0 && v <= (double)(g1 - 1)) {
    const int i0 = min((int)u, g0 - 2), j0 = min((int)v, g1 - 2);
    const double fu = u - (double)i0, fv = v - (double)j0;
    const double* g = grids + (long)L[1] + (long)i0 * g1 + j0;
    const double a = g[0] * (1.0 - fu) + g[g1] * fu, b = g[1] * (1.0 - fu) + g[g1 + 1] * fu;
    d = a * (1.0 - fv) + b * fv;
  }
  const int K = (int)L[8];
  int band = 0;
  for (int k = 0; k < kShadeMaxLevels; ++k) band += (k < K && L[9 + k] <= d) ? 1 : 0;
  return band;
}

// Workgroup (tile of the panel's tile range, panel); a thread owns one pixel
// through every layer of the launch.
__global__ __launch_bounds__(kFigThreads) void density_shade_k(float* __restrict__ image,
                                                               const double* __restrict__ grids, ShadeArgs args,
                                                               int n_layers, int H, int W) {
#pragma clang fp contract(off)
  const int p = blockIdx.z;
  const double* P = args.panel[p];
  const int px0 = (int)P[0], py0 = (int)P[1], px1 = px0 + (int)P[2], py1 = py0 + (int)P[3];
  const int x = (px0 / kTileW + (int)blockIdx.x) * kTileW + (int)(threadIdx.x % kTileW);
  const int y = (py0 / kTileH + (int)blockIdx.y) * kTileH + (int)(threadIdx.x / kTileW);
  if (x < px0 || x >= px1 || y < py0 || y >= py1) return;  // (no barrier below)
  float* px = image + (long)y * W + x;
  const long plane = (long)H * W;
  float c[3] = {px[0], px[plane], px[2 * plane]};
  bool wrote = false;
  for (int l = 0; l < n_layers; ++l) {
    const double* L = args.layer[l];
    if ((int)L[0] != p) continue;  // (uniform over the workgroup)
    const int K = (int)L[8];
    const float rgb[3] = {(float)L[17], (float)L[18], (float)L[19]};
    const float a = (float)L[20];
    const int b = band_at(P, L, grids, x, y);
    if (L[21] != 0.0 && b >= 1) {
      const float t = K > 1 ? (float)min(b, K - 1) / (float)(K - 1) : 1.f;
      for (int q = 0; q < 3; ++q) {
        const float shade = (1.f - t) + rgb[q] * t;
        c[q] = c[q] * (1.f - a) + shade * a;
      }
      wrote = true;
    }
    if (L[22] != 0.0) {
      const bool edge = (x + 1 < px1 && band_at(P, L, grids, x + 1, y) != b) ||
                        (y + 1 < py1 && band_at(P, L, grids, x, y + 1) != b);
      if (edge) {
        for (int q = 0; q < 3; ++q) c[q] = c[q] * (1.f - a) + rgb[q] * a;
        wrote = true;
      }
    }
  }
  if (wrote) {
    px[0] = c[0];
    px[plane] = c[1];
    px[2 * plane] = c[2];
  }
}

// ---------------------------------------------------------------- draw_primitives
// Coverage of the pixel centre (x, y) by the primitive q (kPrimFloats floats:
// kind, x0, y0, x1, y1, x2, y2, r, red, green, blue, alpha, clip x0, y0, x1, y1).
__device__ __forceinline__ float coverage(const float* q, float x, float y) {
  const int kind = (int)q[0];
  const float r = q[7];
  if (kind == CFSD_PRIM_TRIANGLE) {
    const float ax = q[1], ay = q[2], bx = q[3], by = q[4], cx = q[5], cy = q[6];
    const float area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    if (!(area2 != 0.f)) return 0.f;
    const float s = area2 > 0.f ? -1.f : 1.f;  // positive outside
    const float e0 =
        s * ((bx - ax) * (y - ay) - (by - ay) * (x - ax)) / sqrtf((bx - ax) * (bx - ax) + (by - ay) * (by - ay));
    const float e1 =
        s * ((cx - bx) * (y - by) - (cy - by) * (x - bx)) / sqrtf((cx - bx) * (cx - bx) + (cy - by) * (cy - by));
    const float e2 =
        s * ((ax - cx) * (y - cy) - (ay - cy) * (x - cx)) / sqrtf((ax - cx) * (ax - cx) + (ay - cy) * (ay - cy));
    return fminf(fmaxf(0.5f - fmaxf(e0, fmaxf(e1, e2)), 0.f), 1.f);
  }
  float dx = x - q[1], dy = y - q[2];
  if (kind == CFSD_PRIM_SEGMENT) {
    const float bx = q[3] - q[1], by = q[4] - q[2];
    const float len2 = bx * bx + by * by;
    if (len2 > 0.f) {
      const float h = fminf(fmaxf((dx * bx + dy * by) / len2, 0.f), 1.f);
      dx -= bx * h;
      dy -= by * h;
    }
  }
  return fminf(fmaxf(r + 0.5f - sqrtf(dx * dx + dy * dy), 0.f), 1.f);
}

// Workgroup (tile x, tile y, image).  A round stages kPrimRound primitives of
// the image in LDS, one per thread, each culled against the tile; the pixels
// then walk the survivors in primitive order.
__global__ __launch_bounds__(kFigThreads) void draw_primitives_k(float* __restrict__ images,
                                                                 const float* __restrict__ prims,
                                                                 const int32_t* __restrict__ prim_ptr, int H, int W,
                                                                 int n_prims) {
  __shared__ float stage[kPrimRound][kPrimFloats];
  __shared__ unsigned long long live[kFigThreads / 64];
  const int t = threadIdx.x, img = blockIdx.z;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int x = tx0 + t % kTileW, y = ty0 + t / kTileW;
  const bool inside = x < W && y < H;
  const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
  const int begin = min(max(prim_ptr[img], 0), n_prims);
  const int end = min(max(prim_ptr[img + 1], begin), n_prims);
  const long plane = (long)H * W;
  float* px = images + (long)img * 3 * plane + (long)(inside ? y : 0) * W + (inside ? x : 0);
  float c[3] = {0.f, 0.f, 0.f};
  if (inside && begin < end) {
    c[0] = px[0];
    c[1] = px[plane];
    c[2] = px[2 * plane];
  }
  bool wrote = false;
  for (int r0 = begin; r0 < end; r0 += kPrimRound) {
    const int n = min(kPrimRound, end - r0);
    __syncthreads();  // the previous round has been walked
    bool keep = false;
    if (t < n) {
      const f32x4* src = reinterpret_cast<const f32x4*>(prims + (long)(r0 + t) * kPrimFloats);
      f32x4 v[4];
      for (int k = 0; k < 4; ++k) v[k] = src[k];
      for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4*>(&stage[t][4 * k]) = v[k];
      const int kind = (int)v[0].x;
      const float r = v[1].w;
      // bounding box of where the coverage is not 0, grown by kCullSlack for the rounding of the box itself
      float lox = v[0].y, hix = v[0].y, loy = v[0].z, hiy = v[0].z, pad = r + 0.5f + kCullSlack;
      if (kind == CFSD_PRIM_SEGMENT) {
        lox = fminf(lox, v[0].w), hix = fmaxf(hix, v[0].w), loy = fminf(loy, v[1].x), hiy = fmaxf(hiy, v[1].x);
      }
      if (kind == CFSD_PRIM_TRIANGLE) {
        // coverage > 0 is the triangle with every edge line moved out by 1/2: the triangle of the mitre points
        // m_i = p_i + (n_a + n_b) / (2 (1 + n_a . n_b)), n_a and n_b the outward unit normals of p_i's two edges
        // (a tip of interior angle t reaches 1 / (2 sin(t / 2)) past its vertex, not 1/2)
        const float px3[3] = {v[0].y, v[0].w, v[1].y}, py3[3] = {v[0].z, v[1].x, v[1].z};
        const float area2 = (px3[1] - px3[0]) * (py3[2] - py3[0]) - (py3[1] - py3[0]) * (px3[2] - px3[0]);
        const float sgn = area2 > 0.f ? 1.f : -1.f;
        float nx[3], ny[3];  // of the edge p_i -> p_(i+1)
        for (int i = 0; i < 3; ++i) {
          const float ex = px3[(i + 1) % 3] - px3[i], ey = py3[(i + 1) % 3] - py3[i];
          const float inv = sgn / sqrtf(ex * ex + ey * ey);
          nx[i] = ey * inv, ny[i] = -ex * inv;
        }
        bool open = !(area2 != 0.f);  // (a zero-area triangle draws nothing; its box does not matter)
        lox = loy = INFINITY, hix = hiy = -INFINITY;
        for (int i = 0; i < 3; ++i) {
          const int a = (i + 2) % 3;  // the edge that ends in p_i
          const float den = 1.f + nx[a] * nx[i] + ny[a] * ny[i];
          open = open || !(den > 1e-6f);  // a tip too thin to bound: never culled
          const float mx = px3[i] + 0.5f * (nx[a] + nx[i]) / den, my = py3[i] + 0.5f * (ny[a] + ny[i]) / den;
          lox = fminf(lox, mx), hix = fmaxf(hix, mx), loy = fminf(loy, my), hiy = fmaxf(hiy, my);
        }
        if (open || !(lox <= hix) || !(loy <= hiy)) lox = loy = -INFINITY, hix = hiy = INFINITY;
        pad = kCullSlack;
      }
      lox = fmaxf(lox - pad, v[3].x), hix = fminf(hix + pad, v[3].z);
      loy = fmaxf(loy - pad, v[3].y), hiy = fminf(hiy + pad, v[3].w);
      keep = lox <= (float)(tx0 + kTileW) && hix >= (float)tx0 && loy <= (float)(ty0 + kTileH) && hiy >= (float)ty0 &&
             v[2].w > 0.f;
    }
    const unsigned long long mask = __ballot(keep);
    if ((t & 63) == 0) live[t >> 6] = mask;
    __syncthreads();
    for (int w = 0; w < kFigThreads / 64; ++w) {
      unsigned long long m = live[w];  // (uniform over the workgroup)
      while (m) {
        const int k = w * 64 + __builtin_ctzll(m);
        m &= m - 1;
        const float* q = stage[k];
        if (!inside || fx < q[12] || fx > q[14] || fy < q[13] || fy > q[15]) continue;
        const float cov = coverage(q, fx, fy);
        if (!(cov > 0.f)) continue;
        const float wgt = q[11] * cov;
        for (int ch = 0; ch < 3; ++ch) c[ch] = c[ch] * (1.f - wgt) + q[8 + ch] * wgt;
        wrote = true;
      }
    }
  }
  if (wrote) {
    px[0] = c[0];
    px[plane] = c[1];
    px[2 * plane] = c[2];
  }
}

static bool integral(double v, double lo, double hi) { return v >= lo && v <= hi && v == floor(v); }

}  // namespace cfsd

using namespace cfsd;

extern "C" int cfsd_kde2d(const double* points, const int32_t* set_ptr, const double* params, double* density,
                          int n_points, int n_sets, int G, void* stream) {
  if (!set_ptr || !params || !density || (n_points > 0 && !points))
    return set_error(CFSD_EINVAL, "kde2d: null pointer");
  if (G < 2 || G > CFSD_KDE_MAX_G) return set_error(CFSD_EINVAL, "kde2d: G=%d (2..%d supported)", G, CFSD_KDE_MAX_G);
  if (n_sets < 1 || n_points < 0 || n_points >= (1 << 30))
    return set_error(CFSD_EINVAL, "kde2d: bad sizes n_points=%d n_sets=%d", n_points, n_sets);
  if ((long)n_sets * G * G >= (1L << 31)) return set_error(CFSD_EINVAL, "kde2d: n_sets x G x G >= 2^31");
  if (set_ptr[0] < 0 || set_ptr[n_sets] > n_points)
    return set_error(CFSD_EINVAL, "kde2d: set_ptr runs from %d to %d, outside [0, %d]", set_ptr[0], set_ptr[n_sets],
                     n_points);
  for (int s = 0; s < n_sets; ++s) {
    if (set_ptr[s + 1] < set_ptr[s])
      return set_error(CFSD_EINVAL, "kde2d: set_ptr decreases at set %d (%d > %d)", s, set_ptr[s], set_ptr[s + 1]);
    for (int q = 0; q < 8; ++q)
      if (!isfinite(params[s * 8 + q]))
        return set_error(CFSD_EINVAL, "kde2d: set %d: parameter %d is not finite", s, q);
    if (!(params[s * 8 + 5] > 0.0) || !(params[s * 8 + 7] > 0.0))
      return set_error(CFSD_EINVAL, "kde2d: set %d: the grid steps must be positive", s);
  }
  for (int s0 = 0; s0 < n_sets; s0 += kKdeSetsPerLaunch) {
    const int ns = n_sets - s0 < kKdeSetsPerLaunch ? n_sets - s0 : kKdeSetsPerLaunch;
    KdeSets sets;
    for (int s = 0; s < kKdeSetsPerLaunch; ++s) {
      const int src = s < ns ? s0 + s : s0 + ns - 1;
      sets.ptr[s] = set_ptr[src];
      for (int q = 0; q < 8; ++q) sets.p[s][q] = params[src * 8 + q];
    }
    for (int s = ns; s <= kKdeSetsPerLaunch; ++s) sets.ptr[s] = set_ptr[s0 + ns];
    hipLaunchKernelGGL(kde2d_k, dim3((unsigned)((G * G + kFigThreads - 1) / kFigThreads), (unsigned)ns),
                       dim3(kFigThreads), 0, (hipStream_t)stream, points, sets, density + (long)s0 * G * G, G);
    const int rc = launch_status("kde2d");
    if (rc) return rc;
  }
  return CFSD_OK;
}

extern "C" int cfsd_density_shade(float* image, const double* grids, const double* panels, const double* layers,
                                  int H, int W, int n_panels, int n_layers, int grid_doubles, void* stream) {
  if (!image || !grids || !panels || !layers) return set_error(CFSD_EINVAL, "density_shade: null pointer");
  if (H < 1 || W < 1 || H > CFSD_FIG_MAX_SIZE || W > CFSD_FIG_MAX_SIZE)
    return set_error(CFSD_EINVAL, "density_shade: image %d x %d (1..%d supported)", H, W, CFSD_FIG_MAX_SIZE);
  if (n_panels < 1 || n_panels > kShadeMaxPanels)
    return set_error(CFSD_EINVAL, "density_shade: %d panels (1..%d supported)", n_panels, kShadeMaxPanels);
  if (n_layers < 1 || n_layers > CFSD_SHADE_MAX_LAYERS || grid_doubles < 4)
    return set_error(CFSD_EINVAL, "density_shade: bad sizes n_layers=%d grid_doubles=%d", n_layers, grid_doubles);
  int tiles_x = 1, tiles_y = 1;
  for (int p = 0; p < n_panels; ++p) {
    const double* P = panels + p * kPanelDoubles;
    if (!integral(P[0], 0, W - 1) || !integral(P[1], 0, H - 1) || !integral(P[2], 1, W - P[0]) ||
        !integral(P[3], 1, H - P[1]))
      return set_error(CFSD_EINVAL, "density_shade: panel %d: rectangle outside the %d x %d image", p, H, W);
    for (int q = 4; q < 8; ++q)
      if (!isfinite(P[q])) return set_error(CFSD_EINVAL, "density_shade: panel %d: window is not finite", p);
    if (!(P[5] > P[4]) || !(P[7] > P[6])) return set_error(CFSD_EINVAL, "density_shade: panel %d: empty window", p);
    for (int o = 0; o < p; ++o) {
      const double* O = panels + o * kPanelDoubles;
      if (P[0] < O[0] + O[2] && O[0] < P[0] + P[2] && P[1] < O[1] + O[3] && O[1] < P[1] + P[3])
        return set_error(CFSD_EINVAL, "density_shade: panels %d and %d overlap", o, p);
    }
    const int x0 = (int)P[0], y0 = (int)P[1], x1 = x0 + (int)P[2], y1 = y0 + (int)P[3];
    tiles_x = max(tiles_x, (x1 - 1) / kTileW - x0 / kTileW + 1);
    tiles_y = max(tiles_y, (y1 - 1) / kTileH - y0 / kTileH + 1);
  }
  for (int l = 0; l < n_layers; ++l) {
    const double* L = layers + l * kLayerDoubles;
    if (!integral(L[0], 0, n_panels - 1)) return set_error(CFSD_EINVAL, "density_shade: layer %d: no such panel", l);
    if (!integral(L[8], 0, 1e9) || L[8] < 1 || L[8] > kShadeMaxLevels)
      return set_error(CFSD_EINVAL, "density_shade: layer %d: K=%g levels (1..%d supported)", l, L[8], kShadeMaxLevels);
    if (!integral(L[2], 2, CFSD_KDE_MAX_G) || !integral(L[3], 2, CFSD_KDE_MAX_G) || !integral(L[1], 0, grid_doubles) ||
        L[1] + L[2] * L[3] > grid_doubles)
      return set_error(CFSD_EINVAL, "density_shade: layer %d: grid outside the %d doubles given", l, grid_doubles);
    if (!isfinite(L[4]) || !isfinite(L[6]) || !isfinite(L[5]) || !isfinite(L[7]) || !(L[5] > 0.0) || !(L[7] > 0.0))
      return set_error(CFSD_EINVAL, "density_shade: layer %d: grid origin / step", l);
    for (int k = 0; k < (int)L[8]; ++k)
      if (!isfinite(L[9 + k]) || (k > 0 && L[9 + k] < L[8 + k]))
        return set_error(CFSD_EINVAL, "density_shade: layer %d: levels must be finite and ascending", l);
    for (int q = 17; q < 21; ++q)
      if (!(L[q] >= 0.0 && L[q] <= 1.0))
        return set_error(CFSD_EINVAL, "density_shade: layer %d: colour outside [0, 1]", l);
    if ((L[21] != 0.0 && L[21] != 1.0) || (L[22] != 0.0 && L[22] != 1.0))
      return set_error(CFSD_EINVAL, "density_shade: layer %d: flags must be 0 or 1", l);
  }
  ShadeArgs args;
  for (int p = 0; p < kShadeMaxPanels; ++p)
    for (int q = 0; q < kPanelDoubles; ++q) args.panel[p][q] = panels[(p < n_panels ? p : 0) * kPanelDoubles + q];
  for (int l0 = 0; l0 < n_layers; l0 += kShadeLayersPerLaunch) {
    const int nl = n_layers - l0 < kShadeLayersPerLaunch ? n_layers - l0 : kShadeLayersPerLaunch;
    for (int l = 0; l < kShadeLayersPerLaunch; ++l)
      for (int q = 0; q < kLayerDoubles; ++q) args.layer[l][q] = layers[(l0 + (l < nl ? l : 0)) * kLayerDoubles + q];
    hipLaunchKernelGGL(density_shade_k, dim3((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)n_panels),
                       dim3(kFigThreads), 0, (hipStream_t)stream, image, grids, args, nl, H, W);
    const int rc = launch_status("density_shade");
    if (rc) return rc;
  }
  return CFSD_OK;
}

extern "C" int cfsd_draw_primitives(float* images, const float* prims, const int32_t* prim_ptr,
                                    const float* prims_host, const int32_t* prim_ptr_host, int B, int H, int W,
                                    int n_prims, void* stream) {
  if (!images || !prim_ptr || !prim_ptr_host || (n_prims > 0 && (!prims || !prims_host)))
    return set_error(CFSD_EINVAL, "draw_primitives: null pointer");
  if (H < 1 || W < 1 || H > CFSD_FIG_MAX_SIZE || W > CFSD_FIG_MAX_SIZE)
    return set_error(CFSD_EINVAL, "draw_primitives: image %d x %d (1..%d supported)", H, W, CFSD_FIG_MAX_SIZE);
  if (B < 1 || B > 65535 || n_prims < 0 || n_prims > CFSD_PRIM_MAX)
    return set_error(CFSD_EINVAL, "draw_primitives: bad sizes B=%d n_prims=%d", B, n_prims);
  if ((long)B * 3 * H * W >= (1L << 31)) return set_error(CFSD_EINVAL, "draw_primitives: B x 3 x H x W >= 2^31");
  if (prim_ptr_host[0] < 0 || prim_ptr_host[B] > n_prims)
    return set_error(CFSD_EINVAL, "draw_primitives: prim_ptr runs from %d to %d, outside [0, %d]", prim_ptr_host[0],
                     prim_ptr_host[B], n_prims);
  for (int b = 0; b < B; ++b)
    if (prim_ptr_host[b + 1] < prim_ptr_host[b])
      return set_error(CFSD_EINVAL, "draw_primitives: prim_ptr decreases at image %d", b);
  for (int k = 0; k < n_prims; ++k) {
    const float* q = prims_host + (long)k * kPrimFloats;
    if (q[0] != CFSD_PRIM_DISC && q[0] != CFSD_PRIM_SEGMENT && q[0] != CFSD_PRIM_TRIANGLE)
      return set_error(CFSD_EINVAL, "draw_primitives: primitive %d: unknown kind %g", k, (double)q[0]);
    for (int j = 1; j < 8; ++j)
      if (!isfinite(q[j])) return set_error(CFSD_EINVAL, "draw_primitives: primitive %d: geometry is not finite", k);
    if (q[7] < 0.f) return set_error(CFSD_EINVAL, "draw_primitives: primitive %d: negative radius", k);
    for (int j = 8; j < 12; ++j)
      if (!(q[j] >= 0.f && q[j] <= 1.f))
        return set_error(CFSD_EINVAL, "draw_primitives: primitive %d: colour outside [0, 1]", k);
    if (!integral(q[12], 0, W) || !integral(q[14], q[12], W) || !integral(q[13], 0, H) || !integral(q[15], q[13], H))
      return set_error(CFSD_EINVAL, "draw_primitives: primitive %d: clip rectangle outside the %d x %d image", k, H, W);
  }
  hipLaunchKernelGGL(draw_primitives_k,
                     dim3((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)B),
                     dim3(kFigThreads), 0, (hipStream_t)stream, images, prims, prim_ptr, H, W, n_prims);
  return launch_status("draw_primitives");
}
