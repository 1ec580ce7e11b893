// Mesh rendering (gfx950): a deterministic z-buffer rasteriser with per-vertex
// (Gouraud) shading, the pictures of ModelManager.render / log_images
// (model_manager.py:594-658), which the reference draws with pytorch3d's
// rasteriser (no ROCm build).  The convention is DESIGN.md section 9; in short:
//
//   camera    X_view = X R + T (row vectors), x_ndc = s x_view / z_view, NDC +X
//             left and +Y up, pixel (i, j) of an S x S image has its centre at
//             x = 1 - (2j + 1) / S, y = 1 - (2i + 1) / S;
//   coverage  the three edge functions at the pixel centre have the sign of
//             the area OR ARE ZERO (inclusive edges: no crack between two faces
//             sharing an edge); no back-face culling; a zero-area face covers
//             nothing; a face with a vertex at z_view <= znear is dropped whole;
//   depth     perspective-correct barycentrics w_i' = (w_i / z_i) / sum_k (w_k / z_k),
//             z = 1 / sum_k (w_k / z_k); the nearest z wins, equal bits: the
//             lowest face.
//
// Three stages.  rn_vertices_k: one thread per (mesh, vertex) projects it and,
// for Gouraud shading, sums the normals of its incident faces (a vertex ->
// faces CSR, ascending, so the sum's bits are fixed) and lights it in world
// space.  rn_setup_k: one thread per (mesh, group of kRnGroup consecutive
// faces) writes a 48-byte record per face (the projected corners, 1 / z, 1 /
// area, the pixel bounding box) and the group's bounding box.  rn_raster_k: a
// workgroup owns an 8 x 8 pixel tile of one mesh, one pixel per lane of EVERY
// wave; its kRnWaves waves share the face list, wave w taking the groups g = w
// (mod kRnWaves), so that a run of consecutive groups piled on one tile (an
// ear, a nostril: a thousand faces on 64 pixels) is spread over all of them,
// and the per-wave winners are merged by (z, face) in LDS.  A wave tests 64
// group boxes at a time, one per lane, against the tile; a ballot names the
// groups to enter.  The 64 records of four entered groups are then loaded at
// once, one per lane (one memory latency per four groups), a second ballot
// over their boxes names the faces, and only those are evaluated, each record
// broadcast from its lane's registers (v_readlane), so no load stands between
// two faces.  A wave meets its faces in ascending order and a strict '<' keeps
// the first among equal depths; between waves the merge compares (z, face):
// the result is a pure function of the inputs in any order.  No atomics.  One
// instruction sequence per (pixel, face), contraction pinned: a mesh gives the
// same bits alone or in a batch.
#include <math.h>

#include "cfsd_common.h"

namespace cfsd {

constexpr int kRnGroup = CFSD_RN_GROUP;  // faces per group box
constexpr int kRnRec = 12;               // floats per face record
constexpr int kRnTile = 8;               // pixels per tile side: one pixel per lane of a wave
constexpr int kRnWaves = 8;              // waves per workgroup: each takes every kRnWaves-th group of the tile's walk
constexpr int kRnMaxSize = CFSD_RN_MAX_SIZE;
constexpr int kRnNone = 0xffff;          // lower bound of an empty pixel box (lo > every pixel, hi = 0)

typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float rn_dot(float x0, float y0, float z0, float x1, float y1, float z1) {
#pragma clang fp contract(off)
  return x0 * x1 + y0 * y1 + z0 * z1;
}

// v / |v|, or 0 for a zero (or non-finite-length) vector.
__device__ __forceinline__ void rn_normalize(float& x, float& y, float& z) {
#pragma clang fp contract(off)
  const float l = sqrtf(rn_dot(x, y, z, x, y, z));
  const float inv = l > 0.f ? 1.f / l : 0.f;
  x *= inv;
  y *= inv;
  z *= inv;
}

// Area-weighted normal of vertex v: the normalised sum, in ascending face
// order, of cross(v1 - v0, v2 - v0) over the faces vf_idx[vf_ptr[v] .. vf_ptr[v + 1]).
__device__ __forceinline__ void rn_vertex_normal(const float* __restrict__ vb, const int* __restrict__ faces,
                                                 const int* __restrict__ vf_ptr, const int* __restrict__ vf_idx,
                                                 int v, int nv, int nf, float& nx, float& ny, float& nz) {
#pragma clang fp contract(off)
  const int m = 3 * nf;
  const int e0 = min(max(vf_ptr[v], 0), m), e1 = min(max(vf_ptr[v + 1], 0), m);
  nx = ny = nz = 0.f;
  for (int e = e0; e < e1; ++e) {
    const int* fi = faces + (long)min(max(vf_idx[e], 0), nf - 1) * 3;
    float c[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) ld_row<3>(vb + (long)min(max(fi[j], 0), nv - 1) * 3, c + 3 * j);
    const float ux = c[3] - c[0], uy = c[4] - c[1], uz = c[5] - c[2];
    const float wx = c[6] - c[0], wy = c[7] - c[1], wz = c[8] - c[2];
    nx += uy * wz - uz * wy;
    ny += uz * wx - ux * wz;
    nz += ux * wy - uy * wx;
  }
  rn_normalize(nx, ny, nz);
}

__global__ __launch_bounds__(256) void rn_normals_k(const float* __restrict__ verts, const int* __restrict__ faces,
                                                    const int* __restrict__ vf_ptr, const int* __restrict__ vf_idx,
                                                    float* __restrict__ normals, int nv, int nf, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int b, v;
  divmod32(t, nv, b, v);
  float n[3];
  rn_vertex_normal(verts + (long)b * nv * 3, faces, vf_ptr, vf_idx, v, nv, nf, n[0], n[1], n[2]);
  st_row<3>(normals + t * 3, n);
}

struct RnLight {
  float lx, ly, lz, ambient, diffuse, specular, shininess, tex_value;
};

// One thread per (mesh, vertex): NDC xy and view z; with `colors` also the
// Gouraud colour (HardGouraudShader: point light, Phong terms per vertex in
// world space).
__global__ __launch_bounds__(256) void rn_vertices_k(const float* __restrict__ verts, const float* __restrict__ cam,
                                                     const int* __restrict__ faces, const int* __restrict__ vf_ptr,
                                                     const int* __restrict__ vf_idx, const float* __restrict__ tex,
                                                     float* __restrict__ ndc, float* __restrict__ vz,
                                                     float* __restrict__ colors, RnLight lt, int nv, int nf,
                                                     long tex_bs, long total) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int b, v;
  divmod32(t, nv, b, v);
  const float* vb = verts + (long)b * nv * 3;
  float p[3];
  ld_row<3>(vb + (long)v * 3, p);
  float r[9], tr[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = cam[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tr[k] = cam[9 + k];
  const float s = cam[12];
  const float xv = p[0] * r[0] + p[1] * r[3] + p[2] * r[6] + tr[0];
  const float yv = p[0] * r[1] + p[1] * r[4] + p[2] * r[7] + tr[1];
  const float zv = p[0] * r[2] + p[1] * r[5] + p[2] * r[8] + tr[2];
  ndc[t * 2] = s * xv / zv;
  ndc[t * 2 + 1] = s * yv / zv;
  vz[t] = zv;
  if (!colors) return;
  float nx, ny, nz;
  rn_vertex_normal(vb, faces, vf_ptr, vf_idx, v, nv, nf, nx, ny, nz);
  // camera centre C = -T R^T
  const float cx = -(tr[0] * r[0] + tr[1] * r[1] + tr[2] * r[2]);
  const float cy = -(tr[0] * r[3] + tr[1] * r[4] + tr[2] * r[5]);
  const float cz = -(tr[0] * r[6] + tr[1] * r[7] + tr[2] * r[8]);
  float lx = lt.lx - p[0], ly = lt.ly - p[1], lz = lt.lz - p[2];
  float ex = cx - p[0], ey = cy - p[1], ez = cz - p[2];
  rn_normalize(lx, ly, lz);
  rn_normalize(ex, ey, ez);
  const float nl = rn_dot(nx, ny, nz, lx, ly, lz);
  const float d = fmaxf(nl, 0.f);
  const float rx = 2.f * nl * nx - lx, ry = 2.f * nl * ny - ly, rz = 2.f * nl * nz - lz;
  const float rv = fmaxf(rn_dot(rx, ry, rz, ex, ey, ez), 0.f);
  const float sp = nl > 0.f ? powf(rv, lt.shininess) : 0.f;
  float c[3];
  if (tex) ld_row<3>(tex + (long)b * tex_bs + (long)v * 3, c);
  else c[0] = c[1] = c[2] = lt.tex_value;
  const float k = lt.ambient + lt.diffuse * d;
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = k * c[a] + lt.specular * sp;
  st_row<3>(colors + t * 3, c);
}

// Pixel range [lo, hi] whose centres 1 - (2j + 1) / S may lie in [cmin, cmax],
// clamped to the image; lo > hi when the interval misses it.  Pixel j is in
// when u_lo <= j <= u_hi with u = ((1 - c) S - 1) / 2; the float32 u is within
// S 2^-23 <= 5e-4 pixel of the exact one, and so is any centre that the
// float32 edge functions can still call covered: kRnSlack = 1/64 pixel on
// either side keeps every such pixel.
constexpr float kRnSlack = 0.015625f;
__device__ __forceinline__ void rn_pixel_range(float cmin, float cmax, int S, int& lo, int& hi) {
#pragma clang fp contract(off)
  const float fs = (float)S;
  const float ulo = ((1.f - cmax) * fs - 1.f) * 0.5f - kRnSlack, uhi = ((1.f - cmin) * fs - 1.f) * 0.5f + kRnSlack;
  lo = (int)ceilf(fminf(fmaxf(ulo, 0.f), fs));          // [0, S]
  hi = (int)floorf(fminf(fmaxf(uhi, -1.f), fs - 1.f));  // [-1, S - 1]
}

// One thread per (mesh, group): the records of its faces and the group's box.
// Record (12 floats): x0 y0 x1 y1 | x2 y2 1/z0 1/z1 | 1/z2 1/area box_x box_y,
// a box packed as lo | hi << 16 in pixels; a dropped face has the empty box
// (lo = kRnNone, hi = 0), which no tile overlaps.
__global__ __launch_bounds__(256) void rn_setup_k(const float* __restrict__ ndc, const float* __restrict__ vz,
                                                  const int* __restrict__ faces, float* __restrict__ recs,
                                                  int* __restrict__ gbox, int nv, int nf, int ngroups, int S,
                                                  float znear, long total) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int m, g;
  divmod32(t, ngroups, m, g);
  const float* nb = ndc + (long)m * nv * 2;
  const float* zb = vz + (long)m * nv;
  float* rb = recs + ((long)m * nf + (long)g * kRnGroup) * kRnRec;
  const int cnt = min(kRnGroup, nf - g * kRnGroup);
  int gx0 = kRnMaxSize, gx1 = -1, gy0 = kRnMaxSize, gy1 = -1;
  for (int k = 0; k < cnt; ++k) {
    const int* fi = faces + ((long)g * kRnGroup + k) * 3;
    float x[3], y[3], z[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int vi = min(max(fi[j], 0), nv - 1);
      x[j] = nb[(long)vi * 2];
      y[j] = nb[(long)vi * 2 + 1];
      z[j] = zb[vi];
    }
    const float area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]);
    const bool keep = z[0] > znear && z[1] > znear && z[2] > znear && fabsf(area) > 0.f && fabsf(area) < INFINITY;
    int x0 = kRnNone, x1 = 0, y0 = kRnNone, y1 = 0;  // the empty box: lo above every pixel
    if (keep) {
      rn_pixel_range(fminf(x[0], fminf(x[1], x[2])), fmaxf(x[0], fmaxf(x[1], x[2])), S, x0, x1);
      rn_pixel_range(fminf(y[0], fminf(y[1], y[2])), fmaxf(y[0], fmaxf(y[1], y[2])), S, y0, y1);
      if (x0 > x1 || y0 > y1) {
        x0 = y0 = kRnNone;
        x1 = y1 = 0;
      } else {
        gx0 = min(gx0, x0);
        gx1 = max(gx1, x1);
        gy0 = min(gy0, y0);
        gy1 = max(gy1, y1);
      }
    }
    float* r = rb + k * kRnRec;
    st4(r, (f32x4){x[0], y[0], x[1], y[1]});
    st4(r + 4, (f32x4){x[2], y[2], 1.f / z[0], 1.f / z[1]});
    st4(r + 8, (f32x4){1.f / z[2], 1.f / area, __uint_as_float((unsigned)x0 | ((unsigned)x1 << 16)),
                       __uint_as_float((unsigned)y0 | ((unsigned)y1 << 16))});
  }
  if (gx1 < 0) {
    gx0 = gy0 = kRnNone;
    gx1 = gy1 = 0;
  }
  *reinterpret_cast<i32x4*>(gbox + ((long)m * ngroups + g) * 4) = (i32x4){gx0, gx1, gy0, gy1};
}

// Lane `src`'s value in every lane (src wave-uniform).
__device__ __forceinline__ float rn_bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// The image value of a pixel: the barycentric mix of the winning face's
// vertex colours, or the background.  image is planar [B, 3, S, S].
__device__ __forceinline__ void rn_shade_pixel(const int* __restrict__ faces, const float* __restrict__ cb, int f,
                                               float b0, float b1, float b2, int nv, int nf, float bg0, float bg1,
                                               float bg2, float* __restrict__ img, long plane) {
#pragma clang fp contract(off)
  float o[3] = {bg0, bg1, bg2};
  if (f >= 0) {
    const int* fi = faces + (long)min(f, nf - 1) * 3;
    float c[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) ld_row<3>(cb + (long)min(max(fi[j], 0), nv - 1) * 3, c + 3 * j);
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = b0 * c[a] + b1 * c[3 + a] + b2 * c[6 + a];
  }
  img[0] = o[0];
  img[plane] = o[1];
  img[2 * plane] = o[2];
}

// Block (mesh, tile row, tile column); lane l of every wave is the pixel
// (l >> 3, l & 7) of the tile, wave w walks the groups g = w (mod kRnWaves).
// The waves' winners meet in LDS and the one with the smallest (z, face)
// writes the pixel.
__global__ __launch_bounds__(64 * kRnWaves) void rn_raster_k(
    const float* __restrict__ recs, const int* __restrict__ gbox, const int* __restrict__ faces,
    const float* __restrict__ colors, int* __restrict__ pix_to_face, float* __restrict__ zbuf,
    float* __restrict__ bary, float* __restrict__ image, int nv, int nf, int ngroups, int S, int tiles, long c_bs,
    float bg0, float bg1, float bg2) {
#pragma clang fp contract(off)
  const int blk = (int)blockIdx.x;
  const int m = blk / (tiles * tiles), tt = blk - m * tiles * tiles;
  const int ty = tt / tiles, tx = tt - ty * tiles;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int qy0 = ty * kRnTile, qx0 = tx * kRnTile;  // < S: tiles = ceil(S / kRnTile)
  const int qy1 = min(qy0 + kRnTile, S) - 1, qx1 = min(qx0 + kRnTile, S) - 1;
  const int pi = qy0 + (lane >> 3), pj = qx0 + (lane & 7);
  const float px = 1.f - (float)(2 * pj + 1) / (float)S, py = 1.f - (float)(2 * pi + 1) / (float)S;
  const float* rm = recs + (long)m * nf * kRnRec;
  const i32x4* gm = reinterpret_cast<const i32x4*>(gbox) + (long)m * ngroups;
  float best = INFINITY, b0 = 0.f, b1 = 0.f, b2 = 0.f;
  int bf = -1;
  constexpr int kStep = 64 * kRnWaves;  // groups per round of the workgroup
  const int gl = lane * kRnWaves + wave;  // this lane's group of round 0
  i32x4 gnext = gm[min(gl, ngroups - 1)];
  for (int g0 = 0; g0 < ngroups; g0 += kStep) {
    const i32x4 gb = gnext;
    if (g0 + kStep < ngroups) gnext = gm[min(g0 + kStep + gl, ngroups - 1)];  // in flight while this batch is walked
    const bool ghit = g0 + gl < ngroups && gb.x <= qx1 && gb.y >= qx0 && gb.z <= qy1 && gb.w >= qy0;
    unsigned long long gmask = __ballot(ghit);
    while (gmask) {
      // up to four entered groups at a time: lanes 16 k .. 16 k + 15 load the records of the k-th
      int gsel = -1;
#pragma unroll
      for (int k = 0; k < 64 / kRnGroup; ++k) {
        if (gmask) {
          if ((lane >> 4) == k) gsel = g0 + __builtin_ctzll(gmask) * kRnWaves + wave;
          gmask &= gmask - 1;
        }
      }
      const int fl = gsel * kRnGroup + (lane & (kRnGroup - 1));
      const bool have = gsel >= 0 && fl < nf;
      const float* rl = rm + (long)(have ? fl : 0) * kRnRec;
      const f32x4 ra = ld4(rl), rb = ld4(rl + 4), rc = ld4(rl + 8);
      const unsigned bx = __float_as_uint(rc.z), by = __float_as_uint(rc.w);
      const bool fhit = have && (int)(bx & 0xffffu) <= qx1 && (int)(bx >> 16) >= qx0 &&
                        (int)(by & 0xffffu) <= qy1 && (int)(by >> 16) >= qy0;
      unsigned long long fmask = __ballot(fhit);
      while (fmask) {  // ascending lanes = ascending faces; the record comes from its lane's registers
        const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(fmask));
        fmask &= fmask - 1;
        const int f = __builtin_amdgcn_readlane(fl, src);
        const float x0 = rn_bcast(ra.x, src), y0 = rn_bcast(ra.y, src), x1 = rn_bcast(ra.z, src);
        const float y1 = rn_bcast(ra.w, src), x2 = rn_bcast(rb.x, src), y2 = rn_bcast(rb.y, src);
        const float ia = rn_bcast(rc.y, src);
        const float w0 = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1);
        const float w1 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2);
        const float w2 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0);
        const bool in = ia > 0.f ? (w0 >= 0.f && w1 >= 0.f && w2 >= 0.f) : (w0 <= 0.f && w1 <= 0.f && w2 <= 0.f);
        if (in) {
          const float t0 = w0 * ia * rn_bcast(rb.z, src), t1 = w1 * ia * rn_bcast(rb.w, src);
          const float t2 = w2 * ia * rn_bcast(rc.x, src);
          const float z = 1.f / (t0 + t1 + t2);
          if (z < best) {
            best = z;
            bf = f;
            b0 = t0 * z;
            b1 = t1 * z;
            b2 = t2 * z;
          }
        }
      }
    }
  }
  // the waves' (z, face) meet: the smallest pair owns the pixel, wave 0 a pixel nobody hit
  __shared__ float sz[kRnWaves][64];
  __shared__ int sf[kRnWaves][64];
  sz[wave][lane] = best;
  sf[wave][lane] = bf;
  __syncthreads();
  int owner = 0, of = sf[0][lane];
  float oz = sz[0][lane];
#pragma unroll
  for (int w = 1; w < kRnWaves; ++w) {
    const float z = sz[w][lane];
    const int f = sf[w][lane];
    if (f >= 0 && (of < 0 || z < oz || (z == oz && f < of))) {
      owner = w;
      oz = z;
      of = f;
    }
  }
  if (owner != wave || pi >= S || pj >= S) return;
  const long o = ((long)m * S + pi) * S + pj;
  const bool hit = bf >= 0;
  pix_to_face[o] = bf;
  zbuf[o] = hit ? best : -1.f;
  const float v[3] = {hit ? b0 : -1.f, hit ? b1 : -1.f, hit ? b2 : -1.f};
  st_row<3>(bary + o * 3, v);
  if (image) {
    const long plane = (long)S * S;
    rn_shade_pixel(faces, colors + (long)m * c_bs, bf, b0, b1, b2, nv, nf, bg0, bg1, bg2,
                   image + (long)m * 3 * plane + (long)pi * S + pj, plane);
  }
}

// One thread per pixel: the image from a finished raster stage.
__global__ __launch_bounds__(256) void rn_interp_k(const int* __restrict__ pix_to_face, const float* __restrict__ bary,
                                                   const int* __restrict__ faces, const float* __restrict__ colors,
                                                   float* __restrict__ image, int nv, int nf, int npix, long c_bs,
                                                   float bg0, float bg1, float bg2, long total) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int m, p;
  divmod32(t, npix, m, p);
  float w[3];
  ld_row<3>(bary + t * 3, w);
  rn_shade_pixel(faces, colors + (long)m * c_bs, pix_to_face[t], w[0], w[1], w[2], nv, nf, bg0, bg1, bg2,
                 image + (long)m * 3 * npix + p, npix);
}

static size_t rn_workspace(int batch, int nf) {
  const size_t ngroups = ((size_t)nf + kRnGroup - 1) / kRnGroup;
  return (size_t)batch * ((size_t)nf * kRnRec * sizeof(float) + ngroups * 4 * sizeof(int));
}

static int rn_check_mesh(const char* what, int batch, int nv, int nf) {
  if (batch <= 0 || nv <= 0 || nf <= 0)
    return set_error(CFSD_EINVAL, "%s: bad sizes batch=%d nv=%d nf=%d (all must be >= 1)", what, batch, nv, nf);
  if ((long)batch * nv * 3 >= (1L << 31) || (long)batch * nf * kRnRec >= (1L << 31))
    return set_error(CFSD_EINVAL, "%s: batch x vertices x 3 or batch x faces x 12 >= 2^31 (32-bit indices)", what);
  return CFSD_OK;
}

static int rn_check_image(const char* what, int batch, int size) {
  if (size <= 0 || size > kRnMaxSize)
    return set_error(CFSD_EINVAL, "%s: bad sizes image_size=%d (must be in [1, %d])", what, size, kRnMaxSize);
  if ((long)batch * size * size * 3 >= (1L << 31))
    return set_error(CFSD_EINVAL, "%s: batch x pixels x 3 >= 2^31 (32-bit indices)", what);
  return CFSD_OK;
}

}  // namespace cfsd

using namespace cfsd;

extern "C" size_t cfsd_raster_workspace(int batch, int nf) {
  if (batch <= 0 || nf <= 0 || (long)batch * nf * kRnRec >= (1L << 31)) return 0;
  return rn_workspace(batch, nf);
}

extern "C" int cfsd_vertex_normals(const float* verts, const int32_t* faces, const int32_t* vf_ptr,
                                   const int32_t* vf_idx, float* normals, int batch, int nv, int nf, void* stream) {
  if (!verts || !faces || !vf_ptr || !vf_idx || !normals)
    return set_error(CFSD_EINVAL, "vertex_normals: null pointer");
  if (int rc = rn_check_mesh("vertex_normals", batch, nv, nf)) return rc;
  const long total = (long)batch * nv;
  hipLaunchKernelGGL(rn_normals_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts,
                     faces, vf_ptr, vf_idx, normals, nv, nf, total);
  return launch_status("vertex_normals");
}

extern "C" int cfsd_render_vertices(const float* verts, const float* cam, const int32_t* faces,
                                    const int32_t* vf_ptr, const int32_t* vf_idx, const float* tex, float* ndc,
                                    float* vz, float* colors, int batch, int bt, int nv, int nf, float light_x,
                                    float light_y, float light_z, float ambient, float diffuse, float specular,
                                    float shininess, float tex_value, void* stream) {
  if (!verts || !cam || !ndc || !vz) return set_error(CFSD_EINVAL, "render_vertices: null pointer");
  if (colors && (!faces || !vf_ptr || !vf_idx))
    return set_error(CFSD_EINVAL, "render_vertices: null pointer (colours need faces and their vertex runs)");
  if (int rc = rn_check_mesh("render_vertices", batch, nv, colors ? nf : 1)) return rc;
  if (tex && bt != 1 && bt != batch)
    return set_error(CFSD_EINVAL, "render_vertices: texture batch %d must be 1 or %d", bt, batch);
  const long total = (long)batch * nv;
  const RnLight lt{light_x, light_y, light_z, ambient, diffuse, specular, shininess, tex_value};
  hipLaunchKernelGGL(rn_vertices_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts,
                     cam, faces, vf_ptr, vf_idx, colors ? tex : nullptr, ndc, vz, colors, lt, nv, nf,
                     bt == 1 ? 0L : (long)nv * 3, total);
  return launch_status("render_vertices");
}

extern "C" int cfsd_rasterize(const float* ndc, const float* vz, const int32_t* faces, const float* colors,
                              int32_t* pix_to_face, float* zbuf, float* bary, float* image, void* workspace,
                              size_t workspace_bytes, int batch, int bc, int nv, int nf, int image_size, float znear,
                              float bg_r, float bg_g, float bg_b, void* stream) {
  if (!ndc || !vz || !faces || !pix_to_face || !zbuf || !bary)
    return set_error(CFSD_EINVAL, "rasterize: null pointer");
  if ((image != nullptr) != (colors != nullptr))
    return set_error(CFSD_EINVAL, "rasterize: null pointer (image and colors go together)");
  if (int rc = rn_check_mesh("rasterize", batch, nv, nf)) return rc;
  if (int rc = rn_check_image("rasterize", batch, image_size)) return rc;
  if (colors && bc != 1 && bc != batch)
    return set_error(CFSD_EINVAL, "rasterize: colour batch %d must be 1 or %d", bc, batch);
  const size_t need = rn_workspace(batch, nf);
  if (!workspace || workspace_bytes < need)
    return set_error(CFSD_EWORKSPACE, "rasterize: workspace %zu < %zu bytes", workspace_bytes, need);
  if ((uintptr_t)workspace & 15) return set_error(CFSD_EINVAL, "rasterize: workspace is not 16-byte aligned");
  const int ngroups = (nf + kRnGroup - 1) / kRnGroup;
  const int tiles = (image_size + kRnTile - 1) / kRnTile;
  const long blocks = (long)batch * tiles * tiles;
  if (blocks >= (1L << 30)) return set_error(CFSD_EINVAL, "rasterize: too many workgroups");
  float* recs = (float*)workspace;
  int* gbox = (int*)(recs + (size_t)batch * nf * kRnRec);
  const hipStream_t st = (hipStream_t)stream;
  const long total = (long)batch * ngroups;
  hipLaunchKernelGGL(rn_setup_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ndc, vz, faces, recs, gbox,
                     nv, nf, ngroups, image_size, znear, total);
  hipLaunchKernelGGL(rn_raster_k, dim3((unsigned)blocks), dim3(64 * kRnWaves), 0, st, recs, gbox, faces, colors, pix_to_face,
                     zbuf, bary, image, nv, nf, ngroups, image_size, tiles, bc == 1 ? 0L : (long)nv * 3, bg_r, bg_g,
                     bg_b);
  return launch_status("rasterize");
}

extern "C" int cfsd_interpolate_colors(const int32_t* pix_to_face, const float* bary, const int32_t* faces,
                                       const float* colors, float* image, int batch, int bc, int nv, int nf,
                                       int image_size, float bg_r, float bg_g, float bg_b, void* stream) {
  if (!pix_to_face || !bary || !faces || !colors || !image)
    return set_error(CFSD_EINVAL, "interpolate_colors: null pointer");
  if (int rc = rn_check_mesh("interpolate_colors", batch, nv, nf)) return rc;
  if (int rc = rn_check_image("interpolate_colors", batch, image_size)) return rc;
  if (bc != 1 && bc != batch)
    return set_error(CFSD_EINVAL, "interpolate_colors: colour batch %d must be 1 or %d", bc, batch);
  const int npix = image_size * image_size;
  const long total = (long)batch * npix;
  hipLaunchKernelGGL(rn_interp_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     pix_to_face, bary, faces, colors, image, nv, nf, npix, bc == 1 ? 0L : (long)nv * 3, bg_r, bg_g,
                     bg_b, total);
  return launch_status("interpolate_colors");
}
