// Point-to-triangle distance of the surface fitting term (gfx950): for every
// query point the nearest point of a triangle mesh (squared distance, face,
// barycentric weights), and the gradient with respect to the points and to
// the mesh's vertices.
//
// Reference: Tester._point_mesh_distance (test.py:522-533) measures a fit with
// pytorch3d's point_face_distance, which has no ROCm build.  Semantics
// restated here: the distance of a point to a mesh is its distance to the
// nearest point of the nearest CLOSED triangle.
//
// One pair (pf_pair).  Every candidate is a point of the triangle: the clamped
// projection onto each of the three edges and, where the plane projection has
// three positive barycentric numerators, that projection.  The result is the
// candidate with the smallest |p - c|^2, the difference built in coordinates
// relative to corner a (p - a - v (b - a) - w (c - a)), so the error scales
// with the distance to the triangle's corners and not with the distance to
// the origin.  A zero-area face has no interior candidate that can win
// wrongly (it is only one more point of the face) and its edges degrade to
// segments or a point: no division by a zero length is ever made, so finite
// input gives finite output.  One instruction sequence, contraction pinned:
// the same pair gives the same bits wherever it is evaluated.
//
// The search.  A lane owns one query; a wave walks the faces in ascending
// order with wave-uniform addresses (scalar loads), so a strict '<' keeps the
// lowest face among equal distances.  A pre-launch (pf_prepare_k) writes per
// face its corners (48 bytes) and its bounding sphere (16 bytes, an array of
// its own: the spheres of a group are fetched eight at a time, one load
// latency per eight tests) and one sphere per group of kPfGroup consecutive
// faces.  With culling on, a group is entered
// only if some lane of the wave may be nearer to its sphere than the lane's
// bound, and a face of an entered group is evaluated only if some lane may be
// nearer to the face's sphere; a lane's bound is min(seed, running minimum),
// the seed being the distance to ONE face the caller names per query (a face
// at the nearest referenced vertex).  The seed only culls: the running
// minimum starts at +inf and the seed's face is met again in its turn.
//
// Why culling is exact.  Let D be the distance of the query to a sphere's
// centre, r its radius, s = sqrt(bound).  Every face f inside the sphere has
// true distance >= D - r and farthest corner L <= D + r, and pf_pair's result
// is >= d_true^2 - K eps L^2 with K far below kPfK = 1024 (eps = 2^-24; the
// tests measure K against float64).  So the face cannot reach the bound if
//   (D - r)^2 - kPfK eps (D + r)^2 > s^2,
// which follows (sqrt(a + b) <= sqrt(a) + sqrt(b), (D + r)^2 <= 2 (D^2 + r^2))
// from D (1 - mu) > s + r (1 + mu) with mu = sqrt(2 kPfK eps) = 2^-6.5 = 0.0111.
// The kernel tests D^2 > ((s + r') kPfKappa)^2 with r' = kPfKappa r stored by
// the pre-launch and kPfKappa = 1.02 > 1 / (1 - mu): 0.9 % of slack on either
// side for the fp32 rounding of D^2, r and s themselves.  A face whose lower
// bound merely equals the bound is therefore never skipped, and since the
// bound never falls below the final minimum, the skipped faces are exactly
// faces that a brute-force walk would have rejected: the results are
// bit-identical with culling off.
#include <math.h>

#include "cfsd_common.h"

namespace cfsd {

constexpr int kPfGroup = CFSD_PF_GROUP;  // faces per group sphere
constexpr int kPfCor = 12;               // floats per face in the corner array: a, b, c, 3 pad
constexpr int kPfRec = kPfCor + 4;       // floats per face in all: corners + sphere (centre, r')
constexpr int kPfBlock = 64;             // one wave: its queries are neighbours on the surface
constexpr int kPfChunk = 8;              // spheres (of groups, of faces) tested per batch of scalar loads
constexpr float kPfKappa = 1.02f;        // see "Why culling is exact"
constexpr float kPfTiny = 1e-30f;        // squared edge length below which an edge is a point

struct PfHit {
  float d2, v, w;  // closest point = (1 - v - w) a + v b + w c
};

__device__ __forceinline__ float pf_dot(float x0, float y0, float z0, float x1, float y1, float z1) {
#pragma clang fp contract(off)
  return fmaf(z0, z1, fmaf(y0, y1, x0 * x1));
}

// t in [0, 1] minimising |base - t dir|^2 given num = base.dir, den = dir.dir.
__device__ __forceinline__ float pf_param(float num, float den) {
#pragma clang fp contract(off)
  const float t = den > kPfTiny ? num * __builtin_amdgcn_rcpf(den) : 0.f;
  return fminf(fmaxf(t, 0.f), 1.f);
}

__device__ __forceinline__ PfHit pf_pair(float px, float py, float pz, float ax, float ay, float az, float bx,
                                         float by, float bz, float cx, float cy, float cz) {
#pragma clang fp contract(off)
  const float ux = bx - ax, uy = by - ay, uz = bz - az;  // ab
  const float vx = cx - ax, vy = cy - ay, vz = cz - az;  // ac
  const float qx = px - ax, qy = py - ay, qz = pz - az;  // ap
  const float wx = vx - ux, wy = vy - uy, wz = vz - uz;  // bc
  const float sx = qx - ux, sy = qy - uy, sz = qz - uz;  // bp
  const float uu = pf_dot(ux, uy, uz, ux, uy, uz), vv = pf_dot(vx, vy, vz, vx, vy, vz);
  const float uv = pf_dot(ux, uy, uz, vx, vy, vz);
  const float uq = pf_dot(ux, uy, uz, qx, qy, qz), vq = pf_dot(vx, vy, vz, qx, qy, qz);
  PfHit h;
  {  // edge ab
    const float t = pf_param(uq, uu);
    const float ex = fmaf(-t, ux, qx), ey = fmaf(-t, uy, qy), ez = fmaf(-t, uz, qz);
    h.d2 = pf_dot(ex, ey, ez, ex, ey, ez);
    h.v = t;
    h.w = 0.f;
  }
  {  // edge ac
    const float t = pf_param(vq, vv);
    const float ex = fmaf(-t, vx, qx), ey = fmaf(-t, vy, qy), ez = fmaf(-t, vz, qz);
    const float d = pf_dot(ex, ey, ez, ex, ey, ez);
    if (d < h.d2) {
      h.d2 = d;
      h.v = 0.f;
      h.w = t;
    }
  }
  {  // edge bc
    const float t = pf_param(pf_dot(wx, wy, wz, sx, sy, sz), pf_dot(wx, wy, wz, wx, wy, wz));
    const float ex = fmaf(-t, wx, sx), ey = fmaf(-t, wy, sy), ez = fmaf(-t, wz, sz);
    const float d = pf_dot(ex, ey, ez, ex, ey, ez);
    if (d < h.d2) {
      h.d2 = d;
      h.v = 1.f - t;
      h.w = t;
    }
  }
  {  // the plane projection, where it falls inside
    const float det = uu * vv - uv * uv;
    const float nv = vv * uq - uv * vq, nw = uu * vq - uv * uq;
    const float nu = (det - nv) - nw;
    const float inv = det > kPfTiny ? __builtin_amdgcn_rcpf(det) : 0.f;
    const float v = fminf(nv * inv, 1.f), w = fminf(nw * inv, 1.f);
    const float ex = fmaf(-w, vx, fmaf(-v, ux, qx)), ey = fmaf(-w, vy, fmaf(-v, uy, qy));
    const float ez = fmaf(-w, vz, fmaf(-v, uz, qz));
    const float d = pf_dot(ex, ey, ez, ex, ey, ez);
    if (nv > 0.f && nw > 0.f && nu > 0.f && det > kPfTiny && d < h.d2) {
      h.d2 = d;
      h.v = v;
      h.w = w;
    }
  }
  return h;
}

__device__ __forceinline__ PfHit pf_pair_rec(float px, float py, float pz, const float* __restrict__ r) {
  return pf_pair(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]);
}

// May a face inside the sphere (cx, cy, cz, r') reach a lane whose bound is s^2?
__device__ __forceinline__ bool pf_may_hit(float px, float py, float pz, float cx, float cy, float cz, float r1,
                                           float s) {
#pragma clang fp contract(off)
  const float dx = px - cx, dy = py - cy, dz = pz - cz;
  const float t = (s + r1) * kPfKappa;
  return !(pf_dot(dx, dy, dz, dx, dy, dz) > t * t);
}

// One thread per (mesh, group): the corners and spheres of its faces and the group's sphere.
__global__ __launch_bounds__(256) void pf_prepare_k(const float* __restrict__ verts, const int* __restrict__ faces,
                                                    float* __restrict__ cors, float* __restrict__ fsph,
                                                    float* __restrict__ gsph, int nv, int nf, int ngroups,
                                                    long total) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int m = (int)(t / ngroups), g = (int)(t - (long)m * ngroups);
  const float* vb = verts + (long)m * nv * 3;
  float* cb = cors + ((long)m * nf + (long)g * kPfGroup) * kPfCor;
  float* sb = fsph + ((long)m * nf + (long)g * kPfGroup) * 4;
  const int cnt = min(kPfGroup, nf - g * kPfGroup);
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int k = 0; k < cnt; ++k) {
    const int* fi = faces + ((long)g * kPfGroup + k) * 3;
    float c[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int vi = min(max(fi[j], 0), nv - 1);
      ld_row<3>(vb + (long)vi * 3, c + 3 * j);
    }
    const float mx = (c[0] + c[3] + c[6]) * (1.f / 3.f), my = (c[1] + c[4] + c[7]) * (1.f / 3.f);
    const float mz = (c[2] + c[5] + c[8]) * (1.f / 3.f);
    float r2 = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float dx = c[3 * j] - mx, dy = c[3 * j + 1] - my, dz = c[3 * j + 2] - mz;
      r2 = fmaxf(r2, pf_dot(dx, dy, dz, dx, dy, dz));
    }
    float* r = cb + k * kPfCor;
    st4(r, (f32x4){c[0], c[1], c[2], c[3]});
    st4(r + 4, (f32x4){c[4], c[5], c[6], c[7]});
    st4(r + 8, (f32x4){c[8], 0.f, 0.f, 0.f});
    st4(sb + k * 4, (f32x4){mx, my, mz, sqrtf(r2) * kPfKappa});
    gx += mx;
    gy += my;
    gz += mz;
  }
  const float inv = 1.f / (float)cnt;
  gx *= inv;
  gy *= inv;
  gz *= inv;
  float gr = 0.f;
  for (int k = 0; k < cnt; ++k) {  // the spheres just written by this thread
    const float* r = sb + k * 4;
    const float dx = r[0] - gx, dy = r[1] - gy, dz = r[2] - gz;
    gr = fmaxf(gr, sqrtf(pf_dot(dx, dy, dz, dx, dy, dz)) * kPfKappa + r[3]);
  }
  st4(gsph + ((long)m * ngroups + g) * 4, (f32x4){gx, gy, gz, gr});
}

// Block (b, chunk): queries [chunk * 64, +64) of batch b against every face of
// mesh b (or of the one shared mesh: cor_bs = f_bs = g_bs = 0; p_bs = 0 shares
// the points).  stats (may be null): per wave the groups entered and the faces
// evaluated.
__global__ __launch_bounds__(kPfBlock) void point_face_k(const float* __restrict__ points,
                                                         const float* __restrict__ cors,
                                                         const float* __restrict__ fsph,
                                                         const float* __restrict__ gsph,
                                                         const int* __restrict__ seed_face, float* __restrict__ dist2,
                                                         int* __restrict__ face_idx, float* __restrict__ bary,
                                                         int* __restrict__ stats, int n, int nf, int ngroups,
                                                         long p_bs, long cor_bs, long f_bs, long g_bs, int cull,
                                                         int nchunks) {
  const int blk = (int)blockIdx.x;
  const int b = blk / nchunks, ch = blk - b * nchunks;
  const int i = ch * kPfBlock + (int)threadIdx.x;
  const int ic = min(i, n - 1);  // clamped lanes: loads only
  const float* pp = points + (long)b * p_bs + (long)ic * 3;
  const float px = pp[0], py = pp[1], pz = pp[2];
  const float* cor = cors + (long)b * cor_bs;
  const f32x4* fs = reinterpret_cast<const f32x4*>(fsph + (long)b * f_bs);
  const f32x4* gs = reinterpret_cast<const f32x4*>(gsph + (long)b * g_bs);
  float ub = INFINITY;
  if (seed_face) {
    const int f0 = min(max(seed_face[(long)b * n + ic], 0), nf - 1);
    ub = pf_pair_rec(px, py, pz, cor + (long)f0 * kPfCor).d2;
  }
  float best = INFINITY, bv = 0.f, bw = 0.f, s = sqrtf(ub);
  int bf = 0, n_groups = 0, n_faces = 0;
  for (int g0 = 0; g0 < ngroups; g0 += kPfChunk) {
    unsigned mask = 0;
    if (cull) {
      f32x4 q[kPfChunk];
#pragma unroll
      for (int k = 0; k < kPfChunk; ++k) q[k] = gs[min(g0 + k, ngroups - 1)];
#pragma unroll
      for (int k = 0; k < kPfChunk; ++k)
        if (__any(pf_may_hit(px, py, pz, q[k].x, q[k].y, q[k].z, q[k].w, s))) mask |= 1u << k;
    } else {
      mask = (1u << kPfChunk) - 1;
    }
    if (g0 + kPfChunk > ngroups) mask &= (1u << (ngroups - g0)) - 1;
    while (mask) {
      const int g = g0 + __builtin_ctz(mask);
      mask &= mask - 1;
      ++n_groups;
      const int fb = g * kPfGroup, cnt = min(kPfGroup, nf - fb);
      for (int h0 = 0; h0 < cnt; h0 += kPfChunk) {
        unsigned fm = (1u << kPfChunk) - 1;
        if (cull) {
          f32x4 q[kPfChunk];
#pragma unroll
          for (int k = 0; k < kPfChunk; ++k) q[k] = fs[min(fb + h0 + k, nf - 1)];
          fm = 0;
#pragma unroll
          for (int k = 0; k < kPfChunk; ++k)
            if (__any(pf_may_hit(px, py, pz, q[k].x, q[k].y, q[k].z, q[k].w, s))) fm |= 1u << k;
        }
        if (h0 + kPfChunk > cnt) fm &= (1u << (cnt - h0)) - 1;
        while (fm) {  // ascending: the bound a face was tested with is never below the current one
          const int f = fb + h0 + __builtin_ctz(fm);
          fm &= fm - 1;
          ++n_faces;
          const PfHit h = pf_pair_rec(px, py, pz, cor + (long)f * kPfCor);
          if (h.d2 < best) {
            best = h.d2;
            bf = f;
            bv = h.v;
            bw = h.w;
            s = sqrtf(fminf(best, ub));
          }
        }
      }
    }
  }
  if (i < n) {
    const long o = (long)b * n + i;
    dist2[o] = best;
    face_idx[o] = bf;
    bary[o * 3] = (1.f - bv) - bw;
    bary[o * 3 + 1] = bv;
    bary[o * 3 + 2] = bw;
  }
  if (stats && threadIdx.x == 0) {
    stats[(long)blk * 2] = n_groups;
    stats[(long)blk * 2 + 1] = n_faces;
  }
}

// One thread per point (b, i): gp = g 2 (p - c), c the closest point rebuilt
// from the weights relative to corner a, as the forward built it.
__global__ __launch_bounds__(256) void pf_bwd_points_k(const float* __restrict__ points,
                                                       const float* __restrict__ verts, const int* __restrict__ faces,
                                                       const int* __restrict__ face_idx,
                                                       const float* __restrict__ bary, const float* __restrict__ g,
                                                       float* __restrict__ gp, int n, int nv, int nf, long p_bs,
                                                       long v_bs, long total) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int b = (int)(t / n), i = (int)(t - (long)b * n);
  const float* pp = points + (long)b * p_bs + (long)i * 3;
  const float* vb = verts + (long)b * v_bs;
  const int* fi = faces + (long)min(max(face_idx[t], 0), nf - 1) * 3;
  float c[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) ld_row<3>(vb + (long)min(max(fi[j], 0), nv - 1) * 3, c + 3 * j);
  const float v = bary[t * 3 + 1], w = bary[t * 3 + 2], k2 = 2.f * g[t];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float e = fmaf(-w, c[6 + a] - c[a], fmaf(-v, c[3 + a] - c[a], pp[a] - c[a]));
    gp[t * 3 + a] = k2 * e;
  }
}

// One thread per mesh vertex (b, u): gv = - sum over the run of (point i,
// corner k) pairs whose winning face has u as corner k, ascending, of
// gp[b, i] * bary[b, i, k].  An empty run leaves zero.  No atomics.
__global__ __launch_bounds__(256) void pf_bwd_verts_k(const float* __restrict__ gp, const float* __restrict__ bary,
                                                      const int* __restrict__ seg_ptr, const int* __restrict__ seg_e,
                                                      float* __restrict__ gv, int n, int nv, long total) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int b = (int)(t / nv), u = (int)(t - (long)b * nv);
  const int* sp = seg_ptr + (long)b * (nv + 1) + u;
  const int m = 3 * n;
  const int e0 = min(max(sp[0], 0), m), e1 = min(max(sp[1], 0), m);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int e = e0; e < e1; ++e) {
    const int ik = min(max(seg_e[(long)b * m + e], 0), m - 1);  // i * 3 + k
    const long row = (long)b * n + ik / 3;
    const float wk = bary[(long)b * m + ik];
    s0 += gp[row * 3] * wk;
    s1 += gp[row * 3 + 1] * wk;
    s2 += gp[row * 3 + 2] * wk;
  }
  gv[t * 3] = -s0;
  gv[t * 3 + 1] = -s1;
  gv[t * 3 + 2] = -s2;
}

static int pf_check_sizes(const char* what, int batch, int bp, int bv, int n, int nv, int nf) {
  if (batch <= 0 || n <= 0 || nv <= 0 || nf <= 0)
    return set_error(CFSD_EINVAL, "%s: bad sizes batch=%d n=%d nv=%d nf=%d (all must be >= 1)", what, batch, n, nv,
                     nf);
  if ((bp != 1 && bp != batch) || (bv != 1 && bv != batch))
    return set_error(CFSD_EINVAL, "%s: operand batches %d and %d must each be 1 or %d", what, bp, bv, batch);
  if ((long)batch * n * 3 >= (1L << 31) || (long)batch * nv * 3 >= (1L << 31) ||
      (long)batch * nf * kPfRec >= (1L << 31))
    return set_error(CFSD_EINVAL, "%s: batch x points x 3, batch x vertices x 3 or batch x faces x 16 >= 2^31 "
                     "(32-bit indices)", what);
  return CFSD_OK;
}

static size_t pf_workspace(int bv, int nf) {
  const size_t ngroups = ((size_t)nf + kPfGroup - 1) / kPfGroup;
  return (size_t)bv * ((size_t)nf * kPfRec + ngroups * 4) * sizeof(float);
}

}  // namespace cfsd

using namespace cfsd;

extern "C" size_t cfsd_point_face_workspace(int bv, int nf) {
  if (bv <= 0 || nf <= 0 || (long)bv * nf * kPfRec >= (1L << 31)) return 0;
  return pf_workspace(bv, nf);
}

extern "C" int cfsd_point_face(const float* points, const float* verts, const int32_t* faces,
                               const int32_t* seed_face, float* dist2, int32_t* face_idx, float* bary,
                               int32_t* stats, void* workspace, size_t workspace_bytes, int batch, int bp, int bv,
                               int n, int nv, int nf, int flags, void* stream) {
  if (!points || !verts || !faces || !dist2 || !face_idx || !bary)
    return set_error(CFSD_EINVAL, "point_face: null pointer");
  if (int rc = pf_check_sizes("point_face", batch, bp, bv, n, nv, nf)) return rc;
  if (flags & ~(CFSD_PF_CULL | CFSD_PF_PREPARED)) return set_error(CFSD_EINVAL, "point_face: unknown flags %d", flags);
  const size_t need = pf_workspace(bv, nf);
  if (!workspace || workspace_bytes < need)
    return set_error(CFSD_EWORKSPACE, "point_face: workspace %zu < %zu bytes", workspace_bytes, need);
  if ((uintptr_t)workspace & 15) return set_error(CFSD_EINVAL, "point_face: workspace is not 16-byte aligned");
  const int ngroups = (nf + kPfGroup - 1) / kPfGroup;
  const int nchunks = (n + kPfBlock - 1) / kPfBlock;
  const long blocks = (long)batch * nchunks;
  if (blocks >= (1L << 30)) return set_error(CFSD_EINVAL, "point_face: too many workgroups");
  float* cors = (float*)workspace;
  float* fsph = cors + (size_t)bv * nf * kPfCor;
  float* gsph = fsph + (size_t)bv * nf * 4;
  const hipStream_t st = (hipStream_t)stream;
  if (!(flags & CFSD_PF_PREPARED)) {
    const long total = (long)bv * ngroups;
    hipLaunchKernelGGL(pf_prepare_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, verts, faces, cors,
                       fsph, gsph, nv, nf, ngroups, total);
  }
  hipLaunchKernelGGL(point_face_k, dim3((unsigned)blocks), dim3(kPfBlock), 0, st, points, cors, fsph, gsph,
                     seed_face, dist2, face_idx, bary, stats, n, nf, ngroups, bp == 1 ? 0L : (long)n * 3,
                     bv == 1 ? 0L : (long)nf * kPfCor, bv == 1 ? 0L : (long)nf * 4,
                     bv == 1 ? 0L : (long)ngroups * 4,
                     (flags & CFSD_PF_CULL) ? 1 : 0, nchunks);
  return launch_status("point_face");
}

extern "C" int cfsd_point_face_bwd(const float* points, const float* verts, const int32_t* faces,
                                   const int32_t* face_idx, const float* bary, const float* g, float* gp,
                                   const int32_t* seg_ptr, const int32_t* seg_e, float* gv, int batch, int bp,
                                   int bv, int n, int nv, int nf, void* stream) {
  if (!points || !verts || !faces || !face_idx || !bary || !g || !gp)
    return set_error(CFSD_EINVAL, "point_face_bwd: null pointer");
  if (gv && (!seg_ptr || !seg_e)) return set_error(CFSD_EINVAL, "point_face_bwd: null pointer (vertex runs)");
  if (int rc = pf_check_sizes("point_face_bwd", batch, bp, bv, n, nv, nf)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const long total = (long)batch * n;
  hipLaunchKernelGGL(pf_bwd_points_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, points, verts, faces,
                     face_idx, bary, g, gp, n, nv, nf, bp == 1 ? 0L : (long)n * 3, bv == 1 ? 0L : (long)nv * 3,
                     total);
  if (gv) {
    const long tv = (long)batch * nv;
    hipLaunchKernelGGL(pf_bwd_verts_k, dim3((unsigned)((tv + 255) / 256)), dim3(256), 0, st, gp, bary, seg_ptr, seg_e,
                       gv, n, nv, tv);
  }
  return launch_status("point_face_bwd");
}
