// Compute mesh renderer: vertex normals + camera, then a z-buffered tile rasteriser with Lambert shading.
// An Instinct card has no graphics pipe; this turns the (B, V, 3) vertices msmd_lbs_skin_v2 leaves on the device into images
// there.  Two launches per batch of frames, no host synchronisation, no global atomics, bit-identical from run to run.
// A texture adds a mip pyramid (built once per image) and a third, deferred launch that shades the covered pixels from it
// (DESIGN.md 5.14).  The raster and the textured kernel are templates on the samples per pixel: one, or four for anti-aliased
// frames.  Per-vertex colours are a second deferred pass of the textured pass's shape, lit or unlit.
#include "common.h"

namespace {

__device__ __forceinline__ F3 cross3(const F3 a, const F3 b) {
  return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ F3 mat3_mul(const float* R, const F3 v) {
  return F3{R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z};
}
__device__ __forceinline__ F3 unit_or_z(const F3 v) {
  const float n2 = v.x * v.x + v.y * v.y + v.z * v.z;
  if (!(n2 > 0.f)) return F3{0.f, 0.f, 1.f};
  const float n = sqrtf(n2);
  return F3{v.x / n, v.y / n, v.z / n};
}

// ------------------------------------------------------------------------------------------------ vertex stage
// One thread per (frame, vertex): area-weighted normal gathered through the vertex -> face CSR table in CSR order (the sum
// of the incident faces' un-normalised cross products, so no atomics and one fixed order), the optional per-frame rigid
// motion about t_center (Rodrigues as cv2 defines it: angle = |r|, identity at 0), world -> eye, the perspective
// projection with aspect ratio 1 and the viewport transform with row 0 at the top.
__global__ __launch_bounds__(256) void render_vertices_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                              const int* __restrict__ csr_off, const int* __restrict__ csr_face,
                                                              const float* __restrict__ view, const float* __restrict__ t_center,
                                                              const float* __restrict__ rot, float* __restrict__ screen,
                                                              float* __restrict__ normals, int B, int V, int F, float focal,
                                                              float Wf, float Hf) {
  const long t = blockIdx.x * 256L + threadIdx.x;
  if (t >= (long)B * V) return;
  const int b = (int)(t / V), v = (int)(t - (long)b * V);
  const float* vb = verts + (long)b * V * 3;
  F3 p = *(const F3*)(vb + (long)v * 3);
  F3 n{0.f, 0.f, 0.f};
  const int e0 = csr_off[v], e1 = csr_off[v + 1];
  for (int e = e0; e < e1; ++e) {
    const int f = csr_face[e];
    if ((unsigned)f >= (unsigned)F) continue;
    const I3 vi = *(const I3*)(faces + (long)f * 3);
    if ((unsigned)vi.a >= (unsigned)V || (unsigned)vi.b >= (unsigned)V || (unsigned)vi.c >= (unsigned)V) continue;
    const F3 a = *(const F3*)(vb + (long)vi.a * 3), q = *(const F3*)(vb + (long)vi.b * 3), c = *(const F3*)(vb + (long)vi.c * 3);
    const F3 cr = cross3(F3{q.x - a.x, q.y - a.y, q.z - a.z}, F3{c.x - a.x, c.y - a.y, c.z - a.z});
    n.x += cr.x; n.y += cr.y; n.z += cr.z;
  }
  n = unit_or_z(n);
  if (rot != nullptr) {
    const float rx = rot[b * 3], ry = rot[b * 3 + 1], rz = rot[b * 3 + 2];
    const float th = sqrtf(rx * rx + ry * ry + rz * rz);
    if (th > 0.f) {
      const float kx = rx / th, ky = ry / th, kz = rz / th;
      float s, c;
      sincosf(th, &s, &c);
      const float c1 = 1.f - c;
      const float R[9] = {c + c1 * kx * kx, c1 * kx * ky - s * kz, c1 * kx * kz + s * ky,
                          c1 * kx * ky + s * kz, c + c1 * ky * ky, c1 * ky * kz - s * kx,
                          c1 * kx * kz - s * ky, c1 * ky * kz + s * kx, c + c1 * kz * kz};
      const F3 tc{t_center[0], t_center[1], t_center[2]};
      const F3 r = mat3_mul(R, F3{p.x - tc.x, p.y - tc.y, p.z - tc.z});
      p = F3{r.x + tc.x, r.y + tc.y, r.z + tc.z};
      n = mat3_mul(R, n);
    }
  }
  const float M[9] = {view[0], view[1], view[2], view[4], view[5], view[6], view[8], view[9], view[10]};
  F3 pe = mat3_mul(M, p);
  pe.x += view[3]; pe.y += view[7]; pe.z += view[11];
  const F3 ne = mat3_mul(M, n);
  const float d = -pe.z;
  const float xn = focal * pe.x / d, yn = focal * pe.y / d;
  F3 s;
  s.x = (xn * 0.5f + 0.5f) * Wf;
  s.y = (0.5f - yn * 0.5f) * Hf;
  s.z = d;
  *(F3*)(screen + t * 3) = s;
  *(F3*)(normals + t * 3) = ne;
}

// ------------------------------------------------------------------------------------------------ raster stage
#define RT_TILE 64                 // pixels per tile side at one sample per pixel; the strip width of the textured pass
#define RT_TILE_MS 32              // pixels per tile side at four samples per pixel: the same 4096 keys
#define RT_THREADS 256
#define RT_CAP 2048                // compacted face ids held in LDS between two coverage passes
#define RT_WAVE_WALK 256           // an in-tile bounding box of more fragments than this is walked by a whole wave
#define RT_SNAP_LIMIT 1073741824.f // 2^30: |snapped coordinate| below it, so every edge function fits 64 bits (see below)
#define RT_EMPTY 0xffffffffffffffffull

// The sample points of a pixel, in 1 / 256 pixel units from its top-left corner (256 j, 256 i).  S = 1: the centre.  S = 4: the
// rotated grid s0 = (96, 32), s1 = (224, 96), s2 = (32, 160), s3 = (160, 224).  Integers on the snap grid, so an edge function
// at a sample is as exact as at the centre and the 2^30 limit below holds unchanged.
template <int S> struct Rt {
  static_assert(S == 1 || S == 4, "one or four samples per pixel");
  static constexpr int tile = S == 1 ? RT_TILE : RT_TILE_MS;
  static constexpr int keys = tile * tile * S;
  static constexpr int walk = RT_WAVE_WALK / S;          // in pixels
  static constexpr int lo = S == 1 ? 128 : 32;           // the least and the greatest sample offset (the same in x and in y)
  static constexpr int hi = S == 1 ? 128 : 224;
  __device__ static constexpr int sx(int k) { return S == 1 ? 128 : k == 0 ? 96 : k == 1 ? 224 : k == 2 ? 32 : 160; }
  __device__ static constexpr int sy(int k) { return S == 1 ? 128 : 32 + 64 * k; }
};

// A face as the coverage and the shading passes see it, from ONE routine, so both compute the same bits.
// Coordinates are snapped to 8 sub-pixel bits (round half even).  With |X|, |Y| < 2^30 a difference is below 2^31, a product
// below 2^62 and an edge function (a difference of two products) below 2^63: exact in int64 for any image size.
struct FaceSetup {
  int x0, y0, x1, y1, x2, y2;   // oriented so that the doubled area is positive (vertices 1 and 2 swapped if it was not)
  int i0, i1, i2;               // vertex ids in that order
  float q0, q1, q2;             // 1 / eye depth
  long area;                    // e0 + e1 + e2 at any point
  int jmin, jmax, imin, imax;   // pixel box inside the tile and the image (empty if min > max)
  bool ok;
};

__device__ __forceinline__ long edge_fn(int ax, int ay, int bx, int by, long px, long py) {
  return (long)(bx - ax) * (py - ay) - (long)(by - ay) * (px - ax);
}
// top-left rule: a zero edge value counts only on an edge whose oriented vector has dy > 0, or dy == 0 and dx > 0
__device__ __forceinline__ long edge_bias(int ax, int ay, int bx, int by) {
  const int dx = bx - ax, dy = by - ay;
  return (dy > 0 || (dy == 0 && dx > 0)) ? 0L : -1L;
}

template <int S>
__device__ __forceinline__ FaceSetup face_setup(const int* __restrict__ faces, const float* __restrict__ scr, int f, int V,
                                                float near, int tx0, int ty0, int tx1, int ty1) {
  FaceSetup s;
  s.ok = false;
  const I3 vi = *(const I3*)(faces + (long)f * 3);
  if ((unsigned)vi.a >= (unsigned)V || (unsigned)vi.b >= (unsigned)V || (unsigned)vi.c >= (unsigned)V) return s;
  const F3 a = *(const F3*)(scr + (long)vi.a * 3), b = *(const F3*)(scr + (long)vi.b * 3), c = *(const F3*)(scr + (long)vi.c * 3);
  if (!(a.z >= near && b.z >= near && c.z >= near)) return s;                 // no clipping: a face behind `near` is dropped
  const float fx0 = rintf(a.x * 256.f), fy0 = rintf(a.y * 256.f), fx1 = rintf(b.x * 256.f), fy1 = rintf(b.y * 256.f),
              fx2 = rintf(c.x * 256.f), fy2 = rintf(c.y * 256.f);
  if (!(fabsf(fx0) < RT_SNAP_LIMIT && fabsf(fy0) < RT_SNAP_LIMIT && fabsf(fx1) < RT_SNAP_LIMIT && fabsf(fy1) < RT_SNAP_LIMIT &&
        fabsf(fx2) < RT_SNAP_LIMIT && fabsf(fy2) < RT_SNAP_LIMIT)) return s;  // also NaN / inf
  s.x0 = (int)fx0; s.y0 = (int)fy0; s.x1 = (int)fx1; s.y1 = (int)fy1; s.x2 = (int)fx2; s.y2 = (int)fy2;
  s.i0 = vi.a; s.i1 = vi.b; s.i2 = vi.c;
  s.q0 = 1.f / a.z; s.q1 = 1.f / b.z; s.q2 = 1.f / c.z;
  s.area = edge_fn(s.x0, s.y0, s.x1, s.y1, s.x2, s.y2);
  if (s.area == 0) return s;
  if (s.area < 0) {
    int t = s.x1; s.x1 = s.x2; s.x2 = t;
    t = s.y1; s.y1 = s.y2; s.y2 = t;
    t = s.i1; s.i1 = s.i2; s.i2 = t;
    const float q = s.q1; s.q1 = s.q2; s.q2 = q;
    s.area = -s.area;
  }
  // pixels that have some sample point inside the snapped bounding box: the centre (256 j + 128) at one sample, so + 127 and
  // - 128; offsets 32 .. 224 at four, so + 31 and - 32 (a sliver that covers no centre can cover a sample)
  const int xmin = min(s.x0, min(s.x1, s.x2)), xmax = max(s.x0, max(s.x1, s.x2));
  const int ymin = min(s.y0, min(s.y1, s.y2)), ymax = max(s.y0, max(s.y1, s.y2));
  s.jmin = max((xmin + 255 - Rt<S>::hi) >> 8, tx0); s.jmax = min((xmax - Rt<S>::lo) >> 8, tx1);
  s.imin = max((ymin + 255 - Rt<S>::hi) >> 8, ty0); s.imax = min((ymax - Rt<S>::lo) >> 8, ty1);
  s.ok = s.jmin <= s.jmax && s.imin <= s.imax;
  return s;
}

// the three edge functions at sample k of pixel (j, i): e0 is opposite vertex 0, and so on
template <int S>
__device__ __forceinline__ void edges_at(const FaceSetup& s, int j, int i, int k, long& e0, long& e1, long& e2) {
  const long px = 256L * j + Rt<S>::sx(k), py = 256L * i + Rt<S>::sy(k);
  e0 = edge_fn(s.x1, s.y1, s.x2, s.y2, px, py);
  e1 = edge_fn(s.x2, s.y2, s.x0, s.y0, px, py);
  e2 = edge_fn(s.x0, s.y0, s.x1, s.y1, px, py);
}
// what the edge function of (a -> b) at sample k of a pixel adds to its value at sample 0 of that pixel: d e / d x = -(by - ay),
// d e / d y = bx - ax per 1 / 256 pixel, exact integers (0 for k = 0, so nothing at one sample)
template <int S>
__device__ __forceinline__ long sample_step(int ax, int ay, int bx, int by, int k) {
  return -(long)(by - ay) * (Rt<S>::sx(k) - Rt<S>::sx(0)) + (long)(bx - ax) * (Rt<S>::sy(k) - Rt<S>::sy(0));
}
// 1 / depth by the integer barycentrics, one fixed order of operations; w_k are returned for the shading pass
__device__ __forceinline__ float inv_depth(const FaceSetup& s, long e0, long e1, long e2, float& w0, float& w1, float& w2) {
  const float A = (float)s.area;
  w0 = (float)e0 / A; w1 = (float)e1 / A; w2 = (float)e2 / A;
  return fmaf(w2, s.q2, fmaf(w1, s.q1, __fmul_rn(w0, s.q0)));
}

// (1 / pi) sum_k I_k max(0, n . l_k) with n the perspective-correct interpolated vertex normal, renormalised: the lighting of
// the untextured and the textured pass, from ONE routine
__device__ __forceinline__ float lambert_diffuse(const float* __restrict__ nrm, const FaceSetup& s, float p0, float p1, float p2,
                                                 const float* __restrict__ lights, int n_lights) {
  const F3 n0 = *(const F3*)(nrm + (long)s.i0 * 3), n1 = *(const F3*)(nrm + (long)s.i1 * 3), n2 = *(const F3*)(nrm + (long)s.i2 * 3);
  const F3 n = unit_or_z(F3{p0 * n0.x + p1 * n1.x + p2 * n2.x, p0 * n0.y + p1 * n1.y + p2 * n2.y, p0 * n0.z + p1 * n1.z + p2 * n2.z});
  float diff = 0.f;
  for (int k = 0; k < n_lights; ++k) {
    const float ndl = n.x * lights[4 * k] + n.y * lights[4 * k + 1] + n.z * lights[4 * k + 2];
    diff += lights[4 * k + 3] * fmaxf(0.f, ndl);
  }
  return diff * 0.318309886183790672f;
}

template <int S>
__device__ __forceinline__ void fragment(const FaceSetup& s, int f, int j, int i, int k, long e0, long e1, long e2, long b0, long b1,
                                         long b2, float near, float far, int tx0, int ty0, unsigned long long* s_key) {
  if ((e0 + b0) < 0 || (e1 + b1) < 0 || (e2 + b2) < 0) return;
  float w0, w1, w2;
  const float d = 1.f / inv_depth(s, e0, e1, e2, w0, w1, w2);
  if (!(d >= near && d <= far)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)f;
  atomicMin(&s_key[((i - ty0) * Rt<S>::tile + (j - tx0)) * S + k], key);     // LDS; min of (depth, face id): independent of arrival order
}

// every sample of pixel (j, i) from the edge values at its sample 0
template <int S>
__device__ __forceinline__ void fragments(const FaceSetup& s, int f, int j, int i, long e0, long e1, long e2, long b0, long b1, long b2,
                                          float near, float far, int tx0, int ty0, unsigned long long* s_key) {
  fragment<S>(s, f, j, i, 0, e0, e1, e2, b0, b1, b2, near, far, tx0, ty0, s_key);
#pragma unroll
  for (int k = 1; k < S; ++k)
    fragment<S>(s, f, j, i, k, e0 + sample_step<S>(s.x1, s.y1, s.x2, s.y2, k), e1 + sample_step<S>(s.x2, s.y2, s.x0, s.y0, k),
                e2 + sample_step<S>(s.x0, s.y0, s.x1, s.y1, k), b0, b1, b2, near, far, tx0, ty0, s_key);
}

// the untextured colour of face `s` at the point whose edge values are e0, e1, e2: R | G << 8 | B << 16 | 255 << 24
__device__ __forceinline__ unsigned shade_flat(const FaceSetup& s, const float* __restrict__ nrm, long e0, long e1, long e2,
                                               const float* __restrict__ lights, int n_lights, float base_r, float base_g,
                                               float base_b, float amb_r, float amb_g, float amb_b) {
  float w0, w1, w2;
  const float iz = inv_depth(s, e0, e1, e2, w0, w1, w2);
  // perspective-correct weights w_k q_k / (sum), then the interpolated normal
  const float p0 = w0 * s.q0 / iz, p1 = w1 * s.q1 / iz, p2 = w2 * s.q2 / iz;
  const float diff = lambert_diffuse(nrm, s, p0, p1, p2, lights, n_lights);
  const float cr = fminf(fmaxf(base_r * (amb_r + diff), 0.f), 1.f), cg = fminf(fmaxf(base_g * (amb_g + diff), 0.f), 1.f),
              cb = fminf(fmaxf(base_b * (amb_b + diff), 0.f), 1.f);
  const unsigned ur = (unsigned)floorf(255.f * cr + 0.5f), ug = (unsigned)floorf(255.f * cg + 0.5f),
                 ub = (unsigned)floorf(255.f * cb + 0.5f);
  return ur | (ug << 8) | (ub << 16) | 0xff000000u;
}

// The resolve of four RGBA words, (b0 + b1 + b2 + b3 + 2) >> 2 in every byte: the even and the odd bytes are summed in 16-bit
// lanes (a sum is at most 4 * 255 + 2), which start at the rounding term.
struct Resolve4 {
  unsigned even = 0x00020002u, odd = 0x00020002u;
  __device__ __forceinline__ void add(unsigned c) { even += c & 0x00ff00ffu; odd += (c >> 8) & 0x00ff00ffu; }
  __device__ __forceinline__ unsigned word() const { return ((even >> 2) & 0x00ff00ffu) | (((odd >> 2) & 0x00ff00ffu) << 8); }
};

// One workgroup per (frame, tile): 64 x 64 pixels at one sample per pixel, 32 x 32 at four, 4096 keys either way.  (A) the
// frame's faces are streamed 256 at a time and those whose snapped box meets the tile are compacted, in face order, into an
// LDS list; (B) whenever the list could overflow, and at the end, the listed faces are rasterised into the tile's 64-bit
// (depth bits, face id) keys, one per sample at [pixel][sample], with one LDS atomicMin per fragment: a lane owns a face and
// walks its box, a face with a large box is queued and walked by a whole wave; the samples of a pixel take their edge values
// from sample 0's by sample_step; (C) the tile is resolved and shaded pixel-parallel: every covered sample at its own
// position, and at four samples the mean of the four (Resolve4), an uncovered sample counting as the background's bytes.
// sample_depth is written at four samples only (at one it is `depth`).
template <int S>
__global__ __launch_bounds__(RT_THREADS) void render_raster_kernel(const float* __restrict__ screen, const float* __restrict__ normals,
                                                                   const int* __restrict__ faces, const float* __restrict__ shade,
                                                                   const float* __restrict__ lights, int n_lights,
                                                                   unsigned* __restrict__ rgba, float* __restrict__ depth,
                                                                   int* __restrict__ face_id, float* __restrict__ sample_depth, int V,
                                                                   int F, int H, int W, int tiles_x, int tiles_y, float near, float far,
                                                                   unsigned bg) {
  constexpr int TILE = Rt<S>::tile;
  __shared__ unsigned long long s_key[Rt<S>::keys];   // 32 KB
  __shared__ int s_list[RT_CAP];
  __shared__ int s_big[RT_CAP];
  __shared__ int s_wcnt[2][RT_THREADS / 64];
  __shared__ int s_nbig;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int tx0 = tx * TILE, ty0 = ty * TILE;
  const int tx1 = min(tx0 + TILE, W) - 1, ty1 = min(ty0 + TILE, H) - 1;
  const float* scr = screen + (long)b * V * 3;
  const float* nrm = normals + (long)b * V * 3;

  for (int p = tid; p < Rt<S>::keys; p += RT_THREADS) s_key[p] = RT_EMPTY;
  if (tid == 0) s_nbig = 0;
  int count = 0;   // uniform: entries of s_list
  int it = 0;
  for (int base = 0; base < F; base += RT_THREADS, ++it) {
    // (A) compaction of faces [base, base + 256) behind the `count` entries already listed
    const int f = base + tid;
    bool keep = false;
    if (f < F) keep = face_setup<S>(faces, scr, f, V, near, tx0, ty0, tx1, ty1).ok;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wcnt[it & 1][wid] = __popcll(m);
    __syncthreads();     // also orders the key initialisation / the previous pass before what follows
    int off = count, total = 0;
#pragma unroll
    for (int w = 0; w < RT_THREADS / 64; ++w) {
      const int c = s_wcnt[it & 1][w];
      if (w < wid) off += c;
      total += c;
    }
    if (keep) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = f;
    count += total;
    if (count + RT_THREADS <= RT_CAP && base + RT_THREADS < F) continue;
    __syncthreads();
    // (B) coverage, face-parallel
    for (int e = tid; e < count; e += RT_THREADS) {
      const int g = s_list[e];
      const FaceSetup s = face_setup<S>(faces, scr, g, V, near, tx0, ty0, tx1, ty1);
      const int bw = s.jmax - s.jmin + 1, bh = s.imax - s.imin + 1;
      if (bw * bh > Rt<S>::walk) {
        s_big[atomicAdd(&s_nbig, 1)] = g;       // the order of this queue does not reach the result (min of keys)
        continue;
      }
      const long b0 = edge_bias(s.x1, s.y1, s.x2, s.y2), b1 = edge_bias(s.x2, s.y2, s.x0, s.y0), b2 = edge_bias(s.x0, s.y0, s.x1, s.y1);
      long r0, r1, r2;
      edges_at<S>(s, s.jmin, s.imin, 0, r0, r1, r2);
      // d e / d j = -256 (by - ay), d e / d i = 256 (bx - ax): exact integer steps
      const long a0 = -256L * (s.y2 - s.y1), a1 = -256L * (s.y0 - s.y2), a2 = -256L * (s.y1 - s.y0);
      const long c0 = 256L * (s.x2 - s.x1), c1 = 256L * (s.x0 - s.x2), c2 = 256L * (s.x1 - s.x0);
      for (int i = s.imin; i <= s.imax; ++i) {
        long e0 = r0, e1 = r1, e2 = r2;
        for (int j = s.jmin; j <= s.jmax; ++j) {
          fragments<S>(s, g, j, i, e0, e1, e2, b0, b1, b2, near, far, tx0, ty0, s_key);
          e0 += a0; e1 += a1; e2 += a2;
        }
        r0 += c0; r1 += c1; r2 += c2;
      }
    }
    __syncthreads();
    const int nbig = s_nbig;
    for (int e = wid; e < nbig; e += RT_THREADS / 64) {
      const int g = s_big[e];
      const FaceSetup s = face_setup<S>(faces, scr, g, V, near, tx0, ty0, tx1, ty1);
      const long b0 = edge_bias(s.x1, s.y1, s.x2, s.y2), b1 = edge_bias(s.x2, s.y2, s.x0, s.y0), b2 = edge_bias(s.x0, s.y0, s.x1, s.y1);
      const int bw = s.jmax - s.jmin + 1, n = bw * (s.imax - s.imin + 1);
      for (int p = lane; p < n; p += 64) {
        const int i = s.imin + p / bw, j = s.jmin + p % bw;
        long e0, e1, e2;
        edges_at<S>(s, j, i, 0, e0, e1, e2);
        fragments<S>(s, g, j, i, e0, e1, e2, b0, b1, b2, near, far, tx0, ty0, s_key);
      }
    }
    __syncthreads();     // before the lists are refilled
    count = 0;
    if (tid == 0) s_nbig = 0;
  }
  __syncthreads();

  // (C) resolve and shade: a wave stores row segments of the tile's width (256 contiguous bytes of RGBA at one sample per
  // pixel, two of 128 at four) per step
  const float base_r = shade[0], base_g = shade[1], base_b = shade[2], amb_r = shade[3], amb_g = shade[4], amb_b = shade[5];
  for (int p = tid; p < TILE * TILE; p += RT_THREADS) {
    const int i = ty0 + p / TILE, j = tx0 + p % TILE;
    if (i > ty1 || j > tx1) continue;
    const long o = ((long)b * H + i) * W + j;
    if constexpr (S == 1) {
      const unsigned long long key = s_key[p];
      if (key == RT_EMPTY) {
        rgba[o] = bg;
        depth[o] = 0.f;
        if (face_id != nullptr) face_id[o] = -1;
        continue;
      }
      const int g = (int)(unsigned)(key & 0xffffffffull);
      const FaceSetup s = face_setup<S>(faces, scr, g, V, near, tx0, ty0, tx1, ty1);
      long e0, e1, e2;
      edges_at<S>(s, j, i, 0, e0, e1, e2);
      rgba[o] = shade_flat(s, nrm, e0, e1, e2, lights, n_lights, base_r, base_g, base_b, amb_r, amb_g, amb_b);
      depth[o] = __uint_as_float((unsigned)(key >> 32));
      if (face_id != nullptr) face_id[o] = g;
    } else {
      Resolve4 sum;
      unsigned dmin = 0xffffffffu;      // depths are positive, so their bits order as they do
      int ids[S];
      float ds[S];
      int last = -1;                    // the set-up is kept while consecutive samples show the same face
      FaceSetup s;
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const unsigned long long key = s_key[p * S + k];
        unsigned c = bg;
        ids[k] = -1;
        ds[k] = 0.f;
        if (key != RT_EMPTY) {
          const int g = (int)(unsigned)(key & 0xffffffffull);
          if (g != last) {
            s = face_setup<S>(faces, scr, g, V, near, tx0, ty0, tx1, ty1);
            last = g;
          }
          long e0, e1, e2;
          edges_at<S>(s, j, i, k, e0, e1, e2);
          c = shade_flat(s, nrm, e0, e1, e2, lights, n_lights, base_r, base_g, base_b, amb_r, amb_g, amb_b);
          ids[k] = g;
          ds[k] = __uint_as_float((unsigned)(key >> 32));
          dmin = min(dmin, (unsigned)(key >> 32));
        }
        sum.add(c);
      }
      rgba[o] = sum.word();
      depth[o] = dmin == 0xffffffffu ? 0.f : __uint_as_float(dmin);
      if (face_id != nullptr) *(int4*)(face_id + o * 4) = make_int4(ids[0], ids[1], ids[2], ids[3]);
      if (sample_depth != nullptr) *(float4*)(sample_depth + o * 4) = make_float4(ds[0], ds[1], ds[2], ds[3]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ texture
#define TX_MAX_SIDE MSMD_TEXTURE_MAX_SIDE
#define TX_MAX_LEVELS 13           // 1 + log2(4096)
#define TX_ROWS 16                 // rows of a 64-pixel-wide strip per workgroup: a wave stores one row segment per step
#define TX_THREADS 256

__global__ __launch_bounds__(256) void texture_level0_kernel(const unsigned char* __restrict__ img, float4* __restrict__ out, int n,
                                                             int channels) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const unsigned char* p = img + (long)t * channels;
  out[t] = make_float4((float)p[0], (float)p[1], (float)p[2], 0.f);
}

// level l + 1 from level l as it is stored: ((a + b) + (c + d)) * 0.25f, the right / lower neighbour clamped to the level
__global__ __launch_bounds__(256) void texture_reduce_kernel(const float4* __restrict__ src, float4* __restrict__ dst, int Hs, int Ws,
                                                             int Hd, int Wd) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Hd * Wd) return;
  const int y = t / Wd, x = t - y * Wd;
  const int x0 = 2 * x, x1 = min(2 * x + 1, Ws - 1), y0 = 2 * y, y1 = min(2 * y + 1, Hs - 1);
  const float4 a = src[(long)y0 * Ws + x0], b = src[(long)y0 * Ws + x1], c = src[(long)y1 * Ws + x0], d = src[(long)y1 * Ws + x1];
  dst[t] = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f,
                       ((a.z + b.z) + (c.z + d.z)) * 0.25f, ((a.w + b.w) + (c.w + d.w)) * 0.25f);
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN and +-inf

// GL_REPEAT bilinear tap of one level at U, Vv in [0, 1]: four 16-byte texels
__device__ __forceinline__ F3 texture_bilinear(const float4* __restrict__ lvl, int Wl, int Hl, float U, float Vv) {
  const float x = U * (float)Wl - 0.5f, y = (1.f - Vv) * (float)Hl - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  const float fx = x - xf, fy = y - yf;
  // x0 is in [-1, W_l - 1], so the mathematical modulo is one conditional each; the clamp keeps any other value in the level
  int x0 = (int)xf, y0 = (int)yf;
  if (x0 < 0) x0 += Wl;
  if (y0 < 0) y0 += Hl;
  x0 = min(max(x0, 0), Wl - 1);
  y0 = min(max(y0, 0), Hl - 1);
  const int x1 = x0 + 1 < Wl ? x0 + 1 : 0, y1 = y0 + 1 < Hl ? y0 + 1 : 0;
  const float4 t00 = lvl[y0 * Wl + x0], t10 = lvl[y0 * Wl + x1], t01 = lvl[y1 * Wl + x0], t11 = lvl[y1 * Wl + x1];
  const float gx = 1.f - fx, gy = 1.f - fy;
  return F3{gy * (gx * t00.x + fx * t10.x) + fy * (gx * t01.x + fx * t11.x),
            gy * (gx * t00.y + fx * t10.y) + fy * (gx * t01.y + fx * t11.y),
            gy * (gx * t00.z + fx * t10.z) + fy * (gx * t01.z + fx * t11.z)};
}

// The textured colour of face g (set-up `s`) at the point whose edge values are e0, e1, e2: R | G << 8 | B << 16 | 255 << 24, and
// (u, v, lambda) as sampled.  The level table lvl_off / lvl_w / lvl_h holds the offset, width and height of every level.
struct TexturedArgs {
  const float* nrm; const int* faces; const float* vt; const int* ft; const float4* pyramid; const float* lights;
  const int *lvl_off, *lvl_w, *lvl_h;
  int n_lights, Nt, L;
  float amb_r, amb_g, amb_b, Wtf, Htf, top;
};
__device__ __forceinline__ unsigned shade_textured(const FaceSetup& s, int g, long e0, long e1, long e2, const TexturedArgs& t, F3& uvl) {
  float w0, w1, w2;
  const float iz = inv_depth(s, e0, e1, e2, w0, w1, w2);
  const float p0 = w0 * s.q0 / iz, p1 = w1 * s.q1 / iz, p2 = w2 * s.q2 / iz;
  // per-corner texture coordinates in the face's oriented order: face_setup swapped corners 1 and 2 iff it swapped the ids
  const I3 ti = *(const I3*)(t.ft + (long)g * 3);
  const bool swapped = s.i1 != t.faces[(long)g * 3 + 1];
  const int k0 = ti.a, k1 = swapped ? ti.c : ti.b, k2 = swapped ? ti.b : ti.c;
  float2 t0 = make_float2(0.f, 0.f), t1 = t0, t2 = t0;
  if ((unsigned)k0 < (unsigned)t.Nt) t0 = *(const float2*)(t.vt + (long)k0 * 2);
  if ((unsigned)k1 < (unsigned)t.Nt) t1 = *(const float2*)(t.vt + (long)k1 * 2);
  if ((unsigned)k2 < (unsigned)t.Nt) t2 = *(const float2*)(t.vt + (long)k2 * 2);
  const float u = (p0 * t0.x + p1 * t1.x) + p2 * t2.x, v = (p0 * t0.y + p1 * t1.y) + p2 * t2.y;
  // analytic level of detail: d w_k / d j = a_k / A, d w_k / d i = c_k / A with stage (B)'s integer edge steps
  const float A = (float)s.area;
  const float g0 = s.q0 * ((float)(-256L * (s.y2 - s.y1)) / A), g1 = s.q1 * ((float)(-256L * (s.y0 - s.y2)) / A),
              g2 = s.q2 * ((float)(-256L * (s.y1 - s.y0)) / A);
  const float h0 = s.q0 * ((float)(256L * (s.x2 - s.x1)) / A), h1 = s.q1 * ((float)(256L * (s.x0 - s.x2)) / A),
              h2 = s.q2 * ((float)(256L * (s.x1 - s.x0)) / A);
  const float dDj = (g0 + g1) + g2, dDi = (h0 + h1) + h2;
  const float duj = (((g0 * t0.x + g1 * t1.x) + g2 * t2.x) - u * dDj) / iz, dvj = (((g0 * t0.y + g1 * t1.y) + g2 * t2.y) - v * dDj) / iz;
  const float dui = (((h0 * t0.x + h1 * t1.x) + h2 * t2.x) - u * dDi) / iz, dvi = (((h0 * t0.y + h1 * t1.y) + h2 * t2.y) - v * dDi) / iz;
  const float rj2 = (t.Wtf * duj) * (t.Wtf * duj) + (t.Htf * dvj) * (t.Htf * dvj),
              ri2 = (t.Wtf * dui) * (t.Wtf * dui) + (t.Htf * dvi) * (t.Htf * dvi);
  float lam = 0.5f * log2f(fmaxf(rj2, ri2));
  if (!(finite_f(rj2) && finite_f(ri2) && finite_f(lam))) lam = 0.f;
  lam = fminf(fmaxf(lam, 0.f), t.top);
  const float us = finite_f(u) ? u : 0.f, vs = finite_f(v) ? v : 0.f;
  const float U = us - floorf(us), Vv = vs - floorf(vs);
  const int l0 = min((int)floorf(lam), t.L - 1), l1 = min(l0 + 1, t.L - 1);
  const float fl = lam - (float)l0;
  const F3 c0 = texture_bilinear(t.pyramid + t.lvl_off[l0], t.lvl_w[l0], t.lvl_h[l0], U, Vv);
  const F3 c1 = texture_bilinear(t.pyramid + t.lvl_off[l1], t.lvl_w[l1], t.lvl_h[l1], U, Vv);
  const float gl = 1.f - fl;
  const float Tr = gl * c0.x + fl * c1.x, Tg = gl * c0.y + fl * c1.y, Tb = gl * c0.z + fl * c1.z;
  const float diff = lambert_diffuse(t.nrm, s, p0, p1, p2, t.lights, t.n_lights);
  const float cr = fminf(fmaxf((Tr / 255.f) * (t.amb_r + diff), 0.f), 1.f), cg = fminf(fmaxf((Tg / 255.f) * (t.amb_g + diff), 0.f), 1.f),
              cb = fminf(fmaxf((Tb / 255.f) * (t.amb_b + diff), 0.f), 1.f);
  const unsigned ur = (unsigned)floorf(255.f * cr + 0.5f), ug = (unsigned)floorf(255.f * cg + 0.5f),
                 ub = (unsigned)floorf(255.f * cb + 0.5f);
  uvl = F3{us, vs, lam};
  return ur | (ug << 8) | (ub << 16) | 0xff000000u;
}

// One workgroup per (frame, 64 x 16 strip); pixel-parallel in stage (C)'s mapping, so a wave reads 64 contiguous face ids (at
// four samples per pixel 64 contiguous int4) and stores 256 contiguous bytes of RGBA per step.  The face's set-up, the
// barycentrics and the lighting are the routines of the raster pass; the level table is built once per workgroup in LDS.
// At four samples face_id is (B, H, W, 4): every sample with 0 <= id < F is shaded at its own position, any other counts as
// `bg`, and a pixel with a shaded sample receives the mean of the four (Resolve4); uvl is not offered.
template <int S>
__global__ __launch_bounds__(TX_THREADS) void render_shade_textured_kernel(
    const float* __restrict__ screen, const float* __restrict__ normals, const int* __restrict__ faces, const float* __restrict__ vt,
    const int* __restrict__ ft, const float4* __restrict__ pyramid, const float* __restrict__ shade, const float* __restrict__ lights,
    int n_lights, const int* __restrict__ face_id, unsigned* __restrict__ rgba, float* __restrict__ uvl, int V, int F, int Nt,
    int Ht, int Wt, int L, int H, int W, int tiles_x, int strips_y, float near, unsigned bg) {
  __shared__ int s_off[TX_MAX_LEVELS], s_w[TX_MAX_LEVELS], s_h[TX_MAX_LEVELS];
  const int tid = threadIdx.x;
  if (tid < L) {
    int off = 0, w = Wt, h = Ht;
    for (int l = 0; l < tid; ++l) {
      off += w * h;
      w = max(1, w >> 1);
      h = max(1, h >> 1);
    }
    s_off[tid] = off; s_w[tid] = w; s_h[tid] = h;
  }
  __syncthreads();
  const int per_frame = tiles_x * strips_y;
  const int b = blockIdx.x / per_frame, rest = blockIdx.x - b * per_frame;
  const int sy = rest / tiles_x, tx = rest - sy * tiles_x;
  const int tx0 = tx * RT_TILE, ty0 = sy * TX_ROWS;
  const float* scr = screen + (long)b * V * 3;
  TexturedArgs t;
  t.nrm = normals + (long)b * V * 3; t.faces = faces; t.vt = vt; t.ft = ft; t.pyramid = pyramid; t.lights = lights;
  t.lvl_off = s_off; t.lvl_w = s_w; t.lvl_h = s_h;
  t.n_lights = n_lights; t.Nt = Nt; t.L = L;
  t.amb_r = shade[3]; t.amb_g = shade[4]; t.amb_b = shade[5];
  t.Wtf = (float)Wt; t.Htf = (float)Ht; t.top = (float)(L - 1);
  for (int p = tid; p < RT_TILE * TX_ROWS; p += TX_THREADS) {
    const int i = ty0 + p / RT_TILE, j = tx0 + p % RT_TILE;
    if (i >= H || j >= W) continue;
    const long o = ((long)b * H + i) * W + j;
    if constexpr (S == 1) {
      const int g = face_id[o];
      FaceSetup s;
      s.ok = false;
      if ((unsigned)g < (unsigned)F) s = face_setup<S>(faces, scr, g, V, near, 0, 0, W - 1, H - 1);
      if (!s.ok) {                      // background, or a face id the raster pass cannot have written
        if (uvl != nullptr) *(F3*)(uvl + o * 3) = F3{0.f, 0.f, 0.f};
        continue;
      }
      long e0, e1, e2;
      edges_at<S>(s, j, i, 0, e0, e1, e2);
      F3 sampled;
      rgba[o] = shade_textured(s, g, e0, e1, e2, t, sampled);
      if (uvl != nullptr) *(F3*)(uvl + o * 3) = sampled;
    } else {
      const int4 id4 = *(const int4*)(face_id + o * 4);
      const int ids[4] = {id4.x, id4.y, id4.z, id4.w};
      Resolve4 sum;
      bool any = false;
      int last = -1;                    // the set-up is kept while consecutive samples show the same face
      FaceSetup s;
      s.ok = false;
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const int g = ids[k];
        unsigned c = bg;
        if ((unsigned)g < (unsigned)F) {
          if (g != last) {
            s = face_setup<S>(faces, scr, g, V, near, 0, 0, W - 1, H - 1);
            last = g;
          }
          if (s.ok) {
            long e0, e1, e2;
            edges_at<S>(s, j, i, k, e0, e1, e2);
            F3 sampled;
            c = shade_textured(s, g, e0, e1, e2, t, sampled);
            any = true;
          }
        }
        sum.add(c);
      }
      if (any) rgba[o] = sum.word();
    }
  }
}

// ------------------------------------------------------------------------------------------------ vertex colours
// The colour of face `s` at the point whose edge values are e0, e1, e2 from the RGBA bytes at its three vertices (alpha not read):
// per channel C = (p0 c0 + p1 c1) + p2 c2 with the perspective-correct weights of the textured pass, the corners in the order
// face_setup left them in (s.i0, s.i1, s.i2: the face and its colours swap together); then clamp((C / 255)(ambient + diffuse), 0, 1)
// under the raster pass's lighting, or clamp(C / 255, 0, 1) unlit; floor(255 c + 0.5), alpha 255.
struct VertexColorArgs {
  const float* nrm; const unsigned* vcol; const float* lights;
  int n_lights, lit;
  float amb_r, amb_g, amb_b;
};
__device__ __forceinline__ unsigned shade_vertex_color(const FaceSetup& s, long e0, long e1, long e2, const VertexColorArgs& t) {
  float w0, w1, w2;
  const float iz = inv_depth(s, e0, e1, e2, w0, w1, w2);
  const float p0 = w0 * s.q0 / iz, p1 = w1 * s.q1 / iz, p2 = w2 * s.q2 / iz;
  const unsigned c0 = t.vcol[s.i0], c1 = t.vcol[s.i1], c2 = t.vcol[s.i2];
  const float Cr = (p0 * (float)(c0 & 255u) + p1 * (float)(c1 & 255u)) + p2 * (float)(c2 & 255u);
  const float Cg = (p0 * (float)((c0 >> 8) & 255u) + p1 * (float)((c1 >> 8) & 255u)) + p2 * (float)((c2 >> 8) & 255u);
  const float Cb = (p0 * (float)((c0 >> 16) & 255u) + p1 * (float)((c1 >> 16) & 255u)) + p2 * (float)((c2 >> 16) & 255u);
  float cr = Cr / 255.f, cg = Cg / 255.f, cb = Cb / 255.f;
  if (t.lit) {
    const float diff = lambert_diffuse(t.nrm, s, p0, p1, p2, t.lights, t.n_lights);
    cr *= t.amb_r + diff; cg *= t.amb_g + diff; cb *= t.amb_b + diff;
  }
  cr = fminf(fmaxf(cr, 0.f), 1.f); cg = fminf(fmaxf(cg, 0.f), 1.f); cb = fminf(fmaxf(cb, 0.f), 1.f);
  const unsigned ur = (unsigned)floorf(255.f * cr + 0.5f), ug = (unsigned)floorf(255.f * cg + 0.5f),
                 ub = (unsigned)floorf(255.f * cb + 0.5f);
  return ur | (ug << 8) | (ub << 16) | 0xff000000u;
}

// The textured pass's launch shape and mapping: one workgroup per (frame, 64 x 16 strip), pixel-parallel, a wave reads 64 contiguous
// face ids (int4 at four samples) and stores 256 contiguous bytes per step; the three colour gathers per shaded point are 4-byte
// loads from a (V, 4) table that stays in L2.  vcol is the frame's table, or the one shared table (col_stride = 0).
template <int S>
__global__ __launch_bounds__(TX_THREADS) void render_shade_vertex_color_kernel(
    const float* __restrict__ screen, const float* __restrict__ normals, const int* __restrict__ faces, const unsigned* __restrict__ vcol,
    long col_stride, int lit, const float* __restrict__ shade, const float* __restrict__ lights, int n_lights,
    const int* __restrict__ face_id, unsigned* __restrict__ rgba, int V, int F, int H, int W, int tiles_x, int strips_y, float near,
    unsigned bg) {
  const int tid = threadIdx.x;
  const int per_frame = tiles_x * strips_y;
  const int b = blockIdx.x / per_frame, rest = blockIdx.x - b * per_frame;
  const int sy = rest / tiles_x, tx = rest - sy * tiles_x;
  const int tx0 = tx * RT_TILE, ty0 = sy * TX_ROWS;
  const float* scr = screen + (long)b * V * 3;
  VertexColorArgs t;
  t.nrm = normals + (long)b * V * 3; t.vcol = vcol + (long)b * col_stride; t.lights = lights;
  t.n_lights = n_lights; t.lit = lit;
  t.amb_r = shade[3]; t.amb_g = shade[4]; t.amb_b = shade[5];
  for (int p = tid; p < RT_TILE * TX_ROWS; p += TX_THREADS) {
    const int i = ty0 + p / RT_TILE, j = tx0 + p % RT_TILE;
    if (i >= H || j >= W) continue;
    const long o = ((long)b * H + i) * W + j;
    if constexpr (S == 1) {
      const int g = face_id[o];
      if ((unsigned)g >= (unsigned)F) continue;          // background, or a face id the raster pass cannot have written
      const FaceSetup s = face_setup<S>(faces, scr, g, V, near, 0, 0, W - 1, H - 1);
      if (!s.ok) continue;
      long e0, e1, e2;
      edges_at<S>(s, j, i, 0, e0, e1, e2);
      rgba[o] = shade_vertex_color(s, e0, e1, e2, t);
    } else {
      const int4 id4 = *(const int4*)(face_id + o * 4);
      const int ids[4] = {id4.x, id4.y, id4.z, id4.w};
      Resolve4 sum;
      bool any = false;
      int last = -1;                    // the set-up is kept while consecutive samples show the same face
      FaceSetup s;
      s.ok = false;
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const int g = ids[k];
        unsigned c = bg;
        if ((unsigned)g < (unsigned)F) {
          if (g != last) {
            s = face_setup<S>(faces, scr, g, V, near, 0, 0, W - 1, H - 1);
            last = g;
          }
          if (s.ok) {
            long e0, e1, e2;
            edges_at<S>(s, j, i, k, e0, e1, e2);
            c = shade_vertex_color(s, e0, e1, e2, t);
            any = true;
          }
        }
        sum.add(c);
      }
      if (any) rgba[o] = sum.word();
    }
  }
}

}  // namespace

extern "C" long msmd_texture_texels(int Ht, int Wt) {
  if (Ht < 1 || Wt < 1 || Ht > TX_MAX_SIDE || Wt > TX_MAX_SIDE) return -1;
  long n = 0;
  for (int h = Ht, w = Wt;; h = h > 1 ? h >> 1 : 1, w = w > 1 ? w >> 1 : 1) {
    n += (long)h * w;
    if (h == 1 && w == 1) break;
  }
  return n;
}

extern "C" int msmd_texture_mips(const void* img, int Ht, int Wt, int channels, float* pyramid, msmd_stream_t stream) {
  if (msmd_texture_texels(Ht, Wt) < 0 || (channels != 3 && channels != 4)) return 1;
  float4* level = (float4*)pyramid;
  int h = Ht, w = Wt;
  hipLaunchKernelGGL(texture_level0_kernel, dim3((unsigned)((h * w + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)img, level, h * w, channels);
  while (h > 1 || w > 1) {
    const int hd = h > 1 ? h >> 1 : 1, wd = w > 1 ? w >> 1 : 1;
    float4* next = level + (long)h * w;
    hipLaunchKernelGGL(texture_reduce_kernel, dim3((unsigned)((hd * wd + 255) / 256)), dim3(256), 0, (hipStream_t)stream, level, next,
                       h, w, hd, wd);
    level = next; h = hd; w = wd;
  }
  MSMD_RETURN_LAST();
}

namespace {
template <int S>
int launch_shade_textured(const float* screen, const float* normals, const int* faces, const float* vt, const int* ft,
                          const float* pyramid, int Ht, int Wt, const float* shade, const float* lights, int n_lights,
                          const int* face_id, void* rgba, float* uvl, int B, int V, int F, int Nt, int H, int W, float near,
                          unsigned background, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || F <= 0 || Nt <= 0 || H <= 0 || W <= 0 || n_lights < 0 || !(near > 0.f) || face_id == nullptr ||
      msmd_texture_texels(Ht, Wt) < 0) return 1;
  if (S == 4 && ((size_t)face_id & 15) != 0) return 1;      // read as int4
  int L = 1;
  for (int m = Ht > Wt ? Ht : Wt; m > 1; m >>= 1) ++L;
  const int tiles_x = (W + RT_TILE - 1) / RT_TILE, strips_y = (H + TX_ROWS - 1) / TX_ROWS;
  const long grid = (long)B * tiles_x * strips_y;
  if (grid > 2147483647L) return 1;
  hipLaunchKernelGGL(render_shade_textured_kernel<S>, dim3((unsigned)grid), dim3(TX_THREADS), 0, (hipStream_t)stream, screen, normals,
                     faces, vt, ft, (const float4*)pyramid, shade, lights, n_lights, face_id, (unsigned*)rgba, uvl, V, F, Nt, Ht, Wt, L,
                     H, W, tiles_x, strips_y, near, background);
  MSMD_RETURN_LAST();
}
}  // namespace

extern "C" int msmd_render_shade_textured(const float* screen, const float* normals, const int* faces, const float* vt, const int* ft,
                                          const float* pyramid, int Ht, int Wt, const float* shade, const float* lights,
                                          int n_lights, const int* face_id, void* rgba, float* uvl, int B, int V, int F, int Nt,
                                          int H, int W, float near, msmd_stream_t stream) {
  return launch_shade_textured<1>(screen, normals, faces, vt, ft, pyramid, Ht, Wt, shade, lights, n_lights, face_id, rgba, uvl, B, V, F,
                                  Nt, H, W, near, 0u, stream);
}

extern "C" int msmd_render_shade_textured_ms(const float* screen, const float* normals, const int* faces, const float* vt,
                                             const int* ft, const float* pyramid, int Ht, int Wt, const float* shade,
                                             const float* lights, int n_lights, const int* sample_face_id, void* rgba, int B, int V,
                                             int F, int Nt, int H, int W, float near, unsigned background, int samples,
                                             msmd_stream_t stream) {
  if (samples == 1)
    return launch_shade_textured<1>(screen, normals, faces, vt, ft, pyramid, Ht, Wt, shade, lights, n_lights, sample_face_id, rgba,
                                    nullptr, B, V, F, Nt, H, W, near, background, stream);
  if (samples != 4) return 1;
  return launch_shade_textured<4>(screen, normals, faces, vt, ft, pyramid, Ht, Wt, shade, lights, n_lights, sample_face_id, rgba,
                                  nullptr, B, V, F, Nt, H, W, near, background, stream);
}

namespace {
template <int S>
int launch_shade_vertex_color(const float* screen, const float* normals, const int* faces, const unsigned char* vcol, int color_per_frame,
                              int lit, const float* shade, const float* lights, int n_lights, const int* face_id, void* rgba, int B,
                              int V, int F, int H, int W, float near, unsigned background, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0 || n_lights < 0 || !(near > 0.f) || face_id == nullptr || vcol == nullptr ||
      ((size_t)vcol & 3) != 0) return 1;                    // a vertex's four bytes are read as one word
  if (S == 4 && ((size_t)face_id & 15) != 0) return 1;      // read as int4
  const int tiles_x = (W + RT_TILE - 1) / RT_TILE, strips_y = (H + TX_ROWS - 1) / TX_ROWS;
  const long grid = (long)B * tiles_x * strips_y;
  if (grid > 2147483647L) return 1;
  hipLaunchKernelGGL(render_shade_vertex_color_kernel<S>, dim3((unsigned)grid), dim3(TX_THREADS), 0, (hipStream_t)stream, screen,
                     normals, faces, (const unsigned*)vcol, color_per_frame ? (long)V : 0L, lit != 0, shade, lights, n_lights, face_id,
                     (unsigned*)rgba, V, F, H, W, tiles_x, strips_y, near, background);
  MSMD_RETURN_LAST();
}
}  // namespace

extern "C" int msmd_render_shade_vertex_color(const float* screen, const float* normals, const int* faces, const unsigned char* vcol,
                                              int color_per_frame, int lit, const float* shade, const float* lights, int n_lights,
                                              const int* sample_face_id, void* rgba, int B, int V, int F, int H, int W, float near,
                                              unsigned background, int samples, msmd_stream_t stream) {
  if (samples == 1)
    return launch_shade_vertex_color<1>(screen, normals, faces, vcol, color_per_frame, lit, shade, lights, n_lights, sample_face_id, rgba,
                                        B, V, F, H, W, near, background, stream);
  if (samples != 4) return 1;
  return launch_shade_vertex_color<4>(screen, normals, faces, vcol, color_per_frame, lit, shade, lights, n_lights, sample_face_id, rgba,
                                      B, V, F, H, W, near, background, stream);
}

extern "C" int msmd_render_vertices(const float* verts, const int* faces, const int* csr_offsets, const int* csr_faces,
                                    const float* view, const float* t_center, const float* rot, float* screen,
                                    float* normals, int B, int V, int F, float focal, int H, int W, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0 || (rot != nullptr && t_center == nullptr)) return 1;
  const long n = (long)B * V;
  if ((n + 255) / 256 > 2147483647L) return 1;
  hipLaunchKernelGGL(render_vertices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, faces,
                     csr_offsets, csr_faces, view, t_center, rot, screen, normals, B, V, F, focal, (float)W, (float)H);
  MSMD_RETURN_LAST();
}

namespace {
template <int S>
int launch_raster(const float* screen, const float* normals, const int* faces, const float* shade, const float* lights, int n_lights,
                  void* rgba, float* depth, int* face_id, float* sample_depth, int B, int V, int F, int H, int W, float near, float far,
                  unsigned background, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0 || n_lights < 0 || !(near > 0.f) || !(far >= near)) return 1;
  if (S == 4 && ((((size_t)face_id) | ((size_t)sample_depth)) & 15) != 0) return 1;      // stored as int4 / float4
  const int tiles_x = (W + Rt<S>::tile - 1) / Rt<S>::tile, tiles_y = (H + Rt<S>::tile - 1) / Rt<S>::tile;
  const long grid = (long)B * tiles_x * tiles_y;
  if (grid > 2147483647L) return 1;
  hipLaunchKernelGGL(render_raster_kernel<S>, dim3((unsigned)grid), dim3(RT_THREADS), 0, (hipStream_t)stream, screen, normals, faces,
                     shade, lights, n_lights, (unsigned*)rgba, depth, face_id, sample_depth, V, F, H, W, tiles_x, tiles_y, near, far,
                     background);
  MSMD_RETURN_LAST();
}
}  // namespace

extern "C" int msmd_render_raster(const float* screen, const float* normals, const int* faces, const float* shade,
                                  const float* lights, int n_lights, void* rgba, float* depth, int* face_id, int B, int V,
                                  int F, int H, int W, float near, float far, unsigned background, msmd_stream_t stream) {
  return launch_raster<1>(screen, normals, faces, shade, lights, n_lights, rgba, depth, face_id, nullptr, B, V, F, H, W, near, far,
                          background, stream);
}

extern "C" int msmd_render_raster_ms(const float* screen, const float* normals, const int* faces, const float* shade,
                                     const float* lights, int n_lights, void* rgba, float* depth, int* sample_face_id,
                                     float* sample_depth, int B, int V, int F, int H, int W, float near, float far,
                                     unsigned background, int samples, msmd_stream_t stream) {
  if (samples != 1 && samples != 4) return 1;
  if (samples == 4)
    return launch_raster<4>(screen, normals, faces, shade, lights, n_lights, rgba, depth, sample_face_id, sample_depth, B, V, F, H, W,
                            near, far, background, stream);
  const int rc = msmd_render_raster(screen, normals, faces, shade, lights, n_lights, rgba, depth, sample_face_id, B, V, F, H, W, near,
                                    far, background, stream);
  if (rc != 0 || sample_depth == nullptr) return rc;
  // one sample per pixel: the sample's depth is the pixel's
  return (int)hipMemcpyAsync(sample_depth, depth, (size_t)B * H * W * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
}
