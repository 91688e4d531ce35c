// Compute mesh renderer: vertex normals + camera, then a z-buffered tile rasteriser with Lambert shading.
// An Instinct card has no graphics pipe; this turns the (B, V, 3) vertices msmd_lbs_skin_v2 leaves on the device into images
// there.  Two launches per batch of frames, no host synchronisation, no global atomics, bit-identical from run to run.
// A texture adds a mip pyramid (built once per image) and a third, deferred launch that shades the covered pixels from it
// (DESIGN.md 5.14); per-vertex colours, lit or unlit, are that deferred launch with another shader.  The raster
// and the deferred kernel are templates on the samples per pixel: one, or four for anti-aliased frames.
// What the passes must agree on bit for bit is written once: the face's set-up with its edge steps and biases,
// the barycentrics at a point, the lighting, the colour's bytes and the per-pixel resolve; a pass adds its shader.
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

__device__ __forceinline__ long edge_fn(int ax, int ay, int bx, int by, long px, long py) {
  return (long)(bx - ax) * (py - ay) - (long)(by - ay) * (px - ax);
}
// top-left rule: a zero edge value counts only on an edge whose oriented vector has dy > 0, or dy == 0 and dx > 0
__device__ __forceinline__ long edge_bias(int ax, int ay, int bx, int by) {
  const int dx = bx - ax, dy = by - ay;
  return (dy > 0 || (dy == 0 && dx > 0)) ? 0L : -1L;
}

// A face as the coverage and the shading passes see it, from ONE routine, so both compute the same bits.
// Coordinates are snapped to 8 sub-pixel bits (round half even).  With |X|, |Y| < 2^30 a difference is below 2^31, a product
// below 2^62 and an edge function (a difference of two products) below 2^63: exact in int64 for any image size.
struct EdgeSteps { long a0, a1, a2, c0, c1, c2; };
struct EdgeBias { long b0, b1, b2; };
struct FaceSetup {
  int x0, y0, x1, y1, x2, y2;   // oriented so that the doubled area is positive (vertices 1 and 2 swapped if it was not)
  int i0, i1, i2;               // vertex ids in that order
  float q0, q1, q2;             // 1 / eye depth
  long area;                    // e0 + e1 + e2 at any point
  int jmin, jmax, imin, imax;   // pixel box inside the given bounds (empty if min > max)
  bool ok;
  // what one pixel to the right (a_k) and one pixel down (c_k) add to edge function k, the one opposite vertex k:
  // d e / d j = -256 (by - ay), d e / d i = 256 (bx - ax), exact integers.  The coverage walk steps by them and the level of
  // detail differentiates the barycentrics with them.
  __device__ __forceinline__ EdgeSteps steps() const {
    return EdgeSteps{-256L * (y2 - y1), -256L * (y0 - y2), -256L * (y1 - y0), 256L * (x2 - x1), 256L * (x0 - x2), 256L * (x1 - x0)};
  }
  __device__ __forceinline__ EdgeBias biases() const {
    return EdgeBias{edge_bias(x1, y1, x2, y2), edge_bias(x2, y2, x0, y0), edge_bias(x0, y0, x1, y1)};
  }
};

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

// The barycentrics of face `s` at the point whose edge values are e0, e1, e2, as every shader takes them: the screen-space
// weights w_k, iz = 1 / depth and the perspective-correct weights p_k = w_k q_k / iz.  (Coverage needs the depth alone: inv_depth.)
struct Bary { float w0, w1, w2, iz, p0, p1, p2; };
__device__ __forceinline__ Bary barycentrics(const FaceSetup& s, long e0, long e1, long e2) {
  Bary b;
  b.iz = inv_depth(s, e0, e1, e2, b.w0, b.w1, b.w2);
  b.p0 = b.w0 * s.q0 / b.iz; b.p1 = b.w1 * s.q1 / b.iz; b.p2 = b.w2 * s.q2 / b.iz;
  return b;
}

// (1 / pi) sum_k I_k max(0, n . l_k) with n the perspective-correct interpolated vertex normal, renormalised: the lighting of
// every pass
__device__ __forceinline__ float lambert_diffuse(const float* __restrict__ nrm, const FaceSetup& s, const Bary& b,
                                                 const float* __restrict__ lights, int n_lights) {
  const float p0 = b.p0, p1 = b.p1, p2 = b.p2;
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
__device__ __forceinline__ void fragment(const FaceSetup& s, int f, int j, int i, int k, long e0, long e1, long e2, const EdgeBias& bias,
                                         float near, float far, int tx0, int ty0, unsigned long long* s_key) {
  if ((e0 + bias.b0) < 0 || (e1 + bias.b1) < 0 || (e2 + bias.b2) < 0) return;
  float w0, w1, w2;
  const float d = 1.f / inv_depth(s, e0, e1, e2, w0, w1, w2);
  if (!(d >= near && d <= far)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)f;
  atomicMin(&s_key[((i - ty0) * Rt<S>::tile + (j - tx0)) * S + k], key);     // LDS; min of (depth, face id): independent of arrival order
}

// every sample of pixel (j, i) from the edge values at its sample 0
template <int S>
__device__ __forceinline__ void fragments(const FaceSetup& s, int f, int j, int i, long e0, long e1, long e2, const EdgeBias& bias,
                                          float near, float far, int tx0, int ty0, unsigned long long* s_key) {
  fragment<S>(s, f, j, i, 0, e0, e1, e2, bias, near, far, tx0, ty0, s_key);
#pragma unroll
  for (int k = 1; k < S; ++k)
    fragment<S>(s, f, j, i, k, e0 + sample_step<S>(s.x1, s.y1, s.x2, s.y2, k), e1 + sample_step<S>(s.x2, s.y2, s.x0, s.y0, k),
                e2 + sample_step<S>(s.x0, s.y0, s.x1, s.y1, k), bias, near, far, tx0, ty0, s_key);
}

// The bytes of a colour, R | G << 8 | B << 16 | 255 << 24: clamp(albedo (ambient + diffuse), 0, 1) per channel under the lighting,
// clamp(albedo, 0, 1) unlit, then floor(255 c + 0.5).  The albedo is the base colour, a texel / 255 or a vertex colour / 255;
// diffuse() is called for the diffuse term under the lighting only.
template <class Diffuse>
__device__ __forceinline__ unsigned color_bytes(F3 c, bool lit, const F3 amb, Diffuse diffuse) {
  if (lit) {
    const float diff = diffuse();
    c.x *= amb.x + diff; c.y *= amb.y + diff; c.z *= amb.z + diff;
  }
  const auto byte = [](float x) { return (unsigned)floorf(255.f * fminf(fmaxf(x, 0.f), 1.f) + 0.5f); };
  return byte(c.x) | (byte(c.y) << 8) | (byte(c.z) << 16) | 0xff000000u;
}

// A shader is called with a face's set-up, its id and the barycentrics at a point and returns the colour word there; `sampled` is
// what it looked up on the way, (u, v, lambda) for the textured one, and is left alone by the others.
// The untextured one: the base colour under the lighting.
struct FlatShade {
  const float* nrm; const float* lights;
  int n_lights;
  F3 base, amb;
  __device__ __forceinline__ unsigned operator()(const FaceSetup& s, int, const Bary& b, F3&) const {
    return color_bytes(base, true, amb, [&] { return lambert_diffuse(nrm, s, b, lights, n_lights); });
  }
};

// The resolve of four RGBA words, (b0 + b1 + b2 + b3 + 2) >> 2 in every byte: the even and the odd bytes are summed in 16-bit
// lanes (a sum is at most 4 * 255 + 2), which start at the rounding term.
struct Resolve4 {
  unsigned even = 0x00020002u, odd = 0x00020002u;
  __device__ __forceinline__ void add(unsigned c) { even += c & 0x00ff00ffu; odd += (c >> 8) & 0x00ff00ffu; }
  __device__ __forceinline__ unsigned word() const { return ((even >> 2) & 0x00ff00ffu) | (((odd >> 2) & 0x00ff00ffu) << 8); }
};

// Pixel (j, i) from the face ids of its S samples: a sample with 0 <= id < F whose face the set-up accepts is shaded at its own
// position, any other counts as `bg`; `word` is the one colour at one sample and the mean of the four (Resolve4) at four.
// -> whether a sample was shaded.  (bx0, by0, bx1, by1) go to the set-up, the tile in the raster pass and the image in a deferred
// one: they bound its pixel box and decide `ok`; nothing else of them reaches the colour.  Own: the ids are this launch's own
// coverage (stage (C)), -1 or a face whose set-up was accepted in these bounds, so neither is tested again.
template <int S, bool Own, class Shade>
__device__ __forceinline__ bool resolve_pixel(const Shade& shade, const int (&ids)[S], const int* __restrict__ faces,
                                              const float* __restrict__ scr, int V, int F, float near, int bx0, int by0, int bx1,
                                              int by1, int j, int i, unsigned bg, unsigned& word, F3& sampled) {
  Resolve4 sum;
  bool any = false;
  int last = -1;                    // the set-up is kept while consecutive samples show the same face
  FaceSetup s;
  s.ok = false;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const int g = ids[k];
    unsigned c = bg;
    const bool valid = Own ? g >= 0 : (unsigned)g < (unsigned)F;
    if (valid && g != last) {
      s = face_setup<S>(faces, scr, g, V, near, bx0, by0, bx1, by1);
      last = g;
    }
    if (valid && (Own || s.ok)) {
      long e0, e1, e2;
      edges_at<S>(s, j, i, k, e0, e1, e2);
      c = shade(s, g, barycentrics(s, e0, e1, e2), sampled);
      any = true;
    }
    sum.add(c);
    word = c;
  }
  if (S == 4) word = sum.word();
  return any;
}

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
      const EdgeBias bias = s.biases();
      const EdgeSteps d = s.steps();
      long r0, r1, r2;
      edges_at<S>(s, s.jmin, s.imin, 0, r0, r1, r2);
      for (int i = s.imin; i <= s.imax; ++i) {
        long e0 = r0, e1 = r1, e2 = r2;
        for (int j = s.jmin; j <= s.jmax; ++j) {
          fragments<S>(s, g, j, i, e0, e1, e2, bias, near, far, tx0, ty0, s_key);
          e0 += d.a0; e1 += d.a1; e2 += d.a2;
        }
        r0 += d.c0; r1 += d.c1; r2 += d.c2;
      }
    }
    __syncthreads();
    const int nbig = s_nbig;
    for (int e = wid; e < nbig; e += RT_THREADS / 64) {
      const int g = s_big[e];
      const FaceSetup s = face_setup<S>(faces, scr, g, V, near, tx0, ty0, tx1, ty1);
      const EdgeBias bias = s.biases();
      const int bw = s.jmax - s.jmin + 1, n = bw * (s.imax - s.imin + 1);
      for (int p = lane; p < n; p += 64) {
        const int i = s.imin + p / bw, j = s.jmin + p % bw;
        long e0, e1, e2;
        edges_at<S>(s, j, i, 0, e0, e1, e2);
        fragments<S>(s, g, j, i, e0, e1, e2, bias, near, far, tx0, ty0, s_key);
      }
    }
    __syncthreads();     // before the lists are refilled
    count = 0;
    if (tid == 0) s_nbig = 0;
  }
  __syncthreads();

  // (C) resolve and shade: a wave stores row segments of the tile's width (256 contiguous bytes of RGBA at one sample per
  // pixel, two of 128 at four) per step
  const FlatShade flat{nrm, lights, n_lights, F3{shade[0], shade[1], shade[2]}, F3{shade[3], shade[4], shade[5]}};
  for (int p = tid; p < TILE * TILE; p += RT_THREADS) {
    const int i = ty0 + p / TILE, j = tx0 + p % TILE;
    if (i > ty1 || j > tx1) continue;
    const long o = ((long)b * H + i) * W + j;
    unsigned dmin = 0xffffffffu;      // depths are positive, so their bits order as they do
    int ids[S];
    float ds[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const unsigned long long key = s_key[p * S + k];
      const bool covered = key != RT_EMPTY;
      ids[k] = covered ? (int)(unsigned)(key & 0xffffffffull) : -1;
      ds[k] = covered ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
      if (covered) dmin = min(dmin, (unsigned)(key >> 32));
    }
    unsigned word;
    F3 unused;
    resolve_pixel<S, true>(flat, ids, faces, scr, V, F, near, tx0, ty0, tx1, ty1, j, i, bg, word, unused);
    rgba[o] = word;
    depth[o] = dmin == 0xffffffffu ? 0.f : __uint_as_float(dmin);
    if constexpr (S == 1) {
      if (face_id != nullptr) face_id[o] = ids[0];
    } else {
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

// The textured shader: the trilinearly sampled texel / 255 under the lighting, and (u, v, lambda) as sampled.  The launcher fills
// the first two rows; prepare(), once per workgroup, moves nrm to frame b, loads the ambient colour and builds the level table
// lvl_off / lvl_w / lvl_h (the offset, width and height of every level) in LDS.
struct TexturedShade {
  const float* nrm; const int* faces; const float* vt; const int* ft; const float4* pyramid; const float* shade; const float* lights;
  int n_lights, Nt, Ht, Wt, L;
  const int *lvl_off, *lvl_w, *lvl_h;
  F3 amb;
  float Wtf, Htf, top;
  __device__ __forceinline__ void prepare(int b, int V) {
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
    nrm += (long)b * V * 3;
    lvl_off = s_off; lvl_w = s_w; lvl_h = s_h;
    amb = F3{shade[3], shade[4], shade[5]};
    Wtf = (float)Wt; Htf = (float)Ht; top = (float)(L - 1);
  }
  __device__ __forceinline__ unsigned operator()(const FaceSetup& s, int g, const Bary& b, F3& uvl) const {
    const float iz = b.iz, p0 = b.p0, p1 = b.p1, p2 = b.p2;
    // per-corner texture coordinates in the face's oriented order: face_setup swapped corners 1 and 2 iff it swapped the ids
    const I3 ti = *(const I3*)(ft + (long)g * 3);
    const bool swapped = s.i1 != faces[(long)g * 3 + 1];
    const int k0 = ti.a, k1 = swapped ? ti.c : ti.b, k2 = swapped ? ti.b : ti.c;
    float2 t0 = make_float2(0.f, 0.f), t1 = t0, t2 = t0;
    if ((unsigned)k0 < (unsigned)Nt) t0 = *(const float2*)(vt + (long)k0 * 2);
    if ((unsigned)k1 < (unsigned)Nt) t1 = *(const float2*)(vt + (long)k1 * 2);
    if ((unsigned)k2 < (unsigned)Nt) t2 = *(const float2*)(vt + (long)k2 * 2);
    const float u = (p0 * t0.x + p1 * t1.x) + p2 * t2.x, v = (p0 * t0.y + p1 * t1.y) + p2 * t2.y;
    // analytic level of detail: d w_k / d j = a_k / A, d w_k / d i = c_k / A with the set-up's integer edge steps
    const float A = (float)s.area;
    const EdgeSteps d = s.steps();
    const float g0 = s.q0 * ((float)d.a0 / A), g1 = s.q1 * ((float)d.a1 / A), g2 = s.q2 * ((float)d.a2 / A);
    const float h0 = s.q0 * ((float)d.c0 / A), h1 = s.q1 * ((float)d.c1 / A), h2 = s.q2 * ((float)d.c2 / A);
    const float dDj = (g0 + g1) + g2, dDi = (h0 + h1) + h2;
    const float duj = (((g0 * t0.x + g1 * t1.x) + g2 * t2.x) - u * dDj) / iz, dvj = (((g0 * t0.y + g1 * t1.y) + g2 * t2.y) - v * dDj) / iz;
    const float dui = (((h0 * t0.x + h1 * t1.x) + h2 * t2.x) - u * dDi) / iz, dvi = (((h0 * t0.y + h1 * t1.y) + h2 * t2.y) - v * dDi) / iz;
    const float rj2 = (Wtf * duj) * (Wtf * duj) + (Htf * dvj) * (Htf * dvj),
                ri2 = (Wtf * dui) * (Wtf * dui) + (Htf * dvi) * (Htf * dvi);
    float lam = 0.5f * log2f(fmaxf(rj2, ri2));
    if (!(finite_f(rj2) && finite_f(ri2) && finite_f(lam))) lam = 0.f;
    lam = fminf(fmaxf(lam, 0.f), top);
    const float us = finite_f(u) ? u : 0.f, vs = finite_f(v) ? v : 0.f;
    const float U = us - floorf(us), Vv = vs - floorf(vs);
    const int l0 = min((int)floorf(lam), L - 1), l1 = min(l0 + 1, L - 1);
    const float fl = lam - (float)l0;
    const F3 c0 = texture_bilinear(pyramid + lvl_off[l0], lvl_w[l0], lvl_h[l0], U, Vv);
    const F3 c1 = texture_bilinear(pyramid + lvl_off[l1], lvl_w[l1], lvl_h[l1], U, Vv);
    const float gl = 1.f - fl;
    const float Tr = gl * c0.x + fl * c1.x, Tg = gl * c0.y + fl * c1.y, Tb = gl * c0.z + fl * c1.z;
    uvl = F3{us, vs, lam};
    return color_bytes(F3{Tr / 255.f, Tg / 255.f, Tb / 255.f}, true, amb, [&] { return lambert_diffuse(nrm, s, b, lights, n_lights); });
  }
};

// ------------------------------------------------------------------------------------------------ vertex colours
// The vertex-colour shader: from the RGBA bytes at the face's three vertices (alpha not read), per channel C = (p0 c0 + p1 c1) +
// p2 c2 with the perspective-correct weights, the corners in the order face_setup left them in (s.i0, s.i1, s.i2: the face and its
// colours swap together); then C / 255 under the lighting, or as it is unlit.  The three gathers per shaded point are 4-byte loads
// from a (V, 4) table that stays in L2.  The launcher fills the first two rows; prepare() moves nrm and vcol to frame b
// (col_stride = 0: the one shared table) and loads the ambient colour.
struct VertexColorShade {
  const float* nrm; const unsigned* vcol; const float* shade; const float* lights;
  long col_stride; int n_lights, lit;
  F3 amb;
  __device__ __forceinline__ void prepare(int b, int V) {
    nrm += (long)b * V * 3;
    vcol += (long)b * col_stride;
    amb = F3{shade[3], shade[4], shade[5]};
  }
  __device__ __forceinline__ unsigned operator()(const FaceSetup& s, int, const Bary& b, F3&) const {
    const float p0 = b.p0, p1 = b.p1, p2 = b.p2;
    const unsigned c0 = vcol[s.i0], c1 = vcol[s.i1], c2 = vcol[s.i2];
    const float Cr = (p0 * (float)(c0 & 255u) + p1 * (float)(c1 & 255u)) + p2 * (float)(c2 & 255u);
    const float Cg = (p0 * (float)((c0 >> 8) & 255u) + p1 * (float)((c1 >> 8) & 255u)) + p2 * (float)((c2 >> 8) & 255u);
    const float Cb = (p0 * (float)((c0 >> 16) & 255u) + p1 * (float)((c1 >> 16) & 255u)) + p2 * (float)((c2 >> 16) & 255u);
    return color_bytes(F3{Cr / 255.f, Cg / 255.f, Cb / 255.f}, lit, amb, [&] { return lambert_diffuse(nrm, s, b, lights, n_lights); });
  }
};

// ------------------------------------------------------------------------------------------------ the deferred pass
// One workgroup per (frame, 64 x 16 strip); pixel-parallel in stage (C)'s mapping, so a wave reads 64 contiguous face ids (at
// four samples per pixel, where face_id is (B, H, W, 4), 64 contiguous int4) and stores 256 contiguous bytes of RGBA per step.
// A pixel is resolved as the raster pass resolves it (resolve_pixel) with the pass's shader in place of the untextured one, and
// stored only if a sample was shaded: the others keep what the raster pass wrote.  uvl, one sample per pixel only, receives what the
// shader sampled, zeros at a pixel without a shaded sample.
template <int S, class Shade>
__global__ __launch_bounds__(TX_THREADS) void render_shade_kernel(Shade shade, const float* __restrict__ screen,
                                                                  const int* __restrict__ faces, const int* __restrict__ face_id,
                                                                  unsigned* __restrict__ rgba, float* __restrict__ uvl, int V, int F,
                                                                  int H, int W, int tiles_x, int strips_y, float near, unsigned bg) {
  const int per_frame = tiles_x * strips_y;
  const int b = blockIdx.x / per_frame, rest = blockIdx.x - b * per_frame;
  const int sy = rest / tiles_x, tx = rest - sy * tiles_x;
  const int tx0 = tx * RT_TILE, ty0 = sy * TX_ROWS;
  const float* scr = screen + (long)b * V * 3;
  shade.prepare(b, V);
  for (int p = threadIdx.x; p < RT_TILE * TX_ROWS; p += TX_THREADS) {
    const int i = ty0 + p / RT_TILE, j = tx0 + p % RT_TILE;
    if (i >= H || j >= W) continue;
    const long o = ((long)b * H + i) * W + j;
    int ids[S];
    if constexpr (S == 1) {
      ids[0] = face_id[o];
    } else {
      const int4 id4 = *(const int4*)(face_id + o * 4);
      ids[0] = id4.x; ids[1] = id4.y; ids[2] = id4.z; ids[3] = id4.w;
    }
    unsigned word;
    F3 sampled{0.f, 0.f, 0.f};
    const bool any = resolve_pixel<S, false>(shade, ids, faces, scr, V, F, near, 0, 0, W - 1, H - 1, j, i, bg, word, sampled);
    if (S == 1 && uvl != nullptr) *(F3*)(uvl + o * 3) = sampled;
    if (any) rgba[o] = word;
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
// The launch of a deferred pass with its shader: what every such pass checks, the sample count, the 64 x 16 strip grid.
template <class Shade>
int launch_shade(const Shade& shade, const float* screen, const int* faces, const int* face_id, void* rgba, float* uvl, int B, int V,
                 int F, int H, int W, float near, unsigned background, int samples, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0 || shade.n_lights < 0 || !(near > 0.f) || face_id == nullptr) return 1;
  if (samples != 1 && samples != 4) return 1;
  if (samples == 4 && ((size_t)face_id & 15) != 0) return 1;      // read as int4
  const int tiles_x = (W + RT_TILE - 1) / RT_TILE, strips_y = (H + TX_ROWS - 1) / TX_ROWS;
  const long grid = (long)B * tiles_x * strips_y;
  if (grid > 2147483647L) return 1;
  const auto kernel = samples == 4 ? render_shade_kernel<4, Shade> : render_shade_kernel<1, Shade>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(TX_THREADS), 0, (hipStream_t)stream, shade, screen, faces, face_id,
                     (unsigned*)rgba, uvl, V, F, H, W, tiles_x, strips_y, near, background);
  MSMD_RETURN_LAST();
}

int shade_textured(const float* screen, const float* normals, const int* faces, const float* vt, const int* ft, const float* pyramid,
                   int Ht, int Wt, const float* shade, const float* lights, int n_lights, const int* face_id, void* rgba, float* uvl,
                   int B, int V, int F, int Nt, int H, int W, float near, unsigned background, int samples, msmd_stream_t stream) {
  if (Nt <= 0 || msmd_texture_texels(Ht, Wt) < 0) return 1;
  TexturedShade t{};
  t.nrm = normals; t.faces = faces; t.vt = vt; t.ft = ft; t.pyramid = (const float4*)pyramid; t.shade = shade; t.lights = lights;
  t.n_lights = n_lights; t.Nt = Nt; t.Ht = Ht; t.Wt = Wt; t.L = 1;
  for (int m = Ht > Wt ? Ht : Wt; m > 1; m >>= 1) ++t.L;
  return launch_shade(t, screen, faces, face_id, rgba, uvl, B, V, F, H, W, near, background, samples, stream);
}
}  // namespace

extern "C" int msmd_render_shade_textured(const float* screen, const float* normals, const int* faces, const float* vt, const int* ft,
                                          const float* pyramid, int Ht, int Wt, const float* shade, const float* lights,
                                          int n_lights, const int* face_id, void* rgba, float* uvl, int B, int V, int F, int Nt,
                                          int H, int W, float near, msmd_stream_t stream) {
  return shade_textured(screen, normals, faces, vt, ft, pyramid, Ht, Wt, shade, lights, n_lights, face_id, rgba, uvl, B, V, F, Nt, H, W,
                        near, 0u, 1, stream);
}

extern "C" int msmd_render_shade_textured_ms(const float* screen, const float* normals, const int* faces, const float* vt,
                                             const int* ft, const float* pyramid, int Ht, int Wt, const float* shade,
                                             const float* lights, int n_lights, const int* sample_face_id, void* rgba, int B, int V,
                                             int F, int Nt, int H, int W, float near, unsigned background, int samples,
                                             msmd_stream_t stream) {
  return shade_textured(screen, normals, faces, vt, ft, pyramid, Ht, Wt, shade, lights, n_lights, sample_face_id, rgba, nullptr, B, V,
                        F, Nt, H, W, near, background, samples, stream);
}

extern "C" int msmd_render_shade_vertex_color(const float* screen, const float* normals, const int* faces, const unsigned char* vcol,
                                              int color_per_frame, int lit, const float* shade, const float* lights, int n_lights,
                                              const int* sample_face_id, void* rgba, int B, int V, int F, int H, int W, float near,
                                              unsigned background, int samples, msmd_stream_t stream) {
  if (vcol == nullptr || ((size_t)vcol & 3) != 0) return 1;      // a vertex's four bytes are read as one word
  VertexColorShade t{};
  t.nrm = normals; t.vcol = (const unsigned*)vcol; t.shade = shade; t.lights = lights;
  t.col_stride = color_per_frame ? (long)V : 0L; t.n_lights = n_lights; t.lit = lit != 0;
  return launch_shade(t, screen, faces, sample_face_id, rgba, nullptr, B, V, F, H, W, near, background, samples, stream);
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
// sample_depth is stored by the kernel at four samples only (as float4, and face_id as int4)
int launch_raster(const float* screen, const float* normals, const int* faces, const float* shade, const float* lights, int n_lights,
                  void* rgba, float* depth, int* face_id, float* sample_depth, int B, int V, int F, int H, int W, float near, float far,
                  unsigned background, int samples, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0 || n_lights < 0 || !(near > 0.f) || !(far >= near)) return 1;
  if (samples != 1 && samples != 4) return 1;
  if (samples == 4 && ((((size_t)face_id) | ((size_t)sample_depth)) & 15) != 0) return 1;
  const int tile = samples == 4 ? RT_TILE_MS : RT_TILE;
  const int tiles_x = (W + tile - 1) / tile, tiles_y = (H + tile - 1) / tile;
  const long grid = (long)B * tiles_x * tiles_y;
  if (grid > 2147483647L) return 1;
  const auto kernel = samples == 4 ? render_raster_kernel<4> : render_raster_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(RT_THREADS), 0, (hipStream_t)stream, screen, normals, faces, shade, lights,
                     n_lights, (unsigned*)rgba, depth, face_id, samples == 4 ? sample_depth : nullptr, V, F, H, W, tiles_x, tiles_y, near,
                     far, background);
  MSMD_RETURN_LAST();
}
}  // namespace

extern "C" int msmd_render_raster(const float* screen, const float* normals, const int* faces, const float* shade,
                                  const float* lights, int n_lights, void* rgba, float* depth, int* face_id, int B, int V,
                                  int F, int H, int W, float near, float far, unsigned background, msmd_stream_t stream) {
  return launch_raster(screen, normals, faces, shade, lights, n_lights, rgba, depth, face_id, nullptr, B, V, F, H, W, near, far,
                       background, 1, stream);
}

extern "C" int msmd_render_raster_ms(const float* screen, const float* normals, const int* faces, const float* shade,
                                     const float* lights, int n_lights, void* rgba, float* depth, int* sample_face_id,
                                     float* sample_depth, int B, int V, int F, int H, int W, float near, float far,
                                     unsigned background, int samples, msmd_stream_t stream) {
  const int rc = launch_raster(screen, normals, faces, shade, lights, n_lights, rgba, depth, sample_face_id, sample_depth, B, V, F, H, W,
                               near, far, background, samples, stream);
  if (rc != 0 || samples != 1 || sample_depth == nullptr) return rc;
  // one sample per pixel: the sample's depth is the pixel's
  return (int)hipMemcpyAsync(sample_depth, depth, (size_t)B * H * W * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
}
