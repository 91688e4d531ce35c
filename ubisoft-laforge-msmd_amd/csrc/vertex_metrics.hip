// Vertex-space evaluation of a predicted mesh sequence against the ground truth: the per-frame error table behind
// the lip vertex error and the mean / maximum / RMS vertex error, and the per-vertex running moments behind the upper-face
// dynamics deviation.  Both stream the two vertex tensors once.  Everything after the loads is float64 with every operation
// rounded on its own (no fused multiply-add), so a numpy transcription of the lines below holds the same numbers.  No
// floating-point atomics: a frame's row has one workgroup, a (clip, vertex, track) state has one thread, and each is reduced in an
// order that depends on V (on the frame order) alone.  The error FIELD behind those numbers is kept too: the per-vertex
// distance through a colour table, and its running per-clip sum, under the same conventions.
#include "common.h"

#define VM_THREADS 256
#define VM_WAVES (VM_THREADS / MSMD_WAVE)
#define VM_BATCH 8                // loads a thread issues per tensor before it consumes the first
#define VM_UT 32                  // moments: upper vertices per workgroup ...
#define VM_FL (VM_THREADS / VM_UT) // ... times frame lanes
#define VM_TILE (VM_FL * VM_BATCH) // frames per tile
static_assert(2 * VM_UT == MSMD_WAVE, "the owners of a moments workgroup are the threads of wave 0");

struct __attribute__((packed, aligned(2))) H3 { f16_t x, y, z; };
template <typename T> struct Vertex;
template <> struct Vertex<float> { typedef F3 type; };
template <> struct Vertex<f16_t> { typedef H3 type; };

// |a - b|^2 of one vertex, ((dx dx + dy dy) + dz dz), from the exact float64 images of the stored values
template <typename VA, typename VB> __device__ __forceinline__ double dist2(const VA a, const VB b) {
#pragma clang fp contract(off)
  const double dx = (double)(float)a.x - (double)(float)b.x;
  const double dy = (double)(float)a.y - (double)(float)b.y;
  const double dz = (double)(float)a.z - (double)(float)b.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// numpy's maximum: a NaN on either side is the result (fmax / v_max_f64 would drop it)
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

struct FrameAcc { double lip, sum, mx, sq; };

__device__ __forceinline__ FrameAcc acc_join(const FrameAcc a, const FrameAcc b) {
  return FrameAcc{nan_max(a.lip, b.lip), a.sum + b.sum, nan_max(a.mx, b.mx), a.sq + b.sq};
}

// One workgroup per frame.  Lane-per-vertex loads: a wave's load instruction covers 64 consecutive vertices, 768 (384)
// contiguous bytes, and 64 consecutive region bytes.  Thread t folds vertices t, t + 256, ... in ascending order; the wave joins
// its lanes by the xor butterfly 32, 16, .. 1 (both partners form the same commutative sum, so every lane holds the same bits);
// thread 0 joins the four waves in wave order.
template <typename T>
__global__ __launch_bounds__(VM_THREADS) void vertex_frame_errors_kernel(const T* __restrict__ pred, const T* __restrict__ gt,
                                                                         const unsigned char* __restrict__ region,
                                                                         double* __restrict__ out, int V) {
  typedef typename Vertex<T>::type Vtx;
  __shared__ FrameAcc part[VM_WAVES];
  const long base = (long)blockIdx.x * V;
  const Vtx* p = (const Vtx*)pred + base;
  const Vtx* g = (const Vtx*)gt + base;
  FrameAcc a{0.0, 0.0, 0.0, 0.0};                  // every d2 is >= 0 or NaN: 0 is the identity of both maxima
  // VM_BATCH vertices' loads are issued before the first is folded; the last batch re-reads vertex V - 1 in the slots past the end
  // and does not fold them (a remainder loop would wait for one load at a time)
  for (int v0 = threadIdx.x; v0 < V; v0 += VM_BATCH * VM_THREADS) {
    Vtx pv[VM_BATCH], gv[VM_BATCH];
    unsigned char rg[VM_BATCH];
#pragma unroll
    for (int j = 0; j < VM_BATCH; ++j) {
      const int v = min(v0 + j * VM_THREADS, V - 1);
      pv[j] = p[v];
      gv[j] = g[v];
      rg[j] = region[v];
    }
#pragma unroll
    for (int j = 0; j < VM_BATCH; ++j) {
      if (v0 + j * VM_THREADS < V) {
        const double d2 = dist2(pv[j], gv[j]);
        const double d = sqrt(d2);
        if (rg[j] & 1) a.lip = nan_max(a.lip, d2);
        a.sum += d;
        a.mx = nan_max(a.mx, d);
        a.sq += d2;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    FrameAcc b;
    b.lip = __shfl_xor(a.lip, o, 64);
    b.sum = __shfl_xor(a.sum, o, 64);
    b.mx = __shfl_xor(a.mx, o, 64);
    b.sq = __shfl_xor(a.sq, o, 64);
    a = acc_join(a, b);
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    FrameAcc r = part[0];
    for (int w = 1; w < VM_WAVES; ++w) r = acc_join(r, part[w]);
    double* o = out + 4L * blockIdx.x;
    o[0] = r.lip;
    o[1] = r.sum;
    o[2] = r.mx;
    o[3] = r.sq;
  }
}

// Welford's recurrence on m = |v - template|^2, one (count, mean, M2) triple per track:
//   count += 1;  delta = m - mean;  mean += delta / count;  M2 += delta * (m - mean)
struct Moments { double count, mean, m2; };

__device__ __forceinline__ void welford_push(Moments& s, double m) {
#pragma clang fp contract(off)
  s.count += 1.0;
  const double delta = m - s.mean;
  s.mean += delta / s.count;
  s.m2 += delta * (m - s.mean);
}

// One thread OWNS one (clip, u, track): it alone reads, updates and writes that state, walking the frames of its clip that lie in
// [frame0, frame0 + n_chunk) in frame order.  The loads are spread wider than the owners: a workgroup is VM_UT upper vertices x
// VM_FL frame lanes; per tile of VM_TILE = VM_FL * VM_BATCH frames, thread (x, y) loads frames y, y + VM_FL, ... of vertex x from both
// tensors (VM_BATCH loads in flight each) and leaves m in LDS at its frame's slot; then the owners -- wave 0: y = 0 the prediction's
// track, y = 1 the ground truth's -- run the recurrence down the tile's slots.  The state goes through memory between chunks, a
// float64 round trip is exact, and so the final state does not know where the chunks were cut.  clip, lo and hi depend on
// blockIdx and the arguments alone: every branch around a barrier is uniform over the workgroup.
template <typename T>
__global__ __launch_bounds__(VM_THREADS) void vertex_motion_moments_kernel(const T* __restrict__ pred, const T* __restrict__ gt,
                                                                           long frame0, int n_chunk,
                                                                           const long* __restrict__ clip_offsets,
                                                                           const int* __restrict__ upper_idx, int U,
                                                                           const float* __restrict__ tmpl, int template_per_clip,
                                                                           double* __restrict__ state, int V, int tiles) {
  typedef typename Vertex<T>::type Vtx;
  __shared__ double ms[2][VM_TILE][VM_UT];
  const int clip = blockIdx.x / tiles, x = threadIdx.x % VM_UT, y = threadIdx.x / VM_UT;
  const long c0 = clip_offsets[clip], c1 = clip_offsets[clip + 1], end = frame0 + (long)n_chunk;
  const long lo = c0 > frame0 ? c0 : frame0, hi = c1 < end ? c1 : end;
  if (lo >= hi) return;                              // the clip has no frame in this chunk: its state is not touched
  const int u = (blockIdx.x % tiles) * VM_UT + x, uc = min(u, U - 1);
  const int v = min(max(upper_idx[uc], 0), V - 1);
  const F3 t = ((const F3*)tmpl)[(template_per_clip ? (long)clip * V : 0L) + v];
  const bool owner = y < 2 && u < U;
  double* st = state + (((long)clip * U + uc) * 2 + (y & 1)) * 3;
  Moments s{0.0, 0.0, 0.0};
  if (owner) s = Moments{st[0], st[1], st[2]};
  const Vtx* p = (const Vtx*)pred + v;
  const Vtx* g = (const Vtx*)gt + v;
  const long nf = hi - frame0;                       // the clip's frames in this chunk are [lo - frame0, nf) of pred / gt
  for (long f0 = lo - frame0; f0 < nf; f0 += VM_TILE) {
    Vtx pv[VM_BATCH], gv[VM_BATCH];
#pragma unroll
    for (int j = 0; j < VM_BATCH; ++j) {
      const long f = f0 + y + j * VM_FL;
      const long ff = f < nf ? f : nf - 1;           // slots past the end re-read the last frame; the owners do not push them
      pv[j] = p[ff * V];
      gv[j] = g[ff * V];
    }
#pragma unroll
    for (int j = 0; j < VM_BATCH; ++j) {
      ms[0][y + j * VM_FL][x] = dist2(pv[j], t);
      ms[1][y + j * VM_FL][x] = dist2(gv[j], t);
    }
    __syncthreads();
    if (owner) {
      const int cnt = nf - f0 < VM_TILE ? (int)(nf - f0) : VM_TILE;
      for (int k = 0; k < cnt; ++k) welford_push(s, ms[y][k][x]);
    }
    __syncthreads();                                 // the next tile overwrites the slots
  }
  if (owner) { st[0] = s.count; st[1] = s.mean; st[2] = s.m2; }
}

// ------------------------------------------------------------------------------------------------ the error field
#define VM_COLOR_BATCH 4          // vertices (elements) a thread of the colour kernels loads before it consumes the first

// x -> t = x / vmax -> a table row, ONE routine for the distance field and for any float64 array: NaN gives nan_color; t >= 1
// (+inf too) row 255; otherwise floor(t * 255 + 0.5), which is at most 255; t <= 0 (-inf too; a distance is never negative) row 0
__device__ __forceinline__ unsigned colormap_word(double x, double vmax, const unsigned* lut, unsigned nan_color) {
#pragma clang fp contract(off)
  const double t = x / vmax;
  if (t != t) return nan_color;
  const int idx = t >= 1.0 ? 255 : t > 0.0 ? (int)floor(t * 255.0 + 0.5) : 0;
  return lut[idx];
}

// the 256 table rows, one 4-byte word each, into LDS: one load per thread of the workgroup
__device__ __forceinline__ void stage_lut(const unsigned* __restrict__ lut, unsigned* s_lut) {
  static_assert(VM_THREADS == 256, "one table row per thread");
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
}

// The n V vertices as one flat run: a workgroup takes VM_COLOR_BATCH * 256 consecutive vertices, thread t the vertices t, t + 256,
// ... of them, so a wave's load covers 768 (384) contiguous bytes per tensor and its store 256 contiguous bytes.  The distance is
// never stored.  The slots past the end re-read the last vertex and store nothing.
template <typename T>
__global__ __launch_bounds__(VM_THREADS) void vertex_error_colors_kernel(const T* __restrict__ pred, const T* __restrict__ gt,
                                                                         const unsigned* __restrict__ lut, unsigned* __restrict__ out,
                                                                         long N, double vmax, unsigned nan_color) {
  typedef typename Vertex<T>::type Vtx;
  __shared__ unsigned s_lut[256];
  stage_lut(lut, s_lut);
  const Vtx* p = (const Vtx*)pred;
  const Vtx* g = (const Vtx*)gt;
  const long v0 = (long)blockIdx.x * (VM_COLOR_BATCH * VM_THREADS) + threadIdx.x;
  Vtx pv[VM_COLOR_BATCH], gv[VM_COLOR_BATCH];
#pragma unroll
  for (int j = 0; j < VM_COLOR_BATCH; ++j) {
    const long v = v0 + j * VM_THREADS < N ? v0 + j * VM_THREADS : N - 1;
    pv[j] = p[v];
    gv[j] = g[v];
  }
#pragma unroll
  for (int j = 0; j < VM_COLOR_BATCH; ++j) {
    const long v = v0 + j * VM_THREADS;
    if (v < N) out[v] = colormap_word(sqrt(dist2(pv[j], gv[j])), vmax, s_lut, nan_color);
  }
}

__global__ __launch_bounds__(VM_THREADS) void colormap_f64_kernel(const double* __restrict__ x, const unsigned* __restrict__ lut,
                                                                  unsigned* __restrict__ out, long N, double vmax,
                                                                  unsigned nan_color) {
  __shared__ unsigned s_lut[256];
  stage_lut(lut, s_lut);
  const long i0 = (long)blockIdx.x * (VM_COLOR_BATCH * VM_THREADS) + threadIdx.x;
  double xv[VM_COLOR_BATCH];
#pragma unroll
  for (int j = 0; j < VM_COLOR_BATCH; ++j) xv[j] = x[i0 + j * VM_THREADS < N ? i0 + j * VM_THREADS : N - 1];
#pragma unroll
  for (int j = 0; j < VM_COLOR_BATCH; ++j) {
    const long i = i0 + j * VM_THREADS;
    if (i < N) out[i] = colormap_word(xv[j], vmax, s_lut, nan_color);
  }
}

// One thread OWNS one (clip, vertex): it alone reads, updates and writes that sum, adding the distance of the clip's frames that lie
// in [frame0, frame0 + n_chunk) in frame order (VM_BATCH frames' loads in flight; the slots past the end re-read the last frame and
// are not added).  Consecutive threads own consecutive vertices: a frame's reads are contiguous 12- (6-) byte triples.  The sum goes
// through memory between chunks, a float64 round trip is exact, and so the final sum does not know where the chunks were cut.
template <typename T>
__global__ __launch_bounds__(VM_THREADS) void vertex_error_sums_kernel(const T* __restrict__ pred, const T* __restrict__ gt, long frame0,
                                                                       int n_chunk, const long* __restrict__ clip_offsets,
                                                                       double* __restrict__ state, int V, int tiles) {
  typedef typename Vertex<T>::type Vtx;
  const int clip = blockIdx.x / tiles, v = (blockIdx.x % tiles) * VM_THREADS + threadIdx.x;
  const long c0 = clip_offsets[clip], c1 = clip_offsets[clip + 1], end = frame0 + (long)n_chunk;
  const long lo = c0 > frame0 ? c0 : frame0, hi = c1 < end ? c1 : end;
  if (lo >= hi || v >= V) return;                    // the clip has no frame in this chunk: its sums are not touched
  double* st = state + (long)clip * V + v;
  double s = *st;
  const Vtx* p = (const Vtx*)pred + v;
  const Vtx* g = (const Vtx*)gt + v;
  const long nf = hi - frame0;                       // the clip's frames in this chunk are [lo - frame0, nf) of pred / gt
  for (long f0 = lo - frame0; f0 < nf; f0 += VM_BATCH) {
    Vtx pv[VM_BATCH], gv[VM_BATCH];
#pragma unroll
    for (int j = 0; j < VM_BATCH; ++j) {
      const long ff = f0 + j < nf ? f0 + j : nf - 1;
      pv[j] = p[ff * V];
      gv[j] = g[ff * V];
    }
#pragma unroll
    for (int j = 0; j < VM_BATCH; ++j)
      if (f0 + j < nf) s += sqrt(dist2(pv[j], gv[j]));
  }
  *st = s;
}

extern "C" int msmd_vertex_frame_errors(const void* pred, const void* gt, const unsigned char* region, double* out, int n, int V,
                                        int dtype, msmd_stream_t stream) {
  if (n < 0 || V < 1 || (dtype != MSMD_F32 && dtype != MSMD_F16)) return 1;
  if (n == 0) return 0;
  if (!pred || !gt || !region || !out) return 1;
  return dispatch_dtype<float, f16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) T;
    hipLaunchKernelGGL(vertex_frame_errors_kernel<T>, dim3((unsigned)n), dim3(VM_THREADS), 0, (hipStream_t)stream, (const T*)pred,
                       (const T*)gt, region, out, V);
    return (int)hipGetLastError();
  });
}

extern "C" int msmd_vertex_motion_moments(const void* pred, const void* gt, long frame0, int n_chunk, const long* clip_offsets,
                                          int n_clips, const int* upper_idx, int U, const float* tmpl, int template_per_clip,
                                          double* state, int V, int dtype, msmd_stream_t stream) {
  if (n_chunk < 0 || frame0 < 0 || n_clips < 1 || U < 1 || V < 1 || (dtype != MSMD_F32 && dtype != MSMD_F16)) return 1;
  const long tiles = ((long)U + VM_UT - 1) / VM_UT;
  if ((long)n_clips * tiles > 0x7fffffffL) return 1;
  if (n_chunk == 0) return 0;
  if (!pred || !gt || !clip_offsets || !upper_idx || !tmpl || !state) return 1;
  return dispatch_dtype<float, f16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) T;
    hipLaunchKernelGGL(vertex_motion_moments_kernel<T>, dim3((unsigned)(n_clips * tiles)), dim3(VM_THREADS), 0, (hipStream_t)stream,
                       (const T*)pred, (const T*)gt, frame0, n_chunk, clip_offsets, upper_idx, U, tmpl, template_per_clip != 0,
                       state, V, (int)tiles);
    return (int)hipGetLastError();
  });
}

namespace {
// the colour kernels read the table and write the colours as 4-byte words; a workgroup takes VM_COLOR_BATCH * 256 elements
bool color_args_ok(const void* lut, const void* out, long N, double vmax) {
  const bool finite = vmax - vmax == 0.0;            // false for NaN and +-inf
  return finite && vmax > 0.0 && lut && out && ((((size_t)lut) | ((size_t)out)) & 3) == 0 &&
         (N + VM_COLOR_BATCH * VM_THREADS - 1) / (VM_COLOR_BATCH * VM_THREADS) <= 0x7fffffffL;
}
}  // namespace

extern "C" int msmd_vertex_error_colors(const void* pred, const void* gt, const unsigned char* lut, unsigned char* out, int n, int V,
                                        int dtype, double vmax, unsigned nan_color, msmd_stream_t stream) {
  if (n < 0 || V < 1 || (dtype != MSMD_F32 && dtype != MSMD_F16) || !(vmax - vmax == 0.0) || !(vmax > 0.0)) return 1;
  if (n == 0) return 0;
  const long N = (long)n * V;
  if (!pred || !gt || !color_args_ok(lut, out, N, vmax)) return 1;
  const unsigned grid = (unsigned)((N + VM_COLOR_BATCH * VM_THREADS - 1) / (VM_COLOR_BATCH * VM_THREADS));
  return dispatch_dtype<float, f16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) T;
    hipLaunchKernelGGL(vertex_error_colors_kernel<T>, dim3(grid), dim3(VM_THREADS), 0, (hipStream_t)stream, (const T*)pred,
                       (const T*)gt, (const unsigned*)lut, (unsigned*)out, N, vmax, nan_color);
    return (int)hipGetLastError();
  });
}

extern "C" int msmd_colormap_f64(const double* x, const unsigned char* lut, unsigned char* out, long N, double vmax,
                                 unsigned nan_color, msmd_stream_t stream) {
  if (N < 0 || !(vmax - vmax == 0.0) || !(vmax > 0.0)) return 1;
  if (N == 0) return 0;
  if (!x || !color_args_ok(lut, out, N, vmax)) return 1;
  const unsigned grid = (unsigned)((N + VM_COLOR_BATCH * VM_THREADS - 1) / (VM_COLOR_BATCH * VM_THREADS));
  hipLaunchKernelGGL(colormap_f64_kernel, dim3(grid), dim3(VM_THREADS), 0, (hipStream_t)stream, x, (const unsigned*)lut,
                     (unsigned*)out, N, vmax, nan_color);
  return (int)hipGetLastError();
}

extern "C" int msmd_vertex_error_sums(const void* pred, const void* gt, long frame0, int n_chunk, const long* clip_offsets,
                                      int n_clips, double* state, int V, int dtype, msmd_stream_t stream) {
  if (n_chunk < 0 || frame0 < 0 || n_clips < 1 || V < 1 || (dtype != MSMD_F32 && dtype != MSMD_F16)) return 1;
  const long tiles = ((long)V + VM_THREADS - 1) / VM_THREADS;
  if ((long)n_clips * tiles > 0x7fffffffL) return 1;
  if (n_chunk == 0) return 0;
  if (!pred || !gt || !clip_offsets || !state) return 1;
  return dispatch_dtype<float, f16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) T;
    hipLaunchKernelGGL(vertex_error_sums_kernel<T>, dim3((unsigned)(n_clips * tiles)), dim3(VM_THREADS), 0, (hipStream_t)stream,
                       (const T*)pred, (const T*)gt, frame0, n_chunk, clip_offsets, state, V, (int)tiles);
    return (int)hipGetLastError();
  });
}
