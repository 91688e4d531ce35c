// Frame resizing: Pillow's separable fixed-point resampling of 8-bit frames, stated in include/msmd_hip.h.
// Integer VALU code only: the coefficient tables come from the host, a pass is sum(byte * coef) in int32, + 2^21, >> 22, clip.
// Two forms with the same bytes: a horizontal and a vertical launch with the rounded intermediate in HBM, and one fused
// launch that keeps the intermediate rows of a tile in LDS.
#include "common.h"

constexpr int RS_WG = 256;
constexpr int RS_TH = MSMD_RESIZE_TILE_H, RS_TW = MSMD_RESIZE_TILE_W;
constexpr int RS_BITS = MSMD_RESIZE_PRECISION_BITS;

// One axis' tables: T sets of n_out (first, taps) pairs and n_out x ksize weights; n_in bounds what a table may address.
struct RsAxis {
  const int* bounds;
  const int* coef;
  int ksize, T, n_in, n_out;
};

// The taps of output sample o in table t, clamped so that first + i stays inside [0, n_in) for every i < taps.
__device__ __forceinline__ void rs_taps(const RsAxis& a, int t, int o, int& first, int& taps, const int*& k) {
  const long at = (long)t * a.n_out + o;
  first = min(max(a.bounds[2 * at], 0), a.n_in - 1);
  taps = min(max(a.bounds[2 * at + 1], 0), min(a.ksize, a.n_in - first));
  k = a.coef + at * a.ksize;
}
__device__ __forceinline__ int rs_table(const int* __restrict__ table_of_frame, int n, int T) {
  return min(max(table_of_frame[n], 0), T - 1);
}
// The accumulator is carried as unsigned (wrap-around is defined) and read as int32 for the arithmetic shift.
// clip((int)acc >> 22, 0, 255), written on the value biased by 2^31: (acc + 2^31) >> 22 is the arithmetic shift + 512 exactly.
// A first build wrote min(max((int)acc >> 22, 0), 255), which the compiler joined with the packing of two bytes into gfx950's
// v_ashr_pk_u8_i32; the word the fused 4-channel kernel built for LDS then carried wrong bytes in its upper half on the MI355X
// (channels 2 and 3 of every pixel).  The cause is not established.  This form, an add, a shift, a v_med3 and
// a subtract per byte, is not matched to that instruction, and the GPU byte tests are what would notice if it ever were.
__device__ __forceinline__ unsigned rs_round(unsigned acc) {
  const unsigned biased = (acc + 0x80000000u) >> RS_BITS;
  return min(max(biased, 512u), 767u) - 512u;
}

// Four consecutive bytes (byte offset b0 .. b0 + 3 of an output row of n_out * C bytes) of the horizontal pass over one source
// row, as one little-endian word.  A byte past the row's end repeats the last one: computed in bounds, never stored.
// wide4: C == 4, 4-byte pixels and a 4-byte aligned row: one word load per tap serves the four channels.
template <int C>
__device__ __forceinline__ unsigned rs_hword(const unsigned char* __restrict__ row, int pixel_stride, const RsAxis& ax, int t,
                                             int b0, bool wide4) {
  const int last = ax.n_out * C - 1;
  if (C == 4 && wide4) {
    int first, taps;
    const int* k;
    rs_taps(ax, t, min(b0, last) >> 2, first, taps, k);
    const unsigned* p = (const unsigned*)row + first;
    unsigned a0 = 1u << (RS_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int i = 0; i < taps; ++i) {
      const unsigned w = p[i], c = (unsigned)k[i];
      a0 += (w & 255u) * c;
      a1 += ((w >> 8) & 255u) * c;
      a2 += ((w >> 16) & 255u) * c;
      a3 += (w >> 24) * c;
    }
    return rs_round(a0) | rs_round(a1) << 8 | rs_round(a2) << 16 | rs_round(a3) << 24;
  }
  unsigned word = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = min(b0 + e, last), x = b / C, c = b - x * C;
    int first, taps;
    const int* k;
    rs_taps(ax, t, x, first, taps, k);
    const unsigned char* p = row + (long)first * pixel_stride + c;
    unsigned acc = 1u << (RS_BITS - 1);
    for (int i = 0; i < taps; ++i) acc += (unsigned)p[(long)i * pixel_stride] * (unsigned)k[i];
    word |= rs_round(acc) << (8 * e);
  }
  return word;
}

// Four accumulators of the vertical pass take one word of an intermediate row.
__device__ __forceinline__ void rs_vacc(unsigned* acc, unsigned w, unsigned c) {
  acc[0] += (w & 255u) * c;
  acc[1] += ((w >> 8) & 255u) * c;
  acc[2] += ((w >> 16) & 255u) * c;
  acc[3] += (w >> 24) * c;
}
// Bytes b0 .. b0 + 3 of a row of row_bytes: one word store (VEC: the launcher has checked row_bytes % 4 == 0 and the alignment)
// or the bytes that exist.
template <bool VEC>
__device__ __forceinline__ void rs_store(unsigned char* __restrict__ row, int b0, int row_bytes, const unsigned* acc) {
  if constexpr (VEC) {
    *(unsigned*)(row + b0) = rs_round(acc[0]) | rs_round(acc[1]) << 8 | rs_round(acc[2]) << 16 | rs_round(acc[3]) << 24;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (b0 + e < row_bytes) row[b0 + e] = (unsigned char)rs_round(acc[e]);
  }
}

// ---- two-pass form.  One lane per word of four output bytes; the words of the batch are numbered row by row.
template <int C, bool VEC>
__global__ __launch_bounds__(RS_WG) void resize_h_kernel(const unsigned char* __restrict__ src, long frame_stride, long row_stride,
                                                         int pixel_stride, int N, int Hs, RsAxis ax,
                                                         const int* __restrict__ table_of_frame, unsigned char* __restrict__ mid,
                                                         bool wide4) {
  const int row_bytes = ax.n_out * C, row_words = (row_bytes + 3) >> 2;
  const long idx = (long)blockIdx.x * RS_WG + threadIdx.x;
  if (idx >= (long)N * Hs * row_words) return;
  const long line = idx / row_words;
  const int j = (int)(idx - line * row_words), n = (int)(line / Hs), r = (int)(line - (long)n * Hs);
  const unsigned w = rs_hword<C>(src + n * frame_stride + r * row_stride, pixel_stride, ax, rs_table(table_of_frame, n, ax.T), 4 * j, wide4);
  unsigned char* out = mid + line * row_bytes;
  if constexpr (VEC) {
    *(unsigned*)(out + 4 * j) = w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * j + e < row_bytes) out[4 * j + e] = (unsigned char)(w >> (8 * e));
  }
}

// mid (N, Hs = ay.n_in, row_bytes) -> dst (N, Hd = ay.n_out, row_bytes); VEC covers the loads too (same row length).
template <bool VEC>
__global__ __launch_bounds__(RS_WG) void resize_v_kernel(const unsigned char* __restrict__ mid, int N, int row_bytes, RsAxis ay,
                                                         const int* __restrict__ table_of_frame, unsigned char* __restrict__ dst) {
  const int row_words = (row_bytes + 3) >> 2;
  const long idx = (long)blockIdx.x * RS_WG + threadIdx.x;
  if (idx >= (long)N * ay.n_out * row_words) return;
  const long line = idx / row_words;
  const int j = (int)(idx - line * row_words), n = (int)(line / ay.n_out), y = (int)(line - (long)n * ay.n_out);
  int first, taps;
  const int* k;
  rs_taps(ay, rs_table(table_of_frame, n, ay.T), y, first, taps, k);
  const unsigned char* p = mid + ((long)n * ay.n_in + first) * row_bytes + 4 * j;
  unsigned acc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = 1u << (RS_BITS - 1);
  for (int i = 0; i < taps; ++i, p += row_bytes) {
    unsigned w;
    if constexpr (VEC) {
      w = *(const unsigned*)p;
    } else {
      w = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * j + e < row_bytes) w |= (unsigned)p[e] << (8 * e);
    }
    rs_vacc(acc, w, (unsigned)k[i]);
  }
  rs_store<VEC>(dst + line * row_bytes, 4 * j, row_bytes, acc);
}

// ---- fused form.  LDS: rows_cap rows of RS_TW * C bytes, each padded by one word (the pitch in words is odd: the lanes of a
// wave that read one column of neighbouring rows fall on different banks).
template <int C, bool VEC>
__global__ __launch_bounds__(RS_WG) void resize_fused_kernel(const unsigned char* __restrict__ src, long frame_stride, long row_stride,
                                                             int pixel_stride, RsAxis ax, RsAxis ay,
                                                             const int* __restrict__ table_of_frame, unsigned char* __restrict__ dst,
                                                             int rows_cap, int tiles_x, int tiles_y, bool wide4) {
  extern __shared__ unsigned s_mid[];
  constexpr int ROW_WORDS = RS_TW * C / 4, PITCH = ROW_WORDS + 1;
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, n = b / tiles_y;
  const int x0 = tx * RS_TW, y0 = ty * RS_TH;
  const int tab_x = rs_table(table_of_frame, n, ax.T), tab_y = rs_table(table_of_frame, n, ay.T);
  // the source rows this tile's vertical taps touch: [r0, r0 + n_rows)
  int r0 = ay.n_in, r1 = 0;
  for (int j = 0; j < RS_TH; ++j) {
    int first, taps;
    const int* k;
    rs_taps(ay, tab_y, min(y0 + j, ay.n_out - 1), first, taps, k);
    r0 = min(r0, first);
    r1 = max(r1, first + taps);
  }
  const int n_rows = min(max(r1 - r0, 0), rows_cap);
  const int row_bytes = ax.n_out * C;
  const unsigned char* frame = src + n * frame_stride;
  for (int item = threadIdx.x; item < n_rows * ROW_WORDS; item += RS_WG) {
    const int r = item / ROW_WORDS, j = item - r * ROW_WORDS;
    s_mid[r * PITCH + j] = rs_hword<C>(frame + (long)(r0 + r) * row_stride, pixel_stride, ax, tab_x, x0 * C + 4 * j, wide4);
  }
  __syncthreads();
  for (int item = threadIdx.x; item < RS_TH * ROW_WORDS; item += RS_WG) {
    const int jr = item / ROW_WORDS, j = item - jr * ROW_WORDS;
    const int y = y0 + jr, b0 = x0 * C + 4 * j;
    if (y >= ay.n_out || b0 >= row_bytes) continue;
    int first, taps;
    const int* k;
    rs_taps(ay, tab_y, y, first, taps, k);
    unsigned acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = 1u << (RS_BITS - 1);
    for (int i = 0; i < taps; ++i) {
      const int lr = min(max(first + i - r0, 0), rows_cap - 1);
      rs_vacc(acc, s_mid[lr * PITCH + j], (unsigned)k[i]);
    }
    rs_store<VEC>(dst + ((long)n * ay.n_out + y) * row_bytes, b0, row_bytes, acc);
  }
}

static inline int rs_lds_bytes(int C, int rows) { return rows * (RS_TW * C + 4); }

extern "C" int msmd_resize_fits(int C, int rows_span) {
  if (C != 1 && C != 3 && C != 4) return 0;
  return rows_span >= 1 && rows_span <= MSMD_RESIZE_LDS_BYTES / (RS_TW * C + 4);
}

// Fused where it fits, except where it was measured slower: neighbouring tiles repeat the horizontal pass for
// the rows they share, and where that is more than one multiply-add per intermediate byte while the two-pass form's
// intermediate is small enough to stay in the last-level cache, the two launches win.
extern "C" int msmd_resize_route(int C, int rows_span, int N, int Hs, int Hd, int Wd, int kx) {
  if (!msmd_resize_fits(C, rows_span)) return MSMD_RESIZE_TWO_PASS;
  const long tiles_y = (Hd + RS_TH - 1) / RS_TH;
  const bool repeats = ((long)rows_span * tiles_y - Hs) * kx > Hs;
  const bool cached = (long)N * Hs * Wd * C <= (long)MSMD_RESIZE_CACHE_BYTES;
  return repeats && cached ? MSMD_RESIZE_TWO_PASS : MSMD_RESIZE_FUSED;
}

template <int C>
static int resize_launch(const unsigned char* src, long frame_stride, long row_stride, int pixel_stride, int N, int Hs, RsAxis ax,
                         RsAxis ay, const int* table_of_frame, unsigned char* dst, unsigned char* mid, int rows_span, int form,
                         hipStream_t st) {
  const int row_bytes = ax.n_out * C, row_words = (row_bytes + 3) / 4;
  const bool wide4 = C == 4 && pixel_stride == 4 && (uintptr_t)src % 4 == 0 && row_stride % 4 == 0 && frame_stride % 4 == 0;
  const bool vec_dst = row_bytes % 4 == 0 && (uintptr_t)dst % 4 == 0;
  if (form == MSMD_RESIZE_FUSED) {
    const int tiles_x = (ax.n_out + RS_TW - 1) / RS_TW, tiles_y = (ay.n_out + RS_TH - 1) / RS_TH;
    const long blocks = (long)N * tiles_x * tiles_y;
    if (blocks > 2147483647L) return 1;
    const size_t lds = (size_t)rs_lds_bytes(C, rows_span);
    if (vec_dst)
      hipLaunchKernelGGL((resize_fused_kernel<C, true>), dim3((unsigned)blocks), dim3(RS_WG), lds, st, src, frame_stride, row_stride,
                         pixel_stride, ax, ay, table_of_frame, dst, rows_span, tiles_x, tiles_y, wide4);
    else
      hipLaunchKernelGGL((resize_fused_kernel<C, false>), dim3((unsigned)blocks), dim3(RS_WG), lds, st, src, frame_stride, row_stride,
                         pixel_stride, ax, ay, table_of_frame, dst, rows_span, tiles_x, tiles_y, wide4);
    MSMD_RETURN_LAST();
  }
  const long h_blocks = ((long)N * Hs * row_words + RS_WG - 1) / RS_WG, v_blocks = ((long)N * ay.n_out * row_words + RS_WG - 1) / RS_WG;
  if (h_blocks > 2147483647L || v_blocks > 2147483647L) return 1;
  const bool vec = row_bytes % 4 == 0 && (uintptr_t)mid % 4 == 0;
  if (vec)
    hipLaunchKernelGGL((resize_h_kernel<C, true>), dim3((unsigned)h_blocks), dim3(RS_WG), 0, st, src, frame_stride, row_stride,
                       pixel_stride, N, Hs, ax, table_of_frame, mid, wide4);
  else
    hipLaunchKernelGGL((resize_h_kernel<C, false>), dim3((unsigned)h_blocks), dim3(RS_WG), 0, st, src, frame_stride, row_stride,
                       pixel_stride, N, Hs, ax, table_of_frame, mid, wide4);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (vec && vec_dst)
    hipLaunchKernelGGL((resize_v_kernel<true>), dim3((unsigned)v_blocks), dim3(RS_WG), 0, st, mid, N, row_bytes, ay, table_of_frame, dst);
  else
    hipLaunchKernelGGL((resize_v_kernel<false>), dim3((unsigned)v_blocks), dim3(RS_WG), 0, st, mid, N, row_bytes, ay, table_of_frame, dst);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_resize_u8(const void* src, long frame_stride, long row_stride, int pixel_stride, int N, int Hs, int Ws, int C,
                              const int* xbounds, const int* xcoef, int kx, int Tx, const int* ybounds, const int* ycoef, int ky,
                              int Ty, const int* table_of_frame, void* dst, int Hd, int Wd, void* workspace, int rows_span,
                              int form, msmd_stream_t stream) {
  if (N < 0 || (C != 1 && C != 3 && C != 4)) return 1;
  if (!(pixel_stride == C || (C == 3 && pixel_stride == 4))) return 1;
  if (Hs < 1 || Hs > MSMD_JPEG_MAX_SIDE || Ws < 1 || Ws > MSMD_JPEG_MAX_SIDE) return 1;
  if (Hd < 1 || Hd > MSMD_JPEG_MAX_SIDE || Wd < 1 || Wd > MSMD_JPEG_MAX_SIDE) return 1;
  if (kx < 1 || ky < 1 || Tx < 1 || Ty < 1) return 1;
  if (form != MSMD_RESIZE_AUTO && form != MSMD_RESIZE_FUSED && form != MSMD_RESIZE_TWO_PASS) return 1;
  // the last byte read of a row is its last pixel's channel C - 1: rows and frames must not overlap
  if (row_stride < (long)(Ws - 1) * pixel_stride + C) return 1;
  if (N > 1 && frame_stride < (long)(Hs - 1) * row_stride + (long)(Ws - 1) * pixel_stride + C) return 1;
  if (form == MSMD_RESIZE_FUSED && !msmd_resize_fits(C, rows_span)) return 1;
  if (form == MSMD_RESIZE_AUTO) form = msmd_resize_route(C, rows_span, N, Hs, Hd, Wd, kx);
  if (N == 0) return 0;      // an empty batch has empty buffers: no pointer, the workspace included, is looked at
  if (form == MSMD_RESIZE_TWO_PASS && !workspace) return 1;
  if (!src || !dst || !xbounds || !xcoef || !ybounds || !ycoef || !table_of_frame) return 1;
  const RsAxis ax{xbounds, xcoef, kx, Tx, Ws, Wd}, ay{ybounds, ycoef, ky, Ty, Hs, Hd};
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* s = (const unsigned char*)src;
  unsigned char *d = (unsigned char*)dst, *m = (unsigned char*)workspace;
  if (C == 1) return resize_launch<1>(s, frame_stride, row_stride, pixel_stride, N, Hs, ax, ay, table_of_frame, d, m, rows_span, form, st);
  if (C == 3) return resize_launch<3>(s, frame_stride, row_stride, pixel_stride, N, Hs, ax, ay, table_of_frame, d, m, rows_span, form, st);
  return resize_launch<4>(s, frame_stride, row_stride, pixel_stride, N, Hs, ax, ay, table_of_frame, d, m, rows_span, form, st);
}
