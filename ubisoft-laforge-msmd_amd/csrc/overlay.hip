// Overlays: discs, capsules, boxes and 8 x 8 glyphs drawn onto 8-bit frames, stated in include/msmd_hip.h.
// Integer VALU code only.  One launch: a workgroup owns a tile of one frame, scans the frame's records a chunk at a time, keeps
// the ones whose bounding box meets the tile in LDS in their order, and every pixel walks that list.
#include "common.h"

constexpr int OV_WG = 256;
constexpr int OV_TW = MSMD_OVERLAY_TILE_W, OV_TH = MSMD_OVERLAY_TILE_H, OV_CHUNK = MSMD_OVERLAY_CHUNK;
constexpr int OV_PX = 4;                          // horizontally adjacent pixels of one thread
constexpr int OV_ENTRY = 16;                      // words of one LDS entry: the record, its bounding box, a glyph's eight rows
static_assert(OV_TW * OV_TH == OV_WG * OV_PX && OV_TW % OV_PX == 0, "one thread per four pixels of the tile");
static_assert(OV_CHUNK == OV_WG, "one record per thread and chunk");

// A record as the pixels read it from LDS (every lane the same address: a broadcast).
struct OvRec {
  int kind, x0, y0, x1, y1, r, aux;
  unsigned colour;
  int bx0, by0, bx1, by1;                         // conservative bounding box, inclusive, 1/16 px
  unsigned rows_lo, rows_hi;                      // glyph rows 0 .. 3 and 4 .. 7, row v in byte v % 4
};

// Whether the record draws at all (the header's list), and its bounding box.
__device__ __forceinline__ bool ov_prepare(const int* __restrict__ rec, const unsigned char* __restrict__ font, int n_glyphs, int* e) {
  const int kind = rec[0], x0 = rec[1], y0 = rec[2], x1 = rec[3], y1 = rec[4], r = rec[5], aux = rec[6];
  constexpr int MC = MSMD_OVERLAY_MAX_COORD, MR = MSMD_OVERLAY_MAX_RADIUS;
  if (kind < MSMD_OVERLAY_DISC || kind > MSMD_OVERLAY_GLYPH) return false;
  if (x0 < -MC || x0 > MC || y0 < -MC || y0 > MC || r < 0 || r > MR || aux < 0 || aux > MR) return false;
  int bx0, by0, bx1, by1;
  unsigned lo = 0, hi = 0;
  if (kind == MSMD_OVERLAY_GLYPH) {
    if (x1 < 1 || x1 > MR || y1 < 0 || y1 >= n_glyphs) return false;
    bx0 = x0; by0 = y0; bx1 = x0 + 8 * x1 - 1; by1 = y0 + 8 * x1 - 1;
    const unsigned char* g = font + (long)y1 * 8;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      lo |= (unsigned)g[v] << (8 * v);
      hi |= (unsigned)g[4 + v] << (8 * v);
    }
  } else {
    if (x1 < -MC || x1 > MC || y1 < -MC || y1 > MC) return false;
    if (kind == MSMD_OVERLAY_DISC) {
      bx0 = x0 - r; bx1 = x0 + r; by0 = y0 - r; by1 = y0 + r;
    } else if (kind == MSMD_OVERLAY_CAPSULE) {
      bx0 = min(x0, x1) - r; bx1 = max(x0, x1) + r; by0 = min(y0, y1) - r; by1 = max(y0, y1) + r;
    } else {
      bx0 = x0; bx1 = x1; by0 = y0; by1 = y1;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) e[i] = rec[i];
  e[8] = bx0; e[9] = by0; e[10] = bx1; e[11] = by1;
  e[12] = (int)lo; e[13] = (int)hi;
  return true;
}

// a <= b for the 128-bit values (ahi, alo), (bhi, blo)
__device__ __forceinline__ bool ov_le128(unsigned long ahi, unsigned long alo, unsigned long bhi, unsigned long blo) {
  return ahi < bhi || (ahi == bhi && alo <= blo);
}

// One sample point against one record; the kind is the same for every lane.
__device__ __forceinline__ bool ov_inside(const OvRec& R, int px, int py) {
  const long qx = (long)px - R.x0, qy = (long)py - R.y0;
  if (R.kind == MSMD_OVERLAY_DISC) {
    const long d2 = qx * qx + qy * qy;
    return (long)R.aux * R.aux <= d2 && d2 <= (long)R.r * R.r;
  }
  if (R.kind == MSMD_OVERLAY_CAPSULE) {
    const long dx = (long)R.x1 - R.x0, dy = (long)R.y1 - R.y0, r2 = (long)R.r * R.r;
    const long L = dx * dx + dy * dy, s = qx * dx + qy * dy;
    if (s <= 0) return qx * qx + qy * qy <= r2;
    if (s >= L) {
      const long ex = (long)px - R.x1, ey = (long)py - R.y1;
      return ex * ex + ey * ey <= r2;
    }
    const long cr = qx * dy - qy * dx;                       // |cr| < 2^44: its square needs 128 bits
    const unsigned long m = (unsigned long)(cr < 0 ? -cr : cr);
    return ov_le128(__umul64hi(m, m), m * m, __umul64hi((unsigned long)r2, (unsigned long)L), (unsigned long)r2 * (unsigned long)L);
  }
  if (R.kind == MSMD_OVERLAY_BOX) {
    if (px < R.x0 || px > R.x1 || py < R.y0 || py > R.y1) return false;
    if (R.aux > 0 && px >= R.x0 + R.aux && px <= R.x1 - R.aux && py >= R.y0 + R.aux && py <= R.y1 - R.aux) return false;
    return true;
  }
  // glyph: qx, qy >= 0 makes the truncating division the floor division
  if (qx < 0 || qy < 0) return false;
  const unsigned u = (unsigned)qx / (unsigned)R.x1, v = (unsigned)qy / (unsigned)R.x1;
  if (u >= 8u || v >= 8u) return false;
  const unsigned row = ((v < 4u ? R.rows_lo : R.rows_hi) >> (8 * (v & 3u))) & 255u;
  return (row >> (7u - u)) & 1u;
}

// The number of the sample points of pixel (x, y) inside the record.
template <int S>
__device__ __forceinline__ int ov_coverage(const OvRec& R, int x, int y) {
  if constexpr (S == 1) {
    return ov_inside(R, 16 * x + 8, 16 * y + 8) ? 1 : 0;
  } else {
    int cov = 0;
    for (int j = 0; j < 4; ++j)
      for (int i = 0; i < 4; ++i) cov += ov_inside(R, 16 * x + 2 + 4 * i, 16 * y + 2 + 4 * j) ? 1 : 0;
    return cov;
  }
}

// The thread's pixels: NC channels of OV_PX pixels at (x .. x + 3, y); `n` of them lie inside the frame.  VEC: 4-byte aligned rows
// of adjacent C-byte pixels, C in {1, 3}: a full group of four is C whole words.
template <int NC, bool VEC>
__device__ __forceinline__ void ov_load(const unsigned char* __restrict__ p, int pixel_stride, int n, unsigned (*px)[NC]) {
  if (VEC && n == OV_PX) {
    const unsigned* w = (const unsigned*)p;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const unsigned word = w[k];
#pragma unroll
      for (int b = 0; b < 4; ++b) px[(4 * k + b) / NC][(4 * k + b) % NC] = (word >> (8 * b)) & 255u;
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < OV_PX; ++e)
    if (e < n) {
#pragma unroll
      for (int c = 0; c < NC; ++c) px[e][c] = p[(long)e * pixel_stride + c];
    }
}
template <int NC, bool VEC>
__device__ __forceinline__ void ov_store(unsigned char* __restrict__ p, int pixel_stride, int n, const unsigned (*px)[NC]) {
  if (VEC && n == OV_PX) {
    unsigned* w = (unsigned*)p;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      unsigned word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) word |= px[(4 * k + b) / NC][(4 * k + b) % NC] << (8 * b);
      w[k] = word;
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < OV_PX; ++e)
    if (e < n) {
#pragma unroll
      for (int c = 0; c < NC; ++c) p[(long)e * pixel_stride + c] = (unsigned char)px[e][c];
    }
}

template <int NC, int S, bool VEC>
__global__ __launch_bounds__(OV_WG) void overlay_kernel(const unsigned char* src, unsigned char* dst,
                                                        long frame_stride, long row_stride, int pixel_stride, int H, int W,
                                                        const int* __restrict__ prims, long n_prims,
                                                        const int* __restrict__ prim_offsets, const unsigned char* __restrict__ font,
                                                        int n_glyphs, int tiles_x, int tiles_y) {
  __shared__ int s_list[OV_CHUNK * OV_ENTRY];
  __shared__ int s_count[OV_WG / 64];
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, f = b / tiles_y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tx * OV_TW + (threadIdx.x % (OV_TW / OV_PX)) * OV_PX, y = ty * OV_TH + threadIdx.x / (OV_TW / OV_PX);
  const int n = y < H ? min(max(W - x, 0), OV_PX) : 0;         // the thread's pixels inside the frame
  // the tile's and the thread's sample points lie in these inclusive ranges (1/16 px); the first / last offset is 2 / 14 or 8 / 8
  constexpr int LO = S == 1 ? 8 : 2, HI = S == 1 ? 8 : 14;
  const int tile_x0 = 16 * tx * OV_TW + LO, tile_x1 = 16 * (min((tx + 1) * OV_TW, W) - 1) + HI;
  const int tile_y0 = 16 * ty * OV_TH + LO, tile_y1 = 16 * (min((ty + 1) * OV_TH, H) - 1) + HI;
  const int mine_x0 = 16 * x + LO, mine_x1 = 16 * (x + n - 1) + HI, mine_y0 = 16 * y + LO, mine_y1 = 16 * y + HI;
  const long at = (long)f * frame_stride + (long)y * row_stride + (long)x * pixel_stride;
  const long P = min(n_prims, 2147483647L);
  const long begin = min(max((long)prim_offsets[f], 0L), P), end = max(min(max((long)prim_offsets[f + 1], 0L), P), begin);

  unsigned px[OV_PX][NC];
#pragma unroll
  for (int e = 0; e < OV_PX; ++e)
#pragma unroll
    for (int c = 0; c < NC; ++c) px[e][c] = 0;
  bool loaded = false;                                        // the same in every thread of the workgroup

  for (long base = begin; base < end; base += OV_CHUNK) {
    const long idx = base + threadIdx.x;
    int entry[OV_ENTRY - 2];
    bool hit = false;
    if (idx < end && ov_prepare(prims + idx * 8, font, n_glyphs, entry))
      hit = entry[8] <= tile_x1 && entry[10] >= tile_x0 && entry[9] <= tile_y1 && entry[11] >= tile_y0;
    const unsigned long mask = __ballot(hit);
    if (lane == 0) s_count[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < OV_WG / 64; ++w) {
      const int c = s_count[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (hit) {
      int* slot = s_list + (before + __popcll(mask & ((1ul << lane) - 1ul))) * OV_ENTRY;
#pragma unroll
      for (int i = 0; i < OV_ENTRY - 2; ++i) slot[i] = entry[i];
    }
    __syncthreads();            // the list is whole; s_count is not written again before every wave has passed the next barrier
    if (total == 0) continue;
    if (!loaded) {
      if (n > 0) ov_load<NC, VEC>(src + at, pixel_stride, n, px);
      loaded = true;
    }
    for (int k = 0; k < total; ++k) {
      const int* e = s_list + k * OV_ENTRY;
      OvRec R;
      R.kind = e[0]; R.x0 = e[1]; R.y0 = e[2]; R.x1 = e[3]; R.y1 = e[4]; R.r = e[5]; R.aux = e[6];
      R.colour = (unsigned)e[7];
      R.bx0 = e[8]; R.by0 = e[9]; R.bx1 = e[10]; R.by1 = e[11];
      R.rows_lo = (unsigned)e[12]; R.rows_hi = (unsigned)e[13];
      const unsigned A = R.colour >> 24;
      if (n == 0 || A == 0u || R.bx0 > mine_x1 || R.bx1 < mine_x0 || R.by0 > mine_y1 || R.by1 < mine_y0) continue;
#pragma unroll
      for (int p = 0; p < OV_PX; ++p) {
        if (p >= n || R.bx0 > 16 * (x + p) + HI || R.bx1 < 16 * (x + p) + LO) continue;
        const int cov = ov_coverage<S>(R, x + p, y);
        if (cov == 0) continue;
        const unsigned w = (unsigned)cov * (16u / S) * A;
#pragma unroll
        for (int c = 0; c < NC; ++c)
          px[p][c] = (px[p][c] * (4080u - w) + ((R.colour >> (8 * c)) & 255u) * w + 2040u) / 4080u;
      }
    }
  }
  if (n == 0) return;
  if (!loaded) {
    if (src == dst) return;                                    // an untouched tile in place: nothing to write
    ov_load<NC, VEC>(src + at, pixel_stride, n, px);
  }
  ov_store<NC, VEC>(dst + at, pixel_stride, n, px);
}

template <int NC, int S>
static int overlay_launch(const unsigned char* src, unsigned char* dst, long frame_stride, long row_stride, int pixel_stride, int N,
                          int H, int W, const int* prims, long n_prims, const int* prim_offsets, const unsigned char* font,
                          int n_glyphs, hipStream_t st) {
  const int tiles_x = (W + OV_TW - 1) / OV_TW, tiles_y = (H + OV_TH - 1) / OV_TH;
  const long blocks = (long)N * tiles_x * tiles_y;
  if (blocks > 2147483647L) return 1;
  const bool vec = pixel_stride == NC && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0 && frame_stride % 4 == 0 && row_stride % 4 == 0;
  if (vec)
    hipLaunchKernelGGL((overlay_kernel<NC, S, true>), dim3((unsigned)blocks), dim3(OV_WG), 0, st, src, dst, frame_stride, row_stride,
                       pixel_stride, H, W, prims, n_prims, prim_offsets, font, n_glyphs, tiles_x, tiles_y);
  else
    hipLaunchKernelGGL((overlay_kernel<NC, S, false>), dim3((unsigned)blocks), dim3(OV_WG), 0, st, src, dst, frame_stride, row_stride,
                       pixel_stride, H, W, prims, n_prims, prim_offsets, font, n_glyphs, tiles_x, tiles_y);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_draw_overlay(const void* src, void* dst, long frame_stride, long row_stride, int pixel_stride, int N, int H, int W,
                                 int C, const int* prims, long n_prims, const int* prim_offsets, const unsigned char* font,
                                 int n_glyphs, int samples, msmd_stream_t stream) {
  if (N < 0 || n_prims < 0 || n_glyphs < 0 || (C != 1 && C != 3 && C != 4)) return 1;
  if (!(pixel_stride == C || (C == 3 && pixel_stride == 4))) return 1;
  if (H < 1 || H > MSMD_JPEG_MAX_SIDE || W < 1 || W > MSMD_JPEG_MAX_SIDE) return 1;
  if (samples != 1 && samples != 16) return 1;
  // the last byte of a row is its last pixel's channel C - 1: rows and frames must not overlap
  if (row_stride < (long)(W - 1) * pixel_stride + C) return 1;
  if (N > 1 && frame_stride < (long)(H - 1) * row_stride + (long)(W - 1) * pixel_stride + C) return 1;
  if (N == 0) return 0;
  if (!src || !dst || !prim_offsets || (n_prims > 0 && !prims) || (n_glyphs > 0 && !font)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* s = (const unsigned char*)src;
  unsigned char* d = (unsigned char*)dst;
  // a 4-channel pixel's fourth byte is never touched: three channels at a stride of four
#define OV_GO(NC, S) overlay_launch<NC, S>(s, d, frame_stride, row_stride, pixel_stride, N, H, W, prims, n_prims, prim_offsets, font, n_glyphs, st)
  if (C == 1) return samples == 1 ? OV_GO(1, 1) : OV_GO(1, 16);
  return samples == 1 ? OV_GO(3, 1) : OV_GO(3, 16);
#undef OV_GO
}
