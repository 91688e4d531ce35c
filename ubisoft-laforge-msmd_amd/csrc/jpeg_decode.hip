// Baseline JPEG decoder, the inverse of jpeg.hip: B files of one size and sampling in one byte stream on the
// device -> (B, H, W, 3 | 4) uint8.  The host has read the marker segments and found the restart intervals (jpeg_format.py);
// here: (A) the entropy decode, one lane per (frame, interval), int16 coefficients per component plane in block-raster order;
// (B) dequantise + inverse DCT per block, uint8 planes padded to whole blocks; (C) chroma upsampling and colour per output
// pixel.  Integer arithmetic throughout, no global atomics but the OR into status[frame], nothing the host waits for.
#include "jpeg_common.h"

namespace {

#define JD_LANES MSMD_JPEG_DECODE_LANES
#define JD_Q_BYTES 192                                           // three quantiser tables in front of a table set
#define JD_TAB_WORDS ((MSMD_JPEG_TABLE_SET_BYTES - JD_Q_BYTES) / 4)   // selectors (2 words) + four Huffman tables
#define JD_HUFF_WORDS 96                                         // maxcode[16], delta[16], HUFFVAL[256]
#define JD_IDCT_BLOCKS 32                                        // blocks per workgroup of (B): 8 lanes per block
#define JD_THREADS 256
static_assert(JD_TAB_WORDS == 2 + 4 * JD_HUFF_WORDS, "table set layout");
static_assert(JD_LANES == 64, "one wave per workgroup of the entropy decode");

__constant__ Perm64 c_zz2nat = kZz2Nat;   // zig-zag position -> natural index (row * 8 + column)

// Geometry of a frame.  Component 0 has hs x vs blocks per MCU, the others one; every index below is a compile-time constant
// after unrolling, so the record lives in registers.
struct DecGeo {
  int ncomp, hs, vs, mcux, mcuy, n_mcu;
  int bw0, bh0, bwc, bhc;      // blocks across / down: component 0, components 1 and 2
  int cw, ch;                  // true size of a chrominance plane
  long base1, base2, blocks;   // first block of planes 1 and 2, blocks of a frame
};
__device__ __host__ __forceinline__ bool dec_geo(int H, int W, int layout, DecGeo* g) {
  if (jpeg_sides_bad(H, W) || layout < MSMD_JPEG_GREY || layout > MSMD_JPEG_420) return false;
  g->ncomp = layout == MSMD_JPEG_GREY ? 1 : 3;
  g->hs = layout >= MSMD_JPEG_422 ? 2 : 1;
  g->vs = layout == MSMD_JPEG_420 ? 2 : 1;
  g->mcux = (W + 8 * g->hs - 1) / (8 * g->hs);
  g->mcuy = (H + 8 * g->vs - 1) / (8 * g->vs);
  g->n_mcu = g->mcux * g->mcuy;
  g->bw0 = g->mcux * g->hs; g->bh0 = g->mcuy * g->vs;
  g->bwc = g->mcux; g->bhc = g->mcuy;
  g->cw = (W + g->hs - 1) / g->hs; g->ch = (H + g->vs - 1) / g->vs;
  g->base1 = (long)g->bw0 * g->bh0;
  g->base2 = g->base1 + (long)g->bwc * g->bhc;
  g->blocks = g->ncomp == 1 ? g->base1 : g->base2 + (long)g->bwc * g->bhc;
  return true;
}

// ------------------------------------------------------------------------------------------------ (A) entropy decode
// The bit reader of one lane: bytes of [p, end) with the 0x00 behind a 0xFF dropped, zero bits behind the last byte.  acc holds
// n bits left-aligned; `fake` counts the zero bits supplied past the end, which are always the last ones in acc, so bits past
// the end have been consumed exactly when n < fake.
struct Bits {
  const unsigned char* p;
  const unsigned char* end;
  unsigned long acc;
  int n, fake;
  __device__ __forceinline__ void fill() {                       // afterwards n >= 57: a 16-bit code and 16 extra bits
    while (n <= 56) {
      unsigned b = 0;
      if (p < end) {
        b = *p++;
        if (b == 0xFFu && p < end && *p == 0) ++p;
      } else {
        fake += 8;
      }
      acc |= (unsigned long)b << (56 - n);
      n += 8;
    }
  }
  __device__ __forceinline__ void skip(int s) { acc <<= s; n -= s; }      // 0 < s <= 16
  __device__ __forceinline__ int receive(int s) {                        // 0 <= s <= 16
    if (s == 0) return 0;
    const int v = (int)(acc >> (64 - s));
    skip(s);
    return v;
  }
  __device__ __forceinline__ bool overrun() const { return n < fake; }
};

__device__ __forceinline__ int extend(int v, int s) { return (s != 0 && v < (1 << (s - 1))) ? v - (1 << s) + 1 : v; }
__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }

// One Huffman code from a canonical table in LDS (T.81 F.2.2.3): the symbol, or -1 where no code of 16 bits or fewer matches.
__device__ __forceinline__ int huff_decode(Bits& b, const int* t) {
  b.fill();
  const int peek = (int)(b.acc >> 48);
  for (int l = 1; l <= 16; ++l) {
    const int code = peek >> (16 - l);
    if (code <= t[l - 1]) {
      b.skip(l);
      return ((const unsigned char*)(t + 32))[(code + t[16 + l - 1]) & 255];
    }
  }
  return -1;
}

// One block into out[0 .. 63] (zero before): 0, or the error bit that ended it.
__device__ __forceinline__ int decode_block(Bits& b, const int* dc, const int* ac, int& pred, short* __restrict__ out) {
  {
    const int s = huff_decode(b, dc);
    if (s < 0 || s > 16) return MSMD_JPEG_ERR_CODE;
    const int diff = extend(b.receive(s), s);
    if (b.overrun()) return MSMD_JPEG_ERR_OVERRUN;
    pred = sat16(pred + diff);
    if (pred != 0) out[0] = (short)pred;
  }
  int k = 1;
  while (k < 64) {
    const int sym = huff_decode(b, ac);
    if (sym < 0) return MSMD_JPEG_ERR_CODE;
    const int r = sym >> 4, s = sym & 15;
    const int v = extend(b.receive(s), s);
    if (b.overrun()) return MSMD_JPEG_ERR_OVERRUN;
    if (s == 0) {
      if (r != 15) break;
      k += 16;
      if (k > 63) return MSMD_JPEG_ERR_RUN;
      continue;
    }
    k += r;
    if (k > 63) return MSMD_JPEG_ERR_RUN;
    out[k] = (short)sat16(v);
    ++k;
  }
  return 0;
}

// One wave per workgroup, one lane per row of the interval table.  The workgroup's table set (its first row's; the host pads the
// table where the set changes) is staged in LDS in canonical form: 2 + 4 x 96 words = 1544 bytes.
__global__ __launch_bounds__(JD_LANES) void jpeg_entropy_kernel(const unsigned char* __restrict__ stream, long n_bytes,
                                                                const long* __restrict__ intervals,
                                                                const unsigned char* __restrict__ sets, int n_sets, int B, int H,
                                                                int W, int layout, int ri, short* __restrict__ coef,
                                                                int* __restrict__ status) {
  __shared__ int s_tab[JD_TAB_WORDS];
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * JD_LANES;
  const int wg_set = (int)(intervals[3 * row0 + 2] >> 32);
  if (wg_set < 0 || wg_set >= n_sets) return;
  const int* src = (const int*)(sets + (long)wg_set * MSMD_JPEG_TABLE_SET_BYTES + JD_Q_BYTES);
  for (int i = tid; i < JD_TAB_WORDS; i += JD_LANES) s_tab[i] = src[i];
  __syncthreads();
  const long* row = intervals + 3 * (row0 + tid);
  const long off = row[0], w1 = row[1], w2 = row[2];
  const int len = (int)(unsigned)w1, frame = (int)(w1 >> 32), mcu0 = (int)(unsigned)w2, set = (int)(w2 >> 32);
  DecGeo g;
  dec_geo(H, W, layout, &g);
  if (frame < 0 || frame >= B || set != wg_set || mcu0 < 0 || mcu0 >= g.n_mcu || len < 0 || off < 0 || off > n_bytes - len) return;
  const unsigned sel0 = (unsigned)s_tab[0], sel1 = (unsigned)s_tab[1];       // bytes Td0 Ta0 Td1 Ta1 | Td2 Ta2 0 0
  const int* dc0 = s_tab + 2 + (sel0 & 1u) * JD_HUFF_WORDS;
  const int* ac0 = s_tab + 2 + (2 + ((sel0 >> 8) & 1u)) * JD_HUFF_WORDS;
  const int* dc1 = s_tab + 2 + ((sel0 >> 16) & 1u) * JD_HUFF_WORDS;
  const int* ac1 = s_tab + 2 + (2 + ((sel0 >> 24) & 1u)) * JD_HUFF_WORDS;
  const int* dc2 = s_tab + 2 + (sel1 & 1u) * JD_HUFF_WORDS;
  const int* ac2 = s_tab + 2 + (2 + ((sel1 >> 8) & 1u)) * JD_HUFF_WORDS;
  Bits b;
  b.p = stream + off; b.end = b.p + len; b.acc = 0; b.n = 0; b.fake = 0;
  short* fc = coef + (long)frame * g.blocks * 64;
  const int m_end = ri > 0 ? min(mcu0 + ri, g.n_mcu) : g.n_mcu;
  int my = mcu0 / g.mcux, mx = mcu0 - my * g.mcux;
  int p0 = 0, p1 = 0, p2 = 0, err = 0;
  for (int m = mcu0; m < m_end && err == 0; ++m) {
    for (int by = 0; by < g.vs && err == 0; ++by)
      for (int bx = 0; bx < g.hs && err == 0; ++bx) {
        const long blk = (long)(my * g.vs + by) * g.bw0 + mx * g.hs + bx;
        err = decode_block(b, dc0, ac0, p0, fc + blk * 64);
      }
    if (g.ncomp == 3) {
      const long blk = (long)my * g.bwc + mx;
      if (err == 0) err = decode_block(b, dc1, ac1, p1, fc + (g.base1 + blk) * 64);
      if (err == 0) err = decode_block(b, dc2, ac2, p2, fc + (g.base2 + blk) * 64);
    }
    if (++mx == g.mcux) { mx = 0; ++my; }
  }
  if (err) atomicOr(&status[frame], err);
}

// ------------------------------------------------------------------------------------------------ (B) dequantise, inverse DCT
// 256 lanes = 32 blocks x 8.  Lane (block, r) loads zig-zag coefficients 8 r .. 8 r + 7 with one 16-byte load, multiplies by
// Q and scatters F into the LDS block in natural order; pass 1 per (block, column) in int64 (< 2^40) into a second LDS block;
// pass 2 per (block, row) in int64 (< 2^57); round, level shift, clamp; one 8-byte store of the row into the plane.
__global__ __launch_bounds__(JD_THREADS) void jpeg_idct_kernel(const short* __restrict__ coef, const unsigned char* __restrict__ sets,
                                                               int n_sets, const int* __restrict__ frame_set, int B, int H, int W,
                                                               int layout, unsigned char* __restrict__ planes) {
  __shared__ int s_f[JD_IDCT_BLOCKS * 8 * JPEG_ROW];
  __shared__ long s_t[JD_IDCT_BLOCKS * 8 * JPEG_ROW];
  const int tid = threadIdx.x, blk = tid >> 3, r = tid & 7;
  DecGeo g;
  dec_geo(H, W, layout, &g);
  const long gb = (long)blockIdx.x * JD_IDCT_BLOCKS + blk;
  const long frame = gb / g.blocks, in_frame = gb - frame * g.blocks;
  int set = -1;
  if (frame < B) set = frame_set[frame];
  const bool live = set >= 0 && set < n_sets;
  const int comp = g.ncomp == 1 ? 0 : (in_frame >= g.base1) + (in_frame >= g.base2);
  int* f = s_f + blk * 8 * JPEG_ROW;
  long* t = s_t + blk * 8 * JPEG_ROW;
  if (live) {
    const u32x4 c = *(const u32x4*)(coef + gb * 64 + r * 8);
    const u32x2 q = *(const u32x2*)(sets + (long)set * MSMD_JPEG_TABLE_SET_BYTES + comp * 64 + r * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int cv = (int)(short)(c[e >> 1] >> (16 * (e & 1)));
      const int qv = (int)((q[e >> 2] >> (8 * (e & 3))) & 255u);
      const int nat = c_zz2nat.v[r * 8 + e];
      f[(nat >> 3) * JPEG_ROW + (nat & 7)] = cv * qv;
    }
  }
  __syncthreads();
  if (live) {                                                     // pass 1: column r, t[n][r] = sum_k M[k][n] F[k][r]
    int col[8];
    long o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k] = f[k * JPEG_ROW + r];
    idct8<int>(col, o);
#pragma unroll
    for (int n = 0; n < 8; ++n) t[n * JPEG_ROW + r] = o[n];
  }
  __syncthreads();
  if (live) {                                                     // pass 2: row r, x[r][m] = sum_l t[r][l] M[l][m]
    long in[8], o[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) in[l] = t[r * JPEG_ROW + l];
    idct8<long>(in, o);
    unsigned w[2] = {0u, 0u};
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const long s = ((o[m] + (1L << 29)) >> 30) + 128;
      const unsigned u = (unsigned)(s < 0 ? 0 : (s > 255 ? 255 : s));
      w[m >> 2] |= u << (8 * (m & 3));
    }
    const long base = comp == 0 ? 0 : (comp == 1 ? g.base1 : g.base2);
    const int bw = comp == 0 ? g.bw0 : g.bwc;
    const long bi = in_frame - base;
    const long by = bi / bw, bx = bi - by * bw;
    unsigned char* dst = planes + (frame * g.blocks + base) * 64 + (by * 8 + r) * ((long)bw * 8) + bx * 8;
    *(u32x2*)dst = u32x2{w[0], w[1]};
  }
}

// ------------------------------------------------------------------------------------------------ (C) upsample, colour
// Sample (y, x) of a chrominance plane after upsampling; p = the plane, pitch bytes a row, true size ch x cw.
template <int LAYOUT> __device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int pitch, int cw, int ch, int y, int x) {
  if (LAYOUT == MSMD_JPEG_444) return p[(long)y * pitch + x];
  const int i = x >> 1;
  const int in = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);   // the neighbour; at an edge it is the sample itself
  if (LAYOUT == MSMD_JPEG_422) {
    const unsigned char* row = p + (long)y * pitch;
    if ((x & 1) ? i == cw - 1 : i == 0) return row[i];
    return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int j = y >> 1;
  const int jn = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
  const unsigned char* a = p + (long)j * pitch;
  const unsigned char* bq = p + (long)jn * pitch;
  const int r = 3 * a[i] + bq[i], rn = 3 * a[in] + bq[in];       // rn = r at an edge: 3 r + r = 4 r
  return (3 * r + rn + ((x & 1) ? 7 : 8)) >> 4;
}

// pixel (y, x) of one frame -> R | G << 8 | B << 16 | 255 << 24
template <int LAYOUT> __device__ __forceinline__ unsigned pixel_at(const unsigned char* __restrict__ fp, const DecGeo& g, int y, int x) {
  const int Y = fp[(long)y * (g.bw0 * 8) + x];
  if (LAYOUT == MSMD_JPEG_GREY) return (unsigned)Y * 0x010101u | 0xFF000000u;
  const int pitch = g.bwc * 8;
  const int cb = chroma_at<LAYOUT>(fp + g.base1 * 64, pitch, g.cw, g.ch, y, x) - 128;
  const int cr = chroma_at<LAYOUT>(fp + g.base2 * 64, pitch, g.cw, g.ch, y, x) - 128;
  const int R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
  const int G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
  const int Bv = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
  return (unsigned)R | (unsigned)G << 8 | (unsigned)Bv << 16 | 0xFF000000u;
}

// CH = 4: a lane writes one 4-byte pixel.  CH = 3: a lane owns four consecutive pixels of the flat (B H W) order, 12 bytes at a
// multiple of 12: three 4-byte words in one store; the last lane of the call may own fewer and writes bytes.
template <int LAYOUT, int CH> __global__ __launch_bounds__(JD_THREADS) void jpeg_pixels_kernel(const unsigned char* __restrict__ planes,
                                                                                               int B, int H, int W,
                                                                                               unsigned char* __restrict__ out) {
  DecGeo g;
  dec_geo(H, W, LAYOUT, &g);
  const long n_pix = (long)B * H * W, hw = (long)H * W;
  const long i = (long)blockIdx.x * JD_THREADS + threadIdx.x;
  if (CH == 4) {
    if (i >= n_pix) return;
    const long b = i / hw, rem = i - b * hw;
    const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
    ((unsigned*)out)[i] = pixel_at<LAYOUT>(planes + b * g.blocks * 64, g, y, x);
  } else {
    const long first = 4 * i;
    if (first >= n_pix) return;
    const int n = (int)min(4L, n_pix - first);
    long b = first / hw, rem = first - b * hw;
    int y = (int)(rem / W), x = (int)(rem - (long)y * W);
    unsigned px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < n) px[e] = pixel_at<LAYOUT>(planes + b * g.blocks * 64, g, y, x) & 0xFFFFFFu;
      if (++x == W) {
        x = 0;
        if (++y == H) { y = 0; ++b; }
      }
    }
    unsigned char* dst = out + 3 * first;
    if (n == 4) {
      I3 w;
      w.a = (int)(px[0] | px[1] << 24);
      w.b = (int)(px[1] >> 8 | px[2] << 16);
      w.c = (int)(px[2] >> 16 | px[3] << 8);
      *(I3*)dst = w;
    } else {
      for (int e = 0; e < n; ++e) {
        dst[3 * e] = (unsigned char)px[e];
        dst[3 * e + 1] = (unsigned char)(px[e] >> 8);
        dst[3 * e + 2] = (unsigned char)(px[e] >> 16);
      }
    }
  }
}

template <int LAYOUT> int launch_pixels(const unsigned char* planes, int B, int H, int W, int channels, unsigned char* out, hipStream_t st) {
  const long n_pix = (long)B * H * W;
  const long lanes = channels == 4 ? n_pix : (n_pix + 3) / 4;
  const long grid = (lanes + JD_THREADS - 1) / JD_THREADS;
  if (grid > 2147483647L) return 1;
  if (channels == 4)
    hipLaunchKernelGGL((jpeg_pixels_kernel<LAYOUT, 4>), dim3((unsigned)grid), dim3(JD_THREADS), 0, st, planes, B, H, W, out);
  else
    hipLaunchKernelGGL((jpeg_pixels_kernel<LAYOUT, 3>), dim3((unsigned)grid), dim3(JD_THREADS), 0, st, planes, B, H, W, out);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" long msmd_jpeg_decode_blocks(int H, int W, int layout) {
  DecGeo g;
  return dec_geo(H, W, layout, &g) ? g.blocks : -1L;
}

extern "C" int msmd_jpeg_decode_coefficients(const void* stream_bytes, long n_bytes, const long* intervals, int n_entries,
                                             const void* table_sets, int n_sets, int B, int H, int W, int layout,
                                             int restart_interval, short* coef, int* status, msmd_stream_t stream) {
  DecGeo g;
  if (!dec_geo(H, W, layout, &g) || B <= 0 || n_bytes <= 0 || n_entries <= 0 || n_entries % JD_LANES != 0 || n_sets < 1 ||
      restart_interval < 0 || stream_bytes == nullptr || intervals == nullptr || table_sets == nullptr || coef == nullptr ||
      status == nullptr || ((uintptr_t)table_sets & 7) != 0 || ((uintptr_t)coef & 15) != 0 || (long)B * g.blocks > (1L << 33))
    return 1;
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t z = msmd_zero_async(coef, (size_t)B * (size_t)g.blocks * 128, st);
  if (z != hipSuccess) return (int)z;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)(n_entries / JD_LANES)), dim3(JD_LANES), 0, st,
                     (const unsigned char*)stream_bytes, n_bytes, intervals, (const unsigned char*)table_sets, n_sets, B, H, W, layout,
                     restart_interval, coef, status);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_jpeg_decode_planes(const short* coef, const void* table_sets, int n_sets, const int* frame_set, int B, int H,
                                       int W, int layout, void* planes, msmd_stream_t stream) {
  DecGeo g;
  if (!dec_geo(H, W, layout, &g) || B <= 0 || n_sets < 1 || coef == nullptr || table_sets == nullptr || frame_set == nullptr ||
      planes == nullptr || ((uintptr_t)table_sets & 7) != 0 || ((uintptr_t)coef & 15) != 0 || ((uintptr_t)planes & 7) != 0)
    return 1;
  const long grid = ((long)B * g.blocks + JD_IDCT_BLOCKS - 1) / JD_IDCT_BLOCKS;
  if (grid > 2147483647L) return 1;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)grid), dim3(JD_THREADS), 0, (hipStream_t)stream, coef,
                     (const unsigned char*)table_sets, n_sets, frame_set, B, H, W, layout, (unsigned char*)planes);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_jpeg_decode_pixels(const void* planes, int B, int H, int W, int layout, int channels, void* pixels,
                                       msmd_stream_t stream) {
  DecGeo g;
  if (!dec_geo(H, W, layout, &g) || B <= 0 || (channels != 3 && channels != 4) || planes == nullptr || pixels == nullptr ||
      ((uintptr_t)pixels & 3) != 0)
    return 1;
  const unsigned char* p = (const unsigned char*)planes;
  unsigned char* o = (unsigned char*)pixels;
  const hipStream_t st = (hipStream_t)stream;
  switch (layout) {
    case MSMD_JPEG_GREY: return launch_pixels<MSMD_JPEG_GREY>(p, B, H, W, channels, o, st);
    case MSMD_JPEG_444: return launch_pixels<MSMD_JPEG_444>(p, B, H, W, channels, o, st);
    case MSMD_JPEG_422: return launch_pixels<MSMD_JPEG_422>(p, B, H, W, channels, o, st);
    default: return launch_pixels<MSMD_JPEG_420>(p, B, H, W, channels, o, st);
  }
}
