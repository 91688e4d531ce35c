// Baseline JPEG encoder: (B, H, W, 3 | 4) uint8 frames on the device -> one JFIF byte stream per frame.
// 4:4:4, Annex K tables, a restart interval of 32 MCUs, which is the unit of parallelism.  Everything from pixels to bytes
// is integer arithmetic, so the file is a pure function of the frames.  Four kernels, no global atomics, no host
// synchronisation: coefficients; pack (run twice: once for the stuffed length of every interval, once to write the bytes at
// their final place); the two scans in between that turn lengths into offsets.
#include "jpeg_common.h"

namespace {

#define JP_RI MSMD_JPEG_RESTART_INTERVAL   // MCUs per restart interval = per workgroup
#define JP_BLOCKS (3 * JP_RI)              // 8 x 8 blocks of an interval: Y, Cb, Cr of each MCU
#define JP_THREADS 256
#define JP_BLK (8 * JPEG_ROW)
#define JP_BLOCK_BYTES 208                 // worst case of one block: 22 bits of DC + 63 x 26 bits of AC = 1660 bits
#define JP_WORDS (JP_BLOCKS * JP_BLOCK_BYTES / 4)

// T.81 Annex K.1, natural order
__constant__ unsigned char c_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
__constant__ Perm64 c_nat2zz = inverse(kZz2Nat);   // natural index -> position in the zig-zag scan

// T.81 Annex K.3: BITS and HUFFVAL of the four typical tables; the codes are derived at compile time (Annex C).
struct HuffSpec { unsigned char bits[16]; unsigned char vals[162]; int n; };
struct HuffTab { unsigned short code[256]; unsigned char len[256]; };
constexpr HuffTab make_huff(const HuffSpec s) {
  HuffTab t{};
  unsigned code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < s.bits[l - 1]; ++i, ++k, ++code) {
      t.code[s.vals[k]] = (unsigned short)code;
      t.len[s.vals[k]] = (unsigned char)l;
    }
    code <<= 1;
  }
  return t;
}
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};
// [0] luminance, [1] chrominance
__constant__ HuffTab c_dc[2] = {make_huff(kDcLuma), make_huff(kDcChroma)};
__constant__ HuffTab c_ac[2] = {make_huff(kAcLuma), make_huff(kAcChroma)};

// interval geometry shared by the kernels
struct Geo { int mcu_x, n_mcu, n_int; };
__device__ __host__ __forceinline__ Geo geo_of(int H, int W) {
  Geo g;
  g.mcu_x = (W + 7) >> 3;
  g.n_mcu = g.mcu_x * ((H + 7) >> 3);
  g.n_int = (g.n_mcu + JP_RI - 1) / JP_RI;
  return g;
}

// ------------------------------------------------------------------------------------------------ (A) coefficients
// One workgroup per (frame, interval): 32 MCUs = 96 blocks.  Pixels -> level-shifted YCbCr in LDS (a lane reads one pixel, a
// wave 64 consecutive ones of a row), pass 1 along rows in int32 in place (|t| <= 128 * 92680 < 2^24), pass 2 along columns in
// int64 (|c| <= 2^24 * 92680 < 2^41), the quantiser, and the zig-zag int16 block written with 16-byte stores.  MCUs past the
// frame's last one give zeros.
__global__ __launch_bounds__(JP_THREADS) void jpeg_coef_kernel(const unsigned char* __restrict__ frames, long frame_stride,
                                                               long row_stride, int pixel_stride, int wide, int H, int W,
                                                               int quality, short* __restrict__ coef) {
  __shared__ int s_px[JP_BLOCKS * JP_BLK];
  __shared__ __attribute__((aligned(16))) short s_zz[JP_BLOCKS * 64];
  __shared__ unsigned short s_q[2][64];
  const int tid = threadIdx.x;
  const Geo g = geo_of(H, W);
  const int b = blockIdx.x / g.n_int, it = blockIdx.x - b * g.n_int;
  if (tid < 128) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = ((int)c_base[tid >> 6][tid & 63] * scale + 50) / 100;
    s_q[tid >> 6][tid & 63] = (unsigned short)min(max(q, 1), 255);
  }
  const unsigned char* fb = frames + (long)b * frame_stride;
  for (int p = tid; p < JP_RI * 64; p += JP_THREADS) {
    const int r = p >> 8, m = (p >> 3) & (JP_RI - 1), px = p & 7;
    const int mcu = it * JP_RI + m;
    int yy = 0, cb = 0, cr = 0;
    if (mcu < g.n_mcu) {
      const int my = mcu / g.mcu_x, mx = mcu - my * g.mcu_x;
      const int y = min(my * 8 + r, H - 1), x = min(mx * 8 + px, W - 1);
      const unsigned char* pp = fb + (long)y * row_stride + (long)x * pixel_stride;
      int R, G, Bv;
      if (wide) {
        const unsigned u = *(const unsigned*)pp;
        R = u & 255; G = (u >> 8) & 255; Bv = (u >> 16) & 255;
      } else {
        R = pp[0]; G = pp[1]; Bv = pp[2];
      }
      yy = ((19595 * R + 38470 * G + 7471 * Bv + 32768) >> 16) - 128;
      cb = min(max(((-11059 * R - 21709 * G + 32768 * Bv + 32768) >> 16) + 128, 0), 255) - 128;
      cr = min(max(((32768 * R - 27439 * G - 5329 * Bv + 32768) >> 16) + 128, 0), 255) - 128;
    }
    int* o = s_px + (m * 3) * JP_BLK + r * JPEG_ROW + px;
    o[0] = yy; o[JP_BLK] = cb; o[2 * JP_BLK] = cr;
  }
  __syncthreads();
  for (int task = tid; task < JP_BLOCKS * 8; task += JP_THREADS) {      // pass 1: (block, row), in place
    int* row = s_px + (task >> 3) * JP_BLK + (task & 7) * JPEG_ROW;
    int x[8], t[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = row[n];
    dct8<int>(x, t);
#pragma unroll
    for (int n = 0; n < 8; ++n) row[n] = t[n];
  }
  __syncthreads();
  for (int task = tid; task < JP_BLOCKS * 8; task += JP_THREADS) {      // pass 2: (block, column), quantise
    const int blk = task >> 3, l = task & 7;
    const int* col = s_px + blk * JP_BLK + l;
    int t[8];
    long c[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) t[m] = col[m * JPEG_ROW];
    dct8<long>(t, c);
    const unsigned short* qt = s_q[(blk % 3) != 0];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int nat = k * 8 + l;
      const unsigned Q = qt[nat];
      const unsigned long a = (unsigned long)(c[k] < 0 ? -c[k] : c[k]);
      // (2 a + d) div (2 d) with d = Q 2^30 is ((2 a + d) >> 31) div Q: nested floor divisions compose; the shifted value is < 2^12
      const unsigned u = (unsigned)((2 * a + ((unsigned long)Q << (2 * JPEG_DCT_S))) >> (2 * JPEG_DCT_S + 1));
      int q = (int)(u / Q);
      if (nat != 0) q = min(q, 1023);
      s_zz[blk * 64 + c_nat2zz.v[nat]] = (short)(c[k] < 0 ? -q : q);
    }
  }
  __syncthreads();
  u32x4* dst = (u32x4*)(coef + ((long)blockIdx.x * JP_BLOCKS) * 64);
  for (int p = tid; p < JP_BLOCKS * 8; p += JP_THREADS) dst[p] = ((const u32x4*)s_zz)[p];
}

// ------------------------------------------------------------------------------------------------ (B, C) pack
__device__ __forceinline__ void put_bits(unsigned* s_bits, unsigned pos, unsigned val, int len) {     // 0 < len <= 26, val < 2^len
  const unsigned w = pos >> 5, o = pos & 31;
  const unsigned long v = (unsigned long)val << (64 - o - len);
  atomicOr(&s_bits[w], (unsigned)(v >> 32));                 // LDS; OR of disjoint bits: independent of arrival order
  const unsigned lo = (unsigned)v;
  if (lo) atomicOr(&s_bits[w + 1], lo);
}

// The codes of one block from its zig-zag coefficients: counted (EMIT = false) or written at bit `pos`.  Returns the bit count.
template <bool EMIT> __device__ __forceinline__ unsigned walk_block(const short* z, int pred, int tab, unsigned* s_bits, unsigned pos) {
  const unsigned start = pos;
  int diff = min(max((int)z[0] - pred, -2047), 2047);
  int mag = diff < 0 ? -diff : diff;
  int cat = 32 - __clz(mag);                                  // __clz(0) = 32
  {
    const unsigned code = c_dc[tab].code[cat];
    const int len = c_dc[tab].len[cat];
    const unsigned v = (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u);
    if (EMIT) put_bits(s_bits, pos, (code << cat) | v, len + cat);
    pos += len + cat;
  }
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = z[k];
    if (v == 0) { ++run; continue; }
    while (run >= 16) {
      if (EMIT) put_bits(s_bits, pos, c_ac[tab].code[0xF0], c_ac[tab].len[0xF0]);
      pos += c_ac[tab].len[0xF0];
      run -= 16;
    }
    mag = v < 0 ? -v : v;
    cat = 32 - __clz(mag);
    const int sym = (run << 4) | cat;
    const unsigned code = c_ac[tab].code[sym];
    const int len = c_ac[tab].len[sym];
    const unsigned bits = (unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
    if (EMIT) put_bits(s_bits, pos, (code << cat) | bits, len + cat);
    pos += len + cat;
    run = 0;
  }
  if (run > 0) {
    if (EMIT) put_bits(s_bits, pos, c_ac[tab].code[0], c_ac[tab].len[0]);
    pos += c_ac[tab].len[0];
  }
  return pos - start;
}

// exclusive prefix of v over the workgroup's threads in thread order (blockDim = JP_THREADS); *total = the sum
__device__ __forceinline__ long block_exclusive_scan(long v, long* s_w, long* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  __syncthreads();
  if (lane == 63) s_w[wid] = inc;
  __syncthreads();
  long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < JP_THREADS / 64; ++w) {
    const long c = s_w[w];
    if (w < wid) before += c;
    all += c;
  }
  *total = all;
  return before + inc - v;
}

// One workgroup per (frame, interval).  The interval's coefficients come back into LDS; a lane per block counts its bits; the
// blocks' bit offsets are a prefix over at most 96 counts; the lanes write their codes into the zeroed LDS bit buffer; the last
// byte is filled with 1-bits; 0xFF bytes are counted per thread over contiguous runs of the bytes and prefixed.
// out == NULL: only the stuffed length is stored (interval_len).  Otherwise the stuffed bytes go to
// out[frame_off[b] + interval_rel[b, it] ...], followed by RSTn (or EOI after the last interval); interval 0 also copies the header.
__global__ __launch_bounds__(JP_THREADS) void jpeg_pack_kernel(const short* __restrict__ coef, int H, int W,
                                                               int* __restrict__ interval_len, const long* __restrict__ interval_rel,
                                                               const long* __restrict__ frame_off, const unsigned char* __restrict__ header,
                                                               int header_len, unsigned char* __restrict__ out, long out_bytes) {
  __shared__ __attribute__((aligned(16))) short s_zz[JP_BLOCKS * 64];
  __shared__ unsigned s_bits[JP_WORDS + 1];
  __shared__ unsigned s_cnt[JP_BLOCKS];
  __shared__ long s_w[JP_THREADS / 64];
  const int tid = threadIdx.x;
  const Geo g = geo_of(H, W);
  const int b = blockIdx.x / g.n_int, it = blockIdx.x - b * g.n_int;
  const int n_blk = 3 * min(JP_RI, g.n_mcu - it * JP_RI);
  const u32x4* src = (const u32x4*)(coef + ((long)blockIdx.x * JP_BLOCKS) * 64);
  for (int p = tid; p < n_blk * 8; p += JP_THREADS) ((u32x4*)s_zz)[p] = src[p];
  __syncthreads();
  const bool mine = tid < n_blk;
  const int tab = (tid % 3) != 0;
  const int pred = (mine && tid >= 3) ? (int)s_zz[(tid - 3) * 64] : 0;       // the predictor restarts at 0 with the interval
  if (mine) s_cnt[tid] = walk_block<false>(s_zz + tid * 64, pred, tab, nullptr, 0u);
  __syncthreads();
  unsigned pos = 0, total_bits = 0;
  for (int k = 0; k < n_blk; ++k) {
    const unsigned c = s_cnt[k];
    if (k < tid) pos += c;
    total_bits += c;
  }
  const unsigned n_bytes = (total_bits + 7) >> 3;                            // <= 96 * 208 = 4 * JP_WORDS
  for (unsigned w = tid; w <= (n_bytes >> 2); w += JP_THREADS) s_bits[w] = 0u;
  __syncthreads();
  if (mine) walk_block<true>(s_zz + tid * 64, pred, tab, s_bits, pos);
  if (tid == 0 && (total_bits & 7)) put_bits(s_bits, total_bits, (1u << (8 - (total_bits & 7))) - 1u, 8 - (total_bits & 7));
  __syncthreads();
  const unsigned chunk = (n_bytes + JP_THREADS - 1) / JP_THREADS;
  const unsigned k0 = min(tid * chunk, n_bytes), k1 = min(k0 + chunk, n_bytes);
  int ff = 0;
  for (unsigned k = k0; k < k1; ++k) ff += ((s_bits[k >> 2] >> (24 - 8 * (k & 3))) & 255u) == 255u;
  long ff_total;
  const long ff_before = block_exclusive_scan((long)ff, s_w, &ff_total);
  const long stuffed = (long)n_bytes + ff_total;
  if (out == nullptr) {
    if (tid == 0) interval_len[blockIdx.x] = (int)stuffed;
    return;
  }
  const long frame0 = frame_off[b];
  const long base = frame0 + interval_rel[blockIdx.x];
  long o = base + k0 + ff_before;
  for (unsigned k = k0; k < k1; ++k) {
    const unsigned char v = (unsigned char)((s_bits[k >> 2] >> (24 - 8 * (k & 3))) & 255u);
    if (o >= 0 && o < out_bytes) out[o] = v;
    ++o;
    if (v == 255) {
      if (o >= 0 && o < out_bytes) out[o] = 0;
      ++o;
    }
  }
  if (tid < 2) {
    const long e = base + stuffed + tid;
    const unsigned char mk = tid == 0 ? 0xFF : (it == g.n_int - 1 ? 0xD9 : (unsigned char)(0xD0 + (it & 7)));
    if (e >= 0 && e < out_bytes) out[e] = mk;
  }
  if (it == 0)
    for (int k = tid; k < header_len; k += JP_THREADS)
      if (frame0 + k >= 0 && frame0 + k < out_bytes) out[frame0 + k] = header[k];
}

// ------------------------------------------------------------------------------------------------ (D) layout
// One workgroup per frame: interval_rel[b, i] = header_len + sum_{j < i} (len_j + 2) (the two bytes are the interval's RSTn,
// or EOI behind the last), frame_size[b] = the same sum over all intervals.
__global__ __launch_bounds__(JP_THREADS) void jpeg_frame_layout_kernel(const int* __restrict__ interval_len, int n_int, int header_len,
                                                                       long* __restrict__ interval_rel, long* __restrict__ frame_size) {
  __shared__ long s_w[JP_THREADS / 64];
  const int tid = threadIdx.x;
  const long row = (long)blockIdx.x * n_int;
  const int chunk = (n_int + JP_THREADS - 1) / JP_THREADS;
  const int i0 = min(tid * chunk, n_int), i1 = min(i0 + chunk, n_int);
  long sum = 0;
  for (int i = i0; i < i1; ++i) sum += (long)interval_len[row + i] + 2;
  long total;
  long at = header_len + block_exclusive_scan(sum, s_w, &total);
  for (int i = i0; i < i1; ++i) {
    interval_rel[row + i] = at;
    at += (long)interval_len[row + i] + 2;
  }
  if (tid == 0) frame_size[blockIdx.x] = header_len + total;
}

// One workgroup: offsets (B + 1) = exclusive prefix of frame_size, offsets[B] = the stream's length.
__global__ __launch_bounds__(JP_THREADS) void jpeg_offsets_kernel(const long* __restrict__ frame_size, int B, long* __restrict__ offsets) {
  __shared__ long s_w[JP_THREADS / 64];
  const int tid = threadIdx.x;
  const int chunk = (B + JP_THREADS - 1) / JP_THREADS;
  const int i0 = min(tid * chunk, B), i1 = min(i0 + chunk, B);
  long sum = 0;
  for (int i = i0; i < i1; ++i) sum += frame_size[i];
  long total;
  long at = block_exclusive_scan(sum, s_w, &total);
  for (int i = i0; i < i1; ++i) {
    offsets[i] = at;
    at += frame_size[i];
  }
  if (tid == 0) offsets[B] = total;
}

bool jpeg_sizes_ok(int B, int H, int W, long* grid) {
  if (B <= 0 || jpeg_sides_bad(H, W)) return false;
  *grid = (long)B * geo_of(H, W).n_int;
  return *grid <= 2147483647L;
}

}  // namespace

extern "C" int msmd_jpeg_intervals(int H, int W) {
  return jpeg_sides_bad(H, W) ? -1 : geo_of(H, W).n_int;
}

extern "C" int msmd_jpeg_coefficients(const void* frames, long frame_stride, long row_stride, int pixel_stride, int B, int H,
                                      int W, int quality, short* coef, msmd_stream_t stream) {
  long grid;
  if (!jpeg_sizes_ok(B, H, W, &grid) || quality < 1 || quality > 100 || (pixel_stride != 3 && pixel_stride != 4) ||
      row_stride < (long)W * pixel_stride - (pixel_stride - 3) || (B > 1 && frame_stride < (long)(H - 1) * row_stride) ||
      frames == nullptr || coef == nullptr)
    return 1;
  // one 4-byte load per pixel where every pixel's address is a multiple of 4 (the renderer's RGBA buffer), else three byte loads
  const int wide = pixel_stride == 4 && ((uintptr_t)frames & 3) == 0 && (row_stride & 3) == 0 && (frame_stride & 3) == 0;
  hipLaunchKernelGGL(jpeg_coef_kernel, dim3((unsigned)grid), dim3(JP_THREADS), 0, (hipStream_t)stream, (const unsigned char*)frames,
                     frame_stride, row_stride, pixel_stride, wide, H, W, quality, coef);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_jpeg_measure(const short* coef, int B, int H, int W, int header_len, int* interval_len, long* interval_rel,
                                 long* frame_size, long* offsets, msmd_stream_t stream) {
  long grid;
  if (!jpeg_sizes_ok(B, H, W, &grid) || header_len < 0 || coef == nullptr || interval_len == nullptr || interval_rel == nullptr ||
      frame_size == nullptr || offsets == nullptr)
    return 1;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)grid), dim3(JP_THREADS), 0, st, coef, H, W, interval_len, (const long*)nullptr,
                     (const long*)nullptr, (const unsigned char*)nullptr, 0, (unsigned char*)nullptr, 0L);
  hipLaunchKernelGGL(jpeg_frame_layout_kernel, dim3((unsigned)B), dim3(JP_THREADS), 0, st, (const int*)interval_len,
                     geo_of(H, W).n_int, header_len, interval_rel, frame_size);
  hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(JP_THREADS), 0, st, (const long*)frame_size, B, offsets);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_jpeg_write(const short* coef, int B, int H, int W, const void* header, int header_len, const long* interval_rel,
                               const long* offsets, void* out, long out_bytes, msmd_stream_t stream) {
  long grid;
  if (!jpeg_sizes_ok(B, H, W, &grid) || header_len < 0 || coef == nullptr || header == nullptr || interval_rel == nullptr ||
      offsets == nullptr || out == nullptr || out_bytes <= 0)
    return 1;
  hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)grid), dim3(JP_THREADS), 0, (hipStream_t)stream, coef, H, W, (int*)nullptr,
                     interval_rel, offsets, (const unsigned char*)header, header_len, (unsigned char*)out, out_bytes);
  MSMD_RETURN_LAST();
}
