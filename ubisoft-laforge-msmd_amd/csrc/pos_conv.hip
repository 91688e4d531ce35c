// Grouped positional convolution of the wav2vec2 / HuBERT encoders (k = 128, pad = 64, last frame dropped) for the 16-bit
// modes:  y = x + GELU(conv_g(x) + b)  on channels-last x (B, T, G * CG), read in place.
//
// As a GEMM, row t of group g's A operand is the window x[t - 64 .. t + 63][g * CG ..]: row t + 1 is the same memory shifted
// by CG elements.  The generic windowed GEMM (gemm.hip) stages every K tile of every M tile again, ~128 times the distinct
// input, and needs the zero-padded group-major copy msmd_group_pad writes.  Here ONE workgroup owns one (clip, group, block of
// <= 256 frames): it loads the block's rows and their 64 + 63 halo rows into LDS once (rows outside [0, T) as zeros, which is
// what the padded copy held) and every A fragment is read from that image at (row + tap) * PITCH + 2 * channel; only W streams,
// through a 3-deep LDS-DMA ring of CG rows x 128 K.
//
// Arithmetic is the generic kernel's, product for product: per output one v_mfma_f32_16x16x32 per 32 k, k ascending (k = tap *
// CG + channel), W fragment as the A operand and the window as B, fp32 accumulator from zero, then acc + bias -> gelu_poly16 ->
// + x -> one packed conversion.  Results are bit-identical to msmd_group_pad + msmd_gemm (tests/test_pos_conv_gpu.py).
//
// LDS image of the halo: PITCH = 96 B for CG = 48 (the flat view: A[r][k] = halo[r * 48 + k]) and 160 B for CG = 64; with either
// the 16 lanes of every ds_read_b128 lane group fall on 16 different 16-byte slots of the 256-byte bank row (128 B would be
// 4-way).  W tile: 256-byte rows, 16-byte chunk c of row n stored at slot c ^ (n & 15), conflict-free the same way; the
// permutation is applied to the per-lane SOURCE address because an LDS-DMA instruction writes its 1 KiB linearly.
#include "gemm_tiles.h"

#define PC_TAPS 128
#define PC_BM 256      // frames per workgroup at most (16 fragment rows over 4 waves)
#define PC_BK 128      // K elements per W tile (4 MFMA k-steps)
#define PC_NSTAGE 3

struct PosConvArgs {
  const void* x; const void* w; const float* bias; void* y;
  int B, T, G, nblk, rows_blk;   // nblk blocks of rows_blk frames per clip (rows_blk % 16 == 0)
  long ldx;                      // = G * CG
  int gpx;                       // groups per XCD label (blockIdx % 8): an XCD's L2 holds the W of gpx groups only
  int halo_rows;
};

template <int CG> struct PosConvGeom {
  static constexpr int PITCH = CG == 48 ? 96 : 160;
  static constexpr int FN = CG / 16;
  static constexpr int STAGE = CG * PC_BK * 2;         // bytes per W tile
  static constexpr int LPT = STAGE / (256 * 16);       // LDS-DMA instructions per thread per tile (4 waves)
  // byte offset inside a halo row pair (row + tap, channel) of K index k0 (k0 % 8 == 0)
  static __device__ __forceinline__ int koff(int k0) {
    if constexpr (CG == 48) return k0 * 2;
    else return (k0 >> 6) * PITCH + (k0 & 63) * 2;
  }
};

template <typename T, int CG>
__global__ __launch_bounds__(256) void pos_conv_kernel(const PosConvArgs p) {
  typedef PosConvGeom<CG> Gm;
  constexpr int PITCH = Gm::PITCH, FN = Gm::FN, FM = 4, STAGE = Gm::STAGE, LPT = Gm::LPT, CPR = CG / 8;
  constexpr int NK = PC_TAPS * CG / PC_BK;
  // ONE LDS object: [W ring: PC_NSTAGE x STAGE][halo: halo_rows x PITCH]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* halo = smem + PC_NSTAGE * STAGE;

  const int pid = blockIdx.x;
  const int xcd = pid & 7, slot = pid >> 3;
  const int grp = xcd * p.gpx + slot % p.gpx, blk = slot / p.gpx;
  if (grp >= p.G) return;
  const int b = blk / p.nblk, t0 = (blk % p.nblk) * p.rows_blk;
  const int rows = min(p.rows_blk, p.T - t0);
  if (rows <= 0) return;
  const int nf = (rows + 15) >> 4;                       // fragment rows of this block, 1 .. 16
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;

  // W tiles by LDS-DMA
  const T* __restrict__ W = (const T*)p.w + (long)grp * CG * (PC_TAPS * CG);
  const T* src[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int id = (i * 4 + wid) * 64 + lane;            // 16-B slot of the tile image
    const int n = id >> 4, phys = id & 15;
    src[i] = W + (long)n * (PC_TAPS * CG) + ((phys ^ (n & 15)) << 3);
  }
  auto issue = [&](int kt, int stage) {
#pragma unroll
    for (int i = 0; i < LPT; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(src[i] + kt * PC_BK),
                                       (lds_void_t*)(smem + stage * STAGE + (i * 4 + wid) * 1024), 16, 0, 0);
  };
#pragma unroll
  for (int s = 0; s < PC_NSTAGE - 1; ++s) issue(s, s);

  // the block's rows and their halo, once: halo row hr holds frame t0 - 64 + hr, zeros outside the clip
  {
    const T* __restrict__ xg = (const T*)p.x + (long)b * p.T * p.ldx + grp * CG;
    const int n_chunks = p.halo_rows * CPR;
    for (int idx = tid; idx < n_chunks; idx += 256) {
      const int hr = idx / CPR, c = idx - hr * CPR;
      const int t = t0 - PC_TAPS / 2 + hr;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (t >= 0 && t < p.T) v = *(const u32x4*)(xg + (long)t * p.ldx + c * 8);
      *(u32x4*)(halo + hr * PITCH + c * 16) = v;
    }
  }
  __syncthreads();

  // fragment rows of this wave: nf spread evenly over the 4 waves (13 -> 4, 3, 3, 3); a wave always reads FM fragments (rows
  // past its share repeat the block's last fragment row: valid LDS, never stored) and skips the 4th one's MFMAs when it has none
  const int base = nf >> 2, rem = nf & 3;
  const int f0 = wid * base + min(wid, rem);
  const int cnt = __builtin_amdgcn_readfirstlane(base + (wid < rem ? 1 : 0));
  const bool has4 = cnt == FM;
  const unsigned char* xrow[FM];
#pragma unroll
  for (int j = 0; j < FM; ++j) xrow[j] = halo + (min(f0 + j, nf - 1) * 16 + fr) * PITCH;
  int wrow[FN];
#pragma unroll
  for (int i = 0; i < FN; ++i) wrow[i] = (i * 16 + fr) * 256;

  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int stage = 0;
  for (int kt = 0; kt < NK; ++kt) {
    ring_step<PC_NSTAGE, LPT>(kt, NK, stage, issue);
    const unsigned char* sw = smem + stage * STAGE;
    u32x4 fx[2][FM], fw[2][FN];
    auto read = [&](int g, int s) {
      const int xo = Gm::koff(kt * PC_BK + g * 32 + fq * 8);
#pragma unroll
      for (int i = 0; i < FN; ++i) fw[s][i] = *(const u32x4*)(sw + wrow[i] + (((g * 4 + fq) ^ fr) << 4));
#pragma unroll
      for (int j = 0; j < FM; ++j) fx[s][j] = *(const u32x4*)(xrow[j] + xo);
    };
    read(0, 0);
#pragma unroll
    for (int g = 0; g < PC_BK / 32; ++g) {
      if (g + 1 < PC_BK / 32) read(g + 1, (g + 1) & 1);     // the next k-step's fragments land behind this one's MFMAs
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM - 1; ++j) acc[i][j] = mfma16<T>(fw[g & 1][i], fx[g & 1][j], acc[i][j]);
      if (has4) {
#pragma unroll
        for (int i = 0; i < FN; ++i) acc[i][FM - 1] = mfma16<T>(fw[g & 1][i], fx[g & 1][FM - 1], acc[i][FM - 1]);
      }
    }
    stage = ring_next<PC_NSTAGE>(stage);
  }

  // epilogue: lane holds row fr, columns 4 fq .. 4 fq + 3 of each 16 x 16 fragment
  typedef typename Vec4T<T>::type V4;
  const float* __restrict__ bias = p.bias + grp * CG + fq * 4;
  f32x4 bv[FN];
#pragma unroll
  for (int i = 0; i < FN; ++i) bv[i] = *(const f32x4*)(bias + i * 16);
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    const int t = t0 + (f0 + j) * 16 + fr;
    if (j >= cnt || t >= p.T) continue;
    const long off = ((long)b * p.T + t) * p.ldx + grp * CG + fq * 4;
    const T* __restrict__ R = (const T*)p.x + off;
    T* __restrict__ C = (T*)p.y + off;
    V4 rr[FN];
#pragma unroll
    for (int i = 0; i < FN; ++i) rr[i] = *(const V4*)(R + i * 16);
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + bv[i][e];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gelu_poly16(v[e]);
      // the GELU value is ROUNDED before the residual is added, as in the GEMM epilogue (there a branch on the residual
      // pointer separates the two): without the pin hipcc contracts GELU's last product and this add into one fma, and one
      // output in ~2^13 (fp16) lands on the other side of a rounding tie
#pragma unroll
      for (int e = 0; e < 4; ++e) asm("" : "+v"(v[e]));
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += (float)rr[i][e];
      *(V4*)(C + i * 16) = pack4<T>(v[0], v[1], v[2], v[3]);
    }
  }
}

template <typename T, int CG>
static int launch_pos_conv(PosConvArgs& p, hipStream_t st) {
  typedef PosConvGeom<CG> Gm;
  const size_t lds = (size_t)PC_NSTAGE * Gm::STAGE + (size_t)p.halo_rows * Gm::PITCH;
  static bool attr_set = false;      // idempotent: the same value every time
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)pos_conv_kernel<T, CG>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  const unsigned grid = 8u * p.gpx * p.B * p.nblk;
  hipLaunchKernelGGL((pos_conv_kernel<T, CG>), dim3(grid), dim3(256), lds, st, p);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_pos_conv(const void* x, const void* w, const float* bias, void* y, int B, int T, int G, int Cg, int kpos,
                             int dtype, msmd_stream_t stream) {
  if (B <= 0 || T <= 0 || G <= 0 || !x || !w || !bias || !y || x == y) return 1;
  if (kpos != PC_TAPS || (Cg != 48 && Cg != 64) || (dtype != MSMD_BF16 && dtype != MSMD_F16)) return 1;
  PosConvArgs p;
  p.x = x; p.w = w; p.bias = bias; p.y = y;
  p.B = B; p.T = T; p.G = G;
  p.nblk = (T + PC_BM - 1) / PC_BM;
  p.rows_blk = ((T + p.nblk - 1) / p.nblk + 15) / 16 * 16;      // even blocks (T = 499 -> 256 + 243), whole fragment rows
  p.ldx = (long)G * Cg;
  p.gpx = (G + 7) / 8;
  p.halo_rows = p.rows_blk + PC_TAPS - 1;
  if ((long)8 * p.gpx * B * p.nblk > 0x7fffffffL) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MSMD_BF16) return Cg == 48 ? launch_pos_conv<bf16_t, 48>(p, st) : launch_pos_conv<bf16_t, 64>(p, st);
  return Cg == 48 ? launch_pos_conv<f16_t, 48>(p, st) : launch_pos_conv<f16_t, 64>(p, st);
}
