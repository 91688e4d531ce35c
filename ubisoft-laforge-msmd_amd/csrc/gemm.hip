// MFMA GEMM for gfx950:  C = act(A . W^T + bias) + residual
//
// One kernel template serves every dense contraction on the audio->motion path: HF conv stack as a
// windowed GEMM over the channels-last signal (no im2col), Linear layers, attention projections,
// grouped positional conv (batched), style-encoder convs.  Both operands are K-contiguous
// ((M,K) activations, (N,K) torch-layout weights), so A and W tiles are staged identically.
//
// Tile: BM x BN outputs per 256-thread workgroup (4 waves as 2x2), K step = 128 BYTES per row
// (64 bf16 / 32 fp32) so the LDS image and the staging code are byte-identical for both dtypes.
// LDS rows are 128 B with the 16-B chunk index XOR-swizzled by ((row>>1)&7): conflict-free for the
// real ds_read_b128 lane groups of gfx950 (MI355X_MICROARCH.md, LDS table).  Global->register
// prefetch of tile k+1 is issued before the MFMAs of tile k; two LDS buffers, one barrier per K step.
// Operands are swapped (D = W_tile . X_tile^T) so each lane ends up with 4 CONSECUTIVE output
// columns of one row: 16-B (fp32) / 8-B (bf16) epilogue stores and a float4 bias load.
// bf16: v_mfma_f32_16x16x32_bf16; fp32 parity mode: v_mfma_f32_16x16x4_f32 (exact fp32 FMA chain).
#include "gemm_tiles.h"
#include <atomic>
#include <utility>

struct GemmArgs {
  const void* A; const void* W; const float* bias; const void* R; void* C;
  int M, N, K;
  long lda; int rows_per_batch; long a_batch_stride; long ldw, ldc, ldr;
  int act; int vec_ok; float inv_rpb;
  long strideA, strideW, strideC, strideBias, strideR;
  int mt, nt;
  int batch_inner; long strideA2, strideW2, strideC2;  // z = outer * batch_inner + inner (attention: batch x heads)
  // training epilogue (msmd_gemm_ex): optional pre-activation copy Z (layout of C) and dropout on act(.) before the
  // residual add; the keep mask is Philox(rng, site, (m * N + n) / 4), i.e. msmd_dropout's on a contiguous (M, N) C
  void* Z; float p_drop; const unsigned long* rng; unsigned site;
  int xn;  // XCDs along N (1, 2 or 4): the 8 XCDs form an (8 / xn) x xn grid over (M tiles, N tiles)
  int flags;  // GF_* below
  // LayerNorm folded into the GEMMs around it (msmd_gemm_ln; all NULL for plain calls):
  //   a_stats (a_nt, M, 2): A holds UN-normalised rows u, the partial (sum, sum of squares) of each row over 64-column
  //     slabs; W carries gamma folded in, w_colsum[n] = sum_k W'[n][k], bias carries beta . W:  y = rstd (acc - mu s[n]) + c[n]
  //   r_stats (r_nt, M, 2) + r_gamma / r_beta (N): the residual operand holds un-normalised rows: R <- LN(R) on the fly
  //   stats_out (N / slab, M, 2): partial (sum, sum of squares) of the STORED (rounded) output rows, per 64-column slab
  const float* a_stats = nullptr; int a_nt = 0; const float* w_colsum = nullptr;
  const float* r_stats = nullptr; int r_nt = 0; const float* r_gamma = nullptr; const float* r_beta = nullptr;
  float* stats_out = nullptr; float ln_eps = 1e-5f;
  // GF_STAGGER (MSMD_GEMM_STAGGER): the workgroups dispatched second onto their CU start `stagger_ticks` (100 MHz) late
  int stagger_ticks = 0;
};

// GemmArgs::flags: the MSMD_GEMM_* bits 16-18 of `act` shifted down to bits 0-2, bits 19-23 to bits 4-8 (gemm_unpack_act).
enum : int {
  GF_WRITE_THROUGH = 1, GF_PAIRED_STORES = 2, GF_STAGGER = 4,      // how the output is stored; when a CU's second workgroup starts
  GF_ACT_BWD = 8,      // internal (msmd_gemm_actbwd): Z is an INPUT: C = keep_mask / (1 - p) * act'(Z) * (A W^T), no bias / residual
  GF_ONE_TILE = 16, GF_NO_256 = 32,      // opt out of the persistent form / of the 256 x 256 kernel as the library's own choice (A/B)
  GF_W_BELOW_32 = 64,      // split operands: |W| < 32 everywhere
  GF_NO_160 = 128, GF_FORCE_160 = 256,      // msmd_gemm_ln: opt out of / force the 160-row member of variant 17 (A/B; tests and scans)
  GF_ROWS_160 = 512,   // internal (gemm_ln_plan): variant 17 launches its 160 x 128 member; no bit of `act` sets it
};
struct GemmActWord { int act, hint, flags; };   // MSMD_ACT_*, the caller's variant (0 = the library's own choice), GF_*
static constexpr GemmActWord gemm_unpack_act(int act) {
  return {act & 0xff, (act >> 8) & 0xff, ((act >> 16) & 7) | (((act >> 19) & 31) << 4)};
}
static_assert(gemm_unpack_act(MSMD_GEMM_WRITE_THROUGH).flags == GF_WRITE_THROUGH && gemm_unpack_act(MSMD_GEMM_PAIRED_STORES).flags == GF_PAIRED_STORES &&
              gemm_unpack_act(MSMD_GEMM_STAGGER).flags == GF_STAGGER && gemm_unpack_act(MSMD_GEMM_ONE_TILE_PER_WORKGROUP).flags == GF_ONE_TILE &&
              gemm_unpack_act(MSMD_GEMM_NO_256_TILE).flags == GF_NO_256 && gemm_unpack_act(MSMD_GEMM_W_BELOW_32).flags == GF_W_BELOW_32 &&
              gemm_unpack_act(MSMD_GEMM_NO_160_ROW_TILE).flags == GF_NO_160 && gemm_unpack_act(MSMD_GEMM_FORCE_160_ROW_TILE).flags == GF_FORCE_160 &&
              gemm_unpack_act(~0).flags == (0x1ff & ~GF_ACT_BWD),
              "internal flag bits follow include/msmd_hip.h; no bit of `act` sets the internal ones");
// Kernel variants: what the plans return, msmd_gemm_route reports and MSMD_GEMM_VARIANT names.
enum : int {
  GV_GENERIC = 0,       // gemm_kernel: fp32 operands, K % 64 != 0
  GV_SPLIT_128 = 1, GV_SPLIT_64 = 5,      // split pairs: 128 x 128 (64 KB, 2 workgroups / CU: default), 64 x 64 (small grids)
  GV_64_DEEP = 9, GV_64 = 12,      // 64 x 64 with a 4- / 2-stage ring: grids that would not fill the chip
  GV_256x64 = 14,       // narrow outputs (N <= 64): the positional conv; 16-bit and split pairs
  GV_192 = 15,          // 192 x 128, tall grids (M >= 16 k): 80 KB, still 2 workgroups / CU
  GV_128 = 17,          // 128 x 128, 8 waves (4 x 2), 2-stage ring, fragment reads of both k-steps issued first; msmd_gemm_ln's residual form also
                        // as 160 x 128, 10 waves (5 x 2), 4-stage ring (144 KB), where that fits the grid into ONE round of one workgroup per CU
  GV_64x128 = 18,       // 64 x 128, 4 waves (2 x 2) of 17's 32 x 64 wave tile, 4-stage ring (96 KB): one workgroup per CU, twice 17's grid
  GV_128_AB = 13, GV_128_ONE_AB = 66,     // A/B forms of 17, bf16 only: the compiler's own read / multiply interleave; ONE kernel with every epilogue
  GV_256 = 80,          // 256 x 256, 8-phase schedule, one workgroup per CU (gemm8_kernel); 16-bit and split pairs
};

// The epilogues an instantiation carries, and the EPIA code of the kernels' integer template parameter: the family + 10 * (1 +
// activation) when the activation is a constant of the kernel too, the family alone (ACT_RUNTIME) when it is read from p.act.
enum GemmEpi : int { EPI_ALL = 0, EPI_PLAIN = 1, EPI_LN_OPERAND = 2, EPI_LN_RESIDUAL = 3 };
constexpr int ACT_RUNTIME = -1;
constexpr int epia(GemmEpi e, int act) { return e + 10 * (1 + act); }
constexpr GemmEpi epia_family(int code) { return (GemmEpi)(code % 10); }
constexpr int epia_act(int code) { return code / 10 - 1; }

template <typename T> struct Mfma;
template <> struct Mfma<bf16_t> {
  // one 16-B chunk = 8 bf16 = the lane's K-slice of one 16x16x32 MFMA
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                  acc, 0, 0, 0);
  }
};
template <> struct Mfma<f16_t> {
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
  }
};
template <> struct Mfma<float> {
  // one 16-B chunk = 4 fp32; lane (l>>4) owns k = 4*(l>>4)+e in MFMA step e (K is permuted
  // identically for both operands, which leaves the contraction unchanged).
  // NB: __builtin_bit_cast on a vector ELEMENT reads element 0 (hipcc 7.2); convert by value instead.
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& acc) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[e]), __uint_as_float(b[e]), acc, 0, 0, 0);
  }
};

// Row m of the (possibly windowed) A operand -> element offset.  Plain GEMMs skip the division; windowed
// (conv) rows use an fp32 reciprocal with an exact fix-up (m < 2^24), not a 40-instruction integer divide.
__device__ __forceinline__ long a_row_offset(const GemmArgs& p, int m) {
  if (p.rows_per_batch >= p.M) return (long)m * p.lda;
  int q = (int)((float)m * p.inv_rpb);
  int r = m - q * p.rows_per_batch;
  if (r < 0) { q -= 1; r += p.rows_per_batch; }
  if (r >= p.rows_per_batch) { q += 1; r -= p.rows_per_batch; }
  return (long)q * p.a_batch_stride + (long)r * p.lda;
}

// ---------------------------------------------------------------------------------------------------
// Shared pieces of the fragment kernels (gemm_kernel, gemm2_kernel, gemm2p_kernel, gemm2s_kernel); layout in gemm_tiles.h.

// Block id -> tile of the XCD grid (8 / xn) x xn over (M, N) tiles (block ids congruent mod 8 share an XCD's L2): an XCD's L2
// then holds 1 / xn of the weight matrix instead of all of it.  False for the block ids the grid pads with.
__device__ __forceinline__ bool xcd_tile(const GemmArgs& p, int pid, int& m_tile, int& n_tile) {
  const int xcd = pid & 7, slot = pid >> 3;
  const int xm_n = 8 / p.xn, ntx = (p.nt + p.xn - 1) / p.xn;
  m_tile = (slot / ntx) * xm_n + (xcd % xm_n);
  n_tile = (slot % ntx) * p.xn + xcd / xm_n;
  return m_tile < p.mt && n_tile < p.nt;
}
// the operands of problem z = outer * batch_inner + inner of a batched launch
template <typename T> __device__ __forceinline__ const T* batch_a(const GemmArgs& p, int z) {
  return (const T*)p.A + (z / p.batch_inner) * p.strideA + (z % p.batch_inner) * p.strideA2;
}
template <typename T> __device__ __forceinline__ const T* batch_w(const GemmArgs& p, int z) {
  return (const T*)p.W + (z / p.batch_inner) * p.strideW + (z % p.batch_inner) * p.strideW2;
}

// Per-lane LDS-DMA sources of one K-contiguous (BM + BN)-row tile image (A rows, then W rows; 16-bit elements) staged by NLW
// loader waves with LPT wave-instructions (1 KB of the image) each.  The swizzle is applied HERE, to the source address, because
// an LDS-DMA wave-instruction writes its 1 KB linearly; out-of-range rows are clamped to a valid row (never stored).
template <typename T, int BM, int BN, int NLW> struct TileSrc {
  static constexpr int LPT = (BM + BN) / 8 / NLW;
  static_assert(NLW * LPT * 8 == BM + BN, "tile chunks must divide over the loader waves");
  const T* src[LPT];
  __device__ __forceinline__ void set(const GemmArgs& p, const T* A, const T* W, int m0, int n0, int tid) {
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int id = (i * NLW + wid) * 64 + lane;  // 16-B slot of the tile image (past its end in a wave that loads nothing: clamped, never read)
      const int row = id >> 3, phys = id & 7;
      const int c = phys ^ ((row >> 1) & 7);      // logical chunk stored at this physical slot
      if (row < BM) src[i] = A + a_row_offset(p, min(m0 + row, p.M - 1)) + c * 8;
      else src[i] = W + (long)min(n0 + row - BM, p.N - 1) * p.ldw + c * 8;
    }
  }
  // K tile kt (64 elements per row) into the stage at `stage_base`
  __device__ __forceinline__ void issue(unsigned char* stage_base, int kt, int tid) const {
    const int wid = tid >> 6;
#pragma unroll
    for (int i = 0; i < LPT; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(src[i] + kt * 64), (lds_void_t*)(stage_base + (i * NLW + wid) * 1024), 16, 0, 0);
  }
};

// The K tile of a staged image (A rows at sa, W rows at sw): two 32-deep k-steps of FM + FN fragment reads and FN x FM multiplies.
template <typename TI, int FM, int FN>
__device__ __forceinline__ void k_tile_mma(const unsigned char* sa, const unsigned char* sw, const FragLane& l, f32x4 (&acc)[FN][FM]) {
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    u32x4 fx[FM], fw[FN];
#pragma unroll
    for (int j = 0; j < FM; ++j) fx[j] = *(const u32x4*)(sa + lds_off(l.wm + j * 16 + l.fr, g * 4 + l.fq));
#pragma unroll
    for (int i = 0; i < FN; ++i) fw[i] = *(const u32x4*)(sw + lds_off(l.wn + i * 16 + l.fr, g * 4 + l.fq));
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j) Mfma<TI>::run(fw[i], fx[j], acc[i][j]);
  }
}
// Explicit software pipeline: issue the fragment reads of BOTH 32-deep k-steps, then the MFMAs.  Left to
// itself hipcc re-uses 16 fragment registers and emits read / lgkmcnt(0) / 4 MFMA groups, exposing the LDS
// latency four times per K tile; pinned like this the second k-step's reads land behind the first's MFMAs.
template <typename TI, int FM, int FN>
__device__ __forceinline__ void k_tile_mma_pipelined(const unsigned char* sa, const unsigned char* sw, const FragLane& l, f32x4 (&acc)[FN][FM]) {
  u32x4 fx[2][FM], fw[2][FN];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
#pragma unroll
    for (int j = 0; j < FM; ++j) fx[g][j] = *(const u32x4*)(sa + lds_off(l.wm + j * 16 + l.fr, g * 4 + l.fq));
#pragma unroll
    for (int i = 0; i < FN; ++i) fw[g][i] = *(const u32x4*)(sw + lds_off(l.wn + i * 16 + l.fr, g * 4 + l.fq));
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < 2; ++g) {
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j) Mfma<TI>::run(fw[g][i], fx[g][j], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Epilogue of the fragment kernels (gemm_kernel, gemm2_kernel, gemm2p_kernel, gemm2s_kernel; gemm8_kernel stores through LDS and
// shares only act_out_c): lane holds row m = ..+fr, columns n = ..+fq*4 + {0..3} of each 16x16 fragment.
template <typename TO> __device__ __forceinline__ float act_out(float x, int act) {
  // 16-bit outputs: the transcendental-free GELU (|err| <= 5.5e-5, common.h) is below their own rounding;
  // fp32 outputs (parity mode) use the exact erff.
  if (act == MSMD_ACT_GELU) return sizeof(TO) == 2 ? gelu_poly16(x) : gelu_erf(x);
  if (act == MSMD_ACT_ELU) return elu1(x);
  return x;
}
// ACT >= 0: the activation is a compile-time constant of the KERNEL (the launcher picks the instantiation from p.act).  With
// the run-time code tested per ELEMENT the compiler keeps a scalar compare-and-branch around each of a lane's 32 outputs
// (737 branches in the 128 x 128 kernel; per-workgroup stamps put its bias-only epilogue at 2.7-3.0 us of a 15 us tile, almost
// all of it taken branches and instruction fetch); three copies behind ONE test inside the kernel spill.  ACT < 0: run-time.
template <typename TO, int ACT> __device__ __forceinline__ float act_out_c(float x, int act) {
  if constexpr (ACT == MSMD_ACT_GELU) return sizeof(TO) == 2 ? gelu_poly16(x) : gelu_erf(x);
  else if constexpr (ACT == MSMD_ACT_ELU) return elu1(x);
  else if constexpr (ACT == MSMD_ACT_NONE) return x;
  else return act_out<TO>(x, act);
}

// Output stores.  wt = write-through (`sc1`): the bytes leave the XCD's L2 for memory as they are stored instead of
// waiting dirty for the end-of-kernel write-back (MI355X_MICROARCH.md, "stores of each flavour"), so a consumer kernel
// on another XCD never depends on that write-back having completed.
__device__ __forceinline__ void store16_wt(void* p, const u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store8_wt(void* p, const u32x2 v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
template <typename TO> __device__ __forceinline__ void store4_out(TO* p, const float* v, bool wt) {
  if constexpr (sizeof(TO) == 4) {
    const f32x4 o = f32x4{v[0], v[1], v[2], v[3]};
    if (wt) store16_wt(p, __builtin_bit_cast(u32x4, o));
    else *(f32x4*)p = o;
  } else {
    const typename Vec4T<TO>::type o = pack4<TO>(v[0], v[1], v[2], v[3]);
    if (wt) store8_wt(p, __builtin_bit_cast(u32x2, o));
    else *(typename Vec4T<TO>::type*)p = o;
  }
}

// Dropout of the four values at flat index idx .. idx + 3 of a contiguous (M, N) C: the keep mask is msmd_dropout's.
__device__ __forceinline__ void dropout4(const GemmArgs& p, long idx, float (&v)[4]) {
  const Philox4 rb = dropout_bits(p.rng, p.site, (unsigned long)(idx >> 2));
  const unsigned thr = dropout_threshold(p.p_drop);
  const float c = 1.0f / (1.0f - p.p_drop);
  v[0] = rb.x >= thr ? v[0] * c : 0.f;
  v[1] = rb.y >= thr ? v[1] * c : 0.f;
  v[2] = rb.z >= thr ? v[2] * c : 0.f;
  v[3] = rb.w >= thr ? v[3] * c : 0.f;
}
// Paired 16-byte stores: lanes l and l ^ 16 hold columns 4 fq .. 4 fq + 3 and the next four of the same rows.
// They swap one fragment row each (even fq keeps row j0 and takes the partner's half of it, odd fq keeps row
// j0 + 1), so every lane issues ONE 16-byte store per fragment-row pair instead of two 8-byte ones.
// a / b: the lane's packed values of rows j0 / j0 + 1.  The result goes to row j0 + odd, 4 columns to the left when odd.
__device__ __forceinline__ u32x4 pair_swap(const u32x2 a, const u32x2 b, bool odd) {
  const u32x2 send = odd ? a : b;
  u32x2 recv;
  recv[0] = __shfl_xor(send[0], 16, 64);
  recv[1] = __shfl_xor(send[1], 16, 64);
  return odd ? u32x4{recv[0], recv[1], b[0], b[1]} : u32x4{a[0], a[1], recv[0], recv[1]};
}

// Interior tiles (fully inside M x N, vector-aligned): straight-line code, no per-element bounds checks.
// AB: the kernel also serves msmd_gemm_actbwd (GF_ACT_BWD).  Only the LDS-DMA 16-bit kernels carry that code: in the v1 /
// fp32 kernels it cost 272 bytes of scratch (fp32 mode 23.8 -> 34 ms).
// LEAN: the inference epilogue only (no pre-activation copy, no dropout, no activation backward): the launcher sends calls that
// carry those to the kernels that compile them in.
template <typename TO, int FM, int FN, bool AB, bool LEAN, int ACT>
__device__ __forceinline__ void gemm_epilogue_interior(const GemmArgs& p, const f32x4 (&acc)[FN][FM], int z, int m_base,
                                                         int n_base, int fr, int fq) {
  TO* __restrict__ C = (TO*)p.C + (z / p.batch_inner) * p.strideC + (z % p.batch_inner) * p.strideC2 +
                       (long)(m_base + fr) * p.ldc + n_base + fq * 4;
  const TO* __restrict__ R = p.R ? (const TO*)p.R + z * p.strideR + (long)(m_base + fr) * p.ldr + n_base + fq * 4 : nullptr;
  const float* __restrict__ bias = p.bias ? p.bias + z * p.strideBias + n_base + fq * 4 : nullptr;
  const bool wt = p.flags & GF_WRITE_THROUGH;
  f32x4 bv[FN];
#pragma unroll
  for (int i = 0; i < FN; ++i) bv[i] = bias ? *(const f32x4*)(bias + i * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
  // every residual fragment is requested BEFORE the first output store: loads issued between the stores are serialised
  // into one L2 round trip per fragment (load, wait, store, load, ...), 8 of them on a 128 x 128 tile
  // (fp32 outputs: one fragment row at a time -- all of them would take the 128 x 128 kernel past 128 registers)
  typedef typename Vec4T<TO>::type V4;
  constexpr int RJ = sizeof(TO) == 2 ? FM : 1;
  V4 rr[RJ][FN];
  auto load_residual = [&](int j0) {
    if (R) {
#pragma unroll
      for (int j = 0; j < RJ; ++j)
#pragma unroll
        for (int i = 0; i < FN; ++i) rr[j][i] = *(const V4*)(R + (long)(j0 + j) * 16 * p.ldr + i * 16);
    }
  };
  if constexpr (RJ == FM) load_residual(0);
  // the finished 4 values of fragment (i, j): bias, optional pre-activation copy, activation, dropout, residual
  auto finish = [&](int i, int j, float (&v)[4]) {
    TO* crow = C + (long)j * 16 * p.ldc;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + bv[i][e];
    if (AB && (p.flags & GF_ACT_BWD)) {    // the backward of y = dropout(act(z)) applied to this data gradient: z read where C goes
      const V4 z4 = *(const V4*)((const TO*)p.Z + (crow + i * 16 - (TO*)p.C));
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= act_grad_fast((float)z4[e], ACT >= 0 ? ACT : p.act);
    } else {
      if (!LEAN && p.Z) store4_out<TO>((TO*)p.Z + (crow + i * 16 - (TO*)p.C), v, wt);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_out_c<TO, ACT>(v[e], p.act);
    }
    if (!LEAN && p.p_drop > 0.f) {
      dropout4(p, (long)(m_base + j * 16 + fr) * p.N + (n_base + i * 16 + fq * 4), v);
    }
    if (R) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += (float)rr[j % RJ][i][e];
    }
  };
  if constexpr (sizeof(TO) == 2 && FM % 2 == 0) {
    if (p.flags & GF_PAIRED_STORES) {
      const bool odd = fq & 1;     // see pair_swap
#pragma unroll
      for (int jp = 0; jp < FM / 2; ++jp) {
#pragma unroll
        for (int i = 0; i < FN; ++i) {
          float v0[4], v1[4];
          finish(i, 2 * jp, v0);
          finish(i, 2 * jp + 1, v1);
          const u32x2 a = __builtin_bit_cast(u32x2, pack4<TO>(v0[0], v0[1], v0[2], v0[3]));
          const u32x2 b = __builtin_bit_cast(u32x2, pack4<TO>(v1[0], v1[1], v1[2], v1[3]));
          const u32x4 o = pair_swap(a, b, odd);
          TO* dst = C + (long)(2 * jp + (odd ? 1 : 0)) * 16 * p.ldc + i * 16 - (odd ? 4 : 0);
          if (wt) store16_wt(dst, o);
          else *(u32x4*)dst = o;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    if constexpr (RJ != FM) load_residual(j);
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      float v[4];
      finish(i, j, v);
      store4_out<TO>(C + (long)j * 16 * p.ldc + i * 16, v, wt);
    }
  }
}

template <typename TO, int FM, int FN, bool AB = false, bool LEAN = false, int ACT = -1>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& p, const f32x4 (&acc)[FN][FM], int z, int m_base,
                                              int n_base, int fr, int fq) {
  if (p.vec_ok && m_base + FM * 16 <= p.M && n_base + FN * 16 <= p.N) {
    gemm_epilogue_interior<TO, FM, FN, AB, LEAN, ACT>(p, acc, z, m_base, n_base, fr, fq);
    return;
  }
  TO* __restrict__ C = (TO*)p.C + (z / p.batch_inner) * p.strideC + (z % p.batch_inner) * p.strideC2;
  const TO* __restrict__ R = p.R ? (const TO*)p.R + z * p.strideR : nullptr;
  const float* __restrict__ bias = p.bias ? p.bias + z * p.strideBias : nullptr;
#pragma unroll
  for (int i = 0; i < FN; ++i) {
    const int n = n_base + i * 16 + fq * 4;
    if (n >= p.N) continue;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = (n + e < p.N) ? bias[n + e] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int m = m_base + j * 16 + fr;
      if (m >= p.M) continue;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + bv[e];
      TO* cp = C + (long)m * p.ldc + n;
      if (AB && (p.flags & GF_ACT_BWD)) {
        const TO* zp = (const TO*)p.Z + (cp - (TO*)p.C);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < p.N) v[e] *= act_grad_fast((float)zp[e], ACT >= 0 ? ACT : p.act);
      } else {
        if (!LEAN && p.Z) {
          TO* zp = (TO*)p.Z + (cp - (TO*)p.C);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n + e < p.N) zp[e] = (TO)v[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_out_c<TO, ACT>(v[e], p.act);
      }
      if (!LEAN && p.p_drop > 0.f) dropout4(p, (long)m * p.N + n, v);   // launcher guarantees N % 4 == 0 and ldc == N here
      if (p.vec_ok && n + 3 < p.N) {
        if (R) {
          const TO* rp = R + (long)m * p.ldr + n;
          if constexpr (sizeof(TO) == 4) {
            const f32x4 r = *(const f32x4*)rp;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += r[e];
          } else {
            const typename Vec4T<TO>::type r = *(const typename Vec4T<TO>::type*)rp;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += (float)r[e];
          }
        }
        store4_out<TO>(cp, v, p.flags & GF_WRITE_THROUGH);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (n + e < p.N) {
            float o = v[e];
            if (R) o += to_f32(R[(long)m * p.ldr + n + e]);
            cp[e] = from_f32<TO>(o);
          }
        }
      }
    }
  }
}

// LayerNorm folded into the GEMM (see GemmArgs).  Statistics travel as per-row partial (sum, sum of squares) over
// column slabs = what ONE wave of a tile holds of a row (64 columns in the 128 x 128 kernel), so writing them needs no LDS
// and no barrier; the layout is slab-major, (slabs, rows, 2): the 16 rows of a fragment are one 128-byte line of a slab
// (row-major partials cost 16 lines per load instruction -- +13 % on HuBERT-large's FFN1, measured).  Reading them is latency, not bandwidth: the producer ran on other XCDs, so the first touch of a row's partials
// misses this XCD's L2.  Measured on the encoder's FFN1 (49 us): a loop over the slabs in the epilogue +5.5 us (serialised
// round trips), all slabs loaded and reduced before the K loop +8.5 us (every workgroup stalls on the miss before its first
// tile).  So: ln_issue only ISSUES the loads before the K loop -- lane (fr, fq) takes slabs fq, fq + 4, ... of the FM rows
// it owns, 16 registers -- and ln_finish reduces them (two cross-lane adds) in the epilogue, a whole K loop later.
template <int FM>
__device__ __forceinline__ void ln_issue(const float* stats, int nt, int M, int m_base, int fr, int fq, f32x2 (&raw)[FM][4]) {
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    const f32x2* sp = (const f32x2*)stats + min(m_base + j * 16 + fr, M - 1);     // slab-major: 16 rows = one 128-byte line
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[j][q] = fq + 4 * q < nt ? sp[(long)(fq + 4 * q) * M] : f32x2{0.f, 0.f};
  }
}

template <int FM>
__device__ __forceinline__ void ln_finish(const float* stats, int nt, int M, int m_base, int fr, int fq, const f32x2 (&raw)[FM][4],
                                          float inv_cols, float eps, float (&mu)[FM], float (&rs)[FM]) {
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    float S = (raw[j][0][0] + raw[j][1][0]) + (raw[j][2][0] + raw[j][3][0]);
    float Q = (raw[j][0][1] + raw[j][1][1]) + (raw[j][2][1] + raw[j][3][1]);
    if (nt > 16) {     // more than 16 slabs per row: the rest, serially
      const f32x2* sp = (const f32x2*)stats + min(m_base + j * 16 + fr, M - 1);
      for (int t = 16 + fq; t < nt; t += 4) { const f32x2 w = sp[(long)t * M]; S += w[0]; Q += w[1]; }
    }
    S += __shfl_xor(S, 16, 64); S += __shfl_xor(S, 32, 64);
    Q += __shfl_xor(Q, 16, 64); Q += __shfl_xor(Q, 32, 64);
    mu[j] = S * inv_cols;
    rs[j] = rsqrtf(fmaxf(Q * inv_cols - mu[j] * mu[j], 0.f) + eps);
  }
}

// Epilogue of a wave whose FN fragments span exactly one statistics slab (64 columns in the 128 x 128 kernel, 32 in the
// 64 x 64 one).  MODE 1: the operand was LayerNorm'ed
// (folded weights; no residual).  MODE 2: residual add, the residual LayerNorm'ed on the fly when r_stats is given, and
// the statistics of the stored rows written when stats_out is given.  Every load of the epilogue (bias, column sums or
// gamma / beta, the residual fragments) is issued up front, unconditionally: with run-time "is this pointer set" tests
// inside the fragment loops the compiler serialises them into one L2 round trip per fragment column (+4 us per launch).
// EARLY: the MODE 2 operands were requested before the K loop (ln_res_issue, the 4-wave 64 x 128 kernel: 256 registers) and are
// consumed here from `early` with the same arithmetic; the HBM round trip that otherwise stands between the last MFMA and the
// first store, for every workgroup of a one-round launch at the same moment, is then behind the K loop.
// GB = false (the 10-wave 160 x 128 kernel: 168 registers): bias and residual fragments only; gamma / beta, which every workgroup reads and
// the L2 holds, are loaded in the epilogue as without EARLY (all four were 68 bytes of scratch there).
template <typename TO, int FM, int FN, bool GB = true> struct LnResOps { static constexpr bool gb = GB; f32x4 bv[FN], xv[GB ? FN : 1], yv[GB ? FN : 1]; typename Vec4T<TO>::type rr[FM][FN]; };
struct NoEarlyOps {};     // what a kernel without early operands hands to gemm_run_epilogue
template <typename TO, int FM, int FN, bool GB>
__device__ __forceinline__ void ln_res_issue(const GemmArgs& p, int m_base, int n_base, int fr, int fq, LnResOps<TO, FM, FN, GB>& o) {
  typedef typename Vec4T<TO>::type V4;
  const int n = n_base + fq * 4;
#pragma unroll
  for (int i = 0; i < FN; ++i) o.bv[i] = *(const f32x4*)(p.bias + n + i * 16);
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    const TO* rp = (const TO*)p.R + (long)min(m_base + j * 16 + fr, p.M - 1) * p.ldr + n;
#pragma unroll
    for (int i = 0; i < FN; ++i) o.rr[j][i] = *(const V4*)(rp + i * 16);
  }
  if constexpr (GB) {
    if (p.r_stats) {
#pragma unroll
      for (int i = 0; i < FN; ++i) { o.xv[i] = *(const f32x4*)(p.r_gamma + n + i * 16); o.yv[i] = *(const f32x4*)(p.r_beta + n + i * 16); }
    } else {
#pragma unroll
      for (int i = 0; i < FN; ++i) { o.xv[i] = f32x4{1.f, 1.f, 1.f, 1.f}; o.yv[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    }
  }
}

template <typename TO, int FM, int FN, int MODE, int ACT = -1, bool EARLY = false, bool EARLY_GB = true>
__device__ __forceinline__ void gemm_epilogue_ln(const GemmArgs& p, const f32x4 (&acc)[FN][FM], int m_base, int n_base,
                                                 int fr, int fq, const f32x2 (&raw)[FM][4], const LnResOps<TO, FM, FN, EARLY_GB>* early = nullptr) {
  static_assert((FN == 4 || FN == 2) && (FM >= 2 && FM <= 4), "one wave = one statistics slab of 16 FN columns, 2 to 4 fragment rows");
  constexpr int SLAB = FN * 16;
  // fragment columns whose operands are requested together: all of them for the two-row tiles; two at a time for the
  // 192-row tile, whose kernel has 128 registers for everything (all four would need 166: one workgroup per CU)
  constexpr int IB = FM == 3 ? 2 : FN;
  typedef typename Vec4T<TO>::type V4;
  const int n = n_base + fq * 4;
  float mu[FM], rs[FM];
#pragma unroll
  for (int j = 0; j < FM; ++j) { mu[j] = 0.f; rs[j] = 1.f; }      // (r - 0) * 1 * 1 + 0 == r exactly: the plain residual
  if constexpr (MODE == 1) ln_finish<FM>(p.a_stats, p.a_nt, p.M, m_base, fr, fq, raw, 1.0f / (float)p.K, p.ln_eps, mu, rs);
  else if (p.r_stats) ln_finish<FM>(p.r_stats, p.r_nt, p.M, m_base, fr, fq, raw, 1.0f / (float)p.N, p.ln_eps, mu, rs);
  // Statistics of the stored rows, in ONE association for every kernel that writes them (this epilogue on its 128 x 128 /
  // 192 x 128 / 64 x 64 tiles, gemm8_kernel on 256 x 256): a row's result must not depend on the tile the launch's row count
  // routed it to (a clip alone and the same clip in a batch of 32).  Per 16-column fragment i and lane group fq:
  // p_i = the serial sum of its four stored values; (p_0 + p_1) + (p_2 + p_3) over the slab's fragments; then the lane
  // groups fq ^ 1 and fq ^ 2.  (tS / prS: the odd-man-out and the first pair while the fragments go by.)
  float rowS[FM], rowQ[FM], tS[FM], tQ[FM], prS[FM], prQ[FM];
#pragma unroll
  for (int j = 0; j < FM; ++j) rowS[j] = rowQ[j] = tS[j] = tQ[j] = prS[j] = prQ[j] = 0.f;
  const bool odd = fq & 1;
  const bool pair = sizeof(TO) == 2 && (p.flags & GF_PAIRED_STORES);
#pragma unroll
  for (int i0 = 0; i0 < FN; i0 += IB) {
    f32x4 bv[IB], xv[IB], yv[IB];
    V4 rr[FM][IB];
    if constexpr (EARLY) {
      static_assert(MODE == 2 && IB == FN, "the early operands are the LayerNorm-residual form's, all fragment columns at once");
#pragma unroll
      for (int ii = 0; ii < IB; ++ii) {
        bv[ii] = early->bv[ii];
        if constexpr (EARLY_GB) { xv[ii] = early->xv[ii]; yv[ii] = early->yv[ii]; }
#pragma unroll
        for (int j = 0; j < FM; ++j) rr[j][ii] = early->rr[j][ii];
      }
      if constexpr (!EARLY_GB) {
        if (p.r_stats) {
#pragma unroll
          for (int ii = 0; ii < IB; ++ii) { xv[ii] = *(const f32x4*)(p.r_gamma + n + ii * 16); yv[ii] = *(const f32x4*)(p.r_beta + n + ii * 16); }
        } else {
#pragma unroll
          for (int ii = 0; ii < IB; ++ii) { xv[ii] = f32x4{1.f, 1.f, 1.f, 1.f}; yv[ii] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        }
      }
    } else {
#pragma unroll
      for (int ii = 0; ii < IB; ++ii) bv[ii] = *(const f32x4*)(p.bias + n + (i0 + ii) * 16);
      if constexpr (MODE == 1) {
#pragma unroll
        for (int ii = 0; ii < IB; ++ii) xv[ii] = *(const f32x4*)(p.w_colsum + n + (i0 + ii) * 16);
      } else {
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          const TO* rp = (const TO*)p.R + (long)min(m_base + j * 16 + fr, p.M - 1) * p.ldr + n;
#pragma unroll
          for (int ii = 0; ii < IB; ++ii) rr[j][ii] = *(const V4*)(rp + (i0 + ii) * 16);
        }
        if (p.r_stats) {
#pragma unroll
          for (int ii = 0; ii < IB; ++ii) { xv[ii] = *(const f32x4*)(p.r_gamma + n + (i0 + ii) * 16); yv[ii] = *(const f32x4*)(p.r_beta + n + (i0 + ii) * 16); }
        } else {
#pragma unroll
          for (int ii = 0; ii < IB; ++ii) { xv[ii] = f32x4{1.f, 1.f, 1.f, 1.f}; yv[ii] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        }
      }
    }
#pragma unroll
    for (int ii = 0; ii < IB; ++ii) {
      const int i = i0 + ii;
      V4 o[FM];
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float x = acc[i][j][e];
          if constexpr (MODE == 1) x = rs[j] * (x - mu[j] * xv[ii][e]);
          v[e] = act_out_c<TO, ACT>(x + bv[ii][e], p.act);
          if constexpr (MODE == 2) v[e] += fmaf(((float)rr[j][ii][e] - mu[j]) * rs[j], xv[ii][e], yv[ii][e]);
        }
        if constexpr (sizeof(TO) == 4) o[j] = V4{v[0], v[1], v[2], v[3]};
        else o[j] = pack4<TO>(v[0], v[1], v[2], v[3]);
        if constexpr (MODE == 2) {
          float pS = 0.f, pQ = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float w = (float)o[j][e]; pS += w; pQ = fmaf(w, w, pQ); }   // of what the consumer will read
          if ((i & 1) == 0) { tS[j] = pS; tQ[j] = pQ; }
          else {
            const float aS = tS[j] + pS, aQ = tQ[j] + pQ;
            if (FN == 2) { rowS[j] = aS; rowQ[j] = aQ; }
            else if ((i & 2) == 0) { prS[j] = aS; prQ[j] = aQ; }
            else { rowS[j] = prS[j] + aS; rowQ[j] = prQ[j] + aQ; }
          }
        }
      }
      bool stored = false;
      if constexpr (sizeof(TO) == 2) {
        if (pair) {     // lanes l and l ^ 16 swap one fragment row: one 16-byte store each (see pair_swap)
#pragma unroll
          for (int jp = 0; jp + 1 < FM; jp += 2) {
            const u32x4 w = pair_swap(__builtin_bit_cast(u32x2, o[jp]), __builtin_bit_cast(u32x2, o[jp + 1]), odd);
            const int m = m_base + jp * 16 + (odd ? 16 : 0) + fr;
            if (m < p.M) *(u32x4*)((TO*)p.C + (long)m * p.ldc + n + i * 16 - (odd ? 4 : 0)) = w;
          }
          if constexpr (FM % 2 == 1) {   // the last fragment row of the 192-row tile has no partner: plain 8-byte stores
            const int m2 = m_base + (FM - 1) * 16 + fr;
            if (m2 < p.M) *(V4*)((TO*)p.C + (long)m2 * p.ldc + n + i * 16) = o[FM - 1];
          }
          stored = true;
        }
      }
      if (!stored) {
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          const int m = m_base + j * 16 + fr;
          if (m < p.M) *(V4*)((TO*)p.C + (long)m * p.ldc + n + i * 16) = o[j];
        }
      }
    }
  }
  if constexpr (MODE == 2) {
    if (p.stats_out) {
      // row sums over this wave's slab: the 4 lane groups (fq) hold 4 columns of every fragment each
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        rowS[j] += __shfl_xor(rowS[j], 16, 64); rowS[j] += __shfl_xor(rowS[j], 32, 64);
        rowQ[j] += __shfl_xor(rowQ[j], 16, 64); rowQ[j] += __shfl_xor(rowQ[j], 32, 64);
        const int m = m_base + j * 16 + fr;
        if (fq == 0 && m < p.M) *(f32x2*)(p.stats_out + ((long)(n_base / SLAB) * p.M + m) * 2) = f32x2{rowS[j], rowQ[j]};
      }
    }
  }
}

// The 192-row tile: the row statistics are loaded HERE, in the epilogue (no registers to spare in the K loop).
template <typename TO, int FM, int FN, int MODE, int ACT>
__device__ __forceinline__ void gemm_epilogue_ln_late(const GemmArgs& p, const f32x4 (&acc)[FN][FM], int m_base, int n_base, int fr, int fq) {
  f32x2 late[FM][4];
  if constexpr (MODE == 1) ln_issue<FM>(p.a_stats, p.a_nt, p.M, m_base, fr, fq, late);
  else if (p.r_stats) ln_issue<FM>(p.r_stats, p.r_nt, p.M, m_base, fr, fq, late);
  gemm_epilogue_ln<TO, FM, FN, MODE, ACT>(p, acc, m_base, n_base, fr, fq, late);
}

// The epilogue of a gemm2_kernel / gemm2p_kernel instantiation that carries ONE family (EPI_PLAIN, EPI_LN_OPERAND, EPI_LN_RESIDUAL).
// LNK: the wave tile is one statistics slab, i.e. the LayerNorm forms exist (else the family falls back to the plain epilogue);
// LN_LATE: they load the statistics themselves, else `lnraw` holds what ln_issue requested before the K loop; EARLY: the
// LnResOps requested there too, or NoEarlyOps.
template <typename TO, int FM, int FN, int EPI, int ACTK, bool LNK, bool LN_LATE, int LR, typename EARLY>
__device__ __forceinline__ void gemm_run_epilogue(const GemmArgs& p, const f32x4 (&acc)[FN][FM], int z, int m_base, int n_base, int fr, int fq,
                                                  const f32x2 (&lnraw)[LR][4], const EARLY& early) {
  static_assert(EPI != EPI_ALL, "the run-time choice among all epilogues is gemm2_kernel's");
  if constexpr (EPI == EPI_PLAIN) gemm_epilogue<TO, FM, FN, false, true, ACTK>(p, acc, z, m_base, n_base, fr, fq);
  else if constexpr (!std::is_same_v<EARLY, NoEarlyOps>) gemm_epilogue_ln<TO, FM, FN, 2, ACTK, true, EARLY::gb>(p, acc, m_base, n_base, fr, fq, lnraw, &early);
  else if constexpr (LNK && LN_LATE) gemm_epilogue_ln_late<TO, FM, FN, EPI - 1, ACTK>(p, acc, m_base, n_base, fr, fq);
  else if constexpr (LNK) gemm_epilogue_ln<TO, FM, FN, EPI - 1, ACTK>(p, acc, m_base, n_base, fr, fq, lnraw);
  else gemm_epilogue<TO, FM, FN, sizeof(TO) == 2, false, ACTK>(p, acc, z, m_base, n_base, fr, fq);
}

template <typename T, typename TO, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs p) {
  constexpr int E = 16 / sizeof(T);     // elements per 16-B chunk
  constexpr int BKE = 128 / sizeof(T);  // K elements per tile
  constexpr int LA = BM / 32, LW = BN / 32;  // 16-B loads per thread per tile
  constexpr int FM = BM / 32, FN = BN / 32;  // 16x16 fragments per wave (wave tile = BM/2 x BN/2)
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (BM + BN) * 128];

  // XCD-aware tile order: the nt column tiles of one row panel run back to back on ONE XCD
  // (block ids congruent mod 8 share an XCD's L2), so the A panel is fetched from HBM once.
  const int pid = blockIdx.x;
  const int xcd = pid & 7, slot = pid >> 3;
  const int m_tile = (slot / p.nt) * 8 + xcd, n_tile = slot % p.nt;
  if (m_tile >= p.mt) return;
  const int z = blockIdx.z;
  const T* __restrict__ A = batch_a<T>(p, z);
  const T* __restrict__ W = batch_w<T>(p, z);
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  const int tid = threadIdx.x;

  // per-thread staging assignments (fixed across K steps)
  const T* a_ptr[LA]; bool a_ok[LA]; int a_lds[LA];
  const T* w_ptr[LW]; bool w_ok[LW]; int w_lds[LW];
  const int cc = tid & 7;
#pragma unroll
  for (int i = 0; i < LA; ++i) {
    const int row = (tid >> 3) + i * 32;
    const int m = m0 + row;
    a_ok[i] = m < p.M;
    const int mm = a_ok[i] ? m : 0;
    a_ptr[i] = A + a_row_offset(p, mm) + cc * E;
    a_lds[i] = lds_off(row, cc);
  }
#pragma unroll
  for (int i = 0; i < LW; ++i) {
    const int row = (tid >> 3) + i * 32;
    const int n = n0 + row;
    w_ok[i] = n < p.N;
    w_ptr[i] = W + (long)(w_ok[i] ? n : 0) * p.ldw + cc * E;
    w_lds[i] = BM * 128 + lds_off(row, cc);
  }

  u32x4 ra[LA], rw[LW];
  auto load_global = [&](int k0) {
    const bool kin = (k0 + cc * E) < p.K;
#pragma unroll
    for (int i = 0; i < LA; ++i)
      ra[i] = (a_ok[i] && kin) ? *(const u32x4*)(a_ptr[i] + k0) : u32x4{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < LW; ++i)
      rw[i] = (w_ok[i] && kin) ? *(const u32x4*)(w_ptr[i] + k0) : u32x4{0, 0, 0, 0};
  };
  auto store_lds = [&](int buf) {
    unsigned char* base = smem + buf * (BM + BN) * 128;
#pragma unroll
    for (int i = 0; i < LA; ++i) *(u32x4*)(base + a_lds[i]) = ra[i];
#pragma unroll
    for (int i = 0; i < LW; ++i) *(u32x4*)(base + w_lds[i]) = rw[i];
  };

  const FragLane l = frag_lane<BM, BN, 2, 2>(tid);
  f32x4 acc[FN][FM];
  zero_acc(acc);

  const int nk = (p.K + BKE - 1) / BKE;
  load_global(0);
  store_lds(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_global((kt + 1) * BKE);
    const unsigned char* sa = smem + cur * (BM + BN) * 128;
    k_tile_mma<T, FM, FN>(sa, sa + BM * 128, l, acc);
    if (kt + 1 < nk) store_lds(cur ^ 1);
    __syncthreads();
  }

  gemm_epilogue<TO, FM, FN>(p, acc, z, m0 + l.wm, n0 + l.wn, l.fr, l.fq);
}

// ---------------------------------------------------------------------------------------------------
// bf16 kernel v2: LDS-DMA staging (global_load_lds, 16 B/lane) into an NSTAGE-deep LDS ring, counted
// s_waitcnt vmcnt so NSTAGE-2 K tiles stay in flight ACROSS the (single, raw) barrier of each K step.
// Same LDS image / swizzle / fragment reads / epilogue as v1; the swizzle moves to the per-lane SOURCE
// address because an LDS-DMA wave-instruction writes 1 KiB linearly (cdna_hip_programming.md rule 21).
// Requires K % 64 == 0 (no K tail: LDS-DMA cannot zero-fill); out-of-range rows are clamped to a valid
// row (their products are never stored).
// EPI: which epilogues this instantiation carries.  0 = all of them behind run-time tests (training: pre-activation copy,
// dropout, activation backward, both LayerNorm forms); 1 = the plain inference epilogue only (bias, activation, residual);
// 2 / 3 = the LayerNorm-operand / LayerNorm-residual form only.  One instantiation with everything is 127 KB of code of which a
// launch executes a few KB scattered among the branches it does not take: per-workgroup time stamps put the
// epilogue of a 128 x 128 tile at 3.0 us for 32 outputs per lane (bias only), most of it instruction fetch.
// EPIA = EPI + 10 * (1 + activation) when the activation is compiled in as well (11 / 21 plain with none / GELU, 12 / 22
// LayerNorm-operand with none / GELU, 13 LayerNorm-residual with none): see act_out_c.
// The waves that stage a K tile of `slots` LDS-DMA wave-instructions (1 KB each): all `waves` of them where that divides, else the
// largest count that does (the 160 x 128 tile: 36 slots, 9 of its 10 waves with 4 each; the tenth issues none, so every wave's
// counted wait stays one compile-time constant that is right for it -- a wave with nothing in flight passes it at once).
constexpr int gemm2_loader_waves(int slots, int waves) {
  int w = waves;
  while (slots % w) --w;
  return w;
}

template <typename TO, int BM, int BN, int WM, int WN, int NSTAGE, bool PIPE = false, typename TI = bf16_t, int EPIA = 0>
// 8-wave workgroups whose ring fits twice into a CU's LDS are MEANT to run two per CU: 4 waves per SIMD = 128 registers
// (the 192-row tile's LayerNorm epilogues drifted to 145 once, i.e. to one workgroup per CU: HuBERT-large 18.7 -> 21.4 ms).
// Its everything-epilogue instantiation (EPI 0: dropout / pre-activation copies on a tall grid, no caller on the path) does not
// fit 128 without spilling and keeps the register count the compiler picks.
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 8 && NSTAGE * (BM + BN) * 128 <= 80 * 1024 && (epia_family(EPIA) != EPI_ALL || BM * BN <= 128 * 128)) ? 4 : 1) void gemm2_kernel(const GemmArgs p) {
  constexpr int EPI = epia_family(EPIA), ACTK = epia_act(EPIA);
  constexpr int NW = WM * WN;
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int NLW = gemm2_loader_waves((BM + BN) / 8, NW);   // waves that issue LDS-DMA
  constexpr int LPT = (BM + BN) / 8 / NLW;  // LDS-DMA instructions per thread of a loader wave per K tile
  constexpr int FM = BM / WM / 16, FN = BN / WN / 16;
  static_assert((BM + BN) % 8 == 0 && (NLW == NW || NLW * 2 > NW), "tile chunks must divide over the loader waves");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  int m_tile, n_tile;
  const int pid = blockIdx.x;
  if (!xcd_tile(p, pid, m_tile, n_tile)) return;
  const int z = blockIdx.z;
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  const int tid = threadIdx.x;

  TileSrc<bf16_t, BM, BN, NLW> src;
  src.set(p, batch_a<bf16_t>(p, z), batch_w<bf16_t>(p, z), m0, n0, tid);
  const bool loader = NLW == NW || __builtin_amdgcn_readfirstlane(tid >> 6) < NLW;
  auto issue = [&](int kt, int stage) {
    if constexpr (NLW != NW) { if (!loader) return; }
    src.issue(smem + stage * STAGE, kt, tid);
  };

  const FragLane l = frag_lane<BM, BN, WM, WN>(tid);
  const int wm = l.wm, wn = l.wn, fr = l.fr, fq = l.fq;
  f32x4 acc[FN][FM];
  zero_acc(acc);

  const int nk = p.K / 64;
  // The 4-wave 64 x 128 kernel (one workgroup per CU, 256 registers) requests everything its LayerNorm-residual epilogue reads
  // -- the row statistics, bias, residual fragments, gamma / beta -- in front of the ring's prologue: the counted waits of the
  // K loop retire them with the first K tile, and the epilogue starts on registers.  The 10-wave 160 x 128 kernel (three waves on a
  // SIMD: 168 registers) does the same without gamma / beta (EARLY_GB; 152 registers, all four: 68 bytes of scratch).  Requested behind
  // the prologue instead, the first counted wait would take them for ring stages and wait for three K tiles, not one.
  constexpr bool LNK = (BN == 128 || BN == 64) && WN == 2 && (FM == 2 || FM == 3) && sizeof(TO) == 2;   // slab = BN / 2
  // the 192-row tile has no registers to spare during the K loop (124 of 128): its statistics are loaded in the epilogue instead
  // (one batched round trip; with two workgroups per CU and grids of many rounds it hides under the neighbour's K loop)
  constexpr bool LN_LATE = FM == 3;
  constexpr bool EARLY_OPS = LNK && EPI == 3 && ((NW == 4 && BM == 64) || (NW == 10 && BM == 160)) && BN == 128;
  f32x2 lnraw[(LNK && !LN_LATE) ? FM : 1][4];
  constexpr bool EARLY_GB = NW == 4;
  std::conditional_t<EARLY_OPS, LnResOps<TO, FM, FN, EARLY_GB>, NoEarlyOps> early;
  if constexpr (EARLY_OPS) {
    if (p.r_stats) ln_issue<FM>(p.r_stats, p.r_nt, p.M, m0 + wm, fr, fq, lnraw);
    ln_res_issue<TO, FM, FN, EARLY_GB>(p, m0 + wm, n0 + wn, fr, fq, early);
  }
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s)
    if (s < nk) issue(s, s);
  if (p.stagger_ticks > 0 && ((pid >> 8) & 1) && pid < 512) {
    // Two co-resident workgroups that start together stay in lockstep for the whole launch (both multiply, then both run
    // their epilogues, then their two successors start together): the second one of each CU waits half a tile period once,
    // with its first stage already in flight, so that from then on one workgroup's prologue / epilogue runs beside the
    // other's K loop
    const unsigned long t0 = __builtin_amdgcn_s_memrealtime();
    while ((long)(__builtin_amdgcn_s_memrealtime() - t0) < p.stagger_ticks) __builtin_amdgcn_s_sleep(16);
  }
  // LayerNorm-folding mode (msmd_gemm_ln; the 4 x 2-wave 128 x 128 tile only): the row statistics' loads go out now, consumed in the epilogue
  if constexpr (LNK && !LN_LATE && EPI != 1 && !EARLY_OPS) {
    if (EPI == 2 || (EPI == 0 && p.a_stats)) ln_issue<FM>(p.a_stats, p.a_nt, p.M, m0 + wm, fr, fq, lnraw);
    else if (p.r_stats) ln_issue<FM>(p.r_stats, p.r_nt, p.M, m0 + wm, fr, fq, lnraw);
  }
  int stage = 0;
  for (int kt = 0; kt < nk; ++kt) {
    ring_step<NSTAGE, LPT>(kt, nk, stage, issue);
    const unsigned char* sa = smem + stage * STAGE;
    if constexpr (PIPE) k_tile_mma_pipelined<TI, FM, FN>(sa, sa + BM * 128, l, acc);
    else k_tile_mma<TI, FM, FN>(sa, sa + BM * 128, l, acc);
    stage = ring_next<NSTAGE>(stage);
  }
  // the 192-row tile has no register to spare: the lane's fragment coordinates are derived again here instead of living
  // through the K loop (one of them went to scratch otherwise)
  const FragLane le = frag_lane<BM, BN, WM, WN>(LN_LATE ? opaque_tid(tid) : tid);
  if constexpr (EPI != EPI_ALL) {
    gemm_run_epilogue<TO, FM, FN, EPI, ACTK, LNK, LN_LATE>(p, acc, z, m0 + le.wm, n0 + le.wn, le.fr, le.fq, lnraw, early);
  } else {
    // every epilogue behind run-time tests: the form the call's pointers ask for.  (Spelled out in a lambda, the 192-row tile's late
    // statistics with it: as a function of the arguments, or with gemm_epilogue_ln_late per branch, the compiler emits one more
    // load of a statistics pair in the 64-row and 192-row tiles, and the 192-row tile takes 128 registers instead of 124.)
    const int wm_e = le.wm, wn_e = le.wn, fr_e = le.fr, fq_e = le.fq;
    auto run_epilogue = [&]() {
      if constexpr (LNK && !LN_LATE) {
        if (p.a_stats) { gemm_epilogue_ln<TO, FM, FN, 1, ACTK>(p, acc, m0 + wm_e, n0 + wn_e, fr_e, fq_e, lnraw); return; }
        if (p.r_stats || p.stats_out) { gemm_epilogue_ln<TO, FM, FN, 2, ACTK>(p, acc, m0 + wm_e, n0 + wn_e, fr_e, fq_e, lnraw); return; }
      }
      if constexpr (LNK && LN_LATE) {
        if (p.a_stats || p.r_stats || p.stats_out) {
          f32x2 late[FM][4];
          if (p.a_stats) ln_issue<FM>(p.a_stats, p.a_nt, p.M, m0 + wm_e, fr_e, fq_e, late);
          else if (p.r_stats) ln_issue<FM>(p.r_stats, p.r_nt, p.M, m0 + wm_e, fr_e, fq_e, late);
          if (p.a_stats) gemm_epilogue_ln<TO, FM, FN, 1, ACTK>(p, acc, m0 + wm_e, n0 + wn_e, fr_e, fq_e, late);
          else gemm_epilogue_ln<TO, FM, FN, 2, ACTK>(p, acc, m0 + wm_e, n0 + wn_e, fr_e, fq_e, late);
          return;
        }
      }
      gemm_epilogue<TO, FM, FN, sizeof(TO) == 2, false, ACTK>(p, acc, z, m0 + wm_e, n0 + wn_e, fr_e, fq_e);
    };
    run_epilogue();
  }
}

// ---------------------------------------------------------------------------------------------------
// Persistent form of gemm2_kernel<.., 2 stages, pipelined> for launches of MORE THAN ONE ROUND (more tiles than the 512
// workgroups the chip holds at two per CU).  The grid is 512 workgroups; workgroup b multiplies the tiles gemm2_kernel's blocks
// b, b + 512, b + 1024, ... would (same XCD: 512 % 8 == 0) -- and the operand stream never drains between them: the LAST K
// tile of a tile issues the FIRST stage of the next one, so the next tile's prologue (addresses, the first operand round
// trip: 1.2-1.9 us per workgroup on the stamps of DESIGN.md 5d) runs under this tile's last multiply and its epilogue, and
// there is no workgroup retirement / dispatch between rounds (0.8 us on the same stamps).  Per tile the products, their
// order and the epilogue are gemm2_kernel's: results are bit-identical.
template <typename TO, int BM, int BN, int WM, int WN, typename TI, int EPIA>
__global__ __launch_bounds__(WM * WN * 64, 4) void gemm2p_kernel(const GemmArgs p) {
  constexpr int EPI = epia_family(EPIA), ACTK = epia_act(EPIA);
  constexpr int NW = WM * WN;
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int FM = BM / WM / 16, FN = BN / WN / 16;
  static_assert(EPI >= 1 && EPI <= 3 && sizeof(TO) == 2 && NW == 8 && WN == 2 && BN == 128 && (FM == 2 || FM == 3), "the hot 8-wave tiles, inference epilogues");
  constexpr bool LN_LATE = FM == 3;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int xm_n = 8 / p.xn, ntx = (p.nt + p.xn - 1) / p.xn;
  const int vgrid = ((p.mt + xm_n - 1) / xm_n) * ntx * 8;      // gemm2_kernel's grid
  const TI* __restrict__ A = (const TI*)p.A;
  const TI* __restrict__ W = (const TI*)p.W;
  // first block id >= vb of this workgroup's sequence that maps to a tile (the XCD grid pads), or -1
  auto next_tile = [&](int vb, int& m0, int& n0) -> int {
    for (; vb < vgrid; vb += gridDim.x) {
      int m_tile, n_tile;
      if (xcd_tile(p, vb, m_tile, n_tile)) { m0 = m_tile * BM; n0 = n_tile * BN; return vb; }
    }
    return -1;
  };
  // Everything derived from the lane id is derived AGAIN per tile and per phase (t_k for the K loop, another for the epilogue) from
  // copies the compiler cannot match (opaque_tid): kept across the tile loop, the K loop's fragment / staging offsets would be live in
  // the epilogue and the epilogue's in the K loop (+30 registers: 90-250 bytes of scratch in every LayerNorm form)
  TileSrc<TI, BM, BN, NW> src;
  int m0 = 0, n0 = 0;
  int vb = next_tile(blockIdx.x, m0, n0);
  if (vb < 0) return;
  const int nk = p.K / 64;
  src.set(p, A, W, m0, n0, tid);
  int stage = 0;
  src.issue(smem, 0, tid);
  for (;;) {
    const int t_k = opaque_tid(tid);
    const FragLane l = frag_lane<BM, BN, WM, WN>(t_k);
    f32x2 lnraw[LN_LATE ? 1 : FM][4];
    if constexpr (!LN_LATE && EPI != 1) {
      if constexpr (EPI == 2) ln_issue<FM>(p.a_stats, p.a_nt, p.M, m0 + l.wm, l.fr, l.fq, lnraw);
      else if (p.r_stats) ln_issue<FM>(p.r_stats, p.r_nt, p.M, m0 + l.wm, l.fr, l.fq, lnraw);
    }
    f32x4 acc[FN][FM];
    zero_acc(acc);
    int m0n = 0, n0n = 0, vbn = -1;
    for (int kt = 0; kt < nk; ++kt) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 1 < nk) {
        src.issue(smem + (stage ^ 1) * STAGE, kt + 1, t_k);
      } else {
        // the other stage is free (every wave is past this barrier, i.e. done reading it): the next tile's first stage
        vbn = next_tile(vb + (int)gridDim.x, m0n, n0n);
        if (vbn >= 0) { src.set(p, A, W, m0n, n0n, t_k); src.issue(smem + (stage ^ 1) * STAGE, 0, t_k); }
      }
      const unsigned char* sa = smem + stage * STAGE;
      k_tile_mma_pipelined<TI, FM, FN>(sa, sa + BM * 128, l, acc);
      stage ^= 1;
    }
    const FragLane le = frag_lane<BM, BN, WM, WN>(opaque_tid(tid));
    gemm_run_epilogue<TO, FM, FN, EPI, ACTK, true, LN_LATE>(p, acc, 0, m0 + le.wm, n0 + le.wn, le.fr, le.fq, lnraw, NoEarlyOps{});
    if (vbn < 0) break;
    vb = vbn; m0 = m0n; n0 = n0n;
    // the operand addresses again, from values the compiler cannot match with the ones above: they are NOT kept in
    // registers across the epilogue (8 registers the LayerNorm epilogues do not have)
    asm volatile("" : "+s"(m0), "+s"(n0));
    src.set(p, A, W, m0, n0, opaque_tid(tid));
  }
}

// ---------------------------------------------------------------------------------------------------
// MSMD_F16X2 ("split pair", common.h) kernel: the parity-grade speed mode.  Operands are rows of 2K fp16 numbers in
// 32-element blocks [hi x 32 | lo x 32], so ONE 128-byte line = one 32-deep k-step of both planes and the LDS-DMA
// ring, LDS image, swizzle and fragment reads are those of gemm2_kernel (chunks 0-3 of a row = hi, 4-7 = lo).  Per
// k-step and fragment pair: acc0 += Wh.Ah, acc1 += Wh.Al + Wl.Ah (three v_mfma_f32_16x16x32_f16), result
// acc0 + acc1 / 2048.  The launcher passes lda / ldw / strides of A and W already doubled (fp16 units); K stays logical.
// TO = float (fp32 C and residual) or f16_t (C and residual in split storage).
// ACT: see act_out_c (>= 0: a constant of the kernel).  GELU through the 12-instruction erf (|abs err| <= 1.5e-7, i.e.
// <= 0.5 |x| 1.5e-7 on the output: the size of an fp32 rounding error at these magnitudes); libm's erff would be ~15 % of an
// FFN1 launch.
template <int ACT> __device__ __forceinline__ float act_split(float x, int act) {
  if constexpr (ACT == MSMD_ACT_GELU) return gelu_fast(x);
  else if constexpr (ACT == MSMD_ACT_NONE) return x;
  else return act == MSMD_ACT_GELU ? gelu_fast(x) : apply_act(x, act);
}

template <int FM, int FN, int ACT = -1>
__device__ __forceinline__ void gemm_epilogue_split(const GemmArgs& p, const f32x4 (&acc)[FN][FM], int z, int m_base,
                                                    int n_base, int fr, int fq) {
  f16_t* __restrict__ C = (f16_t*)p.C + 2 * ((z / p.batch_inner) * p.strideC + (z % p.batch_inner) * p.strideC2);
  const f16_t* __restrict__ R = p.R ? (const f16_t*)p.R + 2 * (z * p.strideR) : nullptr;
  const float* __restrict__ bias = p.bias ? p.bias + z * p.strideBias : nullptr;
  if (m_base + FM * 16 <= p.M && n_base + FN * 16 <= p.N) {
    // interior tiles: straight-line code, every load (bias, both halves of every residual fragment) requested before the
    // first store -- between the stores they are serialised into one L2 round trip per fragment (see gemm_epilogue_interior)
    const int n = n_base + fq * 4;
    f32x4 bv[FN];
#pragma unroll
    for (int i = 0; i < FN; ++i) bv[i] = bias ? *(const f32x4*)(bias + n + i * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
    f16x4 rh[FM][FN], rl[FM][FN];
    if (R) {
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        const f16_t* rrow = R + (long)(m_base + j * 16 + fr) * 2 * p.ldr;
#pragma unroll
        for (int i = 0; i < FN; ++i) {
          const f16_t* q = rrow + split_col(n + i * 16);
          rh[j][i] = *(const f16x4*)q;
          rl[j][i] = *(const f16x4*)(q + 32);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      f16_t* crow = C + (long)(m_base + j * 16 + fr) * 2 * p.ldc;
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_split<ACT>(acc[i][j][e] + bv[i][e], p.act);
        if (R) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += unsplit_f16x2(rh[j][i][e], rl[j][i][e]);
        }
        store4_split(crow, n + i * 16, v);
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < FN; ++i) {
    const int n = n_base + i * 16 + fq * 4;
    if (n >= p.N) continue;   // N % 4 == 0 (launcher)
    const f32x4 bv = bias ? *(const f32x4*)(bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int m = m_base + j * 16 + fr;
      if (m >= p.M) continue;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_split<ACT>(acc[i][j][e] + bv[e], p.act);
      if (R) {
        float r[4];
        load4_split(R + (long)m * 2 * p.ldr, n, r);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += r[e];
      }
      store4_split(C + (long)m * 2 * p.ldc, n, v);
    }
  }
}

// WS (the call carries MSMD_GEMM_W_BELOW_32, i.e. W is a model weight): gemm8_kernel's fold-free form -- W's hi fragments x 2^11
// in registers, ONE accumulator in units of 2^-11, per K tile and output element the products Wh.AL, WL.Ah, (2^11 Wh).Ah in
// this order -- so that a launch returns the same bits whether its row count routes it to this kernel or to the 256 x 256 one.
template <typename TO, int BM, int BN, int WM, int WN, int NSTAGE, int ACTK = -1, bool WS = false>
__global__ __launch_bounds__(WM * WN * 64) void gemm2s_kernel(const GemmArgs p) {
  constexpr int NW = WM * WN;
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int FM = BM / WM / 16, FN = BN / WN / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  int m_tile, n_tile;
  if (!xcd_tile(p, blockIdx.x, m_tile, n_tile)) return;
  const int z = blockIdx.z;
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  const int tid = threadIdx.x;

  TileSrc<f16_t, BM, BN, NW> src;
  constexpr int LPT = decltype(src)::LPT;
  src.set(p, batch_a<f16_t>(p, z), batch_w<f16_t>(p, z), m0, n0, tid);
  auto issue = [&](int kt, int stage) { src.issue(smem + stage * STAGE, kt, tid); };

  const FragLane l = frag_lane<BM, BN, WM, WN>(tid);
  const int wm = l.wm, wn = l.wn, fr = l.fr, fq = l.fq;
  f32x4 acc0[FN][FM], acc1[FN][FM];
  zero_acc(acc0);
  zero_acc(acc1);

  const int nk = p.K / 32;
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s)
    if (s < nk) issue(s, s);
  int stage = 0;
  for (int kt = 0; kt < nk; ++kt) {
    ring_step<NSTAGE, LPT>(kt, nk, stage, issue);
    const unsigned char* sa = smem + stage * STAGE;
    const unsigned char* sw = sa + BM * 128;
    u32x4 ah[FM], al[FM], wh[FN], wl[FN];
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      ah[j] = *(const u32x4*)(sa + lds_off(wm + j * 16 + fr, fq));
      al[j] = *(const u32x4*)(sa + lds_off(wm + j * 16 + fr, 4 + fq));
    }
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      wh[i] = *(const u32x4*)(sw + lds_off(wn + i * 16 + fr, fq));
      wl[i] = *(const u32x4*)(sw + lds_off(wn + i * 16 + fr, 4 + fq));
    }
    if constexpr (WS) {
      u32x4 ws[FN];
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        f16x8 h = __builtin_bit_cast(f16x8, wh[i]);
        h = h * (f16_t)MSMD_SPLIT_SCALE;
        ws[i] = __builtin_bit_cast(u32x4, h);
      }
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) Mfma<f16_t>::run(wh[i], al[j], acc0[i][j]);
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) Mfma<f16_t>::run(wl[i], ah[j], acc0[i][j]);
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) Mfma<f16_t>::run(ws[i], ah[j], acc0[i][j]);
    } else {
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          Mfma<f16_t>::run(wh[i], ah[j], acc0[i][j]);
          Mfma<f16_t>::run(wh[i], al[j], acc1[i][j]);
          Mfma<f16_t>::run(wl[i], ah[j], acc1[i][j]);
        }
    }
    stage = ring_next<NSTAGE>(stage);
  }
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        acc0[i][j][e] = WS ? acc0[i][j][e] * MSMD_SPLIT_INV : fmaf(acc1[i][j][e], MSMD_SPLIT_INV, acc0[i][j][e]);   // (x 2^-11: exact)
  if constexpr (sizeof(TO) == 4) gemm_epilogue<float, FM, FN, false, false, ACTK>(p, acc0, z, m0 + wm, n0 + wn, fr, fq);
  else gemm_epilogue_split<FM, FN, ACTK>(p, acc0, z, m0 + wm, n0 + wn, fr, fq);
}

// ---------------------------------------------------------------------------------------------------
// gemm8_kernel: 256 x 256 x 64 tiles, ONE 8-wave workgroup per CU, the 8-phase schedule of cdna_hip_programming.md section 5
// ("The 256^2 8-phase template") on this library's operand layout.  tools/gemm8_probe.hip is the bare schedule: 1 305 TFLOP/s at
// 4096^3 and 1 303 at 16384 x 4096 x 3072 on random operands (the guide quotes 1 320-1 340 / 1 470 at 4096^3 / 8192^3) against
// 1 012-1 105 for the 128 x 128 / 192 x 128 kernels above -- round 3's first attempt at this schedule (gemm8p, removed:
// 902) lost a third of that to a branch around every staging step, per-fragment epilogues that fell into 528 bytes of
// scratch and 8-byte stores in 32-byte runs.  What is different here:
//   * the steady-state K tile is branch-free (the last two K tiles are separate copies without staging);
//   * the epilogue goes through LDS: accumulators are written as fp32 into a 64-row x 256-column block (two blocks of 64 KB =
//     the operand ring, alternating), then every wave takes whole 1 KB rows back -- a lane owns 4 consecutive columns of one
//     row per step -- so bias / activation / both LayerNorm forms / residual are a few registers of per-column constants and
//     per-row scalars, residual rows are read and output rows written as whole 512-byte runs, and the statistics of the
//     stored rows (64-column slabs, the layout the 128 x 128 kernels write) are four 16-lane reductions.
//   waves: 2 (wr, along M) x 4 (wc, along N); a wave owns 64 rows of EACH 128-row half of the X tile and 32 columns of EACH
//   128-column half of the W tile: four 64 x 32 quadrants (h, g), 16 MFMAs each per K tile = one PHASE; the two wave rows run
//   one barrier apart, so one multiplies while the other reads fragments and issues the next loads.
//   LDS: 2 K-tile buffers x {X0, X1, W0, W1} half-tiles of 128 rows x 128 bytes (16 KB, swizzled as everywhere here) = 128 KB.
//   phase p of K tile t (buffer t & 1):  fragment reads | ONE half-tile of LDS-DMA (2 pieces per thread) | [counted vmcnt,
//   phase 4 only] | s_barrier | 16 MFMAs | s_barrier
//     ph1: reads W0 (4, issued first) + X0 (8), lgkmcnt(8) retires the W0 reads before the barrier;  quadrant (0,0);  stages X1(t+1)
//     ph2: reads W1 (4);                                                                         quadrant (0,1);  stages W0(t+2)
//     ph3: reads X1 (8);                                                                         quadrant (1,1);  stages X0(t+2)
//     ph4: no reads (W0 is still in registers);  vmcnt(6) -> K tile t+1 has landed;              quadrant (1,0);  stages W1(t+2)
// Per output element the products and their order are gemm2_kernel's (k ascending, one 16x16x32 MFMA per 32): the plain
// outputs are bit-identical to the 128 x 128 kernels'; the row statistics of the LayerNorm forms are summed in another order.
// Calls it takes (launch_gemm8): 16-bit operands and output, N % 256 == 0, K % 64 == 0, K >= 128, one problem per launch,
// inference epilogues (EPIA 11 / 21 plain, 12 / 22 LayerNorm-operand, 13 LayerNorm-residual + statistics).
//
// SPLIT (round 6): the same tile, ring and schedule on MSMD_F16X2 split-pair operands (TI = f16_t; gemm2s_kernel's storage: a
// 128-byte row piece = [hi x 32 | lo x 32] of 32 logical k).  A K tile is then 32 logical k, its "k-step 0" fragments (chunks
// 0-3) are the hi planes and its "k-step 1" fragments (chunks 4-7) the lo planes: staging, LDS image and every fragment address
// are unchanged, only the multiplies differ -- per fragment pair  t = Wh.Al + Wl.Ah  (two MFMAs from a zero accumulator),
// acc = fma(t, 2^-11, acc)  (four vector FMAs, issued under the neighbouring MFMAs),  acc += Wh.Ah:  24 MFMAs per phase
// instead of 16 on the same LDS bytes.  The cross terms are folded once per K tile because a second accumulator set for the
// whole K loop (gemm2s_kernel's acc1) would be another 128 registers.  SPLIT = 1: C and the residual in split storage; 2: fp32.
// SPLIT + 4 (the caller states |W| < 32, MSMD_GEMM_W_BELOW_32): no fold at all -- the wave multiplies its hi-plane W fragments
// by 2^11 in registers (four v_pk_mul_f16 per fragment, exact below 32 in magnitude), so that  (2^11 Wh).Ah + Wh.AL + WL.Ah  is
// ONE sum in units of 2^-11 (AL / WL = the stored lo planes, already x 2^11), scaled back in the epilogue: 16 vector
// instructions per K tile instead of 128, one accumulator set, the matrix pipe 11-17 % busier (conv1 875 -> 779 us, QKV 81 ->
// 68, same box).  LayerNorm forms are not built for it (the split path runs LayerNorm as its own kernel): EPI = 1 only.
//
// CHAIN (msmd_conv_chain): the same K loop and epilogue walk the tiles of 2 to 4 problems, problem l's A being problem
// l - 1's C, in ONE launch.  Tiles are taken by TICKET from one global counter, problem-major and row-block ascending, so a
// workgroup only ever waits for tiles with a lower ticket, which a running workgroup already holds: the launch makes progress
// with any number of resident workgroups.  A finished tile adds one to its row block's counter (the hand-over of
// cdna_hip_programming.md Guideline 16: every storing wave drains, barrier, one lane signals); a consumer tile needs the
// counters of the producer row blocks its windows read at `nt`.  The next ticket is claimed in K tile nk - 2 and its counters are
// read under the last K tile: when they are already full (the producers ran rounds earlier) wave 0 acquires before the barrier
// that ends the K loop and the next tile's first K tile is staged under this tile's epilogue as in the plain kernel; else the
// workgroup waits behind its epilogue, W staged, A not.  Every wait is bounded by CHAIN_WAIT_TICKS of the 100 MHz clock.
struct ChainProblem {
  const void* A; const void* W; const float* bias; void* C;
  long lda, a_batch_stride;      // elements, as GemmArgs
  int M, rows_per_batch, K, mt;
  int t_in, stride, taps;        // rows per clip of A (= the producer's C), window step and length in rows
  int ticket0, cnt0;             // the problem's first ticket; its first row-block counter in the state block
  float inv_rpb;
};
struct ChainTable {
  ChainProblem pr[4];
  unsigned* state;               // [0] ticket counter, [1] status, [CHAIN_STATE_HEAD + cnt0 + row block] finished column tiles
  int n, nt, per_block, total;   // problems; column tiles; 1 = a ticket is a row block (all its column tiles), 0 = one tile; tickets
  int release;                   // 1 = plain stores + one agent-scope release per tile, 0 = write-through stores
};
struct NoChain : ChainTable {};      // the plain kernel: an empty table nothing reads (the chain statements are discarded there)
struct ChainTile { int l, rb, ct, nct, pb0, pb1; };      // problem, row block, first column tile and their number, producer row blocks
constexpr int CHAIN_STATE_HEAD = 4;
constexpr long CHAIN_WAIT_TICKS = 2000000;      // 20 ms per wait (more than 10 x the whole launch at the bench shape)

// ticket -> tile and the producer row blocks it reads (host and device: msmd_conv_chain_plan is this function)
__host__ __device__ inline bool chain_decode(const ChainTable& t, int ticket, ChainTile& o) {
  if (ticket < 0 || ticket >= t.total) return false;
  int l = 0;
  for (int i = 1; i < t.n; ++i)
    if (ticket >= t.pr[i].ticket0) l = i;
  const ChainProblem& q = t.pr[l];
  const int local = ticket - q.ticket0;
  o.l = l; o.pb0 = 0; o.pb1 = -1;
  if (t.per_block) { o.rb = local; o.ct = 0; o.nct = t.nt; }
  else { o.rb = local / t.nt; o.ct = local - o.rb * t.nt; o.nct = 1; }
  if (l > 0) {
    // rows r0 .. r1 of this problem read the rows [first row of r0's window, last tap of r1's window] of the producer's output,
    // clip after clip: every row block in between, whole clips included
    const int r0 = o.rb * 256, r1 = (r0 + 255 < q.M ? r0 + 255 : q.M - 1);
    const int q0 = r0 / q.rows_per_batch, q1 = r1 / q.rows_per_batch;
    const int first = q0 * q.t_in + (r0 - q0 * q.rows_per_batch) * q.stride;
    const int last = q1 * q.t_in + (r1 - q1 * q.rows_per_batch) * q.stride + q.taps - 1;
    o.pb0 = first >> 8; o.pb1 = last >> 8;
  }
  return true;
}

template <typename TI, int EPIA, int SPLIT, typename PA, typename CH>
__device__ __forceinline__ void gemm8_body(PA& p, const CH& ch) {
  constexpr bool CHAIN = !std::is_same_v<CH, NoChain>;
  static_assert(!CHAIN || (SPLIT == 0 && epia_family(EPIA) == EPI_PLAIN), "the chained form: 16-bit operands, plain epilogue");
  typedef typename std::conditional<(SPLIT & 3) == 2, float, TI>::type TO;
  constexpr bool WS = (SPLIT & 4) != 0;   // W's hi plane scaled in registers, single accumulator
  constexpr int EPI = epia_family(EPIA), ACTK = epia_act(EPIA);
  static_assert(SPLIT == 0 || (EPI == 1 && __is_same(TI, f16_t)), "split operands: fp16 planes, plain epilogue");
  constexpr int HALF = 128 * 128;        // bytes of one half-tile
  constexpr int BUF = 4 * HALF;          // X0 X1 W0 W1
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  // Tile order: workgroups pid, pid + 8, ... share an XCD (one L2); each XCD takes one contiguous run of the row-major tile
  // list -- counts differ by at most one, which matters at ONE workgroup per CU (the (8 / xn) x xn XCD grid of the kernels
  // above leaves XCDs with 39 and 26 tiles of the 225 of 6400 x 2304: two rounds).  The grid is min(tiles, 256) workgroups:
  // a workgroup walks its XCD's run with the stride of that XCD's workgroup count (persistent: see the tile loop below).
  const int pid = blockIdx.x, ntiles = p.mt * p.nt, nwg = gridDim.x;
  const int xcd = pid & 7;
  const int run0 = (xcd < (ntiles & 7) ? xcd * ((ntiles >> 3) + 1) : (ntiles & 7) * ((ntiles >> 3) + 1) + (xcd - (ntiles & 7)) * (ntiles >> 3));
  const int run_n = (ntiles >> 3) + (xcd < (ntiles & 7) ? 1 : 0);
  const int stride = (nwg >> 3) + (xcd < (nwg & 7) ? 1 : 0);
  int tl = pid >> 3;                     // position in the XCD's run
  const bf16_t* A = (const bf16_t*)p.A;
  const bf16_t* W = (const bf16_t*)p.W;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;

  // CHAIN: the tile this workgroup takes next (cz), what is left of its ticket, and the mailbox behind the ring through which wave 0
  // tells the workgroup the ticket it claimed ([0], -1 = none left or a wait expired) and whether its producers are done ([1])
  ChainTile cz{};
  int c_left = 0;
  volatile int* mbox = (volatile int*)(smem + 2 * BUF);
  unsigned c_claim = 0, c_cnt = 0;       // wave 0: the claimed ticket (lane 0), the counters of its producer row blocks (one per lane)
  // the problem of tile cz: the operands the staging reads (the epilogue of the tile before keeps its own copies)
  auto chain_problem = [&]() {
    if constexpr (CHAIN) {
      const ChainProblem& q = ch.pr[cz.l];
      p.A = q.A; p.W = q.W; p.bias = q.bias; p.C = q.C; p.M = q.M; p.K = q.K; p.ldw = q.K;
      p.lda = q.lda; p.a_batch_stride = q.a_batch_stride; p.rows_per_batch = q.rows_per_batch; p.inv_rpb = q.inv_rpb;
      A = (const bf16_t*)q.A; W = (const bf16_t*)q.W;
    }
  };
  // all of wave 0: are the producer row blocks of cz finished (counters at nt)?  Relaxed loads, one counter per lane.
  auto chain_counters = [&](const ChainTile& z) -> unsigned {
    unsigned c = ~0u;
    if constexpr (CHAIN) {
      if (z.l > 0) {
        const unsigned* cnt = ch.state + CHAIN_STATE_HEAD + ch.pr[z.l - 1].cnt0;
        c = (unsigned)ch.nt;
        for (int b = z.pb0 + lane; b <= z.pb1; b += 64) {
          const unsigned v = __hip_atomic_load(cnt + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          c = v < c ? v : c;
        }
      }
    }
    return c;
  };
  // all of wave 0, behind the epilogue: poll until they are, bounded by wall clock; then ONE agent-scope acquire, drained, ahead of the
  // workgroup's barrier.  False: the wait expired (status word set).
  auto chain_wait = [&](const ChainTile& z) -> bool {
    if constexpr (CHAIN) {
      if (z.l == 0) return true;
      const long t0 = (long)__builtin_amdgcn_s_memrealtime();
      while (!__all(chain_counters(z) >= (unsigned)ch.nt)) {
        if ((long)__builtin_amdgcn_s_memrealtime() - t0 > CHAIN_WAIT_TICKS) {
          if (lane == 0) __hip_atomic_store(ch.state + 1, (unsigned)MSMD_CONV_CHAIN_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          return false;
        }
        __builtin_amdgcn_s_sleep(8);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return true;
  };

  // LDS-DMA sources: piece i (0, 1) of this wave inside a half-tile is its 1 KB chunk i * 8 + wid = rows 8 chunk .. + 7
  unsigned src[4][2];        // [X0 X1 W0 W1][piece]: byte offsets from A / W (the launcher refuses operands past 4 GB)
  int m0 = 0, n0 = 0;
  // (called twice per tile -- before the epilogue of the previous one for the first K tile, after it for the rest -- from a
  // lane id the compiler cannot match, so that the eight pointers are not kept across the epilogue: with the 128 accumulators
  // and the epilogue's rows live they were the spill)
  auto set_tile = [&](int t) {
    if constexpr (CHAIN) { m0 = cz.rb * 256; n0 = cz.ct * 256; }
    else {
      const int m_tile = (run0 + t) / p.nt, n_tile = (run0 + t) - m_tile * p.nt;
      m0 = m_tile * 256; n0 = n_tile * 256;
    }
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (i * 8 + wid) * 8 + (ln >> 3), phys = ln & 7;
      const int c = phys ^ ((row >> 1) & 7);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        src[h][i] = (unsigned)((a_row_offset(p, min(m0 + h * 128 + row, p.M - 1)) + c * 8) * 2);
        src[2 + h][i] = (unsigned)(((long)min(n0 + h * 128 + row, p.N - 1) * p.ldw + c * 8) * 2);
      }
    }
  };
  const unsigned dma_base = wid * 1024;     // + buffer + half + piece * 8192
  auto stage = [&](int which, int kt, unsigned bufoff) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)((const char*)(which < 2 ? A : W) + (size_t)(src[which][i] + (unsigned)kt * 128u)),
                                       (lds_void_t*)(smem + (dma_base + bufoff + which * HALF + i * 8192)), 16, 0, 0);
  };

  const int fr = lane & 15, fq = lane >> 4;
  const int sw = (fr >> 1) & 7;
  const unsigned ch0 = (fq ^ sw) << 4;
  // fragment addresses (k-step 0 / 1) inside buffer 0; the buffer is toggled by XOR BUF
  unsigned xa0 = (wr * 64 + fr) * 128 + ch0, xa1 = xa0 ^ 64;
  unsigned wa0 = 2 * HALF + (wc * 32 + fr) * 128 + ch0, wa1 = wa0 ^ 64;

  f32x4 acc[2][2][2][4];   // [h][g][i (W fragment)][j (X fragment)]
  u32x4 fx[2][4], fw0[2][2], fw1[2][2];   // [k-step][fragment]
  u32x4 fs0[2], fs1[2];                   // WS: the hi-plane W fragments x 2^11
  auto scale_w = [&](const u32x4 (&fw)[2][2], u32x4 (&fs)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f16x8 h = __builtin_bit_cast(f16x8, fw[0][i]);
      h = h * (f16_t)MSMD_SPLIT_SCALE;
      fs[i] = __builtin_bit_cast(u32x4, h);
    }
  };

  auto read_x = [&](int h) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      fx[0][j] = *(const u32x4*)(smem + xa0 + h * HALF + j * 2048);
      fx[1][j] = *(const u32x4*)(smem + xa1 + h * HALF + j * 2048);
    }
  };
  auto read_w = [&](int g, u32x4 (&fw)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fw[0][i] = *(const u32x4*)(smem + wa0 + g * HALF + i * 2048);
      fw[1][i] = *(const u32x4*)(smem + wa1 + g * HALF + i * 2048);
    }
  };
  auto quadrant = [&](f32x4 (&a)[2][4], const u32x4 (&fw)[2][2], const u32x4 (&fs)[2]) {
    __builtin_amdgcn_s_setprio(1);
    if constexpr (SPLIT == 0) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) Mfma<TI>::run(fw[ks][i], fx[ks][j], a[i][j]);
    } else if constexpr (WS) {
      // one sum in units of 2^-11: Wh.AL, WL.Ah, (2^11 Wh).Ah -- each accumulator is touched every 8th MFMA
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Mfma<TI>::run(fw[0][i], fx[1][j], a[i][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Mfma<TI>::run(fw[1][i], fx[0][j], a[i][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Mfma<TI>::run(fs[i], fx[0][j], a[i][j]);
    } else {
      // [0] = hi planes, [1] = lo planes (x 2^11) of one 32-deep k-step; products in gemm2s_kernel's order (Wh.Al, then Wl.Ah)
      f32x4 t[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { t[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; Mfma<TI>::run(fw[0][i], fx[1][j], t[i][j]); }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Mfma<TI>::run(fw[1][i], fx[0][j], t[i][j]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int e = 0; e < 4; ++e) a[i][j][e] = fmaf(t[i][j][e], MSMD_SPLIT_INV, a[i][j][e]);
          Mfma<TI>::run(fw[0][i], fx[0][j], a[i][j]);
        }
      // issue order: the four FMAs of fold q sit in the shadow of an MFMA issued after the one that finished t[q] (left to
      // itself the scheduler put 17 of the 32 FMAs in one run with the matrix pipe idle behind an s_nop 5)
      __builtin_amdgcn_sched_group_barrier(0x008, 11, 0);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 5, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  };
#define G8_BAR()                        \
  do {                                  \
    __builtin_amdgcn_sched_barrier(0);  \
    __builtin_amdgcn_s_barrier();       \
    __builtin_amdgcn_sched_barrier(0);  \
  } while (0)
#define G8_EBAR()                                      \
  do {                                                 \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    __builtin_amdgcn_s_barrier();                      \
  } while (0)

  // LayerNorm forms: the row statistics of the 32 rows this wave finishes (rows m0 + 64 ps + 8 wid + it) come in by LDS-DMA --
  // no registers across the K loop, and requested a whole K loop before they are read: the producer ran on other XCDs, the
  // first touch misses this L2.  One 16-byte piece = rows (2 rp, 2 rp + 1) of one 64-column slab (slab-major (slabs, M, 2)
  // fp32, M even); lane = 16 so + 4 ps + rp takes slab 4 q + so in piece q; 4 KB per wave behind the operand ring.
  const float* ln_stats = EPI == 2 ? p.a_stats : p.r_stats;
  const int ln_nt = EPI == 2 ? p.a_nt : p.r_nt;
  auto ln_request = [&]() {
    if constexpr (EPI >= 2) {
      if (ln_stats) {
        int ll = lane;
        asm volatile("" : "+v"(ll));
        const int m = min(m0 + ((ll >> 2) & 3) * 64 + wid * 8 + (ll & 3) * 2, p.M - 2);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (4 * q < ln_nt) {
            const int t = min(4 * q + (ll >> 4), ln_nt - 1);
            __builtin_amdgcn_global_load_lds((gbl_void_t*)(ln_stats + ((long)t * p.M + m) * 2),
                                             (lds_void_t*)(smem + (2 * BUF + wid * 4096 + q * 1024)), 16, 0, 0);
          }
        }
      }
    }
  };

  int nk = p.K / (SPLIT ? 32 : 64);       // K tiles of 128 bytes per operand row (CHAIN: of the problem of the tile in the K loop)
  typedef typename Vec4T<TO>::type V4;
  const bool has_r = p.R != nullptr;
  const bool wt = p.flags & GF_WRITE_THROUGH;     // write-through stores (MSMD_GEMM_WRITE_THROUGH): the rows leave the L2 as they are stored

  if constexpr (CHAIN) {
    // the first ticket: claimed, and waited for where it has producers (a grid larger than the first problem), before anything is staged
    if (wid == 0) {
      if (lane == 0) c_claim = __hip_atomic_fetch_add(ch.state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int tk = __builtin_amdgcn_readfirstlane((int)c_claim);
      const bool ok = chain_decode(ch, tk, cz) && chain_wait(cz);
      if (lane == 0) mbox[0] = ok ? tk : -1;
    }
    __syncthreads();
    const int tk = __builtin_amdgcn_readfirstlane(mbox[0]);
    if (tk < 0) return;
    chain_decode(ch, tk, cz);
    c_left = cz.nct - 1;
    chain_problem();
    nk = p.K / 64;
  }
  // prologue of the first tile: K tile 0 whole, K tile 1 except X1 (which phase 1 of tile 0 stages)
  set_tile(tl);
  ln_request();
  stage(2, 0, 0); stage(0, 0, 0); stage(3, 0, 0); stage(1, 0, 0);
  stage(2, 1, BUF); stage(0, 1, BUF); stage(3, 1, BUF);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  while (true) {
    if (wr == 1) __builtin_amdgcn_s_barrier();   // stagger: wave row 1 runs one barrier behind row 0
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[h][g][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned cur = 0;   // byte offset of the buffer of K tile t
    // MODE 0: steady state; 1: K tile nk - 2 (only X1 of the last tile is left to stage); 2: the last K tile
    auto ktile = [&](int t, auto MODE_) {
      constexpr int MODE = decltype(MODE_)::value;
      if constexpr (CHAIN && MODE == 1) {
        // the next ticket: asked for here, three phases ahead of this K tile's vmcnt(0)
        if (wid == 0 && c_left == 0 && lane == 0) c_claim = __hip_atomic_fetch_add(ch.state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      // ---- phase 1
      read_w(0, fw0);
      __builtin_amdgcn_sched_barrier(0);
      read_x(0);
      if (MODE <= 1) stage(1, t + 1, cur ^ BUF);
      asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");   // the four W0 reads (issued first) have returned
      if constexpr (WS) scale_w(fw0, fs0);                 // ... in this wave's read segment, the other wave row is multiplying
      G8_BAR();
      quadrant(acc[0][0], fw0, fs0);
      G8_BAR();
      // ---- phase 2
      read_w(1, fw1);
      if (MODE == 0) stage(2, t + 2, cur);
      if constexpr (WS) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        scale_w(fw1, fs1);
      }
      G8_BAR();
      quadrant(acc[0][1], fw1, fs1);
      G8_BAR();
      // ---- phase 3
      read_x(1);
      if (MODE == 0) stage(0, t + 2, cur);
      G8_BAR();
      quadrant(acc[1][1], fw1, fs1);
      G8_BAR();
      // ---- phase 4
      if (MODE == 0) stage(3, t + 2, cur);
      if (MODE == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // all but the three youngest half-tiles: tile t + 1 is in
      if (MODE == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if constexpr (CHAIN && MODE == 1) {
        // the ticket is in: wave 0 posts it and asks for the counters of its producer row blocks, which the last K tile covers
        if (wid == 0 && c_left == 0) {
          const int tk = __builtin_amdgcn_readfirstlane((int)c_claim);
          ChainTile nz;
          const bool ok = chain_decode(ch, tk, nz);
          c_cnt = ok ? chain_counters(nz) : ~0u;
          if (lane == 0) mbox[0] = ok ? tk : -1;
        }
      }
      G8_BAR();
      quadrant(acc[1][0], fw0, fs0);
      G8_BAR();
      cur ^= BUF; xa0 ^= BUF; xa1 ^= BUF; wa0 ^= BUF; wa1 ^= BUF;
    };
    for (int t = 0; t < nk - 2; ++t) ktile(t, std::integral_constant<int, 0>{});
    ktile(nk - 2, std::integral_constant<int, 1>{});
    ktile(nk - 1, std::integral_constant<int, 2>{});
    if constexpr (CHAIN) {
      // producers done already (the usual case: they ran rounds ago)?  Then the acquire goes here, drained ahead of the barrier
      // below, behind which every wave may load the next tile's A rows.  A first-problem or absent tile has no counters (~0).
      if (wid == 0 && c_left == 0) {
        const bool ready = __all(c_cnt >= (unsigned)ch.nt);
        if (ready && __builtin_amdgcn_readfirstlane((int)c_cnt) != -1) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (lane == 0) mbox[1] = ready;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();   // row 0 pays back the stagger: every wave has read its last fragments
    if (nk & 1) { xa0 ^= BUF; xa1 ^= BUF; wa0 ^= BUF; wa1 ^= BUF; }   // the next tile starts in buffer 0 again

    // ---- epilogue through LDS, in the upper half of the ring (the lower half already takes the next tile's first K tile).
    // Pass ps = 2 h + wr' covers tile rows 64 ps .. 64 ps + 63: the four waves of wave row wr' write their two quadrants of
    // half h as fp32 (16-byte chunk c of row r at r * 1024 + ((c ^ (r & 15)) << 4): conflict-free for the fragment writes and
    // the row reads), then wave w finishes rows 8 w .. 8 w + 7 of the block.
    const int em0 = m0, en0 = n0;                    // this tile (m0 / n0 move on to the next one below)
    // CHAIN: p moves on to the next tile's problem below as well: the epilogue's own copies, whether this tile has consumers in the
    // launch (e_pub: then its row block's counter e_cnt), and how it stores (consumed rows in the form the table names; the last
    // problem's write-through, as launch_gemm8 stores a launch that ends in one burst)
    const int eM = p.M;
    void* const eC = p.C;
    const float* const ebias = p.bias;
    bool e_pub = false, ewt = wt;
    unsigned* e_cnt = nullptr;
    if constexpr (CHAIN) {
      e_pub = cz.l + 1 < ch.n;
      ewt = e_pub ? !ch.release : true;
      e_cnt = ch.state + CHAIN_STATE_HEAD + ch.pr[cz.l].cnt0 + cz.rb;
    }
    // everything the epilogue derives from the lane id comes from a copy the compiler cannot match with the K loop's: hoisted
    // out of the tile loop those values lived across the K loop and pushed its staging pointers into scratch
    int el = lane;
    asm volatile("" : "+v"(el));
    const int efr = el & 15, efq = el >> 4;
    const int ncol = en0 + el * 4;                   // this lane's four columns in every row it finishes
    f32x4 cbias = f32x4{0.f, 0.f, 0.f, 0.f}, cx = f32x4{1.f, 1.f, 1.f, 1.f}, cy = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ebias) cbias = *(const f32x4*)(ebias + ncol);
    if constexpr (EPI == 2) cx = *(const f32x4*)(p.w_colsum + ncol);
    if constexpr (EPI == 3) {
      if (p.r_stats) { cx = *(const f32x4*)(p.r_gamma + ncol); cy = *(const f32x4*)(p.r_beta + ncol); }
    }
    float mu_l = 0.f, rs_l = 1.f;                    // of row (lane & 31) of this wave's 32
    if constexpr (EPI >= 2) {
      if (ln_stats) {
        // ln_finish's association (the 128 x 128 kernels: lane group f holds slabs f, f + 4, f + 8, f + 12 and the tail
        // 16 + f, 20 + f, ...; groups combine as (0 + 1) + (2 + 3)), so that a row's moments are the same bits whichever kernel
        // its launch was routed to.  Both halves of the wave compute the same 32 rows.
        const int r32 = el & 31;
        const unsigned base = 2 * BUF + wid * 4096 + (((r32 >> 3) * 4 + ((r32 & 7) >> 1)) << 4) + ((r32 & 1) << 3);
        float Sf[4], Qf[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          f32x2 w[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int t = f + 4 * q;
            w[q] = *(const f32x2*)(smem + base + (t >> 2) * 1024 + ((t & 3) << 8));
            if (t >= ln_nt) w[q] = f32x2{0.f, 0.f};
          }
          Sf[f] = (w[0][0] + w[1][0]) + (w[2][0] + w[3][0]);
          Qf[f] = (w[0][1] + w[1][1]) + (w[2][1] + w[3][1]);
        }
        if (ln_nt > 16) {             // more than 16 slabs per row: the rest from memory, serially
          const f32x2* rp = (const f32x2*)ln_stats + min(em0 + (r32 >> 3) * 64 + wid * 8 + (r32 & 7), p.M - 1);
#pragma unroll
          for (int f = 0; f < 4; ++f)
            for (int t = 16 + f; t < ln_nt; t += 4) { const f32x2 w = rp[(long)t * p.M]; Sf[f] += w[0]; Qf[f] += w[1]; }
        }
        const float S = (Sf[0] + Sf[1]) + (Sf[2] + Sf[3]), Q = (Qf[0] + Qf[1]) + (Qf[2] + Qf[3]);
        const float inv_cols = 1.0f / (float)(EPI == 2 ? p.K : p.N);
        mu_l = S * inv_cols;
        rs_l = rsqrtf(fmaxf(Q * inv_cols - mu_l * mu_l, 0.f) + p.ln_eps);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's statistics are in registers: its 4 KB may be refilled
      }
    }
    // the next tile of this workgroup: its first K tile goes out now and lands under the epilogue
    bool more, ready = true;
    if constexpr (CHAIN) {
      // the rest of a row-block ticket reads the rows this workgroup has acquired already; else what wave 0 posted
      if (c_left > 0) { --c_left; ++cz.ct; more = true; }
      else {
        const int tk = __builtin_amdgcn_readfirstlane(mbox[0]);
        ready = __builtin_amdgcn_readfirstlane(mbox[1]) != 0;
        more = tk >= 0;
        if (more) {
          chain_decode(ch, tk, cz);
          c_left = cz.nct - 1;
          chain_problem();
          nk = p.K / 64;
        }
      }
    } else {
      tl += stride;
      more = tl < run_n;
    }
    if (more) {
      set_tile(tl);
      // (CHAIN, producers not done: W, which nobody writes in the launch, goes out now; A behind the wait below)
      stage(2, 0, 0); if (ready) stage(0, 0, 0);
      stage(3, 0, 0); if (ready) stage(1, 0, 0);
      ln_request();
    }
    auto write_block = [&](const f32x4 (&q0)[2][4], const f32x4 (&q1)[2][4]) {
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = j * 16 + efr, c = g * 32 + wc * 8 + i * 4 + efq;
            *(f32x4*)(smem + BUF + row * 1024 + ((c ^ efr) << 4)) = g == 0 ? q0[i][j] : q1[i][j];
          }
    };
    auto finish_block = [&](int ps) {
      if constexpr ((SPLIT & 3) == 2) {
        // fp32 C / residual: a lane's four columns are 16 bytes, a row is one 1 KB run
        f32x4 rr[8];
        if (has_r) {
#pragma unroll
          for (int it = 0; it < 8; ++it) {
            const int m = min(em0 + ps * 64 + wid * 8 + it, eM - 1);
            rr[it] = *(const f32x4*)((const float*)p.R + (long)m * p.ldr + ncol);
          }
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int row = wid * 8 + it, m = em0 + ps * 64 + row;
          const f32x4 a = *(const f32x4*)(smem + BUF + row * 1024 + ((el ^ (row & 15)) << 4));
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = act_out_c<float, ACTK>(WS ? fmaf(a[e], MSMD_SPLIT_INV, cbias[e]) : a[e] + cbias[e], p.act);   // gemm2s_kernel's fp32 epilogue
            if (has_r) o[e] += rr[it][e];
          }
          if (m < eM) {
            if (ewt) store16_wt((float*)eC + (long)m * p.ldc + ncol, __builtin_bit_cast(u32x4, o));
            else *(f32x4*)((float*)eC + (long)m * p.ldc + ncol) = o;
          }
        }
      } else if constexpr ((SPLIT & 3) == 1) {
        // split C / residual rows ([hi x 32 | lo x 32] blocks, 2 ldc / 2 ldr fp16 per row).  Lanes 2 q and 2 q + 1 own the
        // eight logical columns 8 q .. 8 q + 7 of a row between them: the even lane moves their hi plane (16 bytes), the odd
        // lane their lo plane (the 16 bytes 64 further), the two exchange halves by DPP -- every wave instruction reads or
        // writes one whole 1 KB row piece instead of 8-byte pieces in 64-byte runs.
        const bool odd = el & 1;
        const long coff = 2L * en0 + ((el >> 3) << 6) + (((el >> 1) & 3) << 3) + (odd ? 32 : 0);
        auto swap1 = [](unsigned x) { return (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false); };   // quad_perm [1, 0, 3, 2]
        u32x4 rr[8];
        if (has_r) {
#pragma unroll
          for (int it = 0; it < 8; ++it) {
            const int m = min(em0 + ps * 64 + wid * 8 + it, eM - 1);
            rr[it] = *(const u32x4*)((const f16_t*)p.R + (long)m * 2 * p.ldr + coff);
          }
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int row = wid * 8 + it, m = em0 + ps * 64 + row;
          const f32x4 a = *(const f32x4*)(smem + BUF + row * 1024 + ((el ^ (row & 15)) << 4));
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = act_split<ACTK>(WS ? fmaf(a[e], MSMD_SPLIT_INV, cbias[e]) : a[e] + cbias[e], p.act);
          if (has_r) {
            // even lane holds [h own | h partner], odd lane [l partner | l own]
            const unsigned g0 = swap1(odd ? rr[it][0] : rr[it][2]), g1 = swap1(odd ? rr[it][1] : rr[it][3]);
            const f16x2 h01 = __builtin_bit_cast(f16x2, odd ? g0 : rr[it][0]), h23 = __builtin_bit_cast(f16x2, odd ? g1 : rr[it][1]);
            const f16x2 l01 = __builtin_bit_cast(f16x2, odd ? rr[it][2] : g0), l23 = __builtin_bit_cast(f16x2, odd ? rr[it][3] : g1);
            v[0] += unsplit_f16x2(h01[0], l01[0]); v[1] += unsplit_f16x2(h01[1], l01[1]);
            v[2] += unsplit_f16x2(h23[0], l23[0]); v[3] += unsplit_f16x2(h23[1], l23[1]);
          }
          f16_t h[4], l[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) split_f16x2(v[e], h[e], l[e]);
          const unsigned hp0 = __builtin_bit_cast(unsigned, f16x2{h[0], h[1]}), hp1 = __builtin_bit_cast(unsigned, f16x2{h[2], h[3]});
          const unsigned lp0 = __builtin_bit_cast(unsigned, f16x2{l[0], l[1]}), lp1 = __builtin_bit_cast(unsigned, f16x2{l[2], l[3]});
          const unsigned g0 = swap1(odd ? hp0 : lp0), g1 = swap1(odd ? hp1 : lp1);
          const u32x4 o = odd ? u32x4{g0, g1, lp0, lp1} : u32x4{hp0, hp1, g0, g1};
          if (m < eM) {
            if (ewt) store16_wt((f16_t*)eC + (long)m * 2 * p.ldc + coff, o);
            else *(u32x4*)((f16_t*)eC + (long)m * 2 * p.ldc + coff) = o;
          }
        }
      } else {
      // residual rows first: eight 512-byte runs per wave, in flight while the block is read back
      V4 rr[8];
      if (EPI != 2 && has_r) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int m = min(em0 + ps * 64 + wid * 8 + it, eM - 1);
          rr[it] = *(const V4*)((const TO*)p.R + (long)m * p.ldr + ncol);
        }
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int row = wid * 8 + it, m = em0 + ps * 64 + row;
        const f32x4 a = *(const f32x4*)(smem + BUF + row * 1024 + ((el ^ (row & 15)) << 4));
        float mu = 0.f, rs = 1.f;
        if constexpr (EPI >= 2) {
          mu = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mu_l), ps * 8 + it));
          rs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rs_l), ps * 8 + it));
        }
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float x = a[e];
          if constexpr (EPI == 2) x = rs * (x - mu * cx[e]);
          v[e] = act_out_c<TO, ACTK>(x + cbias[e], p.act);
          if constexpr (EPI == 3) v[e] += fmaf(((float)rr[it][e] - mu) * rs, cx[e], cy[e]);
          else if (has_r) v[e] += (float)rr[it][e];
        }
        const V4 o = pack4<TO>(v[0], v[1], v[2], v[3]);
        if (m < eM) {
          if (ewt) store8_wt((TO*)eC + (long)m * p.ldc + ncol, __builtin_bit_cast(u32x2, o));
          else *(V4*)((TO*)eC + (long)m * p.ldc + ncol) = o;
        }
        if constexpr (EPI == 3) {
          if (p.stats_out) {      // sums of what the consumer will read, per 64-column slab = 16 lanes
            float S = 0.f, Q = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float w = (float)o[e]; S += w; Q = fmaf(w, w, Q); }
            // the association of gemm_epilogue_ln: a lane's four columns are fragment i = lane bits 2-3, lane group fq = bits 0-1
#pragma unroll
            for (int d : {4, 8, 1, 2}) { S += __shfl_xor(S, d, 64); Q += __shfl_xor(Q, d, 64); }
            if ((el & 15) == 0 && m < p.M) *(f32x2*)(p.stats_out + ((long)((en0 >> 6) + (el >> 4)) * p.M + m) * 2) = f32x2{S, Q};
          }
        }
      }
      }
    };
    if (wr == 0) write_block(acc[0][0], acc[0][1]);
    G8_EBAR();
    finish_block(0);
    G8_EBAR();
    if (wr == 1) write_block(acc[0][0], acc[0][1]);
    G8_EBAR();
    finish_block(1);
    G8_EBAR();
    if (wr == 0) write_block(acc[1][0], acc[1][1]);
    G8_EBAR();
    finish_block(2);
    G8_EBAR();
    if (wr == 1) write_block(acc[1][0], acc[1][1]);
    G8_EBAR();
    finish_block(3);
    if constexpr (CHAIN) {
      if (e_pub) {
        // hand the tile over: every storing wave drains its stores, the workgroup meets, ONE lane signals (plain stores: behind one
        // agent-scope release, its own wait written out -- cdna_hip_programming.md Guideline 16, Pitfall 12)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        G8_EBAR();
        if (tid == 0) {
          if (ch.release) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
          __hip_atomic_fetch_add(e_cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (!more) break;
      if (!e_pub) G8_EBAR();
      if (!ready) {
        // the producers of the next tile were not done when its ticket came in: wave 0 waits for them (bounded), acquires, and only
        // behind the barrier do the A rows of its first K tile go out
        if (wid == 0) {
          const bool ok = chain_wait(cz);
          if (lane == 0) mbox[2] = ok;
        }
        __syncthreads();
        if (!__builtin_amdgcn_readfirstlane(mbox[2])) {      // a wait expired: no more tickets, a normal return
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          break;
        }
        set_tile(tl);
        stage(0, 0, 0); stage(1, 0, 0);
      }
    } else {
      if (!more) break;
      // the upper half of the ring is free again once every wave has read its rows of the last block; the first K tile has
      // been in flight since before the epilogue: K tile 1 except X1 follows, and the loop's own counted waits take over
      G8_EBAR();
    }
    set_tile(tl);
    stage(2, 1, BUF); stage(0, 1, BUF); stage(3, 1, BUF);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
#undef G8_BAR
#undef G8_EBAR
}

template <typename TI, int EPIA, int SPLIT = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm8_kernel(const GemmArgs p) {
  gemm8_body<TI, EPIA, SPLIT>(p, NoChain{});
}
// p: what the problems share (N, ldc, act); the rest of it follows the table's problem of the tile at hand
template <typename TI, int EPIA>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm8_chain_kernel(const GemmArgs p0, const ChainTable ch) {
  GemmArgs p = p0;
  gemm8_body<TI, EPIA, 0>(p, ch);
}

// f(std::integral_constant<int, C>) for the C of the compile-time list that equals the run-time `code`: its result (a launcher's:
// >= 0), or -1 for a code that is not in the list.  Every run-time choice of a kernel's integer template arguments goes through here.
template <int... CODES, typename F>
static int dispatch_code(int code, F&& f) {
  int r = -1;
  (void)((code == CODES && ((r = f(std::integral_constant<int, CODES>{})), true)) || ...);
  return r;
}

// Launches KFN on the current device and returns the last error.  More than 64 KB of dynamic LDS has to be allowed per kernel
// and per DEVICE (hipFuncSetAttribute acts on the current one): once for each, remembered in a bit per device ordinal.
template <auto KFN, typename... ARGS>
static int gemm_launch_kernel(dim3 grid, int threads, int lds, hipStream_t st, const ARGS&... p) {
  if (lds > 0) {
    static std::atomic<unsigned long> allowed{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long bit = (unsigned)dev < 64 ? 1UL << dev : 0;      // ordinals past 63: allowed again at every launch
    if (!(allowed.load(std::memory_order_relaxed) & bit)) {
      (void)hipFuncSetAttribute((const void*)KFN, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      allowed.fetch_or(bit, std::memory_order_relaxed);
    }
  }
  hipLaunchKernelGGL(KFN, grid, dim3(threads), lds, st, p...);
  MSMD_RETURN_LAST();
}

// XCD grid over BM x BN tiles: sets p.mt / p.nt / p.xn and returns the workgroup count, padded to whole XCD blocks.  With all 8 XCDs
// striped along M every L2 streams its own copy of the whole weight matrix from HBM, while the activation rows (the previous
// kernel's output) are still warm: an XCD of an (8 / xn) x xn grid reads 1 / xn of W and xn / 8 of A, so xn is picked per problem
// from  0.7 xn |A| + (8 / xn) |W|  (the 0.7 fitted on the qkv shape, where 2 x 4 ties with 8 x 1 and both trail 4 x 2).  Forward
// step, same-graph A/B in both orders: 8 x 1 4.96 ms, 4 x 2 everywhere 4.89, this rule 4.88.
// `lda` is A's row stride in LOGICAL elements, like p.K (the split-pair kernels pass p.lda / 2).  Bytes are counted at 2 per
// element for every kernel: the split pairs' 4 scale both terms by the same power of two, which no comparison below sees.
static int gemm2_xcd_grid(GemmArgs& p, int BM, int BN, long lda) {
  p.mt = (p.M + BM - 1) / BM; p.nt = (p.N + BN - 1) / BN;
  const double a_bytes = 2.0 * p.M * (double)(p.rows_per_batch < p.M ? lda : p.K), w_bytes = 2.0 * p.N * (double)p.K;
  double best = 1e30;
  int want_xn = 1;
  for (int xn = 1; xn <= 4; xn *= 2) {
    const double c = 0.7 * xn * a_bytes + (8.0 / xn) * w_bytes;
    if (c < best && p.nt >= xn) { best = c; want_xn = xn; }
  }
  p.xn = p.nt >= want_xn ? want_xn : 1;
  const int xm_n = 8 / p.xn;
  return ((p.mt + xm_n - 1) / xm_n) * ((p.nt + p.xn - 1) / p.xn) * 8;
}

// The XCD grid of the 160 x 128 member of variant 17, which is meant to run ONE round of one workgroup per CU: gemm2_xcd_grid's own xn
// where its grid, padding included, stays within 256 workgroups (the chip the rule was fitted on), else the first xn whose grid does.
// Returns that grid's workgroup count, or 0 where none fits (p then holds gemm2_xcd_grid's grid).  6400 x 768: 40 x 6 tiles, 240 workgroups.
static int gemm160_one_round_grid(GemmArgs& p) {
  const int wgs = gemm2_xcd_grid(p, 160, 128, p.lda);
  if (wgs <= 256) return wgs;
  for (int xn = 1; xn <= 4 && xn <= p.nt; xn *= 2) {
    const int xm_n = 8 / xn;
    const int w = ((p.mt + xm_n - 1) / xm_n) * ((p.nt + xn - 1) / xn) * 8;
    if (w <= 256) { p.xn = xn; return w; }
  }
  return 0;
}

// gemm2_kernel on `wgs` workgroups per batch (gemm2_xcd_grid's)
template <typename TO, int BM, int BN, int WM, int WN, int NSTAGE, bool PIPE = false, typename TI = bf16_t, int EPIA = 0>
static int launch_gemm2(GemmArgs& p, int wgs, int batch, hipStream_t st) {
  constexpr int lds = NSTAGE * (BM + BN) * 128;
  // stagger: only where the launch runs more than one round of two workgroups per CU
  p.stagger_ticks = ((p.flags & GF_STAGGER) && batch == 1 && lds <= 80 * 1024 && (long)p.mt * p.nt > 640)
                        ? (int)(100.0 * 0.5 * ((p.K / 64) * 0.5 + 3.0)) : 0;
  return gemm_launch_kernel<gemm2_kernel<TO, BM, BN, WM, WN, NSTAGE, PIPE, TI, EPIA>>(dim3(wgs, 1, batch), WM * WN * 64, lds, st, p);
}

// The EPIA code of a call: its epilogue family (lnk: the tile has the LayerNorm forms) and the activation where it is a constant
// of the kernel (none / GELU: what the path launches; ELU and the LayerNorm-residual form with an activation stay run-time).
static int gemm_epia(const GemmArgs& p, bool lnk) {
  GemmEpi e = EPI_ALL;      // training calls: pre-activation copy / dropout / activation backward
  if (lnk && p.a_stats) e = EPI_LN_OPERAND;
  else if (lnk && (p.r_stats || p.stats_out)) e = EPI_LN_RESIDUAL;
  else if (!p.a_stats && !p.r_stats && !p.stats_out && !p.Z && !(p.p_drop > 0.f) && !(p.flags & GF_ACT_BWD)) e = EPI_PLAIN;
  return epia(e, p.act == MSMD_ACT_NONE ? MSMD_ACT_NONE : (p.act == MSMD_ACT_GELU && e != EPI_LN_RESIDUAL) ? MSMD_ACT_GELU : ACT_RUNTIME);
}

// One instantiation per epilogue family and compiled-in activation, picked per call (see gemm2_kernel's EPI).
template <typename TO, int BM, int BN, int WM, int WN, int NSTAGE, bool PIPE = false, typename TI = bf16_t>
static int launch_gemm2_epi(GemmArgs& p, int batch, hipStream_t st) {
  constexpr bool LNK = (BN == 128 || BN == 64) && WN == 2 && (BM / WM / 16 == 2 || BM / WM / 16 == 3) && sizeof(TO) == 2;
  const int code = gemm_epia(p, LNK), wgs = gemm2_xcd_grid(p, BM, BN, p.lda);
  int r;
  if constexpr (LNK && PIPE && NSTAGE == 2 && WM * WN == 8 && BN == 128 && BM == 128) {
    // gemm_ln_plan's choice (GF_ROWS_160: residual form, no activation, one batch): the 160 x 128 member, 10 waves of this tile's 32 x 64
    // wave tile on a 4-stage ring, one workgroup per CU.  Same k order, MFMA sequence and epilogue: the same bits.  Its one epilogue
    // serves the form with and without statistics on either side.
    if (p.flags & GF_ROWS_160) {
      int wgs160 = gemm160_one_round_grid(p);
      if (!wgs160) wgs160 = gemm2_xcd_grid(p, 160, 128, p.lda);      // forced onto a grid of more than one round
      return launch_gemm2<TO, 160, 128, 5, 2, 4, true, TI, epia(EPI_LN_RESIDUAL, MSMD_ACT_NONE)>(p, wgs160, batch, st);
    }
    // more than one round of two workgroups per CU: the persistent form (gemm2p_kernel: 512 workgroups, two per CU); GF_ONE_TILE =
    // the caller opts out (A/B).  The 128 x 128 tile's plain and LayerNorm-operand epilogues: the LayerNorm-residual one (its
    // launches on the path are single-round) and the 192-row tile do not fit 128 registers in this form (20-128 bytes of scratch).
    if (batch == 1 && wgs > 512 && !(p.flags & GF_ONE_TILE)) {
      auto persistent = [&](auto c) { return gemm_launch_kernel<gemm2p_kernel<TO, BM, BN, WM, WN, TI, decltype(c)::value>>(dim3(512), WM * WN * 64, 2 * (BM + BN) * 128, st, p); };
      if ((r = dispatch_code<11, 21, 12, 22>(code, persistent)) >= 0) return r;
    }
  }
  auto run = [&](auto c) { return launch_gemm2<TO, BM, BN, WM, WN, NSTAGE, PIPE, TI, decltype(c)::value>(p, wgs, batch, st); };
  if constexpr (LNK) {
    if ((r = dispatch_code<2, 12, 22, 3, 13>(code, run)) >= 0) return r;
  }
  if ((r = dispatch_code<1, 11, 21>(code, run)) >= 0) return r;
  if constexpr (__is_same(TI, bf16_t)) {     // the everything-epilogue is the training step's: bf16 only
    if ((r = dispatch_code<10, 20>(code, run)) >= 0) return r;
  }
  return run(std::integral_constant<int, 0>{});
}

// One persistent workgroup per CU: the grid cap is the CURRENT device's CU count (256 on MI355X; the tile-run logic of the kernel
// works for any workgroup count, the shape rules below are fitted on 256).
static int gemm8_workgroup_cap() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  return n;
}

// element offset of A's last row, plain or windowed
static long gemm_last_row_offset(const GemmArgs& p) {
  return p.rows_per_batch < p.M ? ((long)((p.M - 1) / p.rows_per_batch) * p.a_batch_stride + (long)(p.rows_per_batch - 1) * p.lda) : (long)(p.M - 1) * p.lda;
}

// gemm8_kernel: which calls it takes ...
static bool gemm8_takes(const GemmArgs& p, int batch, int osz) {
  if (osz != 2 || batch != 1 || p.batch_inner != 1 || (p.N % 256) || (p.K % 64) || p.K < 128 || !p.vec_ok) return false;
  if (p.Z || p.p_drop > 0.f || (p.flags & GF_ACT_BWD)) return false;               // inference epilogues only
  if (((uintptr_t)p.bias & 15) || ((uintptr_t)p.C & 7) || ((uintptr_t)p.R & 7)) return false;
  if ((gemm_last_row_offset(p) + p.K) * 2 >= (1L << 32) || ((long)(p.N - 1) * p.ldw + p.K) * 2 >= (1L << 32)) return false;   // 32-bit staging offsets from A / W
  const GemmEpi epi = epia_family(gemm_epia(p, true));
  if ((p.a_stats || p.r_stats) && ((p.M & 1) || ((uintptr_t)p.a_stats & 15) || ((uintptr_t)p.r_stats & 15))) return false;   // row pairs by 16-byte LDS-DMA
  if (epi == EPI_LN_OPERAND && (p.R || !p.bias || !p.w_colsum)) return false;
  if (epi == EPI_LN_RESIDUAL && (!p.R || !p.bias || p.act != MSMD_ACT_NONE)) return false;
  return p.act == MSMD_ACT_NONE || p.act == MSMD_ACT_GELU;
}

// ... and which of those it wins (hot, isolated, tools/bench_gemm_variants.py SHAPES=guide|conv|sampler|encoder; us for the
// 128 x 128 / 192 x 128 kernels -> this one): the launch must fill its last round of 256 one-per-CU workgroups and, with a short K
// (12 K tiles or fewer: 13 us of prologue + epilogue per round against 1.4 us per K tile), nearly completely.
//   wins   conv1-4 (204768 ... 25568 x 512 x 1536: 375 -> 323, 198 -> 186, 92 -> 85, 52 -> 44), 6400 x 2304 x 768 (33 -> 29.4),
//          21312 x 1536 x 512 (50 -> 47), 12800 x 2304 x 768 (59 -> 57), HuBERT-large 15968 x {3072, 1024, 4096} x 1024 (114 -> 109,
//          43 -> 37, 153 -> 143) and 15968 x 1024 x 4096 (133 -> 103), 16384 x 4096 x 3072 (364 -> 311 = 1 326 TFLOP/s)
//   loses  under-filled rounds: 6400 x 768 x {768, 3072} (75 tiles), 6400 x 3072 x 768 (300: 40 -> 52), 12800 x 3072 x 768 (600: 80 -> 86),
//          21312 x 512 x {512, 2048} (168: 22.6 -> 26, 49 -> 51), 21312 x 2048 x 512 (672 = 2.6 rounds, K = 512: 67 -> 69)
static bool gemm8_wins(int M, int N, int K) {
  const long tiles = (long)((M + 255) / 256) * (N / 256);
  if (tiles < 192) return false;
  const double fill = (double)tiles / (256.0 * (double)((tiles + 255) / 256));
  return fill >= 0.75 && (K >= 1024 || fill >= 0.878);
}

// gemm8_kernel, 16-bit or split-pair (KFN, its LDS bytes): one workgroup per 256 x 256 tile up to the CU count
constexpr int GEMM8_RING = 2 * 4 * 128 * 128;      // 128 KB operand ring (its upper half = the epilogue's row block)
template <auto KFN, int LDS>
static int launch_gemm8(GemmArgs& p, hipStream_t st) {
  p.mt = (p.M + 255) / 256; p.nt = p.N / 256;
  const int tiles = p.mt * p.nt, cap = gemm8_workgroup_cap();
  // Up to two rounds the launch ends in one burst of output rows: with write-through stores they leave the L2s while the
  // epilogue is still running instead of at the end-of-kernel write-back (6400 x 2304 x 768: 30.3-31.2 -> 28.1-29.3 us, 21312 x
  // 1536 x 512: 50.4 -> 47.3; many-round launches are indifferent or lose: 15968 x 3072 x 1024 101 -> 110)
  if (tiles <= 512) p.flags |= GF_WRITE_THROUGH;
  return gemm_launch_kernel<KFN>(dim3(tiles < cap ? tiles : cap), 512, LDS, st, p);
}

// gemm8_kernel on split-pair operands (SPLIT): the calls it takes, the rule, the launch.  p carries fp16 strides for A / W
// (doubled by gemm_args) and logical ldc / ldr.
static bool gemm8s_takes(const GemmArgs& p, int batch, bool split_out) {
  if (batch != 1 || p.batch_inner != 1 || (p.N % 256) || (p.K % 32) || p.K < 64 || !p.vec_ok) return false;
  if (((uintptr_t)p.bias & 15) || ((uintptr_t)p.C & 15) || ((uintptr_t)p.R & 15)) return false;
  if (split_out ? ((p.ldc % 32) || (p.R && (p.ldr % 32))) : ((p.ldc % 4) || (p.R && (p.ldr % 4)))) return false;
  if ((gemm_last_row_offset(p) + 2L * p.K) * 2 >= (1L << 32) || ((long)(p.N - 1) * p.ldw + 2L * p.K) * 2 >= (1L << 32)) return false;   // 32-bit staging offsets
  return p.act == MSMD_ACT_NONE || p.act == MSMD_ACT_GELU;
}
// ... and which of those it wins (tools/bench_gemm_split.py, us, 128 x 128 gemm2s_kernel -> this kernel folding -> fold-free with
// MSMD_GEMM_W_BELOW_32; fp32 output, GELU).  Three MFMAs per fragment pair on the same staged bytes: a K tile (32 logical k)
// takes 1.5 x the 16-bit kernel's (64 k) while prologue / epilogue cost per round is the same, so under-filled rounds cost
// relatively less than gemm8_wins() charges them.
//   conv1-4 204768 ... 25568 x 512 x 1536 (1 600 ... 200 tiles): 951 -> 870 -> 791, 481 -> 482 -> 438, 254 -> 240 -> 214, 133 -> 114 -> 100
//   6400 x 2304 x 768 (225): 78 -> 76 -> 66;  21312 x 1536 x 512 (504): 118 -> 110 -> 101;  21312 x 2048 x 512 (672): 158 -> 153 -> 139
//   21312 x 512 x 2048 (168, fill 0.66): 135 -> 141 -> 120;  21312 x 512 x 512 (168): 47.9 -> 48.8 -> 44.0
//   loses: 6400 x 3072 x 768 (300, fill 0.59): 100 -> 125 -> 114;  75-100 tiles: 6400 x 768 x {768, 3072} 38 -> 58 -> 52, 114 -> 171 -> 148,
//          12768 x 512 x 1024 49 -> 73 -> 64
static bool gemm8s_wins(int M, int N, int K, bool w_below_32) {
  const long tiles = (long)((M + 255) / 256) * (N / 256);
  if (tiles < 160) return false;
  const double fill = (double)tiles / (256.0 * (double)((tiles + 255) / 256));
  return fill >= (w_below_32 ? 0.65 : 0.75);
}

// gemm2s_kernel: the W-below-32 form and, on the routed tiles, the activation are constants of the kernel
template <typename TO, int BM, int BN, int WM, int WN, int NSTAGE>
static int launch_gemm2s(GemmArgs& p, int batch, hipStream_t st) {
  constexpr int lds = NSTAGE * (BM + BN) * 128;
  const dim3 grid(gemm2_xcd_grid(p, BM, BN, p.lda / 2), 1, batch);      // p.lda is the fp16 stride (doubled by gemm_args)
  return dispatch_code<0, 1>((p.flags & GF_W_BELOW_32) != 0, [&](auto ws) {
    auto run = [&](auto act) {
      return gemm_launch_kernel<gemm2s_kernel<TO, BM, BN, WM, WN, NSTAGE, decltype(act)::value, decltype(ws)::value != 0>>(grid, WM * WN * 64, lds, st, p);
    };
    int r = -1;
    if constexpr (lds <= 80 * 1024) r = dispatch_code<MSMD_ACT_NONE, MSMD_ACT_GELU>(p.act, run);
    return r >= 0 ? r : run(std::integral_constant<int, ACT_RUNTIME>{});
  });
}

template <typename TO>
static int dispatch_gemm2s(GemmArgs& p, int batch, hipStream_t st, int variant) {
  switch (variant) {
    case GV_SPLIT_128: return launch_gemm2s<TO, 128, 128, 4, 2, 2>(p, batch, st);
    case GV_SPLIT_64: return launch_gemm2s<TO, 64, 64, 2, 2, 4>(p, batch, st);
    case GV_256x64: return launch_gemm2s<TO, 256, 64, 8, 1, 2>(p, batch, st);
    case GV_256:      // gemm8_kernel's SPLIT forms: 1 / 2 = split / fp32 output, + 4 with MSMD_GEMM_W_BELOW_32
      if (!gemm8s_takes(p, batch, sizeof(TO) == 2)) return -1;
      return dispatch_code<11, 21>(epia(EPI_PLAIN, p.act), [&](auto c) {
        return dispatch_code<0, 1>((p.flags & GF_W_BELOW_32) != 0, [&](auto ws) {
          return launch_gemm8<gemm8_kernel<f16_t, decltype(c)::value, (sizeof(TO) == 4 ? 2 : 1) + 4 * decltype(ws)::value>, GEMM8_RING>(p, st);
        });
      });
    default: return -1;
  }
}

template <typename T, typename TO>
static int launch_gemm(GemmArgs& p, int batch, hipStream_t st) {
  // Small-N / small-M problems use the 64x64 tile (less padding waste, more workgroups).
  const bool small = (p.N <= 64) || ((long)((p.M + 127) / 128) * ((p.N + 127) / 128) * batch < 128);
  const int B = small ? 64 : 128;
  p.mt = (p.M + B - 1) / B; p.nt = (p.N + B - 1) / B;
  const dim3 grid(((p.mt + 7) / 8) * 8 * p.nt, 1, batch);
  return small ? gemm_launch_kernel<gemm_kernel<T, TO, 64, 64>>(grid, 256, 0, st, p)
               : gemm_launch_kernel<gemm_kernel<T, TO, 128, 128>>(grid, 256, 0, st, p);
}

// Every other family that was built and measured lost and was removed: its numbers are in DESIGN.md section 5 / 5b.
// The LDS-DMA variants dispatch_gemm has for bf16 / fp16 operands; gemm16_route asks the same question, so a routed variant always launches.
static constexpr bool gemm2_has(int variant, bool bf16) {
  if (variant == GV_128_AB || variant == GV_128_ONE_AB) return bf16;
  return variant == GV_64_DEEP || variant == GV_64 || variant == GV_256x64 || variant == GV_192 || variant == GV_128 || variant == GV_64x128 || variant == GV_256;
}

// The launcher of a variant for plain (not split-pair) operands TI and output TO
template <typename TO, typename TI>
static int dispatch_gemm(GemmArgs& p, int batch, hipStream_t st, int variant) {
  if (variant == GV_GENERIC) return launch_gemm<TI, TO>(p, batch, st);
  if constexpr (sizeof(TI) == 2) {
    if (!gemm2_has(variant, __is_same(TI, bf16_t))) return -1;
    if constexpr (__is_same(TI, bf16_t)) {
      if (variant == GV_128_AB) return launch_gemm2<TO, 128, 128, 4, 2, 2>(p, gemm2_xcd_grid(p, 128, 128, p.lda), batch, st);
      if (variant == GV_128_ONE_AB) return launch_gemm2<TO, 128, 128, 4, 2, 2, true>(p, gemm2_xcd_grid(p, 128, 128, p.lda), batch, st);
    }
    switch (variant) {
      case GV_64_DEEP: return launch_gemm2_epi<TO, 64, 64, 2, 2, 4, false, TI>(p, batch, st);
      case GV_64: return launch_gemm2_epi<TO, 64, 64, 2, 2, 2, false, TI>(p, batch, st);
      case GV_256x64: return launch_gemm2_epi<TO, 256, 64, 8, 1, 2, true, TI>(p, batch, st);   // 8 waves of 32 x 64
      case GV_192: return launch_gemm2_epi<TO, 192, 128, 4, 2, 2, true, TI>(p, batch, st);
      case GV_128: return launch_gemm2_epi<TO, 128, 128, 4, 2, 2, true, TI>(p, batch, st);
      case GV_64x128: return launch_gemm2_epi<TO, 64, 128, 2, 2, 4, true, TI>(p, batch, st);
    }
    if constexpr (sizeof(TO) == 2) {      // GV_256
      if (!gemm8_takes(p, batch, 2)) return -1;
      return dispatch_code<11, 21, 12, 22, 13>(gemm_epia(p, true), [&](auto c) {      // the LayerNorm forms add their row statistics to the ring
        constexpr int E = decltype(c)::value;
        return launch_gemm8<gemm8_kernel<TI, E>, GEMM8_RING + (epia_family(E) >= EPI_LN_OPERAND ? 8 * 4096 : 0)>(p, st);
      });
    }
  }
  return -1;
}

// Between 9 600 and 16 000 rows (the training step's M = 12 800: both windows in one batch) the tile follows how full the
// LAST round of 512 workgroups is: 12800 x 768 is 600 tiles of 128 x 128 (one full round + 88 stragglers) but 402 of
// 192 x 128 (one round).  Measured (tools/bench_gemm_variants.py, SHAPES=train): x 768 x 3072 78.9 -> 68.0 us, x 2304 x 768
// 66.1 -> 60.7, x 768 x 768 a tie, x 3072 x 768 79.6 -> 82.4 (kept on 128 x 128 by this rule); 1.2 = the 192-row tile's
// advantage per round-slot on those shapes.
static bool tall_rounds_favour_192(int M, long tiles128, long tiles192) {
  if (M < 9600 || tiles192 < 256) return false;
  const double fill128 = (double)tiles128 / (512.0 * (double)((tiles128 + 511) / 512));
  const double fill192 = (double)tiles192 / (512.0 * (double)((tiles192 + 511) / 512));
  return 1.2 * fill192 > 1.03 * fill128;
}

// An entry's arguments by name; a default means "absent".  The plans read it, gemm_args copies it into the kernels' GemmArgs.
struct GemmCall {
  const void* A = nullptr; const void* W = nullptr; const float* bias = nullptr; const void* residual = nullptr; void* C = nullptr;
  int M = 0, N = 0, K = 0, in_dtype = 0, out_dtype = 0;
  long lda = 0; int rows_per_batch = 0; long a_batch_stride = 0; long ldw = 0, ldc = 0, ldr = 0;
  int act = 0;      // the entry's word: MSMD_ACT_*, MSMD_GEMM_VARIANT, MSMD_GEMM_* flags (gemm_unpack_act)
  int batch = 1; long strideA = 0, strideW = 0, strideC = 0, strideBias = 0, strideR = 0;
  int batch_inner = 1; long strideA2 = 0, strideW2 = 0, strideC2 = 0;
  void* z_out = nullptr; float p_drop = 0.f; const unsigned long* rng = nullptr; unsigned site = 0; int internal_flags = 0;      // the training epilogue; GF_ACT_BWD
  // msmd_gemm_ln: the statistics operands, their slab widths, eps
  const float* a_stats = nullptr; const float* w_colsum = nullptr; const float* r_stats = nullptr; const float* r_gamma = nullptr; const float* r_beta = nullptr;
  float* stats_out = nullptr; int slab_in = 0, slab_out = 0; float eps = 1e-5f;
};

// The one place a GemmArgs is filled; fields it does not name keep the struct's defaults.  act / flags: of the unpacked word, as the
// plan passes them on.  `ab` scales every A / W stride: 2 for split-pair operands (logical sizes in, fp16 strides into the kernel), else 1.
// osz = bytes of an output element, 0 for split-pair output (the entry has required whole 32-element blocks: every vector access is aligned).
static GemmArgs gemm_args(const GemmCall& c, int act, int flags, int osz, int ab = 1) {
  GemmArgs p{};
  const int rows_per_batch = c.rows_per_batch <= 0 ? c.M : c.rows_per_batch;
  p.A = c.A; p.W = c.W; p.bias = c.bias; p.R = c.residual; p.C = c.C;
  p.M = c.M; p.N = c.N; p.K = c.K;
  p.lda = ab * c.lda; p.rows_per_batch = rows_per_batch; p.a_batch_stride = ab * c.a_batch_stride;
  p.ldw = ab * c.ldw; p.ldc = c.ldc; p.ldr = c.ldr; p.act = act;
  p.inv_rpb = 1.0f / (float)rows_per_batch;
  p.strideA = ab * c.strideA; p.strideW = ab * c.strideW; p.strideC = c.strideC; p.strideBias = c.strideBias; p.strideR = c.strideR;
  p.batch_inner = c.batch_inner; p.strideA2 = ab * c.strideA2; p.strideW2 = ab * c.strideW2; p.strideC2 = c.strideC2;
  p.xn = 1;
  p.vec_ok = osz == 0 ||
             ((c.ldc % 4 == 0) && (c.strideC % 4 == 0) && (c.strideC2 % 4 == 0) && (((uintptr_t)c.C % (4 * osz)) == 0) &&
              (!c.residual || ((c.ldr % 4 == 0) && (c.strideR % 4 == 0) && (((uintptr_t)c.residual % (4 * osz)) == 0))));
  if ((flags & GF_PAIRED_STORES) && (osz != 2 || (c.ldc % 8) || (c.strideC % 8) || (c.strideC2 % 8) || ((uintptr_t)c.C % 16) || !p.vec_ok))
    flags &= ~GF_PAIRED_STORES;   // paired stores need 16-byte aligned row pairs
  p.flags = flags;
  return p;
}

// The kernel of a call on split-pair operands: variant 1 / 5 / 14 / 80, -1 for a hint that names none of them.
static int gemm_split_route(const GemmArgs& p, int nz, bool split_out, int hint, int flags) {
  const bool takes8 = gemm8s_takes(p, nz, split_out);
  if (hint == GV_256 && !takes8) hint = 0;   // a hint the call cannot follow
  if (hint) return (hint == GV_SPLIT_128 || hint == GV_SPLIT_64 || hint == GV_256x64 || hint == GV_256) ? hint : -1;
  // the library's own choice takes the 256 x 256 kernel only under MSMD_GEMM_W_BELOW_32: there it returns the bits of
  // gemm2s_kernel's WS form, so the row count of a launch never changes a row's result (its folding form, reachable by the
  // variant hint, sums the cross terms in another order than gemm2s_kernel's two accumulators)
  if (!(flags & GF_NO_256) && (flags & GF_W_BELOW_32) && takes8 && gemm8s_wins(p.M, p.N, p.K, true)) return GV_256;
  if (p.N <= 64) return (long)((p.M + 255) / 256) * nz >= 256 ? GV_256x64 : GV_SPLIT_64;
  return (long)((p.M + 127) / 128) * ((p.N + 127) / 128) * nz >= 192 ? GV_SPLIT_128 : GV_SPLIT_64;
}

// The kernel of a call on 16-bit operands with K % 64 == 0 (msmd_gemm's family and msmd_gemm_ln): the variant dispatch_gemm
// launches, or 0 for gemm_kernel (a hint that names no variant of this operand type).  Measured on MI355X.
// Priority of the library's own choice: 256 x 256, the tall 192 x 128 tile, the last-round fill rule, 128 x 128, 256 x 64, 64 x 64.
// GF_NO_256 (MSMD_GEMM_NO_256_TILE) = the caller opts out of the 256 x 256 kernel (A/B).
// cols: 0 for a plain call, where every tile is open.  msmd_gemm_ln's statistics slabs name the tile family: 128 = the
// 128-column tiles (17 / 15; 64-column slabs, which the 256 x 256 kernel writes too), 64 = the 64 x 64 tiles (9 / 12; 32-column
// slabs, so the 256 x 256 kernel only where the call writes no statistics).  Its hints choose within that family.
static int gemm16_route(const GemmArgs& p, int nz, int osz, bool bf16, int hint, int flags, int cols = 0) {
  const bool takes8 = (cols != 64 || !p.stats_out) && gemm8_takes(p, nz, osz);
  const bool rule8 = hint == 0 && !(flags & GF_NO_256);
  // a hint the call cannot follow leaves the library's own choice: 80 on a call the kernel does not take, and for msmd_gemm_ln
  // anything but 15 / 17 / 18 / 66 inside the 128-column family
  if (!(hint == GV_256 ? takes8 : !cols || (cols == 128 && (hint == GV_192 || hint == GV_128 || hint == GV_128_ONE_AB || hint == GV_64x128)))) hint = 0;
  if (hint) return gemm2_has(hint, bf16) ? hint : GV_GENERIC;
  const int M = p.M, N = p.N;
  const long tiles128 = (long)((M + 127) / 128) * ((N + 127) / 128) * nz;
  const long tiles192 = (long)((M + 191) / 192) * ((N + 127) / 128) * nz;
  const bool wide = cols ? cols == 128 : N > 64;
  if (rule8 && takes8 && gemm8_wins(M, N, p.K)) return GV_256;
  // tall grids: 192 x 128 tiles (76.8 FLOP per staged byte instead of 64, still two workgroups per CU).  Measured against
  // the 128 x 128 tile: conv1 454 -> 379 us, 21312 x 512 x 2048 58.7 -> 49.6, 21312 x 2048 x 512 76.6 -> 64.7; worse
  // below ~16 k rows (12800 x 512 x 1024: 22 -> 28 us) and mixed at M = 6400
  if (wide && M >= 16000 && tiles192 >= 400) return GV_192;
  // inference epilogues only: the 192-row tile's everything-epilogue runs one workgroup per CU
  if (wide && osz == 2 && !p.Z && !(p.p_drop > 0.f) && !(p.flags & GF_ACT_BWD) && tall_rounds_favour_192(M, tiles128, tiles192)) return GV_192;
  // the 128 x 128 LDS-DMA kernel (8 waves as 4 x 2, 2-stage ring, fragment reads pipelined) wins once the grid fills the chip at
  // 2 workgroups per CU; below that, 64 x 64 tiles (deep ring for long K) keep more CUs busy
  // msmd_gemm_ln's 128-column family on a grid that covers half the chip or less with 128 x 128 tiles (the decoder's 3552 x 512:
  // 112 workgroups on 256 CUs, one 32 KB K tile in flight each): 64 x 128 tiles double the workgroups and keep 72 KB in flight.
  // Same wave tile, k order and epilogue: the same bits.  It wins while its one-per-CU workgroups fit ONE round of 256 CUs and
  // loses from the first workgroup of a second round on.  Measured, us hot / cold, 17 -> 18 (tools/bench_small_grid.py bf16 scan):
  //   x 512 x 512:   32 tiles of 128 x 128  15.4 -> 15.4 / 17.4 -> 12.0;  128 tiles 15.3 -> 15.5 / 18.5 -> 13.4;  160 tiles 15.5 -> 17.2 / 18.8 -> 21.0
  //   x 512 x 2048:  32 tiles 24.7 -> 19.0 / 38.4 -> 22.0;  128 tiles 27.3 -> 20.4 / 41.4 -> 24.7;  160 tiles 27.5 -> 36.0 / 43.0 -> 42.8
  // Below 32 tiles nothing was measured: those launches stay on 17.
  const long tiles64x128 = (long)((M + 63) / 64) * ((N + 127) / 128) * nz;
  if (cols == 128 && osz == 2 && !p.Z && !(p.p_drop > 0.f) && !(p.flags & GF_ACT_BWD) && tiles128 >= 32 && tiles64x128 <= 256) return GV_64x128;
  if (cols ? wide : wide && tiles128 >= 192) return GV_128;
  if (!cols && N <= 64 && (long)((M + 255) / 256) * nz >= 256) return GV_256x64;   // the positional conv: 256 x 64 tiles, 140 -> 85 us
  return p.K >= 1024 ? GV_64_DEEP : GV_64;
}

// The plan of a msmd_gemm / msmd_gemm_ex / msmd_gemm_actbwd / msmd_gemm_batched2 call: checks it, fills p and picks the kernel.
// Returns the variant gemm_launch will launch, 0 for gemm_kernel, -1 for a call the library rejects.  Host arithmetic only,
// no HIP call and no state: msmd_gemm_route is this function alone.
static int gemm_plan(GemmArgs& p, const GemmCall& c) {
  if (c.M <= 0 || c.N <= 0 || c.K <= 0 || c.batch <= 0 || c.batch_inner <= 0 || !c.A || !c.W || !c.C) return -1;
  const GemmActWord u = gemm_unpack_act(c.act);
  const int flags = u.flags | c.internal_flags, nz = c.batch * c.batch_inner;
  const auto strides_divide = [&](int E) {
    return !(c.K % E || c.lda % E || c.ldw % E || c.a_batch_stride % E || c.strideA % E || c.strideW % E || c.strideA2 % E || c.strideW2 % E);
  };
  if (c.in_dtype == MSMD_F16X2) {
    // split-pair operands: 32-element blocks must stay whole
    if (c.out_dtype != MSMD_F32 && c.out_dtype != MSMD_F16X2) return -1;
    if (!strides_divide(32) || c.z_out || c.p_drop != 0.f) return -1;
    if (((uintptr_t)c.A & 15) || ((uintptr_t)c.W & 15) || ((uintptr_t)c.C & 15)) return -1;
    if (c.out_dtype == MSMD_F16X2) {
      if ((c.N & 3) || c.ldc % 32 || c.strideC % 32 || c.strideC2 % 32 || (c.residual && (c.ldr % 32 || c.strideR % 32))) return -1;
      if (c.bias && (((uintptr_t)c.bias & 15) || (c.strideBias & 3))) return -1;
    }
    p = gemm_args(c, u.act, flags & (GF_WRITE_THROUGH | GF_W_BELOW_32), c.out_dtype == MSMD_F32 ? 4 : 0, 2);
    return gemm_split_route(p, nz, c.out_dtype == MSMD_F16X2, u.hint, flags);
  }
  if (c.in_dtype == MSMD_F32 ? (c.out_dtype != MSMD_F32 && c.out_dtype != MSMD_F16 && c.out_dtype != MSMD_BF16)
                             : ((c.in_dtype != MSMD_F16 && c.in_dtype != MSMD_BF16) || (c.out_dtype != c.in_dtype && c.out_dtype != MSMD_F32)))
    return -1;
  if (!strides_divide(c.in_dtype == MSMD_F32 ? 4 : 8)) return -1;
  if (((uintptr_t)c.A & 15) || ((uintptr_t)c.W & 15)) return -1;
  if (c.p_drop != 0.f && (!(c.p_drop > 0.f && c.p_drop < 1.f) || !c.rng || (c.N & 3) || c.ldc != c.N || c.batch != 1 || c.batch_inner != 1))
    return -1;  // the mask index assumes one contiguous (M, N) output
  const int osz = c.out_dtype == MSMD_F32 ? 4 : 2;
  p = gemm_args(c, u.act, flags, osz);
  p.Z = c.z_out; p.p_drop = c.p_drop; p.rng = c.rng; p.site = c.site;     // the training epilogue (msmd_gemm_ex, msmd_gemm_actbwd)
  if (c.in_dtype == MSMD_F32 || (c.K % 64)) return GV_GENERIC;    // the LDS-DMA kernels: 16-bit operands in whole 128-byte K tiles
  return gemm16_route(p, nz, osz, c.in_dtype == MSMD_BF16, u.hint, flags);
}

// One dispatch from the (in, out) dtype pair, which the plan has accepted, to the template types.  -1: no such kernel.
static int gemm_launch(GemmArgs& p, int in_dtype, int out_dtype, int nz, int variant, hipStream_t st) {
  switch (in_dtype * 4 + out_dtype) {
    case MSMD_F16X2 * 4 + MSMD_F32: return dispatch_gemm2s<float>(p, nz, st, variant);
    case MSMD_F16X2 * 4 + MSMD_F16X2: return dispatch_gemm2s<f16_t>(p, nz, st, variant);
    case MSMD_BF16 * 4 + MSMD_BF16: return dispatch_gemm<bf16_t, bf16_t>(p, nz, st, variant);
    case MSMD_BF16 * 4 + MSMD_F32: return dispatch_gemm<float, bf16_t>(p, nz, st, variant);
    case MSMD_F16 * 4 + MSMD_F16: return dispatch_gemm<f16_t, f16_t>(p, nz, st, variant);
    case MSMD_F16 * 4 + MSMD_F32: return dispatch_gemm<float, f16_t>(p, nz, st, variant);
    case MSMD_F32 * 4 + MSMD_F32: return dispatch_gemm<float, float>(p, nz, st, variant);
    case MSMD_F32 * 4 + MSMD_F16: return dispatch_gemm<f16_t, float>(p, nz, st, variant);
    case MSMD_F32 * 4 + MSMD_BF16: return dispatch_gemm<bf16_t, float>(p, nz, st, variant);
  }
  return -1;
}

// An entry: the plan, then the launch.
static int gemm_run(int (*plan)(GemmArgs&, const GemmCall&), const GemmCall& c, msmd_stream_t stream) {
  GemmArgs p;
  const int variant = plan(p, c);
  const int r = variant < 0 ? -1 : gemm_launch(p, c.in_dtype, c.out_dtype, c.batch * c.batch_inner, variant, (hipStream_t)stream);
  return r >= 0 ? r : 1;     // a call the plan rejects; a variant the plan chose and the dispatch does not have is an error, never another kernel
}

// The call record of msmd_gemm_ex's argument list (msmd_gemm: the same without the training epilogue; msmd_gemm_route)
static GemmCall gemm_ex_call(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K, int in_dtype,
                             int out_dtype, long lda, int rows_per_batch, long a_batch_stride, long ldw, long ldc, long ldr, int act, int batch,
                             long strideA, long strideW, long strideC, long strideBias, long strideR, void* z_out, float p_drop,
                             const unsigned long* rng_state, unsigned int site) {
  GemmCall c;
  c.A = A; c.W = W; c.bias = bias; c.residual = residual; c.C = C;
  c.M = M; c.N = N; c.K = K; c.in_dtype = in_dtype; c.out_dtype = out_dtype;
  c.lda = lda; c.rows_per_batch = rows_per_batch; c.a_batch_stride = a_batch_stride; c.ldw = ldw; c.ldc = ldc; c.ldr = ldr;
  c.act = act; c.batch = batch;
  c.strideA = strideA; c.strideW = strideW; c.strideC = strideC; c.strideBias = strideBias; c.strideR = strideR;
  c.z_out = z_out; c.p_drop = p_drop; c.rng = rng_state; c.site = site;
  return c;
}

extern "C" int msmd_gemm_ex(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K, int in_dtype,
                            int out_dtype, long lda, int rows_per_batch, long a_batch_stride, long ldw, long ldc, long ldr, int act, int batch,
                            long strideA, long strideW, long strideC, long strideBias, long strideR, void* z_out, float p_drop,
                            const unsigned long* rng_state, unsigned int site, msmd_stream_t stream) {
  return gemm_run(gemm_plan, gemm_ex_call(A, W, bias, residual, C, M, N, K, in_dtype, out_dtype, lda, rows_per_batch, a_batch_stride, ldw, ldc, ldr,
                                          act, batch, strideA, strideW, strideC, strideBias, strideR, z_out, p_drop, rng_state, site), stream);
}

extern "C" int msmd_gemm(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K, int in_dtype,
                         int out_dtype, long lda, int rows_per_batch, long a_batch_stride, long ldw, long ldc, long ldr, int act, int batch,
                         long strideA, long strideW, long strideC, long strideBias, long strideR, msmd_stream_t stream) {
  return msmd_gemm_ex(A, W, bias, residual, C, M, N, K, in_dtype, out_dtype, lda, rows_per_batch, a_batch_stride, ldw, ldc, ldr,
                      act, batch, strideA, strideW, strideC, strideBias, strideR, nullptr, 0.f, nullptr, 0, stream);
}

// What msmd_gemm_ex (and msmd_gemm: z_out = NULL, p_drop = 0) would launch for the same arguments: the variant, 0 for
// gemm_kernel, -1 for a call it rejects.  Launches nothing.
extern "C" int msmd_gemm_route(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K, int in_dtype,
                               int out_dtype, long lda, int rows_per_batch, long a_batch_stride, long ldw, long ldc, long ldr, int act, int batch,
                               long strideA, long strideW, long strideC, long strideBias, long strideR, void* z_out, float p_drop,
                               const unsigned long* rng_state, unsigned int site, msmd_stream_t) {
  GemmArgs p;
  return gemm_plan(p, gemm_ex_call(A, W, bias, residual, C, M, N, K, in_dtype, out_dtype, lda, rows_per_batch, a_batch_stride, ldw, ldc, ldr,
                                   act, batch, strideA, strideW, strideC, strideBias, strideR, z_out, p_drop, rng_state, site));
}

// Whether a msmd_gemm_ln call that routes to variant 17 launches its 160 x 128 member (gemm2_kernel<160, 128, 5 x 2 waves, 4-stage ring>).
// The kernel takes the residual form without an activation in the 128-column family.  The library's own choice (no hint): the
// 128 x 128 tiles are more than the 256 CUs, so some CU would carry two workgroups and take in twice the operands of the others,
// while 160-row tiles put the whole grid, XCD padding included, into one round of one workgroup per CU with 108 KB in flight each.
// MSMD_GEMM_NO_160_ROW_TILE opts out, MSMD_GEMM_FORCE_160_ROW_TILE takes the member wherever the kernel takes the call.
static bool gemm_ln_takes_160_rows(const GemmArgs& p, int cols, const GemmActWord& u) {
  if (cols != 128 || p.a_stats || !p.R || p.act != MSMD_ACT_NONE || (u.flags & GF_NO_160)) return false;
  if (u.flags & GF_FORCE_160) return true;
  if (u.hint) return false;
  if ((long)((p.M + 127) / 128) * ((p.N + 127) / 128) <= 256) return false;
  GemmArgs q = p;
  return gemm160_one_round_grid(q) > 0;
}

// C = act(LN_A(A) . W^T + bias) + LN_R(residual), with the LayerNorms folded into this GEMM's epilogue and (optionally)
// the row statistics of C written for the next consumer: see GemmArgs and include/msmd_hip.h.  Plain row-major operands,
// no batch, 16-bit operands and output.  The statistics' slab width names the kernel that writes them: 64 = the
// 128 x 128 tile, 32 = the 64 x 64 tile (grids that would not fill the chip with 128 x 128 tiles).
static int gemm_ln_plan(GemmArgs& p, const GemmCall& c) {
  const int M = c.M, N = c.N, K = c.K;
  if (M <= 0 || N <= 0 || K <= 0 || !c.A || !c.W || !c.C || (K % 64) || (N % 64)) return -1;
  if ((c.in_dtype != MSMD_BF16 && c.in_dtype != MSMD_F16) || c.out_dtype != c.in_dtype) return -1;   // 16-bit rows in and out
  if ((c.lda % 8) || (c.ldw % 8) || (c.ldc % 4) || (c.residual && (c.ldr % 4))) return -1;
  if (((uintptr_t)c.A & 15) || ((uintptr_t)c.W & 15) || ((uintptr_t)c.C & 15) || ((uintptr_t)c.residual & 7) || ((uintptr_t)c.bias & 15)) return -1;
  if ((c.a_stats != nullptr) != (c.w_colsum != nullptr)) return -1;
  if (!c.bias || (c.a_stats && (c.residual || c.stats_out)) || (!c.a_stats && !c.residual)) return -1;   // the two epilogue modes
  if (c.r_stats && (!c.residual || !c.r_gamma || !c.r_beta || c.a_stats)) return -1;   // one side per call
  if (((uintptr_t)c.w_colsum & 15) || ((uintptr_t)c.r_gamma & 15) || ((uintptr_t)c.r_beta & 15)) return -1;
  if (((uintptr_t)c.a_stats & 7) || ((uintptr_t)c.r_stats & 7) || ((uintptr_t)c.stats_out & 7)) return -1;
  if ((c.a_stats || c.r_stats) && c.slab_in != 32 && c.slab_in != 64) return -1;
  if (c.stats_out && c.slab_out != 32 && c.slab_out != 64) return -1;
  if ((c.a_stats && (K % c.slab_in)) || (c.r_stats && (N % c.slab_in))) return -1;
  // the tile family (gemm16_route's `cols`): the statistics' slab where the call writes them, else by the grid
  const long tiles128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  const int cols = (c.stats_out ? c.slab_out == 64 : (tiles128 >= 192 && (N % 128) == 0)) ? 128 : 64;
  if (cols == 128 && (N % 128)) return -1;
  // of the word's flags this entry honours MSMD_GEMM_ONE_TILE_PER_WORKGROUP, MSMD_GEMM_NO_256_TILE and the two 160-row bits; paired
  // 16-byte stores always, where the rows allow them
  const GemmActWord u = gemm_unpack_act(c.act);
  p = gemm_args(c, u.act, GF_PAIRED_STORES | (u.flags & GF_ONE_TILE), 2);
  p.a_stats = c.a_stats; p.a_nt = c.a_stats ? K / c.slab_in : 0; p.w_colsum = c.w_colsum;
  p.r_stats = c.r_stats; p.r_nt = c.r_stats ? N / c.slab_in : 0; p.r_gamma = c.r_gamma; p.r_beta = c.r_beta;
  p.stats_out = c.stats_out; p.ln_eps = c.eps;
  // the caller's tile hint chooses within the 128-column family (15 = 192 x 128, 17 = 128 x 128, 18 = 64 x 128, 66 = A/B form of 17) or names
  // the 256 x 256 kernel (80), which writes the same 64-column statistics slabs and reads either width
  const int variant = gemm16_route(p, 1, 2, c.in_dtype == MSMD_BF16, u.hint, u.flags & GF_NO_256, cols);
  if (variant == GV_128 && gemm_ln_takes_160_rows(p, cols, u)) p.flags |= GF_ROWS_160;
  return variant != GV_GENERIC ? variant : -1;      // no LayerNorm epilogue in gemm_kernel
}

// The rows of C per workgroup of the launch a msmd_gemm_ln plan describes
static int gemm_ln_plan_rows(const GemmArgs& p, int variant) {
  switch (variant) {
    case GV_64_DEEP: case GV_64: case GV_64x128: return 64;
    case GV_128: return (p.flags & GF_ROWS_160) ? 160 : 128;
    case GV_128_AB: case GV_128_ONE_AB: return 128;
    case GV_192: return 192;
    case GV_256: case GV_256x64: return 256;
  }
  return -1;
}

static GemmCall gemm_ln_call(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K, int in_dtype,
                             int out_dtype, long lda, long ldw, long ldc, long ldr, int act, const float* a_stats, const float* w_colsum,
                             const float* r_stats, const float* r_gamma, const float* r_beta, float* stats_out, int slab_in, int slab_out, float eps) {
  GemmCall c;
  c.A = A; c.W = W; c.bias = bias; c.residual = residual; c.C = C;
  c.M = M; c.N = N; c.K = K; c.in_dtype = in_dtype; c.out_dtype = out_dtype;
  c.lda = lda; c.ldw = ldw; c.ldc = ldc; c.ldr = ldr; c.act = act;
  c.a_stats = a_stats; c.w_colsum = w_colsum; c.r_stats = r_stats; c.r_gamma = r_gamma; c.r_beta = r_beta;
  c.stats_out = stats_out; c.slab_in = slab_in; c.slab_out = slab_out; c.eps = eps;
  return c;
}

extern "C" int msmd_gemm_ln(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K, int in_dtype,
                            int out_dtype, long lda, long ldw, long ldc, long ldr, int act, const float* a_stats, const float* w_colsum,
                            const float* r_stats, const float* r_gamma, const float* r_beta, float* stats_out, int slab_in, int slab_out,
                            float eps, msmd_stream_t stream) {
  return gemm_run(gemm_ln_plan, gemm_ln_call(A, W, bias, residual, C, M, N, K, in_dtype, out_dtype, lda, ldw, ldc, ldr, act, a_stats,
                                             w_colsum, r_stats, r_gamma, r_beta, stats_out, slab_in, slab_out, eps), stream);
}

// What msmd_gemm_ln would launch for the same arguments: the variant, or -1 for a call it rejects.  Launches nothing.
extern "C" int msmd_gemm_ln_route(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K,
                                  int in_dtype, int out_dtype, long lda, long ldw, long ldc, long ldr, int act, const float* a_stats,
                                  const float* w_colsum, const float* r_stats, const float* r_gamma, const float* r_beta, float* stats_out,
                                  int slab_in, int slab_out, float eps, msmd_stream_t) {
  GemmArgs p;
  return gemm_ln_plan(p, gemm_ln_call(A, W, bias, residual, C, M, N, K, in_dtype, out_dtype, lda, ldw, ldc, ldr, act, a_stats,
                                      w_colsum, r_stats, r_gamma, r_beta, stats_out, slab_in, slab_out, eps));
}

// The rows of C per workgroup of the launch msmd_gemm_ln would make for the same arguments, or -1 for a call it rejects.  Launches nothing.
extern "C" int msmd_gemm_ln_rows(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K,
                                 int in_dtype, int out_dtype, long lda, long ldw, long ldc, long ldr, int act, const float* a_stats,
                                 const float* w_colsum, const float* r_stats, const float* r_gamma, const float* r_beta, float* stats_out,
                                 int slab_in, int slab_out, float eps, msmd_stream_t) {
  GemmArgs p;
  const int variant = gemm_ln_plan(p, gemm_ln_call(A, W, bias, residual, C, M, N, K, in_dtype, out_dtype, lda, ldw, ldc, ldr, act, a_stats,
                                                   w_colsum, r_stats, r_gamma, r_beta, stats_out, slab_in, slab_out, eps));
  return variant < 0 ? -1 : gemm_ln_plan_rows(p, variant);
}

// dZ = keep_mask / (1 - p) * act'(Z) * (A . W^T): the data gradient of a Linear whose INPUT was dropout(act(Z)) -- the product
// and the backward of the activation + dropout in one launch (A = the upstream gradient, W = the transposed weight cast,
// Z = the forward's pre-activation, C and Z contiguous (M, N)).  Replaces msmd_gemm + msmd_act_bwd_dropout / msmd_act_bwd.
extern "C" int msmd_gemm_actbwd(const void* A, const void* W, const void* Z, void* C, int M, int N, int K, int in_dtype, int out_dtype, long lda,
                                long ldw, int act, float p_drop, const unsigned long* rng_state, unsigned int site, msmd_stream_t stream) {
  if (!Z || in_dtype != out_dtype || (in_dtype != MSMD_BF16 && in_dtype != MSMD_F16) || (N & 3) || ((uintptr_t)Z & 7)) return 1;
  if (K % 64) return 1;      // the LDS-DMA kernels only (the others do not carry this epilogue)
  GemmCall c;
  c.A = A; c.W = W; c.C = C; c.M = M; c.N = N; c.K = K; c.in_dtype = in_dtype; c.out_dtype = out_dtype;
  c.lda = lda; c.ldw = ldw; c.ldc = N; c.act = act & (0xffff | MSMD_GEMM_WRITE_THROUGH | MSMD_GEMM_PAIRED_STORES);
  c.z_out = const_cast<void*>(Z); c.p_drop = p_drop; c.rng = rng_state; c.site = site; c.internal_flags = GF_ACT_BWD;
  return gemm_run(gemm_plan, c, stream);
}

extern "C" int msmd_gemm_batched2(const void* A, const void* W, void* C, int M, int N, int K, int in_dtype, int out_dtype, long lda, long ldw,
                                  long ldc, int batch_outer, long strideA_o, long strideW_o, long strideC_o, int batch_inner, long strideA_i,
                                  long strideW_i, long strideC_i, msmd_stream_t stream) {
  GemmCall c;
  c.A = A; c.W = W; c.C = C; c.M = M; c.N = N; c.K = K; c.in_dtype = in_dtype; c.out_dtype = out_dtype;
  c.lda = lda; c.ldw = ldw; c.ldc = ldc; c.act = MSMD_ACT_NONE;
  c.batch = batch_outer; c.strideA = strideA_o; c.strideW = strideW_o; c.strideC = strideC_o;
  c.batch_inner = batch_inner; c.strideA2 = strideA_i; c.strideW2 = strideW_i; c.strideC2 = strideC_i;
  return gemm_run(gemm_plan, c, stream);
}

// ---------------------------------------------------------------------------------------------------
// msmd_conv_chain: 2 to 4 strided Conv1d layers over a channels-last signal as ONE launch of gemm8_chain_kernel (see CHAIN at
// gemm8_body).  The table of the shapes alone (no pointers): what msmd_conv_chain_plan and msmd_conv_chain_workspace answer from.
// False for what the kernel does not take.
static bool conv_chain_table(ChainTable& t, int B, int T0, int C, int N, int n, const int* kernel, const int* stride, int flags) {
  if (B <= 0 || T0 <= 0 || C <= 0 || N <= 0 || n < 2 || n > 4 || !kernel || !stride || (N % 256)) return false;
  t = ChainTable{};
  t.n = n; t.nt = N / 256;
  t.per_block = (flags & MSMD_CONV_CHAIN_ROW_BLOCK_TICKETS) != 0;
  t.release = (flags & MSMD_CONV_CHAIN_RELEASE) != 0;
  long t_in = T0, c_in = C;
  int tickets = 0, counters = 0;
  for (int l = 0; l < n; ++l) {
    ChainProblem& q = t.pr[l];
    if (kernel[l] <= 0 || stride[l] <= 0 || t_in < kernel[l]) return false;
    const long t_out = (t_in - kernel[l]) / stride[l] + 1, M = (long)B * t_out, K = kernel[l] * c_in;
    if ((K % 64) || K < 128 || M >= (1L << 24)) return false;      // whole 128-byte K tiles, two of them; a_row_offset's fp32 reciprocal
    q.M = (int)M; q.K = (int)K; q.rows_per_batch = (int)t_out; q.inv_rpb = 1.0f / (float)t_out;
    q.lda = stride[l] * c_in; q.a_batch_stride = t_in * c_in;
    q.t_in = (int)t_in; q.stride = stride[l]; q.taps = kernel[l];
    q.mt = (int)((M + 255) / 256);
    q.ticket0 = tickets; q.cnt0 = counters;
    tickets += t.per_block ? q.mt : q.mt * t.nt;
    counters += q.mt;
    // 32-bit staging offsets from A / W
    if (((long)(B - 1) * q.a_batch_stride + (t_out - 1) * q.lda + K) * 2 >= (1L << 32) || (long)N * K * 2 >= (1L << 32)) return false;
    t_in = t_out; c_in = N;
  }
  t.total = tickets;
  return true;
}
static long conv_chain_state_bytes(const ChainTable& t) {
  const long words = CHAIN_STATE_HEAD + t.pr[t.n - 1].cnt0 + t.pr[t.n - 1].mt;
  return (words * 4 + 15) / 16 * 16;
}

extern "C" long msmd_conv_chain_workspace(int B, int T0, int C, int N, int n_layers, const int* kernel, const int* stride) {
  ChainTable t;
  return conv_chain_table(t, B, T0, C, N, n_layers, kernel, stride, 0) ? conv_chain_state_bytes(t) : 0;
}

extern "C" int msmd_conv_chain_plan(int B, int T0, int C, int N, int n_layers, const int* kernel, const int* stride, int flags, int ticket,
                                    int* out6) {
  ChainTable t;
  if (!out6 || !conv_chain_table(t, B, T0, C, N, n_layers, kernel, stride, flags)) return -1;
  ChainTile z;
  if (!chain_decode(t, ticket, z)) return t.total;      // past the last ticket: the ticket count (>= 1), nothing written
  out6[0] = z.l; out6[1] = z.rb; out6[2] = z.ct; out6[3] = z.nct; out6[4] = z.pb0; out6[5] = z.pb1;
  return 0;
}

extern "C" int msmd_conv_chain(const void* x, int B, int T0, int C, int N, int n_layers, const void* const* w, const float* const* bias,
                               void* const* out, const int* kernel, const int* stride, int act, int dtype, void* workspace,
                               long workspace_bytes, int max_workgroups, int flags, msmd_stream_t stream) {
  ChainTable t;
  if ((dtype != MSMD_BF16 && dtype != MSMD_F16) || (act != MSMD_ACT_NONE && act != MSMD_ACT_GELU) || !x || !w || !bias || !out || !workspace) return 1;
  if (!conv_chain_table(t, B, T0, C, N, n_layers, kernel, stride, flags)) return 1;
  const long state_bytes = conv_chain_state_bytes(t);
  if (workspace_bytes < state_bytes || ((uintptr_t)workspace & 15) || max_workgroups < 0) return 1;
  for (int l = 0; l < n_layers; ++l) {
    ChainProblem& q = t.pr[l];
    q.A = l ? out[l - 1] : x; q.W = w[l]; q.bias = bias[l]; q.C = out[l];
    if (!q.W || !q.C || ((uintptr_t)q.A & 15) || ((uintptr_t)q.W & 15) || ((uintptr_t)q.bias & 15) || ((uintptr_t)q.C & 15)) return 1;
  }
  t.state = (unsigned*)workspace;
  GemmArgs p{};      // what the problems share; gemm8_body's chain_problem fills in the rest per tile
  p.N = N; p.ldc = N; p.act = act; p.vec_ok = 1; p.batch_inner = 1; p.xn = 1; p.nt = t.nt;
  p.A = t.pr[0].A; p.W = t.pr[0].W; p.C = t.pr[0].C; p.M = t.pr[0].M; p.K = t.pr[0].K;
  const int cap = gemm8_workgroup_cap();
  int grid = t.total < cap ? t.total : cap;
  if (max_workgroups > 0 && max_workgroups < grid) grid = max_workgroups;
  hipStream_t st = (hipStream_t)stream;
  // the polled words start from zero in every call: the library's zeroing launch (common.h), under capture a kernel node that is
  // replayed ahead of the chain.  (A hipMemsetAsync here was captured as a memset node that zeroed the block in the first replay
  // and filled it with a 32-byte pattern of other data from the second replay on: DESIGN.md 5.26.)
  if (const hipError_t e = msmd_zero_async(workspace, (size_t)state_bytes, st); e != hipSuccess) return (int)e;
  constexpr int LDS = GEMM8_RING + 16;      // + the workgroup's mailbox
  const int code = epia(EPI_PLAIN, act);
  if (dtype == MSMD_BF16)
    return dispatch_code<11, 21>(code, [&](auto c) { return gemm_launch_kernel<gemm8_chain_kernel<bf16_t, decltype(c)::value>>(dim3(grid), 512, LDS, st, p, t); });
  return dispatch_code<11, 21>(code, [&](auto c) { return gemm_launch_kernel<gemm8_chain_kernel<f16_t, decltype(c)::value>>(dim3(grid), 512, LDS, st, p, t); });
}

// The status word of a finished launch (0, or MSMD_CONV_CHAIN_TIMEOUT where a wait expired): a blocking copy, for tests and tools.
extern "C" int msmd_conv_chain_status(const void* workspace) {
  unsigned s = 0;
  if (!workspace || hipMemcpy(&s, (const unsigned*)workspace + 1, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (int)s;
}
