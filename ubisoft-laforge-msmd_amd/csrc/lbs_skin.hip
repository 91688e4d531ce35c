// FLAME skinning: blendshapes + pose correctives + skinning fused in ONE kernel, in three forms (exact fp32 MFMA; split bf16;
// split bf16 / fp16 with the joint blend on the matrix pipe too), their operand packers and the backward.  The per-frame
// kinematics are in flame.hip, the tile record in lbs_tiles.h.  Reference: utils/lbs.py:141-223.
//
// Skinning kernel (the HBM-relevant one): per frame it must write 5023*3 fp32 (60 276 B) and read 186 coefficients; everything
// else (dirs 11.6 MB, weights, template) is frame-invariant and cache resident.  The contraction v_posed = template +
// coef(186) . dirs(186 x 15069) runs on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): a workgroup owns 64 vertices (16 per
// wave), keeps their three coordinate planes of `dirs` in REGISTERS (3 x 48 VGPRs per lane, loaded once) and streams frame
// tiles of 16 through it, so the reference's materialised (B, V, 4, 4) transforms, W.expand and homogeneous coordinates (about
// 10x the algorithmic bytes) never exist.  The vertex sits on the MFMA lane, so the per-vertex blend T = sum_j w_j A_j and the
// 3x4 transform are lane-local; 16 lanes store 16 consecutive vertices (192 contiguous bytes) per frame.
#include "gemm_tiles.h"
#include "lbs_tiles.h"

// ---------------------------------------------------------------------------------------------------
// Pieces the kernels share.
// Split-bf16 product  coef . dirs ~= c_lo.d_hi + c_hi.d_lo + c_hi.d_hi  on v_mfma_f32_16x16x32_bf16, the small terms first
// (the dropped lo.lo term is 2^-16 relative).
__device__ __forceinline__ f32x4 mma_bf16x3(f32x4 acc, const bf16x8 ah, const bf16x8 al, const u32x4 dh, const u32x4 dl) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, __builtin_bit_cast(bf16x8, dh), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, __builtin_bit_cast(bf16x8, dl), acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, __builtin_bit_cast(bf16x8, dh), acc, 0, 0, 0);
}
// The `dirs` planes of the lane's vertex v -> registers: K octet 4 g + q of K group g, three coordinates.  dirs_hl is
// (2, 3, Kp / 8, Vp, 8), hi then lo; NL = KG loads both planes, anything else the first only (the ONE fp16 plane).
template <int KG, int NL>
__device__ __forceinline__ void load_dirs(const bf16_t* __restrict__ dirs_hl, int Vp, int q, int v, u32x4 (&dh)[3][KG],
                                          u32x4 (&dl)[3][NL]) {
  constexpr int Kp = KG * 32;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      const long off = (((long)c * (Kp / 8) + 4 * g + q) * Vp + v) * 8;
      dh[c][g] = *(const u32x4*)(dirs_hl + off);
      if constexpr (NL == KG) dl[c][g] = *(const u32x4*)(dirs_hl + (long)3 * (Kp / 8) * Vp * 8 + off);
    }
}
// 1-D grids: workgroup L -> (vertex tile, frame split).  Workgroups go to the XCDs round-robin (L & 7), and every frame split
// of one vertex tile runs on the SAME XCD: the tile's blendshape directions (147 KB per 64 vertices) are fetched into one L2
// once and re-read from there by the other splits instead of bouncing through all eight.  vt8 = ceil(vertex tiles / 8); a
// tile number past the last is a workgroup with nothing to do.  adjacent: each XCD owns vt8 ADJACENT tiles and walks them
// fastest; otherwise the tiles are dealt to the XCDs one by one.
struct SkinTile { int v_tile, split; };
__device__ __forceinline__ SkinTile xcd_skin_tile(int L, int vt8, bool adjacent) {
  return {adjacent ? (L & 7) * vt8 + ((L >> 3) % vt8) : (L & 7) + 8 * ((L >> 3) % vt8), (L >> 3) / vt8};
}
// Frame splits per vertex tile: enough workgroups to fill the chip (target_workgroups), at least 64 frames per workgroup to
// amortise its dirs load, whole 16-frame tiles.
struct SkinPlan { int splits, fpb; };
static SkinPlan skin_plan(int B, int vertex_tiles, int target_workgroups) {
  const int splits = max(1, min((B + 63) / 64, (target_workgroups + vertex_tiles - 1) / vertex_tiles));
  const int fpb = (((B + splits - 1) / splits) + 15) / 16 * 16;
  return {(B + fpb - 1) / fpb, fpb};
}

// ---------------------------------------------------------------------------------------------------
// Fused blendshape + skinning.  KS = Kp / 4 MFMA steps; lane (q = l>>4, i = l&15) owns k = q*KS + s at step s for BOTH operands
// (a K permutation leaves the contraction unchanged).
template <int KS, int J>
__global__ __launch_bounds__(256) void lbs_skin_kernel(const float* __restrict__ coef, const float* __restrict__ A,
                                                       const float* __restrict__ tmpl, const float* __restrict__ dirs,
                                                       const float* __restrict__ wts, float* __restrict__ verts, int B,
                                                       int V, int Vp, int frames_per_block) {
  constexpr int Kp = KS * 4;
  __shared__ __attribute__((aligned(16))) float sA[16 * J * 12];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int v = blockIdx.x * 64 + wid * 16 + i;  // < Vp by construction
  const int f_begin = blockIdx.y * frames_per_block;
  const int f_end = min(B, f_begin + frames_per_block);

  // frame-invariant operands -> registers
  float d[3][KS];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int s = 0; s < KS; ++s) d[c][s] = dirs[((long)c * Kp + q * KS + s) * Vp + v];
  float t3[3], w[J];
#pragma unroll
  for (int c = 0; c < 3; ++c) t3[c] = tmpl[(long)c * Vp + v];
#pragma unroll
  for (int j = 0; j < J; ++j) w[j] = wts[(long)j * Vp + v];

  for (int f0 = f_begin; f0 < f_end; f0 += 16) {
    __syncthreads();
    for (int k = tid; k < 16 * J * 12; k += 256) {
      const int f = f0 + k / (J * 12);
      sA[k] = f < f_end ? A[(long)f * J * 12 + k % (J * 12)] : 0.f;
    }
    // A operand: row = frame f0 + i, k = q*KS + s  (16-B loads, 4 steps each)
    const int fa = min(f0 + i, B - 1);
    const float* crow = coef + (long)fa * Kp + q * KS;
    f32x4 acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const f32x4 a = *(const f32x4*)(crow + s4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], d[c][s4 * 4 + e], acc[c], 0, 0, 0);
    }
    __syncthreads();
    // epilogue: lane = vertex v, frames f0 + 4q + e
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int fl = 4 * q + e, f = f0 + fl;
      float T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const f32x4* ap = (const f32x4*)(sA + (fl * J + j) * 12);
        const f32x4 a0 = ap[0], a1 = ap[1], a2 = ap[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          T[k] = fmaf(w[j], a0[k], T[k]);
          T[4 + k] = fmaf(w[j], a1[k], T[4 + k]);
          T[8 + k] = fmaf(w[j], a2[k], T[8 + k]);
        }
      }
      const float px = t3[0] + acc[0][e], py = t3[1] + acc[1][e], pz = t3[2] + acc[2][e];
      if (f < f_end && v < V) {
        float* o = verts + ((long)f * V + v) * 3;
        o[0] = T[0] * px + T[1] * py + T[2] * pz + T[3];
        o[1] = T[4] * px + T[5] * py + T[6] * pz + T[7];
        o[2] = T[8] * px + T[9] * py + T[10] * pz + T[11];
      }
    }
  }
}

extern "C" int msmd_lbs_skin(const float* coef, const float* A, const float* v_template, const float* dirs,
                             const float* lbs_weights, float* verts, int B, int J, int V, int Vp, int Kp, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || Vp < V || (Vp & 63) || J != LBS_J || Kp != LBS_KP) return 1;  // FLAME2020 geometry
  const int vt = Vp / 64;
  const SkinPlan plan = skin_plan(B, vt, 2048);
  dim3 grid(vt, plan.splits), block(256);
  hipLaunchKernelGGL((lbs_skin_kernel<LBS_KP / 4, LBS_J>), grid, block, 0, (hipStream_t)stream, coef, A, v_template, dirs,
                     lbs_weights, verts, B, V, Vp, plan.fpb);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
// Fused blendshape + skinning, split-bf16 form: coef = c_hi + c_lo, dirs = d_hi + d_lo (bf16 each), three products per K
// group (mma_bf16x3) with fp32 accumulation: 54 MFMAs x 16 cycles per 16x16 tile instead of 144 x 32 on
// the fp32 MFMA, which moves the kernel from matrix-bound to the epilogue / HBM-write side.  Same register
// residency of dirs (144 VGPRs), same lane-local epilogue.  dirs_hl: (2, 3, Kp/8, Vp, 8) bf16.
template <int KG, int J>  // KG = Kp / 32 MFMA K groups
__global__ __launch_bounds__(256) void lbs_skin_bf16x3_kernel(const bf16_t* __restrict__ coef_hl, const float* __restrict__ A,
                                                              const float* __restrict__ tmpl, const bf16_t* __restrict__ dirs_hl,
                                                              const float* __restrict__ wts, float* __restrict__ verts,
                                                              int B, int V, int Vp, int frames_per_block) {
  constexpr int Kp = KG * 32;
  static_assert(Kp == LBS_KP, "the stage holds a tile record's coefficient planes");
  constexpr int NCH = 2 * Kp / 8;               // 16-B chunks per frame row of coef_hl (hi then lo)
  constexpr int COEF_BYTES = LBS_TILE_COEF_BYTES;   // one 16-frame tile in the record's chunk-major layout (tile_coef_off)
  constexpr int A_BYTES = 16 * J * 12 * 4;      // 16 frames x J x 3x4 fp32
  constexpr int A_CHUNKS = A_BYTES / 16;
  constexpr int STAGE = COEF_BYTES + ((A_BYTES + 1023) / 1024) * 1024;
  // Two stages, filled by LDS-DMA one tile ahead of the MFMAs (no register staging, one barrier per tile).
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, q = lane >> 4;
  const SkinTile wg = xcd_skin_tile(blockIdx.x, (Vp / 64 + 7) >> 3, false);
  if (wg.v_tile * 64 >= Vp) return;
  const int v = wg.v_tile * 64 + wid * 16 + i;
  const int f_begin = wg.split * frames_per_block;
  const int f_end = min(B, f_begin + frames_per_block);

  u32x4 dh[3][KG], dl[3][KG];
  load_dirs<KG, KG>(dirs_hl, Vp, q, v, dh, dl);
  float t3[3], w[J];
#pragma unroll
  for (int c = 0; c < 3; ++c) t3[c] = tmpl[(long)c * Vp + v];
#pragma unroll
  for (int j = 0; j < J; ++j) w[j] = wts[(long)j * Vp + v];

  auto issue = [&](int f0, int stage) {
    unsigned char* base = smem + stage * STAGE;
    // coefficient tile: LDS slot p = chunk*16 + frame  <-  global (frame f0 + p%16, chunk p/16)
#pragma unroll
    for (int k = 0; k < NCH * 16 / 256; ++k) {
      const int p = (k * 4 + wid) * 64 + lane;
      const int fr = min(f0 + (p & 15), B - 1), ch = p >> 4;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(coef_hl + (long)fr * 2 * Kp + ch * 8),
                                       (lds_void_t*)(base + (k * 4 + wid) * 1024), 16, 0, 0);
    }
    // rigid transforms of the 16 frames: contiguous in global memory
    {
      const int p = wid * 64 + lane;
      const long gofs = min((long)f0 * J * 12 + (long)p * 4, (long)B * J * 12 - 4);
      if (wid * 64 < A_CHUNKS)
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(A + gofs), (lds_void_t*)(base + COEF_BYTES + wid * 1024), 16, 0, 0);
    }
  };

  int stage = 0;
  issue(f_begin, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first tile: nothing younger than the loads yet
  // a wave issues exactly 4 vertex-store instructions per tile unless ALL its vertices are padding
  const bool wave_stores = __builtin_amdgcn_readfirstlane(wg.v_tile * 64 + wid * 16) < V;
  for (int f0 = f_begin; f0 < f_end; f0 += 16) {
    // vmcnt counts stores too: waiting for 0 would serialise on the previous tile's vertex stores (the 4 youngest
    // VMEM ops of this wave).  Leave them in flight and wait only for this tile's 4 LDS-DMA loads, which are older.
    if (wave_stores) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (f0 + 16 < f_end) issue(f0 + 16, stage ^ 1);
    const unsigned char* sc = smem + stage * STAGE;
    const float* sA = (const float*)(sc + COEF_BYTES);
    f32x4 acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const u32x4*)(sc + tile_coef_off(0, 4 * g + q, i)));
      const bf16x8 al = __builtin_bit_cast(bf16x8, *(const u32x4*)(sc + tile_coef_off(1, 4 * g + q, i)));
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = mma_bf16x3(acc[c], ah, al, dh[c][g], dl[c][g]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int fl = 4 * q + e, f = f0 + fl;
      float T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const f32x4* ap = (const f32x4*)(sA + (fl * J + j) * 12);
        const f32x4 a0 = ap[0], a1 = ap[1], a2 = ap[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          T[k] = fmaf(w[j], a0[k], T[k]);
          T[4 + k] = fmaf(w[j], a1[k], T[4 + k]);
          T[8 + k] = fmaf(w[j], a2[k], T[8 + k]);
        }
      }
      const float px = t3[0] + acc[0][e], py = t3[1] + acc[1][e], pz = t3[2] + acc[2][e];
      if (f < f_end && v < V) {
        // (T_c0 px + T_c2 pz) + (T_c1 py + T_c3): the pairing this kernel has had since it summed two-wide vectors; the
        // recorded output bits (tests/test_skin_bits_gpu.py) hold it to that order
        F3 o;
        o.x = fmaf(T[0], px, T[2] * pz) + fmaf(T[1], py, T[3] * 1.0f);
        o.y = fmaf(T[4], px, T[6] * pz) + fmaf(T[5], py, T[7] * 1.0f);
        o.z = fmaf(T[8], px, T[10] * pz) + fmaf(T[9], py, T[11] * 1.0f);
        *(F3*)(verts + ((long)f * V + v) * 3) = o;  // one 12-byte store per lane: 16 lanes = 192 contiguous bytes
      }
    }
    stage ^= 1;
  }
}

extern "C" int msmd_lbs_skin_bf16x3(const void* coef_hl, const float* A, const float* v_template, const void* dirs_hl,
                                    const float* lbs_weights, float* verts, int B, int J, int V, int Vp, int Kp, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || Vp < V || (Vp & 63) || J != LBS_J || Kp != LBS_KP) return 1;
  const int vt = Vp / 64;
  const SkinPlan plan = skin_plan(B, vt, 2048);
  dim3 grid(((vt + 7) / 8) * 8 * plan.splits), block(256);
  hipLaunchKernelGGL((lbs_skin_bf16x3_kernel<LBS_KP / 32, LBS_J>), grid, block, 0, (hipStream_t)stream, (const bf16_t*)coef_hl, A,
                     v_template, (const bf16_t*)dirs_hl, lbs_weights, verts, B, V, Vp, plan.fpb);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
// Skinning, second form (msmd_lbs_skin_v2): the per-(vertex, frame) blend  T = sum_j w_j A_j  moves from the vector
// ALU (60 FMAs + 60 broadcast LDS reads per lane and frame: the epilogue that bounded lbs_skin_bf16x3 at ~20 % of HBM)
// onto the matrix pipe.  For component m of the 3x4 transforms, T_m(frame, vertex) = sum_j A_j[m](frame) w_j(vertex) is
// a contraction over the FIVE joints: with both sides split into fp16 hi + lo it is 15 K slots of ONE
// v_mfma_f32_16x16x32_f16 (frame-side rows [Ah | Al | Ah] written by tile_put_blend, vertex-side column [wh | wh | wl] held
// in one VGPR quad), whose accumulator lands exactly where the blendshape product puts p(vertex, frame): vertex on the
// lane, frames 4q + e in the registers.  12 MFMAs replace ~240 vector instructions per 16 x 16 tile; what is left on
// the vector ALU is out_c = T_c0 px + T_c1 py + T_c2 pz + T_c3 (36 FMAs per lane and tile).
// Workgroup = NWV waves = 16 NWV vertices (their `dirs` planes in registers, 144 VGPRs, as before); frame tiles of 16
// arrive by LDS-DMA through an NS-deep ring (coefficients 12 KB + blend rows 6 KB per tile = 18 one-KiB pieces dealt
// round-robin to the waves) behind counted vmcnt waits that leave younger tiles' loads AND the vertex stores in flight.
// Stores: 12 bytes (x, y, z of the lane's vertex) per lane and frame, 16 lanes = 192 contiguous bytes.  (Turning each
// wave's 16 x 48 floats through an LDS patch into plain dword stores of whole row slices was built and measured: the
// 28 extra LDS instructions per lane and tile cost more than the narrower stores saved, 765 vs 695 us at 25 600 frames.)
// No lane is ever masked: padding vertices (v >= V) and padding frames (f >= B) recompute and re-store vertex V - 1 (OUT16:
// the last vertex pair) / frame B - 1 (identical bytes), so every wave issues exactly 4 store instructions per tile and the
// vmcnt arithmetic is uniform.
template <int N> __device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void vm_wait_n(int n) {   // n = (pieces per load group) a + (stores per tile) b, see the kernel
#define VMW(k) case k: vm_wait<k>(); break;
  switch (n) {
    VMW(1) VMW(2) VMW(3) VMW(4) VMW(5) VMW(6) VMW(7) VMW(8) VMW(9) VMW(10) VMW(11) VMW(12) VMW(13) VMW(14) VMW(15) VMW(16)
    VMW(17) VMW(18) VMW(19) VMW(20) VMW(21) VMW(22) VMW(23) VMW(24) VMW(25) VMW(26) VMW(27) VMW(28) VMW(29) VMW(30) VMW(31)
    VMW(32) VMW(33) VMW(34) VMW(35) VMW(36) VMW(37) VMW(38) VMW(39) VMW(40)
    default: vm_wait<0>(); break;
  }
#undef VMW
}

// NWV waves per workgroup (16 vertices each).
// WP: also store the un-skinned vertices p = template + coef . dirs (B, V, 3) -- what the backward of the skinning needs
// (training through the vertex-space loss); 8 instead of 4 store instructions per tile and wave.
// (Whole-row stores through an LDS image of the tile -- every wave puts its 16 x 16 x 3 results into [16 frames][128 vertices
// x 3] and, one barrier later, the waves write the image out as three wave-wide 16-byte stores of whole 1 536-byte rows, the
// shape that reaches 3.80 instead of 2.99 TB/s as a PURE store stream -- were built again in round 5 with the image double
// buffered on the tile loop's own barrier: 0.703 ms against 0.592 at 25 600 frames, same box, alternating.  The image costs
// 12 LDS writes + 3 reads per lane and tile and ties the waves to one barrier per tile, i.e. it removes the drift between the
// waves that the two-tiles-per-barrier schedule below lives on; the store shape is not what is left to win here.)
// OUT16 (msmd_lbs_skin_v2_f16, round 6): fp16 vertices in rows of V_ld (even, >= V) vertices -- the kernel is bound by its store
// stream, this halves it.  Lanes 2 p and 2 p + 1 (vertices v, v + 1) trade two frames each by DPP so that every lane stores the
// 12 contiguous bytes [x y z x y z] of its vertex PAIR for two of the tile's four frames: 2 store instructions of 96-byte runs
// per 8 lanes instead of 4 of 192-byte runs per 16.  (V = 5023 is odd: a row of V * 3 halves would put every other frame on a
// 2-byte boundary; hence the padded row.  Slot V of a row receives a copy of vertex V - 1.)
// F16P (with OUT16; msmd_lbs_skin_v2_f16's default form): fp16 vertices do not need 16-bit-split operands -- the blendshape
// product runs on ONE fp16 plane of `dirs` (72 registers instead of 144) and ONE fp16 coefficient plane (the 12 KB tile
// records written by msmd_lbs_tiles_f16): 1 MFMA per K group and coordinate instead of 3.  The operands' own rounding
// (2^-12 relative on offsets of <= ~0.03) stays under the fp16 step of the stored vertex.
template <int KG, int NS, int NWV, bool WP = false, int RB = 0, bool OUT16 = false, bool F16P = false>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(2, 2)))
void lbs_skin_v2_kernel(const unsigned char* __restrict__ tiles, const float* __restrict__ tmpl, const bf16_t* __restrict__ dirs_hl,
                        const float* __restrict__ wts, float* __restrict__ verts, int B, int V, int Vp,
                        int frames_per_block, int vtn, float* __restrict__ vposed = nullptr, int xcd_adj = 0,
                        const int* __restrict__ shape_varies = nullptr, const float* __restrict__ tmpl_folded = nullptr, int V_ld = 0) {
  static_assert(!(OUT16 && WP), "the training form stores fp32");
  constexpr int SPT = WP ? 8 : (OUT16 ? 2 : 4);   // store instructions per tile and wave
  // all frames share their first LBS_KFOLD shape coefficients (msmd_flame_prepare): folded template, skip those K groups
  const bool uni = shape_varies != nullptr && tmpl_folded != nullptr && *shape_varies == 0;
  const int g_first = uni ? LBS_KFOLD / 32 : 0;
  if (uni) tmpl = tmpl_folded;
  static_assert(!F16P || OUT16, "the single-plane form is for fp16 vertices");
  static_assert(KG * 32 == LBS_KP, "the ring holds whole tile records");
  constexpr int J = LBS_J, VPB = 16 * NWV;
  constexpr int COEF_BYTES = F16P ? LBS_TILE_COEF16_BYTES : LBS_TILE_COEF_BYTES;
  constexpr int STAGE = F16P ? LBS_TILE16_BYTES : LBS_TILE_BYTES;
  constexpr int NP = STAGE / 1024;           // 18 (F16P: 12) one-KiB LDS-DMA pieces per tile
  static_assert(STAGE % 1024 == 0, "piece map below");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, q = lane >> 4;
  // xcd_adj = 1: each XCD owns ADJACENT vertex tiles, so the 128-byte lines two neighbouring tiles share in a frame row meet
  // in one L2 (554 vs 588 us at 25 600 frames against dealing the tiles one by one, xcd_adj = 0); every launch passes 1.  (The
  // argument stays: without it two instantiations came out with another scalar register count and a shuffled tail.)
  const SkinTile wg = xcd_skin_tile(blockIdx.x, (vtn + 7) >> 3, xcd_adj);
  const int v_tile = wg.v_tile;
  if (v_tile >= vtn) return;
  const int f_begin = wg.split * frames_per_block;
  if (f_begin >= B) return;
  const int f_end = min(B, f_begin + frames_per_block);
  const int ntiles = (f_end - f_begin + 15) >> 4;
  // padding lanes (v >= V) recompute vertex V - 1.  OUT16 stores a vertex PAIR at (ve & ~1): clamp the pair, not the lane, so a
  // pair made only of padding lanes holds [v(base), v(base + 1)] at the last valid pair's base and stores exactly that pair's
  // bytes.  (Clamping each lane to V - 1 put [v(V-1), v(V-1)] at slot V - 2 when V is even, racing the valid pair's store.)
  const int vu = v_tile * VPB + wid * 16 + i;
  const int ve = OUT16 ? min(min(vu & ~1, (V - 1) & ~1) + (vu & 1), V - 1) : min(vu, V - 1);

  u32x4 dh[3][KG], dl[3][F16P ? 1 : KG];     // F16P: dirs_hl points at the ONE fp16 plane (3, Kp / 8, Vp, 8)
  load_dirs<KG, F16P ? 1 : KG>(dirs_hl, Vp, q, ve, dh, dl);
  float t3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) t3[c] = tmpl[(long)c * Vp + ve];
  // vertex-side operand of the blend MFMA: K slots [wh_0..4 | wh_0..4 | wl_0..4 | 0 ...]; lane (i, q) holds slots 8q .. 8q+7
  u32x4 wB;
  {
    f16_t wh[J], wl[J];
#pragma unroll
    for (int j = 0; j < J; ++j) split_f16_hl(wts[(long)j * Vp + ve], wh[j], wl[j]);
    const f16_t z = (f16_t)0.f;
    const f16x8 s0 = f16x8{wh[0], wh[1], wh[2], wh[3], wh[4], wh[0], wh[1], wh[2]};
    const f16x8 s1 = f16x8{wh[3], wh[4], wl[0], wl[1], wl[2], wl[3], wl[4], z};
    const f16x8 zz = f16x8{z, z, z, z, z, z, z, z};
    wB = __builtin_bit_cast(u32x4, q == 0 ? s0 : (q == 1 ? s1 : zz));
  }

  // piece k of a tile -> wave k % NWV; a wave stages pieces wid, wid + NWV, ... (my_np of them: the vmcnt unit)
  const int my_np = (NP - wid + NWV - 1) / NWV;
  auto issue = [&](int t) {   // one tile record = NP contiguous one-KiB LDS-DMA pieces
    unsigned char* base = smem + (t % NS) * STAGE;
    const unsigned char* src = tiles + (long)((f_begin >> 4) + t) * STAGE + lane * 16;
#pragma unroll
    for (int r = 0; r < (NP + NWV - 1) / NWV; ++r) {
      const int k = wid + NWV * r;
      if (k < NP) __builtin_amdgcn_global_load_lds((gbl_void_t*)(src + k * 1024), (lds_void_t*)(base + k * 1024), 16, 0, 0);
    }
  };

  auto do_tile = [&](int t) {
    const unsigned char* sc = smem + (t % NS) * STAGE;
    const unsigned char* sat = sc + COEF_BYTES;
    const int f0 = f_begin + 16 * t;

    f32x4 accp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) accp[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      if (g < g_first) continue;   // wave-uniform
      const u32x4 a0 = *(const u32x4*)(sc + tile_coef_off(0, 4 * g + q, i));
      if constexpr (F16P) {
#pragma unroll
        for (int c = 0; c < 3; ++c) accp[c] = mfma16<f16_t>(a0, dh[c][g], accp[c]);
      } else {
        const bf16x8 ah = __builtin_bit_cast(bf16x8, a0);
        const bf16x8 al = __builtin_bit_cast(bf16x8, *(const u32x4*)(sc + tile_coef_off(1, 4 * g + q, i)));
#pragma unroll
        for (int c = 0; c < 3; ++c) accp[c] = mma_bf16x3(accp[c], ah, al, dh[c][g], dl[c][g]);
      }
    }
    float px[4], py[4], pz[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { px[e] = t3[0] + accp[0][e]; py[e] = t3[1] + accp[1][e]; pz[e] = t3[2] + accp[2][e]; }
    float out[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4 T[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // K slots 16 .. 31 are zero on the vertex side (wB), so lanes q >= 2 may feed any finite values: they re-read
        // octet q & 1 (no divergent branch, no select)
        const u32x4 fa = *(const u32x4*)(sat + tile_blend_off(4 * c + k, q & 1, i));
        T[k] = mfma16<f16_t>(fa, wB, f32x4{0.f, 0.f, 0.f, 0.f});
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) out[c][e] = fmaf(T[0][e], px[e], fmaf(T[1][e], py[e], fmaf(T[2][e], pz[e], T[3][e])));
    }
    if constexpr (OUT16) {
      // even lane keeps frames e = 0, 1 and gives 2, 3; odd lane the other way round; lower vertex of the pair = the even lane's
      const bool oddl = i & 1;
      auto swap1 = [](float x) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, false)); };
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float own[3], got[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          own[c] = oddl ? out[c][2 + s2] : out[c][s2];
          got[c] = swap1(oddl ? out[c][s2] : out[c][2 + s2]);
        }
        const float lo0 = oddl ? got[0] : own[0], lo1 = oddl ? got[1] : own[1], lo2 = oddl ? got[2] : own[2];
        const float up0 = oddl ? own[0] : got[0], up1 = oddl ? own[1] : got[1], up2 = oddl ? own[2] : got[2];
        struct __attribute__((aligned(4))) U3 { unsigned a, b, c; };
        U3 o;
        asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(o.a) : "v"(lo0), "v"(lo1));
        asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(o.b) : "v"(lo2), "v"(up0));
        asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(o.c) : "v"(up1), "v"(up2));
        const int f = min(f0 + 4 * q + (oddl ? 2 : 0) + s2, B - 1);
        *(U3*)((f16_t*)verts + ((long)f * V_ld + (ve & ~1)) * 3) = o;   // 8 lanes = 96 contiguous bytes per frame
      }
      return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = min(f0 + 4 * q + e, B - 1);
      F3 o;
      o.x = out[0][e]; o.y = out[1][e]; o.z = out[2][e];
      *(F3*)(verts + ((long)f * V + ve) * 3) = o;   // 16 lanes = 192 contiguous bytes per frame
      if constexpr (WP) {
        F3 pp;
        pp.x = px[e]; pp.y = py[e]; pp.z = pz[e];
        *(F3*)(vposed + ((long)f * V + ve) * 3) = pp;
      }
    }
  };

  if constexpr (RB == 0) {
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
      if (s < ntiles) issue(s);
    for (int t = 0; t < ntiles; ++t) {
      // ops younger than tile t's loads, in issue order: min(NS-2, ntiles-1-t) load groups (my_np each) and
      // min(NS-1, t) store groups (SPT each)
      vm_wait_n(my_np * min(NS - 2, ntiles - 1 - t) + SPT * min(NS - 1, t));
      __builtin_amdgcn_s_barrier();
      if (t + NS - 1 < ntiles) issue(t + NS - 1);
      do_tile(t);
    }
  } else {
    // One workgroup barrier per RB tiles (NS = 2 RB slots: the group being read and the group in flight): between
    // barriers the waves drift apart, so one wave's vector / store phase can run under its SIMD partner's MFMA phase
    // instead of all eight waves meeting the matrix pipe, then the store path, in lockstep; s_setprio on half the waves
    // keeps the pairs apart.  770 -> 690 us at 25 600 frames.
    static_assert(RB == 0 || NS == 2 * RB, "ring = two barrier groups");
    const int ngroups = (ntiles + RB - 1) / RB;
    if (wid >= NWV / 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int r = 0; r < RB; ++r)
      if (r < ntiles) issue(r);
    for (int g = 0; g < ngroups; ++g) {
      // younger than group g's loads: the stores of group g-1's RB tiles
      if (g == 0) vm_wait<0>(); else vm_wait_n(SPT * RB);
      __builtin_amdgcn_s_barrier();
      if (g + 1 < ngroups) {
#pragma unroll
        for (int r = 0; r < RB; ++r)
          if ((g + 1) * RB + r < ntiles) issue((g + 1) * RB + r);
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int t = g * RB + r;
        if (t < ntiles) do_tile(t);
      }
    }
  }
}

static int lbs_skin_v2_impl(const void* skin_tiles, const float* v_template, const void* dirs_hl, const float* lbs_weights,
                            float* verts, float* vposed, int B, int J, int V, int Vp, int Kp, msmd_stream_t stream,
                            const int* shape_varies = nullptr, const float* tmpl_folded = nullptr, int V_ld16 = 0, bool single_plane = false) {
  if (B <= 0 || V <= 0 || Vp < V || J != LBS_J || Kp != LBS_KP || !skin_tiles) return 1;
  if (V_ld16 && (V_ld16 < V || (V_ld16 & 1) || vposed || ((uintptr_t)verts & 3))) return 1;
  // One 8-wave workgroup per CU (128 vertices, 4-stage ring).  Two 4-wave workgroups per CU (64 vertices each, 3-stage
  // rings) measured 783 vs 732 us at 25 600 frames: the smaller workgroups double the staged bytes per vertex and their
  // phase drift buys less than that costs.
  const int vt = (V + 127) / 128;
  const SkinPlan plan = skin_plan(B, vt, 1024);
  dim3 grid(((vt + 7) / 8) * 8 * plan.splits);
  // every form: 8 waves, 4-stage ring of whole tile records; the template arguments after NWV are (WP, RB, OUT16, F16P)
  auto launch = [&](auto kfn, int tile_bytes) {
    const int lds = 4 * tile_bytes;
    (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(kfn, grid, dim3(512), lds, (hipStream_t)stream, (const unsigned char*)skin_tiles, v_template,
                       (const bf16_t*)dirs_hl, lbs_weights, verts, B, V, Vp, plan.fpb, vt, vposed, /* xcd_adj */ 1, shape_varies,
                       tmpl_folded, V_ld16);
  };
  constexpr int KG = LBS_KP / 32;
  if (vposed) {
    launch(lbs_skin_v2_kernel<KG, 4, 8, true>, LBS_TILE_BYTES);
  } else if (V_ld16 && single_plane) {
    // (143 registers.  Twelve-wave workgroups of 192 vertices at three waves per SIMD measured the same as these eight-wave ones:
    // 0.387-0.392 against 0.388-0.394 ms at 25 600 frames; two 8-wave workgroups per CU need 128 registers and spilled 24 bytes
    // into the counted-vmcnt loop.)
    launch(lbs_skin_v2_kernel<KG, 4, 8, false, 2, true, true>, LBS_TILE16_BYTES);
  } else if (V_ld16) {
    launch(lbs_skin_v2_kernel<KG, 4, 8, false, 2, true>, LBS_TILE_BYTES);
  } else {
    launch(lbs_skin_v2_kernel<KG, 4, 8, false, 2>, LBS_TILE_BYTES);   // one barrier per two tiles + wave priorities
  }
  MSMD_RETURN_LAST();
}

extern "C" int msmd_lbs_skin_v2(const void* skin_tiles, const float* v_template, const void* dirs_hl,
                                const float* lbs_weights, float* verts, int B, int J, int V, int Vp, int Kp,
                                const int* shape_varies, const float* v_template_folded, msmd_stream_t stream) {
  return lbs_skin_v2_impl(skin_tiles, v_template, dirs_hl, lbs_weights, verts, nullptr, B, J, V, Vp, Kp, stream,
                          shape_varies, v_template_folded);
}

extern "C" int msmd_lbs_skin_v2_f16(const void* skin_tiles, const float* v_template, const void* dirs, const float* lbs_weights,
                                    void* verts16, int B, int J, int V, int V_ld, int Vp, int Kp, const int* shape_varies,
                                    const float* v_template_folded, int single_plane, msmd_stream_t stream) {
  if (V_ld <= 0) return 1;
  return lbs_skin_v2_impl(skin_tiles, v_template, dirs, lbs_weights, (float*)verts16, nullptr, B, J, V, Vp, Kp, stream,
                          shape_varies, v_template_folded, V_ld, single_plane != 0);
}

// Training form: the same kernel, additionally writing the un-skinned vertices v_posed (B, V, 3) for msmd_lbs_skin_bwd.
extern "C" int msmd_lbs_skin_v2_train(const void* skin_tiles, const float* v_template, const void* dirs_hl, const float* lbs_weights,
                                      float* verts, float* v_posed, int B, int J, int V, int Vp, int Kp, msmd_stream_t stream) {
  if (!v_posed) return 1;
  return lbs_skin_v2_impl(skin_tiles, v_template, dirs_hl, lbs_weights, verts, v_posed, B, J, V, Vp, Kp, stream);
}

// The split tile records -> the records of the single-plane fp16 form: coefficients hi + lo as ONE fp16 number in the same
// chunk order, then the blend rows unchanged.  One workgroup per tile.
__global__ __launch_bounds__(256) void lbs_tiles_f16_kernel(const unsigned char* __restrict__ tiles, unsigned char* __restrict__ out) {
  const unsigned char* src = tiles + (long)blockIdx.x * LBS_TILE_BYTES;
  unsigned char* dst = out + (long)blockIdx.x * LBS_TILE16_BYTES;
  // chunk by chunk (16 bytes = 8 coefficients of one frame): every plane orders its chunks alike
  for (int id = threadIdx.x; id < LBS_TILE_COEF16_BYTES / 16; id += 256) {
    const bf16x8 h = *(const bf16x8*)(src + tile_coef_off(0, 0, 0) + id * 16), l = *(const bf16x8*)(src + tile_coef_off(1, 0, 0) + id * 16);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16_t)((float)h[e] + (float)l[e]);
    *(f16x8*)(dst + tile_coef_off(0, 0, 0) + id * 16) = o;
  }
  for (int id = threadIdx.x; id < LBS_TILE_BLEND_BYTES / 16; id += 256)
    *(u32x4*)(dst + LBS_TILE_COEF16_BYTES + id * 16) = *(const u32x4*)(src + LBS_TILE_COEF_BYTES + id * 16);
}

extern "C" int msmd_lbs_tiles_f16(const void* skin_tiles, void* tiles16, int B, msmd_stream_t stream) {
  if (B <= 0 || !skin_tiles || !tiles16 || ((uintptr_t)skin_tiles & 15) || ((uintptr_t)tiles16 & 15)) return 1;
  hipLaunchKernelGGL(lbs_tiles_f16_kernel, dim3((B + LBS_FPB - 1) / LBS_FPB), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)skin_tiles, (unsigned char*)tiles16);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
// (coef (B, Kp), A (B, 5, 12)) fp32 -> the skinning kernels' operand formats: coef_hl (B, 2, Kp) bf16 hi / lo and the tile
// records.  For per-frame kinematics that do not come from msmd_lbs_prepare: the differentiable FLAME pass computes them with
// autograd on (B, 5, 3, 3)-sized tensors.
__global__ __launch_bounds__(256) void lbs_pack_kernel(const float* __restrict__ coef, const float* __restrict__ A,
                                                       bf16_t* __restrict__ coef_hl, unsigned char* __restrict__ tiles,
                                                       int B, int Kp) {
  const int fl = threadIdx.x >> 4, ln = threadIdx.x & 15;
  const int b = blockIdx.x * LBS_FPB + fl;
  const bool valid = b < B;
  const int bb = valid ? b : B - 1;
  unsigned char* tile = tiles + (long)blockIdx.x * LBS_TILE_BYTES;
  for (int k = ln; k < Kp; k += 16) {
    bf16_t hi, lo;
    split_bf16_hl(coef[(long)bb * Kp + k], hi, lo);
    if (valid && coef_hl) coef_hl_put(coef_hl, b, Kp, k, hi, lo);
    tile_put_coef(tile, fl, k, hi, lo);
  }
  tile_put_blend(tile, fl, ln, [&](int j, int m) { return A[((long)bb * LBS_J + j) * 12 + m]; });
}

extern "C" int msmd_lbs_pack(const float* coef, const float* A, void* coef_hl, void* at_tiles, int B, int Kp,
                             msmd_stream_t stream) {
  if (B <= 0 || Kp != LBS_KP || !coef || !A || !at_tiles) return 1;
  hipLaunchKernelGGL(lbs_pack_kernel, dim3((B + LBS_FPB - 1) / LBS_FPB), dim3(256), 0, (hipStream_t)stream, coef, A, (bf16_t*)coef_hl,
                     (unsigned char*)at_tiles, B, Kp);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
// Backward of the skinning  v = sum_j w_j (R_j p + t_j),  p = template + coef . dirs  (reference utils/lbs.py:185-221
// differentiated; the reference gets this from autograd through its materialised (B, V, 4, 4) transforms).  Given
// g = dL/dv (B, V, 3) and the forward's p (B, V, 3):
//   dp(b, v)      = (sum_j w_j R_j)^T g                       -> written as coordinate planes (B, 3, Vp) = the A operand of
//                                                                 the contraction  dcoef = dp . dirs^T  (msmd_gemm)
//   dA(b, j, r, :) = sum_v w_j(v) g_r(v) [p(v) ; 1]            -> (B, 5, 12), reduced over the vertices in registers
// One wave per frame: a lane walks vertices lane, lane + 64, ... (768 contiguous bytes per wave-load of g and p), keeps
// the 60 partial sums of dA in registers and folds them across the wave once at the end.
__global__ __launch_bounds__(64) void lbs_skin_bwd_kernel(const float* __restrict__ gverts, const float* __restrict__ vposed,
                                                          const float* __restrict__ A, const float* __restrict__ wts,
                                                          float* __restrict__ dp, float* __restrict__ dA, int V, int Vp) {
  const int b = blockIdx.x, lane = threadIdx.x;
  __shared__ float sA[60];
  if (lane < 60) sA[lane] = A[(long)b * 60 + lane];
  __syncthreads();
  float acc[5][12];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[j][k] = 0.f;
  float* dpb = dp + (long)b * 3 * Vp;
  for (int v = lane; v < Vp; v += 64) {
    float dpx = 0.f, dpy = 0.f, dpz = 0.f;
    if (v < V) {
      const float* gp = gverts + ((long)b * V + v) * 3;
      const float* pp = vposed + ((long)b * V + v) * 3;
      const float g[3] = {gp[0], gp[1], gp[2]};
      const float ph[4] = {pp[0], pp[1], pp[2], 1.0f};
      float R[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const float w = wts[(long)j * Vp + v];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) R[r * 3 + c] = fmaf(w, sA[j * 12 + r * 4 + c], R[r * 3 + c]);
          const float wg = w * g[r];
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[j][r * 4 + c] = fmaf(wg, ph[c], acc[j][r * 4 + c]);
        }
      }
      dpx = R[0] * g[0] + R[3] * g[1] + R[6] * g[2];
      dpy = R[1] * g[0] + R[4] * g[1] + R[7] * g[2];
      dpz = R[2] * g[0] + R[5] * g[1] + R[8] * g[2];
    }
    dpb[v] = dpx;                 // padding vertices: zeros (the contraction runs over Vp)
    dpb[Vp + v] = dpy;
    dpb[2 * Vp + v] = dpz;
  }
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const float t = wave_sum(acc[j][k]);
      if (lane == 0) dA[(long)b * 60 + j * 12 + k] = t;
    }
}

extern "C" int msmd_lbs_skin_bwd(const float* grad_verts, const float* v_posed, const float* A, const float* lbs_weights,
                                 float* dp_planes, float* dA, int B, int J, int V, int Vp, msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || Vp < V || J != 5 || !grad_verts || !v_posed || !A || !dp_planes || !dA) return 1;
  hipLaunchKernelGGL(lbs_skin_bwd_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, grad_verts, v_posed, A, lbs_weights,
                     dp_planes, dA, V, Vp);
  MSMD_RETURN_LAST();
}
