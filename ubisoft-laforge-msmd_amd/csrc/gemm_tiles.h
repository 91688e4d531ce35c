// LDS tile layout and the LDS-DMA operand ring of the GEMM kernels (gemm.hip; the typedefs and the ring step also serve gemm_tn.hip
// and pos_conv.hip, the row swizzle also attention.hip).  What needs GemmArgs -- tile order, operand sources, epilogues -- is the
// "shared pieces" section of gemm.hip.
#pragma once
#include "common.h"

// the two pointer operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

// 128-byte rows (64 16-bit / 32 fp32 elements): 16-byte chunk `chunk` (0..7) of `row`, chunks XOR (row >> 1) & 7, so the
// ds_read_b128 of 16 consecutive rows at one logical chunk is conflict-free (MI355X_MICROARCH.md, LDS table)
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// Where a lane's fragments sit in a BM x BN tile of WM x WN waves: the wave's first row / column, and the lane's row (fr) and
// 4-column group (fq) inside every 16 x 16 fragment.
struct FragLane { int wm, wn, fr, fq; };
template <int BM, int BN, int WM, int WN> __device__ __forceinline__ FragLane frag_lane(int tid) {
  return {((tid >> 6) / WN) * (BM / WM), ((tid >> 6) % WN) * (BN / WN), tid & 15, (tid & 63) >> 4};
}
// a copy of a thread id the compiler cannot match with the original: what is derived from it is derived AGAIN, not kept in
// registers from the first derivation (the callers say what that saved them)
__device__ __forceinline__ int opaque_tid(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}

template <int FM, int FN> __device__ __forceinline__ void zero_acc(f32x4 (&acc)[FN][FM]) {
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// One step of an NSTAGE-deep LDS-DMA ring whose K tile is LPT wave-instructions per lane: the counted wait lets tile kt land and
// keeps the NSTAGE - 2 behind it in flight ACROSS the (single, raw) barrier; behind the barrier every wave has left the stage of
// tile kt - 1, which takes tile kt + NSTAGE - 1.  The caller multiplies stage `stage`, then stage = ring_next(stage).
template <int NSTAGE, int LPT, typename Issue>
__device__ __forceinline__ void ring_step(int kt, int nk, int stage, Issue&& issue) {
  if (kt + NSTAGE - 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 2) * LPT) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (kt + NSTAGE - 1 < nk) issue(kt + NSTAGE - 1, (stage + NSTAGE - 1) % NSTAGE);
}
template <int NSTAGE> __device__ __forceinline__ int ring_next(int stage) { return stage + 1 == NSTAGE ? 0 : stage + 1; }
