// The skinning kernels' tile record (msmd_lbs_skin_v2's skin_tiles): one per 16 frames, read by contiguous one-KiB LDS-DMA
// pieces.  THE definition of its layout: the writers (lbs_prepare_kernel, lbs_pack_kernel), the converter (lbs_tiles_f16_kernel)
// and the readers (lbs_skin_bf16x3_kernel's LDS stage, lbs_skin_v2_kernel) go through the constants and offsets below.
//   split form, 18 432 bytes:  [coefficients bf16 hi | coefficients bf16 lo | blend rows]
//   fp16 form,  12 288 bytes:  [coefficients hi + lo as ONE fp16 plane | blend rows]
// A coefficient plane is chunk-major, [k / 8][frame % 16][k % 8]: one 16-byte chunk per (K octet, frame), the 16 frames of an
// octet contiguous -> conflict-free ds_read_b128 with the frame on the MFMA row.
// Blend rows (frame-side operand of the blend MFMA): for component m of the 3x4 transforms, 16 fp16 K slots per frame =
// [Ah_0..4 | Al_0..4 | Ah_0..4 | 0] (A = Ah + Al, unscaled: |A| = O(1), so the lo halves keep 2^-25 absolute), as
// [m][slot / 8][frame % 16][slot % 8].
// Frames beyond B - 1 of the last tile carry frame B - 1's values (the kernel clamps them to that frame: identical bytes).
#pragma once
#include "common.h"

#define LBS_FPB 16                                           // frames per tile
#define LBS_KP 192                                           // coefficients per frame, zero padded
#define LBS_J 5                                              // joints
#define LBS_KFOLD 96                                         // shape coefficients msmd_flame_prepare folds into the template
#define LBS_TILE_COEF_BYTES (2 * LBS_KP * LBS_FPB * 2)       // 12288: hi and lo planes
#define LBS_TILE_COEF16_BYTES (LBS_KP * LBS_FPB * 2)         // 6144: the single fp16 plane
#define LBS_TILE_BLEND_BYTES (12 * 16 * LBS_FPB * 2)         // 6144
#define LBS_TILE_BYTES (LBS_TILE_COEF_BYTES + LBS_TILE_BLEND_BYTES)       // 18432
#define LBS_TILE16_BYTES (LBS_TILE_COEF16_BYTES + LBS_TILE_BLEND_BYTES)   // 12288

// byte offset of the 16-byte coefficient chunk (plane 0 = hi or the fp16 plane, 1 = lo; K octet k8 = k / 8; frame % 16)
__host__ __device__ constexpr int tile_coef_off(int plane, int k8, int fl) { return ((plane * (LBS_KP / 8) + k8) * LBS_FPB + fl) * 16; }
// byte offset, from the start of the blend rows, of the 16-byte chunk (component m, slot octet, frame % 16)
__host__ __device__ constexpr int tile_blend_off(int m, int octet, int fl) { return ((m * 2 + octet) * LBS_FPB + fl) * 16; }

// v ~= hi + lo in two 16-bit numbers.  v is pinned to ONE register value first (see split_f16x2 in common.h): hi and the
// residual must come from the same fp32 number.
__device__ __forceinline__ void split_bf16_hl(float v, bf16_t& hi, bf16_t& lo) {
  asm volatile("" : "+v"(v));
  hi = (bf16_t)v;
  lo = (bf16_t)(v - (float)hi);
}
__device__ __forceinline__ void split_f16_hl(float v, f16_t& hi, f16_t& lo) {
  asm volatile("" : "+v"(v));
  hi = (f16_t)v;
  lo = (f16_t)(v - (float)hi);
}

// coefficient k of frame fl of the tile
__device__ __forceinline__ void tile_put_coef(unsigned char* tile, int fl, int k, bf16_t hi, bf16_t lo) {
  *(bf16_t*)(tile + tile_coef_off(0, k >> 3, fl) + (k & 7) * 2) = hi;
  *(bf16_t*)(tile + tile_coef_off(1, k >> 3, fl) + (k & 7) * 2) = lo;
}
// the same pair in the row-major coef_hl (B, 2, Kp) of msmd_lbs_skin_bf16x3
__device__ __forceinline__ void coef_hl_put(bf16_t* coef_hl, long b, int Kp, int k, bf16_t hi, bf16_t lo) {
  coef_hl[(b * 2 + 0) * Kp + k] = hi;
  coef_hl[(b * 2 + 1) * Kp + k] = lo;
}
// The blend rows of frame fl, written by the frame's 16 threads (ln = 0 .. 15); a_of(j, m) yields A_j[m] of that frame.
template <typename AOf> __device__ __forceinline__ void tile_put_blend(unsigned char* tile, int fl, int ln, AOf&& a_of) {
  for (int idx = ln; idx < 12 * 16; idx += 16) {
    const int m = idx >> 4, slot = idx & 15;
    f16_t ah, al;
    split_f16_hl(slot < 15 ? a_of(slot % LBS_J, m) : 0.f, ah, al);
    const f16_t val = slot >= 15 ? (f16_t)0.f : ((slot >= 5 && slot < 10) ? al : ah);
    *(f16_t*)(tile + LBS_TILE_COEF_BYTES + tile_blend_off(m, slot >> 3, fl) + (slot & 7) * 2) = val;
  }
}
