// LDS tile layouts of the attention kernels (attention.hip, attention_bwd.hip): byte offsets into [rows][64-element] images.
// Every function returns the offset of something 16-byte aligned unless it says otherwise; `ch` counts 16-byte chunks of a row.
#pragma once
#include "gemm_tiles.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---- 16-bit elements, 128-byte rows
// K image (row reads only): lds_off(row, ch) of gemm_tiles.h, the GEMM kernels' operand image
// V image, and every image of the backward (row reads AND transposed reads): chunk ch (0..7) of `row`; 32-byte blocks XOR
// (row >> 1) & 3, the two chunks of a block stay together
__device__ __forceinline__ int img_off(int row, int ch) { return row * 128 + (((((ch >> 1) ^ ((row >> 1) & 3)) << 1) | (ch & 1)) << 4); }
// the address a lane supplies for a transposed read of an img_off image: lane 4 q' + p' of each 16-lane group passes its row
// (r0 + q'), the 16-column block db (0..3) and pp = p' (8 bytes = 4 columns each)
__device__ __forceinline__ int img_tr(int row, int db, int pp) { return row * 128 + ((db ^ ((row >> 1) & 3)) << 5) + pp * 8; }
// ds_read_b64_tr_b16: the 16 lanes of a group exchange their 4 x 4 blocks; a lane gets 4 rows of ONE column
__device__ __forceinline__ u32x2 tr_read(const unsigned char* p) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p);
  return __builtin_bit_cast(u32x2, v);
}

// ---- 256-byte rows: split-pair storage [hi0 | lo0 | hi1 | lo1] (attn_split_kernel) and fp32 (attn_kernel<float>)
// K image: chunk ch (0..15) of `row`, chunks XOR row & 15 (conflict-free ds_read_b128)
__device__ __forceinline__ int k256_off(int row, int ch) { return row * 256 + ((ch ^ (row & 15)) << 4); }
// split V image: chunk ch (0..15) of `row`, chunks XOR the dual-use pattern that serves row writes and transposed reads
__device__ __forceinline__ int vsw(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int vsplit_off(int row, int ch) { return row * 256 + ((ch ^ vsw(row)) << 4); }
// fp32 V image: chunk ch (0..15) of `row`; rows padded to 68 floats (272 bytes) instead of a swizzle: the product reads single
// floats (ds_read_b32) at v32_off(row, 0) + 4 * column
__device__ __forceinline__ int v32_off(int row, int ch) { return row * 272 + (ch << 4); }
