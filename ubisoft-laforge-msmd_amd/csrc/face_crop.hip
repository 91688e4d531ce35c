// Face crops for an expression encoder (reference dataset_processing/transform.py: crop_v2; Step3_preprocess_expression_code.py:
// crop_img and the ToTensor + Normalize behind it): a bilinear affine warp with a zero border, stated in
// float64 in include/msmd_hip.h, the channel swap and the normalisation as a 256-entry table per channel, in one launch.
#include "common.h"

// Every double operation of this file is rounded on its own: the operator's bytes are defined that way, and a multiply
// fused into the following add would move a value across a .5 tie.
#pragma clang fp contract(off)

constexpr int FC_WG = 256;
constexpr int FC_PIX = 4;             // consecutive pixels of an output row a lane owns

struct __attribute__((packed, aligned(4))) U3 { unsigned a, b, c; };   // 12 bytes of crop_u8: one dwordx3 store

// One output pixel's taps: the weights, which neighbours lie inside the frame, and the twelve bytes (channel, neighbour).
struct FcTap {
  double fx, fy;
  bool m00, m01, m10, m11;
  unsigned b[3][4];
};

// The taps of output pixel (j, i); a: the frame's inverse map.  No branch: all twelve bytes are loaded, from addresses clamped
// into the frame, and fc_finish makes a neighbour outside it 0 by a select.  (Written as conditional loads, every byte became
// a block of its own behind a wait for the one before, and the launch took twice as long.)
__device__ __forceinline__ void fc_load(const unsigned char* __restrict__ frame, long row_stride, int pixel_stride, int H, int W,
                                        const double* a, int j, int i, int swap_rb, FcTap& t) {
  const double sx = ((a[0] * (double)j) + (a[1] * (double)i)) + a[2];
  const double sy = ((a[3] * (double)j) + (a[4] * (double)i)) + a[5];
  const bool inside = sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H;  // false for NaN too
  const double tx = inside ? sx : 0.0, ty = inside ? sy : 0.0;                    // no integer is formed from a wild value
  const double fx0 = floor(tx), fy0 = floor(ty);
  t.fx = tx - fx0;
  t.fy = ty - fy0;
  const int x0 = (int)fx0, y0 = (int)fy0;                                          // in [-1, W - 1], [-1, H - 1]
  const bool xa = inside && x0 >= 0, xb = inside && x0 + 1 < W, ya = y0 >= 0, yb = y0 + 1 < H;
  t.m00 = ya && xa; t.m01 = ya && xb; t.m10 = yb && xa; t.m11 = yb && xb;
  const unsigned char* top_row = frame + (long)max(y0, 0) * row_stride;
  const unsigned char* bot_row = frame + (long)min(y0 + 1, H - 1) * row_stride;
  const long left = (long)max(x0, 0) * pixel_stride, right = (long)min(x0 + 1, W - 1) * pixel_stride;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sc = swap_rb ? 2 - c : c;
    t.b[c][0] = top_row[left + sc];
    t.b[c][1] = top_row[right + sc];
    t.b[c][2] = bot_row[left + sc];
    t.b[c][3] = bot_row[right + sc];
  }
}

// The bytes of the three output channels from a pixel's taps.
__device__ __forceinline__ void fc_finish(FcTap& t, unsigned* u8) {
  const double fx = t.fx, fy = t.fy, gx = 1.0 - fx, gy = 1.0 - fy;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // the loaded bytes pass through an empty asm: a select whose operand is a load itself is turned back into a branch
    // around that load late in the compiler
    asm("" : "+v"(t.b[c][0]), "+v"(t.b[c][1]), "+v"(t.b[c][2]), "+v"(t.b[c][3]));
    const double p00 = (double)(t.m00 ? t.b[c][0] : 0u);
    const double p01 = (double)(t.m01 ? t.b[c][1] : 0u);
    const double p10 = (double)(t.m10 ? t.b[c][2] : 0u);
    const double p11 = (double)(t.m11 ? t.b[c][3] : 0u);
    const double top = (p00 * gx) + (p01 * fx);
    const double bot = (p10 * gx) + (p11 * fx);
    const double v = (top * gy) + (bot * fy);
    const double r = floor(v + 0.5);
    u8[c] = r >= 255.0 ? 255u : (unsigned)(int)r;
  }
}

// One lane per FC_PIX consecutive pixels of an output row; the quads of a frame are numbered row by row and a workgroup takes
// FC_WG of them.  VEC: out_w % FC_PIX == 0 and the buffers are aligned for the wide stores (the launcher checks).
template <typename T, bool VEC>
__global__ __launch_bounds__(FC_WG) void face_crop_kernel(const unsigned char* __restrict__ frames, long frame_stride, long row_stride,
                                                          int pixel_stride, int H, int W, const double* __restrict__ inverse,
                                                          const float* __restrict__ table, int out_h, int out_w, int swap_rb,
                                                          T* __restrict__ out, unsigned char* __restrict__ crop, int blocks_per_frame) {
  __shared__ float s_table[3 * 256];
  for (int k = threadIdx.x; k < 3 * 256; k += FC_WG) s_table[k] = table[k];
  __syncthreads();
  const int f = blockIdx.x / blocks_per_frame;
  const int quads_per_row = (out_w + FC_PIX - 1) / FC_PIX;
  const int q = (blockIdx.x - f * blocks_per_frame) * FC_WG + threadIdx.x;
  if (q >= quads_per_row * out_h) return;
  const int i = q / quads_per_row, j0 = (q - i * quads_per_row) * FC_PIX;
  double a[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) a[k] = inverse[(long)f * 6 + k];
  const unsigned char* frame = frames + (long)f * frame_stride;
  FcTap tap[FC_PIX];
  unsigned u8[FC_PIX][3];
#pragma unroll
  for (int e = 0; e < FC_PIX; ++e)       // a pixel past the row's end is sampled too (its loads are in bounds) and not stored
    fc_load(frame, row_stride, pixel_stride, H, W, a, j0 + e, i, swap_rb, tap[e]);
#pragma unroll
  for (int e = 0; e < FC_PIX; ++e) fc_finish(tap[e], u8[e]);
  const long plane = (long)out_h * out_w, at = (long)i * out_w + j0;
  if (out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T* dst = out + ((long)f * 3 + c) * plane + at;
      const float* t = s_table + c * 256;
      if constexpr (VEC) {
        *(typename Vec4T<T>::type*)dst = pack4<T>(t[u8[0][c]], t[u8[1][c]], t[u8[2][c]], t[u8[3][c]]);
      } else {
#pragma unroll
        for (int e = 0; e < FC_PIX; ++e)
          if (j0 + e < out_w) dst[e] = from_f32<T>(t[u8[e][c]]);
      }
    }
  }
  if (crop) {
    unsigned char* dst = crop + ((long)f * plane + at) * 3;
    if constexpr (VEC) {
      // bytes b0 .. b11 = (pixel 0: c0 c1 c2) (pixel 1: ...) ..., little endian
      U3 w;
      w.a = u8[0][0] | u8[0][1] << 8 | u8[0][2] << 16 | u8[1][0] << 24;
      w.b = u8[1][1] | u8[1][2] << 8 | u8[2][0] << 16 | u8[2][1] << 24;
      w.c = u8[2][2] | u8[3][0] << 8 | u8[3][1] << 16 | u8[3][2] << 24;
      *(U3*)dst = w;
    } else {
#pragma unroll
      for (int e = 0; e < FC_PIX; ++e)
        if (j0 + e < out_w) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dst[e * 3 + c] = (unsigned char)u8[e][c];
        }
    }
  }
}

template <typename T, bool VEC>
static int face_crop_launch(const void* frames, long frame_stride, long row_stride, int pixel_stride, int F, int H, int W,
                            const double* inverse, const float* table, int out_h, int out_w, int swap_rb, void* out, void* crop,
                            int blocks_per_frame, hipStream_t st) {
  hipLaunchKernelGGL((face_crop_kernel<T, VEC>), dim3((unsigned)(F * blocks_per_frame)), dim3(FC_WG), 0, st,
                     (const unsigned char*)frames, frame_stride, row_stride, pixel_stride, H, W, inverse, table, out_h, out_w,
                     swap_rb, (T*)out, (unsigned char*)crop, blocks_per_frame);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_face_crop(const void* frames, long frame_stride, long row_stride, int pixel_stride, int F, int H, int W,
                              const double* inverse, const float* table, int out_h, int out_w, int swap_rb, void* out, int out_dtype,
                              void* crop_u8, msmd_stream_t stream) {
  if (!frames || !inverse || !table || (!out && !crop_u8) || F < 1) return 1;
  if (H < 1 || H > MSMD_JPEG_MAX_SIDE || W < 1 || W > MSMD_JPEG_MAX_SIDE) return 1;
  if (out_h < 1 || out_h > MSMD_CROP_MAX_SIDE || out_w < 1 || out_w > MSMD_CROP_MAX_SIDE) return 1;
  if (pixel_stride != 3 && pixel_stride != 4) return 1;
  // the last byte read of a row is its last pixel's third: rows and frames must not overlap
  if (row_stride < (long)(W - 1) * pixel_stride + 3) return 1;
  if (F > 1 && frame_stride < (long)(H - 1) * row_stride + (long)(W - 1) * pixel_stride + 3) return 1;
  const int quads = ((out_w + FC_PIX - 1) / FC_PIX) * out_h;
  const int blocks_per_frame = (quads + FC_WG - 1) / FC_WG;
  if ((long)F * blocks_per_frame > 2147483647L) return 1;
  hipStream_t st = (hipStream_t)stream;
  return dispatch_dtype<float, bf16_t, f16_t>(out_dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) T;
    const bool vec = out_w % FC_PIX == 0 && (uintptr_t)out % (FC_PIX * sizeof(T)) == 0 && (uintptr_t)crop_u8 % 4 == 0;
    return vec ? face_crop_launch<T, true>(frames, frame_stride, row_stride, pixel_stride, F, H, W, inverse, table, out_h, out_w,
                                           swap_rb, out, crop_u8, blocks_per_frame, st)
               : face_crop_launch<T, false>(frames, frame_stride, row_stride, pixel_stride, F, H, W, inverse, table, out_h, out_w,
                                            swap_rb, out, crop_u8, blocks_per_frame, st);
  });
}
