// What the JPEG encoder (jpeg.hip) and decoder (jpeg_decode.hip, 5.24) share.  The decoder is exact because its
// matrix and its scan order are the encoder's, so each is typed once, here.
#pragma once
#include "common.h"

namespace {

#define JPEG_DCT_S 15   // DCT matrix scale
#define JPEG_ROW 9      // LDS row pitch of a staged 8 x 8 block, in elements: rows and columns both conflict-free
// not (1 <= H, W <= MSMD_JPEG_MAX_SIDE); four compares and no branch
__device__ __host__ __forceinline__ bool jpeg_sides_bad(int H, int W) { return (H < 1) | (W < 1) | (H > MSMD_JPEG_MAX_SIDE) | (W > MSMD_JPEG_MAX_SIDE); }

// The zig-zag scan (T.81 figure A.6): position in the scan -> natural index (row * 8 + column); inverse() gives the other direction.
struct alignas(16) Perm64 { unsigned char v[64]; };
constexpr Perm64 kZz2Nat = {{0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}};
constexpr Perm64 inverse(const Perm64 p) {
  Perm64 q{};
  for (int i = 0; i < 64; ++i) q.v[p.v[i]] = (unsigned char)i;
  return q;
}
constexpr bool composes_to_identity(const Perm64 a, const Perm64 b) {   // a[b[i]] = i for all i: both are bijections, each the other's inverse
  for (int i = 0; i < 64; ++i) if (a.v[b.v[i]] != i) return false;
  return true;
}
static_assert(composes_to_identity(inverse(kZz2Nat), kZz2Nat), "the zig-zag table is no permutation of 0 .. 63");

// M[k][n] = rint(2^15 c_k cos((2 n + 1) k pi / 16)) for n < 4; M[k][7 - n] = (-1)^k M[k][n] holds for the rounded integers too.
// |M| <= 16069; a row's absolute sum is <= 92680, a column's 86567.
__device__ constexpr int kM[8][4] = {{11585, 11585, 11585, 11585},   {16069, 13623, 9102, 3196},   {15137, 6270, -6270, -15137},
                                     {13623, -3196, -16069, -9102}, {11585, -11585, -11585, 11585}, {9102, -16069, 3196, 13623},
                                     {6270, -15137, 15137, -6270},  {3196, -9102, 13623, -16069}};

// One 8-point pass with the even / odd split (the same integers as the plain matrix product: integer sums re-associate).
template <typename Acc> __device__ __forceinline__ void dct8(const int* x, Acc* out) {
  int s[4], d[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) { s[n] = x[n] + x[7 - n]; d[n] = x[n] - x[7 - n]; }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    Acc a = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) a += (Acc)kM[k][n] * (Acc)((k & 1) ? d[n] : s[n]);
    out[k] = a;
  }
}
// One 8-point pass of x = M^T F with the even / odd split: out[n] = e[n] + o[n], out[7 - n] = e[n] - o[n], e over the even k, o
// over the odd ones (the same integers as the plain product: integer sums re-associate).
template <typename In> __device__ __forceinline__ void idct8(const In* f, long* out) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    long e = 0, o = 0;
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      e += (long)kM[k][n] * (long)f[k];
      o += (long)kM[k + 1][n] * (long)f[k + 1];
    }
    out[n] = e + o;
    out[7 - n] = e - o;
  }
}

}  // namespace
