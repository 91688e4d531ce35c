// A float64 Cholesky factorisation and its two triangular solves for ONE WAVE, up to 64 x 64, shared by the per-frame solvers
// (expression_fit.hip, retarget.hip).
//
// The cyclic register layout: lane (ti, tj) = (lane >> 3, lane & 7) of an 8 x 8 grid holds M[8 a + ti][8 b + tj], a, b < 8, in
// acc[a][b].  The factorisation stays in that layout (right-looking: one column through LDS per step, 64 FMAs per lane per
// step); the factor goes to LDS packed by columns for the two triangular solves with one row per lane.  A wave's LDS traffic
// is ordered by the hardware, so inside a wave a fence suffices: no workgroup barrier in here.
#pragma once
#include "common.h"

constexpr int WCHOL_COL = 72;                        // doubles of per-wave LDS for the step's column (64) and pivot (1)
__host__ __device__ constexpr int wchol_packed(int NP) { return NP * (NP + 1) / 2; }   // doubles of per-wave LDS for the factor

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc (cyclic) = L L^T for its leading NP x NP part; L packed by columns into `sL`, its diagonal inverted; `col` is WCHOL_COL
// doubles of scratch.  -> false at the first pivot that is not positive (a NaN included); the factor is then not to be used.
__device__ __forceinline__ bool wave_cholesky(int lane, int NP, double* __restrict__ col, double* __restrict__ sL, double (&acc)[8][8]) {
  const int ti = lane >> 3, tj = lane & 7;
  bool ok = true;
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) {
    for (int jj = 0; jj < 8; ++jj) {
      const int j = jb * 8 + jj;
      if (j >= NP || !ok) break;
      if (ti == jj && tj == jj) col[64] = acc[jb][jb];
      wave_sync();
      const double d = col[64];
      if (!(d > 0.0)) { ok = false; break; }
      const double inv = 1.0 / sqrt(d);
      if (tj == jj) {
        const int off = j * NP - (j * (j - 1)) / 2 - j;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
          const int i = a * 8 + ti;
          const double v = i >= j ? acc[a][jb] * inv : 0.0;
          col[i] = v;
          if (i >= j && i < NP) sL[off + i] = i == j ? inv : v;      // the diagonal holds 1 / L_jj
        }
      }
      wave_sync();
      double la[8], lb[8];
#pragma unroll
      for (int a = 0; a < 8; ++a) { la[a] = col[a * 8 + ti]; lb[a] = col[a * 8 + tj]; }
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = fma(-la[a], lb[b], acc[a][b]);
    }
  }
  wave_sync();
  return ok;
}

// L L^T x = b with one row per lane, L as wave_cholesky packed it: -> x (lanes from NP on keep b).
__device__ __forceinline__ double wave_chol_solve(int lane, int NP, const double* __restrict__ sL, double b) {
  for (int j = 0; j < NP; ++j) {
    const int off = j * NP - (j * (j - 1)) / 2;
    const double z = __shfl(b, j, 64) * sL[off];
    if (lane == j) b = z;
    if (lane > j && lane < NP) b = fma(-sL[off + lane - j], z, b);
  }
  for (int j = NP - 1; j >= 0; --j) {
    const double z = __shfl(b, j, 64) * sL[j * NP - (j * (j - 1)) / 2];
    if (lane == j) b = z;
    if (lane < j) b = fma(-sL[lane * NP - (lane * (lane - 1)) / 2 + j - lane], z, b);
  }
  return b;
}
