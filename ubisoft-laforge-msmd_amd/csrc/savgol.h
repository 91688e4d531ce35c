// The Savitzky-Golay table of msmd_headpose_smooth and msmd_track_resample (include/msmd_hip.h): `window` interior
// coefficients, then the edge table (2 (window / 2), window) whose row r < window / 2 gives frame r from the clip's first
// `window` frames and whose row window / 2 + r gives frame F - window / 2 + r from its last `window`.
#pragma once
#include "common.h"

constexpr int SAVGOL_MAX_WINDOW = MSMD_HEADPOSE_MAX_WINDOW;
constexpr int SAVGOL_TABLE = SAVGOL_MAX_WINDOW * SAVGOL_MAX_WINDOW;      // doubles of LDS a kernel keeps for s_coef

static inline bool savgol_window_ok(int window) { return window >= 3 && window <= SAVGOL_MAX_WINDOW && (window & 1); }

// The copy of the table into LDS by a workgroup of WG threads; the caller's next barrier publishes it.
template <int WG>
__device__ __forceinline__ void savgol_stage(double* __restrict__ s_coef, const double* __restrict__ table, int window) {
  for (int i = threadIdx.x; i < window * window; i += WG) s_coef[i] = table[i];
}

// The coefficients of frame j of a clip of F >= window frames, and `first`, the clip frame of the window's first sample.
__device__ __forceinline__ const double* savgol_row(const double* __restrict__ s_coef, int window, int j, int F, int& first) {
  const int h = window >> 1;
  if (j < h) { first = 0; return s_coef + window + j * window; }
  if (j >= F - h) { first = F - window; return s_coef + window + (h + j - (F - h)) * window; }
  first = j - h;
  return s_coef;
}
