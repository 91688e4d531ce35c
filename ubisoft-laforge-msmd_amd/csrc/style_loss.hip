// Style losses (reference utils/common.py:29-91, 835-875): the style-adherence soft / hard minimum over the
// frames of a style clip, and the NT-Xent contrastive loss of the style encoder, each with its backward.
//
// Adherence: d[t, k] = mean_f (X[t, f] - S[k, f])^2 is formed from the DIFFERENCES in fp32 on the vector ALU, one (row, k)
// pair per accumulator, ascending f by fma.  A workgroup of 256 = 16 rows x 16 lanes; a lane owns k = j, j + 16, j + 32, j + 48 of
// each 64-frame style tile.  Tiles of X and S pass through LDS 64 features at a time, so F is unbounded.  Nothing of size
// T x K is written: the forward keeps a running (min, sum e, sum e d) per lane, and the backward recomputes d, w and c from the
// saved row statistic.  Every sum has one owner and one order that depends on (T, K, F) alone: no floating-point atomics.
#include "common.h"

#define ROWS MSMD_STYLE_ROWS
#define KT MSMD_STYLE_KTILE
#define FC MSMD_STYLE_FCHUNK
#define LDP (FC + 1)              // row pitch in LDS: lanes that read one column of 16 rows hit 16 banks
static_assert(ROWS == 16 && KT == 64 && FC == 64, "the thread maps below are written for 16 x 64 x 64 tiles");

struct StyleTiles {
  float xs[ROWS][LDP];
  float ss[KT][LDP];
};

// rows [row0, row0 + rows) x features [f0, f0 + FC) of a (row_end, F) matrix; zeros outside it
__device__ __forceinline__ void stage_rows(float (*dst)[LDP], int rows, const float* __restrict__ src, int row0, int row_end,
                                           int f0, int F) {
  for (int e = threadIdx.x; e < rows * FC; e += 256) {
    const int r = e / FC, f = e % FC;
    dst[r][f] = (row0 + r < row_end && f0 + f < F) ? src[(long)(row0 + r) * F + f0 + f] : 0.f;
  }
}

// d of the thread's four pairs: row t0 + (tid >> 4) against k0 + (tid & 15) + 16 i.  Leaves the LAST feature chunk of both
// tiles in LDS; with F <= FC that is the whole tile, and a caller that streams one side passes stage_x / stage_s = false for
// the side that is still resident.  The one place d is formed, so that forward and backward hold the same bits.
__device__ __forceinline__ void tile_distances(StyleTiles& sm, const float* __restrict__ xb, int t0, int T,
                                               const float* __restrict__ sb, int k0, int K, int F, bool stage_x, bool stage_s,
                                               float d[4]) {
  const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int f0 = 0; f0 < F; f0 += FC) {
    __syncthreads();
    if (stage_x) stage_rows(sm.xs, ROWS, xb, t0, T, f0, F);
    if (stage_s) stage_rows(sm.ss, KT, sb, k0, K, f0, F);
    __syncthreads();
    const int nf = min(FC, F - f0);
    for (int f = 0; f < nf; ++f) {
      const float x = sm.xs[r][f];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float diff = x - sm.ss[j + 16 * i][f];
        acc[i] = fmaf(diff, diff, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = acc[i] / (float)F;
}

// Running soft minimum: m = the smallest d so far (idx its first index, -1 = nothing yet), se = sum exp(-lambda (d - m)),
// sed = sum exp(-lambda (d - m)) d; both sums are rescaled when the minimum moves.
struct SoftMin { float m, se, sed; int idx; };

template <bool SOFT> __device__ __forceinline__ void softmin_push(SoftMin& s, float d, int k, float lambda) {
  if (s.idx < 0) {
    s = SoftMin{d, 1.f, d, k};
  } else if (d < s.m) {
    if (SOFT) {
      const float sc = exp_neg_accurate(-lambda * (s.m - d));
      s.se = fmaf(s.se, sc, 1.f);
      s.sed = fmaf(s.sed, sc, d);
    }
    s.m = d;
    s.idx = k;
  } else if (SOFT) {
    const float e = exp_neg_accurate(-lambda * (d - s.m));
    s.se += e;
    s.sed = fmaf(e, d, s.sed);
  }
}
template <bool SOFT> __device__ __forceinline__ void softmin_merge(SoftMin& s, const SoftMin o, float lambda) {
  if (o.idx < 0) return;
  if (s.idx < 0) { s = o; return; }
  const bool take = o.m < s.m || (o.m == s.m && o.idx < s.idx);      // a tie keeps the lowest index
  if (SOFT) {
    const float mn = fminf(s.m, o.m);
    const float a = exp_neg_accurate(-lambda * (s.m - mn)), b = exp_neg_accurate(-lambda * (o.m - mn));
    s.se = s.se * a + o.se * b;
    s.sed = s.sed * a + o.sed * b;
  }
  if (take) { s.m = o.m; s.idx = o.idx; }
}

template <bool SOFT>
__global__ __launch_bounds__(256) void style_adherence_fwd_kernel(const float* __restrict__ X, const float* __restrict__ S,
                                                                  float* __restrict__ L, void* __restrict__ stat, int T, int K,
                                                                  int F, int tiles, float lambda) {
  __shared__ StyleTiles sm;
  const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * ROWS;
  const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
  const float* xb = X + (long)b * T * F;
  const float* sb = S + (long)b * K * F;
  SoftMin s{0.f, 0.f, 0.f, -1};
  for (int k0 = 0; k0 < K; k0 += KT) {
    float d[4];
    tile_distances(sm, xb, t0, T, sb, k0, K, F, k0 == 0 || F > FC, true, d);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + j + 16 * i;
      if (k < K) softmin_push<SOFT>(s, d[i], k, lambda);
    }
  }
  // the row's 16 lanes: butterfly 8, 4, 2, 1; lane 0's value is written
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    SoftMin q;
    q.m = __shfl_xor(s.m, o, 64);
    q.se = __shfl_xor(s.se, o, 64);
    q.sed = __shfl_xor(s.sed, o, 64);
    q.idx = __shfl_xor(s.idx, o, 64);
    softmin_merge<SOFT>(s, q, lambda);
  }
  const int t = t0 + r;
  if (j == 0 && t < T) {
    const long row = (long)b * T + t;
    if (SOFT) {
      L[row] = s.sed / s.se;
      // log sum_k exp(-lambda d_k) = -lambda m + log se, kept as its two parts: rounded to one fp32 number it would carry
      // lambda m 2^-24 into every recomputed weight (1e-4 of a far row's, and K = 1 would not give w = 1)
      ((float*)stat)[2 * row] = s.m;
      ((float*)stat)[2 * row + 1] = logf(s.se);
    } else {
      L[row] = s.m;
      ((int*)stat)[row] = s.idx;
    }
  }
}

// c[t, k] of the thread's four pairs into cs[r][.], times `scale` (0 for a row past T): soft w (1 - lambda (d - L)),
// w = exp(-lambda (d - m) - log se); hard [k == argmin]
template <bool SOFT>
__device__ __forceinline__ void write_c(float (*cs)[KT + 1], const float d[4], int k0, int K, float Lt, float m, float logse,
                                        int amin, float scale, float lambda) {
  const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kk = j + 16 * i;
    float c = 0.f;
    if (k0 + kk < K && scale != 0.f) {
      if (SOFT) {
        const float w = exp_neg_accurate(fmaf(-lambda, d[i] - m, -logse));
        c = w * (1.f - lambda * (d[i] - Lt));
      } else {
        c = (k0 + kk == amin) ? 1.f : 0.f;
      }
      c *= scale;
    }
    cs[r][kk] = c;
  }
}

// dX[t] = (2 / F) g[t] sum_k c[t, k] (X[t] - S[k]): one workgroup per row tile, S streamed in ascending k; each style tile's
// partial sum (ascending k by fma) is added to the workgroup's own rows of dX in tile order.
template <bool SOFT>
__global__ __launch_bounds__(256) void style_adherence_dx_kernel(const float* __restrict__ X, const float* __restrict__ S,
                                                                 const float* __restrict__ L, const void* __restrict__ stat,
                                                                 const float* __restrict__ g, int g_stride, float g_scale,
                                                                 float* __restrict__ dX, int T, int K, int F, int tiles,
                                                                 float lambda) {
  __shared__ StyleTiles sm;
  __shared__ float cs[ROWS][KT + 1];
  const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * ROWS;
  const int r = threadIdx.x >> 4, j = threadIdx.x & 15, t = t0 + r;
  const float* xb = X + (long)b * T * F;
  const float* sb = S + (long)b * K * F;
  const long row = (long)b * T + t;
  const bool live = t < T;
  const float Lt = live ? L[row] : 0.f;
  const float smin = live && SOFT ? ((const float*)stat)[2 * row] : 0.f;
  const float slog = live && SOFT ? ((const float*)stat)[2 * row + 1] : 0.f;
  const int amin = live && !SOFT ? ((const int*)stat)[row] : -1;
  const float coef = live ? (2.f / (float)F) * (g[row * g_stride] * g_scale) : 0.f;
  const bool resident = SOFT && F <= FC;          // tile_distances left the only feature chunk in LDS
  for (int k0 = 0; k0 < K; k0 += KT) {
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (SOFT) tile_distances(sm, xb, t0, T, sb, k0, K, F, k0 == 0 || F > FC, true, d);
    __syncthreads();                               // the previous tile's readers of cs are done
    write_c<SOFT>(cs, d, k0, K, Lt, smin, slog, amin, live ? 1.f : 0.f, lambda);
    for (int f0 = 0; f0 < F; f0 += FC) {
      if (!resident) {
        __syncthreads();
        stage_rows(sm.xs, ROWS, xb, t0, T, f0, F);
        stage_rows(sm.ss, KT, sb, k0, K, f0, F);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = j + 16 * i;
        if (!live || f0 + f >= F) continue;
        const float x = sm.xs[r][f];
        float acc = 0.f;
        for (int kk = 0; kk < KT; ++kk) acc = fmaf(cs[r][kk], x - sm.ss[kk][f], acc);     // c = 0 and S = 0 past K
        float* o = dX + row * F + f0 + f;
        *o = k0 == 0 ? coef * acc : *o + coef * acc;
      }
    }
  }
}

// dS[k] = -(2 / F) sum_t g[t] c[t, k] (X[t] - S[k]): one workgroup per style tile, X[b] streamed in ascending t; each row
// tile's partial sum (ascending t by fma) is added to the workgroup's own rows of dS in tile order.
template <bool SOFT>
__global__ __launch_bounds__(256) void style_adherence_ds_kernel(const float* __restrict__ X, const float* __restrict__ S,
                                                                 const float* __restrict__ L, const void* __restrict__ stat,
                                                                 const float* __restrict__ g, int g_stride, float g_scale,
                                                                 float* __restrict__ dS, int T, int K, int F, int ktiles,
                                                                 float lambda) {
  __shared__ StyleTiles sm;
  __shared__ float cs[ROWS][KT + 1];
  const int b = blockIdx.x / ktiles, k0 = (blockIdx.x % ktiles) * KT;
  const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
  const float* xb = X + (long)b * T * F;
  const float* sb = S + (long)b * K * F;
  const bool resident = SOFT && F <= FC;
  for (int t0 = 0; t0 < T; t0 += ROWS) {
    const int t = t0 + r;
    const long row = (long)b * T + t;
    const bool live = t < T;
    const float Lt = live ? L[row] : 0.f;
    const float smin = live && SOFT ? ((const float*)stat)[2 * row] : 0.f;
    const float slog = live && SOFT ? ((const float*)stat)[2 * row + 1] : 0.f;
    const int amin = live && !SOFT ? ((const int*)stat)[row] : -1;
    const float coef = live ? -(2.f / (float)F) * (g[row * g_stride] * g_scale) : 0.f;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (SOFT) tile_distances(sm, xb, t0, T, sb, k0, K, F, true, t0 == 0 || F > FC, d);
    __syncthreads();
    write_c<SOFT>(cs, d, k0, K, Lt, smin, slog, amin, coef, lambda);
    for (int f0 = 0; f0 < F; f0 += FC) {
      if (!resident) {
        __syncthreads();
        stage_rows(sm.xs, ROWS, xb, t0, T, f0, F);
        stage_rows(sm.ss, KT, sb, k0, K, f0, F);
      }
      __syncthreads();
      // thread -> style rows (tid >> 4) + 16 a, features (tid & 15) + 16 i
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int kk = r + 16 * a;
        if (k0 + kk >= K) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int f = j + 16 * i;
          if (f0 + f >= F) continue;
          const float s = sm.ss[kk][f];
          float acc = 0.f;
          for (int rr = 0; rr < ROWS; ++rr) acc = fmaf(cs[rr][kk], sm.xs[rr][f] - s, acc);   // c = 0 for rows past T
          float* o = dS + ((long)b * K + k0 + kk) * F + f0 + f;
          *o = t0 == 0 ? acc : *o + acc;
        }
      }
    }
  }
}

static bool style_shape_ok(int B, int T, int K, int F, float lambda) {
  if (B <= 0 || T <= 0 || K <= 0 || F <= 0 || !(lambda >= 0.f) || !(lambda <= 3.0e38f)) return false;
  const long tiles = ((long)T + ROWS - 1) / ROWS, ktiles = ((long)K + KT - 1) / KT;
  return (long)B * tiles <= 0x7fffffffL && (long)B * ktiles <= 0x7fffffffL;
}

extern "C" int msmd_style_adherence_forward(const float* X, const float* S, float* L, void* stat, int B, int T, int K, int F,
                                            float lambda, int soft, msmd_stream_t stream) {
  if (!style_shape_ok(B, T, K, F, lambda) || !X || !S || !L || !stat) return 1;
  const int tiles = (T + ROWS - 1) / ROWS;
  const dim3 grid((unsigned)(B * tiles)), block(256);
  if (soft)
    hipLaunchKernelGGL(style_adherence_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, X, S, L, stat, T, K, F, tiles, lambda);
  else
    hipLaunchKernelGGL(style_adherence_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, X, S, L, stat, T, K, F, tiles, lambda);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_style_adherence_backward(const float* X, const float* S, const float* L, const void* stat, const float* g,
                                             int g_stride, float g_scale, float* dX, float* dS, int B, int T, int K, int F,
                                             float lambda, int soft, msmd_stream_t stream) {
  if (!style_shape_ok(B, T, K, F, lambda) || !X || !S || !L || !stat || !g || (g_stride != 0 && g_stride != 1) || (!dX && !dS))
    return 1;
  const int tiles = (T + ROWS - 1) / ROWS, ktiles = (K + KT - 1) / KT;
  const dim3 block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dX) {
    const dim3 grid((unsigned)(B * tiles));
    if (soft)
      hipLaunchKernelGGL(style_adherence_dx_kernel<true>, grid, block, 0, st, X, S, L, stat, g, g_stride, g_scale, dX, T, K, F, tiles, lambda);
    else
      hipLaunchKernelGGL(style_adherence_dx_kernel<false>, grid, block, 0, st, X, S, L, stat, g, g_stride, g_scale, dX, T, K, F, tiles, lambda);
  }
  if (dS) {
    const dim3 grid((unsigned)(B * ktiles));
    if (soft)
      hipLaunchKernelGGL(style_adherence_ds_kernel<true>, grid, block, 0, st, X, S, L, stat, g, g_stride, g_scale, dS, T, K, F, ktiles, lambda);
    else
      hipLaunchKernelGGL(style_adherence_ds_kernel<false>, grid, block, 0, st, X, S, L, stat, g, g_stride, g_scale, dS, T, K, F, ktiles, lambda);
  }
  MSMD_RETURN_LAST();
}

// Mean of n fp32 values in a fixed order: thread i adds elements i, i + 256, ... in double, then a halving tree over the 256
// partial sums.  One workgroup whatever n, so the order is a function of n alone.
__global__ __launch_bounds__(256) void ordered_mean_kernel(const float* __restrict__ in, long n, float* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += (double)in[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] / (double)n);
}

extern "C" int msmd_ordered_mean(const float* in, long n, float* out, msmd_stream_t stream) {
  if (n <= 0 || !in || !out) return 1;
  hipLaunchKernelGGL(ordered_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, in, n, out);
  MSMD_RETURN_LAST();
}

// ------------------------------------------------------------------------------------------------ NT-Xent
#define NTX_EPS 1e-12f            // F.normalize's eps
#define NTX_CHUNK MSMD_NT_XENT_CHUNK

// row i of cat(a, b) -> fhat[i] = f / max(|f|, eps), norm[i] = |f|: one workgroup per row
__global__ __launch_bounds__(256) void nt_xent_normalize_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                float* __restrict__ fhat, float* __restrict__ norm, int B, int D) {
  __shared__ float red[16];
  const int i = blockIdx.x;
  const float* f = i < B ? a + (long)i * D : b + (long)(i - B) * D;
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) s = fmaf(f[d], f[d], s);
  const float nrm = sqrtf(block_sum(s, red));
  const float den = fmaxf(nrm, NTX_EPS);
  for (int d = threadIdx.x; d < D; d += 256) fhat[(long)i * D + d] = f[d] / den;
  if (threadIdx.x == 0) norm[i] = nrm;
}

// all lanes of the wave: fhat_i . fhat_j, lane l adding d = l, l + 64, ... by fma, then the xor butterfly
__device__ __forceinline__ float wave_dot(const float* __restrict__ fi, const float* __restrict__ fj, int D) {
  float a = 0.f;
  for (int d = threadIdx.x & 63; d < D; d += 64) a = fmaf(fi[d], fj[d], a);
  return wave_sum(a);
}

// one workgroup per row i: wave w takes j = w, w + 4, ... (j != i) with a running (max, sum exp); thread 0 joins the four
// waves in wave order.  row_loss[i] = lse_i - s_{i p(i)},  s = fhat_i . fhat_j / tau.
__global__ __launch_bounds__(256) void nt_xent_fwd_kernel(const float* __restrict__ fhat, float* __restrict__ row_loss,
                                                          float* __restrict__ lse, int B, int D, float tau) {
  __shared__ float wm[4], ws[4], spos;
  const int N = 2 * B, i = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int pos = i < B ? i + B : i - B;
  const float* fi = fhat + (long)i * D;
  float m = -INFINITY, se = 0.f;
  for (int j = wid; j < N; j += 4) {              // wave-uniform
    if (j == i) continue;
    const float s = wave_dot(fi, fhat + (long)j * D, D) / tau;
    if (j == pos && lane == 0) spos = s;
    if (s > m) {
      se = fmaf(se, exp_neg_accurate(m - s), 1.f);
      m = s;
    } else {
      se += exp_neg_accurate(s - m);
    }
  }
  if (lane == 0) { wm[wid] = m; ws[wid] = se; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3])), tot = 0.f;
    for (int w = 0; w < 4; ++w)
      if (ws[w] > 0.f) tot = fmaf(ws[w], exp_neg_accurate(wm[w] - M), tot);
    const float lt = logf(tot);
    lse[2 * i] = M;                 // the row's log-sum-exp M + log tot as its two parts (see the adherence statistic)
    lse[2 * i + 1] = lt;
    row_loss[i] = (M - spos) + lt;
  }
}

// one workgroup per row i.  coef_j = up ((p_ij - [j = p(i)]) + (p_ji - [j = p(i)])) / (N tau), p_ij = exp((s_ij - max_i) - log_i), for a
// chunk of 256 rows j at a time (wave per j); h_i = sum_j coef_j fhat_j in ascending j by fma, kept in the row's own slot of
// `grad` between chunks; then grad_i = (h_i - fhat_i (fhat_i . h_i)) / |f_i|, or h_i / eps where the norm was clamped.
__global__ __launch_bounds__(256) void nt_xent_bwd_kernel(const float* __restrict__ fhat, const float* __restrict__ norm,
                                                          const float* __restrict__ lse, const float* __restrict__ upstream,
                                                          float* __restrict__ grad, int B, int D, float tau) {
  __shared__ float coef[NTX_CHUNK];
  __shared__ float red[16];
  const int N = 2 * B, i = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int pos = i < B ? i + B : i - B;
  const float* fi = fhat + (long)i * D;
  float* h = grad + (long)i * D;
  const float up = upstream[0] / ((float)N * tau), max_i = lse[2 * i], log_i = lse[2 * i + 1];
  for (int j0 = 0; j0 < N; j0 += NTX_CHUNK) {
    __syncthreads();
    for (int jc = wid; jc < NTX_CHUNK; jc += 4) {   // wave-uniform
      const int j = j0 + jc;
      float c = 0.f;
      if (j < N && j != i) {
        const float s = wave_dot(fi, fhat + (long)j * D, D) / tau;
        const float hot = j == pos ? 1.f : 0.f;
        const float pij = exp_neg_accurate((s - max_i) - log_i), pji = exp_neg_accurate((s - lse[2 * j]) - lse[2 * j + 1]);
        c = up * ((pij - hot) + (pji - hot));
      }
      if (lane == 0) coef[jc] = c;
    }
    __syncthreads();
    const int nj = min(NTX_CHUNK, N - j0);
    for (int d = threadIdx.x; d < D; d += 256) {
      float acc = j0 == 0 ? 0.f : h[d];
      for (int jc = 0; jc < nj; ++jc) acc = fmaf(coef[jc], fhat[(long)(j0 + jc) * D + d], acc);
      h[d] = acc;
    }
  }
  float p = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) p = fmaf(h[d], fi[d], p);      // each thread reads back what it wrote
  p = block_sum(p, red);
  const float nrm = norm[i];
  const bool clamped = !(nrm >= NTX_EPS);
  const float den = fmaxf(nrm, NTX_EPS);
  for (int d = threadIdx.x; d < D; d += 256) h[d] = (clamped ? h[d] : h[d] - fi[d] * p) / den;
}

extern "C" int msmd_nt_xent_forward(const float* a, const float* b, float* fhat, float* norm, float* row_loss, float* lse,
                                    int B, int D, float temperature, msmd_stream_t stream) {
  if (B <= 0 || B > 0x3fffffff || D <= 0 || !(temperature > 0.f) || !(temperature <= 3.0e38f) || !a || !b || !fhat || !norm ||
      !row_loss || !lse)
    return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nt_xent_normalize_kernel, dim3(2 * B), dim3(256), 0, st, a, b, fhat, norm, B, D);
  hipLaunchKernelGGL(nt_xent_fwd_kernel, dim3(2 * B), dim3(256), 0, st, fhat, row_loss, lse, B, D, temperature);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_nt_xent_backward(const float* fhat, const float* norm, const float* lse, const float* upstream, float* grad,
                                     int B, int D, float temperature, msmd_stream_t stream) {
  if (B <= 0 || B > 0x3fffffff || D <= 0 || !(temperature > 0.f) || !(temperature <= 3.0e38f) || !fhat || !norm || !lse ||
      !upstream || !grad)
    return 1;
  hipLaunchKernelGGL(nt_xent_bwd_kernel, dim3(2 * B), dim3(256), 0, (hipStream_t)stream, fhat, norm, lse, upstream, grad, B, D,
                     temperature);
  MSMD_RETURN_LAST();
}
