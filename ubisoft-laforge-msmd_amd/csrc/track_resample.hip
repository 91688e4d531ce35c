// Fourier resampling of motion tracks to the goal frame rate (reference dataset_processing/Step5_resample_and_assemble.py: one
// scipy.signal.resample per track; Step3_preprocess_expression_code.py: savgol_filter(code, 5, 2, axis=0)).
// A clip of Nx frames becomes num frames through its first K + 1 = min(Nx, num) / 2 + 1 Fourier bins: a dense DFT of an
// arbitrary length in two stages, each a workgroup tile of TR_ROWS outputs x TR_CH channels that loops over the other index
// with the twiddle e^{2 pi i r / P} read from a table at the integer residue r = (row * j) mod P.  Everything is double; the
// residue is stepped in integers, so no phase is ever formed in floating point.
#include "savgol.h"

constexpr int TR_WG = 256;
constexpr int TR_ROWS = 16;            // bins (analysis) / output frames (synthesis) per workgroup
constexpr int TR_CH = 16;              // channels per workgroup
constexpr int TR_STAGE = 64;           // frames (analysis) / bins (synthesis) staged in LDS per pass
constexpr int TR_MAX = 4096;           // frames of one clip, in or out
static_assert(TR_ROWS == MSMD_TRACK_ROWS && TR_CH == MSMD_TRACK_CH_TILE && TR_STAGE == MSMD_TRACK_STAGE &&
              TR_MAX == MSMD_TRACK_MAX_FRAMES && 65535 * TR_CH == MSMD_TRACK_MAX_CHANNELS, "header and kernel disagree");
static_assert(TR_ROWS * TR_CH == TR_WG && TR_STAGE % TR_ROWS == 0, "one thread per (row, channel) of the tile");

struct Cplx { double re, im; };

// cos / sin(2 pi r / P) for r = 0 .. P / 2: the upper half of the circle is the lower half mirrored.
__device__ __forceinline__ void fill_twiddles(Cplx* __restrict__ tab, int P) {
  for (int r = threadIdx.x; r <= (P >> 1); r += TR_WG) {
    double s, c;
    sincospi(2.0 * (double)r / (double)P, &s, &c);
    tab[r] = Cplx{c, s};
  }
}
__device__ __forceinline__ Cplx twiddle(const Cplx* __restrict__ tab, int r, int P) {
  const bool mirror = r > (P >> 1);
  const Cplx t = tab[mirror ? P - r : r];
  return Cplx{t.re, mirror ? -t.im : t.im};
}

// The clip a workgroup belongs to, from the device copy of the offsets.  ok is false for sizes the entry point refuses:
// the copy is the array it checked, so this only keeps a stale workspace from indexing anything.
struct Clip { long in0, out0, spec0; int Nx, num, K; bool ok; };
__device__ __forceinline__ Clip clip_of(const int* __restrict__ offs, int n_clips, int i) {
  Clip c;
  c.in0 = offs[i];
  c.Nx = offs[i + 1] - offs[i];
  c.out0 = offs[n_clips + 1 + i];
  c.num = offs[n_clips + 2 + i] - offs[n_clips + 1 + i];
  c.ok = c.Nx >= 1 && c.Nx <= TR_MAX && c.num >= 1 && c.num <= TR_MAX && c.in0 >= 0 && c.out0 >= 0;
  c.K = min(c.Nx, c.num) >> 1;
  c.spec0 = (c.in0 >> 1) + i;          // K + 1 <= Nx / 2 + 1 rows per clip: the rows of two clips never meet
  return c;
}

// Analysis.  grid (clip, tile of TR_ROWS bins, tile of TR_CH channels).  Thread (kl, cl) owns bin k = tile * TR_ROWS + kl of
// channel c = tile * TR_CH + cl; the frames pass through LDS TR_STAGE at a time, read through the filter when there is one.
// spec (rows, C) complex: X[k] times its synthesis weight over Nx, so the synthesis is a plain sum.
__global__ __launch_bounds__(TR_WG) void track_analysis_kernel(const float* __restrict__ x, const int* __restrict__ offs, int n_clips,
                                                               int C, const double* __restrict__ savgol, int window,
                                                               Cplx* __restrict__ spec) {
  __shared__ Cplx s_tab[TR_MAX / 2 + 1];
  __shared__ double s_x[TR_STAGE * TR_CH];
  __shared__ double s_coef[SAVGOL_TABLE];
  const Clip cl = clip_of(offs, n_clips, blockIdx.x);
  const int k0 = blockIdx.y * TR_ROWS;
  if (!cl.ok || k0 > cl.K || cl.Nx < window) return;
  const int Nx = cl.Nx, tid = threadIdx.x, lc = tid % TR_CH, lr = tid / TR_CH;
  const int c = blockIdx.z * TR_CH + lc, k = k0 + lr;
  const bool live_c = c < C;
  fill_twiddles(s_tab, Nx);
  savgol_stage<TR_WG>(s_coef, savgol, window);
  const float* __restrict__ xc = x + cl.in0 * C + (live_c ? c : 0);
  double re = 0.0, im = 0.0;
  for (int n0 = 0; n0 < Nx; n0 += TR_STAGE) {
    const int cnt = min(TR_STAGE, Nx - n0);
    __syncthreads();                      // the table and the coefficients (first pass); the last pass's reads of s_x
    for (int j = lr; j < cnt; j += TR_ROWS) {
      const int n = n0 + j;
      double v = 0.0;
      if (live_c) {
        if (window == 0) {
          v = (double)xc[(long)n * C];
        } else {
          int first;
          const double* __restrict__ row = savgol_row(s_coef, window, n, Nx, first);
          for (int m = 0; m < window; ++m) v = fma(row[m], (double)xc[(long)(first + m) * C], v);
        }
      }
      s_x[j * TR_CH + lc] = v;
    }
    __syncthreads();
    if (k <= cl.K) {
      int r = (int)(((long)k * n0) % Nx);
      for (int j = 0; j < cnt; ++j) {
        const Cplx t = twiddle(s_tab, r, Nx);
        const double v = s_x[j * TR_CH + lc];
        re = fma(v, t.re, re);
        im = fma(-v, t.im, im);
        r += k;
        if (r >= Nx) r -= Nx;
      }
    }
  }
  if (k > cl.K || !live_c) return;
  double wgt = k == 0 ? 1.0 : 2.0;
  const int N = min(Nx, cl.num);
  if (k == cl.K && !(N & 1)) {
    if (cl.num < Nx) wgt *= 2.0;
    else if (cl.num > Nx) wgt *= 0.5;
  }
  if (k > 0 && !(cl.num & 1) && k == (cl.num >> 1)) {     // the output's own Nyquist bin: once, real part only
    wgt *= 0.5;
    im = 0.0;
  }
  spec[(cl.spec0 + k) * C + c] = Cplx{re * wgt / (double)Nx, im * wgt / (double)Nx};
}

// Synthesis.  grid (clip, tile of TR_ROWS output frames, tile of TR_CH channels).  Thread (ml, cl) owns frame m of channel c
// and adds the bins in ascending k, staged through LDS TR_STAGE at a time.
__global__ __launch_bounds__(TR_WG) void track_synthesis_kernel(const Cplx* __restrict__ spec, const int* __restrict__ offs, int n_clips,
                                                                int C, int window, float* __restrict__ y) {
  __shared__ Cplx s_tab[TR_MAX / 2 + 1];
  __shared__ Cplx s_X[TR_STAGE * TR_CH];
  const Clip cl = clip_of(offs, n_clips, blockIdx.x);
  const int m0 = blockIdx.y * TR_ROWS;
  if (!cl.ok || m0 >= cl.num || cl.Nx < window) return;
  const int num = cl.num, tid = threadIdx.x, lc = tid % TR_CH, lr = tid / TR_CH;
  const int c = blockIdx.z * TR_CH + lc, m = m0 + lr;
  const bool live_c = c < C;
  fill_twiddles(s_tab, num);
  const Cplx* __restrict__ sc = spec + cl.spec0 * C + (live_c ? c : 0);
  double acc = 0.0;
  for (int b0 = 0; b0 <= cl.K; b0 += TR_STAGE) {
    const int cnt = min(TR_STAGE, cl.K + 1 - b0);
    __syncthreads();
    for (int j = lr; j < cnt; j += TR_ROWS) s_X[j * TR_CH + lc] = live_c ? sc[(long)(b0 + j) * C] : Cplx{0.0, 0.0};
    __syncthreads();
    if (m < num) {
      int r = (int)(((long)m * b0) % num);
      for (int j = 0; j < cnt; ++j) {
        const Cplx t = twiddle(s_tab, r, num);
        const Cplx X = s_X[j * TR_CH + lc];
        acc = fma(X.re, t.re, acc);
        acc = fma(-X.im, t.im, acc);
        r += m;
        if (r >= num) r -= num;
      }
    }
  }
  if (m < num && live_c) y[(cl.out0 + m) * C + c] = (float)acc;
}

static inline long track_header_bytes(int n_clips) { return ((2L * (n_clips + 1) * (long)sizeof(int)) + 15) & ~15L; }

extern "C" long msmd_track_resample_ws_bytes(long total_in, int n_clips, int C) {
  if (total_in < 1 || total_in > 0x7fffffffL || n_clips < 1 || C < 1) return 0;
  return track_header_bytes(n_clips) + (total_in / 2 + n_clips) * (long)C * (long)sizeof(Cplx);
}

extern "C" int msmd_track_resample(const float* x, const int* in_offsets, const int* out_offsets, int n_clips, int C,
                                   const double* savgol, int window, void* ws, float* y, msmd_stream_t stream) {
  if (!x || !in_offsets || !out_offsets || !ws || !y || n_clips < 1 || C < 1 || C > MSMD_TRACK_MAX_CHANNELS) return 1;
  if (window != 0 && !(savgol_window_ok(window) && savgol)) return 1;
  if (in_offsets[0] != 0 || out_offsets[0] != 0) return 1;
  int max_k = 0, max_m = 0;
  for (int i = 0; i < n_clips; ++i) {
    const long F = (long)in_offsets[i + 1] - in_offsets[i], M = (long)out_offsets[i + 1] - out_offsets[i];
    if (F < 1 || F > TR_MAX || M < 1 || M > TR_MAX || F < window) return 1;
    max_k = max(max_k, (int)(min(F, M) / 2));
    max_m = max(max_m, (int)M);
  }
  hipStream_t st = (hipStream_t)stream;
  int* offs = (int*)ws;
  Cplx* spec = (Cplx*)((char*)ws + track_header_bytes(n_clips));
  const size_t nb = (size_t)(n_clips + 1) * sizeof(int);
  hipError_t e = hipMemcpyAsync(offs, in_offsets, nb, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(offs + n_clips + 1, out_offsets, nb, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  const unsigned cz = (unsigned)((C + TR_CH - 1) / TR_CH);
  hipLaunchKernelGGL(track_analysis_kernel, dim3((unsigned)n_clips, (unsigned)(max_k / TR_ROWS + 1), cz), dim3(TR_WG), 0, st, x, offs,
                     n_clips, C, savgol, window, spec);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(track_synthesis_kernel, dim3((unsigned)n_clips, (unsigned)((max_m + TR_ROWS - 1) / TR_ROWS), cz), dim3(TR_WG), 0, st,
                     spec, offs, n_clips, C, window, y);
  MSMD_RETURN_LAST();
}
