// Audio front end: interleaved PCM -> 16 kHz mono fp32, then per-clip z-normalisation.
// Three launches (resample; per-clip statistics; z-norm) for a ragged group of clips of one (rate, sample type): no host
// synchronisation, no atomics, the same bits for a clip whatever group it is in (a workgroup's run and a clip's partial sums
// depend on the clip's own length only).
#include "common.h"

namespace {

#define AR_THREADS 256
#define AR_RUN MSMD_AUDIO_RUN          // outputs per workgroup of the resample kernel: one per lane
#define AZ_RUN 4096                    // outputs per workgroup of the z-norm kernel
#define AR_LDS_LIMIT 65536             // bytes of dynamic LDS a launch may ask for without an attribute

struct ClipDesc { long in_off, frames, channels, out_off, out_len; };

__device__ __forceinline__ ClipDesc load_desc(const long* __restrict__ desc, int clip) {
  const long* d = desc + (long)clip * 5;
  return ClipDesc{d[0], d[1], d[2], d[3], d[4]};
}

// x[k] = (sum over the frame's channels, in channel order, fp32) / C; int16 samples scale by 2^-15 first (exact).
// Frames outside [0, N), and anything the descriptor would place outside the PCM buffer, read as zero.
template <typename S>
__device__ __forceinline__ float downmix_at(const S* __restrict__ pcm, const ClipDesc& d, long k, long pcm_elems) {
  if (k < 0 || k >= d.frames) return 0.f;
  const long e = d.in_off + k * d.channels;
  if (e < 0 || e + d.channels > pcm_elems) return 0.f;
  float sum = 0.f;
  for (long c = 0; c < d.channels; ++c) {
    float v;
    if constexpr (sizeof(S) == 2) v = (float)pcm[e + c] * 3.0517578125e-5f;
    else v = pcm[e + c];
    sum += v;
  }
  return __fdiv_rn(sum, (float)d.channels);
}

// Fixed-order sum over the workgroup's 256 lanes in double: xor tree inside a wave, then the four waves in wave order.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup per (run of AR_RUN outputs, clip).  The input span the run needs is downmixed, converted and staged ONCE in
// LDS, zero-filled past the clip's ends, so the tap loop has no edge branch.  Lane = output n: input position n M / L splits
// into k0 = n M div L and the phase n M mod L; the bank is tap-major over the OUTPUT's phase order r = n mod L
// (bank[i * L + r] = h(((r M) mod L) / L - (i - half))), so adjacent lanes read adjacent bank words.
// taps == 0: same rate, the output is the downmix itself.
template <typename S>
__global__ __launch_bounds__(AR_THREADS) void audio_resample_kernel(const S* __restrict__ pcm, const long* __restrict__ desc,
                                                                    const float* __restrict__ bank, float* __restrict__ out,
                                                                    double* __restrict__ partials, int L, int M, int taps,
                                                                    int span_cap, long pcm_elems, long out_elems) {
  extern __shared__ float s_x[];
  __shared__ double s_red[2][AR_THREADS / 64];
  const int tid = threadIdx.x, clip = blockIdx.y;
  const ClipDesc d = load_desc(desc, clip);
  const long n0 = (long)blockIdx.x * AR_RUN;
  if (n0 >= d.out_len) return;                                   // uniform: a shorter clip of the ragged group
  const int run = (int)min((long)AR_RUN, d.out_len - n0);
  const long n = n0 + tid;
  float y = 0.f;
  if (taps == 0) {
    if (tid < run) y = downmix_at(pcm, d, n, pcm_elems);
  } else {
    const int half = (taps - 2) / 2;
    const long k_first = (n0 * M) / L;                           // k0 of the run's first output
    const long k_lo = k_first - half;
    const long k_hi = ((n0 + run - 1) * M) / L - half + taps - 1;
    const int span = (int)min(k_hi - k_lo + 1, (long)span_cap);
    for (int p = tid; p < span; p += AR_THREADS) s_x[p] = downmix_at(pcm, d, k_lo + p, pcm_elems);
    __syncthreads();
    if (tid < run) {
      const long pos = n * M;
      const int base = (int)(pos / L - k_first);                 // k0(n) - half - k_lo
      const float* __restrict__ b = bank + (int)(n % L);
      const float* __restrict__ x = s_x + base;
      if (base >= 0 && base + taps <= span) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        const int t4 = taps & ~3;
        int i = 0;
        for (; i < t4; i += 4) {
          a0 = fmaf(x[i], b[(long)i * L], a0);
          a1 = fmaf(x[i + 1], b[(long)(i + 1) * L], a1);
          a2 = fmaf(x[i + 2], b[(long)(i + 2) * L], a2);
          a3 = fmaf(x[i + 3], b[(long)(i + 3) * L], a3);
        }
        if (i < taps) {                                          // taps is even: two left at most
          a0 = fmaf(x[i], b[(long)i * L], a0);
          a1 = fmaf(x[i + 1], b[(long)(i + 1) * L], a1);
        }
        y = (a0 + a1) + (a2 + a3);
      }
    }
  }
  if (tid < run && d.out_off >= 0 && d.out_off + n < out_elems) out[d.out_off + n] = y;
  const double yd = (double)y;                                   // lanes past the run hold 0
  const double s = block_sum_f64(yd, s_red[0]);
  const double q = block_sum_f64(yd * yd, s_red[1]);
  if (tid == 0) {
    double* p = partials + ((long)clip * gridDim.x + blockIdx.x) * 2;
    p[0] = s;
    p[1] = q;
  }
}

// One wave per clip: the clip's per-run partial sums are added in run order (every lane does the same additions), mean and
// population standard deviation in double; stats[clip] = (mean, 1 / (std + 1e-5)).  Linear in the clip's length.
__global__ __launch_bounds__(64) void audio_stats_kernel(const long* __restrict__ desc, const double* __restrict__ partials,
                                                         double* __restrict__ stats, long max_runs) {
  const int clip = blockIdx.x;
  const ClipDesc d = load_desc(desc, clip);
  const long runs = min((d.out_len + AR_RUN - 1) / AR_RUN, max_runs);
  const double* __restrict__ p = partials + (long)clip * max_runs * 2;
  double s = 0.0, q = 0.0;
  for (long r = 0; r < runs; ++r) {
    s += p[2 * r];
    q += p[2 * r + 1];
  }
  const double cnt = (double)max(d.out_len, 1L);
  const double mean = s / cnt;
  const double var = fmax(q / cnt - mean * mean, 0.0);
  if (threadIdx.x == 0) {
    stats[2 * clip] = mean;
    stats[2 * clip + 1] = 1.0 / (sqrt(var) + 1e-5);
  }
}

// One workgroup per (AZ_RUN outputs, clip): (y - mean) / (std + 1e-5) in place, from the clip's stats.
__global__ __launch_bounds__(AR_THREADS) void audio_znorm_kernel(float* __restrict__ out, const long* __restrict__ desc,
                                                                 const double* __restrict__ stats, long out_elems) {
  const int clip = blockIdx.y;
  const ClipDesc d = load_desc(desc, clip);
  const long z0 = (long)blockIdx.x * AZ_RUN;
  if (z0 >= d.out_len || d.out_off < 0) return;
  const double mean = stats[2 * clip], inv = stats[2 * clip + 1];
  const long z1 = min(z0 + AZ_RUN, d.out_len);
  for (long n = z0 + threadIdx.x; n < z1; n += AR_THREADS) {
    const long o = d.out_off + n;
    if (o < out_elems) out[o] = (float)(((double)out[o] - mean) * inv);
  }
}

}  // namespace

extern "C" int msmd_audio_resample(const void* pcm, long pcm_elems, int is_int16, const long* desc, int n_clips,
                                   long max_out_len, int L, int M, int taps, const float* bank, float* out, long out_elems,
                                   double* partials, msmd_stream_t stream) {
  if (n_clips <= 0 || n_clips > MSMD_AUDIO_MAX_CLIPS || max_out_len <= 0 || pcm_elems <= 0 || out_elems <= 0 || L <= 0 || M <= 0) return 1;
  if (taps == 0 ? (L != 1 || M != 1) : (taps < 4 || (taps & 1) || bank == nullptr)) return 1;
  const long runs = (max_out_len + AR_RUN - 1) / AR_RUN;
  if (runs > 2147483647L) return 1;
  // the longest span a run can need: k0 moves by at most (run - 1) M div L + 1 across the run, plus the taps
  const long span_cap = taps == 0 ? 0 : ((long)(AR_RUN - 1) * M) / L + 2 + taps;
  if (span_cap * 4 > AR_LDS_LIMIT) return 1;
  const dim3 grid((unsigned)runs, (unsigned)n_clips);
  if (is_int16)
    hipLaunchKernelGGL(audio_resample_kernel<short>, grid, dim3(AR_THREADS), (size_t)span_cap * 4, (hipStream_t)stream,
                       (const short*)pcm, desc, bank, out, partials, L, M, taps, (int)span_cap, pcm_elems, out_elems);
  else
    hipLaunchKernelGGL(audio_resample_kernel<float>, grid, dim3(AR_THREADS), (size_t)span_cap * 4, (hipStream_t)stream,
                       (const float*)pcm, desc, bank, out, partials, L, M, taps, (int)span_cap, pcm_elems, out_elems);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_audio_znorm(float* out, long out_elems, const long* desc, int n_clips, long max_out_len,
                                const double* partials, double* stats, msmd_stream_t stream) {
  if (n_clips <= 0 || n_clips > MSMD_AUDIO_MAX_CLIPS || max_out_len <= 0 || out_elems <= 0 || stats == nullptr) return 1;
  const long runs = (max_out_len + AR_RUN - 1) / AR_RUN, blocks = (max_out_len + AZ_RUN - 1) / AZ_RUN;
  if (blocks > 2147483647L) return 1;
  hipLaunchKernelGGL(audio_stats_kernel, dim3((unsigned)n_clips), dim3(64), 0, (hipStream_t)stream, desc, partials, stats, runs);
  hipLaunchKernelGGL(audio_znorm_kernel, dim3((unsigned)blocks, (unsigned)n_clips), dim3(AR_THREADS), 0, (hipStream_t)stream,
                     out, desc, stats, out_elems);
  MSMD_RETURN_LAST();
}
