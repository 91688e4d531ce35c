// Denoiser glue and the CFG + DDPM update: small elementwise kernels (HBM/launch-bound), written so
// that one sampler step is a fixed sequence of launches with no host round trip (hipGraph-capturable).
#include "common.h"

// feats rows 1.. = [prev_motion ; x_t] ++ indicator ++ zero pad; row 0 (person token slot) is zero-filled.
// guide_mask (nullable; keyframe in-painting of the denoiser INPUT, reference model.py:762-767: motion_in[:, idx, :] = values
// before every denoiser call): where guide_mask[nm, t] != 0 the motion columns of frame t come from guide_values instead of
// motion.  The mask / value pair is dense, (motion_batch, L) uint8 / (motion_batch, L, dm) fp32, so a captured launch does not
// depend on which frames are pinned or how many; the overwrite is per clip and every CFG entry of a clip reads the same
// overwritten input.  eps (nullable): the q-sample form of the training path (no keyframes there: the entry rejects both).
// The operands of one packing, shared by pack_input_kernel and denoiser_prepare_kernel.  prev_stride: elements between the prev
// rows of two sequences (Lp * dm for a contiguous (N, Lp, dm); 0 = every sequence reads the one start row block).
struct PackInput {
  const float* motion; const float* eps; const float* prev; const float* ind;
  const unsigned char* guide_mask; const float* guide_values;
  int L, Lp, dm, Kpad, motion_batch; long prev_stride;
};

// Element i (row i / Kpad, column i % Kpad) of sequence n's (1 + Lp + L, Kpad) block, before the cast to the storage type.
// c0 / c1: the q-sample coefficients of clip n % motion_batch, read only where eps is set.
__device__ __forceinline__ float pack_input_value(const PackInput& a, int n, int i, float c0, float c1) {
  const int nm = n % a.motion_batch;  // CFG entries share one x_t (reference model.py:389)
  const int r = i / a.Kpad - 1, k = i % a.Kpad;  // r == -1: person-token row, zero-filled here
  float v = 0.f;
  if (r >= 0 && r < a.Lp) {
    if (k < a.dm) v = a.prev[(long)n * a.prev_stride + (long)r * a.dm + k];
  } else if (r >= a.Lp) {
    const int t = r - a.Lp;
    if (k < a.dm) {
      const long at = ((long)nm * a.L + t) * a.dm + k;
      v = a.motion[at];
      if (a.guide_mask && a.guide_mask[(long)nm * a.L + t]) v = a.guide_values[at];
      if (a.eps) v = __fmaf_rn(c0, v, c1 * a.eps[at]);   // one rounding of c1 eps, then one fused multiply-add
    } else if (k == a.dm && a.ind) {
      v = a.ind[(long)n * a.L + t];
    }
  }
  return v;
}

template <typename TO>
__global__ void pack_input_kernel(PackInput a, const float* __restrict__ c0, const float* __restrict__ c1,
                                  TO* __restrict__ feats) {
  const int n = blockIdx.y;
  const int Tn = 1 + a.Lp + a.L;
  const int nm = n % a.motion_batch;
  const float c0n = a.eps ? c0[nm] : 0.f, c1n = a.eps ? c1[nm] : 0.f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Tn * a.Kpad; i += gridDim.x * blockDim.x)
    feats[(long)n * Tn * a.Kpad + i] = from_f32<TO>(pack_input_value(a, n, i, c0n, c1n));
}

extern "C" int msmd_denoiser_pack_input_guided(const float* motion, const float* eps, const float* c0, const float* c1,
                                               const float* prev_motion, const float* indicator,
                                               const unsigned char* guide_mask, const float* guide_values, void* feats,
                                               int N, int L, int Lp, int dm, int Kpad, int motion_batch, int out_dtype,
                                               msmd_stream_t stream) {
  if (guide_mask && (eps || !guide_values)) return 1;  // the q-sample form is the training path: no keyframes there
  if (N <= 0 || L <= 0 || Lp < 0 || dm <= 0 || Kpad < dm + (indicator ? 1 : 0) || motion_batch <= 0) return 1;
  dim3 grid(((1 + Lp + L) * Kpad + 255) / 256, N), block(256);
  const PackInput a{motion, eps, prev_motion, indicator, guide_mask, guide_values, L, Lp, dm, Kpad, motion_batch, (long)Lp * dm};
  return dispatch_dtype<float, f16_t, bf16_t>(out_dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) TO;
    hipLaunchKernelGGL(pack_input_kernel<TO>, grid, block, 0, (hipStream_t)stream, a, c0, c1, (TO*)feats);
    MSMD_RETURN_LAST();
  });
}

extern "C" int msmd_denoiser_pack_input(const float* motion, const float* eps, const float* c0, const float* c1,
                                        const float* prev_motion, const float* indicator, void* feats, int N, int L,
                                        int Lp, int dm, int Kpad, int motion_batch, int out_dtype,
                                        msmd_stream_t stream) {
  return msmd_denoiser_pack_input_guided(motion, eps, c0, c1, prev_motion, indicator, nullptr, nullptr, feats, N, L, Lp,
                                         dm, Kpad, motion_batch, out_dtype, stream);
}

// x (N, T, d) += pe (T, d); row 0 = tok0 (N, d) + row0_add (d, optional) + pe[0]  (row 0 of x is overwritten)
template <typename T>
__global__ void add_pe_token_kernel(T* __restrict__ x, const float* __restrict__ pe, const T* __restrict__ tok0,
                                    const T* __restrict__ row0_add, int Tn, int d) {
  const int n = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Tn * d; i += gridDim.x * blockDim.x) {
    const int t = i / d, c = i % d;
    float base;
    if (t == 0) {
      base = to_f32(tok0[(long)n * d + c]);
      if (row0_add) base += to_f32(row0_add[c]);
    } else {
      base = to_f32(x[(long)n * Tn * d + i]);
    }
    x[(long)n * Tn * d + i] = from_f32<T>(base + pe[i]);
  }
}

// the same on 16-bit rows with d % 8 == 0: 8 elements (one 16-byte access) per thread, the same arithmetic per element
template <typename T>
__global__ __launch_bounds__(256) void add_pe_token_v8_kernel(T* __restrict__ x, const float* __restrict__ pe,
                                                              const T* __restrict__ tok0, const T* __restrict__ row0_add,
                                                              int Tn, int d) {
  typedef typename Vec8T<T>::type V8;
  const int n = blockIdx.y, per_row = d >> 3;
  const int i8 = blockIdx.x * blockDim.x + threadIdx.x;
  if (i8 >= Tn * per_row) return;
  const int t = i8 / per_row, c = (i8 - t * per_row) << 3;
  T* xp = x + ((long)n * Tn + t) * d + c;
  float base[8];
  if (t == 0) {
    const V8 tk = *(const V8*)(tok0 + (long)n * d + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) base[e] = (float)tk[e];
    if (row0_add) {
      const V8 ra = *(const V8*)(row0_add + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) base[e] += (float)ra[e];
    }
  } else {
    const V8 xv = *(const V8*)xp;
#pragma unroll
    for (int e = 0; e < 8; ++e) base[e] = (float)xv[e];
  }
  const f32x4 p0 = *(const f32x4*)(pe + (long)t * d + c), p1 = *(const f32x4*)(pe + (long)t * d + c + 4);
  V8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = (T)(base[e] + p0[e]); o[4 + e] = (T)(base[4 + e] + p1[e]); }
  *(V8*)xp = o;
}

extern "C" int msmd_add_pe_token(void* x, const float* pe, const void* tok0, const void* row0_add, int N, int T, int d,
                                 int dtype, msmd_stream_t stream) {
  if (N <= 0 || T <= 0 || d <= 0 || !tok0) return 1;
  if (dtype != MSMD_F32 && (d & 7) == 0 && !(((uintptr_t)x | (uintptr_t)pe | (uintptr_t)tok0 | (uintptr_t)row0_add) & 15)) {
    dim3 grid8((T * (d >> 3) + 255) / 256, N);
    return dispatch_dtype<f16_t, bf16_t>(dtype, [&](auto tag) {
      typedef MSMD_TAG_T(tag) TX;
      hipLaunchKernelGGL(add_pe_token_v8_kernel<TX>, grid8, dim3(256), 0, (hipStream_t)stream, (TX*)x, pe,
                         (const TX*)tok0, (const TX*)row0_add, T, d);
      MSMD_RETURN_LAST();
    });
  }
  dim3 grid((T * d + 255) / 256, N), block(256);
  return dispatch_dtype<float, f16_t, bf16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) TX;
    hipLaunchKernelGGL(add_pe_token_kernel<TX>, grid, block, 0, (hipStream_t)stream, (TX*)x, pe, (const TX*)tok0,
                       (const TX*)row0_add, T, d);
    MSMD_RETURN_LAST();
  });
}

// out = dyn + sum_b alpha_b * static_b (dims < dm-3, or all dims when use_head_alpha & 1) ; + sum_b static_b (last 3
// dims); use_head_alpha & 2: alpha_b = sigmoid(raw alpha_b)
template <typename T>
__global__ void heads_mix_kernel(const T* __restrict__ dec, long ld_dec, const T* __restrict__ stat,
                                 float* __restrict__ out, int L, int dm, int nb, int stat_batch, int use_head_alpha) {
  const int n = blockIdx.y;
  const int ns = n % stat_batch;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L * dm; i += gridDim.x * blockDim.x) {
    const int t = i / dm, k = i % dm;
    const T* row = dec + ((long)n * L + t) * ld_dec;
    float v = 0.f;
    const bool weighted = (use_head_alpha & 1) || (k < dm - 3);
    for (int b = 0; b < nb; ++b) {
      const float s = to_f32(stat[((long)ns * nb + b) * dm + k]);
      float a = to_f32(row[dm + b]);
      if (use_head_alpha & 2) a = 1.0f / (1.0f + expf(-a));   // regularize_alpha = 'sigmoid' (model.py:973-974)
      v += weighted ? s * a : s;
    }
    out[((long)n * L + t) * dm + k] = to_f32(row[k]) + v;
  }
}

extern "C" int msmd_heads_static_mix(const void* dec, long ld_dec, const void* stat, float* out, int N, int L, int dm,
                                     int nb, int stat_batch, int use_head_alpha, int dtype, msmd_stream_t stream) {
  if (N <= 0 || L <= 0 || dm <= 3 || nb <= 0 || stat_batch <= 0) return 1;
  dim3 grid((L * dm + 255) / 256, N), block(256);
  return dispatch_dtype<float, f16_t, bf16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) T;
    hipLaunchKernelGGL(heads_mix_kernel<T>, grid, block, 0, (hipStream_t)stream, (const T*)dec, ld_dec, (const T*)stat,
                       out, L, dm, nb, stat_batch, use_head_alpha);
    MSMD_RETURN_LAST();
  });
}

// ---------------------------------------------------------------------------------------------------
// The sampler's step kernels (DDPM, few-step solver, solver + diagnostic streams; each with host scalars or, kDev, with the
// per-step coefficients read from device memory) share what follows: the element's place, the CFG combine, the solver
// update and the grid.  One grid-stride loop over the B L dm elements of the last L frames each; fp32 throughout.
struct StepElem {
  int b, t, k;     // batch entry, frame among the last L, motion column of element i
  long off;        // the element inside entry 0's (B, Lp + L, dm) slice of res
  long stride_e;   // from one CFG entry's slice to the next
};
__device__ __forceinline__ StepElem step_elem(long i, int B, int L, int Lp, int dm) {
  const int b = (int)(i / ((long)L * dm));
  const int rem = (int)(i % ((long)L * dm));
  const int t = rem / dm, k = rem % dm;
  const long stride_e = (long)B * (Lp + L) * dm;
  const long off = ((long)b * (Lp + L) + Lp + t) * dm + k;
  return StepElem{b, t, k, off, stride_e};
}
static dim3 step_grid(long total) { return dim3((unsigned)min((total + 255) / 256, (long)2048)); }

// CFG combine.  The reference accumulates theta IN PLACE into entry 0's slice (model.py:407-415): `results[0]` IS the
// running theta, so
//   incremental: theta += s_e * (r[e+1] - r[e])   with r[0] := running theta when e == 0,
//   independent: theta += s_e * (r[e+1] - theta)  (later terms see the already-updated entry 0).
__device__ __forceinline__ float cfg_theta(const float* __restrict__ res, const float* __restrict__ scales,
                                           const StepElem& s, int n_entries, int mode) {
  const long stride_e = s.stride_e, off = s.off;
  float theta = res[off];
  for (int e = 0; e < n_entries - 1; ++e) {
    const float hi = res[(e + 1) * stride_e + off];
    const float lo = (mode == 1 || e == 0) ? theta : res[e * stride_e + off];
    theta += scales[e] * (hi - lo);
  }
  return theta;
}

// CFG combine + DDPM posterior step, in place on x (B, L, dm).  kDev: (c0, c1, sigma) = coefs[0..2], the triple
// msmd_sampler_step_select left on the device (a captured step body takes no per-step host scalars).
struct DdpmCoefs {
  float c0, c1, sigma;
};

template <bool kDev>
__global__ void cfg_ddpm_kernel(float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ z,
                                const float* __restrict__ scales, const float* __restrict__ coefs, DdpmCoefs c,
                                int n_entries, int B, int L, int Lp, int dm, int mode, int target) {
  if (kDev) c = DdpmCoefs{coefs[0], coefs[1], coefs[2]};
  const float c0 = c.c0, c1 = c.c1, sigma = c.sigma;
  const long total = (long)B * L * dm;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const float theta = cfg_theta(res, scales, step_elem(i, B, L, Lp, dm), n_entries, mode);
    const float xt = x[i];
    const float zz = z ? z[i] : 0.f;
    x[i] = (target == 0) ? (c0 * xt + c1 * theta + sigma * zz) : (c0 * (xt - c1 * theta) + sigma * zz);
  }
}

static int launch_cfg_ddpm(bool dev, float* x, const float* res, const float* z, const float* scales,
                           const float* coefs, DdpmCoefs c, int n_entries, int B, int L, int Lp, int dm, int mode,
                           int target, msmd_stream_t stream) {
  if (B <= 0 || L <= 0 || dm <= 0 || n_entries < 1 || (n_entries > 1 && !scales) || (dev && !coefs)) return 1;
  const dim3 grid = step_grid((long)B * L * dm), block(256);
  if (dev)
    hipLaunchKernelGGL(cfg_ddpm_kernel<true>, grid, block, 0, (hipStream_t)stream, x, res, z, scales, coefs, c,
                       n_entries, B, L, Lp, dm, mode, target);
  else
    hipLaunchKernelGGL(cfg_ddpm_kernel<false>, grid, block, 0, (hipStream_t)stream, x, res, z, scales, coefs, c,
                       n_entries, B, L, Lp, dm, mode, target);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_cfg_ddpm_step(float* x, const float* res, const float* z, const float* scales, int n_entries,
                                  int B, int L, int Lp, int dm, int mode, int target, float c0, float c1, float sigma,
                                  msmd_stream_t stream) {
  return launch_cfg_ddpm(false, x, res, z, scales, nullptr, DdpmCoefs{c0, c1, sigma}, n_entries, B, L, Lp, dm, mode,
                         target, stream);
}

extern "C" int msmd_cfg_ddpm_step_dev(float* x, const float* res, const float* z, const float* scales,
                                      const float* coefs, int n_entries, int B, int L, int Lp, int dm, int mode,
                                      int target, msmd_stream_t stream) {
  return launch_cfg_ddpm(true, x, res, z, scales, coefs, DdpmCoefs{}, n_entries, B, L, Lp, dm, mode, target, stream);
}

// ---------------------------------------------------------------------------------------------------
// hipGraph support for the sampler: the captured step body must not take per-step host scalars, so the step
// index lives on the device.  step_select copies row t of the step-embedding table and the (c0, c1, sigma)
// triple of step t into fixed buffers and then decrements t; the kDev step kernels read the triple from there.
// NC = 3 for the DDPM triple, 6 for a few-step solver row (msmd_sampler_solver_select).
template <typename T, int NC = 3>
__global__ void step_select_kernel(const T* __restrict__ emb_all, const float* __restrict__ coef_table,
                                   int* __restrict__ t_dev, T* __restrict__ emb_row, float* __restrict__ coefs, int d) {
  const int t = *t_dev;
  __syncthreads();
  for (int i = threadIdx.x; i < d; i += blockDim.x) emb_row[i] = emb_all[(long)t * d + i];
  if (threadIdx.x < NC) coefs[threadIdx.x] = coef_table[t * NC + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) *t_dev = t - 1;
}

template <int NC>
static int launch_step_select(const void* emb_all, const float* coef_table, int* t_dev, void* emb_row, float* coefs,
                              int d, int dtype, msmd_stream_t stream) {
  if (d <= 0 || !emb_all || !coef_table || !t_dev || !emb_row || !coefs) return 1;
  return dispatch_dtype<float, f16_t, bf16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) T;
    hipLaunchKernelGGL((step_select_kernel<T, NC>), dim3(1), dim3(256), 0, (hipStream_t)stream, (const T*)emb_all,
                       coef_table, t_dev, (T*)emb_row, coefs, d);
    MSMD_RETURN_LAST();
  });
}

extern "C" int msmd_sampler_step_select(const void* emb_all, const float* coef_table, int* t_dev, void* emb_row,
                                        float* coefs, int d, int dtype, msmd_stream_t stream) {
  return launch_step_select<3>(emb_all, coef_table, t_dev, emb_row, coefs, d, dtype, stream);
}

extern "C" int msmd_sampler_solver_select(const void* emb_tab, const float* coef_tab, int* i_dev, void* emb_row,
                                          float* coefs, int d, int dtype, msmd_stream_t stream) {
  return launch_step_select<6>(emb_tab, coef_tab, i_dev, emb_row, coefs, d, dtype, stream);
}

// ---------------------------------------------------------------------------------------------------
// Few-step solvers (DDIM(eta), DPM-Solver++(2M)) in data-prediction form.  The CFG combine is cfg_theta, as in
// cfg_ddpm_kernel; then, with the six per-step scalars (p0, p1, ax, ath, b1, sigma) folded on the
// host in float64 (sampler.solver_table):
//   D = p0 x + p1 theta                       (the x0 prediction: p0 = 0, p1 = 1 for target 'sample')
//   x <- ax x + ath theta + b1 d_prev + sigma z,   d_prev <- D
// Elementwise and bound by HBM bandwidth: per element 4 B of x, 4 B of d_prev, 4 B of z (when drawn) and 4 B per CFG
// entry of res are read, 8 B (x, d_prev) written -- 32 B at 3 entries, 13.7 MB per step at B = 64 (a few us against a
// ~2 ms denoiser call), so a grid-stride loop like its neighbour's is enough.
struct SolverCoefs {
  float p0, p1, ax, ath, b1, sigma;
};
// -> the new x; D = the x0 prediction (the new d_prev)
__device__ __forceinline__ float solver_update(const SolverCoefs& c, float xt, float theta, float dp, float zz, float& D) {
  D = c.p0 * xt + c.p1 * theta;
  return c.ax * xt + c.ath * theta + c.b1 * dp + c.sigma * zz;
}

template <bool kDev>
__global__ void cfg_solver_kernel(float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ z,
                                  const float* __restrict__ scales, float* __restrict__ d_prev,
                                  const float* __restrict__ coefs, SolverCoefs c, int n_entries, int B, int L, int Lp,
                                  int dm, int mode) {
  if (kDev) c = SolverCoefs{coefs[0], coefs[1], coefs[2], coefs[3], coefs[4], coefs[5]};
  const long total = (long)B * L * dm;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const float theta = cfg_theta(res, scales, step_elem(i, B, L, Lp, dm), n_entries, mode);
    const float xt = x[i];
    const float dp = d_prev[i];
    const float zz = z ? z[i] : 0.f;
    float D;
    x[i] = solver_update(c, xt, theta, dp, zz, D);
    d_prev[i] = D;
  }
}

static int launch_cfg_solver(bool dev, float* x, const float* res, const float* z, const float* scales, float* d_prev,
                             const float* coefs, SolverCoefs c, int n_entries, int B, int L, int Lp, int dm, int mode,
                             msmd_stream_t stream) {
  if (B <= 0 || L <= 0 || dm <= 0 || Lp < 0 || n_entries < 1 || (n_entries > 1 && !scales) || !x || !res || !d_prev ||
      (dev && !coefs))
    return 1;
  const dim3 grid = step_grid((long)B * L * dm), block(256);
  if (dev)
    hipLaunchKernelGGL(cfg_solver_kernel<true>, grid, block, 0, (hipStream_t)stream, x, res, z, scales, d_prev, coefs,
                       c, n_entries, B, L, Lp, dm, mode);
  else
    hipLaunchKernelGGL(cfg_solver_kernel<false>, grid, block, 0, (hipStream_t)stream, x, res, z, scales, d_prev,
                       coefs, c, n_entries, B, L, Lp, dm, mode);
  MSMD_RETURN_LAST();
}

extern "C" int msmd_cfg_solver_step(float* x, const float* res, const float* z, const float* scales, float* d_prev,
                                    int n_entries, int B, int L, int Lp, int dm, int mode, float p0, float p1, float ax,
                                    float ath, float b1, float sigma, msmd_stream_t stream) {
  return launch_cfg_solver(false, x, res, z, scales, d_prev, nullptr, SolverCoefs{p0, p1, ax, ath, b1, sigma},
                           n_entries, B, L, Lp, dm, mode, stream);
}

extern "C" int msmd_cfg_solver_step_dev(float* x, const float* res, const float* z, const float* scales,
                                        float* d_prev, const float* coefs, int n_entries, int B, int L, int Lp, int dm,
                                        int mode, msmd_stream_t stream) {
  return launch_cfg_solver(true, x, res, z, scales, d_prev, coefs, SolverCoefs{}, n_entries, B, L, Lp, dm, mode,
                           stream);
}

// ---------------------------------------------------------------------------------------------------
// sample_separate on a few-step solver: the CFG combine and solver update of cfg_solver_kernel (solver_update itself, so x and
// d_prev have its bits under the same res) plus, in the same launch, the three diagnostic streams of reference
// model.py:442-651.  Per element of the last L frames and per CFG entry e (row n = e B + b of dec / res):
//   dyn_e = dec[n][k],  static_e = sum_b a_{e,b} stat_b[k]  (the loop of heads_mix_kernel: same order, plain sum of the bases
//   for the last 3 columns without use_head_alpha & 1, sigmoid under use_head_alpha & 2),  alpha_e = a_{e,k} for k < nb;
// each stream is CFG-combined across entries by the in-place rule of cfg_theta.  The four streams share ONE pass over the
// entries and over scales, so theta is combined in that loop too and not by a call (which would read scales twice): its
// lines there are cfg_theta's, entry for entry.  res is the output of
// msmd_heads_static_mix (after msmd_dynamic_threshold when that is on), so theta is what the plain solver step sees.
//   cum_static += ath theta_static   (the step's coefficient on theta stands where the DDPM chain has c1, model.py:590-618)
//   theta_dyn (B, L, dm) is overwritten;  theta_alpha goes to rows [slot B, (slot + 1) B) of an (n_slots B, L, nb) buffer,
//   slot = 0 for n_slots = 1, else the step ordinal S - i (kDev: i = *step_dev + 1, the counter msmd_sampler_solver_select
//   has just decremented).
// Elementwise and HBM-bound like its neighbours: one grid-stride loop, fp32 throughout, running values instead of
// per-entry arrays (no scratch).
template <typename T, bool kDev>
__global__ void cfg_streams_kernel(float* __restrict__ x, const float* __restrict__ res, const T* __restrict__ dec,
                                   long ld_dec, const T* __restrict__ stat, const float* __restrict__ z,
                                   const float* __restrict__ scales, float* __restrict__ d_prev,
                                   float* __restrict__ cum_static, float* __restrict__ theta_dyn,
                                   float* __restrict__ theta_alpha, const float* __restrict__ coefs,
                                   const int* __restrict__ step_dev, SolverCoefs c, int slot, int n_slots,
                                   int n_entries, int B, int L, int Lp, int dm, int nb, int stat_batch,
                                   int use_head_alpha, int mode) {
  if (kDev) {
    c = SolverCoefs{coefs[0], coefs[1], coefs[2], coefs[3], coefs[4], coefs[5]};
    slot = n_slots > 1 ? n_slots - (*step_dev + 1) : 0;
  }
  if (slot < 0 || slot >= n_slots) slot = n_slots - 1;   // a counter outside the loop's range must not write out of bounds
  const long total = (long)B * L * dm;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const auto [b, t, k, off, stride_e] = step_elem(i, B, L, Lp, dm);
    const bool weighted = (use_head_alpha & 1) || (k < dm - 3);
    float theta = 0.f, th_static = 0.f, th_dyn = 0.f, th_alpha = 0.f;
    float lo_static = 0.f, lo_dyn = 0.f, lo_alpha = 0.f;   // entry e's own values while entry e + 1 is combined
    for (int e = 0; e < n_entries; ++e) {
      const int n = e * B + b;
      const int ns = n % stat_batch;
      const T* row = dec + ((long)n * (Lp + L) + Lp + t) * ld_dec;
      float st = 0.f, al = 0.f;
      for (int bb = 0; bb < nb; ++bb) {
        const float s = to_f32(stat[((long)ns * nb + bb) * dm + k]);
        float a = to_f32(row[dm + bb]);
        if (use_head_alpha & 2) a = 1.0f / (1.0f + expf(-a));
        st += weighted ? s * a : s;
        if (bb == k) al = a;
      }
      const float dy = to_f32(row[k]);
      if (e == 0) {
        theta = res[off];
        th_static = st; th_dyn = dy; th_alpha = al;
      } else {
        const float sc = scales[e - 1];
        const bool running = (mode == 1 || e == 1);        // lo = the running theta (entry 0's slice, updated in place)
        const float hi = res[e * stride_e + off];                          // these three lines: cfg_theta's, at its e + 1
        const float lo = running ? theta : res[(e - 1) * stride_e + off];
        theta += sc * (hi - lo);
        th_static += sc * (st - (running ? th_static : lo_static));
        th_dyn += sc * (dy - (running ? th_dyn : lo_dyn));
        th_alpha += sc * (al - (running ? th_alpha : lo_alpha));
      }
      lo_static = st; lo_dyn = dy; lo_alpha = al;
    }
    const float xt = x[i];
    const float dp = d_prev[i];
    const float zz = z ? z[i] : 0.f;
    float D;
    x[i] = solver_update(c, xt, theta, dp, zz, D);
    d_prev[i] = D;
    cum_static[i] += c.ath * th_static;
    theta_dyn[i] = th_dyn;
    if (k < nb) theta_alpha[(((long)slot * B + b) * L + t) * nb + k] = th_alpha;
  }
}

static int launch_cfg_streams(bool dev, float* x, const float* res, const void* dec, long ld_dec, const void* stat,
                              const float* z, const float* scales, float* d_prev, float* cum_static, float* theta_dyn,
                              float* theta_alpha, const float* coefs, const int* step_dev, SolverCoefs c, int slot,
                              int n_slots, int n_entries, int B, int L, int Lp, int dm, int nb, int stat_batch,
                              int use_head_alpha, int mode, int dtype, msmd_stream_t stream) {
  if (B <= 0 || L <= 0 || dm <= 3 || Lp < 0 || nb <= 0 || nb > dm || n_entries < 1 || (n_entries > 1 && !scales) || !x ||
      !res || !dec || !stat || !d_prev || !cum_static || !theta_dyn || !theta_alpha || ld_dec < dm + nb ||
      (stat_batch != B && stat_batch != 1 && stat_batch != n_entries * B) || n_slots < 1 ||
      (dev ? (!coefs || !step_dev) : (slot < 0 || slot >= n_slots)))
    return 1;
  const dim3 grid = step_grid((long)B * L * dm), block(256);
  return dispatch_dtype<float, f16_t, bf16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) T;
    if (dev)
      hipLaunchKernelGGL((cfg_streams_kernel<T, true>), grid, block, 0, (hipStream_t)stream, x, res, (const T*)dec, ld_dec,
                         (const T*)stat, z, scales, d_prev, cum_static, theta_dyn, theta_alpha, coefs, step_dev, c, slot,
                         n_slots, n_entries, B, L, Lp, dm, nb, stat_batch, use_head_alpha, mode);
    else
      hipLaunchKernelGGL((cfg_streams_kernel<T, false>), grid, block, 0, (hipStream_t)stream, x, res, (const T*)dec, ld_dec,
                         (const T*)stat, z, scales, d_prev, cum_static, theta_dyn, theta_alpha, coefs, step_dev, c, slot,
                         n_slots, n_entries, B, L, Lp, dm, nb, stat_batch, use_head_alpha, mode);
    MSMD_RETURN_LAST();
  });
}

extern "C" int msmd_cfg_streams_step(float* x, const float* res, const void* dec, long ld_dec, const void* stat,
                                     const float* z, const float* scales, float* d_prev, float* cum_static,
                                     float* theta_dyn, float* theta_alpha, int slot, int n_slots, int n_entries, int B,
                                     int L, int Lp, int dm, int nb, int stat_batch, int use_head_alpha, int mode,
                                     int dtype, float p0, float p1, float ax, float ath, float b1, float sigma,
                                     msmd_stream_t stream) {
  return launch_cfg_streams(false, x, res, dec, ld_dec, stat, z, scales, d_prev, cum_static, theta_dyn, theta_alpha,
                            nullptr, nullptr, SolverCoefs{p0, p1, ax, ath, b1, sigma}, slot, n_slots, n_entries, B, L, Lp,
                            dm, nb, stat_batch, use_head_alpha, mode, dtype, stream);
}

extern "C" int msmd_cfg_streams_step_dev(float* x, const float* res, const void* dec, long ld_dec, const void* stat,
                                         const float* z, const float* scales, float* d_prev, float* cum_static,
                                         float* theta_dyn, float* theta_alpha, const float* coefs, const int* step_dev,
                                         int n_slots, int n_entries, int B, int L, int Lp, int dm, int nb,
                                         int stat_batch, int use_head_alpha, int mode, int dtype,
                                         msmd_stream_t stream) {
  return launch_cfg_streams(true, x, res, dec, ld_dec, stat, z, scales, d_prev, cum_static, theta_dyn, theta_alpha, coefs,
                            step_dev, SolverCoefs{}, 0, n_slots, n_entries, B, L, Lp, dm, nb, stat_batch, use_head_alpha,
                            mode, dtype, stream);
}

// ---------------------------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ void pad_cols_kernel(const TI* __restrict__ x, TO* __restrict__ y, long rows, int ci, int co) {
  const long total = rows * co;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / co;
    const int c = (int)(i % co);
    y[i] = from_f32<TO>(c < ci ? to_f32(x[r * ci + c]) : 0.f);
  }
}

extern "C" int msmd_pad_cols(const void* x, void* y, long rows, int cols_in, int cols_out, int in_dtype, int out_dtype,
                             msmd_stream_t stream) {
  if (rows <= 0 || cols_in <= 0 || cols_out <= 0) return 1;
  const long total = rows * cols_out;
  dim3 grid((unsigned)min((total + 255) / 256, (long)4096)), block(256);
  return dispatch_dtype<float, f16_t, bf16_t>(in_dtype, [&](auto ti) {
    return dispatch_dtype<float, f16_t, bf16_t>(out_dtype, [&](auto to) {
      typedef MSMD_TAG_T(ti) TI;
      typedef MSMD_TAG_T(to) TO;
      if constexpr (kStoragePair<TI, TO>) {
        hipLaunchKernelGGL((pad_cols_kernel<TI, TO>), grid, block, 0, (hipStream_t)stream, (const TI*)x, (TO*)y, rows,
                           cols_in, cols_out);
        MSMD_RETURN_LAST();
      } else {
        return 1;
      }
    });
  });
}

extern "C" int msmd_cast(const void* x, void* y, long n, int in_dtype, int out_dtype, msmd_stream_t stream) {
  if (n <= 0 || n > 0x7fffffffL) return 1;
  return msmd_pad_cols(x, y, 1, (int)n, (int)n, in_dtype, out_dtype, stream);
}

// ---------------------------------------------------------------------------------------------------
// msmd_denoiser_prepare: everything the denoiser's forward lays out before its first GEMM, in ONE launch.  The five outputs
// are independent of each other, so the grid is cut into five block ranges ("roles"), each a grid-stride loop over units of 8
// output elements (one 16-byte store) of its own buffer:
//   feats  pack_input_value, with c0 / c1 gathered from the schedule tables at ts[clip]
//   mem    rows [0, Lpa) of every sequence <- prev_audio (fp32), batch stride 0 = the broadcast start rows
//   emb    row ts[n] of the step-embedding table, 16-byte copies
//   pf     [person_a | person_b | zeros] per row: msmd_pad_cols' conversion
//   style  flat fp32 -> storage type: msmd_cast's conversion (the last unit may be short)
// The roles' first-past-the-end blocks are cumulative in `end`; a role with nothing to do has an empty range.
struct PrepareArgs {
  PackInput pack;
  const float* t0; const float* t1; const long* ts; int n_steps;
  const float* prev_audio; long prev_audio_stride, mem_stride; int Lpa, d;
  const void* emb_table;
  const float* person_a; const float* person_b; int cols_a, cols_b, kp_person;
  const float* style; long style_n;
  void* feats; void* mem; void* emb; void* pf; void* style_out;
  int N, end[5];
};

// a time step as a row of a (n_steps, ...) table: an index outside the table reads its nearest end, never past it
__device__ __forceinline__ int prepare_step(const PrepareArgs& p, int n) {
  const long t = p.ts[n];
  return (int)(t < 0 ? 0 : (t >= p.n_steps ? p.n_steps - 1 : t));
}

template <typename TO>
__global__ __launch_bounds__(256) void denoiser_prepare_kernel(PrepareArgs p) {
  typedef typename Vec8T<TO>::type V8;
  const int b = blockIdx.x;
  if (b < p.end[0]) {
    const int per_seq = (1 + p.pack.Lp + p.pack.L) * p.pack.Kpad;
    const long units = (long)p.N * (per_seq >> 3);
    for (long u = b * 256L + threadIdx.x; u < units; u += p.end[0] * 256L) {
      const int n = (int)(u / (per_seq >> 3)), i = (int)(u % (per_seq >> 3)) << 3;
      float c0 = 0.f, c1 = 0.f;
      if (p.pack.eps) {
        const int step = prepare_step(p, n % p.pack.motion_batch);
        c0 = p.t0[step];
        c1 = p.t1[step];
      }
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = from_f32<TO>(pack_input_value(p.pack, n, i + e, c0, c1));
      *(V8*)((TO*)p.feats + (long)n * per_seq + i) = o;
    }
  } else if (b < p.end[1]) {
    const int per_seq = p.Lpa * p.d;
    const long units = (long)p.N * (per_seq >> 3);
    const int nb = p.end[1] - p.end[0];
    for (long u = (b - p.end[0]) * 256L + threadIdx.x; u < units; u += nb * 256L) {
      const int n = (int)(u / (per_seq >> 3)), i = (int)(u % (per_seq >> 3)) << 3;
      const float* src = p.prev_audio + (long)n * p.prev_audio_stride + i;
      const f32x4 lo = *(const f32x4*)src, hi = *(const f32x4*)(src + 4);
      V8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] = from_f32<TO>(lo[e]); o[4 + e] = from_f32<TO>(hi[e]); }
      *(V8*)((TO*)p.mem + (long)n * p.mem_stride + i) = o;
    }
  } else if (b < p.end[2]) {
    const int per_row = p.d >> 3;
    const long units = (long)p.N * per_row;
    const int nb = p.end[2] - p.end[1];
    for (long u = (b - p.end[1]) * 256L + threadIdx.x; u < units; u += nb * 256L) {
      const int n = (int)(u / per_row), c = (int)(u % per_row) << 3;
      *(V8*)((TO*)p.emb + (long)n * p.d + c) = *(const V8*)((const TO*)p.emb_table + (long)prepare_step(p, n) * p.d + c);
    }
  } else if (b < p.end[3]) {
    const int per_row = p.kp_person >> 3;
    const long units = (long)p.N * per_row;
    const int nb = p.end[3] - p.end[2];
    for (long u = (b - p.end[2]) * 256L + threadIdx.x; u < units; u += nb * 256L) {
      const int n = (int)(u / per_row), c0 = (int)(u % per_row) << 3;
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        float v = 0.f;
        if (c < p.cols_a) v = p.person_a[(long)n * p.cols_a + c];
        else if (c < p.cols_a + p.cols_b) v = p.person_b[(long)n * p.cols_b + (c - p.cols_a)];
        o[e] = from_f32<TO>(v);
      }
      *(V8*)((TO*)p.pf + (long)n * p.kp_person + c0) = o;
    }
  } else {
    const long units = (p.style_n + 7) >> 3;
    const int nb = p.end[4] - p.end[3];
    for (long u = (b - p.end[3]) * 256L + threadIdx.x; u < units; u += nb * 256L) {
      const long i = u << 3;
      if (i + 8 <= p.style_n) {
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = from_f32<TO>(p.style[i + e]);
        *(V8*)((TO*)p.style_out + i) = o;
      } else {
        for (long j = i; j < p.style_n; ++j) ((TO*)p.style_out)[j] = from_f32<TO>(p.style[j]);
      }
    }
  }
}

extern "C" int msmd_denoiser_prepare(const float* motion, const float* eps, const float* t0, const float* t1, const long* ts,
                                     int n_steps, const float* prev_motion, long prev_motion_stride, const float* indicator,
                                     void* feats, int N, int L, int Lp, int dm, int Kpad, const float* person_a, int cols_a,
                                     const float* person_b, int cols_b, void* pf, int kp_person, const float* style,
                                     long style_n, void* style_out, const void* emb_table, void* emb, int d,
                                     const float* prev_audio, long prev_audio_stride, int Lpa, void* mem, long mem_stride,
                                     int dtype, msmd_stream_t stream) {
  if (N <= 0 || L <= 0 || Lp < 0 || Lpa < 0 || dm <= 0 || Kpad < dm + (indicator ? 1 : 0) || n_steps <= 0 || d <= 0) return 1;
  if (!motion || !feats || !ts || !emb_table || !emb || !person_a || !pf || (Lp && !prev_motion)) return 1;
  if (eps && (!t0 || !t1)) return 1;
  if (Lpa && (!prev_audio || !mem)) return 1;
  if (cols_a <= 0 || cols_b < 0 || (cols_b && !person_b) || kp_person < cols_a + cols_b || style_n < 0) return 1;
  if (style_n && (!style || !style_out)) return 1;
  // whole 16-byte units: 8 storage elements out, 2 x 4 fp32 in
  if ((Kpad & 7) || (d & 7) || (kp_person & 7) || (mem_stride & 7) || (prev_audio_stride & 3) || mem_stride < (long)Lpa * d) return 1;
  if (prev_motion_stride != 0 && prev_motion_stride < (long)Lp * dm) return 1;
  if (prev_audio_stride != 0 && prev_audio_stride < (long)Lpa * d) return 1;
  if (((uintptr_t)feats | (uintptr_t)mem | (uintptr_t)emb | (uintptr_t)emb_table | (uintptr_t)pf | (uintptr_t)style_out |
       (uintptr_t)prev_audio) & 15)
    return 1;
  PrepareArgs p{};
  p.pack = PackInput{motion, eps, prev_motion, indicator, nullptr, nullptr, L, Lp, dm, Kpad, N, prev_motion_stride};
  p.t0 = t0; p.t1 = t1; p.ts = ts; p.n_steps = n_steps;
  p.prev_audio = prev_audio; p.prev_audio_stride = prev_audio_stride; p.mem_stride = mem_stride; p.Lpa = Lpa; p.d = d;
  p.emb_table = emb_table;
  p.person_a = person_a; p.person_b = person_b; p.cols_a = cols_a; p.cols_b = cols_b; p.kp_person = kp_person;
  p.style = style; p.style_n = style_n;
  p.feats = feats; p.mem = mem; p.emb = emb; p.pf = pf; p.style_out = style_out;
  p.N = N;
  // blocks by the bytes of a role (one 16-byte unit per thread and trip), at most 256 for the largest: launch-bound work
  const long units[5] = {(long)N * (1 + Lp + L) * (Kpad >> 3), (long)N * Lpa * (d >> 3), (long)N * (d >> 3),
                         (long)N * (kp_person >> 3), (style_n + 7) >> 3};
  const int cap[5] = {256, 128, 16, 16, 16};
  int at = 0;
  for (int r = 0; r < 5; ++r) {
    at += (int)min((units[r] + 255) / 256, (long)cap[r]);
    p.end[r] = at;
  }
  return dispatch_dtype<f16_t, bf16_t>(dtype, [&](auto tag) {
    typedef MSMD_TAG_T(tag) TO;
    hipLaunchKernelGGL(denoiser_prepare_kernel<TO>, dim3(at), dim3(256), 0, (hipStream_t)stream, p);
    MSMD_RETURN_LAST();
  });
}

extern "C" int msmd_abi_version(void) { return 2; }   // 2: + msmd_comm_* / msmd_allreduce_bucket (round 4), msmd_comm_version

// ---------------------------------------------------------------------------------------------------
// Dynamic thresholding of the denoiser output (reference model.py:396-402, 578-584):
//   s_n = clamp(quantile_q(|res[n, -L:, :]|), dt_min, dt_max);   res[n] <- clamp(res[n], -s_n, s_n)
// torch.quantile's default 'linear' rule: rank = q (m - 1), lerp between the floor / ceil order statistics.
// One 1024-thread workgroup per sequence keeps the m = L C magnitudes in registers and finds the order statistic by
// bisection on the (non-negative) float bit pattern: 31 rounds of count(x <= mid) instead of a sort.
template <int MAXE>
__global__ __launch_bounds__(1024) void dynamic_threshold_kernel(float* __restrict__ res, int T_all, int L, int C,
                                                                  float q, float dt_min, float dt_max) {
  __shared__ int red[16];
  __shared__ unsigned redu[16];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float* base = res + (long)n * T_all * C;
  const float* tail = base + (long)(T_all - L) * C;
  const int m = L * C;
  unsigned v[MAXE];
#pragma unroll
  for (int e = 0; e < MAXE; ++e) {
    const int i = e * 1024 + tid;
    v[e] = i < m ? (__float_as_uint(tail[i]) & 0x7FFFFFFFu) : 0xFFFFFFFFu;  // padding sorts last
  }
  auto count_le = [&](unsigned x) {
    int c = 0;
#pragma unroll
    for (int e = 0; e < MAXE; ++e) c += (v[e] <= x) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __syncthreads();
    if (lane == 0) red[wid] = c;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];
    return t;
  };
  const float rank = q * (float)(m - 1);
  const int k = (int)floorf(rank);
  const float w = rank - (float)k;
  unsigned lo = 0u, hi = 0x7F800000u;  // smallest x with count(<= x) >= k + 1
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (count_le(mid) >= k + 1) hi = mid; else lo = mid + 1;
  }
  const unsigned b_lo = lo;
  unsigned b_hi = b_lo;
  if (w > 0.f && count_le(b_lo) < k + 2) {  // next order statistic = smallest value above b_lo
    unsigned mn = 0xFFFFFFFFu;
#pragma unroll
    for (int e = 0; e < MAXE; ++e) mn = (v[e] > b_lo && v[e] < mn) ? v[e] : mn;
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, (unsigned)__shfl_xor((int)mn, o, 64));
    __syncthreads();
    if (lane == 0) redu[wid] = mn;
    __syncthreads();
#pragma unroll
    for (int ww = 0; ww < 16; ++ww) mn = min(mn, redu[ww]);
    b_hi = mn;
  }
  const float a = __uint_as_float(b_lo), b = __uint_as_float(b_hi);
  // ATen lerp: a + w (b - a) for w < 0.5, else b - (b - a)(1 - w)
  float sq = (w < 0.5f) ? a + w * (b - a) : b - (b - a) * (1.0f - w);
  sq = fminf(fmaxf(sq, dt_min), dt_max);
  for (int i = tid; i < T_all * C; i += 1024) base[i] = fminf(fmaxf(base[i], -sq), sq);
}

extern "C" int msmd_dynamic_threshold(float* res, int N, int T_all, int L, int C, float ratio, float dt_min,
                                      float dt_max, msmd_stream_t stream) {
  if (N <= 0 || L <= 0 || T_all < L || C <= 0 || !(ratio >= 0.f && ratio <= 1.f)) return 1;
  const long m = (long)L * C;
  hipStream_t st = (hipStream_t)stream;
  if (m <= 8 * 1024)
    hipLaunchKernelGGL(dynamic_threshold_kernel<8>, dim3(N), dim3(1024), 0, st, res, T_all, L, C, ratio, dt_min, dt_max);
  else if (m <= 20 * 1024)
    hipLaunchKernelGGL(dynamic_threshold_kernel<20>, dim3(N), dim3(1024), 0, st, res, T_all, L, C, ratio, dt_min, dt_max);
  else
    return 1;
  MSMD_RETURN_LAST();
}
