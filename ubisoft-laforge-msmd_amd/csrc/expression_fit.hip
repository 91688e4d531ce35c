// Expression code and jaw pose from model-space landmarks (include/msmd_hip.h states the model and the solver):
// a per-frame Levenberg-Marquardt fit of FLAME's expression e (NE) and jaw axis-angle theta to K landmarks, fixed work, frames
// independent.  Everything between the fp32 landmarks and the fp32 outputs is float64.
//
// One wave per frame, EF_FRAMES waves per workgroup.  The reduced model -- per landmark six rows (X then Y, three coordinates
// each) of NC = NE + 9 coefficients over [e | vec(R - I)] -- passes through LDS EF_KS landmarks at a time, staged once for the
// workgroup's frames; the constant column is per subject and is read where it is.  Per slice and wave:
//   A  lane = table row: the row's value at the point (X_k, Y_k) and its product with each d vec(R) / d theta_a
//   r  lane = (landmark, coordinate): l = X + (R - I) Y, the residual, sqrt(w) r into LDS, w r^2 summed
//   B  lane = parameter: its column of sqrt(w) Jm for the slice's 3 EF_KS rows into LDS, and g += column . sqrt(w) r
//   C  lane (ti, tj) of an 8 x 8 grid holds H[8 a + ti][8 b + tj], a, b < 8, in registers: rank-(3 EF_KS) update from LDS
// The Cholesky factorisation stays in that cyclic register layout and the factor goes to LDS packed by columns, over the dead
// Jm slice, for the two triangular solves with one row per lane (wave_chol.h, shared with retarget.hip).  A wave's LDS traffic
// is ordered by the hardware, so inside a wave a fence suffices; the workgroup barriers are those of the staging alone, and
// every wave passes the same number of them whatever its frame does.
#include "common.h"
#include "wave_chol.h"

constexpr int EF_WG = 256;
constexpr int EF_FRAMES = EF_WG / MSMD_WAVE;       // frames per workgroup
constexpr int EF_KS = 4;                           // landmarks per staged slice: with 8 a workgroup's LDS leaves a CU one workgroup
constexpr int EF_ROWS = 3 * EF_KS;                 // rows of Jm per slice
constexpr int EF_TROWS = 6 * EF_KS;                // table rows per slice
constexpr int EF_NP = 64;                          // parameters, padded: one per lane
static_assert(EF_FRAMES == MSMD_EXPFIT_FRAMES && MSMD_EXPFIT_MAX_EXP + 3 == EF_NP, "header and kernel disagree");
static_assert(EF_TROWS <= MSMD_WAVE, "one table row per lane");

struct ExpFitArgs {
  const float* landmarks;      // (n, K, 3)
  const int* subject;          // (n)
  const double* tab;           // (K, 6, NC)
  const double* tab0;          // (S, K, 6)
  const double* w;             // (K)
  float* code;                 // (n, NE)
  float* jaw;                  // (n, 3)
  float* rms;                  // (n)
  int* status;                 // (n)
  int n, K, NE, S, jaw_dof, iterations;
  double lambda_exp, lambda_jaw;
};

// per-wave LDS, in doubles, after the shared part
constexpr int EF_OFF_P = 0;                        // the point, one parameter per lane (64)
constexpr int EF_OFF_ROT = EF_OFF_P + 64;          // R - I (9), then d R / d theta_a (3 x 9)
constexpr int EF_OFF_VAL = EF_OFF_ROT + 36;        // table rows' values (EF_TROWS)
constexpr int EF_OFF_DVAL = EF_OFF_VAL + EF_TROWS; // their products with d vec(R) / d theta_a (3 x EF_TROWS)
constexpr int EF_OFF_RS = EF_OFF_DVAL + 3 * EF_TROWS;
constexpr int EF_OFF_COL = EF_OFF_RS + EF_ROWS;    // Cholesky: the step's column (64) and pivot (1)
constexpr int EF_OFF_BIG = EF_OFF_COL + WCHOL_COL;       // the Jm slice (EF_ROWS x 64), later the packed factor
__host__ __device__ constexpr int ef_big(int NP) { return NP * (NP + 1) / 2 > EF_ROWS * 64 ? NP * (NP + 1) / 2 : EF_ROWS * 64; }
__host__ __device__ constexpr int ef_ncs(int NC) { return NC | 1; }            // odd row pitch: one row per lane meets no bank twice
__host__ __device__ constexpr int ef_shared(int NC) { return EF_TROWS * ef_ncs(NC) + MSMD_EXPFIT_MAX_LANDMARKS + 8; }

// R - I and d R / d theta_a of utils/lbs.py's Rodrigues formula: angle = |theta + 1e-8|, direction = theta / angle.
__device__ __forceinline__ void rodrigues_jet(const double* th, double* out) {
  const double eps = 1e-8;
  const double t0 = th[0] + eps, t1 = th[1] + eps, t2 = th[2] + eps;
  const double al = sqrt(t0 * t0 + t1 * t1 + t2 * t2), ia = 1.0 / al;
  const double d[3] = {th[0] * ia, th[1] * ia, th[2] * ia};
  const double s = sin(al), co = cos(al), sh = sin(0.5 * al), c1 = 2.0 * sh * sh;
  const double Km[9] = {0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0};
  double K2[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) K2[i * 3 + j] = Km[i * 3] * Km[j] + Km[i * 3 + 1] * Km[3 + j] + Km[i * 3 + 2] * Km[6 + j];
#pragma unroll
  for (int m = 0; m < 9; ++m) out[m] = s * Km[m] + c1 * K2[m];
  const double tt[3] = {t0, t1, t2};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double aa = tt[a] * ia;                   // d angle / d theta_a
    double dd[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) dd[k] = (k == a ? ia : 0.0) - th[k] * aa * ia * ia;
    const double Ka[9] = {0, -dd[2], dd[1], dd[2], 0, -dd[0], -dd[1], dd[0], 0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double kak = Ka[i * 3] * Km[j] + Ka[i * 3 + 1] * Km[3 + j] + Ka[i * 3 + 2] * Km[6 + j];
        const double kka = Km[i * 3] * Ka[j] + Km[i * 3 + 1] * Ka[3 + j] + Km[i * 3 + 2] * Ka[6 + j];
        out[9 + a * 9 + i * 3 + j] = co * aa * Km[i * 3 + j] + s * Ka[i * 3 + j] + s * aa * K2[i * 3 + j] + c1 * (kak + kka);
      }
  }
}

struct ExpFitWave {
  double* sh_tab;       // shared: the staged slice
  const double* sh_sw;  // shared: sqrt(w)
  double* wv;           // this wave's LDS
  int lane, wid, frame, subj, NC, NCs, NP;
};

// Make `pv` (one parameter per lane, zero from NP on) the point the next pass evaluates: into LDS with its rotation.
__device__ __forceinline__ void ef_set_point(const ExpFitArgs& p, const ExpFitWave& W, double pv) {
  W.wv[EF_OFF_P + W.lane] = pv;
  wave_sync();
  const double th[3] = {p.jaw_dof >= 1 ? W.wv[EF_OFF_P + p.NE] : 0.0, p.jaw_dof == 3 ? W.wv[EF_OFF_P + p.NE + 1] : 0.0,
                        p.jaw_dof == 3 ? W.wv[EF_OFF_P + p.NE + 2] : 0.0};
  double rot[36];
  rodrigues_jet(th, rot);
  if (W.lane == 0) {
#pragma unroll
    for (int m = 0; m < 36; ++m) W.wv[EF_OFF_ROT + m] = rot[m];
  }
  wave_sync();
}

// One pass over the landmarks at the point in LDS: -> sum_k w_k |r_k|^2 (the same in every lane).  WITH_J: also acc = Jm^T W Jm
// in the cyclic layout and g = Jm^T W r, one parameter per lane.
template <bool WITH_J>
__device__ __forceinline__ double ef_pass(const ExpFitArgs& p, const ExpFitWave& W, double (&acc)[8][8], double& g) {
  const int lane = W.lane, K = p.K, NE = p.NE, NC = W.NC, NCs = W.NCs;
  double* __restrict__ wv = W.wv;
  double* __restrict__ sJ = wv + EF_OFF_BIG;
  const int ti = lane >> 3, tj = lane & 7;
  const int pos = ((lane & 7) << 3) + (lane >> 3);     // where parameter `lane` sits in a stored row of Jm
  double fsum = 0.0;
  if (WITH_J) {
    g = 0.0;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
  }
  double M[9];
#pragma unroll
  for (int m = 0; m < 9; ++m) M[m] = wv[EF_OFF_ROT + m];
  for (int k0 = 0; k0 < K; k0 += EF_KS) {
    __syncthreads();
    for (int row = W.wid; row < EF_TROWS; row += EF_FRAMES) {
      const bool in = k0 + row / 6 < K;
      const double* __restrict__ src = p.tab + ((long)k0 * 6 + row) * NC;
      for (int col = lane; col < NC; col += MSMD_WAVE) W.sh_tab[row * NCs + col] = in ? src[col] : 0.0;
    }
    __syncthreads();
    if (lane < EF_TROWS) {                                                             // A
      const int k = k0 + lane / 6;
      const double* __restrict__ t = W.sh_tab + lane * NCs;
      // two chains, eight products in flight: one lane's dot product is the longest dependent chain of the slice
      double base = k < K ? p.tab0[((long)W.subj * K + k0) * 6 + lane] : 0.0, base1 = 0.0;
      int j = 0;
      for (; j + 8 <= NE; j += 8) {
        double tv[8], pj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { tv[u] = t[j + u]; pj[u] = wv[EF_OFF_P + j + u]; }
#pragma unroll
        for (int u = 0; u < 8; u += 2) { base = fma(tv[u], pj[u], base); base1 = fma(tv[u + 1], pj[u + 1], base1); }
      }
      for (; j < NE; ++j) base = fma(t[j], wv[EF_OFF_P + j], base);
      base += base1;
      double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
      for (int m = 0; m < 9; ++m) {
        const double tp = t[NE + m];
        base = fma(tp, M[m], base);
        if (WITH_J) {
          d0 = fma(tp, wv[EF_OFF_ROT + 9 + m], d0);
          d1 = fma(tp, wv[EF_OFF_ROT + 18 + m], d1);
          d2 = fma(tp, wv[EF_OFF_ROT + 27 + m], d2);
        }
      }
      wv[EF_OFF_VAL + lane] = base;
      if (WITH_J) {
        wv[EF_OFF_DVAL + lane] = d0;
        wv[EF_OFF_DVAL + EF_TROWS + lane] = d1;
        wv[EF_OFF_DVAL + 2 * EF_TROWS + lane] = d2;
      }
    }
    wave_sync();
    if (lane < EF_ROWS) {                                                              // r
      const int kl = lane / 3, c = lane - kl * 3, k = k0 + kl;
      const double* __restrict__ v = wv + EF_OFF_VAL + kl * 6;
      const double* __restrict__ Mr = wv + EF_OFF_ROT + c * 3;           // row c of R - I (from LDS: c differs by lane)
      const double l = v[c] + Mr[0] * v[3] + Mr[1] * v[4] + Mr[2] * v[5];
      const bool in = k < K;
      const double y = in ? (double)p.landmarks[((long)W.frame * K + k) * 3 + c] : 0.0;
      const double sw = in ? W.sh_sw[k] : 0.0;
      const double rs = sw * (l - y);
      fsum = fma(rs, rs, fsum);
      if (WITH_J) wv[EF_OFF_RS + lane] = rs;
    }
    if (WITH_J) {
      wave_sync();
      const int ja = lane - NE;                                                        // B
      const bool is_e = lane < NE, is_j = !is_e && lane < W.NP;
#pragma unroll 1
      for (int kl = 0; kl < EF_KS; ++kl) {
        const double sw = k0 + kl < K ? W.sh_sw[k0 + kl] : 0.0;
        const double* __restrict__ v = wv + EF_OFF_VAL + kl * 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double jv = 0.0;
          if (is_e) {
            const double* __restrict__ t = W.sh_tab + (kl * 6) * NCs + lane;
            jv = t[c * NCs] + M[c * 3] * t[3 * NCs] + M[c * 3 + 1] * t[4 * NCs] + M[c * 3 + 2] * t[5 * NCs];
          } else if (is_j) {
            const double* __restrict__ dv = wv + EF_OFF_DVAL + ja * EF_TROWS + kl * 6;
            const double* __restrict__ dR = wv + EF_OFF_ROT + 9 + ja * 9 + c * 3;
            jv = dv[c] + dR[0] * v[3] + dR[1] * v[4] + dR[2] * v[5] + M[c * 3] * dv[3] + M[c * 3 + 1] * dv[4] + M[c * 3 + 2] * dv[5];
          }
          jv *= sw;
          sJ[(kl * 3 + c) * 64 + pos] = jv;
          g = fma(jv, wv[EF_OFF_RS + kl * 3 + c], g);
        }
      }
      wave_sync();
#pragma unroll 2
      for (int r = 0; r < EF_ROWS; ++r) {                                              // C
        double ja8[8], jb8[8];
#pragma unroll
        for (int a = 0; a < 8; ++a) { ja8[a] = sJ[r * 64 + ti * 8 + a]; jb8[a] = sJ[r * 64 + tj * 8 + a]; }
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) acc[a][b] = fma(ja8[a], jb8[b], acc[a][b]);
      }
    }
  }
  return wave_sum_f64(fsum);
}

__global__ __launch_bounds__(EF_WG) void expression_fit_kernel(const ExpFitArgs p) {
  extern __shared__ __attribute__((aligned(16))) double ef_smem[];
  const int tid = threadIdx.x;
  ExpFitWave W;
  W.lane = tid & 63;
  W.wid = tid >> 6;
  W.NC = p.NE + 9;
  W.NCs = ef_ncs(W.NC);
  W.NP = p.NE + p.jaw_dof;
  W.sh_tab = ef_smem;
  double* __restrict__ sh_sw = ef_smem + EF_TROWS * W.NCs;
  double* __restrict__ sh_misc = sh_sw + MSMD_EXPFIT_MAX_LANDMARKS;
  W.sh_sw = sh_sw;
  W.wv = ef_smem + ef_shared(W.NC) + W.wid * (EF_OFF_BIG + ef_big(W.NP));
  const long fr = (long)blockIdx.x * EF_FRAMES + W.wid;
  const bool live = fr < p.n;                       // a wave past the last frame refits that frame and writes nothing
  W.frame = (int)(live ? fr : p.n - 1);
  const int sj = p.subject[W.frame];
  W.subj = sj < 0 ? 0 : (sj >= p.S ? p.S - 1 : sj);
  const int lane = W.lane, NE = p.NE, NP = W.NP;

  if (tid < MSMD_EXPFIT_MAX_LANDMARKS) sh_sw[tid] = tid < p.K ? sqrt(p.w[tid]) : 0.0;
  if (W.wid == 0) {
    double s = 0.0;
    for (int k = lane; k < p.K; k += MSMD_WAVE) s += p.w[k];
    s = wave_sum_f64(s);
    if (lane == 0) sh_misc[0] = s;
  }
  bool bad = false;
  for (int e = lane; e < p.K * 3; e += MSMD_WAVE) bad |= !isfinite(p.landmarks[(long)W.frame * p.K * 3 + e]);
  bad = __any(bad);
  __syncthreads();
  const double wsum = sh_misc[0];

  const double D = lane < NE ? p.lambda_exp : (lane < NP ? p.lambda_jaw : 0.0);
  double acc[8][8];
  double g = 0.0, pv = 0.0, mu = 1e-3;
  int st = 0;
  ef_set_point(p, W, pv);
  double fdata = ef_pass<false>(p, W, acc, g);
  double f = fdata + wave_sum_f64(D * pv * pv);
  for (int it = 0; it < p.iterations; ++it) {
    ef_set_point(p, W, pv);
    (void)ef_pass<true>(p, W, acc, g);
    g = fma(D, pv, g);
    const int ti = lane >> 3, tj = lane & 7;
    if (ti == tj) {
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        const int i = a * 8 + ti;
        const double di = i < NE ? p.lambda_exp : (i < NP ? p.lambda_jaw : 0.0);
        acc[a][a] = (acc[a][a] + di) * (1.0 + mu);
      }
    }
    const bool ok = wave_cholesky(lane, NP, W.wv + EF_OFF_COL, W.wv + EF_OFF_BIG, acc);
    double delta = 0.0;
    if (ok) delta = wave_chol_solve(lane, NP, W.wv + EF_OFF_BIG, -g);
    else st |= 2;
    const double pt = lane < NP && ok ? pv + delta : pv;
    ef_set_point(p, W, pt);
    const double fd_t = ef_pass<false>(p, W, acc, g);
    const double f_t = fd_t + wave_sum_f64(D * pt * pt);
    if (ok && f_t <= f) {
      pv = pt; f = f_t; fdata = fd_t;
      mu = fmax(mu / 10.0, 1e-9);
    } else {
      mu = mu * 10.0;
    }
  }
  const double j0 = __shfl(pv, NE, 64), j1 = __shfl(pv, min(NE + 1, 63), 64), j2 = __shfl(pv, min(NE + 2, 63), 64);
  if (!live) return;
  const float nanv = __builtin_nanf("");
  if (lane < NE) p.code[(long)W.frame * NE + lane] = bad ? nanv : (float)pv;
  if (lane < 3) {
    const double th = lane == 0 ? j0 : (lane == 1 ? j1 : j2);
    p.jaw[(long)W.frame * 3 + lane] = bad ? nanv : (lane < p.jaw_dof ? (float)th : 0.0f);
  }
  if (lane == 0) {
    p.rms[W.frame] = bad ? nanv : (float)sqrt(fdata / wsum);
    p.status[W.frame] = bad ? 1 : st;
  }
}

extern "C" int msmd_expression_fit(const float* landmarks, const int* subject, const double* tab, const double* tab0, const double* w,
                                   float* code, float* jaw, float* rms, int* status, int n, int K, int NE, int S, int jaw_dof,
                                   int iterations, double lambda_exp, double lambda_jaw, msmd_stream_t stream) {
  if (!landmarks || !subject || !tab || !tab0 || !w || !code || !jaw || !rms || !status) return 1;
  if (n <= 0 || K < 1 || K > MSMD_EXPFIT_MAX_LANDMARKS || NE < 1 || NE > MSMD_EXPFIT_MAX_EXP || S < 1) return 1;
  if ((jaw_dof != 0 && jaw_dof != 1 && jaw_dof != 3) || iterations < 0 || iterations > MSMD_EXPFIT_MAX_ITERATIONS) return 1;
  if (!(lambda_exp >= 0.0) || !(lambda_jaw >= 0.0) || (long)n * K * 3 > 0x7fffffffL) return 1;
  ExpFitArgs p;
  p.landmarks = landmarks; p.subject = subject; p.tab = tab; p.tab0 = tab0; p.w = w;
  p.code = code; p.jaw = jaw; p.rms = rms; p.status = status;
  p.n = n; p.K = K; p.NE = NE; p.S = S; p.jaw_dof = jaw_dof; p.iterations = iterations;
  p.lambda_exp = lambda_exp; p.lambda_jaw = lambda_jaw;
  const size_t lds = sizeof(double) * ((size_t)ef_shared(NE + 9) + (size_t)EF_FRAMES * (EF_OFF_BIG + ef_big(NE + jaw_dof)));
  static bool attr_set = false;      // idempotent: the same value every time
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)expression_fit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL(expression_fit_kernel, dim3((unsigned)((n + EF_FRAMES - 1) / EF_FRAMES)), dim3(EF_WG), lds, (hipStream_t)stream, p);
  MSMD_RETURN_LAST();
}
