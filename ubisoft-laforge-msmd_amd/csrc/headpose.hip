// Head pose from tracked face landmarks (reference dataset_processing/Step2_preprocess_head_pose_mediapipe.py:15-111, 532-568;
// DESIGN.md 5.18): a per-frame similarity fit of S rigid landmarks onto a neutral face (Umeyama 1991), then per clip the
// quaternion sign continuity, a Savitzky-Golay filter with polynomial edge rows and the intrinsic Y-X-Z angles.
// Outside the contract (include/msmd_hip.h): agreement with the reference on a covariance of rank < 3 (collinear points have no
// fit at all), and |pitch| within 1e-3 degrees of 90.
#include "savgol.h"

constexpr int HP_WG = 256;
constexpr int HP_TILE = 1024;          // landmarks staged per pass of the transform
static_assert(HP_WG == MSMD_HEADPOSE_CHUNK && MSMD_WAVE == MSMD_HEADPOSE_MAX_STATIC, "header and kernel disagree");

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// One-sided Jacobi on the columns a0, a1, a2 of a 3 x 3 matrix with V accumulated in v0, v1, v2: one rotation of the pair
// (p, q) that makes the two columns orthogonal.  Everything is addressed by name, so it stays in registers.  (The 3 x 3 stage
// and quat_of are __host__ too: a host program can check them without a GPU.)
__host__ __device__ __forceinline__ void jacobi_pair(double* ap, double* aq, double* vp, double* vq) {
  const double alpha = ap[0] * ap[0] + ap[1] * ap[1] + ap[2] * ap[2];
  const double beta = aq[0] * aq[0] + aq[1] * aq[1] + aq[2] * aq[2];
  const double gamma = ap[0] * aq[0] + ap[1] * aq[1] + ap[2] * aq[2];
  if (gamma * gamma <= 1e-34 * alpha * beta) return;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double x = ap[k], y = aq[k];
    ap[k] = cs * x - sn * y;
    aq[k] = sn * x + cs * y;
    const double u = vp[k], w = vq[k];
    vp[k] = cs * u - sn * w;
    vq[k] = sn * u + cs * w;
  }
}
__host__ __device__ __forceinline__ void swap_cols(double* a, double* b, double* va, double* vb, double& sa, double& sb) {
  if (sa < sb) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double x = a[k]; a[k] = b[k]; b[k] = x;
      x = va[k]; va[k] = vb[k]; vb[k] = x;
    }
    const double x = sa; sa = sb; sb = x;
  }
}
__host__ __device__ __forceinline__ double det3_cols(const double* a, const double* b, const double* c) {
  return a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1]) + c[0] * (a[1] * b[2] - a[2] * b[1]);
}

// cov (row-major 3 x 3) = U D V^T by one-sided Jacobi (columns of cov V made orthogonal; D their norms, sorted descending;
// U the normalised columns), Sg = diag(1, 1, det(U) det(V^T) < 0 ? -1 : 1): R = U Sg V^T and sum(D diag Sg).
// U's third column is u0 x u1 times sigma = +-1, so det(U) = sigma and the third term of R, Sg[2][2] sigma (u0 x u1) v2^T, is
// det(V) (u0 x u1) v2^T whatever sigma is: the column is never divided by the smallest singular value, and a covariance of
// rank 2 (coplanar static points, S = 3) gets the rotation it still determines.  sigma only enters the scale, times D[2].
__host__ __device__ __forceinline__ void fit_rotation(const double* cov, double* R, double& trace_ds) {
  double a0[3] = {cov[0], cov[3], cov[6]}, a1[3] = {cov[1], cov[4], cov[7]}, a2[3] = {cov[2], cov[5], cov[8]};
  double v0[3] = {1, 0, 0}, v1[3] = {0, 1, 0}, v2[3] = {0, 0, 1};
  for (int sweep = 0; sweep < 12; ++sweep) {
    jacobi_pair(a0, a1, v0, v1);
    jacobi_pair(a0, a2, v0, v2);
    jacobi_pair(a1, a2, v1, v2);
  }
  double s0 = sqrt(a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]);
  double s1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
  double s2 = sqrt(a2[0] * a2[0] + a2[1] * a2[1] + a2[2] * a2[2]);
  swap_cols(a0, a1, v0, v1, s0, s1);
  swap_cols(a1, a2, v1, v2, s1, s2);
  swap_cols(a0, a1, v0, v1, s0, s1);
#pragma unroll
  for (int k = 0; k < 3; ++k) { a0[k] /= s0; a1[k] /= s1; }                    // u0, u1
  const double u2[3] = {a0[1] * a1[2] - a0[2] * a1[1], a0[2] * a1[0] - a0[0] * a1[2], a0[0] * a1[1] - a0[1] * a1[0]};
  const double sigma = (a2[0] * u2[0] + a2[1] * u2[1] + a2[2] * u2[2]) < 0.0 ? -1.0 : 1.0;
  const double det_v = det3_cols(v0, v1, v2) < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = a0[i] * v0[j] + a1[i] * v1[j] + det_v * u2[i] * v2[j];
  trace_ds = s0 + s1 + sigma * det_v * s2;
}

// One workgroup per frame.  Wave 0 holds one static point per lane (S <= 64): the means, then the centred second moments,
// are summed across the wave in double (the coordinates sit near 0.5 with a spread of a few hundredths: their variance
// must not drown in fp32); lane 0 runs the 3 x 3 stage in double and leaves c R and t in LDS.  Then the whole workgroup
// passes over the frame's P blended landmarks HP_TILE at a time: linear dword loads into LDS, c R x + t per output
// element, linear dword stores.  A frame is (1 - w) L[a] + w L[b]; w == 0 reads L[a] alone.
__global__ __launch_bounds__(HP_WG) void headpose_fit_kernel(const float* __restrict__ landmarks, const int* __restrict__ plan_a,
                                                             const int* __restrict__ plan_b, const float* __restrict__ plan_w,
                                                             const float* __restrict__ neutral, const int* __restrict__ static_idx,
                                                             float* __restrict__ R_out, float* __restrict__ c_out,
                                                             float* __restrict__ t_out, float* __restrict__ aligned, int n_frames,
                                                             int P, int S) {
  __shared__ float s_tf[12];                    // c R (9), t (3)
  __shared__ float s_pts[HP_TILE * 3];
  const int f = blockIdx.x;
  const int fa = clamp_index(plan_a[f], n_frames), fb = clamp_index(plan_b[f], n_frames);
  const float w = plan_w[f];
  const bool blend = w != 0.0f;
  const float* __restrict__ La = landmarks + (long)fa * P * 3;
  const float* __restrict__ Lb = landmarks + (long)fb * P * 3;
  const int tid = threadIdx.x;
  if (tid < MSMD_WAVE) {
    double x[3] = {0, 0, 0}, y[3] = {0, 0, 0};
    const bool live = tid < S;
    if (live) {
      const int idx = clamp_index(static_idx[tid], P);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float v = La[idx * 3 + k];
        if (blend) v = (1.0f - w) * v + w * Lb[idx * 3 + k];
        x[k] = (double)v;
        y[k] = (double)neutral[idx * 3 + k];
      }
    }
    const double inv = 1.0 / (double)S;
    double mx[3], my[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      mx[k] = wave_sum_f64(x[k]) * inv;
      my[k] = wave_sum_f64(y[k]) * inv;
    }
    double cov[9], rho2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = live ? x[k] - mx[k] : 0.0;
      y[k] = live ? y[k] - my[k] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) rho2 += wave_sum_f64(x[k] * x[k]) * inv;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) cov[i * 3 + j] = wave_sum_f64(y[i] * x[j]) * inv;
    if (tid == 0) {
      double R[9], tr;
      fit_rotation(cov, R, tr);
      const double c = tr / rho2;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double ti = my[i] - c * (R[i * 3] * mx[0] + R[i * 3 + 1] * mx[1] + R[i * 3 + 2] * mx[2]);
        t_out[(long)f * 3 + i] = (float)ti;
        s_tf[9 + i] = (float)ti;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          R_out[(long)f * 9 + i * 3 + j] = (float)R[i * 3 + j];
          s_tf[i * 3 + j] = (float)(c * R[i * 3 + j]);
        }
      }
      c_out[f] = (float)c;
    }
  }
  if (!aligned) return;
  __syncthreads();
  float* __restrict__ out = aligned + (long)f * P * 3;
  for (int p0 = 0; p0 < P; p0 += HP_TILE) {
    const int n = min(HP_TILE, P - p0) * 3;
    if (p0) __syncthreads();
    for (int e = tid; e < n; e += HP_WG) {
      float v = La[p0 * 3 + e];
      if (blend) v = (1.0f - w) * v + w * Lb[p0 * 3 + e];
      s_pts[e] = v;
    }
    __syncthreads();
    for (int e = tid; e < n; e += HP_WG) {
      const int p = e / 3, k = e - p * 3;
      const float r0 = k == 0 ? s_tf[0] : k == 1 ? s_tf[3] : s_tf[6];
      const float r1 = k == 0 ? s_tf[1] : k == 1 ? s_tf[4] : s_tf[7];
      const float r2 = k == 0 ? s_tf[2] : k == 1 ? s_tf[5] : s_tf[8];
      const float tk = k == 0 ? s_tf[9] : k == 1 ? s_tf[10] : s_tf[11];
      out[p0 * 3 + e] = fmaf(r2, s_pts[p * 3 + 2], fmaf(r1, s_pts[p * 3 + 1], r0 * s_pts[p * 3])) + tk;
    }
  }
}

extern "C" int msmd_headpose_fit(const float* landmarks, const int* plan_a, const int* plan_b, const float* plan_w,
                                 const float* neutral, const int* static_idx, float* R, float* c, float* t, float* aligned,
                                 int n_frames, int P, int S, msmd_stream_t stream) {
  if (!landmarks || !plan_a || !plan_b || !plan_w || !neutral || !static_idx || !R || !c || !t) return 1;
  if (n_frames <= 0 || P <= 0 || S < 3 || S > MSMD_HEADPOSE_MAX_STATIC || S > P || (long)P * 3 > 0x7fffffffL) return 1;
  hipLaunchKernelGGL(headpose_fit_kernel, dim3((unsigned)n_frames), dim3(HP_WG), 0, (hipStream_t)stream, landmarks, plan_a, plan_b,
                     plan_w, neutral, static_idx, R, c, t, aligned, n_frames, P, S);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
struct Quat { double x, y, z, w; };

// Unit quaternion of a rotation matrix by the branch with the largest of (m00, m11, m22, trace): that component is positive
// and nothing is divided by a small number.  (The sign convention is free: see the header.)
__host__ __device__ __forceinline__ Quat quat_of(const float* __restrict__ m) {
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
  const double tr = m00 + m11 + m22;
  Quat q;
  if (tr >= m00 && tr >= m11 && tr >= m22) q = Quat{m21 - m12, m02 - m20, m10 - m01, 1.0 + tr};
  else if (m00 >= m11 && m00 >= m22) q = Quat{1.0 - tr + 2.0 * m00, m10 + m01, m20 + m02, m21 - m12};
  else if (m11 >= m22) q = Quat{m10 + m01, 1.0 - tr + 2.0 * m11, m21 + m12, m02 - m20};
  else q = Quat{m20 + m02, m21 + m12, 1.0 - tr + 2.0 * m22, m10 - m01};
  const double s = 1.0 / sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return Quat{q.x * s, q.y * s, q.z * s, q.w * s};
}

// One workgroup per clip; frames go through in chunks of HP_WG, one frame per thread.
//   scan    each thread's flip bit (its raw quaternion against its predecessor's) becomes a prefix parity: ballot + popcount
//           inside a wave, the waves' parities through LDS, the clip's running sign carried from chunk to chunk.
//   filter  the signed quaternions of the chunk sit in s_q behind the last window - 1 of the chunks before, so after chunk k
//           every frame below (k + 1) HP_WG - window / 2 has its whole window in LDS and is written; the last chunk writes
//           the rest.  The first / last window / 2 frames of the clip take their row of the edge table over the clip's
//           first / last `window` frames, which lie in the first chunk / within window - 1 frames of the last.
// Double throughout: the work is a few hundred operations per frame, and the result then carries the rounding of its fp32
// input and output alone.
__global__ __launch_bounds__(HP_WG) void headpose_smooth_kernel(const float* __restrict__ R, const long* __restrict__ clip_offsets,
                                                                const double* __restrict__ coeffs, int window,
                                                                float* __restrict__ ypr_deg, float* __restrict__ R_out) {
  constexpr int HALO = SAVGOL_MAX_WINDOW - 1;
  __shared__ Quat s_q[HALO + HP_WG];
  __shared__ Quat s_raw[HP_WG];
  __shared__ double s_coef[SAVGOL_TABLE];
  __shared__ int s_par[HP_WG / MSMD_WAVE];
  const long begin = clip_offsets[blockIdx.x];
  const int F = (int)(clip_offsets[blockIdx.x + 1] - begin);
  const int h = window >> 1, halo = window - 1;
  if (F < window) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  savgol_stage<HP_WG>(s_coef, coeffs, window);
  Quat carry_q = Quat{0, 0, 0, 0};           // raw quaternion of the frame before this chunk (uniform across the workgroup)
  int carry_par = 0;                         // parity of the flips up to and including that frame
  for (int c0 = 0; c0 < F; c0 += HP_WG) {
    const int n = min(HP_WG, F - c0);
    const bool live = tid < n;
    Quat q = Quat{0, 0, 0, 1};
    if (live) q = quat_of(R + (begin + c0 + tid) * 9);
    s_raw[tid] = q;
    __syncthreads();
    const Quat prev = tid == 0 ? carry_q : s_raw[tid - 1];
    const bool flip = live && (c0 + tid) > 0 && (q.x * prev.x + q.y * prev.y + q.z * prev.z + q.w * prev.w) < 0.0;
    const unsigned long long bal = __ballot(flip);
    const unsigned long long below = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
    int par = __popcll(bal & below) & 1;
    if (lane == 0) s_par[wid] = __popcll(bal) & 1;
    __syncthreads();
    for (int k = 0; k < wid; ++k) par ^= s_par[k];
    par ^= carry_par;
    const double sgn = par ? -1.0 : 1.0;
    if (live) s_q[halo + tid] = Quat{sgn * q.x, sgn * q.y, sgn * q.z, sgn * q.w};
    carry_par ^= s_par[0] ^ s_par[1] ^ s_par[2] ^ s_par[3];
    carry_q = s_raw[n - 1];
    __syncthreads();
    // frames [c0 - halo, c0 + n) of the clip are s_q[0 .. halo + n): write those whose window is complete
    const int lo = max(c0 - h, 0), hi = (c0 + n == F) ? F : c0 + n - h;
    for (int j = lo + tid; j < hi; j += HP_WG) {
      int first;
      const double* __restrict__ row = savgol_row(s_coef, window, j, F, first);
      const Quat* __restrict__ src = s_q + (first - (c0 - halo));
      double x = 0, y = 0, z = 0, ww = 0;
      for (int m = 0; m < window; ++m) {
        const double cm = row[m];
        const Quat s = src[m];
        x = fma(cm, s.x, x); y = fma(cm, s.y, y); z = fma(cm, s.z, z); ww = fma(cm, s.w, ww);
      }
      const double inv = 1.0 / sqrt(x * x + y * y + z * z + ww * ww);
      x *= inv; y *= inv; z *= inv; ww *= inv;
      // rows 1 and 2 of diag(1, -1, -1) times the quaternion's matrix, and the two entries of rows 0 and 2 the angles read
      const double r02 = 2.0 * (x * z + y * ww), r22 = -(1.0 - 2.0 * (x * x + y * y));
      const double r10 = -2.0 * (x * y + z * ww), r11 = -(1.0 - 2.0 * (x * x + z * z)), r12 = -2.0 * (y * z - x * ww);
      const double deg = 57.295779513082320876798154814105;
      const double sx = fmin(fmax(-r12, -1.0), 1.0);
      float* __restrict__ o = ypr_deg + (begin + j) * 3;
      o[0] = (float)(atan2(r02, r22) * deg);
      o[1] = (float)(asin(sx) * deg);
      o[2] = (float)(-atan2(r10, r11) * deg);
      if (R_out) {
        // Ry(yaw) Rx(pitch) Rz(-roll): the angles' sines and cosines are ratios of the entries they were read from
        const double cx = sqrt(1.0 - sx * sx);
        const double ny = 1.0 / sqrt(r02 * r02 + r22 * r22), nz = 1.0 / sqrt(r10 * r10 + r11 * r11);
        const double sy = r02 * ny, cy = r22 * ny, sz = -r10 * nz, cz = r11 * nz;
        float* __restrict__ ro = R_out + (begin + j) * 9;
        ro[0] = (float)(cy * cz + sy * sx * sz); ro[1] = (float)(-cy * sz + sy * sx * cz); ro[2] = (float)(sy * cx);
        ro[3] = (float)(cx * sz); ro[4] = (float)(cx * cz); ro[5] = (float)(-sx);
        ro[6] = (float)(-sy * cz + cy * sx * sz); ro[7] = (float)(sy * sz + cy * sx * cz); ro[8] = (float)(cy * cx);
      }
    }
    __syncthreads();
    // the last window - 1 signed quaternions move to the front for the next chunk
    double kx = 0.0, ky = 0.0, kz = 0.0, kw = 0.0;
    if (tid < halo) { kx = s_q[n + tid].x; ky = s_q[n + tid].y; kz = s_q[n + tid].z; kw = s_q[n + tid].w; }
    __syncthreads();
    if (tid < halo) { s_q[tid].x = kx; s_q[tid].y = ky; s_q[tid].z = kz; s_q[tid].w = kw; }
  }
}

extern "C" int msmd_headpose_smooth(const float* R, const long* clip_offsets, int n_clips, const double* coeffs, int window,
                                    float* ypr_deg, float* R_out, msmd_stream_t stream) {
  if (!R || !clip_offsets || !coeffs || !ypr_deg || n_clips <= 0) return 1;
  if (!savgol_window_ok(window)) return 1;
  hipLaunchKernelGGL(headpose_smooth_kernel, dim3((unsigned)n_clips), dim3(HP_WG), 0, (hipStream_t)stream, R, clip_offsets, coeffs,
                     window, ypr_deg, R_out);
  MSMD_RETURN_LAST();
}
