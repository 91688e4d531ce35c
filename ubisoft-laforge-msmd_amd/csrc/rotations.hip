// Rotation conversions (reference utils/rotation_conversions.py:38-569; PyTorch3D semantics):
// real-first quaternions, small-angle Taylor branch below 1e-6, _sqrt_positive_part, _copysign.
// Elementwise and HBM-bound: one item per thread in registers, LDS-staged linear 16-byte global accesses (see rotation_kernel).
#include "common.h"

__device__ __forceinline__ void quat_to_mat(const float* q, float* o) {
  const float r = q[0], i = q[1], j = q[2], k = q[3];
  const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
  o[0] = 1 - two_s * (j * j + k * k); o[1] = two_s * (i * j - k * r); o[2] = two_s * (i * k + j * r);
  o[3] = two_s * (i * j + k * r); o[4] = 1 - two_s * (i * i + k * k); o[5] = two_s * (j * k - i * r);
  o[6] = two_s * (i * k - j * r); o[7] = two_s * (j * k + i * r); o[8] = 1 - two_s * (i * i + j * j);
}
__device__ __forceinline__ float sqrt_pos(float x) { return x > 0.f ? sqrtf(x) : 0.f; }
__device__ __forceinline__ float copysign_like(float a, float b) { return ((a < 0.f) != (b < 0.f)) ? -a : a; }

__device__ __forceinline__ void mat_to_quat(const float* m, float* o) {
  const float m00 = m[0], m11 = m[4], m22 = m[8];
  o[0] = 0.5f * sqrt_pos(1 + m00 + m11 + m22);
  const float x = 0.5f * sqrt_pos(1 + m00 - m11 - m22);
  const float y = 0.5f * sqrt_pos(1 - m00 + m11 - m22);
  const float z = 0.5f * sqrt_pos(1 - m00 - m11 + m22);
  o[1] = copysign_like(x, m[7] - m[5]);
  o[2] = copysign_like(y, m[2] - m[6]);
  o[3] = copysign_like(z, m[3] - m[1]);
}
__device__ __forceinline__ void aa_to_quat(const float* a, float* o) {
  const float angle = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  const float half = 0.5f * angle;
  const float soa = (fabsf(angle) < 1e-6f) ? (0.5f - (angle * angle) / 48.0f) : (sinf(half) / angle);
  o[0] = cosf(half); o[1] = a[0] * soa; o[2] = a[1] * soa; o[3] = a[2] * soa;
}
__device__ __forceinline__ void quat_to_aa(const float* q, float* o) {
  const float n = sqrtf(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float half = atan2f(n, q[0]);
  const float angle = 2.0f * half;
  const float soa = (fabsf(angle) < 1e-6f) ? (0.5f - (angle * angle) / 48.0f) : (sinf(half) / angle);
  o[0] = q[1] / soa; o[1] = q[2] / soa; o[2] = q[3] / soa;
}
__device__ __forceinline__ void quat_raw_mul(const float* a, const float* b, float* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
__device__ __forceinline__ void normalize3(const float* a, float* o) {
  const float n = fmaxf(sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), 1e-12f);  // F.normalize eps
  o[0] = a[0] / n; o[1] = a[1] / n; o[2] = a[2] / n;
}
__device__ __forceinline__ void axis_rot(int axis, float ang, float* R) {
  const float c = cosf(ang), s = sinf(ang);
  if (axis == 0) { R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = c; R[5] = -s; R[6] = 0; R[7] = s; R[8] = c; }
  else if (axis == 1) { R[0] = c; R[1] = 0; R[2] = s; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = -s; R[7] = 0; R[8] = c; }
  else { R[0] = c; R[1] = -s; R[2] = 0; R[3] = s; R[4] = c; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1; }
}
__device__ __forceinline__ void mat3mul(const float* a, const float* b, float* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}
// _angle_from_tan(axis, other_axis, data(3 values), horizontal, tait_bryan)
__device__ __forceinline__ float angle_from_tan(int axis, int other, const float* data, bool horizontal, bool tb) {
  int i1 = axis == 0 ? 2 : (axis == 1 ? 0 : 1);
  int i2 = axis == 0 ? 1 : (axis == 1 ? 2 : 0);
  if (horizontal) { const int t = i1; i1 = i2; i2 = t; }
  const bool even = (axis == 0 && other == 1) || (axis == 1 && other == 2) || (axis == 2 && other == 0);
  const float d1 = i1 == 0 ? data[0] : (i1 == 1 ? data[1] : data[2]);   // selects: a run-time-indexed local array lives in scratch
  const float d2 = i2 == 0 ? data[0] : (i2 == 1 ? data[1] : data[2]);
  if (horizontal == even) return atan2f(d1, d2);
  if (tb) return atan2f(-d2, d1);
  return atan2f(d2, -d1);
}

// Array-of-structures items (3 / 4 / 6 / 9 floats each) never meet HBM through per-thread strided accesses: a workgroup owns
// 256 consecutive items, i.e. ONE contiguous span of the input and of the output.  The span is staged through LDS with 16-byte
// per-lane loads / stores in linear order (whole 64-byte sectors per 4 lanes, 1 KiB per wave instruction); each thread then
// takes its item from LDS (row stride 3 / 9 words is conflict-free, 4 words reads as one ds_read_b128), computes in registers,
// and puts the result back into the same LDS buffer for the linear store pass.  Unaligned bases (a view into a larger
// tensor) fall back to dword pieces in the same linear order.
constexpr int ROT_WG = 256;

__device__ __forceinline__ void rot_stage_in(float* __restrict__ dst, const float* __restrict__ src, int count) {
  if (((uintptr_t)src & 15) == 0) {
    const int nv = count >> 2;
    for (int i = threadIdx.x; i < nv; i += ROT_WG) ((float4*)dst)[i] = ((const float4*)src)[i];
    for (int i = (nv << 2) + threadIdx.x; i < count; i += ROT_WG) dst[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < count; i += ROT_WG) dst[i] = src[i];
  }
}
__device__ __forceinline__ void rot_stage_out(float* __restrict__ dst, const float* __restrict__ src, int count) {
  if (((uintptr_t)dst & 15) == 0) {
    const int nv = count >> 2;
    for (int i = threadIdx.x; i < nv; i += ROT_WG) ((float4*)dst)[i] = ((const float4*)src)[i];
    for (int i = (nv << 2) + threadIdx.x; i < count; i += ROT_WG) dst[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < count; i += ROT_WG) dst[i] = src[i];
  }
}

__global__ __launch_bounds__(ROT_WG) void rotation_kernel(int op, const float* __restrict__ in, const float* __restrict__ in2,
                                                          float* __restrict__ out, long n, int conv, int in_w, int in2_w,
                                                          int out_w) {
  __shared__ __attribute__((aligned(16))) float s_io[ROT_WG * 9];
  __shared__ __attribute__((aligned(16))) float s_b[ROT_WG * 4];
  const long base = blockIdx.x * (long)ROT_WG;
  const int cnt = (int)min((long)ROT_WG, n - base);
  rot_stage_in(s_io, in + base * in_w, cnt * in_w);
  if (in2) rot_stage_in(s_b, in2 + base * in2_w, cnt * in2_w);
  __syncthreads();
  const int t = threadIdx.x;
  const bool live = t < cnt;
  float a[9], b[4], o[9], q[4];
  const int c0 = conv & 3, c1 = (conv >> 2) & 3, c2 = (conv >> 4) & 3;
  // ---- this thread's item out of LDS (compile-time widths per op: the arrays stay in registers)
  if (live) {
    switch (op) {
      case MSMD_ROT_QUAT_TO_MAT: case MSMD_ROT_QUAT_TO_AA: case MSMD_ROT_QUAT_STANDARDIZE: case MSMD_ROT_QUAT_INVERT:
      case MSMD_ROT_QUAT_RAW_MUL: case MSMD_ROT_QUAT_MUL: case MSMD_ROT_QUAT_APPLY: {
        const float4 v = ((const float4*)s_io)[t];
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
        break;
      }
      case MSMD_ROT_AA_TO_QUAT: case MSMD_ROT_AA_TO_MAT: case MSMD_ROT_AA_TO_6D: case MSMD_ROT_EULER_TO_MAT:
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = s_io[t * 3 + k];
        break;
      case MSMD_ROT_6D_TO_MAT:
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = s_io[t * 6 + k];
        break;
      default:
#pragma unroll
        for (int k = 0; k < 9; ++k) a[k] = s_io[t * 9 + k];
        break;
    }
    if (op == MSMD_ROT_QUAT_RAW_MUL || op == MSMD_ROT_QUAT_MUL) {
      const float4 v = ((const float4*)s_b)[t];
      b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
    } else if (op == MSMD_ROT_QUAT_APPLY) {
      b[0] = 0.f; b[1] = s_b[t * 3]; b[2] = s_b[t * 3 + 1]; b[3] = s_b[t * 3 + 2];
    }
  }
  __syncthreads();      // every item is in registers: the buffer becomes the output span
  if (live) {
    switch (op) {
      case MSMD_ROT_QUAT_TO_MAT:
        quat_to_mat(a, o);
#pragma unroll
        for (int k = 0; k < 9; ++k) s_io[t * 9 + k] = o[k];
        break;
      case MSMD_ROT_MAT_TO_QUAT:
        mat_to_quat(a, o);
        ((float4*)s_io)[t] = float4{o[0], o[1], o[2], o[3]};
        break;
      case MSMD_ROT_AA_TO_QUAT:
        aa_to_quat(a, o);
        ((float4*)s_io)[t] = float4{o[0], o[1], o[2], o[3]};
        break;
      case MSMD_ROT_QUAT_TO_AA:
        quat_to_aa(a, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) s_io[t * 3 + k] = o[k];
        break;
      case MSMD_ROT_AA_TO_MAT:
        aa_to_quat(a, q);
        quat_to_mat(q, o);
#pragma unroll
        for (int k = 0; k < 9; ++k) s_io[t * 9 + k] = o[k];
        break;
      case MSMD_ROT_AA_TO_6D:
        aa_to_quat(a, q);
        quat_to_mat(q, o);
#pragma unroll
        for (int k = 0; k < 6; ++k) s_io[t * 6 + k] = o[k];
        break;
      case MSMD_ROT_MAT_TO_AA:
        mat_to_quat(a, q);
        quat_to_aa(q, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) s_io[t * 3 + k] = o[k];
        break;
      case MSMD_ROT_6D_TO_MAT: {
        float b1[3], b2[3], tmp[3];
        normalize3(a, b1);
        const float dot = b1[0] * a[3] + b1[1] * a[4] + b1[2] * a[5];
#pragma unroll
        for (int k = 0; k < 3; ++k) tmp[k] = a[3 + k] - dot * b1[k];
        normalize3(tmp, b2);
        o[0] = b1[0]; o[1] = b1[1]; o[2] = b1[2]; o[3] = b2[0]; o[4] = b2[1]; o[5] = b2[2];
        o[6] = b1[1] * b2[2] - b1[2] * b2[1]; o[7] = b1[2] * b2[0] - b1[0] * b2[2]; o[8] = b1[0] * b2[1] - b1[1] * b2[0];
#pragma unroll
        for (int k = 0; k < 9; ++k) s_io[t * 9 + k] = o[k];
        break;
      }
      case MSMD_ROT_MAT_TO_6D:
#pragma unroll
        for (int k = 0; k < 6; ++k) s_io[t * 6 + k] = a[k];
        break;
      case MSMD_ROT_EULER_TO_MAT: {
        float R0[9], R1[9], R2[9], R01[9];
        axis_rot(c0, a[0], R0);
        axis_rot(c1, a[1], R1);
        axis_rot(c2, a[2], R2);
        mat3mul(R0, R1, R01);
        mat3mul(R01, R2, o);
#pragma unroll
        for (int k = 0; k < 9; ++k) s_io[t * 9 + k] = o[k];
        break;
      }
      case MSMD_ROT_MAT_TO_EULER: {
        const bool tb = c0 != c2;
        // run-time row / column picks as selects over the nine registers (a run-time-indexed local array lives in scratch)
        auto at = [&](int r, int c) {
          const int i = r * 3 + c;
          return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : i == 3 ? a[3] : i == 4 ? a[4] : i == 5 ? a[5]
                 : i == 6 ? a[6] : i == 7 ? a[7] : a[8];
        };
        float central;
        if (tb) {
          const int df = c0 - c2;
          central = asinf(at(c0, c2) * ((df == -1 || df == 2) ? -1.0f : 1.0f));
        } else {
          central = acosf(at(c0, c0));
        }
        const float col[3] = {at(0, c2), at(1, c2), at(2, c2)};   // matrix[..., i2] (column i2)
        const float rowv[3] = {at(c0, 0), at(c0, 1), at(c0, 2)};  // matrix[..., i0, :]
        s_io[t * 3 + 0] = angle_from_tan(c0, c1, col, false, tb);
        s_io[t * 3 + 1] = central;
        s_io[t * 3 + 2] = angle_from_tan(c2, c1, rowv, true, tb);
        break;
      }
      case MSMD_ROT_QUAT_STANDARDIZE: {
        ((float4*)s_io)[t] = a[0] < 0.f ? float4{-a[0], -a[1], -a[2], -a[3]} : float4{a[0], a[1], a[2], a[3]};
        break;
      }
      case MSMD_ROT_QUAT_INVERT:
        ((float4*)s_io)[t] = float4{a[0], -a[1], -a[2], -a[3]};
        break;
      case MSMD_ROT_QUAT_RAW_MUL:
      case MSMD_ROT_QUAT_MUL:
        quat_raw_mul(a, b, o);
        if (op == MSMD_ROT_QUAT_MUL && o[0] < 0.f) { o[0] = -o[0]; o[1] = -o[1]; o[2] = -o[2]; o[3] = -o[3]; }
        ((float4*)s_io)[t] = float4{o[0], o[1], o[2], o[3]};
        break;
      case MSMD_ROT_QUAT_APPLY: {
        const float inv[4] = {a[0], -a[1], -a[2], -a[3]};
        float tmp[4];
        quat_raw_mul(a, b, tmp);
        quat_raw_mul(tmp, inv, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) s_io[t * 3 + k] = o[1 + k];
        break;
      }
      default: break;
    }
  }
  __syncthreads();
  rot_stage_out(out + base * out_w, s_io, cnt * out_w);
}

extern "C" int msmd_rotation_convert(int op, const float* in, const float* in2, float* out, long n, int conv,
                                     msmd_stream_t stream) {
  if (n <= 0 || op < 0 || op > MSMD_ROT_QUAT_APPLY || !in || !out) return 1;
  if ((op == MSMD_ROT_QUAT_RAW_MUL || op == MSMD_ROT_QUAT_MUL || op == MSMD_ROT_QUAT_APPLY) && !in2) return 1;
  // item widths (floats) by op: input, second input, output
  static const signed char W[MSMD_ROT_QUAT_APPLY + 1][3] = {
      {4, 0, 9}, {9, 0, 4}, {3, 0, 4}, {4, 0, 3}, {3, 0, 9}, {9, 0, 3}, {6, 0, 9}, {9, 0, 6},
      {3, 0, 6}, {3, 0, 9}, {9, 0, 3}, {4, 0, 4}, {4, 0, 4}, {4, 4, 4}, {4, 4, 4}, {4, 3, 3}};
  const bool two = W[op][1] != 0;
  hipLaunchKernelGGL(rotation_kernel, dim3((unsigned)((n + ROT_WG - 1) / ROT_WG)), dim3(ROT_WG), 0, (hipStream_t)stream, op, in,
                     two ? in2 : nullptr, out, n, conv, (int)W[op][0], (int)W[op][1], (int)W[op][2]);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
// Backward: the vector-Jacobian product of every op above, from the forward's INPUTS (intermediates are recomputed in
// registers; the forward saves nothing).  Each piece differentiates the branch its forward takes, as the reference's
// autograd does: the Taylor branch below 1e-6, no gradient through a _sqrt_positive_part argument <= 0, _copysign and
// standardize_quaternion pass +-1, torch.norm has gradient 0 at 0, F.normalize's clamp passes nothing below eps.
// All array indices are compile-time constants (run-time picks are selects), so everything stays in registers.
__device__ __forceinline__ void quat_to_mat_bwd(const float* q, const float* g, float* gq) {
  const float r = q[0], i = q[1], j = q[2], k = q[3];
  const float n = r * r + i * i + j * j + k * k;
  const float two_s = 2.0f / n;
  // o_e = const_e + two_s * p_e:  P = sum_e g_e p_e is the gradient of two_s
  const float P = -g[0] * (j * j + k * k) + g[1] * (i * j - k * r) + g[2] * (i * k + j * r) + g[3] * (i * j + k * r) -
                  g[4] * (i * i + k * k) + g[5] * (j * k - i * r) + g[6] * (i * k - j * r) + g[7] * (j * k + i * r) -
                  g[8] * (i * i + j * j);
  const float gn2 = -2.0f * two_s * P / n;   // 2 * d(two_s)/dn * P: the gradient of n, times the 2 of d(n)/dq = 2 q
  gq[0] = two_s * (k * (g[3] - g[1]) + j * (g[2] - g[6]) + i * (g[7] - g[5])) + gn2 * r;
  gq[1] = two_s * (j * (g[1] + g[3]) + k * (g[2] + g[6]) - 2.0f * i * (g[4] + g[8]) + r * (g[7] - g[5])) + gn2 * i;
  gq[2] = two_s * (i * (g[1] + g[3]) + k * (g[5] + g[7]) - 2.0f * j * (g[0] + g[8]) + r * (g[2] - g[6])) + gn2 * j;
  gq[3] = two_s * (i * (g[2] + g[6]) + j * (g[5] + g[7]) - 2.0f * k * (g[0] + g[4]) + r * (g[3] - g[1])) + gn2 * k;
}
// d(0.5 * sqrt_pos(x)) / dx
__device__ __forceinline__ float half_sqrt_pos_bwd(float x) { return x > 0.f ? 0.25f / sqrtf(x) : 0.f; }

__device__ __forceinline__ void mat_to_quat_bwd(const float* m, const float* g, float* gm) {
  const float m00 = m[0], m11 = m[4], m22 = m[8];
  // _copysign(a, b) with a >= 0: the sign of b goes to a's gradient, nothing to b
  const float g0 = g[0] * half_sqrt_pos_bwd(1 + m00 + m11 + m22);
  const float g1 = ((m[7] - m[5]) < 0.f ? -g[1] : g[1]) * half_sqrt_pos_bwd(1 + m00 - m11 - m22);
  const float g2 = ((m[2] - m[6]) < 0.f ? -g[2] : g[2]) * half_sqrt_pos_bwd(1 - m00 + m11 - m22);
  const float g3 = ((m[3] - m[1]) < 0.f ? -g[3] : g[3]) * half_sqrt_pos_bwd(1 - m00 - m11 + m22);
  gm[0] = g0 + g1 - g2 - g3; gm[1] = 0.f; gm[2] = 0.f;
  gm[3] = 0.f; gm[4] = g0 - g1 + g2 - g3; gm[5] = 0.f;
  gm[6] = 0.f; gm[7] = 0.f; gm[8] = g0 - g1 - g2 + g3;
}
// sin(half) / angle with angle = 2 half, as a function of (half, angle): value and the total derivative by half
__device__ __forceinline__ float soa_bwd_half(float half, float angle) {
  if (fabsf(angle) < 1e-6f) return -angle / 12.0f;                 // d(0.5 - angle^2 / 48) / d angle * 2
  return (cosf(half) - 2.0f * sinf(half) / angle) / angle;         // cos(half) / angle - 2 sin(half) / angle^2
}
__device__ __forceinline__ void aa_to_quat_bwd(const float* a, const float* g, float* ga) {
  const float angle = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  const float half = 0.5f * angle;
  const float soa = (fabsf(angle) < 1e-6f) ? (0.5f - (angle * angle) / 48.0f) : (sinf(half) / angle);
  const float g_soa = g[1] * a[0] + g[2] * a[1] + g[3] * a[2];
  // angle enters through cos(half), and through sin(half) / angle
  const float g_angle = -0.5f * sinf(half) * g[0] + 0.5f * soa_bwd_half(half, angle) * g_soa;
  const float s = angle > 0.f ? g_angle / angle : 0.f;               // torch.norm: gradient 0 at 0
  ga[0] = g[1] * soa + a[0] * s; ga[1] = g[2] * soa + a[1] * s; ga[2] = g[3] * soa + a[2] * s;
}
__device__ __forceinline__ void quat_to_aa_bwd(const float* q, const float* g, float* gq) {
  const float n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const float n = sqrtf(n2);
  const float half = atan2f(n, q[0]);
  const float angle = 2.0f * half;
  const float soa = (fabsf(angle) < 1e-6f) ? (0.5f - (angle * angle) / 48.0f) : (sinf(half) / angle);
  const float inv = 1.0f / soa;
  const float g_soa = -(g[0] * q[1] + g[1] * q[2] + g[2] * q[3]) * inv * inv;
  const float g_half = g_soa * soa_bwd_half(half, angle);
  const float d = n2 + q[0] * q[0];                                  // atan2(n, w): d/dn = w / d, d/dw = -n / d
  const float g_n = g_half * q[0] / d;
  const float s = n > 0.f ? g_n / n : 0.f;
  gq[0] = -g_half * n / d;
  gq[1] = g[0] * inv + q[1] * s; gq[2] = g[1] * inv + q[2] * s; gq[3] = g[2] * inv + q[3] * s;
}
__device__ __forceinline__ void quat_raw_mul_bwd(const float* a, const float* b, const float* g, float* ga, float* gb) {
  ga[0] = g[0] * b[0] + g[1] * b[1] + g[2] * b[2] + g[3] * b[3];
  ga[1] = -g[0] * b[1] + g[1] * b[0] - g[2] * b[3] + g[3] * b[2];
  ga[2] = -g[0] * b[2] + g[1] * b[3] + g[2] * b[0] - g[3] * b[1];
  ga[3] = -g[0] * b[3] - g[1] * b[2] + g[2] * b[1] + g[3] * b[0];
  gb[0] = g[0] * a[0] + g[1] * a[1] + g[2] * a[2] + g[3] * a[3];
  gb[1] = -g[0] * a[1] + g[1] * a[0] + g[2] * a[3] - g[3] * a[2];
  gb[2] = -g[0] * a[2] - g[1] * a[3] + g[2] * a[0] + g[3] * a[1];
  gb[3] = -g[0] * a[3] + g[1] * a[2] - g[2] * a[1] + g[3] * a[0];
}
// o = a / max(|a|, eps): ga from go (F.normalize: the clamp passes the norm's gradient only where |a| >= eps)
__device__ __forceinline__ void normalize3_bwd(const float* a, const float* go, float* ga) {
  const float nrm = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  const float den = fmaxf(nrm, 1e-12f);
  const float g_den = -(go[0] * a[0] + go[1] * a[1] + go[2] * a[2]) / (den * den);
  const float s = (nrm >= 1e-12f && nrm > 0.f) ? g_den / nrm : 0.f;
  ga[0] = go[0] / den + a[0] * s; ga[1] = go[1] / den + a[1] * s; ga[2] = go[2] / den + a[2] * s;
}
__device__ __forceinline__ void rot6d_to_mat_bwd(const float* a, const float* g, float* ga) {
  float b1[3], b2[3], tmp[3];
  normalize3(a, b1);
  const float dot = b1[0] * a[3] + b1[1] * a[4] + b1[2] * a[5];
#pragma unroll
  for (int k = 0; k < 3; ++k) tmp[k] = a[3 + k] - dot * b1[k];
  normalize3(tmp, b2);
  // b3 = b1 x b2:  g_b1 += b2 x g3,  g_b2 += g3 x b1
  float gb1[3] = {g[0] + (b2[1] * g[8] - b2[2] * g[7]), g[1] + (b2[2] * g[6] - b2[0] * g[8]), g[2] + (b2[0] * g[7] - b2[1] * g[6])};
  const float gb2[3] = {g[3] + (g[7] * b1[2] - g[8] * b1[1]), g[4] + (g[8] * b1[0] - g[6] * b1[2]), g[5] + (g[6] * b1[1] - g[7] * b1[0])};
  float gt[3];
  normalize3_bwd(tmp, gb2, gt);
  // tmp = a2 - dot b1, dot = b1 . a2
  const float g_dot = -(gt[0] * b1[0] + gt[1] * b1[1] + gt[2] * b1[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ga[3 + k] = gt[k] + g_dot * b1[k];
    gb1[k] += g_dot * a[3 + k] - dot * gt[k];
  }
  normalize3_bwd(a, gb1, ga);
}
// d(sum_e g_e R_e) / d(angle) of axis_rot
__device__ __forceinline__ float axis_rot_bwd(int axis, float ang, const float* g) {
  const float c = cosf(ang), s = sinf(ang);
  if (axis == 0) return c * (g[7] - g[5]) - s * (g[4] + g[8]);
  if (axis == 1) return c * (g[2] - g[6]) - s * (g[0] + g[8]);
  return c * (g[3] - g[1]) - s * (g[0] + g[4]);
}
__device__ __forceinline__ void mat3mul_nt(const float* a, const float* b, float* o) {   // a . b^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[i * 3 + j] = a[i * 3] * b[j * 3] + a[i * 3 + 1] * b[j * 3 + 1] + a[i * 3 + 2] * b[j * 3 + 2];
}
__device__ __forceinline__ void mat3mul_tn(const float* a, const float* b, float* o) {   // a^T . b
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[i * 3 + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}
__device__ __forceinline__ void euler_to_mat_bwd(int c0, int c1, int c2, const float* e, const float* g, float* ge) {
  float R0[9], R1[9], R2[9], R01[9], g01[9], gk[9];
  axis_rot(c0, e[0], R0);
  axis_rot(c1, e[1], R1);
  axis_rot(c2, e[2], R2);
  mat3mul(R0, R1, R01);
  mat3mul_tn(R01, g, gk);         // R = R01 R2:  g_R2 = R01^T g,  g_R01 = g R2^T
  ge[2] = axis_rot_bwd(c2, e[2], gk);
  mat3mul_nt(g, R2, g01);
  mat3mul_tn(R0, g01, gk);        // R01 = R0 R1:  g_R1 = R0^T g_R01,  g_R0 = g_R01 R1^T
  ge[1] = axis_rot_bwd(c1, e[1], gk);
  mat3mul_nt(g01, R1, gk);
  ge[0] = axis_rot_bwd(c0, e[0], gk);
}
__device__ __forceinline__ float pick9(const float* a, int i) {      // a[i] as selects (see angle_from_tan)
  return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : i == 3 ? a[3] : i == 4 ? a[4] : i == 5 ? a[5] : i == 6 ? a[6] : i == 7 ? a[7] : a[8];
}
__device__ __forceinline__ void add9(float* a, int i, float v) {     // a[i] += v as selects
#pragma unroll
  for (int k = 0; k < 9; ++k) a[k] += (k == i) ? v : 0.f;
}
// _angle_from_tan's gradient.  Its three forms -- atan2(d1, d2), atan2(-d2, d1), atan2(d2, -d1) -- are one angle up to a
// constant, so one rule serves: g_d1 = g d2 / (d1^2 + d2^2), g_d2 = -g d1 / (d1^2 + d2^2).  f1 / f2 are the FLAT matrix
// indices of data[i1] / data[i2] (after the horizontal swap).
__device__ __forceinline__ void angle_from_tan_bwd(const float* m, int f1, int f2, float g, float* gm) {
  const float d1 = pick9(m, f1), d2 = pick9(m, f2);
  const float s = g / (d1 * d1 + d2 * d2);
  add9(gm, f1, s * d2);
  add9(gm, f2, -s * d1);
}
__device__ __forceinline__ void mat_to_euler_bwd(int c0, int c1, int c2, const float* m, const float* g, float* gm) {
  const bool tb = c0 != c2;
#pragma unroll
  for (int k = 0; k < 9; ++k) gm[k] = 0.f;
  if (tb) {
    const int df = c0 - c2;
    const float sgn = (df == -1 || df == 2) ? -1.0f : 1.0f;
    const float x = pick9(m, c0 * 3 + c2) * sgn;
    add9(gm, c0 * 3 + c2, sgn * g[1] / sqrtf(1.0f - x * x));
  } else {
    const float x = pick9(m, c0 * 4);
    add9(gm, c0 * 4, -g[1] / sqrtf(1.0f - x * x));
  }
  // first angle: data = column c2, picks (i1, i2) of axis c0; third: data = row c0, picks of axis c2, swapped
  const int a1 = c0 == 0 ? 2 : (c0 == 1 ? 0 : 1), a2 = c0 == 0 ? 1 : (c0 == 1 ? 2 : 0);
  angle_from_tan_bwd(m, a1 * 3 + c2, a2 * 3 + c2, g[0], gm);
  const int b1 = c2 == 0 ? 2 : (c2 == 1 ? 0 : 1), b2 = c2 == 0 ? 1 : (c2 == 1 ? 2 : 0);
  angle_from_tan_bwd(m, c0 * 3 + b2, c0 * 3 + b1, g[2], gm);
}

template <int W> __device__ __forceinline__ void rot_item_in(const float* __restrict__ s, int t, float* v) {
  if constexpr (W == 4) {
    const float4 x = ((const float4*)s)[t];
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = s[t * W + k];
  }
}
template <int W> __device__ __forceinline__ void rot_item_out(float* __restrict__ s, int t, const float* v) {
  if constexpr (W == 4) {
    ((float4*)s)[t] = float4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) s[t * W + k] = v[k];
  }
}

// One item's vector-Jacobian product: a (IW) / b (the second operand as a quaternion) / g (OW) -> ga (IW) / gb.
template <int OP, int IW, int OW>
__device__ __forceinline__ void rot_item_bwd(const float* a, const float* b, const float* g, float* ga, float* gb, int conv) {
  if constexpr (OP == MSMD_ROT_QUAT_TO_MAT) {
    quat_to_mat_bwd(a, g, ga);
  } else if constexpr (OP == MSMD_ROT_MAT_TO_QUAT) {
    mat_to_quat_bwd(a, g, ga);
  } else if constexpr (OP == MSMD_ROT_AA_TO_QUAT) {
    aa_to_quat_bwd(a, g, ga);
  } else if constexpr (OP == MSMD_ROT_QUAT_TO_AA) {
    quat_to_aa_bwd(a, g, ga);
  } else if constexpr (OP == MSMD_ROT_AA_TO_MAT || OP == MSMD_ROT_AA_TO_6D) {
    float q[4], gq[4], g9[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g9[k] = k < OW ? g[k < OW ? k : 0] : 0.f;   // the 6-D form drops the last row
    aa_to_quat(a, q);
    quat_to_mat_bwd(q, g9, gq);
    aa_to_quat_bwd(a, gq, ga);
  } else if constexpr (OP == MSMD_ROT_MAT_TO_AA) {
    float q[4], gq[4];
    mat_to_quat(a, q);
    quat_to_aa_bwd(q, g, gq);
    mat_to_quat_bwd(a, gq, ga);
  } else if constexpr (OP == MSMD_ROT_6D_TO_MAT) {
    rot6d_to_mat_bwd(a, g, ga);
  } else if constexpr (OP == MSMD_ROT_MAT_TO_6D) {
#pragma unroll
    for (int k = 0; k < 9; ++k) ga[k] = k < 6 ? g[k < 6 ? k : 0] : 0.f;
  } else if constexpr (OP == MSMD_ROT_EULER_TO_MAT) {
    euler_to_mat_bwd(conv & 3, (conv >> 2) & 3, (conv >> 4) & 3, a, g, ga);
  } else if constexpr (OP == MSMD_ROT_MAT_TO_EULER) {
    mat_to_euler_bwd(conv & 3, (conv >> 2) & 3, (conv >> 4) & 3, a, g, ga);
  } else if constexpr (OP == MSMD_ROT_QUAT_STANDARDIZE) {
    const float s = a[0] < 0.f ? -1.0f : 1.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) ga[k] = s * g[k];
  } else if constexpr (OP == MSMD_ROT_QUAT_INVERT) {
    ga[0] = g[0]; ga[1] = -g[1]; ga[2] = -g[2]; ga[3] = -g[3];
  } else if constexpr (OP == MSMD_ROT_QUAT_RAW_MUL) {
    quat_raw_mul_bwd(a, b, g, ga, gb);
  } else if constexpr (OP == MSMD_ROT_QUAT_MUL) {
    float o[4], gs[4];
    quat_raw_mul(a, b, o);
    const float s = o[0] < 0.f ? -1.0f : 1.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) gs[k] = s * g[k];
    quat_raw_mul_bwd(a, b, gs, ga, gb);
  } else if constexpr (OP == MSMD_ROT_QUAT_APPLY) {
    // out = (a b a^-1)[1:] with b = (0, point) and a^-1 = (a0, -a1, -a2, -a3)
    const float inv[4] = {a[0], -a[1], -a[2], -a[3]};
    const float go[4] = {0.f, g[0], g[1], g[2]};
    float tmp[4], gt[4], gi[4];
    quat_raw_mul(a, b, tmp);
    quat_raw_mul_bwd(tmp, inv, go, gt, gi);
    quat_raw_mul_bwd(a, b, gt, ga, gb);
    ga[0] += gi[0]; ga[1] -= gi[1]; ga[2] -= gi[2]; ga[3] -= gi[3];
  }
}

// Same data movement as rotation_kernel: a workgroup owns 256 consecutive items; x, x2 and gout are staged through LDS in
// linear 16-byte pieces, one item per thread in registers, gx / gx2 go back through the buffers x / x2 came in by.
// One instantiation per op (item widths IW / I2W / OW are compile-time): algorithmic traffic 4 n (2 IW + OW + 2 I2W) bytes.
template <int OP, int IW, int I2W, int OW>
__global__ __launch_bounds__(ROT_WG) void rotation_bwd_kernel(const float* __restrict__ in, const float* __restrict__ in2,
                                                              const float* __restrict__ gout, float* __restrict__ gin,
                                                              float* __restrict__ gin2, long n, int conv) {
  __shared__ __attribute__((aligned(16))) float s_io[ROT_WG * IW];
  __shared__ __attribute__((aligned(16))) float s_b[ROT_WG * (I2W ? I2W : 1)];
  __shared__ __attribute__((aligned(16))) float s_g[ROT_WG * OW];
  const long base = blockIdx.x * (long)ROT_WG;
  const int cnt = (int)min((long)ROT_WG, n - base);
  rot_stage_in(s_io, in + base * IW, cnt * IW);
  if constexpr (I2W != 0) rot_stage_in(s_b, in2 + base * I2W, cnt * I2W);
  rot_stage_in(s_g, gout + base * OW, cnt * OW);
  __syncthreads();
  const int t = threadIdx.x;
  const bool live = t < cnt;
  float a[IW], g[OW], ga[IW], b[4], gb[4];
  if (live) {
    rot_item_in<IW>(s_io, t, a);
    rot_item_in<OW>(s_g, t, g);
    if constexpr (I2W == 4) rot_item_in<4>(s_b, t, b);
    if constexpr (I2W == 3) { b[0] = 0.f; b[1] = s_b[t * 3]; b[2] = s_b[t * 3 + 1]; b[3] = s_b[t * 3 + 2]; }
  }
  __syncthreads();      // every item is in registers: the input buffers become the gradient spans
  if (live) {
    rot_item_bwd<OP, IW, OW>(a, b, g, ga, gb, conv);
    rot_item_out<IW>(s_io, t, ga);
    if constexpr (I2W == 4) rot_item_out<4>(s_b, t, gb);
    if constexpr (I2W == 3) { s_b[t * 3] = gb[1]; s_b[t * 3 + 1] = gb[2]; s_b[t * 3 + 2] = gb[3]; }
  }
  __syncthreads();
  rot_stage_out(gin + base * IW, s_io, cnt * IW);
  if constexpr (I2W != 0) rot_stage_out(gin2 + base * I2W, s_b, cnt * I2W);
}

template <int OP, int IW, int I2W, int OW>
static void rotation_bwd_launch(const float* in, const float* in2, const float* gout, float* gin, float* gin2, long n, int conv,
                                hipStream_t stream) {
  hipLaunchKernelGGL((rotation_bwd_kernel<OP, IW, I2W, OW>), dim3((unsigned)((n + ROT_WG - 1) / ROT_WG)), dim3(ROT_WG), 0, stream,
                     in, in2, gout, gin, gin2, n, conv);
}

extern "C" int msmd_rotation_convert_bwd(int op, const float* in, const float* in2, const float* grad_out, float* grad_in,
                                         float* grad_in2, long n, int conv, msmd_stream_t stream) {
  if (n <= 0 || op < 0 || op > MSMD_ROT_QUAT_APPLY || !in || !grad_out || !grad_in) return 1;
  if ((op == MSMD_ROT_QUAT_RAW_MUL || op == MSMD_ROT_QUAT_MUL || op == MSMD_ROT_QUAT_APPLY) && (!in2 || !grad_in2)) return 1;
  if (op == MSMD_ROT_EULER_TO_MAT || op == MSMD_ROT_MAT_TO_EULER) {
    const int c0 = conv & 3, c1 = (conv >> 2) & 3, c2 = (conv >> 4) & 3;
    if (c0 > 2 || c1 > 2 || c2 > 2 || c1 == c0 || c1 == c2) return 1;
  }
  hipStream_t s = (hipStream_t)stream;
#define MSMD_ROT_BWD(OP, IW, I2W, OW) \
  case OP: rotation_bwd_launch<OP, IW, I2W, OW>(in, in2, grad_out, grad_in, grad_in2, n, conv, s); break;
  switch (op) {
    MSMD_ROT_BWD(MSMD_ROT_QUAT_TO_MAT, 4, 0, 9)
    MSMD_ROT_BWD(MSMD_ROT_MAT_TO_QUAT, 9, 0, 4)
    MSMD_ROT_BWD(MSMD_ROT_AA_TO_QUAT, 3, 0, 4)
    MSMD_ROT_BWD(MSMD_ROT_QUAT_TO_AA, 4, 0, 3)
    MSMD_ROT_BWD(MSMD_ROT_AA_TO_MAT, 3, 0, 9)
    MSMD_ROT_BWD(MSMD_ROT_MAT_TO_AA, 9, 0, 3)
    MSMD_ROT_BWD(MSMD_ROT_6D_TO_MAT, 6, 0, 9)
    MSMD_ROT_BWD(MSMD_ROT_MAT_TO_6D, 9, 0, 6)
    MSMD_ROT_BWD(MSMD_ROT_AA_TO_6D, 3, 0, 6)
    MSMD_ROT_BWD(MSMD_ROT_EULER_TO_MAT, 3, 0, 9)
    MSMD_ROT_BWD(MSMD_ROT_MAT_TO_EULER, 9, 0, 3)
    MSMD_ROT_BWD(MSMD_ROT_QUAT_STANDARDIZE, 4, 0, 4)
    MSMD_ROT_BWD(MSMD_ROT_QUAT_INVERT, 4, 0, 4)
    MSMD_ROT_BWD(MSMD_ROT_QUAT_RAW_MUL, 4, 4, 4)
    MSMD_ROT_BWD(MSMD_ROT_QUAT_MUL, 4, 4, 4)
    MSMD_ROT_BWD(MSMD_ROT_QUAT_APPLY, 4, 3, 3)
    default: return 1;
  }
#undef MSMD_ROT_BWD
  MSMD_RETURN_LAST();
}
