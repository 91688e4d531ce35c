// FLAME, everything but the skinning kernels (lbs_skin.hip): Rodrigues, the per-frame kinematics that write the skinning
// kernels' operands (tile records: lbs_tiles.h), the shape fold, landmarks and the dynamic-contour LUT row.
// Reference: utils/lbs.py:102-371, utils/flame.py:126-244.
#include "lbs_tiles.h"

__device__ __forceinline__ void rodrigues(const float* r, float* R) {
  // reference utils/lbs.py:285-300: angle = ||r + 1e-8||, dir = r / angle (un-shifted r)
  const float x = r[0] + 1e-8f, y = r[1] + 1e-8f, z = r[2] + 1e-8f;
  const float angle = sqrtf(x * x + y * y + z * z);
  const float rx = r[0] / angle, ry = r[1] / angle, rz = r[2] / angle;
  const float s = sinf(angle), c1 = 1.0f - cosf(angle);
  // K = [[0,-rz,ry],[rz,0,-rx],[-ry,rx,0]];  R = I + s K + (1-c) K K
  const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float kk = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) kk += K[i * 3 + k] * K[k * 3 + j];
      R[i * 3 + j] = (i == j ? 1.0f : 0.0f) + s * K[i * 3 + j] + c1 * kk;
    }
}

__global__ void rodrigues_kernel(const float* __restrict__ rv, float* __restrict__ R, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float r[3] = {rv[i * 3], rv[i * 3 + 1], rv[i * 3 + 2]}, o[9];
  rodrigues(r, o);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[(long)i * 9 + k] = o[k];
}

extern "C" int msmd_batch_rodrigues(const float* rot_vecs, float* R, int N, msmd_stream_t stream) {
  if (N <= 0) return 1;
  hipLaunchKernelGGL(rodrigues_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, rot_vecs, R, N);
  MSMD_RETURN_LAST();
}

// Backward of rodrigues(): g_r from g_R (reference: autograd through utils/lbs.py:285-300).  With x = r + 1e-8,
// angle = |x|, d = r / angle, R = I + sin K(d) + (1 - cos) K(d)^2:
//   g_K = sin g + (1 - cos) (g K^T + K^T g),  g_angle = cos sum(g K) + sin sum(g K^2) - (g_d . r) / angle^2,
//   g_r = g_d / angle + x g_angle / angle   (the epsilon sits in the norm only)
__device__ __forceinline__ void rodrigues_bwd(const float* r, const float* g, float* gr) {
  const float x = r[0] + 1e-8f, y = r[1] + 1e-8f, z = r[2] + 1e-8f;
  const float angle = sqrtf(x * x + y * y + z * z);
  const float rx = r[0] / angle, ry = r[1] / angle, rz = r[2] / angle;
  const float s = sinf(angle), c = cosf(angle), sh = sinf(0.5f * angle);
  const float c1 = 2.0f * sh * sh;      // 1 - cos without the cancellation: it scales g_d / angle, where u / angle^2 would show
  const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
  float gK[9];
  float gs = 0.f, gc1 = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float kk = 0.f, t = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        kk += K[i * 3 + k] * K[k * 3 + j];
        t += g[i * 3 + k] * K[j * 3 + k] + K[k * 3 + i] * g[k * 3 + j];   // (g K^T + K^T g)[i][j]
      }
      gs += g[i * 3 + j] * K[i * 3 + j];
      gc1 += g[i * 3 + j] * kk;
      gK[i * 3 + j] = s * g[i * 3 + j] + c1 * t;
    }
  const float gd[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
  const float g_angle = c * gs + s * gc1 - (gd[0] * r[0] + gd[1] * r[1] + gd[2] * r[2]) / (angle * angle);
  const float sc = angle > 0.f ? g_angle / angle : 0.f;
  gr[0] = gd[0] / angle + x * sc; gr[1] = gd[1] / angle + y * sc; gr[2] = gd[2] / angle + z * sc;
}

__global__ void rodrigues_bwd_kernel(const float* __restrict__ rv, const float* __restrict__ gR, float* __restrict__ grv, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float r[3] = {rv[i * 3], rv[i * 3 + 1], rv[i * 3 + 2]};
  float g[9], o[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) g[k] = gR[(long)i * 9 + k];
  rodrigues_bwd(r, g, o);
#pragma unroll
  for (int k = 0; k < 3; ++k) grv[(long)i * 3 + k] = o[k];
}

extern "C" int msmd_batch_rodrigues_bwd(const float* rot_vecs, const float* grad_R, float* grad_rot_vecs, int N,
                                        msmd_stream_t stream) {
  if (N <= 0 || !rot_vecs || !grad_R || !grad_rot_vecs) return 1;
  hipLaunchKernelGGL(rodrigues_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, rot_vecs, grad_R,
                     grad_rot_vecs, N);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
// Per-frame kinematics: 16 frames per 256-thread workgroup, 16 lanes per frame.  (The first version ran one 64-thread
// workgroup per frame with the joint chain serial in lane 0: latency bound, 110 us for 25 600 frames -- a sixth of the
// whole FLAME pass.)  The joint-regression table (9 KB) is staged in LDS once per workgroup and shared by its frames;
// the kinematic chain runs joint by joint (parents[i] < i) with 12 lanes computing the 3x4 entries of a transform.
#define LBS_MAXJ 5     // the launchers take J <= 5 (FLAME: 5 joints)
__global__ __launch_bounds__(256) void lbs_prepare_kernel(const float* __restrict__ betas, const float* __restrict__ pose,
                                                          const float* __restrict__ JS, const int* __restrict__ parents,
                                                          float* __restrict__ coef, bf16_t* __restrict__ coef_hl,
                                                          float* __restrict__ A, float* __restrict__ joints_out, int NB, int J,
                                                          int Kp, int pose_is_matrix, f16_t* __restrict__ at_tiles, int B,
                                                          const float* __restrict__ betas2 = nullptr, int NB1 = 0,
                                                          const float* __restrict__ eye = nullptr, int pose_mode = 0,
                                                          int* __restrict__ shape_varies = nullptr, int kfold = 0) {
  // betas2 != NULL: the coefficient row is [betas (B, NB1) | betas2 (B, NB - NB1)] (FLAME's shape | expression, no
  // concatenated copy).  pose_mode 1 / 2: `pose` is FLAME's (B, 6) [global | jaw] axis-angle input, the neck is the
  // identity, `eye` (B, 6) or NULL = identity; 2 also ignores the global rotation (utils/flame.py:199-207).
  // LDS sized by the launcher for THIS model (lbs_prepare_lds): round 6 found the static arrays for the largest admissible one
  // (NB = 256, J = 8: 49.8 KB) held the launch to three workgroups per CU -- three rounds at 25 600 frames, 58 us of latency.
  // The joint-regression table is dead once the joints are known: the chain's transforms sT / sAo live in its space.
  extern __shared__ __attribute__((aligned(16))) float lbs_prep_smem[];
  const int nbp = NB + 4;
  float* sJS = lbs_prep_smem;                                          // (NB + 1) x 3 J, later sT | sAo
  const int region0 = max((NB + 1) * J * 3, 2 * LBS_FPB * LBS_MAXJ * 12);
  float (*sT)[LBS_MAXJ * 12] = (float (*)[LBS_MAXJ * 12])lbs_prep_smem;
  float (*sAo)[LBS_MAXJ * 12] = (float (*)[LBS_MAXJ * 12])(lbs_prep_smem + LBS_FPB * LBS_MAXJ * 12);
  float* sBf = lbs_prep_smem + region0;                                // [frame][NB + 4]
  float (*sJ)[16] = (float (*)[16])(sBf + LBS_FPB * nbp);
  float (*sR)[LBS_MAXJ * 9] = (float (*)[LBS_MAXJ * 9])(sBf + LBS_FPB * nbp + LBS_FPB * 16);
#define sB(f, k) sBf[(f) * nbp + (k)]
  const int tid = threadIdx.x, fl = tid >> 4, ln = tid & 15;
  const int b = blockIdx.x * LBS_FPB + fl;
  const bool valid = b < B;
  const int bb = valid ? b : B - 1;
  const int J3 = J * 3;
  for (int k = tid; k < (NB + 1) * J3; k += 256) sJS[k] = JS[k];
  if (betas2) {
    const float* b1 = betas + (long)bb * NB1;
    const float* b2 = betas2 + (long)bb * (NB - NB1);
    for (int k = ln; k < NB; k += 16) sB(fl, k) = k < NB1 ? b1[k] : b2[k - NB1];
    if (shape_varies) {   // do the first kfold shape coefficients of this frame differ from frame 0's?  (see lbs_shape_fold)
      bool diff = false;
      for (int k = ln; k < kfold; k += 16) diff |= b1[k] != betas[k];
      if (diff) atomicOr(shape_varies, 1);
    }
  } else {
    const float* be = betas + (long)bb * NB;
    for (int k = ln; k < NB; k += 16) sB(fl, k) = be[k];
  }
  if (ln < J) {
    float R[9];
    if (pose_mode) {
      float r[3] = {0.f, 0.f, 0.f};
      const float* src = nullptr;
      if (ln == 0 && pose_mode == 1) src = pose + (long)bb * 6;
      else if (ln == 2) src = pose + (long)bb * 6 + 3;
      else if (ln >= 3 && eye) src = eye + (long)bb * 6 + (ln - 3) * 3;
      if (src) { r[0] = src[0]; r[1] = src[1]; r[2] = src[2]; }
      rodrigues(r, R);
    } else if (pose_is_matrix) {
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = pose[((long)bb * J + ln) * 9 + k];
    } else {
      const float r[3] = {pose[((long)bb * J + ln) * 3], pose[((long)bb * J + ln) * 3 + 1], pose[((long)bb * J + ln) * 3 + 2]};
      rodrigues(r, R);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) sR[fl][ln * 9 + k] = R[k];
  }
  __syncthreads();
  // joints = J_regressor . (template + sum_l beta_l shapedirs_l): linear in the coefficients -> the JS table
  if (ln < J3) {
    float a0 = sJS[ln], a1 = 0.f;
    int l = 0;
    for (; l + 1 < NB; l += 2) {
      a0 = fmaf(sB(fl, l), sJS[(1 + l) * J3 + ln], a0);
      a1 = fmaf(sB(fl, l + 1), sJS[(2 + l) * J3 + ln], a1);
    }
    if (l < NB) a0 = fmaf(sB(fl, l), sJS[(1 + l) * J3 + ln], a0);
    sJ[fl][ln] = a0 + a1;
  }
  __syncthreads();
  // kinematic chain (utils/lbs.py:317-371): T_0 = [R_0 | J_0]; T_i = T_parent . [R_i | J_i - J_parent]; entry (r, c) = lane
  for (int i = 0; i < J; ++i) {
    if (ln < 12) {
      const int r = ln >> 2, c = ln & 3;
      const int pa = i == 0 ? -1 : parents[i];
      auto loc = [&](int rr) { return c < 3 ? sR[fl][i * 9 + rr * 3 + c] : sJ[fl][i * 3 + rr] - (pa >= 0 ? sJ[fl][pa * 3 + rr] : 0.f); };
      float v;
      if (pa < 0) {
        v = loc(r);
      } else {
        const float* Tp = &sT[fl][pa * 12 + r * 4];
        v = Tp[0] * loc(0) + Tp[1] * loc(1) + Tp[2] * loc(2);
        if (c == 3) v += Tp[3];
      }
      sT[fl][i * 12 + ln] = v;
    }
    __syncthreads();
  }
  // A_i = [R | t - R J_i] (relative to the rest pose); posed joints = translation column of T_i
  for (int e = ln; e < J * 12; e += 16) {
    const int i = e / 12, rc = e - i * 12, r = rc >> 2, c = rc & 3;
    const float* Tr = &sT[fl][i * 12 + r * 4];
    float v = Tr[c];
    if (c == 3) v -= Tr[0] * sJ[fl][i * 3] + Tr[1] * sJ[fl][i * 3 + 1] + Tr[2] * sJ[fl][i * 3 + 2];
    sAo[fl][e] = v;
    if (valid) {
      if (A) A[(long)b * J * 12 + e] = v;
      if (joints_out && c == 3) joints_out[((long)b * J + i) * 3 + r] = Tr[3];
    }
  }
  // coefficient row = [betas | pose_feature = (R[1:] - I) | 0 pad]
  // Tile records (lbs_tiles.h) when at_tiles is given: the launchers admit them for J = 5, Kp = 192 only.
  unsigned char* tile = at_tiles ? (unsigned char*)at_tiles + (long)blockIdx.x * LBS_TILE_BYTES : nullptr;
  {
    float* crow = coef + (long)b * Kp;
    for (int k = ln; k < Kp; k += 16) {
      float v = 0.f;
      if (k < NB) v = sB(fl, k);
      else if (k < NB + (J - 1) * 9) {
        const int pf = k - NB, jj = 1 + pf / 9, rc = pf % 9;
        v = sR[fl][jj * 9 + rc] - ((rc == 0 || rc == 4 || rc == 8) ? 1.0f : 0.0f);
      }
      if (valid && coef) crow[k] = v;
      if (coef_hl || tile) {  // bf16 hi/lo split for the 3-product MFMA form: v ~= hi + lo with 16 significant bits
        bf16_t hi, lo;
        split_bf16_hl(v, hi, lo);
        if (coef_hl && valid) coef_hl_put(coef_hl, b, Kp, k, hi, lo);
        if (tile) tile_put_coef(tile, fl, k, hi, lo);
      }
    }
  }
  if (tile) {
    __syncthreads();
    tile_put_blend(tile, fl, ln, [&](int j, int m) { return sAo[fl][j * 12 + m]; });
  }
}
#undef sB
static size_t lbs_prepare_lds(int NB, int J) {
  const int region0 = max((NB + 1) * J * 3, 2 * LBS_FPB * LBS_MAXJ * 12);
  return sizeof(float) * (size_t)(region0 + LBS_FPB * (NB + 4) + LBS_FPB * 16 + LBS_FPB * LBS_MAXJ * 9);
}

extern "C" int msmd_lbs_prepare(const float* betas, const float* pose, const float* JS, const int* parents,
                                float* coef, void* coef_hl, float* A, float* joints, void* at_tiles, int B, int NB, int J,
                                int Kp, int pose_is_matrix, msmd_stream_t stream) {
  if (B <= 0 || NB <= 0 || NB > 256 || J <= 0 || J > 5 || Kp < NB + (J - 1) * 9 || (at_tiles && (J != LBS_J || Kp != LBS_KP))) return 1;
  hipLaunchKernelGGL(lbs_prepare_kernel, dim3((B + LBS_FPB - 1) / LBS_FPB), dim3(256), lbs_prepare_lds(NB, J), (hipStream_t)stream, betas, pose,
                     JS, parents, coef, (bf16_t*)coef_hl, A, joints, NB, J, Kp, pose_is_matrix, (f16_t*)at_tiles, B);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
// FLAME.forward's inputs straight into the skinning kernel's tile records: shape (B, NS) | expression (B, NE) as the
// coefficient row, pose6 (B, 6) = [global | jaw] axis-angle with the identity neck, eye (B, 6) or NULL (identity eyes):
// no concatenated betas / full_pose tensors.  coef / A / joints are optional outputs.
// One subject, many frames (the usual call: every frame carries the same shape row, or zeros): the first LBS_KFOLD shape
// directions can be added to the template ONCE, v_folded = template + sum_{k < LBS_KFOLD} shape_0[k] dirs[k], and the
// skinning kernel then skips those K groups (27 of its 54 blendshape MFMAs per tile).  Whether the frames really share
// the row is decided on the device (shape_varies, set by the kinematics kernel), so nothing reads back to the host and
// the general path stays one uniform branch away.
__global__ __launch_bounds__(256) void lbs_shape_fold_kernel(const float* __restrict__ shape0, const float* __restrict__ dirs,
                                                             const float* __restrict__ tmpl, float* __restrict__ out,
                                                             int Vp, int Kp, int kfold) {
  // 64 vertices x 4 K slices per workgroup (the first version walked all 96 directions serially in 60 workgroups: 24 us)
  __shared__ float part[4][64];
  const int vl = threadIdx.x & 63, ks = threadIdx.x >> 6;
  const int v = blockIdx.x * 64 + vl, c = blockIdx.y;
  const int kn = kfold / 4, k0 = ks * kn;
  float a = 0.f;
  if (v < Vp) {
    const float* d = dirs + ((long)c * Kp + k0) * Vp + v;
#pragma unroll 8
    for (int k = 0; k < kn; ++k) a = fmaf(shape0[k0 + k], d[(long)k * Vp], a);
  }
  part[ks][vl] = a;
  __syncthreads();
  if (ks == 0 && v < Vp) out[(long)c * Vp + v] = tmpl[(long)c * Vp + v] + ((part[0][vl] + part[1][vl]) + (part[2][vl] + part[3][vl]));
}

extern "C" int msmd_flame_prepare(const float* shape, const float* expr, const float* pose6, const float* eye,
                                  const float* JS, const int* parents, float* coef, float* A, float* joints,
                                  void* skin_tiles, int B, int NS, int NE, int ignore_global_rot, int* shape_varies,
                                  float* v_template_folded, const float* dirs, const float* v_template, int Vp,
                                  msmd_stream_t stream) {
  const int NB = NS + NE, J = LBS_J, Kp = LBS_KP;
  if (B <= 0 || NS <= 0 || NE <= 0 || NB > 256 || Kp < NB + (J - 1) * 9 || !shape || !expr || !pose6 || !skin_tiles) return 1;
  hipStream_t st = (hipStream_t)stream;
  const bool fold = shape_varies && v_template_folded && dirs && v_template && NS >= LBS_KFOLD;
  if (shape_varies) {
    // the fold needs the first LBS_KFOLD coefficients to be shape ones: below that (or without the planes to fold) the flag
    // says "varies", so a skinning call handed it takes the general path instead of reading an unwritten folded template
    hipError_t e = msmd_fill_async(shape_varies, sizeof(int), fold ? 0u : 1u, st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(lbs_prepare_kernel, dim3((B + LBS_FPB - 1) / LBS_FPB), dim3(256), lbs_prepare_lds(NB, J), st, shape, pose6,
                     JS, parents, coef, (bf16_t*)nullptr, A, joints, NB, J, Kp, 0, (f16_t*)skin_tiles, B, expr, NS, eye,
                     ignore_global_rot ? 2 : 1, fold ? shape_varies : (int*)nullptr, LBS_KFOLD);
  if (fold)
    hipLaunchKernelGGL(lbs_shape_fold_kernel, dim3((Vp + 63) / 64, 3), dim3(256), 0, st, shape, dirs, v_template,
                       v_template_folded, Vp, Kp, LBS_KFOLD);
  MSMD_RETURN_LAST();
}

// ---------------------------------------------------------------------------------------------------
// One thread per (frame, landmark): face -> three vertex ids -> three 12-byte vertex reads (ONE dwordx3 each: the gathers are
// what this kernel is made of, and a scalar-per-component version issued nine single-dword requests per thread -- 15.7 M L2
// requests for 25 600 frames, which is what its 139 us were) -> one 12-byte store.  The index chain (idx, faces) is read
// through the read-only path; per-landmark tables are cache resident.
__global__ __launch_bounds__(256) void landmarks_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                        const int* __restrict__ idx, long idx_bs, const float* __restrict__ bary,
                                                        long bary_bs, float* __restrict__ out, int B, int V, int L) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * L) return;
  const int b = t / L, l = t - b * L;
  const int face = __ldg(idx + b * idx_bs + l);
  const I3 vi = *(const I3*)(faces + (long)face * 3);
  const F3 bc = *(const F3*)(bary + b * bary_bs + (long)l * 3);
  const float* vb = verts + (long)b * V * 3;
  const F3 p0 = *(const F3*)(vb + (long)vi.a * 3), p1 = *(const F3*)(vb + (long)vi.b * 3), p2 = *(const F3*)(vb + (long)vi.c * 3);
  F3 o;      // the reference's order of accumulation (utils/lbs.py:136: sum over the three corners, corner 0 first)
  o.x = p0.x * bc.x; o.y = p0.y * bc.x; o.z = p0.z * bc.x;
  o.x += p1.x * bc.y; o.y += p1.y * bc.y; o.z += p1.z * bc.y;
  o.x += p2.x * bc.z; o.y += p2.y * bc.z; o.z += p2.z * bc.z;
  *(F3*)(out + (long)t * 3) = o;
}

extern "C" int msmd_landmarks(const float* verts, const int* faces, const int* lmk_faces_idx, long idx_bstride,
                              const float* bary, long bary_bstride, float* out, int B, int V, int L,
                              msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || L <= 0) return 1;
  hipLaunchKernelGGL(landmarks_kernel, dim3((B * L + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, faces,
                     lmk_faces_idx, idx_bstride, bary, bary_bstride, out, B, V, L);
  MSMD_RETURN_LAST();
}

// Backward of landmarks_kernel: the (B, L, 3) landmark gradients scattered to the (B, V, 3) vertex gradients.  Several
// landmarks may share a vertex and the sum must be the same from run to run, so there are no atomics: one workgroup per frame
// lists the frame's 3 L contributions (vertex id, barycentric weight x landmark gradient) in LDS in (landmark, corner) order;
// the FIRST contribution of each vertex id owns that vertex and adds up all contributions of the same id in list order,
// then stores (accumulate = 0) or adds into (accumulate != 0) the vertex gradient.  With accumulate = 0 the same launch
// zero-fills the frame's other vertices first (a barrier orders the fill before the owners' stores).
#define LMK_BWD_MAXL MSMD_LANDMARKS_BWD_MAX_L
__global__ __launch_bounds__(256) void landmarks_bwd_kernel(const float* __restrict__ glmk, const int* __restrict__ faces,
                                                            const int* __restrict__ idx, long idx_bs,
                                                            const float* __restrict__ bary, long bary_bs,
                                                            float* __restrict__ gverts, int V, int L, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float s_lmk[];
  const int C = 3 * L;
  float* s_val = s_lmk;                 // (C, 3)
  int* s_vid = (int*)(s_lmk + 3 * C);   // (C)
  const int b = blockIdx.x;
  float* gv = gverts + (long)b * V * 3;
  for (int c = threadIdx.x; c < C; c += 256) {
    const int l = c / 3, k = c - l * 3;
    const int face = __ldg(idx + b * idx_bs + l);
    const float w = bary[b * bary_bs + (long)l * 3 + k];
    const float* gp = glmk + ((long)b * L + l) * 3;
    s_vid[c] = __ldg(faces + (long)face * 3 + k);
    s_val[c * 3] = gp[0] * w; s_val[c * 3 + 1] = gp[1] * w; s_val[c * 3 + 2] = gp[2] * w;
  }
  if (!accumulate) {
    const int nw = V * 3;
    if ((((uintptr_t)gv) & 15) == 0) {
      const int nv = nw >> 2;
      for (int i = threadIdx.x; i < nv; i += 256) ((float4*)gv)[i] = float4{0.f, 0.f, 0.f, 0.f};
      for (int i = (nv << 2) + threadIdx.x; i < nw; i += 256) gv[i] = 0.f;
    } else {
      for (int i = threadIdx.x; i < nw; i += 256) gv[i] = 0.f;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    const int vid = s_vid[c];
    bool owner = (unsigned)vid < (unsigned)V;      // an id outside the mesh owns nothing
    for (int p = 0; p < c && owner; ++p) owner = s_vid[p] != vid;
    if (!owner) continue;
    float sx = s_val[c * 3], sy = s_val[c * 3 + 1], sz = s_val[c * 3 + 2];
    for (int p = c + 1; p < C; ++p)
      if (s_vid[p] == vid) { sx += s_val[p * 3]; sy += s_val[p * 3 + 1]; sz += s_val[p * 3 + 2]; }
    float* o = gv + (long)vid * 3;
    if (accumulate) { sx += o[0]; sy += o[1]; sz += o[2]; }
    o[0] = sx; o[1] = sy; o[2] = sz;
  }
}

extern "C" int msmd_landmarks_bwd(const float* grad_lmk, const int* faces, const int* lmk_faces_idx, long idx_bstride,
                                  const float* bary, long bary_bstride, float* grad_verts, int B, int V, int L, int accumulate,
                                  msmd_stream_t stream) {
  if (B <= 0 || V <= 0 || L <= 0 || L > LMK_BWD_MAXL || !grad_lmk || !faces || !lmk_faces_idx || !bary || !grad_verts) return 1;
  hipLaunchKernelGGL(landmarks_bwd_kernel, dim3(B), dim3(256), (size_t)L * 3 * 4 * sizeof(float), (hipStream_t)stream, grad_lmk,
                     faces, lmk_faces_idx, idx_bstride, bary, bary_bstride, grad_verts, V, L, accumulate);
  MSMD_RETURN_LAST();
}

// LUT row of utils/flame.py:126-172: relative neck rotation -> yaw degrees -> row in [0, 78].  The pose is axis-angle
// (pose2rot=True, J x 3) or row-major rotation matrices (pose2rot=False, J x 9).
__global__ void dyn_lmk_row_kernel(const float* __restrict__ full_pose, const int* __restrict__ chain, int n_chain,
                                   int* __restrict__ row, int B, int J, int pose_is_matrix) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float rel[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  for (int n = 0; n < n_chain; ++n) {
    const int j = chain[n];
    float r[3] = {0.f, 0.f, 0.f};
    if (!pose_is_matrix) {
      r[0] = full_pose[((long)b * J + j) * 3];
      r[1] = full_pose[((long)b * J + j) * 3 + 1];
      r[2] = full_pose[((long)b * J + j) * 3 + 2];
    }
    float R[9], o[9];
    if (pose_is_matrix) {
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = full_pose[((long)b * J + j) * 9 + k];
    } else {
      rodrigues(r, R);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) o[i * 3 + k] = R[i * 3] * rel[k] + R[i * 3 + 1] * rel[3 + k] + R[i * 3 + 2] * rel[6 + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) rel[k] = o[k];
  }
  const float sy = sqrtf(rel[0] * rel[0] + rel[3] * rel[3]);
  const float ang = atan2f(-rel[6], sy) * 180.0f / 3.14159265358979323846f;
  long y = (long)rintf(fminf(ang, 39.0f));  // torch.round = round-half-to-even
  const long neg = y < 0 ? 1 : 0, m = y < -39 ? 1 : 0;
  const long neg_vals = m * 78 + (1 - m) * (39 - y);
  row[b] = (int)(neg * neg_vals + (1 - neg) * y);
}

extern "C" int msmd_dynamic_lmk_row(const float* full_pose, const int* neck_chain, int n_chain, int* row, int B, int J,
                                    int pose_is_matrix, msmd_stream_t stream) {
  if (B <= 0 || n_chain <= 0) return 1;
  hipLaunchKernelGGL(dyn_lmk_row_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, full_pose,
                     neck_chain, n_chain, row, B, J, pose_is_matrix);
  MSMD_RETURN_LAST();
}
