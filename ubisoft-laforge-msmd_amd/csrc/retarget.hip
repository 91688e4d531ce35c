// FLAME motion onto a blendshape rig (include/msmd_hip.h states the operator and the solver): per frame the
// weights w in a box that bring neutral + sum_k w_k delta_k closest to the frame's vertices.
//
//   retarget_gram_kernel   G = A A^T in float64, once per rig: one workgroup per (k, l <= k), a fixed strided sum and tree.
//   retarget_rhs_kernel    b = A . fl32(x - neutral) in fp32 on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): THE HOT PATH.
//                          A workgroup owns RT_FT frames x all 64 padded columns of one contraction split; it walks the split
//                          RT_VT vertices at a time: the next tile's x and A values are loaded into registers while the
//                          current tile's differences (and A) sit in LDS for the MFMAs.  x is read once; A (3 MB) lives in L2.
//                          Eight waves; wave w owns frames 16 w .. 16 w + 15 and four 16 x 16 accumulators (columns 16 cb + lane % 16).
//                          The split is MSMD_RETARGET_SPLIT_VERTICES vertices, a constant: what a frame's partial sums are and the
//                          order retarget_reduce_kernel adds them in depend on V alone.
//   retarget_solve_kernel  block principal pivoting for the box in float64: one wave per frame, H in LDS for the workgroup's
//                          waves, the Cholesky and the triangular solves of wave_chol.h.  No workgroup barrier after the staging:
//                          a wave leaves its loop when its own frame is done.
//   blendshape_apply_kernel  out = neutral + sum_k w_k delta_k, an fmaf chain in ascending k; a thread owns one coordinate of
//                          RT_AF frames, so a delta is loaded once per RT_AF frames.
#include "common.h"
#include "wave_chol.h"

constexpr int RT_K = MSMD_RETARGET_MAX_SHAPES;       // 64: one weight per lane
constexpr int RT_FT = MSMD_RETARGET_FRAME_TILE;
constexpr int RT_VT = MSMD_RETARGET_VERTEX_TILE;
constexpr int RT_CE = 3 * RT_VT;                     // contraction elements per tile
constexpr int RT_PITCH = RT_CE + 2;                  // 98 = 2 mod 32: lane (m, q) of an operand's ds_read_b32 meets bank 2 m + q, distinct in each half-wave
constexpr int RT_WG = 512;                           // eight waves: wave w owns frames 16 w .. 16 w + 15
constexpr int RT_XR = RT_FT * RT_CE / RT_WG;         // values of x a thread stages per tile
constexpr int RT_AR = RT_K * RT_CE / RT_WG;          // and of A
constexpr int RT_SF = MSMD_RETARGET_SOLVE_FRAMES;
constexpr int RT_AF = MSMD_RETARGET_APPLY_FRAMES;
constexpr int RT_HP = RT_K + 1;                      // row pitch of H in LDS: one row per lane meets no bank twice
static_assert(RT_K == 64 && RT_FT == 16 * (RT_WG / 64) && RT_CE % 32 == 0 && RT_CE % 4 == 0 && RT_XR * RT_WG == RT_FT * RT_CE &&
              RT_AR * RT_WG == RT_K * RT_CE, "tile shape");
static_assert(MSMD_RETARGET_SPLIT_VERTICES % RT_VT == 0, "a split is whole tiles");

// ------------------------------------------------------------------------------------------------ gram
struct RetargetRidge { double v[RT_K]; };

__global__ __launch_bounds__(256) void retarget_gram_kernel(const float* __restrict__ A, const RetargetRidge ridge,
                                                            double* __restrict__ G, double* __restrict__ H, int K, long E) {
  __shared__ double red[256];
  const int k = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  if (l > k) return;
  const float* __restrict__ ak = A + (long)k * E;
  const float* __restrict__ al = A + (long)l * E;
  double s = 0.0;
  for (long j = tid; j < E; j += 256) s = fma((double)ak[j], (double)al[j], s);
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double g = red[0];
    G[(long)k * K + l] = g;
    G[(long)l * K + k] = g;
    const double h = k == l ? g + ridge.v[k] : g;
    H[(long)k * K + l] = h;
    H[(long)l * K + k] = h;
  }
}

extern "C" int msmd_retarget_gram(const float* A, const double* ridge, double* G, double* H, int K, int V, msmd_stream_t stream) {
  if (!A || !G || !H || K < 1 || K > RT_K || V < 1 || V > MSMD_RETARGET_MAX_VERTICES) return 1;
  RetargetRidge r;
  for (int k = 0; k < RT_K; ++k) {
    r.v[k] = ridge && k < K ? ridge[k] : 0.0;
    if (!(r.v[k] >= 0.0)) return 1;
  }
  hipLaunchKernelGGL(retarget_gram_kernel, dim3(K, K), dim3(256), 0, (hipStream_t)stream, A, r, G, H, K, 3L * V);
  MSMD_RETURN_LAST();
}

// ------------------------------------------------------------------------------------------------ rhs
struct RhsTile { float x[RT_XR], a[RT_AR]; };

// Thread (cl, r0) = (tid & 31, tid >> 5) stages columns cl + 32 j, j < RT_CE / 32, of the frame rows r0 + 16 i, i < RT_FT / 16, and of
// the rows r0 + 16 i, i < RT_K / 16, of A: a wave's load is two rows of 32 consecutive floats.  A vertex whose weight is zero, a column past the split and a frame past N are not read:
// their loads are pointed at neutral[0] and the value is dropped, so every load is unconditional and the compiler can issue a
// tile's loads back to back (a load under a branch is waited for at the branch's end, one at a time).
__device__ __forceinline__ void rhs_load(RhsTile& t, const float* __restrict__ x, const float* __restrict__ neutral,
                                         const float* __restrict__ A, const float* __restrict__ vw, long f0, int N, int K, long E,
                                         long e0, int ne, int tid) {
  const int cl = tid & 31, r0 = tid >> 5;
#pragma unroll
  for (int j = 0; j < RT_CE / 32; ++j) {
    const int c = cl + 32 * j;
    const bool in = c < ne;
    const long e = in ? e0 + c : 0;
    const bool used = in && (vw == nullptr || vw[e / 3] != 0.0f);
    const float nv = neutral[e];
#pragma unroll
    for (int i = 0; i < RT_FT / 16; ++i) {
      const long f = f0 + r0 + 16 * i;
      const bool xr = used && f < N;
      const float xv = *(xr ? x + f * E + e : neutral);
      t.x[j * (RT_FT / 16) + i] = xr ? xv - nv : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < RT_K / 16; ++i) {
      const int r = r0 + 16 * i;
      const bool ar = in && r < K;
      const float av = *(ar ? A + (long)r * E + e : neutral);
      t.a[j * (RT_K / 16) + i] = ar ? av : 0.0f;
    }
  }
}

__global__ __launch_bounds__(RT_WG) void retarget_rhs_kernel(const float* __restrict__ x, const float* __restrict__ neutral,
                                                           const float* __restrict__ A, const float* __restrict__ vw,
                                                           float* __restrict__ partial, int N, int V, int K) {
  __shared__ float sD[RT_FT * RT_PITCH];
  __shared__ float sA[RT_K * RT_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, m = lane & 15, q = lane >> 4;
  const int cl = tid & 31, r0 = tid >> 5;
  const long f0 = (long)blockIdx.x * RT_FT, E = 3L * V;
  const int split = blockIdx.y;
  const int v_begin = split * MSMD_RETARGET_SPLIT_VERTICES;
  const int v_end = min(V, v_begin + MSMD_RETARGET_SPLIT_VERTICES);
  f32x4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  RhsTile t;
  rhs_load(t, x, neutral, A, vw, f0, N, K, E, 3L * v_begin, min(RT_CE, 3 * (v_end - v_begin)), tid);
  for (int vt = v_begin; vt < v_end; vt += RT_VT) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RT_CE / 32; ++j) {
#pragma unroll
      for (int i = 0; i < RT_FT / 16; ++i) sD[(r0 + 16 * i) * RT_PITCH + cl + 32 * j] = t.x[j * (RT_FT / 16) + i];
    }
#pragma unroll
    for (int j = 0; j < RT_CE / 32; ++j) {
#pragma unroll
      for (int i = 0; i < RT_K / 16; ++i) sA[(r0 + 16 * i) * RT_PITCH + cl + 32 * j] = t.a[j * (RT_K / 16) + i];
    }
    __syncthreads();
    const int vn = vt + RT_VT;
    if (vn < v_end) rhs_load(t, x, neutral, A, vw, f0, N, K, E, 3L * vn, min(RT_CE, 3 * (v_end - vn)), tid);
    const float* __restrict__ dp = sD + (16 * wid + m) * RT_PITCH + q;
    const float* __restrict__ ap = sA + m * RT_PITCH + q;
#pragma unroll 6
    for (int kk = 0; kk < RT_CE / 4; ++kk) {
      const float d = dp[4 * kk];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(d, ap[16 * cb * RT_PITCH + 4 * kk], acc[cb], 0, 0, 0);
    }
  }
  // accumulator: frame 16 wid + 4 q + e, column 16 cb + m
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long f = f0 + 16 * wid + 4 * q + e;
    if (f >= N) continue;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int k = 16 * cb + m;
      if (k < K) partial[((long)split * N + f) * K + k] = acc[cb][e];
    }
  }
}

// b = the splits' partial sums, added in ascending split order.
__global__ __launch_bounds__(256) void retarget_reduce_kernel(const float* __restrict__ partial, float* __restrict__ b, long NK, int S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= NK) return;
  float s = partial[i];
  for (int sp = 1; sp < S; ++sp) s += partial[(long)sp * NK + i];
  b[i] = s;
}

extern "C" int msmd_retarget_splits(int V) {
  return V < 1 ? 0 : (V + MSMD_RETARGET_SPLIT_VERTICES - 1) / MSMD_RETARGET_SPLIT_VERTICES;
}

extern "C" int msmd_retarget_rhs(const float* x, const float* neutral, const float* A, const float* vertex_weight, float* partial,
                                 float* b, int N, int V, int K, msmd_stream_t stream) {
  if (N < 0 || K < 1 || K > RT_K || V < 1 || V > MSMD_RETARGET_MAX_VERTICES) return 1;
  if (N == 0) return 0;
  if (!x || !neutral || !A || !partial || !b) return 1;
  const int S = msmd_retarget_splits(V);
  hipLaunchKernelGGL(retarget_rhs_kernel, dim3((unsigned)((N + RT_FT - 1) / RT_FT), (unsigned)S), dim3(RT_WG), 0, (hipStream_t)stream,
                     x, neutral, A, vertex_weight, partial, N, V, K);
  const long NK = (long)N * K;
  hipLaunchKernelGGL(retarget_reduce_kernel, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)partial, b, NK, S);
  MSMD_RETURN_LAST();
}

// ------------------------------------------------------------------------------------------------ solve
struct RetargetSolveArgs {
  const double* H;     // (K, K)
  const float* b;      // (N, K)
  float* w;            // (N, K)
  int* status;         // (N)
  int* iterations;     // (N)
  int N, K, cap;
  double lo[RT_K], hi[RT_K];
};

__host__ __device__ constexpr int rt_wave_doubles(int K) { return WCHOL_COL + RT_K + wchol_packed(K); }

__global__ __launch_bounds__(64 * RT_SF) void retarget_solve_kernel(const RetargetSolveArgs p) {
  extern __shared__ __attribute__((aligned(16))) double rt_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, K = p.K;
  double* __restrict__ sH = rt_smem;                                   // K rows of pitch RT_HP
  double* __restrict__ col = rt_smem + K * RT_HP + wid * rt_wave_doubles(K);
  double* __restrict__ wv = col + WCHOL_COL;                           // the wave's weights, one per lane
  double* __restrict__ sL = wv + RT_K;
  for (int idx = tid; idx < K * RT_K; idx += 64 * RT_SF) {
    const int i = idx >> 6, j = idx & 63;
    sH[i * RT_HP + j] = j < K ? p.H[(long)i * K + j] : 0.0;
  }
  __syncthreads();
  const long fr = (long)blockIdx.x * RT_SF + wid;
  const bool live = fr < p.N;                       // a wave past the last frame solves that frame again and writes nothing
  const long frame = live ? fr : p.N - 1;
  const bool mine = lane < K;
  const double lo = mine ? p.lo[lane] : 0.0, hi = mine ? p.hi[lane] : 0.0;     // a padding weight sits at 0 with g = 0: never infeasible
  const double bi = mine ? (double)p.b[frame * K + lane] : 0.0;
  const bool bad = __any(!isfinite(bi));
  const double* __restrict__ row = sH + (mine ? lane : 0) * RT_HP;         // a padding lane reads row 0 and drops what it computes
  const int ti = lane >> 3, tj = lane & 7;
  int st = 0, budget = 3, best = K + 1, it = 0, status = 0;           // st: 0 at lo, 1 free, 2 at hi
  double w = lo;
  while (!bad) {
    ++it;
    const unsigned long long free_mask = __ballot(st == 1);
    const double wb = st == 0 ? lo : (st == 2 ? hi : 0.0);
    wave_sync();
    wv[lane] = wb;
    wave_sync();
    double r = bi;
    for (int j = 0; j < K; ++j) r = fma(-row[j], wv[j], r);             // the free weights stand at 0 here
    double acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int i = a * 8 + ti, j = b * 8 + tj;
        const bool ff = ((free_mask >> i) & 1ull) && ((free_mask >> j) & 1ull);
        const double h = sH[(ff ? i : 0) * RT_HP + (ff ? j : 0)];          // a bound or padding weight reads H[0][0] and drops it
        acc[a][b] = ff ? h : (i == j ? 1.0 : 0.0);
      }
    if (!wave_cholesky(lane, K, col, sL, acc)) { status = 3; break; }
    w = wave_chol_solve(lane, K, sL, st == 1 ? r : wb);
    if (st != 1) w = wb;
    wave_sync();
    wv[lane] = w;
    wave_sync();
    double g = -bi;
    for (int j = 0; j < K; ++j) g = fma(row[j], wv[j], g);
    const bool to_lo = mine && st == 1 && w < lo, to_hi = mine && st == 1 && w > hi;
    const bool to_free = mine && ((st == 0 && g < 0.0) || (st == 2 && g > 0.0));
    const unsigned long long inf = __ballot(to_lo || to_hi || to_free);
    const int n_inf = __popcll(inf);
    if (n_inf == 0) break;
    if (it >= p.cap) { status = 1; break; }
    bool all = true;
    if (n_inf < best) { best = n_inf; budget = 3; }
    else if (budget > 0) --budget;
    else all = false;
    if (all || lane == 63 - __clzll(inf)) st = to_lo ? 0 : (to_hi ? 2 : (to_free ? 1 : st));
  }
  if (!live || !mine) return;
  const double nanv = __builtin_nan("");
  const double out = bad || status == 3 ? nanv : fmin(fmax(w, lo), hi);
  p.w[frame * K + lane] = (float)out;
  if (lane == 0) {
    p.status[frame] = bad ? 2 : status;
    p.iterations[frame] = it;
  }
}

extern "C" int msmd_retarget_solve(const double* H, const float* b, const double* lo, const double* hi, float* w, int* status,
                                   int* iterations, int N, int K, int max_iterations, msmd_stream_t stream) {
  if (N < 0 || K < 1 || K > RT_K || max_iterations < 1 || max_iterations > MSMD_RETARGET_MAX_ITERATIONS) return 1;
  RetargetSolveArgs p;
  for (int k = 0; k < RT_K; ++k) {
    p.lo[k] = k < K ? (lo ? lo[k] : 0.0) : 0.0;
    p.hi[k] = k < K ? (hi ? hi[k] : 1.0) : 0.0;
    if (k < K && !(p.lo[k] < p.hi[k] && __builtin_isfinite(p.lo[k]) && __builtin_isfinite(p.hi[k]))) return 1;
  }
  if (N == 0) return 0;
  if (!H || !b || !w || !status || !iterations) return 1;
  p.H = H; p.b = b; p.w = w; p.status = status; p.iterations = iterations;
  p.N = N; p.K = K; p.cap = max_iterations;
  const size_t lds = sizeof(double) * ((size_t)K * RT_HP + (size_t)RT_SF * rt_wave_doubles(K));
  static bool attr_set = false;      // idempotent: the same value every time
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)retarget_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL(retarget_solve_kernel, dim3((unsigned)((N + RT_SF - 1) / RT_SF)), dim3(64 * RT_SF), lds, (hipStream_t)stream, p);
  MSMD_RETURN_LAST();
}

// ------------------------------------------------------------------------------------------------ apply
__global__ __launch_bounds__(256) void blendshape_apply_kernel(const float* __restrict__ w, const float* __restrict__ neutral,
                                                               const float* __restrict__ deltas, float* __restrict__ out, int N,
                                                               long E, int K) {
  __shared__ __attribute__((aligned(16))) float sW[RT_K * RT_AF];
  const int tid = threadIdx.x;
  const long f0 = (long)blockIdx.y * RT_AF;
  for (int idx = tid; idx < K * RT_AF; idx += 256) {
    const int k = idx / RT_AF, f = idx % RT_AF;
    sW[idx] = f0 + f < N ? w[(f0 + f) * K + k] : 0.0f;
  }
  __syncthreads();
  const long j = (long)blockIdx.x * 256 + tid;
  if (j >= E) return;
  float acc[RT_AF];
  const float nv = neutral[j];
#pragma unroll
  for (int f = 0; f < RT_AF; ++f) acc[f] = nv;
  for (int k = 0; k < K; ++k) {
    const float d = deltas[(long)k * E + j];
#pragma unroll
    for (int f = 0; f < RT_AF; ++f) acc[f] = fmaf(sW[k * RT_AF + f], d, acc[f]);
  }
#pragma unroll
  for (int f = 0; f < RT_AF; ++f)
    if (f0 + f < N) out[(f0 + f) * E + j] = acc[f];
}

extern "C" int msmd_blendshape_apply(const float* w, const float* neutral, const float* deltas, float* out, int N, int V, int K,
                                     msmd_stream_t stream) {
  if (N < 0 || N > 65535 * RT_AF || K < 1 || K > RT_K || V < 1 || V > MSMD_RETARGET_MAX_VERTICES) return 1;
  if (N == 0) return 0;
  if (!w || !neutral || !deltas || !out) return 1;
  const long E = 3L * V;
  hipLaunchKernelGGL(blendshape_apply_kernel, dim3((unsigned)((E + 255) / 256), (unsigned)((N + RT_AF - 1) / RT_AF)), dim3(256), 0,
                     (hipStream_t)stream, w, neutral, deltas, out, N, E, K);
  MSMD_RETURN_LAST();
}
