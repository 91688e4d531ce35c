// FLAMETex albedo model (reference utils/flame.py:247-301): texture = mean + basis . code over the
// (Hs, Ws, 3) source image, nearest-resized to (Hd, Wd), channels reversed.  The reference expression reads all Hs Ws 3 rows of
// the basis, materialises the product and then drops the rows the resize does not select; these kernels read the surviving
// rows only.  A destination pixel's three rows are one contiguous run of 3 n_tex floats of the module's own buffer.
#include "common.h"

#define FT_MAX_SIDE MSMD_FLAMETEX_MAX_SIDE
#define FT_MAX_TEX MSMD_FLAMETEX_MAX_TEX
#define FT_GROUP 16                 // lanes per destination pixel in the forward kernel (4 pixels per wave)
#define FT_FWD_THREADS 256
#define FT_BWD_THREADS 256
#define FT_BWD_ELEMS 3              // 3 FT_MAX_TEX / FT_BWD_THREADS: elements of a pixel's run per backward thread
#define FT_BWD_MAX_BLOCKS 2048
#define FT_BWD_MIN_PIXELS 8
#define FT_RED_K 16                 // reduction kernel: 16 columns x 64 segments per workgroup
#define FT_RED_SEG 64

// F.interpolate's nearest rule: min(int(floorf(d * scale)), S - 1), scale = (float)S / (float)D divided on the host
__device__ __forceinline__ int ft_src(int d, float scale, int S) { return min((int)floorf((float)d * scale), S - 1); }

__device__ __forceinline__ unsigned ft_u8(float c) {
  return (unsigned)floorf(fmaf(255.f, fminf(fmaxf(c, 0.f), 1.f), 0.5f));       // fmaxf(NaN, 0) = 0
}

// One group of FT_GROUP lanes per destination pixel.  Lane l takes columns l, l + 16, ... of the pixel's three rows in
// ascending order (three fma chains), the group adds its 16 partial sums by the xor butterfly 8, 4, 2, 1, and lane ch adds
// row ch's mean and stores channel 2 - ch.  The summation order is a function of n_tex alone.
template <bool U8>
__global__ __launch_bounds__(FT_FWD_THREADS) void flametex_fwd_kernel(
    const float* __restrict__ mean, const float* __restrict__ basis, const float* __restrict__ code, void* __restrict__ out,
    int n_copies, int Hs, int Ws, int Hd, int Wd, int n_tex, float scale_y, float scale_x) {
  __shared__ float code_s[FT_MAX_TEX];
  for (int k = threadIdx.x; k < n_tex; k += FT_FWD_THREADS) code_s[k] = code[k];
  __syncthreads();
  const int n_pix = Hd * Wd;                                 // <= 2^24
  const int p = blockIdx.x * (FT_FWD_THREADS / FT_GROUP) + threadIdx.x / FT_GROUP;
  const int l = threadIdx.x % FT_GROUP;
  const bool live = p < n_pix;
  const int y = live ? p / Wd : 0, x = live ? p - y * Wd : 0;
  const long row0 = ((long)ft_src(y, scale_y, Hs) * Ws + ft_src(x, scale_x, Ws)) * 3;
  const float* __restrict__ run = basis + row0 * n_tex;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  if (live) {
#pragma unroll 4
    for (int k = l; k < n_tex; k += FT_GROUP) {
      const float c = code_s[k];
      a0 = fmaf(run[k], c, a0);
      a1 = fmaf(run[n_tex + k], c, a1);
      a2 = fmaf(run[2 * n_tex + k], c, a2);
    }
  }
#pragma unroll
  for (int o = FT_GROUP / 2; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o, FT_GROUP);
    a1 += __shfl_xor(a1, o, FT_GROUP);
    a2 += __shfl_xor(a2, o, FT_GROUP);
  }
  if (!live || l >= 3) return;
  const float v = mean[row0 + l] + (l == 0 ? a0 : l == 1 ? a1 : a2);
  const int c = 2 - l;
  if constexpr (U8) {
    ((unsigned char*)out)[(long)p * 3 + c] = (unsigned char)ft_u8(v);
  } else {
    float* o = (float*)out + (long)c * n_pix + p;
    for (int b = 0; b < n_copies; ++b) o[(long)b * 3 * n_pix] = v;
  }
}

static bool ft_sizes_ok(int Hs, int Ws, int Hd, int Wd, int n_tex) {
  return Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1 && Hs <= FT_MAX_SIDE && Ws <= FT_MAX_SIDE && Hd <= FT_MAX_SIDE &&
         Wd <= FT_MAX_SIDE && n_tex >= 1 && n_tex <= FT_MAX_TEX;
}

extern "C" int msmd_flametex_forward(const float* mean, const float* basis, const float* code, void* out, int out_format,
                                     int n_copies, int Hs, int Ws, int Hd, int Wd, int n_tex, msmd_stream_t stream) {
  if (!ft_sizes_ok(Hs, Ws, Hd, Wd, n_tex) || n_copies < 0) return (int)hipErrorInvalidValue;
  if (out_format != MSMD_TEX_PLANAR_F32 && out_format != MSMD_TEX_IMAGE_U8) return (int)hipErrorInvalidValue;
  if (n_copies == 0) return (int)hipSuccess;
  if (out_format == MSMD_TEX_IMAGE_U8 && n_copies != 1) return (int)hipErrorInvalidValue;
  const float sy = (float)Hs / (float)Hd, sx = (float)Ws / (float)Wd;
  const long n_pix = (long)Hd * Wd;
  const int per_block = FT_FWD_THREADS / FT_GROUP;
  const dim3 grid((unsigned)((n_pix + per_block - 1) / per_block)), block(FT_FWD_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (out_format == MSMD_TEX_IMAGE_U8)
    hipLaunchKernelGGL(flametex_fwd_kernel<true>, grid, block, 0, st, mean, basis, code, out, n_copies, Hs, Ws, Hd, Wd, n_tex,
                       sy, sx);
  else
    hipLaunchKernelGGL(flametex_fwd_kernel<false>, grid, block, 0, st, mean, basis, code, out, n_copies, Hs, Ws, Hd, Wd, n_tex,
                       sy, sx);
  MSMD_RETURN_LAST();
}

// ------------------------------------------------------------------------------------------------ backward
// grad_code[k] = sum over destination pixels and channels of basis[row, k] * (sum over copies of grad_out).  A workgroup owns a
// run of consecutive destination pixels; thread t owns elements t, t + 256, t + 512 of every pixel's 3 n_tex run (one
// coalesced read of the run per pixel; NI = ceil(3 n_tex / 256) of them exist) and adds them over the workgroup's pixels in
// pixel order.  The three channels of a column are then added through LDS as (ch 0 + ch 1) + ch 2 and the n_tex sums go to the
// workgroup's row of the workspace.  The loop body has no branch (a thread past the run's end re-reads the last element
// and its sum is dropped), so the loads of several pixels are in flight at once; ONE = a single copy, the usual call.
static int ft_bwd_pixels_per_block(int n_pix) {
  const int per = (n_pix + FT_BWD_MAX_BLOCKS - 1) / FT_BWD_MAX_BLOCKS;
  return per < FT_BWD_MIN_PIXELS ? FT_BWD_MIN_PIXELS : per;
}
static int ft_bwd_blocks(int n_pix) {
  const int per = ft_bwd_pixels_per_block(n_pix);
  return (n_pix + per - 1) / per;
}

template <int NI, bool ONE>
__global__ __launch_bounds__(FT_BWD_THREADS) void flametex_bwd_partial_kernel(
    const float* __restrict__ basis, const float* __restrict__ grad_out, int n_copies, float* __restrict__ workspace, int Hs,
    int Ws, int Hd, int Wd, int n_tex, float scale_y, float scale_x, int per_block) {
  __shared__ float sums[FT_BWD_ELEMS * FT_BWD_THREADS];
  const int E = 3 * n_tex, t = threadIdx.x;
  const int n_pix = Hd * Wd;                                 // <= 2^24
  float acc[NI];
  int e[NI];
  long g_off[NI];                       // offset of the element's channel plane in grad_out (channel 2 - row)
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    e[i] = min(t + i * FT_BWD_THREADS, E - 1);
    acc[i] = 0.f;
    g_off[i] = (long)(2 - e[i] / n_tex) * n_pix;
  }
  const int p0 = blockIdx.x * per_block, p1 = min(p0 + per_block, n_pix);
  int y = p0 / Wd, x = p0 - y * Wd;
#pragma unroll 8
  for (int p = p0; p < p1; ++p) {
    const float* __restrict__ run = basis + ((long)ft_src(y, scale_y, Hs) * Ws + ft_src(x, scale_x, Ws)) * E;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      float g;
      if constexpr (ONE) {
        g = grad_out[g_off[i] + p];
      } else {
        g = 0.f;
        for (int b = 0; b < n_copies; ++b) g += grad_out[(long)b * 3 * n_pix + g_off[i] + p];
      }
      acc[i] = fmaf(run[e[i]], g, acc[i]);
    }
    if (++x == Wd) { x = 0; ++y; }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i)
    if (t + i * FT_BWD_THREADS < E) sums[t + i * FT_BWD_THREADS] = acc[i];
  __syncthreads();
  if (t < n_tex) workspace[(long)blockIdx.x * n_tex + t] = (sums[t] + sums[n_tex + t]) + sums[2 * n_tex + t];
}

// grad_code[k] = the workspace's column k added in row order: 64 consecutive segments of rows, each added in order by one
// thread, then the 64 segment sums added in order.  One workgroup per 16 columns.
__global__ __launch_bounds__(FT_RED_K * FT_RED_SEG) void flametex_bwd_reduce_kernel(
    const float* __restrict__ workspace, float* __restrict__ grad_code, int n_blocks, int n_tex) {
  __shared__ float part[FT_RED_SEG][FT_RED_K];
  const int kk = threadIdx.x % FT_RED_K, s = threadIdx.x / FT_RED_K, k = blockIdx.x * FT_RED_K + kk;
  const int len = (n_blocks + FT_RED_SEG - 1) / FT_RED_SEG;
  const int b0 = min(s * len, n_blocks), b1 = min(b0 + len, n_blocks);
  float a = 0.f;
  if (k < n_tex)
    for (int b = b0; b < b1; ++b) a += workspace[(long)b * n_tex + k];
  part[s][kk] = a;
  __syncthreads();
  if (s == 0 && k < n_tex) {
    float total = part[0][kk];
    for (int i = 1; i < FT_RED_SEG; ++i) total += part[i][kk];
    grad_code[k] = total;
  }
}

extern "C" long msmd_flametex_backward_workspace(int Hd, int Wd, int n_tex) {
  if (!ft_sizes_ok(1, 1, Hd, Wd, n_tex)) return -1;
  return (long)ft_bwd_blocks(Hd * Wd) * n_tex;
}

extern "C" int msmd_flametex_backward(const float* basis, const float* grad_out, int n_copies, float* grad_code,
                                      float* workspace, int Hs, int Ws, int Hd, int Wd, int n_tex, msmd_stream_t stream) {
  if (!ft_sizes_ok(Hs, Ws, Hd, Wd, n_tex) || n_copies < 0) return (int)hipErrorInvalidValue;
  const float sy = (float)Hs / (float)Hd, sx = (float)Ws / (float)Wd;
  const int n_pix = Hd * Wd, per_block = ft_bwd_pixels_per_block(n_pix), n_blocks = ft_bwd_blocks(n_pix);
  hipStream_t st = (hipStream_t)stream;
  const int ni = (3 * n_tex + FT_BWD_THREADS - 1) / FT_BWD_THREADS;
#define FT_BWD_LAUNCH(NI, ONE)                                                                                                \
  hipLaunchKernelGGL((flametex_bwd_partial_kernel<NI, ONE>), dim3(n_blocks), dim3(FT_BWD_THREADS), 0, st, basis, grad_out,       \
                     n_copies, workspace, Hs, Ws, Hd, Wd, n_tex, sy, sx, per_block)
  if (n_copies == 1) {
    if (ni == 1) FT_BWD_LAUNCH(1, true); else if (ni == 2) FT_BWD_LAUNCH(2, true); else FT_BWD_LAUNCH(3, true);
  } else {
    if (ni == 1) FT_BWD_LAUNCH(1, false); else if (ni == 2) FT_BWD_LAUNCH(2, false); else FT_BWD_LAUNCH(3, false);
  }
#undef FT_BWD_LAUNCH
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(flametex_bwd_reduce_kernel, dim3((n_tex + FT_RED_K - 1) / FT_RED_K), dim3(FT_RED_K * FT_RED_SEG), 0, st,
                     workspace, grad_code, n_blocks, n_tex);
  MSMD_RETURN_LAST();
}
