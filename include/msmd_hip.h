/*
 * msmd_hip.h -- C ABI of libmsmd_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * audio -> motion-coefficient hot path of ubisoft/ubisoft-laforge-msmd.
 *
 * The reference has no FFI/plugin layer: the path sits behind Python nn.Module calls
 * (SURVEY.md section 8b).  Each entry point below replaces the implicit torch/cuDNN/cuBLAS/HF
 * device ops issued by the cited reference lines.  Conventions:
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory owned by the caller;
 *   - no hidden allocation, no host synchronisation (graph-capturable); workspaces are passed in;
 *   - re-entrant per stream; `stream` is a hipStream_t passed as void*;
 *   - returns a hipError_t-compatible int (0 = success); argument errors return hipErrorInvalidValue (1);
 *   - activations are channels-last, row-major (rows, cols); `dtype` selects fp32 (parity mode)
 *     or bf16 storage with fp32 accumulation (speed mode).  Biases / norm affine params / statistics
 *     are always fp32.
 */
#ifndef MSMD_HIP_H
#define MSMD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSMD_F32 0
#define MSMD_BF16 1
#define MSMD_F16 2 /* IEEE half storage, fp32 accumulate: inference kernels (GEMM, attention, norm, audio, diffusion) */
/* "split pair" storage of fp32-grade values for the parity-grade speed mode (inference kernels): x ~= hi + lo * 2^-11
 * with hi = RN_f16(x), lo = RN_f16((x - hi) * 2^11), |err| <= 2^-22 |x| + 2^-35 (typically 2^-24 |x|) for |x| < 65504.  A logical row of C values
 * (C % 32 == 0) is stored as 2 C fp16 numbers in 32-element blocks [hi x 32 | lo x 32]; all sizes / leading
 * dimensions / strides in this header stay in LOGICAL elements.  Contractions run as three f16 MFMAs per k-step
 * (hi.hi, hi.lo, lo.hi; fp32 accumulate), i.e. at 1/3 of the f16 MFMA rate instead of the 1/16 of the exact-fp32
 * MFMA.  The reference computes in fp32 everywhere (training_script.py:548-551: no autocast); this is the mode that
 * meets its 1e-4 tolerance at speed. */
#define MSMD_F16X2 3

#define MSMD_ACT_NONE 0
#define MSMD_ACT_GELU 1 /* exact erf GELU */
#define MSMD_ACT_ELU 2  /* alpha = 1 */

typedef void* msmd_stream_t; /* hipStream_t */

/* Library / device probe: returns the ABI version; safe to call without a GPU. */
int msmd_abi_version(void);
/* The library keeps NO process-global state: every entry point is re-entrant per stream.  What used to be developer
 * knobs travels per call -- the GEMM kernel variant and epilogue flags in `act` (msmd_gemm below), the contraction
 * split count of msmd_gemm_tn in its `accumulate` argument.  The kernel families of DESIGN.md section 5 / 5b that
 * lost their measurements are not in the sources any more. */
#define MSMD_GEMM_VARIANT(v) ((v) << 8)   /* bits 8-15 of `act`: 0 = shape heuristic, 9 / 12 / 13 / 14 / 15 / 17 / 18 / 80 (bf16, fp16), 1 / 5 / 14 / 80 (f16x2) */
#define MSMD_GEMM_WRITE_THROUGH (1 << 16) /* output stores carry `sc1`: the bytes leave the XCD's L2 as they are stored */
#define MSMD_GEMM_PAIRED_STORES (1 << 17) /* 16-bit outputs: lane pairs swap a fragment row, one 16-byte store each */
#define MSMD_GEMM_STAGGER (1 << 18)       /* multi-round launches: the second workgroup of every CU starts half a tile period late */
#define MSMD_GEMM_ONE_TILE_PER_WORKGROUP (1 << 19) /* opt out of the persistent form of multi-round launches (A/B; same bits) */
#define MSMD_GEMM_NO_256_TILE (1 << 20)   /* opt out of the 256 x 256 8-phase kernel (variant 80) where the heuristic would pick it (A/B) */
#define MSMD_GEMM_W_BELOW_32 (1 << 21)    /* MSMD_F16X2 operands: the caller states |W| < 32 everywhere (model weights).  The 256 x 256
                                             kernel (variant 80) may then scale W's hi plane by 2^11 in registers and keep ONE sum in
                                             units of 2^-11 instead of folding the cross terms once per K tile (11-17 % faster).  Without
                                             the bit nothing is assumed about W.  A W element of 32 or more under this bit overflows fp16. */
#define MSMD_GEMM_NO_160_ROW_TILE (1 << 22)    /* msmd_gemm_ln: opt out of the 160 x 128 member of variant 17 where the library would launch it (A/B; same bits) */
#define MSMD_GEMM_FORCE_160_ROW_TILE (1 << 23) /* msmd_gemm_ln: launch the 160 x 128 member of variant 17 wherever the kernel takes the call (residual form, no
                                                  activation, 64-column slabs, variant 17 by hint or by the library's choice); ignored elsewhere (tests, scans) */

/* Measurement aid: one wavefront that spins for `us` microseconds of the 100 MHz constant clock (s_memrealtime) and
 * optionally stores the ticks it actually spun.  bench.py times it at two lengths to calibrate the overhead of a HIP
 * event pair around ONE launch, so that its per-launch roofline figures agree with rocprofv3 --kernel-trace. */
int msmd_spin_us(float us, long* ticks_out, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dense contraction on MFMA:  C = act(A . W^T + bias) + residual
 *   A: (M, K) activations, row m at  A + (m / rows_per_batch) * a_batch_stride + (m % rows_per_batch) * lda
 *      (elements).  With rows_per_batch = T_out, lda = stride*C_in, a_batch_stride = T_in*C_in and
 *      K = k*C_in this IS a strided Conv1d over a channels-last signal with no im2col buffer.
 *   W: (N, K) row-major, leading dimension ldw (torch Linear layout; conv weights repacked (N, k*C_in)).
 *   bias: fp32 (N) or NULL.  residual: (M, N) ld ldr or NULL.  C: (M, N) ld ldc.
 *   in_dtype: dtype of A and W.  out_dtype: dtype of C and residual.
 *   in_dtype MSMD_F16X2 (split storage, the parity-grade speed mode): three f16 MFMAs per k-step, fp32-grade result;
 *   out_dtype MSMD_F32 or MSMD_F16X2; K, lda, ldw, a_batch_stride and the A / W strides must be multiples of 32, and
 *   for split output also N % 4 == 0 and ldc / ldr / strideC / strideR multiples of 32.
 *   batch > 1 launches independent problems with the given element strides (grouped conv).
 *   act: MSMD_ACT_* in bits 0-7; bits 8-15 may carry a kernel-variant hint (MSMD_GEMM_VARIANT; 0 = the library's own
 *   shape heuristic; every variant computes bit-identical results -- up to one fused multiply-add's rounding
 *   where an activation meets a residual, see tests/test_kernels_gpu.py); bits 16-23 epilogue flags (MSMD_GEMM_WRITE_THROUGH,
 *   MSMD_GEMM_PAIRED_STORES: how the output is stored, never what is stored).
 *   Requirements: K % (16 / sizeof(in)) == 0, lda/ldw/a_batch_stride/strideA/strideW multiples of the same.
 * Replaces: nn.Linear / nn.Conv1d / nn.MultiheadAttention projections at reference model.py:115,856-906,
 *   style_encoder.py:135-175, utils/wav2vec2.py:79,95,111 (HF conv stack, projection, pos-conv, encoder FFN).
 */
int msmd_gemm(const void* A, const void* W, const float* bias, const void* residual, void* C,
              int M, int N, int K, int in_dtype, int out_dtype,
              long lda, int rows_per_batch, long a_batch_stride, long ldw, long ldc, long ldr, int act,
              int batch, long strideA, long strideW, long strideC, long strideBias, long strideR,
              msmd_stream_t stream);

/* msmd_gemm with the training epilogue:  C = dropout_p(act(A . W^T + bias)) + residual, and optionally
 * z_out = A . W^T + bias (the pre-activation the backward needs; layout and dtype of C).  The keep mask is
 * Philox4x32-10(rng_state[seed, step], site, (m * N + n) / 4) -- exactly msmd_dropout's mask on a contiguous (M, N)
 * tensor, so msmd_dropout / msmd_act_bwd_dropout regenerate it in the backward.  p_drop > 0 requires N % 4 == 0,
 * ldc == N, batch == 1.  Replaces nn.Linear -> activation -> nn.Dropout (-> residual add) chains of the HF encoder
 * layers, nn.TransformerDecoderLayer / EncoderLayer and the style encoder in train() mode. */
/* LayerNorm folded into the GEMMs around it (post-LN / pre-LN transformer blocks without LayerNorm launches and without
 * materialising the normalised rows; 16-bit operands and output of one dtype, K % 64 == 0, N % 64 == 0, no batch).
 *   C = act(LN_A(A) . W^T + bias) + LN_R(residual)       bias required; two forms, anything else returns 1:
 *     operand form:  a_stats + w_colsum, no residual, no stats_out;
 *     residual form: residual required, r_stats (+ r_gamma, r_beta) and stats_out each optional.
 *   Row statistics travel as per-row partial (sum, sum of squares) over column slabs, fp32, slab-major: (cols / slab, rows, 2).  The slab
 *   is what one wave of the producing kernel holds of a row: slab_out = 64 selects the 128 x 128 tile (N % 128 == 0),
 *   slab_out = 32 the 64 x 64 tile (for grids that would not fill the chip otherwise); slab_in is the slab the producer
 *   of a_stats / r_stats used.
 *   a_stats (K / slab_in, M, 2) + w_colsum (N): A holds UN-normalised rows u; W must carry the LayerNorm weight folded in
 *     (W'[n][k] = gamma[k] W[n][k]), w_colsum[n] = sum_k W'[n][k] (of the ROUNDED W'), bias[n] = b[n] + sum_k beta[k] W[n][k]:
 *     the epilogue applies  rstd (acc - mu w_colsum[n]) + bias[n].
 *   r_stats (N / slab_in, M, 2) + r_gamma / r_beta (N): the residual operand holds un-normalised rows; LN is applied on the fly.
 *   stats_out (N / slab_out, M, 2): statistics of the stored (rounded) rows of C.
 * Replaces the LayerNorm modules between the Linear layers of HF Wav2Vec2EncoderLayer / HubertEncoderLayer(StableLayerNorm)
 *  and nn.TransformerDecoderLayer (reference model.py:874-878): the sequence Linear -> +residual -> LayerNorm ->
 * Linear becomes two launches. */
int msmd_gemm_ln(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K,
                 int in_dtype, int out_dtype, long lda, long ldw, long ldc, long ldr, int act, const float* a_stats,
                 const float* w_colsum, const float* r_stats, const float* r_gamma, const float* r_beta,
                 float* stats_out, int slab_in, int slab_out, float eps, msmd_stream_t stream);

int msmd_gemm_ex(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K,
                 int in_dtype, int out_dtype, long lda, int rows_per_batch, long a_batch_stride, long ldw, long ldc,
                 long ldr, int act, int batch, long strideA, long strideW, long strideC, long strideBias, long strideR,
                 void* z_out, float p_drop, const unsigned long* rng_state, unsigned int site, msmd_stream_t stream);

/* Which kernel a call would run: each query takes exactly the arguments of the call it mirrors (msmd_gemm_route those of
 * msmd_gemm_ex; a msmd_gemm call is the same with z_out = NULL, p_drop = 0) and returns the MSMD_GEMM_VARIANT number the library
 * would launch for them -- its own choice or the hint, 80 = the 256 x 256-tile kernel --, 0 for the generic kernel (operands
 * the tiled kernels do not take, or a hint that names no variant of the operand type), -1 for a call the library rejects
 * (where the call itself returns 1).  Pure host functions of their arguments: nothing is launched or dereferenced, no HIP call
 * is made (they run without a GPU) and no state is kept.  They run the plan code of the calls themselves, so a caller that
 * times launches (bench.py's roofline leg) files each one under the kernel that ran it.  No counterpart in the reference. */
int msmd_gemm_route(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K,
                    int in_dtype, int out_dtype, long lda, int rows_per_batch, long a_batch_stride, long ldw, long ldc,
                    long ldr, int act, int batch, long strideA, long strideW, long strideC, long strideBias, long strideR,
                    void* z_out, float p_drop, const unsigned long* rng_state, unsigned int site, msmd_stream_t stream);
int msmd_gemm_ln_route(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K,
                       int in_dtype, int out_dtype, long lda, long ldw, long ldc, long ldr, int act, const float* a_stats,
                       const float* w_colsum, const float* r_stats, const float* r_gamma, const float* r_beta,
                       float* stats_out, int slab_in, int slab_out, float eps, msmd_stream_t stream);
/* The rows of C one workgroup of that launch computes: 64 (variants 9 / 12 / 18), 128 (17 / 66), 160 (17's member for grids that 160-row
 * tiles put into ONE round of one workgroup per CU: the encoder's out-projection and FFN-2 at 6400 rows), 192 (15) or 256 (80); -1 for
 * a call msmd_gemm_ln rejects.  The variant number does not change with the member: every tile of the family stores the same bits.
 * Same arguments and the same guarantees as msmd_gemm_ln_route. */
int msmd_gemm_ln_rows(const void* A, const void* W, const float* bias, const void* residual, void* C, int M, int N, int K,
                      int in_dtype, int out_dtype, long lda, long ldw, long ldc, long ldr, int act, const float* a_stats,
                      const float* w_colsum, const float* r_stats, const float* r_gamma, const float* r_beta,
                      float* stats_out, int slab_in, int slab_out, float eps, msmd_stream_t stream);

/* A stack of 2 to 4 strided Conv1d layers (+ bias + activation) over a channels-last 16-bit signal as ONE launch of the 256 x 256
 * kernel (variant 80's K loop and epilogue): layer l is the windowed GEMM msmd_gemm would run for it -- M = B * T_l rows, N outputs,
 * K = kernel[l] * channels in -- and reads layer l - 1's output while other workgroups are still writing later rows of it.  Tiles
 * are handed out by one ticket counter, layer after layer and row block after row block, so a tile only ever waits for tiles with
 * a lower ticket; row-block counters say when a tile's input rows are complete.  Every layer's output holds the
 * bits msmd_gemm stores for the same layer.
 *   x (B, T0, C); layer l: w[l] (N, kernel[l] * C_l) with C_0 = C, C_l = N; bias[l] fp32 (N) or NULL; out[l] (B, T_l, N),
 *   T_l = (T_{l-1} - kernel[l]) / stride[l] + 1.  w / bias / out / kernel / stride are HOST arrays of n_layers entries (the only
 *   host pointers of this header); what they point to is device memory.  act: MSMD_ACT_NONE or MSMD_ACT_GELU, every layer's.
 *   workspace: msmd_conv_chain_workspace() bytes of device memory, 16-byte aligned, zeroed by a launch this call puts on the
 *   stream ahead of the kernel.  max_workgroups: 0 = one workgroup per CU, else a smaller grid (tests).
 *   flags: MSMD_CONV_CHAIN_RELEASE = rows that a later layer reads are stored plainly and published by one agent-scope release
 *   per tile, instead of write-through stores; MSMD_CONV_CHAIN_ROW_BLOCK_TICKETS = a ticket is a row block with all its column
 *   tiles, instead of one tile.  Neither changes what is stored.
 * Returns 1, having launched nothing, for what the kernel does not take: N % 256 != 0, a K % 64 != 0 or K < 128, a dtype other
 * than MSMD_BF16 / MSMD_F16, operand offsets past 4 GB, fewer than 2 or more than 4 layers, 2^24 rows or more in a layer; the
 * caller then runs the layers as msmd_gemm calls.
 * msmd_conv_chain_plan: the kernel's own ticket arithmetic on the host (no HIP call): out6 = (layer, row block, first column tile,
 *   column tiles, first and last row block of layer - 1 that must be complete; the last two 0, -1 for layer 0); returns 0, the
 *   ticket count for a ticket past the last one, -1 for shapes the kernel does not take.
 * msmd_conv_chain_status: a BLOCKING read of the launch's status word, 0 or MSMD_CONV_CHAIN_TIMEOUT (a wait for a producer took
 *   longer than 20 ms of wall clock: the workgroup stopped taking tickets and returned); -1 where the copy failed.  For tests
 *   and tools, never on a timed path.
 * Replaces conv_layers[1..4] of HF Wav2Vec2FeatureEncoder (reference utils/wav2vec2.py:79, the nn.Conv1d + GELU modules). */
#define MSMD_CONV_CHAIN_RELEASE 1
#define MSMD_CONV_CHAIN_ROW_BLOCK_TICKETS 2
#define MSMD_CONV_CHAIN_TIMEOUT 1
int msmd_conv_chain(const void* x, int B, int T0, int C, int N, int n_layers, const void* const* w, const float* const* bias,
                    void* const* out, const int* kernel, const int* stride, int act, int dtype, void* workspace,
                    long workspace_bytes, int max_workgroups, int flags, msmd_stream_t stream);
long msmd_conv_chain_workspace(int B, int T0, int C, int N, int n_layers, const int* kernel, const int* stride);
int msmd_conv_chain_plan(int B, int T0, int C, int N, int n_layers, const int* kernel, const int* stride, int flags, int ticket,
                         int* out6);
int msmd_conv_chain_status(const void* workspace);

/* Two-level batched GEMM C[zo][zi] = A[zo][zi] . W[zo][zi]^T (no bias / residual / activation): operand z =
 * zo * batch_inner + zi starts at base + zo * stride_o + zi * stride_i.  Used by the explicit (materialised-P)
 * training attention, where zo = batch and zi = head index into packed (B, T, H*64) tensors. */
/* dZ = keep_mask / (1 - p_drop) * act'(Z) * (A . W^T)  (16-bit; C and Z contiguous (M, N), N % 4 == 0): the data gradient of a
 * Linear whose input was dropout(act(Z)), with the backward of that activation + dropout applied in the GEMM epilogue (mask
 * regenerated from (rng_state, site) as by msmd_gemm_ex / msmd_act_bwd_dropout; p_drop = 0: no mask).  One launch for
 * autograd's  linear2.backward -> dropout.backward -> GELU.backward  of nn.TransformerEncoder/DecoderLayer and the HF
 * feed-forward blocks (reference model.py:874-878, utils/wav2vec2.py). */
int msmd_gemm_actbwd(const void* A, const void* W, const void* Z, void* C, int M, int N, int K, int in_dtype, int out_dtype,
                     long lda, long ldw, int act, float p_drop, const unsigned long* rng_state, unsigned int site,
                     msmd_stream_t stream);

int msmd_gemm_batched2(const void* A, const void* W, void* C, int M, int N, int K, int in_dtype, int out_dtype,
                       long lda, long ldw, long ldc, int batch_outer, long strideA_o, long strideW_o, long strideC_o,
                       int batch_inner, long strideA_i, long strideW_i, long strideC_i, msmd_stream_t stream);

/* Weight-gradient GEMM: C (N, K) fp32 = A^T . B with A (M, N) bf16 and B (M, K) bf16, both row-major with the
 * contraction index as the slow axis (A = dZ, B = X of a Linear's backward: no transposed copies).  N, K, lda, ldb
 * multiples of 8; pointers 16-byte aligned.  colsum (N) fp32 or NULL: fused bias gradient sum_m A[m][n]
 * (batch must be 1).  B may be a windowed view (row r at (r / b_rows_per_window) * b_window_stride +
 * (r % b_rows_per_window) * ldb; 0 = plain) so a Conv1d weight gradient needs no unfolded copy.
 * C / colsum are fully overwritten, or added to when bit 0 of `accumulate` is set (gradient accumulation in place);
 * bits 8-15 of `accumulate` force the contraction split count (0 = chosen from the shape).  ws / ws_bytes: optional device workspace for
 * split-contraction partial products (msmd_gemm_tn_workspace() bytes fill the chip; NULL = unsplit).  Replaces what autograd computes for nn.Linear in the
 * reference's loss.backward() (training_script.py:196). */
int msmd_gemm_tn(const void* A, const void* B, float* C, float* colsum, int M, int N, int K, long lda, long ldb,
                 long ldc, int batch, long strideA, long strideB, long strideC, int b_rows_per_window,
                 long b_window_stride, int accumulate, void* ws, long ws_bytes, msmd_stream_t stream);
long msmd_gemm_tn_workspace(int M, int N, int K, int batch);

/* ------------------------------------------------------------------------------------------------
 * y = post_act(LayerNorm(act(x + residual)) * gamma + beta) + post_add      (row-wise over `cols`)
 *   `act` carries the pre-activation in its low byte and post_act in bits 8-15 (MSMD_ACT_* codes; the LayerNorm ->
 *   GELU of HF's layer-norm conv stack).  residual, post_add (fp32, cols) may be NULL.  eps as torch (1e-5).
 *   Biased variance.
 * Replaces: nn.LayerNorm at reference style_encoder.py:142,150,170; HF feature_projection.layer_norm,
 *   encoder.layer_norm, layers.N.{layer_norm,final_layer_norm}; decoder norm1-3 (model.py:874-878).
 */
int msmd_layernorm(const void* x, const void* residual, const float* gamma, const float* beta,
                   const float* post_add, void* y, int rows, int cols, float eps, int act,
                   int in_dtype, int out_dtype, msmd_stream_t stream);
/* y = LN_{gamma, beta}( LN_{pre_gamma, pre_beta}(x) + residual ), 16-bit rows: two consecutive post-LN LayerNorms with a branch
 * added in between (nn.TransformerDecoderLayer norm1 -> + cross-attention branch -> norm2, reference model.py:874-878) in one
 * launch; the inner result is rounded to the storage type as the separate launch would have stored it. */
int msmd_layernorm_pre(const void* x, const float* pre_gamma, const float* pre_beta, const void* residual,
                       const float* gamma, const float* beta, void* y, int rows, int cols, float eps, int dtype,
                       msmd_stream_t stream);

/* msmd_layernorm on fp32 input with the row ALSO written in MSMD_F16X2 split storage (y_split; cols % 32 == 0):
 * in the parity-grade speed mode a LayerNorm output is the next contraction's A operand (split) and the residual of
 * the block after it (fp32, y; may be NULL when no fp32 copy is needed).  Same reference lines as msmd_layernorm. */
int msmd_layernorm_f16x2(const float* x, const float* residual, const float* gamma, const float* beta,
                         const float* post_add, float* y, void* y_split, int rows, int cols, float eps, int act,
                         msmd_stream_t stream);

/* fp32 (rows, cols) with leading dimension ldx -> MSMD_F16X2 split rows of cols_out >= cols logical columns
 * (cols_out % 32 == 0; the padding columns are zero), and back.  Streaming conversions for tensors that enter the
 * parity-grade speed mode from fp32 producers (weights at pack time, small glue tensors); the hot producers
 * (msmd_layernorm_f16x2, msmd_gemm with out_dtype MSMD_F16X2, msmd_conv0_gn_gelu) write split rows themselves. */
int msmd_split_f16x2(const float* x, void* y, long rows, int cols, long ldx, int cols_out, msmd_stream_t stream);
int msmd_unsplit_f16x2(const void* x, float* y, long rows, int cols, int cols_in, long ldy, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused softmax attention for short sequences (Tk <= 512), head_dim 64:
 *   O[b, t, h*64:(h+1)*64] = softmax(scale * Q_h K_h^T  (masked -> -inf)) V_h
 *   Q/K/V/O rows are addressed as base + b*bstride + t*tstride + h*64 (elements).
 *   mask: (Tq, Tk) bytes, nonzero = masked out, or NULL.
 * Replaces: HF Wav2Vec2Attention (called from utils/wav2vec2.py:111), nn.MultiheadAttention inside
 *   nn.TransformerDecoderLayer (model.py:874-878,956) and nn.TransformerEncoderLayer (style_encoder.py:158).
 */
/* msmd_attention that additionally READS up to four byte ranges (16-byte aligned; e.g. the weight matrices of the GEMMs that
 * follow in the layer) and drops the data: the ranges are in the memory-side cache when those kernels start.  On MI355X a
 * GEMM whose operands come from HBM instead of the 256 MB Infinity Cache runs 20 % slower (6400 x 768 x 3072: 51 vs 43 us),
 * and one forward step streams ~1.5 GB through that cache between two uses of a weight.  Host arrays, read at launch. */
int msmd_attention_prefetch(const void* Q, const void* K, const void* V, void* O, int B, int H, int Tq, int Tk,
                            long q_bstride, long q_tstride, long k_bstride, long k_tstride, long v_bstride,
                            long v_tstride, long o_bstride, long o_tstride, float scale, const uint8_t* mask, int dtype,
                            const void* const* prefetch_ptrs, const long* prefetch_bytes, int n_prefetch,
                            msmd_stream_t stream);
int msmd_attention(const void* Q, const void* K, const void* V, void* O, int B, int H, int Tq, int Tk,
                   long q_bstride, long q_tstride, long k_bstride, long k_tstride, long v_bstride,
                   long v_tstride, long o_bstride, long o_tstride, float scale, const uint8_t* mask,
                   int dtype, msmd_stream_t stream);

/* msmd_attention on MSMD_F16X2 split operands (the parity-grade speed mode): Q / K / V as written by msmd_gemm with
 * out_dtype MSMD_F16X2, both products as three f16 MFMAs per k-step, softmax in fp32 (expf); O in fp32 or in split
 * storage (out_dtype) for the out-projection GEMM.  Strides in logical elements, multiples of 32. */
int msmd_attention_f16x2(const void* Q, const void* K, const void* V, void* O, int B, int H, int Tq, int Tk,
                         long q_bstride, long q_tstride, long k_bstride, long k_tstride, long v_bstride,
                         long v_tstride, long o_bstride, long o_tstride, float scale, const uint8_t* mask,
                         int out_dtype, msmd_stream_t stream);


/* Person-token cross-attention query, projection + Tq = 1 attention fused (one wave per sequence and head):
 *   out[n, h*64:(h+1)*64] = softmax(scale * (x[n] Wq_h^T + bq_h) K_h[n]^T) V_h[n]     (no mask, head_dim 64, Tk <= 512)
 * x row n at x + n*x_seq_stride (d elements); Wq (d, d) row-major; K/V rows at base + n*kv_bstride + t*kv_tstride + h*64;
 * out (N, d) contiguous; all of `dtype` (fp32 accumulation throughout).
 * Replaces, for row 0 of the sequence (the person / diffusion-step token) under the diagonal alignment mask: the
 * q-projection and softmax of nn.MultiheadAttention in the reference's TransformerDecoderLayer (model.py:874-878,956). */
int msmd_person_query_attention(const void* x, long x_seq_stride, const void* Wq, const float* bq, const void* K,
                                const void* V, long kv_bstride, long kv_tstride, void* out, int N, int H, int Tk, int d,
                                float scale, int dtype, msmd_stream_t stream);
/* msmd_person_query_attention with the LayerNorm in front of the query projection folded in (the decoder's norm1 in the
 * sampler's diagonal path): x row 0 is un-normalised, Wq / bq are the gamma / beta folded operands (as for msmd_gemm_ln's
 * operand form), wq_colsum[r] = sum_k Wq'[r][k]; mean / rstd of the row are computed in the kernel. */
int msmd_person_query_attention_ln(const void* x, long x_seq_stride, const void* Wq, const float* bq,
                                   const float* wq_colsum, float ln_eps, const void* K, const void* V, long kv_bstride,
                                   long kv_tstride, void* out, int N, int H, int Tk, int d, float scale, int dtype,
                                   msmd_stream_t stream);

/* Training-mode attention forward: as msmd_attention with attention-probability dropout p_drop (HF
 * attention_dropout, nn.MultiheadAttention(dropout=0.1) inside the decoder / encoder layers).  The keep mask is
 * Philox4x32-10(seed = rng_state[0], step = rng_state[1], site, counter = ((b H + h) Tq + q) * 128 + 4 * (key / 32) + (key / 4) % 4):
 * one block = the 16-bit draws of the 8 keys {16 f + 4 fq + e, f in a fragment pair} (even fragment: low halves of the 4 words, odd:
 * high halves); keep <=> draw >= floor(65536 p).  msmd_attention_bwd regenerates the same mask.  rng_state is DEVICE memory so a
 * captured hipGraph draws fresh masks on every replay once the host side advances the step.  Tk <= 512. */
int msmd_attention_dropout(const void* Q, const void* K, const void* V, void* O, int B, int H, int Tq, int Tk,
                           long q_bstride, long q_tstride, long k_bstride, long k_tstride, long v_bstride,
                           long v_tstride, long o_bstride, long o_tstride, float scale, const uint8_t* mask,
                           float p_drop, const unsigned long* rng_state, unsigned int site, int dtype,
                           msmd_stream_t stream);
/* msmd_attention_dropout with msmd_attention_prefetch's byte ranges. */
int msmd_attention_dropout_prefetch(const void* Q, const void* K, const void* V, void* O, int B, int H, int Tq, int Tk,
                                    long q_bstride, long q_tstride, long k_bstride, long k_tstride, long v_bstride,
                                    long v_tstride, long o_bstride, long o_tstride, float scale, const uint8_t* mask,
                                    float p_drop, const unsigned long* rng_state, unsigned int site, int dtype,
                                    const void* const* prefetch_ptrs, const long* prefetch_bytes, int n_prefetch,
                                    msmd_stream_t stream);

/* y = x * keep / (1 - p) (+ residual): nn.Dropout in training mode (HF hidden / activation / feat_proj dropout,
 * decoder-layer dropout1-3, PositionalEncoding dropout, style-encoder dropouts; utils/model_common.py:101,
 * style_encoder.py:139-167).  Same Philox stream as above indexed by element / 4; calling it on dy with the same
 * (rng_state, site) is the backward. */
int msmd_dropout(const void* x, const void* residual, void* y, long n, float p, const unsigned long* rng_state,
                 unsigned int site, int dtype, msmd_stream_t stream);

/* Fused attention backward (bf16, head_dim 64, Tk <= 256): recomputes P per 64-row query tile and writes
 * dQ / dK / dV; P, dP and transposed operands never touch HBM.  Same addressing convention as msmd_attention
 * (base + b*bstride + t*tstride + h*64; strides multiples of 8 elements, bases 16-byte aligned); dQ / dK / dV may
 * be slices of one packed gradient buffer.  Replaces autograd of the attention modules listed above under the
 * reference's loss.backward() (training_script.py:196).  p_drop / rng_state / site: attention-probability dropout
 * exactly as the forward msmd_attention_dropout drew it (0 / NULL: none). */
int msmd_attention_bwd(const void* Q, const void* K, const void* V, const void* dO, void* dQ, void* dK, void* dV,
                       int B, int H, int Tq, int Tk, long q_bstride, long q_tstride, long k_bstride,
                       long k_tstride, long v_bstride, long v_tstride, long do_bstride, long do_tstride,
                       long dq_bstride, long dq_tstride, long dk_bstride, long dk_tstride, long dv_bstride,
                       long dv_tstride, float scale, const uint8_t* mask, float p_drop,
                       const unsigned long* rng_state, unsigned int site, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Audio front end.  pad plan = (reflect_len applied twice per side, replicate_len 0/1), computed on
 * the host exactly as reference utils/model_common.py:110-123.
 */
/* out (B, L + 4*reflect_len + 2*replicate_len) fp32 = pad_audio(audio (B, L)). */
int msmd_pad_audio(const float* audio, float* out, int B, int L, int reflect_len, int replicate_len,
                   msmd_stream_t stream);

/* conv0 (1->C, k=10, s=5, no bias) statistics for GroupNorm(C groups): stats (B, C, 2) = {mean, rstd}
 * over the T0 = (Lp - 10)/5 + 1 output frames, reading the UNPADDED audio through the pad map.
 * w0: (C, 10) fp32.  Replaces HF Wav2Vec2GroupNormConvLayer (called at utils/wav2vec2.py:79). */
#define MSMD_CONV0_SPLITS 16 /* ws: (B, MSMD_CONV0_SPLITS, 66) fp64 partial signal moments (shift, S[10], R[55]); at least
                              * B*16*66 doubles.  The conv response is linear in the signal, so per-channel mean / variance
                              * follow from these 66 numbers per clip. */
/* Returns 1 (nothing launched) for reflect_len < 0, replicate_len < 0, reflect_len >= L or no output frame, as
 * msmd_pad_audio does; so do msmd_conv0_gn_gelu and msmd_conv0_ln_gelu. */
int msmd_conv0_stats(const float* audio, const float* w0, float* stats, double* ws, int B, int L, int reflect_len,
                     int replicate_len, int C, float eps, msmd_stream_t stream);

/* out (B, T0, C) = GELU(GroupNorm(conv0(pad(audio)))) with the statistics above. */
int msmd_conv0_gn_gelu(const float* audio, const float* w0, const float* stats, const float* gamma,
                       const float* beta, void* out, int B, int L, int reflect_len, int replicate_len,
                       int C, int out_dtype, msmd_stream_t stream);

/* conv0 of the feat_extract_norm="layer" stack (hubert-large-style configs; HF HubertLayerNormConvLayer, reached from
 * utils/hubert.py:22 `self.feature_extractor(input_values)`): out[b][t][:] = GELU(LayerNorm_c(bias + conv1d(k=10,
 * s=5)(pad_audio(x)))) channels-last, C = 512, pad_audio fused into the loads as above. */
int msmd_conv0_ln_gelu(const float* audio, const float* w0, const float* bias, const float* gamma, const float* beta,
                       void* out, int B, int L, int reflect_len, int replicate_len, int C, float eps, int out_dtype,
                       msmd_stream_t stream);

/* Linear resample along time of a channels-last tensor with F.interpolate(mode='linear',
 * align_corners=False) semantics: y (B, T_out, C) from the first T_crop frames of x (B, T_in, C).
 * Replaces utils/wav2vec2.py:57-63,82-84 and model.py:260. */
int msmd_interp_linear(const void* x, void* y, int B, int T_in, int T_crop, int T_out, int C, int dtype,
                       msmd_stream_t stream);

/* Regroup (B, T, G*Cg) channels-last into the zero-padded group-major layout (B, G, T + 2*pad, Cg_out >= Cg; the
 * extra channels are zero) the positional grouped conv reads as G windowed GEMMs.  out_dtype = dtype, or MSMD_F16X2
 * from fp32 input (Cg_out % 32 == 0: split storage keeps 32-element blocks whole, so 48 channels are padded to 64). */
int msmd_group_pad(const void* x, void* y, int B, int T, int G, int Cg, int Cg_out, int pad, int dtype, int out_dtype,
                   msmd_stream_t stream);

/* The encoders' grouped positional conv in the 16-bit modes, in ONE launch and without the regrouped copy:
 *   y (B, T, G*Cg) = x + GELU(conv1d_groups=G(x, k = kpos, pad = kpos / 2)[:, :T] + bias)
 * x channels-last, read in place (y must not alias it); w (G, Cg, kpos*Cg) with K index = tap*Cg + channel (the packed
 * weight of the windowed-GEMM form); bias (G*Cg) fp32.  dtype MSMD_BF16 / MSMD_F16, Cg 48 or 64, kpos 128; anything else
 * returns 1 and belongs on msmd_group_pad + msmd_gemm.  Each workgroup keeps its <= 256 frames and their halo in LDS and
 * streams only w.  Bit-identical to msmd_group_pad + msmd_gemm(act = GELU, residual = x) on the same tensors. */
int msmd_pos_conv(const void* x, const void* w, const float* bias, void* y, int B, int T, int G, int Cg, int kpos,
                  int dtype, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Denoiser glue (reference model.py:931-951, 961-996, 231-236, 404-432).
 */
/* feats (N, 1+Lp+L, Kpad): row 0 is left to the caller (person token); rows 1.. = [prev_motion ; motion]
 * (dm cols) ++ indicator col (0 for prev rows) ++ zero pad up to Kpad.  motion: (N, L, dm), prev: (N, Lp, dm),
 * indicator (N, L) fp32 or NULL.  x_t = c0[n]*motion + c1[n]*eps when eps != NULL (q-sample, model.py:231-236). */
int msmd_denoiser_pack_input(const float* motion, const float* eps, const float* c0, const float* c1,
                             const float* prev_motion, const float* indicator, void* feats, int N, int L,
                             int Lp, int dm, int Kpad, int motion_batch, int out_dtype, msmd_stream_t stream);

/* msmd_denoiser_pack_input with keyframe in-painting of the denoiser input (model.py:762-767): where guide_mask[nm, t] != 0
 * (nm = n % motion_batch) the motion columns of frame t are guide_values[nm, t, :] instead of motion[nm, t, :]; everything
 * else is msmd_denoiser_pack_input's arithmetic.  guide_mask (motion_batch, L) uint8, guide_values (motion_batch, L, dm)
 * fp32: dense, so a captured launch does not depend on which frames are pinned.  guide_mask == NULL is the plain call;
 * eps != NULL together with a mask returns 1 (the q-sample form is the training path). */
int msmd_denoiser_pack_input_guided(const float* motion, const float* eps, const float* c0, const float* c1,
                                    const float* prev_motion, const float* indicator, const unsigned char* guide_mask,
                                    const float* guide_values, void* feats, int N, int L, int Lp, int dm, int Kpad,
                                    int motion_batch, int out_dtype, msmd_stream_t stream);

/* Everything the eval forward of the denoiser lays out before its first GEMM, in ONE launch (16-bit storage types only:
 * dtype MSMD_BF16 / MSMD_F16, anything else returns 1).  The caller allocates every output; all are written in whole
 * 16-byte units, so Kpad, d, kp_person and mem_stride are multiples of 8 and the 16-bit buffers 16-byte aligned.
 *   feats (N, 1+Lp+L, Kpad)  exactly msmd_denoiser_pack_input's (motion_batch = N), with c0 = t0[ts[n]], c1 = t1[ts[n]] read
 *                            inside from the two fp32 schedule tables (n_steps rows) and the device int64 ts (N); eps NULL =
 *                            no q-sample (t0 / t1 unused); indicator NULL = no indicator column.  prev_motion_stride =
 *                            elements between two sequences' (Lp, dm) blocks, 0 = one block for all.
 *   pf (N, kp_person)        [person_a (N, cols_a) | person_b (N, cols_b) or NULL | zeros]: msmd_pad_cols' conversion.
 *   style_out (style_n)      style (style_n fp32 values, flat) in the storage type: msmd_cast's conversion; style NULL
 *                            with style_n = 0 = no style.
 *   emb (N, d)               row ts[n] of emb_table (n_steps, d), storage type.
 *   mem[n, :Lpa, :]          prev_audio (fp32; prev_audio_stride elements between sequences, 0 = one block for all) into
 *                            the first Lpa rows of each sequence of mem (row length d, mem_stride elements per sequence).
 * A ts entry outside [0, n_steps) reads the nearest end of the tables. */
int msmd_denoiser_prepare(const float* motion, const float* eps, const float* t0, const float* t1, const long* ts,
                          int n_steps, const float* prev_motion, long prev_motion_stride, const float* indicator,
                          void* feats, int N, int L, int Lp, int dm, int Kpad, const float* person_a, int cols_a,
                          const float* person_b, int cols_b, void* pf, int kp_person, const float* style,
                          long style_n, void* style_out, const void* emb_table, void* emb, int d,
                          const float* prev_audio, long prev_audio_stride, int Lpa, void* mem, long mem_stride,
                          int dtype, msmd_stream_t stream);

/* x (N, T, d) += pe (T, d) (learned PE, model.py:949); row 0 is REPLACED by tok0[n] + row0_add + pe[0]
 * (tok0 (N, d) = person projection (+ step embedding); row0_add (d) optional shared step embedding). */
int msmd_add_pe_token(void* x, const float* pe, const void* tok0, const void* row0_add, int N, int T, int d,
                      int dtype, msmd_stream_t stream);

/* out (N, L, dm) fp32 = dyn[:, :, :dm] + sum_b alpha_b * static_b (face dims) / sum_b static_b (last 3 dims)
 * dec: (N, L, dm+nb) decoder head output (row stride ld_dec); stat: (Ns, nb, dm) static bases, Ns in {N, N/entries}.
 * (model.py:961-996.)  use_head_alpha bit 0: weight the last 3 (head pose) dims too; bit 1: alpha = sigmoid(alpha)
 * (regularize_alpha = 'sigmoid', model.py:973-974). */
int msmd_heads_static_mix(const void* dec, long ld_dec, const void* stat, float* out, int N, int L, int dm,
                          int nb, int stat_batch, int use_head_alpha, int dtype, msmd_stream_t stream);

/* One CFG + DDPM ancestral update (model.py:396-432), in place on x (B, L, dm) fp32.
 * res: (n_entries*B, Lp+L, dm) fp32 denoiser outputs; scales[n_entries-1]; coefficients on the host
 * (c0, c1, sigma) as the reference computes them; z (B, L, dm) or NULL for the last step.
 * mode: 0 = incremental, 1 = independent (in-place accumulation order of the reference). target: 0 sample, 1 noise. */
int msmd_cfg_ddpm_step(float* x, const float* res, const float* z, const float* scales, int n_entries,
                       int B, int L, int Lp, int dm, int mode, int target, float c0, float c1, float sigma,
                       msmd_stream_t stream);

/* hipGraph-capturable sampler step (no per-step host scalars): the step index t lives on the device.
 * msmd_sampler_step_select: emb_row (d) = emb_all[t], coefs (3) = coef_table[t] = (c0, c1, sigma_t), then t -= 1.
 * msmd_cfg_ddpm_step_dev: msmd_cfg_ddpm_step with (c0, c1, sigma) read from `coefs` on the device
 * (sigma_1 must be stored as 0: the reference uses z = 0 at t = 1, model.py:378-381). */
int msmd_sampler_step_select(const void* emb_all, const float* coef_table, int* t_dev, void* emb_row,
                             float* coefs, int d, int dtype, msmd_stream_t stream);
int msmd_cfg_ddpm_step_dev(float* x, const float* res, const float* z, const float* scales, const float* coefs,
                           int n_entries, int B, int L, int Lp, int dm, int mode, int target, msmd_stream_t stream);

/* Few-step solver update (DDIM(eta), DPM-Solver++(2M); sampler.solver_table), in place on x (B, L, dm) fp32.
 * The CFG combine of res / scales / mode is msmd_cfg_ddpm_step's, same arithmetic in the same order; then
 *   D = p0 x + p1 theta,  x <- ax x + ath theta + b1 d_prev + sigma z,  d_prev <- D
 * d_prev (B, L, dm) fp32: the previous step's data prediction, in and out.  z (B, L, dm) or NULL (sigma unused).
 * msmd_cfg_solver_step_dev: the same with (p0, p1, ax, ath, b1, sigma) read from `coefs` (6) on the device.
 * msmd_sampler_solver_select: emb_row (d) = emb_tab[i], coefs (6) = coef_tab[i], then i -= 1 (the graph form:
 * emb_tab (S+1, d) holds the step embeddings gathered at the solver's timesteps, coef_tab (S+1, 6) its rows). */
int msmd_cfg_solver_step(float* x, const float* res, const float* z, const float* scales, float* d_prev,
                         int n_entries, int B, int L, int Lp, int dm, int mode, float p0, float p1, float ax,
                         float ath, float b1, float sigma, msmd_stream_t stream);
int msmd_cfg_solver_step_dev(float* x, const float* res, const float* z, const float* scales, float* d_prev,
                             const float* coefs, int n_entries, int B, int L, int Lp, int dm, int mode,
                             msmd_stream_t stream);
int msmd_sampler_solver_select(const void* emb_tab, const float* coef_tab, int* i_dev, void* emb_row,
                               float* coefs, int d, int dtype, msmd_stream_t stream);

/* msmd_cfg_solver_step plus the three streams of sample_separate (model.py:442-651) in one launch.  x, d_prev, res, z,
 * scales, mode and the six scalars are msmd_cfg_solver_step's and x / d_prev come out with its bits.  dec (n_entries*B,
 * Lp+L, dm+nb; row stride ld_dec), stat (stat_batch, nb, dm), stat_batch and use_head_alpha are msmd_heads_static_mix's
 * (res is its output on the same dec, after msmd_dynamic_threshold when that is on); dtype is that of dec and stat.  Per
 * element of the last L frames: dyn_e = dec[e][k], static_e = msmd_heads_static_mix's sum for entry e, alpha_e = the blend
 * weight a_{e,k} (k < nb); each is CFG-combined like res.  Then
 *   cum_static (B, L, dm) += ath * theta_static;   theta_dyn (B, L, dm) = the combined dynamic part (overwritten);
 *   theta_alpha (n_slots*B, L, nb): rows [slot*B, (slot+1)*B) = the combined blend weights.
 * slot in [0, n_slots).  msmd_cfg_streams_step_dev reads the six scalars from `coefs` and takes slot = 0 when n_slots == 1,
 * else n_slots - (*step_dev + 1): the ordinal S - i of step i with n_slots = S and step_dev the counter that
 * msmd_sampler_solver_select has just decremented to i - 1. */
int msmd_cfg_streams_step(float* x, const float* res, const void* dec, long ld_dec, const void* stat, const float* z,
                          const float* scales, float* d_prev, float* cum_static, float* theta_dyn, float* theta_alpha,
                          int slot, int n_slots, int n_entries, int B, int L, int Lp, int dm, int nb, int stat_batch,
                          int use_head_alpha, int mode, int dtype, float p0, float p1, float ax, float ath, float b1,
                          float sigma, msmd_stream_t stream);
int msmd_cfg_streams_step_dev(float* x, const float* res, const void* dec, long ld_dec, const void* stat, const float* z,
                              const float* scales, float* d_prev, float* cum_static, float* theta_dyn,
                              float* theta_alpha, const float* coefs, const int* step_dev, int n_slots, int n_entries,
                              int B, int L, int Lp, int dm, int nb, int stat_batch, int use_head_alpha, int mode,
                              int dtype, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * FLAME: blendshapes + pose correctives + joint regression + Rodrigues + kinematic chain + skinning
 * (reference utils/lbs.py:141-223, utils/flame.py:180-217) in two launches.
 *
 * One-time host-side packing (frame-invariant model constants, done by the caller at load time):
 *   JS   (NB+1, J*3): JS[0] = J_regressor . v_template, JS[1+l] = J_regressor . shapedirs[:, :, l]
 *                     (joint regression is linear in the shape, utils/lbs.py:185-189);
 *   dirs (3, Kp, Vp): dirs[c][k][v] = shapedirs[v][c][k] for k < NB, posedirs[k-NB][3v+c] for the next
 *                     (J-1)*9 rows, 0 beyond (Kp = 192, Vp = V rounded up to 64);
 *   v_template (3, Vp) and lbs_weights (J, Vp) as coordinate / joint planes.
 *
 * msmd_lbs_prepare: per frame, coef (B, Kp) = [betas | pose_feature = (R[1:] - I) | 0], the relative rigid
 *   transforms A (B, J, 12) (3x4 row-major) and optionally the posed joints (B, J, 3).
 *   pose: (B, J*3) axis-angle, or (B, J*9) rotation matrices when pose_is_matrix != 0.
 *   coef_hl (B, 2, Kp) bf16 (msmd_lbs_skin_bf16x3's operand) and at_tiles (msmd_lbs_skin_v2's skin_tiles records,
 *   J = 5 and Kp = 192 only) are optional outputs (NULL = skip).
 * msmd_lbs_skin: verts (B, V, 3) = sum_j w[v][j] A[b][j] . [v_template + coef . dirs ; 1].
 */
int msmd_lbs_prepare(const float* betas, const float* pose, const float* JS, const int* parents,
                     float* coef, void* coef_hl, float* A, float* joints, void* at_tiles, int B, int NB, int J, int Kp,
                     int pose_is_matrix, msmd_stream_t stream);
/* FLAME.forward's inputs (utils/flame.py:180-212) straight into msmd_lbs_skin_v2's tile records: coefficient row =
 * [shape (B, NS) | expr (B, NE)], pose6 (B, 6) = [global | jaw] axis-angle with the identity neck, eye (B, 6) or NULL
 * (identity), global rotation dropped when ignore_global_rot != 0 -- no concatenated betas / full_pose tensors.
 * coef (B, 192), A (B, 5, 12), joints (B, 5, 3): optional outputs (NULL = skip).  J = 5, Kp = 192.
 * One subject, many frames: with shape_varies (1 int) and v_template_folded (3, Vp) given (plus dirs (3, 192, Vp) and
 * v_template (3, Vp) to build it from), the call also writes  v_template_folded = v_template + sum_{k < 96} shape[0][k]
 * dirs[k]  and sets *shape_varies to whether any frame's first 96 shape coefficients differ from frame 0's -- on the
 * device, nothing reads back.  msmd_lbs_skin_v2 handed both skips those K groups when *shape_varies == 0.
 * The fold runs only when NS >= 96 and all four of shape_varies, v_template_folded, dirs and v_template are given; whenever
 * shape_varies is given and the fold does not run, *shape_varies is set nonzero ("varies", v_template_folded untouched), so
 * the pair can always be handed on to the skinning call.  Every write is stream ordered (kernels only: graph-capture safe). */
int msmd_flame_prepare(const float* shape, const float* expr, const float* pose6, const float* eye, const float* JS,
                       const int* parents, float* coef, float* A, float* joints, void* skin_tiles, int B, int NS, int NE,
                       int ignore_global_rot, int* shape_varies, float* v_template_folded, const float* dirs,
                       const float* v_template, int Vp, msmd_stream_t stream);
int msmd_lbs_skin(const float* coef, const float* A, const float* v_template, const float* dirs,
                  const float* lbs_weights, float* verts, int B, int J, int V, int Vp, int Kp,
                  msmd_stream_t stream);
/* Same contraction as msmd_lbs_skin in split-bf16 form (fp32 accumulation): coef_hl (B, 2, Kp) bf16 = hi/lo parts
 * written by msmd_lbs_prepare (may be NULL there when unused); dirs_hl (2, 3, Kp/8, Vp, 8) bf16 = hi/lo parts of
 * dirs regrouped in 8-element K octets.  coef.dirs ~= hi.hi + hi.lo + lo.hi: relative error 2^-16 per product
 * (measured max-abs-err on FLAME vertices vs the fp32 kernel: see tests), 5x fewer MFMA cycles. */
int msmd_lbs_skin_bf16x3(const void* coef_hl, const float* A, const float* v_template, const void* dirs_hl,
                         const float* lbs_weights, float* verts, int B, int J, int V, int Vp, int Kp,
                         msmd_stream_t stream);

/* msmd_lbs_skin_bf16x3 with the per-(vertex, frame) joint blend T = sum_j w_j A_j on the matrix pipe as well: for each
 * of the 12 components of the 3x4 transforms ONE v_mfma_f32_16x16x32_f16 contracts the five joints (both sides split
 * into fp16 hi + lo: 15 of the 32 K slots), its accumulator landing where the blendshape product puts p(vertex,
 * frame).
 * skin_tiles: ceil(B / 16) records of 18 432 bytes, one per 16 frames, written by msmd_lbs_prepare (its at_tiles
 *   argument) or msmd_lbs_pack and read by 18 contiguous one-KiB LDS-DMA pieces.  csrc/lbs_tiles.h DEFINES the record
 *   (sizes, offsets, the writers); in words:
 *     [0, 12 288)       coefficients as bf16 hi then lo, [chunk = (hi|lo) * 24 + k / 8][frame % 16][k % 8]
 *     [12 288, 18 432)  blend rows, fp16, [component m of the 3x4][slot / 8][frame % 16][slot % 8] with the 16 K slots
 *                       [Ah_0..4 | Al_0..4 | Ah_0..4 | 0];
 *   frames beyond B - 1 of the last record repeat frame B - 1.
 * 128 vertices per workgroup (8 waves), 16-frame tiles through a 4-deep LDS-DMA ring, one workgroup barrier per two
 * tiles; Vp = padded vertex count of the constant planes (any value >= V).  HBM-bound target: 60 936 algorithmic bytes
 * per frame.  shape_varies / v_template_folded: NULL, or msmd_flame_prepare's outputs (see there).
 * Reference: utils/lbs.py:141-223. */
int msmd_lbs_skin_v2(const void* skin_tiles, const float* v_template, const void* dirs_hl, const float* lbs_weights,
                     float* verts, int B, int J, int V, int Vp, int Kp, const int* shape_varies,
                     const float* v_template_folded, msmd_stream_t stream);

/* msmd_lbs_skin_v2 with fp16 vertices (opt-in; BASELINE configs[4] names the fp16 LBS pass): verts16 (B, V_ld, 3) fp16, V_ld
 * even and >= V (rows of V * 3 halves would put every other frame on a 2-byte boundary; slot V of a row receives a copy of
 * vertex V - 1).  Half the store stream that bounds the fp32 kernel: 30 144 + 660 algorithmic bytes per frame at V = 5023.
 *   single_plane == 0: skin_tiles / dirs = msmd_lbs_skin_v2's operands (18 KB records, dirs_hl): the fp32 kernel's arithmetic
 *     with one fp16 rounding at the store (equal to its output rounded once);
 *   single_plane != 0: skin_tiles = the 12 KB records of msmd_lbs_tiles_f16, dirs = ONE fp16 plane (3, Kp / 8, Vp, 8) of the
 *     blendshape directions: one MFMA per K group and coordinate instead of three; |error| <= 2^-11 |v| + 2^-10 sum_k
 *     |coef_k| |dirs_k| (the operands' own fp16 rounding, on the un-skinned blendshape offset) + the fp32 kernel's 5e-6.
 * Reference: utils/lbs.py:210-221 (fp32 there). */
int msmd_lbs_skin_v2_f16(const void* skin_tiles, const float* v_template, const void* dirs, const float* lbs_weights,
                         void* verts16, int B, int J, int V, int V_ld, int Vp, int Kp, const int* shape_varies,
                         const float* v_template_folded, int single_plane, msmd_stream_t stream);
/* msmd_lbs_skin_v2's tile records (18 432 bytes per 16 frames) -> the single-plane form's (12 288 bytes: coefficients hi + lo
 * as one fp16 number [k / 8][frame % 16][k % 8], then the blend rows; csrc/lbs_tiles.h defines both). */
int msmd_lbs_tiles_f16(const void* skin_tiles, void* tiles16, int B, msmd_stream_t stream);

/* Training through FLAME (the reference's use_vertex_space branch: training_script.py:167-176 -> utils/common.py:486-513
 * -> utils/lbs.py:141-223, differentiated by autograd there).
 * msmd_lbs_skin_v2_train: msmd_lbs_skin_v2 that also stores the un-skinned vertices v_posed = template + coef . dirs.
 * msmd_lbs_pack: (coef (B, Kp), A (B, 5, 12)) fp32 -> skin_tiles (and coef_hl (B, 2, Kp) bf16 when not NULL), for
 *   per-frame kinematics computed elsewhere (the differentiable pass builds them with autograd on (B, 5, 3, 3)-sized
 *   tensors).  Kp = 192.
 * msmd_lbs_skin_bwd: given grad_verts (B, V, 3) and v_posed: dp_planes (B, 3, Vp) = (sum_j w_j R_j)^T g (the A operand
 *   of dcoef = dp . dirs^T, an msmd_gemm) and dA (B, 5, 12) = sum_v w_j(v) g(v) [v_posed(v) ; 1]^T. */
int msmd_lbs_skin_v2_train(const void* skin_tiles, const float* v_template, const void* dirs_hl,
                           const float* lbs_weights, float* verts, float* v_posed, int B, int J, int V, int Vp, int Kp,
                           msmd_stream_t stream);
int msmd_lbs_pack(const float* coef, const float* A, void* coef_hl, void* skin_tiles, int B, int Kp, msmd_stream_t stream);
int msmd_lbs_skin_bwd(const float* grad_verts, const float* v_posed, const float* A, const float* lbs_weights,
                      float* dp_planes, float* dA, int B, int J, int V, int Vp, msmd_stream_t stream);

/* Landmarks by barycentric interpolation (utils/lbs.py:102-138): out (B, L, 3).
 * faces (F,3) int32; lmk_faces_idx (B or 1, L) int32 with batch stride idx_bstride (0 = shared);
 * bary (B or 1, L, 3) with batch stride bary_bstride. */
int msmd_landmarks(const float* verts, const int* faces, const int* lmk_faces_idx, long idx_bstride,
                   const float* bary, long bary_bstride, float* out, int B, int V, int L, msmd_stream_t stream);

/* Backward of msmd_landmarks: grad_lmk (B, L, 3) scattered to grad_verts (B, V, 3); faces / lmk_faces_idx / bary and their
 * batch strides exactly as the forward takes them.  Landmarks that share a vertex are summed without atomics, in
 * (landmark, corner) order: the result is bit-identical from run to run.  accumulate == 0: every vertex of grad_verts is
 * written (untouched ones with 0, in the same launch); accumulate != 0: the sums are added into grad_verts.
 * L <= MSMD_LANDMARKS_BWD_MAX_L (a frame's 3 L contributions are kept in LDS).  No gradient goes to the tables. */
#define MSMD_LANDMARKS_BWD_MAX_L 1024
int msmd_landmarks_bwd(const float* grad_lmk, const int* faces, const int* lmk_faces_idx, long idx_bstride,
                       const float* bary, long bary_bstride, float* grad_verts, int B, int V, int L, int accumulate,
                       msmd_stream_t stream);

/* Dynamic-contour LUT row (utils/flame.py:126-172): row (B) int32 from the neck-chain yaw; full_pose is (B, J*3)
 * axis-angle (pose2rot=True) or (B, J*9) rotation matrices (pose_is_matrix, pose2rot=False). */
int msmd_dynamic_lmk_row(const float* full_pose, const int* neck_chain, int n_chain, int* row, int B, int J,
                         int pose_is_matrix, msmd_stream_t stream);

/* batch_rodrigues (utils/lbs.py:270-301): R (N, 3, 3) from rot_vecs (N, 3). */
int msmd_batch_rodrigues(const float* rot_vecs, float* R, int N, msmd_stream_t stream);
/* Its vector-Jacobian product: grad_rot_vecs (N, 3) from grad_R (N, 3, 3) and the forward's input. */
int msmd_batch_rodrigues_bwd(const float* rot_vecs, const float* grad_R, float* grad_rot_vecs, int N, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Rotation conversions (reference utils/rotation_conversions.py:38-569), elementwise over n items.
 * op codes below; `conv` packs an Euler convention as 3 axis indices (X=0,Y=1,Z=2): a0 | a1<<2 | a2<<4.
 */
#define MSMD_ROT_QUAT_TO_MAT 0
#define MSMD_ROT_MAT_TO_QUAT 1
#define MSMD_ROT_AA_TO_QUAT 2
#define MSMD_ROT_QUAT_TO_AA 3
#define MSMD_ROT_AA_TO_MAT 4
#define MSMD_ROT_MAT_TO_AA 5
#define MSMD_ROT_6D_TO_MAT 6
#define MSMD_ROT_MAT_TO_6D 7
#define MSMD_ROT_AA_TO_6D 8
#define MSMD_ROT_EULER_TO_MAT 9
#define MSMD_ROT_MAT_TO_EULER 10
#define MSMD_ROT_QUAT_STANDARDIZE 11
#define MSMD_ROT_QUAT_INVERT 12
#define MSMD_ROT_QUAT_RAW_MUL 13 /* in2 = second quaternion */
#define MSMD_ROT_QUAT_MUL 14
#define MSMD_ROT_QUAT_APPLY 15 /* in2 = points (n,3) */
int msmd_rotation_convert(int op, const float* in, const float* in2, float* out, long n, int conv,
                          msmd_stream_t stream);
/* The vector-Jacobian product of msmd_rotation_convert(op, ...): grad_in (n, in width) -- and grad_in2 (n, in2 width) for
 * the two-operand ops, NULL otherwise -- from grad_out (n, out width) and the forward's INPUTS (intermediates are
 * recomputed; the forward saves nothing).  The derivative is that of the branch the forward took, as the reference's
 * autograd gives it: the Taylor branch below |angle| = 1e-6, zero through a _sqrt_positive_part argument <= 0, +-1
 * through _copysign / standardize_quaternion, zero through a norm at 0. */
int msmd_rotation_convert_bwd(int op, const float* in, const float* in2, const float* grad_out, float* grad_in,
                              float* grad_in2, long n, int conv, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Head pose from tracked face landmarks (reference dataset_processing/Step2_preprocess_head_pose_mediapipe.py).
 *
 * msmd_headpose_fit, one workgroup per frame of a ragged batch of clips laid end to end (n_frames frames in all):
 *   landmarks (n_frames, P, 3) fp32.  Frame f is (1 - plan_w[f]) landmarks[plan_a[f]] + plan_w[f] landmarks[plan_b[f]]:
 *   a tracked frame names itself with weight 0 (plan_b is then not read), a missing one its two tracked neighbours.
 *   plan_a, plan_b (n_frames) int32 frame indices into the whole batch, plan_w (n_frames) fp32.
 *   neutral (P, 3) fp32, read at static_idx only; static_idx (S) int32 in [0, P), 3 <= S <= MSMD_HEADPOSE_MAX_STATIC.  plan_a / plan_b / static_idx
 *   outside their ranges are the caller's error; the kernel clamps them, so nothing is read out of bounds.
 *   With X the S static points of the frame and Y those of the neutral shape (Umeyama's similarity fit, the reference's
 *   procrustes_analysis): cov = (1/S) (Y - mu_y)(X - mu_x)^T = U D V^T, Sg = diag(1, 1, det(U) det(V^T) < 0 ? -1 : 1),
 *   R = U Sg V^T, c = sum(D diag Sg) / rho2_x (rho2_x the summed per-axis population variance of X), t = mu_y - c R mu_x.
 *   Means and second moments are summed in double after the mean is subtracted, the 3 x 3 stage (one-sided Jacobi) runs in double.
 *   Outputs: R (n_frames, 9) row-major, c (n_frames), t (n_frames, 3), and, unless `aligned` is NULL, aligned (n_frames, P, 3) =
 *   c R x + t for every blended landmark x of the frame -- all fp32.
 *   OUTSIDE THE CONTRACT: a covariance of rank < 3 (collinear or coplanar static points).  Collinear points have no unique fit
 *   and the outputs are unspecified (possibly NaN).  Coplanar points (S = 3 always) still determine R: U's third column is
 *   completed as u0 x u1 and the sign rule above applies as it stands -- which is the reference's rule for a rank-deficient
 *   covariance, but the reference chooses between that rule and det(cov) < 0 by a numerical rank test, so agreement with it
 *   on (nearly) coplanar points is not promised.  Returns 1 for S outside [3, MSMD_HEADPOSE_MAX_STATIC], S > P or a NULL pointer other than `aligned`.
 *
 * msmd_headpose_smooth, one workgroup per clip: R (n_frames, 9) fp32 as msmd_headpose_fit wrote it; clip_offsets (n_clips + 1)
 *   int64 on the device, clip k owns frames [clip_offsets[k], clip_offsets[k + 1]); a clip shorter than `window` is left unwritten.
 *   Per clip: unit quaternions of R; signs made continuous (s_0 = 1, s_i = s_{i-1} (q_i . q_{i-1} < 0 ? -1 : 1) on the raw
 *   quaternions: a prefix product scanned MSMD_HEADPOSE_CHUNK frames at a time with a carried sign); a Savitzky-Golay filter over each
 *   component; renormalisation; the matrix, premultiplied by diag(1, -1, -1); its intrinsic Y-X-Z angles pitch = asin(-M[1][2]),
 *   yaw = atan2(M[0][2], M[2][2]), roll = atan2(M[1][0], M[1][1]).  ypr_deg (n_frames, 3) fp32 = (yaw, pitch, -roll) in degrees;
 *   R_out (n_frames, 9) fp32 or NULL = Ry(yaw) Rx(pitch) Rz(-roll) of those angles before their rounding to fp32 (the reference's
 *   R_modified).
 *   coeffs: window * window doubles on the device = the `window` symmetric interior coefficients, then the edge table
 *   (2 (window / 2), window): row r < window / 2 gives frame r from the clip's first `window` frames, row window / 2 + r gives
 *   frame F - window / 2 + r from its last `window` (scipy's mode='interp').  window odd, 3 <= window <= MSMD_HEADPOSE_MAX_WINDOW.
 *   The arithmetic is double; the quaternion's sign convention is free (the result depends on it only at a dot product of exactly 0).
 *   OUTSIDE THE CONTRACT: gimbal lock, |pitch| within 1e-3 degrees of 90 (yaw and roll are then not separately defined). */
#define MSMD_HEADPOSE_MAX_WINDOW 33
#define MSMD_HEADPOSE_CHUNK 256
#define MSMD_HEADPOSE_MAX_STATIC 64 /* msmd_headpose_fit: one static landmark per lane of a wave */
int msmd_headpose_fit(const float* landmarks, const int* plan_a, const int* plan_b, const float* plan_w, const float* neutral,
                      const int* static_idx, float* R, float* c, float* t, float* aligned, int n_frames, int P, int S,
                      msmd_stream_t stream);
int msmd_headpose_smooth(const float* R, const long* clip_offsets, int n_clips, const double* coeffs, int window, float* ypr_deg,
                         float* R_out, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Losses / training-step pieces (reference utils/common.py:198-620, 443-454, 769-832; training_script.py:548-551).
 */
/* out[0] = scale * mean over valid (n, t) of mean_{c in [c_lo, c_hi)} crit(D^order gt, D^order pred)
 *   gt, pred: (N, T, C) fp32; D^order = order-th temporal difference (0 = value, 1 = velocity, 2 = smoothness);
 *   frame t of the differenced sequence is valid when mask[t + order] holds, mask[tm] = tm < prefix ||
 *   tm - prefix < end_idx[n] (end_idx NULL: all valid); a NEGATIVE prefix masks the first |prefix| frames OUT instead
 *   (--no_constrain_prev, utils/common.py:382-385).  criterion 0 = squared error, 1 = absolute error.
 *   mode 1: compare D^order pred against 0 (the smoothness term).  acc_ws: 2 doubles of scratch.
 *   out is NaN when no frame is valid (the reference returns None there). */
int msmd_masked_seq_loss(const float* gt, const float* pred, const int* end_idx, float* out, double* acc_ws,
                         int N, int T, int C, int c_lo, int c_hi, int order, int prefix, int criterion, int mode,
                         float scale, msmd_stream_t stream);
/* d msmd_masked_seq_loss / d pred, ADDED into grad_pred (N, T, C) (channels outside [c_lo, c_hi) untouched): acc_ws is
 * the forward call's workspace (its valid-row count), upstream the incoming 0-dim gradient on the device.  What the
 * reference gets from autograd through utils/common.py:198-620 (training through the vertex-space loss). */
int msmd_masked_seq_loss_bwd(const float* gt, const float* pred, const int* end_idx, const double* acc_ws,
                             const float* upstream, float* grad_pred, int N, int T, int C, int c_lo, int c_hi, int order,
                             int prefix, int criterion, int mode, float scale, msmd_stream_t stream);
/* out[0] = -0.5 * sum(1 + logvar - mu^2 - exp(logvar)) over n elements. */
int msmd_kl_loss(const float* mu, const float* logvar, float* out, double* acc_ws, long n, msmd_stream_t stream);
/* In place: x (N, L, inner)[n, end_idx[n]*unit :, :] = 0 (or the last kept row when replicate != 0). */
int msmd_truncate_rows(float* x, const int* end_idx, int N, int L, int inner, int unit, int replicate,
                       msmd_stream_t stream);
/* One Adam step (torch.optim.Adam defaults) on flat fp32 arenas of n elements; grad is multiplied by grad_scale
 * first (1/world_size after a sum all-reduce).  step is the 1-based step count for bias correction. */
int msmd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                   float beta1, float beta2, float eps, int step, float grad_scale, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient exchange over RCCL / xGMI: the one exchange step on the path (SURVEY.md 8b "msmd_allreduce_bucket (RCCL)", 8e;
 * the reference steps one process, training_script.py:190-199 -- its data-parallel form sums the gradient of every
 * parameter over the ranks before optimizer.step()).  One process per GPU, one communicator per process; librccl is
 * resolved with dlopen at first use (csrc/comm.hip), so nothing here costs a process that never exchanges.
 *   msmd_comm_unique_id: rank 0 fills 128 bytes that every rank passes to msmd_comm_init (sent over any side channel);
 *   msmd_comm_init: collective over the job; the calling thread's current HIP device is the rank's GPU;
 *   msmd_allreduce_bucket: buf[0 .. n) <- SUM over ranks, in place, enqueued on `stream` (the reducer's side stream, behind
 *     an event of the compute stream: overlapped with the rest of backward); dtype MSMD_F32 (a bucket of the flat gradient
 *     arena), MSMD_BF16 / MSMD_F16 (its 16-bit staging copy: half the bytes over xGMI).
 *   msmd_comm_version: ncclGetVersion of the librccl in use (a copy the process already mapped -- torch's -- is adopted
 *     before anything is loaded), or -(1000 + n).
 * Return codes: 0, an ncclResult_t, or 1000 + n when librccl could not be loaded (1) / lacks a symbol (2) / reports a
 * major version other than the 2.x whose rccl.h slice csrc/comm.hip restates (3). */
int msmd_comm_version(void);
int msmd_comm_unique_id(void* id_out_128_bytes);
int msmd_comm_init(void** comm_out, int world, int rank, const void* id_128_bytes);
int msmd_comm_destroy(void* comm);
int msmd_allreduce_bucket(void* comm, void* buf, long n, int dtype, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Backward-pass building blocks (training; reference training_script.py:195).  dgrad / wgrad are msmd_gemm calls on
 * transposed operands: dX = dZ . W (W^T as the (K, N) operand), dW = dZ^T . X (both operands transposed).
 * The entries below with a dtype argument take MSMD_F32 or MSMD_BF16 (and msmd_dropout the same) and return 1 for any
 * other code; msmd_transpose and msmd_unfold_t, which only move bits, also take MSMD_F16.
 */
/* y[z][c][r] = x[z][r][c] for batch * batch_inner matrices; matrix z = zo * batch_inner + zi starts at
 * base + zo * stride + zi * stride_i (elements). */
int msmd_transpose(const void* x, void* y, int rows, int cols, long ldx, long ldy, int batch, long stride_x,
                   long stride_y, int batch_inner, long stride_x_i, long stride_y_i, int dtype, msmd_stream_t stream);
/* out[c] (+)= sum_r x[r][c] in fp32 (bias gradient, weight-norm reductions).  With a workspace of
 * msmd_colsum_workspace(rows, cols) bytes the sum is deterministic (per-row-block partial sums added in block order by a
 * second launch); ws = NULL: the row blocks meet through float atomics. */
long msmd_colsum_workspace(long rows, int cols);
int msmd_colsum(const void* x, float* out, long rows, int cols, long ld, int accumulate, int dtype, void* ws, long ws_bytes,
                msmd_stream_t stream);
/* y = act(z);  dz = dy * act'(z)  (exact erf GELU / ELU derivatives). */
int msmd_act_fwd(const void* z, void* y, long n, int act, int dtype, msmd_stream_t stream);
int msmd_act_bwd(const void* dy, const void* z, void* dz, long n, int act, int dtype, msmd_stream_t stream);
/* dz = dropout_mask(dy) * act'(z): backward of y = dropout_p(act(z)) in one pass (mask as msmd_dropout / msmd_gemm_ex). */
int msmd_act_bwd_dropout(const void* dy, const void* z, void* dz, long n, int act, float p,
                         const unsigned long* rng_state, unsigned int site, int dtype, msmd_stream_t stream);
/* LayerNorm backward for y = LN(x)*gamma + beta (x = the LN input, residual already added):
 * dx (rows, cols); dgamma / dbeta (cols) fp32 are ACCUMULATED into (zero them for a fresh gradient).
 * The row statistics are recomputed in two passes (mean, then the sum of squared deviations), as msmd_layernorm forms
 * them: no cancellation on rows whose mean is large against their spread.  cols <= 1024; dtype MSMD_F32 or MSMD_BF16.
 * ws: optional msmd_layernorm_bwd_workspace() bytes for per-workgroup partial sums (NULL: fp32 atomics). */
int msmd_layernorm_bwd(const void* dy, const void* x, const float* gamma, void* dx, float* dgamma, float* dbeta,
                       int rows, int cols, float eps, int dtype, void* ws, long ws_bytes, msmd_stream_t stream);
long msmd_layernorm_bwd_workspace(int rows, int cols);
/* msmd_layernorm_bwd that also writes dx_drop = dropout_mask(dx) / (1 - p) (mask of msmd_dropout / msmd_gemm_ex at
 * (rng_state, site): index = element / 4): the gradient the Linear in front of a post-LN block's LayerNorm wants
 * (x = residual + dropout_p(Linear(..)); reference: nn.TransformerDecoderLayer / HF Wav2Vec2EncoderLayer under
 * loss.backward(), training_script.py:196).  cols % 4 == 0, 16-byte aligned tensors. */
int msmd_layernorm_bwd_dropout(const void* dy, const void* x, const float* gamma, void* dx, void* dx_drop, float* dgamma,
                               float* dbeta, int rows, int cols, float eps, float p_drop, const unsigned long* rng_state,
                               unsigned int site, int dtype, void* ws, long ws_bytes, msmd_stream_t stream);
/* In place row softmax of scale * s over the first `cols` entries of rows with stride ld (the ld - cols padding
 * columns are zeroed), optional (Tq, cols) byte mask (row r uses mask row r % Tq);
 * backward (in place on dP): dS = scale * P o (dP - rowsum(dP o P)). */
int msmd_softmax_rows(void* s, const uint8_t* mask, long rows, int cols, int ld, int Tq, float scale, int dtype,
                      msmd_stream_t stream);
int msmd_softmax_bwd_rows(const void* P, void* dP, long rows, int cols, int ld, float scale, int dtype,
                          msmd_stream_t stream);

/* Transposed unfold of the zero-padded group-major signal xp (B, G, Tp, Cg) for the grouped positional-conv
 * weight gradient: out (G, Kk*Cg, ld_out)[g][kk*Cg + ci][b*T + t] = xp[b][g][t + kk][ci] (columns >= B*T zero). */
int msmd_unfold_t(const void* xp, void* out, int B, int T, int Tp, int G, int Cg, int Kk, long ld_out, int dtype,
                  msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Small utilities.
 */
int msmd_cast(const void* x, void* y, long n, int in_dtype, int out_dtype, msmd_stream_t stream);
/* y (rows, cols_out) = x (rows, cols_in) zero-padded / truncated per row (dtype convert allowed). */
int msmd_pad_cols(const void* x, void* y, long rows, int cols_in, int cols_out, int in_dtype, int out_dtype,
                  msmd_stream_t stream);
/* y[r, :] = mean over T of x[b, t, :]  (B, T, C) -> (B, C) fp32 (style_encoder.py:189). */
int msmd_mean_time(const void* x, float* y, int B, int T, int C, int dtype, msmd_stream_t stream);

/* Dynamic thresholding of the denoiser output, in place (reference model.py:396-402 / 578-584):
 * s_n = clamp(torch.quantile(|res[n, -L:, :]|, ratio), dt_min, dt_max) ('linear' interpolation between order
 * statistics, ATen's lerp), res[n] <- clamp(res[n], -s_n, s_n) over all T_all frames.  res: (N, T_all, C) fp32,
 * L * C <= 20480.  No sort: bisection on the float bit pattern with block-wide counts. */
int msmd_dynamic_threshold(float* res, int N, int T_all, int L, int C, float ratio, float dt_min, float dt_max,
                           msmd_stream_t stream);

/* Mixed-precision weight refresh, ONE launch per optimizer step: for each of n_weights (N, K) fp32 matrices inside
 * the flat parameter arena `base`, write its bf16 cast (N, K) into cast_arena and its bf16 transpose (K, N) into
 * transposed_arena.  meta (n_weights, 6) int64 device array: [src offset, N, K, cast offset, transposed offset, first
 * tile index]; tiles are 32 x 32, total_tiles = sum of ceil(N/32) ceil(K/32).  Replaces the per-weight autocast copies
 * an AMP training step of the reference would make (training_script.py:163-201 runs fp32; this build trains in bf16). */
int msmd_cast_transpose_multi(const float* base, const long* meta, int n_weights, long total_tiles, void* cast_arena,
                              void* transposed_arena, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training-batch assembly from an HBM-resident corpus: both consecutive L-frame windows of B samples in one launch
 * (reference DatasetPickle.__getitem__ + collate_fn, datasets.py:251-368, 424-503).
 *   audio_flat / coef_flat: all clips back to back (coef rows of C floats); desc (B, 8) int64 per sample:
 *   [audio offset, audio length, coef row offset, coef rows, start frame of window 0, zero frames padded in front,
 *    zero audio samples padded in front, clip index]; clip_stats (n_clips, 2) = each clip's audio mean / std.
 *   out_audio (2, B, n_audio): (x - mean) / (std + 1e-5) inside the clip, 0 in padding, window w covering samples
 *   [int(start_w * unit), int(end_w * unit)) then padded / trimmed to n_audio; out_motion (2, B, L, C):
 *   (row - coef_mean) / (coef_std + 1e-9) with zero rows where the reference zero-pads (statistics may be NULL). */
int msmd_batch_windows(const float* audio_flat, const float* coef_flat, const long* desc, const float* clip_stats,
                       const float* coef_mean, const float* coef_std, float* out_audio, float* out_motion, int B, int L,
                       int C, int n_audio, double audio_unit, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh renderer (the reference's utils/renderer.py draws through pyrender / OpenGL; an Instinct card has no graphics
 * pipe, so this is a compute rasteriser with its own Lambert shading: DESIGN.md 5.11).  Two launches per batch of
 * frames, no host synchronisation, no global atomics, the same bits on every run.
 *
 * msmd_render_vertices, one thread per (frame, vertex): verts (B, V, 3) -> screen (B, V, 3) = (x_s, y_s, eye depth d)
 *   and normals (B, V, 3), the eye-space unit vertex normal.
 *   - normal = normalised sum of (v1 - v0) x (v2 - v0) over the vertex's incident faces, gathered through the vertex ->
 *     face table csr_offsets (V + 1) / csr_faces (3 F) in table order; a zero sum gives (0, 0, 1);
 *   - rot (B, 3) or NULL: per-frame axis-angle rotation about t_center (3), angle = |r|, identity at 0 (cv2.Rodrigues);
 *   - view (3, 4) row-major: world -> eye, a rigid transform (the inverse of the camera pose); the camera looks down -z;
 *   - projection with aspect ratio 1: x_ndc = focal x_e / d, d = -z_e, focal = 1 / tan(yfov / 2); viewport
 *     x_s = (x_ndc / 2 + 1/2) W, y_s = (1/2 - y_ndc / 2) H: row 0 is the top, pixel (i, j) has its centre at (j + .5, i + .5).
 * msmd_render_raster, one workgroup per (frame, 64 x 64 tile): rgba (B, H, W, 4) uint8, depth (B, H, W) fp32 eye depth,
 *   face_id (B, H, W) int32 or NULL.
 *   - coordinates snap to 8 sub-pixel bits, rint(x_s * 256) half-even; edge functions at the pixel centres are exact
 *     64-bit integers; top-left fill rule (inside positive: a zero edge counts iff its oriented vector has dy > 0, or
 *     dy == 0 and dx > 0); no back-face culling;
 *   - NO CLIPPING: a face with a vertex at d < near, with zero snapped area, with a snapped coordinate of magnitude
 *     >= 2^30 (or not finite) or with a vertex id outside [0, V) is dropped whole;
 *   - depth: 1/d interpolated by e_k / (e_0 + e_1 + e_2) in fp32, fragments outside [near, far] discarded, the nearest
 *     wins and the lower face id wins a tie;
 *   - colour = base (ambient + (1/pi) sum_k I_k max(0, n . l_k)) clamped to [0, 1], floor(255 c + 0.5), alpha 255, with n
 *     the perspective-correct interpolated vertex normal, renormalised; shade (6) = base rgb, ambient rgb; lights
 *     (n_lights, 4) = eye-space unit direction TOWARDS the light, intensity;
 *   - background pixels: `background` (R | G << 8 | B << 16 | A << 24), depth 0, face id -1. */
int msmd_render_vertices(const float* verts, const int* faces, const int* csr_offsets, const int* csr_faces,
                         const float* view, const float* t_center, const float* rot, float* screen, float* normals,
                         int B, int V, int F, float focal, int H, int W, msmd_stream_t stream);
int msmd_render_raster(const float* screen, const float* normals, const int* faces, const float* shade,
                       const float* lights, int n_lights, void* rgba, float* depth, int* face_id, int B, int V, int F,
                       int H, int W, float near, float far, unsigned background, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Anti-aliased rendering: four samples per pixel.  Opt-in; one sample per pixel is the entry points above
 * and their bits.  The convention is this project's own (no parity with pyrender's sample positions):
 *   - sample points of pixel (i, j), in 1/256 pixel units from the pixel's top-left corner (256 j, 256 i):
 *     s0 = (96, 32), s1 = (224, 96), s2 = (32, 160), s3 = (160, 224): the rotated-grid 4x pattern (0.375, 0.125),
 *     (0.875, 0.375), (0.125, 0.625), (0.625, 0.875).  Integers on the snap grid, so the edge functions at a sample stay
 *     exact in int64 and the 2^30 snap limit holds;
 *   - every sample is rasterised exactly as the pixel centre is at one sample: the same snapped coordinates, orientation
 *     swap and top-left rule, evaluated at the sample point; depth 1/d interpolated at the sample with the same
 *     [near, far] discard; the nearest fragment wins per sample and the lower face id wins a tie; the same faces are
 *     dropped whole;
 *   - a face's pixel box is the pixels that have some sample inside the snapped bounding box: jmin = (xmin + 31) >> 8,
 *     jmax = (xmax - 32) >> 8, likewise for i, clipped to the tile and the image;
 *   - shading runs per sample at the sample's own position (sparse supersampling: no attribute is extrapolated outside
 *     its triangle) with msmd_render_raster's formulas, quantised per sample by floor(255 c + 0.5);
 *   - resolve: each of the four RGBA bytes of a pixel is (b0 + b1 + b2 + b3 + 2) >> 2 over the four samples' bytes; a
 *     covered sample contributes its quantised colour with alpha 255, an uncovered one the four bytes of `background`
 *     (so with a background alpha of 0 the stored alpha is the coverage).
 * msmd_render_raster_ms, samples = 4, one workgroup per (frame, 32 x 32 tile): rgba (B, H, W, 4) uint8 resolved; depth
 *   (B, H, W) the least depth over the pixel's covered samples, 0 if none; sample_face_id (B, H, W, 4) int32 or NULL, -1
 *   for an uncovered sample; sample_depth (B, H, W, 4) fp32 or NULL, 0 for an uncovered sample.  Both sample buffers are
 *   16-byte aligned.  samples = 1 forwards to msmd_render_raster with the sample buffers of shape (B, H, W, 1)
 *   (sample_depth is then a copy of depth).  Any other `samples` returns 1 before anything is launched.
 * msmd_render_shade_textured_ms, samples = 4: the deferred pass of msmd_render_shade_textured over sample_face_id
 *   (B, H, W, 4): every sample with 0 <= id < F is shaded at its own position with that pass's formulas (uv, the analytic
 *   level of detail from the exact per-PIXEL steps, the trilinear fetch), any other sample contributes `background`, and
 *   every pixel with at least one shaded sample is overwritten with the resolve of its four; other pixels are left as they
 *   are.  (u, v, lambda) is not offered.  samples = 1 forwards to msmd_render_shade_textured without uvl. */
int msmd_render_raster_ms(const float* screen, const float* normals, const int* faces, const float* shade,
                          const float* lights, int n_lights, void* rgba, float* depth, int* sample_face_id,
                          float* sample_depth, int B, int V, int F, int H, int W, float near, float far,
                          unsigned background, int samples, msmd_stream_t stream);
int msmd_render_shade_textured_ms(const float* screen, const float* normals, const int* faces, const float* vt, const int* ft,
                                  const float* pyramid, int Ht, int Wt, const float* shade, const float* lights,
                                  int n_lights, const int* sample_face_id, void* rgba, int B, int V, int F, int Nt, int H,
                                  int W, float near, unsigned background, int samples, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Textured shading (the reference's render_mesh(tex_img, tex_uv)).  A deferred, pixel-parallel pass behind
 * msmd_render_raster: it reads that launch's face_id buffer and overwrites rgba at the covered pixels.  The conventions are
 * the ordinary OpenGL / OBJ ones (GL_REPEAT, GL_LINEAR magnification, GL_LINEAR_MIPMAP_LINEAR minification, v up, no sRGB
 * conversion), stated here because they are this project's: there is no pixel parity with pyrender.
 *
 * Pyramid of a (Ht, Wt, 3 | 4) uint8 image (alpha ignored), 1 <= Ht, Wt <= MSMD_TEXTURE_MAX_SIDE, any size: L = 1 + floor(log2(max(Ht, Wt)))
 *   levels, level l + 1 of size max(1, H_l >> 1) x max(1, W_l >> 1), stored one after the other as fp32 RGBA texels (16
 *   bytes, values 0 .. 255, the fourth component 0).  Level 0 is the image's bytes converted; texel (y, x) of level l + 1 is
 *   ((a + b) + (c + d)) * 0.25f in fp32 with a = (2y, 2x), b = (2y, min(2x + 1, W_l - 1)), c = (min(2y + 1, H_l - 1), 2x),
 *   d = (min(2y + 1, H_l - 1), min(2x + 1, W_l - 1)) of level l as stored; a trailing odd row or column is not read.
 * msmd_texture_texels: host only; the pyramid's texel count, or -1 outside the limits.
 * msmd_texture_mips: img (Ht, Wt, channels) uint8, channels 3 or 4 -> pyramid (msmd_texture_texels(Ht, Wt), 4) fp32; one
 *   launch per level.
 * msmd_render_shade_textured, a wave per 64-pixel row segment: at every pixel with 0 <= face_id < F
 *   - corner coordinates (u_k, v_k) = vt[ft[f, k]], vt (Nt, 2) fp32, ft (F, 3) int32 per-corner indices in the face order of
 *     `faces`, swapped with the vertices where face_setup orients the face; an index outside [0, Nt) gives (0, 0);
 *   - u, v interpolated unwrapped with the shading pass's perspective-correct weights p_k = w_k q_k / iz;
 *   - level of detail, analytic per pixel: with D = sum w_k q_k, N_u = sum w_k q_k u_k and the exact per-pixel steps
 *     dw_k/dj = a_k / A, dw_k/di = c_k / A (integer edge steps over the doubled area), du/dj = (dN_u/dj - u dD/dj) / D and
 *     likewise for v and i; rho_j^2 = (Wt du/dj)^2 + (Ht dv/dj)^2, lambda = 0.5 log2(max(rho_j^2, rho_i^2)) clamped to
 *     [0, L - 1]; a lambda that is not finite (or has a rho^2 that is not) is 0;
 *   - level l at (u, v): a u or v that is not finite is 0; U = u - floor(u), x = U W_l - 0.5, y = (1 - (v - floor(v))) H_l -
 *     0.5 (row 0 is the top of the image, v = 0 its bottom edge), x0 = floor(x), fx = x - x0, columns x0 mod W_l and
 *     (x0 + 1) mod W_l (mathematical modulo), rows likewise, c = (1 - fy)((1 - fx) t00 + fx t10) + fy((1 - fx) t01 + fx t11);
 *   - trilinear: l0 = min(floor(lambda), L - 1), l1 = min(l0 + 1, L - 1), f = lambda - l0, T = (1 - f) c_l0 + f c_l1;
 *   - colour = clamp((T / 255)(ambient + diffuse), 0, 1), floor(255 c + 0.5), alpha 255: msmd_render_raster's lighting
 *     (the same device function) with the base colour replaced by the texel;
 *   - uvl (B, H, W, 3) fp32 or NULL: (u, v, lambda) as sampled (u and v after the not-finite rule, unwrapped; lambda
 *     clamped), zeros where face_id is outside [0, F).
 *   Depth and face_id are not written and pixels outside the mesh are left as they are. */
#define MSMD_TEXTURE_MAX_SIDE 4096
long msmd_texture_texels(int Ht, int Wt);
int msmd_texture_mips(const void* img, int Ht, int Wt, int channels, float* pyramid, msmd_stream_t stream);
int msmd_render_shade_textured(const float* screen, const float* normals, const int* faces, const float* vt, const int* ft,
                               const float* pyramid, int Ht, int Wt, const float* shade, const float* lights,
                               int n_lights, const int* face_id, void* rgba, float* uvl, int B, int V, int F, int Nt,
                               int H, int W, float near, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Per-vertex colours: a deferred, pixel-parallel pass behind msmd_render_raster[_ms], the sibling of the textured
 * pass with its launch shape (one workgroup per (frame, 64 x 16 strip)).  It reads that launch's face_id / sample_face_id buffer
 * and overwrites rgba; depth and face ids are not written.
 * msmd_render_shade_vertex_color: vcol (V, 4) uint8 RGBA per vertex, or (B, V, 4) with color_per_frame != 0; 4-byte aligned; alpha
 *   is not read.  At a shaded point of face f
 *   - corner colours c_k are the bytes at the face's vertex ids in the order face_setup oriented them (the face and its colours
 *     swap together);
 *   - per channel C = (p0 c0 + p1 c1) + p2 c2 in fp32 with the perspective-correct weights p_k = w_k q_k / iz of the textured pass;
 *   - lit != 0: colour = clamp((C / 255)(ambient + diffuse), 0, 1) with msmd_render_raster's lighting (the same device function);
 *     lit == 0: colour = clamp(C / 255, 0, 1), the interpolated colour itself; floor(255 c + 0.5), alpha 255.
 *   samples == 1: face_id (B, H, W); a pixel with 0 <= face_id < F whose face the set-up accepts is overwritten, every other is left
 *   as it is (`background` is not read).  samples == 4: sample_face_id (B, H, W, 4), 16-byte aligned; every covered sample is shaded
 *   at its own position, an uncovered one contributes the four bytes of `background`, and a pixel with a shaded sample receives the
 *   rounded mean of its four ((b0 + b1 + b2 + b3 + 2) >> 2 per byte); other pixels are left as they are.
 *   Returns 1 (hipErrorInvalidValue) before a launch for any other `samples`, a size below 1, n_lights < 0, near <= 0, a NULL
 *   sample_face_id or vcol, or a misaligned vcol / sample_face_id. */
int msmd_render_shade_vertex_color(const float* screen, const float* normals, const int* faces, const unsigned char* vcol,
                                   int color_per_frame, int lit, const float* shade, const float* lights, int n_lights,
                                   const int* sample_face_id, void* rgba, int B, int V, int F, int H, int W, float near,
                                   unsigned background, int samples, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * FLAMETex albedo model (reference utils/flame.py:247-301): a linear texture space over an (Hs, Ws, 3)
 * image (the reference's is 512 x 512), evaluated for ONE code, nearest-resized to (Hd, Wd) and channel-reversed.
 *   mean (Hs Ws 3) fp32, basis (Hs Ws 3, n_tex) fp32 row-major and contiguous, code (n_tex) fp32 (reference l.292: row 0 of
 *   texcode; every copy is the same image, l.300).  1 <= Hs, Ws, Hd, Wd <= MSMD_FLAMETEX_MAX_SIDE,
 *   1 <= n_tex <= MSMD_FLAMETEX_MAX_TEX, else hipErrorInvalidValue without a launch.  Row offsets are 64-bit.
 *   - source index of destination index d (F.interpolate's nearest rule, l.299): min((int)floorf(d * scale), S - 1) in fp32
 *     with scale = (float)S / (float)D; at 512 -> 256 the even rows and columns;
 *   - value of channel c at (y, x) (l.296-300): mean[r] + sum_k basis[r, k] code[k], r = (sy(y) Ws + sx(x)) 3 + (2 - c).  The
 *     three rows of a pixel are one run of 3 n_tex floats; 16 lanes read it, lane l adds columns l, l + 16, ... in
 *     ascending order by fma, the 16 sums are added by the xor butterfly 8, 4, 2, 1 and the mean is added last.  The order is a
 *     function of n_tex alone: both formats and every copy hold the same fp32 value.
 * msmd_flametex_forward: out_format MSMD_TEX_PLANAR_F32 -> out (n_copies, 3, Hd, Wd) fp32; MSMD_TEX_IMAGE_U8 -> out
 *   (Hd, Wd, 3) uint8 RGB, byte c = floorf(fmaf(255.f, fminf(fmaxf(value_c, 0.f), 1.f), 0.5f)) (NaN gives 0), n_copies must be
 *   1.  n_copies == 0 succeeds without a launch.  One launch, no allocation, no host synchronisation.
 * msmd_flametex_backward_workspace: host only; the floats msmd_flametex_backward needs in `workspace` (-1 outside the limits).
 * msmd_flametex_backward: grad_out (n_copies, 3, Hd, Wd) fp32 -> grad_code (n_tex) fp32,
 *   grad_code[k] = sum_{c, y, x} basis[r(c, y, x), k] sum_copies grad_out[copy, c, y, x]  (the buffers get no gradient).
 *   Two launches: a workgroup adds its run of consecutive pixels in pixel order (copies first, in copy order; the channels of
 *   a column as (row 0 + row 1) + row 2) into its row of the workspace, then each column of the workspace is added in row
 *   order, 64 consecutive segments first and the 64 segment sums after.  fp32 throughout, no floating-point atomics: the same
 *   inputs give the same bits on every run. */
#define MSMD_TEX_PLANAR_F32 0
#define MSMD_TEX_IMAGE_U8 1
#define MSMD_FLAMETEX_MAX_SIDE 4096
#define MSMD_FLAMETEX_MAX_TEX 256
int msmd_flametex_forward(const float* mean, const float* basis, const float* code, void* out, int out_format, int n_copies,
                          int Hs, int Ws, int Hd, int Wd, int n_tex, msmd_stream_t stream);
long msmd_flametex_backward_workspace(int Hd, int Wd, int n_tex);
int msmd_flametex_backward(const float* basis, const float* grad_out, int n_copies, float* grad_code, float* workspace,
                           int Hs, int Ws, int Hd, int Wd, int n_tex, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Audio front end (the reference calls librosa.load(path, sr=16000), inference.py:232): interleaved PCM of any rate and
 * channel count -> 16 kHz mono fp32, z-normalised per clip.  One call of each entry point
 * (three launches) for a ragged group of clips that share the input rate and the sample type; every step is deterministic
 * and a clip's bits do not depend on its group.
 *
 * Definition, fs_out = 16000, g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g:
 *   downmix   x[k] = (sum_c pcm[k, c]) / C: fp32, summed in channel order, one correctly rounded division; int16 samples
 *             are scaled by 2^-15 first; x is zero outside [0, N);
 *   filter    s = rho min(1, L / M), rho = 0.9475937167399596, beta = 14.769656459379492, 64 zero crossings:
 *             h(t) = s sinc(s t) I0(beta sqrt(1 - (s t / 64)^2)) / I0(beta) for |s t| < 64, else 0 (t in input samples,
 *             sinc(u) = sin(pi u) / (pi u)); no per-phase renormalisation;
 *   output    y[n] = sum_k x[k] h(n M / L - k), n = 0 .. ceil(N L / M) - 1; all index arithmetic in 64 bits;
 *   same rate fs_in == fs_out: y = x exactly, no filter (taps = 0, L = M = 1);
 *   z-norm    (y - mean) / (std + 1e-5), population std, per clip over y; sums and sums of squares in double, one partial
 *             pair per run of MSMD_AUDIO_RUN outputs, combined in run order; no floating-point atomics.
 *
 * desc (n_clips, 5) int64 on the device, per clip: [offset of its first sample in pcm (in samples, not frames), frames N,
 *   channels C, offset of its first output in out, output length ceil(N L / M)].
 * bank (taps, L) fp32, taps = 2 ceil(64 / s) + 2, half = taps / 2 - 1: bank[i][r] = h(((r M) mod L) / L - (i - half)), the
 *   tap-major polyphase table over the OUTPUT's phase order r = n mod L (utils/audio.filter_bank builds it in float64).
 *   Output n with k0 = n M div L is sum_i x[k0 + i - half] bank[i][n mod L]: four interleaved fma chains over i, added as
 *   (a0 + a1) + (a2 + a3).
 * msmd_audio_resample: pcm (pcm_elems samples, int16 if is_int16 else fp32) -> out (out_elems) and partials
 *   (n_clips, ceil(max_out_len / MSMD_AUDIO_RUN), 2) double = each run's (sum, sum of squares); rows past a clip's last
 *   run are not written.  max_out_len = the longest output of the group.  The staged span of a run,
 *   (MSMD_AUDIO_RUN - 1) M div L + 2 + taps samples, must fit 64 KB of LDS (returns 1 otherwise: rates above ~650 kHz).
 *   Reads and writes the descriptors would place outside pcm_elems / out_elems are dropped.
 * msmd_audio_znorm: two launches.  One wave per clip adds the clip's partial pairs in run order and leaves stats (n_clips, 2)
 *   double = (mean, 1 / (std + 1e-5)); then out is normalised in place from stats.  Linear in the clips' lengths.
 * n_clips <= MSMD_AUDIO_MAX_CLIPS per call (the clip is the grid's y index). */
#define MSMD_AUDIO_RUN 256
#define MSMD_AUDIO_MAX_CLIPS 65535
int msmd_audio_resample(const void* pcm, long pcm_elems, int is_int16, const long* desc, int n_clips, long max_out_len,
                        int L, int M, int taps, const float* bank, float* out, long out_elems, double* partials,
                        msmd_stream_t stream);
int msmd_audio_znorm(float* out, long out_elems, const long* desc, int n_clips, long max_out_len, const double* partials,
                     double* stats, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Baseline JPEG encoder: frames (B, H, W, 3 | 4) uint8 on the device -> one JFIF file per frame, back to
 * back in one byte stream.  The reference hands its frames to ffmpeg (utils/media.py); here a Motion-JPEG AVI is written
 * from these bytes by utils/media.py.  Everything is integer arithmetic: the bytes are a pure function of the pixels.
 *
 * Definition (1 <= H, W <= MSMD_JPEG_MAX_SIDE, quality in [1, 100], `>>` arithmetic, `div` floor division):
 *   input     pixel (y, x) of frame b at frames + b frame_stride + y row_stride + x pixel_stride (bytes), R, G, B in that
 *             order; pixel_stride 3 or 4, a fourth byte is ignored.  With pixel_stride 4 and every stride and the base a
 *             multiple of 4 the kernel loads 4 bytes per pixel: the fourth byte of the last pixel must be readable.
 *   padding   to multiples of 8 by repeating the last column and row; SOF0 carries the true H and W.
 *   colour    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *             Cb = clamp(((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128, 0, 255)
 *             Cr = clamp(((32768 R - 27439 G - 5329 B + 32768) >> 16) + 128, 0, 255);  4:4:4, an MCU is (Y, Cb, Cr) of 8 x 8.
 *   DCT       x = sample - 128; M[k][n] = rint(2^15 c_k cos((2 n + 1) k pi / 16)), c_0 = 1 / (2 sqrt 2), c_k = 1 / 2;
 *             C = M X M^T exactly, no intermediate rounding: rows in int32 (< 2^24), columns in int64 (< 2^41); C is the
 *             DCT scaled by 2^30 and within 0.042 (< 1/16) of the real-valued DCT for every input.
 *   quantiser Q = clamp((base s + 50) div 100, 1, 255), s = 5000 div q below 50, else 200 - 2 q, base = T.81 Annex K.1;
 *             value = sign(C) ((2 |C| + d) div (2 d)), d = Q 2^30 (round half away from zero); AC clamped to +-1023.
 *   entropy   zig-zag order; Annex K.3 typical Huffman tables; DC difference per component (clamped to +-2047, which the
 *             ranges above never reach); restart interval MSMD_JPEG_RESTART_INTERVAL MCUs in raster order whatever
 *             the width: predictors reset, the interval's last byte filled with 1-bits, 0xFF -> 0xFF 0x00 inside it, RSTn
 *             (n = interval index mod 8) between intervals.
 *   file      header (SOI, APP0 JFIF 1.01 density 1:1, DQT x 2, SOF0, DHT x 4, DRI, SOS: the same bytes for every frame of
 *             a call, built by the caller) + scan + EOI.
 *
 * msmd_jpeg_intervals: ceil(ceil(H/8) ceil(W/8) / 32), the intervals of one frame (host arithmetic only; -1 if out of range).
 * msmd_jpeg_coefficients, one workgroup per (frame, interval): coef (B, n_int, 32, 3, 64) int16, quantised, zig-zag order;
 *   the MCUs of the last interval past the frame's last MCU are zeros.
 * msmd_jpeg_measure, three launches: the entropy coder run for its lengths only, then two scans.  interval_len (B, n_int)
 *   int32 = stuffed bytes of each interval; interval_rel (B, n_int) int64 = offset of the interval in its frame's file;
 *   frame_size (B) int64; offsets (B + 1) int64 = where each file starts in the stream, offsets[B] = the stream's length
 *   (the one number the host has to read before it can allocate `out`).
 * msmd_jpeg_write, one launch: the entropy coder again, each interval written at offsets[b] + interval_rel[b, i] with its
 *   RSTn / EOI behind it, and `header` (header_len bytes on the device) at each file's start.  Bytes that would fall outside
 *   [0, out_bytes) are dropped. */
#define MSMD_JPEG_RESTART_INTERVAL 32
#define MSMD_JPEG_MAX_SIDE 16384
int msmd_jpeg_intervals(int H, int W);
int msmd_jpeg_coefficients(const void* frames, long frame_stride, long row_stride, int pixel_stride, int B, int H, int W,
                           int quality, short* coef, msmd_stream_t stream);
int msmd_jpeg_measure(const short* coef, int B, int H, int W, int header_len, int* interval_len, long* interval_rel,
                      long* frame_size, long* offsets, msmd_stream_t stream);
int msmd_jpeg_write(const short* coef, int B, int H, int W, const void* header, int header_len, const long* interval_rel,
                    const long* offsets, void* out, long out_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Baseline JPEG decoder, the inverse of the encoder above: B files of one size and sampling, back to back in
 * one byte stream on the device -> pixels (B, H, W, 3 | 4) uint8.  The host (jpeg_format.jpeg_parse) reads the marker segments, finds
 * the restart intervals and builds the tables below; the three entries are the entropy decode, the inverse DCT and the colour
 * pass.  Integer arithmetic throughout: the pixels are a pure function of the file's bytes.
 *
 * Accepted (everything else is refused by the host with ValueError before a launch): SOF0, 8 bit, 1 <= H, W <=
 *   MSMD_JPEG_MAX_SIDE; one scan with all components, Ss = 0, Se = 63, Ah = Al = 0; one component (MSMD_JPEG_GREY; its
 *   sampling factors are ignored, as T.81 A.2.2 has it for a scan of one component) or three with luminance (1,1), (2,1) or
 *   (2,2) and both chrominance components (1,1): MSMD_JPEG_444 / _422 / _420; DQT with 8-bit entries, ids 0-3; DHT classes 0 / 1,
 *   ids 0 / 1, any valid lengths up to 16; no DHT at all: the Annex K.3 tables; DRI any or none (then the scan is one interval).
 * Geometry (`layout` fixes hs, vs = 1,1 / 1,1 / 2,1 / 2,2): an MCU is 8 hs x 8 vs pixels, mcux = ceil(W / 8 hs), mcuy =
 *   ceil(H / 8 vs), n_mcu = mcux mcuy; component c has h_c x v_c blocks per MCU ((hs, vs) for c = 0, else (1, 1)), in the scan row
 *   by row inside the MCU, Y then Cb then Cr.  Its plane is bh_c = mcuy v_c by bw_c = mcux h_c blocks; the planes of a frame
 *   follow one another, msmd_jpeg_decode_blocks(H, W, layout) = sum_c bh_c bw_c blocks in all (-1 if out of range).
 * Table set (MSMD_JPEG_TABLE_SET_BYTES = 192 + 8 + 4 x 384 bytes, built by the host, de-duplicated by its bytes): Q of
 *   component 0, 1, 2 (64 bytes each, zig-zag order as in DQT); the bytes Td0 Ta0 Td1 Ta1 Td2 Ta2 0 0; the Huffman tables DC 0,
 *   DC 1, AC 0, AC 1 in canonical form (T.81 F.2.2.3), each int32 maxcode[16] (-1: no code of that length), int32 delta[16] =
 *   valptr - mincode, then HUFFVAL padded to 256 bytes.
 * Interval table: n_entries rows of three int64, n_entries a multiple of MSMD_JPEG_DECODE_LANES (a workgroup): [0] byte offset
 *   of the interval in the stream, [1] = length | frame << 32, [2] = first MCU | table set << 32.  All rows of one workgroup
 *   name one table set (its first row's); a row with frame = -1 is padding.  A row that points outside the stream, the frame
 *   range or the MCU range is skipped.
 * Entropy decode (T.81 F.2.2) of one interval = MCUs [first, min(first + Ri, n_mcu)) (Ri = 0: to n_mcu), predictors 0 at its
 *   start.  The bits are the interval's bytes with every 0x00 that follows a 0xFF dropped; past the end the reader supplies
 *   zero bits; no byte outside [offset, offset + length) is read.  A unit is a Huffman code and its extra bits.  DC: code ->
 *   category s <= 16, diff = EXTEND(RECEIVE(s), s), pred = sat16(pred + diff), coefficient 0 = pred.  AC from k = 1: code ->
 *   (r, s); s = 0: r = 15 adds 16 to k, any other r ends the block; else k += r, coefficient k = sat16(EXTEND(RECEIVE(s), s)),
 *   k += 1.  Decode errors, checked per unit in this order: no code within 16 bits, or a DC category above 16
 *   (MSMD_JPEG_ERR_CODE); bits consumed past the interval's end (MSMD_JPEG_ERR_OVERRUN); k past 63 after adding a run, ZRL
 *   included (MSMD_JPEG_ERR_RUN).  The lane ORs the bit into status[frame] and stops its interval without storing the unit's
 *   coefficient; what it has not written stays zero.  MSMD_JPEG_ERR_RESTART is set by the host in the initial status where
 *   the number of intervals is not ceil(n_mcu / Ri) or the RSTn do not count mod 8; interval k of the file is then decoded as
 *   interval k of the frame for k below both counts.
 * Inverse DCT: F = coefficient x Q in natural order, x = M^T F M with the encoder's M (S = 15) and no intermediate rounding,
 *   |F| < 2^23, every absolute column sum of M is 86 567 < 2^17: pass 1 < 2^40, pass 2 < 2^57, both int64;
 *   sample = clamp(((x + 2^29) >> 30) + 128, 0, 255).
 * Upsampling (libjpeg's triangle filters) of a chrominance plane of true size cw = ceil(W / hs), ch = ceil(H / vs), p = a row:
 *   (2,1): out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2, out[0] = p[0], out[2cw-1] = p[cw-1].
 *   (2,2): output row 2j: r = 3 p[j] + p[j-1], row 2j+1: r = 3 p[j] + p[j+1] (row -1 is row 0, row ch is row ch - 1); out[2i] =
 *   (3 r[i] + r[i-1] + 8) >> 4, out[2i+1] = (3 r[i] + r[i+1] + 7) >> 4, out[0] = (4 r[0] + 8) >> 4, out[2cw-1] = (4 r[cw-1] + 7) >> 4.
 * Colour, cb = Cb - 128, cr = Cr - 128: R = clamp(Y + ((91881 cr + 32768) >> 16)), G = clamp(Y + ((-22554 cb - 46802 cr +
 *   32768) >> 16)), B = clamp(Y + ((116130 cb + 32768) >> 16)); grey: R = G = B = Y; a fourth channel is 255.
 *
 * msmd_jpeg_decode_coefficients: zeroes coef (B, blocks, 64) int16 (zig-zag order, block-raster order per component plane),
 *   then one lane per interval-table row.  status (B) int32 is ORed into, never cleared: the host uploads its initial value.
 * msmd_jpeg_decode_planes: frame_set (B) int32 = the table set of each frame; planes (B, 64 blocks) uint8, each component's
 *   plane padded to whole blocks, row pitch 8 bw_c.
 * msmd_jpeg_decode_pixels: pixels (B, H, W, channels) uint8 contiguous, 4-byte aligned; channels 3 or 4.
 * Each returns 1 for sizes out of range, a null pointer, n_entries not a positive multiple of the lanes or n_sets < 1. */
#define MSMD_JPEG_GREY 0
#define MSMD_JPEG_444 1
#define MSMD_JPEG_422 2
#define MSMD_JPEG_420 3
#define MSMD_JPEG_ERR_CODE (1 << 0)
#define MSMD_JPEG_ERR_RUN (1 << 1)
#define MSMD_JPEG_ERR_OVERRUN (1 << 2)
#define MSMD_JPEG_ERR_RESTART (1 << 3)
#define MSMD_JPEG_TABLE_SET_BYTES 1736
#define MSMD_JPEG_DECODE_LANES 64
long msmd_jpeg_decode_blocks(int H, int W, int layout);
int msmd_jpeg_decode_coefficients(const void* stream_bytes, long n_bytes, const long* intervals, int n_entries,
                                  const void* table_sets, int n_sets, int B, int H, int W, int layout, int restart_interval,
                                  short* coef, int* status, msmd_stream_t stream);
int msmd_jpeg_decode_planes(const short* coef, const void* table_sets, int n_sets, const int* frame_set, int B, int H, int W,
                            int layout, void* planes, msmd_stream_t stream);
int msmd_jpeg_decode_pixels(const void* planes, int B, int H, int W, int layout, int channels, void* pixels,
                            msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Style losses (reference utils/common.py:29-91 StyleAdherenceLoss, 835-875 nt_xent_loss).  fp32, contiguous,
 * no allocation, no host synchronisation, no floating-point atomics: every sum has one owner and an order that is a function
 * of the shape alone, so the same inputs give the same bits on every run and a batch row's bits do not depend on its batch.
 *
 * Style adherence, X (B, T, F) against S (B, K, F), lambda >= 0:
 *   d[b, t, k] = (1 / F) sum_f (X[b, t, f] - S[b, k, f])^2, from the differences, ascending f by fma, one division by F;
 *   soft != 0: w = softmax_k(-lambda d), L[b, t] = sum_k w_k d_k; stat (B, T, 2) fp32 = (m, log sum_k exp(-lambda (d_k - m))),
 *     m = min_k d_k: the soft minimum's log-sum-exp -lambda m + log(.) kept as its two parts, so that a recomputed weight
 *     exp(-lambda (d_k - m) - log(.)) does not carry the lambda m 2^-24 of a sum rounded to one fp32 number;
 *   soft == 0: L[b, t] = min_k d_k; stat (B, T) int32 = the lowest index that attains it.
 *   The running (min, sum e, sum e d), e = exp(-lambda (d - min)), is kept per lane over k = j, j + 16, ... and rescaled when
 *   the minimum moves; a row's 16 lanes are joined by the xor butterfly 8, 4, 2, 1.
 * msmd_style_adherence_forward: one launch, a workgroup per MSMD_STYLE_ROWS rows of one b; S[b] passes through LDS in tiles of
 *   MSMD_STYLE_KTILE frames, MSMD_STYLE_FCHUNK features at a time (any F).  Writes L (B, T) and stat; no workspace.
 * msmd_style_adherence_backward: g = the gradient of L's rows, read at g[(b T + t) g_stride] * g_scale (g_stride 0: one
 *   device scalar for every row, e.g. the upstream of a mean with g_scale = 1 / (B T); g_stride 1: per row).  With
 *   c[t, k] = w_k (1 - lambda (d_k - L[t])) (soft) or [k = stat[t]] (hard), recomputed from L and stat:
 *     dX[b, t] = (2 / F) g sum_k c[t, k] (X[b, t] - S[b, k])       (= (2 / F) g (X[b, t] - sum_k c S[b, k]), as sum_k c = 1)
 *     dS[b, k] = -(2 / F) sum_t g[b, t] c[t, k] (X[b, t] - S[b, k])
 *   dX: a workgroup per row tile, S streamed in ascending k; dS: a workgroup per tile of k, X[b] streamed in ascending t; each
 *   keeps its running sums in its own rows of the output.  dX or dS may be NULL (not both): that launch is skipped.  One or
 *   two launches, no workspace.
 * msmd_ordered_mean: out[0] = (sum of in[0 .. n)) / n; one workgroup, thread i adds elements i, i + 256, ... in double, then a
 *   halving tree over the 256 partial sums.
 *
 * NT-Xent, rows f = cat(a, b) (N = 2 B rows of D), fhat = f / max(|f|, 1e-12), s_ij = fhat_i . fhat_j / temperature,
 * p(i) = (i + B) mod N:  loss = (1 / N) sum_i [ log sum_{j != i} exp(s_ij) - s_{i p(i)} ].
 * msmd_nt_xent_forward: two launches, a workgroup per row: writes fhat (N, D), norm (N) = |f_i|, lse (N, 2) = the row's
 *   log-sum-exp as (max_j s_ij, log sum_j exp(s_ij - max)) and row_loss (N); the caller takes msmd_ordered_mean of row_loss.
 *   fhat, norm and lse are what the backward reads (N D + 3 N floats).
 * msmd_nt_xent_backward: upstream = the loss's 0-dim gradient on the device.  G_ij = upstream (exp((s_ij - max_i) - log_i) - [j = p(i)])
 *   / (N temperature) for j != i;  h_i = sum_j (G_ij + G_ji) fhat_j in ascending j;  grad[i] = (h_i - fhat_i (fhat_i . h_i)) /
 *   |f_i|, or h_i / 1e-12 where |f_i| < 1e-12 (the clamp passes no gradient to the norm).  grad (N, D): rows [0, B) belong to a,
 *   [B, N) to b.  One launch, a workgroup per row, no workspace.  B = 1 gives loss 0 and a zero gradient.
 *
 * Return codes: 0, a hipError_t of a failed launch, or 1 (hipErrorInvalidValue) before any launch for B, T, K, F or D < 1, a
 * grid beyond 2^31 - 1 workgroups, lambda < 0 or not finite, temperature <= 0 or not finite, g_stride outside {0, 1}, or a
 * NULL operand. */
#define MSMD_STYLE_ROWS 16
#define MSMD_STYLE_KTILE 64
#define MSMD_STYLE_FCHUNK 64
#define MSMD_NT_XENT_CHUNK 256 /* rows j per step of msmd_nt_xent_backward's coefficient table */
int msmd_style_adherence_forward(const float* X, const float* S, float* L, void* stat, int B, int T, int K, int F, float lambda,
                                 int soft, msmd_stream_t stream);
int msmd_style_adherence_backward(const float* X, const float* S, const float* L, const void* stat, const float* g,
                                  int g_stride, float g_scale, float* dX, float* dS, int B, int T, int K, int F, float lambda,
                                  int soft, msmd_stream_t stream);
int msmd_ordered_mean(const float* in, long n, float* out, msmd_stream_t stream);
int msmd_nt_xent_forward(const float* a, const float* b, float* fhat, float* norm, float* row_loss, float* lse, int B, int D,
                         float temperature, msmd_stream_t stream);
int msmd_nt_xent_backward(const float* fhat, const float* norm, const float* lse, const float* upstream, float* grad, int B,
                          int D, float temperature, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fourier resampling of motion tracks to the goal frame rate (reference dataset_processing/Step5_resample_and_assemble.py:
 * scipy.signal.resample per track; Step3_preprocess_expression_code.py: savgol_filter(code, 5, 2, axis=0)).
 *
 * msmd_track_resample: x (total_in, C) fp32, a ragged batch of clips laid end to end; y (total_out, C) fp32.
 *   in_offsets, out_offsets: (n_clips + 1) int32 prefix sums ON THE HOST, both starting at 0: clip i owns input frames
 *   [in_offsets[i], in_offsets[i + 1]) and output frames [out_offsets[i], out_offsets[i + 1]).  They are checked here and
 *   copied into the head of `ws` on the stream; the kernels read that copy.
 *   Per clip, with Nx input frames, num output frames, N = min(Nx, num), K = N / 2:
 *     X[k] = sum_n x[n] e^{-2 pi i k n / Nx}, k = 0 .. K;
 *     N even: X[K] is doubled for num < Nx, halved for num > Nx;
 *     y[m] = (1 / Nx) Re(X[0] + 2 sum_{k = 1 .. K} X[k] e^{+2 pi i k m / num}), where bin K enters once and by its real
 *     part alone when it is the output's own Nyquist bin (num even, K == num / 2): scipy.signal.resample on a real track.
 *   window != 0: x is read through a Savitzky-Golay filter along the frames, `savgol` = window * window doubles on the device
 *   laid out as msmd_headpose_smooth's `coeffs` (interior row, then the 2 (window / 2) edge rows, scipy's mode='interp');
 *   window odd, 3 <= window <= MSMD_HEADPOSE_MAX_WINDOW, every clip at least `window` frames.  window == 0: no filter, savgol
 *   may be NULL.
 *   Arithmetic: inputs widened to double, the twiddles cos / sin(2 pi r / P) tabulated per workgroup in double for the
 *   integer residue r = k n mod Nx (m k mod num) stepped exactly, sums in double in ascending n (k); the only fp32 rounding
 *   is the store of y.  A clip's bits depend on (Nx, num, window) and its own samples alone: no atomics, no cross-clip state.
 *   Two launches behind the copy of the offsets, whatever n_clips is: the analysis, a workgroup per (clip, MSMD_TRACK_ROWS
 *   bins, MSMD_TRACK_CH_TILE channels) with the (filtered) frames staged MSMD_TRACK_STAGE at a time, writes the scaled
 *   spectrum to `ws`; the synthesis, a workgroup per (clip, MSMD_TRACK_ROWS output frames, MSMD_TRACK_CH_TILE channels) with
 *   the bins staged MSMD_TRACK_STAGE at a time.
 *   ws: msmd_track_resample_ws_bytes(total_in, n_clips, C) bytes on the device, 16-byte aligned.
 * Returns 1 (hipErrorInvalidValue) before any launch for a NULL pointer, n_clips or C < 1, C > MSMD_TRACK_MAX_CHANNELS, a
 * window outside the above, offsets that do not start at 0, a clip of fewer than 1 (or `window`) or more than
 * MSMD_TRACK_MAX_FRAMES input or output frames; otherwise 0 or the hipError_t of the copy or a launch.
 * msmd_track_resample_ws_bytes returns 0 for arguments out of range. */
#define MSMD_TRACK_MAX_FRAMES 4096
#define MSMD_TRACK_ROWS 16
#define MSMD_TRACK_CH_TILE 16
#define MSMD_TRACK_STAGE 64
#define MSMD_TRACK_MAX_CHANNELS 1048560 /* 65535 tiles of MSMD_TRACK_CH_TILE: the channel tile is the grid's z index */
long msmd_track_resample_ws_bytes(long total_in, int n_clips, int C);
int msmd_track_resample(const float* x, const int* in_offsets, const int* out_offsets, int n_clips, int C, const double* savgol,
                        int window, void* ws, float* y, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Face crops for an expression encoder (reference dataset_processing/transform.py: crop_v2's cv2.warpAffine(INTER_LINEAR),
 * Step3_preprocess_expression_code.py: cvtColor(RGB2BGR), ToTensor + Normalize).
 *
 * msmd_face_crop, one launch for the batch: frames (F, H, W, 3 | 4) uint8 addressed as msmd_jpeg_coefficients addresses them
 *   (frame_stride / row_stride in bytes, pixel_stride 3 or 4; a 4th byte is never read); inverse (F, 2, 3) float64 on the
 *   device, the map from an OUTPUT pixel (column j, row i) to source coordinates; table (3, 256) fp32 on the device.
 *   Per output pixel, in float64 with every operation rounded on its own (no fused multiply-add):
 *     sx = ((a00 * j) + (a01 * i)) + a02, sy = ((a10 * j) + (a11 * i)) + a12;
 *     x0 = floor(sx), fx = sx - x0, y0 = floor(sy), fy = sy - y0;
 *     p(y, x) = the source byte for 0 <= x < W and 0 <= y < H, else 0 (a neighbour outside the frame is not clamped);
 *     v = ((p00 * (1 - fx) + p01 * fx) * (1 - fy)) + ((p10 * (1 - fx) + p11 * fx) * fy);   u8 = min(255, floor(v + 0.5));
 *     (sx, sy) outside (-1, W) x (-1, H), or not finite: u8 = 0, and no integer is formed from the coordinate.
 *   Output channel c reads source channel 2 - c when swap_rb is set, else c.
 *   out (F, 3, out_h, out_w) of out_dtype (MSMD_F32 / MSMD_BF16 / MSMD_F16), or NULL: table[c][u8], for the 16-bit types rounded to
 *   nearest even; crop_u8 (F, out_h, out_w, 3) uint8, or NULL: u8.  A lane owns four consecutive pixels of an output row
 *   and stores them as 16 (8) bytes per plane and 12 bytes of crop_u8 where out_w % 4 == 0 and the buffers are 16- (8-, 4-)
 *   byte aligned, element by element otherwise: the same bits.  A frame's bits depend on its own pixels and map alone.
 * Returns 1 (hipErrorInvalidValue) before the launch for a NULL frames / inverse / table, both outputs NULL, F < 1, H or W
 * outside [1, MSMD_JPEG_MAX_SIDE], out_h or out_w outside [1, MSMD_CROP_MAX_SIDE], pixel_stride not 3 or 4, strides under
 * which rows or frames would overlap, or an out_dtype other than the three; otherwise 0 or the launch's hipError_t. */
#define MSMD_CROP_MAX_SIDE 1024
int msmd_face_crop(const void* frames, long frame_stride, long row_stride, int pixel_stride, int F, int H, int W,
                   const double* inverse, const float* table, int out_h, int out_w, int swap_rb, void* out, int out_dtype,
                   void* crop_u8, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Expression code and jaw pose from model-space landmarks: a per-frame geometric fit of FLAME.
 *
 * The model.  Global, neck and eye rotations at identity, shape fixed per subject; expression e (NE), jaw axis-angle theta.
 *   R = Rodrigues(theta) in utils/lbs.py's convention (angle = |theta + 1e-8|, direction = theta / angle), M = R - I.
 *   Landmark k is l_k = X_k + M Y_k with X_k and Y_k (3 each) affine in [e | vec(M)]: six rows per landmark (X's three
 *   coordinates, then Y's) of NC = NE + 9 coefficients in `tab` (K, 6, NC) float64, and their constants in `tab0` (S, K, 6)
 *   float64, one set per subject (utils/expression_fit.reduce_flame builds both).
 * The objective, per frame: f(p) = sum_k w_k |l_k(p) - y_k|^2 + lambda_exp |e|^2 + lambda_jaw |theta|^2, p = [e | free theta];
 *   y = landmarks (n, K, 3) fp32, w (K) float64 >= 0, shared by the frames.  jaw_dof 0: theta = 0; 1: theta_x free; 3: all free.
 * The solver, Levenberg-Marquardt with fixed work:
 *   1. p = 0, mu = 1e-3.
 *   2. exactly `iterations` times: r and the analytic Jacobian Jm at p; H = Jm^T W Jm + D, g = Jm^T W r + D p (D the diagonal of
 *      the lambdas); solve (H + mu diag H) delta = -g over the free parameters by Cholesky; if f(p + delta) <= f(p): p += delta,
 *      mu = max(mu / 10, 1e-9); otherwise mu = 10 mu and p stays -- a rejected step uses up its iteration.  A pivot that is not
 *      positive counts as a rejection and sets status bit 1.
 *   3. no data-dependent exit; 4. a frame's result depends on nothing outside that frame.
 *   All of it in float64; the products with W are formed as (sqrt(w) Jm)^T (sqrt(w) Jm).
 * subject (n) int32 selects tab0's set per frame; the kernel clamps it into [0, S).
 * Outputs, fp32: code (n, NE) = e; jaw (n, 3) = theta (locked components 0); rms (n) = sqrt(sum_k w_k |r_k|^2 / sum_k w_k) at the
 *   returned p; status (n) int32: bit 0 = a non-finite landmark in the frame (its code, jaw and rms are NaN, status exactly 1, and
 *   no other frame is touched), bit 1 = a factorisation was refused, the rest zero.
 * One wave per frame, MSMD_EXPFIT_FRAMES frames per workgroup; no atomics, no host synchronisation.
 * Returns 1 before the launch for a NULL pointer, n < 1, K outside [1, MSMD_EXPFIT_MAX_LANDMARKS], NE outside
 * [1, MSMD_EXPFIT_MAX_EXP], S < 1, jaw_dof not 0 / 1 / 3, iterations outside [0, MSMD_EXPFIT_MAX_ITERATIONS], a lambda that is
 * negative or NaN; otherwise 0 or the launch's hipError_t. */
#define MSMD_EXPFIT_MAX_LANDMARKS 128
#define MSMD_EXPFIT_MAX_EXP 61 /* NE + 3 jaw parameters <= 64: one parameter per lane of a wave */
#define MSMD_EXPFIT_MAX_ITERATIONS 64
#define MSMD_EXPFIT_FRAMES 4
int msmd_expression_fit(const float* landmarks, const int* subject, const double* tab, const double* tab0, const double* w,
                        float* code, float* jaw, float* rms, int* status, int n, int K, int NE, int S, int jaw_dof,
                        int iterations, double lambda_exp, double lambda_jaw, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Vertex-space evaluation of a predicted mesh sequence against the ground truth: what the lip vertex error,
 * the upper-face dynamics deviation and the mean / maximum / RMS vertex error are reduced from (utils/metrics.py).
 * pred, gt (n, V, 3) contiguous, both MSMD_F32 or both MSMD_F16; a stored value enters as its exact float64 image and every
 * operation after that is a float64 one rounded on its own (no fused multiply-add).  No floating-point atomics.
 *
 * msmd_vertex_frame_errors: region (V) bytes, bit 0 = lip vertex (bit 1 = upper-face vertex, not read here); out (n, 4) float64.
 *   Per vertex d2 = ((dx dx + dy dy) + dz dz) of the differences pred - gt.  Row f of out:
 *     [0] max over the lip vertices of d2 (0 when region marks none)   [1] sum over all vertices of sqrt(d2)
 *     [2] max over all vertices of sqrt(d2)                            [3] sum over all vertices of d2
 *   The maxima are numpy's: a NaN operand is the result.  So a column is NaN exactly when a vertex that contributes to it has
 *   a NaN difference (inf - inf is one), and a NaN at a vertex off the lips leaves column 0 finite.
 *   One workgroup of 256 per frame; thread t folds vertices t, t + 256, ... in ascending order, the lanes of a wave are joined by
 *   the xor butterfly 32 .. 1 and the four waves in wave order: an order that depends on V alone, never on n.
 *
 * msmd_vertex_motion_moments: the running moments over a clip's frames of m = |v - template|^2 (same parenthesisation) at every
 *   upper-face vertex, for pred and for gt.  pred, gt: the n_chunk frames [frame0, frame0 + n_chunk) of a sequence of clips laid
 *   end to end; clip_offsets (n_clips + 1) int64 on the device, over the WHOLE sequence; upper_idx (U) int32, ascending, clamped
 *   into [0, V) by the kernel; tmpl (V, 3) fp32, or (n_clips, V, 3) with template_per_clip != 0.
 *   state (n_clips, U, 2, 3) float64, [track: 0 pred, 1 gt][count, mean, M2]; the caller zeroes it before the first chunk.
 *   Welford's recurrence per frame:  count += 1;  delta = m - mean;  mean += delta / count;  M2 += delta * (m - mean).
 *   One thread owns one (clip, u, track): it reads the state, walks the clip's frames that fall inside the chunk in frame order, and
 *   writes the state back (the other threads of its workgroup only load vertices and leave m in LDS for it); a clip with no frame
 *   in the chunk is not touched.  The order is the frame order however the sequence is cut, so the state after the last chunk
 *   holds the same bits for every cut.  A frame is counted once if the chunks of
 *   successive calls tile the sequence; that is the caller's to keep.
 * Both return 1 (hipErrorInvalidValue) before the launch for n or n_chunk < 0, frame0 < 0, V < 1, U < 1, n_clips < 1, a dtype
 * other than the two, or a NULL pointer with work to do; n = 0 / n_chunk = 0 returns 0 and launches nothing. */
int msmd_vertex_frame_errors(const void* pred, const void* gt, const unsigned char* region, double* out, int n, int V, int dtype,
                             msmd_stream_t stream);
int msmd_vertex_motion_moments(const void* pred, const void* gt, long frame0, int n_chunk, const long* clip_offsets, int n_clips,
                               const int* upper_idx, int U, const float* tmpl, int template_per_clip, double* state, int V,
                               int dtype, msmd_stream_t stream);

/* The error FIELD of the same pair of sequences, and its colours.  Same loads and float64 conventions: per vertex
 * d = sqrt(d2), d2 as above.  A colour table `lut` is (256, 4) uint8 RGBA, 4-byte aligned, as is every colour output.
 * The colour rule, ONE device function for both colour entry points: t = x / vmax; a NaN t stores the four bytes of nan_color
 *   (R | G << 8 | B << 16 | A << 24); otherwise idx = (t >= 1.0) ? 255 : (int)floor(t * 255.0 + 0.5) (so +inf maps to 255; a t <= 0,
 *   which a distance never gives, to 0) and the four bytes of lut[idx] are stored.
 * msmd_vertex_error_colors: out (n, V, 4) uint8 = the rule at x = d.  The distance is never stored.
 * msmd_colormap_f64: x (N) float64 -> out (N, 4) uint8 = the rule at x; it colours the time-mean map sum / F.
 * msmd_vertex_error_sums: the running per-clip, per-vertex sum of d.  state (n_clips, V) float64, zeroed by the caller; pred, gt,
 *   frame0, n_chunk and clip_offsets as msmd_vertex_motion_moments takes them.  One thread owns one (clip, vertex): it reads its sum,
 *   adds the d of the clip's frames that fall inside the chunk in frame order, and writes it back; a clip with no frame in the chunk
 *   is not touched.  So the state after the last chunk holds the same bits however the sequence is cut and whatever the other
 *   clips hold.  NaN propagates.
 * All three return 1 (hipErrorInvalidValue) before the launch for a vmax that is not finite or not > 0, for the arguments the two
 * entry points above refuse (n, n_chunk or N < 0, frame0 < 0, V < 1, n_clips < 1, a dtype other than the two, a NULL pointer with
 * work to do) and for a misaligned lut / out; n = 0 / n_chunk = 0 / N = 0 returns 0 and launches nothing. */
int msmd_vertex_error_colors(const void* pred, const void* gt, const unsigned char* lut, unsigned char* out, int n, int V, int dtype,
                             double vmax, unsigned nan_color, msmd_stream_t stream);
int msmd_vertex_error_sums(const void* pred, const void* gt, long frame0, int n_chunk, const long* clip_offsets, int n_clips,
                           double* state, int V, int dtype, msmd_stream_t stream);
int msmd_colormap_f64(const double* x, const unsigned char* lut, unsigned char* out, long N, double vmax, unsigned nan_color,
                      msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Frame resizing: separable fixed-point resampling of 8-bit frames.  The operator is Pillow's
 * Image.resize for 8-bit images: integer arithmetic on the device, coefficient tables built in float64 on the host
 * (ops.resize_tables).  No floating point in the kernels; the bytes are a pure function of the source bytes and the tables.
 *
 * One axis is described by `bounds` (T, n_out, 2) int32 = (first source sample, number of taps) and `coef` (T, n_out, ksize)
 * int32, the weights in units of 2^-22; T tables, and table_of_frame (N) int32 names the table of each frame for BOTH axes'
 * table sets (so Tx == Ty is the caller's to keep; the kernels clamp the index into each set).  One 1-D pass:
 *   out = clip((2^21 + sum_{i < taps} in[first + i] * coef[i]) >> 22, 0, 255), int32 accumulator, arithmetic shift.
 * A frame is the horizontal pass over every source row, rounded to uint8 as above, then the vertical pass over that result.
 * A pass that changes nothing is an identity table (first = o, taps = 1, coef = 2^22): the same bytes as no pass.
 * Every index read from a table is clamped before use: first into [0, n_in - 1], taps into [0, min(ksize, n_in - first)],
 * table_of_frame into [0, T - 1].  So no table can take a load outside the source, and the result for such a table is the
 * operator on the clamped table.
 *
 * msmd_resize_u8: src (N, Hs, Ws, C) uint8, C in {1, 3, 4}, addressed by frame_stride / row_stride in bytes and pixel_stride
 *   (1 for C = 1; 3 or 4 for C = 3, a 4th byte is never read; 4 for C = 4), any byte alignment.  dst (N, Hd, Wd, C) contiguous.
 *   form MSMD_RESIZE_TWO_PASS: a horizontal launch into workspace (N, Hs, Wd, C) uint8, then a vertical launch; any sizes.
 *   form MSMD_RESIZE_FUSED: one launch.  A workgroup owns MSMD_RESIZE_TILE_H output rows by MSMD_RESIZE_TILE_W output columns,
 *     runs the horizontal pass for the source rows its vertical taps touch into LDS (uint8, rows padded by one word), then
 *     the vertical pass from LDS.  rows_span is the caller's bound on the source rows one tile touches (the largest, over
 *     the tiles of MSMD_RESIZE_TILE_H consecutive output rows and over the tables, of max(first + taps) - min(first)); the
 *     kernel keeps that many rows and clamps a row index beyond them, so a wrong bound gives wrong bytes, never a wild access.
 *   form MSMD_RESIZE_AUTO: msmd_resize_route chooses.
 *   Output words are stored four bytes at a time where Wd * C % 4 == 0 and the buffer is 4-byte aligned, byte by byte
 *   otherwise; 4-byte source pixels of a 4-channel frame are loaded as words where src and its strides allow: the same bytes.
 * msmd_resize_fits: 1 when C is in {1, 3, 4}, 1 <= rows_span and rows_span * (MSMD_RESIZE_TILE_W * C + 4) <= MSMD_RESIZE_LDS_BYTES: the
 *   fused form can run; else 0.
 * msmd_resize_route: the form MSMD_RESIZE_AUTO takes.  MSMD_RESIZE_TWO_PASS where the fused form does not fit, and also where both
 *   of these hold (measured): the tiles' overlap makes the fused form repeat more than one horizontal
 *   multiply-add per intermediate byte, (rows_span * ceil(Hd / MSMD_RESIZE_TILE_H) - Hs) * kx > Hs, and the two-pass form's
 *   intermediate stays in the last-level cache, N * Hs * Wd * C <= MSMD_RESIZE_CACHE_BYTES.  Else MSMD_RESIZE_FUSED.
 *   Both are host functions: nothing is launched.
 * msmd_resize_u8 returns 1 (hipErrorInvalidValue) before any launch for N < 0, a C outside {1, 3, 4}, a pixel_stride that
 * does not go with C, Hs / Ws / Hd / Wd outside [1, MSMD_JPEG_MAX_SIDE], kx / ky / Tx / Ty < 1, strides under which rows or frames
 * would overlap, a form outside the three, the fused form asked for where msmd_resize_fits refuses it, or, with work to
 * do, a NULL pointer or the two-pass form without a workspace; N = 0 passes those checks, returns 0, looks at no pointer (the
 * workspace included) and writes nothing; otherwise 0 or the launch's hipError_t. */
#define MSMD_RESIZE_AUTO 0
#define MSMD_RESIZE_FUSED 1
#define MSMD_RESIZE_TWO_PASS 2
#define MSMD_RESIZE_TILE_H 32
#define MSMD_RESIZE_TILE_W 64
#define MSMD_RESIZE_LDS_BYTES 65536
#define MSMD_RESIZE_PRECISION_BITS 22
#define MSMD_RESIZE_CACHE_BYTES 134217728
int msmd_resize_fits(int C, int rows_span);
int msmd_resize_route(int C, int rows_span, int N, int Hs, int Hd, int Wd, int kx);
int msmd_resize_u8(const void* src, long frame_stride, long row_stride, int pixel_stride, int N, int Hs, int Ws, int C,
                   const int* xbounds, const int* xcoef, int kx, int Tx, const int* ybounds, const int* ycoef, int ky, int Ty,
                   const int* table_of_frame, void* dst, int Hd, int Wd, void* workspace, int rows_span, int form,
                   msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Overlays: 2-D primitives drawn onto 8-bit frames that are already on the device.  Integer arithmetic
 * throughout; the bytes are a pure function of the source bytes, the records and the font table.
 *
 * Coordinates are int32 in units of 1/16 pixel: pixel (column j, row i) covers [16 j, 16 j + 16) x [16 i, 16 i + 16).  The sample
 * points of a pixel are its corner (16 j, 16 i) plus the offset (8, 8) for samples = 1, and plus the 4 x 4 grid of offsets
 * {2, 6, 10, 14} in each axis for samples = 16.
 *
 * prims (P, 8) int32, one record = [kind, x0, y0, x1, y1, r, aux, colour], colour = R | G << 8 | B << 16 | A << 24.
 * prim_offsets (N + 1) int32: frame f draws the records [off[f], off[f + 1]) in that order; the kernel clamps both ends into
 * [0, P] and makes the end no less than the begin, so a bad table gives wrong pictures, never a load outside prims.
 * With p a sample point and q = p - (x0, y0), p is inside a record of
 *   MSMD_OVERLAY_NONE (0)     never: padding;
 *   MSMD_OVERLAY_DISC (1)     iff aux^2 <= |q|^2 <= r^2: a filled disc for aux = 0, else a ring of inner radius aux;
 *   MSMD_OVERLAY_CAPSULE (2)  the segment a = (x0, y0) -> b = (x1, y1) of half-width r with round caps, decided without a
 *                             division: d = b - a, L = d.d, s = q.d; s <= 0: iff |q|^2 <= r^2; s >= L: iff |p - b|^2 <= r^2;
 *                             otherwise iff (qx dy - qy dx)^2 <= r^2 L, compared on 128-bit products (the left side reaches 2^86
 *                             at the coordinate limits); a = b is the disc;
 *   MSMD_OVERLAY_BOX (3)      iff x0 <= px <= x1 and y0 <= py <= y1 and, for aux > 0, NOT (x0 + aux <= px <= x1 - aux and
 *                             y0 + aux <= py <= y1 - aux): an outline of thickness aux drawn inwards, filled for aux = 0;
 *   MSMD_OVERLAY_GLYPH (4)    one character: font (n_glyphs, 8) uint8, row v of a glyph is one byte, bit 7 - u set = font pixel
 *                             (u, v) is ink; x1 is the side of a font pixel in 1/16 px, y1 the glyph index; u = (px - x0) div x1,
 *                             v = (py - y0) div x1 (floor division); iff 0 <= u, v < 8 and the bit is set.
 * A record draws nothing if its kind is outside 0 .. 4; if x0 or y0, or for the kinds 1 .. 3 x1 or y1, lies outside
 * +-MSMD_OVERLAY_MAX_COORD; if r or aux lies outside [0, MSMD_OVERLAY_MAX_RADIUS]; or if it is a glyph with y1 outside
 * [0, n_glyphs) or x1 outside [1, MSMD_OVERLAY_MAX_RADIUS].
 *
 * Blend: for each record in list order and each pixel, cov = the number of the pixel's sample points inside the record,
 * w = cov * (16 / samples) * A, and every written channel with destination byte d and colour byte c becomes
 *   d <- (d * (4080 - w) + c * w + 2040) div 4080.
 * C = 1 takes colour byte 0; C = 3 and C = 4 take colour bytes 0 .. 2 into channels 0 .. 2 in memory order (RGB or BGR is the
 * caller's business); the fourth byte of a 4-channel pixel is never read or written.
 *
 * msmd_draw_overlay: src, dst (N, H, W, C) uint8, C in {1, 3, 4}, both addressed by frame_stride / row_stride in bytes and
 *   pixel_stride (1 for C = 1; 3 or 4 for C = 3; 4 for C = 4), any byte alignment.  src == dst draws in place; otherwise the two
 *   must not overlap (the caller's to keep) and dst receives every pixel, drawn on or not.  One launch: a workgroup of 256
 *   threads owns MSMD_OVERLAY_TILE_W x MSMD_OVERLAY_TILE_H pixels of one frame, four horizontally adjacent pixels per thread;
 *   per MSMD_OVERLAY_CHUNK records it tests each record's bounding box against the tile, compacts the hits in order into LDS
 *   and every pixel walks that list.  Pixels are loaded once and stored once; a tile no record touches writes nothing in place
 *   and copies otherwise.  Pixels go as whole words where C = pixel_stride is 1 or 3 and both buffers and both strides are
 *   4-byte aligned, byte by byte otherwise: the same bytes.  No allocation, no host synchronisation.
 * Returns 1 (hipErrorInvalidValue) before any launch for N < 0 or n_prims < 0, a C outside {1, 3, 4}, a pixel_stride that does
 * not go with C, H or W outside [1, MSMD_JPEG_MAX_SIDE], strides under which rows or frames would overlap, samples outside
 * {1, 16}, n_glyphs < 0, or, with work to do, a NULL src, dst or prim_offsets, NULL prims with n_prims > 0 or NULL font with
 * n_glyphs > 0; N = 0 passes those checks, returns 0, looks at no pointer and writes nothing; otherwise 0 or the launch's
 * hipError_t. */
#define MSMD_OVERLAY_NONE 0
#define MSMD_OVERLAY_DISC 1
#define MSMD_OVERLAY_CAPSULE 2
#define MSMD_OVERLAY_BOX 3
#define MSMD_OVERLAY_GLYPH 4
#define MSMD_OVERLAY_TILE_W 64
#define MSMD_OVERLAY_TILE_H 16
#define MSMD_OVERLAY_CHUNK 256
#define MSMD_OVERLAY_MAX_COORD (1 << 20)
#define MSMD_OVERLAY_MAX_RADIUS (1 << 16)
int msmd_draw_overlay(const void* src, void* dst, long frame_stride, long row_stride, int pixel_stride, int N, int H, int W, int C,
                      const int* prims, long n_prims, const int* prim_offsets, const unsigned char* font, int n_glyphs,
                      int samples, msmd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Retargeting: FLAME motion onto a blendshape rig, a bounded least-squares fit per frame.
 *
 * The rig: neutral (V, 3) fp32; deltas (K, V, 3) fp32, 1 <= K <= MSMD_RETARGET_MAX_SHAPES; vertex_weight (V) fp32 >= 0 (absent: 1);
 * lo < hi (K) float64 (absent: 0 and 1); ridge (K) float64 >= 0 (absent: 0).  Every sum below reads these stored arrays.
 *   A[k, v, c] = fl32(vertex_weight[v] * deltas[k, v, c])      (utils/retarget.prepare_rig forms it, once per rig)
 *   G = A A^T over the 3 V coordinates, float64;  H = G + diag(ridge), which must be positive definite (prepare_rig checks it).
 * Per frame n with vertices x (V, 3) fp32:
 *   b[n, k] = sum_{v, c} A[k, v, c] * fl32(x[n, v, c] - neutral[v, c]): the difference is rounded to fp32 first; products and
 *     sums are fp32.  A vertex with vertex_weight == 0 is not part of the sum and is never read: a NaN there does not reach b.
 *   w[n] = argmin 1/2 w^T H w - b[n]^T w  subject to lo <= w <= hi, solved in float64 and rounded once to fp32.
 *
 * msmd_retarget_gram: G and H (K, K) float64 from A (K, V, 3).  ridge is a HOST array of K doubles or NULL.  One workgroup of 256
 *   per pair (k, l <= k): thread t adds the exact products of coordinates t, t + 256, ... in ascending order, then the 256 sums
 *   fold in halves (t += t + 128, 64, ... 1).  The order depends on V alone.
 * msmd_retarget_rhs: b (N, K) fp32.  A workgroup owns MSMD_RETARGET_FRAME_TILE frames and one contraction split of
 *   MSMD_RETARGET_SPLIT_VERTICES vertices, which it walks MSMD_RETARGET_VERTEX_TILE vertices at a time on v_mfma_f32_16x16x4_f32; its
 *   sums go to partial (msmd_retarget_splits(V), N, K) fp32, the caller's workspace, and a second launch adds a frame's splits in
 *   ascending order.  The split is a constant, so a frame's bits depend on V, K and the frame alone: not on N, not on the
 *   frame's place in the batch, not on the run.  vertex_weight (V) or NULL (every vertex is read).
 * msmd_retarget_solve: block principal pivoting for a box, float64, one wave per frame, MSMD_RETARGET_SOLVE_FRAMES frames per
 *   workgroup, frames independent.  lo, hi are HOST arrays of K doubles or NULL (0 and 1).  Every weight is at lo (L), free (F) or
 *   at hi (U); all start in L.  One iteration:
 *     1. the L and U weights take their bounds;  2. H_FF w_F = b_F - H_F,L lo_L - H_F,U hi_U by Cholesky (the rows and columns
 *     of the bound weights pinned to the identity);  3. g = H w - b;  4. a weight is infeasible if it is F with w < lo (-> L), F
 *     with w > hi (-> U), L with g < 0 (-> F) or U with g > 0 (-> F);  5. none infeasible: done;  6. otherwise, if the
 *     infeasible count is below every count seen so far, the budget p is reset to 3 and all infeasible weights are exchanged;
 *     else if p > 0, p -= 1 and all are exchanged; else only the infeasible weight of the largest index is exchanged.
 *   Outputs: w (N, K) fp32; iterations (N) int32; status (N) int32: MSMD_RETARGET_CONVERGED; MSMD_RETARGET_CAP_REACHED (the
 *   output is the iterate of iteration max_iterations clipped to the box); MSMD_RETARGET_BAD_INPUT (b not finite: the frame's
 *   weights are NaN, 0 iterations); MSMD_RETARGET_NOT_POSITIVE (a pivot was not positive, which a positive definite H never
 *   gives: weights NaN).
 * msmd_blendshape_apply: out[n, v, c] = neutral[v, c] + sum_k w[n, k] * deltas[k, v, c], (N, V, 3) fp32: an fmaf chain that starts at
 *   neutral and takes k in ascending order.  A thread owns one coordinate of MSMD_RETARGET_APPLY_FRAMES frames.
 * All four return 1 (hipErrorInvalidValue) before any launch for N < 0, K outside [1, MSMD_RETARGET_MAX_SHAPES], V outside
 * [1, MSMD_RETARGET_MAX_VERTICES], a ridge that is negative or NaN, lo >= hi or a bound that is not finite, max_iterations outside
 * [1, MSMD_RETARGET_MAX_ITERATIONS], N above 65535 * MSMD_RETARGET_APPLY_FRAMES for the apply, or, with work to do, a NULL pointer
 * other than the optional ones; N = 0 passes those checks, returns 0 and launches nothing; otherwise 0 or the launch's
 * hipError_t.  msmd_retarget_splits is a host function: ceil(V / MSMD_RETARGET_SPLIT_VERTICES), 0 for V < 1. */
#define MSMD_RETARGET_MAX_SHAPES 64
#define MSMD_RETARGET_MAX_VERTICES (1 << 24)
#define MSMD_RETARGET_FRAME_TILE 128
#define MSMD_RETARGET_VERTEX_TILE 32
#define MSMD_RETARGET_SPLIT_VERTICES 1024
#define MSMD_RETARGET_SOLVE_FRAMES 4
#define MSMD_RETARGET_APPLY_FRAMES 32
#define MSMD_RETARGET_ITERATIONS 256 /* the default cap */
#define MSMD_RETARGET_MAX_ITERATIONS 65536
#define MSMD_RETARGET_CONVERGED 0
#define MSMD_RETARGET_CAP_REACHED 1
#define MSMD_RETARGET_BAD_INPUT 2
#define MSMD_RETARGET_NOT_POSITIVE 3
int msmd_retarget_splits(int V);
int msmd_retarget_gram(const float* A, const double* ridge, double* G, double* H, int K, int V, msmd_stream_t stream);
int msmd_retarget_rhs(const float* x, const float* neutral, const float* A, const float* vertex_weight, float* partial, float* b,
                      int N, int V, int K, msmd_stream_t stream);
int msmd_retarget_solve(const double* H, const float* b, const double* lo, const double* hi, float* w, int* status,
                        int* iterations, int N, int K, int max_iterations, msmd_stream_t stream);
int msmd_blendshape_apply(const float* w, const float* neutral, const float* deltas, float* out, int N, int V, int K,
                          msmd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MSMD_HIP_H */
