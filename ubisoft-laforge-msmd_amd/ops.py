"""Tensor-level shims over the C ABI (include/msmd_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator, so no
hipMalloc in steady state) and the current HIP stream; every op below hands raw
device pointers + sizes to a hand-written gfx950 kernel.  All ops launch on
``torch.cuda.current_stream()`` and never synchronise, so sequences of them can
be captured in a hipGraph (torch.cuda.CUDAGraph).
"""
from __future__ import annotations

import ctypes
import functools
import math
import os

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib

_HEADER = _lib.parse_constants()   # the #define MSMD_<NAME> lines of include/msmd_hip.h: no constant of the C ABI is typed again here


def _h(*names):
    """The header's MSMD_<name> values: one int for one name, a tuple for several."""
    vals = tuple(_HEADER["MSMD_" + n] for n in names)
    return vals if len(vals) > 1 else vals[0]


F32, BF16, F16, F16X2 = _h("F32", "BF16", "F16", "F16X2")
SPLIT = "f16x2"   # dtype token of the parity-grade speed mode (MSMD_F16X2 split storage, include/msmd_hip.h)


class Split:
    """A tensor in MSMD_F16X2 split storage: logical shape (..., C) fp32-grade values, physically `.t` = (..., 2 C)
    fp16 in 32-element blocks [hi x 32 | lo x 32] (x ~= hi + lo / 2048).  Only what the call sites need: logical shape /
    strides, slicing (last-dim slices on multiples of 32), the device pointer.  `.float()` converts back."""
    __slots__ = ("t", "below_32")
    dtype = SPLIT
    is_cuda = True

    def __init__(self, t, below_32=False):
        if t.dtype != torch.float16 or t.shape[-1] % 64 or t.stride(-1) != 1:
            raise TypeError("Split wraps an fp16 tensor whose last dim is 2 x (a multiple of 32)")
        self.t = t
        self.below_32 = below_32    # every |value| < 32, checked once by split_weight(): lets gemm() pass MSMD_GEMM_W_BELOW_32

    @property
    def shape(self):
        return torch.Size((*self.t.shape[:-1], self.t.shape[-1] // 2))

    @property
    def device(self):
        return self.t.device

    def dim(self):
        return self.t.dim()

    def numel(self):
        return self.t.numel() // 2

    def stride(self, i):
        i = i % self.t.dim()
        return 1 if i == self.t.dim() - 1 else self.t.stride(i) // 2

    def data_ptr(self):
        return self.t.data_ptr()

    def is_contiguous(self):
        return self.t.is_contiguous()

    def __getitem__(self, idx):
        if not isinstance(idx, tuple):
            idx = (idx,)
        if Ellipsis in idx:
            k = idx.index(Ellipsis)
            idx = idx[:k] + (slice(None),) * (self.t.dim() - (len(idx) - 1)) + idx[k + 1:]
        if len(idx) == self.t.dim():
            last = idx[-1]
            if not isinstance(last, slice) or last.step not in (None, 1):
                raise IndexError("Split: only contiguous slices along the last dim")
            C = self.shape[-1]
            a, b, _ = last.indices(C)
            if a % 32 or (b % 32 and b != C):
                raise IndexError("Split: last-dim slices must fall on multiples of 32")
            idx = idx[:-1] + (slice(2 * a, 2 * b),)
        return Split(self.t[idx], self.below_32)

    def view(self, *shape):
        shape = shape[0] if len(shape) == 1 and not isinstance(shape[0], int) else shape
        return Split(self.t.view(*shape[:-1], 2 * shape[-1]), self.below_32)

    reshape = view

    def float(self):
        return unsplit(self)


def empty(shape, device, dtype):
    """torch.empty that understands the SPLIT token (last dim must then be a multiple of 32)."""
    if dtype == SPLIT:
        if shape[-1] % 32:
            raise ValueError("split storage needs a last dim that is a multiple of 32")
        return Split(torch.empty(*shape[:-1], 2 * shape[-1], device=device, dtype=torch.float16))
    return torch.empty(*shape, device=device, dtype=dtype)


def to_split(x, cols_out=None):
    """fp32 (..., C) -> Split (..., cols_out) (zero-padded to a multiple of 32); rows may be strided (last dim
    contiguous, uniform row stride)."""
    if isinstance(x, Split):
        return x
    _need_cuda(x)
    if x.dtype != torch.float32:
        x = x.float()
    C = x.shape[-1]
    cols_out = (C + 31) // 32 * 32 if cols_out is None else cols_out
    if not x.is_contiguous():
        x = x.contiguous()
    rows = x.numel() // C
    out = torch.empty(*x.shape[:-1], 2 * cols_out, device=x.device, dtype=torch.float16)
    _lib.check(_lib.load().msmd_split_f16x2(_p(x), _p(out), rows, C, C, cols_out, _stream()), "msmd_split_f16x2")
    return Split(out)


def split_weight(w):
    """to_split for a WEIGHT (packed once at load): also records whether every |w| < 32, which gemm() hands to the library as
    MSMD_GEMM_W_BELOW_32 (include/msmd_hip.h).  One host sync per weight, at pack time only."""
    s = to_split(w.float().contiguous())
    s.below_32 = bool(w.numel() == 0 or float(w.detach().abs().max()) < 31.99)   # RN_f16(31.99) = 31.984375 = 65504 / 2^11
    return s


def unsplit(s, cols=None):
    C = s.shape[-1]
    cols = C if cols is None else cols
    t = s.t if s.t.is_contiguous() else s.t.contiguous()
    rows = t.numel() // (2 * C)
    out = torch.empty(*s.shape[:-1], cols, device=t.device, dtype=torch.float32)
    _lib.check(_lib.load().msmd_unsplit_f16x2(_p(t), _p(out), rows, cols, C, cols, _stream()), "msmd_unsplit_f16x2")
    return out
ACT_NONE, ACT_GELU, ACT_ELU = _h("ACT_NONE", "ACT_GELU", "ACT_ELU")
CONV0_SPLITS = _h("CONV0_SPLITS")

# Optional per-launch timing of the dominant kernel (bench.py roofline leg): when a list is installed
# here, every msmd_gemm launch is bracketed by HIP events recorded on the launch stream.
GEMM_TRACE = None
# Optional FLOP counter (bench.py sampler leg): a one-element list that every msmd_gemm call adds 2 M N K batch to.
GEMM_FLOPS = None


def _dt(t: torch.Tensor) -> int:
    if t.dtype == SPLIT:
        return F16X2
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if isinstance(t, Split):
            t = t.t
        if t is not None and not t.is_cuda:
            raise RuntimeError("msmd_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")


# Host-side GEMM autotune: the first call of a (shape, epilogue) key times the LDS-DMA kernel variants on the real
# operands (all variants are bit-identical in their results) and remembers the winner; later calls pass it as a hint
# in bits 8-15 of `act`.  Never runs during hipGraph capture (it synchronises).  Opt-in (MSMD_GEMM_AUTOTUNE=1): on the
# bench workload the library's shape heuristic is within run-to-run noise of the tuned choice (5.20 vs 5.22 ms/step).
GEMM_AUTOTUNE = os.environ.get("MSMD_GEMM_AUTOTUNE", "0") == "1"
_TUNE_MIN_FLOP = 1.0e9
_TUNE_CANDIDATES = (17, 13, 9, 12)
_TUNED = {}
# Per-call GEMM knobs (include/msmd_hip.h: MSMD_GEMM_VARIANT / _WRITE_THROUGH / _PAIRED_STORES).  The C library has no
# global state; these module-level defaults are what `gemm()` passes when the caller gives none (`gemm_defaults`
# scopes a change, e.g. while a hipGraph is captured -- the choice is then baked into that graph).
GEMM_WRITE_THROUGH, GEMM_PAIRED_STORES, GEMM_STAGGER = _h("GEMM_WRITE_THROUGH", "GEMM_PAIRED_STORES", "GEMM_STAGGER")
GEMM_ONE_TILE_PER_WORKGROUP = _h("GEMM_ONE_TILE_PER_WORKGROUP")      # opt out of the persistent form of multi-round launches (A/B; same bits)
GEMM_NO_256_TILE = _h("GEMM_NO_256_TILE")     # opt out of the 256 x 256 8-phase kernel where the library would pick it (A/B; plain outputs same bits)
GEMM_W_BELOW_32 = _h("GEMM_W_BELOW_32")       # split operands: |W| < 32 everywhere (set by gemm() from Split.below_32)
GEMM_NO_160_ROW_TILE = _h("GEMM_NO_160_ROW_TILE")           # gemm_ln: opt out of the 160 x 128 member of variant 17 (A/B; same bits)
GEMM_FORCE_160_ROW_TILE = _h("GEMM_FORCE_160_ROW_TILE")     # gemm_ln: the 160 x 128 member wherever its kernel takes the call (tests, scans; same bits)
GEMM_LN_FLAGS = 0              # extra `act` bits msmd_gemm_ln calls carry (A/B hook: GEMM_ONE_TILE_PER_WORKGROUP)
GEMM_LN_ROUTER = None          # optional (M, N, K) -> 15 | 17 | 18 | None: tile hint for msmd_gemm_ln's big-tile family
GEMM_LN_ALL_IN_ONE = False     # A/B hook (tools/ab_forward.py): msmd_gemm_ln on the one-kernel-with-every-epilogue form (variant 66)


class capture_guard:
    """Around every hipGraph stream capture of this package: collect garbage first and keep Python's cyclic collector off for
    the duration.  A collection that starts INSIDE a capture runs the destructors of whatever earlier code left in reference
    cycles -- captured graphs, events, communicators: device-runtime calls that are not permitted while a stream is capturing --
    and the process aborts (seen as a rare `Fatal Python error: Aborted ... Garbage-collecting` under the segmented training
    capture, round 4).  torch.cuda.graph() collects at entry too, but does not hold the collector off."""

    def __enter__(self):
        import gc
        gc.collect()
        self.was = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self.was:
            gc.enable()
        return False
# attention launches also pull the layer's remaining weights through the memory-side cache (msmd_attention_prefetch)
PREFETCH_WEIGHTS = os.environ.get("MSMD_PREFETCH", "1") != "0"
# transformer blocks: LayerNorm folded into the neighbouring GEMMs (gemm_ln); False (MSMD_FOLD_LN=0) = LayerNorm kernels
FOLD_LN = os.environ.get("MSMD_FOLD_LN", "1") != "0"
GEMM_ROUTER = None   # developer hook (tools/ab_forward.py): callable (M, N, K, batch) -> variant or None, consulted per call
_GEMM_DEFAULT = {"variant": 0, "flags": GEMM_PAIRED_STORES, "split_variant": 0}   # paired 16-byte stores: -1 % on the forward step
if os.environ.get("MSMD_GEMM_ONE_TILE", "0") == "1":      # developers' A/B switch (tools/ab_env.sh): every launch in the one-tile-per-workgroup form
    _GEMM_DEFAULT["flags"] |= GEMM_ONE_TILE_PER_WORKGROUP
    GEMM_LN_FLAGS = GEMM_ONE_TILE_PER_WORKGROUP


if os.environ.get("MSMD_GEMM_NO_256", "0") == "1":        # developers' A/B switch: no launch on the 256 x 256 kernel
    _GEMM_DEFAULT["flags"] |= GEMM_NO_256_TILE
    GEMM_LN_FLAGS |= GEMM_NO_256_TILE


class gemm_defaults:
    """with ops.gemm_defaults(variant=13, flags=ops.GEMM_WRITE_THROUGH): ...   (None = leave as is)"""

    def __init__(self, variant=None, flags=None, split_variant=None):
        self.new = {k: v for k, v in (("variant", variant), ("flags", flags), ("split_variant", split_variant))
                    if v is not None}

    def __enter__(self):
        self.old = dict(_GEMM_DEFAULT)
        _GEMM_DEFAULT.update(self.new)
        return self

    def __exit__(self, *exc):
        _GEMM_DEFAULT.clear()
        _GEMM_DEFAULT.update(self.old)
        return False


def _trace_begin(M, N, K, batch, dt):
    """Opens the GEMM_FLOPS / GEMM_TRACE bracket of one launch (gemm, gemm_ln, gemm_act_bwd): counts its FLOPs and, with a trace
    installed, records the first event.  Returns what _trace_end needs, None without a trace."""
    if GEMM_FLOPS is not None:
        GEMM_FLOPS[0] += 2.0 * M * N * K * batch
    if GEMM_TRACE is None:
        return None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    return (M, N, K, batch, dt, e0, e1)


def _trace_end(t, route=None, args=None):
    """Closes the bracket: (M, N, K, batch, dtype, e0, e1, on_256).  Last field: did the library run this launch on its
    256 x 256-tile kernel, asked of the entry's *_route twin with the same arguments."""
    if t is not None:
        t[-1].record()
        GEMM_TRACE.append((*t, route is not None and route(*args) == 80))


def _autotune_gemm(lib, args, key, out, residual):
    if torch.cuda.is_current_stream_capturing() or (residual is not None and residual.data_ptr() == out.data_ptr()):
        return 0
    act = args[16]
    best, best_t = 0, float("inf")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for v in _TUNE_CANDIDATES:
        args[16] = act | (v << 8)
        if lib.msmd_gemm(*args) != 0:
            continue
        e0.record()
        for _ in range(3):
            lib.msmd_gemm(*args)
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1)
        if t < best_t:
            best, best_t = v, t
    args[16] = act
    _TUNED[key] = best
    return best


def gemm(a, w, bias=None, residual=None, act=ACT_NONE, out=None, out_dtype=None, *, M=None, K=None, lda=None,
         rows_per_batch=0, a_batch_stride=0, batch=1, strideA=0, strideW=0, strideC=0, strideBias=0, strideR=0,
         N=None, ldw=None, ldc=None, z_out=None, p_drop=0.0, rng_state=None, site=0, variant=None, flags=None):
    """C = dropout_p(act(A @ W^T + bias)) + residual (p_drop = 0: no dropout); z_out (like C) receives the
    pre-activation A @ W^T + bias when given (training epilogue, msmd_gemm_ex).  a: (..., K) contiguous unless M/K/lda describe a windowed view;
    w: (N, K) (or (batch, N, K) with strideW).  Returns C with a's leading dims + (N,)."""
    _need_cuda(a, w, bias, residual)
    lib = _lib.load()
    if isinstance(w, Split) and not isinstance(a, Split):
        # parity-grade speed mode with an fp32 producer: convert here (hot producers hand over Split tensors directly).
        # Only whole contiguous tensors: the caller's lda / strides describe the ORIGINAL layout.
        if not a.is_contiguous() or a.shape[-1] % 32:
            raise ValueError("split GEMM: pass a contiguous fp32 tensor with a last dim % 32 == 0, or a Split")
        a = to_split(a)
    if isinstance(a, Split) and not isinstance(w, Split):
        raise TypeError("split activations need split weights")
    if isinstance(a, Split) and out_dtype is None and out is None:
        out_dtype = torch.float32
    if K is None:
        K = a.shape[-1]
    if M is None:
        M = a.numel() // K
    if N is None:
        N = w.shape[-2]
    if lda is None:
        lda = K
    if ldw is None:
        ldw = w.shape[-1]
    out_dtype = out_dtype or a.dtype
    if out is None:
        lead = a.shape[:-1] if a.numel() // a.shape[-1] == M and batch == 1 else (M,)
        out = empty((*lead, N), a.device, out_dtype)
    if ldc is None:
        ldc = N
    ldr = residual.stride(-2) if residual is not None and residual.dim() >= 2 else N
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("bias must be fp32")
    trace = _trace_begin(M, N, K, batch, _dt(a))
    if variant is None:
        variant = _GEMM_DEFAULT["split_variant"] if isinstance(a, Split) else _GEMM_DEFAULT["variant"]
        if GEMM_ROUTER is not None and not isinstance(a, Split):
            variant = GEMM_ROUTER(M, N, K, batch) or variant
    flags = _GEMM_DEFAULT["flags"] if flags is None else flags
    if isinstance(w, Split) and w.below_32:
        flags |= GEMM_W_BELOW_32
    act = act | (variant << 8) | flags
    args = [_p(a), _p(w), _p(bias), _p(residual), _p(out), M, N, K, _dt(a), _dt(out), lda, rows_per_batch,
            a_batch_stride, ldw, ldc, ldr, act, batch, strideA, strideW, strideC, strideBias, strideR, _stream()]
    if (GEMM_AUTOTUNE and variant == 0 and a.dtype == torch.bfloat16 and K % 64 == 0
            and 2.0 * M * N * K * batch >= _TUNE_MIN_FLOP):
        key = (M, N, K, batch, out.dtype, act, bias is not None, residual is not None, rows_per_batch > 0, lda, ldc)
        v = _TUNED.get(key)
        if v is None:
            v = _autotune_gemm(lib, args, key, out, residual)
        args[16] = act | (v << 8)
    train = z_out is not None or p_drop > 0.0
    if train or trace is not None:
        ex = (*args[:-1], _p(z_out), float(p_drop), _p(rng_state), int(site), args[-1])
    if train:
        _lib.check(lib.msmd_gemm_ex(*ex), "msmd_gemm_ex")
    else:
        _lib.check(lib.msmd_gemm(*args), "msmd_gemm")
    _trace_end(trace, lib.msmd_gemm_route, ex if trace is not None else None)
    return out


GEMM_LN_TILE = None            # 15 | 17 | 18 | None: tile of msmd_gemm_ln's big-tile family for the calls made while it is set (the
                               # sampler sets 15 -- 192 x 128 -- around the capture of a multi-lane step graph, see sampler.py)


def gemm_ln(a, w, bias=None, residual=None, act=ACT_NONE, out=None, out_dtype=None, *, a_stats=None, w_colsum=None,
            r_stats=None, r_gamma=None, r_beta=None, stats_out=False, eps=1e-5):
    """C = act(LN_A(a) @ w^T + bias) + LN_R(residual) with the LayerNorms folded into the GEMM epilogue (msmd_gemm_ln):
    a_stats / r_stats are (cols / slab, M, 2) per-row partial (sum, sum of squares) written by a producer's stats_out;
    w must hold gamma-folded weights with w_colsum = their row sums and bias the beta-folded bias (see fold_layernorm).
    stats_out=True: returns (C, stats) with the partial statistics of the stored rows of C (the slab -- 64 or 32 columns --
    follows the tile the grid is routed to and is read back from the statistics' shape by the consumer)."""
    _need_cuda(a, w, bias, residual)
    lib = _lib.load()
    K = a.shape[-1]
    M = a.numel() // K
    N = w.shape[0]
    out_dtype = out_dtype or a.dtype
    if out is None:
        out = empty((*a.shape[:-1], N), a.device, out_dtype)
    st, slab_out, slab_in = None, 0, 0
    if stats_out:
        # by the problem's N alone, never its row count: a clip's rows must get the same statistics (bit for bit) alone and
        # inside a large batch, so the producer is always the 128 x 128-tile family where that tile divides N
        slab_out = 64 if N % 128 == 0 else 32
        st = empty((N // slab_out, M, 2), a.device, torch.float32)
    sin = a_stats if a_stats is not None else r_stats
    if sin is not None:
        cols = K if a_stats is not None else N
        if sin.dim() != 3 or sin.shape[1] != M or sin.shape[2] != 2 or cols % sin.shape[0]:
            raise ValueError("gemm_ln: statistics must be (cols / slab, M, 2)")
        slab_in = cols // sin.shape[0]
    for t in (bias, w_colsum, r_gamma, r_beta, a_stats, r_stats):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError("gemm_ln: bias / colsum / gamma / beta / stats must be contiguous fp32")
    ldr = residual.stride(-2) if residual is not None and residual.dim() >= 2 else N
    trace = _trace_begin(M, N, K, 1, _dt(a))
    hint = 66 if GEMM_LN_ALL_IN_ONE else ((GEMM_LN_ROUTER(M, N, K) or 0) if GEMM_LN_ROUTER is not None else (GEMM_LN_TILE or 0))
    args = (_p(a), _p(w), _p(bias), _p(residual), _p(out), M, N, K, _dt(a), _dt(out), a.stride(-2) if a.dim() >= 2 else K,
            w.stride(0), N, ldr, act | GEMM_LN_FLAGS | (hint << 8), _p(a_stats), _p(w_colsum), _p(r_stats), _p(r_gamma),
            _p(r_beta), _p(st), slab_in, slab_out, float(eps), _stream())
    _lib.check(lib.msmd_gemm_ln(*args), "msmd_gemm_ln")
    _trace_end(trace, lib.msmd_gemm_ln_route, args)
    return (out, st) if st is not None else out


def fold_layernorm(w, b, gamma, beta, dtype):
    """Weights of `Linear(LayerNorm(u))` for gemm_ln: (W' = dtype(W * gamma), colsum(W') fp32, b + W @ beta)."""
    w32, g32, be32 = w.float(), gamma.float(), beta.float()
    wf = (w32 * g32[None, :]).to(dtype).contiguous()
    cs = wf.float().sum(dim=1).contiguous()
    bf = (w32 @ be32 + (b.float() if b is not None else 0.0)).contiguous()
    return wf, cs, bf


def gemm_act_bwd(dy, wt, z, act, p_drop=0.0, rng_state=None, site=0):
    """dz = keep_mask / (1 - p) * act'(z) * (dy @ wt^T): msmd_gemm_actbwd (the data gradient of the Linear AFTER an
    activation + dropout, with their backward in its epilogue).  dy (..., K) 16-bit, wt (N, K) = the transposed weight
    cast, z (..., N) the forward's pre-activation."""
    _need_cuda(dy, wt, z)
    K = dy.shape[-1]
    M = dy.numel() // K
    N = wt.shape[0]
    if z.numel() != M * N or not z.is_contiguous() or not dy.is_contiguous():
        raise ValueError("gemm_act_bwd: z must be the contiguous (M, N) pre-activation")
    out = torch.empty_like(z)
    trace = _trace_begin(M, N, K, 1, _dt(dy))
    _lib.check(_lib.load().msmd_gemm_actbwd(_p(dy), _p(wt), _p(z), _p(out), M, N, K, _dt(dy), _dt(out), K, wt.stride(0),
                                            act | (_GEMM_DEFAULT["flags"] & GEMM_PAIRED_STORES), float(p_drop), _p(rng_state),
                                            int(site), _stream()), "msmd_gemm_actbwd")
    _trace_end(trace)
    return out


def exp_set_tuning(key, value):
    """Kept as a name for callers of the removed experimental library: the library has no process-global switch."""
    raise _lib.MsmdLibraryError("msmd_exp_set_tuning: the experimental library and its tuning keys were removed; "
                                "use the per-call `variant` / `flags` / `splits` arguments")


g_tn_split = True


def gemm_tn(a, b, want_colsum=False, *, M=None, N=None, K=None, lda=None, ldb=None, batch=1, strideA=0, strideB=0,
            b_rows_per_window=0, b_window_stride=0, out=None, colsum_out=None, accumulate=False, splits=0):
    """C (N, K) fp32 = a^T @ b for bf16 a (M, N), b (M, K) (contraction over rows: the weight-gradient product, no
    transposes).  Returns C, or (C, colsum) with colsum[n] = sum_m a[m, n] (the bias gradient) when asked."""
    _need_cuda(a, b)
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise TypeError("gemm_tn takes bf16 operands")
    lib = _lib.load()
    M = a.shape[-2] if M is None else M
    N = a.shape[-1] if N is None else N
    K = b.shape[-1] if K is None else K
    lda = a.stride(-2) if lda is None else lda
    ldb = b.stride(-2) if ldb is None else ldb
    if out is None:
        out = torch.empty((batch, N, K) if batch > 1 else (N, K), device=a.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != batch * N * K:
        raise ValueError("gemm_tn out must be a contiguous fp32 (N, K) tensor")
    cs = colsum_out if colsum_out is not None else (
        torch.empty(N, device=a.device, dtype=torch.float32) if want_colsum else None)
    nws = lib.msmd_gemm_tn_workspace(M, N, K, batch) if g_tn_split else 0
    ws = torch.empty(nws, device=a.device, dtype=torch.uint8) if nws > 0 else None
    _lib.check(lib.msmd_gemm_tn(_p(a), _p(b), _p(out), _p(cs), M, N, K, lda, ldb, K, batch, strideA, strideB, N * K,
                                b_rows_per_window, b_window_stride, int(bool(accumulate)) | (int(splits) << 8), _p(ws), nws,
                                _stream()), "msmd_gemm_tn")
    return (out, cs) if (want_colsum or colsum_out is not None) else out


def conv1d_cl(x, w_packed, bias=None, *, kernel, stride, act=ACT_NONE, out_dtype=None):
    """Strided Conv1d over a channels-last (B, T, C) signal as ONE windowed GEMM (no im2col).
    w_packed: (Cout, kernel*C) with K index = kk*C + c."""
    B, T, C = x.shape
    T_out = (T - kernel) // stride + 1
    out = empty((B, T_out, w_packed.shape[0]), x.device, out_dtype or x.dtype)
    gemm(x, w_packed, bias, None, act, out=out, M=B * T_out, K=kernel * C, lda=stride * C, rows_per_batch=T_out,
         a_batch_stride=T * C)
    return out


CONV_CHAIN_RELEASE, CONV_CHAIN_ROW_BLOCK_TICKETS = _h("CONV_CHAIN_RELEASE", "CONV_CHAIN_ROW_BLOCK_TICKETS")
CONV_CHAIN_FLAGS = 0      # the forms conv_chain() asks for when the caller names none: write-through hand-over, one tile per ticket


def _int_array(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def conv_chain_plan(B, T0, C, N, kernels, strides, flags, ticket):
    """msmd_conv_chain_plan (host only, no GPU): (layer, row block, first column tile, column tiles, first, last producer row
    block) of `ticket`; the ticket count (an int) for a ticket past the last; None for shapes the kernel does not take."""
    out = (ctypes.c_int * 6)()
    r = _lib.load().msmd_conv_chain_plan(B, T0, C, N, len(kernels), _int_array(kernels), _int_array(strides), flags, ticket, out)
    return None if r < 0 else (tuple(out) if r == 0 else r)


def conv_chain_status(workspace):
    """The status word of the conv_chain launch that used `workspace` (blocks; 0 = no wait expired)."""
    return _lib.load().msmd_conv_chain_status(_p(workspace))


def conv_chain(x, ws_packed, biases, *, kernels, strides, act=ACT_NONE, flags=None, max_workgroups=0, outs=None, workspace=None):
    """2 to 4 strided Conv1d layers over a channels-last 16-bit (B, T, C) signal as ONE launch (msmd_conv_chain): layer l is
    conv1d_cl(., ws_packed[l], biases[l], kernel=kernels[l], stride=strides[l], act=act) of layer l - 1's output, same bits.
    Returns the list of every layer's output, or None -- nothing launched -- where the library declines the shapes (the caller
    then runs the layers one by one).  outs / workspace: buffers to reuse (tests, tools)."""
    _need_cuda(x, *ws_packed, *biases)
    lib = _lib.load()
    B, T0, C = x.shape
    n, N = len(ws_packed), ws_packed[0].shape[0]
    if x.dtype not in (torch.bfloat16, torch.float16) or not x.is_contiguous() or any(w.dtype != x.dtype or not w.is_contiguous() for w in ws_packed):
        return None
    ks, ss = _int_array(kernels), _int_array(strides)
    nbytes = lib.msmd_conv_chain_workspace(B, T0, C, N, n, ks, ss)
    if nbytes <= 0:
        return None
    if outs is None:
        outs, T = [], T0
        for k, s in zip(kernels, strides):
            T = (T - k) // s + 1
            outs.append(torch.empty((B, T, N), device=x.device, dtype=x.dtype))
    if workspace is None:
        workspace = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    Ms = [o.shape[0] * o.shape[1] for o in outs]
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[_p(t) for t in ts])
    flags = CONV_CHAIN_FLAGS if flags is None else flags
    # one bracket for the launch: N is shared and so is K past the first layer, so 2 N sum(M_l K_l) is booked as the first
    # layer's own product plus the rest on the shared K; marked as a 256 x 256-tile launch
    Ks = [k * (C if l == 0 else N) for l, k in enumerate(kernels)]
    if len(set(Ks)) == 1:
        trace = _trace_begin(sum(Ms), N, Ks[0], 1, _dt(x))
    else:
        if GEMM_FLOPS is not None:
            GEMM_FLOPS[0] += 2.0 * N * (sum(m * k for m, k in zip(Ms, Ks)) - sum(Ms[1:]) * Ks[1])
        trace = _trace_begin(sum(Ms[1:]), N, Ks[1], 1, _dt(x))
    r = lib.msmd_conv_chain(_p(x), B, T0, C, N, n, ptrs(ws_packed), ptrs(biases), ptrs(outs), ks, ss, act, _dt(x), _p(workspace),
                            workspace.numel(), max_workgroups, flags, _stream())
    _lib.check(r, "msmd_conv_chain")
    _trace_end(trace, lambda: 80, ())
    return outs


def layernorm(x, gamma, beta, residual=None, post_add=None, act=ACT_NONE, eps=1e-5, out_dtype=None, post_act=ACT_NONE,
              split=None):
    """y = post_act(LayerNorm(act(x + residual)) * gamma + beta) + post_add.
    split="both": returns (y fp32, y Split) from ONE pass; split="only": the Split alone (fp32 input, cols % 32 == 0)."""
    _need_cuda(x, gamma, beta)
    lib = _lib.load()
    cols = x.shape[-1]
    rows = x.numel() // cols
    if split:
        if x.dtype != torch.float32 or (residual is not None and residual.dtype != torch.float32):
            raise TypeError("layernorm(split=...) takes fp32 input")
        y = torch.empty(x.shape, device=x.device, dtype=torch.float32) if split == "both" else None
        ys = empty(tuple(x.shape), x.device, SPLIT)
        _lib.check(lib.msmd_layernorm_f16x2(_p(x), _p(residual), _p(gamma), _p(beta), _p(post_add), _p(y), _p(ys), rows,
                                            cols, eps, act | (post_act << 8), _stream()), "msmd_layernorm_f16x2")
        return (y, ys) if split == "both" else ys
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype or x.dtype)
    _lib.check(lib.msmd_layernorm(_p(x), _p(residual), _p(gamma), _p(beta), _p(post_add), _p(y), rows, cols, eps,
                                  act | (post_act << 8),
                                  _dt(x), _dt(y), _stream()), "msmd_layernorm")
    return y


def layernorm_pre(x, pre_gamma, pre_beta, residual, gamma, beta, eps=1e-5):
    """LN_{gamma, beta}(LN_{pre}(x) + residual) in one launch (16-bit rows): msmd_layernorm_pre."""
    _need_cuda(x, gamma, beta, pre_gamma, pre_beta)
    cols = x.shape[-1]
    rows = x.numel() // cols
    y = torch.empty_like(x)
    _lib.check(_lib.load().msmd_layernorm_pre(_p(x), _p(pre_gamma), _p(pre_beta), _p(residual), _p(gamma), _p(beta), _p(y),
                                              rows, cols, eps, _dt(x), _stream()), "msmd_layernorm_pre")
    return y


def dropout(x, p, rng_state, site, residual=None, out=None):
    """y = x * keep / (1 - p) (+ residual); keep = Philox(rng_state[seed, step], site, element / 4).  Calling it on
    the upstream gradient with the same (rng_state, site) is the backward."""
    _need_cuda(x, rng_state)
    x = x.contiguous()
    if residual is not None:
        residual = residual.contiguous()
    out = torch.empty_like(x) if out is None else out
    _lib.check(_lib.load().msmd_dropout(_p(x), _p(residual), _p(out), x.numel(), float(p), _p(rng_state), int(site),
                                        _dt(x), _stream()), "msmd_dropout")
    return out


def _prefetch_ranges(tensors):
    """(pointer array, byte-count array, count) of the first four live, contiguous device tensors (Split: its storage)."""
    ts = []
    for t in tensors:
        t = t.t if isinstance(t, Split) else t
        if t is not None and t.is_cuda and t.is_contiguous():
            ts.append(t)
    ts = ts[:4]
    ptrs = (ctypes.c_void_p * 4)(*([t.data_ptr() for t in ts] + [None] * (4 - len(ts))))
    nbytes = (ctypes.c_long * 4)(*([t.numel() * t.element_size() for t in ts] + [0] * (4 - len(ts))))
    return ptrs, nbytes, len(ts)


def _attn_args(mask, scale, n_heads, q, k, v, *rest):
    """The leading arguments of every attention entry, in the C order: pointers of q, k, v and `rest`, B, H, Tq, Tk, the
    batch and row stride of each tensor, the scale, the (Tq, Tk) mask (checked here)."""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    if mask is not None:
        assert mask.dtype in (torch.bool, torch.uint8) and mask.shape == (Tq, Tk) and mask.is_contiguous()
    ts = (q, k, v) + rest
    return (*[_p(t) for t in ts], B, n_heads, Tq, Tk, *[t.stride(i) for t in ts for i in (0, 1)], float(scale), _p(mask))


def attention(q, k, v, n_heads, scale, mask=None, out=None, p_drop=0.0, rng_state=None, site=0, out_dtype=None,
              prefetch=None):
    """q: (B, Tq, H*64) view, k/v: (B, Tk, H*64) views (last dim contiguous; may be slices of a packed QKV).
    Split q / k / v (parity-grade speed mode): msmd_attention_f16x2; out_dtype SPLIT (default) or torch.float32.
    Entry per case: split -> msmd_attention_f16x2 (no dropout, prefetch ignored); otherwise msmd_attention,
    msmd_attention_prefetch, msmd_attention_dropout or msmd_attention_dropout_prefetch by p_drop > 0 and prefetch."""
    _need_cuda(q, k, v)
    lib = _lib.load()
    B, Tq, d = q.shape
    assert d == n_heads * 64 and q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1
    split = isinstance(q, Split)
    if split and (not (isinstance(k, Split) and isinstance(v, Split)) or p_drop > 0.0):
        raise TypeError("split attention: q, k, v must all be Split (inference only)")
    if out is None:
        out = empty((B, Tq, d), q.device, out_dtype or SPLIT) if split else torch.empty(B, Tq, d, device=q.device, dtype=q.dtype)
    args = _attn_args(mask, scale, n_heads, q, k, v, out)
    drop = (float(p_drop), _p(rng_state), int(site)) if p_drop > 0.0 else ()
    # up to four tensors (the weights of the GEMMs that follow) pulled through the memory-side cache by this launch
    pf = _prefetch_ranges(prefetch) if prefetch and PREFETCH_WEIGHTS and not split else ()
    name = "msmd_attention_f16x2" if split else "msmd_attention" + ("_dropout" if drop else "") + ("_prefetch" if pf else "")
    _lib.check(getattr(lib, name)(*args, *drop, _dt(out if split else q), *pf, _stream()), name)
    return out


def attention_bwd(q, k, v, do, dq, dk, dv, n_heads, scale, mask=None, p_drop=0.0, rng_state=None, site=0):
    """Fused backward of `attention` (bf16, Tk <= 256): fills dq / dk / dv (views with last dim contiguous)."""
    _need_cuda(q, k, v, do, dq, dk, dv)
    for t in (q, k, v, do, dq, dk, dv):
        if t.dtype != torch.bfloat16 or t.stride(-1) != 1:
            raise TypeError("attention_bwd takes bf16 tensors with a contiguous last dim")
    _lib.check(_lib.load().msmd_attention_bwd(*_attn_args(mask, scale, n_heads, q, k, v, do, dq, dk, dv), float(p_drop),
                                              _p(rng_state), int(site), _stream()), "msmd_attention_bwd")


def dynamic_threshold_(res, L, ratio, dt_min, dt_max):
    """In-place dynamic thresholding of a (N, T_all, C) fp32 denoiser output on its last L frames' quantile."""
    _need_cuda(res)
    if res.dtype != torch.float32 or not res.is_contiguous():
        raise TypeError("dynamic_threshold_ takes a contiguous fp32 tensor")
    N, T_all, C = res.shape
    _lib.check(_lib.load().msmd_dynamic_threshold(_p(res), N, T_all, L, C, float(ratio), float(dt_min), float(dt_max),
                                                  _stream()), "msmd_dynamic_threshold")
    return res


def pad_audio(audio, reflect_len, replicate_len):
    lib = _lib.load()
    B, L = audio.shape
    out = torch.empty(B, L + 4 * reflect_len + 2 * replicate_len, device=audio.device, dtype=torch.float32)
    _lib.check(lib.msmd_pad_audio(_p(audio), _p(out), B, L, reflect_len, replicate_len, _stream()), "msmd_pad_audio")
    return out


def conv0_workspace(B, device):
    """the moment workspace of msmd_conv0_stats: (B, CONV0_SPLITS, 66) doubles"""
    return torch.empty(B, CONV0_SPLITS, 66, device=device, dtype=torch.float64)


def conv0_gn_gelu(audio, w0, gamma, beta, reflect_len, replicate_len, out_dtype, eps=1e-5):
    """GELU(GroupNorm(conv0(pad_audio(audio)))) -> (B, T0, C) channels-last."""
    lib = _lib.load()
    B, L = audio.shape
    C = w0.shape[0]
    Lp = L + 4 * reflect_len + 2 * replicate_len
    T0 = (Lp - 10) // 5 + 1
    stats = torch.empty(B, C, 2, device=audio.device, dtype=torch.float32)
    ws = conv0_workspace(B, audio.device)
    _lib.check(lib.msmd_conv0_stats(_p(audio), _p(w0), _p(stats), _p(ws), B, L, reflect_len, replicate_len, C, eps,
                                    _stream()), "msmd_conv0_stats")
    out = empty((B, T0, C), audio.device, out_dtype)
    _lib.check(lib.msmd_conv0_gn_gelu(_p(audio), _p(w0), _p(stats), _p(gamma), _p(beta), _p(out), B, L, reflect_len,
                                      replicate_len, C, _dt(out), _stream()), "msmd_conv0_gn_gelu")
    return out


def conv0_ln_gelu(audio, w0, bias, gamma, beta, reflect_len, replicate_len, out_dtype, eps=1e-5):
    """GELU(LayerNorm_channels(conv0(pad_audio(audio)) + bias)) -> (B, T0, 512) (feat_extract_norm="layer" stacks)."""
    lib = _lib.load()
    B, L = audio.shape
    C = w0.shape[0]
    Lp = L + 4 * reflect_len + 2 * replicate_len
    T0 = (Lp - 10) // 5 + 1
    out = torch.empty(B, T0, C, device=audio.device, dtype=out_dtype)
    _lib.check(lib.msmd_conv0_ln_gelu(_p(audio), _p(w0), _p(bias), _p(gamma), _p(beta), _p(out), B, L, reflect_len,
                                      replicate_len, C, eps, _dt(out), _stream()), "msmd_conv0_ln_gelu")
    return out


def interp_linear(x, t_out, t_crop=None):
    lib = _lib.load()
    B, T, C = x.shape
    t_crop = T if t_crop is None else min(int(t_crop), T)  # slicing past the end clamps (utils/wav2vec2.py:83)
    y = torch.empty(B, t_out, C, device=x.device, dtype=x.dtype)
    _lib.check(lib.msmd_interp_linear(_p(x), _p(y), B, T, t_crop, t_out, C, _dt(x), _stream()), "msmd_interp_linear")
    return y


def group_pad(x, groups, pad, cg_out=None, split=False):
    """(B, T, G*Cg) -> zero-padded group-major (B, G, T + 2 pad, cg_out >= Cg); split=True writes MSMD_F16X2 rows
    (fp32 input, cg_out % 32 == 0)."""
    lib = _lib.load()
    B, T, C = x.shape
    cg = C // groups
    cg_out = cg if cg_out is None else cg_out
    y = empty((B, groups, T + 2 * pad, cg_out), x.device, SPLIT if split else x.dtype)
    _lib.check(lib.msmd_group_pad(_p(x), _p(y), B, T, groups, cg, cg_out, pad, _dt(x), _dt(y), _stream()),
               "msmd_group_pad")
    return y


def pos_conv(x, w, bias, groups, kpos=128):
    """x + GELU(grouped positional conv(x) + bias) on channels-last 16-bit x (B, T, G*Cg) in one launch; w (G, Cg, kpos*Cg)
    packed as for the windowed-GEMM form (K = tap*Cg + channel).  Bit-identical to group_pad + gemm(ACT_GELU, residual=x)."""
    lib = _lib.load()
    _need_cuda(x)
    B, T, C = x.shape
    cg = C // groups
    if not (x.is_contiguous() and w.is_contiguous() and w.dtype == x.dtype and tuple(w.shape) == (groups, cg, kpos * cg)):
        raise TypeError("pos_conv takes contiguous x (B, T, G*Cg) and w (G, Cg, kpos*Cg) of one 16-bit dtype")
    if bias.dtype != torch.float32 or bias.numel() != C:
        raise TypeError("pos_conv takes an fp32 bias of G*Cg values")
    y = torch.empty_like(x)
    _lib.check(lib.msmd_pos_conv(_p(x), _p(w), _p(bias), _p(y), B, T, groups, cg, kpos, _dt(x), _stream()), "msmd_pos_conv")
    return y


def denoiser_pack_input(motion, prev_motion, indicator, feats, eps=None, c0=None, c1=None):
    lib = _lib.load()
    N, Tn, Kpad = feats.shape
    L, dm = motion.shape[1], motion.shape[2]
    Lp = prev_motion.shape[1]
    assert Tn == 1 + Lp + L
    _lib.check(lib.msmd_denoiser_pack_input(_p(motion), _p(eps), _p(c0), _p(c1), _p(prev_motion), _p(indicator),
                                            _p(feats), N, L, Lp, dm, Kpad, motion.shape[0], _dt(feats), _stream()),
               "msmd_denoiser_pack_input")
    return feats


def denoiser_pack_input_guided(motion, prev_motion, indicator, feats, guide_mask, guide_values, eps=None, c0=None, c1=None):
    """denoiser_pack_input with keyframes: where guide_mask (B, L) uint8 is set, frame t of clip b enters the denoiser as
    guide_values[b, t] (B, L, dm) fp32 instead of motion[b, t]."""
    lib = _lib.load()
    N, Tn, Kpad = feats.shape
    B, L, dm = motion.shape
    Lp = prev_motion.shape[1]
    assert Tn == 1 + Lp + L
    if guide_mask is not None:
        _need_cuda(guide_mask, guide_values)
        if not (guide_mask.dtype == torch.uint8 and tuple(guide_mask.shape) == (B, L) and guide_mask.is_contiguous()
                and guide_values.dtype == torch.float32 and tuple(guide_values.shape) == (B, L, dm)
                and guide_values.is_contiguous()):
            raise TypeError("denoiser_pack_input_guided takes a contiguous uint8 mask (B, L) and fp32 values (B, L, dm)")
    _lib.check(lib.msmd_denoiser_pack_input_guided(_p(motion), _p(eps), _p(c0), _p(c1), _p(prev_motion), _p(indicator),
                                                   _p(guide_mask), _p(guide_values), _p(feats), N, L, Lp, dm, Kpad, B,
                                                   _dt(feats), _stream()), "msmd_denoiser_pack_input_guided")
    return feats


def denoiser_prepare(motion, prev_motion, indicator, feats, ts, emb_table, emb, person_a, person_b, pf, prev_audio, mem,
                     style=None, style_out=None, eps=None, t0=None, t1=None):
    """The denoiser's input layout in one launch (msmd_denoiser_prepare): `feats` as denoiser_pack_input writes it with
    c0 = t0[ts], c1 = t1[ts]; `pf` = [person_a | person_b | zeros] as pad_cols; `style_out` = cast(style); `emb` =
    emb_table[ts]; mem[:, :Lpa] = prev_audio.  Every output is the caller's.  prev_motion (1 | N, Lp, dm) and prev_audio
    (1 | N, Lpa, d) may be expanded views (batch stride 0).  16-bit storage types only."""
    lib = _lib.load()
    N, Tn, Kpad = feats.shape
    L, dm = motion.shape[1], motion.shape[2]
    Lp, Lpa, d = prev_motion.shape[1], prev_audio.shape[1], emb.shape[-1]
    _need_cuda(motion, prev_motion, indicator, feats, ts, emb_table, emb, person_a, person_b, pf, prev_audio, mem, style,
               style_out, eps, t0, t1)

    def rows(t, inner, vec):
        """fp32 (1 | N, ...) whose sequences are contiguous blocks of `inner` elements -> (tensor, batch stride); vec: the
        blocks are read 16 bytes at a time."""
        if t.dtype != torch.float32:
            t = t.float()
        if t.shape[0] != 1 and t.stride(0) == 0:
            t = t[:1]
        if (not t[0].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < inner)
                or (vec and (t.data_ptr() % 16 or t.stride(0) % 4))):
            t = t.contiguous()
        if t.shape[0] not in (1, N):
            raise ValueError("denoiser_prepare: prev_motion / prev_audio hold 1 or N sequences")
        return t, (0 if t.shape[0] == 1 else t.stride(0))
    prev_motion, pm_stride = rows(prev_motion, Lp * dm, False)
    prev_audio, pa_stride = rows(prev_audio, Lpa * d, True)
    for t in (motion, indicator, eps, t0, t1, person_a, person_b, style):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError("denoiser_prepare: motion, indicator, eps, the schedule tables, person and style rows are contiguous fp32")
    if ts.dtype != torch.long or ts.numel() != N or not ts.is_contiguous():
        raise TypeError("denoiser_prepare: ts is a contiguous int64 tensor of N steps")
    if (Tn != 1 + Lp + L or motion.shape[0] != N or (eps is not None and (eps.shape != motion.shape or t0 is None or t1 is None
                                                                            or t0.numel() != emb_table.shape[0] or t1.numel() != t0.numel()))
            or (indicator is not None and indicator.numel() != N * L)):
        raise ValueError("denoiser_prepare: feats (N, 1 + Lp + L, Kpad), motion / eps (N, L, dm), indicator (N, L), tables of one length")
    for t in (feats, emb_table, emb, pf, mem, style_out):
        if t is not None and t.dtype != feats.dtype:
            raise TypeError("denoiser_prepare: feats, emb_table, emb, pf, mem and style_out share one storage type")
    if (not (feats.is_contiguous() and emb.is_contiguous() and emb_table.is_contiguous() and pf.is_contiguous())
            or tuple(emb.shape) != (N, d) or emb_table.shape[-1] != d or emb_table.dim() != 2 or pf.shape[0] != N
            or mem.shape[0] != N or mem.shape[1] < Lpa or mem.shape[2] != d or mem.stride(2) != 1 or mem.stride(1) != d
            or prev_audio.shape[2] != d):
        raise ValueError("denoiser_prepare: emb (N, d), emb_table (steps, d), pf (N, kp), mem (N, >= Lpa, d) with contiguous sequences")
    cols_a = person_a.numel() // N
    cols_b = 0 if person_b is None else person_b.numel() // N
    if person_a.numel() != N * cols_a or (person_b is not None and person_b.numel() != N * cols_b):
        raise ValueError("denoiser_prepare: person rows are (N, cols)")
    if (style is None) != (style_out is None) or (style is not None and (style_out.numel() != style.numel() or not style_out.is_contiguous())):
        raise ValueError("denoiser_prepare: style and style_out come together, with one element count")
    _lib.check(lib.msmd_denoiser_prepare(_p(motion), _p(eps), _p(t0), _p(t1), _p(ts), emb_table.shape[0], _p(prev_motion),
                                         pm_stride, _p(indicator), _p(feats), N, L, Lp, dm, Kpad, _p(person_a), cols_a,
                                         _p(person_b), cols_b, _p(pf), pf.shape[-1], _p(style),
                                         0 if style is None else style.numel(), _p(style_out), _p(emb_table), _p(emb), d,
                                         _p(prev_audio), pa_stride, Lpa, _p(mem), mem.stride(0), _dt(feats), _stream()),
               "msmd_denoiser_prepare")


def add_pe_token(x, pe, tok0, row0_add=None):
    lib = _lib.load()
    N, T, d = x.shape
    _lib.check(lib.msmd_add_pe_token(_p(x), _p(pe), _p(tok0), _p(row0_add), N, T, d, _dt(x), _stream()),
               "msmd_add_pe_token")
    return x


def heads_static_mix(dec, stat, L, dm, nb, use_head_alpha=False, sigmoid_alpha=False):
    lib = _lib.load()
    N = dec.shape[0]
    out = torch.empty(N, L, dm, device=dec.device, dtype=torch.float32)
    _lib.check(lib.msmd_heads_static_mix(_p(dec), dec.stride(1), _p(stat), _p(out), N, L, dm, nb, stat.shape[0],
                                         int(bool(use_head_alpha)) | (2 if sigmoid_alpha else 0), _dt(dec), _stream()),
               "msmd_heads_static_mix")
    return out


def cfg_ddpm_step(x, res, z, scales, n_entries, Lp, mode, target, c0, c1, sigma):
    lib = _lib.load()
    B, L, dm = x.shape
    _lib.check(lib.msmd_cfg_ddpm_step(_p(x), _p(res), _p(z), _p(scales), n_entries, B, L, Lp, dm, mode, target,
                                      float(c0), float(c1), float(sigma), _stream()), "msmd_cfg_ddpm_step")
    return x


def sampler_step_select(emb_all, coef_table, t_dev, emb_row, coefs):
    lib = _lib.load()
    _lib.check(lib.msmd_sampler_step_select(_p(emb_all), _p(coef_table), _p(t_dev), _p(emb_row), _p(coefs),
                                            emb_all.shape[-1], _dt(emb_all), _stream()), "msmd_sampler_step_select")


def cfg_ddpm_step_dev(x, res, z, scales, coefs, n_entries, Lp, mode, target):
    lib = _lib.load()
    B, L, dm = x.shape
    _lib.check(lib.msmd_cfg_ddpm_step_dev(_p(x), _p(res), _p(z), _p(scales), _p(coefs), n_entries, B, L, Lp, dm, mode,
                                          target, _stream()), "msmd_cfg_ddpm_step_dev")
    return x



def cfg_solver_step(x, res, z, scales, d_prev, n_entries, Lp, mode, p0, p1, ax, ath, b1, sigma):
    """Few-step solver update (DDIM / DPM-Solver++(2M) row of sampler.solver_table), in place on x and d_prev."""
    lib = _lib.load()
    B, L, dm = x.shape
    _lib.check(lib.msmd_cfg_solver_step(_p(x), _p(res), _p(z), _p(scales), _p(d_prev), n_entries, B, L, Lp, dm, mode,
                                        float(p0), float(p1), float(ax), float(ath), float(b1), float(sigma), _stream()),
               "msmd_cfg_solver_step")
    return x


def sampler_solver_select(emb_tab, coef_tab, i_dev, emb_row, coefs):
    lib = _lib.load()
    _lib.check(lib.msmd_sampler_solver_select(_p(emb_tab), _p(coef_tab), _p(i_dev), _p(emb_row), _p(coefs),
                                              emb_tab.shape[-1], _dt(emb_tab), _stream()), "msmd_sampler_solver_select")


def cfg_solver_step_dev(x, res, z, scales, d_prev, coefs, n_entries, Lp, mode):
    lib = _lib.load()
    B, L, dm = x.shape
    _lib.check(lib.msmd_cfg_solver_step_dev(_p(x), _p(res), _p(z), _p(scales), _p(d_prev), _p(coefs), n_entries, B, L, Lp,
                                            dm, mode, _stream()), "msmd_cfg_solver_step_dev")
    return x


def _streams_args(x, res, dec, stat, d_prev, cum_static, theta_dyn, theta_alpha, n_entries, Lp, nb):
    """Shape / dtype checks of the two streams-step forms (the kernel indexes every buffer from these sizes)."""
    B, L, dm = x.shape
    _need_cuda(x, res, dec, stat, d_prev, cum_static, theta_dyn, theta_alpha)
    N = n_entries * B
    for t in (x, d_prev, cum_static, theta_dyn):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, L, dm) or not t.is_contiguous():
            raise TypeError("cfg_streams_step: x, d_prev, cum_static and theta_dyn are contiguous fp32 (B, L, dm)")
    if res.dtype != torch.float32 or tuple(res.shape) != (N, Lp + L, dm) or not res.is_contiguous():
        raise TypeError("cfg_streams_step: res is contiguous fp32 (n_entries * B, Lp + L, dm)")
    if (dec.dtype != stat.dtype or dec.ndim != 3 or dec.shape[0] != N or dec.shape[1] != Lp + L or dec.shape[2] != dm + nb
            or dec.stride(2) != 1 or dec.stride(0) != (Lp + L) * dec.stride(1) or dec.stride(1) < dm + nb):
        raise TypeError("cfg_streams_step: dec is (n_entries * B, Lp + L, dm + nb) rows of one stride, in stat's dtype")
    if stat.ndim != 3 or stat.shape[0] not in (1, B, N) or tuple(stat.shape[1:]) != (nb, dm) or not stat.is_contiguous():
        raise TypeError("cfg_streams_step: stat is contiguous (1 | B | n_entries * B, nb, dm)")
    if (theta_alpha.dtype != torch.float32 or theta_alpha.ndim != 3 or theta_alpha.shape[0] % B
            or tuple(theta_alpha.shape[1:]) != (L, nb) or not theta_alpha.is_contiguous()):
        raise TypeError("cfg_streams_step: theta_alpha is contiguous fp32 (n_slots * B, L, nb)")
    return B, L, dm, theta_alpha.shape[0] // B


def cfg_streams_step(x, res, dec, stat, z, scales, d_prev, cum_static, theta_dyn, theta_alpha, slot, n_entries, Lp, nb,
                     use_head_alpha, mode, p0, p1, ax, ath, b1, sigma):
    """cfg_solver_step plus sample_separate's streams in one launch: cum_static += ath theta_static, theta_dyn overwritten,
    theta_alpha's row block `slot` written.  use_head_alpha: the bit pair msmd_heads_static_mix takes."""
    lib = _lib.load()
    B, L, dm, n_slots = _streams_args(x, res, dec, stat, d_prev, cum_static, theta_dyn, theta_alpha, n_entries, Lp, nb)
    _lib.check(lib.msmd_cfg_streams_step(_p(x), _p(res), _p(dec), dec.stride(1), _p(stat), _p(z), _p(scales), _p(d_prev),
                                         _p(cum_static), _p(theta_dyn), _p(theta_alpha), int(slot), n_slots, n_entries, B,
                                         L, Lp, dm, nb, stat.shape[0], int(use_head_alpha), mode, _dt(dec), float(p0),
                                         float(p1), float(ax), float(ath), float(b1), float(sigma), _stream()),
               "msmd_cfg_streams_step")
    return x


def cfg_streams_step_dev(x, res, dec, stat, z, scales, d_prev, cum_static, theta_dyn, theta_alpha, coefs, step_dev,
                         n_entries, Lp, nb, use_head_alpha, mode):
    """cfg_streams_step with the six scalars in `coefs` and the slot taken from the device-side step counter."""
    lib = _lib.load()
    B, L, dm, n_slots = _streams_args(x, res, dec, stat, d_prev, cum_static, theta_dyn, theta_alpha, n_entries, Lp, nb)
    _lib.check(lib.msmd_cfg_streams_step_dev(_p(x), _p(res), _p(dec), dec.stride(1), _p(stat), _p(z), _p(scales),
                                             _p(d_prev), _p(cum_static), _p(theta_dyn), _p(theta_alpha), _p(coefs),
                                             _p(step_dev), n_slots, n_entries, B, L, Lp, dm, nb, stat.shape[0],
                                             int(use_head_alpha), mode, _dt(dec), _stream()), "msmd_cfg_streams_step_dev")
    return x


def pad_cols(x, cols_out, out_dtype=None):
    lib = _lib.load()
    cols_in = x.shape[-1]
    rows = x.numel() // cols_in
    y = torch.empty(*x.shape[:-1], cols_out, device=x.device, dtype=out_dtype or x.dtype)
    _lib.check(lib.msmd_pad_cols(_p(x), _p(y), rows, cols_in, cols_out, _dt(x), _dt(y), _stream()), "msmd_pad_cols")
    return y


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    return pad_cols(x.contiguous(), x.shape[-1], dtype)


def mean_time(x):
    lib = _lib.load()
    B, T, C = x.shape
    y = torch.empty(B, C, device=x.device, dtype=torch.float32)
    _lib.check(lib.msmd_mean_time(_p(x), _p(y), B, T, C, _dt(x), _stream()), "msmd_mean_time")
    return y


# ----------------------------------------------------------------------------- FLAME
# msmd_lbs_skin_v2's input record per 16 frames, and the record of its single-fp16-plane form: csrc/lbs_tiles.h defines both
SKIN_TILE_BYTES, SKIN_TILE16_BYTES = 18432, 12288


def _skin_tiles(B, device, tile_bytes=SKIN_TILE_BYTES):
    """An unwritten tile buffer for B frames: one record per 16 frames."""
    return torch.empty((B + 15) // 16, tile_bytes // 2, device=device, dtype=torch.float16)


def _tile_fed(skin_tiles, B, weight_planes, dirs_hl):
    """-> (J, Vp) of a skinning call that reads tile records, after checking that `skin_tiles` holds B frames' worth."""
    assert skin_tiles.numel() * skin_tiles.element_size() == ((B + 15) // 16) * SKIN_TILE_BYTES
    return weight_planes.shape[0], dirs_hl.shape[-2]


def _verts32(B, V, device):
    return torch.empty(B, V, 3, device=device, dtype=torch.float32)


def lbs_prepare(betas, pose, JS, parents, Kp=192, pose_is_matrix=False, want_joints=True, want_split=False,
                want_blend_tiles=False):
    """-> coef, coef_hl, A, joints[, skin_tiles]: want_blend_tiles adds msmd_lbs_skin_v2's 18 KB-per-16-frames records
    (coefficients as bf16 hi / lo + fp16 blend rows); want_split the row-major coef_hl of msmd_lbs_skin_bf16x3."""
    lib = _lib.load()
    B, NB = betas.shape
    J = parents.shape[0]
    coef = torch.empty(B, Kp, device=betas.device, dtype=torch.float32)
    coef_hl = torch.empty(B, 2, Kp, device=betas.device, dtype=torch.bfloat16) if want_split else None
    A = torch.empty(B, J, 12, device=betas.device, dtype=torch.float32)
    joints = torch.empty(B, J, 3, device=betas.device, dtype=torch.float32) if want_joints else None
    at = _skin_tiles(B, betas.device) if want_blend_tiles else None
    _lib.check(lib.msmd_lbs_prepare(_p(betas), _p(pose), _p(JS), _p(parents), _p(coef), _p(coef_hl), _p(A), _p(joints),
                                    _p(at), B, NB, J, Kp, int(pose_is_matrix), _stream()), "msmd_lbs_prepare")
    return (coef, coef_hl, A, joints, at) if want_blend_tiles else (coef, coef_hl, A, joints)


def flame_prepare(shape, expr, pose6, eye, JS, parents, ignore_global_rot=False, dirs=None, v_template_planes=None):
    """FLAME.forward's (B, NS) shape, (B, NE) expression, (B, 6) [global | jaw] pose (+ optional (B, 6) eye pose) ->
    msmd_lbs_skin_v2's tile records, without the concatenated betas / full_pose tensors.  With `dirs` (3, 192, Vp) and the
    template planes also -> (shape_varies flag, folded template) for the one-subject fast path of lbs_skin_v2.  The fold
    needs NS >= 96 shape coefficients: with fewer the kernel sets the flag to "varies" (nonzero) and leaves the folded
    template unwritten, so the pair may always be passed on to lbs_skin_v2."""
    lib = _lib.load()
    _need_cuda(shape, expr, pose6)
    B = shape.shape[0]
    tiles = _skin_tiles(B, shape.device)
    flag = folded = None
    Vp = 0
    if dirs is not None and v_template_planes is not None:
        Vp = dirs.shape[-1]
        flag = torch.empty(1, device=shape.device, dtype=torch.int32)
        folded = torch.empty(3, Vp, device=shape.device, dtype=torch.float32)
    _lib.check(lib.msmd_flame_prepare(_p(shape), _p(expr), _p(pose6), _p(eye), _p(JS), _p(parents), None, None, None,
                                      _p(tiles), B, shape.shape[1], expr.shape[1], int(ignore_global_rot), _p(flag),
                                      _p(folded), _p(dirs), _p(v_template_planes), Vp, _stream()), "msmd_flame_prepare")
    return tiles, flag, folded


def lbs_skin(coef, A, v_template_planes, dirs, weight_planes, V):
    lib = _lib.load()
    B, Kp = coef.shape
    verts = _verts32(B, V, coef.device)
    _lib.check(lib.msmd_lbs_skin(_p(coef), _p(A), _p(v_template_planes), _p(dirs), _p(weight_planes), _p(verts), B,
                                 A.shape[1], V, dirs.shape[-1], Kp, _stream()), "msmd_lbs_skin")
    return verts


def lbs_skin_bf16x3(coef_hl, A, v_template_planes, dirs_hl, weight_planes, V):
    lib = _lib.load()
    B, _, Kp = coef_hl.shape
    verts = _verts32(B, V, A.device)
    _lib.check(lib.msmd_lbs_skin_bf16x3(_p(coef_hl), _p(A), _p(v_template_planes), _p(dirs_hl), _p(weight_planes),
                                        _p(verts), B, A.shape[1], V, dirs_hl.shape[-2], Kp, _stream()), "msmd_lbs_skin_bf16x3")
    return verts


def lbs_skin_v2(skin_tiles, B, v_template_planes, dirs_hl, weight_planes, V, Kp=192, shape_varies=None, folded=None,
                out_dtype=torch.float32, dirs_f16=None):
    """out_dtype=torch.float16 (opt-in, msmd_lbs_skin_v2_f16): the vertices as fp16 -- a (B, V, 3) VIEW of rows padded to an
    even vertex count (row stride (V + V % 2) * 3); half the store stream.  With dirs_f16 (ONE fp16 plane of the blendshape
    directions, LbsConstants.dirs_f16) the product runs on fp16 operand planes (1 MFMA per K group instead of 3; the tile
    records are converted by msmd_lbs_tiles_f16 first): |error| <= 2^-11 |v| + 2^-10 sum_k |coef_k| |dirs_k|; without it the fp32 kernel's arithmetic,
    rounded once at the store."""
    lib = _lib.load()
    J, Vp = _tile_fed(skin_tiles, B, weight_planes, dirs_hl)
    if out_dtype == torch.float16:
        V_ld = V + (V & 1)
        v16 = torch.empty(B, V_ld, 3, device=skin_tiles.device, dtype=torch.float16)
        tiles, dirs, single = skin_tiles, dirs_hl, 0
        if dirs_f16 is not None:
            tiles = _skin_tiles(B, skin_tiles.device, SKIN_TILE16_BYTES)
            _lib.check(lib.msmd_lbs_tiles_f16(_p(skin_tiles), _p(tiles), B, _stream()), "msmd_lbs_tiles_f16")
            dirs, single = dirs_f16, 1
        _lib.check(lib.msmd_lbs_skin_v2_f16(_p(tiles), _p(v_template_planes), _p(dirs), _p(weight_planes), _p(v16), B, J, V,
                                            V_ld, Vp, Kp, _p(shape_varies), _p(folded), single, _stream()), "msmd_lbs_skin_v2_f16")
        return v16[:, :V]
    if out_dtype != torch.float32:
        raise TypeError("lbs_skin_v2: fp32 or fp16 vertices")
    verts = _verts32(B, V, skin_tiles.device)
    _lib.check(lib.msmd_lbs_skin_v2(_p(skin_tiles), _p(v_template_planes), _p(dirs_hl), _p(weight_planes),
                                    _p(verts), B, J, V, Vp, Kp, _p(shape_varies), _p(folded), _stream()),
               "msmd_lbs_skin_v2")
    return verts


def lbs_pack(coef, A, want_split=False):
    """(coef (B, Kp), A (B, 5, 12)) fp32 -> skin_tiles (, coef_hl): the skinning kernels' operand formats."""
    lib = _lib.load()
    B, Kp = coef.shape
    coef_hl = torch.empty(B, 2, Kp, device=coef.device, dtype=torch.bfloat16) if want_split else None
    at = _skin_tiles(B, coef.device)
    _lib.check(lib.msmd_lbs_pack(_p(coef), _p(A), _p(coef_hl), _p(at), B, Kp, _stream()), "msmd_lbs_pack")
    return (at, coef_hl) if want_split else at


def lbs_skin_v2_train(skin_tiles, B, v_template_planes, dirs_hl, weight_planes, V, Kp=192):
    """-> (verts, v_posed): msmd_lbs_skin_v2 that also stores the un-skinned vertices (needed by lbs_skin_bwd)."""
    lib = _lib.load()
    J, Vp = _tile_fed(skin_tiles, B, weight_planes, dirs_hl)
    verts, vposed = _verts32(B, V, skin_tiles.device), _verts32(B, V, skin_tiles.device)
    _lib.check(lib.msmd_lbs_skin_v2_train(_p(skin_tiles), _p(v_template_planes), _p(dirs_hl),
                                          _p(weight_planes), _p(verts), _p(vposed), B, J, V, Vp, Kp, _stream()),
               "msmd_lbs_skin_v2_train")
    return verts, vposed


def lbs_skin_bwd(grad_verts, vposed, A, weight_planes):
    """-> (dp planes (B, 3, Vp), dA (B, 5, 12)) of the skinning's backward."""
    lib = _lib.load()
    B, V, _ = grad_verts.shape
    J, Vp = weight_planes.shape
    dp = torch.empty(B, 3, Vp, device=grad_verts.device, dtype=torch.float32)
    dA = torch.empty(B, J, 12, device=grad_verts.device, dtype=torch.float32)
    _lib.check(lib.msmd_lbs_skin_bwd(_p(grad_verts), _p(vposed), _p(A), _p(weight_planes), _p(dp), _p(dA), B, J, V, Vp,
                                     _stream()), "msmd_lbs_skin_bwd")
    return dp, dA


def _landmarks_launch(verts, faces_i32, idx, bc):
    lib = _lib.load()
    B, V, _ = verts.shape
    L = idx.shape[1]
    out = torch.empty(B, L, 3, device=verts.device, dtype=torch.float32)
    _lib.check(lib.msmd_landmarks(_p(verts), _p(faces_i32), _p(idx), L if idx.shape[0] > 1 else 0, _p(bc),
                                  L * 3 if bc.shape[0] > 1 else 0, _p(out), B, V, L, _stream()), "msmd_landmarks")
    return out


def landmarks_bwd(grad_lmk, faces_i32, idx, bc, V, out=None):
    """-> grad_verts (B, V, 3): msmd_landmarks_bwd's deterministic scatter (no atomics; see include/msmd_hip.h).  With `out`
    the sums are added into it."""
    lib = _lib.load()
    B, L, _ = grad_lmk.shape
    gv = out if out is not None else torch.empty(B, V, 3, device=grad_lmk.device, dtype=torch.float32)
    _lib.check(lib.msmd_landmarks_bwd(_p(grad_lmk), _p(faces_i32), _p(idx), L if idx.shape[0] > 1 else 0, _p(bc),
                                      L * 3 if bc.shape[0] > 1 else 0, _p(gv), B, V, L, int(out is not None), _stream()),
               "msmd_landmarks_bwd")
    return gv


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


class _LandmarksFn(torch.autograd.Function):
    """msmd_landmarks with msmd_landmarks_bwd: the gradient goes to the vertices only (index tables are integers, the
    barycentric tables are buffers)."""

    @staticmethod
    def forward(ctx, verts, faces_i32, idx, bc):
        ctx.save_for_backward(faces_i32, idx, bc)      # saved, so that an in-place change of a table before backward raises
        ctx.V = verts.shape[1]
        return _landmarks_launch(verts, faces_i32, idx, bc)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return landmarks_bwd(g.float().contiguous(), *ctx.saved_tensors, ctx.V), None, None, None


LANDMARKS_BWD_MAX_L = _h("LANDMARKS_BWD_MAX_L")   # msmd_landmarks_bwd keeps a frame's 3 L contributions in LDS (include/msmd_hip.h)


def landmarks(verts, faces_i32, lmk_faces_idx_i32, bary):
    """lmk_faces_idx: (L,) / (1, L) shared or (B, L) per frame; bary likewise (.., L, 3).  Differentiable (first order) with
    respect to verts: fp32-contiguous is then made by autograd ops, so the gradient returns in verts' dtype and layout."""
    idx = lmk_faces_idx_i32.reshape(-1, lmk_faces_idx_i32.shape[-1])
    bc = bary.reshape(-1, bary.shape[-2], 3)
    if _wants_grad(verts):
        if idx.shape[1] > LANDMARKS_BWD_MAX_L:
            raise ValueError(f"landmarks: the differentiable pass takes at most {LANDMARKS_BWD_MAX_L} landmarks per frame, "
                             f"got {idx.shape[1]}")
        return _LandmarksFn.apply(verts.float().contiguous(), faces_i32, idx, bc.detach())
    return _landmarks_launch(verts, faces_i32, idx, bc)


def dynamic_lmk_row(full_pose, neck_chain_i32, pose_is_matrix=False):
    lib = _lib.load()
    B = full_pose.shape[0]
    J = full_pose.shape[1] // (9 if pose_is_matrix else 3)
    row = torch.empty(B, device=full_pose.device, dtype=torch.int32)
    _lib.check(lib.msmd_dynamic_lmk_row(_p(full_pose), _p(neck_chain_i32), neck_chain_i32.shape[0], _p(row), B, J,
                                        int(pose_is_matrix), _stream()), "msmd_dynamic_lmk_row")
    return row


def _batch_rodrigues_launch(rot_vecs):
    lib = _lib.load()
    N = rot_vecs.shape[0]
    R = torch.empty(N, 3, 3, device=rot_vecs.device, dtype=torch.float32)
    _lib.check(lib.msmd_batch_rodrigues(_p(rot_vecs), _p(R), N, _stream()), "msmd_batch_rodrigues")
    return R


class _RodriguesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rot_vecs):
        ctx.save_for_backward(rot_vecs)
        return _batch_rodrigues_launch(rot_vecs)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (r,) = ctx.saved_tensors
        lib = _lib.load()
        gr = torch.empty_like(r)
        _lib.check(lib.msmd_batch_rodrigues_bwd(_p(r), _p(g.float().contiguous()), _p(gr), r.shape[0], _stream()),
                   "msmd_batch_rodrigues_bwd")
        return gr


def batch_rodrigues(rot_vecs):
    """rot_vecs: (N, 3) fp32 contiguous.  Differentiable (first order: msmd_batch_rodrigues_bwd)."""
    if _wants_grad(rot_vecs):
        return _RodriguesFn.apply(rot_vecs)
    return _batch_rodrigues_launch(rot_vecs)


def _rotation_launch(op, x, x2, out_shape, conv):
    lib = _lib.load()
    out = torch.empty(out_shape, device=x.device, dtype=torch.float32)
    _lib.check(lib.msmd_rotation_convert(op, _p(x), _p(x2), _p(out), x.numel() // _ROT_IN_WIDTH[op], conv, _stream()),
               "msmd_rotation_convert")
    return out


class _RotationFn(torch.autograd.Function):
    """msmd_rotation_convert with msmd_rotation_convert_bwd.  The forward's inputs are all the backward needs."""

    @staticmethod
    def forward(ctx, x, x2, op, out_shape, conv):
        ctx.save_for_backward(x, x2)
        ctx.op, ctx.conv = op, conv
        return _rotation_launch(op, x, x2, out_shape, conv)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, x2 = ctx.saved_tensors
        lib = _lib.load()
        g = g.float().contiguous()
        gx = torch.empty_like(x)
        gx2 = torch.empty_like(x2) if x2 is not None else None
        n = x.numel() // _ROT_IN_WIDTH[ctx.op]
        _lib.check(lib.msmd_rotation_convert_bwd(ctx.op, _p(x), _p(x2), _p(g), _p(gx), _p(gx2), n, ctx.conv, _stream()),
                   "msmd_rotation_convert_bwd")
        return gx, gx2, None, None, None


_ROT_IN_WIDTH = (4, 9, 3, 4, 3, 9, 6, 9, 3, 3, 9, 4, 4, 4, 4, 4)   # floats per item of the first operand, by MSMD_ROT_* op


def rotation_convert(op, x, in_width, out_shape_tail, x2=None, conv=0):
    """Generic elementwise rotation conversion: x (..., in_width[, in_width2]) -> (..., *out_shape_tail).  With grad mode on
    and an input that requires grad the call is differentiable (first order): the casts to contiguous fp32 below are then
    autograd ops, so gradients return in the inputs' dtype and layout (and reduce over broadcast dimensions)."""
    x = x.contiguous().float()
    lead = x.shape[:-1] if in_width in (3, 4, 6) else x.shape[:-2]
    out_shape = (*lead, *out_shape_tail)
    if x2 is not None:
        x2 = x2.contiguous().float()
    if _wants_grad(x, x2):
        return _RotationFn.apply(x, x2, op, out_shape, conv)
    return _rotation_launch(op, x, x2, out_shape, conv)


# ----------------------------------------------------------------------------- losses / training pieces
def masked_seq_loss(gt, pred, end_idx, c_lo, c_hi, order, prefix, criterion=0, mode=0, scale=1.0, return_ws=False):
    """0-dim fp32 tensor = scale * masked mean (see msmd_masked_seq_loss in include/msmd_hip.h); return_ws also hands
    back the workspace (valid-row count) that masked_seq_loss_bwd_ needs."""
    lib = _lib.load()
    _need_cuda(gt, pred)
    N, T, C = pred.shape
    out = torch.empty(1, device=pred.device, dtype=torch.float32)
    ws = torch.empty(2, device=pred.device, dtype=torch.float64)
    _lib.check(lib.msmd_masked_seq_loss(_p(gt), _p(pred), _p(end_idx), _p(out), _p(ws), N, T, C, c_lo, c_hi, order,
                                        prefix, criterion, mode, float(scale), _stream()), "msmd_masked_seq_loss")
    return (out[0], ws) if return_ws else out[0]


def masked_seq_loss_bwd_(grad_pred, gt, pred, end_idx, ws, upstream, c_lo, c_hi, order, prefix, criterion=0, mode=0,
                         scale=1.0):
    """grad_pred += d(masked_seq_loss) / d(pred) * upstream (0-dim device tensor)."""
    lib = _lib.load()
    N, T, C = pred.shape
    up = upstream.reshape(1).float().contiguous()
    _lib.check(lib.msmd_masked_seq_loss_bwd(_p(gt), _p(pred), _p(end_idx), _p(ws), _p(up), _p(grad_pred), N, T, C, c_lo,
                                            c_hi, order, prefix, criterion, mode, float(scale), _stream()),
               "msmd_masked_seq_loss_bwd")
    return grad_pred


def kl_loss(mu, logvar):
    lib = _lib.load()
    out = torch.empty(1, device=mu.device, dtype=torch.float32)
    ws = torch.empty(2, device=mu.device, dtype=torch.float64)
    _lib.check(lib.msmd_kl_loss(_p(mu), _p(logvar), _p(out), _p(ws), mu.numel(), _stream()), "msmd_kl_loss")
    return out[0]


def truncate_rows_(x, end_idx_i32, unit=1, replicate=False):
    """In place on x (N, L[, inner])."""
    lib = _lib.load()
    N, L = x.shape[0], x.shape[1]
    inner = x.numel() // (N * L)
    _lib.check(lib.msmd_truncate_rows(_p(x), _p(end_idx_i32), N, L, inner, unit, int(replicate), _stream()),
               "msmd_truncate_rows")
    return x


def adam_step_(param, grad, exp_avg, exp_avg_sq, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    lib = _lib.load()
    _lib.check(lib.msmd_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), float(lr),
                                  float(beta1), float(beta2), float(eps), int(step), float(grad_scale), _stream()),
               "msmd_adam_step")
    return param


# ----------------------------------------------------------------------------- backward building blocks
def gemm_batched2(a, w, out, M, N, K, lda, ldw, ldc, batch_outer, sA_o, sW_o, sC_o, batch_inner, sA_i, sW_i, sC_i):
    lib = _lib.load()
    _lib.check(lib.msmd_gemm_batched2(_p(a), _p(w), _p(out), M, N, K, _dt(a), _dt(out), lda, ldw, ldc, batch_outer,
                                      sA_o, sW_o, sC_o, batch_inner, sA_i, sW_i, sC_i, _stream()), "msmd_gemm_batched2")
    return out


def transpose(x, out, rows, cols, ldx, ldy, batch=1, sx=0, sy=0, batch_inner=1, sx_i=0, sy_i=0):
    lib = _lib.load()
    _lib.check(lib.msmd_transpose(_p(x), _p(out), rows, cols, ldx, ldy, batch, sx, sy, batch_inner, sx_i, sy_i, _dt(x),
                                  _stream()), "msmd_transpose")
    return out


def transpose2d(x, pad_to=8):
    """(rows, cols) -> (cols, rows_padded) with zero padding of the new inner dim to a multiple of `pad_to`."""
    rows, cols = x.shape
    rp = (rows + pad_to - 1) // pad_to * pad_to
    out = torch.zeros(cols, rp, device=x.device, dtype=x.dtype) if rp != rows else \
        torch.empty(cols, rp, device=x.device, dtype=x.dtype)
    return transpose(x, out, rows, cols, x.stride(0), rp)


def colsum(x2d, out=None, accumulate=False):
    """out[c] (+)= sum_r x2d[r, c] in fp32, deterministic (per-row-block partial sums added in block order)."""
    lib = _lib.load()
    rows, cols = x2d.shape
    if out is None:
        out = torch.empty(cols, device=x2d.device, dtype=torch.float32)
    nws = lib.msmd_colsum_workspace(rows, cols)
    ws = torch.empty(nws, device=x2d.device, dtype=torch.uint8)
    _lib.check(lib.msmd_colsum(_p(x2d), _p(out), rows, cols, x2d.stride(0), int(accumulate), _dt(x2d), _p(ws), nws, _stream()),
               "msmd_colsum")
    return out


def fold_weight_norm(g, v):
    """weight_norm(dim=2) of the positional conv, no autograd: w[o, i, k] = g[k] v[o, i, k] / ||v[:, :, k]||.  The norm
    is a column sum by msmd_colsum: the host library's multi-block reduction returned NaN from the second replay on when it
    sat inside a segmented hipGraph, so no pack / training graph uses it."""
    O, I, K = v.shape
    v2 = v.detach().reshape(O * I, K).float()
    s = g.detach().reshape(K).float() * torch.rsqrt(colsum((v2 * v2).contiguous()))
    return v.detach().float() * s.view(1, 1, K)


def act_fwd(z, act):
    lib = _lib.load()
    y = torch.empty_like(z)
    _lib.check(lib.msmd_act_fwd(_p(z), _p(y), z.numel(), act, _dt(z), _stream()), "msmd_act_fwd")
    return y


def person_query_attention(x, wq, bq, kv, n_heads, scale, wq_colsum=None, eps=1e-5):
    """Row 0 of every sequence of x (N, T, d): softmax(scale (x0 Wq^T + bq)_h K_h^T) V_h against kv (N, Tk, 2d) =
    [K | V]; returns (N, d).  One launch for the projection and the Tq = 1 attention (msmd_person_query_attention)."""
    _need_cuda(x, wq, kv)
    N, _, d = x.shape
    Tk = kv.shape[1]
    if kv.shape[2] != 2 * d or wq.shape[0] != d or wq.shape[1] != d or x.stride(2) != 1 or kv.stride(2) != 1:
        raise ValueError("person_query_attention: shapes")
    if not (x.dtype == wq.dtype == kv.dtype):
        raise TypeError("person_query_attention: x, wq, kv must share a dtype")
    out = torch.empty(N, d, device=x.device, dtype=x.dtype)
    if wq_colsum is not None:      # the LayerNorm in front of the projection folded in (wq / bq folded, x un-normalised)
        _lib.check(_lib.load().msmd_person_query_attention_ln(_p(x), x.stride(0), _p(wq), _p(bq), _p(wq_colsum), float(eps),
                                                              _p(kv), _p(kv[..., d:]), kv.stride(0), kv.stride(1), _p(out),
                                                              N, n_heads, Tk, d, float(scale), _dt(x), _stream()),
                   "msmd_person_query_attention_ln")
        return out
    _lib.check(_lib.load().msmd_person_query_attention(_p(x), x.stride(0), _p(wq), _p(bq), _p(kv), _p(kv[..., d:]),
                                                       kv.stride(0), kv.stride(1), _p(out), N, n_heads, Tk, d,
                                                       float(scale), _dt(x), _stream()), "msmd_person_query_attention")
    return out


def cast_transpose_multi(flat, meta, n, tiles, cast_arena, t_arena):
    """One launch: bf16 cast + bf16 transpose of n (N, K) matrices of the flat fp32 arena (meta: see msmd_hip.h)."""
    _need_cuda(flat, meta, cast_arena, t_arena)
    _lib.check(_lib.load().msmd_cast_transpose_multi(_p(flat), _p(meta), int(n), int(tiles), _p(cast_arena),
                                                     _p(t_arena), _stream()), "msmd_cast_transpose_multi")


def act_bwd_dropout(dy, z, act, p, rng_state, site):
    """dz = dropout_mask(dy) * act'(z) (one pass; mask of the forward msmd_gemm_ex / msmd_dropout)."""
    dz = torch.empty_like(z)
    _lib.check(_lib.load().msmd_act_bwd_dropout(_p(dy), _p(z), _p(dz), z.numel(), act, float(p), _p(rng_state),
                                                int(site), _dt(z), _stream()), "msmd_act_bwd_dropout")
    return dz


def act_bwd(dy, z, act):
    lib = _lib.load()
    dz = torch.empty_like(z)
    _lib.check(lib.msmd_act_bwd(_p(dy), _p(z), _p(dz), z.numel(), act, _dt(z), _stream()), "msmd_act_bwd")
    return dz


def layernorm_bwd(dy, x, gamma, eps=1e-5, dg_out=None, db_out=None, drop=None):
    """dx, dgamma, dbeta.  With dg_out / db_out (fp32, cols) the parameter gradients are ACCUMULATED into those
    buffers (e.g. the parameters' .grad views) instead of fresh tensors.  drop = (p, rng_state, site): the launch also
    writes dropout_mask(dx) / (1 - p) (what the Linear in front of the LayerNorm wants); returned as a 4th value."""
    lib = _lib.load()
    cols = x.shape[-1]
    rows = x.numel() // cols
    dx = torch.empty_like(x)
    if dg_out is None:
        dgb = torch.zeros(2, cols, device=x.device, dtype=torch.float32)
        dg, db = dgb[0], dgb[1]
    else:
        dg, db = dg_out, db_out
    nws = lib.msmd_layernorm_bwd_workspace(rows, cols)
    ws = torch.empty(nws, device=x.device, dtype=torch.uint8)
    if drop is not None:
        p_drop, rng_state, site = drop
        dxd = torch.empty_like(x)
        _lib.check(lib.msmd_layernorm_bwd_dropout(_p(dy), _p(x), _p(gamma), _p(dx), _p(dxd), _p(dg), _p(db), rows, cols, eps,
                                                  float(p_drop), _p(rng_state), int(site), _dt(x), _p(ws), nws, _stream()),
                   "msmd_layernorm_bwd_dropout")
        return dx, dg, db, dxd
    _lib.check(lib.msmd_layernorm_bwd(_p(dy), _p(x), _p(gamma), _p(dx), _p(dg), _p(db), rows, cols, eps, _dt(x),
                                      _p(ws), nws, _stream()), "msmd_layernorm_bwd")
    return dx, dg, db


def softmax_rows_(s, cols, ld, Tq, scale, mask=None):
    lib = _lib.load()
    rows = s.numel() // ld
    _lib.check(lib.msmd_softmax_rows(_p(s), _p(mask), rows, cols, ld, Tq, float(scale), _dt(s), _stream()),
               "msmd_softmax_rows")
    return s


def softmax_bwd_rows_(P, dP, cols, ld, scale):
    lib = _lib.load()
    rows = P.numel() // ld
    _lib.check(lib.msmd_softmax_bwd_rows(_p(P), _p(dP), rows, cols, ld, float(scale), _dt(P), _stream()),
               "msmd_softmax_bwd_rows")
    return dP


def unfold_t(xp, T, Kk):
    """xp (B, G, Tp, Cg) -> (G, Kk*Cg, Mp) with Mp = B*T rounded up to 8 (zero padded)."""
    lib = _lib.load()
    B, G, Tp, Cg = xp.shape
    Mp = (B * T + 7) // 8 * 8
    out = torch.empty(G, Kk * Cg, Mp, device=xp.device, dtype=xp.dtype)
    _lib.check(lib.msmd_unfold_t(_p(xp), _p(out), B, T, Tp, G, Cg, Kk, Mp, _dt(xp), _stream()), "msmd_unfold_t")
    return out


# ----------------------------------------------------------------------------- mesh renderer (csrc/render.hip)
def _arg(name, t, dtype, shape=None, sizes=None, optional=False):
    """The entry points from here on index raw pointers from the stated sizes: t is a contiguous device tensor of one dtype whose
    shape fits `shape` ("B V 3" or a tuple of such entries), TypeError otherwise.  An integer is exact; a name binds in `sizes` (a dict
    the wrapper's calls share) where first seen and must agree afterwards, "n+" is at least 1; a tuple such as (3, 4) is a set."""
    if t is None and optional:
        return
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous {dtype} CUDA tensor")
    if shape is None:
        return
    entries = [e if isinstance(e, tuple) else str(e) for e in (shape.split() if isinstance(shape, str) else shape)]
    known = {} if sizes is None else sizes
    bound = dict(known)
    ok = t.dim() == len(entries)
    for e, n in zip(entries, t.shape):
        if isinstance(e, tuple):
            ok &= n in e
        elif e.isdigit():
            ok &= n == int(e)
        else:
            ok &= n == bound.setdefault(e.rstrip("+"), n) and n >= e.count("+")
    if not ok:
        want = (" | ".join(map(str, e)) if isinstance(e, tuple) else str(known.get(e.rstrip("+"), e.rstrip("+"))) for e in entries)
        raise TypeError(f"{name} must have shape ({', '.join(want)}{',' * (len(entries) == 1)}), got {tuple(t.shape)}")
    known.update(bound)


def render_vertices(verts, faces_i32, csr_offsets, csr_faces, view, focal, height, width, t_center=None, rot=None):
    """-> (screen (B, V, 3) = (x_s, y_s, eye depth), normals (B, V, 3) eye-space unit vertex normals): msmd_render_vertices.
    verts (B, V, 3) fp32; faces (F, 3), csr_offsets (V + 1), csr_faces (3 F) int32 (utils/renderer.vertex_face_csr);
    view (3, 4) fp32 world -> eye; rot (B, 3) axis-angle about t_center (3), both or neither."""
    d = {}
    _arg("verts", verts, torch.float32, "B V 3", d)
    _arg("faces", faces_i32, torch.int32, "F 3", d)
    B, V, Fc = d["B"], d["V"], d["F"]
    _arg("csr_offsets", csr_offsets, torch.int32, (V + 1,))
    _arg("csr_faces", csr_faces, torch.int32, (3 * Fc,))
    _arg("view", view, torch.float32, "3 4")
    if (rot is None) != (t_center is None):
        raise TypeError("rot and t_center are given together")
    _arg("rot", rot, torch.float32, "B 3", d, optional=True)
    _arg("t_center", t_center, torch.float32, "3", optional=True)
    lib = _lib.load()
    screen = torch.empty(B, V, 3, device=verts.device, dtype=torch.float32)
    normals = torch.empty(B, V, 3, device=verts.device, dtype=torch.float32)
    _lib.check(lib.msmd_render_vertices(_p(verts), _p(faces_i32), _p(csr_offsets), _p(csr_faces), _p(view), _p(t_center),
                                        _p(rot), _p(screen), _p(normals), B, V, Fc, float(focal), int(height), int(width),
                                        _stream()), "msmd_render_vertices")
    return screen, normals


RENDER_SAMPLES = (1, 4)


def render_raster(screen, normals, faces_i32, shade, lights, height, width, near, far, background, want_face_id=False, samples=1,
                  want_sample_depth=False):
    """-> (rgba (B, H, W, 4) uint8, depth (B, H, W) fp32, face_id (B, H, W) int32 or None): msmd_render_raster.
    screen / normals (B, V, 3) fp32 as render_vertices returns them; shade (6) = base rgb, ambient rgb; lights (L, 4) =
    eye-space unit direction towards the light, intensity; background = R | G << 8 | B << 16 | A << 24.
    samples = 4 (msmd_render_raster_ms) rasterises and shades four sample points per pixel: rgba is their
    resolve, depth the least depth over the pixel's covered samples, face_id (B, H, W, 4) per sample.  want_sample_depth
    appends sample_depth to the result: (B, H, W, 4) fp32 at four samples, 0 on an uncovered sample; (B, H, W), a copy of
    depth, at one (that call goes through msmd_render_raster_ms as well)."""
    d = {}
    _arg("screen", screen, torch.float32, "B V 3", d)
    _arg("normals", normals, torch.float32, "B V 3", d)
    _arg("faces", faces_i32, torch.int32, "F 3", d)
    _arg("shade", shade, torch.float32, "6")
    _arg("lights", lights, torch.float32, "L 4", d)
    if samples not in RENDER_SAMPLES:
        raise ValueError(f"samples must be one of {RENDER_SAMPLES}, got {samples!r}")
    B, V, H, W = d["B"], d["V"], int(height), int(width)
    lib = _lib.load()
    per_sample = (B, H, W) if samples == 1 else (B, H, W, samples)
    rgba = torch.empty(B, H, W, 4, device=screen.device, dtype=torch.uint8)
    depth = torch.empty(B, H, W, device=screen.device, dtype=torch.float32)
    face_id = torch.empty(per_sample, device=screen.device, dtype=torch.int32) if want_face_id else None
    head = (_p(screen), _p(normals), _p(faces_i32), _p(shade), _p(lights), lights.shape[0], _p(rgba), _p(depth), _p(face_id))
    tail = (B, V, faces_i32.shape[0], H, W, float(near), float(far), int(background) & 0xffffffff)
    if samples == 1 and not want_sample_depth:
        _lib.check(lib.msmd_render_raster(*head, *tail, _stream()), "msmd_render_raster")
        return rgba, depth, face_id
    sample_depth = torch.empty(per_sample, device=screen.device, dtype=torch.float32) if want_sample_depth else None
    _lib.check(lib.msmd_render_raster_ms(*head, _p(sample_depth), *tail, int(samples), _stream()), "msmd_render_raster_ms")
    return (rgba, depth, face_id, sample_depth) if want_sample_depth else (rgba, depth, face_id)


TEXTURE_MAX_SIDE = _h("TEXTURE_MAX_SIDE")


def texture_pyramid(img_u8):
    """(Ht, Wt, 3 | 4) uint8 image on the device (alpha ignored) -> its mip pyramid, (n_texels, 4) fp32 RGBA texels with the
    levels one after the other (level l + 1 is max(1, H_l >> 1) x max(1, W_l >> 1)): msmd_texture_mips."""
    _arg("img", img_u8, torch.uint8, ("Ht", "Wt", (3, 4)))
    Ht, Wt, C = img_u8.shape
    lib = _lib.load()
    n = lib.msmd_texture_texels(Ht, Wt)
    if n < 0:
        raise ValueError(f"a {Ht} x {Wt} texture is outside [1, {TEXTURE_MAX_SIDE}]")
    pyramid = torch.empty(n, 4, device=img_u8.device, dtype=torch.float32)
    _lib.check(lib.msmd_texture_mips(_p(img_u8), Ht, Wt, C, _p(pyramid), _stream()), "msmd_texture_mips")
    return pyramid


def _deferred_pass_args(screen, normals, faces_i32, shade, lights, face_id, rgba, samples, background):
    """What the deferred passes refuse and check alike -> the sizes their tensors bind (B, V, F, L, H, W)."""
    if samples not in RENDER_SAMPLES:
        raise ValueError(f"samples must be one of {RENDER_SAMPLES}, got {samples!r}")
    if samples != 1 and background is None:
        raise ValueError("samples=4 needs the background the raster pass was given: its uncovered samples take part in the resolve")
    d = {}
    _arg("screen", screen, torch.float32, "B V 3", d)
    _arg("normals", normals, torch.float32, "B V 3", d)
    _arg("faces", faces_i32, torch.int32, "F 3", d)
    _arg("shade", shade, torch.float32, "6")
    _arg("lights", lights, torch.float32, "L 4", d)
    _arg("face_id", face_id, torch.int32, "B H W" if samples == 1 else f"B H W {samples}", d)
    _arg("rgba", rgba, torch.uint8, "B H W 4", d)
    return d


def render_shade_textured(screen, normals, faces_i32, vt, ft, pyramid, tex_height, tex_width, shade, lights, face_id, rgba, near,
                          want_uvl=False, samples=1, background=None):
    """Overwrites rgba (B, H, W, 4) uint8 at the pixels face_id (B, H, W) int32 marks as covered with the mip-mapped,
    trilinearly sampled texture under render_raster's lighting: msmd_render_shade_textured.  screen / normals / faces / shade /
    lights as render_raster takes them; vt (Nt, 2) fp32, ft (F, 3) int32 per-corner indices into vt; pyramid as
    texture_pyramid returns it for a tex_height x tex_width image.  -> uvl (B, H, W, 3) fp32 = (u, v, lambda) per pixel (zeros
    on the background) if want_uvl, else None.
    samples = 4 (msmd_render_shade_textured_ms): face_id is render_raster's (B, H, W, 4) at four samples, every
    covered sample is shaded at its own position and every pixel with a covered sample receives the resolve of its four, an
    uncovered sample counting as `background` (R | G << 8 | B << 16 | A << 24, the one render_raster was given: required).
    There is no uvl at four samples: want_uvl is a ValueError."""
    d = _deferred_pass_args(screen, normals, faces_i32, shade, lights, face_id, rgba, samples, background)
    if samples != 1 and want_uvl:
        raise ValueError("(u, v, level of detail) is per pixel: it is not offered at four samples per pixel")
    _arg("vt", vt, torch.float32, "Nt+ 2", d)
    _arg("ft", ft, torch.int32, "F 3", d)
    B, V, Fc, H, W = (d[k] for k in "BVFHW")
    lib = _lib.load()
    Ht, Wt = int(tex_height), int(tex_width)
    n = lib.msmd_texture_texels(Ht, Wt)
    if n < 0:
        raise ValueError(f"a {Ht} x {Wt} texture is outside [1, {TEXTURE_MAX_SIDE}]")
    _arg("pyramid", pyramid, torch.float32, (n, 4))
    if samples != 1:
        _lib.check(lib.msmd_render_shade_textured_ms(_p(screen), _p(normals), _p(faces_i32), _p(vt), _p(ft), _p(pyramid), Ht, Wt,
                                                     _p(shade), _p(lights), lights.shape[0], _p(face_id), _p(rgba), B, V, Fc,
                                                     vt.shape[0], H, W, float(near), int(background) & 0xffffffff, int(samples),
                                                     _stream()), "msmd_render_shade_textured_ms")
        return None
    uvl = torch.empty(B, H, W, 3, device=screen.device, dtype=torch.float32) if want_uvl else None
    _lib.check(lib.msmd_render_shade_textured(_p(screen), _p(normals), _p(faces_i32), _p(vt), _p(ft), _p(pyramid), Ht, Wt,
                                              _p(shade), _p(lights), lights.shape[0], _p(face_id), _p(rgba), _p(uvl), B, V, Fc,
                                              vt.shape[0], H, W, float(near), _stream()), "msmd_render_shade_textured")
    return uvl


def render_shade_vertex_color(screen, normals, faces_i32, vcol, shade, lights, face_id, rgba, near, lit=True, samples=1,
                              background=None):
    """Overwrites rgba (B, H, W, 4) uint8 at the pixels face_id marks as covered with the colour interpolated from the vertices:
    msmd_render_shade_vertex_color.  screen / normals / faces / shade / lights / face_id as render_shade_textured
    takes them; vcol (V, 4) uint8 RGBA per vertex (alpha ignored), shared by the frames, or (B, V, 4) per frame.  lit=True
    multiplies the colour by render_raster's lighting as a texel is; lit=False stores the interpolated colour itself.  samples = 4:
    face_id is (B, H, W, 4), every covered sample is shaded at its own position and `background` (the one render_raster was
    given: required) stands for the uncovered samples of a pixel that has a covered one."""
    d = _deferred_pass_args(screen, normals, faces_i32, shade, lights, face_id, rgba, samples, background)
    per_frame = torch.is_tensor(vcol) and vcol.dim() == 3
    _arg("vcol", vcol, torch.uint8, "B V 4" if per_frame else "V 4", d)
    B, V, Fc, H, W = (d[k] for k in "BVFHW")
    _lib.check(_lib.load().msmd_render_shade_vertex_color(_p(screen), _p(normals), _p(faces_i32), _p(vcol), int(per_frame), int(bool(lit)),
                                                          _p(shade), _p(lights), lights.shape[0], _p(face_id), _p(rgba), B, V, Fc, H, W,
                                                          float(near), 0 if background is None else int(background) & 0xffffffff,
                                                          int(samples), _stream()), "msmd_render_shade_vertex_color")


# ----------------------------------------------------------------------------- FLAMETex albedo model (csrc/flametex.hip)
TEX_PLANAR_F32, TEX_IMAGE_U8 = _h("TEX_PLANAR_F32", "TEX_IMAGE_U8")
FLAMETEX_MAX_SIDE, FLAMETEX_MAX_TEX = _h("FLAMETEX_MAX_SIDE", "FLAMETEX_MAX_TEX")


def _flametex_sizes(basis, src_hw, dst_hw):
    (Hs, Ws), (Hd, Wd) = (int(v) for v in src_hw), (int(v) for v in dst_hw)
    _arg("basis", basis, torch.float32, "rows n_tex")
    n_tex = basis.shape[1]
    if not all(1 <= v <= FLAMETEX_MAX_SIDE for v in (Hs, Ws, Hd, Wd)) or not 1 <= n_tex <= FLAMETEX_MAX_TEX:
        raise ValueError(f"flametex: sides {(Hs, Ws, Hd, Wd)} outside [1, {FLAMETEX_MAX_SIDE}] or n_tex = {n_tex} outside "
                         f"[1, {FLAMETEX_MAX_TEX}]")
    if basis.shape[0] != Hs * Ws * 3:
        raise ValueError(f"basis has {basis.shape[0]} rows for a {Hs} x {Ws} x 3 image")
    return Hs, Ws, Hd, Wd, n_tex


def flametex_forward(mean, basis, code, n_copies=1, src_hw=(512, 512), dst_hw=(256, 256), out_format=TEX_PLANAR_F32):
    """mean (Hs Ws 3) + basis (Hs Ws 3, n_tex) . code (n_tex), nearest-resized to dst_hw and channel-reversed, in one pass over
    the rows the resize keeps: msmd_flametex_forward.  -> (n_copies, 3, Hd, Wd) fp32 (TEX_PLANAR_F32) or (Hd, Wd, 3) uint8 RGB
    (TEX_IMAGE_U8, n_copies = 1).  All operands contiguous fp32 on the device."""
    Hs, Ws, Hd, Wd, n_tex = _flametex_sizes(basis, src_hw, dst_hw)
    _arg("mean", mean, torch.float32, (Hs * Ws * 3,))
    _arg("code", code, torch.float32, (n_tex,))
    n_copies = int(n_copies)
    if out_format == TEX_IMAGE_U8:
        if n_copies != 1:
            raise ValueError("flametex_forward: the uint8 image has one copy")
        out = torch.empty(Hd, Wd, 3, device=basis.device, dtype=torch.uint8)
    elif out_format == TEX_PLANAR_F32:
        if n_copies < 0:
            raise ValueError(f"flametex_forward: n_copies = {n_copies}")
        out = torch.empty(n_copies, 3, Hd, Wd, device=basis.device, dtype=torch.float32)
    else:
        raise ValueError(f"flametex_forward: out_format {out_format!r}")
    _lib.check(_lib.load().msmd_flametex_forward(_p(mean), _p(basis), _p(code), _p(out), out_format, n_copies, Hs, Ws, Hd, Wd,
                                                 n_tex, _stream()), "msmd_flametex_forward")
    return out


def flametex_backward(basis, grad_out, src_hw=(512, 512), out=None):
    """grad_out (n_copies, 3, Hd, Wd) fp32 -> the gradient of flametex_forward's code, (n_tex,) fp32, summed over the copies:
    msmd_flametex_backward (per-workgroup partial sums in a workspace, then one ordered reduction; the same bits every run).
    out: a contiguous (n_tex,) fp32 tensor to write instead of a new one."""
    _arg("grad_out", grad_out, torch.float32, "n_copies 3 Hd Wd")
    Hs, Ws, Hd, Wd, n_tex = _flametex_sizes(basis, src_hw, grad_out.shape[2:])
    lib = _lib.load()
    workspace = torch.empty(lib.msmd_flametex_backward_workspace(Hd, Wd, n_tex), device=basis.device, dtype=torch.float32)
    _arg("out", out, torch.float32, (n_tex,), optional=True)
    grad_code = out if out is not None else torch.empty(n_tex, device=basis.device, dtype=torch.float32)
    _lib.check(lib.msmd_flametex_backward(_p(basis), _p(grad_out), grad_out.shape[0], _p(grad_code), _p(workspace), Hs, Ws, Hd,
                                          Wd, n_tex, _stream()), "msmd_flametex_backward")
    return grad_code


# ----------------------------------------------------------------------------- JPEG codec (csrc/jpeg.hip, csrc/jpeg_decode.hip)
# The file format (tables, header writer, parser, decode plan) is host code in jpeg_format.py; what follows launches.
from .jpeg_format import (JPEG_420, JPEG_422, JPEG_444, JPEG_BASE_CHROMA, JPEG_BASE_LUMA, JPEG_DECODE_LANES,  # noqa: E402,F401
                          JPEG_ERR_CODE, JPEG_ERR_NAMES, JPEG_ERR_OVERRUN, JPEG_ERR_RESTART, JPEG_ERR_RUN, JPEG_GREY, JPEG_HUFFMAN,
                          JPEG_MAX_SIDE, JPEG_RESTART_INTERVAL, JPEG_TABLE_SET_BYTES, JPEG_ZIGZAG, _jpeg_plan, jpeg_header,
                          jpeg_layout_geometry, jpeg_parse, jpeg_quant_table, jpeg_status_text)


def _u8_tensor(frames):
    """The TypeErrors of `_u8_frames` that need no sizes: a caller with a check of its own (the encoder's quality) runs these,
    its check, then `_u8_frames`, so a call that is wrong in two ways reports what it always did."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise TypeError("frames must be a uint8 tensor")
    if not frames.is_cuda:
        raise TypeError("frames must be on the MI355X (cuda) device; there is no CPU encoder")
    if frames.dim() != 4 or frames.shape[3] not in (3, 4):
        raise TypeError(f"frames must have shape (B, H, W, 3 | 4), got {tuple(frames.shape)}")


def _u8_frames(frames):
    """Checks of (B, H, W, 3 | 4) uint8 device frames and their strides -> (B, H, W, frame stride, row stride, pixel stride).
    The kernels (msmd_jpeg_coefficients, msmd_face_crop) index raw pointers from these numbers."""
    _u8_tensor(frames)
    B, H, W, C = frames.shape
    if B < 1 or not (1 <= H <= JPEG_MAX_SIDE and 1 <= W <= JPEG_MAX_SIDE):
        raise ValueError(f"frames of shape {tuple(frames.shape)}: B >= 1 and 1 <= H, W <= {JPEG_MAX_SIDE} are required")
    sb, sh, sw, sc = frames.stride()
    if sc != 1 or sw not in (3, 4) or sw < C or sh < W * sw - (sw - C) or (B > 1 and sb < H * sh - (sh - W * sw)) :
        raise TypeError(f"frames with strides {frames.stride()}: channels must be adjacent bytes, pixels 3 or 4 bytes apart, "
                        "rows and frames must not overlap (call .contiguous())")
    if sw == 4 and C == 3:
        # the (B, H, W, 3) view of an RGBA buffer: the kernel reads whole 4-byte pixels, so the last alpha byte must exist
        last = frames.storage_offset() + (B - 1) * sb + (H - 1) * sh + (W - 1) * sw + 4
        if last > frames.untyped_storage().nbytes():
            raise TypeError("frames is a 3-channel view with 4-byte pixels whose storage ends before the last pixel's 4th byte")
    return B, H, W, sb, sh, sw


def _jpeg_launch_coefficients(frames, quality):
    """The encoder's checks and its first launch, msmd_jpeg_coefficients -> (coef (B n_int 32 3 64,) int16, n_int)."""
    _u8_tensor(frames)
    jpeg_quant_table(JPEG_BASE_LUMA, quality)           # the quality's ValueError
    B, H, W, sb, sh, sw = _u8_frames(frames)
    lib = _lib.load()
    n_int = lib.msmd_jpeg_intervals(H, W)
    coef = torch.empty(B * n_int * JPEG_RESTART_INTERVAL * 3 * 64, device=frames.device, dtype=torch.int16)
    _lib.check(lib.msmd_jpeg_coefficients(_p(frames), sb, sh, sw, B, H, W, int(quality), _p(coef), _stream()), "msmd_jpeg_coefficients")
    return coef, n_int


def jpeg_coefficients(frames, quality=90):
    """-> (B, n_mcu, 3, 64) int16: the quantised DCT coefficients of every MCU (Y, Cb, Cr) in zig-zag order, MCUs in raster
    order over the frame padded to multiples of 8: msmd_jpeg_coefficients."""
    coef, n_int = _jpeg_launch_coefficients(frames, quality)
    B, H, W, _ = frames.shape
    return coef.view(B, n_int * JPEG_RESTART_INTERVAL, 3, 64)[:, :((H + 7) // 8) * ((W + 7) // 8)]


@functools.lru_cache(maxsize=16)
def _jpeg_header_on(H, W, quality, device):
    """`jpeg_header` as a uint8 tensor on the device of that name: uploaded once for the calls of a video."""
    return torch.frombuffer(bytearray(jpeg_header(H, W, quality)), dtype=torch.uint8).to(device)


def jpeg_encode(frames, quality=90):
    """frames (B, H, W, 3 | 4) uint8 on the device (alpha ignored; a row stride larger than the row and the renderer's
    (B, H, W, 3) view of its RGBA buffer are taken as they are) -> (stream (n,) uint8, offsets (B + 1,) int64), both on the
    device: frame b is the JFIF file stream[offsets[b]:offsets[b + 1]].  Baseline, 4:4:4, Annex K tables, restart interval 32;
    the bytes are a pure function of the pixels.  Five launches and one host read (the stream's length)."""
    coef, n_int = _jpeg_launch_coefficients(frames, quality)
    B, H, W, _ = frames.shape
    lib = _lib.load()
    dev = frames.device
    header = _jpeg_header_on(H, W, int(quality), str(dev))
    interval_len = torch.empty(B * n_int, device=dev, dtype=torch.int32)
    interval_rel = torch.empty(B * n_int, device=dev, dtype=torch.int64)
    frame_size = torch.empty(B, device=dev, dtype=torch.int64)
    offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    st = _stream()
    _lib.check(lib.msmd_jpeg_measure(_p(coef), B, H, W, header.numel(), _p(interval_len), _p(interval_rel), _p(frame_size),
                                     _p(offsets), st), "msmd_jpeg_measure")
    total = int(offsets[B].item())                      # the one device-to-host read: the output cannot be allocated without it
    out = torch.empty(total, device=dev, dtype=torch.uint8)
    _lib.check(lib.msmd_jpeg_write(_p(coef), B, H, W, _p(header), header.numel(), _p(interval_rel), _p(offsets), _p(out), total,
                                   st), "msmd_jpeg_write")
    return out, offsets


def _jpeg_upload(plan, device):
    up = lambda a: torch.from_numpy(a).to(device)
    return up(plan.stream), up(plan.intervals), up(plan.sets.copy()), up(plan.frame_set), up(plan.status)


def _jpeg_decode_coefficients(plan, device):
    lib = _lib.load()
    stream, intervals, sets, frame_set, status = _jpeg_upload(plan, device)
    coef = torch.empty(plan.B, plan.blocks, 64, device=device, dtype=torch.int16)
    _lib.check(lib.msmd_jpeg_decode_coefficients(_p(stream), stream.numel(), _p(intervals), intervals.shape[0], _p(sets), plan.n_sets,
                                                 plan.B, plan.H, plan.W, plan.layout, plan.ri, _p(coef), _p(status), _stream()),
               "msmd_jpeg_decode_coefficients")
    return coef, status, sets, frame_set


def _jpeg_device(device):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("msmd_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    return device


def jpeg_decode_coefficients(files, device=None):
    """files as `jpeg_decode` takes them -> (coef (B, blocks, 64) int16 on the device, status (B,) int32): the entropy decode alone,
    msmd_jpeg_decode_coefficients.  Zig-zag order; the blocks of a frame are its component planes one after the other, each in
    block-raster order over the plane padded to whole MCUs (`jpeg_layout_geometry`)."""
    device = _jpeg_device(device)
    coef, status, _, _ = _jpeg_decode_coefficients(_jpeg_plan(files), device)
    return coef, status


def jpeg_decode(files, channels=3, strict=True, out=None, device=None):
    """Baseline JPEG files -> pixels (B, H, W, channels) uint8 on the device (integer arithmetic, the pixels are
    a pure function of the files' bytes).  files: a list of bytes-like objects, or (uint8 array holding the files back to back,
    B + 1 offsets) on the host, which is what `jpeg_encode` returns after `.cpu()`.  All files of a call share height, width,
    component count, sampling and restart interval; tables may differ.  channels 3 (RGB) or 4 (RGBA, alpha 255, one word per pixel).  out: a
    contiguous (B, H, W, channels) uint8 device tensor to write instead of a new one.  A file outside the accepted subset raises
    ValueError before any launch (`jpeg_format.jpeg_parse`).  strict: a damaged stream (a non-zero status) raises ValueError naming
    the frames and the kinds, which costs one device-to-host read; otherwise -> (pixels, status (B,) int32 on the device).  Three
    launches and a fill, five uploads."""
    if out is not None:
        _need_cuda(out)
    if channels not in (3, 4):
        raise ValueError(f"channels must be 3 or 4, got {channels!r}")
    plan = _jpeg_plan(files)
    _arg("out", out, torch.uint8, (plan.B, plan.H, plan.W, channels), optional=True)
    if out is not None and out.data_ptr() % 4:
        raise TypeError("out must start at a multiple of 4 bytes (the pixel kernel stores words)")
    device = out.device if out is not None else _jpeg_device(device)
    lib = _lib.load()
    coef, status, sets, frame_set = _jpeg_decode_coefficients(plan, device)
    planes = torch.empty(plan.B, plan.blocks * 64, device=device, dtype=torch.uint8)
    _lib.check(lib.msmd_jpeg_decode_planes(_p(coef), _p(sets), plan.n_sets, _p(frame_set), plan.B, plan.H, plan.W, plan.layout,
                                           _p(planes), _stream()), "msmd_jpeg_decode_planes")
    pixels = out if out is not None else torch.empty(plan.B, plan.H, plan.W, channels, device=device, dtype=torch.uint8)
    _lib.check(lib.msmd_jpeg_decode_pixels(_p(planes), plan.B, plan.H, plan.W, plan.layout, channels, _p(pixels), _stream()),
               "msmd_jpeg_decode_pixels")
    if not strict:
        return pixels, status
    bad = status.cpu().tolist()
    if any(bad):
        raise ValueError("damaged JPEG stream: " + jpeg_status_text(bad))
    return pixels


# ----------------------------------------------------------------------------- audio front end (csrc/audio_io.hip)
AUDIO_RUN, AUDIO_MAX_CLIPS = _h("AUDIO_RUN", "AUDIO_MAX_CLIPS")     # outputs per partial-sum pair; clips per call


def _audio_desc(desc, desc_host, pcm_elems=None):
    """desc (n, 5) int64 on the device and the host array it was copied from.  The kernels index raw pointers from these
    numbers, so the host copy is checked here: every clip inside the PCM buffer, output ranges disjoint and in order."""
    _arg("desc", desc, torch.int64)
    h = desc_host.numpy() if torch.is_tensor(desc_host) else desc_host
    if h.ndim != 2 or h.shape[1] != 5 or h.shape[0] == 0 or str(h.dtype) != "int64" or tuple(desc.shape) != tuple(h.shape):
        raise TypeError("desc_host must be the (n_clips, 5) int64 array desc was copied from")
    if h.shape[0] > AUDIO_MAX_CLIPS:
        raise ValueError(f"{h.shape[0]} clips in one call: the audio entry points take at most {AUDIO_MAX_CLIPS} (the clip is the "
                         "grid's y index); utils/audio.load_clips splits larger groups")
    end = 0
    for in_off, frames, channels, out_off, out_len in h.tolist():
        if frames <= 0 or channels <= 0 or out_len <= 0 or in_off < 0 or out_off < end:
            raise ValueError(f"bad clip descriptor {(in_off, frames, channels, out_off, out_len)}")
        if pcm_elems is not None and in_off + frames * channels > pcm_elems:
            raise ValueError(f"clip descriptor {(in_off, frames, channels)} runs past the {pcm_elems} PCM samples")
        end = out_off + out_len
    return h, end


def resample_audio(pcm, desc, desc_host, bank, L, M):
    """-> (out (sum of output lengths) fp32 16 kHz mono, partials (n_clips, runs, 2) float64): msmd_audio_resample.
    pcm: 1-D int16 or fp32 interleaved samples of a group of clips of one rate; desc / desc_host (n_clips, 5) int64 = [sample
    offset in pcm, frames, channels, offset in out, output length ceil(frames L / M)], on the device and on the host;
    bank (taps, L) fp32 from utils/audio.filter_bank, or None with L = M = 1 (same rate: the downmix itself)."""
    if not torch.is_tensor(pcm) or not pcm.is_cuda or pcm.dim() != 1 or not pcm.is_contiguous() or \
            pcm.dtype not in (torch.int16, torch.float32):
        raise TypeError("pcm must be a contiguous 1-D int16 or float32 CUDA tensor")
    h, total = _audio_desc(desc, desc_host, pcm.numel())
    L, M = int(L), int(M)
    for _, frames, _, _, out_len in h.tolist():
        if out_len != (frames * L + M - 1) // M:
            raise ValueError(f"output length {out_len} is not ceil({frames} * {L} / {M})")
    if bank is None:
        if (L, M) != (1, 1):
            raise ValueError("resample_audio: no filter bank is the same-rate bypass, L = M = 1")
        taps = 0
    else:
        _arg("bank", bank, torch.float32, ("taps", L))
        taps = bank.shape[0]
    lib = _lib.load()
    max_out = int(h[:, 4].max())
    out = torch.empty(total, device=pcm.device, dtype=torch.float32)
    partials = torch.empty(h.shape[0], (max_out + AUDIO_RUN - 1) // AUDIO_RUN, 2, device=pcm.device, dtype=torch.float64)
    code = lib.msmd_audio_resample(_p(pcm), pcm.numel(), int(pcm.dtype == torch.int16), _p(desc), h.shape[0], max_out, L, M,
                                   taps, _p(bank), _p(out), total, _p(partials), _stream())
    if code == 1:
        raise ValueError(f"msmd_audio_resample does not take L = {L}, M = {M}, taps = {taps}: a run's staged span of "
                         f"{(AUDIO_RUN - 1) * M // L + 2 + taps} samples must fit 64 KB of LDS, taps even and >= 4 (or 0 with L = M = 1)")
    _lib.check(code, "msmd_audio_resample")
    return out, partials


def znorm_audio(out, desc, desc_host, partials):
    """In place (y - mean) / (std + 1e-5) per clip, population std: msmd_audio_znorm on what resample_audio returned (one
    wave per clip adds its partial sums in run order, then the samples are normalised)."""
    _arg("out", out, torch.float32)
    h, total = _audio_desc(desc, desc_host)
    max_out = int(h[:, 4].max())
    _arg("partials", partials, torch.float64, (h.shape[0], (max_out + AUDIO_RUN - 1) // AUDIO_RUN, 2))
    if out.dim() != 1 or out.numel() < total:
        raise TypeError(f"out must be 1-D with at least {total} samples")
    stats = torch.empty(h.shape[0], 2, device=out.device, dtype=torch.float64)
    _lib.check(_lib.load().msmd_audio_znorm(_p(out), out.numel(), _p(desc), h.shape[0], max_out, _p(partials), _p(stats),
                                            _stream()), "msmd_audio_znorm")
    return out


# ----------------------------------------------------------------------------- head pose from landmarks (csrc/headpose.hip)
HEADPOSE_MAX_WINDOW, HEADPOSE_CHUNK, HEADPOSE_MAX_STATIC = _h("HEADPOSE_MAX_WINDOW", "HEADPOSE_CHUNK", "HEADPOSE_MAX_STATIC")


def _clip_offsets(name, offsets, total, window=0, max_frames=None):
    """The HOST offsets of a ragged batch of clips laid end to end -> a list of ints: ascending from 0 to `total`, every clip
    of max(1, window) .. max_frames frames (None: no cap, and the window rule alone speaks); ValueError otherwise."""
    off = [int(o) for o in offsets]
    if len(off) < 2 or off[0] != 0 or off[-1] != total:
        raise ValueError(f"{name} must run from 0 to {total}, got {off[:1]} .. {off[-1:]}")
    for a, b in zip(off[:-1], off[1:]):
        if max_frames is not None and not 1 <= b - a <= max_frames:
            raise ValueError(f"{name}: a clip must have 1 .. {max_frames} frames, got {b - a}")
        if b - a < max(window, 1):
            raise ValueError(f"a clip of {b - a} frames is shorter than the window of {window}")
    return off


def _savgol_window(window, table=None, allow_zero=False, name="window"):
    """-> int(window): odd and in [3, HEADPOSE_MAX_WINDOW], or 0 (no filter, and then no table) if allow_zero; ValueError
    otherwise.  table = (its name, tensor): the (window * window,) float64 device tensor of utils/head_pose.savgol_table (TypeError)."""
    window = int(window)
    if window == 0 and allow_zero:
        if table is not None and table[1] is not None:
            raise ValueError(f"{table[0]} given with {name} = 0")
    elif window < 3 or window > HEADPOSE_MAX_WINDOW or window % 2 == 0:
        raise ValueError(f"{name} must be {'0 or ' if allow_zero else ''}odd and in [3, {HEADPOSE_MAX_WINDOW}], got {window}")
    elif table is not None:
        _arg(*table, torch.float64, (window * window,))
    return window


def headpose_fit(landmarks, plan_a, plan_b, plan_w, neutral, static_idx, want_aligned=True):
    """-> (R (n, 3, 3), c (n), t (n, 3), aligned (n, P, 3) or None) fp32: msmd_headpose_fit, the per-frame similarity fit of
    the static landmarks onto `neutral` and the fitted transform applied to every landmark.  landmarks (n, P, 3) fp32, the
    clips of a batch end to end; plan_a / plan_b (n) int32 and plan_w (n) fp32: frame f is (1 - w) L[a] + w L[b]
    (utils/head_pose.gap_plan); neutral (P, 3) fp32, read at static_idx (S) int32 in [0, P), 3 <= S <= HEADPOSE_MAX_STATIC.  The index
    arrays live on the device and are not read back here: the kernel clamps them into range."""
    _need_cuda(landmarks, plan_a, plan_b, plan_w, neutral, static_idx)
    d = {}
    _arg("landmarks", landmarks, torch.float32, "n+ P 3", d)
    _arg("plan_a", plan_a, torch.int32, "n", d)
    _arg("plan_b", plan_b, torch.int32, "n", d)
    _arg("plan_w", plan_w, torch.float32, "n", d)
    _arg("neutral", neutral, torch.float32, "P 3", d)
    _arg("static_idx", static_idx, torch.int32)
    n, P, S = d["n"], d["P"], static_idx.numel()
    if static_idx.dim() != 1 or not 3 <= S <= min(HEADPOSE_MAX_STATIC, P):
        raise ValueError(f"static_idx must hold 3 .. min({HEADPOSE_MAX_STATIC}, P) indices, got shape {tuple(static_idx.shape)}")
    dev = landmarks.device
    R = torch.empty(n, 3, 3, device=dev, dtype=torch.float32)
    c = torch.empty(n, device=dev, dtype=torch.float32)
    t = torch.empty(n, 3, device=dev, dtype=torch.float32)
    aligned = torch.empty(n, P, 3, device=dev, dtype=torch.float32) if want_aligned else None
    _lib.check(_lib.load().msmd_headpose_fit(_p(landmarks), _p(plan_a), _p(plan_b), _p(plan_w), _p(neutral), _p(static_idx),
                                             _p(R), _p(c), _p(t), _p(aligned), n, P, S, _stream()), "msmd_headpose_fit")
    return R, c, t, aligned


def headpose_smooth(R, clip_offsets, table, window, want_matrix=False):
    """-> (ypr (n, 3) fp32 yaw / pitch / -roll in degrees, R_modified (n, 3, 3) fp32 or None): msmd_headpose_smooth over
    the clips [clip_offsets[k], clip_offsets[k + 1]) of R (n, 3, 3) fp32.  clip_offsets: the (n_clips + 1) offsets on the
    HOST (checked here: ascending from 0 to n, every clip at least `window` frames; copied to the device as int64);
    table (window * window) float64 on the device (utils/head_pose.savgol_table)."""
    _need_cuda(R, table)
    _arg("R", R, torch.float32, "n+ 3 3")
    window = _savgol_window(window, ("table", table))
    off = _clip_offsets("clip_offsets", clip_offsets, R.shape[0], window)
    off_dev = torch.tensor(off, dtype=torch.int64).to(R.device)
    ypr = torch.empty(R.shape[0], 3, device=R.device, dtype=torch.float32)
    R_mod = torch.empty_like(R) if want_matrix else None
    _lib.check(_lib.load().msmd_headpose_smooth(_p(R), _p(off_dev), len(off) - 1, _p(table), window, _p(ypr), _p(R_mod),
                                                _stream()), "msmd_headpose_smooth")
    return ypr, R_mod


# ----------------------------------------------------------------------------- expression fit (csrc/expression_fit.hip)
EXPFIT_MAX_LANDMARKS, EXPFIT_MAX_EXP, EXPFIT_MAX_ITERATIONS, EXPFIT_FRAMES = _h(
    "EXPFIT_MAX_LANDMARKS", "EXPFIT_MAX_EXP", "EXPFIT_MAX_ITERATIONS", "EXPFIT_FRAMES")


def expression_fit(landmarks, subject, tab, tab0, weights, jaw_dof=1, lambda_exp=1e-6, lambda_jaw=0.0, iterations=12):
    """-> (code (n, NE), jaw (n, 3), rms (n)) fp32 and status (n) int32: msmd_expression_fit, the per-frame Levenberg-Marquardt
    fit of FLAME's expression and jaw pose to landmarks (n, K, 3) fp32 in model space, the clips of a batch end to end.
    tab (K, 6, NE + 9) and tab0 (S, K, 6) float64: the reduced model (utils/expression_fit.reduce_flame); subject (n) int32 picks
    tab0's set per frame -- it lives on the device and is not read back here: the kernel clamps it into [0, S).
    weights (K) float64 >= 0 (checked by utils/expression_fit.fit_expression, which has them on the host).
    jaw_dof 0 / 1 / 3 free jaw components; `iterations` in [0, EXPFIT_MAX_ITERATIONS] of fixed work; the include file states the
    solver and the status bits.  ValueError for a size or option outside the kernel's limits."""
    _need_cuda(landmarks, subject, tab, tab0, weights)
    d = {}
    _arg("landmarks", landmarks, torch.float32, "n+ K+ 3", d)
    _arg("subject", subject, torch.int32, "n", d)
    _arg("tab0", tab0, torch.float64, "S+ K 6", d)
    _arg("tab", tab, torch.float64, "K 6 NC+", d)
    _arg("weights", weights, torch.float64, "K", d)
    n, K, NE = d["n"], d["K"], d["NC"] - 9
    if K > EXPFIT_MAX_LANDMARKS:
        raise ValueError(f"{K} landmarks; the kernel takes up to {EXPFIT_MAX_LANDMARKS}")
    if not 1 <= NE <= EXPFIT_MAX_EXP:
        raise ValueError(f"tab has {NE} expression columns; the kernel takes 1 .. {EXPFIT_MAX_EXP}")
    if jaw_dof not in (0, 1, 3):
        raise ValueError(f"jaw_dof must be 0, 1 or 3, got {jaw_dof!r}")
    iterations = int(iterations)
    if not 0 <= iterations <= EXPFIT_MAX_ITERATIONS:
        raise ValueError(f"iterations must be in [0, {EXPFIT_MAX_ITERATIONS}], got {iterations}")
    lambda_exp, lambda_jaw = float(lambda_exp), float(lambda_jaw)
    if not (0.0 <= lambda_exp < float("inf") and 0.0 <= lambda_jaw < float("inf")):
        raise ValueError(f"lambda_exp and lambda_jaw must be finite and >= 0, got {lambda_exp!r}, {lambda_jaw!r}")
    if n * K * 3 > 0x7fffffff:
        raise ValueError(f"{n} frames of {K} landmarks are more than one call addresses")
    dev = landmarks.device
    code = torch.empty(n, NE, device=dev, dtype=torch.float32)
    jaw = torch.empty(n, 3, device=dev, dtype=torch.float32)
    rms = torch.empty(n, device=dev, dtype=torch.float32)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().msmd_expression_fit(_p(landmarks), _p(subject), _p(tab), _p(tab0), _p(weights), _p(code), _p(jaw),
                                               _p(rms), _p(status), n, K, NE, d["S"], int(jaw_dof), iterations, lambda_exp,
                                               lambda_jaw, _stream()), "msmd_expression_fit")
    return code, jaw, rms, status


# ----------------------------------------------------------------------------- track resampling (csrc/track_resample.hip)
TRACK_MAX_FRAMES, TRACK_MAX_CHANNELS, TRACK_ROWS, TRACK_CH_TILE, TRACK_STAGE = _h(
    "TRACK_MAX_FRAMES", "TRACK_MAX_CHANNELS", "TRACK_ROWS", "TRACK_CH_TILE", "TRACK_STAGE")    # limits and the kernels' tile


def track_resample(x, in_offsets, out_offsets, savgol_table=None, window=0):
    """-> y (out_offsets[-1], C) fp32: msmd_track_resample, scipy.signal.resample along the frames of every clip
    [in_offsets[k], in_offsets[k + 1]) of x (n, C) fp32 to out_offsets[k + 1] - out_offsets[k] frames, one call for the whole
    list.  The offsets are on the HOST (checked here: ascending from 0, 1 .. TRACK_MAX_FRAMES frames a clip).
    window != 0: the track is read through the Savitzky-Golay filter of `savgol_table` (window * window) float64 on the
    device (utils/head_pose.savgol_table), window odd in [3, HEADPOSE_MAX_WINDOW], every clip at least `window` frames."""
    _need_cuda(x, savgol_table)
    _arg("x", x, torch.float32, "n+ C+")
    window = _savgol_window(window, ("savgol_table", savgol_table), allow_zero=True)
    n, C = x.shape
    if C > TRACK_MAX_CHANNELS:
        raise ValueError(f"x has {C} channels; the kernel takes up to {TRACK_MAX_CHANNELS}")
    off_in = _clip_offsets("in_offsets", in_offsets, n, window, TRACK_MAX_FRAMES)
    if len(out_offsets) != len(off_in):
        raise ValueError(f"{len(off_in) - 1} input clips but {len(out_offsets) - 1} output clips")
    off_out = _clip_offsets("out_offsets", out_offsets, int(out_offsets[-1]), 0, TRACK_MAX_FRAMES)
    n_clips = len(off_in) - 1
    lib = _lib.load()
    host_in, host_out = torch.tensor(off_in, dtype=torch.int32), torch.tensor(off_out, dtype=torch.int32)
    ws = torch.empty(lib.msmd_track_resample_ws_bytes(n, n_clips, C), device=x.device, dtype=torch.uint8)
    y = torch.empty(off_out[-1], C, device=x.device, dtype=torch.float32)
    _lib.check(lib.msmd_track_resample(_p(x), _p(host_in), _p(host_out), n_clips, C, _p(savgol_table), window, _p(ws), _p(y),
                                       _stream()), "msmd_track_resample")
    return y


# ----------------------------------------------------------------------------- face crops (csrc/face_crop.hip)
CROP_MAX_SIDE = _h("CROP_MAX_SIDE")     # largest output side of msmd_face_crop
_CROP_DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def face_crop(frames, inverse, table, out_size, dtype=torch.float32, swap_rb=True, want_normalised=True, want_uint8=False):
    """-> (out (F, 3, S_h, S_w) of `dtype` or None, crop (F, S_h, S_w, 3) uint8 or None): msmd_face_crop, the float64 bilinear
    affine warp with a zero border of include/msmd_hip.h, one launch for the batch.  frames (F, H, W, 3 | 4) uint8 on the
    device, laid out as `jpeg_encode` takes them (alpha ignored); inverse (F, 2, 3) float64 on the device, output pixel ->
    source coordinates; table (3, 256) fp32 on the device, out[f, c] = table[c][byte]; out_size = S or (S_h, S_w), each in
    [1, CROP_MAX_SIDE].  swap_rb: output channel c reads source channel 2 - c."""
    F, H, W, sb, sh, sw = _u8_frames(frames)
    d = {"F": F}
    _arg("inverse", inverse, torch.float64, "F 2 3", d)
    _arg("table", table, torch.float32, "3 256")
    S_h, S_w = (int(out_size),) * 2 if isinstance(out_size, int) else (int(s) for s in out_size)
    if not (1 <= S_h <= CROP_MAX_SIDE and 1 <= S_w <= CROP_MAX_SIDE):
        raise ValueError(f"out_size {out_size!r} is outside [1, {CROP_MAX_SIDE}]")
    if dtype not in _CROP_DTYPES:
        raise TypeError(f"dtype must be torch.float32, torch.bfloat16 or torch.float16, got {dtype}")
    if not (want_normalised or want_uint8):
        raise ValueError("face_crop: neither output is asked for")
    out = torch.empty(F, 3, S_h, S_w, device=frames.device, dtype=dtype) if want_normalised else None
    crop = torch.empty(F, S_h, S_w, 3, device=frames.device, dtype=torch.uint8) if want_uint8 else None
    _lib.check(_lib.load().msmd_face_crop(_p(frames), sb, sh, sw, F, H, W, _p(inverse), _p(table), S_h, S_w, int(bool(swap_rb)),
                                          _p(out), _CROP_DTYPES[dtype], _p(crop), _stream()), "msmd_face_crop")
    return out, crop


# ----------------------------------------------------------------------------- frame resizing (csrc/resize.hip)
RESIZE_AUTO, RESIZE_FUSED, RESIZE_TWO_PASS = _h("RESIZE_AUTO", "RESIZE_FUSED", "RESIZE_TWO_PASS")
RESIZE_TILE_H, RESIZE_TILE_W, RESIZE_LDS_BYTES = _h("RESIZE_TILE_H", "RESIZE_TILE_W", "RESIZE_LDS_BYTES")
RESIZE_PRECISION_BITS, RESIZE_CACHE_BYTES = _h("RESIZE_PRECISION_BITS", "RESIZE_CACHE_BYTES")
RESIZE_FORMS = {None: RESIZE_AUTO, "fused": RESIZE_FUSED, "two_pass": RESIZE_TWO_PASS}
_RESIZE_FORM_NAMES = {RESIZE_FUSED: "fused", RESIZE_TWO_PASS: "two_pass"}


def _resize_box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _resize_bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _resize_bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _resize_sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _resize_lanczos(x):
    return _resize_sinc(x) * _resize_sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


RESIZE_FILTERS = {"box": (_resize_box, 0.5), "bilinear": (_resize_bilinear, 1.0), "bicubic": (_resize_bicubic, 2.0),
                  "lanczos": (_resize_lanczos, 3.0)}


@functools.lru_cache(maxsize=256)
def resize_tables(n_in, n_out, filter, in0=None, in1=None):
    """One axis of Pillow's 8-bit `Image.resize`: n_in samples -> n_out over the source interval [in0, in1) (the whole axis by
    default) -> (bounds (n_out, 2) int32 = (first tap, taps), coef (n_out, ksize) int32 in units of 2^-22, zero behind the
    taps).  Python floats in Pillow's order of operations; the arrays are cached and read-only.  Raises
    ValueError for an unknown filter, a size below 1, an interval that is empty or leaves the axis, and a table under which
    the int32 accumulator could overflow."""
    if filter not in RESIZE_FILTERS:
        raise ValueError(f"filter must be one of {sorted(RESIZE_FILTERS)}, got {filter!r}")
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_tables: sizes {n_in} -> {n_out} must be at least 1")
    in0, in1 = float(0 if in0 is None else in0), float(n_in if in1 is None else in1)
    if not 0.0 <= in0 < in1 <= n_in:
        raise ValueError(f"resize_tables: the interval [{in0}, {in1}) is empty or leaves [0, {n_in}]")
    f, support = RESIZE_FILTERS[filter]
    scale = (in1 - in0) / n_out
    fs = max(scale, 1.0)
    sup = support * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    ss = 1.0 / fs
    one = float(1 << RESIZE_PRECISION_BITS)
    bounds = np.zeros((n_out, 2), np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = in0 + (xx + 0.5) * scale
        xmin = max(0, int(center - sup + 0.5))
        xmax = min(n_in, int(center + sup + 0.5)) - xmin
        w = [f((i + xmin - center + 0.5) * ss) for i in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(0.5 + v * one) if v >= 0 else int(-0.5 + v * one) for v in w]
        if sum(abs(v) for v in k) * 255 + (1 << (RESIZE_PRECISION_BITS - 1)) >= 1 << 31:
            raise ValueError(f"resize_tables: {n_in} -> {n_out} ({filter}): output {xx} could overflow the int32 accumulator")
        bounds[xx] = (xmin, xmax)
        coef[xx, :xmax] = k
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def _resize_identity(n):
    """The table of a pass that is skipped: one tap of weight 1 at the output's own position."""
    bounds = np.stack([np.arange(n, dtype=np.int32), np.ones(n, np.int32)], 1)
    return bounds, np.full((n, 1), 1 << RESIZE_PRECISION_BITS, np.int32)


def _resize_axis(n_in, n_out, filter, in0, in1):
    """`resize_tables`, or the identity where the pass is skipped: the axis keeps its size over the whole-axis interval."""
    if n_in == n_out and in0 == 0.0 and in1 == float(n_in):
        if filter not in RESIZE_FILTERS:
            raise ValueError(f"filter must be one of {sorted(RESIZE_FILTERS)}, got {filter!r}")
        return _resize_identity(n_in)
    return resize_tables(n_in, n_out, filter, in0, in1)


def _resize_stack(tables):
    """[(bounds, coef)] of one axis -> (bounds (T, n_out, 2), coef (T, n_out, ksize)), the weights padded with zeros to one ksize."""
    ksize = max(c.shape[1] for _, c in tables)
    coef = np.zeros((len(tables), tables[0][1].shape[0], ksize), np.int32)
    for t, (_, c) in enumerate(tables):
        coef[t, :, :c.shape[1]] = c
    return np.ascontiguousarray(np.stack([b for b, _ in tables])), coef


def resize_rows_span(ybounds, n_in, ksize):
    """The source rows one tile of RESIZE_TILE_H output rows touches, at most, over the tables of ybounds (T, n_out, 2): what
    msmd_resize_u8 takes as rows_span.  The bounds are clamped as the kernel clamps them."""
    b = np.asarray(ybounds).reshape(-1, np.asarray(ybounds).shape[-2], 2).astype(np.int64)
    first = np.clip(b[..., 0], 0, n_in - 1)
    end = first + np.clip(b[..., 1], 0, np.minimum(ksize, n_in - first))
    span = 0
    for y0 in range(0, b.shape[1], RESIZE_TILE_H):
        span = max(span, int((end[:, y0:y0 + RESIZE_TILE_H].max(1) - first[:, y0:y0 + RESIZE_TILE_H].min(1)).max()))
    return span


def resize_fits(C, rows_span):
    """-> bool: msmd_resize_fits, whether the fused form can run: the tile's rows_span intermediate rows of RESIZE_TILE_W * C + 4
    bytes fit RESIZE_LDS_BYTES."""
    return bool(_lib.load().msmd_resize_fits(int(C), int(rows_span)))


def resize_route(C, rows_span, N, Hs, Hd, Wd, kx):
    """-> "fused" | "two_pass": msmd_resize_route, the rule msmd_resize_u8 follows when no form is forced.  Fused where it fits,
    except where the tiles' overlap repeats more than one horizontal multiply-add per intermediate byte
    ((rows_span * ceil(Hd / RESIZE_TILE_H) - Hs) * kx > Hs) while the two-pass intermediate of N * Hs * Wd * C bytes stays within
    RESIZE_CACHE_BYTES: there the two launches were measured faster."""
    return _RESIZE_FORM_NAMES[_lib.load().msmd_resize_route(int(C), int(rows_span), int(N), int(Hs), int(Hd), int(Wd), int(kx))]


def _resize_source(frames):
    """Checks of (N, H, W, 1 | 3 | 4) uint8 device frames, laid out as `_u8_frames` accepts them (one byte per pixel for one
    channel) -> (N, H, W, C, frame stride, row stride, pixel stride).  N = 0 is allowed."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise TypeError("frames must be a uint8 tensor")
    if not frames.is_cuda:
        raise TypeError("frames must be on the MI355X (cuda) device; there is no CPU resampler")
    if frames.dim() != 4 or frames.shape[3] not in (1, 3, 4):
        raise TypeError(f"frames must have shape (N, H, W, 1 | 3 | 4), got {tuple(frames.shape)}")
    N, H, W, C = frames.shape
    if not (1 <= H <= JPEG_MAX_SIDE and 1 <= W <= JPEG_MAX_SIDE):
        raise ValueError(f"frames of shape {tuple(frames.shape)}: 1 <= H, W <= {JPEG_MAX_SIDE} is required")
    sb, sh, sw, sc = frames.stride()
    if C == 1:
        sc = 1                                          # the stride of a dimension of size 1 is arbitrary
    if N == 0:
        sb, sh, sw = H * W * C, W * C, C                 # an empty batch has no addresses: whatever strides it carries are not used
    elif sc != 1 or not (sw == C or (C == 3 and sw == 4)) or sh < (W - 1) * sw + C or (N > 1 and sb < (H - 1) * sh + (W - 1) * sw + C):
        raise TypeError(f"frames with strides {frames.stride()}: channels must be adjacent bytes, pixels {C} bytes apart (3 or 4 "
                        "for 3 channels), rows and frames must not overlap (call .contiguous())")
    return N, H, W, C, sb, sh, sw


def resize_u8(frames, xbounds, xcoef, ybounds, ycoef, table_of_frame, size, out=None, form=None, rows_span=None):
    """msmd_resize_u8 on tables that are already on the device: frames (N, Hs, Ws, C) -> (N, Hd, Wd, C), size = (Hd, Wd).
    xbounds (T, Wd, 2), xcoef (T, Wd, kx), ybounds (T, Hd, 2), ycoef (T, Hd, ky), table_of_frame (N), all int32.  rows_span as
    `resize_rows_span` gives it for ybounds (required for the fused form; the route without it is two_pass).  form: None for
    `resize_route`'s choice.  The two-pass
    workspace is allocated here."""
    N, Hs, Ws, C, sb, sh, sw = _resize_source(frames)
    Hd, Wd = int(size[0]), int(size[1])
    if form not in RESIZE_FORMS:
        raise ValueError(f"form must be None, 'fused' or 'two_pass', got {form!r}")
    d = {"N": N, "Hd": Hd, "Wd": Wd}
    _arg("xbounds", xbounds, torch.int32, "T+ Wd 2", d)
    _arg("xcoef", xcoef, torch.int32, "T Wd kx+", d)
    _arg("ybounds", ybounds, torch.int32, "T Hd 2", d)
    _arg("ycoef", ycoef, torch.int32, "T Hd ky+", d)
    _arg("table_of_frame", table_of_frame, torch.int32, "N", d)
    _arg("out", out, torch.uint8, (N, Hd, Wd, C), optional=True)
    rows_span = 0 if rows_span is None else int(rows_span)
    lib = _lib.load()
    route = lib.msmd_resize_route(C, rows_span, N, Hs, Hd, Wd, d["kx"])
    if form == "fused" and not lib.msmd_resize_fits(C, rows_span):
        raise ValueError(f"resize: the fused form does not fit: {rows_span} intermediate rows of {RESIZE_TILE_W * C + 4} bytes "
                         f"against {RESIZE_LDS_BYTES} bytes of LDS")
    code = RESIZE_FORMS[form] or route
    dst = out if out is not None else torch.empty(N, Hd, Wd, C, device=frames.device, dtype=torch.uint8)
    ws = torch.empty(N * Hs * Wd * C, device=frames.device, dtype=torch.uint8) if code == RESIZE_TWO_PASS else None
    _lib.check(lib.msmd_resize_u8(_p(frames), sb, sh, sw, N, Hs, Ws, C, _p(xbounds), _p(xcoef), d["kx"], d["T"], _p(ybounds),
                                  _p(ycoef), d["ky"], d["T"], _p(table_of_frame), _p(dst), Hd, Wd, _p(ws), rows_span, code,
                                  _stream()), "msmd_resize_u8")
    return dst


def _resize_plan(Hs, Ws, Hd, Wd, filter, boxes, device):
    """The tables of the distinct boxes of a call, on the device of that name -> (xbounds, xcoef, ybounds, ycoef, rows_span).
    boxes: a tuple of (x0, y0, x1, y1), already rounded to float32.  Nothing on the device is kept: a set of boxes per frame
    is unlikely to come again (the 1-D host tables behind it are cached by `resize_tables`)."""
    xs = [_resize_axis(Ws, Wd, filter, b[0], b[2]) for b in boxes]
    ys = [_resize_axis(Hs, Hd, filter, b[1], b[3]) for b in boxes]
    (xb, xc), (yb, yc) = _resize_stack(xs), _resize_stack(ys)
    up = lambda a: torch.from_numpy(a).to(device)
    return up(xb), up(xc), up(yb), up(yc), resize_rows_span(yb, Hs, yc.shape[2])


@functools.lru_cache(maxsize=32)
def _resize_plan_shared(Hs, Ws, Hd, Wd, filter, box, device):
    """`_resize_plan` for one box shared by every frame, uploaded once for the calls of a video (a few hundred KB at most)."""
    return _resize_plan(Hs, Ws, Hd, Wd, filter, (box,), device)


def resize_frames(frames, size, filter="bilinear", box=None, out=None, form=None):
    """frames (N, Hs, Ws, 1 | 3 | 4) uint8 on the device -> (N, Hd, Wd, C) uint8, size = (Wd, Hd) as Pillow orders it: the bytes
    of `PIL.Image.resize(size, filter, box=, reducing_gap=None)` on every frame (four channels are four plain channels, Pillow's
    CMYK).  filter: "box", "bilinear", "bicubic" or "lanczos".  box: None, one (x0, y0, x1, y1) for all frames
    or (N, 4) with one per frame, in source pixels, rounded to float32, 0 <= x0 < x1 <= Ws and the same in y; frames with equal
    boxes share a table.  out: a contiguous (N, Hd, Wd, C) uint8 device tensor to write.  form: None (the route's choice,
    `resize_route`), "fused" or "two_pass"; a forced fused form that does not fit raises ValueError.  A row stride above the row,
    the renderer's RGB view of RGBA and any byte alignment are taken as they are."""
    N, Hs, Ws, C, _, _, _ = _resize_source(frames)
    if filter not in RESIZE_FILTERS:
        raise ValueError(f"filter must be one of {sorted(RESIZE_FILTERS)}, got {filter!r}")
    try:
        Wd, Hd = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (width, height), got {size!r}") from None
    if not (1 <= Hd <= JPEG_MAX_SIDE and 1 <= Wd <= JPEG_MAX_SIDE):
        raise ValueError(f"size {size!r}: 1 <= width, height <= {JPEG_MAX_SIDE} is required")
    if box is None:
        boxes = np.array([[0, 0, Ws, Hs]], np.float64)
    else:
        boxes = np.asarray(box.cpu() if torch.is_tensor(box) else box, dtype=np.float64)
        if boxes.shape != (4,) and boxes.shape != (N, 4):
            raise ValueError(f"box must be None, (x0, y0, x1, y1) or ({N}, 4), got shape {boxes.shape}")
        boxes = boxes.reshape(-1, 4).astype(np.float32).astype(np.float64)      # Pillow's C code stores a box as float32
        if not (np.isfinite(boxes).all() and (0 <= boxes[:, :2]).all() and (boxes[:, :2] < boxes[:, 2:]).all()
                and (boxes[:, 2] <= Ws).all() and (boxes[:, 3] <= Hs).all()):
            raise ValueError(f"box {box!r}: 0 <= x0 < x1 <= {Ws} and 0 <= y0 < y1 <= {Hs} are required")
    keys = [tuple(b) for b in boxes.tolist()] or [(0.0, 0.0, float(Ws), float(Hs))]     # an empty batch with an empty (0, 4) box
    distinct = tuple(dict.fromkeys(keys))
    if len(distinct) == 1:
        xb, xc, yb, yc, span = _resize_plan_shared(Hs, Ws, Hd, Wd, filter, distinct[0], str(frames.device))
    else:
        xb, xc, yb, yc, span = _resize_plan(Hs, Ws, Hd, Wd, filter, distinct, str(frames.device))
    if len(keys) == 1:
        tof = torch.zeros(N, device=frames.device, dtype=torch.int32)
    else:
        at = {k: t for t, k in enumerate(distinct)}
        tof = torch.tensor([at[k] for k in keys], dtype=torch.int32).to(frames.device)
    return resize_u8(frames, xb, xc, yb, yc, tof, (Hd, Wd), out=out, form=form, rows_span=span)


# ----------------------------------------------------------------------------- overlays (csrc/overlay.hip)
OVERLAY_NONE, OVERLAY_DISC, OVERLAY_CAPSULE, OVERLAY_BOX, OVERLAY_GLYPH = _h("OVERLAY_NONE", "OVERLAY_DISC", "OVERLAY_CAPSULE",
                                                                             "OVERLAY_BOX", "OVERLAY_GLYPH")
OVERLAY_TILE_W, OVERLAY_TILE_H, OVERLAY_CHUNK = _h("OVERLAY_TILE_W", "OVERLAY_TILE_H", "OVERLAY_CHUNK")
OVERLAY_MAX_COORD, OVERLAY_MAX_RADIUS = _h("OVERLAY_MAX_COORD", "OVERLAY_MAX_RADIUS")
OVERLAY_SAMPLES = (1, 16)


def draw_overlay(frames, prims, prim_offsets, font=None, samples=16, out=None):
    """msmd_draw_overlay: the records of prims (P, 8) int32 = [kind, x0, y0, x1, y1, r, aux, colour] drawn onto frames (N, H, W,
    1 | 3 | 4) uint8 on the device, frame f taking the records [prim_offsets[f], prim_offsets[f + 1]) in that order (prim_offsets
    (N + 1) int32); coordinates in 1/16 pixel, the rule in include/msmd_hip.h.  font (n_glyphs, 8) uint8 serves the glyph records
    (None: no glyph draws).  samples: 1 or 16 sample points per pixel.  frames may be a strided view (a panel of a wider frame, a
    4-byte pixel stride under 3 channels, any byte alignment) whose channels are adjacent bytes.  out=None draws in place and
    returns frames; otherwise out is a uint8 device tensor of the same shape and strides that does not overlap frames, receives
    every pixel and is returned."""
    _need_cuda(frames, prims, prim_offsets, font, out)
    N, H, W, C, sb, sh, sw = _resize_source(frames)
    if samples not in OVERLAY_SAMPLES:
        raise ValueError(f"samples must be one of {OVERLAY_SAMPLES}, got {samples!r}")
    d = {}
    _arg("prims", prims, torch.int32, "P 8", d)
    _arg("prim_offsets", prim_offsets, torch.int32, (N + 1,))
    _arg("font", font, torch.uint8, "G 8", d, optional=True)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or not out.is_cuda or out.shape != frames.shape:
            raise TypeError(f"out must be a uint8 CUDA tensor of shape {tuple(frames.shape)}")
        if _resize_source(out)[4 if N > 1 else 5:] != ((sb, sh, sw) if N > 1 else (sh, sw)):      # one frame has no frame stride
            raise TypeError(f"out with strides {out.stride()} must share the strides of frames, {frames.stride()}")
    dst = frames if out is None else out
    _lib.check(_lib.load().msmd_draw_overlay(_p(frames), _p(dst), sb, sh, sw, N, H, W, C, _p(prims), d["P"], _p(prim_offsets), _p(font),
                                             d.get("G", 0), int(samples), _stream()), "msmd_draw_overlay")
    return dst


# ----------------------------------------------------------------------------- style losses (csrc/style_loss.hip)
STYLE_ROWS, STYLE_KTILE, STYLE_FCHUNK = _h("STYLE_ROWS", "STYLE_KTILE", "STYLE_FCHUNK")    # the kernels' tile (include/msmd_hip.h)
NT_XENT_CHUNK = _h("NT_XENT_CHUNK")  # rows j per step of the NT-Xent backward's coefficient table


def _style_shapes(X, S, lambda_softmin):
    """(B, T, K, F) of X (B, T, F) against S (B, K, F); ValueError before anything touches the device or the library."""
    if X.dim() != 3 or S.dim() != 3:
        raise ValueError(f"style adherence takes X (B, T, F) and S (B, K, F), got {tuple(X.shape)} and {tuple(S.shape)}")
    (B, T, F), (Bs, K, Fs) = X.shape, S.shape
    if B != Bs or F != Fs:
        raise ValueError(f"style adherence: X {tuple(X.shape)} and S {tuple(S.shape)} differ in batch or feature size")
    if min(B, T, K, F) < 1:
        raise ValueError(f"style adherence: empty operand, X {tuple(X.shape)}, S {tuple(S.shape)} (K = 0 has no minimum)")
    lam = float(lambda_softmin)
    if not 0.0 <= lam < float("inf"):
        raise ValueError(f"style adherence: lambda_softmin = {lambda_softmin!r} must be finite and >= 0")
    return B, T, K, F, lam


def style_adherence_forward(X, S, lambda_softmin=10.0, soft=True):
    """-> (L (B, T) fp32, stat (B, T)): msmd_style_adherence_forward.  X (B, T, F), S (B, K, F) contiguous fp32.  soft: L =
    sum_k softmax_k(-lambda d) d over d[t, k] = mean_f (X[t] - S[k])^2, stat (B, T, 2) fp32 = (min_k d, log sum_k exp(-lambda (d -
    min))); hard: L = min_k d, stat (B, T) int32 = the lowest index that attains it.  stat is what style_adherence_backward
    reads."""
    B, T, K, F, lam = _style_shapes(X, S, lambda_softmin)
    _need_cuda(X, S)
    _arg("X", X, torch.float32)
    _arg("S", S, torch.float32)
    L = torch.empty(B, T, device=X.device, dtype=torch.float32)
    stat = torch.empty((B, T, 2) if soft else (B, T), device=X.device, dtype=torch.float32 if soft else torch.int32)
    _lib.check(_lib.load().msmd_style_adherence_forward(_p(X), _p(S), _p(L), _p(stat), B, T, K, F, lam, int(bool(soft)),
                                                        _stream()), "msmd_style_adherence_forward")
    return L, stat


def style_adherence_backward(X, S, L, stat, g, lambda_softmin=10.0, soft=True, need_dS=True, g_scale=1.0, need_dX=True):
    """-> (dX (B, T, F) or None, dS (B, K, F) or None): msmd_style_adherence_backward from the forward's L and stat.  g: the
    rows' gradient, (B, T) fp32, or one element (the upstream of a mean; pass g_scale = 1 / (B T)) that every row reads.  A
    gradient that is not needed is not computed (its launch is skipped)."""
    if not (need_dX or need_dS):
        return None, None
    B, T, K, F, lam = _style_shapes(X, S, lambda_softmin)
    _need_cuda(X, S, L, stat, g)
    _arg("X", X, torch.float32)
    _arg("S", S, torch.float32)
    _arg("L", L, torch.float32, (B, T))
    _arg("stat", stat, torch.float32 if soft else torch.int32, (B, T, 2) if soft else (B, T))
    _arg("g", g, torch.float32)
    if g.numel() != 1 and tuple(g.shape) != (B, T):
        raise TypeError(f"g must have one element or shape {(B, T)}, got {tuple(g.shape)}")
    dX = torch.empty_like(X) if need_dX else None
    dS = torch.empty_like(S) if need_dS else None
    _lib.check(_lib.load().msmd_style_adherence_backward(_p(X), _p(S), _p(L), _p(stat), _p(g), 0 if g.numel() == 1 else 1,
                                                         float(g_scale), _p(dX), _p(dS), B, T, K, F, lam, int(bool(soft)),
                                                         _stream()), "msmd_style_adherence_backward")
    return dX, dS


def ordered_mean(x):
    """0-dim fp32 mean of a contiguous fp32 tensor, summed in an order that depends on its size alone: msmd_ordered_mean."""
    _need_cuda(x)
    _arg("x", x, torch.float32)
    if x.numel() < 1:
        raise ValueError("ordered_mean of an empty tensor")
    out = torch.empty((), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().msmd_ordered_mean(_p(x), x.numel(), _p(out), _stream()), "msmd_ordered_mean")
    return out


def _nt_xent_shapes(a, b, temperature):
    if a.dim() != 2 or b.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"nt_xent takes two (batch, feature) tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"nt_xent: empty features {tuple(a.shape)}")
    tau = float(temperature)
    if not 0.0 < tau < float("inf"):
        raise ValueError(f"nt_xent: temperature = {temperature!r} must be finite and > 0")
    return a.shape[0], a.shape[1], tau


def nt_xent_forward(a, b, temperature):
    """-> (loss 0-dim fp32, row_loss (2 B), (fhat (2 B, D), norm (2 B), lse (2 B, 2))): msmd_nt_xent_forward and the ordered mean of
    its row losses.  a, b (B, D) contiguous fp32; the last tuple is what nt_xent_backward reads."""
    B, D, tau = _nt_xent_shapes(a, b, temperature)
    _need_cuda(a, b)
    _arg("feature_a", a, torch.float32)
    _arg("feature_b", b, torch.float32)
    fhat = torch.empty(2 * B, D, device=a.device, dtype=torch.float32)
    norm, row_loss = (torch.empty(2 * B, device=a.device, dtype=torch.float32) for _ in range(2))
    lse = torch.empty(2 * B, 2, device=a.device, dtype=torch.float32)
    _lib.check(_lib.load().msmd_nt_xent_forward(_p(a), _p(b), _p(fhat), _p(norm), _p(row_loss), _p(lse), B, D, tau, _stream()),
               "msmd_nt_xent_forward")
    return ordered_mean(row_loss), row_loss, (fhat, norm, lse)


def nt_xent_backward(saved, upstream, temperature):
    """-> grad (2 B, D) fp32, rows [0, B) for feature_a and [B, 2 B) for feature_b: msmd_nt_xent_backward.  saved: the forward's
    (fhat, norm, lse); upstream: the loss's gradient, one fp32 element on the device."""
    fhat, norm, lse = saved
    _need_cuda(fhat, norm, lse, upstream)
    _arg("fhat", fhat, torch.float32, "N D")
    N, D = fhat.shape
    _arg("norm", norm, torch.float32, (N,))
    _arg("lse", lse, torch.float32, (N, 2))
    _arg("upstream", upstream, torch.float32)
    tau = float(temperature)
    if upstream.numel() != 1 or N % 2 or not 0.0 < tau < float("inf"):
        raise ValueError("nt_xent_backward: upstream has one element, fhat an even number of rows, temperature > 0")
    grad = torch.empty_like(fhat)
    _lib.check(_lib.load().msmd_nt_xent_backward(_p(fhat), _p(norm), _p(lse), _p(upstream), _p(grad), N // 2, D, tau, _stream()),
               "msmd_nt_xent_backward")
    return grad


# ----------------------------------------------------------------------------- vertex-space metrics (csrc/vertex_metrics.hip)
def _vertex_pair(pred, gt, d):
    """pred and gt (n, V, 3) contiguous on the device, one dtype, fp32 or fp16 -> the MSMD_* code of that dtype."""
    _need_cuda(pred, gt)
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dtype != gt.dtype:
        raise TypeError(f"pred and gt must be tensors of one dtype, got {getattr(pred, 'dtype', type(pred))} and {getattr(gt, 'dtype', type(gt))}")
    if pred.dtype not in (torch.float32, torch.float16):
        raise TypeError(f"pred and gt must be torch.float32 or torch.float16, got {pred.dtype}")
    _arg("pred", pred, pred.dtype, "n V+ 3", d)
    _arg("gt", gt, pred.dtype, "n V 3", d)
    return _dt(pred)


def vertex_frame_errors(pred, gt, region):
    """-> (n, 4) float64: msmd_vertex_frame_errors.  Row f = (max over the lip vertices of d2, sum of sqrt(d2), max of sqrt(d2), sum of
    d2) over the vertices of frame f, d2 the squared distance pred - gt in float64.  pred, gt (n, V, 3) contiguous, both fp32 or
    both fp16; region (V) uint8 on the device, bit 0 = lip vertex (utils/metrics.regions).  n = 0 gives an empty table."""
    d = {}
    dt = _vertex_pair(pred, gt, d)
    _need_cuda(region)
    _arg("region", region, torch.uint8, "V", d)
    n, V = d["n"], d["V"]
    out = torch.empty(n, 4, device=pred.device, dtype=torch.float64)
    _lib.check(_lib.load().msmd_vertex_frame_errors(_p(pred), _p(gt), _p(region), _p(out), n, V, dt, _stream()),
               "msmd_vertex_frame_errors")
    return out


def vertex_motion_moments_(state, pred, gt, frame0, clip_offsets_dev, upper_idx, template):
    """msmd_vertex_motion_moments, in place on state (n_clips, U, 2, 3) float64 = [pred | gt][count, mean, M2] of m = |v - template|^2
    over each clip's frames (zero it before the first chunk).  pred, gt (n_chunk, V, 3): the frames [frame0, frame0 + n_chunk) of
    the sequence; clip_offsets_dev (n_clips + 1) int64 on the device, over the whole sequence (its values are not read back
    here: the kernel clamps the frame range into the chunk); upper_idx (U) int32 ascending (clamped into [0, V) by the kernel);
    template (V, 3) or (n_clips, V, 3) fp32.  Returns state."""
    d = {}
    dt = _vertex_pair(pred, gt, d)
    _need_cuda(state, clip_offsets_dev, upper_idx, template)
    _arg("clip_offsets_dev", clip_offsets_dev, torch.int64, "C1+")
    d["C"] = clip_offsets_dev.numel() - 1
    if d["C"] < 1:
        raise TypeError("clip_offsets_dev must hold at least two offsets")
    _arg("upper_idx", upper_idx, torch.int32, "U+", d)
    _arg("state", state, torch.float64, "C U 2 3", d)
    if torch.is_tensor(template) and template.dim() == 2:
        _arg("template", template, torch.float32, "V 3", d)
    else:
        _arg("template", template, torch.float32, "C V 3", d)
    frame0 = int(frame0)
    if frame0 < 0:
        raise ValueError(f"frame0 = {frame0} is negative")
    _lib.check(_lib.load().msmd_vertex_motion_moments(_p(pred), _p(gt), frame0, d["n"], _p(clip_offsets_dev), d["C"], _p(upper_idx),
                                                      d["U"], _p(template), int(template.dim() == 3), _p(state), d["V"], dt,
                                                      _stream()), "msmd_vertex_motion_moments")
    return state


# the error field and its colours
def _color_table(lut, vmax, nan_color):
    """lut (256, 4) uint8 contiguous on the device, vmax finite and > 0, nan_color (R, G, B[, A]) bytes -> (vmax, nan_color word)."""
    _need_cuda(lut)
    _arg("lut", lut, torch.uint8, "256 4")
    vmax = float(vmax)
    if not 0.0 < vmax < float("inf"):
        raise ValueError(f"vmax = {vmax} must be finite and greater than 0")
    c = tuple(int(x) for x in nan_color)
    if len(c) not in (3, 4) or any(not 0 <= x <= 255 for x in c):
        raise ValueError(f"nan_color must be 3 or 4 bytes, got {nan_color!r}")
    r, g, b, a = c if len(c) == 4 else c + (255,)
    return vmax, r | g << 8 | b << 16 | a << 24


def vertex_error_colors(pred, gt, vmax, lut, nan_color=(255, 0, 255)):
    """-> (n, V, 4) uint8: msmd_vertex_error_colors.  The distance |pred - gt| of every vertex, in float64, through the colour table:
    t = d / vmax, row 255 at t >= 1 (+inf too), else row floor(t * 255 + 0.5); a NaN distance gives nan_color.  pred, gt (n, V, 3)
    contiguous, both fp32 or both fp16; lut (256, 4) uint8 on the device (utils/metrics.colormap_table); vmax finite and > 0."""
    d = {}
    dt = _vertex_pair(pred, gt, d)
    vmax, word = _color_table(lut, vmax, nan_color)
    n, V = d["n"], d["V"]
    out = torch.empty(n, V, 4, device=pred.device, dtype=torch.uint8)
    _lib.check(_lib.load().msmd_vertex_error_colors(_p(pred), _p(gt), _p(lut), _p(out), n, V, dt, vmax, word, _stream()),
               "msmd_vertex_error_colors")
    return out


def colormap(x, vmax, lut, nan_color=(255, 0, 255)):
    """-> x.shape + (4,) uint8: msmd_colormap_f64, vertex_error_colors' rule applied to any contiguous float64 device tensor."""
    _need_cuda(x)
    _arg("x", x, torch.float64)
    vmax, word = _color_table(lut, vmax, nan_color)
    out = torch.empty(tuple(x.shape) + (4,), device=x.device, dtype=torch.uint8)
    _lib.check(_lib.load().msmd_colormap_f64(_p(x), _p(lut), _p(out), x.numel(), vmax, word, _stream()), "msmd_colormap_f64")
    return out


def vertex_error_sums_(state, pred, gt, frame0, clip_offsets_dev):
    """msmd_vertex_error_sums, in place on state (n_clips, V) float64 = the sum over each clip's frames of the per-vertex distance
    (zero it before the first chunk).  pred, gt, frame0 and clip_offsets_dev as vertex_motion_moments_ takes them.  Returns state."""
    d = {}
    dt = _vertex_pair(pred, gt, d)
    _need_cuda(state, clip_offsets_dev)
    _arg("clip_offsets_dev", clip_offsets_dev, torch.int64, "C1+")
    d["C"] = clip_offsets_dev.numel() - 1
    if d["C"] < 1:
        raise TypeError("clip_offsets_dev must hold at least two offsets")
    _arg("state", state, torch.float64, "C V", d)
    frame0 = int(frame0)
    if frame0 < 0:
        raise ValueError(f"frame0 = {frame0} is negative")
    _lib.check(_lib.load().msmd_vertex_error_sums(_p(pred), _p(gt), frame0, d["n"], _p(clip_offsets_dev), d["C"], _p(state), d["V"], dt,
                                                  _stream()), "msmd_vertex_error_sums")
    return state


# ----------------------------------------------------------------------------- retargeting (csrc/retarget.hip)
RETARGET_MAX_SHAPES, RETARGET_MAX_VERTICES, RETARGET_ITERATIONS, RETARGET_MAX_ITERATIONS = _h(
    "RETARGET_MAX_SHAPES", "RETARGET_MAX_VERTICES", "RETARGET_ITERATIONS", "RETARGET_MAX_ITERATIONS")
RETARGET_FRAME_TILE, RETARGET_VERTEX_TILE, RETARGET_SPLIT_VERTICES, RETARGET_SOLVE_FRAMES, RETARGET_APPLY_FRAMES = _h(
    "RETARGET_FRAME_TILE", "RETARGET_VERTEX_TILE", "RETARGET_SPLIT_VERTICES", "RETARGET_SOLVE_FRAMES", "RETARGET_APPLY_FRAMES")
RETARGET_CONVERGED, RETARGET_CAP_REACHED, RETARGET_BAD_INPUT, RETARGET_NOT_POSITIVE = _h(
    "RETARGET_CONVERGED", "RETARGET_CAP_REACHED", "RETARGET_BAD_INPUT", "RETARGET_NOT_POSITIVE")


def _retarget_sizes(K, V):
    if not 1 <= K <= RETARGET_MAX_SHAPES:
        raise ValueError(f"{K} blendshapes; the kernels take 1 .. {RETARGET_MAX_SHAPES}")
    if not 1 <= V <= RETARGET_MAX_VERTICES:
        raise ValueError(f"{V} vertices; the kernels take 1 .. {RETARGET_MAX_VERTICES}")


def _host_f64(name, v, K):
    """An optional per-shape host array -> contiguous float64 numpy (K) or None."""
    if v is None:
        return None
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
    if a.shape != (K,):
        raise ValueError(f"{name} must hold {K} values, got shape {a.shape}")
    return a


def retarget_gram(A, ridge=None):
    """-> (G, H) (K, K) float64: msmd_retarget_gram, G = A A^T over the 3 V coordinates of A (K, V, 3) fp32 in float64 and a fixed
    order, H = G + diag(ridge).  ridge: K values >= 0 on the HOST, or None."""
    _need_cuda(A)
    d = {}
    _arg("A", A, torch.float32, "K+ V+ 3", d)
    K, V = d["K"], d["V"]
    _retarget_sizes(K, V)
    ridge = _host_f64("ridge", ridge, K)
    if ridge is not None and not (ridge >= 0.0).all():
        raise ValueError("ridge must be >= 0")
    G = torch.empty(K, K, device=A.device, dtype=torch.float64)
    H = torch.empty(K, K, device=A.device, dtype=torch.float64)
    _lib.check(_lib.load().msmd_retarget_gram(_p(A), None if ridge is None else ridge.ctypes.data, _p(G), _p(H), K, V, _stream()),
               "msmd_retarget_gram")
    return G, H


def retarget_rhs(x, neutral, A, vertex_weight=None):
    """-> b (N, K) fp32: msmd_retarget_rhs, b[n, k] = sum A[k, v, c] * fl32(x[n, v, c] - neutral[v, c]) in fp32 on the exact-fp32
    MFMA.  x (N, V, 3), neutral (V, 3), A (K, V, 3) fp32; vertex_weight (V) fp32 or None: a vertex whose weight is 0 is never read.
    A frame's bits do not depend on N or on where the frame sits.  N = 0 gives an empty table."""
    _need_cuda(x, neutral, A, vertex_weight)
    d = {}
    _arg("A", A, torch.float32, "K+ V+ 3", d)
    _arg("x", x, torch.float32, "N V 3", d)
    _arg("neutral", neutral, torch.float32, "V 3", d)
    _arg("vertex_weight", vertex_weight, torch.float32, "V", d, optional=True)
    N, K, V = d["N"], d["K"], d["V"]
    _retarget_sizes(K, V)
    lib = _lib.load()
    b = torch.empty(N, K, device=x.device, dtype=torch.float32)
    partial = torch.empty(lib.msmd_retarget_splits(V), N, K, device=x.device, dtype=torch.float32)
    _lib.check(lib.msmd_retarget_rhs(_p(x), _p(neutral), _p(A), _p(vertex_weight), _p(partial), _p(b), N, V, K, _stream()),
               "msmd_retarget_rhs")
    return b


def retarget_solve(H, b, lo=None, hi=None, max_iterations=RETARGET_ITERATIONS):
    """-> (w (N, K) fp32, status (N) int32, iterations (N) int32): msmd_retarget_solve, per frame the minimiser of
    1/2 w^T H w - b^T w in the box lo <= w <= hi by block principal pivoting in float64 (the include file states the rule).
    H (K, K) float64 positive definite, b (N, K) fp32 on the device; lo, hi K values on the HOST (None: 0 and 1).
    status: RETARGET_CONVERGED / _CAP_REACHED / _BAD_INPUT / _NOT_POSITIVE."""
    _need_cuda(H, b)
    d = {}
    _arg("H", H, torch.float64, "K+ K", d)
    _arg("b", b, torch.float32, "N K", d)
    N, K = d["N"], d["K"]
    _retarget_sizes(K, 1)
    lo, hi = _host_f64("lo", lo, K), _host_f64("hi", hi, K)
    lo_v, hi_v = np.zeros(K) if lo is None else lo, np.ones(K) if hi is None else hi
    if not (np.isfinite(lo_v).all() and np.isfinite(hi_v).all() and (lo_v < hi_v).all()):
        raise ValueError("the bounds must be finite with lo < hi")
    max_iterations = int(max_iterations)
    if not 1 <= max_iterations <= RETARGET_MAX_ITERATIONS:
        raise ValueError(f"max_iterations must be in [1, {RETARGET_MAX_ITERATIONS}], got {max_iterations}")
    w = torch.empty(N, K, device=b.device, dtype=torch.float32)
    status = torch.empty(N, device=b.device, dtype=torch.int32)
    its = torch.empty(N, device=b.device, dtype=torch.int32)
    _lib.check(_lib.load().msmd_retarget_solve(_p(H), _p(b), None if lo is None else lo.ctypes.data,
                                               None if hi is None else hi.ctypes.data, _p(w), _p(status), _p(its), N, K,
                                               max_iterations, _stream()), "msmd_retarget_solve")
    return w, status, its


def blendshape_apply(w, neutral, deltas):
    """-> (N, V, 3) fp32: msmd_blendshape_apply, neutral + sum_k w[n, k] * deltas[k], an fp32 fmaf chain in ascending k.
    w (N, K), neutral (V, 3), deltas (K, V, 3) fp32."""
    _need_cuda(w, neutral, deltas)
    d = {}
    _arg("deltas", deltas, torch.float32, "K+ V+ 3", d)
    _arg("w", w, torch.float32, "N K", d)
    _arg("neutral", neutral, torch.float32, "V 3", d)
    N, K, V = d["N"], d["K"], d["V"]
    _retarget_sizes(K, V)
    if N > 65535 * RETARGET_APPLY_FRAMES:
        raise ValueError(f"{N} frames are more than one call takes ({65535 * RETARGET_APPLY_FRAMES}); cut the sequence")
    out = torch.empty(N, V, 3, device=w.device, dtype=torch.float32)
    _lib.check(_lib.load().msmd_blendshape_apply(_p(w), _p(neutral), _p(deltas), _p(out), N, V, K, _stream()),
               "msmd_blendshape_apply")
    return out
