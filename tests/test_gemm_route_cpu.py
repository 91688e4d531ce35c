"""msmd_gemm_route / msmd_gemm_ln_route: which kernel the library picks for a call, as a table.

The expected values were recorded from the routing code as it was BEFORE the three copies of the rule were merged: that
version of csrc/gemm.hip, with an early return of the chosen variant in front of each dispatch call (0 where it fell through
to gemm_kernel, -1 where it returned 1), was built host-only and fed the rows below.  They are not outputs of the code under
test.  Two rows differ from that recording on purpose: hint 62 named the gemm4_kernel family, which is gone, and is now an
unknown hint like 37 (recorded: 62); and bf16 operands with an fp16 output, a pair the library has no kernel for, are
rejected whatever the hint, like fp16 -> bf16 always was (recorded for hint 17: 17, the bf16 -> fp32 kernel launched on the
fp16 buffer; without a hint that shape was rejected before too).

The queries are pure host arithmetic: pointers are made-up integers that are never dereferenced (some deliberately
misaligned), and no GPU is needed.

Every `return false` of gemm8_takes / gemm8s_takes is hit by a row that the 256 x 256 kernel would otherwise take, except
two that no call can reach: gemm8_takes' `epi == 2 && (R || !bias || !w_colsum)` (msmd_gemm_ln rejects those operand
combinations first) and gemm8s_takes' ldc / ldr line (msmd_gemm has rejected them, or cleared vec_ok, before)."""
from msmd_amd import _lib

F32, BF16, F16, F16X2 = 0, 1, 2, 3
NONE, GELU, ELU = 0, 1, 2
NO_256, W_BELOW_32 = 1 << 20, 1 << 21
A, W, C, R, BIAS, Z, RNG = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
STATS, COLSUM, GAMMA, BETA, STATS_OUT = 0x80000, 0x90000, 0xA0000, 0xB0000, 0xC0000


def g(M, N, K, dt=BF16, out=None, *, hint=0, flags=0, act=NONE, batch=1, rpb=0, a_batch=0, lda=None, ldc=None, bias=BIAS,
      res=None, c=C, z=None, p_drop=0.0):
    """The argument list of msmd_gemm_ex for a plain (M, K) x (N, K) problem."""
    out = dt if out is None else out
    s = (M * K, N * K, M * N, N, 0) if batch > 1 else (0, 0, 0, 0, 0)
    return (A, W, bias, res, c, M, N, K, dt, out, K if lda is None else lda, rpb, a_batch, K, N if ldc is None else ldc, N,
            act | (hint << 8) | flags, batch, *s, z, p_drop, RNG if p_drop else None, 7, None)


def ln(M, N, K, dt=BF16, *, hint=0, flags=0, act=NONE, a_stats=None, r_stats=None, stats_out=None, slab_in=64, slab_out=64,
       res=None, colsum=None):
    """The argument list of msmd_gemm_ln: operand form with a_stats (+ colsum), residual form otherwise."""
    if a_stats is not None and colsum is None:
        colsum = COLSUM
    if a_stats is None and res is None:
        res = R
    gb = (GAMMA, BETA) if r_stats is not None else (None, None)
    return (A, W, BIAS, res, C, M, N, K, dt, dt, K, K, N, N, act | (hint << 8) | flags, a_stats, colsum, r_stats, *gb,
            stats_out, slab_in if (a_stats or r_stats) else 0, slab_out if stats_out else 0, 1e-5, None)


# 204768 x 512 x 1536 as the strided conv it is: 32 clips of 6399 output rows, 3 taps of 512 channels, stride 2
CONV1 = dict(rpb=6399, lda=1024, a_batch=12799 * 512)

GEMM_ROWS = [
    # --- the library's own choice on the shapes the rule comments name (bf16 -> bf16)
    (17, "6400 x 768 x 768: 75 tiles of 256 x 256", g(6400, 768, 768)),
    (80, "6400 x 2304 x 768: 225 tiles, fill 0.879", g(6400, 2304, 768)),
    (17, "6400 x 3072 x 768: 300 tiles, fill 0.59", g(6400, 3072, 768)),
    (15, "12800 x 768 x 3072: last round favours 192 rows", g(12800, 768, 3072)),
    (17, "12800 x 3072 x 768: last round favours 128 rows", g(12800, 3072, 768)),
    (80, "12800 x 2304 x 768: 450 tiles, fill 0.879", g(12800, 2304, 768)),
    (15, "21312 x 512 x 2048: tall grid, 168 tiles of 256", g(21312, 512, 2048)),
    (80, "21312 x 1536 x 512: 504 tiles, fill 0.98", g(21312, 1536, 512)),
    (80, "204768 x 512 x 1536", g(204768, 512, 1536)),
    (80, "15968 x 1024 x 4096: fill 0.98", g(15968, 1024, 4096)),
    (80, "3584 x 4096 x 1024: fill 0.875 with K >= 1024", g(3584, 4096, 1024)),
    (17, "3584 x 4096 x 768: fill 0.875 with K < 1024", g(3584, 4096, 768)),
    # --- dtypes
    (15, "bf16 -> fp32: no 256 x 256 kernel, tall grid", g(21312, 1536, 512, BF16, F32)),
    (17, "bf16 -> fp32: last-round rule is for 16-bit outputs", g(12800, 768, 3072, BF16, F32)),
    (80, "fp16 -> fp16", g(6400, 2304, 768, F16)),
    (15, "fp16 -> fp16, last-round rule", g(12800, 768, 3072, F16)),
    (15, "fp16 -> fp32, tall grid", g(21312, 1536, 512, F16, F32)),
    (17, "fp16 -> fp32", g(6400, 2304, 768, F16, F32)),
    (0, "fp32 -> fp32", g(6400, 2304, 768, F32)),
    (0, "fp32 -> bf16", g(6400, 2304, 768, F32, BF16)),
    (-1, "fp16 -> bf16 is no pair the library has", g(6400, 2304, 768, F16, BF16)),
    (-1, "bf16 -> fp16 neither", g(6400, 2304, 768, BF16, F16)),
    (-1, "bf16 -> fp16 with hint 17 neither", g(6400, 2304, 768, BF16, F16, hint=17)),
    (-1, "fp16 -> split neither", g(6400, 2304, 768, F16, F16X2)),
    (1, "split -> fp32: 128 x 128 without W_BELOW_32", g(6400, 2304, 768, F16X2, F32)),
    (80, "split -> fp32 with W_BELOW_32", g(6400, 2304, 768, F16X2, F32, flags=W_BELOW_32)),
    (80, "split -> split with W_BELOW_32", g(6400, 2304, 768, F16X2, F16X2, flags=W_BELOW_32)),
    (1, "split -> split", g(6400, 2304, 768, F16X2, F16X2)),
    (80, "split 2816 x 4096 x 64: 176 tiles, fill 0.69", g(2816, 4096, 64, F16X2, F32, flags=W_BELOW_32)),
    (1, "split 6400 x 3072 x 768: fill 0.59", g(6400, 3072, 768, F16X2, F32, flags=W_BELOW_32)),
    (5, "split, small grid", g(200, 768, 768, F16X2, F32, flags=W_BELOW_32)),
    (14, "split, N <= 64 with 256 tiles of 256 rows", g(65536, 64, 128, F16X2, F32)),
    (5, "split, N <= 64 below that", g(65280, 64, 128, F16X2, F32)),
    (-1, "split -> bf16 is rejected", g(6400, 2304, 768, F16X2, BF16)),
    (-1, "split with K % 32 != 0 is rejected", g(6400, 2304, 776, F16X2, F32)),
    (-1, "split with a training epilogue is rejected", g(6400, 2304, 768, F16X2, F32, z=Z)),
    # --- hints (bf16: 9 12 13 14 15 17 66 80; fp16: the same without 13 and 66; split: 1 5 14 80)
    (9, "hint 9", g(6400, 2304, 768, hint=9)),
    (12, "hint 12", g(6400, 2304, 768, hint=12)),
    (13, "hint 13", g(6400, 2304, 768, hint=13)),
    (14, "hint 14", g(6400, 2304, 768, hint=14)),
    (15, "hint 15", g(6400, 2304, 768, hint=15)),
    (17, "hint 17", g(6400, 2304, 768, hint=17)),
    (66, "hint 66", g(6400, 2304, 768, hint=66)),
    (80, "hint 80 on a shape the rule leaves to 128 x 128", g(6400, 768, 768, hint=80)),
    (0, "unknown hint 37: the generic kernel", g(6400, 2304, 768, hint=37)),
    (0, "hint 62 (the removed family) is an unknown hint", g(6400, 2304, 768, hint=62)),
    (17, "hint 80 on bf16 -> fp32: the library's own choice", g(6400, 2304, 768, BF16, F32, hint=80)),
    (9, "fp16 hint 9", g(6400, 2304, 768, F16, hint=9)),
    (12, "fp16 hint 12", g(6400, 2304, 768, F16, hint=12)),
    (14, "fp16 hint 14", g(6400, 2304, 768, F16, hint=14)),
    (15, "fp16 hint 15", g(6400, 2304, 768, F16, hint=15)),
    (17, "fp16 hint 17", g(6400, 2304, 768, F16, hint=17)),
    (80, "fp16 hint 80", g(6400, 768, 768, F16, hint=80)),
    (0, "fp16 hint 13: bf16 only", g(6400, 2304, 768, F16, hint=13)),
    (0, "fp16 hint 66: bf16 only", g(6400, 2304, 768, F16, hint=66)),
    (0, "fp16 unknown hint 37", g(6400, 2304, 768, F16, hint=37)),
    (17, "fp16 hint 80 the call cannot follow (N = 320)", g(12800, 320, 768, F16, hint=80)),
    (1, "split hint 1", g(6400, 2304, 768, F16X2, F32, hint=1, flags=W_BELOW_32)),
    (5, "split hint 5", g(6400, 2304, 768, F16X2, F32, hint=5)),
    (14, "split hint 14", g(6400, 2304, 768, F16X2, F32, hint=14)),
    (80, "split hint 80 without W_BELOW_32: the folding form", g(6400, 768, 768, F16X2, F32, hint=80)),
    (-1, "split unknown hint 37 is rejected", g(6400, 2304, 768, F16X2, F32, hint=37)),
    (5, "split hint 80 the call cannot follow (K = 32)", g(3200, 768, 32, F16X2, F32, hint=80)),
    (0, "hint on fp32 operands is ignored", g(6400, 2304, 768, F32, hint=17)),
    # --- flags
    (17, "NO_256_TILE", g(6400, 2304, 768, flags=NO_256)),
    (80, "NO_256_TILE does not stop hint 80", g(6400, 2304, 768, hint=80, flags=NO_256)),
    (15, "NO_256_TILE on a tall grid", g(21312, 1536, 512, flags=NO_256)),
    (1, "split NO_256_TILE", g(6400, 2304, 768, F16X2, F32, flags=NO_256 | W_BELOW_32)),
    (1, "split 2816 x 4096 x 64 without W_BELOW_32", g(2816, 4096, 64, F16X2, F32)),
    # --- training epilogues (msmd_gemm_actbwd's flags bit 3 takes the same exits as z_out)
    (17, "z_out: no 256 x 256 kernel", g(6400, 2304, 768, z=Z)),
    (17, "p_drop = 0.1", g(6400, 2304, 768, p_drop=0.1)),
    (17, "z_out: the last-round rule is for inference epilogues", g(12800, 768, 3072, z=Z)),
    (15, "z_out on a tall grid", g(21312, 1536, 512, z=Z)),
    (17, "hint 80 with z_out: the library's own choice", g(6400, 2304, 768, hint=80, z=Z)),
    (17, "fp16 p_drop = 0.1", g(12800, 768, 3072, F16, p_drop=0.1)),
    (-1, "p_drop = 1.5 is rejected", g(6400, 2304, 768, p_drop=1.5)),
    # --- what gemm8_takes declines, on a shape the rule would give it (6400 x 2304 x 768)
    (17, "bias + 8 bytes", g(6400, 2304, 768, bias=BIAS + 8)),
    (80, "no bias", g(6400, 2304, 768, bias=None)),
    (17, "C + 4 bytes: no vector stores", g(6400, 2304, 768, c=C + 4)),
    (17, "ldc % 4 != 0", g(6400, 2304, 768, ldc=2306)),
    (80, "residual", g(6400, 2304, 768, res=R)),
    (17, "residual + 2 bytes", g(6400, 2304, 768, res=R + 2)),
    (80, "GELU", g(6400, 2304, 768, act=GELU)),
    (17, "ELU", g(6400, 2304, 768, act=ELU)),
    (17, "batch = 4", g(6400, 2304, 768, batch=4)),
    (-1, "A + 8 bytes is rejected", (A + 8,) + g(6400, 2304, 768)[1:]),
    # --- what gemm8s_takes declines
    (1, "split bias + 8 bytes", g(6400, 2304, 768, F16X2, F32, flags=W_BELOW_32, bias=BIAS + 8)),
    (-1, "split -> split bias + 8 bytes is rejected", g(6400, 2304, 768, F16X2, F16X2, flags=W_BELOW_32, bias=BIAS + 8)),
    (1, "split -> split residual + 8 bytes", g(6400, 2304, 768, F16X2, F16X2, flags=W_BELOW_32, res=R + 8)),
    (1, "split ldc % 4 != 0", g(6400, 2304, 768, F16X2, F32, flags=W_BELOW_32, ldc=2306)),
    (1, "split ELU", g(6400, 2304, 768, F16X2, F32, flags=W_BELOW_32, act=ELU)),
    (1, "split batch = 4", g(6400, 2304, 768, F16X2, F32, flags=W_BELOW_32, batch=4)),
    (1, "split N = 320", g(12800, 320, 768, F16X2, F32, flags=W_BELOW_32)),
    # --- edge shapes
    (14, "N <= 64 with 256 tiles of 256 rows", g(65536, 64, 768)),
    (12, "N <= 64 below that", g(65280, 64, 768)),
    (9, "N <= 64 below that, K >= 1024", g(65280, 64, 1024)),
    (14, "fp16 N <= 64 with 256 tiles of 256 rows", g(65536, 64, 768, F16)),
    (17, "K = 64: below the 256 x 256 kernel's two K tiles", g(6400, 2304, 64)),
    (0, "K = 96: K % 64 != 0", g(6400, 2304, 96)),
    (0, "K = 96 with hint 17", g(6400, 2304, 96, hint=17)),
    (-1, "K = 100: K % 8 != 0 is rejected", g(6400, 2304, 100)),
    (17, "N = 320: N % 256 != 0", g(12800, 320, 768)),
    (15, "N = 320 on a tall grid", g(51200, 320, 768)),
    (12, "a small grid", g(200, 768, 768)),
    (9, "a small grid, K >= 1024", g(200, 768, 3072)),
    (17, "batch = 4 of 1600 x 768 x 768", g(1600, 768, 768, batch=4)),
    (12, "batch = 4 of a small problem", g(200, 256, 64, batch=4)),
    (14, "batch = 4, N <= 64", g(16384, 64, 128, batch=4)),
    (-1, "M = 0 is rejected", g(0, 2304, 768)),
    # --- windowed A (a strided conv): inside and beyond the 32-bit staging offsets
    (80, "conv1 as windows", g(204768, 512, 1536, **CONV1)),
    (15, "conv1 with clips 80 M elements apart", g(204768, 512, 1536, **dict(CONV1, a_batch=80_000_000))),
    (80, "split conv1 as windows", g(204768, 512, 1536, F16X2, F32, flags=W_BELOW_32, **CONV1)),
    (1, "split conv1 with clips 80 M elements apart", g(204768, 512, 1536, F16X2, F32, flags=W_BELOW_32, **dict(CONV1, a_batch=80_000_000))),
]

LN_ROWS = [
    # --- the three forms on an encoder shape (6400 rows: 300 tiles of 128 x 128 at N = 768)
    (17, "operand form, 6400 x 768 x 768", ln(6400, 768, 768, a_stats=STATS)),
    (80, "operand form, 6400 x 2304 x 768", ln(6400, 2304, 768, a_stats=STATS)),
    (80, "operand form, 32-column slabs in", ln(6400, 2304, 768, a_stats=STATS, slab_in=32)),
    (80, "operand form with GELU, 12800 x 2304 x 768", ln(12800, 2304, 768, a_stats=STATS, act=GELU)),
    (17, "residual form + stats_out", ln(6400, 768, 3072, r_stats=STATS, stats_out=STATS_OUT)),
    (17, "stats_out alone", ln(6400, 768, 768, stats_out=STATS_OUT)),
    (17, "plain residual form", ln(6400, 768, 768)),
    (80, "stats_out on 6400 x 2304 x 768", ln(6400, 2304, 768, stats_out=STATS_OUT)),
    (80, "fp16 operand form", ln(6400, 2304, 768, F16, a_stats=STATS)),
    (15, "last round favours 192 rows", ln(12800, 768, 3072, r_stats=STATS, stats_out=STATS_OUT)),
    (15, "tall grid", ln(21312, 512, 2048, r_stats=STATS, stats_out=STATS_OUT)),
    # --- slabs name the tile family
    (12, "slab_out = 32: 64 x 64 tiles", ln(6400, 768, 768, stats_out=STATS_OUT, slab_out=32)),
    (9, "slab_out = 32, K >= 1024", ln(6400, 768, 3072, stats_out=STATS_OUT, slab_out=32)),
    (12, "slab_out = 32 on a shape the 256 x 256 rule wins", ln(6400, 2304, 768, stats_out=STATS_OUT, slab_out=32)),
    (12, "slab_out = 32 with hint 80", ln(6400, 2304, 768, stats_out=STATS_OUT, slab_out=32, hint=80)),
    (12, "slab_out = 32 with hint 17", ln(6400, 2304, 768, stats_out=STATS_OUT, slab_out=32, hint=17)),
    (17, "slab_out = 64 on a small grid", ln(200, 768, 768, stats_out=STATS_OUT)),
    (12, "a small grid without stats_out", ln(200, 768, 768, a_stats=STATS)),
    (9, "a small grid without stats_out, K >= 1024", ln(200, 768, 3072, a_stats=STATS)),
    (12, "a small grid with hint 17: not its family", ln(200, 768, 768, a_stats=STATS, hint=17)),
    (80, "a small grid with hint 80", ln(200, 768, 768, a_stats=STATS, hint=80)),
    (12, "N % 128 != 0: 64 x 64 tiles", ln(6400, 320, 768, a_stats=STATS)),
    (-1, "slab_out = 64 with N % 128 != 0 is rejected", ln(6400, 320, 768, stats_out=STATS_OUT)),
    # --- hints
    (15, "hint 15", ln(6400, 768, 768, a_stats=STATS, hint=15)),
    (17, "hint 17 on a shape the 256 x 256 rule wins", ln(6400, 2304, 768, a_stats=STATS, hint=17)),
    (66, "hint 66", ln(6400, 768, 768, a_stats=STATS, hint=66)),
    (80, "hint 80", ln(6400, 768, 768, a_stats=STATS, hint=80)),
    (-1, "fp16 hint 66: bf16 only, and no LayerNorm form in the generic kernel", ln(6400, 768, 768, F16, a_stats=STATS, hint=66)),
    (17, "hint 9 is none of its hints: own choice, without the 256 x 256 rule", ln(6400, 2304, 768, a_stats=STATS, hint=9)),
    (17, "NO_256_TILE", ln(6400, 2304, 768, a_stats=STATS, flags=NO_256)),
    (80, "NO_256_TILE does not stop hint 80", ln(6400, 2304, 768, a_stats=STATS, hint=80, flags=NO_256)),
    # --- what gemm8_takes declines of the LayerNorm forms
    (17, "odd M with row statistics", ln(6399, 2304, 768, a_stats=STATS)),
    (17, "odd M with row statistics, hint 80", ln(6399, 2304, 768, a_stats=STATS, hint=80)),
    (80, "odd M with stats_out alone", ln(6655, 2304, 768, stats_out=STATS_OUT)),
    (17, "a_stats + 8 bytes", ln(6400, 2304, 768, a_stats=STATS + 8)),
    (17, "r_stats + 8 bytes", ln(6400, 2304, 768, r_stats=STATS + 8)),
    (17, "residual form with GELU", ln(6400, 2304, 768, r_stats=STATS, act=GELU)),
    (80, "residual + 8 bytes: aligned enough for its 8-byte reads", ln(6400, 2304, 768, res=R + 8)),
    # --- rejected calls
    (-1, "operand form with a residual", ln(6400, 2304, 768, a_stats=STATS, res=R)),
    (-1, "K % 64 != 0", ln(6400, 2304, 800, a_stats=STATS)),
    (-1, "a_stats + 4 bytes", ln(6400, 2304, 768, a_stats=STATS + 4)),
    (-1, "fp32 rows", ln(6400, 2304, 768, F32, a_stats=STATS)),
]


def _check(fn, rows):
    seen = set()
    bad = []
    for want, label, args in rows:
        got = fn(*args)
        seen.add(want)
        if got != want:
            bad.append(f"{label}: routed to {got}, the table says {want}")
    assert not bad, "\n".join(bad)
    return seen


def test_gemm_route_table():
    lib = _lib.load()
    assert _check(lib.msmd_gemm_route, GEMM_ROWS) == {-1, 0, 1, 5, 9, 12, 13, 14, 15, 17, 66, 80}
    assert _check(lib.msmd_gemm_ln_route, LN_ROWS) == {-1, 9, 12, 15, 17, 66, 80}
    # pure functions of their arguments: the same answer in any order, any number of times
    assert _check(lib.msmd_gemm_route, GEMM_ROWS[::-1]) and _check(lib.msmd_gemm_ln_route, LN_ROWS[::-1])
