"""msmd_gemm_ln's residual form with statistics in and out on the tiles of the 128-column family, in isolation: the 128 x 128
tile (hint 17 with the 160-row member opted out), its 160 x 128 member (forced), and for reference the 192 x 128 (hint 15) and
64 x 128 (hint 18) tiles.  Each hot (back to back, median of 30 groups of 20) and cold (a 512 MB fill between launches; median
of 30 single launches), as tools/bench_small_grid.py measures.
   model: the encoder's shapes (M = 6400: 300 tiles of 128 x 128, some CU carries two) against M = 5376 (252 tiles: one per CU)
   scan:  M over the grids around both bounds of the 160-row member's rule, N = 768 / 512, K = 512 / 768 / 2048 / 3072
   python tools/bench_tall_tile.py [dtype=bf16] [model|scan]   (MSMD_LIB: another build; one without the 160-row member times the rest)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msmd_amd import _lib, ops

dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[sys.argv[1] if len(sys.argv) > 1 else "bf16"]
what = sys.argv[2] if len(sys.argv) > 2 else "model"
g = torch.Generator(device="cuda").manual_seed(0)
rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
HAS_160 = hasattr(_lib.load(), "msmd_gemm_ln_rows")


def timed(fn, cold):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    ts = []
    for _ in range(30):
        if cold:
            flush.fill_(1)
        e0.record()
        for _ in range(1 if cold else 20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / (1 if cold else 20))
    return statistics.median(ts)


def forms(M, N, K, which):
    a, u = rn(M, K).to(dt), rn(M, N).to(dt)
    w, b = (rn(N, K) / K ** 0.5).to(dt), rn(N)
    gam, bet = rn(N).abs() + 0.5, rn(N) * 0.1
    st = torch.stack([u.float().reshape(M, N // 64, 64).sum(-1), (u.float() ** 2).reshape(M, N // 64, 64).sum(-1)], -1).transpose(0, 1).contiguous()
    call = lambda: ops.gemm_ln(a, w, b, u, r_stats=st, r_gamma=gam, r_beta=bet, stats_out=True)
    row, outs = [], {}
    for name in which:
        tile, flags = {"128": (17, ops.GEMM_NO_160_ROW_TILE), "160": (17, ops.GEMM_FORCE_160_ROW_TILE), "192": (15, 0), "64": (18, 0),
                       "own": (None, 0)}[name]
        if name == "160" and not HAS_160:
            continue
        ops.GEMM_LN_TILE, ops.GEMM_LN_FLAGS = tile, flags
        try:
            outs[name] = call()
            row.append(f"{name} hot {timed(call, False):6.2f} cold {timed(call, True):6.2f}")
        finally:
            ops.GEMM_LN_TILE, ops.GEMM_LN_FLAGS = None, 0
    same = all(torch.equal(x, y) for o in outs.values() for x, y in zip(o, outs[which[0]]))
    t128, t160 = (M + 127) // 128 * (N // 128), (M + 159) // 160 * (N // 128)
    print(f"{M:5d} x {N} x {K:4d} ({t128:3d} tiles of 128, {t160:3d} of 160): " + "   ".join(row) + ("" if same else "   DIFFERENT RESULTS"), flush=True)


if what == "model":
    for K in (768, 3072):
        for M in (6400, 5376):
            forms(M, 768, K, ("128", "160", "192", "64", "own") if M == 6400 else ("128", "160"))
else:
    for N, Ks in ((768, (768, 3072)), (512, (512, 2048))):
        nt = N // 128
        # grids of 128 x 128 tiles just below and above one per CU, in between, and around the last grid 160-row tiles fit into one round
        Ms = sorted({(256 // nt) * 128, (256 // nt) * 128 + 1, (256 // nt + 4) * 128, (256 // nt) * 160 - 320, (256 // nt // 8 * 8) * 160, (256 // nt // 8 * 8) * 160 + 1})
        for K in Ks:
            for M in Ms:
                forms(M, N, K, ("128", "160", "own"))
