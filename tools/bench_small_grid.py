"""The launches whose grids do not match the 256 CUs, in isolation: the encoder's self-attention (T = 200, 12 heads) at
B H = 384 and 768 units, alone and with four prefetch ranges, and the decoder's LayerNorm-residual GEMMs (3552 x 512 x 512 and
x 2048, statistics in and out) on the 128 x 128 tile (hint 17) and the 64 x 128 tile (hint 18).  Each hot (back to back, median
of 30 groups of 20) and cold (a 512 MB fill between launches, as in the step where other kernels' data has passed through
the caches; median of 30 single launches).  With `scan` it then times both tiles by hint over grids of 32 ... 256 tiles of 128 x 128 (N = 512,
K = 512 and 2048): where the routing bounds of the 64 x 128 tile come from.
   python tools/bench_small_grid.py [dtype=bf16] [scan]   (MSMD_LIB: another build)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msmd_amd import ops

dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[sys.argv[1] if len(sys.argv) > 1 else "bf16"]
g = torch.Generator(device="cuda").manual_seed(0)
rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")


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


def report(name, fn):
    print(f"{name:64s} hot {timed(fn, False):7.2f} us   cold {timed(fn, True):7.2f} us", flush=True)


H, T = 12, 200
weights = tuple((rn(n) / 28).to(dt) for n in (768 * 768, 3072 * 768, 768 * 3072, 2304 * 768))
for B in (32, 64):
    qkv = rn(B, T, 3 * H * 64).to(dt)
    q, k, v = qkv[..., :H * 64], qkv[..., H * 64:2 * H * 64], qkv[..., 2 * H * 64:]
    report(f"attention B H = {B * H}, T = {T}", lambda: ops.attention(q, k, v, H, 0.125))
    report(f"attention B H = {B * H}, T = {T}, 4 prefetch ranges (14 MB)", lambda: ops.attention(q, k, v, H, 0.125, prefetch=weights))

M, N = 3552, 512
for K in (512, 2048):
    a, u = rn(M, K).to(dt), rn(M, N).to(dt)
    w, b = (rn(N, K) / K ** 0.5).to(dt), rn(N)
    gam, bet = rn(N).abs() + 0.5, rn(N) * 0.1
    st = torch.stack([u.float().reshape(M, N // 64, 64).sum(-1), (u.float() ** 2).reshape(M, N // 64, 64).sum(-1)], -1).transpose(0, 1).contiguous()
    call = lambda: ops.gemm_ln(a, w, b, u, r_stats=st, r_gamma=gam, r_beta=bet, stats_out=True)
    outs = {}
    for tile in (17, 18):
        ops.GEMM_LN_TILE = tile
        try:
            outs[tile] = call()
            report(f"gemm_ln {M} x {N} x {K}, LN(residual) + stats out, tile hint {tile}", call)
        finally:
            ops.GEMM_LN_TILE = None
    same = all(torch.equal(x, y) for x, y in zip(outs[17], outs[18]))
    report(f"gemm_ln {M} x {N} x {K}, LN(residual) + stats out, library's choice", call)
    print(f"    hints 17 and 18: {'the same bits' if same else 'DIFFERENT RESULTS'}")

# `scan` as a second argument: where the 64 x 128 tile's routing bounds sit -- both tiles by hint over grids of 32 ... 256 tiles of 128 x 128
if len(sys.argv) > 2 and sys.argv[2] == "scan":
    for K in (512, 2048):
        for tiles in (32, 48, 64, 80, 96, 128, 160, 176, 192, 224, 256):
            M = tiles // 4 * 128 - 32
            a, u = rn(M, K).to(dt), rn(M, N).to(dt)
            w, b = (rn(N, K) / K ** 0.5).to(dt), rn(N)
            gam, bet = rn(N).abs() + 0.5, rn(N) * 0.1
            st = torch.stack([u.float().reshape(M, N // 64, 64).sum(-1), (u.float() ** 2).reshape(M, N // 64, 64).sum(-1)], -1).transpose(0, 1).contiguous()
            call = lambda: ops.gemm_ln(a, w, b, u, r_stats=st, r_gamma=gam, r_beta=bet, stats_out=True)
            row = []
            for tile in (17, 18):
                ops.GEMM_LN_TILE = tile
                try:
                    row += [timed(call, False), timed(call, True)]
                finally:
                    ops.GEMM_LN_TILE = None
            print(f"scan {M:5d} x {N} x {K:4d} ({tiles:3d} tiles of 128 x 128): hint 17 hot {row[0]:6.2f} cold {row[1]:6.2f}   hint 18 hot {row[2]:6.2f} cold {row[3]:6.2f} us", flush=True)
