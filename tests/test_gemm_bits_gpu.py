"""The bits every GEMM kernel family returns, as a recorded table.

The other GEMM tests compare variants with each other and with float64 within a tolerance.  A change of the k order or of the
MFMA sequence made in a piece the kernels SHARE (csrc/gemm_tiles.h, the "shared pieces" of csrc/gemm.hip) moves all variants
together and stays inside those tolerances; this test holds each family to the SHA-256 of its outputs instead -- C, and where
the call produces them the pre-activation copy and the LayerNorm statistics -- on seeded inputs generated on the host.

tests/golden/gemm_bits.json was recorded from the library of the commit BEFORE the device half of csrc/gemm.hip was
refactored: that commit's libmsmd_hip.so, built beside this checkout and loaded through MSMD_LIB, ran this module's own recorder

    MSMD_LIB=<the parent's csrc/libmsmd_hip.so> python tests/test_gemm_bits_gpu.py --record FILE

twice, with identical files.  It is not an output of the code under test.  A row whose variant the library declines falls back
to the library's own choice: still one deterministic launch.

Shapes are the smallest that reach every code path: M = 334 (even, ragged against every tile height), N = 264 (N % 8 == 0,
ragged against 64 and 128), K = 320 (five K tiles of 64, one more than the deepest ring: prologue, steady state and drain).
Every output buffer is zero-filled first, so bytes a launch leaves alone (padding columns) hash the same."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from msmd_amd import _lib, ops, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_bits.json")
M, N, K = 334, 264, 320
NONE, GELU = ops.ACT_NONE, ops.ACT_GELU
PAIRED, WT = ops.GEMM_PAIRED_STORES, ops.GEMM_WRITE_THROUGH
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def normal(tag, shape, dt=torch.float32, scale=1.0):
    g = np.random.default_rng(synth.name_seed(f"gemm_bits/{tag}") & 0xFFFFFFFF)
    return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32)).to(DEV).to(dt)


def zeros(shape, dt):
    return torch.zeros(shape, device=DEV, dtype=dt)


def digest(*outs):
    h = hashlib.sha256()
    for t in outs:
        t = t.t if isinstance(t, ops.Split) else t
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def operands(tag, m, n, k, dt):
    """A (m, k), W (n, k), bias (n) fp32."""
    return normal(f"{tag}/a", (m, k), dt), normal(f"{tag}/w", (n, k), dt, 0.06), normal(f"{tag}/bias", (n,))


# ----------------------------------------------------------------------------- the calls
def plain(dt, variant, epilogue, flags, m=M, n=N, k=K):
    """msmd_gemm on 16-bit operands.  Epilogue "full": bias + GELU + residual, 16-bit out; "bare": nothing, fp32 out."""
    a, w, bias = operands(f"plain/{m}x{n}x{k}", m, n, k, DT[dt])
    if epilogue == "full":
        out, res = zeros((m, n), DT[dt]), normal(f"plain/{m}x{n}/res", (m, n), DT[dt])
        return digest(ops.gemm(a, w, bias, res, GELU, out=out, variant=variant, flags=flags))
    act = GELU if epilogue == "gelu" else NONE
    out = zeros((m, n), DT[dt] if epilogue in ("gelu", "none16") else torch.float32)
    return digest(ops.gemm(a, w, None if epilogue == "bare" else bias, None, act, out=out, variant=variant, flags=flags))


def ln_residual(dt, hint, flags, with_r_stats, m=M, n=256, k=K):
    """msmd_gemm_ln, residual form: C = A W^T + bias + LN(R) or + R, with the statistics of the stored rows."""
    a, w, bias = operands(f"ln_res/{m}x{n}x{k}", m, n, k, DT[dt])
    res = normal("ln_res/res", (m, n), DT[dt])
    kw = {}
    if with_r_stats:
        r = res.float().view(m, n // 64, 64)
        kw = dict(r_stats=torch.stack([r.sum(-1), (r * r).sum(-1)], -1).permute(1, 0, 2).contiguous(),
                  r_gamma=1.0 + normal("ln_res/gamma", (n,), scale=0.1), r_beta=normal("ln_res/beta", (n,), scale=0.1))
    old = ops.GEMM_LN_TILE, ops.GEMM_LN_FLAGS
    ops.GEMM_LN_TILE, ops.GEMM_LN_FLAGS = hint, flags
    try:
        out, st = ops.gemm_ln(a, w, bias, res, NONE, out=zeros((m, n), DT[dt]), stats_out=True, **kw)
    finally:
        ops.GEMM_LN_TILE, ops.GEMM_LN_FLAGS = old
    return digest(out, st)


def ln_operand(dt, hint, flags, act, m=M, n=512, k=K):
    """msmd_gemm_ln, operand form: C = act(LN(A) W'^T + bias) from A's partial statistics and W' row sums."""
    a, w, bias = operands(f"ln_op/{m}x{n}x{k}", m, n, k, DT[dt])
    u = a.float().view(m, k // 64, 64)
    a_stats = torch.stack([u.sum(-1), (u * u).sum(-1)], -1).permute(1, 0, 2).contiguous()
    old = ops.GEMM_LN_TILE, ops.GEMM_LN_FLAGS
    ops.GEMM_LN_TILE, ops.GEMM_LN_FLAGS = hint, flags
    try:
        out = ops.gemm_ln(a, w, bias, None, act, out=zeros((m, n), DT[dt]), a_stats=a_stats, w_colsum=w.float().sum(1).contiguous())
    finally:
        ops.GEMM_LN_TILE, ops.GEMM_LN_FLAGS = old
    return digest(out)


def rng_state():
    return torch.tensor([4321, 3], dtype=torch.int64, device=DEV)


def training(variant):
    """msmd_gemm_ex: pre-activation copy and dropout on GELU(.) before the residual add (bf16)."""
    a, w, bias = operands("train", M, N, K, torch.bfloat16)
    res, z = normal("train/res", (M, N), torch.bfloat16), zeros((M, N), torch.bfloat16)
    out = ops.gemm(a, w, bias, res, GELU, out=zeros((M, N), torch.bfloat16), z_out=z, p_drop=0.1, rng_state=rng_state(), site=3,
                   variant=variant)
    return digest(out, z)


def act_bwd(p_drop):
    dy, wt, _ = operands("act_bwd", M, 256, K, torch.bfloat16)
    z = normal("act_bwd/z", (M, 256), torch.bfloat16)
    return digest(ops.gemm_act_bwd(dy, wt, z, GELU, p_drop=p_drop, rng_state=rng_state() if p_drop else None, site=3))


def generic(dt, m, n):
    """gemm_kernel on a K tail: K = 100 for fp32; 104 for bf16, whose rows msmd_gemm takes in whole 16-byte chunks only."""
    a, w, bias = operands(f"generic/{m}x{n}", m, n, 100 if dt == "fp32" else 104, DT[dt])
    res = normal(f"generic/{m}x{n}/res", (m, n), DT[dt])
    return digest(ops.gemm(a, w, bias, res, GELU, out=zeros((m, n), DT[dt])))


def conv(dt, variant):
    """The windowed A operand: Conv1d(kernel 3, stride 2) over a channels-last (3, 201, 64) signal as one GEMM."""
    x, w = normal("conv/x", (3, 201, 64), DT[dt]), normal("conv/w", (N, 3 * 64), DT[dt], 0.06)
    with ops.gemm_defaults(variant=variant):
        return digest(ops.conv1d_cl(x, w, normal("conv/bias", (N,)), kernel=3, stride=2, act=GELU))


def batched(dt, product):
    """msmd_gemm_batched2 on the attention products of tests/test_backward_gpu.py: B = 3, H = 8, Tq = 111, Tk = 110."""
    B, H, Tq, Tk, Tkp = 3, 8, 111, 110, 112
    d = H * 64
    if product == "qk":
        q, k = normal("b2/qkv", (B, Tq, 3 * d), DT[dt])[..., :d], normal("b2/kv", (B, Tk, 2 * d), DT[dt])[..., :d]
        P = zeros((B, H, Tq, Tkp), DT[dt])
        ops.gemm_batched2(q, k, P, Tq, Tk, 64, q.stride(1), k.stride(1), Tkp, B, q.stride(0), k.stride(0), H * Tq * Tkp, H, 64, 64,
                          Tq * Tkp)
        return digest(P)
    Pt, VT = normal("b2/p", (B, H, Tq, Tkp), DT[dt]).abs(), normal("b2/vt", (B, H, 64, Tkp), DT[dt])
    Pt[..., Tk:] = 0
    VT[..., Tk:] = 0
    O = zeros((B, Tq, d + 16), DT[dt])
    ops.gemm_batched2(Pt, VT, O, Tq, 64, Tkp, Tkp, Tkp, d + 16, B, H * Tq * Tkp, H * 64 * Tkp, Tq * (d + 16), H, Tq * Tkp, 64 * Tkp, 64)
    return digest(O)


def split(variant, split_out, below_32, m=M, n=N, k=K):
    """Split-pair operands (the f16x2 mode), GELU + residual; C and the residual fp32, or in split storage -- then in rows
    padded to a multiple of 32 columns, which split storage needs (ldc = ldr = 288 for N = 264)."""
    a = ops.to_split(normal(f"split/{m}x{k}/a", (m, k)))
    w = ops.to_split(normal(f"split/{n}x{k}/w", (n, k), scale=0.06))
    w.below_32 = below_32
    bias, npad = normal(f"split/{n}/bias", (n,)), (n + 31) // 32 * 32
    res = normal(f"split/{m}x{n}/res", (m, npad))
    if split_out:
        res, out = ops.to_split(res), ops.Split(zeros((m, 2 * npad), torch.float16))
    else:
        out = zeros((m, npad), torch.float32)
    ops.gemm(a, w, bias, res, GELU, out=out, N=n, ldc=npad, variant=variant)
    return digest(out)


def table():
    rows = {}
    for dt in ("bf16", "fp16"):
        for v in (9, 12, 14, 15, 17, 18) + ((13, 66) if dt == "bf16" else ()):
            for epi in ("full", "bare"):
                for fname, flags in (("none", 0), ("paired", PAIRED), ("paired+write-through", PAIRED | WT)):
                    rows[f"16-bit {dt} variant {v} {epi} stores {fname}"] = (plain, dt, v, epi, flags)
        for m, n, k in ((300, 512, 128), (1100, 256, 192)):     # no steady-state K tile of the 8-phase schedule, and exactly one
            for epi in ("full", "bare"):
                rows[f"variant 80 {dt} {m}x{n}x{k} {epi}"] = (plain, dt, 80, epi, PAIRED, m, n, k)
        for hint, flags, hname in ((15, 0, "15"), (17, 0, "17"), (18, 0, "18"), (80, 0, "80"), (17, ops.GEMM_FORCE_160_ROW_TILE, "17 forced 160")):
            for rs in (False, True):
                rows[f"gemm_ln residual {dt} tile {hname} r_stats {rs}"] = (ln_residual, dt, hint, flags, rs)
            for act in (NONE, GELU):
                rows[f"gemm_ln operand {dt} tile {hname} act {act}"] = (ln_operand, dt, hint, flags, act)
    # the persistent form: 33 x 16 = 528 tiles > 512 workgroups, ragged last row tile; K = 128: the hand-over to the next tile
    # straight after the first K tile
    for k in (128, 192):
        for epi in ("none16", "gelu"):
            for fname, flags in (("persistent", PAIRED), ("one tile per workgroup", PAIRED | ops.GEMM_ONE_TILE_PER_WORKGROUP)):
                rows[f"variant 17 bf16 4200x2048x{k} {epi} {fname}"] = (plain, "bf16", 17, epi, flags, 4200, 2048, k)
    for act in (NONE, GELU):
        rows[f"gemm_ln operand bf16 4200x2048x128 persistent act {act}"] = (ln_operand, "bf16", 17, 0, act, 4200, 2048, 128)
    for v in (9, 15, 17):
        rows[f"training epilogue bf16 variant {v}"] = (training, v)
    for p in (0.0, 0.1):
        rows[f"gemm_act_bwd bf16 GELU p_drop {p}"] = (act_bwd, p)
    for dt in ("fp32", "bf16"):
        rows[f"generic {dt} 334x200 K tail (64 x 64 tile)"] = (generic, dt, 334, 200)
        rows[f"generic {dt} 1500x1500 K tail (128 x 128 tile)"] = (generic, dt, 1500, 1500)
        for product in ("qk", "pv"):
            rows[f"batched2 {dt} {product}"] = (batched, dt, product)
    rows["windowed conv bf16 variant 15"] = (conv, "bf16", 15)
    rows["windowed conv fp32 generic"] = (conv, "fp32", 0)
    for split_out in (False, True):
        for below in (False, True):
            for v in (1, 5, 14):
                rows[f"split variant {v} split out {split_out} below_32 {below}"] = (split, v, split_out, below)
            rows[f"split variant 80 300x512x96 split out {split_out} below_32 {below}"] = (split, 80, split_out, below, 300, 512, 96)
    return rows


TABLE = table()


def run_row(name):
    f, *args = TABLE[name]
    got = f(*args)
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_the_table(recorded):
    assert sorted(recorded) == sorted(TABLE) and len(TABLE) > 150


@pytest.mark.parametrize("name", list(TABLE))
def test_gemm_bits_are_the_recorded_ones(name, recorded):
    assert run_row(name) == recorded[name], f"{name}: the output bits differ from the parent commit's"


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_gemm_bits_gpu.py --record FILE")
    print(f"recording the bits of {_lib.LIB_PATH}", file=sys.stderr)
    with open(sys.argv[2], "w") as out:
        json.dump({name: run_row(name) for name in TABLE}, out, indent=0, sort_keys=True)
        out.write("\n")
