"""The 64 x 128 tile (variant 18: gemm2_kernel<64, 128, 2 x 2 waves, 4-stage ring>) against the 128 x 128 tile (17) it shares
the wave tile, the k order and the epilogues with: the same bits on the same operands, outputs and stored-row statistics, in
the plain form with a residual and in msmd_gemm_ln's LayerNorm-operand and LayerNorm-residual forms, plus the float64
reference at the bound of test_kernels_gpu.py::test_gemm_ln_forms_meet_the_float64_reference (two units in the last place at
the row's largest value; statistics to 1e-5 of the row's sum of squares).

Shapes: M = 70 (two 64-row tiles, the last ragged with clamped rows; one 128-row tile) and 130 (three / two); N = 128 and 256
(one and two N tiles: the XCD grid with xn = 1 and 2); K = 64 (one K tile, fewer than the ring's three-tile prologue), 128,
256 (the ring depth) and 320 (five tiles: the ring wraps).  msmd_gemm_ln's hints choose inside the 128-column family only; a
call that writes no statistics is in that family from 192 tiles of 128 x 128 on, so the LayerNorm-operand form is compared at
2950 x 1024 (24 x 8 tiles, a ragged last M tile) with K = 64 and 320."""
import math

import pytest
import torch

from test_gemm_route_cpu import ln as ln_route_args, STATS, STATS_OUT
from test_kernels_gpu import _ulp_of_row_max

pytestmark = pytest.mark.gpu
DEV = "cuda"
GV_128, GV_64x128 = 17, 18
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(M, N, K) for M in (70, 130) for N in (128, 256) for K in (64, 128, 256, 320)]


def ops():
    from msmd_amd import ops as _ops
    return _ops


def lib():
    from msmd_amd import _lib
    return _lib.load()


def slab_stats(x):
    """(cols / 64, M, 2) fp32 partial (sum, sum of squares) of x's rows over 64-column slabs, from float64"""
    xs = x.double().reshape(x.shape[0], -1, 64)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).transpose(0, 1).float().contiguous()


def moments(st, cols):
    S, Q = st.double().sum(0)[:, 0], st.double().sum(0)[:, 1]
    mu = S / cols
    return mu[:, None], torch.rsqrt((Q / cols - mu * mu).clamp_min(0) + 1e-5)[:, None]


def on_tile(tile, fn):
    from msmd_amd import ops as O
    O.GEMM_LN_TILE = tile
    try:
        return fn()
    finally:
        O.GEMM_LN_TILE = None


@pytest.mark.parametrize("dtype", DTYPES)
def test_plain_form_with_residual_same_bits_as_the_128_tile(dtype):
    o = ops()
    g = torch.Generator(device="cpu").manual_seed(18)
    for M, N, K in SHAPES:
        a = torch.randn(M, K, generator=g).to(DEV, dtype)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV, dtype)
        b = torch.randn(N, generator=g).to(DEV)
        r = torch.randn(M, N, generator=g).to(DEV, dtype)
        for act in (o.ACT_NONE, o.ACT_GELU):
            for res in (r, None):
                c18 = o.gemm(a, w, b, res, act=act, variant=GV_64x128, flags=0)
                c17 = o.gemm(a, w, b, res, act=act, variant=GV_128, flags=0)
                assert torch.equal(c18, c17), (M, N, K, act, res is not None, int((c18 != c17).sum()))
        ref = a.double() @ w.double().T + b.double() + r.double()
        got = o.gemm(a, w, b, r, variant=GV_64x128, flags=0).double()
        assert not bool(((got - ref).abs() > 2 * _ulp_of_row_max(ref, dtype)).any()), (M, N, K)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_residual_form_same_bits_and_statistics_as_the_128_tile(dtype):
    o = ops()
    dt = 1 if dtype == torch.bfloat16 else 2
    g = torch.Generator(device="cpu").manual_seed(1817)
    for M, N, K in SHAPES:
        for hint in (GV_64x128, GV_128):     # the hint is one the call follows
            assert lib().msmd_gemm_ln_route(*ln_route_args(M, N, K, dt, hint=hint, r_stats=STATS, stats_out=STATS_OUT)) == hint
            assert lib().msmd_gemm_ln_route(*ln_route_args(M, N, K, dt, hint=hint, stats_out=STATS_OUT)) == hint
        u0 = (torch.randn(M, N, generator=g) * 2 + 0.3).to(DEV, dtype)
        a = torch.randn(M, K, generator=g).to(DEV, dtype)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV, dtype)
        b = torch.randn(N, generator=g).to(DEV)
        g0, be0 = (torch.rand(N, generator=g) + 0.5).to(DEV), (torch.randn(N, generator=g) * 0.1).to(DEV)
        st0 = slab_stats(u0)
        with_ln = lambda: o.gemm_ln(a, w, b, u0, r_stats=st0, r_gamma=g0, r_beta=be0, stats_out=True)
        without = lambda: o.gemm_ln(a, w, b, u0, stats_out=True)
        (c18, s18), (p18, q18) = on_tile(GV_64x128, with_ln), on_tile(GV_64x128, without)
        (c17, s17), (p17, q17) = on_tile(GV_128, with_ln), on_tile(GV_128, without)
        assert torch.equal(c18, c17) and torch.equal(s18, s17), (M, N, K, "r_stats")
        assert torch.equal(p18, p17) and torch.equal(q18, q17), (M, N, K, "no r_stats")
        mu0, rs0 = moments(st0, N)
        lin = a.double() @ w.double().T + b.double()
        for got, st, ref in ((c18, s18, lin + (u0.double() - mu0) * rs0 * g0.double() + be0.double()), (p18, q18, lin + u0.double())):
            assert not bool(((got.double() - ref).abs() > 2 * _ulp_of_row_max(ref, dtype)).any()), (M, N, K)
            want = slab_stats(got).double()
            assert st.shape == want.shape
            assert float(((st.double() - want).abs() / want[..., 1:2].clamp_min(1.0)).max()) < 1e-5, (M, N, K)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_operand_form_same_bits_as_the_128_tile(dtype):
    o = ops()
    dt = 1 if dtype == torch.bfloat16 else 2
    g = torch.Generator(device="cpu").manual_seed(1802)
    M, N = 2950, 1024
    for K in (64, 320):
        for hint in (GV_64x128, GV_128):
            assert lib().msmd_gemm_ln_route(*ln_route_args(M, N, K, dt, hint=hint, a_stats=STATS)) == hint
        x = (torch.randn(M, K, generator=g) * 2 + 0.3).to(DEV, dtype)
        st = slab_stats(x)
        wf, cs, bf = o.fold_layernorm(torch.randn(N, K, generator=g).to(DEV) / math.sqrt(K), torch.randn(N, generator=g).to(DEV),
                                      (torch.rand(K, generator=g) + 0.5).to(DEV), (torch.randn(K, generator=g) * 0.1).to(DEV), dtype)
        for act in (o.ACT_NONE, o.ACT_GELU):
            call = lambda: o.gemm_ln(x, wf, bf, act=act, a_stats=st, w_colsum=cs)
            f18, f17 = on_tile(GV_64x128, call), on_tile(GV_128, call)
            assert torch.equal(f18, f17), (K, act, int((f18 != f17).sum()))
            mu, rs = moments(st, K)
            ref = rs * (x.double() @ wf.double().T - mu * cs.double()) + bf.double()
            if act == o.ACT_GELU:
                ref = torch.nn.functional.gelu(ref)
            assert not bool(((f18.double() - ref).abs() > 2 * _ulp_of_row_max(ref, dtype)).any()), (K, act)


def test_the_decoders_residual_gemms_route_to_the_64_row_tile():
    route = lib().msmd_gemm_ln_route
    for M, N, K in ((3552, 512, 512), (3552, 512, 2048)):       # 28 x 4 = 112 tiles of 128 x 128 on 256 CUs
        assert route(*ln_route_args(M, N, K, r_stats=STATS, stats_out=STATS_OUT)) == GV_64x128
        assert route(*ln_route_args(M, N, K, 2, stats_out=STATS_OUT)) == GV_64x128
    for M, N, K in ((6400, 768, 768), (10656, 512, 2048)):      # 300 and 336 tiles: as before
        assert route(*ln_route_args(M, N, K, r_stats=STATS, stats_out=STATS_OUT)) == GV_128
        assert route(*ln_route_args(M, N, K, stats_out=STATS_OUT)) == GV_128


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_decoder_clip_has_the_same_bits_alone_and_in_a_batch_of_32(dtype):
    """The denoiser (2 layers) on one clip alone (111 rows: one 128 x 128 tile per N tile, variant 17) and as clip 0 of 32
    (3552 rows: variant 18): every LayerNorm-residual GEMM of the trunk runs on another tile, the result is the same bits."""
    import numpy as np
    from helpers import denoiser_inputs
    from msmd_amd.config import synthetic_args
    from msmd_amd.model import get_diffusion_model
    args = synthetic_args(compute_dtype=dtype, encoder_layers=2, n_layers=2)
    model = get_diffusion_model(args, DEV).eval()
    x = denoiser_inputs(32, args, tag="smallgrid")
    t = lambda v, n: torch.from_numpy(np.ascontiguousarray(v[:n])).to(DEV)

    def run(n):
        person = torch.cat([t(x["shape"], n)[:, None], t(x["style"], n)[:, None]], dim=-1)
        step = torch.full((n,), 250, dtype=torch.long, device=DEV)
        return model.denoising_net(t(x["motion"], n), t(x["audio_feat"], n), person, t(x["style"], n)[:, None],
                                   t(x["prev_motion"], n), t(x["prev_audio"], n), step, t(x["indicator"], n))

    batch, alone = run(32), run(1)
    torch.cuda.synchronize()
    assert batch.shape == (32, 110, 67) and bool(torch.isfinite(batch).all())
    assert torch.equal(batch[0], alone[0]), int((batch[0] != alone[0]).sum())
