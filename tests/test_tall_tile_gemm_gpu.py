"""The 160 x 128 member of variant 17 (gemm2_kernel<160, 128, 5 x 2 waves, 4-stage ring>; nine of its ten waves stage the K
tiles) against the 128 x 128 tile it shares the wave tile, the k order and the epilogue with: msmd_gemm_ln's residual form with
MSMD_GEMM_FORCE_160_ROW_TILE against the same call with MSMD_GEMM_NO_160_ROW_TILE, the same bits in the output and in the
stored-row statistics, with and without statistics on either side; and both against the float64 reference at the bound of
tests/test_small_grid_gemm_gpu.py (two units in the last place at the row's largest value; statistics to 1e-5 of the row's
sum of squares).

Shapes: M = 150 (one partial 160-row tile), 161 (one row into a second tile) and 330 (two tiles and a partial one); N = 128 and
256 (one and two N tiles: the XCD grid with xn = 1 and 2); K = 64, 128, 256 and 320 (1, 2, 4 and 5 K tiles: below, at and
above the ring's depth, so the short prologue, the steady state and the tail all run)."""
import math

import pytest
import torch

from test_gemm_route_cpu import ln as ln_route_args, STATS, STATS_OUT
from test_kernels_gpu import _ulp_of_row_max
from test_small_grid_gemm_gpu import slab_stats, moments

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_160, FORCE_160 = 1 << 22, 1 << 23
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(M, N, K) for M in (150, 161, 330) for N in (128, 256) for K in (64, 128, 256, 320)]


def ops():
    from msmd_amd import ops as _ops
    return _ops


def lib():
    from msmd_amd import _lib
    return _lib.load()


def with_flags(flags, fn):
    from msmd_amd import ops as O
    saved, O.GEMM_LN_FLAGS = O.GEMM_LN_FLAGS, flags
    try:
        return fn()
    finally:
        O.GEMM_LN_FLAGS = saved


@pytest.mark.parametrize("dtype", DTYPES)
def test_forms_with_statistics_out_same_bits_as_the_128_tile_and_within_the_float64_bound(dtype):
    o = ops()
    assert o.GEMM_FORCE_160_ROW_TILE == FORCE_160 and o.GEMM_NO_160_ROW_TILE == NO_160
    dt = 1 if dtype == torch.bfloat16 else 2
    g = torch.Generator(device="cpu").manual_seed(160)
    for M, N, K in SHAPES:
        for kw in (dict(r_stats=STATS, stats_out=STATS_OUT), dict(stats_out=STATS_OUT)):      # the forced call does run the member
            assert lib().msmd_gemm_ln_rows(*ln_route_args(M, N, K, dt, flags=FORCE_160, **kw)) == 160
            assert lib().msmd_gemm_ln_rows(*ln_route_args(M, N, K, dt, flags=NO_160, **kw)) == 128
        u0 = (torch.randn(M, N, generator=g) * 2 + 0.3).to(DEV, dtype)
        a = torch.randn(M, K, generator=g).to(DEV, dtype)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV, dtype)
        b = torch.randn(N, generator=g).to(DEV)
        g0, be0 = (torch.rand(N, generator=g) + 0.5).to(DEV), (torch.randn(N, generator=g) * 0.1).to(DEV)
        st0 = slab_stats(u0)
        mu0, rs0 = moments(st0, N)
        lin = a.double() @ w.double().T + b.double()
        refs = {True: lin + (u0.double() - mu0) * rs0 * g0.double() + be0.double(), False: lin + u0.double()}
        for r_in in (True, False):      # without statistics out these grids are 64 x 64-tile calls: that half is the next test's
            kw = dict(r_stats=st0, r_gamma=g0, r_beta=be0) if r_in else {}
            call = lambda: o.gemm_ln(a, w, b, u0, stats_out=True, **kw)
            tall, base = with_flags(FORCE_160, call), with_flags(NO_160, call)
            assert torch.equal(tall[0], base[0]), (M, N, K, r_in, int((tall[0] != base[0]).sum()))
            assert torch.equal(tall[1], base[1]), (M, N, K, r_in, "statistics")
            ref = refs[r_in]
            assert not bool(((tall[0].double() - ref).abs() > 2 * _ulp_of_row_max(ref, dtype)).any()), (M, N, K, r_in)
            want = slab_stats(tall[0]).double()
            assert tall[1].shape == want.shape
            assert float(((tall[1].double() - want).abs() / want[..., 1:2].clamp_min(1.0)).max()) < 1e-5, (M, N, K, r_in)


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_form_without_statistics_on_a_grid_of_the_128_column_family(dtype):
    """Without statistics out, msmd_gemm_ln is in the 128-column family from 192 tiles of 128 x 128 on: the form with neither
    statistics, and with statistics in only, at 3050 x 1024 (24 x 8 tiles of 128 x 128, 20 x 8 of 160 x 128 with a ragged last
    row of tiles), K = 64 and 320."""
    o = ops()
    dt = 1 if dtype == torch.bfloat16 else 2
    g = torch.Generator(device="cpu").manual_seed(161)
    M, N = 3050, 1024
    for K in (64, 320):
        u0 = (torch.randn(M, N, generator=g) * 2 + 0.3).to(DEV, dtype)
        a = torch.randn(M, K, generator=g).to(DEV, dtype)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV, dtype)
        b = torch.randn(N, generator=g).to(DEV)
        g0, be0 = (torch.rand(N, generator=g) + 0.5).to(DEV), (torch.randn(N, generator=g) * 0.1).to(DEV)
        st0 = slab_stats(u0)
        mu0, rs0 = moments(st0, N)
        lin = a.double() @ w.double().T + b.double()
        for r_in, ref in ((True, lin + (u0.double() - mu0) * rs0 * g0.double() + be0.double()), (False, lin + u0.double())):
            assert lib().msmd_gemm_ln_rows(*ln_route_args(M, N, K, dt, flags=FORCE_160, r_stats=STATS if r_in else None)) == 160
            assert lib().msmd_gemm_ln_rows(*ln_route_args(M, N, K, dt, flags=NO_160, r_stats=STATS if r_in else None)) == 128
            kw = dict(r_stats=st0, r_gamma=g0, r_beta=be0) if r_in else {}
            call = lambda: o.gemm_ln(a, w, b, u0, **kw)
            tall, base = with_flags(FORCE_160, call), with_flags(NO_160, call)
            assert torch.equal(tall, base), (K, r_in, int((tall != base).sum()))
            assert not bool(((tall.double() - ref).abs() > 2 * _ulp_of_row_max(ref, dtype)).any()), (K, r_in)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_encoder_clip_has_the_same_bits_alone_and_in_a_batch_of_32(dtype):
    """The audio encoder (2 layers) on one four-second clip alone (200 rows: 128 x 128 tiles) and as clip 0 of 32 (6400 rows: the
    out-projection and FFN-2 of every layer run the 160 x 128 member): the same bits."""
    from msmd_amd import synth
    from msmd_amd.config import synthetic_args
    from msmd_amd.model import get_diffusion_model
    dt = 1 if dtype == "bf16" else 2
    kw = dict(r_stats=STATS, stats_out=STATS_OUT)
    for K in (768, 3072):
        assert lib().msmd_gemm_ln_rows(*ln_route_args(6400, 768, K, dt, **kw)) == 160
        assert lib().msmd_gemm_ln_rows(*ln_route_args(200, 768, K, dt, **kw)) == 128
    model = get_diffusion_model(synthetic_args(compute_dtype=dtype, encoder_layers=2, n_layers=2), DEV).eval()
    audio = torch.from_numpy(synth.audio_clips(32, 64000, tag="talltile")).to(DEV)
    with torch.no_grad():
        batch, alone = model.extract_audio_feature(audio), model.extract_audio_feature(audio[:1])
    torch.cuda.synchronize()
    assert batch.shape[0] == 32 and batch.shape[1:] == alone.shape[1:] and bool(torch.isfinite(batch).all())
    assert torch.equal(batch[0], alone[0]), int((batch[0] != alone[0]).sum())
