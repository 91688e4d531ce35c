"""msmd_pos_conv (csrc/pos_conv.hip): the encoders' grouped positional conv with each block of frames and its halo staged
once in LDS, against (a) the two launches it replaces, bit for bit, and (b) a float64 grouped conv + GELU + residual."""
import math

import numpy as np
import pytest
import torch

from test_kernels_gpu import _ulp_of_row_max      # the bound of test_gemm_every_routed_variant_meets_the_float64_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
KPOS = 128

# (B, T, G, cg): T shorter than the pad (both zero halos inside one block); a partial last fragment row and a clip boundary
# that must not leak the neighbouring clip's rows; two row blocks sharing a halo; the HuBERT-large group width
SHAPES = [(2, 5, 16, 48), (2, 130, 16, 48), (1, 300, 16, 48), (1, 70, 16, 64)]

_inputs = {}


def _case(shape):
    """fp32 inputs of a shape and the float64 conv of each 16-bit rounding of them, computed once and left unchanged"""
    if shape not in _inputs:
        B, T, G, cg = shape
        g = torch.Generator(device="cpu").manual_seed(1280 + T + cg)
        x = torch.randn(B, T, G * cg, generator=g)
        w = torch.randn(G * cg, cg, KPOS, generator=g) / math.sqrt(KPOS * cg)       # torch Conv1d layout (out, in / G, k)
        b = torch.randn(G * cg, generator=g)
        _inputs[shape] = (x, w, b, {})
    return _inputs[shape]


def _reference(shape, dtype):
    x, w, b, refs = _case(shape)
    if dtype not in refs:
        B, T, G, cg = shape
        xr, wr = x.to(dtype).double().numpy(), w.to(dtype).double().numpy()
        xp = np.zeros((B, T + KPOS, G * cg))
        xp[:, KPOS // 2:KPOS // 2 + T] = xr
        conv = np.empty((B, T, G * cg))
        for gi in range(G):
            sl = slice(gi * cg, (gi + 1) * cg)
            win = np.lib.stride_tricks.sliding_window_view(xp[:, :, sl], KPOS, axis=1)[:, :T]     # (B, T, cg_in, tap)
            conv[:, :, sl] = np.einsum("btck,ock->bto", win, wr[sl])
        z = torch.from_numpy(conv + b.double().numpy())
        refs[dtype] = (torch.nn.functional.gelu(z) + torch.from_numpy(xr)).reshape(B * T, G * cg)
    return refs[dtype]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", SHAPES)
def test_pos_conv_equals_group_pad_gemm_and_meets_the_float64_reference(shape, dtype):
    from msmd_amd import ops as o
    B, T, G, cg = shape
    x, w, b, _ = _case(shape)
    d = G * cg
    h = x.to(DEV, dtype)
    # the encoder's packing: (G, cg, kpos * cg), K index = tap * cg + channel
    wp = w.reshape(G, cg, cg, KPOS).permute(0, 1, 3, 2).reshape(G, cg, KPOS * cg).contiguous().to(DEV, dtype)
    bias = b.to(DEV)
    got = o.pos_conv(h, wp, bias, G, KPOS)
    # the two launches it replaces (utils/wav2vec2.py encode_features)
    xp = o.group_pad(h, G, KPOS // 2, cg_out=cg)
    Tp = T + KPOS
    two = torch.empty_like(h)
    o.gemm(xp, wp, bias, h, o.ACT_GELU, out=two, M=B * T, N=cg, K=KPOS * cg, lda=cg, rows_per_batch=T,
           a_batch_stride=G * Tp * cg, ldw=KPOS * cg, ldc=d, batch=G, strideA=Tp * cg, strideW=cg * KPOS * cg, strideC=cg,
           strideBias=cg, strideR=cg)
    torch.cuda.synchronize()
    assert torch.equal(got, two), (shape, dtype, int((got != two).sum()))
    ref = _reference(shape, dtype)
    err = (got.reshape(B * T, d).double().cpu() - ref).abs()
    bound = _ulp_of_row_max(ref, dtype)
    print(f"pos_conv {shape} {dtype}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    bad = err > bound
    assert not bool(bad.any()), (shape, dtype, int(bad.sum()), float(err.max()))
