"""The audio front end (csrc/audio.hip) against the float64 references of tests/conv0_ref.py at every dispatch edge: pad_audio,
conv0 + GroupNorm + GELU in its four forms (VALU fp32, VALU split storage, the 16-bit VALU fallback, the 16-bit MFMA
kernel), its statistics on their own, conv0 + LayerNorm + GELU, interp_linear and group_pad.  Every comparison covers every
element.  tests/test_conv0_cpu.py proves the references and the conditions the case set relies on without a GPU.

Bounds: 16-bit outputs one unit in the last place of the type at the frame row's largest reference value; fp32 and split
outputs 2e-5 max(1, row max); the statistics 1e-5 on a normalised value (half of the fp32 figure).

Measured on an MI355X, largest max err / bound over the cases of a kind:
  conv0 + GroupNorm + GELU   fp32 0.032   split 0.033   bf16 0.502   fp16 0.513        (9 shapes)
  constant clip              fp32 0.173   split 0.175   bf16 0.466   fp16 0.473
  quiet clip (sigma 3e-5)    fp32 0.000   bf16 0.500    fp16 0.502
  statistics / 1e-5          z-normalised 0.020   DC 0.211   400 zeros then DC 0.063   constant 0.435   T0 = 7: 0.014
  conv0 + LayerNorm + GELU   fp32 0.014   bf16 0.501    fp16 0.511
  interp_linear              fp32 0.378 and bit-equal to the oracle   bf16 1.000   fp16 1.000 (exact ties of a 0.5 blend)
  group_pad, pad_audio       exact
Before the fixes that came with this file the same cases gave: statistics of the clip of 400 zeros then DC, 8.573 (the split
totals of the moments were rounded to fp32 and centred on the first 256 samples); quiet clip in fp16, 3.169 (the MFMA
kernel split the unscaled signal into two fp16 subnormals); interp_linear in fp32 within its bound (0.365) but one ulp
from the oracle at two shapes (the blend was contracted to mul + fma).
"""
import numpy as np
import pytest
import torch

import conv0_ref as cr
from oracle import nn as onn
from test_kernels_gpu import _ulp_of_row_max      # one ulp of the 16-bit type at each row's largest |reference|

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPLIT = "f16x2"                                   # ops.SPLIT
TYPES = [torch.float32, torch.bfloat16, torch.float16, SPLIT]
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}


def _ops():
    from msmd_amd import ops
    assert ops.SPLIT == SPLIT
    return ops


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _name(t):
    return t if isinstance(t, str) else str(t).replace("torch.", "")


def _check(tag, got, ref, dtype):
    """every element of got (a device tensor or Split, (..., C)) against the float64 reference rows"""
    ref = torch.from_numpy(np.ascontiguousarray(ref)).reshape(-1, ref.shape[-1])
    got = got.float().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), tag
    if dtype in (torch.bfloat16, torch.float16):
        bound = _ulp_of_row_max(ref, dtype)
    else:
        bound = 2e-5 * ref.abs().amax(dim=1, keepdim=True).clamp_min(1.0)
    err = (got - ref).abs()
    print(f"{tag} {_name(dtype)}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    bad = err > bound
    assert not bool(bad.any()), (tag, _name(dtype), int(bad.sum()), float(err.max()), float((err / bound).max()))


def _gn(o, c, r, rep, dtype):
    out = o.conv0_gn_gelu(_dev(c["audio"]), _dev(c["w0"]), _dev(c["gamma"]), _dev(c["beta"]), r, rep, dtype)
    torch.cuda.synchronize()
    return out


GN_PARAMS = [(s, t) for s in cr.gn_shapes() for t in TYPES if not (t == SPLIT and s[4] % 32)]


@pytest.mark.parametrize("shape,dtype", GN_PARAMS, ids=[f"{s}-{_name(t)}" for s, t in GN_PARAMS])
def test_conv0_gn_gelu_meets_the_float64_reference(shape, dtype):
    o = _ops()
    B, L, r, rep, C = shape
    c = cr.gn_case(shape)
    out = _gn(o, c, r, rep, dtype)
    assert tuple(out.shape) == (B, cr.frames(L, r, rep), C)
    _check(f"conv0_gn {shape}", out, c["ref"], dtype)
    if dtype == SPLIT:          # and the relation to the fp32 kernel that test_split_layernorm_and_conv0_outputs asserts
        f = _gn(o, c, r, rep, torch.float32)
        assert isinstance(out, o.Split)
        assert bool(torch.all((out.float() - f).abs() <= f.abs() * 2.0 ** -21 + 1.0e-6))


@pytest.mark.parametrize("name", cr.STATS_CASES)
def test_conv0_stats_meet_the_float64_statistics(name):
    """msmd_conv0_stats through the library handle: mean and rstd from 66 moments of the centred signal"""
    from msmd_amd import _lib
    o = _ops()
    c = cr.stats_case(name)
    B, L = c["audio"].shape
    C = c["w0"].shape[0]
    audio, w0 = _dev(c["audio"]), _dev(c["w0"])
    stats = torch.full((B, C, 2), float("nan"), device=DEV)
    ws = o.conv0_workspace(B, DEV)
    rc = _lib.load().msmd_conv0_stats(audio.data_ptr(), w0.data_ptr(), stats.data_ptr(), ws.data_ptr(), B, L, 0, 0, C, 1e-5,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    s = stats.double().cpu().numpy()
    assert np.isfinite(s).all()
    e = cr.stats_error(c, s[..., 0], s[..., 1])
    print(f"conv0_stats {name}: max |d mean| rstd |gamma|max + zmax |d rstd| / rstd = {e.max():.3e}, / 1e-5 = {e.max() / 1e-5:.3f}")
    if name == "constant":
        assert float(np.abs(s[..., 1] * np.sqrt(1e-5) - 1.0).max()) <= 2.0 ** -22      # variance 0: rstd = 1 / sqrt(eps)
    assert float(e.max()) <= 1e-5, (name, float(e.max()))


@pytest.mark.parametrize("dtype", TYPES, ids=_name)
def test_conv0_gn_gelu_of_a_constant_clip_is_gelu_of_beta(dtype):
    o = _ops()
    c = cr.stats_case("constant")
    _check("conv0_gn constant clip", _gn(o, c, 0, 0, dtype), c["ref"], dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=_name)
def test_conv0_gn_gelu_of_a_quiet_clip(dtype):
    """one LSB of 16-bit noise: the MFMA kernel's fp16 hi / lo halves of the signal are both subnormal; fp32 is the control"""
    o = _ops()
    c = cr.quiet_case()
    _check("conv0_gn quiet clip", _gn(o, c, *cr.QUIET_SHAPE[2:4], dtype), c["ref"], dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=_name)
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", cr.LN_SHAPES, ids=str)
def test_conv0_ln_gelu_meets_the_float64_reference(shape, with_bias, dtype):
    o = _ops()
    B, L, r, rep = shape
    c = cr.ln_case(shape, with_bias)
    out = o.conv0_ln_gelu(_dev(c["audio"]), _dev(c["w0"]), _dev(c["bias"]), _dev(c["gamma"]), _dev(c["beta"]), r, rep, dtype)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (B, cr.frames(L, r, rep), 512)
    _check(f"conv0_ln {shape} {'bias' if with_bias else 'no bias'}", out, c["ref"], dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=_name)
@pytest.mark.parametrize("shape", cr.INTERP_SHAPES, ids=str)
def test_interp_linear_is_one_rounding_of_the_float64_blend(shape, dtype):
    """rows past T_crop hold NaN and must not be read; bound 0.5 ulp_type(|ref|) + 2^-22 |ref| per element"""
    o = _ops()
    B, T_in, T_crop, T_out, C = shape
    x = torch.from_numpy(cr.interp_input(shape)).to(dtype)
    ref = torch.from_numpy(cr.interp_linear_ref(x.double().numpy(), T_out, T_crop))
    got = o.interp_linear(x.to(DEV), T_out, T_crop)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, T_out, C) and got.dtype == dtype
    got = got.cpu()
    assert bool(torch.isfinite(got).all())
    bound = 0.5 * torch.exp2(torch.floor(torch.log2(ref.abs())) - MANT[dtype]) + 2.0 ** -22 * ref.abs()
    err = (got.double() - ref).abs()
    print(f"interp_linear {shape} {_name(dtype)}: max err / bound {float((err / bound).max()):.3f}")
    assert not bool((err > bound).any()), (shape, dtype, int((err > bound).sum()), float((err / bound).max()))
    if dtype == torch.float32:
        assert np.array_equal(got.numpy(), onn.interp_linear_cl(x.numpy()[:, :T_crop], T_out))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=_name)
@pytest.mark.parametrize("shape", cr.GROUP_PAD_SHAPES, ids=str)
def test_group_pad_equals_plain_indexing(shape, dtype):
    """into a NaN-filled output: every element is written, pad rows and extra channels exactly zero"""
    from msmd_amd import _lib
    o = _ops()
    B, T, G, cg, cg_out, pad = shape
    g = torch.Generator(device="cpu").manual_seed(sum(shape))
    x = torch.randn(B, T, G * cg, generator=g).to(dtype)
    want = torch.from_numpy(cr.group_pad_ref(x.float().numpy(), G, pad, cg_out)).to(dtype)
    xd = x.to(DEV)
    y = torch.full((B, G, T + 2 * pad, cg_out), float("nan"), device=DEV, dtype=dtype)
    rc = _lib.load().msmd_group_pad(xd.data_ptr(), y.data_ptr(), B, T, G, cg, cg_out, pad, o._dt(xd), o._dt(y),
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(y.cpu(), want), (shape, dtype, int((y.cpu() != want).sum()))
    assert torch.equal(o.group_pad(xd, G, pad, cg_out=cg_out).cpu(), want)


@pytest.mark.parametrize("L,r,rep", cr.PAD_AUDIO_SHAPES)
def test_pad_audio_equals_np_pad(L, r, rep):
    o = _ops()
    x = (np.arange(2 * L, dtype=np.float32).reshape(2, L) + 0.25) * np.float32(1.5)
    got = o.pad_audio(_dev(x), r, rep)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), x[:, cr.pad_index(L, r, rep)])
