"""Float64 numpy references of the audio front end (csrc/audio.hip) and the case set that test_conv0_cpu.py proves on the
CPU and test_conv0_gpu.py runs on the GPU: pad_audio, conv0 + GroupNorm + GELU, conv0 + LayerNorm + GELU, interp_linear,
group_pad.  Nothing here is a port of the kernels: the pad map comes from np.pad, the conv from a strided window product."""
import math

import numpy as np

try:
    from scipy.special import erf as _erf
except ImportError:                                      # pragma: no cover
    import torch

    def _erf(x):
        return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()

KERNEL, STRIDE = 10, 5


def frames(L, r, rep):
    """T0 of a clip of L samples under pad_audio(r, rep)"""
    return (L + 4 * r + 2 * rep - KERNEL) // STRIDE + 1


def pad_index(L, r, rep):
    """Gather map of reflect(r) o reflect(r) o replicate(rep) on a clip of L samples: out[j] = clip[pad_index[j]]"""
    idx = np.arange(L, dtype=np.int64)
    for _ in range(2):
        if r > 0:
            idx = np.pad(idx, r, mode="reflect")
    if rep > 0:
        idx = np.pad(idx, rep, mode="edge")
    return idx


def gelu64(z):
    return 0.5 * z * (1.0 + _erf(z / math.sqrt(2.0)))


def conv0_ref(audio, w0, r, rep):
    """(B, L) clips, (C, 10) taps -> (B, T0, C) float64 stride-5 conv of the padded clips"""
    a = np.asarray(audio, dtype=np.float64)
    x = a[:, pad_index(a.shape[1], r, rep)]
    win = np.lib.stride_tricks.sliding_window_view(x, KERNEL, axis=1)[:, ::STRIDE]       # (B, T0, 10)
    assert win.shape[1] == frames(a.shape[1], r, rep)
    return win @ np.asarray(w0, dtype=np.float64).T


def conv0_gn_gelu_ref(audio, w0, gamma, beta, r, rep, eps=1e-5):
    """GELU(GroupNorm(C groups of one channel)(conv0(pad_audio(audio)))): returns out (B, T0, C), (mean, rstd) each (B, C),
    and the pre-GELU values z (B, T0, C), all float64"""
    y = conv0_ref(audio, w0, r, rep)
    mean = y.mean(axis=1)
    rstd = 1.0 / np.sqrt(y.var(axis=1) + eps)                                            # biased variance over frames
    z = (y - mean[:, None]) * rstd[:, None] * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return gelu64(z), (mean, rstd), z


def conv0_ln_gelu_ref(audio, w0, bias, gamma, beta, r, rep, eps=1e-5):
    """GELU(LayerNorm over channels(conv0(pad_audio(audio)) + bias)): returns out (B, T0, C) and the pre-GELU values"""
    y = conv0_ref(audio, w0, r, rep)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    mean = y.mean(axis=2, keepdims=True)
    rstd = 1.0 / np.sqrt(y.var(axis=2, keepdims=True) + eps)
    z = (y - mean) * rstd * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return gelu64(z), z


def interp_table(in_len, out_len):
    """(i0, i1, w1) of F.interpolate(mode='linear', align_corners=False): src = scale (dst + 0.5) - 0.5 in fp32 with ONE
    rounding (ATen's fused form; the fp32 x fp32 product is exact in float64), clamped at 0"""
    scale = np.float32(in_len) / np.float32(out_len)
    dst = np.arange(out_len, dtype=np.float32) + np.float32(0.5)
    src = np.maximum((np.float64(scale) * dst.astype(np.float64) - 0.5).astype(np.float32), np.float32(0.0))
    i0 = np.minimum(np.floor(src).astype(np.int64), in_len - 1)
    i1 = np.minimum(i0 + 1, in_len - 1)
    return i0, i1, src - i0.astype(np.float32)


def interp_linear_ref(x, t_out, t_crop=None):
    """(B, T_in, C) -> (B, t_out, C): linear resampling of rows [0, t_crop), blended in float64"""
    x = np.asarray(x, dtype=np.float64)
    t_crop = x.shape[1] if t_crop is None else t_crop
    i0, i1, w1 = interp_table(t_crop, t_out)
    w1 = w1.astype(np.float64)[None, :, None]
    return (1.0 - w1) * x[:, i0] + w1 * x[:, i1]


def group_pad_ref(x, groups, pad, cg_out=None):
    """(B, T, G * cg) -> (B, G, T + 2 pad, cg_out): group-major, zero rows either side, zero channels past cg"""
    B, T, C = x.shape
    cg = C // groups
    cg_out = cg if cg_out is None else cg_out
    y = np.zeros((B, groups, T + 2 * pad, cg_out), x.dtype)
    y[:, :, pad:pad + T, :cg] = x.reshape(B, T, groups, cg).transpose(0, 2, 1, 3)
    return y


# ------------------------------------------------------------------------------------------------- the case set
def plan_case_len():
    """A clip length <= 6500 whose pad_audio_plan has r > 0 and rep > 0 (test_conv0_cpu.py checks the choice)"""
    return 6402


# (B, L, r, rep, C) of the GroupNorm form; the plan case is appended by gn_shapes()
GN_SHAPES = [(1, 40, 0, 0, 32), (3, 330, 0, 0, 512), (2, 650, 0, 0, 512), (2, 1443, 0, 0, 40), (1, 650, 0, 0, 1024),
             (1, 330, 0, 0, 1056), (2, 600, 40, 15, 512), (1, 40, 39, 0, 64)]
LN_SHAPES = [(1, 40, 0, 0), (3, 330, 0, 0), (2, 600, 40, 15)]          # (B, L, r, rep), C = 512
QUIET_SHAPE = (1, 650, 0, 0, 64)
STATS_CASES = ["znorm", "dc", "late_dc", "constant", "tiny"]           # C = 32, B = 1
CLIP_SCALE_OFFSET = [(1.0, 0.0), (0.2, 0.3), (3.0, 0.0)]               # clip b of a batch: sigma, DC


def gn_shapes():
    from oracle import audio_encoder as oa
    L = plan_case_len()
    return GN_SHAPES + [(2, L, *oa.pad_audio_plan(L), 512)]


def _rng(*key):
    return np.random.default_rng([20240, *key])


def clips(B, L, seed):
    g = _rng(1, B, L, seed)
    a = g.standard_normal((B, L))
    for b in range(B):
        s, dc = CLIP_SCALE_OFFSET[b % 3]
        a[b] = a[b] * s + dc
    return a.astype(np.float32)


def params(C, seed, bias=False):
    """w0 (C, 10), gamma (C,) with magnitudes in [0.5, 2.5] and both signs, beta (C,), all distinct per channel"""
    g = _rng(2, C, seed)
    w0 = (g.standard_normal((C, KERNEL)) / math.sqrt(KERNEL)).astype(np.float32)
    gamma = (g.uniform(0.5, 2.5, C) * np.where(g.random(C) < 0.25, -1.0, 1.0)).astype(np.float32)
    beta = g.uniform(-0.5, 0.5, C).astype(np.float32)
    if bias:
        return w0, gamma, beta, g.uniform(-0.3, 0.3, C).astype(np.float32)
    return w0, gamma, beta


_cache = {}


def gn_case(shape):
    """inputs and float64 reference of one GroupNorm-form shape, computed once and left unchanged"""
    if shape not in _cache:
        B, L, r, rep, C = shape
        audio = clips(B, L, r + rep)
        w0, gamma, beta = params(C, L)
        out, stats, z = conv0_gn_gelu_ref(audio, w0, gamma, beta, r, rep)
        _cache[shape] = dict(audio=audio, w0=w0, gamma=gamma, beta=beta, ref=out, stats=stats, z=z)
    return _cache[shape]


def ln_case(shape, with_bias):
    key = ("ln", shape, with_bias)
    if key not in _cache:
        B, L, r, rep = shape
        audio = clips(B, L, 7 + r + rep)
        w0, gamma, beta, bias = params(512, 3 * L, bias=True)
        bias = bias if with_bias else None
        out, z = conv0_ln_gelu_ref(audio, w0, bias, gamma, beta, r, rep)
        _cache[key] = dict(audio=audio, w0=w0, bias=bias, gamma=gamma, beta=beta, ref=out, z=z)
    return _cache[key]


def quiet_case():
    """a silent 16-bit recording: one LSB of noise (sigma = 3e-5); beta = 0 so that the shift does not set the row maximum"""
    if "quiet" not in _cache:
        B, L, r, rep, C = QUIET_SHAPE
        audio = (3e-5 * _rng(3).standard_normal((B, L))).astype(np.float32)
        w0, gamma, _ = params(C, 11)
        beta = np.zeros(C, np.float32)
        out, stats, z = conv0_gn_gelu_ref(audio, w0, gamma, beta, r, rep)
        _cache["quiet"] = dict(audio=audio, w0=w0, gamma=gamma, beta=beta, ref=out, stats=stats, z=z)
    return _cache["quiet"]


def stats_case(name):
    """the statistics cases: C = 32, one clip, r = rep = 0"""
    key = ("stats", name)
    if name == "tiny":                            # the first shape's clip: T0 = 7 frames, 9 of the 16 moment splits empty
        return gn_case(GN_SHAPES[0])
    if key not in _cache:
        L = 6405
        g = _rng(4, STATS_CASES.index(name))
        n = g.standard_normal(L)
        if name == "znorm":                       # the loader's clip: zero mean, unit variance
            a = (n - n.mean()) / n.std()
        elif name == "dc":
            a = 0.5 + 0.05 * n
        elif name == "late_dc":
            a = 0.5 + 0.01 * n
            a[:400] = 0.0
        else:
            # rstd = 1 / sqrt(eps) = 316 here, so the fp32 rounding of the stored mean alone costs 316 |gamma|_max 2^-25 |mean|:
            # within the statistics' 1e-5 only for |mean| = 0.05 |sum_k w_k| < 0.25
            a = np.full(L, 0.05)
        audio = a.astype(np.float32)[None]
        w0, gamma, beta = params(32, 5)
        out, stats, z = conv0_gn_gelu_ref(audio, w0, gamma, beta, 0, 0)
        _cache[key] = dict(audio=audio, w0=w0, gamma=gamma, beta=beta, ref=out, stats=stats, z=z)
    return _cache[key]


def stats_error(case, mean, rstd):
    """|d mean| rstd_ref |gamma|_max + z_max |d rstd| / rstd_ref per (clip, channel): the share of a normalised value
    that wrong statistics move, z_max = that clip / channel's largest normalised reference magnitude"""
    mref, rref = case["stats"]
    y = conv0_ref(case["audio"], case["w0"], 0, 0)
    zmax = np.abs((y - mref[:, None]) * rref[:, None]).max(axis=1)
    gmax = float(np.abs(case["gamma"]).max())
    return np.abs(mean - mref) * rref * gmax + zmax * np.abs(rstd - rref) / rref


# (B, T_in, T_crop, T_out, C)
INTERP_SHAPES = [(2, 50, 50, 25, 768), (1, 50, 41, 60, 1000), (1, 9, 1, 4, 4), (2, 400, 333, 200, 8)]
# (B, T, G, cg, cg_out, pad)
GROUP_PAD_SHAPES = [(2, 5, 16, 48, 48, 64), (1, 300, 16, 48, 64, 64), (2, 7, 1, 8, 8, 0), (1, 3, 2, 4, 12, 1)]
PAD_AUDIO_SHAPES = [(40, 39, 0), (7, 3, 11), (1, 0, 5)]                # (L, r, rep)


def interp_input(shape):
    """fp32 rows whose neighbours along time have one sign per channel and magnitudes in [0.25, 4]: the bound of the interp
    test is relative to |reference|, which describes an fp32 blend only where the two products do not cancel.  Rows past
    T_crop are NaN: the kernel must not read them."""
    B, T_in, T_crop, T_out, C = shape
    g = _rng(5, *shape)
    x = np.exp2(g.uniform(-2.0, 2.0, (B, T_in, C))) * np.where(g.random(C) < 0.5, -1.0, 1.0)
    x[:, T_crop:] = np.nan
    return x.astype(np.float32)
