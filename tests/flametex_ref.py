"""float64 numpy restatement of the FLAMETex albedo model (reference utils/flame.py:247-301; include/msmd_hip.h) and the error
bounds its tests use.  Nothing here imports the product."""
import functools

import numpy as np

U = 2.0 ** -24
SRC_HW, DST_HW = (512, 512), (256, 256)


def nearest_index(S, D):
    """Source index of every destination index 0 .. D - 1 under F.interpolate's nearest rule, all in fp32:
    min(int(floorf(d * scale)), S - 1) with scale = (float)S / (float)D."""
    scale = np.float32(S) / np.float32(D)
    d = np.arange(D, dtype=np.float32)
    return np.minimum(np.floor(d * scale).astype(np.int64), S - 1)


def rows(src_hw, dst_hw):
    """(3, Hd, Wd) int64: the basis row behind output element (c, y, x), ((sy(y) Ws + sx(x)) 3 + (2 - c))."""
    (Hs, Ws), (Hd, Wd) = src_hw, dst_hw
    pix = nearest_index(Hs, Hd)[:, None] * Ws + nearest_index(Ws, Wd)[None, :]
    return np.stack([pix * 3 + (2 - c) for c in range(3)])


def forward(mean, basis, code, src_hw=SRC_HW, dst_hw=DST_HW):
    """mean (R,), basis (R, n_tex), code (n_tex,) -> (value (3, Hd, Wd) float64, magnitude (3, Hd, Wd) float64 =
    |mean| + sum_k |basis_k code_k| per element)."""
    r = rows(src_hw, dst_hw)
    b = np.asarray(basis)[r].astype(np.float64)                       # (3, Hd, Wd, n_tex)
    c = np.asarray(code, np.float64)
    m = np.asarray(mean, np.float64)[r]
    return m + b @ c, np.abs(m) + np.abs(b) @ np.abs(c)


def forward_bound(magnitude, n_tex):
    """The dot-product bound (n_tex + 2) u magnitude: n_tex products and n_tex additions in any order, with or without fma."""
    return (n_tex + 2) * U * magnitude


def image_u8(planar):
    """(3, Hd, Wd) float32 -> (Hd, Wd, 3) uint8: floorf(fmaf(255, clamp(c, 0, 1), 0.5)) emulated exactly (the fused form rounds
    once, and 255 c + 0.5 is exact in float64), NaN -> 0."""
    c = np.asarray(planar, np.float32).astype(np.float64)
    c = np.where(np.isnan(c), 0.0, np.clip(c, 0.0, 1.0))
    return np.floor((255.0 * c + 0.5).astype(np.float32)).astype(np.uint8).transpose(1, 2, 0)


def gradient(basis, grad_out, src_hw=SRC_HW):
    """grad_out (n_copies, 3, Hd, Wd) -> (grad_code (n_tex,) float64, sum of |terms| (n_tex,) float64, N = 3 Hd Wd n_copies)."""
    g = np.asarray(grad_out, np.float64)
    r = rows(src_hw, g.shape[2:]).reshape(-1)
    b = np.asarray(basis)[r].astype(np.float64)                       # (3 Hd Wd, n_tex)
    gs = g.reshape(g.shape[0], -1)
    return b.T @ gs.sum(axis=0), np.abs(b).T @ np.abs(gs).sum(axis=0), g.size


def gamma(N):
    return N * U / (1.0 - N * U)


def ternary(name, shape):
    """grad_out in {-1, 0, 1} from the named synth key."""
    from msmd_amd import synth
    return (np.floor(synth.uniform01(name, int(np.prod(shape))) * np.float32(3.0)) - np.float32(1.0)).astype(np.float32).reshape(shape)


@functools.lru_cache(maxsize=None)
def asset(tex_type, n_tex, quantised=False):
    from msmd_amd import synth
    return synth.flametex_asset(tex_type, n_tex, quantised)


def buffers(a, tex_type, n_tex):
    """The module's (mean (R,), basis (R, n_tex)) fp32 from an asset, by the constructor's rules."""
    if tex_type == "BFM":
        return (np.asarray(a["MU"], np.float32).reshape(-1),
                np.ascontiguousarray(np.asarray(a["PC"], np.float32).reshape(-1, a["PC"].shape[-1])[:, :n_tex]))
    pc = a["tex_dir"].reshape(-1, a["tex_dir"].shape[-1])[:, :n_tex]
    return (a["mean"].reshape(-1) / 255.).astype(np.float32), np.ascontiguousarray((pc / 255.).astype(np.float32))
