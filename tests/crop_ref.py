"""The face-crop operator of include/msmd_hip.h (msmd_face_crop) restated in numpy float64, written from its
text: a bilinear affine warp with a zero border in which every operation is rounded on its own, so the bytes are a pure
function of the inputs; and the normalisation in torch on the CPU, written as the reference writes it."""
import numpy as np
import torch


def invert(trans):
    """(F, 2, 3) forward maps -> inverse maps, by the 2 x 2 closed form in float64."""
    tr = np.asarray(trans, np.float64)
    a, b, c, d = tr[:, 0, 0], tr[:, 0, 1], tr[:, 1, 0], tr[:, 1, 1]
    det = a * d - b * c
    inv = np.empty_like(tr)
    inv[:, 0, 0], inv[:, 0, 1], inv[:, 1, 0], inv[:, 1, 1] = d / det, -b / det, -c / det, a / det
    inv[:, 0, 2] = -(inv[:, 0, 0] * tr[:, 0, 2] + inv[:, 0, 1] * tr[:, 1, 2])
    inv[:, 1, 2] = -(inv[:, 1, 0] * tr[:, 0, 2] + inv[:, 1, 1] * tr[:, 1, 2])
    return inv


def warp(frames, inverse, out_h, out_w, swap_rb=True):
    """frames (F, H, W, 3 | 4) uint8, inverse (F, 2, 3) float64 (output pixel -> source) -> (F, out_h, out_w, 3) uint8."""
    frames = np.asarray(frames)
    F, H, W = frames.shape[:3]
    out = np.zeros((F, out_h, out_w, 3), np.uint8)
    j = np.arange(out_w, dtype=np.float64)[None, :]
    i = np.arange(out_h, dtype=np.float64)[:, None]
    for f in range(F):
        a = np.asarray(inverse[f], np.float64)
        sx = ((a[0, 0] * j) + (a[0, 1] * i)) + a[0, 2]
        sy = ((a[1, 0] * j) + (a[1, 1] * i)) + a[1, 2]
        inside = (sx > -1.0) & (sx < W) & (sy > -1.0) & (sy < H)
        sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
        x0f, y0f = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0f, sy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        src = frames[f, :, :, :3].astype(np.float64)
        if swap_rb:
            src = src[:, :, ::-1]

        def p(y, x):
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            return np.where(ok[..., None], src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0)
        gx, gy = (1.0 - fx)[..., None], (1.0 - fy)[..., None]
        top = (p(y0, x0) * gx) + (p(y0, x0 + 1) * fx[..., None])
        bot = (p(y0 + 1, x0) * gx) + (p(y0 + 1, x0 + 1) * fx[..., None])
        v = (top * gy) + (bot * fy[..., None])
        u8 = np.minimum(255.0, np.floor(v + 0.5))
        out[f] = np.where(inside[..., None], u8, 0.0).astype(np.uint8)
    return out


def normalise(crop_u8, mean, std):
    """(F, S, S, 3) uint8 -> (F, 3, S, S) fp32: ToTensor (`.float().div(255)` on the channels-first image), then Normalize
    (`.sub_(mean).div_(std)` with fp32 mean / std of shape (3, 1, 1))."""
    x = torch.from_numpy(np.ascontiguousarray(crop_u8)).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(-1, 1, 1)
    return x.sub_(m).div_(s)
