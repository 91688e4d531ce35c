"""The resize operator restated in numpy: Pillow's `Image.resize` for 8-bit images, written from the rule
alone and independently of `msmd_amd.ops.resize_tables`.  Tables in plain Python floats, int64 accumulation, the horizontal pass
rounded to uint8, then the vertical pass.  `MUTANTS` names deliberate departures from the rule: the CPU test shows that each
one changes bytes on its inputs, so the inputs can tell the rule from its neighbours."""
import functools
import math

import numpy as np

P = 22
FILTERS = ("box", "bilinear", "bicubic", "lanczos")
MUTANTS = ("float32_accumulation", "no_rounding_between_passes", "vertical_first", "round_xmin", "not_normalised", "p16")


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _filter(name):
    if name == "box":
        return (lambda x: 1.0 if -0.5 < x <= 0.5 else 0.0), 0.5
    if name == "bilinear":
        return (lambda x: 1.0 - abs(x) if abs(x) < 1.0 else 0.0), 1.0
    if name == "bicubic":
        def keys(x, a=-0.5):
            x = abs(x)
            if x < 1.0:
                return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
            if x < 2.0:
                return (((x - 5) * x + 8) * x - 4) * a
            return 0.0
        return keys, 2.0
    if name == "lanczos":
        return (lambda x: _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0), 3.0
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def weights(n_in, n_out, filter, in0=None, in1=None, mutant=None):
    """-> (bounds [(xmin, taps)], w [[float]], ksize): the float64 weights of one axis, steps 1 and 2 of the rule."""
    f, support = _filter(filter)
    in0 = 0.0 if in0 is None else float(in0)
    in1 = float(n_in) if in1 is None else float(in1)
    scale = (in1 - in0) / n_out
    fs = max(scale, 1.0)
    sup = support * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    ss = 1.0 / fs
    bounds, rows = [], []
    for xx in range(n_out):
        center = in0 + (xx + 0.5) * scale
        lo, hi = center - sup + 0.5, center + sup + 0.5
        xmin = max(0, int(round(lo)) if mutant == "round_xmin" else int(lo))
        xmax = min(n_in, int(hi)) - xmin
        w = [f((i + xmin - center + 0.5) * ss) for i in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0 and mutant != "not_normalised":
            w = [v / ww for v in w]
        bounds.append((xmin, xmax))
        rows.append(w)
    return bounds, rows, ksize


def tables(n_in, n_out, filter, in0=None, in1=None, mutant=None):
    """-> (bounds (n_out, 2) int32, coef (n_out, ksize) int32): the fixed-point tables, step 3 of the rule."""
    bounds, rows, ksize = weights(n_in, n_out, filter, in0, in1, mutant)
    one = float(1 << (16 if mutant == "p16" else P))
    coef = np.zeros((n_out, ksize), np.int32)
    for xx, w in enumerate(rows):
        coef[xx, :len(w)] = [int(0.5 + v * one) if v >= 0 else int(-0.5 + v * one) for v in w]
    return np.asarray(bounds, np.int32).reshape(n_out, 2), coef


def accumulator_peak(coef):
    """The largest value the accumulator of step 4 can reach in magnitude under a table: max sum |k| * 255 + 2^21."""
    return int(np.abs(coef.astype(np.int64)).sum(1).max()) * 255 + (1 << (P - 1))


def clamp_tables(bounds, coef, n_in):
    """The clamp msmd_resize_u8 applies to what it reads from a table: first into [0, n_in - 1], taps into
    [0, min(ksize, n_in - first)]."""
    b = np.asarray(bounds).astype(np.int64)
    first = np.clip(b[..., 0], 0, n_in - 1)
    taps = np.clip(b[..., 1], 0, np.minimum(coef.shape[-1], n_in - first))
    return np.stack([first, taps], -1).astype(np.int32), coef


def pass_axis0(a, bounds, coef, bits=P, raw=False):
    """One pass along axis 0 of an integer array a (n_in, ...) -> (n_out, ...): step 4 with an int64 accumulator, checked to
    stay inside int32.  raw: the accumulator before the shift."""
    a = a.astype(np.int64)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.int64)
    for o, (first, taps) in enumerate(bounds.tolist()):
        k = coef[o, :taps].astype(np.int64)
        out[o] = np.tensordot(k, a[first:first + taps], axes=(0, 0)) + (1 << (bits - 1))
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out if raw else np.clip(out >> bits, 0, 255).astype(np.uint8)


def resize_with_tables(img, xt, yt):
    """img (H, W, C) uint8 through the horizontal tables xt = (bounds, coef), rounded, then the vertical tables yt; None skips
    a pass."""
    mid = img if xt is None else pass_axis0(img.transpose(1, 0, 2), *xt).transpose(1, 0, 2)
    return mid if yt is None else pass_axis0(mid, *yt)


def _axis(n_in, n_out, filter, in0, in1, mutant=None):
    if n_in == n_out and in0 == 0.0 and in1 == float(n_in):
        return None                                    # the pass is skipped
    return tables(n_in, n_out, filter, in0, in1, mutant)


def float32_box(box, W, H):
    """A box as Pillow's C code stores it, rounded to float32, or the whole image."""
    if box is None:
        return 0.0, 0.0, float(W), float(H)
    return tuple(float(np.float32(v)) for v in box)


def resize(img, size, filter, box=None, mutant=None):
    """img (H, W, C) or (H, W) uint8 -> (size[1], size[0], C) uint8; size = (width, height) as Pillow orders it."""
    flat = img.ndim == 2
    img = img[:, :, None] if flat else img
    H, W, _ = img.shape
    Wd, Hd = size
    x0, y0, x1, y1 = float32_box(box, W, H)
    tab_mutant = mutant if mutant in ("round_xmin", "not_normalised", "p16") else None
    bits = 16 if mutant == "p16" else P
    xt, yt = _axis(W, Wd, filter, x0, x1, tab_mutant), _axis(H, Hd, filter, y0, y1, tab_mutant)
    if mutant is None:
        out = resize_with_tables(img, xt, yt)
    elif mutant == "vertical_first":
        mid = img if yt is None else pass_axis0(img, *yt)
        out = mid if xt is None else pass_axis0(mid.transpose(1, 0, 2), *xt).transpose(1, 0, 2)
    elif mutant == "no_rounding_between_passes":
        mid = img.astype(np.float64) if xt is None else \
            (pass_axis0(img.transpose(1, 0, 2), *xt, raw=True).transpose(1, 0, 2) - (1 << (P - 1))) / float(1 << P)
        if yt is None:
            out = np.clip(np.floor(mid + 0.5), 0, 255).astype(np.uint8)
        else:
            acc = np.stack([np.tensordot(yt[1][o, :t].astype(np.float64), mid[f:f + t], axes=(0, 0)) for o, (f, t) in enumerate(yt[0].tolist())])
            out = np.clip(np.floor(acc / float(1 << P) + 0.5), 0, 255).astype(np.uint8)
    elif mutant == "float32_accumulation":
        def f32_pass(a, bounds, coef):
            rows = []
            for o, (f, t) in enumerate(bounds.tolist()):
                acc = np.full(a.shape[1:], np.float32(1 << (P - 1)), np.float32)
                for i in range(t):
                    acc = acc + a[f + i].astype(np.float32) * np.float32(coef[o, i])
                rows.append(acc)
            return np.clip(np.floor(np.stack(rows).astype(np.float64) / float(1 << P)), 0, 255).astype(np.uint8)
        mid = img if xt is None else f32_pass(img.transpose(1, 0, 2), *xt).transpose(1, 0, 2)
        out = mid if yt is None else f32_pass(mid, *yt)
    else:
        def shifted(a, t):
            return pass_axis0(a, t[0], t[1], bits=bits)
        mid = img if xt is None else shifted(img.transpose(1, 0, 2), xt).transpose(1, 0, 2)
        out = mid if yt is None else shifted(mid, yt)
    return out[:, :, 0] if flat else out


def resize_frames(frames, size, filter, boxes=None):
    """frames (N, H, W, C) uint8, boxes None, one box or one per frame -> (N, size[1], size[0], C) uint8."""
    N = frames.shape[0]
    if boxes is None or np.asarray(boxes).ndim == 1:
        boxes = [boxes] * N
    return np.stack([resize(frames[n], size, filter, None if boxes[n] is None else tuple(boxes[n])) for n in range(N)])


def frames_at(n_out, fps_out, n_src, fps_src):
    """The source frame nearest in time to every output frame, in exact rational arithmetic: frame k of the output is shown at
    k / fps_out, which is source frame k fps_src / fps_out; nearest = floor(that + 1 / 2), clamped to the last frame."""
    from fractions import Fraction
    ratio = Fraction(fps_src) / Fraction(fps_out)
    return [min(n_src - 1, math.floor(k * ratio + Fraction(1, 2))) for k in range(n_out)]


def content(kind, shape, tag=""):
    """Test images (H, W, C) or batches of them: "zeros", "full" (all 255), "checker" (0 / 255 per pixel) or "random" bytes
    from a seed derived from the tag and the shape."""
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "full":
        return np.full(shape, 255, np.uint8)
    if kind == "checker":
        idx = np.indices(shape[:-1]).sum(0) & 1
        return np.broadcast_to((idx * 255).astype(np.uint8)[..., None], shape).copy()
    seed = sum((i + 1) * b for i, b in enumerate(f"{tag}/{shape}".encode())) % (2 ** 32)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
