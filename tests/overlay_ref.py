"""The overlay operator of include/msmd_hip.h restated in numpy from its text: per frame, per record in list
order, per pixel, per sample point.  No tiles, no culling, no chunks.  int64 wherever it is exact; the capsule's middle comparison
(q x d)^2 <= r^2 L is made on Python integers (object arrays) unless both sides provably fit int64.

`mutant` plants one wrong reading of the rule, for tests/test_overlay_cpu.py to show that a named case catches each:
  "lt"        `<` in place of `<=` in the disc, capsule and box comparisons
  "no_caps"   the capsule's end caps dropped (the middle band only, cut at s = 0 and s = L)
  "backwards" a frame's list walked from its end
  "no_round"  the blend's + 2040 dropped
  "wrap64"    the capsule's products wrapped to 64 bits
  "inner_lt"  the outline's inner box tested with `<`"""
import numpy as np

NONE, DISC, CAPSULE, BOX, GLYPH = range(5)
TILE_W, TILE_H, CHUNK = 64, 16, 256          # checked against the header's in tests/test_overlay_cpu.py
MAX_COORD, MAX_RADIUS = 1 << 20, 1 << 16
MUTANTS = ("lt", "no_caps", "backwards", "no_round", "wrap64", "inner_lt")


def colour_word(c):
    c = tuple(int(v) for v in c)
    r, g, b, a = c if len(c) == 4 else c + (255,)
    return r | g << 8 | b << 16 | a << 24


def record(kind, x0=0, y0=0, x1=0, y1=0, r=0, aux=0, colour=(255, 255, 255, 255)):
    """One row of prims; the colour word is stored as the int32 with the same bits."""
    w = colour_word(colour) if not isinstance(colour, (int, np.integer)) else int(colour)
    return np.array([kind, x0, y0, x1, y1, r, aux, w - (1 << 32) if w >= 1 << 31 else w], np.int64).astype(np.int32)


def sample_points(H, W, samples):
    """-> px, py (H, W, S) int64 in 1/16 px."""
    offs = np.array([8] if samples == 1 else [2, 6, 10, 14], np.int64)
    oy, ox = np.meshgrid(offs, offs, indexing="ij")
    px = 16 * np.arange(W, dtype=np.int64)[None, :, None] + ox.reshape(-1)[None, None, :]
    py = 16 * np.arange(H, dtype=np.int64)[:, None, None] + oy.reshape(-1)[None, None, :]
    return np.broadcast_to(px, (H, W, offs.size ** 2)), np.broadcast_to(py, (H, W, offs.size ** 2))


def draws(rec, n_glyphs):
    """Whether a record draws at all: the header's list."""
    kind, x0, y0, x1, y1, r, aux = (int(v) for v in rec[:7])
    if kind < DISC or kind > GLYPH:
        return False
    if abs(x0) > MAX_COORD or abs(y0) > MAX_COORD or not 0 <= r <= MAX_RADIUS or not 0 <= aux <= MAX_RADIUS:
        return False
    if kind == GLYPH:
        return 1 <= x1 <= MAX_RADIUS and 0 <= y1 < n_glyphs
    return abs(x1) <= MAX_COORD and abs(y1) <= MAX_COORD


def _le(a, b, mutant):
    return a < b if mutant == "lt" else a <= b


def inside(rec, px, py, font, mutant=None):
    """rec (8,) of a record that draws; px, py int64 arrays of sample points -> bool array."""
    kind, x0, y0, x1, y1, r, aux = (int(v) for v in rec[:7])
    qx, qy = px - x0, py - y0
    if kind == DISC:
        d2 = qx * qx + qy * qy
        return _le(aux * aux, d2, mutant) & _le(d2, r * r, mutant)
    if kind == CAPSULE:
        dx, dy, r2 = x1 - x0, y1 - y0, r * r
        L = dx * dx + dy * dy
        s = qx * dx + qy * dy
        ex, ey = px - x1, py - y1
        cap_a, cap_b = _le(qx * qx + qy * qy, r2, mutant), _le(ex * ex + ey * ey, r2, mutant)
        cr = qx * dy - qy * dx                                     # |cr| < 2^44: exact in int64
        if mutant == "wrap64":
            with np.errstate(over="ignore"):
                mid = _le(cr * cr, np.int64(r2) * np.int64(L), mutant)
        elif int(np.abs(cr).max(initial=0)) < 1 << 31 and r2 * L < 1 << 63:
            mid = _le(cr * cr, r2 * L, mutant)
        else:
            mid = _le(cr.astype(object) ** 2, r2 * L, mutant).astype(bool)
        if mutant == "no_caps":
            return (s > 0) & (s < L) & mid
        return np.where(s <= 0, cap_a, np.where(s >= L, cap_b, mid))
    if kind == BOX:
        ins = _le(x0, px, mutant) & _le(px, x1, mutant) & _le(y0, py, mutant) & _le(py, y1, mutant)
        if aux > 0:
            if mutant == "inner_lt":
                inner = (x0 + aux < px) & (px < x1 - aux) & (y0 + aux < py) & (py < y1 - aux)
            else:
                inner = (x0 + aux <= px) & (px <= x1 - aux) & (y0 + aux <= py) & (py <= y1 - aux)
            ins = ins & ~inner
        return ins
    u, v = qx // x1, qy // x1                                      # numpy's // is the floor division
    ok = (u >= 0) & (u < 8) & (v >= 0) & (v < 8)
    rows = np.asarray(font, np.uint8)[y1].astype(np.int64)[np.clip(v, 0, 7)]
    return ok & (((rows >> (7 - np.clip(u, 0, 7))) & 1) == 1)


def coverage(rec, H, W, samples, font, mutant=None):
    """-> (H, W) int64: the number of each pixel's sample points inside the record."""
    px, py = sample_points(H, W, samples)
    return inside(rec, px, py, font, mutant).sum(-1).astype(np.int64)


def blend(d, c, w, mutant=None):
    return (d * (4080 - w) + c * w + (0 if mutant == "no_round" else 2040)) // 4080


def clamp_offsets(prim_offsets, P):
    off = np.clip(np.asarray(prim_offsets, np.int64), 0, P)
    return [(int(b), int(max(b, e))) for b, e in zip(off[:-1], off[1:])]


def draw(frames, prims, prim_offsets, font=None, samples=16, mutant=None):
    """frames (N, H, W, C) uint8, C in {1, 3, 4} -> a new array with the records drawn.  The fourth channel is never touched."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] in (1, 3, 4) and samples in (1, 16)
    N, H, W, C = frames.shape
    prims = np.asarray(prims, np.int32).reshape(-1, 8)
    font = np.zeros((0, 8), np.uint8) if font is None else np.asarray(font, np.uint8)
    out = frames.copy()
    nc = 1 if C == 1 else 3
    for f, (b, e) in enumerate(clamp_offsets(prim_offsets, prims.shape[0])):
        img = out[f, :, :, :nc].astype(np.int64)
        order = range(e - 1, b - 1, -1) if mutant == "backwards" else range(b, e)
        for k in order:
            rec = prims[k]
            if not draws(rec, font.shape[0]):
                continue
            word = int(rec[7]) & 0xFFFFFFFF
            w = coverage(rec, H, W, samples, font, mutant) * (16 // samples) * (word >> 24)
            for c in range(nc):
                img[:, :, c] = blend(img[:, :, c], (word >> (8 * c)) & 255, w, mutant)
        out[f, :, :, :nc] = img.astype(np.uint8)
    return out
