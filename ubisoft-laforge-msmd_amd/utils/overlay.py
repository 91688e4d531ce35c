"""Checking videos of the dataset preparation: boxes, landmarks, head-pose arrows and text drawn onto frames that are already on the
device (csrc/overlay.hip through ops.draw_overlay).

`Overlay(n_frames)` collects vectorised batches of primitives; `build` turns them into the (prims, prim_offsets) pair of the
operator and `draw` runs it.  Coordinates follow cv2's convention: integer (x, y) is the CENTRE of pixel (x, y); the operator's
fixed-point value is floor((x + 0.5) * 16 + 0.5) in float64 (1/16 pixel).  A point with a NaN coordinate, which is how a tracker
marks a missing landmark, is left out, and so is one beyond the operator's coordinate limit.  A colour is 3 or 4 bytes in the
frames' own channel order; alpha defaults to 255.

`box_overlay`, `landmark_overlay` and `head_pose_overlay` mirror the videos the reference writes after its Steps 1, 3 and 2.  The
operator has its own rasteriser and its own font: the pictures say the same thing as cv2's, pixel for pixel they differ.

Command line:  python -m msmd_amd.utils.overlay --frames clip.avi|clip.npy --out OUT.avi [--boxes step1.pickle]
                   [--landmarks lm.npy] [--head_rot rot.pickle] [--samples 1|16] [--fps F] [--audio WAV] [--quality Q]"""
from __future__ import annotations

import pickle as pkl

import numpy as np

_GLYPHS = (                          # ASCII 32 .. 126, a 5 x 7 face: seven rows of five font pixels, top row first
    "..... ..... ..... ..... ..... ..... .....",      # space
    "..#.. ..#.. ..#.. ..#.. ..#.. ..... ..#..",      # !
    ".#.#. .#.#. .#.#. ..... ..... ..... .....",      # "
    ".#.#. .#.#. ##### .#.#. ##### .#.#. .#.#.",      # #
    "..#.. .#### #.#.. .###. ..#.# ####. ..#..",      # $
    "##... ##..# ...#. ..#.. .#... #..## ...##",      # %
    ".##.. #..#. #.#.. .#... #.#.# #..#. .##.#",      # &
    "..#.. ..#.. .#... ..... ..... ..... .....",      # '
    "...#. ..#.. .#... .#... .#... ..#.. ...#.",      # (
    ".#... ..#.. ...#. ...#. ...#. ..#.. .#...",      # )
    "..... ..#.. #.#.# .###. #.#.# ..#.. .....",      # *
    "..... ..#.. ..#.. ##### ..#.. ..#.. .....",      # +
    "..... ..... ..... ..... .##.. ..#.. .#...",      # ,
    "..... ..... ..... ##### ..... ..... .....",      # -
    "..... ..... ..... ..... ..... .##.. .##..",      # .
    "..... ....# ...#. ..#.. .#... #.... .....",      # /
    ".###. #...# #..## #.#.# ##..# #...# .###.",      # 0
    "..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.",      # 1
    ".###. #...# ....# ...#. ..#.. .#... #####",      # 2
    "##### ...#. ..#.. ...#. ....# #...# .###.",      # 3
    "...#. ..##. .#.#. #..#. ##### ...#. ...#.",      # 4
    "##### #.... ####. ....# ....# #...# .###.",      # 5
    "..##. .#... #.... ####. #...# #...# .###.",      # 6
    "##### ....# ...#. ..#.. .#... .#... .#...",      # 7
    ".###. #...# #...# .###. #...# #...# .###.",      # 8
    ".###. #...# #...# .#### ....# ...#. .##..",      # 9
    "..... .##.. .##.. ..... .##.. .##.. .....",      # :
    "..... .##.. .##.. ..... .##.. ..#.. .#...",      # ;
    "...#. ..#.. .#... #.... .#... ..#.. ...#.",      # <
    "..... ..... ##### ..... ##### ..... .....",      # =
    ".#... ..#.. ...#. ....# ...#. ..#.. .#...",      # >
    ".###. #...# ....# ...#. ..#.. ..... ..#..",      # ?
    ".###. #...# #.### #.#.# #.### #.... .####",      # @
    ".###. #...# #...# #...# ##### #...# #...#",      # A
    "####. #...# #...# ####. #...# #...# ####.",      # B
    ".###. #...# #.... #.... #.... #...# .###.",      # C
    "###.. #..#. #...# #...# #...# #..#. ###..",      # D
    "##### #.... #.... ####. #.... #.... #####",      # E
    "##### #.... #.... ####. #.... #.... #....",      # F
    ".###. #...# #.... #.### #...# #...# .####",      # G
    "#...# #...# #...# ##### #...# #...# #...#",      # H
    ".###. ..#.. ..#.. ..#.. ..#.. ..#.. .###.",      # I
    "..### ...#. ...#. ...#. ...#. #..#. .##..",      # J
    "#...# #..#. #.#.. ##... #.#.. #..#. #...#",      # K
    "#.... #.... #.... #.... #.... #.... #####",      # L
    "#...# ##.## #.#.# #.#.# #...# #...# #...#",      # M
    "#...# #...# ##..# #.#.# #..## #...# #...#",      # N
    ".###. #...# #...# #...# #...# #...# .###.",      # O
    "####. #...# #...# ####. #.... #.... #....",      # P
    ".###. #...# #...# #...# #.#.# #..#. .##.#",      # Q
    "####. #...# #...# ####. #.#.. #..#. #...#",      # R
    ".#### #.... #.... .###. ....# ....# ####.",      # S
    "##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",      # T
    "#...# #...# #...# #...# #...# #...# .###.",      # U
    "#...# #...# #...# #...# #...# .#.#. ..#..",      # V
    "#...# #...# #...# #.#.# #.#.# #.#.# .#.#.",      # W
    "#...# #...# .#.#. ..#.. .#.#. #...# #...#",      # X
    "#...# #...# #...# .#.#. ..#.. ..#.. ..#..",      # Y
    "##### ....# ...#. ..#.. .#... #.... #####",      # Z
    ".###. .#... .#... .#... .#... .#... .###.",      # [
    "..... #.... .#... ..#.. ...#. ....# .....",      # backslash
    ".###. ...#. ...#. ...#. ...#. ...#. .###.",      # ]
    "..#.. .#.#. #...# ..... ..... ..... .....",      # ^
    "..... ..... ..... ..... ..... ..... #####",      # _
    ".#... ..#.. ...#. ..... ..... ..... .....",      # `
    "..... ..... .###. ....# .#### #...# .####",      # a
    "#.... #.... #.##. ##..# #...# #...# ####.",      # b
    "..... ..... .###. #.... #.... #...# .###.",      # c
    "....# ....# .##.# #..## #...# #...# .####",      # d
    "..... ..... .###. #...# ##### #.... .###.",      # e
    "..##. .#..# .#... ###.. .#... .#... .#...",      # f
    "..... .#### #...# #...# .#### ....# .###.",      # g
    "#.... #.... #.##. ##..# #...# #...# #...#",      # h
    "..#.. ..... .##.. ..#.. ..#.. ..#.. .###.",      # i
    "...#. ..... ..##. ...#. ...#. #..#. .##..",      # j
    "#.... #.... #..#. #.#.. ##... #.#.. #..#.",      # k
    ".##.. ..#.. ..#.. ..#.. ..#.. ..#.. .###.",      # l
    "..... ..... ##.#. #.#.# #.#.# #...# #...#",      # m
    "..... ..... #.##. ##..# #...# #...# #...#",      # n
    "..... ..... .###. #...# #...# #...# .###.",      # o
    "..... ####. #...# #...# ####. #.... #....",      # p
    "..... .#### #...# #...# .#### ....# ....#",      # q
    "..... ..... #.##. ##..# #.... #.... #....",      # r
    "..... ..... .###. #.... .###. ....# ####.",      # s
    ".#... .#... ###.. .#... .#... .#..# ..##.",      # t
    "..... ..... #...# #...# #...# #..## .##.#",      # u
    "..... ..... #...# #...# #...# .#.#. ..#..",      # v
    "..... ..... #...# #...# #.#.# #.#.# .#.#.",      # w
    "..... ..... #...# .#.#. ..#.. .#.#. #...#",      # x
    "..... #...# #...# #...# .#### ....# .###.",      # y
    "..... ..... ##### ...#. ..#.. .#... #####",      # z
    "...#. ..#.. ..#.. .#... ..#.. ..#.. ...#.",      # {
    "..#.. ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",      # |
    ".#... ..#.. ..#.. ...#. ..#.. ..#.. .#...",      # }
    "..... ..... .#... #.#.# ...#. ..... .....",      # ~
)


def _font_table():
    table = np.zeros((len(_GLYPHS), 8), np.uint8)
    for g, rows in enumerate(_GLYPHS):
        for v, row in enumerate(rows.split()):
            table[g, v] = sum(128 >> u for u, ch in enumerate(row) if ch == "#")
    table.setflags(write=False)
    return table


FONT = _font_table()      # (95, 8) uint8: row v of a glyph is one byte, bit 7 - u set = font pixel (u, v) is ink; row 7 is empty
FONT_FIRST, FONT_ADVANCE, FONT_ROWS = 32, 6, 7
KIND_DISC, KIND_CAPSULE, KIND_BOX, KIND_GLYPH = 1, 2, 3, 4       # ops.OVERLAY_*; typed here so that the builder needs no library
MAX_COORD, MAX_RADIUS = 1 << 20, 1 << 16


def fixed(x):
    """cv2's pixel coordinate (integer = pixel centre) -> the operator's 1/16 pixel, float64: floor((x + 0.5) * 16 + 0.5); NaN stays."""
    return np.floor((np.asarray(x, np.float64) + 0.5) * 16.0 + 0.5)


def colour_words(colour):
    """(..., 3 | 4) bytes -> (...) int64 words R | G << 8 | B << 16 | A << 24 (ops._color_table's packing), alpha 255 by default."""
    c = np.asarray(colour)
    if c.ndim < 1 or c.shape[-1] not in (3, 4) or not np.issubdtype(c.dtype, np.integer) or (c < 0).any() or (c > 255).any():
        raise ValueError(f"a colour is 3 or 4 bytes, got {colour!r}")
    c = c.astype(np.int64)
    a = c[..., 3] if c.shape[-1] == 4 else np.full(c.shape[:-1], 255, np.int64)
    return c[..., 0] | c[..., 1] << 8 | c[..., 2] << 16 | a << 24


def ypr_to_matrix(ypr):
    """(F, 3) yaw / pitch / roll in degrees -> (F, 3, 3) float64 on the host: R = Ry(yaw) Rx(pitch) Rz(roll), the inverse of the
    intrinsic 'YXZ' Euler rule by which the head-pose stage makes its angles."""
    a = np.radians(np.asarray(ypr, np.float64).reshape(-1, 3))
    cy, sy, cx, sx, cz, sz = np.cos(a[:, 0]), np.sin(a[:, 0]), np.cos(a[:, 1]), np.sin(a[:, 1]), np.cos(a[:, 2]), np.sin(a[:, 2])
    R = np.empty((a.shape[0], 3, 3), np.float64)
    R[:, 0, 0] = cy * cz + sy * sx * sz
    R[:, 0, 1] = -cy * sz + sy * sx * cz
    R[:, 0, 2] = sy * cx
    R[:, 1, 0] = cx * sz
    R[:, 1, 1] = cx * cz
    R[:, 1, 2] = -sx
    R[:, 2, 0] = -sy * cz + cy * sx * sz
    R[:, 2, 1] = sy * sz + cy * sx * cz
    R[:, 2, 2] = cy * cx
    return R


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


class Overlay:
    """Primitives for `n_frames` frames.  Points come as (n_frames, K, 2) or (n_frames, 2), one set per frame, or, with
    `frames` (M,) naming each point's frame, as (M, 2).  Sizes (radius, width, ...) are in pixels, one number or one per point."""

    def __init__(self, n_frames):
        self.n_frames = int(n_frames)
        if self.n_frames < 0:
            raise ValueError(f"n_frames = {n_frames} is negative")
        self._frames, self._records = [], []

    # ---- the batches
    def _points(self, xy, frames):
        """-> (points (M, 2) float64, frame index (M,) int64, the leading shape the per-point arguments broadcast against)."""
        p = _host(xy).astype(np.float64)
        if frames is None:
            if p.ndim == 2:
                p = p[:, None, :]
            if p.ndim != 3 or p.shape[0] != self.n_frames or p.shape[2] != 2:
                raise ValueError(f"points must be ({self.n_frames}, K, 2) or ({self.n_frames}, 2), got {p.shape}")
            f = np.broadcast_to(np.arange(self.n_frames, dtype=np.int64)[:, None], p.shape[:2])
            return p.reshape(-1, 2), f.reshape(-1), p.shape[:2]
        f = _host(frames).astype(np.int64).reshape(-1)
        if p.shape != (f.size, 2):
            raise ValueError(f"with frames of {f.size} entries points must be ({f.size}, 2), got {p.shape}")
        if f.size and (f.min() < 0 or f.max() >= self.n_frames):
            raise ValueError(f"frames holds an index outside [0, {self.n_frames})")
        return p, f, (f.size,)

    @staticmethod
    def _per_point(v, lead, name):
        try:
            return np.broadcast_to(np.asarray(v, np.float64), lead).reshape(-1)
        except ValueError:
            raise ValueError(f"{name} of shape {np.shape(v)} does not broadcast against the points {lead}") from None

    def _add(self, f, kind, x0, y0, x1, y1, r, aux, colour, lead, coords=4):
        """One batch: float64 columns -> int32 records, the rows with a NaN or with a value beyond the operator's limits left out."""
        cols = np.stack([np.broadcast_to(np.asarray(c, np.float64), f.shape) for c in (x0, y0, x1, y1, r, aux)], 1)
        words = np.broadcast_to(colour_words(colour), lead).reshape(-1) if np.ndim(colour) > 1 else np.full(f.shape, colour_words(colour))
        keep = np.isfinite(cols).all(1) & (np.abs(cols[:, :coords]) <= MAX_COORD).all(1)
        keep &= (cols[:, 4:] >= 0).all(1) & (cols[:, 4:] <= MAX_RADIUS).all(1)
        rec = np.empty((int(keep.sum()), 8), np.int64)
        rec[:, 0] = kind
        rec[:, 1:7] = cols[keep]
        rec[:, 7] = words[keep]
        self._frames.append(f[keep])
        self._records.append(rec.astype(np.uint32).view(np.int32) if rec.size else np.zeros((0, 8), np.int32))
        return self

    def discs(self, xy, radius, colour, inner=0, frames=None):
        """Filled discs, or rings with `inner` > 0.  `radius` as cv2.circle takes it: a disc of radius r reaches the far edge of the
        pixels r away, so its geometric radius is r + 0.5 pixels (radius 0 is one pixel); `inner` likewise, 0 for none."""
        p, f, lead = self._points(xy, frames)
        r = np.floor((self._per_point(radius, lead, "radius") + 0.5) * 16.0 + 0.5)
        inner = self._per_point(inner, lead, "inner")
        aux = np.where(inner > 0, np.floor((inner + 0.5) * 16.0 + 0.5), 0.0)
        return self._add(f, KIND_DISC, fixed(p[:, 0]), fixed(p[:, 1]), 0, 0, r, aux, colour, lead, coords=2)

    def segments(self, a, b, width, colour, frames=None):
        """Strokes from a to b, `width` pixels wide, with round caps (cv2.line's thickness)."""
        pa, f, lead = self._points(a, frames)
        pb, _, lead_b = self._points(b, frames)
        if lead != lead_b:
            raise ValueError(f"a and b differ in shape: {lead} and {lead_b}")
        r = np.floor(self._per_point(width, lead, "width") * 8.0 + 0.5)
        return self._add(f, KIND_CAPSULE, fixed(pa[:, 0]), fixed(pa[:, 1]), fixed(pb[:, 0]), fixed(pb[:, 1]), r, 0, colour, lead)

    def boxes(self, xywh, colour, thickness=0):
        """One box per frame, xywh (n_frames, 4): the pixels x .. x + w by y .. y + h, corners included (cv2.rectangle's two points).
        thickness 0 fills it; otherwise an outline of that many pixels, drawn inwards."""
        b = _host(xywh).astype(np.float64)
        if b.shape != (self.n_frames, 4):
            raise ValueError(f"boxes must be ({self.n_frames}, 4), got {b.shape}")
        f = np.arange(self.n_frames, dtype=np.int64)
        aux = np.floor(self._per_point(thickness, f.shape, "thickness") * 16.0 + 0.5)
        return self._add(f, KIND_BOX, fixed(b[:, 0]) - 8, fixed(b[:, 1]) - 8, fixed(b[:, 0] + b[:, 2]) + 8, fixed(b[:, 1] + b[:, 3]) + 8,
                         0, aux, colour, f.shape)

    def arrows(self, a, b, width, colour, tip=0.2, frames=None):
        """cv2.arrowedLine: the shaft a -> b and two tip strokes from b, of length tip * |b - a|, at +-45 degrees back towards a."""
        pa, pb = _host(a).astype(np.float64), _host(b).astype(np.float64)
        back = (pa - pb) * float(tip)
        c = np.sqrt(0.5)
        left = pb + np.stack([c * (back[..., 0] - back[..., 1]), c * (back[..., 0] + back[..., 1])], -1)
        right = pb + np.stack([c * (back[..., 0] + back[..., 1]), c * (back[..., 1] - back[..., 0])], -1)
        self.segments(pa, pb, width, colour, frames)
        self.segments(pb, left, width, colour, frames)
        return self.segments(pb, right, width, colour, frames)

    def text(self, strings, xy, colour, scale=2, frames=None):
        """One line per point: strings[i] with the bottom-left corner of its first cell's ink at pixel xy[i], as cv2.putText takes
        it.  `scale` is the side of a font pixel in pixels; a character is 5 x 7 font pixels and the advance is 6.  Characters
        outside ASCII 32 .. 126 print as `?`."""
        p = _host(xy).astype(np.float64)
        if frames is None:
            if p.shape != (self.n_frames, 2):
                raise ValueError(f"xy must be ({self.n_frames}, 2), got {p.shape}")
            f = np.arange(self.n_frames, dtype=np.int64)
        else:
            p, f, _ = self._points(p, frames)
        strings = [strings] * f.size if isinstance(strings, str) else list(strings)
        if len(strings) != f.size:
            raise ValueError(f"{len(strings)} strings for {f.size} points")
        side = float(np.floor(float(scale) * 16.0 + 0.5))
        if not 1 <= side <= MAX_RADIUS:
            raise ValueError(f"scale = {scale} gives a font pixel of {side:.0f}/16 pixels: outside [1, {MAX_RADIUS}]")
        lengths = np.array([len(s) for s in strings], np.int64)
        codes = np.frombuffer("".join(strings).encode("latin-1", "replace"), np.uint8).astype(np.int64)
        codes = np.where((codes < FONT_FIRST) | (codes >= FONT_FIRST + len(_GLYPHS)), ord("?"), codes) - FONT_FIRST
        line = np.repeat(np.arange(f.size), lengths)                                   # the line of every character
        column = np.arange(codes.size) - np.repeat(np.cumsum(lengths) - lengths, lengths)
        x0 = fixed(p[line, 0]) - 8 + column * (FONT_ADVANCE * side)
        y0 = fixed(p[line, 1]) + 8 - FONT_ROWS * side
        keep = np.isfinite(x0) & np.isfinite(y0) & (np.abs(x0) <= MAX_COORD) & (np.abs(y0) <= MAX_COORD)
        rec = np.zeros((int(keep.sum()), 8), np.int64)
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] = KIND_GLYPH, x0[keep], y0[keep], side, codes[keep]
        rec[:, 7] = colour_words(colour)
        self._frames.append(f[line][keep])
        self._records.append(rec.astype(np.uint32).view(np.int32) if rec.size else np.zeros((0, 8), np.int32))
        return self

    # ---- the operator's tables
    def build_host(self):
        """-> (prims (P, 8) int32, prim_offsets (n_frames + 1) int32) as numpy arrays: the records ordered by frame and, within a
        frame, by call order and by position within a call (a stable sort)."""
        f = np.concatenate(self._frames) if self._frames else np.zeros(0, np.int64)
        rec = np.concatenate(self._records) if self._records else np.zeros((0, 8), np.int32)
        order = np.argsort(f, kind="stable")
        offsets = np.zeros(self.n_frames + 1, np.int64)
        offsets[1:] = np.cumsum(np.bincount(f, minlength=self.n_frames))
        if offsets[-1] >= 1 << 31:
            raise ValueError(f"{offsets[-1]} records do not fit the operator's int32 offsets")
        return np.ascontiguousarray(rec[order]), offsets.astype(np.int32)

    def build(self, device="cuda"):
        """`build_host` as tensors on `device`."""
        import torch
        prims, offsets = self.build_host()
        return torch.from_numpy(prims).to(device), torch.from_numpy(offsets).to(device)

    def draw(self, frames, samples=16, out=None):
        """Draws onto frames (n_frames, H, W, 1 | 3 | 4) uint8 on the device: ops.draw_overlay with this project's FONT."""
        import torch
        from .. import ops
        if frames.shape[0] != self.n_frames:
            raise ValueError(f"{frames.shape[0]} frames for an overlay of {self.n_frames}")
        prims, offsets = self.build(frames.device)
        return ops.draw_overlay(frames, prims, offsets, torch.from_numpy(np.array(FONT)).to(frames.device), samples, out)


# ----------------------------------------------------------------------------- the reference's three checking videos
def box_overlay(boxes, colour=(0, 255, 0), thickness=2, into=None):
    """Step 1's video: the smoothed box (F, 4) = x, y, w, h of every frame, outlined (cv2.rectangle(image, (x, y), (x + w, y + h),
    (0, 255, 0), 2)).  A frame whose box holds a NaN gets none.  into: an Overlay to add to."""
    b = _host(boxes)
    ov = Overlay(b.shape[0]) if into is None else into
    return ov.boxes(b, colour, thickness)


def landmark_overlay(points, radius=1, colour=(255, 255, 0), into=None):
    """Step 3's video: the landmarks (F, K, 2 | 3) in pixel coordinates as filled circles (cv2.circle(image, (x, y), 1, (255, 255,
    0), -1)); only x and y are used, at their sub-pixel positions."""
    p = _host(points)
    if p.ndim != 3 or p.shape[2] not in (2, 3):
        raise ValueError(f"points must be (F, K, 2 | 3), got {p.shape}")
    ov = Overlay(p.shape[0]) if into is None else into
    return ov.discs(p[:, :, :2], radius, colour)


AXIS_COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255))      # X, Y, Z in red, green, blue for RGB frames


def head_pose_overlay(ypr, boxes, axis_length=200, into=None):
    """Step 2's video: the head's three axes as arrows from the box centre (x + w // 2, y + h // 2) to the centre plus the first
    two rows of R = ypr_to_matrix(ypr) times the axis (an orthographic view), truncated to whole pixels as the reference does,
    width 2, tip 0.2; and the line `Yaw: .., Pitch: .., Roll: ..` in white at (x, y - 10).  ypr (F, 3) in degrees, boxes (F, 4) =
    x, y, w, h.  A frame with a NaN in either gets nothing."""
    a, b = _host(ypr).astype(np.float64).reshape(-1, 3), _host(boxes).astype(np.float64)
    if b.shape != (a.shape[0], 4):
        raise ValueError(f"boxes must be ({a.shape[0]}, 4) for {a.shape[0]} rotations, got {b.shape}")
    ov = Overlay(a.shape[0]) if into is None else into
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    a, b = np.where(ok[:, None], a, 0.0), np.where(ok[:, None], b, np.nan)         # NaN drops the frame's arrows
    R = ypr_to_matrix(a)
    centre = np.stack([b[:, 0] + np.floor(b[:, 2] / 2), b[:, 1] + np.floor(b[:, 3] / 2)], 1)
    for k, colour in enumerate(AXIS_COLOURS):
        ov.arrows(centre, np.trunc(centre + float(axis_length) * R[:, :2, k]), 2, colour, tip=0.2)
    idx = np.flatnonzero(ok)
    lines = [f"Yaw: {a[i, 0]:.2f}, Pitch: {a[i, 1]:.2f}, Roll: {a[i, 2]:.2f}" for i in idx]
    at = np.stack([np.rint(b[idx, 0]), np.rint(b[idx, 1]) - 10], 1)
    return ov.text(lines, at, (255, 255, 255), scale=2, frames=idx)


# ----------------------------------------------------------------------------- command line
def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m msmd_amd.utils.overlay",
                                 description="Draw the box track, the landmarks and the head pose of a clip onto its frames.")
    ap.add_argument("--frames", required=True, help="a Motion-JPEG .avi, or an .npy of (F, H, W, 3) uint8")
    ap.add_argument("--out", required=True, metavar="OUT.avi")
    ap.add_argument("--boxes", default=None, help="Step 1's .pickle: processed_bbox_frames if present, else raw_bbox_frames")
    ap.add_argument("--landmarks", default=None, help=".npy of (F, K, 2 | 3) landmarks in pixel coordinates; x and y are used")
    ap.add_argument("--head_rot", default=None, help="Step 2's pickle of (F, 3) yaw / pitch / roll in degrees (needs --boxes)")
    ap.add_argument("--samples", type=int, default=16, choices=(1, 16), help="sample points per pixel")
    ap.add_argument("--fps", type=float, default=None, help="default: the rate of an .avi given as --frames, else the pickle's, else 30")
    ap.add_argument("--audio", default=None, metavar="WAV")
    ap.add_argument("--quality", type=int, default=90, help="JPEG quality, 1 .. 100")
    ap.add_argument("--chunk", type=int, default=64, help="frames on the device at a time")
    return ap


def _clip_overlay(args, F):
    """The tables named on the command line -> (Overlay over F frames, the box pickle's fps or None)."""
    ov, fps, boxes = Overlay(F), None, None

    def rows(a):
        a = np.asarray(a, np.float64)
        if a.shape[0] < F:                                       # a track that ends early: the rest of the clip gets nothing
            a = np.concatenate([a, np.full((F - a.shape[0],) + a.shape[1:], np.nan)], 0)
        return a[:F]

    if args.boxes is not None:
        with open(args.boxes, "rb") as f:
            meta = pkl.load(f)
        raw = meta["processed_bbox_frames"] if "processed_bbox_frames" in meta else meta["raw_bbox_frames"]
        boxes = rows(np.array([[np.nan] * 4 if b is None or len(b) != 4 else list(b) for b in raw], np.float64).reshape(-1, 4))
        fps = meta.get("fps")
        box_overlay(boxes, into=ov)
    if args.landmarks is not None:
        landmark_overlay(rows(np.load(args.landmarks)), into=ov)
    if args.head_rot is not None:
        with open(args.head_rot, "rb") as f:
            head_pose_overlay(rows(np.asarray(pkl.load(f), np.float64).reshape(-1, 3)), boxes, into=ov)
    return ov, fps


def main(argv=None):
    import torch
    from .. import ops
    from . import media
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.head_rot is not None and args.boxes is None:
        ap.error("--head_rot needs --boxes: the arrows start at the box centre")
    if not 1 <= args.quality <= 100 or args.chunk < 1:
        ap.error("--quality is 1 .. 100 and --chunk at least 1")
    clip = host = None
    if args.frames.lower().endswith(".avi"):
        clip = media.read_avi(args.frames)
        F = len(clip.frames)
    else:
        host = np.load(args.frames, mmap_mode="r")
        F = host.shape[0]
    ov, box_fps = _clip_overlay(args, F)
    prims, offsets = ov.build_host()
    font = torch.from_numpy(np.array(FONT)).to("cuda")
    prims_dev = torch.from_numpy(prims).to("cuda")
    jpegs, size = [], None
    for i in range(0, F, args.chunk):
        j = min(i + args.chunk, F)
        if clip is not None:
            frames = ops.jpeg_decode([clip.jpeg(k) for k in range(i, j)])
        else:
            frames = torch.from_numpy(np.array(host[i:j])).to("cuda")
        off = torch.from_numpy(offsets[i:j + 1].copy()).to("cuda")       # the chunk's ranges of the one record table
        ops.draw_overlay(frames, prims_dev, off, font, args.samples)
        jpegs += media.encode_jpeg(frames, args.quality)
        size = (frames.shape[2], frames.shape[1])
    fps = args.fps if args.fps is not None else clip.fps if clip is not None else box_fps if box_fps is not None else 30
    audio = None
    if args.audio is not None:
        from .audio import read_wav
        audio = read_wav(args.audio)
    elif clip is not None:
        audio = clip.audio
    n = media.write_avi(args.out, jpegs, fps, size, audio)
    print(f"wrote {args.out}: {F} frames with {prims.shape[0]} primitives, {n} bytes")


if __name__ == "__main__":
    main()
