"""The resize operator on the host: the numpy restatement of tests/resize_ref.py against Pillow byte for byte,
`ops.resize_tables` against the restatement entry for entry, the int32 condition, planted mutants of the restatement that the
inputs must tell apart, `media.frames_at` against Fraction arithmetic, and the route rule at the edges of its LDS bound."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from PIL import Image

import resize_ref as rr
from msmd_amd import ops

PIL_FILTER = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
              "lanczos": Image.Resampling.LANCZOS}
SOURCES = [(1, 1), (7, 5), (33, 64), (65, 31), (120, 97)]          # (width, height)
MODE = {1: "L", 3: "RGB", 4: "CMYK"}


def targets(w, h):
    """1 x 1, the same size, about 2x up on one axis only (each axis), about 1/2 and 1/3 down, and 224 x 224."""
    t = [(1, 1), (w, h), (2 * w + 1, h), (w, 2 * h - 1 if h > 1 else 2), (max(1, (w + 1) // 2), max(1, h // 2)),
         (max(1, w // 3), max(1, (h + 2) // 3)), (224, 224)]
    return list(dict.fromkeys(t))


def boxes(w, h):
    """The whole image, an integer box and a fractional one on the quarter-pixel grid (exact in float32)."""
    out = [None]
    if w >= 5 and h >= 5:
        out += [(1, 2, w - 2, h - 1), (0.25, 1.5, w - 1.75, h - 0.25)]
    return out


CASES = [(src, dst, f, C, box) for src in SOURCES for dst in targets(*src) for f in rr.FILTERS for C in (1, 3, 4)
         for box in boxes(*src)]


@functools.lru_cache(maxsize=None)
def image(w, h, C):
    a = rr.content("random", (h, w, C), "resize_cpu")
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pillow(src, dst, f, C, box):
    im = Image.fromarray(image(src[0], src[1], C)[:, :, 0] if C == 1 else image(src[0], src[1], C), MODE[C])
    out = np.asarray(im.resize(dst, PIL_FILTER[f], box=box, reducing_gap=None))
    return out[:, :, None] if C == 1 else out


def test_restatement_equals_pillow():
    bad = [c for c in CASES if not np.array_equal(rr.resize(image(c[0][0], c[0][1], c[3]), c[1], c[2], c[4]), pillow(*c))]
    assert not bad, f"{len(bad)} of {len(CASES)} cases differ from Pillow, first {bad[:3]}"


def axes_of(cases):
    """The distinct 1-D tables the cases use: (n_in, n_out, filter, in0, in1) of every pass that is not skipped."""
    seen = {}
    for (w, h), (wd, hd), f, _, box in cases:
        x0, y0, x1, y1 = rr.float32_box(box, w, h)
        for n_in, n_out, a, b in ((w, wd, x0, x1), (h, hd, y0, y1)):
            if not (n_in == n_out and a == 0.0 and b == float(n_in)):
                seen[(n_in, n_out, f, a, b)] = None
    return list(seen)


def test_tables_equal_the_restatement():
    axes = axes_of(CASES)
    assert len(axes) > 100
    for n_in, n_out, f, a, b in axes:
        bounds, coef = ops.resize_tables(n_in, n_out, f, a, b)
        rb, rc = rr.tables(n_in, n_out, f, a, b)
        assert bounds.dtype == np.int32 and coef.dtype == np.int32
        assert np.array_equal(bounds, rb) and np.array_equal(coef, rc), (n_in, n_out, f, a, b)
    # the whole axis by default
    assert all(np.array_equal(u, v) for u, v in zip(ops.resize_tables(33, 7, "lanczos"), rr.tables(33, 7, "lanczos", 0.0, 33.0)))


def test_int32_condition():
    extra = [(4096, 1, f, 0.0, 4096.0) for f in rr.FILTERS] + [(5, 4096, f, 0.0, 5.0) for f in rr.FILTERS]
    peak = 0
    for n_in, n_out, f, a, b in axes_of(CASES) + extra:
        p = rr.accumulator_peak(rr.tables(n_in, n_out, f, a, b)[1])
        assert p < 2 ** 31, (n_in, n_out, f, a, b, p)
        peak = max(peak, p)
        ops.resize_tables(n_in, n_out, f, a, b)           # raises where the condition fails
    print(f"largest accumulator bound: {peak / 2 ** 22 / 255:.3f} x 255 x 2^22")


@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_mutant_is_caught(mutant):
    """Every planted departure from the rule changes at least one case's bytes: the inputs tell the rule from its neighbours."""
    caught = 0
    for c in CASES:
        (w, h), dst, f, C, box = c
        caught += not np.array_equal(rr.resize(image(w, h, C), dst, f, box, mutant=mutant), pillow(*c))
        if caught:
            break
    assert caught, f"mutant {mutant} equals Pillow on every case: the inputs are too weak"


def test_resize_tables_refuses():
    for bad in [dict(n_in=4, n_out=0, filter="box"), dict(n_in=0, n_out=3, filter="box"), dict(n_in=4, n_out=2, filter="nearest"),
                dict(n_in=4, n_out=2, filter="box", in0=2.0, in1=2.0), dict(n_in=4, n_out=2, filter="box", in0=-1.0, in1=3.0),
                dict(n_in=4, n_out=2, filter="box", in0=0.0, in1=4.5)]:
        with pytest.raises(ValueError):
            ops.resize_tables(**bad)


def test_frames_at():
    from msmd_amd.utils import media
    rates = [25, 30, Fraction(30000, 1001), 50]
    for fo in rates:
        for fs in rates:
            for n_src in (1, 2, 97):
                n_out = math.ceil(n_src * Fraction(fo) / Fraction(fs)) + 3        # runs past the source's end: the clamp
                got = media.frames_at(n_out, fo, n_src, fs)
                assert got == rr.frames_at(n_out, fo, n_src, fs), (fo, fs, n_src)
                assert got[0] == 0 and got[-1] == n_src - 1 and all(b >= a for a, b in zip(got, got[1:]))
    assert media.frames_at(5, 25, 10, 50) == [0, 2, 4, 6, 8]
    assert media.frames_at(4, 50, 10, 25) == [0, 1, 1, 2]                          # a tie goes to the later frame
    assert media.frames_at(3, 29.97, 9, 29.97) == [0, 1, 2]


def test_route_at_the_edges_of_the_lds_rule():
    for C in (1, 3, 4):
        row = ops.RESIZE_TILE_W * C + 4
        fit = ops.RESIZE_LDS_BYTES // row
        assert fit * row <= ops.RESIZE_LDS_BYTES < (fit + 1) * row
        assert ops.resize_fits(C, 1) and ops.resize_fits(C, fit) and not ops.resize_fits(C, fit + 1) and not ops.resize_fits(C, 0)
        # a shape whose tiles do not overlap (one tile, span = Hs) follows the LDS rule alone
        route = lambda span: ops.resize_route(C, span, 4, span, 1, 8, 3)
        assert route(1) == "fused" and route(fit) == "fused" and route(fit + 1) == "two_pass"
        assert ops.resize_route(C, 0, 4, 8, 1, 8, 3) == "two_pass"
    assert not ops.resize_fits(2, 1) and ops.resize_route(2, 1, 1, 1, 1, 1, 1) == "two_pass"
    # the span the rule is fed: lanczos 600 -> 2 needs every source row; bilinear 2x down has the taps [2 y - 1, 2 y + 3), so a
    # tile of T rows touches 2 (T - 1) + 4 rows inside the image (6 T -> 3 T has such a tile) and one less where the image's
    # edge cuts a tap off (4 T -> 2 T has only such tiles)
    span = lambda n_in, n_out, f: ops.resize_rows_span(ops.resize_tables(n_in, n_out, f)[0][None], n_in, ops.resize_tables(n_in, n_out, f)[1].shape[1])
    T = ops.RESIZE_TILE_H
    assert span(600, 2, "lanczos") == 600 and not ops.resize_fits(3, 600) and ops.resize_route(3, 600, 1, 600, 2, 5, 3) == "two_pass"
    assert span(4 * T, 2 * T, "bilinear") == 2 * T + 1 and span(6 * T, 3 * T, "bilinear") == 2 * T + 2
    assert ops.resize_fits(3, 2 * T + 2)
    # the measured part of the rule, at its two edges: tiles_y tiles of `s` rows repeat (s tiles_y - Hs) kx multiply-adds per Hs
    # intermediate bytes; two launches where that is more than one and the intermediate N Hs Wd C stays within RESIZE_CACHE_BYTES
    Hs, Hd, Wd, kx, C = 512, 8 * T, 256, 13, 3                  # 8 tiles
    s_edge = (Hs // kx + Hs) // 8                                # the largest span with (8 s - Hs) kx <= Hs
    assert (8 * s_edge - Hs) * kx <= Hs < (8 * (s_edge + 1) - Hs) * kx
    n_edge = ops.RESIZE_CACHE_BYTES // (Hs * Wd * C)
    assert ops.resize_route(C, s_edge, n_edge, Hs, Hd, Wd, kx) == "fused"
    assert ops.resize_route(C, s_edge + 1, n_edge, Hs, Hd, Wd, kx) == "two_pass"
    assert ops.resize_route(C, s_edge + 1, n_edge + 1, Hs, Hd, Wd, kx) == "fused"
    b, c = rr.tables(4 * T, 2 * T, "bilinear")
    assert span(4 * T, 2 * T, "bilinear") == max(int((b[y:y + T, 0] + b[y:y + T, 1]).max() - b[y:y + T, 0].min()) for y in (0, T))
