"""The overlay operator's numpy restatement (tests/overlay_ref.py) against facts that do not come from it, six
planted mutants of the restatement each caught by a named case, and the host side of utils/overlay.py: the builder, the font and
ypr_to_matrix.  No GPU."""
import os

import numpy as np
import pytest

import headpose_ref as hr
import overlay_ref as R
from msmd_amd import _lib
from msmd_amd.utils import overlay as ov

HEADER = _lib.parse_constants()
WHITE = (255, 255, 255, 255)


def one(frame, recs, samples=16, font=None, mutant=None):
    """One frame (H, W, C) and a list of records -> the drawn frame."""
    prims = np.stack(recs) if recs else np.zeros((0, 8), np.int32)
    return R.draw(frame[None], prims, [0, len(recs)], font, samples, mutant)[0]


def grey(H, W, C=1, value=10):
    return np.full((H, W, C), value, np.uint8)


# ----------------------------------------------------------------------------- the cases: each takes the mutant to plant
def case_box_equals_pillow(mutant=None):
    """An opaque box with integer corners at samples = 1, filled and as an outline of thickness 2: PIL.ImageDraw.rectangle's bytes."""
    Image = pytest.importorskip("PIL.Image")
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    x0, y0, x1, y1 = 3, 2, 11, 9
    colour = (200, 30, 90)
    for aux, kw in ((0, dict(fill=colour)), (32, dict(outline=colour, width=2))):
        im = Image.new("RGB", (23, 17), (10, 10, 10))
        ImageDraw.Draw(im).rectangle([x0, y0, x1, y1], **kw)
        got = one(grey(17, 23, 3), [R.record(R.BOX, 16 * x0, 16 * y0, 16 * x1 + 16, 16 * y1 + 16, 0, aux, colour)], 1, mutant=mutant)
        assert np.array_equal(got, np.asarray(im)), aux


def case_alpha_ends(mutant=None):
    """A = 0 changes nothing; A = 255 with full coverage gives the colour."""
    rng = np.random.default_rng(1)
    frame = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    for s in (1, 16):
        box = lambda a: R.record(R.BOX, 16 * 2, 16 * 3, 16 * 8, 16 * 7, 0, 0, (7, 99, 250, a))
        assert np.array_equal(one(frame, [box(0)], s, mutant=mutant), frame)
        got = one(frame, [box(255)], s, mutant=mutant)
        assert (got[3:7, 2:8] == (7, 99, 250)).all()
        got[3:7, 2:8] = frame[3:7, 2:8]
        assert np.array_equal(got, frame)


def case_half_pixel(mutant=None):
    """A box over the left half of pixel (row 1, column 2): cov = 8 of 16, and the byte is the blend formula's."""
    rec = R.record(R.BOX, 32, 16, 40, 32, 0, 0, (21, 21, 21, 255))
    assert R.coverage(rec, 3, 4, 16, None, mutant)[1, 2] == 8 and R.coverage(rec, 3, 4, 16, None, mutant).sum() == 8
    got = one(grey(3, 4), [rec], 16, mutant=mutant)
    assert got[1, 2, 0] == (10 * (4080 - 2040) + 21 * 2040 + 2040) // 4080 == 16
    rec = R.record(R.BOX, 32, 16, 40, 32, 0, 0, (21, 21, 21, 100))             # translucent: w = 8 * 100
    assert one(grey(3, 4), [rec], 16, mutant=mutant)[1, 2, 0] == (10 * (4080 - 800) + 21 * 800 + 2040) // 4080 == 12


def case_edges_are_inside(mutant=None):
    """`<=` everywhere: at samples = 1 a disc of radius 5 px centred on a pixel centre holds the pixels (3, 4) and (5, 0) away, 81
    pixels in all; a box from one pixel centre to another holds both; its outline of 16/16 px is exactly the border pixels."""
    disc = R.record(R.DISC, 16 * 8 + 8, 16 * 8 + 8, 0, 0, 80, 0, WHITE)
    cov = R.coverage(disc, 17, 17, 1, None, mutant)
    assert cov[8 + 4, 8 + 3] == 1 and cov[8, 8 + 5] == 1 and cov[8 - 5, 8] == 1 and cov.sum() == 81
    ring = R.record(R.DISC, 16 * 8 + 8, 16 * 8 + 8, 0, 0, 80, 80, WHITE)      # aux = r: the lattice points on the circle, 12
    assert R.coverage(ring, 17, 17, 1, None, mutant).sum() == 12
    box = R.record(R.BOX, 16 * 2 + 8, 16 * 2 + 8, 16 * 8 + 8, 16 * 8 + 8, 0, 0, WHITE)
    cov = R.coverage(box, 11, 11, 1, None, mutant)
    assert cov.sum() == 49 and cov[2:9, 2:9].all()
    outline = R.record(R.BOX, 16 * 2 + 8, 16 * 2 + 8, 16 * 8 + 8, 16 * 8 + 8, 0, 16, WHITE)
    cov = R.coverage(outline, 11, 11, 1, None, mutant)
    assert cov.sum() == 24 and not cov[3:8, 3:8].any()


def case_disc_symmetry(mutant=None):
    """A disc centred on a pixel centre is unchanged by the eight symmetries of the square."""
    for r in (13, 40, 57):
        for s in (1, 16):
            cov = R.coverage(R.record(R.DISC, 16 * 6 + 8, 16 * 6 + 8, 0, 0, r, 0, WHITE), 13, 13, s, None, mutant)
            assert cov.sum() > 0
            for k in range(4):
                assert np.array_equal(np.rot90(cov, k), cov) and np.array_equal(np.rot90(cov, k).T, cov)


def case_capsule_point_is_disc(mutant=None):
    """A capsule with a = b gives the disc's bytes."""
    frame = np.random.default_rng(2).integers(0, 256, (12, 14, 3), dtype=np.uint8)
    for s in (1, 16):
        disc = one(frame, [R.record(R.DISC, 101, 77, 0, 0, 50, 0, (9, 200, 30, 180))], s, mutant=mutant)
        caps = one(frame, [R.record(R.CAPSULE, 101, 77, 101, 77, 50, 0, (9, 200, 30, 180))], s, mutant=mutant)
        assert np.array_equal(disc, caps) and not np.array_equal(disc, frame)


def case_capsule_ends_swap(mutant=None):
    """Swapping a and b changes nothing; and the capsule holds the discs at both ends and the band between them."""
    frame = grey(20, 24, 3)
    for a, b in (((40, 50), (300, 260)), ((333, 17), (20, 290)), ((100, 100), (100, 250))):
        for s in (1, 16):
            ab = one(frame, [R.record(R.CAPSULE, *a, *b, 37, 0, (250, 0, 120, 200))], s, mutant=mutant)
            ba = one(frame, [R.record(R.CAPSULE, *b, *a, 37, 0, (250, 0, 120, 200))], s, mutant=mutant)
            assert np.array_equal(ab, ba) and not np.array_equal(ab, frame)
            cap = R.coverage(R.record(R.CAPSULE, *a, *b, 37, 0, WHITE), 20, 24, s, None, mutant)
            for c in (a, b):
                assert (cap >= R.coverage(R.record(R.DISC, *c, 0, 0, 37, 0, WHITE), 20, 24, s, None, mutant)).all()


def case_glyph_scales(mutant=None):
    """A glyph at font-pixel side 32 and samples = 1 is np.kron of the glyph at side 16, which is the font's bits."""
    for g in (ord("A") - 32, ord("g") - 32, ord("%") - 32):
        small = R.coverage(R.record(R.GLYPH, 16, 32, 16, g), 12, 12, 1, ov.FONT, mutant)
        bits = np.unpackbits(ov.FONT[g][:, None], axis=1).astype(np.int64)
        assert np.array_equal(small[2:10, 1:9], bits) and small.sum() == bits.sum()
        big = R.coverage(R.record(R.GLYPH, 16, 32, 32, g), 20, 20, 1, ov.FONT, mutant)
        assert np.array_equal(big[2:18, 1:17], np.kron(bits, np.ones((2, 2), np.int64))) and big.sum() == 4 * bits.sum()


def case_order_matters(mutant=None):
    """Two translucent overlapping records in the two orders give different bytes, each the formula applied in that order."""
    a = R.record(R.BOX, 0, 0, 64, 64, 0, 0, (200, 200, 200, 128))
    b = R.record(R.BOX, 32, 32, 96, 96, 0, 0, (30, 30, 30, 128))
    step = lambda d, c: (d * (4080 - 16 * 128) + c * 16 * 128 + 2040) // 4080
    ab, ba = one(grey(6, 6), [a, b], mutant=mutant), one(grey(6, 6), [b, a], mutant=mutant)
    assert ab[2, 2, 0] == step(step(10, 200), 30) and ba[2, 2, 0] == step(step(10, 30), 200) and ab[2, 2, 0] != ba[2, 2, 0]
    assert ab[0, 0, 0] == ba[0, 0, 0] == step(10, 200) and ab[5, 5, 0] == ba[5, 5, 0] == step(10, 30)


def wide_capsule():
    return R.record(R.CAPSULE, 37, -2 ** 20 + 5, -11, 2 ** 20 - 3, 40, 0, WHITE)


def case_128_bit_products(mutant=None):
    """The capsule from (37, -2^20 + 5) to (-11, 2^20 - 3) with r = 40 on 4096 x 2 pixels covers 104 of the 131 072 sample points,
    counted here with Python integers one row of sample points at a time."""
    rec = wide_capsule()
    cov = R.coverage(rec, 2, 4096, 16, None, mutant)
    x0, y0, x1, y1, r = (int(v) for v in rec[1:6])
    dx, dy = x1 - x0, y1 - y0
    L, count = dx * dx + dy * dy, 0
    for py in (2, 6, 10, 14, 18, 22, 26, 30):
        for px in range(2, 16 * 4096, 4):
            qx, qy = px - x0, py - y0
            s = qx * dx + qy * dy
            assert 0 < s < L
            count += (qx * dy - qy * dx) ** 2 <= r * r * L
    assert count == 104 and cov.sum() == 104


CASES = [case_box_equals_pillow, case_alpha_ends, case_half_pixel, case_edges_are_inside, case_disc_symmetry, case_capsule_point_is_disc,
         case_capsule_ends_swap, case_glyph_scales, case_order_matters, case_128_bit_products]
CAUGHT_BY = {"lt": case_edges_are_inside, "no_caps": case_capsule_point_is_disc, "backwards": case_order_matters,
             "no_round": case_half_pixel, "wrap64": case_128_bit_products, "inner_lt": case_edges_are_inside}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_restatement(case):
    case()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_planted_mutant_is_caught(mutant):
    assert set(CAUGHT_BY) == set(R.MUTANTS)
    with pytest.raises(AssertionError):
        CAUGHT_BY[mutant](mutant)


def test_wrapped_products_decide_64360_sample_points_differently():
    px, py = R.sample_points(2, 4096, 16)
    assert int((R.inside(wide_capsule(), px, py, None) != R.inside(wide_capsule(), px, py, None, "wrap64")).sum()) == 64360


def test_constants_are_the_headers():
    assert (R.TILE_W, R.TILE_H, R.CHUNK) == (HEADER["MSMD_OVERLAY_TILE_W"], HEADER["MSMD_OVERLAY_TILE_H"], HEADER["MSMD_OVERLAY_CHUNK"])
    assert R.MAX_COORD == ov.MAX_COORD == HEADER["MSMD_OVERLAY_MAX_COORD"] == 1 << 20
    assert R.MAX_RADIUS == ov.MAX_RADIUS == HEADER["MSMD_OVERLAY_MAX_RADIUS"] == 1 << 16
    kinds = [HEADER["MSMD_OVERLAY_" + n] for n in ("NONE", "DISC", "CAPSULE", "BOX", "GLYPH")]
    assert kinds == [R.NONE, R.DISC, R.CAPSULE, R.BOX, R.GLYPH] == [0, ov.KIND_DISC, ov.KIND_CAPSULE, ov.KIND_BOX, ov.KIND_GLYPH]


def test_records_that_draw_nothing():
    ok = R.record(R.DISC, 5, 5, 0, 0, 9)
    assert R.draws(ok, 0)
    for field, value in ((0, 5), (0, -1), (0, 0), (1, R.MAX_COORD + 1), (2, -R.MAX_COORD - 1), (3, R.MAX_COORD + 1), (5, -1),
                         (5, R.MAX_RADIUS + 1), (6, R.MAX_RADIUS + 1)):
        rec = ok.copy()
        rec[field] = value
        assert not R.draws(rec, 0), (field, value)
    for field, value in ((1, R.MAX_COORD), (2, -R.MAX_COORD), (4, -R.MAX_COORD), (5, R.MAX_RADIUS), (6, R.MAX_RADIUS)):
        rec = ok.copy()
        rec[field] = value
        assert R.draws(rec, 0), (field, value)
    glyph = R.record(R.GLYPH, 0, 0, 16, 3)
    assert R.draws(glyph, 4) and not R.draws(glyph, 3) and not R.draws(R.record(R.GLYPH, 0, 0, 0, 3), 4)
    assert not R.draws(R.record(R.GLYPH, 0, 0, R.MAX_RADIUS + 1, 3), 4) and not R.draws(R.record(R.GLYPH, 0, 0, 16, -1), 4)


# ----------------------------------------------------------------------------- the builder
def test_fixed_point_rule():
    assert ov.fixed(0) == 8 and ov.fixed(-0.5) == 0 and ov.fixed(3) == 56
    assert ov.fixed(1 / 32) == 9 and ov.fixed(1 / 32 - 1e-9) == 8                       # a half rounds up
    assert ov.fixed(-1 / 32) == 8 and ov.fixed(-1 / 32 - 1e-9) == 7
    assert np.isnan(ov.fixed(np.nan))
    prims, off = ov.Overlay(1).discs(np.array([[2.0, 3.0]]), 0, (1, 2, 3)).build_host()
    assert prims.tolist() == [[ov.KIND_DISC, 40, 56, 0, 0, 8, 0, R.record(0, colour=(1, 2, 3))[7]]] and off.tolist() == [0, 1]
    assert prims.dtype == np.int32 and off.dtype == np.int32


def test_nan_and_far_points_are_left_out_and_an_empty_frame_gets_an_empty_range():
    xy = np.zeros((4, 3, 2))
    xy[0, 1, 0] = np.nan
    xy[1] = np.nan                                     # frame 1: nothing tracked
    xy[2, 2, 1] = 1e6                                  # beyond the coordinate limit
    xy[3, 0] = (65535.0, -65536.5)                     # 16 * 65535.5 <= 2^20 and -2^20: the last ones inside
    prims, off = ov.Overlay(4).discs(xy, 1, (9, 9, 9)).build_host()
    assert off.tolist() == [0, 2, 2, 4, 7] and prims.shape == (7, 8)
    assert prims[4, 1] == (1 << 20) - 8 and prims[4, 2] == -(1 << 20)
    assert all(R.draws(p, 0) for p in prims)
    p0, o0 = ov.Overlay(3).build_host()
    assert p0.shape == (0, 8) and o0.tolist() == [0, 0, 0, 0]
    assert ov.Overlay(0).build_host()[1].tolist() == [0]


def test_frames_are_ordered_stably_across_interleaved_calls():
    o = ov.Overlay(3)
    o.discs(np.array([[1.0, 1], [2, 2], [3, 3]]), 0, (1, 0, 0), frames=[2, 0, 2])
    o.boxes(np.array([[0, 0, 4, 4.0]] * 3), (2, 0, 0))
    o.discs(np.array([[4.0, 4], [5, 5]]), 0, (3, 0, 0), frames=[0, 2])
    prims, off = o.build_host()
    assert off.tolist() == [0, 3, 4, 8]
    assert (prims[:, 7] & 255).tolist() == [1, 2, 3, 2, 1, 1, 2, 3]                     # call order within every frame
    assert prims[[4, 5], 1].tolist() == [int(ov.fixed(1)), int(ov.fixed(3))]           # and position within a call
    with pytest.raises(ValueError):
        o.discs(np.zeros((1, 2)), 0, (1, 1, 1), frames=[3])
    with pytest.raises(ValueError):
        o.discs(np.zeros((2, 1, 2)), 0, (1, 1, 1))
    with pytest.raises(ValueError):
        o.discs(np.zeros((3, 2)), 0, (1, 1))


def test_boxes_and_colours():
    prims, _ = ov.Overlay(1).boxes(np.array([[3, 2, 8, 7.0]]), (1, 2, 3, 4), thickness=2).build_host()
    assert prims[0, :7].tolist() == [ov.KIND_BOX, 48, 32, 16 * 11 + 16, 16 * 9 + 16, 0, 32]          # the Pillow case's record
    assert int(prims[0, 7]) == 1 | 2 << 8 | 3 << 16 | 4 << 24
    assert ov.colour_words((255, 255, 0)) == 255 | 255 << 8 | 255 << 24
    words = ov.Overlay(1).discs(np.zeros((1, 2, 2)), 0, np.array([[[1, 2, 3], [4, 5, 6]]])).build_host()[0][:, 7]
    assert (words & 0xFFFFFF).tolist() == [1 | 2 << 8 | 3 << 16, 4 | 5 << 8 | 6 << 16]


def test_arrow_geometry():
    a, b, tip = np.array([[10.0, 20.0]]), np.array([[90.0, 80.0]]), 0.2
    prims, off = ov.Overlay(1).arrows(a, b, 2, (255, 0, 0), tip=tip).build_host()
    assert off.tolist() == [0, 3] and (prims[:, 0] == ov.KIND_CAPSULE).all() and (prims[:, 5] == 16).all()
    assert prims[0, 1:5].tolist() == [int(ov.fixed(v)) for v in (10, 20, 90, 80)]
    length, heading = np.hypot(80, 60), np.arctan2(-60, -80)                   # of the way back from b to a
    ends = set()
    for k, sign in ((1, +1), (2, -1)):
        assert prims[k, 1:3].tolist() == [int(ov.fixed(90)), int(ov.fixed(80))]
        want = b[0] + tip * length * np.array([np.cos(heading + sign * np.pi / 4), np.sin(heading + sign * np.pi / 4)])
        assert np.abs(prims[k, 3:5] - ((want + 0.5) * 16)).max() <= 1.0
        assert abs(np.hypot(*(prims[k, 3:5] - prims[k, 1:3])) / 16 - tip * length) < 0.1
        ends.add(tuple(prims[k, 3:5]))
    assert len(ends) == 2


def test_text_advance_and_origin():
    prims, off = ov.Overlay(2).text(["AB", "é~\n"], np.array([[5.0, 20.0], [0.0, 6.0]]), (255, 255, 255), scale=2).build_host()
    assert off.tolist() == [0, 2, 5] and (prims[:, 0] == ov.KIND_GLYPH).all() and (prims[:, 3] == 32).all()
    assert prims[:, 4].tolist() == [ord("A") - 32, ord("B") - 32, ord("?") - 32, ord("~") - 32, ord("?") - 32]
    assert prims[:2, 1].tolist() == [80, 80 + 6 * 32] and prims[:2, 2].tolist() == [16 * 21 - 7 * 32] * 2
    img = R.draw(np.zeros((1, 24, 30, 1), np.uint8), prims, [0, 2], ov.FONT, 1)[0, :, :, 0]
    ys, xs = np.nonzero(img)
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (7, 20, 5, 5 + 12 + 10 - 1)      # 'A': rows 7 .. 20; 'B' ends at column 26
    assert not img[:, 15:17].any()                                                      # the sixth font pixel is the gap
    one_px = ov.Overlay(1).text("A", np.array([[0.0, 6.0]]), (255, 255, 255), scale=1).build_host()[0]
    img = R.draw(np.zeros((1, 8, 8, 1), np.uint8), one_px, [0, 1], ov.FONT, 1)[0, :, :, 0]
    assert np.array_equal(img[:8, :8] > 0, np.unpackbits(ov.FONT[ord("A") - 32][:, None], axis=1) > 0)


def test_font():
    F = ov.FONT
    assert F.shape == (95, 8) and F.dtype == np.uint8
    assert (F & 0b111).max() == 0 and F[:, 7].max() == 0                     # inside 5 x 7 of the 8 x 8 cell
    assert F[0].max() == 0 and (F[1:].max(1) > 0).all()                     # the space alone is empty
    assert len({bytes(g) for g in F}) == 95
    with pytest.raises(ValueError):
        F[0, 0] = 1


def test_ypr_to_matrix_inverts_the_euler_rule():
    rng = np.random.default_rng(5)
    ypr = np.stack([rng.uniform(-180, 180, 200), rng.uniform(-89, 89, 200), rng.uniform(-180, 180, 200)], 1)
    Rm = ov.ypr_to_matrix(ypr)
    assert Rm.dtype == np.float64 and Rm.shape == (200, 3, 3)
    assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-12
    assert np.abs(hr.euler_yxz_deg(Rm) - ypr).max() < 1e-9
    assert np.abs(Rm - hr.euler_yxz_to_mat(ypr)).max() < 1e-15


def test_the_three_overlays():
    F = 4
    boxes = np.array([[10, 20, 31, 41.0]] * F)
    ypr = np.array([[0, 0, 0.0], [90, 0, 0], [0, 0, 90], [np.nan, 0, 0]])
    prims, off = ov.head_pose_overlay(ypr, boxes, axis_length=20).build_host()
    text = "Yaw: 0.00, Pitch: 0.00, Roll: 0.00"
    assert off.tolist() == [0, 9 + len(text), 2 * (9 + len(text)) - 0 + 1, 3 * (9 + len(text)) + 2, 3 * (9 + len(text)) + 2]
    cx, cy = 10 + 31 // 2, 20 + 41 // 2
    shafts = prims[off[0]:off[1]][[0, 3, 6]]
    assert (shafts[:, 1:3] == [ov.fixed(cx), ov.fixed(cy)]).all()
    assert shafts[:, 3:5].tolist() == [[ov.fixed(cx + 20), ov.fixed(cy)], [ov.fixed(cx), ov.fixed(cy + 20)], [ov.fixed(cx), ov.fixed(cy)]]
    assert [int(w) & 0xFFFFFF for w in shafts[:, 7]] == [255, 255 << 8, 255 << 16]                    # X red, Y green, Z blue
    yaw90 = prims[off[1]:off[2]][[0, 6]]                       # R = Ry(90): X goes to -Z (a point), Z goes to +X
    assert yaw90[0, 3:5].tolist() == [ov.fixed(cx), ov.fixed(cy)] and yaw90[1, 3:5].tolist() == [ov.fixed(cx + 20), ov.fixed(cy)]
    glyphs = prims[off[0] + 9:off[1]]
    assert "".join(chr(32 + g) for g in glyphs[:, 4]) == text
    assert glyphs[0, 1] == ov.fixed(10) - 8 and glyphs[0, 2] == ov.fixed(20 - 10) + 8 - 7 * 32
    b = boxes.copy()
    b[2] = np.nan
    prims, off = ov.box_overlay(b).build_host()
    assert off.tolist() == [0, 1, 2, 2, 3] and prims[0].tolist()[:7] == [ov.KIND_BOX, 160, 320, 16 * 41 + 16, 16 * 61 + 16, 0, 32]
    assert int(prims[0, 7]) & 0xFFFFFF == 255 << 8
    pts = np.random.default_rng(3).uniform(0, 50, (F, 5, 3))
    pts[1, 2, 0] = np.nan
    prims, off = ov.landmark_overlay(pts).build_host()
    assert off.tolist() == [0, 5, 9, 14, 19] and (prims[:, 5] == 24).all() and (prims[:, 0] == ov.KIND_DISC).all()
    assert prims[0, 1:3].tolist() == ov.fixed(pts[0, 0, :2]).tolist() and int(prims[0, 7]) & 0xFFFFFF == 255 | 255 << 8


def test_the_command_line_parses():
    a = ov.build_parser().parse_args(["--frames", "clip.avi", "--out", "o.avi", "--landmarks", "lm.npy", "--samples", "1"])
    assert a.samples == 1 and a.boxes is None and a.quality == 90
    with pytest.raises(SystemExit):
        ov.build_parser().parse_args(["--frames", "clip.avi", "--out", "o.avi", "--samples", "4"])
    assert os.path.basename(ov.__file__) == "overlay.py"
