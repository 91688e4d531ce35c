"""Overlays on the MI355X: `ops.draw_overlay` against the numpy restatement of tests/overlay_ref.py, byte for byte:
frame sizes around the tile's edges, record counts around the chunk's, empty ranges, the 128-bit comparison, records at and beyond
the limits, strided frames, in place and out of place, the C ABI's refusals and clamps, and the overlays built on it end to end."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import overlay_ref as R
from msmd_amd import _lib, ops, synth
from msmd_amd.utils import media, overlay as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TW, TH = ops.OVERLAY_TILE_W, ops.OVERLAY_TILE_H
WIDTHS, HEIGHTS = (1, TW - 1, TW, TW + 1, 2 * TW + 3), (1, TH - 1, TH, TH + 1, 2 * TH + 1)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared inputs are read-only arrays


@functools.lru_cache(maxsize=None)
def random_font(n=40):
    f = np.random.default_rng(11).integers(0, 256, (n, 8), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def content(N, H, W, C, tag=0):
    a = np.random.default_rng([N, H, W, C, tag]).integers(0, 256, (N, H, W, C), dtype=np.uint8)
    a.setflags(write=False)
    return a


def mixed_records(seed, H, W, n, n_glyphs):
    """A seeded mix of the four kinds around an (H, W) frame: centres up to 24 px outside it, so that records straddle the frame's
    edges and some lie wholly outside; every fourth record sits on a tile edge; padding records in between."""
    g = np.random.default_rng(seed)
    recs = []
    for k in range(n):
        kind = (R.DISC, R.CAPSULE, R.BOX, R.GLYPH, R.NONE)[k % 5]
        x, y = int(g.integers(-24 * 16, (W + 24) * 16)), int(g.integers(-24 * 16, (H + 24) * 16))
        if k % 4 == 0:
            x, y = 16 * TW * int(g.integers(0, 3)) + int(g.integers(-20, 20)), 16 * TH * int(g.integers(0, 3)) + int(g.integers(-20, 20))
        colour = tuple(int(v) for v in g.integers(0, 256, 3)) + (int(g.choice([255, 255, 128, 31, 0])),)
        if kind == R.DISC:
            r = int(g.integers(0, 12 * 16))
            recs.append(R.record(kind, x, y, 0, 0, r, int(g.integers(0, r + 1)) * int(g.integers(0, 2)), colour))
        elif kind == R.CAPSULE:
            recs.append(R.record(kind, x, y, x + int(g.integers(-60 * 16, 60 * 16)), y + int(g.integers(-30 * 16, 30 * 16)),
                                 int(g.integers(0, 3 * 16)), 0, colour))
        elif kind == R.BOX:
            recs.append(R.record(kind, x, y, x + int(g.integers(-16, 40 * 16)), y + int(g.integers(-16, 20 * 16)), 0,
                                 int(g.integers(0, 40)) * int(g.integers(0, 2)), colour))
        elif kind == R.GLYPH:
            recs.append(R.record(kind, x, y, int(g.integers(1, 49)), int(g.integers(0, n_glyphs)), 0, 0, colour))
        else:
            recs.append(R.record(kind, x, y, 7, 7, 7, 7, colour))
    return np.stack(recs)


def run(frames, prims, offsets, font=None, samples=16, out=None):
    """ops.draw_overlay on a device copy of host arrays -> the drawn frames on the host."""
    f = dev(frames)
    got = ops.draw_overlay(f, dev(prims), dev(np.asarray(offsets, np.int32)), None if font is None else dev(font), samples,
                           out=out)
    assert got is (f if out is None else out)
    return got.cpu().numpy()


@pytest.mark.parametrize("samples", (1, 16))
@pytest.mark.parametrize("C", (1, 3, 4))
def test_frame_sizes(C, samples):
    font = random_font()
    for H in HEIGHTS:
        for W in WIDTHS:
            frames = content(2, H, W, C)
            prims = mixed_records([H, W, C], H, W, 30, font.shape[0])
            offsets = [0, 17, 30]
            ref = R.draw(frames, prims, offsets, font, samples)
            assert np.array_equal(run(frames, prims, offsets, font, samples), ref), (H, W)
            if C == 4:
                assert np.array_equal(ref[..., 3], frames[..., 3])
    assert not np.array_equal(ref, frames)


def test_chunk_edges():
    """0, 1, CHUNK - 1, CHUNK, CHUNK + 1 and 600 translucent discs per frame, every one touching the first tile, in one batch: the
    order of a frame's list survives the compaction and the chunk boundaries."""
    counts = (0, 1, ops.OVERLAY_CHUNK - 1, ops.OVERLAY_CHUNK, ops.OVERLAY_CHUNK + 1, 600)
    H, W = TH + 1, TW + 1
    g = np.random.default_rng(4)
    n = sum(counts)
    prims = np.zeros((n, 8), np.int32)
    prims[:, 0] = R.DISC
    prims[:, 1], prims[:, 2] = g.integers(0, 16 * TW, n), g.integers(0, 16 * TH, n)
    prims[:, 5] = g.integers(8, 8 * 16, n)
    prims[:, 7] = (g.integers(0, 1 << 24, n) | (g.integers(60, 200, n) << 24)).astype(np.uint32).view(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    for C, samples in ((3, 16), (1, 1)):
        frames = content(len(counts), H, W, C)
        ref = R.draw(frames, prims, offsets, None, samples)
        assert np.array_equal(run(frames, prims, offsets, None, samples), ref), (C, samples)
        assert np.array_equal(ref[0], frames[0])
        assert not np.array_equal(ref[3], R.draw(frames[3:4], prims[offsets[3]:offsets[4]][::-1], [0, counts[3]], None, samples)[0])


def test_empty_ranges_and_a_frame_alone():
    H, W, C = TH + 5, TW + 9, 3
    font = np.array(ov.FONT)
    frames = content(8, H, W, C)
    per = [mixed_records([n, 77], H, W, 12, 95) for n in range(8)]
    per[1] = per[1][:0]                                                  # the middle frame of the first three: an empty range
    offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in per])])
    prims = np.concatenate(per)
    three = run(frames[:3], prims[:offsets[3]], offsets[:4], font)
    assert np.array_equal(three, R.draw(frames[:3], prims, offsets[:4], font)) and np.array_equal(three[1], frames[1])
    eight = run(frames, prims, offsets, font)
    assert np.array_equal(eight[:3], three)
    for n in (0, 5, 7):
        alone = run(frames[n:n + 1], per[n], [0, per[n].shape[0]], font)
        assert np.array_equal(alone[0], eight[n]), n
    assert not np.array_equal(eight[5], frames[5])
    assert run(frames[:0], prims, [0], font).shape == (0, H, W, C)      # an empty batch


def test_the_128_bit_comparison():
    """(q x d)^2 reaches 2^86: a product wrapped to 64 bits decides 64 360 of these sample points differently."""
    frames = np.zeros((1, 2, 4096, 1), np.uint8)
    prims = R.record(R.CAPSULE, 37, -2 ** 20 + 5, -11, 2 ** 20 - 3, 40, 0, (255, 255, 255, 255))[None]
    ref = R.draw(frames, prims, [0, 1])
    assert int((ref > 0).sum()) > 0 and R.coverage(prims[0], 2, 4096, 16, None).sum() == 104
    assert np.array_equal(run(frames, prims, [0, 1]), ref)
    # r = 2^15: r^2 L needs 72 bits; the capsule's edge crosses the frame
    frames = content(1, 2, 2048, 3)
    prims = R.record(R.CAPSULE, 16384 - 32768 + 3, -2 ** 20 + 1, 16384 - 32768 - 40, 2 ** 20 - 7, 1 << 15, 0, (250, 10, 90, 200))[None]
    cov = R.coverage(prims[0], 2, 2048, 16, None)
    assert 0 < (cov == 16).sum() < cov.size and ((cov > 0) & (cov < 16)).any()
    for samples in (1, 16):
        assert np.array_equal(run(frames, prims, [0, 1], None, samples), R.draw(frames, prims, [0, 1], None, samples))


@pytest.mark.parametrize("font_name", ("random", "FONT"))
def test_records_at_and_beyond_the_limits(font_name):
    font = random_font() if font_name == "random" else np.array(ov.FONT)
    G, MC, MR = font.shape[0], ops.OVERLAY_MAX_COORD, ops.OVERLAY_MAX_RADIUS
    H, W = TH + 3, TW + 3
    c = lambda k: (40 * k % 256, 255 - 30 * k % 256, 90, 160)
    at = [R.record(R.CAPSULE, -MC, 40, MC, 200, 30, 0, c(1)), R.record(R.BOX, -MC, -MC, MC, MC, 0, MR, c(2)),
          R.record(R.BOX, 100, 50, MC, MC, 0, 0, c(3)), R.record(R.DISC, 500, 130, MC, -MC, MR, MR - 300, c(4)),
          R.record(R.DISC, 300, 100, 0, 0, MR, 0, c(5)), R.record(R.GLYPH, 10, 10, MR, G - 1, 0, 0, c(6)),
          R.record(R.GLYPH, 200, 30, 20, G - 1, MR, MR, c(7)), R.record(R.GLYPH, 400, 60, 17, 0, 0, 0, c(8)),
          R.record(R.CAPSULE, 10, -MC, 900, MC, MR, 0, c(9))]
    beyond = [R.record(R.CAPSULE, -MC - 1, 40, MC, 200, 30, 0, c(1)), R.record(R.CAPSULE, -MC, 40, MC + 1, 200, 30, 0, c(1)),
              R.record(R.BOX, 100, 50, MC, MC + 1, 0, 0, c(3)), R.record(R.BOX, 100, -MC - 1, MC, MC, 0, 0, c(3)),
              R.record(R.DISC, 300, 100, 0, 0, MR + 1, 0, c(5)), R.record(R.DISC, 300, 100, 0, 0, 50, MR + 1, c(5)),
              R.record(R.DISC, 300, 100, 0, 0, -1, 0, c(5)), R.record(R.DISC, 300, 100, 0, 0, 50, -1, c(5)),
              R.record(R.DISC, 300, 100, MC + 1, 0, 50, 0, c(5)), R.record(5, 300, 100, 400, 200, 50, 0, c(5)),
              R.record(-1, 300, 100, 400, 200, 50, 0, c(5)), R.record(R.GLYPH, 10, 10, 32, G, 0, 0, c(6)),
              R.record(R.GLYPH, 10, 10, 32, -1, 0, 0, c(6)), R.record(R.GLYPH, 10, 10, 0, 1, 0, 0, c(6)),
              R.record(R.GLYPH, 10, 10, MR + 1, 1, 0, 0, c(6)), R.record(R.GLYPH, 10, 10, -5, 1, 0, 0, c(6)),
              R.record(R.GLYPH, 10, 10, 32, 1, MR + 1, 0, c(6)), R.record(R.NONE, 10, 10, 100, 100, 50, 0, c(6)),
              R.record(-2 ** 31, 10, 10, 100, 100, 50, 0, c(6)), R.record(2 ** 31 - 1, 10, 10, 100, 100, 50, 0, c(6))]
    assert all(R.draws(r, G) for r in at) and not any(R.draws(r, G) for r in beyond)
    frames = content(3, H, W, 3)
    prims = np.stack(at + beyond + at[::-1])
    offsets = [0, len(at), len(at) + len(beyond), prims.shape[0]]
    for samples in (1, 16):
        got = run(frames, prims, offsets, font, samples)
        assert np.array_equal(got, R.draw(frames, prims, offsets, font, samples)), samples
        assert np.array_equal(got[1], frames[1]) and not np.array_equal(got[0], frames[0]) and not np.array_equal(got[0], got[2])
    # without a font no glyph draws, and nothing is read
    no_font = run(frames, prims, offsets, None, 16)
    assert np.array_equal(no_font, R.draw(frames, prims, offsets, None, 16)) and not np.array_equal(no_font, got)


def test_strided_frames():
    """A panel cut out of a wider frame at an odd base address equals the drawing on a contiguous copy, and the bytes around the
    panel stay; so do a panel at a 4-byte aligned address whose width is no multiple of four (whole words and a ragged end in one
    row) and the RGB view of an RGBA buffer."""
    N, H, W, Hp, Wp = 2, 40, 152, TH + 7, TW + 6
    font = np.array(ov.FONT)
    for C in (1, 3, 4):
        wide = content(N, H, W, C, tag=1)
        prims = mixed_records([C, 5], Hp, Wp, 24, 95)
        offsets = [0, 11, 24]
        for samples in (1, 16):
            buf = torch.zeros(wide.size + 4, dtype=torch.uint8, device=DEV)
            for off in ((0, 1, 3) if C == 4 else (0, 1, 2)):
                col = 8 if off == 0 else 5 if (off + (3 * W + 5) * C) % 2 == 1 else 6
                buf.zero_()
                whole = buf[off:off + wide.size].view(N, H, W, C)
                whole.copy_(dev(wide))
                panel = whole[:, 3:3 + Hp, col:col + Wp]
                assert panel.data_ptr() % 4 == 0 if off == 0 else panel.data_ptr() % 2 == 1
                assert not panel.is_contiguous()
                ref = R.draw(np.ascontiguousarray(wide[:, 3:3 + Hp, col:col + Wp]), prims, offsets, font, samples)
                assert ops.draw_overlay(panel, dev(prims), dev(np.asarray(offsets, np.int32)), dev(font), samples) is panel
                want = wide.copy()
                want[:, 3:3 + Hp, col:col + Wp] = ref
                assert np.array_equal(whole.cpu().numpy(), want), (C, samples, off)
                assert int(buf[:off].sum()) == 0 and int(buf[off + wide.size:].sum()) == 0
    rgba = content(N, Hp, Wp, 4, tag=2)
    prims = mixed_records([9, 9], Hp, Wp, 24, 95)
    t = dev(rgba)
    ops.draw_overlay(t[..., :3], dev(prims), dev(np.asarray([0, 11, 24], np.int32)), dev(font))
    want = rgba.copy()
    want[..., :3] = R.draw(np.ascontiguousarray(rgba[..., :3]), prims, [0, 11, 24], font)
    assert np.array_equal(t.cpu().numpy(), want)


def test_in_place_and_out_of_place():
    N, H, W = 2, 3 * TH + 2, 3 * TW + 5                     # nine tiles and a fringe; most of them untouched
    for C in (1, 3, 4):
        frames = content(N, H, W, C, tag=3)
        prims = np.stack([R.record(R.DISC, 16 * TW + 40, 16 * TH + 9, 0, 0, 100, 0, (255, 0, 80, 200)),
                          R.record(R.GLYPH, 16 * (2 * TW + 60), 16 * (2 * TH + 10), 24, 33, 0, 0, (0, 255, 0, 255))])
        offsets = [0, 1, 2]
        ref = R.draw(frames, prims, offsets, ov.FONT)
        assert np.array_equal(run(frames, prims, offsets, ov.FONT), ref)
        src = dev(frames)
        out = torch.full((N, H, W, C), 7, dtype=torch.uint8, device=DEV)
        got = run(frames, prims, offsets, ov.FONT, out=out)
        want = ref.copy()
        if C == 4:
            want[..., 3] = 7                              # the fourth byte is neither read nor written
        assert np.array_equal(got, want) and np.array_equal(src.cpu().numpy(), frames), C
        with pytest.raises(TypeError):
            ops.draw_overlay(src, dev(prims), dev(np.asarray(offsets, np.int32)), out=out[:, :, :W - 1])
    with pytest.raises(ValueError):
        ops.draw_overlay(src, dev(prims), dev(np.asarray(offsets, np.int32)), samples=4)
    with pytest.raises(TypeError):
        ops.draw_overlay(src, dev(prims).long(), dev(np.asarray(offsets, np.int32)))
    with pytest.raises(TypeError):
        ops.draw_overlay(src, dev(prims), dev(np.asarray(offsets[:2], np.int32)))
    with pytest.raises(RuntimeError):
        ops.draw_overlay(src, dev(prims).cpu(), dev(np.asarray(offsets, np.int32)))


def _abi(src, dst, N, H, W, C, prims, n_prims, offsets, font, n_glyphs, samples, frame_stride=None, row_stride=None, pixel_stride=None):
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    ps = C if pixel_stride is None else pixel_stride
    rs = W * ps if row_stride is None else row_stride
    fs = H * rs if frame_stride is None else frame_stride
    code = _lib.load().msmd_draw_overlay(p(src), p(dst), fs, rs, ps, N, H, W, C, p(prims), n_prims, p(offsets), p(font), n_glyphs,
                                         samples, None)
    torch.cuda.synchronize()
    return code


def test_c_abi_refusals_and_clamps():
    N, H, W, C = 2, TH + 1, TW + 2, 3
    frames = content(N, H, W, C, tag=4)
    host = mixed_records([1, 2, 3], H, W, 20, 95)
    src, prims, font = dev(frames), dev(host), dev(ov.FONT)
    offsets = dev(np.array([0, 9, 20], np.int32))
    fresh = lambda: torch.full((N, H, W, C), 7, dtype=torch.uint8, device=DEV)
    base = dict(src=src, N=N, H=H, W=W, C=C, prims=prims, n_prims=20, offsets=offsets, font=font, n_glyphs=95, samples=16)
    dst = fresh()
    assert _abi(dst=dst, **base) == 0 and np.array_equal(dst.cpu().numpy(), R.draw(frames, host, [0, 9, 20], ov.FONT))
    dst = fresh()
    refused = [dict(N=-1), dict(n_prims=-1), dict(C=2), dict(C=5), dict(C=0), dict(pixel_stride=4, C=1), dict(pixel_stride=2),
               dict(H=0), dict(W=0), dict(H=ops.JPEG_MAX_SIDE + 1), dict(W=-3), dict(row_stride=W * C - 1),
               dict(frame_stride=H * W * C - 1), dict(row_stride=-W * C), dict(samples=0), dict(samples=4), dict(samples=17),
               dict(n_glyphs=-1), dict(src=None), dict(offsets=None), dict(prims=None), dict(font=None)]
    for kw in refused:
        args = dict(base, dst=dst)
        args.update(kw)
        assert _abi(**args) == 1, kw
        assert int(dst.min()) == 7 and int(dst.max()) == 7, kw
    assert _abi(**dict(base, dst=None)) == 1
    # no work: no pointer is looked at
    assert _abi(None, None, 0, H, W, C, None, 20, None, None, 95, 16) == 0
    # what need not exist when it is not used: prims without records, a font without glyphs
    assert _abi(**dict(base, dst=dst, prims=None, n_prims=0, font=None, n_glyphs=0)) == 0
    assert np.array_equal(dst.cpu().numpy(), frames)
    # prim_offsets that descend or run past the table: clamped into [0, P], the end no less than the begin
    for wild in ([15, 4, 20], [-7, 12, 2 ** 31 - 1], [30, 40, -5], [-2 ** 31, 20, 3]):
        dst = fresh()
        assert _abi(**dict(base, dst=dst, offsets=dev(np.array(wild, np.int32)))) == 0
        b, e = R.clamp_offsets(wild, 20)
        assert (b[0] <= b[1] <= 20) and (e[0] <= e[1] <= 20)
        assert np.array_equal(dst.cpu().numpy(), R.draw(frames, host, wild, ov.FONT)), wild


def _clip():
    """A synthetic 96 x 80 clip of six frames with its tracks: boxes, head angles, landmarks (one missing)."""
    F, H, W = 6, 80, 96
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([2 * xx, 128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0), 3 * yy], -1)
    frames = np.clip(img[None] + 12 * np.arange(F)[:, None, None, None], 0, 255).astype(np.uint8)
    boxes = np.array([[20 + f, 22 + f // 2, 50, 40] for f in range(F)], np.float64)
    ypr = np.array([[10.0 * f - 20, 5.0 * f, -8.0 * f] for f in range(F)])
    g = np.random.default_rng(8)
    points = boxes[:, None, :2] + g.uniform(0, 1, (F, 30, 2)) * boxes[:, None, 2:]
    points[2, 4] = np.nan
    return frames, boxes, ypr, points


def test_end_to_end_overlays_to_a_video(tmp_path):
    frames, boxes, ypr, points = _clip()
    F, H, W, _ = frames.shape
    o = ov.box_overlay(boxes)
    ov.head_pose_overlay(ypr, boxes, axis_length=30, into=o)
    ov.landmark_overlay(points, into=o)
    prims, offsets = o.build_host()
    assert offsets[-1] == F * (1 + 9 + 30) - 1 + sum(len(f"Yaw: {a:.2f}, Pitch: {b:.2f}, Roll: {c:.2f}") for a, b, c in ypr)
    for samples in (16, 1):
        ref = R.draw(frames, prims, offsets, ov.FONT, samples)
        t = dev(frames)
        assert o.draw(t, samples=samples) is t and np.array_equal(t.cpu().numpy(), ref), samples
        out = torch.empty_like(t)
        assert o.draw(dev(frames), samples=samples, out=out) is out and torch.equal(out, t)
    assert (ref != frames).any(-1).mean() > 0.03                       # the drawing is there: boxes, arrows, text and dots
    with pytest.raises(ValueError):
        o.draw(t[:5])
    path = tmp_path / "overlay.avi"
    media.write_avi(path, media.encode_jpeg(dev(ref), 90), 25, (W, H))
    back = media.read_video(path)
    assert tuple(back.shape) == (F, H, W, 3) and media.read_avi(path).fps == 25
    assert float((back.float() - dev(ref).float()).abs().mean()) < 6.0
    # the command line, on the same clip and tracks
    import pickle as pkl
    from msmd_amd.utils import head_pose
    np.save(tmp_path / "frames.npy", frames)
    np.save(tmp_path / "lm.npy", points)
    with open(tmp_path / "boxes.pickle", "wb") as f:
        pkl.dump({"processed_bbox_frames": [list(map(int, b)) for b in boxes], "fps": 30}, f)
    head_pose.save_head_rot(str(tmp_path / "rot.pickle"), ypr)
    ov.main(["--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "cli.avi"), "--boxes", str(tmp_path / "boxes.pickle"),
             "--landmarks", str(tmp_path / "lm.npy"), "--head_rot", str(tmp_path / "rot.pickle"), "--chunk", "4"])
    cli = media.read_video(tmp_path / "cli.avi")
    assert tuple(cli.shape) == (F, H, W, 3) and media.read_avi(tmp_path / "cli.avi").fps == 30
    o2 = ov.box_overlay(boxes)
    ov.landmark_overlay(points, into=o2)
    ov.head_pose_overlay(ypr, boxes, into=o2)
    want = media.decode_jpeg(media.encode_jpeg(o2.draw(dev(frames)), 90))
    assert torch.equal(cli, want)


def test_legend_labels():
    from msmd_amd.utils import metrics as M
    from msmd_amd.utils.renderer import MeshRenderer
    v, f = synth.latlong_sphere(7, 16, 0.09)
    n, W, H = 3, 128, 144
    g = np.random.default_rng(3)
    gt = dev(np.stack([v * np.float32(1.0 + 0.02 * b) for b in range(n)]))
    pred = gt + dev((0.004 * g.standard_normal((n,) + v.shape)).astype(np.float32))
    r = MeshRenderer((W, H))
    plain = M.render_comparison(pred, gt, f, r, 0.01)
    assert torch.equal(plain, M.render_comparison(pred, gt, f, r, 0.01, legend_labels=None))
    labels = ("0", "10.0 mm")
    out = M.render_comparison(pred, gt, f, r, 0.01, legend_labels=labels)
    assert out.shape == plain.shape and not torch.equal(out, plain)
    inside = torch.zeros(H, 3 * W, dtype=torch.bool, device=DEV)
    for x0, y0, x1, y1 in M.legend_label_boxes(H, W, labels):
        assert 0 <= x0 < x1 <= W - max(4, W // 32) and 0 <= y0 < y1 <= H
        inside[y0:y1, 2 * W + x0:2 * W + x1] = True
    changed = (out != plain).any(-1)
    assert not bool((changed & ~inside[None]).any()) and int(changed[0].sum()) > 20
    assert bool(changed[:, :H // 2].any()) and bool(changed[:, H // 2:].any())          # both ends of the bar are labelled
    # the text is the overlay's: black ink (the renderer's background is white) of the restatement, on the error panel alone
    ref_panel = plain[:, :, 2 * W:].cpu().numpy()
    o = ov.Overlay(n)
    for s, at, scale in M.legend_label_layout(H, W, labels):
        o.text([s] * n, np.tile(np.asarray(at, np.float64), (n, 1)), (0, 0, 0), scale=scale)
    assert np.array_equal(out[:, :, 2 * W:].cpu().numpy(), R.draw(ref_panel, *o.build_host(), ov.FONT))
    dark = M.render_comparison(pred, gt, f, MeshRenderer((W, H), black_bg=True), 0.01, legend_labels=labels)[:, :, 2 * W:]
    x0, y0, x1, y1 = M.legend_label_boxes(H, W, labels)[0]
    assert int(dark[:, y0:y1, x0:x1].max()) == 255 and int(out[:, y0:y1, 2 * W + x0:2 * W + x1].min()) == 0
    with pytest.raises(ValueError):
        M.render_comparison(pred, gt, f, r, 0.01, legend_labels=("mm",))
