"""Frame resizing on the MI355X: `ops.resize_frames` in both forms against the numpy restatement of
tests/resize_ref.py (and against Pillow where it is importable), byte for byte: sizes around the fused tile's edges, every filter
and channel count, sources at any alignment, boxes, the C ABI's refusals and clamps, and the media helpers built on it."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resize_ref as rr
from msmd_amd import _lib, ops
from msmd_amd.utils import media

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, TW = ops.RESIZE_TILE_H, ops.RESIZE_TILE_W
# (Hs, Ws, Hd, Wd): down on both axes onto tile - 1, tile, tile + 1 and 1; up on both; each axis alone, up and down; mixed; odd
SHAPES = [(40, 150, TH - 1, TW - 1), (40, 150, TH, TW), (40, 150, TH + 1, TW + 1), (40, 150, 1, 1), (9, 30, TH + 1, TW + 1),
          (20, 50, 20, 2 * TW + 1), (20, 50, 2 * TH + 1, 50), (40, 150, 40, TW - 1), (40, 150, TH - 1, 150), (10, 150, 31, 33),
          (21, 33, 17, 35)]
try:
    from PIL import Image
    PIL_FILTER = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
                  "lanczos": Image.Resampling.LANCZOS}
except ImportError:
    Image = None


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared inputs are read-only arrays


@functools.lru_cache(maxsize=None)
def source(N, H, W, C, kind="random"):
    a = rr.content(kind, (N, H, W, C), "resize_gpu")
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(N, H, W, C, Hd, Wd, f, kind="random"):
    """The restatement on a case's frames, computed once and never modified."""
    out = rr.resize_frames(source(N, H, W, C, kind), (Wd, Hd), f)
    out.setflags(write=False)
    return out


def fits(H, Hd, C, f):
    b, c = ops._resize_axis(H, Hd, f, 0.0, float(H))
    return ops.resize_fits(C, ops.resize_rows_span(b[None], H, c.shape[1]))


def both_forms(frames, size, f, H, C, box=None):
    """`resize_frames` in every form the shape admits -> {form: bytes on the host}."""
    out = {"auto": ops.resize_frames(frames, size, f, box=box).cpu().numpy(),
           "two_pass": ops.resize_frames(frames, size, f, box=box, form="two_pass").cpu().numpy()}
    if box is None and fits(H, size[1], C, f):
        out["fused"] = ops.resize_frames(frames, size, f, form="fused").cpu().numpy()
    return out


@pytest.mark.parametrize("f", rr.FILTERS)
def test_bytes_equal_the_restatement(f):
    n_fused = 0
    for Hs, Ws, Hd, Wd in SHAPES:
        for C in (1, 3, 4):
            ref = reference(3, Hs, Ws, C, Hd, Wd, f)
            for N in (1, 3):
                got = both_forms(dev(source(3, Hs, Ws, C)[:N]), (Wd, Hd), f, Hs, C)
                n_fused += "fused" in got
                for form, g in got.items():
                    assert g.shape == (N, Hd, Wd, C) and np.array_equal(g, ref[:N]), (Hs, Ws, Hd, Wd, C, N, form)
            if Image is not None:
                a = source(3, Hs, Ws, C)[0]
                im = Image.fromarray(a[:, :, 0] if C == 1 else a, {1: "L", 3: "RGB", 4: "CMYK"}[C])
                pil = np.asarray(im.resize((Wd, Hd), PIL_FILTER[f], reducing_gap=None)).reshape(Hd, Wd, C)
                assert np.array_equal(ref[0], pil), (Hs, Ws, Hd, Wd, C)
    assert n_fused == 2 * 3 * len(SHAPES)          # every one of these shapes fits the fused form


def test_sources_at_any_alignment():
    """Odd widths with three channels, a source that starts 1, 2 and 3 bytes into a buffer, a row stride above the row, the RGB view
    of an RGBA buffer, and a destination that starts off a word."""
    Hs, Ws, Hd, Wd, f = 21, 33, 17, 36, "bicubic"
    for C in (1, 3, 4):
        a = source(3, Hs, Ws, C)
        ref = reference(3, Hs, Ws, C, Hd, Wd, f)
        for off in (1, 2, 3):
            buf = torch.zeros(a.size + 8, dtype=torch.uint8, device=DEV)
            buf[off:off + a.size] = dev(a).reshape(-1)
            frames = buf[off:off + a.size].view(3, Hs, Ws, C)
            assert frames.data_ptr() % 4 == off
            for form, g in both_forms(frames, (Wd, Hd), f, Hs, C).items():
                assert np.array_equal(g, ref), (C, off, form)
            for form in (None, "two_pass"):
                obuf = torch.full((ref.size + 8,), 7, dtype=torch.uint8, device=DEV)
                out = obuf[off:off + ref.size].view(ref.shape)
                assert ops.resize_frames(frames, (Wd, Hd), f, out=out, form=form) is out
                assert np.array_equal(out.cpu().numpy(), ref) and int(obuf[:off].min()) == 7 and int(obuf[off + ref.size:].min()) == 7
        wide = torch.zeros(3, Hs, Ws + 5, C, dtype=torch.uint8, device=DEV)
        wide[:, :, :Ws] = dev(a)
        for form, g in both_forms(wide[:, :, :Ws], (Wd, Hd), f, Hs, C).items():
            assert np.array_equal(g, ref), (C, "row stride", form)
    rgba = dev(source(3, Hs, Ws, 4))
    ref = rr.resize_frames(source(3, Hs, Ws, 4)[..., :3], (Wd, Hd), f)
    for form, g in both_forms(rgba[..., :3], (Wd, Hd), f, Hs, 3).items():
        assert np.array_equal(g, ref), ("RGB view of RGBA", form)


def test_a_reduction_that_does_not_fit_takes_the_two_pass_form():
    Hs, Ws, Hd, Wd, f = 600, 9, 2, 5, "lanczos"
    assert not fits(Hs, Hd, 3, f)
    frames = dev(source(2, Hs, Ws, 3))
    assert np.array_equal(ops.resize_frames(frames, (Wd, Hd), f).cpu().numpy(), reference(2, Hs, Ws, 3, Hd, Wd, f))
    with pytest.raises(ValueError):
        ops.resize_frames(frames, (Wd, Hd), f, form="fused")
    assert ops.resize_frames(frames[:0], (Wd, Hd), f).shape == (0, Hd, Wd, 3)      # an empty batch on the routed two-pass form


@pytest.mark.parametrize("kind", ["zeros", "full", "checker", "random"])
def test_content(kind):
    Hs, Ws = 24, 40
    for Hd, Wd in ((50, 90), (11, 19)):
        for f in rr.FILTERS:
            for C in (1, 3):
                ref = reference(2, Hs, Ws, C, Hd, Wd, f, kind)
                if kind in ("zeros", "full"):
                    assert (ref == (255 if kind == "full" else 0)).all()
                for form, g in both_forms(dev(source(2, Hs, Ws, C, kind)), (Wd, Hd), f, Hs, C).items():
                    assert np.array_equal(g, ref), (kind, Hd, Wd, f, C, form)
    if kind == "checker":       # the negative lobes overshoot on both sides: the clip is exercised
        raw = rr.pass_axis0(source(1, Hs, Ws, 1, kind)[0], *rr.tables(Hs, 50, "lanczos"), raw=True) >> rr.P
        assert raw.min() < 0 and raw.max() > 255


def test_boxes():
    Hs, Ws, Hd, Wd, N = 30, 44, 17, 23, 3
    a = source(N, Hs, Ws, 3)
    frames = dev(a)
    one, frac = (3, 2, 40, 29), (0.25, 1.5, 40.75, 28.5)
    per_frame = [one, (10, 5, 30, 20), one]                     # frames 0 and 2 share a table
    for f in ("bilinear", "lanczos"):
        for box in (one, frac, per_frame):
            ref = rr.resize_frames(a, (Wd, Hd), f, box)
            for form in (None, "fused", "two_pass"):
                got = ops.resize_frames(frames, (Wd, Hd), f, box=box, form=form)
                assert np.array_equal(got.cpu().numpy(), ref), (f, box, form)
    # a frame's bytes depend on its own pixels and box alone, and a second run gives the same bytes
    three = [one, frac, (10, 5, 30, 20)]
    batch = ops.resize_frames(frames, (Wd, Hd), "bicubic", box=three)
    for n in range(N):
        alone = ops.resize_frames(frames[n:n + 1], (Wd, Hd), "bicubic", box=three[n])
        assert torch.equal(alone[0], batch[n])
    assert torch.equal(batch, ops.resize_frames(frames, (Wd, Hd), "bicubic", box=three))
    for bad in [(0, 0, 45, 30), (5, 5, 5, 9), (-1, 0, 4, 4), (0, 0, 44, 30.5), [(0, 0, 4, 4)] * 2]:
        with pytest.raises(ValueError):
            ops.resize_frames(frames, (Wd, Hd), "bilinear", box=bad)
    for kw in [dict(size=(0, 4)), dict(size=(4, 0)), dict(size=(4, 4), filter="nearest"), dict(size=(4, 4), form="fast")]:
        with pytest.raises(ValueError):
            ops.resize_frames(frames, **kw)


def _abi(src, N, Hs, Ws, C, tabs, tof, dst, Hd, Wd, ws, span, form, pixel_stride=None):
    xb, xc, yb, yc = tabs
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    ps = C if pixel_stride is None else pixel_stride
    code = _lib.load().msmd_resize_u8(p(src), Hs * Ws * ps, Ws * ps, ps, N, Hs, Ws, C, p(xb), p(xc), xc.shape[2], xb.shape[0], p(yb), p(yc),
                                      yc.shape[2], yb.shape[0], p(tof), p(dst), Hd, Wd, p(ws), span, form, None)
    torch.cuda.synchronize()
    return code


def test_c_abi_refusals_and_clamps():
    Hs, Ws, Hd, Wd, C, N, f = 20, 31, 9, 14, 3, 2, "bicubic"
    a = source(N, Hs, Ws, C)
    src = dev(a)
    host = [t[None].copy() for t in ops.resize_tables(Ws, Wd, f) + ops.resize_tables(Hs, Hd, f)]
    tabs = [dev(t) for t in host]
    span = ops.resize_rows_span(host[2], Hs, host[3].shape[2])
    tof = torch.zeros(N, dtype=torch.int32, device=DEV)
    ws = torch.empty(N * Hs * Wd * C, dtype=torch.uint8, device=DEV)
    fresh = lambda: torch.full((N, Hd, Wd, C), 7, dtype=torch.uint8, device=DEV)
    for form in (ops.RESIZE_FUSED, ops.RESIZE_TWO_PASS, ops.RESIZE_AUTO):
        dst = fresh()
        assert _abi(src, N, Hs, Ws, C, tabs, tof, dst, Hd, Wd, ws, span, form) == 0
        assert np.array_equal(dst.cpu().numpy(), reference(N, Hs, Ws, C, Hd, Wd, f))
    dst = fresh()
    refused = [dict(Hd=0), dict(Wd=0), dict(Hs=0), dict(Ws=-3), dict(C=2), dict(C=5), dict(N=-1), dict(form=3), dict(pixel_stride=1),
               dict(span=0, form=ops.RESIZE_FUSED), dict(span=10 ** 6, form=ops.RESIZE_FUSED), dict(ws=None, form=ops.RESIZE_TWO_PASS),
               dict(src=None), dict(tof=None)]
    for kw in refused:
        args = dict(src=src, N=N, Hs=Hs, Ws=Ws, C=C, tabs=tabs, tof=tof, dst=dst, Hd=Hd, Wd=Wd, ws=ws, span=span, form=ops.RESIZE_AUTO)
        args.update(kw)
        assert _abi(**args) == 1, kw
        assert int(dst.min()) == 7 and int(dst.max()) == 7, kw
    assert _abi(src, 0, Hs, Ws, C, tabs, tof, dst, Hd, Wd, ws, span, ops.RESIZE_AUTO) == 0 and int(dst.min()) == 7 and int(dst.max()) == 7
    # an empty batch has an empty workspace too: the two-pass form returns 0 without one, forced or routed
    assert _abi(src, 0, Hs, Ws, C, tabs, tof, dst, Hd, Wd, None, span, ops.RESIZE_TWO_PASS) == 0 and int(dst.min()) == 7 and int(dst.max()) == 7
    assert _abi(src, 0, Hs, Ws, C, tabs, tof, dst, Hd, Wd, None, 0, ops.RESIZE_AUTO) == 0
    for form in (None, "fused", "two_pass"):
        assert ops.resize_frames(src[:0], (Wd, Hd), f, form=form).shape == (0, Hd, Wd, C)
    assert ops.resize_frames(src[:0], (Wd, Hd), f, box=np.zeros((0, 4))).shape == (0, Hd, Wd, C)
    # tables whose bounds point outside the source: clamped, and the bytes are the restatement's on the clamped tables
    wild = [t.copy() for t in host]
    wild[0][0, 0] = (-5, 4)
    wild[0][0, 3] = (Ws + 10, 3)
    wild[0][0, 5] = (Ws - 2, 1000)
    wild[0][0, 7] = (4, -3)
    wild[2][0, 1] = (-2 ** 31, 2 ** 31 - 1)
    wild[2][0, 4] = (Hs - 1, 6)
    wild[2][0, 8] = (2 ** 31 - 1, 2)
    tof_wild = torch.tensor([-4, 9], dtype=torch.int32, device=DEV)          # clamped into the one table there is
    xt, yt = rr.clamp_tables(wild[0][0], wild[1][0], Ws), rr.clamp_tables(wild[2][0], wild[3][0], Hs)
    ref = np.stack([rr.resize_with_tables(a[n], xt, yt) for n in range(N)])
    span = ops.resize_rows_span(wild[2], Hs, wild[3].shape[2])
    for form in ("fused", "two_pass"):
        got = ops.resize_u8(src, *[dev(t) for t in wild], tof_wild, (Hd, Wd), form=form, rows_span=span)
        assert np.array_equal(got.cpu().numpy(), ref), form


def test_read_video_side_by_side_and_the_command_line(tmp_path):
    yy, xx = np.mgrid[0:48, 0:72]
    img = np.stack([3 * xx, 128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0), 5 * yy], -1)
    frames = dev(np.clip(img[None] + 15 * np.arange(5)[:, None, None, None], 0, 255).astype(np.uint8))
    path = tmp_path / "clip.avi"
    media.combine_frames_and_audio(frames, None, 25, path)
    full = media.read_video(path)
    assert full.shape == (5, 48, 72, 3)
    for size, f in (((36, 24), "bilinear"), ((100, 31), "lanczos")):
        small = media.read_video(path, chunk=2, size=size, resample=f)
        assert torch.equal(small, ops.resize_frames(full, size, f))
        assert np.array_equal(small.cpu().numpy(), rr.resize_frames(full.cpu().numpy(), size, f))
    # two panels of different sizes at the first one's height: 33 x 21 becomes 20 x round(21 * 20 / 33) = 20 x 13
    a, b = source(2, 20, 30, 3), source(2, 33, 21, 3)
    got = media.side_by_side([dev(a), dev(b)])
    assert np.array_equal(got.cpu().numpy(), np.concatenate([a, rr.resize_frames(b, (13, 20), "bilinear")], 2))
    got = media.side_by_side([dev(a), dev(b)], height=11, resample="bicubic")
    assert np.array_equal(got.cpu().numpy(), np.concatenate([rr.resize_frames(a, (17, 11), "bicubic"), rr.resize_frames(b, (7, 11), "bicubic")], 2))
    # the inference script's source panel: the clip at the render's height, then the frames nearest in time left of a render chunk
    from msmd_amd import inference
    panel, fps = inference.load_source_panel(path, 20, DEV)
    assert fps == 25 and torch.equal(panel, ops.resize_frames(full, (30, 20), "bilinear"))      # 72 * 20 / 48 = 30
    part = dev(source(3, 20, 20, 4))                                                            # frames 2 .. 4 of a 50 fps render, RGBA
    got = inference.beside_source(part, 2, panel, fps, 50)
    assert media.frames_at(5, 50, 5, 25)[2:] == [1, 2, 2]
    assert torch.equal(got, torch.cat([panel[[1, 2, 2]], part[..., :3]], 2))
    out = tmp_path / "small.avi"
    r = subprocess.run([sys.executable, "-m", "msmd_amd.utils.media", "--resize", str(path), str(out), "--size", "40x26", "--filter", "bicubic"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    back = media.read_video(out)
    assert back.shape == (5, 26, 40, 3) and media.read_avi(out).fps == 25
