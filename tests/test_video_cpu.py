"""Host side of the video writer, no GPU: the tables against what Pillow writes, the numpy restatement of the
encoder (tests/jpeg_ref.py) against Pillow's decoder and encoder, the integer DCT against float64, the AVI writer against a
parser, the size guard and the command line."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as jr
from msmd_amd import inference, ops
from msmd_amd.utils import media

# How far below Pillow's own encoder (same tables, same quality, 4:4:4) the PSNR may lie, in dB.  Both codecs quantise the same
# DCT with the same tables and differ in how they round (libjpeg's fixed-point DCT and colour conversion, ties).  Up to quality 90
# the gap measured here is hundredths of a dB (-0.03 .. +0.07).  At quality 100 every step is 1 and the whole error (MSE ~ 0.6)
# is rounding noise, in which the two codecs differ by independent draws: -0.30 .. +0.27 dB on these images.
# 0.5 dB (12 % of the mean squared error) covers that and nothing coarser: one quantiser step of difference in a table entry
# costs more.
PSNR_MARGIN_DB = 0.5


def images():
    rng = np.random.default_rng(0)
    H, W = 72, 104
    y, x = np.mgrid[0:H, 0:W]
    g = np.clip(128 + 80 * np.sin(x / 9.0) * np.cos(y / 7.0) + rng.normal(0, 6, (H, W)), 0, 255)
    g[20:50, 30:70] = 255
    g = np.rint(g).astype(np.uint8)
    smooth = np.stack([g, np.roll(g, 3, 1), 255 - g], -1)
    noise = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    checker = np.broadcast_to((((y // 8 + x // 8) & 1) * 255).astype(np.uint8)[..., None], (H, W, 3)).copy()
    odd = smooth[:23, :37].copy()
    return {"smooth": smooth, "noise": noise, "checker": checker, "odd": odd}


def pillow_jpeg(img, q):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=0, optimize=False, restart_marker_rows=1)
    return b.getvalue()


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("q", [1, 50, 90, 100])
def test_tables_equal_what_pillow_writes(q):
    img = images()["smooth"]
    dqt, dht, dri = jr.tables_of(pillow_jpeg(img, q))
    assert dri is not None and len(dht) == 4 and len(dqt) == 2
    ours_q, ours_h, ours_ri = jr.tables_of(ops.jpeg_header(img.shape[0], img.shape[1], q) + b"")
    assert ours_q == dqt and ours_h == dht and ours_ri == ops.JPEG_RESTART_INTERVAL == jr.RI
    for tid, base in ((0, ops.JPEG_BASE_LUMA), (1, ops.JPEG_BASE_CHROMA)):
        t = ops.jpeg_quant_table(base, q)
        assert [t[n] for n in ops.JPEG_ZIGZAG] == dqt[tid]
    # the reference's own copy of the tables and its header are the same bytes
    assert jr.header(img.shape[0], img.shape[1], q) == ops.jpeg_header(img.shape[0], img.shape[1], q)
    assert list(ops.JPEG_ZIGZAG) == jr.ZZ.tolist()
    assert {(c, t): (list(b), list(v)) for c, t, b, v in ops.JPEG_HUFFMAN} == dht


def test_quality_range():
    for bad in (0, 101, -1, 50.5):
        with pytest.raises(ValueError):
            ops.jpeg_quant_table(ops.JPEG_BASE_LUMA, bad)
        with pytest.raises(ValueError):
            ops.jpeg_header(8, 8, bad)
    with pytest.raises(ValueError):
        ops.jpeg_header(0, 8, 90)
    with pytest.raises(ValueError):
        ops.jpeg_header(8, 16385, 90)


@pytest.mark.parametrize("name", ["smooth", "noise", "checker", "odd"])
def test_reference_frame_opens_in_pillow_and_matches_its_quality(name):
    img = images()[name]
    for q in (50, 90, 100):
        data = jr.encode(img, q)
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (img.shape[1], img.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
        ours = psnr(np.asarray(im), img)
        theirs = psnr(np.asarray(Image.open(io.BytesIO(pillow_jpeg(img, q))).convert("RGB")), img)
        print(f"{name} q={q}: ours {ours:.3f} dB, Pillow {theirs:.3f} dB, {len(data)} bytes")
        if np.isinf(theirs):
            # the 8-pixel checkerboard at quality 50: white blocks have DC = 1016 = 63.5 steps of 16, an exact tie, which the
            # fixed-point DCT sees as 63.497 (inside its 0.042 bound): white decodes as 254.  Nothing else differs.
            assert name == "checker" and np.abs(np.asarray(im).astype(int) - img).max() <= 1
            continue
        assert ours >= theirs - PSNR_MARGIN_DB, (name, q, ours, theirs)
    # an RGBA frame: alpha is ignored
    rgba = np.concatenate([img, np.full(img.shape[:2] + (1,), 7, np.uint8)], -1)
    assert jr.encode(rgba, 90) == jr.encode(img, 90)


def test_integer_dct_is_within_a_sixteenth_of_float64():
    bound = jr.dct_worst_case_error()
    print(f"worst-case bound of the fixed-point DCT (S = {jr.S}): {bound:.6f} coefficient units")
    assert bound <= 1.0 / 16
    rng = np.random.default_rng(1)
    blocks = [jr.blocks_of(im).reshape(-1, 8, 8) for im in images().values()]
    blocks.append(rng.integers(-128, 128, (4096, 8, 8)))
    ext = rng.choice(np.array([-128, 127]), (4096, 8, 8))
    blocks.append(ext)
    # the sign patterns that maximise single coefficients: sign of the basis functions
    A = jr.dct_matrix_f64()
    basis = np.stack([np.where(np.outer(A[a], A[b]) >= 0, 127, -128) for a in range(8) for b in range(8)])
    blocks += [basis, -1 - basis]
    x = np.concatenate(blocks).astype(np.int64)
    fixed = jr.fdct_fixed(x)
    # the accumulator bounds of DESIGN.md 5.13
    assert np.abs(jr.DCT_M).sum(1).max() <= 92680 and np.abs(jr.DCT_M).max() <= 16069
    assert np.abs(jr.DCT_M @ x).max() < 2 ** 24 and np.abs(fixed).max() < 2 ** 41
    err = np.abs(fixed / 4.0 ** jr.S - jr.fdct_f64(x)).max()
    print(f"measured maximum over {x.shape[0]} blocks: {err:.6f}")
    assert err <= bound + 1e-9 and err <= 1.0 / 16


def test_quantiser_rounds_half_away_from_zero():
    Q = np.full(64, 3, np.int64)
    one = 1 << (2 * jr.S)
    c = np.zeros((8, 8), np.int64)
    c[0, 0], c[0, 1], c[0, 2], c[0, 3], c[1, 0], c[1, 1] = 3 * one // 2, -3 * one // 2, 3 * one // 2 - 1, 4 * one, -5000 * one, 9 * one // 2
    q = jr.quantise(c, Q)
    assert q[0, 0] == 1 and q[0, 1] == -1 and q[0, 2] == 0 and q[0, 3] == 1 and q[1, 0] == -1023 and q[1, 1] == 2


def wav_like(n, channels, rate, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(-32768, 32768, (n, channels)).astype(np.int16), rate


@pytest.mark.parametrize("fps, frac", [(25, (25, 1)), (29.97, (2997, 100)), (30000 / 1001, (30000, 1001)), (12.5, (25, 2))])
def test_avi_round_trip(tmp_path, fps, frac):
    rng = np.random.default_rng(2)
    frames = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (101, 64, 33, 1000, 7) * 13]      # odd and even lengths
    pcm, rate = wav_like(int(22050 * 2.3), 2, 22050)
    path = tmp_path / "a.avi"
    n = media.write_avi(path, frames, fps, (104, 72), (pcm, rate))
    blob = path.read_bytes()
    assert n == len(blob)
    avi = jr.parse_avi(blob)
    assert avi["frames"] == frames
    assert avi["audio"] == pcm.astype("<i2").tobytes()
    v, a = avi["streams"]
    assert (v["type"], v["handler"], v["rate"], v["scale"], v["length"]) == (b"vids", b"MJPG", frac[0], frac[1], len(frames))
    assert v["rect"] == (0, 0, 104, 72)
    size, w, h, planes, bits, comp = struct.unpack_from("<IiiHH4s", v["strf"])
    assert (size, w, h, planes, bits, comp) == (40, 104, 72, 1, 24, b"MJPG") and len(v["strf"]) == 40
    assert (a["type"], a["scale"], a["rate"], a["length"], a["samplesize"]) == (b"auds", 4, 22050 * 4, pcm.shape[0], 4)
    assert struct.unpack("<HHIIHHH", a["strf"]) == (1, 2, 22050, 22050 * 4, 4, 16, 0)
    us, _, _, flags, total, _, streams, _, aw, ah = avi["avih"][:10]
    assert us == int(round(1e6 * frac[1] / frac[0])) and total == len(frames) and streams == 2 and (aw, ah) == (104, 72)
    assert flags & 0x10 and flags & 0x100
    # the index names every chunk in file order, flags key frames, and its offsets lead to the chunk headers
    assert [e[0] for e in avi["index"]] == avi["chunk_order"]
    for cid, fl, off, sz in avi["index"]:
        at = avi["movi_pos"] + off
        assert blob[at:at + 4] == cid and struct.unpack_from("<I", blob, at + 4)[0] == sz and at % 2 == 0
        assert fl & 0x10
    # audio is interleaved about a second at a time: a chunk before the first frame and none longer than a second + the tail
    order = avi["chunk_order"]
    assert order[0] == b"01wb" and order.count(b"01wb") == min(int(np.ceil(len(frames) / fps)), 3)     # 2.3 s of audio
    # silent file
    media.write_avi(path, frames[:3], fps, (104, 72))
    silent = jr.parse_avi(path.read_bytes())
    assert silent["frames"] == frames[:3] and silent["audio"] == b"" and len(silent["streams"]) == 1 and silent["avih"][6] == 1


def test_avi_audio_conversion_and_mono():
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -3.0, 1.5 / 32768, 2.5 / 32768, 0.99999], np.float32)
    assert media.pcm16(x).tolist() == [0, 16384, -16384, 32767, -32768, 32767, -32768, 2, 2, 32767]
    i = np.array([[1, -2], [3, 4]], np.int16)
    assert media.pcm16(i) is i


def test_avi_float_mono_track(tmp_path):
    x = np.linspace(-1.2, 1.2, 1601, dtype=np.float32).reshape(-1, 1)
    media.write_avi(tmp_path / "m.avi", [b"\xff\xd8\xff\xd9"] * 5, 25, (8, 8), (x, 8000))
    avi = jr.parse_avi((tmp_path / "m.avi").read_bytes())
    assert avi["audio"] == media.pcm16(x).astype("<i2").tobytes()
    assert struct.unpack("<HHIIHHH", avi["streams"][1]["strf"]) == (1, 1, 8000, 16000, 2, 16, 0)


def test_avi_two_gib_guard(tmp_path):
    big = bytes(1 << 20)
    path = tmp_path / "big.avi"
    with pytest.raises(ValueError, match=r"\d{10} bytes"):
        media.write_avi(path, [big] * 2048, 25, (512, 512))
    assert not path.exists()
    with pytest.raises(ValueError):
        media.write_avi(path, [], 25, (8, 8))


def test_cli_flags():
    need = ["--model_root", "r", "--model_name", "n", "--model_iter", "1", "--style_clip_exp_code_path", "e",
            "--style_clip_head_rot_path", "h", "--audio_clip", "a.wav"]
    a = inference.parse_args(need)
    assert a.video is False and a.video_quality == 90 and a.render_size == 0
    a = inference.parse_args(need + ["--render_size", "256", "--video", "--video_quality", "75"])
    assert a.video is True and a.video_quality == 75
    for bad in (["--video"], ["--video", "--render_size", "0"], ["--render_size", "64", "--video", "--video_quality", "0"]):
        with pytest.raises(SystemExit):
            inference.parse_args(need + bad)
