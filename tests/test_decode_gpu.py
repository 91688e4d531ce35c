"""The HIP JPEG decoder (csrc/jpeg_decode.hip) against the numpy restatement of its definition (tests/jpeg_decode_ref.py): every
comparison is equality of integers -- coefficients, pixels and status -- on files from this project's encoder and from Pillow,
whole and damaged.  Also the ends around it: AVI -> frames, the face-crop command line on an `.avi`, the argument checks."""
import functools
import io
import pickle
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_decode_ref as dr
from msmd_amd import ops
from msmd_amd.utils import media

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def content(kind, H, W, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "const":
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (H, W, 3)).copy()
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = 30 + 200 * x / max(W - 1, 1)
    g = 128 + 100 * np.sin(x / 11.0 + seed) * np.cos(y / 5.0)
    b = 255 * y / max(H - 1, 1)
    img = np.rint(np.stack([r, g, b], -1)).astype(np.int64) + rng.integers(-9, 10, (H, W, 3))
    img[H // 3:H // 2 + 1, W // 4:W // 2 + 1] = 255
    return np.clip(img, 0, 255).astype(np.uint8)


def pillow_jpeg(img, q=90, sub=0, restart=0, **kw):
    b = io.BytesIO()
    if sub == "grey":
        Image.fromarray(img[..., 1]).save(b, "JPEG", quality=q, restart_marker_blocks=restart, **kw)
    else:
        Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=sub, restart_marker_blocks=restart, **kw)
    return b.getvalue()


def own_jpeg(frames_np, q):
    """The files of this project's encoder for (B, H, W, 3) uint8 frames."""
    return media.encode_jpeg(torch.from_numpy(np.ascontiguousarray(frames_np)).to(DEV), q)


@functools.lru_cache(maxsize=None)
def reference(data):
    """(coefficients (blocks, 64) int16, status, pixels (H, W, 3)) of one file by the numpy definition; computed once per file."""
    coef, status, f = dr.decode_coefficients(data)
    assert np.abs(coef).max() <= 32768
    return coef.astype(np.int16), status, dr.pixels_of(coef, f, 3)


def check(files, channels=3):
    """Coefficients, pixels and status of one call equal the restatement's for every file; -> the pixels (numpy)."""
    coef, status_c = ops.jpeg_decode_coefficients(files)
    px, status = ops.jpeg_decode(files, channels=channels, strict=False)
    coef, status_c, px, status = coef.cpu().numpy(), status_c.cpu().numpy(), px.cpu().numpy(), status.cpu().numpy()
    assert px.shape[0] == len(files) and px.shape[3] == channels and px.dtype == np.uint8
    for b, data in enumerate(files):
        ref_coef, ref_status, ref_px = reference(bytes(data))
        assert coef[b].shape == ref_coef.shape and px[b].shape[:2] == ref_px.shape[:2]
        assert np.array_equal(coef[b], ref_coef), (b, "coefficients", int((coef[b] != ref_coef).sum()))
        assert status[b] == ref_status == status_c[b], (b, "status", status[b], ref_status)
        assert np.array_equal(px[b][..., :3], ref_px), (b, "pixels", int((px[b][..., :3] != ref_px).sum()))
        if channels == 4:
            assert (px[b][..., 3] == 255).all()
    return px


@pytest.mark.parametrize("quality", [1, 50, 90, 100])
@pytest.mark.parametrize("H, W", [(1, 1), (7, 9), (8, 8), (8, 248), (8, 256), (8, 264), (16, 536), (24, 2056)])
def test_own_encoder_files(H, W, quality):
    files = own_jpeg(content("mixed", H, W, seed=H + W)[None], quality)
    h, iv = ops.jpeg_parse(files[0])
    assert h["restart_interval"] == 32 and len(iv) == -(-h["n_mcu"] // 32) and h["layout"] == ops.JPEG_444
    check(files)


@pytest.mark.parametrize("restart", [1, 5, 0])
@pytest.mark.parametrize("sub", [0, 1, 2, "grey"])
@pytest.mark.parametrize("H, W", [(16, 16), (17, 33), (23, 37)])
def test_pillow_files(H, W, sub, restart):
    check([pillow_jpeg(content("mixed", H, W, seed=3), 90, sub, restart)])
    check([pillow_jpeg(content("noise", H, W, seed=4), 75, sub, restart)], channels=4)


def test_sixty_five_intervals_use_the_second_wave():
    data = pillow_jpeg(content("mixed", 8, 520, seed=5), 90, 0, 1)
    assert ops.jpeg_parse(data)[1].shape[0] == 65
    check([data])


def test_optimised_tables_stuffed_bytes_and_constant_frames():
    opt = pillow_jpeg(content("mixed", 23, 37, seed=6), 90, 2, 0, optimize=True)
    plain = pillow_jpeg(content("mixed", 23, 37, seed=6), 90, 2, 0)
    assert ops.jpeg_parse(opt)[0]["table_set"] != ops.jpeg_parse(plain)[0]["table_set"]
    check([opt, plain])
    noise = pillow_jpeg(content("noise", 40, 56, seed=7), 100, 0, 3)
    h = ops.jpeg_parse(noise)[0]
    assert b"\xff\x00" in noise[h["scan"][0]:h["scan"][1]]
    check([noise])
    const = pillow_jpeg(content("const", 24, 40), 90, 1, 2)
    px = check([const])
    assert np.abs(px[0].astype(int) - content("const", 24, 40)).max() <= 3
    check(own_jpeg(content("const", 24, 40)[None], 90))


def test_batch_of_three_table_sets_and_members_alone():
    imgs = [content("mixed", 24, 72, seed=s) for s in (1, 2, 3)]
    files = [pillow_jpeg(im, q, 2, 4) for im, q in zip(imgs, (50, 90, 100))]
    assert ops._jpeg_plan(files).n_sets == 3
    whole = check(files)
    again = ops.jpeg_decode(files).cpu().numpy()
    assert np.array_equal(whole, again)
    for b in range(3):
        assert np.array_equal(ops.jpeg_decode([files[b]]).cpu().numpy()[0], whole[b])
    # the second input form: the encoder's stream and offsets, copied to the host once
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    stream, offsets = ops.jpeg_encode(frames, 90)
    px = ops.jpeg_decode((stream.cpu().numpy(), offsets.cpu().numpy())).cpu().numpy()
    assert np.array_equal(px, ops.jpeg_decode(media.encode_jpeg(frames, 90)).cpu().numpy())
    assert np.array_equal(px, ops.jpeg_decode((stream.cpu(), offsets.cpu())).cpu().numpy())


@pytest.mark.parametrize("B", [64, 65])
def test_many_small_frames_in_one_call(B):
    rng = np.random.default_rng(B)
    files = own_jpeg(rng.integers(0, 256, (B, 8, 8, 3), dtype=np.uint8), 90)
    assert ops._jpeg_plan(files).intervals.shape[0] == 64 * -(-B // 64)
    check(files)
    check(files, channels=4)


def test_four_channels_equal_three():
    files = [pillow_jpeg(content("mixed", 23, 37, seed=8), 90, 2, 2)] * 2
    three = ops.jpeg_decode(files, channels=3).cpu().numpy()
    four = ops.jpeg_decode(files, channels=4).cpu().numpy()
    assert four.shape == (2, 23, 37, 4) and (four[..., 3] == 255).all() and np.array_equal(four[..., :3], three)
    # written in place, inside guard bands: 23 x 37 pixels are no multiple of four, so the last lane writes single bytes
    for channels in (3, 4):
        n = 23 * 37 * channels
        buf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        out = buf[64:64 + n].view(1, 23, 37, channels)
        assert ops.jpeg_decode(files[:1], channels=channels, out=out).data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        assert (host[:64] == 0xAB).all() and (host[64 + n:] == 0xAB).all()
        assert np.array_equal(host[64:64 + n].reshape(23, 37, channels)[..., :3], three[0])


def damaged_flip(data, interval):
    """One byte of `interval` flipped so that no marker appears and the restatement reports an error; the first such byte."""
    h, iv = ops.jpeg_parse(data)
    a, e = (int(v) for v in iv[interval])
    for p in range(a + 2, e - 2):
        if 0xFF in data[p - 1:p + 2] or (data[p] ^ 0x10) == 0xFF:
            continue
        bad = data[:p] + bytes((data[p] ^ 0x10,)) + data[p + 1:]
        if reference(bad)[1]:
            return bad
    raise AssertionError("no damaging byte found")


def test_damaged_streams_equal_the_restatement():
    imgs = [content("mixed", 24, 72, seed=s) for s in (11, 12, 13)]
    files = [pillow_jpeg(im, 90, 1, 3) for im in imgs]
    good = check(files)
    h, iv = ops.jpeg_parse(files[2])
    cut = files[2][:int(iv[-1, 1]) - 3] + b"\xff\xd9"
    assert reference(cut)[1] != 0
    flipped = damaged_flip(files[1], 2)
    batch = [files[0], flipped, cut]
    px, status = ops.jpeg_decode(batch, strict=False)
    px, status = px.cpu().numpy(), status.cpu().tolist()
    check(batch)
    assert status[0] == 0 and status[1] != 0 and status[2] != 0
    assert np.array_equal(px[0], good[0])
    with pytest.raises(ValueError, match="frame 1:.*frame 2:"):
        ops.jpeg_decode(batch)
    with pytest.raises(ValueError, match="frame 1"):
        ops.jpeg_decode([files[0], flipped, files[2]])
    # a lost RSTn: flagged by the host, the intervals in front of it as before
    a = int(iv[1, 1])
    gone = files[2][:a] + files[2][a + 2:]
    px, status = ops.jpeg_decode([files[0], gone], strict=False)
    assert status.cpu().tolist()[0] == 0 and status.cpu().tolist()[1] & ops.JPEG_ERR_RESTART
    check([files[0], gone])


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_round_trip_through_the_own_encoder():
    img = content("mixed", 72, 104, seed=9)
    for q in (50, 90, 100):
        files = own_jpeg(img[None], q)
        px = check(files)
        pil = np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB"))
        d = np.abs(px[0].astype(int) - pil)
        print(f"quality {q}: PSNR against the source {psnr(px[0], img):.3f} dB, Pillow's decode of the same bytes {psnr(pil, img):.3f} dB; "
              f"max difference {d.max()}, differing {100 * (d > 0).mean():.2f} %")
        assert d.max() <= 4 and (d > 0).mean() <= 2 * 0.0411          # the CPU table of DESIGN.md 5.24 (tests/test_decode_cpu.py)


def write_wav(path, pcm, rate):
    path.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm.nbytes) + b"WAVEfmt " +
                     struct.pack("<IHHIIHH", 16, 1, pcm.shape[1], rate, rate * 2 * pcm.shape[1], 2 * pcm.shape[1], 16) +
                     b"data" + struct.pack("<I", pcm.nbytes) + pcm.tobytes())


def test_avi_to_frames_and_the_face_crop_command_line(tmp_path):
    from msmd_amd.utils import face_crop as FC
    T, H, W = 7, 48, 64
    frames_np = np.stack([content("mixed", H, W, seed=20 + t) for t in range(T)])
    frames = torch.from_numpy(frames_np).to(DEV)
    pcm = np.random.default_rng(7).integers(-32768, 32768, (int(0.2 * 22050), 2)).astype("<i2")
    write_wav(tmp_path / "s.wav", pcm, 22050)
    avi = tmp_path / "clip.avi"
    media.combine_frames_and_audio(frames, str(tmp_path / "s.wav"), 12.5, str(avi), quality=90)
    direct = media.decode_jpeg(media.encode_jpeg(frames, 90))
    for chunk in (256, 3):                                  # one call, and calls of 3, 3 and 1 frames
        video = media.read_video(avi, chunk=chunk)
        assert tuple(video.shape) == (T, H, W, 3) and torch.equal(video, direct)
    assert torch.equal(media.read_video(avi, channels=4)[..., :3], direct)
    clip = media.read_avi(avi)
    assert clip.fps == 12.5 and clip.size == (W, H) and clip.audio[1] == 22050 and np.array_equal(clip.audio[0], pcm)
    assert np.array_equal(direct[0].cpu().numpy(), reference(clip.jpeg(0).tobytes())[2])
    # the command line on the .avi writes what it writes on the decoded frames saved as .npy
    np.save(tmp_path / "clip.npy", direct.cpu().numpy())
    with open(tmp_path / "clip.pickle", "wb") as f:
        pickle.dump({"processed_bbox_frames": [(18 + t, 10, 30, 30) for t in range(T)]}, f)
    common = ["--boxes", str(tmp_path / "clip.pickle"), "--size", "17", "--batch_size", "4"]
    FC.main(["--frames", str(avi), "--out", str(tmp_path / "a.npy"), "--video", str(tmp_path / "a.avi")] + common)
    FC.main(["--frames", str(tmp_path / "clip.npy"), "--out", str(tmp_path / "b.npy"), "--video", str(tmp_path / "b.avi"), "--fps", "12.5"] + common)
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert a.shape == (T, 3, 17, 17) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (tmp_path / "a.avi").read_bytes() == (tmp_path / "b.avi").read_bytes()      # --fps defaulted to the file's 25 / 2
    # a frame of another size inside the file
    odd = media.encode_jpeg(frames[:1, :40], 90)
    media.write_avi(tmp_path / "mixed.avi", media.encode_jpeg(frames[:2], 90) + odd, 25, (W, H))
    with pytest.raises(ValueError, match="share size"):
        media.read_video(tmp_path / "mixed.avi")
    with pytest.raises(ValueError, match="frame 2"):
        media.read_video(tmp_path / "mixed.avi", chunk=2)


def test_argument_checks():
    files = [pillow_jpeg(content("mixed", 16, 16), 90, 0, 0)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.jpeg_decode(files, out=torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.jpeg_decode(files, device="cpu")
    with pytest.raises(TypeError, match="out must have shape"):
        ops.jpeg_decode(files, out=torch.zeros(1, 16, 16, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.jpeg_decode(files, out=torch.zeros(1, 16, 16, 3, dtype=torch.int8, device=DEV))
    with pytest.raises(TypeError, match="multiple of 4"):
        ops.jpeg_decode(files, out=torch.zeros(16 * 16 * 3 + 1, dtype=torch.uint8, device=DEV)[1:].view(1, 16, 16, 3))
    with pytest.raises(ValueError, match="channels"):
        ops.jpeg_decode(files, channels=2)
    with pytest.raises(ValueError, match="share size"):
        ops.jpeg_decode(files + [pillow_jpeg(content("mixed", 16, 24), 90, 0, 0)])
    with pytest.raises(ValueError, match="share size"):
        ops.jpeg_decode(files + [pillow_jpeg(content("mixed", 16, 16), 90, 2, 0)])
    with pytest.raises(ValueError, match="SOF2"):
        ops.jpeg_decode([pillow_jpeg(content("mixed", 16, 16), 90, 0, 0, progressive=True)])
    with pytest.raises(TypeError):
        ops.jpeg_decode((torch.zeros(8, dtype=torch.uint8, device=DEV), [0, 8]))
    lib = ops._lib.load()
    assert lib.msmd_jpeg_decode_blocks(23, 37, ops.JPEG_420) == 2 * 3 * 4 + 2 * 2 * 3 and lib.msmd_jpeg_decode_blocks(0, 8, 0) == -1
    assert lib.msmd_jpeg_decode_blocks(8, 8, 4) == -1 and lib.msmd_jpeg_decode_pixels(None, 1, 8, 8, 0, 3, None, None) == 1
