"""The HIP JPEG encoder (csrc/jpeg.hip) against the numpy restatement of its definition (tests/jpeg_ref.py): every comparison
is equality of integers or bytes.  Also the two ends around it: renderer -> AVI with a sound track, and the argument checks."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as jr
from msmd_amd import ops, synth
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
    if kind == "checker8":
        return np.broadcast_to((((y // 8 + x // 8) & 1) * 255).astype(np.uint8)[..., None], (H, W, 3)).copy()
    if kind == "checker1":
        return np.broadcast_to((((y + x) & 1) * 255).astype(np.uint8)[..., None], (H, W, 3)).copy()
    if kind == "gradient":
        r = 30 + 200 * x / max(W - 1, 1)
        g = 128 + 100 * np.sin(x / 11.0 + seed) * np.cos(y / 5.0)
        b = 255 * y / max(H - 1, 1)
        return np.clip(np.rint(np.stack([r, g, b], -1)), 0, 255).astype(np.uint8)
    if kind == "mixed":                                     # shaded gradient + a little noise + a saturated patch
        img = content("gradient", H, W, seed).astype(np.int64) + rng.integers(-9, 10, (H, W, 3))
        img[H // 3:H // 2 + 1, W // 4:W // 2 + 1] = 255
        return np.clip(img, 0, 255).astype(np.uint8)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, H, W, seed, quality):
    """(coefficients (n_mcu, 3, 64), file bytes) of one frame by the numpy definition; computed once per case."""
    img = content(kind, H, W, seed)
    coefs = jr.coefficients(img, quality)
    return coefs, jr.header(H, W, quality) + jr.scan(coefs) + b"\xff\xd9"


def split(stream, offsets):
    blob, off = stream.cpu().numpy().tobytes(), offsets.cpu().tolist()
    assert off[0] == 0 and off[-1] == len(blob)
    return [blob[a:b] for a, b in zip(off[:-1], off[1:])]


def check_against_reference(frames_np, frames_dev, specs, quality):
    """frames_dev holds the frames of `specs` = [(kind, H, W, seed)]: coefficients, bytes and offsets equal the reference's."""
    coef = ops.jpeg_coefficients(frames_dev, quality).cpu().numpy()
    files = split(*ops.jpeg_encode(frames_dev, quality))
    assert len(files) == len(specs)
    for b, spec in enumerate(specs):
        ref_coef, ref_file = reference(*spec, quality)
        assert coef[b].shape == ref_coef.shape
        assert np.array_equal(coef[b].astype(np.int64), ref_coef), (spec, "coefficients")
        assert files[b] == ref_file, (spec, "bytes", len(files[b]), len(ref_file))
        im = Image.open(io.BytesIO(files[b]))
        im.load()
        assert im.size == (spec[2], spec[1]) and im.mode == "RGB"
    return files


SHAPES = [(1, 1), (7, 9), (8, 8), (8, 248), (8, 256), (8, 264), (16, 536), (24, 2056), (72, 104)]


@pytest.mark.parametrize("H, W", SHAPES)
def test_shapes(H, W):
    spec = ("mixed", H, W, 1)
    img = content(*spec)
    check_against_reference(img, torch.from_numpy(img[None]).to(DEV), [spec], 90)
    if (H, W) == (24, 2056):
        n_int = -(-(3 * 257) // 32)
        assert n_int > 8 and reference(*spec, 90)[1].count(b"\xff\xd0") >= 2        # RSTn wrapped past 7


@pytest.mark.parametrize("quality", [1, 50, 90, 100])
def test_batch_of_three_rgba_with_padded_rows(quality):
    """B = 3, RGBA, a row stride larger than the row; and each frame alone gives the bytes it has inside the batch."""
    H, W = 72, 104
    specs = [("mixed", H, W, 2), ("gradient", H, W, 3), ("mixed", H, W, 4)]
    buf = torch.full((3, H, W + 5, 4), 77, dtype=torch.uint8)
    for b, s in enumerate(specs):
        buf[b, :, :W, :3] = torch.from_numpy(content(*s))
    dev = buf.to(DEV)
    view = dev[:, :, :W]
    assert not view.is_contiguous()
    files = check_against_reference(None, view, specs, quality)
    for b in (0, 2):
        alone = split(*ops.jpeg_encode(view[b:b + 1], quality))
        assert alone == [files[b]]
    # the same input twice: the same bytes, and the 3-channel view of the RGBA buffer (what the renderer returns) as well
    again = split(*ops.jpeg_encode(view, quality))
    rgb_view = split(*ops.jpeg_encode(view[..., :3], quality))
    assert again == files and rgb_view == files


@pytest.mark.parametrize("kind, quality", [("const", 90), ("noise", 100), ("checker8", 50), ("checker8", 100), ("checker1", 100),
                                           ("checker1", 1), ("gradient", 90)])
def test_content(kind, quality):
    H, W = 40, 264
    spec = (kind, H, W, 5)
    img = content(*spec)
    files = check_against_reference(img, torch.from_numpy(img[None]).to(DEV), [spec], quality)
    coefs = reference(*spec, quality)[0]
    if kind == "const":
        assert not coefs[:, :, 1:].any()                    # every block is EOB only
    if kind == "noise":
        scan = files[0][len(jr.header(H, W, quality)):]
        assert scan.count(b"\xff\x00") > 20                 # stuffing is exercised
    if kind == "checker8" and quality == 100:
        dc = coefs[:, 0, 0]
        assert dc.min() == -1024 and dc.max() == 1016       # DC differences of +-2040: category 11
    if kind == "checker1" and quality == 100:
        assert np.abs(coefs[:, :, 1:]).max() >= 800         # the largest AC magnitude a block can hold: category 10


def test_rgb_odd_strides_take_the_byte_path():
    """A contiguous RGB tensor (3-byte pixels) and an RGBA view at an odd byte offset: the same bytes as the aligned RGBA path."""
    spec = ("mixed", 23, 37, 6)
    img = content(*spec)
    ref = reference(*spec, 90)[1]
    rgb = torch.from_numpy(img[None]).to(DEV)
    assert split(*ops.jpeg_encode(rgb, 90)) == [ref]
    flat = torch.zeros(1 + 23 * 37 * 4 + 3, dtype=torch.uint8, device=DEV)
    odd = flat[1:1 + 23 * 37 * 4].view(1, 23, 37, 4)
    odd[..., :3] = rgb
    assert odd.data_ptr() % 4 == 1
    assert split(*ops.jpeg_encode(odd, 90)) == [ref]


def test_argument_checks():
    ok = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError):
        ops.jpeg_encode(ok.float())
    with pytest.raises(TypeError):
        ops.jpeg_encode(ok.cpu())
    with pytest.raises(ValueError):
        ops.jpeg_encode(ok, quality=0)
    with pytest.raises(ValueError):
        ops.jpeg_encode(ok, quality=101)
    with pytest.raises(ValueError):
        ops.jpeg_encode(torch.zeros(1, 8, 0, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.jpeg_encode(torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.jpeg_encode(torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.jpeg_encode(torch.zeros(1, 8, 3, 8, dtype=torch.uint8, device=DEV).permute(0, 1, 3, 2))
    with pytest.raises(TypeError):       # a 3-channel view with 4-byte pixels whose storage ends with the last blue byte
        ops.jpeg_encode(torch.zeros(8 * 8 * 4 - 1, dtype=torch.uint8, device=DEV).as_strided((1, 8, 8, 3), (256, 32, 4, 1)))


def test_sphere_to_avi_with_sound(tmp_path):
    """MeshRenderer.render_vertices -> combine_frames_and_audio with a stereo int16 WAV: the file parses back to the frames'
    count and size, the frame rate and the WAV's own bytes; every frame opens and looks like the rendered one."""
    import struct
    from msmd_amd.utils.audio import read_wav
    from msmd_amd.utils.renderer import MeshRenderer
    v, f = synth.latlong_sphere(7, 16, 0.09)
    T, W, H = 6, 72, 56
    verts = torch.from_numpy(v[None] * (1.0 + 0.05 * np.arange(T, dtype=np.float32)[:, None, None])).to(DEV)
    frames = MeshRenderer((W, H)).render_vertices(verts, f)[0]
    assert tuple(frames.shape) == (T, H, W, 3) and frames.stride(2) == 4
    rng = np.random.default_rng(7)
    pcm = rng.integers(-32768, 32768, (int(0.2 * 22050), 2)).astype("<i2")
    wav = tmp_path / "s.wav"
    wav.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, 22050, 88200, 4, 16)
                    + b"data" + struct.pack("<I", pcm.nbytes) + pcm.tobytes())
    back, rate = read_wav(wav)
    assert back.dtype == np.int16 and rate == 22050
    out = tmp_path / "sphere.avi"
    n = media.combine_frames_and_audio(frames, str(wav), 25, str(out), quality=90)
    blob = out.read_bytes()
    assert n == len(blob)
    avi = jr.parse_avi(blob)
    assert len(avi["frames"]) == T and avi["audio"] == pcm.tobytes()
    vs, au = avi["streams"]
    assert (vs["rate"], vs["scale"], vs["length"], vs["rect"]) == (25, 1, T, (0, 0, W, H))
    assert struct.unpack("<HHIIHHH", au["strf"]) == (1, 2, 22050, 88200, 4, 16, 0)
    host = frames.cpu().numpy()
    for t, data in enumerate(avi["frames"]):
        assert data == jr.encode(host[t], 90)
        im = Image.open(io.BytesIO(data))
        assert im.size == (W, H)
        assert np.abs(np.asarray(im.convert("RGB")).astype(int) - host[t]).mean() < 2.0
    assert media.encode_jpeg(frames, 90) == avi["frames"]
