"""Frames out: rendered frames on the device -> a Motion-JPEG AVI with the clip's sound track (the reference's utils/media.py
pipes PNG files and the audio through ffmpeg to H.264; there is no ffmpeg here, and no other library is used).

Each frame is compressed on the device by the baseline JPEG encoder of csrc/jpeg.hip (`ops.jpeg_encode`) and
leaves it at its compressed size; this module only lays the bytes out as RIFF `AVI ` on the host.  The file is AVI 1.0 with an
`idx1` index, at most 2^31 - 1 bytes: OpenDML (AVI 2.0), H.264 and 4:2:0 stay outside.

Frames in: `read_avi` finds the JPEG files inside a Motion-JPEG AVI, this project's or another writer's,
`read_video` decodes them on the device with `ops.jpeg_decode` (baseline, grey / 4:4:4 / 4:2:2 / 4:2:0), and `extract_frames`
writes them out as `.jpg` files, which is what the reference's helper of that name does through ffmpeg.

Frames of another size: `read_video(size=)` stores a clip at the size it is wanted, `side_by_side` joins panels of
different sizes at one height, `frames_at` picks the source frame nearest in time, and `python -m msmd_amd.utils.media --resize
IN.avi OUT.avi --size WxH` re-encodes a clip; all of them resize with `ops.resize_frames` (csrc/resize.hip).
"""
from __future__ import annotations

import os
import struct
from fractions import Fraction
from typing import NamedTuple, Optional

import numpy as np

from .. import ops
from ..jpeg_format import jpeg_dht

AVI_MAX_BYTES = 2 ** 31 - 1
_AVIF_HASINDEX, _AVIF_ISINTERLEAVED, _AVIIF_KEYFRAME = 0x10, 0x100, 0x10


def encode_jpeg(frames, quality=90):
    """frames (B, H, W, 3 | 4) uint8 on the device -> list of B `bytes`, one JFIF file each (ops.jpeg_encode)."""
    stream, offsets = ops.jpeg_encode(frames, quality)
    blob, off = stream.cpu().numpy().tobytes(), offsets.cpu().tolist()
    return [blob[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def pcm16(pcm):
    """Samples as `utils.audio.read_wav` returns them, (frames, channels) or (frames,), -> int16 of the same shape: int16 as it
    is, anything else as float in [-1, 1) scaled by 2^15, rounded half to even and saturated."""
    a = np.asarray(pcm)
    if a.dtype == np.int16:
        return a
    return np.clip(np.rint(a.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def fps_fraction(fps):
    """-> (dwRate, dwScale): fps as a reduced fraction (a float is taken to the nearest fraction with a denominator <= 100000:
    29.97 -> 2997 / 100, 30000 / 1001 stays)."""
    f = Fraction(fps).limit_denominator(100000)
    if f <= 0:
        raise ValueError(f"fps must be positive, got {fps!r}")
    return f.numerator, f.denominator


def _chunk(fourcc, body):
    return [fourcc + struct.pack("<I", len(body)), body] + ([b"\x00"] if len(body) & 1 else [])


def _list(kind, pieces):
    size = 4 + sum(len(p) for p in pieces)
    return [b"LIST" + struct.pack("<I", size) + kind] + pieces


def write_avi(path, jpeg_frames, fps, size, audio=None):
    """Motion-JPEG AVI: `jpeg_frames` (list of JFIF files as bytes) at `fps` (int, float or Fraction), `size` = (width, height);
    `audio` = None or (pcm, rate) as `utils.audio.read_wav` returns it: the sound track keeps its rate and channel count and
    is stored as 16-bit PCM (`pcm16`).  Layout: `hdrl` (`avih`, a `vids` / `MJPG` stream, an optional `auds` stream), `movi`
    with one `00dc` chunk per frame and, before the frames of each second, one `01wb` chunk with that second's samples (what is
    left after the last frame goes into a final chunk), `idx1` with every frame a key frame.  Chunks are padded to even
    lengths.  A file that would be larger than 2^31 - 1 bytes raises ValueError before anything is written.  -> bytes written."""
    frames = list(jpeg_frames)
    if not frames:
        raise ValueError("write_avi: no frames")
    width, height = int(size[0]), int(size[1])
    rate, scale = fps_fraction(fps)
    n = len(frames)
    tracks = []                                             # audio chunk to write before frame k
    wave = None
    if audio is not None:
        pcm, arate = audio
        pcm = pcm16(pcm)
        pcm = np.ascontiguousarray(pcm.reshape(pcm.shape[0], -1).astype("<i2"))
        channels, arate = pcm.shape[1], int(arate)
        align = 2 * channels
        wave = (channels, arate, align, pcm.shape[0])
        raw = pcm.tobytes()
        seconds = -(-n * scale // rate)                     # ceil(n / fps)
        at = 0
        for s in range(seconds):
            first = s * rate // scale                       # the frame on screen at second s
            end = pcm.shape[0] if s == seconds - 1 else min((s + 1) * arate, pcm.shape[0])
            if end > at:
                tracks.append((first, raw[at * align:end * align]))
            at = max(at, end)
    # sizes first: the guard has to speak before the file exists
    video_bytes = sum(8 + len(f) + (len(f) & 1) for f in frames)
    audio_bytes = sum(8 + len(a) for _, a in tracks)
    n_chunks = n + len(tracks)
    hdrl_bytes = 12 + (8 + 56) + (12 + (8 + 56) + (8 + 40)) + ((12 + (8 + 56) + (8 + 18)) if wave else 0)
    total = 12 + hdrl_bytes + 12 + video_bytes + audio_bytes + 8 + 16 * n_chunks
    if total > AVI_MAX_BYTES:
        raise ValueError(f"write_avi: the file would be {total} bytes, more than the {AVI_MAX_BYTES} an AVI 1.0 file can hold "
                         "(OpenDML is not written): lower the quality, the size or the number of frames")
    biggest = max(len(f) for f in frames)
    byte_rate = int(sum(len(f) for f in frames) * rate / (scale * n)) + (wave[2] * wave[1] if wave else 0)
    avih = struct.pack("<14I", int(round(1e6 * scale / rate)), byte_rate, 0, _AVIF_HASINDEX | _AVIF_ISINTERLEAVED, n, 0,
                       2 if wave else 1, biggest, width, height, 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xFFFFFFFF, 0,
                         0, 0, width, height)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    strls = _list(b"strl", _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v))
    if wave:
        channels, arate, align, n_samples = wave
        strh_a = struct.pack("<4s4sIHHIIIIIIII4h", b"auds", b"\x00\x00\x00\x00", 0, 0, 0, 0, align, arate * align, 0, n_samples,
                             max((len(a) for _, a in tracks), default=0), 0xFFFFFFFF, align, 0, 0, 0, 0)
        strf_a = struct.pack("<HHIIHHH", 1, channels, arate, arate * align, align, 16, 0)
        strls += _list(b"strl", _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a))
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + strls)
    movi, index, pos = [], [], 4                            # idx1 offsets count from the `movi` fourcc
    pending = list(tracks)
    for k, f in enumerate(frames):
        while pending and pending[0][0] <= k:
            a = pending.pop(0)[1]
            index.append(struct.pack("<4sIII", b"01wb", _AVIIF_KEYFRAME, pos, len(a)))
            movi += _chunk(b"01wb", a)
            pos += 8 + len(a)
        index.append(struct.pack("<4sIII", b"00dc", _AVIIF_KEYFRAME, pos, len(f)))
        movi += _chunk(b"00dc", f)
        pos += 8 + len(f) + (len(f) & 1)
    assert not pending
    body = hdrl + _list(b"movi", movi) + _chunk(b"idx1", b"".join(index))
    size_riff = 4 + sum(len(p) for p in body)
    assert size_riff + 8 == total, (size_riff + 8, total)
    with open(os.fspath(path), "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", size_riff) + b"AVI ")
        fh.writelines(body)
    return total


def combine_frames_and_audio(frames, audio_file, fps, output, quality=90, chunk=256):
    """The reference helper's name and argument order (utils/media.py: frame files + an audio file -> a video through ffmpeg),
    with two differences that its callers must know: `frames` is a (T, H, W, 3 | 4) uint8 tensor on the device (what
    `MeshRenderer.render_vertices` / `inference.render_coeffs` return), not a file pattern; and `quality` is the JPEG quality
    in [1, 100] (higher is better), not an x264 CRF (lower is better).  The result is a Motion-JPEG AVI, not H.264 in MP4.
    audio_file: a `.wav` (any rate, channel count and sample type `utils.audio.read_wav` reads; stored as 16-bit PCM) or None
    for a silent file.  `chunk` frames are encoded per call.  -> bytes written."""
    audio = None
    if audio_file is not None:
        from .audio import read_wav
        audio = read_wav(audio_file)
    jpegs = []
    for i in range(0, frames.shape[0], chunk):
        jpegs += encode_jpeg(frames[i:i + chunk], quality)
    return write_avi(output, jpegs, fps, (frames.shape[2], frames.shape[1]), audio)


# ----------------------------------------------------------------------------- frames in
def decode_jpeg(files, channels=3):
    """JFIF files (a list of bytes, or what `ops.jpeg_encode` returns, copied to the host) -> (B, H, W, channels) uint8 on the
    device: `ops.jpeg_decode`, strict."""
    return ops.jpeg_decode(files, channels=channels)


class AviClip(NamedTuple):
    """What `read_avi` returns.  data: the file as a uint8 array; frames: [(first, end)] byte ranges of the JPEG files in it, one
    per frame in display order; fps: Fraction; size: (width, height); audio: (pcm int16 (n, channels), rate) or None."""
    data: np.ndarray
    frames: list
    fps: Fraction
    size: tuple
    audio: Optional[tuple]

    def jpeg(self, k):
        return self.data[self.frames[k][0]:self.frames[k][1]]


def _riff_chunks(blob, pos, end):
    """(fourcc, body offset, size) of the chunks in blob[pos:end]; a size that runs past `end` (a cut file) is clipped."""
    while pos + 8 <= end:
        cid, size = bytes(blob[pos:pos + 4]), struct.unpack_from("<I", blob, pos + 4)[0]
        size = min(size, end - pos - 8)
        yield cid, pos + 8, size
        pos += 8 + size + (size & 1)


def read_avi(path):
    """A Motion-JPEG AVI 1.0 file -> AviClip.  Reads `avih`, the `vids` stream (handler or compression `MJPG` / `mjpg`; any other
    raises ValueError naming the fourcc), an optional 16-bit PCM `auds` stream, and the `movi` chunks through `idx1` where the
    file has one, else by walking `movi` (`LIST rec ` groups included; so a file cut short behind `movi` still reads).  Chunks
    are padded to even lengths.  A video chunk of length zero (a dropped frame) repeats the frame before it.  OpenDML (AVI
    2.0: `RIFF AVIX`, an `odml` list, `indx`) raises ValueError.  Nothing is decoded here."""
    data = np.fromfile(os.fspath(path), dtype=np.uint8)
    n = data.size
    if n < 12 or bytes(data[:4]) != b"RIFF" or bytes(data[8:12]) != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    riff_end = min(n, 8 + struct.unpack_from("<I", data, 4)[0])
    if riff_end + 12 <= n and bytes(data[riff_end:riff_end + 4]) == b"RIFF" and bytes(data[riff_end + 8:riff_end + 12]) == b"AVIX":
        raise ValueError(f"{path}: OpenDML file (RIFF AVIX): only AVI 1.0 is read")
    streams, movi, index = [], None, None
    for cid, body, size in _riff_chunks(data, 12, riff_end):
        kind = bytes(data[body:body + 4]) if cid == b"LIST" else None
        if kind == b"hdrl":
            for c2, b2, s2 in _riff_chunks(data, body + 4, body + size):
                k2 = bytes(data[b2:b2 + 4]) if c2 == b"LIST" else None
                if k2 == b"odml":
                    raise ValueError(f"{path}: OpenDML file (LIST odml): only AVI 1.0 is read")
                if k2 != b"strl":
                    continue
                st = {}
                for c3, b3, s3 in _riff_chunks(data, b2 + 4, b2 + s2):
                    if c3 == b"strh" and s3 >= 36:
                        st["type"], st["handler"] = bytes(data[b3:b3 + 4]), bytes(data[b3 + 4:b3 + 8])
                        st["scale"], st["rate"] = struct.unpack_from("<II", data, b3 + 20)
                    elif c3 == b"strf":
                        st["strf"] = bytes(data[b3:b3 + s3])
                    elif c3 == b"indx":
                        raise ValueError(f"{path}: OpenDML file (indx): only AVI 1.0 is read")
                streams.append(st)
        elif kind == b"movi":
            movi = (body, body + size)
        elif cid == b"idx1":
            index = (body, size // 16)
    if movi is None:
        raise ValueError(f"{path}: no movi list")
    video = [k for k, st in enumerate(streams) if st.get("type") == b"vids"]
    if not video:
        raise ValueError(f"{path}: no video stream")
    v = video[0]
    vs = streams[v]
    strf = vs.get("strf", b"")
    compression = strf[16:20] if len(strf) >= 20 else b""
    if vs["handler"] not in (b"MJPG", b"mjpg") and compression not in (b"MJPG", b"mjpg"):
        raise ValueError(f"{path}: video stream {vs['handler']!r} / {compression!r} is not Motion-JPEG (MJPG)")
    if vs["scale"] == 0 or vs["rate"] == 0:
        raise ValueError(f"{path}: the video stream has dwRate / dwScale = {vs['rate']} / {vs['scale']}")
    width, height = struct.unpack_from("<ii", strf, 4) if len(strf) >= 12 else (0, 0)
    audio = [k for k, st in enumerate(streams) if st.get("type") == b"auds"]
    wave = None
    if audio:
        a = audio[0]
        fmt = streams[a].get("strf", b"")
        if len(fmt) < 16:
            raise ValueError(f"{path}: the audio stream has no WAVEFORMAT")
        tag, channels, arate, _, _, bits = struct.unpack_from("<HHIIHH", fmt)
        if tag != 1 or bits != 16 or channels < 1:
            raise ValueError(f"{path}: audio format tag {tag}, {bits} bits: only 16-bit PCM is read")
        wave = (a, channels, arate)
    vid_ids = (b"%02ddc" % v, b"%02ddb" % v)
    aud_id = b"%02dwb" % wave[0] if wave else None
    chunks = []                                         # (fourcc, body offset, size) in file order
    if index is not None and index[1] > 0:
        entries = np.frombuffer(data[index[0]:index[0] + 16 * index[1]].tobytes(), dtype=[("id", "S4"), ("flags", "<u4"), ("off", "<u4"), ("size", "<u4")])
        # offsets count from the `movi` fourcc; some writers count from the start of the file
        first_off = int(entries["off"][0])
        rel = movi[0] if bytes(data[movi[0] + first_off:movi[0] + first_off + 4]) == bytes(entries["id"][0]).ljust(4, b"\x00") else 0
        for cid, off, size in zip(entries["id"].tolist(), entries["off"].tolist(), entries["size"].tolist()):
            at = rel + off + 8
            if at + size > n:
                raise ValueError(f"{path}: idx1 names bytes {at} .. {at + size} of a file of {n}")
            chunks.append((cid.ljust(4, b"\x00"), at, size))
    else:
        def walk(pos, end):
            for cid, body, size in _riff_chunks(data, pos, end):
                if cid == b"LIST":
                    if bytes(data[body:body + 4]) == b"rec ":
                        walk(body + 4, body + size)
                else:
                    chunks.append((cid, body, size))
        walk(movi[0] + 4, movi[1])
    frames, pcm = [], []
    for cid, body, size in chunks:
        if cid in vid_ids:
            if size == 0:
                if not frames:
                    raise ValueError(f"{path}: the first video chunk is empty")
                frames.append(frames[-1])
            else:
                frames.append((body, body + size))
        elif cid == aud_id:
            pcm.append(data[body:body + size])
    if not frames:
        raise ValueError(f"{path}: no video frames")
    track = None
    if wave:
        raw = np.concatenate(pcm) if pcm else np.zeros(0, np.uint8)
        align = 2 * wave[1]
        track = (np.frombuffer(raw[:raw.size // align * align].tobytes(), "<i2").reshape(-1, wave[1]).astype(np.int16), wave[2])
    return AviClip(data, frames, Fraction(vs["rate"], vs["scale"]), (int(width), abs(int(height))), track)


def read_video(path, channels=3, chunk=256, device="cuda", size=None, resample="bilinear"):
    """A Motion-JPEG AVI -> its frames as one (F, H, W, channels) uint8 tensor on the device, `chunk` frames decoded per call of
    `ops.jpeg_decode`.  A frame whose size or sampling differs from the first raises ValueError; so does a damaged one.
    size = (width, height): every decoded chunk is resized with `ops.resize_frames(chunk, size, resample)` before it is stored,
    so the clip never lives on the device at its full size; the result is `resize_frames` of what `size=None` returns."""
    import torch
    clip = read_avi(path)
    first = ops.jpeg_parse(clip.jpeg(0))[0]
    shape = (first["height"], first["width"], first["layout"])
    width, height = (shape[1], shape[0]) if size is None else (int(s) for s in size)
    out = torch.empty(len(clip.frames), height, width, channels, device=device, dtype=torch.uint8)
    for i in range(0, len(clip.frames), int(chunk)):
        j = min(i + int(chunk), len(clip.frames))
        h = ops.jpeg_parse(clip.jpeg(i))[0]
        if (h["height"], h["width"], h["layout"]) != shape:
            raise ValueError(f"{path}: frame {i} is {h['height']} x {h['width']} layout {h['layout']}, frame 0 is "
                             f"{shape[0]} x {shape[1]} layout {shape[2]}")
        files = [clip.jpeg(k) for k in range(i, j)]
        if size is not None:
            ops.resize_frames(ops.jpeg_decode(files, channels=channels, device=out.device), (width, height), resample, out=out[i:j])
        elif out[i:j].data_ptr() % 4 == 0:
            ops.jpeg_decode(files, channels=channels, out=out[i:j])
        else:
            out[i:j] = ops.jpeg_decode(files, channels=channels, device=out.device)
    return out


def extract_frames(filename, output_dir, quality=1):
    """The reference helper's name and argument order (utils/media.py: ffmpeg writes `%06d.jpg` from 0): the frames of a
    Motion-JPEG AVI as JPEG files in `output_dir`.  Nothing is decoded or re-encoded: a file is the frame's chunk as it stands in
    the AVI, with the Annex K.3 `DHT` segments inserted in front of `SOS` where the frame carries none (the AVI `MJPG`
    convention, which stand-alone readers do not know).  `quality` is accepted for the reference's callers and ignored.  Only
    Motion-JPEG is read: an H.264 file raises ValueError in `read_avi`.  -> the paths written."""
    clip = read_avi(filename)
    os.makedirs(os.fspath(output_dir), exist_ok=True)
    paths = []
    for k in range(len(clip.frames)):
        raw = clip.jpeg(k).tobytes()
        header = ops.jpeg_parse(raw)[0]
        if header["default_huffman"]:
            sos = header["scan"][0] - 8 - 2 * header["components"]
            raw = raw[:sos] + jpeg_dht() + raw[sos:]
        p = os.path.join(os.fspath(output_dir), "%06d.jpg" % k)
        with open(p, "wb") as fh:
            fh.write(raw)
        paths.append(p)
    return paths


# ----------------------------------------------------------------------------- frames of another size
def frames_at(n_out, fps_out, n_src, fps_src):
    """-> list of n_out source frame numbers: for output frame k, shown at k / fps_out, the source frame nearest in time,
    min(n_src - 1, (2 k a + b) // (2 b)) with a / b = fps_src / fps_out in lowest terms.  Integer arithmetic on `fps_fraction`'s
    numerators and denominators: a tie goes to the later frame, and no float decides a frame."""
    if n_src < 1:
        raise ValueError(f"frames_at: n_src = {n_src} must be at least 1")
    (rs, ss), (ro, so) = fps_fraction(fps_src), fps_fraction(fps_out)
    ratio = Fraction(rs * so, ss * ro)
    a, b = ratio.numerator, ratio.denominator
    return [min(n_src - 1, (2 * k * a + b) // (2 * b)) for k in range(int(n_out))]


def side_by_side(panels, height=None, resample="bilinear"):
    """panels: a list of (F, H_i, W_i, 3) uint8 device tensors with one F -> (F, height, sum W_i', 3): every panel scaled to the
    common height (the first panel's by default) with `ops.resize_frames`, its width W_i' = max(1, (2 W_i height + H_i) //
    (2 H_i)), the nearest integer that keeps its aspect, and the panels laid left to right.  A panel that already has the
    height is copied as it is."""
    import torch
    panels = list(panels)
    if not panels:
        raise ValueError("side_by_side: no panels")
    F = panels[0].shape[0]
    for p in panels:
        if not torch.is_tensor(p) or p.dim() != 4 or p.shape[3] != 3 or p.shape[0] != F or p.dtype != torch.uint8:
            raise TypeError(f"side_by_side: every panel must be a ({F}, H, W, 3) uint8 tensor, got {getattr(p, 'shape', type(p))}")
    height = int(panels[0].shape[1] if height is None else height)
    if height < 1:
        raise ValueError(f"side_by_side: height = {height} must be at least 1")
    widths = [max(1, (2 * p.shape[2] * height + p.shape[1]) // (2 * p.shape[1])) for p in panels]
    out = torch.empty(F, height, sum(widths), 3, device=panels[0].device, dtype=torch.uint8)
    at = 0
    for p, w in zip(panels, widths):
        if (p.shape[1], p.shape[2]) == (height, w):
            out[:, :, at:at + w] = p
        else:
            out[:, :, at:at + w] = ops.resize_frames(p, (w, height), resample)
        at += w
    return out


def resize_video(src, dst, size, resample="bilinear", quality=90, chunk=64):
    """Re-encode the Motion-JPEG AVI `src` at size = (width, height) into `dst`: decode, `ops.resize_frames`, encode, `chunk`
    frames at a time; the frame rate and the audio track are carried over.  -> bytes written."""
    clip = read_avi(src)
    width, height = (int(s) for s in size)
    jpegs = []
    for i in range(0, len(clip.frames), int(chunk)):
        files = [clip.jpeg(k) for k in range(i, min(i + int(chunk), len(clip.frames)))]
        jpegs += encode_jpeg(ops.resize_frames(ops.jpeg_decode(files), (width, height), resample), quality)
    return write_avi(dst, jpegs, clip.fps, (width, height), clip.audio)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m msmd_amd.utils.media", description="Re-encode a Motion-JPEG AVI at a new size.")
    ap.add_argument("--resize", nargs=2, metavar=("IN.avi", "OUT.avi"), required=True)
    ap.add_argument("--size", required=True, metavar="WxH")
    ap.add_argument("--filter", default="bilinear", choices=sorted(ops.RESIZE_FILTERS))
    ap.add_argument("--quality", type=int, default=90)
    a = ap.parse_args(argv)
    try:
        width, height = (int(v) for v in a.size.lower().split("x"))
    except ValueError:
        ap.error(f"--size must be WxH, got {a.size!r}")
    n = resize_video(a.resize[0], a.resize[1], (width, height), a.filter, a.quality)
    print(f"{a.resize[1]}: {width} x {height}, {n} bytes")


if __name__ == "__main__":
    main()
