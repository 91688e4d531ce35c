"""Frames out: rendered frames on the device -> a Motion-JPEG AVI with the clip's sound track (the reference's utils/media.py
pipes PNG files and the audio through ffmpeg to H.264; there is no ffmpeg here, and no other library is used).

Each frame is compressed on the device by the baseline JPEG encoder of csrc/jpeg.hip (`ops.jpeg_encode`) and
leaves it at its compressed size; this module only lays the bytes out as RIFF `AVI ` on the host.  The file is AVI 1.0 with an
`idx1` index, at most 2^31 - 1 bytes: OpenDML (AVI 2.0), H.264 and 4:2:0 stay outside.
"""
from __future__ import annotations

import os
import struct
from fractions import Fraction

import numpy as np

from .. import ops

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
