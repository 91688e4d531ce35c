"""Audio files in: WAV reader / writer and the device front end that turns clips of any rate and channel count into the
16 kHz mono float32 tensors `inference.infer_coeffs_batch` takes (the reference calls `librosa.load(path, sr=16000)`,
inference.py:232, and z-normalises, inference.py:234).

The definition of the resampler (a Kaiser-windowed sinc with this project's own fixed parameters) is in
`include/msmd_hip.h` and DESIGN.md 5.12; the arithmetic runs in `csrc/audio_io.hip`.  This module parses files on the host,
builds the polyphase table in float64 and moves raw PCM to the device at its compact size.  There is no CPU resampler.
"""
from __future__ import annotations

import functools
import math
import os
import struct
from collections import namedtuple

import numpy as np

RATE_OUT = 16000
ZERO_CROSSINGS = 64
KAISER_BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596
MAX_L = 640
_LDS_SPAN_BYTES = 65536          # msmd_audio_resample stages one run's input span in at most this much LDS

FilterBank = namedtuple("FilterBank", "L M taps half table")    # table (taps, L) float32, or None when the rates are equal


# ----------------------------------------------------------------------------- WAV files
def _sample_format(tag, bits, path):
    if tag == 1 and bits in (8, 16, 24, 32):
        return
    if tag == 3 and bits in (32, 64):
        return
    if tag in (1, 3):
        raise ValueError(f"{path}: {bits}-bit samples with format tag {tag} are not supported")
    raise ValueError(f"{path}: compressed or unknown WAV format tag 0x{tag:04x} (PCM and IEEE float only)")


def read_wav(path):
    """-> (pcm (frames, channels), rate).  pcm is int16 for 16-bit PCM and float32 in [-1, 1) otherwise: unsigned 8-bit as
    (b - 128) / 128, 24-bit / 2^23, 32-bit / 2^31, float32 as stored, float64 rounded.  A RIFF chunk walker of our own (the
    `wave` module reads neither float nor extensible files): unknown chunks are skipped, odd-sized chunks are padded to even,
    a `data` length of 0, 0xFFFFFFFF or past the end of the file means "to the end of the file", a truncated last frame is
    dropped.  RF64, compressed formats, zero channels, zero frames and a missing `fmt ` / `data` chunk raise ValueError."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) >= 4 and blob[:4] in (b"RF64", b"BW64"):
        raise ValueError(f"{path}: RF64 files are not supported")
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = data = None
    pos = 12
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack_from("<I", blob, pos + 4)[0]
        body = pos + 8
        if cid == b"data":
            end = body + size
            if size in (0, 0xFFFFFFFF) or end > len(blob):
                end = len(blob)
            data = (body, end)
            break                                   # samples run to the chunk's end; nothing behind them is needed
        if cid == b"fmt ":
            if size < 16 or body + 16 > len(blob):
                raise ValueError(f"{path}: `fmt ` chunk of {size} bytes is too short")
            tag, channels, rate, _, _, bits = struct.unpack_from("<HHIIHH", blob, body)
            if tag == 0xFFFE:                       # WAVE_FORMAT_EXTENSIBLE: the sub-format GUID's first two bytes are the tag
                if size < 40 or body + 40 > len(blob):
                    raise ValueError(f"{path}: extensible `fmt ` chunk of {size} bytes is too short")
                tag = struct.unpack_from("<H", blob, body + 24)[0]
            fmt = (tag, channels, rate, bits)
        pos = body + size + (size & 1)
    if fmt is None:
        raise ValueError(f"{path}: no `fmt ` chunk before the samples")
    if data is None:
        raise ValueError(f"{path}: no `data` chunk")
    tag, channels, rate, bits = fmt
    _sample_format(tag, bits, path)
    if channels == 0:
        raise ValueError(f"{path}: zero channels")
    if rate == 0:
        raise ValueError(f"{path}: sample rate 0")
    width = bits // 8
    frames = (data[1] - data[0]) // (width * channels)
    if frames == 0:
        raise ValueError(f"{path}: zero frames")
    raw = np.frombuffer(blob, dtype=np.uint8, count=frames * channels * width, offset=data[0])
    if tag == 3:
        pcm = raw.view("<f4" if bits == 32 else "<f8").astype(np.float32)
    elif bits == 16:
        pcm = raw.view("<i2").astype(np.int16)
    elif bits == 8:
        pcm = (raw.astype(np.float32) - np.float32(128)) / np.float32(128)
    elif bits == 24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)             # sign extension
        pcm = (v.astype(np.float64) / float(1 << 23)).astype(np.float32)
    else:
        pcm = (raw.view("<i4").astype(np.float64) / float(1 << 31)).astype(np.float32)
    return np.ascontiguousarray(pcm.reshape(frames, channels)), int(rate)


def write_wav(path, samples, rate=RATE_OUT):
    """Mono float32 WAV (format tag 3): what `read_wav` returns bit for bit.  samples: 1-D array or tensor."""
    if hasattr(samples, "detach"):
        samples = samples.detach().cpu().numpy()
    x = np.ascontiguousarray(np.asarray(samples, dtype="<f4"))
    if x.ndim != 1:
        raise ValueError(f"write_wav takes 1-D mono samples, got shape {x.shape}")
    n = x.size * 4
    if n > 0xFFFFFFFF - 36:
        raise ValueError("write_wav: more than 4 GiB of samples does not fit a RIFF file")
    head = b"RIFF" + struct.pack("<I", 36 + n) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 3, 1, int(rate), int(rate) * 4, 4, 32)
    with open(os.fspath(path), "wb") as f:
        f.write(head + b"data" + struct.pack("<I", n))
        f.write(x.tobytes())


# ----------------------------------------------------------------------------- the filter
def rate_ratio(rate_in, rate_out=RATE_OUT):
    """-> (L, M) = (rate_out, rate_in) / gcd; ValueError for a rate the front end does not take."""
    if int(rate_in) != rate_in or rate_in <= 0:
        raise ValueError(f"unsupported sample rate {rate_in!r}")
    g = math.gcd(int(rate_in), int(rate_out))
    L, M = int(rate_out) // g, int(rate_in) // g
    if L > MAX_L:
        raise ValueError(f"unsupported sample rate {rate_in} Hz: {rate_out}/{rate_in} reduces to {L}/{M}, more than {MAX_L} filter phases")
    return L, M


def kaiser_sinc(t, L, M):
    """h(t) of DESIGN.md 5.12 in float64, t in input samples (any shape)."""
    s = ROLLOFF * min(1.0, L / M)
    u = s * np.asarray(t, dtype=np.float64)
    w = u / ZERO_CROSSINGS
    inside = np.abs(u) < ZERO_CROSSINGS
    win = np.i0(KAISER_BETA * np.sqrt(np.clip(1.0 - w * w, 0.0, None))) / np.i0(KAISER_BETA)
    return np.where(inside, s * np.sinc(u) * win, 0.0)


@functools.lru_cache(maxsize=None)
def filter_bank(rate_in, rate_out=RATE_OUT):
    """The polyphase table of one rate pair, built once in float64 and stored as float32: table[i, r] =
    h(((r M) mod L) / L - (i - half)), taps = 2 ceil(64 / s) + 2 rows, half = taps / 2 - 1.  Tap-major over the output's phase
    order r = n mod L: output n reads row i at column n mod L, so adjacent outputs read adjacent addresses.  Output n is
    sum_i x[n M div L + i - half] table[i, n mod L]."""
    L, M = rate_ratio(rate_in, rate_out)
    if L == M:
        return FilterBank(1, 1, 0, 0, None)
    s = ROLLOFF * min(1.0, L / M)
    half = math.ceil(ZERO_CROSSINGS / s)
    taps = 2 * half + 2
    if (((255 * M) // L) + 2 + taps) * 4 > _LDS_SPAN_BYTES:
        raise ValueError(f"unsupported sample rate {rate_in} Hz: a run's input span at {L}/{M} does not fit the staging buffer")
    phase = (np.arange(L, dtype=np.int64) * M) % L
    j = np.arange(taps, dtype=np.int64) - half
    num = phase[None, :] - j[:, None] * L                        # exact integer numerator of t = phase / L - j
    table = kaiser_sinc(num.astype(np.float64) / L, L, M).astype(np.float32)
    table.setflags(write=False)
    return FilterBank(L, M, taps, half, table)


def output_length(frames, L, M):
    return (int(frames) * L + M - 1) // M


@functools.lru_cache(maxsize=None)
def _device_bank(rate_in, rate_out, device):
    import torch
    fb = filter_bank(rate_in, rate_out)
    return None if fb.table is None else torch.from_numpy(fb.table.copy()).to(device)


# ----------------------------------------------------------------------------- files / arrays -> device tensors
def _as_pcm(src, rate):
    if isinstance(src, (str, os.PathLike)):
        return read_wav(src)
    if rate is None:
        raise ValueError("load_clips: an array source needs its sample rate in `rates`")
    a = np.asarray(src)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError(f"load_clips: samples must be 1-D or (frames, channels) and not empty, got shape {a.shape}")
    if a.dtype != np.int16:
        a = a.astype(np.float32)
    return np.ascontiguousarray(a), int(rate)


def load_clips(sources, device="cuda", normalize=True, rates=None):
    """WAV paths, or arrays ((frames, channels) or 1-D; int16 or floating) with their rates in `rates`, -> one 1-D float32
    device tensor of 16 kHz mono samples per source, in input order: what `infer_coeffs_batch` takes as `audios`.
    normalize: (y - mean) / (std + 1e-5) per clip.  Clips are grouped by (rate, sample type); a group is one pinned staging
    buffer (descriptors, then the interleaved PCM as it is), one host-to-device copy and three launches (one if not normalize).
    A clip's result does not depend on what else is in the call."""
    import torch
    from .. import ops
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("load_clips needs the MI355X (cuda) device; there is no CPU path")
    sources = list(sources)
    rates = [None] * len(sources) if rates is None else list(rates)
    if len(rates) != len(sources):
        raise ValueError(f"load_clips: {len(sources)} sources but {len(rates)} rates")
    clips = [_as_pcm(s, r) for s, r in zip(sources, rates)]
    groups = {}
    for i, (pcm, rate) in enumerate(clips):
        filter_bank(rate)                                        # raises ValueError, naming the rate, before any copy
        groups.setdefault((rate, pcm.dtype == np.int16), []).append(i)
    result = [None] * len(clips)
    pieces = [(key, members[a:a + ops.AUDIO_MAX_CLIPS]) for key, members in groups.items()
              for a in range(0, len(members), ops.AUDIO_MAX_CLIPS)]           # an entry point takes that many clips per call
    for (rate, is_int16), members in pieces:
        fb = filter_bank(rate)
        width = 2 if is_int16 else 4
        desc = np.zeros((len(members), 5), np.int64)
        in_off = out_off = 0
        for row, i in enumerate(members):
            frames, channels = clips[i][0].shape
            n_out = output_length(frames, fb.L, fb.M)
            desc[row] = (in_off, frames, channels, out_off, n_out)
            in_off += frames * channels
            out_off += n_out
        head = (desc.nbytes + 15) // 16 * 16
        stage = torch.empty(head + in_off * width, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        host[:desc.nbytes] = desc.reshape(-1).view(np.uint8)
        for row, i in enumerate(members):
            a, b = head + int(desc[row, 0]) * width, head + (int(desc[row, 0]) + clips[i][0].size) * width
            host[a:b] = clips[i][0].reshape(-1).view(np.uint8)
        dev = stage.to(device, non_blocking=True)
        desc_dev = dev[:desc.nbytes].view(torch.int64).view(len(members), 5)
        pcm_dev = dev[head:].view(torch.int16 if is_int16 else torch.float32)
        out, partials = ops.resample_audio(pcm_dev, desc_dev, desc, _device_bank(rate, RATE_OUT, device), fb.L, fb.M)
        if normalize:
            ops.znorm_audio(out, desc_dev, desc, partials)
        for row, i in enumerate(members):
            result[i] = out[int(desc[row, 3]):int(desc[row, 3] + desc[row, 4])]
    return result
