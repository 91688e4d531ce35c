"""Host side of the audio front end (utils/audio.py) and its numpy truth (tests/audio_ref.py): the WAV parser on files written
here with `struct` / `wave`, the polyphase table against the filter in closed form and against direct evaluation, output
lengths, and what the stated filter does to tones.  No GPU."""
import struct
import wave

import numpy as np
import pytest

import audio_ref as ar
from msmd_amd.utils import audio

RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000)
TAPS = {44100: 376, 48000: 408, 32000: 274, 22050: 190, 8000: 138, 11025: 138}       # 2 ceil(64 / s) + 2


def rng(tag):
    return np.random.default_rng(sum(map(ord, tag)) * 7919)


# ----------------------------------------------------------------------------- WAV files
def chunk(cid, body, size=None):
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def fmt_body(tag, channels, rate, bits, extensible=False):
    block = channels * bits // 8
    base = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block, block, bits)
    if not extensible:
        return base
    guid_tail = bytes.fromhex("000000001000800000aa00389b71")
    return base + struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + guid_tail


def riff(path, chunks, form=b"RIFF"):
    body = b"WAVE" + b"".join(chunks)
    path.write_bytes(form + struct.pack("<I", len(body)) + body)
    return path


def encode(values, kind):
    """values float64 in [-1, 1) on the format's own grid -> (bytes, tag, bits, expected array as read_wav returns it)."""
    v = np.asarray(values)
    if kind == "u8":
        q = np.round(v * 128).astype(np.int64) + 128
        return q.astype(np.uint8).tobytes(), 1, 8, ((q - 128) / 128).astype(np.float32)
    if kind == "i16":
        q = np.round(v * 32768).astype(np.int16)
        return q.astype("<i2").tobytes(), 1, 16, q
    if kind == "i24":
        q = np.round(v * (1 << 23)).astype(np.int64)
        raw = b"".join(struct.pack("<i", int(s))[:3] for s in q.reshape(-1))
        return raw, 1, 24, (q / float(1 << 23)).astype(np.float32)
    if kind == "i32":
        q = np.round(v * (1 << 31)).astype(np.int64)
        return q.astype("<i4").tobytes(), 1, 32, (q / float(1 << 31)).astype(np.float32)
    if kind == "f32":
        return v.astype("<f4").tobytes(), 3, 32, v.astype(np.float32)
    if kind == "f64":
        return v.astype("<f8").tobytes(), 3, 64, v.astype(np.float32)
    raise KeyError(kind)


def samples(frames, channels, tag):
    v = rng(tag).uniform(-1, 1, size=(frames, channels))
    v[0, 0], v[-1, -1] = -1.0, 0.0
    return np.clip(v, -1.0, 1.0 - 2.0 ** -7)


@pytest.mark.parametrize("kind", ["u8", "i16", "i24", "i32", "f32", "f64"])
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("extensible", [False, True])
def test_read_wav_round_trips_every_sample_format(tmp_path, kind, channels, extensible):
    v = samples(37, channels, f"{kind}{channels}")
    raw, tag, bits, want = encode(v, kind)
    p = riff(tmp_path / "a.wav", [chunk(b"fmt ", fmt_body(tag, channels, 22050, bits, extensible)), chunk(b"data", raw)])
    pcm, rate = audio.read_wav(p)
    assert rate == 22050 and pcm.shape == (37, channels)
    assert pcm.dtype == (np.int16 if kind == "i16" else np.float32)
    assert np.array_equal(pcm, want.reshape(37, channels))
    assert pcm.min() >= -1.0 if kind != "i16" else pcm.min() == -32768      # the negative full scale survives


def test_read_wav_sign_extends_24_bit_and_centres_8_bit(tmp_path):
    raw24 = bytes([0xff, 0xff, 0xff, 0x00, 0x00, 0x80, 0xff, 0xff, 0x7f, 0x01, 0x00, 0x00])
    p = riff(tmp_path / "a.wav", [chunk(b"fmt ", fmt_body(1, 1, 8000, 24)), chunk(b"data", raw24)])
    assert audio.read_wav(p)[0][:, 0].tolist() == [-(2.0 ** -23), -1.0, 1.0 - 2.0 ** -23, 2.0 ** -23]
    p = riff(tmp_path / "b.wav", [chunk(b"fmt ", fmt_body(1, 1, 8000, 8)), chunk(b"data", bytes([0, 128, 255, 64]))])
    assert audio.read_wav(p)[0][:, 0].tolist() == [-1.0, 0.0, 127 / 128, -0.5]


@pytest.mark.parametrize("width", [1, 2])
def test_read_wav_reads_what_the_wave_module_writes(tmp_path, width):
    v = samples(50, 2, f"wave{width}")
    raw, _, bits, want = encode(v, "u8" if width == 1 else "i16")
    with wave.open(str(tmp_path / "w.wav"), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(width)
        w.setframerate(44100)
        w.writeframes(raw)
    pcm, rate = audio.read_wav(tmp_path / "w.wav")
    assert rate == 44100 and np.array_equal(pcm, want.reshape(50, 2))


def test_read_wav_skips_unknown_and_odd_sized_chunks(tmp_path):
    raw, tag, bits, want = encode(samples(20, 2, "list"), "i16")
    p = riff(tmp_path / "a.wav", [chunk(b"JUNK", b"\1\2\3\4"), chunk(b"fmt ", fmt_body(tag, 2, 48000, bits)),
                                  chunk(b"LIST", b"INFOabc"), chunk(b"data", raw), chunk(b"cue ", b"\0" * 5)])
    pcm, rate = audio.read_wav(p)
    assert rate == 48000 and np.array_equal(pcm, want.reshape(20, 2))


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF, 10 ** 6])
def test_read_wav_clips_a_wrong_data_length_to_the_file(tmp_path, size):
    raw, tag, bits, want = encode(samples(20, 2, "stream"), "i16")
    p = riff(tmp_path / "a.wav", [chunk(b"fmt ", fmt_body(tag, 2, 16000, bits)), chunk(b"data", raw, size=size)])
    assert np.array_equal(audio.read_wav(p)[0], want.reshape(20, 2))


def test_read_wav_drops_a_truncated_last_frame(tmp_path):
    raw, tag, bits, want = encode(samples(20, 3, "trunc"), "i24")
    p = riff(tmp_path / "a.wav", [chunk(b"fmt ", fmt_body(tag, 3, 16000, bits)), chunk(b"data", raw[:-4])])
    assert np.array_equal(audio.read_wav(p)[0], want.reshape(20, 3)[:19])


def test_read_wav_errors(tmp_path):
    raw, tag, bits, _ = encode(samples(8, 1, "err"), "i16")
    fmt, data = chunk(b"fmt ", fmt_body(tag, 1, 16000, bits)), chunk(b"data", raw)
    cases = {
        "rf64": lambda p: riff(p, [fmt, data], form=b"RF64"),
        "not_riff": lambda p: p.write_bytes(b"OggS" + b"\0" * 40),
        "mu_law": lambda p: riff(p, [chunk(b"fmt ", fmt_body(7, 1, 8000, 8)), data]),
        "adpcm_extensible": lambda p: riff(p, [chunk(b"fmt ", fmt_body(2, 1, 8000, 16, True)), data]),
        "pcm_12_bit": lambda p: riff(p, [chunk(b"fmt ", fmt_body(1, 1, 8000, 12)), data]),
        "float_16_bit": lambda p: riff(p, [chunk(b"fmt ", fmt_body(3, 1, 8000, 16)), data]),
        "zero_channels": lambda p: riff(p, [chunk(b"fmt ", fmt_body(1, 0, 8000, 16)), data]),
        "zero_frames": lambda p: riff(p, [fmt, chunk(b"data", b"\0")]),
        "no_fmt": lambda p: riff(p, [data]),
        "fmt_after_data": lambda p: riff(p, [data, fmt]),
        "no_data": lambda p: riff(p, [fmt, chunk(b"LIST", b"INFO")]),
        "short_fmt": lambda p: riff(p, [chunk(b"fmt ", b"\1\0\1\0"), data]),
    }
    for name, make in cases.items():
        p = tmp_path / f"{name}.wav"
        make(p)
        with pytest.raises(ValueError):
            audio.read_wav(p)


def test_write_wav_then_read_wav_is_exact(tmp_path):
    x = rng("write").standard_normal(1001).astype(np.float32)
    x[:3] = [np.float32(1e-41), -0.0, 3.0]              # a denormal, a signed zero and a value past full scale survive
    audio.write_wav(tmp_path / "o.wav", x, 16000)
    pcm, rate = audio.read_wav(tmp_path / "o.wav")
    assert rate == 16000 and pcm.shape == (1001, 1) and pcm.dtype == np.float32
    assert np.array_equal(pcm[:, 0].view(np.uint32), x.view(np.uint32))
    head = (tmp_path / "o.wav").read_bytes()[:44]
    assert head[:4] == b"RIFF" and struct.unpack_from("<I", head, 4)[0] == 36 + 4 * 1001 and head[20:22] == b"\3\0"
    with pytest.raises(ValueError):
        audio.write_wav(tmp_path / "s.wav", np.zeros((4, 2), np.float32))


# ----------------------------------------------------------------------------- the filter and its table
@pytest.mark.parametrize("rate", RATES)
def test_filter_bank_is_the_filter_in_closed_form(rate):
    fb = audio.filter_bank(rate)
    L, M = ar.ratio(rate)
    s = ar.ROLLOFF * min(1.0, L / M)
    assert (fb.L, fb.M) == (L, M) and L <= 640
    assert fb.half == int(np.ceil(64 / s)) and fb.taps == 2 * fb.half + 2
    assert fb.table.shape == (fb.taps, L) and fb.table.dtype == np.float32
    if rate in TAPS:
        assert fb.taps == TAPS[rate]
    r = np.arange(L)
    phase = (r * M) % L
    t = phase[None, :] / L - (np.arange(fb.taps)[:, None] - fb.half)
    want = ar.h(t, L, M)
    assert np.array_equal(fb.table, want.astype(np.float32))
    # the closed form written out once more, independent of audio_ref.h, at a few points
    for i, c in ((fb.half, 0), (fb.half + 3, L // 2), (5, L - 1)):
        u = s * t[i, c]
        val = s * (1.0 if u == 0 else np.sin(np.pi * u) / (np.pi * u)) * np.i0(ar.BETA * np.sqrt(1 - (u / 64) ** 2)) / np.i0(ar.BETA)
        assert abs(float(fb.table[i, c]) - val) <= 2.0 ** -24 * abs(val) + 1e-30
    assert fb.table[fb.half, 0] == np.float32(s)                  # h(0) = s: no per-phase renormalisation
    # every tap the definition makes non-zero is inside the table: the first and last rows are all outside the window
    assert not fb.table[0].any() and not fb.table[-1, phase == 0].any()
    assert np.all(np.abs(s * (phase / L + fb.half)) >= 64) and np.all(np.abs(s * (phase / L - fb.half - 1))[phase == 0] >= 64)


@pytest.mark.parametrize("rate", RATES)
def test_filter_bank_symmetry(rate):
    """h is even: the column of phase p read forwards is the column of phase L - p read backwards (one row apart), and the
    phase-0 column is symmetric about its centre tap."""
    fb = audio.filter_bank(rate)
    L, M, T, half = fb.L, fb.M, fb.table.astype(np.float64), fb.half
    col = {int((r * M) % L): r for r in range(L)}
    c0 = T[:, col[0]]
    assert np.array_equal(c0[1:2 * half], c0[1:2 * half][::-1])
    for p in sorted(set(sorted(col)[1:4] + sorted(col)[-2:]) - {0}):
        a, b = T[:, col[p]], T[:, col[L - p]]
        # h(p/L - (i - half)) = h((L-p)/L - (i' - half)) with i' = 2 half + 1 - i
        ii = np.arange(fb.taps)
        assert np.allclose(a[ii], b[2 * half + 1 - ii], rtol=0, atol=2.0 ** -24 * np.abs(a).max())


def test_filter_bank_same_rate_and_unsupported_rates():
    fb = audio.filter_bank(16000)
    assert fb.table is None and fb.taps == 0 and (fb.L, fb.M) == (1, 1)
    for bad in (44101, 16001, 7999, 1):
        with pytest.raises(ValueError, match=str(bad)):
            audio.filter_bank(bad)
    with pytest.raises(ValueError, match="16000000"):
        audio.filter_bank(16000000)                               # L = 1, but a run's span no longer fits the staging buffer
    with pytest.raises(ValueError):
        audio.filter_bank(0)
    assert audio.filter_bank(48000) is audio.filter_bank(48000)  # cached per rate pair


def table_resample(x, rate):
    """y from the polyphase table, in float64 of the float64 table (rebuilt here: the stored one is rounded to float32)."""
    fb = audio.filter_bank(rate)
    L, M, half, taps = fb.L, fb.M, fb.half, fb.taps
    phase = (np.arange(L) * M) % L
    T = ar.h(phase[None, :] / L - (np.arange(taps)[:, None] - half), L, M)
    n = np.arange(audio.output_length(len(x), L, M))
    k0 = (n * M) // L
    xp = np.concatenate([np.zeros(half), x, np.zeros(taps)])
    y = np.zeros(len(n))
    for i in range(taps):
        y += xp[k0 + i] * T[i, n % L]
    return y, T


@pytest.mark.parametrize("rate", [44100, 48000, 32000, 22050, 11025, 8000])
def test_polyphase_table_reproduces_direct_evaluation(rate):
    x = rng(f"direct{rate}").standard_normal(700)
    y, T = table_resample(x, rate)
    ref = ar.resample_ref(x, rate)
    assert y.shape == ref.shape
    err = np.abs(y - ref).max()
    print(f"rate {rate}: table vs direct evaluation {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("rate", [44100, 48000, 8000, 11025])
def test_polyphase_table_matches_scipy_upfirdn(rate):
    signal = pytest.importorskip("scipy.signal")
    L, M = ar.ratio(rate)
    fb = audio.filter_bank(rate)
    x = rng(f"scipy{rate}").standard_normal(500)
    # the prototype filter on the L-times upsampled grid: g[m] = h((m - c) / L), c = (half + 1) L; upfirdn zero-stuffs by L,
    # filters and keeps every M-th sample, so its output c / M + n ... only when M divides c; take an offset that does
    c = (fb.half + 1) * L
    g = ar.h((np.arange(2 * c + 1) - c) / L, L, M)
    full = signal.upfirdn(g, x, up=L, down=1)                     # full[m] = sum_k x[k] g[m - k L]
    n = np.arange(audio.output_length(len(x), L, M))
    got = full[c + n * M]
    y, _ = table_resample(x, rate)
    assert np.abs(got - y).max() <= 1e-13


@pytest.mark.parametrize("rate", [48000, 44100, 8000, 11025, 22050])
def test_output_length_is_ceil(rate):
    L, M = ar.ratio(rate)
    for N in [1, 2, 3] + [M * k + d for k in (1, 2, 7) for d in (-1, 0, 1)]:
        want = int(np.ceil(N * L / M))
        assert audio.output_length(N, L, M) == want == ar.out_len(N, L, M)
        assert ar.resample_ref(np.zeros(N), rate).shape == (want,)
    # 64-bit: an hour at 192 kHz
    assert audio.output_length(3600 * 192000, *ar.ratio(192000)) == 3600 * 16000


# ----------------------------------------------------------------------------- what the filter does
def tone_gain_db(rate, f):
    N = int(0.12 * rate)
    x = np.sin(2 * np.pi * f * np.arange(N) / rate)
    y, _ = table_resample(x, rate)
    mid = y[len(y) // 4:len(y) * 3 // 4]
    return 20 * np.log10(max(np.sqrt(2 * np.mean(mid ** 2)), 1e-300))


@pytest.mark.parametrize("rate", [44100, 48000])
def test_tones_pass_below_and_vanish_above_the_band_edge(rate):
    for f in (1000, 7000):
        g = tone_gain_db(rate, f)
        print(f"rate {rate}: {f} Hz passes at {g:+.4f} dB")
        assert abs(g) <= 0.05
    for f in (9000, 12000):
        g = tone_gain_db(rate, f)
        print(f"rate {rate}: {f} Hz comes out at {g:.1f} dB")
        assert g < -120


def test_same_rate_bypass_is_exact_and_downmix_order():
    x = rng("bypass").standard_normal(300).astype(np.float32)
    assert np.array_equal(ar.resample_ref(x, 16000, np.float32), x)
    pcm = np.array([[32767, -32768, 1], [3, 3, 4]], np.int16)
    want = [np.float32(np.float32(np.float32(32767 / 32768) + np.float32(-1.0)) + np.float32(2.0 ** -15)) / np.float32(3),
            np.float32(10 / 32768) / np.float32(3)]
    assert ar.downmix_ref(pcm, np.float32).tolist() == want
    assert ar.downmix_ref(pcm[:, :2], np.float64).tolist() == [-(2.0 ** -16), 3 / 32768]
    z = ar.znorm_ref(np.arange(5.0))
    assert abs(z.mean()) < 1e-15 and abs(z.std() - 1) < 1e-5
