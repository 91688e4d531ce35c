"""The HIP audio front end (csrc/audio_io.hip, utils/audio.load_clips) against the numpy truth of tests/audio_ref.py.

Stage by stage against float64: error |g - g64| / max(1, |g64|) must be <= max(16 u, 4 x yardstick), u = 2^-24, the yardstick
being the same direct evaluation with float32 taps, products and sums on the same input (4-9 u for unit-scale noise on the CPU;
the factor 4 allows for another summation order).  Every test prints the kernel's maximum and the yardstick's (`pytest -s`).

Clips are at most 0.25 s long, with two exceptions made on purpose: `test_positions_past_two_to_the_31` uploads one 306 s clip
(27 MB of int16), the smallest at which n M leaves 32 bits and so the only check that would catch 32-bit positions, and
`test_more_clips_than_one_launch_takes` sends 65 537 one-frame clips, one more than an entry point takes per call.

DESIGN.md 5.12 has the bound table."""
import functools
import wave

import numpy as np
import pytest
import torch

import audio_ref as ar
from msmd_amd import ops
from msmd_amd.utils import audio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
RUN = ops.AUDIO_RUN
RATES = (48000, 44100, 8000, 11025, 16000)
KINDS = [(1, "f32"), (2, "i16"), (3, "f32"), (1, "i16"), (2, "f32"), (3, "i16"), (2, "full")]


def rng(tag):
    return np.random.default_rng(sum(map(ord, tag)) * 7919)


def make_pcm(frames, channels, kind, tag, scale=1.0):
    r = rng(f"{tag}/{frames}/{channels}/{kind}")
    if kind == "f32":
        return (scale * r.standard_normal((frames, channels))).astype(np.float32)
    if kind == "full":                                            # int16 at +- full scale
        return np.where(r.random((frames, channels)) < 0.5, -32768, 32767).astype(np.int16)
    return r.integers(-32768, 32768, size=(frames, channels)).astype(np.int16)


def frames_for(outputs, L, M):
    """The fewest input frames that give at least `outputs` output samples."""
    n = max(1, (outputs - 1) * M // L)
    while ar.out_len(n, L, M) < outputs:
        n += 1
    return n


def lengths(rate):
    L, M = ar.ratio(rate)
    k = 7
    ns = [1, 2, 50, M * k - 1, M * k, M * k + 1]
    around = [frames_for(t, L, M) for t in (RUN - 1, RUN, RUN + 1, 2 * RUN + 3)]
    return ns + around + [frames_for(RUN, L, M) - 1]


def references(pcm, rate):
    g64 = ar.resample_ref(ar.downmix_ref(pcm, np.float64), rate, np.float64)
    y32 = ar.resample_ref(ar.downmix_ref(pcm, np.float32), rate, np.float32)
    return g64, y32


def rel_err(g, g64):
    return float(np.max(np.abs(np.asarray(g, np.float64) - g64) / np.maximum(1.0, np.abs(g64))))


@functools.lru_cache(maxsize=None)
def stage(rate):
    """All of one rate's clips (every length of `lengths`, the sample kinds in rotation) through load_clips without and with
    z-norm, and their references; computed once and shared, nothing below modifies it."""
    clips = [make_pcm(n, *KINDS[i % len(KINDS)], tag=f"stage{rate}") for i, n in enumerate(lengths(rate))]
    # every kind at the length the tap windows are clipped at both ends (50 frames is shorter than the filter's half width)
    clips += [make_pcm(50, c, kind, tag=f"short{rate}") for c, kind in KINDS]
    raw = audio.load_clips(clips, DEV, normalize=False, rates=[rate] * len(clips))
    zn = audio.load_clips(clips, DEV, normalize=True, rates=[rate] * len(clips))
    torch.cuda.synchronize()
    refs = [references(p, rate) for p in clips]
    return clips, [t.cpu().numpy() for t in raw], [t.cpu().numpy() for t in zn], refs


def test_case_lengths_cover_the_run_boundaries():
    for rate in RATES:
        L, M = ar.ratio(rate)
        outs = sorted({ar.out_len(n, L, M) for n in lengths(rate)})
        assert any(RUN - 3 <= o < RUN for o in outs) and RUN in outs and any(RUN < o <= RUN + 2 for o in outs)
        assert any(2 * RUN + 3 <= o <= 2 * RUN + 4 for o in outs)
        assert 50 < audio.filter_bank(rate).half or rate == 16000


@pytest.mark.parametrize("rate", RATES)
def test_resample_stage_against_float64(rate):
    clips, raw, _, refs = stage(rate)
    L, M = ar.ratio(rate)
    worst = worst_y = 0.0
    for pcm, g, (g64, y32) in zip(clips, raw, refs):
        assert g.dtype == np.float32 and g.shape == (ar.out_len(pcm.shape[0], L, M),)
        if rate == 16000:
            assert np.array_equal(g, ar.downmix_ref(pcm, np.float32)), "the same-rate path is the exact downmix"
        err, yard = rel_err(g, g64), rel_err(y32, g64)
        worst, worst_y = max(worst, err), max(worst_y, yard)
        assert err <= max(16 * U, 4 * yard), (pcm.shape, str(pcm.dtype), err / U, yard / U)
    print(f"resample {rate} Hz: kernel max {worst / U:.2f} u, float32 yardstick max {worst_y / U:.2f} u over {len(clips)} clips")


@pytest.mark.parametrize("rate", RATES)
def test_znorm_pipeline_against_float64(rate):
    clips, _, zn, refs = stage(rate)
    worst = worst_y = 0.0
    n = 0
    for pcm, g, (g64, y32) in zip(clips, zn, refs):
        if g64.std() < 0.1 or g64.size < 2:
            continue
        n += 1
        z64, z32 = ar.znorm_ref(g64, np.float64), ar.znorm_ref(y32, np.float32)
        err, yard = rel_err(g, z64), rel_err(z32, z64)
        worst, worst_y = max(worst, err), max(worst_y, yard)
        assert err <= max(16 * U, 4 * yard), (pcm.shape, str(pcm.dtype), err / U, yard / U)
    assert n >= 10
    print(f"z-norm {rate} Hz: kernel max {worst / U:.2f} u, float32 yardstick max {worst_y / U:.2f} u over {n} clips")


def test_znorm_constant_clip_and_moments():
    const = np.full((1000, 2), 1234, np.int16)
    # (y - mean) / (std + 1e-5) has std = s / (s + 1e-5): within 1e-5 of 1 needs s > 1, so the noise is scaled to std 4
    loud = make_pcm(4000, 2, "f32", "moments", scale=4.0 * np.sqrt(2))
    outs = audio.load_clips([const, loud, loud[:3001]], DEV, rates=[16000, 48000, 44100])
    z = [t.cpu().numpy().astype(np.float64) for t in outs]
    assert z[0].shape == (1000,) and not z[0].any(), "a constant clip normalises to zeros"
    for y in z[1:]:
        print(f"z-norm moments: mean {y.mean():+.2e}, std - 1 {y.std() - 1:+.2e}")
        assert abs(y.mean()) <= 1e-5 and abs(y.std() - 1.0) <= 1e-5


@pytest.mark.parametrize("rate,channels,kind", [(44100, 2, "i16"), (8000, 3, "f32"), (16000, 1, "i16")])
def test_a_clip_has_the_same_bits_alone_and_in_any_batch(rate, channels, kind):
    L, M = ar.ratio(rate)
    clip = make_pcm(frames_for(2 * RUN + 3, L, M), channels, kind, "member")
    others = [make_pcm(n, channels, kind, f"other{i}") for i, n in
              enumerate((1, frames_for(RUN, L, M), 50, frames_for(3 * RUN + 1, L, M), 777, 2))]
    for normalize in (False, True):
        alone = audio.load_clips([clip], DEV, normalize=normalize, rates=[rate])[0].clone()
        for pos in (0, 3, 6):
            batch = others[:pos] + [clip] + others[pos:]
            a = audio.load_clips(batch, DEV, normalize=normalize, rates=[rate] * 7)
            b = audio.load_clips(batch, DEV, normalize=normalize, rates=[rate] * 7)
            assert len(a) == 7 and torch.equal(a[pos], alone), (normalize, pos)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), "two runs of one batch give the same bits"
            assert all(t.shape == (ar.out_len(p.shape[0], L, M),) for t, p in zip(a, batch))


def write_int16_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def test_load_clips_from_files_keeps_input_order(tmp_path):
    a = make_pcm(3000, 2, "i16", "file_a")
    b = make_pcm(2500, 1, "f32", "file_b", scale=0.3)
    c = make_pcm(1700, 1, "i16", "file_c")
    write_int16_wav(tmp_path / "a.wav", a, 44100)
    audio.write_wav(tmp_path / "b.wav", b[:, 0], 48000)
    write_int16_wav(tmp_path / "c.wav", c, 16000)
    paths = [tmp_path / "a.wav", str(tmp_path / "b.wav"), tmp_path / "c.wav"]
    for normalize in (False, True):
        got = audio.load_clips(paths, DEV, normalize=normalize)
        for g, path, pcm, rate in zip(got, paths, (a, b, c), (44100, 48000, 16000)):
            assert g.dim() == 1 and g.dtype == torch.float32 and g.is_cuda
            assert torch.equal(g, audio.load_clips([path], DEV, normalize=normalize)[0])
            assert torch.equal(g, audio.load_clips([pcm], DEV, normalize=normalize, rates=[rate])[0])
    # a mixed call with an array in it, and the errors
    mixed = audio.load_clips([c[:, 0], paths[0]], DEV, normalize=False, rates=[16000, None])
    assert torch.equal(mixed[1], audio.load_clips(paths[:1], DEV, normalize=False)[0])
    assert np.array_equal(mixed[0].cpu().numpy(), ar.downmix_ref(c, np.float32))
    with pytest.raises(ValueError, match="44101"):
        audio.load_clips([a], DEV, rates=[44101])
    with pytest.raises(ValueError):
        audio.load_clips([a], DEV)


def test_load_audio_16k_reads_wav_and_still_reads_npy(tmp_path):
    from msmd_amd import inference
    pcm = make_pcm(4000, 2, "i16", "load16k")
    write_int16_wav(tmp_path / "speech.wav", pcm, 44100)
    got = inference.load_audio_16k(tmp_path / "speech.wav")
    g64, y32 = references(pcm, 44100)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == g64.shape
    err, yard = rel_err(got, g64), rel_err(y32, g64)
    print(f"load_audio_16k: kernel {err / U:.2f} u, yardstick {yard / U:.2f} u")
    assert err <= max(16 * U, 4 * yard)
    x = rng("npy").standard_normal(321)
    np.save(tmp_path / "decoded.npy", x)
    back = inference.load_audio_16k(str(tmp_path / "decoded.npy"))
    assert back.dtype == np.float32 and np.array_equal(back, x.astype(np.float32))


def test_positions_past_two_to_the_31():
    """n M passes 2^31 at output 4 869 546 of a 44.1 kHz clip (M = 441): the tail of a 306 s clip against float64.  The
    reference is evaluated on the clip's last 2 328 frames only: cutting the input at a multiple of M frames keeps every
    phase, and outputs further than the filter's half width from the cut do not see it."""
    L, M = ar.ratio(44100)
    q_all, q_tail = 30600, 5                                     # blocks of M frames / L outputs
    pcm = rng("long").integers(-32768, 32768, size=(q_all * M + 123, 1)).astype(np.int16)
    g = audio.load_clips([pcm], DEV, normalize=False, rates=[44100])[0]
    assert g.shape == (ar.out_len(pcm.shape[0], L, M),)
    first = (q_all - q_tail) * L                                  # first output of the tail's reference
    assert (first + 2 * L) * M > 2 ** 31
    tail = pcm[(q_all - q_tail) * M:]
    g64, y32 = references(tail, 44100)
    keep = slice(2 * L, None)                                     # 882 frames behind the cut: beyond the half width of 187
    got = g[first:].cpu().numpy()
    assert got.shape == g64.shape
    err, yard = rel_err(got[keep], g64[keep]), rel_err(y32[keep], g64[keep])
    print(f"positions past 2^31: kernel {err / U:.2f} u, yardstick {yard / U:.2f} u")
    assert err <= max(16 * U, 4 * yard)


def test_more_clips_than_one_launch_takes():
    """An entry point takes 65 535 clips per call (the clip is the grid's y index): load_clips splits a larger group, and
    ops says why when it is handed one."""
    n = ops.AUDIO_MAX_CLIPS + 2
    values = rng("many").integers(-32768, 32768, size=n).astype(np.int16)
    got = audio.load_clips([values[i:i + 1] for i in range(n)], DEV, normalize=False, rates=[16000] * n)
    assert len(got) == n and all(t.shape == (1,) for t in got[:3] + got[-3:])
    assert np.array_equal(torch.cat(got).cpu().numpy(), ar.downmix_ref(values, np.float32))
    desc = np.array([[i, 1, 1, i, 1] for i in range(n)], np.int64)
    pcm = torch.from_numpy(values).to(DEV)
    with pytest.raises(ValueError, match="65535"):
        ops.resample_audio(pcm, torch.from_numpy(desc).to(DEV), desc, None, 1, 1)
