"""The bits the data-prep kernels return, as a recorded table.

csrc/headpose.hip, csrc/track_resample.hip and csrc/audio_io.hip share their device pieces: the Savitzky-Golay staging and
row rule of csrc/savgol.h (headpose_smooth_kernel, track_analysis_kernel) and the double-precision wave sum of csrc/common.h
(headpose_fit_kernel, the audio front end's block sum).  Their own tests compare with float64 references inside tolerances; a
slip in a shared piece that stays inside them would go unseen.  This test holds each call to the SHA-256 of its outputs
instead, on seeded inputs generated on the host.

tests/golden/dataprep_bits.json was recorded from the library of the commit BEFORE those pieces were shared: that commit's
libmsmd_hip.so, built beside this checkout and loaded through MSMD_LIB (the C ABI is the same), ran this module's own recorder

    MSMD_LIB=<the parent's csrc/libmsmd_hip.so> python tests/test_dataprep_bits_gpu.py --record FILE

twice, with identical files.  It is not an output of the code under test.

Rows, the smallest shapes at which a shared piece can go wrong.
  headpose_smooth  window 5 at F = 5 (every frame an edge row), 6, 255 / 256 / 257 (around the 256-frame scan chunk) and 600 (two
                   chunks and a remainder); window 33 at F = 33 and 600; each alone, and the six window-5 lengths as one ragged
                   call; both outputs.
  headpose_fit     7 frames, one of them blended from its neighbours; (P, S) = (20, 3) and (1025, 64): two landmark tiles, a
                   full wave of static points.
  track_resample   (F, M) = (31, 31), (32, 40), (64, 17), (65, 130), (130, 65) at C = 1 and 17 without a filter: the bin count on
                   a 16-bin tile and one past it, the frames on the 64-frame stage and one past it, up and down; (33, 33) and
                   (65, 130) at C = 17 through windows 5 and 33; the five unfiltered pairs as one ragged call.
  audio            a 44.1 kHz two-channel int16 group and a 16 kHz mono fp32 group (the bypass) of clips with 255, 256, 257 and
                   4097 output samples (around the 256-output resample run and the 4096-output z-norm run): `out` and the
                   written rows of `partials` after resample_audio, `out` after znorm_audio.
(msmd_conv0_gn_gelu has no row: csrc/audio.hip is as it was.)"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmd_amd import _lib, ops  # noqa: E402
from msmd_amd.utils import audio as A  # noqa: E402
from msmd_amd.utils.head_pose import gap_plan, savgol_table  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataprep_bits.json")
DEV = "cuda:0"
SMOOTH_5, SMOOTH_33 = (5, 6, 255, 256, 257, 600), (33, 600)
TRACK_PAIRS = ((31, 31), (32, 40), (64, 17), (65, 130), (130, 65))
AUDIO_OUT = (255, 256, 257, 4097)
POLYORDER = {5: 2, 33: 3}


def rng(tag):
    return np.random.default_rng(int.from_bytes(hashlib.sha256(tag.encode()).digest()[:8], "little"))


def dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)


def digest(*outs):
    h = hashlib.sha256()
    for t in outs:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def table_of(window):
    return dev(savgol_table(window, POLYORDER[window]))


# ----------------------------------------------------------------------------- the calls
def rotations(tag, F):
    """(F, 3, 3) fp32 rotation matrices of a smooth quaternion path that wanders over the whole sphere, so the raw quaternions
    change branch and sign along the clip."""
    g = rng(tag)
    t = np.arange(F, dtype=np.float64)[:, None]
    q = (g.standard_normal((1, 4)) + np.sin(t * g.uniform(0.01, 0.08, (1, 4)) + g.uniform(0, 6.28, (1, 4))) * 1.5
         + 0.02 * g.standard_normal((F, 4)))
    x, y, z, w = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)
    return R.reshape(F, 3, 3).astype(np.float32)


def smooth(window, lengths):
    R = np.concatenate([rotations(f"smooth/{window}/{F}", F) for F in lengths])
    offsets = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    return digest(*ops.headpose_smooth(dev(R), offsets, table_of(window), window, want_matrix=True))


def fit(P, S):
    g = rng(f"fit/{P}/{S}")
    n = 7
    neutral = (0.5 + 0.05 * g.standard_normal((P, 3))).astype(np.float32)
    L = (0.5 + 0.05 * g.standard_normal((n, P, 3))).astype(np.float32)
    a, b, w = gap_plan(np.array([1, 1, 0, 1, 1, 1, 1], bool))
    assert w[2] != 0.0
    sidx = np.sort(g.choice(P, S, replace=False)).astype(np.int32)
    return digest(*ops.headpose_fit(dev(L), dev(a), dev(b), dev(w.astype(np.float32)), dev(neutral), dev(sidx)))


def track(pairs, C, window):
    x = np.concatenate([rng(f"track/{F}/{M}/{C}").standard_normal((F, C)) for F, M in pairs]).astype(np.float32)
    off_in = np.concatenate([[0], np.cumsum([p[0] for p in pairs])]).tolist()
    off_out = np.concatenate([[0], np.cumsum([p[1] for p in pairs])]).tolist()
    return digest(ops.track_resample(dev(x), off_in, off_out, table_of(window) if window else None, window))


def audio(rate, channels, int16):
    fb = A.filter_bank(rate)
    desc, pcm, in_off, out_off = np.zeros((len(AUDIO_OUT), 5), np.int64), [], 0, 0
    for row, n_out in enumerate(AUDIO_OUT):
        frames = n_out * fb.M // fb.L
        assert A.output_length(frames, fb.L, fb.M) == n_out
        s = 0.3 * rng(f"audio/{rate}/{n_out}").standard_normal(frames * channels)
        pcm.append(np.clip(np.rint(s * 32768), -32768, 32767).astype(np.int16) if int16 else s.astype(np.float32))
        desc[row] = (in_off, frames, channels, out_off, n_out)
        in_off, out_off = in_off + frames * channels, out_off + n_out
    desc_dev = dev(desc)
    bank = None if fb.table is None else dev(fb.table)
    out, partials = ops.resample_audio(dev(np.concatenate(pcm)), desc_dev, desc, bank, fb.L, fb.M)
    written = [partials[row, :(n + ops.AUDIO_RUN - 1) // ops.AUDIO_RUN] for row, n in enumerate(AUDIO_OUT)]
    resampled = digest(out, *written)
    return resampled + digest(ops.znorm_audio(out, desc_dev, desc, partials))


def table():
    rows = {}
    for window, lengths in ((5, SMOOTH_5), (33, SMOOTH_33)):
        for F in lengths:
            rows[f"headpose_smooth window {window} F {F}"] = (smooth, window, (F,))
    rows["headpose_smooth window 5 ragged"] = (smooth, 5, SMOOTH_5)
    for P, S in ((20, 3), (1025, 64)):
        rows[f"headpose_fit P {P} S {S}"] = (fit, P, S)
    for C in (1, 17):
        for pair in TRACK_PAIRS:
            rows[f"track_resample {pair} C {C}"] = (track, (pair,), C, 0)
        rows[f"track_resample ragged C {C}"] = (track, TRACK_PAIRS, C, 0)
    for window in (5, 33):
        for pair in ((33, 33), (65, 130)):
            rows[f"track_resample {pair} C 17 window {window}"] = (track, (pair,), 17, window)
    rows["audio 44100 Hz 2 channels int16"] = (audio, 44100, 2, True)
    rows["audio 16000 Hz mono fp32"] = (audio, 16000, 1, False)
    return rows


TABLE = table()


def run_row(name):
    f, *args = TABLE[name]
    return f(*args)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_the_table(recorded):
    assert sorted(recorded) == sorted(TABLE) and len(TABLE) == 29


@pytest.mark.parametrize("name", list(TABLE))
def test_dataprep_bits_are_the_recorded_ones(name, recorded):
    assert run_row(name) == recorded[name], f"{name}: the output bits differ from the parent commit's"


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_dataprep_bits_gpu.py --record FILE")
    print(f"recording the bits of {_lib.LIB_PATH}", file=sys.stderr)
    with open(sys.argv[2], "w") as out:
        json.dump({name: run_row(name) for name in TABLE}, out, indent=0, sort_keys=True)
        out.write("\n")
