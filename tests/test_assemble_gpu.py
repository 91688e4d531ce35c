"""Track resampling and record assembly on the MI355X: csrc/track_resample.hip through msmd_amd.utils.assemble against the float64
restatement (tests/track_ref.py, itself pinned to scipy's recorded outputs by tests/test_assemble_cpu.py).

Bound, for every output element:  |y - y64| <= 2^-23 sum_n |W[m, n]| |x[n, c]|, W the operator matrix of the restatement (the
filter composed in when there is one).  Derived, not measured: the kernel sums in double, so its only fp32 rounding is the
store, 2^-24 |y| <= 2^-24 sum |W| |x|; the factor 2 covers the double twiddles and sums (about 1e-13 of the same sum).  A kernel
that accumulated in fp32 would miss it.  The worst ratio of every case is printed before it is asserted."""
import json
import os
import pickle as pkl
import subprocess
import sys

import numpy as np
import pytest
import torch

import track_ref as TR
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 16        # MSMD_TRACK_ROWS: bins per workgroup of the analysis (K + 1 bins, K = min(F, M) // 2), output frames per workgroup of the synthesis
CH_TILE = 16     # MSMD_TRACK_CH_TILE: channels per workgroup
STAGE = 64       # MSMD_TRACK_STAGE: frames (analysis) / bins (synthesis) staged in LDS per pass

PARITY = [(5, 5), (5, 6), (6, 5), (6, 7), (7, 6), (8, 4), (4, 8), (6, 6), (1, 4), (4, 1), (2, 3), (3, 2), (1, 1),
          (300, 300), (125, 150), (240, 120), (719, 899)]
# K + 1 = ROWS - 1, ROWS, ROWS + 1 bins, by F and by M (K = 14, 15, 16: N = 29, 30 / 31, 32 / 33)
BIN_TILE = [(n, 40) for n in (2 * ROWS - 3, 2 * ROWS - 2, 2 * ROWS - 1, 2 * ROWS, 2 * ROWS + 1)] + \
           [(40, n) for n in (2 * ROWS - 3, 2 * ROWS - 2, 2 * ROWS - 1, 2 * ROWS, 2 * ROWS + 1)]
# M = ROWS - 1, ROWS, ROWS + 1 output frames (and the same F)
FRAME_TILE = [(40, ROWS - 1), (40, ROWS), (40, ROWS + 1), (ROWS - 1, 40), (ROWS, 40), (ROWS + 1, 40), (2 * ROWS + 1, 3 * ROWS + 1)]
# F = STAGE - 1, STAGE, STAGE + 1 frames per pass of the analysis (and 2 STAGE), the same M
FRAME_STAGE = [(STAGE - 1, 50), (STAGE, 50), (STAGE + 1, 50), (2 * STAGE - 1, 50), (2 * STAGE, 50), (2 * STAGE + 1, 50),
               (50, STAGE - 1), (50, STAGE), (50, STAGE + 1)]
# K + 1 = STAGE - 1, STAGE, STAGE + 1 bins per pass of the synthesis, by F and by M (K = 62, 63, 64)
BIN_STAGE = [(n, 200) for n in (2 * STAGE - 4, 2 * STAGE - 3, 2 * STAGE - 2, 2 * STAGE - 1, 2 * STAGE, 2 * STAGE + 1)] + \
            [(200, n) for n in (2 * STAGE - 4, 2 * STAGE - 3, 2 * STAGE - 2, 2 * STAGE - 1, 2 * STAGE, 2 * STAGE + 1)]
CAP = [(4096, 4095), (4095, 4096)]


def track(seed, F, C):
    """(F, C) fp32: three low-frequency sinusoids, an offset and white noise, so every kept bin carries energy."""
    rng = np.random.default_rng(seed)
    t = np.arange(F, dtype=np.float64)[:, None]
    f, ph = rng.uniform(0.2, 3.0, (3, C)), rng.uniform(0, 2 * np.pi, (3, C))
    x = sum(np.sin(2 * np.pi * f[i] * t / max(F, 8) + ph[i]) for i in range(3)) + 0.5 + 0.25 * rng.standard_normal((F, C))
    return x.astype(np.float32)


def run(x, M, smooth=None):
    from msmd_amd.utils.assemble import resample_track
    y = resample_track(torch.from_numpy(x).to(DEV), M, smooth)
    assert y.shape == (M, x.shape[1]) and y.dtype == torch.float32
    return y.cpu().numpy()


def check(tag, x, M, y, smooth=None):
    y64, W = TR.resample(x, M, smooth)
    bound = TR.error_bound(W, x)
    err = np.abs(y.astype(np.float64) - y64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{tag}: worst |y - y64| / bound = {ratio:.3f} (max error {err.max():.2e})")
    assert np.isfinite(y).all() and (err <= bound).all(), (tag, ratio)
    return W


@pytest.mark.parametrize("F,M", PARITY + BIN_TILE + FRAME_TILE + FRAME_STAGE + BIN_STAGE)
def test_resample_within_the_bound(F, M):
    x = track(1000 * F + M, F, 3)
    check(f"({F}, {M})", x, M, run(x, M))


@pytest.mark.parametrize("F,M", CAP)
def test_resample_at_the_cap(F, M):
    x = track(F, F, 2)
    check(f"({F}, {M})", x, M, run(x, M))


@pytest.mark.parametrize("C", [1, 3, 50, 53, CH_TILE - 1, CH_TILE, CH_TILE + 1])
def test_channel_counts(C):
    for F, M in ((125, 150), (33, 31)):
        x = track(C, F, C)
        check(f"C = {C} ({F}, {M})", x, M, run(x, M))


@pytest.mark.parametrize("w,p", [(5, 2), (7, 3), (33, 4)])
def test_filter_fused_into_the_analysis(w, p):
    for F in (w, w + 1, 2 * w):
        for M in (F + 3, F, max(F - 2, 1)):
            x = track(100 * w + F, F, 5)
            check(f"savgol({w}, {p}) ({F}, {M})", x, M, run(x, M, (w, p)), smooth=(w, p))
    x = track(w, 300, 53)
    check(f"savgol({w}, {p}) (300, 360) C = 53", x, 360, run(x, 360, (w, p)), smooth=(w, p))


@pytest.mark.parametrize("smooth", [None, (5, 2)])
def test_ragged_batch_bits_do_not_depend_on_the_batch(smooth):
    """7 clips in one call: a 1-frame clip (5 frames under the filter), M == F, clips on both sides of the frame stage and of the
    bin tile, a long one.  Each clip's bits equal the bits it gets alone, and a second run repeats them."""
    from msmd_amd.utils.assemble import resample_track
    shapes = [(1, 4) if smooth is None else (5, 7), (300, 300), (STAGE - 1, 50), (STAGE + 1, 50), (2 * ROWS - 2, 40), (2 * ROWS + 1, 40),
              (719, 899)]
    C = CH_TILE + 1
    xs = [track(7 + i, F, C) for i, (F, _) in enumerate(shapes)]
    dev = [torch.from_numpy(x).to(DEV) for x in xs]
    Ms = [M for _, M in shapes]
    together = [y.cpu().numpy() for y in resample_track(dev, Ms, smooth)]
    again = [y.cpu().numpy() for y in resample_track(dev, Ms, smooth)]
    reverse = [y.cpu().numpy() for y in resample_track(dev[::-1], Ms[::-1], smooth)][::-1]
    for i, (x, M) in enumerate(zip(xs, Ms)):
        alone = run(x, M, smooth)
        check(f"clip {i} {shapes[i]}", x, M, together[i], smooth)
        assert np.array_equal(alone.view(np.uint32), together[i].view(np.uint32)), shapes[i]
        assert np.array_equal(again[i].view(np.uint32), together[i].view(np.uint32)), shapes[i]
        assert np.array_equal(reverse[i].view(np.uint32), together[i].view(np.uint32)), shapes[i]


def test_constant_track_stays_constant():
    for F, M in ((10, 13), (13, 10), (64, 64), (1, 7), (300, 360)):
        c = np.float32(0.7)
        x = np.full((F, 2), c, np.float32)
        y = run(x, M)
        W = check(f"constant ({F}, {M})", x, M, y)
        assert (np.abs(y.astype(np.float64) - float(c)) <= 2.0 ** -23 * np.abs(W).sum(1, keepdims=True) * float(c)).all()


def test_sinusoid_below_both_nyquist_limits_lands_on_its_samples():
    """x[n] = sin(2 pi f n / F + phi) with f whole cycles, f < min(F, M) / 2: y[m] = sin(2 pi f m / M + phi).  The bound's two
    halves are spent on the rounding of x to fp32 and on the store."""
    for F, M, f in ((50, 60, 3), (60, 50, 7), (125, 150, 20), (240, 120, 31), (33, 64, 16)):
        phi = np.array([0.3, 1.1])
        x64 = np.sin(2 * np.pi * f * np.arange(F)[:, None] / F + phi)
        x = x64.astype(np.float32)
        y = run(x, M)
        W = check(f"sinusoid ({F}, {M}, f = {f})", x, M, y)
        want = np.sin(2 * np.pi * f * np.arange(M)[:, None] / M + phi)
        err, bound = np.abs(y - want), TR.error_bound(W, x)
        print(f"  against the analytic samples: worst ratio {float((err / bound).max()):.3f}")
        assert (err <= bound).all()


def test_argument_errors_name_the_offending_value():
    from msmd_amd import ops
    from msmd_amd.utils.assemble import resample_track
    from msmd_amd.utils.head_pose import savgol_table
    x = torch.zeros(12, 3, device=DEV)
    tab = torch.from_numpy(savgol_table(5, 2)).to(DEV)
    with pytest.raises(TypeError, match="x must be"):
        ops.track_resample(x.double(), [0, 12], [0, 10])
    with pytest.raises(TypeError, match="x must be"):
        ops.track_resample(x.t(), [0, 3], [0, 10])
    with pytest.raises(TypeError, match="shape"):
        ops.track_resample(x.reshape(-1), [0, 36], [0, 10])
    with pytest.raises(ValueError, match="run from 0 to 12"):
        ops.track_resample(x, [0, 5, 11], [0, 6, 12])
    with pytest.raises(ValueError, match="got 0"):
        ops.track_resample(x, [0, 5, 5, 12], [0, 6, 8, 12])
    with pytest.raises(ValueError, match="got -2"):
        ops.track_resample(x, [0, 7, 5, 12], [0, 6, 8, 12])
    with pytest.raises(ValueError, match="got 4097"):
        ops.track_resample(x, [0, 12], [0, 4097])
    with pytest.raises(ValueError, match="1 input clips but 2 output clips"):
        ops.track_resample(x, [0, 12], [0, 5, 10])
    with pytest.raises(ValueError, match="got 4"):
        ops.track_resample(x, [0, 12], [0, 10], tab, 4)
    with pytest.raises(TypeError, match="savgol_table"):
        ops.track_resample(x, [0, 12], [0, 10], tab.float(), 5)
    with pytest.raises(ValueError, match="shorter than the window of 5"):
        ops.track_resample(x, [0, 4, 12], [0, 4, 12], tab, 5)
    with pytest.raises(ValueError, match="window = 0"):
        ops.track_resample(x, [0, 12], [0, 10], tab, 0)
    with pytest.raises(TypeError, match=r"\(F, 3\)"):
        resample_track([x, torch.zeros(5, 4, device=DEV)], [3, 3])
    with pytest.raises(ValueError):
        resample_track(x, 10, smooth=(4, 2))
    assert ops.track_resample(x, [0, 5, 12], [0, 6, 12]).shape == (12, 3)     # and the same arguments, well-formed, run


def synthetic_clip(seed, F, fps):
    rng = np.random.default_rng(seed)
    exp, head = track(seed, F, 50), 10 * track(seed + 1, F, 3)
    audio = (0.1 * rng.standard_normal(int(F / fps * 16000))).astype(np.float32)
    return exp, head, audio


def test_end_to_end_records_feed_the_dataset(tmp_path):
    from msmd_amd.datasets import DatasetPickle
    from msmd_amd.inference import resample_linear
    from msmd_amd.utils.assemble import assemble_clip, resampled_length, save_dict_in_chunks
    fps = [25, 29.97, 60]
    clips = [synthetic_clip(40 + i, F, r) for i, (F, r) in enumerate(zip((150, 241, 500), fps))]
    records = assemble_clip([c[0] for c in clips], [torch.from_numpy(c[1]).to(DEV) for c in clips],
                            [torch.from_numpy(c[2]) for c in clips], fps, smooth_expression=(5, 2))
    data = {f"clip{i}": r for i, r in enumerate(records)}
    for (e, h, a), r, rate in zip(clips, records, fps):
        M = resampled_length(e.shape[0], rate)
        assert r["expression_code"].shape == (M, 50) and r["head_orientation"].shape == (M, 3) and r["audio"].shape == a.shape
        assert all(v.dtype == np.float32 for v in r.values()) and np.array_equal(r["audio"], a)
        check("expression", e, M, r["expression_code"], (5, 2))
        check("head", h, M, r["head_orientation"])
    one = assemble_clip(clips[1][0], clips[1][1], clips[1][2], fps[1], smooth_expression=(5, 2))
    assert all(np.array_equal(one[k], records[1][k]) for k in one)
    save_dict_in_chunks(data, tmp_path / "data.pkl", chunk_size=2)
    (tmp_path / "keys.txt").write_text("\n".join(data))
    ds = DatasetPickle(str(tmp_path / "data.pkl"), str(tmp_path / "keys.txt"), full_dataset=True, celebv_text=False, device=DEV, seed=0)
    assert len(ds) == 3
    want = []
    for r in records:
        n_new = int(round(r["expression_code"].shape[0] / 30 * 25))
        want.append(np.concatenate([resample_linear(r["expression_code"], n_new), resample_linear(r["head_orientation"], n_new)],
                                   -1).astype(np.float32))
    assert np.array_equal(ds.coef_flat.cpu().numpy(), np.concatenate(want, 0))
    audio, coef, _ = ds.batch([0, 2])
    assert audio[0].shape == (2, 64000) and coef[0]["motion"].shape == (2, 100, 53) and torch.isfinite(coef[1]["motion"]).all()


def test_command_line_writes_the_pickle_and_the_key_files(tmp_path):
    from msmd_amd.datasets import load_dict_in_chunks
    from msmd_amd.utils.assemble import KEY_FILES, resampled_length
    from msmd_amd.utils.audio import write_wav
    from msmd_amd.utils.head_pose import save_head_rot
    manifest = []
    for i, (F, fps) in enumerate(((100, 25), (120, 60))):
        e, h, a = synthetic_clip(60 + i, F, fps)
        write_wav(tmp_path / f"c{i}.wav", a)
        save_head_rot(tmp_path / f"c{i}_rot.pkl", h)
        if i == 0:
            np.save(tmp_path / "c0_exp.npy", e)
        else:
            with open(tmp_path / "c1_exp.pkl", "wb") as f:
                pkl.dump(torch.from_numpy(e), f)
        manifest.append(dict(key=f"c{i}", expression_code=str(tmp_path / ("c0_exp.npy" if i == 0 else "c1_exp.pkl")),
                             head_orientation=str(tmp_path / f"c{i}_rot.pkl"), wav=str(tmp_path / f"c{i}.wav"), fps=fps))
    manifest.append(dict(key="broken", expression_code=str(tmp_path / "none.npy"), head_orientation=str(tmp_path / "none.pkl"),
                         wav=str(tmp_path / "none.wav"), fps=30))
    (tmp_path / "clips.json").write_text(json.dumps(manifest))
    r = subprocess.run([sys.executable, "-m", "msmd_amd.utils.assemble", "--manifest", str(tmp_path / "clips.json"), "--out",
                        str(tmp_path / "data.pkl"), "--split_dir", str(tmp_path / "split"), "--chunk_size", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    data = {}
    for chunk in load_dict_in_chunks(tmp_path / "data.pkl"):
        data.update(chunk)
    assert sorted(data) == ["c0", "c1"]
    for i, (F, fps) in enumerate(((100, 25), (120, 60))):
        M = resampled_length(F, fps)
        assert data[f"c{i}"]["expression_code"].shape == (M, 50) and data[f"c{i}"]["head_orientation"].shape == (M, 3)
        assert data[f"c{i}"]["audio"].ndim == 1 and data[f"c{i}"]["audio"].dtype == np.float32
    with open(tmp_path / "data_error_files.pkl", "rb") as f:
        assert pkl.load(f) == ["broken"]
    lists = [(tmp_path / "split" / n).read_text().split() for n in KEY_FILES]     # 2 keys cut at int(1.6), int(1.8): valid is empty
    assert sorted(lists[0]) == ["c0", "c1"] and sorted(lists[1] + lists[2] + lists[3]) == ["c0", "c1"] and lists[2] == []
