"""Records tests/golden/g15_assemble.npz: the numeric core of the REFERENCE's record assembly run on synthetic tracks.

    python tests/golden/make_goldens_assemble.py

dataset_processing/Step5_resample_and_assemble.py cannot be imported (lmdb / cv2 / librosa); what it computes per track is the
one call `signal.resample(track, int(len(track) * goal_fps / fps))`, restated here with scipy itself (1.15.3 at recording; the
archive notes the version), as is Step 3's `signal.savgol_filter(code, 5, 2, axis=0)` in front of it.  Step 6's key split is a
literal restatement of its draw sequence on the global np.random (script lines 73-75 and 183-189, the toy-set block skipped).
The archive holds data only: inputs exactly representable in fp32, scipy's float64 outputs, scipy's outputs on float32 copies
(the reference's real arithmetic for the expression code; its error is quoted in DESIGN.md 5.21, nothing asserts it), the four
key lists and the resampled-length table.  tests/test_assemble_cpu.py pins tests/track_ref.py's restatement to these values."""
import os

import numpy as np
import scipy
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))

PAIRS = ((5, 5), (5, 6), (6, 5), (6, 7), (7, 6), (8, 4), (4, 8), (6, 6), (1, 4), (4, 1), (2, 3), (3, 2), (1, 1),
         (300, 300), (125, 150), (240, 120), (719, 899), (4096, 4095), (4095, 4096))
SMOOTH_PAIRS = ((5, 5), (5, 6), (6, 5), (10, 12), (125, 150), (240, 120), (719, 899))
LENGTHS = ((300, 29.97), (125, 25), (240, 60), (100, 30), (719, 23.976), (1, 60))


def track(rng, F, C):
    """(F, C) float32: a few low-frequency sinusoids plus white noise, so every kept bin carries energy."""
    t = np.arange(F, dtype=np.float64)[:, None]
    f = rng.uniform(0.2, 3.0, (3, C))
    ph = rng.uniform(0, 2 * np.pi, (3, C))
    x = sum(np.sin(2 * np.pi * f[i] * t / max(F, 8) + ph[i]) for i in range(3)) + 0.5 + 0.25 * rng.standard_normal((F, C))
    return x.astype(np.float32)


def step6_split(valid_keys, present):
    """Step 6's draw sequence for the full set, on the global generator."""
    all_valid_files = list(valid_keys)
    np.random.seed(42)
    np.random.shuffle(all_valid_files)
    # (toy-set block skipped)
    dict_to_save = {}
    for key in all_valid_files:
        if key in present:
            dict_to_save[key] = None
    train_split = 0.8
    val_split = 0.1
    np.random.seed(42)
    np.random.shuffle(all_valid_files)
    all_valid_files = list(dict_to_save.keys())
    np.random.shuffle(all_valid_files)
    train_keys = all_valid_files[:int(len(all_valid_files) * train_split)]
    val_keys = all_valid_files[int(len(all_valid_files) * train_split):int(len(all_valid_files) * (train_split + val_split))]
    test_keys = all_valid_files[int(len(all_valid_files) * (train_split + val_split)):]
    return all_valid_files, train_keys, val_keys, test_keys


def main():
    rng = np.random.default_rng(20260115)
    out = {"scipy_version": np.array(scipy.__version__), "pairs": np.array(PAIRS, np.int32),
           "smooth_pairs": np.array(SMOOTH_PAIRS, np.int32)}
    err32 = []
    for F, M in PAIRS:
        x = track(rng, F, 2 if max(F, M) > 1024 else 3)
        y = signal.resample(x.astype(np.float64), M)
        y32 = signal.resample(x, M)
        out[f"x_{F}_{M}"], out[f"y_{F}_{M}"], out[f"y32_{F}_{M}"] = x, y, y32
        err32.append(np.abs(y32.astype(np.float64) - y).max() / np.abs(y).max())
    for F, M in SMOOTH_PAIRS:
        x = track(rng, F, 3)
        y = signal.resample(signal.savgol_filter(x.astype(np.float64), 5, 2, axis=0), M)
        y32 = signal.resample(signal.savgol_filter(x, 5, 2, axis=0), M)
        out[f"sx_{F}_{M}"], out[f"sy_{F}_{M}"], out[f"sy32_{F}_{M}"] = x, y, y32
        err32.append(np.abs(y32.astype(np.float64) - y).max() / np.abs(y).max())
    out["err32"] = np.array(err32)
    keys = [f"clip_{i:03d}_{'abcdefg'[i % 7]}" for i in range(37)]
    missing = {keys[i] for i in (3, 11, 12, 25, 36)}
    lists = step6_split(keys, set(keys) - missing)
    out["split/valid_keys"], out["split/missing"] = np.array(keys), np.array(sorted(missing))
    for name, lst in zip(("all", "train", "valid", "test"), lists):
        out[f"split/{name}"] = np.array(lst)
    out["lengths/frames_fps"] = np.array(LENGTHS, np.float64)
    out["lengths/n_out"] = np.array([int(int(F) * 30 / fps) for F, fps in LENGTHS], np.int64)      # 0: raises
    path = os.path.join(HERE, "g15_assemble.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, scipy {scipy.__version__}, float32 error up to {max(err32):.2e}")


if __name__ == "__main__":
    main()
