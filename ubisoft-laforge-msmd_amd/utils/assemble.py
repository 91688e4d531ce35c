"""Training records from tracked clips: the numeric stage of the reference's dataset_processing/Step5_resample_and_assemble.py
(every motion track Fourier-resampled to the goal frame rate, scipy.signal.resample) with Step3_preprocess_expression_code.py's
Savitzky-Golay smoothing of the expression code folded in, on the device (csrc/track_resample.hip through
`ops.track_resample`), and the host side of Step6_train_test_validation_split_and_save_pkl.py: the chunked
pickle `datasets.DatasetPickle(full_dataset=True)` reads and the four key lists.

Two deviations from the reference: the head track is stored as float32 (the reader casts it anyway), and the audio is not
Fourier-resampled but comes from `utils.audio.load_clips` (polyphase filter, 16 kHz mono, un-normalised).  Video decoding,
`.m4a` decoding and lmdb stay outside: the caller arrives with the tracks, a WAV and the clip's frame rate.

    python -m msmd_amd.utils.assemble --manifest clips.json --out data.pkl [--goal_fps 30] [--smooth_expression 5 2]
                                      [--split_dir DIR] [--chunk_size 1000]
"""
from __future__ import annotations

import argparse
import json
import os
import pickle as pkl

import numpy as np
import torch

from .. import ops
from .common import clip_list, cut_clips, flatten_clips
from .head_pose import savgol_table

KEY_FILES = ("keys.txt", "keys_train.txt", "keys_valid.txt", "keys_test.txt")


def resampled_length(n_frames, fps, goal_fps=30):
    """int(n_frames * goal_fps / fps) in Python floats, truncated as Step 5 does; ValueError when nothing is left."""
    n = int(int(n_frames) * goal_fps / fps)
    if n < 1:
        raise ValueError(f"{n_frames} frames at {fps} fps leave no frame at {goal_fps} fps")
    return n


def resample_track(x, n_out, smooth=None):
    """scipy.signal.resample(x, n_out) along the frames, on the device.  x: one (F, C) fp32 device tensor, or a list of them
    (one C, any F in 1 .. ops.TRACK_MAX_FRAMES) resampled in ONE call; n_out: an int, or a list of ints.  smooth =
    (window, polyorder): the track is read through scipy's savgol_filter(x, window, polyorder, axis=0) first.
    -> a tensor (n_out, C), or a list of them for a list."""
    clips, single = clip_list(x)
    n_outs = [n_out] * len(clips) if isinstance(n_out, (int, np.integer)) else [int(n) for n in n_out]
    if len(n_outs) != len(clips):
        raise ValueError(f"{len(clips)} clips but {len(n_outs)} output lengths")
    ops._need_cuda(*clips)
    flat, in_off, _ = flatten_clips(clips, (None,))
    out_off = [0] + np.cumsum(n_outs).tolist()
    window = 0 if smooth is None else int(smooth[0])
    table = None if smooth is None else torch.from_numpy(savgol_table(window, smooth[1])).to(flat.device)
    return cut_clips(ops.track_resample(flat, in_off, out_off, table, window), out_off, single)


def _track(a, width, name, device):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    if t.dim() != 2 or (width is not None and t.shape[1] != width) or t.shape[0] == 0:
        raise TypeError(f"{name} must have shape (F, {width if width is not None else 'E'}), got {tuple(t.shape)}")
    return t.detach().to(device=device, dtype=torch.float32)


def _audio(a, device):
    """A WAV path or (samples, rate) goes through utils.audio.load_clips; a 1-D tensor / array is 16 kHz mono as it is."""
    from .audio import load_clips
    if isinstance(a, (str, os.PathLike)):
        return load_clips([a], device=device, normalize=False)[0].cpu().numpy()
    if isinstance(a, tuple):
        return load_clips([a[0]], device=device, normalize=False, rates=[a[1]])[0].cpu().numpy()
    s = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float32)
    if s.ndim != 1 or s.size == 0:
        raise TypeError(f"audio samples must be 1-D and not empty, got shape {s.shape}")
    return s


def assemble_clip(expression_code, head_orientation, audio, fps, goal_fps=30, smooth_expression=None, device="cuda"):
    """One clip's record {"head_orientation": (M, 3), "expression_code": (M, E), "audio": (S,)} as float32 numpy arrays, what
    `datasets.ResidentDataset` takes, M = resampled_length(F, fps, goal_fps) per track.  expression_code (F, E) and
    head_orientation (F', 3): tensors or arrays; audio: a WAV path, (samples, rate), or 16 kHz mono samples; fps: the clip's.
    Lists in every argument (fps too) give a list of records, with ONE `resample_track` call per track kind.
    smooth_expression = (5, 2) is Step 3's smoothing for callers whose code is unsmoothed; Step 5 reads smoothed code."""
    single = not isinstance(expression_code, (list, tuple))
    if single:
        expression_code, head_orientation, audio, fps = [expression_code], [head_orientation], [audio], [fps]
    n = len(expression_code)
    if not (len(head_orientation) == len(audio) == len(fps) == n) or n == 0:
        raise ValueError(f"{n} expression codes, {len(head_orientation)} head tracks, {len(audio)} audio clips, {len(fps)} frame rates")
    if torch.device(device).type != "cuda":
        raise RuntimeError("assemble_clip needs the MI355X (cuda) device; there is no CPU path")
    exp = [_track(e, None, "expression_code", device) for e in expression_code]
    head = [_track(h, 3, "head_orientation", device) for h in head_orientation]
    exp_r = resample_track(exp, [resampled_length(e.shape[0], f, goal_fps) for e, f in zip(exp, fps)], smooth_expression)
    head_r = resample_track(head, [resampled_length(h.shape[0], f, goal_fps) for h, f in zip(head, fps)])
    records = [{"head_orientation": h.cpu().numpy(), "expression_code": e.cpu().numpy(), "audio": _audio(a, device)}
               for e, h, a in zip(exp_r, head_r, audio)]
    return records[0] if single else records


def save_dict_in_chunks(data, path, chunk_size=1000):
    """The reference's chunked pickle: dicts of `chunk_size` entries back to back, in the dictionary's order."""
    chunk_size = int(chunk_size)
    if chunk_size < 1:
        raise ValueError(f"chunk_size must be at least 1, got {chunk_size}")
    keys = list(data.keys())
    with open(path, "wb") as f:
        for i in range(0, len(keys), chunk_size):
            pkl.dump({k: data[k] for k in keys[i:i + chunk_size]}, f)


def split_keys(valid_keys, present):
    """-> (all, train, valid, test) key lists with Step 6's draw sequence for the full set: the valid keys shuffled under seed
    42 (and once more under seed 42 behind the toy-set block), the present ones taken in the order of the first shuffle,
    shuffled on the continuing stream, cut at 0.8 / 0.9."""
    keys = list(valid_keys)
    present = set(present)
    rs = np.random.RandomState(42)
    rs.shuffle(keys)
    kept = [k for k in keys if k in present]
    rs = np.random.RandomState(42)
    rs.shuffle(keys)
    rs.shuffle(kept)
    a, b = int(len(kept) * 0.8), int(len(kept) * (0.8 + 0.1))
    return kept, kept[:a], kept[a:b], kept[b:]


def write_key_files(directory, all_keys, train, valid, test):
    """The four '\\n'-joined key files (KEY_FILES) of a split, as Step 6 writes them."""
    os.makedirs(directory, exist_ok=True)
    for name, keys in zip(KEY_FILES, (all_keys, train, valid, test)):
        with open(os.path.join(directory, name), "w") as f:
            f.write("\n".join(keys))


def _load_expression(path):
    if str(path).endswith(".npy"):
        return np.load(path)
    with open(path, "rb") as f:
        a = pkl.load(f)
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="chunked training pickle and key lists from tracked clips")
    p.add_argument("--manifest", required=True, help="JSON list of {key, expression_code, head_orientation, wav, fps}")
    p.add_argument("--out", required=True, help="the chunked pickle to write")
    p.add_argument("--goal_fps", type=int, default=30)
    p.add_argument("--smooth_expression", type=int, nargs=2, default=None, metavar=("WINDOW", "POLYORDER"))
    p.add_argument("--split_dir", default=None, help="write the four key files here")
    p.add_argument("--chunk_size", type=int, default=1000)
    p.add_argument("--device", default="cuda")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    with open(args.manifest) as f:
        manifest = json.load(f)
    loaded, errors = [], []
    for item in manifest:
        try:                       # a clip that cannot be read is skipped, as Step 5 skips it
            with open(item["head_orientation"], "rb") as f:
                head = np.asarray(pkl.load(f), dtype=np.float32)
            loaded.append((item["key"], _load_expression(item["expression_code"]), head, item["wav"], float(item["fps"])))
        except Exception as e:
            print(f"skipped {item.get('key')}: {e}")
            errors.append(item.get("key"))
    data = {}
    smooth = tuple(args.smooth_expression) if args.smooth_expression else None
    try:
        records = assemble_clip([c[1] for c in loaded], [c[2] for c in loaded], [c[3] for c in loaded], [c[4] for c in loaded],
                                args.goal_fps, smooth, args.device) if loaded else []
        data = {c[0]: r for c, r in zip(loaded, records)}
    except (ValueError, TypeError, OSError):
        for c in loaded:           # one clip of the list is at fault: find it by going one at a time
            try:
                data[c[0]] = assemble_clip(c[1], c[2], c[3], c[4], args.goal_fps, smooth, args.device)
            except (ValueError, TypeError, OSError) as e:
                print(f"skipped {c[0]}: {e}")
                errors.append(c[0])
    save_dict_in_chunks(data, args.out, args.chunk_size)
    with open(os.path.splitext(args.out)[0] + "_error_files.pkl", "wb") as f:
        pkl.dump(errors, f)
    if args.split_dir:
        write_key_files(args.split_dir, *split_keys([item["key"] for item in manifest], data.keys()))
    print(f"wrote {args.out}: {len(data)} clips, {len(errors)} skipped")


if __name__ == "__main__":
    main()
