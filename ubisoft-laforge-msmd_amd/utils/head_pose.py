"""Head rotation of a clip from tracked face landmarks: the numeric stage of the reference's
dataset_processing/Step2_preprocess_head_pose_mediapipe.py (gap filling, per-frame Procrustes fit onto a canonical face,
quaternion smoothing, yaw / pitch / roll) on the device, csrc/headpose.hip through `ops.headpose_fit` / `ops.headpose_smooth`
(DESIGN.md 5.18).  Its output is the head-rotation pickle `inference.query_for_motion_coeff` reads for a style clip.

Face detection, the landmark tracker, video decoding and the arrow overlay stay outside: the caller arrives with landmarks
(F, P, 3), a bool array saying which frames were tracked, and their own copies of the canonical face (.obj) and of the index
mapping (.json) -- the product ships neither.

    python -m msmd_amd.utils.head_pose --landmarks L.npy [--valid V.npy] --neutral face.obj --mapping map.json --out clip.pkl
"""
from __future__ import annotations

import argparse
import json
import pickle as pkl

import numpy as np
import torch

from .. import ops
from .common import clip_list, cut_clips, flatten_clips


def gap_plan(valid):
    """valid (F) bool -> (src_a (F) int32, src_b (F) int32, w (F) float64): frame f of the filled clip is
    (1 - w[f]) L[src_a[f]] + w[f] L[src_b[f]].  A tracked frame names itself with weight 0.  Frames before the first
    tracked frame copy it, frames after the last copy it.  Missing frame number i (from 0) of a gap of g frames between the
    tracked frames a < b gets tau = (i + 1) / (g + 2) -- the denominator is the REFERENCE's (interpolate_landmarks), kept as
    it is: g + 1 would space the frames evenly, g + 2 leaves the last filled frame short of b.
    ValueError when no frame is tracked, or when the missing frames number F // 2 or more (the reference skips such a video)."""
    valid = np.asarray(valid)
    if valid.ndim != 1 or valid.dtype != np.bool_:
        raise TypeError("valid must be a 1-D bool array")
    F = valid.shape[0]
    idx = np.flatnonzero(valid)
    if idx.size == 0:
        raise ValueError("no frame of the clip is valid")
    if F - idx.size >= F // 2:
        raise ValueError(f"{F - idx.size} of {F} frames are missing: half or more (the reference skips such a video)")
    a = np.arange(F, dtype=np.int32)
    b = a.copy()
    w = np.zeros(F, np.float64)
    a[:idx[0]] = b[:idx[0]] = idx[0]
    a[idx[-1] + 1:] = b[idx[-1] + 1:] = idx[-1]
    for lo, hi in zip(idx[:-1], idx[1:]):
        g = hi - lo - 1
        for i in range(g):
            a[lo + 1 + i], b[lo + 1 + i], w[lo + 1 + i] = lo, hi, (i + 1) / (g + 2)
    return a, b, w


def savgol_table(window, polyorder):
    """-> float64 (window + 2 (window // 2) window,) = window^2 numbers: the `window` symmetric interior coefficients of the
    Savitzky-Golay filter, then the edge table (2 (window // 2), window) whose row r < window // 2 gives frame r from the
    first `window` samples and whose row window // 2 + r gives frame F - window // 2 + r from the last `window`: the
    polynomial of order `polyorder` fitted to those samples, evaluated at that frame (scipy's mode='interp').
    From the definition: A the Vandermonde matrix of the window's positions (centred, scaled to [-1, 1]), A = Q R, and
    H = Q Q^T takes the samples to their least-squares polynomial at every position.
    ValueError for an even window, a window outside [3, 33], or polyorder >= window."""
    window, polyorder = ops._savgol_window(window, name="window_length"), int(polyorder)
    if polyorder >= window or polyorder < 0:
        raise ValueError(f"polyorder must be in [0, window_length), got {polyorder} for a window of {window}")
    h = window // 2
    pos = (np.arange(window, dtype=np.float64) - h) / h
    A = pos[:, None] ** np.arange(polyorder + 1)[None, :]
    Q = np.linalg.qr(A)[0]
    H = Q @ Q.T
    return np.concatenate([H[h], H[:h].reshape(-1), H[window - h:].reshape(-1)])


def head_pose_from_landmarks(landmarks, neutral, static_idx, valid=None, window_length=5, polyorder=2, return_details=False):
    """Yaw / pitch / roll in degrees per frame, (F, 3) fp32 on the device, as the reference's Step 2 pickles them.

    landmarks: one (F, P, 3) fp32 device tensor, or a list of them (clips of different lengths, one P): they are
    concatenated once and each kernel is launched once for the whole list; a list comes back as a list.
    neutral (N, 3): the canonical face; static_idx (S), 3 <= S <= ops.HEADPOSE_MAX_STATIC, each below min(N, P): the rigid landmarks the fit uses.
    valid: per clip a bool array (F), False where the tracker found no face (None: every frame is valid).  Missing frames are
    filled as `gap_plan` says; what the landmark array holds at those frames is never read.
    The reference also lets a frame whose landmarks are all zero hold its predecessor; after its own gap filling no such
    frame is left, so that pass is dead code and is not mirrored here: mark such frames invalid.
    window_length / polyorder: the Savitzky-Golay filter over the quaternion components (the reference runs 5 / 2).

    return_details: also a dict (or a list of dicts) with R (F, 3, 3) the raw per-frame fit, c (F), t (F, 3), aligned
    (F, P, 3) = c R x + t, and R_smoothed (F, 3, 3), the matrix of the returned angles (the reference's R_modified).

    Outside the contract: agreement with the reference on static landmarks that are collinear or coplanar (collinear ones
    have no fit; three points still get the rotation they determine), and |pitch| within 1e-3 degrees of 90."""
    clips, single = clip_list(landmarks)
    valids = [valid] if single else (list(valid) if valid is not None else [None] * len(clips))
    if len(valids) != len(clips):
        raise ValueError(f"{len(clips)} clips but {len(valids)} valid arrays")
    ops._need_cuda(*clips)
    table = savgol_table(window_length, polyorder)
    L, offsets, _ = flatten_clips(clips, (None, 3))
    P, dev = L.shape[1], L.device
    plan_a, plan_b, plan_w = [], [], []
    for begin, end, v in zip(offsets[:-1], offsets[1:], valids):
        F = end - begin
        if F < window_length:
            raise ValueError(f"a clip of {F} frames is shorter than window_length = {window_length}")
        v = np.ones(F, bool) if v is None else np.asarray(v)
        if v.shape != (F,):
            raise ValueError(f"valid has shape {v.shape} for a clip of {F} frames")
        a, b, w = gap_plan(v)
        plan_a.append(a + begin)
        plan_b.append(b + begin)
        plan_w.append(w)
    neutral = np.asarray(neutral.detach().cpu() if torch.is_tensor(neutral) else neutral, dtype=np.float32)
    sidx = np.asarray(static_idx.detach().cpu() if torch.is_tensor(static_idx) else static_idx).astype(np.int64).reshape(-1)
    if neutral.ndim != 2 or neutral.shape[1] != 3:
        raise TypeError(f"neutral must have shape (N, 3), got {neutral.shape}")
    if not 3 <= sidx.size <= ops.HEADPOSE_MAX_STATIC:
        raise ValueError(f"static_idx must hold 3 .. {ops.HEADPOSE_MAX_STATIC} indices, got {sidx.size}")
    if sidx.min() < 0 or sidx.max() >= min(P, neutral.shape[0]):
        raise ValueError(f"static_idx must lie in [0, {min(P, neutral.shape[0])}): the landmarks have {P} points, neutral {neutral.shape[0]}")
    rows = np.zeros((P, 3), np.float32)                 # the kernel takes (P, 3) and reads it at static_idx only
    rows[:min(P, neutral.shape[0])] = neutral[:P]
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    R, c, t, aligned = ops.headpose_fit(L, up(np.concatenate(plan_a), torch.int32), up(np.concatenate(plan_b), torch.int32),
                                        up(np.concatenate(plan_w), torch.float32), up(rows, torch.float32),
                                        up(sidx, torch.int32), want_aligned=return_details)
    ypr, R_mod = ops.headpose_smooth(R, offsets, up(table, torch.float64), window_length, want_matrix=return_details)
    cut = lambda x: cut_clips(x, offsets)
    out = cut(ypr)
    if not return_details:
        return out[0] if single else out
    details = [dict(R=r, c=cc, t=tt, aligned=al, R_smoothed=rm)
               for r, cc, tt, al, rm in zip(cut(R), cut(c), cut(t), cut(aligned), cut(R_mod))]
    return (out[0], details[0]) if single else (out, details)


def save_head_rot(path, ypr):
    """The reference's head-rotation pickle: a float64 numpy array (F, 3) of yaw / pitch / roll in degrees."""
    a = np.asarray(ypr.detach().cpu() if torch.is_tensor(ypr) else ypr, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"head rotation must have shape (F, 3), got {a.shape}")
    with open(path, "wb") as f:
        pkl.dump(a, f)


def load_canonical_obj(path):
    """The vertices of a Wavefront .obj, (N, 3) float64: its `v` lines only."""
    verts = []
    with open(path, errors="replace") as f:
        for line in f:
            if line.startswith("v "):
                verts.append([float(x) for x in line.split()[1:4]])
    if not verts:
        raise ValueError(f"{path} has no `v` line")
    return np.array(verts, np.float64)


def load_static_indices(mapping_json):
    """The rigid landmarks of the reference's fit: nose.dorsum + nose.tipLower + additional_anchors of the semantic mapping."""
    with open(mapping_json) as f:
        m = json.load(f)
    return np.array(m["nose"]["dorsum"] + m["nose"]["tipLower"] + m["additional_anchors"], np.int32)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="head rotation pickle of a style clip from tracked face landmarks")
    p.add_argument("--landmarks", required=True, help=".npy, (F, P, 3)")
    p.add_argument("--valid", default=None, help=".npy, (F) bool: frames the tracker found a face in (default: all)")
    p.add_argument("--neutral", required=True, help="the canonical face, Wavefront .obj")
    p.add_argument("--mapping", required=True, help="the semantic index mapping, .json")
    p.add_argument("--out", required=True, help="the pickle to write")
    p.add_argument("--window_length", type=int, default=5)
    p.add_argument("--polyorder", type=int, default=2)
    p.add_argument("--device", default="cuda")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    L = torch.from_numpy(np.load(args.landmarks).astype(np.float32)).to(args.device)
    valid = None if args.valid is None else np.load(args.valid).astype(bool)
    ypr = head_pose_from_landmarks(L, load_canonical_obj(args.neutral), load_static_indices(args.mapping), valid,
                                   args.window_length, args.polyorder)
    save_head_rot(args.out, ypr)
    print(f"wrote {args.out}: {tuple(ypr.shape)} yaw / pitch / roll in degrees")


if __name__ == "__main__":
    main()
