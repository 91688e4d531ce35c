"""Windowed inference driver (drop-in surface of reference inference.py:34-75, 85-103).

``infer_coeffs`` keeps the reference's signature and window maths (bit-exact integer arithmetic) and
its behaviours (one encoder pass over the whole zero-padded clip; window i>0 re-uses window 0's x_T,
inference.py:64; last 10 motion/audio frames handed to the next window).

SURVEY.md section 8(f) n3, the callers either side of the sampler:
  * ``normalize_motion_coeff`` / ``query_for_motion_coeff`` -- style-clip ingestion (inference.py:109-183): coefficient
    statistics, optional 30 -> 25 fps linear resampling on a normalised time axis (scipy.interpolate.interp1d's
    linear rule), concatenation to (1, T, 53) + the dummy (1, 100) shape row;
  * ``denormalize_coeffs`` -- output de-normalisation (inference.py:274-275);
  * ``infer_coeffs_batch`` -- many clips at once: window i of every clip that still has one goes through ONE
    ``model.sample`` call (the sampler is launch-bound at batch 1: 0.71 ms/step at B = 1 vs 3.5 ms/step at B = 64), one
    encoder pass per distinct padded length; per-clip results equal ``infer_coeffs`` on that clip.
  * ``render_coeffs`` -- coefficients -> FLAME vertices -> images on the device (utils/renderer.MeshRenderer), the step the
    reference script leaves as a comment (inference.py:277-279) and its utils/renderer.py serves.
  * ``load_audio_16k`` -- a `.wav` of any rate and channel count -> 16 kHz mono on the device (utils/audio.py, csrc/audio_io.hip).
  * ``--video`` -- the frames, JPEG-compressed on the device chunk by chunk (csrc/jpeg.hip), and the input WAV as one
    Motion-JPEG AVI (utils/media.py), where the reference calls ffmpeg (utils/media.py:combine_frames_and_audio).
  * ``--source_video`` -- a Motion-JPEG AVI shown left of the render in that video, sampled to the render's frame rate and resized
    to its height on the device (csrc/resize.hip).
  * ``--texture`` -- an `.npz` with `tex_img`, `vt`, `ft`: the frames are drawn with that texture.
  * ``--flame_tex`` -- an albedo `.npz` (BFM or FLAME texture space, plus `vt`, `ft`): the texture is evaluated by
    utils/flame.FLAMETex from ``--tex_code`` (default: the mean face) and the frames are drawn with it.
  * ``--style_adherence`` -- every generated frame's soft-min distance to the whole normalised style clip
    (utils/common.StyleAdherenceLoss), written beside the pickles.
The rest of the reference script's media IO (compressed audio codecs, cv2, H.264) stays outside.
"""
from __future__ import annotations

import math
import pickle as pkl
from pathlib import Path

import numpy as np

import torch
import torch.nn.functional as F

from .model import get_diffusion_model
from .sampler import DenseGuide
from .style_encoder import get_style_encoder
from .utils.common import coef_dict_to_vertices, get_coef_dict
from .utils.model_common import load_args


def window_plan(n_samples: int, fps, n_motions: int, audio_unit: float):
    """reference inference.py:38-43."""
    clip_len = int(n_samples / 16000 * fps)
    n_audio_samples = round(audio_unit * n_motions)
    n_subdivision = 1 if clip_len <= n_motions else math.ceil(clip_len / n_motions)
    n_padding_audio_samples = n_audio_samples * n_subdivision - n_samples
    n_padding_frames = math.ceil(n_padding_audio_samples / audio_unit)
    return clip_len, n_audio_samples, n_subdivision, n_padding_audio_samples, n_padding_frames


def window_keyframes(keyframes, clip_len: int, n_motions: int, n_windows: int):
    """Keyframes of a whole clip -> per-window local guidance.  keyframes = (frame_indices, values): indices in [0, clip_len)
    along the clip (an index >= clip_len or < 0 raises IndexError), values (K, C).  Returns a list of n_windows entries, each
    (local index list, values (k, C)) for the keyframes that fall into that window, in their given order, or None."""
    if keyframes is None:
        return [None] * n_windows
    frames, values = keyframes
    frames = [int(f) for f in (frames.tolist() if hasattr(frames, "tolist") else frames)]
    if len(frames) != len(values):
        raise ValueError(f"keyframes: {len(frames)} frame indices for {len(values)} rows of values")
    for f in frames:
        if not 0 <= f < clip_len:
            raise IndexError(f"keyframe index {f} is out of range for a clip of {clip_len} frames")
    out = []
    for w in range(n_windows):
        mine = [j for j, f in enumerate(frames) if f // n_motions == w]
        rows = values[mine] if hasattr(values, "shape") else [values[j] for j in mine]      # tensor / array, or a list of rows
        out.append(([frames[j] - w * n_motions for j in mine], rows) if mine else None)
    return out


@torch.no_grad()
def infer_coeffs(model, args, audio, shape_coef, audio_unit, style_feats=None, n_repetitions: int = 1, cfg_mode=None,
                 cfg_cond=None, cfg_scale: float = 1.15, include_shape: bool = False, dynamic_threshold=(0, 1, 4),
                 noise=None, sample_steps=None, solver="ddpm", eta=0.0, *, keyframes=None):
    """Coefficients for one clip of any length (reference inference.py:34-75; same signature, window arithmetic and hand-off
    rules).  The clip is zero-padded to a whole number of n_motions-frame windows and encoded ONCE; each window is one
    `model.sample` call conditioned on the previous window's last n_prev_motions motion / audio-feature frames, every
    window after the first starts from window 0's x_T, and the frames that only cover the padding are cut from the result.
    ``noise`` (optional, replay): {'xT': tensor, 'z': [per-window dict of per-step draws]}.
    ``sample_steps`` / ``solver`` / ``eta``: the sampler of every window (MSMD.sample); the default is the reference's.
    ``keyframes`` = (frame_indices, values (K, C)): poses pinned along the whole clip; every window receives its own as local
    guidance (MSMD.sample_with_guide), a window without any takes the plain call.  On the graph loop the two kinds of window have
    two captures, and one graph is resident per model: a clip pinned in windows 0 and 2 but not 1 captures three times."""
    L, keep = args.n_motions, args.n_prev_motions
    clip_len, _, n_windows, pad_samples, pad_frames = window_plan(len(audio), args.fps, L, audio_unit)
    pinned = window_keyframes(keyframes, clip_len, L, n_windows)
    tail = max(pad_frames, 0)                       # frames of the last window that lie entirely in the zero padding
    wave = F.pad(audio, (0, pad_samples), value=0) if pad_samples > 0 else audio
    per_window = model.extract_audio_feature(wave.unsqueeze(0), L * n_windows).split(L, dim=1)
    guidance = dict(cfg_mode=cfg_mode, cfg_cond=cfg_cond, cfg_scale=cfg_scale, dynamic_threshold=dynamic_threshold,
                    sample_steps=sample_steps, solver=solver, eta=eta)
    history = (None, None, None if noise is None else noise["xT"])      # (prev motion, prev audio features, x_T)
    pieces = []
    for w, feat in enumerate(per_window):
        cut = tail if w == n_windows - 1 else 0
        indicator = None
        if args.use_indicator:
            indicator = torch.ones((n_repetitions, L), device=model.device)
            if cut:
                indicator[:, L - cut:] = 0
        style = style_feats[w] if isinstance(style_feats, list) else style_feats
        call, kf = model.sample, {}
        if pinned[w] is not None:
            call, kf = model.sample_with_guide, dict(guidance_indice=pinned[w][0], guidance_values=pinned[w][1])
        x0, x_T, feat_used = call(feat.expand(n_repetitions, -1, -1), shape_coef, style, *history, indicator=indicator,
                                  noise=None if noise is None else noise["z"][w], **guidance, **kf)
        history = (x0[:, -keep:].clone(), feat_used[:, -keep:], x_T)
        pieces.append(x0[:, :L - cut] if cut else x0)
    return torch.cat(pieces, dim=1)


def load_model(model_root: str, model_name: str, iter_num: str, device: torch.device):
    """reference inference.py:85-103 (same directory layout and checkpoint keys)."""
    import os
    model_args = load_args(Path(os.path.join(model_root, "DPT", model_name)))
    # the checkpoint holds every audio-encoder tensor (strict load below): no Hugging Face copy is needed to rebuild the model
    model_args.audio_encoder_weights = "checkpoint"
    model = get_diffusion_model(model_args, device)
    ckpt = Path(model_root) / "DPT" / model_name / "checkpoints" / f"iter_{iter_num}.pt"
    data = torch.load(ckpt, map_location=device, weights_only=False)  # reference checkpoints pickle their args Namespace
    style_enc = get_style_encoder(model_args, model_args.style_enc_model_style)
    style_enc.load_state_dict(data["style_enc"])
    style_enc.to(device).eval()
    model.load_state_dict(data["model"])
    model.eval()
    return model, style_enc, model_args


# ----------------------------------------------------------------------------- style-clip ingestion / output scaling
def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def resample_linear(x, n_out):
    """scipy.interpolate.interp1d(linspace(0, 1, n), x, axis=0)(linspace(0, 1, n_out)) (inference.py:160-170): linear
    interpolation on a normalised time axis, endpoints included."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if n_out == n:
        return x
    xs, xn = np.linspace(0, 1, num=n), np.linspace(0, 1, num=n_out)
    hi = np.clip(np.searchsorted(xs, xn, side="left"), 1, n - 1)   # interp1d: x_new in (xs[hi-1], xs[hi]]
    lo = hi - 1
    slope = (x[hi] - x[lo]) / (xs[hi] - xs[lo])[:, None]
    return slope * (xn - xs[lo])[:, None] + x[lo]


def normalize_motion_coeff(expression_coef, head_rot, coef_stats, device="cuda", original_fps=30, target_fps=25):
    """Body of reference query_for_motion_coeff (inference.py:139-181) on in-memory arrays / tensors."""
    e = (_np(expression_coef) - _np(coef_stats["exp_mean"])) / (_np(coef_stats["exp_std"]) + 1e-9)
    h = (_np(head_rot) - _np(coef_stats["pose_mean"])) / (_np(coef_stats["pose_std"]) + 1e-9)
    if original_fps is not None and original_fps != target_fps:
        n_new = int(round(e.shape[0] / original_fps * target_fps))
        e, h = resample_linear(e, n_new), resample_linear(h, n_new)
    et = torch.from_numpy(np.ascontiguousarray(e)).to(device).unsqueeze(0).float()
    ht = torch.from_numpy(np.ascontiguousarray(h)).to(device).unsqueeze(0).float()
    return torch.cat([et, ht], dim=2).float(), torch.zeros((1, 100), device=device).float()


def query_for_motion_coeff(args, expression_code_full_path, head_rot_full_path, device="cuda", original_fps=30,
                           target_fps=25):
    """reference inference.py:109-183 (same signature; pickle inputs)."""
    with open(args.coef_dict_path, "rb") as f:
        coef_stats = pkl.load(f)
    with open(expression_code_full_path, "rb") as f:
        expression_coef = pkl.load(f)
    with open(head_rot_full_path, "rb") as f:
        head_rot = pkl.load(f)
    return normalize_motion_coeff(expression_coef, head_rot, coef_stats, device, original_fps, target_fps)


def denormalize_coeffs(overall_coef, coef_stats):
    """reference inference.py:274-275: (n_rep, T, 53) normalised -> (expression code (T, 50), head rotation (T, 3))
    of repetition 0 in the data's units."""
    st = {k: (v.to(overall_coef.device) if torch.is_tensor(v) else torch.as_tensor(v, device=overall_coef.device))
          for k, v in coef_stats.items()}
    return (overall_coef[0, :, :-3] * st["exp_std"] + st["exp_mean"],
            overall_coef[0, :, -3:] * st["pose_std"] + st["pose_mean"])


@torch.no_grad()
def style_adherence_per_frame(coef, style_clip, lambda_softmin=10.0):
    """(1, T, C) generated coefficients against (1, K, C) style-clip coefficients, both normalised -> (T,) fp32: every frame's
    soft-min mean squared distance to the clip's frames (utils/common.StyleAdherenceLoss, reduce=False)."""
    from .utils.common import StyleAdherenceLoss
    return StyleAdherenceLoss(True, lambda_softmin)(coef, style_clip, reduce=False)[0]


@torch.no_grad()
def render_coeffs_chunks(coef, shape_coef, flame, coef_stats, renderer, chunk=512, *, with_global_pose=True, tex_img=None,
                         tex_uv=None):
    """`render_coeffs` as a generator: yields the frames of `chunk` coefficients at a time, (n, H, W, 3) uint8 views of the
    renderer's RGBA buffer, so a consumer that compresses each chunk keeps one chunk of raw pixels alive.  tex_img / tex_uv:
    a texture for FLAME's faces, as MeshRenderer.render_vertices takes it."""
    coef = coef.reshape(-1, coef.shape[-1]).float()
    if coef.shape[-1] == 53:
        coef = torch.cat([coef, torch.zeros_like(coef[:, :1])], dim=-1)
    shape = shape_coef.reshape(-1, shape_coef.shape[-1]).float().expand(coef.shape[0], -1)
    for i in range(0, coef.shape[0], chunk):
        coef_dict = get_coef_dict(coef[i:i + chunk], shape[i:i + chunk], coef_stats, with_global_pose=with_global_pose)
        verts = coef_dict_to_vertices(coef_dict, flame, flame_batch_size=chunk)
        yield renderer.render_vertices(verts, flame.faces_tensor, tex_img=tex_img, tex_uv=tex_uv)[0]


@torch.no_grad()
def render_coeffs(coef, shape_coef, flame, coef_stats, renderer, chunk=512, *, with_global_pose=True, tex_img=None, tex_uv=None):
    """Motion coefficients (T, C) or (1, T, C) -> frames (T, H, W, 3) uint8 on the device: get_coef_dict -> coef_dict_to_vertices
    -> renderer.render_vertices on FLAME's faces, `chunk` frames at a time (one chunk's vertices are the only intermediate
    alive).  coef is in get_coef_dict's layout (50 expression + 4 pose: global rotation, jaw opening); a 53-wide row
    (expression + head rotation, what `denormalize_coeffs` returns side by side) gets a closed jaw.  coef_stats: None for
    coefficients in the data's units, or get_coef_dict's denorm_stats (`exp` / `pose` / `shape` means and stds).
    shape_coef: (1, 100) or (T, 100).  tex_img (Ht, Wt, 3 | 4) uint8 with tex_uv = {'vt', 'ft'} draws the frames textured
    (MeshRenderer.render_vertices)."""
    return torch.cat(list(render_coeffs_chunks(coef, shape_coef, flame, coef_stats, renderer, chunk,
                                               with_global_pose=with_global_pose, tex_img=tex_img, tex_uv=tex_uv)), dim=0)


# ----------------------------------------------------------------------------- many clips per denoise step
@torch.no_grad()
def infer_coeffs_batch(model, args, audios, shape_coefs, audio_unit, style_feats, cfg_mode=None, cfg_cond=None,
                       cfg_scale: float = 1.15, dynamic_threshold=(0, 1, 4), noise=None, sample_steps=None, solver="ddpm",
                       eta=0.0, *, keyframes=None):
    """`infer_coeffs` for a list of clips (1-D audio tensors of any lengths), one repetition each, with window i of
    all clips batched into one `model.sample` call.  shape_coefs: (n_clips, 100); style_feats: (n_clips, d_style).
    `noise` (optional): list of per-clip {'xT', 'z'} dicts as `infer_coeffs` takes; `sample_steps` / `solver` / `eta`
    as `infer_coeffs` takes them; `keyframes`: one (frame_indices, values) pair or None per clip, as `infer_coeffs` takes
    it (a window in which no active clip has a keyframe takes the plain call); clips pin different frames, which needs a
    few-step solver (solver="ddpm" raises ValueError: loop over `infer_coeffs` there).  Returns a list of (1, clip_len, C)
    tensors, clip c equal to infer_coeffs(model, args, audios[c], shape_coefs[c:c+1], audio_unit, style_feats[c:c+1])."""
    n = len(audios)
    L, Lp = args.n_motions, args.n_prev_motions
    plans = [window_plan(len(a), args.fps, L, audio_unit) for a in audios]
    if keyframes is not None and solver == "ddpm":
        raise ValueError("infer_coeffs_batch: per-clip keyframes need solver='ddim' or 'dpmpp_2m' (solver='ddpm': one "
                         "infer_coeffs call per clip)")
    if keyframes is not None and len(keyframes) != n:
        raise ValueError(f"keyframes: one entry per clip expected ({n}), got {len(keyframes)}")
    pinned = [window_keyframes(keyframes[c] if keyframes is not None else None, plans[c][0], L, plans[c][2]) for c in range(n)]
    # one encoder pass per distinct padded length
    feats = [None] * n
    by_sub = {}
    for c, pl in enumerate(plans):
        by_sub.setdefault(pl[2], []).append(c)
    for n_sub, clips in by_sub.items():
        batch = torch.stack([F.pad(audios[c], (0, plans[c][3]), value=0) if plans[c][3] > 0 else audios[c]
                             for c in clips])
        f = model.extract_audio_feature(batch, L * n_sub)
        for j, c in enumerate(clips):
            feats[c] = f[j:j + 1]
    outs = [[] for _ in range(n)]
    prev_m = [None] * n
    prev_a = [None] * n
    x_T = [None] * n
    for i in range(max(pl[2] for pl in plans)):
        act = [c for c in range(n) if i < plans[c][2]]
        ind = torch.ones((len(act), L), device=model.device) if args.use_indicator else None
        for j, c in enumerate(act):
            if ind is not None and i == plans[c][2] - 1 and plans[c][4] > 0:
                ind[j, -plans[c][4]:] = 0
        audio_in = torch.cat([feats[c][:, i * L:(i + 1) * L] for c in act], dim=0)
        kw = dict(indicator=ind, cfg_mode=cfg_mode, cfg_cond=cfg_cond, cfg_scale=cfg_scale,
                  dynamic_threshold=dynamic_threshold, sample_steps=sample_steps, solver=solver, eta=eta)
        if noise is not None:
            kw["noise"] = {t: torch.cat([noise[c]["z"][i][t] for c in act], dim=0) for t in noise[act[0]]["z"][i]}
        idx = torch.as_tensor(act, device=model.device)
        shape_in, style_in = shape_coefs[idx], style_feats[idx]
        call = model.sample
        if any(pinned[c][i] is not None for c in act):
            call = model.sample_with_guide
            kw["guidance_indice"] = DenseGuide.stack([pinned[c][i] for c in act], L, model.motion_feat_dim)
        if i == 0:
            xT = torch.cat([noise[c]["xT"] for c in act], dim=0) if noise is not None else None
            motion, nT, pa = call(audio_in, shape_in, style_in, motion_at_T=xT, **kw)
        else:
            # windows i > 0 re-use their clip's x_T and take the previous window's last frames (inference.py:60-69);
            # model.sample substitutes the learned start tokens only when BOTH prev tensors are None, which cannot
            # happen here because every active clip ran window i - 1
            motion, nT, pa = call(audio_in, shape_in, style_in, torch.cat([prev_m[c] for c in act], dim=0),
                                  torch.cat([prev_a[c] for c in act], dim=0), torch.cat([x_T[c] for c in act], dim=0), **kw)
        for j, c in enumerate(act):
            prev_m[c] = motion[j:j + 1, -Lp:].clone()
            prev_a[c] = pa[j:j + 1, -Lp:]
            x_T[c] = nT[j:j + 1]
            m = motion[j:j + 1]
            if i == plans[c][2] - 1 and plans[c][4] > 0:
                m = m[:, :-plans[c][4]]
            outs[c].append(m)
    return [torch.cat(o, dim=1) for o in outs]


# ----------------------------------------------------------------------------- command line (reference flag names)
def build_parser():
    """The reference's inference flags (inference.py:190-201), same names and defaults."""
    import argparse
    ap = argparse.ArgumentParser(description="Single style + audio inference for MSMD on MI355X.")
    for name in ("model_root", "model_name", "model_iter", "style_clip_exp_code_path", "style_clip_head_rot_path",
                 "audio_clip"):
        ap.add_argument("--" + name, type=str, required=True)
    ap.add_argument("--coef_dict_path", type=str, default="PATH-TO-COEF-STATS")
    ap.add_argument("--cfg_level", type=float, default=1.4)
    ap.add_argument("--output_dir", type=str, default="/experiments/refactor")
    ap.add_argument("--versions_of_render", type=int, default=1)
    # sampler choice (not in the reference; the defaults are its DDPM chain over all n_diff_steps)
    ap.add_argument("--sample_steps", type=int, default=None, help="steps of a few-step solver (default: all)")
    ap.add_argument("--solver", type=str, default="ddpm", choices=["ddpm", "ddim", "dpmpp_2m"])
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise scale: 0 deterministic, 1 ancestral")
    # rendering (the reference script stops before it; 0 = off: the files written are then exactly the two pickles)
    ap.add_argument("--render_size", type=int, default=0, help="side of the square frames rendered from the result (0: none)")
    ap.add_argument("--render_samples", type=int, default=1, choices=(1, 4),
                    help="sample points per pixel of the rendered frames: 4 draws them anti-aliased (needs --render_size > 0)")
    ap.add_argument("--flame_model_path", type=str, default=None, help="FLAME generic_model.pkl (with --render_size)")
    ap.add_argument("--flame_lmk_embedding_path", type=str, default=None, help="FLAME landmark embedding (with --render_size)")
    ap.add_argument("--texture", type=str, default=None, help=".npz with tex_img (Ht, Wt, 3 | 4) uint8, vt (Nt, 2) and ft (F, 3) "
                                                              "for FLAME's faces: the frames are drawn textured "
                                                              "(needs --render_size > 0)")
    ap.add_argument("--flame_tex", type=str, default=None, help="albedo .npz (MU / PC for BFM, mean / tex_dir for FLAME) that also "
                                                                "holds vt (Nt, 2) and ft (F, 3): the frames are drawn with the "
                                                                "FLAMETex texture of --tex_code (needs --render_size > 0)")
    ap.add_argument("--tex_type", type=str, default="BFM", choices=["BFM", "FLAME"], help="texture space of --flame_tex")
    ap.add_argument("--tex_code", type=str, default=None, help=".npy texture code, (n_tex,) or (1, n_tex) (default: zeros, the "
                                                               "mean face; needs --flame_tex)")
    # video (the reference pipes frames and audio through ffmpeg; here a Motion-JPEG AVI is written, utils/media.py)
    ap.add_argument("--video", action="store_true", help="write video_<clip>_seed_<s>.avi instead of the raw frames "
                                                         "(needs --render_size > 0)")
    ap.add_argument("--video_quality", type=int, default=90, help="JPEG quality of the video's frames, 1 .. 100")
    ap.add_argument("--source_video", type=str, default=None, help="Motion-JPEG AVI shown left of the render in the video, sampled "
                                                                   "to the render's frame rate and scaled to its height (needs --video)")
    # metric (not in the reference script; the loss is its utils/common.StyleAdherenceLoss)
    ap.add_argument("--style_adherence", action="store_true", help="write style_adherence_<clip>_seed_<s>.npy: every generated "
                                                                   "frame's soft-min distance to the whole style clip")
    # retargeting (not in the reference: DESIGN.md 5.33)
    ap.add_argument("--retarget", type=str, default=None, metavar="RIG.npz",
                    help="blendshape rig on FLAME's topology (utils/retarget.load_rig): write retarget_<clip>_seed_<s>.csv, one "
                         "weight curve per slider (needs --flame_model_path)")
    ap.add_argument("--comparison_video", action="store_true",
                    help="with --retarget: also write retarget_<clip>_seed_<s>.avi, FLAME | the rig's reconstruction | its error "
                         "heat map (needs --render_size > 0)")
    return ap


def parse_args(argv=None):
    """build_parser().parse_args with the checks that span flags: --video, --render_samples 4, --texture and --flame_tex need --render_size > 0,
    --flame_tex and --texture exclude each other, --tex_code needs --flame_tex, and the quality lies in [1, 100]."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.video and args.render_size <= 0:
        ap.error("--video needs --render_size > 0: there are no frames to encode")
    if args.render_samples != 1 and args.render_size <= 0:
        ap.error("--render_samples needs --render_size > 0: there are no frames to draw")
    if args.texture is not None and args.render_size <= 0:
        ap.error("--texture needs --render_size > 0: there are no frames to draw it on")
    if args.flame_tex is not None and args.render_size <= 0:
        ap.error("--flame_tex needs --render_size > 0: there are no frames to draw it on")
    if args.flame_tex is not None and args.texture is not None:
        ap.error("--flame_tex and --texture both name the frames' texture: give one")
    if args.tex_code is not None and args.flame_tex is None:
        ap.error("--tex_code needs --flame_tex: there is no texture space to evaluate it in")
    if not 1 <= args.video_quality <= 100:
        ap.error(f"--video_quality {args.video_quality} is outside [1, 100]")
    if args.source_video is not None and not args.video:
        ap.error("--source_video needs --video: it is a panel of the video")
    if args.retarget is not None and args.flame_model_path is None:
        ap.error("--retarget needs --flame_model_path: the rig is fitted to FLAME's vertices")
    if args.comparison_video and (args.retarget is None or args.render_size <= 0):
        ap.error("--comparison_video needs --retarget and --render_size > 0: it draws the rig's reconstruction")
    return args


@torch.no_grad()
def write_retarget(coef, shape_coef, flame, rig, fps, csv_path, video_path=None, renderer=None, quality=90, chunk=256,
                   with_global_pose=False):
    """Motion coefficients (T, 53 | 54) in the data's units -> FLAME vertices -> blendshape weights (utils/retarget.py), written to
    `csv_path` (or .json) as one curve per slider.  The head is held still unless with_global_pose: a rig's neutral does not
    turn.  video_path: also a Motion-JPEG AVI of FLAME (as ground truth) | the rig's reconstruction | its error heat map through
    utils/metrics.render_comparison, the colour scale topped at the clip's largest error (a second pass over the chunks).
    -> {'frames', 'mean', 'max', 'rms' (vertex error of the reconstruction), 'flagged' (frames whose status is not 0)}."""
    from .utils import retarget as RT
    from .utils.metrics import VertexMetrics, _scale_or_one, _track
    coef = _track(coef)
    T = coef.shape[0]
    if T < 1:
        raise ValueError("no frames to retarget")
    rig = RT.prepare_rig(rig, coef.device)
    shape = shape_coef.reshape(-1, shape_coef.shape[-1]).float().expand(T, -1)
    cd = get_coef_dict(coef, shape, None, with_global_pose=with_global_pose)
    vm = VertexMetrics([0, T], rig.V, [0], [0], rig.neutral, coef.device)
    weights, status = RT.retarget_coeffs(cd, flame, rig, chunk, on_chunk=lambda v, w, i: vm.update(RT.rig_vertices(w, rig), v))
    RT.write_curves(csv_path, weights, rig.names, fps)
    r = vm.result()["all"]
    rep = dict(frames=T, mean=r["mve"], max=r["max_ve"], rms=r["rmse"], flagged=int((status != 0).sum()))
    if video_path is not None:
        from .utils import media
        vmax, jpegs = _scale_or_one(r["max_ve"]), []
        for v, i in RT._flame_chunks(cd, flame, chunk):
            jpegs += media.encode_jpeg(RT.comparison_frames(v, weights[i:i + v.shape[0]], rig, flame.faces_tensor, renderer, vmax).contiguous(),
                                       quality)
        media.write_avi(video_path, jpegs, fps, (3 * renderer.width, renderer.height))
    return rep


def load_source_panel(path, height, device="cuda"):
    """--source_video's clip as the left panel of the video -> (frames (F, height, W', 3) uint8 on the device, fps as a Fraction):
    decoded and scaled chunk by chunk (utils/media.read_video(size=)) to the render's height, the width keeping the aspect as
    `media.side_by_side` rounds it."""
    from . import ops
    from .utils import media
    clip = media.read_avi(path)
    w, h = clip.size
    if w < 1 or h < 1:
        head = ops.jpeg_parse(clip.jpeg(0))[0]
        w, h = head["width"], head["height"]
    width = max(1, (2 * w * height + h) // (2 * h))
    return media.read_video(path, device=device, size=(width, height)), clip.fps


def beside_source(part, first, source, source_fps, fps):
    """The frames [first, first + n) of the render, `part` (n, H, W, 3 | 4) uint8, with the source panel left of them: the source
    frame of every output frame is `media.frames_at`'s, the one nearest in time."""
    from .utils import media
    n = part.shape[0]
    idx = media.frames_at(first + n, fps, source.shape[0], source_fps)[first:]
    left = source[torch.tensor(idx, device=source.device)]
    return media.side_by_side([left, part[..., :3]], height=part.shape[1])


def load_texture(path):
    """--texture's `.npz` -> (tex_img, {'vt', 'ft'}) as MeshRenderer takes them."""
    with np.load(path) as z:
        missing = [k for k in ("tex_img", "vt", "ft") if k not in z.files]
        if missing:
            raise ValueError(f"{path} lacks {missing}: a texture file holds tex_img, vt and ft")
        return z["tex_img"], {"vt": z["vt"], "ft": z["ft"]}


def load_flame_texture(path, tex_type="BFM", code_path=None, device="cuda"):
    """--flame_tex's `.npz` -> (tex_img (256, 256, 3) uint8 on the device, {'vt', 'ft'}) as MeshRenderer takes them: the albedo
    space is loaded into utils/flame.FLAMETex with every component the file holds and evaluated at the code of `code_path`
    (`.npy`, (n_tex,) or (1, n_tex); None = zeros, the mean face)."""
    from types import SimpleNamespace
    from .utils.flame import FLAMETex
    pc_key = {"BFM": "PC", "FLAME": "tex_dir"}.get(tex_type)
    if pc_key is None:
        raise NotImplementedError(f"texture type {tex_type!r} does not exist")
    with np.load(path) as z:
        missing = [k for k in ("vt", "ft") if k not in z.files]
        if missing:
            raise ValueError(f"{path} lacks {missing}: an albedo file for rendering also holds vt and ft")
        asset = {k: z[k] for k in z.files}
    n_tex = asset[pc_key].shape[-1]
    tex = FLAMETex(SimpleNamespace(tex_type=tex_type, n_tex=n_tex, tex_asset=asset)).to(device)
    code = np.zeros((1, n_tex), np.float32) if code_path is None else np.load(code_path).astype(np.float32)
    if code.shape not in ((n_tex,), (1, n_tex)):
        raise ValueError(f"{code_path} has shape {code.shape}: a texture code is ({n_tex},) or (1, {n_tex})")
    return tex.image(torch.from_numpy(code.reshape(1, n_tex)).to(device)), {"vt": asset["vt"], "ft": asset["ft"]}


def load_audio_16k(path, device="cuda"):
    """16 kHz mono float32 samples, un-normalised.  A `.wav` of any rate and channel count is read, downmixed and resampled on
    the device (utils/audio.load_clips; the reference calls librosa.load(path, sr=16000), inference.py:232); a `.npy` or a
    pickle holds samples somebody else has already decoded to 16 kHz mono (`device` is not used for those).  The `.wav`
    suffix is matched in either case (recorders write `.WAV`).  Compressed codecs stay outside."""
    path = str(path)
    if path.lower().endswith(".wav"):
        from .utils.audio import load_clips
        return load_clips([path], device, normalize=False)[0].cpu().numpy()
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32)
    with open(path, "rb") as f:
        return np.asarray(pkl.load(f), dtype=np.float32)


def main(argv=None):
    """The non-media part of reference inference.py:189-279: load model + style encoder, ingest the style clip, z-norm
    the audio, sample the style code, run infer_coeffs per repetition seed, de-normalise and write the two pickles
    (`overall_exp_code_*`, `overall_head_rot_*`) under <output_dir>/<model>_iter_<iter>/temp/.  With --render_size N > 0 the
    coefficients are also decoded by FLAME and rendered on the device (render_coeffs), and `frames_<clip>_seed_<s>.npy`
    ((T, N, N, 3) uint8) is written beside them.  With --video as well, `video_<clip>_seed_<s>.avi` is written in its place: the
    frames are JPEG-compressed on the device chunk by chunk as they are rendered (so one chunk of raw pixels is alive at a
    time), at model_args.fps, with --audio_clip as the sound track when it is a `.wav` and silent otherwise.  --source_video
    CLIP.avi puts that clip left of the render (`load_source_panel`, `beside_source`); the sound stays --audio_clip.  --texture PATH
    (an `.npz` with tex_img, vt, ft) draws the frames textured, in either form; --flame_tex PATH (an albedo `.npz` with vt, ft)
    does so with the FLAMETex texture of --tex_code.  --render_samples 4 draws the frames anti-aliased, four samples per pixel
    (MeshRenderer(samples=4)), in every one of these forms.  --style_adherence also writes `style_adherence_<clip>_seed_<s>.npy`, (T,)
    float32: the soft adherence (lambda 10) of repetition 0's normalised coefficients to the whole normalised style clip, and
    prints its mean; it needs the style clip's coefficients to be as wide as the model's."""
    import os
    args = parse_args(argv)
    device = torch.device("cuda")
    model, style_enc, model_args = load_model(args.model_root, args.model_name, args.model_iter, device)
    motion_coeff, shape_coef = query_for_motion_coeff(args, args.style_clip_exp_code_path, args.style_clip_head_rot_path,
                                                      device=device)
    shape_coef = shape_coef.unsqueeze(1)
    if args.audio_clip.lower().endswith(".wav"):
        from .utils.audio import load_clips
        audio_tensor = load_clips([args.audio_clip], device, normalize=True)[0]
    else:
        audio = load_audio_16k(args.audio_clip)
        audio = (audio - audio.mean()) / (audio.std() + 1e-5)
        audio_tensor = torch.from_numpy(audio).float().to(device)
    style_clip = motion_coeff[:, :100, :]
    style_coeff = style_enc.sample(style_clip) if model_args.style_enc_model_style.startswith("vae") else style_enc(style_clip)
    with open(args.coef_dict_path, "rb") as f:
        coef_stats = {k: v.to(device) for k, v in pkl.load(f).items()}
    style_name = os.path.splitext(os.path.basename(args.style_clip_exp_code_path))[0]
    audio_name = os.path.splitext(os.path.basename(args.audio_clip))[0]
    clip = f"style=_{style_name}_audio={audio_name}"
    temp = os.path.join(args.output_dir, f"{args.model_name}_iter_{args.model_iter}", "temp")
    os.makedirs(temp, exist_ok=True)
    written = []
    flame = renderer = source = source_fps = None
    tex_img, tex_uv = load_texture(args.texture) if args.texture is not None else (None, None)
    if args.flame_tex is not None:
        tex_img, tex_uv = load_flame_texture(args.flame_tex, args.tex_type, args.tex_code, device)
    if args.render_size > 0 or args.retarget is not None:
        from .utils.flame import FLAME, FLAMEConfig
        from .utils.renderer import MeshRenderer
        from types import SimpleNamespace
        cfg = SimpleNamespace(**{k: v for k, v in vars(FLAMEConfig).items() if not k.startswith("__")})
        if args.flame_model_path is not None:
            cfg.flame_model_path = args.flame_model_path
        if args.flame_lmk_embedding_path is not None:
            cfg.flame_lmk_embedding_path = args.flame_lmk_embedding_path
        flame = FLAME(cfg).to(device)
        renderer = MeshRenderer((args.render_size, args.render_size), samples=args.render_samples) if args.render_size > 0 else None
    rig = None
    if args.retarget is not None:
        from .utils.retarget import load_rig, prepare_rig
        rig = prepare_rig(load_rig(args.retarget), device)
    for seed in range(args.versions_of_render):
        np.random.seed(seed)
        torch.manual_seed(seed)
        coef = infer_coeffs(model, model_args, audio_tensor, shape_coef, 640.0, style_coeff, cfg_scale=args.cfg_level,
                            dynamic_threshold=None, sample_steps=args.sample_steps, solver=args.solver, eta=args.eta)
        exp_code, head_rot = denormalize_coeffs(coef, coef_stats)
        for tag, val in (("exp_code", exp_code), ("head_rot", head_rot)):
            out = os.path.join(temp, f"overall_{tag}_{clip}_seed_{seed}.pkl")
            with open(out, "wb") as f:
                pkl.dump(val.cpu().numpy(), f)
            written.append(out)
        if args.style_adherence:
            # the normalised coefficients of repetition 0 against the WHOLE normalised style clip, not only the 100 frames
            # the style encoder saw
            per_frame = style_adherence_per_frame(coef[0:1], motion_coeff)
            out = os.path.join(temp, f"style_adherence_{clip}_seed_{seed}.npy")
            np.save(out, per_frame.cpu().numpy())
            written.append(out)
            print(f"style adherence (seed {seed}): mean {float(per_frame.mean()):.6f} over {per_frame.numel()} frames")
        if rig is not None:
            out = os.path.join(temp, f"retarget_{clip}_seed_{seed}.csv")
            video = os.path.join(temp, f"retarget_{clip}_seed_{seed}.avi") if args.comparison_video else None
            rep = write_retarget(torch.cat([exp_code, head_rot], dim=-1), shape_coef.reshape(1, -1), flame, rig, model_args.fps, out,
                                 video, renderer, args.video_quality)
            written += [out] + ([video] if video else [])
            print(f"retarget (seed {seed}): {rep}")
        if renderer is not None and args.video:
            from .utils import media
            jpegs, first, width = [], 0, args.render_size
            if args.source_video is not None and source is None:
                source, source_fps = load_source_panel(args.source_video, args.render_size, device)
            for part in render_coeffs_chunks(torch.cat([exp_code, head_rot], dim=-1), shape_coef.reshape(1, -1), flame, None,
                                             renderer, chunk=256, tex_img=tex_img, tex_uv=tex_uv):
                if source is not None:
                    n = part.shape[0]
                    part = beside_source(part, first, source, source_fps, model_args.fps)
                    first, width = first + n, part.shape[2]
                jpegs += media.encode_jpeg(part, args.video_quality)
            sound = None
            if args.audio_clip.lower().endswith(".wav"):
                from .utils.audio import read_wav
                sound = read_wav(args.audio_clip)
            out = os.path.join(temp, f"video_{clip}_seed_{seed}.avi")
            media.write_avi(out, jpegs, model_args.fps, (width, args.render_size), sound)
            written.append(out)
        elif renderer is not None:
            frames = render_coeffs(torch.cat([exp_code, head_rot], dim=-1), shape_coef.reshape(1, -1), flame, None, renderer,
                                   tex_img=tex_img, tex_uv=tex_uv)
            out = os.path.join(temp, f"frames_{clip}_seed_{seed}.npy")
            np.save(out, frames.cpu().numpy())
            written.append(out)
    return written


if __name__ == "__main__":
    main()
