"""Expression code of a clip from tracked 3-D landmarks: a per-frame geometric fit of FLAME's expression and jaw pose, batched
over every frame of every clip in one launch (csrc/expression_fit.hip through `ops.expression_fit`).  The
reference's Step 3 leaves this to a learned encoder whose weights it does not ship; this is NOT that network but a least-squares
fit of the same FLAME parameters the model consumes (`get_coef_dict`: 50 expression numbers, the jaw opening).

The caller arrives with landmarks (F, K, 3) in FLAME's model space -- `align_to_flame` takes tracked landmarks there through the
head-pose fit -- the subject's shape, and the landmark embedding (a face index and barycentric weights per landmark).

    python -m msmd_amd.utils.expression_fit --landmarks L.npy [--valid V.npy] --flame generic_model.pkl --embedding emb.npz \\
           --static static.json --shape shape.npy --out clip_code.pkl [--jaw_dof 1] [--jaw_out jaw.npy] [--report fit.json]

Outside: 2-D landmarks or a camera model; fitting shape, neck, eyes or global pose; per-frame landmark weights; temporal priors
and warm starts (frames are independent); robust losses; the dynamic contour tables; more than 61 expression components.
"""
from __future__ import annotations

import argparse
import json
import pickle as pkl
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops
from .common import clip_list, cut_clips, flatten_clips

JAW = 2                      # FLAME's joints: global, neck, jaw, two eyes


def _embedding(flame, lmk_faces_idx, lmk_bary):
    """-> (vidx (K, 3) int64 vertex indices, bary (K, 3) float64) on the model's device; ValueError for more landmarks than the
    kernel takes or a face index outside the mesh."""
    dev = flame.v_template.device
    fidx = torch.as_tensor(lmk_faces_idx).reshape(-1).to(torch.int64)
    bary = torch.as_tensor(lmk_bary).to(torch.float64).reshape(-1, 3)
    K = fidx.numel()
    if K < 1 or bary.shape[0] != K:
        raise ValueError(f"{K} face indices but {bary.shape[0]} barycentric triples")
    if K > ops.EXPFIT_MAX_LANDMARKS:
        raise ValueError(f"{K} landmarks; the kernel takes up to {ops.EXPFIT_MAX_LANDMARKS}")
    n_faces = flame.faces_tensor.shape[0]
    if int(fidx.min()) < 0 or int(fidx.max()) >= n_faces:
        raise ValueError(f"lmk_faces_idx must lie in [0, {n_faces}), the mesh's faces")
    return flame.faces_tensor.to(torch.int64)[fidx.to(dev)], bary.to(dev)


def reduce_flame(flame, lmk_faces_idx, lmk_bary, shape):
    """The per-landmark reduced model of FLAME with the global, neck and eye rotations at identity, in float64 on the model's
    device: (tab (K, 6, NE + 9), tab0 (S, K, 6)).  With M = R(jaw) - I, landmark k is l_k = X_k + M Y_k where
    [X_k; Y_k] (6) = tab0[s, k] + tab[k] @ [e | vec(M)]:
        X_k = sum_c b_kc s_c x_c,  Y_k = sum_c b_kc w_c,jaw (x_c - J_jaw),  x_c = v_template + S beta + E e + P vec(M)
    over the corners c of the landmark's face (P: rows 9..17 of posedirs; s_c the sum of the vertex's skinning weights, 1 up to
    their fp32 rounding, which the full path carries too).  shape: (100,) or (S, 100); only tab0 depends on it.
    Gathers and small products, built once per (embedding, subject)."""
    vidx, bary = _embedding(flame, lmk_faces_idx, lmk_bary)
    dev = vidx.device
    f64 = lambda t: t.detach().to(torch.float64)
    shape = torch.as_tensor(shape).detach().to(dev).to(torch.float64)
    shape = shape[None] if shape.dim() == 1 else shape
    sd = f64(flame.shapedirs)                                        # (V, 3, n_shape + NE)
    n_shape = shape.shape[1]
    NE = sd.shape[2] - n_shape
    if shape.dim() != 2 or NE < 1:
        raise ValueError(f"shape must be ({n_shape},) or (S, {n_shape}) with fewer columns than the model's {sd.shape[2]} directions")
    if NE > ops.EXPFIT_MAX_EXP:
        raise ValueError(f"the model has {NE} expression components; the kernel takes up to {ops.EXPFIT_MAX_EXP}")
    if flame.J_regressor.shape[0] != 5:
        raise ValueError("the reduced model is written for FLAME's 5-joint tree")
    V, K = sd.shape[0], vidx.shape[0]
    vt, jr, wts = f64(flame.v_template), f64(flame.J_regressor)[JAW], f64(flame.lbs_weights)
    pd = f64(flame.posedirs)[9 * (JAW - 1):9 * JAW].reshape(9, V, 3)
    # one subject at a time, so that a subject's constants do not depend on how many subjects the call has
    v_shaped = torch.stack([vt + sd[:, :, :n_shape] @ b for b in shape])                   # (S, V, 3)
    x0 = v_shaped[:, vidx]                                                                 # (S, K, 3 corners, 3)
    xe = sd[:, :, n_shape:][vidx]                                                          # (K, 3, 3, NE)
    xp = pd[:, vidx].permute(1, 2, 3, 0)                                                   # (K, 3, 3, 9)
    j0 = torch.stack([jr @ v for v in v_shaped])                                           # (S, 3)
    je = torch.einsum("v,vcl->cl", jr, sd[:, :, n_shape:])                                 # (3, NE)
    bs = bary * wts[vidx].sum(-1)                                                          # (K, 3)
    bw = bary * wts[vidx, JAW]
    tab = torch.empty(K, 6, NE + 9, device=dev, dtype=torch.float64)
    tab[:, :3, :NE] = torch.einsum("kc,kcxl->kxl", bs, xe)
    tab[:, :3, NE:] = torch.einsum("kc,kcxl->kxl", bs, xp)
    tab[:, 3:, :NE] = torch.einsum("kc,kcxl->kxl", bw, xe - je[None, None])
    tab[:, 3:, NE:] = torch.einsum("kc,kcxl->kxl", bw, xp)
    tab0 = torch.stack([torch.cat([(bs[..., None] * x).sum(1), (bw[..., None] * (x - j)).sum(1)], 1) for x, j in zip(x0, j0)])
    return tab.contiguous(), tab0.contiguous()


def _weights(weights, K, dev):
    w = np.ones(K, np.float64) if weights is None else \
        np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64).reshape(-1)
    if w.shape != (K,):
        raise ValueError(f"weights must have shape ({K},), got {w.shape}")
    if not np.all(np.isfinite(w)) or w.min() < 0 or w.max() <= 0:
        raise ValueError("weights must be finite, >= 0 and not all zero")
    return torch.from_numpy(w).to(dev)


def _options(jaw_dof, iterations):
    if jaw_dof not in (0, 1, 3):
        raise ValueError(f"jaw_dof must be 0, 1 or 3, got {jaw_dof!r}")
    if not 0 <= int(iterations) <= ops.EXPFIT_MAX_ITERATIONS:
        raise ValueError(f"iterations must be in [0, {ops.EXPFIT_MAX_ITERATIONS}], got {iterations}")


def _shapes(shape, n_clips, single):
    """-> (S, n_shape) tensor and the clip -> subject map; ValueError when several shapes do not match the clips."""
    shape = torch.as_tensor(shape)
    if shape.dim() == 1:
        return shape[None], [0] * n_clips
    if shape.dim() != 2 or shape.shape[0] != n_clips:
        raise ValueError(f"{n_clips} clip{'s' * (n_clips != 1)} but shape has shape {tuple(shape.shape)}: one shape for all, or one per clip")
    return shape, list(range(n_clips))


def fit_expression(landmarks, flame, shape, lmk_faces_idx, lmk_bary, weights=None, jaw_dof=1, lambda_exp=1e-6, lambda_jaw=0.0,
                   iterations=12, return_details=False):
    """FLAME's expression code per frame, (F, NE) fp32 on the device, fitted to landmarks in model space.

    landmarks: one (F, K, 3) fp32 device tensor or a list of them (one K): concatenated once, one kernel launch for the whole
    list; a list comes back as a list.  shape: (100,) for every clip, or (n_clips, 100).  lmk_faces_idx (K) / lmk_bary (K, 3): the
    landmark embedding, K <= ops.EXPFIT_MAX_LANDMARKS.  weights (K) >= 0, not all zero (None: ones), shared by all frames.
    jaw_dof: 0 locks the jaw closed (the 53-wide row of `render_coeffs`), 1 frees the jaw opening (`get_coef_dict`'s 54th
    number), 3 frees the whole jaw rotation.  The fit is Levenberg-Marquardt with exactly `iterations` iterations of fixed
    work from p = 0, in float64 (include/msmd_hip.h states it); a frame's result depends on that frame alone.
    lambda_exp / lambda_jaw: Tikhonov weights on |e|^2 / |theta|^2, lengths in FLAME's metres.  The defaults (1e-6, 0) have
    NOT been tuned on real footage.

    return_details: also a dict (or a list of dicts) with jaw (F, 3) axis-angle, rms (F) = sqrt(sum w |r|^2 / sum w) in metres,
    and status (F) int32: bit 0 a non-finite landmark (the frame's outputs are NaN), bit 1 a refused factorisation.

    ValueError for K above the limit, a face index outside the mesh, negative or all-zero weights, more than
    ops.EXPFIT_MAX_EXP expression components, jaw_dof outside {0, 1, 3}, iterations outside [0, 64], several shapes that do
    not match the clips."""
    clips, single = clip_list(landmarks)
    _options(jaw_dof, iterations)
    shapes, clip_subject = _shapes(shape, len(clips), single)
    vidx, _ = _embedding(flame, lmk_faces_idx, lmk_bary)
    w = _weights(weights, vidx.shape[0], "cpu")
    NE = flame.shapedirs.shape[2] - shapes.shape[1]
    if NE > ops.EXPFIT_MAX_EXP:
        raise ValueError(f"the model has {NE} expression components; the kernel takes up to {ops.EXPFIT_MAX_EXP}")
    ops._need_cuda(*clips)                     # every refusal above speaks before the device is needed
    L, offsets, _ = flatten_clips(clips, (vidx.shape[0], 3))
    dev = L.device
    w = w.to(dev)
    tab, tab0 = reduce_flame(flame, lmk_faces_idx, lmk_bary, shapes)
    subject = np.concatenate([np.full(b - a, s, np.int32) for a, b, s in zip(offsets[:-1], offsets[1:], clip_subject)])
    code, jaw, rms, status = ops.expression_fit(L, torch.from_numpy(subject).to(dev), tab.to(dev), tab0.to(dev), w, jaw_dof,
                                                lambda_exp, lambda_jaw, iterations)
    out = cut_clips(code, offsets)
    if not return_details:
        return out[0] if single else out
    details = [dict(jaw=j, rms=r, status=s) for j, r, s in zip(cut_clips(jaw, offsets), cut_clips(rms, offsets), cut_clips(status, offsets))]
    return (out[0], details[0]) if single else (out, details)


def align_to_flame(landmarks, flame, shape, lmk_faces_idx, lmk_bary, static_idx, valid=None):
    """Tracked landmarks (F, K, 3) (or a list of clips) -> the same landmarks in FLAME's model space, gap-filled: the `aligned`
    output of `head_pose_from_landmarks(..., return_details=True)` with the subject's neutral FLAME landmarks (e = 0, jaw closed)
    as the canonical face and static_idx naming the rigid landmarks.  shape as in `fit_expression`.  No new kernel."""
    from .head_pose import head_pose_from_landmarks
    clips, single = clip_list(landmarks)
    shapes, clip_subject = _shapes(shape, len(clips), single)
    neutral = reduce_flame(flame, lmk_faces_idx, lmk_bary, shapes)[1][:, :, :3].float()
    if shapes.shape[0] == 1:
        _, det = head_pose_from_landmarks(landmarks, neutral[0], static_idx, valid, return_details=True)
        return det["aligned"] if single else [d["aligned"] for d in det]
    valids = [None] * len(clips) if valid is None else list(valid)
    return [head_pose_from_landmarks(c, neutral[s], static_idx, v, return_details=True)[1]["aligned"]
            for c, s, v in zip(clips, clip_subject, valids)]


def save_expression_code(path, code):
    """The expression-code pickle `inference.query_for_motion_coeff` and `utils.assemble` read: a float32 numpy array (F, NE)."""
    a = np.asarray(code.detach().cpu() if torch.is_tensor(code) else code, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f"the expression code must have shape (F, NE), got {a.shape}")
    with open(path, "wb") as f:
        pkl.dump(a, f)


def fit_report(rms, status):
    """What a Step-4-style filter reads: the clip's median and maximum rms over the frames that have one, and the flagged frames."""
    rms, status = np.asarray(rms, np.float64), np.asarray(status)
    ok = np.isfinite(rms)
    return dict(frames=int(rms.size), rms_median=float(np.median(rms[ok])) if ok.any() else None,
                rms_max=float(rms[ok].max()) if ok.any() else None, flagged=int((status != 0).sum()),
                non_finite=int((status & 1 != 0).sum()), refused=int((status & 2 != 0).sum()))


def load_embedding(path):
    """(.npz or a pickled dict in .npy) -> (lmk_faces_idx (K), lmk_bary (K, 3)): the keys `lmk_face_idx` / `lmk_b_coords` of the
    mediapipe -> FLAME embedding, or FLAME's own `full_lmk_faces_idx` / `full_lmk_bary_coords`."""
    d = np.load(path, allow_pickle=True, encoding="latin1")
    d = d[()] if isinstance(d, np.ndarray) else d
    for fk, bk in (("lmk_face_idx", "lmk_b_coords"), ("full_lmk_faces_idx", "full_lmk_bary_coords")):
        if fk in d:
            return np.asarray(d[fk]).reshape(-1).astype(np.int64), np.asarray(d[bk], np.float64).reshape(-1, 3)
    raise ValueError(f"{path} holds neither lmk_face_idx nor full_lmk_faces_idx")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="expression-code pickle of a clip from tracked 3-D face landmarks")
    p.add_argument("--landmarks", required=True, help=".npy, (F, K, 3), the embedding's K landmarks")
    p.add_argument("--valid", default=None, help=".npy, (F) bool: frames the tracker found a face in (default: all)")
    p.add_argument("--flame", required=True, help="FLAME's generic_model.pkl")
    p.add_argument("--embedding", required=True, help="the landmark embedding (.npz / .npy)")
    p.add_argument("--static", required=True, help="JSON list: indices (into the K landmarks) of the rigid ones")
    p.add_argument("--shape", required=True, help=".npy, (100,): the subject's shape")
    p.add_argument("--out", required=True, help="the pickle to write")
    p.add_argument("--jaw_dof", type=int, default=1, choices=(0, 1, 3))
    p.add_argument("--jaw_out", default=None, help=".npy for the jaw axis-angle (F, 3)")
    p.add_argument("--report", default=None, help=".json for the fit's rms and flags")
    p.add_argument("--iterations", type=int, default=12)
    p.add_argument("--device", default="cuda")
    return p.parse_args(argv)


def main(argv=None):
    from .flame import FLAME, FLAMEConfig
    args = parse_args(argv)
    fidx, bary = load_embedding(args.embedding)
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.flame_model_path = args.flame
    with open(args.flame, "rb") as f:
        cfg.asset = dict(pkl.load(f, encoding="latin1"))
    z = lambda *s: np.zeros(s, np.int64)
    cfg.asset["lmk"] = dict(static_lmk_faces_idx=z(51), static_lmk_bary_coords=np.zeros((51, 3), np.float32),
                            dynamic_lmk_faces_idx=z(79, 17), dynamic_lmk_bary_coords=np.zeros((79, 17, 3), np.float32),
                            full_lmk_faces_idx=fidx[None], full_lmk_bary_coords=bary[None].astype(np.float32))
    flame = FLAME(cfg).to(args.device)
    L = torch.from_numpy(np.load(args.landmarks).astype(np.float32)).to(args.device)
    valid = None if args.valid is None else np.load(args.valid).astype(bool)
    shape = np.load(args.shape).astype(np.float64).reshape(-1)
    with open(args.static) as f:
        static_idx = np.asarray(json.load(f), np.int32)
    aligned = align_to_flame(L, flame, shape, fidx, bary, static_idx, valid)
    code, det = fit_expression(aligned, flame, shape, fidx, bary, jaw_dof=args.jaw_dof, iterations=args.iterations,
                               return_details=True)
    save_expression_code(args.out, code)
    if args.jaw_out:
        np.save(args.jaw_out, det["jaw"].cpu().numpy())
    report = fit_report(det["rms"].cpu().numpy(), det["status"].cpu().numpy())
    if args.report:
        with open(args.report, "w") as f:
            json.dump(report, f, indent=1)
    print(f"wrote {args.out}: {tuple(code.shape)} expression code; rms median {report['rms_median']}, max {report['rms_max']}, "
          f"{report['flagged']} flagged frames")


if __name__ == "__main__":
    main()
