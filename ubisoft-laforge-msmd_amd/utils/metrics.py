"""Vertex-space evaluation on the FLAME mesh: how close a generated clip is to the ground-truth motion for the same audio
(csrc/vertex_metrics.hip through ops.vertex_frame_errors / ops.vertex_motion_moments_).

Definitions, for a clip of F frames of V vertices, p = prediction, g = ground truth, d2[f, v] = |p[f, v] - g[f, v]|^2:

  lve     lip vertex error (Richard et al. 2021, MeshTalk; as computed by CodeTalker's cal_metric.py):
              mean_f max_{v in lips} d2[f, v]
  fdd     upper-face dynamics deviation (Xing et al. 2023, CodeTalker, eq. 13 / cal_metric.py): with m_x[f, v] = |x[f, v] -
          template[v]|^2, the squared displacement from the neutral mesh, and std_f the population standard deviation over time,
              mean_{v in upper} std_f m_g[., v]  -  mean_{v in upper} std_f m_p[., v]
          (ground truth minus prediction; 0 for a clip of one frame)
  mve     mean vertex error:     sum_{f, v} sqrt(d2) / (F V)
  max_ve  maximum vertex error:  max_{f, v} sqrt(d2)
  rmse    sqrt(sum_{f, v} d2 / (F V))

The device reduces every frame to four float64 numbers and every (clip, upper vertex) to Welford moments of m; `result()` copies
both to the host and reduces EACH CLIP OVER ITS OWN SLICE in float64 (math.fsum, numpy's NaN-propagating max), so a clip's numbers
do not depend on the other clips of the batch, nor on how the frames were cut into `update` calls.  A NaN vertex makes the
numbers it contributes to NaN; nothing drops it.

Command line:  python -m msmd_amd.utils.metrics --pred_exp P.pkl --pred_rot P_rot.pkl --gt_exp G.pkl --gt_rot G_rot.pkl
                   --regions masks.pkl --out metrics.json [--flame_model_path ... --flame_lmk_embedding_path ...]
The four pickles are the (T, 50) expression codes and (T, 3) head rotations `inference.py` writes and `utils/assemble.py` reads."""
from __future__ import annotations

import math
import pickle as pkl

import numpy as np
import torch

from .. import ops
from .common import get_coef_dict

LIP_BIT, UPPER_BIT = 1, 2     # the region byte of include/msmd_hip.h


def _index_list(name, idx, V):
    a = np.asarray(idx)
    if a.size == 0:
        raise ValueError(f"{name} is empty")
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be a flat list of integers, got shape {a.shape} of {a.dtype}")
    a = np.sort(a.astype(np.int64))
    if a[0] < 0 or a[-1] >= V:
        raise ValueError(f"{name} holds an index outside [0, {V}): {int(a[0] if a[0] < 0 else a[-1])}")
    if (a[1:] == a[:-1]).any():
        raise ValueError(f"{name} holds a duplicate: {int(a[1:][a[1:] == a[:-1]][0])}")
    return a


def regions(V, lips, upper, device="cuda"):
    """Host index lists -> (region (V) uint8 with LIP_BIT / UPPER_BIT set, upper_idx (U) int32 ascending), both on `device`.
    ValueError for an empty list, an index outside [0, V) or a duplicate."""
    V = int(V)
    if V < 1:
        raise ValueError(f"V = {V} must be at least 1")
    lip, up = _index_list("lips", lips, V), _index_list("upper", upper, V)
    region = np.zeros(V, np.uint8)
    region[lip] |= LIP_BIT
    region[up] |= UPPER_BIT
    return torch.from_numpy(region).to(device), torch.from_numpy(up.astype(np.int32)).to(device)


def _clip_numbers(table, state, V):
    """One clip: its (F, 4) rows of the frame table and its (U, 2, 3) moments, float64 numpy -> the metrics."""
    F = table.shape[0]
    count = state[:, :, 0]
    if (count != F).any():
        raise RuntimeError(f"a clip of {F} frames holds moments of {count.min():.0f} .. {count.max():.0f} frames")
    std = np.sqrt(state[:, :, 2] / F)                                  # (U, 2): population std of m, pred | gt
    U = std.shape[0]
    return dict(lve=math.fsum(table[:, 0]) / F, mve=math.fsum(table[:, 1]) / (F * V), max_ve=float(np.max(table[:, 2])),
                rmse=math.sqrt(math.fsum(table[:, 3]) / (F * V)), fdd=math.fsum(std[:, 1]) / U - math.fsum(std[:, 0]) / U, frames=F)


def reduce_clips(table, state, offsets, V):
    """The host half of `VertexMetrics.result`: table (n, 4) and state (n_clips, U, 2, 3) float64 numpy -> {'clips': [per-clip
    dict], 'all': pooled dict}.  Pooled: lve / mve / rmse over all frames (frame-weighted), max_ve the maximum, fdd the mean of the
    clips'."""
    clips = [_clip_numbers(table[a:b], state[k], V) for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:]))]
    n = offsets[-1]
    pooled = dict(lve=math.fsum(table[:, 0]) / n, mve=math.fsum(table[:, 1]) / (n * V), max_ve=float(np.max(table[:, 2])),
                  rmse=math.sqrt(math.fsum(table[:, 3]) / (n * V)), fdd=math.fsum(c["fdd"] for c in clips) / len(clips), frames=n)
    return {"clips": clips, "all": pooled}


class VertexMetrics:
    """Streaming vertex-space metrics of a ragged batch of clips laid end to end.  clip_offsets: the (n_clips + 1) HOST offsets,
    ascending from 0; V vertices; lips / upper: host index lists (`regions`); template (V, 3), or (n_clips, V, 3) for a neutral
    mesh per clip: the mesh `fdd`'s displacement is measured from.  `update(pred, gt)` takes the next frames of the sequence, any
    number at a time; `result()` needs every frame seen."""

    def __init__(self, clip_offsets, V, lips, upper, template, device="cuda"):
        off = [int(o) for o in clip_offsets]
        self.offsets = ops._clip_offsets("clip_offsets", off, off[-1] if off else 0)
        self.V, self.device = int(V), torch.device(device)
        self.region, self.upper_idx = regions(V, lips, upper, self.device)
        n_clips = len(self.offsets) - 1
        template = torch.as_tensor(template, dtype=torch.float32).to(self.device).contiguous()
        if tuple(template.shape) not in ((self.V, 3), (n_clips, self.V, 3)):
            raise ValueError(f"template must have shape ({self.V}, 3) or ({n_clips}, {self.V}, 3), got {tuple(template.shape)}")
        self.template = template
        self.offsets_dev = torch.tensor(self.offsets, dtype=torch.int64).to(self.device)
        self.state = torch.zeros(n_clips, self.upper_idx.numel(), 2, 3, device=self.device, dtype=torch.float64)
        self.tables, self.seen = [], 0

    def update(self, pred, gt):
        """The next pred.shape[0] frames, (n, V, 3) contiguous on the device, both fp32 or both fp16.  ValueError past the end."""
        if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dtype != gt.dtype:
            raise TypeError(f"pred and gt must be tensors of one dtype, got {getattr(pred, 'dtype', None)} and {getattr(gt, 'dtype', None)}")
        n = pred.shape[0] if pred.dim() == 3 else -1
        if n < 0 or tuple(pred.shape) != (n, self.V, 3) or pred.shape != gt.shape:
            raise ValueError(f"pred and gt must both be (n, {self.V}, 3), got {tuple(pred.shape)} and {tuple(gt.shape)}")
        if self.seen + n > self.offsets[-1]:
            raise ValueError(f"{self.seen} frames seen and {n} more given: the sequence has {self.offsets[-1]}")
        if n == 0:
            return self
        self.tables.append(ops.vertex_frame_errors(pred, gt, self.region))
        ops.vertex_motion_moments_(self.state, pred, gt, self.seen, self.offsets_dev, self.upper_idx, self.template)
        self.seen += n
        return self

    def result(self):
        """{'clips': [{'lve', 'mve', 'max_ve', 'rmse', 'fdd', 'frames'} per clip], 'all': the pooled values}; ValueError unless every
        frame has been seen."""
        if self.seen != self.offsets[-1]:
            raise ValueError(f"{self.seen} of {self.offsets[-1]} frames seen")
        table = torch.cat(self.tables, 0).cpu().numpy()
        return reduce_clips(table, self.state.cpu().numpy(), self.offsets, self.V)


def vertex_metrics(pred, gt, clip_offsets, lips, upper, template):
    """One call: pred, gt (n, V, 3) on the device, clip_offsets from 0 to n -> `VertexMetrics.result()`."""
    if not torch.is_tensor(pred) or pred.dim() != 3:
        raise ValueError("pred must be an (n, V, 3) tensor")
    off = ops._clip_offsets("clip_offsets", clip_offsets, pred.shape[0])
    return VertexMetrics(off, pred.shape[1], lips, upper, template, pred.device).update(pred, gt).result()


def _track(coef):
    """(T, 54) get_coef_dict rows from (T, 54) or (T, 53) (expression + head rotation: the jaw is closed), (1, T, C) taken too."""
    coef = coef.reshape(-1, coef.shape[-1]).float()
    if coef.shape[-1] == 53:
        coef = torch.cat([coef, torch.zeros_like(coef[:, :1])], dim=-1)
    if coef.shape[-1] != 54:
        raise ValueError(f"a coefficient track is 53 or 54 wide, got {coef.shape[-1]}")
    return coef


def _vertices(coef, shape, flame, coef_stats, with_global_pose):
    c = get_coef_dict(coef, shape, coef_stats, with_global_pose=with_global_pose)
    return flame(c["shape"], c["exp"], c["pose"], return_lm2d=False, return_lm3d=False)[0].float().contiguous()


@torch.no_grad()
def evaluate_coeffs(pred_coef, gt_coef, shape_coef, flame, coef_stats, clip_offsets, lips, upper, chunk=512, with_global_pose=False):
    """Two coefficient tracks (T, 54 | 53) in get_coef_dict's layout, the clips of `clip_offsets` end to end -> the vertex metrics.
    Both run through get_coef_dict / FLAME `chunk` frames at a time and each pair of chunks goes to `VertexMetrics.update`: two
    chunks of vertices are alive at a time.  shape_coef (1, 100), or (n_clips, 100) for a shape per clip; coef_stats: None for
    coefficients in the data's units, or get_coef_dict's denorm_stats.  The template is FLAME at the clip's shape with zero
    expression and pose.  Head rotation is ignored unless with_global_pose, as the published protocols do."""
    pred, gt = _track(pred_coef), _track(gt_coef)
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError(f"the two tracks differ: {tuple(pred.shape)} on {pred.device} and {tuple(gt.shape)} on {gt.device}")
    T = pred.shape[0]
    off = ops._clip_offsets("clip_offsets", clip_offsets, T)
    n_clips = len(off) - 1
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk = {chunk} must be at least 1")
    shape = shape_coef.reshape(-1, shape_coef.shape[-1]).float().to(pred.device)
    if shape.shape[0] not in (1, n_clips):
        raise ValueError(f"shape_coef holds {shape.shape[0]} shapes for {n_clips} clips")
    # every FLAME call below holds ONE shape (FLAME's one-subject path): with a shape per clip the chunks stop at the clip's end, so
    # a clip's vertices do not depend on its neighbours' shapes nor on `chunk`
    one = shape.shape[0] == 1
    spans = [(0, T, 0)] if one else [(a, b, k) for k, (a, b) in enumerate(zip(off[:-1], off[1:]))]
    rest = get_coef_dict(torch.zeros(shape.shape[0], 54, device=pred.device), shape, coef_stats, with_global_pose=False)
    template = torch.cat([flame(rest["shape"][k:k + 1].contiguous(), torch.zeros_like(rest["exp"][:1]), torch.zeros_like(rest["pose"][:1]),
                                return_lm2d=False, return_lm3d=False)[0].float() for k in range(shape.shape[0])], 0)
    template = template[0].contiguous() if one else template.contiguous()
    vm = VertexMetrics(off, template.shape[-2], lips, upper, template, pred.device)
    for a, b, k in spans:
        for i in range(a, b, chunk):
            j = min(i + chunk, b)
            s = shape[k:k + 1].expand(j - i, -1)
            vm.update(_vertices(pred[i:j], s, flame, coef_stats, with_global_pose), _vertices(gt[i:j], s, flame, coef_stats, with_global_pose))
    return vm.result()


# ----------------------------------------------------------------------------- command line
def load_regions(path):
    """--regions FILE -> (lips, upper) int64 arrays.  An `.npz` or a pickle with `lips` and `upper`; a FLAME_masks-style pickle
    without `upper` gives the union of its `forehead` and `eye_region`."""
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
    else:
        with open(path, "rb") as f:
            d = dict(pkl.load(f, encoding="latin1"))
    if "lips" not in d:
        raise ValueError(f"{path} has no `lips`: it holds {sorted(d)}")
    if "upper" in d:
        upper = np.asarray(d["upper"])
    elif "forehead" in d and "eye_region" in d:
        upper = np.union1d(np.asarray(d["forehead"]), np.asarray(d["eye_region"]))
    else:
        raise ValueError(f"{path} has neither `upper` nor `forehead` and `eye_region`: it holds {sorted(d)}")
    return np.asarray(d["lips"]).astype(np.int64).ravel(), upper.astype(np.int64).ravel()


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(description="Vertex-space metrics (LVE, FDD, mean / max / RMS vertex error) of a generated clip "
                                             "against the ground truth, on the MI355X.")
    for name in ("pred_exp", "pred_rot", "gt_exp", "gt_rot"):
        ap.add_argument("--" + name, type=str, required=True, help="pickle of a (T, 50) expression code / (T, 3) head rotation")
    ap.add_argument("--regions", type=str, required=True, help=".npz or pickle with `lips` and `upper` vertex indices "
                                                               "(FLAME_masks.pkl: `upper` = forehead + eye_region)")
    ap.add_argument("--out", type=str, default="metrics.json")
    ap.add_argument("--coef_dict_path", type=str, default=None, help="coefficient statistics (with --normalised)")
    ap.add_argument("--normalised", action="store_true", help="the pickles hold normalised coefficients: de-normalise them with "
                                                              "--coef_dict_path (inference.py writes them in the data's units)")
    ap.add_argument("--flame_model_path", type=str, default=None, help="FLAME generic_model.pkl")
    ap.add_argument("--flame_lmk_embedding_path", type=str, default=None, help="FLAME landmark embedding")
    ap.add_argument("--with_global_pose", action="store_true", help="keep the head rotation (default: compared with the head still)")
    ap.add_argument("--chunk", type=int, default=512, help="frames decoded by FLAME at a time")
    return ap


def parse_args(argv=None):
    """build_parser().parse_args with the checks that span flags: --normalised needs --coef_dict_path and the other way round,
    and --chunk is at least 1."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.normalised and args.coef_dict_path is None:
        ap.error("--normalised needs --coef_dict_path: there are no statistics to de-normalise with")
    if args.coef_dict_path is not None and not args.normalised:
        ap.error("--coef_dict_path is read only with --normalised: coefficients in the data's units need no statistics")
    if args.chunk < 1:
        ap.error(f"--chunk {args.chunk} must be at least 1")
    return args


def _load_track(exp_path, rot_path):
    with open(exp_path, "rb") as f:
        e = np.asarray(pkl.load(f), dtype=np.float32)
    with open(rot_path, "rb") as f:
        r = np.asarray(pkl.load(f), dtype=np.float32)
    e, r = e.reshape(-1, e.shape[-1]), r.reshape(-1, r.shape[-1])
    if e.shape[0] != r.shape[0] or e.shape[1] != 50 or r.shape[1] != 3:
        raise ValueError(f"{exp_path} holds {e.shape} and {rot_path} holds {r.shape}: a track is (T, 50) and (T, 3)")
    return torch.from_numpy(np.concatenate([e, r], 1))


def main(argv=None):
    """One clip: the two tracks -> FLAME -> the metrics, printed and written to --out as JSON ({'clips': [...], 'all': {...}})."""
    import json
    from types import SimpleNamespace
    from .flame import FLAME, FLAMEConfig
    args = parse_args(argv)
    device = torch.device("cuda")
    pred, gt = _load_track(args.pred_exp, args.pred_rot).to(device), _load_track(args.gt_exp, args.gt_rot).to(device)
    if pred.shape != gt.shape:
        raise ValueError(f"the prediction has {pred.shape[0]} frames and the ground truth {gt.shape[0]}")
    lips, upper = load_regions(args.regions)
    coef_stats = None
    if args.normalised:
        with open(args.coef_dict_path, "rb") as f:
            coef_stats = {k: torch.as_tensor(v).to(device) for k, v in pkl.load(f).items()}
        coef_stats.setdefault("shape_mean", torch.zeros(100, device=device))     # the zero shape below is then the mean shape
        coef_stats.setdefault("shape_std", torch.ones(100, device=device))
    cfg = SimpleNamespace(**{k: v for k, v in vars(FLAMEConfig).items() if not k.startswith("__")})
    if args.flame_model_path is not None:
        cfg.flame_model_path = args.flame_model_path
    if args.flame_lmk_embedding_path is not None:
        cfg.flame_lmk_embedding_path = args.flame_lmk_embedding_path
    flame = FLAME(cfg).to(device)
    res = evaluate_coeffs(pred, gt, torch.zeros(1, 100, device=device), flame, coef_stats, [0, pred.shape[0]], lips, upper,
                          chunk=args.chunk, with_global_pose=args.with_global_pose)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["all"]))
    return res


if __name__ == "__main__":
    main()
