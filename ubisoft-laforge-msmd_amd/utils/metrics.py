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

Seeing the error: `VertexErrorMap` keeps the per-vertex distance summed over each clip's frames, `colormap_table`
and ops.vertex_error_colors / ops.colormap turn a distance into a colour, and `render_comparison` draws ground truth | prediction |
error heat map side by side through `MeshRenderer.render_vertices(vertex_colors=, lit=False)`.

Command line:  python -m msmd_amd.utils.metrics --pred_exp P.pkl --pred_rot P_rot.pkl --gt_exp G.pkl --gt_rot G_rot.pkl
                   --regions masks.pkl --out metrics.json [--flame_model_path ... --flame_lmk_embedding_path ...]
                   [--comparison_video OUT.avi --error_map OUT.jpg --error_max METRES --colormap jet --legend_labels --render_size 256
                    --render_samples 1 --fps 25 --audio A.wav --video_quality 90]
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


# ----------------------------------------------------------------------------- seeing the error
# stops of the named colour tables, (position in [0, 1], (R, G, B)): piecewise linear between them
COLORMAPS = {
    "jet": [(0.0, (0, 0, 255)), (0.25, (0, 255, 255)), (0.5, (0, 255, 0)), (0.75, (255, 255, 0)), (1.0, (255, 0, 0))],
    "heat": [(0.0, (0, 0, 0)), (1.0 / 3.0, (255, 0, 0)), (2.0 / 3.0, (255, 255, 0)), (1.0, (255, 255, 255))],
    "gray": [(0.0, (0, 0, 0)), (1.0, (255, 255, 255))],
}
NAN_COLOR = (255, 0, 255)


def colormap_table(name):
    """-> (256, 4) uint8 RGBA on the host, alpha 255.  A name of COLORMAPS ("jet": blue - cyan - green - yellow - red; "heat": black -
    red - yellow - white; "gray") is interpolated piecewise linearly between its stops, row i at i / 255, rounded half up; a (256,
    3 | 4) uint8 array (or tensor) is taken as it is, three channels padded with alpha 255."""
    if isinstance(name, str):
        if name not in COLORMAPS:
            raise ValueError(f"colormap {name!r} is not one of {sorted(COLORMAPS)}")
        pos = np.array([p for p, _ in COLORMAPS[name]], np.float64)
        stops = np.array([c for _, c in COLORMAPS[name]], np.float64)
        x = np.arange(256, dtype=np.float64) / 255.0
        rgb = np.stack([np.interp(x, pos, stops[:, c]) for c in range(3)], axis=1)
        table = np.full((256, 4), 255, np.uint8)
        table[:, :3] = np.floor(rgb + 0.5).astype(np.uint8)
        return table
    a = name.detach().cpu().numpy() if torch.is_tensor(name) else np.asarray(name)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] != 256 or a.shape[1] not in (3, 4):
        raise ValueError(f"a colour table is a name of {sorted(COLORMAPS)} or a (256, 3 | 4) uint8 array, got {a.dtype} {a.shape}")
    table = np.full((256, 4), 255, np.uint8)
    table[:, :a.shape[1]] = a
    return table


def _table_on(table, device):
    return torch.from_numpy(colormap_table(table)).to(device)


class VertexErrorMap:
    """Streaming per-vertex mean distance of a ragged batch of clips laid end to end, `VertexMetrics`'s way: `update(pred, gt)` takes
    the next frames, any number at a time; `result()` -> (n_clips, V) float64 on the device, the sum of |pred - gt| over each clip's
    frames (ops.vertex_error_sums_: the same bits however the frames were cut) divided by the clip's frame count."""

    def __init__(self, clip_offsets, V, device="cuda"):
        off = [int(o) for o in clip_offsets]
        self.offsets = ops._clip_offsets("clip_offsets", off, off[-1] if off else 0)
        self.V, self.device = int(V), torch.device(device)
        self.offsets_dev = torch.tensor(self.offsets, dtype=torch.int64).to(self.device)
        self.state = torch.zeros(len(self.offsets) - 1, self.V, device=self.device, dtype=torch.float64)
        self.seen = 0

    def update(self, pred, gt):
        n = pred.shape[0] if torch.is_tensor(pred) and pred.dim() == 3 else -1
        if n < 0 or tuple(pred.shape) != (n, self.V, 3):
            raise ValueError(f"pred and gt must both be (n, {self.V}, 3), got {tuple(getattr(pred, 'shape', ()))}")
        if self.seen + n > self.offsets[-1]:
            raise ValueError(f"{self.seen} frames seen and {n} more given: the sequence has {self.offsets[-1]}")
        if n == 0:
            return self
        ops.vertex_error_sums_(self.state, pred, gt, self.seen, self.offsets_dev)
        self.seen += n
        return self

    def result(self):
        if self.seen != self.offsets[-1]:
            raise ValueError(f"{self.seen} of {self.offsets[-1]} frames seen")
        frames = torch.tensor(np.diff(np.asarray(self.offsets, np.int64)), dtype=torch.float64).to(self.device)
        return self.state / frames[:, None]


def vertex_error_map(pred, gt, clip_offsets):
    """One call: pred, gt (n, V, 3) on the device, clip_offsets from 0 to n -> `VertexErrorMap.result()`."""
    if not torch.is_tensor(pred) or pred.dim() != 3:
        raise ValueError("pred must be an (n, V, 3) tensor")
    off = ops._clip_offsets("clip_offsets", clip_offsets, pred.shape[0])
    return VertexErrorMap(off, pred.shape[1], pred.device).update(pred, gt).result()


def paint_legend(frames, table):
    """The colour bar of a heat map, in place on frames (n, H, W, 3) uint8: the max(4, W // 32) rightmost columns, row i showing row
    255 - (i * 256) // H of the table (its top is the top of the scale).  No text: the scale's maximum travels beside the picture."""
    n, H, W, _ = frames.shape
    lut = table if torch.is_tensor(table) else _table_on(table, frames.device)
    rows = 255 - (torch.arange(H, device=frames.device) * 256) // H
    frames[:, :, W - max(4, W // 32):, :] = lut[rows, :3][None, :, None, :]
    return frames


def legend_label_layout(H, W, labels):
    """Where `paint_legend_labels` prints labels = (bottom, top) on an (H, W) panel -> [(text, (x, y), scale)] with (x, y) the
    bottom-left pixel of the line as `Overlay.text` takes it: right-aligned two pixels left of `paint_legend`'s bar, the top
    label's ink from row 2 down, the bottom label's down to row H - 3; a font pixel is max(1, H // 128) pixels."""
    from .overlay import FONT_ADVANCE, FONT_ROWS
    try:
        bottom, top = (str(s) for s in labels)
    except (TypeError, ValueError):
        raise ValueError(f"legend_labels must be (bottom, top) strings, got {labels!r}") from None
    scale = max(1, H // 128)
    right = W - max(4, W // 32) - 2                             # the first column the labels leave free
    x = lambda s: right - (FONT_ADVANCE * len(s) - 1) * scale
    return [(top, (x(top), 2 + FONT_ROWS * scale - 1), scale), (bottom, (x(bottom), H - 3), scale)]


def legend_label_boxes(H, W, labels):
    """The pixels the labels may touch -> [(x0, y0, x1, y1)], ends excluded, clipped to the panel."""
    from .overlay import FONT_ADVANCE, FONT_ROWS
    return [(max(x, 0), max(y - FONT_ROWS * scale + 1, 0), min(x + (FONT_ADVANCE * len(s) - 1) * scale, W), min(y + 1, H))
            for s, (x, y), scale in legend_label_layout(H, W, labels)]


def paint_legend_labels(frames, labels, colour=(0, 0, 0)):
    """The ends of the scale in words, in place on frames (n, H, W, 3) uint8 on the device: labels = (bottom, top) in `colour` at
    `legend_label_layout`'s places, the same on every frame, drawn by ops.draw_overlay."""
    from .overlay import Overlay
    n, H, W, _ = frames.shape
    ov = Overlay(n)
    for s, at, scale in legend_label_layout(H, W, labels):
        ov.text([s] * n, np.tile(np.asarray(at, np.float64), (n, 1)), colour, scale=scale)
    return ov.draw(frames)


PANELS = ("gt", "pred", "error")


@torch.no_grad()
def render_comparison(pred, gt, faces, renderer, vmax, table="jet", panels=PANELS, legend=True, t_center=None, rot=None,
                      legend_labels=None):
    """pred, gt (n, V, 3) on the device, both fp32 or both fp16 -> (n, H, len(panels) * W, 3) uint8 on the device, the panels side by
    side: "gt" and "pred" the plain render of each track, "error" the prediction's geometry drawn UNLIT in the colours
    ops.vertex_error_colors gives its vertices (distance / vmax through `table`: a name of COLORMAPS or a (256, 3 | 4) uint8
    array), with the colour bar of `paint_legend` at its right edge if `legend`, and with legend_labels = (bottom, top) strings
    printed left of the bar's two ends, black on the renderer's white background and white on its black one (`paint_legend_labels`; None: no text, the bytes of the bar alone).  t_center, rot as
    `renderer.render_vertices` takes them."""
    panels = tuple(panels)
    if not panels or any(p not in PANELS for p in panels):
        raise ValueError(f"panels must be taken from {PANELS}, got {panels!r}")
    lut = _table_on(table, pred.device)
    out = []
    for p in panels:
        if p == "error":
            colours = ops.vertex_error_colors(pred.contiguous(), gt.contiguous(), vmax, lut, NAN_COLOR)
            frames = renderer.render_vertices(pred, faces, t_center=t_center, rot=rot, vertex_colors=colours, lit=False)[0]
            if legend:
                frames = paint_legend(frames.contiguous(), lut)
                if legend_labels is not None:
                    dark = sum(getattr(renderer, "bg_color", (255, 255, 255))) < 384       # white ink on a dark background
                    frames = paint_legend_labels(frames, legend_labels, (255, 255, 255) if dark else (0, 0, 0))
        else:
            frames = renderer.render_vertices(gt if p == "gt" else pred, faces, t_center=t_center, rot=rot)[0]
        out.append(frames)
    return torch.cat(out, dim=2)


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


def _chunk_pairs(pred, gt, a, b, shape_row, chunk, flame, coef_stats, with_global_pose):
    """The frames [a, b) of two (T, 54) tracks under one shape (1, 100), `chunk` at a time -> (pred vertices, gt vertices, i, j)."""
    for i in range(a, b, chunk):
        j = min(i + chunk, b)
        s = shape_row.expand(j - i, -1)
        yield _vertices(pred[i:j], s, flame, coef_stats, with_global_pose), _vertices(gt[i:j], s, flame, coef_stats, with_global_pose), i, j


def _template(shape, flame, coef_stats):
    """FLAME at every row of shape (S, 100) with zero expression and pose -> (S, V, 3) fp32: the neutral meshes."""
    rest = get_coef_dict(torch.zeros(shape.shape[0], 54, device=shape.device), shape, coef_stats, with_global_pose=False)
    return torch.cat([flame(rest["shape"][k:k + 1].contiguous(), torch.zeros_like(rest["exp"][:1]), torch.zeros_like(rest["pose"][:1]),
                            return_lm2d=False, return_lm3d=False)[0].float() for k in range(shape.shape[0])], 0)


@torch.no_grad()
def evaluate_coeffs(pred_coef, gt_coef, shape_coef, flame, coef_stats, clip_offsets, lips, upper, chunk=512, with_global_pose=False,
                    on_chunk=None):
    """Two coefficient tracks (T, 54 | 53) in get_coef_dict's layout, the clips of `clip_offsets` end to end -> the vertex metrics.
    Both run through get_coef_dict / FLAME `chunk` frames at a time and each pair of chunks goes to `VertexMetrics.update`: two
    chunks of vertices are alive at a time.  shape_coef (1, 100), or (n_clips, 100) for a shape per clip; coef_stats: None for
    coefficients in the data's units, or get_coef_dict's denorm_stats.  The template is FLAME at the clip's shape with zero
    expression and pose.  Head rotation is ignored unless with_global_pose, as the published protocols do.
    on_chunk(pred_vertices, gt_vertices, i, j), when given, is called once per pair of chunks, the frames [i, j) of the tracks,
    after the metrics have seen it (a heat map or a comparison video rides on the same pass: DESIGN.md 5.30)."""
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
    template = _template(shape, flame, coef_stats)
    template = template[0].contiguous() if one else template.contiguous()
    vm = VertexMetrics(off, template.shape[-2], lips, upper, template, pred.device)
    for a, b, k in spans:
        for pv, gv, i, j in _chunk_pairs(pred, gt, a, b, shape[k:k + 1], chunk, flame, coef_stats, with_global_pose):
            vm.update(pv, gv)
            if on_chunk is not None:
                on_chunk(pv, gv, i, j)
            del pv, gv                               # before the next pair is built: two chunks of vertices alive, not four
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
    # seeing the error
    ap.add_argument("--comparison_video", type=str, default=None, metavar="OUT.avi",
                    help="Motion-JPEG AVI of ground truth | prediction | error heat map, side by side")
    ap.add_argument("--error_map", type=str, default=None, metavar="OUT.jpg",
                    help="JPEG of the neutral template coloured by the per-vertex error averaged over the clip")
    ap.add_argument("--error_max", type=float, default=None, metavar="METRES",
                    help="the error drawn in the top colour (default: the clip's max_ve for the video, which costs a second pass "
                         "over the chunks, and the map's own maximum for the still)")
    ap.add_argument("--colormap", type=str, default="jet", choices=sorted(COLORMAPS))
    ap.add_argument("--legend_labels", action="store_true", help="print the ends of the scale, 0 and the maximum in mm, beside the "
                                                                 "colour bar of --comparison_video")
    ap.add_argument("--render_size", type=int, default=None, help="side of a panel in pixels (default 256)")
    ap.add_argument("--render_samples", type=int, default=1, choices=ops.RENDER_SAMPLES, help="samples per pixel")
    ap.add_argument("--fps", type=float, default=None, help="frame rate of the video (default 25)")
    ap.add_argument("--audio", type=str, default=None, metavar="WAV", help="sound track of the video")
    ap.add_argument("--video_quality", type=int, default=90, help="JPEG quality of the video's frames and of the still, 1 .. 100")
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
    if args.comparison_video is None and args.error_map is None:
        for flag in ("render_size", "error_max"):
            if getattr(args, flag) is not None:
                ap.error(f"--{flag} is read only with --comparison_video or --error_map: nothing would be drawn")
    if args.comparison_video is None:
        for flag in ("fps", "audio"):
            if getattr(args, flag) is not None:
                ap.error(f"--{flag} is read only with --comparison_video")
        if args.legend_labels:
            ap.error("--legend_labels is read only with --comparison_video")
    if args.error_max is not None and not 0.0 < args.error_max < float("inf"):
        ap.error(f"--error_max {args.error_max} must be finite and greater than 0")
    if args.render_size is not None and not 1 <= args.render_size <= 16384:
        ap.error(f"--render_size {args.render_size} is outside [1, 16384]")
    if args.fps is not None and not 0.0 < args.fps < float("inf"):
        ap.error(f"--fps {args.fps} must be finite and greater than 0")
    if not 1 <= args.video_quality <= 100:
        ap.error(f"--video_quality {args.video_quality} is outside [1, 100]")
    args.render_size = 256 if args.render_size is None else args.render_size
    args.fps = 25.0 if args.fps is None else args.fps
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


def _scale_or_one(x):
    """A data-derived top of the colour scale: x where it is finite and > 0, else 1.0 (two identical tracks: every colour is row 0)."""
    x = float(x)
    return x if 0.0 < x < float("inf") else 1.0


class _Drawing:
    """What --comparison_video and --error_map hang on the chunk pairs of the metrics pass: at most one chunk of frames is alive, and
    what is kept between chunks is the JPEG files on the host and the (1, V) error sums on the device."""

    def __init__(self, args, flame, T):
        from .renderer import MeshRenderer
        self.args, self.faces, self.T = args, flame.faces_tensor, T
        self.renderer = MeshRenderer((args.render_size, args.render_size), samples=args.render_samples)
        self.want_video, self.want_map = args.comparison_video is not None, args.error_map is not None
        self.video_max = args.error_max
        self.video_pending = self.want_video and self.video_max is None
        self.jpegs, self.sums = [], None

    def video_chunk(self, pv, gv):
        from . import media
        labels = ("0", f"{self.video_max * 1000:.1f} mm") if self.args.legend_labels else None
        frames = render_comparison(pv, gv, self.faces, self.renderer, self.video_max, self.args.colormap, legend_labels=labels)
        self.jpegs += media.encode_jpeg(frames, self.args.video_quality)

    def on_chunk(self, pv, gv, i, j):
        if self.want_map:
            if self.sums is None:
                self.sums = VertexErrorMap([0, self.T], pv.shape[1], pv.device)
            self.sums.update(pv, gv)
        if self.want_video and not self.video_pending:
            self.video_chunk(pv, gv)

    def finish(self, template):
        """Writes the files -> what goes into the JSON beside the metrics."""
        from . import media
        args = self.args
        out = {"colormap": args.colormap}
        if self.want_video:
            audio = None
            if args.audio is not None:
                from .audio import read_wav
                audio = read_wav(args.audio)
            media.write_avi(args.comparison_video, self.jpegs, args.fps, (len(PANELS) * args.render_size, args.render_size), audio)
            out["error_max_video"] = self.video_max
        if self.want_map:
            mean = self.sums.result()[0].contiguous()                     # (V) float64: the clip's time-mean distance
            top = args.error_max if args.error_max is not None else _scale_or_one(mean.max())
            lut = _table_on(args.colormap, mean.device)
            colours = ops.colormap(mean, top, lut, NAN_COLOR)
            still = self.renderer.render_vertices(template[:1].contiguous(), self.faces, vertex_colors=colours, lit=False)[0]
            with open(args.error_map, "wb") as f:
                f.write(media.encode_jpeg(paint_legend(still.contiguous(), lut), args.video_quality)[0])
            out["error_max_map"] = top
        return out


def main(argv=None):
    """One clip: the two tracks -> FLAME -> the metrics, printed and written to --out as JSON ({'clips': [...], 'all': {...}}; with
    --comparison_video / --error_map also 'colormap' and the scale maxima 'error_max_video' / 'error_max_map', in metres)."""
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
    shape = torch.zeros(1, 100, device=device)
    T = pred.shape[0]
    draw = _Drawing(args, flame, T) if args.comparison_video is not None or args.error_map is not None else None
    res = evaluate_coeffs(pred, gt, shape, flame, coef_stats, [0, T], lips, upper, chunk=args.chunk,
                          with_global_pose=args.with_global_pose, on_chunk=None if draw is None else draw.on_chunk)
    if draw is not None:
        if draw.video_pending:
            # the video's scale is the clip's own maximum, known only now: a second pass over the same chunks
            draw.video_max = _scale_or_one(res["all"]["max_ve"])
            for pv, gv, i, j in _chunk_pairs(_track(pred), _track(gt), 0, T, shape, args.chunk, flame, coef_stats, args.with_global_pose):
                draw.video_chunk(pv, gv)
                del pv, gv
        res.update(draw.finish(_template(shape, flame, coef_stats)))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["all"]))
    return res


if __name__ == "__main__":
    main()
