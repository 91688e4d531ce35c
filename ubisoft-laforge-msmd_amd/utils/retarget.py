"""FLAME motion onto a blendshape rig: one weight curve per slider.

A rig is a neutral mesh, K <= 64 vertex deltas on the SAME topology as the motion, a box [lo, hi] per weight and, optionally,
per-vertex weights and a ridge.  Per frame the weights are the minimiser of the weighted squared vertex distance between
neutral + sum_k w_k delta_k and the frame, inside the box: a bounded least-squares problem solved on the device
(include/msmd_hip.h states the operator and the solver; csrc/retarget.hip holds the kernels).

    rig = prepare_rig(load_rig("rig.npz"))
    weights, status = retarget(vertices, rig)                 # (N, V, 3) fp32 on the device -> (N, K) fp32, (N) int32
    write_curves("curves.csv", weights, rig.names, fps=25)

    python -m msmd_amd.utils.retarget --coeffs C.npy --rig rig.npz --out curves.csv [--video OUT.avi]

Frames are independent and a frame's bits do not depend on the batch it is in, so the chunk size changes nothing.
"""
from __future__ import annotations

import csv
import json

import numpy as np
import torch

from .. import ops

RIG_FIELDS = ("neutral", "deltas", "names", "vertex_weight", "lo", "hi", "ridge")
STATUS_NAMES = {ops.RETARGET_CONVERGED: "converged", ops.RETARGET_CAP_REACHED: "cap_reached",
                ops.RETARGET_BAD_INPUT: "bad_input", ops.RETARGET_NOT_POSITIVE: "not_positive"}


class Rig:
    """The rig as stored, on the host: neutral (V, 3) and deltas (K, V, 3) fp32, names (K), vertex_weight (V) fp32 or None (1),
    lo / hi (K) float64 (default 0 / 1), ridge (K) float64 (default 0).  ValueError for anything the kernels would refuse."""

    def __init__(self, neutral, deltas, names=None, vertex_weight=None, lo=None, hi=None, ridge=None):
        self.neutral = np.ascontiguousarray(np.asarray(neutral), dtype=np.float32)
        self.deltas = np.ascontiguousarray(np.asarray(deltas), dtype=np.float32)
        if self.deltas.ndim != 3 or self.deltas.shape[2] != 3 or self.neutral.shape != self.deltas.shape[1:]:
            raise ValueError(f"neutral must be (V, 3) and deltas (K, V, 3), got {self.neutral.shape} and {self.deltas.shape}")
        K, V = self.deltas.shape[:2]
        if not 1 <= K <= ops.RETARGET_MAX_SHAPES:
            raise ValueError(f"{K} blendshapes; the fit takes 1 .. {ops.RETARGET_MAX_SHAPES}")
        if V < 1:
            raise ValueError("the rig has no vertices")
        self.K, self.V = K, V
        self.names = [f"shape_{k:02d}" for k in range(K)] if names is None else [str(n) for n in np.asarray(names).reshape(-1)]
        if len(self.names) != K:
            raise ValueError(f"{len(self.names)} names for {K} blendshapes")
        per_shape = lambda name, v, fill: np.full(K, fill, np.float64) if v is None else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (K,)))
        self.lo, self.hi, self.ridge = per_shape("lo", lo, 0.0), per_shape("hi", hi, 1.0), per_shape("ridge", ridge, 0.0)
        if not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all() and (self.lo < self.hi).all()):
            raise ValueError("the bounds must be finite with lo < hi for every blendshape")
        if not (np.isfinite(self.ridge).all() and (self.ridge >= 0.0).all()):
            raise ValueError("ridge must be finite and >= 0")
        self.vertex_weight = None
        if vertex_weight is not None:
            vw = np.ascontiguousarray(np.asarray(vertex_weight), dtype=np.float32)
            if vw.shape != (V,) or not (np.isfinite(vw).all() and (vw >= 0.0).all()):
                raise ValueError(f"vertex_weight must hold {V} finite values >= 0")
            self.vertex_weight = vw
        if not (np.isfinite(self.neutral).all() and np.isfinite(self.deltas).all()):
            raise ValueError("the rig's neutral and deltas must be finite")

    def save(self, path):
        d = dict(neutral=self.neutral, deltas=self.deltas, names=np.array(self.names), lo=self.lo, hi=self.hi, ridge=self.ridge)
        if self.vertex_weight is not None:
            d["vertex_weight"] = self.vertex_weight
        np.savez(path, **d)


def load_rig(path):
    """An .npz with `neutral` and `deltas`, and optionally `names`, `vertex_weight`, `lo`, `hi`, `ridge` -> Rig."""
    with np.load(path, allow_pickle=False) as z:
        unknown = sorted(set(z.files) - set(RIG_FIELDS))
        if unknown:
            raise ValueError(f"{path} holds fields a rig does not have: {unknown}")
        for need in ("neutral", "deltas"):
            if need not in z.files:
                raise ValueError(f"{path} has no `{need}`")
        return Rig(**{k: z[k] for k in z.files})


def as_rig(rig):
    if isinstance(rig, (Rig, PreparedRig)):
        return rig
    if isinstance(rig, dict):
        return Rig(**{k: v for k, v in rig.items() if k in RIG_FIELDS})
    raise TypeError(f"a rig is a Rig, a PreparedRig or a dict of its fields, got {type(rig).__name__}")


def check_positive_definite(H, used_vertices=None):
    """Host float64 Cholesky of H (K, K): ValueError that names the fix unless H is positive definite."""
    H = np.asarray(H, dtype=np.float64)
    K = H.shape[0]
    why = None
    if not np.isfinite(H).all():
        why = "it is not finite"
    else:
        try:
            np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            why = "its Cholesky factorisation meets a pivot that is not positive"
    if why is None:
        return
    hint = ""
    if used_vertices is not None and K > 3 * used_vertices:
        hint = f" ({K} blendshapes cannot be told apart by {used_vertices} weighted vertices, 3 coordinates each)"
    raise ValueError(f"the rig's normal matrix H = A A^T + diag(ridge) is not positive definite: {why}{hint}.  The blendshapes are "
                     "linearly dependent on the weighted vertices: give the rig a `ridge` > 0 (a small multiple of trace(H) / K "
                     "is usual), or drop the redundant shapes")


class PreparedRig:
    """A Rig on the device with what the per-frame kernels read: A = fl32(vertex_weight * deltas), G = A A^T and
    H = G + diag(ridge) in float64.  `prepare_rig` builds it, once per rig."""

    def __init__(self, rig, device="cuda"):
        self.rig, self.device = rig, torch.device(device)
        self.K, self.V, self.names, self.lo, self.hi, self.ridge = rig.K, rig.V, rig.names, rig.lo, rig.hi, rig.ridge
        self.neutral = torch.from_numpy(rig.neutral).to(self.device)
        self.deltas = torch.from_numpy(rig.deltas).to(self.device)
        if rig.vertex_weight is None:
            self.vertex_weight, self.A, used = None, self.deltas, rig.V
        else:
            self.vertex_weight = torch.from_numpy(rig.vertex_weight).to(self.device)
            self.A = (self.vertex_weight[None, :, None] * self.deltas).contiguous()     # one fp32 product, rounded once
            used = int((rig.vertex_weight != 0).sum())
        self.used_vertices = used
        self.G, self.H = ops.retarget_gram(self.A, rig.ridge)
        check_positive_definite(self.H.cpu().numpy(), used)


def prepare_rig(rig, device="cuda"):
    """Rig (or a dict of its fields, or a path) -> PreparedRig on `device`.  ValueError if H is not positive definite."""
    if isinstance(rig, PreparedRig):
        return rig
    if isinstance(rig, str):
        rig = load_rig(rig)
    return PreparedRig(as_rig(rig), device)


@torch.no_grad()
def retarget(vertices, rig, chunk=4096, max_iterations=ops.RETARGET_ITERATIONS, return_iterations=False):
    """vertices (N, V, 3) fp32 on the device -> (weights (N, K) fp32, status (N) int32[, iterations (N) int32]).  `chunk` frames
    go through the kernels at a time; the bits do not depend on it.  status: ops.RETARGET_CONVERGED, _CAP_REACHED (the weights are
    the last iterate clipped to the box) or _BAD_INPUT (a non-finite used vertex: the frame's weights are NaN)."""
    rig = prepare_rig(rig, vertices.device if torch.is_tensor(vertices) else "cuda")
    if not torch.is_tensor(vertices) or vertices.dim() != 3 or tuple(vertices.shape[1:]) != (rig.V, 3):
        raise ValueError(f"vertices must be an (N, {rig.V}, 3) tensor on the rig's topology, got {tuple(getattr(vertices, 'shape', ()))}")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk = {chunk} must be at least 1")
    N = vertices.shape[0]
    ws, ss, its = [], [], []
    for i in range(0, max(N, 1), chunk):
        x = vertices[i:i + chunk].float().contiguous()
        b = ops.retarget_rhs(x, rig.neutral, rig.A, rig.vertex_weight)
        w, s, it = ops.retarget_solve(rig.H, b, rig.lo, rig.hi, max_iterations)
        ws.append(w), ss.append(s), its.append(it)
    out = (torch.cat(ws, 0), torch.cat(ss, 0))
    return out + (torch.cat(its, 0),) if return_iterations else out


@torch.no_grad()
def rig_vertices(weights, rig):
    """weights (N, K) fp32 on the device -> the rig's mesh (N, V, 3) fp32: neutral + sum_k w_k delta_k."""
    rig = prepare_rig(rig, weights.device)
    return ops.blendshape_apply(weights.float().contiguous(), rig.neutral, rig.deltas)


def _flame_chunks(coef_dict, flame, chunk):
    c = {k: v.reshape(-1, v.shape[-1]) for k, v in coef_dict.items()}
    T = c["exp"].shape[0]
    for i in range(0, T, chunk):
        yield flame(c["shape"][i:i + chunk].contiguous(), c["exp"][i:i + chunk].contiguous(), c["pose"][i:i + chunk].contiguous(),
                    return_lm2d=False, return_lm3d=False)[0].float().contiguous(), i


@torch.no_grad()
def retarget_coeffs(coef_dict, flame, rig, chunk=512, max_iterations=ops.RETARGET_ITERATIONS, on_chunk=None):
    """get_coef_dict's {'shape', 'exp', 'pose'} -> FLAME vertices `chunk` frames at a time -> (weights (T, K), status (T)): one chunk
    of vertices is alive.  on_chunk(vertices, weights, i), when given, sees every chunk (a report or a video rides on the pass)."""
    rig = prepare_rig(rig, coef_dict["exp"].device)
    ws, ss = [], []
    for v, i in _flame_chunks(coef_dict, flame, int(chunk)):
        w, s = retarget(v, rig, chunk=v.shape[0], max_iterations=max_iterations)
        ws.append(w), ss.append(s)
        if on_chunk is not None:
            on_chunk(v, w, i)
        del v
    K = rig.K
    dev = coef_dict["exp"].device
    return (torch.cat(ws, 0) if ws else torch.empty(0, K, device=dev), torch.cat(ss, 0) if ss else torch.empty(0, dtype=torch.int32, device=dev))


@torch.no_grad()
def retarget_report(vertices, weights, rig, chunk=4096):
    """How much of the motion the rig reproduces: {'mean', 'max', 'rms'} vertex error in the vertices' unit between `vertices` and
    rig_vertices(weights), through utils/metrics.VertexMetrics (all vertices, weighted or not), plus 'frames'."""
    from .metrics import VertexMetrics
    rig = prepare_rig(rig, vertices.device)
    N = vertices.shape[0]
    if N < 1:
        raise ValueError("no frames to report on")
    vm = VertexMetrics([0, N], rig.V, [0], [0], rig.neutral, vertices.device)
    for i in range(0, N, int(chunk)):
        vm.update(rig_vertices(weights[i:i + chunk], rig), vertices[i:i + chunk].float().contiguous())
    r = vm.result()["all"]
    return dict(mean=r["mve"], max=r["max_ve"], rms=r["rmse"], frames=N)


def write_curves(path, weights, names, fps):
    """One curve per blendshape.  `.csv`: a header row of the names, then one row per frame (repr of the fp32 value: it reads back
    to the same bits); `.json`: {"fps", "names", "weights"}, weights a list of rows."""
    w = weights.detach().cpu().numpy() if torch.is_tensor(weights) else np.asarray(weights)
    w = np.asarray(w, dtype=np.float32)
    names = [str(n) for n in names]
    if w.ndim != 2 or w.shape[1] != len(names):
        raise ValueError(f"weights {w.shape} do not go with {len(names)} names")
    fps = float(fps)
    if not 0.0 < fps < float("inf"):
        raise ValueError(f"fps = {fps} must be finite and greater than 0")
    low = str(path).lower()
    if low.endswith(".csv"):
        with open(path, "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(names)
            for row in w:
                wr.writerow([repr(float(v)) for v in row])
    elif low.endswith(".json"):
        with open(path, "w") as f:
            json.dump(dict(fps=fps, names=names, weights=[[float(v) for v in row] for row in w]), f)
    else:
        raise ValueError(f"{path}: curves are written as .csv or .json")


def read_curves(path):
    """-> (names, weights (T, K) fp32, fps or None): what write_curves wrote (a .csv does not hold the frame rate)."""
    low = str(path).lower()
    if low.endswith(".csv"):
        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        names = rows[0]
        return names, np.array([[float(v) for v in r] for r in rows[1:]], dtype=np.float32).reshape(len(rows) - 1, len(names)), None
    if low.endswith(".json"):
        with open(path) as f:
            d = json.load(f)
        return d["names"], np.array(d["weights"], dtype=np.float32).reshape(len(d["weights"]), len(d["names"])), d["fps"]
    raise ValueError(f"{path}: curves are read from .csv or .json")


@torch.no_grad()
def comparison_frames(vertices, weights, rig, faces, renderer, vmax, table="jet"):
    """FLAME as ground truth | the rig's reconstruction | its error heat map: utils/metrics.render_comparison on one chunk."""
    from .metrics import render_comparison
    return render_comparison(rig_vertices(weights, rig), vertices.float().contiguous(), faces, renderer, vmax, table)


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(description="Retarget a FLAME coefficient track to a blendshape rig on the MI355X: one weight "
                                             "curve per slider.")
    ap.add_argument("--coeffs", type=str, required=True, help=".npy of a (T, 53 | 54) track: 50 expression, 3 head rotation[, jaw]")
    ap.add_argument("--rig", type=str, required=True, help=".npz with neutral (V, 3), deltas (K, V, 3) and optionally names, "
                                                           "vertex_weight, lo, hi, ridge")
    ap.add_argument("--out", type=str, required=True, help="curves.csv or curves.json")
    ap.add_argument("--shape", type=str, default=None, help=".npy of the subject's (100) shape code (default: zeros)")
    ap.add_argument("--fps", type=float, default=25.0)
    ap.add_argument("--chunk", type=int, default=512, help="frames decoded by FLAME at a time")
    ap.add_argument("--max_iterations", type=int, default=ops.RETARGET_ITERATIONS)
    ap.add_argument("--with_global_pose", action="store_true", help="keep the head rotation (default: the head is still, as a rig's "
                                                                    "neutral is)")
    ap.add_argument("--flame_model_path", type=str, default=None)
    ap.add_argument("--flame_lmk_embedding_path", type=str, default=None)
    ap.add_argument("--video", type=str, default=None, metavar="OUT.avi", help="Motion-JPEG AVI of FLAME | rig | error heat map")
    ap.add_argument("--error_max", type=float, default=None, metavar="METRES", help="top of the video's colour scale (default: "
                                                                                     "the clip's maximum error, a second pass)")
    ap.add_argument("--render_size", type=int, default=256)
    ap.add_argument("--video_quality", type=int, default=90)
    return ap


def main(argv=None):
    from types import SimpleNamespace
    from .common import get_coef_dict
    from .flame import FLAME, FLAMEConfig
    from .metrics import _track
    args = build_parser().parse_args(argv)
    if args.chunk < 1 or not 0.0 < args.fps < float("inf"):
        raise SystemExit("--chunk must be at least 1 and --fps finite and > 0")
    device = torch.device("cuda")
    coef = _track(torch.from_numpy(np.load(args.coeffs)).to(device))
    shape = torch.zeros(1, 100, device=device) if args.shape is None else \
        torch.from_numpy(np.load(args.shape).astype(np.float32)).reshape(1, 100).to(device)
    cfg = SimpleNamespace(**{k: v for k, v in vars(FLAMEConfig).items() if not k.startswith("__")})
    if args.flame_model_path is not None:
        cfg.flame_model_path = args.flame_model_path
    if args.flame_lmk_embedding_path is not None:
        cfg.flame_lmk_embedding_path = args.flame_lmk_embedding_path
    flame = FLAME(cfg).to(device)
    rig = prepare_rig(load_rig(args.rig), device)
    T = coef.shape[0]
    cd = get_coef_dict(coef, shape.expand(T, -1), None, with_global_pose=args.with_global_pose)
    from .metrics import VertexMetrics
    vm = VertexMetrics([0, max(T, 1)], rig.V, [0], [0], rig.neutral, device)

    def see(v, w, i):
        vm.update(rig_vertices(w, rig), v)
    weights, status = retarget_coeffs(cd, flame, rig, args.chunk, args.max_iterations, on_chunk=see)
    write_curves(args.out, weights, rig.names, args.fps)
    r = vm.result()["all"] if T else dict(mve=0.0, max_ve=0.0, rmse=0.0)
    st = status.cpu().numpy()
    rep = dict(frames=T, mean=r["mve"], max=r["max_ve"], rms=r["rmse"],
               status={name: int((st == code).sum()) for code, name in STATUS_NAMES.items()})
    if args.video is not None and T:
        from . import media
        from .metrics import _scale_or_one
        from .renderer import MeshRenderer
        renderer = MeshRenderer((args.render_size, args.render_size))
        vmax = args.error_max if args.error_max is not None else _scale_or_one(r["max_ve"])
        jpegs = []
        for v, i in _flame_chunks(cd, flame, args.chunk):
            jpegs += media.encode_jpeg(comparison_frames(v, weights[i:i + v.shape[0]], rig, flame.faces_tensor, renderer, vmax),
                                       args.video_quality)
        media.write_avi(args.video, jpegs, args.fps, (3 * args.render_size, args.render_size), None)
        rep["error_max_video"] = vmax
    print(json.dumps(rep))
    return rep


if __name__ == "__main__":
    main()
