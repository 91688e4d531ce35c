"""Times the vertex-space metrics (utils/metrics.VertexMetrics, csrc/vertex_metrics.hip) on a validation-sized case:
25 600 frames of 5 023 vertices in 256 clips of 100 frames, fp32 and fp16, an upper-face mask of 1 000 vertices in runs of 50 and a
lip mask of 254, consumed in chunks of 512 frames.

Per dtype, HIP events around one pass over all chunks, median of --rounds after one warm-up pass:
  update      VertexMetrics.update per chunk (both kernels, the wrappers' checks and allocations included)
  frame       msmd_vertex_frame_errors alone per chunk, raw C calls on preallocated buffers
  frame, 1 launch   the same kernel over all frames in ONE call: what the 512-frame launches' boundaries and ramps cost
  moments     msmd_vertex_motion_moments alone per chunk, raw C calls
  torch       the same metrics written in plain torch on the same device and chunks (float64 after the loads, as the kernels): the
              only way to get them without this module, so the baseline
GB/s counts the bytes of the two vertex tensors ONCE per pass (2 n V 3 elements); `update` reads the upper-face vertices a second
time.  The share of the HBM peak is against 8.0 TB/s.  The two results are compared before anything is printed.

    python tools/bench_vertex_metrics.py [--frames 25600] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmd_amd import _lib, ops  # noqa: E402
from msmd_amd.utils import metrics as M  # noqa: E402

V, CLIP, CHUNK, HBM_PEAK = 5023, 100, 512, 8.0e12


def timed(fn, rounds):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def torch_metrics(pred, gt, off, lips, upper, template):
    """What a user would write on top of coef_dict_to_vertices: chunked, float64 after the loads."""
    rows, mp, mg = [], [], []
    tu = template[upper].double()
    for i in range(0, pred.shape[0], CHUNK):
        p, g = pred[i:i + CHUNK].double(), gt[i:i + CHUNK].double()
        d2 = (p - g).square().sum(-1)
        d = d2.sqrt()
        rows.append(torch.stack([d2[:, lips].amax(1), d.sum(1), d.amax(1), d2.sum(1)], 1))
        mp.append((p[:, upper] - tu).square().sum(-1))
        mg.append((g[:, upper] - tu).square().sum(-1))
    table, mp, mg = torch.cat(rows), torch.cat(mp), torch.cat(mg)
    n_clips = len(off) - 1       # equal clips: one reshape instead of a loop over them
    sp, sg = (m.view(n_clips, CLIP, -1).std(1, unbiased=False).mean(1) for m in (mp, mg))
    t = table.view(n_clips, CLIP, 4)
    return dict(lve=t[:, :, 0].mean(1), mve=t[:, :, 1].sum(1) / (CLIP * V), max_ve=t[:, :, 2].amax(1),
                rmse=(t[:, :, 3].sum(1) / (CLIP * V)).sqrt(), fdd=sg - sp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25600)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    n = args.frames - args.frames % CLIP
    dev = torch.device("cuda:0")
    off = list(range(0, n + 1, CLIP))
    upper = np.concatenate([np.arange(s, s + 50) for s in range(200, 5000, 240)])
    lips = np.arange(1500, 1754)
    g = torch.Generator(device=dev).manual_seed(1)
    template = 0.1 * torch.randn(V, 3, device=dev, generator=g)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    lines = [f"vertex metrics: {n} frames x {V} vertices, {len(off) - 1} clips of {CLIP}, chunks of {CHUNK}, U = {len(upper)}, "
             f"{len(lips)} lip vertices; {torch.cuda.get_device_name(0)}; median (min .. max) of {args.rounds} passes"]
    for dt in (torch.float32, torch.float16):
        gt = (template + 0.01 * torch.randn(n, V, 3, device=dev, generator=g)).to(dt)
        pred = (gt.float() + 0.002 * torch.randn(n, V, 3, device=dev, generator=g)).to(dt)
        nbytes = 2 * n * V * 3 * gt.element_size()
        region, up = M.regions(V, lips, upper, dev)
        lips_t, upper_t = torch.from_numpy(lips).to(dev), torch.from_numpy(upper).to(dev)
        off_dev = torch.tensor(off, dtype=torch.int64).to(dev)
        res = {}

        def update():
            vm = M.VertexMetrics(off, V, lips, upper, template, dev)
            for i in range(0, n, CHUNK):
                vm.update(pred[i:i + CHUNK], gt[i:i + CHUNK])
            res["vm"] = vm

        out = torch.empty(n, 4, device=dev, dtype=torch.float64)
        state = torch.zeros(len(off) - 1, len(upper), 2, 3, device=dev, dtype=torch.float64)
        code = ops._dt(gt)

        def frame():
            for i in range(0, n, CHUNK):
                c = min(CHUNK, n - i)
                lib.msmd_vertex_frame_errors(pred[i:].data_ptr(), gt[i:].data_ptr(), region.data_ptr(), out[i:].data_ptr(), c, V, code, st)

        def frame_one_launch():
            lib.msmd_vertex_frame_errors(pred.data_ptr(), gt.data_ptr(), region.data_ptr(), out.data_ptr(), n, V, code, st)

        def moments():
            for i in range(0, n, CHUNK):
                c = min(CHUNK, n - i)
                lib.msmd_vertex_motion_moments(pred[i:].data_ptr(), gt[i:].data_ptr(), i, c, off_dev.data_ptr(), len(off) - 1,
                                               up.data_ptr(), len(upper), template.data_ptr(), 0, state.data_ptr(), V, code, st)

        def baseline():
            res["torch"] = torch_metrics(pred, gt, off, lips_t, upper_t, template)

        t_upd, t_frame, t_one, t_mom, t_torch = (timed(f, args.rounds) for f in (update, frame, frame_one_launch, moments, baseline))
        ours, theirs = res["vm"].result(), res["torch"]
        worst = {k: float(max(abs(c[k] - float(theirs[k][i])) / max(abs(c[k]), 1e-300) for i, c in enumerate(ours["clips"])))
                 for k in ("lve", "mve", "max_ve", "rmse")}
        worst["fdd (absolute)"] = float(max(abs(c["fdd"] - float(theirs["fdd"][i])) for i, c in enumerate(ours["clips"])))
        name = str(dt).split(".")[-1]
        lines.append(f"{name}: largest relative difference, kernels against torch, per clip: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        for tag, (med, lo, hi) in (("update", t_upd), ("frame", t_frame), ("frame, 1 launch", t_one), ("moments", t_mom), ("torch", t_torch)):
            rate = nbytes / (med * 1e-3)
            lines.append(f"{name} {tag:15s} {med:9.3f} ms ({lo:.3f} .. {hi:.3f})  {rate / 1e9:8.1f} GB/s of vertex bytes  "
                         f"{rate / HBM_PEAK:.3f} of the HBM peak" + (f"  {t_torch[0] / med:.2f}x torch" if tag != "torch" else ""))
        del pred, gt
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
