"""Time the retargeting kernels at the shape of the LBS benchmark.

    timeout 300 python tools/bench_retarget.py [--frames 25600] [--V 5023] [--K 52] [--noise 0.01] [--out FILE]

The work: the synthetic rig `synth.blendshape_rig(V, K, 0)`, `--frames` meshes made on the device from random weights (about a
fifth at each bound) plus vertex noise of `--noise` times the largest delta.  Each of `ops.retarget_rhs` (two launches),
`ops.retarget_solve` and `ops.blendshape_apply` is timed alone with HIP events around the call: the median of 9 after three
warm-up calls, every operand already on the device.  Beside them, for scale, FLAME's forward (blendshapes + LBS) for the same
number of frames on the synthetic asset when V is FLAME's.
The rhs time is set against two ceilings: the x stream at 6.0 TB/s and the 2 N 64 3V FLOP of the padded product at 155 TF/s
(exact-fp32 MFMA); the apply time against its store stream at the same 6.0 TB/s.
Prints one JSON line.  No threshold is asserted.  Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from msmd_amd import ops, synth  # noqa: E402
from msmd_amd.utils import retarget as RT  # noqa: E402

HBM_TBS, MFMA_F32_TFS = 6.0, 155.0


def timed(call, reps):
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = call()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return out, float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25600)
    ap.add_argument("--V", type=int, default=5023)
    ap.add_argument("--K", type=int, default=52)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_retarget.py needs an MI355X"
    N, V, K = a.frames, a.V, a.K
    raw = synth.blendshape_rig(V, K, 0)
    rig = RT.prepare_rig(raw, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    w_true = (1.6 * torch.rand(N, K, device="cuda", generator=gen) - 0.3).clamp_(0.0, 1.0)
    x = RT.rig_vertices(w_true, rig)
    step = max(1, N // 8)
    for i in range(0, N, step):           # noise in slices: one more copy of the stream is never alive
        x[i:i + step] += a.noise * float(np.abs(raw["deltas"]).max()) * torch.randn(x[i:i + step].shape, device="cuda", generator=gen)
    b, rhs_ms, rhs_min, rhs_max = timed(lambda: ops.retarget_rhs(x, rig.neutral, rig.A, rig.vertex_weight), a.reps)
    (w, status, its), solve_ms, solve_min, solve_max = timed(lambda: ops.retarget_solve(rig.H, b, rig.lo, rig.hi), a.reps)
    recon, apply_ms, apply_min, apply_max = timed(lambda: ops.blendshape_apply(w, rig.neutral, rig.deltas), a.reps)
    stream_ms = 1e3 * (4.0 * N * V * 3) / (HBM_TBS * 1e12)
    mfma_ms = 1e3 * (2.0 * N * 64 * 3 * V) / (MFMA_F32_TFS * 1e12)
    res = dict(device=torch.cuda.get_device_name(0), frames=N, V=V, K=K, reps=a.reps, cond_H=float(np.linalg.cond(rig.H.cpu().numpy())),
               rhs_ms=round(rhs_ms, 4), rhs_ms_min=round(rhs_min, 4), rhs_ms_max=round(rhs_max, 4),
               rhs_stream_ceiling_ms=round(stream_ms, 4), rhs_mfma_ceiling_ms=round(mfma_ms, 4),
               rhs_over_stream=round(rhs_ms / stream_ms, 2), rhs_over_mfma=round(rhs_ms / mfma_ms, 2),
               rhs_tbs=round(4.0 * N * V * 3 / rhs_ms / 1e9, 3), rhs_tflops_padded=round(2.0 * N * 64 * 3 * V / rhs_ms / 1e9, 2),
               solve_ms=round(solve_ms, 4), solve_ms_min=round(solve_min, 4), solve_ms_max=round(solve_max, 4),
               solve_us_per_frame=round(1e3 * solve_ms / max(N, 1), 4),
               iterations_mean=float(its.float().mean()), iterations_max=int(its.max()), flagged=int((status != 0).sum()),
               apply_ms=round(apply_ms, 4), apply_ms_min=round(apply_min, 4), apply_ms_max=round(apply_max, 4),
               apply_over_stream=round(apply_ms / stream_ms, 2), apply_tbs=round(4.0 * N * V * 3 / apply_ms / 1e9, 3),
               weight_err_median=float((w - w_true).abs().median()), weight_err_max=float((w - w_true).abs().max()),
               vertex_rms=float(((recon - x) ** 2).sum(-1).mean().sqrt()))
    if V == synth.FLAME_V:
        from msmd_amd.utils.flame import FLAME, FLAMEConfig
        cfg = SimpleNamespace(**vars(FLAMEConfig))
        cfg.asset = synth.flame_asset()
        fl = FLAME(cfg).cuda()
        shp = torch.zeros(N, 100, device="cuda")
        exp = 0.5 * torch.randn(N, 50, device="cuda", generator=gen)
        pose = 0.1 * torch.randn(N, 6, device="cuda", generator=gen)
        _, lbs_ms, _, _ = timed(lambda: fl(shp, exp, pose, return_lm2d=False, return_lm3d=False)[0], a.reps)
        res["flame_forward_ms"] = round(lbs_ms, 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
