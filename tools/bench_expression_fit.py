"""Time msmd_expression_fit at the shape of a preprocessing batch.

    timeout 300 python tools/bench_expression_fit.py [--frames 25600] [--K 68] [--NE 50] [--jaw_dof 1] [--iterations 12] [--out FILE]

The work: `--frames` frames of K landmarks on the synthetic FLAME asset, model-space targets from random (e, theta) plus noise of
2e-4, one `ops.expression_fit` call (one launch) per measurement, HIP events around the call, the median of 9 after three
warm-up calls; the landmarks and the reduced tables are already on the device.  The same call is then captured once into a
hipGraph and replayed: its outputs must be the eager call's bits.
FLOPs are counted from the algorithm, per frame and iteration, as 2 per multiply-add:
    the two evaluations of the landmarks (12 K (NE + 9)), the Jacobian (18 K NE + 42 K jaw_dof), the lower triangle of
    Jm^T W Jm (3 K NP (NP + 1)), g (6 K NP), the Cholesky factorisation (NP^3 / 3) and the two solves (2 NP^2), NP = NE + jaw_dof;
`executed` counts what the kernel issues instead: the full 64 x 64 product and update per row and per pivot.
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
from msmd_amd.utils import expression_fit as EF  # noqa: E402
from msmd_amd.utils.flame import FLAME, FLAMEConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25600)
    ap.add_argument("--K", type=int, default=68)
    ap.add_argument("--NE", type=int, default=50)
    ap.add_argument("--jaw_dof", type=int, default=1)
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_expression_fit.py needs an MI355X"
    n, K, NE, jd, its = a.frames, a.K, a.NE, a.jaw_dof, a.iterations
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset, cfg.n_exp = synth.flame_asset(), NE
    fl = FLAME(cfg).cuda()
    g = np.random.default_rng(0)
    fidx = g.integers(0, fl.faces_tensor.shape[0], K)
    bary = g.random((K, 3)) + 0.05
    bary /= bary.sum(1, keepdims=True)
    tab, tab0 = EF.reduce_flame(fl, fidx, bary, torch.from_numpy(0.5 * g.standard_normal(100)))
    # targets through the reduced tables in float64 on the device: l = X + M Y at random (e, theta_x)
    gen = torch.Generator(device="cuda").manual_seed(0)
    e = 1.5 * torch.randn(n, NE, device="cuda", dtype=torch.float64, generator=gen)
    th = torch.zeros(n, 3, device="cuda", dtype=torch.float64)
    th[:, 0] = 0.5 * torch.rand(n, device="cuda", dtype=torch.float64, generator=gen)
    from msmd_amd.utils.lbs import _rodrigues_torch
    M = _rodrigues_torch(th) - torch.eye(3, device="cuda", dtype=torch.float64)
    v = tab0[0][None] + torch.einsum("kru,nu->nkr", tab, torch.cat([e, M.reshape(n, 9)], 1))
    y = v[..., :3] + torch.einsum("nxy,nky->nkx", M, v[..., 3:])
    y = (y + 2e-4 * torch.randn(y.shape, device="cuda", dtype=torch.float64, generator=gen)).float().contiguous()
    subject = torch.zeros(n, device="cuda", dtype=torch.int32)
    w = torch.ones(K, device="cuda", dtype=torch.float64)
    call = lambda: ops.expression_fit(y, subject, tab, tab0, w, jd, 1e-6, 0.0, its)
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = call()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    code, jaw, rms, status = out
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard():
        with torch.cuda.graph(graph):
            gout = call()
    graph.replay()
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int32), z.view(torch.int32)) for x, z in zip(out, gout))
    NP = NE + jd
    algo = 12 * K * (NE + 9) + 18 * K * NE + 42 * K * jd + 3 * K * NP * (NP + 1) + 6 * K * NP + NP ** 3 / 3 + 2 * NP * NP
    executed = 12 * K * (NE + 9) + 18 * K * NE + 42 * K * jd + 2 * 3 * K * 64 * 64 + 6 * K * NP + 2 * NP * 64 * 64 + 2 * NP * NP
    med = float(np.median(ms))
    res = dict(device=torch.cuda.get_device_name(0), frames=n, K=K, NE=NE, jaw_dof=jd, iterations=its, reps=a.reps,
               ms_median=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
               us_per_frame=round(1e3 * med / n, 3), mflop_per_frame_iteration=round(algo / 1e6, 3),
               tflops_fp64_algorithmic=round(algo * its * n / med / 1e9, 2), tflops_fp64_executed=round(executed * its * n / med / 1e9, 2),
               graph_replay_same_bits=bool(same), rms_median=float(rms.median()), code_err_median=float((code.double() - e).abs().median()),
               flagged=int((status != 0).sum()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    assert same, "the captured call did not reproduce the eager call's bits"


if __name__ == "__main__":
    main()
