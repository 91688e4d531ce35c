"""Dev tool: MSMD.sample per call on the hipGraph path, DDPM over T = 500 against the few-step solvers (DDIM S = 50 / 100,
DPM-Solver++(2M) S = 25 / 50), at B = 64 (BASELINE configs[4]: fp16, 3 CFG entries) and B = 1 (one infer_coeffs window).
HIP-event timing, one warm-up call (packs, graph capture) then the median of --reps calls.  Prints one JSON line: ms per
call, ms per step, and per solver the per-step slope (t(S2) - t(S1)) / (S2 - S1) next to DDPM's per-step cost."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from msmd_amd import synth  # noqa: E402
from msmd_amd.config import synthetic_args  # noqa: E402
from msmd_amd.model import get_diffusion_model  # noqa: E402

CASES = [("ddpm", None), ("ddim", 50), ("ddim", 100), ("dpmpp_2m", 25), ("dpmpp_2m", 50)]


def time_calls(fn, reps):
    fn()                                   # warm-up: captures this solver's step graph
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = "cuda"
    model = get_diffusion_model(synthetic_args(compute_dtype=a.dtype), dev).eval()
    T = model.diffusion_sched.num_steps
    out = dict(tool="tools/bench_sampler_solvers.py", dtype=a.dtype, T=T, cfg_entries=3, reps=a.reps,
               timing="HIP events around one model.sample call (hipGraph path), median", device=torch.cuda.get_device_name())
    for B in (int(b) for b in a.batches.split(",")):
        t = lambda x: torch.from_numpy(x).to(dev)
        af, style = t(synth.normalish("bss/af", (B, 100, 512))), t(synth.normalish("bss/style", (B, 256)))
        shape, ind = torch.zeros(B, 100, device=dev), torch.ones(B, 100, device=dev)
        xT = t(synth.normalish("bss/xT", (B, 100, 67)))
        r = {}
        for solver, S in CASES:
            kw = {} if solver == "ddpm" else dict(solver=solver, sample_steps=S)
            ms = time_calls(lambda: model.sample(af, shape, style, motion_at_T=xT, indicator=ind, cfg_scale=1.15, **kw),
                            a.reps)
            n = S or T
            r[f"{solver}_S{n}"] = dict(ms=round(ms, 3), ms_per_step=round(ms / n, 4))
        ddpm_step = r[f"ddpm_S{T}"]["ms_per_step"]
        slopes = {}
        for solver, (s1, s2) in (("ddim", (50, 100)), ("dpmpp_2m", (25, 50))):
            sl = (r[f"{solver}_S{s2}"]["ms"] - r[f"{solver}_S{s1}"]["ms"]) / (s2 - s1)
            slopes[solver] = dict(ms_per_step=round(sl, 4), vs_ddpm_step=round(sl / ddpm_step, 4))
        r["slope"] = slopes
        r["dpmpp_2m_S25_over_ddpm_S500"] = round(r["dpmpp_2m_S25"]["ms"] / r[f"ddpm_S{T}"]["ms"], 4)
        out[f"B{B}"] = r
        model.__dict__.pop("_step_graphs", None)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return line


if __name__ == "__main__":
    main()
