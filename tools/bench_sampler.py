"""Dev tool: MSMD.sample throughput (T=500, 3 CFG entries) at several batch sizes.

`bench_sampler.py controlled [B,B,...] [out.json]` instead times the two controllable entry points, sample_with_guide (4
keyframes per clip) and sample_separate, as the default call (500 eager DDPM steps) against solver="dpmpp_2m",
sample_steps=25 on the graph loop: same process, the two forms alternating, HIP events around one call, median of PAIRS
(default 5) pairs after one warm-up call each.  Prints one JSON line (DTYPE defaults to fp16 in this mode)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from msmd_amd.config import synthetic_args
from msmd_amd.model import get_diffusion_model


def controlled(batches, out_path=None):
    import json, statistics
    dtype, pairs = os.environ.get("DTYPE", "fp16"), max(5, int(os.environ.get("PAIRS", "5")))
    model = get_diffusion_model(synthetic_args(compute_dtype=dtype), "cuda").eval()
    T = model.diffusion_sched.num_steps
    out = dict(tool="tools/bench_sampler.py controlled", dtype=dtype, T=T, cfg_entries=3, pairs=pairs,
               timing="HIP events around one call, the two forms alternating in one process, median",
               device=torch.cuda.get_device_name())

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        return a.elapsed_time(b)

    for B in batches:
        g = torch.Generator(device="cuda").manual_seed(B)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
        af, shape, style, ind = rn(B, 100, 512), torch.zeros(B, 100, device="cuda"), rn(B, 256), torch.ones(B, 100, device="cuda")
        kw = dict(indicator=ind, cfg_scale=1.15)
        guide = dict(guidance_indice=[0, 33, 66, 99], guidance_values=rn(4, 67))
        few = dict(solver="dpmpp_2m", sample_steps=25)
        r = {}
        for name, call, extra in (("guided", model.sample_with_guide, guide), ("separated", model.sample_separate, {})):
            slow = lambda: call(af, shape, style, **kw, **extra)
            fast = lambda: call(af, shape, style, **kw, **extra, **few)
            slow(); fast()                                   # warm-up: packs, lazy kernel loading, graph capture
            ts = [(timed(slow), timed(fast)) for _ in range(pairs)]
            a, b = statistics.median(t[0] for t in ts), statistics.median(t[1] for t in ts)
            r[name] = dict(ddpm_500_eager_ms=round(a, 2), dpmpp_2m_25_graph_ms=round(b, 3), ratio=round(b / a, 4),
                           speedup=round(a / b, 1), pairs_ms=[[round(x, 2), round(y, 3)] for x, y in ts])
        out[f"B{B}"] = r
        model.__dict__.pop("_step_graphs", None)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if len(sys.argv) > 1 and sys.argv[1] == "controlled":
    controlled([int(b) for b in (sys.argv[2] if len(sys.argv) > 2 else "1,64").split(",")], sys.argv[3] if len(sys.argv) > 3 else None)
    sys.exit(0)
model = get_diffusion_model(synthetic_args(compute_dtype=os.environ.get("DTYPE", "bf16")), "cuda").eval()
if os.environ.get("PQA") == "0":
    model.denoising_net.fused_person_query = False
T = int(os.environ.get("T", "500"))
for B in [int(b) for b in (sys.argv[1] if len(sys.argv) > 1 else "1,8,64").split(",")]:
    af = torch.randn(B, 100, 512, device="cuda"); shape = torch.zeros(B, 100, device="cuda"); style = torch.randn(B, 256, device="cuda")
    ind = torch.ones(B, 100, device="cuda")
    if T != 500:
        from msmd_amd.model import DiffusionSchedule
        model.diffusion_sched = DiffusionSchedule(T, "cosine").to("cuda")
    model.sample(af, shape, style, indicator=ind, cfg_scale=1.15)  # warm-up
    torch.cuda.synchronize(); t0 = time.perf_counter()
    model.sample(af, shape, style, indicator=ind, cfg_scale=1.15)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f"B={B}: {dt:.3f} s for {T} steps x 3 entries -> {B * 100 / dt:.1f} frames/s, {dt / T * 1e3:.3f} ms/step, "
          f"{B * 3 * 7.886e9 * T / dt / 1e12:.1f} TFLOP/s")
