"""Style-adherence loss, forward + backward (csrc/style_loss.hip), next to the reference's own broadcast
expression run by torch on the same card, alternated in the same call.

    timeout 300 python tools/bench_style_loss.py [--B 32] [--T 100] [--K 100 750] [--F 53] [--seconds 0.5] [--out FILE]

Two forms of loss(X, S).backward() with gradients into both operands:
  hip        utils/common.StyleAdherenceLoss (msmd_style_adherence_forward / _backward and the ordered mean through autograd);
  torch_ref  the reference's expression (utils/common.py:56-82): X.unsqueeze(2) - S.unsqueeze(1), square, mean over F,
             softmax(-lambda d), weighted sum, mean -- what a user runs without the kernels; autograd keeps (B, T, K, F)
             intermediates alive for its backward.
Device events around batches of forward + backward calls after warm-up; the forms take turns batch by batch until each has
filled --seconds; the median batch gives the per-call time.  Peak memory: torch.cuda.max_memory_allocated over one forward +
backward of each form, above what was allocated before the call (the inputs; so the two gradients count for both forms).  The outputs and gradients of the two forms are
compared first.  One JSON line per K."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from msmd_amd.utils.common import StyleAdherenceLoss  # noqa: E402


def torch_ref(X, S, lam):
    d = torch.mean((X.float().unsqueeze(2) - S.float().unsqueeze(1)) ** 2, dim=-1)
    return torch.mean(torch.sum(F.softmax(-lam * d, dim=-1) * d, dim=-1))


def batch_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, seconds):
    """{name: (median per-call ms, min, max, batches)}: warm-up, a batch size that fills ~20 ms per form, the forms in turn."""
    inner = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        inner[name] = max(1, min(2000, int(20.0 / max(batch_ms(fn, 5), 1e-3))))
    times, spent = {n: [] for n in fns}, {n: 0.0 for n in fns}
    while min(spent.values()) < seconds * 1e3:
        for name, fn in fns.items():
            ms = batch_ms(fn, inner[name])
            times[name].append(ms)
            spent[name] += ms * inner[name]
    return {n: (statistics.median(v), min(v), max(v), len(v)) for n, v in times.items()}


def peak_bytes(fn, leaves):
    for t in leaves:                       # the gradients of an earlier call are not part of "before"
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--K", type=int, nargs="+", default=[100, 750])
    ap.add_argument("--F", type=int, default=53)
    ap.add_argument("--lambda_softmin", type=float, default=10.0)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_style_loss needs an MI355X"
    dev = torch.device("cuda:0")
    loss = StyleAdherenceLoss(True, a.lambda_softmin)
    lines = []
    for K in a.K:
        gen = torch.Generator(device=dev).manual_seed(K)
        X = (0.6 * torch.randn(a.B, a.T, a.F, device=dev, generator=gen)).requires_grad_(True)
        S = (0.6 * torch.randn(a.B, K, a.F, device=dev, generator=gen)).requires_grad_(True)

        def step(form):
            X.grad = S.grad = None
            y = loss(X, S) if form == "hip" else torch_ref(X, S, a.lambda_softmin)
            y.backward()
            return y
        vals = {}
        for form in ("hip", "torch_ref"):
            y = step(form)
            vals[form] = (float(y.detach()), X.grad.clone(), S.grad.clone())
        rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
        diff = dict(loss=abs(vals["hip"][0] - vals["torch_ref"][0]) / abs(vals["torch_ref"][0]),
                    dX=rel(vals["hip"][1], vals["torch_ref"][1]), dS=rel(vals["hip"][2], vals["torch_ref"][2]))
        peaks = {form: peak_bytes(lambda form=form: step(form), (X, S)) for form in ("hip", "torch_ref")}
        ms = alternate({form: (lambda form=form: step(form)) for form in ("hip", "torch_ref")}, a.seconds)
        # per (b, t, k, f): 3 flop for d in the forward; in each of the two backward launches d again and an fma on the difference
        flop = (3.0 + 6.0 + 6.0) * a.B * a.T * K * a.F
        line = dict(op="style_adherence_fwd_bwd", device=torch.cuda.get_device_name(0), B=a.B, T=a.T, K=K, F=a.F,
                    lambda_softmin=a.lambda_softmin,
                    ms={k: round(v[0], 5) for k, v in ms.items()},
                    ms_min_max_batches={k: [round(v[1], 5), round(v[2], 5), v[3]] for k, v in ms.items()},
                    speedup_vs_torch_ref=round(ms["torch_ref"][0] / ms["hip"][0], 2),
                    hip_GFLOPs=round(flop / (ms["hip"][0] * 1e-3) / 1e9, 1),
                    peak_bytes_above_inputs=peaks, peak_ratio=round(peaks["torch_ref"] / max(peaks["hip"], 1), 1),
                    one_BTKF_tensor_bytes=a.B * a.T * K * a.F * 4, input_bytes=(a.B * a.T + a.B * K) * a.F * 4,
                    max_rel_diff_vs_torch_ref=diff)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del X, S, vals
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
