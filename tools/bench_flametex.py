"""FLAMETex forward and backward (csrc/flametex.hip) next to the same semantics written with torch ops on the
device, alternated in the same call.

    timeout 300 python tools/bench_flametex.py [--n_tex 50 200] [--bs 1] [--seconds 0.4] [--out FILE]

Three forms, all on the full 512 x 512 x 3 model:
  hip        utils/flame.FLAMETex (msmd_flametex_forward / msmd_flametex_backward through autograd);
  torch_ref  the reference's expression (utils/flame.py:296-300): broadcast product, sum, permute, F.interpolate, channel
             index, repeat -- what a user runs without the kernels;
  torch_rows the rules restated with the surviving rows gathered first (index_select of 3 Hd Wd rows, then a matrix-vector
             product): the least traffic torch ops allow.
Device events around batches of calls after warm-up; the forms take turns batch by batch until each has filled --seconds;
the median batch gives the per-call time.  Backward = torch.autograd.grad of a retained forward graph, for every form.
`hip_launcher` is ops.flametex_forward / ops.flametex_backward called directly (no autograd node); GB/s and the share of the
8 TB/s peak are taken on it, on the algorithmic bytes: forward 3 Hd Wd n_tex 4 (basis) + 3 Hd Wd 4 (mean) + bs 3 Hd Wd 4
(output); backward the basis rows + bs 3 Hd Wd 4 (grad_out).  The same model is called back to back, so the surviving rows may
be served from the Infinity Cache.  One JSON line per n_tex; the outputs of the three forms are compared first."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from msmd_amd import ops  # noqa: E402
from msmd_amd.utils.flame import FLAMETex  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X specification
R = 512 * 512 * 3


def torch_ref(mean, basis, texcode):
    bs = texcode.shape[0]
    texcode = texcode[:1]
    tex = mean + (basis * texcode[:, None, :]).sum(-1)
    tex = tex.reshape(1, 512, 512, 3).permute(0, 3, 1, 2)
    tex = F.interpolate(tex, [256, 256])
    return tex[:, [2, 1, 0], :, :].repeat(bs, 1, 1, 1)


def surviving_rows(device):
    idx = lambda S, D: torch.clamp(torch.floor(torch.arange(D, dtype=torch.float32) * (np.float32(S) / np.float32(D))).long(), max=S - 1)
    pix = idx(512, 256)[:, None] * 512 + idx(512, 256)[None, :]
    return torch.stack([pix * 3 + (2 - c) for c in range(3)]).reshape(-1).to(device)


def torch_rows(mean, basis, texcode, rows):
    bs = texcode.shape[0]
    tex = mean.reshape(-1)[rows] + basis[0].index_select(0, rows) @ texcode[0]
    return tex.reshape(1, 3, 256, 256).repeat(bs, 1, 1, 1)


def batch_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, seconds):
    """{name: median per-call ms}: warm-up, a batch size that fills ~20 ms per form, then the forms in turn."""
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
    return {n: statistics.median(v) for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_tex", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--bs", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_flametex needs an MI355X"
    dev = torch.device("cuda:0")
    rows = surviving_rows(dev)
    lines = []
    for n_tex in a.n_tex:
        zeros = dict(MU=np.zeros(R, np.float32), PC=np.zeros((R, n_tex), np.float32))
        m = FLAMETex(SimpleNamespace(tex_type="BFM", n_tex=n_tex, tex_asset=zeros)).to(dev)
        gen = torch.Generator(device=dev).manual_seed(n_tex)
        m.texture_mean.copy_(torch.rand(m.texture_mean.shape, device=dev, generator=gen))
        m.texture_basis.copy_(torch.rand(m.texture_basis.shape, device=dev, generator=gen) * 2 - 1)
        code = torch.randn(a.bs, n_tex, device=dev, generator=gen).requires_grad_(True)
        g = torch.randn(a.bs, 3, 256, 256, device=dev, generator=gen)
        mean, basis = m.texture_mean, m.texture_basis
        fwd = {"hip": lambda: m(code), "torch_ref": lambda: torch_ref(mean, basis, code),
               "torch_rows": lambda: torch_rows(mean, basis, code, rows)}
        outs = {k: f() for k, f in fwd.items()}
        grads = {k: torch.autograd.grad(o, code, g, retain_graph=True)[0] for k, o in outs.items()}
        diff = {k: float((outs[k] - outs["hip"]).detach().abs().max()) for k in ("torch_ref", "torch_rows")}
        gdiff = {k: float(((grads[k] - grads["hip"]).abs() / grads["hip"].abs().clamp_min(1.0)).max()) for k in ("torch_ref", "torch_rows")}
        # the launchers alone (ops.flametex_*: output and workspace allocation + the launches, no autograd node) ride along
        flat_mean, flat_basis, code0 = mean.reshape(-1), basis.reshape(-1, n_tex), code[0].detach().contiguous()
        with torch.no_grad():
            f_ms = alternate(dict(fwd, hip_launcher=lambda: ops.flametex_forward(flat_mean, flat_basis, code0, a.bs)), a.seconds)
        bwd = {k: (lambda o=o: torch.autograd.grad(o, code, g, retain_graph=True)) for k, o in outs.items()}
        b_ms = alternate(dict(bwd, hip_launcher=lambda: ops.flametex_backward(flat_basis, g)), a.seconds)
        n_out = 3 * 256 * 256
        f_bytes = n_out * n_tex * 4 + n_out * 4 + a.bs * n_out * 4
        b_bytes = n_out * n_tex * 4 + a.bs * n_out * 4
        line = dict(op="flametex", device=torch.cuda.get_device_name(0), n_tex=n_tex, bs=a.bs,
                    fwd_ms={k: round(v, 5) for k, v in f_ms.items()}, bwd_ms={k: round(v, 5) for k, v in b_ms.items()},
                    fwd_speedup_vs_torch_ref=round(f_ms["torch_ref"] / f_ms["hip"], 2),
                    fwd_speedup_vs_torch_rows=round(f_ms["torch_rows"] / f_ms["hip"], 2),
                    bwd_speedup_vs_torch_ref=round(b_ms["torch_ref"] / b_ms["hip"], 2),
                    bwd_speedup_vs_torch_rows=round(b_ms["torch_rows"] / b_ms["hip"], 2),
                    fwd_GBps=round(f_bytes / f_ms["hip_launcher"] / 1e6, 1), bwd_GBps=round(b_bytes / b_ms["hip_launcher"] / 1e6, 1),
                    fwd_share_of_8TBps=round(f_bytes / (f_ms["hip_launcher"] * 1e-3) / HBM_PEAK, 4),
                    bwd_share_of_8TBps=round(b_bytes / (b_ms["hip_launcher"] * 1e-3) / HBM_PEAK, 4),
                    fwd_max_abs_diff=diff, bwd_max_rel_diff=gdiff,
                    not_slower=bool(f_ms["hip"] <= min(f_ms["torch_ref"], f_ms["torch_rows"])
                                    and b_ms["hip"] <= min(b_ms["torch_ref"], b_ms["torch_rows"])))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del m, outs, grads, fwd
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
