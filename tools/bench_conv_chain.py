"""conv1-4 of the feature extractor at the forward step's shape (32 clips of 64 000 samples: 32 x 12 799 x 512 into the stack):
four per-layer launches against ONE chained launch (ops.conv_chain), in each hand-over form and ticket size.

    python tools/bench_conv_chain.py [--reps 30] [--rounds 5] [--dtypes bf16 fp16]

First every variant's four outputs are checked bit for bit against the per-layer launches and its status word is read.  Then the
variants alternate inside each round (HIP events around `reps` back-to-back calls of one variant) so that clock and
temperature drift hits all of them alike; the table gives the median over rounds and the min-max range, in us per stack."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from msmd_amd import ops, shapes

B, SAMPLES, C = 32, 64000, 512
KERNELS, STRIDES = shapes.CONV_KERNEL[1:5], shapes.CONV_STRIDE[1:5]
VARIANTS = [
    ("per-layer", None),
    ("chain write-through, tile tickets", 0),
    ("chain write-through, row-block tickets", ops.CONV_CHAIN_ROW_BLOCK_TICKETS),
    ("chain release, tile tickets", ops.CONV_CHAIN_RELEASE),
    ("chain release, row-block tickets", ops.CONV_CHAIN_RELEASE | ops.CONV_CHAIN_ROW_BLOCK_TICKETS),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp16"])
    a = ap.parse_args()
    T0 = (SAMPLES - shapes.CONV_KERNEL[0]) // shapes.CONV_STRIDE[0] + 1
    for name in a.dtypes:
        dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[name]
        g = torch.Generator(device="cpu").manual_seed(1)
        x = torch.randn(B, T0, C, generator=g).to("cuda", dtype)
        ws = [(torch.randn(C, k * C, generator=g) / (k * C) ** 0.5).to("cuda", dtype) for k in KERNELS]
        bs = [(0.1 * torch.randn(C, generator=g)).to("cuda") for _ in KERNELS]

        def per_layer():
            y, outs = x, []
            for w, b, k, s in zip(ws, bs, KERNELS, STRIDES):
                y = ops.conv1d_cl(y, w, b, kernel=k, stride=s, act=ops.ACT_GELU)
                outs.append(y)
            return outs

        ref = per_layer()
        outs = [torch.empty_like(r) for r in ref]
        workspace = torch.empty(1 << 16, device="cuda", dtype=torch.uint8)
        runs = {}
        for label, flags in VARIANTS:
            if flags is None:
                runs[label] = per_layer
                continue
            run = lambda flags=flags: ops.conv_chain(x, ws, bs, kernels=KERNELS, strides=STRIDES, act=ops.ACT_GELU, flags=flags,
                                                     outs=outs, workspace=workspace)
            for o in outs:
                o.zero_()
            assert run() is not None, "the library declined the bench shape"
            status = ops.conv_chain_status(workspace)
            equal = [bool(torch.equal(o, r)) for o, r in zip(outs, ref)]
            print(f"{name} {label}: status {status}, outputs equal to the per-layer launches: {equal}", flush=True)
            assert status == 0 and all(equal)
            runs[label] = run
        times = {label: [] for label in runs}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.rounds):
            for label, run in runs.items():
                run()
                e0.record()
                for _ in range(a.reps):
                    run()
                e1.record()
                e1.synchronize()
                times[label].append(1e3 * e0.elapsed_time(e1) / a.reps)
        for label, t in times.items():
            print(f"{name} {label:42s} median {statistics.median(t):8.1f} us   range {min(t):8.1f} - {max(t):8.1f}", flush=True)
        print(json.dumps({"dtype": name, "reps": a.reps, "rounds": a.rounds,
                          "us": {label: [round(v, 2) for v in t] for label, t in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
