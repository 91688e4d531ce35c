"""Times frame resizing (ops.resize_frames, csrc/resize.hip) on 256 frames:
  1080 x 1920 x 3 -> 256 x 455      a 1080p clip brought to the render's height
  512 x 512 x 3   -> 256 x 256      a 2x reduction
  256 x 256 x 3   -> 512 x 512      a 2x enlargement
each for `bilinear` and `lanczos`, in three ways:
  fused       one launch, the intermediate rows of a tile in LDS (form="fused")
  two_pass    a horizontal and a vertical launch, the intermediate in HBM (form="two_pass"; its workspace is allocated per call)
  torch       torch.nn.functional.interpolate(antialias=True) on the same frames converted to float NCHW and back to uint8 NHWC,
              the only way to get a resized frame without this module, so the baseline.  It has no lanczos: the lanczos rows are
              timed against its bicubic.  Its bytes are not compared: it is a float operator with another rounding.
HIP events around one call, median of --rounds after one warm-up call.  GB/s counts the source and the destination bytes once;
the share of the HBM peak is against 8.0 TB/s.  The two forms' bytes are compared before anything is printed, and the route's own
choice is named per case.

    python tools/bench_resize.py [--frames 256] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmd_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12
CASES = [((1080, 1920), (256, 455)), ((512, 512), (256, 256)), ((256, 256), (512, 512))]     # (H, W) -> (H, W)


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


def torch_resize(frames, size_hw, mode):
    x = frames.permute(0, 3, 1, 2).float()
    y = torch.nn.functional.interpolate(x, size=size_hw, mode=mode, antialias=True, align_corners=False)
    return y.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    n = args.frames
    lines = [f"resize: {n} frames, 3 channels; {torch.cuda.get_device_name(0)}; median (min .. max) of {args.rounds} calls; "
             f"tile {ops.RESIZE_TILE_H} x {ops.RESIZE_TILE_W}, LDS budget {ops.RESIZE_LDS_BYTES}"]
    for (Hs, Ws), (Hd, Wd) in CASES:
        frames = torch.randint(0, 256, (n, Hs, Ws, 3), device=dev, dtype=torch.uint8, generator=g)
        nbytes = n * 3 * (Hs * Ws + Hd * Wd)
        for f in ("bilinear", "lanczos"):
            yb, yc = ops.resize_tables(Hs, Hd, f)
            span = ops.resize_rows_span(yb[None], Hs, yc.shape[1])
            route = ops.resize_route(3, span, n, Hs, Hd, Wd, ops.resize_tables(Ws, Wd, f)[1].shape[1])
            res = {}
            ways = [("two_pass", lambda: res.__setitem__("two_pass", ops.resize_frames(frames, (Wd, Hd), f, form="two_pass")))]
            if ops.resize_fits(3, span):
                ways.insert(0, ("fused", lambda: res.__setitem__("fused", ops.resize_frames(frames, (Wd, Hd), f, form="fused"))))
            mode = "bilinear" if f == "bilinear" else "bicubic"
            ways.append((f"torch {mode}", lambda: res.__setitem__("torch", torch_resize(frames, (Hd, Wd), mode))))
            times = {tag: timed(fn, args.rounds) for tag, fn in ways}
            if "fused" in res:
                assert torch.equal(res["fused"], res["two_pass"]), "the two forms differ"
            off = (res["two_pass"].int() - res["torch"].int()).abs()
            faster = min((t for t in times if not t.startswith("torch")), key=lambda t: times[t][0])
            lines.append(f"{Hs} x {Ws} -> {Hd} x {Wd} {f}: a tile touches {span} source rows, the route takes {route}, the faster is {faster}; "
                         f"against torch {mode}: {float((off > 1).float().mean()):.4f} of the bytes differ by more than 1, largest {int(off.max())}")
            base = times[f"torch {mode}"][0]
            for tag, (med, lo, hi) in times.items():
                rate = nbytes / (med * 1e-3)
                lines.append(f"    {tag:15s} {med:9.3f} ms ({lo:.3f} .. {hi:.3f})  {rate / 1e9:8.1f} GB/s  {rate / HBM_PEAK:.3f} of the HBM peak"
                             + (f"  {base / med:.2f}x torch" if not tag.startswith("torch") else ""))
            del res
        del frames
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
