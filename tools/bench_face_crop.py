"""Time msmd_face_crop against what a user would write without it, on the same device.

    python tools/bench_face_crop.py [--frames 32] [--repeats 20]

The work: `--frames` frames of 1080 x 1920 and of 720 x 1280, square boxes of 300 and 600 pixels around the frame's centre (each
frame's box offset by a few pixels, so no two frames share a map), outputs of 224 and 256, fp32 and bf16, with and without
the uint8 crop.  One `ops.face_crop` call per measurement (one launch), device events on the stream around each call after a
warm-up, the median of `--repeats` calls; the frames, the inverse maps and the table are already on the device.
The yardstick: `torch.nn.functional.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True)` on the float copy
of the frames, then the channel swap and (x / 255 - mean) / std -- timed twice: with the float copy and the sampling grid
already resident ("sample"), and with both made inside the timed region ("total"), as a loop over clips would have to.
Bytes are counted from the shapes: in, the 3 bytes of every source pixel under the crop's footprint (box * 1.15 squared, clipped
to the frame); out, 3 S^2 elements per frame plus 3 S^2 bytes with the uint8 crop.  The fraction of HBM is given against
a copy measured in this run (1 GiB device to device, read + write) and against bench.py's PEAK_HBM_GBS.
Prints one JSON line.  No threshold is asserted.  Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from msmd_amd import ops  # noqa: E402
from msmd_amd.utils import face_crop as FC  # noqa: E402

PEAK_HBM_GBS = 8000.0           # bench.py's figure for the MI355X


def timed(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def copy_gbs(repeats):
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    med, _, _ = timed(lambda: dst.copy_(src), repeats)
    return 2 * src.numel() / med / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_face_crop.py needs an MI355X"
    n = args.frames
    live = copy_gbs(args.repeats)
    result = dict(device=torch.cuda.get_device_name(0), frames=n, copy_gb_per_s=round(live, 1), peak_hbm_gb_per_s=PEAK_HBM_GBS, rows=[])
    table = FC.normalise_table().cuda()
    mean = torch.tensor(FC.IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(FC.IMAGENET_STD, device="cuda").view(1, 3, 1, 1)
    rng = np.random.default_rng(0)
    for H, W in ((1080, 1920), (720, 1280)):
        frames = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda()
        as_float = frames.permute(0, 3, 1, 2).float()
        for box in (300, 600):
            boxes = np.array([[box, box, W // 2 + 3 * (f % 7) - 9, H // 2 + 2 * (f % 5) - 4] for f in range(n)], np.int32)
            side = min(box * 1.15, H)
            for S in (224, 256):
                trans = FC.crop_transforms(boxes, S)
                inv_host = FC.invert_transforms(trans)
                inv = torch.from_numpy(inv_host).cuda()
                inv32 = inv.float()

                def grid():
                    j = torch.arange(S, device="cuda", dtype=torch.float32)
                    ones = torch.ones(S, S, device="cuda")
                    pix = torch.stack([j[None, :] * ones, j[:, None] * ones, ones], -1)                  # (S, S, 3) as j, i, 1
                    src = torch.einsum("fkc,ijc->fijk", inv32, pix)                                     # (F, S, S, 2) as sx, sy
                    return src * torch.tensor([2.0 / (W - 1), 2.0 / (H - 1)], device="cuda") - 1.0
                g = grid()

                def sample(x=as_float, gr=g):
                    y = F.grid_sample(x, gr, mode="bilinear", padding_mode="zeros", align_corners=True)
                    return (y.flip(1) / 255 - mean) / std
                t_sample = timed(sample, args.repeats)
                t_total = timed(lambda: sample(frames.permute(0, 3, 1, 2).float(), grid()), args.repeats)
                # the two paths agree to the fp32 path's own error (grid_sample rounds coordinates and weights in fp32)
                ours = ops.face_crop(frames, inv, table, S)[0]
                diff = float((ours - sample()).abs().max())
                for dtype in (torch.float32, torch.bfloat16):
                    for u8 in (False, True):
                        t = timed(lambda: ops.face_crop(frames, inv, table, S, dtype=dtype, want_uint8=u8), args.repeats)
                        nbytes = n * (side * side * 3 + S * S * 3 * (dtype.itemsize + (1 if u8 else 0)))
                        gbs = nbytes / t[0] / 1e6
                        result["rows"].append(dict(
                            frame=f"{H}x{W}", box=box, out=S, dtype=str(dtype).replace("torch.", ""), uint8=u8,
                            us_median=round(t[0] * 1e3, 1), us_min=round(t[1] * 1e3, 1), us_max=round(t[2] * 1e3, 1),
                            mbytes=round(nbytes / 1e6, 1), gb_per_s=round(gbs, 1), frac_of_copy=round(gbs / live, 4),
                            frac_of_peak=round(gbs / PEAK_HBM_GBS, 4), grid_sample_us=round(t_sample[0] * 1e3, 1),
                            grid_sample_total_us=round(t_total[0] * 1e3, 1), max_abs_diff_vs_grid_sample=round(diff, 4)))
        del frames, as_float
    print(json.dumps(result))


if __name__ == "__main__":
    main()
