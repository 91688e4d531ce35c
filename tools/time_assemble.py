"""Time the track resampler against the reference's host path on the same machine.

    python tools/time_assemble.py [--clips 256] [--repeats 20] [--cpu_repeats 3]

The work: `--clips` clips, F uniform in [75, 1200] frames, C = 53 channels (50 expression + 3 head), frame rate drawn from
23.976 / 25 / 29.97 / 60, every clip resampled to 30 fps -- once plain, once through the (5, 2) Savitzky-Golay filter.
GPU: one `ops.track_resample` call for the whole list (the offsets' copy and both launches), device events on the stream around
each call after a warm-up, the median of `--repeats` calls.  The tracks are already on the device and already concatenated.
CPU: scipy.signal.resample (after savgol_filter for the filtered run) per clip in float64, the reference's Step 5 / Step 3 calls,
under the process's thread limit (OMP_NUM_THREADS; 16 where none is set), the median of `--cpu_repeats` passes.
Prints one JSON line.  Needs the MI355X: there is no fallback."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import signal  # noqa: E402

from msmd_amd import ops  # noqa: E402
from msmd_amd.utils.assemble import resampled_length  # noqa: E402
from msmd_amd.utils.head_pose import savgol_table  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--cpu_repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_assemble.py needs an MI355X"
    torch.set_num_threads(int(os.environ["OMP_NUM_THREADS"]))
    rng = np.random.default_rng(0)
    C = 53
    F = rng.integers(75, 1201, args.clips)
    fps = rng.choice([23.976, 25.0, 29.97, 60.0], args.clips)
    M = [resampled_length(int(f), float(r)) for f, r in zip(F, fps)]
    tracks = [rng.standard_normal((int(f), C)).astype(np.float32) for f in F]
    in_off, out_off = np.concatenate([[0], np.cumsum(F)]).tolist(), np.concatenate([[0], np.cumsum(M)]).tolist()
    x = torch.from_numpy(np.concatenate(tracks, 0)).cuda()
    table = torch.from_numpy(savgol_table(5, 2)).cuda()
    result = dict(device=torch.cuda.get_device_name(0), clips=args.clips, channels=C, frames_in=int(F.sum()), frames_out=int(sum(M)),
                  cpu_threads=int(os.environ["OMP_NUM_THREADS"]), scipy=__import__("scipy").__version__)
    for tag, tab, w in (("plain", None, 0), ("savgol_5_2", table, 5)):
        for _ in range(3):
            y = ops.track_resample(x, in_off, out_off, tab, w)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            y = ops.track_resample(x, in_off, out_off, tab, w)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        cpu = []
        for _ in range(args.cpu_repeats):
            t0 = time.perf_counter()
            ref = [signal.resample(signal.savgol_filter(t.astype(np.float64), 5, 2, axis=0) if w else t.astype(np.float64), m)
                   for t, m in zip(tracks, M)]
            cpu.append((time.perf_counter() - t0) * 1e3)
        err = float(np.abs(y.cpu().numpy() - np.concatenate(ref, 0)).max())
        result[tag] = dict(gpu_ms_median=float(np.median(times)), gpu_ms_min=float(min(times)), gpu_ms_max=float(max(times)),
                           cpu_ms_median=float(np.median(cpu)), max_abs_diff_vs_scipy=err)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
