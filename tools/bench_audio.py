"""Times the two audio front-end entry points (csrc/audio_io.hip) on 32 stereo int16 clips of 10 s, at 44.1 kHz and at 48 kHz.

HIP events around each C entry point called on preallocated buffers (msmd_audio_znorm is two launches: per-clip statistics,
then the normalisation), median of 9 after 3 warm-up rounds.  Prints one line per (rate, entry point) with the time and the
achieved bytes/s against the algorithmic bytes of the pair, PCM in plus fp32 out twice (the resampler writes the output once,
the z-norm reads it and writes it once more; each entry point is charged its own share), and the pair's seconds of audio per
second.  The staging copy is not timed.  Needs an MI355X; there is no CPU path.

    python tools/bench_audio.py [--out profiles/r09_audio.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from msmd_amd import _lib, ops  # noqa: E402
from msmd_amd.utils import audio  # noqa: E402


def timed(fn, reps=9, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_audio needs an MI355X"
    dev = torch.device("cuda:0")
    B, C = args.clips, 2
    lines = []
    for rate in (44100, 48000):
        fb = audio.filter_bank(rate)
        frames = int(round(args.seconds * rate))
        n_out = audio.output_length(frames, fb.L, fb.M)
        pcm = torch.from_numpy(np.random.default_rng(rate).integers(-32768, 32768, size=B * frames * C).astype(np.int16)).to(dev)
        desc = np.array([[b * frames * C, frames, C, b * n_out, n_out] for b in range(B)], np.int64)
        desc_dev = torch.from_numpy(desc).to(dev)
        bank = torch.from_numpy(fb.table.copy()).to(dev)
        out, partials = ops.resample_audio(pcm, desc_dev, desc, bank, fb.L, fb.M)     # checks the descriptors once; allocates
        kept = out.clone()
        stats = torch.empty(B, 2, device=dev, dtype=torch.float64)
        lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
        # the timed calls are the C entry points on preallocated buffers: no validation, no allocation between the events

        def resample():
            _lib.check(lib.msmd_audio_resample(pcm.data_ptr(), pcm.numel(), 1, desc_dev.data_ptr(), B, n_out, fb.L, fb.M, fb.taps,
                                               bank.data_ptr(), out.data_ptr(), out.numel(), partials.data_ptr(), st), "resample")

        def znorm():     # in place: every timed call normalises the last one's result again, which costs the same
            _lib.check(lib.msmd_audio_znorm(out.data_ptr(), out.numel(), desc_dev.data_ptr(), B, n_out, partials.data_ptr(),
                                            stats.data_ptr(), st), "znorm")

        t_r, t_z = timed(resample), timed(znorm)
        resample()
        assert torch.equal(out, kept), "the same bits on every run"
        b_r, b_z = pcm.numel() * 2 + B * n_out * 4, 2 * B * n_out * 4
        for name, (med, lo, hi), nbytes in (("msmd_audio_resample", t_r, b_r), ("msmd_audio_znorm", t_z, b_z)):
            lines.append(f"{name} {B} clips x {args.seconds:g} s x {C} ch int16 {rate} Hz (L/M = {fb.L}/{fb.M}, {fb.taps} taps): median "
                         f"{med:.4f} ms (min {lo:.4f}, max {hi:.4f}, 9 runs), {nbytes / med * 1e3 / 1e9:.2f} GB/s of {nbytes / 1e6:.1f} MB")
        both = t_r[0] + t_z[0]
        lines.append(f"both entry points (three launches) {rate} Hz: {both:.4f} ms, {B * args.seconds / both * 1e3:.0f} s of audio per second, "
                     f"{(b_r + b_z - B * n_out * 4) / both * 1e3 / 1e9:.2f} GB/s of the pair's algorithmic bytes (PCM in + fp32 out twice)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
