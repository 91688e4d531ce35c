"""Bandwidth of the rotation-conversion backward kernels and the landmark scatter, next to their forward kernels in the same run.

    timeout 300 python tools/bench_rotation_bwd.py [--items 4194304] [--frames 25600] [--reps 9]

HIP events around single launches, 3 warm-up launches, median of --reps (>= 5).  GB/s on the algorithmic bytes:
forward 4 n (in_w + in2_w + out_w); backward 4 n (2 in_w + 2 in2_w + out_w) (inputs and the upstream gradient read, input
gradients written); landmarks backward 4 B (3 L + 3 V) (+ the tables, cache resident).  One JSON line per op."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from msmd_amd import _lib, ops, synth  # noqa: E402

OPS = {"q2m": (0, 4, 0, 9), "m2q": (1, 9, 0, 4), "aa2m": (4, 3, 0, 9), "m2e": (10, 9, 0, 3)}


def timed(fn, reps):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 22)
    ap.add_argument("--frames", type=int, default=25600)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    reps = max(5, a.reps)
    lib = _lib.load()
    n, p, st = a.items, ops._p, ops._stream
    q = torch.randn(n, 4, device="cuda")
    q = q / q.norm(dim=1, keepdim=True)
    R = torch.empty(n, 9, device="cuda")
    _lib.check(lib.msmd_rotation_convert(0, p(q), None, p(R), n, 0, st()), "q2m")
    aa = torch.randn(n, 3, device="cuda")
    inputs = {"q2m": q, "m2q": R, "aa2m": aa, "m2e": R}
    for name, (op, iw, i2w, ow) in OPS.items():
        x = inputs[name]
        out, g, gx = torch.empty(n, ow, device="cuda"), torch.randn(n, ow, device="cuda"), torch.empty(n, iw, device="cuda")
        conv = 0 | (1 << 2) | (2 << 4)
        f_ms = timed(lambda: _lib.check(lib.msmd_rotation_convert(op, p(x), None, p(out), n, conv, st()), name), reps)
        b_ms = timed(lambda: _lib.check(lib.msmd_rotation_convert_bwd(op, p(x), None, p(g), p(gx), None, n, conv, st()), name), reps)
        f_gbs = 4.0 * n * (iw + ow) / f_ms / 1e6
        b_gbs = 4.0 * n * (2 * iw + ow) / b_ms / 1e6
        print(json.dumps(dict(op=name, items=n, fwd_ms=round(f_ms, 4), fwd_GBps=round(f_gbs, 1), bwd_ms=round(b_ms, 4),
                              bwd_GBps=round(b_gbs, 1), bwd_over_fwd=round(b_gbs / f_gbs, 3))))
    # landmarks: FLAME's 68 full landmarks on 5023 vertices
    asset = synth.flame_asset()
    B, V, L = a.frames, 5023, 68
    faces = torch.from_numpy(asset["f"].astype("int32")).cuda()
    idx = torch.from_numpy(asset["lmk"]["full_lmk_faces_idx"].astype("int32")).cuda().reshape(1, L)
    bary = torch.from_numpy(asset["lmk"]["full_lmk_bary_coords"]).cuda().reshape(1, L, 3)
    verts, gl = torch.randn(B, V, 3, device="cuda"), torch.randn(B, L, 3, device="cuda")
    gv = torch.empty(B, V, 3, device="cuda")
    f_ms = timed(lambda: ops.landmarks(verts, faces, idx, bary), reps)
    b_ms = timed(lambda: ops.landmarks_bwd(gl, faces, idx, bary, V, None), reps)
    acc_ms = timed(lambda: ops.landmarks_bwd(gl, faces, idx, bary, V, gv), reps)
    print(json.dumps(dict(op="landmarks", frames=B, fwd_ms=round(f_ms, 4), bwd_ms=round(b_ms, 4),
                          bwd_GBps=round(4.0 * B * 3 * (L + V) / b_ms / 1e6, 1), bwd_accumulate_ms=round(acc_ms, 4))))


if __name__ == "__main__":
    main()
