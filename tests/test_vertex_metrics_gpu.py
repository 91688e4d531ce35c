"""Vertex-space metrics on the MI355X: csrc/vertex_metrics.hip through ops.vertex_frame_errors / ops.vertex_motion_moments_ and
utils/metrics.VertexMetrics, against the float64 restatement and the exact rational truth of tests/vertex_metrics_ref.py, within
the bounds derived in that module's docstring (tests/test_vertex_metrics_cpu.py shows that they hold for a faithful emulation of
the kernels on these very inputs and that they catch the planted mutants).  Every figure is printed before it is asserted."""
import json
import os
import pickle as pkl
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vertex_metrics_ref as VR
from msmd_amd import _lib, ops, synth
from msmd_amd.utils import metrics as M
from msmd_amd.utils.common import get_coef_dict
from msmd_amd.utils.flame import FLAME, FLAMEConfig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = list(VR.MOMENT_CLIPS)


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dt is None else t.to(dt)).to(DEV)


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def same_result(a, b):
    """Two result dicts hold the same bits (a NaN equals itself)."""
    flat = lambda r: np.array([[c[k] for k in ("lve", "mve", "max_ve", "rmse", "fdd", "frames")] for c in r["clips"] + [r["all"]]], np.float64)
    return np.array_equal(bits(flat(a)), bits(flat(b)))


@pytest.mark.parametrize("V", VR.FRAME_V)
def test_frame_table_against_the_restatement(V):
    worst_all = 0.0
    for half in (False, True):
        for n in (1, 3):
            for kind in VR.LIP_MASKS:
                for plant in ("first", "last"):
                    pred, gt, lips, region = VR.frame_case(V, n, half, kind, plant)
                    got = ops.vertex_frame_errors(dev(pred), dev(gt), dev(region)).cpu().numpy()
                    want = VR.frame_table(pred, gt, lips)
                    ok, worst = VR.table_ok(got, want, V)
                    worst_all = max(worst_all, worst)
                    exact = np.array_equal(bits(got), bits(VR.emulate_frame_table(pred, gt, region)))
                    if not ok or not exact:
                        print(f"V {V} fp16 {half} n {n} lips {kind} planted {plant}: worst error / bound {worst:.3e}, bits equal to the emulator: {exact}")
                    assert got.shape == (n, 4) and got.dtype == np.float64
                    assert ok
                    if (0 if plant == "first" else V - 1) not in lips:
                        assert (got[:, 0] < 0.5 * got[:, 2] ** 2).all()
    print(f"V {V}: worst error / bound over fp32 / fp16, n 1 / 3, four masks, two plants: {worst_all:.3e}")


@pytest.mark.parametrize("V,half", [(65, False), (257, True), (5023, False)])
def test_nan_propagation(V, half):
    pred0, gt0, lips, region = (np.array(x) for x in VR.frame_case(V, 3, half, "third", "last"))
    base = ops.vertex_frame_errors(dev(pred0), dev(gt0), dev(region)).cpu().numpy()
    off_lip, last_lip = 1, int(lips[-1])
    for at, value, cols in ((off_lip, np.nan, [1, 2, 3]), (last_lip, np.nan, [0, 1, 2, 3]), (last_lip, np.inf, [0, 1, 2, 3])):
        pred, gt = pred0.copy(), gt0.copy()
        pred[1, at, 2] = value
        if np.isinf(value):
            gt[1, at, 2] = value
        got = ops.vertex_frame_errors(dev(pred), dev(gt), dev(region)).cpu().numpy()
        print(f"V {V} fp16 {half}: {value} at vertex {at} of frame 1 -> row {got[1].tolist()}")
        assert np.isnan(got[1, cols]).all() and np.isnan(got[1]).sum() == len(cols)
        assert np.array_equal(bits(got[[0, 2]]), bits(base[[0, 2]]))
        assert VR.table_ok(got, VR.frame_table(pred, gt, lips), V)[0]


def run_moments(pred, gt, upper, template, cuts):
    """state after the chunks [cuts[i], cuts[i + 1]) through ops.vertex_motion_moments_."""
    state = torch.zeros(len(OFF) - 1, len(upper), 2, 3, device=DEV, dtype=torch.float64)
    p, g, o, u, t = dev(pred), dev(gt), dev(np.array(OFF, np.int64)), dev(upper), dev(template)
    for a, b in zip(cuts[:-1], cuts[1:]):
        ops.vertex_motion_moments_(state, p[a:b], g[a:b], a, o, u, t)
    return state.cpu().numpy()


@pytest.mark.parametrize("U,per_clip,half", [(u, pc, False) for u in VR.MOMENT_U for pc in (False, True)] + [(65, False, True)])
def test_moments_against_the_exact_truth(U, per_clip, half):
    pred, gt, upper, template = VR.moments_case(U, per_clip, half)
    state = run_moments(pred, gt, upper, template, [0, OFF[-1]])
    ok, worst = VR.check_state(state, VR.moments_exact_case(U, per_clip, half))
    ok_std, worst_std = VR.check_std(VR.state_std(state), VR.moments_exact_case(U, per_clip, half))
    exact = np.array_equal(bits(state), bits(VR.emulate_moments(pred, gt, OFF, upper, template)))
    print(f"U {U}, per-clip template {per_clip}, fp16 {half}: worst error / bound {worst:.3e} (count, mean, M2), {worst_std:.3e} (std); "
          f"bits equal to the emulator: {exact}")
    assert ok and ok_std


def test_chunking_and_batch_independence_bit_for_bit():
    pred, gt, upper, template = VR.moments_case(65, True)
    n = OFF[-1]
    cuts = {"one chunk": [0, n], "chunks of 7": list(range(0, n, 7)) + [n], "chunks of 1": list(range(n + 1))}
    states = {k: run_moments(pred, gt, upper, template, c) for k, c in cuts.items()}
    lips = np.arange(5, 60)
    p, g = dev(pred), dev(gt)
    results = {}
    for k, c in cuts.items():
        vm = M.VertexMetrics(OFF, VR.MOMENT_V, lips, upper, template, DEV)
        for a, b in zip(c[:-1], c[1:]):
            vm.update(p[a:b], g[a:b])
        results[k] = vm.result()
        assert np.array_equal(bits(vm.state.cpu().numpy()), bits(states[k]))
    for k in cuts:
        same = np.array_equal(bits(states[k]), bits(states["one chunk"])), same_result(results[k], results["one chunk"])
        print(f"{k}: state and result bits equal to one chunk's: {same}")
        assert all(same)
    again = M.vertex_metrics(p, g, OFF, lips, upper, template)
    assert same_result(again, results["one chunk"])
    for k, (a, b) in enumerate(zip(OFF[:-1], OFF[1:])):
        alone = M.vertex_metrics(p[a:b].contiguous(), g[a:b].contiguous(), [0, b - a], lips, upper, template[k])
        eq = same_result({"clips": alone["clips"], "all": alone["clips"][0]}, {"clips": [again["clips"][k]], "all": again["clips"][k]})
        print(f"clip {k} ({b - a} frames) alone against inside the batch: bits equal {eq}")
        assert eq
    # and the numbers themselves: the restatement within the frame table's bounds, fdd within the bound from the exact moments
    want = VR.metrics(pred, gt, OFF, lips, upper, template)
    fb = VR.fdd_exact_and_bound(VR.moments_exact_case(65, True))
    for c, w, (fe, bound) in zip(again["clips"], want["clips"], fb):
        for key in ("lve", "mve", "max_ve", "rmse"):
            assert abs(c[key] - w[key]) <= (VR.MOMENT_V + 8) * VR.U52 * abs(w[key]), key
        print(f"clip of {c['frames']} frames: fdd {c['fdd']:.9e}, exact {fe:.9e}, bound {bound:.3e}")
        assert c["frames"] == w["frames"] and abs(c["fdd"] - fe) <= bound
    assert again["clips"][3]["fdd"] == 0.0
    assert again["all"]["max_ve"] == max(c["max_ve"] for c in again["clips"]) and again["all"]["frames"] == n


def test_c_abi_guards_and_clamp():
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    pred, gt, upper, template = VR.moments_case(65, False)
    n, V, U, C = OFF[-1], VR.MOMENT_V, 65, len(OFF) - 1
    p, g, o, t = dev(pred), dev(gt), dev(np.array(OFF, np.int64)), dev(template)
    region = dev(np.ones(V, np.uint8))
    SENT = -7.25
    out = torch.full((n * 4 + 64,), SENT, device=DEV, dtype=torch.float64)
    frame = lambda n_, V_, dt=ops.F32: lib.msmd_vertex_frame_errors(p.data_ptr(), g.data_ptr(), region.data_ptr(), out.data_ptr(), n_, V_, dt, st)
    assert frame(-1, V) == 1 and frame(n, 0) == 1 and frame(n, -3) == 1 and frame(n, V, ops.BF16) == 1
    assert frame(0, V) == 0
    torch.cuda.synchronize()
    assert (out == SENT).all(), "n = 0 wrote something"
    assert frame(n, V) == 0
    torch.cuda.synchronize()
    assert (out[n * 4:] == SENT).all() and (out[:n * 4] != SENT).all()
    wild = upper.copy()
    wild[0], wild[-1] = -1, V
    state = torch.full((C * U * 6 + 64,), SENT, device=DEV, dtype=torch.float64)
    state[:C * U * 6] = 0
    u = dev(wild)
    mom = lambda n_, U_, V_, C_=C, f0=0, dt=ops.F32: lib.msmd_vertex_motion_moments(
        p.data_ptr(), g.data_ptr(), f0, n_, o.data_ptr(), C_, u.data_ptr(), U_, t.data_ptr(), 0, state.data_ptr(), V_, dt, st)
    assert mom(-1, U, V) == 1 and mom(n, 0, V) == 1 and mom(n, -2, V) == 1 and mom(n, U, 0) == 1 and mom(n, U, V, 0) == 1
    assert mom(n, U, V, C, -1) == 1 and mom(n, U, V, C, 0, ops.BF16) == 1
    assert mom(0, U, V) == 0
    torch.cuda.synchronize()
    assert (state[:C * U * 6] == 0).all() and (state[C * U * 6:] == SENT).all(), "n_chunk = 0 wrote something"
    assert mom(n, U, V) == 0
    torch.cuda.synchronize()
    got = state.cpu().numpy()
    assert (got[C * U * 6:] == SENT).all()
    ok, worst = VR.check_state(got[:C * U * 6].reshape(C, U, 2, 3), VR.exact_moments(pred, gt, OFF, wild, template))
    print(f"upper_idx holding -1 and V: worst error / bound against the truth on the clamped list {worst:.3e}")
    assert ok
    with pytest.raises(TypeError):
        ops.vertex_frame_errors(p, g.half(), region)
    with pytest.raises(TypeError):
        ops.vertex_frame_errors(p.double(), g.double(), region)
    with pytest.raises(TypeError):
        ops.vertex_frame_errors(p[:, :, :2], g[:, :, :2], region)
    with pytest.raises(TypeError):
        ops.vertex_motion_moments_(torch.zeros(C, U, 2, 2, device=DEV, dtype=torch.float64), p, g, 0, o, u, t)
    with pytest.raises(TypeError):
        ops.vertex_motion_moments_(torch.zeros(C, U, 2, 3, device=DEV, dtype=torch.float64), p, g, 0, o, u, t[:-1].contiguous())
    assert tuple(ops.vertex_frame_errors(p[:0], g[:0], region).shape) == (0, 4)


def test_end_to_end_with_flame_and_the_command_line(tmp_path):
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = synth.flame_asset()
    fl = FLAME(cfg).to(DEV)
    g = np.random.default_rng(5)
    T, off = 11, [0, 4, 11]
    gt_coef = dev(np.concatenate([0.8 * g.standard_normal((T, 50)), 0.2 * g.standard_normal((T, 3)), 0.2 * g.random((T, 1))], 1).astype(np.float32))
    pred_coef = gt_coef + dev((0.05 * g.standard_normal((T, 54))).astype(np.float32))
    shape = dev((0.5 * g.standard_normal((2, 100))).astype(np.float32))
    lips, upper = np.arange(1000, 1200), np.arange(3000, 4000, 3)
    zero = M.evaluate_coeffs(gt_coef, gt_coef, shape, fl, None, off, lips, upper)
    print("a track against itself:", zero["all"])
    for c in zero["clips"] + [zero["all"]]:
        assert all(c[k] == 0.0 for k in ("lve", "mve", "max_ve", "rmse", "fdd"))
    res = M.evaluate_coeffs(pred_coef, gt_coef, shape, fl, None, off, lips, upper, chunk=512)
    res3 = M.evaluate_coeffs(pred_coef, gt_coef, shape, fl, None, off, lips, upper, chunk=3)
    # the same FLAME calls: one shape per call, a clip at a time
    verts = []
    for coef in (pred_coef, gt_coef):
        parts = []
        for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
            c = get_coef_dict(coef[a:b], shape[k:k + 1].expand(b - a, -1), None, with_global_pose=False)
            parts.append(fl(c["shape"], c["exp"], c["pose"], return_lm2d=False, return_lm3d=False)[0].float())
        verts.append(torch.cat(parts, 0).contiguous())
    template = torch.cat([fl(shape[k:k + 1], torch.zeros(1, 50, device=DEV), torch.zeros(1, 6, device=DEV), return_lm2d=False,
                             return_lm3d=False)[0].float() for k in range(2)], 0).contiguous()
    own = M.vertex_metrics(verts[0], verts[1], off, lips, upper, template)
    print("perturbed track:", res["all"])
    assert same_result(res, own) and same_result(res, res3)
    assert res["all"]["lve"] > 0 and res["all"]["max_ve"] > 0 and [c["frames"] for c in res["clips"]] == [4, 7]
    # the command line, in a child process: one clip, the zero shape, FLAME read from files
    asset = {k: v for k, v in cfg.asset.items() if k != "lmk"}
    with open(tmp_path / "flame.pkl", "wb") as f:
        pkl.dump(asset, f)
    np.save(tmp_path / "lmk.npy", np.array(cfg.asset["lmk"], dtype=object), allow_pickle=True)
    for name, val in (("pe", pred_coef[:, :50]), ("pr", pred_coef[:, 50:53]), ("ge", gt_coef[:, :50]), ("gr", gt_coef[:, 50:53])):
        with open(tmp_path / f"{name}.pkl", "wb") as f:
            pkl.dump(val.cpu().numpy(), f)
    with open(tmp_path / "masks.pkl", "wb") as f:
        pkl.dump(dict(lips=lips, forehead=upper[:100], eye_region=upper[90:]), f)
    r = subprocess.run([sys.executable, "-m", "msmd_amd.utils.metrics", "--pred_exp", str(tmp_path / "pe.pkl"), "--pred_rot",
                        str(tmp_path / "pr.pkl"), "--gt_exp", str(tmp_path / "ge.pkl"), "--gt_rot", str(tmp_path / "gr.pkl"),
                        "--regions", str(tmp_path / "masks.pkl"), "--flame_model_path", str(tmp_path / "flame.pkl"),
                        "--flame_lmk_embedding_path", str(tmp_path / "lmk.npy"), "--out", str(tmp_path / "metrics.json")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    with open(tmp_path / "metrics.json") as f:
        written = json.load(f)
    closed_jaw = lambda c: torch.cat([c[:, :53], torch.zeros_like(c[:, :1])], 1)
    here = M.evaluate_coeffs(closed_jaw(pred_coef), closed_jaw(gt_coef), torch.zeros(1, 100, device=DEV), fl, None, [0, T], lips, upper)
    assert same_result(written, here) and written["all"]["frames"] == T
