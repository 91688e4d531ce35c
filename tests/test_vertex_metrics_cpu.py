"""Vertex-space metrics without a GPU: the float64 restatement (tests/vertex_metrics_ref.py) against a literal transcription of the
published LVE / FDD code, the numpy emulators of the two kernels against the exact truth within the derived bounds -- with planted
mutants that the bounds must catch -- and the refusals of utils/metrics.py that need no device."""
import pickle as pkl

import numpy as np
import pytest
import torch

import vertex_metrics_ref as VR
from msmd_amd.utils import metrics as M


def test_restatement_against_the_published_formulas():
    """CodeTalker's cal_metric.py, transcribed: LVE = mean over frames of the max over the mouth map of the summed squared
    differences; FDD = mean over the upper map of the std over time of the summed squared displacement, ground truth minus
    prediction."""
    g = np.random.default_rng(3)
    F, V = 17, 40
    template = g.standard_normal((V, 3)).astype(np.float32)
    vertices_gt = (template + 0.1 * g.standard_normal((F, V, 3))).astype(np.float32)
    vertices_pred = (vertices_gt + 0.02 * g.standard_normal((F, V, 3))).astype(np.float32)
    mouth_map, upper_map = [3, 4, 9, 30], [0, 1, 2, 12, 39]
    a, b, t = vertices_gt.astype(np.float64), vertices_pred.astype(np.float64), template.astype(np.float64)
    L2_dis_mouth_max = np.array([np.square(a[:, v, :] - b[:, v, :]) for v in mouth_map])
    L2_dis_mouth_max = np.transpose(L2_dis_mouth_max, (1, 0, 2))
    L2_dis_mouth_max = np.sum(L2_dis_mouth_max, axis=2)
    L2_dis_mouth_max = np.max(L2_dis_mouth_max, axis=1)
    lve = np.mean(L2_dis_mouth_max)
    motion_std = []
    for x in (a, b):
        motion = x - t
        L2_dis_upper = np.array([np.square(motion[:, v, :]) for v in upper_map])
        L2_dis_upper = np.transpose(L2_dis_upper, (1, 0, 2))
        L2_dis_upper = np.sum(L2_dis_upper, axis=2)
        L2_dis_upper = np.std(L2_dis_upper, axis=0)
        motion_std.append(np.mean(L2_dis_upper))
    fdd = motion_std[0] - motion_std[1]
    dist = np.linalg.norm(a - b, axis=-1)
    got = VR.metrics(vertices_pred, vertices_gt, [0, F], mouth_map, upper_map, template)["clips"][0]
    print(f"lve {got['lve']:.6e} / {lve:.6e}, fdd {got['fdd']:.6e} / {fdd:.6e}, mve {got['mve']:.6e} / {dist.mean():.6e}")
    assert got["lve"] == pytest.approx(lve, rel=1e-13) and got["fdd"] == pytest.approx(fdd, rel=1e-10, abs=1e-16)
    assert got["mve"] == pytest.approx(dist.mean(), rel=1e-13) and got["max_ve"] == pytest.approx(dist.max(), rel=1e-14)
    assert got["rmse"] == pytest.approx(np.sqrt((dist ** 2).mean()), rel=1e-13) and got["frames"] == F


def test_host_reduction_against_the_restatement():
    """utils/metrics.reduce_clips on the emulators' table and state equals the restatement's metrics, per clip and pooled."""
    pred, gt, upper, template = VR.moments_case(65, True)
    off = list(VR.MOMENT_CLIPS)
    lips = np.arange(5, 60)
    region = np.zeros(VR.MOMENT_V, np.uint8)
    region[lips] = 1
    got = M.reduce_clips(VR.emulate_frame_table(pred, gt, region), VR.emulate_moments(pred, gt, off, upper, template), off, VR.MOMENT_V)
    want = VR.metrics(pred, gt, off, lips, upper, template)
    fb = VR.fdd_exact_and_bound(VR.moments_exact_case(65, True))
    for c, w, (fe, bound) in zip(got["clips"] + [got["all"]], want["clips"] + [want["all"]], fb + [(None, None)]):
        for k in ("lve", "mve", "max_ve", "rmse"):
            assert c[k] == pytest.approx(w[k], rel=(VR.MOMENT_V + 8) * VR.U52)
        assert c["frames"] == w["frames"]
        if fe is not None:
            assert abs(c["fdd"] - fe) <= bound
    assert got["clips"][3]["fdd"] == 0.0 and got["clips"][3]["frames"] == 1
    assert got["all"]["fdd"] == pytest.approx(np.mean([c["fdd"] for c in got["clips"]]), rel=1e-15, abs=1e-300)


@pytest.mark.parametrize("U,per_clip,half", [(u, pc, False) for u in VR.MOMENT_U for pc in (False, True)] + [(65, False, True)])
def test_moments_emulator_within_the_derived_bound_and_mutants_outside(U, per_clip, half):
    pred, gt, upper, template = VR.moments_case(U, per_clip, half)
    exact = VR.moments_exact_case(U, per_clip, half)
    off = list(VR.MOMENT_CLIPS)
    state = VR.emulate_moments(pred, gt, off, upper, template)
    ok, worst = VR.check_state(state, exact)
    ok_std, worst_std = VR.check_std(VR.state_std(state), exact)
    print(f"U {U}, per-clip template {per_clip}, fp16 {half}: Welford float64 worst error / bound {worst:.3e} (state), {worst_std:.3e} (std)")
    assert ok and ok_std
    if half or U < 63:
        return      # the mutants' errors are rounding accidents: they are asked to show on the cases with enough vertices
    for mode in ("fp32", "unshifted"):
        bad = VR.emulate_moments(pred, gt, off, upper, template, mode)
        ok_m, worst_m = VR.check_state(bad, exact)
        ok_s, worst_s = VR.check_std(VR.state_std(bad), exact)
        print(f"  mutant {mode}: worst error / bound {worst_m:.3e} (state), {worst_s:.3e} (std)")
        assert not ok_m and not ok_s
    ok_s, worst_s = VR.check_std(VR.state_std(state, sample=True), exact)
    print(f"  mutant sample variance: worst error / bound {worst_s:.3e} (std)")
    assert not ok_s


@pytest.mark.parametrize("V", VR.FRAME_V)
def test_frame_emulator_within_the_bounds_and_mutants_outside(V):
    for half in (False, True):
        for kind in VR.LIP_MASKS:
            for plant in ("first", "last"):
                pred, gt, lips, region = VR.frame_case(V, 3, half, kind, plant)
                want = VR.frame_table(pred, gt, lips)
                ok, worst = VR.table_ok(VR.emulate_frame_table(pred, gt, region), want, V)
                assert ok, (V, half, kind, plant, worst)
                planted_on_lip = (0 if plant == "first" else V - 1) in lips
                if not planted_on_lip:
                    assert (want[:, 0] < want[:, 2] ** 2 * 0.5).all()            # columns 0 and 2 must differ here ...
                    assert not VR.table_ok(VR.emulate_frame_table(pred, gt, region, lip_all=True), want, V)[0]   # ... and the mutant shows
    # NaN: at a vertex off the lips, at the last lip vertex, inf in both tensors
    if V < 3:
        return
    pred, gt, lips, region = (np.array(x) for x in VR.frame_case(V, 3, False, "third", "first"))
    off_lip, last_lip = 1, int(lips[-1])
    for at, value, cols in ((off_lip, np.nan, [1, 2, 3]), (last_lip, np.nan, [0, 1, 2, 3]), (last_lip, np.inf, [0, 1, 2, 3])):
        p, q = pred.copy(), gt.copy()
        p[1, at, 2] = value
        if np.isinf(value):
            q[1, at, 2] = value
        want = VR.frame_table(p, q, lips)
        assert np.isnan(want[1, cols]).all() and np.isfinite(np.delete(want, 1, 0)).all() and np.isnan(want).sum() == len(cols)
        assert VR.table_ok(VR.emulate_frame_table(p, q, region), want, V)[0]
        assert not VR.table_ok(VR.emulate_frame_table(p, q, region, vmax=np.fmax), want, V)[0]      # fmax drops the NaN


def test_regions_and_vertex_metrics_refusals():
    for lips, upper in (([], [1]), ([1], []), ([0, 5], [1]), ([-1], [1]), ([1, 1], [2]), ([1], [2, 3, 2]), ([[1, 2]], [1]), ([0.5], [1])):
        with pytest.raises(ValueError):
            M.regions(5, lips, upper, "cpu")
    with pytest.raises(ValueError):
        M.regions(0, [0], [0], "cpu")
    region, up = M.regions(6, [4, 1], [5, 0, 1], "cpu")
    assert region.dtype == torch.uint8 and region.tolist() == [2, 3, 0, 0, 1, 2] and up.dtype == torch.int32 and up.tolist() == [0, 1, 5]
    t = np.zeros((6, 3), np.float32)
    for off in ([1, 4], [0], [], [0, 3, 3], [0, 4, 2]):
        with pytest.raises(ValueError):
            M.VertexMetrics(off, 6, [1], [2], t, "cpu")
    with pytest.raises(ValueError):
        M.VertexMetrics([0, 4], 6, [1], [2], np.zeros((5, 3), np.float32), "cpu")
    with pytest.raises(ValueError):
        M.VertexMetrics([0, 2, 4], 6, [1], [2], np.zeros((3, 6, 3), np.float32), "cpu")
    vm = M.VertexMetrics([0, 2, 4], 6, [1], [2], t, "cpu")
    x = torch.zeros(3, 6, 3)
    with pytest.raises(ValueError):
        vm.result()                                       # before the end
    with pytest.raises(ValueError):
        vm.update(torch.zeros(5, 6, 3), torch.zeros(5, 6, 3))      # past the end
    with pytest.raises(TypeError):
        vm.update(x, x.half())                            # mixed dtypes
    with pytest.raises(ValueError):
        vm.update(x, torch.zeros(3, 5, 3))
    with pytest.raises(ValueError):
        vm.update(torch.zeros(3, 7, 3), torch.zeros(3, 7, 3))
    with pytest.raises(RuntimeError):
        vm.update(x, x)                                   # no CPU path
    with pytest.raises(ValueError):
        M.vertex_metrics(x, x, [0, 4], [1], [2], t)       # offsets not from 0 to n
    assert vm.update(x[:0], x[:0]) is vm and vm.seen == 0


def test_command_line_flag_checks_and_regions_file(tmp_path, capsys):
    base = ["--pred_exp", "a", "--pred_rot", "b", "--gt_exp", "c", "--gt_rot", "d", "--regions", "r"]
    args = M.parse_args(base)
    assert args.out == "metrics.json" and args.chunk == 512 and not args.with_global_pose and args.coef_dict_path is None
    for extra, word in ((["--normalised"], "--coef_dict_path"), (["--coef_dict_path", "s.pkl"], "--normalised"), (["--chunk", "0"], "--chunk")):
        with pytest.raises(SystemExit) as e:
            M.parse_args(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        M.parse_args(base[2:])
    capsys.readouterr()
    assert M.parse_args(base + ["--normalised", "--coef_dict_path", "s.pkl"]).normalised
    np.savez(tmp_path / "r.npz", lips=np.array([[3, 1]]), upper=np.array([7, 2]))
    lips, upper = M.load_regions(tmp_path / "r.npz")
    assert lips.tolist() == [3, 1] and upper.tolist() == [7, 2]
    with open(tmp_path / "masks.pkl", "wb") as f:       # FLAME_masks-style: no `upper`
        pkl.dump(dict(lips=np.array([3, 1]), forehead=np.array([9, 4]), eye_region=np.array([4, 6]), nose=np.array([0])), f)
    lips, upper = M.load_regions(tmp_path / "masks.pkl")
    assert lips.tolist() == [3, 1] and upper.tolist() == [4, 6, 9]
    for bad in (dict(upper=np.array([1])), dict(lips=np.array([1]), forehead=np.array([2]))):
        with open(tmp_path / "bad.pkl", "wb") as f:
            pkl.dump(bad, f)
        with pytest.raises(ValueError):
            M.load_regions(tmp_path / "bad.pkl")
