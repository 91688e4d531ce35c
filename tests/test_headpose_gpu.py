"""Head pose from landmarks on the MI355X: csrc/headpose.hip through msmd_amd.utils.head_pose against the float64 restatement
(tests/headpose_ref.py, itself pinned to the reference's recorded outputs by tests/test_headpose_cpu.py).

Bounds (max over the frames of a clip):
  fit      R as a geodesic angle in degrees, c relative, t and the aligned landmarks relative to their largest magnitude: at most
           8 x the recorded err32_fit (the reference's own functions on float32 copies of the inputs against their float64 run;
           the smallest of the recorded cases is taken), and not below 4 ulp of fp32 at the value's magnitude -- an entry of R
           has magnitude 1, so the floor on the angle is 4 * 2^-23 rad = 2.7e-5 degrees.
  angles   at most 8 x the error of headpose_ref with dtype=float32 against its float64 run on the same clip, with the same
           floor at the clip's largest angle.  Angles are compared on the circle (a difference of 360 degrees is none).
           R_smoothed is held to the same multiple of the float32 run's own R_modified error.
Every figure is printed before it is asserted."""
import pickle as pkl
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import headpose_ref as HR
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 256                      # MSMD_HEADPOSE_CHUNK: frames per step of the smoothing kernel's sign scan
ULP4 = 4 * 2.0 ** -23


@pytest.fixture(scope="module")
def g():
    return load_golden("g13_headpose")


def points(g, kind):
    """-> (neutral (N, 3) fp32, static_idx): 478 tracked points with the 20 static ones; the 20 static points alone (P = S);
    30 points with a static triangle (nose tip and the two outer face anchors)."""
    canon, static = g["canonical"], g["static_idx"]
    if kind == "478":
        return np.concatenate([canon, canon[458:468] + np.float32([0, 0, 0.5])], 0), static
    if kind == "20":
        return canon[static], np.arange(20, dtype=np.int32)
    small = np.concatenate([static, np.arange(200, 210, dtype=np.int32)])
    assert (static[[8, 12, 13]] == [1, 127, 356]).all()
    return canon[small], np.array([8, 12, 13], np.int32)


def synth_clip(seed, F, neutral, yaw=35.0, turns=1.0, mirror=False):
    """(F, N, 3) fp32 landmarks: the neutral points under Y-X-Z poses (yaw swings +-`yaw` `turns` times, pitch within 20, roll
    within 15 degrees), scale 1 / 30 about (0.5, 0.5, 0), noise 2e-4."""
    rng = np.random.default_rng(seed)
    u = np.linspace(0, 1, F)
    pose = HR.euler_yxz_to_mat(np.stack([yaw * np.sin(2 * np.pi * turns * u), 20 * np.cos(3 * u), 15 * np.sin(5 * u)], 1))
    flip = np.diag([1.0, -1.0, -1.0])
    L = np.einsum("fij,nj->fni", np.einsum("fji,jk->fik", pose, flip), neutral.astype(np.float64)) / 30.0 + [0.5, 0.5, 0.0]
    L += 2e-4 * rng.standard_normal(L.shape)
    if mirror:
        L[..., 0] = 1.0 - L[..., 0]
    return L.astype(np.float32)


def circle(d):
    return (d + 180.0) % 360.0 - 180.0


def floor_rel(x):
    m = float(np.abs(x).max())
    return 4 * float(np.spacing(np.float32(m))) / m


def check_clip(g, tag, L, neutral, sidx, valid, window, polyorder, ypr, det):
    """One clip's device results against the float64 restatement, under the bounds of the module docstring."""
    r64 = HR.head_pose(L, neutral, sidx, valid, window, polyorder)
    r32 = HR.head_pose(L, neutral, sidx, valid, window, polyorder, dtype=np.float32)
    e32 = np.min([g[f"{n}/err32_fit"] for n in g["cases"]], 0)
    ypr = ypr.cpu().numpy()
    assert ypr.dtype == np.float32 and ypr.shape == (L.shape[0], 3) and np.isfinite(ypr).all()
    err = float(np.abs(circle(ypr - r64["ypr"])).max())
    yard = float(np.abs(circle(r32["ypr"] - r64["ypr"])).max())
    bound = max(8 * yard, 4 * float(np.spacing(np.float32(np.abs(r64["ypr"]).max()))))
    print(f"{tag}: angles err {err:.3e} deg, float32 restatement {yard:.3e}, bound {bound:.3e}")
    assert np.abs(r64["ypr"][:, 1]).max() <= 60.0
    assert err <= bound
    if det is None:
        return
    d = {k: v.cpu().numpy() for k, v in det.items()}
    figures = [("R (deg)", HR.geodesic_deg(d["R"], r64["R"]).max(), max(8 * e32[0], np.degrees(ULP4))),
               ("c", np.abs(d["c"] / r64["c"] - 1).max(), max(8 * e32[1], floor_rel(r64["c"]))),
               ("t", np.abs(d["t"] - r64["t"]).max() / np.abs(r64["t"]).max(), max(8 * e32[2], floor_rel(r64["t"]))),
               ("aligned", np.abs(d["aligned"] - r64["aligned"]).max() / np.abs(r64["aligned"]).max(),
                max(8 * e32[3], floor_rel(r64["aligned"]))),
               ("R_smoothed (deg)", HR.geodesic_deg(d["R_smoothed"], r64["R_modified"]).max(),
                max(8 * HR.geodesic_deg(r32["R_modified"], r64["R_modified"]).max(), np.degrees(ULP4)))]
    for name, e, b in figures:
        print(f"{tag}: {name} err {e:.3e}, bound {b:.3e}")
    for name, e, b in figures:
        assert e <= b, (name, e, b)


def run(L, neutral, sidx, valid=None, window=5, polyorder=2, details=True):
    from msmd_amd.utils.head_pose import head_pose_from_landmarks
    dev = [torch.from_numpy(x).to(DEV) for x in L] if isinstance(L, list) else torch.from_numpy(L).to(DEV)
    out = head_pose_from_landmarks(dev, neutral, sidx, valid, window, polyorder, return_details=details)
    torch.cuda.synchronize()
    return out if details else (out, None)


def gaps(F, g_len):
    """g_len frames missing at the start, in the middle and at the end."""
    v = np.ones(F, bool)
    v[:g_len] = False
    v[F // 2:F // 2 + g_len] = False
    v[F - g_len:] = False
    return v


@pytest.mark.parametrize("F", [5, 6, 7])
def test_short_clips_are_all_or_mostly_edge_frames(g, F):
    neutral, sidx = points(g, "478")
    L = synth_clip(F, F, neutral)
    ypr, det = run(L, neutral, sidx)
    check_clip(g, f"F={F}", L, neutral, sidx, None, 5, 2, ypr, det)


@pytest.mark.parametrize("F,window,polyorder", [(CHUNK - 1, 5, 2), (CHUNK, 5, 2), (CHUNK + 1, 5, 2), (2 * CHUNK + 88, 5, 2),
                                                (CHUNK + 1, 9, 4), (2 * CHUNK + 3, 9, 4)])
def test_clip_lengths_around_the_scan_chunk(g, F, window, polyorder):
    """P = S = 20.  The yaw swings +-125 degrees once in 150 frames, so the raw quaternions change sign near frames 94, 132,
    244, 281, ...: several times in every chunk, and the sign carried across the first chunk boundary is -1."""
    neutral, sidx = points(g, "20")
    L = synth_clip(1000 + F, F, neutral, yaw=125.0, turns=F / 150.0)
    q = HR.mat_to_quat(HR.fit(L, neutral, sidx)[0])
    par = np.cumsum((q[1:] * q[:-1]).sum(1) < 0) % 2
    if F > CHUNK:
        assert par[CHUNK - 2] == 1, "the sign carried into the second chunk should be -1"
    assert par.any()
    ypr, det = run(L, neutral, sidx, None, window, polyorder)
    check_clip(g, f"F={F} ({window}, {polyorder})", L, neutral, sidx, None, window, polyorder, ypr, det)


@pytest.mark.parametrize("g_len", [1, 2, 3])
def test_gaps_at_the_start_inside_and_at_the_end(g, g_len):
    neutral, sidx = points(g, "478")
    L = synth_clip(50 + g_len, 37, neutral)
    valid = gaps(37, g_len)
    L[~valid] = np.nan                                   # what a missing frame holds is never read
    ypr, det = run(L, neutral, sidx, valid)
    check_clip(g, f"gaps of {g_len}", np.nan_to_num(L), neutral, sidx, valid, 5, 2, ypr, det)


@pytest.mark.parametrize("name", ["clip37", "mirror", "flip"])
def test_recorded_cases(g, name):
    """clip37: 8 of 37 frames missing; mirror: det(cov) < 0, the sign matrix flips; flip: the raw quaternions change sign."""
    L, neutral, sidx, valid = (g[f"{name}/{k}"] for k in ("landmarks", "neutral", "static_idx", "valid"))
    ypr, det = run(L, neutral, sidx, valid)
    check_clip(g, name, L, neutral, sidx, valid, 5, 2, ypr, det)
    # and against the reference's recorded angles themselves
    assert np.abs(circle(ypr.cpu().numpy() - g[f"{name}/ypr"])).max() <= 1e-3


@pytest.mark.parametrize("window,polyorder,F", [(7, 3, 37), (9, 4, 37), (7, 3, 7), (9, 4, 9), (9, 4, 10)])
def test_filter_windows(g, window, polyorder, F):
    neutral, sidx = points(g, "478" if F == 37 else "20")
    L = synth_clip(70 + F + window, F, neutral, yaw=125.0 if F == 37 else 35.0)
    ypr, det = run(L, neutral, sidx, None, window, polyorder)
    check_clip(g, f"({window}, {polyorder}) F={F}", L, neutral, sidx, None, window, polyorder, ypr, det)


def test_three_static_points(g):
    """S = 3, the minimum: a covariance of rank 2, which still determines the rotation."""
    neutral, sidx = points(g, "S3")
    L = synth_clip(3, 21, neutral)
    ypr, det = run(L, neutral, sidx)
    check_clip(g, "S=3", L, neutral, sidx, None, 5, 2, ypr, det)


def test_details_off_gives_the_same_angles(g):
    neutral, sidx = points(g, "478")
    L = synth_clip(9, 37, neutral)
    valid = gaps(37, 2)
    ypr, det = run(L, neutral, sidx, valid)
    only, none = run(L, neutral, sidx, valid, details=False)
    assert none is None and torch.equal(only, ypr)
    assert sorted(det) == ["R", "R_smoothed", "aligned", "c", "t"]
    assert det["R"].shape == (37, 3, 3) and det["aligned"].shape == (37, 478, 3) and det["R_smoothed"].shape == (37, 3, 3)
    # the ops level: aligned and the matrix are optional outputs of the two launches
    from msmd_amd import ops
    from msmd_amd.utils.head_pose import gap_plan, savgol_table
    a, b, w = gap_plan(valid)
    t = lambda x, dt: torch.from_numpy(x).to(dt).to(DEV)
    rows = np.zeros((478, 3), np.float32)
    rows[:] = neutral
    args = (t(L, torch.float32), t(a, torch.int32), t(b, torch.int32), t(w, torch.float32), t(rows, torch.float32), t(sidx, torch.int32))
    R1, c1, t1, al = ops.headpose_fit(*args, want_aligned=False)
    assert al is None and torch.equal(R1, det["R"]) and torch.equal(c1, det["c"]) and torch.equal(t1, det["t"])
    y1, m1 = ops.headpose_smooth(R1, [0, 37], t(savgol_table(5, 2), torch.float64), 5)
    assert m1 is None and torch.equal(y1, ypr)


def test_ragged_list_gives_each_clip_the_bits_it_gets_alone(g):
    neutral, sidx = points(g, "478")
    Ls = [synth_clip(20 + F, F, neutral, yaw=125.0) for F in (5, 37, 130)]
    valids = [None, gaps(37, 3), gaps(130, 2)]
    yprs, dets = run(Ls, neutral, sidx, valids)
    assert isinstance(yprs, list) and [tuple(y.shape) for y in yprs] == [(5, 3), (37, 3), (130, 3)]
    for L, v, y, d in zip(Ls, valids, yprs, dets):
        alone, d_alone = run(L, neutral, sidx, v)
        assert torch.equal(alone, y)
        for k in d:
            assert torch.equal(d[k], d_alone[k]), k
    check_clip(g, "ragged[2]", Ls[2], neutral, sidx, valids[2], 5, 2, yprs[2], dets[2])


def test_errors(g):
    from msmd_amd import ops
    from msmd_amd.utils.head_pose import head_pose_from_landmarks, savgol_table
    neutral, sidx = points(g, "20")
    L = torch.from_numpy(synth_clip(1, 12, neutral)).to(DEV)
    with pytest.raises(ValueError, match="shorter"):
        head_pose_from_landmarks(L[:4], neutral, sidx)
    with pytest.raises(ValueError, match="shorter"):
        head_pose_from_landmarks(L[:6], neutral, sidx, window_length=7, polyorder=3)
    with pytest.raises(ValueError):
        head_pose_from_landmarks(L, neutral, sidx, window_length=6)
    with pytest.raises(ValueError):
        head_pose_from_landmarks(L, neutral, sidx, window_length=5, polyorder=5)
    with pytest.raises(ValueError, match="missing"):
        head_pose_from_landmarks(L, neutral, sidx, valid=np.arange(12) % 2 == 0)
    with pytest.raises(ValueError, match="valid"):
        head_pose_from_landmarks(L, neutral, sidx, valid=np.zeros(12, bool))
    with pytest.raises(ValueError):
        head_pose_from_landmarks(L, neutral, sidx, valid=np.ones(11, bool))
    with pytest.raises(ValueError, match="static_idx"):
        head_pose_from_landmarks(L, neutral, np.array([0, 1, 20]))
    with pytest.raises(ValueError, match="static_idx"):
        head_pose_from_landmarks(L, neutral, np.array([0, 1]))
    with pytest.raises(TypeError):
        head_pose_from_landmarks([L, L[:, :10]], neutral, sidx)
    with pytest.raises(RuntimeError, match="no CPU path"):
        head_pose_from_landmarks(L.cpu(), neutral, sidx)
    R = torch.eye(3, device=DEV).repeat(12, 1, 1)
    tab = torch.from_numpy(savgol_table(5, 2)).to(DEV)
    for off in ([0, 11], [1, 12], [0, 4, 12], [0, 8, 12]):
        with pytest.raises(ValueError):
            ops.headpose_smooth(R, off, tab, 5)
    with pytest.raises(ValueError):
        ops.headpose_smooth(R, [0, 12], tab, 4)
    with pytest.raises(TypeError):
        ops.headpose_smooth(R, [0, 12], tab[:10], 5)


def test_command_line_writes_the_pickle_the_style_clip_loader_reads(g, tmp_path, capsys):
    from msmd_amd.inference import query_for_motion_coeff
    from msmd_amd.utils import head_pose
    L, valid = g["clip37/landmarks"], g["clip37/valid"]
    np.save(tmp_path / "L.npy", L)
    np.save(tmp_path / "V.npy", valid)
    with open(tmp_path / "face.obj", "w") as f:
        f.write("".join(f"v {x!r} {y!r} {z!r}\n" for x, y, z in g["canonical"].astype(np.float64).tolist()) + "f 1 2 3\n")
    with open(tmp_path / "map.json", "w") as f:
        f.write('{"nose": {"dorsum": [6,197,195,5,4], "tipLower": [218,237,44,1,274,457,438]}, '
                '"additional_anchors": [127,356,132,361,33,133,362,263]}')
    head_pose.main(["--landmarks", str(tmp_path / "L.npy"), "--valid", str(tmp_path / "V.npy"), "--neutral", str(tmp_path / "face.obj"),
                    "--mapping", str(tmp_path / "map.json"), "--out", str(tmp_path / "clip.pkl")])
    assert "clip.pkl" in capsys.readouterr().out
    with open(tmp_path / "clip.pkl", "rb") as f:
        rot = pkl.load(f)
    assert type(rot) is np.ndarray and rot.dtype == np.float64 and rot.shape == (37, 3)
    assert np.abs(circle(rot - g["clip37/ypr"])).max() <= 1e-3
    stats = {"exp_mean": torch.zeros(50), "exp_std": torch.ones(50), "pose_mean": torch.zeros(3), "pose_std": torch.ones(3)}
    with open(tmp_path / "stats.pkl", "wb") as f:
        pkl.dump(stats, f)
    with open(tmp_path / "exp.pkl", "wb") as f:
        pkl.dump(np.zeros((37, 50), np.float32), f)
    m, _ = query_for_motion_coeff(SimpleNamespace(coef_dict_path=str(tmp_path / "stats.pkl")), str(tmp_path / "exp.pkl"),
                                  str(tmp_path / "clip.pkl"), device=DEV, original_fps=25, target_fps=25)
    assert m.shape == (1, 37, 53) and np.abs(m[0, :, 50:].cpu().numpy() - rot).max() < 1e-4
