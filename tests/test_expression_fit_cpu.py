"""The expression fit without a GPU: the float64 restatement (tests/expression_fit_ref.py) against the FLAME oracle, its analytic
Jacobian against central differences, recovery of generating parameters, the reduced tables of utils/expression_fit.reduce_flame
(torch on the CPU) against the full FLAME path, the host-side refusals, the pickle, and the condition the GPU tests rest on."""
import pickle as pkl
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import expression_fit_ref as ER
from msmd_amd import synth
from msmd_amd.utils import expression_fit as EF
from msmd_amd.utils.flame import FLAME, FLAMEConfig
from oracle import flame as ofl


@pytest.fixture(scope="module")
def asset():
    return synth.flame_asset()


@pytest.fixture(scope="module")
def flame_cpu(asset):
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = asset
    return FLAME(cfg)


def rng_inputs(seed, B, NE=50):
    g = np.random.default_rng(seed)
    f32 = lambda x: x.astype(np.float32)
    return f32(0.3 * g.standard_normal((B, 100))), f32(0.5 * g.standard_normal((B, NE))), f32(0.3 * g.standard_normal((B, 3)))


def test_restated_landmarks_match_the_oracle(asset):
    """FlameOracle.forward(...)[2] is numpy fp32 throughout: the float64 restatement must agree to that oracle's own accuracy,
    taken as 64 ulp of fp32 at the largest coordinate (150 + 36 products per vertex, three corners per landmark)."""
    o = ofl.FlameOracle(asset)
    shp, e, th = rng_inputs(1, 4)
    pose = np.concatenate([np.zeros((4, 3), np.float32), th], 1)
    lm = o.forward(shp, e, pose, return_lm2d=False)[2]
    m = ER.model(50)
    mine = np.concatenate([ER.landmarks_full(m, o.full_faces_idx[0], o.full_bary[0], shp[i:i + 1], e[i:i + 1], th[i:i + 1]) for i in range(4)])
    err, bound = float(np.abs(lm - mine).max()), 64 * float(np.spacing(np.float32(np.abs(mine).max())))
    print(f"restatement vs oracle: {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("theta", [(0.0, 0.0, 0.0), (0.3, -0.3, 0.26457513110645906)], ids=["theta0", "theta0.5"])
def test_jacobian_against_central_differences(theta):
    theta = np.array(theta)
    assert theta.any() == (abs(np.linalg.norm(theta) - 0.5) < 1e-12)
    m = ER.model(50)
    fidx, bary = ER.embedding(18, m["faces"].shape[0])
    shp, e, _ = rng_inputs(2, 1)
    s0, e0 = shp[0].astype(np.float64), 3.0 * e[0].astype(np.float64)
    Ja = ER.jacobian(m, fidx, bary, s0, e0, theta)
    p, h = np.concatenate([e0, theta]), 1e-5
    Jn = np.zeros_like(Ja)
    for j in range(53):
        d = np.zeros(53)
        d[j] = h
        lp = ER.landmarks_full(m, fidx, bary, s0[None], (p + d)[None, :50], (p + d)[None, 50:])[0]
        lm = ER.landmarks_full(m, fidx, bary, s0[None], (p - d)[None, :50], (p - d)[None, 50:])[0]
        Jn[:, :, j] = (lp - lm) / (2 * h)
    rel = float(np.abs(Ja - Jn).max() / np.abs(Jn).max())
    print(f"analytic vs central differences: {rel:.3e} relative")
    assert rel < 1e-6


@pytest.mark.parametrize("jaw_dof", [0, 1, 3])
def test_fit_returns_the_generating_parameters(jaw_dof):
    """Noise-free float64 targets, lambda = 0: the fit lands on (e, theta) to the float64 floor times the problem's condition."""
    m = ER.model(50)
    fidx, bary = ER.embedding(68, m["faces"].shape[0])
    g = np.random.default_rng(3)
    shapes = 0.5 * g.standard_normal((1, 100))
    e = 1.5 * g.standard_normal((2, 50))
    th = np.zeros((2, 3))
    th[:, :jaw_dof] = np.array([0.4, 0.1, -0.08])[:jaw_dof]
    y = ER.landmarks_full(m, fidx, bary, shapes, e, th)
    r = ER.fit(m, fidx, bary, shapes, [0, 0], y, None, jaw_dof, 0.0, 0.0, 12)
    err = float(max(np.abs(r["code"] - e).max(), np.abs(r["jaw"] - th).max()))
    print(f"jaw_dof {jaw_dof}: recovered to {err:.3e}, rms {r['rms'].max():.3e}")
    assert err < 1e-9 and r["rms"].max() < 1e-12 and not r["status"].any()


def test_float32_switch_runs_the_same_code():
    r = ER.reference("K68-jaw1")
    r32 = ER.fit(r["m"], r["fidx"], r["bary"], r["shapes"], r["subject"][:1], r["y"][:1], r["w"], 1, 1e-6, 0.0, 12, dtype=np.float32)
    assert r32["hist"].dtype == np.float32
    err = float(np.abs(r32["hist"][-1] - r["p"][:1]).max())
    print(f"float32 restatement vs float64: {err:.3e}")
    assert err < 1e-2


@pytest.mark.parametrize("K", [1, 68, 128])
def test_reduced_tables_reproduce_the_full_path(flame_cpu, K):
    """utils/expression_fit.reduce_flame (torch, float64, here on the CPU) and its numpy twin against FLAME's full path."""
    m = ER.model(50)
    fidx, bary = ER.embedding(K, m["faces"].shape[0])
    shp, e, th = rng_inputs(4, 3)
    tab, tab0 = EF.reduce_flame(flame_cpu, fidx, bary, torch.from_numpy(shp))
    assert tab.dtype == torch.float64 and tuple(tab.shape) == (K, 6, 59) and tuple(tab0.shape) == (3, K, 6)
    tn, t0n = ER.reduce_tables(m, fidx, bary, shp)
    worst = 0.0
    for s in range(3):
        full = ER.landmarks_full(m, fidx, bary, shp[s:s + 1], e[s:s + 1], th[s:s + 1])[0]
        worst = max(worst, float(np.abs(ER.landmarks_reduced(tab.numpy(), tab0.numpy(), s, e[s], th[s]) - full).max()),
                    float(np.abs(ER.landmarks_reduced(tn, t0n, s, e[s], th[s]) - full).max()))
    print(f"K = {K}: reduced tables vs full path {worst:.3e}")
    assert worst < 1e-15
    one = EF.reduce_flame(flame_cpu, fidx, bary, shp[1])[1]
    assert tuple(one.shape) == (1, K, 6) and torch.equal(one[0], tab0[1])      # one shape or several: the same bits


def test_refusals(flame_cpu):
    m = ER.model(50)
    F = m["faces"].shape[0]
    fidx, bary = ER.embedding(68, F)
    shape = np.zeros(100, np.float32)
    L = torch.zeros(6, 68, 3)
    fit = lambda **k: EF.fit_expression(k.pop("L", L), k.pop("flame", flame_cpu), k.pop("shape", shape), k.pop("fidx", fidx),
                                        k.pop("bary", bary), **k)
    f129, b129 = ER.embedding(129, F)
    with pytest.raises(ValueError, match="129 landmarks"):
        fit(L=torch.zeros(6, 129, 3), fidx=f129, bary=b129)
    for bad in (-1, F):
        with pytest.raises(ValueError, match="lmk_faces_idx"):
            fit(fidx=np.concatenate([fidx[:-1], [bad]]))
    w = np.ones(68)
    w[3] = -1e-3
    with pytest.raises(ValueError, match="weights"):
        fit(weights=w)
    with pytest.raises(ValueError, match="weights"):
        fit(weights=np.zeros(68))
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset, cfg.n_exp = synth.flame_asset(), 62
    with pytest.raises(ValueError, match="62 expression"):
        fit(flame=FLAME(cfg))
    for jd in (2, -1, 4):
        with pytest.raises(ValueError, match="jaw_dof"):
            fit(jaw_dof=jd)
    for its in (-1, 65):
        with pytest.raises(ValueError, match="iterations"):
            fit(iterations=its)
    with pytest.raises(ValueError, match="one per clip"):
        fit(L=[L, L, L], shape=np.zeros((2, 100), np.float32))
    with pytest.raises(RuntimeError, match="cuda"):      # everything on the host passed: the launch itself needs the device
        fit()


def test_pickle_round_trips_through_query_for_motion_coeff(tmp_path):
    from msmd_amd import inference
    g = np.random.default_rng(5)
    code = g.standard_normal((30, 50)).astype(np.float32)
    head = g.standard_normal((30, 3))
    stats = dict(exp_mean=np.zeros(50, np.float32), exp_std=np.ones(50, np.float32), pose_mean=np.zeros(3, np.float32),
                 pose_std=np.ones(3, np.float32))
    paths = {k: str(tmp_path / f"{k}.pkl") for k in ("stats", "head")}
    for k, v in (("stats", stats), ("head", head)):
        with open(paths[k], "wb") as f:
            pkl.dump(v, f)
    EF.save_expression_code(str(tmp_path / "code.pkl"), torch.from_numpy(code))
    with open(tmp_path / "code.pkl", "rb") as f:
        back = pkl.load(f)
    assert isinstance(back, np.ndarray) and back.dtype == np.float32 and np.array_equal(back, code)
    coef, shape = inference.query_for_motion_coeff(SimpleNamespace(coef_dict_path=paths["stats"]), str(tmp_path / "code.pkl"),
                                                   paths["head"], device="cpu", original_fps=25, target_fps=25)
    assert tuple(coef.shape) == (1, 30, 53) and coef.dtype == torch.float32 and tuple(shape.shape) == (1, 100)
    assert np.allclose(coef[0, :, :50].numpy(), code, rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        EF.save_expression_code(str(tmp_path / "bad.pkl"), np.zeros(50))


def test_fit_report():
    rep = EF.fit_report(np.array([1e-3, 3e-3, np.nan, 2e-3]), np.array([0, 2, 1, 0]))
    assert rep == dict(frames=4, rms_median=2e-3, rms_max=3e-3, flagged=2, non_finite=1, refused=1)


@pytest.mark.parametrize("name", list(ER.CASES))
def test_restatement_sits_still_on_every_gpu_case(name):
    """The condition tests/test_expression_fit_gpu.py rests on: by `iterations` the float64 run has stopped moving, so it and the
    kernel are both at the optimum: |iterate(N - 4) - iterate(N)| < 2^-26 max(1, |p|).  (iterations = 0 has nothing to converge.)"""
    r = ER.reference(name)
    assert not r["status"].any()
    if r["its"] == 0:
        assert not r["p"].any()
        return
    lim = 2.0 ** -26 * max(1.0, float(np.abs(r["p"]).max()))
    print(f"{name}: |iterate(N - 4) - iterate(N)| = {r['still']:.3e}, limit {lim:.3e}; floor |iterate(N) - iterate(N + 4)| = {r['floor']:.3e}")
    assert r["still"] < lim
