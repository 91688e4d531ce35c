"""The expression fit on the MI355X: csrc/expression_fit.hip through ops.expression_fit / utils.expression_fit against the
float64 restatement (tests/expression_fit_ref.py; tests/test_expression_fit_cpu.py pins it and checks that it sits still on
every case used here).

Bounds.  Both runs are at the optimum and the kernel's result is that optimum rounded once to fp32, so per parameter
    |p_gpu - p_ref| <= 2^-23 max(1, |p_ref|) + 8 floor,   floor = max |iterate(N) - iterate(N + 4)| of the float64 run on the case;
rms is held to 4 ulp of fp32 at its value plus the floor carried through: 8 floor times the largest 1-norm of a row of the
Jacobian (a change dp moves no landmark coordinate, and so not the weighted rms, by more than that times max |dp|).
Every figure is printed before it is asserted."""
import pickle as pkl
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import expression_fit_ref as ER
from msmd_amd import _lib, ops, synth
from msmd_amd.utils import expression_fit as EF
from msmd_amd.utils.flame import FLAME, FLAMEConfig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_FLAMES = {}


def flame(NE=50):
    if NE not in _FLAMES:
        cfg = SimpleNamespace(**vars(FLAMEConfig))
        cfg.asset, cfg.n_exp = synth.flame_asset(), NE
        _FLAMES[NE] = FLAME(cfg).to(DEV)
    return _FLAMES[NE]


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dt is None else t.to(dt)).to(DEV)


def run_case(r, **over):
    """One launch for the case's n frames through ops.expression_fit -> numpy (code, jaw, rms, status)."""
    assert ops.EXPFIT_FRAMES == ER.FRAMES
    tab, tab0 = EF.reduce_flame(flame(r["NE"]), r["fidx"], r["bary"], dev(r["shapes"]))
    out = ops.expression_fit(dev(r["y"]), dev(over.get("subject", r["subject"]), torch.int32), tab, tab0, dev(r["w"]), r["jd"],
                             r["le"], r["lj"], over.get("its", r["its"]))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", list(ER.CASES))
def test_parameters_against_the_float64_restatement(name):
    r = ER.reference(name)
    code, jaw, rms, status = run_case(r)
    n, NE, jd = r["n"], r["NE"], r["jd"]
    assert code.shape == (n, NE) and jaw.shape == (n, 3) and rms.shape == (n,) and status.shape == (n,)
    assert code.dtype == jaw.dtype == rms.dtype == np.float32 and status.dtype == np.int32
    p_gpu, p_ref = np.concatenate([code, jaw], 1).astype(np.float64), r["p"]
    bound = 2.0 ** -23 * np.maximum(1.0, np.abs(p_ref)) + 8 * r["floor"]
    err = np.abs(p_gpu - p_ref)
    lip = max(float(np.abs(ER.jacobian(r["m"], r["fidx"], r["bary"], r["shapes"][r["subject"][i]], r["p"][i, :NE], r["p"][i, NE:])).sum(-1).max())
              for i in range(min(n, r["D"])))
    rms_bound = 4 * np.spacing(r["rms"].astype(np.float32)).astype(np.float64) + 8 * r["floor"] * lip
    rms_err = np.abs(rms.astype(np.float64) - r["rms"])
    print(f"{name}: parameters err {err.max():.3e} (worst err / bound {np.max(err / bound):.3f}, floor {r['floor']:.3e}); "
          f"rms {r['rms'].max():.3e} err {rms_err.max():.3e} (worst err / bound {np.max(rms_err / rms_bound):.3f}); status {status.max()}")
    assert not status.any()
    assert (jaw[:, jd:] == 0).all()
    assert (err <= bound).all()
    assert (rms_err <= rms_bound).all()
    if r["its"] == 0:
        assert not code.any() and not jaw.any()


def test_reproduces_flame():
    """Noise-free fp32 targets made by FLAME.forward -> ops.landmarks on the device; the fitted (code, jaw) put back through the
    same path returns them.  Residual rms <= 4 x what the float64 restatement leaves on those targets, not asked below
    16 * 2^-24 max |y|."""
    fl = flame(50)
    g = np.random.default_rng(11)
    n = 6
    shape = (0.5 * g.standard_normal((1, 100))).astype(np.float32)
    e = (1.5 * g.standard_normal((n, 50))).astype(np.float32)
    th = (np.array([[0.4, 0.1, -0.08]]) * (1 + 0.2 * g.standard_normal((n, 1)))).astype(np.float32)
    fwd = lambda ee, tt: fl(dev(shape).expand(n, -1).contiguous(), ee, torch.cat([torch.zeros_like(tt), tt], 1).contiguous(),
                            return_lm2d=False, return_lm3d=True)[2]
    y = fwd(dev(e), dev(th))
    fidx, bary = fl.full_lmk_faces_idx[0].cpu().numpy(), fl.full_lmk_bary_coords[0].cpu().numpy()
    code, det = EF.fit_expression(y, fl, shape[0], fidx, bary, jaw_dof=3, return_details=True)
    back = fwd(code, det["jaw"])
    res = float(((back - y).double() ** 2).sum(-1).mean().sqrt())
    ref = ER.fit(ER.model(50), fidx, bary, shape, np.zeros(n, int), y.cpu().numpy(), None, 3, 1e-6, 0.0, 12)
    ymax = float(y.abs().max())
    bound = max(4 * float(np.sqrt((ref["rms"] ** 2).mean())), 16 * 2.0 ** -24 * ymax)
    perr = float(max(np.abs(code.cpu().numpy() - e).max(), np.abs(det["jaw"].cpu().numpy() - th).max()))
    print(f"reproduces FLAME: residual rms {res:.3e}, float64 restatement leaves {np.sqrt((ref['rms'] ** 2).mean()):.3e}, bound {bound:.3e}; "
          f"kernel rms {float(det['rms'].max()):.3e}; parameters off the generating ones by {perr:.3e} (the prior's pull)")
    assert int(det["status"].abs().max()) == 0
    assert res <= bound


def test_bits_alone_and_inside_a_ragged_batch():
    r = ER.reference("subjects3")
    fl = flame(50)
    y = dev(r["y"])
    a, b, c = y[:3].contiguous(), y[:7].contiguous(), y[2:7].contiguous()
    shapes = np.stack([r["shapes"][1], r["shapes"][0], r["shapes"][2]]).astype(np.float32)
    kw = dict(weights=r["w"], jaw_dof=3, return_details=True)
    code1, det1 = EF.fit_expression(b, fl, shapes[1], r["fidx"], r["bary"], **kw)
    codes, dets = EF.fit_expression([a, b, c], fl, shapes, r["fidx"], r["bary"], **kw)
    code2, det2 = EF.fit_expression(b, fl, shapes[1], r["fidx"], r["bary"], **kw)
    torch.cuda.synchronize()
    words = lambda t: t.cpu().numpy().view(np.int32)
    for tag, (x, d) in (("inside a batch of three", (codes[1], dets[1])), ("second run", (code2, det2))):
        same = [np.array_equal(words(x), words(code1))] + [np.array_equal(words(d[k]), words(det1[k])) for k in ("jaw", "rms", "status")]
        print(f"{tag}: code / jaw / rms / status words identical: {same}")
        assert all(same)
    assert [tuple(x.shape) for x in codes] == [(3, 50), (7, 50), (5, 50)] and torch.isfinite(code1).all()


def test_c_abi_guards_clamp_and_nan():
    """The raw entry point: guard elements behind every output stay untouched, every output element is written, a subject outside
    [0, S) is clamped, a frame with one NaN landmark returns NaN with status 1 and its neighbours keep their bits."""
    r = ER.reference("subjects3")
    n, K, NE, S = r["n"], r["K"], r["NE"], 3
    tab, tab0 = EF.reduce_flame(flame(NE), r["fidx"], r["bary"], dev(r["shapes"]))
    w = dev(r["w"])
    G = 64
    SENT_F, SENT_I = np.float32(-7.25), np.int32(-77)

    def call(y, subject):
        bufs = [torch.full((n * NE + G,), float(SENT_F), device=DEV), torch.full((n * 3 + G,), float(SENT_F), device=DEV),
                torch.full((n + G,), float(SENT_F), device=DEV), torch.full((n + G,), int(SENT_I), device=DEV, dtype=torch.int32)]
        yd, sd = dev(y), dev(subject, torch.int32)
        rc = _lib.load().msmd_expression_fit(yd.data_ptr(), sd.data_ptr(), tab.data_ptr(), tab0.data_ptr(), w.data_ptr(),
                                             *[b.data_ptr() for b in bufs], n, K, NE, S, r["jd"], r["its"], r["le"], r["lj"],
                                             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        return [b.cpu().numpy() for b in bufs]
    base = call(r["y"], r["subject"])
    sizes = (n * NE, n * 3, n, n)
    for b, size, sent in zip(base, sizes, (SENT_F, SENT_F, SENT_F, SENT_I)):
        assert (b[size:] == sent).all(), "a guard element was written"
        assert (b[:size] != sent).all(), "an output element was not written"
    p = np.concatenate([base[0][:n * NE].reshape(n, NE), base[1][:n * 3].reshape(n, 3)], 1)
    print(f"C ABI: parameters off the restatement by {np.abs(p - r['p']).max():.3e}")
    assert (np.abs(p - r["p"]) <= 2.0 ** -23 * np.maximum(1.0, np.abs(r["p"])) + 8 * r["floor"]).all()
    wild = r["subject"].copy()
    wild[r["subject"] == 0] = -5
    wild[r["subject"] == 2] = 2 ** 30
    clamped = call(r["y"], wild)
    print("out-of-range subjects: words identical to the in-range call:", [np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(base, clamped)])
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(base, clamped))
    y = r["y"].copy()
    bad = 5
    y[bad, K // 2, 1] = np.nan
    out = call(y, r["subject"])
    code, jaw, rms, status = out[0][:n * NE].reshape(n, NE), out[1][:n * 3].reshape(n, 3), out[2][:n], out[3][:n]
    print(f"NaN landmark in frame {bad}: status {status.tolist()}")
    assert np.isnan(code[bad]).all() and np.isnan(jaw[bad]).all() and np.isnan(rms[bad]) and status[bad] == 1
    keep = np.arange(n) != bad
    for a, b, width in zip(base, out, (NE, 3, 1, 1)):
        assert np.array_equal(a[:n * width].reshape(n, width)[keep].view(np.int32), b[:n * width].reshape(n, width)[keep].view(np.int32))
    for s_out in out:
        assert (s_out[len(s_out) - G:] == (SENT_I if s_out.dtype == np.int32 else SENT_F)).all()
    for args in (dict(K=129), dict(NE=62), dict(jd=2), dict(its=65), dict(n=0)):
        a = dict(n=n, K=K, NE=NE, jd=1, its=12)
        a.update(args)
        rc = _lib.load().msmd_expression_fit(dev(r["y"]).data_ptr(), dev(r["subject"], torch.int32).data_ptr(), tab.data_ptr(),
                                             tab0.data_ptr(), w.data_ptr(), *[torch.zeros(8, device=DEV).data_ptr()] * 4, a["n"], a["K"],
                                             a["NE"], S, a["jd"], a["its"], 1e-6, 0.0, torch.cuda.current_stream().cuda_stream)
        assert rc == 1, args


def test_end_to_end_landmarks_to_style_clip(tmp_path):
    """Tracker-space landmarks from known (e, theta, head rotation, scale, translation) -> align_to_flame -> fit_expression ->
    save_expression_code -> query_for_motion_coeff.  The synthetic asset has no rigid landmarks (every vertex moves with the
    expression), so what comes back through the alignment is NOT compared with the generating code: shapes, dtypes and flags only."""
    from msmd_amd import inference
    from msmd_amd.utils.head_pose import save_head_rot, head_pose_from_landmarks
    fl = flame(50)
    g = np.random.default_rng(21)
    F = 12
    m = ER.model(50)
    fidx, bary = fl.full_lmk_faces_idx[0].cpu().numpy(), fl.full_lmk_bary_coords[0].cpu().numpy()
    shape = (0.5 * g.standard_normal(100)).astype(np.float32)
    e, th = 0.5 * g.standard_normal((F, 50)), np.array([[0.3, 0.0, 0.0]]) * g.random((F, 1))
    lm = ER.landmarks_full(m, fidx, bary, shape[None], e, th)
    ang = 0.3 * np.sin(np.linspace(0, 3, F))
    Ry = np.stack([np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) for a in ang])
    tracked = dev((3.0 * np.einsum("fij,fkj->fki", Ry, lm) + [0.5, 0.5, 0.0]).astype(np.float32))
    static = np.arange(0, 68, 4, dtype=np.int32)
    valid = np.ones(F, bool)
    valid[4] = False
    aligned = EF.align_to_flame(tracked, fl, shape, fidx, bary, static, valid)
    assert tuple(aligned.shape) == (F, 68, 3) and aligned.dtype == torch.float32 and torch.isfinite(aligned).all()
    code, det = EF.fit_expression(aligned, fl, shape, fidx, bary, jaw_dof=1, return_details=True)
    assert tuple(code.shape) == (F, 50) and code.dtype == torch.float32 and code.is_cuda and torch.isfinite(code).all()
    assert tuple(det["jaw"].shape) == (F, 3) and tuple(det["rms"].shape) == (F,) and det["status"].dtype == torch.int32
    report = EF.fit_report(det["rms"].cpu().numpy(), det["status"].cpu().numpy())
    print(f"end to end: {report}")
    assert report["flagged"] == 0 and report["frames"] == F
    neutral = EF.reduce_flame(fl, fidx, bary, shape)[1][0, :, :3].float()
    ypr = head_pose_from_landmarks(tracked, neutral, static, valid)
    EF.save_expression_code(str(tmp_path / "code.pkl"), code)
    save_head_rot(str(tmp_path / "head.pkl"), ypr)
    stats = dict(exp_mean=np.zeros(50, np.float32), exp_std=np.ones(50, np.float32), pose_mean=np.zeros(3, np.float32),
                 pose_std=np.ones(3, np.float32))
    with open(tmp_path / "stats.pkl", "wb") as f:
        pkl.dump(stats, f)
    coef, shp = inference.query_for_motion_coeff(SimpleNamespace(coef_dict_path=str(tmp_path / "stats.pkl")), str(tmp_path / "code.pkl"),
                                                 str(tmp_path / "head.pkl"), device=DEV, original_fps=25, target_fps=25)
    assert tuple(coef.shape) == (1, F, 53) and coef.dtype == torch.float32 and coef.is_cuda and tuple(shp.shape) == (1, 100)
    assert float((coef[0, :, :50] - code).abs().max()) <= 1e-6 * float(code.abs().max())      # (x - 0) / (1 + 1e-9)
