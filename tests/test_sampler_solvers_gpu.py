"""Few-step solvers on the HIP sampler (DDIM(eta), DPM-Solver++(2M); sampler.solver_table): the fused update kernel
against numpy, DDIM(eta = 1, S = T) against the DDPM chain, the sampler against a torch-CPU restatement on the real
schedule, hipGraph against eager, infer_coeffs against its own window loop, and step-count convergence."""
import math
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msmd_amd import synth
from msmd_amd.config import default_args

from helpers import denoiser_inputs, maxabs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


_MODELS = {}


def get_model(audio_model="wav2vec2", dtype="fp32", **kw):
    from msmd_amd.model import get_diffusion_model
    key = (audio_model, dtype, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS.clear()  # keep one model resident
        args = default_args(audio_model=audio_model, compute_dtype=dtype, **kw)
        _MODELS[key] = (get_diffusion_model(args, DEV).eval(), args)
    return _MODELS[key]


def zero_noise(B, L, dm, d):
    return torch.zeros(B, L, dm, device=d)


# ----------------------------------------------------------------------------- 1. the kernel
def solver_step_numpy(x, res, z, scales, d_prev, n_entries, L, mode, c):
    """fp32 restatement: the CFG combine of cfg_ddpm_step (in place into entry 0's head, model.py:407-415), then the
    solver update of msmd_cfg_solver_step."""
    p0, p1, ax, ath, b1, sg = (np.float32(v) for v in c)
    r = [e.copy() for e in np.split(res, n_entries, axis=0)]
    theta = r[0][:, -L:]
    for i in range(n_entries - 1):
        theta += scales[i] * (r[i + 1][:, -L:] - (r[0] if mode == 1 else r[i])[:, -L:])
    D = p0 * x + p1 * theta
    xn = ax * x + ath * theta + b1 * d_prev + (sg * z if z is not None else np.float32(0))
    return xn, D


def test_cfg_solver_step_matches_numpy():
    from msmd_amd import ops
    B, L, Lp, dm = 3, 37, 5, 67          # B L dm = 7437: not a multiple of the 256-thread block
    assert (B * L * dm) % 256
    forms = {"sample": (0.0, 1.0, 0.93, 0.21, -0.04, 0.11), "noise": (1.7, -1.3, 0.62, -0.35, 0.08, 0.0)}
    for n_entries in (1, 2, 3):
        scales = np.array([1.3, 0.9][:n_entries - 1], np.float32)
        for mode in (0, 1):
            res = synth.normalish(f"solv/res{n_entries}{mode}", (n_entries * B, Lp + L, dm))
            x = synth.normalish("solv/x", (B, L, dm))
            dp = synth.normalish("solv/dp", (B, L, dm))
            zz = synth.normalish("solv/z", (B, L, dm))
            for form, c in forms.items():
                for z in (zz, None):
                    ref_x, ref_d = solver_step_numpy(x, res, z, scales, dp, n_entries, L, mode, c)
                    sc = dev(scales) if n_entries > 1 else None
                    xt, dt = dev(x).clone(), dev(dp).clone()
                    ops.cfg_solver_step(xt, dev(res), dev(z) if z is not None else None, sc, dt, n_entries, Lp, mode, *c)
                    xd, dd = dev(x).clone(), dev(dp).clone()
                    coefs = torch.tensor(c, dtype=torch.float32, device=DEV)
                    ops.cfg_solver_step_dev(xd, dev(res), dev(z) if z is not None else None, sc, dd, coefs, n_entries, Lp,
                                            mode)
                    torch.cuda.synchronize()
                    what = (n_entries, mode, form, z is None)
                    assert maxabs(xt.cpu().numpy(), ref_x) <= 2e-6, what
                    assert maxabs(dt.cpu().numpy(), ref_d) <= 2e-6, what
                    assert torch.equal(xt, xd) and torch.equal(dt, dd), what


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_sampler_solver_select(dtype):
    from msmd_amd import ops
    S, d = 7, 300
    emb = torch.randn(S + 1, d, device=DEV).to(dtype)
    tab = torch.randn(S + 1, 6, device=DEV)
    i_dev = torch.full((1,), S, device=DEV, dtype=torch.int32)
    row, coefs = torch.zeros(d, device=DEV, dtype=dtype), torch.zeros(6, device=DEV)
    for i in range(S, 0, -1):
        ops.sampler_solver_select(emb, tab, i_dev, row, coefs)
        torch.cuda.synchronize()
        assert torch.equal(row, emb[i]) and torch.equal(coefs, tab[i]) and int(i_dev) == i - 1


# ----------------------------------------------------------------------------- 2. DDIM(1, S = T) == DDPM
@pytest.mark.parametrize("target", ["sample", "noise"])
def test_ddim_eta1_full_steps_equals_ddpm_sampler(target):
    """At S = T with eta = 1 DDIM is the DDPM posterior step (the coefficients agree to the rounding of the fp32 schedule,
    tests/test_sampler_solvers_cpu.py); the same injected noise keyed by timestep gives the same x_0 within 1e-5 of the
    output's scale.  For 'sample' |x_0| is a few units and the bound is 1e-5 absolute (measured 5.4e-6).  The untrained
    'noise'-target chain grows x to |x_0| ~ 3e3, where one fp32 ulp is 2.4e-4: an absolute 1e-5 would ask for less than
    an ulp, and the DDPM update c0 (x - c1 theta) and the folded ax x + ath theta round differently (measured 2.7e-3,
    8.6e-7 of |x_0|), so the same 1e-5 is applied relative to max |x_0| there."""
    T, B = 20, 2
    model, args = get_model("wav2vec2", "fp32", n_diff_steps=T, target=target)
    x = denoiser_inputs(B, args, tag="ddim1")
    xT = dev(synth.normalish("ddim1/xT", (B, 100, 67)))
    zs = {t: dev(synth.normalish(f"ddim1/z{t}", (B, 100, 67))) for t in range(2, T + 1)}
    common = lambda: (dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]), dev(x["prev_audio"]))
    ddpm, _, _ = model.sample(*common(), motion_at_T=xT, indicator=dev(x["indicator"]), noise=zs, cfg_scale=1.15)
    ddim, _, _ = model.sample(*common(), motion_at_T=xT, indicator=dev(x["indicator"]), noise=zs, cfg_scale=1.15,
                              sample_steps=T, solver="ddim", eta=1.0)
    torch.cuda.synchronize()
    err = float((ddpm - ddim).abs().max())
    print(f"DDIM(eta=1, S=T={T}) vs DDPM, target {target!r}: max-abs x0 difference {err:.3g} (|x0| max {float(ddpm.abs().max()):.3g})")
    assert torch.isfinite(ddim).all() and err <= 1e-5 * max(1.0, float(ddpm.abs().max()))


# ----------------------------------------------------------------------------- 3. against a torch-CPU restatement
def solver_rows_f64(ab, T, S, solver, eta):
    """(taus, [(a, b0, b1, sig)] per step i = S..1) from the formulas, independently of sampler.solver_table."""
    taus = [math.floor(i * T / S + 0.5) for i in range(S + 1)]
    al = lambda u: math.sqrt(ab[u])
    sg = lambda u: math.sqrt(1 - ab[u])
    lam = lambda u: 0.5 * math.log(ab[u] / (1 - ab[u]))
    out, h_prev = {}, None
    for i in range(S, 0, -1):
        s, t = taus[i], taus[i - 1]
        h = lam(t) - lam(s) if t > 0 else None
        if solver == "dpmpp_2m" and i < S and t > 0:
            r = h_prev / h
            out[i] = (sg(t) / sg(s), -al(t) * (math.exp(-h) - 1) * (1 + 1 / (2 * r)), al(t) * (math.exp(-h) - 1) / (2 * r), 0.0)
        else:
            e = eta if solver == "ddim" else 0.0
            sig = e * math.sqrt((1 - ab[t]) / (1 - ab[s])) * math.sqrt(1 - ab[s] / ab[t])
            a = math.sqrt(max(1 - ab[t] - sig ** 2, 0.0)) / sg(s)
            out[i] = (a, al(t) - a * al(s), 0.0, sig)
        h_prev = h
    return taus, out


_CPU_REFS = {}


def cpu_solver_reference(model, B, case):
    """oracle.torch_cpu.denoise_step per step (incremental CFG over [null, audio, audio + style], start tokens as the
    previous window), the CFG combine in place as the reference's, then x <- a x + b0 D + b1 D_prev + sig z in float64
    coefficients.  Cached per case and weights (the modes' models hold the same fp32 weights when their init is seeded)."""
    from oracle import torch_cpu as tc
    solver, eta, S = case
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    key = (case, tuple(float(v.double().sum()) for v in sd.values()))
    if key in _CPU_REFS:
        return _CPU_REFS[key]
    T = model.diffusion_sched.num_steps
    ab = model.diffusion_sched.alpha_bars.double().cpu().tolist()
    taus, co = solver_rows_f64(ab, T, S, solver, eta)
    af = synth.normalish("slv3/af", (B, 100, 512))
    style, xT = synth.normalish("slv3/style", (B, 256)), synth.normalish("slv3/xT", (B, 100, 67))
    shape, ind = np.zeros((B, 100), np.float32), np.ones((B, 100), np.float32)
    zs = {t: synth.normalish(f"slv3/z{t}", (B, 100, 67)) for t in taus[1:]}
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    x, d_prev = t_(xT), torch.zeros(B, 100, 67)
    with torch.no_grad():
        for i in range(S, 0, -1):
            res = tc.denoise_step(sd, x, t_(af), t_(shape), t_(style), taus[i], t_(ind), n_entries=3)
            e = [r.clone() for r in res.chunk(3, dim=0)]
            theta = e[0][:, -100:]
            theta += torch.tensor(1.15) * (e[1][:, -100:] - e[0][:, -100:])
            theta += torch.tensor(1.15) * (e[2][:, -100:] - e[1][:, -100:])
            a, b0, b1, sig = co[i]
            xn = (a * x.double() + b0 * theta.double() + b1 * d_prev.double()
                  + (sig * t_(zs[taus[i]]).double() if sig else 0.0))
            x, d_prev = xn.float(), theta.clone()
    _CPU_REFS[key] = (x.numpy(), dict(af=af, style=style, xT=xT, shape=shape, ind=ind, zs=zs))
    return _CPU_REFS[key]


@pytest.mark.parametrize("dtype", ["fp32", "f16x2", "fp16"])
def test_solvers_against_torch_cpu_on_real_schedule(dtype):
    """T = 500 cosine, B = 4, x_T and every draw injected; the three cases against the CPU restatement within
    config.PARITY_BOUNDS of the mode (1e-4 fp32 / f16x2, 2^-6 fp16)."""
    from msmd_amd.config import PARITY_BOUNDS
    B = 4
    model, args = get_model("wav2vec2", dtype)
    assert model.diffusion_sched.num_steps == 500 and model.target == "sample"
    for case in (("ddim", 0.0, 20), ("ddim", 1.0, 10), ("dpmpp_2m", 0.0, 10)):
        ref, inp = cpu_solver_reference(model, B, case)
        solver, eta, S = case
        x0, _, _ = model.sample(dev(inp["af"]), dev(inp["shape"]), dev(inp["style"]), motion_at_T=dev(inp["xT"]),
                                indicator=dev(inp["ind"]), cfg_scale=1.15, noise={t: dev(z) for t, z in inp["zs"].items()},
                                sample_steps=S, solver=solver, eta=eta)
        torch.cuda.synchronize()
        err = maxabs(x0.float().cpu().numpy(), ref)
        print(f"{solver}(eta={eta}) S={S} {dtype}: max-abs-err vs torch-CPU restatement {err:.3g} "
              f"(|x0| max {np.abs(ref).max():.3g}; bound {PARITY_BOUNDS[dtype]:.3g})")
        assert err < PARITY_BOUNDS[dtype], case


# ----------------------------------------------------------------------------- 4. graph == eager
def test_solver_hip_graph_matches_eager():
    """The captured solver loop (device-side step counter, 6-wide coefficient rows, per-lane d_prev) equals the eager loop
    bit for bit under the same noise (zeros: _step_noise patched), on one lane and on two, and with dynamic_threshold."""
    from msmd_amd import sampler as smp
    model, args = get_model("wav2vec2", "fp32", n_diff_steps=20)
    x = denoiser_inputs(2, args, tag="sg")
    xT = dev(synth.normalish("sg/xT", (2, 100, 67)))
    common = lambda scale=1.0: (dev(x["audio_feat"]) * scale, dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                dev(x["prev_audio"]))
    zeros = {t: torch.zeros(2, 100, 67, device=DEV) for t in range(0, 21)}
    cases = [dict(solver="ddim", eta=0.0, sample_steps=5), dict(solver="ddim", eta=1.0, sample_steps=7),
             dict(solver="dpmpp_2m", sample_steps=6),
             dict(solver="dpmpp_2m", sample_steps=4, cfg_scale=1.4, dynamic_threshold=(0.9, 0.5, 2.0))]
    try:
        for kw in cases:
            model.use_hip_graph = False
            eager, _, _ = model.sample(*common(), motion_at_T=xT, indicator=dev(x["indicator"]), noise=zeros, **kw)
            model.use_hip_graph = True
            for lanes in (1, 2):
                model.__dict__.pop("_step_graphs", None)
                with mock.patch.object(smp, "MIN_LANE_SEQS", 1), mock.patch.object(smp, "LANES", lanes), \
                        mock.patch.object(smp, "_step_noise", side_effect=zero_noise) as draws:
                    graph, _, _ = model.sample(*common(), motion_at_T=xT, indicator=dev(x["indicator"]), **kw)
                    g = next(iter(model._step_graphs.values()))
                    assert g.lanes == lanes and g.k <= kw["sample_steps"] and kw["sample_steps"] % g.k == 0
                    assert draws.called == (kw.get("eta", 0.0) > 0)       # deterministic solvers draw nothing
                    assert torch.equal(eager, graph), (kw, lanes)
                    # a second call re-uses the cached graph with new operands
                    again, _, _ = model.sample(*common(0.5), motion_at_T=xT, indicator=dev(x["indicator"]), **kw)
                    assert next(iter(model._step_graphs.values())) is g
            model.use_hip_graph = False
            ref, _, _ = model.sample(*common(0.5), motion_at_T=xT, indicator=dev(x["indicator"]), noise=zeros, **kw)
            model.use_hip_graph = True
            assert torch.equal(again, ref), kw
            assert not torch.equal(again, graph)
        # ret_traj: {taus[i]: x}
        traj, _, _ = model.sample(*common(), motion_at_T=xT, indicator=dev(x["indicator"]), ret_traj=True, noise=zeros,
                                  **cases[2])
        assert sorted(traj) == [0, 3, 7, 10, 13, 17, 20]
    finally:
        model.__dict__.pop("use_hip_graph", None)
        model.__dict__.pop("_step_graphs", None)


# ----------------------------------------------------------------------------- 5. infer_coeffs
def test_infer_coeffs_with_solver_equals_its_window_loop():
    from msmd_amd.inference import infer_coeffs, window_plan
    model, args = get_model("wav2vec2", "fp32", n_diff_steps=20)
    L, keep = args.n_motions, args.n_prev_motions
    n = 160000                                    # 2.5 windows
    _, _, n_win, pad, pad_frames = window_plan(n, args.fps, L, 640.0)
    assert n_win == 3 and pad_frames > 0
    audio = dev(synth.audio_clips(1, n, tag="slv5")[0])
    style = dev(synth.normalish("slv5/style", (1, args.d_style)))
    shape = torch.zeros(1, 1, 100, device=DEV)
    S = 5
    taus = [math.floor(i * 20 / S + 0.5) for i in range(S + 1)]
    noise = dict(xT=dev(synth.normalish("slv5/xT", (1, 100, 67))),
                 z=[{t: dev(synth.normalish(f"slv5/z{w}_{t}", (1, 100, 67))) for t in taus[1:]} for w in range(n_win)])
    kw = dict(sample_steps=S, solver="ddim", eta=1.0)
    y = infer_coeffs(model, args, audio, shape, 640.0, style, cfg_scale=1.4, dynamic_threshold=None, noise=noise, **kw)
    # by hand: one encoder pass over the padded clip, window w conditioned on window w - 1's last frames, window 0's x_T
    feats = model.extract_audio_feature(F.pad(audio, (0, pad)).unsqueeze(0), L * n_win).split(L, dim=1)
    hist, pieces = (None, None, noise["xT"]), []
    for w, f in enumerate(feats):
        ind = torch.ones(1, L, device=DEV)
        if w == n_win - 1:
            ind[:, L - pad_frames:] = 0
        x0, xT, fu = model.sample(f, shape, style, *hist, indicator=ind, cfg_scale=1.4, noise=noise["z"][w], **kw)
        hist = (x0[:, -keep:].clone(), fu[:, -keep:], xT)
        pieces.append(x0[:, :L - pad_frames] if w == n_win - 1 else x0)
    want = torch.cat(pieces, dim=1)
    assert y.shape == want.shape == (1, int(n / 16000 * args.fps), 67)
    assert torch.equal(y, want)
    # deterministic DPM-Solver++(2M) on the hipGraph path: the same bits twice under the same seed (only x_T is drawn)
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        runs.append(infer_coeffs(model, args, audio, shape, 640.0, style, sample_steps=4, solver="dpmpp_2m"))
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])


# ----------------------------------------------------------------------------- 6. step-count convergence
def test_step_count_convergence_reported():
    """Distance of x_0 at S steps from the same deterministic solver at S = T = 500 (fp32, fixed x_T, B = 2).  The
    weights are synthetic (no trained checkpoint), so only the direction is asserted: 250 steps land closer than 25."""
    model, args = get_model("wav2vec2", "fp32")
    x = denoiser_inputs(2, args, tag="conv")
    xT = dev(synth.normalish("conv/xT", (2, 100, 67)))
    run = lambda **kw: model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                    dev(x["prev_audio"]), motion_at_T=xT, indicator=dev(x["indicator"]), **kw)[0]
    table = {}
    for solver in ("ddim", "dpmpp_2m"):
        ref = run(sample_steps=500, solver=solver).clone()
        table[solver] = {S: float((run(sample_steps=S, solver=solver) - ref).abs().max()) for S in (25, 50, 100, 250)}
    print("max-abs distance of x0 from S = 500:")
    for solver, row in table.items():
        print(f"  {solver:9s} " + "  ".join(f"S={S}: {d:.3g}" for S, d in row.items()))
    for solver, row in table.items():
        assert all(math.isfinite(d) for d in row.values())
        assert row[250] < row[25], solver
