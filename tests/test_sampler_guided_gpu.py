"""Few-step solvers with keyframe guidance and stream separation: the guided pack kernel and the streams step against their
neighbours and a float64 restatement, the sampler against CPU restatements, hipGraph against eager, infer_coeffs with
keyframes against its own window loop, and the DDPM defaults of the two entry points."""
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


# ----------------------------------------------------------------------------- 1. the guided pack kernel
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("with_ind", [True, False])
def test_guided_pack_equals_pack_of_overwritten_input(out_dtype, with_ind):
    from msmd_amd import ops
    from msmd_amd._lib import MsmdLibraryError
    B, E, L, Lp, dm, Kpad = 2, 3, 37, 5, 67, 80
    N = B * E
    x = dev(synth.normalish("gp/x", (B, L, dm)))
    prev = dev(synth.normalish("gp/prev", (N, Lp, dm)))
    ind = dev((synth.normalish("gp/ind", (N, L)) > 0).astype(np.float32)) if with_ind else None
    vals = dev(synth.normalish("gp/vals", (B, L, dm)))
    for pins in ([[0, 10, L - 1], [3]], [[0, L - 1], []], [[], []], [list(range(L)), [L - 1]]):
        mask = torch.zeros(B, L, dtype=torch.uint8, device=DEV)
        for b, frames in enumerate(pins):
            mask[b, frames] = 1
        over = x.clone()
        for b, frames in enumerate(pins):
            over[b, frames] = vals[b, frames]
        want = torch.full((N, 1 + Lp + L, Kpad), 7.0, device=DEV, dtype=out_dtype)
        got = torch.full((N, 1 + Lp + L, Kpad), -3.0, device=DEV, dtype=out_dtype)
        ops.denoiser_pack_input(over, prev, ind, want)
        ops.denoiser_pack_input_guided(x, prev, ind, got, mask, vals)
        torch.cuda.synchronize()
        assert torch.equal(got, want), pins
    # no mask: the plain call
    ops.denoiser_pack_input(x, prev, ind, want)
    ops.denoiser_pack_input_guided(x, prev, ind, got, None, None)
    assert torch.equal(got, want)
    # the q-sample form takes no keyframes
    c = torch.ones(B, device=DEV)
    with pytest.raises(MsmdLibraryError):
        ops.denoiser_pack_input_guided(x, prev, ind, got, mask, vals, eps=torch.zeros_like(x), c0=c, c1=c)


# ----------------------------------------------------------------------------- 2. the streams step
def streams_f64(x, dec, stat, res, scales, cum, n_entries, B, L, Lp, dm, nb, uha, mode, ath):
    """float64 restatement of the three streams on the same fp32 (or bf16) inputs; every quantity is returned with its
    magnitude twin (the same expression with each term replaced by its absolute value), which scales the error bound."""
    f = lambda a: np.asarray(a, np.float64)
    dec, stat = f(dec)[:, -L:], f(stat)
    per = []
    for e in range(n_entries):
        d = dec[e * B:(e + 1) * B]
        a = d[..., dm:]
        if uha & 2:
            a = 1.0 / (1.0 + np.exp(-a))
        s = stat[(np.arange(e * B, (e + 1) * B)) % stat.shape[0]]                 # (B, nb, dm)
        w = np.einsum("bln,bnk->blk", a, s)
        wa = np.einsum("bln,bnk->blk", np.abs(a), np.abs(s))
        plain, pa = s.sum(axis=1)[:, None, :], np.abs(s).sum(axis=1)[:, None, :]
        static, sabs = w.copy(), wa.copy()
        if not uha & 1:
            static[..., -3:] = np.broadcast_to(plain, w.shape)[..., -3:]
            sabs[..., -3:] = np.broadcast_to(pa, w.shape)[..., -3:]
        per.append(dict(static=(static, sabs), dyn=(d[..., :dm], np.abs(d[..., :dm])), alpha=(a, np.abs(a))))
    out = {}
    for name in ("static", "dyn", "alpha"):
        th, ab = (v.copy() for v in per[0][name])
        for e in range(1, n_entries):
            hi, hia = per[e][name]
            lo, loa = (th, ab) if (mode == 1 or e == 1) else per[e - 1][name]
            th, ab = th + float(scales[e - 1]) * (hi - lo), ab + abs(float(scales[e - 1])) * (hia + loa)
        out[name] = (th, ab)
    st, sta = out["static"]
    out["cum"] = (f(cum) + float(ath) * st, np.abs(f(cum)) + abs(float(ath)) * sta)
    return out


@pytest.mark.parametrize("dec_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_entries", [1, 2, 3])
def test_streams_step(dec_dtype, n_entries):
    """x / d_prev: the bits of cfg_solver_step on the same res, host form == device form.  theta_dyn, cum_static, theta_alpha:
    within 32 * 2^-24 * (the float64 restatement with every term replaced by its absolute value) per element -- a running
    error bound for the <= 24 fp32 operations behind one output (2 nb for the static sum, 3 per CFG term, 2 for the
    accumulation; the sigmoid's expf and division are a few ulp of a value below 1)."""
    from msmd_amd import ops
    B, L, Lp, dm, nb, S = 3, 37, 5, 67, 4, 4
    assert (B * L * dm) % 256
    N = n_entries * B
    coef = (0.3, 0.8, 0.93, 0.21, -0.04, 0.11)
    scales = np.array([1.3, 0.9][:n_entries - 1], np.float32)
    sc = dev(scales) if n_entries > 1 else None
    x0, dp0, z0 = (dev(synth.normalish(f"st/{n}", (B, L, dm))) for n in ("x", "dp", "z"))
    cum0 = dev(synth.normalish("st/cum", (B, L, dm)))
    dec = dev(synth.normalish(f"st/dec{n_entries}", (N, Lp + L, dm + nb))).to(dec_dtype)
    for stat_batch in (1, B):
        stat = dev(synth.normalish(f"st/stat{stat_batch}", (stat_batch, nb, dm))).to(dec_dtype)
        for uha in (0, 1, 3):
            res = ops.heads_static_mix(dec, stat, Lp + L, dm, nb, bool(uha & 1), bool(uha & 2))
            for mode in (0, 1):
                for z in (z0, None):
                    for n_slots, slot in ((1, 0), (S, 2)):
                        what = (stat_batch, uha, mode, z is None, n_slots)
                        xs, ds = x0.clone(), dp0.clone()
                        ops.cfg_solver_step(xs, res, z, sc, ds, n_entries, Lp, mode, *coef)
                        outs = []
                        for form in ("host", "dev"):
                            xt, dt, cum = x0.clone(), dp0.clone(), cum0.clone()
                            thd = torch.full((B, L, dm), 9.0, device=DEV)
                            tha = torch.full((n_slots * B, L, nb), 9.0, device=DEV)
                            if form == "host":
                                ops.cfg_streams_step(xt, res, dec, stat, z, sc, dt, cum, thd, tha, slot, n_entries, Lp, nb,
                                                     uha, mode, *coef)
                            else:
                                # step i = S - slot; msmd_sampler_solver_select has left i - 1 in the counter
                                counter = torch.tensor([S - slot - 1], dtype=torch.int32, device=DEV)
                                ops.cfg_streams_step_dev(xt, res, dec, stat, z, sc, dt, cum, thd, tha,
                                                         torch.tensor(coef, device=DEV), counter, n_entries, Lp, nb, uha, mode)
                            torch.cuda.synchronize()
                            assert torch.equal(xt, xs) and torch.equal(dt, ds), (what, form)
                            outs.append((cum, thd, tha))
                        for a, b in zip(*outs):
                            assert torch.equal(a, b), what
                        cum, thd, tha = outs[0]
                        ref = streams_f64(x0.cpu(), dec.float().cpu(), stat.float().cpu(), res.cpu(), scales, cum0.cpu(),
                                          n_entries, B, L, Lp, dm, nb, uha, mode, np.float32(coef[3]))
                        block = tha[slot * B:(slot + 1) * B]
                        others = torch.cat([tha[:slot * B], tha[(slot + 1) * B:]])
                        assert bool((others == 9.0).all()), what                  # the other slots are untouched
                        for name, got in (("dyn", thd), ("cum", cum), ("alpha", block)):
                            val, mag = ref[name]
                            if name == "alpha":
                                val, mag = val[..., :nb], mag[..., :nb]
                            err = np.abs(got.double().cpu().numpy() - val)
                            bound = 32 * 2.0 ** -24 * mag
                            assert (err <= bound).all(), (what, name, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))


# ----------------------------------------------------------------------------- restated solver rows
def solver_rows_f64(ab, T, S, solver, eta):
    """(taus, {i: (a, b0, b1, sig)}) from the formulas, independently of sampler.solver_table."""
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


# ----------------------------------------------------------------------------- 3. guided few-step against a CPU restatement
_CPU_REFS = {}
KEYFRAMES = ([0, 1, 50, 99], [7])                         # frames pinned in clip 0 / clip 1


def cpu_guided_reference(model, B, case):
    """The step loop of the unguided solver test's CPU reference (oracle.torch_cpu.denoise_step per step, CFG combine in place,
    x <- a x + b0 D + b1 D_prev + sig z in float64 coefficients) with the denoiser INPUT overwritten at the keyframes before
    every call (reference model.py:762-767); x itself is not overwritten."""
    from oracle import torch_cpu as tc
    solver, eta, S = case
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    key = (case, tuple(float(v.double().sum()) for v in sd.values()))
    if key in _CPU_REFS:
        return _CPU_REFS[key]
    T = model.diffusion_sched.num_steps
    ab = model.diffusion_sched.alpha_bars.double().cpu().tolist()
    taus, co = solver_rows_f64(ab, T, S, solver, eta)
    af = synth.normalish("gd3/af", (B, 100, 512))
    style, xT = synth.normalish("gd3/style", (B, 256)), synth.normalish("gd3/xT", (B, 100, 67))
    shape, ind = np.zeros((B, 100), np.float32), np.ones((B, 100), np.float32)
    zs = {t: synth.normalish(f"gd3/z{t}", (B, 100, 67)) for t in taus[1:]}
    kv = [synth.normalish(f"gd3/kv{b}", (len(fr), 67)) for b, fr in enumerate(KEYFRAMES)]
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    x, d_prev = t_(xT), torch.zeros(B, 100, 67)
    with torch.no_grad():
        for i in range(S, 0, -1):
            x_in = x.clone()
            for b, fr in enumerate(KEYFRAMES):
                x_in[b, fr] = t_(kv[b])
            res = tc.denoise_step(sd, x_in, t_(af), t_(shape), t_(style), taus[i], t_(ind), n_entries=3)
            e = [r.clone() for r in res.chunk(3, dim=0)]
            theta = e[0][:, -100:]
            theta += torch.tensor(1.15) * (e[1][:, -100:] - e[0][:, -100:])
            theta += torch.tensor(1.15) * (e[2][:, -100:] - e[1][:, -100:])
            a, b0, b1, sig = co[i]
            xn = (a * x.double() + b0 * theta.double() + b1 * d_prev.double()
                  + (sig * t_(zs[taus[i]]).double() if sig else 0.0))
            x, d_prev = xn.float(), theta.clone()
    _CPU_REFS[key] = (x.numpy(), dict(af=af, style=style, xT=xT, shape=shape, ind=ind, zs=zs, kv=kv))
    return _CPU_REFS[key]


@pytest.mark.parametrize("dtype", ["fp32", "f16x2", "fp16"])
def test_guided_solvers_against_torch_cpu_on_real_schedule(dtype):
    """T = 500 cosine, B = 2, keyframes at frames 0, 1, 50, 99 of clip 0 and frame 7 of clip 1, x_T and every draw injected;
    within config.PARITY_BOUNDS of the mode, the bounds of the unguided solver test."""
    from msmd_amd.config import PARITY_BOUNDS
    from msmd_amd.sampler import DenseGuide
    B = 2
    model, args = get_model("wav2vec2", dtype)
    assert model.diffusion_sched.num_steps == 500 and model.target == "sample"
    for case in (("dpmpp_2m", 0.0, 6), ("ddim", 1.0, 5)):
        ref, inp = cpu_guided_reference(model, B, case)
        solver, eta, S = case
        guide = DenseGuide.stack([(fr, inp["kv"][b]) for b, fr in enumerate(KEYFRAMES)], 100, 67)
        x0, _, _ = model.sample_with_guide(dev(inp["af"]), dev(inp["shape"]), dev(inp["style"]), motion_at_T=dev(inp["xT"]),
                                           indicator=dev(inp["ind"]), cfg_scale=1.15, guidance_indice=guide,
                                           noise={t: dev(z) for t, z in inp["zs"].items()}, sample_steps=S, solver=solver,
                                           eta=eta)
        plain, _, _ = model.sample(dev(inp["af"]), dev(inp["shape"]), dev(inp["style"]), motion_at_T=dev(inp["xT"]),
                                   indicator=dev(inp["ind"]), cfg_scale=1.15, noise={t: dev(z) for t, z in inp["zs"].items()},
                                   sample_steps=S, solver=solver, eta=eta)
        torch.cuda.synchronize()
        err = maxabs(x0.float().cpu().numpy(), ref)
        print(f"guided {solver}(eta={eta}) S={S} {dtype}: max-abs-err vs torch-CPU restatement {err:.3g} "
              f"(|x0| max {np.abs(ref).max():.3g}; bound {PARITY_BOUNDS[dtype]:.3g}; moved by the keyframes "
              f"{float((x0 - plain).abs().max()):.3g})")
        assert err < PARITY_BOUNDS[dtype], case
        assert not torch.equal(x0, plain)                                   # the keyframes do reach the denoiser


# ----------------------------------------------------------------------------- 4. separated few-step
def oracle_separate_fewstep(sd, ab, x, xT, zs, solver, eta, S, cfg_scale, T):
    """sample_separate on a few-step solver restated on the numpy oracle: oracle.diffusion.denoising_net(keep_separate=True) on
    the [null, audio, audio + style] entries of incremental CFG, the in-place CFG combine of every stream, float64 solver
    coefficients, cum_static += ath theta_static (ath = b0 for target 'sample')."""
    from oracle import diffusion as od
    f32 = np.float32
    taus, co = solver_rows_f64(ab, T, S, solver, eta)
    B = xT.shape[0]
    shape, style = x["shape"][:, None], x["style"][:, None]
    null_a = np.broadcast_to(sd["null_audio_feat"], x["audio_feat"].shape)
    null_s = np.broadcast_to(sd["null_style_feat"], style.shape)
    audio_in = np.concatenate([null_a, x["audio_feat"], x["audio_feat"]], 0).astype(f32)
    person_in = np.concatenate([np.concatenate([shape, s], -1) for s in (null_s, null_s, style)], 0).astype(f32)
    rep = lambda v: np.concatenate([v] * 3, 0).astype(f32)
    cur, d_prev, cum = xT.astype(f32), np.zeros_like(xT, dtype=f32), np.zeros(xT.shape, np.float64)
    alphas = []
    for i in range(S, 0, -1):
        dyn, static4, alpha = od.denoising_net(sd, rep(cur), audio_in, person_in, rep(style), rep(x["prev_motion"]),
                                               rep(x["prev_audio"]), np.full((3 * B,), taus[i]), rep(x["indicator"]),
                                               keep_separate=True, n_diff_steps=T)
        static = np.concatenate([(static4[..., :-3] * alpha[..., None]).sum(axis=2), static4[..., -3:].sum(axis=2)], axis=-1)
        streams = [[r.copy() for r in np.split(v.astype(f32), 3, axis=0)] for v in (dyn + static, static, dyn, alpha)]
        heads = [st[0][:, -100:] for st in streams]
        for e in range(2):
            for st, hd in zip(streams, heads):
                hd += f32(cfg_scale) * (st[e + 1][:, -100:] - st[e][:, -100:])
        theta, th_static, th_dyn, th_alpha = heads
        a, b0, b1, sig = co[i]
        z = zs[taus[i]].astype(np.float64) if sig else 0.0
        nxt = a * cur.astype(np.float64) + b0 * theta.astype(np.float64) + b1 * d_prev.astype(np.float64) + sig * z
        cum = cum + b0 * th_static.astype(np.float64)
        cur, d_prev = nxt.astype(f32), theta.copy()
        alphas.append(th_alpha.copy())
    return cur, th_dyn, cum.astype(f32), th_alpha, alphas


def test_separated_fewstep():
    """(a) DDIM(eta = 1, S = T) against oracle.diffusion.sample(separate=True); (b) DPM-Solver++(2M), S = 4, against the float64
    restatement; (c) x0 of sample_separate(solver) has the bits of sample(solver); (d) return_all_alpha keeps S B rows in
    step order.  All within PARITY_BOUNDS['fp32']."""
    from msmd_amd.config import PARITY_BOUNDS
    from oracle import diffusion as od
    T, B = 20, 2
    bound = PARITY_BOUNDS["fp32"]
    model, args = get_model("wav2vec2", "fp32", n_diff_steps=T)
    sd = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    ab = model.diffusion_sched.alpha_bars.double().cpu().tolist()
    x = denoiser_inputs(B, args, tag="sep4")
    xT = synth.normalish("sep4/xT", (B, 100, 67))
    zs = {t: synth.normalish(f"sep4/z{t}", (B, 100, 67)) for t in range(1, T + 1)}
    common = lambda: (dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]), dev(x["prev_audio"]))
    kw = dict(motion_at_T=dev(xT), indicator=dev(x["indicator"]), cfg_scale=1.15, noise={t: dev(z) for t, z in zs.items()})

    def check(got, want, what):
        for g, w, name in zip(got, want, ("x0", "dyn", "static", "alpha")):
            err = maxabs(g.cpu().numpy(), w)
            print(f"{what}: {name} max-abs-err {err:.3g} (max |.| {np.abs(w).max():.3g}; bound {bound:.3g})")
            assert g.shape == w.shape and err < bound, (what, name, err)

    # (a)
    ref = od.sample(sd, od.diffusion_schedule(T, "cosine"), x["audio_feat"], x["shape"], x["style"], xT, zs, x["prev_motion"],
                    x["prev_audio"], x["indicator"], cfg_scale=1.15, separate=True, n_diff_steps=T)
    r = model.sample_separate(*common(), sample_steps=T, solver="ddim", eta=1.0, **kw)
    assert len(r) == 6
    check((r[0], r[3], r[4], r[5]), ref, "ddim(eta=1) S=T vs oracle.sample(separate=True)")
    plain, _, _ = model.sample(*common(), sample_steps=T, solver="ddim", eta=1.0, **kw)
    assert torch.equal(r[0], plain)                                                             # (c)
    # (b)
    ref = oracle_separate_fewstep(sd, ab, x, xT, zs, "dpmpp_2m", 0.0, 4, 1.15, T)
    r = model.sample_separate(*common(), sample_steps=4, solver="dpmpp_2m", **kw)
    check((r[0], r[3], r[4], r[5]), ref[:4], "dpmpp_2m S=4 vs float64 restatement")
    plain, _, _ = model.sample(*common(), sample_steps=4, solver="dpmpp_2m", **kw)
    assert torch.equal(r[0], plain)                                                             # (c)
    # (d)
    ra = model.sample_separate(*common(), sample_steps=4, solver="dpmpp_2m", return_all_alpha=True, **kw)
    assert tuple(ra[5].shape) == (4 * B, 100, 4) and torch.equal(ra[5][-B:], r[5])
    assert torch.equal(ra[0], r[0]) and torch.equal(ra[3], r[3]) and torch.equal(ra[4], r[4])
    for s_, want in enumerate(ref[4]):
        assert maxabs(ra[5][s_ * B:(s_ + 1) * B].cpu().numpy(), want) < bound, s_
    # guidance and separation together: x0 has the bits of the guided call
    gv = dev(synth.normalish("sep4/gv", (3, 67)))
    from msmd_amd import sampler as smp
    g_only = model.sample_with_guide(*common(), guidance_indice=[0, 40, 99], guidance_values=gv, sample_steps=4,
                                     solver="dpmpp_2m", **kw)[0]
    both = smp.sample(model, *common(), guidance=([0, 40, 99], gv), separate=dict(alpha_mod=None, return_all_alpha=False),
                      sample_steps=4, solver="dpmpp_2m", **kw)
    assert len(both) == 6 and torch.equal(both[0], g_only) and not torch.equal(g_only, plain)


# ----------------------------------------------------------------------------- 5. graph == eager
def test_guided_and_separated_hip_graph_matches_eager():
    """The captured loop with keyframes and / or streams equals the eager loop bit for bit under the same noise (zeros:
    _step_noise patched), on one lane and on two; other keyframes re-use the captured graph; alpah_t_modification runs eagerly."""
    from msmd_amd import sampler as smp
    from msmd_amd.sampler import DenseGuide
    model, args = get_model("wav2vec2", "fp32", n_diff_steps=20)
    B = 2
    x = denoiser_inputs(B, args, tag="gg")
    xT = dev(synth.normalish("gg/xT", (B, 100, 67)))
    common = lambda: (dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]), dev(x["prev_audio"]))
    zeros = {t: torch.zeros(B, 100, 67, device=DEV) for t in range(0, 21)}
    kv = lambda tag, n: synth.normalish(f"gg/kv{tag}", (n, 67))
    guide_a = DenseGuide.stack([([0, 1, 50, 99], kv("a0", 4)), ([7], kv("a1", 1))], 100, 67)
    guide_b = DenseGuide.stack([([33], kv("b0", 1)), ([2, 98, 60], kv("b1", 3))], 100, 67)
    sep = lambda **k: dict(alpha_mod=None, return_all_alpha=False, **k)
    cases = [
        (dict(solver="dpmpp_2m", sample_steps=6), True, None),
        (dict(solver="ddim", eta=0.0, sample_steps=5), False, dict(alpha_mod=None, return_all_alpha=True)),
        (dict(solver="dpmpp_2m", sample_steps=4, cfg_scale=1.4, dynamic_threshold=(0.9, 0.5, 2.0)), True, sep()),
    ]

    def run(kw, guide, separate, **extra):
        out = smp.sample(model, *common(), motion_at_T=xT, indicator=dev(x["indicator"]),
                         guidance=(guide, None) if guide is not None else None, separate=separate, **kw, **extra)
        return (out[0],) + tuple(out[3:])

    try:
        for kw, guided, separate in cases:
            ga, gb = (guide_a, guide_b) if guided else (None, None)
            model.use_hip_graph = False
            eager = run(kw, ga, separate, noise=zeros)
            eager_b = run(kw, gb, separate, noise=zeros) if guided else None
            assert len(eager) == (4 if separate else 1)
            model.use_hip_graph = True
            for lanes in (1, 2):
                model.__dict__.pop("_step_graphs", None)
                with mock.patch.object(smp, "MIN_LANE_SEQS", 1), mock.patch.object(smp, "LANES", lanes), \
                        mock.patch.object(smp, "_step_noise", side_effect=zero_noise):
                    graph = run(kw, ga, separate)
                    g = next(iter(model._step_graphs.values()))
                    assert g.lanes == lanes and kw["sample_steps"] % g.k == 0
                    for a, b in zip(eager, graph):
                        assert a.shape == b.shape and torch.equal(a, b), (kw, lanes)
                    if guided:
                        # other keyframe positions and values: the same captured graph, its eager twin's bits
                        again = run(kw, gb, separate)
                        assert len(model._step_graphs) == 1 and next(iter(model._step_graphs.values())) is g
                        for a, b in zip(eager_b, again):
                            assert torch.equal(a, b), (kw, lanes)
                        assert not torch.equal(again[0], graph[0])
        # alpah_t_modification: an arbitrary host callable, so the eager loop.  Halving is exact in fp32, so after ONE step the
        # blend weights and the weighted (face) columns of the static stream are exactly half of the unmodified call's, the
        # unweighted head-pose columns and the dynamic stream are unchanged.
        model.__dict__.pop("_step_graphs", None)
        calls = []
        halve = lambda a: (calls.append(tuple(a.shape)), a * 0.5)[1]
        base = model.sample_separate(*common(), motion_at_T=xT, indicator=dev(x["indicator"]), sample_steps=1, solver="ddim",
                                     noise=zeros)
        mod = model.sample_separate(*common(), motion_at_T=xT, indicator=dev(x["indicator"]), sample_steps=1, solver="ddim",
                                    alpah_t_modification=halve)
        assert not model.__dict__.get("_step_graphs") and calls == [(3 * B, 110, 4)]
        assert not model.denoising_net.use_head_alpha
        assert torch.equal(mod[5], base[5] * 0.5) and torch.equal(mod[3], base[3])
        assert torch.equal(mod[4][..., :-3], base[4][..., :-3] * 0.5) and torch.equal(mod[4][..., -3:], base[4][..., -3:])
        more = model.sample_separate(*common(), motion_at_T=xT, indicator=dev(x["indicator"]), sample_steps=3,
                                     solver="dpmpp_2m", alpah_t_modification=halve)
        assert not model.__dict__.get("_step_graphs") and len(calls) == 4 and all(torch.isfinite(v).all() for v in more[3:])
    finally:
        model.__dict__.pop("use_hip_graph", None)
        model.__dict__.pop("_step_graphs", None)


# ----------------------------------------------------------------------------- 6. infer_coeffs with keyframes
def test_infer_coeffs_with_keyframes_equals_its_window_loop():
    from msmd_amd.inference import infer_coeffs, infer_coeffs_batch, window_plan
    model, args = get_model("wav2vec2", "fp32", n_diff_steps=20)
    L, keep = args.n_motions, args.n_prev_motions
    n = 160000                                    # 10 s: clip_len 250, 2.5 windows
    clip_len, _, n_win, pad, pad_frames = window_plan(n, args.fps, L, 640.0)
    assert (clip_len, n_win) == (250, 3) and pad_frames > 0
    audio = dev(synth.audio_clips(1, n, tag="kf6")[0])
    style = dev(synth.normalish("kf6/style", (1, args.d_style)))
    shape = torch.zeros(1, 1, 100, device=DEV)
    frames, vals = [3, 99, 100, 249], dev(synth.normalish("kf6/vals", (4, 67)))
    noise = dict(xT=dev(synth.normalish("kf6/xT", (1, 100, 67))), z=[{} for _ in range(n_win)])   # dpmpp_2m draws nothing
    kw = dict(sample_steps=4, solver="dpmpp_2m")
    y = infer_coeffs(model, args, audio, shape, 640.0, style, cfg_scale=1.4, dynamic_threshold=None, noise=noise,
                     keyframes=(frames, vals), **kw)
    feats = model.extract_audio_feature(F.pad(audio, (0, pad)).unsqueeze(0), L * n_win).split(L, dim=1)
    local = [([3, 99], vals[:2]), ([0], vals[2:3]), ([49], vals[3:])]
    hist, pieces = (None, None, noise["xT"]), []
    for w, f in enumerate(feats):
        ind = torch.ones(1, L, device=DEV)
        if w == n_win - 1:
            ind[:, L - pad_frames:] = 0
        x0, xT, fu = model.sample_with_guide(f, shape, style, *hist, indicator=ind, cfg_scale=1.4, noise={},
                                             guidance_indice=local[w][0], guidance_values=local[w][1], **kw)
        hist = (x0[:, -keep:].clone(), fu[:, -keep:], xT)
        pieces.append(x0[:, :L - pad_frames] if w == n_win - 1 else x0)
    want = torch.cat(pieces, dim=1)
    assert y.shape == want.shape == (1, clip_len, 67)
    assert torch.equal(y, want)
    unpinned = infer_coeffs(model, args, audio, shape, 640.0, style, cfg_scale=1.4, dynamic_threshold=None, noise=noise, **kw)
    assert not torch.equal(y, unpinned)
    with pytest.raises(IndexError):
        infer_coeffs(model, args, audio, shape, 640.0, style, keyframes=([clip_len], vals[:1]), **kw)
    # two clips, one of them without keyframes: the per-clip calls
    short = dev(synth.audio_clips(1, 64000, tag="kf6s")[0])
    styles = torch.cat([style, dev(synth.normalish("kf6/style2", (1, args.d_style)))])
    noise2 = dict(xT=dev(synth.normalish("kf6/xT2", (1, 100, 67))), z=[{}])
    ys = infer_coeffs_batch(model, args, [audio, short], torch.zeros(2, 100, device=DEV), 640.0, styles, cfg_scale=1.4,
                            dynamic_threshold=None, noise=[noise, noise2], keyframes=[(frames, vals), None], **kw)
    y2 = infer_coeffs(model, args, short, torch.zeros(1, 100, device=DEV), 640.0, styles[1:], cfg_scale=1.4,
                      dynamic_threshold=None, noise=noise2, **kw)
    y1 = infer_coeffs(model, args, audio, torch.zeros(1, 100, device=DEV), 640.0, styles[:1], cfg_scale=1.4,
                      dynamic_threshold=None, noise=noise, keyframes=(frames, vals), **kw)
    assert torch.equal(ys[0], y1) and torch.equal(ys[1], y2)


# ----------------------------------------------------------------------------- 7. the defaults
def test_defaults_of_guided_and_separated_calls_are_untouched():
    """Without the new arguments both entry points are the DDPM chain in the eager loop: the bits of sampler.sample(guidance= /
    separate=) with use_hip_graph off, and no graph is captured when the noise is drawn."""
    from msmd_amd import sampler as smp
    from msmd_amd.model import DiffusionSchedule
    model, args = get_model("wav2vec2", "fp32", n_diff_steps=20)
    B, T = 2, 3
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(T, "cosine").to(DEV)
    x = denoiser_inputs(B, args, tag="df")
    xT = dev(synth.normalish("df/xT", (B, 100, 67)))
    zs = {t: dev(synth.normalish(f"df/z{t}", (B, 100, 67))) for t in range(1, T + 1)}
    common = lambda: (dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]), dev(x["prev_audio"]))
    kw = dict(motion_at_T=xT, indicator=dev(x["indicator"]), cfg_scale=1.3)
    idx, gv = [0, 5, 99], dev(synth.normalish("df/gv", (3, 67)))
    try:
        model.__dict__.pop("_step_graphs", None)
        got = model.sample_with_guide(*common(), guidance_indice=idx, guidance_values=gv, noise=zs, **kw)
        sep = model.sample_separate(*common(), noise=zs, return_all_alpha=True, **kw)
        model.use_hip_graph = False
        want = smp.sample(model, *common(), noise=zs, guidance=(idx, gv), **kw)
        want_sep = smp.sample(model, *common(), noise=zs, separate=dict(alpha_mod=None, return_all_alpha=True), **kw)
        model.__dict__.pop("use_hip_graph", None)
        assert len(got) == 3 and torch.equal(got[0], want[0])
        assert len(sep) == 6 and tuple(sep[5].shape) == (T * B, 100, 4)
        for a, b in zip(sep, want_sep):
            assert torch.equal(a, b)
        # drawn noise: still the eager loop, nothing captured -- without indices too (the pair (None, None) is not "no guidance"
        # to the DDPM chain's choice of loop)
        torch.manual_seed(5)
        a = model.sample_with_guide(*common(), guidance_indice=idx, guidance_values=gv, **kw)[0]
        b = model.sample_separate(*common(), **kw)
        assert not model.__dict__.get("_step_graphs")
        torch.manual_seed(6)
        c = model.sample_with_guide(*common(), **kw)[0]
        assert not model.__dict__.get("_step_graphs")
        model.use_hip_graph = False
        torch.manual_seed(6)
        d = model.sample(*common(), **kw)[0]                                  # the eager chain's own draws
        model.__dict__.pop("use_hip_graph", None)
        assert torch.equal(c, d)
        with pytest.raises(ValueError):                                        # per-clip keyframes: few-step solvers only
            model.sample_with_guide(*common(), guidance_indice=smp.DenseGuide.stack([([1], gv[:1]), None], 100, 67), **kw)
        assert torch.isfinite(a).all() and all(torch.isfinite(v).all() for v in b)
    finally:
        model.diffusion_sched = old
        model.__dict__.pop("use_hip_graph", None)
        model.__dict__.pop("_step_graphs", None)
