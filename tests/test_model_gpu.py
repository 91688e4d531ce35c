"""GPU parity of the model-level call surface (MSMD / DenoisingNetwork_MSMD / StyleEncoder_VAE2 / infer_coeffs)
against the goldens produced by the imported reference (tests/golden/make_goldens.py).

fp32 parity mode: max-abs-err < 1e-4 on the motion coefficients (BASELINE.json north_star).
bf16 speed mode: reported with its own tolerance (stated in test_bf16_mode_tolerance)."""
from unittest import mock

import numpy as np
import pytest
import torch

from msmd_amd import synth
from msmd_amd.config import default_args

from conftest import load_golden
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


@pytest.mark.parametrize("am", ["wav2vec2", "hubert"])
def test_extract_audio_feature_fp32(am):
    g = load_golden(f"g3_audio_{am}")
    model, args = get_model(am, "fp32")
    audio = dev(synth.audio_clips(2, 64000))
    feat = model.extract_audio_feature(audio)
    f768 = model.extract_audio_768_feature(audio)
    torch.cuda.synchronize()
    assert feat.shape == (2, 100, 512) and feat.dtype == torch.float32
    assert maxabs(f768.cpu().numpy()[:, ::2, ::3], g["feat768"]) < 1e-4
    assert maxabs(feat.cpu().numpy(), g["feat"]) < 1e-4
    # wrapper surface (already padded audio, 30 fps crop + interpolation path)
    from msmd_amd.utils.model_common import pad_audio
    a2 = dev(synth.audio_clips(1, 32000, tag="audio30"))
    y = model.audio_encoder(pad_audio(a2), 30, frame_num=60).last_hidden_state
    assert maxabs(y.cpu().numpy(), g["hidden_fps30_60"]) < 1e-4


def test_encoder_stages_fp32():
    g = load_golden("g3_audio_wav2vec2")
    model, _ = get_model("wav2vec2", "fp32")
    enc = model.audio_encoder
    audio = dev(synth.audio_clips(2, 64000))
    x = enc.feature_extractor_cl(audio, torch.float32, 20, 0)
    assert x.shape == (2, 200, 512)
    assert maxabs(x.cpu().numpy()[:, ::3, ::5], g["conv"]) < 5e-5


def test_denoiser_fp32():
    g = load_golden("g3_denoiser")
    for width in (1, 2):
        model, args = get_model("wav2vec2", "fp32", align_mask_width=width)
        x = denoiser_inputs(2, args)
        person = torch.cat([dev(x["shape"])[:, None], dev(x["style"])[:, None]], dim=-1)
        y = model.denoising_net(dev(x["motion"]), dev(x["audio_feat"]), person, dev(x["style"])[:, None],
                                dev(x["prev_motion"]), dev(x["prev_audio"]), dev(g["step"]), dev(x["indicator"]))
        assert y.shape == (2, 110, 67) and y.dtype == torch.float32
        assert maxabs(y.cpu().numpy(), g[f"target_w{width}"]) < 1e-4, width
    model, args = get_model("wav2vec2", "fp32")
    x = denoiser_inputs(2, args)
    person = torch.cat([dev(x["shape"])[:, None], dev(x["style"])[:, None]], dim=-1)
    dyn, stat, al = model.denoising_net(dev(x["motion"]), dev(x["audio_feat"]), person, dev(x["style"])[:, None],
                                        dev(x["prev_motion"]), dev(x["prev_audio"]), dev(g["step"]),
                                        dev(x["indicator"]), keep_separate=True)
    assert maxabs(dyn.cpu().numpy(), g["dynamic"]) < 1e-4 and maxabs(al.cpu().numpy(), g["alphas"]) < 1e-4
    assert maxabs(stat.cpu().numpy()[:, :2], g["static"]) < 1e-4
    with pytest.raises(TypeError):  # reference model.py:944 fails the same way without an indicator
        model.denoising_net(dev(x["motion"]), dev(x["audio_feat"]), person, dev(x["style"])[:, None],
                            dev(x["prev_motion"]), dev(x["prev_audio"]), dev(g["step"]), None)


@pytest.mark.parametrize("name,kw", [("sigmoid", dict(regularize_alpha="sigmoid")), ("sinpe", dict(no_use_learnable_pe=True))])
def test_denoiser_options_fp32(name, kw):
    """regularize_alpha='sigmoid' (msmd_heads_static_mix flag) and the sinusoidal PE module (one table row on every
    position): HIP forward vs goldens from the reference built with each switch (1e-4), the differentiable training
    graph in eval mode vs the same goldens, and the sampler running through the same switches."""
    from msmd_amd import train_graph as tg
    g = load_golden("g3_denoiser_options")
    model, args = get_model("wav2vec2", "fp32", **kw)
    net = model.denoising_net
    assert ("PE" in dict(net.named_parameters())) == (name != "sinpe")
    x = denoiser_inputs(2, args)
    person = torch.cat([dev(x["shape"])[:, None], dev(x["style"])[:, None]], dim=-1)
    a = (dev(x["motion"]), dev(x["audio_feat"]), person, dev(x["style"])[:, None], dev(x["prev_motion"]),
         dev(x["prev_audio"]), dev(g["step"]), dev(x["indicator"]))
    y = net(*a)
    assert maxabs(y.cpu().numpy(), g[f"target_{name}"]) < 1e-4
    _, _, al = net(*a, keep_separate=True)
    assert maxabs(al.cpu().numpy(), g[f"alphas_{name}"]) < 1e-4
    with torch.no_grad():
        yt = tg.denoiser_train(net, a[0], a[1], person, a[3], a[4], a[5], a[6], a[7], torch.float32)
    assert maxabs(yt.cpu().numpy(), g[f"target_{name}"]) < 1e-4
    out, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), indicator=dev(x["indicator"]))
    assert out.shape == (2, 100, 67) and bool(torch.isfinite(out).all())


def test_msmd_forward_fp32():
    g = load_golden("g3_forward")
    model, args = get_model("wav2vec2", "fp32")
    x = denoiser_inputs(2, args, tag="fw")
    audio = dev(synth.audio_clips(2, 64000, tag="fw_audio"))
    eps, target, m_det, afeat = model(dev(x["motion"]), audio, dev(x["shape"]), dev(x["style"]), time_step=[3, 499],
                                      indicator=dev(x["indicator"]), train_with_CFG=False, eps=dev(g["a_eps"]))
    assert target.shape == (2, 110, 67) and afeat.shape == (2, 100, 512)
    assert maxabs(afeat.cpu().numpy()[:, ::2, ::3], g["a_audio_feat"]) < 1e-4
    assert maxabs(target.cpu().numpy(), g["a_target"]) < 1e-4
    # feature input + previous window + CFG masking with the reference's recorded coin flips
    flag = dev(g["b_flag"])
    with mock.patch("torch.rand", return_value=flag):
        _, target, _, _ = model(dev(x["motion"]), dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]),
                                dev(x["prev_motion"]), dev(x["prev_audio"]), time_step=[250, 1],
                                indicator=dev(x["indicator"]), train_with_CFG=True, eps=dev(g["b_eps"]))
    assert maxabs(target.cpu().numpy(), g["b_target"]) < 1e-4
    with pytest.raises(AssertionError):
        model(dev(x["motion"]), audio[:, :100], dev(x["shape"]), dev(x["style"]))
    with pytest.raises(ValueError):
        model(dev(x["motion"]), audio[0, :1], dev(x["shape"]), dev(x["style"]))


def test_style_encoder_fp32():
    from msmd_amd.style_encoder import get_style_encoder
    g = load_golden("g3_style")
    enc = get_style_encoder(default_args(compute_dtype="fp32"), "vae2").to(DEV).eval()
    assert get_style_encoder(default_args(), "other") is None
    for B, T in ((2, 100), (1, 60)):
        m = dev(synth.motion_clips(B, T, tag="style_in"))
        mu, logvar = enc.mu_logvar(m)
        assert maxabs(mu.cpu().numpy(), g[f"mu_{B}_{T}"]) < 5e-5 and maxabs(logvar.cpu().numpy(), g[f"logvar_{B}_{T}"]) < 5e-5
        with mock.patch("torch.randn_like", return_value=dev(g[f"eps_{B}_{T}"])):
            z, mu2, lv2 = enc(m)
        assert maxabs(z.cpu().numpy(), g[f"z_{B}_{T}"]) < 1e-4
        assert enc.sample(m).shape == (B, 256)


def test_sampler_fp32():
    from msmd_amd.model import DiffusionSchedule
    g = load_golden("g3_sample")
    model, args = get_model("wav2vec2", "fp32")
    x = denoiser_inputs(2, args, tag="sm")
    T = 3
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(T, "cosine").to(DEV)
    xT = dev(synth.normalish("sm/xT", (2, 100, 67)))
    cases = {
        "inc": dict(cfg_mode="incremental", cfg_scale=1.15),
        "ind": dict(cfg_mode="independent", cfg_scale=[1.3, 0.9]),
        "audio_only": dict(cfg_cond=["audio"], cfg_scale=2.0),
        "nocfg": dict(cfg_cond=[]),
        "dt": dict(cfg_mode="incremental", cfg_scale=1.4, dynamic_threshold=(0.9, 0.5, 2.0)),
        "flex": dict(cfg_mode="incremental", cfg_scale=1.15, flexibility=0.5),
    }
    try:
        for name, kw in cases.items():
            z = g[f"{name}_z"]
            noise = {T - i: dev(z[i]) for i in range(T - 1)}
            y, xT_out, af = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                         dev(x["prev_audio"]), motion_at_T=xT, indicator=dev(x["indicator"]),
                                         noise=noise, **kw)
            assert maxabs(y.cpu().numpy(), g[f"{name}_x0"]) < 1e-4, (name, maxabs(y.cpu().numpy(), g[f"{name}_x0"]))
        # sample_separate vs the reference's own output
        z = g["sep_z"]
        r = model.sample_separate(dev(x["audio_feat"][:1]), dev(x["shape"][:1]), dev(x["style"][:1]),
                                  dev(x["prev_motion"][:1]), dev(x["prev_audio"][:1]), motion_at_T=xT[:1],
                                  indicator=dev(x["indicator"][:1]), cfg_scale=1.3,
                                  noise={T - i: dev(z[i]) for i in range(T - 1)})
        for got, key in zip((r[0], r[3], r[4], r[5]), ("sep_x0", "sep_dyn", "sep_static", "sep_alpha")):
            assert maxabs(got.cpu().numpy(), g[key]) < 1e-4, key
        # sample_with_guide: the reference's call is broken (model.py:770); parity is pinned on the oracle
        from oracle import diffusion as od
        from helpers import msmd_state_dict
        sd, _ = msmd_state_dict("wav2vec2")
        idx = [0, 5, 99]
        gv = synth.normalish("sm/guide", (3, 67))
        zi = g["inc_z"]
        ref = od.sample(sd, od.diffusion_schedule(T, "cosine"), x["audio_feat"], x["shape"], x["style"],
                        synth.normalish("sm/xT", (2, 100, 67)), {T - i: zi[i] for i in range(T - 1)}, x["prev_motion"],
                        x["prev_audio"], x["indicator"], cfg_scale=1.15, guidance=(idx, gv))
        y, _, _ = model.sample_with_guide(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                          dev(x["prev_audio"]), motion_at_T=xT, indicator=dev(x["indicator"]),
                                          guidance_indice=idx, guidance_values=dev(gv),
                                          noise={T - i: dev(zi[i]) for i in range(T - 1)})
        assert maxabs(y.cpu().numpy(), ref) < 1e-4
        traj, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), motion_at_T=xT,
                                  indicator=dev(x["indicator"]), ret_traj=True)
        assert sorted(traj) == [0, 1, 2, 3]
        with pytest.raises(NotImplementedError):
            model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), motion_at_T=xT,
                         indicator=dev(x["indicator"]), cfg_mode="bogus")
    finally:
        model.diffusion_sched = old


def test_sampler_target_noise_fp32():
    from msmd_amd.model import DiffusionSchedule
    g = load_golden("g3_sample")
    model, args = get_model("wav2vec2", "fp32", target="noise")
    x = denoiser_inputs(2, args, tag="sm")
    T = 3
    model.diffusion_sched = DiffusionSchedule(T, "linear").to(DEV)
    z = g["noise_z"]
    inputs = (dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]))
    kw = dict(motion_at_T=dev(synth.normalish("sm/xT", (2, 100, 67))), cfg_scale=1.15, indicator=dev(x["indicator"]))
    y, _, _ = model.sample(*inputs, noise={T - i: dev(z[i]) for i in range(T - 1)}, **kw)
    assert maxabs(y.cpu().numpy(), g["noise_x0"]) < 2e-4
    # the captured loop takes target 'noise' through msmd_cfg_ddpm_step_dev: the eager loop's bits under the same (zero)
    # noise, on one lane and on two
    from msmd_amd import sampler as smp
    eager, _, _ = model.sample(*inputs, noise={t: torch.zeros(2, 100, 67, device=DEV) for t in range(2, T + 1)}, **kw)
    try:
        for lanes in (1, 2):
            model.__dict__.pop("_step_graphs", None)
            with mock.patch.object(smp, "MIN_LANE_SEQS", 1), mock.patch.object(smp, "LANES", lanes), \
                    mock.patch.object(smp, "_step_noise", side_effect=lambda B, L, dm, d: torch.zeros(B, L, dm, device=d)):
                graph, _, _ = model.sample(*inputs, **kw)
                assert next(iter(model._step_graphs.values())).lanes == lanes
            assert torch.equal(eager, graph), lanes
    finally:
        model.__dict__.pop("_step_graphs", None)


def test_infer_coeffs_fp32():
    from msmd_amd.inference import infer_coeffs, window_plan
    from msmd_amd.model import DiffusionSchedule
    g = load_golden("g3_infer")
    gi = load_golden("g1_index")
    model, args = get_model("wav2vec2", "fp32")
    T = 2
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(T, "cosine").to(DEV)
    try:
        for S in (100000, 32000):
            clip_len, _, n_sub, n_pad, n_pad_frames = window_plan(S, args.fps, args.n_motions, 640.0)
            assert [clip_len, n_sub, n_pad, n_pad_frames] == gi[f"plan_{S}"].tolist()
            audio = dev(synth.audio_clips(1, S, tag="infer")[0])
            style = dev(synth.normalish("infer/style", (1, args.d_style)))
            shape = torch.zeros(1, 1, 100, device=DEV)
            draws = g[f"draws_{S}"]
            noise = dict(xT=dev(draws[0]), z=[{2: dev(draws[1 + i])} for i in range(n_sub)])
            y = infer_coeffs(model, args, audio, shape, 640.0, style, cfg_scale=1.4, dynamic_threshold=None, noise=noise)
            assert y.shape == g[f"coef_{S}"].shape
            assert maxabs(y.cpu().numpy(), g[f"coef_{S}"]) < 1e-4, S
    finally:
        model.diffusion_sched = old


def test_infer_coeffs_edge_lengths():
    """Edge lengths of the window driver, following the reference's integer arithmetic (inference.py:38-45, 71-72):
    an EMPTY clip and a 100-sample clip (0 frames at 25 fps) pad to one window and trim to (n_rep, 0, 67); 641 samples
    yield exactly one frame; exactly one window needs no padding; one sample over is still one window (clip_len stays
    100, the encoder sees 64001 samples); 102 frames' worth starts a second window trimmed to 102 frames."""
    import math
    from msmd_amd.inference import infer_coeffs, infer_coeffs_batch, window_plan
    from msmd_amd.model import DiffusionSchedule
    model, args = get_model("wav2vec2", "fp32")
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(2, "cosine").to(DEV)
    style = dev(synth.normalish("edge/style", (1, args.d_style)))
    shape = torch.zeros(1, 1, 100, device=DEV)
    try:
        outs = {}
        for S in (0, 100, 641, 64000, 64001, 65280):
            clip_len = int(S / 16000 * args.fps)
            n_sub = 1 if clip_len <= args.n_motions else math.ceil(clip_len / args.n_motions)
            n_pad = 64000 * n_sub - S
            n_pad_frames = math.ceil(n_pad / 640.0)
            assert list(window_plan(S, args.fps, args.n_motions, 640.0))[2:] == [n_sub, n_pad, n_pad_frames]
            audio = dev(synth.audio_clips(1, max(S, 1), tag="edge")[0][:S])
            y = infer_coeffs(model, args, audio, shape, 640.0, style.expand(2, -1), n_repetitions=2,
                             dynamic_threshold=None)
            want = n_sub * args.n_motions - (n_pad_frames if n_pad_frames > 0 else 0)
            assert y.shape == (2, want, 67) and bool(torch.isfinite(y).all()), (S, y.shape)
            outs[S] = want
        assert outs == {0: 0, 100: 0, 641: 1, 64000: 100, 64001: 100, 65280: 102}
        # the batched driver takes the same ragged lengths in one call
        auds = [dev(synth.audio_clips(1, S, tag="edge")[0]) for S in (641, 65280, 32000)]
        ys = infer_coeffs_batch(model, args, auds, torch.zeros(3, 100, device=DEV), 640.0, style.expand(3, -1),
                                dynamic_threshold=None)
        assert [tuple(v.shape) for v in ys] == [(1, 1, 67), (1, 102, 67), (1, 50, 67)]
    finally:
        model.diffusion_sched = old


def test_bf16_mode_tolerance():
    """Speed mode (bf16 storage, fp32 accumulate) on the 2-clip reference goldens: max-abs-err <= 0.08 on O(1) outputs after
    12 encoder + 8 decoder layers.  The mode's STATED bound, config.PARITY_BOUNDS["bf16"] = 2^-3, is asserted on the
    B = 32 bench batch (all clips) by test_bench_batch_b32_16_bit_modes_within_their_stated_bound below."""
    g = load_golden("g3_forward")
    ga = load_golden("g3_audio_wav2vec2")
    model, args = get_model("wav2vec2", "bf16")
    x = denoiser_inputs(2, args, tag="fw")
    audio = dev(synth.audio_clips(2, 64000, tag="fw_audio"))
    eps, target, _, afeat = model(dev(x["motion"]), audio, dev(x["shape"]), dev(x["style"]), time_step=[3, 499],
                                  indicator=dev(x["indicator"]), train_with_CFG=False, eps=dev(g["a_eps"]))
    e_t = maxabs(target.cpu().numpy(), g["a_target"])
    e_a = maxabs(afeat.cpu().numpy()[:, ::2, ::3], g["a_audio_feat"])
    print(f"bf16 mode: target err {e_t:.4f}, audio feat err {e_a:.4f}, |target| max {np.abs(g['a_target']).max():.2f}")
    assert e_t <= 0.08 and e_a <= 0.08
    feat = model.extract_audio_feature(dev(synth.audio_clips(2, 64000)))
    assert maxabs(feat.cpu().numpy(), ga["feat"]) <= 0.08


@pytest.mark.parametrize("mode", ["bf16", "fp16", "f16x2"])
def test_a_clips_result_does_not_depend_on_its_batch(mode):
    """extract_audio_feature and a 3-step sample() of clip 0 alone, with four other clips and inside the bench's batch of 32:
    the same bits.  (Round 5: up to 0.04-0.06 in bf16 -- 64 x 64 / 128 x 128 / 256 x 256-tile kernels summed the LayerNorm
    statistics in different associations and the person-token query changed form at 64 sequences.)"""
    from msmd_amd.model import DiffusionSchedule
    model, args = get_model("wav2vec2", mode)
    T = 3
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(T, "cosine").to(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    audio = dev(synth.audio_clips(32, 64000, tag="binv"))
    style = torch.randn(32, 256, device=DEV, generator=g)
    xT = torch.randn(32, 100, 67, device=DEV, generator=g)
    noise = {t: torch.randn(32, 100, 67, device=DEV, generator=g) for t in range(2, T + 1)}
    shape, ind = torch.zeros(32, 100, device=DEV), torch.ones(32, 100, device=DEV)
    outs = []
    try:
        for B in (1, 5, 32):
            f = model.extract_audio_feature(audio[:B])
            x, _, _ = model.sample(f, shape[:B], style[:B], motion_at_T=xT[:B], indicator=ind[:B],
                                   noise={t: z[:B] for t, z in noise.items()})
            outs.append((f[0].clone(), x[0].clone()))
    finally:
        model.diffusion_sched = old
    for f, x in outs[1:]:
        assert torch.equal(f, outs[0][0]) and torch.equal(x, outs[0][1])


@pytest.mark.parametrize("mode", ["fp32", "f16x2", "bf16"])
def test_sampler_last_layer_person_chain_skip_returns_the_same_bits(mode):
    """On the diagonal-mask path the last decoder layer's person-token cross-attention feeds row 0 only, and the network's
    output is rows 1.. (reference model.py:986-996 slices them): trunk() skips that chain.  Same bits with and without."""
    from msmd_amd.model import DiffusionSchedule
    model, args = get_model("wav2vec2", mode)
    x = denoiser_inputs(2, args, tag="sm")
    T = 3
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(T, "cosine").to(DEV)
    xT = dev(synth.normalish("sm/xT", (2, 100, 67)))
    noise = {t: dev(synth.normalish(f"sm/z{t}", (2, 100, 67))) for t in range(2, T + 1)}
    outs = []
    try:
        for skip in (True, False):
            model.denoising_net.skip_dead_person_chain = skip
            o, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                   dev(x["prev_audio"]), motion_at_T=xT, indicator=dev(x["indicator"]), noise=noise)
            outs.append(o)
    finally:
        model.diffusion_sched = old
        model.denoising_net.__dict__.pop("skip_dead_person_chain", None)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_sampler_hip_graph_matches_eager():
    """The captured-step (hipGraph, device-side step counter) loop must equal the eager loop bit for bit when
    both draw the same noise (zeros here: sampler._step_noise is patched before capture).  With real noise, a seeded run gives
    the same bits on one lane and on two (the step's noise is drawn once for the whole batch and sliced per lane)."""
    from msmd_amd.model import DiffusionSchedule
    from msmd_amd import sampler as smp
    model, args = get_model("wav2vec2", "fp32")
    x = denoiser_inputs(2, args, tag="sm")
    T = 6
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(T, "cosine").to(DEV)
    xT = dev(synth.normalish("sm/xT", (2, 100, 67)))
    try:
        zeros = {t: torch.zeros(2, 100, 67, device=DEV) for t in range(2, T + 1)}
        for kw in (dict(cfg_scale=1.15), dict(cfg_scale=1.4, dynamic_threshold=(0.9, 0.5, 2.0)),
                   dict(cfg_mode="independent", cfg_scale=[1.3, 0.9], flexibility=0.3)):
            eager, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                       dev(x["prev_audio"]), motion_at_T=xT, indicator=dev(x["indicator"]), noise=zeros,
                                       **kw)
            model.__dict__.pop("_step_graphs", None)
            with mock.patch.object(smp, "_step_noise", side_effect=lambda B, L, dm, d: torch.zeros(B, L, dm, device=d)):
                graph, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]),
                                           dev(x["prev_motion"]), dev(x["prev_audio"]), motion_at_T=xT,
                                           indicator=dev(x["indicator"]), **kw)
            assert torch.equal(eager, graph), kw
            # two LANES (each clip's chain of steps on a HIP stream of its own, forked / joined inside the captured graph;
            # the default from 48 sequences per lane up): the same bits again
            model.__dict__.pop("_step_graphs", None)
            with mock.patch.object(smp, "MIN_LANE_SEQS", 1), mock.patch.object(smp, "LANES", 2), \
                    mock.patch.object(smp, "_step_noise", side_effect=lambda B, L, dm, d: torch.zeros(B, L, dm, device=d)):
                laned, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]),
                                           dev(x["prev_motion"]), dev(x["prev_audio"]), motion_at_T=xT,
                                           indicator=dev(x["indicator"]), **kw)
                assert next(iter(model._step_graphs.values())).lanes == 2
            assert torch.equal(eager, laned), kw
            model.__dict__.pop("_step_graphs", None)
            with mock.patch.object(smp, "_step_noise", side_effect=lambda B, L, dm, d: torch.zeros(B, L, dm, device=d)):     # back to the one-lane graph
                model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]), dev(x["prev_audio"]),
                             motion_at_T=xT, indicator=dev(x["indicator"]), **kw)
        # second call re-uses the cached graph with new operands
        with mock.patch.object(smp, "_step_noise", side_effect=lambda B, L, dm, d: torch.zeros(B, L, dm, device=d)):
            again, _, _ = model.sample(dev(x["audio_feat"]) * 0.5, dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                       dev(x["prev_audio"]), motion_at_T=xT, indicator=dev(x["indicator"]), **kw)
        ref, _, _ = model.sample(dev(x["audio_feat"]) * 0.5, dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                 dev(x["prev_audio"]), motion_at_T=xT, indicator=dev(x["indicator"]), noise=zeros, **kw)
        assert torch.equal(again, ref)
        # real noise: finite, and different from the zero-noise trajectory
        rnd, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), motion_at_T=xT,
                                 indicator=dev(x["indicator"]))
        assert torch.isfinite(rnd).all() and not torch.equal(rnd, eager)
        # ... and the same clip gets the same noise under a given seed whatever the lane count
        seeded = []
        for lanes in (1, 2):
            model.__dict__.pop("_step_graphs", None)
            with mock.patch.object(smp, "MIN_LANE_SEQS", 1), mock.patch.object(smp, "LANES", lanes):
                torch.manual_seed(4242)
                out, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), motion_at_T=xT,
                                         indicator=dev(x["indicator"]))
                assert next(iter(model._step_graphs.values())).lanes == lanes
            seeded.append(out)
        assert torch.equal(seeded[0], seeded[1]) and not torch.equal(seeded[0], rnd)
        # the eager loop's own draws (noise=None: one generator call per step t > 1): the same bits under the same seed, and
        # not the zero-noise ones
        model.use_hip_graph = False
        drawn = []
        for _ in range(2):
            torch.manual_seed(4242)
            out, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]),
                                     dev(x["prev_audio"]), motion_at_T=xT, indicator=dev(x["indicator"]), **kw)
            drawn.append(out)
        assert torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[0], eager)
    finally:
        model.diffusion_sched = old
        model.__dict__.pop("use_hip_graph", None)
        model.__dict__.pop("_step_graphs", None)


def test_hubert_large_architecture_fp32_and_bf16():
    """BASELINE.json configs[3]: HuBERT-large ARCHITECTURE (LayerNorm conv stack with biases, stable-layer-norm
    encoder, 1024 wide, 16 heads; 2 layers here) on a 10 s clip: fp32 HIP path against the reference wrapper's golden
    (< 1e-4 on the hidden states) and the bf16 mode's tolerance; then MSMD with audio_model='hubert_large'."""
    from msmd_amd.utils.hubert import HubertModel
    from msmd_amd.utils.model_common import pad_audio
    g = load_golden("g3_audio_hubert_large")
    enc = HubertModel.large(num_hidden_layers=2)
    synth.load_synthetic(enc, prefix="audio_encoder.")
    enc = enc.to(DEV).eval()
    a10 = dev(synth.audio_clips(1, 160000, tag="audio10s"))
    x = enc.feature_extractor_cl(a10, torch.float32, 20, 0)
    assert x.shape == (1, 500, 512)
    assert maxabs(x.cpu().numpy()[:, ::5, ::5], g["conv_10s"]) < 5e-5
    h = enc(pad_audio(a10), 25, frame_num=500).last_hidden_state
    torch.cuda.synchronize()
    assert h.shape == (1, 500, 1024)
    assert maxabs(h.cpu().numpy()[:, ::2, ::3], g["hidden_10s"]) < 1e-4
    a4 = dev(synth.audio_clips(2, 64000))
    assert maxabs(enc(pad_audio(a4), 25, frame_num=200).last_hidden_state.cpu().numpy()[:, ::2, ::3], g["hidden_4s"]) < 1e-4
    a2 = dev(synth.audio_clips(1, 32000, tag="audio30"))
    assert maxabs(enc(pad_audio(a2), 30, frame_num=60).last_hidden_state.cpu().numpy(), g["hidden_fps30_60"]) < 1e-4
    hb = enc(pad_audio(a10), 25, frame_num=500, dtype=torch.bfloat16).last_hidden_state.float()
    err = maxabs(hb.cpu().numpy()[:, ::2, ::3], g["hidden_10s"])
    print(f"hubert-large bf16 max-abs-err on LayerNorm-ed hidden states: {err:.4f}")
    assert err < 0.15
    # model-level swap: 10 s clips, 250 motion frames
    model, args = get_model("hubert_large", "bf16", encoder_layers=2, n_motions=250)
    assert model.audio_feature_map.weight.shape == (512, 1024)
    feat = model.extract_audio_feature(dev(synth.audio_clips(2, 160000, tag="audio10s_b")))
    torch.cuda.synchronize()
    assert feat.shape == (2, 250, 512) and bool(torch.isfinite(feat).all())
    frozen = [n for n, p in model.audio_encoder.named_parameters() if not p.requires_grad]
    assert any(n.startswith("feature_extractor.conv_layers.6.layer_norm") for n in frozen)


def test_infer_coeffs_batch_equals_per_clip_and_reference_goldens():
    """infer_coeffs_batch (window i of all clips in one sample() call, one encoder pass per padded length): every
    clip's result equals the per-clip driver with the same injected noise, and the two golden clips still match the
    reference's infer_coeffs outputs when batched together with a third clip."""
    from msmd_amd.inference import infer_coeffs, infer_coeffs_batch, window_plan
    from msmd_amd.model import DiffusionSchedule
    g = load_golden("g3_infer")
    model, args = get_model("wav2vec2", "fp32")
    T = 2
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(T, "cosine").to(DEV)
    try:
        audios, noises, subs = [], [], []
        for S in (100000, 32000):
            n_sub = window_plan(S, args.fps, args.n_motions, 640.0)[2]
            draws = g[f"draws_{S}"]
            audios.append(dev(synth.audio_clips(1, S, tag="infer")[0]))
            noises.append(dict(xT=dev(draws[0]), z=[{2: dev(draws[1 + i])} for i in range(n_sub)]))
            subs.append(n_sub)
        S3 = 150001                                     # third clip: 3 windows, ragged length
        n3 = window_plan(S3, args.fps, args.n_motions, 640.0)[2]
        audios.append(dev(synth.audio_clips(1, S3, tag="infer3")[0]))
        noises.append(dict(xT=dev(synth.normalish("ib/xT", (1, 100, 67))),
                           z=[{2: dev(synth.normalish(f"ib/z{i}", (1, 100, 67)))} for i in range(n3)]))
        style1 = dev(synth.normalish("infer/style", (1, args.d_style)))
        styles = torch.cat([style1, style1, dev(synth.normalish("ib/style", (1, args.d_style)))], dim=0)
        shapes3 = torch.zeros(3, 100, device=DEV)
        ys = infer_coeffs_batch(model, args, audios, shapes3, 640.0, styles, cfg_scale=1.4, dynamic_threshold=None,
                                noise=noises)
        torch.cuda.synchronize()
        for c, S in enumerate((100000, 32000)):
            assert ys[c].shape == g[f"coef_{S}"].shape
            assert maxabs(ys[c].cpu().numpy(), g[f"coef_{S}"]) < 1e-4, S
        for c in range(3):
            y1 = infer_coeffs(model, args, audios[c], shapes3[c:c + 1].unsqueeze(0), 640.0, styles[c:c + 1], cfg_scale=1.4,
                              dynamic_threshold=None, noise=noises[c])
            assert ys[c].shape == y1.shape
            assert maxabs(ys[c].cpu().numpy(), y1.cpu().numpy()) < 2e-5, c
    finally:
        model.diffusion_sched = old


def test_fp16_mode_tolerance_and_sampler():
    """fp16 storage mode (BASELINE.json configs[4] names fp16): IEEE half operands on v_mfma_f32_16x16x32_f16, fp32
    accumulation / LayerNorm / softmax.  11 significand bits instead of bf16's 8: stated tolerance 0.012 max-abs on
    the same goldens the bf16 test holds to 0.08; the hipGraph sampler runs in the same mode."""
    g = load_golden("g3_forward")
    ga = load_golden("g3_audio_wav2vec2")
    model, args = get_model("wav2vec2", "fp16")
    assert model.compute_dtype == torch.float16
    x = denoiser_inputs(2, args, tag="fw")
    audio = dev(synth.audio_clips(2, 64000, tag="fw_audio"))
    eps, target, _, afeat = model(dev(x["motion"]), audio, dev(x["shape"]), dev(x["style"]), time_step=[3, 499],
                                  indicator=dev(x["indicator"]), train_with_CFG=False, eps=dev(g["a_eps"]))
    e_t = maxabs(target.cpu().numpy(), g["a_target"])
    e_a = maxabs(afeat.cpu().numpy()[:, ::2, ::3], g["a_audio_feat"])
    print(f"fp16 mode: target err {e_t:.5f}, audio feat err {e_a:.5f}, |target| max {np.abs(g['a_target']).max():.2f}")
    assert np.isfinite(e_t) and e_t <= 0.012 and e_a <= 0.012
    feat = model.extract_audio_feature(dev(synth.audio_clips(2, 64000)))
    assert maxabs(feat.cpu().numpy(), ga["feat"]) <= 0.012
    xs = denoiser_inputs(2, args, tag="sm")
    out, _, _ = model.sample(dev(xs["audio_feat"]), dev(xs["shape"]), dev(xs["style"]), indicator=dev(xs["indicator"]))
    torch.cuda.synchronize()
    assert out.shape == (2, 100, 67) and bool(torch.isfinite(out).all())


def test_diagonal_cross_attention_fast_path_equals_general_path():
    """align_mask_width = 1: a motion token's cross-attention softmax has one admissible key, so the branch returns
    V[t - 1] W_o^T + b_o for t >= 1 irrespective of the query (exactly, in any precision); only the person token needs
    scores.  The fast path (and its step-invariant hoisting in the sampler) must reproduce the general masked kernels;
    width 2 keeps the general path."""
    from msmd_amd.model import DiffusionSchedule
    model, args = get_model("wav2vec2", "fp32")
    net = model.denoising_net
    assert net.pack(torch.float32).diag
    x = denoiser_inputs(3, args, tag="dg")
    person = torch.cat([dev(x["shape"])[:, None], dev(x["style"])[:, None]], dim=-1)
    call = lambda: net(dev(x["motion"]), dev(x["audio_feat"]), person, dev(x["style"])[:, None], dev(x["prev_motion"]),
                       dev(x["prev_audio"]), [7, 250, 499], dev(x["indicator"]))
    net.diag_single_pass = True
    net.fused_person_query = False
    fast2 = call()                              # two launches: q-projection GEMM + Tq = 1 attention for the person row
    net.fused_person_query = True
    fast = call()                               # the default for any batch (round 6): msmd_person_query_attention
    del net.fused_person_query
    net.diag_single_pass = False
    net.diag_fast_path = False
    try:
        slow = call()
        assert maxabs(fast2.cpu().numpy(), slow.cpu().numpy()) < 2e-6
        # msmd_person_query_attention: fp32 VALU, its own summation order
        assert maxabs(fast.cpu().numpy(), slow.cpu().numpy()) < 1e-5
        old = model.diffusion_sched
        model.diffusion_sched = DiffusionSchedule(4, "cosine").to(DEV)
        xT = dev(synth.normalish("dg/xT", (3, 100, 67)))
        zs = {t: dev(synth.normalish(f"dg/z{t}", (3, 100, 67))) for t in range(2, 5)}
        kw = dict(motion_at_T=xT, indicator=dev(x["indicator"]), cfg_scale=1.3)
        s_slow, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), noise=zs, **kw)
        net.diag_fast_path = True
        s_fast, _, _ = model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), noise=zs, **kw)
        assert maxabs(s_fast.cpu().numpy(), s_slow.cpu().numpy()) < 1e-5
        model.diffusion_sched = old
    finally:
        net.diag_fast_path = True
    m2, _ = get_model("wav2vec2", "fp32", align_mask_width=2)
    assert not m2.denoising_net.pack(torch.float32).diag


def test_capture_forward_replays_equal_eager_on_new_inputs():
    """MSMD.capture_forward: one hipGraph per static shape; replays on NEW inputs equal the eager forward bit for bit."""
    model, args = get_model("wav2vec2", "bf16")
    x = denoiser_inputs(2, args, tag="cf")
    mk = lambda tag: dev(synth.audio_clips(2, 64000, tag=tag))
    ts = torch.tensor([3, 499], device=DEV)
    eps = dev(synth.normalish("cf/eps", (2, 100, 67)))
    run = model.capture_forward(dev(x["motion"]), mk("cf_a0"), dev(x["shape"]), dev(x["style"]), ts, dev(x["indicator"]), eps)
    for tag, t2 in (("cf_a1", [10, 20]), ("cf_a2", [400, 1])):
        a = mk(tag)
        t2 = torch.tensor(t2, device=DEV)
        got = [o.clone() for o in run(audio=a, time_step=t2)]
        ref = model(dev(x["motion"]), a, dev(x["shape"]), dev(x["style"]), time_step=t2, indicator=dev(x["indicator"]),
                    train_with_CFG=False, eps=eps)
        torch.cuda.synchronize()
        assert all(torch.equal(g, r) for g, r in zip(got, ref))
    # lanes: the two clips as two groups, each on a HIP stream of its own inside the one graph -- every group's result is
    # `forward` of that group bit for bit (capture_forward verifies this itself on perturbed inputs); against the one-lane
    # forward of the whole batch the 16-bit mode may differ in last bits (statistics slabs / tiles follow the row count)
    run2 = model.capture_forward(dev(x["motion"]), mk("cf_a0"), dev(x["shape"]), dev(x["style"]), ts, dev(x["indicator"]), eps, lanes=2)
    assert run2.lanes == 2 and run2.lane_drift is not None
    assert run2.lane_drift == 0.0        # round 6: a clip's result no longer depends on the batch (or lane) it is computed in
    a = mk("cf_a3")
    got = [o.clone() for o in run2(audio=a)]
    torch.cuda.synchronize()
    for i in range(2):
        sl = slice(i, i + 1)
        ref = model(dev(x["motion"])[sl], a[sl], dev(x["shape"])[sl], dev(x["style"])[sl], time_step=ts[sl],
                    indicator=dev(x["indicator"])[sl], train_with_CFG=False, eps=eps[sl])
        assert all(torch.equal(g[sl], r) for g, r in zip(got, ref))
    with pytest.raises(ValueError):
        model.capture_forward(dev(x["motion"]), mk("cf_a0"), dev(x["shape"]), dev(x["style"]), ts, dev(x["indicator"]), eps, lanes=3)


@pytest.mark.parametrize("B,S,frames", [(1, 32000, 50), (3, 48000, 75), (33, 16000, 25), (2, 31999, 50), (2, 64001, 100)])
def test_ragged_batches_and_clip_lengths_against_oracle(B, S, frames):
    """Odd batch sizes (1, 3, 33) and clip lengths -- incl. lengths that are NOT a multiple of the 320-sample audio unit
    (31999: no padding branch; 64001: reflect + replicate branch of pad_audio) -- through extract_audio_feature in fp32
    against the oracle on a 2-layer encoder."""
    from msmd_amd import shapes
    from oracle import audio_encoder as oae
    model, args = get_model("wav2vec2", "fp32", encoder_layers=2, n_layers=2)
    sd = synth.fill_state_dict(shapes.msmd_shapes(args, 2))
    audio = synth.audio_clips(B, S, tag=f"rag{B}_{S}")
    got = model.extract_audio_feature(dev(audio), frames)
    torch.cuda.synchronize()
    ref = oae.extract_audio_feature(sd, audio[:3], fps=args.fps, frame_num=frames)
    assert got.shape == (B, frames, 512)
    assert maxabs(got[:3].cpu().numpy(), ref) < 1e-4
    if B > 3:   # rows are independent: the same clip gives the same features wherever it sits in the batch
        again = model.extract_audio_feature(dev(audio[-2:]), frames)
        assert torch.equal(again, got[-2:])


@pytest.mark.parametrize("dtype", ["bf16", "f16x2"])
def test_two_streams_in_one_process_reproduce_the_serial_result_bit_for_bit(dtype):
    """Two independent encoder + feature-map passes in flight on two HIP streams of one process must each equal their
    one-at-a-time result, bit for bit.  With packed-fp32 VALU math in the kernels 10-40 % of such passes differed
    (round 2: DESIGN.md 5b; round 3 traced it to v_pk_* results of the conv0 + GroupNorm + GELU kernel, wrong in lanes
    48-63); the library is built without packed fp32 and this test keeps it that way: at the old rate the
    chance of 40 clean pass pairs was < 1e-3."""
    from msmd_amd.model import get_diffusion_model
    model = get_diffusion_model(default_args(compute_dtype=dtype), DEV).eval()
    B = 32
    audio = [dev(synth.audio_clips(B, 64000, tag=f"two_streams_{i}")) for i in range(2)]
    refs = []
    for i in range(2):
        model.extract_audio_feature(audio[i])            # packs / allocator warm-up
        torch.cuda.synchronize()
        refs.append(model.extract_audio_feature(audio[i]).clone())
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bad = []
    for rep in range(20):
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
        for k in range(2):
            outs = []
            for i in range(2):
                with torch.cuda.stream(streams[i]):
                    outs.append(model.extract_audio_feature(audio[i]))
        torch.cuda.synchronize()
        bad += [(rep, i, int((outs[i] != refs[i]).sum())) for i in range(2) if not torch.equal(outs[i], refs[i])]
    assert not bad, bad[:6]


@pytest.mark.parametrize("dtype", ["fp32", "f16x2", "bf16"])
def test_hubert_large_full_depth_10s_against_torch_cpu_restatement(dtype):
    """BASELINE configs[3] at FULL size: all 24 layers of the HuBERT-large architecture (1024 wide, 16 heads, LayerNorm
    conv stack), B = 2 x 10 s clips, in both parity-grade modes against oracle/torch_cpu.py (the torch-CPU restatement
    pinned to the reference wrapper's 2-layer golden by tests/test_oracle_vs_golden.py) on one clip: < 1e-4 on the final
    LayerNorm-ed hidden states of all 500 frames; the second clip is checked for batch-independence.  bf16 (the mode the
    bench's hubert_large leg is timed in): the stated bound of config.PARITY_BOUNDS."""
    from msmd_amd.config import PARITY_BOUNDS
    from oracle import torch_cpu as tc
    from oracle import audio_encoder as oae
    model, args = get_model("hubert_large", dtype, n_motions=250)
    enc = model.audio_encoder
    assert enc.config.num_hidden_layers == 24
    audio = synth.audio_clips(2, 160000, tag="hl_full")
    cd = torch.bfloat16 if dtype == "bf16" else torch.float32      # storage dtype of the activations (f16x2: fp32 + split operands)
    h = enc.encode(dev(audio), 25, frame_num=500, dtype=cd, pad=True)
    h1 = enc.encode(dev(audio[1:]), 25, frame_num=500, dtype=cd, pad=True)
    torch.cuda.synchronize()
    assert h.shape == (2, 500, 1024)
    sd = {"audio_encoder." + k: v.detach().float().cpu() for k, v in enc.state_dict().items()}
    torch.set_num_threads(min(32, torch.get_num_threads() or 8))
    ref = tc.audio_encoder(sd, torch.from_numpy(oae.pad_audio(audio[:1])), 25, frame_num=500, n_heads=16,
                           stable_layer_norm=True).numpy()
    err = maxabs(h[:1].float().cpu().numpy(), ref)
    from msmd_amd.config import HUBERT_LARGE_BF16_HIDDEN_BOUND
    bound = HUBERT_LARGE_BF16_HIDDEN_BOUND if dtype == "bf16" else PARITY_BOUNDS[dtype]
    print(f"hubert-large 24 layers, {dtype}: max-abs-err vs torch-CPU {err:.3g} (|h| max {np.abs(ref).max():.3g}; bound {bound:.3g})")
    assert err < bound
    # rows do not depend on their batch: the same bits for clip 1 alone and behind clip 0 (16-bit modes: every kernel sums a
    # row's LayerNorm statistics in one association whatever tile the launch's row count routes it to)
    assert np.array_equal(h[1:].float().cpu().numpy(), h1.float().cpu().numpy())


@pytest.mark.parametrize("dtype", ["f16x2", "fp16"])
def test_sampler_b64_t20_against_torch_cpu_sampler(dtype):
    """BASELINE configs[4]'s batch (B = 64, 3 CFG entries = 192 sequences per step) through sample() in the parity-grade
    f16x2 mode AND in the fp16 storage mode configs[4] names, T = 20 steps, x_T and the noise of every step injected,
    against oracle/torch_cpu.sample (pinned to the numpy sampler / g3_sample) run on rows 0 and 63 of the SAME inputs:
    < config.PARITY_BOUNDS[dtype] on x_0 (1e-4 / 2^-6).  Then the hipGraph loop (device noise) on the same batch: finite,
    and its first-row statistics stay in the range of the injected-noise run."""
    from oracle import diffusion as od, torch_cpu as tc
    from msmd_amd.config import PARITY_BOUNDS
    B, T = 64, 20
    model, args = get_model("wav2vec2", dtype, n_diff_steps=T)
    af = synth.normalish("s64/af", (B, 100, 512))
    style, xT = synth.normalish("s64/style", (B, 256)), synth.normalish("s64/xT", (B, 100, 67))
    shape, ind = np.zeros((B, 100), np.float32), np.ones((B, 100), np.float32)
    zs = {t: synth.normalish(f"s64/z{t}", (B, 100, 67)) for t in range(2, T + 1)}
    x0, _, _ = model.sample(dev(af), dev(shape), dev(style), motion_at_T=dev(xT), indicator=dev(ind), cfg_scale=1.15,
                            noise={t: dev(z) for t, z in zs.items()})
    torch.cuda.synchronize()
    rows = [0, 63]
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    ref = tc.sample(sd, od.diffusion_schedule(T, "cosine"), t(af[rows]), t(shape[rows]), t(style[rows]), t(xT[rows]),
                    {k: t(v[rows]) for k, v in zs.items()}, t(ind[rows]), cfg_scale=1.15).numpy()
    err = maxabs(x0[rows].float().cpu().numpy(), ref)
    print(f"sample() B=64 T=20 {dtype}: max-abs-err vs torch-CPU sampler on rows {rows}: {err:.3g} (|x0| max {np.abs(ref).max():.3g}; bound {PARITY_BOUNDS[dtype]:.3g})")
    assert err < PARITY_BOUNDS[dtype]
    xg, _, _ = model.sample(dev(af), dev(shape), dev(style), motion_at_T=dev(xT), indicator=dev(ind), cfg_scale=1.15)
    torch.cuda.synchronize()
    assert xg.shape == (B, 100, 67) and bool(torch.isfinite(xg).all())
    assert float(xg.abs().max()) < 4 * float(x0.abs().max()) + 1.0


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_bench_batch_b32_16_bit_modes_within_their_stated_bound(dtype):
    """The HEADLINE workload (configs[1]: MSMD.forward, B = 32 x 4 s clips, 12 + 8 layers) in the mode the headline is timed in
    (bf16) and in fp16 storage, ALL 32 clips against the torch-CPU restatement of the reference (oracle/torch_cpu.py, pinned
    to the reference goldens): one stated bound per mode, config.PARITY_BOUNDS (bf16 2^-3, fp16 2^-6 on |x| <= ~5) -- the
    same number bench.py prints as `error_bound` and exits non-zero on.  The f16x2 / fp32 modes' 1e-4 on this batch:
    tests/test_split_gpu.py::test_bench_batch_b32_matches_cpu_restatement_in_parity_modes."""
    import bench
    from oracle import diffusion as od, torch_cpu as tc
    from msmd_amd import shapes
    from msmd_amd.config import PARITY_BOUNDS
    model, args = get_model("wav2vec2", dtype)
    b = bench.synth_batch(32, 0, DEV)
    _, target, _, _ = bench.step(model, b)
    torch.cuda.synchronize()
    sd = tc.to_torch(synth.fill_state_dict(shapes.msmd_shapes(args)))
    cpu = lambda t: t.float().cpu()
    torch.set_num_threads(min(32, torch.get_num_threads() or 8))
    _, ref, _ = tc.msmd_forward(sd, od.diffusion_schedule(500, "cosine"), cpu(b["motion"]), cpu(b["audio"]), cpu(b["shape"]),
                                cpu(b["style"]), list(b["time_step"]), cpu(b["eps"]), cpu(b["indicator"]))
    err = maxabs(target.float().cpu().numpy(), ref.numpy())
    print(f"B=32 bench batch, {dtype}: max-abs-err vs CPU restatement on all 32 clips = {err:.4f} (|x| max {float(ref.abs().max()):.2f}; "
          f"bound {PARITY_BOUNDS[dtype]:.4f})")
    assert err < PARITY_BOUNDS[dtype]
    assert err > 1e-4      # (a 16-bit mode that met 1e-4 would be mislabelled)


@pytest.mark.parametrize("am,kw", [("wav2vec2", {}), ("hubert_large", dict(encoder_layers=4, n_motions=100))])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_layernorm_folded_into_gemms_keeps_the_16_bit_modes_error(am, kw, dtype):
    """ops.FOLD_LN (msmd_gemm_ln: no LayerNorm launches inside the encoder blocks, post-LN and pre-LN forms) against the
    LayerNorm-kernel path of the same mode, both measured against the fp32 path on the same weights and audio: the
    folded path rounds the gamma-folded weights instead of the normalised rows -- its error must stay in the same class
    (<= 1.5 x the unfused error + 0.01 on O(1) features)."""
    from msmd_amd import ops
    audio = dev(synth.audio_clips(3, 64000, tag="fold"))
    ref = get_model(am, "fp32", **kw)[0].extract_audio_feature(audio).float().cpu().numpy()
    model, _ = get_model(am, dtype, **kw)
    assert model.audio_encoder.pack({"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]).fold
    with mock.patch.object(ops, "FOLD_LN", True):
        with mock.patch.object(ops, "layernorm", wraps=ops.layernorm) as ln:
            folded = model.extract_audio_feature(audio).float().cpu().numpy()
            n_fold = ln.call_count
    with mock.patch.object(ops, "FOLD_LN", False):
        with mock.patch.object(ops, "layernorm", wraps=ops.layernorm) as ln:
            plain = model.extract_audio_feature(audio).float().cpu().numpy()
            n_plain = ln.call_count
    layers = model.audio_encoder.config.num_hidden_layers
    assert n_plain - n_fold == 2 * layers - (1 if am == "wav2vec2" else 1), (n_plain, n_fold)
    e_f, e_p = maxabs(folded, ref), maxabs(plain, ref)
    print(f"{am} {dtype}: folded err {e_f:.4f}, LayerNorm-kernel err {e_p:.4f}")
    assert e_f <= 1.5 * e_p + 0.01


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_layernorm_fold_in_the_denoiser_trunk_and_sampler(dtype):
    """The decoder layers' three LayerNorms folded into their GEMMs (general masked path: all but the last norm3; diagonal
    sampler path: norm3 only) against the LayerNorm-kernel path of the same 16-bit mode, both against the fp32 path:
    the error must stay in the same class (<= 1.5 x + 0.01).  The 500-step sampler is compared in fp16 only (bf16's own
    drift over 500 steps is larger than any difference between the two paths)."""
    from msmd_amd import ops
    args = default_args()
    x = denoiser_inputs(4, args, tag="foldd")
    xs = denoiser_inputs(2, args, tag="folds")
    audio = dev(synth.audio_clips(4, 64000, tag="foldd_audio"))
    eps = torch.randn(x["motion"].shape, generator=torch.Generator().manual_seed(3)).to(DEV)

    def fwd(model):
        return model(dev(x["motion"]), audio, dev(x["shape"]), dev(x["style"]), time_step=[3, 499, 100, 250],
                     indicator=dev(x["indicator"]), train_with_CFG=False, eps=eps)[1].float().cpu().numpy()

    def smp(model):
        torch.manual_seed(7)
        return model.sample(dev(xs["audio_feat"]), dev(xs["shape"]), dev(xs["style"]),
                            indicator=dev(xs["indicator"]))[0].float().cpu().numpy()

    m32 = get_model("wav2vec2", "fp32")[0]
    ref, ref_s = fwd(m32), (smp(m32) if dtype == "fp16" else None)
    model, _ = get_model("wav2vec2", dtype)
    res = {}
    for on in (True, False):
        with mock.patch.object(ops, "FOLD_LN", on):
            with mock.patch.object(ops, "layernorm", wraps=ops.layernorm) as ln:
                res[on] = fwd(model)
                res[on, "n"] = ln.call_count
            if dtype == "fp16":
                res[on, "s"] = smp(model)
    e_f, e_p = maxabs(res[True], ref), maxabs(res[False], ref)
    print(f"forward {dtype}: folded err {e_f:.4f} ({res[True, 'n']} LayerNorm launches), LayerNorm kernels err {e_p:.4f} ({res[False, 'n']})")
    assert res[False, "n"] - res[True, "n"] == 23 + 23      # encoder 2 x 12 - 1, denoiser 3 x 8 - 1
    assert e_f <= 1.5 * e_p + 0.01
    if dtype == "fp16":
        s_f, s_p = maxabs(res[True, "s"], ref_s), maxabs(res[False, "s"], ref_s)
        print(f"sampler fp16 (500 steps): folded err {s_f:.4f}, LayerNorm kernels err {s_p:.4f}")
        assert s_f <= 1.5 * s_p + 0.01


@pytest.mark.gpu
def test_style_clip_ingestion_on_device_matches_the_reference_function(tmp_path):
    """SURVEY.md 8(f) n3 with device="cuda": the tensors `query_for_motion_coeff` puts on the GPU equal the outputs of the
    reference's own function (g3_ingest: reference inference.py:109-183, built from its AST at generation time)."""
    from helpers import check_ingestion_against_reference
    check_ingestion_against_reference(tmp_path, "cuda")
