"""Training-step gradient parity: the HIP autograd path (train_graph.py) against the reference's own autograd
(eval-mode, fixed noise) recorded in tests/golden/g6_train.npz -- losses, target, and the gradients of 27
parameters spread over the audio encoder (incl. weight-normed positional conv), audio_feature_map, start tokens,
denoiser and style encoder."""
import numpy as np
import pytest
import torch

from msmd_amd import synth
from msmd_amd.config import default_args

from conftest import load_golden
from helpers import maxabs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def test_training_step_gradients_match_reference_autograd():
    from msmd_amd import train_graph as tg
    from msmd_amd import autograd as ag
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    g = load_golden("g6_train")
    args = default_args(compute_dtype="fp32", encoder_layers=2, n_layers=2)
    model = get_diffusion_model(args, DEV).eval()
    se = get_style_encoder(args, "vae2").to(DEV).eval()
    ag.CACHE.clear()
    B = 2
    audio = dev(synth.audio_clips(B, 64000, tag="g6_audio"))
    motion = dev(synth.motion_clips(B, tag="g6_motion"))
    eps = dev(synth.normalish("g6/eps", (B, 100, 67)))
    zst = dev(synth.normalish("g6/zstyle", (B, 256)))
    shape = torch.zeros(B, 100, device=DEV)
    ind = torch.ones(B, 100, device=DEV)
    ind[1, 70:] = 0
    end_idx = torch.tensor([100, 70], device=DEV)
    with torch.enable_grad():
        mu, logvar = tg.style_encoder_train(se, motion, torch.float32)
        style = mu + zst * torch.exp(0.5 * logvar)
        _, target, _, _ = tg.msmd_forward_train(model, motion, audio, shape, style, None, None, [7, 311], ind, eps)
        losses = tg.loss_no_vert_train(args, True, motion, target, None, end_idx=end_idx)
        kl = tg.kl_train(mu, logvar)
        wts = [args.l_vert, args.l_vel * 4.5, args.l_smooth * 4.0, args.l_head_angle, args.l_head_vel, args.l_head_smooth]
        total = sum(w * l for w, l in zip(wts, losses[:6])) + 1e-3 * kl
        total.backward()
    assert maxabs(target.detach().cpu().numpy(), g["target"]) < 1e-4
    assert maxabs(mu.detach().cpu().numpy(), g["mu"]) < 5e-5
    got = np.array([float(l) for l in losses[:6]] + [float(kl), float(total)])
    assert np.max(np.abs(got - g["losses"]) / np.maximum(1.0, np.abs(g["losses"]))) < 1e-5, (got, g["losses"])
    named = dict(model.named_parameters())
    worst = 0.0
    for key in [k[3:] for k in g.files if k.startswith("gn/")]:
        gr = named[key].grad
        assert gr is not None, key
        ref_n, ref_8 = float(g["gn/" + key]), g["g8/" + key]
        rel_n = abs(float(gr.double().norm()) - ref_n) / (ref_n + 1e-12)
        rel_8 = np.max(np.abs(gr.reshape(-1)[:8].cpu().numpy() - ref_8)) / (np.max(np.abs(ref_8)) + 1e-9 * ref_n + 1e-20)
        worst = max(worst, rel_n, min(rel_8, 1.0) if np.max(np.abs(ref_8)) > 1e-3 * ref_n / np.sqrt(gr.numel()) else 0.0)
        # fp32 forward+backward through 2+2 transformer layers on MFMA vs CPU autograd: 1e-3 relative
        assert rel_n < 1e-3, (key, rel_n)
    snamed = dict(se.named_parameters())
    for key in [k[3:] for k in g.files if k.startswith("sn/")]:
        gr = snamed[key].grad
        ref_n = float(g["sn/" + key])
        assert abs(float(gr.double().norm()) - ref_n) / (ref_n + 1e-12) < 1e-3, key
        ref_8 = g["s8/" + key]
        assert np.max(np.abs(gr.reshape(-1)[:8].cpu().numpy() - ref_8)) <= 1e-3 * max(np.max(np.abs(ref_8)), ref_n / np.sqrt(gr.numel())), key
    # frozen feature extractor receives no gradient (reference model.py:97)
    assert named["audio_encoder.feature_extractor.conv_layers.1.conv.weight"].grad is None
    print(f"worst relative gradient deviation: {worst:.2e}")


def test_training_step_gradients_match_reference_autograd_full_depth():
    """The same fixed-noise training forward + backward at FULL depth (12 encoder + 8 decoder layers, fp32 kernels)
    against the reference's autograd (g6_train_full): for 28 parameters spread over every component -- first and last
    layers of both stacks included -- 64 entries sampled across each gradient tensor agree ELEMENT-WISE within 2e-4 of
    the tensor's scale (max |entry| floor-ed at norm / sqrt(numel)), and the norms within 2e-4 relative."""
    from msmd_amd import train_graph as tg
    from msmd_amd import autograd as ag
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    g = load_golden("g6_train_full")
    args = default_args(compute_dtype="fp32")
    model = get_diffusion_model(args, DEV).eval()
    se = get_style_encoder(args, "vae2").to(DEV).eval()
    ag.CACHE.clear()
    B = 2
    audio = dev(synth.audio_clips(B, 64000, tag="g6_audio"))
    motion = dev(synth.motion_clips(B, tag="g6_motion"))
    eps = dev(synth.normalish("g6/eps", (B, 100, 67)))
    zst = dev(synth.normalish("g6/zstyle", (B, 256)))
    shape = torch.zeros(B, 100, device=DEV)
    ind = torch.ones(B, 100, device=DEV)
    ind[1, 70:] = 0
    end_idx = torch.tensor([100, 70], device=DEV)
    with torch.enable_grad():
        mu, logvar = tg.style_encoder_train(se, motion, torch.float32)
        style = mu + zst * torch.exp(0.5 * logvar)
        _, target, _, _ = tg.msmd_forward_train(model, motion, audio, shape, style, None, None, [7, 311], ind, eps)
        losses = tg.loss_no_vert_train(args, True, motion, target, None, end_idx=end_idx)
        kl = tg.kl_train(mu, logvar)
        wts = [args.l_vert, args.l_vel * 4.5, args.l_smooth * 4.0, args.l_head_angle, args.l_head_vel, args.l_head_smooth]
        total = sum(w * l for w, l in zip(wts, losses[:6])) + 1e-3 * kl
        total.backward()
    assert maxabs(target.detach().cpu().numpy(), g["target"]) < 1e-4
    got = np.array([float(l) for l in losses[:6]] + [float(kl), float(total)])
    assert np.max(np.abs(got - g["losses"]) / np.maximum(1.0, np.abs(g["losses"]))) < 2e-5, (got, g["losses"])

    def check(named, prefix_n, prefix_s):
        worst = 0.0
        keys = [k[len(prefix_n):] for k in g.files if k.startswith(prefix_n)]
        for key in keys:
            gr = named[key].grad
            assert gr is not None, key
            flat = gr.reshape(-1)
            ref_n, ref_s = float(g[prefix_n + key]), g[prefix_s + key]
            pick = flat[::max(1, flat.numel() // 64) | 1][:64].cpu().numpy()   # the generator's odd stride
            scale = max(float(np.max(np.abs(ref_s))), ref_n / np.sqrt(flat.numel()))
            rel_e = float(np.max(np.abs(pick - ref_s))) / (scale + 1e-30)
            rel_n = abs(float(gr.double().norm()) - ref_n) / (ref_n + 1e-30)
            assert rel_e < 2e-4 and rel_n < 2e-4, (key, rel_e, rel_n, float(gr.double().norm()), ref_n)
            worst = max(worst, rel_e, rel_n)
        return worst, len(keys)
    w1, n1 = check(dict(model.named_parameters()), "gn/", "g8/")
    w2, n2 = check(dict(se.named_parameters()), "sn/", "s8/")
    assert n1 >= 27 and n2 >= 5
    print(f"full depth: worst relative deviation {max(w1, w2):.2e} over {n1 + n2} tensors x 64 sampled entries")


def test_bf16_train_mode_hipgraph_loss_decreases():
    """bf16 kernels, model.train() (dropout / LayerDrop / SpecAugment live), whole-iteration hipGraph, all draws on the
    device: 60 iterations on one fixed synthetic batch of 8 at lr 1e-4 (10 warm-up iterations) bring the 10-iteration
    mean loss down by more than 15 % and every loss stays finite."""
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    args = default_args(compute_dtype="bf16", lr=1e-4, warm_iter=10, gradient_accumulation_steps=1)
    torch.manual_seed(0)
    model = get_diffusion_model(args, DEV).train()
    se = get_style_encoder(args, "vae2").to(DEV).train()
    tr = Trainer(args, model, se, use_graph=True)
    batch = synthetic_batch(8, 0, DEV)
    losses = []
    for it in range(1, 61):
        losses.append(tr.step(batch, it=it)["loss"])
    vals = torch.stack(losses).float().cpu().numpy()
    assert np.all(np.isfinite(vals))
    first, last = vals[:10].mean(), vals[-10:].mean()
    print(f"bf16 train-mode hipGraph overfit: mean loss {first:.3f} -> {last:.3f}")
    assert last < 0.85 * first, (first, last)


def test_trainer_step_adam_and_overfit():
    """Trainer.step (2 windows, truncation, cross-style, hand-off, flat-arena gradients, fused Adam): the update
    equals torch.optim.Adam applied to the same gradients, and a fixed batch is over-fitted."""
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch, load_loss_weights
    args = default_args(compute_dtype="fp32", encoder_layers=1, n_layers=1, lr=1e-3, warm_iter=0,
                        gradient_accumulation_steps=1)
    w = load_loss_weights(args)
    assert abs(w["vel"] - 0.5 * 4.5e-8) < 1e-20 and abs(w["smooth"] - 10 * 4e-7) < 1e-18 and w["kl_div"] == 1e-7
    torch.manual_seed(0)
    model = get_diffusion_model(args, DEV).eval()
    se = get_style_encoder(args, "vae2").to(DEV).eval()
    tr = Trainer(args, model, se)
    n_train = sum(p.numel() for p in list(se.parameters()) + list(model.parameters()) if p.requires_grad)
    assert tr.flat_param.numel() == tr.reducer.arena.numel() >= n_train
    B = 2
    batch = synthetic_batch(B, 0, DEV)
    draws = dict(cross=[False, True], end_idx=[torch.tensor([60, 100], device=DEV), None], t=[[5, 400], [250, 20]],
                 eps=[dev(synth.normalish(f"tr/eps{i}", (B, 100, 67))) for i in range(2)],
                 style_eps=[dev(synth.normalish(f"tr/se{i}", (B, 256))) for i in range(2)],
                 cfg_flag=[dev(np.array([0.1, 0.7], np.float32)), dev(np.array([0.95, 0.3], np.float32))])
    p0 = tr.flat_param.clone()
    out = tr.step(batch, it=1, draws=draws)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in out.values())
    # Adam reference on the gradient that was just applied: recompute it with a second backward at the OLD weights
    p1 = tr.flat_param.clone()
    tr.flat_param.copy_(p0)
    tr.exp_avg.zero_(); tr.exp_avg_sq.zero_(); tr.opt_step = 0
    tr._invalidate_caches()
    # capture the gradient by running the step with lr = 0
    tr.lr = 0.0
    tr.step(batch, it=1, draws=draws)
    gflat = tr.exp_avg / (1 - 0.9)  # m_1 = (1 - b1) * g
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=1e-3)
    ref.grad = gflat.clone()
    opt.step()
    # the gradient is recomputed by a second backward (fp32 atomics reorder sums): Adam's first update is
    # lr * g / (|g| + eps), so entries with |g| ~ eps move by a fraction of lr; everything else matches to 1e-6
    diff = (p1 - ref.detach()).abs()
    solid = gflat.abs() > 1e-5            # d(update)/dg = lr * eps / (|g| + eps)^2: negligible there
    assert float(diff[solid].max()) < 5e-6 and float(diff.max()) <= 2.1e-3
    assert float((diff > 2e-6).float().mean()) < 1e-2
    # over-fit a fixed batch with fixed draws
    tr.flat_param.copy_(p0)
    tr.exp_avg.zero_(); tr.exp_avg_sq.zero_(); tr.opt_step = 0
    tr.lr = 1e-3
    tr._invalidate_caches()
    first = None
    for it in range(1, 16):
        o = tr.step(batch, it=it, draws=draws)
        first = float(o["noise"]) if first is None else first
    last = float(o["noise"])
    print(f"noise loss {first:.4f} -> {last:.4f}")
    assert last < 0.7 * first


def test_trainer_hipgraph_step_matches_eager():
    """use_graph=True replays forward+backward as one hipGraph: with injected draws the losses and the applied
    update equal the eager step's; with device-drawn noise (graph-safe Philox) consecutive replays differ and a
    second truncation pattern captures its own variant."""
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    args = default_args(compute_dtype="fp32", encoder_layers=1, n_layers=1, lr=1e-3, warm_iter=0,
                        gradient_accumulation_steps=1)
    B = 2
    batch = synthetic_batch(B, 0, DEV)
    draws = dict(cross=[False, True], end_idx=[torch.tensor([60, 100], device=DEV), None], t=[[5, 400], [250, 20]],
                 eps=[dev(synth.normalish(f"tr/eps{i}", (B, 100, 67))) for i in range(2)],
                 style_eps=[dev(synth.normalish(f"tr/se{i}", (B, 256))) for i in range(2)],
                 cfg_flag=[dev(np.array([0.1, 0.7], np.float32)), dev(np.array([0.95, 0.3], np.float32))])
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        model = get_diffusion_model(args, DEV).eval()
        se = get_style_encoder(args, "vae2").to(DEV).eval()
        tr = Trainer(args, model, se, use_graph=use_graph)
        outs = [tr.step(batch, it=it, draws=draws) for it in (1, 2, 3)]
        torch.cuda.synchronize()
        res.append((outs, tr.flat_param.clone(), tr))
    (oe, pe, _), (og, pg, trg) = res
    for a, b in zip(oe, og):
        for k in a:
            assert abs(float(a[k]) - float(b[k])) <= 1e-4 * max(1.0, abs(float(a[k]))), k
    d = (pe - pg).abs()
    assert float(d.max()) < 3e-3 and float((d > 1e-5).float().mean()) < 1e-2   # 3 Adam steps of lr 1e-3 (see above)
    assert len(trg._graphs) == 1
    # cross-style flag is data, not structure: flipping it reuses the same graph and changes the result
    d2 = dict(draws, cross=[True, False])
    o2 = trg.step(batch, it=4, draws=d2)
    assert len(trg._graphs) == 1
    # device-drawn noise: new variants, finite losses, replays differ from each other
    o3 = trg.step(batch, it=5)
    o4 = trg.step(batch, it=6)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in list(o2.values()) + list(o3.values()) + list(o4.values()))
    assert len(trg._graphs) >= 2


@pytest.mark.parametrize("truncate_first", [False, True])
def test_two_windows_as_one_batch_equals_window_after_window(truncate_first):
    """Trainer(batch_windows=True) runs the style encoder, the audio encoder and the denoiser once on [window 0 | window 1]
    rows; batch_windows=False is the reference's order (training_script.py:99-195).  Eval mode, every draw injected: the same
    per-key losses (1e-5 relative) and the same gradient arena -- fp32 sums of 2 B rows in one weight-gradient product
    instead of two accumulated ones: 2e-4 of the arena's largest entry, per-element mismatches above 1e-5 relative rare --
    with window 0 whole (hand-off = its own last frames) and truncated (hand-off from the complete clip's extra pass)."""
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    args = default_args(compute_dtype="fp32", encoder_layers=2, n_layers=2, lr=1e-3, warm_iter=0, gradient_accumulation_steps=1)
    B = 2
    batch = synthetic_batch(B, 0, DEV)
    draws = dict(cross=[False, True], end_idx=[torch.tensor([60, 100], device=DEV) if truncate_first else None,
                                               torch.tensor([100, 33], device=DEV)], t=[[5, 400], [250, 20]],
                 eps=[dev(synth.normalish(f"bw/eps{i}", (B, 100, 67))) for i in range(2)],
                 style_eps=[dev(synth.normalish(f"bw/se{i}", (B, 256))) for i in range(2)],
                 cfg_flag=[dev(np.array([0.1, 0.7], np.float32)), dev(np.array([0.95, 0.3], np.float32))])
    res = []
    for bw in (False, True):
        torch.manual_seed(0)
        model = get_diffusion_model(args, DEV).eval()
        se = get_style_encoder(args, "vae2").to(DEV).eval()
        tr = Trainer(args, model, se, batch_windows=bw)
        tr.reducer.begin_backward()
        tr.reducer.arena.zero_()
        out = tr._fwd_bwd(batch, draws, [truncate_first, True], draws["cross"])
        torch.cuda.synchronize()
        res.append((out, tr.reducer.arena.clone()))
    (o0, g0), (o1, g1) = res
    for k in o0:
        assert abs(float(o0[k]) - float(o1[k])) <= 1e-5 * max(1.0, abs(float(o0[k]))), (k, float(o0[k]), float(o1[k]))
    scale = float(g0.abs().max())
    assert scale > 0 and float((g0 - g1).abs().max()) <= 2e-4 * scale, (float((g0 - g1).abs().max()), scale)
    assert float(((g0 - g1).abs() > 1e-5 * scale).float().mean()) < 1e-3


def test_two_windows_as_one_batch_full_depth_bf16():
    """The same comparison on the full-depth model in the bench's arithmetic (bf16, 12 + 8 layers, B = 4, eval mode, injected
    draws): per-key losses within 2 % and the two gradient arenas at cosine > 0.999 / relative L2 distance < 3 % -- the size of
    bf16 rounding differences between one weight-gradient product over 2 B rows and two accumulated ones (fp32 form of this
    test: 2e-4)."""
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    args = default_args(compute_dtype="bf16", lr=1e-4, warm_iter=0, gradient_accumulation_steps=1)
    B = 4
    batch = synthetic_batch(B, 0, DEV)
    draws = dict(cross=[False, True], end_idx=[None, torch.tensor([100, 33, 80, 100], device=DEV)], t=[[5, 400, 77, 300], [250, 20, 499, 1]],
                 eps=[dev(synth.normalish(f"bw16/eps{i}", (B, 100, 67))) for i in range(2)],
                 style_eps=[dev(synth.normalish(f"bw16/se{i}", (B, 256))) for i in range(2)],
                 cfg_flag=[dev(np.array([0.1, 0.7, 0.95, 0.2], np.float32)), dev(np.array([0.95, 0.3, 0.6, 0.1], np.float32))])
    res = []
    for bw in (False, True):
        torch.manual_seed(0)
        model = get_diffusion_model(args, DEV).eval()
        se = get_style_encoder(args, "vae2").to(DEV).eval()
        tr = Trainer(args, model, se, batch_windows=bw)
        tr.reducer.begin_backward()
        tr.reducer.arena.zero_()
        out = tr._fwd_bwd(batch, draws, [False, True], draws["cross"])
        torch.cuda.synchronize()
        res.append((out, tr.reducer.arena.double().clone()))
        del tr, model, se
    (o0, g0), (o1, g1) = res
    for k in o0:
        assert abs(float(o0[k]) - float(o1[k])) <= 2e-2 * max(1e-3, abs(float(o0[k]))), (k, float(o0[k]), float(o1[k]))
    cos = float((g0 * g1).sum() / (g0.norm() * g1.norm()))
    rel = float((g0 - g1).norm() / g0.norm())
    assert cos > 0.999 and rel < 3e-2, (cos, rel)


def test_bf16_training_gradients_against_the_fp32_path_full_depth():
    """The error of the bf16 training arithmetic, quantified: the gradient arena of one full-depth iteration (12 + 8 layers,
    B = 4, eval mode, every draw injected) in bf16 against the same iteration in the fp32 mode (whose gradients are pinned to the
    reference's autograd by the golden tests above).  Asserted: every loss term within 2 % (absolute floor 1e-3), cosine of the
    two arenas > 0.999, relative L2 distance < 4 %, and per component (audio encoder / denoiser / style encoder / rest)
    cosine > 0.999.  Measured (printed with `-s`): cosine 0.99987, relative L2 1.6 %; audio encoder 2.0 %, denoiser 1.0 %,
    style encoder 0.7 %."""
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    B = 4
    batch = synthetic_batch(B, 0, DEV)
    draws = dict(cross=[False, True], end_idx=[None, torch.tensor([100, 33, 80, 100], device=DEV)], t=[[5, 400, 77, 300], [250, 20, 499, 1]],
                 eps=[dev(synth.normalish(f"bg/eps{i}", (B, 100, 67))) for i in range(2)],
                 style_eps=[dev(synth.normalish(f"bg/se{i}", (B, 256))) for i in range(2)],
                 cfg_flag=[dev(np.array([0.1, 0.7, 0.95, 0.2], np.float32)), dev(np.array([0.95, 0.3, 0.6, 0.1], np.float32))])
    res = []
    for mode in ("fp32", "bf16"):
        args = default_args(compute_dtype=mode, lr=1e-4, warm_iter=0, gradient_accumulation_steps=1)
        torch.manual_seed(0)
        model = get_diffusion_model(args, DEV).eval()
        se = get_style_encoder(args, "vae2").to(DEV).eval()
        tr = Trainer(args, model, se)
        tr.reducer.begin_backward()
        tr.reducer.arena.zero_()
        out = tr._fwd_bwd(batch, draws, [False, True], draws["cross"])
        torch.cuda.synchronize()
        groups = {}
        for name, p_ in list(model.named_parameters()) + [("style_enc." + k, v) for k, v in se.named_parameters()]:
            if p_.grad is None:
                continue
            key = "audio_encoder" if name.startswith("audio_encoder.") else "denoiser" if name.startswith("denoising_net.") \
                else "style_encoder" if name.startswith("style_enc.") else "rest"
            groups.setdefault(key, []).append(p_.grad.detach().double().reshape(-1).clone())
        res.append((out, tr.reducer.arena.double().clone(), {k: torch.cat(v) for k, v in groups.items()}))
        del tr, model, se
    (o0, g0, c0), (o1, g1, c1) = res
    for k in o0:
        assert abs(float(o0[k]) - float(o1[k])) <= 2e-2 * max(5e-2, abs(float(o0[k]))), (k, float(o0[k]), float(o1[k]))
    cos = float((g0 * g1).sum() / (g0.norm() * g1.norm()))
    rel = float((g0 - g1).norm() / g0.norm())
    per = {k: (float((c0[k] * c1[k]).sum() / (c0[k].norm() * c1[k].norm())), float((c0[k] - c1[k]).norm() / c0[k].norm())) for k in c0}
    print(f"bf16 vs fp32 gradient arena: cosine {cos:.5f}, relative L2 {rel:.4f}; per component (cosine, relative L2): "
          + ", ".join(f"{k} {v[0]:.5f} / {v[1]:.4f}" for k, v in per.items()))
    assert cos > 0.999 and rel < 0.04, (cos, rel)
    assert all(v[0] > 0.999 for v in per.values()), per


def test_trainer_segmented_hipgraph_matches_single_graph(monkeypatch):
    """hipGraph mode for more than one rank (forced here on one): the iteration is captured as SEGMENTS that end where a
    gradient bucket receives its last write of the backward (autograd accumulations AND the wgrad GEMM's direct arena
    writes, two windows per weight), so each bucket's all-reduce can start under the rest of the backward.  Same
    injected draws: losses and the applied Adam update equal the one-graph mode bit for bit; every bucket is handed to
    the reducer exactly once per step, in a segment that precedes the last one for most of the bytes."""
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    args = default_args(compute_dtype="bf16", encoder_layers=2, n_layers=2, lr=1e-3, warm_iter=0,
                        gradient_accumulation_steps=1)
    B = 2
    batch = synthetic_batch(B, 0, DEV)
    draws = dict(cross=[False, True], end_idx=[torch.tensor([60, 100], device=DEV), None], t=[[5, 400], [250, 20]],
                 eps=[dev(synth.normalish(f"tr/eps{i}", (B, 100, 67))) for i in range(2)],
                 style_eps=[dev(synth.normalish(f"tr/se{i}", (B, 256))) for i in range(2)],
                 cfg_flag=[dev(np.array([0.1, 0.7], np.float32)), dev(np.array([0.95, 0.3], np.float32))])
    res = []
    for seg in (False, True):
        monkeypatch.setenv("MSMD_SEGMENT_GRAPHS", "1" if seg else "0")
        torch.manual_seed(0)
        model = get_diffusion_model(args, DEV).eval()
        se = get_style_encoder(args, "vae2").to(DEV).eval()
        tr = Trainer(args, model, se, use_graph=True, bucket_mb=4.0)
        assert tr.segment_graphs == seg
        launched = []
        orig = tr.reducer._launch
        tr.reducer._launch = lambda b, _o=orig, _l=launched: (_l.append(b), _o(b))[1]
        outs = [tr.step(batch, it=it, draws=draws) for it in (1, 2)]
        torch.cuda.synchronize()
        res.append((outs, tr.flat_param.clone(), tr, list(launched)))
    (o1, p1, tr1, _), (o2, p2, tr2, l2) = res
    for a, b in zip(o1, o2):
        for k in a:     # float atomics (column sums of the weight-norm fold, bias gradients) order differently: last bits
            assert abs(float(a[k]) - float(b[k])) <= 2e-4 * max(1.0, abs(float(a[k]))), k
    d = (p1 - p2).abs()          # split-contraction wgrad kernels reduce through workspaces: last-bit differences only
    assert float(d.max()) < 2e-5 and float((d > 1e-6).float().mean()) < 1e-3, (float(d.max()), float((d > 1e-6).float().mean()))
    (segs,) = [ent[3] for ent in tr2._graphs.values()]
    nb = len(tr2.reducer.buckets)
    assert len(segs) >= 3 and nb >= 4
    # segment accounting: one segment per distinct "bucket became final" write position; a stretch in which nothing was
    # recorded (after the LAST gradient write there is nothing left to capture) holds no graph and is not replayed -- the
    # host library's "The CUDA Graph is empty" warning of earlier rounds was exactly that stretch
    (n_graphs, n_empty), = tr2.graph_segments.values()
    assert n_graphs == sum(1 for g_, _ in segs if g_ is not None) and n_graphs >= 3
    assert n_empty == sum(1 for g_, _ in segs if g_ is None) < n_graphs      # consecutive final writes with no launch between them
    assert all(bks for g_, bks in segs if g_ is None)                 # a graph-less segment exists only to carry buckets
    assert sum(len(bks) for _, bks in segs) == nb                      # every bucket belongs to exactly one segment
    (n1, e1), = tr1.graph_segments.values()
    assert (n1, e1) == (1, 0)                                          # one-graph mode: one non-empty graph
    per_step = l2[: len(l2) // 2]
    assert sorted(set(per_step)) == list(range(nb))            # every bucket handed over (finish() re-visits are no-ops)
    early = [b for _, bks in segs[:-1] for b in bks]
    early_bytes = sum(tr2.reducer.buckets[b][1] - tr2.reducer.buckets[b][0] for b in early)
    assert early_bytes >= 0.5 * tr2.reducer.arena.numel(), (early_bytes, tr2.reducer.arena.numel())


def test_trainer_vertex_space_branch_steps_through_flame():
    """use_vertex_space on a legacy FLAME dataset type (reference training_script.py:167-176): Trainer.step runs the
    vertex / velocity / smoothness terms through the differentiable FLAME pass; the vertex terms are live (their
    weights change the gradient), the loss is finite and a few Adam steps on a fixed batch reduce it."""
    from types import SimpleNamespace
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    from msmd_amd.utils.flame import FLAME, FLAMEConfig
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = synth.flame_asset()
    fl = FLAME(cfg).to(DEV)
    stats = {"exp_mean": np.zeros(50, np.float32), "exp_std": np.full(50, 0.3, np.float32),
             "pose_mean": np.zeros(6, np.float32), "pose_std": np.full(6, 0.1, np.float32),
             "shape_mean": np.zeros(100, np.float32), "shape_std": np.ones(100, np.float32)}
    args = default_args(compute_dtype="bf16", encoder_layers=1, n_layers=1, lr=2e-4, warm_iter=0,
                        gradient_accumulation_steps=1, use_vertex_space=True, dataset_type="flame_mead_ravdess",
                        l_vert=2e5, l_vel=1e6, l_smooth=1e5)
    B = 2
    batch = synthetic_batch(B, 0, DEV)
    draws = dict(cross=[False, False], end_idx=[torch.tensor([60, 100], device=DEV), None], t=[[5, 400], [250, 20]],
                 eps=[dev(synth.normalish(f"tr/eps{i}", (B, 100, 67))) for i in range(2)],
                 style_eps=[dev(synth.normalish(f"tr/se{i}", (B, 256))) for i in range(2)],
                 cfg_flag=[None, None])
    torch.manual_seed(0)
    model = get_diffusion_model(args, DEV).eval()
    se = get_style_encoder(args, "vae2").to(DEV).eval()
    with pytest.raises(ValueError):
        Trainer(args, model, se)
    tr = Trainer(args, model, se, flame=fl, coef_stats=stats)
    assert tr.vertex_space
    outs = [tr.step(batch, it=i, draws=draws) for i in range(1, 9)]
    torch.cuda.synchronize()
    vert = [float(o["vert"]) for o in outs]
    tot = [float(o["loss"]) for o in outs]
    assert all(np.isfinite(v) for v in vert + tot) and vert[0] > 0
    assert tot[-1] < tot[0], tot
    # the same branch under hipGraph capture (the FLAME kinematics used to read its parent table back from the device
    # inside the capture): first step of a fresh trainer, captured, against the eager trainer's first step
    torch.manual_seed(0)
    model2 = get_diffusion_model(args, DEV).eval()
    se2 = get_style_encoder(args, "vae2").to(DEV).eval()
    trg = Trainer(args, model2, se2, flame=fl, coef_stats=stats, use_graph=True)
    og = [trg.step(batch, it=i, draws=draws) for i in range(1, 4)]
    torch.cuda.synchronize()
    assert all(np.isfinite(float(o["loss"])) for o in og)
    assert abs(float(og[0]["vert"]) - vert[0]) <= 2e-3 * abs(vert[0]), (float(og[0]["vert"]), vert[0])


def test_trainer_train_mode_noise_eager_and_graph():
    """model.train(): dropout / LayerDrop / SpecAugment are live (losses differ from eval mode and from step to
    step on a fixed batch with fixed draws), in eager mode and under hipGraph replay; eval mode is unaffected."""
    from msmd_amd import autograd as ag
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    args = default_args(compute_dtype="bf16", encoder_layers=2, n_layers=2, lr=0.0, warm_iter=0,
                        gradient_accumulation_steps=1)
    B = 2
    batch = synthetic_batch(B, 0, DEV)
    draws = dict(cross=[False, True], end_idx=[torch.tensor([60, 100], device=DEV), None], t=[[5, 400], [250, 20]],
                 eps=[dev(synth.normalish(f"tr/eps{i}", (B, 100, 67))) for i in range(2)],
                 style_eps=[dev(synth.normalish(f"tr/se{i}", (B, 256))) for i in range(2)],
                 cfg_flag=[dev(np.array([0.1, 0.7], np.float32)), dev(np.array([0.95, 0.3], np.float32))])
    try:
        vals = {}
        for mode, use_graph in (("eval", False), ("train", False), ("train", True)):
            torch.manual_seed(0)
            model = get_diffusion_model(args, DEV)
            se = get_style_encoder(args, "vae2").to(DEV)
            (model.train() if mode == "train" else model.eval())
            tr = Trainer(args, model, se, use_graph=use_graph)
            outs = [float(tr.step(batch, it=i, draws=draws)["noise"]) for i in (1, 2, 3)]
            torch.cuda.synchronize()
            assert all(np.isfinite(outs)), (mode, use_graph, outs)
            vals[(mode, use_graph)] = outs
            # gradients reached the SpecAugment embedding only in train mode (lr = 0: weights never move)
        e, t_eager, t_graph = vals[("eval", False)], vals[("train", False)], vals[("train", True)]
        assert max(abs(a - e[0]) for a in e) < 2e-2 * abs(e[0])               # eval: same loss every step (lr = 0)
        for t in (t_eager, t_graph):
            assert len({round(x, 5) for x in t}) == 3                           # fresh masks every step
            assert all(abs(x - e[0]) > 1e-4 for x in t)                          # and not the eval value
            assert all(abs(x - e[0]) < 0.5 * abs(e[0]) for x in t)               # yet the same ballpark
    finally:
        ag.TrainNoise.active = False
        ag.TrainNoise.graph_safe = False
        ag.TrainNoise.spec_masks = None


def test_hubert_large_training_graph_matches_inference_path():
    """The differentiable stable-layer-norm encoder (train_graph) reproduces the no-grad inference kernels on the
    HuBERT-large architecture, and its backward reaches the trainable layers only (layers 0-1 / conv stack /
    projection frozen as for hubert-base, model.py:103-110)."""
    from msmd_amd import train_graph as tg
    from msmd_amd.model import get_diffusion_model
    args = default_args(audio_model="hubert_large", compute_dtype="fp32", encoder_layers=3, n_motions=50)
    model = get_diffusion_model(args, DEV).eval()
    audio = dev(synth.audio_clips(2, 32000, tag="hl_train"))
    ref = model.extract_audio_feature(audio)
    with torch.enable_grad():
        got = tg.audio_feat_train(model, audio, 50, torch.float32).float()
        got.square().mean().backward()
    torch.cuda.synchronize()
    assert maxabs(got.detach().cpu().numpy(), ref.cpu().numpy()) < 1e-4
    enc = model.audio_encoder
    assert enc.get_parameter("encoder.layers.2.attention.q_proj.weight").grad is not None
    assert enc.get_parameter("encoder.layer_norm.weight").grad is not None
    assert enc.get_parameter("encoder.layers.0.attention.q_proj.weight").grad is None
    assert enc.get_parameter("feature_extractor.conv_layers.3.layer_norm.weight").grad is None


def test_trainer_checkpoint_roundtrip_and_reference_schedule(tmp_path):
    """save_checkpoint writes the reference's dict (+ optimizer / scheduler / rng extensions); a fresh Trainer that
    loads it continues bit-identically (same losses and weights as the uninterrupted run); the learning rate follows
    the reference's GradualWarmupScheduler -> CosineAnnealingLR chain."""
    import math
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    args = default_args(compute_dtype="fp32", encoder_layers=1, n_layers=1, lr=1e-3, warm_iter=4, scheduler="WarmupThenDecay",
                        cos_max_iter=12, min_lr_ratio=0.1, gradient_accumulation_steps=1)
    B = 2
    batch = synthetic_batch(B, 0, DEV)

    def make():
        torch.manual_seed(0)
        model = get_diffusion_model(args, DEV).eval()
        se = get_style_encoder(args, "vae2").to(DEV).eval()
        return Trainer(args, model, se)

    def draws(i):
        return dict(cross=[False, i % 2 == 1], end_idx=[None, None], t=[[5 + i, 400], [250, 20 + i]],
                    eps=[dev(synth.normalish(f"ck/eps{i}{j}", (B, 100, 67))) for j in range(2)],
                    style_eps=[dev(synth.normalish(f"ck/se{i}{j}", (B, 256))) for j in range(2)],
                    cfg_flag=[dev(np.array([0.1, 0.7], np.float32)), dev(np.array([0.95, 0.3], np.float32))])
    a = make()
    lrs = []
    for it in range(6):
        lrs.append(a.current_lr())
        a.step(batch, it=it, draws=draws(it))
    # reference schedule (pinned against the reference's own scheduler classes in tests/test_host_cpu.py): warm-up
    # 0, 1/4, 2/4, 3/4, 1 x lr, one hand-over iteration at lr, then the cosine towards 0.1 lr
    assert np.allclose(lrs, [0.0, 2.5e-4, 5e-4, 7.5e-4, 1e-3, 1e-3])
    path = tmp_path / "iter_0000005.pt"
    a.save_checkpoint(path, 5)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert {"args", "model", "style_enc", "iter"} <= set(ck) and ck["iter"] == 5
    out_a = [a.step(batch, it=it, draws=draws(it)) for it in range(6, 9)]
    b = make()
    assert b.load_checkpoint(path) == 5
    out_b = [b.step(batch, it=it, draws=draws(it)) for it in range(6, 9)]
    torch.cuda.synchronize()
    for x, y in zip(out_a, out_b):
        assert abs(float(x["loss"]) - float(y["loss"])) <= 1e-5 * abs(float(x["loss"]))
    d = (a.flat_param - b.flat_param).abs()
    assert float(d.max()) < 1e-4 and float((d > 2e-6).float().mean()) < 1e-2
    assert abs(a.current_lr() - b.current_lr()) < 1e-12


@pytest.mark.parametrize("exchange", ["standin", "rccl"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_backward_with_the_side_stream_busy_equals_backward_alone(use_graph, exchange, monkeypatch):
    """exchange = "rccl": the REAL collective on the side stream -- a one-rank RCCL communicator through the C ABI
    (dp.RcclComm: msmd_comm_init / msmd_allreduce_bucket; GradBucketReducer(exchange_at_world_1=True)): librccl is loaded,
    every bucket's ncclAllReduce is enqueued behind the compute stream's event under the rest of backward, and the sum over
    one rank must leave the gradients as they are.  exchange = "standin":
    One-GPU rehearsal of the data-parallel step's two-queue regime (round-2 VERDICT item 1): with
    world_size 1 `GradBucketReducer.standin` runs value-preserving work on every gradient bucket ON THE SIDE STREAM exactly
    where the RCCL all-reduce would run -- behind the same event, under the rest of backward (segmented hipGraph replays /
    autograd hooks in eager mode).  Each iteration runs forward + backward twice from the same parameters, inputs and
    injected draws, side stream idle vs busy, and compares the gradient arenas: float atomics (bias-gradient column sums)
    allow last-bit noise (measured floor 8e-8 of a bucket's max, tools/dp_sidestream_check.py), a stale or corrupted
    tile would be 1e-2 .. 1.  Parameters are stepped with the busy run's gradients, so the comparison walks along a
    training trajectory."""
    from msmd_amd import autograd as ag
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    monkeypatch.setenv("MSMD_SEGMENT_GRAPHS", "1")
    args = default_args(compute_dtype="bf16", encoder_layers=3, n_layers=2, lr=2e-5, warm_iter=0,
                        gradient_accumulation_steps=1)
    from msmd_amd import dp
    rccl = exchange == "rccl"
    B, steps = 8, ((200 if use_graph else 24) if not rccl else (60 if use_graph else 12))
    torch.manual_seed(0)
    model = get_diffusion_model(args, DEV).eval()
    se = get_style_encoder(args, "vae2").to(DEV).eval()
    comm = dp.RcclComm(DEV) if rccl else None
    tr = Trainer(args, model, se, use_graph=use_graph, bucket_mb=4.0, comm=comm, exchange_at_world_1=rccl)
    red = tr.reducer
    assert tr.segment_graphs == use_graph and len(red.buckets) >= 8
    launched = []

    def busy(view):
        launched.append(view.numel())
        for _ in range(6):
            view.mul_(1.0)

    if rccl:
        assert comm.world == 1 and "librccl" in open("/proc/self/maps").read()      # the library is mapped into THIS process
        real = comm.all_reduce

        def counted(t, stream=None):
            assert stream is red.side                       # enqueued on the reducer's side stream, not the compute stream
            launched.append(t.numel())
            return real(t, stream)
        comm.all_reduce = counted

    def fwd_bwd(batch, draws):
        ag.DIRECT_GRAD = tr.direct_grad
        cross, trunc = tr._host_choices(draws)
        ag.TrainNoise.graph_safe = tr.use_graph
        ag.TrainNoise.spec_masks = None
        red.begin_backward()
        tr._stepping = True
        red.enabled = not tr.use_graph
        out = tr._graph_fwd_bwd(batch, draws, trunc, cross) if tr.use_graph else tr._fwd_bwd(batch, draws, trunc, cross)
        red.finish()
        torch.cuda.synchronize()
        return out

    worst = 0.0
    for it in range(1, steps + 1):
        g = np.random.RandomState(100 + it)
        batch = synthetic_batch(B, 0, DEV, it=it % 3)
        draws = dict(cross=[bool(g.rand() < 0.5), False], end_idx=[dev(g.randint(1, 100, size=B)) if it % 2 else None, None],
                     t=[g.randint(1, 501, size=B).tolist() for _ in range(2)],
                     eps=[dev(g.standard_normal((B, 100, 67)).astype(np.float32)) for _ in range(2)],
                     style_eps=[dev(g.standard_normal((B, 256)).astype(np.float32)) for _ in range(2)],
                     cfg_flag=[dev(g.rand(B).astype(np.float32)) for _ in range(2)])
        tr.noise_state[1] += 1
        red.standin, red.mute = None, rccl                   # side stream idle: no stand-in / the exchange muted
        o1 = fwd_bwd(batch, draws)
        g1 = red.arena.clone()
        red.arena.zero_()
        red.standin, red.mute = (None if rccl else busy), False
        n0 = len(launched)
        o2 = fwd_bwd(batch, draws)
        assert len(launched) - n0 == len(red.buckets)            # every bucket went through the side stream once
        l1, l2 = float(o1["loss"]), float(o2["loss"])
        assert np.isfinite(l1) and abs(l1 - l2) <= 1e-6 * max(1.0, abs(l1)), (it, l1, l2)
        for (s, e, _m) in red.buckets:
            rel = float((g1[s:e] - red.arena[s:e]).abs().max() / g1[s:e].abs().max().clamp_min(1e-30))
            worst = max(worst, rel)
            assert rel < 1e-5, (it, s, e, rel)
        red.standin = None
        tr._optimizer_step()
    assert worst < 1e-5
    if rccl:
        comm.all_reduce = real
        del tr
        comm.destroy()


def test_rccl_bucket_all_reduce_through_the_c_abi_fp32_and_bf16_staging():
    """msmd_allreduce_bucket on a one-rank communicator: (1) fp32 buckets in place on a side stream are the identity and ordered
    behind the stream's earlier work; (2) the 16-bit staging option of the reducer (bucket_dtype=torch.bfloat16: half the
    bytes over xGMI) costs ONE bf16 rounding of each rank's contribution -- relative L2 error of a gradient-like arena
    <= 2^-8, cosine >= 0.99999 (the figure DESIGN.md 6 quotes; the ring's 16-bit partial sums add ~sqrt(hops) of the same
    on a real node)."""
    from msmd_amd import dp
    comm = dp.RcclComm(DEV)
    try:
        g = torch.Generator(device="cpu").manual_seed(7)
        x = (torch.randn(3_000_000, generator=g) * torch.logspace(-6, 0, 3_000_000)).to(DEV)
        ref = x.clone()
        side = torch.cuda.Stream()
        x.mul_(2.0)                                  # compute-stream work the collective must wait for
        ev = torch.cuda.Event(); ev.record()
        side.wait_event(ev)
        comm.all_reduce(x, side)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(x, ref * 2.0)
        params = [torch.nn.Parameter(torch.zeros(1_000_000, device=DEV)), torch.nn.Parameter(torch.zeros(512, 1024, device=DEV))]
        red = dp.GradBucketReducer(params, bucket_mb=1.0, comm=comm, bucket_dtype=torch.bfloat16, exchange_at_world_1=True)
        assert len(red.buckets) >= 2 and red.stage.dtype == torch.bfloat16
        grad = (torch.randn(red.arena.numel(), generator=g) * 1e-3).to(DEV)
        red.arena.copy_(grad)
        red.begin_backward()
        out, scale = red.finish()
        torch.cuda.synchronize()
        rel = float((out - grad).norm() / grad.norm())
        cos = float(torch.nn.functional.cosine_similarity(out, grad, dim=0))
        print(f"bf16 bucket staging: relative L2 error {rel:.2e}, cosine {cos:.7f}")
        assert scale == 1.0 and rel <= 2.0 ** -8 and cos >= 0.99999
        assert torch.equal(out, grad.to(torch.bfloat16).float())          # exactly one rounding at one rank
    finally:
        comm.destroy()


def test_bench_two_ranks_rehearsal_on_one_gpu():
    """bench.py's N-rank control flow with N = 2 on ONE GPU (gloo rendezvous, both ranks on cuda:0; the real launch is RCCL,
    one device per rank): forward line and training line must come out -- barriers, max-over-ranks timing, rank-0-only
    legs, the bucket reducer's exchange in capture / replay / eager modes with train-mode LayerDrop drawing different
    layers per rank.  (Found in round 3: capture_all() launched all-reduces inside a capture; eager LayerDrop made the
    ranks launch their buckets in different orders.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MSMD_DIST_BACKEND="gloo", MSMD_ONE_DEVICE="1")
    for mode, port in (("forward", "29531"), ("train", "29532")):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", port, os.path.join(root, "bench.py"), "--gpus", "2",
                            "--steps", "2", "--warmup", "1", "--mode", mode, "--full", "--no-cpu-baseline"],
                           capture_output=True, text=True, env=env, timeout=900, cwd=root)
        assert r.returncode == 0, (mode, r.stderr[-3000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1, (mode, r.stdout[-2000:])
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "weak"
        assert "roofline" in d


def test_bench_eight_ranks_rehearsal_on_one_gpu():
    """The same with EIGHT ranks in --mode train with hipGraph segments (the launch the driver makes on an 8-GPU node, RCCL
    there): eight real processes on cuda:0 go through rendezvous, capture, the bucket reducer's exchange between graph
    segments in bucket order, the all-rank non-finite stop and rank 0's line.  8 clips per rank (at the real 32 eight ranks
    need 8 x 36 GB of the one device); children by subprocess only -- no exec of a process that has initialised the GPU."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MSMD_DIST_BACKEND="gloo", MSMD_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8",
                        "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(root, "bench.py"), "--gpus", "8",
                        "--steps", "2", "--warmup", "1", "--mode", "train", "--batch", "8", "--full", "--no-cpu-baseline"],
                       capture_output=True, text=True, env=env, timeout=1500, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["value"] > 0 and d["scaling"] == "weak" and d["config"]["parallelism"] == "dp8"
    assert "hipGraph" in d["config"]["launch"]


def test_first_graph_replay_after_another_variant_equals_the_eager_backward():
    """Segmented hipGraphs of the four truncation variants share one memory pool and alternate from iteration to iteration.
    Every gradient of the FIRST replay of a variant after another variant (and an optimizer step) has run must equal the
    eager backward from the same parameters, inputs and injected draws -- not only later replays of the same variant, which
    is all a replay-vs-replay comparison sees.  (Round 4: null_audio_feat's gradient was off by O(1) on exactly those first
    replays -- the host library's multi-block reduction behind torch.where's expand; train_graph.NullTokenSelectFn.)"""
    import os
    from msmd_amd import autograd as ag
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    old = os.environ.get("MSMD_SEGMENT_GRAPHS")
    os.environ["MSMD_SEGMENT_GRAPHS"] = "1"
    try:
        args = default_args(compute_dtype="bf16", encoder_layers=3, n_layers=2, lr=2e-5, warm_iter=0, gradient_accumulation_steps=1)
        B = 8
        torch.manual_seed(0)
        model = get_diffusion_model(args, DEV).eval()
        se = get_style_encoder(args, "vae2").to(DEV).eval()
        tr = Trainer(args, model, se, use_graph=True, bucket_mb=4.0)
        red = tr.reducer
        names = {id(p): "se." + n for n, p in se.named_parameters()}
        names.update({id(p): n for n, p in model.named_parameters()})

        def backward(batch, draws, graph):
            ag.DIRECT_GRAD = tr.direct_grad
            cross, trunc = tr._host_choices(draws)
            ag.TrainNoise.graph_safe, ag.TrainNoise.spec_masks = graph, None
            red.arena.zero_()
            red.begin_backward()
            tr._stepping, red.enabled = True, False
            (tr._graph_fwd_bwd if graph else tr._fwd_bwd)(batch, draws, trunc, cross)
            red.finish()
            torch.cuda.synchronize()
            return red.arena.clone()

        for it in range(1, 9):
            g = np.random.RandomState(100 + it)
            batch = synthetic_batch(B, 0, DEV, it=it % 3)
            draws = dict(cross=[bool(g.rand() < 0.5), False], end_idx=[dev(g.randint(1, 100, size=B)) if it % 2 else None, None],
                         t=[g.randint(1, 501, size=B).tolist() for _ in range(2)],
                         eps=[dev(g.standard_normal((B, 100, 67)).astype(np.float32)) for _ in range(2)],
                         style_eps=[dev(g.standard_normal((B, 256)).astype(np.float32)) for _ in range(2)],
                         cfg_flag=[dev(g.rand(B).astype(np.float32)) for _ in range(2)])
            tr.noise_state[1] += 1
            first = backward(batch, draws, True)        # the variants alternate: this replay follows the OTHER variant's
            again = backward(batch, draws, True)
            eager = backward(batch, draws, False)
            for p in red.params:
                _, off, n = red.slot[id(p)]
                scale = float(eager[off:off + n].abs().max())
                for tag, got in (("first replay", first), ("second replay", again)):
                    d = float((got[off:off + n] - eager[off:off + n]).abs().max())
                    assert d <= 1e-5 * max(scale, 1e-12) + 1e-9, (it, tag, names[id(p)], d, scale)
            red.arena.copy_(eager)
            tr._optimizer_step()
    finally:
        if old is None:
            os.environ.pop("MSMD_SEGMENT_GRAPHS", None)
        else:
            os.environ["MSMD_SEGMENT_GRAPHS"] = old


def test_checkpoint_moments_land_on_their_parameters_across_arena_layouts(tmp_path):
    """Trainer.load_checkpoint remaps the flat Adam moments parameter by parameter from the WRITER's arena order to this
    trainer's: (1) a checkpoint written by this build (arena_order recorded: the encoder's Q / K / V pulled together),
    (2) one written before round 3 (no arena_order: plain reverse registration order, ALIGN-rounded offsets).  Each parameter's
    slice of exp_avg / exp_avg_sq carries a recognisable per-parameter pattern; a wrong offset would only show up as slightly
    wrong optimizer state after a resume.  A moments tensor whose length does not match the order is refused."""
    from msmd_amd import dp
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer
    args = default_args(compute_dtype="bf16", encoder_layers=2, n_layers=1, lr=1e-4, warm_iter=0)
    tr = Trainer(args, get_diffusion_model(args, DEV).eval(), get_style_encoder(args, "vae2").to(DEV).eval())
    named = tr._named_trainable()
    code = {n: float(i + 1) for i, (n, _) in enumerate(named)}
    al = lambda k: (k + dp.ALIGN - 1) // dp.ALIGN * dp.ALIGN

    def moments(order):
        m = torch.zeros(sum(al(p.numel()) for _, p in named))
        off = 0
        for n in order:
            k = dict(named)[n].numel()
            m[off:off + k] = code[n] + torch.arange(k) * 1e-7
            off += al(k)
        return m

    base = tr.flat_param.data_ptr()
    for tag, order, record in (("this build", tr._arena_names(), True),
                               ("before round 3", [n for n, _ in named][::-1], False)):
        assert (order == tr._arena_names()) == record      # the two layouts really differ (Q / K / V adjacency)
        opt = {"exp_avg": moments(order), "exp_avg_sq": moments(order) * 2, "step": 7,
               "layout": [(n, int(p.numel())) for n, p in named]}
        if record:
            opt["arena_order"] = order
        ck = {"args": args, "model": tr.model.state_dict(), "style_enc": tr.style_enc.state_dict(), "iter": 3, "optimizer": opt}
        path = tmp_path / f"ck_{record}.pt"
        torch.save(ck, path)
        tr.exp_avg.zero_(); tr.exp_avg_sq.zero_()
        assert tr.load_checkpoint(path) == 3 and tr.opt_step == 7
        for n, p in named:
            dst, k = (p.data_ptr() - base) // 4, p.numel()
            want = code[n] + torch.arange(k) * 1e-7
            assert torch.equal(tr.exp_avg[dst:dst + k].cpu(), want), (tag, n)
            assert torch.equal(tr.exp_avg_sq[dst:dst + k].cpu(), want * 2), (tag, n)
    bad = dict(ck)
    bad["optimizer"] = dict(opt, exp_avg=opt["exp_avg"][:-dp.ALIGN])
    with pytest.raises(ValueError, match="optimizer moments hold"):
        tr.load_checkpoint(bad)
