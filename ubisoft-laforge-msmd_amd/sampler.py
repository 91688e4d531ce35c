"""CFG + DDPM ancestral sampler (reference model.py:283-440) driven from the host, arithmetic in HIP.

Per step the device runs: pack x_t into the denoiser input -> decoder trunk -> heads/static mix ->
one fused CFG-combine + DDPM-posterior kernel that updates x_t in place.  Step-invariant work is
hoisted out of the T x n_entries loop: cross-attention K/V projections of
the audio memory for all layers, the static-style bases, the person projection and ALL T step
embeddings (one GEMM pair).  Nothing is copied to the host inside the loop (the reference moves
traj[t] to the CPU every step, model.py:433); per-step scalars come from host copies of the schedule.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import ops

SOLVERS = ("ddpm", "ddim", "dpmpp_2m")


def check_solver(T, sample_steps=None, solver="ddpm", eta=0.0, flexibility=0):
    """Validate the sampler's solver arguments; returns the step count S."""
    if solver not in SOLVERS:
        raise ValueError(f"Unknown solver {solver!r}; expected one of {SOLVERS}")
    if solver == "ddpm":
        if sample_steps not in (None, T):
            raise ValueError(f"solver='ddpm' runs all T = {T} steps (got sample_steps={sample_steps}); for fewer "
                             f"ancestral steps use solver='ddim', eta=1")
        return T
    if flexibility != 0:
        raise ValueError(f"flexibility applies to solver='ddpm' only; solver={solver!r} takes eta instead")
    if solver == "ddim" and not 0.0 <= eta <= 1.0:
        raise ValueError(f"eta must lie in [0, 1], got {eta}")
    if solver == "dpmpp_2m" and eta != 0:
        raise ValueError("solver='dpmpp_2m' is deterministic: eta must be 0")
    S = T if sample_steps is None else sample_steps
    if isinstance(S, bool) or int(S) != S or not 1 <= S <= T:
        raise ValueError(f"sample_steps must be an integer in [1, {T}], got {sample_steps}")
    return int(S)


def solver_table(sched, steps, solver, eta=0.0, target="sample"):
    """Timesteps and per-step coefficients of a few-step solver in data-prediction (x0) form, in float64.

    taus[i] = round(i T / S) (half up), i = 0..S ("trailing" spacing: taus[S] = T, taus[0] = 0).  Step i = S..1 goes
    from s = taus[i] to t = taus[i-1]; rows[i] = (p0, p1, ax, ath, b1, sigma) is what msmd_cfg_solver_step applies:
    D = p0 x + p1 theta, x <- ax x + ath theta + b1 D_prev + sigma z.  With alpha_u = sqrt(abar_u), sigma_u =
    sqrt(1 - abar_u), lambda_u = ln(alpha_u / sigma_u), each solver is x <- a x + b0 D + b1 D_prev + sig z:
      ddim(eta):  sig = eta sqrt((1 - abar_t) / (1 - abar_s)) sqrt(1 - abar_s / abar_t),
                  a = sqrt(1 - abar_t - sig^2) / sigma_s, b0 = alpha_t - a alpha_s, b1 = 0;
      dpmpp_2m:   the ddim(0) row for the first step (i = S) and the last (t = 0); otherwise, with h = lambda_t - lambda_s
                  and r = h_prev / h: a = sigma_t / sigma_s, b0 = -alpha_t (e^-h - 1)(1 + 1/(2r)),
                  b1 = alpha_t (e^-h - 1) / (2r), sig = 0.
    ax = a + b0 p0 and ath = b0 p1 are folded here (for target 'noise', p0 = 1/alpha_s reaches ~1e4 at s = T and would
    cancel in fp32 on the device).  Row 0 is unused (zeros)."""
    T = int(sched.num_steps)
    S = check_solver(T, steps, solver, eta)
    if solver == "ddpm":
        raise ValueError("solver='ddpm' has no solver table: its per-step coefficients are the reference's")
    if target not in ("sample", "noise"):
        raise ValueError("Unknown target type: {}".format(target))
    ab = sched.alpha_bars.detach().cpu().double()
    taus = [(2 * i * T + S) // (2 * S) for i in range(S + 1)]
    al = lambda u: float(torch.sqrt(ab[u]))
    sg = lambda u: float(torch.sqrt(1 - ab[u]))
    lam = lambda u: math.log(al(u) / sg(u))
    rows = torch.zeros(S + 1, 6, dtype=torch.float64)
    h_prev = None
    for i in range(S, 0, -1):
        s, t = taus[i], taus[i - 1]
        abs_, abt = float(ab[s]), float(ab[t])
        if solver == "dpmpp_2m" and i != S and t != 0:
            h = lam(t) - lam(s)
            r = h_prev / h
            em1 = math.expm1(-h)
            a = sg(t) / sg(s)
            b0 = -al(t) * em1 * (1 + 1 / (2 * r))
            b1 = al(t) * em1 / (2 * r)
            sig = 0.0
        else:
            e = eta if solver == "ddim" else 0.0
            sig = e * math.sqrt((1 - abt) / (1 - abs_)) * math.sqrt(max(1 - abs_ / abt, 0.0))
            a = math.sqrt(max(1 - abt - sig * sig, 0.0)) / sg(s)
            b0 = al(t) - a * al(s)
            b1 = 0.0
        if solver == "dpmpp_2m" and t != 0:
            h_prev = lam(t) - lam(s)
        p0, p1 = (0.0, 1.0) if target == "sample" else (1 / al(s), -sg(s) / al(s))
        rows[i] = torch.tensor([p0, p1, a + b0 * p0, b0 * p1, b1, sig], dtype=torch.float64)
    return taus, rows


def ddpm_table(sched, flexibility=0, target="sample"):
    """Per-step coefficients of the reference's ancestral chain (model.py:383-395) as one fp32 host table of shape (T+1, 3).

    Row t = (c0, c1, sigma) is what msmd_cfg_ddpm_step applies on the step from t to t - 1:
      target 'sample':  x <- c0 x + c1 theta + sigma z,  c0 = (1 - abar_{t-1}) sqrt(alpha_t) / (1 - abar_t),
                                                        c1 = (1 - alpha_t) sqrt(abar_{t-1}) / (1 - abar_t);
      target 'noise':   x <- c0 (x - c1 theta) + sigma z,  c0 = 1 / sqrt(alpha_t),  c1 = (1 - alpha_t) / sqrt(1 - abar_t);
      sigma = sigmas_flex[t] flexibility + sigmas_inflex[t] (1 - flexibility).
    Every operation is the reference's fp32 tensor operation in the reference's order, on whole columns of
    sched.host_tables() instead of one element at a time, so each entry has the bits the reference computes.  Row 1's sigma
    is 0 (the last step adds no noise: z = 0 at t = 1); row 0 is unused (zeros)."""
    if target not in ("sample", "noise"):
        raise ValueError("Unknown target type: {}".format(target))
    tab = sched.host_tables()
    alpha, alpha_bar, alpha_bar_prev = tab["alphas"][1:], tab["alpha_bars"][1:], tab["alpha_bars"][:-1]
    sigma = tab["sigmas_flex"][1:] * flexibility + tab["sigmas_inflex"][1:] * (1 - flexibility)
    if target == "noise":
        c0 = 1 / torch.sqrt(alpha)
        c1 = (1 - alpha) / torch.sqrt(1 - alpha_bar)
    else:
        c0 = (1 - alpha_bar_prev) * torch.sqrt(alpha) / (1 - alpha_bar)
        c1 = (1 - alpha) * torch.sqrt(alpha_bar_prev) / (1 - alpha_bar)
    table = torch.zeros(int(sched.num_steps) + 1, 3)
    table[1:] = torch.stack([c0, c1, sigma], dim=1)
    table[1, 2] = 0.0
    return table


# The update rule of one sample() call, for both loops: they take steps i = steps .. 1, and step i leaves timestep times[i] for
# times[i - 1].  table: (steps + 1, width) fp32 on the host, row i = the step's coefficients; the eager loop passes the row
# as scalars and the graph loop copies the table to the device, so both apply the same bits.  noisy[i]: step i takes a draw z
# (noise[times[i]], or one generator call); the others get z = None.  has_d_prev: the step also reads and writes the previous
# data prediction.  select(emb_all, coef_table, t_dev, emb_row, coefs): row t_dev of both tables, on the device.
# step / step_dev(o, x, dec, res, z, d_prev, row, i): the fused CFG combine + update of step i with the row as host scalars and
# i a host integer / with the row in device memory and i the device-side counter (already decremented to i - 1 by select).  A
# few-step rule with streams=True takes the pair that also writes sample_separate's streams (o.cum_static, o.theta_dyn,
# o.theta_alpha) from dec; the others ignore dec and i.
_Rule = namedtuple("_Rule", "name target steps times table noisy has_d_prev select step step_dev")


def _update_rule(sched, solver, steps, eta, flexibility, target, streams=False):
    tgt = 0 if target == "sample" else 1
    if solver == "ddpm":
        # the reference's ancestral chain: every timestep T .. 1, a draw for every t > 1
        T = int(sched.num_steps)
        return _Rule(
            solver, tgt, T, list(range(T + 1)), ddpm_table(sched, flexibility, target), [t > 1 for t in range(T + 1)], False,
            ops.sampler_step_select,
            lambda o, x, dec, res, z, d_prev, row, i: ops.cfg_ddpm_step(x, res, z, o.scales, o.n_entries, o.Lp, o.mode, tgt, *row),
            lambda o, x, dec, res, z, d_prev, row, i: ops.cfg_ddpm_step_dev(x, res, z, o.scales, row, o.n_entries, o.Lp, o.mode,
                                                                        tgt))
    # a few-step solver draws only where its row's sigma is not 0; its float64 rows are rounded to fp32 here as the scalar
    # arguments of msmd_cfg_solver_step are
    taus, rows = solver_table(sched, steps, solver, eta, target)
    if streams:
        # theta_alpha's row block: the step ordinal steps - i when every step's blend weights are kept, else 0
        step = lambda o, x, dec, res, z, d_prev, row, i: ops.cfg_streams_step(
            x, res, dec, o.stat, z, o.scales, d_prev, o.cum_static, o.theta_dyn, o.theta_alpha,
            steps - i if o.theta_alpha.shape[0] > o.B else 0, o.n_entries, o.Lp, o.nb, o.head_alpha_bits, o.mode, *row)
        step_dev = lambda o, x, dec, res, z, d_prev, row, i: ops.cfg_streams_step_dev(
            x, res, dec, o.stat, z, o.scales, d_prev, o.cum_static, o.theta_dyn, o.theta_alpha, row, i, o.n_entries, o.Lp,
            o.nb, o.head_alpha_bits, o.mode)
    else:
        step = lambda o, x, dec, res, z, d_prev, row, i: ops.cfg_solver_step(x, res, z, o.scales, d_prev, o.n_entries, o.Lp,
                                                                             o.mode, *row)
        step_dev = lambda o, x, dec, res, z, d_prev, row, i: ops.cfg_solver_step_dev(x, res, z, o.scales, d_prev, row,
                                                                                     o.n_entries, o.Lp, o.mode)
    return _Rule(solver, tgt, steps, taus, rows.float(), (rows[:, 5] != 0).tolist(), True, ops.sampler_solver_select, step,
                 step_dev)


def dense_guidance(indices, values, B, L, dm):
    """Keyframes (indices, values) as msmd_denoiser_pack_input_guided takes them: (mask (B, L) uint8, dense (B, L, dm) fp32) on
    the host, the result of `motion_in[:, indices, :] = values` (reference model.py:762-767) restated as "which frames, and
    what they hold".  indices: anything that indexes a length-L axis (int, int list / array / tensor, slice, bool mask of
    length L, negative entries); out of range raises IndexError.  values is broadcast to (B, G, dm), G = the number of frames
    indexed.  Where an index repeats the last occurrence wins (numpy's assignment rule, which oracle/diffusion.py follows)."""
    if not isinstance(indices, slice):
        indices = indices.detach().cpu().numpy() if torch.is_tensor(indices) else np.asarray(indices)
        if indices.size == 0:
            indices = indices.astype(np.int64)         # an empty list is an empty float array to numpy
    pos = np.arange(L)[indices]                        # numpy's own index rules, IndexError included
    if pos.ndim > 1:
        raise IndexError(f"keyframe indices must index one axis of length {L}, got an index of shape {pos.shape}")
    vals = values.detach().float().cpu().numpy() if torch.is_tensor(values) else np.asarray(values, dtype=np.float32)
    if pos.ndim == 0:
        pos, vals = pos[None], np.broadcast_to(vals, (B, dm))[:, None, :]
    vals = np.broadcast_to(vals, (B, len(pos), dm))
    mask, dense = np.zeros((B, L), np.uint8), np.zeros((B, L, dm), np.float32)
    for g, t in enumerate(pos.tolist()):               # in order: a repeated frame keeps its last value
        dense[:, t] = vals[:, g]
        mask[:, t] = 1
    return torch.from_numpy(mask), torch.from_numpy(dense)


class DenseGuide(namedtuple("DenseGuide", "mask values")):
    """Keyframes already in the dense form (dense_guidance's pair, any device), for callers whose clips pin different frames:
    pass it as the `indices` of a guidance pair with values None (inference.infer_coeffs_batch does)."""

    @staticmethod
    def stack(pairs, L, dm):
        """One clip per entry of `pairs`: (indices, values) or None (no keyframes in that clip)."""
        each = [dense_guidance(*p, 1, L, dm) if p is not None else dense_guidance([], np.zeros((0, dm), np.float32), 1, L, dm)
                for p in pairs]
        return DenseGuide(torch.cat([m for m, _ in each]), torch.cat([v for _, v in each]))


class _Operands(namedtuple("_Operands", "net P dtype dev B n_entries N L Lp dm nb mode dyn "
                                        "prev_m ind mem kv_list cross_list stat tok_person emb_all scales "
                                        "guide_mask guide_values alpha_mod cum_static theta_dyn theta_alpha",
                             defaults=(None,) * 6)):
    """Everything the hoisted section of sample() produces and a denoising step consumes.  N = n_entries * B rows, entry-major;
    mode: the CFG combine, 0 incremental / 1 independent; dyn: the dynamic threshold's (ratio, min, max) or None; stat has B rows
    or one; emb_all has one step embedding per row of the rule's table; ind, cross_list and scales may be None.  A lane of the
    graph loop holds the same record with B, N and the tensors of its own rows (_Lane).
    Few-step solvers only (the DDPM chain keeps these None): guide_mask (B, L) uint8 / guide_values (B, L, dm), the keyframes
    that overwrite the denoiser input in the pack kernel; alpha_mod, sample_separate's callable on the blend weights; cum_static
    and theta_dyn (B, L, dm) and theta_alpha (n_slots B, L, nb), the streams the streams step writes."""

    @property
    def head_alpha_bits(self):
        """msmd_heads_static_mix's use_head_alpha argument."""
        return int(bool(self.net.use_head_alpha)) | (2 if self.net.regularize_alpha == "sigmoid" else 0)

    def trunk(self, x, feats, emb_row):
        """pack x (keyframes overwritten where a guide is set) into the denoiser input -> decoder trunk; returns dec
        (N, Lp + L, dm + nb)."""
        if self.guide_mask is not None:
            ops.denoiser_pack_input_guided(x, self.prev_m, self.ind, feats, self.guide_mask, self.guide_values)
        else:
            ops.denoiser_pack_input(x, self.prev_m, self.ind, feats)
        return self.net.trunk(feats, self.tok_person, self.mem, self.dtype, kv_list=self.kv_list, row0_add=emb_row,
                              cross_list=self.cross_list)

    def threshold(self, res):
        if self.dyn:
            # K15 (off in the reference's inference driver, inference.py:272): quantile + clamp in one launch
            res = ops.dynamic_threshold_(res.float().contiguous(), self.L, *self.dyn)
        return res

    def heads(self, dec):
        """heads / static mix -> optional dynamic threshold; returns res (N, Lp + L, dm).  alpha_mod (eager loop only: an
        arbitrary host callable) rewrites dec's blend-weight columns first, so the mix and the streams step read its result.
        It sees the decoder's raw columns: with regularize_alpha='sigmoid' those are logits (the kernels apply the sigmoid after it,
        where the reference's callable sees the weights after the sigmoid, model.py:973 then :560), and its result is stored in
        dec's dtype."""
        if self.alpha_mod is not None:
            dec[..., self.dm:] = self.alpha_mod(dec[..., self.dm:])
        return self.threshold(ops.heads_static_mix(dec, self.stat, self.Lp + self.L, self.dm, self.nb, self.net.use_head_alpha,
                                                   self.net.regularize_alpha == "sigmoid"))


class _Streams:
    """sample_separate's step (reference model.py:442-651): the diagnostic variant that also tracks the dynamic / static /
    alpha streams, in host-library tensor algebra on (N, 110, 4, 67)-sized data."""

    def __init__(self, o, x, separate, cfg_scale):
        self.o, self.sep, self.cfg_scale = o, separate, cfg_scale
        self.cum_static, self.alpha_traj = torch.zeros_like(x), []
        self.stat_full = o.stat[torch.arange(o.N, device=o.dev) % o.stat.shape[0]]  # (N, nb, dm): real style for every entry

    def step(self, dec, x, z, target, row):
        o, (c0, c1, sigma) = self.o, row
        dyn, alpha_t = dec[..., :o.dm], dec[..., o.dm:]
        if self.sep.get("alpha_mod") is not None:
            alpha_t = self.sep["alpha_mod"](alpha_t)
        sf = self.stat_full[:, None]  # (N, 1, nb, dm)
        if o.net.use_head_alpha:
            static = (sf * alpha_t.unsqueeze(-1)).sum(dim=2)
        else:
            static = torch.cat([(sf[..., :-3] * alpha_t.unsqueeze(-1)).sum(dim=2),
                                sf[..., -3:].sum(dim=2).expand(-1, o.Lp + o.L, -1)], dim=-1)
        res = o.threshold(dyn + static)
        streams = [list(v.contiguous().clone().chunk(o.n_entries)) for v in (res, static, dyn, alpha_t)]
        heads = [st[0][:, -o.L:] for st in streams]  # views: in-place accumulation as the reference (model.py:590-618)
        for i in range(o.n_entries - 1):
            for st, hd in zip(streams, heads):
                base = st[0] if o.mode == 1 else st[i]
                hd += self.cfg_scale[i] * (st[i + 1][:, -o.L:] - base[:, -o.L:])
        theta, theta_static, self.theta_dyn, self.theta_alpha = heads
        zz = z if z is not None else torch.zeros_like(x)
        if target == 1:
            x = c0 * (x - c1 * theta) + sigma * zz
        else:
            x = c0 * x + c1 * theta + sigma * zz
        self.cum_static = self.cum_static + c1 * theta_static
        self.alpha_traj.append(self.theta_alpha)
        return x

    def outputs(self):
        last_alpha = torch.cat(self.alpha_traj, dim=0) if self.sep.get("return_all_alpha") else self.theta_alpha
        return self.theta_dyn, self.cum_static, last_alpha


def _entries(cfg_cond, cfg_mode):
    """(use_audio, use_style) per CFG entry in batch order; entry 0 is the null entry (model.py:340-366)."""
    ent = [("audio" not in cfg_cond, "style" not in cfg_cond)]
    for cond in cfg_cond:
        if cond == "audio":
            ent.append((True, "style" not in cfg_cond))
        elif cond == "style":
            if cfg_mode == "independent":
                ent.append(("audio" not in cfg_cond, True))
            elif cfg_mode == "incremental":
                ent.append((True, True))
            else:
                raise NotImplementedError(f"Unknown cfg_mode {cfg_mode}")
    return ent


def sample(model, audio_or_feat, shape_feat, style_feat=None, prev_motion_feat=None, prev_audio_feat=None,
           motion_at_T=None, indicator=None, cfg_mode=None, cfg_cond=None, cfg_scale=1.15, flexibility=0,
           dynamic_threshold=None, ret_traj=False, noise=None, guidance=None, separate=None, sample_steps=None,
           solver="ddpm", eta=0.0):
    """guidance = (indices, values): naive in-painting of the denoiser INPUT (reference model.py:762-767).
    separate = dict(alpha_mod=callable|None, return_all_alpha=bool): also track the dynamic / static / alpha
    streams (reference sample_separate, model.py:442-651).
    solver: "ddpm" (the reference's ancestral chain over all T steps), or "ddim" (eta in [0, 1]) / "dpmpp_2m" over
    sample_steps timesteps (solver_table); noise is then keyed by the source timestep of each step.
    With a few-step solver guidance and separation (alone or together) are part of the one step body: the keyframes overwrite the
    denoiser input inside the pack kernel (dense_guidance; indices may also be a DenseGuide with values None) and the streams are
    written by the streams step (msmd_cfg_streams_step), cum_static accumulating ath theta_static; x0 has the bits of the plain
    call.  They take the hipGraph loop under sample()'s own rule unless alpha_mod is set.  solver="ddpm" keeps the reference's
    tensor algebra (_Streams, index put) in the eager loop."""
    S = check_solver(model.diffusion_sched.num_steps, sample_steps, solver, eta, flexibility)
    few = solver != "ddpm"
    if few and guidance is not None and guidance[0] is None:
        guidance = None                      # no keyframes: the plain body (the DDPM chain keeps its own test of the pair below)
    if not few and guidance is not None and isinstance(guidance[0], DenseGuide):
        raise ValueError("per-clip keyframes (DenseGuide) need solver='ddim' or 'dpmpp_2m'; solver='ddpm' takes (indices, values)")
    net = model.denoising_net
    dtype = model.compute_dtype
    dev = model.device
    batch_size = audio_or_feat.shape[0]
    if cfg_mode is None:
        cfg_mode = model.cfg_mode
    if cfg_cond is None:
        cfg_cond = model.guiding_conditions
    cfg_cond = [c for c in cfg_cond if c in ["audio", "style"]]
    if not isinstance(cfg_scale, list):
        cfg_scale = [cfg_scale] * len(cfg_cond)
    if len(cfg_cond) > 0:
        cfg_cond, cfg_scale = zip(*sorted(zip(cfg_cond, cfg_scale), key=lambda x: ["audio", "style"].index(x[0])))
    else:
        cfg_cond, cfg_scale = [], []
    if cfg_mode not in ("incremental", "independent") and len(cfg_cond) > 0:
        raise NotImplementedError(f"Unknown cfg_mode {cfg_mode}")
    if model.target not in ("sample", "noise"):
        raise ValueError("Unknown target type: {}".format(model.target))
    if "style" in cfg_cond:
        assert model.use_style and style_feat is not None
    if model.use_style:
        if style_feat is None:
            style_feat = model.null_style_feat.expand(batch_size, -1, -1)
    else:
        assert style_feat is None, "This model does not support style feature input!"

    if audio_or_feat.ndim == 2:
        assert audio_or_feat.shape[1] == 16000 * model.n_motions / model.fps, \
            f"Incorrect audio length {audio_or_feat.shape[1]}"
        audio_feat = model._audio_feat(audio_or_feat, model.n_motions, dtype).float()
    elif audio_or_feat.ndim == 3:
        assert audio_or_feat.shape[1] == model.n_motions, f"Incorrect audio feature length {audio_or_feat.shape[1]}"
        audio_feat = audio_or_feat
    else:
        raise ValueError(f"Incorrect audio input shape {audio_or_feat.shape}")
    if shape_feat.ndim == 2:
        shape_feat = shape_feat.unsqueeze(1)
    if style_feat is not None and style_feat.ndim == 2:
        style_feat = style_feat.unsqueeze(1)
    if shape_feat.shape[0] != batch_size:
        shape_feat = shape_feat.expand(batch_size, -1, -1)
    if prev_motion_feat is None:
        prev_motion_feat = model.start_motion_feat.expand(batch_size, -1, -1)
    if prev_audio_feat is None:
        prev_audio_feat = model.start_audio_feat.expand(batch_size, -1, -1)
    if motion_at_T is None:
        motion_at_T = torch.randn((batch_size, model.n_motions, model.motion_feat_dim)).to(dev)

    L, Lp, dm, nb = model.n_motions, model.n_prev_motions, net.motion_feat_dim, net.num_of_basis
    null_audio = model.null_audio_feat.expand(batch_size, L, -1) if "audio" in cfg_cond else audio_feat
    audio_in, person_in = [], []
    for use_a, use_s in _entries(cfg_cond, cfg_mode):
        audio_in.append(audio_feat if use_a else null_audio)
        st = style_feat if (use_s or "style" not in cfg_cond) else model.null_style_feat.expand(batch_size, -1, -1)
        person_in.append(torch.cat([shape_feat, st], dim=-1) if model.use_style else shape_feat)
    n_entries = len(audio_in)
    N = n_entries * batch_size
    audio_in = torch.cat(audio_in, dim=0)
    person_in = torch.cat(person_in, dim=0)
    prev_m = torch.cat([prev_motion_feat] * n_entries, dim=0).float().contiguous()
    prev_a = torch.cat([prev_audio_feat] * n_entries, dim=0)
    ind_in = torch.cat([indicator] * n_entries, dim=0).float().contiguous() if indicator is not None else None
    if net.use_indicator and ind_in is None:
        raise TypeError("expected Tensor as element 1 in argument 0, but got NoneType")  # reference model.py:944

    # ---- step-invariant work, hoisted
    P = net.pack(dtype)
    T = model.diffusion_sched.num_steps
    rule = _update_rule(model.diffusion_sched, solver, S, eta, flexibility, model.target, streams=few and separate is not None)
    mem = torch.cat([ops.cast(prev_a.contiguous(), dtype), ops.cast(audio_in.contiguous(), dtype)], dim=1)
    kv_list = net.memory_kv(mem, dtype)
    cross_list = net.memory_cross(kv_list, dtype) if (P.diag and getattr(net, "diag_fast_path", True)) else None
    stat = net.static_bases(style_feat, dtype).float().contiguous()  # real style for every entry (model.py:374)
    pf = ops.pad_cols(person_in.reshape(N, -1).float().contiguous(), P.kp_person, dtype)
    tok_person = ops.gemm(pf, *P.pp)                                   # (N, d) without the step embedding
    # a few-step solver: only the rows it visits (emb_all[i] is the step embedding of timestep taus[i])
    te = P.te[: T + 1] if solver == "ddpm" else P.te[torch.as_tensor(rule.times, device=P.te.device)]
    te_all = ops.cast(te.contiguous(), dtype)
    emb_all = ops.gemm(ops.gemm(te_all, *P.ds0, act=ops.ACT_GELU), *P.ds2)  # (T+1, d); (S+1, d) for a few-step solver
    scales = torch.tensor(list(cfg_scale), device=dev, dtype=torch.float32) if n_entries > 1 else None
    o = _Operands(net=net, P=P, dtype=dtype, dev=dev, B=batch_size, n_entries=n_entries, N=N, L=L, Lp=Lp, dm=dm, nb=nb,
                  mode=1 if cfg_mode == "independent" else 0, dyn=tuple(dynamic_threshold) if dynamic_threshold else None,
                  prev_m=prev_m, ind=ind_in, mem=mem, kv_list=kv_list, cross_list=cross_list, stat=stat,
                  tok_person=tok_person, emb_all=emb_all, scales=scales)
    dense = None
    if few and guidance is not None:
        dense = guidance[0] if isinstance(guidance[0], DenseGuide) else DenseGuide(
            *dense_guidance(guidance[0], guidance[1], batch_size, L, dm))
        if tuple(dense.mask.shape) != (batch_size, L) or tuple(dense.values.shape) != (batch_size, L, dm):
            raise ValueError(f"dense keyframes must be ({batch_size}, {L}) / ({batch_size}, {L}, {dm}), got "
                             f"{tuple(dense.mask.shape)} / {tuple(dense.values.shape)}")
        dense = DenseGuide(dense.mask.to(dev, torch.uint8).contiguous(), dense.values.to(dev, torch.float32).contiguous())
    if few:
        if dense is not None:
            o = o._replace(guide_mask=dense.mask, guide_values=dense.values)
        if separate is not None:
            n_slots = S if separate.get("return_all_alpha") else 1
            o = o._replace(alpha_mod=separate.get("alpha_mod"),
                           cum_static=torch.zeros(batch_size, L, dm, device=dev), theta_dyn=torch.zeros(batch_size, L, dm, device=dev),
                           theta_alpha=torch.zeros(n_slots * batch_size, L, nb, device=dev))
    streams_out = lambda oo: (oo.theta_dyn, oo.cum_static, oo.theta_alpha) if few and separate is not None else ()

    if (noise is None and not ret_traj and getattr(model, "use_hip_graph", True) and T > 1
            and (few and o.alpha_mod is None or (guidance is None and separate is None))):
        x, outs = _graph_loop(model, o, rule, motion_at_T.float())
        return (x, motion_at_T, audio_feat) + streams_out(outs)

    x = motion_at_T.float().clone().contiguous()
    d_prev = torch.zeros_like(x) if rule.has_d_prev else None
    traj = {rule.times[-1]: motion_at_T} if ret_traj else None
    feats = torch.empty(N, 1 + Lp + L, P.kp_feat, device=dev, dtype=dtype)
    streams = _Streams(o, x, separate, cfg_scale) if separate is not None and not few else None
    for i in range(rule.steps, 0, -1):
        z = None
        if rule.noisy[i]:
            z = noise[rule.times[i]].float().contiguous() if noise is not None else torch.randn_like(x)
        row = rule.table[i].tolist()
        x_in = x
        if not few and guidance is not None and guidance[0] is not None:
            x_in = x.clone()
            x_in[:, guidance[0], :] = guidance[1].to(x_in.dtype)
        dec = o.trunk(x_in, feats, emb_all[i])
        if streams is None:
            rule.step(o, x, dec, o.heads(dec), z, d_prev, row, i)
        else:
            x = streams.step(dec, x, z, rule.target, row)
        if ret_traj:
            traj[rule.times[i - 1]] = x.clone()
    if ret_traj:
        return traj, motion_at_T, audio_feat
    if streams is not None:
        return (x, motion_at_T, audio_feat) + streams.outputs()
    return (x, motion_at_T, audio_feat) + streams_out(o)


# clamped to [1, 50]: k bodies in one graph keep k steps of intermediates alive in the graph's private pool (about 0.2 GB per
# step at B = 64, fp16: 2 GB at the default 10 of the 288 GB)
STEPS_PER_GRAPH = min(50, max(1, int(os.environ.get("MSMD_SAMPLER_STEPS_PER_GRAPH", "10"))))


# Lanes: the batch of a hipGraph loop is cut into LANES contiguous groups of clips; every group runs its own chain of denoising
# steps on a HIP stream of its own, forked and joined inside each captured graph.  Sequences are independent, so
# every lane computes exactly what it would compute alone; the lanes drift against each other, and one lane's launch tails,
# epilogue store bursts and small grids (person-token attention, heads, CFG / DDPM update) run under another lane's K loops.
# Used from MIN_LANE_SEQS sequences per lane up (a lane must still fill the chip on its own); MSMD_SAMPLER_LANES=1 turns it off.
LANES = min(4, max(1, int(os.environ.get("MSMD_SAMPLER_LANES", "2"))))
MIN_LANE_SEQS = 48


def _step_noise(B, L, dm, dev):
    """z ~ N(0, I) of one denoising step for the whole batch (reference model.py:383: torch.randn_like(x)); tests patch this."""
    return torch.randn(B, L, dm, device=dev, dtype=torch.float32)


class _Lane:
    """Static operand buffers + the step body of one lane (Bl clips x n_entries CFG entries, entry-major rows): the operands
    record of its own rows (self.o), the state x (and d_prev where the rule has one) and the device-side step counter."""

    def __init__(self, o, rule, shared, rows, clips):
        dev, Bl = o.dev, len(clips)
        take = lambda t, idx=rows: torch.zeros((len(idx),) + tuple(t.shape[1:]), device=dev, dtype=t.dtype)
        self.rule, self.shared = rule, shared
        self.rows, self.clips = rows, clips          # index tensors into the N-row / B-row operands of the whole batch
        self.x = torch.zeros(Bl, o.L, o.dm, device=dev, dtype=torch.float32)
        self.own_stat = o.stat.shape[0] == o.B and o.B > 1      # one row of static bases per clip (not one shared row)
        self.o = o._replace(
            B=Bl, N=len(rows), prev_m=take(o.prev_m), ind=take(o.ind) if o.ind is not None else None, mem=take(o.mem),
            kv_list=[take(k) for k in o.kv_list],
            cross_list=[take(r) for r in o.cross_list] if o.cross_list is not None else None,
            stat=take(o.stat, clips) if self.own_stat else shared.stat,
            tok_person=take(o.tok_person), emb_all=shared.emb_all, scales=shared.scales,
            # keyframes and the streams: static buffers of the lane's clips, like x (theta_alpha keeps the whole batch's slots)
            guide_mask=take(o.guide_mask, clips) if o.guide_mask is not None else None,
            guide_values=take(o.guide_values, clips) if o.guide_mask is not None else None,
            cum_static=take(o.cum_static, clips) if o.cum_static is not None else None,
            theta_dyn=take(o.theta_dyn, clips) if o.cum_static is not None else None,
            theta_alpha=torch.zeros(o.theta_alpha.shape[0] // o.B * Bl, o.L, o.nb, device=dev) if o.cum_static is not None
            else None)
        self.t_dev = torch.zeros(1, device=dev, dtype=torch.int32)
        self.emb_row = torch.zeros(o.emb_all.shape[-1], device=dev, dtype=o.emb_all.dtype)
        self.coefs = torch.zeros(rule.table.shape[1], device=dev, dtype=torch.float32)
        self.d_prev = torch.zeros_like(self.x) if rule.has_d_prev else None
        self.feats = torch.zeros(len(rows), 1 + o.Lp + o.L, o.P.kp_feat, device=dev, dtype=o.dtype)

    def body(self, z):
        o = self.o
        self.rule.select(o.emb_all, self.shared.coef_table, self.t_dev, self.emb_row, self.coefs)
        dec = o.trunk(self.x, self.feats, self.emb_row)
        # z: this lane's clips of the step's noise, drawn for the WHOLE batch on the forking stream (_StepGraph.bodies): what a
        # clip receives under a given seed does not depend on the lane count; sigma_1 = 0 reproduces z = 0 at t = 1
        self.rule.step_dev(o, self.x, dec, o.heads(dec), z, self.d_prev, self.coefs, self.t_dev)

    def load(self, motion_at_T, whole):
        """Copy this lane's rows of the whole batch's operands into its static buffers."""
        o = self.o
        self.x.copy_(motion_at_T[self.clips])
        if self.d_prev is not None:
            self.d_prev.zero_()
        if o.guide_mask is not None:
            o.guide_mask.copy_(whole.guide_mask[self.clips])
            o.guide_values.copy_(whole.guide_values[self.clips])
        if o.cum_static is not None:
            o.cum_static.zero_()
        o.prev_m.copy_(whole.prev_m[self.rows])
        o.mem.copy_(whole.mem[self.rows])
        if self.own_stat:
            o.stat.copy_(whole.stat[self.clips])
        o.tok_person.copy_(whole.tok_person[self.rows])
        if o.ind is not None:
            o.ind.copy_(whole.ind[self.rows])
        for dst, src in zip(o.kv_list, whole.kv_list):
            dst.copy_(src[self.rows])
        if o.cross_list is not None:
            for dst, src in zip(o.cross_list, whole.cross_list):
                dst.copy_(src[self.rows])


class _StepGraph:
    """k captured denoise steps per lane (one hipGraph): device-side step counters, static operand buffers.  The loop takes
    rule.steps steps (the schedule's T for DDPM, S for a few-step solver); no noise is drawn when no step of the rule is noisy."""

    def __init__(self, o, rule, lanes):
        B, dev, T, draw = o.B, o.dev, rule.steps, any(rule.noisy)
        self.lanes = lanes
        self.shared = SimpleNamespace(emb_all=torch.zeros_like(o.emb_all), stat=torch.zeros_like(o.stat),
                                      scales=torch.zeros_like(o.scales) if o.scales is not None else None,
                                      coef_table=torch.zeros_like(rule.table, device=dev))
        Bl = B // lanes
        self.lane = []
        for l in range(lanes):
            clips = torch.arange(l * Bl, (l + 1) * Bl, device=dev)
            rows = torch.cat([clips + e * B for e in range(o.n_entries)])
            self.lane.append(_Lane(o, rule, self.shared, rows, clips))
        self.streams = [torch.cuda.Stream() for _ in range(lanes)] if lanes > 1 else [None]

        def bodies(k):
            # one (B, L, dm) draw per step from the graph-safe philox stream, on the forking stream, sliced per lane: the same
            # generator calls whatever the lane count (each lane drawing its own made seeded output depend on MSMD_SAMPLER_LANES)
            zs = [_step_noise(B, o.L, o.dm, dev) if draw else None for _ in range(k)]
            if lanes == 1:
                for s_ in range(k):
                    self.lane[0].body(zs[s_])
                return
            cur = torch.cuda.current_stream()
            for li, (ln, st) in enumerate(zip(self.lane, self.streams)):     # fork ... every lane records its k steps back to back ...
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    for s_ in range(k):
                        ln.body(zs[s_][li * Bl:(li + 1) * Bl] if draw else None)
            for st in self.streams:                         # ... join
                cur.wait_stream(st)
        # With more than one lane the LayerNorm-epilogue GEMMs (QKV, out-projection, FFN-2 of a lane: M = 10 656 rows at B = 64) take
        # the 192 x 128 tile: alone on the chip its grids are short of a round (672 / 224 tiles on 512 slots) and the 128 x 128
        # tile wins, but beside another lane's launches the holes are filled and the larger tile's better loop shows (same box,
        # alternating: 2.286 -> 2.237, 2.208 -> 2.177 ms per step).  Same products in the same order: results are bit-identical.
        lane_tile = int(os.environ.get("MSMD_SAMPLER_LANE_TILE", "15")) or None      # developers' A/B: 0 = the library's own choice
        tile_keep, ops.GEMM_LN_TILE = ops.GEMM_LN_TILE, (lane_tile if lanes > 1 else ops.GEMM_LN_TILE)
        # warm-up on a side stream (allocator + lazy kernel loading), then capture
        for ln in self.lane:
            ln.t_dev.fill_(1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            bodies(1)
        torch.cuda.current_stream().wait_stream(side)
        # STEPS_PER_GRAPH consecutive denoising steps per captured graph (the step counter lives on the device, so the body is
        # simply recorded that many times): T / k replays instead of T.  k = the largest divisor of T up to the cap, so one
        # graph serves the whole loop.
        self.k = max(d for d in range(1, min(STEPS_PER_GRAPH, T) + 1) if T % d == 0)
        self.graph = torch.cuda.CUDAGraph()
        try:
            with ops.capture_guard():
                with torch.cuda.graph(self.graph):
                    bodies(self.k)
        finally:
            ops.GEMM_LN_TILE = tile_keep

    def run(self, o, rule, motion_at_T):
        for ln in self.lane:
            ln.load(motion_at_T, o)
        self.shared.emb_all.copy_(o.emb_all)
        self.shared.stat.copy_(o.stat)
        if self.shared.scales is not None:
            self.shared.scales.copy_(o.scales)
        self.shared.coef_table.copy_(rule.table)
        for ln in self.lane:
            ln.t_dev.fill_(rule.steps)
        for _ in range(rule.steps // self.k):
            self.graph.replay()
        x = torch.cat([ln.x for ln in self.lane], dim=0) if self.lanes > 1 else self.lane[0].x.clone()
        if o.cum_static is None:
            return x, o
        # the streams, concatenated across lanes as x is; a lane's theta_alpha is (n_slots, Bl, L, nb) in step order
        cat = lambda name: torch.cat([getattr(ln.o, name) for ln in self.lane], dim=0)
        alpha = torch.cat([ln.o.theta_alpha.view(-1, ln.o.B, o.L, o.nb) for ln in self.lane], dim=1).reshape(-1, o.L, o.nb)
        return x, o._replace(cum_static=cat("cum_static"), theta_dyn=cat("theta_dyn"), theta_alpha=alpha)


def _graph_loop(model, o, rule, motion_at_T):
    """The hipGraph loop: one resident _StepGraph per model, rebuilt when anything the capture depends on changes (guided or not,
    separated or not and the number of alpha slots included; which frames are pinned is an operand, not part of the key).
    Returns (x0, the operand record holding the streams of the whole batch)."""
    lanes = getattr(model, "sampler_lanes", LANES)
    while lanes > 1 and (o.B % lanes or o.N // lanes < MIN_LANE_SEQS):
        lanes -= 1
    key = (rule.steps, o.N, o.n_entries, o.Lp, o.L, o.mode, rule.target, o.dtype, o.ind is not None,
           getattr(o.net, "_pack_gen", 0), o.dyn, o.cross_list is not None, STEPS_PER_GRAPH, lanes, rule.name, any(rule.noisy),
           o.stat.shape[0], o.guide_mask is not None, o.cum_static is not None,
           o.theta_alpha.shape[0] // o.B if o.cum_static is not None else 0)
    cache = model.__dict__.setdefault("_step_graphs", {})
    g = cache.get(key)
    if g is None:
        cache.clear()  # one resident graph (its private memory pool holds all step intermediates)
        g = cache[key] = _StepGraph(o, rule, lanes)
    return g.run(o, rule, motion_at_T)
