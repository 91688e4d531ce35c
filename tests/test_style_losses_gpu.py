"""The style losses on the GPU (csrc/style_loss.hip) against the float64 run of tests/style_losses_ref.py.

Bounds (the convention of DESIGN.md 5.18, `style_losses_ref.allowed`): per case and per tensor, the float32 run of the
restatement against its float64 run is the yardstick; the device may be 8 x that far from the float64 truth, and is never held
to less than 4 fp32 ulp at the tensor's largest magnitude.  For a gradient tensor both sides are read relative to the tensor's
largest entry, which is the same inequality.  The translation identity sum_t dX + sum_k dS = 0 is held to the sum of the bounds
of the entries it adds (T of dX's and K of dS's).  Bit-for-bit claims (determinism, batch independence, the public classes
against the ops path, dX with and without dS) are exact comparisons.

Shapes: each axis at its edges around the kernels' tiles (R = ops.STYLE_ROWS rows, KT = ops.STYLE_KTILE style frames, 64-feature
chunks) with the others small, plus two mixed cases.  Every printed line `ERR <tensor> <error> <bound>` is a measurement."""
import functools
import pickle
import re

import numpy as np
import pytest
import torch

import style_losses_ref as R
from msmd_amd import _lib, ops, synth
from msmd_amd.autograd import NtXentFn, StyleAdherenceFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, KT = ops.STYLE_ROWS, ops.STYLE_KTILE
GUARD, MARK = 64, -7.0

# (B, T, K, F): T, K, F and B at their edges, then two mixed cases
SHAPES = ([(1, T, 5, 3) for T in (1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1)] +
          [(1, 3, K, 3) for K in (1, 2, KT - 1, KT, KT + 1, 2 * KT + 1)] +
          [(1, 3, 5, F) for F in (1, 3, 53, 64, 67, 130)] +
          [(3, 5, 7, 6), (3, 2 * ROWS + 1, 2 * KT + 1, 67), (2, ROWS + 1, KT + 1, 130)])
NT_SHAPES = [(1, 3), (2, 1), (2, 64), (16, 64), (16, 256), (33, 300), (33, 3)]


def dev(a):
    a = np.asarray(a)
    return torch.from_numpy(np.array(a, order="C")).to(DEV) if a.ndim else torch.tensor(a.item(), dtype=torch.float32, device=DEV)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def operands(B, T, K, F, planted=False, offset=0.0):
    """X (B, T, F), S (B, K, F) fp32, a different S per batch row.  planted: every X row is a style frame plus a little
    noise, so the smallest distance is far below the second smallest (an unambiguous arg-min)."""
    tag = f"style_loss/{B}x{T}x{K}x{F}"
    S = synth.normalish(tag + "/S", (B, K, F), 0.6)
    X = synth.normalish(tag + "/X", (B, T, F), 0.6)
    if planted:
        k = (7 * np.arange(T) + 3) % K
        X = (S[:, k] + np.float32(0.05) * X).astype(np.float32)
    X = (X + np.float32(offset)).astype(np.float32)
    for a in (X, S):
        a.setflags(write=False)
    return X, S


def upstream(B, T, reduce):
    return synth.normalish(f"style_loss/g/{B}x{T}", (B, T)) if not reduce else np.float32(1.7)


def row_gradient(up, B, T, reduce):
    return np.full((B, T), np.float64(up) / (B * T)) if reduce else up


@functools.lru_cache(maxsize=None)
def truth(B, T, K, F, lam, soft, reduce, planted=False, offset=0.0):
    """(value, dX, dS) in float64 and the bound of each, computed once per case."""
    X, S = operands(B, T, K, F, planted, offset)
    g = row_gradient(upstream(B, T, reduce), B, T, reduce)
    out = []
    for dt in (np.float64, np.float32):
        L = R.adherence_rows(X, S, lam, soft, dt)[0]
        out.append((L.mean(dtype=dt) if reduce else L,) + R.adherence_grads(X, S, g, lam, soft, dt))
    return out[0], tuple(R.allowed(t64, r32) for t64, r32 in zip(*out))


def check(name, got, want, bound):
    err = R.worst(got.detach().cpu().numpy(), want)
    scale = float(np.abs(want).max()) or 1.0
    print(f"ERR {name} {err / scale:.3e} {bound / scale:.3e}")
    assert np.isfinite(got.detach().cpu().numpy()).all() and err <= bound, (name, err, bound)


def run_fn(X, S, lam, soft, reduce, up, s_grad=True):
    x, s = dev(X).requires_grad_(True), dev(S).requires_grad_(s_grad)
    y = StyleAdherenceFn.apply(x, s, lam, soft, reduce)
    y.backward(dev(np.asarray(up, np.float32)))
    return y.detach(), x.grad, s.grad


# ------------------------------------------------------------------------------------------------ adherence against float64
@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_adherence_forward_and_gradients_against_float64(shape, soft):
    B, T, K, F = shape
    planted = not soft
    X, S = operands(B, T, K, F, planted)
    if not soft:
        assert R.second_smallest_gap(X, S) > 1e-3                     # the arg-min is unambiguous in every row
    for reduce in (True, False):
        (want, dX, dS), bounds = truth(B, T, K, F, 10.0, soft, reduce, planted)
        y, gx, gs = run_fn(X, S, 10.0, soft, reduce, upstream(B, T, reduce))
        assert y.shape == (() if reduce else (B, T)) and gx.shape == (B, T, F) and gs.shape == (B, K, F)
        tag = f"{'soft' if soft else 'hard'}/{'mean' if reduce else 'rows'}"
        check(tag + "/L", y, want, bounds[0])
        check(tag + "/dX", gx, dX, bounds[1])
        check(tag + "/dS", gs, dS, bounds[2])
        # the translation identity, within the bounds of the T + K entries it adds
        resid = gx.double().sum(1) + gs.double().sum(1)
        assert float(resid.abs().max()) <= T * bounds[1] + K * bounds[2]


@pytest.mark.parametrize("shape,lam", [((2, ROWS + 1, KT + 1, 53), 100.0), ((2, 5, 1, 53), 100.0), ((2, ROWS + 1, 1, 6), 10.0)],
                         ids=["lambda100", "lambda100_K1", "K1"])
def test_adherence_lambda_100_and_a_single_style_frame(shape, lam):
    B, T, K, F = shape
    X, S = operands(B, T, K, F)
    for reduce in (True, False):
        (want, dX, dS), bounds = truth(B, T, K, F, lam, True, reduce)
        y, gx, gs = run_fn(X, S, lam, True, reduce, upstream(B, T, reduce))
        check(f"lambda{lam:g}/K{K}/L", y, want, bounds[0])
        check(f"lambda{lam:g}/K{K}/dX", gx, dX, bounds[1])
        check(f"lambda{lam:g}/K{K}/dS", gs, dS, bounds[2])
    if K == 1:                                     # c = 1: the loss is the distance itself, whatever lambda
        soft_rows = ops.style_adherence_forward(dev(X), dev(S), lam, True)[0]
        hard_rows, amin = ops.style_adherence_forward(dev(X), dev(S), lam, False)
        assert np.array_equal(bits(soft_rows), bits(hard_rows)) and not amin.any()
        check("K1/L against d", soft_rows, R.distances(X, S)[..., 0], R.allowed(R.distances(X, S), R.distances(X, S, np.float32)))


@pytest.mark.parametrize("moves_last", [False, True], ids=["min_in_first_tile", "min_moves_in_last_tile"])
def test_adherence_far_rows(moves_last):
    """Every d >= 100 at lambda = 10: the naive sum exp(-lambda d) is 0.0 in fp32 and the soft minimum 0 / 0; the running
    minimum keeps it finite and right.  moves_last: the closest style frame is the clip's last, so every lane's running sums
    are rescaled in the last style tile."""
    B, T, K, F = 2, ROWS + 1, 2 * KT + 1, 53
    X, S = operands(B, T, K, F, False, 12.0)
    S = S.copy()
    S[:, K - 1 if moves_last else 3] += np.float32(1.0)               # one frame a little closer than the rest
    d = R.distances(X, S)
    assert d.min() >= 100.0 and float(np.exp(np.float32(-10.0) * d.astype(np.float32)).sum()) == 0.0
    assert (d.argmin(-1) == (K - 1 if moves_last else 3)).all()
    g = upstream(B, T, False)
    L64, L32 = R.adherence_rows(X, S, 10.0)[0], R.adherence_rows(X, S, 10.0, True, np.float32)[0]
    y, gx, gs = run_fn(X, S, 10.0, True, False, g)
    check("far/L", y, L64, R.allowed(L64, L32))
    assert torch.isfinite(gx).all() and torch.isfinite(gs).all() and float(gx.abs().max()) > 0 and float(gs.abs().max()) > 0
    dX, dS = R.adherence_grads(X, S, g, 10.0)
    d32 = R.adherence_grads(X, S, g, 10.0, True, np.float32)
    for name, got, want, r32 in (("far/dX", gx, dX, d32[0]), ("far/dS", gs, dS, d32[1])):      # measured, not asserted
        print(f"ERR {name} {R.worst(got.cpu().numpy(), want) / np.abs(want).max():.3e} {R.allowed(want, r32) / np.abs(want).max():.3e}")


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
def test_adherence_batch_independence_determinism_and_no_style_gradient(soft):
    B, T, K, F = 3, 2 * ROWS + 1, 2 * KT + 1, 67
    X, S = operands(B, T, K, F, not soft)
    g = upstream(B, T, False)
    y, gx, gs = run_fn(X, S, 10.0, soft, False, g)
    y2, gx2, gs2 = run_fn(X, S, 10.0, soft, False, g)
    for a, b in ((y, y2), (gx, gx2), (gs, gs2)):
        assert np.array_equal(bits(a), bits(b))                                      # the same bits twice
    for b in range(B):                                                               # each row of the batch alone
        y1, gx1, gs1 = run_fn(X[b:b + 1], S[b:b + 1], 10.0, soft, False, g[b:b + 1])
        assert np.array_equal(bits(y1), bits(y[b:b + 1])) and np.array_equal(bits(gx1), bits(gx[b:b + 1]))
        assert np.array_equal(bits(gs1), bits(gs[b:b + 1]))
    _, gx3, gs3 = run_fn(X, S, 10.0, soft, False, g, s_grad=False)
    assert gs3 is None and np.array_equal(bits(gx3), bits(gx))
    dx_only = ops.style_adherence_backward(dev(X), dev(S), *ops.style_adherence_forward(dev(X), dev(S), 10.0, soft), dev(g), 10.0,
                                           soft, need_dS=False)
    assert dx_only[1] is None and np.array_equal(bits(dx_only[0]), bits(gx))
    m1, m2 = ops.ordered_mean(y), ops.ordered_mean(y)
    assert np.array_equal(bits(m1), bits(m2)) and abs(float(m1) - float(y.double().mean())) <= 4 * np.spacing(np.float32(float(m1)))


# ------------------------------------------------------------------------------------------------ NT-Xent
def nt_operands(B, D, tiny_row=False):
    a, b = synth.normalish(f"ntx/a/{B}x{D}", (B, D)), synth.normalish(f"ntx/b/{B}x{D}", (B, D))
    if tiny_row:
        a = a.copy()
        a[B // 2] *= np.float32(1e-20) / np.float32(np.linalg.norm(a[B // 2].astype(np.float64)))
    return a, b


def run_nt(a, b, tau, up=1.0):
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    y = NtXentFn.apply(ta, tb, tau)
    y.backward(dev(np.float32(up)))
    return y.detach(), ta.grad, tb.grad


@pytest.mark.parametrize("tau", [0.07, 0.5])
@pytest.mark.parametrize("shape", NT_SHAPES, ids=lambda s: f"B{s[0]}_D{s[1]}")
def test_nt_xent_forward_and_gradient_against_float64(shape, tau):
    B, D = shape
    a, b = nt_operands(B, D)
    y, ga, gb = run_nt(a, b, tau, 1.3)
    y2, ga2, gb2 = run_nt(a, b, tau, 1.3)
    assert np.array_equal(bits(y), bits(y2)) and np.array_equal(bits(ga), bits(ga2)) and np.array_equal(bits(gb), bits(gb2))
    want, want32 = R.nt_xent(a, b, tau), R.nt_xent(a, b, tau, np.float32)
    d64, d32 = R.nt_xent_grads(a, b, tau, 1.3), R.nt_xent_grads(a, b, tau, 1.3, np.float32)
    assert y.shape == () and ga.shape == (B, D) and gb.shape == (B, D)
    check("ntx/loss", y, want, R.allowed(want, want32))
    check("ntx/da", ga, d64[0], R.allowed(d64[0], d32[0]))
    check("ntx/db", gb, d64[1], R.allowed(d64[1], d32[1]))
    if B == 1:                                             # one positive, no negative: loss 0 and no gradient
        assert float(y) == 0.0 and not ga.any() and not gb.any()


@pytest.mark.parametrize("shape", [(2, 3), (16, 64), (33, 300)], ids=lambda s: f"B{s[0]}_D{s[1]}")
def test_nt_xent_row_with_a_tiny_norm_is_clamped(shape):
    B, D = shape
    a, b = nt_operands(B, D, tiny_row=True)
    assert np.linalg.norm(a[B // 2].astype(np.float64)) < 1e-19
    y, ga, gb = run_nt(a, b, 0.5)
    want, want32 = R.nt_xent(a, b, 0.5), R.nt_xent(a, b, 0.5, np.float32)
    d64, d32 = R.nt_xent_grads(a, b, 0.5), R.nt_xent_grads(a, b, 0.5, 1.0, np.float32)
    check("ntx_tiny/loss", y, want, R.allowed(want, want32))
    check("ntx_tiny/da", ga, d64[0], R.allowed(d64[0], d32[0]))           # the clamped row's entries are the largest: ~ 1 / 1e-12
    check("ntx_tiny/db", gb, d64[1], R.allowed(d64[1], d32[1]))
    rest = np.arange(B) != B // 2                                         # and the other rows on their own scale
    check("ntx_tiny/da_rest", ga[torch.from_numpy(rest).to(DEV)], d64[0][rest], R.allowed(d64[0][rest], d32[0][rest]))


# ------------------------------------------------------------------------------------------------ the public surface
def test_public_classes_give_the_ops_bits_and_take_bf16():
    from msmd_amd.utils.common import StyleAdherenceLoss, nt_xent_loss
    B, T, K, F = 2, ROWS + 1, KT + 1, 53
    X, S = operands(B, T, K, F)
    x, s = dev(X).requires_grad_(True), dev(S).requires_grad_(True)
    loss = StyleAdherenceLoss()(x, s)
    loss.backward()
    L, stat = ops.style_adherence_forward(dev(X), dev(S), 10.0, True)
    dX, dS = ops.style_adherence_backward(dev(X), dev(S), L, stat, torch.ones((), device=DEV), 10.0, True, g_scale=1.0 / (B * T))
    assert np.array_equal(bits(loss), bits(ops.ordered_mean(L)))
    assert np.array_equal(bits(x.grad), bits(dX)) and np.array_equal(bits(s.grad), bits(dS))
    rows = StyleAdherenceLoss()(dev(X), dev(S), reduce=False)
    assert rows.shape == (B, T) and np.array_equal(bits(rows), bits(L))
    hard = StyleAdherenceLoss(use_soft_min=False)
    h_mean, h_rows = hard(dev(X), dev(S)), hard(dev(X), dev(S), reduce=False)        # the hard form ignores `reduce`
    assert h_mean.shape == h_rows.shape == () and np.array_equal(bits(h_mean), bits(h_rows))
    assert np.array_equal(bits(h_mean), bits(ops.ordered_mean(ops.style_adherence_forward(dev(X), dev(S), 10.0, False)[0])))
    # bf16 operands go through .float(): the value is the fp32 path's on the rounded operands, the gradients come back in bf16
    xb, sb = dev(X).bfloat16().requires_grad_(True), dev(S).bfloat16().requires_grad_(True)
    lb = StyleAdherenceLoss()(xb, sb)
    lb.backward()
    assert lb.dtype == torch.float32 and xb.grad.dtype == torch.bfloat16 and sb.grad.dtype == torch.bfloat16
    assert np.array_equal(bits(lb), bits(StyleAdherenceLoss()(xb.detach().float(), sb.detach().float())))
    a, b = nt_operands(16, 64)
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    y = nt_xent_loss(ta, tb, 0.07)
    y.backward()
    y0, _, saved = ops.nt_xent_forward(dev(a), dev(b), 0.07)
    grad = ops.nt_xent_backward(saved, torch.ones((), device=DEV), 0.07)
    assert np.array_equal(bits(y), bits(y0)) and np.array_equal(bits(ta.grad), bits(grad[:16]))
    assert np.array_equal(bits(tb.grad), bits(grad[16:]))
    ab, bb = dev(a).bfloat16().requires_grad_(True), dev(b).bfloat16().requires_grad_(True)
    yb = nt_xent_loss(ab, bb, 0.07)
    yb.backward()
    assert yb.dtype == torch.float32 and ab.grad.dtype == torch.bfloat16 and torch.isfinite(ab.grad.float()).all()
    assert np.array_equal(bits(yb), bits(nt_xent_loss(ab.detach().float(), bb.detach().float(), 0.07)))


def test_style_adherence_flag_of_the_inference_script(tmp_path, monkeypatch, capsys):
    """--style_adherence on a tiny synthetic model: one more file per seed, (T,) float32, equal to the ops result on the
    tensors main() itself held (the generated coefficients and the WHOLE normalised style clip)."""
    from msmd_amd import inference
    from msmd_amd.config import default_args
    from msmd_amd.model import DiffusionSchedule, get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    args = default_args(compute_dtype="fp32", encoder_layers=2, n_layers=2)
    model = get_diffusion_model(args, DEV).eval()
    model.diffusion_sched = DiffusionSchedule(2, "cosine").to(DEV)
    style_enc = get_style_encoder(args, "vae2").to(DEV).eval()
    monkeypatch.setattr(inference, "load_model", lambda *a: (model, style_enc, args))
    held = {}
    real_infer, real_query = inference.infer_coeffs, inference.query_for_motion_coeff

    def keep_coef(*a, **k):
        held["coef"] = real_infer(*a, **k)
        return held["coef"]

    def keep_style(*a, **k):
        held["style"], shape = real_query(*a, **k)
        return held["style"], shape
    monkeypatch.setattr(inference, "infer_coeffs", keep_coef)
    monkeypatch.setattr(inference, "query_for_motion_coeff", keep_style)
    C, K = model.motion_feat_dim, 150
    stats = {"exp_mean": torch.zeros(C - 3), "exp_std": torch.ones(C - 3), "pose_mean": torch.zeros(3), "pose_std": torch.ones(3)}
    files = {"stats": stats, "exp": torch.from_numpy(synth.normalish("sa/exp", (K, C - 3))),
             "rot": synth.normalish("sa/rot", (K, 3)).astype(np.float64)}
    for name, obj in files.items():
        with open(tmp_path / f"{name}.pkl", "wb") as f:
            pickle.dump(obj, f)
    np.save(tmp_path / "speech.npy", synth.audio_clips(1, 40000, tag="sa")[0])
    argv = ["--model_root", str(tmp_path), "--model_name", "tiny", "--model_iter", "1", "--style_clip_exp_code_path",
            str(tmp_path / "exp.pkl"), "--style_clip_head_rot_path", str(tmp_path / "rot.pkl"), "--audio_clip",
            str(tmp_path / "speech.npy"), "--coef_dict_path", str(tmp_path / "stats.pkl"), "--output_dir", str(tmp_path / "out")]
    assert inference.parse_args(argv).style_adherence is False
    out = inference.main(argv + ["--style_adherence"])
    assert len(out) == 3 and out[2].endswith("_seed_0.npy") and "style_adherence_" in out[2]
    got = np.load(out[2])
    T = int(40000 / 16000 * args.fps)
    assert got.shape == (T,) and got.dtype == np.float32 and np.isfinite(got).all() and (got > 0).all()
    assert held["style"].shape == (1, 125, C) and held["coef"].shape == (1, T, C)          # 150 frames at 30 fps -> 125 at 25
    want = ops.style_adherence_forward(held["coef"][0:1].float().contiguous(), held["style"].contiguous(), 10.0, True)[0][0]
    assert np.array_equal(got.view(np.uint32), bits(want))
    printed = re.search(r"style adherence \(seed 0\): mean ([0-9.]+) over (\d+) frames", capsys.readouterr().out)
    assert printed and int(printed.group(2)) == T and abs(float(printed.group(1)) - float(got.mean(dtype=np.float64))) <= 2e-6 * got.max()


# ------------------------------------------------------------------------------------------------ the raw entry points
def guarded(n, dtype=torch.float32):
    t = torch.full((n + GUARD,), MARK, device=DEV, dtype=dtype)
    t[:n] = float("nan") if dtype.is_floating_point else -1
    return t


def intact(t, n):
    body = t[:n]
    written = not (torch.isnan(body).any() if t.dtype.is_floating_point else (body == -1).any())
    return bool((t[n:] == MARK).all()) and bool(written)


@pytest.mark.parametrize("soft", [1, 0], ids=["soft", "hard"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, ROWS + 1, KT + 1, 67), (3, 2 * ROWS - 1, 2 * KT - 1, 130)],
                         ids=lambda s: "x".join(map(str, s)))
def test_adherence_entry_points_write_exactly_their_buffers(shape, soft):
    B, T, K, F = shape
    X, S = operands(B, T, K, F, not soft)
    x, s, g = dev(X), dev(S), dev(upstream(B, T, False))
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    n_stat = B * T * (2 if soft else 1)
    L, stat = guarded(B * T), guarded(n_stat, torch.float32 if soft else torch.int32)
    assert lib.msmd_style_adherence_forward(x.data_ptr(), s.data_ptr(), L.data_ptr(), stat.data_ptr(), B, T, K, F, 10.0, soft, st) == 0
    torch.cuda.synchronize()
    assert intact(L, B * T) and intact(stat, n_stat)
    dX, dS = guarded(B * T * F), guarded(B * K * F)
    assert lib.msmd_style_adherence_backward(x.data_ptr(), s.data_ptr(), L.data_ptr(), stat.data_ptr(), g.data_ptr(), 1, 1.0,
                                             dX.data_ptr(), dS.data_ptr(), B, T, K, F, 10.0, soft, st) == 0
    torch.cuda.synchronize()
    assert intact(dX, B * T * F) and intact(dS, B * K * F)
    want = truth(B, T, K, F, 10.0, bool(soft), False, not soft)
    check("abi/L", L[:B * T].view(B, T), want[0][0], want[1][0])
    check("abi/dX", dX[:B * T * F].view(B, T, F), want[0][1], want[1][1])
    check("abi/dS", dS[:B * K * F].view(B, K, F), want[0][2], want[1][2])
    mean = guarded(1)
    assert lib.msmd_ordered_mean(L.data_ptr(), B * T, mean.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert intact(mean, 1) and abs(float(mean[0]) - float(L[:B * T].double().mean())) <= 4 * np.spacing(np.float32(float(mean[0])))
    # refused before any launch: nothing is written
    L2 = guarded(B * T)
    for bad in ((0, T, K, F, 10.0), (B, 0, K, F, 10.0), (B, T, 0, F, 10.0), (B, T, K, 0, 10.0), (B, T, K, F, -1.0)):
        assert lib.msmd_style_adherence_forward(x.data_ptr(), s.data_ptr(), L2.data_ptr(), stat.data_ptr(), *bad, soft, st) == 1
    torch.cuda.synchronize()
    assert torch.isnan(L2[:B * T]).all()


@pytest.mark.parametrize("shape", [(1, 1), (2, 67), (33, 300), (130, 5)], ids=lambda s: f"B{s[0]}_D{s[1]}")
def test_nt_xent_entry_points_write_exactly_their_buffers(shape):
    B, D = shape
    N = 2 * B
    a, b = (dev(v) for v in nt_operands(B, D))
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    fhat, norm, rows, lse = guarded(N * D), guarded(N), guarded(N), guarded(2 * N)
    assert lib.msmd_nt_xent_forward(a.data_ptr(), b.data_ptr(), fhat.data_ptr(), norm.data_ptr(), rows.data_ptr(), lse.data_ptr(),
                                    B, D, 0.5, st) == 0
    torch.cuda.synchronize()
    assert intact(fhat, N * D) and intact(norm, N) and intact(rows, N) and intact(lse, 2 * N)
    up, grad = torch.ones(1, device=DEV), guarded(N * D)
    assert lib.msmd_nt_xent_backward(fhat.data_ptr(), norm.data_ptr(), lse.data_ptr(), up.data_ptr(), grad.data_ptr(), B, D, 0.5,
                                     st) == 0
    torch.cuda.synchronize()
    assert intact(grad, N * D)
    d64, d32 = R.nt_xent_grads(*nt_operands(B, D), 0.5), R.nt_xent_grads(*nt_operands(B, D), 0.5, 1.0, np.float32)
    want, r32 = np.concatenate(d64), np.concatenate(d32)
    check("abi/ntx_grad", grad[:N * D].view(N, D), want, R.allowed(want, r32))
    for bad in ((0, D, 0.5), (B, 0, 0.5), (B, D, 0.0), (B, D, -0.5)):
        assert lib.msmd_nt_xent_forward(a.data_ptr(), b.data_ptr(), fhat.data_ptr(), norm.data_ptr(), rows.data_ptr(),
                                        lse.data_ptr(), *bad, st) == 1
