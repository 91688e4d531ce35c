"""Retargeting on the MI355X: csrc/retarget.hip through ops.retarget_* / ops.blendshape_apply / utils.retarget against the float64
restatement (tests/retarget_ref.py; tests/test_retarget_cpu.py pins it against scipy's BVLS on every case used here).

Bounds, all from the number formats (u32 = 2^-24, u64 = 2^-53):
  rhs     |b - b64| <= gamma_{n+1}(u32) sum |A d|, n = 3 V: any order of an n-term fp32 sum of fp32 products;
  gram    |G - G_exact| <= gamma_n(u64) sum |a_k a_l| (the products of two fp32 are exact in float64), G_exact in 80-bit arithmetic;
  solve   |w - w_ref| <= u32 max(1, |w_ref|) + 8 K u64 cond_2(H) max(1, |w_ref|_inf): one rounding to fp32 plus the CPU bound;
  whole   the solve bound plus |H^-1|_inf (max_k rhs bound + u32 |b64|_inf): the reference rounds its b to fp32 too;
  apply   |out - out64| <= (K + 2) u32 (|neutral| + sum |w_k delta_k|): K fused multiply-adds.
Every figure is printed before it is asserted."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import retarget_ref as R
from msmd_amd import _lib, ops, synth
from msmd_amd.utils import media, metrics
from msmd_amd.utils import retarget as RT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FT, VT, SV = ops.RETARGET_FRAME_TILE, ops.RETARGET_VERTEX_TILE, ops.RETARGET_SPLIT_VERTICES


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dt is None else t.to(dt)).to(DEV)


def random_problem(V, K, N, seed, zero_every=0):
    """A rig and N frames around its neutral -> (rig dict, prep, x fp32)."""
    rig = R._rig(V, K, seed, zero_weight_every=zero_every)
    p = R.prepare(rig)
    x = rig["neutral"][None] + 0.02 * synth.normalish(f"gpu/x/{V}/{K}/{N}/{seed}", (N, V, 3)).astype(np.float32)
    return rig, p, x.astype(np.float32)


def gpu_rhs(p, x, with_weights=True):
    vw = dev(p["vw"]) if with_weights and "vw" in p else None
    b = ops.retarget_rhs(dev(x), dev(p["neutral"]), dev(p["A"]), vw)
    torch.cuda.synchronize()
    return b.cpu().numpy()


def check_rhs(p, x, label):
    b = gpu_rhs(p, x)
    b64, absum = R.rhs(p, x)
    bound = R.rhs_bound(absum, 3 * p["V"])
    err = np.abs(b.astype(np.float64) - b64)
    assert b.shape == b64.shape and b.dtype == np.float32
    if b.size:
        print(f"rhs {label}: err {err.max():.3e}, worst err / bound {np.max(err / np.maximum(bound, 1e-300)):.4f}")
    assert (err <= bound).all()
    return b


def with_weights(rig, p):
    if rig.get("vertex_weight") is not None:
        p = dict(p, vw=np.asarray(rig["vertex_weight"], np.float32))
    return p


@pytest.mark.parametrize("V", [1, VT - 1, VT, VT + 1, SV - 1, SV, SV + 1])
def test_rhs_at_the_vertex_tile_and_the_split(V):
    rig, p, x = random_problem(V, 7, 5, 11, zero_every=4 if V > 4 else 0)
    check_rhs(with_weights(rig, p), x, f"V {V}")


@pytest.mark.parametrize("K", [1, 7, 52, 64])
def test_rhs_shape_counts(K):
    rig, p, x = random_problem(VT + 1, K, 5, 12)
    check_rhs(p, x, f"K {K}")


@pytest.mark.parametrize("N", [0, 1, FT - 1, FT, FT + 1])
def test_rhs_frame_counts(N):
    rig, p, x = random_problem(97, 7, N, 13, zero_every=3)
    b = check_rhs(with_weights(rig, p), x, f"N {N}")
    assert b.shape == (N, 7)


def test_rhs_at_flame_size():
    rig, p, x = random_problem(5023, 52, FT + 1, 14)
    assert ops.retarget_rhs(dev(x[:0]), dev(p["neutral"]), dev(p["A"])).shape == (0, 52)
    check_rhs(p, x, "V 5023, K 52")


def test_rhs_and_apply_leave_guard_elements_alone():
    """The entry points called on buffers with 64 extra elements behind every output and workspace."""
    rig, p, x = random_problem(SV + 1, 7, FT + 1, 15)
    N, K, V = x.shape[0], 7, SV + 1
    S = _lib.load().msmd_retarget_splits(V)
    assert S == 2
    part = torch.full((S * N * K + 64,), 7.5, device=DEV)
    b = torch.full((N * K + 64,), -3.25, device=DEV)
    xs, nt, A = dev(x), dev(p["neutral"]), dev(p["A"])
    assert _lib.load().msmd_retarget_rhs(ops._p(xs), ops._p(nt), ops._p(A), None, ops._p(part), ops._p(b), N, V, K, ops._stream()) == 0
    torch.cuda.synchronize()
    assert (part[S * N * K:] == 7.5).all() and (b[N * K:] == -3.25).all()
    assert np.array_equal(b[:N * K].cpu().numpy().reshape(N, K), gpu_rhs(p, x))
    w = torch.rand(N, K, device=DEV)
    out = torch.full((N * V * 3 + 64,), 9.0, device=DEV)
    d = dev(rig["deltas"])
    assert _lib.load().msmd_blendshape_apply(ops._p(w), ops._p(nt), ops._p(d), ops._p(out), N, V, K, ops._stream()) == 0
    torch.cuda.synchronize()
    assert (out[N * V * 3:] == 9.0).all()
    assert torch.equal(out[:N * V * 3].view(N, V, 3), ops.blendshape_apply(w, nt, d))
    ws, st, it = (torch.full((N * K + 64,), 5.0, device=DEV), torch.full((N + 64,), 77, device=DEV, dtype=torch.int32),
                  torch.full((N + 64,), 78, device=DEV, dtype=torch.int32))
    H = dev(p["H"])
    assert _lib.load().msmd_retarget_solve(ops._p(H), ops._p(b), None, None, ops._p(ws), ops._p(st), ops._p(it), N, K, 256, ops._stream()) == 0
    torch.cuda.synchronize()
    assert (ws[N * K:] == 5.0).all() and (st[N:] == 77).all() and (it[N:] == 78).all() and (st[:N] == 0).all()


def test_nan_in_a_weightless_vertex_is_never_read_and_elsewhere_marks_its_frame():
    c = R.case("K7-V97-noisy")
    rig = RT.prepare_rig(c["rig"], DEV)
    x = dev(c["x"])
    b0 = ops.retarget_rhs(x, rig.neutral, rig.A, rig.vertex_weight)
    w0, s0 = RT.retarget(x, rig)
    unused, used = np.nonzero(~c["prep"]["used"])[0], np.nonzero(c["prep"]["used"])[0]
    xn = x.clone()
    xn[:, unused] = float("nan")
    assert torch.equal(ops.retarget_rhs(xn, rig.neutral, rig.A, rig.vertex_weight), b0)
    w1, s1 = RT.retarget(xn, rig)
    assert torch.equal(w1, w0) and torch.equal(s1, s0) and not s0.any()
    xu = x.clone()
    xu[2, int(used[5]), 1] = float("nan")
    bu = ops.retarget_rhs(xu, rig.neutral, rig.A, rig.vertex_weight)
    assert torch.isnan(bu[2]).any() and torch.equal(bu[[0, 1, 3, 4, 5]], b0[[0, 1, 3, 4, 5]])
    w2, s2, it2 = RT.retarget(xu, rig, return_iterations=True)
    assert s2.tolist() == [0, 0, ops.RETARGET_BAD_INPUT, 0, 0, 0] and torch.isnan(w2[2]).all() and it2[2] == 0
    assert torch.equal(w2[[0, 1, 3, 4, 5]], w0[[0, 1, 3, 4, 5]])


def test_a_frame_does_not_depend_on_its_batch():
    """b, w and status of a frame: alone, among 69 others at two places, in two chunkings and in two runs: the same bits."""
    c = R.case("K52-V700-noisy")
    rig = RT.prepare_rig(c["rig"], DEV)
    g = synth.uniform01("gpu/batch/w", 70 * 52).reshape(70, 52) * 1.4 - 0.3
    x70 = R.apply(c["rig"], g)[0] + 2e-4 * synth.normalish("gpu/batch/noise", (70, 700, 3))
    x70 = dev(x70.astype(np.float32))
    rhs = lambda x: ops.retarget_rhs(x, rig.neutral, rig.A, rig.vertex_weight)
    b70 = rhs(x70)
    w70, s70, i70 = RT.retarget(x70, rig, chunk=70, return_iterations=True)
    for f in (0, 37, 69):
        assert torch.equal(rhs(x70[f:f + 1].contiguous())[0], b70[f])
        w1, s1 = RT.retarget(x70[f:f + 1].contiguous(), rig)
        assert torch.equal(w1[0], w70[f]) and s1[0] == s70[f]
    moved = torch.cat([x70[37:], x70[:37]]).contiguous()
    assert torch.equal(rhs(moved)[0], b70[37]) and torch.equal(rhs(moved)[-1], b70[36])
    w17, s17, i17 = RT.retarget(x70, rig, chunk=17, return_iterations=True)
    assert torch.equal(w17, w70) and torch.equal(s17, s70) and torch.equal(i17, i70)
    again = RT.retarget(x70, rig, chunk=70)
    assert torch.equal(again[0], w70) and torch.equal(again[1], s70) and torch.equal(rhs(x70), b70)
    assert not s70.any() and int(i70.max()) < R.CAP
    print(f"70 frames of K 52: iterations {int(i70.min())} .. {int(i70.max())}")


@pytest.mark.parametrize("name", ["K7-V97-noisy", "K52-V700-noisy", "K64-V15-ridge"])
def test_gram_against_extended_precision(name):
    c = R.case(name)
    p = c["prep"]
    ridge = c["rig"].get("ridge")
    G, H = ops.retarget_gram(dev(p["A"]), ridge)
    torch.cuda.synchronize()
    G, H = G.cpu().numpy(), H.cpu().numpy()
    A = p["A"].reshape(p["K"], -1).astype(np.longdouble)
    exact, mag = A @ A.T, np.abs(A) @ np.abs(A).T
    n = A.shape[1]
    bound = (n * R.U64 / (1 - n * R.U64)) * mag.astype(np.float64) + 2.0 ** -63 * mag.astype(np.float64)
    err = np.abs(G.astype(np.longdouble) - exact).astype(np.float64)
    print(f"gram {name}: err {err.max():.3e}, worst err / bound {np.max(err / bound):.4f}")
    assert (err <= bound).all() and np.array_equal(G, G.T)
    want = G + np.diag(np.zeros(p["K"]) if ridge is None else ridge)
    assert np.array_equal(H, want)
    assert np.abs(H - p["H"]).max() <= 2 * bound.max()


def gpu_solve(H, b, lo, hi, cap=ops.RETARGET_ITERATIONS):
    out = ops.retarget_solve(dev(H), dev(b, torch.float32), lo, hi, cap)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", list(R.CASES) + ["backup"])
def test_solve_alone_on_given_h_and_b(name):
    if name == "backup":
        H, b, lo, hi = R.backup_case()
        w_ref, st_ref, it_ref = R.solve(H, b, lo, hi)
    else:
        c = R.case(name)
        H, b, lo, hi, w_ref, st_ref, it_ref = c["prep"]["H"], c["b32"], c["prep"]["lo"], c["prep"]["hi"], c["w"], c["status"], c["iterations"]
    w, st, it = gpu_solve(H, b, lo, hi)
    assert w.dtype == np.float32 and st.dtype == np.int32 and it.dtype == np.int32 and w.shape == w_ref.shape
    bound = R.U32 * np.maximum(1.0, np.abs(w_ref)) + R.solve_bound(H, w_ref)
    err = np.abs(w.astype(np.float64) - w_ref)
    print(f"solve {name}: err {err.max():.3e}, worst err / bound {np.max(err / bound):.4f}; iterations {it.tolist()} (restatement {it_ref.tolist()})")
    assert not st.any() and (it < R.CAP).all() and (it >= 1).all()
    assert (err <= bound).all()
    assert (w >= lo.astype(np.float32)).all() and (w <= hi.astype(np.float32)).all()


def test_solve_statuses():
    H, b, lo, hi = R.backup_case()
    assert R.solve(H, b, lo, hi)[2][0] > 1
    w, st, it = gpu_solve(H, b, lo, hi, cap=1)
    assert st.tolist() == [ops.RETARGET_CAP_REACHED] and it.tolist() == [1] and (w >= 0).all() and (w <= 1).all()
    w4, st4, it4 = gpu_solve(H, b, lo, hi, cap=4)
    assert st4.tolist() == [ops.RETARGET_CAP_REACHED] and it4.tolist() == [4] and (w4 >= 0).all() and (w4 <= 1).all()
    ref4 = R.solve(H, b, lo, hi, cap=4)[0]
    assert np.abs(w4 - ref4).max() <= R.U32 + R.solve_bound(H, ref4)
    bb = np.repeat(b, 3, 0)
    bb[1, 4] = np.inf
    w, st, it = gpu_solve(H, bb, lo, hi)
    assert st.tolist() == [0, ops.RETARGET_BAD_INPUT, 0] and np.isnan(w[1]).all() and it[1] == 0 and np.array_equal(w[0], w[2])
    w, st, it = gpu_solve(np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[1.0, 1.0]]), None, None)
    assert st.tolist() == [ops.RETARGET_NOT_POSITIVE] and np.isnan(w).all()     # indefinite: both weights go free, the second pivot is -3
    with pytest.raises(ValueError, match="lo < hi"):
        ops.retarget_solve(dev(H), dev(b), np.zeros(6), np.zeros(6))
    with pytest.raises(ValueError, match="max_iterations"):
        ops.retarget_solve(dev(H), dev(b), None, None, 0)
    with pytest.raises(ValueError, match="ridge"):
        ops.retarget_gram(torch.zeros(2, 5, 3, device=DEV), [-1.0, 0.0])
    with pytest.raises(ValueError, match="65 blendshapes"):
        ops.retarget_gram(torch.zeros(65, 5, 3, device=DEV))


@pytest.mark.parametrize("name", list(R.CASES))
def test_end_to_end_against_the_restatement(name):
    c = R.case(name)
    p = c["prep"]
    rig = RT.prepare_rig(c["rig"], DEV)
    w, st, it = RT.retarget(dev(c["x"]), rig, return_iterations=True)
    torch.cuda.synchronize()
    w, st = w.cpu().numpy().astype(np.float64), st.cpu().numpy()
    Hinv = np.abs(np.linalg.inv(p["H"])).sum(1).max()
    db = R.rhs_bound(c["absum"], 3 * p["V"]).max(1) + R.U32 * np.abs(c["b64"]).max(1)
    bound = R.U32 * np.maximum(1.0, np.abs(c["w"])) + R.solve_bound(p["H"], c["w"]) + (Hinv * db)[:, None]
    err = np.abs(w - c["w"])
    print(f"whole {name}: err {err.max():.3e}, worst err / bound {np.max(err / bound):.4f}, |H^-1| {Hinv:.3e}; iterations {it.tolist()}")
    assert not st.any()
    assert (err <= bound).all()


def test_planted_weights_come_back_through_apply_and_retarget():
    """x = rig_vertices(w*) on the device, w* in the box with exact 0 and 1 -> w* again, within the bound of the whole pipeline
    plus what the fp32 mesh itself is off by, (K + 2) u32 terms + u32 |d| per coordinate, carried through |A| and |H^-1|."""
    c = R.case("K52-V700-planted")
    p, K = c["prep"], 52
    rig = RT.prepare_rig(c["rig"], DEV)
    w_star = c["w_star"].astype(np.float32)
    assert (w_star[0, ::2] == 0).all() and (w_star[0, 1::2] == 1).all()
    x = RT.rig_vertices(dev(w_star), rig)
    out64, terms = R.apply(c["rig"], w_star)
    xa = x.cpu().numpy()
    assert (np.abs(xa - out64) <= (K + 2) * R.U32 * terms).all()
    w, st = RT.retarget(x, rig)
    w = w.cpu().numpy().astype(np.float64)
    b64, absum = R.rhs(p, xa)
    d = np.abs(xa.astype(np.float64) - p["neutral"][None])
    mesh = ((K + 2) * R.U32 * terms + R.U32 * d).reshape(len(w), -1) @ np.abs(p["A"].reshape(K, -1).astype(np.float64)).T
    Hinv = np.abs(np.linalg.inv(p["H"])).sum(1).max()
    db = (R.rhs_bound(absum, 3 * p["V"]) + mesh).max(1) + R.U32 * np.abs(b64).max(1)
    bound = R.U32 + R.solve_bound(p["H"], w_star) + Hinv * db
    err = np.abs(w - w_star).max(1)
    print(f"planted: |w - w*| = {err.max():.3e}, worst err / bound {np.max(err / bound):.4f}")
    assert not st.any() and (err <= bound).all()


@pytest.mark.parametrize("shape", [(1, 1, 1), (SV + 1, 7, 17), (97, 64, 16), (33, 52, 15)])
def test_blendshape_apply(shape):
    V, K, N = shape
    rig = synth.blendshape_rig(V, K, 21)
    w = (synth.uniform01(f"gpu/apply/{shape}", N * K).reshape(N, K) * 1.5 - 0.25).astype(np.float32)
    out = ops.blendshape_apply(dev(w), dev(rig["neutral"]), dev(rig["deltas"]))
    torch.cuda.synchronize()
    out64, terms = R.apply(rig, w)
    err, bound = np.abs(out.cpu().numpy() - out64), (K + 2) * R.U32 * terms
    print(f"apply {shape}: err {err.max():.3e}, worst err / bound {np.max(err / bound):.4f}")
    assert out.shape == (N, V, 3) and (err <= bound).all()
    assert ops.blendshape_apply(dev(w[:0]), dev(rig["neutral"]), dev(rig["deltas"])).shape == (0, V, 3)


def test_prepare_rig_refuses_a_singular_rig():
    c = R.case("K64-V15-ridge")
    RT.prepare_rig(c["rig"], DEV)
    bare = {k: v for k, v in c["rig"].items() if k != "ridge"}
    with pytest.raises(ValueError, match="ridge"):
        RT.prepare_rig(bare, DEV)


def test_flame_to_curves_to_video(tmp_path):
    """FLAME.forward on the synthetic asset -> retarget_coeffs -> report, CSV and the comparison video."""
    from msmd_amd.utils.flame import FLAME, FLAMEConfig
    from msmd_amd.utils.renderer import MeshRenderer
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = synth.flame_asset()
    fl = FLAME(cfg).to(DEV)
    T, K, S = 7, 12, 48
    cd = dict(shape=torch.zeros(T, 100, device=DEV), exp=dev(0.5 * synth.normalish("gpu/flame/exp", (T, 50))),
              pose=dev(0.05 * synth.normalish("gpu/flame/pose", (T, 6))))
    neutral = fl(cd["shape"][:1], torch.zeros(1, 50, device=DEV), torch.zeros(1, 6, device=DEV), return_lm2d=False, return_lm3d=False)[0][0]
    rig = RT.prepare_rig(synth.blendshape_rig(5023, K, 31, neutral=neutral.cpu().numpy()), DEV)
    seen = []
    w, st = RT.retarget_coeffs(cd, fl, rig, chunk=3, on_chunk=lambda v, ww, i: seen.append((i, v.shape[0])))
    assert seen == [(0, 3), (3, 3), (6, 1)] and w.shape == (T, K) and not st.any()
    verts = fl(cd["shape"], cd["exp"], cd["pose"], return_lm2d=False, return_lm3d=False)[0].float().contiguous()
    w_all, _ = RT.retarget(verts, rig)
    assert torch.equal(w_all, w)                                     # the chunks of the FLAME pass change nothing
    rep = RT.retarget_report(verts, w, rig, chunk=4)
    recon = RT.rig_vertices(w, rig)
    vm = metrics.vertex_metrics(recon, verts, [0, T], [0], [0], rig.neutral)["all"]
    rest = metrics.vertex_metrics(rig.neutral[None].expand(T, -1, -1).contiguous(), verts, [0, T], [0], [0], rig.neutral)["all"]
    print(f"report {rep}; the neutral alone is off by rms {rest['rmse']:.3e}")
    assert rep == dict(mean=vm["mve"], max=vm["max_ve"], rms=vm["rmse"], frames=T)
    assert rep["rms"] < rest["rmse"]                                 # the fit explains some of the motion
    RT.write_curves(tmp_path / "c.csv", w, rig.names, 25)
    names, back, _ = RT.read_curves(tmp_path / "c.csv")
    assert names == rig.names and np.array_equal(back, w.cpu().numpy())
    faces = dev(cfg.asset["f"].astype(np.int64))
    frames = RT.comparison_frames(verts, w, rig, getattr(fl, "faces_tensor", faces), MeshRenderer((S, S)), rep["max"])
    assert tuple(frames.shape) == (T, S, 3 * S, 3)
    media.write_avi(tmp_path / "c.avi", media.encode_jpeg(frames.contiguous(), 90), 25, (3 * S, S))
    clip = media.read_avi(tmp_path / "c.avi")
    assert len(clip.frames) == T and tuple(clip.size) == (3 * S, S)


def test_inference_writes_curves_and_the_comparison_video(tmp_path):
    """inference.write_retarget, what `inference.py --retarget RIG.npz [--comparison_video]` calls per repetition."""
    from msmd_amd import inference
    from msmd_amd.utils.flame import FLAME, FLAMEConfig
    from msmd_amd.utils.renderer import MeshRenderer
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = synth.flame_asset()
    fl = FLAME(cfg).to(DEV)
    T, S = 5, 40
    zero = torch.zeros(1, 100, device=DEV)
    neutral = fl(zero, torch.zeros(1, 50, device=DEV), torch.zeros(1, 6, device=DEV), return_lm2d=False, return_lm3d=False)[0][0]
    rig = RT.Rig(**synth.blendshape_rig(5023, 9, 32, neutral=neutral.cpu().numpy()))
    rig.save(tmp_path / "rig.npz")
    coef = dev(np.concatenate([0.5 * synth.normalish("gpu/inf/exp", (T, 50)), 0.2 * synth.normalish("gpu/inf/rot", (T, 3))], 1).astype(np.float32))
    rep = inference.write_retarget(coef, zero, fl, RT.load_rig(tmp_path / "rig.npz"), 25, tmp_path / "r.csv", tmp_path / "r.avi",
                                   MeshRenderer((S, S)), chunk=2)
    names, w, _ = RT.read_curves(tmp_path / "r.csv")
    assert names == rig.names and w.shape == (T, 9) and (w >= 0).all() and (w <= 1).all()
    assert rep["frames"] == T and rep["flagged"] == 0 and 0 < rep["rms"] <= rep["max"]
    clip = media.read_avi(tmp_path / "r.avi")
    assert len(clip.frames) == T and tuple(clip.size) == (3 * S, S)
    a = inference.parse_args
    base = ["--model_root", "m", "--model_name", "n", "--model_iter", "1", "--style_clip_exp_code_path", "e", "--style_clip_head_rot_path",
            "h", "--audio_clip", "a.wav"]
    for bad in (["--retarget", "rig.npz"], ["--comparison_video"], ["--retarget", "rig.npz", "--flame_model_path", "f", "--comparison_video"]):
        with pytest.raises(SystemExit):
            a(base + bad)
    ok = a(base + ["--retarget", "rig.npz", "--flame_model_path", "f", "--comparison_video", "--render_size", "64"])
    assert ok.retarget == "rig.npz" and ok.comparison_video
