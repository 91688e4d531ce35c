"""Geometry kernels (csrc/flame.hip, csrc/lbs_skin.hip, csrc/rotations.hip) against float64 restatements written here from the formulas, at the
shapes where these kernels go wrong: vertex counts around the 64 / 128-vertex tiles and the fp16 lane pairs (odd and even V),
frame counts around the 16-frame tile, every coefficient width the 192-wide K row admits, item counts around the 256-item
workgroup of the rotation kernel and unaligned input views.  Every output element is compared; each tolerance is a stated
error bound (u = 2^-24, the fp32 unit roundoff) or bit equality.  The reference repository's utils/lbs.py, utils/flame.py and
utils/rotation_conversions.py define the operations (PyTorch3D / SMPL-X conventions)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from msmd_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
KP = 192
J = 5


def ops():
    from msmd_amd import ops as _ops
    return _ops


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def rng(tag):
    return np.random.default_rng(synth.name_seed(tag) & 0xFFFFFFFF)


# ----------------------------------------------------------------------------- float64 building blocks
def rodrigues64(r):
    """(N, 3) -> (N, 3, 3): utils/lbs.py's batch_rodrigues, angle = ||r + 1e-8||, direction = r / angle (un-shifted r)."""
    r = np.asarray(r, np.float64)
    angle = np.sqrt(((r + 1e-8) ** 2).sum(1, keepdims=True))
    d = r / angle
    s, c1 = np.sin(angle)[:, :, None], (1.0 - np.cos(angle))[:, :, None]
    z = np.zeros(len(r))
    K = np.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
    return np.eye(3)[None] + s * K + c1 * (K @ K)


@functools.lru_cache(maxsize=16)
def asset(V):
    """synth.flame_asset()'s recipe and scales at any vertex count (400 shape directions, 36 pose directions, 5 joints)."""
    tag = f"geom_asset/{V}"
    vt = (0.1 * synth.uniform(tag + "/v_template", (V, 3))).astype(np.float32)
    sd = (0.01 * synth.uniform(tag + "/shapedirs", (V, 3, 400))).astype(np.float32)
    pd = (0.01 * synth.uniform(tag + "/posedirs", (V, 3, 36))).astype(np.float32)
    jr = np.zeros((J, V), np.float64)
    w = synth.uniform01(tag + "/J_regressor", J * 64).reshape(J, 64)
    for j in range(J):
        np.add.at(jr[j], (np.arange(64) * 71 + j * 997) % V, w[j] / w[j].sum())   # a window of vertices (repeats add up)
    wts = synth.uniform01(tag + "/weights", V * J).reshape(V, J).astype(np.float32) ** 4
    wts = (wts / wts.sum(1, keepdims=True)).astype(np.float32)
    return dict(v_template=vt, shapedirs=sd, posedirs=pd, J_regressor=jr.astype(np.float32), weights=wts,
                parents=np.array([-1, 0, 1, 1, 1]))


def model(V, NB):
    """(float32 arrays as the kernels get them, LbsConstants) for the first NB shape directions of asset(V)."""
    from msmd_amd.utils.lbs import LbsConstants
    a = asset(V)
    m = dict(v_template=a["v_template"], shapedirs=np.ascontiguousarray(a["shapedirs"][:, :, :NB]),
             posedirs=np.ascontiguousarray(a["posedirs"].reshape(V * 3, 36).T), J_regressor=a["J_regressor"],
             weights=a["weights"], parents=a["parents"])
    t = {k: dev(v) for k, v in m.items()}
    c = LbsConstants(t["v_template"], t["shapedirs"], t["posedirs"], t["J_regressor"], t["parents"], t["weights"])
    return m, t, c


def lbs64(m, betas, pose, pose_is_matrix=False):
    """utils/lbs.py:141-223 in float64: v = sum_j w_j (R_j p + t_j), p = template + sum_k coef_k dirs_k with the
    coefficients [betas | R[1:] - I].  -> (verts (B, V, 3), p (B, V, 3), A (B, J, 3, 4), coef (B, NB + 36))."""
    f = lambda x: np.asarray(x, np.float64)
    betas = f(betas)
    B, NB = betas.shape
    V = m["v_template"].shape[0]
    sd, pd = f(m["shapedirs"]), f(m["posedirs"])
    v_shaped = f(m["v_template"])[None] + (betas @ sd.reshape(V * 3, NB).T).reshape(B, V, 3)
    joints = np.einsum("jv,bvc->bjc", f(m["J_regressor"]), v_shaped)
    R = f(pose).reshape(B, J, 3, 3) if pose_is_matrix else rodrigues64(f(pose).reshape(B * J, 3)).reshape(B, J, 3, 3)
    pf = (R[:, 1:] - np.eye(3)).reshape(B, (J - 1) * 9)
    p = v_shaped + (pf @ pd).reshape(B, V, 3)
    par = m["parents"]
    wR, wt = [R[:, 0]], [joints[:, 0]]
    for i in range(1, J):
        wR.append(wR[par[i]] @ R[:, i])
        wt.append(np.einsum("brc,bc->br", wR[par[i]], joints[:, i] - joints[:, par[i]]) + wt[par[i]])
    A = np.stack([np.concatenate([wR[i], (wt[i] - np.einsum("brc,bc->br", wR[i], joints[:, i]))[:, :, None]], 2)
                  for i in range(J)], 1)                                          # (B, J, 3, 4) relative transforms
    T = np.einsum("vj,bjk->bvk", f(m["weights"]), A.reshape(B, J, 12)).reshape(B, V, 3, 4)
    v = np.einsum("bvrc,bvc->bvr", T[..., :3], p) + T[..., 3]
    return v, p, A, np.concatenate([betas, pf], 1)


def lbs_inputs(tag, B, NB):
    g = rng(tag)
    return (0.5 * g.standard_normal((B, NB))).astype(np.float32), (0.4 * g.standard_normal((B, J * 3))).astype(np.float32)


def fp16_plane_bound(m, coef, vref):
    """ops.lbs_skin_v2's stated bound of the fp16-operand-plane form: 2^-11 |v| (the store) + 2^-10 sum_k |coef_k| |dirs_k|
    (the operands' own fp16 rounding, on the un-skinned offset; a rotation mixes at most the three coordinates' worth) +
    the fp32 kernel's 5e-6."""
    V, NB = m["shapedirs"].shape[0], m["shapedirs"].shape[2]
    ad = np.concatenate([np.abs(m["shapedirs"]).reshape(V * 3, NB).T, np.abs(m["posedirs"])], 0).astype(np.float64)
    S = (np.abs(coef) @ ad).reshape(len(coef), V, 3).sum(-1, keepdims=True)
    return np.abs(vref) * 2.0 ** -11 + 2.0 ** -10 * S + 5e-6


# ----------------------------------------------------------------------------- 1. skinning at arbitrary meshes
VS = (1, 2, 15, 16, 17, 127, 128, 129, 130, 1000, 5022, 5023, 5024)
BS = (1, 16, 17, 65, 300)


@pytest.mark.parametrize("V", VS)
def test_skinning_forms_at_any_vertex_and_frame_count(V):
    """utils.lbs.lbs at its three precisions, ops.lbs_skin_v2 (fp32, fp16 vertex_exact, fp16 operand planes) and
    ops.lbs_skin_v2_train against the float64 LBS.  FLAME-scale vertices (|v| ~ 0.1): the fp32-output forms are held to the
    5e-6 the golden tests use (exact-fp32 MFMA or split-bf16 products with fp32 accumulation: ~1e-6 observed), v_posed to the
    same; the fp16 forms to the header's bounds; and the vertex_exact fp16 output must be the fp32 kernel's output rounded to
    fp16 BIT FOR BIT at every V -- a lane pair made only of padding lanes must not overwrite slot V - 2 (even V)."""
    from msmd_amd.utils.lbs import lbs
    o = ops()
    m, t, c = model(V, 150)
    for B in BS:
        betas, pose = lbs_inputs(f"geom_lbs/{V}/{B}", B, 150)
        vref, pref, _, coef = lbs64(m, betas, pose)
        for prec in ("fp32", "bf16x3_valu", "bf16x3"):
            v, _ = lbs(dev(betas), dev(pose), t["v_template"], t["shapedirs"], t["posedirs"], t["J_regressor"],
                       t["parents"], t["weights"], constants=c, precision=prec)
            assert v.shape == (B, V, 3)
            err = float(np.abs(host(v) - vref).max())
            assert err <= 5e-6, (V, B, prec, err)
        tiles = o.lbs_prepare(dev(betas), dev(pose), c.JS, c.parents, KP, want_blend_tiles=True)[4]
        v32 = o.lbs_skin_v2(tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, V)
        assert float(np.abs(host(v32) - vref).max()) <= 5e-6, (V, B)
        V_ld = V + (V & 1)
        for planes in (None, c.dirs_f16):
            v16 = o.lbs_skin_v2(tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, V, out_dtype=torch.float16,
                                dirs_f16=planes)
            assert v16.dtype == torch.float16 and v16.shape == (B, V, 3) and v16.stride(0) == V_ld * 3
            err = np.abs(host(v16) - vref)
            if planes is None:
                assert torch.equal(v16, v32.to(torch.float16)), (V, B, np.argwhere((v16 != v32.half()).cpu().numpy())[:4])
                assert np.all(err <= np.abs(vref) * 2.0 ** -11 + 5e-6), (V, B)
            else:
                assert np.all(err <= fp16_plane_bound(m, coef, vref)), (V, B, float(err.max()))
            if V & 1:   # the padded slot V of each row holds a copy of vertex V - 1 (include/msmd_hip.h)
                rows = torch.as_strided(v16, (B, V_ld, 3), (V_ld * 3, 3, 1))
                assert torch.equal(rows[:, V], rows[:, V - 1]), (V, B)
        vt_, vp_ = o.lbs_skin_v2_train(tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, V)
        assert float(np.abs(host(vt_) - vref).max()) <= 5e-6, (V, B)
        assert float(np.abs(host(vp_) - pref).max()) <= 5e-6, (V, B)


@pytest.mark.parametrize("NB", [1, 10, 150, 156])
def test_skinning_every_coefficient_width_and_matrix_poses(NB):
    """NB shape coefficients + 36 pose features in the 192-wide K row: 1, 10, FLAME's 150 and 156 (the widest KP = 192 admits),
    axis-angle and rotation-matrix poses (pose2rot=False: the coefficients are the given matrices minus I), at an even, an odd
    and a 128-multiple vertex count; fp32-output forms to 5e-6, vertex_exact fp16 bit for bit, fp16 planes to the header bound."""
    from msmd_amd.utils.lbs import lbs
    o = ops()
    for V in (130, 5023, 1024):
        m, t, c = model(V, NB)
        for B in (17, 65):
            betas, pose = lbs_inputs(f"geom_nb/{NB}/{V}/{B}", B, NB)
            R = rodrigues64(pose.reshape(-1, 3)).astype(np.float32).reshape(B, J * 9)
            for p, is_mat in ((pose, False), (R, True)):
                vref, _, _, coef = lbs64(m, betas, p, pose_is_matrix=is_mat)
                for prec in ("fp32", "bf16x3_valu", "bf16x3"):
                    v, _ = lbs(dev(betas), dev(p), t["v_template"], t["shapedirs"], t["posedirs"], t["J_regressor"],
                               t["parents"], t["weights"], pose2rot=not is_mat, constants=c, precision=prec)
                    err = float(np.abs(host(v) - vref).max())
                    assert err <= 5e-6, (NB, V, B, is_mat, prec, err)
                tiles = o.lbs_prepare(dev(betas), dev(p), c.JS, c.parents, KP, pose_is_matrix=is_mat, want_blend_tiles=True)[4]
                v32 = o.lbs_skin_v2(tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, V)
                v16 = o.lbs_skin_v2(tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, V, out_dtype=torch.float16)
                assert torch.equal(v16, v32.to(torch.float16)), (NB, V, B, is_mat)
                v16p = o.lbs_skin_v2(tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, V, out_dtype=torch.float16,
                                     dirs_f16=c.dirs_f16)
                assert np.all(np.abs(host(v16p) - vref) <= fp16_plane_bound(m, coef, vref)), (NB, V, B, is_mat)


# ----------------------------------------------------------------------------- 2. FLAME's fast path at other widths
def flame_model(n_shape, n_exp):
    from msmd_amd.utils.flame import FLAME, FLAMEConfig
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset, cfg.n_shape, cfg.n_exp = synth.flame_asset(), n_shape, n_exp
    return FLAME(cfg).to(DEV)


def flame64(fl, shape, exp, pose6):
    """FLAME.forward's vertices in float64: betas = [shape | exp], full pose = [global | identity neck | jaw | identity eyes]."""
    B = len(shape)
    m = dict(v_template=host(fl.v_template), shapedirs=host(fl.shapedirs), posedirs=host(fl.posedirs),
             J_regressor=host(fl.J_regressor), weights=host(fl.lbs_weights), parents=fl.parents.cpu().numpy())
    z = np.zeros((B, 3))
    full = np.concatenate([pose6[:, :3], z, pose6[:, 3:], z, z], 1)
    return lbs64(m, np.concatenate([shape, exp], 1), full)[0]


@pytest.mark.parametrize("n_shape,n_exp", [(50, 50), (95, 10), (96, 10), (100, 50), (120, 36)])
def test_flame_fast_path_at_every_shape_and_expression_width(n_shape, n_exp):
    """FLAME(config).forward's in-place kinematics + skinning path (utils/flame.py: NS + NE + 36 <= 192) at shape / expression
    widths other than 100 / 50: one-subject batches (the folded template when NS >= 96), mixed batches, and a batch equal to a
    one-subject batch in its first 96 shape coefficients but not in coefficient 97 (the fold stays on: it covers only the
    first 96).  fp32 vertices to 5e-6 against float64; fp16 vertex_exact vertices are the fp32 ones rounded, bit for bit."""
    fl = flame_model(n_shape, n_exp)
    o = ops()
    g = rng(f"geom_flame/{n_shape}/{n_exp}")
    cases = []
    for B, kind in ((100, "one"), (37, "mixed"), (1, "one"), (100, "k97")):
        shape = (0.5 * g.standard_normal((B, n_shape))).astype(np.float32)
        if kind != "mixed":
            shape[:] = shape[:1]
        if kind == "k97":
            if n_shape <= 96:
                continue
            shape[B // 2, 96] += 0.5
        cases.append((B, kind, shape, (0.5 * g.standard_normal((B, n_exp))).astype(np.float32),
                      (0.4 * g.standard_normal((B, 6))).astype(np.float32)))
    for B, kind, shape, exp, pose in cases:
        args = (dev(shape), dev(exp), dev(pose))
        vref = flame64(fl, shape, exp, pose)
        v = fl(*args, return_lm2d=False, return_lm3d=False)[0]
        err = float(np.abs(host(v) - vref).max())
        assert err <= 5e-6, (n_shape, n_exp, B, kind, err)
        fl.vertex_dtype, fl.vertex_exact = torch.float16, True
        try:
            v16 = fl(*args, return_lm2d=False, return_lm3d=False)[0]
        finally:
            del fl.vertex_dtype, fl.vertex_exact
        assert torch.equal(v16, v.to(torch.float16)), (n_shape, n_exp, B, kind)
        # the device's own fold decision: on for one subject (and for the coefficient-97 batch), off otherwise
        c = fl._pack()["lbs"]
        _, flag, _ = o.flame_prepare(*args, None, c.JS, c.parents, False, c.dirs, c.template_planes)
        folds = n_shape >= 96 and kind in ("one", "k97")
        assert (int(flag.item()) == 0) == folds, (n_shape, n_exp, B, kind, int(flag.item()))


def test_flame_prepare_below_96_shape_coefficients_reports_varies():
    """msmd_flame_prepare with NS < 96 cannot fold: handed a flag buffer that holds zero (here filled by the test, in a real
    call whatever the allocator returns) and a folded-template buffer of garbage, it must set the flag to "varies", so that
    msmd_lbs_skin_v2 takes the general path and never reads the unwritten template."""
    from msmd_amd import _lib
    o = ops()
    lib = _lib.load()
    fl = flame_model(50, 50)
    c = fl._pack()["lbs"]
    g = rng("geom_flag")
    B = 40
    shape = np.repeat((0.5 * g.standard_normal((1, 50))).astype(np.float32), B, 0)   # one subject: would fold if it could
    exp = (0.5 * g.standard_normal((B, 50))).astype(np.float32)
    pose = (0.4 * g.standard_normal((B, 6))).astype(np.float32)
    ts, te, tp = dev(shape), dev(exp), dev(pose)
    tiles = torch.empty((B + 15) // 16, o.SKIN_TILE_BYTES // 2, device=DEV, dtype=torch.float16)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    folded = torch.full((3, c.Vp), float("nan"), device=DEV)
    rc = lib.msmd_flame_prepare(o._p(ts), o._p(te), o._p(tp), None, o._p(c.JS), o._p(c.parents), None, None, None,
                                o._p(tiles), B, 50, 50, 0, o._p(flag), o._p(folded), o._p(c.dirs), o._p(c.template_planes),
                                c.Vp, o._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert int(flag.item()) != 0
    v = o.lbs_skin_v2(tiles, B, c.template_planes, c.dirs_hl, c.weight_planes, c.V, shape_varies=flag, folded=folded)
    assert float(np.abs(host(v) - flame64(fl, shape, exp, pose)).max()) <= 5e-6
    # the same call with NS >= 96 folds: flag 0 whatever it held before
    fl = flame_model(100, 50)
    c = fl._pack()["lbs"]
    shape = np.repeat((0.5 * g.standard_normal((1, 100))).astype(np.float32), B, 0)
    flag.fill_(7)
    _, flag2, folded2 = o.flame_prepare(dev(shape), te, tp, None, c.JS, c.parents, False, c.dirs, c.template_planes)
    rc = lib.msmd_flame_prepare(o._p(dev(shape)), o._p(te), o._p(tp), None, o._p(c.JS), o._p(c.parents), None, None, None,
                                o._p(tiles), B, 100, 50, 0, o._p(flag), o._p(folded), o._p(c.dirs), o._p(c.template_planes),
                                c.Vp, o._stream())
    assert rc == 0 and int(flag.item()) == 0 and int(flag2.item()) == 0
    assert torch.equal(folded, folded2)


# ----------------------------------------------------------------------------- 3. skinning backward
def bwd64(g, p, A, W):
    """float64 backward of v = sum_j w_j (R_j p + t_j): dp = (sum_j w_j R_j)^T g, dA(j, r, :) = sum_v w_j g_r [p ; 1], and
    the magnitudes the bounds are stated in: sum_c |g_c| sum_j w_j |R_j[c, r]|, and sum_v w_j |g_r| |[p ; 1]|."""
    ph = np.concatenate([p, np.ones(p.shape[:2] + (1,))], 2)
    Rb = np.einsum("vj,bjrc->bvrc", W, A[..., :3])
    dp = np.einsum("bvrc,bvr->bvc", Rb, g)
    dp_mag = np.einsum("vj,bjrc,bvr->bvc", W, np.abs(A[..., :3]), np.abs(g))
    G = (g[:, :, :, None] * ph[:, :, None, :]).reshape(len(g), -1, 12)
    dA = np.einsum("vj,bvk->bjk", W, G)
    dA_mag = np.einsum("vj,bvk->bjk", W, np.abs(G))
    return dp, dp_mag, dA, dA_mag


@pytest.mark.parametrize("V", VS)
def test_skinning_backward_against_float64(V):
    """ops.lbs_skin_bwd (one wave per frame; lane l walks vertices l, l + 64, ..., then a 64-lane tree) against float64 on the
    kernel's own fp32 inputs.  dp: a 5-term blend of R then a 3-term dot -> |err| <= 8 u sum_c |g_c| sum_j w_j |R_j| (+2 u
    slack); the padding vertices V..Vp-1 exactly 0.  dA: ceil(V / 64) sequential terms per lane, 6 tree levels and 2
    roundings per term -> |err| <= (ceil(V / 64) + 8) u sum_v |w g p|.  A dropped or double-counted vertex is off by orders
    of magnitude."""
    o = ops()
    m, t, c = model(V, 150)
    W = m["weights"].astype(np.float64)
    for B in BS:
        betas, pose = lbs_inputs(f"geom_bwd/{V}/{B}", B, 150)
        _, pref, Aref, _ = lbs64(m, betas, pose)
        p32 = pref.astype(np.float32)
        A32 = Aref.astype(np.float32)
        g32 = rng(f"geom_bwd_g/{V}/{B}").standard_normal((B, V, 3)).astype(np.float32)
        dp, dA = o.lbs_skin_bwd(dev(g32), dev(p32), dev(A32.reshape(B, J, 12)), c.weight_planes)
        dp, dA = host(dp), host(dA)
        assert dp.shape == (B, 3, c.Vp) and np.all(dp[:, :, V:] == 0), (V, B)
        rdp, rdp_mag, rdA, rdA_mag = bwd64(g32.astype(np.float64), p32.astype(np.float64), A32.astype(np.float64), W)
        assert np.all(np.abs(dp[:, :, :V].transpose(0, 2, 1) - rdp) <= 10 * U * rdp_mag), (V, B)
        bound = (math.ceil(V / 64) + 8) * U * rdA_mag
        err = np.abs(dA - rdA)
        assert np.all(err <= bound), (V, B, float((err / bound).max()))


@pytest.mark.parametrize("NB", [10, 150])
def test_skin_fn_gradients_against_float64(NB):
    """SkinFn (the differentiable FLAME pass: msmd_lbs_skin_v2_train forward, msmd_lbs_skin_bwd + one fp32 GEMM backward)
    end to end: dcoef = dp . dirs^T and dA against float64 from the same coef / A.  dA: the backward's bound above plus
    sum_v w |g| |delta p| for the forward's p (5e-6, the fp32-output tolerance).  dcoef: dp's bound carried through |dirs|,
    plus the GEMM's fp32 accumulation over K = 3 Vp terms (worst case (K / 4 + 8) u sum |dp| |dirs|: 4-product MFMA steps in
    sequence)."""
    from msmd_amd.utils.lbs import SkinFn
    for V in (130, 5023):
        m, t, c = model(V, NB)
        W = m["weights"].astype(np.float64)
        for B in (17, 65):
            betas, pose = lbs_inputs(f"geom_skinfn/{NB}/{V}/{B}", B, NB)
            _, pref, Aref, coef = lbs64(m, betas, pose)
            coef32 = np.zeros((B, KP), np.float32)
            coef32[:, :coef.shape[1]] = coef
            A32 = Aref.astype(np.float32).reshape(B, J, 12)
            tc = dev(coef32).requires_grad_(True)
            tA = dev(A32).requires_grad_(True)
            g32 = rng(f"geom_skinfn_g/{NB}/{V}/{B}").standard_normal((B, V, 3)).astype(np.float32)
            SkinFn.apply(tc, tA, c).backward(dev(g32))
            g64 = g32.astype(np.float64)
            rdp, rdp_mag, rdA, rdA_mag = bwd64(g64, pref, A32.astype(np.float64).reshape(B, J, 3, 4), W)
            dp_slack = np.einsum("vj,bv->bj", W, np.abs(g64).sum(2)) * 5e-6
            err = np.abs(host(tA.grad).reshape(B, J, 12) - rdA)
            bound = (math.ceil(V / 64) + 8) * U * rdA_mag + dp_slack[:, :, None] * 1.0
            assert np.all(err <= bound), (NB, V, B, float((err / bound).max()))
            dirs = host(c.dirs)[:, :, :V]                                        # (3, KP, V)
            rdc = np.einsum("bvc,ckv->bk", rdp, dirs)
            mag = np.einsum("bvc,ckv->bk", np.abs(rdp), np.abs(dirs))
            dpb = np.einsum("bvc,ckv->bk", 10 * U * rdp_mag, np.abs(dirs))
            # the forward's p enters dp only through A (not p): dp's error is its own bound; add the GEMM's accumulation
            bound = dpb + (3 * c.Vp / 4 + 8) * U * mag
            err = np.abs(host(tc.grad) - rdc)
            assert np.all(err <= bound), (NB, V, B, float((err / bound).max()))


# ----------------------------------------------------------------------------- 4. landmarks, contour row, Rodrigues
@pytest.mark.parametrize("V", [3, 130, 5023])
def test_landmarks_shared_and_per_frame_against_float64(V):
    """ops.landmarks / vertices2landmarks (one thread per (frame, landmark), 256 per workgroup): shared (L,) and per-frame
    (B, L) face ids, shared and per-frame barycentrics, B * L on both sides of 256-thread boundaries, faces that touch vertex
    V - 1.  out = sum_k p_k bc_k as one product and two sums: |err| <= 4 u sum_k |p_k bc_k|."""
    from msmd_amd.utils.lbs import vertices2landmarks
    o = ops()
    for B, L in ((1, 255), (1, 256), (1, 257), (3, 85), (4, 64), (257, 1), (17, 68), (33, 79)):
        g = rng(f"geom_lmk/{V}/{B}/{L}")
        F = 97
        faces = g.integers(0, V, (F, 3)).astype(np.int32)
        faces[0] = [V - 1, 0, V - 1]
        faces[F - 1] = [V // 2, V - 1, max(V - 2, 0)]
        verts = (0.3 * g.standard_normal((B, V, 3))).astype(np.float32)
        idx_s = g.integers(0, F, L).astype(np.int32)
        idx_s[:: 7] = 0
        idx_b = g.integers(0, F, (B, L)).astype(np.int32)
        idx_b[:, -1] = F - 1
        bc_s = g.uniform(0.05, 1.0, (L, 3)).astype(np.float32)
        bc_b = g.uniform(-0.2, 1.0, (B, L, 3)).astype(np.float32)
        v64 = verts.astype(np.float64)
        for idx, bc in ((idx_s, bc_s), (idx_b, bc_b), (idx_s, bc_b), (idx_b, bc_s)):
            fi = np.broadcast_to(idx, (B, L))
            corners = v64[np.arange(B)[:, None, None], faces[fi]]                # (B, L, 3 corners, 3)
            w = np.broadcast_to(bc, (B, L, 3)).astype(np.float64)[..., None]
            ref = (corners * w).sum(2)
            mag = np.abs(corners * w).sum(2)
            got = o.landmarks(dev(verts), dev(faces), dev(idx), dev(bc))
            assert got.shape == (B, L, 3)
            assert np.all(np.abs(host(got) - ref) <= 4 * U * mag), (V, B, L, idx.ndim, bc.ndim)
            got2 = vertices2landmarks(dev(verts), dev(faces.astype(np.int64)), dev(idx.astype(np.int64)), dev(bc))
            assert torch.equal(got2, got)


def lmk_row64(full_pose, chain, is_matrix):
    """utils/flame.py:126-172 in float64: rel = product of the chain's rotations (chain order, left-multiplied), yaw =
    atan2(-rel[2, 0], sqrt(rel[0, 0]^2 + rel[1, 0]^2)) in degrees, round half to even, clamp <= 39, negative -> 39 - y
    (78 below -39).  -> (rows, yaw in degrees)."""
    B = len(full_pose)
    Rs = full_pose.reshape(B, -1, 3, 3) if is_matrix else rodrigues64(full_pose.reshape(-1, 3)).reshape(B, -1, 3, 3)
    rel = np.broadcast_to(np.eye(3), (B, 3, 3))
    for j in chain:
        rel = Rs[:, j] @ rel
    yaw = np.degrees(np.arctan2(-rel[:, 2, 0], np.sqrt(rel[:, 0, 0] ** 2 + rel[:, 1, 0] ** 2)))
    y = np.round(np.minimum(yaw, 39.0))
    row = np.where(y < 0, np.where(y < -39, 78, 39 - y), y)
    return row.astype(np.int64), yaw


def test_dynamic_lmk_row_sweeps_yaw_exactly():
    """ops.dynamic_lmk_row against the float64 LUT row as an exact integer, yaw swept through [-90, 90] degrees (with tilt,
    roll and a neck rotation mixed in) in axis-angle and matrix form; poses within 1e-3 degrees of a .5 rounding boundary are
    left out (fp32 yaw is good to ~1e-5 degrees there)."""
    o = ops()
    B = 4001
    g = rng("geom_lmk_row")
    yaw = np.radians(np.linspace(-90.0, 90.0, B))
    glob = np.stack([0.2 * g.standard_normal(B), yaw, 0.2 * g.standard_normal(B)], 1)
    neck = 0.15 * g.standard_normal((B, 3))
    full = np.concatenate([glob, neck, 0.2 * g.standard_normal((B, 9))], 1).astype(np.float32)
    chain = np.array([1, 0], np.int32)
    mats = rodrigues64(full.reshape(-1, 3)).astype(np.float32).reshape(B, 45)
    for pose, is_mat in ((full, False), (mats, True)):
        ref, ydeg = lmk_row64(pose.astype(np.float64), chain, is_mat)
        keep = np.abs(np.abs(ydeg - np.floor(ydeg)) - 0.5) > 1e-3
        assert keep.sum() > 0.99 * B and ydeg.min() < -80 and ydeg.max() > 80
        row = o.dynamic_lmk_row(dev(pose), dev(chain), pose_is_matrix=is_mat).cpu().numpy()
        assert np.array_equal(row[keep], ref[keep]), (is_mat, np.argwhere(row[keep] != ref[keep])[:4])


@pytest.mark.parametrize("N", [1, 255, 256, 257, 100003])
def test_batch_rodrigues_against_float64(N):
    """utils.lbs.batch_rodrigues (the reference's +1e-8 formula) against float64 of the same formula on the same fp32 input,
    r = 0, |r| ~ 1e-7 and angles up to pi included.  Entries of R are <= 1: the angle's sqrt of a 3-term sum (3 u relative)
    moves sin / cos by at most pi * 3 u, sinf / cosf / the division add 2 u each, the 3-term K.K products 3 u and the sum with
    I 1 u: |err| <= 32 u."""
    from msmd_amd.utils.lbs import batch_rodrigues
    g = rng(f"geom_rod/{N}")
    d = g.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = d * g.uniform(0.0, math.pi, (N, 1))
    r[0] = 0.0
    if N > 2:
        r[1] = 1e-7 * d[1]
        r[2] = (math.pi - 1e-6) * d[2]
    if N > 4:
        r[N // 2] = 1.2e-7 * d[N // 2]
    r = r.astype(np.float32)
    got = host(batch_rodrigues(dev(r)))
    assert got.shape == (N, 3, 3)
    err = np.abs(got - rodrigues64(r))
    assert float(err.max()) <= 32 * U, float(err.max() / U)
    assert np.array_equal(got[0], np.eye(3))


# ----------------------------------------------------------------------------- 5. rotation conversions
# float64 restatements of utils/rotation_conversions.py (PyTorch3D: real-first quaternions, the 1e-6 small-angle branch,
# _sqrt_positive_part, _copysign)
def q2m64(q):
    r, i, j, k = np.moveaxis(q, -1, 0)
    s = 2.0 / (q * q).sum(-1)
    o = np.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                  s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                  s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def m2q64(m):
    sp = lambda x: np.sqrt(np.maximum(x, 0.0))
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    cs = lambda a, b: np.where((a < 0) != (b < 0), -a, a)
    return np.stack([0.5 * sp(1 + m00 + m11 + m22), cs(0.5 * sp(1 + m00 - m11 - m22), m[..., 2, 1] - m[..., 1, 2]),
                     cs(0.5 * sp(1 - m00 + m11 - m22), m[..., 0, 2] - m[..., 2, 0]),
                     cs(0.5 * sp(1 - m00 - m11 + m22), m[..., 1, 0] - m[..., 0, 1])], -1)


def _soa(angle, half):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.abs(angle) < 1e-6, 0.5 - angle * angle / 48, np.sin(half) / angle)


def aa2q64(a):
    angle = np.sqrt((a * a).sum(-1, keepdims=True))
    return np.concatenate([np.cos(0.5 * angle), a * _soa(angle, 0.5 * angle)], -1)


def q2aa64(q):
    half = np.arctan2(np.sqrt((q[..., 1:] ** 2).sum(-1, keepdims=True)), q[..., :1])
    return q[..., 1:] / _soa(2 * half, half)


def d62m64(d6):
    nrm = lambda x: x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)
    b1 = nrm(d6[..., :3])
    b2 = nrm(d6[..., 3:] - (b1 * d6[..., 3:]).sum(-1, keepdims=True) * b1)
    return np.stack([b1, b2, np.cross(b1, b2)], -2)


def axis64(axis, a):
    c, s, one, z = np.cos(a), np.sin(a), np.ones_like(a), np.zeros_like(a)
    R = {"X": (one, z, z, z, c, -s, z, s, c), "Y": (c, z, s, z, one, z, -s, z, c), "Z": (c, -s, z, s, c, z, z, z, one)}[axis]
    return np.stack(R, -1).reshape(a.shape + (3, 3))


def e2m64(e, conv):
    return axis64(conv[0], e[..., 0]) @ axis64(conv[1], e[..., 1]) @ axis64(conv[2], e[..., 2])


def m2e64(m, conv):
    def tan(axis, other, data, horizontal, tb):
        i1, i2 = {"X": (2, 1), "Y": (0, 2), "Z": (1, 0)}[axis]
        if horizontal:
            i1, i2 = i2, i1
        if horizontal == ((axis + other) in ("XY", "YZ", "ZX")):
            return np.arctan2(data[..., i1], data[..., i2])
        return np.arctan2(-data[..., i2], data[..., i1]) if tb else np.arctan2(data[..., i2], -data[..., i1])
    i0, i2 = "XYZ".index(conv[0]), "XYZ".index(conv[2])
    tb = i0 != i2
    central = np.arcsin(m[..., i0, i2] * (-1.0 if i0 - i2 in (-1, 2) else 1.0)) if tb else np.arccos(m[..., i0, i0])
    return np.stack([tan(conv[0], conv[1], m[..., i2], False, tb), central, tan(conv[2], conv[1], m[..., i0, :], True, tb)], -1)


def qraw64(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def qstd64(q):
    return np.where(q[..., :1] < 0, -q, q)


def qinv64(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def qapply64(q, p):
    return qraw64(qraw64(q, np.concatenate([np.zeros(p.shape[:-1] + (1,)), p], -1)), qinv64(q))[..., 1:]


CONVENTIONS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX", "XYX", "XZX", "YXY", "YZY", "ZXZ", "ZYZ")


def unit(g, n, k):
    x = g.standard_normal((n, k))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def conditioned_inputs(g, n):
    """Inputs away from the 1e-6 small-angle threshold (angles >= 0.2), from theta = pi (<= 3.0), from gimbal lock and from
    zero quaternion components (|q_i| >= 0.15: the square roots of matrix_to_quaternion see arguments >= 0.09)."""
    aa = unit(g, n, 3) * g.uniform(0.2, 3.0, (n, 1))
    q = unit(g, 4 * n + 64, 4)
    q = q[np.all(np.abs(q) >= 0.15, 1)][:n]
    assert len(q) == n
    q = q * np.where(q[:, :1] < 0, -1.0, 1.0)
    qs = q * g.uniform(0.5, 2.0, (n, 1))                      # unnormalised input of quaternion_to_matrix
    q2 = unit(g, n, 4)
    d6 = g.standard_normal((3 * n + 64, 6))                     # first row not tiny, second at least 30 degrees off it
    a1, a2 = d6[:, :3], d6[:, 3:]
    perp = np.linalg.norm(a2 - (a1 * a2).sum(1, keepdims=True) * a1 / (a1 * a1).sum(1, keepdims=True), axis=1)
    d6 = d6[(np.linalg.norm(a1, axis=1) >= 0.3) & (perp >= 0.5 * np.linalg.norm(a2, axis=1))][:n]
    assert len(d6) == n
    pts = 2.0 * g.standard_normal((n, 3))
    return dict(aa=aa, q=q, qs=qs, q2=q2, d6=d6, pts=pts, R=q2m64(q))


def euler_inputs(g, n, conv):
    e = g.uniform(-3.0, 3.0, (n, 3))
    e[:, 1] = g.uniform(-1.2, 1.2, n) if conv[0] != conv[2] else g.uniform(0.4, 2.7, n)
    return e


# op -> (function name, float64 restatement, inputs, c): elementwise |err| <= c u max(1, |ref| of the item).  c per op: the
# quaternion / axis-angle forward maps (entries <= 1, a handful of roundings, sinf / cosf within 2 ulp): 16, 24 where a
# quaternion becomes a matrix (2 / |q|^2 and two-product sums on every entry); the matrix ->
# quaternion / axis-angle maps (square roots of arguments >= 0.09 and atan2 of components >= 0.15): 48; rotation_6d_to_matrix
# (two normalisations and a cross product): 32; quaternion products (4-term dot products of unit quaternions): 8, twice for
# quaternion_apply: 24 of the point's scale; copies and sign flips: 0 (bit equality).
ROT_OPS = {
    "quaternion_to_matrix": (lambda RC, x: RC.quaternion_to_matrix(x[0]), lambda x: q2m64(x[0]), ("qs",), 24),
    "matrix_to_quaternion": (lambda RC, x: RC.matrix_to_quaternion(x[0]), lambda x: m2q64(x[0]), ("R",), 48),
    "axis_angle_to_quaternion": (lambda RC, x: RC.axis_angle_to_quaternion(x[0]), lambda x: aa2q64(x[0]), ("aa",), 16),
    "quaternion_to_axis_angle": (lambda RC, x: RC.quaternion_to_axis_angle(x[0]), lambda x: q2aa64(x[0]), ("q",), 16),
    "axis_angle_to_matrix": (lambda RC, x: RC.axis_angle_to_matrix(x[0]), lambda x: q2m64(aa2q64(x[0])), ("aa",), 24),
    "matrix_to_axis_angle": (lambda RC, x: RC.matrix_to_axis_angle(x[0]), lambda x: q2aa64(m2q64(x[0])), ("R",), 48),
    "rotation_6d_to_matrix": (lambda RC, x: RC.rotation_6d_to_matrix(x[0]), lambda x: d62m64(x[0]), ("d6",), 32),
    "matrix_to_rotation_6d": (lambda RC, x: RC.matrix_to_rotation_6d(x[0]),
                              lambda x: x[0][..., :2, :].reshape(x[0].shape[:-2] + (6,)), ("R",), 0),
    "axis_angle_to_rotation_6d": (lambda RC, x: RC.axis_angle_to_rotation_6d(x[0]),
                                  lambda x: q2m64(aa2q64(x[0]))[..., :2, :].reshape(x[0].shape[:-1] + (6,)), ("aa",), 24),
    "standardize_quaternion": (lambda RC, x: RC.standardize_quaternion(x[0]), lambda x: qstd64(x[0]), ("q2",), 0),
    "quaternion_invert": (lambda RC, x: RC.quaternion_invert(x[0]), lambda x: qinv64(x[0]), ("q2",), 0),
    "quaternion_raw_multiply": (lambda RC, x: RC.quaternion_raw_multiply(x[0], x[1]), lambda x: qraw64(x[0], x[1]),
                                ("q2", "q"), 8),
    "quaternion_multiply": (lambda RC, x: RC.quaternion_multiply(x[0], x[1]), lambda x: qstd64(qraw64(x[0], x[1])),
                            ("q2", "q"), 8),
    "quaternion_apply": (lambda RC, x: RC.quaternion_apply(x[0], x[1]), lambda x: qapply64(x[0], x[1]), ("q", "pts"), 24),
}


def unaligned(t):
    """The same values as a view 4 bytes into a larger buffer: the kernel's dword staging path (base not 16-byte aligned)."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16
    return v


def check_rot(name, got, ref, c):
    got = host(got)
    assert got.shape == ref.shape, name
    n = ref.shape[0]
    scale = np.maximum(1.0, np.abs(ref.reshape(n, -1)).max(1)).reshape((n,) + (1,) * (ref.ndim - 1))
    err = np.abs(got - ref)
    if c == 0:
        assert np.array_equal(got, ref), name
    else:
        assert np.all(err <= c * U * scale), (name, float((err / (c * U * scale)).max()))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 262147])
def test_rotation_conversions_past_one_workgroup_against_float64(n):
    """All 16 MSMD_ROT_* ops through utils/rotation_conversions.py at n items (256 per workgroup: one partial, exactly one,
    one plus one, many, and a 1024-workgroup grid with a 3-item tail), as (n, ...) and as a leading (1, n, ...) shape, from
    16-byte-aligned tensors and from unaligned views (first input, second input) -- compared elementwise with float64 of the
    same formulas on the same fp32 inputs.  All 12 Euler conventions in both directions."""
    from msmd_amd.utils import rotation_conversions as RC
    g = rng(f"geom_rot/{n}")
    x = conditioned_inputs(g, n)
    x32 = {k: v.astype(np.float32) for k, v in x.items()}
    for name, (fn, ref_fn, keys, c) in ROT_OPS.items():
        ref = ref_fn([x32[k].astype(np.float64) for k in keys])
        ts = [dev(x32[k]) for k in keys]
        check_rot(name, fn(RC, ts), ref, c)
        got = fn(RC, [t.reshape((1, n) + t.shape[1:]) for t in ts])
        assert got.shape[:2] == (1, n), name
        check_rot(name, got.reshape(ref.shape), ref, c)
        for which in range(len(ts)):
            tu = list(ts)
            tu[which] = unaligned(ts[which])
            check_rot(f"{name} unaligned input {which}", fn(RC, tu), ref, c)
    # Euler angles: matrix -> angles on matrices built from conditioned angles, angles -> matrix on any angles in (-3, 3)
    for conv in CONVENTIONS:
        e32 = euler_inputs(g, n, conv).astype(np.float32)
        R32 = e2m64(e32.astype(np.float64), conv).astype(np.float32)
        te, tR = dev(e32), dev(R32)
        check_rot(f"e2m {conv}", RC.euler_angles_to_matrix(te, conv), e2m64(e32.astype(np.float64), conv), 16)
        check_rot(f"e2m {conv} unaligned", RC.euler_angles_to_matrix(unaligned(te), conv), e2m64(e32.astype(np.float64), conv), 16)
        # asin / acos of a central entry with |x| <= 0.93 (slope <= 2.7) and atan2 of pairs of norm >= 0.36: 48 u of max(1, |angle|)
        check_rot(f"m2e {conv}", RC.matrix_to_euler_angles(tR, conv), m2e64(R32.astype(np.float64), conv), 48)
        check_rot(f"m2e {conv} unaligned", RC.matrix_to_euler_angles(unaligned(tR), conv), m2e64(R32.astype(np.float64), conv), 48)


def test_rotation_conversions_singular_inputs():
    """Angle 0, 1e-7 (the small-angle branch), pi and pi - 1e-4, quaternions with w = 0 or w < 0, unnormalised quaternions and
    gimbal-lock Euler angles: every result finite, equal to oracle/rotations.py (the same fp32 branches) within the golden
    test's 2e-5, and the round trips hold -- axis_angle_to_matrix(matrix_to_axis_angle(R)) = R to 2e-3 near pi (w = 1/2
    sqrt(1 + tr R) of an O(u) argument: <= 1/2 sqrt(8 u) = 3.5e-4, doubled for the angle and once more for R) and 1e-5
    elsewhere; at Tait-Bryan gimbal lock matrix_to_euler_angles then euler_angles_to_matrix gives R back to 1e-5 (the angles are
    not unique there, the matrix is)."""
    from msmd_amd.utils import rotation_conversions as RC
    from oracle import rotations as orot
    g = rng("geom_rot_singular")
    d = unit(g, 8, 3)
    ang = np.array([0.0, 1e-7, 5e-7, 2e-6, math.pi, math.pi - 1e-4, 1.0, 3.0])
    aa = (d * ang[:, None]).astype(np.float32)
    aa = np.concatenate([aa, np.array([[math.pi, 0, 0], [0, -math.pi, 0], [0, 0, 1e-7]], np.float32)])
    q = np.concatenate([np.concatenate([np.zeros((4, 1)), unit(g, 4, 3)], 1),           # w = 0: half-turns
                        -np.abs(unit(g, 4, 4)),                                          # w < 0
                        3.0 * unit(g, 4, 4), 0.01 * unit(g, 4, 4),                       # unnormalised
                        [[1, 0, 0, 0], [-1, 0, 0, 0], [1, 1e-7, 0, 0]]]).astype(np.float32)
    taa, tq = dev(aa), dev(q)
    R = RC.axis_angle_to_matrix(taa)
    cases = dict(
        axis_angle_to_matrix=(R, orot.axis_angle_to_matrix(aa)),
        axis_angle_to_quaternion=(RC.axis_angle_to_quaternion(taa), orot.axis_angle_to_quaternion(aa)),
        axis_angle_to_rotation_6d=(RC.axis_angle_to_rotation_6d(taa), orot.axis_angle_to_rotation_6d(aa)),
        quaternion_to_matrix=(RC.quaternion_to_matrix(tq), orot.quaternion_to_matrix(q)),
        quaternion_to_axis_angle=(RC.quaternion_to_axis_angle(tq), orot.quaternion_to_axis_angle(q)),
        standardize_quaternion=(RC.standardize_quaternion(tq), orot.standardize_quaternion(q)),
        quaternion_multiply=(RC.quaternion_multiply(tq, tq.flip(0)), orot.quaternion_multiply(q, q[::-1])),
        matrix_to_quaternion=(RC.matrix_to_quaternion(R), orot.matrix_to_quaternion(host(R).astype(np.float32))),
        matrix_to_axis_angle=(RC.matrix_to_axis_angle(R), orot.matrix_to_axis_angle(host(R).astype(np.float32))),
    )
    for k, (got, want) in cases.items():
        got = host(got)
        assert np.all(np.isfinite(got)), k
        assert float(np.abs(got - want).max()) <= 2e-5, (k, float(np.abs(got - want).max()))
    Rh = host(R)
    back = host(RC.axis_angle_to_matrix(RC.matrix_to_axis_angle(R)))
    near_pi = np.linalg.norm(aa.astype(np.float64), axis=1) > 3.1
    err = np.abs(back - Rh).reshape(len(aa), -1).max(1)
    assert np.all(err[near_pi] <= 2e-3) and np.all(err[~near_pi] <= 1e-5), err
    # quaternion_to_axis_angle(axis_angle_to_quaternion(aa)) = aa below pi, through the small-angle branch included
    small = ~near_pi
    back_aa = host(RC.quaternion_to_axis_angle(RC.axis_angle_to_quaternion(taa)))
    assert np.all(np.abs(back_aa - aa)[small] <= 1e-6 + 4e-7 * np.abs(aa)[small].max())
    # gimbal lock: central angle 0 / pi (proper Euler) or +-pi/2 (Tait-Bryan)
    for conv in CONVENTIONS:
        c0 = (0.0, math.pi) if conv[0] == conv[2] else (math.pi / 2, -math.pi / 2)
        e = np.array([[0.3, c0[0], -0.7], [1.1, c0[1], 0.4], [-2.0, c0[0], 2.5]], np.float32)
        Re = RC.euler_angles_to_matrix(dev(e), conv)
        eb = RC.matrix_to_euler_angles(Re, conv)
        ebh = host(eb)
        assert np.all(np.isfinite(ebh)), conv
        assert float(np.abs(ebh - orot.matrix_to_euler_angles(host(Re).astype(np.float32), conv)).max()) <= 2e-5, conv
        if conv[0] != conv[2]:
            # Tait-Bryan: the outer angles come from entries scaled by cos(central) ~ -4e-8, consistently: R comes back.
            # (Proper Euler at central 0 / pi takes both from atan2 of O(u) entries -- the reference's formula, PyTorch3D's too --
            # so there only finiteness and agreement with the oracle on the same entries are asserted.)
            assert float(np.abs(host(RC.euler_angles_to_matrix(eb, conv)) - host(Re)).max()) <= 1e-5, conv
