"""Gradients of the geometry surface on the GPU (msmd_rotation_convert_bwd, msmd_batch_rodrigues_bwd, msmd_landmarks_bwd and the
autograd wiring in ops.py / utils) against float64 torch autograd of tests/geometry_grad_ref.py's restatements, which
tests/test_geometry_grad_cpu.py pins to the reference implementation's own gradients.  Every gradient element is compared.

Error measure: |g - g64| / max(1, |g64_item|_inf) in units of u = 2^-24.  Bound per op: c_op = max(16, 4 x yardstick), the
yardstick being the float32 torch-CPU autograd of the same restatement on the same inputs (`python tests/geometry_grad_ref.py`
prints it); the factor 4 covers device sinf / cosf / atan2f / division a few ulp looser than host libm and a different
association in the hand-written VJP.

    op         yardstick [u]   c_op [u]   GPU max [u]
    q2m            40.54        162.2        50.66
    m2q            12.22         48.9        12.33
    aa2q            4.00         16.0         3.52
    q2aa            4.16         16.6         4.60
    aa2m           16.66         66.6        12.65
    m2aa           14.12         56.5        13.18
    d62m          144.16        576.6       194.68
    m2d6            0.00         16.0         0.00
    aa2d6          11.75         47.0        10.62
    qstd            0.00         16.0         0.00
    qinv            0.00         16.0         0.00
    qraw            3.21         16.0         3.30
    qmul            3.21         16.0         3.30
    qapply          4.67         18.7         3.95
    e2m            10.56         42.2        11.12
    m2e            25.74        103.0         3.19
    rodrigues      24.98         99.9        24.98

(GPU max: the largest figure this file printed on an MI355X over all sizes, layouts and dtypes.)"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import geometry_grad_ref as G
from conftest import load_golden
from msmd_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = G.U
YARDSTICK = G.YARDSTICK      # re-measured by tests/test_geometry_grad_cpu.py
C_OP = {k: max(16.0, 4.0 * v) for k, v in YARDSTICK.items()}
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def RC():
    from msmd_amd.utils import rotation_conversions
    return rotation_conversions


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def host(t):
    return t.detach().double().cpu().numpy()


def shaped(key, x):
    """generator rows -> the public function's input shape (matrices as (n, 3, 3))."""
    return x.reshape(-1, 3, 3) if key == "R" else x


def call(key, ts, conv=None):
    name = (G.OPS.get(key) or G.EULER_OPS[key])[1]
    fn = getattr(RC(), name)
    return fn(*ts, conv) if conv is not None else fn(*ts)


def ref_fn(key, conv=None):
    if conv is not None:
        f = G.EULER_OPS[key][0]
        return lambda t: f(t, conv)
    return G.OPS[key][0]


def check(key, grads, refs, what, dtype=torch.float32):
    worst = 0.0
    for i, (g, r) in enumerate(zip(grads, refs)):
        assert g is not None, (what, "no gradient for operand", i)
        assert tuple(g.shape) == r.shape and g.dtype == dtype, (what, g.shape, g.dtype)
        got = host(g)
        n = r.shape[0]
        scale = np.maximum(1.0, np.abs(r.reshape(n, -1)).max(1)).reshape((n,) + (1,) * (r.ndim - 1))
        slack = EPS.get(dtype, 0.0) * np.abs(r)                  # the rounding of the returned gradient to the input's dtype
        err = np.maximum(np.abs(got - r) - slack, 0.0) / scale / U
        worst = max(worst, float(err.max()))
    print(f"{what}: max error {worst:.2f} u (bound {C_OP[key]:.1f})")
    assert worst <= C_OP[key], (what, worst, C_OP[key])
    return worst


def run_case(key, xs, g, what, conv=None, dtype=torch.float32, wrap=None):
    """xs: float32 numpy operands (already shaped).  wrap(i, leaf) -> the tensor handed to the op (a view of the leaf)."""
    leaves = [dev(x, dtype).requires_grad_(True) for x in xs]
    ins = [wrap(i, t) if wrap else t for i, t in enumerate(leaves)]
    out = call(key, ins, conv)
    assert out.grad_fn is not None and out.requires_grad, what
    out.backward(dev(g).reshape(out.shape))
    base = [host(t.detach()) for t in leaves]                     # the values the kernel saw (rounded to `dtype`)
    refs = G.vjp(ref_fn(key, conv), base, g)
    check(key, [t.grad for t in leaves], refs, what, dtype)
    return out.detach(), ins


# ----------------------------------------------------------------------------- 1. the 16 conversions
@pytest.mark.parametrize("n", G.SIZES)
def test_rotation_conversion_gradients_against_float64(n):
    """Every op (all 12 Euler conventions both ways) at item counts around the 256-item workgroup; every item satisfies the
    conditioning predicates; the forward output is bit-equal with and without requires_grad."""
    x = G.rotation_inputs(f"geom_grad/rot/{n}", n)
    assert G.predicates(x).all()
    for key, (_, _, operands) in G.OPS.items():
        xs = [shaped(o, x[o]) for o in operands]
        out, ins = run_case(key, xs, x[f"g{G.out_width(key)}"], f"{key} n={n}")
        with torch.no_grad():
            plain = call(key, [t.detach() for t in ins])
        assert plain.grad_fn is None and torch.equal(plain, out), key
    for conv in G.CONVENTIONS:
        xe = G.euler_inputs(f"geom_grad/euler/{n}", n, conv)
        assert G.euler_predicate(xe, conv).all()
        run_case("e2m", [xe["e"]], xe["g9"], f"e2m {conv} n={n}", conv)
        run_case("m2e", [xe["R"].reshape(-1, 3, 3)], xe["g3"], f"m2e {conv} n={n}", conv)


def layout_and_dtype_cases(key, xs, g, n, conv=None):
    """One op at n items: an unaligned view (leaf[1:] of a leaf one float longer), every second row of a (2 n)-row leaf, and
    fp16 / bf16 / float64 inputs (gradient in the input's dtype; the truth is float64 autograd at the values the kernel saw)."""
    tag = key if conv is None else f"{key} {conv}"
    refs = G.vjp(ref_fn(key, conv), xs, g)
    leaves, ins = [], []
    for a in xs:
        buf = torch.zeros(a.size + 1, device=DEV)
        buf[1:] = dev(a).reshape(-1)
        buf.requires_grad_(True)
        leaves.append(buf)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16
        ins.append(v)
    out = call(key, ins, conv)
    out.backward(dev(g).reshape(out.shape))
    assert all(float(b.grad[0]) == 0.0 for b in leaves), tag
    check(key, [b.grad[1:].view(a.shape) for b, a in zip(leaves, xs)], refs, f"{tag} unaligned")
    leaves = [torch.zeros((2 * n,) + a.shape[1:], device=DEV) for a in xs]
    for b, a in zip(leaves, xs):
        b[::2] = dev(a)
        b.requires_grad_(True)
    out = call(key, [b[::2] for b in leaves], conv)
    out.backward(dev(g).reshape(out.shape))
    assert all(float(b.grad[1::2].abs().max()) == 0.0 for b in leaves), tag
    check(key, [b.grad[::2] for b in leaves], refs, f"{tag} non-contiguous")
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        run_case(key, xs, g, f"{tag} {dt}", conv, dtype=dt)


def test_rotation_gradients_layouts_dtypes_and_broadcast():
    """n = 1000, every op -- the two Euler ops in three Tait-Bryan and two proper conventions: unaligned, non-contiguous and
    fp16 / bf16 / float64 inputs; then broadcast operands of the two-operand ops."""
    n = 1000
    x = G.rotation_inputs(f"geom_grad/rot/{n}", n)
    for key, (_, _, operands) in G.OPS.items():
        layout_and_dtype_cases(key, [shaped(o, x[o]) for o in operands], x[f"g{G.out_width(key)}"], n)
    for conv in ("XYZ", "ZXY", "YZX", "ZXZ", "XYX"):
        xe = G.euler_inputs(f"geom_grad/euler/{n}", n, conv)
        layout_and_dtype_cases("e2m", [xe["e"]], xe["g9"], n, conv)
        layout_and_dtype_cases("m2e", [xe["R"].reshape(-1, 3, 3)], xe["g3"], n, conv)
    # broadcast: one quaternion against n, and (7, 1, 4) x (1, 11, 4): the gradient is reduced over the broadcast dimension
    g4, g3 = x["g4"], x["g3"]
    for key, second, gk in (("qraw", "qb", g4), ("qmul", "qb", g4), ("qapply", "pts", g3)):
        a1 = x["qa"][:1]
        b = x[second]
        ta, tb = dev(a1).requires_grad_(True), dev(b).requires_grad_(True)
        out = call(key, [ta, tb])
        assert out.shape[0] == n
        out.backward(dev(gk))
        ra, rb = G.vjp(lambda p, q: ref_fn(key)(p.expand(n, -1), q), [a1, b], gk)
        # the n-term reduction of the first operand's gradient: n roundings on top of the per-item bound, in the sum's scale
        ga = host(ta.grad)
        per_item = G.vjp(ref_fn(key), [np.repeat(a1, n, 0), b], gk)[0]
        bound = (C_OP[key] * np.maximum(1.0, np.abs(per_item).max(1, keepdims=True)) + n * np.abs(per_item)).sum(0) * U
        assert ta.grad.shape == (1, 4) and np.all(np.abs(ga - ra) <= bound), (key, np.abs(ga - ra), bound)
        check(key, [tb.grad], [rb], f"{key} broadcast first operand")
        a2, b2 = x["qa"][:7].reshape(7, 1, 4), b[:11].reshape(1, 11, -1)
        ta, tb = dev(a2).requires_grad_(True), dev(b2).requires_grad_(True)
        out = call(key, [ta, tb])
        gg = gk[:77].reshape(7, 11, -1)
        out.backward(dev(gg))
        ra, rb = G.vjp(lambda p, q: ref_fn(key)(p.expand(7, 11, -1), q.expand(7, 11, -1)), [a2, b2], gg)
        assert ta.grad.shape == a2.shape and tb.grad.shape == b2.shape
        for got, want in ((host(ta.grad), ra), (host(tb.grad), rb)):
            assert float(np.abs(got - want).max()) <= (C_OP[key] + 11) * 11 * U * max(1.0, float(np.abs(want).max())), key


def test_rotation_special_branches_against_recorded_reference_gradients():
    """|a| = 1e-7 and a quaternion of angle 4e-7 (the Taylor branch), matrices with _sqrt_positive_part arguments <= 0 (no
    gradient through them), w < 0 (standardize_quaternion and quaternion_multiply pass -1): against the reference's own float64
    gradients in g11 (recorded on these float32 inputs)."""
    g11 = load_golden("g11_geometry_grad")
    sp = G.special_inputs()
    for key, (operands, gk) in G.SPECIAL_CASES.items():
        xs = [shaped(o, sp[o]) for o in operands]
        leaves = [dev(a).requires_grad_(True) for a in xs]
        out = call(key, leaves)
        assert out.grad_fn is not None
        out.backward(dev(sp[gk]).reshape(out.shape))
        refs = [g11[f"special/grad/{key}/{i}"].reshape(a.shape) for i, a in enumerate(xs)]
        assert all(np.all(np.isfinite(host(t.grad))) for t in leaves), key
        check(key, [t.grad for t in leaves], refs, f"{key} special branch")
    # m2q: only the diagonal carries gradient, and a radicand <= 0 contributes none: rows 0-3 have three radicands at 0
    t = dev(sp["R"]).requires_grad_(True)
    RC().matrix_to_quaternion(t)[:, 0].sum().backward()
    assert float(t.grad.abs().max()) == 0.0


def test_second_order_request_raises_and_no_grad_builds_no_graph():
    x = G.rotation_inputs("geom_grad/rot/257", 257)
    t = dev(x["aa"]).requires_grad_(True)
    R = RC().axis_angle_to_matrix(t)
    (g,) = torch.autograd.grad(R.sum(), t, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with torch.no_grad():
        assert RC().axis_angle_to_matrix(t).grad_fn is None
    assert RC().axis_angle_to_matrix(t.detach()).grad_fn is None
    # the Rodrigues and landmark Functions likewise
    from msmd_amd import ops
    from msmd_amd.utils.lbs import batch_rodrigues
    (g,) = torch.autograd.grad(batch_rodrigues(t).sum(), t, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    v = torch.randn(2, 9, 3, device=DEV, requires_grad=True)
    faces = torch.tensor([[0, 1, 2], [3, 4, 8]], device=DEV, dtype=torch.int32)
    idx = torch.tensor([0, 1, 1], device=DEV, dtype=torch.int32)
    bary = torch.full((3, 3), 1.0 / 3.0, device=DEV)
    (g,) = torch.autograd.grad(ops.landmarks(v, faces, idx, bary).square().sum(), v, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with torch.no_grad():
        assert ops.landmarks(v, faces, idx, bary).grad_fn is None and batch_rodrigues(t).grad_fn is None
    with pytest.raises(ValueError):      # more landmarks per frame than the backward kernel takes: refused at the forward
        ops.landmarks(v, faces, torch.zeros(1025, device=DEV, dtype=torch.int32), torch.full((1025, 3), 1.0 / 3.0, device=DEV))


# ----------------------------------------------------------------------------- 2. Rodrigues
@pytest.mark.parametrize("n", G.SIZES)
def test_batch_rodrigues_gradient_against_float64(n):
    from msmd_amd.utils.lbs import batch_rodrigues
    r, g = G.rodrigues_inputs(f"geom_grad/rod/{n}", n)
    t = dev(r).requires_grad_(True)
    R = batch_rodrigues(t)
    assert R.grad_fn is not None
    R.backward(dev(g))
    check("rodrigues", [t.grad], G.vjp(G.rodrigues, [r], g), f"rodrigues n={n}")
    assert torch.equal(R.detach(), batch_rodrigues(t.detach()))


def test_batch_rodrigues_gradient_at_zero_and_tiny_angles_matches_recorded_reference():
    """r = 0 and |r| = 1e-7 among ordinary angles, against the reference's recorded float64 gradient: finite, and within the op's
    bound in the usual measure, |g - g64| / max(1, |g64_item|_inf) <= c_op u.  At these two items the 1e-8 inside the norm decides
    the result (angle = |r + 1e-8| while the direction is r / angle).  Then 2000 vectors with |r| from 1e-9 to 1e-3 against float64
    autograd of the restatement, same bound: the VJP takes 1 - cos(angle) as 2 sin^2(angle / 2), so nothing cancels there (the
    float32 torch-CPU autograd of the formula as written reaches 8 500 u at |r| = 2.5e-4)."""
    from msmd_amd.utils.lbs import batch_rodrigues
    g11 = load_golden("g11_geometry_grad")
    r, g, ref = g11["rod/r"], g11["rod/g"], g11["rod/grad"]
    assert not r[0].any() and abs(np.linalg.norm(r[1].astype(np.float64)) - 1e-7) < 1e-9
    t = dev(r).requires_grad_(True)
    batch_rodrigues(t).backward(dev(g))
    assert np.all(np.isfinite(host(t.grad)))
    err = G.item_error(host(t.grad), ref).max(1)
    print(f"rodrigues recorded items: r = 0 {err[0]:.2f} u, |r| = 1e-7 {err[1]:.2f} u, all {err.max():.2f} u")
    check("rodrigues", [t.grad], [ref], "rodrigues r = 0, |r| = 1e-7 and recorded angles")
    gen = G.rng("geom_grad/rod/tiny")
    r = (G._unit(gen, 2000, 3) * 10.0 ** gen.uniform(-9.0, -3.0, (2000, 1))).astype(np.float32)
    g = gen.standard_normal((2000, 3, 3)).astype(np.float32)
    t = dev(r).requires_grad_(True)
    batch_rodrigues(t).backward(dev(g))
    check("rodrigues", [t.grad], G.vjp(G.rodrigues, [r], g), "rodrigues |r| in [1e-9, 1e-3]")


# ----------------------------------------------------------------------------- 3. landmarks
def lmk_tables(g, V, F, B, L):
    faces = g.integers(0, V, (F, 3)).astype(np.int32)
    faces[0] = [V - 1, 0, V - 1]
    idx_s = g.integers(0, F, L).astype(np.int32)
    idx_s[::7] = 0
    idx_b = g.integers(0, F, (B, L)).astype(np.int32)
    bc_s = g.uniform(0.05, 1.0, (L, 3)).astype(np.float32)
    bc_b = g.uniform(-0.2, 1.0, (B, L, 3)).astype(np.float32)
    return faces, idx_s, idx_b, bc_s, bc_b


def lmk_ref(gl, faces, idx, bc, V):
    """float64 scatter and, per vertex element, the number of contributions and the sum of their magnitudes."""
    B, L, _ = gl.shape
    fi = faces[np.broadcast_to(idx, (B, L))]                                       # (B, L, 3)
    w = np.broadcast_to(bc, (B, L, 3)).astype(np.float64)
    contrib = gl.astype(np.float64)[:, :, None, :] * w[..., None]                  # (B, L, corner, xyz)
    gv, mag, cnt = np.zeros((B, V, 3)), np.zeros((B, V, 3)), np.zeros((B, V, 1))
    bi = np.broadcast_to(np.arange(B)[:, None, None], fi.shape)
    np.add.at(gv, (bi, fi), contrib)
    np.add.at(mag, (bi, fi), np.abs(contrib))
    np.add.at(cnt, (bi, fi), 1.0)
    return gv, mag, cnt


def check_landmarks_bwd(what, V, faces, idx, bc, verts, gl, prev):
    """ops.landmarks under autograd and ops.landmarks_bwd directly on one set of tables: forward bits unchanged by requires_grad;
    |err| <= (cnt + 1) u sum |w g| per vertex element (a sum of cnt products in a fixed order); vertices no landmark touches
    exactly 0; a second run bit-equal; accumulate = 1 adds into an existing gradient (one more rounding) and leaves untouched
    vertices as they were."""
    from msmd_amd import ops
    L = idx.shape[-1]
    ref, mag, cnt = lmk_ref(gl, faces, idx, bc, V)
    tv = dev(verts).requires_grad_(True)
    out = ops.landmarks(tv, dev(faces), dev(idx), dev(bc))
    assert out.grad_fn is not None, what
    assert torch.equal(out.detach(), ops.landmarks(tv.detach(), dev(faces), dev(idx), dev(bc))), what
    out.backward(dev(gl))
    got = host(tv.grad)
    untouched = np.broadcast_to(cnt == 0, got.shape)
    assert np.all(got[untouched] == 0.0), what
    assert np.all(np.abs(got - ref) <= (cnt + 1) * U * mag), (what, float(np.abs(got - ref).max()))
    idx2 = dev(idx).reshape(-1, L)
    bc2 = dev(bc).reshape(-1, L, 3)
    again = ops.landmarks_bwd(dev(gl), dev(faces), idx2, bc2, V)
    assert torch.equal(again, tv.grad), what
    acc = dev(prev).clone()
    ops.landmarks_bwd(dev(gl), dev(faces), idx2, bc2, V, out=acc)
    a = host(acc)
    p64 = prev.astype(np.float64)
    assert np.all(a[untouched] == p64[untouched]), what
    assert np.all(np.abs(a - (ref + p64)) <= (cnt + 2) * U * (mag + np.abs(p64))), what
    return int(cnt.max())


@pytest.mark.parametrize("V", [3, 130, 5023])
def test_landmarks_backward_scatter_is_exact_in_structure_and_deterministic(V):
    """Random tables: shared and per-frame face ids and barycentrics, a table in which every landmark uses the same face (worst-case
    collisions), frame counts around 16 and 256, L up to 257; accumulate 0 and 1 (see check_landmarks_bwd)."""
    for B, L in ((1, 68), (15, 68), (16, 68), (17, 68), (257, 7), (3, 257)):
        g = G.rng(f"geom_grad/lmk/{V}/{B}/{L}")
        faces, idx_s, idx_b, bc_s, bc_b = lmk_tables(g, V, 97, B, L)
        same = np.full(L, 5, np.int32)
        verts = (0.3 * g.standard_normal((B, V, 3))).astype(np.float32)
        gl = g.standard_normal((B, L, 3)).astype(np.float32)
        prev = g.standard_normal((B, V, 3)).astype(np.float32)
        for idx, bc in ((idx_s, bc_s), (idx_b, bc_b), (idx_s, bc_b), (idx_b, bc_s), (same, bc_s)):
            check_landmarks_bwd((V, B, L, idx.ndim, bc.ndim), V, faces, idx, bc, verts, gl, prev)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 79])
def test_landmarks_backward_on_flame_tables(B):
    """FLAME's own tables from synth.flame_asset() on its 9976 faces at V = 5023: the shared 68 full landmarks (seletec_3d68 /
    landmarks3d) and the per-frame 2-D set FLAME.forward builds -- 17 contour landmarks from a per-frame row of the dynamic
    tables (every one of the 79 rows is used at B = 79) followed by the 51 static ones -- with the same per-element bound,
    exact zeros, bit-equal second run and accumulate 0 / 1 as on the random tables."""
    a = synth.flame_asset()
    lm = a["lmk"]
    faces = a["f"].astype(np.int32)
    V = a["v_template"].shape[0]
    g = G.rng(f"geom_grad/lmk_flame/{B}")
    verts = (0.1 * g.standard_normal((B, V, 3))).astype(np.float32)
    gl = g.standard_normal((B, 68, 3)).astype(np.float32)
    prev = g.standard_normal((B, V, 3)).astype(np.float32)
    full_idx = lm["full_lmk_faces_idx"].astype(np.int32).reshape(68)
    full_bc = lm["full_lmk_bary_coords"].astype(np.float32).reshape(68, 3)
    check_landmarks_bwd(("full", B), V, faces, full_idx, full_bc, verts, gl, prev)
    row = g.permutation(79)[:B]
    idx = np.concatenate([lm["dynamic_lmk_faces_idx"][row], np.broadcast_to(lm["static_lmk_faces_idx"], (B, 51))], 1).astype(np.int32)
    bc = np.concatenate([lm["dynamic_lmk_bary_coords"][row], np.broadcast_to(lm["static_lmk_bary_coords"], (B, 51, 3))],
                        1).astype(np.float32)
    assert idx.shape == (B, 68) and bc.shape == (B, 68, 3)
    check_landmarks_bwd(("contour + static", B), V, faces, idx, bc, verts, gl, prev)
    check_landmarks_bwd(("contour + static ids, shared full barycentrics", B), V, faces, idx, full_bc, verts, gl, prev)


# ----------------------------------------------------------------------------- 4. FLAME end to end
def flame_model(V):
    from msmd_amd.utils.flame import FLAME, FLAMEConfig
    a = synth.flame_asset()
    if V != a["v_template"].shape[0]:
        a = dict(a)
        jr = a["J_regressor"][:, :V] + 1e-3
        a.update(v_template=a["v_template"][:V], shapedirs=a["shapedirs"][:V], posedirs=a["posedirs"][:V],
                 J_regressor=(jr / jr.sum(1, keepdims=True)).astype(np.float32), weights=a["weights"][:V],
                 f=(a["f"].astype(np.int64) % V).astype(np.uint32))
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = a
    return FLAME(cfg).to(DEV)


@pytest.mark.parametrize("V", [5023, 130])
@pytest.mark.parametrize("pose2rot", [True, False])
def test_flame_forward_gradients_end_to_end(V, pose2rot):
    """FLAME.forward(shape, exp, pose, return_lm2d=True, return_lm3d=True) with all three inputs requiring grad; loss = a
    weighted sum of the vertices and both landmark sets; gradients against the float64 chain (lbs + landmark gather, the
    contour rows as the device picked them).  Bound, per gradient tensor: |g - g64| <= 1e-3 max |g64|.  Reasoning: the chain
    runs in fp32 throughout -- the skinning forward keeps p to 5e-6 on |v| ~ 0.1 (5e-5 relative, tests/test_geometry_gpu.py),
    the backward contraction accumulates 3 Vp ~ 15 000 fp32 products ((K / 4 + 8) u = 2.2e-4 of sum |terms| worst case) -- so
    a correct chain sits well inside 1e-3, while a dropped landmark set or a cut branch moves a gradient by O(1) of its size
    (the landmark weights are scaled so that each set contributes as much as the vertices)."""
    from msmd_amd import ops
    fl = flame_model(V)
    B = 19
    g = G.rng(f"geom_grad/flame/{V}/{pose2rot}")
    shape = (0.5 * g.standard_normal((B, 100))).astype(np.float32)
    exp = (0.5 * g.standard_normal((B, 50))).astype(np.float32)
    pose6 = (0.3 * g.standard_normal((B, 6))).astype(np.float32)
    if pose2rot:
        pose = pose6
    else:
        pose = G.rodrigues(torch.from_numpy(pose6.reshape(-1, 3)).double()).numpy().astype(np.float32).reshape(B, 18)
    gv = g.standard_normal((B, V, 3)).astype(np.float32)
    g2 = (V / 68.0 * g.standard_normal((B, 68, 3))).astype(np.float32)
    g3 = (V / 68.0 * g.standard_normal((B, 68, 3))).astype(np.float32)
    ts, te, tp = (dev(a).requires_grad_(True) for a in (shape, exp, pose))
    v, l2, l3 = fl(ts, te, tp, pose2rot=pose2rot, return_lm2d=True, return_lm3d=True)
    assert v.grad_fn is not None and l2.grad_fn is not None and l3.grad_fn is not None
    ((v * dev(gv)).sum() + (l2 * dev(g2)).sum() + (l3 * dev(g3)).sum()).backward()
    with torch.no_grad():
        v0, l20, l30 = fl(ts, te, tp, pose2rot=pose2rot, return_lm2d=True, return_lm3d=True)
        assert v0.grad_fn is None and l20.grad_fn is None
    assert torch.equal(l2.detach(), ops.landmarks(v.detach(), fl._pack()["faces"], *contour(fl, tp.detach(), pose2rot, B)))
    # float64 chain
    m = dict(v_template=fl.v_template.double().cpu(), shapedirs=fl.shapedirs.double().cpu(), posedirs=fl.posedirs.double().cpu(),
             J_regressor=fl.J_regressor.double().cpu(), weights=fl.lbs_weights.double().cpu(),
             parents=[int(p) for p in fl.parents.cpu()])
    faces = fl.faces_tensor.cpu()
    idx2, bary2 = contour(fl, tp.detach(), pose2rot, B)
    idx2, bary2 = idx2.long().cpu(), bary2.double().cpu()
    full_idx, full_bary = fl.full_lmk_faces_idx.cpu().reshape(-1), fl.full_lmk_bary_coords.double().cpu().reshape(-1, 3)
    w = 3 if pose2rot else 9
    ident = torch.zeros(B, 3).double() if pose2rot else torch.eye(3).double().reshape(1, 9).expand(B, -1)

    def chain(s, e, p):
        full = torch.cat([p[:, :w], ident, p[:, w:], ident, ident], 1)
        vv = G.lbs(m, torch.cat([s, e], 1), full, pose_is_matrix=not pose2rot)
        return ((vv * torch.from_numpy(gv).double()).sum() + (G.landmarks(vv, faces, idx2, bary2) * torch.from_numpy(g2).double()).sum()
                + (G.landmarks(vv, faces, full_idx, full_bary) * torch.from_numpy(g3).double()).sum())
    refs = G.vjp(chain, [shape, exp, pose], np.ones(()))
    for name, t, r in zip(("shape", "exp", "pose"), (ts, te, tp), refs):
        assert t.grad is not None and t.grad.shape == r.shape, name
        rel = float(np.abs(host(t.grad) - r).max() / np.abs(r).max())
        print(f"FLAME V={V} pose2rot={pose2rot} d{name}: max error {rel:.2e} of max |g| (bound 1e-3)")
        assert rel <= 1e-3, (name, rel)


def contour(fl, pose, pose2rot, B):
    """The per-frame 2-D landmark tables as FLAME.forward builds them (contour rows picked by the device)."""
    from msmd_amd import ops
    p = fl._pack()
    if pose2rot:
        z = torch.zeros(B, 3, device=DEV)
        full = torch.cat([pose[:, :3], z, pose[:, 3:], z, z], 1).contiguous()
    else:
        eye = torch.eye(3, device=DEV).reshape(1, 9).expand(B, -1)
        full = torch.cat([pose[:, :9], eye, pose[:, 9:], eye, eye], 1).contiguous()
    row = ops.dynamic_lmk_row(full, p["chain"], pose_is_matrix=not pose2rot).long()
    idx = torch.cat([p["dyn_idx"][row], p["static_idx"].unsqueeze(0).expand(B, -1)], 1).contiguous()
    bary = torch.cat([fl.dynamic_lmk_bary_coords[row], fl.lmk_bary_coords.unsqueeze(0).expand(B, -1, -1)], 1).contiguous()
    return idx, bary


def test_public_lbs_and_landmark_helpers_carry_gradients():
    """utils.lbs.lbs(...) with grad-requiring betas / pose returns vertices (and joints) with a grad_fn whose gradients match
    the float64 chain; FLAME.seletec_3d68 and utils.lbs.vertices2landmarks carry the gradient to the vertices."""
    from msmd_amd.utils.lbs import lbs, vertices2landmarks
    fl = flame_model(5023)
    B = 5
    g = G.rng("geom_grad/public_lbs")
    betas = (0.5 * g.standard_normal((B, 150))).astype(np.float32)
    pose = (0.3 * g.standard_normal((B, 15))).astype(np.float32)
    gv = g.standard_normal((B, 5023, 3)).astype(np.float32)
    tb, tp = dev(betas).requires_grad_(True), dev(pose).requires_grad_(True)
    v, joints = lbs(tb, tp, fl.v_template, fl.shapedirs, fl.posedirs, fl.J_regressor, fl.parents, fl.lbs_weights)
    assert v.grad_fn is not None and joints.shape == (B, 5, 3)
    v0, j0 = lbs(tb.detach(), tp.detach(), fl.v_template, fl.shapedirs, fl.posedirs, fl.J_regressor, fl.parents, fl.lbs_weights)
    assert v0.grad_fn is None and float((v.detach() - v0).abs().max()) <= 1e-5 and float((joints.detach() - j0).abs().max()) <= 1e-5
    v.backward(dev(gv))
    m = dict(v_template=fl.v_template.double().cpu(), shapedirs=fl.shapedirs.double().cpu(), posedirs=fl.posedirs.double().cpu(),
             J_regressor=fl.J_regressor.double().cpu(), weights=fl.lbs_weights.double().cpu(),
             parents=[int(p) for p in fl.parents.cpu()])
    rb, rp = G.vjp(lambda b, p: G.lbs(m, b, p), [betas, pose], gv)
    for t, r in ((tb, rb), (tp, rp)):
        assert float(np.abs(host(t.grad) - r).max() / np.abs(r).max()) <= 1e-3
    tv = v0.clone().requires_grad_(True)
    l3 = fl.seletec_3d68(tv)
    assert l3.grad_fn is not None
    l3.sum().backward()
    assert tv.grad is not None and float(tv.grad.abs().sum()) > 0
    tv2 = v0.clone().requires_grad_(True)
    l = vertices2landmarks(tv2, fl.faces_tensor, fl.full_lmk_faces_idx.reshape(-1), fl.full_lmk_bary_coords.reshape(-1, 3))
    assert l.grad_fn is not None
    l.sum().backward()
    assert torch.equal(tv2.grad, tv.grad)
