"""Torch restatements of the geometry surface (utils/rotation_conversions.py, utils/lbs.py's batch_rodrigues, landmark
gather and LBS chain), written from the formulas (PyTorch3D / SMPL-X conventions) so that torch.autograd on them is the truth
for the HIP backward kernels: in float64 the reference gradient, in float32 the yardstick the tolerances are set against.
Nothing here touches the package's kernels.  The branch idioms are chosen so that autograd differentiates the branch taken:
`where` over a guarded denominator for the small-angle Taylor branch, a masked square root with zero gradient at arguments
<= 0, sign factors for _copysign / standardize_quaternion, torch's norm (gradient 0 at 0), a clamped norm for F.normalize.

Also here: the deterministic input generators of the gradient tests and the conditioning predicates they are held to."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # `python tests/geometry_grad_ref.py`

from msmd_amd import synth  # noqa: E402

CONVENTIONS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX", "XYX", "XZX", "YXY", "YZY", "ZXZ", "ZYZ")
U = 2.0 ** -24


# ----------------------------------------------------------------------------- the 16 conversions
def q2m(q):
    r, i, j, k = torch.unbind(q, -1)
    s = 2.0 / (q * q).sum(-1)
    o = torch.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                     s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                     s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def _sqrt_pos(x):
    pos = x > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def _sign_of(b):
    """+-1 as a constant: _copysign(a, b) for a >= 0 is a * sign, with no gradient to b."""
    return torch.where(b.detach() < 0, -torch.ones_like(b), torch.ones_like(b)).detach()


def m2q(m):
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    return torch.stack([0.5 * _sqrt_pos(1 + m00 + m11 + m22),
                        0.5 * _sqrt_pos(1 + m00 - m11 - m22) * _sign_of(m[..., 2, 1] - m[..., 1, 2]),
                        0.5 * _sqrt_pos(1 - m00 + m11 - m22) * _sign_of(m[..., 0, 2] - m[..., 2, 0]),
                        0.5 * _sqrt_pos(1 - m00 - m11 + m22) * _sign_of(m[..., 1, 0] - m[..., 0, 1])], -1)


def _soa(angle, half):
    """sin(half) / angle, 0.5 - angle^2 / 48 below |angle| = 1e-6."""
    small = angle.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(angle), angle)
    return torch.where(small, 0.5 - angle * angle / 48, torch.sin(half) / safe)


def aa2q(a):
    angle = torch.linalg.norm(a, dim=-1, keepdim=True)
    half = 0.5 * angle
    return torch.cat([torch.cos(half), a * _soa(angle, half)], -1)


def q2aa(q):
    n = torch.linalg.norm(q[..., 1:], dim=-1, keepdim=True)
    half = torch.atan2(n, q[..., :1])
    return q[..., 1:] / _soa(2 * half, half)


def aa2m(a):
    return q2m(aa2q(a))


def m2aa(m):
    return q2aa(m2q(m))


def _normalize(x):
    return x / torch.linalg.norm(x, dim=-1, keepdim=True).clamp_min(1e-12)


def d62m(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = _normalize(a1)
    b2 = _normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1)
    return torch.stack([b1, b2, torch.linalg.cross(b1, b2, dim=-1)], -2)


def m2d6(m):
    return m[..., :2, :].reshape(m.shape[:-2] + (6,))


def aa2d6(a):
    return m2d6(aa2m(a))


def _axis(axis, a):
    c, s, one, z = torch.cos(a), torch.sin(a), torch.ones_like(a), torch.zeros_like(a)
    R = {"X": (one, z, z, z, c, -s, z, s, c), "Y": (c, z, s, z, one, z, -s, z, c), "Z": (c, -s, z, s, c, z, z, z, one)}[axis]
    return torch.stack(R, -1).reshape(a.shape + (3, 3))


def e2m(e, conv):
    return _axis(conv[0], e[..., 0]) @ _axis(conv[1], e[..., 1]) @ _axis(conv[2], e[..., 2])


def m2e(m, conv):
    def tan(axis, other, data, horizontal, tb):
        i1, i2 = {"X": (2, 1), "Y": (0, 2), "Z": (1, 0)}[axis]
        if horizontal:
            i1, i2 = i2, i1
        if horizontal == ((axis + other) in ("XY", "YZ", "ZX")):
            return torch.atan2(data[..., i1], data[..., i2])
        return torch.atan2(-data[..., i2], data[..., i1]) if tb else torch.atan2(data[..., i2], -data[..., i1])
    i0, i2 = "XYZ".index(conv[0]), "XYZ".index(conv[2])
    tb = i0 != i2
    central = torch.asin(m[..., i0, i2] * (-1.0 if i0 - i2 in (-1, 2) else 1.0)) if tb else torch.acos(m[..., i0, i0])
    return torch.stack([tan(conv[0], conv[1], m[..., i2], False, tb), central, tan(conv[2], conv[1], m[..., i0, :], True, tb)], -1)


def qstd(q):
    return q * _sign_of(q[..., :1])


def qinv(q):
    return q * q.new_tensor([1.0, -1.0, -1.0, -1.0])


def qraw(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def qmul(a, b):
    return qstd(qraw(a, b))


def qapply(q, p):
    pq = torch.cat([torch.zeros_like(p[..., :1]), p], -1)
    return qraw(qraw(q, pq), qinv(q))[..., 1:]


# op key -> (restatement, public function name, generator keys of its operands).  Euler ops take the convention.
OPS = {
    "q2m": (q2m, "quaternion_to_matrix", ("qs",)),
    "m2q": (m2q, "matrix_to_quaternion", ("R",)),
    "aa2q": (aa2q, "axis_angle_to_quaternion", ("aa",)),
    "q2aa": (q2aa, "quaternion_to_axis_angle", ("qs",)),
    "aa2m": (aa2m, "axis_angle_to_matrix", ("aa",)),
    "m2aa": (m2aa, "matrix_to_axis_angle", ("R",)),
    "d62m": (d62m, "rotation_6d_to_matrix", ("d6",)),
    "m2d6": (m2d6, "matrix_to_rotation_6d", ("R",)),
    "aa2d6": (aa2d6, "axis_angle_to_rotation_6d", ("aa",)),
    "qstd": (qstd, "standardize_quaternion", ("qa",)),
    "qinv": (qinv, "quaternion_invert", ("qa",)),
    "qraw": (qraw, "quaternion_raw_multiply", ("qa", "qb")),
    "qmul": (qmul, "quaternion_multiply", ("qa", "qb")),
    "qapply": (qapply, "quaternion_apply", ("qa", "pts")),
}
EULER_OPS = {"e2m": (e2m, "euler_angles_to_matrix"), "m2e": (m2e, "matrix_to_euler_angles")}


# ----------------------------------------------------------------------------- FLAME pieces
def rodrigues(r):
    """utils/lbs.py's batch_rodrigues: angle = |r + 1e-8|, direction = r / angle (the un-shifted r)."""
    angle = torch.linalg.norm(r + 1e-8, dim=1, keepdim=True)
    d = r / angle
    s, c1 = torch.sin(angle)[:, :, None], (1 - torch.cos(angle))[:, :, None]
    z = torch.zeros_like(d[:, 0])
    K = torch.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
    return torch.eye(3, dtype=r.dtype)[None] + s * K + c1 * (K @ K)


def landmarks(verts, faces, idx, bary):
    """verts (B, V, 3); faces (F, 3) long; idx (L,) or (B, L) long; bary (L, 3) or (B, L, 3) -> (B, L, 3)."""
    B = verts.shape[0]
    fi = faces[idx.expand(B, -1) if idx.dim() == 2 else idx[None].expand(B, -1)]              # (B, L, 3)
    corners = verts[torch.arange(B)[:, None, None], fi]                                        # (B, L, 3 corners, 3)
    w = bary.expand(B, -1, -1) if bary.dim() == 3 else bary[None].expand(B, -1, -1)
    return (corners * w[..., None]).sum(2)


def lbs(m, betas, pose, pose_is_matrix=False):
    """utils/lbs.py:141-223: v = sum_j w_j (R_j p + t_j), p = template + sum_k coef_k dirs_k, coef = [betas | R[1:] - I].
    m: dict of tensors v_template (V, 3), shapedirs (V, 3, NB), posedirs (P, V * 3), J_regressor (J, V), weights (V, J) and
    the python list parents."""
    B, NB = betas.shape
    V = m["v_template"].shape[0]
    J = m["J_regressor"].shape[0]
    v_shaped = m["v_template"][None] + (betas @ m["shapedirs"].reshape(V * 3, NB).T).reshape(B, V, 3)
    joints = torch.einsum("jv,bvc->bjc", m["J_regressor"], v_shaped)
    R = pose.reshape(B, J, 3, 3) if pose_is_matrix else rodrigues(pose.reshape(B * J, 3)).reshape(B, J, 3, 3)
    pf = (R[:, 1:] - torch.eye(3, dtype=R.dtype)).reshape(B, (J - 1) * 9)
    p = v_shaped + (pf @ m["posedirs"]).reshape(B, V, 3)
    par = m["parents"]
    wR, wt = [R[:, 0]], [joints[:, 0]]
    for i in range(1, J):
        wR.append(wR[par[i]] @ R[:, i])
        wt.append(torch.einsum("brc,bc->br", wR[par[i]], joints[:, i] - joints[:, par[i]]) + wt[par[i]])
    A = torch.stack([torch.cat([wR[i], (wt[i] - torch.einsum("brc,bc->br", wR[i], joints[:, i]))[:, :, None]], 2)
                     for i in range(J)], 1)
    T = torch.einsum("vj,bjk->bvk", m["weights"], A.reshape(B, J, 12)).reshape(B, V, 3, 4)
    return torch.einsum("bvrc,bvc->bvr", T[..., :3], p) + T[..., 3]


# ----------------------------------------------------------------------------- autograd helpers
def vjp(fn, xs, g, dtype=torch.float64):
    """Gradients of sum(fn(*xs) * g) by torch autograd on the CPU in `dtype`; xs / g numpy arrays -> list of float64 arrays."""
    ts = [torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True) for x in xs]
    out = fn(*ts)
    out.backward(torch.from_numpy(np.ascontiguousarray(g)).to(dtype).reshape(out.shape))
    return [t.grad.double().numpy() for t in ts]


def item_error(got, ref):
    """|got - ref| / max(1, |ref_item|_inf) in units of u, per element; items along axis 0."""
    n = ref.shape[0]
    scale = np.maximum(1.0, np.abs(ref.reshape(n, -1)).max(1)).reshape((n,) + (1,) * (ref.ndim - 1))
    return np.abs(np.asarray(got, np.float64) - ref) / scale / U


# ----------------------------------------------------------------------------- conditioned inputs
def rng(tag):
    return np.random.default_rng(synth.name_seed(tag) & 0xFFFFFFFF)


def _unit(g, n, k):
    x = g.standard_normal((n, k))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _draw(g, n, make, keep):
    """n rows of make(count) that satisfy keep (rejection sampling in deterministic blocks)."""
    rows = []
    have = 0
    while have < n:
        x = make(2 * n + 64)
        x = x[keep(x)]
        rows.append(x)
        have += len(x)
    return np.concatenate(rows)[:n]


def rotation_inputs(tag, n):
    """float32 operands of the 14 non-Euler ops (see `predicates`) and one upstream gradient per output width."""
    g = rng(tag)
    # unit quaternions with every |component| >= 0.12: matrix_to_quaternion's radicands 4 q_i^2 >= 0.0576, rotation angle
    # 2 atan2(|v|, w) in [0.41, 2.9]; real part made positive so the angle is the principal one
    q = _draw(g, n, lambda c: _unit(g, c, 4), lambda x: np.all(np.abs(x) >= 0.12, 1))
    q = q * np.where(q[:, :1] < 0, -1.0, 1.0)
    qs = q * g.uniform(0.5, 2.0, (n, 1))
    aa = _unit(g, n, 3) * g.uniform(0.05, math.pi - 0.1, (n, 1))

    def d6_ok(x):
        a1, a2 = x[:, :3], x[:, 3:]
        n1, n2 = np.linalg.norm(a1, axis=1), np.linalg.norm(a2, axis=1)
        sin = np.linalg.norm(np.cross(a1, a2), axis=1) / (n1 * n2)
        return (n1 >= 0.1) & (sin >= 0.1)
    d6 = _draw(g, n, lambda c: g.standard_normal((c, 6)), d6_ok)
    qa = _unit(g, n, 4) * g.uniform(0.5, 2.0, (n, 1))
    qb = _unit(g, n, 4) * g.uniform(0.5, 2.0, (n, 1))
    pts = 2.0 * g.standard_normal((n, 3))
    R = q2m(torch.from_numpy(q)).numpy()
    x = dict(qs=qs, aa=aa, d6=d6, qa=qa, qb=qb, pts=pts, R=R)
    x = {k: v.astype(np.float32) for k, v in x.items()}
    for w in (3, 4, 6, 9):
        x[f"g{w}"] = g.standard_normal((n, w)).astype(np.float32)
    return x


def euler_inputs(tag, n, conv):
    """float32 (angles, matrices built from them in float64, gradients): outer angles in (-3, 3); central angle with
    |cos| >= 0.1, inside asin's range for Tait-Bryan conventions, and for proper Euler conventions (acos of the central entry,
    atan2 pairs of length |sin|) also |sin| >= 0.1."""
    g = rng(f"{tag}/{conv}")
    e = g.uniform(-3.0, 3.0, (n, 3))
    lim = math.acos(0.1)
    if conv[0] != conv[2]:
        e[:, 1] = g.uniform(-lim, lim, n)
    else:
        lo = math.asin(0.1)
        c = g.uniform(lo, math.pi - lo - 2 * (math.pi / 2 - lim), n)      # (lo, pi - lo) minus the band |cos| < 0.1
        e[:, 1] = np.where(c > lim, c + 2 * (math.pi / 2 - lim), c)
    e = e.astype(np.float32)
    R = e2m(torch.from_numpy(e.astype(np.float64)), conv).numpy().astype(np.float32)
    return dict(e=e, R=R, g3=g.standard_normal((n, 3)).astype(np.float32), g9=g.standard_normal((n, 9)).astype(np.float32))


def predicates(x):
    """The conditioning every item of rotation_inputs must satisfy (asserted by the tests on ALL items, none left out)."""
    R = x["R"].astype(np.float64)
    d = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], 1)
    rad = np.stack([1 + d[:, 0] + d[:, 1] + d[:, 2], 1 + d[:, 0] - d[:, 1] - d[:, 2], 1 - d[:, 0] + d[:, 1] - d[:, 2],
                    1 - d[:, 0] - d[:, 1] + d[:, 2]], 1)
    qs = x["qs"].astype(np.float64)
    ang_q = 2 * np.arctan2(np.linalg.norm(qs[:, 1:], axis=1), qs[:, 0])
    ang_a = np.linalg.norm(x["aa"].astype(np.float64), axis=1)
    a1, a2 = x["d6"][:, :3].astype(np.float64), x["d6"][:, 3:].astype(np.float64)
    n1, n2 = np.linalg.norm(a1, axis=1), np.linalg.norm(a2, axis=1)
    sin = np.linalg.norm(np.cross(a1, a2), axis=1) / (n1 * n2)
    ok = np.all(rad >= 0.05, 1) & (n1 >= 0.1 - 1e-6) & (sin >= 0.1 - 1e-6)
    for a in (ang_q, ang_a):
        ok &= (a >= 0.05 - 1e-6) & (a <= math.pi - 0.1 + 1e-6)
    for k in ("qs", "qa", "qb"):
        nq = np.linalg.norm(x[k].astype(np.float64), axis=1)
        ok &= (nq >= 0.5 - 1e-6) & (nq <= 2.0 + 1e-6)
    return ok


def euler_predicate(xe, conv):
    c = xe["e"][:, 1].astype(np.float64)
    ok = np.abs(np.cos(c)) >= 0.1 - 1e-6
    if conv[0] == conv[2]:
        ok &= (np.abs(np.sin(c)) >= 0.1 - 1e-6) & (c > 0) & (c < math.pi)
    else:
        ok &= np.abs(c) < math.pi / 2
    return ok


def special_inputs():
    """The branches on their own (float32): |a| = 1e-7 axis-angles and quaternions of angle < 1e-6 (Taylor branch), matrices
    with a _sqrt_positive_part argument <= 0 (a half-turn about x: three radicands are exactly 0; the same with m22 pushed
    down: negative radicands), quaternions with w < 0."""
    g = rng("geom_grad/special")
    d = _unit(g, 8, 3)
    aa = (1e-7 * d).astype(np.float32)
    q_small = np.concatenate([np.ones((8, 1)), 2e-7 * d], 1).astype(np.float32)
    R = np.tile(np.diag([1.0, -1.0, -1.0]), (8, 1, 1))
    R[4:, 2, 2] = -1.0 - 0.01 * np.arange(1, 5)
    R[:, 2, 1] += 0.01 * g.standard_normal(8)
    R[:, 0, 2] += 0.01 * g.standard_normal(8)
    R[:, 1, 0] += 0.01 * g.standard_normal(8)
    q_neg = _unit(g, 8, 4)
    q_neg[:, 0] = -np.abs(q_neg[:, 0]) - 0.05
    x = dict(aa=aa, q_small=q_small, R=R.astype(np.float32), q_neg=q_neg.astype(np.float32), qb=_unit(g, 8, 4).astype(np.float32))
    for w in (3, 4, 6, 9):
        x[f"g{w}"] = g.standard_normal((8, w)).astype(np.float32)
    return x


# op key -> (operand keys in special_inputs(), gradient key): the special-branch cases
SPECIAL_CASES = {
    "aa2q": (("aa",), "g4"), "aa2m": (("aa",), "g9"), "aa2d6": (("aa",), "g6"), "q2aa": (("q_small",), "g3"),
    "m2q": (("R",), "g4"), "qstd": (("q_neg",), "g4"), "qmul": (("q_neg", "qb"), "g4"),
}


def out_width(key):
    return dict(q2m=9, m2q=4, aa2q=4, q2aa=3, aa2m=9, m2aa=3, d62m=9, m2d6=6, aa2d6=6, qstd=4, qinv=4, qraw=4, qmul=4,
                qapply=3, e2m=9, m2e=3)[key]


SIZES = (1, 255, 256, 257, 1000, 70001)


def rodrigues_inputs(tag, n):
    """float32 (r (n, 3) with angles in [0.05, pi - 0.1], upstream gradient (n, 3, 3))."""
    g = rng(tag)
    r = _unit(g, n, 3) * g.uniform(0.05, math.pi - 0.1, (n, 1))
    return r.astype(np.float32), g.standard_normal((n, 3, 3)).astype(np.float32)


# yardstick() as recorded (u): the GPU test's bounds are c_op = max(16, 4 x this); tests/test_geometry_grad_cpu.py re-measures it
YARDSTICK = dict(q2m=40.54, m2q=12.22, aa2q=4.00, q2aa=4.16, aa2m=16.66, m2aa=14.12, d62m=144.16, m2d6=0.0, aa2d6=11.75,
                 qstd=0.0, qinv=0.0, qraw=3.21, qmul=3.21, qapply=4.67, e2m=10.56, m2e=25.74, rodrigues=24.98)


def yardstick():
    """{op: max over SIZES of the per-item-normalised error (in u) of the float32 torch-CPU autograd of the restatement against
    its float64 autograd, same inputs}: the measure the GPU test's bounds c_op = max(16, 4 x yardstick) are set by."""
    res = {}

    def note(key, fn, xs, g):
        ref, y = vjp(fn, xs, g), vjp(fn, xs, g, torch.float32)
        res[key] = max(res.get(key, 0.0), max(float(item_error(a, b).max()) for a, b in zip(y, ref)))
    for n in SIZES:
        x = rotation_inputs(f"geom_grad/rot/{n}", n)
        for key, (fn, _, operands) in OPS.items():
            note(key, fn, [x[o] for o in operands], x[f"g{out_width(key)}"])
        for conv in CONVENTIONS:
            xe = euler_inputs(f"geom_grad/euler/{n}", n, conv)
            note("e2m", lambda e: e2m(e, conv), [xe["e"]], xe["g9"])
            note("m2e", lambda m: m2e(m, conv), [xe["R"]], xe["g3"])
        r, g = rodrigues_inputs(f"geom_grad/rod/{n}", n)
        note("rodrigues", rodrigues, [r], g)
    return res


if __name__ == "__main__":
    for k, v in yardstick().items():
        print(f"{k:10s} yardstick {v:8.2f} u   c_op {max(16.0, 4 * v):8.1f}")
