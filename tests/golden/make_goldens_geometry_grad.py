"""Records tests/golden/g11_geometry_grad.npz: inputs, upstream gradients and the REFERENCE implementation's own autograd
gradients (float64, CPU) of every rotation conversion (all 12 Euler conventions, both directions), batch_rodrigues,
vertices2landmarks and a small lbs + landmarks chain, plus the special-branch inputs of tests/geometry_grad_ref.py.

    python tests/golden/make_goldens_geometry_grad.py /path/to/reference/checkout

The reference's utils/rotation_conversions.py and utils/lbs.py are imported from that checkout at recording time only; the
archive holds data only.  tests/test_geometry_grad_cpu.py pins tests/geometry_grad_ref.py's restatements to these gradients."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import geometry_grad_ref as G  # noqa: E402

N_OP, N_EULER = 20, 8


def load(ref_root, name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref_root, "utils", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ref_vjp(fn, xs, g):
    ts = [torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(True) for x in xs]
    out = fn(*ts)
    out.backward(torch.from_numpy(np.ascontiguousarray(g)).double().reshape(out.shape))
    grads = [t.grad.numpy() for t in ts]
    assert all(np.all(np.isfinite(x)) for x in grads), "reference gradient not finite"
    return grads


def small_model(g, V, NB, J=5):
    m = dict(v_template=0.1 * g.standard_normal((V, 3)), shapedirs=0.01 * g.standard_normal((V, 3, NB)),
             posedirs=0.01 * g.standard_normal(((J - 1) * 9, V * 3)), J_regressor=np.abs(g.standard_normal((J, V))),
             weights=np.abs(g.standard_normal((V, J))) ** 2)
    m["J_regressor"] /= m["J_regressor"].sum(1, keepdims=True)
    m["weights"] /= m["weights"].sum(1, keepdims=True)
    return {k: v.astype(np.float32) for k, v in m.items()}


def main(ref_root):
    RC, LBS = load(ref_root, "rotation_conversions"), load(ref_root, "lbs")
    out = {}
    x = G.rotation_inputs("g11/ops", N_OP)
    assert G.predicates(x).all()
    for k, v in x.items():
        out[f"in/{k}"] = v
    for key, (_, name, operands) in G.OPS.items():
        grads = ref_vjp(getattr(RC, name), [x[o] for o in operands], x[f"g{G.out_width(key)}"])
        for i, gr in enumerate(grads):
            out[f"grad/{key}/{i}"] = gr
    for conv in G.CONVENTIONS:
        xe = G.euler_inputs("g11/euler", N_EULER, conv)
        assert G.euler_predicate(xe, conv).all()
        for k, v in xe.items():
            out[f"euler/{conv}/{k}"] = v
        out[f"grad/e2m/{conv}"] = ref_vjp(lambda e: RC.euler_angles_to_matrix(e, conv), [xe["e"]], xe["g9"])[0]
        out[f"grad/m2e/{conv}"] = ref_vjp(lambda m: RC.matrix_to_euler_angles(m, conv), [xe["R"]], xe["g3"])[0]
    sp = G.special_inputs()
    for k, v in sp.items():
        out[f"special/in/{k}"] = v
    for key, (operands, gk) in G.SPECIAL_CASES.items():
        grads = ref_vjp(getattr(RC, G.OPS[key][1]), [sp[o] for o in operands], sp[gk])
        for i, gr in enumerate(grads):
            out[f"special/grad/{key}/{i}"] = gr
    # batch_rodrigues: ordinary angles, r = 0 and |r| = 1e-7
    g = G.rng("g11/flame")
    r = (G._unit(g, 24, 3) * g.uniform(0.0, 3.0, (24, 1))).astype(np.float32)
    r[0] = 0.0
    r[1] *= 1e-7 / max(np.linalg.norm(r[1]), 1e-30)
    gR = g.standard_normal((24, 3, 3)).astype(np.float32)
    out["rod/r"], out["rod/g"] = r, gR
    out["rod/grad"] = ref_vjp(lambda t: LBS.batch_rodrigues(t, dtype=torch.float64), [r], gR)[0]
    # vertices2landmarks with per-frame tables and repeated faces; the reference adds the frame offset in place, hence clones
    B, V, F, L = 3, 40, 30, 9
    faces = g.integers(0, V, (F, 3)).astype(np.int64)
    idx = g.integers(0, F, (B, L)).astype(np.int64)
    idx[:, :3] = 4
    bary = g.uniform(0.0, 1.0, (B, L, 3)).astype(np.float32)
    verts = g.standard_normal((B, V, 3)).astype(np.float32)
    gl = g.standard_normal((B, L, 3)).astype(np.float32)
    out.update({"lmk/faces": faces, "lmk/idx": idx, "lmk/bary": bary, "lmk/verts": verts, "lmk/g": gl})
    out["lmk/grad"] = ref_vjp(lambda v: LBS.vertices2landmarks(v, torch.from_numpy(faces), torch.from_numpy(idx),
                                                               torch.from_numpy(bary).double()), [verts], gl)[0]
    # lbs + landmarks chain, axis-angle and matrix poses
    V, NB, Bc = 16, 6, 3
    m = small_model(g, V, NB)
    parents = np.array([-1, 0, 1, 1, 1], np.int64)
    betas = (0.5 * g.standard_normal((Bc, NB))).astype(np.float32)
    pose = (0.4 * g.standard_normal((Bc, 15))).astype(np.float32)
    cf = g.integers(0, V, (12, 3)).astype(np.int64)
    ci = g.integers(0, 12, (5,)).astype(np.int64)
    cb = g.uniform(0.0, 1.0, (5, 3)).astype(np.float32)
    gv = g.standard_normal((Bc, V, 3)).astype(np.float32)
    gl = g.standard_normal((Bc, 5, 3)).astype(np.float32)
    for k, v in m.items():
        out[f"chain/m/{k}"] = v
    out.update({"chain/parents": parents, "chain/betas": betas, "chain/pose": pose, "chain/faces": cf, "chain/idx": ci,
                "chain/bary": cb, "chain/gv": gv, "chain/gl": gl})
    md = {k: torch.from_numpy(v).double() for k, v in m.items()}

    def chain(pose2rot):
        def f(b, p):
            v, _ = LBS.lbs(b, p, md["v_template"][None], md["shapedirs"], md["posedirs"], md["J_regressor"],
                           torch.from_numpy(parents), md["weights"], pose2rot=pose2rot, dtype=torch.float64)
            lm = LBS.vertices2landmarks(v, torch.from_numpy(cf), torch.from_numpy(ci).repeat(Bc),
                                        torch.from_numpy(cb).double()[None].expand(Bc, -1, -1))
            return (v * torch.from_numpy(gv).double()).sum() + (lm * torch.from_numpy(gl).double()).sum()
        return f
    ga = ref_vjp(chain(True), [betas, pose], np.ones(()))
    out["chain/grad/betas"], out["chain/grad/pose"] = ga
    mats = G.rodrigues(torch.from_numpy(pose).double().reshape(-1, 3)).numpy().astype(np.float32).reshape(Bc, 45)
    out["chain/mats"] = mats
    gm = ref_vjp(chain(False), [betas, mats], np.ones(()))
    out["chain/grad_mat/betas"], out["chain/grad_mat/pose"] = gm
    path = os.path.join(HERE, "g11_geometry_grad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
