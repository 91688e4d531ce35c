"""tests/geometry_grad_ref.py (the float64 torch restatements that serve as the truth of tests/test_geometry_grad_gpu.py) pinned
to the reference implementation's own autograd gradients recorded in tests/golden/g11_geometry_grad.npz: every gradient element
within 1e-10 of max(1, |item|_inf) -- float64 rounding (1.1e-16) times the condition numbers the conditioned input domains
allow (< 1e4) with two orders to spare.  Also: the input generators satisfy their conditioning predicates at every size the
GPU test uses, with none left out, and the float64 gradients are finite there.  No GPU."""
import numpy as np
import pytest
import torch

import geometry_grad_ref as G
from conftest import load_golden

TOL = 1e-10
SIZES = (1, 255, 256, 257, 1000, 70001)


def close(got, want, what):
    err = G.item_error(got, want) * G.U
    assert got.shape == want.shape, what
    assert float(err.max()) <= TOL, (what, float(err.max()))


@pytest.fixture(scope="module")
def g11():
    return load_golden("g11_geometry_grad")


def test_restated_conversions_match_recorded_reference_gradients(g11):
    x = {k[3:]: g11[k] for k in g11.files if k.startswith("in/")}
    assert G.predicates(x).all()
    for key, (fn, _, operands) in G.OPS.items():
        grads = G.vjp(fn, [x[o] for o in operands], x[f"g{G.out_width(key)}"])
        for i, gr in enumerate(grads):
            close(gr, g11[f"grad/{key}/{i}"], (key, i))


@pytest.mark.parametrize("conv", G.CONVENTIONS)
def test_restated_euler_conversions_match_recorded_reference_gradients(g11, conv):
    xe = {k: g11[f"euler/{conv}/{k}"] for k in ("e", "R", "g3", "g9")}
    assert G.euler_predicate(xe, conv).all()
    close(G.vjp(lambda e: G.e2m(e, conv), [xe["e"]], xe["g9"])[0], g11[f"grad/e2m/{conv}"], ("e2m", conv))
    close(G.vjp(lambda m: G.m2e(m, conv), [xe["R"]], xe["g3"])[0], g11[f"grad/m2e/{conv}"], ("m2e", conv))


def test_restated_special_branches_match_recorded_reference_gradients(g11):
    """Taylor branch (|a| = 1e-7, quaternion angle 4e-7), _sqrt_positive_part arguments <= 0, w < 0."""
    sp = {k[len("special/in/"):]: g11[k] for k in g11.files if k.startswith("special/in/")}
    assert np.all(np.linalg.norm(sp["aa"].astype(np.float64), axis=1) < 1e-6)
    R = sp["R"].astype(np.float64)
    assert np.all(1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] <= 0) and np.all(sp["q_neg"][:, 0] < 0)
    for key, (operands, gk) in G.SPECIAL_CASES.items():
        grads = G.vjp(G.OPS[key][0], [sp[o] for o in operands], sp[gk])
        for i, gr in enumerate(grads):
            close(gr, g11[f"special/grad/{key}/{i}"], ("special", key, i))
    # the generator still produces the recorded inputs
    now = G.special_inputs()
    for k, v in sp.items():
        assert np.array_equal(now[k], v), k


def test_restated_flame_pieces_match_recorded_reference_gradients(g11):
    close(G.vjp(G.rodrigues, [g11["rod/r"]], g11["rod/g"])[0], g11["rod/grad"], "rodrigues")
    faces, idx = torch.from_numpy(g11["lmk/faces"]), torch.from_numpy(g11["lmk/idx"])
    bary = torch.from_numpy(g11["lmk/bary"]).double()
    close(G.vjp(lambda v: G.landmarks(v, faces, idx, bary), [g11["lmk/verts"]], g11["lmk/g"])[0], g11["lmk/grad"], "landmarks")
    m = {k[len("chain/m/"):]: torch.from_numpy(g11[k]).double() for k in g11.files if k.startswith("chain/m/")}
    m["parents"] = [int(p) for p in g11["chain/parents"]]
    cf, ci = torch.from_numpy(g11["chain/faces"]), torch.from_numpy(g11["chain/idx"])
    cb = torch.from_numpy(g11["chain/bary"]).double()
    gv, gl = torch.from_numpy(g11["chain/gv"]).double(), torch.from_numpy(g11["chain/gl"]).double()
    for pose_key, grad_key, is_mat in (("chain/pose", "chain/grad", False), ("chain/mats", "chain/grad_mat", True)):
        def chain(b, p):
            v = G.lbs(m, b, p, pose_is_matrix=is_mat)
            return (v * gv).sum() + (G.landmarks(v, cf, ci, cb) * gl).sum()
        gb, gp = G.vjp(chain, [g11["chain/betas"], g11[pose_key]], np.ones(()))
        close(gb, g11[f"{grad_key}/betas"], (grad_key, "betas"))
        close(gp, g11[f"{grad_key}/pose"], (grad_key, "pose"))


@pytest.mark.parametrize("n", SIZES)
def test_generators_satisfy_their_predicates_and_gradients_are_finite(n):
    """Every item of every size: radicands >= 0.05, angles in [0.05, pi - 0.1], 6-D pairs |a1| >= 0.1 and |sin| >= 0.1,
    quaternion norms in [0.5, 2], Euler central angles |cos| >= 0.1 (proper Euler also |sin| >= 0.1)."""
    x = G.rotation_inputs(f"geom_grad/rot/{n}", n)
    ok = G.predicates(x)
    assert ok.shape == (n,) and ok.all()
    for key, (fn, _, operands) in G.OPS.items():
        for gr in G.vjp(fn, [x[o] for o in operands], x[f"g{G.out_width(key)}"]):
            assert np.all(np.isfinite(gr)), key
    for conv in G.CONVENTIONS:
        xe = G.euler_inputs(f"geom_grad/euler/{n}", n, conv)
        ok = G.euler_predicate(xe, conv)
        assert ok.shape == (n,) and ok.all(), conv
        assert np.all(np.isfinite(G.vjp(lambda e: G.e2m(e, conv), [xe["e"]], xe["g9"])[0]))
        assert np.all(np.isfinite(G.vjp(lambda m: G.m2e(m, conv), [xe["R"]], xe["g3"])[0]))


def test_recorded_yardstick_is_what_float32_autograd_measures():
    """The GPU test's bounds are 4 x G.YARDSTICK (floor 16 u): the float32 torch-CPU autograd of the restatements, re-measured
    here on the GPU test's own inputs, must still give the recorded figures -- to 2 % (another libm may move a last digit) -- so
    that a changed generator or restatement cannot leave a bound wider than the rule allows."""
    now = G.yardstick()
    assert set(now) == set(G.YARDSTICK)
    for k, v in G.YARDSTICK.items():
        assert abs(now[k] - v) <= 0.02 * v + 0.005, (k, now[k], v)
