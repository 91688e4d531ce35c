"""Retargeting without a GPU: the float64 restatement (tests/retarget_ref.py) against scipy's BVLS and against the optimality
conditions on every case the GPU tests use, planted mutants, the header / library / ops agreement, the refusals, and the host
side of utils/retarget (rig checks, the positive-definiteness check, the curve files)."""
import ctypes

import numpy as np
import pytest
from scipy.optimize import lsq_linear

import retarget_ref as R
from msmd_amd import _lib, ops, synth
from msmd_amd.utils import retarget as RT

ALL_CASES = list(R.CASES) + ["backup"]


def _problem(name):
    """-> (H, b (N, K) float64 of the fp32 values, lo, hi, w, status, iterations) of a shared case or of the backup case."""
    if name == "backup":
        H, b, lo, hi = R.backup_case()
        w, st, it = R.solve(H, b, lo, hi)
        return H, b.astype(np.float64), lo, hi, w, st, it
    c = R.case(name)
    p = c["prep"]
    return p["H"], c["b32"].astype(np.float64), p["lo"], p["hi"], c["w"], c["status"], c["iterations"]


@pytest.mark.parametrize("name", ALL_CASES)
def test_restatement_against_bvls(name):
    """scipy.optimize.lsq_linear(method='bvls') on the Cholesky factor of H: min |L^T w - L^-1 b|^2 in the box is the same problem.
    Bound: 8 K 2^-53 cond_2(H) max(1, |w*|_inf).  Also the condition the GPU tests rest on: status 0 under the cap."""
    H, b, lo, hi, w, st, it = _problem(name)
    assert (st == 0).all() and (it < R.CAP).all(), (st, it)
    L = np.linalg.cholesky(H)
    worst = 0.0
    for n in range(len(b)):
        ref = lsq_linear(L.T, np.linalg.solve(L, b[n]), bounds=(lo, hi), method="bvls", tol=1e-15).x
        worst = max(worst, float(np.abs(ref - w[n]).max()))
    bound = R.solve_bound(H, w)
    print(f"{name}: cond {np.linalg.cond(H):.3g}, iterations {it.min()} .. {it.max()}, |w - bvls| = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    assert (w >= lo).all() and (w <= hi).all()


@pytest.mark.parametrize("name", ALL_CASES)
def test_optimality_conditions(name):
    """g = H w - b is >= 0 at lo, <= 0 at hi and 0 inside, to the residual of a backward-stable solve:
    8 K 2^-53 (|H|_inf max(1, |w|_inf) + |b|_inf)."""
    H, b, lo, hi, w, st, it = _problem(name)
    K = H.shape[0]
    for n in range(len(b)):
        tol = 8 * K * R.U64 * (np.abs(H).sum(1).max() * max(1.0, np.abs(w[n]).max()) + np.abs(b[n]).max())
        assert R.kkt_violation(H, b[n], lo, hi, w[n]) <= tol


def test_cases_cover_what_they_claim():
    c = R.case("K52-V700-planted")
    p = c["prep"]
    assert (c["w_star"][0, ::2] == p["lo"][::2]).all() and (c["w_star"][0, 1::2] == p["hi"][1::2]).all()
    g = R.case("K7-V97-general")["prep"]
    assert (g["lo"] == -0.25).all() and (g["hi"] == 1.0).all()
    for name in R.CASES:
        c = R.case(name)
        at = (c["w"] <= c["prep"]["lo"]) | (c["w"] >= c["prep"]["hi"])
        assert at.any() and (~at).any(), name                       # bound and free weights in every case
    assert not R.case("K7-V97-noisy")["prep"]["used"].all()
    r = R.case("K64-V15-ridge")
    assert r["prep"]["K"] > 3 * r["prep"]["V"] and np.linalg.matrix_rank(r["prep"]["G"]) < 64
    assert (np.abs(R.case("K52-V700-planted")["w"] - R.case("K52-V700-planted")["w_star"]) < 1e-5).all()    # noise-free: recovered


# ----------------------------------------------------------------------------- mutants
MUTANT_CASES = [n for n in R.CASES if "5023" not in n]


def _run(mutant):
    """The whole restated pipeline on every small case, on a copy of K7-V97-noisy with a NaN in a weightless vertex, and on the
    backup case -> {label: (w, status)}; a matrix the positive-definiteness check refuses is recorded as 'refused'."""
    out = {}
    for name in MUTANT_CASES:
        c = R.case(name)
        xs = {name: c["x"]}
        if name == "K7-V97-noisy":
            x = c["x"].copy()
            x[1, np.nonzero(~c["prep"]["used"])[0][0], 2] = np.nan
            xs[name + "+nan"] = x
        for label, x in xs.items():
            try:
                RT.check_positive_definite(R.prepare(c["rig"], mutant)["H"])
                out[label] = R.retarget(c["rig"], x, mutant=mutant)[:2]
            except ValueError:
                out[label] = "refused"
    H, b, lo, hi = R.backup_case()
    out["backup"] = R.solve(H, b, lo, hi, mutant=mutant)[:2]
    return out


def _differs(got, want, label):
    if isinstance(got, str) or isinstance(want, str):
        return got is not want and not (isinstance(got, str) and isinstance(want, str))
    if not np.array_equal(got[1], want[1]):
        return True
    H = R.backup_case()[0] if label == "backup" else R.case(label.split("+")[0])["prep"]["H"]
    bound = R.solve_bound(H, want[0])
    return not bool((np.abs(got[0] - want[0]) <= bound).all())      # a NaN differs


@pytest.fixture(scope="module")
def unmutated():
    return _run(None)


def test_the_unmutated_pipeline_is_not_flagged(unmutated):
    again = _run(None)
    assert not [k for k in unmutated if _differs(again[k], unmutated[k], k)]
    assert all(not isinstance(v, str) and (v[1] == 0).all() and np.isfinite(v[0]).all() for v in unmutated.values())
    nan, plain = unmutated["K7-V97-noisy+nan"], unmutated["K7-V97-noisy"]
    assert np.array_equal(nan[0], plain[0])             # the NaN sits in a vertex that is never read


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_planted_mutant_is_caught(mutant, unmutated):
    got = _run(mutant)
    caught = [k for k in unmutated if _differs(got[k], unmutated[k], k)]
    print(f"{mutant}: caught on {caught}")
    assert caught
    if mutant == "no_backup":
        assert caught == ["backup"] and got["backup"][1][0] == 1            # it cycles up to the cap
    if mutant == "no_ridge":
        assert got["K64-V15-ridge"] == "refused"
    if mutant == "read_zero_weight":
        assert caught == ["K7-V97-noisy+nan"] and got["K7-V97-noisy+nan"][1][1] == 2


# ----------------------------------------------------------------------------- header, library, ops
ENTRIES = ("msmd_retarget_splits", "msmd_retarget_gram", "msmd_retarget_rhs", "msmd_retarget_solve", "msmd_blendshape_apply")


def test_header_library_and_ops_agree():
    lib = _lib.load()
    protos, c = _lib.parse_header(), _lib.parse_constants()
    for name in ENTRIES:
        assert name in protos and hasattr(lib, name)
    assert len(protos["msmd_retarget_rhs"]) == 10 and len(protos["msmd_retarget_solve"]) == 11
    assert c["MSMD_RETARGET_MAX_SHAPES"] == ops.RETARGET_MAX_SHAPES == 64
    assert c["MSMD_RETARGET_ITERATIONS"] == ops.RETARGET_ITERATIONS == R.CAP == 256
    assert c["MSMD_RETARGET_FRAME_TILE"] == ops.RETARGET_FRAME_TILE and c["MSMD_RETARGET_VERTEX_TILE"] == ops.RETARGET_VERTEX_TILE
    assert c["MSMD_RETARGET_SPLIT_VERTICES"] == ops.RETARGET_SPLIT_VERTICES and ops.RETARGET_SPLIT_VERTICES % ops.RETARGET_VERTEX_TILE == 0
    assert (ops.RETARGET_CONVERGED, ops.RETARGET_CAP_REACHED, ops.RETARGET_BAD_INPUT, ops.RETARGET_NOT_POSITIVE) == (0, 1, 2, 3)
    S = ops.RETARGET_SPLIT_VERTICES
    assert [lib.msmd_retarget_splits(v) for v in (0, 1, S, S + 1, 5023)] == [0, 1, 1, 2, -(-5023 // S)]
    for f in ("retarget_gram", "retarget_rhs", "retarget_solve", "blendshape_apply"):
        assert callable(getattr(ops, f))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    fake = ctypes.addressof(buf)
    p = lambda a: a.ctypes.data
    ones, zeros = np.ones(64), np.zeros(64)
    # rhs
    rhs = lambda x=fake, n=fake, A=fake, part=fake, b=fake, N=1, V=5, K=3: lib.msmd_retarget_rhs(x, n, A, None, part, b, N, V, K, None)
    for bad in (dict(x=None), dict(n=None), dict(A=None), dict(part=None), dict(b=None), dict(N=-1), dict(K=0), dict(K=65), dict(V=0)):
        assert rhs(**bad) == 1, bad
    assert rhs(N=0) == 0 and rhs(N=0, x=None, b=None) == 0 and rhs(N=0, K=65) == 1
    # gram
    gram = lambda A=fake, ridge=None, G=fake, H=fake, K=3, V=5: lib.msmd_retarget_gram(A, ridge, G, H, K, V, None)
    neg = zeros.copy()
    neg[2] = -1e-300
    nan = zeros.copy()
    nan[0] = np.nan
    for bad in (dict(A=None), dict(G=None), dict(H=None), dict(K=0), dict(K=65), dict(V=0), dict(ridge=p(neg)), dict(ridge=p(nan))):
        assert gram(**bad) == 1, bad
    # solve
    solve = lambda H=fake, b=fake, lo=None, hi=None, w=fake, st=fake, it=fake, N=1, K=3, cap=256: \
        lib.msmd_retarget_solve(H, b, lo, hi, w, st, it, N, K, cap, None)
    eq = zeros.copy()
    eq[1] = 1.0                      # lo[1] == hi[1]
    inf = ones.copy()
    inf[0] = np.inf
    for bad in (dict(H=None), dict(b=None), dict(w=None), dict(st=None), dict(it=None), dict(N=-1), dict(K=0), dict(K=65), dict(cap=0),
                dict(lo=p(eq)), dict(lo=p(ones), hi=p(zeros)), dict(hi=p(inf)), dict(lo=p(nan))):
        assert solve(**bad) == 1, bad
    assert solve(N=0, H=None, b=None) == 0 and solve(N=0, lo=p(eq)) == 1
    # apply
    app = lambda w=fake, n=fake, d=fake, out=fake, N=1, V=5, K=3: lib.msmd_blendshape_apply(w, n, d, out, N, V, K, None)
    for bad in (dict(w=None), dict(n=None), dict(d=None), dict(out=None), dict(N=-1), dict(K=0), dict(K=65), dict(V=0)):
        assert app(**bad) == 1, bad
    assert app(N=0, out=None) == 0


def test_rig_refusals():
    r = synth.blendshape_rig(9, 3, 1)
    RT.Rig(**r)
    with pytest.raises(ValueError, match="lo < hi"):
        RT.Rig(**r, lo=[0, 1, 0], hi=[1, 1, 1])
    with pytest.raises(ValueError, match="ridge"):
        RT.Rig(**r, ridge=[0, -1e-9, 0])
    with pytest.raises(ValueError, match="vertex_weight"):
        RT.Rig(**r, vertex_weight=-np.ones(9))
    with pytest.raises(ValueError, match="names"):
        RT.Rig(r["neutral"], r["deltas"], ["a", "b"])
    with pytest.raises(ValueError, match="65 blendshapes"):
        RT.Rig(**{**synth.blendshape_rig(9, 65, 1)})
    with pytest.raises(ValueError, match="neutral"):
        RT.Rig(r["neutral"][:5], r["deltas"])


def test_positive_definite_check_names_the_fix():
    c = R.case("K64-V15-ridge")
    RT.check_positive_definite(c["prep"]["H"], 15)
    with pytest.raises(ValueError, match=r"ridge.*"):
        RT.check_positive_definite(c["prep"]["G"], 15)
    with pytest.raises(ValueError, match="64 blendshapes cannot be told apart by 15 weighted vertices"):
        RT.check_positive_definite(c["prep"]["G"], 15)
    with pytest.raises(ValueError, match="not positive definite"):
        RT.check_positive_definite(np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(ValueError, match="not finite"):
        RT.check_positive_definite(np.array([[np.nan]]))


def test_rig_file_round_trip(tmp_path):
    r = synth.blendshape_rig(11, 4, 2)
    rig = RT.Rig(**r, lo=-0.25, ridge=[0, 1e-6, 0, 0], vertex_weight=np.arange(11) % 3)
    rig.save(tmp_path / "rig.npz")
    back = RT.load_rig(tmp_path / "rig.npz")
    for k in ("neutral", "deltas", "vertex_weight", "lo", "hi", "ridge"):
        assert np.array_equal(getattr(back, k), getattr(rig, k)), k
    assert back.names == rig.names == r["names"]
    np.savez(tmp_path / "bad.npz", neutral=r["neutral"], deltas=r["deltas"], faces=np.zeros(3))
    with pytest.raises(ValueError, match="faces"):
        RT.load_rig(tmp_path / "bad.npz")


def test_write_curves_round_trip(tmp_path):
    g = np.random.default_rng(7)
    w = g.random((5, 3)).astype(np.float32)
    w[0, 0], w[1, 1], w[2, 2] = 0.0, 1.0, np.float32(1e-30)
    names = ["jawOpen", "mouth,Smile \"L\"", "browDown_R"]
    RT.write_curves(tmp_path / "c.csv", w, names, 25)
    lines = open(tmp_path / "c.csv").read().splitlines()
    assert len(lines) == 6 and lines[0].startswith("jawOpen,")
    n2, w2, fps = RT.read_curves(tmp_path / "c.csv")
    assert n2 == names and fps is None and w2.dtype == np.float32 and np.array_equal(w2, w)
    RT.write_curves(tmp_path / "c.json", w, names, 29.97)
    n3, w3, fps3 = RT.read_curves(tmp_path / "c.json")
    assert n3 == names and fps3 == 29.97 and np.array_equal(w3, w)
    RT.write_curves(tmp_path / "e.csv", np.zeros((0, 3), np.float32), names, 25)
    assert RT.read_curves(tmp_path / "e.csv")[1].shape == (0, 3)
    with pytest.raises(ValueError, match="names"):
        RT.write_curves(tmp_path / "x.csv", w, names[:2], 25)
    with pytest.raises(ValueError, match="csv or .json"):
        RT.write_curves(tmp_path / "x.fbx", w, names, 25)
    with pytest.raises(ValueError, match="fps"):
        RT.write_curves(tmp_path / "x.csv", w, names, 0)


def test_synthetic_rig_is_deterministic_and_overlapping():
    a, b = synth.blendshape_rig(300, 12, 3), synth.blendshape_rig(300, 12, 3)
    assert np.array_equal(a["deltas"], b["deltas"]) and a["deltas"].shape == (300, 12, 3)[1::-1] + (3,) and a["deltas"].dtype == np.float32
    assert not np.array_equal(a["deltas"], synth.blendshape_rig(300, 12, 4)["deltas"])
    A = a["deltas"].reshape(12, -1).astype(np.float64)
    G = A @ A.T
    corr = G / np.sqrt(np.outer(np.diag(G), np.diag(G)))
    assert np.abs(corr - np.eye(12)).max() > 0.3 and np.linalg.cond(G) < 1e6
