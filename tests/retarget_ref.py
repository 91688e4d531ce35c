"""Float64 numpy restatement of the retargeting operator and of its solver rule (include/msmd_hip.h), the cases
the CPU and GPU tests share, and the error bounds both hold results against.

Every sum reads the STORED fp32 arrays (A = fl32(vertex_weight * deltas), d = fl32(x - neutral)) as their exact float64 images,
so what separates this file from the kernels is summation order and fp32 rounding alone.  `mutant=` plants one defect at a time
(tests/test_retarget_cpu.py checks that each is caught)."""
import functools

import numpy as np

from msmd_amd import synth

U32, U64 = 2.0 ** -24, 2.0 ** -53
CAP = 256
MUTANTS = ("no_neutral", "weights_twice", "no_upper", "sign_g_upper", "no_backup", "no_ridge", "read_zero_weight")


# ----------------------------------------------------------------------------- the operator
def prepare(rig, mutant=None):
    """rig: dict with neutral, deltas and optionally vertex_weight, lo, hi, ridge -> dict(A fp32 (K, V, 3), used (V) bool, G, H,
    lo, hi float64)."""
    deltas = np.asarray(rig["deltas"], np.float32)
    K, V = deltas.shape[:2]
    vw = rig.get("vertex_weight")
    vw = np.ones(V, np.float32) if vw is None else np.asarray(vw, np.float32)
    A = (vw[None, :, None] * deltas).astype(np.float32)              # one fp32 product
    if mutant == "weights_twice":
        A = (vw[None, :, None] * A).astype(np.float32)
    A64 = A.reshape(K, -1).astype(np.float64)
    G = A64 @ A64.T
    ridge = np.zeros(K) if rig.get("ridge") is None or mutant == "no_ridge" else np.broadcast_to(np.asarray(rig["ridge"], np.float64), (K,))
    lo = np.zeros(K) if rig.get("lo") is None else np.broadcast_to(np.asarray(rig["lo"], np.float64), (K,)).copy()
    hi = np.ones(K) if rig.get("hi") is None else np.broadcast_to(np.asarray(rig["hi"], np.float64), (K,)).copy()
    return dict(A=A, used=vw != 0, G=G, H=G + np.diag(ridge), lo=lo, hi=hi, neutral=np.asarray(rig["neutral"], np.float32), K=K, V=V)


def rhs(prep, x, mutant=None):
    """x (N, V, 3) fp32 -> (b64 (N, K) float64, absum (N, K) = sum |A d|): the float64 sum over the stored fp32 A and the fp32
    difference, over the used vertices only."""
    x = np.asarray(x, np.float32)
    used = np.ones_like(prep["used"]) if mutant == "read_zero_weight" else prep["used"]
    d = x[:, used] if mutant == "no_neutral" else (x[:, used] - prep["neutral"][None, used]).astype(np.float32)
    A = prep["A"][:, used].reshape(prep["K"], -1).astype(np.float64)
    d = d.reshape(x.shape[0], A.shape[1]).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return d @ A.T, np.abs(d) @ np.abs(A).T


def rhs_bound(absum, n_terms):
    """|fl(sum) - sum| <= gamma_{n + 1} sum |A d| with u = 2^-24, for any order of an n-term fp32 sum of fp32 products."""
    g = (n_terms + 1) * U32
    return g / (1.0 - g) * absum


def bpp(H, b, lo, hi, cap=CAP, mutant=None):
    """Block principal pivoting for the box, the rule of include/msmd_hip.h -> (w, status, iterations)."""
    K = len(b)
    if not np.isfinite(b).all():
        return np.full(K, np.nan), 2, 0
    hi_used = np.full(K, np.inf) if mutant == "no_upper" else hi
    st = np.zeros(K, int)                    # 0 at lo, 1 free, 2 at hi
    budget, best, it = 3, K + 1, 0
    while True:
        it += 1
        F = st == 1
        w = np.where(st == 0, lo, hi).astype(np.float64)
        if F.any():
            w[F] = np.linalg.solve(H[np.ix_(F, F)], b[F] - H[np.ix_(F, ~F)] @ w[~F])
        g = H @ w - b
        to_lo, to_hi = F & (w < lo), F & (w > hi_used)
        to_free = ((st == 0) & (g < 0)) | ((st == 2) & ((g < 0) if mutant == "sign_g_upper" else (g > 0)))
        bad = to_lo | to_hi | to_free
        n = int(bad.sum())
        if n == 0:
            return np.clip(w, lo, hi_used), 0, it
        if it >= cap:
            return np.clip(w, lo, hi_used), 1, it
        if n < best:
            best, budget, everything = n, 3, True
        elif budget > 0 or mutant == "no_backup":
            budget, everything = budget - 1, True
        else:
            everything = False
        sel = np.ones(K, bool) if everything else np.arange(K) == np.nonzero(bad)[0].max()
        st = np.where(sel & to_lo, 0, np.where(sel & to_hi, 2, np.where(sel & to_free, 1, st)))


def solve(H, b, lo, hi, cap=CAP, mutant=None):
    """b (N, K) -> (w (N, K) float64, status (N), iterations (N))."""
    out = [bpp(H, np.asarray(r, np.float64), lo, hi, cap, mutant) for r in b]
    return np.array([o[0] for o in out]).reshape(len(b), len(lo)), np.array([o[1] for o in out], int), np.array([o[2] for o in out], int)


def retarget(rig, x, cap=CAP, mutant=None):
    """The whole operator: x (N, V, 3) fp32 -> (w float64, status, iterations); b is rounded to fp32 on the way, as the kernels
    store it."""
    p = prepare(rig, mutant)
    b = rhs(p, x, mutant)[0].astype(np.float32)
    return solve(p["H"], b, p["lo"], p["hi"], cap, mutant)


def apply(rig, w):
    """-> (out float64 (N, V, 3), terms = |neutral| + sum_k |w_k delta_k|) from the stored fp32 arrays."""
    n, d, w = np.asarray(rig["neutral"], np.float64), np.asarray(rig["deltas"], np.float64), np.asarray(w, np.float64)
    return n[None] + np.einsum("nk,kvc->nvc", w, d), np.abs(n)[None] + np.einsum("nk,kvc->nvc", np.abs(w), np.abs(d))


def solve_bound(H, w):
    """8 K 2^-53 cond_2(H) max(1, |w|_inf): the Cholesky backward-error form."""
    return 8 * H.shape[0] * U64 * np.linalg.cond(H) * max(1.0, float(np.abs(w).max()))


def kkt_violation(H, b, lo, hi, w):
    """max over the weights of how far w is from satisfying the optimality conditions of the box problem: g >= 0 at lo, g <= 0
    at hi, g = 0 strictly inside, with g = H w - b; and the distance outside the box."""
    g = H @ w - b
    at_lo, at_hi = w <= lo, w >= hi
    v = np.where(at_lo, np.maximum(-g, 0), np.where(at_hi, np.maximum(g, 0), np.abs(g)))
    return float(max(v.max(), np.maximum(lo - w, 0).max(), np.maximum(w - hi, 0).max()))


# ----------------------------------------------------------------------------- the cases
def _rig(V, K, seed, lo=None, hi=None, ridge_rel=0.0, zero_weight_every=0):
    r = synth.blendshape_rig(V, K, seed)
    if lo is not None:
        r["lo"], r["hi"] = np.full(K, lo), np.full(K, hi)
    if zero_weight_every:
        vw = (0.5 + synth.uniform01(f"case/vw/{V}/{K}/{seed}", V)).astype(np.float32)
        vw[::zero_weight_every] = 0.0
        r["vertex_weight"] = vw
    if ridge_rel:
        A = prepare(r)["G"]
        r["ridge"] = np.full(K, ridge_rel * np.trace(A) / K)
    return r


# name -> (V, K, seed, lo, hi, relative ridge, every n-th vertex weightless, frames, noise in units of the largest delta)
CASES = {
    "K1-V1": (1, 1, 1, None, None, 0.0, 0, 4, 0.0),
    "K7-V97-general": (97, 7, 2, -0.25, 1.0, 0.0, 0, 6, 0.0),
    "K7-V97-noisy": (97, 7, 3, None, None, 0.0, 3, 6, 0.05),
    "K52-V700-planted": (700, 52, 4, None, None, 0.0, 0, 6, 0.0),
    "K52-V700-noisy": (700, 52, 5, -0.25, 1.0, 0.0, 5, 6, 0.02),
    "K64-V700-noisy": (700, 64, 6, None, None, 0.0, 0, 6, 0.02),
    "K64-V15-ridge": (15, 64, 7, None, None, 1e-3, 0, 6, 0.01),          # K > 3 V: singular without the ridge
    "K52-V5023-noisy": (5023, 52, 8, None, None, 0.0, 0, 4, 0.01),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(rig, w_star (N, K) float64 in the box with weights planted exactly at lo and hi, x (N, V, 3) fp32 =
    fl32(neutral + sum w* delta + noise), prep, b32 (the reference's b rounded to fp32), w, status, iterations (the
    restatement's result))."""
    V, K, seed, lo, hi, ridge_rel, zw, N, noise = CASES[name]
    rig = _rig(V, K, seed, lo, hi, ridge_rel, zw)
    p = prepare(rig)
    u = synth.uniform01(f"case/w/{name}", N * K).reshape(N, K).astype(np.float64)
    span = p["hi"] - p["lo"]
    w_star = p["lo"] + span * np.clip(1.6 * u - 0.3, 0.0, 1.0)           # about a fifth at each bound, exactly
    w_star[0, ::2] = p["lo"][::2]
    w_star[0, 1::2] = p["hi"][1::2]
    x = apply(rig, w_star)[0]
    if noise:
        x = x + noise * float(np.abs(rig["deltas"]).max()) * synth.normalish(f"case/noise/{name}", x.shape).astype(np.float64)
    x = x.astype(np.float32)
    b64, absum = rhs(p, x)
    b32 = b64.astype(np.float32)
    w, status, its = solve(p["H"], b32, p["lo"], p["hi"])
    return dict(name=name, rig=rig, prep=p, w_star=w_star, x=x, b64=b64, absum=absum, b32=b32, w=w, status=status, iterations=its)


# A problem on which exchanging every infeasible weight every time cycles for ever: found by a random search over 6 x 6
# problems (about one in 200 such problems cycles), its numbers rounded to two decimals.  The rule's backup -- single exchanges
# once the budget is spent -- ends it in 9 iterations.  H = M M^T + 0.01 I, cond_2 about 190, box [0, 1].
BACKUP_M = np.array([[0.15, -0.83, 0.6, 1.15, -0.09, -0.02], [-1.33, 0.05, -1.59, 1.3, -1.62, 1.53], [0.9, 0.82, 0.78, 0.37, 1.77, 0.62],
                     [-1.2, -0.14, 1.29, -0.86, 0.17, -0.74], [0.04, -1.07, 0.21, 0.34, -0.69, -0.07], [0.15, 1.94, -1.11, -0.88, 1.86, 0.38]])
BACKUP_B = np.array([1.17, 0.55, 1.19, 2.27, -1.62, 1.31], np.float32)


def backup_case():
    """-> (H (6, 6) float64, b (1, 6) fp32, lo, hi)."""
    return BACKUP_M @ BACKUP_M.T + 0.01 * np.eye(6), BACKUP_B[None].copy(), np.zeros(6), np.ones(6)
