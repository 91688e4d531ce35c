"""numpy restatement of the attention forward (csrc/attention.hip: attn_whole_kernel, attn_kernel): the truth, the yardstick and
the bound the attention tests compare against, with the input families, masks and the emulator of the 16-bit arithmetic that
tests/test_attention_cpu.py and tests/test_attention_gpu.py share.  Nothing in the product imports this file.

float64 is the truth; float32 (the same operations, no storage rounding) is the yardstick.  Operands are (B, T, H * 64) float32
arrays already rounded to the storage type ("fp32", "bf16" or "fp16"), so the only differences between a kernel and the truth are
the ones the bound has a term for (see `bound`)."""
import functools

import numpy as np

from msmd_amd import synth
from oracle import diffusion as od

U = 2.0 ** -24
U_T = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}      # unit roundoff of the storage types (round to nearest)
SUB = 2.0 ** -14                                                      # smallest normal fp16
LOG2E = 1.4426950408889634


def round_to(x, T):
    """float32 array -> the nearest value of the storage type (ties to even), as float32."""
    x = np.ascontiguousarray(x, np.float32)
    if T == "fp32":
        return x
    if T == "fp16":
        return x.astype(np.float16).astype(np.float32)
    if T == "bf16":
        b = x.view(np.uint32).astype(np.uint64)
        b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
        return b.astype(np.uint32).view(np.float32).reshape(x.shape)
    raise KeyError(T)


def _heads(x, H, dtype):
    B, T, d = x.shape
    assert d == H * 64
    return np.asarray(x).astype(dtype).reshape(B, T, H, 64).transpose(0, 2, 1, 3)


def _merge(x):
    B, H, T, _ = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B, T, H * 64)


def probabilities(q, k, H, scale, mask=None, keep=None, p_drop=0.0, dtype=np.float64):
    """(P~, rel), both (B, H, Tq, Tk): P~ the softmax probabilities with `keep` applied AFTER the denominator and the factor
    1 / (1 - p_drop); rel = exp(s - row maximum), the value a kernel holds before it divides (1 at the row's largest score).
    A fully masked row is NaN."""
    qh, kh = _heads(q, H, dtype), _heads(k, H, dtype)
    s = np.matmul(qh, kh.transpose(0, 1, 3, 2)) * dtype(scale)
    if mask is not None:
        s = np.where(np.asarray(mask)[None, None] != 0, dtype(-np.inf), s)
    with np.errstate(invalid="ignore"):
        rel = np.exp(s - s.max(-1, keepdims=True))               # -inf - -inf = NaN in a fully masked row
        P = rel / rel.sum(-1, keepdims=True, dtype=dtype)
    if keep is not None:
        P = np.where(keep, P, dtype(0)) / dtype(1.0 - p_drop)
    return P.astype(dtype), rel.astype(dtype)


def attention(q, k, v, H, scale, mask=None, keep=None, p_drop=0.0, dtype=np.float64):
    """(O, A), both (B, Tq, H * 64): O = P~ V and A = sum_k P~_k |v_k|, the magnitude every error term scales with (|O| <= A)."""
    P, _ = probabilities(q, k, H, scale, mask, keep, p_drop, dtype)
    vh = _heads(v, H, dtype)
    return _merge(np.matmul(P, vh)), _merge(np.matmul(P, np.abs(vh)))


def bound(A64, A32_err, T, Tk, n_sub=None, vmax=None):
    """Per-element tolerance on |O - O64|, an array shaped like A64.

    fp32 term, every type: max(16 u, 4 x yardstick) A, u = 2^-24, yardstick A32_err = max |O32 - O64| / A of the float32
    restatement on the same inputs (DESIGN.md 5.9's form): scores, exponentials, the denominator and the P V sums in fp32.
    16-bit storage adds 2 u_T A (u_bf16 = 2^-8, u_f16 = 2^-11):
      u_T A  each probability is rounded to the storage type for the P V product, error <= u_T p_k each, sum_k u_T p_k |v_k| / l;
             the denominator l is summed from the unrounded fp32 values, so this error is not normalised away;
      u_T A  the output is rounded to the storage type, error <= u_T |O| <= u_T A.
    fp16 adds two absolute terms:
      n_sub 2^-24 vmax  a probability below 2^-14 of its row's maximum is an fp16 subnormal (spacing 2^-24): its rounding error is
             absolute.  n_sub = such live keys in the row, vmax = max |v|; the denominator is >= 1 (the row's largest p is 1), so
             dividing by it does not enlarge the term.  Assumes gradual underflow in the conversion and the MFMA.
      2^-25  an output below 2^-14 is a subnormal too: rounding it costs up to half of 2^-24 whatever its size (u_T |O| only holds
             for normal results).  Only the probe family has outputs that small next to an A as small.
    """
    A = np.asarray(A64, np.float64)
    b = max(16.0 * U, 4.0 * float(A32_err)) * A
    if T != "fp32":
        b = b + 2.0 * U_T[T] * A
    if T == "fp16":
        n_sub = np.asarray(n_sub, np.float64)
        assert n_sub.max(initial=0) <= Tk
        b = b + n_sub * 2.0 ** -24 * float(vmax) + 2.0 ** -25
    return b


def yardstick(O32, O64, A64):
    """max |O32 - O64| / A over the elements with A > 0 (NaN rows left out; A = 0 means O = 0 in both)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(np.asarray(O32, np.float64) - O64) / A64
    r = r[np.isfinite(r)]
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ inputs
FAMILIES = ("flat", "peaked", "rampup", "rampdown", "probe")


def probe_v(B, H, Tk, window):
    """V = block identity: column c of every head is 1 at key 64 window + c, so O[b, q, h * 64 + c] = P~[b, h, q, 64 window + c]."""
    v = np.zeros((B, Tk, H, 64), np.float32)
    c = np.arange(64)
    key = 64 * window + c
    v[:, key[key < Tk], :, c[key < Tk]] = 1.0
    return v.reshape(B, Tk, H * 64)


def n_windows(Tk):
    return (Tk + 63) // 64


@functools.lru_cache(maxsize=8)
def _inputs(family, B, H, Tq, Tk):
    """(q, k, v) with at least YARD_ROWS query rows: a case with fewer uses the first Tq of them (see `yard_queries`)."""
    d = H * 64
    Tq = max(Tq, YARD_ROWS)
    tag = f"attn/{family}/{B}x{H}x{Tq}x{Tk}"
    nq, nk = synth.normalish(tag + "/q", (B, Tq, d)), synth.normalish(tag + "/k", (B, Tk, d))
    v = synth.normalish(tag + "/v", (B, Tk, d))
    if family == "flat":                      # scaled scores ~ N(0, 1): a nearly flat softmax
        q, k = nq, nk
    elif family == "peaked":                  # scaled scores ~ N(0, 81): a spread of about +-30
        q, k = 3.0 * nq, 3.0 * nk
    elif family in ("rampup", "rampdown"):    # score ~ 8 r(j) (|w|^2 ~ 64, scale 1/8), r monotone over 0 .. 4: the row maximum
        w = synth.normalish(tag + "/w", (B, 1, d))            # rises on every 64-key tile, or sits in the first
        r = 4.0 * np.arange(Tk, dtype=np.float32) / max(Tk - 1, 1)
        r = r if family == "rampup" else r[::-1]
        q, k = w + 0.5 * nq, r[None, :, None] * w + 0.5 * nk
    elif family in ("probe", "warm"):         # scaled scores ~ N(0, 4): probabilities over a few orders of magnitude
        q, k = 2.0 * nq, nk
        if family == "probe":
            v = probe_v(B, H, Tk, 0)
    else:
        raise KeyError(family)
    out = tuple(np.ascontiguousarray(x, np.float32) for x in (q, k, v))
    for x in out:
        x.setflags(write=False)
    return out


def inputs(family, B, H, Tq, Tk, T):
    """(q, k, v) float32, rounded to T.  Every batch and head carries its own data (the probe's V is the same in every head; its
    probabilities are not)."""
    q, k, v = (round_to(x, T) for x in _inputs(family, B, H, Tq, Tk))
    return np.ascontiguousarray(q[:, :Tq]), k, v


YARD_ROWS = 64


def yard_queries(family, B, H, Tq, Tk, T):
    """The queries the yardstick of a case with Tq < YARD_ROWS is taken over: YARD_ROWS rows of the same family against the same
    K and V, the case's own rows first.  The yardstick is a sample maximum of the float32 restatement's error, and over the
    B x H = 6 rows of a Tq = 1 case it is no estimate of it: on the peaked family 11-20 u where 63-65 rows of the same family give
    204-276 u (and the fp32 kernel, at 100 u there, sits where it sits on every other shape).  None where Tq is large enough."""
    if Tq >= YARD_ROWS:
        return None
    return round_to(_inputs(family, B, H, Tq, Tk)[0], T)


MASKS = ("random", "align", "first64", "lastonly", "frag", "fullrow")


@functools.lru_cache(maxsize=None)
def mask(kind, Tq, Tk):
    """uint8 (Tq, Tk), non-zero = dead."""
    rnd = synth.uniform01(f"attn/mask/{Tq}x{Tk}", Tq * Tk).reshape(Tq, Tk) < 0.3
    rnd[:, 0] = False
    q = np.arange(Tq)[:, None]
    j = np.arange(Tk)[None, :]
    if kind == "random":                      # 30 %, column 0 live
        m = rnd
    elif kind == "align":                     # the project's alignment mask: (Tk + 1, Tk)
        assert Tq == Tk + 1 and Tk > 10
        m = od.alignment_mask(10, Tk - 10, 1)
    elif kind == "first64":                   # rows q % 3 == 0: the whole first 64-key tile dead
        assert Tk > 64
        m = (q % 3 == 0) & (j < 64)
    elif kind == "lastonly":                  # rows q % 5 == 0: a single live key, the last
        m = (q % 5 == 0) & (j < Tk - 1)
    elif kind == "frag":                      # one whole 16-key fragment dead in every row, another one from row to row
        assert Tk >= 32
        m = (j // 16) == (q % (Tk // 16))
    elif kind == "fullrow":                   # the random mask with one row dead altogether
        m = rnd.copy()
        m[full_row(Tq)] = True
    else:
        raise KeyError(kind)
    m = np.ascontiguousarray(m, np.uint8)
    assert m.shape == (Tq, Tk)
    m.setflags(write=False)
    return m


def full_row(Tq):
    return Tq // 2


# ------------------------------------------------------------------------------------------------ the dispatch, restated (attention_impl)
def attn_waves(Tq, H, B):
    """attention.hip attn_waves(): waves per workgroup of the tiled kernel."""
    best, best_cost = 4, 1 << 60
    for nw in (16, 13, 7, 4):
        blocks = -(-Tq // (16 * nw)) * H * B
        cost = -(-blocks // 256) * nw
        if cost < best_cost:
            best, best_cost = nw, cost
    return best


def region(T, Tq, Tk, H, B):
    """attention.hip attention_impl(): (kernel region, waves per workgroup) a call lands on."""
    if T != "fp32" and Tk <= 272:
        return ("w13", 7 if Tq <= 112 else 13) if Tk <= 208 else ("w17", 9)
    return ("t32" if T == "fp32" else "t16"), attn_waves(Tq, H, B)


def smallest_grid(nw):
    """The smallest H * B (H >= 2, so that the head stride counts) at Tq = 16 nw for which the tiled kernel runs nw waves."""
    Tq = 16 * nw
    for hb in range(2, 257):
        for h in (8, 4, 3, 2):
            if hb % h == 0 and attn_waves(Tq, h, hb // h) == nw:
                return Tq, h, hb // h
    raise AssertionError(nw)


# ------------------------------------------------------------------------------------------------ reference of one case
def reference(q, k, v, H, scale, T, mask=None, keep=None, p_drop=0.0, probe_window=None, q_yard=None):
    """Everything a comparison needs, computed once: O64, A64, the yardstick, the bound per element, NaN rows.
    probe_window: v is probe_v(.., window), so an output element holds ONE key's probability and the fp16 subnormal count of
    that element is 1 or 0 (that key's), not the row's.
    q_yard: the rows the yardstick is taken over where the case has too few of its own (`yard_queries`)."""
    Tk = k.shape[1]
    O64, A64 = attention(q, k, v, H, scale, mask, keep, p_drop)
    if q_yard is None:
        O32, _ = attention(q, k, v, H, scale, mask, keep, p_drop, dtype=np.float32)
        y = yardstick(O32, O64, A64)
    else:
        assert mask is None and keep is None and np.array_equal(q_yard[:, :q.shape[1]], q)
        y = yardstick(attention(q_yard, k, v, H, scale, dtype=np.float32)[0], *attention(q_yard, k, v, H, scale))
    n_sub = None
    if T == "fp16":
        _, rel = probabilities(q, k, H, scale, mask)
        with np.errstate(invalid="ignore"):
            sub = (rel > 0) & (rel < SUB)                                             # dead keys have rel = 0
        if probe_window is None:
            n_sub = np.repeat(sub.sum(-1).transpose(0, 2, 1), 64, axis=-1).astype(np.float64)     # (B, Tq, H * 64)
        else:
            win = np.zeros(sub.shape[:3] + (64,), np.float64)
            n = min(64, Tk - 64 * probe_window)
            win[..., :n] = sub[..., 64 * probe_window:64 * probe_window + n]
            n_sub = _merge(win)
    bnd = bound(A64, y, T, Tk, n_sub, float(np.abs(v).max()))
    return dict(O=O64, A=A64, yardstick=y, bound=bnd, nan=np.isnan(O64))


def ratio(got, ref):
    """Worst err / bound over EVERY element outside the reference's NaN rows; inf if a NaN sits where none belongs, a finite value
    where the row is NaN in the reference, or an error where the bound is 0."""
    got = np.asarray(got, np.float64)
    if not np.array_equal(np.isnan(got), ref["nan"]):
        return float("inf")
    ok = ~ref["nan"]
    err, bnd = np.abs(got - ref["O"])[ok], ref["bound"][ok]
    if not err.size:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    return float(r.max())


# ------------------------------------------------------------------------------------------------ the 16-bit arithmetic, emulated
MUTANTS = ("drop_last_key", "drop_last_fragment", "swap_v_rows", "denominator", "mask_next_row", "keep_before_denominator")


def emulate(q, k, v, H, scale, T, mask=None, keep=None, p_drop=0.0, mutant=None):
    """attn_whole_kernel's arithmetic in numpy: fp32 scores, p = exp2(s c - m c) against the row maximum with c = scale log2(e),
    the denominator from the unrounded p, `keep`, p rounded to T, fp32 P V, one division, the output rounded to T.
    `mutant` plants one of the MUTANTS."""
    assert T in ("bf16", "fp16")
    f32 = np.float32
    qh, kh, vh = _heads(q, H, f32), _heads(k, H, f32), _heads(v, H, f32)
    Tq, Tk = qh.shape[2], kh.shape[2]
    s = np.matmul(qh, kh.transpose(0, 1, 3, 2))
    if mask is not None:
        m = np.asarray(mask)
        if mutant == "mask_next_row":
            m = m[np.minimum(np.arange(Tq) + 1, Tq - 1)]
        s = np.where(m[None, None] != 0, f32(-np.inf), s)
    c = f32(f32(scale) * f32(LOG2E))
    mx = s.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        mc = np.where(np.isinf(mx), f32(0), mx * c).astype(f32)
        x = (s.astype(np.float64) * np.float64(c) - mc).astype(f32)       # one rounding: the kernel's fmaf
        p = np.exp2(x).astype(f32)
    kp = np.ones(p.shape, bool) if keep is None else np.asarray(keep)
    if mutant == "keep_before_denominator":
        p = np.where(kp, p, f32(0))
    l = p.sum(-1, keepdims=True, dtype=f32)
    p = np.where(kp, p, f32(0))
    pT = round_to(p, T)
    if mutant == "drop_last_key":
        pT[..., Tk - 1] = 0
    if mutant == "drop_last_fragment":
        pT[..., 16 * ((Tk - 1) // 16):] = 0
    if mutant == "swap_v_rows" and Tk > 1:
        i, j = Tk // 3, Tk - 1
        vh = vh.copy()
        vh[:, :, [i, j]] = vh[:, :, [j, i]]
    if mutant == "denominator":
        l = pT.sum(-1, keepdims=True, dtype=f32) * f32(1 + 2.0 ** -7)
    with np.errstate(invalid="ignore", divide="ignore"):
        o = np.matmul(pT, vh).astype(f32) * (f32(1) / (l * f32(1.0 - p_drop)))
    return round_to(_merge(o), T)
