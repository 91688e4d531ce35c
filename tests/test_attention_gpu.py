"""The attention forward kernels (csrc/attention.hip: attn_whole_kernel<NF = 13 / 17>, attn_kernel<NW = 4 / 7 / 13 / 16>) against
the float64 truth of tests/attention_ref.py at every edge of the dispatch in attention_impl.

Bound per output element (attention_ref.bound; derived there, measured ratios in DESIGN.md 5.9a): max(16 u, 4 x yardstick) A for
the fp32 arithmetic, plus 2 u_T A in 16-bit storage, plus the fp16 subnormal terms; A = sum_k P_k |v_k|.  Every output element
of every case is compared; the only rows left out are the fully masked ones, which must be NaN.  One test id per
(region, dtype, family, shape, mask, layout)."""
import numpy as np
import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 0.125
B, H = 2, 3
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = 7.25                     # exact in every storage type


# ------------------------------------------------------------------------------------------------ running one case
def ops():
    from msmd_amd import ops as _ops
    return _ops


def dev(x, T=None):
    t = torch.from_numpy(np.array(x)).to(DEV)
    return t if T is None else t.to(TD[T])


def run_gpu(q, k, v, n_heads, T, mask=None, layout="separate", **kw):
    """ops.attention on operands already rounded to T (the cast is exact); returns float64 numpy."""
    d = q.shape[-1]
    m = dev(mask) if mask is not None else None
    tq, tk, tv = dev(q, T), dev(k, T), dev(v, T)
    if layout == "packed":                      # views of one (B, T, 3 d) tensor
        qkv = torch.cat([tq, tk, tv], dim=-1)
        tq, tk, tv = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    elif layout == "kvpacked":                  # K / V views of one (B, Tk, 2 d) tensor, Tq != Tk
        kv = torch.cat([tk, tv], dim=-1)
        tk, tv = kv[..., :d], kv[..., d:]
    if layout == "out_slice":                   # the middle third of a wider, longer buffer
        Bq, Tq = q.shape[:2]
        buf = torch.full((Bq, Tq + 3, 3 * d), SENTINEL, device=DEV, dtype=TD[T])
        out = ops().attention(tq, tk, tv, n_heads, SCALE, mask=m, out=buf[:, :Tq, d:2 * d], **kw)
        torch.cuda.synchronize()
        outside = buf.clone()
        outside[:, :Tq, d:2 * d] = SENTINEL
        assert bool((outside == SENTINEL).all()), "attention wrote outside its output slab"
        assert out.data_ptr() == buf[:, :Tq, d:2 * d].data_ptr()
    else:
        out = ops().attention(tq, tk, tv, n_heads, SCALE, mask=m, **kw)
        torch.cuda.synchronize()
    return out.double().cpu().numpy()


def check(tag, q, k, v, n_heads, T, mask=None, layout="separate", probe=False, keep=None, p_drop=0.0, q_yard=None, **kw):
    """One comparison (one per 64-key window for the probe family); returns the worst err / bound."""
    worst, yard = 0.0, 0.0
    Bq, Tk = k.shape[0], k.shape[1]
    for w in range(ar.n_windows(Tk) if probe else 1):
        vw = ar.probe_v(Bq, n_heads, Tk, w) if probe else v
        ref = ar.reference(q, k, vw, n_heads, SCALE, T, mask, keep, p_drop, probe_window=w if probe else None, q_yard=q_yard)
        r = ar.ratio(run_gpu(q, k, vw, n_heads, T, mask, layout, p_drop=p_drop, **kw), ref)
        worst, yard = max(worst, r), max(yard, ref["yardstick"])
    print(f"attn {tag}: err/bound {worst:.3f}, yardstick {yard / ar.U:.2f} u")
    return worst


# ------------------------------------------------------------------------------------------------ shapes x families
def cross(tks, tqs, tq_all, tk_all):
    """Sparse cross: every Tk once with Tq = tq_all, every Tq once with each Tk of tk_all."""
    out = [(tq_all, tk) for tk in tks]
    out += [(tq, tk) for tk in tk_all for tq in tqs if (tq, tk) not in out]
    return out


SHAPES = {
    "w13": cross((1, 15, 16, 17, 31, 33, 110, 207, 208), (1, 16, 17, 111, 112, 113, 209), 17, (33, 208)),
    "w17": cross((209, 224, 250, 271, 272), (1, 144, 145, 261), 145, (209, 272)),
    "t16": cross((273, 320, 321, 512, 513), (1, 65, 250), 65, (273, 513)),
    "t32": cross((1, 63, 64, 65, 127, 129, 200), (1, 63, 64, 65), 65, (65, 200)),
}
TYPES = {"w13": ("bf16", "fp16"), "w17": ("bf16", "fp16"), "t16": ("bf16", "fp16"), "t32": ("fp32",)}

CASES = [(reg, T, fam, Tq, Tk) for reg, shapes in SHAPES.items() for (Tq, Tk) in shapes for fam in ar.FAMILIES for T in TYPES[reg]]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}x{c[4]}")
def test_forward(case):
    reg, T, fam, Tq, Tk = case
    got = ar.region(T, Tq, Tk, H, B)
    assert got[0] == reg and (reg[0] != "t" or got[1] == 4)
    q, k, v = ar.inputs(fam, B, H, Tq, Tk, T)
    assert check(f"{reg} {T} {fam} {Tq}x{Tk}", q, k, v, H, T, probe=fam == "probe",
                 q_yard=ar.yard_queries(fam, B, H, Tq, Tk, T)) <= 1.0


# ------------------------------------------------------------------------------------------------ masks
# odd and even Tk in each region; the alignment mask is (Tk + 1, Tk)
MASK_SHAPES = {"w13": ((113, 207), (113, 208)), "w17": ((145, 271), (145, 272)), "t16": ((65, 513), (65, 320)),
               "t32": ((65, 129), (65, 200))}
MASK_CASES = [(reg, T, kind, Tk + 1 if kind == "align" else Tq, Tk)
              for reg, shapes in MASK_SHAPES.items() for (Tq, Tk) in shapes for kind in ar.MASKS for T in TYPES[reg]]


@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: f"{c[0]}-{c[1]}-flat-{c[3]}x{c[4]}-{c[2]}")
def test_forward_masked(case):
    reg, T, kind, Tq, Tk = case
    assert ar.region(T, Tq, Tk, H, B)[0] == reg
    q, k, v = ar.inputs("flat", B, H, Tq, Tk, T)
    m = ar.mask(kind, Tq, Tk)
    assert check(f"{reg} {T} flat {Tq}x{Tk} mask={kind}", q, k, v, H, T, mask=m) <= 1.0
    if kind in ("first64", "lastonly", "fullrow"):       # the probabilities themselves, key by key
        assert check(f"{reg} {T} probe {Tq}x{Tk} mask={kind}", q, k, v, H, T, mask=m, probe=True) <= 1.0


def test_a_fully_masked_row_is_nan_and_nothing_else_is():
    """Today's behaviour of both kernels (0 x inf), torch's too: pinned so that a change is a decision."""
    for T, Tq, Tk in (("bf16", 113, 207), ("bf16", 65, 513), ("fp32", 65, 129)):
        q, k, v = ar.inputs("flat", B, H, Tq, Tk, T)
        o = run_gpu(q, k, v, H, T, ar.mask("fullrow", Tq, Tk))
        nan = np.isnan(o)
        assert nan[:, ar.full_row(Tq)].all() and not np.delete(nan, ar.full_row(Tq), axis=1).any()
        assert np.isfinite(np.delete(o, ar.full_row(Tq), axis=1)).all()


# ------------------------------------------------------------------------------------------------ layouts
LAYOUT_SHAPES = {"w13": (113, 207), "w17": (145, 271), "t16": (65, 321), "t32": (65, 129)}
LAYOUT_CASES = [(reg, T, lay) for reg in LAYOUT_SHAPES for lay in ("packed", "separate", "kvpacked", "out_slice") for T in TYPES[reg]]


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda c: f"{c[0]}-{c[1]}-flat-{c[2]}")
def test_forward_layouts(case):
    reg, T, lay = case
    Tq, Tk = LAYOUT_SHAPES[reg]
    Tq = Tk if lay == "packed" else Tq
    assert ar.region(T, Tq, Tk, H, B)[0] == reg
    q, k, v = ar.inputs("flat", B, H, Tq, Tk, T)
    m = ar.mask("random", Tq, Tk) if lay == "out_slice" else None
    assert check(f"{reg} {T} flat {Tq}x{Tk} layout={lay}", q, k, v, H, T, mask=m, layout=lay) <= 1.0


# ------------------------------------------------------------------------------------------------ tiled kernel, NW = 7, 13, 16
NW_CASES = [(T, nw, masked) for T in ("fp32", "bf16") for nw in (7, 13, 16) for masked in (False, True)]


@pytest.mark.parametrize("case", NW_CASES, ids=lambda c: f"{'t32' if c[0] == 'fp32' else 't16'}-nw{c[1]}-{c[0]}-flat-{'random' if c[2] else 'nomask'}")
def test_forward_tiled_wave_counts(case):
    """The only large grids of this file: ceil(workgroups / 256) x waves only leaves NW = 4 with more than 256 workgroups."""
    T, nw, masked = case
    Tq, h, b = ar.smallest_grid(nw)
    Tk = 65 if T == "fp32" else 273
    reg = ar.region(T, Tq, Tk, h, b)
    assert reg == ("t32" if T == "fp32" else "t16", nw)
    q, k, v = ar.inputs("flat", b, h, Tq, Tk, T)
    m = ar.mask("random", Tq, Tk) if masked else None
    assert check(f"{reg[0]}-nw{nw} {T} flat {Tq}x{Tk} B{b} H{h} mask={'random' if masked else None}", q, k, v, h, T, mask=m) <= 1.0


# ------------------------------------------------------------------------------------------------ prefetch
@pytest.mark.parametrize("T", ["bf16", "fp16"])
@pytest.mark.parametrize("Tq,Tk", [(111, 110), (113, 207), (145, 271), (65, 321)])
def test_prefetch_changes_no_bit(Tq, Tk, T):
    """One shape per 16-bit kernel with Tk <= 208 (7 and 13 waves), and two with Tk > 208."""
    q, k, v = (dev(x, T) for x in ar.inputs("flat", B, H, Tq, Tk, T))
    m = dev(ar.mask("random", Tq, Tk))
    ranges = [dev(ar.synth.normalish(f"attn/pf{n}", (n,))) for n in (100, 70001, 300000)]
    keep = [r.clone() for r in ranges]
    for mask in (None, m):
        plain = ops().attention(q, k, v, H, SCALE, mask=mask)
        pf = ops().attention(q, k, v, H, SCALE, mask=mask, prefetch=ranges)
        torch.cuda.synchronize()
        assert torch.equal(plain.view(torch.int16), pf.view(torch.int16))
    assert all(torch.equal(a, b) for a, b in zip(ranges, keep))


# ------------------------------------------------------------------------------------------------ dropout
DROP_CASES = [("bf16", 113, 48), ("bf16", 113, 208), ("bf16", 145, 209), ("bf16", 145, 272), ("bf16", 65, 273), ("bf16", 65, 512),
              ("fp32", 65, 65), ("fp32", 65, 200)]


def read_keep(q, k, T, p_drop, state, site):
    """The kernel's keep mask (B, H, Tq, Tk), read through the probe V one 64-key window at a time."""
    Bq, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    keep = np.zeros((Bq, H, Tq, Tk), bool)
    for w in range(ar.n_windows(Tk)):
        o = run_gpu(q, k, ar.probe_v(Bq, H, Tk, w), H, T, p_drop=p_drop, rng_state=state, site=site)
        n = min(64, Tk - 64 * w)
        keep[..., 64 * w:64 * w + n] = o.reshape(Bq, Tq, H, 64).transpose(0, 2, 1, 3)[..., :n] != 0
    return keep


@pytest.mark.parametrize("p_drop", [0.1, 0.5])
@pytest.mark.parametrize("T,Tq,Tk", DROP_CASES, ids=lambda x: str(x))
def test_dropout(T, Tq, Tk, p_drop):
    """Operands rounded to bf16 for both kernels, so that the float64 probabilities are the same: the keep mask is a function
    of (rng_state, site, batch, head, query, key) alone and must not depend on the kernel that draws it."""
    q, k, v = ar.inputs("warm", B, H, Tq, Tk, "bf16")
    state, site = torch.tensor([31, 2], dtype=torch.int64, device=DEV), 5
    keep = {TT: read_keep(q, k, TT, p_drop, state, site) for TT in ("bf16", "fp32")}
    P64, _ = ar.probabilities(q, k, H, SCALE)
    n = keep[T].size                               # bf16 and fp32 hold any probability of these inputs: kept = non-zero
    assert abs(float(keep[T].mean()) - (1 - p_drop)) <= 5.0 * (p_drop * (1 - p_drop) / n) ** 0.5
    sure = P64 > 2.0 ** -6
    assert sure.sum() >= 2500                      # the rate's standard deviation is then at most 0.01
    assert np.array_equal(keep["bf16"][sure], keep["fp32"][sure])
    rate = float(keep[T][sure].mean())
    print(f"attn dropout {T} {Tq}x{Tk} p={p_drop}: keep rate {rate:.4f} over {int(sure.sum())} entries")
    assert abs(rate - (1 - p_drop)) <= 0.03
    kw = dict(keep=keep[T], p_drop=p_drop, rng_state=state, site=site)
    reg = ar.region(T, Tq, Tk, H, B)[0]
    assert check(f"{reg}-drop {T} warm {Tq}x{Tk} p={p_drop}", q, k, v, H, T, **kw) <= 1.0
    assert check(f"{reg}-drop {T} probe {Tq}x{Tk} p={p_drop}", q, k, v, H, T, probe=True, **kw) <= 1.0
    # another site draws another mask
    other = run_gpu(q, k, v, H, T, p_drop=p_drop, rng_state=state, site=site + 1)
    assert ar.ratio(other, ar.reference(q, k, v, H, SCALE, T, keep=keep[T], p_drop=p_drop)) > 1.0


@pytest.mark.parametrize("T", ["bf16", "fp32"])
def test_dropout_past_512_keys_is_refused_and_writes_nothing(T):
    from msmd_amd import _lib
    q, k, v = (dev(x, T) for x in ar.inputs("flat", B, H, 65, 513, T))
    out = torch.full((B, 65, H * 64), SENTINEL, device=DEV, dtype=TD[T])
    state = torch.tensor([31, 2], dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.MsmdLibraryError):
        ops().attention(q, k, v, H, SCALE, out=out, p_drop=0.1, rng_state=state, site=1)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
