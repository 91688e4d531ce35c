"""Training-path kernels (csrc/backward.hip, csrc/losses.hip, the msmd_gemm_actbwd / msmd_gemm_batched2 entries of
csrc/gemm.hip) called directly and compared with float64 restatements written here from the formulas, at the shapes their
launch code branches on: the 4-wide and scalar LayerNorm backward kernels at every chunk count, 8 / 16 rows per workgroup
and the unrolled partial reduction; column sums around the 4-row unroll and the 128-row blocks; the activation grid-stride
loop; softmax rows with padding, shared masks and large logits; the AttentionFn transposes and batched products; the fused
activation-backward GEMM; and the masked sequence losses around their narrow / wide split.  Every output element is
compared.  Each tolerance is a stated bound: u = 2^-24 (fp32 unit roundoff), gamma_n = n u / (1 - n u) times the sum of
|terms| of an n-term fp32 sum, plus half an output ulp of the reference for 16-bit outputs.  16-bit inputs are rounded
first and the reference is built from the rounded values.  Moves, masks and deterministic sums are held to bit equality."""
import math

import numpy as np
import pytest
import torch

from msmd_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
TINY = 2.0 ** -125          # flushed / underflowed fp32 results (twice the smallest normal)
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTS = (torch.float32, torch.bfloat16)
ACT_NONE, ACT_GELU, ACT_ELU = 0, 1, 2


def ops():
    from msmd_amd import ops as _ops
    return _ops


def lib():
    from msmd_amd import _lib
    return _lib


def gam(n):
    return n * U / (1.0 - n * U)


def rng(tag):
    return np.random.default_rng(synth.name_seed(tag) & 0xFFFFFFFF)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def dev_in(a, dt):
    """(device tensor of dtype dt, float64 host copy of its ROUNDED values)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dt)
    return t, host(t)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def rng_state(seed=4321, step=3):
    return torch.tensor([seed, step], dtype=torch.int64, device=DEV)


def keep_mask(n, p, state, site):
    """The Philox keep mask of msmd_dropout (element / 4 indexing) for n elements, as a bool array."""
    return (ops().dropout(torch.ones(n, device=DEV), p, state, site) != 0).cpu().numpy()


def check_bound(name, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), err.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} elements outside the bound; worst at {i}: "
                             f"got {np.asarray(got)[i]!r} ref {ref[i]!r} err {err[i]:.3e} bound {bound[i]:.3e}")


# ----------------------------------------------------------------------------- 1. LayerNorm backward
def ln_bwd64(x, dy, gamma, eps, dg0, db0, out_dt):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma, two-pass statistics; dgamma = dg0 + sum_r dy xhat,
    dbeta = db0 + sum_r dy; and a first-order bound of any fp32 evaluation that forms mean, the sum of squared deviations
    from the computed mean, and the two row means of g in that order (the forms of both kernels)."""
    rows, n = x.shape
    mean = x.mean(1, keepdims=True)
    d = x - mean
    q = (d * d).sum(1, keepdims=True)
    var = q / n
    rstd = 1.0 / np.sqrt(var + eps)
    xh = d * rstd
    g = dy * gamma[None]
    m1 = g.mean(1, keepdims=True)
    m2 = (g * xh).mean(1, keepdims=True)
    T = g - m1 - xh * m2
    dx = rstd * T
    # mean: an n-term sum and the scaling by 1/n;  sum (x - mean_c)^2 = q + n (mean_c - mean)^2 exactly, each square
    # carries the rounding of x - mean_c and of the square;  rstd: var / n, + eps, sqrt and reciprocal
    e_mean = gam(n) * np.abs(x).sum(1, keepdims=True) / n + 2 * U * np.abs(mean)
    e_q = n * e_mean ** 2 + gam(n + 2) * (q + n * e_mean ** 2)
    e_r = 0.5 * (e_q / n + 3 * U * (var + eps)) / (var + eps) + 4 * U
    e_xh = rstd * (e_mean + U * np.abs(d)) + np.abs(xh) * (e_r + U)
    ag = np.abs(g)
    e_m1 = gam(n + 1) * ag.sum(1, keepdims=True) / n + 2 * U * np.abs(m1)
    e_m2 = (gam(n + 2) * np.abs(g * xh).sum(1, keepdims=True) + (ag * e_xh).sum(1, keepdims=True)) / n + 3 * U * np.abs(m2)
    e_T = U * ag + e_m1 + np.abs(xh) * e_m2 + e_xh * np.abs(m2) + 3 * U * (ag + np.abs(m1) + np.abs(xh * m2))
    bdx = rstd * (e_T + (e_r + U) * np.abs(T)) + HALF_ULP[out_dt] * np.abs(dx)
    dg = dg0 + (dy * xh).sum(0)
    bdg = (np.abs(dy) * e_xh).sum(0) + gam(rows + 1) * (np.abs(dy * xh).sum(0) + np.abs(dg0))
    db = db0 + dy.sum(0)
    bdb = gam(rows + 1) * (np.abs(dy).sum(0) + np.abs(db0))
    return (dx, bdx), (dg, bdg), (db, bdb)


def ln_inputs(tag, rows, cols, dt, mean=0.2, std=1.7, offset=0):
    g = rng(tag)
    x = (mean + std * g.standard_normal((rows, cols))).astype(np.float32)
    dy = g.standard_normal((rows, cols)).astype(np.float32)
    gamma = (1.0 + 0.3 * g.standard_normal(cols)).astype(np.float32)
    if offset:    # the rows read from a view `offset` elements into a buffer: 16-byte alignment lost
        xb = torch.zeros(rows * cols + offset, device=DEV, dtype=dt)
        xb[offset:] = torch.from_numpy(x.reshape(-1)).to(DEV).to(dt)
        xt = xb[offset:].view(rows, cols)
    else:
        xt = torch.from_numpy(x).to(DEV).to(dt)
    dyt, dy64 = dev_in(dy, dt)
    return xt, host(xt), dyt, dy64, torch.from_numpy(gamma).to(DEV), gamma.astype(np.float64)


def run_ln(tag, rows, cols, dt, accumulate=False, offset=0, eps=1e-5, **kw):
    o = ops()
    xt, x64, dyt, dy64, gt, g64 = ln_inputs(tag, rows, cols, dt, offset=offset, **kw)
    if accumulate:
        g = rng(tag + "/acc")
        dg0 = g.standard_normal(cols).astype(np.float32)
        db0 = g.standard_normal(cols).astype(np.float32)
        dgt, dbt = torch.from_numpy(dg0).to(DEV), torch.from_numpy(db0).to(DEV)
        dx, dg, db = o.layernorm_bwd(dyt, xt, gt, eps, dg_out=dgt, db_out=dbt)
        assert dg.data_ptr() == dgt.data_ptr() and db.data_ptr() == dbt.data_ptr()
    else:
        dg0 = db0 = np.zeros(cols)
        dx, dg, db = o.layernorm_bwd(dyt, xt, gt, eps)
    torch.cuda.synchronize()
    assert dx.dtype == dt and dg.dtype == torch.float32
    (rdx, bdx), (rdg, bdg), (rdb, bdb) = ln_bwd64(x64, dy64, g64, eps, np.asarray(dg0, np.float64),
                                                   np.asarray(db0, np.float64), dt)
    what = f"layernorm_bwd {dt} rows={rows} cols={cols} offset={offset}"
    check_bound(what + " dx", host(dx), rdx, bdx)
    check_bound(what + " dgamma", host(dg), rdg, bdg)
    check_bound(what + " dbeta", host(db), rdb, bdb)


COLS4 = (4, 252, 256, 260, 512, 516, 768, 772, 1024)        # 4-wide kernel: NCH = 1, 2, 3, 4 and their boundaries
COLS1 = (1, 63, 65, 67, 511, 513, 767, 769, 1023)           # scalar kernel: fp32 MAXC 8 / 16, bf16 MAXC 8 / 12 / 16
LN_ROWS = (1, 7, 9, 455, 457, 2047, 2048, 2049, 12800)      # 8 / 16 rows per workgroup; nblocks > 56 from 449 rows on


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cols", COLS4 + COLS1)
def test_layernorm_bwd_every_width(dt, cols):
    """Both kernels at every width boundary their dispatch knows, with 9 rows (one workgroup, partial) and 457 rows
    (58 workgroups: the 8-way unrolled loop of ln_partial_reduce_kernel), fresh and accumulated dgamma / dbeta."""
    for rows in (9, 457):
        run_ln(f"bwd_ln/w/{cols}/{rows}", rows, cols, dt, accumulate=rows == 457)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_bwd_every_row_count(dt, rows):
    """8 rows per workgroup below 2048 rows, 16 from 2048 on, for the 4-wide kernel (768), the scalar kernel (767) and
    the scalar kernel on the model width read through an 8-byte aligned view (768 from 2 elements in)."""
    run_ln(f"bwd_ln/r/{rows}/a", rows, 768, dt, accumulate=True)
    run_ln(f"bwd_ln/r/{rows}/b", rows, 767, dt, accumulate=rows % 2 == 1)
    run_ln(f"bwd_ln/r/{rows}/c", rows, 768, dt, offset=2 if dt == torch.float32 else 4)


@pytest.mark.parametrize("ratio", (20, 50, 100))
@pytest.mark.parametrize("cols", (256, 768, 1024, 767))
def test_layernorm_bwd_rows_with_a_large_mean(ratio, cols):
    """Rows whose mean is `ratio` times their spread (a residual stream with an offset): the row variance must not cancel.
    A one-pass sum(x^2) / n - mean^2 in fp32 puts rstd off by ~1.5e-2 at ratio 100 and ~3e-4 at ratio 50 (768 columns)."""
    for dt in DTS:
        run_ln(f"bwd_ln/ratio/{ratio}/{cols}", 64, cols, dt, mean=float(ratio), std=1.0, accumulate=True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cols", (4, 260, 768, 1024))
def test_layernorm_bwd_dropped_copy_is_the_dropout_of_dx(dt, cols):
    """msmd_layernorm_bwd_dropout: dx, dgamma, dbeta as without the copy, and dx_drop == ops.dropout(dx) bit for bit."""
    o = ops()
    state = rng_state()
    for rows in (9, 2049):
        xt, _, dyt, _, gt, _ = ln_inputs(f"bwd_ln/drop/{cols}/{rows}", rows, cols, dt)
        dx, dg, db, dxd = o.layernorm_bwd(dyt, xt, gt, drop=(0.1, state, 11))
        dx2, dg2, db2 = o.layernorm_bwd(dyt, xt, gt)
        assert torch.equal(bits(dx), bits(dx2))
        assert torch.equal(bits(dg), bits(dg2)) and torch.equal(bits(db), bits(db2))
        assert torch.equal(bits(dxd), bits(o.dropout(dx, 0.1, state, 11)))
        if rows * cols >= 4096:
            assert float((dxd == 0).float().mean()) > 0.05


def test_layernorm_bwd_refuses_what_it_cannot_do():
    o, L = ops(), lib()
    xt, _, dyt, _, gt, _ = ln_inputs("bwd_ln/refuse", 4, 1025, torch.float32)
    with pytest.raises(L.MsmdLibraryError):
        o.layernorm_bwd(dyt, xt, gt)
    xt, _, dyt, _, gt, _ = ln_inputs("bwd_ln/refuse2", 4, 766, torch.float32)
    with pytest.raises(L.MsmdLibraryError):      # the dropped copy exists in the 4-wide kernel only
        o.layernorm_bwd(dyt, xt, gt, drop=(0.1, rng_state(), 1))


# ----------------------------------------------------------------------------- 2. column sums
CS_CASES = [(r, c) for r in (1, 3, 4, 5, 127, 128, 129, 2047, 2049) for c in (1, 65, 257)] + \
           [(129, c) for c in (63, 64, 255, 256, 1000)] + [(2049, 1000), (100000, 64), (100000, 65)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,cols", CS_CASES)
def test_colsum(dt, rows, cols):
    """out (+)= sum_r x[r, c] through a strided view (ld = cols + 37): the deterministic two-launch form (twice, bit
    identical) and the atomic form (ws = NULL), fresh and accumulated; gamma_{rows+1} sum |terms| each."""
    o, L = ops(), lib()
    g = rng(f"bwd_colsum/{rows}/{cols}")
    ld = cols + 37
    base, b64 = dev_in(g.standard_normal((rows, ld)) * 3.0 + 0.5, dt)
    x, x64 = base[:, :cols], b64[:, :cols]
    out0 = g.standard_normal(cols).astype(np.float32)
    for acc in (False, True):
        init = out0 if acc else np.full(cols, np.nan, np.float32)   # a fresh sum must not read what was there
        ref = x64.sum(0) + (out0 if acc else 0.0)
        bound = gam(rows + 1) * (np.abs(x64).sum(0) + (np.abs(out0) if acc else 0.0))
        a = torch.from_numpy(init).to(DEV)
        o.colsum(x, a, accumulate=acc)
        b = torch.from_numpy(init).to(DEV)
        o.colsum(x, b, accumulate=acc)
        c = torch.from_numpy(init).to(DEV)
        L.check(L.load().msmd_colsum(x.data_ptr(), c.data_ptr(), rows, cols, ld, int(acc), o._dt(x), None, 0,
                                     o._stream()), "msmd_colsum")
        torch.cuda.synchronize()
        assert torch.equal(bits(a), bits(b))
        check_bound(f"colsum {dt} {rows}x{cols} acc={acc}", host(a), ref, bound)
        check_bound(f"colsum (atomic) {dt} {rows}x{cols} acc={acc}", host(c), ref, bound)


# ----------------------------------------------------------------------------- 3. activations
def phi64(z):
    """(Phi(z), z phi(z)) in float64 (Phi through erfc: no cancellation in the lower tail)."""
    zt = torch.from_numpy(z)
    Phi = (0.5 * torch.special.erfc(-zt / math.sqrt(2.0))).numpy()
    return Phi, z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def act64(z, act):
    """(act(z), act'(z), bound of the fp32 forward, bound of the fp32 derivative) -- libm erff / expf / expm1f within
    2 ulp; the derivative's erf term is within 4u absolute (a 2-ulp error of erf near +-1 survives 1 + erf), its
    z phi(z) term carries the rounding of -z^2 / 2 amplified by exp: (z^2 + 8) u relative."""
    if act == ACT_GELU:
        Phi, zphi = phi64(z)
        return (z * Phi, Phi + zphi, 4 * U * np.abs(z) + 2 * U * np.abs(z * Phi),
                4 * U + (z * z + 8) * U * (np.abs(Phi) + np.abs(zphi)))
    if act == ACT_ELU:
        e = np.exp(np.minimum(z, 0.0))
        y = np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
        return y, np.where(z > 0, 1.0, e), 4 * U * np.abs(y), np.where(z > 0, 0.0, 4 * U * e)
    return z, np.ones_like(z), np.zeros_like(z), np.zeros_like(z)


ACT_NS = (1, 3, 255, 257, 8192 * 256 + 4099)


def act_z(tag, n):
    g = rng(tag)
    z = g.uniform(-12.0, 12.0, n)
    z[: min(n, 3)] = (0.0, 1e-30, -1e-30)[: min(n, 3)]
    if n > 1000:
        z[3:1003] = np.linspace(-1.5, 0.0, 1000)         # around GELU''s zero at z ~ -0.75
    return z.astype(np.float32)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act", (ACT_GELU, ACT_ELU))
@pytest.mark.parametrize("n", ACT_NS)
def test_activation_forward_backward_and_dropout_backward(dt, act, n):
    o = ops()
    zt, z = dev_in(act_z(f"bwd_act/{n}/z", n), dt)
    dyt, dy = dev_in(rng(f"bwd_act/{n}/dy").standard_normal(n), dt)
    y, dg, by, bg = act64(z, act)
    h = HALF_ULP[dt]
    check_bound(f"act_fwd {act} {dt} n={n}", host(o.act_fwd(zt, act)), y, by + h * np.abs(y))
    ref = dy * dg
    bound = np.abs(dy) * bg + 2 * U * np.abs(ref) + h * np.abs(ref)
    check_bound(f"act_bwd {act} {dt} n={n}", host(o.act_bwd(dyt, zt, act)), ref, bound)
    p, state, site = 0.1, rng_state(77, 5), 9
    got = host(o.act_bwd_dropout(dyt, zt, act, p, state, site))
    keep = keep_mask(n, p, state, site)
    assert np.all(got[~keep] == 0.0)
    c = 1.0 / (1.0 - p)
    check_bound(f"act_bwd_dropout {act} {dt} n={n}", got[keep], (c * ref)[keep],
                (c * (bound + 2 * U * np.abs(ref)))[keep])


def test_activation_dropout_backward_mask_at_ragged_lengths():
    """The mask of act_bwd_dropout is the mask of msmd_dropout (element / 4) exactly, with n % 4 != 0."""
    o = ops()
    state = rng_state(99, 1)
    for n in (5, 1023, 70001):
        z = torch.ones(n, device=DEV)
        dy = torch.ones(n, device=DEV)
        got = o.act_bwd_dropout(dy, z, ACT_NONE, 0.3, state, 4)
        assert torch.equal(got != 0, o.dropout(torch.ones(n, device=DEV), 0.3, state, 4) != 0)


# ----------------------------------------------------------------------------- 4. softmax rows
SM_COLS = (1, 63, 64, 65, 110, 256, 257, 600)


def softmax64(s, scale, mask_rows):
    v = s * scale
    v = np.where(mask_rows, -np.inf, v)
    mx = v.max(1, keepdims=True)
    e = np.exp(v - mx)
    P = e / e.sum(1, keepdims=True)
    vf = np.where(mask_rows, 0.0, v)
    ec = U * (np.abs(vf) + np.abs(np.where(mask_rows, 0.0, v - mx))) + 4 * U
    ec = np.where(mask_rows, 0.0, ec)
    n = s.shape[1]
    bound = P * (ec + ec.max(1, keepdims=True) + gam(n) + 2 * U) + TINY
    return P, bound


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cols", SM_COLS)
def test_softmax_rows_forward_and_backward(dt, cols):
    """21 rows (not a multiple of 4) = 3 x Tq with Tq = 7: the byte mask is shared by row % Tq; scaled logits up to +-80;
    ld = cols rounded up to 8 and cols + 64, padding columns pre-filled with garbage must come back zero.  The backward
    against scale P o (dP - rowsum(P o dP)) in float64 from the stored P."""
    o = ops()
    Tq, rows, scale = 7, 21, 0.125
    g = rng(f"bwd_sm/{cols}")
    amp = np.where(np.arange(rows) % 2 == 0, 80.0, 4.0)[:, None] / scale
    s_np = (g.uniform(-1.0, 1.0, (rows, cols)) * amp).astype(np.float32)
    m = (g.uniform(size=(Tq, cols)) < 0.3).astype(np.uint8)
    m[np.arange(Tq), g.integers(0, cols, Tq)] = 0                  # every mask row keeps at least one column
    for ld in ((cols + 7) // 8 * 8, cols + 64):
        for masked in (False, True):
            buf = torch.full((rows, ld), 7.0, device=DEV, dtype=dt)
            buf[:, :cols] = torch.from_numpy(s_np).to(DEV).to(dt)
            s64 = host(buf[:, :cols])
            mt = torch.from_numpy(m).to(DEV) if masked else None
            o.softmax_rows_(buf, cols, ld, Tq if masked else 1, scale, mt)
            mrows = m[np.arange(rows) % Tq].astype(bool) if masked else np.zeros((rows, cols), bool)
            P, bound = softmax64(s64, scale, mrows)
            got = host(buf)
            what = f"softmax_rows {dt} cols={cols} ld={ld} masked={masked}"
            assert np.all(got[:, cols:] == 0.0), what + ": padding"
            assert np.all(got[:, :cols][mrows] == 0.0), what + ": masked"
            check_bound(what, got[:, :cols], P, bound + HALF_ULP[dt] * P)
            # backward from the stored P
            Pst = got[:, :cols]
            dP = torch.full((rows, ld), -3.0, device=DEV, dtype=dt)
            dP[:, :cols] = torch.from_numpy(g.standard_normal((rows, cols)).astype(np.float32)).to(DEV).to(dt)
            d64 = host(dP[:, :cols])
            o.softmax_bwd_rows_(buf, dP, cols, ld, scale)
            dot = (Pst * d64).sum(1, keepdims=True)
            ref = scale * Pst * (d64 - dot)
            e_dot = gam(cols + 1) * np.abs(Pst * d64).sum(1, keepdims=True)
            bnd = scale * Pst * (e_dot + 3 * U * np.abs(d64 - dot)) + TINY * scale * (np.abs(d64) + np.abs(dot) + 1)
            got = host(dP)
            assert np.all(got[:, cols:] == 0.0), what + ": backward padding"
            check_bound(what + " backward", got[:, :cols], ref, bnd + HALF_ULP[dt] * np.abs(ref))


# ----------------------------------------------------------------------------- 5. transposes and the unfold
TR_DIMS = (1, 63, 64, 65, 130)
SENT = {torch.float32: -12345.5, torch.bfloat16: -123.5, torch.float16: -123.5}


@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16, torch.float16))
@pytest.mark.parametrize("rows", TR_DIMS)
def test_transpose_batched_strided_bit_exact(dt, rows):
    """y[zo][zi][c][r] = x[zo][zi][r][c] with two-level batch strides and leading dimensions above the extents; every
    element the call must not write keeps its sentinel."""
    o = ops()
    for cols in TR_DIMS:
        bo, bi, ldx, ldy = 2, 3, cols + 3, rows + 5
        sxi, syi = rows * ldx + 7, cols * ldy + 9
        sx, sy = bi * sxi + 11, bi * syi + 13
        g = rng(f"bwd_tr/{rows}/{cols}")
        x = torch.from_numpy(g.standard_normal(bo * sx).astype(np.float32)).to(DEV).to(dt)
        y = torch.full((bo * sy,), SENT[dt], device=DEV, dtype=dt)
        o.transpose(x, y, rows, cols, ldx, ldy, bo, sx, sy, bi, sxi, syi)
        xh, yh = bits(x).cpu().numpy(), bits(y).cpu().numpy()
        want = np.full_like(yh, bits(torch.tensor([SENT[dt]], dtype=dt)).item())
        for zo in range(bo):
            for zi in range(bi):
                xs = np.lib.stride_tricks.as_strided(xh[zo * sx + zi * sxi:], (rows, cols), (ldx * xh.itemsize, xh.itemsize))
                ys = np.lib.stride_tricks.as_strided(want[zo * sy + zi * syi:], (cols, rows), (ldy * want.itemsize, want.itemsize))
                ys[...] = xs.T
        assert np.array_equal(yh, want), f"transpose {dt} {rows}x{cols}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Tk", (1, 63, 64, 65, 110, 130))
def test_transpose_attention_operands_and_transpose2d(dt, Tk):
    """AttentionFn's V^T: v (B, Tk, H*64) a view of a packed K|V tensor -> (B, H, 64, Tkp), columns >= Tk untouched; and
    ops.transpose2d, whose padding must be zeros."""
    o = ops()
    B, H = 3, 8
    d, Tkp = H * 64, (Tk + 7) // 8 * 8
    kv = torch.from_numpy(rng(f"bwd_trv/{Tk}").standard_normal((B, Tk, 2 * d)).astype(np.float32)).to(DEV).to(dt)
    v = kv[..., d:]
    VT = torch.full((B, H, 64, Tkp), SENT[dt], device=DEV, dtype=dt)
    o.transpose(v, VT, Tk, 64, v.stride(1), Tkp, B, v.stride(0), H * 64 * Tkp, H, 64, 64 * Tkp)
    want = v.reshape(B, Tk, H, 64).permute(0, 2, 3, 1)
    assert torch.equal(bits(VT[..., :Tk]), bits(want))
    assert torch.all(VT[..., Tk:] == SENT[dt])
    x2 = kv[0, :, :100]
    t2 = o.transpose2d(x2)
    assert t2.shape == (100, Tkp)
    assert torch.equal(bits(t2[:, :Tk]), bits(x2.t())) and torch.all(t2[:, Tk:] == 0)


@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16, torch.float16))
@pytest.mark.parametrize("B,T,G,Cg,Kk,extra", [(3, 37, 16, 48, 128, 0), (1, 1, 1, 1, 1, 0), (2, 5, 3, 7, 3, 2),
                                               (1, 9, 2, 5, 4, 1), (2, 64, 16, 48, 128, 3)])
def test_unfold_t_bit_exact(dt, B, T, G, Cg, Kk, extra):
    """out[g][kk Cg + ci][b T + t] = xp[b][g][t + kk][ci], the Mp - B T padding columns zero (out is torch.empty)."""
    o = ops()
    Tp = T + Kk - 1 + extra
    xp = torch.from_numpy(rng(f"bwd_unf/{B}/{T}/{G}").standard_normal((B, G, Tp, Cg)).astype(np.float32)).to(DEV).to(dt)
    out = o.unfold_t(xp, T, Kk)
    Mp = (B * T + 7) // 8 * 8
    assert out.shape == (G, Kk * Cg, Mp)
    xh = bits(xp).cpu().numpy()
    t = np.arange(T)
    win = xh[:, :, t[:, None] + np.arange(Kk)[None], :]                 # (B, G, T, Kk, Cg)
    want = np.zeros((G, Kk * Cg, Mp), xh.dtype)
    want[:, :, :B * T] = win.transpose(1, 3, 4, 0, 2).reshape(G, Kk * Cg, B * T)
    assert np.array_equal(bits(out).cpu().numpy(), want)


# ----------------------------------------------------------------------------- 6. batched products (AttentionFn)
@pytest.mark.parametrize("dt", DTS)
def test_gemm_batched2_attention_products(dt):
    """P = Q K^T per (batch, head) on packed views (B = 3, H = 8, Tq = 111, Tk = 110 -> Tkp = 112: columns >= Tk keep the
    sentinel) and O = P V over the zero-padded Tkp (written through ldc = d + 16: the gap keeps the sentinel); bound
    gamma_{K+1} sum_k |a_k b_k| plus the output's half ulp."""
    o = ops()
    B, H, Tq, Tk = 3, 8, 111, 110
    d, Tkp = H * 64, 112
    g = rng(f"bwd_gb2/{dt}")
    qkv, qkv64 = dev_in(g.standard_normal((B, Tq, 3 * d)), dt)
    kv, kv64 = dev_in(g.standard_normal((B, Tk, 2 * d)), dt)
    q, k = qkv[..., :d], kv[..., :d]
    P = torch.full((B, H, Tq, Tkp), SENT[dt], device=DEV, dtype=dt)
    o.gemm_batched2(q, k, P, Tq, Tk, 64, q.stride(1), k.stride(1), Tkp, B, q.stride(0), k.stride(0), H * Tq * Tkp,
                    H, 64, 64, Tq * Tkp)
    q4 = qkv64[..., :d].reshape(B, Tq, H, 64)
    k4 = kv64[..., :d].reshape(B, Tk, H, 64)
    ref = np.einsum("bihc,bjhc->bhij", q4, k4, optimize=True)
    bound = gam(65) * np.einsum("bihc,bjhc->bhij", np.abs(q4), np.abs(k4), optimize=True) + HALF_ULP[dt] * np.abs(ref)
    check_bound(f"gemm_batched2 QK^T {dt}", host(P[..., :Tk]), ref, bound)
    assert torch.all(P[..., Tk:] == SENT[dt])
    # O = P V: A (B, H, Tq, Tkp), W = V^T (B, H, 64, Tkp), both zero in the padded columns
    Pa = np.zeros((B, H, Tq, Tkp), np.float32)
    Pa[..., :Tk] = g.uniform(0.0, 1.0, (B, H, Tq, Tk))
    VTa = np.zeros((B, H, 64, Tkp), np.float32)
    VTa[..., :Tk] = g.standard_normal((B, H, 64, Tk))
    Pt, P64 = dev_in(Pa, dt)
    VTt, VT64 = dev_in(VTa, dt)
    ldc = d + 16
    O = torch.full((B, Tq, ldc), SENT[dt], device=DEV, dtype=dt)
    o.gemm_batched2(Pt, VTt, O, Tq, 64, Tkp, Tkp, Tkp, ldc, B, H * Tq * Tkp, H * 64 * Tkp, Tq * ldc, H, Tq * Tkp,
                    64 * Tkp, 64)
    ref = np.einsum("bhij,bhcj->bihc", P64, VT64, optimize=True).reshape(B, Tq, d)
    bound = gam(Tkp + 1) * np.einsum("bhij,bhcj->bihc", np.abs(P64), np.abs(VT64), optimize=True).reshape(B, Tq, d) + \
        HALF_ULP[dt] * np.abs(ref)
    check_bound(f"gemm_batched2 PV {dt}", host(O[..., :d]), ref, bound)
    assert torch.all(O[..., d:] == SENT[dt])


# ----------------------------------------------------------------------------- 7. fused activation-backward GEMM
GAB_SHAPES = [(1, 8, 64), (1, 3072, 768), (37, 68, 768), (37, 8, 3072), (37, 3072, 64), (3552, 68, 64),
              (3552, 3072, 768), (3552, 8, 3072), (12800, 68, 3072), (12800, 3072, 768)]


def act_grad_fast64(z, act):
    """(act'(z), bound of the epilogue's evaluation): erf by Abramowitz-Stegun 7.1.26 (1.5e-7 absolute) and v_exp_f32
    ((|x| + 8) u relative for exp(x))."""
    if act == ACT_GELU:
        Phi = 0.5 * torch.special.erfc(-z / math.sqrt(2.0))
        zphi = z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        return Phi + zphi, 1.5e-7 + 8 * U + (z * z + 16) * U * (Phi.abs() + zphi.abs())
    if act == ACT_ELU:
        e = torch.exp(torch.clamp(z, max=0.0))
        return torch.where(z > 0, torch.ones_like(z), e), torch.where(z > 0, torch.zeros_like(z), (z.abs() + 8) * U * e)
    return torch.ones_like(z), torch.zeros_like(z)


@pytest.mark.parametrize("dt", (torch.bfloat16, torch.float16))
@pytest.mark.parametrize("M,N,K", GAB_SHAPES)
def test_gemm_act_bwd(dt, M, N, K):
    """dz = keep / (1 - p) act'(z) (dy @ wt^T) against float64 (on the device) for NONE / GELU / ELU and p = 0 / 0.1;
    bound |act'| gamma_{K+1} sum_k |dy_k w_k| + |dy @ wt^T| e_act + 3u |dz| + the output's half ulp (+ fp16 subnormal
    spacing / 2)."""
    o = ops()
    g = torch.Generator(device="cpu").manual_seed(synth.name_seed(f"bwd_gab/{M}/{N}/{K}") & 0x7FFFFFFF)
    dy = torch.randn(M, K, generator=g).to(DEV).to(dt)
    wt = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV).to(dt)
    z = (torch.rand(M, N, generator=g) * 12.0 - 6.0).to(DEV).to(dt)
    dy64, wt64, z64 = dy.double(), wt.double(), z.double()
    acc = dy64 @ wt64.t()
    acc_abs = dy64.abs() @ wt64.abs().t()
    state = rng_state(555, 2)
    for act in (ACT_NONE, ACT_GELU, ACT_ELU):
        dg, e_act = act_grad_fast64(z64, act)
        for p in (0.0, 0.1):
            got = o.gemm_act_bwd(dy, wt, z, act, p, state if p else None, 21)
            c = 1.0 / (1.0 - p)
            ref = c * dg * acc
            bound = c * (dg.abs() * gam(K + 1) * acc_abs + acc.abs() * e_act) + 3 * U * ref.abs() + \
                HALF_ULP[dt] * ref.abs() + (2.0 ** -25 if dt == torch.float16 else 0.0)
            if p:
                keep = torch.from_numpy(keep_mask(M * N, p, state, 21)).to(DEV).view(M, N)
                assert torch.all(got[~keep] == 0)
                ref, bound = torch.where(keep, ref, torch.zeros_like(ref)), torch.where(keep, bound, torch.zeros_like(bound))
            err = (got.double() - ref).abs()
            bad = ~(err <= bound)
            assert not bool(bad.any()), (f"gemm_act_bwd {dt} {M}x{N}x{K} act={act} p={p}: {int(bad.sum())} elements out; "
                                         f"worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}")


def test_gemm_act_bwd_refuses_unsupported_shapes():
    o, L = ops(), lib()
    dy = torch.randn(16, 96, device=DEV).bfloat16()
    with pytest.raises(L.MsmdLibraryError):      # K % 64
        o.gemm_act_bwd(dy, torch.randn(8, 96, device=DEV).bfloat16(), torch.randn(16, 8, device=DEV).bfloat16(), ACT_GELU)
    dy = torch.randn(16, 64, device=DEV).bfloat16()
    with pytest.raises(L.MsmdLibraryError):      # N % 4
        o.gemm_act_bwd(dy, torch.randn(6, 64, device=DEV).bfloat16(), torch.randn(16, 6, device=DEV).bfloat16(), ACT_GELU)


# ----------------------------------------------------------------------------- 8. weight-arena cast + transpose
def test_cast_transpose_multi_at_multiples_of_8():
    """N and K multiples of 8 but not of 32 (ragged 32 x 32 tiles on both axes): cast == w.bfloat16() and
    transposed == w.t().bfloat16() bit for bit; the arena gaps keep their sentinel."""
    o = ops()
    shapes = [(8, 8), (72, 40), (520, 776), (32, 8), (8, 104)]
    g = rng("bwd_ctm")
    rows, src, dst, tiles = [], 5, 3, 0
    for N, K in shapes:
        rows.append((src, N, K, dst, dst + 1, tiles))
        src += N * K + 13
        dst += N * K + 64
        tiles += ((N + 31) // 32) * ((K + 31) // 32)
    flat = torch.from_numpy(g.standard_normal(src + 7).astype(np.float32)).to(DEV)
    meta = torch.tensor(rows, dtype=torch.int64, device=DEV)
    cast = torch.full((dst + 8,), -123.5, device=DEV, dtype=torch.bfloat16)
    tr = torch.full((dst + 8,), -123.5, device=DEV, dtype=torch.bfloat16)
    o.cast_transpose_multi(flat, meta, len(shapes), tiles, cast, tr)
    want_c = cast.clone().fill_(-123.5)
    want_t = tr.clone().fill_(-123.5)
    for s, N, K, dc, dtr, _ in rows:
        w = flat[s:s + N * K].view(N, K)
        want_c[dc:dc + N * K] = w.bfloat16().reshape(-1)
        want_t[dtr:dtr + N * K] = w.t().bfloat16().reshape(-1)
    assert torch.equal(bits(cast), bits(want_c))
    assert torch.equal(bits(tr), bits(want_t))


# ----------------------------------------------------------------------------- 9. losses
def diff64(a, order):
    if order == 0:
        return a
    if order == 1:
        return a[:, 1:] - a[:, :-1]
    return (a[:, 2:] - a[:, 1:-1]) - (a[:, 1:-1] - a[:, :-2])


def diff32(a, order):
    """The kernel's fp32 difference, bit for bit (no products: nothing to contract)."""
    a = a.astype(np.float32)
    if order == 0:
        return a
    if order == 1:
        return a[:, 1:] - a[:, :-1]
    return (a[:, 2:] - a[:, 1:-1]) - (a[:, 1:-1] - a[:, :-2])


def loss_valid(N, T, order, prefix, end_idx):
    """(N, T - order) rows that count: the first |prefix| frames always (prefix > 0) or never (prefix < 0); later frames
    while (t + order - |prefix|) < end_idx[n] (end_idx None: T - |prefix|)."""
    pf = abs(prefix)
    tm = np.arange(order, T)[None]
    e = (np.asarray(end_idx)[:, None] if end_idx is not None else np.full((N, 1), T - pf))
    return ((prefix > 0) & (tm < pf)) | ((tm >= pf) & ((tm - pf) < e))


def loss_e_d(g, p, order, mode):
    """Bound of the kernel's fp32 difference d = D gt - D pred: each subtraction rounds once, its operands are at most
    2^order max|values| (D gt = 0 in mode 1)."""
    return 4 * U * 2.0 ** order * (np.abs(g).max() * (mode == 0) + np.abs(p).max())


def masked_loss64(gt, pred, end_idx, c_lo, c_hi, order, prefix, crit, mode, scale):
    """(loss, bound, valid): float64 from the formulas.  The bound adds the rounding of the fp32 differences and terms,
    and gamma_m of the fp32 running sums, m = the longest chain of fp32 additions a term can take (a lane's running sum
    over every row it visits, then the wave / workgroup reduction), and the final fp32 rounding."""
    N, T, _ = pred.shape
    nc = c_hi - c_lo
    g, p = gt[..., c_lo:c_hi], pred[..., c_lo:c_hi]
    d = (0.0 if mode == 1 else diff64(g, order)) - diff64(p, order)
    e_d = loss_e_d(g, p, order, mode)
    valid = loss_valid(N, T, order, prefix, end_idx)
    cnt = valid.sum()
    if cnt == 0:
        return float("nan") if order == 0 else 0.0, 0.0, valid
    term = d * d if crit == 0 else np.abs(d)
    e_term = (2 * np.abs(d) * e_d + e_d * e_d + U * d * d) if crit == 0 else np.full_like(d, e_d)
    m = N * T * ((nc + 63) // 64) + 16
    tot = term[valid].sum()
    loss = scale * tot / (cnt * nc)
    bound = abs(scale) * (e_term[valid].sum() + gam(m) * (tot + e_term[valid].sum())) / (cnt * nc) + 2 * U * abs(loss)
    return loss, bound, valid


def masked_loss_grad64(valid, d32, d64, e_d, T, order, crit, scale, up):
    """d loss / d pred[n, tau, c] = -scale up / (cnt nc) sum_k s_k crit'(d[n, tau - k, c]) over the valid rows tau - k,
    with s = (1), (-1, 1), (1, -2, 1) the difference stencil (d[t] depends on pred[t + k] through -s_k); the sign of an
    L1 difference is taken from the kernel's own fp32 difference d32.  Bound: the error 2 e_d of each L2 derivative, a
    3-term fp32 fma chain (gamma_3) and the 3u of the fp32 scale factor and product."""
    N, Td, nc = d64.shape
    cnt = valid.sum()
    stencil = {0: (1.0,), 1: (-1.0, 1.0), 2: (1.0, -2.0, 1.0)}[order]
    dc = (2.0 * d64 if crit == 0 else np.sign(d32).astype(np.float64)) * valid[..., None]
    e_dc = (2.0 * e_d if crit == 0 else 0.0) * valid[..., None]
    g0 = -scale * up / (cnt * nc)
    a, ab, ae = np.zeros((N, T, nc)), np.zeros((N, T, nc)), np.zeros((N, T, nc))
    for k, s in enumerate(stencil):
        a[:, k:k + Td] += s * dc
        ab[:, k:k + Td] += abs(s) * np.abs(dc)
        ae[:, k:k + Td] += abs(s) * e_dc
    ref = g0 * a
    return ref, abs(g0) * (ae + gam(3) * ab) + 3 * U * np.abs(ref)


LOSS_NC = (1, 67, 256, 257, 1023, 1024, 15069)


@pytest.mark.parametrize("nc", LOSS_NC)
@pytest.mark.parametrize("order", (0, 1, 2))
def test_masked_seq_loss_forward_and_backward(nc, order):
    """msmd_masked_seq_loss / _bwd at channel widths around the narrow (<= 256) / wide split and the 64 -> 256-thread
    switch (1024), c_lo = 3, prefix +2 / 0 / -2, both criteria, both modes, end_idx at order + 1 and at T.  The gradient
    is added into a pre-filled buffer; channels outside [c_lo, c_hi) keep their bits."""
    o = ops()
    N, T, c_lo = 3, 12, 3
    C = c_lo + nc + 2
    g = rng(f"bwd_loss/{nc}/{order}")
    gt = g.standard_normal((N, T, C)).astype(np.float32)
    pred = g.standard_normal((N, T, C)).astype(np.float32)
    gtt, predt = torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV)
    pre = g.standard_normal((N, T, C)).astype(np.float32)
    up = 0.75
    for end in (None, [order + 1, T, 5]):
        et = None if end is None else torch.tensor(end, dtype=torch.int32, device=DEV)
        for prefix in (2, 0, -2):
            for crit in (0, 1):
                for mode in (0, 1):
                    what = f"masked_seq_loss nc={nc} order={order} end={end} prefix={prefix} crit={crit} mode={mode}"
                    loss, ws = o.masked_seq_loss(gtt, predt, et, c_lo, c_lo + nc, order, prefix, crit, mode, 1.5,
                                                 return_ws=True)
                    ref, bound, valid = masked_loss64(gt.astype(np.float64), pred.astype(np.float64), end, c_lo,
                                                      c_lo + nc, order, prefix, crit, mode, 1.5)
                    assert abs(float(loss) - ref) <= bound, (what, float(loss), ref, bound)
                    grad = torch.from_numpy(pre).to(DEV)
                    o.masked_seq_loss_bwd_(grad, gtt, predt, et, ws, torch.tensor(up, device=DEV), c_lo, c_lo + nc,
                                           order, prefix, crit, mode, 1.5)
                    gh = grad.cpu().numpy()
                    assert np.array_equal(gh[..., :c_lo].view(np.int32), pre[..., :c_lo].view(np.int32)), what
                    assert np.array_equal(gh[..., c_lo + nc:].view(np.int32), pre[..., c_lo + nc:].view(np.int32)), what
                    g32, p32 = gt[..., c_lo:c_lo + nc], pred[..., c_lo:c_lo + nc]
                    g64, p64 = g32.astype(np.float64), p32.astype(np.float64)
                    d64 = (0.0 if mode == 1 else diff64(g64, order)) - diff64(p64, order)
                    d32 = (np.float32(0.0) if mode == 1 else diff32(g32, order)) - diff32(p32, order)
                    rg, bg = masked_loss_grad64(valid, d32, d64, loss_e_d(g64, p64, order, mode), T, order, crit,
                                                1.5, up)
                    base = pre[..., c_lo:c_lo + nc].astype(np.float64)
                    check_bound(what + " grad", gh[..., c_lo:c_lo + nc], base + rg, bg + U * np.abs(base + rg))


@pytest.mark.parametrize("order", (0, 1, 2))
def test_masked_seq_loss_empty_selection(order):
    """No valid row: NaN at order 0 (torch's mean of nothing), 0 at order > 0 (the reference's None terms); the backward
    adds nothing."""
    o = ops()
    for nc in (67, 1024):
        N, T, C = 2, 9, nc + 1
        gt = torch.randn(N, T, C, device=DEV)
        pred = torch.randn(N, T, C, device=DEV)
        end = torch.zeros(N, dtype=torch.int32, device=DEV)
        for prefix in (0, -3):
            loss, ws = o.masked_seq_loss(gt, pred, end, 1, 1 + nc, order, prefix, 0, 0, 1.0, return_ws=True)
            v = float(loss)
            assert (math.isnan(v) if order == 0 else v == 0.0), (order, nc, prefix, v)
            grad = torch.randn(N, T, C, device=DEV)
            before = grad.clone()
            o.masked_seq_loss_bwd_(grad, gt, pred, end, ws, torch.tensor(1.0, device=DEV), 1, 1 + nc, order, prefix)
            assert torch.equal(bits(grad), bits(before))


@pytest.mark.parametrize("n", (1, 255, 65537))
def test_kl_loss(n):
    """-0.5 sum(1 + logvar - mu^2 - exp(logvar)): per-term rounding (four operations, expf within 2 ulp), an fp32 block
    sum (gamma_n) and the final rounding."""
    g = rng(f"bwd_kl/{n}")
    mu = g.standard_normal(n).astype(np.float32)
    lv = (0.5 * g.standard_normal(n)).astype(np.float32)
    m64, l64 = mu.astype(np.float64), lv.astype(np.float64)
    t = 1.0 + l64 - m64 * m64 - np.exp(l64)
    ref = -0.5 * t.sum()
    e_t = U * (np.abs(1 + l64) + np.abs(1 + l64 - m64 * m64) + np.abs(t) + m64 * m64) + 4 * U * np.exp(l64)
    bound = 0.5 * (e_t.sum() + gam(n) * (np.abs(t).sum() + e_t.sum())) + U * abs(ref)
    got = float(ops().kl_loss(torch.from_numpy(mu).to(DEV), torch.from_numpy(lv).to(DEV)))
    assert abs(got - ref) <= bound, (got, ref, bound)


@pytest.mark.parametrize("unit,inner", [(1, 1), (3, 1), (1, 5), (4, 7)])
def test_truncate_rows_bit_exact(unit, inner):
    """x[n, end[n] unit:] = 0 or the last kept value (replicate), bit for bit; the kept prefix untouched."""
    o = ops()
    N, L = 4, 24
    end = np.array([1, L // unit, 3, 2], np.int32)
    et = torch.from_numpy(end).to(DEV)
    x = rng(f"bwd_trunc/{unit}/{inner}").standard_normal((N, L, inner)).astype(np.float32)
    for rep in (False, True):
        xt = torch.from_numpy(x).to(DEV)
        o.truncate_rows_(xt, et, unit, rep)
        want = x.copy()
        for n in range(N):
            e = end[n] * unit
            want[n, e:] = want[n, e - 1] if rep else 0.0
        assert np.array_equal(xt.cpu().numpy().view(np.int32), want.view(np.int32)), (unit, inner, rep)


# ----------------------------------------------------------------------------- 10. dtype codes
def test_backward_entries_refuse_fp16():
    """The training kernels are fp32 / bf16 only: fp16 storage is refused, not read as bf16."""
    o, L = ops(), lib()
    h = torch.randn(8, 64, device=DEV).half()
    with pytest.raises(L.MsmdLibraryError):
        o.act_bwd(h, h, ACT_GELU)
    with pytest.raises(L.MsmdLibraryError):
        o.act_fwd(h, ACT_GELU)
    with pytest.raises(L.MsmdLibraryError):
        o.layernorm_bwd(h, h, torch.ones(64, device=DEV))
    with pytest.raises(L.MsmdLibraryError):
        o.colsum(h)
    with pytest.raises(L.MsmdLibraryError):
        o.softmax_rows_(h, 64, 64, 1, 1.0)
    with pytest.raises(L.MsmdLibraryError):
        o.softmax_bwd_rows_(h, h.clone(), 64, 64, 1.0)
    with pytest.raises(L.MsmdLibraryError):
        o.dropout(h, 0.1, rng_state(), 1)
    with pytest.raises(L.MsmdLibraryError):
        o.act_bwd_dropout(h, h, ACT_GELU, 0.1, rng_state(), 1)
