"""The attention tests' numpy truth (tests/attention_ref.py) pinned by closed forms, and its bound proved to bite: an emulator of
the kernels' 16-bit arithmetic stays inside the bound on every input family, and every planted mutant of it leaves the bound on
the family named for it.  Every output element of every case is compared."""
import numpy as np
import pytest

import attention_ref as ar

SCALE = 0.125
B, H = 2, 2
# the smallest shape of each family that still has a ragged last fragment and, for the ramps, more than one 64-key tile
SHAPES = {"flat": (17, 33), "peaked": (17, 33), "rampup": (17, 129), "rampdown": (17, 129), "probe": (17, 33)}


def _mask_rows(Tq, Tk):
    m = np.zeros((Tq, Tk), np.uint8)
    m[::2, 1::2] = 1
    return m


def test_zero_queries_give_the_mean_of_the_live_value_rows():
    q, k, v = ar.inputs("flat", B, H, 5, 9, "fp32")
    m = np.zeros((5, 9), np.uint8)
    m[:, [2, 7]] = 1
    O, A = ar.attention(np.zeros_like(q), k, v, H, SCALE, m)
    live = [j for j in range(9) if j not in (2, 7)]
    want = v[:, live].astype(np.float64).mean(1, keepdims=True)
    assert np.abs(O - want).max() <= 1e-15
    assert np.abs(A - np.abs(v[:, live]).astype(np.float64).mean(1, keepdims=True)).max() <= 1e-15
    assert (np.abs(O) <= A + 1e-15).all()


def test_one_key_far_above_the_rest_gives_its_value_row():
    q, k, v = (x.copy() for x in ar.inputs("flat", B, H, 4, 9, "fp32"))
    q[:] = 1.0
    k[:] = 0.0
    k[:, 6] = 100.0                                   # score 800 against 0: the others weigh exp(-800) = 0 in float64
    O, _ = ar.attention(q, k, v, H, SCALE)
    assert np.array_equal(O, np.broadcast_to(v[:, 6:7].astype(np.float64), O.shape))


def test_a_masked_key_has_weight_exactly_zero():
    q, k, v = ar.inputs("peaked", B, H, 6, 10, "fp32")
    m = _mask_rows(6, 10)
    P, rel = ar.probabilities(q, k, H, SCALE, m)
    assert (P[:, :, m != 0] == 0).all() and (rel[:, :, m != 0] == 0).all()
    assert (P[:, :, m == 0] > 0).all()
    assert np.abs(P.sum(-1) - 1).max() <= 1e-15
    v2 = v.copy()
    v2[:, 1::2] = 1e30                                # rows 0, 2, 4 never see the odd keys
    assert np.array_equal(ar.attention(q, k, v2, H, SCALE, m)[0][:, ::2], ar.attention(q, k, v, H, SCALE, m)[0][:, ::2])


def test_keep_is_applied_after_the_denominator_with_the_factor_on_the_output():
    q, k, v = ar.inputs("flat", B, H, 6, 10, "fp32")
    keep = ar.synth.uniform01("attn/cpu/keep", B * H * 6 * 10).reshape(B, H, 6, 10) >= 0.3
    O, A = ar.attention(q, k, v, H, SCALE, keep=keep, p_drop=0.3)
    P0, _ = ar.probabilities(q, k, H, SCALE)
    vh = v.astype(np.float64).reshape(B, 10, H, 64)
    want = np.einsum("bhqk,bkhc->bqhc", P0 * keep / 0.7, vh).reshape(B, 6, H * 64)
    assert np.abs(O - want).max() <= 1e-15
    assert np.abs(A - np.einsum("bhqk,bkhc->bqhc", P0 * keep / 0.7, np.abs(vh)).reshape(B, 6, H * 64)).max() <= 1e-15


def test_a_fully_masked_row_is_nan_in_that_row_only():
    q, k, v = ar.inputs("flat", B, H, 8, 20, "bf16")
    m = ar.mask("fullrow", 8, 20)
    for dt in (np.float64, np.float32):
        O, A = ar.attention(q, k, v, H, SCALE, m, dtype=dt)
        nan = np.isnan(O)
        assert nan[:, ar.full_row(8)].all() and not np.delete(nan, ar.full_row(8), axis=1).any()
    e = ar.emulate(q, k, v, H, SCALE, "bf16", m)
    assert np.array_equal(np.isnan(e), nan)


def test_storage_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.3, 2.0 ** -130], np.float32)
    assert np.array_equal(ar.round_to(x, "bf16")[:4], np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7], np.float32))
    import torch
    big = ar.synth.normalish("attn/cpu/round", (4096,)) * 100
    assert np.array_equal(ar.round_to(big, "bf16"), torch.from_numpy(big).bfloat16().float().numpy())
    assert np.array_equal(ar.round_to(big, "fp16"), torch.from_numpy(big).half().float().numpy())


def _case(family, T, masked=False, drop=False):
    Tq, Tk = SHAPES[family]
    q, k, v = ar.inputs(family, B, H, Tq, Tk, T)
    m = ar.mask("random", Tq, Tk) if masked else None
    keep = (ar.synth.uniform01(f"attn/cpu/keep/{family}", B * H * Tq * Tk).reshape(B, H, Tq, Tk) >= 0.5) if drop else None
    pd = 0.5 if drop else 0.0
    return (q, k, v, H, SCALE, T), dict(mask=m, keep=keep, p_drop=pd)


@pytest.mark.parametrize("T", ["bf16", "fp16"])
@pytest.mark.parametrize("variant", ["plain", "masked", "dropout"])
@pytest.mark.parametrize("family", ar.FAMILIES)
def test_the_emulated_16_bit_arithmetic_stays_inside_the_bound(family, variant, T):
    args, kw = _case(family, T, variant == "masked", variant == "dropout")
    ref = ar.reference(*args, **kw)
    r = ar.ratio(ar.emulate(*args, **kw), ref)
    print(f"{family} {variant} {T}: emulator at {r:.3f} of the bound, yardstick {ref['yardstick'] / ar.U:.2f} u")
    assert r <= 1.0


# which family catches which mutant (the family's smallest shape, both storage types).  `denominator` needs |O| = A, i.e. one
# key holding the row (peaked) or a one-hot V (probe); the mask and dropout mutants need the masked / dropout variant.
CAUGHT_BY = {"drop_last_key": ("flat", "plain"), "drop_last_fragment": ("flat", "plain"), "swap_v_rows": ("probe", "plain"),
             "denominator": ("probe", "plain"), "mask_next_row": ("flat", "masked"),
             "keep_before_denominator": ("flat", "dropout")}


@pytest.mark.parametrize("T", ["bf16", "fp16"])
@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_every_mutant_leaves_the_bound_on_its_family(mutant, T):
    family, variant = CAUGHT_BY[mutant]
    args, kw = _case(family, T, variant == "masked", variant == "dropout")
    ref = ar.reference(*args, **kw)
    assert ar.ratio(ar.emulate(*args, **kw), ref) <= 1.0
    r = ar.ratio(ar.emulate(*args, mutant=mutant, **kw), ref)
    print(f"{mutant} on {family} {variant} {T}: {r:.2f} of the bound")
    assert r > 1.0


@pytest.mark.parametrize("T", ["bf16", "fp16"])
def test_which_families_catch_which_mutant(T):
    """The whole table, printed: a record of how far each mutant leaves the bound on each family (no family is blind to all)."""
    seen = {f: 0 for f in ar.FAMILIES}
    for mutant in ar.MUTANTS:
        variant = {"mask_next_row": "masked", "keep_before_denominator": "dropout"}.get(mutant, "plain")
        row = []
        for family in ar.FAMILIES:
            args, kw = _case(family, T, variant == "masked", variant == "dropout")
            r = ar.ratio(ar.emulate(*args, mutant=mutant, **kw), ar.reference(*args, **kw))
            seen[family] += r > 1.0
            row.append(f"{family} {r:9.2f}")
        print(f"{T} {mutant:24s}", " | ".join(row))
    assert all(n > 0 for n in seen.values()), seen


def test_the_fp32_bound_has_no_16_bit_term_and_the_fp16_bound_counts_subnormals():
    A = np.full((1, 2, 64), 0.5)
    assert np.array_equal(ar.bound(A, 0.0, "fp32", 8), 16 * ar.U * A)
    assert np.array_equal(ar.bound(A, 10 * ar.U, "fp32", 8), 40 * ar.U * A)
    assert np.array_equal(ar.bound(A, 0.0, "bf16", 8), (16 * ar.U + 2.0 ** -7) * A)
    n = np.zeros_like(A)
    n[0, 1] = 3
    b = ar.bound(A, 0.0, "fp16", 8, n, 2.0)
    assert np.array_equal(b[0, 0], (16 * ar.U + 2.0 ** -10) * A[0, 0] + 2.0 ** -25)
    assert np.array_equal(b[0, 1], (16 * ar.U + 2.0 ** -10) * A[0, 1] + 6 * 2.0 ** -24 + 2.0 ** -25)


def test_wave_rule_by_hand():
    """attn_waves restated: 256 (batch, head) pairs give one workgroup each at Tq = 16 nw; the small grids of the GPU tests all
    land on 4 waves; the smallest grids that reach 7, 13 and 16."""
    assert [ar.attn_waves(t, 8, 32) for t in (112, 208, 256)] == [7, 13, 16]
    assert all(ar.attn_waves(t, 3, 2) == 4 for t in (1, 63, 64, 65, 250, 514))
    assert [ar.smallest_grid(nw) for nw in (7, 13, 16)] == [(112, 3, 43), (208, 2, 97), (256, 2, 97)]
    assert ar.region("bf16", 112, 208, 3, 2) == ("w13", 7) and ar.region("fp16", 113, 208, 3, 2) == ("w13", 13)
    assert ar.region("bf16", 1, 209, 3, 2) == ("w17", 9) and ar.region("bf16", 1, 272, 3, 2) == ("w17", 9)
    assert ar.region("bf16", 1, 273, 3, 2) == ("t16", 4) and ar.region("fp32", 1, 1, 3, 2) == ("t32", 4)


def test_the_yardstick_of_a_short_case_is_taken_over_64_rows_of_its_family():
    q, k, v = ar.inputs("peaked", B, H, 1, 65, "fp32")
    qy = ar.yard_queries("peaked", B, H, 1, 65, "fp32")
    assert qy.shape == (B, 64, H * 64) and np.array_equal(qy[:, :1], q) and ar.yard_queries("peaked", B, H, 64, 65, "fp32") is None
    own, wide = ar.reference(q, k, v, H, SCALE, "fp32"), ar.reference(q, k, v, H, SCALE, "fp32", q_yard=qy)
    assert wide["yardstick"] >= own["yardstick"] and np.array_equal(own["O"], wide["O"]) and np.array_equal(own["A"], wide["A"])
    assert np.array_equal(wide["bound"], max(16 * ar.U, 4 * wide["yardstick"]) * wide["A"])
