"""msmd_denoiser_prepare against the entries it stands in for, bit for bit.

One launch writes the packed denoiser input, the padded person rows, the style rows in the compute dtype, the gathered step
embedding and the previous window's rows of the audio memory.  The reference for every buffer is what the forward ran before:
`denoiser_pack_input` on torch-gathered coefficients, `pad_cols` on the concatenated person rows, `cast`, torch indexing and
`copy_`.  Shapes are the smallest with more than one 8-element unit per row and a person width (124) that is no multiple of
64 before padding."""
import numpy as np
import pytest
import torch

from msmd_amd import synth
from msmd_amd.config import default_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
L, LP, DM, KP, D, LPA, LA = 3, 2, 5, 64, 64, 2, 3
N_SHAPE, N_STYLE, KP_PERSON, STEPS = 100, 24, 128, 11      # 124 person columns, padded to 128; steps 0 .. 10
SENTINEL = 7.0


def ops():
    from msmd_amd import ops as o
    return o


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ts_lists(N):
    """0, 1 and the last step; for N = 3 also a call in which one step repeats."""
    last = STEPS - 1
    return [[0], [1], [last]] if N == 1 else [[0, 1, last], [last, 1, 1]]


@pytest.mark.parametrize("per_clip_prev", [False, True])
@pytest.mark.parametrize("with_eps", [False, True])
@pytest.mark.parametrize("with_ind", [False, True])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_prepare_writes_the_bits_of_the_entries_it_replaces(dtype, N, with_ind, with_eps, per_clip_prev):
    o = ops()
    tag = f"prep/{N}"
    motion = dev(synth.normalish(f"{tag}/motion", (N, L, DM)))
    eps = dev(synth.normalish(f"{tag}/eps", (N, L, DM))) if with_eps else None
    ind = dev(synth.normalish(f"{tag}/ind", (N, L))) if with_ind else None
    shape = dev(synth.normalish(f"{tag}/shape", (N, 1, N_SHAPE)))
    style = dev(synth.normalish(f"{tag}/style", (N, 1, N_STYLE)))
    rows = N if per_clip_prev else 1
    prev_m = dev(synth.normalish(f"{tag}/prev_m", (rows, LP, DM))).expand(N, -1, -1)      # batch stride 0 when rows == 1
    prev_a = dev(synth.normalish(f"{tag}/prev_a", (rows, LPA, D))).expand(N, -1, -1)
    t0 = dev(np.linspace(1.0, 0.05, STEPS).astype(np.float32))
    t1 = dev(np.sqrt(1.0 - np.linspace(1.0, 0.05, STEPS) ** 2).astype(np.float32))
    table = dev(synth.normalish("prep/table", (STEPS, D))).to(dtype)
    for steps in ts_lists(N):
        ts = torch.tensor(steps, device=DEV, dtype=torch.long)
        # the reference: the existing entries and torch
        want_feats = torch.full((N, 1 + LP + L, KP), SENTINEL, device=DEV, dtype=dtype)
        o.denoiser_pack_input(motion, prev_m.contiguous(), ind, want_feats, eps,
                              t0[ts] if with_eps else None, t1[ts] if with_eps else None)
        want_pf = o.pad_cols(torch.cat([shape, style], dim=-1).reshape(N, -1).contiguous(), KP_PERSON, dtype)
        want_style = o.cast(style.reshape(N, -1).contiguous(), dtype)
        want_emb = table[ts]
        want_mem = torch.full((N, LPA + LA, D), SENTINEL, device=DEV, dtype=dtype)
        want_mem[:, :LPA].copy_(prev_a)
        # the one launch
        feats = torch.full((N, 1 + LP + L, KP), SENTINEL, device=DEV, dtype=dtype)
        pf = torch.full((N, KP_PERSON), SENTINEL, device=DEV, dtype=dtype)
        style_cd = torch.full((N, N_STYLE), SENTINEL, device=DEV, dtype=dtype)
        emb = torch.full((N, D), SENTINEL, device=DEV, dtype=dtype)
        mem = torch.full((N, LPA + LA, D), SENTINEL, device=DEV, dtype=dtype)       # rows LPA.. must keep the sentinel
        o.denoiser_prepare(motion, prev_m, ind, feats, ts, table, emb, shape.reshape(N, -1), style.reshape(N, -1), pf, prev_a,
                           mem, style=style.reshape(N, -1), style_out=style_cd, eps=eps, t0=t0 if with_eps else None,
                           t1=t1 if with_eps else None)
        torch.cuda.synchronize()
        for name, got, want in (("feats", feats, want_feats), ("pf", pf, want_pf), ("style", style_cd, want_style),
                                ("emb", emb, want_emb), ("mem", mem, want_mem)):
            assert got.shape == want.shape and torch.equal(got, want), (name, steps)


def test_prepare_takes_one_person_block_and_no_style():
    """The direct denoiser call hands the person rows over already joined (person_b null), and a style in the compute dtype
    needs no cast (style null): the other outputs are written as before."""
    o = ops()
    N, dtype = 3, torch.bfloat16
    motion = dev(synth.normalish("prep1/motion", (N, L, DM)))
    person = dev(synth.normalish("prep1/person", (N, N_SHAPE + N_STYLE)))
    prev_m = dev(synth.normalish("prep1/prev_m", (N, LP, DM)))
    prev_a = dev(synth.normalish("prep1/prev_a", (N, LPA, D)))
    table = dev(synth.normalish("prep/table", (STEPS, D))).to(dtype)
    ts = torch.tensor([2, 0, STEPS - 1], device=DEV, dtype=torch.long)
    want_feats = torch.empty(N, 1 + LP + L, KP, device=DEV, dtype=dtype)
    o.denoiser_pack_input(motion, prev_m, None, want_feats)
    feats, emb = torch.empty_like(want_feats), torch.empty(N, D, device=DEV, dtype=dtype)
    pf = torch.empty(N, KP_PERSON, device=DEV, dtype=dtype)
    mem = torch.zeros(N, LPA + LA, D, device=DEV, dtype=dtype)
    o.denoiser_prepare(motion, prev_m, None, feats, ts, table, emb, person, None, pf, prev_a, mem)
    torch.cuda.synchronize()
    assert torch.equal(feats, want_feats) and torch.equal(emb, table[ts])
    assert torch.equal(pf, o.pad_cols(person, KP_PERSON, dtype))
    assert torch.equal(mem[:, :LPA], prev_a.to(dtype)) and not mem[:, LPA:].any()


def test_prepare_refuses_fp32_and_unknown_storage_types():
    """16-bit storage only: MSMD_F32 (0), MSMD_F16X2 (3) and a code that names no type return non-zero and write nothing."""
    from msmd_amd import _lib
    lib = _lib.load()
    N = 1
    f32 = lambda *s: torch.ones(s, device=DEV, dtype=torch.float32)
    outs = [torch.full(s, SENTINEL, device=DEV, dtype=torch.float32)
            for s in ((N, 1 + LP + L, KP), (N, KP_PERSON), (N, D), (N, LPA + LA, D))]
    feats, pf, emb, mem = outs
    motion, prev_m, person, prev_a, table = f32(N, L, DM), f32(N, LP, DM), f32(N, 124), f32(N, LPA, D), f32(STEPS, D)
    ts = torch.zeros(N, device=DEV, dtype=torch.long)
    P = lambda t: t.data_ptr()
    for code in (0, 3, 7):
        rc = lib.msmd_denoiser_prepare(P(motion), None, None, None, P(ts), STEPS, P(prev_m), LP * DM, None, P(feats), N, L, LP,
                                       DM, KP, P(person), 124, None, 0, P(pf), KP_PERSON, None, 0, None, P(table), P(emb), D,
                                       P(prev_a), LPA * D, LPA, P(mem), (LPA + LA) * D, code,
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc != 0, code
        assert all(bool((t == SENTINEL).all()) for t in outs), code


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_step_embedding_table_rows_are_the_gathered_gemms(dtype):
    """Rows 0, 1 and last of the per-pack table equal the two diff_step_map GEMMs run on those three rows alone: a GEMM row
    does not depend on the rows around it, so the table row is what person_token computes for that step."""
    from msmd_amd.model import DenoisingNetwork_MSMD
    o = ops()
    args = default_args(compute_dtype="bf16" if dtype == torch.bfloat16 else "fp16", n_layers=1)
    torch.manual_seed(0)
    net = DenoisingNetwork_MSMD(args, DEV, motion_feat_dim=67, use_head_alpha=False).eval()
    P = net.pack(dtype)
    assert P.emb_table is None                      # lazily, by the first eval forward
    table = net.step_embeddings(dtype)
    assert table is net.step_embeddings(dtype) and table is P.emb_table
    assert tuple(table.shape) == (args.n_diff_steps + 1, args.feature_dim) and table.dtype == dtype
    idx = torch.tensor([0, 1, args.n_diff_steps], device=DEV)
    want = o.gemm(o.gemm(P.te_cd[idx], *P.ds0, act=o.ACT_GELU), *P.ds2)
    torch.cuda.synchronize()
    assert torch.equal(table[idx], want)
    net.float()                                     # any _apply drops the pack, and the table with it
    assert net._packed is None and net.pack(dtype).emb_table is None
