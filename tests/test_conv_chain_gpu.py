"""ops.conv_chain (msmd_conv_chain): conv layers chained in one launch store the bits of the per-layer ops.conv1d_cl launches.

Shapes: 3 clips of 1 031 rows, so the layers have 515 / 257 / 128 / 63 rows per clip -- 1 545 / 771 / 384 / 189 rows: tiles that
straddle clip boundaries, ragged last row blocks, a last layer of one row block -- at 256 channels (one column tile) and 512
(two).  The grid is cut to 1 workgroup (the whole ticket list in order), 2 and 5 (the persistent loop wraps, consumers run right
behind their producers and wait) and left alone (one workgroup per ticket).  Both hand-over forms and both ticket sizes.  Every
case runs twice into the same buffers on different inputs: the second call finds the first call's intermediate rows in the
caches and must not read them, and finds the first call's counters in the state block, which the launch zeroes itself.  No
test tries to make a wait expire."""
import ctypes
from unittest import mock

import pytest
import torch

from msmd_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T0 = 3, 1031
KERNELS, STRIDES = (3, 3, 3, 3), (2, 2, 2, 2)
FORMS = [0, ops.CONV_CHAIN_RELEASE, ops.CONV_CHAIN_ROW_BLOCK_TICKETS, ops.CONV_CHAIN_RELEASE | ops.CONV_CHAIN_ROW_BLOCK_TICKETS]

_CASES = {}


def case(C, dtype):
    """Weights, two inputs and the per-layer reference outputs of each, computed once per (C, dtype) and never written again."""
    key = (C, dtype)
    if key not in _CASES:
        g = torch.Generator(device="cpu").manual_seed(C + (dtype == torch.float16))
        rnd = lambda *s: torch.randn(*s, generator=g)
        ws = [(rnd(C, 3 * C) / (3 * C) ** 0.5).to(DEV, dtype) for _ in KERNELS]
        bs = [(0.1 * rnd(C)).to(DEV) for _ in KERNELS]
        xs = [rnd(B, T0, C).to(DEV, dtype) for _ in range(2)]
        refs = []
        for x in xs:
            outs = []
            for w, b, k, s in zip(ws, bs, KERNELS, STRIDES):
                x = ops.conv1d_cl(x, w, b, kernel=k, stride=s, act=ops.ACT_GELU)
                outs.append(x)
            refs.append(outs)
        torch.cuda.synchronize()
        _CASES[key] = (ws, bs, xs, refs)
    return _CASES[key]


def workspace_for(C, n):
    nbytes = _lib.load().msmd_conv_chain_workspace(B, T0, C, C, n, ops._int_array(KERNELS[:n]), ops._int_array(STRIDES[:n]))
    assert nbytes > 0 and nbytes % 16 == 0
    return torch.full((nbytes,), 0xA5, device=DEV, dtype=torch.uint8)      # never zeroed by the caller


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [256, 512])
def test_chain_stores_the_per_layer_bits(C, dtype, n):
    ws, bs, xs, refs = case(C, dtype)
    outs = [torch.empty_like(r) for r in refs[0][:n]]
    workspace = workspace_for(C, n)
    for max_wg in (1, 2, 5, 0):
        for form in FORMS:
            for x, ref in zip(xs, refs):
                got = ops.conv_chain(x, ws[:n], bs[:n], kernels=KERNELS[:n], strides=STRIDES[:n], act=ops.ACT_GELU, flags=form,
                                     max_workgroups=max_wg, outs=outs, workspace=workspace)
                assert got is outs
                assert ops.conv_chain_status(workspace) == 0, (max_wg, form)
                for l in range(n):
                    assert torch.equal(outs[l], ref[l]), (max_wg, form, l)


def test_no_bias_no_activation():
    ws, _, xs, _ = case(512, torch.bfloat16)
    x = xs[0]
    got = ops.conv_chain(x, ws[:2], [None, None], kernels=KERNELS[:2], strides=STRIDES[:2])
    for w, o in zip(ws, got):
        x = ops.conv1d_cl(x, w, None, kernel=3, stride=2)
        assert torch.equal(o, x)


def two_clips_of_four_seconds():
    """The shape of a 2-clip forward (12 815 rows into the stack, a 416-byte state block, 190 tiles: every workgroup's first
    ticket, consumers included, is claimed at once); weights of case(512, bf16)."""
    ws, bs, _, _ = case(512, torch.bfloat16)
    g = torch.Generator(device="cpu").manual_seed(7)
    xs = [torch.randn(2, 12815, 512, generator=g).to(DEV, torch.bfloat16) for _ in range(2)]
    refs = []
    for x in xs:
        outs = []
        for w, b, k, s in zip(ws, bs, KERNELS, STRIDES):
            x = ops.conv1d_cl(x, w, b, kernel=k, stride=s, act=ops.ACT_GELU)
            outs.append(x)
        refs.append(outs)
    return ws, bs, xs, refs


@pytest.mark.parametrize("shape", ["small", "two_clips"])
def test_chain_replays_in_a_graph(shape):
    ws, bs, xs, refs = case(512, torch.bfloat16) if shape == "small" else two_clips_of_four_seconds()
    x = xs[0].clone()
    outs = [torch.empty_like(r) for r in refs[0]]
    workspace = torch.full((4096,), 0xA5, device=DEV, dtype=torch.uint8)
    run = lambda: ops.conv_chain(x, ws, bs, kernels=KERNELS, strides=STRIDES, act=ops.ACT_GELU, outs=outs, workspace=workspace)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture_guard(), torch.cuda.graph(graph):
        run()
    for n, i in enumerate((1, 0, 1)):
        x.copy_(xs[i])
        if n == 1:
            workspace.fill_(0x5A)      # the replayed graph, not the caller, zeroes the state: from this, and from the last replay's counters
        graph.replay()
        assert ops.conv_chain_status(workspace) == 0
        for o, r in zip(outs, refs[i]):
            assert torch.equal(o, r), i


def test_declined_shapes_launch_nothing():
    C, dtype = 320, torch.bfloat16
    x = torch.randn(B, T0, C, device=DEV).to(dtype)
    ws = [torch.randn(C, 3 * C, device=DEV).to(dtype) for _ in range(2)]
    bs = [torch.zeros(C, device=DEV) for _ in range(2)]
    assert ops.conv_chain(x, ws, bs, kernels=(3, 3), strides=(2, 2)) is None
    outs = [torch.full((B, T, C), 7.0, device=DEV, dtype=dtype) for T in (515, 257)]
    workspace = torch.full((4096,), 0xA5, device=DEV, dtype=torch.uint8)
    ptrs = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])
    r = _lib.load().msmd_conv_chain(x.data_ptr(), B, T0, C, C, 2, ptrs(ws), ptrs(bs), ptrs(outs), ops._int_array((3, 3)),
                                    ops._int_array((2, 2)), ops.ACT_GELU, ops.BF16, workspace.data_ptr(), workspace.numel(), 0, 0,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert r == 1
    assert all(bool((o == 7.0).all()) for o in outs) and bool((workspace == 0xA5).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_feature_extractor_with_and_without_the_chain(dtype):
    from msmd_amd import synth
    from msmd_amd.config import synthetic_args
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.utils.model_common import pad_audio_plan
    args = synthetic_args(compute_dtype="bf16", encoder_layers=1, n_layers=1)
    enc = get_diffusion_model(args, DEV).eval().audio_encoder
    assert enc.conv_chain is True
    real = ops.conv_chain
    for nb, length in ((1, 64000), (2, 51234)):
        audio = torch.from_numpy(synth.audio_clips(nb, length)).to(DEV)
        r, rep = pad_audio_plan(length)
        taken = []
        with mock.patch.object(ops, "conv_chain", side_effect=lambda *a, **k: taken.append(real(*a, **k)) or taken[-1]):
            on = enc.feature_extractor_cl(audio, dtype, r, rep)
            assert len(taken) == 1 and taken[0] is not None, "the library takes the model's conv1-4"
            kept = enc.feature_extractor_cl(audio, dtype, r, rep, chain=False)
            enc.conv_chain = False
            try:
                off = enc.feature_extractor_cl(audio, dtype, r, rep)
            finally:
                enc.conv_chain = True
            assert len(taken) == 1
        assert on.shape == off.shape and torch.equal(on, off) and torch.equal(kept, off), (nb, length)
