"""The launches `Wav2Vec2Model.encode_features` and `DenoisingNetwork_MSMD.trunk` make, path by path, as a recorded table.

Both functions write a transformer layer once and leave the form of every LayerNorm (a kernel, folded into the GEMMs around
it, split storage) to msmd_amd.blocks.  The timed forward step and the sampler loop are hipGraph replays of these launches,
so "same calls, same order, same scalar arguments, same optional operands" is "same bits, same speed" -- and that is all
this test asserts; it says nothing about what a kernel computes.

tests/golden/launch_sequences.txt was recorded from the commit BEFORE the layer loops were merged (five hand-written
encoder loops, three decoder loops): that commit's Python, checked out beside this file, importable first and pointed at the
same built library (MSMD_LIB), ran this module's own recorder

    PYTHONPATH=<checkout of the earlier commit> MSMD_LIB=<csrc/libmsmd_hip.so> python tests/test_launch_sequence_gpu.py --record FILE

It is not an output of the code under test.

The recorder stands in for the loaded library (msmd_amd._lib._lib) during one call: every C-ABI entry is logged with its
arguments and forwarded.  Pointer arguments -- the stream included -- are logged as set (`*`) or null (`-`), since addresses
do not compare between runs; integers and floats as they are.  Only launches made while one of the two methods is on the
stack count.  Shapes: 3 encoder + 3 decoder layers (a first, a middle and a last layer), 2 clips of 64 000 samples."""
import os
import sys

import numpy as np
import pytest
import torch

os.environ.setdefault("MSMD_SYNTHETIC_WEIGHTS", "1")

from msmd_amd import _lib, ops, synth  # noqa: E402
from msmd_amd.config import default_args  # noqa: E402

from helpers import denoiser_inputs, load_fixture, recording  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequences.txt")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _recording():
    from msmd_amd.model import DenoisingNetwork_MSMD
    from msmd_amd.utils.wav2vec2 import Wav2Vec2Model
    return recording([(Wav2Vec2Model, "encode_features"), (DenoisingNetwork_MSMD, "trunk")])


_MODELS = {}


def get_model(audio_model, dtype, **kw):
    from msmd_amd.model import get_diffusion_model
    key = (audio_model, dtype, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS.clear()  # keep one model resident
        args = default_args(audio_model=audio_model, compute_dtype=dtype, encoder_layers=3, n_layers=3, **kw)
        _MODELS[key] = (get_diffusion_model(args, DEV).eval(), args)
    return _MODELS[key]


def run_encoder(model, args):
    model.extract_audio_768_feature(dev(synth.audio_clips(2, 64000, tag="ls_audio")))


def run_trunk(model, args):
    x = denoiser_inputs(2, args, tag="ls")
    person = torch.cat([dev(x["shape"])[:, None], dev(x["style"])[:, None]], dim=-1)
    model.denoising_net(dev(x["motion"]), dev(x["audio_feat"]), person, dev(x["style"])[:, None], dev(x["prev_motion"]),
                        dev(x["prev_audio"]), [7, 250], dev(x["indicator"]))


def run_sample(model, args):
    """Two eager denoising steps (injected noise) with the hoisted kv_list / cross_list; the first one is compared."""
    from msmd_amd.model import DiffusionSchedule
    x = denoiser_inputs(2, args, tag="ls")
    old = model.diffusion_sched
    model.diffusion_sched = DiffusionSchedule(2, "cosine").to(DEV)
    try:
        model.sample(dev(x["audio_feat"]), dev(x["shape"]), dev(x["style"]), dev(x["prev_motion"]), dev(x["prev_audio"]),
                     motion_at_T=dev(synth.normalish("ls/xT", (2, 100, 67))), indicator=dev(x["indicator"]),
                     noise={2: dev(synth.normalish("ls/z2", (2, 100, 67)))})
    finally:
        model.diffusion_sched = old


HL = dict(n_motions=100)
SINGLE = dict(diag_single_pass=True)
# name: (audio model, compute dtype, model arguments, ops.FOLD_LN, switches set on the denoiser, what runs)
CASES = {
    "encoder wav2vec2 bf16 fold": ("wav2vec2", "bf16", {}, True, {}, run_encoder),
    "encoder wav2vec2 bf16 plain": ("wav2vec2", "bf16", {}, False, {}, run_encoder),
    "trunk general bf16 fold": ("wav2vec2", "bf16", {}, True, {}, run_trunk),
    "trunk general bf16 plain": ("wav2vec2", "bf16", {}, False, {}, run_trunk),
    "trunk diagonal single pass bf16 fused person query": ("wav2vec2", "bf16", {}, True,
                                                           dict(SINGLE, fused_person_query=True), run_trunk),
    "trunk diagonal single pass bf16 two-launch person query": ("wav2vec2", "bf16", {}, True,
                                                                dict(SINGLE, fused_person_query=False), run_trunk),
    "trunk diagonal single pass bf16 dead person chain kept": ("wav2vec2", "bf16", {}, True,
                                                               dict(SINGLE, skip_dead_person_chain=False), run_trunk),
    "trunk sampler step bf16": ("wav2vec2", "bf16", {}, True, {}, run_sample),
    "trunk mask width 2 bf16": ("wav2vec2", "bf16", dict(align_mask_width=2), True, {}, run_trunk),
    "encoder wav2vec2 fp32": ("wav2vec2", "fp32", {}, True, {}, run_encoder),
    "trunk general fp32": ("wav2vec2", "fp32", {}, True, {}, run_trunk),
    "trunk diagonal single pass fp32": ("wav2vec2", "fp32", {}, True, SINGLE, run_trunk),
    "encoder wav2vec2 f16x2": ("wav2vec2", "f16x2", {}, True, {}, run_encoder),
    "trunk general f16x2": ("wav2vec2", "f16x2", {}, True, {}, run_trunk),
    "trunk sampler step f16x2": ("wav2vec2", "f16x2", {}, True, {}, run_sample),
    "encoder hubert_large bf16 fold": ("hubert_large", "bf16", HL, True, {}, run_encoder),
    "encoder hubert_large bf16 plain": ("hubert_large", "bf16", HL, False, {}, run_encoder),
    "encoder hubert_large f16x2": ("hubert_large", "f16x2", HL, True, {}, run_encoder),   # the pre-LN loop, split weights
}


def record(name):
    """The launch lines of one case: the first recorded invocation of the wrapped method the case is about."""
    am, dtype, kw, fold, switches, run = CASES[name]
    model, args = get_model(am, dtype, **kw)
    net = model.denoising_net
    run(model, args)                # packs the weights (their launches are none of the layers')
    torch.cuda.synchronize()
    for k, v in switches.items():
        setattr(net, k, v)
    old_fold, ops.FOLD_LN = ops.FOLD_LN, fold
    try:
        with _recording() as rec:
            run(model, args)
    finally:
        ops.FOLD_LN = old_fold
        for k in switches:
            net.__dict__.pop(k, None)
    torch.cuda.synchronize()
    assert rec.invocations, name
    return rec.invocations[0]


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_is_the_recorded_one(name):
    want = load_fixture(FIXTURE)[name]
    got = record(name)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: launch {i} differs\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{name}: {len(got)} launches, recorded {len(want)}"
    assert len(want) >= 3 * 5    # a layer is at least QKV, attention, out-projection, FFN 1, FFN 2: an empty recording compares nothing


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_launch_sequence_gpu.py --record FILE")
    print(f"recording the launches of {os.path.dirname(os.path.abspath(_lib.__file__))}", file=sys.stderr)
    with open(sys.argv[2], "w") as out:
        out.write("# launches of encode_features / trunk per path: see tests/test_launch_sequence_gpu.py\n")
        for case in CASES:
            out.write(f"[{case}]\n" + "\n".join(record(case)) + "\n")
