"""What one training iteration (`Trainer._fwd_bwd`: two windows, losses, one backward) launches, as a recorded table.

The step is about 10^4 launches replayed as a hipGraph, so "same calls, same order, same scalar arguments" is "same bits,
same speed" -- and that is all this test asserts.  train_graph.py writes the transformer layer, the loss window and the
window body once; autograd.py picks the destination of a weight gradient in one place.  That none of it changed what is
launched is checked here against a recording of the commit BEFORE that rewrite (four hand-written layer copies, two window
bodies, six wgrad branches), not against the code under test.

tests/golden/train_launch_sequences.txt.gz (7 463 lines of text, gzip-compressed: read it with `zcat`; `--record FILE` writes
the text, `gzip -n` makes the fixture of it) was recorded from that earlier commit's Python, checked out beside this file,
importable first and pointed at the same built library (MSMD_LIB), running this module's own recorder

    PYTHONPATH=<checkout of the parent> MSMD_LIB=<csrc/libmsmd_hip.so> python tests/test_train_launch_sequence_gpu.py --record FILE

twice, with identical files.  It is never regenerated from the code under test.

Two kinds of line, in the order they happen (helpers.Recorder):
  * every C-ABI call, as in tests/test_launch_sequence_gpu.py: pointers as `*` / `-`, integers and floats as they are (the
    dropout `site` numbers are integer arguments, so mask placement is pinned);
  * every aten op a TorchDispatchMode sees -- `aten <overload> <output shapes> <dtypes>` -- which pins the torch-side glue
    that also becomes graph nodes (cat, where, elementwise ops, autograd's accumulations).  Views and pure allocation /
    metadata ops are skipped; `_local_scalar_dense` is logged, since a host sync must not appear.
The backward runs with autograd's multithreading off, so its ops are on the recording thread (the Trainer does the same
in segmented capture).

Each case builds a fresh model and Trainer after ag.CACHE.clear() (LayerDrop's cached zero dropped too), runs one step to
fill the caches and records the second one with the same injected draws.  Shapes: 2 encoder + 2 decoder layers (a first
layer, a last layer and a "next layer" for the prefetch / alias lookups), B = 2, 64 000-sample clips."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

os.environ.setdefault("MSMD_SYNTHETIC_WEIGHTS", "1")

from msmd_amd import _lib, synth  # noqa: E402
from msmd_amd import autograd as ag  # noqa: E402
from msmd_amd import train_graph as tg  # noqa: E402
from msmd_amd.config import default_args  # noqa: E402

from helpers import load_fixture, recording  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_launch_sequences.txt.gz")
B = 2


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def draws_of(cross, cfg):
    """The injected draws of test_trainer_step_adam_and_overfit: window 0 truncated, cross-style on window 1, CFG flags."""
    return dict(cross=cross, end_idx=[torch.tensor([60, 100], device=DEV), None], t=[[5, 400], [250, 20]],
                eps=[dev(synth.normalish(f"tr/eps{i}", (B, 100, 67))) for i in range(2)],
                style_eps=[dev(synth.normalish(f"tr/se{i}", (B, 256))) for i in range(2)], cfg_flag=cfg)


def vertex_setup():
    """FLAME module, coefficient statistics and arguments of test_trainer_vertex_space_branch_steps_through_flame."""
    from msmd_amd.utils.flame import FLAME, FLAMEConfig
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = synth.flame_asset()
    stats = {"exp_mean": np.zeros(50, np.float32), "exp_std": np.full(50, 0.3, np.float32),
             "pose_mean": np.zeros(6, np.float32), "pose_std": np.full(6, 0.1, np.float32),
             "shape_mean": np.zeros(100, np.float32), "shape_std": np.ones(100, np.float32)}
    return dict(flame=FLAME(cfg).to(DEV), coef_stats=stats)


VERTEX = dict(lr=2e-4, use_vertex_space=True, dataset_type="flame_mead_ravdess", l_vert=2e5, l_vel=1e6, l_smooth=1e5)
# name: dict(args: model arguments, train: model.train(), layerdrop: set on the encoder's config, trainer: Trainer keywords,
#            direct_grad: set on the Trainer after construction, vertex: the vertex-space branch through FLAME)
CASES = {
    "bf16 eval eager batched": dict(),
    "bf16 train eager batched layerdrop 0.5": dict(train=True, layerdrop=0.5),
    "bf16 train hipgraph warm-up": dict(train=True, trainer=dict(use_graph=True)),
    "fp32 eval eager in turn": dict(args=dict(compute_dtype="fp32"), trainer=dict(batch_windows=False)),
    "bf16 eval eager gradients through autograd": dict(direct_grad=False),
    "hubert_large bf16 train eager": dict(args=dict(audio_model="hubert_large", n_motions=100), train=True),
    "bf16 eval eager vertex space": dict(args=VERTEX, vertex=True),
}


def record(name):
    """The lines of one case: the first `_fwd_bwd` of the second step (in hipGraph mode: the warm-up pass of its capture)."""
    from msmd_amd.model import get_diffusion_model
    from msmd_amd.style_encoder import get_style_encoder
    from msmd_amd.training_script import Trainer, synthetic_batch
    case = CASES[name]
    kw = dict(dict(compute_dtype="bf16", encoder_layers=2, n_layers=2, lr=1e-3, warm_iter=0, gradient_accumulation_steps=1),
              **case.get("args", {}))
    args = default_args(**kw)
    ag.CACHE.clear()
    tg._ZERO.clear()        # per-process constants made on first use: a case must not depend on what ran before it
    torch.manual_seed(0)
    model = get_diffusion_model(args, DEV)
    se = get_style_encoder(args, "vae2").to(DEV)
    for m in (model, se):
        m.train() if case.get("train") else m.eval()
    if "layerdrop" in case:
        model.audio_encoder.config.layerdrop = case["layerdrop"]
    tkw = dict(case.get("trainer", {}), **(vertex_setup() if case.get("vertex") else {}))
    tr = Trainer(args, model, se, **tkw)
    if "direct_grad" in case:
        tr.direct_grad = case["direct_grad"]
    batch = synthetic_batch(B, 0, DEV)
    if case.get("vertex"):
        draws = draws_of([False, False], [None, None])
    else:
        draws = draws_of([False, True], [dev(np.array([0.1, 0.7], np.float32)), dev(np.array([0.95, 0.3], np.float32))])
    try:
        tr.step(batch, it=1, draws=draws)       # fills the weight caches (their launches are none of the step's)
        torch.cuda.synchronize()
        tr._graphs.clear()                      # hipGraph mode: the recorded step captures again, warm-up pass first
        with recording([(Trainer, "_fwd_bwd")], aten=True) as rec:
            tr.step(batch, it=2, draws=draws)
        torch.cuda.synchronize()
    finally:
        ag.TrainNoise.active = ag.TrainNoise.graph_safe = False
        ag.TrainNoise.spec_masks = None
        ag.DIRECT_GRAD = False
    assert rec.invocations, name
    return rec.invocations[0]


@pytest.mark.parametrize("name", list(CASES))
def test_training_step_launch_sequence_is_the_recorded_one(name):
    want = load_fixture(FIXTURE)[name]
    got = record(name)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: line {i} differs\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{name}: {len(got)} lines, recorded {len(want)}"
    assert len(want) >= 100     # an empty recording compares nothing


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_train_launch_sequence_gpu.py --record FILE")
    print(f"recording the launches of {os.path.dirname(os.path.abspath(_lib.__file__))}", file=sys.stderr)
    with open(sys.argv[2], "w") as out:
        out.write("# launches and aten ops of Trainer._fwd_bwd per case: see tests/test_train_launch_sequence_gpu.py\n")
        for case in CASES:
            out.write(f"[{case}]\n" + "\n".join(record(case)) + "\n")
