"""Host side of few-step guided / separated sampling: the keyframe helper against numpy assignment, the solver arguments of the
public entry points, and the split of a clip's keyframes over its windows."""
import inspect

import numpy as np
import pytest
import torch

from msmd_amd import sampler
from msmd_amd.inference import infer_coeffs, infer_coeffs_batch, window_keyframes, window_plan

L, DM = 37, 67


def numpy_assign(B, idx, values):
    """(mask, dense) from numpy's own `a[:, idx, :] = values` on a zero array, and on an array of ones for the mask."""
    dense = np.zeros((B, L, DM), np.float32)
    dense[:, idx, :] = values
    seen = np.zeros((B, L, DM), np.float32)
    seen[:, idx, :] = 1.0
    return seen[:, :, 0].astype(np.uint8), dense


def rows(n, seed=0):
    return np.random.default_rng(seed).standard_normal((n, DM)).astype(np.float32)


BOOL = np.zeros(L, bool)
BOOL[[0, 5, L - 1]] = True

CASES = {
    "list": ([0, 5, L - 1], rows(3)),
    "negative": ([-1, -L, 4], rows(3, 1)),
    "slice": (slice(3, 20, 4), rows(5, 2)),
    "slice_all": (slice(None), rows(L, 3)),
    "bool": (BOOL, rows(3, 4)),
    "one_row_for_all": ([2, 9], rows(1, 5)),
    "scalar": (7, rows(1, 6)[0]),
    "empty": ([], rows(0)),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("B", [1, 3])
def test_dense_guidance_equals_numpy_assignment(name, B):
    idx, vals = CASES[name]
    want_mask, want = numpy_assign(B, idx, vals)
    for as_tensor in (False, True):
        i = torch.as_tensor(idx) if as_tensor and not isinstance(idx, slice) else idx
        v = torch.from_numpy(np.asarray(vals)) if as_tensor else vals
        mask, dense = sampler.dense_guidance(i, v, B, L, DM)
        assert mask.dtype == torch.uint8 and dense.dtype == torch.float32
        assert tuple(mask.shape) == (B, L) and tuple(dense.shape) == (B, L, DM)
        assert np.array_equal(mask.numpy(), want_mask) and np.array_equal(dense.numpy(), want), name


def test_dense_guidance_per_clip_values_and_repeats():
    # (B, G, dm) values: every clip its own rows
    B = 2
    vals = np.random.default_rng(7).standard_normal((B, 3, DM)).astype(np.float32)
    mask, dense = sampler.dense_guidance([1, 2, 30], vals, B, L, DM)
    want_mask, want = numpy_assign(B, [1, 2, 30], vals)
    assert np.array_equal(dense.numpy(), want) and np.array_equal(mask.numpy(), want_mask)
    # a repeated index: the last occurrence wins
    v = rows(3, 8)
    mask, dense = sampler.dense_guidance([4, 9, 4], v, 1, L, DM)
    assert np.array_equal(dense.numpy()[0, 4], v[2]) and np.array_equal(dense.numpy()[0, 9], v[1])
    assert mask.numpy().sum() == 2
    mask, dense = sampler.dense_guidance([4, -L + 4], v[:2], 1, L, DM)      # the same frame under two spellings
    assert np.array_equal(dense.numpy()[0, 4], v[1]) and mask.numpy().sum() == 1


@pytest.mark.parametrize("idx", [[L], [0, -L - 1], np.ones(L + 1, bool), torch.tensor([3, L + 5])])
def test_dense_guidance_out_of_range_raises(idx):
    n = int(np.asarray(idx).sum()) if np.asarray(idx).dtype == bool else len(idx)
    with pytest.raises(IndexError):
        sampler.dense_guidance(idx, rows(n), 1, L, DM)


def test_dense_guide_stack_mixes_clips_with_and_without_keyframes():
    v = rows(2, 9)
    g = sampler.DenseGuide.stack([([0, L - 1], v), None, ([5], v[:1])], L, DM)
    assert tuple(g.mask.shape) == (3, L) and tuple(g.values.shape) == (3, L, DM)
    assert g.mask[0].nonzero().flatten().tolist() == [0, L - 1] and int(g.mask[1].sum()) == 0
    assert g.mask[2].nonzero().flatten().tolist() == [5] and np.array_equal(g.values[2, 5].numpy(), v[0])


def test_solver_arguments_of_the_guided_and_separated_entry_points():
    """sample_separate / sample_with_guide take sample_steps, solver and eta after the reference's parameters, with the DDPM
    defaults, and hand them to check_solver's rules (the refusal of a few-step solver beside guidance or separation is gone)."""
    from msmd_amd.model import MSMD
    for fn in (MSMD.sample_separate, MSMD.sample_with_guide):
        p = inspect.signature(fn).parameters
        assert list(p)[-3:] == ["sample_steps", "solver", "eta"]
        assert (p["sample_steps"].default, p["solver"].default, p["eta"].default) == (None, "ddpm", 0.0)
    assert "guidance" in inspect.signature(sampler.sample).parameters
    assert sampler.check_solver(500, 25, "dpmpp_2m") == 25
    assert sampler.check_solver(500, 5, "ddim", 1.0) == 5
    assert sampler.check_solver(500, None, "ddpm") == 500
    for bad in (dict(sample_steps=25, solver="ddpm"), dict(sample_steps=4, solver="dpmpp_2m", eta=0.5),
                dict(sample_steps=0, solver="ddim"), dict(sample_steps=4, solver="heun")):
        with pytest.raises(ValueError):
            sampler.check_solver(500, **bad)
    for fn in (infer_coeffs, infer_coeffs_batch):
        kf = inspect.signature(fn).parameters["keyframes"]
        assert kf.kind is inspect.Parameter.KEYWORD_ONLY and kf.default is None


def test_per_clip_keyframes_need_a_few_step_solver():
    """infer_coeffs_batch's clips pin different frames (a dense per-clip guide), which the DDPM chain's index put cannot take."""
    from types import SimpleNamespace
    args = SimpleNamespace(n_motions=100, n_prev_motions=10, fps=25)
    with pytest.raises(ValueError, match="few-step|ddim"):
        infer_coeffs_batch(None, args, [torch.zeros(64000)], None, 640.0, None, keyframes=[([3], torch.zeros(1, 67))])


def test_keyframes_are_split_over_windows():
    n_motions = 100
    clip_len, _, n_win, _, _ = window_plan(160000, 25, n_motions, 640.0)          # a 10 s clip
    assert (clip_len, n_win) == (250, 3)
    vals = torch.arange(4 * 5, dtype=torch.float32).reshape(4, 5)
    per = window_keyframes(([3, 99, 100, 249], vals), clip_len, n_motions, n_win)
    assert [p[0] for p in per] == [[3, 99], [0], [49]]
    assert torch.equal(per[0][1], vals[:2]) and torch.equal(per[1][1], vals[2:3]) and torch.equal(per[2][1], vals[3:])
    # tensors of indices, windows without keyframes, no keyframes at all
    per = window_keyframes((torch.tensor([120]), vals[:1]), clip_len, n_motions, n_win)
    assert per[0] is None and per[2] is None and per[1][0] == [20]
    assert window_keyframes(None, clip_len, n_motions, n_win) == [None] * 3
    per = window_keyframes(([3, 249, 99], [[1.0], [2.0], [3.0]]), clip_len, n_motions, n_win)        # a plain list of rows
    assert per[0] == ([3, 99], [[1.0], [3.0]]) and per[1] is None and per[2] == ([49], [[2.0]])
    for bad in (250, 300, -1):
        with pytest.raises(IndexError):
            window_keyframes(([3, bad], vals[:2]), clip_len, n_motions, n_win)
