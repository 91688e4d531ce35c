"""FLAMETex without a GPU: the index rule against F.interpolate, the float64 restatement (tests/flametex_ref.py) against the
reference's recorded outputs and gradient (tests/golden/g12_flametex.npz), the module's surface and constructor, the C
header, and the command line."""
import inspect
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flametex_ref as R
from conftest import load_golden

N_TEX = 5


@pytest.mark.parametrize("S,D", [(512, 256), (7, 3), (5, 5), (3, 7), (10, 4), (4096, 1), (1, 1), (513, 256)])
def test_nearest_index_is_interpolates_rule(S, D):
    ramp = torch.arange(S, dtype=torch.float32).reshape(1, 1, 1, S)
    want = F.interpolate(ramp, [1, D]).reshape(-1).long().numpy()
    assert np.array_equal(R.nearest_index(S, D), want)
    if (S, D) == (512, 256):
        assert np.array_equal(want, 2 * np.arange(256))


@pytest.mark.parametrize("tex_type", ["BFM", "FLAME"])
@pytest.mark.parametrize("bs", [1, 3])
def test_restatement_reproduces_the_reference_outputs(tex_type, bs):
    g = load_golden("g12_flametex")
    tag = f"{tex_type}/bs{bs}"
    code = g[f"{tag}/code"]
    assert np.array_equal(code, __import__("msmd_amd.synth", fromlist=["x"]).normalish(f"flametex/code/{tag}", (bs, N_TEX)))
    assert tuple(g[f"{tag}/shape"]) == (bs, 3, 256, 256) and str(g[f"{tag}/dtype"]) == "torch.float32"
    assert bool(g[f"{tag}/copies_equal"])
    mean, basis = R.buffers(R.asset(tex_type, N_TEX), tex_type, N_TEX)
    value, mag = R.forward(mean, basis, code[0])
    pos = g["sample_pos"]
    err = np.abs(g[f"{tag}/samples"].astype(np.float64) - value.reshape(-1)[pos])
    bound = R.forward_bound(mag, N_TEX).reshape(-1)[pos]
    print(f"{tag}: worst error / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # the whole image through its sum: every element within its bound
    assert abs(float(g[f"{tag}/sum"]) - value.sum()) <= R.forward_bound(mag, N_TEX).sum()


@pytest.mark.parametrize("bs", [1, 2])
def test_restatement_reproduces_the_reference_gradient_exactly(bs):
    g = load_golden("g12_flametex")
    _, basis = R.buffers(R.asset("BFM", N_TEX, True), "BFM", N_TEX)
    assert np.array_equal(basis * 16, np.round(basis * 16))
    grad, _, _ = R.gradient(basis, R.ternary(f"flametex/grad_out/bs{bs}", (bs, 3, 256, 256)))
    want = g[f"grad/bs{bs}/texcode_grad"]
    assert want.shape == (bs, N_TEX) and np.array_equal(want[0].astype(np.float64), grad) and not want[1:].any()
    assert np.abs(grad).max() > 16


def test_module_surface_matches_the_recorded_reference():
    from msmd_amd.utils.flame import FLAMETex, FLAMEConfig
    g = load_golden("g12_flametex")
    assert str(inspect.signature(FLAMETex.__init__)) == str(g["signature/__init__"])
    assert str(inspect.signature(FLAMETex.forward)) == str(g["signature/forward"])
    assert hasattr(FLAMEConfig, "flame_tex_path") and hasattr(FLAMEConfig, "tex_path")
    for tex_type in ("BFM", "FLAME"):
        m = FLAMETex(SimpleNamespace(tex_type=tex_type, n_tex=N_TEX, tex_asset=R.asset(tex_type, N_TEX)))
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == json.loads(str(g[f"{tex_type}/state_dict"]))


def test_constructor_rules(tmp_path):
    from msmd_amd.utils.flame import FLAMETex
    for tex_type in ("BFM", "FLAME"):
        a = R.asset(tex_type, N_TEX)
        m = FLAMETex(SimpleNamespace(tex_type=tex_type, n_tex=3, tex_asset=a))            # the column slice
        mean, basis = R.buffers(a, tex_type, 3)
        assert m.texture_mean.shape == (1, 1, 786432) and m.texture_basis.shape == (1, 786432, 3)
        assert m.texture_mean.dtype == m.texture_basis.dtype == torch.float32
        assert m.texture_basis.is_contiguous() and m.texture_mean.is_contiguous()
        assert np.array_equal(m.texture_mean.numpy().reshape(-1), mean) and np.array_equal(m.texture_basis.numpy()[0], basis)
    # the /255 of the 'FLAME' space (reference l.272-273) and the keys of each space
    a = R.asset("FLAME", N_TEX)
    assert np.array_equal(mean, (a["mean"].reshape(-1) / 255.).astype(np.float32)) and a["mean"].max() > 200
    assert np.array_equal(basis[:, 0], (a["tex_dir"].reshape(-1, N_TEX)[:, 0] / 255.).astype(np.float32))
    # from a file, through the path the type reads
    bfm = R.asset("BFM", N_TEX)
    path = tmp_path / "bfm.npz"
    np.savez(path, MU=bfm["MU"], PC=bfm["PC"])
    m = FLAMETex(SimpleNamespace(tex_type="BFM", n_tex=N_TEX, tex_path=str(path), flame_tex_path="/nonexistent"))
    assert np.array_equal(m.texture_basis.numpy()[0], bfm["PC"])
    # the three errors
    with pytest.raises(NotImplementedError):
        FLAMETex(SimpleNamespace(tex_type="AlbedoMM", n_tex=N_TEX, tex_asset=bfm))
    with pytest.raises(ValueError, match="n_tex"):
        FLAMETex(SimpleNamespace(tex_type="BFM", n_tex=N_TEX + 1, tex_asset=bfm))
    with pytest.raises(ValueError, match="786432"):
        FLAMETex(SimpleNamespace(tex_type="BFM", n_tex=2, tex_asset=dict(MU=bfm["MU"][:300], PC=bfm["PC"][:300])))


def test_forward_on_a_cpu_tensor_raises():
    from msmd_amd.utils.flame import FLAMETex
    m = FLAMETex(SimpleNamespace(tex_type="BFM", n_tex=N_TEX, tex_asset=R.asset("BFM", N_TEX)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, N_TEX))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.image(torch.zeros(1, N_TEX))
    with pytest.raises(ValueError):
        m(torch.zeros(1, N_TEX + 1))


def test_header_declares_the_launchers_and_formats():
    from msmd_amd import _lib
    protos = _lib.parse_header()
    assert len(protos["msmd_flametex_forward"]) == 12 and len(protos["msmd_flametex_backward"]) == 11
    assert len(protos["msmd_flametex_backward_workspace"]) == 3
    assert _lib.RESTYPE["msmd_flametex_backward_workspace"] is __import__("ctypes").c_long
    src = open(_lib.HEADER).read()
    assert "#define MSMD_TEX_PLANAR_F32 0" in src and "#define MSMD_TEX_IMAGE_U8 1" in src
    from msmd_amd import ops
    assert (ops.TEX_PLANAR_F32, ops.TEX_IMAGE_U8) == (0, 1)
    lib = _lib.load()                                             # host-only entry: no GPU needed
    assert lib.msmd_flametex_backward_workspace(0, 4, 5) == -1 and lib.msmd_flametex_backward_workspace(4, 4, 257) == -1
    assert lib.msmd_flametex_backward_workspace(4097, 4, 5) == -1
    assert lib.msmd_flametex_backward_workspace(1, 1, 7) == 7 and lib.msmd_flametex_backward_workspace(256, 256, 50) % 50 == 0


REQUIRED = ["--model_root", "r", "--model_name", "n", "--model_iter", "1", "--style_clip_exp_code_path", "e",
            "--style_clip_head_rot_path", "h", "--audio_clip", "a.wav"]


def test_parse_args_rules(capsys):
    from msmd_amd.inference import parse_args
    a = parse_args(REQUIRED + ["--render_size", "64", "--flame_tex", "t.npz", "--tex_type", "FLAME", "--tex_code", "c.npy"])
    assert (a.flame_tex, a.tex_type, a.tex_code) == ("t.npz", "FLAME", "c.npy")
    a = parse_args(REQUIRED)
    assert (a.flame_tex, a.tex_type, a.tex_code) == (None, "BFM", None)
    for bad in (["--flame_tex", "t.npz"],                                                   # no frames to draw on
                ["--render_size", "64", "--flame_tex", "t.npz", "--texture", "u.npz"],      # two textures
                ["--render_size", "64", "--tex_code", "c.npy"],                             # a code without a space
                ["--render_size", "64", "--flame_tex", "t.npz", "--tex_type", "AlbedoMM"]):
        with pytest.raises(SystemExit):
            parse_args(REQUIRED + bad)
    capsys.readouterr()


def test_load_flame_texture_names_the_missing_keys(tmp_path):
    from msmd_amd.inference import load_flame_texture
    bfm = R.asset("BFM", N_TEX)
    path = tmp_path / "albedo.npz"
    np.savez(path, MU=bfm["MU"][:30], PC=bfm["PC"][:30], vt=bfm["vt"])
    with pytest.raises(ValueError, match="ft"):
        load_flame_texture(str(path), "BFM", None)
