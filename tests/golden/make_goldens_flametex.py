"""Records tests/golden/g12_flametex.npz: the REFERENCE FLAMETex (utils/flame.py:247-301) run on the CPU over the synthetic
albedo assets of msmd_amd.synth.flametex_asset -- both texture types, n_tex = 5, batch sizes 1 and 3 -- plus its module
surface and its own autograd gradient on the quantised BFM asset.

    python tests/golden/make_goldens_flametex.py /path/to/reference/checkout

The reference class is imported from that checkout at recording time only; the archive holds data only.  The asset is written
to a temporary directory with the components zero-padded to the 199 / 200 columns the reference hard-codes.
tests/test_flametex_cpu.py pins tests/flametex_ref.py's restatement to these values."""
import importlib
import inspect
import json
import os
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import flametex_ref as R  # noqa: E402
from msmd_amd import synth  # noqa: E402

N_TEX, N_SAMPLES = 5, 2048
SPACES = {"BFM": ("MU", "PC", 199, "tex_path"), "FLAME": ("mean", "tex_dir", 200, "flame_tex_path")}


def load_reference(ref_root):
    """utils/flame.py of the checkout as refutils.flame, without running the package's __init__ (it pulls in the whole project)."""
    pkg = types.ModuleType("refutils")
    pkg.__path__ = [os.path.join(ref_root, "utils")]
    sys.modules["refutils"] = pkg
    return importlib.import_module("refutils.flame")


def reference_module(ref, tex_type, asset, tmp):
    mu_key, pc_key, n_pc, path_attr = SPACES[tex_type]
    pc = asset[pc_key]
    padded = np.zeros(pc.shape[:-1] + (n_pc,), np.float32)
    padded[..., :pc.shape[-1]] = pc
    path = os.path.join(tmp, f"{tex_type}.npz")
    np.savez(path, **{mu_key: asset[mu_key], pc_key: padded})
    return ref.FLAMETex(SimpleNamespace(tex_type=tex_type, n_tex=N_TEX, **{path_attr: path}))


def main(ref_root):
    ref = load_reference(ref_root)
    out = {}
    pos = np.minimum((synth.uniform01("flametex/sample", N_SAMPLES) * np.float32(3 * 256 * 256)).astype(np.int64),
                     3 * 256 * 256 - 1)
    out["sample_pos"] = pos
    with tempfile.TemporaryDirectory() as tmp:
        for tex_type in SPACES:
            m = reference_module(ref, tex_type, synth.flametex_asset(tex_type, N_TEX), tmp)
            out[f"{tex_type}/state_dict"] = np.array(json.dumps({k: list(v.shape) for k, v in m.state_dict().items()}))
            for bs in (1, 3):
                code = synth.normalish(f"flametex/code/{tex_type}/bs{bs}", (bs, N_TEX))
                with torch.no_grad():
                    tex = m(torch.from_numpy(code))
                tag = f"{tex_type}/bs{bs}"
                out[f"{tag}/code"] = code
                out[f"{tag}/shape"] = np.array(tex.shape, np.int64)
                out[f"{tag}/dtype"] = np.array(str(tex.dtype))
                out[f"{tag}/samples"] = tex[0].reshape(-1).numpy()[pos]
                out[f"{tag}/sum"] = np.array(tex[0].double().sum().item())
                out[f"{tag}/copies_equal"] = np.array(all(torch.equal(tex[0], tex[k]) for k in range(bs)))
        # the reference's own gradient where it is exact: quantised BFM asset, grad_out in {-1, 0, 1}
        m = reference_module(ref, "BFM", synth.flametex_asset("BFM", N_TEX, quantised=True), tmp)
        for bs in (1, 2):
            code = torch.from_numpy(synth.normalish(f"flametex/code/grad/bs{bs}", (bs, N_TEX))).requires_grad_(True)
            m(code).backward(torch.from_numpy(R.ternary(f"flametex/grad_out/bs{bs}", (bs, 3, 256, 256))))
            out[f"grad/bs{bs}/code"] = code.detach().numpy()
            out[f"grad/bs{bs}/texcode_grad"] = code.grad.numpy()
    out["signature/__init__"] = np.array(str(inspect.signature(ref.FLAMETex.__init__)))
    out["signature/forward"] = np.array(str(inspect.signature(ref.FLAMETex.forward)))
    out["versions"] = np.array(json.dumps({"numpy": np.__version__, "torch": torch.__version__,
                                           "python": sys.version.split()[0]}))
    path = os.path.join(HERE, "g12_flametex.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
