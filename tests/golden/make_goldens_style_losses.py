"""Records tests/golden/g14_style_losses.npz: the REFERENCE `StyleAdherenceLoss` and `nt_xent_loss` (utils/common.py) run on
small synthetic inputs.

    python tests/golden/make_goldens_style_losses.py /path/to/reference/checkout

The reference module is imported at recording time only (it needs nothing but torch).  The archive holds data only: inputs
that are exactly representable in fp32, the reference's outputs and autograd gradients as it runs (fp32), the same code
evaluated in float64 (`torch.Tensor.float` is the identity for the duration of the adherence call, which casts its inputs;
`nt_xent_loss` takes doubles as they are), and the `inspect.signature` strings of the three callables.
tests/test_style_losses_cpu.py pins tests/style_losses_ref.py's restatement to these values."""
import contextlib
import importlib.util
import inspect
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (B, T, K, F, lambda, soft, offset added to X)
ADHERENCE = {
    "soft10": (2, 5, 7, 6, 10.0, True, 0.0),
    "soft100": (2, 5, 7, 6, 100.0, True, 0.0),
    "hard": (2, 5, 7, 6, 10.0, False, 0.0),
    "k1": (2, 4, 1, 3, 10.0, True, 0.0),
    "far": (1, 4, 9, 5, 10.0, True, 11.0),         # every d >= 100: sum exp(-lambda d) underflows in fp32
}
# name: (B, D, temperature)
NT_XENT = {"b1": (1, 8, 0.5), "b2": (2, 8, 0.5), "b16": (16, 8, 0.5), "b16_t007": (16, 8, 0.07)}


def load_reference(ref_root):
    spec = importlib.util.spec_from_file_location("reference_utils_common", os.path.join(ref_root, "utils", "common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fp32_values(rng, shape, scale):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def run_adherence(ref, X, S, g_rows, lam, soft, dtype):
    """-> dict: loss (reduce=True), rows (reduce=False; the scalar again in the hard form), and the autograd gradients of both."""
    out = {}
    identity = mock.patch.object(torch.Tensor, "float", lambda self: self) if dtype == torch.float64 else contextlib.nullcontext()
    with identity:
        loss_fn = ref.StyleAdherenceLoss(use_soft_min=soft, lambda_softmin=lam)
        for reduce in (True, False):
            x = torch.from_numpy(X).to(dtype).requires_grad_(True)
            s = torch.from_numpy(S).to(dtype).requires_grad_(True)
            y = loss_fn(x, s, reduce=reduce)
            assert y.dtype == dtype
            up = torch.from_numpy(g_rows).to(dtype) if y.dim() else torch.ones((), dtype=dtype)
            y.backward(up)
            tag = "mean" if reduce else "rows"
            out[tag], out[tag + "_dX"], out[tag + "_dS"] = y.detach().numpy(), x.grad.numpy(), s.grad.numpy()
    return out


def run_nt_xent(ref, a, b, tau, dtype):
    ta = torch.from_numpy(a).to(dtype).requires_grad_(True)
    tb = torch.from_numpy(b).to(dtype).requires_grad_(True)
    y = ref.nt_xent_loss(ta, tb, tau)
    assert y.dtype == dtype
    y.backward()
    return dict(loss=y.detach().numpy(), da=ta.grad.numpy(), db=tb.grad.numpy())


def main(ref_root):
    ref = load_reference(ref_root)
    rng = np.random.default_rng(20261020)
    z = {"adherence_cases": np.array(list(ADHERENCE)), "nt_xent_cases": np.array(list(NT_XENT)),
         "torch_version": np.array(torch.__version__),
         "signatures": np.array([str(inspect.signature(ref.StyleAdherenceLoss)),
                                 str(inspect.signature(ref.StyleAdherenceLoss.forward)),
                                 str(inspect.signature(ref.nt_xent_loss))])}
    for name, (B, T, K, F, lam, soft, offset) in ADHERENCE.items():
        X = (fp32_values(rng, (B, T, F), 0.6) + np.float32(offset)).astype(np.float32)
        S = fp32_values(rng, (B, K, F), 0.6)
        g = fp32_values(rng, (B, T), 1.0)
        z.update({f"{name}/X": X, f"{name}/S": S, f"{name}/g": g, f"{name}/lambda": np.float64(lam), f"{name}/soft": np.bool_(soft)})
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            for k, v in run_adherence(ref, X, S, g, lam, soft, dtype).items():
                z[f"{name}/{tag}/{k}"] = v
        if offset:
            d = ((X.astype(np.float64)[:, :, None] - S.astype(np.float64)[:, None]) ** 2).mean(-1)
            assert d.min() >= 100.0, d.min()
            assert float(np.exp(np.float32(-lam) * d.astype(np.float32)).sum()) == 0.0
            assert np.isfinite(z[f"{name}/f32/rows"]).all()
    for name, (B, D, tau) in NT_XENT.items():
        a, b = fp32_values(rng, (B, D), 1.0), fp32_values(rng, (B, D), 1.0)
        z.update({f"{name}/a": a, f"{name}/b": b, f"{name}/temperature": np.float64(tau)})
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            for k, v in run_nt_xent(ref, a, b, tau, dtype).items():
                z[f"{name}/{tag}/{k}"] = v
    out = os.path.join(HERE, "g14_style_losses.npz")
    np.savez_compressed(out, **z)
    print(f"wrote {out}: {len(z)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
