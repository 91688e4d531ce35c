"""The style losses without a GPU: the float64 restatement (tests/style_losses_ref.py) and its closed-form gradients against the
reference's recorded outputs and autograd gradients (tests/golden/g14_style_losses.npz), the reference's own fp32 run against
the float32 yardstick, the public signatures, the ValueError cases, the C header and the built library's exports.

Tolerances.  The restatement against the float64 recording: 64 ulp of float64 at the tensor's largest magnitude (2^-52 x 64 =
1.4e-14 relative to the largest entry) -- two float64 evaluations of the same formula in different association; the far-row
case (lambda d ~ 1000, so exp's argument carries 1000 x 2^-53) gets the same 64 ulp scaled by lambda d_max.  The recorded fp32
run: `style_losses_ref.allowed`, i.e. 8 x the float32 restatement's distance from the truth, never less than 4 fp32 ulp."""
import inspect

import numpy as np
import pytest
import torch

import style_losses_ref as R
from conftest import load_golden
from msmd_amd.utils.common import StyleAdherenceLoss, nt_xent_loss      # the product's two public names: every test needs them

ADHERENCE = ("soft10", "soft100", "hard", "k1", "far")
NT_XENT = ("b1", "b2", "b16", "b16_t007")
U64 = 2.0 ** -52


@pytest.fixture(scope="module")
def g():
    return load_golden("g14_style_losses")


def case(g, name):
    X, S, rows_g = g[f"{name}/X"], g[f"{name}/S"], g[f"{name}/g"]
    return X, S, rows_g, float(g[f"{name}/lambda"]), bool(g[f"{name}/soft"])


def tol64(truth, amplification=1.0):
    return 64 * U64 * max(amplification, 1.0) * float(np.abs(truth).max())


def amplification(X, S, lam, soft):
    """How many float64 ulps of d reach the soft-min's weights: lambda d_max."""
    return lam * float(R.distances(X, S).max()) if soft else 1.0


def test_archive_holds_the_cases_and_fp32_inputs(g):
    assert tuple(str(c) for c in g["adherence_cases"]) == ADHERENCE and tuple(str(c) for c in g["nt_xent_cases"]) == NT_XENT
    for n in ADHERENCE:
        assert g[f"{n}/X"].dtype == np.float32 and g[f"{n}/S"].dtype == np.float32 and g[f"{n}/f64/mean"].dtype == np.float64
        assert g[f"{n}/f32/mean"].dtype == np.float32 and g[f"{n}/f32/mean"].shape == ()
    assert g["k1/S"].shape[1] == 1 and float(g["soft100/lambda"]) == 100.0 and not bool(g["hard/soft"])
    assert g["hard/f64/rows"].shape == ()                   # the hard form returns the scalar whatever `reduce` says
    assert g["soft10/f64/rows"].shape == g["soft10/g"].shape == (2, 5)
    assert R.distances(g["far/X"], g["far/S"]).min() >= 100.0
    assert [g[f"{n}/a"].shape[0] for n in NT_XENT] == [1, 2, 16, 16] and float(g["b16_t007/temperature"]) == 0.07


@pytest.mark.parametrize("name", ADHERENCE)
def test_adherence_restatement_equals_the_float64_recording(g, name):
    X, S, rows_g, lam, soft = case(g, name)
    amp = amplification(X, S, lam, soft)
    B, T = rows_g.shape
    mean, rows = R.adherence(X, S, lam, soft, True), R.adherence(X, S, lam, soft, False)
    assert np.shape(rows) == g[f"{name}/f64/rows"].shape
    errs = {"mean": (R.worst(mean, g[f"{name}/f64/mean"]), tol64(g[f"{name}/f64/mean"], amp)),
            "rows": (R.worst(rows, g[f"{name}/f64/rows"]), tol64(g[f"{name}/f64/rows"], amp))}
    grads = {"mean": R.adherence_grads(X, S, np.full((B, T), 1.0 / (B * T)), lam, soft)}
    # reduce=False with the recorded upstream; the hard form ignored `reduce`, so its second recording is the mean's again
    grads["rows"] = R.adherence_grads(X, S, rows_g, lam, soft) if soft else grads["mean"]
    for tag, (dX, dS) in grads.items():
        errs[tag + "_dX"] = (R.worst(dX, g[f"{name}/f64/{tag}_dX"]), tol64(g[f"{name}/f64/{tag}_dX"], amp))
        errs[tag + "_dS"] = (R.worst(dS, g[f"{name}/f64/{tag}_dS"]), tol64(g[f"{name}/f64/{tag}_dS"], amp))
    print(name, {k: f"{e:.1e} / {t:.1e}" for k, (e, t) in errs.items()})
    assert all(e <= t for e, t in errs.values()), errs


@pytest.mark.parametrize("name", ADHERENCE)
def test_adherence_identities_of_the_closed_form(g, name):
    """sum_k c = 1; the translation identity sum_t dX + sum_k dS = 0; K = 1 gives c = 1 and L = d."""
    X, S, rows_g, lam, soft = case(g, name)
    L, c, d = R.adherence_rows(X, S, lam, soft)
    amp = max(1.0, amplification(X, S, lam, soft))          # c holds lambda (d - L): lambda d_max ulps of d
    assert np.abs(c.sum(-1) - 1).max() <= 64 * U64 * amp * max(1.0, np.abs(c).max()) * c.shape[-1]
    dX, dS = R.adherence_grads(X, S, rows_g, lam, soft)
    scale = max(np.abs(dX).max() * dX.shape[1], np.abs(dS).max() * dS.shape[1])
    assert np.abs(dX.sum(1) + dS.sum(1)).max() <= 64 * U64 * scale
    if d.shape[-1] == 1:
        assert np.array_equal(c, np.ones_like(c)) and np.array_equal(L, d[..., 0])


@pytest.mark.parametrize("name", NT_XENT)
def test_nt_xent_restatement_equals_the_float64_recording(g, name):
    a, b, tau = g[f"{name}/a"], g[f"{name}/b"], float(g[f"{name}/temperature"])
    loss = R.nt_xent(a, b, tau)
    da, db = R.nt_xent_grads(a, b, tau)
    amp = 1.0 / tau                                        # the logits are 1 / tau times the cosines
    errs = {"loss": (R.worst(loss, g[f"{name}/f64/loss"]), 64 * U64 * amp * max(1.0, abs(float(g[f"{name}/f64/loss"])))),
            "da": (R.worst(da, g[f"{name}/f64/da"]), tol64(g[f"{name}/f64/da"], amp)),
            "db": (R.worst(db, g[f"{name}/f64/db"]), tol64(g[f"{name}/f64/db"], amp))}
    print(name, {k: f"{e:.1e} / {t:.1e}" for k, (e, t) in errs.items()})
    assert all(e <= t for e, t in errs.values()), errs
    if name == "b1":
        assert float(loss) == 0.0 and not da.any() and not db.any()


def test_nt_xent_clamped_row_gets_the_unprojected_gradient():
    """A row shorter than 1e-12 is divided by the constant 1e-12: torch's autograd (float64) passes nothing to its norm."""
    import torch.nn.functional as F
    rs = np.random.RandomState(3)
    a, b = rs.randn(3, 5), rs.randn(3, 5)
    a[1] *= 1e-20 / np.linalg.norm(a[1])
    ta, tb = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    f = F.normalize(torch.cat([ta, tb]), dim=1)
    s = (f @ f.T) / 0.5
    s = s.masked_fill(torch.eye(6, dtype=torch.bool), -np.inf)
    loss = (torch.logsumexp(s, 1) - s[torch.arange(6), (torch.arange(6) + 3) % 6]).mean()
    loss.backward()
    da, db = R.nt_xent_grads(a, b, 0.5)
    assert abs(float(loss.detach()) - float(R.nt_xent(a, b, 0.5))) <= 1e-14
    assert np.abs(da - ta.grad.numpy()).max() <= 1e-12 * np.abs(da).max() and np.abs(db - tb.grad.numpy()).max() <= 1e-14


@pytest.mark.parametrize("name", ADHERENCE)
def test_recorded_fp32_adherence_lies_within_the_yardstick(g, name):
    X, S, rows_g, lam, soft = case(g, name)
    B, T = rows_g.shape
    pairs = {"mean": R.adherence(X, S, lam, soft, True, np.float32), "rows": R.adherence(X, S, lam, soft, False, np.float32)}
    pairs["mean_dX"], pairs["mean_dS"] = R.adherence_grads(X, S, np.full((B, T), 1.0 / (B * T)), lam, soft, np.float32)
    if soft:
        pairs["rows_dX"], pairs["rows_dS"] = R.adherence_grads(X, S, rows_g, lam, soft, np.float32)
    for key, run32 in pairs.items():
        assert np.asarray(run32).dtype == np.float32
        truth = g[f"{name}/f64/{key}"]
        err, bound = R.worst(g[f"{name}/f32/{key}"], truth), R.allowed(truth, run32)
        print(f"{name}/{key}: the reference in fp32 is {err:.2e} from the truth, allowed {bound:.2e}")
        assert err <= bound, (name, key)


@pytest.mark.parametrize("name", NT_XENT)
def test_recorded_fp32_nt_xent_lies_within_the_yardstick(g, name):
    a, b, tau = g[f"{name}/a"], g[f"{name}/b"], float(g[f"{name}/temperature"])
    da, db = R.nt_xent_grads(a, b, tau, 1.0, np.float32)
    for key, run32 in (("loss", R.nt_xent(a, b, tau, np.float32)), ("da", da), ("db", db)):
        assert np.asarray(run32).dtype == np.float32
        truth = g[f"{name}/f64/{key}"]
        err, bound = R.worst(g[f"{name}/f32/{key}"], truth), R.allowed(truth, run32)
        print(f"{name}/{key}: the reference in fp32 is {err:.2e} from the truth, allowed {bound:.2e}")
        assert err <= bound, (name, key)


def test_signatures_equal_the_recorded_ones(g):
    got = [str(inspect.signature(StyleAdherenceLoss)), str(inspect.signature(StyleAdherenceLoss.forward)),
           str(inspect.signature(nt_xent_loss))]
    assert got == [str(s) for s in g["signatures"]]
    m = StyleAdherenceLoss()
    assert isinstance(m, torch.nn.Module) and m.use_soft_min is True and m.lambda_softmin == 10.0 and not list(m.parameters())


def test_value_errors_come_before_the_device_and_the_library(monkeypatch):
    from msmd_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    X, S = torch.zeros(2, 5, 6), torch.zeros(2, 7, 6)
    for loss in (StyleAdherenceLoss(), StyleAdherenceLoss(use_soft_min=False)):
        for bad_x, bad_s in ((X, torch.zeros(3, 7, 6)), (X, torch.zeros(2, 7, 5)), (X, torch.zeros(2, 0, 6)), (X[0], S),
                             (torch.zeros(2, 0, 6), S)):
            with pytest.raises(ValueError):
                loss(bad_x, bad_s)
    with pytest.raises(ValueError):
        StyleAdherenceLoss(lambda_softmin=-1.0)(X, S)
    for fn in (ops.style_adherence_forward, lambda x, s: ops.style_adherence_backward(x, s, None, None, None)):
        with pytest.raises(ValueError):
            fn(X, torch.zeros(2, 0, 6))
        with pytest.raises(ValueError):
            fn(X, torch.zeros(3, 7, 6))
    a = torch.zeros(4, 8)
    for bad_a, bad_b, tau in ((a, torch.zeros(3, 8), 0.5), (a, torch.zeros(4, 7), 0.5), (a, a, 0.0), (a, a, -0.07),
                              (a, a, float("nan")), (a[0], a[0], 0.5), (torch.zeros(0, 8), torch.zeros(0, 8), 0.5)):
        with pytest.raises(ValueError):
            nt_xent_loss(bad_a, bad_b, tau)
        with pytest.raises(ValueError):
            ops.nt_xent_forward(bad_a, bad_b, tau)
    # well-formed operands on the host: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        StyleAdherenceLoss()(X, S)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nt_xent_loss(a, a, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ordered_mean(torch.zeros(4))


def test_header_declares_and_the_library_exports_the_entry_points():
    from msmd_amd import _lib, autograd, ops
    protos = _lib.parse_header()
    counts = {"msmd_style_adherence_forward": 11, "msmd_style_adherence_backward": 16, "msmd_ordered_mean": 4,
              "msmd_nt_xent_forward": 10, "msmd_nt_xent_backward": 9}
    assert {n: len(protos[n]) for n in counts} == counts
    src = open(_lib.HEADER).read()
    for name, value in (("MSMD_STYLE_ROWS", ops.STYLE_ROWS), ("MSMD_STYLE_KTILE", ops.STYLE_KTILE),
                        ("MSMD_STYLE_FCHUNK", ops.STYLE_FCHUNK)):
        assert f"#define {name} {value}\n" in src
    for name in ("style_adherence_forward", "style_adherence_backward", "ordered_mean", "nt_xent_forward", "nt_xent_backward"):
        assert callable(getattr(ops, name))
    assert issubclass(autograd.StyleAdherenceFn, torch.autograd.Function) and issubclass(autograd.NtXentFn, torch.autograd.Function)
    lib = _lib.load()
    for name in counts:
        assert hasattr(lib, name)
    # argument checks come before any launch: no GPU needed
    one = ctypes_float_buffer()
    assert lib.msmd_style_adherence_forward(one, one, one, one, 1, 1, 0, 1, 10.0, 1, None) == 1
    assert lib.msmd_style_adherence_forward(one, one, one, one, 1, 1, 1, 0, 10.0, 1, None) == 1
    assert lib.msmd_style_adherence_forward(one, one, one, one, 1, 1, 1, 1, -1.0, 1, None) == 1
    assert lib.msmd_style_adherence_forward(None, one, one, one, 1, 1, 1, 1, 10.0, 1, None) == 1
    assert lib.msmd_style_adherence_backward(one, one, one, one, one, 2, 1.0, one, one, 1, 1, 1, 1, 10.0, 1, None) == 1
    assert lib.msmd_style_adherence_backward(one, one, one, one, one, 1, 1.0, None, None, 1, 1, 1, 1, 10.0, 1, None) == 1
    assert lib.msmd_ordered_mean(one, 0, one, None) == 1
    assert lib.msmd_nt_xent_forward(one, one, one, one, one, one, 0, 4, 0.5, None) == 1
    assert lib.msmd_nt_xent_forward(one, one, one, one, one, one, 1, 4, 0.0, None) == 1
    assert lib.msmd_nt_xent_backward(one, one, one, one, one, 1, 0, 0.5, None) == 1
    assert lib.msmd_nt_xent_backward(one, one, one, None, one, 1, 4, 0.5, None) == 1


def ctypes_float_buffer():
    """A non-NULL pointer for the argument checks; nothing is launched, so nothing reads it."""
    import ctypes
    buf = (ctypes.c_float * 4)()
    ctypes_float_buffer.keep = buf
    return ctypes.addressof(buf)
