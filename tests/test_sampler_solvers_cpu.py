"""Update-rule tables on the host: the DDPM table (sampler.ddpm_table) against its per-step restatement, and the few-step solver
tables (sampler.solver_table): timesteps, the DDPM identity of DDIM(eta = 1, S = T), the first-order rows of
DPM-Solver++(2M), and the argument checks.  No GPU."""
import math

import pytest
import torch

from msmd_amd.model import DiffusionSchedule
from msmd_amd.sampler import check_solver, ddpm_table, solver_table

SCHEDS = {T: DiffusionSchedule(T, "cosine") for T in (500, 20)}


def ddpm_coefficients(sched, t, target, flexibility=0):
    """The DDPM step's (c0, c1, sigma) at timestep t, restated one element at a time in fp32 as the reference computes them."""
    alpha, ab, abp = sched.alphas.float()[t], sched.alpha_bars.float()[t], sched.alpha_bars.float()[t - 1]
    if target == "noise":
        c0 = 1 / torch.sqrt(alpha)
        c1 = (1 - alpha) / torch.sqrt(1 - ab)
    else:
        c0 = (1 - abp) * torch.sqrt(alpha) / (1 - ab)
        c1 = (1 - alpha) * torch.sqrt(abp) / (1 - ab)
    sigma = sched.sigmas_flex.float()[t] * flexibility + sched.sigmas_inflex.float()[t] * (1 - flexibility)
    return float(c0), float(c1), float(sigma)


@pytest.mark.parametrize("T", [500, 20])
@pytest.mark.parametrize("target", ["sample", "noise"])
@pytest.mark.parametrize("flexibility", [0, 0.3])
def test_ddpm_table_is_the_per_step_restatement(T, target, flexibility):
    """Exact: the table's column operations and the restatement's scalar ones are the same correctly rounded IEEE fp32
    operations (sub, mul, div, sqrt) in the same order.  Row 1 carries sigma = 0 (no noise on the last step)."""
    sched = SCHEDS[T]
    table = ddpm_table(sched, flexibility, target)
    assert table.dtype == torch.float32 and table.shape == (T + 1, 3)
    for t in range(2, T + 1):
        assert tuple(table[t].tolist()) == ddpm_coefficients(sched, t, target, flexibility), t
    assert tuple(table[1].tolist()) == ddpm_coefficients(sched, 1, target, flexibility)[:2] + (0.0,)


@pytest.mark.parametrize("T", [500, 20])
@pytest.mark.parametrize("S", [1, 2, 3, 7, 10, 20, 25, 50, 200, 500])
def test_taus_trailing_spacing(T, S):
    if S > T:
        return
    for solver in ("ddim", "dpmpp_2m"):
        taus, rows = solver_table(SCHEDS[T], S, solver)
        assert len(taus) == S + 1 and taus[0] == 0 and taus[S] == T
        assert all(b > a for a, b in zip(taus, taus[1:]))
        assert taus == [math.floor(i * T / S + 0.5) for i in range(S + 1)]
        assert rows.dtype == torch.float64 and rows.shape == (S + 1, 6)
        assert torch.isfinite(rows).all() and not rows[0].any()


@pytest.mark.parametrize("T", [500, 20])
@pytest.mark.parametrize("target", ["sample", "noise"])
def test_ddim_eta1_full_steps_is_ddpm(T, target):
    """For adjacent steps abar_s = abar_t (1 - beta_s), so DDIM(eta = 1) is the DDPM posterior.  The table is computed from
    the fp32 alpha_bars buffer, which holds that identity only to its own rounding: 1 - abar_s / abar_t recovers beta_s
    with an absolute error of a few 2^-24, i.e. a relative one of a few 2^-24 / beta_s (beta_s >= 1e-4 here)."""
    sched = SCHEDS[T]
    taus, rows = solver_table(sched, T, "ddim", eta=1.0, target=target)
    assert taus == list(range(T + 1))
    u = 2.0 ** -24
    for s in range(1, T + 1):
        c0, c1, sig = ddpm_coefficients(sched, s, target)
        want = (c0, c1) if target == "sample" else (c0, -c0 * c1)
        p0, p1, ax, ath, b1, sigma = rows[s].tolist()
        if target == "sample":
            assert (p0, p1) == (0.0, 1.0)
        tol = 8 * u * (1 + 1 / float(sched.betas[s]))
        assert abs(ax - want[0]) <= tol * abs(want[0]), (s, ax, want[0])
        assert abs(ath - want[1]) <= tol * abs(want[1]), (s, ath, want[1])
        assert b1 == 0.0
        if s == 1:
            assert sigma == 0.0              # abar_0 = 1: the last step draws nothing, as the DDPM chain's z = 0 at t = 1
        else:
            assert abs(sigma - sig) <= tol * sig, (s, sigma, sig)
    if target == "noise":
        ab = sched.alpha_bars.double()
        assert torch.allclose(rows[1:, 0], 1 / ab[1:].sqrt(), rtol=1e-15)
        assert torch.allclose(rows[1:, 1], -(1 - ab[1:]).sqrt() / ab[1:].sqrt(), rtol=1e-15)


@pytest.mark.parametrize("T,S", [(500, 10), (500, 25), (500, 50), (500, 500), (20, 5), (20, 20), (20, 2)])
@pytest.mark.parametrize("target", ["sample", "noise"])
def test_dpmpp_first_order_rows_are_ddim0(T, S, target):
    sched = SCHEDS[T]
    taus, dpm = solver_table(sched, S, "dpmpp_2m", target=target)
    _, ddim = solver_table(sched, S, "ddim", eta=0.0, target=target)
    assert torch.equal(dpm[S], ddim[S]) and torch.equal(dpm[1], ddim[1])
    assert not dpm[:, 5].any() and not ddim[:, 5].any()
    if S > 2:
        assert dpm[2:S, 4].ne(0).all()     # second-order rows carry the previous data prediction
    # DPM-Solver++ at first order equals DDIM(0): a = sigma_t / sigma_s, b0 = -alpha_t (e^-h - 1)
    ab = sched.alpha_bars.double()
    s, t = taus[S], taus[S - 1]
    h = 0.5 * (math.log(ab[t] / (1 - ab[t])) - math.log(ab[s] / (1 - ab[s])))
    a, b0 = math.sqrt((1 - ab[t]) / (1 - ab[s])), -math.sqrt(ab[t]) * math.expm1(-h)
    p0, p1 = dpm[S, 0].item(), dpm[S, 1].item()
    assert dpm[S, 2].item() == pytest.approx(a + b0 * p0, rel=1e-12, abs=1e-12)
    assert dpm[S, 3].item() == pytest.approx(b0 * p1, rel=1e-12, abs=1e-12)


def test_solver_argument_errors():
    T = 500
    sched = SCHEDS[T]
    assert check_solver(T) == T and check_solver(T, T, "ddpm") == T and check_solver(T, 25, "ddim", 0.5) == 25
    with pytest.raises(ValueError, match="eta=1"):
        check_solver(T, 50, "ddpm")
    with pytest.raises(ValueError, match="flexibility"):
        check_solver(T, 50, "ddim", 0.0, flexibility=0.5)
    with pytest.raises(ValueError, match="flexibility"):
        check_solver(T, 50, "dpmpp_2m", flexibility=1)
    with pytest.raises(ValueError, match="Unknown solver"):
        check_solver(T, 50, "unipc")
    with pytest.raises(ValueError, match="Unknown solver"):
        solver_table(sched, 50, "dpmpp_3m")
    for bad in (0, -1, T + 1, 2.5):
        with pytest.raises(ValueError, match="sample_steps"):
            solver_table(sched, bad, "ddim")
        with pytest.raises(ValueError, match="sample_steps"):
            check_solver(T, bad, "dpmpp_2m")
    with pytest.raises(ValueError):
        solver_table(sched, T, "ddpm")
    with pytest.raises(ValueError, match="eta"):
        solver_table(sched, 50, "ddim", eta=1.5)
    with pytest.raises(ValueError, match="eta"):
        solver_table(sched, 50, "dpmpp_2m", eta=0.5)
