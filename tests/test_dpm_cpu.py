"""CPU: the data-prediction ODE solvers (deterministic DDIM, DPM-Solver++ 2M) and the log-SNR step grid (an extension not in the
reference) -- the C ABI and Python surface exist, the hydra `sampler=dpm` option resolves, bad arguments are refused before any device
work, the grid is what it says, and the float64 restatement the GPU parity tests compare against (tests/dpm_ref.py) integrates the
ODE correctly: against the exact Gaussian flow of tests/test_ode_cpu.py its error falls at the solver's order."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from tests import dpm_ref as D
from tests.test_ode_cpu import B, C, SDES, T, _exact, _gauss, _model, _x1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "cmd", "conf")


def _scheduler(kind, p0, p1, eps=1e-5):
    from fourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler
    return (VPScheduler if kind == "vp" else VEScheduler)(p0, p1, eps=eps)


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_sampler_run_dpm", "fd_dpm_stage"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


def test_sampler_surface_and_hydra_option():
    import inspect

    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler, ODESampler
    from fourierdiffusion_amd.schedulers.sde import SDE
    for name in ("sample_ode", "encode", "decode"):
        assert "schedule" in inspect.signature(getattr(DiffusionSampler, name)).parameters
    for name in ("log_snr", "t_of_log_snr", "dpm_step"):
        assert callable(getattr(SDE, name))
    cfg = compose(CONF, "sample", ["sampler=dpm", "num_diffusion_steps=20"])
    s = instantiate(cfg.sampler)(score_model=_model())
    assert type(s) is ODESampler and s.solver == "dpmpp2m" and s.schedule == "logsnr" and s.sample_batch_size == 200
    assert cfg.num_diffusion_steps == 20
    s = instantiate(compose(CONF, "sample", ["sampler=dpm", "sampler.solver=ddim", "sampler.schedule=time"]).sampler)(score_model=_model())
    assert s.solver == "ddim" and s.schedule == "time"
    # the existing option keeps its behaviour
    s = instantiate(compose(CONF, "sample", ["sampler=ode"]).sampler)(score_model=_model())
    assert s.solver == "heun" and s.schedule == "time"


@pytest.mark.parametrize("bad", ["schedule", "ctor_schedule", "encode_ddim", "encode_dpmpp2m", "likelihood", "solver", "ctor_solver",
                                 "encode_schedule"])
def test_rejects_bad_arguments(bad):
    """Every check runs before anything touches a device (there is none here)."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler, ODESampler
    s = DiffusionSampler(score_model=_model(), sample_batch_size=4)
    x = torch.zeros(2, 20, 3)
    with pytest.raises(ValueError):
        if bad == "schedule":
            s.sample_ode(4, 5, solver="dpmpp2m", schedule="cosine")
        elif bad == "ctor_schedule":
            ODESampler(score_model=_model(), sample_batch_size=4, solver="dpmpp2m", schedule="karras")
        elif bad == "encode_ddim":
            s.encode(x, 4, solver="ddim")
        elif bad == "encode_dpmpp2m":
            s.encode(x, 4, solver="dpmpp2m", schedule="logsnr")
        elif bad == "likelihood":
            s.log_likelihood(x, 4, solver="dpmpp2m")
        elif bad == "solver":
            s.decode(x, 4, solver="dpmpp3m")
        elif bad == "ctor_solver":
            ODESampler(score_model=_model(), sample_batch_size=4, solver="rk4")
        else:
            s.encode(x, 4, schedule="logsnr ")


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("kind,p0,p1", SDES)
def test_log_snr_inverts(kind, p0, p1):
    sch = _scheduler(kind, p0, p1)
    sde = O.SDEParams(kind, p0, p1, O.noise_scaling(T, False))
    worst = 0.0
    for t in (1e-5, 0.3, 1.0):
        lam = sch.log_snr(t)
        alpha, s = sch.marginal_coef(t)
        assert math.isclose(lam, D.log_snr(sde, t), rel_tol=1e-13, abs_tol=1e-13)
        if t > 1e-5:      # (marginal_coef's own s = sqrt(1 - alpha^2) has lost half its digits at eps)
            assert math.isclose(lam, math.log(alpha / s), rel_tol=1e-9, abs_tol=1e-9)
        back = sch.t_of_log_snr(lam)
        worst = max(worst, abs(back - t) / t)
        assert abs(back - t) <= 1e-9 * t, (kind, t, back)
        assert abs(D.t_of_log_snr(sde, lam) - t) <= 1e-9 * t
    assert sch.log_snr(0.2) > sch.log_snr(0.3)      # decreasing in t
    print(f"{kind}: worst relative inversion error {worst:.2e}")


@pytest.mark.parametrize("kind,p0,p1", SDES)
def test_logsnr_grid_ends_and_monotone(kind, p0, p1):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    sch = _scheduler(kind, p0, p1)
    sde = O.SDEParams(kind, p0, p1, O.noise_scaling(T, False))
    for N in (1, 2, 10, 50, 333, 1000):
        ts = DiffusionSampler.logsnr_grid(sch, N)
        assert ts.dtype == torch.float32 and ts.shape == (N + 1,)
        assert float(ts[0]) == 1.0 and float(ts[-1]) == float(np.float32(1e-5))
        gaps = (ts[:-1] - ts[1:]).numpy()
        assert (gaps > 0).all(), (kind, N, gaps.min())
        np.testing.assert_array_equal(ts.numpy(), D.grid(sde, N, "logsnr"))
        # uniform in lambda: the float32 cast moves t by at most 2^-24 t and lambda by |dlambda/dt| times that, which is largest at
        # t = 1 (VP beta_1 / 2 = 10, VE ln(sigma_max / sigma_min) = 8.5): 6e-7 per point, two points per difference
        lam = np.array([sch.log_snr(float(t)) for t in ts])
        h = np.diff(lam)
        assert (h > 0).all() and np.abs(h - h.mean()).max() <= 2e-6, (kind, N, np.abs(h - h.mean()).max())
    print(f"{kind}: smallest float32 gap at N = 1000: {gaps.min():.2e}")


def test_ve_logsnr_grid_is_the_time_grid():
    """VE: t is affine in lambda, so the two grids are the same points: every one within one float32 ulp (of that point) of
    torch.linspace's."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    sch = _scheduler("ve", 0.01, 50.0)
    for N in (1, 7, 10, 50, 100, 1000):
        a = DiffusionSampler.logsnr_grid(sch, N).numpy()
        b = torch.linspace(1.0, 1e-5, N + 1).numpy()
        ulps = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(a, b)).astype(np.float64)
        assert ulps.max() <= 1.0, (N, ulps.max())


def test_sampler_grid_schedules():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    s = DiffusionSampler(score_model=_model(), sample_batch_size=4)
    arr, N = s._ode_grid(12, to_noise=False)
    np.testing.assert_array_equal(np.array(arr[:]), torch.linspace(1.0, 1e-5, 13).numpy())      # the default is today's grid
    arr_t, _ = s._ode_grid(12, to_noise=False, schedule="time")
    assert arr_t[:] == arr[:]
    down, _ = s._ode_grid(12, to_noise=False, schedule="logsnr")
    up, _ = s._ode_grid(12, to_noise=True, schedule="logsnr")
    assert down[:] == up[:][::-1] and down[0] == 1.0 and up[0] == float(np.float32(1e-5))
    np.testing.assert_array_equal(np.array(down[:], dtype=np.float32), DiffusionSampler.logsnr_grid(s.noise_scheduler, 12).numpy())


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kind,p0,p1", SDES)
@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("solver,order", [("dpmpp2m", 2), ("ddim", 1)])
def test_convergence_order_against_exact_flow(kind, p0, p1, scaling, solver, order):
    sde, var, score = _gauss(kind, p0, p1, scaling)
    x1 = _x1(var)
    errs = []
    for N in (80, 160, 320):
        ts = D.grid(sde, N, "logsnr")
        ref = _exact(var, x1, float(ts[0]), float(ts[-1]))
        errs.append(np.abs(D.solve(sde, score, x1, ts, solver) - ref).max() / np.abs(ref).max())
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print(f"{kind} scaling={scaling} {solver}: errors {errs}, ratios {ratios}")
    lo, hi = (3.4, 4.6) if order == 2 else (1.75, 2.25)
    assert all(lo <= r <= hi for r in ratios), ratios
    if order == 2:
        assert errs[-1] < 1e-3


@pytest.mark.parametrize("kind,p0,p1", SDES)
@pytest.mark.parametrize("scaling", [False, True])
def test_2m_without_correction_is_ddim_and_ddim_is_its_closed_form(kind, p0, p1, scaling):
    sde, var, score = _gauss(kind, p0, p1, scaling)
    x1 = _x1(var)
    ts = D.grid(sde, 12, "logsnr")
    a = D.solve(sde, score, x1, ts, "dpmpp2m", r_inf=True)
    b = D.solve(sde, score, x1, ts, "ddim")
    np.testing.assert_array_equal(a, b)
    assert np.abs(D.solve(sde, score, x1, ts, "dpmpp2m") - b).max() > 1e-6 * np.abs(b).max()      # (the correction does something)
    rng = np.random.default_rng(3)
    x, s = rng.standard_normal((B, T, C)), rng.standard_normal((B, T, C))
    for t0, t1 in ((1.0, 0.8), (0.37, 0.2), (1e-3, 1e-5)):
        d = D.data_prediction(sde, s, t0, x)
        got, ref = D.step(sde, x, d, t0, t1), D.ddim_closed_form(sde, x, d, t0, t1)
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
