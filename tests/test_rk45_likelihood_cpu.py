"""CPU: adaptive (RK45) log-likelihood -- the C ABI entry exists, the float64 restatement the GPU tests compare against
(tests/rk45_ref.py) is scipy's RK45 (same tableau, same evaluations, same accepted times) and converges to the closed-form
divergence integral of Gaussian data as rtol shrinks, and bad rk45 arguments are refused before any engine call."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from tests import likelihood_ref as L
from tests import rk45_ref as K

integrate = pytest.importorskip("scipy.integrate")


def test_entry_point_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    assert "fd_likelihood_run_adaptive" in declared_symbols()
    assert "fd_likelihood_run_adaptive" in _C.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), "fd_likelihood_run_adaptive")


def test_tableau_equals_scipy():
    from scipy.integrate._ivp.rk import RK45
    assert np.array_equal(K.C, RK45.C)
    assert np.array_equal(K.A, RK45.A)
    assert np.array_equal(K.B, RK45.B)
    assert np.array_equal(K.E, RK45.E)
    assert RK45.error_estimator_order == 4 and RK45.n_stages == 6


def _sde(kind, scaling, T):
    p = (0.1, 20.0) if kind == "vp" else (0.01, 50.0)
    return O.SDEParams(kind, p[0], p[1], O.noise_scaling(T, scaling))


def _gauss_case(kind, scaling, T=6, C=2, B=3, sigma0=0.8, seed=0):
    sde = _sde(kind, scaling, T)
    x0 = sigma0 * np.random.default_rng(seed).standard_normal((B, T, C))
    return sde, x0, sigma0


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("rtol", [1e-3, 1e-5])
def test_restatement_is_scipy_rk45(kind, scaling, rtol):
    sde, x0, s0 = _gauss_case(kind, scaling)
    T, C = x0.shape[1:]
    score, trace = L.gaussian_score(sde, s0), L.gaussian_trace(sde, s0, C)
    rows = K.log_likelihood(sde, score, x0, rtol, rtol, trace_fn=trace)
    for b, r in enumerate(rows):
        fun = K.augmented(sde, score, trace, T, C)
        ref = integrate.solve_ivp(fun, (1e-5, 1.0), np.concatenate([x0[b].ravel(), [0.0]]), method="RK45", rtol=rtol, atol=rtol)
        assert ref.status == 0 and r["status"] == K.CONVERGED
        assert r["nfe"] == ref.nfev
        assert r["t"].shape == ref.t.shape
        assert np.max(np.abs(r["t"] - ref.t)) <= 1e-12
        assert np.max(np.abs(r["y"] - ref.y[:, -1])) <= 1e-12 * max(1.0, np.max(np.abs(ref.y[:, -1])))


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("scaling", [False, True])
def test_restatement_converges_to_the_closed_form(kind, scaling):
    sde, x0, s0 = _gauss_case(kind, scaling)
    C = x0.shape[2]
    exact = K.gaussian_delta(sde, s0, x0)
    errs, nfes = [], []
    for rtol in (1e-3, 1e-5, 1e-7):
        rows = K.log_likelihood(sde, L.gaussian_score(sde, s0), x0, rtol, rtol, trace_fn=L.gaussian_trace(sde, s0, C))
        err = max(abs(r["delta"] - exact) / abs(exact) for r in rows)
        assert err <= 10 * rtol, (rtol, err)
        errs.append(err)
        nfes.append(max(r["nfe"] for r in rows))
    assert errs[0] > errs[1] > errs[2]
    assert nfes[0] < nfes[1] < nfes[2]


def test_max_evals_freezes_the_row():
    sde, x0, s0 = _gauss_case("vp", True, B=1)
    r = K.log_likelihood(sde, L.gaussian_score(sde, s0), x0, 1e-7, 1e-7, trace_fn=L.gaussian_trace(sde, s0, 2), max_evals=20)[0]
    assert r["status"] == K.MAX_EVALS and r["nfe"] == 20 and r["nfe"] == 2 + 6 * len(r["err_norms"])


def _model(T=8, C=3):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler(fourier_noise_scaling=True)
    sch.set_noise_scaling(T)
    return ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=8, num_layers=1, n_head=4)


@pytest.mark.parametrize("bad", ["rtol", "atol", "max_evals", "interval", "rtol_nan"])
def test_rejects_bad_rk45_arguments(bad):
    """The model stays on the CPU, where any engine call would raise FdError (not a ValueError)."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    T, C = 8, 3
    kw = dict(X=torch.zeros(2, T, C), solver="rk45")
    m = _model(T, C)
    if bad == "rtol":
        kw["rtol"] = 0.0
    elif bad == "atol":
        kw["atol"] = -1e-5
    elif bad == "max_evals":
        kw["max_evals"] = 7
    elif bad == "interval":
        m.noise_scheduler.eps = 1.0
    elif bad == "rtol_nan":
        kw["rtol"] = float("nan")
    with pytest.raises(ValueError):
        DiffusionSampler(m, sample_batch_size=4).log_likelihood(**kw)


def test_rk45_ignores_num_diffusion_steps_in_its_checks():
    """num_diffusion_steps = 0 is refused for Heun but ignored by rk45: the call gets past every check to the engine, which a model
    on the CPU refuses with FdError."""
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    with pytest.raises(_C.FdError):
        DiffusionSampler(_model(), sample_batch_size=4).log_likelihood(torch.zeros(2, 8, 3), num_diffusion_steps=0, solver="rk45")


@pytest.mark.parametrize("call", ["encode", "decode"])
def test_ode_maps_reject_rk45(call):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    s = DiffusionSampler(_model(), sample_batch_size=4)
    with pytest.raises(ValueError, match="rk45"):
        getattr(s, call)(torch.zeros(2, 8, 3), 4, solver="rk45")
