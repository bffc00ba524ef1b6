"""CPU: log-likelihood through the probability-flow ODE (an extension not in the reference) -- the C ABI exists, the float64
restatement the GPU tests compare against is right (against the closed-form density of Gaussian data it converges at the solver's
order; the published prior's error stays within its bound; the Hutchinson estimator is unbiased), the change of variables to data
space is right for odd and even T, and bad arguments are refused before any device work."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from tests import likelihood_ref as L
from tests import ode_ref as R


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_score_input_vjp", "fd_prior_logp", "fd_likelihood_run"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


def _sde(kind, scaling, T):
    p = (0.1, 20.0) if kind == "vp" else (0.01, 50.0)
    return O.SDEParams(kind, p[0], p[1], O.noise_scaling(T, scaling))


def _gauss_case(kind, scaling, T=6, C=2, B=3, sigma0=0.8, seed=0):
    sde = _sde(kind, scaling, T)
    x0 = sigma0 * np.random.default_rng(seed).standard_normal((B, T, C))
    return sde, x0, sigma0


def _ll_exact_marginal(sde, x0, sigma0, N, solver):
    """The restatement with the closed-form trace and the exact marginal at t = 1 as the prior."""
    T, C = x0.shape[1], x0.shape[2]
    ts = R.grid(N, to_noise=True)
    lp, *_ = L.log_likelihood(sde, L.gaussian_score(sde, sigma0), L.gaussian_trace(sde, sigma0, C), x0, ts, solver,
                              prior_fn=lambda z: L.normal_logp(z, L.gaussian_var(sde, sigma0, 1.0)))
    return lp


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("solver,ratio,Ns", [("heun", (3.0, 5.0), (64, 128, 256)), ("euler", (1.6, 2.4), (256, 512, 1024))])
def test_restatement_converges_to_the_closed_form(kind, scaling, solver, ratio, Ns):
    sde, x0, sigma0 = _gauss_case(kind, scaling)
    # data N(0, sigma0^2) at t = eps: the ODE starts from the marginal at eps (alpha(eps)^2 sigma0^2 + s(eps)^2 G^2)
    truth = L.normal_logp(x0, L.gaussian_var(sde, sigma0, float(R.grid(1, to_noise=True)[0])))
    errs = [np.abs(_ll_exact_marginal(sde, x0, sigma0, N, solver) - truth).max() for N in Ns]
    # (and the closed form at eps is the one of sigma0^2 up to the tiny noise level there)
    assert np.abs(truth - L.normal_logp(x0, np.full(x0.shape[1], sigma0 ** 2))).max() < 5e-3
    assert errs[2] < 0.02 * np.abs(truth).max(), errs
    for a, b in zip(errs, errs[1:]):
        assert ratio[0] <= a / b <= ratio[1], (errs, a / b)


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("scaling", [False, True])
def test_published_prior_error_within_its_bound(kind, scaling):
    sde, x0, sigma0 = _gauss_case(kind, scaling, seed=1)
    ts = R.grid(64, to_noise=True)
    score, tr = L.gaussian_score(sde, sigma0), L.gaussian_trace(sde, sigma0, x0.shape[2])
    v1 = L.gaussian_var(sde, sigma0, 1.0)
    lp_pub, prior, _, _, x1 = L.log_likelihood(sde, score, tr, x0, ts, "heun")
    lp_ex, *_ = L.log_likelihood(sde, score, tr, x0, ts, "heun", prior_fn=lambda z: L.normal_logp(z, v1))
    vp = ((sde.p1 if kind == "ve" else 1.0) * sde.G) ** 2
    # |log N(x; 0, vp) - log N(x; 0, v1)| <= sum 0.5 |log(vp / v1)| + 0.5 x^2 |1/vp - 1/v1|
    bound = (0.5 * np.abs(np.log(vp / v1))[None, :, None] + 0.5 * x1 ** 2 * np.abs(1 / vp - 1 / v1)[None, :, None]).sum(axis=(1, 2))
    assert np.all(np.abs(lp_pub - lp_ex) <= bound + 1e-12)
    np.testing.assert_allclose(prior, L.prior_logp(sde, x1))


@pytest.mark.parametrize("estimator", ["rademacher", "gaussian"])
def test_hutchinson_mean_matches_exact_trace(estimator):
    T, C, P = 5, 2, 4000
    rng = np.random.default_rng(3)
    G = O.noise_scaling(T, True).astype(np.float64)
    M = rng.standard_normal((T * C, T * C)) / math.sqrt(T * C)
    score = lambda x, t: (x.reshape(x.shape[0], -1) @ M.T).reshape(x.shape) * (1.0 + t)      # noqa: E731 (dense Jacobian)
    x = rng.standard_normal((1, T, C))
    exact = L.fd_trace(score, G)(x, 0.3)[0]
    g2 = np.repeat(G ** 2, C)
    np.testing.assert_allclose(exact, 1.3 * float(np.sum(g2 * np.diag(M))), rtol=1e-6)
    e = rng.standard_normal((1, P, T, C))
    if estimator == "rademacher":
        e = np.where(e >= 0, 1.0, -1.0)
    est = L.fd_probe_trace(score, G, e)(x, 0.3)[0]
    se = est.std(ddof=1) / math.sqrt(P)
    assert se > 0 and abs(est.mean() - exact) <= 4 * se, (est.mean(), exact, se)


@pytest.mark.parametrize("T", [7, 8])
@pytest.mark.parametrize("fourier", [False, True])
def test_data_space_conversion(T, fourier):
    from fourierdiffusion_amd.sampling.likelihood import bits_per_dim, to_data_space
    C, sig = 3, 1.7
    rng = np.random.default_rng(T)
    y = sig * rng.standard_normal((4, T, C))                    # time-domain Gaussian data, as the user holds it
    F = L.dft_matrix(T) if fourier else np.eye(T)
    if fourier:
        assert abs(np.linalg.slogdet(F)[1] + ((T - 1) // 2) * math.log(2.0)) < 1e-9
    mean = rng.standard_normal((T, C))
    std = 0.5 + rng.random((T, C))
    x = (np.einsum("st,btc->bsc", F, y) - mean) / std           # sample space: standardised (spectrum)
    lp_sample = np.zeros(4)
    for c in range(C):                                          # x[:, :, c] ~ N(-mean / std, diag(1/std) F sig^2 F^T diag(1/std))
        cov = (F * sig ** 2) @ F.T / np.outer(std[:, c], std[:, c])
        d = x[:, :, c] + mean[:, c] / std[:, c]
        sign, logdet = np.linalg.slogdet(cov)
        lp_sample += -0.5 * np.einsum("bi,ij,bj->b", d, np.linalg.inv(cov), d) - 0.5 * logdet - 0.5 * T * math.log(2 * math.pi)
    truth = L.normal_logp(y, np.full(T, sig ** 2))
    got = to_data_space(torch.from_numpy(lp_sample), fourier, torch.from_numpy(std)).numpy()
    np.testing.assert_allclose(got, truth, rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(bits_per_dim(torch.from_numpy(truth), T, C).numpy(), -truth / (T * C * math.log(2.0)))
    if not fourier:      # no standardisation, no transform: the identity
        np.testing.assert_allclose(to_data_space(torch.from_numpy(truth), False, max_len=T, n_channels=C).numpy(), truth)


def test_packed_dft_log_det_values():
    from fourierdiffusion_amd.sampling.likelihood import data_space_offset
    for T, want in ((8, -3 * math.log(2.0)), (100, -49 * math.log(2.0))):
        assert abs(np.linalg.slogdet(L.dft_matrix(T))[1] - want) < 1e-8
        assert abs(data_space_offset(T, 1, True) - want) < 1e-12


def _model(T=8, C=3):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler(fourier_noise_scaling=True)
    sch.set_noise_scaling(T)
    return ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=8, num_layers=1, n_head=4)


@pytest.mark.parametrize("bad", ["grid", "shape", "n_probes", "exact_limit", "probe_shape", "estimator", "solver", "steps"])
def test_rejects_bad_arguments(bad):
    """Every check runs before the engine is touched: the model stays on the CPU, where any engine call would raise FdError."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    T, C = 8, 3
    kw = dict(X=torch.zeros(2, T, C), num_diffusion_steps=4)
    m = _model(T, C)
    if bad == "grid":
        m.noise_scheduler.eps = 1.0                 # linspace(1, 1, N + 1): not increasing
    elif bad == "shape":
        kw["X"] = torch.zeros(2, T + 1, C)
    elif bad == "n_probes":
        kw["n_probes"] = 0
    elif bad == "exact_limit":
        m = _model(200, 6)
        kw.update(X=torch.zeros(1, 200, 6), estimator="exact")
    elif bad == "probe_shape":
        kw.update(n_probes=2, probes=torch.zeros(2, 3, T, C))
    elif bad == "estimator":
        kw["estimator"] = "hutch"
    elif bad == "solver":
        kw["solver"] = "rk4"
    elif bad == "steps":
        kw["num_diffusion_steps"] = 0
    with pytest.raises(ValueError):
        DiffusionSampler(m, sample_batch_size=4).log_likelihood(**kw)


def test_drift_part_matches_the_restatement():
    from fourierdiffusion_amd.sampling.likelihood import drift_divergence
    sde = _sde("vp", True, 6)
    x0 = np.zeros((1, 6, 2))
    ts = R.grid(10, to_noise=True)
    for solver in ("euler", "heun"):
        _, _, drift, _, _ = L.log_likelihood(sde, lambda x, t: 0 * x, lambda x, t: np.zeros(x.shape[0]), x0, ts, solver)
        assert abs(drift_divergence(0, 0.1, 20.0, [float(t) for t in ts], solver, 12) - drift) < 1e-9 * abs(drift)
