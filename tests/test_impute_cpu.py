"""CPU: conditional sampling (imputation / forecasting, an extension not in the reference) -- the C ABI and Python surface exist,
the float64 restatement of the projection has the properties the engine's kernel relies on, and the mask builder of
cmd/impute.py hides what it should."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from tests import impute_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_impute_project", "fd_sampler_run_impute"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


def test_sampler_surface():
    from fdiff.sampling.sampler import DiffusionSampler as Alias
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    for name in ("impute", "impute_project", "observed_to_sample_space"):
        assert callable(getattr(DiffusionSampler, name))
    assert Alias is DiffusionSampler


def _sampler(T=20, C=3, corrector_steps=0):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler()
    sch.set_noise_scaling(T)
    m = ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=8, num_layers=1, n_head=4)
    return DiffusionSampler(score_model=m, sample_batch_size=4, corrector_steps=corrector_steps)


@pytest.mark.parametrize("bad", ["shape", "dtype", "mask_dtype", "mask_shape", "empty", "stats", "corrector"])
def test_impute_rejects_bad_arguments(bad):
    """Every check runs before anything touches a device."""
    s = _sampler(corrector_steps=1 if bad == "corrector" else 0)
    obs, mask = torch.zeros(2, 20, 3), torch.ones(2, 20, 3, dtype=torch.bool)
    kw = {}
    if bad == "shape":
        obs = torch.zeros(2, 21, 3)
    elif bad == "dtype":
        obs = torch.zeros(2, 20, 3, dtype=torch.int32)
    elif bad == "mask_dtype":
        mask = torch.ones(2, 20, 3)
    elif bad == "mask_shape":
        mask = torch.ones(20, 2, dtype=torch.bool)
    elif bad == "empty":
        obs, mask = torch.zeros(0, 20, 3), torch.ones(20, 3, dtype=torch.bool)
    elif bad == "stats":
        kw = dict(feature_mean=torch.zeros(20, 3))
    with pytest.raises(ValueError):
        s.impute(obs, mask, 5, fourier_transform=True, **kw)


def test_marginal_coef_matches_oracle():
    from fourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler
    for sch, osde in ((VPScheduler(0.1, 20.0), O.SDEParams("vp", 0.1, 20.0, np.ones(4))),
                      (VEScheduler(0.01, 50.0), O.SDEParams("ve", 0.01, 50.0, np.ones(4)))):
        for t in (1.0, 0.5, 1e-3):
            a, s = sch.marginal_coef(t)
            mean, std = O.marginal_prob(osde, np.ones((1, 4, 1)), np.array([t]))
            assert abs(a - mean[0, 0, 0]) <= 1e-12 and abs(s - std[0, 0]) <= 1e-12


@pytest.mark.parametrize("T", [24, 37, 100, 187])
def test_packed_dft_rows_orthogonal(T):
    """F F^T = diag(r), r = 1 at DC and Nyquist (T even), 1/2 elsewhere: idft = F^T diag(1/r) (the kernel's one basis)."""
    F = O.dft(np.eye(T)[None])[0]            # column t = dft of the unit impulse at t: F[r][t]
    r = np.full(T, 0.5)
    r[0] = 1.0
    if T % 2 == 0:
        r[T // 2] = 1.0
    np.testing.assert_allclose(F @ F.T, np.diag(r), atol=1e-12)
    y = np.random.RandomState(T).randn(1, T, 2)
    np.testing.assert_allclose(O.idft(y)[0], F.T @ (y[0] / r[:, None]), atol=1e-12)


def _case(T, C, standardize, seed=0):
    rs = np.random.RandomState(seed + T)
    B = 3
    mu = rs.randn(T, C) if standardize else np.zeros((T, C))
    sigma = rs.uniform(0.5, 2.0, (T, C)) if standardize else np.ones((T, C))
    G = O.noise_scaling(T, True).astype(np.float64)
    x, z, y = rs.randn(B, T, C), rs.randn(B, T, C), rs.randn(B, T, C)
    m = rs.rand(B, T, C) < 0.6
    y[~m] = np.nan                            # unobserved entries are ignored
    return B, mu, sigma, G, x, z, y, m


@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("T", [24, 37])
def test_projection_properties(T, standardize, fourier):
    C = 2
    B, mu, sigma, G, x, z, y, m = _case(T, C, standardize)
    x0 = R.x0_obs(y, m, mu, sigma, fourier)
    assert np.isfinite(x0).all()
    alpha, s = 0.7, 0.4
    # m = 0: identity;  m = 1: x_obs = alpha x0 + s G z
    np.testing.assert_allclose(R.project(x, x0, np.zeros((T, C), bool), sigma, G, alpha, s, z, fourier), x, atol=1e-12)
    x_obs = alpha * x0 + s * G[None, :, None] * z
    np.testing.assert_allclose(R.project(x, x0, np.ones((T, C), bool), sigma, G, alpha, s, z, fourier), x_obs, atol=1e-10)
    # the hard projection reproduces y on the observed entries and keeps A(x) on the others
    xp = R.project(x, x0, m, sigma, G, 1.0, 0.0, z, fourier)
    Ax, Axp = R.forward_map(x, mu, sigma, fourier), R.forward_map(xp, mu, sigma, fourier)
    np.testing.assert_allclose(Axp[m], y[m], atol=1e-10)
    np.testing.assert_allclose(Axp[~m], Ax[~m], atol=1e-10)
    # equals A^-1(m A(x_obs) + (1 - m) A(x)) at any level
    xs = R.project(x, x0, m, sigma, G, alpha, s, z, fourier)
    mix = np.where(m, R.forward_map(x_obs, mu, sigma, fourier), Ax)
    np.testing.assert_allclose(xs, ((O.dft(mix) if fourier else mix) - mu[None]) / sigma[None], atol=1e-10)


def test_mask_builder_random():
    from fourierdiffusion_amd.sampling.masks import observation_mask
    g = torch.Generator().manual_seed(0)
    m = observation_mask("random", (200, 50, 4), p=0.3, generator=g)
    assert m.dtype == torch.bool and m.shape == (200, 50, 4)
    assert abs((~m).double().mean().item() - 0.3) < 0.01
    again = observation_mask("random", (200, 50, 4), p=0.3, generator=torch.Generator().manual_seed(0))
    assert torch.equal(m, again)
    assert observation_mask("random", (2, 5, 3), p=0.0).all()
    assert not observation_mask("random", (2, 5, 3), p=1.0).any()
    with pytest.raises(ValueError):
        observation_mask("random", (2, 5, 3), p=1.5)


def test_mask_builder_forecast():
    from fourierdiffusion_amd.sampling.masks import observation_mask
    m = observation_mask("forecast", (3, 10, 2), horizon=4)
    assert m[:, :6].all() and not m[:, 6:].any()
    assert observation_mask("forecast", (1, 10, 2), horizon=10).sum() == 0
    for h in (0, 11):
        with pytest.raises(ValueError):
            observation_mask("forecast", (1, 10, 2), horizon=h)
    with pytest.raises(ValueError):
        observation_mask("blocks", (1, 10, 2))
