"""CPU: gradient-guided conditional sampling (impute(conditioning="dps"), an extension not in the reference) -- the float64
restatement of tests/dps_ref.py gives g = -grad ||r||^2 (central differences through the closed-form Gaussian score, whose Jacobian
is exact, and through an oracle network), the new entry points exist, impute / impute_guidance check their arguments before any
device work, and cmd/conf/impute.yaml composes with the new keys."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W
from tests import dps_ref as R
from tests import impute_ref as I
from tests import likelihood_ref as L
from tests import ode_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_sampler_run_impute_dps", "fd_impute_guidance"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    assert callable(DiffusionSampler.impute_guidance)


@pytest.mark.parametrize("T", [7, 8, 24])
def test_idft_adjoint_is_the_transpose_of_idft(T):
    rs = np.random.RandomState(T)
    a, b = rs.randn(2, T, 3), rs.randn(2, T, 3)
    np.testing.assert_allclose((O.idft(a) * b).sum(), (a * R.idft_adjoint(b)).sum(), rtol=1e-12)
    F = L.dft_matrix(T)
    np.testing.assert_allclose(F @ F.T, np.diag(1.0 / R.inv_rho(T)), atol=1e-12)


def _case(T, C, B, kind, fourier, standardize, per_series, seed):
    rs = np.random.RandomState(seed)
    p = (0.1, 20.0) if kind == "vp" else (0.01, 2.0)
    sde = O.SDEParams(kind, p[0], p[1], O.noise_scaling(T, True))
    mu = 0.3 * rs.randn(T, C) if standardize else np.zeros((T, C))
    sigma = rs.uniform(0.3, 2.0, (T, C)) if standardize else np.ones((T, C))
    y = np.sin(np.linspace(0, 4, T))[None, :, None] + 0.3 * rs.randn(B, T, C)
    m = rs.rand(B, T, C) < 0.5 if per_series else rs.rand(T, C) < 0.5
    x0 = I.x0_obs(y, m, mu, sigma, fourier)
    return sde, sigma, x0, m, rs.randn(B, T, C)


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("per_series", [True, False])
def test_guidance_is_minus_the_gradient_gaussian_score(kind, fourier, standardize, per_series):
    T, C, B = 10, 2, 3
    sde, sigma, x0, m, x = _case(T, C, B, kind, fourier, standardize, per_series, 5)
    score_fn = L.gaussian_score(sde, 0.8)
    teeth = 0.0
    for t in (0.9, 0.3, 0.05):
        g, rn2, _ = R.guidance(score_fn, sde, x, t, x0, m, sigma, fourier, rel=1e-2)      # (the score is linear in x)
        # ||r||^2 is quadratic in x under this score: central differences are exact but for rounding, at any step
        ref = -R.grad_fd(lambda z: R.rnorm2(score_fn, sde, z, t, x0, m, sigma, fourier), x, rel=1e-2)
        scale = np.abs(ref).max()
        assert np.abs(g - ref).max() <= 1e-8 * scale, (t, np.abs(g - ref).max() / scale)
        np.testing.assert_allclose(rn2, R.rnorm2(score_fn, sde, x, t, x0, m, sigma, fourier), rtol=1e-12)
        g0, _, _ = R.guidance(score_fn, sde, x, t, x0, m, sigma, fourier, jacobian=False)
        teeth = max(teeth, np.abs(g0 - ref).max() / scale)
    assert teeth > 0.1      # the Jacobian-free form misses a term that is not small at some t: the check above has teeth


def test_guidance_is_minus_the_gradient_oracle_network():
    cfg = dict(T=8, C=3, D=8, L=2, H=4)
    sd = W.make_state_dict(cfg["C"], cfg["T"], cfg["D"], cfg["L"], seed=1234)
    score_fn = ode_ref.model_score(sd, "transformer", cfg["H"])
    sde, sigma, x0, m, x = _case(cfg["T"], cfg["C"], 2, "vp", True, True, True, 9)
    t = 0.4
    g, _, _ = R.guidance(score_fn, sde, x, t, x0, m, sigma, True)
    ref = -R.grad_fd(lambda z: R.rnorm2(score_fn, sde, z, t, x0, m, sigma, True), x, rel=1e-7)
    assert np.abs(g - ref).max() <= 1e-5 * np.abs(ref).max()


def test_zero_scale_trajectory_is_the_sampler():
    T, C, B, N = 12, 2, 2, 6
    sde, sigma, x0, m, _ = _case(T, C, B, "vp", True, True, True, 3)
    score_fn = L.gaussian_score(sde, 1.0)
    rs = np.random.RandomState(1)
    zp, zs = rs.randn(B, T, C), list(rs.randn(N, B, T, C))
    X = R.trajectory(score_fn, sde, zp, zs, x0, m, sigma, True, 0.0, jacobian=False)
    ts, dt = O.timesteps(N)
    Y = O.prior_sampling(sde, zp)
    for i, t in enumerate(ts):
        Y = O.sde_step(sde, score_fn(Y, float(t)), float(t), Y, zs[i], float(dt))
    np.testing.assert_allclose(X, Y, rtol=0, atol=0)


def test_guidance_pulls_toward_the_observations():
    """A small step along g lowers ||r||^2 (first-order descent), with and without Fourier."""
    for fourier in (True, False):
        sde, sigma, x0, m, x = _case(16, 3, 4, "vp", fourier, True, True, 11)
        score_fn = L.gaussian_score(sde, 0.8)
        t = 0.2
        g, rn2, _ = R.guidance(score_fn, sde, x, t, x0, m, sigma, fourier)
        step = 1e-3 / np.abs(g).max()
        assert (R.rnorm2(score_fn, sde, x + step * g, t, x0, m, sigma, fourier) < rn2).all()


def _sampler(T=20, C=3, corrector_steps=0):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler()
    sch.set_noise_scaling(T)
    m = ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=8, num_layers=1, n_head=4)
    return DiffusionSampler(score_model=m, sample_batch_size=4, corrector_steps=corrector_steps)


@pytest.mark.parametrize("bad", ["conditioning", "scale_nan", "scale_inf", "scale_neg", "scale_bool", "scale_str", "jacobian",
                                 "obs_noise", "corrector"])
def test_impute_dps_rejects_bad_arguments(bad):
    """Every check runs before anything touches a device (this machine may have none)."""
    s = _sampler(corrector_steps=1 if bad == "corrector" else 0)
    obs, mask = torch.zeros(2, 20, 3), torch.ones(2, 20, 3, dtype=torch.bool)
    kw = dict(conditioning="dps")
    kw.update({"conditioning": dict(conditioning="project"), "scale_nan": dict(guidance_scale=float("nan")),
               "scale_inf": dict(guidance_scale=float("inf")), "scale_neg": dict(guidance_scale=-0.5),
               "scale_bool": dict(guidance_scale=True), "scale_str": dict(guidance_scale="1"),
               "jacobian": dict(guidance_jacobian=1), "obs_noise": dict(obs_noise=[torch.zeros(5, 2, 20, 3)]),
               "corrector": {}}[bad])
    with pytest.raises(ValueError):
        s.impute(obs, mask, 5, fourier_transform=True, **kw)


@pytest.mark.parametrize("bad", ["shape", "x0_shape", "timestep", "timestep_zero", "mask", "std"])
def test_impute_guidance_rejects_bad_arguments(bad):
    s = _sampler()
    X, x0, mask = torch.zeros(2, 20, 3), torch.zeros(2, 20, 3), torch.ones(20, 3, dtype=torch.bool)
    kw, t = {}, 0.5
    if bad == "shape":
        X, x0 = torch.zeros(2, 21, 3), torch.zeros(2, 21, 3)
    elif bad == "x0_shape":
        x0 = torch.zeros(3, 20, 3)
    elif bad == "timestep":
        t = float("nan")
    elif bad == "timestep_zero":
        t = 0.0
    elif bad == "mask":
        mask = torch.ones(20, 3)
    elif bad == "std":
        kw = dict(feature_std=torch.ones(3, 20))
    with pytest.raises(ValueError):
        s.impute_guidance(X, x0, mask, t, fourier_transform=True, **kw)


def test_impute_config_composes_with_the_guidance_keys(tmp_path):
    from fourierdiffusion_amd.config import compose
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "impute", [], cwd=str(tmp_path))
    assert cfg.conditioning == "replace" and cfg.guidance.scale == 1.0 and cfg.guidance.jacobian is True
    cfg = compose(conf, "impute", ["conditioning=dps", "guidance.scale=0.3", "guidance.jacobian=false"], cwd=str(tmp_path))
    assert cfg.conditioning == "dps" and cfg.guidance.scale == 0.3 and cfg.guidance.jacobian is False
