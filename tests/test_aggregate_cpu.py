"""CPU: conditioning on window means (impute(aggregate=w), an extension not in the reference) -- the float64 restatement of
tests/aggregate_ref.py has the algebra the kernels rely on (P P^+ = I, the projection's fixed points, w = 1 is the mask path,
g = -grad ||r||^2 by central differences through the closed-form Gaussian score), the masks helpers, every argument check runs
before any device work, cmd/conf/impute.yaml composes with the new key, and the four entry points are declared, bound and exported."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from tests import aggregate_ref as A
from tests import dps_ref as R
from tests import impute_ref as I
from tests import likelihood_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fd_impute_project_agg", "fd_sampler_run_impute_agg", "fd_impute_guidance_agg", "fd_sampler_run_impute_dps_agg")


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in SYMBOLS:
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


@pytest.mark.parametrize("T,w", [(20, 3), (20, 20), (37, 2), (16, 4), (9, 1)])
def test_operator_algebra(T, w):
    rs = np.random.RandomState(T + w)
    J = A.n_windows(T, w)
    r, v = rs.randn(2, J, 3), rs.randn(2, T, 3)
    np.testing.assert_allclose(A.P(A.P_pinv(r, w, T), w), r, atol=1e-14)                      # P P^+ = I
    np.testing.assert_allclose((A.P(v, w) * r).sum(), (v * A.P_T(r, w, T)).sum(), rtol=1e-12)  # P^T is the adjoint
    assert A.lengths(T, w).sum() == T and A.lengths(T, w)[-1] == T - (J - 1) * w


def _case(T, C, B, w, kind, fourier, standardize, per_series, seed):
    rs = np.random.RandomState(seed)
    p = (0.1, 20.0) if kind == "vp" else (0.01, 2.0)
    sde = O.SDEParams(kind, p[0], p[1], O.noise_scaling(T, True))
    mu = 0.3 * rs.randn(T, C) if standardize else np.zeros((T, C))
    sigma = rs.uniform(0.3, 2.0, (T, C)) if standardize else np.ones((T, C))
    J = A.n_windows(T, w)
    y = A.P(np.sin(np.linspace(0, 4, T))[None, :, None] + 0.3 * rs.randn(B, T, C), w)
    m = rs.rand(B, J, C) < 0.6 if per_series else rs.rand(J, C) < 0.6
    yn = np.where(np.broadcast_to(m, y.shape), y, np.nan)
    return sde, mu, sigma, yn, m, A.x0_obs(yn, m, mu, sigma, fourier, w), rs.randn(B, T, C)


@pytest.mark.parametrize("T,w", [(20, 3), (20, 20), (37, 2)])
@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("per_series", [True, False])
def test_projection_fixes_observed_windows_and_moves_windows_rigidly(T, w, fourier, per_series):
    sde, mu, sigma, yn, m, x0, x = _case(T, 3, 2, w, "vp", fourier, True, per_series, 5)
    z = np.random.RandomState(1).randn(*x.shape)
    alpha, s = 0.7, 0.4
    xn = A.project(x, x0, m, sigma, sde.G, alpha, s, z, fourier, w)
    x_obs = alpha * x0 + s * sde.G[None, :, None] * z
    mb = np.broadcast_to(m, yn.shape)
    Ax, Axn, Ao = (I.forward_map(v, mu, sigma, fourier) for v in (x, xn, x_obs))
    # P A(x') = where(m, P A(x_obs), P A(x))
    np.testing.assert_allclose(A.P(Axn, w), np.where(mb, A.P(Ao, w), A.P(Ax, w)), atol=1e-12)
    # A(x') - A(x) is constant within each window
    d = Axn - Ax
    np.testing.assert_allclose(d, A.P_pinv(A.P(d, w), w, T), atol=1e-12)
    # the hard projection reproduces y on the observed windows
    xh = A.project(x, x0, m, sigma, sde.G, 1.0, 0.0, 0.0 * z, fourier, w)
    np.testing.assert_allclose(A.P(I.forward_map(xh, mu, sigma, fourier), w)[mb], yn[mb], atol=1e-12)


@pytest.mark.parametrize("fourier", [True, False])
def test_window_one_is_the_mask_path(fourier):
    T = 12
    sde, mu, sigma, yn, m, x0, x = _case(T, 2, 3, 1, "vp", fourier, True, True, 7)
    np.testing.assert_allclose(x0, I.x0_obs(yn, m, mu, sigma, fourier), atol=1e-12)
    z = np.random.RandomState(2).randn(*x.shape)
    np.testing.assert_allclose(A.project(x, x0, m, sigma, sde.G, 0.6, 0.5, z, fourier, 1),
                               I.project(x, x0, m, sigma, sde.G, 0.6, 0.5, z, fourier), atol=1e-12)
    score_fn = L.gaussian_score(sde, 0.8)
    for jac in (True, False):
        g, rn2, _ = A.guidance(score_fn, sde, x, 0.3, x0, m, sigma, fourier, 1, jacobian=jac)
        gr, rr, _ = R.guidance(score_fn, sde, x, 0.3, x0, m, sigma, fourier, jacobian=jac)
        np.testing.assert_allclose(g, gr, atol=1e-12)
        np.testing.assert_allclose(rn2, rr, atol=1e-12)


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("T,w", [(10, 3), (10, 10), (9, 2)])
def test_guidance_is_minus_the_gradient_gaussian_score(kind, fourier, standardize, T, w):
    sde, mu, sigma, yn, m, x0, x = _case(T, 2, 3, w, kind, fourier, standardize, True, 5)
    score_fn = L.gaussian_score(sde, 0.8)
    for t in (0.9, 0.3, 0.05):
        g, rn2, _ = A.guidance(score_fn, sde, x, t, x0, m, sigma, fourier, w,
                               vjp_fn=lambda xx, tt, v: R.vjp(score_fn, xx, tt, v, rel=1e-2))      # (the score is linear in x)
        # ||r||^2 is quadratic in x under this score: central differences are exact but for rounding, at any step
        ref = -R.grad_fd(lambda q: A.rnorm2(score_fn, sde, q, t, x0, m, sigma, fourier, w), x, rel=1e-2)
        scale = np.abs(ref).max()
        assert np.abs(g - ref).max() <= 1e-8 * scale, (t, np.abs(g - ref).max() / scale)
        np.testing.assert_allclose(rn2, A.rnorm2(score_fn, sde, x, t, x0, m, sigma, fourier, w), rtol=1e-12)


def test_all_false_mask_is_the_plain_step():
    sde, mu, sigma, yn, m, x0, x = _case(12, 2, 2, 4, "vp", True, True, False, 3)
    none = np.zeros_like(m)
    z = np.random.RandomState(4).randn(*x.shape)
    np.testing.assert_array_equal(A.project(x, x0, none, sigma, sde.G, 0.7, 0.4, z, True, 4), x)
    g, rn2, _ = A.guidance(L.gaussian_score(sde, 0.8), sde, x, 0.5, x0, none, sigma, True, 4, jacobian=False)
    assert (rn2 == 0).all() and (g == 0).all()


# ---------------------------------------------------------------- masks helpers
def test_window_means_and_lift():
    from fourierdiffusion_amd.sampling.masks import lift_windows, window_means
    rs = np.random.RandomState(0)
    X = rs.randn(3, 20, 2)
    for w in (1, 3, 7, 20):
        Y = window_means(torch.from_numpy(X), w)
        assert Y.shape == (3, A.n_windows(20, w), 2)
        np.testing.assert_allclose(Y.numpy(), A.P(X, w), atol=1e-14)
        Z = lift_windows(Y, w, 20)
        assert Z.shape == (3, 20, 2)
        np.testing.assert_allclose(Z.numpy(), A.P_pinv(Y.numpy(), w, 20), atol=0)
        np.testing.assert_allclose(window_means(Z, w).numpy(), Y.numpy(), atol=1e-14)
    m = torch.tensor([[True], [False], [True]])
    assert lift_windows(m, 2, 5).squeeze(-1).tolist() == [True, True, False, False, True]
    assert window_means(torch.arange(5.0).view(5, 1), 2).squeeze(-1).tolist() == [0.5, 2.5, 4.0]
    for bad in (dict(w=0), dict(w=21), dict(w=True), dict(w=2.0)):
        with pytest.raises(ValueError):
            window_means(torch.from_numpy(X), bad["w"])
    with pytest.raises(ValueError):
        window_means(torch.zeros(20, dtype=torch.int64).view(20, 1), 2)
    for w, T in ((0, 20), (3, 0), (21, 20), (True, 20)):
        with pytest.raises(ValueError):
            lift_windows(torch.zeros(7, 2), w, T)
    with pytest.raises(ValueError):
        lift_windows(torch.zeros(6, 2), 3, 20)


# ---------------------------------------------------------------- argument checks, before any device work
def _sampler(T=20, C=3, n_classes=0):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler()
    sch.set_noise_scaling(T)
    kw = dict(n_classes=n_classes) if n_classes else {}
    m = ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=8, num_layers=1, n_head=4, **kw)
    return DiffusionSampler(score_model=m, sample_batch_size=4)


@pytest.mark.parametrize("bad", ["zero", "negative", "bool", "float", "str", "too_long", "resample", "obs_fine", "obs_J", "mask_fine",
                                 "mask_J", "mask_dtype"])
@pytest.mark.parametrize("conditioning", ["replace", "dps"])
def test_impute_rejects_bad_aggregate_arguments(bad, conditioning):
    """Every check runs before anything touches a device (this machine may have none).  T = 20, w = 3: J = 7."""
    s = _sampler()
    obs, mask = torch.zeros(2, 7, 3), torch.ones(2, 7, 3, dtype=torch.bool)
    kw = dict(aggregate=3, conditioning=conditioning)
    if bad in ("zero", "negative", "bool", "float", "str", "too_long"):
        kw["aggregate"] = dict(zero=0, negative=-2, bool=True, float=3.0, str="3", too_long=21)[bad]
    elif bad == "resample":
        kw.update(resample=2)
    elif bad == "obs_fine":
        obs = torch.zeros(2, 20, 3)
    elif bad == "obs_J":
        obs = torch.zeros(2, 6, 3)
    elif bad == "mask_fine":
        mask = torch.ones(2, 20, 3, dtype=torch.bool)
    elif bad == "mask_J":
        mask = torch.ones(6, 3, dtype=torch.bool)
    elif bad == "mask_dtype":
        mask = torch.ones(7, 3)
    with pytest.raises(ValueError):
        s.impute(obs, mask, 5, fourier_transform=True, **kw)


@pytest.mark.parametrize("conditioning", ["replace", "dps"])
@pytest.mark.parametrize("guide", [dict(y=1), dict(cfg_scale=2.0), dict(y=0, cfg_scale=1.5)])
def test_impute_rejects_aggregate_with_labels_or_cfg(conditioning, guide):
    obs, mask = torch.zeros(2, 7, 3), torch.ones(7, 3, dtype=torch.bool)
    for n_classes in (0, 3):
        with pytest.raises(ValueError):
            _sampler(n_classes=n_classes).impute(obs, mask, 5, fourier_transform=True, aggregate=3, conditioning=conditioning, **guide)
    X = torch.zeros(2, 20, 3)
    with pytest.raises(ValueError, match="aggregate"):
        _sampler(n_classes=3).impute_guidance(X, X, mask, 0.5, fourier_transform=True, aggregate=3, **guide)


@pytest.mark.parametrize("bad", [0, -1, True, 2.0, 21])
def test_step_wise_twins_reject_bad_aggregate(bad):
    s = _sampler()
    X, mask = torch.zeros(2, 20, 3), torch.ones(7, 3, dtype=torch.bool)
    with pytest.raises(ValueError):
        s.impute_project(X, X, mask, 0.5, fourier_transform=True, aggregate=bad)
    with pytest.raises(ValueError):
        s.impute_guidance(X, X, mask, 0.5, fourier_transform=True, aggregate=bad)
    with pytest.raises(ValueError):
        s.observed_to_sample_space(torch.zeros(2, 7, 3), mask, fourier_transform=True, aggregate=bad)


def test_step_wise_twins_reject_wrong_window_shapes():
    s = _sampler()
    X = torch.zeros(2, 20, 3)
    with pytest.raises(ValueError):
        s.impute_guidance(X, X, torch.ones(20, 3, dtype=torch.bool), 0.5, fourier_transform=True, aggregate=3)
    with pytest.raises(ValueError):
        s.observed_to_sample_space(torch.zeros(2, 20, 3), torch.ones(7, 3, dtype=torch.bool), fourier_transform=True, aggregate=3)
    with pytest.raises(ValueError):
        s.impute_project(X, X, torch.ones(7, 3, dtype=torch.bool), 0.5, fourier_transform=True, aggregate=3, renoise_to=0.8)


def test_impute_config_composes_with_the_aggregate_key(tmp_path):
    from fourierdiffusion_amd.config import compose
    conf = os.path.join(ROOT, "cmd", "conf")
    assert compose(conf, "impute", [], cwd=str(tmp_path)).aggregate == 1
    cfg = compose(conf, "impute", ["aggregate=4", "mask.kind=forecast", "mask.horizon=2"], cwd=str(tmp_path))
    assert cfg.aggregate == 4 and cfg.mask.kind == "forecast" and cfg.mask.horizon == 2
