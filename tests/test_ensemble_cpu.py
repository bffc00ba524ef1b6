"""CPU: ensemble imputation / forecasting scores (an extension, not in the reference) -- the float64 restatement of
tests/ensemble_ref.py has the properties the kernel relies on, forecast.aggregate matches it, and the new entry points, the
impute(num_samples=...) argument checks and cmd/conf/impute.yaml's new keys exist."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import ensemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_sampler_run_impute_rep", "fd_ensemble_scores"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


@pytest.mark.parametrize("K", [1, 2, 3, 7, 64, 101])
def test_sorted_crps_equals_pairwise(K):
    rs = np.random.RandomState(K)
    x = rs.randn(50, K)
    x[:10] = np.round(x[:10] * 2) / 2                     # ties
    x[10:15] = 0.25                                       # constant ensembles
    y = rs.randn(50)
    np.testing.assert_allclose(R.crps_sorted(x, y), R.crps_pairwise(x, y), rtol=1e-12, atol=1e-12)
    assert (R.crps_sorted(x, y) >= -1e-12).all()


def test_single_member_crps_is_absolute_error():
    rs = np.random.RandomState(0)
    x, y = rs.randn(40, 1), rs.randn(40)
    np.testing.assert_allclose(R.crps_sorted(x, y), np.abs(x[:, 0] - y), rtol=0, atol=1e-15)


@pytest.mark.parametrize("mu,sigma,y", [(0.0, 1.0, 0.0), (1.0, 2.0, -1.5), (-0.3, 0.5, 0.4)])
def test_gaussian_ensemble_approaches_closed_form(mu, sigma, y):
    """The estimator is biased by E|X - X'| / (2K) = sigma / (sqrt(pi) K); at K = 20000 the Monte Carlo error is ~1e-2 sigma."""
    x = mu + sigma * np.random.RandomState(1).randn(20000)
    got = float(R.crps_sorted(x[None], np.array([y]))[0])
    assert abs(got - R.crps_gaussian(mu, sigma, y)) <= 1.5e-2 * sigma


@pytest.mark.parametrize("K", [1, 2, 5, 100])
def test_quantiles_match_numpy(K):
    rs = np.random.RandomState(K)
    x = rs.randn(2, K, 3, 4)
    crps, q, mean = R.entry_scores(x, rs.randn(2, 3, 4))
    np.testing.assert_allclose(q, np.quantile(x, R.LEVELS, axis=1, method="linear"), rtol=0, atol=1e-14)
    np.testing.assert_allclose(q, torch.quantile(torch.from_numpy(x), torch.tensor(R.LEVELS, dtype=torch.float64), dim=1).numpy(),
                               rtol=0, atol=1e-12)
    np.testing.assert_allclose(mean, x.mean(1), atol=1e-14)


def test_nan_stays_in_its_entry():
    rs = np.random.RandomState(3)
    x, y = rs.randn(2, 8, 4, 3), rs.randn(2, 4, 3)
    x[0, 3, 1, 2] = np.nan
    y[1, 0, 0] = np.nan
    crps, q, mean = R.entry_scores(x, y)
    bad = np.zeros((2, 4, 3), bool)
    bad[0, 1, 2] = bad[1, 0, 0] = True
    assert np.isnan(crps[bad]).all() and np.isnan(mean[bad]).all() and np.isnan(q[:, bad]).all()
    assert np.isfinite(crps[~bad]).all() and np.isfinite(mean[~bad]).all() and np.isfinite(q[:, ~bad]).all()


def _mask(kind, shape, rs):
    n, T, C = shape
    if kind == "random":
        return rs.rand(n, T, C) >= 0.5
    m = np.ones(shape, bool)
    m[:, T - 5:] = False
    return m


@pytest.mark.parametrize("kind", ["random", "forecast"])
def test_aggregate_matches_restatement(kind):
    """forecast.aggregate (torch float64) against ensemble_ref.aggregate on random per-entry inputs, and forecast.channel_sums
    against the restatement's channel sums."""
    from fourierdiffusion_amd.sampling.forecast import DEFAULT_LEVELS, aggregate, channel_sums
    assert tuple(DEFAULT_LEVELS) == R.LEVELS and 0.5 in DEFAULT_LEVELS
    rs = np.random.RandomState(11)
    n, K, T, C = 6, 9, 20, 3
    m = _mask(kind, (n, T, C), rs)
    x, y = rs.randn(n, K, T, C), rs.randn(n, T, C) + 0.5
    crps, q, mean = R.entry_scores(x, y)
    xs_t, ys_t, sm_t = channel_sums(torch.from_numpy(x).float(), torch.from_numpy(y).float(), torch.from_numpy(m))
    H = ~m
    np.testing.assert_allclose(ys_t.numpy()[..., 0], np.where(H, y, 0).sum(-1), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(xs_t.numpy()[..., 0], np.where(H[:, None], x, 0).sum(-1), rtol=1e-6, atol=1e-6)
    assert np.array_equal(sm_t.numpy(), H.any(-1))
    ys = np.where(H, y, 0).sum(-1)
    _, qs, _ = R.entry_scores(np.where(H[:, None], x, 0).sum(-1, keepdims=True), ys[..., None])
    ref = R.aggregate(y, m, crps, q, mean, R.LEVELS, ys, qs[..., 0], H.any(-1))
    t = torch.from_numpy
    got = aggregate(t(y), t(m), t(crps), t(q), t(mean), DEFAULT_LEVELS, t(ys), t(qs[..., 0]), t(H.any(-1)))
    assert set(got) == set(ref) == {"crps", "crps_quantile", "crps_sum_quantile", "mae_median", "rmse_median", "mse_mean",
                                    "coverage_90", "width_90"}
    for k in ref:
        assert math.isfinite(got[k]) and abs(got[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (k, got[k], ref[k])
    # the whole protocol of the restatement reproduces its own pieces
    full = R.ensemble_metrics(x, y, m)
    for k in ref:
        assert abs(full[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), k


def test_aggregate_rejects_levels_without_the_interval():
    from fourierdiffusion_amd.sampling.forecast import aggregate
    z = torch.zeros(1, 2, 1)
    with pytest.raises(ValueError):
        aggregate(z, z.bool(), z, torch.zeros(2, 1, 2, 1), z, (0.25, 0.75), z[..., 0], torch.zeros(2, 1, 2), z[..., 0].bool())


def _sampler(T=20, C=3, corrector_steps=0):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler()
    sch.set_noise_scaling(T)
    m = ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=8, num_layers=1, n_head=4)
    return DiffusionSampler(score_model=m, sample_batch_size=4, corrector_steps=corrector_steps)


@pytest.mark.parametrize("bad", [0, -2, 2.0, "4", True, "corrector"])
def test_impute_rejects_bad_num_samples(bad):
    """Every check runs before anything touches a device (this machine may have none)."""
    s = _sampler(corrector_steps=1 if bad == "corrector" else 0)
    obs, mask = torch.zeros(2, 20, 3), torch.ones(2, 20, 3, dtype=torch.bool)
    with pytest.raises(ValueError):
        s.impute(obs, mask, 5, fourier_transform=True, num_samples=4 if bad == "corrector" else bad)


def test_impute_config_composes_with_the_new_keys(tmp_path):
    from fourierdiffusion_amd.config import compose
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "impute", [], cwd=str(tmp_path))
    assert cfg.num_samples_per_series == 1 and cfg.num_series is None
    cfg = compose(conf, "impute", ["num_samples_per_series=50", "num_series=16", "mask.kind=forecast"], cwd=str(tmp_path))
    assert cfg.num_samples_per_series == 50 and cfg.num_series == 16 and cfg.mask.kind == "forecast"
