"""GPU: ensemble imputation / forecasting (an extension, not in the reference) -- fd_ensemble_scores against the float64
restatement of tests/ensemble_ref.py, DiffusionSampler.impute(num_samples=K) (fd_sampler_run_impute_rep) against impute on
repeated observations, and cmd/impute.py num_samples_per_series=K end to end.

Tolerance of the scores kernel: it sums in double and rounds each output once to fp32, so it stays within a few fp32 ulps of
the float64 restatement on the same fp32 inputs.  The tests assert 1e-6 of the case's scale (max |sample|, |truth|, >= 1), which
is 8 ulps at that scale and far below the size of any indexing or sorting mistake."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import ensemble_ref as R
from tests.gpu_util import dev, host, make_model

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _scores_c(x, y, levels=R.LEVELS):
    from fourierdiffusion_amd import _C
    n, K, T, Cn = x.shape
    h = _C.ctx(x.device)
    lv = torch.tensor(levels, dtype=torch.float64, device=x.device)
    crps, mean = torch.full((n, T, Cn), 7.0, device=x.device), torch.full((n, T, Cn), 7.0, device=x.device)
    q = torch.full((len(levels), n, T, Cn), 7.0, device=x.device)
    rc = _C.lib().fd_ensemble_scores(h, x.data_ptr(), y.data_ptr(), n, K, T, Cn, lv.data_ptr(), len(levels), crps.data_ptr(),
                                     q.data_ptr(), mean.data_ptr(), _C.stream_of(x))
    _C.check(rc, h)
    return host(crps), host(q), host(mean)


@pytest.mark.parametrize("shape", [(3, 24, 40), (5, 100, 12), (2, 187, 1), (1, 1024, 16)])
@pytest.mark.parametrize("K", [1, 2, 3, 64, 100, 257, 1024])
def test_scores_kernel_vs_float64(K, shape):
    n, T, Cn = shape
    rs = np.random.RandomState(K * 7 + T)
    x = (rs.randn(n, K, T, Cn) * rs.uniform(0.2, 3.0, (1, 1, T, Cn)) + rs.randn(1, 1, T, Cn)).astype(np.float32)
    y = rs.randn(n, T, Cn).astype(np.float32)
    x[:, :, 0, 0] = np.round(x[:, :, 0, 0] * 2) / 2                   # ties on a coarse grid
    x[:, :, T // 2, :] = np.round(x[:, :, T // 2, :] * 4) / 4
    x[:, :, T - 1, Cn - 1] = 1.5                                        # a constant ensemble
    bad = np.zeros((n, T, Cn), bool)
    y[0, 1, 0] = np.nan                                                 # one NaN truth entry
    bad[0, 1, 0] = True
    if n > 1:
        x[1, K // 2, T // 3, 0] = np.nan                                # one NaN sample
        bad[1, T // 3, 0] = True
    crps, q, mean = _scores_c(dev(x), torch.from_numpy(y).cuda())
    rc, rq, rm = R.entry_scores(x, y)
    assert np.array_equal(np.isnan(rc), bad)
    # NaN exactly at those entries, in every output; every other entry finite
    for got in (crps, mean):
        assert np.array_equal(np.isnan(got), bad)
    assert np.array_equal(np.isnan(q), np.broadcast_to(bad, q.shape))
    scale = max(1.0, np.nanmax(np.abs(x)), np.nanmax(np.abs(y)))
    ok = ~bad
    for name, got, ref in (("crps", crps[ok], rc[ok]), ("mean", mean[ok], rm[ok]), ("quantiles", q[:, ok], rq[:, ok])):
        err = np.abs(got - ref).max() / scale
        assert err <= 1e-6, (name, err)
    assert (crps[ok] >= 0).all()
    const = (slice(None), T - 1, Cn - 1)                                 # the constant ensemble: exact quantiles, CRPS |1.5 - y|
    assert (q[(slice(None),) + const] == 1.5).all() and (mean[const] == 1.5).all()
    np.testing.assert_allclose(crps[const], np.abs(1.5 - y[const].astype(np.float64)), rtol=0, atol=1e-6 * scale)
    if K == 1:
        np.testing.assert_allclose(crps[ok], np.abs(x[:, 0].astype(np.float64) - y)[ok], rtol=0, atol=1e-6 * scale)


def _problem(cfg, n, per_series, seed=5):
    rs = np.random.RandomState(seed)
    T, Cn = cfg["T"], cfg["C"]
    mu, sigma = 0.3 * rs.randn(T, Cn), rs.uniform(0.5, 2.0, (T, Cn))
    y = np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(n, T, Cn)
    if per_series:
        m = rs.rand(n, T, Cn) < 0.5
        m[: n // 2, -T // 4:] = False
    else:
        m = np.ones((T, Cn), bool)
        m[-T // 4:] = False
    yn = np.where(m if per_series else m[None], y, np.nan)
    return (torch.from_numpy(yn).float(), torch.from_numpy(m), torch.from_numpy(mu).float(), torch.from_numpy(sigma).float(), y)


def _repeat(obs, mask, K, per_series):
    return obs.repeat_interleave(K, 0), (mask.repeat_interleave(K, 0) if per_series else mask)


@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("per_series", [True, False])
def test_replicated_equals_repeated_injected_f32(per_series, fourier):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(T=24, C=4, D=24, L=2, H=4)
    n, K, N = 3, 4, 8
    m_, _, _ = make_model(cfg, precision="fp32")
    obs, mask, mean, std, _ = _problem(cfg, n, per_series)
    rows = n * K
    rs = np.random.RandomState(1)
    zp = dev(rs.randn(rows, cfg["T"], cfg["C"]))
    zs, zo = dev(rs.randn(N, rows, cfg["T"], cfg["C"])), dev(rs.randn(N, rows, cfg["T"], cfg["C"]))
    s = DiffusionSampler(score_model=m_, sample_batch_size=rows)
    kw = dict(fourier_transform=fourier, feature_mean=mean, feature_std=std, prior_noise=[zp], step_noise=[zs], obs_noise=[zo])
    Xr = s.impute(obs, mask, N, num_samples=K, **kw)
    assert Xr.shape == (n, K, cfg["T"], cfg["C"])
    Xp = s.impute(*_repeat(obs, mask, K, per_series), N, **kw)
    assert torch.isfinite(Xr).all()
    assert torch.equal(Xr.reshape(rows, cfg["T"], cfg["C"]), Xp)


def test_replicated_equals_repeated_philox_and_replicas_differ():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.utils.fourier import destandardize_idft
    cfg = dict(T=40, C=5, D=24, L=2, H=4)
    n, K, N = 4, 6, 12
    m_, _, _ = make_model(cfg, precision="fp32")
    obs, mask, mean, std, y = _problem(cfg, n, True, seed=9)
    s = DiffusionSampler(score_model=m_, sample_batch_size=2 * K)          # two launches of two series each
    kw = dict(fourier_transform=True, feature_mean=mean, feature_std=std)
    torch.manual_seed(17)
    Xr = s.impute(obs, mask, N, num_samples=K, **kw)
    torch.manual_seed(17)
    Xp = s.impute(*_repeat(obs, mask, K, True), N, **kw)
    assert torch.equal(Xr.reshape(n * K, cfg["T"], cfg["C"]), Xp)
    A = host(destandardize_idft(Xr.reshape(n * K, cfg["T"], cfg["C"]).cuda(), mean.cuda(), std.cuda())).reshape(Xr.shape)
    m = mask.numpy()
    for i in range(n):
        hid = ~m[i]
        for k in range(1, K):                                               # replicas differ on the hidden entries
            assert np.abs(A[i, k][hid] - A[i, 0][hid]).mean() > 1e-3
        scale = max(1.0, np.abs(A[i]).max(), np.abs(y[i]).max())
        err = np.abs(A[i][:, m[i]] - y[i][m[i]][None]).max() / scale      # every replica reproduces the observations
        assert err <= 1e-4, (i, err)


def test_bf16_ecg_replicated_equals_repeated():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(T=100, C=12, D=72, L=10, H=12)
    n, K, N = 16, 8, 10
    m_, _, _ = make_model(cfg, precision="bf16")
    obs, mask, mean, std, _ = _problem(cfg, n, True, seed=3)
    s = DiffusionSampler(score_model=m_, sample_batch_size=n * K)
    kw = dict(fourier_transform=True, feature_mean=mean, feature_std=std)
    torch.manual_seed(2)
    Xr = s.impute(obs, mask, N, num_samples=K, **kw)
    torch.manual_seed(2)
    Xp = s.impute(*_repeat(obs, mask, K, True), N, **kw)
    assert torch.isfinite(Xr).all()
    assert torch.equal(Xr.reshape(n * K, cfg["T"], cfg["C"]), Xp)


def test_one_sample_equals_default_call():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(T=24, C=4, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision="fp32")
    obs, mask, mean, std, _ = _problem(cfg, 5, False)
    s = DiffusionSampler(score_model=m_, sample_batch_size=4)
    kw = dict(fourier_transform=True, feature_mean=mean, feature_std=std)
    torch.manual_seed(4)
    X1 = s.impute(obs, mask, 6, num_samples=1, **kw)
    torch.manual_seed(4)
    X0 = s.impute(obs, mask, 6, **kw)
    assert X1.shape == (5, 1, 24, 4) and X0.shape == (5, 24, 4)
    assert torch.equal(X1[:, 0], X0)


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_ensemble_impute(tmp_path):
    from fourierdiffusion_amd.sampling.masks import observation_mask
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=ensrun"], tmp_path)
    run_dir = tmp_path / "lightning_logs" / "ensrun"
    base = [str(ROOT / "cmd" / "impute.py"), "model_id=ensrun", "num_diffusion_steps=10", "sampler.sample_batch_size=40",
            "mask.kind=forecast", "mask.horizon=6"]
    _run(base, tmp_path)
    res1 = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert set(res1) == {"mask_kind", "num_series", "hidden_fraction", "mse_hidden", "mae_hidden", "max_abs_err_observed"}
    assert torch.load(run_dir / "imputations.pt").shape == (96, 24, 4)
    _run(base + ["num_samples_per_series=4", "num_series=30"], tmp_path)
    X = torch.load(run_dir / "imputations.pt")
    assert X.shape == (30, 4, 24, 4) and torch.isfinite(X).all()
    res = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert "mse_hidden" not in res and "mae_hidden" not in res
    assert res["num_series"] == 30 and res["num_samples_per_series"] == 4 and res["mask_kind"] == "forecast"
    assert abs(res["hidden_fraction"] - 0.25) < 1e-12 and res["max_abs_err_observed"] <= 1e-3
    # the truth the CLI scored against: the synthetic test split of the saved training config, the same forecast mask
    from fourierdiffusion_amd.config import instantiate, load_yaml
    dm = instantiate(load_yaml(run_dir / "train_config.yaml").datamodule)
    dm.prepare_data()
    dm.setup()
    truth = dm.X_test.float()[:30].numpy()
    mask = observation_mask("forecast", truth.shape, horizon=6).numpy()
    ref = R.ensemble_metrics(X.numpy(), truth, mask)
    for k, v in ref.items():
        assert abs(res[k] - v) <= 1e-5 * max(1.0, abs(v)), (k, res[k], v)
