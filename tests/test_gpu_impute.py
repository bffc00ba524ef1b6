"""GPU: conditional sampling (DiffusionSampler.impute / fd_sampler_run_impute / fd_impute_project, an extension not in the
reference) against the float64 restatement of tests/impute_ref.py."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from oracle import fdiff_oracle as O
from oracle import weights as W
from oracle.make_golden import CFG_DEFAULT, CFG_TINY
from tests import impute_ref as R
from tests.gpu_util import dev, host, make_model, oracle_sde, report_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _project_c(x, x0, m_u8, per_series, std, fourier, G, alpha, s, z, seed=0, offset=0):
    from fourierdiffusion_amd import _C
    B, T, Cn = x.shape
    out = torch.empty_like(x)
    h = _C.ctx(x.device)
    rc = _C.lib().fd_impute_project(h, x.data_ptr(), x0.data_ptr(), m_u8.data_ptr(), int(per_series), _C.ptr(std), int(fourier),
                                    G.data_ptr(), float(alpha), float(s), _C.ptr(z), seed, offset, out.data_ptr(), B, T, Cn,
                                    _C.stream_of(x))
    _C.check(rc, h)
    return out


def test_project_vs_float64():
    alpha, s, B = 0.7, 0.4, 3
    worst = 0.0
    for T in (24, 100, 187, 252, 1024):
        for Cn in (1, 5, 12, 16, 20):
            rs = np.random.RandomState(T * 100 + Cn)
            x, z, x0 = rs.randn(B, T, Cn), rs.randn(B, T, Cn), rs.randn(B, T, Cn)
            sig = rs.uniform(0.5, 2.0, (T, Cn))
            masks = {True: rs.rand(B, T, Cn) < 0.5, False: rs.rand(T, Cn) < 0.5}
            for fourier in (True, False):
                for standardize in (True, False):
                    for scaling in (True, False):
                        for per_series, m in masks.items():
                            G = O.noise_scaling(T, scaling).astype(np.float64)
                            sigma = sig if standardize else np.ones((T, Cn))
                            ref = R.project(x, x0, m, sigma, G, alpha, s, z, fourier)
                            got = host(_project_c(dev(x), dev(x0), torch.from_numpy(m.astype(np.uint8)).cuda(), per_series,
                                                  dev(sigma) if standardize else None, fourier, dev(G), alpha, s, dev(z)))
                            err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
                            worst = max(worst, err)
                            assert err <= 1e-5, (T, Cn, fourier, standardize, scaling, per_series, err)
    print(f"fd_impute_project: worst max err / scale = {worst:.3e}")


def test_project_philox_equals_injected():
    """z = NULL draws element e at counter offset + e/4 under `seed`: fd_prior_sample (VP, G = 1) has the same layout."""
    from fourierdiffusion_amd import _C
    B, T, Cn, seed, offset = 5, 100, 12, 1234567, 4096
    rs = np.random.RandomState(7)
    x, x0, sig = dev(rs.randn(B, T, Cn)), dev(rs.randn(B, T, Cn)), dev(rs.uniform(0.5, 2.0, (T, Cn)))
    m = torch.from_numpy((rs.rand(B, T, Cn) < 0.5).astype(np.uint8)).cuda()
    G = dev(O.noise_scaling(T, True))
    z = torch.empty_like(x)
    h = _C.ctx(x.device)
    p = _C.SdeParams(0, 0.1, 20.0)
    _C.check(_C.lib().fd_prior_sample(h, C.byref(p), dev(np.ones(T)).data_ptr(), None, seed, offset, z.data_ptr(), B, T, Cn,
                                      _C.stream_of(x)), h)
    a = _project_c(x, x0, m, True, sig, True, G, 0.6, 0.5, None, seed, offset)
    b = _project_c(x, x0, m, True, sig, True, G, 0.6, 0.5, z)
    assert torch.equal(a, b)


def _inputs(cfg, mask_kind, seed):
    rs = np.random.RandomState(seed)
    T, Cn = cfg["T"], cfg["C"]
    mu, sigma = 0.3 * rs.randn(T, Cn), rs.uniform(0.5, 2.0, (T, Cn))
    y = np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(4, T, Cn)
    if mask_kind == "random":
        m = rs.rand(*y.shape) < 0.5
    else:
        m = np.ones(y.shape, bool)
        m[:, -T // 4:] = False
    return mu, sigma, y, m


@pytest.mark.parametrize("name", ["tiny", "default"])
@pytest.mark.parametrize("kind,p", [("vp", (0.1, 20.0)), ("ve", (0.01, 2.0))])
@pytest.mark.parametrize("mask_kind", ["random", "forecast"])
def test_trajectory_f32_vs_float64(name, kind, p, mask_kind):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = {"tiny": CFG_TINY, "default": dict(CFG_DEFAULT, L=2)}[name]
    N, T, Cn = 20, cfg["T"], cfg["C"]
    mu, sigma, y, m = _inputs(cfg, mask_kind, 11)
    B = y.shape[0]
    yn = np.where(m, y, np.nan)
    m_, sch, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    shape = (B, T, Cn)
    zp = W.randn(f"imp_p_{name}", shape, 1)
    zs = np.stack([W.randn(f"imp_z{i}_{name}", shape, 1) for i in range(N)])
    zo = np.stack([W.randn(f"imp_o{i}_{name}", shape, 1) for i in range(N)])
    sampler = DiffusionSampler(score_model=m_, sample_batch_size=B)
    X = sampler.impute(torch.from_numpy(yn).float(), torch.from_numpy(m), N, fourier_transform=True,
                       feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
                       prior_noise=[dev(zp)], step_noise=[dev(zs)], obs_noise=[dev(zo)]).numpy()
    mu32, sig32 = mu.astype(np.float32).astype(np.float64), sigma.astype(np.float32).astype(np.float64)
    x0 = R.x0_obs(yn.astype(np.float32), m, mu32, sig32, True)
    ref = R.impute_trajectory(sd, oracle_sde(kind, p, True, T), zp, list(zs), list(zo), x0, m, sig32, True, cfg["H"])
    err, _ = report_err(f"impute f32 {name} {kind} {p[1]} {mask_kind}", X, ref)
    assert err <= 1e-4, err
    Ax = R.forward_map(X, mu32, sig32, True)
    assert np.abs(Ax[m] - yn.astype(np.float32)[m]).max() <= 1e-4 * max(1.0, np.abs(y).max())


def test_zero_mask_equals_sample():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(T=40, C=5, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision="fp32")
    n = 8
    sampler = DiffusionSampler(score_model=m_, sample_batch_size=n, merge_batches=False)
    torch.manual_seed(3)
    Xs = sampler.sample(num_samples=n, num_diffusion_steps=15)
    torch.manual_seed(3)
    rs = np.random.RandomState(0)
    Xi = sampler.impute(torch.from_numpy(rs.randn(n, 40, 5)).float(), torch.zeros(40, 5, dtype=torch.bool), 15,
                        fourier_transform=True, feature_mean=torch.zeros(40, 5), feature_std=torch.from_numpy(rs.uniform(0.5, 2, (40, 5))).float())
    assert torch.isfinite(Xs).all()
    assert ((Xi - Xs).abs().max() / Xs.abs().max()).item() <= 1e-6


def _bf16_case(cfg, B, N):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.utils.fourier import destandardize_idft
    T, Cn = cfg["T"], cfg["C"]
    m_, _, _ = make_model(cfg, precision="bf16")
    rs = np.random.RandomState(5)
    mu, sigma = 0.3 * rs.randn(T, Cn), rs.uniform(0.5, 2.0, (T, Cn))
    y = np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(B, T, Cn)
    m = rs.rand(B, T, Cn) < 0.5
    m[: B // 2, -T // 5:] = False                       # half the batch forecasts its last fifth
    yn = torch.from_numpy(np.where(m, y, np.nan)).float()
    mean, std = torch.from_numpy(mu).float(), torch.from_numpy(sigma).float()
    sampler = DiffusionSampler(score_model=m_, sample_batch_size=B)
    torch.manual_seed(0)
    X = sampler.impute(yn, torch.from_numpy(m), N, fourier_transform=True, feature_mean=mean, feature_std=std)
    assert torch.isfinite(X).all()                      # NaN at unobserved entries did not leak
    Ax = host(destandardize_idft(X.cuda(), mean.cuda(), std.cuda()))
    mt = torch.from_numpy(m).numpy()
    # the hard projection's residue is f32 transform rounding at the magnitude of the state it transforms: scale = max |A(x)|
    scale = max(1.0, np.abs(Ax).max(), np.abs(y).max())
    err = np.abs(Ax[mt] - yn.numpy()[mt]).max() / scale
    print(f"bf16 impute T={T} C={Cn} B={B}: observed entries reproduced to {err:.3e} of scale {scale:.3e}")
    assert err <= 1e-4


def test_bf16_ecg_shape():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _bf16_case(dict(T=100, C=12, D=72, L=10, H=12), 2 * cus, 10)


def test_bf16_long_horizon():
    _bf16_case(dict(T=1024, C=16, D=72, L=10, H=12), 64, 10)


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_impute(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=imprun"], tmp_path)
    _run([str(ROOT / "cmd" / "impute.py"), "model_id=imprun", "num_diffusion_steps=10", "sampler.sample_batch_size=40",
          "mask.kind=forecast", "mask.horizon=6"], tmp_path)
    run_dir = tmp_path / "lightning_logs" / "imprun"
    X = torch.load(run_dir / "imputations.pt")
    assert X.shape == (96, 24, 4) and torch.isfinite(X).all()           # the synthetic test split: num_samples series
    res = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert res["num_series"] == 96 and res["mask_kind"] == "forecast" and abs(res["hidden_fraction"] - 0.25) < 1e-12
    for k in ("mse_hidden", "mae_hidden"):
        assert np.isfinite(res[k]) and res[k] >= 0.0, k
    assert res["max_abs_err_observed"] <= 1e-3
