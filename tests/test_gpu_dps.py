"""GPU: gradient-guided conditional sampling (DiffusionSampler.impute(conditioning="dps") / fd_sampler_run_impute_dps /
fd_impute_guidance, an extension not in the reference) against the float64 restatement of tests/dps_ref.py: one guidance
evaluation for the three backbones, trajectories with and without the network's Jacobian, the zero-scale Jacobian-free loop against
sample(), reproducibility, batch independence and replication, bf16 at the ecg shape, and the CLI end to end.  Measured errors are
logged by tests/gpu_util.report_err."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from oracle import weights as W
from oracle.make_golden import CFG_DEFAULT, CFG_TINY
from tests import dps_ref as R
from tests import impute_ref as I
from tests import likelihood_ref as L
from tests import ode_ref
from tests.gpu_util import dev, host, make_model, oracle_sde, report_err
from tests.test_gpu_likelihood import make_bb

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG_T8 = dict(T=8, C=3, D=8, L=2, H=4)


def _model(backbone, cfg, precision="fp32"):
    if backbone == "transformer":
        m, sch, sd = make_model(cfg, precision=precision)
        return m, sd, ode_ref.model_score(sd, "transformer", cfg["H"])
    m, sch, sd = make_bb(backbone, cfg)
    return m, sd, ode_ref.model_score(sd, backbone)


def _inputs(T, C, B, mask_kind, seed, fourier=True):
    """mu, sigma (f32-representable), observations y (NaN where hidden), mask, and x0_obs in float64."""
    rs = np.random.RandomState(seed)
    mu = (0.3 * rs.randn(T, C)).astype(np.float32).astype(np.float64)
    sigma = rs.uniform(0.5, 2.0, (T, C)).astype(np.float32).astype(np.float64)
    y = (np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(B, T, C)).astype(np.float32)
    if mask_kind == "random":
        m = rs.rand(B, T, C) < 0.5
    else:
        m = np.ones(y.shape, bool)
        m[:, -max(1, T // 4):] = False
    yn = np.where(m, y, np.nan).astype(np.float32)
    return mu, sigma, yn, m, I.x0_obs(yn, m, mu, sigma, fourier)


def _sampler(m, bs):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    return DiffusionSampler(score_model=m, sample_batch_size=bs)


# ---------------------------------------------------------------- one evaluation
@pytest.mark.parametrize("backbone", ["transformer", "mlp", "lstm"])
@pytest.mark.parametrize("fourier", [True, False])
def test_guidance_against_float64(backbone, fourier):
    cfg, B = CFG_T8, 2
    T, Cn = cfg["T"], cfg["C"]
    m, sd, score_fn = _model(backbone, cfg)
    osde = oracle_sde("vp", (0.1, 20.0), True, T)
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, "random", 3, fourier)
    s = _sampler(m, B)
    worst = 0.0
    for t in (0.7, 0.3, 0.05):
        x = W.randn(f"dpsg_x_{backbone}_{t}", (B, T, Cn), 0)
        t32 = float(np.float32(t))
        g, rn2 = s.impute_guidance(torch.from_numpy(x), dev(x0), torch.from_numpy(mk), t32, fourier_transform=fourier,
                                   feature_std=torch.from_numpy(sigma).float())
        gr, rr, _ = R.guidance(score_fn, osde, x, t32, x0, mk, sigma, fourier)
        err, _ = report_err(f"dps guidance fp32 {backbone} fourier={fourier} T=8 t={t}", host(g), gr)
        worst = max(worst, err)
        np.testing.assert_allclose(rn2.cpu().numpy(), rr, rtol=1e-5)
        assert err <= 1e-5, (t, err)
    print(f"dps guidance {backbone} fourier={fourier}: worst {worst:.3e} of max|g|")


@pytest.mark.parametrize("backbone,cfg", [("transformer", CFG_DEFAULT), ("mlp", dict(T=100, C=12, D=72, L=3)),
                                          ("lstm", dict(T=100, C=12, D=72, L=3))])
def test_guidance_directional_at_default_shape(backbone, cfg):
    """<v, g> = (2 / alpha) (<v, u> + <J v, s^2 G^2 u>), J v by one central difference of the oracle score."""
    B, T, Cn = 2, cfg["T"], cfg["C"]
    m, sd, score_fn = _model(backbone, cfg)
    osde = oracle_sde("vp", (0.1, 20.0), True, T)
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, "random", 4)
    x = W.randn(f"dpsd_x_{backbone}", (B, T, Cn), 0).astype(np.float64)
    v = W.randn(f"dpsd_v_{backbone}", (B, T, Cn), 1).astype(np.float64)
    t = float(np.float32(0.4))
    g, _ = _sampler(m, B).impute_guidance(torch.from_numpy(x).float(), dev(x0), torch.from_numpy(mk), t, fourier_transform=True,
                                          feature_std=torch.from_numpy(sigma).float())
    g = host(g)
    alpha, s = R.coef(osde, t)
    score = score_fn(x, t)
    _, u = R.residual(x, score, x0, mk, sigma, osde.G, alpha, s, True)
    w = (s * s) * (osde.G ** 2)[None, :, None] * u
    ref = (2.0 / alpha) * ((v * u).sum(axis=(1, 2)) + (L.jvp(score_fn, x, t, v) * w).sum(axis=(1, 2)))
    got = (g * v).sum(axis=(1, 2))
    scale = np.linalg.norm(g.reshape(B, -1), axis=1) * np.linalg.norm(v.reshape(B, -1), axis=1)
    err = float(np.abs(got - ref).max() / scale.max())
    print(f"dps guidance {backbone} directional: {err:.3e} of |g| |v|")
    assert err <= 1e-5


# ---------------------------------------------------------------- trajectories
def _trajectory(cfg, kind, p, mask_kind, jacobian, zeta, N=10, B=3, tag=""):
    T, Cn = cfg["T"], cfg["C"]
    m, sch, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, mask_kind, 11)
    shape = (B, T, Cn)
    zp = W.randn(f"dps_p_{tag}", shape, 1)
    zs = np.stack([W.randn(f"dps_z{i}_{tag}", shape, 1) for i in range(N)])
    X = _sampler(m, B).impute(torch.from_numpy(yn), torch.from_numpy(mk), N, fourier_transform=True,
                              feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
                              prior_noise=[dev(zp)], step_noise=[dev(zs)], conditioning="dps", guidance_scale=zeta,
                              guidance_jacobian=jacobian).numpy()
    ref = R.trajectory(ode_ref.model_score(sd, "transformer", cfg["H"]), oracle_sde(kind, p, True, T), zp, list(zs), x0, mk, sigma,
                       True, zeta, jacobian)
    assert np.isfinite(X).all()
    return report_err(f"dps trajectory f32 T={T} {kind} {mask_kind} jacobian={jacobian} zeta={zeta}", X, ref)[0]


@pytest.mark.parametrize("mask_kind", ["random", "forecast"])
@pytest.mark.parametrize("kind,p", [("vp", (0.1, 20.0)), ("ve", (0.01, 2.0))])
def test_trajectory_with_jacobian_vs_float64(kind, p, mask_kind):
    err = _trajectory(CFG_TINY, kind, p, mask_kind, True, 0.3, tag=f"j_{kind}_{mask_kind}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("mask_kind", ["random", "forecast"])
@pytest.mark.parametrize("name", ["tiny", "default"])
def test_trajectory_without_jacobian_vs_float64(name, mask_kind):
    cfg = {"tiny": CFG_TINY, "default": dict(CFG_DEFAULT, L=2)}[name]
    err = _trajectory(cfg, "vp", (0.1, 20.0), mask_kind, False, 0.3, tag=f"n_{name}_{mask_kind}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_zero_scale_without_jacobian_is_sample(precision, monkeypatch):
    """guidance_scale = 0, no Jacobian: the same score launch, fd_sde_apply and noise as sample()'s step-by-step loop, bit for bit."""
    monkeypatch.setenv("FDIFF_SAMPLER_STEPWISE", "1")
    cfg, B, N = dict(T=40, C=5, D=72, L=2, H=12), 6, 8
    m, _, _ = make_model(cfg, precision=precision)
    shape = (B, cfg["T"], cfg["C"])
    zp = dev(W.randn("dps0_p", shape, 1))
    zs = dev(np.stack([W.randn(f"dps0_z{i}", shape, 1) for i in range(N)]))
    s = _sampler(m, B)
    Xs = s.sample(num_samples=B, num_diffusion_steps=N, prior_noise=[zp], step_noise=[zs])
    mu, sigma, yn, mk, _ = _inputs(cfg["T"], cfg["C"], B, "random", 2)
    Xd = s.impute(torch.from_numpy(yn), torch.from_numpy(mk), N, fourier_transform=True, feature_mean=torch.from_numpy(mu).float(),
                  feature_std=torch.from_numpy(sigma).float(), prior_noise=[zp], step_noise=[zs], conditioning="dps",
                  guidance_scale=0.0, guidance_jacobian=False)
    assert torch.isfinite(Xs).all() and torch.equal(Xs.cpu(), Xd)
    # the same with the engine's Philox stream: one seed gives both calls the same prior, key and offset, so the step kernel's
    # counters (group q of step i at offset + i ceil(BTC/4) + q) must be the sampler's
    torch.manual_seed(17)
    Ps = s.sample(num_samples=B, num_diffusion_steps=N)
    torch.manual_seed(17)
    Pd = s.impute(torch.from_numpy(yn), torch.from_numpy(mk), N, fourier_transform=True, feature_mean=torch.from_numpy(mu).float(),
                  feature_std=torch.from_numpy(sigma).float(), conditioning="dps", guidance_scale=0.0, guidance_jacobian=False)
    assert torch.isfinite(Ps).all() and not torch.equal(Ps.cpu(), Xs.cpu()) and torch.equal(Ps.cpu(), Pd)


# ---------------------------------------------------------------- reproducibility, batch independence, replication
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_reproducible_batch_independent_and_replicated(precision):
    cfg, n, K, N = dict(T=40, C=5, D=72, L=2, H=12), 4, 3, 6
    T, Cn = cfg["T"], cfg["C"]
    m, _, _ = make_model(cfg, precision=precision)
    mu, sigma, yn, mk, _ = _inputs(T, Cn, n, "random", 7)
    kw = dict(fourier_transform=True, feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
              conditioning="dps", guidance_scale=0.5)
    obs, mask = torch.from_numpy(yn), torch.from_numpy(mk)
    s = _sampler(m, n * K)
    for jac in (True, False):
        torch.manual_seed(9)
        a = s.impute(obs, mask, N, guidance_jacobian=jac, **kw)
        torch.manual_seed(9)
        b = s.impute(obs, mask, N, guidance_jacobian=jac, **kw)
        assert torch.isfinite(a).all() and torch.equal(a, b), (precision, jac)
    # replicas read one observation in place: bit-identical to repeat_interleave'd observations under the same noise
    shape = (n * K, T, Cn)
    zp = dev(W.randn("dpsr_p", shape, 1))
    zs = dev(np.stack([W.randn(f"dpsr_z{i}", shape, 1) for i in range(N)]))
    rep = s.impute(obs, mask, N, num_samples=K, prior_noise=[zp], step_noise=[zs], **kw)
    big = s.impute(obs.repeat_interleave(K, 0), mask.repeat_interleave(K, 0), N, prior_noise=[zp], step_noise=[zs], **kw)
    assert rep.shape == (n, K, T, Cn) and torch.equal(rep.reshape(n * K, T, Cn), big)
    if precision != "fp32":
        return
    # one series alone against the same series inside the batch (its noise injected identically)
    one = _sampler(m, 1).impute(obs[2:3], mask[2:3], N, prior_noise=[zp[6:7]], step_noise=[zs[:, 6:7]], **kw)
    d = float((one[0] - big[6]).abs().max() / big[6].abs().max())
    print(f"dps batch independence fp32: {d:.3e} relative")
    assert torch.equal(one[0], big[6])


# ---------------------------------------------------------------- bf16 at the ecg shape
def test_bf16_ecg_shape():
    cfg, B, N = CFG_DEFAULT, 64, 10
    T, Cn = cfg["T"], cfg["C"]
    mb, _, _ = make_model(cfg, precision="bf16")
    mf, _, _ = make_model(cfg, precision="fp32")
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, "random", 5)
    obs, mask = torch.from_numpy(yn), torch.from_numpy(mk)
    kw = dict(fourier_transform=True, feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
              conditioning="dps", guidance_scale=1.0)
    for jac in (True, False):
        torch.manual_seed(1)
        X = _sampler(mb, B).impute(obs, mask, N, guidance_jacobian=jac, **kw)
        assert torch.isfinite(X).all(), jac
    x = torch.from_numpy(W.randn("dpsb_x", (8, T, Cn), 0))
    for t in (0.8, 0.4, 0.1):
        res = {}
        for prec, mm in (("bf16", mb), ("fp32", mf)):
            g, rn2 = _sampler(mm, 8).impute_guidance(x, dev(x0[:8]), mask[:8], t, fourier_transform=True,
                                                    feature_std=torch.from_numpy(sigma).float())
            assert torch.isfinite(g).all() and torch.isfinite(rn2).all()
            res[prec] = host(g).ravel()
        a, b = res["bf16"], res["fp32"]
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        print(f"bf16 dps guidance t={t}: cosine {cos:.6f} vs fp32")
        assert cos >= 0.998, (t, cos)


# ---------------------------------------------------------------- CLI
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_impute_dps(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=dpsrun"], tmp_path)
    run_dir = tmp_path / "lightning_logs" / "dpsrun"
    _run([str(ROOT / "cmd" / "impute.py"), "model_id=dpsrun", "num_diffusion_steps=10", "sampler.sample_batch_size=40",
          "mask.kind=forecast", "mask.horizon=6", "conditioning=dps", "guidance.scale=0.5", "num_samples_per_series=4",
          "num_series=20"], tmp_path)
    X = torch.load(run_dir / "imputations.pt")
    assert X.shape == (20, 4, 24, 4) and torch.isfinite(X).all()
    res = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert res["conditioning"] == "dps" and res["guidance_scale"] == 0.5 and res["guidance_jacobian"] is True
    assert res["num_series"] == 20 and res["num_samples_per_series"] == 4
    assert np.isfinite(res["crps"])
