"""GPU: log-likelihood through the probability-flow ODE (csrc/fd_likelihood.hip, an extension not in the reference) and the
input-only VJP under it (fd_score_input_vjp): the VJP against central differences of the oracle score for the three backbones,
bf16 against fp32, no effect on the gradient state; fd_prior_logp against the closed form; fd_likelihood_run against the float64
restatement driven by the oracle score (tests/likelihood_ref.py); latents against encode; the exact estimator; reproducibility and
batch independence; the CLI end to end.  Measured errors are logged by tests/gpu_util.report_err."""
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
from oracle.make_golden import CFG_DEFAULT
from tests import likelihood_ref as L
from tests import ode_ref as R
from tests.gpu_util import DEV, dev, host, make_model, oracle_sde, report_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG_T8 = dict(T=8, C=3, D=8, L=2, H=4)


def make_bb(kind, cfg, d_mlp=16, seed=4321):
    from fourierdiffusion_amd.models.score_models import LSTMScoreModule, MLPScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler(beta_min=0.1, beta_max=20.0, fourier_noise_scaling=True)
    sch.set_noise_scaling(cfg["T"])
    if kind == "mlp":
        m = MLPScoreModule(n_channels=cfg["C"], max_len=cfg["T"], noise_scheduler=sch, d_model=cfg["D"], d_mlp=d_mlp,
                           num_layers=cfg["L"])
    else:
        m = LSTMScoreModule(n_channels=cfg["C"], max_len=cfg["T"], noise_scheduler=sch, d_model=cfg["D"], num_layers=cfg["L"])
    sd = W.make_state_dict_backbone(kind, cfg["C"], cfg["T"], cfg["D"], cfg["L"], d_mlp=d_mlp, seed=seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.to(DEV)
    m.precision = m.train_precision = "fp32"
    return m, sch, sd


def _model(backbone, cfg, precision="fp32"):
    if backbone == "transformer":
        m, sch, sd = make_model(cfg, precision=precision)
        return m, sch, sd, R.model_score(sd, "transformer", cfg["H"])
    m, sch, sd = make_bb(backbone, cfg)
    return m, sch, sd, R.model_score(sd, backbone)


def _vjp(m, x, t, u):
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    m.train()
    m.dropout = 0.0
    out = m(DiffusableBatch(X=dev(x), timesteps=dev(t)))
    return host(out), host(m.input_vjp(dev(u)))


@pytest.mark.parametrize("backbone", ["transformer", "mlp", "lstm"])
def test_input_vjp_against_the_oracle_jacobian(backbone):
    cfg, B = CFG_T8, 2
    m, _, sd, _ = _model(backbone, cfg)
    x = W.randn(f"llv_x_{backbone}", (B, cfg["T"], cfg["C"]), 0)
    t = W.uniform(f"llv_t_{backbone}", (B,), 0, 0.05, 1.0)
    u = W.randn(f"llv_u_{backbone}", (B, cfg["T"], cfg["C"]), 1)
    _, dx = _vjp(m, x, t, u)
    if backbone == "transformer":
        fn = lambda z: O.score_forward(sd, z, t, cfg["H"])      # noqa: E731
    else:
        fn = lambda z: getattr(O, f"{backbone}_score_forward")(sd, z, t)      # noqa: E731
    d = 1e-7      # (float64; small enough that no relu pre-activation of the 2048-wide FFN crosses its kink)
    ref = np.zeros_like(dx)
    for k in range(cfg["T"] * cfg["C"]):           # column k of every series' Jacobian, (J^T u)_k = <u, J e_k>
        e = np.zeros((cfg["T"], cfg["C"]))
        e.flat[k] = 1.0
        col = (fn(x + d * e) - fn(x - d * e)) / (2 * d)
        ref.reshape(B, -1)[:, k] = (u * col).sum(axis=(1, 2))
    err, _ = report_err(f"input_vjp fp32 {backbone} T=8 vs oracle central differences", dx, ref)
    assert err <= 1e-5


@pytest.mark.parametrize("backbone,cfg", [("transformer", CFG_DEFAULT), ("mlp", dict(T=100, C=12, D=72, L=3)),
                                          ("lstm", dict(T=100, C=12, D=72, L=3))])
def test_input_vjp_directional_at_default_shape(backbone, cfg):
    B = 2
    m, _, sd, _ = _model(backbone, cfg)
    x = W.randn(f"lld_x_{backbone}", (B, cfg["T"], cfg["C"]), 0)
    t = W.uniform(f"lld_t_{backbone}", (B,), 0, 0.05, 1.0)
    u = W.randn(f"lld_u_{backbone}", (B, cfg["T"], cfg["C"]), 1)
    v = W.randn(f"lld_v_{backbone}", (B, cfg["T"], cfg["C"]), 2)
    _, dx = _vjp(m, x, t, u)
    got = (dx * v).sum(axis=(1, 2))
    if backbone == "transformer":
        sfn = lambda z: O.score_forward(sd, z, t, cfg["H"])      # noqa: E731
    else:
        sfn = lambda z: getattr(O, f"{backbone}_score_forward")(sd, z, t)      # noqa: E731
    d = 1e-7
    x64, v64 = x.astype(np.float64), v.astype(np.float64)      # (a float32 x + d v would round the step away)
    jv = (sfn(x64 + d * v64) - sfn(x64 - d * v64)) / (2 * d)
    ref = (u * jv).sum(axis=(1, 2))
    scale = np.linalg.norm(dx.reshape(B, -1), axis=1) * np.linalg.norm(v.reshape(B, -1), axis=1)
    err = float(np.abs(got - ref).max() / scale.max())
    report_err(f"input_vjp fp32 {backbone} T=100 <u, J v> (relative to |J^T u| |v|)", got, ref)
    print(f"input_vjp {backbone} directional: {err:.3e} of |J^T u| |v|")
    assert err <= 1e-5


@pytest.mark.parametrize("cfg,B", [(CFG_DEFAULT, 16), (dict(T=252, C=8, D=72, L=4, H=12), 8)])
def test_input_vjp_bf16_against_fp32(cfg, B):
    x = W.randn(f"llb_x_{cfg['T']}", (B, cfg["T"], cfg["C"]), 0)
    t = W.uniform(f"llb_t_{cfg['T']}", (B,), 0, 0.05, 1.0)
    u = W.randn(f"llb_u_{cfg['T']}", (B, cfg["T"], cfg["C"]), 1)
    res = {}
    for prec in ("fp32", "bf16"):
        m, _, _ = make_model(cfg, precision=prec)
        res[prec] = _vjp(m, x, t, u)[1]
        assert m.train_mode_effective == prec
    err, rms = report_err(f"input_vjp bf16 vs fp32 T={cfg['T']} C={cfg['C']} L={cfg['L']}", res["bf16"], res["fp32"])
    a, b = res["bf16"].ravel(), res["fp32"].ravel()
    cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    print(f"bf16 input_vjp T={cfg['T']}: cosine {cos:.6f} vs fp32")
    assert rms <= 5e-2 and cos >= 0.998


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_input_vjp_leaves_gradient_state_alone(precision):
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    from fourierdiffusion_amd.utils.losses import get_sde_loss_fn
    cfg, B = dict(T=40, C=5, D=72, L=2, H=12), 3
    m, sch, _ = make_model(cfg, precision=precision)
    m.dropout = 0.0
    X = W.randn("llg_x", (B, cfg["T"], cfg["C"]), 0)
    z = W.randn("llg_z", (B, cfg["T"], cfg["C"]), 1)
    tt = W.uniform("llg_t", (B,), 0, 0.05, 1.0)
    loss_fn = get_sde_loss_fn(sch, train=True, likelihood_weighting=False)

    def step():
        torch.manual_seed(5)
        m.train()
        m.zero_grad()
        loss = loss_fn(m, DiffusableBatch(X=dev(X), y=None, timesteps=dev(tt)), noise=dev(z))
        return float(loss.item()), m.grads.detach().clone()

    l1, g1 = step()
    m.zero_grad()
    pending, before = m._zero_pending, m._grads.detach().clone()
    m.train()
    m(DiffusableBatch(X=dev(X), timesteps=dev(tt)))
    dx = m.input_vjp(dev(z))
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()
    assert m._zero_pending == pending and torch.equal(m._grads, before)
    l2, g2 = step()
    assert l1 == l2 and torch.equal(g1, g2)


@pytest.mark.parametrize("kind,p", [("vp", (0.1, 20.0)), ("ve", (0.01, 50.0))])
def test_prior_logp_closed_form(kind, p):
    from fourierdiffusion_amd import _C
    T, Cn, B = 20, 3, 5
    _, sch, _ = make_model(dict(T=T, C=Cn, D=8, L=1, H=4), kind=kind, p=p)
    x = W.randn(f"llp_x_{kind}", (B, T, Cn), 0) * (p[1] if kind == "ve" else 1.0)
    xd = dev(x)
    out = torch.empty(B, device=DEV)
    ctx = _C.ctx(xd.device)
    prm = sch._c_params()
    _C.check(_C.lib().fd_prior_logp(ctx, C.byref(prm), sch.G_on(xd.device).data_ptr(), xd.data_ptr(), out.data_ptr(), B, T, Cn,
                                    _C.stream_of(xd)), ctx)
    ref = L.prior_logp(oracle_sde(kind, p, True, T), x)
    err, _ = report_err(f"fd_prior_logp {kind}", host(out), ref)
    assert err <= 1e-6


def _probes(name, n, P, T, Cn):
    e = W.randn(name, (n, P, T, Cn), 3)
    return np.where(e >= 0, 1.0, -1.0)


@pytest.mark.parametrize("kind,p", [("vp", (0.1, 20.0)), ("ve", (0.01, 50.0))])
@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_likelihood_run_against_the_restatement(kind, p, solver):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg, n, P, N = dict(T=20, C=3, D=8, L=2, H=4), 3, 2, 6
    m, sch, sd = make_model(cfg, kind=kind, p=p)
    x0 = W.randn(f"llr_x_{kind}", (n, cfg["T"], cfg["C"]), 0)
    e = _probes(f"llr_e_{kind}", n, P, cfg["T"], cfg["C"])
    res = DiffusionSampler(m, sample_batch_size=8).log_likelihood(torch.from_numpy(x0).float(), N, solver, n_probes=P,
                                                                  probes=torch.from_numpy(e).float())
    osde = oracle_sde(kind, p, True, cfg["T"])
    score = R.model_score(sd, "transformer", cfg["H"])
    lp, prior, drift, sdiv, x1 = L.log_likelihood(osde, score, L.fd_probe_trace(score, osde.G, e), x0, R.grid(N, to_noise=True), solver)
    scale = max(1.0, np.abs(x1).max())
    lat_err = float(np.abs(res.latents.numpy() - x1).max() / scale)
    err, _ = report_err(f"log_prob fp32 {kind} {solver} N={N}", res.log_prob.numpy(), lp)
    report_err(f"delta_log_prob fp32 {kind} {solver} N={N}", res.delta_log_prob.numpy(), drift + sdiv.mean(axis=1))
    print(f"latents fp32 {kind} {solver}: {lat_err:.3e} of scale")
    assert lat_err <= 1e-5
    assert err <= 1e-5
    np.testing.assert_allclose(res.prior_log_prob.numpy(), prior, rtol=1e-5)
    assert res.std_err is not None and res.std_err.shape == (n,)


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-6), ("bf16", 5e-2)])
def test_latents_equal_encode(precision, tol):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg, n, N = CFG_DEFAULT, 8, 5
    m, _, _ = make_model(cfg, precision=precision)
    X = torch.from_numpy(W.randn("lle_x", (n, cfg["T"], cfg["C"]), 0)).float()
    s = DiffusionSampler(m, sample_batch_size=n)
    res = s.log_likelihood(X, N, "heun", seed=7)
    enc = s.encode(X, N, "heun")
    scale = max(1.0, float(enc.abs().max()))
    err = float((res.latents - enc).abs().max()) / scale
    print(f"latents vs encode ({precision}, ecg shape, Heun N={N}): {err:.3e} of scale")
    report_err(f"latents vs encode {precision}", res.latents.numpy(), enc.numpy())
    assert np.isfinite(res.log_prob.numpy()).all()
    assert err <= tol


def test_exact_estimator_reproducibility_and_batch_independence():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg, n, N = CFG_T8, 3, 4
    m, sch, sd = make_model(cfg)
    x0 = W.randn("llx_x", (n, cfg["T"], cfg["C"]), 0)
    s = DiffusionSampler(m, sample_batch_size=4 * cfg["T"] * cfg["C"])
    X = torch.from_numpy(x0).float()
    ex = s.log_likelihood(X, N, "heun", estimator="exact")
    osde = oracle_sde("vp", (0.1, 20.0), True, cfg["T"])
    score = R.model_score(sd, "transformer", cfg["H"])
    lp, *_ = L.log_likelihood(osde, score, L.fd_trace(score, osde.G), x0, R.grid(N, to_noise=True), "heun")
    err, _ = report_err("exact estimator fp32 T=8 C=3 vs restatement", ex.log_prob.numpy(), lp)
    assert err <= 1e-5
    a = s.log_likelihood(X, N, "heun", n_probes=3, seed=11)
    b = s.log_likelihood(X, N, "heun", n_probes=3, seed=11)
    assert torch.equal(a.log_prob, b.log_prob) and torch.equal(a.latents, b.latents)
    assert torch.isfinite(a.std_err).all()
    # one series alone against the same series in a batch of three (its probes injected identically)
    e = torch.from_numpy(_probes("llx_e", n, 2, cfg["T"], cfg["C"])).float()
    full = s.log_likelihood(X, N, "heun", n_probes=2, probes=e)
    one = s.log_likelihood(X[1:2], N, "heun", n_probes=2, probes=e[1:2])
    d = abs(float(full.log_prob[1] - one.log_prob[0])) / max(1.0, abs(float(one.log_prob[0])))
    print(f"batch independence: {d:.3e} relative")
    assert d <= 1e-6 and torch.allclose(full.latents[1], one.latents[0], atol=1e-6, rtol=0)


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_likelihood(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=llrun"], tmp_path)
    _run([str(ROOT / "cmd" / "likelihood.py"), "model_id=llrun", "num_diffusion_steps=10", "n_probes=2", "max_series=40",
          "sampler.sample_batch_size=32"], tmp_path)
    res = yaml.safe_load(open(tmp_path / "lightning_logs" / "llrun" / "results.yaml"))["likelihood"]
    assert res["num_series"] == 40 and res["n_probes"] == 2 and res["fourier_transform"] is True
    for k in ("nll_data", "nll_data_se", "bits_per_dim", "nll_sample"):
        assert np.isfinite(res[k]), k
