"""GPU: the probability-flow ODE sampler (SDE.ode_drift / DiffusionSampler.sample_ode, encode, decode / fd_pf_ode_drift,
fd_sampler_run_ode; an extension not in the reference) against the float64 restatement of tests/ode_ref.py, and its three loop
forms (persistent kernel, long-series fused launch, per-op launches) against each other."""
import contextlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W
from oracle.make_golden import CFG_DEFAULT, CFG_TINY
from tests import ode_ref as R
from tests.gpu_util import dev, host, make_model, oracle_sde, report_err
from tests.test_gpu_backbones import make_bb

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SDES = [("vp", (0.1, 20.0)), ("ve", (0.01, 2.0))]


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_drift_vs_float64():
    from fourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler
    worst = 0.0
    for kind, p in SDES:
        for scaling in (False, True):
            for Cn in (1, 3, 12, 20):
                T, B = 37, 3
                sch = (VPScheduler if kind == "vp" else VEScheduler)(p[0], p[1], fourier_noise_scaling=scaling)
                sch.set_noise_scaling(T)
                sde = oracle_sde(kind, p, scaling, T)
                rs = np.random.RandomState(Cn)
                x, s = rs.randn(B, T, Cn).astype(np.float32), rs.randn(B, T, Cn).astype(np.float32)
                for t in (1e-5, 0.37, 1.0):
                    got = host(sch.ode_drift(dev(s), t, dev(x)))
                    ref = R.velocity(sde, s, t, x)
                    err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
                    worst = max(worst, err)
                    assert err <= 1e-6, (kind, scaling, Cn, t, err)
    print(f"fd_pf_ode_drift: worst max err / scale = {worst:.3e}")


def _f32_case(m_, sd, kind, p, solver, N, B, T, Cn, tag, backbone="transformer", n_head=None):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    zp = W.randn(f"ode_p_{tag}", (B, T, Cn), 3)
    got = DiffusionSampler(score_model=m_, sample_batch_size=B).sample_ode(B, N, solver=solver, prior_noise=[dev(zp)]).numpy()
    ref = R.sample_ode(sd, oracle_sde(kind, p, True, T), zp, N, solver, backbone, n_head)
    err, _ = report_err(f"sample_ode f32 {tag}", got, ref)
    assert err <= 1e-5, err


@pytest.mark.parametrize("name", ["tiny", "default"])
@pytest.mark.parametrize("kind,p", SDES)
@pytest.mark.parametrize("solver,N", [("euler", 20), ("heun", 8)])
def test_sample_ode_f32_vs_float64(name, kind, p, solver, N):
    cfg = {"tiny": CFG_TINY, "default": dict(CFG_DEFAULT, L=2)}[name]
    m_, _, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    _f32_case(m_, sd, kind, p, solver, N, 4, cfg["T"], cfg["C"], f"{name} {kind} {solver} N={N}", n_head=cfg["H"])


@pytest.mark.parametrize("backbone", ["mlp", "lstm"])
@pytest.mark.parametrize("solver,N", [("euler", 12), ("heun", 8)])
def test_sample_ode_backbones_vs_float64(backbone, solver, N):
    cfg = dict(T=20, C=3, D=16, L=2)
    m_, _, sd = make_bb(backbone, cfg, 64)
    _f32_case(m_, sd, "vp", (0.1, 20.0), solver, N, 5, cfg["T"], cfg["C"], f"{backbone} {solver} N={N}", backbone=backbone)


def _bf16_pair(cfg, B, N, solver, switch):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    outs = []
    zp = dev(W.randn(f"ode_bf16_{cfg['T']}_{cfg['C']}", (B, cfg["T"], cfg["C"]), 4))
    for off in (False, True):
        m_, _, _ = make_model(cfg, precision="bf16")
        with _env(**{switch: "1" if off else None}):
            outs.append(DiffusionSampler(score_model=m_, sample_batch_size=B).sample_ode(B, N, solver=solver, prior_noise=[zp]).numpy())
    assert np.isfinite(outs[0]).all() and np.isfinite(outs[1]).all()
    return outs


@pytest.mark.parametrize("C", [3, 6, 12])
@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_persistent_ode_equals_stepwise_bf16(C, solver):
    """The one-launch ODE loop in k_mega (ODE instantiation; C = 3, 6: the ragged epilogue, 12: the float4 one) against one score
    launch + one stage launch per evaluation (FDIFF_SAMPLER_STEPWISE).  Bound as for the SDE loop: 2e-3 of scale."""
    cfg = dict(T=40, C=C, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision="bf16")
    assert m_.plan(5, "bf16")[0].startswith("k_mega"), m_.plan(5, "bf16")
    a, b = _bf16_pair(cfg, 5, 10, solver, "FDIFF_SAMPLER_STEPWISE")
    err, _ = report_err(f"ode bf16 persistent vs stepwise C={C} {solver}", a, b)
    assert err <= 2e-3, err


@pytest.mark.parametrize("T,C", [(260, 3), (300, 12)])
@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_long_series_fused_ode_equals_unfused_bf16(T, C, solver):
    """T > 256: layer launches + ONE unembed / ODE stage / next embedding launch (k_unembed_step_embed's ODE form) against the
    separate launches (FDIFF_SAMPLER_UNFUSED_STEP).  5e-3 of scale."""
    cfg = dict(T=T, C=C, D=72, L=2, H=12)
    a, b = _bf16_pair(cfg, 3, 6, solver, "FDIFF_SAMPLER_UNFUSED_STEP")
    err, _ = report_err(f"ode bf16 long fused vs unfused T={T} C={C} {solver}", a, b)
    assert err <= 5e-3, err


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_deterministic(precision):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(T=40, C=5, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision=precision)
    s = DiffusionSampler(score_model=m_, sample_batch_size=6)
    zp = dev(W.randn("ode_det", (6, 40, 5), 5))
    a = s.sample_ode(6, 15, prior_noise=[zp])
    b = s.sample_ode(6, 15, prior_noise=[zp])
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_encode_decode_round_trip_f32():
    """decode(encode(x)), fp32 Heun, VP, default shape: both directions match the float64 restatement, so the round trip returns x
    up to the solver's discretisation error for this network -- which is not small for random weights (no trained score field):
    measured 1.25e-1 of scale at N = 50 (bound 2.5e-1) and 5.3e-3 at N = 200: it must shrink with the step count."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(CFG_DEFAULT, L=2)
    m_, _, sd = make_model(cfg, precision="fp32")
    s = DiffusionSampler(score_model=m_, sample_batch_size=4)
    x = W.randn("ode_rt", (4, cfg["T"], cfg["C"]), 6).astype(np.float32)
    sde, fn = oracle_sde("vp", (0.1, 20.0), True, cfg["T"]), R.model_score(sd, n_head=cfg["H"])
    lat = s.encode(torch.from_numpy(x), 50)
    back = s.decode(lat, 50)
    ref_lat = R.solve(sde, fn, x, R.grid(50, to_noise=True), "heun")
    ref_back = R.solve(sde, fn, lat.numpy(), R.grid(50), "heun")
    e_lat, _ = report_err("encode f32 heun N=50", lat.numpy(), ref_lat)
    e_back, _ = report_err("decode f32 heun N=50", back.numpy(), ref_back)
    assert e_lat <= 1e-4 and e_back <= 1e-4, (e_lat, e_back)      # (measured 9.4e-6 for decode: f32 rounding grows along 100 evaluations)
    errs = []
    for N, b in ((50, back), (200, s.decode(s.encode(torch.from_numpy(x), 200), 200))):
        errs.append(float(np.abs(b.numpy() - x).max() / np.abs(x).max()))
        print(f"[parity] encode/decode round trip fp32 heun N={N}: max err / scale = {errs[-1]:.3e}")
    assert errs[0] <= 2.5e-1 and errs[1] < errs[0], errs


def test_launch_merging_and_ode_sampler():
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.sampler import ODESampler
    cfg = dict(T=40, C=5, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision="bf16")
    s = instantiate(compose(ROOT / "cmd" / "conf", "sample", ["sampler=ode", "sampler.sample_batch_size=7"]).sampler)(score_model=m_)
    assert type(s) is ODESampler and s.solver == "heun"
    sizes = s._launch_sizes(7 * 9, 1)
    assert sum(sizes) == 63
    X = s.sample(num_samples=65, num_diffusion_steps=4)          # 9 batches of 7; the remainder dropped as in sample()
    assert X.shape == (63, 40, 5) and torch.isfinite(X).all()


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_sample_ode(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=oderun"], tmp_path)
    _run([str(ROOT / "cmd" / "sample.py"), "model_id=oderun", "sampler=ode", "num_diffusion_steps=10", "num_samples=40",
          "sampler.sample_batch_size=20"], tmp_path)
    X = torch.load(tmp_path / "lightning_logs" / "oderun" / "samples.pt")
    assert X.shape == (40, 24, 4) and torch.isfinite(X).all()
