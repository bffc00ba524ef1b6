"""GPU: the data-prediction ODE solvers (deterministic DDIM, DPM-Solver++ 2M: SDE.dpm_step / DiffusionSampler.sample_ode, decode /
fd_dpm_stage, fd_sampler_run_dpm; an extension not in the reference) and the log-SNR step grid against the float64 restatement of
tests/dpm_ref.py, and their three loop forms (persistent kernel, long-series fused launch, per-op launches) against each other.
The bounds are those of the same comparisons for Euler / Heun in tests/test_gpu_ode.py."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import weights as W
from oracle.make_golden import CFG_DEFAULT, CFG_TINY
from tests import dpm_ref as D
from tests.gpu_util import dev, host, make_model, oracle_sde, report_err
from tests.test_gpu_backbones import make_bb
from tests.test_gpu_ode import _env

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SDES = [("vp", (0.1, 20.0)), ("ve", (0.01, 2.0))]
SOLVERS = ["ddim", "dpmpp2m"]
SCHEDULES = ["time", "logsnr"]


def _f32(t):
    return float(np.float32(t))


def test_stage_vs_float64():
    """fd_dpm_stage (the loops' stage kernel on given x, score and previous D) against float64: first order and 2M, early, middle
    and last steps.  The engine rounds the times to float32 as the loop's grid is; so does the reference."""
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
                x, s, dp = (rs.randn(B, T, Cn).astype(np.float32) for _ in range(3))
                for tp, t, tn in ((1.0, 0.8, 0.55), (0.45, 0.37, 0.3), (1e-3, 1e-4, 1e-5)):
                    tp, t, tn = _f32(tp), _f32(t), _f32(tn)
                    d_ref = D.data_prediction(sde, s, t, x)
                    for second in (False, True):
                        if second:
                            got_x, got_d = sch.dpm_step(dev(s), t, tn, dev(x), prev_data=dev(dp), prev_timestep=tp)
                            ref_x = D.step(sde, x, d_ref, t, tn, dp, tp)
                        else:
                            got_x, got_d = sch.dpm_step(dev(s), t, tn, dev(x))
                            ref_x = D.step(sde, x, d_ref, t, tn)
                        for got, ref in ((host(got_x), ref_x), (host(got_d), d_ref)):
                            err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
                            worst = max(worst, err)
                            assert err <= 1e-6, (kind, scaling, Cn, t, second, err)
    print(f"fd_dpm_stage: worst max err / scale = {worst:.3e}")


def _f32_case(m_, sd, kind, p, solver, schedule, N, B, T, Cn, tag, backbone="transformer", n_head=None):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    zp = W.randn(f"dpm_p_{tag}", (B, T, Cn), 3)
    got = DiffusionSampler(score_model=m_, sample_batch_size=B).sample_ode(B, N, solver=solver, schedule=schedule,
                                                                           prior_noise=[dev(zp)]).numpy()
    ref = D.sample_ode(sd, oracle_sde(kind, p, True, T), zp, N, solver, schedule, backbone, n_head)
    err, _ = report_err(f"sample_ode f32 {tag}", got, ref)
    assert err <= 1e-5, err


@pytest.mark.parametrize("name", ["tiny", "default"])
@pytest.mark.parametrize("kind,p", SDES)
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("solver", SOLVERS)
def test_sample_ode_f32_vs_float64(name, kind, p, solver, schedule):
    cfg = {"tiny": CFG_TINY, "default": dict(CFG_DEFAULT, L=2)}[name]
    m_, _, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    _f32_case(m_, sd, kind, p, solver, schedule, 12, 4, cfg["T"], cfg["C"], f"{name} {kind} {solver} {schedule} N=12", n_head=cfg["H"])


@pytest.mark.parametrize("kind,p", SDES)
@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_euler_heun_on_the_logsnr_grid_f32_vs_float64(kind, p, solver):
    """The schedule is independent of the solver: Euler and Heun on the log-SNR grid, sampling and decoding."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = CFG_TINY
    m_, _, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    _f32_case(m_, sd, kind, p, solver, "logsnr", 10, 4, cfg["T"], cfg["C"], f"tiny {kind} {solver} logsnr N=10", n_head=cfg["H"])
    zp = W.randn("dpm_dec", (4, cfg["T"], cfg["C"]), 3).astype(np.float32)
    s = DiffusionSampler(score_model=m_, sample_batch_size=4)
    a = s.decode(torch.from_numpy(zp), 10, solver="dpmpp2m", schedule="logsnr")
    sde = oracle_sde(kind, p, True, cfg["T"])
    ref = D.solve(sde, D.R.model_score(sd, n_head=cfg["H"]), zp, D.grid(sde, 10, "logsnr"), "dpmpp2m")
    err, _ = report_err(f"decode f32 tiny {kind} dpmpp2m logsnr N=10", a.numpy(), ref)
    assert err <= 1e-5, err


@pytest.mark.parametrize("backbone", ["mlp", "lstm"])
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("solver", SOLVERS)
def test_sample_ode_backbones_vs_float64(backbone, solver, schedule):
    cfg = dict(T=20, C=3, D=16, L=2)
    m_, _, sd = make_bb(backbone, cfg, 64)
    _f32_case(m_, sd, "vp", (0.1, 20.0), solver, schedule, 12, 5, cfg["T"], cfg["C"], f"{backbone} {solver} {schedule} N=12",
              backbone=backbone)


def _bf16_pair(cfg, B, N, solver, schedule, switch):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    outs = []
    zp = dev(W.randn(f"dpm_bf16_{cfg['T']}_{cfg['C']}", (B, cfg["T"], cfg["C"]), 4))
    for off in (False, True):
        m_, _, _ = make_model(cfg, precision="bf16")
        with _env(**{switch: "1" if off else None}):
            outs.append(DiffusionSampler(score_model=m_, sample_batch_size=B).sample_ode(B, N, solver=solver, schedule=schedule,
                                                                                         prior_noise=[zp]).numpy())
    assert np.isfinite(outs[0]).all() and np.isfinite(outs[1]).all()
    return outs


@pytest.mark.parametrize("C", [3, 6, 12])
@pytest.mark.parametrize("solver", SOLVERS)
def test_persistent_dpm_equals_stepwise_bf16(C, solver):
    """The one-launch loop in k_mega (ODE instantiation, run-time stage; C = 3, 6: the ragged epilogue, 12: the float4 one) against
    one score launch + one stage launch per evaluation (FDIFF_SAMPLER_STEPWISE).  2e-3 of scale."""
    cfg = dict(T=40, C=C, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision="bf16")
    assert m_.plan(5, "bf16")[0].startswith("k_mega"), m_.plan(5, "bf16")
    a, b = _bf16_pair(cfg, 5, 10, solver, "logsnr", "FDIFF_SAMPLER_STEPWISE")
    err, _ = report_err(f"dpm bf16 persistent vs stepwise C={C} {solver}", a, b)
    assert err <= 2e-3, err


@pytest.mark.parametrize("T,C", [(260, 3), (300, 12)])
@pytest.mark.parametrize("solver", SOLVERS)
def test_long_series_fused_dpm_equals_unfused_bf16(T, C, solver):
    """T > 256: layer launches + ONE unembed / stage / next embedding launch (k_unembed_step_embed's ODE form) against the separate
    launches (FDIFF_SAMPLER_UNFUSED_STEP).  5e-3 of scale."""
    cfg = dict(T=T, C=C, D=72, L=2, H=12)
    a, b = _bf16_pair(cfg, 3, 6, solver, "logsnr", "FDIFF_SAMPLER_UNFUSED_STEP")
    err, _ = report_err(f"dpm bf16 long fused vs unfused T={T} C={C} {solver}", a, b)
    assert err <= 5e-3, err


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_deterministic(precision, solver):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(T=40, C=5, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision=precision)
    s = DiffusionSampler(score_model=m_, sample_batch_size=6)
    zp = dev(W.randn("dpm_det", (6, 40, 5), 5))
    a = s.sample_ode(6, 15, solver=solver, schedule="logsnr", prior_noise=[zp])
    b = s.sample_ode(6, 15, solver=solver, schedule="logsnr", prior_noise=[zp])
    assert torch.isfinite(a).all() and torch.equal(a, b)


def _launch_flops(sampler, zp, N, solver):
    """(kernel name, launches, algorithmic flops per launch) of one sample_ode call, from the engine's profiling bracket."""
    from fourierdiffusion_amd import _C
    ctx, _ = sampler.score_model._engine()
    lib = _C.lib()
    _C.check(lib.fd_prof_begin(ctx), ctx)
    sampler.sample_ode(zp.shape[0], N, solver=solver, schedule="logsnr", prior_noise=[zp])
    name, avg_us, cnt, flops = C.create_string_buffer(128), C.c_double(0), C.c_int(0), C.c_double(0)
    _C.check(lib.fd_prof_end(ctx, name, C.byref(avg_us), C.byref(cnt), C.byref(flops)), ctx)
    return name.value.decode(), cnt.value, flops.value


def test_n_steps_cost_n_evaluations():
    """The persistent kernel's launch record carries (flops of one forward) x series x evaluations: N steps of either new solver
    are N evaluations, as Euler's, and half of Heun's."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(T=40, C=5, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision="bf16")
    assert m_.plan(6, "bf16")[0].startswith("k_mega")
    s = DiffusionSampler(score_model=m_, sample_batch_size=6)
    zp = dev(W.randn("dpm_cnt", (6, 40, 5), 5))
    N = 12
    rec = {sol: _launch_flops(s, zp, N, sol) for sol in ("euler", "heun", "ddim", "dpmpp2m")}
    print(rec)
    for name, cnt, fl in rec.values():
        assert name.startswith("k_mega") and cnt == 1 and fl > 0, rec
    per_eval = rec["euler"][2] / N
    assert rec["ddim"][2] == N * per_eval and rec["dpmpp2m"][2] == N * per_eval and rec["heun"][2] == 2 * N * per_eval
    assert _launch_flops(s, zp, 2 * N, "dpmpp2m")[2] == 2 * N * per_eval


def test_engine_rejects_bad_grids():
    """fd_sampler_run_dpm refuses an increasing or non-finite grid; fd_sampler_run_ode keeps refusing the new solver ids."""
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = dict(T=40, C=5, D=24, L=2, H=4)
    m_, _, _ = make_model(cfg, precision="fp32")
    s = DiffusionSampler(score_model=m_, sample_batch_size=2)
    ctx, h, p, G, mode = s._engine_args()
    X = s.sample_prior(2)
    before = X.clone()
    lib = _C.lib()

    def arr(v):
        return (C.c_float * len(v))(*v)
    for grid in ([1e-5, 0.5, 1.0], [1.0, 0.5, 0.5], [1.0, float("nan"), 1e-5], [1.0, float("inf"), 1e-5]):
        for sid in (2, 3):
            rc = lib.fd_sampler_run_dpm(h, C.byref(p), G.data_ptr(), arr(grid), 2, sid, X.data_ptr(), 2, mode, _C.stream_of(X))
            assert rc != 0, grid
    for sid in (0, 1, 4, -1):
        assert lib.fd_sampler_run_dpm(h, C.byref(p), G.data_ptr(), arr([1.0, 0.5, 1e-5]), 2, sid, X.data_ptr(), 2, mode, _C.stream_of(X)) != 0
    for sid in (2, 3):
        assert lib.fd_sampler_run_ode(h, C.byref(p), G.data_ptr(), arr([1.0, 0.5, 1e-5]), 2, sid, X.data_ptr(), 2, mode, _C.stream_of(X)) != 0
    assert torch.equal(X, before)


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_sample_dpm(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=dpmrun"], tmp_path)
    _run([str(ROOT / "cmd" / "sample.py"), "model_id=dpmrun", "sampler=dpm", "num_diffusion_steps=20", "num_samples=40",
          "sampler.sample_batch_size=20"], tmp_path)
    X = torch.load(tmp_path / "lightning_logs" / "dpmrun" / "samples.pt")
    assert X.shape == (40, 24, 4) and torch.isfinite(X).all()
