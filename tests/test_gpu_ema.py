"""GPU: the exponential moving average of the weights, fused into the AdamW pass (fd_adamw_ema_step; an extension, not in the
reference) -- bit-identity of the parameter update with fd_adamw_step, the recurrence against tests/ema_ref.py, the two exact
end points, the frozen range and the on-device skip, the swap of the weights the engine runs on (use_ema), the trainer end to end
and one other backbone."""
import importlib.util
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import weights as W
from oracle.make_golden import CFG_TINY

from . import ema_ref as E
from .gpu_util import DEV, dev, host, make_model

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HP = (0.9, 0.999, 1e-8, 1e-2)                  # betas, eps, weight decay of the existing optimizer test


def batch_of(X, t):
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    return DiffusableBatch(X=dev(X), y=None, timesteps=dev(t))


def _grad(name, n):
    return dev(W.randn(name, (n,), 6) * np.float32(3.0))


def _ema_step(p, g, m, v, ema, d, step, lr, sq=None, max_norm=0.0, frozen=(0, 0)):
    from fourierdiffusion_amd import _C
    h = _C.ctx(p.device)
    _C.check(_C.lib().fd_adamw_ema_step(h, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(), d, p.numel(), step,
                                        lr, *HP, None if sq is None else sq.data_ptr(), max_norm, 1.0, frozen[0], frozen[1], None), h)


@pytest.mark.parametrize("n", [257, 1 << 20])
def test_parameter_update_is_bit_identical_to_the_plain_step(n):
    """Three steps, clipping on, a frozen range: p, m, v of fd_adamw_ema_step are those of fd_adamw_step.  (n = 2^20 is more than
    the grid holds threads: the grid-stride loop runs.)"""
    from fourierdiffusion_amd import _C
    L = _C.lib()
    p0 = dev(W.randn("opt_p", (n,), 6))
    a = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    b = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    ema = p0.clone()
    sq = torch.zeros(1, device=DEV)
    h = _C.ctx(p0.device)
    for it in range(3):
        g = _grad(f"opt_g{it}", n)
        _C.check(L.fd_grad_sqnorm(h, g.data_ptr(), n, sq.data_ptr(), None), h)
        lr = 1e-3 * (it + 1) / 3
        _C.check(L.fd_adamw_step(h, a[0].data_ptr(), g.data_ptr(), a[1].data_ptr(), a[2].data_ptr(), n, it + 1, lr, *HP,
                                 sq.data_ptr(), 1.0, 1.0, 10, 20, None), h)
        _ema_step(b[0], g, b[1], b[2], ema, 0.9, it + 1, lr, sq, 1.0, (10, 20))
        for x, y, name in zip(a, b, "pmv"):
            assert torch.equal(x, y), (name, it)
        assert torch.equal(ema[10:20], p0[10:20]) and torch.equal(b[0][10:20], p0[10:20])
    assert not torch.equal(a[0], p0) and not torch.equal(ema, p0) and not torch.equal(ema, b[0])


def _run_recurrence(n, K, decay, warmup, frozen=(0, 0)):
    p = dev(W.randn("ema_p", (n,), 6))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ema = dev(W.randn("ema_e0", (n,), 6))
    e0 = ema.cpu().numpy().copy()
    ps, es, ds = [], [], []
    for k in range(K):
        d = E.decay_at(k, decay, warmup)
        _ema_step(p, _grad(f"ema_g{k}", n), m, v, ema, d, k + 1, 1e-2, frozen=frozen)
        ps.append(p.cpu().numpy().copy())
        es.append(ema.cpu().numpy().copy())
        ds.append(d)
    return e0, ps, es, ds


def test_recurrence_matches_the_restatement():
    """K = 20 steps with the warm-up schedule: the device's float32 average against the float64 recurrence on the device's own
    float32 parameters, within K * 2^-23 * max_k max(|p_k|, |e_k|) per element (tests/ema_ref.py: two float32 roundings per step)."""
    K = 20
    e0, ps, es, ds = _run_recurrence(4099, K, 0.999, True)
    assert ds[0] == 0.1 and ds == sorted(ds) and ds[-1] == 20 / 29
    ref = E.recurrence(e0, ps, ds)
    tol = E.tolerance(ps, ref)
    err = np.abs(es[-1].astype(np.float64) - ref[-1])
    print(f"[ema] recurrence after {K} steps: worst |device - float64| / bound = {(err / tol).max():.3f}, "
          f"worst abs {err.max():.3e}, bound there {tol[np.argmax(err / tol)]:.3e}")
    assert (tol > 0).all() and (err <= tol).all(), float((err / tol).max())
    assert np.abs(es[-1] - ps[-1]).max() > 1e-3                   # (the average is not simply the weights)


def test_end_points_are_exact():
    e0, ps, es, _ = _run_recurrence(1031, 4, 0.0, False)
    for p, e in zip(ps, es):
        assert np.array_equal(p, e)                               # d = 0: the average IS the updated weights
    e0, ps, es, _ = _run_recurrence(1031, 4, 1.0, False)
    for e in es:
        assert np.array_equal(e, e0)                              # d = 1: untouched
    assert not np.array_equal(ps[-1], ps[0])


def test_frozen_range_and_bad_arguments():
    from fourierdiffusion_amd import _C
    e0, ps, es, _ = _run_recurrence(1031, 3, 0.5, False, frozen=(100, 164))
    p0 = W.randn("ema_p", (1031,), 6)
    for p, e in zip(ps, es):
        assert np.array_equal(e[100:164], e0[100:164]) and np.array_equal(p[100:164], p0[100:164])
    assert (es[-1][:100] != e0[:100]).all() and (es[-1][164:] != e0[164:]).all()
    p = dev(p0)
    z = torch.zeros_like(p)
    for d in (-0.01, 1.01):
        with pytest.raises(_C.FdError, match="ema_decay"):
            _ema_step(p, z, z.clone(), z.clone(), p.clone(), d, 1, 1e-3)
    h = _C.ctx(p.device)
    rc = _C.lib().fd_adamw_ema_step(h, p.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 0.5, 1031, 1, 1e-3, *HP, None, 0.0,
                                    1.0, 0, 0, None)
    assert rc != 0 and b"ema" in _C.lib().fd_last_error(h)
    assert torch.equal(p, dev(p0))


def test_update_skipped_on_the_device_leaves_the_average_untouched(monkeypatch):
    """The bounded-wait test hook of tests/test_gpu_train_persist.py (a cluster member never raises its flags; every wait gives up
    after FDIFF_TR_TIMEOUT_MS) sets the training error word: the optimizer pass enqueued behind that step skips itself in stream
    order -- the average with the parameters and the moments."""
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.optim import FusedAdamW
    from fourierdiffusion_amd.utils.losses import get_sde_loss_fn
    from .test_gpu_train_persist import _data, _step
    cfg, B = dict(T=100, C=12, D=72, L=2, H=12), 9
    X, z, t = _data("stall", cfg, B)
    m, sch, _ = make_model(cfg, precision="bf16")
    fn = get_sde_loss_fn(sch, train=True)
    ctx, _h = m._engine()
    lib = _C.lib()
    monkeypatch.setenv("FDIFF_TR_FSPLIT", "0")
    _step(m, fn, X, z, t, seed=92)
    assert lib.fd_ctx_check(ctx) == 0
    assert "k_tr_fwd_layers NT=2, 4 x 9 workgroups" in m.train_plan(B)[0], m.train_plan(B)[0]
    opt = FusedAdamW(m, lr=1e-3, ema_decay=0.5, ema_warmup=False)
    opt.step()                                         # a real update first: moments and average are not trivial
    _step(m, fn, X, z, t, seed=92)
    torch.cuda.synchronize()
    assert not torch.equal(m.ema_parameters, m.flat_parameters)
    before = [x.clone() for x in (m.flat_parameters, m.ema_parameters, opt.exp_avg, opt.exp_avg_sq)]
    monkeypatch.setenv("FDIFF_TR_PERSIST_TEST_STALL", "1")
    monkeypatch.setenv("FDIFF_TR_TIMEOUT_MS", "100")
    m.zero_grad()
    torch.manual_seed(92)
    fn(m, batch_of(X, t), noise=dev(z))
    opt.step()
    torch.cuda.synchronize()
    monkeypatch.delenv("FDIFF_TR_PERSIST_TEST_STALL")
    monkeypatch.delenv("FDIFF_TR_TIMEOUT_MS")
    try:
        for x, y, name in zip((m.flat_parameters, m.ema_parameters, opt.exp_avg, opt.exp_avg_sq), before, ("p", "ema", "m", "v")):
            assert torch.equal(x, y), f"{name} changed in an update whose training step timed out"
    finally:
        rc = lib.fd_ctx_check(ctx)                     # reported once; then the context is handed back as the other tests expect it
        assert lib.fd_ctx_check(ctx) == 0 and lib.fd_ctx_rearm(ctx) == 0
    assert rc != 0


CFG_PERSIST = dict(T=100, C=12, D=72, L=2, H=12)       # the default width: bf16 MFMA, served by the persistent kernel


@pytest.mark.parametrize("precision,cfg", [("fp32", CFG_TINY), ("bf16", CFG_PERSIST)], ids=["fp32", "bf16"])
def test_engine_runs_on_the_swapped_weights(precision, cfg):
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.optim import FusedAdamW
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    B = 8
    m, sch, _ = make_model(cfg, precision=precision)
    X = W.randn("ema_x", (B, cfg["T"], cfg["C"]), 3)
    z = W.randn("ema_z", (B, cfg["T"], cfg["C"]), 3)
    t = W.uniform("ema_t", (B,), 3, 0.05, 1.0)
    opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0, ema_decay=0.9)
    torch.manual_seed(3)
    for _ in range(30):
        opt.zero_grad()
        m.training_loss_fn(m, batch_of(X, t), noise=dev(z))
        opt.step()
    assert opt.ema_num_updates == 30 and m.train_mode_effective == precision
    m.eval()
    if precision == "bf16":
        assert m.precision_effective == "bf16" and m.plan(B)[0].startswith("k_mega"), m.plan(B)[0]
    ema_sd, raw_sd = m.ema_state_dict(), m.state_dict()
    assert not torch.equal(ema_sd["embedder.weight"], raw_sd["embedder.weight"])
    raw_out = m(batch_of(X, t)).clone()
    with m.use_ema():
        in_out = m(batch_of(X, t)).clone()
        torch.manual_seed(5)
        in_samples = DiffusionSampler(score_model=m, sample_batch_size=B).sample(num_samples=B, num_diffusion_steps=5)
        with pytest.raises(_C.FdError, match="use_ema"):
            opt.step()
    assert torch.equal(m(batch_of(X, t)), raw_out)                # back on the raw weights (and their images), bit for bit
    assert not torch.equal(in_out, raw_out)
    fresh, _, _ = make_model(cfg, precision=precision)
    fresh.load_state_dict(ema_sd)
    fresh.eval()
    assert torch.equal(fresh(batch_of(X, t)), in_out)
    torch.manual_seed(5)
    fresh_samples = DiffusionSampler(score_model=fresh, sample_batch_size=B).sample(num_samples=B, num_diffusion_steps=5)
    assert torch.isfinite(in_samples).all() and torch.equal(in_samples, fresh_samples)
    # a second visit (both buffers prepared, nothing changed in between) gives the same two answers again
    with m.use_ema():
        assert torch.equal(m(batch_of(X, t)), in_out)
    assert torch.equal(m(batch_of(X, t)), raw_out)
    # and training goes on from the raw weights
    m.train()
    opt.zero_grad()
    m.training_loss_fn(m, batch_of(X, t), noise=dev(z))
    opt.step()
    assert opt.ema_num_updates == 31


def _train_module():
    spec = importlib.util.spec_from_file_location("fdiff_cmd_train", str(ROOT / "cmd" / "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_end_to_end(tmp_path, monkeypatch):
    from fourierdiffusion_amd.config import compose
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.trainer import Callback
    monkeypatch.chdir(tmp_path)
    T = _train_module()
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32", "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
              "trainer.max_epochs=2", "trainer.enable_progress_bar=false", "trainer.callbacks.2.every_n_epochs=1",
              "trainer.callbacks.2.num_samples=32", "trainer.callbacks.2.num_diffusion_steps=5"]

    class SaveLast(Callback):
        def on_validation_end(self, trainer, model) -> None:
            if trainer.current_epoch + 1 == trainer.max_epochs:
                model.save_checkpoint(Path(trainer.default_root_dir) / "last.ckpt", optimizer_state=trainer.optimizer.state_dict())

    runs = {}
    for run_id, extra in (("emarun", ["trainer=ema", "trainer.ema_decay=0.99"]), ("rawrun", [])):
        cfg = compose(ROOT / "cmd" / "conf", "train", extra + common + [f"run_id={run_id}"], cwd=str(tmp_path))
        runner = T.TrainingRunner(cfg)
        runner.trainer.callbacks.append(SaveLast())
        runner.train()
        runs[run_id] = runner
    ema_run, raw_run = runs["emarun"], runs["rawrun"]
    tr, model = ema_run.trainer, ema_run.score_model
    assert tr.ema_decay == 0.99 and raw_run.trainer.ema_decay is None and raw_run.score_model.ema_parameters is None
    assert tr.global_step == 6 and tr.optimizer.ema_num_updates == 6
    # averaging, and evaluating on the average, left the trajectory alone
    assert torch.equal(model.flat_parameters, raw_run.score_model.flat_parameters)
    assert "val/loss_raw" not in raw_run.trainer.logged
    for k in ("val/loss", "val/loss_raw"):
        assert np.isfinite(tr.logged[k]), (k, tr.logged)
    assert tr.logged["val/loss"] != tr.logged["val/loss_raw"]
    assert tr.logged["val/loss_raw"] == raw_run.trainer.logged["val/loss"]      # same weights, same timesteps and noise
    print(f"[ema] trainer: val/loss {tr.logged['val/loss']:.5f} (averaged), val/loss_raw {tr.logged['val/loss_raw']:.5f}")
    # the checkpoint ModelCheckpoint chose holds both weight sets and the optimizer state
    ckpts = list((ema_run.save_dir / "checkpoints").glob("epoch=*-val_loss=*.ckpt"))
    assert len(ckpts) == 1
    ck = torch.load(ckpts[0], map_location="cpu", weights_only=False)
    assert sorted(ck["ema_state_dict"]) == sorted(ck["state_dict"])
    assert any(not torch.equal(ck["ema_state_dict"][k], v) for k, v in ck["state_dict"].items())
    assert ck["ema"]["decay"] == 0.99 and ck["ema"]["warmup"] is True
    assert ck["ema"]["num_updates"] == ck["optimizer_state"]["ema_num_updates"] == ck["global_step"]
    # weights="ema" reloads the model the scope runs; weights="raw" the trained one with the average attached
    last = ema_run.save_dir / "last.ckpt"
    reloaded = ScoreModule.load_from_checkpoint(last, weights="ema").to(DEV).eval()
    both = ScoreModule.load_from_checkpoint(last).to(DEV).eval()
    assert reloaded.weights_loaded == "ema" and reloaded.ema_parameters is None
    assert torch.equal(reloaded.flat_parameters, model.ema_parameters)
    assert torch.equal(both.flat_parameters, model.flat_parameters) and torch.equal(both.ema_parameters, model.ema_parameters)
    X = W.randn("ema_tx", (5, 24, 4), 3)
    t = W.uniform("ema_tt", (5,), 3, 0.05, 1.0)
    # (A loaded model prepares the stored weights anew, which applies the reference's max_norm renormalisation of the positional
    #  table once more to rows that sit AT the bound and moves their last bits -- tests/test_gpu_train_persist.py meets the same.  The
    #  trained model is told to do as much, so that the comparison is of the same weights through the same preparation.)
    model.mark_parameters_changed()
    model.mark_ema_changed()
    model.eval()
    with model.use_ema():
        in_out = model(batch_of(X, t)).clone()
    raw_out = model(batch_of(X, t)).clone()
    assert not torch.equal(in_out, raw_out)
    assert torch.equal(reloaded(batch_of(X, t)), in_out)
    assert torch.equal(both(batch_of(X, t)), raw_out)
    with both.use_ema():
        assert torch.equal(both(batch_of(X, t)), in_out)
    # cmd/sample.py picks the averaged weights of that run directory, and says so
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    outs = {}
    for w in ("auto", "raw"):
        r = subprocess.run([sys.executable, str(ROOT / "cmd" / "sample.py"), "model_id=emarun", "num_samples=32", "num_diffusion_steps=5",
                            "sampler.sample_batch_size=32", f"weights={w}"], cwd=tmp_path, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert ("averaged (EMA) weights" in r.stderr) == (w == "auto") and ("raw weights" in r.stderr) == (w == "raw"), r.stderr[-2000:]
        outs[w] = torch.load(ema_run.save_dir / "samples.pt")
    assert outs["auto"].shape == (32, 24, 4) and torch.isfinite(outs["auto"]).all() and not torch.equal(outs["auto"], outs["raw"])


def test_average_on_the_mlp_backbone():
    """Through FusedAdamW on MLPScoreModule: the mechanism is the flat buffer, not the backbone."""
    from fourierdiffusion_amd.models.score_models import MLPScoreModule
    from fourierdiffusion_amd.optim import FusedAdamW
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    T, C, B, K = 16, 3, 6, 12
    sch = VPScheduler(beta_min=0.1, beta_max=20.0, fourier_noise_scaling=True)
    sch.set_noise_scaling(T)
    torch.manual_seed(11)
    m = MLPScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=24, d_mlp=48, num_layers=2).to(DEV)
    X = W.randn("ema_mx", (B, T, C), 3)
    z = W.randn("ema_mz", (B, T, C), 3)
    t = W.uniform("ema_mt", (B,), 3, 0.05, 1.0)
    opt = FusedAdamW(m, lr=1e-2, max_grad_norm=1.0, ema_decay=0.95)
    e0 = host(m.ema_parameters)
    assert np.array_equal(e0, host(m.flat_parameters))
    ps, ds = [], []
    for k in range(K):
        opt.zero_grad()
        m.training_loss_fn(m, batch_of(X, t), noise=dev(z))
        opt.step()
        ps.append(m.flat_parameters.cpu().numpy().copy())
        ds.append(E.decay_at(k, 0.95, True))
    ref = E.recurrence(e0, ps, ds)
    tol = E.tolerance(ps, ref)
    err = np.abs(host(m.ema_parameters) - ref[-1])
    moved = tol > 0                                               # (parameters that are zero throughout have a zero bound and a zero error)
    assert (err <= tol).all() and moved.any(), float((err[moved] / tol[moved]).max())
    lo, hi = opt._frozen
    assert hi > lo and np.array_equal(host(m.ema_parameters)[lo:hi], e0[lo:hi])
    m.eval()
    raw_out = m(batch_of(X, t)).clone()
    with m.use_ema():
        assert not torch.equal(m(batch_of(X, t)), raw_out)
    assert torch.equal(m(batch_of(X, t)), raw_out)
