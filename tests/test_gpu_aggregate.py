"""GPU: conditioning on window means (DiffusionSampler.impute(aggregate=w) / fd_impute_project_agg / fd_sampler_run_impute_agg /
fd_impute_guidance_agg / fd_sampler_run_impute_dps_agg, an extension not in the reference) against the float64 restatement of
tests/aggregate_ref.py: the projection and one guidance evaluation at the shapes where the rectangular products change path,
trajectories under both conditionings, window = 1 against the mask entry points bit for bit, the all-false mask against sample(),
reproducibility and replication, bf16 at the ecg shape, and the CLI end to end.  Bounds are those of tests/test_gpu_impute.py and
tests/test_gpu_dps.py for the same quantities.  Measured errors are logged by tests/gpu_util.report_err."""
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
from tests import aggregate_ref as A
from tests import impute_ref as I
from tests import ode_ref
from tests.gpu_util import dev, host, log_line, make_model, oracle_sde, report_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _sampler(m, bs):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    return DiffusionSampler(score_model=m, sample_batch_size=bs)


def _inputs(T, Cn, B, w, seed, per_series=True, standardize=True, fourier=True, empty_row=False):
    """mu, sigma (f32-representable), window means y (NaN where hidden), the window mask, and x0_obs in float64."""
    rs = np.random.RandomState(seed)
    mu = (0.3 * rs.randn(T, Cn)).astype(np.float32).astype(np.float64)
    sigma = rs.uniform(0.5, 2.0, (T, Cn)).astype(np.float32).astype(np.float64)
    if not standardize:
        mu, sigma = np.zeros((T, Cn)), np.ones((T, Cn))
    J = A.n_windows(T, w)
    y = A.P(np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(B, T, Cn), w).astype(np.float32)
    m = rs.rand(B, J, Cn) < 0.6 if per_series else rs.rand(J, Cn) < 0.6
    if J == 1:
        m[...] = True          # a single window: observed (but for the emptied row below)
    if empty_row and per_series:
        m[0] = False
    yn = np.where(np.broadcast_to(m, y.shape), y, np.nan).astype(np.float32)
    return mu, sigma, yn, m, A.x0_obs(yn, m, mu, sigma, fourier, w)


# ---------------------------------------------------------------- the projection and one guidance evaluation
# (T, C, w): a short last window and windows that cross the 4-row quads; one window; odd T, two window tiles and a second channel
# block of one channel; nine window tiles on eight waves; a window that spans row tiles
SHAPES = [(20, 3, 3), (20, 3, 20), (37, 17, 2), (260, 5, 2), (130, 17, 24)]


@pytest.mark.parametrize("T,Cn,w", SHAPES)
def test_projection_and_guidance_against_float64(T, Cn, w):
    B, t = 3, float(np.float32(0.3))
    cfg = dict(T=T, C=Cn, D=8, L=1, H=4)
    m_, _, sd = make_model(cfg, precision="fp32")
    s = _sampler(m_, B)
    osde = oracle_sde("vp", (0.1, 20.0), True, T)
    score_fn = ode_ref.model_score(sd, "transformer", cfg["H"])
    x = W.randn(f"agg_x_{T}_{Cn}", (B, T, Cn), 0)
    z = W.randn(f"agg_z_{T}_{Cn}", (B, T, Cn), 1)
    score = score_fn(x.astype(np.float64), t)          # one float64 forward per shape, shared by every combination below
    t_proj = 0.35
    alpha, sdev = (float(np.float32(v)) for v in m_.noise_scheduler.marginal_coef(t_proj))      # (the engine takes them as floats)
    worst_p = worst_g = 0.0
    for fourier in (True, False):
        for standardize in (True, False):
            for per_series in (True, False):
                tag = f"T={T} C={Cn} w={w} fourier={fourier} std={standardize} per_series={per_series}"
                mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, w, T + w, per_series, standardize, fourier, empty_row=True)
                std = torch.from_numpy(sigma).float() if standardize else None
                mean = torch.from_numpy(mu).float() if standardize else None
                x0d = s.observed_to_sample_space(torch.from_numpy(yn), torch.from_numpy(mk), fourier_transform=fourier,
                                                 feature_mean=mean, feature_std=std, aggregate=w)
                assert np.abs(host(x0d) - x0).max() <= 1e-5 * max(1.0, np.abs(x0).max()), tag
                # the projection at the level of t_proj, from the float64 x0_obs so that its own rounding stays out
                got = host(s.impute_project(torch.from_numpy(x), dev(x0), torch.from_numpy(mk), t_proj, fourier_transform=fourier,
                                            feature_std=std, noise=dev(z), aggregate=w))
                ref = A.project(x, x0, mk, sigma, osde.G, alpha, sdev, z, fourier, w)
                err = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
                worst_p = max(worst_p, err)
                assert err <= 1e-5, (tag, err)
                # one Jacobian-free guidance evaluation
                g, rn2 = s.impute_guidance(torch.from_numpy(x), dev(x0), torch.from_numpy(mk), t, fourier_transform=fourier,
                                           feature_std=std, jacobian=False, aggregate=w)
                gr, rr, _ = A.guidance(score_fn, osde, x, t, x0, mk, sigma, fourier, w, jacobian=False, score=score)
                errg = float(np.abs(host(g) - gr).max() / np.abs(gr).max())
                worst_g = max(worst_g, errg)
                assert errg <= 1e-5, (tag, errg)
                np.testing.assert_allclose(rn2.cpu().numpy(), rr, rtol=1e-5, err_msg=tag)
                if per_series:       # the row without an observed window
                    assert float(rn2[0]) == 0.0 and rr[0] == 0.0 and not host(g)[0].any(), tag
    log_line(f"[parity] aggregate T={T} C={Cn} w={w}: projection worst {worst_p:.3e} of scale, guidance worst {worst_g:.3e} of max|g|")


# ---------------------------------------------------------------- trajectories
def _noise(tag, shape, N):
    zp = W.randn(f"aggt_p_{tag}", shape, 1)
    zs = np.stack([W.randn(f"aggt_z{i}_{tag}", shape, 1) for i in range(N)])
    zo = np.stack([W.randn(f"aggt_o{i}_{tag}", shape, 1) for i in range(N)])
    return zp, zs, zo


@pytest.mark.parametrize("kind,p", [("vp", (0.1, 20.0)), ("ve", (0.01, 2.0))])
def test_replace_trajectory_vs_float64(kind, p):
    cfg, N, B, w = CFG_TINY, 10, 3, 3
    T, Cn = cfg["T"], cfg["C"]
    m_, _, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, w, 11)
    zp, zs, zo = _noise(f"r_{kind}", (B, T, Cn), N)
    X = _sampler(m_, B).impute(torch.from_numpy(yn), torch.from_numpy(mk), N, fourier_transform=True,
                               feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
                               prior_noise=[dev(zp)], step_noise=[dev(zs)], obs_noise=[dev(zo)], aggregate=w).numpy()
    ref = A.impute_trajectory(sd, oracle_sde(kind, p, True, T), zp, list(zs), list(zo), x0, mk, sigma, True, cfg["H"], w)
    err, _ = report_err(f"aggregate replace f32 T={T} w={w} {kind}", X, ref)
    assert np.isfinite(X).all() and err <= 1e-4, err
    got = A.P(I.forward_map(X, mu, sigma, True), w)
    dev_y = float(np.abs(got[mk] - yn[mk]).max())
    print(f"aggregate replace {kind}: observed window means reproduced to {dev_y:.3e}")
    assert dev_y <= 1e-4 * max(1.0, float(np.abs(yn[mk]).max()))


@pytest.mark.parametrize("kind,p,jacobian", [("vp", (0.1, 20.0), False), ("ve", (0.01, 2.0), False), ("vp", (0.1, 20.0), True)])
def test_dps_trajectory_vs_float64(kind, p, jacobian):
    cfg, N, B, w, zeta = CFG_TINY, 10, 3, 3, 0.3
    T, Cn = cfg["T"], cfg["C"]
    m_, _, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, w, 13)
    zp, zs, _ = _noise(f"d_{kind}_{jacobian}", (B, T, Cn), N)
    X = _sampler(m_, B).impute(torch.from_numpy(yn), torch.from_numpy(mk), N, fourier_transform=True,
                               feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
                               prior_noise=[dev(zp)], step_noise=[dev(zs)], conditioning="dps", guidance_scale=zeta,
                               guidance_jacobian=jacobian, aggregate=w).numpy()
    ref = A.trajectory(ode_ref.model_score(sd, "transformer", cfg["H"]), oracle_sde(kind, p, True, T), zp, list(zs), x0, mk, sigma,
                       True, zeta, w, jacobian)
    err, _ = report_err(f"aggregate dps f32 T={T} w={w} {kind} jacobian={jacobian}", X, ref)
    assert np.isfinite(X).all() and err <= 1e-5, err


# ---------------------------------------------------------------- window = 1 is the mask path, bit for bit
def test_window_one_is_bit_identical():
    from fourierdiffusion_amd import _C
    cfg, B, N = CFG_TINY, 4, 5
    T, Cn = cfg["T"], cfg["C"]
    m_, _, _ = make_model(cfg, precision="fp32")
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, 1, 3)
    s = _sampler(m_, B)
    x, z, x0d, std = dev(W.randn("agg1_x", (B, T, Cn), 0)), dev(W.randn("agg1_z", (B, T, Cn), 1)), dev(x0), dev(sigma)
    m_u8 = torch.from_numpy(mk.astype(np.uint8)).cuda()
    G = m_.noise_scheduler.G_on(x.device)
    ctx, h, p, _, mode = s._engine_args()
    for fourier in (1, 0):
        a, b = torch.empty_like(x), torch.empty_like(x)
        _C.check(_C.lib().fd_impute_project(ctx, x.data_ptr(), x0d.data_ptr(), m_u8.data_ptr(), 1, std.data_ptr(), fourier, G.data_ptr(),
                                            0.7, 0.4, z.data_ptr(), 0, 0, a.data_ptr(), B, T, Cn, _C.stream_of(x)), ctx)
        _C.check(_C.lib().fd_impute_project_agg(ctx, x.data_ptr(), x0d.data_ptr(), m_u8.data_ptr(), 1, std.data_ptr(), fourier,
                                                G.data_ptr(), 0.7, 0.4, z.data_ptr(), 0, 0, b.data_ptr(), B, T, Cn, 1,
                                                _C.stream_of(x)), ctx)
        assert torch.isfinite(a).all() and torch.equal(a, b), fourier
        for jac in (1, 0):
            res = []
            for agg in (False, True):
                g, rn2 = torch.empty_like(x), torch.empty(B, dtype=torch.float64, device=x.device)
                head = (h, C.byref(p), G.data_ptr(), 0.4, x.data_ptr(), x0d.data_ptr(), m_u8.data_ptr(), 1, std.data_ptr(), fourier, jac,
                        g.data_ptr(), rn2.data_ptr(), B, 1)
                rc = (_C.lib().fd_impute_guidance_agg(*head, 1, mode, _C.stream_of(x)) if agg
                      else _C.lib().fd_impute_guidance(*head, mode, _C.stream_of(x)))
                _C.check(rc, ctx)
                res.append((g, rn2))
            assert torch.isfinite(res[0][0]).all() and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    # window outside [1, T]: FD_ERR_ARG
    for bad in (0, -3, T + 1):
        rc = _C.lib().fd_impute_project_agg(ctx, x.data_ptr(), x0d.data_ptr(), m_u8.data_ptr(), 1, std.data_ptr(), 1, G.data_ptr(),
                                            0.7, 0.4, z.data_ptr(), 0, 0, a.data_ptr(), B, T, Cn, bad, _C.stream_of(x))
        assert rc == -1, (bad, rc)          # FD_ERR_ARG
    # a 5-step impute
    zp, zs, zo = _noise("one", (B, T, Cn), N)
    kw = dict(fourier_transform=True, feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
              prior_noise=[dev(zp)], step_noise=[dev(zs)])
    obs, mask = torch.from_numpy(yn), torch.from_numpy(mk)
    for extra in (dict(obs_noise=[dev(zo)]), dict(conditioning="dps", guidance_scale=0.3, guidance_jacobian=False)):
        a = s.impute(obs, mask, N, **kw, **extra)
        b = s.impute(obs, mask, N, aggregate=1, **kw, **extra)
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---------------------------------------------------------------- the all-false window mask is the plain sampler
def test_zero_window_mask_equals_sample(monkeypatch):
    monkeypatch.setenv("FDIFF_SAMPLER_STEPWISE", "1")
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg, n, N, w = dict(T=40, C=5, D=24, L=2, H=4), 8, 15, 4
    m_, _, _ = make_model(cfg, precision="fp32")
    sampler = DiffusionSampler(score_model=m_, sample_batch_size=n, merge_batches=False)
    rs = np.random.RandomState(0)
    std = torch.from_numpy(rs.uniform(0.5, 2, (40, 5))).float()
    for fourier in (True, False):
        torch.manual_seed(3)
        Xs = sampler.sample(num_samples=n, num_diffusion_steps=N)
        torch.manual_seed(3)
        Xi = sampler.impute(torch.from_numpy(rs.randn(n, 10, 5)).float(), torch.zeros(10, 5, dtype=torch.bool), N,
                            fourier_transform=fourier, feature_mean=torch.zeros(40, 5), feature_std=std, aggregate=w)
        assert torch.isfinite(Xs).all()
        assert ((Xi - Xs.cpu()).abs().max() / Xs.abs().max()).item() <= 1e-6, fourier


# ---------------------------------------------------------------- reproducibility, replication, Philox
def test_reproducible_and_replicated():
    cfg, n, K, N, w = dict(T=40, C=5, D=24, L=2, H=4), 4, 3, 6, 3
    T, Cn = cfg["T"], cfg["C"]
    m_, _, _ = make_model(cfg, precision="fp32")
    mu, sigma, yn, mk, _ = _inputs(T, Cn, n, w, 7)
    obs, mask = torch.from_numpy(yn), torch.from_numpy(mk)
    s = _sampler(m_, n * K)
    shape = (n * K, T, Cn)
    zp, zs, zo = _noise("rep", shape, N)
    for fourier in (True, False):
        kw = dict(fourier_transform=fourier, feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
                  aggregate=w)
        for extra in (dict(), dict(conditioning="dps", guidance_scale=0.5, guidance_jacobian=False),
                      dict(conditioning="dps", guidance_scale=0.5, guidance_jacobian=True)):
            torch.manual_seed(9)
            a = s.impute(obs, mask, N, **kw, **extra)
            torch.manual_seed(9)
            b = s.impute(obs, mask, N, **kw, **extra)
            assert torch.isfinite(a).all() and torch.equal(a, b), (fourier, extra)
            # replicas read one observation in place: bit-identical to repeat_interleave'd observations under the same noise
            inj = dict(prior_noise=[dev(zp)], step_noise=[dev(zs)])
            if not extra:
                inj.update(obs_noise=[dev(zo)])
            rep = s.impute(obs, mask, N, num_samples=K, **inj, **kw, **extra)
            big = s.impute(obs.repeat_interleave(K, 0), mask.repeat_interleave(K, 0), N, **inj, **kw, **extra)
            assert rep.shape == (n, K, T, Cn) and torch.equal(rep.reshape(n * K, T, Cn), big), (fourier, extra)


def test_project_philox_equals_injected():
    """z = NULL draws element e at counter offset + e/4 under `seed`, as fd_impute_project: fd_prior_sample (VP, G = 1) has that layout."""
    from fourierdiffusion_amd import _C
    B, T, Cn, w, seed, offset = 5, 100, 12, 4, 1234567, 4096
    J = A.n_windows(T, w)
    rs = np.random.RandomState(7)
    x, x0, sig = dev(rs.randn(B, T, Cn)), dev(rs.randn(B, T, Cn)), dev(rs.uniform(0.5, 2.0, (T, Cn)))
    m = torch.from_numpy((rs.rand(B, J, Cn) < 0.5).astype(np.uint8)).cuda()
    G = dev(O.noise_scaling(T, True))
    z = torch.empty_like(x)
    h = _C.ctx(x.device)
    p = _C.SdeParams(0, 0.1, 20.0)
    _C.check(_C.lib().fd_prior_sample(h, C.byref(p), dev(np.ones(T)).data_ptr(), None, seed, offset, z.data_ptr(), B, T, Cn,
                                      _C.stream_of(x)), h)
    for fourier in (1, 0):
        outs = []
        for zz, sd, off in ((None, seed, offset), (z, 0, 0)):
            out = torch.empty_like(x)
            _C.check(_C.lib().fd_impute_project_agg(h, x.data_ptr(), x0.data_ptr(), m.data_ptr(), 1, sig.data_ptr(), fourier, G.data_ptr(),
                                                    0.6, 0.5, _C.ptr(zz), sd, off, out.data_ptr(), B, T, Cn, w, _C.stream_of(x)), h)
            outs.append(out)
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], x), fourier


# ---------------------------------------------------------------- bf16 at the ecg shape
def test_bf16_ecg_shape():
    cfg, B, N, w = CFG_DEFAULT, 64, 10, 4
    T, Cn = cfg["T"], cfg["C"]
    mb, _, _ = make_model(cfg, precision="bf16")
    mu, sigma, yn, mk, _ = _inputs(T, Cn, B, w, 5)
    kw = dict(fourier_transform=True, feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
              aggregate=w)
    for extra in (dict(), dict(conditioning="dps", guidance_scale=1.0, guidance_jacobian=False)):
        torch.manual_seed(1)
        X = _sampler(mb, B).impute(torch.from_numpy(yn), torch.from_numpy(mk), N, **kw, **extra)
        assert X.shape == (B, T, Cn) and torch.isfinite(X).all(), extra


# ---------------------------------------------------------------- CLI
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_impute_aggregate(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=aggrun"], tmp_path)
    _run([str(ROOT / "cmd" / "impute.py"), "model_id=aggrun", "num_diffusion_steps=10", "sampler.sample_batch_size=40",
          "aggregate=4", "mask.kind=forecast", "mask.horizon=2"], tmp_path)
    run_dir = tmp_path / "lightning_logs" / "aggrun"
    X = torch.load(run_dir / "imputations.pt")
    assert X.shape == (96, 24, 4) and torch.isfinite(X).all()
    res = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert res["aggregate"] == 4 and res["mask_kind"] == "forecast" and res["hidden_fraction"] == 1.0
    assert np.isfinite(res["mse_hidden"]) and np.isfinite(res["mae_hidden"])
    assert res["max_abs_err_window_means"] <= 1e-3
