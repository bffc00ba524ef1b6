"""GPU: RePaint resampling in replacement conditioning (DiffusionSampler.impute(resample, jump_length), impute_project(renoise_to),
fd_sampler_run_impute_repaint, fd_impute_project_renoise; the RENOISE variants of k_impute) against the float64 restatement of
tests/repaint_ref.py.

Shapes of the kernel tests: T = 24, 100, 187 (T no multiple of 16), C = 1, 5, 20 (C no multiple of 4: Philox groups straddle series
and rows; C > 16: two channel blocks), B = 3 (B T C no multiple of 4 at the odd shapes).  Every test prints what it measures before it
asserts."""
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
from tests import cfg_ref
from tests import impute_ref as I
from tests import repaint_ref as R
from tests.gpu_util import DEV, dev, host, make_model, oracle_sde, report_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
VP, VE = ("vp", (0.1, 20.0)), ("ve", (0.01, 2.0))
RJ = ((2, 1), (3, 2), (2, 5))
N = 8


def _sampler(m, bs):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    return DiffusionSampler(score_model=m, sample_batch_size=bs)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _u8(m):
    return torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8)).to(DEV)


def _project_c(x, x0, m_u8, per_series, std, fourier, G, alpha, s, z, seed=0, offset=0):
    from fourierdiffusion_amd import _C
    B, T, Cn = x.shape
    out = torch.empty_like(x)
    h = _C.ctx(x.device)
    _C.check(_C.lib().fd_impute_project(h, x.data_ptr(), x0.data_ptr(), m_u8.data_ptr(), int(per_series), _C.ptr(std), int(fourier),
                                        G.data_ptr(), float(alpha), float(s), _C.ptr(z), seed, offset, out.data_ptr(), B, T, Cn,
                                        _C.stream_of(x)), h)
    return out


def _project_renoise_c(x, x0, m_u8, per_series, std, fourier, G, alpha, s, z, a, b, z_re, seed=0, offset=0, offset_re=0):
    from fourierdiffusion_amd import _C
    B, T, Cn = x.shape
    out = torch.empty_like(x)
    h = _C.ctx(x.device)
    _C.check(_C.lib().fd_impute_project_renoise(h, x.data_ptr(), x0.data_ptr(), m_u8.data_ptr(), int(per_series), _C.ptr(std),
                                                int(fourier), G.data_ptr(), float(alpha), float(s), _C.ptr(z), seed, offset, float(a),
                                                float(b), _C.ptr(z_re), offset_re, out.data_ptr(), B, T, Cn, _C.stream_of(x)), h)
    return out


def _randn_dev(seed, offset, shape):
    """Standard normals of the engine's Philox stream: element e at counter offset + e/4 under `seed` (fd_prior_sample, VP, G = 1)."""
    from fourierdiffusion_amd import _C
    B, T, Cn = shape
    z = torch.empty(shape, device=DEV, dtype=torch.float32)
    h = _C.ctx(z.device)
    p = _C.SdeParams(0, 0.1, 20.0)
    _C.check(_C.lib().fd_prior_sample(h, C.byref(p), dev(np.ones(T)).data_ptr(), None, seed, offset, z.data_ptr(), B, T, Cn,
                                      _C.stream_of(z)), h)
    return z


def _levels():
    """(alpha, s, a, b) of the projection level and the transition back: VP and VE between two grid levels, and from the clean one."""
    out = {}
    for kind, p in (VP, VE):
        sde = O.SDEParams(kind, p[0], p[1], np.ones(4))
        ts, _ = O.timesteps(N)
        lo, hi = R.level_coef(sde, ts, 4), R.level_coef(sde, ts, 2)
        out[kind] = lo + R.transition_coef(lo, hi)
    sde = O.SDEParams("vp", 0.1, 20.0, np.ones(4))
    out["clean"] = (1.0, 0.0) + R.transition_coef((1.0, 0.0), R.level_coef(sde, O.timesteps(N)[0], N - 2))
    return out


# ------------------------------------------------------------------------------------------------ 1. the fused kernel alone
@pytest.mark.parametrize("T", [24, 100, 187])
def test_project_renoise_vs_float64(T):
    B, worst = 3, 0.0
    levels = _levels()
    for Cn in (1, 5, 20):
        rs = np.random.RandomState(T * 100 + Cn)
        x, z, zr, x0 = (rs.randn(B, T, Cn) for _ in range(4))
        sig = rs.uniform(0.5, 2.0, (T, Cn))
        masks = {True: rs.rand(B, T, Cn) < 0.5, False: rs.rand(T, Cn) < 0.5}
        xd, zd, zrd, x0d = dev(x), dev(z), dev(zr), dev(x0)
        for fourier in (True, False):
            for standardize in (True, False):
                sigma = sig if standardize else np.ones((T, Cn))
                std = dev(sigma) if standardize else None
                for scaling in (True, False):
                    G = O.noise_scaling(T, scaling).astype(np.float64)
                    Gd = dev(G)
                    for per_series, m in masks.items():
                        md = _u8(m)
                        for tag, (alpha, s, a, b) in levels.items():
                            # the coefficients as the engine receives them: float32
                            al, sf, af, bf = (float(np.float32(v)) for v in (alpha, s, a, b))
                            ref = R.project_renoise(x, x0, m, sigma, G, al, sf, z, af, bf, zr, fourier)
                            got = host(_project_renoise_c(xd, x0d, md, per_series, std, fourier, Gd, al, sf, zd, af, bf, zrd))
                            err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
                            worst = max(worst, err)
                            assert err <= 1e-5, (T, Cn, fourier, standardize, scaling, per_series, tag, err)
                        # a = 1, b = 0: the plain projection, to the bit
                        one = _project_renoise_c(xd, x0d, md, per_series, std, fourier, Gd, 0.7, 0.4, zd, 1.0, 0.0, zrd)
                        assert torch.equal(one, _project_c(xd, x0d, md, per_series, std, fourier, Gd, 0.7, 0.4, zd)), \
                            (T, Cn, fourier, standardize, scaling, per_series)
    print(f"fd_impute_project_renoise T={T}: worst max err / scale = {worst:.3e}")


def test_impute_project_renoise_to_public():
    """DiffusionSampler.impute_project(renoise_to=...) is the same launch with (a, b) of the scheduler's two levels."""
    cfg = CFG_TINY
    T, Cn, B = cfg["T"], cfg["C"], 3
    m_, sch, _ = make_model(cfg, precision="fp32")
    s = _sampler(m_, B)
    rs = np.random.RandomState(2)
    x, z, zr, x0 = (dev(rs.randn(B, T, Cn)) for _ in range(4))
    sig = dev(rs.uniform(0.5, 2.0, (T, Cn)))
    mk = rs.rand(B, T, Cn) < 0.5
    for t_lo, t_hi in ((0.3, 0.6), (None, 0.2)):
        lo = (1.0, 0.0) if t_lo is None else sch.marginal_coef(t_lo)
        a, b = R.transition_coef(lo, sch.marginal_coef(t_hi))
        pub = s.impute_project(x, x0, torch.from_numpy(mk), t_lo, fourier_transform=True, feature_std=sig, noise=z, renoise_to=t_hi,
                               renoise_noise=zr)
        raw = _project_renoise_c(x, x0, _u8(mk), True, sig, True, sch.G_on(x.device), lo[0], lo[1], z, a, b, zr)
        assert torch.equal(pub, raw)
    with pytest.raises(ValueError):
        s.impute_project(x, x0, torch.from_numpy(mk), 0.5, fourier_transform=True, renoise_to=0.2)       # backwards
    with pytest.raises(ValueError):
        s.impute_project(x, x0, torch.from_numpy(mk), 0.5, fourier_transform=True, renoise_noise=zr)     # nothing to re-noise


# ------------------------------------------------------------------------------------------------ 2. the re-noise Philox stream
@pytest.mark.parametrize("shape", [(5, 100, 12), (3, 37, 5)])
def test_renoise_philox_equals_injected(shape):
    B, T, Cn = shape
    seed, offset_re = 1234567, 4096
    rs = np.random.RandomState(7)
    x, x0, z, sig = dev(rs.randn(B, T, Cn)), dev(rs.randn(B, T, Cn)), dev(rs.randn(B, T, Cn)), dev(rs.uniform(0.5, 2.0, (T, Cn)))
    m = _u8(rs.rand(B, T, Cn) < 0.5)
    G = dev(O.noise_scaling(T, True))
    zre = _randn_dev(seed, offset_re, shape)
    for fourier in (True, False):
        a = _project_renoise_c(x, x0, m, True, sig, fourier, G, 0.6, 0.5, z, 0.8, 0.55, None, seed, 0, offset_re)
        b = _project_renoise_c(x, x0, m, True, sig, fourier, G, 0.6, 0.5, z, 0.8, 0.55, zre)
        assert torch.equal(a, b), fourier


# ------------------------------------------------------------------------------------------------ 3. trajectories vs float64
def _inputs(cfg, mask_kind, seed, B=4):
    rs = np.random.RandomState(seed)
    T, Cn = cfg["T"], cfg["C"]
    mu, sigma = 0.3 * rs.randn(T, Cn), rs.uniform(0.5, 2.0, (T, Cn))
    y = np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(B, T, Cn)
    if mask_kind == "random":
        m = rs.rand(*y.shape) < 0.5
    else:
        m = np.ones(y.shape, bool)
        m[:, -T // 4:] = False
    mu32, sig32 = mu.astype(np.float32).astype(np.float64), sigma.astype(np.float32).astype(np.float64)
    yn = np.where(m, y, np.nan).astype(np.float32)
    return mu32, sig32, y, yn, m


def _streams(tag, rows, T, Cn, r, j, n=N):
    E, K = R.counts(n, r, j)
    shape = (rows, T, Cn)
    zp = W.randn(f"rp_p_{tag}", shape, 1)
    zs = np.stack([W.randn(f"rp_z{i}_{tag}", shape, 1) for i in range(E)])
    zo = np.stack([W.randn(f"rp_o{i}_{tag}", shape, 1) for i in range(E)])
    zr = np.stack([W.randn(f"rp_r{i}_{tag}", shape, 1) for i in range(K)])
    return zp, zs, zo, zr


@pytest.mark.parametrize("name", ["tiny", "default"])
@pytest.mark.parametrize("kind,p", [VP, VE])
@pytest.mark.parametrize("mask_kind", ["random", "forecast"])
def test_trajectory_f32_vs_float64(name, kind, p, mask_kind):
    cfg = {"tiny": CFG_TINY, "default": dict(CFG_DEFAULT, L=2)}[name]
    T, Cn = cfg["T"], cfg["C"]
    mu, sigma, y, yn, m = _inputs(cfg, mask_kind, 11)
    B = y.shape[0]
    m_, sch, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    sampler = _sampler(m_, B)
    x0 = I.x0_obs(yn, m, mu, sigma, True)
    sde = oracle_sde(kind, p, True, T)
    for r, j in RJ:
        zp, zs, zo, zr = _streams(f"{name}_{r}_{j}", B, T, Cn, r, j)
        X = sampler.impute(torch.from_numpy(yn), torch.from_numpy(m), N, fourier_transform=True, feature_mean=_t(mu),
                           feature_std=_t(sigma), prior_noise=[dev(zp)], step_noise=[dev(zs)], obs_noise=[dev(zo)],
                           renoise_noise=[dev(zr)], resample=r, jump_length=j).numpy()
        ref = R.repaint_trajectory(sd, sde, zp, list(zs), list(zo), list(zr), x0, m, sigma, True, cfg["H"], resample=r, jump_length=j)
        err, _ = report_err(f"repaint f32 {name} {kind} {p[1]} {mask_kind} r={r} j={j}", X, ref)
        assert err <= 1e-4, (r, j, err)
        Ax = I.forward_map(X, mu, sigma, True)
        assert np.abs(Ax[m] - yn[m]).max() <= 1e-4 * max(1.0, np.abs(y).max()), (r, j)


# ------------------------------------------------------------------------------------------------ 4. the Philox layout of the loop
def _run_c(m, x_init, x0_obs, m_u8, per_series, std, fourier, n_steps, r, j, zs=None, zo=None, zr=None, seed=(0, 0), y=None, w=1.0,
           reps=1, pair_buffer=False):
    """fd_sampler_run_impute_repaint in place on a copy of x_init (pair_buffer: a NaN-filled (2B,T,C) buffer with x_init in its first
    half); returns the whole buffer."""
    from fourierdiffusion_amd import _C
    s = _sampler(m, x_init.shape[0])
    m.eval()
    Nn, ts_arr, dt = s._sde_grid(n_steps)
    ctx, h, p, Gd, mode = s._engine_args()
    rows = x_init.shape[0]
    buf = torch.full(((2 if pair_buffer else 1) * rows,) + tuple(x_init.shape[1:]), float("nan"), device=DEV)
    buf[:rows].copy_(x_init)
    yd = None if y is None else torch.tensor(y, dtype=torch.int32, device=DEV)
    rc = _C.lib().fd_sampler_run_impute_repaint(h, C.byref(p), Gd.data_ptr(), ts_arr, Nn, dt, buf.data_ptr(), x0_obs.data_ptr(),
                                                m_u8.data_ptr(), int(per_series), _C.ptr(std), int(fourier), _C.ptr(zs), _C.ptr(zo),
                                                seed[0], seed[1], rows, reps, mode, _C.ptr(yd), float(w), _C.ptr(zr), int(r), int(j),
                                                _C.stream_of(buf))
    _C.check(rc, ctx)
    return buf


@pytest.mark.parametrize("cfg,B", [(CFG_TINY, 3), (dict(T=37, C=5, D=24, L=2, H=4), 3)])
def test_philox_run_equals_injected_streams(cfg, B):
    """Predictor noise of executed step e at offset + e per, observation noise at offset + (E + e) per, re-noise k at
    offset + (2E + k) per, per = ceil(B T C / 4)."""
    T, Cn = cfg["T"], cfg["C"]
    n, r, j = 5, 2, 2
    E, K = R.counts(n, r, j)
    m_, sch, _ = make_model(cfg, precision="fp32")
    mu, sigma, y, yn, mk = _inputs(cfg, "random", 5, B)
    s = _sampler(m_, B)
    x0o = s.observed_to_sample_space(torch.from_numpy(yn), torch.from_numpy(mk), fourier_transform=True, feature_mean=_t(mu),
                                     feature_std=_t(sigma))
    xi = dev(W.randn("rp_phx", (B, T, Cn), 1))
    seed, offset = 0x5EED, 1 << 12
    per = (B * T * Cn + 3) // 4
    shape = (B, T, Cn)
    zs = torch.stack([_randn_dev(seed, offset + e * per, shape) for e in range(E)])
    zo = torch.stack([_randn_dev(seed, offset + (E + e) * per, shape) for e in range(E)])
    zr = torch.stack([_randn_dev(seed, offset + (2 * E + k) * per, shape) for k in range(K)])
    args = (m_, xi, x0o, _u8(mk), True, dev(sigma), True, n, r, j)
    a = _run_c(*args, seed=(seed, offset))
    b = _run_c(*args, zs=zs, zo=zo, zr=zr)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    # each stream on its own falls back to Philox at the same counters
    c = _run_c(*args, zs=zs, seed=(seed, offset))
    assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ 5. resample = 1 is today's call
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resample_one_is_the_plain_call(precision):
    cfg = dict(T=40, C=5, D=72, L=2, H=12)
    T, Cn, B = cfg["T"], cfg["C"], 6
    m_, _, _ = make_model(cfg, precision=precision)
    mu, sigma, y, yn, mk = _inputs(cfg, "random", 9, B)
    s = _sampler(m_, B)
    kw = dict(fourier_transform=True, feature_mean=_t(mu), feature_std=_t(sigma))
    outs = []
    for extra in ({}, dict(resample=1), dict(resample=1, jump_length=3), dict(jump_length=50)):
        torch.manual_seed(17)
        outs.append(s.impute(torch.from_numpy(yn), torch.from_numpy(mk), 7, **kw, **extra))
    assert torch.isfinite(outs[0]).all()
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    torch.manual_seed(17)
    assert not torch.equal(outs[0], s.impute(torch.from_numpy(yn), torch.from_numpy(mk), 7, resample=2, **kw))


# ------------------------------------------------------------------------------------------------ 6. ensembles and guidance
def test_ensemble_rows_read_their_own_observation():
    cfg = CFG_TINY
    T, Cn, n, Ke, r, j = cfg["T"], cfg["C"], 2, 3, 2, 3
    m_, sch, sd = make_model(cfg, precision="fp32")
    mu, sigma, y, yn, mk = _inputs(cfg, "random", 13, n)
    zp, zs, zo, zr = _streams("ens", n * Ke, T, Cn, r, j)
    X = _sampler(m_, n * Ke).impute(torch.from_numpy(yn), torch.from_numpy(mk), N, fourier_transform=True, feature_mean=_t(mu),
                                    feature_std=_t(sigma), prior_noise=[dev(zp)], step_noise=[dev(zs)], obs_noise=[dev(zo)],
                                    renoise_noise=[dev(zr)], num_samples=Ke, resample=r, jump_length=j)
    assert X.shape == (n, Ke, T, Cn)
    rep = np.repeat(np.arange(n), Ke)
    x0 = I.x0_obs(yn, mk, mu, sigma, True)[rep]
    ref = R.repaint_trajectory(sd, oracle_sde("vp", VP[1], True, T), zp, list(zs), list(zo), list(zr), x0, mk[rep], sigma, True,
                               cfg["H"], resample=r, jump_length=j)
    got = X.numpy().reshape(n * Ke, T, Cn)
    scale = max(1.0, np.abs(ref).max())
    for row in range(n * Ke):
        err = np.abs(got[row] - ref[row]).max() / scale
        print(f"repaint ensemble row {row} (series {rep[row]}): max err / scale = {err:.3e}")
        assert err <= 1e-4, (row, err)


def test_guided_pair_vs_float64():
    from tests.test_gpu_cfg import make_cond
    cfg = CFG_TINY
    T, Cn, B, r, j, w = cfg["T"], cfg["C"], 5, 2, 3, 1.5
    ylab = [0, 2, 1, 0, 2]
    m_, sch, sd, tab = make_cond(cfg, "fp32")
    mu, sigma, y, yn, mk = _inputs(cfg, "random", 15, B)
    zp, zs, zo, zr = _streams("cfg", B, T, Cn, r, j)
    x0 = I.x0_obs(yn, mk, mu, sigma, True)
    ref = R.repaint_trajectory(None, oracle_sde("vp", VP[1], True, T), zp, list(zs), list(zo), list(zr), x0, mk, sigma, True, cfg["H"],
                               resample=r, jump_length=j, score_fn=cfg_ref.guided_score_fn(sd, tab, ylab, w, cfg["H"]))
    s = _sampler(m_, 2 * B)
    kw = dict(fourier_transform=True, feature_mean=_t(mu), feature_std=_t(sigma))
    X = s.impute(torch.from_numpy(yn), torch.from_numpy(mk), N, prior_noise=[dev(zp)], step_noise=[dev(zs)], obs_noise=[dev(zo)],
                 renoise_noise=[dev(zr)], resample=r, jump_length=j, y=torch.tensor(ylab), cfg_scale=w, **kw)
    err, _ = report_err(f"repaint guided w={w} r={r} j={j}", X.numpy(), ref)
    assert err <= 1e-4, err
    # the same launch through the C entry point: both halves of the paired state, bit-equal
    x0p = s.observed_to_sample_space(torch.from_numpy(yn), torch.from_numpy(mk), **kw)
    xi = sch.prior_sampling((B, T, Cn), noise=dev(zp), device=torch.device(DEV))
    buf = _run_c(m_, xi, x0p, _u8(mk), True, dev(sigma), True, N, r, j, zs=dev(zs), zo=dev(zo), zr=dev(zr), y=ylab, w=w,
                 pair_buffer=True)
    assert torch.isfinite(buf).all() and torch.equal(buf[:B], buf[B:])
    assert torch.equal(buf[:B].cpu(), X)
    # without the transform: the RENOISE variant that writes both halves in phase 1
    x0t = s.observed_to_sample_space(torch.from_numpy(yn), torch.from_numpy(mk), fourier_transform=False)
    buf = _run_c(m_, xi, x0t, _u8(mk), True, None, False, N, r, j, zs=dev(zs), zo=dev(zo), zr=dev(zr), y=ylab, w=w, pair_buffer=True)
    assert torch.isfinite(buf).all() and torch.equal(buf[:B], buf[B:])


# ------------------------------------------------------------------------------------------------ 7. bf16 at the product shapes
def _bf16_case(cfg, B, n, r, j):
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
    torch.manual_seed(0)
    X = _sampler(m_, B).impute(yn, torch.from_numpy(m), n, fourier_transform=True, feature_mean=mean, feature_std=std, resample=r,
                               jump_length=j)
    assert torch.isfinite(X).all()                      # NaN at unobserved entries did not leak
    Ax = host(destandardize_idft(X.cuda(), mean.cuda(), std.cuda()))
    # the hard projection's residue is f32 transform rounding at the magnitude of the state it transforms: scale = max |A(x)|
    scale = max(1.0, np.abs(Ax).max(), np.abs(y).max())
    err = np.abs(Ax[m] - yn.numpy()[m]).max() / scale
    print(f"bf16 repaint T={T} C={Cn} B={B} r={r} j={j}: observed entries reproduced to {err:.3e} of scale {scale:.3e}")
    assert err <= 1e-4


def test_bf16_ecg_shape():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _bf16_case(dict(T=100, C=12, D=72, L=10, H=12), 2 * cus, 6, 2, 3)


def test_bf16_long_horizon():
    _bf16_case(dict(T=1024, C=16, D=72, L=10, H=12), 8, 6, 2, 3)


# ------------------------------------------------------------------------------------------------ 8. validation
def test_validation_errors():
    cfg = CFG_TINY
    T, Cn, B = cfg["T"], cfg["C"], 2
    m_, _, _ = make_model(cfg, precision="fp32")
    s = _sampler(m_, B)
    obs, mask = torch.zeros(B, T, Cn), torch.ones(B, T, Cn, dtype=torch.bool)
    E, K = R.counts(4, 2, 3)
    z = lambda k: [torch.zeros(k, B, T, Cn)]              # noqa: E731
    bad = [dict(conditioning="dps", resample=2), dict(resample=0), dict(resample=True), dict(resample=2.0), dict(resample="2"),
           dict(jump_length=0), dict(jump_length=False), dict(jump_length=1.5), dict(resample=2, jump_length=-1),
           dict(renoise_noise=z(K)),                                              # resample = 1 re-noises nothing
           dict(resample=2, jump_length=3, step_noise=z(4)),                      # E = 8 slots
           dict(resample=2, jump_length=3, step_noise=z(E), obs_noise=z(4)),
           dict(resample=2, jump_length=3, renoise_noise=z(K + 1)),
           dict(resample=2, jump_length=3, renoise_noise=z(E))]
    for kw in bad:
        with pytest.raises(ValueError):
            s.impute(obs, mask, 4, fourier_transform=True, **kw)
    # the right slot counts run
    X = s.impute(obs, mask, 4, fourier_transform=True, resample=2, jump_length=3, step_noise=z(E), obs_noise=z(E), renoise_noise=z(K))
    assert torch.isfinite(X).all()
    # the engine's own checks
    from fourierdiffusion_amd import _C
    x0 = torch.zeros(B, T, Cn, device=DEV)
    with pytest.raises(_C.FdError):
        _run_c(m_, x0, x0, _u8(np.ones((T, Cn))), False, None, True, 4, 0, 1)
    with pytest.raises(_C.FdError):
        _run_c(m_, x0, x0, _u8(np.ones((T, Cn))), False, None, True, 4, 2, 0)
    with pytest.raises(_C.FdError):                                               # labels on an unlabelled model
        _run_c(m_, x0, x0, _u8(np.ones((T, Cn))), False, None, True, 4, 2, 1, y=[0, 0], w=1.5, pair_buffer=True)


# ------------------------------------------------------------------------------------------------ 9. the command line
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_impute_resampled(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=rprun"], tmp_path)
    _run([str(ROOT / "cmd" / "impute.py"), "model_id=rprun", "num_diffusion_steps=6", "sampler.sample_batch_size=40",
          "mask.kind=forecast", "mask.horizon=6", "resample=2", "jump_length=3"], tmp_path)
    run_dir = tmp_path / "lightning_logs" / "rprun"
    X = torch.load(run_dir / "imputations.pt")
    assert X.shape == (96, 24, 4) and torch.isfinite(X).all()
    res = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert res["resample"] == 2 and res["jump_length"] == 3
    assert res["max_abs_err_observed"] <= 1e-3
