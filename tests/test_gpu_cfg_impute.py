"""GPU: labels and classifier-free guidance in conditional sampling and the likelihood (DiffusionSampler.impute / impute_guidance /
log_likelihood with y and cfg_scale; fd_sampler_run_impute_cfg, fd_impute_guidance_cfg, fd_sampler_run_impute_dps_cfg; the PAIR forms
of k_impute, k_dps_residual and k_dps_step) against the float64 restatement of tests/cfg_impute_ref.py.

Shapes: cfg_ref.CFG (T = 24, C = 4: 16-byte path, on-device noise possible), cfg_ref.CFG_TAIL (T = 21, C = 3: Tp padding, scalar tail,
Philox groups straddling rows) and T = 8, C = 20 (two channel blocks), d_model 72, 12 heads, 2 layers; K = 3 classes, B = 5, 8 steps,
fp32, injected noise wherever float64 is compared.  The eight-step DPS trajectory WITH the Jacobian runs at T = 8, C = 3, d_model 8
(the likelihood shape): its float64 reference takes 2 T C oracle evaluations of the guided score per step, 36 s at T = 21, and the
sum of the two halves of the VJP is already held to float64 at the two larger shapes by the one-evaluation test; a two-step
trajectory with the Jacobian at T = 21, C = 3 runs the paired step on its own output on the tail shape.

Every test prints what it measures before it asserts.  One margin is recorded (DESIGN 3.19 has the same and lists the rest as owed):
replace, T = 24, C = 4, Fourier + standardised, random mask, w = 1.7: composition vs float64 1.9e-7, fused vs float64 1.6e-7, fused
vs composition 1.4e-7.  No other figure measured on the GPU is recorded yet.
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from oracle import weights as W
from tests import cfg_impute_ref as G
from tests import cfg_ref as R
from tests import likelihood_ref as L
from tests import ode_ref
from tests.gpu_util import DEV, dev, host, oracle_sde, report_err
from tests.test_gpu_cfg import make_cond

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K, B, N = R.K, R.B, R.N_STEPS
VP = ("vp", (0.1, 20.0))
WG = G.W_GUIDE
SHAPES = {"T24C4": R.CFG, "T21C3": R.CFG_TAIL, "T8C20": G.CFG_WIDE}


def _sampler(m, bs=B):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    return DiffusionSampler(score_model=m, sample_batch_size=bs)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _noise(tag, T, Cn, rows=B, steps=N):
    zp = W.randn(f"ci_p_{tag}", (rows, T, Cn), 21)
    zs = W.randn(f"ci_s_{tag}", (steps, rows, T, Cn), 21)
    zo = W.randn(f"ci_o_{tag}", (steps, rows, T, Cn), 21)
    return zp, zs, zo


def _kw(mu, sigma, fourier, standardize):
    kw = dict(fourier_transform=fourier)
    if standardize:
        kw.update(feature_mean=_t(mu), feature_std=_t(sigma))
    return kw


class _env:
    """FDIFF_CFG_FORCE_PAIR set (or cleared) for a block."""

    def __init__(self, force):
        self.force = force

    def __enter__(self):
        self.old = os.environ.pop("FDIFF_CFG_FORCE_PAIR", None)
        if self.force:
            os.environ["FDIFF_CFG_FORCE_PAIR"] = "1"

    def __exit__(self, *a):
        os.environ.pop("FDIFF_CFG_FORCE_PAIR", None)
        if self.old is not None:
            os.environ["FDIFF_CFG_FORCE_PAIR"] = self.old


def _bound(m, y):
    """Context: y bound on the model through fd_score_set_labels (the unpaired entry points then read them)."""
    ctx, h = m._engine()
    yd = torch.tensor(y, dtype=torch.int32, device=DEV)
    return m._labels_bound(h, ctx, yd)


def run_impute_cfg(m, x0, x0_obs, m_u8, per_series, std, fourier, y, w, zs, zo, force_pair=False, seed=(0, 0), entry="cfg", reps=1):
    """fd_sampler_run_impute_cfg (or, entry="rep", fd_sampler_run_impute_rep) on a NaN-filled (2B,T,C) buffer whose first half is x0;
    returns the whole buffer."""
    from fourierdiffusion_amd import _C
    s = _sampler(m)
    m.eval()
    Nn, ts_arr, dt = s._sde_grid(N)
    ctx, h, p, Gd, mode = s._engine_args()
    rows = x0.shape[0]
    buf = torch.full((2 * rows,) + tuple(x0.shape[1:]), float("nan"), device=DEV)
    buf[:rows].copy_(x0)
    yd = None if y is None else torch.tensor(y, dtype=torch.int32, device=DEV)
    args = [h, C.byref(p), Gd.data_ptr(), ts_arr, Nn, dt, buf.data_ptr(), x0_obs.data_ptr(), m_u8.data_ptr(), int(per_series),
            _C.ptr(std), int(fourier), _C.ptr(zs), _C.ptr(zo), seed[0], seed[1], rows, reps, mode]
    with _env(force_pair):
        if entry == "rep":
            rc = _C.lib().fd_sampler_run_impute_rep(*args, _C.stream_of(buf))
        else:
            rc = _C.lib().fd_sampler_run_impute_cfg(*args, _C.ptr(yd), float(w), _C.stream_of(buf))
    _C.check(rc, ctx)
    return buf


def compose_replace(m, sch, s, x0, x0_obs, mask, std, fourier, y, w, zs, zo):
    """The host loop over the public pieces: forward on 2B rows with [y ; null], the combine in torch fp32, noise_scheduler.step,
    impute_project at t_{i+1} (the last one exact)."""
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    m.eval()
    sch.set_timesteps(N)
    w32 = torch.tensor(np.float32(w), device=DEV)
    omw32 = torch.tensor(np.float32(1.0 - float(np.float32(w))), device=DEV)
    rows = x0.shape[0]
    y2 = torch.tensor(list(y) + [K] * rows)
    ts = sch.timesteps.tolist()
    x = x0.clone()
    for i, tt in enumerate(ts):
        t2 = torch.full((2 * rows,), tt, device=DEV, dtype=torch.float32)
        s2 = m(DiffusableBatch(X=torch.cat([x, x]).contiguous(), y=y2, timesteps=t2))
        sc = w32 * s2[:rows] + omw32 * s2[rows:]
        x = sch.step(model_output=sc.contiguous(), timestep=tt, sample=x, noise=zs[i]).prev_sample
        last = i + 1 == len(ts)
        x = s.impute_project(x, x0_obs, mask, None if last else ts[i + 1], fourier_transform=fourier, feature_std=std,
                             noise=None if last else zo[i])
    return x


# ------------------------------------------------------------------------------------------------------------------ 1. replace
@pytest.mark.parametrize("mask_kind", ["random", "forecast"])
@pytest.mark.parametrize("domain", ["fourier_std", "time"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_replace_fused_vs_float64_and_composition(shape, domain, mask_kind):
    cfg = SHAPES[shape]
    T, Cn = cfg["T"], cfg["C"]
    fourier = standardize = domain == "fourier_std"
    m, sch, sd, tab = make_cond(cfg, "fp32")
    s = _sampler(m)
    mu, sigma, yn, mk, x0o = G.conditioning(T, Cn, B, mask_kind, 31, fourier, standardize)
    zp, zs, zo = _noise(shape, T, Cn)
    sde = oracle_sde("vp", VP[1], True, T)
    w = float(np.float32(WG))
    ref = G.replace_trajectory(sd, tab, sde, zp, list(zs), list(zo), x0o, mk, sigma, fourier, G.Y_CLASSES, w, cfg["H"])
    x0 = sch.prior_sampling((B, T, Cn), noise=dev(zp), device=torch.device(DEV))
    maskt = torch.from_numpy(mk)
    m_u8, per_series = s._mask_u8(maskt, B, T, Cn, DEV)
    std = dev(sigma) if standardize else None
    zsd, zod = dev(zs), dev(zo)
    buf = run_impute_cfg(m, x0, dev(x0o), m_u8, per_series, std, fourier, G.Y_CLASSES, WG, zsd, zod)
    comp = host(compose_replace(m, sch, s, x0, dev(x0o), maskt, std, fourier, G.Y_CLASSES, WG, zsd, zod))
    fused = host(buf[:B])
    scale = max(1.0, np.abs(ref).max())
    e_comp, e_fused, e_pair = (np.abs(a - b).max() / scale for a, b in ((comp, ref), (fused, ref), (fused, comp)))
    print(f"[cfg-impute] replace {shape} {domain} {mask_kind} w=1.7: composition vs float64 {e_comp:.3e}, fused vs float64 "
          f"{e_fused:.3e}, fused vs composition {e_pair:.3e} (of max(1, max |x|))")
    assert e_fused <= 1e-4, e_fused                               # tests/test_gpu_impute.py, unguided trajectories
    assert e_pair <= 4 * e_comp, (e_pair, e_comp)                  # tests/test_gpu_cfg.py
    assert torch.equal(buf[:B], buf[B:])
    # the public call is the same launch (a paired launch holds sample_batch_size // 2 series)
    pub = _sampler(m, 2 * B).impute(_t(yn), maskt, N, prior_noise=[dev(zp)], step_noise=[zsd], obs_noise=[zod], y=torch.tensor(G.Y_CLASSES),
                   cfg_scale=WG, **_kw(mu, sigma, fourier, standardize))
    x0p = s.observed_to_sample_space(_t(yn), maskt, **_kw(mu, sigma, fourier, standardize))      # (fp32 transform of the observations)
    bufp = run_impute_cfg(m, x0, x0p, m_u8, per_series, std, fourier, G.Y_CLASSES, WG, zsd, zod)
    assert torch.equal(pub, bufp[:B].cpu())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_replace_forced_pair_equals_one_evaluation(shape):
    cfg = SHAPES[shape]
    T, Cn = cfg["T"], cfg["C"]
    m, sch, _, _ = make_cond(cfg, "fp32")
    s = _sampler(m)
    mu, sigma, yn, mk, x0o = G.conditioning(T, Cn, B, "random", 32, True)
    zp, zs, zo = _noise(shape + "fp", T, Cn)
    x0 = sch.prior_sampling((B, T, Cn), noise=dev(zp), device=torch.device(DEV))
    m_u8, per_series = s._mask_u8(torch.from_numpy(mk), B, T, Cn, DEV)
    args = (m, x0, dev(x0o), m_u8, per_series, dev(sigma), True)
    noises = [(dev(zs), dev(zo), (0, 0))] + ([(None, None, (0x5EED, 1 << 12))] if (T * Cn) % 4 == 0 and shape == "T24C4" else [])
    for zsd, zod, seed in noises:
        for wx in (1.0, 0.0):
            pair = run_impute_cfg(*args, G.Y_MIXED, wx, zsd, zod, force_pair=True, seed=seed)
            one = run_impute_cfg(*args, G.Y_MIXED, wx, zsd, zod, seed=seed)
            assert torch.equal(pair[:B], pair[B:]) and torch.isfinite(pair).all()
            assert torch.isnan(one[B:]).all()                     # the one-evaluation form never touches a second half
            assert torch.equal(pair[:B], one[:B]), (wx, seed)
        # w = 1, one evaluation: fd_sampler_run_impute_rep with the same labels bound
        one = run_impute_cfg(*args, G.Y_MIXED, 1.0, zsd, zod, seed=seed)
        with _bound(m, G.Y_MIXED):
            rep = run_impute_cfg(*args, None, 1.0, zsd, zod, seed=seed, entry="rep")
        assert torch.equal(one[:B], rep[:B]), seed
        # and w = 0 is the model with nothing bound
        zero = run_impute_cfg(*args, G.Y_MIXED, 0.0, zsd, zod, seed=seed)
        rep0 = run_impute_cfg(*args, None, 1.0, zsd, zod, seed=seed, entry="rep")
        assert torch.equal(zero[:B], rep0[:B]) and not torch.equal(zero[:B], one[:B])


def test_replace_defaults_unchanged_and_ensembles():
    cfg = R.CFG
    T, Cn = cfg["T"], cfg["C"]
    m, _, _, _ = make_cond(cfg, "bf16")
    mu, sigma, yn, mk, _ = G.conditioning(T, Cn, B, "random", 33, True)
    obs, mask = _t(yn), torch.from_numpy(mk)
    kw = _kw(mu, sigma, True, True)
    s = _sampler(m, 6 * B)
    outs = []
    for extra in ({}, dict(y=None, cfg_scale=1.0)):
        for cond in ("replace", "dps"):
            torch.manual_seed(13)
            outs.append(s.impute(obs, mask, N, conditioning=cond, **kw, **extra))
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]) and torch.isfinite(outs[0]).all()
    # ensembles: K rows of a series share its label, bit-identical to repeat_interleave'd observations and labels as plain rows
    Ke = 3
    zp, zs, zo = _noise("ens", T, Cn, rows=B * Ke)
    y = torch.tensor(G.Y_MIXED)
    for cond, wx in (("replace", WG), ("dps", WG), ("replace", 1.0)):
        nz = dict(prior_noise=[dev(zp)], step_noise=[dev(zs)], conditioning=cond, **({} if cond == "dps" else dict(obs_noise=[dev(zo)])))
        ens = s.impute(obs, mask, N, num_samples=Ke, y=y, cfg_scale=wx, **nz, **kw)
        big = s.impute(obs.repeat_interleave(Ke, 0), mask.repeat_interleave(Ke, 0), N, y=y.repeat_interleave(Ke), cfg_scale=wx, **nz, **kw)
        assert ens.shape == (B, Ke, T, Cn) and torch.isfinite(ens).all()
        assert torch.equal(ens.reshape(B * Ke, T, Cn), big), (cond, wx)
    # a paired call holds sample_batch_size // (2 K) series per launch: two launches here, one Philox key each, finite, reproducible
    s2 = _sampler(m, 4 * Ke)
    res = []
    for _ in range(2):
        torch.manual_seed(14)
        res.append(s2.impute(obs, mask, N, num_samples=Ke, y=y, cfg_scale=2.0, **kw))
    assert res[0].shape == (B, Ke, T, Cn) and torch.isfinite(res[0]).all() and torch.equal(res[0], res[1])


# ---------------------------------------------------------------------------------------------------------------------- 2. dps
def _dps_setup(cfg, seed, label_dropout=0.0):
    T, Cn = cfg["T"], cfg["C"]
    m, sch, sd, tab = make_cond(cfg, "fp32", label_dropout=label_dropout)
    mu, sigma, yn, mk, x0o = G.conditioning(T, Cn, B, "random", seed, True)
    return m, sch, sd, tab, mu, sigma, yn, mk, x0o


@pytest.mark.parametrize("t", [0.7, 0.3, 0.05])
@pytest.mark.parametrize("shape", ["T24C4", "T21C3"])
def test_dps_guidance_vs_float64(shape, t):
    cfg = SHAPES[shape]
    T, Cn = cfg["T"], cfg["C"]
    m, sch, sd, tab, mu, sigma, yn, mk, x0o = _dps_setup(cfg, 34)
    s = _sampler(m)
    sde = oracle_sde("vp", VP[1], True, T)
    x = W.randn(f"ci_gx_{shape}_{t}", (B, T, Cn), 22)
    t32, w = float(np.float32(t)), float(np.float32(WG))
    y = torch.tensor(G.Y_MIXED)
    for jac in (True, False):
        g, rn2 = s.impute_guidance(_t(x), dev(x0o), torch.from_numpy(mk), t32, fourier_transform=True, feature_std=_t(sigma),
                                   jacobian=jac, y=y, cfg_scale=WG)
        gr, rr = G.dps_guidance(sd, tab, sde, x, t32, x0o, mk, sigma, True, G.Y_MIXED, w, cfg["H"], jac)
        err, _ = report_err(f"cfg dps guidance fp32 {shape} t={t} jacobian={jac} w=1.7", host(g), gr)
        assert err <= 1e-5, (jac, err)                            # tests/test_gpu_dps.py
        np.testing.assert_allclose(rn2.cpu().numpy(), rr, rtol=1e-5)
        if not jac:
            continue
        # forced pair at w = 1 / w = 0 with the Jacobian: the summed halves change the rounding, so the same bound
        for wx in (1.0, 0.0):
            with _env(True):
                gp, _ = s.impute_guidance(_t(x), dev(x0o), torch.from_numpy(mk), t32, fourier_transform=True, feature_std=_t(sigma),
                                          jacobian=True, y=y, cfg_scale=wx)
            gr1, _ = G.dps_guidance(sd, tab, sde, x, t32, x0o, mk, sigma, True, G.Y_MIXED, wx, cfg["H"], True)
            err, _ = report_err(f"cfg dps guidance fp32 {shape} t={t} forced pair w={wx}", host(gp), gr1)
            assert err <= 1e-5, (wx, err)


def _dps_traj(cfg, tag, jac, y, w, seed=35, steps=N):
    T, Cn = cfg["T"], cfg["C"]
    m, sch, sd, tab, mu, sigma, yn, mk, x0o = _dps_setup(cfg, seed)
    zp, zs, _ = _noise(tag, T, Cn, steps=steps)
    X = _sampler(m, 2 * B).impute(_t(yn), torch.from_numpy(mk), steps, prior_noise=[dev(zp)], step_noise=[dev(zs)], conditioning="dps",
                           guidance_scale=0.3, guidance_jacobian=jac, y=None if y is None else torch.tensor(y), cfg_scale=w,
                           **_kw(mu, sigma, True, True)).numpy()
    ref = G.dps_trajectory(sd, tab, oracle_sde("vp", VP[1], True, T), zp, list(zs), x0o, mk, sigma, True, 0.3, y,
                           float(np.float32(w)), cfg["H"], jac)
    assert np.isfinite(X).all()
    return report_err(f"cfg dps trajectory f32 T={T} C={Cn} steps={steps} jacobian={jac} y={'set' if y else 'none'} w={w}", X, ref)[0]


@pytest.mark.parametrize("shape,jac", [("T24C4", False), ("T21C3", False), ("T8C3", True)])
def test_dps_trajectory_vs_float64(shape, jac):
    cfg = dict(G.CFG_LL) if shape == "T8C3" else SHAPES[shape]
    err = _dps_traj(cfg, f"dt_{shape}", jac, G.Y_CLASSES, WG)
    if err > 1e-5:      # the issue's rule: is it the unguided loop's own kink-crossing?  Printed for the record.
        print(f"[cfg-impute] unguided loop on the same inputs: {_dps_traj(cfg, f'dt_{shape}', jac, None, 1.0):.3e}")
    assert err <= 1e-5, err                                       # tests/test_gpu_dps.py


def test_dps_short_jacobian_trajectory_on_the_tail_shape():
    """k_dps_step<GRAD, PAIR> fed by its own output, WITH the Jacobian, where T has a Tp tail, the scalar path runs and Philox groups
    straddle rows (T = 21, C = 3): two steps, which is what the float64 reference (2 T C guided oracle evaluations per step) allows
    in a few seconds.  The second step reads the state that the first wrote to both halves."""
    err = _dps_traj(SHAPES["T21C3"], "dtj_T21C3", True, G.Y_CLASSES, WG, steps=2)
    assert err <= 1e-5, err                                       # tests/test_gpu_dps.py


@pytest.mark.parametrize("shape", ["T24C4", "T21C3"])
def test_dps_forced_pair_equals_the_bound_unpaired_path(shape):
    cfg = SHAPES[shape]
    T, Cn = cfg["T"], cfg["C"]
    m, sch, sd, tab, mu, sigma, yn, mk, x0o = _dps_setup(cfg, 36)
    s = _sampler(m, 2 * B)
    zp, zs, _ = _noise(f"dfp_{shape}", T, Cn)
    obs, mask = _t(yn), torch.from_numpy(mk)
    kw = dict(prior_noise=[dev(zp)], step_noise=[dev(zs)], conditioning="dps", guidance_scale=0.3, guidance_jacobian=False,
              **_kw(mu, sigma, True, True))
    y = torch.tensor(G.Y_MIXED)
    x = W.randn(f"ci_fx_{shape}", (B, T, Cn), 23)
    gkw = dict(fourier_transform=True, feature_std=_t(sigma), jacobian=False)
    for wx in (1.0, 0.0):
        with _env(True):
            pair = s.impute(obs, mask, N, y=y, cfg_scale=wx, **kw)
            gp, rp = s.impute_guidance(_t(x), dev(x0o), mask, 0.3, y=y, cfg_scale=wx, **gkw)
        one = s.impute(obs, mask, N, y=y, cfg_scale=wx, **kw)
        if wx == 1.0:
            with _bound(m, G.Y_MIXED):
                ref = s.impute(obs, mask, N, **kw)
                gu, ru = s.impute_guidance(_t(x), dev(x0o), mask, 0.3, **gkw)
        else:
            ref = s.impute(obs, mask, N, **kw)
            gu, ru = s.impute_guidance(_t(x), dev(x0o), mask, 0.3, **gkw)
        assert torch.isfinite(pair).all()
        assert torch.equal(pair, ref) and torch.equal(one, ref), wx
        assert torch.equal(gp, gu) and torch.equal(rp, ru), wx


def test_label_dropout_is_inert_in_guidance_and_likelihood():
    cfg = R.CFG
    T, Cn = cfg["T"], cfg["C"]
    x = W.randn("ci_ld_x", (B, T, Cn), 24)
    res = {}
    for p in (0.0, 0.5):
        m, sch, sd, tab, mu, sigma, yn, mk, x0o = _dps_setup(cfg, 37, label_dropout=p)
        assert m.label_dropout == p
        s = _sampler(m)
        y = torch.tensor(G.Y_CLASSES)
        out = []
        for _ in range(2):
            for wx in (1.0, WG):
                g, rn2 = s.impute_guidance(_t(x), dev(x0o), torch.from_numpy(mk), 0.3, fourier_transform=True, feature_std=_t(sigma),
                                           jacobian=True, y=y, cfg_scale=wx)
                out += [g.clone(), rn2.clone()]
            ll = s.log_likelihood(_t(x), 3, "heun", n_probes=2, seed=5, y=y)
            out += [ll.log_prob, ll.latents]
        half = len(out) // 2
        for a, b in zip(out[:half], out[half:]):
            assert torch.equal(a, b)
        res[p] = out[:half]
    for a, b in zip(res[0.0], res[0.5]):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------- 3. likelihood
def test_log_likelihood_with_labels():
    cfg, n, Ns = G.CFG_LL, 4, 4
    T, Cn = cfg["T"], cfg["C"]
    m, sch, sd, tab = make_cond(cfg, "fp32")
    s = _sampler(m, 4 * T * Cn)
    x0 = W.randn("ci_ll_x", (n, T, Cn), 25)
    X = _t(x0)
    ylist = [0, 2, 3, 0]
    y = torch.tensor(ylist)
    ex = s.log_likelihood(X, Ns, "heun", estimator="exact", y=y)
    osde = oracle_sde("vp", VP[1], True, T)
    lp = np.empty(n)
    for k in sorted(set(ylist)):
        rows = [i for i, v in enumerate(ylist) if v == k]
        score = ode_ref.model_score(G.shifted(sd, tab, k), "transformer", cfg["H"])
        lp[rows] = L.log_likelihood(osde, score, L.fd_trace(score, osde.G), x0[rows], ode_ref.grid(Ns, to_noise=True), "heun")[0]
    err, _ = report_err("cfg exact log_likelihood fp32 T=8 C=3 mixed labels vs per-label restatement", ex.log_prob.numpy(), lp)
    assert err <= 1e-5, err                                       # tests/test_gpu_likelihood.py, the exact estimator
    # the mixed batch against per-label launches, and against the unlabelled value
    stitched = torch.empty(n, dtype=ex.log_prob.dtype)
    for k in sorted(set(ylist)):
        rows = [i for i, v in enumerate(ylist) if v == k]
        stitched[rows] = s.log_likelihood(X[rows], Ns, "heun", estimator="exact", y=k).log_prob
    err2, _ = report_err("cfg exact log_likelihood mixed batch vs per-label launches", ex.log_prob.numpy(), stitched.numpy())
    assert err2 <= 1e-5, err2
    un = s.log_likelihood(X, Ns, "heun", estimator="exact")
    assert torch.equal(un.log_prob[2], s.log_likelihood(X, Ns, "heun", estimator="exact", y=K).log_prob[2])
    d = (un.log_prob - ex.log_prob).abs()
    print(f"[cfg-impute] |log p(x) - log p(x | y)| = {d.tolist()}")
    assert float(d[2]) <= 1e-5 * max(1.0, float(un.log_prob[2].abs())) and bool((d[[0, 1, 3]] > 1e-3).all())
    # the binding found is back afterwards
    from fourierdiffusion_amd import _C
    ctx, h = m._engine()
    keep = torch.tensor([1, 1, 1], dtype=torch.int32, device=DEV)
    _C.check(_C.lib().fd_score_set_labels(h, keep.data_ptr(), 3), ctx)
    try:
        s.log_likelihood(X, Ns, "heun", n_probes=1, seed=3, y=y)
        py, pb = C.c_void_p(), C.c_int(0)
        _C.check(_C.lib().fd_score_get_labels(h, C.byref(py), C.byref(pb)), ctx)
        assert py.value == keep.data_ptr() and pb.value == 3
    finally:
        _C.lib().fd_score_set_labels(h, None, 0)


def test_rk45_log_likelihood_with_labels_converges_to_the_fixed_grid():
    cfg, n, P = G.CFG_LL, 2, 1
    T, Cn = cfg["T"], cfg["C"]
    m, _, _, _ = make_cond(cfg, "fp32")
    s = _sampler(m, 8)
    X = _t(W.randn("ci_rk_x", (n, T, Cn), 26))
    rs = np.random.RandomState(4)
    e = _t(np.where(rs.rand(n, P, T, Cn) < 0.5, -1.0, 1.0))
    y = torch.tensor([0, 2])
    heun = s.log_likelihood(X, 4000, "heun", n_probes=P, probes=e, y=y).log_prob.numpy()
    out = {}
    for tol in (1e-3, 1e-5):
        r = s.log_likelihood(X, solver="rk45", rtol=tol, atol=tol, n_probes=P, probes=e, y=y)
        assert bool(r.converged.all())
        out[tol] = (r.nfe.numpy(), np.abs(r.log_prob.numpy() - heun).max())
        print(f"[cfg-impute] rk45 with labels rtol={tol:g}: nfe {out[tol][0].tolist()}, |rk45 - Heun(4000)| = {out[tol][1]:.3e} nats")
    assert (out[1e-3][0] < out[1e-5][0]).all()                    # tests/test_gpu_rk45_likelihood.py::test_convergence_against_fine_heun
    assert out[1e-5][1] < out[1e-3][1]
    un = s.log_likelihood(X, solver="rk45", rtol=1e-5, atol=1e-5, n_probes=P, probes=e)
    assert not torch.equal(un.log_prob, r.log_prob)


# ------------------------------------------------------------------------------------------------------- 4. errors and front end
def test_value_errors_and_entry_points_on_an_unlabelled_model():
    from fourierdiffusion_amd import _C
    cfg = R.CFG
    T, Cn = cfg["T"], cfg["C"]
    mk_, sch, _, _ = make_cond(cfg, "fp32")
    m0, _, _, _ = make_cond(cfg, "fp32", n_classes=0)
    sk, s0 = _sampler(mk_), _sampler(m0)
    mu, sigma, yn, mk, x0o = G.conditioning(T, Cn, B, "random", 38, True)
    obs, mask, kw = _t(yn), torch.from_numpy(mk), _kw(mu, sigma, True, True)
    x = _t(W.randn("ci_err_x", (B, T, Cn), 27))
    for extra in (dict(y=1), dict(cfg_scale=2.0)):
        with pytest.raises(ValueError):
            s0.impute(obs, mask, N, **kw, **extra)
        with pytest.raises(ValueError):
            s0.impute_guidance(x, dev(x0o), mask, 0.3, fourier_transform=True, **extra)
    with pytest.raises(ValueError):
        s0.log_likelihood(x, 3, y=1)
    for bad in (dict(y=1, cfg_scale=float("nan")), dict(y=1, cfg_scale=float("inf")), dict(y=torch.tensor([0, 1, 2])),
                dict(y=torch.tensor([0, 1, 2, 0, K + 1])), dict(y=K + 1)):
        with pytest.raises(ValueError):
            sk.impute(obs, mask, N, **kw, **bad)
        with pytest.raises(ValueError):
            sk.impute_guidance(x, dev(x0o), mask, 0.3, fourier_transform=True, **bad)
    for bad in (torch.tensor([0, 1, 2]), K + 1):
        with pytest.raises(ValueError):
            sk.log_likelihood(x, 3, y=bad)
    with pytest.raises(ValueError, match="cfg_scale"):
        sk.log_likelihood(x, 3, y=1, cfg_scale=2.0)
    # every new entry point on an unlabelled model: FD_ERR_ARG and a message
    m0.eval()
    Nn, ts_arr, dt = s0._sde_grid(N)
    ctx, h, p, Gd, mode = s0._engine_args()
    m_u8, per_series = s0._mask_u8(mask, B, T, Cn, DEV)
    buf = torch.zeros(2 * B, T, Cn, device=DEV)
    x0d, std = dev(x0o), dev(sigma)
    g, rn2 = torch.empty(B, T, Cn, device=DEV), torch.empty(B, dtype=torch.float64, device=DEV)
    lib = _C.lib()
    calls = {
        "fd_sampler_run_impute_cfg": lambda: lib.fd_sampler_run_impute_cfg(
            h, C.byref(p), Gd.data_ptr(), ts_arr, Nn, dt, buf.data_ptr(), x0d.data_ptr(), m_u8.data_ptr(), int(per_series),
            std.data_ptr(), 1, None, None, 0, 0, B, 1, mode, None, 1.0, _C.stream_of(buf)),
        "fd_sampler_run_impute_dps_cfg": lambda: lib.fd_sampler_run_impute_dps_cfg(
            h, C.byref(p), Gd.data_ptr(), ts_arr, Nn, dt, buf.data_ptr(), x0d.data_ptr(), m_u8.data_ptr(), int(per_series),
            std.data_ptr(), 1, 0.3, 0, None, 0, 0, B, 1, mode, None, 1.0, _C.stream_of(buf)),
        "fd_impute_guidance_cfg": lambda: lib.fd_impute_guidance_cfg(
            h, C.byref(p), Gd.data_ptr(), 0.3, buf.data_ptr(), x0d.data_ptr(), m_u8.data_ptr(), int(per_series), std.data_ptr(), 1, 0,
            g.data_ptr(), rn2.data_ptr(), B, 1, mode, None, 1.0, _C.stream_of(buf)),
    }
    for name, call in calls.items():
        assert call() == -1, name                                  # FD_ERR_ARG
        with pytest.raises(_C.FdError, match=name):
            _C.check(-1, ctx)


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_labels_and_cfg_scale(tmp_path):
    common = ["fourier_transform=true", "datamodule=synthetic_classes", "datamodule.max_len=24", "datamodule.num_samples=96",
              "datamodule.n_channels=4", "datamodule.batch_size=32", "datamodule.n_classes=3"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model=conditional", "score_model.n_classes=3", "score_model.d_model=24",
          "score_model.num_layers=2", "score_model.n_head=4", "trainer.max_epochs=1", "trainer.callbacks.2.every_n_epochs=1",
          "trainer.callbacks.2.num_samples=32", "trainer.callbacks.2.num_diffusion_steps=5", "run_id=cfgimp"], tmp_path)
    res_path = tmp_path / "lightning_logs" / "cfgimp" / "results.yaml"
    imp = [str(ROOT / "cmd" / "impute.py"), "model_id=cfgimp", "num_diffusion_steps=8", "mask.kind=forecast", "mask.horizon=6",
           "num_series=16", "sampler.sample_batch_size=16", "conditioning=dps", "guidance.jacobian=false"]
    ll = [str(ROOT / "cmd" / "likelihood.py"), "model_id=cfgimp", "num_diffusion_steps=6", "n_probes=2", "max_series=16",
          "sampler.sample_batch_size=32"]
    # without the new keys: the blocks as they are written today
    _run(imp, tmp_path)
    _run(ll, tmp_path)
    res = yaml.safe_load(open(res_path))
    assert set(res["impute"]) == {"mask_kind", "num_series", "hidden_fraction", "mse_hidden", "mae_hidden", "max_abs_err_observed",
                                  "conditioning", "guidance_scale", "guidance_jacobian"}
    assert "labels" not in res["likelihood"]
    plain_ll = res["likelihood"]["nll_sample"]
    _run(imp + ["labels=data", "cfg_scale=1.5"], tmp_path)
    _run(ll + ["labels=data"], tmp_path)
    res = yaml.safe_load(open(res_path))
    assert res["impute"]["labels"] == "data" and res["impute"]["cfg_scale"] == 1.5 and res["impute"]["num_series"] == 16
    assert np.isfinite(res["impute"]["mse_hidden"]) and np.isfinite(res["impute"]["mae_hidden"])
    assert res["likelihood"]["labels"] == "data" and res["likelihood"]["num_series"] == 16
    for k in ("nll_data", "bits_per_dim", "nll_sample"):
        assert np.isfinite(res["likelihood"][k]), k
    assert res["likelihood"]["nll_sample"] != plain_ll
