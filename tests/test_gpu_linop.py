"""GPU: conditioning on a dense linear observation (DiffusionSampler.impute(operator=P) / fd_linop_create / fd_impute_project_op /
fd_sampler_run_impute_op / fd_impute_guidance_op / fd_sampler_run_impute_dps_op, an extension not in the reference) against the
float64 restatement of tests/linop_ref.py: the projection and one guidance evaluation at the shapes where the tiling of the
rectangular products can go wrong, trajectories under both conditionings, the window-mean matrix against aggregate=w, the lowpass
operator pasting packed coordinates, the all-false mask against sample(), reproducibility and replication, Philox against injected
noise, the handle's argument checks, bf16 at the ecg shape, and the CLI end to end.  Bounds are those of
tests/test_gpu_aggregate.py for the same quantities.  Measured errors are logged by tests/gpu_util.report_err / log_line."""
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
from tests import impute_ref as I
from tests import linop_ref as Q
from tests import ode_ref
from tests.gpu_util import dev, host, log_line, make_model, oracle_sde, report_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _sampler(m, bs):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    return DiffusionSampler(score_model=m, sample_batch_size=bs)


def _operator(name, T):
    from fourierdiffusion_amd.sampling import masks as M
    return {"lowpass": lambda: M.lowpass_operator(T, 4), "blur_full": lambda: M.gaussian_blur_operator(T, 1.0, 1),
            "difference": lambda: M.difference_operator(T), "moving_average": lambda: M.moving_average_operator(T, 4, 2),
            "blur": lambda: M.gaussian_blur_operator(T, 2.0, 4)}[name]()


def _inputs(T, Cn, B, Pm, seed, per_series=True, standardize=True, fourier=True, rows=False, empty_row=False):
    """mu, sigma (f32-representable), observations y = P x (NaN where hidden), the mask over P's rows -- single rows when `rows`
    (orthogonal operators), else whole (series, channel) columns -- and x0_obs in float64."""
    rs = np.random.RandomState(seed)
    mu = (0.3 * rs.randn(T, Cn)).astype(np.float32).astype(np.float64)
    sigma = rs.uniform(0.5, 2.0, (T, Cn)).astype(np.float32).astype(np.float64)
    if not standardize:
        mu, sigma = np.zeros((T, Cn)), np.ones((T, Cn))
    M = Pm.shape[0]
    y = Q.P(np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(B, T, Cn), Pm).astype(np.float32)
    if rows:
        m = rs.rand(B, M, Cn) < 0.6 if per_series else rs.rand(M, Cn) < 0.6
    else:
        col = rs.rand(B, 1, Cn) < 0.6 if per_series else rs.rand(1, Cn) < 0.6
        col[..., 0] = True           # (at least one observed column)
        m = np.broadcast_to(col, (B, M, Cn) if per_series else (M, Cn)).copy()
    if empty_row and per_series:
        m[0] = False
    yn = np.where(np.broadcast_to(m, y.shape), y, np.nan).astype(np.float32)
    return mu, sigma, yn, m, Q.x0_obs(yn, m, mu, sigma, fourier, Pm)


# ---------------------------------------------------------------- float32 numpy restatements (the rounding a case may claim)
def _f32_bases(T, Pm, fourier):
    """The matrices of one domain in float32: to the observation, back from it, and the adjoint's (with 1 / rho folded in)."""
    eye = np.eye(T)[None]                                               # (1, T, T): column c is the unit vector e_c along the time axis
    Fi = O.idft(eye)[0] if fourier else np.eye(T)                       # idft and dft as matrices acting on that axis
    Fm = O.dft(eye)[0] if fourier else np.eye(T)
    Pp = np.linalg.pinv(Pm)
    return (Pm @ Fi).astype(np.float32), (Fm @ Pp).astype(np.float32), (Fi.T @ Pm.T).astype(np.float32)


def _f32_project_err(x, x0, m, sigma, G, alpha, s, z, fourier, Pm, ref):
    A, Bm, _ = _f32_bases(x.shape[1], Pm, fourier)
    f = np.float32
    x32, sg = x.astype(f), sigma.astype(f)[None]
    d = f(alpha) * x0.astype(f) + f(s) * (G.astype(f)[None, :, None] * z.astype(f)) - x32
    pm = np.einsum("mt,btc->bmc", A, sg * d)
    v = np.einsum("tm,bmc->btc", Bm, np.where(np.broadcast_to(m, pm.shape), pm, f(0)))
    out = x32 + v / sg
    assert out.dtype == np.float32
    return float(np.abs(out - ref).max() / max(1.0, np.abs(ref).max()))


def _f32_guidance_err(x, score, x0, m, sigma, G, alpha, s, fourier, Pm, ref):
    A, _, Bt = _f32_bases(x.shape[1], Pm, fourier)
    f = np.float32
    sg = sigma.astype(f)[None]
    sg2 = f(s * s) * (G.astype(f) ** 2)[None, :, None]
    x0h = (x.astype(f) + sg2 * score.astype(f)) / f(alpha)
    pm = np.einsum("mt,btc->bmc", A, sg * (x0.astype(f) - x0h))
    r = np.where(np.broadcast_to(m, pm.shape), pm, f(0))
    g = (f(2.0) / f(alpha)) * (sg * np.einsum("tm,bmc->btc", Bt, r))
    assert g.dtype == np.float32
    return float(np.abs(g - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------- the projection and one guidance evaluation
# (T, C, operator): Mp < Tp with M = 7 in one row tile; M = T; two channel blocks (the second of one channel) with M = 36 and 17,
# neither a multiple of 16; nine packed row tiles on eight waves with three tiles of P's rows
CASES = [(20, 3, "lowpass"), (20, 3, "blur_full"), (37, 17, "difference"), (37, 17, "moving_average"), (130, 17, "blur")]
# the cases whose bound is 8 x the error of the float32 numpy restatement instead of 1e-5: none needed it
F32_BOUND_PROJECTION: set = set()
F32_BOUND_GUIDANCE: set = set()


@pytest.mark.parametrize("T,Cn,name", CASES)
def test_projection_and_guidance_against_float64(T, Cn, name):
    from fourierdiffusion_amd.sampling.masks import LinearOperator
    B, t = 3, float(np.float32(0.3))
    Pm = _operator(name, T)
    op = LinearOperator(Pm)
    cfg = dict(T=T, C=Cn, D=8, L=1, H=4)
    m_, _, sd = make_model(cfg, precision="fp32")
    s = _sampler(m_, B)
    osde = oracle_sde("vp", (0.1, 20.0), True, T)
    score_fn = ode_ref.model_score(sd, "transformer", cfg["H"])
    x = W.randn(f"lin_x_{T}_{Cn}", (B, T, Cn), 0)
    z = W.randn(f"lin_z_{T}_{Cn}", (B, T, Cn), 1)
    score = score_fn(x.astype(np.float64), t)          # one float64 forward per shape, shared by every combination below
    t_proj = 0.35
    alpha, sdev = (float(np.float32(v)) for v in m_.noise_scheduler.marginal_coef(t_proj))      # (the engine takes them as floats)
    al_g, s_g = Q.D.coef(osde, t)
    worst_p = worst_g = worst_p32 = worst_g32 = 0.0
    for fourier in (True, False):
        for standardize in (True, False):
            for per_series in (True, False):
                tag = f"T={T} C={Cn} {name} fourier={fourier} std={standardize} per_series={per_series}"
                mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, Pm, T + op.M, per_series, standardize, fourier, rows=name == "lowpass",
                                                empty_row=True)
                std = torch.from_numpy(sigma).float() if standardize else None
                mean = torch.from_numpy(mu).float() if standardize else None
                x0d = s.observed_to_sample_space(torch.from_numpy(yn), torch.from_numpy(mk), fourier_transform=fourier,
                                                 feature_mean=mean, feature_std=std, operator=op)
                assert np.abs(host(x0d) - x0).max() <= 1e-5 * max(1.0, np.abs(x0).max()), tag
                # the projection at the level of t_proj, from the float64 x0_obs so that its own rounding stays out
                got = host(s.impute_project(torch.from_numpy(x), dev(x0), torch.from_numpy(mk), t_proj, fourier_transform=fourier,
                                            feature_std=std, noise=dev(z), operator=op))
                ref = Q.project(x, x0, mk, sigma, osde.G, alpha, sdev, z, fourier, Pm)
                err = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
                e32 = _f32_project_err(x, x0, mk, sigma, osde.G, alpha, sdev, z, fourier, Pm, ref)
                print(f"{tag}: projection {err:.3e} of scale (float32 numpy {e32:.3e})")
                worst_p, worst_p32 = max(worst_p, err), max(worst_p32, e32)
                assert err <= (8 * e32 if (T, Cn, name) in F32_BOUND_PROJECTION else 1e-5), (tag, err, e32)
                # one Jacobian-free guidance evaluation
                g, rn2 = s.impute_guidance(torch.from_numpy(x), dev(x0), torch.from_numpy(mk), t, fourier_transform=fourier,
                                           feature_std=std, jacobian=False, operator=op)
                gr, rr, _ = Q.guidance(score_fn, osde, x, t, x0, mk, sigma, fourier, Pm, jacobian=False, score=score)
                errg = float(np.abs(host(g) - gr).max() / np.abs(gr).max())
                g32 = _f32_guidance_err(x, score, x0, mk, sigma, osde.G, al_g, s_g, fourier, Pm, gr)
                print(f"{tag}: guidance {errg:.3e} of max|g| (float32 numpy {g32:.3e})")
                worst_g, worst_g32 = max(worst_g, errg), max(worst_g32, g32)
                assert errg <= (8 * g32 if (T, Cn, name) in F32_BOUND_GUIDANCE else 1e-5), (tag, errg, g32)
                np.testing.assert_allclose(rn2.cpu().numpy(), rr, rtol=1e-5, err_msg=tag)
                if per_series:       # the row without an observed entry
                    assert float(rn2[0]) == 0.0 and rr[0] == 0.0 and not host(g)[0].any(), tag
    log_line(f"[parity] linop T={T} C={Cn} {name} M={op.M} cond={op.condition:.1f}: projection worst {worst_p:.3e} of scale (float32 numpy "
             f"{worst_p32:.3e}), guidance worst {worst_g:.3e} of max|g| (float32 numpy {worst_g32:.3e})")


# ---------------------------------------------------------------- trajectories
def _noise(tag, shape, N):
    zp = W.randn(f"lint_p_{tag}", shape, 1)
    zs = np.stack([W.randn(f"lint_z{i}_{tag}", shape, 1) for i in range(N)])
    zo = np.stack([W.randn(f"lint_o{i}_{tag}", shape, 1) for i in range(N)])
    return zp, zs, zo


@pytest.mark.parametrize("kind,p,name", [("vp", (0.1, 20.0), "lowpass"), ("ve", (0.01, 2.0), "moving_average")])
def test_replace_trajectory_vs_float64(kind, p, name):
    cfg, N, B = CFG_TINY, 10, 3
    T, Cn = cfg["T"], cfg["C"]
    Pm = _operator(name, T)
    m_, _, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, Pm, 11, rows=name == "lowpass")
    zp, zs, zo = _noise(f"r_{kind}", (B, T, Cn), N)
    X = _sampler(m_, B).impute(torch.from_numpy(yn), torch.from_numpy(mk), N, fourier_transform=True,
                               feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
                               prior_noise=[dev(zp)], step_noise=[dev(zs)], obs_noise=[dev(zo)], operator=Pm).numpy()
    ref = Q.impute_trajectory(sd, oracle_sde(kind, p, True, T), zp, list(zs), list(zo), x0, mk, sigma, True, cfg["H"], Pm)
    err, _ = report_err(f"linop replace f32 T={T} {name} {kind}", X, ref)
    assert np.isfinite(X).all() and err <= 1e-4, err
    got = Q.P(I.forward_map(X, mu, sigma, True), Pm)          # the last step is hard: P A(result) = y on the observed rows
    dev_y = float(np.abs(got[mk] - yn[mk]).max())
    print(f"linop replace {kind} {name}: observed rows reproduced to {dev_y:.3e}")
    assert dev_y <= 1e-4 * max(1.0, float(np.abs(yn[mk]).max()))


@pytest.mark.parametrize("kind,p,name,jacobian", [("vp", (0.1, 20.0), "lowpass", False), ("ve", (0.01, 2.0), "moving_average", False),
                                                  ("vp", (0.1, 20.0), "moving_average", True)])
def test_dps_trajectory_vs_float64(kind, p, name, jacobian):
    cfg, N, B, zeta = CFG_TINY, 10, 3, 0.3
    T, Cn = cfg["T"], cfg["C"]
    Pm = _operator(name, T)
    m_, _, sd = make_model(cfg, kind=kind, p=p, precision="fp32")
    mu, sigma, yn, mk, x0 = _inputs(T, Cn, B, Pm, 13, rows=True)          # any row mask under dps
    zp, zs, _ = _noise(f"d_{kind}_{jacobian}", (B, T, Cn), N)
    X = _sampler(m_, B).impute(torch.from_numpy(yn), torch.from_numpy(mk), N, fourier_transform=True,
                               feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
                               prior_noise=[dev(zp)], step_noise=[dev(zs)], conditioning="dps", guidance_scale=zeta,
                               guidance_jacobian=jacobian, operator=Pm).numpy()
    ref = Q.trajectory(ode_ref.model_score(sd, "transformer", cfg["H"]), oracle_sde(kind, p, True, T), zp, list(zs), x0, mk, sigma,
                       True, zeta, Pm, jacobian)
    err, _ = report_err(f"linop dps f32 T={T} {name} {kind} jacobian={jacobian}", X, ref)
    assert np.isfinite(X).all() and err <= 1e-5, err


# ---------------------------------------------------------------- the window-mean matrix is aggregate=w up to rounding
@pytest.mark.parametrize("T,Cn,w", [(20, 3, 3), (37, 17, 2)])
def test_window_mean_operator_equals_aggregate(T, Cn, w):
    """The two paths round their bases from different sums, so the results agree to 1e-5 of scale, not to the bit."""
    from fourierdiffusion_amd.sampling.masks import LinearOperator, window_mean_operator
    B, N = 3, 5
    op = LinearOperator(window_mean_operator(T, w))
    assert op.rows_orthogonal
    m_, _, _ = make_model(dict(T=T, C=Cn, D=8, L=1, H=4), precision="fp32")
    s = _sampler(m_, B)
    mu, sigma, yn, mk, _ = _inputs(T, Cn, B, op.P, 3, rows=True)
    obs, mask = torch.from_numpy(yn), torch.from_numpy(mk)
    mean, std = torch.from_numpy(mu).float(), torch.from_numpy(sigma).float()
    x, z = W.randn(f"linw_x_{T}", (B, T, Cn), 0), W.randn(f"linw_z_{T}", (B, T, Cn), 1)
    zp, zs, zo = _noise(f"w_{T}", (B, T, Cn), N)

    def close(a, b, what):
        a, b = host(a) if a.is_cuda else a.numpy(), host(b) if b.is_cuda else b.numpy()
        err = float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))
        assert np.isfinite(a).all() and err <= 1e-5, (what, err)

    for fourier in (True, False):
        kw = dict(fourier_transform=fourier, feature_mean=mean, feature_std=std)
        xa = s.observed_to_sample_space(obs, mask, aggregate=w, **kw)
        xo = s.observed_to_sample_space(obs, mask, operator=op, **kw)
        close(xo, xa, ("x0_obs", fourier))
        close(s.impute_project(torch.from_numpy(x), xa, mask, 0.35, fourier_transform=fourier, feature_std=std, noise=dev(z), operator=op),
              s.impute_project(torch.from_numpy(x), xa, mask, 0.35, fourier_transform=fourier, feature_std=std, noise=dev(z), aggregate=w),
              ("project", fourier))
        ga, ra = s.impute_guidance(torch.from_numpy(x), xa, mask, 0.3, fourier_transform=fourier, feature_std=std, jacobian=False,
                                   aggregate=w)
        go, ro = s.impute_guidance(torch.from_numpy(x), xa, mask, 0.3, fourier_transform=fourier, feature_std=std, jacobian=False,
                                   operator=op)
        assert float((go - ga).abs().max() / ga.abs().max()) <= 1e-5, fourier
        np.testing.assert_allclose(ro.cpu().numpy(), ra.cpu().numpy(), rtol=1e-5)
        inj = dict(prior_noise=[dev(zp)], step_noise=[dev(zs)])
        for extra in (dict(obs_noise=[dev(zo)]), dict(conditioning="dps", guidance_scale=0.3, guidance_jacobian=False)):
            close(s.impute(obs, mask, N, operator=op, **kw, **inj, **extra), s.impute(obs, mask, N, aggregate=w, **kw, **inj, **extra),
                  ("impute", fourier, tuple(extra)))


# ---------------------------------------------------------------- lowpass on an unstandardised Fourier model pastes packed coordinates
def test_lowpass_pastes_packed_coordinates():
    from fourierdiffusion_amd.sampling.masks import LinearOperator, lowpass_operator
    T, Cn, B, nf = 20, 3, 4, 4
    op = LinearOperator(lowpass_operator(T, nf))
    m_, _, _ = make_model(dict(T=T, C=Cn, D=8, L=1, H=4), precision="fp32")
    s = _sampler(m_, B)
    rs = np.random.RandomState(2)
    y = Q.P(rs.randn(B, T, Cn), op.P).astype(np.float32)
    mk = rs.rand(B, op.M, Cn) < 0.6
    x0 = host(s.observed_to_sample_space(torch.from_numpy(y), torch.from_numpy(mk), fourier_transform=True, operator=op))
    x = W.randn("linlp_x", (B, T, Cn), 0)
    got = host(s.impute_project(torch.from_numpy(x), dev(x0), torch.from_numpy(mk), None, fourier_transform=True, operator=op))
    # row 0 is packed coordinate 0, rows 2k - 1 / 2k (cos / sin of bin k) are Re X_k / Im X_k: packed k and T // 2 + k
    coord = np.array([0] + [c for k in range(1, nf) for c in (k, T // 2 + k)])
    pasted = np.zeros((B, T, Cn), bool)
    for j, c in enumerate(coord):
        pasted[:, c] = mk[:, j]
    assert pasted.any() and (~pasted).any()
    assert np.abs(got[pasted] - x0[pasted]).max() <= 1e-6
    assert np.abs(got[~pasted] - x[~pasted]).max() <= 1e-6


# ---------------------------------------------------------------- the all-false mask is the plain sampler
def test_zero_mask_equals_sample(monkeypatch):
    monkeypatch.setenv("FDIFF_SAMPLER_STEPWISE", "1")
    from fourierdiffusion_amd.sampling.masks import moving_average_operator
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg, n, N = dict(T=40, C=5, D=24, L=2, H=4), 8, 15
    Pm = moving_average_operator(40, 4, 2)
    m_, _, _ = make_model(cfg, precision="fp32")
    sampler = DiffusionSampler(score_model=m_, sample_batch_size=n, merge_batches=False)
    rs = np.random.RandomState(0)
    std = torch.from_numpy(rs.uniform(0.5, 2, (40, 5))).float()
    for fourier in (True, False):
        torch.manual_seed(3)
        Xs = sampler.sample(num_samples=n, num_diffusion_steps=N)
        torch.manual_seed(3)
        Xi = sampler.impute(torch.from_numpy(rs.randn(n, Pm.shape[0], 5)).float(), torch.zeros(Pm.shape[0], 5, dtype=torch.bool), N,
                            fourier_transform=fourier, feature_mean=torch.zeros(40, 5), feature_std=std, operator=Pm)
        assert torch.isfinite(Xs).all()
        assert ((Xi - Xs.cpu()).abs().max() / Xs.abs().max()).item() <= 1e-6, fourier


# ---------------------------------------------------------------- reproducibility, replication, Philox
def test_reproducible_and_replicated():
    from fourierdiffusion_amd.sampling.masks import LinearOperator, moving_average_operator
    cfg, n, K, N = dict(T=40, C=5, D=24, L=2, H=4), 4, 3, 6
    T, Cn = cfg["T"], cfg["C"]
    op = LinearOperator(moving_average_operator(T, 4, 2))
    m_, _, _ = make_model(cfg, precision="fp32")
    mu, sigma, yn, mk, _ = _inputs(T, Cn, n, op.P, 7)
    obs, mask = torch.from_numpy(yn), torch.from_numpy(mk)
    s = _sampler(m_, n * K)
    shape = (n * K, T, Cn)
    zp, zs, zo = _noise("rep", shape, N)
    for fourier in (True, False):
        kw = dict(fourier_transform=fourier, feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
                  operator=op)
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
    from fourierdiffusion_amd.sampling.masks import LinearOperator, gaussian_blur_operator
    B, T, Cn, seed, offset = 5, 100, 12, 1234567, 4096
    op = LinearOperator(gaussian_blur_operator(T, 2.0, 4))
    rs = np.random.RandomState(7)
    x, x0, sig = dev(rs.randn(B, T, Cn)), dev(rs.randn(B, T, Cn)), dev(rs.uniform(0.5, 2.0, (T, Cn)))
    m = torch.from_numpy(np.broadcast_to(rs.rand(B, 1, Cn) < 0.5, (B, op.M, Cn)).astype(np.uint8).copy()).cuda()
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
            _C.check(_C.lib().fd_impute_project_op(h, x.data_ptr(), x0.data_ptr(), m.data_ptr(), 1, sig.data_ptr(), fourier, G.data_ptr(),
                                                   0.6, 0.5, _C.ptr(zz), sd, off, out.data_ptr(), B, T, Cn, op.handle(h),
                                                   _C.stream_of(x)), h)
            outs.append(out)
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], x), fourier


def test_handle_argument_checks():
    """Null, wrong-T and M > T handles are FD_ERR_ARG; a handle can be destroyed and made again."""
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.masks import LinearOperator, lowpass_operator
    B, T, Cn = 2, 20, 3
    x = dev(np.zeros((B, T, Cn)))
    out = torch.empty_like(x)
    m = torch.ones(7, Cn, dtype=torch.uint8).cuda()
    G = dev(O.noise_scaling(T, True))
    h = _C.ctx(x.device)
    P = np.ascontiguousarray(lowpass_operator(T, 4))
    Pp = np.ascontiguousarray(np.linalg.pinv(P))
    lo = _C._vp()
    assert _C.lib().fd_linop_create(h, T, T + 1, P.ctypes.data, Pp.ctypes.data, C.byref(lo)) == -1        # M > T
    assert _C.lib().fd_linop_create(h, T, 0, P.ctypes.data, Pp.ctypes.data, C.byref(lo)) == -1
    assert _C.lib().fd_linop_create(h, T, 7, None, Pp.ctypes.data, C.byref(lo)) == -1
    assert _C.lib().fd_linop_destroy(None) == 0

    def project(handle, t):
        return _C.lib().fd_impute_project_op(h, x.data_ptr(), x.data_ptr(), m.data_ptr(), 0, None, 1, G.data_ptr(), 1.0, 0.0, None, 0, 0,
                                             out.data_ptr(), B, t, Cn, handle, _C.stream_of(x))
    assert project(None, T) == -1                                                     # a null handle
    op24 = LinearOperator(lowpass_operator(24, 4))
    assert project(op24.handle(h), T) == -1                                           # a handle of another T
    op = LinearOperator(P)
    assert project(op.handle(h), T) == 0
    first = op.handle(h).value
    assert op.handle(h).value == first                                                # created once per context
    op.close()
    assert project(op.handle(h), T) == 0 and torch.isfinite(out).all()                # ... and again after close()


# ---------------------------------------------------------------- bf16 at the ecg shape
def test_bf16_ecg_shape():
    from fourierdiffusion_amd.sampling.masks import LinearOperator, lowpass_operator
    cfg, B, N = CFG_DEFAULT, 64, 10
    T, Cn = cfg["T"], cfg["C"]
    op = LinearOperator(lowpass_operator(T, 8))
    mb, _, _ = make_model(cfg, precision="bf16")
    mu, sigma, yn, mk, _ = _inputs(T, Cn, B, op.P, 5, rows=True)
    kw = dict(fourier_transform=True, feature_mean=torch.from_numpy(mu).float(), feature_std=torch.from_numpy(sigma).float(),
              operator=op)
    for extra in (dict(), dict(conditioning="dps", guidance_scale=1.0, guidance_jacobian=False)):
        torch.manual_seed(1)
        X = _sampler(mb, B).impute(torch.from_numpy(yn), torch.from_numpy(mk), N, **kw, **extra)
        assert X.shape == (B, T, Cn) and torch.isfinite(X).all(), extra


# ---------------------------------------------------------------- CLI
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_impute_operator(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=linoprun"], tmp_path)
    _run([str(ROOT / "cmd" / "impute.py"), "model_id=linoprun", "num_diffusion_steps=10", "sampler.sample_batch_size=40",
          "operator.kind=lowpass", "operator.n_freq=4", "mask.kind=forecast", "mask.horizon=2"], tmp_path)
    run_dir = tmp_path / "lightning_logs" / "linoprun"
    X = torch.load(run_dir / "imputations.pt")
    assert X.shape == (96, 24, 4) and torch.isfinite(X).all()
    res = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert res["operator"]["kind"] == "lowpass" and res["operator"]["n_freq"] == 4 and res["operator"]["M"] == 7
    assert res["mask_kind"] == "forecast" and res["hidden_fraction"] == 1.0
    assert np.isfinite(res["mse_hidden"]) and np.isfinite(res["mae_hidden"])
    assert res["max_abs_err_operator"] <= 1e-3
