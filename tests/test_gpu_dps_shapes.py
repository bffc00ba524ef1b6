"""GPU: gradient-guided conditioning (csrc/fd_dps.hip: k_dps_residual, k_dps_step and their PAIR forms, under
DiffusionSampler.impute_guidance and impute(conditioning="dps")) element by element against float64 at dataset shapes: more than one
channel block (C > 16, ragged last block), more than 8 row tiles (T > 128), more than 64 KiB of LDS (T > 512, up to T = 1024:
128 KiB dynamic under the 4 KiB static reduction array), the elementwise kernel past one block of threads (fourier = 0, T > 32),
feature_std = None, a shared (T,C) mask and the paired kernels on these.  Shapes, inputs and references: tests/shapes_ref.py (each
reference computed once); the Jacobian's reference is tests/autograd_ref.py.

Bounds (tests/test_gpu_dps.py's at T = 8): g to 1e-5 of max|g|, ||r||^2 to rtol 1e-5.  r, ||r||^2, u and the Jacobian-free g depend on
the network through its forward alone and are continuous across relu kinks: the plain bound.  Whatever contains J gets the plain bound
or the kink rule of autograd_ref.explained_by_flips (the difference is +- g_k d_k of units within tau of their kink, exactly, and
nothing else).  Trajectories: 1e-4 (tests/test_gpu_impute.py's fp32 trajectories) per step, or the kink rule per step.

Every measured value is logged by tests/gpu_util.report_err."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import autograd_ref as A
from tests import shapes_ref as S
from tests.gpu_util import dev, host, make_model, report_err
from tests.test_gpu_cfg import make_cond

pytestmark = pytest.mark.gpu
B = S.B
_MODELS = {}


def _model(cfg, kind="vp", p=(0.1, 20.0)):
    key = (S.cfg_key(cfg), kind)
    if key not in _MODELS:
        _MODELS[key] = make_model(cfg, kind=kind, p=p, precision="fp32")[0]
    return _MODELS[key]


def _cond_model(cfg):
    key = (S.cfg_key(cfg), "cond")
    if key not in _MODELS:
        _MODELS[key] = make_cond(cfg, "fp32")[0]
    return _MODELS[key]


def _sampler(m, bs=B):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    return DiffusionSampler(score_model=m, sample_batch_size=bs)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


class _force_pair:
    """FDIFF_CFG_FORCE_PAIR=1 for a block."""

    def __enter__(self):
        self.old = os.environ.pop("FDIFF_CFG_FORCE_PAIR", None)
        os.environ["FDIFF_CFG_FORCE_PAIR"] = "1"

    def __exit__(self, *a):
        os.environ.pop("FDIFF_CFG_FORCE_PAIR", None)
        if self.old is not None:
            os.environ["FDIFF_CFG_FORCE_PAIR"] = self.old


def _check_flips(tag, got, case):
    """The plain 1e-5 bound on g, or the kink rule."""
    report_err(f"{tag} (tau {case['tau']:.3e}, {case['near']} units within tau)", got, case["g"])
    ok, plain, left, fits = A.explained_by_flips(got, case["g"], case["flips"], 1e-5, case["scale"])
    print(f"{tag}: plain {plain:.3e}, after flips {left:.3e}, fitted (row, coefficient / g_k) {fits}")
    assert ok, (tag, plain, left, fits)


# ------------------------------------------------------------------------------------------------------- Jacobian-free guidance
@pytest.mark.parametrize("t", S.DPS_T)
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_guidance_without_jacobian_vs_float64(name, t):
    cfg = S.SHAPES[name]
    s = _sampler(_model(cfg))
    x, t32 = S.dps_x(name, cfg, t), float(np.float32(t))
    for fourier in (True, False):
        for std_given in (True, False):
            for mask_kind in ("random", "forecast"):            # per-series (B,T,C) / one shared (T,C)
                mu, sigma, yn, mk, x0 = S.conditioning(name, cfg, fourier, std_given, mask_kind)
                gr, rr = S.guidance_free_case(name, t, fourier, std_given, mask_kind)
                g, rn2 = s.impute_guidance(_t(x), dev(x0), torch.from_numpy(mk), t32, fourier_transform=fourier,
                                           feature_std=_t(sigma) if std_given else None, jacobian=False)
                tag = f"dps guidance fp32 {name} T={cfg['T']} C={cfg['C']} no jacobian fourier={fourier} std={std_given} " \
                      f"mask={mask_kind} t={t}"
                err, _ = report_err(tag, host(g), gr)
                rerr, _ = report_err(tag + " ||r||^2", rn2.cpu().numpy(), rr)
                assert (rr > 0).all()
                assert err <= 1e-5, (tag, err)
                np.testing.assert_allclose(rn2.cpu().numpy(), rr, rtol=1e-5, err_msg=tag)


# ------------------------------------------------------------------------------------------------------- guidance with the Jacobian
@pytest.mark.parametrize("t", S.DPS_T)
@pytest.mark.parametrize("name", list(S.DPS_JAC))
def test_guidance_with_jacobian_vs_float64(name, t):
    cfg = S.DPS_JAC[name]
    c = S.guidance_jac_case(name, t)
    mu, sigma, yn, mk, x0 = S.conditioning(name, cfg, True, True, "random")
    g, rn2 = _sampler(_model(cfg)).impute_guidance(_t(S.dps_x(name, cfg, t)), dev(x0), torch.from_numpy(mk), float(np.float32(t)),
                                                   fourier_transform=True, feature_std=_t(sigma), jacobian=True)
    np.testing.assert_allclose(rn2.cpu().numpy(), c["rn2"], rtol=1e-5)
    _check_flips(f"dps guidance fp32 {name} T={cfg['T']} C={cfg['C']} with jacobian t={t}", host(g), c)


# ------------------------------------------------------------------------------------------------------- classifier-free guidance
@pytest.mark.parametrize("name", S.CFG_SHAPES)
def test_guidance_cfg_vs_float64(name):
    cfg = S.SHAPES[name]
    m = _cond_model(cfg)
    s = _sampler(m)
    mu, sigma, yn, mk, x0 = S.conditioning(name, cfg, True, True, "random")
    x, t32, y = _t(S.dps_x(name, cfg, S.CFG_T)), float(np.float32(S.CFG_T)), torch.tensor(S.CFG_Y)
    kw = dict(fourier_transform=True, feature_std=_t(sigma))
    mask = torch.from_numpy(mk)
    for jac in (True, False):
        c = S.guidance_cfg_case(name, jac)
        g, rn2 = s.impute_guidance(x, dev(x0), mask, t32, jacobian=jac, y=y, cfg_scale=S.CFG_W, **kw)
        np.testing.assert_allclose(rn2.cpu().numpy(), c["rn2"], rtol=1e-5)
        tag = f"cfg dps guidance fp32 {name} T={cfg['T']} C={cfg['C']} jacobian={jac} w={S.CFG_W}"
        if jac:
            _check_flips(tag, host(g), c)
        else:
            err, _ = report_err(tag, host(g), c["g"])
            assert err <= 1e-5, (tag, err)
    # the forced pair at w = 1: without the Jacobian the bound unpaired path to the bit (tests/test_gpu_cfg_impute.py on small shapes);
    # with it the two halves are summed, which changes the rounding: float64 and the kink rule
    from tests.test_gpu_cfg_impute import _bound
    with _force_pair():
        gp, rp = s.impute_guidance(x, dev(x0), mask, t32, jacobian=False, y=y, cfg_scale=1.0, **kw)
        gj, rj = s.impute_guidance(x, dev(x0), mask, t32, jacobian=True, y=y, cfg_scale=1.0, **kw)
    with _bound(m, S.CFG_Y):
        gu, ru = s.impute_guidance(x, dev(x0), mask, t32, jacobian=False, **kw)
    assert torch.isfinite(gp).all() and torch.equal(gp, gu) and torch.equal(rp, ru)
    c1 = S.guidance_cfg_case(name, True, 1.0)
    np.testing.assert_allclose(rj.cpu().numpy(), c1["rn2"], rtol=1e-5)
    _check_flips(f"cfg dps guidance fp32 {name} forced pair w=1 with jacobian", host(gj), c1)


# ------------------------------------------------------------------------------------------------------- trajectories
def _one_step(s, X, i, x0d, m_u8, stdd, zs):
    """fd_sampler_run_impute_dps for step i of the TRAJ_STEPS-step grid alone, on X in place (what impute() runs for all steps)."""
    from fourierdiffusion_amd import _C
    N, ts_arr, dt = s._sde_grid(S.TRAJ_STEPS)
    ctx, h, p, G, mode = s._engine_args()
    one = (C.c_float * 1)(ts_arr[i])
    rc = _C.lib().fd_sampler_run_impute_dps(h, C.byref(p), G.data_ptr(), one, 1, dt, X.data_ptr(), x0d.data_ptr(), m_u8.data_ptr(), 1,
                                            stdd.data_ptr(), 1, float(S.TRAJ_ZETA), 1, zs[i].data_ptr(), 0, 0, X.shape[0], 1, mode,
                                            _C.stream_of(X))
    _C.check(rc, ctx)


@pytest.mark.parametrize("name", ["mimic", "ragged"])
def test_trajectory_with_jacobian_vs_float64(name):
    """Four guided steps with injected noise; row 1's mask is entirely false, so its ||r|| is 0 and it takes the plain reverse-SDE
    steps.  The engine's loop is run whole through impute() and step by step; each step is compared with the float64 step FROM THE
    ENGINE'S OWN STATE, so that a kink crossed at one step is judged at that step (1e-4 of the state's maximum, or the kink rule)
    and cannot hide in, or be blamed for, what later steps make of it."""
    cfg = S.SHAPES[name]
    kind, p = S.TRAJ_SDE[name]
    m = _model(cfg, kind, p)
    s = _sampler(m)
    d = S.traj_inputs(name)
    N = S.TRAJ_STEPS
    zp, zs = dev(d["zp"]), dev(d["zs"])
    obs, mask = _t(d["yn"]), torch.from_numpy(d["mk"])
    whole = s.impute(obs, mask, N, fourier_transform=True, feature_mean=_t(d["mu"]), feature_std=_t(d["sigma"]), prior_noise=[zp],
                     step_noise=[zs], conditioning="dps", guidance_scale=S.TRAJ_ZETA, guidance_jacobian=True)
    assert torch.isfinite(whole).all()
    # the same loop one step per call
    s.score_model.eval()
    X = s.sample_prior(B, noise=zp)
    x0d = s.observed_to_sample_space(obs, mask, fourier_transform=True, feature_mean=_t(d["mu"]), feature_std=_t(d["sigma"]))
    report_err(f"dps x0_obs {name}", host(x0d), d["x0"])
    m_u8, stdd = mask.to(device=X.device, dtype=torch.uint8).contiguous(), dev(d["sigma"])
    states = [host(X)]
    for i in range(N):
        _one_step(s, X, i, x0d, m_u8, stdd, zs)
        states.append(host(X))
    assert torch.equal(X.cpu(), whole), "the loop run one step per call must be the loop run whole"
    # the unobserved row: zero residual, and the plain reverse-SDE steps (the guided reference's c = 0 branch says the same; this
    # restates it without any guidance code)
    from oracle import fdiff_oracle as O
    from tests.gpu_util import oracle_sde
    sde = oracle_sde(kind, p, True, cfg["T"])
    ts, dt = O.timesteps(N)
    g, rn2 = s.impute_guidance(dev(states[1]), x0d, mask, float(ts[1]), fourier_transform=True, feature_std=_t(d["sigma"]))
    assert float(rn2[1]) == 0.0 and (rn2.cpu().numpy()[[0, 2]] > 0).all()
    sd = S.weights(cfg)
    for i in range(N):
        row = states[i][1:2]
        plain = O.sde_step(sde, A.score(sd, row, float(ts[i]), cfg["H"]), float(ts[i]), row, d["zs"][i][1:2], float(dt))
        err, _ = report_err(f"dps trajectory {name} {kind} step {i} unobserved row vs plain reverse-SDE step", states[i + 1][1:2], plain)
        assert err <= 1e-4, (i, err)
    # every step from the engine's own state
    crossed = []
    for i in range(N):
        nxt, tau, near, flips, scale = S.traj_step_case(name, i, states[i])
        tag = f"dps trajectory fp32 {name} {kind} T={cfg['T']} C={cfg['C']} with jacobian step {i}"
        report_err(f"{tag} (tau {tau:.3e}, {near} units within tau)", states[i + 1], nxt)
        assert near <= A.MAX_FLIPS, (i, near)
        ok, plain, left, fits = A.explained_by_flips(states[i + 1], nxt, flips, 1e-4, scale)
        print(f"{tag}: plain {plain:.3e}, after flips {left:.3e}, fitted {fits}")
        assert ok, (tag, plain, left, fits)
        crossed += fits
    # and the whole trajectory against the float64 trajectory from the same noise.  A step that needed the kink rule sends the two
    # trajectories down different branches of J from there on: the steps above are then the whole check, and this figure is a record
    err, _ = report_err(f"dps trajectory fp32 {name} {kind} T={cfg['T']} C={cfg['C']} with jacobian, {N} steps, vs float64 trajectory"
                        f" ({len(crossed)} fitted flips on the way)", whole.numpy(), S.traj_reference(name)[-1])
    assert crossed or err <= 1e-4, err
