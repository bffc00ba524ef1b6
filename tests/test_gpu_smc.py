"""GPU: twisted sequential Monte Carlo conditioning (DiffusionSampler.impute(conditioning="smc") / fd_sampler_run_impute_smc /
fd_smc_resample / fd_smc_step, an extension not in the reference) against the float64 restatement of tests/smc_ref.py: the stage and
the proposal alone, the loop on the case table of tests/smc_cases.py (whose decision margins tests/test_smc_cpu.py asserts, so that
ancestors and resample decisions must be EQUAL here), the bit anchors, bf16 at the ecg shape, and the CLI end to end."""
import ctypes as C
import math
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
from tests import dps_ref as D
from tests import ode_ref
from tests import smc_cases as Cs
from tests import smc_ref as S
from tests.gpu_util import dev, host, make_model, oracle_sde, report_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda"


def _ctx():
    from fourierdiffusion_amd import _C
    return _C, _C.ctx(torch.device(DEV))


def _sampler(m, bs):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    return DiffusionSampler(score_model=m, sample_batch_size=bs)


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


# ---------------------------------------------------------------- fd_smc_resample
def _resample(logw, u, thr, force=False, final=False):
    _C, ctx = _ctx()
    n, K = logw.shape
    lw = torch.from_numpy(np.ascontiguousarray(logw, dtype=np.float64)).to(DEV)
    ud = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64)).to(DEV)
    anc = torch.full((n, K), -1, dtype=torch.int32, device=DEV)
    ess = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
    res = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    dz = torch.full((n,), 99.0, dtype=torch.float64, device=DEV)
    rc = _C.lib().fd_smc_resample(ctx, lw.data_ptr(), ud.data_ptr(), n, K, float(thr), int(force), int(final), anc.data_ptr(),
                                  ess.data_ptr(), res.data_ptr(), dz.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _C.check(rc, ctx)
    return dict(logw=lw.cpu().numpy(), anc=anc.cpu().numpy(), ess=ess.cpu().numpy(), resampled=res.cpu().numpy().astype(bool),
                dlogz=dz.cpu().numpy())


def _same_stage(got, ref):
    assert np.array_equal(got["anc"], ref["anc"])
    assert np.array_equal(got["resampled"], ref["resampled"])
    assert np.array_equal(got["logw"], ref["logw"], equal_nan=True)
    np.testing.assert_allclose(got["ess"], ref["ess"], rtol=1e-12)
    np.testing.assert_allclose(got["dlogz"], ref["dlogz"], rtol=1e-12)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("K", [2, 3, 64, 100, 257, 1024])
def test_resample_random_weights(K, n):
    """Series alternate between spread-out weights (resampled) and nearly uniform ones (kept) at threshold 0.5."""
    rs = np.random.RandomState(7 * K + n)
    scale = np.where(np.arange(n) % 2 == 0, 3.0, 0.3)[:, None]
    logw = scale * rs.randn(n, K) + rs.uniform(-50, 50, (n, 1))
    u = rs.rand(n)
    ref = S.stage(logw, u, 0.5, False)
    mc = min([float(np.abs(ref["cum"][q][:, None] - ref["target"][q][None, :]).min()) for q in range(n) if ref["resampled"][q]],
             default=1.0)
    me = float(np.abs(ref["ess"] - 0.5 * K).min() / K)
    assert mc >= 1e-9 and me >= 1e-9, (mc, me)      # (holds for every case of the table: no case is dropped)
    assert ref["resampled"][0] or K <= 3      # (two or three particles keep ESS >= K / 2 more often than not)
    _same_stage(_resample(logw, u, 0.5), ref)
    # forced, as the final stage under final_resample; and the final stage without it
    _same_stage(_resample(logw, u, 0.0, force=True, final=True), S.stage(logw, u, 0.0, True, final=True))
    _same_stage(_resample(logw, u, 0.0, final=True), S.stage(logw, u, 0.0, False, final=True))


def test_resample_closed_form_cases():
    K = 7
    for u in (0.01, 0.3, 0.5, 0.99):      # uniform weights: the identity
        got = _resample(np.full((1, K), -3.25), [u], 1.0, force=True)
        assert (got["anc"][0] == np.arange(K)).all() and got["resampled"][0] and (got["logw"] == 0).all()
        assert abs(got["ess"][0] - K) < 1e-12 and abs(got["dlogz"][0] + 3.25) < 1e-12
    lw = np.full((1, 5), -800.0)            # one dominant weight
    lw[0, 3] = 2.0
    got = _resample(lw, [0.4], 0.5)
    assert got["resampled"][0] and (got["anc"][0] == 3).all() and abs(got["ess"][0] - 1.0) < 1e-12
    assert abs(got["dlogz"][0] - (2.0 - math.log(5))) < 1e-12
    # -inf and NaN entries have weight 0; a series of them alone is kept as it is, with ESS 0 and evidence -inf
    lw = np.array([[-np.inf, 0.0, np.nan, 0.0], [-np.inf, np.nan, -np.inf, -np.inf], [0.0, 0.0, 0.0, -np.inf]])
    got = _resample(lw, [0.5, 0.5, 0.5], 0.9)
    _same_stage(got, S.stage(lw, [0.5, 0.5, 0.5], 0.9, False))
    assert got["anc"][0].tolist() == [1, 1, 3, 3] and got["anc"][1].tolist() == [0, 1, 2, 3]
    assert got["ess"][1] == 0 and got["dlogz"][1] == -np.inf and not got["resampled"][1]
    assert got["resampled"][2] and 3 not in got["anc"][2]
    # ESS exactly above the threshold: kept
    lw = np.log(np.array([[1.0, 1.0, 1.0, 3.0]]))
    keep = _resample(lw, [0.2], 0.75 - 1e-9)
    assert not keep["resampled"][0] and np.array_equal(keep["logw"], lw) and keep["dlogz"][0] == 0
    cut = _resample(lw, [0.2], 0.75 + 1e-9)
    assert cut["resampled"][0] and cut["anc"][0].tolist() == [0, 1, 3, 3]


def test_entry_points_reject_bad_arguments():
    _C, ctx = _ctx()
    lib = _C.lib()
    d = torch.zeros(64, dtype=torch.float64, device=DEV)
    a = torch.zeros(64, dtype=torch.int32, device=DEV)
    for K, thr in ((1, 0.5), (1025, 0.5), (4, 1.5), (4, -0.1)):
        assert lib.fd_smc_resample(ctx, d.data_ptr(), d.data_ptr(), 1, K, thr, 0, 0, a.data_ptr(), None, None, None, None) != 0
    m, _, _ = make_model(dict(T=8, C=3, D=8, L=2, H=4))
    s = _sampler(m, 8)
    s.score_model.eval()
    X = s.sample_prior(8)
    _ctx2, h, p, G, mode = s._engine_args()
    N, ts_arr, dt = s._sde_grid(4)
    mk = torch.ones(8, 3, dtype=torch.uint8, device=DEV)

    def run(B=8, K=4, obs_std=0.3, tw=1.0, thr=0.5):
        return lib.fd_sampler_run_impute_smc(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), X.data_ptr(), mk.data_ptr(), 0,
                                             None, 1, 0, obs_std, tw, thr, 1, None, None, 1, 0, B, K, mode, None, None, None, None,
                                             None, _C.stream_of(X))
    before = X.clone()
    for kw in (dict(K=1), dict(K=1025, B=1025), dict(B=6), dict(obs_std=0.0), dict(obs_std=-1.0), dict(thr=1.1), dict(thr=-0.5),
               dict(tw=-1.0), dict(tw=float("inf")), dict(tw=float("nan"))):
        assert run(**kw) != 0, kw
    assert torch.equal(X, before)
    assert run() == 0 and torch.isfinite(X).all()


# ---------------------------------------------------------------- fd_smc_step
def _step(sde_p, G, t, dt, x, score, g, anc, z, inv2v, K, seed=0, offset=0):
    _C, ctx = _ctx()
    B, T, Cn = x.shape
    xo = torch.empty_like(x)
    c1 = torch.empty(B, dtype=torch.float64, device=DEV)
    c2 = torch.empty(B, dtype=torch.float64, device=DEV)
    rc = _C.lib().fd_smc_step(ctx, C.byref(sde_p), G.data_ptr(), float(t), float(dt), x.data_ptr(), score.data_ptr(), g.data_ptr(),
                              None if anc is None else anc.data_ptr(), None if z is None else z.data_ptr(), seed, offset,
                              float(inv2v), xo.data_ptr(), c1.data_ptr(), c2.data_ptr(), B, K, T, Cn,
                              torch.cuda.current_stream().cuda_stream)
    _C.check(rc, ctx)
    return xo, c1.cpu().numpy(), c2.cpu().numpy()


@pytest.mark.parametrize("kind,p", [("vp", (0.1, 20.0)), ("ve", (0.01, 2.0))])
@pytest.mark.parametrize("T,Cn", [(8, 3), (5, 3), (24, 40), (130, 17)])
def test_step_against_float64(T, Cn, kind, p):
    from fourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler
    _C, ctx = _ctx()
    n, K = 3, 4
    B = n * K
    sch = (VPScheduler(beta_min=p[0], beta_max=p[1], fourier_noise_scaling=True) if kind == "vp"
           else VEScheduler(sigma_min=p[0], sigma_max=p[1], fourier_noise_scaling=True))
    sch.set_noise_scaling(T)
    osde = oracle_sde(kind, p, True, T)
    tag = f"smcs_{T}_{Cn}_{kind}"
    x, score, g, z = (W.randn(f"{tag}_{k}", (B, T, Cn), 0) for k in "xsgz")
    anc = np.array([1, 1, 3, 0, 2, 2, 2, 2, 3, 0, 1, 2], dtype=np.int32)
    src = (np.arange(B) // K) * K + anc
    t, dt, inv2v = float(np.float32(0.4)), float(np.float32(0.01)), 0.7
    G = sch.G_on(torch.device(DEV))
    xd, sd_, gd, zd, ad = dev(x), dev(score), dev(g), dev(z), torch.from_numpy(anc).to(DEV)
    xo, c1, c2 = _step(sch._c_params(), G, t, dt, xd, sd_, gd, ad, zd, inv2v, K)
    xr, r1, r2 = S.step(osde, x, score, g, src, z, t, dt, inv2v)
    err, _ = report_err(f"smc step fp32 T={T} C={Cn} {kind}", host(xo), xr)
    print(f"smc step T={T} C={Cn} {kind}: c1 {np.abs(c1 / r1 - 1).max():.3e}, c2 {np.abs(c2 / r2 - 1).max():.3e} relative")
    assert err <= 1e-6, err
    # c1 is a sum of signed terms: where it cancels, rtol 1e-5 of the SUM is below what single-precision inputs allow, so a row may
    # instead lie within twice the distance between the restatement run in float32 and in float64 (measured: one row of (8, 3) VE,
    # |c1| = 4.5e-5, misses rtol 1e-5 by 3.0e-5 relative, 1.4e-9 absolute)
    f1, _ = S.step_sums_f32(osde, g, src, z, t, dt, inv2v)
    assert (np.abs(c1 - r1) <= np.maximum(1e-5 * np.abs(r1), 2.0 * np.abs(f1 - r1))).all(), (c1, r1, f1)
    np.testing.assert_allclose(c2, r2, rtol=1e-5)
    # the identity without an ancestor vector; rows of other series do not matter (series 1 alone, bit for bit)
    xi, i1, i2 = _step(sch._c_params(), G, t, dt, xd, sd_, gd, None, zd, inv2v, K)
    xa, a1, a2 = _step(sch._c_params(), G, t, dt, xd[K:2 * K].contiguous(), sd_[K:2 * K].contiguous(), gd[K:2 * K].contiguous(),
                       ad[K:2 * K].contiguous(), zd[K:2 * K].contiguous(), inv2v, K)
    assert torch.equal(xa, xo[K:2 * K]) and np.array_equal(a1, c1[K:2 * K]) and np.array_equal(a2, c2[K:2 * K])
    np.testing.assert_allclose(i1, S.step(osde, x, score, g, np.arange(B), z, t, dt, inv2v)[1], rtol=1e-5)
    # Philox: element e is lane e % 4 of counter offset + e / 4 -- the draws of fd_randn, also where a row straddles a group
    seed, off = 1234567, 1000
    zp = torch.empty(B, T, Cn, dtype=torch.float32, device=DEV)
    _C.check(_C.lib().fd_randn(ctx, zp.data_ptr(), zp.numel(), seed, off, torch.cuda.current_stream().cuda_stream), ctx)
    xp, p1, p2 = _step(sch._c_params(), G, t, dt, xd, sd_, gd, ad, None, inv2v, K, seed, off)
    xq, q1, q2 = _step(sch._c_params(), G, t, dt, xd, sd_, gd, ad, zp, inv2v, K)
    assert torch.equal(xp, xq) and np.array_equal(p1, q1) and np.array_equal(p2, q2)


# ---------------------------------------------------------------- the loop
def _loop_model(i):
    c, d = Cs.LOOP, Cs.loop_inputs(i)
    m, sch, sd = make_model(c, kind=d["kind"], p=d["p"], precision="fp32")
    return m, sch, d


def _impute(s, d, K, N, final_resample=True, **kw):
    c = Cs.LOOP
    return s.impute(_t(d["yn"]), torch.from_numpy(d["m"]), N, fourier_transform=d["fourier"], feature_mean=_t(d["mu"]),
                    feature_std=_t(d["sigma"]), num_samples=K, conditioning="smc", obs_std=c["obs_std"], twist_scale=c["twist_scale"],
                    ess_threshold=c["thr"], final_resample=final_resample, guidance_jacobian=d["jac"], return_info=True, **kw)


@pytest.mark.parametrize("i", range(len(Cs.LOOP_CASES)))
def test_loop_against_float64(i):
    """The whole loop through impute(): ancestors and resample flags of all N + 1 stages EQUAL the reference's (the case table keeps
    every decision 1e-3 from its threshold), ESS within that margin, the final ensemble within 1e-5 of scale.  The log weights and
    the evidence are sums of terms each held to rtol 1e-5 (||r||^2: 3.14's bound; c1, c2: the step test's), so their bound is
    4e-5 times the size of those terms (tests/smc_ref.py's `mag`; the factor covers g's own 1e-5 of scale and the 1e-5 drift of the
    state), summed over the stages for the evidence.

    Then the same loop stage by stage from the ENGINE'S OWN STATE, composed from fd_impute_guidance, fd_smc_resample and
    fd_smc_step: every stage's guidance, log weights, decision and next state are compared with the float64 formulas applied to the
    engine's previous state, so that no error is carried from stage to stage; the composition ends at the loop's own ensemble."""
    c = Cs.LOOP
    n, K, N, T, Cn = c["n"], c["K"], c["N"], c["T"], c["C"]
    B = n * K
    m, sch, d = _loop_model(i)
    tr = Cs.loop_reference(i)
    s = _sampler(m, B)
    kw = dict(prior_noise=[dev(d["zp"])], step_noise=[dev(d["zs"])], resample_noise=[torch.from_numpy(d["u"])])
    X, info = _impute(s, d, K, N, **kw)
    assert X.shape == (n, K, T, Cn) and torch.isfinite(X).all()
    assert np.array_equal(info.ancestors.numpy(), np.stack(tr["anc"]))
    assert np.array_equal(info.resampled.numpy(), np.stack(tr["resampled"]))
    assert float(np.abs(info.ess.numpy() - np.stack(tr["ess"])).max()) / K <= 1e-3
    err, _ = report_err(f"smc loop fp32 case {i} {Cs.LOOP_CASES[i]} final ensemble", X.reshape(B, T, Cn).numpy(), tr["x"])
    assert err <= 1e-5, err
    mag = np.stack(tr["mag"]).reshape(N + 1, n, K).max(axis=2)
    n_obs = d["m"].reshape(n, -1).sum(axis=1)
    ev_ref = tr["log_evidence"] + S.gaussian_constant(n_obs, c["obs_std"])
    dev_ev = np.abs(info.log_evidence.numpy() - ev_ref)
    print(f"smc loop case {i}: |log evidence - ref| {dev_ev.max():.3e} (bound {4e-5 * mag.sum(axis=0).min():.3e})")
    assert (dev_ev <= 4e-5 * mag.sum(axis=0)).all(), (dev_ev, mag.sum(axis=0))
    assert (info.log_weights == 0).all() and not info.degenerate.any()
    # final_resample=False: the particles before the final resampling and their weights
    Xw, infow = _impute(s, d, K, N, final_resample=False, **kw)
    src = (np.arange(B) // K) * K + tr["anc"][N].reshape(B)
    assert torch.equal(Xw.reshape(B, T, Cn)[torch.from_numpy(src)], X.reshape(B, T, Cn))
    assert not infow.resampled[N].any() and np.array_equal(infow.ancestors[N].numpy(), np.tile(np.arange(K), (n, 1)))
    lw_ref = tr["logw_in"][N]
    assert (np.abs(infow.log_weights.numpy().reshape(B) - lw_ref) <= 4e-5 * np.stack(tr["mag"]).sum(axis=0)).all()
    np.testing.assert_allclose(infow.log_evidence.numpy(), info.log_evidence.numpy(), rtol=1e-12)

    # ---- stage by stage from the engine's own state
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    osde = oracle_sde(d["kind"], d["p"], True, T)
    score_fn = ode_ref.model_score(Cs.loop_weights(), "transformer", c["H"])
    x0r, mr = np.repeat(d["x0"], K, 0), np.repeat(d["m"], K, 0)
    x0d, mask_t, stdt = dev(x0r), torch.from_numpy(mr), _t(d["sigma"])
    ts, dt = O.timesteps(N)
    G = sch.G_on(torch.device(DEV))
    base = (np.arange(B) // K) * K
    Xe = s.sample_prior(B, noise=dev(d["zp"]))
    logw = np.zeros(B)
    ltw_prev = np.zeros(B)
    c1 = c2 = np.zeros(B)
    ref_prev = None      # (c1, c2, c1abs, ltw of the previous state permuted) from the float64 formulas on the engine's state
    for j in range(N):
        t = float(ts[j])
        xe = host(Xe)
        ge, rn2 = s.impute_guidance(Xe, x0d, mask_t, t, fourier_transform=d["fourier"], feature_std=stdt, jacobian=d["jac"])
        gr, rr, sr = D.guidance(score_fn, osde, xe, t, x0r, mr, d["sigma"], d["fourier"], d["jac"])
        eg, _ = report_err(f"smc loop case {i} stage {j} guidance from the engine's state", host(ge), gr)
        assert eg <= 1e-5, (j, eg)
        np.testing.assert_allclose(rn2.cpu().numpy(), rr, rtol=1e-5)
        inv2v = S.twist_inv2v(osde, t, c["obs_std"], c["twist_scale"])
        ltw, ltw_r = -rn2.cpu().numpy() * inv2v, -rr * inv2v
        new = logw + (-c1 - 0.5 * c2) + (ltw - ltw_prev)
        if ref_prev is None:
            want, tol = ltw_r, 4e-5 * np.abs(ltw_r)
        else:
            want = logw + (-ref_prev[0] - 0.5 * ref_prev[1]) + (ltw_r - ref_prev[3])
            tol = 4e-5 * (ref_prev[2] + 0.5 * ref_prev[1] + np.abs(ltw_r) + np.abs(ref_prev[3]))
        assert (np.abs(new - want) <= tol + 1e-12).all(), (j, np.abs(new - want).max(), tol.min())
        got = _resample(new.reshape(n, K), d["u"][j], c["thr"])
        st = S.stage(want.reshape(n, K), d["u"][j], c["thr"], False)
        assert np.array_equal(got["anc"], st["anc"]) and np.array_equal(got["resampled"], st["resampled"]), j
        assert np.array_equal(got["anc"], info.ancestors[j].numpy()) and np.array_equal(got["resampled"], info.resampled[j].numpy())
        logw = got["logw"].reshape(B)
        src = base + got["anc"].reshape(B)
        with torch.no_grad():
            se = m(DiffusableBatch(X=Xe, timesteps=torch.full((B,), t, device=DEV)))
        es, _ = report_err(f"smc loop case {i} stage {j} score from the engine's state", host(se), sr)
        assert es <= 1e-5, (j, es)
        Xn, c1, c2 = _step(sch._c_params(), G, t, float(dt), Xe, se.contiguous(), ge, torch.from_numpy(got["anc"].reshape(B)).to(DEV),
                           dev(d["zs"][j]), inv2v, K)
        xr, r1, r2, rabs = S.step(osde, xe, sr, gr, src, d["zs"][j], t, dt, inv2v, with_abs=True)
        ex, _ = report_err(f"smc loop case {i} stage {j} proposal from the engine's state", host(Xn), xr)
        assert ex <= 1e-5, (j, ex)
        ltw_prev = ltw[src]
        ref_prev = (r1, r2, rabs, ltw_r[src])
        Xe = Xn
    # the final stage: the likelihood of x_N itself, and the resampling of the loop
    rho = S.final_rho(host(Xe), x0r, mr, d["sigma"], osde.G, d["fourier"])
    ltw_r = -rho * S.twist_inv2v(osde, None, c["obs_std"], c["twist_scale"])
    want = logw + (-ref_prev[0] - 0.5 * ref_prev[1]) + (ltw_r - ref_prev[3])
    st = S.stage(want.reshape(n, K), d["u"][N], c["thr"], True, final=True)
    assert np.array_equal(st["anc"], info.ancestors[N].numpy())
    srcN = base + st["anc"].reshape(B)
    comp = host(Xe)[srcN]
    e2, _ = report_err(f"smc loop case {i}: the composition of the three entry points against the loop", comp, X.reshape(B, T, Cn).numpy())
    assert e2 <= 1e-5, e2


# ---------------------------------------------------------------- bit anchors
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_all_false_mask_is_unguided_dps_to_the_bit(precision):
    """Nothing observed: zero residual, unit weights, no resampling before the final stage, whose uniform weights resample to the
    identity -- the rows of impute(conditioning="dps", guidance_scale=0, guidance_jacobian=False), with injected noise and with the
    Philox stream (the predictor counters are those of every other loop)."""
    cfg, n, K, N = dict(T=40, C=5, D=72, L=2, H=12), 3, 4, 6
    T, Cn = cfg["T"], cfg["C"]
    B = n * K
    m, _, _ = make_model(cfg, precision=precision)
    rs = np.random.RandomState(3)
    mu, sigma = _t(0.3 * rs.randn(T, Cn)), _t(rs.uniform(0.5, 2.0, (T, Cn)))
    obs, mask = _t(rs.randn(n, T, Cn)), torch.zeros(n, T, Cn, dtype=torch.bool)
    s = _sampler(m, B)
    base = dict(fourier_transform=True, feature_mean=mu, feature_std=sigma, num_samples=K, guidance_jacobian=False)
    zp = dev(W.randn("smc0_p", (B, T, Cn), 1))
    zs = dev(np.stack([W.randn(f"smc0_z{i}", (B, T, Cn), 1) for i in range(N)]))
    Xd = s.impute(obs, mask, N, conditioning="dps", guidance_scale=0.0, prior_noise=[zp], step_noise=[zs], **base)
    Xs, info = s.impute(obs, mask, N, conditioning="smc", obs_std=0.2, prior_noise=[zp], step_noise=[zs], return_info=True, **base)
    assert torch.isfinite(Xd).all() and torch.equal(Xs, Xd)
    assert not info.resampled[:N].any() and info.resampled[N].all()
    assert (info.ancestors == torch.arange(K, dtype=torch.int32)).all() and (info.ess == K).all()
    assert (info.log_evidence == 0).all() and not info.degenerate.any()
    torch.manual_seed(23)
    Pd = s.impute(obs, mask, N, conditioning="dps", guidance_scale=0.0, **base)
    torch.manual_seed(23)
    Ps = s.impute(obs, mask, N, conditioning="smc", obs_std=0.2, **base)
    assert torch.isfinite(Pd).all() and not torch.equal(Pd, Xd) and torch.equal(Ps, Pd)


@pytest.mark.parametrize("jac", [False, True])
def test_reproducible_and_batch_independent(jac):
    cfg, n, K, N = dict(T=13, C=5, D=72, L=2, H=12), 3, 8, 6      # T C = 65: rows straddle Philox groups
    T, Cn = cfg["T"], cfg["C"]
    B = n * K
    m, _, _ = make_model(cfg, precision="fp32")
    rs = np.random.RandomState(5)
    mu, sigma = _t(0.3 * rs.randn(T, Cn)), _t(rs.uniform(0.5, 2.0, (T, Cn)))
    obs = _t(np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(n, T, Cn))
    mask = torch.from_numpy(rs.rand(n, T, Cn) < 0.5)
    kw = dict(fourier_transform=True, feature_mean=mu, feature_std=sigma, num_samples=K, conditioning="smc", obs_std=0.3,
              guidance_jacobian=jac, return_info=True)
    s = _sampler(m, B)
    torch.manual_seed(9)
    a, ia = s.impute(obs, mask, N, **kw)
    torch.manual_seed(9)
    b, ib = s.impute(obs, mask, N, **kw)
    assert torch.isfinite(a).all() and torch.equal(a, b) and ia.resampled[:N].any()
    for f in ("log_evidence", "log_weights", "ess", "resampled", "ancestors"):
        assert torch.equal(getattr(ia, f), getattr(ib, f)), f
    # one series alone against the same series inside the batch of three (its noise and uniforms injected identically)
    zp = dev(W.randn("smcb_p", (B, T, Cn), 1))
    zs = dev(np.stack([W.randn(f"smcb_z{i}", (B, T, Cn), 1) for i in range(N)]))
    u = torch.from_numpy(rs.rand(N + 1, n))
    big, ibig = s.impute(obs, mask, N, prior_noise=[zp], step_noise=[zs], resample_noise=[u], **kw)
    one, ione = _sampler(m, K).impute(obs[1:2], mask[1:2], N, prior_noise=[zp[K:2 * K]], step_noise=[zs[:, K:2 * K]],
                                      resample_noise=[u[:, 1:2]], **kw)
    assert ibig.resampled[:N, 1].any()
    assert torch.equal(one[0], big[1]) and torch.equal(ione.ancestors[:, 0], ibig.ancestors[:, 1])
    assert torch.equal(ione.log_evidence[0], ibig.log_evidence[1]) and torch.equal(ione.ess[:, 0], ibig.ess[:, 1])


# ---------------------------------------------------------------- bf16 at the ecg shape
def test_bf16_ecg_shape():
    cfg, n, K, N = CFG_DEFAULT, 4, 16, 10
    T, Cn = cfg["T"], cfg["C"]
    mb, _, _ = make_model(cfg, precision="bf16")
    rs = np.random.RandomState(5)
    mu, sigma = _t(0.3 * rs.randn(T, Cn)), _t(rs.uniform(0.5, 2.0, (T, Cn)))
    obs = _t(np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(n, T, Cn))
    mask = torch.from_numpy(rs.rand(n, T, Cn) < 0.5)
    for jac in (True, False):
        torch.manual_seed(1)
        X, info = _sampler(mb, n * K).impute(obs, mask, N, fourier_transform=True, feature_mean=mu, feature_std=sigma, num_samples=K,
                                             conditioning="smc", obs_std=0.3, guidance_jacobian=jac, return_info=True)
        assert X.shape == (n, K, T, Cn) and torch.isfinite(X).all(), jac
        assert torch.isfinite(info.log_evidence).all() and not info.degenerate.any()
        assert (info.ess >= 1 - 1e-9).all() and (info.ess <= K + 1e-9).all()
        assert (info.ancestors >= 0).all() and (info.ancestors < K).all()
        print(f"smc bf16 ecg jacobian={jac}: {int(info.resampled.sum())} resamples, final ESS / K "
              f"{float(info.ess[-1].mean()) / K:.3f}, log evidence {info.log_evidence.tolist()}")


# ---------------------------------------------------------------- CLI
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_train_then_impute_smc(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=smcrun"], tmp_path)
    run_dir = tmp_path / "lightning_logs" / "smcrun"
    _run([str(ROOT / "cmd" / "impute.py"), "model_id=smcrun", "num_diffusion_steps=10", "sampler.sample_batch_size=40",
          "mask.kind=forecast", "mask.horizon=6", "conditioning=smc", "smc.obs_std=0.2", "guidance.jacobian=false",
          "num_samples_per_series=4", "num_series=20"], tmp_path)
    X = torch.load(run_dir / "imputations.pt")
    assert X.shape == (20, 4, 24, 4) and torch.isfinite(X).all()
    res = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert res["conditioning"] == "smc" and res["smc_obs_std"] == 0.2 and res["guidance_jacobian"] is False
    assert np.isfinite(res["smc_log_evidence_mean"]) and 0 < res["smc_ess_final_mean"] <= 1
    assert res["smc_resamples_mean"] >= 1 and 0 < res["smc_unique_final_mean"] <= 1
    assert np.isfinite(res["crps"])
