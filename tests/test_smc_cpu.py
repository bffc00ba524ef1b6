"""CPU: twisted sequential Monte Carlo conditioning (impute(conditioning="smc"), an extension not in the reference).  The float64
restatement of tests/smc_ref.py recovers the closed-form evidence and posterior mean of a linear-Gaussian problem; its stage has the
closed-form behaviour; the case table of the GPU loop test keeps its decisions away from the thresholds; the entry points exist,
impute checks its arguments before any device work, and cmd/conf/impute.yaml composes with the new keys.

The Gaussian check was applied by hand once to three one-token mutations of the weight formula in smc_ref.trajectory (the sign of
c1, dropping c2, not subtracting the old twist): seed 1 then misses log Z by 14.1, 35.0 and 70.5 nats in the time domain and by
13.4, 24.7 and 44.6 nats in the Fourier case, against the 0.3 and 0.45 the test allows: red under each of them."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import impute_ref as I
from tests import smc_cases as Cs
from tests import smc_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- (a) closed-form evidence and posterior mean
# Bounds.  Time domain: 0.3 nats and 0.2 (measured over seeds 1-3: log Z 0.026 / 0.077 / 0.049, posterior mean 0.029 observed and
# 0.095 hidden).  Fourier + random (mu, sigma): the residual is in data scale, sigma <= 2 times the sample-space error, so the twist
# variance takes twist_scale = sigma_max^2 = 4; measured over seeds 1-3: log Z 0.198 / 0.294 / 0.111, observed 0.038 / 0.071 / 0.041,
# hidden 0.191 / 0.598 / 0.292 (a hidden entry's posterior std reaches 1.6 there).  Its bounds are 1.5 x the three-seed maximum where
# that exceeds the time domain's: 0.45 nats, 0.2 observed, 0.9 hidden.  The smallest mutation of the weight formula moves log Z by
# 13 nats.
BOUNDS = {False: (0.3, 0.2, 0.2), True: (0.45, 0.2, 0.9)}


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("fourier", [False, True])
def test_gaussian_evidence_and_posterior_mean(fourier, seed):
    g = Cs.GAUSS
    n, K, T, C, N = g["n"], g["K"], g["T"], g["C"], g["N"]
    pr = Cs.gaussian_problem(seed, fourier)
    rs = np.random.RandomState(1000 + seed)
    B = n * K
    zp, zs, u = rs.randn(B, T, C), rs.randn(N, B, T, C), rs.rand(N + 1, n)
    tr = S.trajectory(pr["score_fn"], pr["sde"], zp, zs, u, np.repeat(pr["x0"], K, 0), np.repeat(pr["m"], K, 0), pr["sigma"],
                      fourier, K, g["obs_std"], twist_scale=4.0 if fourier else 1.0)
    ev = tr["log_evidence"] + S.gaussian_constant(pr["n_obs"], g["obs_std"])
    ym = I.forward_map(tr["x"], pr["mu"], pr["sigma"], fourier).reshape(n, K, T, C).mean(axis=1)
    err = np.abs(ym - pr["post"])
    ez, eo, eh = float(np.abs(ev - pr["logz"]).max()), float(err[pr["m"]].max()), float(err[~pr["m"]].max())
    print(f"smc gaussian fourier={fourier} seed={seed}: |log Z_hat - log Z| {ez:.3f}, posterior mean observed {eo:.3f} hidden {eh:.3f}, "
          f"{sum(int(r.sum()) for r in tr['resampled'])} resamples")
    bz, bo, bh = BOUNDS[fourier]
    assert ez <= bz and eo <= bo and eh <= bh, (ez, eo, eh)


# ---------------------------------------------------------------- (b) the stage
def test_stage_uniform_weights_are_the_identity():
    K = 7
    for u in (0.01, 0.3, 0.5, 0.99):
        st = S.stage(np.full((1, K), -3.25), [u], 1.0, True)
        assert (st["anc"][0] == np.arange(K)).all() and st["resampled"][0] and (st["logw"] == 0).all()
        assert abs(st["ess"][0] - K) < 1e-12 and abs(st["dlogz"][0] + 3.25) < 1e-12


def test_stage_one_dominant_weight():
    lw = np.full((1, 5), -800.0)
    lw[0, 3] = 2.0
    st = S.stage(lw, [0.4], 0.5, False)
    assert st["resampled"][0] and (st["anc"][0] == 3).all() and abs(st["ess"][0] - 1.0) < 1e-12
    assert abs(st["dlogz"][0] - (2.0 - np.log(5))) < 1e-12


def test_stage_infinite_and_nan_entries_have_weight_zero():
    lw = np.array([[-np.inf, 0.0, np.nan, 0.0], [-np.inf, np.nan, -np.inf, -np.inf]])
    st = S.stage(lw, [0.5, 0.5], 0.9, False)
    assert st["resampled"].tolist() == [True, False]
    assert st["anc"][0].tolist() == [1, 1, 3, 3] and abs(st["ess"][0] - 2.0) < 1e-12
    assert abs(st["dlogz"][0] - np.log(0.5)) < 1e-12
    # all weights zero: kept as it is, ESS 0, evidence -inf
    assert st["anc"][1].tolist() == [0, 1, 2, 3] and st["ess"][1] == 0 and st["dlogz"][1] == -np.inf
    assert np.array_equal(st["logw"][1], lw[1], equal_nan=True)


def test_stage_keeps_the_weights_above_the_threshold():
    lw = np.log(np.array([[1.0, 1.0, 1.0, 3.0]]))       # ESS = 36 / 12 = 3
    keep = S.stage(lw, [0.2], 0.75 - 1e-9, False)
    assert not keep["resampled"][0] and np.array_equal(keep["logw"], lw) and keep["dlogz"][0] == 0
    assert (keep["anc"][0] == np.arange(4)).all() and abs(keep["ess"][0] - 3.0) < 1e-12
    # final stage without a resample: the evidence still takes logsumexp - log K
    fin = S.stage(lw, [0.2], 0.5, False, final=True)
    assert not fin["resampled"][0] and abs(fin["dlogz"][0] - np.log(6.0 / 4.0)) < 1e-12
    cut = S.stage(lw, [0.2], 0.75 + 1e-9, False)
    assert cut["resampled"][0] and cut["anc"][0].tolist() == [0, 1, 3, 3]


# ---------------------------------------------------------------- (c) the GPU loop test's case table
@pytest.mark.parametrize("i", range(len(Cs.LOOP_CASES)))
def test_loop_cases_decide_away_from_their_thresholds(i):
    tr = Cs.loop_reference(i)
    mc, me = S.margins(tr, Cs.LOOP["thr"])
    nres = sum(int(r.sum()) for r in tr["resampled"][:-1])
    print(f"smc loop case {i} {Cs.LOOP_CASES[i]}: margins cumW {mc:.3e}, ESS {me:.3e}; {nres} resamples before the final stage")
    assert mc >= 1e-3 and me >= 1e-3, (mc, me)
    assert np.isfinite(tr["x"]).all() and np.isfinite(tr["log_evidence"]).all()


def test_loop_cases_exercise_resampling():
    """Over the table, some series resample before the final stage and some stages keep their weights."""
    flags = np.concatenate([np.stack(Cs.loop_reference(i)["resampled"][:-1]).ravel() for i in range(len(Cs.LOOP_CASES))])
    assert flags.any() and not flags.all()


# ---------------------------------------------------------------- (d) entry points, arguments, config
def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_sampler_run_impute_smc", "fd_smc_resample", "fd_smc_step"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)
    from fourierdiffusion_amd.sampling.sampler import SMCInfo
    assert {"log_evidence", "log_weights", "ess", "resampled", "ancestors", "degenerate"} <= set(SMCInfo.__dataclass_fields__)


def _sampler(T=20, C=3, corrector_steps=0):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler()
    sch.set_noise_scaling(T)
    m = ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=8, num_layers=1, n_head=4)
    return DiffusionSampler(score_model=m, sample_batch_size=4, corrector_steps=corrector_steps)


@pytest.mark.parametrize("bad", [
    dict(num_samples=None), dict(num_samples=1), dict(num_samples=1025), dict(y=0), dict(cfg_scale=2.0), dict(aggregate=2),
    dict(resample=2), dict(obs_noise=[torch.zeros(5, 8, 20, 3)]), dict(obs_std=None), dict(obs_std=0.0), dict(obs_std=-1.0),
    dict(obs_std=float("nan")), dict(twist_scale=-0.1), dict(twist_scale=float("inf")), dict(ess_threshold=1.5),
    dict(ess_threshold=-0.1), dict(final_resample=1), dict(guidance_jacobian=1), "corrector",
])
def test_impute_smc_rejects_bad_arguments(bad):
    """Every check runs before anything touches a device (this machine may have none)."""
    s = _sampler(corrector_steps=1 if bad == "corrector" else 0)
    obs, mask = torch.zeros(2, 20, 3), torch.ones(20, 3, dtype=torch.bool)
    kw = dict(conditioning="smc", num_samples=4, obs_std=0.1)
    if bad == "corrector":
        bad = {}
    kw.update(bad)
    if "aggregate" in kw:
        obs, mask = torch.zeros(2, 10, 3), torch.ones(10, 3, dtype=torch.bool)
    with pytest.raises(ValueError):
        s.impute(obs, mask, 5, fourier_transform=True, **kw)


@pytest.mark.parametrize("conditioning", ["replace", "dps"])
def test_other_conditionings_reject_the_smc_arguments(conditioning):
    s = _sampler()
    obs, mask = torch.zeros(2, 20, 3), torch.ones(20, 3, dtype=torch.bool)
    for kw in (dict(obs_std=0.1), dict(return_info=True), dict(resample_noise=[torch.zeros(6, 2)])):
        with pytest.raises(ValueError):
            s.impute(obs, mask, 5, fourier_transform=True, conditioning=conditioning, **kw)


def test_impute_config_composes_with_the_smc_keys():
    from fourierdiffusion_amd.config import compose
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "impute", overrides=[])
    assert cfg.conditioning == "replace" and cfg.smc.twist_scale == 1.0 and cfg.smc.ess_threshold == 0.5 and cfg.smc.obs_std > 0
    cfg = compose(conf, "impute", overrides=["conditioning=smc", "smc.obs_std=0.25", "smc.twist_scale=2.0", "smc.ess_threshold=0.7"])
    assert cfg.conditioning == "smc" and cfg.smc.obs_std == 0.25 and cfg.smc.twist_scale == 2.0 and cfg.smc.ess_threshold == 0.7
