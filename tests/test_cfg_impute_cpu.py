"""CPU: labels and classifier-free guidance in conditional sampling and the likelihood -- the float64 restatement of
tests/cfg_impute_ref.py against tests/impute_ref.py and tests/dps_ref.py on bias-shifted weights, the argument validation of
``impute`` / ``impute_guidance`` / ``log_likelihood`` that runs before any device work, the `labels` parsing of cmd/impute.py and
cmd/likelihood.py and their configs.  No engine call: nothing here needs a GPU."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W
from tests import cfg_impute_ref as G
from tests import cfg_ref as R
from tests import dps_ref as D
from tests import impute_ref as I

ROOT = Path(__file__).resolve().parent.parent
CONF = ROOT / "cmd" / "conf"
SMALL = dict(T=12, C=2, D=8, L=1, H=2)


def model(n_classes=0, cfg=R.CFG, **kw):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    return ScoreModule(n_channels=cfg["C"], max_len=cfg["T"], noise_scheduler=VPScheduler(), d_model=cfg["D"], num_layers=cfg["L"],
                       n_head=cfg["H"], n_classes=n_classes, **kw)


def _setup(cfg, B, N, fourier, seed):
    T, Cn = cfg["T"], cfg["C"]
    tab = R.table(cfg["D"])
    sd, _ = R.state_dict(cfg, tab)
    sde = O.SDEParams("vp", 0.1, 20.0, O.noise_scaling(T, True))
    mu, sigma, yn, m, x0 = G.conditioning(T, Cn, B, "random", seed, fourier)
    zp = W.randn(f"cic_p_{T}", (B, T, Cn), seed)
    zs = [W.randn(f"cic_s{i}_{T}", (B, T, Cn), seed) for i in range(N)]
    zo = [W.randn(f"cic_o{i}_{T}", (B, T, Cn), seed) for i in range(N)]
    return tab, sd, sde, sigma, m, x0, zp, zs, zo


@pytest.mark.parametrize("fourier", [True, False])
def test_one_label_at_w1_is_the_bias_shifted_unlabelled_trajectory(fourier):
    """All rows on label k, w = 1: the guided replace trajectory is impute_ref.impute_trajectory on the weights with table[k] added
    to time_encoder.dense.bias -- the same float64 operations in the same order, so the bound is float64 rounding."""
    cfg, B, N, k = SMALL, 3, 4, 2
    tab, sd, sde, sigma, m, x0, zp, zs, zo = _setup(cfg, B, N, fourier, 3)
    got = G.replace_trajectory(sd, tab, sde, zp, zs, zo, x0, m, sigma, fourier, [k] * B, 1.0, cfg["H"])
    ref = I.impute_trajectory(G.shifted(sd, tab, k), sde, zp, zs, zo, x0, m, sigma, fourier, cfg["H"])
    err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
    print(f"[cfg-impute] float64 self-check fourier={fourier}: {err:.3e}")
    assert err <= 1e-12, err
    # and w = 0 ignores the labels: the null row of the table
    got0 = G.replace_trajectory(sd, tab, sde, zp, zs, zo, x0, m, sigma, fourier, [k] * B, 0.0, cfg["H"])
    ref0 = I.impute_trajectory(G.shifted(sd, tab, R.K), sde, zp, zs, zo, x0, m, sigma, fourier, cfg["H"])
    assert np.abs(got0 - ref0).max() <= 1e-12 * max(1.0, np.abs(ref0).max())
    assert np.abs(got - got0).max() > 1e-3


def test_guided_dps_gradient_is_the_weighted_sum_of_the_two_models():
    """The derivation behind the paired VJP: with u fixed by the guided score, J_guided^T v = w J_c^T v + (1 - w) J_u^T v."""
    cfg, B, w, t = SMALL, 2, 1.7, 0.4
    tab, sd, sde, sigma, m, x0, zp, _, _ = _setup(cfg, B, 1, True, 5)
    y = [0, 2]
    fn = R.guided_score_fn(sd, tab, y, w, cfg["H"])
    fc, fu = R.guided_score_fn(sd, tab, y, 1.0, cfg["H"]), R.guided_score_fn(sd, tab, None, 1.0, cfg["H"])
    x = np.asarray(zp, dtype=np.float64)
    alpha, s = D.coef(sde, t)
    _, u = D.residual(x, fn(x, t), x0, m, sigma, sde.G, alpha, s, True)
    v = (s * s) * (sde.G ** 2)[None, :, None] * u
    dx = D.vjp(fn, x, t, v)
    dx2 = w * D.vjp(fc, x, t, v) + (1.0 - w) * D.vjp(fu, x, t, v)
    err = np.abs(dx - dx2).max() / np.abs(dx).max()
    print(f"[cfg-impute] J_guided^T v against w J_c^T v + (1 - w) J_u^T v: {err:.3e}")
    assert err <= 1e-6, err          # central differences of step 1e-7 (tests/likelihood_ref.jvp)
    g, rn2 = G.dps_guidance(sd, tab, sde, x, t, x0, m, sigma, True, y, w, cfg["H"], True)
    assert np.abs(g - (2.0 / alpha) * (u + dx)).max() <= 1e-12 * np.abs(g).max() and (rn2 > 0).all()


def test_argument_validation_before_any_device_work():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    T, Cn = R.CFG["T"], R.CFG["C"]
    m0, mk = model(0), model(R.K)
    s0, sk = DiffusionSampler(m0, 8), DiffusionSampler(mk, 8)
    obs, mask = torch.zeros(5, T, Cn), torch.ones(5, T, Cn, dtype=torch.bool)
    for kw in (dict(y=1), dict(cfg_scale=2.0), dict(y=torch.zeros(5, dtype=torch.int64))):
        with pytest.raises(ValueError):
            s0.impute(obs, mask, 4, fourier_transform=True, **kw)
        with pytest.raises(ValueError):
            s0.impute_guidance(obs, obs, mask, 0.5, fourier_transform=True, **kw)
    with pytest.raises(ValueError):
        s0.log_likelihood(obs, 4, y=1)
    for bad in (float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError):
            sk.impute(obs, mask, 4, fourier_transform=True, y=1, cfg_scale=bad)
        with pytest.raises(ValueError):
            sk.impute_guidance(obs, obs, mask, 0.5, fourier_transform=True, y=1, cfg_scale=bad)
    for s in (s0, sk):
        with pytest.raises(ValueError, match="cfg_scale"):
            s.log_likelihood(obs, 4, y=None, cfg_scale=1.0)
        with pytest.raises(TypeError):
            s.log_likelihood(obs, 4, guidance=1.0)
    # one label per SERIES, in range
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(5), R.K + 1, -1, torch.tensor([0, 1, 2, 3, 4])):
        with pytest.raises(ValueError):
            sk._series_labels(bad, 5, "impute")
    assert sk._series_labels(None, 5, "impute") is None
    # the signatures keep today's positional order and gain the two keywords last
    import inspect
    for fn, new in ((DiffusionSampler.impute, ["y", "cfg_scale"]), (DiffusionSampler.impute_guidance, ["y", "cfg_scale"])):
        assert list(inspect.signature(fn).parameters)[-2:] == new
    assert inspect.signature(DiffusionSampler.impute).parameters["cfg_scale"].default == 1.0
    assert "y" in inspect.signature(DiffusionSampler.log_likelihood).parameters


def test_labels_setting_of_the_front_ends():
    from types import SimpleNamespace

    from fourierdiffusion_amd.sampling.sampler import series_labels
    dm = SimpleNamespace(y_test=torch.tensor([0, 2, 1, 1, 0, 2]))
    assert series_labels(None, dm, 4, 3) is None and series_labels("null", dm, 4, 3) is None and series_labels(None, dm, 4, 0) is None
    assert series_labels("data", dm, 4, 3).tolist() == [0, 2, 1, 1] and series_labels("data", dm, 6, 3).dtype == torch.int64
    assert series_labels(2, dm, 3, 3).tolist() == [2, 2, 2] and series_labels("1", dm, 2, 3).tolist() == [1, 1]
    for spec, d, n, K in (("data", SimpleNamespace(y_test=None), 4, 3), ("data", SimpleNamespace(), 4, 3), ("data", dm, 4, 2),
                          ("data", dm, 4, 0), ("data", dm, 7, 3), (3, dm, 4, 3), ("balanced", dm, 4, 3), (1, dm, 4, 0)):
        with pytest.raises(ValueError):
            series_labels(spec, d, n, K)


def test_configs_carry_the_new_keys_with_inert_defaults(tmp_path):
    from fourierdiffusion_amd.config import compose
    imp = compose(CONF, "impute", ["model_id=abc", f"model_path={tmp_path}"])
    assert imp.labels is None and float(imp.cfg_scale) == 1.0
    imp = compose(CONF, "impute", ["model_id=abc", f"model_path={tmp_path}", "labels=data", "cfg_scale=1.5"])
    assert imp.labels == "data" and float(imp.cfg_scale) == 1.5
    ll = compose(CONF, "likelihood", ["model_id=abc", f"model_path={tmp_path}"])
    assert ll.labels is None and "cfg_scale" not in ll
    assert compose(CONF, "likelihood", ["model_id=abc", f"model_path={tmp_path}", "labels=2"]).labels == 2


def test_abi_declares_the_new_entry_points():
    from fourierdiffusion_amd import _C
    header = (ROOT / "include" / "fdiff_hip.h").read_text()
    for name, base in (("fd_sampler_run_impute_cfg", "fd_sampler_run_impute_rep"), ("fd_impute_guidance_cfg", "fd_impute_guidance"),
                       ("fd_sampler_run_impute_dps_cfg", "fd_sampler_run_impute_dps")):
        assert f"int {name}(" in header
        assert len(_C._PROTOS[name][1]) == len(_C._PROTOS[base][1]) + 2      # y and cfg_scale
    assert "int fd_score_get_labels(" in header and "fd_score_get_labels" in _C._PROTOS
