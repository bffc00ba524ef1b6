"""CPU: covariate-conditional score models -- the parameter layout, hyper-parameters and checkpoints of ScoreModule(cond_dim=P),
argument validation, the configs and cmd/sample.py's `covariates` parsing, and the float64 restatement of tests/cov_ref.py against
itself.  No engine call: nothing here needs a GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests import cov_ref as R

ROOT = Path(__file__).resolve().parent.parent
CONF = ROOT / "cmd" / "conf"
PARENT_HPARAMS = ["n_channels", "max_len", "noise_scheduler", "fourier_noise_scaling", "d_model", "num_layers", "n_head",
                  "num_training_steps", "lr_max", "likelihood_weighting"]


def model(cond_dim=0, **kw):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    cfg = R.CFG
    return ScoreModule(n_channels=cfg["C"], max_len=cfg["T"], noise_scheduler=VPScheduler(), d_model=cfg["D"], num_layers=cfg["L"],
                       n_head=cfg["H"], cond_dim=cond_dim, **kw)


def test_layout_gains_exactly_five_trailing_tensors():
    from fourierdiffusion_amd import _C
    cfg = R.CFG
    Dm = cfg["D"]
    dims = _C.model_dims(cfg["C"], cfg["T"], Dm, cfg["H"], cfg["L"])
    old, n_old = _C.score_layout(dims)
    new, n_new = _C.score_layout(dims, cond_dim=7)
    assert new[:-5] == old
    want = [("cov_encoder.0.weight", (Dm, 7)), ("cov_encoder.0.bias", (Dm,)), ("cov_encoder.2.weight", (Dm, Dm)),
            ("cov_encoder.2.bias", (Dm,)), ("cov_encoder.null", (Dm,))]
    end = n_old - 3
    for (name, off, numel, shape, trainable), (wname, wshape) in zip(new[-5:], want):
        assert (name, shape, trainable) == (wname, wshape, True) and numel == int(np.prod(wshape))
        assert off >= end and off % 4 == 0
        end = off + numel
    assert n_new >= end
    assert _C.score_layout(dims, cond_dim=0) == (old, n_old)
    assert _C.score_layout(dims, n_classes=3, cond_dim=0) == _C.score_layout(dims, n_classes=3)
    for bad in (dict(cond_dim=65), dict(cond_dim=2, n_classes=3)):
        with pytest.raises(_C.FdError):
            _C.score_layout(dims, **bad)


def test_model_without_covariates_is_unchanged(tmp_path):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    cfg = R.CFG
    torch.manual_seed(5)
    m0 = model(0)
    torch.manual_seed(5)
    mp = ScoreModule(n_channels=cfg["C"], max_len=cfg["T"], noise_scheduler=VPScheduler(), d_model=cfg["D"], num_layers=cfg["L"],
                     n_head=cfg["H"])
    assert list(m0.hparams) == PARENT_HPARAMS == list(mp.hparams)
    assert list(m0.state_dict()) == list(mp.state_dict()) and torch.equal(m0.flat_parameters, mp.flat_parameters)
    m0.save_checkpoint(tmp_path / "a.ckpt")
    ck = torch.load(tmp_path / "a.ckpt", weights_only=False)
    assert list(ck["hyper_parameters"]) == PARENT_HPARAMS
    assert not any(k.startswith("cov_encoder") for k in ck["state_dict"]) and len(ck["state_dict"]) == 8 + 12 * cfg["L"]
    mk = model(0, n_classes=3)
    assert list(mk.hparams) == PARENT_HPARAMS + ["n_classes", "label_dropout"] and list(mk.state_dict())[-1] == "class_encoder.weight"
    # the covariate model draws the reference's weights first and its encoder behind them; the null vector starts at zero
    torch.manual_seed(5)
    mc = model(R.P)
    n = m0.flat_parameters.numel()
    assert torch.equal(mc.flat_parameters[:n], m0.flat_parameters)
    sd = mc.state_dict()
    assert list(sd)[-5:] == list(R.NAMES)
    assert not sd["cov_encoder.null"].any()
    for name, fan_in in (("cov_encoder.0", R.P), ("cov_encoder.2", cfg["D"])):      # nn.Linear's initialisation: within 1 / sqrt(fan_in)
        for part in ("weight", "bias"):
            v = sd[f"{name}.{part}"]
            assert v.any() and float(v.abs().max()) <= 1.0 / np.sqrt(fan_in)
    assert mc.hparams["cond_dim"] == R.P and mc.hparams["cond_dropout"] == 0.1 and list(mc.hparams) == PARENT_HPARAMS + ["cond_dim", "cond_dropout"]
    assert all(mc.trainable_mask()[k] is True for k in R.NAMES)


def test_checkpoint_round_trip_keeps_the_encoder_and_its_ema_copy(tmp_path):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    mc = model(R.P, cond_dropout=0.2)
    mc.load_state_dict(dict(mc.state_dict(), **{k: torch.from_numpy(v) for k, v in R.encoder(R.CFG["D"]).items()}))
    ema = mc.enable_ema()
    ema.mul_(0.5)
    mc.mark_ema_changed()
    mc.save_checkpoint(tmp_path / "c.ckpt")
    raw = ScoreModule.load_from_checkpoint(tmp_path / "c.ckpt", weights="raw")
    assert raw.cond_dim == R.P and raw.cond_dropout == 0.2 and raw.n_classes == 0
    auto = ScoreModule.load_from_checkpoint(tmp_path / "c.ckpt", weights="auto")
    assert auto.weights_loaded == "ema"
    for k in R.NAMES:
        assert torch.equal(raw.state_dict()[k], mc.state_dict()[k]) and mc.state_dict()[k].any()
        assert torch.equal(raw.ema_state_dict()[k], 0.5 * mc.state_dict()[k])
        assert torch.equal(auto.state_dict()[k], 0.5 * mc.state_dict()[k])


def test_argument_validation():
    from fourierdiffusion_amd.models.score_models import LSTMScoreModule, MLPScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    for cls in (MLPScoreModule, LSTMScoreModule):
        with pytest.raises(ValueError):
            cls(n_channels=3, max_len=20, noise_scheduler=VPScheduler(), d_model=16, num_layers=1, cond_dim=2)
        cls(n_channels=3, max_len=20, noise_scheduler=VPScheduler(), d_model=16, num_layers=1)
    for bad in (dict(cond_dim=-1), dict(cond_dim=65), dict(cond_dim=2, cond_dropout=1.5), dict(cond_dim=2, cond_dropout=-0.1),
                dict(cond_dim=2, n_classes=3)):
        with pytest.raises(ValueError):
            model(**bad)
    model(1), model(64)
    mc, m0 = model(R.P), model(0)
    ok = torch.zeros(5, R.P)
    nan, inf = ok.clone(), ok.clone()
    nan[1, 0], inf[4, 2] = float("nan"), float("inf")
    for bad in (torch.zeros(5, R.P + 1), torch.zeros(4, R.P), torch.zeros(5, R.P, dtype=torch.int64), torch.zeros(5, R.P, dtype=torch.bool),
                nan, inf, 1, 0.5, [0.0] * R.P, torch.zeros(5, R.P, 1)):
        with pytest.raises(ValueError):
            mc.covariates_on_device(bad, 5)
    with pytest.raises(ValueError):
        m0.covariates_on_device(ok, 5)
    assert mc.covariates_on_device(None, 5) is None
    c = mc.covariates_on_device(torch.arange(5 * R.P, dtype=torch.float64).view(5, R.P), 5)
    assert c.dtype == torch.float32 and c.shape == (5, R.P) and c.is_contiguous()
    one = mc.covariates_on_device(torch.tensor([1.0, 2.0, 3.0]), 4)          # (P,): every row the same covariates
    assert one.shape == (4, R.P) and one.is_contiguous() and one.tolist() == [[1.0, 2.0, 3.0]] * 4
    s0, sc = DiffusionSampler(m0, 5), DiffusionSampler(mc, 5)
    with pytest.raises(ValueError):
        s0._guided(ok, 1.0)
    assert sc._guided(None, 1.0) == (False, False) and sc._guided(None, 2.0) == (True, False)
    assert sc._guided(ok, 1.0) == (True, False) and sc._guided(ok, 0.0) == (True, False) and sc._guided(ok, 1.7) == (True, True)
    with pytest.raises(ValueError):
        sc._labels(torch.zeros(4, R.P), 5)
    assert sc._labels(torch.zeros(R.P), 5).shape == (5, R.P)
    with pytest.raises(ValueError):
        DiffusionSampler(mc, 5, corrector_steps=1).sample(5, 4, y=ok)
    for who in ("impute", "impute_guidance", "log_likelihood"):
        with pytest.raises(ValueError, match="not built"):
            sc._series_labels(ok, 5, who)


def test_covariates_parsing_of_the_sampling_front_end(tmp_path):
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticCovariatesDatamodule, TensorDatamodule
    from fourierdiffusion_amd.sampling.sampler import parse_covariates
    dm = SyntheticCovariatesDatamodule(data_dir=tmp_path, max_len=16, num_samples=20, n_channels=1)
    dm.prepare_data()
    dm.setup()
    assert parse_covariates(None, 6, 2, dm) is None and parse_covariates("null", 6, 2, dm) is None and parse_covariates(None, 6, 0) is None
    got = parse_covariates([3.0, 1.5], 4, 2, dm)                 # data units -> the model's standardised units
    want = ((torch.tensor([3.0, 1.5]) - dm.cov_mean) / dm.cov_std).to(torch.float32)
    assert got.shape == (4, 2) and got.dtype == torch.float32 and torch.allclose(got, want.expand(4, 2), atol=1e-6)
    assert torch.equal(parse_covariates([3, 1.5], 1, 2), torch.tensor([[3.0, 1.5]]))      # no statistics: as given
    data = parse_covariates("data", 25, 2, dm)
    assert data.shape == (25, 2) and torch.equal(data[:20], dm.y_test) and torch.equal(data[20:], dm.y_test[:5])
    for bad in ([1.0], [1.0, 2.0, 3.0], "many", 1.5, True, [1.0, "a"], [1.0, float("nan")], [True, 1.0]):
        with pytest.raises(ValueError):
            parse_covariates(bad, 4, 2, dm)
    with pytest.raises(ValueError):
        parse_covariates([1.0, 2.0], 4, 0, dm)
    with pytest.raises(ValueError):
        parse_covariates("data", 4, 2, TensorDatamodule(torch.zeros(4, 16, 1)))
    with pytest.raises(ValueError):
        parse_covariates("data", 4, 3, dm)


def test_configs_compose_and_instantiate(tmp_path):
    from functools import partial

    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticCovariatesDatamodule, TensorDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler, ODESampler
    cfg = compose(CONF, "train", ["score_model=covariates", "datamodule=synthetic_covariates", "fourier_transform=true",
                                  "datamodule.num_samples=400", "datamodule.max_len=32"], cwd=str(tmp_path))
    sm = instantiate(cfg.score_model)
    assert isinstance(sm, partial) and sm.func is ScoreModule and sm.keywords["cond_dim"] == 2 and sm.keywords["cond_dropout"] == 0.1
    m = sm(n_channels=1, max_len=32, num_training_steps=10)
    assert m.cond_dim == 2 and "cov_encoder.null" in m.state_dict()
    dm = instantiate(cfg.datamodule)
    assert isinstance(dm, SyntheticCovariatesDatamodule) and dm.dataset_name == "synthetic_covariates"
    dm.prepare_data()
    dm.setup()
    assert dm.X_train.shape == (400, 32, 1) and dm.y_train.shape == (400, 2) and dm.y_train.dtype == torch.float32
    assert torch.allclose(dm.y_train.mean(dim=0), torch.zeros(2), atol=1e-5) and torch.allclose(dm.y_train.std(dim=0), torch.ones(2), atol=1e-5)
    raw = dm.covariates_in_data_units(torch.cat([dm.y_train, dm.y_test]))
    assert 1.0 <= float(raw[:, 0].min()) and float(raw[:, 0].max()) <= 6.0 + 1e-4
    assert 0.5 - 1e-4 <= float(raw[:, 1].min()) and float(raw[:, 1].max()) <= 2.0 + 1e-4
    # the covariates are what the series show: the periodogram peak is the frequency (to the bin), sqrt(2) rms the amplitude
    X = torch.cat([dm.X_train, dm.X_test]).to(torch.float64)[:, :, 0]
    peak = torch.fft.rfft(X, dim=1).abs()[:, 1:].argmax(dim=1) + 1
    assert float((peak - raw[:, 0]).abs().max()) <= 1.0
    amp = np.sqrt(2.0) * X.pow(2).mean(dim=1).sqrt()
    assert float((amp - raw[:, 1]).abs().max()) <= 0.25 * 2.0
    for name, cls in (("default", DiffusionSampler), ("ode", ODESampler), ("dpm", ODESampler)):
        scfg = compose(CONF, "sample", ["model_id=abc", f"model_path={tmp_path}", f"sampler={name}", "sampler.covariates=[3.0,1.5]",
                                        "sampler.cfg_scale=2.5"])
        s = instantiate(scfg.sampler)(score_model=m)
        assert type(s) is cls and s.cfg_scale == 2.5 and list(s.covariates) == [3.0, 1.5]
        s = instantiate(compose(CONF, "sample", ["model_id=abc", f"model_path={tmp_path}", f"sampler={name}"]).sampler)(score_model=m)
        assert s.cfg_scale == 1.0 and s.covariates is None and s.labels is None
    sys.path.insert(0, str(ROOT / "cmd"))
    try:
        import train as train_cmd
    finally:
        sys.path.pop(0)
    train_cmd.check_covariates(m, dm)
    with pytest.raises(ValueError, match="no covariates"):
        train_cmd.check_covariates(m, TensorDatamodule(torch.zeros(4, 32, 1)))
    dm.y_train = torch.zeros(400, dtype=torch.long)
    with pytest.raises(ValueError, match="not floats"):
        train_cmd.check_covariates(m, dm)
    dm.y_train = torch.zeros(400, 3)
    with pytest.raises(ValueError, match="shape"):
        train_cmd.check_covariates(m, dm)
    train_cmd.check_covariates(model(0), TensorDatamodule(torch.zeros(4, 32, 1)))


def test_float64_restatement_is_consistent():
    """tests/cov_ref.py against itself: dropped rows and absent covariates read the null vector, the per-row conditioned forward
    equals the plain oracle forward on a shifted bias, the encoder gradient agrees with central differences of sum(e * dtemb), and
    the torch-autograd gradient of the loss through the encoder is that encoder gradient at autograd's own dtemb."""
    from oracle import fdiff_oracle as O
    cfg = dict(T=12, C=2, D=8, L=1, H=2)
    Pn, n = 3, 4
    enc = R.encoder(cfg["D"], Pn)
    sd, sd_cov = R.state_dict(cfg, enc)
    assert list(sd_cov)[-5:] == list(R.NAMES)
    c = R.covariates(n, Pn)
    keep = [1, 0, 1, 1]
    e = R.encode(enc, c, keep)
    nul = enc[R.NAMES[4]].astype(np.float64)
    assert np.array_equal(e[1], nul) and np.array_equal(R.encode(enc, None, n=n), np.tile(nul, (n, 1)))
    assert np.array_equal(R.encode(enc, c)[[0, 2, 3]], e[[0, 2, 3]]) and not np.array_equal(R.encode(enc, c)[1], nul)
    X = W.randn("covcpu_x", (n, cfg["T"], cfg["C"]), 1)
    t = W.uniform("covcpu_t", (n,), 1, 0.05, 1.0)
    z = W.randn("covcpu_z", (n, cfg["T"], cfg["C"]), 1)
    s = R.score(sd, e, X, t, cfg["H"])
    same = np.tile(e[0], (n, 1))
    p = dict(sd)
    p["time_encoder.dense.bias"] = sd["time_encoder.dense.bias"].astype(np.float64) + e[0]
    np.testing.assert_allclose(R.score(sd, same, X, t, cfg["H"]), O.score_forward(p, X.astype(np.float64), t, cfg["H"]), rtol=0, atol=1e-12)
    assert np.abs(s[1:] - R.score(sd, same, X, t, cfg["H"])[1:]).max() > 1e-6
    # encoder gradient against central differences, in float64
    dtemb = W.randn("covcpu_g", (n, cfg["D"]), 2)
    g = R.encoder_grad(enc, c, keep, dtemb)
    h = 1e-6
    for name in R.NAMES:
        flat = enc[name].astype(np.float64).ravel()
        for idx in list(range(0, flat.size, max(1, flat.size // 7)))[:8]:
            vals = []
            for sgn in (+1.0, -1.0):
                pert = flat.copy()
                pert[idx] += sgn * h
                vals.append(R.encoder_loss(dict(enc, **{name: pert.reshape(enc[name].shape)}), c, keep, dtemb))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[name].ravel()[idx]) <= 1e-7 * max(1.0, abs(fd)), (name, idx, fd, g[name].ravel()[idx])
    assert not R.encoder_grad(enc, c, [0] * n, dtemb)[R.NAMES[0]].any() and not R.encoder_grad(enc, c, [1] * n, dtemb)[R.NAMES[4]].any()
    gn = R.encoder_grad(enc, None, None, dtemb)
    assert not any(gn[k].any() for k in R.NAMES[:4]) and np.allclose(gn[R.NAMES[4]], dtemb.sum(axis=0))
    # the loss gradient through the encoder (torch autograd) is the encoder gradient at autograd's dtemb
    sde = O.SDEParams("vp", 0.1, 20.0, O.noise_scaling(cfg["T"], True))
    loss, ge, gbias, gtemb = R.cov_grad(sd, enc, sde, X, t, z, c, keep, cfg["H"], dim_ff=2048)
    ga = R.encoder_grad(enc, c, keep, gtemb)
    for name in R.NAMES:
        np.testing.assert_allclose(ge[name], ga[name], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(ge[R.NAMES[3]] + ge[R.NAMES[4]], gbias, rtol=1e-9, atol=1e-14)
    assert np.isfinite(loss) and loss > 0
