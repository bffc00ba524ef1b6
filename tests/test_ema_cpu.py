"""CPU: the exponential moving average of the weights (an extension not in the reference) -- the C ABI entry exists, the warm-up
schedule is what it says, the model's weight swap (use_ema) and the checkpoint keys work on a CPU-resident model, the optimizer
state carries the update count, and the hydra `trainer=ema` option resolves."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import ema_ref as E
from tests.test_checkpoint_compat import CKPT, _pickled_globals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "cmd", "conf")


def _model(with_ema=True):
    import fdiff  # noqa: F401
    from fourierdiffusion_amd.models.score_models import ScoreModule
    m = ScoreModule.load_from_checkpoint(CKPT)
    if with_ema:
        ema = m.enable_ema()
        assert ema is m.enable_ema()                                        # idempotent
        ema.copy_(torch.arange(ema.numel(), dtype=torch.float32) * 0.5 + 3.0)      # distinct values, none equal to a raw weight
    return m


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def test_entry_point_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    assert "fd_adamw_ema_step" in declared_symbols()
    assert "fd_adamw_ema_step" in _C.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), "fd_adamw_ema_step")
    assert len(_C._PROTOS["fd_adamw_ema_step"][1]) == len(_C._PROTOS["fd_adamw_step"][1]) + 2


def test_decay_schedule():
    from fourierdiffusion_amd.optim import ema_decay_at
    assert ema_decay_at(0, 0.9999) == 0.1
    for decay in (0.9, 0.999, 0.9999):
        ds = [ema_decay_at(k, decay, True) for k in range(200000)]
        assert all(b >= a for a, b in zip(ds, ds[1:]))                      # monotone non-decreasing
        for k in (0, 1, 5, 50, 80, 81, 100, 8990, 8991, 89990, 89991, 199999):
            ramp = (1 + k) / (10 + k)
            assert ds[k] == (ramp if ramp <= decay else decay) == E.decay_at(k, decay, True)
        assert ds[-1] == decay
        assert {ema_decay_at(k, decay, False) for k in (0, 1, 10, 10 ** 6)} == {decay}
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            ema_decay_at(0, bad)
    with pytest.raises(ValueError):
        ema_decay_at(-1, 0.9)


def test_use_ema_swaps_and_restores():
    from fourierdiffusion_amd import _C
    m = _model()
    raw, ema = m.state_dict(), m.ema_state_dict()
    assert list(raw) == list(ema) and not torch.equal(raw["embedder.weight"], ema["embedder.weight"])
    assert m.ema_parameters.shape == m.flat_parameters.shape and m.ema_parameters.device == m.flat_parameters.device
    with m.use_ema() as inside:
        assert inside is m
        _same(m.state_dict(), ema)
        _same(m.ema_state_dict(), ema)
        assert m.flat_parameters.data_ptr() == m.ema_parameters.data_ptr()      # a swap, not a copy
        with pytest.raises(_C.FdError, match="nest"):
            with m.use_ema():
                pass
        _same(m.state_dict(), ema)                                          # the refused entry left the scope intact
    _same(m.state_dict(), raw)
    _same(m.ema_state_dict(), ema)
    with pytest.raises(KeyError):
        with m.use_ema():
            raise KeyError("body")
    _same(m.state_dict(), raw)
    with m.use_ema():                                                       # usable again after the exceptional exit
        _same(m.state_dict(), ema)
    _same(m.state_dict(), raw)


def test_use_ema_without_a_shadow_raises():
    from fourierdiffusion_amd import _C
    m = _model(with_ema=False)
    assert m.ema_parameters is None
    with pytest.raises(_C.FdError, match="ema_decay"):
        with m.use_ema():
            pass
    with pytest.raises(_C.FdError):
        m.ema_state_dict()


def test_load_ema_state_dict_mirrors_load_state_dict():
    m = _model(with_ema=False)
    sd = {k: v + 1.0 for k, v in m.state_dict().items()}
    m.load_ema_state_dict(sd)
    _same(m.ema_state_dict(), m.state_dict().__class__(sd))
    with pytest.raises(RuntimeError):
        m.load_ema_state_dict({k: v for k, v in sd.items() if k != "embedder.bias"})
    m.load_ema_state_dict({"embedder.bias": sd["embedder.bias"] * 2}, strict=False)
    assert torch.equal(m.ema_state_dict()["embedder.bias"], sd["embedder.bias"] * 2)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_ema_state_dict({"embedder.bias": torch.zeros(1)}, strict=False)


def test_optimizer_step_inside_the_scope_raises():
    """(the check comes before anything touches a device)"""
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.optim import FusedAdamW
    m = _model()
    opt = FusedAdamW(m, ema_decay=0.9)
    with m.use_ema():
        with pytest.raises(_C.FdError, match="use_ema"):
            opt.step()


def test_checkpoint_round_trip_and_weight_selection(tmp_path):
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.models.score_models import ScoreModule
    m = _model()
    m._ema_meta = {"decay": 0.999, "warmup": True, "num_updates": 17}
    raw, ema = m.state_dict(), m.ema_state_dict()
    path, plain = tmp_path / "ema.ckpt", tmp_path / "plain.ckpt"
    m.save_checkpoint(path, epoch=3, global_step=51)
    _model(with_ema=False).save_checkpoint(plain, epoch=3, global_step=51)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    ckp = torch.load(plain, map_location="cpu", weights_only=False)
    _same(ck["state_dict"], raw)
    _same(ck["ema_state_dict"], ema)
    assert all(t.device.type == "cpu" for t in ck["ema_state_dict"].values())
    assert ck["ema"] == {"decay": 0.999, "warmup": True, "num_updates": 17}
    assert [type(v) for v in ck["ema"].values()] == [float, bool, int]
    # the raw half is the file the same model writes without an average
    assert "ema_state_dict" not in ckp and "ema" not in ckp
    _same(ck["state_dict"], ckp["state_dict"])
    assert sorted(ck["hyper_parameters"]) == sorted(ckp["hyper_parameters"])
    for k, v in ckp["hyper_parameters"].items():
        if k == "noise_scheduler":
            assert type(ck["hyper_parameters"][k]) is type(v) and vars(ck["hyper_parameters"][k]).keys() == vars(v).keys()
        else:
            assert ck["hyper_parameters"][k] == v
    assert set(ck) - set(ckp) == {"ema_state_dict", "ema"}
    # nothing pickled that the reference cannot import
    names, ref_names = _pickled_globals(path), _pickled_globals(CKPT)
    assert "fdiff.schedulers.sde.VPScheduler" in names and names <= ref_names, names - ref_names
    # written inside the scope, the file is the same: "state_dict" stays the raw weights
    inside = tmp_path / "inside.ckpt"
    with m.use_ema():
        m.save_checkpoint(inside, epoch=3, global_step=51)
    cki = torch.load(inside, map_location="cpu", weights_only=False)
    _same(cki["state_dict"], raw)
    _same(cki["ema_state_dict"], ema)
    # weight selection
    a = ScoreModule.load_from_checkpoint(path)                              # "raw" is the default
    _same(a.state_dict(), raw)
    _same(a.ema_state_dict(), ema)
    assert a.weights_loaded == "raw" and a._ema_meta == ck["ema"]
    for w in ("ema", "auto"):
        b = ScoreModule.load_from_checkpoint(path, weights=w)
        _same(b.state_dict(), ema)
        assert b.weights_loaded == "ema" and b.ema_parameters is None      # a plain inference model
    with pytest.raises(_C.FdError, match="no averaged weights"):
        ScoreModule.load_from_checkpoint(plain, weights="ema")
    c = ScoreModule.load_from_checkpoint(plain, weights="auto")
    _same(c.state_dict(), raw)
    assert c.weights_loaded == "raw" and c.ema_parameters is None
    d = ScoreModule.load_from_checkpoint(CKPT, weights="auto")              # the reference's own file
    _same(d.state_dict(), raw)
    with pytest.raises(ValueError):
        ScoreModule.load_from_checkpoint(path, weights="best")
    # a second round trip of the loaded model reproduces the file's contents bit for bit
    again = tmp_path / "again.ckpt"
    a.save_checkpoint(again)
    ck2 = torch.load(again, map_location="cpu", weights_only=False)
    _same(ck2["state_dict"], raw)
    _same(ck2["ema_state_dict"], ema)
    assert ck2["ema"] == ck["ema"]


def test_optimizer_state_round_trips_the_update_count():
    from fourierdiffusion_amd.optim import FusedAdamW
    m = _model(with_ema=False)
    plain = FusedAdamW(m)
    assert plain.ema_decay is None and m.ema_parameters is None
    assert sorted(plain.state_dict()) == ["exp_avg", "exp_avg_sq", "lr", "step"]      # unchanged without the average
    opt = FusedAdamW(m, ema_decay=0.999, ema_warmup=False)
    assert m.ema_parameters is not None and torch.equal(m.ema_parameters, m.flat_parameters)
    assert m.ema_parameters.data_ptr() != m.flat_parameters.data_ptr()
    opt.ema_num_updates, opt.step_count = 41, 41
    sd = opt.state_dict()
    assert sd["ema_num_updates"] == 41
    other = FusedAdamW(m, ema_decay=0.999)
    other.load_state_dict(sd)
    assert other.ema_num_updates == 41 and other.step_count == 41
    old = {k: v for k, v in sd.items() if k != "ema_num_updates"}           # a state dict written before the average existed
    other.load_state_dict(old)
    assert other.ema_num_updates == 0 and other.step_count == 41
    with pytest.raises(ValueError):
        FusedAdamW(m, ema_decay=1.5)


def test_hydra_trainer_ema_option(tmp_path):
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.trainer import LearningRateMonitor, ModelCheckpoint, Trainer
    from fourierdiffusion_amd.utils.callbacks import SamplingCallback
    cfg = compose(CONF, "train", ["trainer=ema", "fourier_transform=true"], cwd=str(tmp_path))
    assert cfg.trainer.ema_decay == 0.9999 and cfg.trainer.ema_warmup is True
    tr = instantiate(cfg.trainer)
    assert isinstance(tr, Trainer) and tr.ema_decay == 0.9999 and tr.ema_warmup is True and tr.ema_eval is True
    assert tr.max_epochs == 200 and tr.gradient_clip_val == 1.0            # the default group's contents
    assert [type(c) for c in tr.callbacks] == [LearningRateMonitor, ModelCheckpoint, SamplingCallback]
    base = compose(CONF, "train", ["fourier_transform=true"], cwd=str(tmp_path))
    assert {k: v for k, v in dict(cfg.trainer).items() if not k.startswith("ema_")}.keys() == dict(base.trainer).keys()
    tr0 = instantiate(base.trainer)
    assert tr0.ema_decay is None
    tr2 = instantiate(compose(CONF, "train", ["trainer=ema", "trainer.ema_decay=0.999", "+trainer.ema_eval=false"]).trainer)
    assert tr2.ema_decay == 0.999 and tr2.ema_eval is False
    for name in ("sample", "impute", "likelihood"):
        assert compose(CONF, name, []).get("weights", "auto") == "auto"
        assert compose(CONF, name, ["weights=raw"]).weights == "raw"


def test_restatement_end_points():
    rng = np.random.default_rng(0)
    e0 = rng.standard_normal(64).astype(np.float32)
    ps = [rng.standard_normal(64).astype(np.float32) for _ in range(5)]
    out = E.recurrence(e0, ps, [0.0] * 5)
    assert all(np.array_equal(o, p.astype(np.float64)) for o, p in zip(out, ps))
    out = E.recurrence(e0, ps, [1.0] * 5)
    assert all(np.array_equal(o, e0.astype(np.float64)) for o in out)
    tol = E.tolerance(ps, E.recurrence(e0, ps, [0.5] * 5))
    assert tol.shape == (64,) and (tol > 0).all() and tol.max() < 5 * 2.0 ** -23 * 10
