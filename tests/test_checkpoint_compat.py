"""Lightning-checkpoint compatibility with the reference, CPU part: a checkpoint in the reference's layout
-- written by the reference itself (oracle/make_golden.py gen_ckpt -> tests/golden/reference_tiny.ckpt; the scheduler object
is pickled inside under fdiff.schedulers.sde.VPScheduler) -- loads here, and a checkpoint written here names the reference's
class paths and carries what the reference's loader consumes (pinned by that reference-written checkpoint)."""
import os
import pickletools
import zipfile

import numpy as np
import torch

from oracle import weights as W
from oracle.make_golden import CFG_TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "reference_tiny.ckpt")


def test_reference_checkpoint_loads_through_the_alias():
    import fdiff  # noqa: F401  (the alias package: fdiff.schedulers.sde -> fourierdiffusion_amd.schedulers.sde)
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    ck = torch.load(CKPT, map_location="cpu", weights_only=False)
    assert ck["pytorch-lightning_version"] and ck["hparams_name"] == "kwargs"
    sch = ck["hyper_parameters"]["noise_scheduler"]
    assert type(sch) is VPScheduler and sch.beta_0 == 0.1 and sch.beta_1 == 20.0 and sch.noise_scaling is True
    m = ScoreModule.load_from_checkpoint(CKPT)
    assert (m.n_channels, m.max_len, m.d_model, m.num_layers, m.n_head) == (3, 20, 8, 2, 4)
    assert isinstance(m.noise_scheduler, VPScheduler) and m.noise_scheduler.G.shape == (20,)
    want = W.make_state_dict(CFG_TINY["C"], CFG_TINY["T"], CFG_TINY["D"], CFG_TINY["L"], seed=1234)
    got = m.state_dict()
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        if k == "pos_encoder.pe.weight":
            continue        # (rows above the max_norm are renormalised on load, as the reference does on first use)
        np.testing.assert_array_equal(got[k].cpu().numpy(), v, err_msg=k)


def _pickled_globals(path):
    with zipfile.ZipFile(path) as z:
        name = [n for n in z.namelist() if n.endswith("data.pkl")][0]
        ops = pickletools.genops(z.read(name))
        out, strings = set(), []
        for op, arg, _ in ops:
            if op.name in ("SHORT_BINUNICODE", "BINUNICODE", "UNICODE"):
                strings.append(arg)
            elif op.name == "STACK_GLOBAL" and len(strings) >= 2:
                out.add(f"{strings[-2]}.{strings[-1]}")
            elif op.name == "GLOBAL":
                out.add(arg.replace(" ", "."))
        return out


def test_checkpoint_written_here_names_reference_paths_and_round_trips(tmp_path):
    import fdiff  # noqa: F401
    from fourierdiffusion_amd.models.score_models import ScoreModule
    m = ScoreModule.load_from_checkpoint(CKPT)
    path = tmp_path / "epoch=0-val_loss=0.50.ckpt"
    m.save_checkpoint(path, epoch=0, global_step=7)
    names = _pickled_globals(path)
    assert "fdiff.schedulers.sde.VPScheduler" in names
    assert not [n for n in names if n.startswith("fourierdiffusion_amd")], names      # nothing the reference cannot import
    again = ScoreModule.load_from_checkpoint(path)
    for k, v in m.state_dict().items():
        np.testing.assert_array_equal(again.state_dict()[k].cpu().numpy(), v.cpu().numpy(), err_msg=k)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    for key in ("epoch", "global_step", "pytorch-lightning_version", "state_dict", "hparams_name", "hyper_parameters"):
        assert key in ck


def test_reference_loads_a_checkpoint_written_here(tmp_path):
    """What the reference needs to load a checkpoint written here, pinned by the checkpoint the reference wrote itself
    (reference_tiny.ckpt): unpickling names no global that the reference's own checkpoint does not name, the hyper-parameters
    are the reference's (ScoreModule(**hyper_parameters) builds the same model), the state_dict has the reference model's keys,
    shapes and values (load_state_dict(strict=True)), and those weights give the reference's golden forward output through the
    oracle's restatement of the reference forward."""
    import fdiff  # noqa: F401
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from oracle import fdiff_oracle as O
    path = tmp_path / "engine.ckpt"
    ScoreModule.load_from_checkpoint(CKPT).save_checkpoint(path)
    names, ref_names = _pickled_globals(path), _pickled_globals(CKPT)
    assert "fdiff.schedulers.sde.VPScheduler" in names and names <= ref_names, names - ref_names
    ck = torch.load(path, map_location="cpu", weights_only=False)
    ref = torch.load(CKPT, map_location="cpu", weights_only=False)
    hp, hr = ck["hyper_parameters"], ref["hyper_parameters"]
    assert sorted(hp) == sorted(hr)
    for k, v in hr.items():
        if k == "noise_scheduler":
            assert (type(hp[k]), hp[k].beta_0, hp[k].beta_1, hp[k].noise_scaling) == (type(v), v.beta_0, v.beta_1, v.noise_scaling)
        else:
            assert type(hp[k]) is type(v) and hp[k] == v, (k, hp[k], v)
    sd, sr = ck["state_dict"], ref["state_dict"]
    assert sorted(sd) == sorted(sr)
    for k, v in sr.items():
        assert sd[k].dtype == v.dtype and sd[k].shape == v.shape, k
        np.testing.assert_array_equal(sd[k].numpy(), v.numpy(), err_msg=k)
    X = W.randn("score_x_tiny", (3, 20, 3), 2)
    t = W.uniform("score_t_tiny", (3,), 2, 1e-5, 1.0)
    out = O.score_forward({k: v.numpy() for k, v in sd.items()}, X, t, hp["n_head"])
    g = np.load(os.path.join(ROOT, "tests", "golden", "score_forward.npz"))
    np.testing.assert_allclose(out, g["fast_tiny"], atol=5e-6, rtol=0)
