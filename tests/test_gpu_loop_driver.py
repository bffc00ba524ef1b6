"""GPU: every step-by-step sampling loop runs through one engine driver (csrc/fd_loop.h, fd_step_loop), which either fills the t
vectors of all evaluations in one launch or, under FDIFF_SAMPLER_FILL_PER_STEP, refills one vector before every evaluation.  Same
values on both paths, so every loop form must give bit-identical samples (FDIFF_SAMPLER_STEPWISE=1 keeps the bf16 model off the
fused loop forms, which do not use the driver).

Shapes: (T=48, C=8), the 16-byte branches of the step kernels, batch 4; (T=9, C=3) with batch 3, B T C = 81: the scalar branches and
a ragged last Philox group.  d_model 24, 2 layers, 4 heads, 3 classes, 5 steps.  Noise from the engine's Philox stream, except the
corrector's on the small model (fd_langevin_step draws on the device only when T C % 4 == 0).
"""
import os

import numpy as np
import pytest
import torch

from tests import cfg_ref as R
from tests.gpu_util import DEV, make_model

pytestmark = pytest.mark.gpu
N = 5
MODELS = {"T48C8": (dict(T=48, C=8, D=24, L=2, H=4), 4), "T9C3": (dict(T=9, C=3, D=24, L=2, H=4), 3)}
# (id, method, keyword arguments, class-conditional model)
LOOPS = [
    ("sample", "sample", {}, False),
    ("sample_pc2", "sample", {"corrector_steps": 2}, False),
    ("ode_euler", "sample_ode", {"solver": "euler"}, False),
    ("ode_heun", "sample_ode", {"solver": "heun"}, False),
    ("ode_ddim", "sample_ode", {"solver": "ddim"}, False),
    ("ode_dpmpp2m", "sample_ode", {"solver": "dpmpp2m"}, False),
    ("impute_rep2", "impute", {"num_samples": 2}, False),
    ("cfg_sample", "sample", {"cfg_scale": 2.0}, True),
    ("cfg_ode_heun", "sample_ode", {"solver": "heun", "cfg_scale": 2.0}, True),
    ("cfg_ode_dpmpp2m", "sample_ode", {"solver": "dpmpp2m", "cfg_scale": 2.0}, True),
]
CASES = [(mid, "fp32", loop) for mid in MODELS for loop in LOOPS] + \
        [("T48C8", "bf16", loop) for loop in LOOPS if loop[0] in ("sample", "cfg_ode_heun")]
ENV_KEYS = ("FDIFF_SAMPLER_STEPWISE", "FDIFF_SAMPLER_FILL_PER_STEP")


def make_cond(cfg, precision):
    """A class-conditional ScoreModule (R.K classes) with the oracle's weights and the class table of tests/cfg_ref.py."""
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler(0.1, 20.0, fourier_noise_scaling=True)
    sch.set_noise_scaling(cfg["T"])
    m = ScoreModule(n_channels=cfg["C"], max_len=cfg["T"], noise_scheduler=sch, fourier_noise_scaling=True, d_model=cfg["D"],
                    num_layers=cfg["L"], n_head=cfg["H"], n_classes=R.K)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.state_dict(cfg, R.table(cfg["D"]))[1].items()})
    m.to(DEV)
    m.precision = m.train_precision = precision
    return m


def run_loop(mid, precision, loop, seed=11, injected=False):
    """One launch of the loop `loop` on model `mid`: a CPU tensor.  injected: every N(0, 1) draw comes from a seeded host generator
    instead of the engine's Philox stream."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    _, method, kw, cond = loop
    kw = dict(kw)
    cfg, B = MODELS[mid]
    T, Cn = cfg["T"], cfg["C"]
    m = make_cond(cfg, precision) if cond else make_model(cfg, precision=precision)[0]
    n_corr = kw.pop("corrector_steps", 0)
    # (a two-evaluation guided loop cuts its launches to half a batch: twice the batch keeps all B series in one launch)
    s = DiffusionSampler(score_model=m, sample_batch_size=2 * B if cond else B, corrector_steps=n_corr)
    rs = np.random.RandomState(seed)
    randn = lambda *shape: torch.from_numpy(rs.randn(*shape).astype(np.float32)).to(DEV)
    if cond:
        kw["y"] = torch.arange(B) % R.K
    if method == "impute":
        rows = B * kw["num_samples"]
        obs, mask = randn(B, T, Cn).cpu(), torch.from_numpy(rs.rand(B, T, Cn) < 0.5)
        if injected:
            kw.update(prior_noise=[randn(rows, T, Cn)], step_noise=[randn(N, rows, T, Cn)], obs_noise=[randn(N, rows, T, Cn)])
        torch.manual_seed(seed)
        return s.impute(obs, mask, N, fourier_transform=True, **kw).reshape(rows, T, Cn)
    if injected:
        kw["prior_noise"] = [randn(B, T, Cn)]
        if method == "sample":
            kw["step_noise"] = [randn(N, B, T, Cn)]
    if n_corr and (injected or (T * Cn) % 4):
        kw["corrector_noise"] = [randn(N, n_corr, B, T, Cn)]
    torch.manual_seed(seed)
    return getattr(s, method)(B, N, **kw)


@pytest.mark.parametrize("mid,precision,loop", CASES, ids=[f"{c[0]}-{c[1]}-{c[2][0]}" for c in CASES])
def test_step_table_and_fill_per_step_are_bit_identical(mid, precision, loop):
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    outs = []
    try:
        os.environ["FDIFF_SAMPLER_STEPWISE"] = "1"
        for per_step in (False, True):
            if per_step:
                os.environ["FDIFF_SAMPLER_FILL_PER_STEP"] = "1"
            else:
                os.environ.pop("FDIFF_SAMPLER_FILL_PER_STEP", None)
            outs.append(run_loop(mid, precision, loop))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
