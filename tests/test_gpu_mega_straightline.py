"""The persistent kernel's owner phases (embed epilogue, out-proj + LayerNorm1, FFN combine + LayerNorm2, fragment writes) take the
feature-padding guard of the last 16-row tile as selects on values with clamped vector indices (csrc/fd_mega_kernel.h: row_live /
row_clamped).  Which lane groups of that tile are live depends on d_model mod 16, so every width class is run, at shapes where

  * the batch is odd (B = 3: the last workgroup holds one series),
  * T = 20 gives two token tiles, the second ragged (4 real tokens),
  * and, at d_model 72 with T = 40 and B = 5, some waves own a single tile in the owner phases (the "first tile twice" path).

bf16 forward against the float64 oracle with the bounds of test_gpu_widths.py (<= 2e-2 of the output scale max, <= 1e-2 relative
rms); the bench instantiation (ShapeStatic, two series per workgroup) with the bounds of test_gpu_bench_instantiation.py, and its
sampler loop must be bit-reproducible from one Philox state -- the basis of comparing two builds' samples with array_equal."""
import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W

from .gpu_util import dev, host, make_model, report_err

pytestmark = pytest.mark.gpu

ECG = dict(T=100, C=12, D=72, L=10, H=12)                 # the bench workload and its static instantiation, as in
ECG_STATIC = "ShapeStatic<100,72,12,12,2,3,2,10,2048>"     # test_gpu_bench_instantiation.py

# d_model / heads: the last row tile's live lane groups (rows 16 (DT - 1) + 4 g < d_model)
CLASSES = {
    "d72_h12": dict(D=72, H=12),     # g < 2
    "d60_h12": dict(D=60, H=12),     # <2,4,3>: g < 3
    "d64_h8": dict(D=64, H=8),       # the last tile holds only the bias slot
    "d32_h4": dict(D=32, H=4),       # the same, two row tiles below
    "d24_h4": dict(D=24, H=4),       # g < 2
    "d16_h4": dict(D=16, H=4),       # bias slot only
    "d8_h4": dict(D=8, H=4),         # one row tile, g < 2
}


def _fwd(model, X, t):
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    model.eval()
    return host(model(DiffusableBatch(X=dev(X), y=None, timesteps=dev(t))))


def _check_forward(name, cfg, B):
    X = W.randn(f"sl_x_{name}", (B, cfg["T"], cfg["C"]), 2)
    t = W.uniform(f"sl_t_{name}", (B,), 2, 1e-5, 1.0)
    m, _, sd = make_model(cfg, precision="bf16")
    desc, _ = m.plan(B)
    assert "k_mega" in desc, desc
    out = _fwd(m, X, t)
    ref = O.score_forward(sd, X, t, cfg["H"])
    err, rms = report_err(f"forward bf16 {name} B={B} T={cfg['T']} ({desc.split(' S=')[0]})", out, ref)
    assert np.isfinite(out).all()
    assert err <= 2e-2 and rms <= 1e-2, (err, rms)


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_forward_every_width_class_ragged_tile_odd_batch(name):
    _check_forward(name, dict(T=20, C=3, L=2, **CLASSES[name]), B=3)


def test_forward_d72_waves_owning_a_single_tile():
    _check_forward("d72_h12_T40", dict(T=40, C=3, L=2, **CLASSES["d72_h12"]), B=5)


def test_forward_guarded_form_four_tile_shape_model():
    """The 4-tile ShapeModel kernel keeps the guarded form of the owner phases (STRAIGHT is off for it): 16 token tiles, the last ragged."""
    cfg = dict(T=250, C=3, D=72, L=10, H=12)
    m, _, _ = make_model(cfg, precision="bf16")
    assert "k_mega<3,5,3,4,ShapeModel<72,12,10,2048>" in m.plan(2)[0], m.plan(2)[0]
    _check_forward("d72_h12_T250_shape_model", cfg, B=2)


def test_bench_instantiation_forward_and_bit_reproducible_sampler():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    B = torch.cuda.get_device_properties(0).multi_processor_count + 1     # the smallest batch with two series in a workgroup
    m, _, sd = make_model(ECG, precision="bf16")
    desc, S = m.plan(B)
    assert ECG_STATIC in desc and S == 2, desc
    X = W.randn("sl_x_ecg", (B, ECG["T"], ECG["C"]), 2)
    t = W.uniform("sl_t_ecg", (B,), 2, 1e-5, 1.0)
    out = _fwd(m, X, t)
    rows = [0, 1, B // 2 - (B // 2) % 2, B // 2 - (B // 2) % 2 + 1, B - 1]     # both series of the first and a middle workgroup, the lone last one
    ref = O.score_forward(sd, X[rows], t[rows], ECG["H"])
    err, rms = report_err(f"forward bf16 {desc.split(' S=')[0]} B={B} rows={rows}", out[rows], ref)
    assert np.isfinite(out).all()
    assert err <= 1e-2 and rms <= 7e-3, (err, rms)
    for i, r in enumerate(rows):
        e = np.abs(out[r] - ref[i]).max() / np.abs(ref[i]).max()
        assert e <= 1.2e-2, (r, e)
    smp = DiffusionSampler(score_model=m, sample_batch_size=B)
    runs = []
    for _ in range(2):
        torch.manual_seed(123)
        runs.append(smp.sample(num_samples=B, num_diffusion_steps=5).numpy())
    assert np.isfinite(runs[0]).all()
    assert np.array_equal(runs[0], runs[1]), "5-step sampler run is not bit-reproducible from one Philox state"
