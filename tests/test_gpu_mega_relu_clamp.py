"""GPU parity of the persistent kernel's pair-form FFN loop with the relu inside the conversion (FD_RELU_CLAMP, fd_mega_params.h).

The pair-form weight image holds 2^-40 W1 | b1 and 2^40 W2; `v_cvt_pk_bf16_f32 ... clamp` turns the scaled hidden tile into relu'd bf16
in one instruction.  Four cases, each against the float64 oracle at the tolerances of tests/test_gpu_bench_instantiation.py
(forward: max <= 1e-2 of the output scale, relative rms <= 7e-3; trajectory: 1e-2, 5e-3):

  (a) the benched instantiation, three diffusion steps.  Its quarters of 4, 4, 3, 3 token tiles run both loop shapes (two pairs;
      pair + single).  plan_mega packs S = ceil(B / #CU) series into a workgroup, so the smallest batch that reaches the benched S = 2
      kernel is #CU + 1 (B = 2 plans S = 1, a seven-tile workgroup without the pair form); the first and last workgroups are checked.
  (b) a run-time-specialised shape whose three-tile quarters start on an odd tile (T = 187: 12 tiles = 3, 3, 3, 3; quarters 1 and 3 run
      single + pair).
  (c) (a)'s model with linear1 scaled by 2^s and linear2 by 2^-s in every layer, s chosen so that hidden pre-activations reach +-2^20
      for LayerNorm'd inputs: the same function in exact arithmetic (relu is positively homogeneous, powers of two are exact), so the
      oracle of the scaled weights is the reference; a saturating clamp or a negative that is not exactly 0 is an O(1) error.
  (d) a model whose linear2 fails the image's range check (one weight of 2^90 on a hidden unit that never fires): no pair-form image,
      the 16x16x32 loop on the unscaled image, and the plan says so.
"""
import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W

from .gpu_util import DEV, dev, host, make_model, oracle_sde, report_err

pytestmark = pytest.mark.gpu

ECG = dict(T=100, C=12, D=72, L=10, H=12)
ECG_STATIC = "ShapeStatic<100,72,12,12,2,3,2,10,2048>"


def _cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _fwd(model, X, t):
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    model.eval()
    return host(model(DiffusableBatch(X=dev(X), y=None, timesteps=dev(t))))


def _model_from(cfg, sd):
    m, _, _ = make_model(cfg, precision="bf16")
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    m.to(DEV)
    return m


def _check_forward(tag, out, ref, rows):
    err, rms = report_err(tag, out[rows], ref)
    assert err <= 1e-2 and rms <= 7e-3, (err, rms)
    for i, r in enumerate(rows):
        e = np.abs(out[r] - ref[i]).max() / np.abs(ref[i]).max()
        assert e <= 1.2e-2, (r, e)
    assert np.isfinite(out).all()


def test_benched_instantiation_three_steps_vs_oracle(monkeypatch):
    monkeypatch.delenv("FDIFF_MEGA_DBG", raising=False)
    B = _cu_count() + 1 + (_cu_count() & 1)             # even: every workgroup holds two series
    N = 3
    kind, p = "vp", (0.1, 20.0)
    m, sch, sd = make_model(ECG, kind=kind, p=p, precision="bf16")
    desc, S = m.plan(B)
    assert ECG_STATIC in desc and "ffn32" in desc and S == 2, desc
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    g = torch.Generator(device="cpu").manual_seed(23)
    shape = (B, ECG["T"], ECG["C"])
    zp = torch.randn(shape, generator=g)
    zs = torch.randn((N,) + shape, generator=g)
    smp = DiffusionSampler(score_model=m, sample_batch_size=B)
    got = smp.sample(num_samples=B, num_diffusion_steps=N, prior_noise=[zp.to(DEV)], step_noise=[zs.to(DEV)]).numpy().astype(np.float64)
    rows = [0, 1, B - 2, B - 1]                         # both series of the first and of the last workgroup
    ref, _ = O.sample_trajectory(sd, oracle_sde(kind, p, True, ECG["T"]), zp.numpy()[rows].astype(np.float64),
                                 [z[rows].astype(np.float64) for z in zs.numpy()], ECG["H"])
    err, rms = report_err(f"relu clamp 3-step trajectory bf16 ecg B={B} rows={rows}", got[rows], ref)
    assert err <= 1e-2 and rms <= 5e-3, (err, rms)
    for i, r in enumerate(rows):
        e = np.abs(got[r] - ref[i]).max() / np.abs(ref).max()
        assert e <= 1e-2, (r, e)
    assert np.isfinite(got).all()


def test_forward_specialised_187x1_single_then_pair_vs_oracle(monkeypatch, tmp_path_factory):
    cfg = dict(T=187, C=1, D=72, L=10, H=12)
    B = 5
    monkeypatch.setenv("FDIFF_CACHE_DIR", str(tmp_path_factory.getbasetemp() / "fdiff_jit_cache"))
    monkeypatch.setenv("FDIFF_MEGA_JIT", "1")
    monkeypatch.delenv("FDIFF_MEGA_DBG", raising=False)
    m, _, sd = make_model(cfg, precision="bf16")
    desc, S = m.plan(B)
    assert S == 1 and "(hiprtc)" in desc and "ShapeStatic<187,72,1,12,1," in desc and desc.endswith(" ffn32"), desc
    X = W.randn("rc_x_ecg187", (B, cfg["T"], cfg["C"]), 2)
    t = W.uniform("rc_t_ecg187", (B,), 2, 1e-5, 1.0)
    out = _fwd(m, X, t)
    rows = [0, 2, B - 1]
    ref = O.score_forward(sd, X[rows], t[rows], cfg["H"])
    _check_forward(f"relu clamp forward bf16 hiprtc (187, 1) B={B}", out, ref, rows)


def test_forward_hidden_values_to_2p20_vs_oracle(monkeypatch):
    monkeypatch.delenv("FDIFF_MEGA_DBG", raising=False)
    monkeypatch.delenv("FDIFF_MEGA_JIT", raising=False)
    B = _cu_count() + 1 + (_cu_count() & 1)
    sd = dict(W.make_state_dict(ECG["C"], ECG["T"], ECG["D"], ECG["L"], seed=1234))
    for l in range(ECG["L"]):
        w1 = sd[f"backbone.layers.{l}.linear1.weight"]
        # LayerNorm'd inputs have |x|^2 ~ D: a hidden unit with row norm r sees pre-activations of the order r, both signs
        s = int(np.ceil(20 - np.log2(np.sqrt((w1.astype(np.float64) ** 2).sum(axis=1)).max())))
        assert 15 <= s <= 30, s
        sd[f"backbone.layers.{l}.linear1.weight"] = np.ldexp(w1, s).astype(np.float32)
        sd[f"backbone.layers.{l}.linear1.bias"] = np.ldexp(sd[f"backbone.layers.{l}.linear1.bias"], s).astype(np.float32)
        sd[f"backbone.layers.{l}.linear2.weight"] = np.ldexp(sd[f"backbone.layers.{l}.linear2.weight"], -s).astype(np.float32)
    m = _model_from(ECG, sd)
    X = W.randn("rc_x_big", (B, ECG["T"], ECG["C"]), 2)
    t = W.uniform("rc_t_big", (B,), 2, 1e-5, 1.0)
    out = _fwd(m, X, t)
    desc, S = m.plan(B)
    assert ECG_STATIC in desc and "ffn32" in desc and S == 2, desc      # (the scaled weights pass the range check)
    rows = [0, 1, B - 2, B - 1]
    ref = O.score_forward(sd, X[rows], t[rows], ECG["H"])
    _check_forward(f"relu clamp forward bf16 ecg, hidden to 2^20, B={B}", out, ref, rows)


def test_forward_range_check_fallback_vs_oracle(monkeypatch):
    monkeypatch.delenv("FDIFF_MEGA_DBG", raising=False)
    monkeypatch.delenv("FDIFF_MEGA_JIT", raising=False)
    B = _cu_count() + 1 + (_cu_count() & 1)
    sd = dict(W.make_state_dict(ECG["C"], ECG["T"], ECG["D"], ECG["L"], seed=1234))
    l, f, d = 3, 777, 5
    w1, b1, w2 = (sd[f"backbone.layers.{l}.linear{k}"].copy() for k in ("1.weight", "1.bias", "2.weight"))
    w1[f, :] = 0.0
    b1[f] = -1.0e4                     # the unit never fires: its linear2 column multiplies an exact 0
    w2[d, f] = np.float32(2.0 ** 90)   # >= 2^87: 2^40 w is no finite bf16
    sd[f"backbone.layers.{l}.linear1.weight"], sd[f"backbone.layers.{l}.linear1.bias"] = w1, b1
    sd[f"backbone.layers.{l}.linear2.weight"] = w2
    m = _model_from(ECG, sd)
    X = W.randn("rc_x_fb", (B, ECG["T"], ECG["C"]), 2)
    t = W.uniform("rc_t_fb", (B,), 2, 1e-5, 1.0)
    out = _fwd(m, X, t)                # (the first bf16 call builds the images and with them the verdict the plan reports)
    desc, S = m.plan(B)
    assert S == 2 and desc.startswith("k_mega<3,5,3,4,ShapeModel<72,12,10,2048>>") and "ffn32" not in desc, desc
    rows = [0, 1, B - 2, B - 1]
    ref = O.score_forward(sd, X[rows], t[rows], ECG["H"])
    _check_forward(f"relu clamp range-check fallback forward bf16 ecg B={B}", out, ref, rows)
