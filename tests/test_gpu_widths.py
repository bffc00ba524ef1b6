"""The score network at widths OTHER than the four the persistent kernel is shaped around (VERDICT r2 missing 1: the
reference's ScoreModule takes any d_model / n_head, score_models.py:23-65).

bf16 mode at a width outside the persistent kernel's family runs fp32-MFMA projections + attention (bf16 kernel when
head_dim <= 7, exact-f32 otherwise) + the bf16 FFN kernel k_ffn_ln, instantiated for every d_model % 4 == 0 up to 143; a
width with no bf16 instantiation at all (d_model > 143, d_model % 4 != 0) must still evaluate and sample: the engine falls
back to the exact-f32 kernels and says so through ``precision_effective`` (like ``train_mode_effective`` for training).

Tolerances as everywhere: fp32 5e-6 abs (2e-5 beyond d_model 96: longer fp32 sums), bf16 <= 2e-2 of the output scale (max)
and <= 1e-2 relative rms against the float64 oracle."""
import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W

from .gpu_util import dev, host, make_model, oracle_sde, report_err

pytestmark = pytest.mark.gpu

WIDTHS = {
    # name: (cfg, expected effective eval precision, substring of the plan)
    "d64_h8": (dict(T=100, C=12, D=64, L=3, H=8), "bf16", "k_mega<3,5,2"),       # head_dim 8 inside the persistent kernel since round 4 (exact two-pass units)
    "d64_h8_long": (dict(T=300, C=4, D=64, L=2, H=8), "bf16", "per-layer"),      # the same width beyond the persistent kernel's length limit
    "d128_h8": (dict(T=60, C=5, D=128, L=2, H=8), "bf16", "per-layer"),          # head_dim 16, FFN <5,9>
    "d96_h12": (dict(T=100, C=7, D=96, L=2, H=12), "bf16", "per-layer"),         # head_dim 8, FFN <4,7>
    "d32_h4": (dict(T=48, C=3, D=32, L=2, H=4), "bf16", "k_mega<2,3,1"),         # head_dim 8 inside the persistent kernel (round 4)
    "d112_h16": (dict(T=40, C=4, D=112, L=2, H=16), "bf16", "per-layer"),        # head_dim 7: bf16 attention, FFN <4,8>
    "d80_h16": (dict(T=300, C=4, D=80, L=2, H=16), "bf16", "per-layer"),         # head_dim 5, FFN <3,6>, T > 256
    "d48_h8": (dict(T=64, C=6, D=48, L=2, H=8), "bf16", "per-layer"),            # head_dim 6, class <2,4> without its W_o image
    "d16_h4": (dict(T=40, C=3, D=16, L=2, H=4), "bf16", "k_mega"),               # newly inside the persistent kernel's family
    "d64_h16": (dict(T=100, C=12, D=64, L=2, H=16), "bf16", "per-layer"),        # head_dim 4, four k-steps of head slots
    "d160_h8": (dict(T=32, C=3, D=160, L=2, H=8), "fp32", "fp32"),               # beyond every bf16 instantiation
    "d42_h6": (dict(T=32, C=3, D=42, L=2, H=6), "fp32", "fp32"),                 # d_model % 4 != 0
    # head_dim classes beyond 16 and the scalar staging of the wide kernel (kernel by kernel: test_gpu_attention_kernels.py)
    "d128_h4": (dict(T=50, C=3, D=128, L=2, H=4), "bf16", "k_attention_wide"),   # head_dim 32: k_attention_wide<32>, 16-byte staging
    "d72_h4": (dict(T=33, C=3, D=72, L=2, H=4), "bf16", "k_attention_wide"),     # head_dim 18: wide<32>, scalar staging, odd key-tile count
    "d40_h4": (dict(T=40, C=3, D=40, L=2, H=4), "bf16", "k_attention_wide"),     # head_dim 10: wide<16>, scalar staging
    "d128_h2": (dict(T=40, C=3, D=128, L=2, H=2), "bf16", "exact-f32 kernel (head_dim > 32)"),   # head_dim 64: bf16 FFN + k_attention_f32<64>
    "d96_h2": (dict(T=40, C=3, D=96, L=2, H=2), "bf16", "exact-f32 kernel (head_dim > 32)"),     # head_dim 48: the same; fp32 mode runs f32<64> too
}


def _fwd(model, X, t):
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    model.eval()
    return host(model(DiffusableBatch(X=dev(X), y=None, timesteps=dev(t))))


@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_forward_both_modes_vs_oracle(name):
    cfg, eff, plan_sub = WIDTHS[name]
    B = 5
    X = W.randn(f"wd_x_{name}", (B, cfg["T"], cfg["C"]), 2)
    t = W.uniform(f"wd_t_{name}", (B,), 2, 1e-5, 1.0)
    m, _, sd = make_model(cfg, precision="fp32")
    ref = O.score_forward(sd, X, t, cfg["H"])
    out32 = _fwd(m, X, t)
    np.testing.assert_allclose(out32, ref, atol=2e-5 if cfg["D"] > 96 else 5e-6, rtol=0)
    m.precision = "bf16"
    assert m.precision_effective == eff, (name, m.precision_effective)
    desc, _ = m.plan(B)
    assert plan_sub in desc, desc
    out = _fwd(m, X, t)
    err, rms = report_err(f"forward {m.precision_effective} (asked bf16) {name} ({desc.split(' S=')[0]})", out, ref)
    if eff == "bf16":
        assert err <= 2e-2 and rms <= 1e-2, (err, rms)
        assert np.abs(out - out32).max() > 0, "bf16 mode must not silently run the fp32 kernels at an instantiated width"
    else:
        np.testing.assert_allclose(out, ref, atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", ["d64_h8", "d64_h8_long", "d128_h8", "d160_h8", "d128_h4"])
def test_sampler_default_precision_at_other_widths(name):
    """DiffusionSampler.sample with ``precision`` left at its default ("bf16"), as test_sampler.py of the reference drives it
    (tests/test_sampler.py: any model the config builds must sample): 10 reverse-diffusion steps with injected normals
    against the oracle's loop."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg, eff, _ = WIDTHS[name]
    B, N = 3, 10
    m, sch, sd = make_model(cfg, precision="bf16")
    m.precision = "bf16"
    zp = W.randn(f"wd_zp_{name}", (B, cfg["T"], cfg["C"]), 3)
    zs = np.stack([W.randn(f"wd_zs_{name}_{i}", (B, cfg["T"], cfg["C"]), 3) for i in range(N)])
    smp = DiffusionSampler(score_model=m, sample_batch_size=B)
    got = smp.sample(num_samples=B, num_diffusion_steps=N, prior_noise=[dev(zp)], step_noise=[dev(zs)]).numpy().astype(np.float64)
    ref, _ = O.sample_trajectory(sd, oracle_sde("vp", (0.1, 20.0), True, cfg["T"]), zp, list(zs), cfg["H"])
    err, rms = report_err(f"10-step trajectory {m.precision_effective} (default precision) {name}", got, ref)
    assert m.precision_effective == eff
    assert err <= (1e-2 if eff == "bf16" else 1e-4) and np.isfinite(got).all(), (err, rms)


@pytest.mark.parametrize("cfg", [dict(T=100, C=12, D=64, L=3, H=8), dict(T=48, C=3, D=32, L=2, H=4), dict(T=200, C=4, D=64, L=2, H=8)],
                         ids=["d64_h8", "d32_h4", "d64_h8_T200_one_head_attention_backward"])
def test_bf16_training_at_head_dim_8(cfg):
    """d_model 64 with 8 heads and d_model 32 with 4 heads (head_dim 8: no free k-slot beside a head's dims) train on the fused
    bf16 MFMA kernels since round 4 (classes <3,5,2> and <2,3,1>).  Same injected t and z, dropout off: bf16 gradients per tensor against the
    exact-f32 engine (which test_gpu_train_bf16.py anchors to the reference's autograd fixture), at that file's tolerances;
    bit-reproducible; with dropout on a finite loss and an optimizer step.  score_models.py:96-130, losses.py:39-125."""
    from fourierdiffusion_amd.optim import FusedAdamW
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    from fourierdiffusion_amd.utils.losses import get_sde_loss_fn
    from .test_gpu_train_bf16 import _compare_grads, _grads_of, batch_of
    B = 9 if cfg["T"] <= 100 else 3
    X = W.randn("wd_h8_x", (B, cfg["T"], cfg["C"]), 5)
    z = W.randn("wd_h8_z", (B, cfg["T"], cfg["C"]), 5)
    t = W.uniform("wd_h8_t", (B,), 5, 0.05, 1.0)
    res = {}
    for prec in ("fp32", "bf16"):
        m, sch, _ = make_model(cfg, precision=prec)
        m.dropout = 0.0
        fn = get_sde_loss_fn(sch, train=True)
        runs = []
        for rep in range(2 if prec == "bf16" else 1):
            m.zero_grad()
            loss = fn(m, batch_of(X, t), noise=dev(z)).item()
            runs.append((loss, m.grads.clone()))
        assert m.train_mode_effective == prec, (prec, m.train_mode_effective)
        if prec == "bf16":
            assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]), "bf16 step not bit-reproducible"
        res[prec] = (runs[0][0], _grads_of(m))
    lf, lb = res["fp32"][0], res["bf16"][0]
    assert abs(lb - lf) <= 1e-2 * abs(lf), (lb, lf)
    _compare_grads(f"d_model {cfg['D']} / {cfg['H']} heads (head_dim 8), bf16 vs exact-f32 engine, dropout off", res["bf16"][1], res["fp32"][1],
                   **(dict(max_tol=None, l2_tol=8e-2) if cfg["D"] < 64 else {}))      # (toy-width rule of test_gpu_train_bf16.py: per-tensor l2 + whole-gradient cosine, no per-tensor max bound)
    # dropout on: one optimizer step through the fused training call
    m, _, _ = make_model(cfg, precision="bf16")
    m.train()
    opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0)
    torch.manual_seed(3)
    m.zero_grad()
    loss = m.training_step(DiffusableBatch(X=dev(X)), 0)
    opt.step()
    assert m.train_mode_effective == "bf16" and torch.isfinite(loss) and torch.isfinite(m.flat_parameters).all()


def test_training_falls_back_and_says_so_at_other_widths():
    """Training at a width without bf16 training kernels runs the exact-f32 path (train_mode_effective), one optimizer step."""
    from fourierdiffusion_amd.optim import FusedAdamW
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    cfg = WIDTHS["d128_h8"][0]
    m, _, _ = make_model(cfg, precision="bf16")
    m.train_precision = "bf16"
    m.train()
    opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0)
    X = dev(W.randn("wd_train_x", (4, cfg["T"], cfg["C"]), 5))
    torch.manual_seed(3)
    m.zero_grad()
    before = m.flat_parameters.clone()
    loss = m.training_step(DiffusableBatch(X=X), 0)
    opt.step()
    assert m.train_mode_effective == "fp32" and torch.isfinite(loss) and torch.isfinite(m.flat_parameters).all()
    # the step moved every trainable tensor (head_dim 16: the exact-f32 attention backward attn_bwd_t<16> feeds in_proj and all below)
    for pname, off, numel, _, trainable in m._layout:
        moved = float((m.flat_parameters[off:off + numel] - before[off:off + numel]).abs().max())
        assert (moved > 0) == bool(trainable), (pname, moved)
    # and the fallback computes the reference's loss: dropout off, injected t and z, against the float64 oracle at the fp32 bound
    from fourierdiffusion_amd.utils.losses import get_sde_loss_fn
    m2, sch, sd = make_model(cfg, precision="bf16")
    m2.train_precision = "bf16"
    m2.dropout = 0.0
    Xn = W.randn("wd_train_x", (4, cfg["T"], cfg["C"]), 5)
    z = W.randn("wd_train_z", (4, cfg["T"], cfg["C"]), 5)
    t = W.uniform("wd_train_t", (4,), 5, 0.05, 1.0)
    m2.zero_grad()
    got = get_sde_loss_fn(sch, train=True)(m2, DiffusableBatch(X=dev(Xn), y=None, timesteps=dev(t)), noise=dev(z)).item()
    ref = O.loss_fn(sd, oracle_sde("vp", (0.1, 20.0), True, cfg["T"]), Xn, t, z, cfg["H"], False)
    assert m2.train_mode_effective == "fp32"
    np.testing.assert_allclose(got, ref, rtol=2e-5)
    assert torch.isfinite(m2.grads).all() and float(m2.grads.abs().max()) > 0
