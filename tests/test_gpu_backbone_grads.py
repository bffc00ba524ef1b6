"""GPU: training of the MLP / LSTM backbones (csrc/fd_backbones.hip) element by element against float64 beyond the toy shape.

Reference: tests/bb_autograd_ref.py (torch CPU autograd in float64, the engine's dropout masks restated from the call's Philox key),
pinned by tests/test_bb_autograd_ref_cpu.py; cases and what each crosses: tests/bb_shapes_ref.py (computed once).  Per case: a training
forward with the dropout key pinned (torch.manual_seed before the forward: the key is the generator's first draw), backward(u), a fresh
forward and input_vjp(u).

    score                      5e-6 * max(1, max|ref|)             the forward bound of tests/test_gpu_backbones.py
    every gradient tensor, dx  max|got - ref| <= 1e-5 * max|ref|   what tests/test_gpu_vjp_shapes.py holds the exact-f32 engine to against
                                                                   float64; the float32 restatement alone costs <= 1.04e-6 at these
                                                                   cases (bb_shapes_ref.F32_MEASURED), asserted <= 2.5e-6 on the CPU
    dropout-on cases           the score differs from the float64 score without dropout by more than the score bound
    time_encoder.W             gradient exactly 0 (frozen); lstm_T1: weight_hh gradient exactly 0 (no recurrence)
    bias_ih / bias_hh          bit-equal (the engine writes one column sum to both)
    LSTM cases                 the eval forward (TRAIN = false kernels, ping-pong buffers) against O.lstm_score_forward, 5e-6 rule

Every measured value is logged by tests/gpu_util.report_err."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from tests import bb_shapes_ref as S
from tests.gpu_util import DEV, dev, host, log_line, report_err
from tests.test_gpu_backbones import batch_of, make_bb

pytestmark = pytest.mark.gpu
SCORE_TOL = 5e-6
GRAD_TOL = 1e-5


def _model(tag):
    c = S.CASES[tag]
    m, _, _ = make_bb(c["kind"], dict(T=c["T"], C=c["C"], D=c["D"], L=c["L"]), c["F"], seed=S.WEIGHT_SEED)
    m.train()
    m.dropout = c["p"]
    return m


def _forward(m, cs):
    """A training forward whose dropout key is bb_shapes_ref.dropout_key() at offset 0."""
    from fourierdiffusion_amd import _rng
    assert _rng.base_offset() == S.OFFSET
    torch.manual_seed(S.KEY_SEED)
    return m(batch_of(cs["x"], cs["t"]))


def _forward_backward(m, cs):
    _forward(m, cs)
    return m.backward(dev(cs["u"]))


@pytest.mark.parametrize("tag", list(S.CASES))
def test_score_and_gradients_elementwise_vs_float64(tag):
    cs = S.case(tag)
    c, ref = cs["cfg"], cs["ref"]
    label = f"backbone {tag} T={c['T']} C={c['C']} D={c['D']} d_mlp={c['F']} L={c['L']} B={c['B']} p={c['p']}"
    m = _model(tag)
    score = host(_forward(m, cs))
    m.backward(dev(cs["u"]))
    views = m.grad_views()
    got = {k: host(v) for k, v in views.items()}
    _forward(m, cs)
    dx = host(m.input_vjp(dev(cs["u"])))
    assert "backbone" in m.plan(c["B"])[0]

    tol = SCORE_TOL * max(1.0, np.abs(ref["score"]).max())
    report_err(f"{label} score vs float64", score, ref["score"])
    assert np.abs(score - ref["score"]).max() <= tol, np.abs(score - ref["score"]).max()
    if c["p"] > 0:
        moved = float(np.abs(score - cs["score0"]).max())
        log_line(f"[parity] {label} score: dropout moves it by {moved:.3e} (bound of the comparison {tol:.3e})")
        assert moved > tol

    assert set(got) == set(ref["grads"]) | {"time_encoder.W"}
    assert float(np.abs(got["time_encoder.W"]).max()) == 0.0
    missed, worst = [], ("", 0.0)
    for k, r in list(ref["grads"].items()) + [("dx", ref["dx"])]:
        g = dx if k == "dx" else got[k]
        assert g.shape == r.shape, k
        if np.abs(r).max() == 0.0:
            assert tag == "lstm_T1" and k == "backbone.0.weight_hh_l0"
            assert float(np.abs(g).max()) == 0.0
            continue
        err, _ = report_err(f"{label} {k} vs float64 autograd", g, r)
        if err > worst[1]:
            worst = (k, err)
        if not err <= GRAD_TOL:
            missed.append((k, err))
    log_line(f"[parity] {label}: worst tensor {worst[0]} at {worst[1]:.3e} of its maximum (bound {GRAD_TOL:.0e})")
    assert not missed, missed
    if tag == "lstm_T1":
        assert float(np.abs(got["backbone.0.weight_hh_l0"]).max()) == 0.0
    if c["kind"] == "lstm":
        for i in range(c["L"]):
            assert torch.equal(views[f"backbone.{i}.bias_ih_l0"], views[f"backbone.{i}.bias_hh_l0"])
        m.eval()
        out = host(m(batch_of(cs["x"], cs["t"])))
        fwd = O.lstm_score_forward(cs["sd"], cs["x"], cs["t"])
        report_err(f"{label} eval forward vs the oracle", out, fwd)
        assert np.abs(out - fwd).max() <= SCORE_TOL * max(1.0, np.abs(fwd).max())


@pytest.mark.parametrize("tag", ["lstm_100", "mlp_rows"])
def test_gradients_are_bit_reproducible_at_the_split_k_shapes(tag):
    cs = S.case(tag)
    m = _model(tag)
    g1 = _forward_backward(m, cs).clone()
    m.zero_grad()
    g2 = _forward_backward(m, cs)
    assert float(g1.abs().max()) > 0 and torch.equal(g1, g2)


@pytest.mark.parametrize("tag", ["lstm_73", "mlp_tails"])
def test_backward_accumulates_until_zero_grad(tag):
    """A second backward without zero_grad() doubles every tensor (to 1e-6 of its maximum: g + g is exact, the bound only allows for a
    reduction that adds the old value in another place); after zero_grad() the next backward overwrites, bit for bit the first run."""
    cs = S.case(tag)
    m = _model(tag)
    g1 = _forward_backward(m, cs).clone()
    g2 = _forward_backward(m, cs).clone()
    for name, off, numel, _, _ in m._layout:
        a, b = g1[off:off + numel], g2[off:off + numel]
        assert float((b - 2.0 * a).abs().max()) <= 1e-6 * float(a.abs().max()), name
    assert float(g1.abs().max()) > 0
    m.zero_grad()
    g3 = _forward_backward(m, cs)
    assert torch.equal(g3, g1)


def test_lstm_width_limit_is_100():
    """d_model = 101 is refused, by the module and by fd_score_create_ex, with a message that names the limit the engine enforces;
    d_model = 100 is accepted (and trained: the lstm_100 case)."""
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.models.score_models import LSTMScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler(beta_min=0.1, beta_max=20.0, fourier_noise_scaling=True)
    sch.set_noise_scaling(4)
    with pytest.raises(_C.FdError, match="d_model <= 100"):
        LSTMScoreModule(n_channels=2, max_len=4, noise_scheduler=sch, d_model=101, num_layers=1)
    ctx = _C.ctx(torch.device(DEV))
    for D, ok in ((101, False), (100, True)):
        dims, h = _C.model_dims(2, 4, D, 1, 1), C.c_void_p()
        rc = _C.lib().fd_score_create_ex(ctx, C.byref(dims), _C.FD_BACKBONE_LSTM, 0, C.byref(h))
        if ok:
            assert rc == 0 and h.value
            assert _C.lib().fd_score_destroy(h) == 0
        else:
            msg = _C.lib().fd_last_error(ctx).decode()
            assert rc != 0 and not h.value
            assert "d_model <= 100" in msg and "128" not in msg, msg
    assert LSTMScoreModule(n_channels=2, max_len=4, noise_scheduler=sch, d_model=100, num_layers=1).d_model == 100
