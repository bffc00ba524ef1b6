"""GPU: the post-hoc scores on the engine (csrc/fd_posthoc.hip, utils/posthoc.py) against the float64 restatement of
tests/posthoc_ref.py, which tests/test_posthoc_cpu.py pins on its own.

    fd_posthoc_head    loss and per_series within 1e-6 relative (double sums, one rounding to float); dout bit-exact zero where zero is
                       specified, within 2 ulp (predict: a constant times a sign) or 1e-6 relative (classify) elsewhere
    fd_posthoc_batch   indices = the numpy rule on fd_philox_words; rows = (pool[idx] - mean) * inv_std to 1 ulp; labels; determinism
    fd_posthoc_fit     20 steps against the reference fed the engine's index trace.  Step 0 within 5e-6 max(1, max |ref out|), the
                       forward bound of tests/test_gpu_backbones.py (both losses are 1-Lipschitz in the outputs under the max norm).
                       Later steps drift: the bound is FOUR TIMES the largest loss difference between the restatement run in float32
                       and in float64 on the CPU (DRIFT_F32 below, measured by measure_drift()), never less than the step-0 bound.
    end to end         the four learnability conditions of the CPU test, the keys of the two Metric classes, their view
"""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests import posthoc_ref as R
from tests.gpu_util import DEV, dev, host, log_line, report_err
from tests.test_posthoc_cpu import LEARN, SEEDS

pytestmark = pytest.mark.gpu

TASK = {"classify": 0, "predict": 1}            # FD_POSTHOC_CLASSIFY, FD_POSTHOC_PREDICT
FIT = dict(T=24, C=2, D=16, L=1, B=32, steps=20, lr=1e-2, seed=7, na=100, nb=77)
# max over the 20 steps of |loss(float32 restatement) - loss(float64 restatement)| on the CPU, per task: measure_drift()
DRIFT_F32 = {"classify": 1.118e-6, "predict": 1.304e-7}


def _lib():
    from fourierdiffusion_amd import _C
    return _C, _C.lib(), _C.ctx(torch.device(DEV))


def _i32(n):
    return torch.empty(n, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ fd_posthoc_head
def _head_inputs(task, B, T, C):
    out = W.randn(f"ph_out_{task}", (B, T, C), 3)
    x = W.randn(f"ph_x_{task}", (B, T, C), 4)
    if task == "predict" and T >= 2:
        out[0, 0, 0] = x[0, 1, 0]                          # sign(0) = 0
    return out, x, (np.arange(B) % 2).astype(np.int64)


def _head(task, out, x, label, with_dout=True):
    _C, lib, ctx = _lib()
    B, T, Cn = out.shape
    o, xd = dev(out), dev(x)
    lab = torch.from_numpy(label.astype(np.int32)).to(DEV)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    dout = torch.full((B, T, Cn), float("nan"), dtype=torch.float32, device=DEV) if with_dout else None
    per = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    rc = lib.fd_posthoc_head(ctx, TASK[task], o.data_ptr(), xd.data_ptr(), lab.data_ptr(), B, T, Cn, loss.data_ptr(), _C.ptr(dout),
                             per.data_ptr(), _C.stream_of(o))
    torch.cuda.synchronize()
    return rc, loss, dout, per


@pytest.mark.parametrize("task", ["predict", "classify"])
@pytest.mark.parametrize("B,T,C", [(3, 5, 1), (5, 17, 3), (130, 24, 2), (4, 2, 1), (6, 24, 40)])
def test_head_against_float64(task, B, T, C):
    out, x, label = _head_inputs(task, B, T, C)
    ref = R.head_with_grad(task, out, x, label)
    rc, loss, dout, per = _head(task, out, x, label)
    assert rc == 0
    got_loss, got, got_per = float(loss.item()), dout.cpu().numpy(), per.cpu().numpy()
    log_line(f"[posthoc] head {task} {(B, T, C)}: loss rel err {abs(got_loss - ref['loss']) / abs(ref['loss']):.2e}")
    assert abs(got_loss - ref["loss"]) <= 1e-6 * abs(ref["loss"])
    assert np.all(np.abs(got_per - ref["per_series"]) <= 1e-6 * np.abs(ref["per_series"]))
    zero = ref["dout"] == 0.0
    if task == "predict":
        assert zero[:, -1].all() and zero[0, 0, 0] and zero.sum() == B * C + 1
    else:
        assert zero[:, :-1].all() and not zero[:, -1].any()
    assert np.all(got.view(np.uint32)[zero] == 0)                                    # +0.0, bit for bit
    live, want = got[~zero].astype(np.float64), ref["dout"][~zero]
    if task == "predict":
        assert np.all(np.abs(live - want) <= 2.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    else:
        assert np.all(np.abs(live - want) <= 1e-6 * np.abs(want))
    # evaluation only: the same loss and per-series values without a gradient buffer
    rc, loss2, _, per2 = _head(task, out, x, label, with_dout=False)
    assert rc == 0 and torch.equal(loss, loss2) and torch.equal(per, per2)


def test_head_refuses_predict_on_one_point():
    out, x, label = _head_inputs("predict", 3, 1, 2)
    rc, loss, _, _ = _head("predict", out, x, label)
    assert rc == -1 and bool(torch.isnan(loss).all())       # FD_ERR_ARG, nothing launched
    rc, _, dout, _ = _head("classify", out, x, label)
    assert rc == 0 and not bool(torch.isnan(dout).any())    # T = 1 is a series the classifier can still read


# ------------------------------------------------------------------------------------------------ fd_posthoc_batch
def _philox_words(seed, offset, n):
    _C, lib, ctx = _lib()
    buf = torch.empty((n, 4), dtype=torch.int32, device=DEV)
    _C.check(lib.fd_philox_words(ctx, buf.data_ptr(), n, seed, offset, _C.stream_of(buf)), ctx)
    return buf.cpu().numpy().view(np.uint32)


def _batch(task, a, b, mean, inv, seed, offset, step, B):
    _C, lib, ctx = _lib()
    T, Cn = a.shape[1:]
    x = torch.full((B, T, Cn), float("nan"), dtype=torch.float32, device=DEV)
    label, idx = _i32(B), _i32(B)
    rc = lib.fd_posthoc_batch(ctx, TASK[task], a.data_ptr(), a.shape[0], _C.ptr(b), b.shape[0] if b is not None else 0, mean.data_ptr(), inv.data_ptr(), seed, offset, step, B, T, Cn, x.data_ptr(), label.data_ptr(),
                              idx.data_ptr(), _C.stream_of(x))
    _C.check(rc, ctx)
    torch.cuda.synchronize()
    return x, label, idx


@pytest.mark.parametrize("task", ["classify", "predict"])
@pytest.mark.parametrize("na,nb,B", [(7, 7, 6), (100003, 100003, 130), (50, 9, 8)])
def test_batch_follows_the_index_rule(task, na, nb, B):
    T, Cn, seed, offset, step = 3, 2, 0x1234567890ABCDEF, 11, 5
    pool_a, pool_b = W.randn("ph_pool_a", (na, T, Cn), 1), W.randn("ph_pool_b", (nb, T, Cn), 2)
    mean_h, inv_h = np.array([0.3, -1.2], dtype=np.float32), np.array([1.7, 0.4], dtype=np.float32)
    a, b, mean, inv = dev(pool_a), (dev(pool_b) if task == "classify" else None), dev(mean_h), dev(inv_h)
    x, label, idx = _batch(task, a, b, mean, inv, seed, offset, step, B)
    cps = R.counters_per_step(B)
    want_idx, want_label = R.indices_from_words(_philox_words(seed, offset + step * cps, cps), B, na, nb if task == "classify" else None)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(label.cpu().numpy(), want_label)
    assert want_idx.min() >= 0 and np.all(want_idx < np.where(want_label == 1, na, nb))
    want = R.gather(pool_a, pool_b if task == "classify" else None, want_idx, want_label, mean_h, inv_h)
    got = x.cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
    x2, label2, idx2 = _batch(task, a, b, mean, inv, seed, offset, step, B)
    assert torch.equal(x, x2) and torch.equal(label, label2) and torch.equal(idx, idx2)
    _, _, idx3 = _batch(task, a, b, mean, inv, seed, offset, step + 1, B)
    if na > 1:
        assert not torch.equal(idx, idx3)


# ------------------------------------------------------------------------------------------------ fd_posthoc_fit
def fit_case():
    c = FIT
    sd = W.make_state_dict_backbone("lstm", c["C"], c["T"], c["D"], c["L"], seed=4321)
    a, b = R.ar1(c["na"], c["T"], c["C"], 1), R.noise(c["nb"], c["T"], c["C"], 2)
    mean, inv = R.stats(a)
    return sd, a, b, mean, inv


def measure_drift():
    """The CPU measurement behind DRIFT_F32 (python -c "from tests.test_gpu_posthoc import measure_drift; print(measure_drift())")."""
    c = FIT
    sd, a, b, mean, inv = fit_case()
    drift = {}
    for task in ("classify", "predict"):
        trace = R.index_trace(c["seed"], c["steps"], c["B"], c["na"], c["nb"] if task == "classify" else None)
        r64 = R.fit(task, sd, a, b, mean, inv, trace, c["lr"])
        r32 = R.fit(task, sd, a, b, mean, inv, trace, c["lr"], dtype=torch.float32)
        drift[task] = float(np.abs(r64["loss"] - r32["loss"]).max())
    return drift


def _engine_fit(task, fused=True):
    from fourierdiffusion_amd.utils.posthoc import PosthocNetwork
    c = FIT
    sd, a, b, mean, inv = fit_case()
    net = PosthocNetwork(c["C"], c["T"], d_model=c["D"], num_layers=c["L"], seed=c["seed"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    loss = net.fit(task, a, b if task == "classify" else None, steps=c["steps"], batch_size=c["B"], lr=c["lr"], mean=mean, inv_std=inv,
                   trace_indices=True, fused=fused)
    torch.cuda.synchronize()
    return net, loss


@pytest.fixture(scope="module", params=["classify", "predict"])
def fitted(request):
    task = request.param
    net, loss = _engine_fit(task)
    sd, a, b, mean, inv = fit_case()
    ref = R.fit(task, sd, a, b, mean, inv, net.last_indices.cpu().numpy(), FIT["lr"])
    return task, net, loss, ref


def test_fit_draws_the_batches_of_the_index_rule(fitted):
    task, net, _, _ = fitted
    c = FIT
    want = R.index_trace(c["seed"], c["steps"], c["B"], c["na"], c["nb"] if task == "classify" else None)
    np.testing.assert_array_equal(net.last_indices.cpu().numpy(), want)


def test_fit_against_the_reference(fitted):
    task, _, loss, ref = fitted
    got = host(loss)
    step0 = 5e-6 * max(1.0, ref["out_max"][0])
    diff = np.abs(got - ref["loss"])
    report_err(f"posthoc fit {task}: loss trace of {FIT['steps']} steps", got, ref["loss"])
    log_line(f"[posthoc] fit {task}: step-0 |diff| {diff[0]:.3e} (bound {step0:.3e}), max |diff| {diff.max():.3e} "
             f"(bound {max(4 * DRIFT_F32[task], step0):.3e})")
    assert diff[0] <= step0
    assert diff.max() <= max(4.0 * DRIFT_F32[task], step0)
    assert got[-1] < got[0]                                  # and it trains


def test_two_identical_fits_are_bit_equal(fitted):
    task, net, loss, _ = fitted
    net2, loss2 = _engine_fit(task)
    assert torch.equal(loss, loss2)
    assert torch.equal(net.module.flat_parameters, net2.module.flat_parameters)


def test_loop_driven_from_python_is_bit_equal(fitted):
    task, net, loss, _ = fitted
    net2, loss2 = _engine_fit(task, fused=False)
    assert torch.equal(loss, loss2)
    assert torch.equal(net.last_indices, net2.last_indices)
    assert torch.equal(net.module.flat_parameters, net2.module.flat_parameters)
    assert torch.equal(net.exp_avg_sq, net2.exp_avg_sq)


def test_fit_refuses_a_transformer():
    from tests.gpu_util import make_model
    _C, lib, ctx = _lib()
    m, _, _ = make_model(dict(T=24, C=2, D=8, L=1, H=4), precision="fp32")
    _, h = m._engine()
    flat = m.flat_parameters
    g, m1, m2 = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
    before = flat.clone()
    a = dev(R.ar1(16, 24, 2, 1))
    stats = torch.ones(2, dtype=torch.float32, device=DEV)
    loss = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
    need = C.c_size_t(0)
    _C.check(lib.fd_posthoc_fit_workspace_bytes(ctx, 4, 24, 2, C.byref(need)), ctx)
    work = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    rc = lib.fd_posthoc_fit(h, 1, flat.data_ptr(), g.data_ptr(), m1.data_ptr(), m2.data_ptr(), a.data_ptr(), 16, None, 0,
                            stats.data_ptr(), stats.data_ptr(), 0, 0, 0, 2, 4, 1e-3, 0.0, loss.data_ptr(), None, work.data_ptr(),
                            need.value, _C.stream_of(flat))
    torch.cuda.synchronize()
    assert rc == -5                                           # FD_ERR_UNSUPPORTED
    assert b"LSTM" in lib.fd_last_error(ctx)
    assert torch.equal(flat, before) and bool(torch.isnan(loss).all())


# ------------------------------------------------------------------------------------------------ end to end
def _knobs():
    c = LEARN
    return dict(steps=c["steps"], batch_size=c["B"], lr=c["lr"], d_model=c["D"], num_layers=c["L"])


@pytest.mark.parametrize("seed", SEEDS)
def test_discriminative_score_learns(seed):
    from fourierdiffusion_amd.utils.posthoc import discriminative_score
    c = LEARN
    real = R.ar1(c["n"], c["T"], c["C"], 10 * seed + 1)
    apart = discriminative_score(real, R.noise(c["n"], c["T"], c["C"], 10 * seed + 2), seed=seed, **_knobs())
    alike = discriminative_score(real, R.ar1(c["n"], c["T"], c["C"], 10 * seed + 3), seed=seed, **_knobs())
    log_line(f"[posthoc] seed {seed}: discriminative score AR against noise {apart['score']:.3f}, AR against AR {alike['score']:.3f}")
    assert apart["score"] >= 0.40
    assert alike["score"] <= 0.15
    assert apart["n_train"] == 512 and apart["n_test"] == 128 and len(apart["loss_trace"]) == c["steps"]
    assert apart["accuracy"] == 0.5 * (apart["accuracy_real"] + apart["accuracy_generated"])


@pytest.mark.parametrize("seed", SEEDS)
def test_predictive_score_learns(seed):
    from fourierdiffusion_amd.utils.posthoc import predictive_score
    c = LEARN
    real = R.ar1(c["n"], c["T"], c["C"], 10 * seed + 1)
    good = predictive_score(R.ar1(c["n"], c["T"], c["C"], 10 * seed + 3), real, stats_from=real, seed=seed, **_knobs())
    bad = predictive_score(R.noise(c["n"], c["T"], c["C"], 10 * seed + 2), real, stats_from=real, seed=seed, **_knobs())
    log_line(f"[posthoc] seed {seed}: predictive MAE trained on AR {good['mae']:.3f}, trained on noise {bad['mae']:.3f}")
    assert good["mae"] <= 0.40          # the floor is 0.798 sqrt(1 - 0.81) = 0.348
    assert bad["mae"] >= 0.65           # predicting zero gives 0.798
    assert len(good["loss_trace"]) == c["steps"]


@pytest.mark.parametrize("holdout", [False, True])
def test_metric_classes_return_the_documented_keys(holdout):
    from fourierdiffusion_amd.sampling.metrics import DiscriminativeScore, MetricCollection, PredictiveScore
    real, held, fake = R.ar1(96, 12, 2, 1), R.ar1(40, 12, 2, 2), R.noise(96, 12, 2, 3)
    knobs = dict(steps=10, batch_size=16, lr=1e-2, d_model=8, random_seed=3)
    coll = MetricCollection([partial(DiscriminativeScore, **knobs), partial(PredictiveScore, **knobs)], original_samples=real,
                            holdout_samples=held if holdout else None)
    assert [type(m) for m in coll.metrics_time] == [DiscriminativeScore, PredictiveScore] and coll.metrics_freq == []
    res = coll(fake)
    want = {"discriminative_score", "discriminative_accuracy", "discriminative_score_self", "predictive_score", "predictive_score_self"}
    if holdout:
        want |= {"discriminative_score_holdout", "discriminative_accuracy_holdout", "predictive_score_holdout"}
    assert set(res) == {f"time_{k}" for k in want}
    assert all(isinstance(v, float) and np.isfinite(v) for v in res.values())
    assert 0.0 <= res["time_discriminative_score"] <= 0.5
    assert coll(fake) == res                                  # deterministic given the seed
