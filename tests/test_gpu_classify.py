"""GPU: the label-aware post-hoc score on the engine (the multiclass entry points of csrc/fd_posthoc.hip, utils/posthoc.py,
ClassificationScore) against the float64 restatement of tests/classify_ref.py, which tests/test_classify_cpu.py pins on its own.

    fd_posthoc_head_multiclass  loss and logp within 1e-6 relative (1e-6 absolute where |logp| < 1); pred equal, a planted tie
                                included; dout +0.0 bit for bit at every t < T - 1 and in the channels >= K, within 1e-6 relative
                                elsewhere; logits of +-1e4; evaluation-only calls; refusals leave NaN-filled outputs alone
    fd_posthoc_batch_labelled   indices and labels = the numpy rule on fd_philox_words, uniform and balanced; rows to 1 ulp in the
                                channels < C, +0.0 in the others; determinism
    fd_posthoc_confusion        numpy.add.at
    fd_posthoc_fit_multiclass   20 steps against the reference fed the engine's index trace.  Step 0 within
                                2 * 5e-6 max(1, max |ref out|): cross-entropy is 2-Lipschitz in the logits under the max norm and
                                5e-6 is the forward bound of tests/test_gpu_backbones.py.  Later steps within FOUR TIMES the largest
                                loss difference between the restatement in float32 and in float64 on the CPU (DRIFT_F32, measured by
                                tests/test_classify_cpu.measure_drift()), never less than the step-0 bound.
    end to end                  the two learnability conditions of the CPU test, the keys of ClassificationScore through a
                                MetricCollection, TSTR against the TRTR baseline, and the binary task's loss bits, unchanged
"""
from functools import partial

import numpy as np
import pytest
import torch

from tests import classify_ref as CR
from tests import posthoc_ref as R
from tests.gpu_util import DEV, dev, host, log_line, report_err
from tests.test_classify_cpu import CASES, FIT, LEARN, SEEDS, fit_case, learn_data

pytestmark = pytest.mark.gpu

MAX_K = 256                                      # FD_POSTHOC_MAX_CLASSES
# max over the 20 steps of |loss(float32 restatement) - loss(float64 restatement)| on the CPU: measure_drift()
DRIFT_F32 = {"uniform": 1.458e-7, "balanced": 1.444e-7}
NAN = float("nan")


def _lib():
    from fourierdiffusion_amd import _C
    return _C, _C.lib(), _C.ctx(torch.device(DEV))


def _i32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int32)).to(DEV)


def _full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------ fd_posthoc_head_multiclass
def _head(out, label, K, want=("logp", "pred", "loss", "dout", "nll"), Cn=None):
    _C, lib, ctx = _lib()
    B, T, C = out.shape
    o = dev(out)
    bufs = dict(logp=_full((B, K), NAN, torch.float64), pred=_full((B,), -7, torch.int32), loss=_full((1,), NAN, torch.float32),
                dout=_full((B, T, C), NAN, torch.float32), nll=_full((B,), NAN, torch.float64))
    p = {k: (bufs[k].data_ptr() if k in want else None) for k in bufs}
    lab = None if label is None else _i32(label)
    rc = lib.fd_posthoc_head_multiclass(ctx, o.data_ptr(), _C.ptr(lab), B, T, C if Cn is None else Cn, K, p["logp"], p["pred"], p["loss"],
                                        p["dout"], p["nll"], _C.stream_of(o))
    torch.cuda.synchronize()
    return rc, bufs


def _untouched(bufs):
    return all(bool(torch.isnan(v).all()) if v.is_floating_point() else bool((v == -7).all()) for v in bufs.values())


def _check_head(out, label, K):
    B, T, Cn = out.shape
    ref = CR.head_with_grad(out, K, label)
    rc, got = _head(out, label, K)
    assert rc == 0
    loss, logp, dout = float(got["loss"].item()), got["logp"].cpu().numpy(), got["dout"].cpu().numpy()
    log_line(f"[classify] head {(B, T, Cn, K)}: loss rel err {abs(loss - ref['loss']) / abs(ref['loss']):.2e}, "
             f"logp max err {np.abs(logp - ref['logp']).max():.2e}")
    assert abs(loss - ref["loss"]) <= 1e-6 * abs(ref["loss"])
    assert np.all(np.isfinite(logp)) and np.all(np.abs(logp - ref["logp"]) <= 1e-6 * np.maximum(np.abs(ref["logp"]), 1.0))
    np.testing.assert_array_equal(got["pred"].cpu().numpy(), ref["pred"])
    nll = got["nll"].cpu().numpy()
    assert np.all(np.abs(nll + ref["logp"][np.arange(B), label]) <= 1e-6 * np.maximum(np.abs(nll), 1.0))
    dead = np.ones(out.shape, dtype=bool)
    dead[:, -1, :K] = False
    assert np.all(ref["dout"][dead] == 0.0)
    assert np.all(dout.view(np.uint32)[dead] == 0)                                   # +0.0, bit for bit
    live, want = dout[~dead].astype(np.float64), ref["dout"][~dead]
    assert np.all(np.isfinite(live)) and np.all(np.abs(live - want) <= 1e-6 * np.abs(want))
    # evaluation only: the same logp and pred bits with no label, loss, gradient or per-series buffer
    rc, only = _head(out, None, K, want=("logp", "pred"))
    assert rc == 0 and torch.equal(only["logp"], got["logp"]) and torch.equal(only["pred"], got["pred"])
    assert _untouched({k: only[k] for k in ("loss", "dout", "nll")})
    rc, one = _head(out, None, K, want=("pred",))
    assert rc == 0 and torch.equal(one["pred"], got["pred"])
    return ref


@pytest.mark.parametrize("B,T,Cn,K", [(3, 5, 3, 3), (5, 17, 4, 2), (130, 24, 5, 5), (4, 1, 2, 2), (6, 24, 40, 3), (2, 3, MAX_K, MAX_K)])
def test_head_against_float64(B, T, Cn, K):
    from oracle import weights as W
    out = W.randn(f"cls_out_{B}_{T}_{Cn}_{K}", (B, T, Cn), 3)
    out[0, -1, K - 1] = out[0, -1, 0] = np.abs(out[0, -1]).max() + 1.0        # a tie between the first and the last class
    if B > 1:
        out[1, -1, :K] = 0.25                                                    # and one between all of them
    ref = _check_head(out, np.arange(B) % K, K)
    assert ref["pred"][0] == 0 and (B == 1 or ref["pred"][1] == 0)


def test_head_is_finite_at_large_logits():
    out = np.zeros((4, 3, 4), dtype=np.float32)
    out[0, -1, :3] = [1e4, 0.0, -1e4]
    out[1, -1, :3] = [-1e4, -1e4, 1e4]
    out[2, -1, :3] = [1e4, 1e4, -1e4]
    out[3, -1, :3] = [-1e4, 0.5, 0.25]
    out[:, -1, 3] = 3e4                                                           # no logit at K = 3
    _check_head(out, np.array([0, 1, 2, 0]), 3)


def test_head_refusals_launch_nothing():
    from oracle import weights as W
    out, label = W.randn("cls_refuse", (3, 4, 4), 1), np.array([0, 1, 2])
    _, lib, ctx = _lib()
    for kwargs, word in ((dict(K=1), b"K=1"), (dict(K=MAX_K + 1), b"K=257"), (dict(K=3, Cn=2), b"fewer"),
                         (dict(K=3, label=None), b"need the labels"), (dict(K=3, want=("loss",)), b"nll"), (dict(K=3, want=()), b"null")):
        kw = dict(dict(label=label), **kwargs)
        rc, bufs = _head(out, kw.pop("label"), kw.pop("K"), **kw)
        assert rc == -1 and word in lib.fd_last_error(ctx), (kwargs, lib.fd_last_error(ctx))       # FD_ERR_ARG
        assert _untouched(bufs), kwargs


# ------------------------------------------------------------------------------------------------ fd_posthoc_batch_labelled
def _philox_words(seed, offset, n):
    _C, lib, ctx = _lib()
    buf = torch.empty((n, 4), dtype=torch.int32, device=DEV)
    _C.check(lib.fd_philox_words(ctx, buf.data_ptr(), n, seed, offset, _C.stream_of(buf)), ctx)
    return buf.cpu().numpy().view(np.uint32)


def _batch(a, ya, K, mean, inv, seed, offset, step, B, tables=None, Cn=None, na=None):
    _C, lib, ctx = _lib()
    T, C = a.shape[1:]
    Cn = max(C, K) if Cn is None else Cn
    x = _full((B, T, max(Cn, 1)), NAN, torch.float32)
    label, idx = _full((B,), -7, torch.int32), _full((B,), -7, torch.int32)
    order, start = (None, None) if tables is None else tables
    rc = lib.fd_posthoc_batch_labelled(ctx, a.data_ptr(), a.shape[0] if na is None else na, ya.data_ptr(), _C.ptr(order), _C.ptr(start),
                                       K, mean.data_ptr(), inv.data_ptr(), seed, offset, step, B, T, C, Cn, x.data_ptr(),
                                       label.data_ptr(), idx.data_ptr(), _C.stream_of(x))
    torch.cuda.synchronize()
    return rc, x, label, idx


def _check_batch(pool, labels, K, mean_h, inv_h, B, step, balanced):
    seed, offset = 0x1234567890ABCDEF, 11
    na, T, C = pool.shape
    Cn = max(C, K)
    a, ya, mean, inv = dev(pool), _i32(labels), dev(mean_h), dev(inv_h)
    tables = None
    if balanced:
        order, start = CR.class_tables(labels, K)
        tables = (_i32(order), _i32(start))
    rc, x, label, idx = _batch(a, ya, K, mean, inv, seed, offset, step, B, tables)
    assert rc == 0
    cps = R.counters_per_step(B)
    want_idx = CR.indices_from_words(_philox_words(seed, offset + step * cps, cps), B, na, step, labels if balanced else None, K)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(label.cpu().numpy(), labels[want_idx])
    assert want_idx.min() >= 0 and want_idx.max() < na
    want = CR.gather(pool, want_idx, mean_h, inv_h, Cn)
    got = x.cpu().numpy()
    assert got.shape == (B, T, Cn)
    assert np.all(np.abs(got[:, :, :C].astype(np.float64) - want[:, :, :C].astype(np.float64))
                  <= np.spacing(np.abs(want[:, :, :C])).astype(np.float64))
    assert np.all(got[:, :, C:].view(np.uint32) == 0)                                # +0.0, bit for bit
    rc, x2, label2, idx2 = _batch(a, ya, K, mean, inv, seed, offset, step, B, tables)
    assert rc == 0 and torch.equal(x, x2) and torch.equal(label, label2) and torch.equal(idx, idx2)
    return want_idx


def test_uniform_batch_follows_the_index_rule():
    from oracle import weights as W
    pool, labels = W.randn("cls_pool_u", (100, 7, 1), 1), np.arange(100) % 5
    one = _check_batch(pool, labels, 5, np.array([0.3], dtype=np.float32), np.array([1.7], dtype=np.float32), 32, 5, False)
    two = _check_batch(pool, labels, 5, np.array([0.3], dtype=np.float32), np.array([1.7], dtype=np.float32), 32, 6, False)
    assert not np.array_equal(one, two)


@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("B", [32, 6])
def test_balanced_batch_follows_the_index_rule(B, step):
    from oracle import weights as W
    labels = np.array([3] * 40 + [0] * 59 + [2])            # K = 4: class 1 is absent, class 2 holds a single row
    np.random.default_rng(3).shuffle(labels)
    pool = W.randn("cls_pool_b", (100, 5, 3), 2)
    idx = _check_batch(pool, labels, 4, np.array([0.3, -1.2, 0.0], dtype=np.float32), np.array([1.7, 0.4, 1.0], dtype=np.float32), B, step,
                       True)
    np.testing.assert_array_equal(labels[idx], np.array([0, 2, 3])[(step * B + np.arange(B)) % 3])


def test_batch_refusals_launch_nothing():
    from oracle import weights as W
    _, lib, ctx = _lib()
    pool, labels = W.randn("cls_pool_r", (10, 4, 2), 1), np.arange(10) % 3
    a, ya, stats = dev(pool), _i32(labels), dev(np.ones(2, dtype=np.float32))
    order = _i32(np.argsort(labels, kind="stable"))
    for kwargs, word in ((dict(K=1, Cn=2), b"K=1"), (dict(K=MAX_K + 1), b"K=257"), (dict(K=3, Cn=2), b"max(C, K)"),
                         (dict(K=3, Cn=4), b"max(C, K)"), (dict(K=3, na=0), b"empty"), (dict(K=3, tables=(order, None)), b"together")):
        rc, x, label, idx = _batch(a, ya, kwargs.pop("K"), stats, stats, 1, 0, 0, 8, **kwargs)
        assert rc == -1 and word in lib.fd_last_error(ctx), (word, lib.fd_last_error(ctx))
        assert bool(torch.isnan(x).all()) and bool((label == -7).all()) and bool((idx == -7).all())


# ------------------------------------------------------------------------------------------------ fd_posthoc_confusion
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("n", [1, 255, 1000])
def test_confusion_against_numpy(n, K):
    from fourierdiffusion_amd.utils.posthoc import confusion_matrix
    rng = np.random.default_rng(100 * n + K)
    label, pred = rng.integers(0, K, size=n), rng.integers(0, K, size=n)
    got = confusion_matrix(_i32(label), _i32(pred), K)
    assert got.dtype == torch.int32 and tuple(got.shape) == (K, K)
    np.testing.assert_array_equal(got.cpu().numpy(), CR.confusion(label, pred, K))
    assert torch.equal(got, confusion_matrix(_i32(label), _i32(pred), K))


def test_confusion_refuses_a_class_count_out_of_range():
    _C, lib, ctx = _lib()
    label, counts = _i32(np.zeros(4)), _full((4,), -7, torch.int32)
    for K in (1, MAX_K + 1):
        rc = lib.fd_posthoc_confusion(ctx, label.data_ptr(), label.data_ptr(), 4, K, counts.data_ptr(), _C.stream_of(label))
        torch.cuda.synchronize()
        assert rc == -1 and bool((counts == -7).all())


# ------------------------------------------------------------------------------------------------ fd_posthoc_fit_multiclass
def _engine_fit(balance, fused=True, steps=None):
    from fourierdiffusion_amd.utils.posthoc import PosthocNetwork
    c = FIT
    sd, a, ya, mean, inv = fit_case()
    net = PosthocNetwork(c["C"], c["T"], d_model=c["D"], num_layers=c["L"], seed=c["seed"], n_classes=c["K"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    losses, traces = [], []
    for n in steps or (c["steps"],):
        losses.append(net.fit("multiclass", a, labels=ya, balance=balance, steps=n, batch_size=c["B"], lr=c["lr"], mean=mean, inv_std=inv,
                              trace_indices=True, fused=fused))
        traces.append(net.last_indices)
    torch.cuda.synchronize()
    return net, torch.cat(losses), torch.cat(traces)


@pytest.fixture(scope="module", params=["uniform", "balanced"])
def fitted(request):
    balance = request.param == "balanced"
    net, loss, trace = _engine_fit(balance)
    sd, a, ya, mean, inv = fit_case()
    ref = CR.fit(sd, a, ya, FIT["K"], mean, inv, trace.cpu().numpy(), FIT["lr"])
    return request.param, net, loss, trace, ref


def test_fit_draws_the_batches_of_the_index_rule(fitted):
    name, _, _, trace, _ = fitted
    c = FIT
    _, _, ya, _, _ = fit_case()
    want = CR.index_trace(c["seed"], c["steps"], c["B"], c["na"], ya if name == "balanced" else None, c["K"])
    np.testing.assert_array_equal(trace.cpu().numpy(), want)


def test_fit_against_the_reference(fitted):
    name, _, loss, _, ref = fitted
    got = host(loss)
    step0 = 2.0 * 5e-6 * max(1.0, ref["out_max"][0])
    diff = np.abs(got - ref["loss"])
    report_err(f"classify fit {name}: loss trace of {FIT['steps']} steps", got, ref["loss"])
    log_line(f"[classify] fit {name}: step-0 |diff| {diff[0]:.3e} (bound {step0:.3e}), max |diff| {diff.max():.3e} "
             f"(bound {max(4 * DRIFT_F32[name], step0):.3e})")
    assert diff[0] <= step0
    assert diff.max() <= max(4.0 * DRIFT_F32[name], step0)
    assert got[-1] < got[0]                                  # and it trains


def test_loop_driven_from_python_is_bit_equal(fitted):
    name, net, loss, trace, _ = fitted
    net2, loss2, trace2 = _engine_fit(name == "balanced", fused=False)
    assert torch.equal(loss, loss2) and torch.equal(trace, trace2)
    assert torch.equal(net.module.flat_parameters, net2.module.flat_parameters)
    assert torch.equal(net.exp_avg_sq, net2.exp_avg_sq)


def test_a_second_fit_continues_the_index_stream(fitted):
    name, net, loss, trace, _ = fitted
    net2, loss2, trace2 = _engine_fit(name == "balanced", steps=(7, FIT["steps"] - 7))
    assert net2.steps_done == FIT["steps"]
    assert torch.equal(trace, trace2) and torch.equal(loss, loss2)
    assert torch.equal(net.module.flat_parameters, net2.module.flat_parameters)


def test_evaluate_pads_the_channels_and_matches_the_reference(fitted):
    name, net, _, _, ref = fitted
    _, a, ya, mean, inv = fit_case()
    z = (a - mean) * inv
    logp, pred = net.evaluate("multiclass", z, labels=ya)
    assert logp.dtype == torch.float64 and tuple(logp.shape) == (FIT["na"], FIT["K"]) and pred.dtype == torch.int32
    want_logp, want_pred = ref["fit"].predict(CR.pad(z, max(FIT["C"], FIT["K"])))
    # the mean negative log-likelihood over the pool is one more loss of the trace's kind, after the last update: the trace's bound
    rows = np.arange(FIT["na"])
    got_nll, want_nll = -logp.cpu().numpy()[rows, ya].mean(), -want_logp[rows, ya].mean()
    bound = max(4.0 * DRIFT_F32[name], 2.0 * 5e-6 * max(1.0, ref["out_max"][-1]))
    log_line(f"[classify] evaluate {name}: |mean nll - reference| {abs(got_nll - want_nll):.3e} (bound {bound:.3e})")
    assert abs(got_nll - want_nll) <= bound
    sure =np.sort(want_logp, axis=1)[:, -1] - np.sort(want_logp, axis=1)[:, -2] > 1e-3
    np.testing.assert_array_equal(pred.cpu().numpy()[sure], want_pred[sure])
    with pytest.raises(ValueError, match="one class per series"):
        net.evaluate("multiclass", z, labels=ya[:5])
    with pytest.raises(ValueError, match="multiclass task, not for"):
        net.evaluate("classify", z)


# ------------------------------------------------------------------------------------------------ end to end
def _knobs():
    c = LEARN
    return dict(steps=c["steps"], batch_size=c["B"], lr=c["lr"], d_model=c["D"], num_layers=c["L"])


@pytest.mark.parametrize("seed", SEEDS)
def test_classification_score_learns(seed):
    from fourierdiffusion_amd.utils.posthoc import classification_score
    K, C = 3, 2
    train, y_train, permuted, test, y_test = learn_data(K, C, seed)
    score = partial(classification_score, n_classes=K, stats_from=train, seed=seed, **_knobs())
    right, wrong = score(train, y_train, test, y_test), score(train, permuted, test, y_test)
    log_line(f"[classify] seed {seed}: accuracy {right['accuracy']:.3f} (balanced {right['balanced_accuracy']:.3f}, macro F1 "
             f"{right['macro_f1']:.3f}, nll {right['nll']:.3f}), permuted training labels {wrong['accuracy']:.3f}")
    assert right["accuracy"] >= CASES[(K, C)]["right"]
    assert wrong["accuracy"] <= CASES[(K, C)]["permuted"]
    assert set(right) == {"accuracy", "balanced_accuracy", "macro_f1", "nll", "per_class_recall", "confusion", "loss_trace", "n_train",
                          "n_test"}
    cm = np.array(right["confusion"])
    assert cm.shape == (K, K) and right["n_train"] == LEARN["n"] and right["n_test"] == LEARN["n_test"] == cm.sum()
    np.testing.assert_array_equal(cm.sum(axis=1), np.bincount(y_test, minlength=K))
    assert right["accuracy"] == np.trace(cm) / cm.sum() and len(right["loss_trace"]) == LEARN["steps"]
    np.testing.assert_allclose(right["per_class_recall"], np.diag(cm) / cm.sum(axis=1))
    np.testing.assert_allclose(right["balanced_accuracy"], np.mean(right["per_class_recall"]))


@pytest.mark.parametrize("holdout", [False, True])
def test_metric_class_returns_the_documented_keys(holdout):
    from fourierdiffusion_amd.sampling.metrics import ClassificationScore, MetricCollection
    (real, y), (held, yh), (fake, yf) = (CR.ar1_classes(n, 12, 2, 3, s) for n, s in ((96, 1), (40, 2), (64, 3)))
    knobs = dict(steps=10, batch_size=16, lr=1e-2, d_model=8, random_seed=3)
    coll = MetricCollection([partial(ClassificationScore, **knobs)], original_samples=real, original_labels=torch.from_numpy(y),
                            holdout_samples=held if holdout else None, holdout_labels=yh if holdout else None)
    assert [type(m) for m in coll.metrics_time] == [ClassificationScore] and coll.metrics_freq == []
    assert coll.metrics_time[0].n_classes == 3
    res = coll(fake, other_labels=yf)
    want = {"tstr_accuracy", "tstr_balanced_accuracy", "trts_accuracy", "trts_balanced_accuracy", "trtr_accuracy_self",
            "trtr_balanced_accuracy_self"}
    if holdout:
        want |= {"tstr_accuracy_holdout", "tstr_balanced_accuracy_holdout"}
    assert set(res) == {f"time_{k}" for k in want}
    assert all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res.values())
    assert coll(fake, torch.from_numpy(yf)) == res            # deterministic given the seed; the real-set classifier is cached
    with pytest.raises(ValueError, match="sampler.labels"):
        coll(fake)
    with pytest.raises(ValueError, match=r"other_labels must lie in \[0, 3\)"):
        coll(fake, other_labels=yf + 1)


def test_tstr_tracks_the_real_baseline_and_sees_permuted_labels():
    from fourierdiffusion_amd.sampling.metrics import ClassificationScore, MetricCollection
    c = LEARN
    (real, y), (other, yo) = (CR.ar1_classes(c["n"], c["T"], 2, 3, s) for s in (1, 2))
    knobs = dict(steps=c["steps"], batch_size=c["B"], lr=c["lr"], d_model=c["D"], num_layers=c["L"], random_seed=0)
    coll = MetricCollection([partial(ClassificationScore, **knobs)], original_samples=real, original_labels=y)
    right = coll(other, other_labels=yo)
    wrong = coll(other, other_labels=yo[np.random.default_rng(5).permutation(len(yo))])
    base = right["time_trtr_accuracy_self"]
    log_line(f"[classify] real against real: TRTR {base:.3f}, TSTR {right['time_tstr_accuracy']:.3f}, TRTS "
             f"{right['time_trts_accuracy']:.3f}; permuted labels: TSTR {wrong['time_tstr_accuracy']:.3f}, TRTS "
             f"{wrong['time_trts_accuracy']:.3f}")
    assert abs(right["time_tstr_accuracy"] - base) <= 0.1
    assert wrong["time_tstr_accuracy"] <= base - 0.3
    assert wrong["time_trtr_accuracy_self"] == base


# float32 bits of the 20 losses of the binary tasks at the FIT shape of tests/test_gpu_posthoc.py, recorded from the library as it
# was before the multiclass task shared fd_posthoc_fit's loop
BINARY_LOSS_BITS = {
    "classify": [0x3f3871bb, 0x3f338898, 0x3f2ef7c7, 0x3f31d7b7, 0x3f2a535b, 0x3f3f4178, 0x3f2d1ff9, 0x3f30041e, 0x3f323712, 0x3f2b8304,
                 0x3f252480, 0x3f2b8c76, 0x3f2289bf, 0x3f1fd445, 0x3f2baae8, 0x3f195afb, 0x3f148495, 0x3f0e39db, 0x3f174e32, 0x3f067c8c],
    "predict": [0x3f149238, 0x3f0acb4b, 0x3f03e61b, 0x3eeb2fb8, 0x3ecbb747, 0x3ec5399d, 0x3ec58395, 0x3eb499e9, 0x3ec297f0, 0x3ec5caa9,
                0x3ec63f8b, 0x3ec8d000, 0x3ec02d8c, 0x3ebc88d9, 0x3ebc8484, 0x3eb876a3, 0x3eb5979b, 0x3eb15b75, 0x3eb3b474, 0x3ebf515f],
}


@pytest.mark.parametrize("task", ["classify", "predict"])
def test_binary_tasks_keep_their_loss_bits(task):
    from fourierdiffusion_amd.utils.posthoc import PosthocNetwork
    from tests.test_gpu_posthoc import FIT as BIN
    from tests.test_gpu_posthoc import fit_case as bin_case
    sd, a, b, mean, inv = bin_case()
    net = PosthocNetwork(BIN["C"], BIN["T"], d_model=BIN["D"], num_layers=BIN["L"], seed=BIN["seed"], n_classes=None)
    assert net.net_channels == BIN["C"]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    loss = net.fit(task, a, b if task == "classify" else None, steps=BIN["steps"], batch_size=BIN["B"], lr=BIN["lr"], mean=mean,
                   inv_std=inv)
    bits = [int(v) for v in loss.cpu().numpy().view(np.uint32)]
    log_line(f"[classify] binary {task} loss bits: " + " ".join(f"{v:08x}" for v in bits))
    assert bits == BINARY_LOSS_BITS[task]


def test_cli_hands_the_labels_to_the_metric(tmp_path):
    """cmd/sample.py metrics=conditional on a class-conditional synthetic_classes run: the classes of both splits reach the collection,
    the drawn classes reach the metric, and the documented keys land in results.yaml."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    import yaml
    root = Path(__file__).resolve().parent.parent

    def run(cmd):
        return subprocess.run([sys.executable] + cmd, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=str(root)), capture_output=True,
                              text=True, timeout=600)

    common = ["fourier_transform=true", "datamodule=synthetic_classes", "datamodule.max_len=24", "datamodule.num_samples=96",
              "datamodule.n_channels=2", "datamodule.batch_size=32", "datamodule.n_classes=3"]
    r = run([str(root / "cmd" / "train.py"), *common, "score_model=conditional", "score_model.n_classes=3", "score_model.d_model=24",
             "score_model.num_layers=1", "score_model.n_head=4", "trainer.max_epochs=1", "trainer.callbacks.2.every_n_epochs=1",
             "trainer.callbacks.2.num_samples=32", "trainer.callbacks.2.num_diffusion_steps=5", "run_id=clsrun"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    sample = [str(root / "cmd" / "sample.py"), "model_id=clsrun", "num_samples=64", "num_diffusion_steps=5", "sampler.sample_batch_size=32",
              "metrics=conditional", "metrics.metrics.2.steps=20", "metrics.metrics.2.batch_size=32", "metrics.metrics.2.d_model=8"]
    r = run(sample + ["sampler.labels=balanced"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run_dir = tmp_path / "lightning_logs" / "clsrun"
    res = yaml.safe_load(open(run_dir / "results.yaml"))
    for k in ("tstr_accuracy", "tstr_balanced_accuracy", "tstr_accuracy_holdout", "tstr_balanced_accuracy_holdout", "trts_accuracy",
              "trts_balanced_accuracy", "trtr_accuracy_self", "trtr_balanced_accuracy_self"):
        assert 0.0 <= res[f"time_{k}"] <= 1.0, k
    assert not [k for k in res if k.startswith("freq_t")] and "time_sliced_wasserstein_mean" in res
    labels = torch.load(run_dir / "labels.pt")
    assert labels.shape == (64,) and sorted(set(labels.tolist())) == [0, 1, 2]
