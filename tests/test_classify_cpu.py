"""CPU: the float64 restatement of the label-aware post-hoc score (tests/classify_ref.py) is pinned on its own -- the head's gradient
against central differences, ties and large logits, the two index rules -- and it LEARNS: on AR(1) series whose class sets phi it
meets the two conditions the GPU test (tests/test_gpu_classify.py) asks of the engine.  Plus the argument checks of utils/posthoc.py,
ClassificationScore and the MetricCollection plumbing that need no GPU, and the `metrics=conditional` config."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests import classify_ref as CR
from tests import posthoc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2, 3, 4)
LEARN = dict(T=24, n=640, n_test=320, D=16, L=1, steps=200, B=128, lr=1e-2)
# (K, C): accuracy with the right labels at least `right`, with permuted training labels at most `permuted`, on every seed
CASES = {(3, 2): dict(right=0.90, permuted=0.50), (5, 1): dict(right=0.60, permuted=0.35)}
# the fit the GPU test compares step by step
FIT = dict(T=24, C=2, K=3, D=16, L=1, B=32, steps=20, lr=1e-2, seed=7, na=100)


def fit_case():
    c = FIT
    sd = W.make_state_dict_backbone("lstm", max(c["C"], c["K"]), c["T"], c["D"], c["L"], seed=4321)
    a, ya = CR.ar1_classes(c["na"], c["T"], c["C"], c["K"], 1)
    mean, inv = R.stats(a)
    return sd, a, ya, mean, inv


def measure_drift():
    """The CPU measurement behind DRIFT_F32 of tests/test_gpu_classify.py: the largest |loss(float32) - loss(float64)| of the
    restatement over the 20 steps of FIT, uniform and balanced (python -c "from tests.test_classify_cpu import measure_drift;
    print(measure_drift())")."""
    sd, a, ya, mean, inv = fit_case()
    drift = {}
    for name, balance in (("uniform", False), ("balanced", True)):
        trace = CR.index_trace(FIT["seed"], FIT["steps"], FIT["B"], FIT["na"], ya if balance else None, FIT["K"])
        r64 = CR.fit(sd, a, ya, FIT["K"], mean, inv, trace, FIT["lr"])
        r32 = CR.fit(sd, a, ya, FIT["K"], mean, inv, trace, FIT["lr"], dtype=torch.float32)
        drift[name] = float(np.abs(r64["loss"] - r32["loss"]).max())
    return drift


# ------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("B,T,Cn,K", [(3, 5, 3, 3), (5, 7, 4, 2), (4, 1, 2, 2)])
def test_head_gradient_matches_central_differences(B, T, Cn, K):
    rng = np.random.default_rng(11)
    out, label = rng.standard_normal((B, T, Cn)), np.arange(B) % K
    g = CR.head_with_grad(out, K, label)
    h = 1e-6
    num = np.zeros_like(out)
    for i in np.ndindex(*out.shape):
        up, dn = out.copy(), out.copy()
        up[i] += h
        dn[i] -= h
        num[i] = (CR.head_with_grad(up, K, label)["loss"] - CR.head_with_grad(dn, K, label)["loss"]) / (2 * h)
    np.testing.assert_allclose(g["dout"], num, atol=1e-8)
    assert np.all(g["dout"][:, :-1] == 0.0) and np.all(g["dout"][:, -1, K:] == 0.0)
    soft = np.exp(g["logp"])
    np.testing.assert_allclose(soft.sum(axis=1), 1.0, rtol=1e-14)
    np.testing.assert_allclose(g["dout"][:, -1, :K], (soft - np.eye(K)[label]) / B, rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(g["loss"], -g["logp"][np.arange(B), label].mean(), rtol=1e-14)


def test_ties_go_to_the_lowest_class_and_large_logits_stay_finite():
    out = np.zeros((3, 2, 4))
    out[0, -1] = [1.0, 2.0, 2.0, 0.0]            # classes 1 and 2 tie
    out[1, -1] = [5.0, 5.0, 5.0, 99.0]           # all three classes tie; channel 3 is no logit at K = 3
    out[2, -1] = [-1.0, -3.0, -1.0, 0.0]
    g = CR.head_with_grad(out, 3, np.array([0, 1, 2]))
    assert list(g["pred"]) == [1, 0, 0]
    for v in (1e4, -1e4):
        out = np.zeros((2, 3, 3))
        out[:, -1, 0] = v
        g = CR.head_with_grad(out, 3, np.array([0, 1]))
        assert np.isfinite(g["loss"]) and np.all(np.isfinite(g["logp"])) and np.all(np.isfinite(g["dout"]))
        assert abs(g["loss"] - (0.5e4 + (np.log(2.0) if v < 0 else 0.0))) <= 1e-12 * 1e4


# ------------------------------------------------------------------------------------------------ index rule
@pytest.mark.parametrize("na", [1, 7, 100003])
def test_uniform_rule_stays_in_range(na):
    for step in range(10):
        idx = CR.step_indices(99, 5, step, 130, na)
        assert idx.shape == (130,) and idx.min() >= 0 and idx.max() < na
        np.testing.assert_array_equal(idx, R.step_indices(99, 5, step, 130, na)[0])        # the predict task's draw
    words = np.array([[0, 0xFFFFFFFF, 0x80000000, 1]], dtype=np.uint32)
    assert list(CR.indices_from_words(words, 4, na)) == [0, na - 1, na // 2, 0]


def test_balanced_rule_never_names_an_absent_class_and_takes_turns():
    K, B = 4, 6
    labels = np.array([3] * 40 + [0] * 59 + [2])            # class 1 is absent, class 2 holds a single row
    rng = np.random.default_rng(3)
    rng.shuffle(labels)
    lone = int(np.flatnonzero(labels == 2)[0])
    visits = np.zeros(K, dtype=np.int64)
    for step in range(64):
        idx = CR.step_indices(7, 0, step, B, len(labels), labels, K)
        assert idx.min() >= 0 and idx.max() < len(labels)
        cls = labels[idx]
        assert not np.any(cls == 1)
        want = np.array([0, 2, 3])[(step * B + np.arange(B)) % 3]
        np.testing.assert_array_equal(cls, want)
        assert np.all(idx[cls == 2] == lone)
        visits += np.bincount(cls, minlength=K)
    assert visits[1] == 0 and visits[[0, 2, 3]].max() - visits[[0, 2, 3]].min() <= 1
    order, start = CR.class_tables(labels, K)
    assert list(start) == [0, 59, 59, 60, 100] and order[59] == lone
    assert np.all(np.diff(order[:59]) > 0)                   # stable: the rows of a class keep their order
    words = np.array([[0, 0xFFFFFFFF, 0, 0xFFFFFFFF], [0, 0xFFFFFFFF, 0, 0]], dtype=np.uint32)
    idx = CR.indices_from_words(words, 6, len(labels), 0, labels, K)
    assert list(idx) == [order[0], lone, order[60], order[58], lone, order[99]]


def test_gather_pads_the_channels():
    a = W.randn("cls_gather", (9, 4, 2), 1)
    mean, inv = np.array([0.5, -1.0], dtype=np.float32), np.array([2.0, 0.25], dtype=np.float32)
    x = CR.gather(a, np.array([3, 3, 8]), mean, inv, 5)
    assert x.shape == (3, 4, 5) and x.dtype == np.float32
    np.testing.assert_array_equal(x[:, :, :2], (a[[3, 3, 8]] - mean) * inv)
    assert np.all(x[:, :, 2:].view(np.uint32) == 0)


# ------------------------------------------------------------------------------------------------ the reference learns
def learn_data(K, C, seed):
    c = LEARN
    train, y_train = CR.ar1_classes(c["n"], c["T"], C, K, 10 * seed + 1)
    test, y_test = CR.ar1_classes(c["n_test"], c["T"], C, K, 10 * seed + 2)
    permuted = y_train[np.random.default_rng(10 * seed + 3).permutation(c["n"])]
    return train, y_train, permuted, test, y_test


def _state_dict(K, C, seed):
    c = LEARN
    return W.make_state_dict_backbone("lstm", max(C, K), c["T"], c["D"], c["L"], seed=1000 + seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K,C", list(CASES))
def test_reference_learns_the_classes(K, C, seed):
    c = LEARN
    train, y_train, permuted, test, y_test = learn_data(K, C, seed)
    score = partial(CR.classification_score, K=K, stats_from=train, seed=seed, steps=c["steps"], B=c["B"], lr=c["lr"])
    right = score(_state_dict(K, C, seed), train, y_train, test, y_test)
    wrong = score(_state_dict(K, C, seed), train, permuted, test, y_test)
    print(f"[classify ref] K={K} C={C} seed {seed}: accuracy {right['accuracy']:.3f}, permuted labels {wrong['accuracy']:.3f}")
    assert right["accuracy"] >= CASES[(K, C)]["right"]
    assert wrong["accuracy"] <= CASES[(K, C)]["permuted"]
    assert right["confusion"].sum() == c["n_test"] and np.isfinite(right["nll"])
    assert right["loss"][-1] < right["loss"][0]


def test_float32_restatement_tracks_float64():
    """The yardstick behind the drift bound of the GPU test is usable: 20 steps in float32 and in float64 agree to four digits."""
    sd, a, ya, mean, inv = fit_case()
    for balance in (False, True):
        trace = CR.index_trace(FIT["seed"], FIT["steps"], FIT["B"], FIT["na"], ya if balance else None, FIT["K"])
        r64 = CR.fit(sd, a, ya, FIT["K"], mean, inv, trace, FIT["lr"])
        r32 = CR.fit(sd, a, ya, FIT["K"], mean, inv, trace, FIT["lr"], dtype=torch.float32)
        assert np.abs(r64["loss"] - r32["loss"]).max() < 1e-4
        assert r64["loss"][-1] < r64["loss"][0]


# ------------------------------------------------------------------------------------------------ utils/posthoc.py without a GPU
def test_label_and_class_checks_have_plain_messages():
    from fourierdiffusion_amd.utils import posthoc as P
    with pytest.raises(ValueError, match="integer classes"):
        P._labels(np.zeros(4), 4, 3)
    with pytest.raises(ValueError, match="integer classes"):
        P._labels(np.zeros(4, dtype=bool), 4, 3)
    with pytest.raises(ValueError, match="one class per series"):
        P._labels(np.zeros(5, dtype=np.int64), 4, 3)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        P._labels(np.array([0, 1, 3]), 3, 3)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        P._labels(torch.tensor([0, -1, 2]), 3, 3)
    with pytest.raises(ValueError, match="missing"):
        P._labels(None, 3, 3)
    assert P._labels(torch.tensor([2, 0, 1], dtype=torch.int32), 3, 3).dtype == np.int64
    for bad in (1, 0, 257, 2.0, True):
        with pytest.raises(ValueError, match="n_classes"):
            P.PosthocNetwork(2, 24, n_classes=bad)
    x, y = np.zeros((8, 24, 2), dtype=np.float32), np.arange(8) % 3
    with pytest.raises(ValueError, match="n_classes"):
        P.classification_score(x, y, x, y, n_classes=1, stats_from=x, seed=0)
    with pytest.raises(ValueError, match=r"train_labels must lie in \[0, 2\)"):
        P.classification_score(x, y, x, y % 2, n_classes=2, stats_from=x, seed=0)
    with pytest.raises(ValueError, match="test_labels of shape"):
        P.classification_score(x, y, x, y[:5], n_classes=3, stats_from=x, seed=0)
    with pytest.raises(ValueError, match="expected"):
        P.classification_score(x, y, x[:, :12], y, n_classes=3, stats_from=x, seed=0)


def test_scores_from_confusion():
    from fourierdiffusion_amd.utils.posthoc import scores_from_confusion
    s = scores_from_confusion(np.array([[3, 1, 0], [0, 0, 0], [1, 0, 5]]))
    assert s["accuracy"] == 0.8
    np.testing.assert_allclose(s["balanced_accuracy"], 0.5 * (3 / 4 + 5 / 6))        # class 1 is absent from the test set
    np.testing.assert_allclose(s["macro_f1"], 0.5 * (2 * 3 / (4 + 4) + 2 * 5 / (6 + 5)))
    assert s["per_class_recall"][0] == 0.75 and np.isnan(s["per_class_recall"][1])
    ref = CR.scores(np.array([[3, 1, 0], [0, 0, 0], [1, 0, 5]]))
    assert ref["accuracy"] == s["accuracy"] and ref["balanced_accuracy"] == s["balanced_accuracy"]


# ------------------------------------------------------------------------------------------------ ClassificationScore, MetricCollection
def test_classification_score_refuses_bad_arguments_before_any_engine_call():
    import inspect

    from fourierdiffusion_amd.sampling.metrics import ClassificationScore
    assert ClassificationScore.views == ("time",) and ClassificationScore.needs_labels is True
    params = inspect.signature(ClassificationScore).parameters
    assert {"original_labels", "holdout_samples", "holdout_labels", "n_classes", "balance"} <= set(params)
    x, y = np.zeros((8, 24, 2), dtype=np.float32), np.arange(8) % 3
    with pytest.raises(ValueError, match="lost its time axis"):
        ClassificationScore(x.reshape(8, 48), original_labels=y)
    with pytest.raises(ValueError, match="needs original_labels"):
        ClassificationScore(x)
    with pytest.raises(ValueError, match="integer classes"):
        ClassificationScore(x, original_labels=y.astype(np.float32))
    with pytest.raises(ValueError, match="one class per sample"):
        ClassificationScore(x, original_labels=y[:5])
    with pytest.raises(ValueError, match="n_classes"):
        ClassificationScore(x, original_labels=np.zeros(8, dtype=np.int64))        # one class: largest label + 1 = 1
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        ClassificationScore(x, original_labels=y, n_classes=2)
    with pytest.raises(ValueError, match="without holdout_labels"):
        ClassificationScore(x, original_labels=y, holdout_samples=x)
    with pytest.raises(ValueError, match=r"holdout_labels must lie in \[0, 3\)"):
        ClassificationScore(x, original_labels=torch.from_numpy(y), holdout_samples=x, holdout_labels=y + 1)
    with pytest.raises(ValueError, match="<= 100"):
        ClassificationScore(x, original_labels=y, d_model=128)
    # a call without the classes of the samples is refused before anything else is looked at
    unbound = ClassificationScore.__new__(ClassificationScore)
    with pytest.raises(ValueError, match="sampler.labels"):
        unbound(x)
    with pytest.raises(ValueError, match="classes the samples were drawn for"):
        unbound(x, None)


class _StubLabelMetric:
    """A label-taking metric that needs no engine: it reports what it was handed."""
    views = ("time",)
    needs_labels = True
    baseline_metrics: dict = {}

    def __init__(self, original_samples, original_labels=None, holdout_samples=None, holdout_labels=None):
        self.bound = dict(n=len(original_samples), labels=original_labels, held=holdout_samples, held_labels=holdout_labels)

    def __call__(self, other_samples, other_labels=None):
        return {"stub_n": len(other_samples), "stub_labels": None if other_labels is None else [int(v) for v in other_labels]}


class _StubPlainMetric:
    views = ("time",)                                        # (the freq view maps the samples on the engine)
    baseline_metrics: dict = {}

    def __init__(self, original_samples, holdout_samples=None):
        self.held = holdout_samples

    def __call__(self, other_samples):                       # a second argument would be a TypeError
        return {"plain_sum": float(torch.as_tensor(other_samples).abs().sum())}


def test_collection_hands_labels_only_to_the_metrics_that_take_them():
    from fourierdiffusion_amd.sampling.metrics import MetricCollection
    x = torch.from_numpy(W.randn("cls_coll", (6, 8, 2), 1))
    y, yh, yo = np.arange(6) % 2, np.arange(4) % 2, np.array([1, 0, 1])
    coll = MetricCollection([partial(_StubLabelMetric), partial(_StubPlainMetric)], original_samples=x, holdout_samples=x[:4],
                            original_labels=y, holdout_labels=yh, include_baselines=True)
    stub, plain = coll.metrics_time
    assert stub.bound["labels"] is y and stub.bound["held_labels"] is yh and len(stub.bound["held"]) == 4
    assert plain.held is not None and coll.metrics_freq == []
    res = coll(x[:3], other_labels=yo)
    assert res["time_stub_labels"] == [1, 0, 1] and res["time_stub_n"] == 3 and "freq_stub_n" not in res
    assert coll(x[:3])["time_stub_labels"] is None
    # held-out samples without their labels do not reach a label-taking metric
    coll = MetricCollection([partial(_StubLabelMetric)], original_samples=x, holdout_samples=x[:4], original_labels=y)
    assert coll.metrics_time[0].bound["held"] is None and coll.metrics_time[0].bound["held_labels"] is None
    # a collection without a label-aware metric: the same results with and without labels, and its factories see no label
    plain_only = MetricCollection([partial(_StubPlainMetric)], original_samples=x, original_labels=y, holdout_labels=yh)
    assert plain_only(x[:3]) == plain_only(x[:3], other_labels=yo) == plain_only(x[:3], yo)
    assert set(plain_only(x[:3])) == {"time_plain_sum"}


# ------------------------------------------------------------------------------------------------ config
def test_conditional_config_composes_and_names_the_class():
    import fdiff.sampling.metrics as alias
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.metrics import ClassificationScore, MarginalWasserstein, MetricCollection, SlicedWasserstein
    assert alias.ClassificationScore is ClassificationScore
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "sample", ["metrics=conditional", "random_seed=7"]).metrics
    assert cfg.holdout is True and cfg.labels is True
    make = instantiate({k: v for k, v in cfg.items() if k not in ("holdout", "labels")})
    assert isinstance(make, partial) and make.func is MetricCollection
    assert make.keywords["include_spectral_density"] is True and make.keywords["include_baselines"] is True
    assert [m.func for m in make.keywords["metrics"]] == [SlicedWasserstein, MarginalWasserstein, ClassificationScore]
    assert make.keywords["metrics"][2].keywords == dict(steps=2000, batch_size=128, lr=0.001, d_model=32, num_layers=1, max_samples=10000,
                                                        random_seed=7, n_classes=None, balance=False)
    assert [dict(m) for m in cfg.metrics[:2]] == [dict(m) for m in compose(conf, "sample", ["random_seed=7"]).metrics.metrics]


def test_default_and_posthoc_configs_compose_to_what_they_did():
    from fourierdiffusion_amd.config import compose
    conf = os.path.join(ROOT, "cmd", "conf")
    default = compose(conf, "sample", []).metrics
    assert "holdout" not in default and "labels" not in default
    assert [m["_target_"].rsplit(".", 1)[1] for m in default.metrics] == ["SlicedWasserstein", "MarginalWasserstein"]
    posthoc = compose(conf, "sample", ["metrics=posthoc"]).metrics
    assert posthoc.holdout is True and "labels" not in posthoc
    assert [m["_target_"].rsplit(".", 1)[1] for m in posthoc.metrics] == ["SlicedWasserstein", "MarginalWasserstein",
                                                                          "DiscriminativeScore", "PredictiveScore"]
    assert {k: v for k, v in dict(posthoc.metrics[2]).items() if k not in ("_target_", "_partial_", "random_seed")} == dict(
        steps=2000, batch_size=128, lr=0.001, d_model=32, num_layers=1, test_fraction=0.2, max_samples=10000)
