"""CPU: nearest-neighbour metrics (an extension, not in the reference) -- the float64 restatement of tests/knn_ref.py has the
properties the metrics are read by, the argument checks of utils/neighbours.py and of the two Metric classes fire before anything
touches a device, MetricCollection without a holdout is what it was, and the new entry points and config exist."""
import ctypes
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests import knn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_knn_rows_workspace_bytes", "fd_knn_rows", "fd_ball_counts"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


# ---------------------------------------------------------------------------------------------- the reference's own algebra
def test_ref_knn_orders_by_distance_then_index():
    r = np.array([[0.0], [1.0], [1.0], [3.0], [-1.0]])
    d, i = R.knn(np.array([[0.0], [2.0]]), r, 4)
    np.testing.assert_array_equal(i, [[0, 1, 2, 4], [1, 2, 3, 0]])
    np.testing.assert_array_equal(d, [[0, 1, 1, 1], [1, 1, 1, 4]])
    d, i = R.knn(r, r, 2, exclude_self=True)
    np.testing.assert_array_equal(i, [[1, 2], [2, 0], [1, 0], [1, 2], [0, 1]])
    np.testing.assert_array_equal(R.ball_counts(np.array([[0.0], [2.0]]), r, [0.0, 1.0, 0.5, 1.0, 4.0]), [3, 2])


def test_ref_identical_sets_score_one_and_disjoint_sets_zero():
    rs = np.random.RandomState(0)
    X = rs.randn(120, 6)
    same = R.precision_recall(X, X, k=3)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["density"] > 1.0
    far = R.precision_recall(X, rs.randn(90, 6) + 100.0, k=3)
    assert far == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}


def test_ref_mode_collapse_keeps_precision_and_loses_recall():
    rs = np.random.RandomState(1)
    X = np.concatenate([rs.randn(100, 4), rs.randn(100, 4) + 20.0])
    got = R.precision_recall(X, rs.randn(100, 4), k=3)          # only the first mode
    assert got["precision"] >= 0.8 and 0.3 <= got["recall"] <= 0.6 and 0.3 <= got["coverage"] <= 0.6


def test_ref_replayed_rows_are_not_authentic():
    rs = np.random.RandomState(2)
    X, H = rs.randn(200, 8), rs.randn(200, 8)
    replay = R.memorisation(X, X[:150] + 1e-6 * rs.randn(150, 8), holdout=H)
    assert replay["authenticity"] == 0.0 and replay["train_closer_share"] == 1.0 and replay["nn_distance_median"] < 1e-4
    exact = R.memorisation(X, X[:50], holdout=np.concatenate([X[:10], H[:190]]))
    assert exact["nn_distance_min"] == 0.0 and exact["authenticity"] == 0.0
    assert exact["train_closer_share"] == pytest.approx((40 + 0.5 * 10) / 50)       # rows that are in both sets tie: one half


def test_ref_independent_draw_is_as_near_to_the_holdout_as_to_the_training_set():
    rs = np.random.RandomState(3)
    X, H, G = rs.randn(400, 8), rs.randn(400, 8), rs.randn(400, 8)
    got = R.memorisation(X, G, holdout=H)
    assert abs(got["train_closer_share"] - 0.5) <= 0.1
    assert got["authenticity"] >= 0.3
    # a training set larger than the holdout is subsampled to its size, or the share would only measure the sizes
    big = R.memorisation(np.concatenate([X, rs.randn(1200, 8)]), G, holdout=H, seed=5)
    assert abs(big["train_closer_share"] - 0.5) <= 0.1


def test_ref_expansion_bound_covers_the_f32_expansion():
    """The band of the GPU tests is the worst case of what the engine computes: restated here in f32 numpy on shifted data."""
    rs = np.random.RandomState(4)
    q, r = (rs.randn(40, 62) + 3.0).astype(np.float32), (rs.randn(50, 62) + 3.0).astype(np.float32)
    mu = r.astype(np.float64).mean(axis=0).astype(np.float32)
    qc, rc = q - mu, r - mu
    qn = (qc.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    rn = (rc.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    dot = np.zeros((40, 50), np.float32)
    for c in range(62):
        dot = dot + qc[:, c:c + 1] * rc[None, :, c]
    got = (qn[:, None] + rn[None, :]) - 2.0 * dot
    err = np.abs(got.astype(np.float64) - R.dist2(q, r))
    assert (err <= R.expansion_bound(q, r)).all() and err.max() > 0


# ---------------------------------------------------------------------------------------------- argument checks
def test_knn_and_ball_counts_refuse_bad_arguments_before_the_device():
    from fourierdiffusion_amd.utils.neighbours import ball_counts, knn
    q, r = np.zeros((5, 4), np.float32), np.zeros((7, 4), np.float32)
    for bad_k in (0, -1, 8, 17, 2.5):
        with pytest.raises(ValueError, match="k="):
            knn(q, r, bad_k)
    with pytest.raises(ValueError, match="k="):
        knn(r, r, 7, exclude_self=True)                          # only 6 other rows
    with pytest.raises(ValueError, match="k="):
        knn(q, np.zeros((40, 4), np.float32), 17)
    with pytest.raises(ValueError, match="exclude_self"):
        knn(q, r, 1, exclude_self=True)
    with pytest.raises(ValueError, match="features"):
        knn(q, np.zeros((7, 3), np.float32), 1)
    with pytest.raises(ValueError, match="non-empty"):
        knn(np.zeros((0, 4), np.float32), r, 1)
    with pytest.raises(ValueError, match="non-empty"):
        ball_counts(q, np.zeros((7,), np.float32), np.zeros(7))
    with pytest.raises(ValueError, match="radii for"):
        ball_counts(q, r, np.zeros(6))
    for bad in (-1e-3, np.nan, np.inf):
        rad = np.ones(7)
        rad[3] = bad
        with pytest.raises(ValueError, match="finite"):
            ball_counts(q, r, rad)
        with pytest.raises(ValueError, match="finite"):
            ball_counts(q, r, torch.from_numpy(rad))


def test_metric_classes_refuse_bad_arguments_before_the_device():
    from fourierdiffusion_amd.sampling.metrics import Memorisation, PrecisionRecall
    X = np.zeros((20, 5, 2), np.float32)
    for bad_k in (0, 17, 1.5):
        with pytest.raises(ValueError, match="k="):
            PrecisionRecall(X, k=bad_k)
    with pytest.raises(ValueError, match="max_original"):
        PrecisionRecall(X, k=5, max_original=5)
    with pytest.raises(ValueError, match="max_original"):
        PrecisionRecall(X, k=5, max_original=7.5)
    with pytest.raises(ValueError, match="cannot supply"):
        PrecisionRecall(X[:5], k=5)
    with pytest.raises(ValueError, match="at least two"):
        Memorisation(X[:1])
    with pytest.raises(ValueError, match="empty"):
        Memorisation(X, holdout_samples=X[:0])


def test_subsample_is_the_reference_restatement():
    from fourierdiffusion_amd.sampling.metrics import subsample_indices
    got = subsample_indices(1000, 100, 7)
    np.testing.assert_array_equal(got, R.subsample_indices(1000, 100, 7))
    assert len(set(got.tolist())) == 100 and (np.diff(got) > 0).all() and got.min() >= 0 and got.max() < 1000


# ---------------------------------------------------------------------------------------------- MetricCollection
class _Plain:
    """A metric with today's constructor: original samples and its own arguments."""

    def __init__(self, original_samples, scale=1.0):
        self.original, self.scale = original_samples, scale

    def __call__(self, other):
        return {"plain_gap": float((other.mean() - self.original.mean()) * self.scale)}

    baseline_metrics = {"plain_gap_self": 0.0}


class _Held(_Plain):
    def __init__(self, original_samples, holdout_samples=None, scale=1.0):
        super().__init__(original_samples, scale)
        self.holdout = holdout_samples

    def __call__(self, other):
        return {"held_rows": -1 if self.holdout is None else int(self.holdout.shape[0])}

    baseline_metrics = {}


def test_metric_collection_without_holdout_is_unchanged_and_with_it_binds_per_view(monkeypatch):
    from fourierdiffusion_amd.sampling import metrics as M
    monkeypatch.setattr(M, "dft", lambda x: 2.0 * x)              # the views' transforms run on the engine; any map does here
    X, Y, H = torch.arange(24.0).reshape(4, 3, 2), torch.ones(5, 3, 2), torch.zeros(6, 3, 2)
    today = M.MetricCollection(metrics=[partial(_Plain, scale=3.0)], original_samples=X)
    keys = ["freq_plain_gap", "freq_plain_gap_self", "time_plain_gap", "time_plain_gap_self"]
    res = today(Y)
    assert list(res) == keys and res["time_plain_gap"] == (1.0 - 11.5) * 3.0 and res["freq_plain_gap"] == (2.0 - 23.0) * 3.0
    explicit = M.MetricCollection(metrics=[partial(_Plain, scale=3.0)], original_samples=X, holdout_samples=None)
    assert explicit(Y) == res
    # a holdout reaches only the classes that take one, mapped into each view; everything else is bound as before
    both = M.MetricCollection(metrics=[partial(_Plain, scale=3.0), partial(_Held)], original_samples=X, holdout_samples=H)
    got = both(Y)
    assert {k: got[k] for k in keys} == res and got["time_held_rows"] == 6 and got["freq_held_rows"] == 6
    assert isinstance(both.metrics_time[0], _Plain) and both.metrics_time[1].holdout is not None
    assert torch.equal(both.metrics_freq[1].holdout, 2.0 * H) and torch.equal(both.metrics_time[1].holdout, H)
    none = M.MetricCollection(metrics=[partial(_Held)], original_samples=X)
    assert none(Y)["time_held_rows"] == -1


def test_new_config_instantiates_and_default_is_untouched():
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.metrics import (MarginalWasserstein, Memorisation, MetricCollection, PrecisionRecall,
                                                       SlicedWasserstein)
    conf = os.path.join(ROOT, "cmd", "conf")
    default = compose(conf, "sample", []).metrics
    assert "holdout" not in default and [m["_target_"].rsplit(".", 1)[1] for m in default.metrics] == [
        "SlicedWasserstein", "MarginalWasserstein"]
    cfg = compose(conf, "sample", ["metrics=neighbours", "random_seed=7"]).metrics
    assert cfg.holdout is True
    make = instantiate({k: v for k, v in cfg.items() if k != "holdout"})
    assert isinstance(make, partial) and make.func is MetricCollection
    assert make.keywords["include_spectral_density"] is True and make.keywords["include_baselines"] is True
    kinds = [m.func for m in make.keywords["metrics"]]
    assert kinds == [SlicedWasserstein, MarginalWasserstein, PrecisionRecall, Memorisation]
    assert make.keywords["metrics"][2].keywords == {"k": 5, "random_seed": 7}
    assert make.keywords["metrics"][3].keywords == {"random_seed": 7}
    # the first two entries are the default list, word for word
    assert [dict(m) for m in cfg.metrics[:2]] == [dict(m) for m in compose(conf, "sample", ["random_seed=7"]).metrics.metrics]
