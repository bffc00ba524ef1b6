"""CPU: banded dynamic time warping (an extension, not in the reference) -- the float64 restatement of tests/dtw_ref.py against an
independent enumeration of warping paths and against the properties the metrics lean on, the error bound of the GPU tests against a
float32 restatement of the kernel's cell, every host-side check of utils/dtw.py and of the two Metric classes with no device
present, the view logic of MetricCollection, and the shifted-replay experiment the feature exists for."""
import ctypes
import itertools
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests import dtw_ref as R
from tests import knn_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fd_dtw_pairs", "fd_dtw_knn_workspace_bytes", "fd_dtw_knn", "fd_dtw_ball_counts_workspace_bytes", "fd_dtw_ball_counts")


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in SYMBOLS:
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


# ---------------------------------------------------------------------------------------------- the reference's own algebra
@pytest.mark.parametrize("T,C", [(1, 1), (2, 1), (3, 2), (4, 1), (5, 3)])
def test_ref_recurrence_is_the_minimum_over_all_warping_paths(T, C):
    rs = np.random.RandomState(10 * T + C)
    a, b = rs.randn(6, T, C), rs.randn(6, T, C)
    for w in range(T):
        got = R.dtw2(a, b, w)
        want = np.array([R.dtw2_paths(a[p], b[p], w) for p in range(6)])
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


def test_ref_window_zero_is_squared_euclidean_and_the_matrix_form_agrees():
    rs = np.random.RandomState(1)
    q, r = rs.randn(7, 12, 3), rs.randn(9, 12, 3)
    np.testing.assert_allclose(R.dtw2_matrix(q, r, 0), K.dist2(q, r), rtol=1e-13)
    M = R.dtw2_matrix(q, r, 4)
    for i, j in itertools.product(range(7), range(9)):
        assert M[i, j] == R.dtw2(q[i:i + 1], r[j:j + 1], 4)[0]
    assert R.dtw2(rs.randn(3, 12), rs.randn(3, 12), 2).shape == (3,)          # (n, T) is read as C = 1


def test_ref_does_not_increase_with_the_window_and_is_symmetric():
    rs = np.random.RandomState(2)
    a, b = rs.randn(20, 17, 2), rs.randn(20, 17, 2)
    prev = None
    for w in range(17):
        d = R.dtw2(a, b, w)
        assert np.array_equal(d, R.dtw2(b, a, w))                 # the same float64 operations in the same order: bit for bit
        if prev is not None:
            assert (d <= prev).all()
        prev = d
    assert (prev < R.dtw2(a, b, 0)).any() and (R.dtw2(a, a, 3) == 0.0).all()


@pytest.mark.parametrize("T,C,w", [(24, 1, 3), (24, 3, 3), (37, 5, 36), (48, 1, 5), (64, 1, 63), (30, 40, 3), (187, 1, 19)])
def test_float32_cell_stays_inside_the_bound(T, C, w):
    """dtw_bound is the worst case of what the kernel computes: its cell restated in float32 numpy stays far inside."""
    rs = np.random.RandomState(T + C + w)
    a, b = rs.randn(30, T, C).astype(np.float32), (rs.randn(30, T, C) * 1.1 + 0.05).astype(np.float32)
    want = R.dtw2(a, b, w)
    got = R.dtw2_f32(a, b, w).astype(np.float64)
    rel = np.abs(got - want) / want
    print(f"[dtw] float32 cell, T={T} C={C} w={w}: max error / bound {rel.max() / R.dtw_bound(T, C):.3e}")
    assert (rel <= R.dtw_bound(T, C)).all() and rel.max() > 0
    assert np.array_equal(R.dtw2_f32(a, b, w), R.dtw2_f32(b, a, w))            # and it is symmetric bit for bit
    assert (R.dtw2_f32(a, a, w) == 0.0).all()


def test_default_window():
    from fourierdiffusion_amd.utils.dtw import default_window
    for T, want in ((1, 0), (2, 1), (5, 1), (10, 1), (11, 2), (24, 3), (134, 14), (187, 19), (251, 26), (252, 26), (365, 37), (1024, 103)):
        assert default_window(T) == want == R.default_window(T), T
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="T="):
            default_window(bad)


# ---------------------------------------------------------------------------------------------- argument checks
def test_dtw_functions_refuse_bad_arguments_before_the_device():
    from fourierdiffusion_amd.utils.dtw import dtw_ball_counts, dtw_knn, dtw_pairs
    q, r = np.zeros((5, 12, 2), np.float32), np.zeros((7, 12, 2), np.float32)
    for bad_k in (0, -1, 8, 17, 2.5):
        with pytest.raises(ValueError, match="k="):
            dtw_knn(q, r, bad_k)
    with pytest.raises(ValueError, match="k="):
        dtw_knn(r, r, 7, exclude_self=True)                      # only 6 other series
    with pytest.raises(ValueError, match="k="):
        dtw_knn(q, np.zeros((40, 12, 2), np.float32), 17)
    with pytest.raises(ValueError, match="exclude_self"):
        dtw_knn(q, r, 1, exclude_self=True)
    for bad_w in (-1, 12, 1.5, "wide", True):
        with pytest.raises(ValueError, match="window="):
            dtw_knn(q, r, 1, window=bad_w)
        with pytest.raises(ValueError, match="window="):
            dtw_pairs(q, q, window=bad_w)
        with pytest.raises(ValueError, match="window="):
            dtw_ball_counts(q, r, np.ones(7), window=bad_w)
    long = np.zeros((2, 600, 1), np.float32)
    with pytest.raises(ValueError, match="band column"):
        dtw_pairs(long, long, window=128)                        # 257 entries
    with pytest.raises(ValueError, match="band column"):
        dtw_knn(long, long, 1, window="full")
    with pytest.raises(ValueError, match="at most 1024"):
        dtw_pairs(np.zeros((2, 1025), np.float32), np.zeros((2, 1025), np.float32))
    with pytest.raises(ValueError, match="equal lengths"):
        dtw_knn(q, np.zeros((7, 11, 2), np.float32), 1)
    with pytest.raises(ValueError, match="equal lengths"):
        dtw_knn(q, np.zeros((7, 12, 3), np.float32), 1)
    with pytest.raises(ValueError, match="equal lengths"):
        dtw_pairs(q, np.zeros((5, 24), np.float32))              # (n, T) is C = 1, not a flattened (T, C)
    with pytest.raises(ValueError, match="non-empty"):
        dtw_knn(np.zeros((0, 12, 2), np.float32), r, 1)
    with pytest.raises(ValueError, match="non-empty"):
        dtw_knn(np.zeros((5,), np.float32), r, 1)
    with pytest.raises(ValueError, match="non-empty"):
        dtw_ball_counts(q, np.zeros((7, 12, 2, 1), np.float32), np.zeros(7))
    with pytest.raises(ValueError, match="series and b"):
        dtw_pairs(q, r)
    with pytest.raises(ValueError, match="radii for"):
        dtw_ball_counts(q, r, np.zeros(6))
    for bad in (-1e-3, np.nan, np.inf):
        rad = np.ones(7)
        rad[3] = bad
        with pytest.raises(ValueError, match="finite"):
            dtw_ball_counts(q, r, rad)
        with pytest.raises(ValueError, match="finite"):
            dtw_ball_counts(q, r, torch.from_numpy(rad))


def test_metric_classes_refuse_bad_arguments_before_the_device():
    from fourierdiffusion_amd.sampling.metrics import DTWMemorisation, DTWPrecisionRecall
    X = np.zeros((20, 12, 2), np.float32)
    for cls in (DTWPrecisionRecall, DTWMemorisation):
        with pytest.raises(ValueError, match="lost its time axis"):
            cls(X.reshape(20, 24))
        with pytest.raises(ValueError, match="lost its time axis"):
            cls(torch.zeros(20, 24))
        for bad_w in (-1, 12, "wide"):
            with pytest.raises(ValueError, match="window="):
                cls(X, window=bad_w)
    for bad_k in (0, 17, 1.5):
        with pytest.raises(ValueError, match="k="):
            DTWPrecisionRecall(X, k=bad_k)
    with pytest.raises(ValueError, match="max_original"):
        DTWPrecisionRecall(X, k=5, max_original=5)
    with pytest.raises(ValueError, match="cannot supply"):
        DTWPrecisionRecall(X[:5], k=5)
    with pytest.raises(ValueError, match="at least two"):
        DTWMemorisation(X[:1])
    with pytest.raises(ValueError, match="empty"):
        DTWMemorisation(X, holdout_samples=X[:0])


# ---------------------------------------------------------------------------------------------- MetricCollection, config
class _Both:
    def __init__(self, original_samples, scale=1.0):
        self.original, self.scale = original_samples, scale

    def __call__(self, other):
        return {"gap": float((other.mean() - self.original.mean()) * self.scale)}

    baseline_metrics = {"gap_self": 0.0}


class _TimeOnly(_Both):
    views = ("time",)

    def __init__(self, original_samples, holdout_samples=None):
        super().__init__(original_samples)
        self.holdout = holdout_samples

    def __call__(self, other):
        return {"rows": int(other.shape[0])}

    baseline_metrics = {"rows_self": 1}


def test_metric_collection_binds_a_class_only_in_the_views_it_names(monkeypatch):
    from fourierdiffusion_amd.sampling import metrics as M
    monkeypatch.setattr(M, "dft", lambda x: 2.0 * x)              # the views' transforms run on the engine; any map does here
    X, Y, H = torch.arange(24.0).reshape(4, 3, 2), torch.ones(5, 3, 2), torch.zeros(6, 3, 2)
    plain = M.MetricCollection(metrics=[partial(_Both, scale=3.0)], original_samples=X)(Y)
    assert list(plain) == ["freq_gap", "freq_gap_self", "time_gap", "time_gap_self"]
    both = M.MetricCollection(metrics=[partial(_Both, scale=3.0), partial(_TimeOnly)], original_samples=X, holdout_samples=H)
    got = both(Y)
    assert list(got) == ["freq_gap", "freq_gap_self", "time_gap", "time_gap_self", "time_rows", "time_rows_self"]
    assert {key: got[key] for key in plain} == plain and got["time_rows"] == 5
    assert [type(m) for m in both.metrics_time] == [_Both, _TimeOnly] and [type(m) for m in both.metrics_freq] == [_Both]
    assert torch.equal(both.metrics_time[1].holdout, H)
    alone = M.MetricCollection(metrics=[partial(_TimeOnly)], original_samples=X)
    assert list(alone(Y)) == ["time_rows", "time_rows_self"] and alone.metrics_freq == []
    # every class of the package keeps both views, the two new ones name the time view
    for name in ("SlicedWasserstein", "MarginalWasserstein", "PrecisionRecall", "Memorisation", "KernelTwoSample"):
        assert getattr(M, name).views == ("time", "freq"), name
    assert M.DTWPrecisionRecall.views == M.DTWMemorisation.views == ("time",)


def test_new_config_composes_and_the_others_are_untouched():
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.metrics import (DTWMemorisation, DTWPrecisionRecall, MarginalWasserstein, Memorisation,
                                                       MetricCollection, PrecisionRecall, SlicedWasserstein)
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "sample", ["metrics=dtw", "random_seed=7"]).metrics
    assert cfg.holdout is True
    make = instantiate({k: v for k, v in cfg.items() if k != "holdout"})
    assert isinstance(make, partial) and make.func is MetricCollection
    assert make.keywords["include_spectral_density"] is True and make.keywords["include_baselines"] is True
    kinds = [m.func for m in make.keywords["metrics"]]
    assert kinds == [SlicedWasserstein, MarginalWasserstein, PrecisionRecall, Memorisation, DTWPrecisionRecall, DTWMemorisation]
    assert make.keywords["metrics"][4].keywords == {"k": 5, "random_seed": 7, "window": None}
    assert make.keywords["metrics"][5].keywords == {"random_seed": 7, "window": None}
    # the first four entries are the `neighbours` list, word for word
    neighbours = compose(conf, "sample", ["metrics=neighbours", "random_seed=7"]).metrics
    assert [dict(m) for m in cfg.metrics[:4]] == [dict(m) for m in neighbours.metrics]
    assert DTWPrecisionRecall.__init__.__code__.co_varnames[1:6] == ("original_samples", "k", "max_original", "random_seed", "window")


# ---------------------------------------------------------------------------------------------- the shifted-replay experiment
def test_ref_shifted_replays_are_found_by_dtw_and_missed_by_euclid():
    """A generator that replays its training series three samples late: the Euclidean nearest training row is mostly NOT the source
    and many replays pass for authentic; under banded DTW every replay is found at its source and none is authentic, while fresh
    draws keep theirs."""
    f = R.replay_fixture()
    train, replay, fresh, w = f["train"], f["replay"], f["fresh"], f["window"]
    n = train.shape[0]
    E_rt, E_tt = K.dist2(replay, train), K.dist2(train, train)
    D_rt, D_tt, D_ft = R.dtw2_matrix(replay, train, w), R.dtw2_matrix(train, train, w), R.dtw2_matrix(fresh, train, w)
    found_euclid = float((np.argmin(E_rt, axis=1) == np.arange(n)).mean())
    found_dtw = float((np.argmin(D_rt, axis=1) == np.arange(n)).mean())
    auth_euclid = R.memorisation(E_rt, E_tt)["authenticity"]
    auth_replay = R.memorisation(D_rt, D_tt)["authenticity"]
    auth_fresh = R.memorisation(D_ft, D_tt)["authenticity"]
    print(f"[replay] source found: euclid {found_euclid:.3f}, dtw {found_dtw:.3f}; authenticity: euclid {auth_euclid:.3f}, "
          f"dtw replay {auth_replay:.3f}, dtw fresh {auth_fresh:.3f}")
    assert found_euclid < 0.5
    assert found_dtw == 1.0
    assert auth_replay == 0.0
    assert auth_fresh > 0.25
