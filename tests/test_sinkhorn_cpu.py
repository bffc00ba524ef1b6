"""CPU: the Sinkhorn divergence (an extension, not in the reference) -- the float64 reference of tests/sinkhorn_ref.py is consistent
with what entropic transport must satisfy (the assignment cost up to the entropic gap, S(X, X) = 0, S >= 0, the sorted-quantile
W2 in one dimension, a marginal error that falls with the iterations), its float32 restatement of the engine's arithmetic stays
inside the derived bound, the schedule is what the contract says, every argument check fires before anything touches a device,
and the new entry points, config and result keys exist."""
import ctypes
import os
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mmd_ref as W
from tests import sinkhorn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_softmin_pairs_workspace_bytes", "fd_softmin_pairs", "fd_sinkhorn_potentials_workspace_bytes",
                 "fd_sinkhorn_potentials"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


# ---------------------------------------------------------------------------------------------- the reference itself
def schedule(reg, n_final, base):
    """The default descent, then reg n_final times (the reference takes any number of iterations), in absolute units."""
    from fourierdiffusion_amd.utils.sinkhorn import epsilon_schedule
    return np.concatenate([epsilon_schedule(reg, n_final=1)[:-1], np.full(n_final, reg)]) * base


@pytest.mark.parametrize("n,d", [(2, 1), (5, 3), (7, 4)])
def test_entropic_cost_is_the_assignment_cost_up_to_the_entropic_gap(n, d):
    """OT_0 <= OT_eps <= OT_0 + eps log n for uniform weights (the plan of the best permutation has KL(pi | a x b) = log n), and
    the dual value <a, f> + <b, g> of a converged iteration is OT_eps."""
    rng = np.random.default_rng(n * 10 + d)
    x, y = rng.standard_normal((n, d)), rng.standard_normal((n, d)) + 0.5
    base = R.eps_base(x, y)
    exact = R.assignment_cost(x, y)
    for reg in (0.05, 0.01):
        eps = reg * base
        r = R.divergence(x, y, schedule(reg, 3000, base))
        assert r["marginal_error"] < 1e-4
        assert exact - 1e-6 * base <= r["ot_xy"] <= exact + eps * np.log(n) + 1e-9 * base, (reg, exact, r["ot_xy"])


def test_divergence_of_a_set_with_itself_is_zero_and_otherwise_positive():
    rng = np.random.default_rng(3)
    x, y = W.waves(rng, 40, 12), 0.9 * W.waves(rng, 55, 12)
    base = R.eps_base(x, y)
    a = rng.uniform(0.5, 1.5, 40)
    a /= a.sum()
    # x against a copy of itself runs the alternating iteration, whose (f, g) reach the symmetric potential (up to the constant
    # that f + c, g - c leaves free) only in the limit
    same = [abs(R.divergence(x, x.copy(), schedule(0.05, k, base), a, a)["divergence"]) for k in (200, 1000, 3000)]
    assert same[0] > same[1] > same[2] and same[2] <= 1e-5 * base, same
    sched = schedule(0.05, 200, base)
    for wx in (None, a):
        r = R.divergence(x, y, sched, wx, None)
        assert r["divergence"] > 0 and r["w2"] == np.sqrt(r["divergence"]) and r["divergence"] < r["ot_xy"]
    tiny = R.divergence(x, x + 1e-3, schedule(0.05, 3000, base))      # W2^2 = 12 * 1e-6, up to what the iteration still lacks
    assert -1e-5 * base <= tiny["divergence"] < 1e-4


def test_one_dimensional_w2_approaches_the_sorted_quantile_distance_as_reg_falls():
    rng = np.random.default_rng(8)
    x, y = rng.standard_normal((60, 1)), 1.5 * rng.standard_normal((60, 1)) + 1.0
    base = R.eps_base(x, y)
    exact = R.w2_sorted(x, y)
    gaps = [abs(R.divergence(x, y, schedule(reg, 4000, base))["w2"] - exact) for reg in (0.5, 0.1, 0.02, 0.004)]
    assert all(later < earlier for earlier, later in zip(gaps, gaps[1:])), gaps
    assert gaps[-1] <= 0.02 * exact, (gaps, exact)


def test_marginal_error_falls_with_the_iterations():
    rng = np.random.default_rng(4)
    x, y = W.waves(rng, 60, 20), W.waves(rng, 45, 20)
    base = R.eps_base(x, y)
    errs = [R.divergence(x, y, schedule(0.05, k, base))["marginal_error"] for k in (1, 5, 20, 80)]
    assert all(later < earlier for earlier, later in zip(errs, errs[1:])) and errs[-1] < 1e-3, errs


def test_closed_form_of_eps_base_is_the_mean_pair_distance():
    rng = np.random.default_rng(5)
    x, y = W.waves(rng, 30, 13) + 2.0, W.waves(rng, 11, 13)
    z = np.concatenate([x, y])
    closed = 2.0 * ((z - z.mean(axis=0)) ** 2).sum() / (len(z) - 1)
    assert R.eps_base(x, y) == pytest.approx(closed, rel=1e-12)
    assert R.eps_base_closed(x, y) == closed and R.eps_base_closed(x) == pytest.approx(R.eps_base(x), rel=1e-12)
    assert R.eps_base(x[:1]) == 1.0 and R.eps_base(np.ones((4, 3))) == 1.0 and R.eps_base_closed(np.ones((4, 3))) == 1.0


@pytest.mark.parametrize("n,m,d", [(5, 7, 3), (129, 127, 17), (40, 300, 9)])
def test_float32_restatement_stays_inside_the_derived_bound(n, m, d):
    rng = np.random.default_rng(n + m + d)
    x, y = W.waves(rng, n, d).astype(np.float32), (W.waves(rng, m, d) + 3.0).astype(np.float32)
    base = R.eps_base(x, y)
    D = R.dist2(x, y)
    h = base * rng.standard_normal(m)
    xc, yc, xn, yn = R.centred_f32(x, y)
    for reg in (1.0, 0.05, 0.01):
        eps = reg * base
        err = np.abs(R.softmin_f32(xc, yc, xn, yn, h, eps) - R.softmin(D, h, eps))
        bound = R.error_bounds(x, y, h, eps, D)
        assert (err <= bound).all() and err.max() > 0, (reg, (err / bound).max())
    a, b = R.uniform(n), R.uniform(m)
    sched = schedule(0.05, 6, base)
    f, g, bf, bg = R.potentials_with_bounds(x, y, a, b, sched, D)
    np.testing.assert_array_equal(R.potentials(D, a, b, sched)[1], g)
    f32, g32 = R.potentials_f32(x, y, a, b, sched)
    assert 0 < np.abs(f32 - f).max() <= bf and 0 < np.abs(g32 - g).max() <= bg
    p, bp = R.symmetric_with_bound(x, a, sched)
    np.testing.assert_array_equal(R.potentials_symmetric(R.dist2(x, x), a, sched), p)
    assert 0 < np.abs(R.potentials_symmetric_f32(x, a, sched) - p).max() <= bp


# ---------------------------------------------------------------------------------------------- schedule, arguments
def test_epsilon_schedule_values():
    from fourierdiffusion_amd.utils.sinkhorn import MAX_STEPS, epsilon_schedule
    np.testing.assert_array_equal(epsilon_schedule(0.05), [4.0, 1.0, 0.25, 0.0625] + [0.05] * 20)
    np.testing.assert_array_equal(epsilon_schedule(0.3, scaling=0.5, n_final=2, start=1.0), [1.0, 0.3, 0.3])
    np.testing.assert_array_equal(epsilon_schedule(2.0, n_final=3, start=1.0), [2.0, 2.0, 2.0])       # reg above the start: no descent
    s = epsilon_schedule(0.01, scaling=0.9, n_final=1)
    assert s[0] == 4.0 and s[-1] == 0.01 and (np.diff(s) < 0).all() and np.allclose(s[1:-1] / s[:-2], 0.81)
    assert epsilon_schedule(0.25, n_final=1).tolist() == [4.0, 1.0, 0.25]                               # reg on the grid comes once
    assert s.dtype == np.float64 and len(epsilon_schedule(0.05, n_final=MAX_STEPS - 4)) == MAX_STEPS
    for kwargs, needle in (({"reg": 0.0}, "reg"), ({"reg": -1.0}, "reg"), ({"reg": np.nan}, "reg"), ({"reg": np.inf}, "reg"),
                           ({"reg": 0.1, "scaling": 0.0}, "scaling"), ({"reg": 0.1, "scaling": 1.0}, "scaling"),
                           ({"reg": 0.1, "n_final": 0}, "n_final"), ({"reg": 0.1, "n_final": 2.5}, "n_final"),
                           ({"reg": 0.1, "n_final": True}, "n_final"), ({"reg": 0.1, "start": 0.0}, "start"),
                           ({"reg": 0.05, "n_final": MAX_STEPS - 3}, "at most"), ({"reg": 1e-9, "scaling": 0.99}, "at most")):
        with pytest.raises(ValueError, match=needle):
            epsilon_schedule(**kwargs)


def test_functions_refuse_bad_arguments_before_the_device():
    from fourierdiffusion_amd.utils.sinkhorn import sinkhorn_divergence, sinkhorn_potentials, softmin_pairs
    x, y, h = np.zeros((6, 4), np.float32), np.zeros((5, 4), np.float32), np.zeros(5)
    for fn in (lambda a, b: softmin_pairs(a, b, h, 1.0), sinkhorn_potentials, sinkhorn_divergence):
        with pytest.raises(ValueError, match="non-empty"):
            fn(np.zeros((6,), np.float32), y)
        with pytest.raises(ValueError, match="non-empty"):
            fn(x, np.zeros((0, 4), np.float32))
        with pytest.raises(ValueError, match="features"):
            fn(x, np.zeros((5, 3), np.float32))
        with pytest.raises(ValueError, match="too large"):
            fn(np.broadcast_to(np.zeros((1, 1), np.float32), (1 << 22, 1 << 9)), np.zeros((5, 1 << 9), np.float32))
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="eps"):
            softmin_pairs(x, y, h, bad)
        for fn in (sinkhorn_potentials, sinkhorn_divergence):
            with pytest.raises(ValueError, match="reg"):
                fn(x, y, reg=bad)
            with pytest.raises(ValueError, match="epsilon"):
                fn(x, y, epsilon=bad)
            with pytest.raises(ValueError, match="schedule"):
                fn(x, y, schedule=[1.0, bad])
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="splits"):
            softmin_pairs(x, y, h, 1.0, splits=bad)
    for bad in (np.zeros(6), np.zeros((5, 1))):
        with pytest.raises(ValueError, match="expected"):
            softmin_pairs(x, y, bad, 1.0)
    for fn in (sinkhorn_potentials, sinkhorn_divergence):
        with pytest.raises(ValueError, match="schedule"):
            fn(x, y, schedule=[])
        with pytest.raises(ValueError, match="schedule"):
            fn(x, y, schedule=3.0)
        with pytest.raises(ValueError, match="schedule"):
            fn(x, y, schedule=[1.0] * 257)
        with pytest.raises(ValueError, match="weights_x has 5 entries"):
            fn(x, y, weights_x=np.full(5, 0.2))
        with pytest.raises(ValueError, match="weights_y has 6 entries"):
            fn(x, y, weights_y=np.full(6, 1 / 6))
        with pytest.raises(ValueError, match="weights_x must be finite and > 0"):
            fn(x, y, weights_x=np.array([0.5, 0.5, 0.0, 0.0, 0.0, 0.0]))
        with pytest.raises(ValueError, match="weights_y must be finite and > 0"):
            fn(x, y, weights_y=np.array([0.5, 0.7, -0.2, 0.0, 0.0]))
        with pytest.raises(ValueError, match="weights_x must sum to 1"):
            fn(x, y, weights_x=np.full(6, 0.2))
    with pytest.raises(ValueError, match="one weight vector"):
        sinkhorn_potentials(x, x, weights_y=np.full(6, 1 / 6))


def test_no_gpu_means_an_engine_error_and_not_a_cpu_result():
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.utils.sinkhorn import sinkhorn_divergence, sinkhorn_potentials, softmin_pairs
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x, y = np.zeros((6, 4), np.float32), np.ones((5, 4), np.float32)
    for call in (lambda: softmin_pairs(x, y, np.zeros(5), 1.0), lambda: sinkhorn_potentials(x, y), lambda: sinkhorn_divergence(x, y)):
        with pytest.raises(_C.FdError):
            call()


def test_metric_class_refuses_bad_arguments_before_the_device():
    from fourierdiffusion_amd.sampling.metrics import SinkhornDivergence
    X = np.zeros((20, 5, 2), np.float32)
    for bad in (0.0, -0.1, np.nan, np.inf, True):
        with pytest.raises(ValueError, match="reg"):
            SinkhornDivergence(X, reg=bad)
    for bad in (1, 7.5):
        with pytest.raises(ValueError, match="max_original"):
            SinkhornDivergence(X, max_original=bad)
    with pytest.raises(ValueError, match="one original"):
        SinkhornDivergence(X[:0])
    with pytest.raises(ValueError, match="one held-out"):
        SinkhornDivergence(X, holdout_samples=X[:0])


# ---------------------------------------------------------------------------------------------- MetricCollection, config
def _reference_engine(monkeypatch, calls):
    """The engine call of the metric class replaced by the float64 reference under the same schedule."""
    from fourierdiffusion_amd.sampling import metrics as M
    from fourierdiffusion_amd.utils.sinkhorn import epsilon_schedule

    def reference(x, y, reg):
        x, y = x.double().numpy(), y.double().numpy()
        calls.append((x.shape, y.shape, reg))
        r = R.divergence(x, y, epsilon_schedule(reg) * R.eps_base(x, y))
        return SimpleNamespace(divergence=r["divergence"], w2=r["w2"], marginal_error=r["marginal_error"])

    monkeypatch.setattr(M, "sinkhorn_divergence", reference)
    monkeypatch.setattr(M, "check_flat_array", lambda x: torch.as_tensor(x).reshape(len(x), -1).float())
    monkeypatch.setattr(M, "dft", lambda x: 2.0 * x)
    return M


def test_metric_collection_keys_with_and_without_a_holdout(monkeypatch):
    calls = []
    M = _reference_engine(monkeypatch, calls)
    rng = np.random.default_rng(1)
    X, Y, H = (torch.from_numpy(W.waves(rng, k, 6).reshape(k, 3, 2)) for k in (10, 5, 6))
    make = partial(M.SinkhornDivergence, reg=0.1, random_seed=4)
    res = M.MetricCollection(metrics=[make], original_samples=X)(Y)
    names = ("sinkhorn_divergence", "sinkhorn_marginal_error", "sinkhorn_w2")
    assert list(res) == sorted(f"{view}_{name}{suffix}" for view in ("time", "freq") for name in names for suffix in ("", "_self"))
    assert all(isinstance(v, float) for v in res.values())
    assert calls[0] == ((5, 6), (10, 6), 0.1) and ((5, 6), (5, 6), 0.1) in calls     # samples first, then the original set; the two folds
    assert res["time_sinkhorn_divergence"] > 0 and res["time_sinkhorn_w2"] == np.sqrt(res["time_sinkhorn_divergence"])
    assert res["freq_sinkhorn_divergence"] == pytest.approx(4.0 * res["time_sinkhorn_divergence"], rel=1e-6)   # the stub view is 2 x
    calls.clear()
    got = M.MetricCollection(metrics=[make], original_samples=X, holdout_samples=H)(Y)
    assert sorted(got) == sorted(list(res) + [f"{view}_{name}_holdout" for view in ("time", "freq") for name in names])
    assert ((5, 6), (6, 6), 0.1) in calls
    assert M.MetricCollection(metrics=[make], original_samples=X, include_baselines=False)(Y).keys() == {
        f"{view}_{name}" for view in ("time", "freq") for name in names}
    assert M.SinkhornDivergence(X).name == "sinkhorn_divergence" and M.SinkhornDivergence(X[:1]).baseline_metrics == {}


def test_max_original_draws_the_seeded_subsample(monkeypatch):
    M = _reference_engine(monkeypatch, [])
    X = torch.arange(40.0).reshape(20, 2)
    metric = M.SinkhornDivergence(X, max_original=8, random_seed=3)
    assert torch.equal(metric.original_samples, X[torch.from_numpy(M.subsample_indices(20, 8, 3))])
    assert M.SinkhornDivergence(X, max_original=20).original_samples.shape[0] == 20


def test_new_config_instantiates_and_default_is_untouched():
    import fdiff.sampling.metrics as alias
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SinkhornDivergence, SlicedWasserstein
    assert alias.SinkhornDivergence is SinkhornDivergence
    conf = os.path.join(ROOT, "cmd", "conf")
    default = compose(conf, "sample", []).metrics
    assert "holdout" not in default and [m["_target_"].rsplit(".", 1)[1] for m in default.metrics] == [
        "SlicedWasserstein", "MarginalWasserstein"]
    cfg = compose(conf, "sample", ["metrics=sinkhorn", "random_seed=7"]).metrics
    assert cfg.holdout is True
    make = instantiate({k: v for k, v in cfg.items() if k != "holdout"})
    assert isinstance(make, partial) and make.func is MetricCollection
    assert make.keywords["include_spectral_density"] is True and make.keywords["include_baselines"] is True
    assert [m.func for m in make.keywords["metrics"]] == [SlicedWasserstein, MarginalWasserstein, SinkhornDivergence]
    assert make.keywords["metrics"][2].keywords == {"reg": 0.05, "random_seed": 7}
    assert [dict(m) for m in cfg.metrics[:2]] == [dict(m) for m in compose(conf, "sample", ["random_seed=7"]).metrics.metrics]
