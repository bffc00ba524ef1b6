"""CPU: the multivariate ensemble scores (an extension, not in the reference) -- identities of the float64 restatement in
tests/multivariate_ref.py, the experiment the feature rests on (per-entry CRPS cannot tell a coherent ensemble from one permuted
independently at every entry, the variogram score can), rank_histogram / reliability_index against the restatement, every argument
check of sampling/forecast.py (all raised before the engine is touched: this machine may have no GPU), the C ABI's new symbols and
the new keys of cmd/conf/impute.yaml."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import ensemble_ref as E
from tests import multivariate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_energy_score_workspace_bytes", "fd_energy_score", "fd_variogram_score_workspace_bytes", "fd_variogram_score",
               "fd_ensemble_ranks")


def _case(n=3, K=7, T=6, Cn=3, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, K, T, Cn) * 1.5 + 0.3
    y = rs.randn(n, T, Cn)
    m = rs.rand(n, T, Cn) < 0.4
    m[:, 0, 0] = False
    m[:, T - 1, Cn - 1] = False
    return x, y, m


# ------------------------------------------------------------------------------------------- identities of the restatement
def test_energy_with_one_entry_is_the_crps():
    rs = np.random.RandomState(1)
    for K in (1, 2, 9):
        x, y = rs.randn(K), rs.randn()
        assert abs(R.energy_series(x[:, None], np.array([y])) - E.crps_pairwise(x, y)) <= 1e-14


def test_energy_with_one_member_is_the_distance():
    rs = np.random.RandomState(2)
    x, y = rs.randn(1, 11), rs.randn(11)
    assert abs(R.energy_series(x, y) - np.linalg.norm(x[0] - y)) <= 1e-14


@pytest.mark.parametrize("fair", [False, True])
def test_energy_is_homogeneous_and_shift_invariant(fair):
    x, y, m = _case()
    base, hid = R.energy_score(x, y, m, fair)
    assert np.array_equal(hid, (~m).reshape(3, -1).sum(1)) and np.isfinite(base).all()
    for a in (-2.5, 0.125):
        np.testing.assert_allclose(R.energy_score(a * x, a * y, m, fair)[0], abs(a) * base, rtol=1e-13)
    shift = np.random.RandomState(3).randn(1, 6, 3)
    np.testing.assert_allclose(R.energy_score(x + shift[:, None], y + shift, m, fair)[0], base, rtol=1e-12)
    # the fair form differs from the plain one by the factor K / (K - 1) on the spread term
    plain = R.energy_score(x, y, m, False)[0]
    K = x.shape[1]
    t1 = np.array([np.mean([np.linalg.norm((x[s, k] - y[s])[~m[s]]) for k in range(K)]) for s in range(3)])
    np.testing.assert_allclose(t1 - R.energy_score(x, y, m, True)[0], (t1 - plain) * K / (K - 1), rtol=1e-12)


@pytest.mark.parametrize("order", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("weights", ["inverse_lag", "uniform"])
def test_variogram_shift_invariances(order, weights):
    x, y, m = _case(seed=4)
    num, den = R.variogram_score(x, y, m, order, 2, weights)
    assert (den > 0).all() and np.isfinite(num).all()
    n2, d2 = R.variogram_score(x - 3.5, y - 3.5, m, order, 2, weights)                   # a shift common to samples and truth
    np.testing.assert_allclose(n2, num, rtol=1e-10)
    assert np.array_equal(d2, den)
    n3, _ = R.variogram_score(x + 7.25, y, m, order, 2, weights)                          # one constant on every member entry
    np.testing.assert_allclose(n3, num, rtol=1e-10)


def test_variogram_pairs_and_weights_by_hand():
    """T = 3, C = 2, all hidden: 15 pairs; lag 0 pairs 3, lag 1 pairs 8, lag 2 pairs 4."""
    x, y = np.zeros((1, 1, 3, 2)), np.zeros((1, 3, 2))
    m = np.zeros((3, 2), bool)
    for lag, pairs, wsum in ((None, 15, 3 + 8 / 2 + 4 / 3), (0, 3, 3.0), (1, 11, 3 + 8 / 2), (2, 15, 3 + 8 / 2 + 4 / 3)):
        assert R.variogram_score(x, y, m, 1.0, lag, "uniform")[1][0] == pairs
        assert abs(R.variogram_score(x, y, m, 1.0, lag, "inverse_lag")[1][0] - wsum) <= 1e-14
    m1 = np.ones((3, 2), bool)
    m1[1, 0] = False                                                                       # one hidden entry: no pair
    num, den = R.variogram_score(x, y, m1, 1.0, None, "uniform")
    assert np.isnan(num[0]) and den[0] == 0


# ------------------------------------------------------------------------------------------- why the feature exists
def test_marginal_scores_miss_a_shuffled_ensemble_and_the_variogram_score_does_not():
    """Truth and a K = 32 ensemble from one AR(1) law (rho = 0.95); the members permuted independently at every entry keep every
    marginal.  The per-entry CRPS moves by rounding only; the lag-limited variogram score rises by >= 1.25 (measured 1.45 to 1.53
    over three seeds); the energy score rises too."""
    n, K, T, Cn = 8, 32, 24, 3
    truth, x, shuffled = R.ar1_ensemble(n, K, T, Cn, 0.95, seed=0)
    mask = np.zeros((T, Cn), bool)
    mask[:2] = True
    xe, se = np.moveaxis(x, 1, -1), np.moveaxis(shuffled, 1, -1)
    crps_gap = np.abs(E.crps_sorted(xe, truth) - E.crps_sorted(se, truth)).max()
    assert crps_gap <= 1e-6, crps_gap
    vs = [np.mean(np.divide(*R.variogram_score(v, truth, mask, 0.5, 2, "uniform"))) for v in (x, shuffled)]
    assert vs[1] >= 1.25 * vs[0], vs
    es = [R.energy_score(v, truth, mask)[0].mean() for v in (x, shuffled)]
    assert es[1] > es[0], es


# ------------------------------------------------------------------------------------------- rank histogram
def test_rank_histogram_and_reliability_index_match_the_restatement():
    from fourierdiffusion_amd.sampling.forecast import rank_histogram, reliability_index
    rs = np.random.RandomState(6)
    for K in (1, 5, 16):
        x = np.round(rs.randn(4, K, 5, 3) * 2) / 2                                        # a coarse grid: many ties
        y = np.round(rs.randn(4, 5, 3) * 2) / 2
        x[0, :, 0, 0] = y[0, 0, 0]                                                         # a constant ensemble equal to the truth
        m = rs.rand(4, 5, 3) < 0.3
        m[0, 0, 0] = False
        below, equal = R.rank_counts(x, y)
        assert (equal > 0).any() and equal[0, 0, 0] == K and below[0, 0, 0] == 0
        ref = R.rank_histogram(below, equal, m, K)
        got = rank_histogram(torch.from_numpy(below).int(), torch.from_numpy(equal).int(), torch.from_numpy(m), K)
        assert got.dtype == torch.float64 and tuple(got.shape) == (K + 1,)
        np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-14)
        assert abs(float(got.sum()) - 1.0) <= 1e-13
        assert abs(reliability_index(got) - R.reliability_index(ref)) <= 1e-13
    flat = torch.full((9,), 1.0 / 9, dtype=torch.float64)
    assert reliability_index(flat) <= 1e-15
    spike = torch.zeros(9, dtype=torch.float64)
    spike[0] = 1.0
    assert abs(reliability_index(spike) - 2.0 * 8 / 9) <= 1e-15


def test_rank_histogram_shared_mask_nan_entries_and_errors():
    from fourierdiffusion_amd.sampling.forecast import rank_histogram
    below = torch.tensor([[[0, 2], [1, 3]]], dtype=torch.int32)
    equal = torch.tensor([[[0, 1], [2, 0]]], dtype=torch.int32)
    shared = torch.tensor([[False, True], [False, False]])
    got = rank_histogram(below, equal, shared, 3)                                          # entries (0; 1 +2 ties; 3)
    np.testing.assert_allclose(got.numpy(), np.array([1.0, 1 / 3, 1 / 3, 1 / 3 + 1.0]) / 3, atol=1e-15)
    bad = below.clone()
    bad[0, 0, 0] = -1
    assert torch.isnan(rank_histogram(bad, equal, shared, 3)).all()                        # a NaN entry is not dropped silently
    assert torch.isnan(rank_histogram(below, equal, torch.ones(2, 2, dtype=torch.bool), 3)).all()
    with pytest.raises(ValueError):
        rank_histogram(below, equal, shared, 2)                                            # below + equal > K
    with pytest.raises(ValueError):
        rank_histogram(below, equal, shared.int(), 3)
    with pytest.raises(ValueError):
        rank_histogram(below, equal, shared, 0)


# ------------------------------------------------------------------------------------------- argument checks
def _args(n=2, K=4, T=5, Cn=3):
    return torch.zeros(n, K, T, Cn), torch.zeros(n, T, Cn), torch.zeros(T, Cn, dtype=torch.bool)


def test_argument_errors_are_raised_before_the_engine_is_touched(monkeypatch):
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling import forecast as F

    def no_engine(*a, **k):
        raise AssertionError("an argument check let a bad call through to the engine")
    monkeypatch.setattr(_C, "ctx", no_engine)
    monkeypatch.setattr(_C, "lib", no_engine)
    x, y, m = _args()
    calls = {
        "energy": lambda **k: F.energy_score(k.pop("x", x), k.pop("y", y), k.pop("m", m), **k),
        "variogram": lambda **k: F.variogram_score(k.pop("x", x), k.pop("y", y), k.pop("m", m), **k),
        "all": lambda **k: F.multivariate_scores(k.pop("x", x), k.pop("y", y), k.pop("m", m), **k),
    }
    for name, call in calls.items():
        for bad in (dict(m=m.float()), dict(m=m.to(torch.uint8)), dict(m=None),                       # mask dtype
                    dict(m=torch.zeros(5, 4, dtype=torch.bool)), dict(m=torch.zeros(3, 5, 3, dtype=torch.bool)),   # mask shape
                    dict(x=torch.zeros(2, 4, 5)), dict(y=torch.zeros(2, 5)), dict(y=torch.zeros(3, 5, 3)),
                    dict(y=torch.zeros(2, 6, 3)),                                                       # shapes
                    dict(x=torch.zeros(2, 0, 5, 3)), dict(x=torch.zeros(2, 1025, 5, 3)),               # K out of range
                    dict(scale=0.0), dict(scale=-1.0), dict(scale=torch.tensor([1.0, 0.0, 2.0])),
                    dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=torch.ones(4))):   # scale
            with pytest.raises(ValueError):
                call(**bad)
    for name in ("variogram", "all"):
        for bad in (dict(order=0.75), dict(order=3), dict(order="half"), dict(order=None), dict(weights="lag"),
                    dict(weights=None), dict(max_lag=-1), dict(max_lag=1.5)):
            with pytest.raises(ValueError):
                calls[name](**bad)
    x1 = torch.zeros(2, 1, 5, 3)
    for name in ("energy", "all"):
        with pytest.raises(ValueError, match="fair"):
            calls[name](x=x1, fair=True)
    for bad in (dict(x=torch.zeros(2, 4, 5)), dict(y=torch.zeros(2, 6, 3)), dict(x=torch.zeros(2, 0, 5, 3)),
                dict(x=torch.zeros(2, 1025, 5, 3))):
        with pytest.raises(ValueError):
            F.rank_counts(bad.get("x", x), bad.get("y", y))


def test_good_arguments_reach_the_engine(monkeypatch):
    """The counterpart of the test above: the same calls with good arguments get as far as asking for a context."""
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling import forecast as F

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(_C, "ctx", reached)
    x, y, m = _args()
    d = "cuda:0"
    for call in (lambda: F.energy_score(x, y, m, fair=True, scale=torch.tensor([1.0, 2.0, 0.5]), device=d),
                 lambda: F.variogram_score(x, y, m, order=2, max_lag=0, weights="uniform", scale=2.0, device=d),
                 lambda: F.variogram_score(x, y, torch.zeros(2, 5, 3, dtype=torch.bool), order=1, device=d),
                 lambda: F.rank_counts(x, y, device=d),
                 lambda: F.multivariate_scores(x[:, :1], y, m, scale=torch.ones(5, 3), device=d)):
        with pytest.raises(Reached):
            call()


# ------------------------------------------------------------------------------------------- C ABI, config, CLI
def test_library_exports_and_binds_the_new_symbols():
    from fourierdiffusion_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in _C.EXPORTED_SYMBOLS, sym
    assert (_C.FD_VARIOGRAM_HALF, _C.FD_VARIOGRAM_ONE, _C.FD_VARIOGRAM_TWO) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "fdiff_hip.h")).read()
    assert "FD_VARIOGRAM_HALF = 0, FD_VARIOGRAM_ONE = 1, FD_VARIOGRAM_TWO = 2" in header


def test_impute_config_composes_with_the_flag_off(tmp_path):
    from fourierdiffusion_amd.config import compose
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "impute", [], cwd=str(tmp_path))
    assert cfg.multivariate_scores is False
    assert dict(cfg.variogram) == {"order": 0.5, "max_lag": None, "weights": "inverse_lag"}
    cfg = compose(conf, "impute", ["multivariate_scores=true", "variogram.order=2", "variogram.max_lag=3",
                                   "variogram.weights=uniform"], cwd=str(tmp_path))
    assert cfg.multivariate_scores is True
    assert dict(cfg.variogram) == {"order": 2, "max_lag": 3, "weights": "uniform"}


def _impute_module():
    spec = importlib.util.spec_from_file_location("cmd_impute_for_multivariate", os.path.join(ROOT, "cmd", "impute.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_multivariate_results_needs_an_ensemble():
    mod = _impute_module()
    truth, mask = torch.zeros(3, 6, 2), torch.zeros(3, 6, 2, dtype=torch.bool)
    with pytest.raises(ValueError, match="num_samples_per_series"):
        mod.multivariate_results(torch.zeros(3, 1, 6, 2), truth, mask, {})
    with pytest.raises(ValueError, match="num_samples_per_series"):
        mod.multivariate_results(torch.zeros(3, 6, 2), truth, mask, {})                    # the K = 1 run's (n, T, C) result
