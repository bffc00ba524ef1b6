"""CPU: the multivariate rank histograms (an extension, not in the reference) -- closed forms and invariances of the float64
restatement in tests/mvrank_ref.py, the experiment the feature rests on (a per-entry rank histogram cannot tell a coherent ensemble
from one permuted independently at every entry; the average-rank, band-depth and minimum-spanning-tree histograms can), every
argument check of the Python layer (raised before the engine is touched: this machine may have no GPU), the C ABI's new symbols
and the new key of cmd/conf/impute.yaml."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import mvrank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_multivariate_ranks_workspace_bytes", "fd_multivariate_ranks")


# ------------------------------------------------------------------------------------------- closed forms
def test_three_points_two_entries_with_a_tie():
    """x_0 = (0, 1), x_1 = (1, 1), x_2 = (2, 0): entry 0 has no tie, entry 1 has the tie 1 = 1.  By hand, m = 3, C(3, 2) = 3:
    average     (1 + 3, 2 + 3, 3 + 1); band depth (2 + 3, 3 + 3, 2 + 2); dominance (1, 2, 1)."""
    S = np.array([[0.0, 1.0], [1.0, 1.0], [2.0, 0.0]])
    assert R.integer_preranks(S, "average").tolist() == [4, 5, 4]
    assert R.integer_preranks(S, "band_depth").tolist() == [5, 6, 4]
    assert R.integer_preranks(S, "dominance").tolist() == [1, 2, 1]
    out = R.multivariate_ranks(S[1:].reshape(1, 2, 2, 1), S[0].reshape(1, 2, 1), np.zeros((2, 1), bool), "average")
    assert out["prerank"].tolist() == [[4.0, 5.0, 4.0]] and out["below"][0] == 0 and out["equal"][0] == 1 and out["hidden"][0] == 2


def test_band_depth_without_ties_is_thorarinsdottirs_form():
    rs = np.random.RandomState(0)
    for m, d in ((2, 1), (5, 3), (20, 7)):
        S = rs.randn(m, d)                                                     # continuous: no tie
        r = (S[:, None, :] > S[None, :, :]).sum(1) + 1                         # r[j, e]: the rank of x_j[e] among the m values
        assert np.array_equal(R.integer_preranks(S, "band_depth"), ((m - r) * (r - 1) + (m - 1)).sum(1))
        assert np.array_equal(R.integer_preranks(S, "average"), r.sum(1))     # and the average rank is the rank sum


def test_dominance_of_a_componentwise_largest_point_is_m():
    rs = np.random.RandomState(1)
    S = rs.randn(9, 5)
    S[4] = S.max(axis=0)                                                       # ties with the largest value of every entry
    G = R.integer_preranks(S, "dominance")
    assert G[4] == 9 and (G >= 1).all()
    S[2] = S.min(axis=0) - 1.0
    assert R.integer_preranks(S, "dominance")[2] == 1


def test_mst_of_collinear_points():
    """Points p_i u on a line: the tree of any subset is the chain, its length (max - min) |u|."""
    p = np.array([0.0, 3.0, 1.0, 7.0, 4.5])
    u = np.array([3.0, 4.0])                                                   # |u| = 5
    L, edge = R.mst_preranks(p[:, None] * u[None])
    expect = [5.0 * (np.delete(p, j).max() - np.delete(p, j).min()) for j in range(5)]
    np.testing.assert_allclose(L, expect, rtol=1e-14)
    assert abs(edge - 35.0) <= 1e-13
    assert R.mst_preranks(p[:2, None] * u[None])[0].tolist() == [0.0, 0.0]     # one point left: no edge
    Lc, _ = R.mst_preranks(p[:, None] * u[None], candidates=[0, 3])
    assert Lc[0] == L[0] and Lc[3] == L[3] and np.isnan(Lc[[1, 2, 4]]).all()


def test_integer_kinds_are_invariant_under_a_positive_scale_per_entry():
    rs = np.random.RandomState(2)
    S = np.round(rs.randn(12, 6) * 2) / 2                                      # a coarse grid: ties
    scale = np.array([0.25, 8.0, 1.0, 3.0, 0.5, 1024.0])                       # exact in binary or not: the order is kept
    for kind in ("average", "band_depth", "dominance"):
        assert np.array_equal(R.integer_preranks(S, kind), R.integer_preranks(S * scale, kind)), kind
    assert not np.allclose(R.mst_preranks(S)[0], R.mst_preranks(S * scale)[0])


def test_edge_series_of_the_restatement():
    rs = np.random.RandomState(3)
    x, y = rs.randn(3, 4, 5, 2).astype(np.float32), rs.randn(3, 5, 2).astype(np.float32)
    mask = rs.rand(3, 5, 2) < 0.4
    mask[1] = True                                                             # series 1: nothing hidden
    mask[2, 0, 0] = False
    x[2, 1, 0, 0] = np.nan                                                     # series 2: a NaN at a hidden entry
    x[0][:, mask[0]] = np.nan                                                  # series 0: NaN at observed entries only
    for kind in R.KINDS:
        out = R.multivariate_ranks(x, y, mask, kind)
        assert out["below"][1] == 0 and out["equal"][1] == 4 and out["hidden"][1] == 0
        assert out["below"][2] == -1 and out["equal"][2] == -1
        assert np.isnan(out["prerank"][2]).all() if kind == "mst" else (out["prerank"][2] == -1).all()
        assert out["below"][0] >= 0 and np.isfinite(out["prerank"][0]).all()
    hist = R.rank_histogram(np.array([2, 0, 4]), np.array([0, 4, 0]), np.array([3, 0, 1]), 4)
    np.testing.assert_allclose(hist, [0, 0, 0.5, 0, 0.5])
    assert np.isnan(R.rank_histogram(np.array([2, -1]), np.array([0, -1]), np.array([3, 1]), 4)).all()


# ------------------------------------------------------------------------------------------- why the feature exists
@pytest.fixture(scope="module")
def experiment():
    truth, x, shuffled = R.coherent_and_shuffled()                             # n = 400, K = 19, T = 12, C = 2
    mask = np.zeros(truth.shape[1:], bool)
    return truth, x, shuffled, mask


def test_per_entry_histogram_is_blind_to_the_shuffle(experiment):
    truth, x, shuffled, _ = experiment
    a, b = R.entry_rank_histogram(x, truth, 19), R.entry_rank_histogram(shuffled, truth, 19)
    assert np.array_equal(a, b)
    assert R.reliability_index(a) < 0.05


@pytest.mark.parametrize("kind", ["average", "band_depth", "mst"])
def test_multivariate_histograms_see_the_shuffle(experiment, kind):
    """Reliability index of the shuffled set at least 3x the coherent one's (float64 data: 8.5x, 11x and 7.8x)."""
    truth, x, shuffled, mask = experiment
    ri, gaps = [], []
    for v in (x, shuffled):
        out = R.multivariate_ranks(v, truth, mask, kind)
        ri.append(R.reliability_index(R.rank_histogram(out["below"], out["equal"], out["hidden"], 19)))
        gaps.append(R.mst_relative_gaps(out["prerank"]).min() if kind == "mst" else None)
    print(f"[mvrank] {kind}: reliability index coherent {ri[0]:.3f}, shuffled {ri[1]:.3f}; smallest relative mst gaps {gaps}")
    assert ri[1] >= 3.0 * ri[0], (kind, ri)
    if kind == "mst":                                                          # no rank rests on a gap that rounding could close
        assert min(gaps) > 1e-9, gaps


# ------------------------------------------------------------------------------------------- Python layer
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
    assert F.PRERANKS == ("average", "band_depth", "dominance", "mst")
    calls = {
        "counts": lambda **k: F.multivariate_rank_counts(k.pop("x", x), k.pop("y", y), k.pop("m", m), k.pop("kind", "average"), **k),
        "histogram": lambda **k: F.multivariate_rank_histogram(k.pop("x", x), k.pop("y", y), k.pop("m", m),
                                                               [k.pop("kind", "average")], **k),
    }
    for call in calls.values():
        for bad in (dict(kind="median"), dict(kind=None), dict(kind=0),
                    dict(m=m.float()), dict(m=None), dict(m=torch.zeros(5, 4, dtype=torch.bool)),
                    dict(m=torch.zeros(3, 5, 3, dtype=torch.bool)),
                    dict(x=torch.zeros(2, 4, 5)), dict(y=torch.zeros(2, 5)), dict(y=torch.zeros(3, 5, 3)), dict(y=torch.zeros(2, 6, 3)),
                    dict(x=torch.zeros(2, 0, 5, 3)), dict(x=torch.zeros(2, 1024, 5, 3)), dict(x=torch.zeros(2, 1025, 5, 3)),
                    dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=torch.ones(4))):
            with pytest.raises(ValueError):
                call(**bad)
    for bad in ("average", [], ()):
        with pytest.raises(ValueError):
            F.multivariate_rank_histogram(x, y, m, bad)


def test_good_arguments_reach_the_engine(monkeypatch):
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling import forecast as F

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(_C, "ctx", reached)
    x, y, m = _args()
    for call in (lambda: F.multivariate_rank_counts(x, y, m, "mst", scale=torch.tensor([1.0, 2.0, 0.5]), device="cuda:0"),
                 lambda: F.multivariate_rank_counts(torch.zeros(2, 1023, 5, 3), y, torch.zeros(2, 5, 3, dtype=torch.bool), "dominance",
                                                    device="cuda:0"),
                 lambda: F.multivariate_rank_histogram(x[:, :1], y, m, device="cuda:0"),
                 lambda: F.multivariate_rank_histogram(x, y, m, F.PRERANKS, scale=2.0, device="cuda:0")):
        with pytest.raises(Reached):
            call()


def test_histogram_of_per_series_counts_matches_the_restatement():
    from fourierdiffusion_amd.sampling.forecast import rank_histogram, reliability_index
    rs = np.random.RandomState(5)
    K = 6
    below = rs.randint(0, K + 1, 40)
    equal = np.array([rs.randint(0, K - b + 1) for b in below])
    hidden = rs.randint(0, 3, 40)
    ref = R.rank_histogram(below, equal, hidden, K)
    got = rank_histogram(torch.from_numpy(below).int(), torch.from_numpy(equal).int(), torch.from_numpy(hidden == 0), K)
    np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-14)
    assert abs(reliability_index(got) - R.reliability_index(ref)) <= 1e-13


# ------------------------------------------------------------------------------------------- C ABI, config, CLI
def test_library_exports_and_binds_the_new_symbols():
    from fourierdiffusion_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in _C.EXPORTED_SYMBOLS, sym
    assert (_C.FD_PRERANK_AVERAGE, _C.FD_PRERANK_BAND_DEPTH, _C.FD_PRERANK_DOMINANCE, _C.FD_PRERANK_MST) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "fdiff_hip.h")).read()
    assert "FD_PRERANK_AVERAGE = 0, FD_PRERANK_BAND_DEPTH = 1, FD_PRERANK_DOMINANCE = 2, FD_PRERANK_MST = 3" in header


def test_impute_config_default_and_override(tmp_path):
    from fourierdiffusion_amd.config import compose
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "impute", [], cwd=str(tmp_path))
    assert list(cfg.multivariate_ranks) == []
    cfg = compose(conf, "impute", ["multivariate_ranks=[average,mst]"], cwd=str(tmp_path))
    assert list(cfg.multivariate_ranks) == ["average", "mst"]


def test_multivariate_rank_results_needs_an_ensemble():
    spec = importlib.util.spec_from_file_location("cmd_impute_for_mvrank", os.path.join(ROOT, "cmd", "impute.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    truth, mask = torch.zeros(3, 6, 2), torch.zeros(3, 6, 2, dtype=torch.bool)
    with pytest.raises(ValueError, match="num_samples_per_series"):
        mod.multivariate_rank_results(torch.zeros(3, 1, 6, 2), truth, mask, ["average"])
    with pytest.raises(ValueError, match="num_samples_per_series"):
        mod.multivariate_rank_results(torch.zeros(3, 6, 2), truth, mask, ["average"])
