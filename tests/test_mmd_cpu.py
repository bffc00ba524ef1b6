"""CPU: the kernel two-sample test (an extension, not in the reference) -- the float64 host arithmetic of utils/two_sample.py equals
the direct three-sum definition of tests/mmd_ref.py, the p-value rule and the permutation rule are what the contract says, every
argument check fires before anything touches a device, and the new entry points, config and result keys exist."""
import ctypes
import os
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mmd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_kernel_quadforms_workspace_bytes", "fd_kernel_quadforms"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


# ---------------------------------------------------------------------------------------------- host arithmetic
@pytest.mark.parametrize("n,m,P", [(7, 9, 12), (2, 30, 5), (25, 2, 5), (1, 12, 3)])
def test_host_arithmetic_is_the_three_sum_definition(n, m, P):
    from fourierdiffusion_amd.utils import two_sample as T
    rng = np.random.default_rng(n * 100 + m)
    z = np.concatenate([R.waves(rng, n, 11), 1.3 * R.waves(rng, m, 11)])
    D = R.dist2(z, z)
    K = R.kernel_matrix(D, R.DEFAULT_SCALES, R.pooled_base2(D))
    A = R.permutation_members(n, m, P - 1, seed=3)
    quad, rowsum, col0 = R.quadforms(K, A)
    direct = R.mmd2_direct(K, A)
    np.testing.assert_allclose(T.mmd2_from_quadforms(quad, rowsum, A), direct, rtol=0, atol=1e-13)
    np.testing.assert_allclose(R.mmd2_from_sums(quad, rowsum, A), direct, rtol=0, atol=1e-13)
    np.testing.assert_allclose(T.witness_from_quadforms(rowsum, col0, A[:, 0]), R.witness(K, A[:, 0]), rtol=0, atol=1e-13)
    assert T.permutation_p_value(direct) == R.p_value(direct)


def test_pooled_bandwidth_closed_form():
    rng = np.random.default_rng(5)
    z = R.waves(rng, 40, 13) + 2.0
    closed = 2.0 * ((z - z.mean(axis=0)) ** 2).sum() / (len(z) - 1)
    assert R.pooled_base2(R.dist2(z, z)) == pytest.approx(closed, rel=1e-12)


def test_p_value_rule_counts_ties_and_the_observed_split():
    from fourierdiffusion_amd.utils.two_sample import permutation_p_value
    assert permutation_p_value([0.5, 0.1, 0.2, 0.3]) == 1 / 4
    assert permutation_p_value([0.2, 0.1, 0.2, 0.3]) == 3 / 4          # a tie counts as "at least as large"
    assert permutation_p_value([0.0, 0.1, 0.2, 0.3]) == 1.0
    assert permutation_p_value([0.3]) == 1.0                            # no permutation: nothing can be said
    assert permutation_p_value([-0.1, -0.2, -0.1]) == 2 / 3


def test_permutation_members_rule():
    from fourierdiffusion_amd.utils.two_sample import permutation_members
    A = permutation_members(7, 12, 30, seed=11)
    assert A.dtype == np.uint8 and A.shape == (19, 31) and set(np.unique(A)) == {0, 1}
    assert (A.sum(axis=0) == 7).all()
    np.testing.assert_array_equal(A[:, 0], [1] * 7 + [0] * 12)
    np.testing.assert_array_equal(A, permutation_members(7, 12, 30, seed=11))
    np.testing.assert_array_equal(A, R.permutation_members(7, 12, 30, 11))
    assert (A != permutation_members(7, 12, 30, seed=12)).any()
    rng = np.random.default_rng(11)                                     # one generator, the permutations drawn in order
    for p in (1, 2, 3):
        np.testing.assert_array_equal(np.flatnonzero(A[:, p]), np.sort(rng.permutation(19)[:7]))
    np.testing.assert_array_equal(permutation_members(3, 4, 0, seed=0), [[1]] * 3 + [[0]] * 4)


# ---------------------------------------------------------------------------------------------- argument checks
def test_two_sample_functions_refuse_bad_arguments_before_the_device():
    from fourierdiffusion_amd.utils.two_sample import kernel_quadforms, mmd_permutation_test, permutation_members
    z, A = np.zeros((6, 4), np.float32), np.zeros((6, 3), np.uint8)
    with pytest.raises(ValueError, match="non-empty"):
        kernel_quadforms(np.zeros((6,), np.float32), A)
    with pytest.raises(ValueError, match="at least two"):
        kernel_quadforms(z[:1], A[:1])
    with pytest.raises(ValueError, match="expected"):
        kernel_quadforms(z, A[:5])
    with pytest.raises(ValueError, match="expected"):
        kernel_quadforms(z, A[:, 0])
    with pytest.raises(ValueError, match="columns"):
        kernel_quadforms(z, np.zeros((6, 0), np.uint8))
    with pytest.raises(ValueError, match="columns"):
        kernel_quadforms(z, np.zeros((6, 1025), np.uint8))
    with pytest.raises(ValueError, match="uint8 or bool"):
        kernel_quadforms(z, A.astype(np.float32))
    with pytest.raises(ValueError, match="uint8 or bool"):
        kernel_quadforms(z, torch.zeros(6, 3))
    with pytest.raises(ValueError, match="numpy array or a torch tensor"):
        kernel_quadforms(z, [[1, 0, 1]] * 6)
    for bad in ((), (1.0,) * 9, (1.0, 0.0), (1.0, -2.0), (np.nan,), (np.inf,)):
        with pytest.raises(ValueError, match="scales"):
            kernel_quadforms(z, A, scales=bad)
    with pytest.raises(ValueError, match="scales"):
        kernel_quadforms(z, A, scales=3.0)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="bandwidth2"):
            kernel_quadforms(z, A, bandwidth2=bad)
        with pytest.raises(ValueError, match="bandwidth2"):
            mmd_permutation_test(z, z, bandwidth2=bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="col_splits"):
            kernel_quadforms(z, A, col_splits=bad)
    with pytest.raises(ValueError, match="too large"):
        kernel_quadforms(np.broadcast_to(np.zeros((1, 1), np.float32), (1 << 22, 1 << 9)), np.broadcast_to(A[:1, :1], (1 << 22, 1)))
    with pytest.raises(ValueError, match="features"):
        mmd_permutation_test(z, np.zeros((6, 5), np.float32))
    with pytest.raises(ValueError, match="at least two rows"):
        mmd_permutation_test(z[:1], z)
    with pytest.raises(ValueError, match="at least two rows"):
        mmd_permutation_test(z, z[:1])
    for bad in (-1, 2.5, 1024):
        with pytest.raises(ValueError, match="n_permutations"):
            mmd_permutation_test(z, z, n_permutations=bad)
    with pytest.raises(ValueError, match="scales"):
        mmd_permutation_test(z, z, scales=(0.0,))
    with pytest.raises(ValueError, match="n=0"):
        permutation_members(0, 5, 3, 0)
    with pytest.raises(ValueError, match="m=0"):
        permutation_members(5, 0, 3, 0)


def test_host_arithmetic_refuses_an_empty_group():
    from fourierdiffusion_amd.utils.two_sample import mmd2_from_quadforms
    with pytest.raises(ValueError, match="each group"):
        mmd2_from_quadforms(np.zeros(2), np.zeros(4), np.array([[1, 1], [1, 0], [1, 0], [1, 1]], np.uint8))


def test_metric_class_refuses_bad_arguments_before_the_device():
    from fourierdiffusion_amd.sampling.metrics import KernelTwoSample
    X = np.zeros((20, 5, 2), np.float32)
    for bad in (0, 1024, 2.5, True):
        with pytest.raises(ValueError, match="n_permutations"):
            KernelTwoSample(X, n_permutations=bad)
    for bad in (1, 7.5):
        with pytest.raises(ValueError, match="max_original"):
            KernelTwoSample(X, max_original=bad)
    with pytest.raises(ValueError, match="two original"):
        KernelTwoSample(X[:1])
    with pytest.raises(ValueError, match="two held-out"):
        KernelTwoSample(X, holdout_samples=X[:1])
    with pytest.raises(ValueError, match="scales"):
        KernelTwoSample(X, scales=(1.0, -1.0))


# ---------------------------------------------------------------------------------------------- MetricCollection, config
def _stub_engine(monkeypatch, calls):
    from fourierdiffusion_amd.sampling import metrics as M

    def fake_test(x, y, n_permutations, scales, seed):
        calls.append((tuple(x.shape), tuple(y.shape), n_permutations, tuple(scales), seed))
        return SimpleNamespace(mmd2=float(len(calls)), p_value=1.0 / (1 + n_permutations))

    monkeypatch.setattr(M, "mmd_permutation_test", fake_test)
    monkeypatch.setattr(M, "check_flat_array", lambda x: torch.as_tensor(x).reshape(len(x), -1).float())
    monkeypatch.setattr(M, "dft", lambda x: 2.0 * x)
    return M


def test_metric_collection_keys_with_and_without_a_holdout(monkeypatch):
    calls = []
    M = _stub_engine(monkeypatch, calls)
    X, Y, H = torch.randn(10, 3, 2), torch.randn(5, 3, 2), torch.randn(6, 3, 2)
    make = partial(M.KernelTwoSample, n_permutations=19, random_seed=4)
    plain = M.MetricCollection(metrics=[make], original_samples=X)
    res = plain(Y)
    assert list(res) == ["freq_mmd2", "freq_mmd2_self", "freq_mmd_p_value", "freq_mmd_p_value_self",
                         "time_mmd2", "time_mmd2_self", "time_mmd_p_value", "time_mmd_p_value_self"]
    assert all(isinstance(v, float) for v in res.values()) and res["time_mmd_p_value"] == 1 / 20
    assert calls[0] == ((5, 6), (10, 6), 19, R.DEFAULT_SCALES, 4)                     # samples first, then the original set
    assert ((5, 6), (5, 6), 19, R.DEFAULT_SCALES, 4) in calls                          # the two folds
    calls.clear()
    held = M.MetricCollection(metrics=[make], original_samples=X, holdout_samples=H)
    got = held(Y)
    assert sorted(got) == sorted(list(res) + ["freq_mmd2_holdout", "freq_mmd_p_value_holdout", "time_mmd2_holdout",
                                              "time_mmd_p_value_holdout"])
    assert ((5, 6), (6, 6), 19, R.DEFAULT_SCALES, 4) in calls
    assert M.MetricCollection(metrics=[make], original_samples=X, include_baselines=False)(Y).keys() == {
        "freq_mmd2", "freq_mmd_p_value", "time_mmd2", "time_mmd_p_value"}


def test_max_original_draws_the_seeded_subsample(monkeypatch):
    calls = []
    M = _stub_engine(monkeypatch, calls)
    X = torch.arange(40.0).reshape(20, 2)
    metric = M.KernelTwoSample(X, max_original=8, random_seed=3)
    assert torch.equal(metric.original_samples, X[torch.from_numpy(M.subsample_indices(20, 8, 3))])
    assert M.KernelTwoSample(X, max_original=20).original_samples.shape[0] == 20
    assert metric.name == "kernel_two_sample"


def test_new_config_instantiates_and_default_is_untouched():
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.metrics import KernelTwoSample, MarginalWasserstein, MetricCollection, SlicedWasserstein
    conf = os.path.join(ROOT, "cmd", "conf")
    default = compose(conf, "sample", []).metrics
    assert "holdout" not in default and [m["_target_"].rsplit(".", 1)[1] for m in default.metrics] == [
        "SlicedWasserstein", "MarginalWasserstein"]
    cfg = compose(conf, "sample", ["metrics=two_sample", "random_seed=7"]).metrics
    assert cfg.holdout is True
    make = instantiate({k: v for k, v in cfg.items() if k != "holdout"})
    assert isinstance(make, partial) and make.func is MetricCollection
    assert make.keywords["include_spectral_density"] is True and make.keywords["include_baselines"] is True
    assert [m.func for m in make.keywords["metrics"]] == [SlicedWasserstein, MarginalWasserstein, KernelTwoSample]
    assert make.keywords["metrics"][2].keywords == {"n_permutations": 200, "random_seed": 7}
    assert [dict(m) for m in cfg.metrics[:2]] == [dict(m) for m in compose(conf, "sample", ["random_seed=7"]).metrics.metrics]
