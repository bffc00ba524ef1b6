"""CPU: the float64 signature reference against itself (tests/signature_ref.py: the Horner form against the tensor-algebra product,
closed forms, the shuffle identity), the host side of utils/signature.py (dimensions, every ValueError, the distance arithmetic against
a brute-force Gram matrix) and the `metrics=signature` config.  The engine is never called: there is no CPU fallback to call."""
from __future__ import annotations

import math
import os
from functools import partial

import numpy as np
import pytest
import torch

from tests import signature_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, T, C, depth, flags): the shapes of tests/test_gpu_signature.py
CASES = {
    "lower_ends": (1, 2, 1, 1, 0),
    "depth_limit": (3, 5, 1, 6, R.TIME),
    "ecg": (7, 187, 1, 4, R.TIME | R.BASEPOINT),
    "mimic": (5, 24, 40, 2, R.TIME),
    "feature_cap": (2, 6, 64, 2, R.TIME),
    "lead_lag": (4, 16, 3, 3, R.LEAD_LAG | R.TIME),
    "T_limit": (2, 1024, 2, 3, 0),
    "chunk_boundaries": (3 * R.CHUNK_SERIES + 1, 9, 2, 3, R.TIME),
    "odd": (65, 9, 5, 3, R.BASEPOINT),
}
DIMS = {"lower_ends": 1, "depth_limit": 126, "ecg": 30, "mimic": 1722, "feature_cap": 4290, "lead_lag": 399, "T_limit": 14,
        "chunk_boundaries": 39, "odd": 155}


def make_series(name):
    n, T, C, depth, flags = CASES[name]
    rs = np.random.RandomState(len(name) * 100 + n + T + C)
    return np.cumsum(rs.standard_normal((n, T, C)), axis=1).astype(np.float32)


def channel_maps(name):
    """(offset, scale) of a case: two cases have non-trivial ones, one of them with a zero scale."""
    C = CASES[name][2]
    if name == "mimic":
        rs = np.random.RandomState(40)
        scale = np.exp(rs.uniform(-1, 1, size=C))
        scale[7] = 0.0
        return rs.standard_normal(C), scale
    if name == "odd":
        return np.array([0.5, -1.25, 3.0, 0.0, 100.0]), np.array([2.0, 0.3, 1.0, 1.7, 0.01])
    return None, None


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_reference_forms_agree_within_the_bound(name):
    n, T, C, depth, flags = CASES[name]
    off, scl = channel_maps(name)
    inc = R.increments(make_series(name), flags, off, scl)
    d, D = R.signature_dim(C, depth, flags)
    assert D == DIMS[name] and inc.shape == (n, (T - 1 + (flags & R.BASEPOINT)) * (2 if flags & R.LEAD_LAG else 1), d)
    a, b = R.signature(inc, depth), R.signature_direct(inc, depth)
    bound = R.error_bounds(inc, depth)
    assert a.shape == b.shape == bound.shape == (n, D)
    share = float((np.abs(a - b) / np.maximum(bound, 1e-300)).max())
    print(f"{name:18s} max |horner - direct| {np.abs(a - b).max():.3e}  share of bound {share:.4f}")
    assert (np.abs(a - b) <= bound).all(), (name, share)
    # the majorant behind the bound: every level's absolute sum is at most l^k / k!
    ell = np.abs(inc).sum(axis=(1, 2))
    for k, sl in enumerate(R.level_slices(d, depth), start=1):
        assert (np.abs(a[:, sl]).sum(axis=1) <= ell ** k / math.factorial(k) * (1 + 1e-9)).all()


def test_the_path_is_built_in_the_stated_order():
    x = np.array([[[1.0, 10.0], [3.0, 14.0], [6.0, 12.0]]])
    off, scl = np.array([1.0, 10.0]), np.array([2.0, 0.5])
    assert np.array_equal(R.increments(x, 0, off, scl), [[[4.0, 2.0], [6.0, -1.0]]])
    assert np.array_equal(R.increments(x, R.BASEPOINT, off, scl), [[[0.0, 0.0], [4.0, 2.0], [6.0, -1.0]]])
    assert np.array_equal(R.increments(x, R.BASEPOINT), [[[1.0, 10.0], [2.0, 4.0], [3.0, -2.0]]])
    ll = R.increments(x, R.LEAD_LAG | R.TIME, off, scl)
    assert np.array_equal(ll, [[[4, 2, 0, 0, 0.25], [0, 0, 4, 2, 0.25], [6, -1, 0, 0, 0.25], [0, 0, 6, -1, 0.25]]])
    assert np.array_equal(R.increments(x, R.TIME)[..., -1], [[0.5, 0.5]])


def test_a_linear_path_gives_the_tensor_exponential():
    rs = np.random.RandomState(0)
    v = rs.standard_normal(3)
    for pieces in (1, 7):
        inc = np.tile(v / pieces, (1, pieces, 1))
        got = R.signature(inc, 4)
        want, level = [], np.ones(1)
        for k in range(1, 5):
            level = np.multiply.outer(level, v).reshape(-1)
            want.append(level / math.factorial(k))
        want = np.concatenate(want)[None]
        assert (np.abs(got - want) <= R.error_bounds(inc, 4)).all()


def test_level_one_is_the_total_increment_and_the_shuffle_identity():
    for name in ("ecg", "lead_lag", "odd", "chunk_boundaries"):
        n, T, C, depth, flags = CASES[name]
        off, scl = channel_maps(name)
        inc = R.increments(make_series(name), flags, off, scl)
        d, D = R.signature_dim(C, depth, flags)
        sig, bound = R.signature(inc, depth), R.error_bounds(inc, depth)
        assert (np.abs(sig[:, :d] - inc.sum(axis=1)) <= bound[:, :d]).all()
        # S_i S_j = S_ij + S_ji
        l1, l2 = sig[:, :d], sig[:, d: d + d * d].reshape(n, d, d)
        b1, b2 = bound[:, :1], bound[:, d: d + 1]
        tol = (np.abs(l1)[:, :, None] * b1[:, :, None] + np.abs(l1)[:, None, :] * b1[:, :, None] + b1[:, :, None] ** 2
               + 2 * b2[:, :, None])
        assert (np.abs(l1[:, :, None] * l1[:, None, :] - l2 - l2.transpose(0, 2, 1)) <= tol).all(), name


def test_signature_dim_and_level_slices():
    from fourierdiffusion_amd.utils.signature import level_slices, signature_dim
    assert signature_dim(1, 4, time_augment=True, lead_lag=False) == (2, 30)
    assert signature_dim(40, 2, time_augment=True, lead_lag=False) == (41, 1722)
    assert signature_dim(64, 2, time_augment=True, lead_lag=False) == (65, 4290)
    assert signature_dim(3, 3, time_augment=True, lead_lag=True) == (7, 399)
    assert signature_dim(2, 3, time_augment=False, lead_lag=False) == (2, 14)
    assert signature_dim(1, 6, time_augment=False, lead_lag=False) == (1, 6)
    assert level_slices(2, 4) == [slice(0, 2), slice(2, 6), slice(6, 14), slice(14, 30)]
    assert level_slices(7, 1) == [slice(0, 7)]
    for name, (n, T, C, depth, flags) in CASES.items():
        got = signature_dim(C, depth, time_augment=bool(flags & R.TIME), lead_lag=bool(flags & R.LEAD_LAG))
        assert got == R.signature_dim(C, depth, flags) and got[1] == DIMS[name]
        assert level_slices(got[0], depth) == R.level_slices(got[0], depth) and level_slices(got[0], depth)[-1].stop == got[1]
    for bad in (dict(channels=0, depth=2), dict(channels=65, depth=2), dict(channels=2, depth=0), dict(channels=2, depth=7),
                dict(channels=2, depth=2.0), dict(channels=True, depth=2)):
        with pytest.raises(ValueError, match="must be an integer in"):
            signature_dim(bad["channels"], bad["depth"], time_augment=True, lead_lag=False)


def test_every_value_error_comes_before_the_engine():
    from fourierdiffusion_amd.utils.signature import series_signature
    x = np.zeros((4, 8, 2), dtype=np.float32)
    cases = [
        (dict(X=np.zeros((4, 8), dtype=np.float32)), "must be an \\(n, T, C\\) array"),
        (dict(X=np.zeros((0, 8, 2), dtype=np.float32)), "must be an \\(n, T, C\\) array"),
        (dict(X=np.zeros((4, 1, 2), dtype=np.float32)), "T >= 2"),
        (dict(X=np.zeros((4, 8, 0), dtype=np.float32)), "C >= 1"),
        (dict(X=np.zeros((1, 1025, 1), dtype=np.float32)), "at most 1024 and 64"),
        (dict(X=np.zeros((1, 4, 65), dtype=np.float32)), "at most 1024 and 64"),
        (dict(X=x, depth=0), "depth=0 must be an integer in \\[1, 6\\]"),
        (dict(X=x, depth=7), "depth=7 must be an integer in \\[1, 6\\]"),
        (dict(X=x, depth=2.5), "must be an integer in \\[1, 6\\]"),
        (dict(X=np.zeros((1, 4, 64), dtype=np.float32), depth=3), "at most 8192"),                # 65 + 65^2 + 65^3
        (dict(X=np.zeros((1, 4, 45), dtype=np.float32), depth=2, lead_lag=True), "D = 8372 features, at most 8192"),
        (dict(X=torch.zeros(1).expand(600000, 2, 64), depth=2, time_augment=False), "n \\* D = 2496000000 must stay below 2\\^31"),
        (dict(X=x, channel_scale=[1.0, -1.0]), "channel_scale must be finite and >= 0"),
        (dict(X=x, channel_scale=[1.0, float("inf")]), "channel_scale must be finite and >= 0"),
        (dict(X=x, channel_scale=[1.0, float("nan")]), "channel_scale must be finite and >= 0"),
        (dict(X=x, channel_scale=[1.0]), "1 entries for 2 channels"),
        (dict(X=x, channel_offset=[0.0, float("nan")]), "channel_offset must be finite"),
        (dict(X=x, channel_offset=[0.0, 1.0, 2.0]), "3 entries for 2 channels"),
        (dict(X=x, path_scale=-1.0), "path_scale=-1.0 must be a finite number >= 0"),
        (dict(X=x, path_scale=float("nan")), "must be a finite number >= 0"),
        (dict(X=x, channel_scale=[1e300, 1.0], path_scale=1e300), "channel_scale \\* path_scale must be finite"),
        (dict(X=x, per_series=("sig", "mean")), "per_series names 'mean'"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            series_signature(**kw)


def test_no_cpu_fallback():
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.metrics import SignatureDistance
    from fourierdiffusion_amd.utils.signature import series_signature
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_C.FdError, match="no CPU fallback"):
        series_signature(np.zeros((4, 8, 2), dtype=np.float32))
    with pytest.raises(_C.FdError, match="no CPU fallback"):
        SignatureDistance(torch.zeros(4, 8, 2))


def _as_signature(rows, d, depth):
    from fourierdiffusion_amd.utils.signature import SeriesSignature, level_slices
    t = torch.from_numpy(rows)
    return SeriesSignature(sig=t.float(), sqnorm=(t * t).sum(dim=1), mean=t.mean(dim=0), d=d, depth=depth,
                           levels=level_slices(d, depth), n=rows.shape[0])


def test_distance_arithmetic_against_the_gram_matrices():
    from fourierdiffusion_amd.utils.signature import expected_signature_distance
    rs = np.random.RandomState(3)
    d, depth = 3, 3
    D = 39
    for na, nb in ((17, 23), (2, 5), (1, 9), (1, 1)):
        sa, sb = rs.standard_normal((na, D)) + 0.3, rs.standard_normal((nb, D)) * 1.5
        got = expected_signature_distance(_as_signature(sa, d, depth), _as_signature(sb, d, depth))
        want = R.expected_signature_distance(sa, sb, d, depth)
        assert sorted(got) == ["sig_mmd2", "sig_w1", "sig_w1_levels"] and len(got["sig_w1_levels"]) == depth
        scale = (sa ** 2).sum(axis=1).max() + (sb ** 2).sum(axis=1).max()
        assert abs(got["sig_w1"] - want["sig_w1"]) <= 1e-13 * max(1.0, want["sig_w1"])
        assert np.abs(np.array(got["sig_w1_levels"]) - want["sig_w1_levels"]).max() <= 1e-13 * max(1.0, want["sig_w1"])
        assert abs(got["sig_mmd2"] - want["sig_mmd2"]) <= 1e-12 * scale, (na, nb)
        assert abs(sum(v * v for v in got["sig_w1_levels"]) - got["sig_w1"] ** 2) <= 1e-12 * max(1.0, got["sig_w1"] ** 2)
    same = _as_signature(sa, d, depth)
    assert expected_signature_distance(same, same)["sig_w1"] == 0.0
    with pytest.raises(ValueError, match="different shape"):
        expected_signature_distance(_as_signature(sa, d, depth), _as_signature(sb[:, :12], 3, 2))


def test_the_reversed_sawtooth_separates_in_the_reference():
    """What tests/test_gpu_signature.py asserts of the engine holds for the float64 reference alone (same seed and shapes): the
    expected signatures of a sawtooth and of its time reversal are further apart than two folds of the sawtooth."""
    rng = np.random.default_rng(2025)
    real, fake = R.sawtooth(rng, 400, 64), R.sawtooth(rng, 200, 64)[:, ::-1].copy()
    x = real.astype(np.float64).reshape(-1, 1)
    off, scl = x.mean(axis=0), 1.0 / x.std(axis=0)
    sig = lambda s: R.signature(R.increments(s, R.TIME, off, scl), 4)
    d, depth = 2, 4
    w1 = R.expected_signature_distance(sig(fake), sig(real), d, depth)["sig_w1"]
    w1_self = R.expected_signature_distance(sig(real[:200]), sig(real[200:]), d, depth)["sig_w1"]
    print(f"sig_w1 reversed {w1:.4f}  self {w1_self:.4f}")
    assert w1 > w1_self


def test_signature_config_composes_and_the_others_are_untouched():
    from fourierdiffusion_amd.config import compose, instantiate
    from fourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SignatureDistance, SlicedWasserstein
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "sample", ["metrics=signature", "random_seed=7"]).metrics
    assert cfg.holdout is True
    make = instantiate({k: v for k, v in cfg.items() if k != "holdout"})
    assert isinstance(make, partial) and make.func is MetricCollection
    assert make.keywords["include_spectral_density"] is True and make.keywords["include_baselines"] is True
    assert [m.func for m in make.keywords["metrics"]] == [SlicedWasserstein, MarginalWasserstein, SignatureDistance]
    assert make.keywords["metrics"][2].keywords == dict(depth=3, time_augment=True, basepoint=False, lead_lag=False, path_scale=1.0,
                                                        standardise=True)
    default = compose(conf, "sample", ["random_seed=7"]).metrics
    assert [dict(m) for m in cfg.metrics[:2]] == [dict(m) for m in default.metrics]
    assert SignatureDistance.views == ("time",)
    names = SignatureDistance.__init__.__code__.co_varnames[1:9]
    assert set(names) == {"original_samples", "holdout_samples", "depth", "time_augment", "basepoint", "lead_lag", "path_scale",
                          "standardise"}
