"""CPU checks of the dependence features' reference (tests/dependence_ref.py) and of the argument validation that raises before any
engine call.  No engine calls here."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import dependence_ref as ref
from fourierdiffusion_amd.sampling.metrics import Metric, TemporalDependence
from fourierdiffusion_amd.utils.dependence import resolve_lags, series_dependence


def _series(seed, n, T, C):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, T, C))
    return np.cumsum(x, axis=1) * 0.3 + rng.standard_normal((n, 1, C))      # correlated in time, a different level per channel


# ---------------------------------------------------------------------------------------------- reference against the FFT route
@pytest.mark.parametrize("n,T,C,L,Lx", [(3, 2, 1, 1, -1), (4, 5, 1, 4, -1), (3, 187, 1, 46, -1), (3, 24, 7, 6, 6), (2, 65, 3, 64, 64)])
def test_reference_matches_fft_route(n, T, C, L, Lx):
    x = _series(1, n, T, C)
    a, b = ref.features(x, L, Lx), ref.features_fft(x, L, Lx)
    np.testing.assert_allclose(a.moments, b.moments, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a.acf, b.acf, rtol=0, atol=1e-12)
    if Lx >= 0:
        np.testing.assert_allclose(a.ccf, b.ccf, rtol=0, atol=1e-12)
        idx = np.arange(C)
        assert np.array_equal(a.ccf[:, 1: min(L, Lx) + 1, idx, idx], a.acf[:, : min(L, Lx)])
        np.testing.assert_allclose(a.ccf[:, 0, idx, idx], 1.0, rtol=0, atol=1e-15)
    assert np.abs(a.acf).max() <= 1 + 1e-12


def test_moments_against_direct_formulas():
    x = _series(2, 5, 40, 3)
    f = ref.features(x, 3, 0)
    mu = x.mean(axis=1)
    e = x - mu[:, None]
    np.testing.assert_allclose(f.moments[..., 0], mu, atol=1e-14)
    np.testing.assert_allclose(f.moments[..., 1], x.std(axis=1), atol=1e-13)
    np.testing.assert_allclose(f.moments[..., 2], (e ** 3).mean(axis=1) / x.std(axis=1) ** 3, atol=1e-12)
    np.testing.assert_allclose(f.moments[..., 3], (e ** 4).mean(axis=1) / x.var(axis=1) ** 2 - 3, atol=1e-12)
    # lag 0 of the cross-correlation is the correlation matrix
    np.testing.assert_allclose(f.ccf[:, 0], np.stack([np.corrcoef(s.T) for s in x]), atol=1e-12)


# ---------------------------------------------------------------------------------------------- closed forms
def test_alternating_series_closed_form():
    T = 12
    x = ((-1.0) ** np.arange(T))[None, :, None]
    acf = ref.features(x, T - 1).acf[0, :, 0]
    lags = np.arange(1, T)
    np.testing.assert_allclose(acf, (-1.0) ** lags * (T - lags) / T, atol=1e-15)


def test_affine_invariance():
    x = _series(3, 4, 30, 3)
    a = np.array([0.5, 2.0, 7.0])
    b = np.array([-3.0, 0.0, 11.0])
    f, g = ref.features(x, 7, 5), ref.features(x * a + b, 7, 5)
    np.testing.assert_allclose(f.acf, g.acf, atol=1e-12)
    np.testing.assert_allclose(f.ccf, g.ccf, atol=1e-12)
    np.testing.assert_allclose(f.moments[..., 2:], g.moments[..., 2:], atol=1e-10)


def test_delayed_channel_peaks_at_its_delay():
    rng = np.random.default_rng(4)
    T, s = 200, 5
    base = rng.standard_normal(T + s)
    x = np.stack([base[s:], base[:T]], axis=-1)[None]          # channel 1 is channel 0 delayed by s: x1[t] = x0[t - s]
    ccf = ref.features(x, 1, 12).ccf[0]
    assert int(np.argmax(ccf[:, 0, 1])) == s                  # sum_t e0[t] e1[t + l] peaks where t + l - s = t
    assert ccf[s, 0, 1] > 0.9
    assert np.abs(ccf[:, 1, 0]).max() < 0.35                  # the negative lags of the pair hold nothing but noise


def test_constant_channel_is_zero_and_leaves_the_others_alone():
    x = _series(5, 3, 24, 4)
    y = x.copy()
    y[:, :, 2] = 7.25
    f, g = ref.features(x, 6, 6), ref.features(y, 6, 6)
    assert np.array_equal(g.moments[:, 2], np.tile([7.25, 0.0, 0.0, 0.0], (3, 1)))
    assert not g.acf[:, :, 2].any() and not g.ccf[:, :, 2, :].any() and not g.ccf[:, :, :, 2].any()
    keep = [0, 1, 3]
    assert np.array_equal(f.acf[:, :, keep], g.acf[:, :, keep])
    assert np.array_equal(f.ccf[:, :, keep][:, :, :, keep], g.ccf[:, :, keep][:, :, :, keep])
    assert np.array_equal(f.moments[:, keep], g.moments[:, keep])
    for feats in (g, ref.features_f32(y, 6, 6), ref.error_bounds(y, 6, 6)):
        assert np.isfinite(feats.flat()).all()


# ---------------------------------------------------------------------------------------------- the bound and the restatement
def test_restatement_sits_inside_the_derived_bound():
    for shape, L, Lx in (((6, 50, 3), 12, 8), ((4, 187, 1), 46, -1)):
        x = _series(6, *shape).astype(np.float32)
        exact, low, bound = ref.features(x, L, Lx), ref.features_f32(x, L, Lx), ref.error_bounds(x, L, Lx)
        assert (np.abs(low.flat() - exact.flat()) <= bound.flat()).all()
        # Cauchy-Schwarz: an acf / ccf entry's bound is an absolute c u with c independent of T
        assert bound.acf.max() <= ref.closed_form_constant(shape[1]) * ref.U32
        if Lx >= 0:
            assert bound.ccf.max() <= ref.closed_form_constant(shape[1]) * ref.U32


def test_bound_survives_an_offset():
    x = np.round(_series(7, 4, 60, 2) * 1024) / 1024                      # on a grid where x + 1000 is exact in float32
    shifted = (x + 1000.0).astype(np.float32)
    assert np.array_equal(shifted.astype(np.float64), x + 1000.0)
    exact, low = ref.features(x, 15, 8), ref.features_f32(shifted, 15, 8)
    bound = ref.error_bounds(x, 15, 8, mean_of=shifted)
    assert (np.abs(low.flat() - exact.flat())[:, 8:] <= bound.flat()[:, 8:]).all()
    assert (np.abs(low.moments[..., 1:] - exact.moments[..., 1:]) <= bound.moments[..., 1:]).all()


def test_marginal_w2_reference():
    rng = np.random.default_rng(8)
    a = rng.standard_normal((40, 3))
    np.testing.assert_allclose(ref.w2_marginals(a, a + 2.0), 2.0, atol=1e-12)            # a shift moves every quantile by 2
    np.testing.assert_allclose(ref.w2_marginals(a, a[::-1]), 0.0, atol=1e-12)
    b = rng.standard_normal((30, 3))
    q = (np.arange(12000) + 0.5) / 12000                                                 # 12000 = a multiple of 40 and 30
    qa, qb = np.sort(a, axis=0)[(q * 40).astype(int)], np.sort(b, axis=0)[(q * 30).astype(int)]
    np.testing.assert_allclose(ref.w2_marginals(a, b), np.sqrt(((qa - qb) ** 2).mean(axis=0)), atol=1e-12)


# ---------------------------------------------------------------------------------------------- the metric's arithmetic
def test_ar1_against_iid_noise_on_the_reference():
    """The failure the metric exists for: i.i.d. noise with the right marginal variance in place of an AR(1) process."""
    rng = np.random.default_rng(2024)
    phi, T, L = 0.8, 100, 25
    real = ref.ar1(rng, 800, T, phi)
    fake = rng.standard_normal((400, T, 1)) / np.sqrt(1 - phi * phi)
    real_a, real_b = ref.features(real[:400], L), ref.features(real[400:], L)
    vals = ref.metric_values(ref.set_means(ref.features(fake, L)), ref.set_means(ref.features(real, L)), 1)
    self_vals = ref.metric_values(ref.set_means(real_a), ref.set_means(real_b), 1, "_self")
    print(vals["acf_distance"], self_vals["acf_distance_self"])
    assert vals["acf_distance"] > 0.1
    assert vals["acf_distance"] > 5 * self_vals["acf_distance_self"]
    assert "ccf_distance" not in vals


# ---------------------------------------------------------------------------------------------- validation before any engine call
def test_resolve_lags_defaults():
    assert resolve_lags(187, 1) == (46, -1)
    assert resolve_lags(24, 40) == (6, 6)
    assert resolve_lags(365, 13) == (91, 8)
    assert resolve_lags(2, 1) == (1, -1)
    assert resolve_lags(1, 3) == (0, 0)
    assert resolve_lags(100, 2, lags=10, cross_lags=-1) == (10, -1)


@pytest.mark.parametrize("kwargs,match", [
    (dict(lags=-1), "lags"), (dict(lags=24), "lags"), (dict(lags=2.5), "lags"), (dict(lags=True), "lags"),
    (dict(cross_lags=-2), "cross_lags"), (dict(cross_lags=24), "cross_lags"), (dict(per_series=("acf", "spectrum")), "per_series"),
])
def test_series_dependence_refuses_bad_arguments(kwargs, match):
    with pytest.raises(ValueError, match=match):
        series_dependence(torch.zeros(3, 24, 2), **kwargs)


def test_series_dependence_refuses_bad_shapes():
    with pytest.raises(ValueError, match=r"\(n, T, C\)"):
        series_dependence(torch.zeros(3, 24))
    with pytest.raises(ValueError, match=r"\(n, T, C\)"):
        series_dependence(torch.zeros(0, 24, 2))
    with pytest.raises(ValueError, match="at most"):
        series_dependence(torch.zeros(1, 1025, 1))
    with pytest.raises(ValueError, match="at most"):
        series_dependence(torch.zeros(1, 8, 65))
    with pytest.raises(ValueError, match="no cross lags"):
        series_dependence(torch.zeros(3, 24, 1), per_series=("ccf",))


@pytest.mark.parametrize("kwargs,match", [
    (dict(lags=40), "lags"), (dict(cross_lags=31), "cross_lags"), (dict(max_original=1), "max_original"),
    (dict(max_original=2.5), "max_original"), (dict(holdout_samples=torch.zeros(0, 31, 2)), "held-out"),
    (dict(holdout_samples=torch.zeros(4, 30, 2)), "same number of features"),
])
def test_metric_refuses_bad_arguments(kwargs, match):
    with pytest.raises(ValueError, match=match):
        TemporalDependence(torch.zeros(10, 31, 2), **kwargs)


def test_metric_needs_series():
    with pytest.raises(ValueError, match="time axis"):
        TemporalDependence(torch.zeros(10, 62))
    assert issubclass(TemporalDependence, Metric) and TemporalDependence.views == ("time",)
