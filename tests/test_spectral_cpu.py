"""CPU checks of the spectral features' reference (tests/spectral_ref.py) against scipy.signal, of the derived bound against the
float32 restatement on every GPU case's inputs, of the metric's arithmetic on the reference features and of the argument validation
that raises before any engine call.  No engine calls here."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

from tests import spectral_ref as ref
from fourierdiffusion_amd.sampling import metrics as M
from fourierdiffusion_amd.utils import spectral as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, VARIANTS, make_series = ref.CASES, ref.VARIANTS, ref.make_series


def _series(seed, n, T, C):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, T, C))
    return np.cumsum(x, axis=1) * 0.3 + rng.standard_normal((n, 1, C))


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_series_spectra", "fd_series_spectra_workspace_bytes"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


# ---------------------------------------------------------------------------------------------- the reference against scipy
@pytest.mark.parametrize("window", ["hann", "boxcar"])
@pytest.mark.parametrize("detrend", [True, False])
@pytest.mark.parametrize("T,S,noverlap", [(187, 64, 32), (24, 24, 0), (9, 4, 3), (30, 7, 2), (11, 2, 1)])
def test_reference_matches_scipy(T, S, noverlap, window, detrend):
    from scipy import signal
    n, C = 3, 3
    x = _series(1, n, T, C)
    f = ref.spectra_f64(x, S, noverlap, window, detrend)
    kw = dict(fs=1.0, window=window, nperseg=S, noverlap=noverlap, detrend="constant" if detrend else False, scaling="density",
              return_onesided=True)
    freqs, psd = signal.welch(x, axis=1, **kw)                              # (n, K, C)
    np.testing.assert_allclose(freqs, np.arange(S // 2 + 1) / S, rtol=0, atol=1e-15)
    np.testing.assert_allclose(f.psd, psd, rtol=1e-12, atol=1e-12 * np.abs(psd).max())
    ci, di = ref.pairs(C)
    for p, (c, d) in enumerate(zip(ci, di)):
        _, z = signal.csd(x[:, :, c], x[:, :, d], axis=1, **kw)
        scale = np.sqrt(psd[:, :, c].max() * psd[:, :, d].max())
        np.testing.assert_allclose(f.csd[:, :, p, 0] + 1j * f.csd[:, :, p, 1], z, rtol=1e-12, atol=1e-12 * scale)
    # for one series per set, the set-level coherence is scipy's per-series one
    for i in range(n):
        one = ref.Spectra(f.psd[i: i + 1], f.csd[i: i + 1], f.summary[i: i + 1])
        coh = ref.coherence(ref.full_csd(one.psd.mean(axis=0), one.csd.mean(axis=0)))
        for c, d in zip(ci, di):
            _, want = signal.coherence(x[i, :, c], x[i, :, d], **{k: v for k, v in kw.items() if k not in ("scaling", "return_onesided")})
            k0 = 1 if detrend and window == "boxcar" else 0             # that bin 0 is rounding noise over rounding noise
            np.testing.assert_allclose(coh[k0:, c, d], want[k0:], rtol=1e-12, atol=1e-12)
    # the summaries straight from scipy's psd
    tail = psd[:, 1:, :]
    np.testing.assert_allclose(f.summary[..., 0], psd.sum(axis=1), rtol=1e-12)
    np.testing.assert_allclose(f.summary[..., 1], (np.arange(1, S // 2 + 1)[None, :, None] / S * tail).sum(axis=1) / tail.sum(axis=1), rtol=1e-12)
    if S // 2 + 1 > 2:
        p = tail / tail.sum(axis=1, keepdims=True)
        np.testing.assert_allclose(f.summary[..., 2], -(p * np.log(p)).sum(axis=1) / np.log(S // 2), rtol=1e-12)
    else:
        assert not f.summary[..., 2].any()


def test_hann_window_is_scipys():
    from scipy import signal
    for S in (2, 3, 7, 24, 93, 256):
        np.testing.assert_allclose(ref.get_window("hann", S), signal.get_window("hann", S), rtol=0, atol=1e-15)


def test_constant_channel_is_zero_and_leaves_the_others_alone():
    x = _series(5, 3, 24, 4)
    y = x.copy()
    y[:, :, 2] = 7.25
    f, g = ref.spectra_f64(x, 12, 6), ref.spectra_f64(y, 12, 6)
    ci, di = ref.pairs(4)
    hit = (ci == 2) | (di == 2)
    assert not g.psd[:, :, 2].any() and not g.summary[:, 2].any() and not g.csd[:, :, hit].any()
    assert np.array_equal(f.psd[:, :, [0, 1, 3]], g.psd[:, :, [0, 1, 3]]) and np.array_equal(f.csd[:, :, ~hit], g.csd[:, :, ~hit])
    for feats in (g, ref.spectra_f32(y, 12, 6), ref.error_bounds(y, 12, 6)):
        assert np.isfinite(feats.flat()).all()
    assert not ref.spectra_f32(y, 12, 6).psd[:, :, 2].any()


def test_delayed_channel_has_full_coherence_and_a_linear_phase():
    rng = np.random.default_rng(4)
    n, T, s, S = 64, 128, 3, 32
    base = rng.standard_normal((n, T + s))
    x = np.stack([base[:, s:], base[:, :T]], axis=-1)                      # channel 1 is channel 0 delayed by s
    f = ref.spectra_f64(x, S, S // 2)
    P = ref.full_csd(f.psd.mean(axis=0), f.csd.mean(axis=0))
    coh = ref.coherence(P)[1:-1, 0, 1]
    assert coh.min() > 0.6                                                  # the segment edges cost the rest
    k = np.arange(1, 6)
    np.testing.assert_allclose(np.angle(P[k, 0, 1]), -2 * np.pi * k * s / S, atol=0.2)


# ---------------------------------------------------------------------------------------------- the bound and the restatement
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}-{'detrend' if v[1] else 'raw'}")
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_sits_inside_the_derived_bound_on_every_gpu_case(name, variant):
    n, T, C, S, ov = CASES[name]
    x = make_series(name).astype(np.float32)
    exact, low, bound = ref.spectra_f64(x, S, ov, *variant), ref.spectra_f32(x, S, ov, *variant), ref.error_bounds(x, S, ov, *variant)
    err = np.abs(low.flat().astype(np.float64) - exact.flat())
    assert np.isfinite(bound.flat()).all()
    assert (err <= bound.flat()).all(), float((err / np.maximum(bound.flat(), 1e-300)).max())
    # the bound is worth something: the psd's is a small multiple of (S + 4) u of the channel's total power
    total = exact.summary[..., 0][:, None, :]
    live = np.broadcast_to(total > 0, bound.psd.shape)
    assert (bound.psd[live] <= 16 * (S + 4) * ref.U32 * np.broadcast_to(total * S, bound.psd.shape)[live]).all()


def test_restatement_gives_the_same_bits_under_an_offset():
    x = make_series("ecg").astype(np.float32)
    shifted = (x.astype(np.float64) + 1000.0).astype(np.float32)
    assert np.array_equal(shifted.astype(np.float64), x.astype(np.float64) + 1000.0)
    a, b = ref.spectra_f32(x, 93, 46), ref.spectra_f32(shifted, 93, 46)
    assert np.array_equal(a.flat(), b.flat())


# ---------------------------------------------------------------------------------------------- the metric's arithmetic
class _NumpyWasserstein:
    """utils.wasserstein.WassersteinDistances' marginal distances from the reference's exact quantile integral."""

    def __init__(self, original_data, other_data, seed=None):
        self.a, self.b = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t) for t in (original_data, other_data))

    def marginal_distances(self):
        return ref.w2_marginals(self.a, self.b)


def _host_flat_array(x):
    """utils.tensors.check_flat_array without the move to the device."""
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x.detach()
    return x.reshape(x.shape[0], -1).float().contiguous()


@pytest.fixture
def reference_engine(monkeypatch):
    monkeypatch.setattr(M, "series_spectra", ref.reference_series_spectra)
    monkeypatch.setattr(M, "WassersteinDistances", _NumpyWasserstein)
    monkeypatch.setattr(M, "check_flat_array", _host_flat_array)


@pytest.mark.parametrize("nperseg,noverlap,factor", [(64, 32, 5.0), (128, 64, 5.0)])
def test_delayed_coupling_is_seen_by_coherence_and_missed_by_ccf(reference_engine, nperseg, noverlap, factor):
    """The failure the metric exists for: two channels with the right marginal spectra and no relation to one another, where the real
    ones are coupled at a delay of 20 steps -- beyond TemporalDependence's 8 cross lags."""
    from tests import dependence_ref as D
    real, fake = (a.astype(np.float32) for a in ref.delayed_coupling())      # the metric holds its samples in float32
    metric = M.SpectralDependence(torch.from_numpy(real), nperseg=nperseg, noverlap=noverlap)
    res, base = metric(torch.from_numpy(fake)), metric.baseline_metrics
    print(nperseg, res["coherence_distance"], base["coherence_distance_self"], res["psd_log_distance"], base["psd_log_distance_self"])
    assert res["coherence_distance"] > factor * base["coherence_distance_self"]
    assert res["coherence_distance"] > 0.15
    # the marginal spectra are equal by construction: the PSD distance stays near its baseline
    assert res["psd_log_distance"] < 3 * base["psd_log_distance_self"]
    # the time-domain metric at its default 8 cross lags sees nothing
    L, Lx = 32, 8
    vals = D.metric_values(D.set_means(D.features(fake, L, Lx)), D.set_means(D.features(real, L, Lx)), 2)
    assert vals["ccf_distance"] < 0.05
    # and the keys agree with the reference's own arithmetic
    S, ov = metric.nperseg, metric.noverlap
    direct = ref.metric_values(ref.spectra_f64(fake, S, ov), ref.spectra_f64(real, S, ov))
    assert sorted(direct) == sorted(res)
    for key, val in direct.items():
        assert abs(res[key] - val) <= 1e-9 + 1e-9 * abs(val), key


def test_metric_on_one_channel_and_on_itself(reference_engine):
    x = _series(9, 40, 32, 3).astype(np.float32)
    one = M.SpectralDependence(torch.from_numpy(x[:, :, :1].copy()))
    res = one(torch.from_numpy(x[::-1, :, 1:2].copy()))
    assert sorted(res) == ["psd_log_distance", "psd_log_distance_max", "spectral_centroid_wasserstein", "spectral_entropy_wasserstein"]
    assert (one.nperseg, one.noverlap, one.window) == (16, 8, "hann")
    same = M.SpectralDependence(torch.from_numpy(x))(torch.from_numpy(x))
    assert "phase_distance" in same and all(v == 0.0 for v in same.values())
    assert sorted(M.SpectralDependence(torch.from_numpy(x)).baseline_metrics) == sorted(k + "_self" for k in same)
    assert issubclass(M.SpectralDependence, M.Metric) and M.SpectralDependence.views == ("time",)
    assert M.SpectralDependence(torch.from_numpy(x)).name == "spectral_dependence"


def test_set_mean_assembly_is_hermitian_with_the_psd_on_its_diagonal():
    f = ref.spectra_f64(_series(3, 6, 20, 4), 8, 4)
    sm = U.assemble_set_mean(torch.from_numpy(f.set_mean()), 5, 4)
    full = sm.csd.numpy()
    assert np.array_equal(full, ref.full_csd(f.psd.mean(axis=0), f.csd.mean(axis=0)))
    assert np.array_equal(full, np.conj(np.swapaxes(full, 1, 2))) and np.array_equal(np.einsum("kcc->kc", full).real, sm.psd.numpy())
    np.testing.assert_allclose(sm.coherence().numpy(), ref.coherence(full), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(np.exp(1j * sm.phase().numpy()), np.exp(1j * np.angle(full)), rtol=0, atol=1e-15)   # (pi and -pi are one phase)
    assert np.array_equal(sm.summary.numpy(), f.summary.mean(axis=0))
    dead = U.assemble_set_mean(torch.zeros(5 * 2 + 2 * 5 + 6, dtype=torch.float64), 5, 2)
    assert not dead.coherence().numpy().any()                               # 0 where a denominator is 0, not NaN


# ---------------------------------------------------------------------------------------------- the configuration
def test_spectral_config_composes_and_instantiates():
    from functools import partial

    from fourierdiffusion_amd.config import compose, instantiate
    conf = os.path.join(ROOT, "cmd", "conf")
    cfg = compose(conf, "sample", ["metrics=spectral", "random_seed=7"]).metrics
    assert cfg.holdout is True
    make = instantiate({k: v for k, v in cfg.items() if k != "holdout"})
    assert isinstance(make, partial) and make.func is M.MetricCollection
    kinds = [m.func for m in make.keywords["metrics"]]
    assert kinds == [M.SlicedWasserstein, M.MarginalWasserstein, M.SpectralDependence]
    assert make.keywords["metrics"][2].keywords == {"random_seed": 7, "nperseg": None, "noverlap": None, "window": "hann"}
    default = compose(conf, "sample", ["random_seed=7"]).metrics
    assert [dict(m) for m in cfg.metrics[:2]] == [dict(m) for m in default.metrics]
    assert M.SpectralDependence.__init__.__code__.co_varnames[1:8] == ("original_samples", "holdout_samples", "nperseg", "noverlap",
                                                                        "window", "max_original", "random_seed")


# ---------------------------------------------------------------------------------------------- validation before any engine call
def test_resolve_segments_defaults():
    assert U.resolve_segments(187) == (93, 46)
    assert U.resolve_segments(24) == (24, 12)
    assert U.resolve_segments(31) == (31, 15)
    assert U.resolve_segments(32) == (16, 8)
    assert U.resolve_segments(365) == (182, 91)
    assert U.resolve_segments(2) == (2, 1)
    assert U.resolve_segments(100, 10) == (10, 5)
    assert U.resolve_segments(100, 10, 0) == (10, 0)
    assert U.resolve_segments(100, np.int64(100), 99) == (100, 99)


@pytest.mark.parametrize("args,match", [
    ((24, 1), "nperseg"), ((24, 25), "nperseg"), ((24, 2.5), "nperseg"), ((24, True), "nperseg"), ((24, "8"), "nperseg"),
    ((24, 8, -1), "noverlap"), ((24, 8, 8), "noverlap"), ((24, 8, 1.0), "noverlap"), ((24, 8, False), "noverlap"), ((1,), "at least 2"),
])
def test_resolve_segments_refuses(args, match):
    with pytest.raises(ValueError, match=match):
        U.resolve_segments(*args)


@pytest.mark.parametrize("kwargs,match", [
    (dict(nperseg=1), "nperseg"), (dict(nperseg=25), "nperseg"), (dict(noverlap=12, nperseg=12), "noverlap"),
    (dict(window="hamming"), "window"), (dict(window=1), "window"), (dict(detrend="linear"), "detrend"), (dict(detrend=False), "detrend"),
    (dict(per_series=("psd", "coherence")), "per_series"),
])
def test_series_spectra_refuses_bad_arguments(kwargs, match):
    with pytest.raises(ValueError, match=match):
        U.series_spectra(torch.zeros(3, 24, 2), **kwargs)


def test_series_spectra_refuses_bad_shapes():
    with pytest.raises(ValueError, match=r"\(n, T, C\)"):
        U.series_spectra(torch.zeros(3, 24))
    with pytest.raises(ValueError, match=r"\(n, T, C\)"):
        U.series_spectra(torch.zeros(0, 24, 2))
    with pytest.raises(ValueError, match="at most"):
        U.series_spectra(torch.zeros(1, 1025, 1))
    with pytest.raises(ValueError, match="at most"):
        U.series_spectra(torch.zeros(1, 8, 65))
    with pytest.raises(ValueError, match="no pairs"):
        U.series_spectra(torch.zeros(3, 24, 1), per_series=("csd",))
    with pytest.raises(ValueError, match="too large"):
        U.series_spectra(torch.zeros(1, 1, 1).expand(1 << 22, 1024, 1))


@pytest.mark.parametrize("kwargs,match", [
    (dict(nperseg=40), "nperseg"), (dict(noverlap=16), "noverlap"), (dict(window="blackman"), "window"),
    (dict(max_original=1), "max_original"), (dict(max_original=2.5), "max_original"),
    (dict(holdout_samples=torch.zeros(0, 32, 2)), "held-out"), (dict(holdout_samples=torch.zeros(4, 30, 2)), "same number of features"),
])
def test_metric_refuses_bad_arguments(kwargs, match):
    with pytest.raises(ValueError, match=match):
        M.SpectralDependence(torch.zeros(10, 32, 2), **kwargs)


def test_metric_needs_series():
    with pytest.raises(ValueError, match="time axis"):
        M.SpectralDependence(torch.zeros(10, 64))
