"""GPU: fd_series_spectra (csrc/fd_spectral.hip), utils/spectral.py and sampling/metrics.py SpectralDependence against the float64
reference of tests/spectral_ref.py.

Every per-series output and the set mean are held to spectral_ref.error_bounds, the derived per-entry bound (nothing tuned: u = 2^-24
enters through the centred, windowed segment, through the float32 basis and DFT accumulation and through the returned value).  The
engine is also held to the float32 restatement (spectral_ref.spectra_f32), which rounds where the kernel rounds, in the kernel's
order, and differs from it only in the order of the float64 additions: per output array
    max |engine - float64| <= 2 max |restatement - float64| + 2 u max |value|.
DESIGN.md 3.34 holds the measured shares of the bound per case.

Bit-level properties: a series' features do not depend on the batch, its position, the outputs asked for or the grid
(FDIFF_SPEC_SPLITS); a constant channel gives exact zeros and leaves the rest bit-identical; x + 1000 on the 1/1024 grid gives the bits
of x under detrend; csd of a duplicated channel is the psd with imaginary part 0; the set means are bit-identical for every grid and
run; nothing is written outside the outputs."""
from __future__ import annotations

import ctypes as C
import functools
import os
from functools import partial
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import spectral_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CHUNK = R.CHUNK_SERIES
SENTINEL = -777.0
GUARD = 64

CASES, VARIANTS = R.CASES, R.VARIANTS
MAIN = VARIANTS[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


class forced_splits:
    def __init__(self, splits):
        self.splits = splits

    def __enter__(self):
        self.old = os.environ.get("FDIFF_SPEC_SPLITS")
        if self.splits is not None:
            os.environ["FDIFF_SPEC_SPLITS"] = str(self.splits)
        else:
            os.environ.pop("FDIFF_SPEC_SPLITS", None)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("FDIFF_SPEC_SPLITS", None)
        else:
            os.environ["FDIFF_SPEC_SPLITS"] = self.old


def _guarded(shape, dtype):
    size = int(np.prod(shape))
    return torch.full((size + GUARD,), SENTINEL, dtype=dtype, device="cuda")


def shapes_of(n, Cn, S):
    K, NP = S // 2 + 1, Cn * (Cn - 1) // 2
    return {"psd": (n, K, Cn), "csd": (n, K, NP, 2), "summary": (n, Cn, 3), "mean": (K * Cn + 2 * K * NP + 3 * Cn,)}


def spec_raw(x, S, noverlap, window="hann", detrend=True, want=("psd", "csd", "summary", "mean"), splits=None):
    """fd_series_spectra through the C ABI on an (n, T, C) device tensor.  Every output is pre-filled with a sentinel and followed by
    guard entries, the workspace is guarded; returns {name: numpy array} after checking that the guards are intact and the bodies
    overwritten.  The set mean is always asked for (the entry point requires it)."""
    from fourierdiffusion_amd import _C
    n, T, Cn = x.shape
    shapes = shapes_of(n, Cn, S)
    want = tuple(want) + (("mean",) if "mean" not in want else ())
    bufs = {k: _guarded(shapes[k], torch.float64 if k == "mean" else torch.float32) for k in want if not (k == "csd" and Cn < 2)}
    h, lib = _C.ctx(x.device), _C.lib()
    with forced_splits(splits):
        need = C.c_size_t(0)
        _C.check(lib.fd_series_spectra_workspace_bytes(h, n, T, Cn, S, noverlap, C.byref(need)), h)
        work = torch.full((need.value + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        _C.check(lib.fd_series_spectra(h, x.data_ptr(), n, T, Cn, S, noverlap, R.WINDOWS[window], int(bool(detrend)),
                                       _C.ptr(bufs.get("psd")), _C.ptr(bufs.get("csd")), _C.ptr(bufs.get("summary")),
                                       _C.ptr(bufs.get("mean")), work.data_ptr(), need.value, _C.stream_of(x)), h)
    torch.cuda.synchronize()
    assert bool((work[need.value:] == 0x5A).all()), "written past the workspace"
    out = {}
    for k, b in bufs.items():
        size = int(np.prod(shapes[k]))
        host = b.cpu().numpy()
        assert (host[size:] == SENTINEL).all(), f"written past {k}"
        assert not (host[:size] == SENTINEL).any(), f"{k} not fully written"
        out[k] = host[:size].reshape(shapes[k]).copy()
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    x = R.make_series(name).astype(np.float32)
    return x, dev(x)


@functools.lru_cache(maxsize=None)
def case(name, variant=MAIN):
    """Inputs, the float64 reference, its bound, the restatement and ONE engine run with every output, shared (nothing writes to
    them)."""
    n, T, Cn, S, ov = CASES[name]
    window, detrend = variant
    x, xd = inputs(name)
    return dict(x=x, xd=xd, ref=R.spectra_f64(x, S, ov, window, detrend), bound=R.error_bounds(x, S, ov, window, detrend),
                low=R.spectra_f32(x, S, ov, window, detrend), got=spec_raw(xd, S, ov, window, detrend))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _arrays(f):
    out = {"psd": f.psd, "total_power": f.summary[..., 0], "centroid": f.summary[..., 1], "entropy": f.summary[..., 2]}
    if f.csd is not None:
        out["csd"] = f.csd
    return out


def _got_spectra(got):
    return R.Spectra(got["psd"].astype(np.float64), got["csd"].astype(np.float64) if "csd" in got else None,
                     got["summary"].astype(np.float64))


# ---------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}-{'detrend' if v[1] else 'raw'}")
@pytest.mark.parametrize("name", list(CASES))
def test_outputs_within_the_derived_bound_and_near_the_restatement(name, variant):
    n, T, Cn, S, ov = CASES[name]
    c = case(name, variant)
    got = _got_spectra(c["got"])
    ref, bound, low = _arrays(c["ref"]), _arrays(c["bound"]), _arrays(c["low"])
    for key, g in _arrays(got).items():
        err, dev_low = np.abs(g - ref[key]), np.abs(low[key].astype(np.float64) - ref[key])
        share = float((err / np.maximum(bound[key], 1e-300)).max())
        print(f"{name:18s} {variant[0]:6s} {int(variant[1])} {key:11s} max err {err.max():.3e}  share of bound {share:.4f}  "
              f"restatement {dev_low.max():.3e}")
        assert np.isfinite(g).all()
        assert (err <= bound[key]).all(), (name, key, float(err.max()), share)
        assert err.max() <= 2 * dev_low.max() + 2 * R.U32 * np.abs(ref[key]).max(), (name, key)
    # the set mean: the mean of the float32 features as returned (n 2^-53 relative), hence within the mean bound of the reference's
    flat = got.flat()
    mean = c["got"]["mean"]
    assert np.abs(mean - flat.mean(axis=0)).max() <= n * R.V64 * max(1.0, np.abs(flat).max())
    assert (np.abs(mean - c["ref"].set_mean()) <= c["bound"].flat().mean(axis=0) + n * R.V64 * np.abs(flat).max(axis=0)).all()


def test_psd_is_real_nonnegative_and_coherence_at_most_one():
    for name in ("mimic", "droughts", "odd_everything"):
        n, T, Cn, S, ov = CASES[name]
        got = case(name)["got"]
        assert (got["psd"] >= 0).all()
        ci, di = R.pairs(Cn)
        mag2 = got["csd"][..., 0].astype(np.float64) ** 2 + got["csd"][..., 1].astype(np.float64) ** 2
        den = got["psd"][:, :, ci].astype(np.float64) * got["psd"][:, :, di]
        assert (mag2 <= den * (1 + 1e-4) + 1e-30).all(), name                # Cauchy-Schwarz over the segments, per series


def test_constant_channel():
    n, T, Cn, S, ov = CASES["mimic"]
    c = case("mimic")
    x = c["x"].copy()
    x[:, :, 7] = 3.3                                                        # not representable: float32(3.3) T times
    x[2, :, 11] = -1000.25
    got = spec_raw(dev(x), S, ov)
    base = c["got"]
    ci, di = R.pairs(Cn)
    for s, ch in [(slice(None), 7), (2, 11)]:
        assert not got["psd"][s, :, ch].any() and not got["summary"][s, ch].any()
        assert not got["csd"][s][..., (ci == ch) | (di == ch), :].any()
    for key in ("psd", "csd", "summary", "mean"):
        assert np.isfinite(got[key]).all()
    keep = np.ones((n, Cn), dtype=bool)
    keep[:, 7] = False
    keep[2, 11] = False
    kp = np.broadcast_to(keep[:, None, :], got["psd"].shape)
    assert np.array_equal(bits(got["psd"][kp]), bits(base["psd"][kp]))
    assert np.array_equal(bits(got["summary"][keep]), bits(base["summary"][keep]))
    kc = np.broadcast_to((keep[:, ci] & keep[:, di])[:, None, :, None], got["csd"].shape)
    assert np.array_equal(bits(got["csd"][kc]), bits(base["csd"][kc]))


@pytest.mark.parametrize("name", ["ecg", "mimic", "odd_S_hop_1", "droughts"])
def test_offset_of_1000_gives_the_same_bits(name):
    """series + 1000 (exact in float32 on the cases' grid): under detrend S x and the segment sum are exact in double, so the centred
    entry, and with it every output, has the bits of the unshifted series'."""
    n, T, Cn, S, ov = CASES[name]
    c = case(name)
    shifted = (c["x"].astype(np.float64) + 1000.0).astype(np.float32)
    assert np.array_equal(shifted.astype(np.float64), c["x"].astype(np.float64) + 1000.0)
    got = spec_raw(dev(shifted), S, ov)
    for key, val in got.items():
        assert np.array_equal(bits(val), bits(c["got"][key])), (name, key)


def test_duplicated_channel():
    """csd of a channel copied into two columns: imaginary part exactly 0, real part the psd to the bit."""
    n, T, Cn, S, ov = CASES["droughts"]
    x = case("droughts")["x"].copy()
    x[:, :, 9] = x[:, :, 4]
    x[:, :, 12] = x[:, :, 0]
    got = spec_raw(dev(x), S, ov)
    ci, di = R.pairs(Cn)
    for a, b in ((4, 9), (0, 12)):
        p = int(np.flatnonzero((ci == a) & (di == b))[0])
        assert not got["csd"][:, :, p, 1].any()
        assert np.array_equal(bits(got["csd"][:, :, p, 0]), bits(got["psd"][:, :, a]))
        assert np.array_equal(bits(got["psd"][:, :, a]), bits(got["psd"][:, :, b]))


# ---------------------------------------------------------------------------------------------- purity and determinism
@pytest.mark.parametrize("name", ["ecg", "mimic", "odd_everything", "chunk_boundaries"])
def test_a_series_alone_and_in_the_batch(name):
    n, T, Cn, S, ov = CASES[name]
    c = case(name)
    for i in sorted({0, n // 2, n - 1}):
        alone = spec_raw(c["xd"][i: i + 1].contiguous(), S, ov)
        for key in ("psd", "csd", "summary"):
            if key in alone:
                assert np.array_equal(bits(alone[key][0]), bits(c["got"][key][i])), (name, i, key)
        assert np.array_equal(bits(alone["mean"]), bits(_got_spectra(alone).flat()[0]))        # a mean over one series is the series


@pytest.mark.parametrize("name", ["mimic", "droughts"])
def test_any_subset_of_outputs(name):
    n, T, Cn, S, ov = CASES[name]
    c = case(name)
    for want in (("psd",), ("csd",), ("summary",), ("mean",), ("psd", "summary"), ("csd", "summary")):
        got = spec_raw(c["xd"], S, ov, want=want)
        assert set(got) == set(want) | {"mean"}
        for key in got:
            assert np.array_equal(bits(got[key]), bits(c["got"][key])), (name, want, key)


@pytest.mark.parametrize("name", ["ecg", "mimic", "odd_everything", "chunk_boundaries"])
def test_bit_identical_for_every_grid_and_run(name):
    n, T, Cn, S, ov = CASES[name]
    c = case(name)
    for splits in (None, 1, 3, 1000):
        got = spec_raw(c["xd"], S, ov, splits=splits)
        for key, val in got.items():
            assert np.array_equal(bits(val), bits(c["got"][key])), (name, splits, key)


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors_and_limits():
    """Every refusal the header lists is FD_ERR_ARG with a retrievable message, and nothing is launched: the outputs keep their
    sentinel."""
    from fourierdiffusion_amd import _C
    x = torch.zeros(8, 6, 2, device="cuda")
    sh = shapes_of(8, 2, 4)
    ps, cs, su, me = (_guarded(sh[k], torch.float64 if k == "mean" else torch.float32) for k in ("psd", "csd", "summary", "mean"))
    h, lib = _C.ctx(x.device), _C.lib()
    need = C.c_size_t(0)
    assert lib.fd_series_spectra_workspace_bytes(h, 8, 6, 2, 4, 2, C.byref(need)) == 0 and need.value > 0
    work = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    p, a, b, c, m, w, nb = x.data_ptr(), ps.data_ptr(), cs.data_ptr(), su.data_ptr(), me.data_ptr(), work.data_ptr(), need.value
    ws, run = lib.fd_series_spectra_workspace_bytes, lib.fd_series_spectra
    cases = [
        (lambda: ws(h, 8, 6, 2, 4, 2, None), b"null"),
        (lambda: ws(h, 0, 6, 2, 4, 2, C.byref(need)), b"bad shape"),
        (lambda: ws(h, 8, 6, 0, 4, 2, C.byref(need)), b"bad shape"),
        (lambda: ws(h, 8, 1025, 2, 4, 2, C.byref(need)), b"at most T=1024"),
        (lambda: ws(h, 8, 6, 65, 4, 2, C.byref(need)), b"C=64"),
        (lambda: ws(h, 8, 6, 2, 1, 0, C.byref(need)), b"nperseg=1"),
        (lambda: ws(h, 8, 6, 2, 7, 0, C.byref(need)), b"nperseg=7"),
        (lambda: ws(h, 8, 6, 2, 4, -1, C.byref(need)), b"noverlap=-1"),
        (lambda: ws(h, 8, 6, 2, 4, 4, C.byref(need)), b"noverlap=4"),
        (lambda: ws(h, 8, 1024, 64, 512, 256, C.byref(need)), b"bytes of LDS per series"),
        (lambda: ws(h, 8, 1024, 16, 16, 15, C.byref(need)), b"at most 163840"),
        (lambda: ws(h, 1 << 22, 1024, 1, 512, 0, C.byref(need)), b"too large"),
        (lambda: run(h, None, 8, 6, 2, 4, 2, 1, 1, a, b, c, m, w, nb, None), b"null x"),
        (lambda: run(h, p, 0, 6, 2, 4, 2, 1, 1, a, b, c, m, w, nb, None), b"bad shape"),
        (lambda: run(h, p, 8, 1025, 2, 4, 2, 1, 1, a, b, c, m, w, nb, None), b"at most"),
        (lambda: run(h, p, 8, 6, 2, 7, 2, 1, 1, a, b, c, m, w, nb, None), b"nperseg=7"),
        (lambda: run(h, p, 8, 6, 2, 4, 4, 1, 1, a, b, c, m, w, nb, None), b"noverlap=4"),
        (lambda: run(h, p, 8, 6, 2, 4, 2, 2, 1, a, b, c, m, w, nb, None), b"window=2"),
        (lambda: run(h, p, 8, 6, 2, 4, 2, 1, 2, a, b, c, m, w, nb, None), b"detrend=2"),
        (lambda: run(h, p, 8, 1024, 64, 512, 256, 1, 1, a, b, c, m, w, nb, None), b"bytes of LDS per series"),
        (lambda: run(h, p, 8, 6, 2, 4, 2, 1, 1, a, b, c, None, w, nb, None), b"null out_set_mean"),
        (lambda: run(h, p, 16, 6, 1, 4, 2, 1, 1, a, b, c, m, w, nb, None), b"out_csd with C=1"),
        (lambda: run(h, p, 8, 6, 2, 4, 2, 1, 1, a, b, c, m, None, nb, None), b"workspace"),
        (lambda: run(h, p, 8, 6, 2, 4, 2, 1, 1, a, b, c, m, w, nb - 1, None), b"workspace"),
    ]
    for i, (call, text) in enumerate(cases):
        assert call() == -1, i                                                  # FD_ERR_ARG
        assert text in lib.fd_last_error(h), (i, lib.fd_last_error(h))
    torch.cuda.synchronize()
    for buf in (ps, cs, su, me):
        assert bool((buf == SENTINEL).all())
    assert run(h, p, 8, 6, 2, 4, 2, 1, 1, None, None, None, m, w, nb, None) == 0          # the set mean alone
    assert lib.fd_series_spectra(None, p, 8, 6, 2, 4, 2, 1, 1, a, b, c, m, w, nb, None) == -1
    # every dataset shape fits at the default segments
    from fourierdiffusion_amd.utils.spectral import resolve_segments
    for T, Cn in ((187, 1), (252, 5), (251, 4), (134, 5), (24, 40), (365, 13)):
        S, ov = resolve_segments(T)
        assert ws(h, 64, T, Cn, S, ov, C.byref(need)) == 0, (T, Cn, lib.fd_last_error(h))


def test_wrapper_raises_the_engines_message_over_the_lds_limit():
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.utils.spectral import series_spectra
    with pytest.raises(_C.FdError, match="bytes of LDS per series"):
        series_spectra(torch.zeros(2, 1024, 64, device="cuda"))


# ---------------------------------------------------------------------------------------------- the wrapper and the metric
def _metric_sets():
    rs = np.random.RandomState(5)
    real = np.cumsum(rs.standard_normal((64, 32, 3)), axis=1) * 0.5
    real[:, 3:, 1] += real[:, :-3, 0]
    fake = rs.standard_normal((50, 32, 3)) ** 3
    held = np.cumsum(rs.standard_normal((20, 32, 3)), axis=1) * 0.5
    return real.astype(np.float32), fake.astype(np.float32), held.astype(np.float32)


def test_wrapper_matches_the_raw_call_the_defaults_and_the_reference():
    from fourierdiffusion_amd.utils.spectral import series_spectra
    real, _, _ = _metric_sets()
    res = series_spectra(real, per_series=("psd", "csd", "summary"))          # a host array is moved; the defaults at T = 32 are (16, 8)
    assert (res.nperseg, res.noverlap, res.n_segments) == (16, 8, 3)
    raw = spec_raw(dev(real), 16, 8)
    for key in ("psd", "csd", "summary"):
        assert np.array_equal(bits(getattr(res, key).cpu().numpy()), bits(raw[key]))
    want = R.reference_series_spectra(real, per_series=("psd", "csd", "summary"))
    bound = R.error_bounds(real, 16, 8)
    assert np.array_equal(res.freqs.cpu().numpy(), np.arange(9) / 16)
    sm, wm = res.set_mean, want.set_mean
    assert (np.abs(sm.psd.cpu().numpy() - wm.psd.numpy()) <= bound.psd.mean(axis=0) + 1e-15).all()
    assert (np.abs(sm.summary.cpu().numpy() - wm.summary.numpy()) <= bound.summary.mean(axis=0) + 1e-15).all()
    full = sm.csd.cpu().numpy()
    assert np.array_equal(full, np.conj(np.swapaxes(full, 1, 2)))                           # Hermitian
    assert np.array_equal(np.einsum("kcc->kc", full).real, sm.psd.cpu().numpy()) and not np.einsum("kcc->kc", full).imag.any()
    ci, di = R.pairs(3)
    tol = bound.csd.mean(axis=0).max(axis=-1) * np.sqrt(2) + 1e-15
    assert (np.abs(full[:, ci, di] - wm.csd.numpy()[:, ci, di]) <= tol).all()
    coh, ref_coh = sm.coherence().cpu().numpy(), R.coherence(wm.csd.numpy())
    assert coh.shape == (9, 3, 3) and np.abs(coh - ref_coh).max() <= 1e-5
    dphi = sm.phase().cpu().numpy()[1:, 0, 1] - np.angle(wm.csd.numpy())[1:, 0, 1]
    assert np.abs((dphi + np.pi) % (2 * np.pi) - np.pi).max() <= 1e-4               # (pi and -pi are one phase: the Nyquist bin is real)
    one = series_spectra(case("ecg")["xd"], 93, 46)                           # no csd for one channel
    assert one.csd is None and one.set_mean.csd.shape == (47, 1, 1)
    assert np.array_equal(bits(one.psd.cpu().numpy()), bits(case("ecg")["got"]["psd"]))


def test_metric_keys_and_values_against_the_reference(monkeypatch):
    from fourierdiffusion_amd.sampling import metrics as M
    real, fake, held = _metric_sets()
    metric = M.SpectralDependence(torch.from_numpy(real), holdout_samples=torch.from_numpy(held))
    got, base = metric(torch.from_numpy(fake)), metric.baseline_metrics
    monkeypatch.setattr(M, "series_spectra", R.reference_series_spectra)
    ref_metric = M.SpectralDependence(torch.from_numpy(real), holdout_samples=torch.from_numpy(held))
    want, want_base = ref_metric(torch.from_numpy(fake)), ref_metric.baseline_metrics
    f = {k: R.spectra_f64(v, 16, 8) for k, v in (("real", real), ("fake", fake), ("held", held), ("a", real[:32]), ("b", real[32:]))}
    direct = R.metric_values(f["fake"], f["real"])
    direct.update(R.metric_values(f["fake"], f["held"], "_holdout"))
    direct_base = R.metric_values(f["a"], f["b"], "_self")
    stems = ["psd_log_distance", "psd_log_distance_max", "coherence_distance", "coherence_distance_max", "phase_distance",
             "spectral_centroid_wasserstein", "spectral_entropy_wasserstein"]
    assert sorted(got) == sorted(want) == sorted(direct) == sorted(s + x for s in stems for x in ("", "_holdout"))
    assert sorted(base) == sorted(want_base) == sorted(direct_base) == sorted(s + "_self" for s in stems)
    for src, ref, ind in ((got, want, direct), (base, want_base, direct_base)):
        for key, val in ref.items():
            print(f"{key:40s} engine {src[key]:.6e} reference {val:.6e} direct {ind[key]:.6e}")
            # set means over >= 20 series of features within a few u of their scale: 1e-4 absolute in dB / radians / coherence is two
            # orders above the engine's error; the float32 quantile arithmetic of utils/wasserstein.py adds 1e-5 relative
            assert abs(src[key] - val) <= 1e-4 + 1e-5 * abs(val), (key, src[key], val)
            assert abs(ind[key] - val) <= 1e-9 + 1e-5 * abs(val), (key, ind[key], val)
    same = M.SpectralDependence(torch.from_numpy(real))(torch.from_numpy(real))
    assert same and all(v == 0.0 for v in same.values()), same


def _yaml_metrics(name):
    from fourierdiffusion_amd.sampling import metrics as M
    node = yaml.safe_load(open(ROOT / "cmd" / "conf" / "metrics" / name))
    out = []
    for item in node["metrics"]:
        kw = {k: (0 if v == "${random_seed}" else v) for k, v in item.items() if not k.startswith("_")}
        if "num_directions" in kw:
            kw["num_directions"] = 16
        out.append(partial(getattr(M, item["_target_"].rsplit(".", 1)[1]), **kw))
    return node, out


def test_collection_over_the_spectral_config():
    from fourierdiffusion_amd.sampling.metrics import MetricCollection, SpectralDependence
    node, metrics = _yaml_metrics("spectral.yaml")
    default_node, default_metrics = _yaml_metrics("default.yaml")
    assert node["holdout"] is True and [m.func for m in metrics[:-1]] == [m.func for m in default_metrics]
    assert metrics[-1].func is SpectralDependence
    rs = np.random.RandomState(6)
    real = torch.from_numpy(np.cumsum(rs.standard_normal((40, 16, 3)), axis=1).astype(np.float32))
    held = torch.from_numpy(np.cumsum(rs.standard_normal((12, 16, 3)), axis=1).astype(np.float32))
    fake = torch.from_numpy(rs.standard_normal((30, 16, 3)).astype(np.float32))
    plain = MetricCollection(metrics=default_metrics, original_samples=real)(fake)
    with_holdout = MetricCollection(metrics=metrics, original_samples=real, holdout_samples=held)
    res = with_holdout(fake)
    assert {k: res[k] for k in plain} == plain                                  # every other key is as it was
    new = sorted(set(res) - set(plain))
    stems = ["psd_log_distance", "psd_log_distance_max", "coherence_distance", "coherence_distance_max", "phase_distance",
             "spectral_centroid_wasserstein", "spectral_entropy_wasserstein"]
    assert new == sorted(f"time_{s}{suffix}" for s in stems for suffix in ("", "_holdout", "_self"))
    assert all(np.isfinite(res[k]) for k in new)


def test_delayed_coupling_through_the_engine():
    """The CPU test's assertions (test_spectral_cpu.py, same sets), now on the engine."""
    from fourierdiffusion_amd.sampling.metrics import SpectralDependence, TemporalDependence
    real, fake = R.delayed_coupling()
    real, fake = torch.from_numpy(real.astype(np.float32)), torch.from_numpy(fake.astype(np.float32))
    metric = SpectralDependence(real, nperseg=64, noverlap=32)
    res, base = metric(fake), metric.baseline_metrics
    print(res["coherence_distance"], base["coherence_distance_self"])
    assert res["coherence_distance"] > 5 * base["coherence_distance_self"]
    assert TemporalDependence(real)(fake)["ccf_distance"] < 0.05
