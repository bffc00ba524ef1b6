"""GPU: fd_series_dependence (csrc/fd_dependence.hip), utils/dependence.py and sampling/metrics.py TemporalDependence against the
float64 reference of tests/dependence_ref.py.

Every per-series output and the set mean are held to dependence_ref.error_bounds, the derived per-entry bound (nothing tuned:
u = 2^-24 enters through e = f32(x - mu) and through the returned value, every sum is a float64 chain, so an acf / ccf entry is
within about 5 u whatever T is).  The engine is also held to the float32 restatement (dependence_ref.features_f32), which rounds
where the kernel rounds and differs from it only in the order of the float64 additions: a re-ordered double sum can move e or a
returned value across a float32 rounding boundary, never further, so per output array
    max |engine - float64| <= 2 max |restatement - float64| + 2 u max |value|.
Measured on an MI355X (max over the array of |engine - float64|, as a share of the derived bound at that entry, and the
restatement's own deviation in the same units): DESIGN.md 3.29 holds the per-shape table.

Bit-level properties: a series' features do not depend on the batch, its position, the outputs asked for or the grid
(FDIFF_DEP_SPLITS); ccf's diagonal is acf; a constant channel gives exact zeros and leaves the rest bit-identical; the set means
are bit-identical for every grid and run; nothing is written outside the outputs."""
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

from tests import dependence_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CHUNK = R.CHUNK_SERIES
SENTINEL = -777.0
GUARD = 64

# (n, T, C, L, Lx)
CASES = {
    "lower_ends": (1, 2, 1, 1, -1),
    "lag_T-1": (3, 5, 1, 4, -1),
    "ecg": (7, 187, 1, 46, -1),
    "mimic": (5, 24, 40, 6, 6),
    "droughts": (4, 365, 13, 91, 8),
    "T_limit": (3, 1024, 2, 256, 8),
    "odd_everything": (65, 9, 17, 2, 2),
    "chunk_boundaries": (3 * CHUNK + 1, 16, 3, 4, 4),
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


class forced_splits:
    def __init__(self, splits):
        self.splits = splits

    def __enter__(self):
        self.old = os.environ.get("FDIFF_DEP_SPLITS")
        if self.splits is not None:
            os.environ["FDIFF_DEP_SPLITS"] = str(self.splits)
        else:
            os.environ.pop("FDIFF_DEP_SPLITS", None)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("FDIFF_DEP_SPLITS", None)
        else:
            os.environ["FDIFF_DEP_SPLITS"] = self.old


def _guarded(shape, dtype):
    size = int(np.prod(shape))
    return torch.full((size + GUARD,), SENTINEL, dtype=dtype, device="cuda")


def dep_raw(x, L, Lx, want=("moments", "acf", "ccf", "mean"), splits=None):
    """fd_series_dependence through the C ABI on an (n, T, C) device tensor.  Every output is pre-filled with a sentinel and
    followed by guard entries; returns {name: numpy array} after checking that the guards are intact and the body is overwritten."""
    from fourierdiffusion_amd import _C
    n, T, Cn = x.shape
    F = 4 * Cn + L * Cn + (Lx + 1) * Cn * Cn
    shapes = {"moments": (n, Cn, 4), "acf": (n, L, Cn), "ccf": (n, Lx + 1, Cn, Cn), "mean": (F,)}
    bufs = {k: _guarded(shapes[k], torch.float64 if k == "mean" else torch.float32) for k in want
            if not (k == "ccf" and Lx < 0) and not (k == "acf" and L < 1)}
    h, lib = _C.ctx(x.device), _C.lib()
    with forced_splits(splits):
        need = C.c_size_t(0)
        _C.check(lib.fd_series_dependence_workspace_bytes(h, n, T, Cn, L, Lx, C.byref(need)), h)
        work = torch.full((need.value + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        _C.check(lib.fd_series_dependence(h, x.data_ptr(), n, T, Cn, L, Lx, _C.ptr(bufs.get("moments")), _C.ptr(bufs.get("acf")),
                                          _C.ptr(bufs.get("ccf")), _C.ptr(bufs.get("mean")), work.data_ptr(), need.value,
                                          _C.stream_of(x)), h)
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


def make_series(name):
    n, T, Cn, L, Lx = CASES[name]
    rs = np.random.RandomState(len(name) * 100 + n + T + Cn)
    x = np.cumsum(rs.standard_normal((n, T, Cn)), axis=1) * 0.4 + rs.standard_normal((n, 1, Cn)) * 2.0 + rs.standard_normal((n, T, Cn))
    x *= np.exp(rs.uniform(-2, 2, size=(1, 1, Cn)))                       # a different scale per channel
    return np.round(x * 1024) / 1024                                       # on a grid: x + 1000 stays exact in float32


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the float64 reference, its bound, the restatement and ONE engine run with every output, shared (nothing writes to
    them)."""
    n, T, Cn, L, Lx = CASES[name]
    x = make_series(name).astype(np.float32)
    xd = dev(x)
    return dict(x=x, xd=xd, ref=R.features(x, L, Lx), bound=R.error_bounds(x, L, Lx), low=R.features_f32(x, L, Lx),
                got=dep_raw(xd, L, Lx))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _arrays(feats):
    out = {"mean": feats.moments[..., 0], "deviation": feats.moments[..., 1], "skewness": feats.moments[..., 2],
           "kurtosis": feats.moments[..., 3], "acf": feats.acf}
    if feats.ccf is not None:
        out["ccf"] = feats.ccf
    return out


def _got_features(got):
    return R.Features(got["moments"].astype(np.float64), got["acf"].astype(np.float64) if "acf" in got else np.zeros((got["moments"].shape[0], 0, got["moments"].shape[1])),
                      got["ccf"].astype(np.float64) if "ccf" in got else None)


# ---------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", list(CASES))
def test_outputs_within_the_derived_bound_and_near_the_restatement(name):
    n, T, Cn, L, Lx = CASES[name]
    c = case(name)
    got = _got_features(c["got"])
    ref, bound, low = _arrays(c["ref"]), _arrays(c["bound"]), _arrays(c["low"])
    for key, g in _arrays(got).items():
        err, dev_low = np.abs(g - ref[key]), np.abs(low[key].astype(np.float64) - ref[key])
        share = float((err / np.maximum(bound[key], 1e-300)).max()) if err.size else 0.0
        print(f"{name:18s} {key:9s} max err {err.max() if err.size else 0:.3e}  share of bound {share:.3f}  "
              f"restatement {dev_low.max() if err.size else 0:.3e}")
        assert np.isfinite(g).all()
        assert (err <= bound[key]).all(), (name, key, float(err.max()), share)
        if err.size:
            assert err.max() <= 2 * dev_low.max() + 2 * R.U32 * np.abs(ref[key]).max(), (name, key)
    # the set mean: the mean of the float32 features as returned (n 2^-53 relative), hence within the mean bound of the reference's
    flat = got.flat()
    mean = c["got"]["mean"]
    assert np.abs(mean - flat.mean(axis=0)).max() <= n * R.V64 * max(1.0, np.abs(flat).max())
    assert (np.abs(mean - c["ref"].set_mean()) <= c["bound"].flat().mean(axis=0) + n * R.V64 * np.abs(flat).max(axis=0)).all()


def test_ccf_diagonal_is_acf_and_lag_zero_is_one():
    for name in ("mimic", "droughts", "T_limit", "odd_everything", "chunk_boundaries"):
        n, T, Cn, L, Lx = CASES[name]
        got = case(name)["got"]
        idx = np.arange(Cn)
        k = min(L, Lx)
        assert np.array_equal(bits(got["ccf"][:, 1: k + 1, idx, idx]), bits(got["acf"][:, :k])), name
        assert (got["ccf"][:, 0, idx, idx] == 1.0).all(), name          # exact: the two double sums of e^2 agree to T 2^-52
        assert np.abs(got["ccf"]).max() <= 1.0 + R.closed_form_constant(T) * R.U32


@pytest.mark.parametrize("name", ["ecg", "mimic"])
def test_offset_of_1000(name):
    """series + 1000 (exact in float32 on the cases' grid): the normalised features stay within the bound of the UNSHIFTED
    reference plus the mean's term rho = (T + 2) 2^-53 max |x|, which error_bounds takes from the shifted series."""
    n, T, Cn, L, Lx = CASES[name]
    x = case(name)["x"].astype(np.float64)
    shifted = (x + 1000.0).astype(np.float32)
    assert np.array_equal(shifted.astype(np.float64), x + 1000.0)
    got = _got_features(dep_raw(dev(shifted), L, Lx))
    ref, bound = _arrays(case(name)["ref"]), _arrays(R.error_bounds(x, L, Lx, mean_of=shifted))
    for key, g in _arrays(got).items():
        want = ref[key] + 1000.0 if key == "mean" else ref[key]
        tol = bound[key] + (R.U32 * 1000.0 if key == "mean" else 0.0)          # the mean itself is returned in float32 at 1000
        err = np.abs(g - want)
        print(f"{name} +1000 {key:9s} max err {err.max():.3e}  share of bound {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
        assert (err <= tol).all(), (name, key, float(err.max()))


def test_constant_channel():
    n, T, Cn, L, Lx = CASES["mimic"]
    c = case("mimic")
    x = c["x"].copy()
    x[:, :, 7] = 3.3                                                            # not representable: float32(3.3) T times
    x[2, :, 11] = -1000.25
    got = dep_raw(dev(x), L, Lx)
    base = c["got"]
    for s, ch in [(slice(None), 7), (2, 11)]:
        assert (got["moments"][s, ch, 0] == x[s, 0, ch]).all() and not got["moments"][s, ch, 1:].any()
        assert not got["acf"][s, :, ch].any() and not got["ccf"][s, :, ch, :].any() and not got["ccf"][s, :, :, ch].any()
    assert np.isfinite(got["ccf"]).all() and np.isfinite(got["mean"]).all()
    keep = np.ones((n, Cn), dtype=bool)
    keep[:, 7] = False
    keep[2, 11] = False
    assert np.array_equal(bits(got["moments"][keep]), bits(base["moments"][keep]))
    kl = np.broadcast_to(keep[:, None, :], got["acf"].shape)
    assert np.array_equal(bits(got["acf"][kl]), bits(base["acf"][kl]))
    kp = np.broadcast_to((keep[:, :, None] & keep[:, None, :])[:, None], got["ccf"].shape)
    assert np.array_equal(bits(got["ccf"][kp]), bits(base["ccf"][kp]))


# ---------------------------------------------------------------------------------------------- purity and determinism
@pytest.mark.parametrize("name", ["ecg", "mimic", "odd_everything", "chunk_boundaries"])
def test_a_series_alone_and_in_the_batch(name):
    n, T, Cn, L, Lx = CASES[name]
    c = case(name)
    for i in sorted({0, n // 2, n - 1}):
        alone = dep_raw(c["xd"][i: i + 1].contiguous(), L, Lx)
        for key in ("moments", "acf", "ccf"):
            if key in alone:
                assert np.array_equal(bits(alone[key][0]), bits(c["got"][key][i])), (name, i, key)
        assert np.array_equal(bits(alone["mean"]), bits(_got_features(alone).flat()[0]))      # a mean over one series is the series


@pytest.mark.parametrize("name", ["mimic", "droughts"])
def test_any_subset_of_outputs(name):
    n, T, Cn, L, Lx = CASES[name]
    c = case(name)
    for want in (("moments",), ("acf",), ("ccf",), ("mean",), ("acf", "mean"), ("moments", "ccf")):
        got = dep_raw(c["xd"], L, Lx, want=want)
        assert set(got) == set(want)
        for key in want:
            assert np.array_equal(bits(got[key]), bits(c["got"][key])), (name, want, key)


@pytest.mark.parametrize("name", ["ecg", "mimic", "odd_everything", "chunk_boundaries"])
def test_bit_identical_for_every_grid_and_run(name):
    n, T, Cn, L, Lx = CASES[name]
    c = case(name)
    for splits in (None, 1, 2, 7):
        got = dep_raw(c["xd"], L, Lx, splits=splits)
        for key, val in got.items():
            assert np.array_equal(bits(val), bits(c["got"][key])), (name, splits, key)


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """Every refusal the header lists is FD_ERR_ARG with a retrievable message, and nothing is launched: the outputs keep their
    sentinel."""
    from fourierdiffusion_amd import _C
    x = torch.zeros(8, 6, 2, device="cuda")
    mo, ac, cc, me = _guarded((8, 2, 4), torch.float32), _guarded((8, 3, 2), torch.float32), _guarded((8, 2, 2, 2), torch.float32), \
        _guarded((22,), torch.float64)
    h, lib = _C.ctx(x.device), _C.lib()
    need = C.c_size_t(0)
    assert lib.fd_series_dependence_workspace_bytes(h, 8, 6, 2, 3, 1, C.byref(need)) == 0 and need.value > 0
    work = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    p, m, a, c, s, w, nb = x.data_ptr(), mo.data_ptr(), ac.data_ptr(), cc.data_ptr(), me.data_ptr(), work.data_ptr(), need.value
    ws, run = lib.fd_series_dependence_workspace_bytes, lib.fd_series_dependence
    big = 1 << 30
    cases = [
        (lambda: ws(h, 8, 6, 2, 3, 1, None), b"null"),
        (lambda: ws(h, 0, 6, 2, 3, 1, C.byref(need)), b"bad shape"),
        (lambda: ws(h, 8, 0, 2, 0, -1, C.byref(need)), b"bad shape"),
        (lambda: ws(h, 8, 6, 0, 3, 1, C.byref(need)), b"bad shape"),
        (lambda: ws(h, 8, 1025, 2, 3, 1, C.byref(need)), b"at most"),
        (lambda: ws(h, 8, 6, 65, 3, 1, C.byref(need)), b"at most"),
        (lambda: ws(h, 8, 6, 2, -1, 1, C.byref(need)), b"acf_lags=-1"),
        (lambda: ws(h, 8, 6, 2, 6, 1, C.byref(need)), b"acf_lags=6"),
        (lambda: ws(h, 8, 6, 2, 3, -2, C.byref(need)), b"ccf_lags=-2"),
        (lambda: ws(h, 8, 6, 2, 3, 6, C.byref(need)), b"ccf_lags=6"),
        (lambda: ws(h, 8, 1024, 16, 0, 1023, C.byref(need)), b"LDS"),
        (lambda: ws(h, big, 6, 2, 3, 1, C.byref(need)), b"too large"),
        (lambda: ws(h, 1 << 22, 1024, 1, 0, -1, C.byref(need)), b"too large"),          # n T C = 2^32 with n F = 2^24
        (lambda: run(h, None, 8, 6, 2, 3, 1, m, a, c, s, w, nb, None), b"null x"),
        (lambda: run(h, p, 0, 6, 2, 3, 1, m, a, c, s, w, nb, None), b"bad shape"),
        (lambda: run(h, p, 8, 0, 2, 0, -1, m, a, c, s, w, nb, None), b"bad shape"),
        (lambda: run(h, p, 8, 6, 0, 3, 1, m, a, c, s, w, nb, None), b"bad shape"),
        (lambda: run(h, p, 8, 1025, 2, 3, 1, m, a, c, s, w, nb, None), b"at most"),
        (lambda: run(h, p, 8, 6, 65, 3, 1, m, a, c, s, w, nb, None), b"at most"),
        (lambda: run(h, p, 8, 6, 2, -1, 1, m, a, c, s, w, nb, None), b"acf_lags=-1"),
        (lambda: run(h, p, 8, 6, 2, 6, 1, m, a, c, s, w, nb, None), b"acf_lags=6"),
        (lambda: run(h, p, 8, 6, 2, 3, -2, m, a, c, s, w, nb, None), b"ccf_lags=-2"),
        (lambda: run(h, p, 8, 6, 2, 3, 6, m, a, c, s, w, nb, None), b"ccf_lags=6"),
        (lambda: run(h, p, 8, 1024, 16, 0, 1023, m, a, c, s, w, nb, None), b"LDS"),
        (lambda: run(h, p, big, 6, 2, 3, 1, m, a, c, s, w, nb, None), b"too large"),
        (lambda: run(h, p, 8, 6, 2, 3, 1, None, None, None, None, w, nb, None), b"every output is null"),
        (lambda: run(h, p, 8, 6, 2, 0, 1, m, a, c, s, w, nb, None), b"out_acf"),
        (lambda: run(h, p, 8, 6, 2, 3, -1, m, a, c, s, w, nb, None), b"out_ccf"),
        (lambda: run(h, p, 8, 6, 2, 3, 1, m, a, c, s, None, nb, None), b"workspace"),
        (lambda: run(h, p, 8, 6, 2, 3, 1, m, a, c, s, w, nb - 1, None), b"workspace"),
    ]
    for i, (call, text) in enumerate(cases):
        assert call() == -1, i                                                  # FD_ERR_ARG
        assert text in lib.fd_last_error(h), (i, lib.fd_last_error(h))
    torch.cuda.synchronize()
    for buf in (mo, ac, cc, me):
        assert bool((buf == SENTINEL).all())
    assert run(h, p, 8, 6, 2, 3, 1, m, None, None, None, None, 0, None) == 0    # no set mean: no workspace needed
    assert lib.fd_series_dependence(None, p, 8, 6, 2, 3, 1, m, a, c, s, w, nb, None) == -1


def test_wrapper_matches_the_raw_call_and_the_defaults():
    from fourierdiffusion_amd.utils.dependence import series_dependence
    n, T, Cn, L, Lx = CASES["mimic"]
    c = case("mimic")
    res = series_dependence(c["xd"], per_series=("moments", "acf", "ccf"))      # the defaults at (24, 40) are (6, 6)
    assert (res.lags, res.cross_lags) == (L, Lx)
    for key in ("moments", "acf", "ccf"):
        assert np.array_equal(bits(getattr(res, key).cpu().numpy()), bits(c["got"][key]))
    mean = np.concatenate([res.set_mean.moments.cpu().numpy().ravel(), res.set_mean.acf.cpu().numpy().ravel(),
                           res.set_mean.ccf.cpu().numpy().ravel()])
    assert np.array_equal(bits(mean), bits(c["got"]["mean"]))
    small = series_dependence(case("ecg")["x"])                                 # a host array is moved; no ccf for one channel
    assert small.ccf is None and small.set_mean.ccf is None and small.cross_lags == -1 and small.lags == 46
    assert np.array_equal(bits(small.acf.cpu().numpy()), bits(case("ecg")["got"]["acf"]))


# ---------------------------------------------------------------------------------------------- the metric
def _metric_reference(samples, real, L, Lx, suffix=""):
    Cn = real.shape[2]
    fs, fr = R.features(samples, L, Lx), R.features(real, L, Lx)
    out = R.metric_values(R.set_means(fs), R.set_means(fr), Cn, suffix)
    w = R.w2_marginals(fs.acf.reshape(len(samples), -1), fr.acf.reshape(len(real), -1))
    out[f"acf_marginal_wasserstein_mean{suffix}"], out[f"acf_marginal_wasserstein_max{suffix}"] = float(w.mean()), float(w.max())
    return out, max(R.error_bounds(samples, L, Lx).moments[..., 2:].max(), R.error_bounds(real, L, Lx).moments[..., 2:].max())


def test_metric_keys_against_the_reference_arithmetic():
    from fourierdiffusion_amd.sampling.metrics import TemporalDependence
    rs = np.random.RandomState(5)
    real = (np.cumsum(rs.standard_normal((60, 31, 2)), axis=1) * 0.5).astype(np.float32)
    fake = (rs.standard_normal((50, 31, 2)) ** 3).astype(np.float32)
    held = (np.cumsum(rs.standard_normal((20, 31, 2)), axis=1) * 0.5).astype(np.float32)
    metric = TemporalDependence(torch.from_numpy(real), holdout_samples=torch.from_numpy(held), lags=7, cross_lags=3)
    got = metric(torch.from_numpy(fake))
    want, mom_tol = _metric_reference(fake, real, 7, 3)
    want_h, mom_tol_h = _metric_reference(fake, held, 7, 3, "_holdout")
    want.update(want_h)
    want_s, mom_tol_s = _metric_reference(real[:30], real[30:], 7, 3, "_self")
    corr_tol = 2 * R.closed_form_constant(31) * R.U32                           # two set means, each within the acf / ccf bound
    assert sorted(got) == sorted(want)
    for src, ref, mt in ((got, want, max(mom_tol, mom_tol_h)), (metric.baseline_metrics, want_s, mom_tol_s)):
        assert sorted(src) == sorted(ref)
        for key, val in ref.items():
            if "wasserstein" in key:
                # a point moved by at most delta moves W2 by at most delta; 1e-5 relative for the float32 quantile arithmetic of
                # utils/wasserstein.py, which is not under test here
                tol = corr_tol + 1e-5 * val
            else:
                tol = 2 * mt if ("skewness" in key or "kurtosis" in key) else corr_tol
            assert abs(src[key] - val) <= tol, (key, src[key], val)
    same = TemporalDependence(torch.from_numpy(real), lags=7, cross_lags=3)(torch.from_numpy(real))
    assert same and all(v == 0.0 for v in same.values()), same
    one = TemporalDependence(torch.from_numpy(real[:, :, :1].copy()))
    res = one(torch.from_numpy(fake[:, :, :1].copy()))
    assert (one.lags, one.cross_lags) == (7, -1)
    assert not any("ccf" in key for key in list(res) + list(one.baseline_metrics)) and "acf_distance" in res


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


def test_collection_over_the_dependence_config():
    from fourierdiffusion_amd.sampling.metrics import MetricCollection, TemporalDependence
    node, metrics = _yaml_metrics("dependence.yaml")
    default_node, default_metrics = _yaml_metrics("default.yaml")
    assert node["holdout"] is True and [m.func for m in metrics[:-1]] == [m.func for m in default_metrics]
    assert metrics[-1].func is TemporalDependence
    rs = np.random.RandomState(6)
    real = torch.from_numpy(np.cumsum(rs.standard_normal((40, 16, 3)), axis=1).astype(np.float32))
    held = torch.from_numpy(np.cumsum(rs.standard_normal((12, 16, 3)), axis=1).astype(np.float32))
    fake = torch.from_numpy(rs.standard_normal((30, 16, 3)).astype(np.float32))
    plain = MetricCollection(metrics=default_metrics, original_samples=real)(fake)
    with_holdout = MetricCollection(metrics=metrics, original_samples=real, holdout_samples=held)
    res = with_holdout(fake)
    assert list(res) == sorted(res)
    assert {k: res[k] for k in plain} == plain                                  # every other key is as it was
    new = sorted(set(res) - set(plain))
    stems = ["acf_distance", "acf_distance_max", "ccf_distance", "ccf_distance_max", "skewness_distance", "kurtosis_distance",
             "acf_marginal_wasserstein_mean", "acf_marginal_wasserstein_max"]
    assert new == sorted(f"time_{s}{suffix}" for s in stems for suffix in ("", "_holdout", "_self"))
    assert len(with_holdout.metrics_time) == 3 and len(with_holdout.metrics_freq) == 2
    without = MetricCollection(metrics=metrics, original_samples=real)(fake)
    assert not any(k.endswith("_holdout") for k in without) and "time_acf_distance_self" in without
    assert all(np.isfinite(v) for k, v in res.items() if k in new)


def test_ar1_against_iid_noise_through_the_engine():
    """The CPU test's assertions (test_dependence_cpu.py, same seed), now on the engine."""
    from fourierdiffusion_amd.sampling.metrics import TemporalDependence
    rng = np.random.default_rng(2024)
    phi, T, L = 0.8, 100, 25
    real = R.ar1(rng, 800, T, phi).astype(np.float32)
    fake = (rng.standard_normal((400, T, 1)) / np.sqrt(1 - phi * phi)).astype(np.float32)
    metric = TemporalDependence(torch.from_numpy(real), lags=L)
    res, base = metric(torch.from_numpy(fake)), metric.baseline_metrics
    print(res["acf_distance"], base["acf_distance_self"])
    assert res["acf_distance"] > 0.1
    assert res["acf_distance"] > 5 * base["acf_distance_self"]


# ---------------------------------------------------------------------------------------------- dataset scale
def test_ecg_scale():
    from fourierdiffusion_amd.utils.dependence import series_dependence
    n, T = 87554, 187
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.cumsum(torch.randn((n, T, 1), generator=gen, device="cuda"), dim=1) * 0.2 + torch.randn((n, T, 1), generator=gen, device="cuda")
    res = series_dependence(x)
    assert res.lags == 46 and res.acf.shape == (n, 46, 1) and res.moments.shape == (n, 1, 4)
    assert bool(torch.isfinite(res.acf).all()) and bool(torch.isfinite(res.moments).all())
    assert float(res.acf.abs().max()) <= 1.0 + R.closed_form_constant(T) * R.U32
    for got, per_series in ((res.set_mean.acf, res.acf), (res.set_mean.moments, res.moments)):
        per = per_series.double().cpu().numpy()
        want = per.mean(axis=0)
        assert (np.abs(got.cpu().numpy() - want) <= n * R.V64 * np.abs(per).mean(axis=0)).all()
