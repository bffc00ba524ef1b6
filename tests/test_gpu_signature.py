"""GPU: fd_series_signature (csrc/fd_signature.hip), utils/signature.py and sampling/metrics.py SignatureDistance against the float64
reference of tests/signature_ref.py.

Every output is held to the derived bound of signature_ref (nothing tuned): with u = 2^-53, S' segments, l = sum_s ||D[s]||_1 and
b_k = 32 S' u l^k / k! at a level-k entry,
    sig (float32)   |got - ref| <= 2^-24 |ref| + b_k
    sqnorm          |got - ref| <= sum_w (2 |ref_w| b_k + b_k^2) + D u ref_sqnorm
    mean            |got - ref| <= mean_i b_k(i) + (CHUNK + n / CHUNK + 2) u mean_i |ref_i|
The engine's operation order is the reference's (the Horner form, every division a division, nothing contracted), so the constant of
signature_ref stands as derived there.

Bit-level properties: a series' sig and sqnorm do not depend on the batch, its position, the outputs asked for or the grid
(FDIFF_SIG_SPLITS); the set mean is bit-identical for every grid and run; a repeated point changes nothing without the time channel;
a channel of scale 0 gives exact zeros in every word that holds it; nothing is written outside the outputs."""
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

from tests import signature_ref as R
from tests.test_signature_cpu import CASES, DIMS, channel_maps, make_series

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CHUNK = R.CHUNK_SERIES
SENTINEL = -777.0
GUARD = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


class forced_splits:
    def __init__(self, splits):
        self.splits = splits

    def __enter__(self):
        self.old = os.environ.get("FDIFF_SIG_SPLITS")
        if self.splits is not None:
            os.environ["FDIFF_SIG_SPLITS"] = str(self.splits)
        else:
            os.environ.pop("FDIFF_SIG_SPLITS", None)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("FDIFF_SIG_SPLITS", None)
        else:
            os.environ["FDIFF_SIG_SPLITS"] = self.old


def _guarded(size, dtype):
    return torch.full((size + GUARD,), SENTINEL, dtype=dtype, device="cuda")


def sig_raw(x, depth, flags, offset=None, scale=None, want=("sig", "sqnorm"), splits=None):
    """fd_series_signature through the C ABI on an (n, T, C) device tensor.  Every output is pre-filled with a sentinel and followed
    by guard entries, the workspace by guard bytes; returns {name: numpy array} after checking that the guards are intact and the
    body is overwritten.  An output that is not wanted is passed as a null pointer."""
    from fourierdiffusion_amd import _C
    n, T, Cn = x.shape
    d, D = R.signature_dim(Cn, depth, flags)
    shapes = {"sig": (n, D), "sqnorm": (n,), "mean": (D,)}
    bufs = {k: _guarded(int(np.prod(shapes[k])), torch.float32 if k == "sig" else torch.float64) for k in tuple(want) + ("mean",)}
    od = torch.from_numpy(np.asarray(offset, dtype=np.float64)).to("cuda") if offset is not None else None
    sd = torch.from_numpy(np.asarray(scale, dtype=np.float64)).to("cuda") if scale is not None else None
    h, lib = _C.ctx(x.device), _C.lib()
    with forced_splits(splits):
        need = C.c_size_t(0)
        _C.check(lib.fd_series_signature_workspace_bytes(h, n, T, Cn, depth, flags, C.byref(need)), h)
        work = torch.full((need.value + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        _C.check(lib.fd_series_signature(h, x.data_ptr(), n, T, Cn, depth, flags, _C.ptr(od), _C.ptr(sd), _C.ptr(bufs.get("sig")),
                                         _C.ptr(bufs.get("sqnorm")), bufs["mean"].data_ptr(), work.data_ptr(), need.value,
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


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the float64 reference, its bound and ONE engine run with every output, shared (nothing writes to them)."""
    n, T, Cn, depth, flags = CASES[name]
    x = make_series(name)
    off, scl = channel_maps(name)
    inc = R.increments(x, flags, off, scl)
    xd = dev(x)
    return dict(x=x, xd=xd, off=off, scl=scl, inc=inc, ref=R.signature(inc, depth), bound=R.error_bounds(inc, depth),
                got=sig_raw(xd, depth, flags, off, scl))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", list(CASES))
def test_outputs_within_the_derived_bound(name):
    n, T, Cn, depth, flags = CASES[name]
    c = case(name)
    got, ref, bound = c["got"], c["ref"], c["bound"]
    assert got["sig"].shape == (n, DIMS[name])
    checks = {
        "sig": (got["sig"].astype(np.float64), ref, R.U32 * np.abs(ref) + bound),
        "sqnorm": (got["sqnorm"], (ref ** 2).sum(axis=1), R.sqnorm_bound(ref, bound)),
        "mean": (got["mean"], ref.mean(axis=0), R.mean_bound(ref, bound)),
    }
    for key, (g, want, tol) in checks.items():
        err = np.abs(g - want)
        share = float((err / np.maximum(tol, 1e-300)).max())
        print(f"{name:18s} {key:7s} max err {err.max():.3e}  share of bound {share:.4f}")
        assert np.isfinite(g).all()
        assert (err <= tol).all(), (name, key, float(err.max()), share)


def test_level_one_and_the_shuffle_identity_on_the_engine_alone():
    """S_i S_j = S_ij + S_ji on the engine's own float32 output: no reference enters, only the bound of every entry."""
    for name in ("ecg", "lead_lag", "odd", "chunk_boundaries", "mimic"):
        n, T, Cn, depth, flags = CASES[name]
        c = case(name)
        d, D = R.signature_dim(Cn, depth, flags)
        sig, bound = c["got"]["sig"].astype(np.float64), c["bound"]
        l1, l2 = sig[:, :d], sig[:, d: d + d * d].reshape(n, d, d)
        e1 = R.U32 * np.abs(l1) + bound[:, :d]
        e2 = R.U32 * np.abs(l2) + bound[:, d: d + 1, None]
        a1 = np.abs(l1) + e1
        tol = a1[:, :, None] * e1[:, None, :] + a1[:, None, :] * e1[:, :, None] + e2 + e2.transpose(0, 2, 1)
        gap = np.abs(l1[:, :, None] * l1[:, None, :] - l2 - l2.transpose(0, 2, 1))
        assert (gap <= tol).all(), (name, float((gap / np.maximum(tol, 1e-300)).max()))
        assert (np.abs(l1 - c["inc"].sum(axis=1)) <= e1).all(), name


def test_zero_scale_channel_gives_exact_zeros():
    n, T, Cn, depth, flags = CASES["mimic"]
    c = case("mimic")
    assert c["scl"][7] == 0.0
    d, D = R.signature_dim(Cn, depth, flags)
    sig = c["got"]["sig"]
    l1, l2 = sig[:, :d], sig[:, d:].reshape(n, d, d)
    assert not l1[:, 7].any() and not l2[:, 7, :].any() and not l2[:, :, 7].any()
    assert not c["got"]["mean"][7] and not c["got"]["mean"][d:].reshape(d, d)[7].any() and not c["got"]["mean"][d:].reshape(d, d)[:, 7].any()
    keep = np.ones(d, dtype=bool)
    keep[7] = False
    assert (l1[:, keep] != 0).all() and np.count_nonzero(l2[:, keep][:, :, keep]) > 0.99 * n * (d - 1) ** 2


def test_a_repeated_point_changes_nothing_without_the_time_channel():
    for name, flags in (("odd", R.BASEPOINT), ("lead_lag", R.LEAD_LAG), ("lead_lag", 0)):
        n, T, Cn, depth, _ = CASES[name]
        x = case(name)["x"]
        off, scl = channel_maps(name)
        base = sig_raw(dev(x), depth, flags, off, scl)
        for at in (0, T // 2, T - 1):
            twice = np.concatenate([x[:, : at + 1], x[:, at:]], axis=1)
            assert twice.shape[1] == T + 1 and np.array_equal(twice[:, at], twice[:, at + 1])
            got = sig_raw(dev(twice), depth, flags, off, scl)
            for key in ("sig", "sqnorm", "mean"):
                assert np.array_equal(bits(got[key]), bits(base[key])), (name, flags, at, key)


# ---------------------------------------------------------------------------------------------- purity and determinism
@pytest.mark.parametrize("name", ["ecg", "mimic", "lead_lag", "chunk_boundaries", "odd"])
def test_a_series_alone_in_the_batch_and_at_another_position(name):
    n, T, Cn, depth, flags = CASES[name]
    c = case(name)
    for i in sorted({0, n // 2, n - 1}):
        alone = sig_raw(c["xd"][i: i + 1].contiguous(), depth, flags, c["off"], c["scl"])
        for key in ("sig", "sqnorm"):
            assert np.array_equal(bits(alone[key][0]), bits(c["got"][key][i])), (name, i, key)
    turned = sig_raw(c["xd"].flip(0).contiguous(), depth, flags, c["off"], c["scl"])
    for key in ("sig", "sqnorm"):
        assert np.array_equal(bits(turned[key][::-1]), bits(c["got"][key])), (name, key)


@pytest.mark.parametrize("name", ["ecg", "mimic", "feature_cap", "chunk_boundaries", "odd"])
def test_bit_identical_for_every_grid_run_and_set_of_outputs(name):
    n, T, Cn, depth, flags = CASES[name]
    c = case(name)
    for splits in (None, 1, 3, 7):
        for want in (("sig", "sqnorm"), (), ("sqnorm",), ("sig",)):
            if splits in (1, 7) and len(want) == 1:
                continue
            got = sig_raw(c["xd"], depth, flags, c["off"], c["scl"], want=want, splits=splits)
            assert set(got) == set(want) | {"mean"}
            for key, val in got.items():
                assert np.array_equal(bits(val), bits(c["got"][key])), (name, splits, want, key)


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """Every refusal the header lists is FD_ERR_ARG with a retrievable message, and nothing is launched: the outputs keep their
    sentinel."""
    from fourierdiffusion_amd import _C
    x = torch.zeros(8, 6, 2, device="cuda")
    D = 3 + 9 + 27
    sg, sq, me = _guarded(8 * D, torch.float32), _guarded(8, torch.float64), _guarded(D, torch.float64)
    h, lib = _C.ctx(x.device), _C.lib()
    need = C.c_size_t(0)
    assert lib.fd_series_signature_workspace_bytes(h, 8, 6, 2, 3, 4, C.byref(need)) == 0 and need.value > 0
    work = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    p, g, q, m, w, nb = x.data_ptr(), sg.data_ptr(), sq.data_ptr(), me.data_ptr(), work.data_ptr(), need.value
    ws, run = lib.fd_series_signature_workspace_bytes, lib.fd_series_signature
    shapes = [
        ((0, 6, 2, 3, 4), b"bad shape"),
        ((8, 1, 2, 3, 4), b"bad shape"),                      # T = 1: no segment
        ((8, 6, 0, 3, 4), b"bad shape"),
        ((8, 1025, 2, 3, 4), b"at most"),
        ((8, 6, 65, 1, 4), b"at most"),
        ((8, 6, 2, 0, 4), b"depth=0"),
        ((8, 6, 2, 7, 4), b"depth=7"),
        ((8, 6, 2, 3, 8), b"flags=8"),
        ((8, 6, 2, 3, -1), b"flags=-1"),
        ((8, 6, 64, 3, 4), b"more than 8192 features"),       # 65 + 65^2 + 65^3
        ((8, 6, 45, 2, 6), b"more than 8192 features"),       # 91 + 91^2 = 8372
        ((8, 6, 4, 6, 0), None),                               # 4 + ... + 4^6 = 5460: fine
        ((8, 6, 5, 6, 0), b"more than 8192 features"),        # 5 + ... + 5^6 = 19530
        ((1 << 30, 6, 2, 3, 4), b"too large"),
        ((1 << 22, 1024, 1, 1, 0), b"too large"),             # n T C = 2^32 with n D = 2^22
    ]
    for i, (shape, text) in enumerate(shapes):
        if text is None:
            assert ws(h, *shape, C.byref(need)) == 0, i
            continue
        for call in (lambda: ws(h, *shape, C.byref(need)), lambda: run(h, p, *shape, None, None, g, q, m, w, nb, None)):
            assert call() == -1, (i, shape)                                         # FD_ERR_ARG
            assert text in lib.fd_last_error(h), (i, lib.fd_last_error(h))
    others = [
        (lambda: ws(h, 8, 6, 2, 3, 4, None), b"null"),
        (lambda: run(h, None, 8, 6, 2, 3, 4, None, None, g, q, m, w, nb, None), b"null x"),
        (lambda: run(h, p, 8, 6, 2, 3, 4, None, None, g, q, None, w, nb, None), b"null mean"),
        (lambda: run(h, p, 8, 6, 2, 3, 4, None, None, g, q, m, None, nb, None), b"workspace"),
        (lambda: run(h, p, 8, 6, 2, 3, 4, None, None, g, q, m, w, nb - 1, None), b"workspace"),
    ]
    for i, (call, text) in enumerate(others):
        assert call() == -1, i
        assert text in lib.fd_last_error(h), (i, lib.fd_last_error(h))
    torch.cuda.synchronize()
    for buf in (sg, sq, me):
        assert bool((buf == SENTINEL).all())
    assert lib.fd_series_signature(None, p, 8, 6, 2, 3, 4, None, None, g, q, m, w, nb, None) == -1
    assert run(h, p, 8, 6, 2, 3, 4, None, None, None, None, m, w, nb, None) == 0     # the set mean alone
    torch.cuda.synchronize()
    assert bool((me[:D] != SENTINEL).all()) and bool((me[D:] == SENTINEL).all()) and bool((sg == SENTINEL).all())
    assert abs(float(me[2]) - 1.0) <= 8 * R.V64 and not bool(me[:2].any())                            # a path that only moves in time


def test_wrapper_matches_the_raw_call():
    from fourierdiffusion_amd.utils.signature import series_signature
    n, T, Cn, depth, flags = CASES["lead_lag"]
    c = case("lead_lag")
    res = series_signature(c["xd"], depth, time_augment=True, lead_lag=True, per_series=("sig", "sqnorm"))
    assert (res.d, res.depth, res.n) == (7, 3, n) and res.levels == R.level_slices(7, 3)
    for key in ("sig", "sqnorm", "mean"):
        assert np.array_equal(bits(getattr(res, key).cpu().numpy()), bits(c["got"][key])), key
    assert res.sqnorm_sum == float(c["got"]["sqnorm"].sum())
    bare = series_signature(c["x"], depth, lead_lag=True)                        # a host array is moved; nothing per series by default
    assert bare.sig is None and bare.sqnorm is None and np.array_equal(bits(bare.mean.cpu().numpy()), bits(c["got"]["mean"]))
    # path_scale multiplies the channel scales: level k of the words without the time letter scales by path_scale^k
    n, T, Cn, depth, flags = CASES["odd"]
    c = case("odd")
    scaled = series_signature(c["xd"], depth, time_augment=False, basepoint=True, channel_offset=c["off"], channel_scale=c["scl"],
                              path_scale=2.0, per_series=("sig",))
    raw = sig_raw(c["xd"], depth, flags, c["off"], 2.0 * c["scl"])
    assert np.array_equal(bits(scaled.sig.cpu().numpy()), bits(raw["sig"]))
    for k, sl in enumerate(R.level_slices(Cn, depth), start=1):                  # powers of two: exact
        assert np.array_equal(bits(raw["sig"][:, sl]), bits(c["got"]["sig"][:, sl] * np.float32(2.0 ** k)))


# ---------------------------------------------------------------------------------------------- the metric
def _norm(v):
    return float(np.sqrt((v ** 2).sum()))


def _reference_set(x, off, scl, depth, flags):
    inc = R.increments(x, flags, off, scl)
    ref, bound = R.signature(inc, depth), R.error_bounds(inc, depth)
    return dict(ref=ref, mean=ref.mean(axis=0), e_mean=R.mean_bound(ref, bound), sq=(ref ** 2).sum(axis=1).sum(),
                e_sq=R.sqnorm_bound(ref, bound).sum(), n=len(x))


def _distance_tolerances(a, b, d, depth):
    """The entry bounds carried through the three scalars.  ||ma - mb|| moves by at most ||ea|| + ||eb|| (per level too); an own term
    (n^2 ||m||^2 - sum sq) / (n (n - 1)) by (n^2 (2 ||m|| ||e|| + ||e||^2) + e_sq) / (n (n - 1)); the cross term 2 <ma, mb> by
    2 (||ma|| ||eb|| + ||mb|| ||ea|| + ||ea|| ||eb||); the host's float64 arithmetic on D terms by 8 D u of the terms' magnitudes."""
    D = len(a["mean"])
    w1 = _norm(a["e_mean"]) + _norm(b["e_mean"]) + 8 * D * R.V64 * (_norm(a["mean"]) + _norm(b["mean"]))
    levels = [_norm(a["e_mean"][sl]) + _norm(b["e_mean"][sl]) + 8 * D * R.V64 * (_norm(a["mean"][sl]) + _norm(b["mean"][sl]))
              for sl in R.level_slices(d, depth)]
    mmd, size = 0.0, 0.0
    for s in (a, b):
        if s["n"] > 1:
            m, e, n = _norm(s["mean"]), _norm(s["e_mean"]), s["n"]
            mmd += (n * n * (2 * m * e + e * e) + s["e_sq"]) / (n * (n - 1))
            size += (n * n * m * m + s["sq"]) / (n * (n - 1))
    ma, mb, ea, eb = _norm(a["mean"]), _norm(b["mean"]), _norm(a["e_mean"]), _norm(b["e_mean"])
    mmd += 2 * (ma * eb + mb * ea + ea * eb)
    size += 2 * ma * mb
    return w1, levels, mmd + 8 * D * R.V64 * size


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


def test_wrapper_distance_and_metric_against_the_reference_pipeline():
    from fourierdiffusion_amd.sampling.metrics import MetricCollection, SignatureDistance
    from fourierdiffusion_amd.utils.signature import expected_signature_distance, series_signature
    rs = np.random.RandomState(11)
    real = np.cumsum(rs.standard_normal((40, 16, 2)), axis=1).astype(np.float32)
    fake = (np.cumsum(rs.standard_normal((40, 16, 2)), axis=1) * 1.2 + 0.3).astype(np.float32)
    held = np.cumsum(rs.standard_normal((13, 16, 2)), axis=1).astype(np.float32)
    depth, flags, d = 3, R.TIME, 3
    flat = real.astype(np.float64).reshape(-1, 2)
    off, scl = flat.mean(axis=0), 1.0 / flat.std(axis=0)
    sets = {k: _reference_set(v, off, scl, depth, flags) for k, v in
            dict(real=real, fake=fake, held=held, fold0=real[:20], fold1=real[20:]).items()}

    def check(got, a, b, suffix=""):
        want = R.expected_signature_distance(sets[a]["ref"], sets[b]["ref"], d, depth)
        t_w1, t_levels, t_mmd = _distance_tolerances(sets[a], sets[b], d, depth)
        assert abs(got[f"sig_w1{suffix}"] - want["sig_w1"]) <= t_w1, (a, b, got, want)
        assert len(got[f"sig_w1_levels{suffix}"]) == depth
        for g, w, t in zip(got[f"sig_w1_levels{suffix}"], want["sig_w1_levels"], t_levels):
            assert abs(g - w) <= t, (a, b, got, want)
        assert abs(got[f"sig_mmd2{suffix}"] - want["sig_mmd2"]) <= t_mmd, (a, b, got, want, t_mmd)

    # the wrapper and the distance
    sa = series_signature(fake, depth, channel_offset=off, channel_scale=scl, per_series=("sig", "sqnorm"))
    sb = series_signature(real, depth, channel_offset=off, channel_scale=scl)
    check(expected_signature_distance(sa, sb), "fake", "real")
    one = series_signature(fake[:1], depth, channel_offset=off, channel_scale=scl)
    sets["one"] = _reference_set(fake[:1], off, scl, depth, flags)
    check(expected_signature_distance(one, sb), "one", "real")
    # the metric, alone and through the collection of cmd/conf/metrics/signature.yaml
    metric = SignatureDistance(torch.from_numpy(real), holdout_samples=torch.from_numpy(held), depth=depth)
    assert np.array_equal(metric.channel_offset, off) and np.array_equal(metric.channel_scale, scl)
    got = metric(torch.from_numpy(fake))
    assert sorted(got) == sorted(f"{k}{s}" for k in ("sig_w1", "sig_w1_levels", "sig_mmd2") for s in ("", "_holdout"))
    check(got, "fake", "real")
    check(got, "fake", "held", "_holdout")
    base = metric.baseline_metrics
    assert sorted(base) == ["sig_mmd2_self", "sig_w1_levels_self", "sig_w1_self"]
    check(base, "fold0", "fold1", "_self")
    same = SignatureDistance(torch.from_numpy(real), depth=depth)(torch.from_numpy(real))
    assert same["sig_w1"] == 0.0 and same["sig_w1_levels"] == [0.0] * depth
    node, metrics = _yaml_metrics("signature.yaml")
    default_node, default_metrics = _yaml_metrics("default.yaml")
    assert node["holdout"] is True and [m.func for m in metrics[:-1]] == [m.func for m in default_metrics]
    assert metrics[-1].func is SignatureDistance
    plain = MetricCollection(metrics=default_metrics, original_samples=torch.from_numpy(real))(torch.from_numpy(fake))
    collection = MetricCollection(metrics=metrics, original_samples=torch.from_numpy(real), holdout_samples=torch.from_numpy(held))
    res = collection(torch.from_numpy(fake))
    assert list(res) == sorted(res) and {k: res[k] for k in plain} == plain      # every other key is as it was
    new = sorted(set(res) - set(plain))
    assert new == sorted(f"time_{k}{s}" for k in ("sig_w1", "sig_w1_levels", "sig_mmd2") for s in ("", "_holdout", "_self"))
    assert len(collection.metrics_time) == 3 and len(collection.metrics_freq) == 2
    assert {k[5:]: res[k] for k in new if not k.endswith("_self")} == got and {k[5:]: res[k] for k in new if k.endswith("_self")} == base
    # a constant channel: scale 0, exact zeros, nothing else moves
    flatline = real.copy()
    flatline[:, :, 1] = 2.5
    m0 = SignatureDistance(torch.from_numpy(flatline), depth=2)
    assert m0.channel_scale[1] == 0.0 and np.isfinite(list(m0(torch.from_numpy(fake)).values())[0])
    mean = m0._real.mean.cpu().numpy()
    assert mean[1] == 0.0 and not mean[3:].reshape(3, 3)[1].any() and not mean[3:].reshape(3, 3)[:, 1].any() and mean[0] != 0.0


def test_reversed_sawtooth_through_the_engine():
    """tests/test_signature_cpu.py asserts the same ordering of the float64 reference alone (same seed and shapes).  The marginals,
    the autocorrelation and the spectrum of the reversed set are those of the real one; the expected signature is not."""
    from fourierdiffusion_amd.sampling.metrics import SignatureDistance
    rng = np.random.default_rng(2025)
    real, fake = R.sawtooth(rng, 400, 64), R.sawtooth(rng, 200, 64)[:, ::-1].copy()
    metric = SignatureDistance(torch.from_numpy(real), depth=4)
    res, base = metric(torch.from_numpy(fake)), metric.baseline_metrics
    print(f"sig_w1 reversed {res['sig_w1']:.4f}  self {base['sig_w1_self']:.4f}")
    assert res["sig_w1"] > base["sig_w1_self"]


# ---------------------------------------------------------------------------------------------- dataset scale
def test_ecg_scale():
    from fourierdiffusion_amd.utils.signature import series_signature
    n, T = 87554, 187
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.cumsum(torch.randn((n, T, 1), generator=gen, device="cuda"), dim=1) * 0.1
    res = series_signature(x, 4, per_series=("sig", "sqnorm"))
    assert res.sig.shape == (n, 30) and res.sqnorm.shape == (n,) and res.mean.shape == (30,)
    sig = res.sig.double().cpu().numpy()
    assert np.isfinite(sig).all()
    # the mean of the double states against the mean of their float32 roundings, both summed in float64
    got = res.mean.cpu().numpy()
    assert (np.abs(got - sig.mean(axis=0)) <= (R.U32 + n * R.V64) * np.abs(sig).mean(axis=0)).all()
    sq = res.sqnorm.cpu().numpy()
    assert (np.abs(sq - (sig ** 2).sum(axis=1)) <= (2 * R.U32 + R.U32 ** 2 + 32 * R.V64) * sq).all()
    # level 1 is the total increment; the time letter's is exactly 1 up to the 186 additions of 1 / 186
    xh = x[:, :, 0].double().cpu().numpy()
    assert (np.abs(sig[:, 0] - (xh[:, -1] - xh[:, 0])) <= R.U32 * np.abs(sig[:, 0]) + 2 * T * R.V64 * np.abs(np.diff(xh, axis=1)).sum(axis=1)).all()
    assert np.abs(sig[:, 1] - 1.0).max() <= R.U32
