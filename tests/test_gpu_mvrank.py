"""GPU: the multivariate rank histograms (an extension, not in the reference) -- fd_multivariate_ranks against the float64
restatement of tests/mvrank_ref.py at the tile edges, masks of every kind, ties, K = 1023, NaN poisoning, determinism, the C ABI's
argument errors, and the Python layer of sampling/forecast.py and cmd/impute.py.

The integer kinds (average, band_depth, dominance) must equal the restatement exactly: prerank, below, equal and hidden.
mst: every pre-rank within (m - 2) (d + 4) 2^-52 of the largest edge of its series (m - 2 edges, each the root of a sum of d squares
carried in double on both sides); below and equal exactly, on inputs whose reference gaps |L_j - L_0| exceed 1e-9 of the largest
length -- that is asserted first, for every series, so that none is left out.  One kind of series cannot meet that: with a single
hidden entry the points are collinear, every interior point left out gives the same length max - min, and the ranks rest on exact
ties between sums of rounded terms; such a series is held to the pre-rank bound and to the interval of ranks that bound allows.
Every comparison logs its largest error (gpu_util.log_line) before it asserts."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import mvrank_ref as R
from tests.gpu_util import dev, log_line

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KIND = {"average": 0, "band_depth": 1, "dominance": 2, "mst": 3}
INTEGER = ("average", "band_depth", "dominance")


def _ranks_c(kind, x, y, mask):
    """fd_multivariate_ranks on numpy x (n,K,T,C), y (n,T,C); mask numpy bool (n,T,C) or (T,C), True = observed.  The workspace
    and the outputs start from junk."""
    from fourierdiffusion_amd import _C
    xd, yd = dev(x), dev(y)
    n, K, T, Cn = x.shape
    h, L = _C.ctx(xd.device), _C.lib()
    need = C.c_size_t(0)
    _C.check(L.fd_multivariate_ranks_workspace_bytes(h, KIND[kind], n, K, T, Cn, C.byref(need)), h)
    work = torch.full((max(1, need.value),), 0xA5, dtype=torch.uint8, device=xd.device)
    m8 = torch.from_numpy(np.ascontiguousarray(mask)).to(torch.uint8).cuda()
    pre = torch.full((n, K + 1), 7.0, dtype=torch.float64, device=xd.device)
    below, equal, hidden = (torch.full((n,), -7, dtype=torch.int32, device=xd.device) for _ in range(3))
    _C.check(L.fd_multivariate_ranks(h, KIND[kind], xd.data_ptr(), yd.data_ptr(), m8.data_ptr(), int(mask.ndim == 3), n, K, T, Cn,
                                     pre.data_ptr(), below.data_ptr(), equal.data_ptr(), hidden.data_ptr(), work.data_ptr(),
                                     need.value, _C.stream_of(xd)), h)
    return dict(prerank=pre.cpu().numpy(), below=below.cpu().numpy(), equal=equal.cpu().numpy(), hidden=hidden.cpu().numpy())


def _check(tag, kind, x, y, mask, candidates=None):
    """One kernel call against the restatement; returns the kernel's outputs."""
    ref = R.multivariate_ranks(x, y, mask, kind, candidates)
    n, K = x.shape[:2]
    m = K + 1
    clean = ref["below"] != -1
    got = _ranks_c(kind, x, y, mask)
    assert np.array_equal(got["hidden"], ref["hidden"]), (tag, kind)
    if kind != "mst":
        assert np.array_equal(got["prerank"], ref["prerank"]), (tag, kind)
        assert np.array_equal(got["below"], ref["below"]) and np.array_equal(got["equal"], ref["equal"]), (tag, kind)
        return got
    # a series with ONE hidden entry is collinear: leaving out any interior point gives the same length, max - min, so its ranks
    # rest on exact ties of sums of rounded terms; it is held to the pre-rank bound and to the rank interval the bound allows.
    # Every other series must have reference gaps above 1e-9: asserted first, none is left out.
    strict = clean & (ref["hidden"] != 1)
    ranked = strict & (ref["hidden"] > 0)
    if candidates is None and ranked.any() and K > 1:
        gap = float(R.mst_relative_gaps(ref["prerank"][ranked]).min())
        log_line(f"[mvrank] {tag} mst: smallest reference gap {gap:.3e} of the largest length")
        assert gap > 1e-9, (tag, gap)
    cols = list(range(m)) if candidates is None else list(candidates)
    bound = (m - 2) * (ref["hidden"] + 4) * 2.0 ** -52 * ref["edge"]
    err = np.zeros(n)
    err[clean] = np.abs(got["prerank"][clean][:, cols] - ref["prerank"][clean][:, cols]).max(axis=1)
    worst = float((err[clean] / np.maximum(bound[clean], 1e-300)).max()) if m > 2 and clean.any() else 0.0
    log_line(f"[mvrank] {tag} mst: largest |L - ref| {float(err.max()):.3e}, {worst:.3f} of the bound")
    assert (err <= bound).all(), (tag, err, bound)
    assert np.isnan(got["prerank"][~clean]).all()
    if candidates is not None:
        return got
    keep = strict | ~clean
    assert np.array_equal(got["below"][keep], ref["below"][keep]) and np.array_equal(got["equal"][keep], ref["equal"][keep]), tag
    for s in np.nonzero(clean & (ref["hidden"] == 1))[0]:
        L = ref["prerank"][s]
        lo, hi = int((L[1:] < L[0] - 2 * bound[s]).sum()), int((L[1:] <= L[0] + 2 * bound[s]).sum())
        assert lo <= got["below"][s] and got["below"][s] + got["equal"][s] <= hi, (tag, s, lo, hi, got["below"][s], got["equal"][s])
    return got


def _data(n, K, T, Cn, seed, grid=False):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, K, T, Cn) * rs.uniform(0.2, 3.0, (1, 1, T, Cn)) + rs.randn(1, 1, T, Cn)
    y = rs.randn(n, T, Cn)
    if grid:
        x, y = np.round(x * 2) / 2, np.round(y * 2) / 2     # a 0.5 grid: ties dominate
    return x.astype(np.float32), y.astype(np.float32), rs


def _mask(name, n, T, Cn, rs):
    if name == "shared":
        m = rs.rand(T, Cn) < 0.4
        m[rs.randint(T), rs.randint(Cn)] = False             # at least one hidden entry
        return m
    if name == "forecast":
        m = np.ones((T, Cn), bool)
        m[-max(1, T // 4):] = False
        return m
    m = rs.rand(n, T, Cn) < 0.5                              # per series; series 0 keeps a hidden entry, one series gets none
    m[:, 0, 0] = False
    if n > 1:
        m[n // 2] = True
    return m


SHAPES = [(1, 1), (3, 1), (21, 3), (13, 5), (65, 2)]          # T*C = 1, 3, 63, 65, 130
MASKS = ("shared", "per_series", "forecast")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K", [1, 2, 18, 63, 64, 65])
def test_all_kinds_vs_float64(K, shape):
    """Tile edges: m = K + 1 in {2, 3, 19, 64, 65, 66} against the 64-row tiles, T*C against the 8-entry and 64-entry chunks;
    n = 1 and n = 5 and the three mask kinds alternate over the cases (n = 5 with a per-series mask has an all-observed series)."""
    T, Cn = shape
    case = SHAPES.index(shape) + K
    n = 5 if case % 2 else 1
    name = MASKS[case % 3]
    x, y, rs = _data(n, K, T, Cn, seed=100 * K + T)
    mask = _mask(name, n, T, Cn, rs)
    for kind in R.KINDS:
        _check(f"n={n} K={K} T={T} C={Cn} {name}", kind, x, y, mask)


@pytest.mark.parametrize("K", [2, 18, 65])
def test_ties_on_a_coarse_grid(K):
    """Data on a 0.5 grid: most entries tie.  The integer kinds only: equal minimum-spanning-tree lengths are equal up to rounding,
    which is no exact test."""
    n, T, Cn = 5, 13, 5
    x, y, rs = _data(n, K, T, Cn, seed=K, grid=True)
    x[0, :, 2, 1] = y[0, 2, 1]                               # a constant ensemble equal to the truth at one entry
    x[1] = y[1][None]                                        # a whole series of ties: every pre-rank equal
    for name in ("per_series", "forecast"):
        mask = _mask(name, n, T, Cn, rs)
        for kind in INTEGER:
            got = _check(f"grid K={K} {name}", kind, x, y, mask)
            assert (got["equal"] > 0).any()
            if name == "forecast":
                assert got["below"][1] == 0 and got["equal"][1] == K


def test_largest_ensemble():
    """K = 1023 (m = 1024, sixteen row tiles, four keys per thread in Prim), n = 1, T*C = 3; mst at 8 candidates."""
    x, y, _ = _data(1, 1023, 3, 1, seed=9)
    mask = np.zeros((3, 1), bool)
    for kind in INTEGER:
        _check("K=1023", kind, x, y, mask)
    _check("K=1023", "mst", x, y, mask, candidates=[0, 1, 63, 64, 511, 512, 1000, 1023])


@functools.lru_cache(maxsize=None)
def _edge_case():
    n, K, T, Cn = 5, 20, 30, 5
    x, y, rs = _data(n, K, T, Cn, seed=8)
    mask = rs.rand(n, T, Cn) < 0.5
    mask[1] = True                                           # series 1: all observed
    clean = {kind: _ranks_c(kind, x, y, mask) for kind in R.KINDS}
    return x, y, mask, clean


@pytest.mark.parametrize("kind", R.KINDS)
def test_nan_poisons_one_series_and_observed_nans_do_nothing(kind):
    x, y, mask, clean = _edge_case()
    n, K = x.shape[:2]
    base = clean[kind]
    assert base["below"][1] == 0 and base["equal"][1] == K and base["hidden"][1] == 0
    assert (base["prerank"][1] == base["prerank"][1, 0]).all()
    rs = np.random.RandomState(1)
    xo, yo = x.copy(), y.copy()                              # NaN at observed entries, every series, truth and members
    xo[np.broadcast_to(mask[:, None], x.shape) & (rs.rand(*x.shape) < 0.2)] = np.nan
    yo[mask & (rs.rand(*y.shape) < 0.2)] = np.nan
    assert np.isnan(xo).any() and np.isnan(yo).any()
    got = _ranks_c(kind, xo, yo, mask)
    for key in ("prerank", "below", "equal", "hidden"):
        assert got[key].tobytes() == base[key].tobytes(), (kind, key)
    others = [i for i in range(n) if i != 3]
    for where in ("member", "truth"):                        # NaN at a hidden entry of series 3
        xh, yh = x.copy(), y.copy()
        t, c = np.argwhere(~mask[3])[-1]
        if where == "member":
            xh[3, K // 2, t, c] = np.nan
        else:
            yh[3, t, c] = np.nan
        got = _check(f"nan in the {where}", kind, xh, yh, mask)
        assert got["below"][3] == -1 and got["equal"][3] == -1
        assert np.isnan(got["prerank"][3]).all() if kind == "mst" else (got["prerank"][3] == -1).all()
        for key in ("prerank", "below", "equal", "hidden"):
            assert got[key][others].tobytes() == base[key][others].tobytes(), (kind, where, key)


@pytest.mark.parametrize("kind", R.KINDS)
def test_bit_reproducible_and_independent_of_batch_position(kind):
    K, T, Cn = 70, 50, 3                                     # two row tiles, 250 entries: several splits of the entry chunks
    x, y, rs = _data(5, K, T, Cn, seed=12)
    mask = rs.rand(5, T, Cn) < 0.5
    a, b = _ranks_c(kind, x, y, mask), _ranks_c(kind, x, y, mask)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), (kind, key)
    alone = _ranks_c(kind, x[:1], y[:1], mask[:1])
    for pos in (0, 3):
        perm = [i for i in range(1, 5)]
        perm.insert(pos, 0)                                  # series 0 at position pos
        got = _ranks_c(kind, x[perm], y[perm], mask[perm])
        for key in got:
            assert got[key][pos:pos + 1].tobytes() == alone[key].tobytes(), (kind, key, pos)
    shared = _ranks_c(kind, x[:1], y[:1], mask[0])           # and the shared-mask path reads the same mask
    for key in shared:
        assert shared[key].tobytes() == alone[key].tobytes(), (kind, key)


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_argument_errors():
    from fourierdiffusion_amd import _C
    n, K, T, Cn = 2, 4, 6, 3
    x, y = torch.zeros(n, K, T, Cn, device="cuda"), torch.zeros(n, T, Cn, device="cuda")
    m8 = torch.zeros(n, T, Cn, dtype=torch.uint8, device="cuda")
    pre = torch.zeros(n, K + 1, dtype=torch.float64, device="cuda")
    ob, oe, oh = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    h, L = _C.ctx(x.device), _C.lib()
    needs = []
    for kind in range(4):
        need = C.c_size_t(0)
        assert L.fd_multivariate_ranks_workspace_bytes(h, kind, n, K, T, Cn, C.byref(need)) == 0 and need.value > 0
        needs.append(need.value)
    work = torch.zeros(max(needs), dtype=torch.uint8, device="cuda")
    need = C.c_size_t(0)

    def ranks(**k):
        a = dict(kind=0, x=x.data_ptr(), y=y.data_ptr(), m=m8.data_ptr(), n=n, K=K, T=T, C=Cn, pre=pre.data_ptr(), below=ob.data_ptr(),
                 equal=oe.data_ptr(), hid=oh.data_ptr(), work=work.data_ptr())
        a.update(k)
        a.setdefault("bytes", needs[a["kind"]] if 0 <= a["kind"] < 4 else max(needs))
        return L.fd_multivariate_ranks(h, a["kind"], a["x"], a["y"], a["m"], 1, a["n"], a["K"], a["T"], a["C"], a["pre"], a["below"],
                                       a["equal"], a["hid"], a["work"], a["bytes"], None)

    def size(kind=0, n=n, K=K, T=T, Cn=Cn, out=C.byref(need)):
        return L.fd_multivariate_ranks_workspace_bytes(h, kind, n, K, T, Cn, out)

    cases = [
        (lambda: size(out=None), b"null"), (lambda: size(kind=4), b"kind=4"), (lambda: size(kind=-1), b"kind=-1"),
        (lambda: size(n=0), b"bad shape"), (lambda: size(T=0), b"bad shape"), (lambda: size(Cn=-2), b"bad shape"),
        (lambda: size(K=0), b"K=0"), (lambda: size(K=1024), b"K=1024"), (lambda: size(T=1 << 30, Cn=4), b"too large"),
        (lambda: size(kind=3, n=1 << 22, K=1023), b"too large"),
        (lambda: ranks(x=None), b"null"), (lambda: ranks(y=None), b"null"), (lambda: ranks(m=None), b"null"),
        (lambda: ranks(pre=None), b"null"), (lambda: ranks(below=None), b"null"), (lambda: ranks(equal=None), b"null"),
        (lambda: ranks(work=None), b"null"),
        (lambda: ranks(kind=4), b"kind=4"), (lambda: ranks(kind=-1), b"kind=-1"),
        (lambda: ranks(n=0), b"bad shape"), (lambda: ranks(T=-1), b"bad shape"), (lambda: ranks(C=0), b"bad shape"),
        (lambda: ranks(K=0), b"K=0"), (lambda: ranks(K=1024), b"K=1024"),
    ]
    for kind in range(4):
        cases += [(lambda kind=kind: ranks(kind=kind, bytes=needs[kind] - 1), b"workspace"),
                  (lambda kind=kind: ranks(kind=kind, bytes=0), b"workspace")]
    for i, (call, needle) in enumerate(cases):
        assert call() == -1, i
        assert needle in L.fd_last_error(h), (i, L.fd_last_error(h))
    torch.cuda.synchronize()
    assert (oh.cpu().numpy() == -7).all()                    # no refused call wrote anything
    for kind in range(4):                                    # the good arguments, with and without the hidden counts
        assert ranks(kind=kind) == 0 and ranks(kind=kind, hid=None) == 0
    assert L.fd_multivariate_ranks(None, 0, x.data_ptr(), y.data_ptr(), m8.data_ptr(), 1, n, K, T, Cn, pre.data_ptr(), ob.data_ptr(),
                                   oe.data_ptr(), oh.data_ptr(), work.data_ptr(), max(needs), None) == -1     # no context: code only
    assert L.fd_multivariate_ranks_workspace_bytes(None, 0, n, K, T, Cn, C.byref(need)) == -1
    torch.cuda.synchronize()
    assert (oh.cpu().numpy() == T * Cn).all() and (ob.cpu().numpy() == 0).all() and (oe.cpu().numpy() == K).all()


# ------------------------------------------------------------------------------------------------ Python layer
@functools.lru_cache(maxsize=None)
def _experiment():
    truth, x, shuffled = R.coherent_and_shuffled(n=64)
    return torch.from_numpy(truth), torch.from_numpy(x), torch.from_numpy(shuffled), torch.zeros(truth.shape[1:], dtype=torch.bool)


def test_coherent_and_shuffled_histograms_match_the_restatement():
    from fourierdiffusion_amd.sampling import forecast as F
    truth, x, shuffled, mask = _experiment()
    for name, v in (("coherent", x), ("shuffled", shuffled)):
        got = F.multivariate_rank_histogram(v, truth, mask, F.PRERANKS)
        assert tuple(got) == F.PRERANKS
        for kind in F.PRERANKS:
            ref = R.multivariate_ranks(v.numpy(), truth.numpy(), mask.numpy(), kind)
            if kind == "mst":
                assert R.mst_relative_gaps(ref["prerank"]).min() > 1e-9
            hist = R.rank_histogram(ref["below"], ref["equal"], ref["hidden"], 19)
            err = float(np.abs(got[kind]["histogram"].numpy() - hist).max())
            log_line(f"[mvrank] {name} {kind}: reliability index {got[kind]['reliability_index']:.4f}, histogram error {err:.1e}")
            assert err <= 1e-12, (name, kind, err)
            assert abs(got[kind]["reliability_index"] - R.reliability_index(hist)) <= 1e-12
            assert got[kind]["n_series_ranked"] == 64 and got[kind]["histogram"].dtype == torch.float64
    two = F.multivariate_rank_histogram(x, truth, mask)     # the default kinds
    assert tuple(two) == ("average", "band_depth")


def test_chunked_equals_one_chunk_scale_and_unranked_series(monkeypatch):
    from fourierdiffusion_amd.sampling import forecast as F
    truth, x, _, _ = _experiment()
    truth, x = truth[:8], x[:8]
    mask = torch.from_numpy(np.random.RandomState(2).rand(*truth.shape) < 0.5)            # per series: the chunks slice it
    mask[5] = True                                                                         # one series without a hidden entry
    scale = torch.tensor([1.0, 3.0])
    one = {k: F.multivariate_rank_counts(x, truth, mask, k, scale=scale) for k in F.PRERANKS}
    plain = {k: F.multivariate_rank_counts(x, truth, mask, k) for k in F.PRERANKS}
    hists = F.multivariate_rank_histogram(x, truth, mask, F.PRERANKS, scale=scale)
    monkeypatch.setattr(F, "CHUNK_BYTES", 3 * 4 * x[0].numel())                            # 3 series per call: 3 + 3 + 2
    for k in F.PRERANKS:
        three = F.multivariate_rank_counts(x, truth, mask, k, scale=scale)
        for key in ("prerank", "below", "equal", "hidden"):
            assert torch.equal(getattr(one[k], key), getattr(three, key)), (k, key)
        assert one[k].prerank.dtype == torch.float64 and tuple(one[k].prerank.shape) == (8, 20)
        assert one[k].below.dtype == torch.int32 and tuple(one[k].below.shape) == (8,)
        assert int(one[k].hidden[5]) == 0 and int(one[k].below[5]) == 0 and int(one[k].equal[5]) == 19
        assert hists[k]["n_series_ranked"] == 7
        if k == "mst":                                                                     # the scale reaches the distances ...
            assert not torch.equal(one[k].prerank, plain[k].prerank)
            by_hand = F.multivariate_rank_counts((x.double() / scale).float(), (truth.double() / scale).float(), mask, k)
            assert torch.equal(by_hand.prerank, one[k].prerank)
        else:                                                                              # ... and cannot move an order
            assert torch.equal(one[k].prerank, plain[k].prerank)
    hists3 = F.multivariate_rank_histogram(x, truth, mask, F.PRERANKS, scale=scale)
    for k in F.PRERANKS:
        assert torch.equal(hists[k]["histogram"], hists3[k]["histogram"])
    xn = x.clone()
    xn[2, 5][~mask[2]] = float("nan")                                                      # NaN data is not dropped silently
    bad = F.multivariate_rank_histogram(xn, truth, mask, ("average", "mst"))
    assert all(np.isnan(v["reliability_index"]) and torch.isnan(v["histogram"]).all() for v in bad.values())


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_multivariate_ranks(tmp_path):
    from fourierdiffusion_amd.sampling.masks import observation_mask
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=1", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=rankrun"], tmp_path)
    run_dir = tmp_path / "lightning_logs" / "rankrun"
    base = [str(ROOT / "cmd" / "impute.py"), "model_id=rankrun", "num_diffusion_steps=5", "sampler.sample_batch_size=40",
            "mask.kind=forecast", "mask.horizon=6", "num_samples_per_series=4", "num_series=12"]
    _run(base, tmp_path)
    plain = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    assert not [k for k in plain if k.startswith("rank_") or k == "n_series_ranked"]
    _run(base + ["multivariate_ranks=[average,mst]"], tmp_path)
    res = yaml.safe_load(open(run_dir / "results.yaml"))["impute"]
    new = set(res) - set(plain)
    assert new == {"rank_reliability_index_average", "rank_histogram_average", "rank_reliability_index_mst", "rank_histogram_mst",
                   "n_series_ranked"}, new
    assert set(plain) <= set(res)
    assert res["n_series_ranked"] == 12
    # against the restatement on what the CLI wrote: the same truth split, mask and channel scale
    from fourierdiffusion_amd.config import instantiate, load_yaml
    X = torch.load(run_dir / "imputations.pt").numpy()
    dm = instantiate(load_yaml(run_dir / "train_config.yaml").datamodule)
    dm.prepare_data()
    dm.setup()
    truth = dm.X_test.float()[:12].numpy()
    mask = observation_mask("forecast", truth.shape, horizon=6).numpy()
    ref = R.multivariate_ranks(X, truth, mask, "average")
    hist = R.rank_histogram(ref["below"], ref["equal"], ref["hidden"], 4)
    np.testing.assert_allclose(res["rank_histogram_average"], hist, rtol=0, atol=1e-12)
    assert abs(res["rank_reliability_index_average"] - R.reliability_index(hist)) <= 1e-12
    assert len(res["rank_histogram_mst"]) == 5 and abs(sum(res["rank_histogram_mst"]) - 1.0) <= 1e-12
