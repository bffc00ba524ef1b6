"""GPU: the multivariate ensemble scores (an extension, not in the reference) -- fd_energy_score, fd_variogram_score and
fd_ensemble_ranks against the float64 restatement of tests/multivariate_ref.py, exact lattices, a tight ensemble far from the
origin, edge series, determinism, the C ABI's argument errors, and the Python layer of sampling/forecast.py and cmd/impute.py.

Tolerance of the two scores: 1e-6 relative to the reference value (the tolerance of the per-entry scores).  The kernel takes
differences in fp32 (exact for the data here up to one rounding of the difference), sums at most 64 terms in fp32 and carries the
rest in double; a CPU emulation of that scheme stays at or below 5e-8, so the bound has a margin of 20.  Every comparison logs its
largest error (gpu_util.log_line) before it asserts."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import multivariate_ref as R
from tests.gpu_util import dev, log_line

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ORDERS = {0.5: 0, 1.0: 1, 2.0: 2}
SENTINEL = 7.0


def _mask8(mask):
    return torch.from_numpy(np.ascontiguousarray(mask)).to(torch.uint8).cuda()


def _energy_c(x, y, mask, fair=False):
    """fd_energy_score on device tensors x (n,K,T,C), y (n,T,C); mask numpy bool (n,T,C) or (T,C), True = observed."""
    from fourierdiffusion_amd import _C
    n, K, T, Cn = x.shape
    h, L = _C.ctx(x.device), _C.lib()
    need = C.c_size_t(0)
    _C.check(L.fd_energy_score_workspace_bytes(h, n, K, T, Cn, C.byref(need)), h)
    work = torch.full((max(1, need.value),), 0xA5, dtype=torch.uint8, device=x.device)
    m8 = _mask8(mask)
    es = torch.full((n,), SENTINEL, dtype=torch.float64, device=x.device)
    hid = torch.full((n,), -7, dtype=torch.int32, device=x.device)
    _C.check(L.fd_energy_score(h, x.data_ptr(), y.data_ptr(), m8.data_ptr(), int(mask.ndim == 3), n, K, T, Cn, int(fair),
                               es.data_ptr(), hid.data_ptr(), work.data_ptr(), need.value, _C.stream_of(x)), h)
    return es.cpu().numpy(), hid.cpu().numpy()


def _variogram_c(x, y, mask, order=0.5, max_lag=None, weights="inverse_lag"):
    from fourierdiffusion_amd import _C
    n, K, T, Cn = x.shape
    h, L = _C.ctx(x.device), _C.lib()
    lag = -1 if max_lag is None else max_lag
    need = C.c_size_t(0)
    _C.check(L.fd_variogram_score_workspace_bytes(h, n, K, T, Cn, lag, C.byref(need)), h)
    work = torch.full((max(1, need.value),), 0xA5, dtype=torch.uint8, device=x.device)
    m8 = _mask8(mask)
    num, den = (torch.full((n,), SENTINEL, dtype=torch.float64, device=x.device) for _ in range(2))
    hid = torch.full((n,), -7, dtype=torch.int32, device=x.device)
    _C.check(L.fd_variogram_score(h, x.data_ptr(), y.data_ptr(), m8.data_ptr(), int(mask.ndim == 3), n, K, T, Cn, ORDERS[order],
                                  lag, int(weights == "inverse_lag"), num.data_ptr(), den.data_ptr(), hid.data_ptr(),
                                  work.data_ptr(), need.value, _C.stream_of(x)), h)
    return num.cpu().numpy(), den.cpu().numpy(), hid.cpu().numpy()


def _ranks_c(x, y):
    from fourierdiffusion_amd import _C
    n, K, T, Cn = x.shape
    h = _C.ctx(x.device)
    below, equal = (torch.full((n, T, Cn), -7, dtype=torch.int32, device=x.device) for _ in range(2))
    _C.check(_C.lib().fd_ensemble_ranks(h, x.data_ptr(), y.data_ptr(), n, K, T, Cn, below.data_ptr(), equal.data_ptr(),
                                        _C.stream_of(x)), h)
    return below.cpu().numpy(), equal.cpu().numpy()


def _rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _data(n, K, T, Cn, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(n, K, T, Cn) * rs.uniform(0.2, 3.0, (1, 1, T, Cn)) + rs.randn(1, 1, T, Cn)).astype(np.float32)
    y = rs.randn(n, T, Cn).astype(np.float32)
    per_series = rs.rand(n, T, Cn) < 0.5                    # random, p = 0.5
    forecast = np.ones((T, Cn), bool)
    forecast[-max(1, T // 4):] = False                      # one shared forecast mask
    return x, y, (("random", per_series), ("forecast", forecast))


COMBOS = [(lag, w) for lag in (None, 0, 2) for w in ("inverse_lag", "uniform")]


def _check_against_float64(tag, x, y, mask, combos):
    xd, yd = dev(x), dev(y)
    n = x.shape[0]
    hidden = (~np.broadcast_to(mask, y.shape)).reshape(n, -1).sum(1)
    worst = 0.0
    for fair in ((False, True) if x.shape[1] > 1 else (False,)):
        es, hid = _energy_c(xd, yd, mask, fair)
        ref, _ = R.energy_score(x, y, mask, fair)
        assert np.array_equal(hid, hidden)
        err = _rel(es, ref)
        worst = max(worst, err)
        log_line(f"[multivariate] {tag} energy fair={fair}: max rel err {err:.3e}")
        assert err <= 1e-6, (tag, fair, err)
    for order in (0.5, 1.0, 2.0):
        refs = R.variogram_scores_multi(x, y, mask, order, combos)
        for lag, w in combos:
            num, den, hid = _variogram_c(xd, yd, mask, order, lag, w)
            rnum, rden = refs[(lag, w)]
            assert np.array_equal(hid, hidden)
            if w == "uniform":
                assert np.array_equal(den, rden), (tag, order, lag)
            else:
                assert np.abs(den - rden).max() <= 1e-12 * rden.max(), (tag, order, lag, den, rden)
            some = rden > 0                                  # C = 1 with max_lag = 0 has no pair: num NaN, den 0
            assert np.array_equal(den == 0, ~some) and np.isnan(num[~some]).all() and np.isnan(rnum[~some]).all()
            if not some.any():
                continue
            err = _rel(num[some], rnum[some])
            worst = max(worst, err)
            log_line(f"[multivariate] {tag} variogram p={order} max_lag={lag} {w}: max rel err {err:.3e}")
            assert err <= 1e-6, (tag, order, lag, w, err)
    log_line(f"[multivariate] {tag}: largest rel err {worst:.3e}")


@pytest.mark.parametrize("shape", [(3, 24, 40), (5, 100, 12), (2, 187, 1)])
@pytest.mark.parametrize("K", [1, 2, 3, 63, 64, 65, 100, 257])
def test_scores_vs_float64(K, shape):
    n, T, Cn = shape
    x, y, masks = _data(n, K, T, Cn, seed=K * 11 + T)
    for name, mask in masks:
        _check_against_float64(f"n={n} T={T} C={Cn} K={K} {name}", x, y, mask, COMBOS)


def test_scores_vs_float64_long_series_banded():
    """(1, 1024, 16), K = 64: 16384 rows, 256 row tiles; the variogram score runs with max_lag = 1 only (the band)."""
    n, K, T, Cn = 1, 64, 1024, 16
    x, y, masks = _data(n, K, T, Cn, seed=5)
    for name, mask in masks:
        _check_against_float64(f"n={n} T={T} C={Cn} K={K} {name}", x, y, mask, [(1, "inverse_lag"), (1, "uniform")])


# ------------------------------------------------------------------------------------------------ exact lattices
@pytest.mark.parametrize("K", [64, 65, 129, 1024])
def test_energy_exact_lattice(K):
    """x_k = k u, k = 1 .. K, u = (1, 1, 1, 1) on four hidden entries, y = 0: ||x_k - y|| = 2 k and ||x_j - x_k|| = 2 |j - k|,
    every norm an even integer, so ES = (K + 1) - (K^2 - 1) / (3 K) and a dropped or doubled pair shows at any K."""
    T, Cn = 30, 5
    hidden = [3, 63, 64, 149]                                # in three of the staged chunks of 64 entries
    rs = np.random.RandomState(K)
    x = (rs.randn(2, K, T * Cn) * 50).astype(np.float32)     # observed entries: anything
    y = (rs.randn(2, T * Cn) * 50).astype(np.float32)
    mask = np.ones((2, T * Cn), bool)
    mask[:, hidden] = False
    x[:, :, hidden] = np.arange(1, K + 1, dtype=np.float32)[None, :, None]
    y[:, hidden] = 0.0
    x[1] = x[1][rs.permutation(K)]                           # the member order does not matter
    es, hid = _energy_c(dev(x.reshape(2, K, T, Cn)), dev(y.reshape(2, T, Cn)), mask.reshape(2, T, Cn))
    closed = (K + 1) - (K * K - 1) / (3.0 * K)
    assert (hid == 4).all()
    assert np.abs(es - closed).max() <= 1e-12 * closed, (es, closed)
    fair, _ = _energy_c(dev(x.reshape(2, K, T, Cn)), dev(y.reshape(2, T, Cn)), mask.reshape(2, T, Cn), fair=True)
    closed_fair = (K + 1) - (K + 1) / 3.0
    assert np.abs(fair - closed_fair).max() <= 1e-12 * closed_fair, (fair, closed_fair)


@pytest.mark.parametrize("TC", [(63, 1), (64, 1), (13, 5), (127, 1), (32, 4), (43, 3), (26, 5)])
@pytest.mark.parametrize("K", [64, 128])
def test_variogram_exact_lattice(K, TC):
    """Small integers, every entry hidden, p in {1, 2}, K a power of two: every fp32 sum and every mean is exact, so the kernel
    equals the restatement to double rounding; D = T C crosses the 64-row tile edges (63 .. 130)."""
    T, Cn = TC
    rs = np.random.RandomState(K + T)
    x = rs.randint(-8, 9, (2, K, T, Cn)).astype(np.float32)
    y = rs.randint(-8, 9, (2, T, Cn)).astype(np.float32)
    mask = np.zeros((T, Cn), bool)
    for order in (1.0, 2.0):
        refs = R.variogram_scores_multi(x, y, mask, order, COMBOS)
        for lag, w in COMBOS:
            num, den, hid = _variogram_c(dev(x), dev(y), mask, order, lag, w)
            rnum, rden = refs[(lag, w)]
            assert (hid == T * Cn).all()
            if Cn == 1 and lag == 0:                         # one channel: no pair at lag 0
                assert (rden == 0).all() and (den == 0).all() and np.isnan(num).all()
                continue
            assert _rel(den, rden) <= 1e-12 and _rel(num, rnum) <= 1e-12, (order, lag, w, num, rnum, den, rden)
            if w == "uniform":
                assert np.array_equal(den, rden) and np.array_equal(num, rnum), (order, lag)


# ------------------------------------------------------------------------------------------------ tight and biased
def test_tight_ensemble_far_from_the_origin():
    """x = 100 + 1e-2 z against the truth 100.5: member distances are 1e-4 of the values' size.  The expansion
    |a|^2 + |b|^2 - 2 a.b would keep no digit of them in fp32; direct differences keep them all."""
    n, K, T, Cn = 2, 100, 24, 6
    rs = np.random.RandomState(3)
    x = (100.0 + 1e-2 * rs.randn(n, K, T, Cn)).astype(np.float32)
    y = np.full((n, T, Cn), 100.5, np.float32)
    mask = rs.rand(n, T, Cn) < 0.3
    _check_against_float64("tight and biased", x, y, mask, COMBOS)


# ------------------------------------------------------------------------------------------------ edge series
def test_edge_series():
    from fourierdiffusion_amd.sampling.forecast import kernel_scores
    n, K, T, Cn = 5, 20, 30, 5
    rs = np.random.RandomState(8)
    x = rs.randn(n, K, T, Cn).astype(np.float32)
    y = rs.randn(n, T, Cn).astype(np.float32)
    mask = rs.rand(n, T, Cn) < 0.5
    mask[0] = True                                           # series 0: all observed
    mask[1] = True
    mask[1, 17, 3] = False                                   # series 1: exactly one hidden entry
    clean = (_energy_c(dev(x), dev(y), mask), _variogram_c(dev(x), dev(y), mask, 0.5, 2, "inverse_lag"))
    es, hid = clean[0]
    num, den, vhid = clean[1]
    assert np.array_equal(hid, (~mask).reshape(n, -1).sum(1)) and np.array_equal(vhid, hid)
    assert np.isnan(es[0]) and hid[0] == 0 and np.isnan(num[0]) and den[0] == 0
    crps = kernel_scores(torch.from_numpy(x), torch.from_numpy(y))[0].numpy()
    scale = max(1.0, np.abs(x).max(), np.abs(y).max())
    assert abs(es[1] - crps[1, 17, 3]) <= 1e-6 * scale, (es[1], crps[1, 17, 3])
    assert hid[1] == 1 and np.isnan(num[1]) and den[1] == 0
    assert np.isfinite(es[2:]).all() and np.isfinite(num[2:]).all() and (den[2:] > 0).all()
    # NaN at observed entries (truth and members, every series): no effect, bitwise
    xo, yo = x.copy(), y.copy()
    xo[np.broadcast_to(mask[:, None], x.shape) & (rs.rand(*x.shape) < 0.2)] = np.nan
    yo[mask & (rs.rand(*y.shape) < 0.2)] = np.nan
    assert np.isnan(xo).any() and np.isnan(yo).any()
    es_o, hid_o = _energy_c(dev(xo), dev(yo), mask)
    num_o, den_o, _ = _variogram_c(dev(xo), dev(yo), mask, 0.5, 2, "inverse_lag")
    for a, b in ((es_o, es), (num_o, num), (den_o, den)):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(hid_o, hid)
    # NaN at a hidden entry: that series alone, whether it sits in a member or in the truth
    for where in ("member", "truth"):
        xh, yh = x.copy(), y.copy()
        t, c = np.argwhere(~mask[3])[-1]
        if where == "member":
            xh[3, K // 2, t, c] = np.nan
        else:
            yh[3, t, c] = np.nan
        es_h, _ = _energy_c(dev(xh), dev(yh), mask)
        others = [i for i in range(n) if i != 3]
        assert np.isnan(es_h[3]) and es_h[others].tobytes() == es[others].tobytes(), where
        for order in (0.5, 1.0, 2.0):
            for lag in (None, 0):
                base, bden, _ = _variogram_c(dev(x), dev(y), mask, order, lag, "uniform")
                num_h, den_h, _ = _variogram_c(dev(xh), dev(yh), mask, order, lag, "uniform")
                assert np.isnan(num_h[3]) and num_h[others].tobytes() == base[others].tobytes(), (where, order, lag)
                assert den_h.tobytes() == bden.tobytes()


def test_nan_at_a_hidden_entry_without_a_partner_in_the_band():
    """max_lag = 0 and the NaN entry is the only hidden one of its time step: it is in no pair, and the series is NaN all the same."""
    K, T, Cn = 8, 12, 3
    rs = np.random.RandomState(4)
    x, y = rs.randn(1, K, T, Cn).astype(np.float32), rs.randn(1, T, Cn).astype(np.float32)
    mask = np.zeros((1, T, Cn), bool)
    mask[0, 5, 1:] = True                                    # (5, 0) is alone at t = 5
    num, den, _ = _variogram_c(dev(x), dev(y), mask, 1.0, 0, "uniform")
    assert np.isfinite(num[0]) and den[0] == 3 * (T - 1)
    x[0, 2, 5, 0] = np.nan
    num_h, den_h, _ = _variogram_c(dev(x), dev(y), mask, 1.0, 0, "uniform")
    assert np.isnan(num_h[0]) and den_h[0] == den[0]


# ------------------------------------------------------------------------------------------------ determinism
def test_bit_reproducible_and_independent_of_batch_position():
    K, T, Cn = 70, 50, 3                                     # 150 rows: three row tiles; two member tiles
    rs = np.random.RandomState(12)
    x = rs.randn(5, K, T, Cn).astype(np.float32)
    y = rs.randn(5, T, Cn).astype(np.float32)
    mask = rs.rand(5, T, Cn) < 0.5
    runs = [(_energy_c(dev(x), dev(y), mask, True)[0], _variogram_c(dev(x), dev(y), mask, 0.5, 4, "inverse_lag")) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    assert runs[0][1][0].tobytes() == runs[1][1][0].tobytes() and runs[0][1][1].tobytes() == runs[1][1][1].tobytes()
    alone_e = _energy_c(dev(x[:1]), dev(y[:1]), mask[:1], True)[0]
    alone_n, alone_d, _ = _variogram_c(dev(x[:1]), dev(y[:1]), mask[:1], 0.5, 4, "inverse_lag")
    for pos in range(5):
        perm = [i for i in range(1, 5)]
        perm.insert(pos, 0)                                  # series 0 at position pos
        e = _energy_c(dev(x[perm]), dev(y[perm]), mask[perm], True)[0]
        vn, vd, _ = _variogram_c(dev(x[perm]), dev(y[perm]), mask[perm], 0.5, 4, "inverse_lag")
        assert e[pos:pos + 1].tobytes() == alone_e.tobytes(), pos
        assert vn[pos:pos + 1].tobytes() == alone_n.tobytes() and vd[pos:pos + 1].tobytes() == alone_d.tobytes(), pos
    shared = mask[0]                                         # and the shared-mask path reads the same mask
    assert _energy_c(dev(x[:1]), dev(y[:1]), shared, True)[0].tobytes() == alone_e.tobytes()


# ------------------------------------------------------------------------------------------------ ranks
@pytest.mark.parametrize("K", [1, 7, 100])
def test_ranks_against_the_restatement(K):
    n, T, Cn = 3, 37, 7                                      # 259 entries: more than one workgroup, a ragged tail
    rs = np.random.RandomState(K)
    x = (np.round(rs.randn(n, K, T, Cn) * 2) / 2).astype(np.float32)       # a coarse grid: ties
    y = (np.round(rs.randn(n, T, Cn) * 2) / 2).astype(np.float32)
    x[0, :, 3, 2] = y[0, 3, 2]                                              # a constant ensemble equal to the truth
    x[1, K // 2, 5, 0] = np.nan
    y[2, 36, 6] = np.nan
    below, equal = _ranks_c(dev(x), dev(y))
    rb, re = R.rank_counts(x, y)
    assert np.array_equal(below, rb) and np.array_equal(equal, re)
    assert below[0, 3, 2] == 0 and equal[0, 3, 2] == K
    assert below[1, 5, 0] == -1 and equal[1, 5, 0] == -1 and below[2, 36, 6] == -1 and equal[2, 36, 6] == -1
    assert (below >= 0).sum() == below.size - 2 and (equal > 0).any()


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_argument_errors():
    """Every new entry point refuses each bad argument with FD_ERR_ARG and a retrievable message."""
    from fourierdiffusion_amd import _C
    n, K, T, Cn = 2, 4, 6, 3
    x, y = torch.zeros(n, K, T, Cn, device="cuda"), torch.zeros(n, T, Cn, device="cuda")
    m8 = torch.zeros(n, T, Cn, dtype=torch.uint8, device="cuda")
    o1, o2 = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
    oh = torch.zeros(n, dtype=torch.int32, device="cuda")
    rb, re = (torch.zeros(n, T, Cn, dtype=torch.int32, device="cuda") for _ in range(2))
    h, L = _C.ctx(x.device), _C.lib()
    need_e, need_v = C.c_size_t(0), C.c_size_t(0)
    assert L.fd_energy_score_workspace_bytes(h, n, K, T, Cn, C.byref(need_e)) == 0 and need_e.value > 0
    assert L.fd_variogram_score_workspace_bytes(h, n, K, T, Cn, -1, C.byref(need_v)) == 0 and need_v.value > 0
    work = torch.zeros(max(need_e.value, need_v.value), dtype=torch.uint8, device="cuda")
    xp, yp, mp, p1, p2, hp, wp = (t.data_ptr() for t in (x, y, m8, o1, o2, oh, work))
    ne, nv = need_e.value, need_v.value
    big = 1 << 30

    def energy(**k):
        a = dict(x=xp, y=yp, m=mp, n=n, K=K, T=T, C=Cn, fair=0, out=p1, hid=hp, work=wp, bytes=ne)
        a.update(k)
        return L.fd_energy_score(h, a["x"], a["y"], a["m"], 1, a["n"], a["K"], a["T"], a["C"], a["fair"], a["out"], a["hid"],
                                 a["work"], a["bytes"], None)

    def variogram(**k):
        a = dict(x=xp, y=yp, m=mp, n=n, K=K, T=T, C=Cn, order=0, lag=-1, num=p1, den=p2, hid=hp, work=wp, bytes=nv)
        a.update(k)
        return L.fd_variogram_score(h, a["x"], a["y"], a["m"], 1, a["n"], a["K"], a["T"], a["C"], a["order"], a["lag"], 1, a["num"],
                                    a["den"], a["hid"], a["work"], a["bytes"], None)

    def ranks(**k):
        a = dict(x=xp, y=yp, n=n, K=K, T=T, C=Cn, below=rb.data_ptr(), equal=re.data_ptr())
        a.update(k)
        return L.fd_ensemble_ranks(h, a["x"], a["y"], a["n"], a["K"], a["T"], a["C"], a["below"], a["equal"], None)

    cases = [
        (lambda: L.fd_energy_score_workspace_bytes(h, n, K, T, Cn, None), b"null"),
        (lambda: L.fd_energy_score_workspace_bytes(h, 0, K, T, Cn, C.byref(need_e)), b"bad shape"),
        (lambda: L.fd_energy_score_workspace_bytes(h, n, 0, T, Cn, C.byref(need_e)), b"K=0"),
        (lambda: L.fd_energy_score_workspace_bytes(h, n, 1025, T, Cn, C.byref(need_e)), b"K=1025"),
        (lambda: L.fd_energy_score_workspace_bytes(h, n, K, big, 4, C.byref(need_e)), b"too large"),
        (lambda: L.fd_variogram_score_workspace_bytes(h, n, K, T, Cn, -1, None), b"null"),
        (lambda: L.fd_variogram_score_workspace_bytes(h, n, K, 0, Cn, -1, C.byref(need_v)), b"bad shape"),
        (lambda: L.fd_variogram_score_workspace_bytes(h, n, 1025, T, Cn, -1, C.byref(need_v)), b"K=1025"),
        (lambda: L.fd_variogram_score_workspace_bytes(h, big, K, 1 << 20, 1, -1, C.byref(need_v)), b"too large"),
        (lambda: energy(x=None), b"null"), (lambda: energy(y=None), b"null"), (lambda: energy(m=None), b"null"),
        (lambda: energy(out=None), b"null"), (lambda: energy(hid=None), b"null"), (lambda: energy(work=None), b"null"),
        (lambda: energy(n=0), b"bad shape"), (lambda: energy(T=-1), b"bad shape"), (lambda: energy(C=0), b"bad shape"),
        (lambda: energy(K=0), b"K=0"), (lambda: energy(K=1025), b"K=1025"),
        (lambda: energy(K=1, fair=1), b"fair"),
        (lambda: energy(bytes=ne - 1), b"workspace"), (lambda: energy(bytes=0), b"workspace"),
        (lambda: variogram(x=None), b"null"), (lambda: variogram(y=None), b"null"), (lambda: variogram(m=None), b"null"),
        (lambda: variogram(num=None), b"null"), (lambda: variogram(den=None), b"null"), (lambda: variogram(work=None), b"null"),
        (lambda: variogram(n=0), b"bad shape"), (lambda: variogram(T=0), b"bad shape"),
        (lambda: variogram(K=0), b"K=0"), (lambda: variogram(K=1025), b"K=1025"),
        (lambda: variogram(order=3), b"order=3"), (lambda: variogram(order=-1), b"order=-1"),
        (lambda: variogram(bytes=nv - 1), b"workspace"), (lambda: variogram(bytes=0), b"workspace"),
        (lambda: ranks(x=None), b"null"), (lambda: ranks(y=None), b"null"), (lambda: ranks(below=None), b"null"),
        (lambda: ranks(equal=None), b"null"), (lambda: ranks(n=0), b"bad shape"), (lambda: ranks(C=0), b"bad shape"),
        (lambda: ranks(K=0), b"K=0"), (lambda: ranks(K=1025), b"K=1025"), (lambda: ranks(n=65536), b"too large"),
    ]
    for i, (call, needle) in enumerate(cases):
        assert call() == -1, i
        assert needle in L.fd_last_error(h), (i, L.fd_last_error(h))
    assert energy() == 0 and variogram() == 0 and variogram(hid=None) == 0 and ranks() == 0       # the good arguments
    assert L.fd_energy_score(None, xp, yp, mp, 1, n, K, T, Cn, 0, p1, hp, wp, ne, None) == -1             # no context: code only
    assert L.fd_variogram_score(None, xp, yp, mp, 1, n, K, T, Cn, 0, -1, 1, p1, p2, hp, wp, nv, None) == -1
    assert L.fd_ensemble_ranks(None, xp, yp, n, K, T, Cn, rb.data_ptr(), re.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (oh.cpu().numpy() == T * Cn).all() and (o1.cpu().numpy() == 0).all() and (re.cpu().numpy() == K).all()
    # a banded workspace is smaller than the full one and is what the banded call asks for
    full, band = C.c_size_t(0), C.c_size_t(0)
    assert L.fd_variogram_score_workspace_bytes(h, 1, 8, 1024, 16, -1, C.byref(full)) == 0
    assert L.fd_variogram_score_workspace_bytes(h, 1, 8, 1024, 16, 8, C.byref(band)) == 0
    assert 0 < band.value * 20 < full.value


# ------------------------------------------------------------------------------------------------ Python layer
def _ar1_case():
    n, K, T, Cn = 8, 32, 24, 3
    truth, x, shuffled = R.ar1_ensemble(n, K, T, Cn, 0.95, seed=0)
    mask = np.zeros((T, Cn), bool)
    mask[:2] = True
    return torch.from_numpy(truth), torch.from_numpy(x), torch.from_numpy(shuffled), torch.from_numpy(mask)


def test_multivariate_scores_chunked_equals_one_chunk(monkeypatch):
    from fourierdiffusion_amd.sampling import forecast as F
    truth, x, _, _ = _ar1_case()
    mask = torch.from_numpy(np.random.RandomState(2).rand(*truth.shape) < 0.5)            # per series: the chunks slice it
    one = F.multivariate_scores(x, truth, mask, fair=True, order=1, max_lag=3, scale=torch.tensor([1.0, 2.0, 0.5]))
    monkeypatch.setattr(F, "CHUNK_BYTES", 3 * 4 * x[0].numel())                            # 3 series per call: 3 + 3 + 2
    three = F.multivariate_scores(x, truth, mask, fair=True, order=1, max_lag=3, scale=torch.tensor([1.0, 2.0, 0.5]))
    for key in ("energy", "variogram", "variogram_num", "variogram_den", "hidden", "below", "equal", "rank_histogram"):
        assert torch.equal(getattr(one, key), getattr(three, key)), key
    assert one.metrics == three.metrics
    assert one.energy.dtype == torch.float64 and tuple(one.energy.shape) == (8,) and one.hidden.dtype == torch.int32
    assert one.metrics["n_series_scored_energy"] == 8 and one.metrics["n_series_scored_variogram"] == 8
    assert one.metrics["energy_fair"] is True and one.metrics["variogram_order"] == 1.0
    assert one.metrics["variogram_max_lag"] == 3 and one.metrics["variogram_weights"] == "inverse_lag"
    assert len(one.metrics["rank_histogram"]) == 33 and abs(sum(one.metrics["rank_histogram"]) - 1.0) <= 1e-12
    # and the single-score functions return the same arrays
    assert torch.equal(F.energy_score(x, truth, mask, fair=True, scale=torch.tensor([1.0, 2.0, 0.5])), one.energy)
    assert torch.equal(F.variogram_score(x, truth, mask, order=1, max_lag=3, scale=torch.tensor([1.0, 2.0, 0.5])), one.variogram)
    below, equal = F.rank_counts(x, truth)
    assert torch.equal(below, one.below) and torch.equal(equal, one.equal)


def test_shuffled_ensemble_on_the_device():
    """The experiment of tests/test_multivariate_cpu.py through the engine: same marginals, the dependence gone."""
    from fourierdiffusion_amd.sampling import forecast as F
    truth, x, shuffled, mask = _ar1_case()
    crps = [F.kernel_scores(v, truth)[0] for v in (x, shuffled)]
    gap = float((crps[0] - crps[1]).abs().max())
    log_line(f"[multivariate] shuffle experiment: largest per-entry CRPS difference {gap:.3e}")
    assert gap <= 1e-6, gap
    got = [F.multivariate_scores(v, truth, mask, max_lag=2, weights="uniform") for v in (x, shuffled)]
    vs = [g.metrics["variogram_score"] for g in got]
    log_line(f"[multivariate] shuffle experiment: variogram score {vs[0]:.6f} -> {vs[1]:.6f}, "
             f"energy score {got[0].metrics['energy_score']:.6f} -> {got[1].metrics['energy_score']:.6f}")
    assert vs[1] >= 1.25 * vs[0], vs
    assert got[1].metrics["energy_score"] > got[0].metrics["energy_score"]
    ref = np.mean(np.divide(*R.variogram_score(x.numpy(), truth.numpy(), mask.numpy(), 0.5, 2, "uniform")))
    assert abs(vs[0] - ref) <= 1e-6 * ref
    # a series of NaN data is not dropped from the mean; a series without a hidden entry is
    xn = x.clone()
    xn[2, 5, 10, 1] = float("nan")
    bad = F.multivariate_scores(xn, truth, mask, max_lag=2, weights="uniform")
    assert np.isnan(bad.metrics["energy_score"]) and np.isnan(bad.metrics["variogram_score"])
    assert np.isnan(bad.metrics["rank_reliability_index"]) and bad.metrics["n_series_scored_energy"] == 8
    m3 = mask[None].repeat(8, 1, 1)
    m3[4] = True
    part = F.multivariate_scores(x, truth, m3, max_lag=2, weights="uniform")
    assert part.metrics["n_series_scored_energy"] == 7 and part.metrics["n_series_scored_variogram"] == 7
    keep = [i for i in range(8) if i != 4]
    assert abs(part.metrics["energy_score"] - float(got[0].energy[keep].mean())) <= 1e-15
    assert torch.isnan(part.energy[4]) and torch.isnan(part.variogram[4])


def test_scale_equals_dividing_by_hand():
    from fourierdiffusion_amd.sampling import forecast as F
    truth, x, _, mask = _ar1_case()
    scale = torch.tensor([0.5, 3.0, 1.7], dtype=torch.float64)
    by_hand = F.multivariate_scores((x.double() / scale).float(), (truth.double() / scale).float(), mask, max_lag=2)
    scaled = F.multivariate_scores(x, truth, mask, max_lag=2, scale=scale)
    plain = F.multivariate_scores(x, truth, mask, max_lag=2)
    assert torch.equal(scaled.energy, by_hand.energy) and torch.equal(scaled.variogram, by_hand.variogram)
    assert not torch.equal(scaled.energy, plain.energy)
    assert torch.equal(scaled.below, plain.below) and torch.equal(scaled.equal, plain.equal)       # ranks see the data as it is
    full = F.multivariate_scores(x, truth, mask, max_lag=2, scale=scale[None].expand(24, 3))       # a (T, C) scale
    assert torch.equal(full.energy, scaled.energy)


def _impute_module():
    spec = importlib.util.spec_from_file_location("cmd_impute_for_multivariate_gpu", ROOT / "cmd" / "impute.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_multivariate_results():
    mod = _impute_module()
    n, K, T, Cn = 30, 4, 24, 4
    rs = np.random.RandomState(21)
    chan = np.array([1.0, 10.0, 0.1, 3.0])
    truth = (rs.randn(n, T, Cn) * chan).astype(np.float32)
    X = (truth[:, None] + rs.randn(n, K, T, Cn) * chan * 0.5).astype(np.float32)
    mask = np.ones((n, T, Cn), bool)
    mask[:, -6:] = False                                     # forecast: the last 6 steps hidden
    opts = {"order": 1, "max_lag": 2, "weights": "uniform"}
    got = mod.multivariate_results(torch.from_numpy(X), torch.from_numpy(truth), torch.from_numpy(mask), opts)
    std = truth.astype(np.float64).reshape(-1, Cn).std(0)
    xs, ys = (X.astype(np.float64) / std).astype(np.float32), (truth.astype(np.float64) / std).astype(np.float32)
    ref_e = R.energy_score(xs, ys, mask)[0].mean()
    ref_v = np.mean(np.divide(*R.variogram_score(xs, ys, mask, 1.0, 2, "uniform")))
    below, equal = R.rank_counts(X, truth)
    ref_h = R.rank_histogram(below, equal, mask, K)
    assert abs(got["energy_score"] - ref_e) <= 1e-6 * ref_e and abs(got["variogram_score"] - ref_v) <= 1e-6 * ref_v
    np.testing.assert_allclose(got["rank_histogram"], ref_h, rtol=0, atol=1e-12)
    assert abs(got["rank_reliability_index"] - R.reliability_index(ref_h)) <= 1e-12
    assert got["multivariate_scale"] == "channel_std" and got["n_series_scored_energy"] == n
    assert (got["variogram_order"], got["variogram_max_lag"], got["variogram_weights"]) == (1.0, 2, "uniform")
    assert all(isinstance(v, (bool, int, float, str, list)) for v in got.values())          # plain values: they go to results.yaml
    # with the flag off the ensemble block is what it was
    plain = mod.ensemble_results(torch.from_numpy(X), torch.from_numpy(truth), torch.from_numpy(mask))
    assert set(plain) == {"num_series", "num_samples_per_series", "hidden_fraction", "max_abs_err_observed", "crps",
                          "crps_quantile", "crps_sum_quantile", "mae_median", "rmse_median", "mse_mean", "coverage_90", "width_90"}
    assert not set(plain) & set(got)
