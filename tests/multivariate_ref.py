"""Float64 numpy restatement of the multivariate ensemble scores (csrc/fd_multivariate.hip, fourierdiffusion_amd/sampling/
forecast.py), written from the definitions: O(K^2 d) and O(d^2 K) loops over one series at a time.  Shared by
tests/test_multivariate_cpu.py and tests/test_gpu_multivariate.py."""
import numpy as np


def _hidden(mask, n, T, Cn):
    return ~np.broadcast_to(np.asarray(mask, dtype=bool), (n, T, Cn))


def energy_series(x, y, fair=False):
    """One series: x (K, d) members, y (d,) truth over its hidden entries.
    (1/K) sum_k ||x_k - y|| - 1/(2 K^2) sum_{j,k} ||x_j - x_k||; fair: 1/(2 K (K - 1))."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K, d = x.shape
    if d == 0:
        return np.nan
    t1 = sum(np.sqrt(((x[k] - y) ** 2).sum()) for k in range(K)) / K
    t2 = 0.0
    for j in range(K):
        t2 += np.sqrt(((x[j][None] - x) ** 2).sum(-1)).sum()
    if fair:
        return t1 - t2 / (2.0 * K * (K - 1))
    return t1 - t2 / (2.0 * K * K)


def energy_score(samples, truth, mask, fair=False):
    """(scores (n,) float64, hidden counts (n,) int): samples (n, K, T, C), truth (n, T, C), mask True = observed."""
    x, y = np.asarray(samples, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    n, K, T, Cn = x.shape
    H = _hidden(mask, n, T, Cn)
    out = np.array([energy_series(x[s][:, H[s]], y[s][H[s]], fair) for s in range(n)])
    return out, H.reshape(n, -1).sum(1)


def _power(v, order):
    return np.sqrt(v) if order == 0.5 else v if order == 1 else v * v


def variogram_series_multi(x, y, t, order, combos):
    """One series: x (K, d), y (d,), t (d,) the time index of every hidden entry, in entry order; combos: (max_lag or None,
    inverse_lag) pairs.  For each combo (num, den) with
    num = sum_{a<b, |t_a - t_b| <= max_lag} w_ab (|y_a - y_b|^p - (1/K) sum_k |x_ka - x_kb|^p)^2, den = sum w_ab,
    w_ab = 1 / (1 + |t_a - t_b|) or 1; num is NaN when den is 0.  The pair terms are computed once, for the widest max_lag."""
    x, y, t = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(t, dtype=np.int64)
    K, d = x.shape
    widest = None if any(c[0] is None for c in combos) else max(c[0] for c in combos)
    num, den = np.zeros(len(combos)), np.zeros(len(combos))
    for a in range(d - 1):
        lag = np.abs(t[a + 1:] - t[a])
        b = a + 1 + (np.arange(lag.size) if widest is None else np.nonzero(lag <= widest)[0])
        if b.size == 0:
            continue
        lag = lag[b - a - 1]
        vy = _power(np.abs(y[b] - y[a]), order)
        vx = _power(np.abs(x[:, b] - x[:, a:a + 1]), order).mean(0)
        term = (vy - vx) ** 2
        for i, (max_lag, inverse_lag) in enumerate(combos):
            keep = np.ones(lag.shape, bool) if max_lag is None else lag <= max_lag
            w = 1.0 / (1.0 + lag[keep]) if inverse_lag else np.ones(int(keep.sum()))
            num[i] += (w * term[keep]).sum()
            den[i] += w.sum()
    return [((nu if de > 0 else np.nan), de) for nu, de in zip(num, den)]


def variogram_series(x, y, t, order=0.5, max_lag=None, inverse_lag=True):
    return variogram_series_multi(x, y, t, order, [(max_lag, inverse_lag)])[0]


def variogram_scores_multi(samples, truth, mask, order, combos):
    """{(max_lag, weights): (num (n,), den (n,))} for combos of (max_lag or None, "inverse_lag" | "uniform")."""
    x, y = np.asarray(samples, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    n, K, T, Cn = x.shape
    H = _hidden(mask, n, T, Cn)
    tt = np.broadcast_to(np.arange(T)[:, None], (T, Cn))
    cs = [(lag, w == "inverse_lag") for lag, w in combos]
    res = [variogram_series_multi(x[s][:, H[s]], y[s][H[s]], tt[H[s]], order, cs) for s in range(n)]
    return {c: (np.array([r[i][0] for r in res]), np.array([r[i][1] for r in res])) for i, c in enumerate(combos)}


def variogram_score(samples, truth, mask, order=0.5, max_lag=None, weights="inverse_lag"):
    """(num (n,), den (n,)) float64; the score is num / den."""
    return variogram_scores_multi(samples, truth, mask, order, [(max_lag, weights)])[(max_lag, weights)]


def rank_counts(samples, truth):
    """(below, equal) int (n, T, C), -1 in both where the truth or a member is NaN."""
    x, y = np.asarray(samples), np.asarray(truth)
    with np.errstate(invalid="ignore"):
        below, equal = (x < y[:, None]).sum(1), (x == y[:, None]).sum(1)
    bad = np.isnan(x).any(1) | np.isnan(y)
    return np.where(bad, -1, below), np.where(bad, -1, equal)


def rank_histogram(below, equal, mask, K):
    """(K + 1,) frequencies over the hidden entries: entry by entry, unit mass spread evenly over bins below .. below + equal."""
    below, equal = np.asarray(below), np.asarray(equal)
    H = ~np.broadcast_to(np.asarray(mask, dtype=bool), below.shape)
    hist = np.zeros(K + 1)
    for b, e in zip(below[H], equal[H]):
        for r in range(b, b + e + 1):
            hist[r] += 1.0 / (e + 1)
    return hist / H.sum()


def reliability_index(hist):
    hist = np.asarray(hist, dtype=np.float64)
    return np.abs(hist - 1.0 / hist.size).sum()


def ar1_ensemble(n, K, T, Cn, rho, seed):
    """truth (n, T, C) and a K-member ensemble (n, K, T, C) from the same stationary AR(1) law along t, unit variance, float32;
    and the same ensemble with its members permuted independently at every entry (same marginals, no dependence)."""
    rs = np.random.RandomState(seed)
    z = rs.randn(n, K + 1, T, Cn)
    a = np.empty_like(z)
    a[:, :, 0] = z[:, :, 0]
    for t in range(1, T):
        a[:, :, t] = rho * a[:, :, t - 1] + np.sqrt(1.0 - rho * rho) * z[:, :, t]
    truth, x = a[:, 0].astype(np.float32), a[:, 1:].astype(np.float32)
    order = np.argsort(rs.rand(n, K, T, Cn), axis=1)
    shuffled = np.take_along_axis(x, order, axis=1)
    return truth, x, shuffled
