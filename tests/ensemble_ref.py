"""Float64 numpy restatement of the ensemble scores (csrc/fd_forecast.hip, fourierdiffusion_amd/sampling/forecast.py).  Shared by
tests/test_ensemble_cpu.py and tests/test_gpu_ensemble.py."""
import math

import numpy as np

LEVELS = tuple(round(0.05 * i, 2) for i in range(1, 20))


def crps_pairwise(x, y):
    """The O(K^2) definition: x (..., K), y (...): (1/K) sum_k |x_k - y| - (1/(2K^2)) sum_{j,k} |x_j - x_k|."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K = x.shape[-1]
    t1 = np.abs(x - y[..., None]).mean(-1)
    t2 = np.abs(x[..., :, None] - x[..., None, :]).sum((-1, -2)) / (2.0 * K * K)
    return t1 - t2


def crps_sorted(x, y):
    """The sorted form: (1/K) sum_k |x_k - y| - (1/K^2) sum_i (2i - K - 1) x_(i)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K = x.shape[-1]
    xs = np.sort(x, axis=-1)
    w = 2.0 * np.arange(1, K + 1) - K - 1
    return np.abs(x - y[..., None]).mean(-1) - (xs * w).sum(-1) / (K * K)


def crps_gaussian(mu, sigma, y):
    """Closed form of the CRPS of N(mu, sigma^2): sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1/sqrt(pi)], z = (y - mu) / sigma."""
    z = (y - mu) / sigma
    Phi = 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
    phi = math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return sigma * (z * (2.0 * Phi - 1.0) + 2.0 * phi - 1.0 / math.sqrt(math.pi))


def entry_scores(samples, truth, levels=LEVELS):
    """Per entry of samples (n, K, T, C) against truth (n, T, C): crps (n,T,C), quantiles (L,n,T,C), mean (n,T,C), in float64.
    A NaN sample or truth makes that entry's outputs NaN."""
    x = np.moveaxis(np.asarray(samples, dtype=np.float64), 1, -1)          # (n, T, C, K)
    y = np.asarray(truth, dtype=np.float64)
    bad = np.isnan(x).any(-1) | np.isnan(y)
    xc = np.where(np.isnan(x), 0.0, x)
    yc = np.where(np.isnan(y), 0.0, y)
    crps = crps_sorted(xc, yc)
    q = np.quantile(xc, np.asarray(levels, dtype=np.float64), axis=-1, method="linear")
    mean = xc.mean(-1)
    crps[bad], mean[bad] = np.nan, np.nan
    q[:, bad] = np.nan
    return crps, q, mean


def quantile_crps(y, Q, levels):
    """CSDI's normalised quantile CRPS over the entries of y (m,) and quantiles Q (L, m)."""
    y, Q = np.asarray(y, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    lv = np.asarray(levels, dtype=np.float64)[:, None]
    loss = (2.0 * np.abs((y[None] - Q) * ((y[None] <= Q).astype(np.float64) - lv)).sum(1)).mean()
    den = np.abs(y).sum()
    return loss / den if den > 0 else np.nan


def aggregate(truth, mask, crps, quantiles, mean, levels, sum_truth, sum_quantiles, sum_mask):
    """The aggregates of forecast.aggregate over the hidden entries (mask False)."""
    lv = list(levels)
    i05, i50, i95 = lv.index(0.05), lv.index(0.5), lv.index(0.95)
    H = ~np.broadcast_to(np.asarray(mask, dtype=bool), np.shape(truth))
    y = np.asarray(truth, dtype=np.float64)[H]
    Q = np.asarray(quantiles, dtype=np.float64)[:, H]
    sm = np.asarray(sum_mask, dtype=bool)
    ys = np.asarray(sum_truth, dtype=np.float64)[sm]
    Qs = np.asarray(sum_quantiles, dtype=np.float64)[:, sm]
    med, lo, hi = Q[i50], Q[i05], Q[i95]
    return {
        "crps": np.asarray(crps, dtype=np.float64)[H].mean(),
        "crps_quantile": quantile_crps(y, Q, lv),
        "crps_sum_quantile": quantile_crps(ys, Qs, lv),
        "mae_median": np.abs(y - med).mean(),
        "rmse_median": np.sqrt(((y - med) ** 2).mean()),
        "mse_mean": ((y - np.asarray(mean, dtype=np.float64)[H]) ** 2).mean(),
        "coverage_90": ((lo <= y) & (y <= hi)).mean(),
        "width_90": (hi - lo).mean(),
    }


def ensemble_metrics(samples, truth, mask, levels=LEVELS):
    """The whole protocol in float64: per-entry scores, the same on the channel sums over the hidden channels, aggregated."""
    x, y = np.asarray(samples, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    H = ~np.broadcast_to(np.asarray(mask, dtype=bool), y.shape)
    crps, q, mean = entry_scores(x, y, levels)
    xs = np.where(H[:, None], x, 0.0).sum(-1, keepdims=True)
    ys = np.where(H, y, 0.0).sum(-1, keepdims=True)
    _, qs, _ = entry_scores(xs, ys, levels)
    return aggregate(y, ~H, crps, q, mean, levels, ys[..., 0], qs[..., 0], H.any(-1))
