"""Float64 reference of the dependence features (include/fdiff_hip.h, fd_series_dependence): direct O(T L) sums straight from the
definitions, the constant-channel rule, the derived per-entry error bound, a float32 restatement of the engine's arithmetic and
the metric's arithmetic on set means.  numpy only; the engine is never called here.

Definitions, per series x (T, C) and channel c (biased estimators):
    mu = mean_t x,  e = x - mu,  m_k = mean_t e^k,  moments = (mu, sqrt(m_2), m_3 / m_2^1.5, m_4 / m_2^2 - 3)
    acf[l-1, c]   = sum_{t < T-l} e[t,c] e[t+l,c] / (T m_2(c)),                 l = 1..L
    ccf[l, c, d]  = sum_{t < T-l} e[t,c] e[t+l,d] / (T sqrt(m_2(c) m_2(d))),    l = 0..Lx
A channel whose T entries are bit-equal has e = 0: skewness, kurtosis, acf and every ccf entry it takes part in are 0."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32
V64 = 2.0 ** -53          # and of float64
CHUNK_SERIES = 32         # the engine's chunk of the set means (fd_dependence.hip, DEP_CHUNK)


@dataclass
class Features:
    moments: np.ndarray               # (n, C, 4)
    acf: np.ndarray                   # (n, L, C)
    ccf: Optional[np.ndarray]         # (n, Lx + 1, C, C) or None

    def flat(self) -> np.ndarray:
        """(n, F) in the engine's order moments | acf | ccf."""
        n = self.moments.shape[0]
        parts = [self.moments.reshape(n, -1), self.acf.reshape(n, -1)]
        if self.ccf is not None:
            parts.append(self.ccf.reshape(n, -1))
        return np.concatenate(parts, axis=1)

    def set_mean(self) -> np.ndarray:
        return self.flat().mean(axis=0)


def _constant(x: np.ndarray) -> np.ndarray:
    """(n, C): the channel's T entries are all equal."""
    return (x == x[:, :1, :]).all(axis=1)


def _centre(x: np.ndarray):
    x = np.asarray(x, dtype=np.float64)
    const = _constant(x)
    mu = x.mean(axis=1)
    mu = np.where(const, x[:, 0, :], mu)
    e = x - mu[:, None, :]
    e[np.broadcast_to(const[:, None, :], e.shape)] = 0.0
    return x, mu, e, const


def _moments(mu, e, const):
    T = e.shape[1]
    m2, m3, m4 = (e ** 2).sum(axis=1) / T, (e ** 3).sum(axis=1) / T, (e ** 4).sum(axis=1) / T
    safe = np.where(const | (m2 == 0), 1.0, m2)
    skew = np.where(const | (m2 == 0), 0.0, m3 / safe ** 1.5)
    kurt = np.where(const | (m2 == 0), 0.0, m4 / safe ** 2 - 3.0)
    return np.stack([mu, np.sqrt(m2), skew, kurt], axis=-1), m2


def _lag_sums(e: np.ndarray, lags: range) -> np.ndarray:
    """(n, len(lags), C, C): sum_{t < T-l} e[t,c] e[t+l,d], the direct sum."""
    n, T, C = e.shape
    out = np.zeros((n, len(lags), C, C))
    for i, l in enumerate(lags):
        out[:, i] = np.einsum("ntc,ntd->ncd", e[:, : T - l, :], e[:, l:, :])
    return out


def _diag_lag_sums(e: np.ndarray, lags: range) -> np.ndarray:
    n, T, C = e.shape
    out = np.zeros((n, len(lags), C))
    for i, l in enumerate(lags):
        out[:, i] = (e[:, : T - l, :] * e[:, l:, :]).sum(axis=1)
    return out


def features(x, L: int, Lx: int = -1) -> Features:
    """The float64 reference.  x (n, T, C); L in [0, T-1]; Lx in [-1, T-1]."""
    x, mu, e, const = _centre(x)
    n, T, C = x.shape
    assert 0 <= L <= T - 1 and -1 <= Lx <= T - 1
    moments, m2 = _moments(mu, e, const)
    S = m2 * T
    dead = const | (S == 0)
    Ssafe = np.where(dead, 1.0, S)
    acf = _diag_lag_sums(e, range(1, L + 1)) / Ssafe[:, None, :]
    acf[np.broadcast_to(dead[:, None, :], acf.shape)] = 0.0
    ccf = None
    if Lx >= 0:
        den = np.sqrt(Ssafe[:, :, None] * Ssafe[:, None, :])
        ccf = _lag_sums(e, range(0, Lx + 1)) / den[:, None]
        pair_dead = dead[:, :, None] | dead[:, None, :]
        ccf[np.broadcast_to(pair_dead[:, None], ccf.shape)] = 0.0
    return Features(moments, acf, ccf)


def features_fft(x, L: int, Lx: int = -1) -> Features:
    """The same features by an independent route: zero-pad to 2 T, FFT, |X|^2 or conj(X_c) X_d, inverse, normalise."""
    x, mu, e, const = _centre(x)
    n, T, C = x.shape
    moments, m2 = _moments(mu, e, const)
    S = m2 * T
    dead = const | (S == 0)
    Ssafe = np.where(dead, 1.0, S)
    E = np.fft.fft(e, n=2 * T, axis=1)                                     # (n, 2T, C)
    auto = np.fft.ifft(np.abs(E) ** 2, axis=1).real                        # lag l at index l
    acf = auto[:, 1: L + 1, :] / Ssafe[:, None, :]
    acf[np.broadcast_to(dead[:, None, :], acf.shape)] = 0.0
    ccf = None
    if Lx >= 0:
        # sum_t e[t,c] e[t+l,d] = ifft(conj(E_c) E_d)[l]
        cross = np.fft.ifft(np.conj(E)[:, :, :, None] * E[:, :, None, :], axis=1).real
        ccf = cross[:, : Lx + 1] / np.sqrt(Ssafe[:, :, None] * Ssafe[:, None, :])[:, None]
        pair_dead = dead[:, :, None] | dead[:, None, :]
        ccf[np.broadcast_to(pair_dead[:, None], ccf.shape)] = 0.0
    return Features(moments, acf, ccf)


def features_f32(x, L: int, Lx: int = -1) -> Features:
    """Restatement of the engine's arithmetic: the mean in float64, e = float32(x - mu) with the difference in float64, every sum of
    products of e in float64, value = float32(sum / sqrt(S_c S_d)).  float32 enters exactly where it does in the kernel; what differs
    is the order of the float64 additions (relative T 2^-52)."""
    x32 = np.asarray(x, dtype=np.float32)
    xd = x32.astype(np.float64)
    n, T, C = xd.shape
    const = _constant(x32)
    mu = np.where(const, xd[:, 0, :], xd.sum(axis=1) / T)
    e = (xd - mu[:, None, :]).astype(np.float32).astype(np.float64)
    S2, S3, S4 = (e ** 2).sum(axis=1), (e ** 3).sum(axis=1), (e ** 4).sum(axis=1)
    dead = S2 == 0
    m2 = S2 / T
    safe = np.where(dead, 1.0, m2)
    skew = np.where(dead, 0.0, (S3 / T) / (safe * np.sqrt(safe)))
    kurt = np.where(dead, 0.0, (S4 / T) / (safe * safe) - 3.0)
    moments = np.stack([mu, np.sqrt(m2), skew, kurt], axis=-1).astype(np.float32)
    Ssafe = np.where(dead, 1.0, S2)
    acf = _diag_lag_sums(e, range(1, L + 1)) * (1.0 / np.sqrt(Ssafe * Ssafe))[:, None, :]
    acf[np.broadcast_to(dead[:, None, :], acf.shape)] = 0.0
    ccf = None
    if Lx >= 0:
        inv = 1.0 / np.sqrt(Ssafe[:, :, None] * Ssafe[:, None, :])
        ccf = _lag_sums(e, range(0, Lx + 1)) * inv[:, None]
        pair_dead = dead[:, :, None] | dead[:, None, :]
        ccf[np.broadcast_to(pair_dead[:, None], ccf.shape)] = 0.0
        ccf = ccf.astype(np.float32)
    return Features(moments, acf.astype(np.float32), ccf)


def _quotient(A, dA, B, dB):
    """|A~/B~ - A/B| <= (dA + |A/B| dB) / (B - dB) for |A~ - A| <= dA, |B~ - B| <= dB < B."""
    q = np.abs(A) / B
    return (dA + q * dB) / (B - dB)


def error_bounds(x, L: int, Lx: int = -1, mean_of=None) -> Features:
    """Per-entry bound on |engine - float64 reference| (include/fdiff_hip.h), nothing tuned.  With u = 2^-24,
    v = 2^-53: the engine's e~_t = e_t + eta_t, |eta_t| <= h_t = (u + 2 v) |e_t| + rho, rho = (T + 2) v max_t |x_t| (the double sum
    of the mean, its division and the double subtraction); every sum of products is a float64 chain (relative T v on the sum of
    absolute terms); one float32 rounding of the returned value.  A constant channel is exact (bound 0 but for the mean's own
    rounding).  `mean_of`: the array whose max |x| sets rho when the features are compared with those of ANOTHER (unshifted) array:
    the offset test passes the shifted series here."""
    x, mu, e, const = _centre(x)
    n, T, C = x.shape
    amax = np.abs(x if mean_of is None else np.asarray(mean_of, dtype=np.float64)).max(axis=1)        # (n, C)
    rho = np.where(const, 0.0, (T + 2) * V64 * amax)
    ae = np.abs(e)
    h = (U32 + 2 * V64) * ae + rho[:, None, :]
    h[np.broadcast_to(const[:, None, :], h.shape)] = 0.0
    up = ae + h                                                                   # |e~| at most
    chain = (T + 4) * V64
    S2, S3, S4 = (e ** 2).sum(axis=1), (e ** 3).sum(axis=1), (e ** 4).sum(axis=1)
    dS2 = (up ** 2 - ae ** 2).sum(axis=1) + chain * (up ** 2).sum(axis=1)
    dS3 = (up ** 3 - ae ** 3).sum(axis=1) + chain * (up ** 3).sum(axis=1)
    dS4 = (up ** 4 - ae ** 4).sum(axis=1) + chain * (up ** 4).sum(axis=1)
    dead = const | (S2 == 0)
    S2s = np.where(dead, 1.0, S2)
    dS2 = np.where(dead, 0.0, dS2)
    sd = np.sqrt(S2s / T)
    moments, _ = _moments(mu, e, const)
    b_mean = U32 * np.abs(mu) * (1 + 4 * V64) + rho
    b_sd = np.where(dead, 0.0, (dS2 / T) / (np.sqrt(np.maximum(S2s - dS2, 0.0) / T) + sd) * (1 + U32) + (U32 + 4 * V64) * sd)
    B15, dB15 = S2s ** 1.5, (S2s + dS2) ** 1.5 - S2s ** 1.5
    B2, dB2 = S2s ** 2, (S2s + dS2) ** 2 - S2s ** 2
    skew, kurt = moments[..., 2], moments[..., 3]
    b_skew = np.where(dead, 0.0, np.sqrt(T) * _quotient(S3, dS3, B15, dB15) * (1 + U32) + (U32 + 8 * V64) * np.abs(skew))
    b_kurt = np.where(dead, 0.0, T * _quotient(S4, dS4, B2, dB2) * (1 + U32) + (U32 + 8 * V64) * (np.abs(kurt) + 3.0))
    b_mom = np.stack([b_mean, b_sd, b_skew, b_kurt], axis=-1)

    ref = features(x, L, Lx)

    def lag_bound(l, cs, ds, r):
        """bound for the pairs (cs[i], ds[i]) at lag l; r the reference values (n, len)"""
        a, ha = ae[:, : T - l, :][:, :, cs], h[:, : T - l, :][:, :, cs]
        b, hb = ae[:, l:, :][:, :, ds], h[:, l:, :][:, :, ds]
        dN = (a * hb + ha * b + ha * hb).sum(axis=1) + chain * ((a + ha) * (b + hb)).sum(axis=1)
        D = np.sqrt(S2s[:, cs] * S2s[:, ds])
        dD = D - np.sqrt((S2s[:, cs] - dS2[:, cs]) * (S2s[:, ds] - dS2[:, ds])) + 4 * V64 * D
        out = (dN + np.abs(r) * dD) / (D - dD) * (1 + U32) + (U32 + 8 * V64) * np.abs(r)
        return np.where(dead[:, cs] | dead[:, ds], 0.0, out)

    idx = np.arange(C)
    b_acf = np.zeros_like(ref.acf)
    for l in range(1, L + 1):
        b_acf[:, l - 1] = lag_bound(l, idx, idx, ref.acf[:, l - 1])
    b_ccf = None
    if Lx >= 0:
        cs, ds = np.repeat(idx, C), np.tile(idx, C)
        b_ccf = np.zeros_like(ref.ccf)
        for l in range(0, Lx + 1):
            b_ccf[:, l] = lag_bound(l, cs, ds, ref.ccf[:, l].reshape(n, C * C)).reshape(n, C, C)
    return Features(b_mom, b_acf, b_ccf)


def closed_form_constant(T: int) -> float:
    """The constant c of the absolute bound c u on an acf / ccf entry with rho = 0: 2 u from each of e and e' (Cauchy-Schwarz:
    sum |e e'| <= D), 2 u |r| from the denominator, u |r| from the returned float32, and the float64 chains."""
    return 5.0 + 8.0 * (T + 4) * V64 / U32 + 64 * U32


# ---------------------------------------------------------------------------------------------- the metric's arithmetic
def w2_marginals(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Wasserstein-2 per column between two (n, k) / (m, k) samples with uniform weights: the quantile functions are step functions,
    integrated exactly over the merged grid of both sets' steps."""
    a, b = np.sort(np.asarray(a, dtype=np.float64), axis=0), np.sort(np.asarray(b, dtype=np.float64), axis=0)
    n, m = a.shape[0], b.shape[0]
    grid = np.unique(np.concatenate([np.arange(n + 1) / n, np.arange(m + 1) / m]))
    mid, width = 0.5 * (grid[1:] + grid[:-1]), np.diff(grid)
    ia, ib = np.minimum((mid * n).astype(int), n - 1), np.minimum((mid * m).astype(int), m - 1)
    return np.sqrt((width[:, None] * (a[ia] - b[ib]) ** 2).sum(axis=0))


def metric_values(samples_mean: dict, real_mean: dict, C: int, suffix: str = "") -> dict:
    """The set-mean keys of TemporalDependence from two dicts of set means {"moments": (C, 4), "acf": (L, C), "ccf": (Lx+1, C, C) or
    None}."""
    out = {}
    d = np.abs(np.asarray(samples_mean["acf"], dtype=np.float64) - np.asarray(real_mean["acf"], dtype=np.float64))
    if d.size:
        out[f"acf_distance{suffix}"], out[f"acf_distance_max{suffix}"] = float(d.mean()), float(d.max())
    if C > 1 and samples_mean.get("ccf") is not None:
        dc = np.abs(np.asarray(samples_mean["ccf"], dtype=np.float64) - np.asarray(real_mean["ccf"], dtype=np.float64))
        off = ~np.eye(C, dtype=bool)
        dc = dc[:, off]
        out[f"ccf_distance{suffix}"], out[f"ccf_distance_max{suffix}"] = float(dc.mean()), float(dc.max())
    dm = np.abs(np.asarray(samples_mean["moments"], dtype=np.float64) - np.asarray(real_mean["moments"], dtype=np.float64))
    out[f"skewness_distance{suffix}"], out[f"kurtosis_distance{suffix}"] = float(dm[:, 2].mean()), float(dm[:, 3].mean())
    return out


def set_means(f: Features) -> dict:
    return {"moments": f.moments.mean(axis=0), "acf": f.acf.mean(axis=0), "ccf": None if f.ccf is None else f.ccf.mean(axis=0)}


def ar1(rng: np.random.Generator, n: int, T: int, phi: float) -> np.ndarray:
    """(n, T, 1) stationary AR(1) with unit innovations: variance 1 / (1 - phi^2)."""
    x = np.empty((n, T))
    x[:, 0] = rng.standard_normal(n) / np.sqrt(1 - phi * phi)
    eps = rng.standard_normal((n, T))
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + eps[:, t]
    return x[:, :, None]
