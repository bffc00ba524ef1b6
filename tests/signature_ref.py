"""Float64 reference of the path signature (include/fdiff_hip.h, fd_series_signature), written from the definition; numpy only, the
engine is never called here.

The path of a series x (T, C), in this order:
    1. p[t, c] = scale_c (x[t, c] - offset_c), in double
    2. BASEPOINT: the point 0 is prepended
    3. D[s] = p[s + 1] - p[s] over S = T - 1 segments (T with a basepoint)
    4. LEAD_LAG: 2 S segments over 2 C channels [lead_0..lead_{C-1}, lag_0..lag_{C-1}]; segment 2 k moves the lead channels by D[k],
       segment 2 k + 1 the lag channels by D[k]
    5. TIME: one last channel that moves by 1.0 / S' per segment, S' the final number of segments
d = the final channel count; the features are the levels 1..m concatenated, a level row-major over its words, first letter slowest.

`signature` is the Horner form of Chen's identity with the exponential of a linear segment (for a level-k word w:
acc = D[w_1] / k; acc = (acc + S_j[w_1..w_j]) D[w_{j+1}] / (k - j), j = 1..k-1; S_k[w] += acc, every read of the state before the
segment); `signature_direct` is the truncated tensor-algebra product S (x) exp(D) with exp(D)_k = D^{(x) k} / k! formed on its own.

The bound (error_bounds).  u = 2^-53, l = sum_s ||D[s]||_1, M_k = l^k / k!.  M_k majorises every level-k entry at every step (the
signature of a path of 1-variation l has level-k entries of absolute sum at most l^k / k!).  A Horner update of a level-k entry is
k - 1 additions, k - 1 multiplications, k divisions and the final addition: at most 2 k + 2 <= 14 roundings of quantities bounded by
M_k.  After S' segments an entry is within 14 S' u M_k (1 + O(S' u)) of the exact value; two such computations differ by at most twice
that, and b_k = 32 S' u M_k covers both sides with room for a contracted product.  (The increments themselves are formed the same
way on both sides -- one subtraction, one product, one subtraction, none contracted -- and are bit-identical.)"""
from __future__ import annotations

import math

import numpy as np

U32 = 2.0 ** -24
V64 = 2.0 ** -53
CHUNK_SERIES = 32
BASEPOINT, LEAD_LAG, TIME = 1, 2, 4
MAX_FEATURES = 8192


def signature_dim(channels: int, depth: int, flags: int) -> tuple[int, int]:
    d = channels * (2 if flags & LEAD_LAG else 1) + (1 if flags & TIME else 0)
    return d, sum(d ** k for k in range(1, depth + 1))


def level_slices(d: int, depth: int) -> list[slice]:
    out, lo = [], 0
    for k in range(1, depth + 1):
        out.append(slice(lo, lo + d ** k))
        lo += d ** k
    return out


def increments(x, flags: int = 0, offset=None, scale=None) -> np.ndarray:
    """(n, S', d) float64 increments of the path of every series of x (n, T, C)."""
    x = np.asarray(x, dtype=np.float64)
    n, T, C = x.shape
    off = np.zeros(C) if offset is None else np.asarray(offset, dtype=np.float64)
    scl = np.ones(C) if scale is None else np.asarray(scale, dtype=np.float64)
    p = scl * (x - off)
    if flags & BASEPOINT:
        p = np.concatenate([np.zeros((n, 1, C)), p], axis=1)
    inc = p[:, 1:] - p[:, :-1]
    if flags & LEAD_LAG:
        S = inc.shape[1]
        both = np.zeros((n, 2 * S, 2 * C))
        both[:, 0::2, :C] = inc
        both[:, 1::2, C:] = inc
        inc = both
    if flags & TIME:
        S = inc.shape[1]
        inc = np.concatenate([inc, np.full((n, S, 1), 1.0 / S)], axis=2)
    return inc


def signature(inc: np.ndarray, depth: int) -> np.ndarray:
    """(n, D) from the increments (n, S', d): the Horner form."""
    n, S, d = inc.shape
    state = [np.zeros((n, d ** k)) for k in range(1, depth + 1)]
    for s in range(S):
        dl = inc[:, s, :]
        new = []
        for k in range(1, depth + 1):
            acc = dl / k
            for j in range(1, k):
                acc = ((acc + state[j - 1])[:, :, None] * dl[:, None, :] / (k - j)).reshape(n, -1)
            new.append(state[k - 1] + acc)
        state = new
    return np.concatenate(state, axis=1)


def signature_direct(inc: np.ndarray, depth: int) -> np.ndarray:
    """(n, D): the truncated tensor-algebra product of the segment exponentials, S <- S (x) exp(D), level by level."""
    n, S, d = inc.shape

    def outer(a, b):
        return (a[:, :, None] * b[:, None, :]).reshape(n, -1)

    state = [np.ones((n, 1))] + [np.zeros((n, d ** k)) for k in range(1, depth + 1)]
    for s in range(S):
        dl = inc[:, s, :]
        ex = [np.ones((n, 1))]
        for k in range(1, depth + 1):
            ex.append(outer(ex[-1], dl) / k)
        state = [sum(outer(state[i], ex[k - i]) for i in range(k + 1)) for k in range(depth + 1)]
    return np.concatenate(state[1:], axis=1)


def error_bounds(inc: np.ndarray, depth: int) -> np.ndarray:
    """(n, D): b_k = 32 S' u l^k / k! at every level-k entry."""
    n, S, d = inc.shape
    ell = np.abs(inc).sum(axis=(1, 2))
    cols = [np.repeat((32.0 * S * V64 * ell ** k / math.factorial(k))[:, None], d ** k, axis=1) for k in range(1, depth + 1)]
    return np.concatenate(cols, axis=1)


def sqnorm_bound(ref: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """(n): sum_w (2 |ref_w| b + b^2) + D u ref_sqnorm."""
    return (2 * np.abs(ref) * bound + bound ** 2).sum(axis=1) + ref.shape[1] * V64 * (ref ** 2).sum(axis=1)


def mean_bound(ref: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """(D): mean_i b(i) + (CHUNK + n / CHUNK + 2) u mean_i |ref_i|."""
    n = ref.shape[0]
    return bound.mean(axis=0) + (CHUNK_SERIES + n / CHUNK_SERIES + 2) * V64 * np.abs(ref).mean(axis=0)


def expected_signature_distance(sa: np.ndarray, sb: np.ndarray, d: int, depth: int) -> dict:
    """Sig-W1 and the unbiased linear-kernel MMD^2 by brute force from the feature rows (the Gram matrices, diagonal left out)."""
    ma, mb = sa.mean(axis=0), sb.mean(axis=0)
    diff = ma - mb

    def own(s):
        g = s @ s.T
        m = len(s)
        return (g.sum() - np.trace(g)) / (m * (m - 1)) if m > 1 else 0.0

    return {"sig_w1": float(np.sqrt((diff ** 2).sum())),
            "sig_w1_levels": [float(np.sqrt((diff[sl] ** 2).sum())) for sl in level_slices(d, depth)],
            "sig_mmd2": float(own(sa) + own(sb) - 2.0 * (sa @ sb.T).mean())}


def sawtooth(rng: np.random.Generator, n: int, T: int, rise: float = 0.8, period: float = 25.0, noise: float = 0.05) -> np.ndarray:
    """(n, T, 1) float32: a stationary sawtooth with a slow rise (a share `rise` of the period) and a fast fall, a random phase and
    white noise; played backwards it has the same autocorrelation, spectrum and marginals."""
    phase = rng.uniform(0.0, 1.0, size=(n, 1))
    u = (np.arange(T)[None, :] / period + phase) % 1.0
    wave = np.where(u < rise, u / rise, (1.0 - u) / (1.0 - rise))
    return (wave + noise * rng.standard_normal((n, T)))[:, :, None].astype(np.float32)
