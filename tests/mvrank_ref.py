"""Float64 numpy restatement of the multivariate rank histograms (csrc/fd_mvrank.hip, fourierdiffusion_amd/sampling/forecast.py),
written from the definitions: O(m^2 d) counting and Prim's algorithm over one series at a time.  For one series S = {x_0 = truth,
x_1 .. x_K}, m = K + 1 points over its hidden entries H; for candidate j and entry e, over all m points i (j included),
b = #{i : x_i[e] < x_j[e]} and a = #{i : x_i[e] > x_j[e]}.

  average     R_j = sum_e (m - a)
  band_depth  B_j = sum_e [C(m,2) - C(b,2) - C(a,2)]
  dominance   G_j = #{i : x_i[e] <= x_j[e] for every e}
  mst         L_j = length of the Euclidean minimum spanning tree of S without x_j (0 with fewer than two points left)

Shared by tests/test_mvrank_cpu.py and tests/test_gpu_mvrank.py, with the generator of the coherent and the shuffled ensemble."""
import numpy as np

KINDS = ("average", "band_depth", "dominance", "mst")


def integer_preranks(S, kind):
    """S (m, d): the points of one series over its hidden entries.  int64 (m,)."""
    S = np.asarray(S)
    m, d = S.shape
    out = np.zeros(m, dtype=np.int64)
    cm2 = m * (m - 1) // 2
    for j in range(m):
        if kind == "dominance":
            out[j] = int((S <= S[j]).all(axis=1).sum())
            continue
        b = (S < S[j]).sum(axis=0).astype(np.int64)
        a = (S > S[j]).sum(axis=0).astype(np.int64)
        out[j] = (m - a).sum() if kind == "average" else (cm2 - b * (b - 1) // 2 - a * (a - 1) // 2).sum()
    return out


def distances(S):
    """(m, m) float64 Euclidean distances of the rows of S (m, d)."""
    S = np.asarray(S, dtype=np.float64)
    m = S.shape[0]
    D = np.zeros((m, m))
    for i in range(m):
        D[i] = np.sqrt(((S - S[i]) ** 2).sum(axis=1))
    return D


def mst_length(D, leave_out=None):
    """Length of the minimum spanning tree of the complete graph with edge lengths D (m, m), without vertex leave_out: Prim."""
    keep = [v for v in range(D.shape[0]) if v != leave_out]
    if len(keep) < 2:
        return 0.0
    D = D[np.ix_(keep, keep)]
    k = D.shape[0]
    key = D[0].copy()
    inside = np.zeros(k, bool)
    inside[0] = True
    total = 0.0
    for _ in range(k - 1):
        u = int(np.argmin(np.where(inside, np.inf, key)))
        total += key[u]
        inside[u] = True
        key = np.minimum(key, D[u])
    return total


def mst_preranks(S, candidates=None):
    """(L (m,) float64 with NaN at the candidates not asked for, the largest edge length)."""
    D = distances(S)
    m = D.shape[0]
    L = np.full(m, np.nan)
    for j in (range(m) if candidates is None else candidates):
        L[j] = mst_length(D, j)
    return L, float(D.max())


def multivariate_ranks(samples, truth, mask, kind, candidates=None):
    """dict(prerank (n, K + 1) float64, below (n,), equal (n,), hidden (n,), edge (n,): the largest distance, mst only).  samples
    (n, K, T, C), truth (n, T, C), mask True = observed, (n, T, C) or (T, C).  A NaN at a hidden entry poisons the series: below =
    equal = -1, pre-ranks -1 (NaN for mst).  candidates (mst only): the pre-ranks to compute, the truth's among them; below and
    equal are then -2 (not computed)."""
    x, y = np.asarray(samples), np.asarray(truth)
    n, K, T, Cn = x.shape
    m = K + 1
    H = ~np.broadcast_to(np.asarray(mask, dtype=bool), (n, T, Cn))
    pre = np.zeros((n, m))
    below, equal, edge = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n)
    for s in range(n):
        S = np.concatenate([y[s][H[s]][None], x[s][:, H[s]]], axis=0)          # (m, d), row 0 the truth
        if np.isnan(S).any():
            pre[s] = np.nan if kind == "mst" else -1.0
            below[s] = equal[s] = -1
            continue
        if kind == "mst":
            pre[s], edge[s] = mst_preranks(S, candidates)
        else:
            pre[s] = integer_preranks(S, kind)
        if candidates is not None:
            below[s] = equal[s] = -2
            continue
        below[s] = int((pre[s, 1:] < pre[s, 0]).sum())
        equal[s] = int((pre[s, 1:] == pre[s, 0]).sum())
    return dict(prerank=pre, below=below, equal=equal, hidden=H.reshape(n, -1).sum(1), edge=edge)


def rank_histogram(below, equal, hidden, K):
    """(K + 1,) frequencies over the series with a hidden entry: unit mass spread evenly over bins below .. below + equal."""
    hist = np.zeros(K + 1)
    count = 0
    for b, e, h in zip(below, equal, hidden):
        if h == 0:
            continue
        if b < 0:
            return np.full(K + 1, np.nan)
        count += 1
        hist[b:b + e + 1] += 1.0 / (e + 1)
    return hist / count if count else np.full(K + 1, np.nan)


def reliability_index(hist):
    hist = np.asarray(hist, dtype=np.float64)
    return float(np.abs(hist - 1.0 / hist.size).sum())


def entry_rank_histogram(samples, truth, K):
    """The per-entry rank histogram over every entry (K + 1,), for comparison: blind to a shuffle."""
    x, y = np.asarray(samples), np.asarray(truth)
    below, equal = (x < y[:, None]).sum(1).ravel(), (x == y[:, None]).sum(1).ravel()
    hist = np.zeros(K + 1)
    for b, e in zip(below, equal):
        hist[b:b + e + 1] += 1.0 / (e + 1)
    return hist / below.size


def coherent_and_shuffled(n=400, K=19, T=12, Cn=2, seed=0):
    """(truth (n, T, C), coherent (n, K, T, C), shuffled (n, K, T, C)) float32: every point of a series is a common level plus
    noise, row 0 the truth; the shuffled copy permutes the members independently at every entry (same marginals, no dependence)."""
    rng = np.random.default_rng(seed)
    d = T * Cn
    level = rng.normal(size=(n, K + 1, 1))
    X = (level + 0.5 * rng.normal(size=(n, K + 1, d))).astype(np.float32)
    Y = X.copy()
    for s in range(n):
        for e in range(d):
            Y[s, 1:, e] = X[s, 1 + rng.permutation(K), e]
    shape = (n, K, T, Cn)
    return X[:, 0].reshape(n, T, Cn), X[:, 1:].reshape(shape), Y[:, 1:].reshape(shape)


def mst_relative_gaps(prerank):
    """Per series, the smallest |L_j - L_0| over the members j over the largest length of the series."""
    pre = np.asarray(prerank)
    return np.abs(pre[:, 1:] - pre[:, :1]).min(axis=1) / pre.max(axis=1)
