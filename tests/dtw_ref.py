"""Float64 restatements of banded dynamic time warping (utils/dtw.py, csrc/fd_dtw.hip) and what the DTW tests share.  Not a test.

Definition, for series a, b of shape (T, C) and a window w in [0, T - 1]:
    c(i, j) = sum_c (a[i, c] - b[j, c])^2,   D(0, 0) = c(0, 0),
    D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1))   for |i - j| <= w, absent neighbours = +inf,
    dtw2(a, b; w) = D(T-1, T-1).

  dtw2 / dtw2_matrix / dtw2_self_matrix   the recurrence in float64, vectorised over pairs with a Python loop over cells
  dtw2_paths           an independent brute force that enumerates every warping path (T <= 5)
  dtw2_f32             the kernel's arithmetic restated in float32 numpy (the fused multiply-add through float64)
  dtw_bound            the error bound of the GPU tests, derived and not tuned (see its docstring)
  replay_fixture       the shifted-replay experiment of the metrics tests"""
import numpy as np

U = 2.0 ** -24


def default_window(T):
    return min(T - 1, -(-T // 10))


def series(x):
    x = np.asarray(x, dtype=np.float64)
    return x[:, :, None] if x.ndim == 2 else x


def dtw2(a, b, w):
    """(n,) dtw2 of row i of a against row i of b; a, b (n, T, C) or (n, T).  Two rows of D are kept, (T, n) each."""
    a, b = series(a), series(b)
    n, T, _ = a.shape
    assert a.shape == b.shape and 0 <= w <= T - 1
    prev = np.full((T, n), np.inf)
    for i in range(T):
        jlo, jhi = max(0, i - w), min(T - 1, i + w)
        diff = a[:, i, None, :] - b[:, jlo:jhi + 1, :]
        cost = np.einsum("nbc,nbc->bn", diff, diff)              # (band, n)
        cur = np.full((T, n), np.inf)
        for j in range(jlo, jhi + 1):
            if i == 0 and j == 0:
                cur[0] = cost[0]
                continue
            best = prev[j]                                       # D(i-1, j); +inf where absent
            if j > 0:
                best = np.minimum(best, np.minimum(cur[j - 1], prev[j - 1]))
            cur[j] = cost[j - jlo] + best
        prev = cur
    return prev[T - 1].copy()


def dtw2_matrix(q, r, w):
    """(n, m) dtw2 of every row of q against every row of r."""
    q, r = series(q), series(r)
    n, m = q.shape[0], r.shape[0]
    qq = np.repeat(q, m, axis=0)
    rr = np.tile(r, (n, 1, 1))
    return dtw2(qq, rr, w).reshape(n, m)


def dtw2_self_matrix(x, w):
    """(n, n) dtw2 of a set against itself: the pairs i <= j, mirrored (dtw2 is symmetric, in float64 bit for bit)."""
    x = series(x)
    i, j = np.triu_indices(x.shape[0])
    D = np.empty((x.shape[0], x.shape[0]))
    D[i, j] = dtw2(x[i], x[j], w)
    D[j, i] = D[i, j]
    return D


def dtw2_paths(a, b, w):
    """dtw2 of ONE pair (T, C) by enumerating every monotone path from (0, 0) to (T-1, T-1) with steps (1, 0), (0, 1), (1, 1) that
    stays inside the band: nothing in common with the recurrence but the definition."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim == 1:
        a, b = a[:, None], b[:, None]
    T = a.shape[0]
    assert T <= 5
    cost = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    best = [np.inf]

    def walk(i, j, total):
        total = total + cost[i, j]
        if i == T - 1 and j == T - 1:
            best[0] = min(best[0], total)
            return
        for di, dj in ((1, 0), (0, 1), (1, 1)):
            ni, nj = i + di, j + dj
            if ni < T and nj < T and abs(ni - nj) <= w:
                walk(ni, nj, total)

    walk(0, 0, 0.0)
    return best[0]


def _fma32(d, acc):
    """float32 fma(d, d, acc): the product of two float32 is exact in float64; one float64 addition and the rounding to float32 (a
    double rounding differs from the fused one by at most half an ulp in rare cases, far inside what the bound test looks at)."""
    return (d.astype(np.float64) * d.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def dtw2_f32(a, b, w):
    """The kernel's cell in float32: D = fma(d_last, d_last, m + P), P the fma chain of the channels before the last started at 0
    (C = 1: D = fma(d, d, m)), m the min of the three predecessors (0 at the corner)."""
    a, b = series(a).astype(np.float32), series(b).astype(np.float32)
    n, T, C = a.shape
    inf = np.float32(np.inf)
    D = np.full((n, T, T), inf, dtype=np.float32)
    for i in range(T):
        for j in range(max(0, i - w), min(T - 1, i + w) + 1):
            m = np.full(n, inf, dtype=np.float32)
            if i == 0 and j == 0:
                m = np.zeros(n, dtype=np.float32)
            if i > 0:
                m = np.minimum(m, D[:, i - 1, j])
            if j > 0:
                m = np.minimum(m, D[:, i, j - 1])
            if i > 0 and j > 0:
                m = np.minimum(m, D[:, i - 1, j - 1])
            base = m
            if C > 1:
                P = np.zeros(n, dtype=np.float32)
                for c in range(C - 1):
                    P = _fma32(a[:, i, c] - b[:, j, c], P)
                base = m + P
            D[:, i, j] = _fma32(a[:, i, C - 1] - b[:, j, C - 1], base)
    return D[:, T - 1, T - 1]


def dtw_bound(T, C):
    """eps with |computed - D| <= eps * D, D the float64 dtw2.  All terms are non-negative and min is exact and monotone, so the
    computed value carries at most the roundings along one warping path: a cell's cost meets at most C + 2 roundings when it is
    formed (its subtraction counts twice, it is squared; the C fused multiply-adds or, for C > 1, C - 1 of them, one addition and
    one more) and every later cell of the path adds at most C more (in the kernel: two); a path has at most 2 T - 1 cells.  So
    eps = 1.01 (C + 2) (2 T - 1) 2^-24, the 1.01 for the second-order terms."""
    return 1.01 * (C + 2) * (2 * T - 1) * U


def knn(D, k, exclude_self=False):
    """(dist2 (n, k), idx (n, k)) from a distance matrix, ascending in (distance, index)."""
    D = np.array(D, dtype=np.float64)
    if exclude_self:
        assert D.shape[0] == D.shape[1]
        np.fill_diagonal(D, np.inf)
    assert 1 <= k <= D.shape[1] - (1 if exclude_self else 0)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(D, idx, axis=1), idx


def nnd(Dself, k):
    """NND_k (a distance, not squared) of every row of a set from its own dtw2 matrix."""
    return np.sqrt(knn(Dself, k, exclude_self=True)[0][:, k - 1])


def precision_recall(D_gen_real, D_real_real, D_gen_gen, k):
    """The formulas of sampling/metrics.py PrecisionRecall on dtw2 matrices: (|G|, |R|), (|R|, |R|), (|G|, |G|)."""
    rad_real, rad_gen = nnd(D_real_real, k) ** 2, nnd(D_gen_gen, k) ** 2
    in_real = (D_gen_real <= rad_real[None, :]).sum(axis=1)
    in_gen = (D_gen_real.T <= rad_gen[None, :]).sum(axis=1)
    return {"precision": float((in_real > 0).mean()), "recall": float((in_gen > 0).mean()),
            "density": float(in_real.sum()) / (k * D_gen_real.shape[0]),
            "coverage": float((D_gen_real.min(axis=0) <= rad_real).mean())}


def memorisation(D_gen_train, D_train_train):
    """authenticity, nn_distance_min, nn_distance_median of sampling/metrics.py Memorisation on dtw2 matrices."""
    dist = np.sqrt(D_gen_train)
    nearest = np.argmin(dist, axis=1)
    d = dist[np.arange(dist.shape[0]), nearest]
    return {"authenticity": float((d > nnd(D_train_train, 1)[nearest]).mean()), "nn_distance_min": float(d.min()),
            "nn_distance_median": float(np.median(d))}


def sinusoid_series(rs, n, T):
    """n series of three random sinusoids, (n, T, 1)."""
    t = np.arange(T)[None, None, :]
    freq = rs.uniform(0.5, 4.0, size=(n, 3, 1))
    phase = rs.uniform(0.0, 2.0 * np.pi, size=(n, 3, 1))
    amp = rs.uniform(0.5, 1.5, size=(n, 3, 1))
    return (amp * np.sin(2.0 * np.pi * freq * t / T + phase)).sum(axis=1)[:, :, None].astype(np.float32)


def replay_fixture(n=40, T=48, shift=3, seed=4):
    """The shifted-replay experiment: `train`, n series of three random sinusoids; `replay`, every training series delayed by
    `shift` samples with its first value repeated; `fresh`, n new draws.  window 5.  What a replay cannot match is its source's
    last `shift` points, so a source that ends on a steep slope can lose to a chance neighbour: over seeds 0..5 of this
    construction the float64 reference finds 97.5 to 100 % of the sources under DTW (32.5 to 45 % under Euclid) and calls 0 to 5 % of
    the replays authentic; seed 4 is one of those with 100 % and 0, which test_dtw_cpu.py re-checks."""
    rs = np.random.RandomState(seed)
    train = sinusoid_series(rs, n, T)
    replay = np.concatenate([np.repeat(train[:, :1], shift, axis=1), train[:, :T - shift]], axis=1)
    fresh = sinusoid_series(rs, n, T)
    return dict(train=train, replay=replay, fresh=fresh, window=5)
