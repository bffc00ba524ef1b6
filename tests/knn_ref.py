"""Float64 brute-force restatements of the nearest-neighbour primitives (utils/neighbours.py) and of the metrics built on them
(sampling/metrics.py: PrecisionRecall, Memorisation).  Everything is the direct form sum (q - r)^2 on the full (n, m) matrix: the
thing the engine must not build, and small enough here."""
import numpy as np

U = 2.0 ** -24


def flat(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(x.shape[0], -1)


def dist2(q, r, chunk=64):
    """(n, m) squared Euclidean distances, direct form."""
    q, r = flat(q), flat(r)
    out = np.empty((q.shape[0], r.shape[0]))
    for a in range(0, q.shape[0], chunk):
        out[a: a + chunk] = ((q[a: a + chunk, None, :] - r[None, :, :]) ** 2).sum(axis=2)
    return out


def knn(q, r, k, exclude_self=False, D=None):
    """(dist2 (n, k), idx (n, k)): the k nearest rows of r for every row of q, ascending in (distance, index)."""
    D = dist2(q, r) if D is None else np.array(D, dtype=np.float64)
    if exclude_self:
        assert D.shape[0] == D.shape[1]
        D = D.copy()
        np.fill_diagonal(D, np.inf)
    assert 1 <= k <= D.shape[1] - (1 if exclude_self else 0)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]          # stable: ties go to the lower index
    return np.take_along_axis(D, idx, axis=1), idx


def ball_counts(q, r, radius2, D=None):
    """counts[i] = #{j : d2(q_i, r_j) <= radius2[j]}."""
    D = dist2(q, r) if D is None else D
    return (D <= np.asarray(radius2, dtype=np.float64)[None, :]).sum(axis=1)


def expansion_bound(q, r):
    """delta (n, m) = 2 (d + 3) u (||q_i - mu||^2 + ||r_j - mu||^2), mu the mean of r: the worst-case error of the f32 expansion
    ||q||^2 + ||r||^2 - 2 q.r of the two sets centred by mu (d products and d additions of the dot product, the two norms, the
    centring and the final combination, each a relative error u of terms bounded by the two norms)."""
    q, r = flat(q), flat(r)
    mu = r.mean(axis=0)
    qn, rn = ((q - mu) ** 2).sum(axis=1), ((r - mu) ** 2).sum(axis=1)
    return 2.0 * (q.shape[1] + 3) * U * (qn[:, None] + rn[None, :])


def nnd(x, k):
    """NND_k: the distance of every row to its k-th nearest neighbour in its own set."""
    return np.sqrt(knn(x, x, k, exclude_self=True)[0][:, k - 1])


def subsample_indices(n, size, seed):
    return np.sort(np.random.default_rng(seed).choice(n, size=size, replace=False))


def precision_recall(real, generated, k=5):
    real, generated = flat(real), flat(generated)
    D = dist2(generated, real)                                  # (|G|, |R|)
    rad_real, rad_gen = nnd(real, k) ** 2, nnd(generated, k) ** 2
    in_real = (D <= rad_real[None, :]).sum(axis=1)
    in_gen = (D.T <= rad_gen[None, :]).sum(axis=1)
    return {"precision": float((in_real > 0).mean()), "recall": float((in_gen > 0).mean()),
            "density": float(in_real.sum()) / (k * generated.shape[0]),
            "coverage": float((D.min(axis=0) <= rad_real).mean())}


def memorisation(train, generated, holdout=None, seed=0):
    train, generated = flat(train), flat(generated)
    D = np.sqrt(dist2(generated, train))
    nearest = np.argmin(D, axis=1)
    dist = D[np.arange(D.shape[0]), nearest]
    out = {"authenticity": float((dist > nnd(train, 1)[nearest]).mean()), "nn_distance_min": float(dist.min()),
           "nn_distance_median": float(np.median(dist))}
    if holdout is not None:
        holdout = flat(holdout)
        sub = train if train.shape[0] <= holdout.shape[0] else train[subsample_indices(train.shape[0], holdout.shape[0], seed)]
        to_train = np.sqrt(dist2(generated, sub)).min(axis=1)
        to_held = np.sqrt(dist2(generated, holdout)).min(axis=1)
        out["train_closer_share"] = float((to_train < to_held).mean() + 0.5 * (to_train == to_held).mean())
    return out
