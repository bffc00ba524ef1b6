"""Float64 brute-force restatement of the kernel two-sample test (utils/two_sample.py, csrc/fd_mmd.hip): direct differences on the
full (N, N) matrix -- the thing the engine must not build, and small enough here -- the definitions of the three sums, and the same
permutation rule.  `restate_f32` is the engine's arithmetic (centred expansion, exp2, product with the memberships) in numpy
float32; `error_bounds` is the worst-case bound the engine's contract states."""
import numpy as np

from tests.knn_ref import U, dist2, expansion_bound, flat

DEFAULT_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)


def waves(rng, n, d, fmax=4.0, noise=0.3):
    """n noisy sine waves of d points: amplitude, frequency and phase drawn per row, in that order."""
    t = np.arange(d) / d
    a = rng.uniform(0.5, 1.5, (n, 1))
    f = rng.uniform(1.0, fmax, (n, 1))
    phi = rng.uniform(0.0, 2.0 * np.pi, (n, 1))
    return a * np.sin(2.0 * np.pi * f * t + phi) + noise * rng.standard_normal((n, d))


def permutation_members(n, m, n_permutations, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((n + m, 1 + n_permutations), dtype=np.uint8)
    A[:n, 0] = 1
    for p in range(1, 1 + n_permutations):
        A[rng.permutation(n + m)[:n], p] = 1
    return A


def pooled_base2(D):
    """Mean squared distance over the pairs i != j."""
    N = D.shape[0]
    return (D.sum() - np.trace(D)) / (N * (N - 1))


def kernel_matrix(D, scales, base2):
    """(N, N) Gaussian mixture on squared distances D, diagonal set to 0 (every sum below runs over i != j)."""
    K = np.zeros_like(D)
    for c in scales:
        K += np.exp(-D / (c * base2))
    K /= len(scales)
    np.fill_diagonal(K, 0.0)
    return K


def quadforms(K, A):
    """(quad (P), rowsum (N), col0 (N)) of the engine's contract from the (zero-diagonal) kernel matrix."""
    A = A.astype(np.float64)
    return np.einsum("ip,ip->p", A, K @ A), K.sum(axis=1), K @ A[:, 0]


def mmd2_direct(K, A):
    """(P,) unbiased MMD^2 by its definition: the three sums over the index sets of every column."""
    out = np.empty(A.shape[1])
    for p in range(A.shape[1]):
        X, Y = np.flatnonzero(A[:, p] == 1), np.flatnonzero(A[:, p] == 0)
        n, m = len(X), len(Y)
        xx = K[np.ix_(X, X)].sum() / (n * (n - 1)) if n > 1 else 0.0
        yy = K[np.ix_(Y, Y)].sum() / (m * (m - 1)) if m > 1 else 0.0
        out[p] = xx + yy - 2.0 * K[np.ix_(X, Y)].sum() / (n * m)
    return out


def mmd2_from_sums(quad, rowsum, A):
    """The same from (quad, rowsum): xy = A.rowsum - quad, yy = S - 2 A.rowsum + quad."""
    A = A.astype(np.float64)
    n = A.sum(axis=0)
    m = A.shape[0] - n
    ar = A.T @ rowsum
    pairs_x, pairs_y = np.maximum(n * (n - 1), 1.0), np.maximum(m * (m - 1), 1.0)
    return (quad * (n > 1)) / pairs_x + ((rowsum.sum() - 2.0 * ar + quad) * (m > 1)) / pairs_y - 2.0 * (ar - quad) / (n * m)


def p_value(mmd2):
    return (1 + int(np.sum(mmd2[1:] >= mmd2[0]))) / len(mmd2)


def witness(K, a0):
    """mean_{x' != i} k(z_i, x') - mean_{y' != i} k(z_i, y') for the split a0."""
    a0 = a0.astype(np.float64)
    n, m = a0.sum(), len(a0) - a0.sum()
    to_x, to_y = K @ a0, K @ (1.0 - a0)
    return to_x / np.maximum(n - a0, 1.0) - to_y / np.maximum(m - (1.0 - a0), 1.0)


def group_rows(N):
    """Rows of the longest fp32 addition chain of the engine: 128 * min(16, max(1, tiles / 16)), tiles = ceil(N / 128)."""
    tiles = -(-N // 128)
    return 128 * min(16, max(1, tiles // 16))


def restate_f32(z, A, scales, base2):
    """(quad, rowsum, col0) as the engine forms them, in numpy float32: rows centred by the f32-rounded mean, norms, the expansion
    ||a||^2 + ||b||^2 - 2 a.b clamped at 0, exp2 on d2 * f32(-log2 e / (c base2)) summed over the scales, the diagonal zeroed by
    index and the product with the memberships accumulated in f32; only the last sum over the owned rows and 1/Q are float64."""
    z = flat(z).astype(np.float32)
    mean = z.astype(np.float64).mean(axis=0).astype(np.float32)
    zc = z - mean
    norm = (zc.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    d2 = np.maximum((norm[:, None] + norm[None, :]) - np.float32(2.0) * (zc @ zc.T), np.float32(0.0))
    K = np.zeros_like(d2)
    for c in scales:
        K = K + np.exp2(d2 * np.float32(-np.log2(np.e) / (c * base2)))
    np.fill_diagonal(K, np.float32(0.0))
    assert K.dtype == np.float32
    Af = A.astype(np.float32)
    T = (K @ np.concatenate([Af, np.ones((len(Af), 1), np.float32)], axis=1)).astype(np.float64)
    q = float(len(scales))
    return (A.astype(np.float64) * T[:, :-1]).sum(axis=0) / q, T[:, -1] / q, T[:, 0] / q


def error_bounds(z, A, scales, base2, K):
    """(quad (P), rowsum (N), col0 (N)) worst-case errors of the engine's contract: eps_ij = delta_ij / (min_q c_q base2) + 8 u per
    pair (delta: the expansion error, knn_ref.expansion_bound) and c u of the value for the fp32 chain of c additions."""
    z = flat(z)
    eps = expansion_bound(z, z) / (min(scales) * base2) + 8.0 * U
    np.fill_diagonal(eps, 0.0)
    Af = A.astype(np.float64)
    quad, rowsum, col0 = quadforms(K, A)
    c = group_rows(z.shape[0])
    return (np.einsum("ip,ip->p", Af, eps @ Af) + c * U * quad, eps.sum(axis=1) + c * U * rowsum, eps @ Af[:, 0] + c * U * col0)

