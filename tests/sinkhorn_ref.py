"""Float64 brute-force restatement of the entropic optimal transport of utils/sinkhorn.py (csrc/fd_sinkhorn.hip): the soft-min, the
alternating and the symmetric Sinkhorn iterations, the debiased divergence and the marginal error on the full (n, m) matrix of
direct differences -- the thing the engine must not build, and small enough here.  `softmin_f32` is the engine's arithmetic
(centred expansion, one scaled exponent per pair, running (max, sum) per half-wave and group) in numpy float32; `error_bounds` is
the worst-case bound of one pass that the engine's contract states."""
import numpy as np

from tests.knn_ref import U, dist2, flat

LOG2E = 1.4426950408889634074


def uniform(n):
    return np.full(n, 1.0 / n)


def eps_base(x, y=None):
    """Mean squared distance over the pairs i != j of the pooled rows (of x alone when y is None), by its definition; 1 when it is 0."""
    z = flat(x) if y is None else np.concatenate([flat(x), flat(y)])
    N = z.shape[0]
    if N < 2:
        return 1.0
    D = dist2(z, z)
    base = (D.sum() - np.trace(D)) / (N * (N - 1))
    return base if base > 0 else 1.0


def softmin(D, h, eps):
    """out_i = -eps log sum_j exp((h_j - D_ij) / eps), stabilised by the row maximum."""
    t = (np.asarray(h, dtype=np.float64)[None, :] - D) / eps
    top = t.max(axis=1)
    return -eps * (top + np.log(np.exp(t - top[:, None]).sum(axis=1)))


def potentials(D, a, b, eps_list):
    """(f, g): f <- softmin_Y(g + eps log b), g <- softmin_X(f + eps log a) per entry of eps_list, from g = 0."""
    f, g = np.zeros(D.shape[0]), np.zeros(D.shape[1])
    la, lb = np.log(a), np.log(b)
    for eps in eps_list:
        f = softmin(D, g + eps * lb, eps)
        g = softmin(D.T, f + eps * la, eps)
    return f, g


def potentials_symmetric(D, a, eps_list):
    """p <- (p + softmin_X(p + eps log a)) / 2 per entry of eps_list, from p = 0."""
    p = np.zeros(D.shape[0])
    la = np.log(a)
    for eps in eps_list:
        p = 0.5 * (p + softmin(D, p + eps * la, eps))
    return p


def marginal_error(D, f, g, a, b, eps):
    """sum_i a_i |exp((f_i - softmin_Y(g)_i) / eps) - 1|: how far the first marginal of the plan of (f, g) is from a."""
    return float((a * np.abs(np.exp((f - softmin(D, g + eps * np.log(b), eps)) / eps) - 1.0)).sum())


def divergence(x, y, eps_list, a=None, b=None):
    """Everything of the debiased Sinkhorn divergence S = <a, f - p_x> + <b, g - p_y> at the absolute schedule eps_list."""
    x, y = flat(x), flat(y)
    a = uniform(x.shape[0]) if a is None else np.asarray(a, dtype=np.float64)
    b = uniform(y.shape[0]) if b is None else np.asarray(b, dtype=np.float64)
    Dxy = dist2(x, y)
    f, g = potentials(Dxy, a, b, eps_list)
    px, py = potentials_symmetric(dist2(x, x), a, eps_list), potentials_symmetric(dist2(y, y), b, eps_list)
    cost_x, cost_y = f - px, g - py
    div = float(a @ cost_x + b @ cost_y)
    return dict(divergence=div, w2=float(np.sqrt(max(div, 0.0))), ot_xy=float(a @ f + b @ g), f=f, g=g, px=px, py=py,
                cost_x=cost_x, cost_y=cost_y, marginal_error=marginal_error(Dxy, f, g, a, b, eps_list[-1]), eps=float(eps_list[-1]))


def assignment_cost(x, y):
    """min over permutations of mean_i ||x_i - y_perm(i)||^2 (n = m small): the unregularised transport cost of uniform weights."""
    from itertools import permutations
    D = dist2(x, y)
    n = D.shape[0]
    return min(sum(D[i, p[i]] for i in range(n)) for p in permutations(range(n))) / n


def w2_sorted(x, y):
    """W2 of two 1-D samples of the same size and uniform weights: sorted quantiles."""
    return float(np.sqrt(np.mean((np.sort(np.ravel(x)) - np.sort(np.ravel(y))) ** 2)))


# ---------------------------------------------------------------------------------------------- the engine's arithmetic
def group_tiles(m):
    """Streamed tiles of a group: min(16, max(1, tiles / 16)), tiles = ceil(m / 128)."""
    tiles = -(-m // 128)
    return min(16, max(1, tiles // 16))


def chain_length(m):
    """The longest fp32 addition chain of a pass over m streamed rows: 64 rows of each of a group's tiles in a lane, plus the
    other half-wave's sum."""
    return 64 * group_tiles(m) + 1


def centred_f32(x, y, same=False):
    """Both sets centred by the f32-rounded mean of the pooled rows (of x alone when the sets are one), and the f32 norms (double
    sums of the f32 values' squares)."""
    x, y = flat(x).astype(np.float32), flat(y).astype(np.float32)
    mean = (x if same else np.concatenate([x, y])).astype(np.float64).mean(axis=0).astype(np.float32)
    xc, yc = x - mean, y - mean
    return xc, yc, (xc.astype(np.float64) ** 2).sum(axis=1).astype(np.float32), (yc.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)


def softmin_f32(xc, yc, xn, yn, h, eps):
    """One pass as the engine forms it, in numpy float32, on centred rows: d2 = max(0, (||x||^2 + ||y||^2) - 2 x.y), the exponent
    d2 * -s + f32(h s) with s = f32(log2 e / eps), -inf in the padding; per half-wave (streamed rows with (row % 8) // 4 equal) a
    running (max, sum) over the tiles of a group in f32, where the maximum that is subtracted is 0 while it is -inf; the half-waves
    merged at the end of the group, the groups merged in group order in float64."""
    f32 = np.float32
    s = f32(LOG2E / eps)
    hs = (np.asarray(h, dtype=np.float64) * np.float64(s)).astype(f32)
    d2 = np.maximum((xn[:, None] + yn[None, :]) - f32(2.0) * (xc @ yc.T), f32(0.0))
    e = d2 * (-s) + hs[None, :]
    assert e.dtype == np.float32
    n, m = e.shape
    gt = group_tiles(m)
    G = -(-m // (128 * gt))
    ep = np.full((n, G * gt * 128), -np.inf, f32)
    ep[:, :m] = e
    e6 = ep.reshape(n, G, gt, 16, 2, 4)
    halves = []
    for half in (0, 1):
        mx, sm = np.full((n, G), -np.inf, f32), np.zeros((n, G), f32)
        for k in range(gt):
            et = e6[:, :, k, :, half, :].reshape(n, G, 64)
            top = np.maximum(mx, et.max(axis=2))
            sub = np.where(np.isinf(top), f32(0.0), top)
            sm = sm * np.exp2(mx - sub) + np.exp2(et - sub[:, :, None]).sum(axis=2, dtype=f32)
            mx = top
        assert sm.dtype == np.float32
        halves.append((mx, sm))
    (m0, s0), (m1, s1) = halves
    both = np.maximum(m0, m1)
    bsub = np.where(np.isinf(both), f32(0.0), both)
    gs = (s0 * np.exp2(m0 - bsub) + s1 * np.exp2(m1 - bsub)).astype(np.float64)
    both = both.astype(np.float64)
    M, S = both[:, 0], gs[:, 0]
    for z in range(1, G):
        top = np.maximum(M, both[:, z])
        S = S * np.exp2(M - top) + gs[:, z] * np.exp2(both[:, z] - top)
        M = top
    return -eps * np.log(2.0) * (M + np.log2(S))


def potentials_f32(x, y, a, b, eps_list):
    """The alternating iteration on softmin_f32: (f, g)."""
    xc, yc, xn, yn = centred_f32(x, y)
    f, g = np.zeros(len(xc)), np.zeros(len(yc))
    la, lb = np.log(a), np.log(b)
    for eps in eps_list:
        f = softmin_f32(xc, yc, xn, yn, g + eps * lb, eps)
        g = softmin_f32(yc, xc, yn, xn, f + eps * la, eps)
    return f, g


def potentials_symmetric_f32(x, a, eps_list):
    x = flat(x).astype(np.float32)
    xc = x - x.astype(np.float64).mean(axis=0).astype(np.float32)
    xn = (xc.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    p, la = np.zeros(len(xc)), np.log(a)
    for eps in eps_list:
        p = 0.5 * (p + softmin_f32(xc, xc, xn, xn, p + eps * la, eps))
    return p


# ---------------------------------------------------------------------------------------------- the contract
def expansion_bound_pooled(x, y, same=False):
    """delta (n, m) of knn_ref.expansion_bound with mu the mean of the pooled rows (of x alone when the sets are one)."""
    x, y = flat(x), flat(y)
    mu = x.mean(axis=0) if same else np.concatenate([x, y]).mean(axis=0)
    xn, yn = ((x - mu) ** 2).sum(axis=1), ((y - mu) ** 2).sum(axis=1)
    return 2.0 * (x.shape[1] + 3) * U * (xn[:, None] + yn[None, :])


def error_bounds(x, y, h, eps, D=None, same=False):
    """(n,) worst-case error of one engine pass out_i = softmin over the rows of y of h, u = 2^-24.

    The soft-min is 1-Lipschitz in its exponents t_ij = h_j - d2_ij under the sup norm over j, so the error of out_i is at most the
    largest perturbation of a t_ij plus eps times the relative error of the sum.

    Exponent.  The engine forms e = fl(d2~ * -s + hs_j) with s = fl(log2 e / eps) = (log2 e / eps)(1 + t0), hs_j = fl(h_j s) =
    h_j s (1 + t1) (h_j and the product in double), one fma rounding (1 + t2), all |t| <= u.  So
      e / (log2 e / eps) - t_ij = -(d2~ - d2) + t1 h_j + (t0 + t2)(h_j - d2~)    to first order,
    at most delta_ij + u |h_j| + 2 u |t_ij| with delta the expansion error (clamping d2~ at 0 only moves it towards d2 >= 0).  The
    subtraction of the running maximum rounds once more: u |e_j - max| <= 2 u max_j |e_j|; the rescalings of the running sum by
    exp2(old max - new max) telescope, since the maximum only grows: together at most another 2 u max_j |e_j|.  In all
      max_j (delta_ij + u |h_j|) + 6 u max_j |t_ij|.
    Sum.  Relative error of the sum: 2 u per v_exp_f32 (one ulp), c u for the fp32 chain of c = 64 gt + 1 additions
    (chain_length), and (1 + 2) u for each of the at most gt + 2 rescalings and hand-overs (a product and an exponential): (2 + c +
    3 (gt + 2)) u = (67 gt + 9) u.  The merge of the groups, the logarithm and the product with eps are float64."""
    x, y = flat(x), flat(y)
    D = dist2(x, y) if D is None else D
    t = np.abs(np.asarray(h, dtype=np.float64)[None, :] - D)
    expo = (expansion_bound_pooled(x, y, same) + U * np.abs(h)[None, :]).max(axis=1) + 6.0 * U * t.max(axis=1)
    gt = group_tiles(y.shape[0])
    return expo + eps * (2 + chain_length(y.shape[0]) + 3 * (gt + 2)) * U


def potentials_with_bounds(x, y, a, b, eps_list, D=None):
    """(f, g, bound on f, bound on g): the alternating iteration in float64 and, in the sup norm, the sum of the per-pass bounds
    along it (each pass is non-expansive in h under the sup norm)."""
    x, y = flat(x), flat(y)
    D = dist2(x, y) if D is None else D
    f, g = np.zeros(D.shape[0]), np.zeros(D.shape[1])
    la, lb = np.log(a), np.log(b)
    total = bf = 0.0
    for eps in eps_list:
        total += error_bounds(x, y, g + eps * lb, eps, D).max()
        f = softmin(D, g + eps * lb, eps)
        bf = total
        total += error_bounds(y, x, f + eps * la, eps, D.T).max()
        g = softmin(D.T, f + eps * la, eps)
    return f, g, bf, total


def symmetric_with_bound(x, a, eps_list, D=None):
    """(p, bound on p) for p <- (p + softmin(p)) / 2: the averaged step is non-expansive too, and adds half a pass bound."""
    x = flat(x)
    D = dist2(x, x) if D is None else D
    p, la, total = np.zeros(D.shape[0]), np.log(a), 0.0
    for eps in eps_list:
        total += 0.5 * error_bounds(x, x, p + eps * la, eps, D, same=True).max()
        p = 0.5 * (p + softmin(D, p + eps * la, eps))
    return p, total


def eps_base_closed(x, y=None):
    """eps_base in its closed form 2 sum ||z_i - mean||^2 / (N - 1) (no (N, N) matrix)."""
    z = flat(x) if y is None else np.concatenate([flat(x), flat(y)])
    ss = ((z - z.mean(axis=0)) ** 2).sum()
    return 2.0 * ss / (len(z) - 1) if len(z) > 1 and ss > 0 else 1.0
