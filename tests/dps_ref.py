"""Float64 restatement of gradient-guided conditional sampling (DiffusionSampler.impute(conditioning="dps"), csrc/fd_dps.hip),
built from the oracle's dft, idft, marginal_prob, sde_step and score_forward and tests/impute_ref.py's maps.  Per row and step
t_i -> t_{i+1}, (alpha, s) the perturbation kernel at t_i:

    x0_hat = (x + s^2 G^2 . score) / alpha
    r      = m . idft(sigma . (x0_obs - x0_hat))          (no Fourier: m . sigma . (x0_obs - x0_hat))
    u      = sigma . idft^T(r)                            (no Fourier: sigma . r)
    dx     = J^T (s^2 G^2 . u)                            (0 without the Jacobian)
    g      = (2 / alpha) (u + dx)                         = -grad_x ||r||^2
    x'     = sde_step(x, score, z) + (zeta / ||r||) g     (0 where ||r|| = 0)

J^T v comes from (J^T v)_j = <v, J e_j>, J e_j by central differences (tests/likelihood_ref.jvp).  score_fn(x, t) -> (B,T,C): every
row's score depends on that row alone.  Shared by tests/test_dps_cpu.py and tests/test_gpu_dps.py."""
import numpy as np

from oracle import fdiff_oracle as O
from tests import likelihood_ref as L


def coef(sde, t):
    """(alpha, s) at t from the oracle's marginal_prob (the std of frequency k is s G_k)."""
    mean, std = O.marginal_prob(sde, np.ones((1, 1, 1)), np.array([float(t)]))
    return float(mean.ravel()[0]), float(std[0, 0] / sde.G[0])


def inv_rho(T):
    """1 / rho_k of the packed rows: 1 at DC and Nyquist (T even), 2 elsewhere."""
    w = np.full(T, 2.0)
    w[0] = 1.0
    if T % 2 == 0:
        w[T // 2] = 1.0
    return w


def idft_adjoint(r):
    """idft^T = diag(1/rho) F: the packed DFT of r with every row k scaled by 1 / rho_k."""
    r = np.asarray(r, dtype=np.float64)
    return O.dft(r) * inv_rho(r.shape[1])[None, :, None]


def residual(x, score, x0, m, sigma, G, alpha, s, fourier):
    """(r, u) of one evaluation; m (B,T,C) or (T,C)."""
    x = np.asarray(x, dtype=np.float64)
    sg2 = (s * s) * (np.asarray(G, dtype=np.float64) ** 2)[None, :, None]
    x0h = (x + sg2 * np.asarray(score, dtype=np.float64)) / alpha
    d = sigma[None] * (np.asarray(x0, dtype=np.float64) - x0h)
    m = np.broadcast_to(np.asarray(m, dtype=bool), x.shape)
    r = np.where(m, O.idft(d) if fourier else d, 0.0)
    u = sigma[None] * (idft_adjoint(r) if fourier else r)
    return r, u


def vjp(score_fn, x, t, v, rel=1e-7):
    """J^T v per row, J = d score / d x, over the T*C basis directions (all rows at once); rel: the step of likelihood_ref.jvp
    (a score linear in x takes any step exactly)."""
    x = np.asarray(x, dtype=np.float64)
    B, T, C = x.shape
    out = np.zeros_like(x)
    for k in range(T * C):
        e = np.zeros((T, C))
        e.flat[k] = 1.0
        je = L.jvp(score_fn, x, t, np.broadcast_to(e, x.shape), rel)
        out.reshape(B, -1)[:, k] = (v * je).sum(axis=(1, 2))
    return out


def guidance(score_fn, sde, x, t, x0, m, sigma, fourier, jacobian=True, score=None, rel=1e-7, vjp_fn=None):
    """(g, ||r||^2 per row, score) at (x, t); score: the evaluation's score if the caller has it.  vjp_fn(x, t, v) -> J^T v replaces
    the central differences (tests/autograd_ref.vjp_fn: exact, and affordable at any shape)."""
    alpha, s = coef(sde, t)
    x = np.asarray(x, dtype=np.float64)
    score = score_fn(x, t) if score is None else score
    r, u = residual(x, score, x0, m, sigma, sde.G, alpha, s, fourier)
    v = (s * s) * (sde.G ** 2)[None, :, None] * u
    dx = (vjp(score_fn, x, t, v, rel) if vjp_fn is None else vjp_fn(x, t, v)) if jacobian else 0.0
    return (2.0 / alpha) * (u + dx), (r * r).sum(axis=(1, 2)), score


def rnorm2(score_fn, sde, x, t, x0, m, sigma, fourier):
    """||r(x)||^2 per row: the objective g is minus the gradient of."""
    alpha, s = coef(sde, t)
    r, _ = residual(x, score_fn(x, t), x0, m, sigma, sde.G, alpha, s, fourier)
    return (r * r).sum(axis=(1, 2))


def step(score_fn, sde, X, t, dt, z, x0, m, sigma, fourier, zeta, jacobian=True, vjp_fn=None):
    """One guided reverse step from X at t with predictor noise z."""
    g, rn2, score = guidance(score_fn, sde, X, float(t), x0, m, sigma, fourier, jacobian, vjp_fn=vjp_fn)
    nr = np.sqrt(rn2)
    c = np.where(nr > 0, zeta / np.where(nr > 0, nr, 1.0), 0.0)
    return O.sde_step(sde, score, float(t), X, z, float(dt)) + c[:, None, None] * g


def trajectory(score_fn, sde, z_prior, z_steps, x0, m, sigma, fourier, zeta, jacobian=True, eps=1e-5, vjp_fn=None):
    """impute(conditioning="dps") for one batch from injected prior / predictor noise; x0 (B,T,C) per state row."""
    N = len(z_steps)
    ts, dt = O.timesteps(N, eps)
    X = O.prior_sampling(sde, z_prior)
    for i, t in enumerate(ts):
        X = step(score_fn, sde, X, t, dt, z_steps[i], x0, m, sigma, fourier, zeta, jacobian, vjp_fn)
    return X


def grad_fd(fn, x, rel=1e-6):
    """Central-difference gradient of the per-row objective fn(x) -> (B,), all rows at once."""
    x = np.asarray(x, dtype=np.float64)
    B, T, C = x.shape
    h = rel * max(1.0, float(np.abs(x).max()))
    out = np.zeros_like(x)
    for k in range(T * C):
        e = np.zeros((T, C))
        e.flat[k] = h
        out.reshape(B, -1)[:, k] = (fn(x + e[None]) - fn(x - e[None])) / (2.0 * h)
    return out

