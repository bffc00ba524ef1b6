"""Float64 restatement of conditional sampling on a dense linear observation (DiffusionSampler.impute(operator=P),
csrc/fd_linop.hip), built on tests/impute_ref.py and tests/dps_ref.py in the manner of tests/aggregate_ref.py.  Per channel y = P v,
Pm (M, T) of full row rank, Pp = pinv(Pm):

    x0_obs = A^-1(P^+ where(m, y, 0))
    replace: x' = x + dft(P^+ (m . P idft(sigma . d))) / sigma          (no Fourier: x + P^+ (m . P (sigma . d)) / sigma)
    dps:     r  = m . P idft(sigma . (x0_obs - x0_hat)),  u = sigma . idft^T(P^T r)     (no Fourier: P for P idft, u = sigma . P^T r)

Arrays are (B, T, C) at full resolution and (B, M, C) over the operator's rows; m is (B, M, C) or (M, C).  Shared by
tests/test_linop_cpu.py and tests/test_gpu_linop.py."""
import numpy as np

from oracle import fdiff_oracle as O
from tests import dps_ref as D
from tests import impute_ref as I


def pinv(Pm):
    return np.linalg.pinv(np.asarray(Pm, dtype=np.float64))


def P(v, Pm):
    """(B, T, C) -> (B, M, C)."""
    return np.einsum("mt,btc->bmc", np.asarray(Pm, dtype=np.float64), np.asarray(v, dtype=np.float64))


def P_pinv(r, Pm):
    """(B, M, C) -> (B, T, C)."""
    return np.einsum("tm,bmc->btc", pinv(Pm), np.asarray(r, dtype=np.float64))


def P_T(r, Pm):
    """The adjoint of P: (B, M, C) -> (B, T, C)."""
    return np.einsum("mt,bmc->btc", np.asarray(Pm, dtype=np.float64), np.asarray(r, dtype=np.float64))


def x0_obs(y, m, mu, sigma, fourier, Pm):
    """A^-1(P^+ where(m, y, 0)); y, m over the operator's rows, NaN at unobserved rows of y is ignored."""
    T = mu.shape[0]
    y0 = np.where(np.broadcast_to(m, np.shape(y)), np.asarray(y, dtype=np.float64), 0.0)
    return I.x0_obs(P_pinv(y0, Pm), np.ones((1, T, 1), bool), mu, sigma, fourier)


def project(x, x0, m, sigma, G, alpha, s, z, fourier, Pm):
    x = np.asarray(x, dtype=np.float64)
    d = alpha * np.asarray(x0, dtype=np.float64) + s * np.asarray(G, dtype=np.float64)[None, :, None] * z - x
    sd = sigma[None] * d
    pm = P(O.idft(sd) if fourier else sd, Pm)
    v = P_pinv(np.where(np.broadcast_to(m, pm.shape), pm, 0.0), Pm)
    return x + (O.dft(v) if fourier else v) / sigma[None]


def impute_trajectory(p, sde, z_prior, z_steps, z_obs, x0, m, sigma, fourier, n_head, Pm, eps=1e-5):
    """impute_ref.impute_trajectory with the operator's projection behind every step."""
    N = len(z_steps)
    ts, dt = O.timesteps(N, eps)
    X = O.prior_sampling(sde, z_prior)
    B = X.shape[0]
    for i, t in enumerate(ts):
        score = O.score_forward(p, X, np.full((B,), t, dtype=np.float32), n_head)
        X = O.sde_step(sde, score, float(t), X, z_steps[i], float(dt))
        if i + 1 < N:
            alpha, s = D.coef(sde, ts[i + 1])
            X = project(X, x0, m, sigma, sde.G, alpha, s, z_obs[i], fourier, Pm)
        else:
            X = project(X, x0, m, sigma, sde.G, 1.0, 0.0, np.zeros_like(X), fourier, Pm)
    return X


def residual(x, score, x0, m, sigma, G, alpha, s, fourier, Pm):
    """(r (B,M,C), u (B,T,C)) of one evaluation."""
    x = np.asarray(x, dtype=np.float64)
    sg2 = (s * s) * (np.asarray(G, dtype=np.float64) ** 2)[None, :, None]
    x0h = (x + sg2 * np.asarray(score, dtype=np.float64)) / alpha
    d = sigma[None] * (np.asarray(x0, dtype=np.float64) - x0h)
    pm = P(O.idft(d) if fourier else d, Pm)
    r = np.where(np.broadcast_to(m, pm.shape), pm, 0.0)
    pt = P_T(r, Pm)
    return r, sigma[None] * (D.idft_adjoint(pt) if fourier else pt)


def guidance(score_fn, sde, x, t, x0, m, sigma, fourier, Pm, jacobian=True, score=None, vjp_fn=None):
    """(g, ||r||^2 per row, score) at (x, t), as dps_ref.guidance."""
    alpha, s = D.coef(sde, t)
    x = np.asarray(x, dtype=np.float64)
    score = score_fn(x, t) if score is None else score
    r, u = residual(x, score, x0, m, sigma, sde.G, alpha, s, fourier, Pm)
    v = (s * s) * (sde.G ** 2)[None, :, None] * u
    dx = (D.vjp(score_fn, x, t, v) if vjp_fn is None else vjp_fn(x, t, v)) if jacobian else 0.0
    return (2.0 / alpha) * (u + dx), (r * r).sum(axis=(1, 2)), score


def rnorm2(score_fn, sde, x, t, x0, m, sigma, fourier, Pm):
    alpha, s = D.coef(sde, t)
    r, _ = residual(x, score_fn(x, t), x0, m, sigma, sde.G, alpha, s, fourier, Pm)
    return (r * r).sum(axis=(1, 2))


def trajectory(score_fn, sde, z_prior, z_steps, x0, m, sigma, fourier, zeta, Pm, jacobian=True, eps=1e-5, vjp_fn=None):
    """impute(conditioning="dps", operator=P) for one batch from injected prior / predictor noise."""
    N = len(z_steps)
    ts, dt = O.timesteps(N, eps)
    X = O.prior_sampling(sde, z_prior)
    for i, t in enumerate(ts):
        g, rn2, score = guidance(score_fn, sde, X, float(t), x0, m, sigma, fourier, Pm, jacobian, vjp_fn=vjp_fn)
        nr = np.sqrt(rn2)
        c = np.where(nr > 0, zeta / np.where(nr > 0, nr, 1.0), 0.0)
        X = O.sde_step(sde, score, float(t), X, z_steps[i], float(dt)) + c[:, None, None] * g
    return X
