"""Float64 restatement of conditional sampling (DiffusionSampler.impute, csrc/fd_impute.hip), built from the oracle's dft, idft,
marginal_prob, sde_step and score_forward.  Shared by tests/test_impute_cpu.py and tests/test_gpu_impute.py."""
import numpy as np

from oracle import fdiff_oracle as O


def forward_map(x, mu, sigma, fourier):
    """A(x): sample space -> data-scale time domain."""
    y = sigma[None] * np.asarray(x, dtype=np.float64) + mu[None]
    return O.idft(y) if fourier else y


def x0_obs(y, m, mu, sigma, fourier):
    """A^-1(where(m, y, 0)); NaN at unobserved entries of y is ignored."""
    y0 = np.where(m, np.asarray(y, dtype=np.float64), 0.0)
    return ((O.dft(y0) if fourier else y0) - mu[None]) / sigma[None]


def project(x, x0, m, sigma, G, alpha, s, z, fourier):
    """x' = x + dft(m . idft(sigma . d)) / sigma (fourier) or x + m . d, d = alpha x0 + s G z - x; m (B,T,C) or (T,C)."""
    x = np.asarray(x, dtype=np.float64)
    d = alpha * np.asarray(x0, dtype=np.float64) + s * np.asarray(G, dtype=np.float64)[None, :, None] * z - x
    m = np.broadcast_to(np.asarray(m, dtype=bool), x.shape)
    if not fourier:
        return x + np.where(m, d, 0.0)
    return x + O.dft(np.where(m, O.idft(sigma[None] * d), 0.0)) / sigma[None]


def impute_trajectory(p, sde, z_prior, z_steps, z_obs, x0, m, sigma, fourier, n_head, eps=1e-5):
    """O.sample_trajectory with the projection behind every step: at t_{i+1} (alpha, s of marginal_prob), the last one exact."""
    N = len(z_steps)
    ts, dt = O.timesteps(N, eps)
    X = O.prior_sampling(sde, z_prior)
    B = X.shape[0]
    for i, t in enumerate(ts):
        score = O.score_forward(p, X, np.full((B,), t, dtype=np.float32), n_head)
        X = O.sde_step(sde, score, float(t), X, z_steps[i], float(dt))
        if i + 1 < N:
            mean, std = O.marginal_prob(sde, np.ones((1, 1, 1)), np.array([float(ts[i + 1])]))
            alpha, s = float(mean.ravel()[0]), float(std[0, 0] / sde.G[0])
            X = project(X, x0, m, sigma, sde.G, alpha, s, z_obs[i], fourier)
        else:
            X = project(X, x0, m, sigma, sde.G, 1.0, 0.0, np.zeros_like(X), fourier)
    return X
