"""Float64 restatement of class-conditional conditional sampling and likelihood (DiffusionSampler.impute / impute_guidance /
log_likelihood with y and cfg_scale; csrc/fd_impute.hip, csrc/fd_dps.hip in their paired forms), built from the pieces that exist:
the guided score of tests/cfg_ref.py, the projection of tests/impute_ref.py, the guidance of tests/dps_ref.py (both take a score
function) and the likelihood of tests/likelihood_ref.py.  No oracle change.  Shared by tests/test_cfg_impute_cpu.py and
tests/test_gpu_cfg_impute.py.
"""
import numpy as np

from oracle import fdiff_oracle as O
from tests import cfg_ref as C
from tests import dps_ref as D
from tests import impute_ref as I

CFG_WIDE = dict(T=8, C=20, D=72, L=2, H=12)      # two channel blocks of 16: the paired write-back of the second block
CFG_LL = dict(T=8, C=3, D=8, L=2, H=4)           # the exact-estimator shape of tests/test_gpu_likelihood.py
Y_MIXED = [0, 2, 3, 0, 2]                        # class 1 absent, one null row
Y_CLASSES = [0, 2, 1, 0, 2]
W_GUIDE = 1.7


def shifted(sd, tab, k):
    """The unlabelled weights that ARE the labelled network on label k: table[k] added to time_encoder.dense.bias (float64)."""
    p = dict(sd)
    p["time_encoder.dense.bias"] = np.asarray(sd["time_encoder.dense.bias"], dtype=np.float64) + np.asarray(tab[k], dtype=np.float64)
    return p


def conditioning(T, Cn, B, mask_kind, seed, fourier, standardize=True):
    """mu, sigma (f32-representable; zeros / ones without standardisation), observations (NaN where hidden), the mask -- (B,T,C)
    per series for "random", one shared (T,C) forecast mask for "forecast" -- and x0_obs in float64."""
    rs = np.random.RandomState(seed)
    mu = (0.3 * rs.randn(T, Cn)).astype(np.float32).astype(np.float64)
    sigma = rs.uniform(0.5, 2.0, (T, Cn)).astype(np.float32).astype(np.float64)
    if not standardize:
        mu, sigma = np.zeros((T, Cn)), np.ones((T, Cn))
    y = (np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(B, T, Cn)).astype(np.float32)
    if mask_kind == "random":
        m = rs.rand(B, T, Cn) < 0.5
    else:
        m = np.ones((T, Cn), bool)
        m[-max(1, T // 4):] = False
    mb = np.broadcast_to(m, y.shape)
    yn = np.where(mb, y, np.nan).astype(np.float32)
    return mu, sigma, yn, m, I.x0_obs(yn, mb, mu, sigma, fourier)


def replace_trajectory(sd, tab, sde, z_prior, z_steps, z_obs, x0, m, sigma, fourier, y, w, n_head, eps=1e-5):
    """impute(conditioning="replace", y, cfg_scale=w) for one batch: O.sde_step on the guided score, then impute_ref.project at
    t_{i+1} (the last one exact) -- impute_ref.impute_trajectory with cfg_ref.guided_score_fn in place of the oracle forward."""
    fn = C.guided_score_fn(sd, tab, y, w, n_head)
    N = len(z_steps)
    ts, dt = O.timesteps(N, eps)
    X = O.prior_sampling(sde, z_prior)
    for i, t in enumerate(ts):
        X = O.sde_step(sde, fn(X, float(t)), float(t), X, z_steps[i], float(dt))
        if i + 1 < N:
            alpha, s = D.coef(sde, float(ts[i + 1]))
            X = I.project(X, x0, m, sigma, sde.G, alpha, s, z_obs[i], fourier)
        else:
            X = I.project(X, x0, m, sigma, sde.G, 1.0, 0.0, np.zeros_like(X), fourier)
    return X


def dps_guidance(sd, tab, sde, x, t, x0, m, sigma, fourier, y, w, n_head, jacobian):
    """(g, ||r||^2) of impute_guidance(y, cfg_scale=w): dps_ref.guidance on the guided score."""
    g, rn2, _ = D.guidance(C.guided_score_fn(sd, tab, y, w, n_head), sde, x, t, x0, m, sigma, fourier, jacobian)
    return g, rn2


def dps_trajectory(sd, tab, sde, z_prior, z_steps, x0, m, sigma, fourier, zeta, y, w, n_head, jacobian):
    """impute(conditioning="dps", y, cfg_scale=w) for one batch: dps_ref.trajectory on the guided score (y None and w = 1: the
    unguided loop of the model run unconditionally)."""
    return D.trajectory(C.guided_score_fn(sd, tab, y, w, n_head), sde, z_prior, z_steps, x0, m, sigma, fourier, zeta, jacobian)
