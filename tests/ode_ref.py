"""Float64 restatement of the probability-flow ODE sampler (SDE.ode_drift, DiffusionSampler.sample_ode / encode / decode,
csrc/fd_ode.hip), built from the oracle's SDE parameters and score networks.  Shared by tests/test_ode_cpu.py and
tests/test_gpu_ode.py."""
import math

import numpy as np

from oracle import fdiff_oracle as O


def coef(sde, t):
    """(a, g) of the SDE at t: VP a = beta/2, g = sqrt(beta); VE a = 0, g = sigma_min sqrt(2 ln r) r^t (as O.sde_step)."""
    t = float(t)
    if sde.kind == "vp":
        beta = sde.p0 + t * (sde.p1 - sde.p0)
        return 0.5 * beta, math.sqrt(beta)
    r = sde.p1 / sde.p0
    return 0.0, sde.p0 * math.sqrt(2.0 * math.log(r)) * r ** t


def velocity(sde, score, t, x):
    """v = -a x - 0.5 (g G_k)^2 score on (B,T,C)."""
    a, g = coef(sde, t)
    gk = (g * sde.G)[None, :, None]
    return -a * np.asarray(x, dtype=np.float64) - 0.5 * (gk * gk) * np.asarray(score, dtype=np.float64)


def grid(N, to_noise=False, eps=1e-5):
    """torch.linspace(1, eps, N + 1) (sampling / decoding) or torch.linspace(eps, 1, N + 1) (encoding), float32."""
    return O.linspace_f32(eps, 1.0, N + 1) if to_noise else O.linspace_f32(1.0, eps, N + 1)


def solve(sde, score_fn, x, ts, solver="heun"):
    """Euler or Heun over the grid ts (N + 1 points, either direction); score_fn(x, t) -> score (B,T,C)."""
    x = np.asarray(x, dtype=np.float64)
    for i in range(len(ts) - 1):
        t0, t1 = float(ts[i]), float(ts[i + 1])
        h = t1 - t0
        v0 = velocity(sde, score_fn(x, t0), t0, x)
        if solver == "euler":
            x = x + h * v0
        else:
            xt = x + h * v0
            x = x + 0.5 * h * (v0 + velocity(sde, score_fn(xt, t1), t1, xt))
    return x


def model_score(p, backbone="transformer", n_head=None):
    """score_fn of an oracle network; every series gets the evaluation's t as a float32 (as the engine's t vector)."""
    def fn(x, t):
        tb = np.full((x.shape[0],), t, dtype=np.float32)
        if backbone == "mlp":
            return O.mlp_score_forward(p, x, tb)
        if backbone == "lstm":
            return O.lstm_score_forward(p, x, tb)
        return O.score_forward(p, x, tb, n_head)
    return fn


def sample_ode(p, sde, z_prior, N, solver, backbone="transformer", n_head=None, eps=1e-5):
    """DiffusionSampler.sample_ode for one batch from the injected prior draws z_prior (B,T,C)."""
    return solve(sde, model_score(p, backbone, n_head), O.prior_sampling(sde, z_prior), grid(N, False, eps), solver)
