"""Float64 restatement of the data-prediction exponential integrators of the probability-flow ODE (deterministic DDIM and
DPM-Solver++ 2M: SDE.dpm_step, DiffusionSampler.sample_ode(solver="ddim" / "dpmpp2m"), csrc/fd_ode.hip) and of the log-SNR step
grid, built from the oracle's SDE parameters and score networks.  Shared by tests/test_dpm_cpu.py and tests/test_gpu_dpm.py.

With (alpha, s) the perturbation kernel x_t = alpha x_0 + s G z and lambda = log(alpha / s), on a grid t_0 > ... > t_N:
    D_i     = (x_i + (s_i G_k)^2 score(x_i, t_i)) / alpha_i
    Dbar    = D_i                                      (DDIM; 2M at i = 0)
              (1 + 1/(2 r_i)) D_i - 1/(2 r_i) D_{i-1}  (2M, i >= 1; r_i = h_{i-1} / h_i, h_i = lambda_{i+1} - lambda_i)
    x_{i+1} = (s_{i+1} / s_i) x_i - alpha_{i+1} (exp(-h_i) - 1) Dbar
"""
import math

import numpy as np

from tests import ode_ref as R


def marginal(sde, t):
    """(alpha, s, lambda) at t in double; VP's s^2 = 1 - alpha^2 from expm1 (it cancels at small t)."""
    t = float(t)
    if sde.kind == "vp":
        lmc = -0.25 * t * t * (sde.p1 - sde.p0) - 0.5 * t * sde.p0
        s2 = -math.expm1(2.0 * lmc)
        return math.exp(lmc), math.sqrt(s2), lmc - 0.5 * math.log(s2)
    ls = math.log(sde.p0) + t * math.log(sde.p1 / sde.p0)
    return 1.0, math.exp(ls), -ls


def log_snr(sde, t):
    return marginal(sde, t)[2]


def t_of_log_snr(sde, lam):
    """The inverse of log_snr: VE affine; VP the positive root of 0.25 (b1 - b0) t^2 + 0.5 b0 t + lmc = 0."""
    lam = float(lam)
    if sde.kind == "vp":
        lmc = -0.5 * math.log1p(math.exp(-2.0 * lam))
        a, b = 0.25 * (sde.p1 - sde.p0), 0.5 * sde.p0
        return -2.0 * lmc / (b + math.sqrt(b * b - 4.0 * a * lmc))      # (the root, in the form that does not cancel at small t)
    return (-lam - math.log(sde.p0)) / math.log(sde.p1 / sde.p0)


def grid(sde, N, schedule="time", eps=1e-5):
    """The sampling grid, float32: "time" = linspace(1, eps, N + 1); "logsnr" = N + 1 points uniform in lambda, ends exactly 1, eps."""
    if schedule == "time":
        return R.grid(N, False, eps)
    l1, l0 = log_snr(sde, 1.0), log_snr(sde, eps)
    ts = [1.0] + [t_of_log_snr(sde, l1 + (l0 - l1) * (i / N)) for i in range(1, N)] + [eps]
    return np.asarray(ts, dtype=np.float64).astype(np.float32)


def data_prediction(sde, score, t, x):
    """Tweedie's estimate D = (x + (s G_k)^2 score) / alpha on (B,T,C)."""
    alpha, s, _ = marginal(sde, t)
    sg = (s * sde.G)[None, :, None]
    return (np.asarray(x, dtype=np.float64) + sg * sg * np.asarray(score, dtype=np.float64)) / alpha


def step(sde, x, d, t, t_next, d_prev=None, t_prev=None, r_inf=False):
    """x_{i+1} from x_i and D_i = d; d_prev (taken at t_prev > t): the 2M correction.  r_inf: r forced to infinity."""
    _, s0, l0 = marginal(sde, t)
    a1, s1, l1 = marginal(sde, t_next)
    h = l1 - l0
    dbar = d
    if d_prev is not None and not r_inf:
        r = (l0 - log_snr(sde, t_prev)) / h
        dbar = (1.0 + 0.5 / r) * d - (0.5 / r) * d_prev
    return (s1 / s0) * np.asarray(x, dtype=np.float64) - a1 * math.expm1(-h) * dbar


def ddim_closed_form(sde, x, d, t, t_next):
    """x' = alpha' D + (s'/s)(x - alpha D): the predicted x_0 re-noised with the same (deterministic) noise estimate."""
    a0, s0, _ = marginal(sde, t)
    a1, s1, _ = marginal(sde, t_next)
    return a1 * d + (s1 / s0) * (np.asarray(x, dtype=np.float64) - a0 * d)


def solve(sde, score_fn, x, ts, solver="dpmpp2m", r_inf=False):
    """DDIM or DPM-Solver++ 2M over the decreasing grid ts (N + 1 points): N evaluations of score_fn(x, t)."""
    x = np.asarray(x, dtype=np.float64)
    d_prev = None
    for i in range(len(ts) - 1):
        t0, t1 = float(ts[i]), float(ts[i + 1])
        d = data_prediction(sde, score_fn(x, t0), t0, x)
        if solver == "dpmpp2m" and i > 0:
            x = step(sde, x, d, t0, t1, d_prev, float(ts[i - 1]), r_inf)
        else:
            x = step(sde, x, d, t0, t1)
        d_prev = d
    return x


def sample_ode(p, sde, z_prior, N, solver, schedule="time", backbone="transformer", n_head=None, eps=1e-5):
    """DiffusionSampler.sample_ode for one batch from the injected prior draws z_prior (B,T,C), any solver and schedule."""
    from oracle import fdiff_oracle as O
    fn, x, ts = R.model_score(p, backbone, n_head), O.prior_sampling(sde, z_prior), grid(sde, N, schedule, eps)
    if solver in ("euler", "heun"):
        return R.solve(sde, fn, x, ts, solver)
    return solve(sde, fn, x, ts, solver)
