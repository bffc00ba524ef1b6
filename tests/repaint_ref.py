"""Float64 restatement of RePaint resampling in replacement conditioning (DiffusionSampler.impute(resample=r, jump_length=j),
fd_sampler_run_impute_repaint, fd_impute_project_renoise; Lugmayr et al. 2022), built from tests/impute_ref.py (the projection) and,
for guided models, the score functions of tests/cfg_ref.py through ``score_fn``.  Shared by tests/test_repaint_cpu.py and
tests/test_gpu_repaint.py.

Grid t_0 > ... > t_{N-1} and dt as the sampler's; level i < N is t_i, level N the clean one (alpha = 1, s = 0).  The N steps are cut
into blocks [i0, i1), i1 = min(i0 + j, N); a block is executed r times before the next one starts, one execution being step +
projection (at level i + 1) for i = i0 .. i1-1, and between two executions the state is diffused forward from level i1 back to level
i0 by the transition kernel x <- a x + b G z.
"""
import math

import numpy as np

from oracle import fdiff_oracle as O
from tests import dps_ref as D
from tests import impute_ref as I


def level_coef(sde, ts, i):
    """(alpha, s) of level i of the grid ts: the perturbation kernel at ts[i], the clean level (1, 0) at i = len(ts)."""
    return D.coef(sde, float(ts[i])) if i < len(ts) else (1.0, 0.0)


def transition_radicand(lo, hi):
    """b^2 of transition_coef before any clamp: s_hi^2 - a^2 s_lo^2."""
    a = hi[0] / lo[0]
    return hi[1] * hi[1] - a * a * lo[1] * lo[1]


def transition_coef(lo, hi):
    """(a, b) of the forward transition kernel from the level lo = (alpha_lo, s_lo) to the noisier level hi = (alpha_hi, s_hi):
    x_hi = a x_lo + b G z with a = alpha_hi / alpha_lo and b = sqrt(s_hi^2 - a^2 s_lo^2), the same expression for VP and VE (a = 1)."""
    a = hi[0] / lo[0]
    rad = transition_radicand(lo, hi)
    assert rad >= -1e-15, (lo, hi, rad)           # the forward process only adds variance: a negative value is a bug, not rounding
    return a, math.sqrt(max(rad, 0.0))


def schedule(N, resample=1, jump_length=1):
    """The execution order: ("step", i) and ("renoise", i1, i0)."""
    assert N >= 1 and resample >= 1 and jump_length >= 1
    ops = []
    i0 = 0
    while i0 < N:
        i1 = min(i0 + jump_length, N)
        for u in range(resample):
            for i in range(i0, i1):
                ops.append(("step", i))
            if u + 1 < resample:
                ops.append(("renoise", i1, i0))
        i0 = i1
    return ops


def counts(N, resample, jump_length):
    """(E, K): score evaluations and re-noises."""
    return resample * N, (resample - 1) * -(-N // jump_length)


def renoise(x, G, a, b, z):
    """x <- a x + b G z."""
    return a * np.asarray(x, dtype=np.float64) + b * np.asarray(G, dtype=np.float64)[None, :, None] * np.asarray(z, dtype=np.float64)


def project_renoise(x, x0, m, sigma, G, alpha, s, z, a, b, z_re, fourier):
    """The fused form of the kernel: xt + P(a d), xt = a x + b G z_re, d = alpha x0 + s G z - x, P = A^-1 m A."""
    x = np.asarray(x, dtype=np.float64)
    Gc = np.asarray(G, dtype=np.float64)[None, :, None]
    d = alpha * np.asarray(x0, dtype=np.float64) + s * Gc * z - x
    xt = a * x + b * Gc * z_re
    mb = np.broadcast_to(np.asarray(m, dtype=bool), x.shape)
    if not fourier:
        return xt + np.where(mb, a * d, 0.0)
    return xt + O.dft(np.where(mb, O.idft(sigma[None] * (a * d)), 0.0)) / sigma[None]


def repaint_trajectory(p, sde, z_prior, z_steps, z_obs, z_re, x0, m, sigma, fourier, n_head, resample=1, jump_length=1, eps=1e-5,
                       score_fn=None):
    """impute_ref.impute_trajectory under the schedule: z_steps and z_obs hold E = r N slots and z_re K = (r - 1) ceil(N / j), all
    in execution order.  score_fn(X, t) -> score; default: the oracle's score_forward on the weights p."""
    E, K = len(z_steps), len(z_re)
    assert E % resample == 0
    N = E // resample
    assert (E, K) == counts(N, resample, jump_length) and len(z_obs) == E
    ts, dt = O.timesteps(N, eps)
    X = O.prior_sampling(sde, z_prior)
    B = X.shape[0]
    if score_fn is None:
        def score_fn(x, t):
            return O.score_forward(p, x, np.full((B,), t, dtype=np.float32), n_head)
    e = k = 0
    for op in schedule(N, resample, jump_length):
        if op[0] == "step":
            i = op[1]
            t = ts[i]
            X = O.sde_step(sde, score_fn(X, t), float(t), X, z_steps[e], float(dt))
            if i + 1 < N:
                alpha, s = level_coef(sde, ts, i + 1)
                X = I.project(X, x0, m, sigma, sde.G, alpha, s, z_obs[e], fourier)
            else:
                X = I.project(X, x0, m, sigma, sde.G, 1.0, 0.0, np.zeros_like(X), fourier)
            e += 1
        else:
            a, b = transition_coef(level_coef(sde, ts, op[1]), level_coef(sde, ts, op[2]))
            X = renoise(X, sde.G, a, b, z_re[k])
            k += 1
    assert (e, k) == (E, K)
    return X
