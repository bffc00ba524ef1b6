"""Float64 restatement of the probability-flow ODE likelihood (DiffusionSampler.log_likelihood, csrc/fd_likelihood.hip):
    log p_0(x_0) = log p_1(x_1) + int_eps^1 div v dt,   div v = -a T C - 0.5 g^2 tr(diag(G_k^2) ds/dx)
integrated by the Euler / Heun steps of tests/ode_ref.py, the divergence over the same quadrature (Heun: the trapezoid of its two
stages).  The trace comes from central differences of a score function (exact: every basis vector; Hutchinson: given probes),
or from a closed form.  Shared by tests/test_likelihood_cpu.py and tests/test_gpu_likelihood.py."""
import math

import numpy as np

from tests import ode_ref as R


def marginal_coef(sde, t):
    """(alpha(t), s(t)) of x_t = alpha x_0 + s G z (VP / VE, as SDE.marginal_coef)."""
    t = float(t)
    if sde.kind == "vp":
        lmc = -0.25 * t * t * (sde.p1 - sde.p0) - 0.5 * t * sde.p0
        return math.exp(lmc), math.sqrt(1.0 - math.exp(2.0 * lmc))
    return 1.0, sde.p0 * (sde.p1 / sde.p0) ** t


def gaussian_var(sde, sigma0, t):
    """(T,) variance of the marginal at t of data N(0, sigma0^2 I): alpha^2 sigma0^2 + s^2 G_k^2."""
    al, s = marginal_coef(sde, t)
    return al * al * sigma0 * sigma0 + s * s * sde.G ** 2


def gaussian_score(sde, sigma0):
    """The exact score of the marginals of Gaussian data, -x / (alpha^2 sigma0^2 + s^2 G_k^2)."""
    return lambda x, t: -np.asarray(x, dtype=np.float64) / gaussian_var(sde, sigma0, t)[None, :, None]


def gaussian_trace(sde, sigma0, C):
    """Closed-form tr(diag(G^2) ds/dx) of gaussian_score, per series."""
    def fn(x, t):
        return np.full(x.shape[0], -C * float(np.sum(sde.G ** 2 / gaussian_var(sde, sigma0, t))))
    return fn


def normal_logp(x, var):
    """sum_{t,c} log N(x; 0, var_t) per series, var (T,)."""
    x = np.asarray(x, dtype=np.float64)
    v = np.asarray(var, dtype=np.float64)[None, :, None]
    return (-0.5 * x * x / v - 0.5 * np.log(2.0 * math.pi * v)).sum(axis=(1, 2))


def prior_logp(sde, x):
    """log density of the published prior N(0, (sigma_p G_k)^2), sigma_p = 1 (VP) or sigma_max (VE) (fd_prior_logp)."""
    sp = sde.p1 if sde.kind == "ve" else 1.0
    return normal_logp(x, (sp * sde.G) ** 2)


def jvp(score_fn, x, t, e, rel=1e-7):
    """(ds/dx) e by central differences in float64, step rel * max(1, |x|_inf) (small: a network's relu pre-activations must not
    cross their kink within the step)."""
    d = rel * max(1.0, float(np.abs(x).max()))
    return (score_fn(x + d * e, t) - score_fn(x - d * e, t)) / (2.0 * d)


def fd_trace(score_fn, G):
    """tr(diag(G^2) ds/dx) per series over all T*C basis vectors."""
    def fn(x, t):
        B, T, C = x.shape
        out = np.zeros(B)
        for k in range(T * C):
            e = np.zeros((T, C))
            e.flat[k] = 1.0
            e = np.broadcast_to(e, x.shape)
            out += ((G ** 2)[None, :, None] * e * jvp(score_fn, x, t, e)).sum(axis=(1, 2))
        return out
    return fn


def fd_probe_trace(score_fn, G, probes):
    """e^T diag(G^2) (ds/dx) e per (series, probe): probes (B, P, T, C) -> (B, P)."""
    def fn(x, t):
        return np.stack([((G ** 2)[None, :, None] * probes[:, j] * jvp(score_fn, x, t, probes[:, j])).sum(axis=(1, 2))
                         for j in range(probes.shape[1])], axis=1)
    return fn


def log_likelihood(sde, score_fn, trace_fn, x0, ts, solver="heun", prior_fn=None):
    """(log_prob, prior, drift part, score part, x_1).  trace_fn(x, t) -> (B,) or (B, P) of tr(diag(G^2) ds/dx) estimates
    (score part then (B,) or (B, P)); prior_fn(x_1) -> (B,) log p_1, default the published prior."""
    x = np.asarray(x0, dtype=np.float64)
    T, C = x.shape[1], x.shape[2]
    drift, sdiv = 0.0, 0.0
    for i in range(len(ts) - 1):
        t0, t1 = float(ts[i]), float(ts[i + 1])
        h = t1 - t0
        a0, g0 = R.coef(sde, t0)
        v0 = R.velocity(sde, score_fn(x, t0), t0, x)
        d0 = -0.5 * g0 * g0 * trace_fn(x, t0)
        if solver == "euler":
            drift += h * (-a0 * T * C)
            sdiv = sdiv + h * d0
            x = x + h * v0
        else:
            xt = x + h * v0
            a1, g1 = R.coef(sde, t1)
            v1 = R.velocity(sde, score_fn(xt, t1), t1, xt)
            d1 = -0.5 * g1 * g1 * trace_fn(xt, t1)
            drift += 0.5 * h * (-(a0 + a1) * T * C)
            sdiv = sdiv + 0.5 * h * (d0 + d1)
            x = x + 0.5 * h * (v0 + v1)
    prior = (prior_fn or (lambda z: prior_logp(sde, z)))(x)
    div = sdiv.mean(axis=1) if np.ndim(sdiv) == 2 else sdiv
    return prior + drift + div, prior, drift, sdiv, x


def dft_matrix(T):
    """The packed real DFT of utils/fourier.py as a (T, T) matrix (oracle.fdiff_oracle.dft on the basis vectors)."""
    from oracle import fdiff_oracle as O
    return O.dft(np.eye(T)[:, :, None])[:, :, 0].T
