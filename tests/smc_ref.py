"""Float64 restatement of twisted sequential Monte Carlo conditioning (DiffusionSampler.impute(conditioning="smc"),
csrc/fd_smc.hip; the Twisted Diffusion Sampler of Wu et al. 2023) on tests/dps_ref.py and tests/impute_ref.py.  Per state row and
step t_i -> t_{i+1}, (alpha_i, s_i) the perturbation kernel at t_i, rho_i = ||r||^2 and g_i = -grad rho_i of dps_ref.guidance,
n = sqrt(dt) g(t_i) G_k z the step's noise term per element and S = dt g(t_i)^2 G_k^2 its variance:

    v_i      = obs_std^2 + twist_scale (s_i / alpha_i)^2
    ltw_i(x) = -rho_i(x) / (2 v_i),   h_i = g_i / (2 v_i)
    x_{i+1}  = sde_step(x_i, score_i, z_i) + S . h_i
    c1 = sum n h,  c2 = sum S h^2
    logw    += -c1 - c2 / 2 + ltw_{i+1}(x_{i+1}) - ltw_i(x_i)              (logw = ltw_0(x_0) at the prior)

rho_N is the residual of x_N itself (alpha = 1, s = 0) and v_N = obs_std^2.  Stage j = 0 .. N runs after evaluation j and before step
j, per series over its K adjacent rows (``stage``).  Shared by tests/test_smc_cpu.py and tests/test_gpu_smc.py."""
import math

import numpy as np

from oracle import fdiff_oracle as O
from tests import dps_ref as D


def stage(logw, u, thr, force, final=False):
    """One stage on logw (n, K) with one uniform u (n,) per series: W = softmax(logw), a NaN or infinite entry counting as weight 0;
    ESS = 1 / sum W^2; if force or ESS < thr K the series is resampled systematically, a[k] = min{j : cumW[j] > (u + k) / K}
    clamped to K - 1, its logw becomes 0 and dlogz = logsumexp(logw) - log K; else logw is kept and dlogz = 0 (final: the same
    logsumexp - log K).  A series whose entries all have weight 0 is kept, with ESS 0 and dlogz = -inf.
    Returns dict(logw, anc (n, K) int, ess, resampled, dlogz, cum (n, K), target (n, K))."""
    logw = np.array(logw, dtype=np.float64)
    n, K = logw.shape
    out = dict(logw=logw.copy(), anc=np.tile(np.arange(K), (n, 1)), ess=np.zeros(n), resampled=np.zeros(n, bool),
               dlogz=np.zeros(n), cum=np.full((n, K), np.nan), target=np.full((n, K), np.nan))
    for q in range(n):
        lw = logw[q]
        valid = np.isfinite(lw)
        if not valid.any():
            out["dlogz"][q] = -np.inf
            continue
        m = lw[valid].max()
        w = np.where(valid, np.exp(np.where(valid, lw, m) - m), 0.0)
        tot = w.sum()
        W = w / tot
        ess = 1.0 / np.sum(W * W)
        cum = np.cumsum(W)
        out["ess"][q] = ess
        res = bool(force) or ess < thr * K
        if res or final:
            out["dlogz"][q] = m + math.log(tot) - math.log(K)
        if res:
            target = (float(u[q]) + np.arange(K)) / K
            out["anc"][q] = np.minimum(np.searchsorted(cum, target, side="right"), K - 1)
            out["logw"][q] = 0.0
            out["resampled"][q] = True
            out["cum"][q], out["target"][q] = cum, target
    return out


def diffusion(sde, t):
    """g(t) of the reverse step (before G_k), as O.sde_step."""
    if sde.kind == "vp":
        return math.sqrt(sde.p0 + t * (sde.p1 - sde.p0))
    return sde.p0 * math.sqrt(2.0 * math.log(sde.p1 / sde.p0)) * (sde.p1 / sde.p0) ** t


def twist_inv2v(sde, t, obs_std, twist_scale):
    """1 / (2 v) at t; t None: the final stage, v = obs_std^2."""
    if t is None:
        return 1.0 / (2.0 * obs_std * obs_std)
    alpha, s = D.coef(sde, t)
    return 1.0 / (2.0 * (obs_std * obs_std + twist_scale * (s / alpha) ** 2))


def step(sde, x, score, g, src, z, t, dt, inv2v, with_abs=False):
    """The proposal from rows src (B,) of x, score, g with noise z (B,T,C) of the new rows: (x', c1, c2); with_abs: also
    sum |n h| per row, the size of the terms c1 is summed from."""
    x, score, g = (np.asarray(a, dtype=np.float64)[src] for a in (x, score, g))
    z = np.asarray(z, dtype=np.float64)
    gk = (diffusion(sde, float(t)) * sde.G)[None, :, None]
    nz = math.sqrt(float(dt)) * gk * z
    S = float(dt) * gk * gk
    h = g * inv2v
    xn = O.sde_step(sde, score, float(t), x, z, float(dt)) + S * h
    out = (xn, (nz * h).sum(axis=(1, 2)), (S * h * h).sum(axis=(1, 2)))
    return out + (np.abs(nz * h).sum(axis=(1, 2)),) if with_abs else out


def step_sums_f32(sde, g, src, z, t, dt, inv2v):
    """(c1, c2) of ``step`` with every product and sum in float32: what single precision alone does to the two sums (a test's
    bound for a cancelling c1 is set at a stated margin over this against float64)."""
    f = np.float32
    g = np.asarray(g, dtype=f)[src]
    gk = (f(diffusion(sde, float(t))) * sde.G.astype(f))[None, :, None]
    nz = f(math.sqrt(float(dt))) * (gk * np.asarray(z, dtype=f))
    S = f(dt) * (gk * gk)
    h = g * f(inv2v)
    return (nz * h).sum(axis=(1, 2), dtype=f).astype(np.float64), (S * h * h).sum(axis=(1, 2), dtype=f).astype(np.float64)


def final_rho(x, x0, m, sigma, G, fourier):
    """||r||^2 per row of x itself (alpha = 1, s = 0)."""
    r, _ = D.residual(x, np.zeros_like(x), x0, m, sigma, G, 1.0, 0.0, fourier)
    return (r * r).sum(axis=(1, 2))


def trajectory(score_fn, sde, z_prior, z_steps, u_stages, x0, m, sigma, fourier, K, obs_std, twist_scale=1.0, thr=0.5,
               final_resample=True, jacobian=False, eps=1e-5, vjp_fn=None, x_init=None):
    """impute(conditioning="smc") for one launch from injected prior / predictor noise and uniforms u_stages (N + 1, n); x0 and m
    per state row (B,T,C), B = n K.  Returns dict: x (B,T,C) the final ensemble, log_evidence (n,) (without the Gaussian
    constant), log_weights (B,), and per stage j = 0 .. N the lists states (the rows the stage saw), logw_in (the updated log
    weights the stage saw), ess, resampled, anc (n, K), cum, target, and mag (B,): sum |n h| + c2 / 2 + |ltw_j| + |ltw_{j-1}|, the size
    of the terms the stage's log-weight update is summed from."""
    N = len(z_steps)
    ts, dt = O.timesteps(N, eps)
    X = O.prior_sampling(sde, z_prior) if x_init is None else np.asarray(x_init, dtype=np.float64)
    B = X.shape[0]
    n = B // K
    base = (np.arange(B) // K) * K
    logw = np.zeros(B)
    logz = np.zeros(n)
    ltw_prev = np.zeros(B)
    c1 = c2 = c1abs = np.zeros(B)
    tr = dict(states=[], logw_in=[], ess=[], resampled=[], anc=[], cum=[], target=[], mag=[])
    for j in range(N + 1):
        last = j == N
        if last:
            rho = final_rho(X, x0, m, sigma, sde.G, fourier)
            inv2v = twist_inv2v(sde, None, obs_std, twist_scale)
        else:
            t = float(ts[j])
            g, rho, score = D.guidance(score_fn, sde, X, t, x0, m, sigma, fourier, jacobian, vjp_fn=vjp_fn)
            inv2v = twist_inv2v(sde, t, obs_std, twist_scale)
        ltw = -rho * inv2v
        logw = logw + (-c1 - 0.5 * c2) + (ltw - ltw_prev)
        tr["mag"].append(c1abs + 0.5 * c2 + np.abs(ltw) + np.abs(ltw_prev))
        tr["states"].append(X.copy())
        tr["logw_in"].append(logw.copy())
        # (the final stage resamples under final_resample alone)
        st = stage(logw.reshape(n, K), u_stages[j], 0.0 if last else thr, last and final_resample, final=last)
        for key in ("ess", "resampled", "anc", "cum", "target"):
            tr[key].append(st[key])
        logw = st["logw"].reshape(B)
        logz = logz + st["dlogz"]
        src = base + st["anc"].reshape(B)
        ltw_prev = ltw[src]
        if last:
            X = X[src]
        else:
            X, c1, c2, c1abs = step(sde, X, score, g, src, z_steps[j], t, dt, inv2v, with_abs=True)
    return dict(x=X, log_evidence=logz, log_weights=logw, **tr)


def margins(tr, thr, final_resample=True):
    """(the smallest |cumW[j] - (u + k) / K| over all threshold comparisons of the resampled stages, the smallest
    |ESS - thr K| / K over the stages whose decision depends on it) of one trajectory."""
    mc, me = np.inf, np.inf
    N1 = len(tr["ess"])
    for j in range(N1):
        K = tr["anc"][j].shape[1]
        for q in range(tr["ess"][j].shape[0]):
            if tr["resampled"][j][q]:
                mc = min(mc, float(np.abs(tr["cum"][j][q][:, None] - tr["target"][j][q][None, :]).min()))
            if not (j == N1 - 1 and final_resample):
                me = min(me, abs(float(tr["ess"][j][q]) - thr * K) / K)
    return mc, me


def gaussian_constant(n_obs, obs_std):
    """-(n_obs / 2) log(2 pi obs_std^2): what the Python layer adds to the engine's evidence."""
    return -0.5 * np.asarray(n_obs, dtype=np.float64) * math.log(2.0 * math.pi * obs_std * obs_std)
