"""Float64 restatement of the adaptive likelihood (DiffusionSampler.log_likelihood(solver="rk45"), csrc/fd_likelihood.hip): the
Dormand-Prince 5(4) pair with the step control of scipy.integrate.RK45, run per row on the augmented state y = [x_b, acc_b],

    dx/dt = v(x, t) = -a x - 0.5 (g G_k)^2 s(x, t),      dacc/dt = div v = -a T C - 0.5 g^2 tr_b(x, t)

from t0 = eps to 1.  numpy only (tests/test_rk45_likelihood_cpu.py checks it against scipy); shared with
tests/test_gpu_rk45_likelihood.py."""
import numpy as np

from tests import likelihood_ref as L
from tests import ode_ref as R

# Dormand & Prince (1980), the tableau of scipy's RK45: nodes C, stage matrix A, 5th-order weights B, error weights E (7 stages)
C = np.array([0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0])
A = np.array([
    [0.0, 0.0, 0.0, 0.0, 0.0],
    [1 / 5, 0.0, 0.0, 0.0, 0.0],
    [3 / 40, 9 / 40, 0.0, 0.0, 0.0],
    [44 / 45, -56 / 15, 32 / 9, 0.0, 0.0],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729, 0.0],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
])
B = np.array([35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84])
E = np.array([-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40])
SAFETY, MIN_FACTOR, MAX_FACTOR = 0.9, 0.2, 10.0
ERROR_EXPONENT = -1 / 5

# row status, as fd_likelihood_run_adaptive's status_out
CONVERGED, STEP_TOO_SMALL, MAX_EVALS = 1, 2, 3


def rms(v):
    return float(np.linalg.norm(v)) / v.size ** 0.5


def initial_step(fun, t0, y0, t_bound, f0, rtol, atol, order=4):
    """scipy's select_initial_step (forward direction, no max_step); one evaluation of fun."""
    interval = abs(t_bound - t0)
    scale = atol + np.abs(y0) * rtol
    d0, d1 = rms(y0 / scale), rms(f0 / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    h0 = min(h0, interval)
    f1 = fun(t0 + h0, y0 + h0 * f0)
    d2 = rms((f1 - f0) / scale) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1 / (order + 1))
    return min(100 * h0, h1, interval)


def dp_step(fun, t, y, f, h):
    """One Dormand-Prince step: (y_new, f_new, K (7, n)) as scipy's rk_step."""
    K = np.empty((7, y.size))
    K[0] = f
    for s in range(1, 6):
        K[s] = fun(t + C[s] * h, y + np.dot(K[:s].T, A[s, :s]) * h)
    y_new = y + h * np.dot(K[:-1].T, B)
    f_new = fun(t + h, y_new)
    K[-1] = f_new
    return y_new, f_new, K


def rk45(fun, t0, y0, t_bound, rtol, atol, max_evals=None):
    """Integrate y' = fun(t, y) from t0 to t_bound (> t0) with the semantics of scipy.integrate.RK45 (scipy 1.15).  Returns a dict:
    t (accepted times, t0 first), y (the last accepted state), nfe (scipy's nfev: 2 + 6 per attempted step), status (CONVERGED,
    STEP_TOO_SMALL or MAX_EVALS: an attempt that would take nfe past max_evals is not started), err_norms (every attempt's)."""
    y = np.asarray(y0, dtype=np.float64).copy()
    t = float(t0)
    f = fun(t, y)
    h_abs = initial_step(fun, t, y, t_bound, f, rtol, atol)
    nfe, ts, errs, status = 2, [t], [], None
    while status is None:
        min_step = 10 * abs(np.nextafter(t, np.inf) - t)
        h_abs = max(h_abs, min_step)
        rejected = False
        while True:
            if h_abs < min_step:
                status = STEP_TOO_SMALL
                break
            if max_evals is not None and nfe + 6 > max_evals:
                status = MAX_EVALS
                break
            nfe += 6
            t_new = min(t + h_abs, t_bound)
            h = t_new - t
            h_abs = abs(h)
            y_new, f_new, K = dp_step(fun, t, y, f, h)
            scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
            en = rms(np.dot(K.T, E) * h / scale)
            errs.append(en)
            if en < 1:
                factor = MAX_FACTOR if en == 0 else min(MAX_FACTOR, SAFETY * en ** ERROR_EXPONENT)
                if rejected:
                    factor = min(1, factor)
                h_abs *= factor
                t, y, f = t_new, y_new, f_new
                ts.append(t)
                if t >= t_bound:
                    status = CONVERGED
                break
            h_abs *= max(MIN_FACTOR, SAFETY * en ** ERROR_EXPONENT)
            rejected = True
    return dict(t=np.array(ts), y=y, nfe=nfe, status=status, err_norms=errs)


def dp_fixed(fun, ts, y0):
    """The 5th-order Dormand-Prince solution over the given grid (no step control)."""
    y = np.asarray(y0, dtype=np.float64).copy()
    f = fun(float(ts[0]), y)
    for i in range(len(ts) - 1):
        y, f, _ = dp_step(fun, float(ts[i]), y, f, float(ts[i + 1]) - float(ts[i]))
    return y


def augmented(sde, score_fn, trace_fn, T, C):
    """fun(t, y) of one row's augmented ODE; trace_fn(x (1,T,C), t) -> tr(diag(G^2) ds/dx) (scalar or (1,))."""
    def fun(t, y):
        x = y[:-1].reshape(1, T, C)
        a, g = R.coef(sde, t)
        v = R.velocity(sde, score_fn(x, t), t, x)
        div = -a * T * C - 0.5 * g * g * float(np.ravel(trace_fn(x, t))[0])
        return np.concatenate([v.ravel(), [div]])
    return fun


def _row_fun(sde, score_fn, trace_fn, probes, b, T, C):
    """fun of row b: the closed-form trace_fn, or the probe e_b of probes (B,T,C) by central differences."""
    if probes is None:
        return augmented(sde, score_fn, trace_fn, T, C)
    e = probes[b:b + 1]
    return augmented(sde, score_fn, lambda x, t: float(((sde.G ** 2)[None, :, None] * e * L.jvp(score_fn, x, t, e)).sum()), T, C)


def log_likelihood(sde, score_fn, x0, rtol, atol, *, trace_fn=None, probes=None, t0=1e-5, t1=1.0, max_evals=None, prior_fn=None):
    """Per row b of x0 (B,T,C): the adaptive integration of its augmented ODE.  The trace is trace_fn(x, t) (closed form) or, with
    probes (B,T,C), e_b^T diag(G^2) (ds/dx) e_b by central differences.  Returns a list of per-row dicts (rk45's, plus latents
    x_1 (T,C), delta (= acc, the divergence integral) and log_prob = prior + delta)."""
    x0 = np.asarray(x0, dtype=np.float64)
    Bn, T, Cn = x0.shape
    out = []
    for b in range(Bn):
        fun = _row_fun(sde, score_fn, trace_fn, probes, b, T, Cn)
        r = rk45(fun, t0, np.concatenate([x0[b].ravel(), [0.0]]), t1, rtol, atol, max_evals)
        lat = r["y"][:-1].reshape(T, Cn)
        prior = float((prior_fn or (lambda z: L.prior_logp(sde, z)))(lat[None])[0])
        r.update(latents=lat, delta=float(r["y"][-1]), prior=prior, log_prob=prior + float(r["y"][-1]))
        out.append(r)
    return out


def rows_on_grid(sde, score_fn, x0, grids, *, trace_fn=None, probes=None):
    """The fixed-step Dormand-Prince solution of every row of x0 (B,T,C) on its grid (grids (B, S), NaN padding dropped): a list
    of (latents (T,C), delta)."""
    x0 = np.asarray(x0, dtype=np.float64)
    Bn, T, Cn = x0.shape
    out = []
    for b in range(Bn):
        ts = np.asarray(grids[b], dtype=np.float64)
        y = dp_fixed(_row_fun(sde, score_fn, trace_fn, probes, b, T, Cn), ts[~np.isnan(ts)], np.concatenate([x0[b].ravel(), [0.0]]))
        out.append((y[:-1].reshape(T, Cn), float(y[-1])))
    return out


def gaussian_delta(sde, sigma0, x0, t0=1e-5, t1=1.0):
    """Closed form of the divergence integral for data N(0, sigma0^2 I) under the exact score: the flow is linear and diagonal,
    so int div v dt = log det(dx_1 / dx_0) = sum_{t,c} 0.5 log(var_t(t1) / var_t(t0))."""
    C_ = x0.shape[2]
    return C_ * 0.5 * float(np.sum(np.log(L.gaussian_var(sde, sigma0, t1) / L.gaussian_var(sde, sigma0, t0))))

