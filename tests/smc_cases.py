"""Inputs shared by tests/test_smc_cpu.py and tests/test_gpu_smc.py: the linear-Gaussian problem whose posterior and evidence are
closed-form, and the case table of the GPU loop test (the CPU test asserts its decision margins, so that the GPU test can demand
equal ancestors and resample decisions with no case excluded)."""
import math

import numpy as np

from oracle import fdiff_oracle as O
from oracle import weights as W
from tests import impute_ref as I
from tests import likelihood_ref as L

# ---------------------------------------------------------------- the linear-Gaussian problem
GAUSS = dict(T=6, C=2, sigma0=0.8, obs_std=0.3, N=200, K=2048, n=8, p_obs=0.5)


def gaussian_problem(seed, fourier, kind="vp", p=(0.1, 20.0)):
    """Data x_0 ~ N(0, sigma0^2 I) in sample space, y = A(x_0) + obs_std eps on a random mask.  Returns the SDE, the exact score, the
    conditioning of smc_ref.trajectory per series, and the closed-form log evidence and posterior mean of A(x_0) per series."""
    g = GAUSS
    T, C, n = g["T"], g["C"], g["n"]
    rs = np.random.RandomState(seed)
    sde = O.SDEParams(kind, p[0], p[1], O.noise_scaling(T, fourier))
    if fourier:
        mu, sigma = 0.3 * rs.randn(T, C), rs.uniform(0.5, 2.0, (T, C))
    else:
        mu, sigma = np.zeros((T, C)), np.ones((T, C))
    m = rs.rand(n, T, C) < g["p_obs"]
    m[:, 0, 0] = True
    xt = g["sigma0"] * rs.randn(n, T, C)
    y = I.forward_map(xt, mu, sigma, fourier) + g["obs_std"] * rs.randn(n, T, C)
    x0 = I.x0_obs(np.where(m, y, np.nan), m, mu, sigma, fourier)
    # dense algebra: A(x) = Amat x + a0 on the flattened (T C) vector
    a0 = I.forward_map(np.zeros((1, T, C)), mu, sigma, fourier).reshape(-1)
    Amat = np.stack([I.forward_map(e.reshape(1, T, C), mu, sigma, fourier).reshape(-1) - a0 for e in np.eye(T * C)], axis=1)
    logz, post = np.zeros(n), np.zeros((n, T, C))
    for q in range(n):
        idx = np.flatnonzero(m[q].reshape(-1))
        MA = Amat[idx]
        cov = g["sigma0"] ** 2 * MA @ MA.T + g["obs_std"] ** 2 * np.eye(len(idx))
        d = y[q].reshape(-1)[idx] - a0[idx]
        sol = np.linalg.solve(cov, d)
        logz[q] = -0.5 * d @ sol - 0.5 * np.linalg.slogdet(cov)[1] - 0.5 * len(idx) * math.log(2.0 * math.pi)
        post[q] = (Amat @ (g["sigma0"] ** 2 * MA.T @ sol) + a0).reshape(T, C)
    return dict(sde=sde, score_fn=L.gaussian_score(sde, g["sigma0"]), mu=mu, sigma=sigma, m=m, y=y, x0=x0, logz=logz, post=post,
                n_obs=m.reshape(n, -1).sum(axis=1))


# ---------------------------------------------------------------- the GPU loop test's cases
LOOP = dict(T=8, C=3, D=8, L=2, H=4, n=2, K=4, N=6, obs_std=0.3, twist_scale=1.0, thr=0.5)
# (kind, p, fourier, jacobian) -> seed of the case's inputs, picked by tests/test_smc_cpu.py's margin check
LOOP_CASES = [
    ("vp", (0.1, 20.0), True, False), ("vp", (0.1, 20.0), True, True), ("vp", (0.1, 20.0), False, False),
    ("vp", (0.1, 20.0), False, True), ("ve", (0.01, 2.0), True, False), ("ve", (0.01, 2.0), True, True),
    ("ve", (0.01, 2.0), False, False), ("ve", (0.01, 2.0), False, True),
]
LOOP_SEEDS = {}      # case index -> seed, where the default (its index + 1) does not clear the margins


def loop_seed(i):
    return LOOP_SEEDS.get(i, i + 1)


def loop_inputs(i):
    """The injected noise and conditioning of loop case i (f32-representable where the engine reads f32)."""
    kind, p, fourier, jac = LOOP_CASES[i]
    c = LOOP
    T, C, n, K, N = c["T"], c["C"], c["n"], c["K"], c["N"]
    B = n * K
    rs = np.random.RandomState(100 + loop_seed(i))
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    if fourier:
        mu, sigma = f32(0.3 * rs.randn(T, C)), f32(rs.uniform(0.5, 2.0, (T, C)))
    else:
        mu, sigma = np.zeros((T, C)), np.ones((T, C))
    y = f32(np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(n, T, C))
    m = rs.rand(n, T, C) < 0.5
    m[:, 0, 0] = True
    yn = np.where(m, y, np.nan)
    return dict(kind=kind, p=p, fourier=fourier, jac=jac, mu=mu, sigma=sigma, yn=yn, m=m,
                x0=I.x0_obs(yn, m, mu, sigma, fourier), zp=f32(rs.randn(B, T, C)), zs=f32(rs.randn(N, B, T, C)),
                u=rs.rand(N + 1, n))


def loop_weights():
    c = LOOP
    return W.make_state_dict(c["C"], c["T"], c["D"], c["L"], seed=1234)


_loop_cache = {}


def loop_reference(i):
    """The float64 trajectory of loop case i (computed once per process)."""
    if i not in _loop_cache:
        from tests import ode_ref
        from tests import smc_ref as S
        c, d = LOOP, loop_inputs(i)
        sde = O.SDEParams(d["kind"], d["p"][0], d["p"][1], O.noise_scaling(c["T"], True))
        score_fn = ode_ref.model_score(loop_weights(), "transformer", c["H"])
        _loop_cache[i] = S.trajectory(score_fn, sde, d["zp"], list(d["zs"]), d["u"], np.repeat(d["x0"], c["K"], 0),
                                      np.repeat(d["m"], c["K"], 0), d["sigma"], d["fourier"], c["K"], c["obs_std"],
                                      c["twist_scale"], c["thr"], True, d["jac"])
    return _loop_cache[i]
