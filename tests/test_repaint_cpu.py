"""CPU: RePaint resampling in replacement conditioning (an extension, not in the reference) -- the float64 restatement of
tests/repaint_ref.py has the properties the engine relies on (transition coefficients, schedule, the fused project + re-noise), it is
impute_ref.impute_trajectory at resample = 1, and it removes the bias of plain replacement on a correlated Gaussian."""
import ctypes

import numpy as np
import pytest

from oracle import fdiff_oracle as O
from oracle import weights as W
from oracle.make_golden import CFG_TINY
from tests import impute_ref as I
from tests import repaint_ref as R


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in ("fd_impute_project_renoise", "fd_sampler_run_impute_repaint"):
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


@pytest.mark.parametrize("kind,p", [("vp", (0.1, 20.0)), ("ve", (0.01, 2.0))])
def test_transition_coefficients(kind, p):
    """alpha_hi = a alpha_lo and s_hi^2 = a^2 s_lo^2 + b^2 with b real, for level pairs including the clean one."""
    sde = O.SDEParams(kind, p[0], p[1], np.ones(4))
    for N in (8, 50):
        ts, _ = O.timesteps(N)
        pairs = [(i1, i0) for i0 in range(N) for i1 in (i0 + 1, min(i0 + 5, N), N)] + [(1, 0), (N, N - 1), (N, 0)]
        for i1, i0 in pairs:
            lo, hi = R.level_coef(sde, ts, i1), R.level_coef(sde, ts, i0)
            assert R.transition_radicand(lo, hi) >= -1e-15, (kind, N, i1, i0)          # before any clamp
            a, b = R.transition_coef(lo, hi)
            assert b >= 0.0 and np.isfinite(a) and np.isfinite(b)
            assert abs(hi[0] - a * lo[0]) <= 1e-12
            assert abs(hi[1] ** 2 - (a * a * lo[1] ** 2 + b * b)) <= 1e-12
            if kind == "ve":
                assert a == 1.0
    assert R.level_coef(sde, ts, N) == (1.0, 0.0)


def test_scheduler_marginal_coef_gives_the_same_transition():
    """DiffusionSampler.impute_project(renoise_to=...) forms (a, b) from the scheduler's marginal_coef: the reference's numbers."""
    from fourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler
    for sch, sde in ((VPScheduler(0.1, 20.0), O.SDEParams("vp", 0.1, 20.0, np.ones(4))),
                     (VEScheduler(0.01, 2.0), O.SDEParams("ve", 0.01, 2.0, np.ones(4)))):
        ts, _ = O.timesteps(8)
        for i1, i0 in ((3, 1), (8, 6), (8, 0)):
            lo = sch.marginal_coef(float(ts[i1])) if i1 < 8 else (1.0, 0.0)
            hi = sch.marginal_coef(float(ts[i0]))
            got, ref = R.transition_coef(lo, hi), R.transition_coef(R.level_coef(sde, ts, i1), R.level_coef(sde, ts, i0))
            assert abs(got[0] - ref[0]) <= 1e-12 and abs(got[1] - ref[1]) <= 1e-12


def test_schedule():
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    for j in (1, 2, 5, 9):
        assert R.schedule(8, 1, j) == [("step", i) for i in range(8)]
    for N, r, j in ((8, 2, 1), (8, 3, 2), (8, 2, 5), (7, 3, 3), (5, 2, 9)):
        ops = R.schedule(N, r, j)
        steps = [op[1] for op in ops if op[0] == "step"]
        E, K = R.counts(N, r, j)
        assert len(steps) == E == r * N
        assert sum(op[0] == "renoise" for op in ops) == K == (r - 1) * ((N + j - 1) // j)
        # every block runs r times, consecutively, with a re-noise back to its first level between two runs and none after the last
        pos = 0
        for i0 in range(0, N, j):
            i1 = min(i0 + j, N)
            for u in range(r):
                assert ops[pos:pos + i1 - i0] == [("step", i) for i in range(i0, i1)]
                pos += i1 - i0
                if u + 1 < r:
                    assert ops[pos] == ("renoise", i1, i0)
                    pos += 1
        assert pos == len(ops)
        assert DiffusionSampler.repaint_schedule(N, r, j) == ops
    assert DiffusionSampler.repaint_schedule(8, 1, 3) == R.schedule(8, 1, 3)
    for bad in ((0, 1, 1), (8, 0, 1), (8, 1, 0), (8, True, 1), (8, 2.0, 1)):
        with pytest.raises(ValueError):
            DiffusionSampler.repaint_schedule(*bad)


def _tiny_case(N, E, K, seed=3):
    cfg = CFG_TINY
    T, Cn, B = cfg["T"], cfg["C"], 3
    rs = np.random.RandomState(seed)
    sd = W.make_state_dict(Cn, T, cfg["D"], cfg["L"], seed=1234)
    sde = O.SDEParams("vp", 0.1, 20.0, O.noise_scaling(T, True))
    mu, sigma = 0.3 * rs.randn(T, Cn), rs.uniform(0.5, 2.0, (T, Cn))
    y = rs.randn(B, T, Cn)
    m = rs.rand(B, T, Cn) < 0.5
    x0 = I.x0_obs(np.where(m, y, np.nan), m, mu, sigma, True)
    shape = (B, T, Cn)
    zp = rs.randn(*shape)
    zs, zo, zr = rs.randn(E, *shape), rs.randn(E, *shape), rs.randn(K, *shape)
    return cfg, sd, sde, mu, sigma, y, m, x0, zp, zs, zo, zr


def test_trajectory_resample_one_is_impute_ref():
    N = 4
    cfg, sd, sde, mu, sigma, y, m, x0, zp, zs, zo, _ = _tiny_case(N, N, 0)
    ref = I.impute_trajectory(sd, sde, zp, list(zs), list(zo), x0, m, sigma, True, cfg["H"])
    for j in (1, 3, 7):
        got = R.repaint_trajectory(sd, sde, zp, list(zs), list(zo), [], x0, m, sigma, True, cfg["H"], resample=1, jump_length=j)
        assert np.array_equal(got, ref)


def test_trajectory_resampled_reproduces_observations():
    """The last executed step of the last block projects hard, whatever was re-noised before it."""
    N, r, j = 3, 2, 2
    E, K = R.counts(N, r, j)
    cfg, sd, sde, mu, sigma, y, m, x0, zp, zs, zo, zr = _tiny_case(N, E, K)
    X = R.repaint_trajectory(sd, sde, zp, list(zs), list(zo), list(zr), x0, m, sigma, True, cfg["H"], resample=r, jump_length=j)
    np.testing.assert_allclose(I.forward_map(X, mu, sigma, True)[m], y[m], atol=1e-9)


@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("T,C", [(24, 2), (37, 5)])
def test_project_renoise_is_renoise_of_project(T, C, fourier):
    rs = np.random.RandomState(T)
    B = 3
    sigma = rs.uniform(0.5, 2.0, (T, C)) if fourier else np.ones((T, C))
    G = O.noise_scaling(T, True).astype(np.float64)
    x, z, zr, x0 = rs.randn(B, T, C), rs.randn(B, T, C), rs.randn(B, T, C), rs.randn(B, T, C)
    for m in (rs.rand(B, T, C) < 0.6, rs.rand(T, C) < 0.6):
        for alpha, s, a, b in ((0.7, 0.4, 0.9, 0.3), (1.0, 0.0, 0.8, 0.6), (1.0, 0.3, 1.0, 0.5), (0.6, 0.5, 1.0, 0.0)):
            fused = R.project_renoise(x, x0, m, sigma, G, alpha, s, z, a, b, zr, fourier)
            plain = R.renoise(I.project(x, x0, m, sigma, G, alpha, s, z, fourier), G, a, b, zr)
            np.testing.assert_allclose(fused, plain, atol=1e-12, rtol=0)


def _gaussian_hidden(r, j, N=50, n=20000, rho=0.95, yobs=1.5, seed=0):
    """Mean and variance of the hidden variable of a 2-variable Gaussian (correlation rho, the first variable observed at yobs) over
    n chains of repaint_trajectory with the exact analytic score: VP (0.1, 20), no transform, G = 1."""
    sde = O.SDEParams("vp", 0.1, 20.0, np.ones(2))
    S = np.array([[1.0, rho], [rho, 1.0]])

    def score_fn(x, t):
        alpha, s = R.level_coef(sde, [float(t)], 0)
        Cinv = np.linalg.inv(alpha * alpha * S + s * s * np.eye(2))
        return -np.einsum("ij,bjc->bic", Cinv, x)

    rs = np.random.RandomState(seed)
    E, K = R.counts(N, r, j)
    shape = (n, 2, 1)
    x0 = np.zeros(shape)
    x0[:, 0, 0] = yobs
    m = np.array([[True], [False]])
    X = R.repaint_trajectory(None, sde, rs.randn(*shape), [rs.randn(*shape) for _ in range(E)], [rs.randn(*shape) for _ in range(E)],
                             [rs.randn(*shape) for _ in range(K)], x0, m, np.ones((2, 1)), False, 1, resample=r, jump_length=j,
                             score_fn=score_fn)
    np.testing.assert_allclose(X[:, 0, 0], yobs, atol=1e-12)
    return float(X[:, 1, 0].mean()), float(X[:, 1, 0].var())


def test_gaussian_bias_of_replacement_and_its_removal():
    """True conditional of the hidden variable: mean 1.425, variance 0.0975.  Plain replacement is biased by about one conditional
    standard deviation at any grid size (measured: mean 1.116 at N = 50); four runs per level remove it (measured |mean - 1.425| =
    0.022, |var - 0.0975| = 0.003 at Monte-Carlo standard errors 0.002 and 0.001)."""
    mean1, var1 = _gaussian_hidden(1, 1)
    mean4, var4 = _gaussian_hidden(4, 1)
    print(f"gaussian: r=1 mean {mean1:.4f} var {var1:.4f}; r=4 j=1 mean {mean4:.4f} var {var4:.4f}; exact 1.4250 0.0975")
    assert mean1 <= 1.225
    assert abs(mean4 - 1.425) <= 0.06
    assert abs(var4 - 0.0975) <= 0.02
