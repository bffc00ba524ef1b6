"""CPU: conditioning on a dense linear observation (impute(operator=P), an extension not in the reference) -- the float64 restatement
of tests/linop_ref.py has the algebra the kernels rely on (P P^+ = I, P^+ P an orthogonal projector, the window-mean matrix is the
aggregate path, g = -grad ||r||^2 by central differences through the closed-form Gaussian score), the row-mask rule of replacement
has a counter-example and a validator, the constructors of sampling.masks, every argument check runs before any device work,
cmd/conf/impute.yaml composes with the new block, and the six entry points are declared, bound and exported."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from tests import aggregate_ref as A
from tests import dps_ref as R
from tests import impute_ref as I
from tests import likelihood_ref as L
from tests import linop_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fd_linop_create", "fd_linop_destroy", "fd_impute_project_op", "fd_sampler_run_impute_op", "fd_impute_guidance_op",
           "fd_sampler_run_impute_dps_op")


def _ops():
    from fourierdiffusion_amd.sampling import masks as M
    return {"lowpass": M.lowpass_operator(20, 4), "blur_full": M.gaussian_blur_operator(20, 1.0, 1), "difference": M.difference_operator(37),
            "moving_average": M.moving_average_operator(37, 4, 2), "blur": M.gaussian_blur_operator(130, 2.0, 4)}


def test_entry_points_declared_bound_and_exported():
    from fourierdiffusion_amd import _C
    from tests.test_cabi import declared_symbols
    for name in SYMBOLS:
        assert name in declared_symbols()
        assert name in _C.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)


@pytest.mark.parametrize("name,shape,cond", [("lowpass", (7, 20), 1.0), ("blur_full", (20, 20), 62.7), ("difference", (36, 37), 23.5),
                                             ("moving_average", (17, 37), 11.4), ("blur", (33, 130), 2.7)])
def test_operator_algebra(name, shape, cond):
    from fourierdiffusion_amd.sampling.masks import LinearOperator
    Pm = _ops()[name]
    op = LinearOperator(Pm)
    assert Pm.shape == shape == (op.M, op.T) and abs(op.condition - cond) <= 0.05 + 1e-3 * cond
    assert op.rows_orthogonal == (name == "lowpass")
    np.testing.assert_allclose(op.P @ op.P_pinv, np.eye(op.M), atol=1e-11)             # P P^+ = I
    proj = op.P_pinv @ op.P
    np.testing.assert_allclose(proj, proj.T, atol=1e-11)                              # P^+ P: the orthogonal projector on the row space
    np.testing.assert_allclose(proj @ proj, proj, atol=1e-11)
    rs = np.random.RandomState(3)
    r, v = rs.randn(2, op.M, 3), rs.randn(2, op.T, 3)
    np.testing.assert_allclose((Q.P(v, Pm) * r).sum(), (v * Q.P_T(r, Pm)).sum(), rtol=1e-12)      # P^T is the adjoint
    np.testing.assert_allclose(Q.P(Q.P_pinv(r, Pm), Pm), r, atol=1e-11)


def test_constructors():
    from fourierdiffusion_amd.sampling import masks as M
    Pl = M.lowpass_operator(20, 4)
    np.testing.assert_allclose(Pl @ Pl.T, np.eye(7), atol=1e-13)                      # orthonormal rows
    assert M.lowpass_operator(8, 5).shape == (8, 8)                                   # up to the Nyquist bin of an even T: one row
    np.testing.assert_allclose(M.lowpass_operator(8, 5) @ M.lowpass_operator(8, 5).T, np.eye(8), atol=1e-13)
    x = np.random.RandomState(0).randn(2, 20, 3)
    lp = M.apply_operator(torch.from_numpy(x), Pl).numpy()
    spec = np.fft.rfft(x, axis=1, norm="ortho")
    np.testing.assert_allclose(lp[:, 0], spec[:, 0].real, atol=1e-13)
    np.testing.assert_allclose(lp[:, 1], np.sqrt(2) * spec[:, 1].real, atol=1e-13)
    np.testing.assert_allclose(lp[:, 2], -np.sqrt(2) * spec[:, 1].imag, atol=1e-13)
    Pa = M.moving_average_operator(37, 4, 2)
    assert Pa.shape == (17, 37) and (Pa[3, 6:10] == 0.25).all() and Pa[3].sum() == 1.0 and Pa[-1, 36] == 0.0
    assert M.moving_average_operator(10, 3).shape == (8, 10)
    Pd = M.difference_operator(5)
    np.testing.assert_array_equal(Pd @ np.arange(5.0) ** 2, [1, 3, 5, 7])
    Pb = M.gaussian_blur_operator(130, 2.0, 4)
    assert Pb.shape == (33, 130) and np.abs(Pb.sum(1) - 1).max() < 1e-14 and Pb[5].argmax() == 20
    np.testing.assert_allclose(Pb[5, 22] / Pb[5, 20], np.exp(-0.5), rtol=1e-12)
    for w in (1, 3, 7, 20):
        Pw = M.window_mean_operator(20, w)
        np.testing.assert_allclose(M.apply_operator(torch.from_numpy(x), Pw).numpy(), A.P(x, w), atol=1e-14)
        np.testing.assert_allclose(np.linalg.pinv(Pw), (Pw > 0).T.astype(float), atol=1e-13)      # P^+ is the broadcast
    y = torch.from_numpy(np.random.RandomState(1).randn(2, 7, 3))
    np.testing.assert_allclose(M.apply_operator(M.lift_operator(y, Pl), Pl).numpy(), y.numpy(), atol=1e-13)
    np.testing.assert_allclose(M.lift_operator(y, M.LinearOperator(Pl)).numpy(), Q.P_pinv(y.numpy(), Pl), atol=1e-13)
    for bad in (lambda: M.lowpass_operator(20, 0), lambda: M.lowpass_operator(20, 12), lambda: M.moving_average_operator(20, 21),
                lambda: M.moving_average_operator(20, 3, 0), lambda: M.difference_operator(1), lambda: M.gaussian_blur_operator(20, 0.0),
                lambda: M.gaussian_blur_operator(20, 1.0, 0), lambda: M.window_mean_operator(20, 0), lambda: M.lowpass_operator(2000, 3),
                lambda: M.apply_operator(torch.zeros(2, 19, 3), Pl), lambda: M.lift_operator(torch.zeros(2, 8, 3), Pl),
                lambda: M.operator_from_config("median", 20)):
        with pytest.raises(ValueError):
            bad()
    assert M.operator_from_config(None, 20) is None and M.operator_from_config("null", 20) is None
    np.testing.assert_array_equal(M.operator_from_config("gaussian_blur", 20, sigma=1.0, stride=1), M.gaussian_blur_operator(20, 1.0, 1))
    np.testing.assert_array_equal(M.operator_from_config("moving_average", 20, w=3, stride=2), M.moving_average_operator(20, 3, 2))


def test_linear_operator_validation():
    from fourierdiffusion_amd.sampling.masks import LinearOperator, difference_operator
    rs = np.random.RandomState(0)
    good = rs.randn(3, 8)
    op = LinearOperator(torch.from_numpy(good).float())                                # tensors and float32 are accepted
    assert (op.M, op.T) == (3, 8) and op.P.dtype == np.float64 and not op.rows_orthogonal
    dep = np.vstack([good, good[0] + good[1]])                                        # a dependent row: rank 3 < M = 4
    with pytest.raises(ValueError, match="rank"):
        LinearOperator(dep)
    with pytest.raises(ValueError, match="rank"):
        LinearOperator(np.zeros((2, 8)))
    ill = np.vstack([good[0], good[0] + 1e-6 * good[1]])                              # full rank, cond ~ 1e6
    with pytest.raises(ValueError, match="2\\^-24"):
        LinearOperator(ill)
    assert LinearOperator(ill, max_condition=1e8).condition > 1e4                     # ... unless the caller accepts it
    for bad in (np.zeros(8), np.zeros((9, 8)), np.zeros((0, 8)), np.full((2, 8), np.nan), np.zeros((2, 1025)), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError):
            LinearOperator(bad)
    for mc in (0.5, True, "1e4", float("nan")):
        with pytest.raises(ValueError):
            LinearOperator(good, max_condition=mc)
    # a T = 1024 difference operator: cond ~ 652, inside the default
    assert LinearOperator(difference_operator(1024)).M == 1023


# ---------------------------------------------------------------- the reference against aggregate_ref on the window-mean matrix
def _case(T, C, B, Pm, kind, fourier, standardize, per_series, seed, columns=False):
    rs = np.random.RandomState(seed)
    p = (0.1, 20.0) if kind == "vp" else (0.01, 2.0)
    sde = O.SDEParams(kind, p[0], p[1], O.noise_scaling(T, True))
    mu = 0.3 * rs.randn(T, C) if standardize else np.zeros((T, C))
    sigma = rs.uniform(0.3, 2.0, (T, C)) if standardize else np.ones((T, C))
    M = Pm.shape[0]
    y = Q.P(np.sin(np.linspace(0, 4, T))[None, :, None] + 0.3 * rs.randn(B, T, C), Pm)
    if columns:
        m = np.broadcast_to((rs.rand(B, 1, C) < 0.6) if per_series else (rs.rand(1, C) < 0.6), (B, M, C) if per_series else (M, C)).copy()
    else:
        m = rs.rand(B, M, C) < 0.6 if per_series else rs.rand(M, C) < 0.6
    yn = np.where(np.broadcast_to(m, y.shape), y, np.nan)
    return sde, mu, sigma, yn, m, Q.x0_obs(yn, m, mu, sigma, fourier, Pm), rs.randn(B, T, C)


@pytest.mark.parametrize("T,w", [(20, 3), (20, 20), (37, 2)])
@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("per_series", [True, False])
def test_window_mean_matrix_is_the_aggregate_reference(T, w, fourier, per_series):
    from fourierdiffusion_amd.sampling.masks import window_mean_operator
    Pm = window_mean_operator(T, w)
    sde, mu, sigma, yn, m, x0, x = _case(T, 3, 2, Pm, "vp", fourier, True, per_series, 5)
    np.testing.assert_allclose(x0, A.x0_obs(yn, m, mu, sigma, fourier, w), atol=1e-12)
    z = np.random.RandomState(1).randn(*x.shape)
    np.testing.assert_allclose(Q.project(x, x0, m, sigma, sde.G, 0.7, 0.4, z, fourier, Pm),
                               A.project(x, x0, m, sigma, sde.G, 0.7, 0.4, z, fourier, w), atol=1e-12)
    score_fn = L.gaussian_score(sde, 0.8)
    for jac in (True, False):
        g, rn2, _ = Q.guidance(score_fn, sde, x, 0.3, x0, m, sigma, fourier, Pm, jacobian=jac)
        gr, rr, _ = A.guidance(score_fn, sde, x, 0.3, x0, m, sigma, fourier, w, jacobian=jac)
        np.testing.assert_allclose(g, gr, atol=1e-12)
        np.testing.assert_allclose(rn2, rr, atol=1e-12)


@pytest.mark.parametrize("name", ["lowpass", "blur_full", "difference", "moving_average"])
@pytest.mark.parametrize("fourier", [True, False])
def test_projection_reproduces_the_observed_rows(name, fourier):
    """P A(x') = where(m, P A(x_obs), P A(x)) under the mask rule (rows on the orthonormal operator, columns elsewhere), and
    A(x') - A(x) lies in the row space of P."""
    Pm = _ops()[name]
    T = Pm.shape[1]
    sde, mu, sigma, yn, m, x0, x = _case(T, 3, 2, Pm, "vp", fourier, True, True, 5, columns=name != "lowpass")
    z = np.random.RandomState(1).randn(*x.shape)
    alpha, s = 0.7, 0.4
    xn = Q.project(x, x0, m, sigma, sde.G, alpha, s, z, fourier, Pm)
    x_obs = alpha * x0 + s * sde.G[None, :, None] * z
    Ax, Axn, Ao = (I.forward_map(v, mu, sigma, fourier) for v in (x, xn, x_obs))
    np.testing.assert_allclose(Q.P(Axn, Pm), np.where(m, Q.P(Ao, Pm), Q.P(Ax, Pm)), atol=1e-10)
    d = Axn - Ax
    np.testing.assert_allclose(d, Q.P_pinv(Q.P(d, Pm), Pm), atol=1e-10)
    xh = Q.project(x, x0, m, sigma, sde.G, 1.0, 0.0, 0.0 * z, fourier, Pm)
    np.testing.assert_allclose(Q.P(I.forward_map(xh, mu, sigma, fourier), Pm)[m], yn[m], atol=1e-10)


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("fourier", [True, False])
@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("name", ["lowpass", "difference", "moving_average"])
def test_guidance_is_minus_the_gradient_gaussian_score(kind, fourier, standardize, name):
    """Any row mask: the guidance reads P and P^T alone."""
    from fourierdiffusion_amd.sampling import masks as M
    Pm = {"lowpass": M.lowpass_operator(10, 3), "difference": M.difference_operator(9), "moving_average": M.moving_average_operator(10, 4, 2)}[name]
    sde, mu, sigma, yn, m, x0, x = _case(Pm.shape[1], 2, 3, Pm, kind, fourier, standardize, True, 5)
    score_fn = L.gaussian_score(sde, 0.8)
    for t in (0.9, 0.3, 0.05):
        g, rn2, _ = Q.guidance(score_fn, sde, x, t, x0, m, sigma, fourier, Pm,
                               vjp_fn=lambda xx, tt, v: R.vjp(score_fn, xx, tt, v, rel=1e-2))      # (the score is linear in x)
        # ||r||^2 is quadratic in x under this score: central differences are exact but for rounding, at any step
        ref = -R.grad_fd(lambda q: Q.rnorm2(score_fn, sde, q, t, x0, m, sigma, fourier, Pm), x, rel=1e-2)
        scale = np.abs(ref).max()
        assert np.abs(g - ref).max() <= 1e-8 * scale, (t, np.abs(g - ref).max() / scale)      # (the bound of test_aggregate_cpu.py)
        np.testing.assert_allclose(rn2, Q.rnorm2(score_fn, sde, x, t, x0, m, sigma, fourier, Pm), rtol=1e-12)


def test_all_false_mask_is_the_plain_step():
    Pm = _ops()["moving_average"]
    sde, mu, sigma, yn, m, x0, x = _case(37, 2, 2, Pm, "vp", True, True, False, 3)
    none = np.zeros_like(m)
    z = np.random.RandomState(4).randn(*x.shape)
    np.testing.assert_array_equal(Q.project(x, x0, none, sigma, sde.G, 0.7, 0.4, z, True, Pm), x)
    g, rn2, _ = Q.guidance(L.gaussian_score(sde, 0.8), sde, x, 0.5, x0, none, sigma, True, Pm, jacobian=False)
    assert (rn2 == 0).all() and (g == 0).all()


# ---------------------------------------------------------------- the row-mask rule of replacement
def test_masked_rows_need_orthogonal_rows():
    """P^+ diag(m) is the pseudo-inverse of diag(m) P only for mutually orthogonal rows.  Overlapping windows, one row hidden: since
    P P^+ = I the kept rows ARE still reproduced (P x' = P x + m . (y - P x)), but the update is no longer the orthogonal projection
    onto {x : (P x)_kept = y_kept}: it moves x further than pinv(diag(m) P) does, because it also pins P x on the hidden row, and
    P^+ diag(m) P is not symmetric -- and the validator refuses that mask."""
    from fourierdiffusion_amd.sampling.masks import LinearOperator, lowpass_operator, moving_average_operator
    T = 12
    Pm = moving_average_operator(T, 4, 2)
    rs = np.random.RandomState(0)
    mu, sigma = np.zeros((T, 1)), np.ones((T, 1))
    y = Q.P(rs.randn(1, T, 1), Pm)
    m = np.ones(y.shape, bool)
    m[0, 2, 0] = False
    x = rs.randn(1, T, 1)
    G = np.ones(T)
    xh = Q.project(x, Q.x0_obs(y, m, mu, sigma, False, Pm), m, sigma, G, 1.0, 0.0, 0.0 * x, False, Pm)
    assert np.abs(Q.P(xh, Pm)[m] - y[m]).max() <= 1e-12                               # kept rows: reproduced
    assert np.abs(Q.P(xh, Pm)[~m] - Q.P(x, Pm)[~m]).max() <= 1e-12                    # the hidden row of P x: pinned, not free
    keep = m[0, :, 0]
    Pk = Pm[keep]                                                                     # the true projection: the kept rows alone
    xo = x + np.einsum("tm,bmc->btc", np.linalg.pinv(Pk), y[:, keep] - Q.P(x, Pk))
    assert np.abs(Q.P(xo, Pk) - y[:, keep]).max() <= 1e-12
    far = np.abs(xh - xo).max()
    assert far > 1e-2, far                                                            # ... which P^+ diag(m) is NOT
    assert np.linalg.norm(xh - x) > np.linalg.norm(xo - x) * (1 + 1e-3)               # (it moves x further than necessary)
    proj = np.linalg.pinv(Pm) @ np.diag(keep.astype(float)) @ Pm
    np.testing.assert_allclose(proj @ proj, proj, atol=1e-12)                         # idempotent, but oblique:
    assert np.abs(proj - proj.T).max() > 1e-2
    assert np.abs(np.linalg.pinv(Pm) @ np.diag(keep.astype(float)) - np.linalg.pinv(np.diag(keep.astype(float)) @ Pm)).max() > 1e-2
    full = np.ones(y.shape, bool)
    xf = Q.project(x, Q.x0_obs(y, full, mu, sigma, False, Pm), full, sigma, G, 1.0, 0.0, 0.0 * x, False, Pm)
    assert np.abs(Q.P(xf, Pm) - y).max() <= 1e-12                                     # ... while the full mask reproduces all of them
    op = LinearOperator(Pm)
    assert not op.rows_orthogonal
    with pytest.raises(ValueError, match="orthogonal"):
        op.check_row_mask(torch.from_numpy(m), "impute")
    op.check_row_mask(torch.from_numpy(full), "impute")
    cols = torch.tensor([[True, False, True]]).expand(op.M, 3)                        # whole (series, channel) columns: fine
    op.check_row_mask(cols, "impute")
    # orthonormal rows: the same experiment IS the orthogonal projection on the kept rows, and any mask passes
    Pl = lowpass_operator(T, 3)
    yl = Q.P(rs.randn(1, T, 1), Pl)
    ml = np.ones(yl.shape, bool)
    ml[0, 2, 0] = False
    xl = Q.project(x, Q.x0_obs(yl, ml, mu, sigma, False, Pl), ml, sigma, G, 1.0, 0.0, 0.0 * x, False, Pl)
    assert np.abs(Q.P(xl, Pl)[ml] - yl[ml]).max() <= 1e-12
    kl = ml[0, :, 0]
    xlo = x + np.einsum("tm,bmc->btc", np.linalg.pinv(Pl[kl]), yl[:, kl] - Q.P(x, Pl[kl]))
    assert np.abs(xl - xlo).max() <= 1e-12
    LinearOperator(Pl).check_row_mask(torch.from_numpy(ml), "impute")


# ---------------------------------------------------------------- argument checks, before any device work
def _sampler(T=20, C=3, n_classes=0):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler()
    sch.set_noise_scaling(T)
    kw = dict(n_classes=n_classes) if n_classes else {}
    m = ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, d_model=8, num_layers=1, n_head=4, **kw)
    return DiffusionSampler(score_model=m, sample_batch_size=4)


@pytest.mark.parametrize("bad", ["wrong_T", "rank", "condition", "not_matrix", "aggregate", "resample", "smc", "obs_fine", "obs_M",
                                 "mask_fine", "mask_M", "mask_dtype"])
@pytest.mark.parametrize("conditioning", ["replace", "dps"])
def test_impute_rejects_bad_operator_arguments(bad, conditioning):
    """Every check runs before anything touches a device (this machine may have none).  T = 20, lowpass 4: M = 7."""
    from fourierdiffusion_amd.sampling.masks import lowpass_operator
    s = _sampler()
    obs, mask = torch.zeros(2, 7, 3), torch.ones(2, 7, 3, dtype=torch.bool)
    kw = dict(operator=lowpass_operator(20, 4), conditioning=conditioning)
    if bad == "wrong_T":
        kw["operator"] = lowpass_operator(24, 4)
    elif bad == "rank":
        kw["operator"] = np.ones((2, 20))
    elif bad == "condition":
        kw["operator"] = np.vstack([np.ones(20), np.ones(20) + 1e-6 * np.arange(20)])
    elif bad == "not_matrix":
        kw["operator"] = np.ones(20)
    elif bad == "aggregate":
        kw.update(aggregate=3)
    elif bad == "resample":
        kw.update(resample=2)
    elif bad == "smc":
        kw.update(conditioning="smc", num_samples=4, obs_std=0.1)
    elif bad == "obs_fine":
        obs = torch.zeros(2, 20, 3)
    elif bad == "obs_M":
        obs = torch.zeros(2, 6, 3)
    elif bad == "mask_fine":
        mask = torch.ones(2, 20, 3, dtype=torch.bool)
    elif bad == "mask_M":
        mask = torch.ones(6, 3, dtype=torch.bool)
    elif bad == "mask_dtype":
        mask = torch.ones(7, 3)
    with pytest.raises(ValueError):
        s.impute(obs, mask, 5, fourier_transform=True, **kw)


@pytest.mark.parametrize("conditioning", ["replace", "dps"])
@pytest.mark.parametrize("guide", [dict(y=1), dict(cfg_scale=2.0), dict(y=0, cfg_scale=1.5)])
def test_impute_rejects_operator_with_labels_or_cfg(conditioning, guide):
    from fourierdiffusion_amd.sampling.masks import lowpass_operator
    Pm = lowpass_operator(20, 4)
    obs, mask = torch.zeros(2, 7, 3), torch.ones(7, 3, dtype=torch.bool)
    for n_classes in (0, 3):
        with pytest.raises(ValueError):
            _sampler(n_classes=n_classes).impute(obs, mask, 5, fourier_transform=True, operator=Pm, conditioning=conditioning, **guide)
    X = torch.zeros(2, 20, 3)
    with pytest.raises(ValueError, match="operator"):
        _sampler(n_classes=3).impute_guidance(X, X, mask, 0.5, fourier_transform=True, operator=Pm, **guide)


def test_replace_refuses_row_masks_on_overlapping_rows():
    from fourierdiffusion_amd.sampling.masks import LinearOperator, moving_average_operator
    s = _sampler()
    op = LinearOperator(moving_average_operator(20, 4, 2))                            # M = 9
    obs = torch.zeros(2, 9, 3)
    mask = torch.ones(2, 9, 3, dtype=torch.bool)
    mask[1, 4, 2] = False
    with pytest.raises(ValueError, match="orthogonal"):
        s.impute(obs, mask, 5, fourier_transform=True, operator=op)
    X = torch.zeros(2, 20, 3)
    with pytest.raises(ValueError, match="orthogonal"):
        s.impute_project(X, X, mask, 0.5, fourier_transform=True, operator=op)


def test_step_wise_twins_reject_bad_operator_arguments():
    from fourierdiffusion_amd.sampling.masks import lowpass_operator
    s = _sampler()
    Pm = lowpass_operator(20, 4)
    X, mask = torch.zeros(2, 20, 3), torch.ones(7, 3, dtype=torch.bool)
    for kw in (dict(operator=Pm, aggregate=3), dict(operator=lowpass_operator(24, 4)), dict(operator=np.ones((2, 20)))):
        with pytest.raises(ValueError):
            s.impute_project(X, X, mask, 0.5, fourier_transform=True, **kw)
        with pytest.raises(ValueError):
            s.impute_guidance(X, X, mask, 0.5, fourier_transform=True, **kw)
        with pytest.raises(ValueError):
            s.observed_to_sample_space(torch.zeros(2, 7, 3), mask, fourier_transform=True, **kw)
    with pytest.raises(ValueError):
        s.impute_project(X, X, mask, 0.5, fourier_transform=True, operator=Pm, renoise_to=0.8)
    with pytest.raises(ValueError):
        s.impute_guidance(X, X, torch.ones(20, 3, dtype=torch.bool), 0.5, fourier_transform=True, operator=Pm)
    with pytest.raises(ValueError):
        s.observed_to_sample_space(torch.zeros(2, 20, 3), mask, fourier_transform=True, operator=Pm)


def test_impute_config_composes_with_the_operator_block(tmp_path):
    from fourierdiffusion_amd.config import compose
    conf = os.path.join(ROOT, "cmd", "conf")
    base = compose(conf, "impute", [], cwd=str(tmp_path))
    assert base.operator.kind is None and base.aggregate == 1
    cfg = compose(conf, "impute", ["operator.kind=gaussian_blur", "operator.sigma=1.5", "operator.stride=2", "mask.kind=forecast"],
                  cwd=str(tmp_path))
    assert cfg.operator.kind == "gaussian_blur" and cfg.operator.sigma == 1.5 and cfg.operator.stride == 2
    assert cfg.operator.max_condition == 1e4 and cfg.mask.kind == "forecast"
