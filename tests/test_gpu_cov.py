"""GPU: covariate-conditional score models and classifier-free guidance on covariates (ScoreModule(cond_dim=P),
DiffusionSampler.sample / sample_ode with y = covariates and cfg_scale, csrc/fd_cov.hip; an extension not in the reference) against
the float64 restatement of tests/cov_ref.py.

Shapes: T = 24, C = 4 (16-byte path) and T = 21, C = 3 (scalar tail, T no multiple of 16; injected noise only), d_model 72, 12 heads,
2 layers, P = 3 covariates, B = 5 (2B = 10 rows in the guided forward), 8 steps.  Test 1 holds the encoder kernels alone to float64
with bounds derived from their operation counts; every later float64 reference adds the ENGINE's e (ScoreModule.cov_embedding) to
time_encoder.dense.bias, so the network-level bounds are those of tests/test_gpu_cfg.py.

Every test prints what it measures before it asserts.  First MI355X run: largest share of test 1's bounds 0.057 forward
and 0.326 backward; encoder gradients max-rel 3.3e-7 (fp32), 9.0e-3 (bf16, bf16 fused); guided SDE loop 3.2e-7 of max(1, max |x|),
guided ODE solvers at most 1.3e-6.  No bound here is taken from those figures.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests import cov_ref as R
from tests.gpu_util import DEV, dev, host, oracle_sde, report_err

pytestmark = pytest.mark.gpu
P, B, N = R.P, R.B, R.N_STEPS
KEEP_MIXED = [1, 0, 1, 1, 0]
VP = ("vp", (0.1, 20.0))
F32_ATOL = 5e-6                      # tests/test_gpu_score.py, fp32 golden forward
U = 2.0 ** -24                       # unit roundoff of fp32
TINY = 2.0 ** -126                   # (a result below the normal range may lose its last bits)
SUM_ROWS_U = 2.0 ** -24              # tests/test_gpu_cfg.py


def make_cov(cfg, precision, cond_dim=P, cond_dropout=0.0, sde=VP, **kw):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VEScheduler, VPScheduler
    kind, p = sde
    sch = (VPScheduler if kind == "vp" else VEScheduler)(p[0], p[1], fourier_noise_scaling=True)
    sch.set_noise_scaling(cfg["T"])
    enc = R.encoder(cfg["D"], cond_dim or P)
    sd, sd_cov = R.state_dict(cfg, enc)
    if cond_dim is not None:
        kw = dict(kw, cond_dim=cond_dim, cond_dropout=cond_dropout)
    m = ScoreModule(n_channels=cfg["C"], max_len=cfg["T"], noise_scheduler=sch, fourier_noise_scaling=True, d_model=cfg["D"],
                    num_layers=cfg["L"], n_head=cfg["H"], **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in (sd_cov if cond_dim else sd).items()}, strict=not kw.get("n_classes"))
    m.to(DEV)
    m.precision = m.train_precision = precision
    m.dropout = 0.0
    return m, sch, sd, enc


def batch_of(X, t, c=None):
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    return DiffusableBatch(X=dev(X), y=None if c is None else torch.as_tensor(c), timesteps=dev(t))


def inputs(cfg, tag):
    X = W.randn(f"cov_x_{tag}", (B, cfg["T"], cfg["C"]), 5)
    t = W.uniform(f"cov_t_{tag}", (B,), 5, 0.05, 1.0)
    z = W.randn(f"cov_z_{tag}", (B, cfg["T"], cfg["C"]), 5)
    return X, t, z


def engine_e(m, c, keep=None, n=B):
    """The engine's own added vectors (n, D) in float64: e(c) where kept, the null vector elsewhere / everywhere for c None."""
    if c is None:
        return np.tile(host(m.state_dict()["cov_encoder.null"]), (n, 1))
    return host(m.cov_embedding(torch.as_tensor(c), keep=None if keep is None else torch.tensor(keep)))


# ------------------------------------------------------------------------------------------------- 1. the encoder kernels alone
def raw_embed(enc, c, keep, Bn, Pn, Dn):
    from fourierdiffusion_amd import _C
    ctx = _C.ctx(torch.device(DEV, torch.cuda.current_device()))
    t = [dev(enc[k]) for k in R.NAMES]
    cd = None if c is None else dev(c)
    kd = None if keep is None else torch.tensor(keep, dtype=torch.uint8, device=DEV)
    out = torch.full((Bn, Dn), float("nan"), device=DEV)
    rc = _C.lib().fd_cov_embed(ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), _C.ptr(cd),
                               _C.ptr(kd), out.data_ptr(), Bn, Pn, Dn, _C.stream_of(out))
    _C.check(rc, ctx)
    return out


def raw_backward(enc, c, keep, dtemb, Bn, Pn, Dn, into=None):
    """fd_cov_embed_backward; into: the five output tensors of an earlier call (accumulate = 1), else fresh NaN-filled ones."""
    from fourierdiffusion_amd import _C
    ctx = _C.ctx(torch.device(DEV, torch.cuda.current_device()))
    t = [dev(enc[k]) for k in R.NAMES]
    cd = None if c is None else dev(c)
    kd = None if keep is None else torch.tensor(keep, dtype=torch.uint8, device=DEV)
    g = dev(dtemb)
    outs = into or [torch.full(tuple(enc[k].shape), float("nan"), device=DEV) for k in R.NAMES]
    rc = _C.lib().fd_cov_embed_backward(ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), _C.ptr(cd), _C.ptr(kd), g.data_ptr(),
                                        outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                        outs[4].data_ptr(), Bn, Pn, Dn, 1 if into else 0, _C.stream_of(g))
    _C.check(rc, ctx)
    return outs


def forward_bounds(enc, c):
    """Per-entry bounds on |h_gpu - h| (n, D) and |e_gpu - e| (n, D) for kept rows, from the kernel's operation counts.
    pre_j: a chain of P fmas onto b1_j, P + 1 terms: (P + 1) u sum |terms| (Higham, Accuracy and Stability, sec. 3.1).
    h_j = pre / (1 + exp(-pre)): expf is within 1 ulp = 2 u relative (HIP math API, expf: 1 ulp), the addition rounds once (u, and
    the exponential's error enters the sum with weight exp / (1 + exp) <= 1), the division is correctly rounded (HIP: 0 ulp off
    the IEEE result under the default -fhip-fp32-correctly-rounded-divide-sqrt, i.e. u): 4 u relative to first order, taken with
    1 % for the second-order terms; the error of pre enters through |silu'| <= 1.1.
    e_d: a chain of D fmas onto b2_d, D + 1 terms, on the computed h: (D + 1) u sum |terms| + sum_j |W2_dj| err_h_j."""
    W1, b1, W2, b2, _ = [np.asarray(enc[k], dtype=np.float64) for k in R.NAMES]
    c = np.asarray(c, dtype=np.float64)
    Pn, Dn = W1.shape[1], W1.shape[0]
    pre, h = R.hidden(enc, c)
    s1 = np.abs(b1)[None, :] + np.abs(c) @ np.abs(W1).T
    err_pre = (Pn + 1) * U * s1 + TINY
    err_h = 1.1 * err_pre + 4.04 * U * np.abs(h) + TINY
    s2 = np.abs(b2)[None, :] + (np.abs(h) + err_h) @ np.abs(W2).T
    err_e = (Dn + 1) * U * s2 + err_h @ np.abs(W2).T + TINY
    return err_pre, err_h, err_e


def backward_bounds(enc, c, keep, dtemb):
    """Per-entry bounds on the five gradients: every sum over rows is a chain of n fmas / additions, (n + 1) u sum |terms|, plus the
    propagated errors of h (forward_bounds) and of dpre = g silu'(pre): g_j a chain of D fmas from zero ((D + 1) u sum |terms|),
    silu'(x) = s (1 + x (1 - s)) with s within 4.04 u relative (as h), each of its four further operations rounding once, the error
    of pre entering through |silu''| <= 0.5, and one rounding for the product."""
    W1, b1, W2, b2, _ = [np.asarray(enc[k], dtype=np.float64) for k in R.NAMES]
    c = np.asarray(c, dtype=np.float64)
    g = np.asarray(dtemb, dtype=np.float64)
    k = np.asarray(keep).astype(bool)
    Dn = W1.shape[0]
    err_pre, err_h, _ = forward_bounds(enc, c)
    pre, h = R.hidden(enc, c)
    gj = g @ W2
    err_g = (Dn + 1) * U * (np.abs(g) @ np.abs(W2)) + TINY
    s = 1.0 / (1.0 + np.exp(-pre))
    a = 1.0 - s
    q = 1.0 + pre * a
    ds = s * q
    d_s = 4.04 * U * s
    err_a = d_s + U * np.abs(a)
    err_m = np.abs(pre) * err_a + U * np.abs(pre * a)
    err_q = err_m + U * np.abs(q)
    err_ds = np.abs(q) * d_s + s * err_q + U * np.abs(ds) + 0.5 * err_pre + TINY
    dpre = gj * ds
    err_dpre = np.abs(ds) * err_g + (np.abs(gj) + err_g) * err_ds + U * np.abs(dpre) + TINY
    kk = k[:, None].astype(np.float64)
    nk, nd = int(k.sum()), int((~k).sum())
    ga, ha, ca, da = np.abs(g) * kk, np.abs(h) * kk, np.abs(c) * kk, np.abs(dpre) * kk
    eh, ed = err_h * kk, err_dpre * kk
    return {
        R.NAMES[0]: (nk + 1) * U * ((da + ed).T @ ca) + ed.T @ ca + TINY,
        R.NAMES[1]: (nk + 1) * U * (da + ed).sum(axis=0) + ed.sum(axis=0) + TINY,
        R.NAMES[2]: (nk + 1) * U * (ga.T @ (ha + eh)) + ga.T @ eh + TINY,
        R.NAMES[3]: (nk + 1) * U * ga.sum(axis=0) + TINY,
        R.NAMES[4]: (nd + 1) * U * (np.abs(g) * (1.0 - kk)).sum(axis=0) + TINY,
    }


def keep_patterns(Bn):
    mixed = [(b * 7 + 3) % 5 not in (0, 3) for b in range(Bn)]
    if Bn == 1:
        return {"kept": [1], "dropped": [0]}
    return {"kept": [1] * Bn, "dropped": [0] * Bn, "mixed": [int(v) for v in mixed]}


@pytest.mark.parametrize("Bn", [1, 5, 300])
@pytest.mark.parametrize("Dn", [32, 72])
@pytest.mark.parametrize("Pn", [1, 7, 64])
def test_encoder_kernels_alone(Pn, Dn, Bn):
    enc = R.encoder(Dn, Pn)
    c = R.covariates(Bn, Pn)
    dtemb = W.randn(f"cov_dtemb_{Bn}_{Dn}", (Bn, Dn), 13).astype(np.float32)
    _, _, err_e = forward_bounds(enc, c)
    nul = torch.from_numpy(enc[R.NAMES[4]]).to(DEV)
    share_f, share_b = 0.0, 0.0
    for name, keep in keep_patterns(Bn).items():
        k = np.asarray(keep).astype(bool)
        # ---- forward
        e = raw_embed(enc, c, keep, Bn, Pn, Dn)
        assert torch.equal(e[torch.from_numpy(~k).to(DEV)], nul.expand(int((~k).sum()), Dn)), "dropped rows are the null vector, exactly"
        ref = R.encode(enc, c, keep)
        diff = np.abs(host(e) - ref)
        if k.any():
            share_f = max(share_f, float((diff[k] / err_e[k]).max()))
        assert (diff[k] <= err_e[k]).all(), (name, float((diff[k] / err_e[k]).max()))
        if name == "kept":
            assert torch.equal(e, raw_embed(enc, c, None, Bn, Pn, Dn)), "keep = NULL keeps every row"
        # ---- backward
        outs = raw_backward(enc, c, keep, dtemb, Bn, Pn, Dn)
        refg = R.encoder_grad(enc, c, keep, dtemb)
        bnd = backward_bounds(enc, c, keep, dtemb)
        for nm, o in zip(R.NAMES, outs):
            d = np.abs(host(o) - refg[nm].reshape(o.shape))
            bb = bnd[nm].reshape(o.shape)
            share_b = max(share_b, float((d / bb).max()))
            assert (d <= bb).all(), (name, nm, float((d / bb).max()))
        if name == "kept":
            assert not outs[4].any(), "kept rows contribute exactly zero to dnull"
        if name == "dropped":
            assert not any(bool(o.any()) for o in outs[:4]), "dropped rows contribute exactly zero to dW1, db1, dW2, db2"
        if name == "mixed":
            # the kept rows alone, in their order, are the same chains: bit for bit; likewise the dropped rows for dnull
            kc, kg = c[k], dtemb[k]
            only_kept = raw_backward(enc, kc, [1] * int(k.sum()), kg, int(k.sum()), Pn, Dn)
            for a, b_ in zip(outs[:4], only_kept[:4]):
                assert torch.equal(a, b_)
            only_drop = raw_backward(enc, c[~k], [0] * int((~k).sum()), dtemb[~k], int((~k).sum()), Pn, Dn)
            assert torch.equal(outs[4], only_drop[4])
        # two runs are bit-identical, and accumulate = 1 doubles the gradient bit for bit
        again = raw_backward(enc, c, keep, dtemb, Bn, Pn, Dn)
        for a, b_ in zip(outs, again):
            assert torch.equal(a, b_)
        raw_backward(enc, c, keep, dtemb, Bn, Pn, Dn, into=again)
        for a, b_ in zip(outs, again):
            assert torch.equal(2 * a, b_)
    # no covariates at all: the null vector on every row, its gradient the column sums
    assert torch.equal(raw_embed(enc, None, None, Bn, Pn, Dn), nul.expand(Bn, Dn))
    print(f"[cov] encoder kernels P={Pn} D={Dn} B={Bn}: largest share of the forward bound {share_f:.3f}, of the backward bounds {share_b:.3f}")


# ------------------------------------------------------------------------------------------------------------------ 2. forward
@pytest.mark.parametrize("which", ["mixed", "none"])
@pytest.mark.parametrize("cfg", [R.CFG, R.CFG_TAIL], ids=["T24C4", "T21C3"])
def test_forward_vs_float64(cfg, which, monkeypatch):
    from fourierdiffusion_amd import _rng
    X, t, _ = inputs(cfg, "fwd")
    c = R.covariates(B) if which == "mixed" else None
    for prec in ("fp32", "bf16"):
        m, _, sd, enc = make_cov(cfg, prec, cond_dropout=0.4)
        m.eval()
        out = host(m(batch_of(X, t, c)))        # eval never drops: every row its own covariates, or none
        e = engine_e(m, c)
        ref = R.score(sd, e, X, t, cfg["H"])
        if prec == "fp32":
            np.testing.assert_allclose(out, ref, atol=F32_ATOL, rtol=0)
        else:
            desc = m.plan(B)[0]
            assert "per-layer" in desc and "covariate-conditional" in desc, desc
            err, rms = report_err(f"cov forward bf16 T={cfg['T']} c={which}", out, ref)
            assert err <= 2e-2 and rms <= 1e-2, (err, rms)      # tests/test_gpu_baseline_shapes.py, per-layer path
        if c is not None and prec == "fp32":
            # rows with and without covariates in ONE batch: the exact-f32 training forward (layer dropout 0) under a key whose keep
            # bytes are KEEP_MIXED -- the kernels of the eval forward, so the same bound
            key = find_key(m, KEEP_MIXED, 0.4)
            monkeypatch.setattr(_rng, "stream", lambda: (key, 0))
            m.train()
            out = host(m(batch_of(X, t, c)))
            monkeypatch.undo()
            ref = R.score(sd, engine_e(m, c, KEEP_MIXED), X, t, cfg["H"])
            np.testing.assert_allclose(out, ref, atol=F32_ATOL, rtol=0)


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals():
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.models.score_models import LSTMScoreModule, MLPScoreModule, ScoreModule
    m, sch, _, _ = make_cov(R.CFG, "fp32")
    m.eval()
    X, t, _ = inputs(R.CFG, "fwd")
    ctx, h = m._engine()
    cd = dev(R.covariates(3))
    assert _C.lib().fd_score_set_covariates(h, cd.data_ptr(), 3) == 0
    out = torch.empty(B, R.CFG["T"], R.CFG["C"], device=DEV)
    rc = _C.lib().fd_score_forward(h, dev(X).data_ptr(), dev(t).data_ptr(), out.data_ptr(), B, 0, 0)
    assert rc == -1                                              # FD_ERR_ARG
    rc = _C.lib().fd_score_forward_train(h, dev(X).data_ptr(), dev(t).data_ptr(), out.data_ptr(), B, 0.0, 1, 0, 0)
    assert rc == -1
    assert _C.lib().fd_score_set_covariates(h, None, 0) == 0
    with pytest.raises(ValueError):
        m(batch_of(X, t, R.covariates(B, P + 1)))                # wrong P
    with pytest.raises(ValueError):
        m(batch_of(X, t, R.covariates(B - 1)))
    bad = R.covariates(B).copy()
    bad[2, 1] = np.inf
    with pytest.raises(ValueError):
        m(batch_of(X, t, bad))
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        m(batch_of(X, t, bad))
    with pytest.raises(ValueError):
        m(batch_of(X, t, torch.zeros(B, P, dtype=torch.int64)))
    with pytest.raises(ValueError):
        ScoreModule(n_channels=4, max_len=24, noise_scheduler=sch, d_model=72, num_layers=2, n_head=12, cond_dim=2, n_classes=3)
    with pytest.raises(ValueError):
        ScoreModule(n_channels=4, max_len=24, noise_scheduler=sch, d_model=72, num_layers=2, n_head=12, cond_dim=65)
    with pytest.raises(ValueError):
        MLPScoreModule(n_channels=4, max_len=24, noise_scheduler=sch, cond_dim=2)
    with pytest.raises(ValueError):
        LSTMScoreModule(n_channels=4, max_len=24, noise_scheduler=sch, cond_dim=2)
    hh = C.c_void_p()
    dims = _C.model_dims(4, 24, 72, 12, 2)
    assert _C.lib().fd_score_create_cov(ctx, C.byref(dims), 3, 2, C.byref(hh)) == -1
    # impute / impute_guidance / log_likelihood: covariates are not built there; without them they run on the null vector
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    s = DiffusionSampler(score_model=m, sample_batch_size=B)
    x = dev(X)
    with pytest.raises(ValueError, match="not built"):
        s.log_likelihood(x, N, y=torch.from_numpy(R.covariates(B)))
    with pytest.raises(ValueError, match="not built"):
        s.impute(x, torch.ones_like(x, dtype=torch.bool), N, fourier_transform=False, y=torch.from_numpy(R.covariates(B)))
    with pytest.raises(ValueError, match="not built"):
        s.impute(x, torch.ones_like(x, dtype=torch.bool), N, fourier_transform=False, cfg_scale=2.0)
    ll = s.log_likelihood(x, N)                                  # y=None: the null vector
    assert all(torch.isfinite(v).all() for v in vars(ll).values() if isinstance(v, torch.Tensor))
    s.corrector_steps = 1
    with pytest.raises(ValueError):
        s.sample(B, N, y=torch.from_numpy(R.covariates(B)))


# ------------------------------------------------------------------------------------- 4. nothing moved for cond_dim = 0
@pytest.mark.parametrize("n_classes", [0, 3])
def test_cond_dim_zero_is_the_parent_model_bit_for_bit(n_classes):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.utils.losses import get_sde_loss_fn
    cfg = R.CFG
    X, t, z = inputs(cfg, "zero")
    zp = dev(W.randn("cov_zero_p", (B, cfg["T"], cfg["C"]), 6))
    zs = dev(W.randn("cov_zero_s", (N, B, cfg["T"], cfg["C"]), 6))
    y = None if n_classes == 0 else torch.tensor([0, 2, 3, 0, 2])
    res = []
    for explicit in (True, False):
        torch.manual_seed(21)
        kw = dict(n_classes=n_classes, label_dropout=0.0) if n_classes else {}
        m, sch, sd, _ = make_cov(cfg, "bf16", cond_dim=0 if explicit else None, **kw)
        assert not any(k.startswith("cov_encoder") for k in m.state_dict())
        assert "cond_dim" not in m.hparams and "cond_dropout" not in m.hparams
        m.eval()
        desc, spw = m.plan(B)
        if n_classes == 0:
            assert spw >= 1 and "per-layer" not in desc, desc     # the persistent kernel
        assert "covariate" not in desc
        fwd = m(batch_of(X, t, y)).clone()
        kws = {} if y is None else dict(y=y, cfg_scale=1.7)
        smp = DiffusionSampler(score_model=m, sample_batch_size=B).sample(B, N, prior_noise=[zp], step_noise=[zs], **kws)
        m.train()
        m.zero_grad()
        loss = get_sde_loss_fn(sch, train=True)(m, batch_of(X, t, y), noise=dev(z))
        res.append((fwd, smp, loss.clone(), m.grads.clone(), m.flat_parameters.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 5. gradients
def find_key(m, want, p=0.4):
    """A Philox key whose keep bytes at offset 0 and dropout p are `want` (B = 5: one of 32 patterns, found within a few hundred
    keys): the training forward of a step that draws this key drops exactly those rows -- nothing in the engine is patched."""
    want = torch.tensor(want, dtype=torch.uint8)
    for key in range(1, 4000):
        if torch.equal(m.effective_keep(len(want), key, 0, p).cpu(), want):
            return key
    raise AssertionError("no key gives the keep pattern")


@pytest.mark.parametrize("form", ["fp32", "bf16", "bf16_fused"])
def test_encoder_gradient(form, monkeypatch):
    from fourierdiffusion_amd import _rng
    from fourierdiffusion_amd.utils.losses import get_sde_loss_fn
    cfg = R.CFG
    X, t, z = inputs(cfg, "grad")
    c = R.covariates(B)
    prec = "fp32" if form == "fp32" else "bf16"
    p_drop = 0.4
    m, sch, sd, enc = make_cov(cfg, prec, cond_dropout=p_drop)
    if form == "bf16":
        m._no_fused_dsm = True
    key = find_key(m, KEEP_MIXED, p_drop)
    monkeypatch.setattr(_rng, "stream", lambda: (key, 0))        # the one key of the step: dropout p = 0 in the layers, so only the keep bytes read it
    fn = get_sde_loss_fn(sch, train=True)

    def step(cc=c):
        return fn(m, batch_of(X, t, cc), noise=dev(z)).item()

    m.zero_grad()
    loss = step()
    assert m.train_mode_effective == prec
    gv = m.grad_views()
    got = {k: host(gv[k]) for k in R.NAMES + ("time_encoder.dense.bias",)}
    flat1 = m.grads.clone()
    ref_loss, r_enc, r_bias, r_temb = R.cov_grad(sd, enc, oracle_sde("vp", VP[1], True, cfg["T"]), X, t, z, c, KEEP_MIXED, cfg["H"])
    assert abs(loss - ref_loss) <= (2e-5 if prec == "fp32" else 1e-2) * abs(ref_loss), (loss, ref_loss)
    for name in R.NAMES + ("time_encoder.dense.bias",):
        g, r = got[name], (r_bias if name.startswith("time") else r_enc[name])
        mx = np.abs(g - r).max() / np.abs(r).max()
        l2 = np.linalg.norm(g - r) / np.linalg.norm(r)
        print(f"[cov] {form} d {name}: max-rel {mx:.3e}, l2-rel {l2:.3e}")
        if prec == "fp32":
            assert mx < 2e-4, (name, mx)                         # tests/test_gpu_train.py
        else:
            assert mx <= 8e-2 and l2 <= 3e-2, (name, mx, l2)     # tests/test_gpu_train_bf16.py, default width
    # db2 + dnull and d time_encoder.dense.bias are the same B numbers dtemb[b, d] per column, summed in two orders
    diff = np.abs(got[R.NAMES[3]] + got[R.NAMES[4]] - got["time_encoder.dense.bias"])
    bound = 1.25 * 2 * (B - 1) * SUM_ROWS_U * np.abs(r_temb).sum(axis=0)
    print(f"[cov] {form} db2 + dnull vs d time_encoder.dense.bias: max difference {diff.max():.3e}, largest share of the "
          f"summation-order bound {(diff / bound).max():.3f}")
    assert (diff <= bound).all(), (diff / bound).max()
    # accumulate = 1 doubles the gradient
    step()
    off0 = m._layout[-5][1]
    assert torch.equal(m.grads[off0:], 2 * flat1[off0:])
    assert torch.allclose(m.grads, 2 * flat1, rtol=1e-5, atol=1e-7)
    # two runs are bit-identical
    m.zero_grad()
    step()
    assert torch.equal(m.grads, flat1)
    # a batch with every row dropped (no covariates at all) leaves the four MLP gradients exactly zero
    m.zero_grad()
    step(None)
    gv = m.grad_views()
    for name in R.NAMES[:4]:
        assert not gv[name].any(), name
    assert gv[R.NAMES[4]].any()


# ------------------------------------------------------------------------------------------------------------------ 6. dropout
def test_covariate_dropout():
    from fourierdiffusion_amd.models.score_models import ScoreModule
    cfg = R.CFG
    m, sch, _, _ = make_cov(cfg, "fp32")
    K = 3
    mk = ScoreModule(n_channels=cfg["C"], max_len=cfg["T"], noise_scheduler=sch, d_model=cfg["D"], num_layers=cfg["L"],
                     n_head=cfg["H"], n_classes=K).to(DEV)
    n = 4096
    y = torch.arange(n) % K
    key, off = 0x1234_5678_9ABC, 1 << 20
    for p in (0.0, 0.25, 0.5, 1.0):
        keep = m.effective_keep(n, key, off, p).cpu()
        assert torch.equal(keep.bool(), mk.effective_labels(y, n, key, off, p=p).cpu() != K), p
    assert bool(m.effective_keep(n, key, off, 0.0).all()) and not bool(m.effective_keep(n, key, off, 1.0).any())
    keep = m.effective_keep(n, key, off, 0.25).cpu()
    dropped = int((keep == 0).sum())
    print(f"[cov] covariate dropout p = 0.25, B = 4096: {dropped} dropped rows")
    assert abs(dropped - 1024) <= 139, dropped                   # five binomial sigmas (tests/test_gpu_cfg.py, test_label_dropout)
    assert not torch.equal(m.effective_keep(n, key, off + 1024, 0.25).cpu(), keep)
    # the training forward really applies it, eval never does: a model that always drops
    X, t, _ = inputs(cfg, "drop")
    c = R.covariates(B)
    m1, _, _, _ = make_cov(cfg, "fp32", cond_dropout=1.0)
    m1.eval()
    m.eval()
    assert torch.equal(m1(batch_of(X, t, c)), m(batch_of(X, t, c)))
    m1.train()
    a = m1(batch_of(X, t, c)).clone()
    b = m1(batch_of(X, t, None)).clone()
    m.train()
    cc = m(batch_of(X, t, c)).clone()
    assert torch.equal(a, b) and not torch.equal(a, cc)


# ------------------------------------------------------------------------------- 7. guided loop against its step-wise composition
def run_cov(m, x0, c, w, zs, force_pair=False):
    """fd_sampler_run_cov on a (2B,T,C) buffer whose first half is x0; returns the whole buffer."""
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    s = DiffusionSampler(score_model=m, sample_batch_size=B)
    m.eval()
    Nn, ts_arr, dt = s._sde_grid(N)
    ctx, h, p, G, mode = s._engine_args()
    buf = torch.full((2 * B,) + tuple(x0.shape[1:]), float("nan"), device=DEV)
    buf[:B].copy_(x0)
    cd = None if c is None else dev(c)
    old = os.environ.pop("FDIFF_CFG_FORCE_PAIR", None)
    if force_pair:
        os.environ["FDIFF_CFG_FORCE_PAIR"] = "1"
    try:
        rc = _C.lib().fd_sampler_run_cov(h, C.byref(p), G.data_ptr(), ts_arr, Nn, dt, buf.data_ptr(), _C.ptr(cd), float(w),
                                         _C.ptr(zs), 0, 0, B, mode, _C.stream_of(buf))
    finally:
        os.environ.pop("FDIFF_CFG_FORCE_PAIR", None)
        if old is not None:
            os.environ["FDIFF_CFG_FORCE_PAIR"] = old
    _C.check(rc, ctx)
    return buf


def compose(m, sch, x0, c, w, zs):
    """The host loop over the public pieces: forwards on 2B rows (x twice) with the covariates bound and with none bound -- the
    conditional half of the first and the null half of the second are the rows of the loop's one forward with keep = [1 ; 0] --, the
    combine in torch fp32, fd_sde_step."""
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    m.eval()
    sch.set_timesteps(N)
    w32 = torch.tensor(np.float32(w), device=DEV)
    omw32 = torch.tensor(np.float32(1.0 - float(np.float32(w))), device=DEV)
    x = x0.clone()
    for i, tt in enumerate(sch.timesteps.tolist()):
        t2 = torch.full((2 * B,), tt, device=DEV, dtype=torch.float32)
        x2 = torch.cat([x, x]).contiguous()
        sc = m(DiffusableBatch(X=x2, y=torch.from_numpy(np.concatenate([c, c])), timesteps=t2))[:B]
        su = m(DiffusableBatch(X=x2, y=None, timesteps=t2))[B:]
        s = w32 * sc + omw32 * su
        x = sch.step(model_output=s.contiguous(), timestep=tt, sample=x, noise=zs[i]).prev_sample
    return x


@pytest.mark.parametrize("cfg", [R.CFG, R.CFG_TAIL], ids=["T24C4", "T21C3"])
def test_guided_loop_vs_composition_and_float64(cfg):
    m, sch, sd, enc = make_cov(cfg, "fp32")
    T, Cn = cfg["T"], cfg["C"]
    zp = W.randn(f"cov_loop_p_{T}", (B, T, Cn), 7)
    zs = W.randn(f"cov_loop_s_{T}", (N, B, T, Cn), 7)
    c = R.covariates(B)
    x0 = sch.prior_sampling((B, T, Cn), noise=dev(zp), device=torch.device(DEV))
    zsd = dev(zs)
    sde = oracle_sde("vp", VP[1], True, T)
    w = 1.7
    e_c, e_0 = engine_e(m, c), engine_e(m, None)
    ref = R.sample_sde(sd, e_c, e_0, sde, zp, zs, float(np.float32(w)), cfg["H"])
    comp = host(compose(m, sch, x0, c, w, zsd))
    buf = run_cov(m, x0, c, w, zsd)
    fused = host(buf[:B])
    scale = max(1.0, np.abs(ref).max())
    e_comp = np.abs(comp - ref).max() / scale
    e_fused = np.abs(fused - ref).max() / scale
    e_pair = np.abs(fused - comp).max() / scale
    print(f"[cov] guided SDE loop T={T} w=1.7: composition vs float64 {e_comp:.3e}, fused vs float64 {e_fused:.3e}, "
          f"fused vs composition {e_pair:.3e} (of max(1, max |x|))")
    assert e_comp <= 1e-5, e_comp                                 # the fp32 sampler's own bound (tests/test_gpu_dpm.py)
    assert e_pair <= 4 * e_comp and e_fused <= 5 * e_comp, (e_pair, e_fused, e_comp)
    assert torch.equal(buf[:B], buf[B:])
    # w = 1 and w = 0: the combine is exact, so the two-evaluation form is the composition bit for bit
    for wx in (1.0, 0.0):
        buf = run_cov(m, x0, c, wx, zsd, force_pair=True)
        assert torch.equal(buf[:B], buf[B:])
        assert torch.equal(buf[:B], compose(m, sch, x0, c, wx, zsd)), wx
        one = run_cov(m, x0, c, wx, zsd)                          # and the one-evaluation form is the same numbers
        assert torch.equal(one[:B], buf[:B]), wx


# ------------------------------------------------------------------------------------------------------------------ 8. ODE solvers
@pytest.mark.parametrize("solver", ["euler", "heun", "ddim", "dpmpp2m"])
@pytest.mark.parametrize("cfg", [R.CFG, R.CFG_TAIL], ids=["T24C4", "T21C3"])
def test_guided_ode_solvers_vs_float64(cfg, solver):
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    m, sch, sd, enc = make_cov(cfg, "fp32")
    T, Cn = cfg["T"], cfg["C"]
    zp = W.randn(f"cov_ode_p_{T}", (B, T, Cn), 9)
    s = DiffusionSampler(score_model=m, sample_batch_size=B)
    c = torch.from_numpy(R.covariates(B))
    sde = oracle_sde("vp", VP[1], True, T)
    w = 1.7
    e_c, e_0 = engine_e(m, c), engine_e(m, None)
    got = s.sample_ode(B, N, solver=solver, prior_noise=[dev(zp)], y=c, cfg_scale=w).numpy()
    ref = R.sample_ode(sd, e_c, e_0, sde, zp, N, solver, float(np.float32(w)), cfg["H"])
    err, _ = report_err(f"cov sample_ode f32 T={T} {solver} w=1.7", got, ref)
    assert err <= 1e-5, err                                       # tests/test_gpu_dpm.py / test_gpu_ode.py
    # w = 1: the unguided step-wise solver with the covariates bound
    one = s.sample_ode(B, N, solver=solver, prior_noise=[dev(zp)], y=c, cfg_scale=1.0)
    ctx, h = m._engine()
    cd = c.to(DEV).contiguous()
    _C.check(_C.lib().fd_score_set_covariates(h, cd.data_ptr(), B), ctx)
    try:
        bound = s.sample_ode(B, N, solver=solver, prior_noise=[dev(zp)])
    finally:
        _C.lib().fd_score_set_covariates(h, None, 0)
    assert torch.equal(one, bound)
    ref1 = R.sample_ode(sd, e_c, e_0, sde, zp, N, solver, 1.0, cfg["H"])
    err1, _ = report_err(f"cov sample_ode f32 T={T} {solver} w=1", one.numpy(), ref1)
    assert err1 <= 1e-5, err1


# ------------------------------------------------------------------------------------------------------------ 9. on-device noise
def test_on_device_noise_w1_equals_the_stepwise_sampler_with_covariates_bound():
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    cfg = R.CFG
    m, sch, _, _ = make_cov(cfg, "bf16")
    s = DiffusionSampler(score_model=m, sample_batch_size=B)
    zp = dev(W.randn("cov_dev_p", (B, cfg["T"], cfg["C"]), 8))
    c = torch.from_numpy(R.covariates(B))
    outs = []
    for _ in range(2):
        torch.manual_seed(11)
        outs.append(s.sample(B, N, prior_noise=[zp], y=c, cfg_scale=1.0))
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    torch.manual_seed(11)
    ctx, h = m._engine()
    cd = c.to(DEV).contiguous()
    _C.check(_C.lib().fd_score_set_covariates(h, cd.data_ptr(), B), ctx)
    try:
        ref = s.sample(B, N, prior_noise=[zp])
    finally:
        _C.lib().fd_score_set_covariates(h, None, 0)
    assert torch.equal(outs[0], ref)
    torch.manual_seed(11)
    w2 = s.sample(B, N, prior_noise=[zp], y=c, cfg_scale=2.0)
    torch.manual_seed(11)
    assert torch.equal(w2, s.sample(B, N, prior_noise=[zp], y=c, cfg_scale=2.0))
    assert torch.isfinite(w2).all() and not torch.equal(w2, outs[0])
    # one covariate row for every sample
    torch.manual_seed(11)
    same = s.sample(B, N, prior_noise=[zp], y=c[0], cfg_scale=2.0)
    torch.manual_seed(11)
    assert torch.equal(same, s.sample(B, N, prior_noise=[zp], y=c[0:1].expand(B, P).contiguous(), cfg_scale=2.0))


# ---------------------------------------------------------------------------------------------------------------- 10. end to end
def test_train_save_load_sample_end_to_end(tmp_path):
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticCovariatesDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    from fourierdiffusion_amd.trainer import Trainer
    torch.manual_seed(3)
    dm = SyntheticCovariatesDatamodule(data_dir=tmp_path, batch_size=16, fourier_transform=True, standardize=True, max_len=24,
                                       num_samples=160, n_channels=4)
    dm.prepare_data()
    dm.setup()
    assert dm.y_train.shape == (160, 2) and dm.y_train.dtype == torch.float32
    assert torch.allclose(dm.y_train.mean(dim=0), torch.zeros(2), atol=1e-5)
    sch = VPScheduler(fourier_noise_scaling=True)
    sch.set_noise_scaling(24)
    m = ScoreModule(n_channels=4, max_len=24, noise_scheduler=sch, d_model=72, num_layers=2, n_head=12, num_training_steps=30,
                    cond_dim=2, cond_dropout=0.25)
    before = {k: m.state_dict()[k].clone() for k in R.NAMES}
    Trainer(max_epochs=3, enable_progress_bar=False, default_root_dir=str(tmp_path), ema_decay=0.9).fit(m, dm)     # 3 x 10 steps
    after = {k: m.state_dict()[k].cpu() for k in R.NAMES}
    for k in R.NAMES:
        assert torch.isfinite(after[k]).all(), k
        assert bool(((after[k] - before[k]).abs() > 0).any()), k   # the null vector included: covariate dropout reached it
    m.save_checkpoint(tmp_path / "cov.ckpt")
    m2 = ScoreModule.load_from_checkpoint(tmp_path / "cov.ckpt", weights="auto").to(DEV)
    assert m2.weights_loaded == "ema" and m2.cond_dim == 2 and m2.cond_dropout == 0.25 and m2.n_classes == 0
    out = DiffusionSampler(score_model=m2, sample_batch_size=8).sample(8, N, y=dm.y_test[:8], cfg_scale=2.0)
    assert out.shape == (8, 24, 4) and torch.isfinite(out).all()
