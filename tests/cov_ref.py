"""Float64 restatement of covariate-conditional score models and classifier-free guidance on covariates (ScoreModule(cond_dim=P),
DiffusionSampler.sample / sample_ode with y = covariates and cfg_scale, csrc/fd_cov.hip), built from the oracle without changing it.
Shared by tests/test_cov_cpu.py and tests/test_gpu_cov.py.

The encoder: e(c) = W2 silu(W1 c + b1) + b2 with hidden width d_model, and a learned null vector wherever a row's covariates are
dropped (keep = 0) or absent.  The conditioned forward: the added vector acts as a per-row addition to time_encoder.dense.bias (the
time embedding is emb Wd^T + bd), so ``score`` calls oracle.fdiff_oracle.score_forward once per row with that row's vector added to
the bias.  The vector is an ARGUMENT here: the network-level GPU tests pass the engine's own e (ScoreModule.cov_embedding), which
test 1 of tests/test_gpu_cov.py holds to ``encode`` on its own, so that no network-level tolerance has to absorb the encoder's error.

The guided score is s = w s(x, t, c) + (1 - w) s(x, t, null); the guided reverse-SDE step is the oracle's sde_step on it, the guided
ODE solvers are those of tests/ode_ref.py and tests/dpm_ref.py with it as their score function.
"""
import numpy as np

from oracle import fdiff_oracle as O
from oracle import weights as W
from tests import cfg_ref
from tests import dpm_ref as D
from tests import ode_ref as R

CFG = cfg_ref.CFG              # T=24, C=4, D=72, L=2, H=12
CFG_TAIL = cfg_ref.CFG_TAIL    # T=21, C=3
P = 3
B = cfg_ref.B
N_STEPS = cfg_ref.N_STEPS
NAMES = ("cov_encoder.0.weight", "cov_encoder.0.bias", "cov_encoder.2.weight", "cov_encoder.2.bias", "cov_encoder.null")


def encoder(d_model, cond_dim=P, seed=11):
    """The five tensors in float32: the two linear layers uniform within +-1/sqrt(fan_in) like nn.Linear, a non-zero null vector."""
    k1, k2 = 1.0 / np.sqrt(cond_dim), 1.0 / np.sqrt(d_model)
    tag = f"{cond_dim}_{d_model}"
    return {
        NAMES[0]: W.uniform(f"cov_w1_{tag}", (d_model, cond_dim), seed, -k1, k1).astype(np.float32),
        NAMES[1]: W.uniform(f"cov_b1_{tag}", (d_model,), seed, -k1, k1).astype(np.float32),
        NAMES[2]: W.uniform(f"cov_w2_{tag}", (d_model, d_model), seed, -k2, k2).astype(np.float32),
        NAMES[3]: W.uniform(f"cov_b2_{tag}", (d_model,), seed, -k2, k2).astype(np.float32),
        NAMES[4]: (0.5 * W.randn(f"cov_null_{tag}", (d_model,), seed)).astype(np.float32),
    }


def covariates(n, cond_dim=P, seed=12, tag="c"):
    return W.randn(f"cov_{tag}_{n}_{cond_dim}", (n, cond_dim), seed).astype(np.float32)


def state_dict(cfg, enc, seed=1234):
    """(unlabelled oracle weights, the same plus the encoder: what a covariate ScoreModule loads)."""
    sd = W.make_state_dict(cfg["C"], cfg["T"], cfg["D"], cfg["L"], seed=seed)
    return sd, dict(sd, **enc)


def _f64(enc):
    return [np.asarray(enc[k], dtype=np.float64) for k in NAMES]


def silu(x):
    return x / (1.0 + np.exp(-x))


def dsilu(x):
    s = 1.0 / (1.0 + np.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def keep_or_all(keep, n, present=True):
    if not present:
        return np.zeros((n,), dtype=bool)
    return np.ones((n,), dtype=bool) if keep is None else np.asarray(keep).astype(bool)


def hidden(enc, c):
    """(pre, h) (n, D) in float64."""
    W1, b1, _, _, _ = _f64(enc)
    pre = np.asarray(c, dtype=np.float64) @ W1.T + b1
    return pre, silu(pre)


def encode(enc, c, keep=None, n=None):
    """e (n, D) in float64: the encoder on the kept rows, the null vector on the others; c None: the null vector on all n rows."""
    _, _, W2, b2, nul = _f64(enc)
    if c is None:
        return np.tile(nul, (n, 1))
    _, h = hidden(enc, c)
    e = h @ W2.T + b2
    k = keep_or_all(keep, e.shape[0])
    e[~k] = nul
    return e


def encoder_grad(enc, c, keep, dtemb):
    """The encoder's gradient for an injected dtemb (n, D), in float64: dict over NAMES, plus "dpre" and "h" (n, D; zero rows where
    dropped)."""
    W1, b1, W2, b2, nul = _f64(enc)
    g = np.asarray(dtemb, dtype=np.float64)
    n = g.shape[0]
    k = keep_or_all(keep, n, c is not None)
    cc = np.zeros((n, W1.shape[1])) if c is None else np.asarray(c, dtype=np.float64)
    pre, h = hidden(enc, cc)
    gk = g * k[:, None]
    h = h * k[:, None]
    dpre = (gk @ W2) * dsilu(pre)
    return {NAMES[0]: dpre.T @ cc, NAMES[1]: dpre.sum(axis=0), NAMES[2]: gk.T @ h, NAMES[3]: gk.sum(axis=0),
            NAMES[4]: (g * (~k)[:, None]).sum(axis=0), "dpre": dpre, "h": h}


def encoder_loss(enc, c, keep, dtemb):
    """sum(e * dtemb): the scalar whose gradient ``encoder_grad`` is (central differences in tests/test_cov_cpu.py)."""
    return float((encode(enc, c, keep, n=np.asarray(dtemb).shape[0]) * np.asarray(dtemb, dtype=np.float64)).sum())


# ---------------------------------------------------------------------------------------------------- the conditioned network
def score(sd, e, X, t, n_head):
    """The network on (X, t) with e[b] added to row b's time embedding, in float64: one oracle forward per row."""
    X = np.asarray(X, dtype=np.float64)
    t = np.asarray(t, dtype=np.float32)
    e = np.asarray(e, dtype=np.float64)
    bias = np.asarray(sd["time_encoder.dense.bias"], dtype=np.float64)
    out = np.empty_like(X)
    for b in range(X.shape[0]):
        p = dict(sd)
        p["time_encoder.dense.bias"] = bias + e[b]
        out[b:b + 1] = O.score_forward(p, X[b:b + 1], t[b:b + 1], n_head)
    return out


def guided_score_fn(sd, e_cond, e_null, w, n_head):
    """score_fn(x, t) of the guided model: w s_cond + (1 - w) s_uncond (one evaluation where the other's weight is zero); e_cond
    None: no covariates."""
    def fn(x, t):
        tb = np.full((x.shape[0],), t, dtype=np.float32)
        if e_cond is None or w == 0.0:
            return score(sd, e_null, x, tb, n_head)
        sc = score(sd, e_cond, x, tb, n_head)
        if w == 1.0:
            return sc
        return w * sc + (1.0 - w) * score(sd, e_null, x, tb, n_head)
    return fn


def sample_sde(sd, e_cond, e_null, sde, z_prior, z_steps, w, n_head, eps=1e-5):
    fn = guided_score_fn(sd, e_cond, e_null, w, n_head)
    ts, dt = O.timesteps(len(z_steps), eps)
    X = O.prior_sampling(sde, z_prior)
    for i, t in enumerate(ts):
        X = O.sde_step(sde, fn(X, float(t)), float(t), X, z_steps[i], float(dt))
    return X


def sample_ode(sd, e_cond, e_null, sde, z_prior, N, solver, w, n_head, schedule="time", eps=1e-5):
    fn, x, ts = guided_score_fn(sd, e_cond, e_null, w, n_head), O.prior_sampling(sde, z_prior), D.grid(sde, N, schedule, eps)
    if solver in ("euler", "heun"):
        return R.solve(sde, fn, x, ts, solver)
    return D.solve(sde, fn, x, ts, solver)


# ---------------------------------------------------------------------------------------------------- gradients (torch CPU, float64)
def cov_grad(sd, enc, sde, X, t, z, c, keep, n_head, dim_ff=2048):
    """(loss, {name: d loss / d tensor} over NAMES, d loss / d time_encoder.dense.bias, d loss / d temb (B, D)) of the denoising
    score-matching loss (default weighting, dropout 0) by torch autograd in float64: an nn.TransformerEncoder loaded with the same
    weights between the same embedding and unembedding, the encoder's output (or the null vector) added to the time embedding."""
    import math

    import torch

    from tests import autograd_ref
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    Dm = sd["embedder.weight"].shape[0]
    enc_net = autograd_ref.encoder(sd, n_head, dim_ff)
    pw = [f64(enc[k]).requires_grad_(True) for k in NAMES]
    W1, b1, W2, b2, nul = pw
    bias = f64(sd["time_encoder.dense.bias"]).requires_grad_(True)
    Xn, target, std = O.perturb(sde, X, t, z)
    n = Xn.shape[0]
    k = torch.tensor(keep_or_all(keep, n, c is not None))
    cc = torch.zeros(n, W1.shape[1], dtype=torch.float64) if c is None else f64(c)
    e = torch.nn.functional.silu(cc @ W1.T + b1) @ W2.T + b2
    add = torch.where(k[:, None], e, nul[None, :].expand_as(e))
    pe = f64(O.renorm_rows(sd["pos_encoder.embedding.weight"], math.sqrt(Dm)))
    emb = f64(O.gfp_embedding(t, sd["time_encoder.W"], Dm))
    temb = emb @ f64(sd["time_encoder.dense.weight"]).T + bias + add
    temb.retain_grad()
    h = f64(Xn) @ f64(sd["embedder.weight"]).T + f64(sd["embedder.bias"]) + pe[None, :Xn.shape[1]] + temb[:, None, :]
    out = enc_net(h) @ f64(sd["unembedder.weight"]).T + f64(sd["unembedder.bias"])
    stdt = f64(std)
    wgt = 1.0 / (1.0 / stdt ** 2).sum(dim=1)
    loss = (wgt[:, None, None] * (out + f64(target)) ** 2).reshape(out.shape[0], -1).mean(dim=-1).mean()
    loss.backward()
    grads = {name: (torch.zeros_like(p) if p.grad is None else p.grad).numpy() for name, p in zip(NAMES, pw)}
    return float(loss.detach()), grads, bias.grad.numpy(), temb.grad.numpy()
