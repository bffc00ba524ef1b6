"""Float64 restatement of class-conditional score models and classifier-free guidance (ScoreModule(n_classes=K),
DiffusionSampler.sample / sample_ode with y and cfg_scale, csrc/fd_cfg.hip), built from the oracle without changing it.  Shared by
tests/test_cfg_cpu.py and tests/test_gpu_cfg.py.

The labelled forward: for a batch whose rows all carry label k, the labelled network IS the unlabelled network with table[k] added
to time_encoder.dense.bias (the class embedding is added to the time embedding, which is emb Wd^T + bd).  ``score`` therefore calls
oracle.fdiff_oracle.score_forward once per label value present, on that label's rows, and stitches the rows back together.  Row K
of the table is the null (unconditional) token; a missing label (y = None) reads it.

The guided score is s = w s(x, t, y) + (1 - w) s(x, t, null); the guided reverse-SDE step is the oracle's sde_step on it, the guided
ODE solvers are those of tests/ode_ref.py and tests/dpm_ref.py with it as their score function.
"""
import numpy as np

from oracle import fdiff_oracle as O
from oracle import weights as W
from tests import dpm_ref as D
from tests import ode_ref as R

CFG = dict(T=24, C=4, D=72, L=2, H=12)        # 16-byte path: C % 4 == 0, on-device noise possible (T C % 4 == 0)
CFG_TAIL = dict(T=21, C=3, D=72, L=2, H=12)   # scalar tail, T no multiple of 16: injected noise only
K = 3
B = 5
N_STEPS = 8


def table(d_model, n_classes=K, seed=7):
    """class_encoder.weight (n_classes + 1, d_model), N(0, 1) like nn.Embedding; row n_classes = null token."""
    return W.randn(f"cfg_table_{n_classes}_{d_model}", (n_classes + 1, d_model), seed).astype(np.float32)


def state_dict(cfg, tab, seed=1234):
    """(unlabelled oracle weights, the same plus class_encoder.weight: what a labelled ScoreModule loads)."""
    sd = W.make_state_dict(cfg["C"], cfg["T"], cfg["D"], cfg["L"], seed=seed)
    return sd, dict(sd, **{"class_encoder.weight": tab})


def labels_or_null(y, n, n_classes):
    return np.full((n,), n_classes, dtype=np.int64) if y is None else np.asarray(y, dtype=np.int64)


def score(sd, tab, X, t, y, n_head):
    """The labelled network on (X, t, y) in float64: one oracle forward per label value present."""
    X = np.asarray(X, dtype=np.float64)
    t = np.asarray(t, dtype=np.float32)
    y = labels_or_null(y, X.shape[0], tab.shape[0] - 1)
    out = np.empty_like(X)
    for k in np.unique(y):
        rows = np.nonzero(y == k)[0]
        p = dict(sd)
        p["time_encoder.dense.bias"] = np.asarray(sd["time_encoder.dense.bias"], dtype=np.float64) + np.asarray(tab[k], dtype=np.float64)
        out[rows] = O.score_forward(p, X[rows], t[rows], n_head)
    return out


def guided_score_fn(sd, tab, y, w, n_head):
    """score_fn(x, t) of the guided model: w s_cond + (1 - w) s_uncond (one evaluation where the other's weight is zero)."""
    def fn(x, t):
        tb = np.full((x.shape[0],), t, dtype=np.float32)
        if y is None or w == 0.0:
            return score(sd, tab, x, tb, None, n_head)
        sc = score(sd, tab, x, tb, y, n_head)
        if w == 1.0:
            return sc
        return w * sc + (1.0 - w) * score(sd, tab, x, tb, None, n_head)
    return fn


def sample_sde(sd, tab, sde, z_prior, z_steps, y, w, n_head, eps=1e-5):
    """The guided reverse-SDE loop for one batch with injected noise (O.sample_trajectory with the guided score)."""
    fn = guided_score_fn(sd, tab, y, w, n_head)
    ts, dt = O.timesteps(len(z_steps), eps)
    X = O.prior_sampling(sde, z_prior)
    for i, t in enumerate(ts):
        X = O.sde_step(sde, fn(X, float(t)), float(t), X, z_steps[i], float(dt))
    return X


def sample_ode(sd, tab, sde, z_prior, N, solver, y, w, n_head, schedule="time", eps=1e-5):
    """The guided probability-flow ODE for one batch: Euler / Heun (tests/ode_ref.py), DDIM / DPM-Solver++ 2M (tests/dpm_ref.py)."""
    fn, x, ts = guided_score_fn(sd, tab, y, w, n_head), O.prior_sampling(sde, z_prior), D.grid(sde, N, schedule, eps)
    if solver in ("euler", "heun"):
        return R.solve(sde, fn, x, ts, solver)
    return D.solve(sde, fn, x, ts, solver)


# ---------------------------------------------------------------------------------------------------- gradients (torch CPU, float64)
def class_table_grad(sd, tab, sde, X, t, z, y, n_head, dim_ff=2048):
    """(loss, d loss / d class_encoder.weight, d loss / d time_encoder.dense.bias, d loss / d temb (B, D)) of the denoising
    score-matching loss (default weighting, dropout 0) by torch autograd in float64: an nn.TransformerEncoder loaded with the same
    weights between the same embedding and unembedding, the class embedding added to the time embedding."""
    import math

    import torch

    from tests import autograd_ref
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    Dm = sd["embedder.weight"].shape[0]
    enc = autograd_ref.encoder(sd, n_head, dim_ff)      # (nn.TransformerEncoder in float64, train mode, dropout 0)
    tabp = f64(tab).requires_grad_(True)
    bias = f64(sd["time_encoder.dense.bias"]).requires_grad_(True)
    Xn, target, std = O.perturb(sde, X, t, z)
    yv = torch.tensor(labels_or_null(y, Xn.shape[0], tab.shape[0] - 1))
    pe = f64(O.renorm_rows(sd["pos_encoder.embedding.weight"], math.sqrt(Dm)))
    emb = f64(O.gfp_embedding(t, sd["time_encoder.W"], Dm))
    temb = emb @ f64(sd["time_encoder.dense.weight"]).T + bias + tabp[yv]
    temb.retain_grad()
    h = f64(Xn) @ f64(sd["embedder.weight"]).T + f64(sd["embedder.bias"]) + pe[None, :Xn.shape[1]] + temb[:, None, :]
    out = enc(h) @ f64(sd["unembedder.weight"]).T + f64(sd["unembedder.bias"])
    stdt = f64(std)
    wgt = 1.0 / (1.0 / stdt ** 2).sum(dim=1)
    loss = (wgt[:, None, None] * (out + f64(target)) ** 2).reshape(out.shape[0], -1).mean(dim=-1).mean()
    loss.backward()
    return float(loss.detach()), tabp.grad.numpy(), bias.grad.numpy(), temb.grad.numpy()
