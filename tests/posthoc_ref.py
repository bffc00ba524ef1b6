"""Float64 restatement of the post-hoc scores (csrc/fd_posthoc.hip, utils/posthoc.py): torch on the CPU.

    network     tests/bb_autograd_ref.Net("lstm", ...) at diffusion time 0
    heads       predict:  mean over b, t < T - 1, c of |out[b,t,c] - x[b,t+1,c]|
                classify: mean_b softplus(l_b) - y_b l_b,  l_b = mean_c out[b, T - 1, c]       (torch autograd gives the gradients)
    optimiser   torch.optim.AdamW (its defaults, constant lr) in the dtype of the network
    index rule  row j of step s takes word j % 4 of Philox counter offset + s ceil(B / 4) + j / 4 under the key seed;
                idx = (uint64(word) n) >> 32, n the size of the pool the row draws from -- classify: rows j < B / 2 from a (label 1),
                the others from b (label 0); predict: every row from a.  `indices_from_words` takes the RAW words, so the GPU test feeds
                it fd_philox_words and the CPU test the oracle's Philox.

dtype=torch.float32 runs the same restatement in float32: a rounding yardstick only, never a reference."""
import numpy as np
import torch

from oracle import fdiff_oracle as O
from tests.bb_autograd_ref import Net

PHI = 0.9


# ------------------------------------------------------------------------------------------------ index rule
def counters_per_step(B):
    return (B + 3) // 4


def indices_from_words(words, B, na, nb=None):
    """words: (ceil(B / 4), 4) uint32 of one step.  nb=None: the predict task.  (idx (B,) int64, label (B,) int64)."""
    w = np.asarray(words, dtype=np.uint64).reshape(-1)[:B]
    j = np.arange(B)
    from_b = (j >= B // 2) if nb is not None else np.zeros(B, dtype=bool)
    n = np.where(from_b, np.uint64(nb if nb is not None else 1), np.uint64(na))
    idx = (w * n) >> np.uint64(32)
    return idx.astype(np.int64), np.where(from_b, 0, 1).astype(np.int64)


def step_indices(seed, offset, step, B, na, nb=None):
    """The rule on the oracle's Philox (no GPU)."""
    words = O.engine_philox_words(int(seed), int(offset) + int(step) * counters_per_step(B), counters_per_step(B))
    return indices_from_words(words, B, na, nb)


def gather(a, b, idx, label, mean, inv_std):
    """(B, T, C) float32: (pool[idx] - mean) * inv_std in float32, one rounding each, as the gather kernel."""
    a = np.asarray(a, dtype=np.float32)
    rows = a[idx].copy()
    if b is not None:
        from_b = np.asarray(label) == 0
        rows[from_b] = np.asarray(b, dtype=np.float32)[idx[from_b]]
    return (rows - np.asarray(mean, dtype=np.float32)) * np.asarray(inv_std, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ heads
def head(task, out, x=None, label=None):
    """(loss (scalar tensor), per_series (B,) tensor) of the outputs `out` (B, T, C); x and label in out's dtype."""
    B, T, C = out.shape
    if task == "predict":
        if T < 2:
            raise ValueError("predict needs T >= 2")
        err = (out[:, :-1] - x[:, 1:]).abs()
        return err.mean(), err.sum(dim=(1, 2))
    logit = out[:, -1].mean(dim=1)
    return (torch.nn.functional.softplus(logit) - label * logit).mean(), logit


def head_with_grad(task, out, x=None, label=None):
    """float64 numpy: dict(loss, dout, per_series).  torch's |.| has subgradient 0 at 0: sign(0) = 0."""
    o = torch.tensor(np.asarray(out, dtype=np.float64), requires_grad=True)
    xt = None if x is None else torch.tensor(np.asarray(x, dtype=np.float64))
    yt = None if label is None else torch.tensor(np.asarray(label, dtype=np.float64))
    loss, per = head(task, o, xt, yt)
    loss.backward()
    return dict(loss=float(loss.detach()), dout=o.grad.numpy(), per_series=per.detach().numpy())


# ------------------------------------------------------------------------------------------------ training
class Fit:
    """The network and torch.optim.AdamW in one dtype."""

    def __init__(self, sd, lr, dtype=torch.float64):
        self.net, self.dtype = Net("lstm", sd, dtype), dtype
        self.opt = torch.optim.AdamW(list(self.net.params.values()), lr=lr)

    def forward(self, x):
        return self.net.forward(torch.tensor(np.asarray(x, dtype=np.float64)).to(self.dtype), 0.0)

    def step(self, task, x, label=None):
        """One step on the standardised batch x (B, T, C): (loss before the update, max |out|)."""
        xt = torch.tensor(np.asarray(x, dtype=np.float64)).to(self.dtype)
        yt = None if label is None else torch.tensor(np.asarray(label, dtype=np.float64)).to(self.dtype)
        self.opt.zero_grad()
        out = self.net.forward(xt, 0.0)
        loss, _ = head(task, out, xt, yt)
        loss.backward()
        self.opt.step()
        return float(loss.detach()), float(out.detach().abs().max())

    def evaluate(self, task, x):
        with torch.no_grad():
            xt = torch.tensor(np.asarray(x, dtype=np.float64)).to(self.dtype)
            out = self.net.forward(xt, 0.0)
            return head(task, out, xt, torch.zeros(xt.shape[0], dtype=self.dtype))[1].double().numpy()


def fit(task, sd, a, b, mean, inv_std, idx_trace, lr, dtype=torch.float64):
    """Trains on the batches the index trace (steps, B) names.  dict(loss (steps,), out_max (steps,), fit)."""
    f = Fit(sd, lr, dtype)
    idx_trace = np.asarray(idx_trace, dtype=np.int64)
    B = idx_trace.shape[1]
    label = np.where(np.arange(B) >= B // 2, 0, 1) if task == "classify" else np.ones(B, dtype=np.int64)
    loss, out_max = [], []
    for idx in idx_trace:
        x = gather(a, b if task == "classify" else None, idx, label, mean, inv_std)
        l, m = f.step(task, x, label if task == "classify" else None)
        loss.append(l)
        out_max.append(m)
    return dict(loss=np.array(loss), out_max=np.array(out_max), fit=f)


def index_trace(seed, steps, B, na, nb=None, offset=0):
    return np.stack([step_indices(seed, offset, s, B, na, nb)[0] for s in range(steps)])


# ------------------------------------------------------------------------------------------------ data and scores
def ar1(n, T, C, seed, phi=PHI):
    """AR(1) series with unit marginal variance, (n, T, C) float32."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, T, C))
    x = np.empty((n, T, C))
    x[:, 0] = e[:, 0]
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + np.sqrt(1.0 - phi * phi) * e[:, t]
    return x.astype(np.float32)


def noise(n, T, C, seed):
    return np.random.default_rng(seed).standard_normal((n, T, C)).astype(np.float32)


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    sd = x.std(axis=(0, 1))
    return x.mean(axis=(0, 1)).astype(np.float32), np.where(sd > 0, 1.0 / np.where(sd > 0, sd, 1.0), 1.0).astype(np.float32)


def discriminative_score(sd, real, generated, seed, steps, B, lr, test_fraction=0.2):
    n = min(len(real), len(generated))
    n_test = max(1, int(round(n * test_fraction)))
    mean, inv = stats(real)
    a, b = real[n_test:n], generated[n_test:n]
    run = fit("classify", sd, a, b, mean, inv, index_trace(seed, steps, B, len(a), len(b)), lr)
    lr_, lg = (run["fit"].evaluate("classify", (s[:n_test] - mean) * inv) for s in (real, generated))
    acc = 0.5 * ((lr_ > 0).mean() + (lg <= 0).mean())
    return abs(acc - 0.5)


def predictive_score(sd, train_set, test_set, seed, steps, B, lr):
    mean, inv = stats(test_set)
    run = fit("predict", sd, train_set, None, mean, inv, index_trace(seed, steps, B, len(train_set)), lr)
    T, C = test_set.shape[1:]
    return run["fit"].evaluate("predict", (test_set - mean) * inv).sum() / (len(test_set) * (T - 1) * C)
