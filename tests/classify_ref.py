"""Float64 restatement of the label-aware post-hoc score (the multiclass task of csrc/fd_posthoc.hip and utils/posthoc.py): torch on
the CPU, on top of tests/posthoc_ref.py.

    network     tests/bb_autograd_ref.Net("lstm", ...) with Cn = max(C, K) channels at diffusion time 0; the series fill the input
                channels < C, the others are zero; the logits of series b are out[b, T - 1, :K]
    head        torch.nn.functional.cross_entropy on those logits (mean over the batch); torch autograd gives the gradient
    optimiser   torch.optim.AdamW (its defaults, constant lr) in the dtype of the network
    index rule  the Philox word of row j of step s is the one of tests/posthoc_ref.py.  Uniform: idx = (uint64(word) na) >> 32.
                Balanced: with `order` the rows sorted stably by class, `start` the offsets of the classes in it and P the number
                of classes that hold a row, row j of step s draws from the (s B + j) % P-th such class c in ascending order:
                idx = order[start[c] + ((uint64(word) count[c]) >> 32)].  `indices_from_words` takes the RAW words.

dtype=torch.float32 runs the same restatement in float32: a rounding yardstick only, never a reference."""
import numpy as np
import torch

from oracle import fdiff_oracle as O
from tests import posthoc_ref as R
from tests.bb_autograd_ref import Net

PHIS = (-0.6, 0.2, 0.9, 0.6, -0.2)


# ------------------------------------------------------------------------------------------------ index rule
def class_tables(labels, K):
    """(order (na,), start (K + 1,)): the rows sorted stably by class and where each class begins."""
    y = np.asarray(labels, dtype=np.int64)
    return np.argsort(y, kind="stable"), np.concatenate([[0], np.cumsum(np.bincount(y, minlength=K))]).astype(np.int64)


def indices_from_words(words, B, na, step=0, labels=None, K=None):
    """words: (ceil(B / 4), 4) uint32 of one step.  labels=None: the uniform draw; otherwise the balanced one.  idx (B,) int64."""
    w = np.asarray(words, dtype=np.uint64).reshape(-1)[:B]
    if labels is None:
        return ((w * np.uint64(na)) >> np.uint64(32)).astype(np.int64)
    order, start = class_tables(labels, K)
    count = np.diff(start)
    present = np.flatnonzero(count > 0)
    cls = present[(step * B + np.arange(B)) % len(present)]
    within = (w * count[cls].astype(np.uint64)) >> np.uint64(32)
    return order[start[cls] + within.astype(np.int64)]


def step_indices(seed, offset, step, B, na, labels=None, K=None):
    """The rule on the oracle's Philox (no GPU)."""
    cps = R.counters_per_step(B)
    words = O.engine_philox_words(int(seed), int(offset) + int(step) * cps, cps)
    return indices_from_words(words, B, na, step, labels, K)


def index_trace(seed, steps, B, na, labels=None, K=None, offset=0, first_step=0):
    return np.stack([step_indices(seed, offset, first_step + s, B, na, labels, K) for s in range(steps)])


def gather(a, idx, mean, inv_std, Cn):
    """(B, T, Cn) float32: (pool[idx] - mean) * inv_std in float32 in the channels < C, +0.0 in the others."""
    rows = R.gather(a, None, np.asarray(idx), None, mean, inv_std)
    x = np.zeros(rows.shape[:2] + (Cn,), dtype=np.float32)
    x[:, :, :rows.shape[2]] = rows
    return x


def pad(x, Cn):
    x = np.asarray(x)
    z = np.zeros(x.shape[:2] + (Cn,), dtype=x.dtype)
    z[:, :, :x.shape[2]] = x
    return z


# ------------------------------------------------------------------------------------------------ head
def head(out, K, label=None):
    """(loss or None, logp (B, K)) of the outputs `out` (B, T, Cn), tensors; label: int64 tensor."""
    logits = out[:, -1, :K]
    loss = None if label is None else torch.nn.functional.cross_entropy(logits, label)
    return loss, torch.log_softmax(logits, dim=1)


def head_with_grad(out, K, label):
    """float64 numpy: dict(loss, dout, logp, pred); argmax ties go to the lowest class."""
    o = torch.tensor(np.asarray(out, dtype=np.float64), requires_grad=True)
    loss, logp = head(o, K, torch.tensor(np.asarray(label, dtype=np.int64)))
    loss.backward()
    logits = o.detach().numpy()[:, -1, :K]
    return dict(loss=float(loss.detach()), dout=o.grad.numpy(), logp=logp.detach().numpy(), pred=np.argmax(logits, axis=1))


# ------------------------------------------------------------------------------------------------ training
class Fit(R.Fit):
    """The network and torch.optim.AdamW in one dtype, for the K-way task."""

    def __init__(self, sd, lr, K, dtype=torch.float64):
        super().__init__(sd, lr, dtype)
        self.K = K

    def step_multiclass(self, x, label):
        """One step on the padded standardised batch x (B, T, Cn): (loss before the update, max |out|)."""
        xt = torch.tensor(np.asarray(x, dtype=np.float64)).to(self.dtype)
        self.opt.zero_grad()
        out = self.net.forward(xt, 0.0)
        loss, _ = head(out, self.K, torch.tensor(np.asarray(label, dtype=np.int64)))
        loss.backward()
        self.opt.step()
        return float(loss.detach()), float(out.detach().abs().max())

    def predict(self, x):
        """(logp (n, K) float64, pred (n,)) of padded standardised series."""
        with torch.no_grad():
            out = self.net.forward(torch.tensor(np.asarray(x, dtype=np.float64)).to(self.dtype), 0.0)
            logp = head(out, self.K)[1].double().numpy()
        return logp, np.argmax(logp, axis=1)


def fit(sd, a, labels, K, mean, inv_std, idx_trace, lr, dtype=torch.float64):
    """Trains on the batches the index trace (steps, B) names.  dict(loss (steps,), out_max (steps,), fit)."""
    Cn = max(np.asarray(a).shape[2], K)
    f = Fit(sd, lr, K, dtype)
    labels = np.asarray(labels, dtype=np.int64)
    loss, out_max = [], []
    for idx in np.asarray(idx_trace, dtype=np.int64):
        l, m = f.step_multiclass(gather(a, idx, mean, inv_std, Cn), labels[idx])
        loss.append(l)
        out_max.append(m)
    return dict(loss=np.array(loss), out_max=np.array(out_max), fit=f)


# ------------------------------------------------------------------------------------------------ data and scores
def ar1_classes(n, T, C, K, seed):
    """n AR(1) series whose class k (uniform) sets phi = PHIS[k]: ((n, T, C) float32, (n,) int64)."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, K, size=n)
    phi = np.asarray(PHIS[:K])[y][:, None]
    e = rng.standard_normal((n, T, C))
    x = np.empty((n, T, C))
    x[:, 0] = e[:, 0]
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + np.sqrt(1.0 - phi * phi) * e[:, t]
    return x.astype(np.float32), y.astype(np.int64)


def confusion(labels, pred, K):
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (np.asarray(labels), np.asarray(pred)), 1)
    return cm


def scores(cm):
    cm = np.asarray(cm, dtype=np.float64)
    support = cm.sum(axis=1)
    present = support > 0
    recall = np.diag(cm)[present] / support[present]
    return dict(accuracy=float(np.trace(cm) / cm.sum()), balanced_accuracy=float(recall.mean()))


def classification_score(sd, train_set, train_labels, test_set, test_labels, K, stats_from, seed, steps, B, lr, balance=False):
    """dict(accuracy, balanced_accuracy, nll, confusion) of the restatement trained by the index rule on the oracle's Philox."""
    mean, inv = R.stats(stats_from)
    trace = index_trace(seed, steps, B, len(train_set), train_labels if balance else None, K)
    run = fit(sd, train_set, train_labels, K, mean, inv, trace, lr)
    Cn = max(train_set.shape[2], K)
    logp, pred = run["fit"].predict(pad((test_set - mean) * inv, Cn))
    cm = confusion(test_labels, pred, K)
    nll = float(-logp[np.arange(len(test_labels)), test_labels].mean())
    return dict(scores(cm), nll=nll, confusion=cm, loss=run["loss"])
