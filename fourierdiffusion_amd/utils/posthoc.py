"""Post-hoc discriminative and predictive scores on the HIP engine (not in the reference; TimeGAN, Yoon et al. 2019, and TSGBench):

    discriminative score   train a classifier AFTER the fact to tell real series from generated ones; |accuracy - 0.5| on held-out
                           series of both (0: indistinguishable, 0.5: told apart every time)
    predictive score       train a next-step forecaster on one set, test it on another ("train on synthetic, test on real"); the mean
                           absolute error in standardised units

The network is the engine's causal sequence model, `LSTMScoreModule` at diffusion time 0 (embedder, unidirectional LSTM layers with a
residual, unembedder): its output at time t sees the inputs <= t only, so out[:, t] regressed on x[:, t + 1] is the forecaster and
the mean over channels of out[:, T - 1], which has seen the whole series, the classifier logit.  The minibatch draw, the two heads
with their gradients and the whole training loop run in csrc/fd_posthoc.hip (`fd_posthoc_fit`: one engine call per fit, no host
synchronisation between steps); everything is deterministic given the seed.  There is no CPU fallback.

Label-aware scores (RCGAN, Esteban et al. 2017; the classification accuracy score of Ravuri & Vinyals 2019):

    classification score   train a K-way classifier on one LABELLED set, test it on another: trained on the samples with the classes
                           they were asked for and tested on real series (TSTR), the other way round (TRTS), or on two real folds
                           (TRTR, the baseline)

`PosthocNetwork(n_classes=K)` is the same LSTM with max(C, K) channels: the series fill the first C input channels, the rest are
fed zeros, and out[:, T - 1, :K] are the K logits (`fd_posthoc_fit_multiclass`, `fd_posthoc_head_multiclass`)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _C

MAX_D_MODEL = 100          # the engine's LSTM limit: the widest W_hh the backward through time holds in the LDS
TASKS = {"classify": _C.FD_POSTHOC_CLASSIFY, "predict": _C.FD_POSTHOC_PREDICT}
MAX_CLASSES = _C.FD_POSTHOC_MAX_CLASSES          # one logit per thread of a workgroup
EVAL_CHUNK = 4096          # series per evaluation forward


def _task(task: str) -> int:
    if task not in TASKS:
        raise ValueError(f"task={task!r}: one of {tuple(TASKS)}")
    return TASKS[task]


def _count(name: str, value, lo: int) -> int:
    if isinstance(value, bool) or int(value) != value or value < lo:
        raise ValueError(f"{name}={value!r} must be an integer >= {lo}")
    return int(value)


def _n_classes(n_classes) -> int:
    if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or not 2 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"n_classes={n_classes!r} must be an integer from 2 to {MAX_CLASSES}")
    return int(n_classes)


def _labels(labels, n: int, n_classes: int, what: str = "labels") -> np.ndarray:
    """labels as an int64 (n,) numpy array on the host, checked: integer, one per series, in [0, n_classes)."""
    if labels is None:
        raise ValueError(f"{what} are missing: the multiclass task needs one class per series")
    y = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if y.dtype == np.bool_ or not np.issubdtype(y.dtype, np.integer):
        raise ValueError(f"{what} must be integer classes, got dtype {y.dtype}")
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError(f"{what} of shape {tuple(y.shape)} for {n} series: one class per series")
    y = y.astype(np.int64)
    if n and (y.min() < 0 or y.max() >= n_classes):
        raise ValueError(f"{what} must lie in [0, {n_classes}), got values from {int(y.min())} to {int(y.max())}")
    return y


def _series(x, what: str, shape: Optional[tuple] = None) -> torch.Tensor:
    """x as an (n, T, C) float32 tensor (wherever it lives)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise _C.FdError(f"{what} must be a torch.Tensor or a numpy array")
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"{what} must be a non-empty (n, T, C) array, got shape {tuple(x.shape)}")
    if shape is not None and tuple(x.shape[1:]) != tuple(shape):
        raise ValueError(f"{what} holds series of shape {tuple(x.shape[1:])}, expected {tuple(shape)}")
    return x.detach().float()


def _on_device(x: torch.Tensor, device) -> torch.Tensor:
    return x.to(device).contiguous()


def channel_stats(x) -> tuple[torch.Tensor, torch.Tensor]:
    """(mean, inv_std), float32 (C,) on the host: per channel over series and time, computed in float64; a constant channel keeps
    inv_std = 1."""
    x64 = _series(x, "the series the statistics come from").double().cpu()
    mean = x64.mean(dim=(0, 1))
    std = x64.std(dim=(0, 1), unbiased=False)
    inv = torch.where(std > 0, 1.0 / std, torch.ones_like(std))
    return mean.float(), inv.float()


def standardise(x: torch.Tensor, mean: torch.Tensor, inv_std: torch.Tensor) -> torch.Tensor:
    """(x - mean) * inv_std per channel in float32: the arithmetic of the gather kernel, bit for bit."""
    return ((x - mean.to(x.device)) * inv_std.to(x.device)).contiguous()


class PosthocNetwork:
    """The post-hoc network and its optimiser state.  `fit` trains it for a task on device-resident pools, `evaluate` returns the
    per-series logits (classify) or sums of absolute one-step errors (predict).  `n_classes=K` makes it the K-way classifier of the
    "multiclass" task: the module then has max(n_channels, K) channels (`net_channels`), the series still have `n_channels`."""

    def __init__(self, n_channels: int, max_len: int, d_model: int = 32, num_layers: int = 1, seed: int = 0, device=None,
                 n_classes: Optional[int] = None) -> None:
        from ..models.score_models import LSTMScoreModule
        from ..schedulers.sde import VPScheduler
        d_model = _count("d_model", d_model, 2)
        if d_model % 2 != 0 or d_model > MAX_D_MODEL:
            raise ValueError(f"d_model={d_model} must be even and <= {MAX_D_MODEL}, the widest LSTM the engine trains (its backward "
                             "through time keeps W_hh in the LDS)")
        self.n_channels, self.max_len = _count("n_channels", n_channels, 1), _count("max_len", max_len, 1)
        self.d_model, self.num_layers, self.seed = d_model, _count("num_layers", num_layers, 1), int(seed)
        self.n_classes = None if n_classes is None else _n_classes(n_classes)
        self.net_channels = self.n_channels if self.n_classes is None else max(self.n_channels, self.n_classes)
        # a throw-away scheduler: the backbone never sees a diffusion time other than 0
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(self.seed)
            self.module = LSTMScoreModule(n_channels=self.net_channels, max_len=self.max_len, noise_scheduler=VPScheduler(),
                                          d_model=d_model, num_layers=self.num_layers)
        if device is None:
            if not torch.cuda.is_available():
                raise _C.FdError("the post-hoc network trains on the HIP engine and no GPU is visible (no CPU fallback)")
            device = "cuda"
        self.module.to(device)
        flat = self.module.flat_parameters
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
        self.grads = torch.zeros_like(flat)
        self.steps_done = 0
        self.last_indices: Optional[torch.Tensor] = None      # (steps, batch_size) int32 of the last fit(trace_indices=True)

    @property
    def device(self) -> torch.device:
        return self.module.device

    def load_state_dict(self, state_dict) -> None:
        """Weights under LSTMScoreModule's names; the optimiser starts over."""
        self.module.load_state_dict(state_dict)
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.steps_done = 0

    def _stats(self, mean, inv_std) -> tuple[torch.Tensor, torch.Tensor]:
        Cn = self.n_channels
        mean = torch.zeros(Cn) if mean is None else torch.as_tensor(mean).detach().float().reshape(-1)
        inv_std = torch.ones(Cn) if inv_std is None else torch.as_tensor(inv_std).detach().float().reshape(-1)
        if mean.shape[0] != Cn or inv_std.shape[0] != Cn:
            raise ValueError(f"mean and inv_std must hold one value per channel ({Cn})")
        return _on_device(mean, self.device), _on_device(inv_std, self.device)

    def fit(self, task: str, a, b=None, *, steps: int, batch_size: int, lr: float = 1e-3, mean=None, inv_std=None,
            max_norm: Optional[float] = None, trace_indices: bool = False, fused: bool = True, labels=None,
            balance: bool = False) -> torch.Tensor:
        """`steps` AdamW steps (constant lr, torch's defaults, optional global-norm clipping) on minibatches drawn with replacement
        from the pools: classify -- half of a batch from `a` (label 1), half from `b` (label 0); predict -- every row from `a`.  The
        pools are raw series; `mean` / `inv_std` (per channel) standardise them inside the gather kernel.  Returns the loss of every
        step, before its update: float32 (steps,) on the device.  A second call goes on where the first one stopped (optimiser
        state, step count and position in the index stream).  `fused=False` drives the same loop from Python, one engine call per
        stage: the same bits, for tests and timing.

        multiclass (a network built with `n_classes=K`) -- every row from the one pool `a` with its class from `labels` (integer,
        one per series, in [0, K)), and the softmax cross-entropy of the K logits.  `balance=True` draws class by class instead of
        row by row: the classes that hold a row take turns, so a rare class is seen as often as a common one."""
        steps, B = _count("steps", steps, 1), _count("batch_size", batch_size, 1)
        if not lr > 0:
            raise ValueError(f"lr={lr} must be positive")
        if task == "multiclass":
            return self._fit_multiclass(a, labels, bool(balance), steps, B, float(lr), mean, inv_std, max_norm, trace_indices, fused)
        code = _task(task)
        if labels is not None or balance:
            raise ValueError(f"labels and balance belong to the multiclass task, not to {task!r}")
        if self.n_classes is not None:
            raise ValueError(f"this network was built with n_classes={self.n_classes} for the multiclass task, not for {task!r}")
        shape = (self.max_len, self.n_channels)
        dev = self.device
        a = _on_device(_series(a, "a", shape), dev)
        if code == _C.FD_POSTHOC_CLASSIFY:
            if b is None:
                raise ValueError("the classify task draws from two pools: b is missing")
            if B % 2:
                raise ValueError(f"batch_size={B} must be even: the classify task takes half of a batch from each pool")
            b = _on_device(_series(b, "b", shape), dev)
        else:
            if self.max_len < 2:
                raise ValueError("the predict task regresses out[:, t] on x[:, t + 1] and needs series of at least 2 points")
            b = None
        mean_d, inv_d = self._stats(mean, inv_std)
        lib, m = _C.lib(), self.module
        ctx, h = m._engine()
        flat, stream = m.flat_parameters, _C.stream_of(m.flat_parameters)
        T, Cn = shape
        loss = torch.empty(steps, dtype=torch.float32, device=dev)
        idx = torch.empty((steps, B), dtype=torch.int32, device=dev) if trace_indices else None
        need = C.c_size_t(0)
        _C.check(lib.fd_posthoc_fit_workspace_bytes(ctx, B, T, Cn, C.byref(need)), ctx)
        clip = float(max_norm) if max_norm else 0.0
        na, nb = a.shape[0], (b.shape[0] if b is not None else 0)
        try:
            if fused:
                work = torch.empty(need.value, dtype=torch.uint8, device=dev)
                _C.check(lib.fd_posthoc_fit(h, code, flat.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(),
                                            self.exp_avg_sq.data_ptr(), a.data_ptr(), na, _C.ptr(b), nb, mean_d.data_ptr(),
                                            inv_d.data_ptr(), self.seed, 0, self.steps_done, steps, B, float(lr), clip,
                                            loss.data_ptr(), _C.ptr(idx), work.data_ptr(), need.value, stream), ctx)
            else:
                self._fit_stepwise(ctx, h, code, a, b, mean_d, inv_d, steps, B, float(lr), clip, loss, idx, stream)
        finally:
            m.mark_parameters_changed()
        self.steps_done += steps
        self.last_indices = idx
        return loss

    def _fit_stepwise(self, ctx, h, code, a, b, mean_d, inv_d, steps, B, lr, clip, loss, idx, stream) -> None:
        """fd_posthoc_fit's loop, one ctypes call per stage."""
        lib, m = _C.lib(), self.module
        T, Cn, dev = self.max_len, self.n_channels, self.device
        flat, n = m.flat_parameters, m.flat_parameters.numel()
        x = torch.empty((B, T, Cn), dtype=torch.float32, device=dev)
        out, dout = torch.empty_like(x), torch.empty_like(x)
        t0 = torch.zeros(B, dtype=torch.float32, device=dev)
        label = torch.empty(B, dtype=torch.int32, device=dev)
        idx_one = torch.empty(B, dtype=torch.int32, device=dev)
        per_series = torch.empty(B, dtype=torch.float64, device=dev)
        sqnorm = torch.zeros(1, dtype=torch.float32, device=dev)
        frozen = [(off, off + numel) for _, off, numel, _, tr in m._layout if not tr]
        fz0, fz1 = frozen[0] if frozen else (0, 0)
        na, nb = a.shape[0], (b.shape[0] if b is not None else 0)
        for k in range(steps):
            s = self.steps_done + k
            ik = idx[k] if idx is not None else idx_one
            _C.check(lib.fd_posthoc_batch(ctx, code, a.data_ptr(), na, _C.ptr(b), nb, mean_d.data_ptr(), inv_d.data_ptr(), self.seed,
                                          0, s, B, T, Cn, x.data_ptr(), label.data_ptr(), ik.data_ptr(), stream), ctx)
            _C.check(lib.fd_score_forward_train(h, x.data_ptr(), t0.data_ptr(), out.data_ptr(), B, 0.0, 0, 0, stream), ctx)
            _C.check(lib.fd_posthoc_head(ctx, code, out.data_ptr(), x.data_ptr(), label.data_ptr(), B, T, Cn, loss[k:].data_ptr(),
                                         dout.data_ptr(), per_series.data_ptr(), stream), ctx)
            _C.check(lib.fd_score_backward(h, dout.data_ptr(), self.grads.data_ptr(), 0, stream), ctx)
            if clip > 0:
                _C.check(lib.fd_grad_sqnorm(ctx, self.grads.data_ptr(), n, sqnorm.data_ptr(), stream), ctx)
            _C.check(lib.fd_adamw_step(ctx, flat.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                       n, s + 1, lr, 0.9, 0.999, 1e-8, 1e-2, sqnorm.data_ptr() if clip > 0 else None, clip, 1.0,
                                       fz0, fz1, stream), ctx)

    def _need_classes(self) -> int:
        if self.n_classes is None:
            raise ValueError("the multiclass task needs a network built with n_classes=K (K >= 2)")
        return self.n_classes

    def _fit_multiclass(self, a, labels, balance, steps, B, lr, mean, inv_std, max_norm, trace_indices, fused) -> torch.Tensor:
        K = self._need_classes()
        T, Cd, Cn = self.max_len, self.n_channels, self.net_channels
        a = _series(a, "a", (T, Cd))
        y = _labels(labels, a.shape[0], K)
        dev = self.device
        a = _on_device(a, dev)
        ya = torch.from_numpy(y.astype(np.int32)).to(dev)
        order = start = None
        if balance:
            # rows sorted stably by class, and where each class begins
            order = torch.from_numpy(np.argsort(y, kind="stable").astype(np.int32)).to(dev)
            start = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(y, minlength=K))]).astype(np.int32)).to(dev)
        mean_d, inv_d = self._stats(mean, inv_std)
        lib, m = _C.lib(), self.module
        ctx, h = m._engine()
        flat, stream = m.flat_parameters, _C.stream_of(m.flat_parameters)
        loss = torch.empty(steps, dtype=torch.float32, device=dev)
        idx = torch.empty((steps, B), dtype=torch.int32, device=dev) if trace_indices else None
        need = C.c_size_t(0)
        _C.check(lib.fd_posthoc_fit_multiclass_workspace_bytes(ctx, B, T, Cn, C.byref(need)), ctx)
        clip = float(max_norm) if max_norm else 0.0
        na = a.shape[0]
        try:
            if fused:
                work = torch.empty(need.value, dtype=torch.uint8, device=dev)
                _C.check(lib.fd_posthoc_fit_multiclass(h, K, flat.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(),
                                                       self.exp_avg_sq.data_ptr(), a.data_ptr(), na, ya.data_ptr(), _C.ptr(order),
                                                       _C.ptr(start), Cd, mean_d.data_ptr(), inv_d.data_ptr(), self.seed, 0,
                                                       self.steps_done, steps, B, lr, clip, loss.data_ptr(), _C.ptr(idx),
                                                       work.data_ptr(), need.value, stream), ctx)
            else:
                self._fit_multiclass_stepwise(ctx, h, K, a, ya, order, start, mean_d, inv_d, steps, B, lr, clip, loss, idx, stream)
        finally:
            m.mark_parameters_changed()
        self.steps_done += steps
        self.last_indices = idx
        return loss

    def _fit_multiclass_stepwise(self, ctx, h, K, a, ya, order, start, mean_d, inv_d, steps, B, lr, clip, loss, idx, stream) -> None:
        """fd_posthoc_fit_multiclass's loop, one ctypes call per stage."""
        lib, m = _C.lib(), self.module
        T, Cd, Cn, dev = self.max_len, self.n_channels, self.net_channels, self.device
        flat, n = m.flat_parameters, m.flat_parameters.numel()
        x = torch.empty((B, T, Cn), dtype=torch.float32, device=dev)
        out, dout = torch.empty_like(x), torch.empty_like(x)
        t0 = torch.zeros(B, dtype=torch.float32, device=dev)
        label = torch.empty(B, dtype=torch.int32, device=dev)
        idx_one = torch.empty(B, dtype=torch.int32, device=dev)
        nll = torch.empty(B, dtype=torch.float64, device=dev)
        sqnorm = torch.zeros(1, dtype=torch.float32, device=dev)
        frozen = [(off, off + numel) for _, off, numel, _, tr in m._layout if not tr]
        fz0, fz1 = frozen[0] if frozen else (0, 0)
        na = a.shape[0]
        for k in range(steps):
            s = self.steps_done + k
            ik = idx[k] if idx is not None else idx_one
            _C.check(lib.fd_posthoc_batch_labelled(ctx, a.data_ptr(), na, ya.data_ptr(), _C.ptr(order), _C.ptr(start), K,
                                                   mean_d.data_ptr(), inv_d.data_ptr(), self.seed, 0, s, B, T, Cd, Cn, x.data_ptr(),
                                                   label.data_ptr(), ik.data_ptr(), stream), ctx)
            _C.check(lib.fd_score_forward_train(h, x.data_ptr(), t0.data_ptr(), out.data_ptr(), B, 0.0, 0, 0, stream), ctx)
            _C.check(lib.fd_posthoc_head_multiclass(ctx, out.data_ptr(), label.data_ptr(), B, T, Cn, K, None, None, loss[k:].data_ptr(),
                                                    dout.data_ptr(), nll.data_ptr(), stream), ctx)
            _C.check(lib.fd_score_backward(h, dout.data_ptr(), self.grads.data_ptr(), 0, stream), ctx)
            if clip > 0:
                _C.check(lib.fd_grad_sqnorm(ctx, self.grads.data_ptr(), n, sqnorm.data_ptr(), stream), ctx)
            _C.check(lib.fd_adamw_step(ctx, flat.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                       n, s + 1, lr, 0.9, 0.999, 1e-8, 1e-2, sqnorm.data_ptr() if clip > 0 else None, clip, 1.0,
                                       fz0, fz1, stream), ctx)

    def _evaluate_multiclass(self, x, labels) -> tuple[torch.Tensor, torch.Tensor]:
        K = self._need_classes()
        T, Cd, Cn, dev = self.max_len, self.n_channels, self.net_channels, self.device
        x = _on_device(_series(x, "x", (T, Cd)), dev)
        n = x.shape[0]
        if labels is not None:
            _labels(labels, n, K)
        lib, m = _C.lib(), self.module
        ctx, h = m._engine()
        stream = _C.stream_of(x)
        logp = torch.empty((n, K), dtype=torch.float64, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev)
        chunk = min(n, EVAL_CHUNK)
        xs = torch.zeros((chunk, T, Cn), dtype=torch.float32, device=dev)      # the channels >= C stay +0.0
        out = torch.empty((chunk, T, Cn), dtype=torch.float32, device=dev)
        t0 = torch.zeros(chunk, dtype=torch.float32, device=dev)
        for lo in range(0, n, chunk):
            rows = min(chunk, n - lo)
            xs[:rows, :, :Cd] = x[lo:lo + rows]
            _C.check(lib.fd_score_forward(h, xs.data_ptr(), t0.data_ptr(), out.data_ptr(), rows, _C.FD_MODE_F32, stream), ctx)
            _C.check(lib.fd_posthoc_head_multiclass(ctx, out.data_ptr(), None, rows, T, Cn, K, logp[lo:].data_ptr(),
                                                    pred[lo:].data_ptr(), None, None, None, stream), ctx)
        return logp, pred

    def evaluate(self, task: str, x, labels=None):
        """Per series of x (n, T, C), which is already standardised: the logit (classify) or the sum over t < T - 1 and channels of
        |out[t] - x[t + 1]| (predict), float64 (n,) on the device.  Neither needs `labels`; when given they are only checked for
        their length.  multiclass: (logp (n, K) float64, the log-softmax of the K logits, pred (n,) int32, their argmax with ties
        to the lowest class), both on the device; the channels are padded here; `labels`, when given, are only checked."""
        if task == "multiclass":
            return self._evaluate_multiclass(x, labels)
        code = _task(task)
        if self.n_classes is not None:
            raise ValueError(f"this network was built with n_classes={self.n_classes} for the multiclass task, not for {task!r}")
        shape = (self.max_len, self.n_channels)
        dev = self.device
        x = _on_device(_series(x, "x", shape), dev)
        n = x.shape[0]
        if labels is not None and len(labels) != n:
            raise ValueError(f"{len(labels)} labels for {n} series")
        if code == _C.FD_POSTHOC_PREDICT and self.max_len < 2:
            raise ValueError("the predict task needs series of at least 2 points")
        lib, m = _C.lib(), self.module
        ctx, h = m._engine()
        stream = _C.stream_of(x)
        T, Cn = shape
        per_series = torch.empty(n, dtype=torch.float64, device=dev)
        chunk = min(n, EVAL_CHUNK)
        out = torch.empty((chunk, T, Cn), dtype=torch.float32, device=dev)
        t0 = torch.zeros(chunk, dtype=torch.float32, device=dev)
        for lo in range(0, n, chunk):
            rows = min(chunk, n - lo)
            xs = x[lo:lo + rows]
            _C.check(lib.fd_score_forward(h, xs.data_ptr(), t0.data_ptr(), out.data_ptr(), rows, _C.FD_MODE_F32, stream), ctx)
            _C.check(lib.fd_posthoc_head(ctx, code, out.data_ptr(), xs.data_ptr(), None, rows, T, Cn, None, None,
                                         per_series[lo:].data_ptr(), stream), ctx)
        return per_series


def _subsample(n: int, size: int, rng: np.random.Generator) -> np.ndarray:
    return rng.permutation(n)[:size]


def discriminative_score(real, generated, *, seed: int, steps: int = 2000, batch_size: int = 128, lr: float = 1e-3, d_model: int = 32,
                         num_layers: int = 1, test_fraction: float = 0.2, max_samples: int = 10_000) -> dict:
    """Can a classifier trained after the fact tell `generated` from `real` (both (n, T, C))?  Both sets are standardised per channel
    with the real set's mean and deviation, cut to a common size n <= max_samples and split into train and test rows by a seeded
    permutation; the network is fitted on the train rows and scored on the test rows.  Returns accuracy, score = |accuracy - 0.5|,
    accuracy_real and accuracy_generated (the accuracy on each class), loss_trace, n_train and n_test."""
    real = _series(real, "real")
    generated = _series(generated, "generated", tuple(real.shape[1:]))
    if not 0.0 < test_fraction < 1.0:
        raise ValueError(f"test_fraction={test_fraction} must lie strictly between 0 and 1")
    n = min(real.shape[0], generated.shape[0], _count("max_samples", max_samples, 2))
    if n < 2:
        raise ValueError("the discriminative score needs at least 2 series in each set (one to train on, one to test on)")
    n_test = min(n - 1, max(1, int(round(n * test_fraction))))
    rng = np.random.default_rng(seed)
    mean, inv_std = channel_stats(real)
    net = PosthocNetwork(real.shape[2], real.shape[1], d_model=d_model, num_layers=num_layers, seed=seed)
    dev = net.device
    rows_r, rows_g = _subsample(real.shape[0], n, rng), _subsample(generated.shape[0], n, rng)
    real_d = _on_device(real, dev)[torch.from_numpy(rows_r).to(dev)]
    gen_d = _on_device(generated, dev)[torch.from_numpy(rows_g).to(dev)]
    trace = net.fit("classify", real_d[n_test:], gen_d[n_test:], steps=steps, batch_size=batch_size, lr=lr, mean=mean, inv_std=inv_std)
    logit_r = net.evaluate("classify", standardise(real_d[:n_test], mean, inv_std))
    logit_g = net.evaluate("classify", standardise(gen_d[:n_test], mean, inv_std))
    acc_r, acc_g = float((logit_r > 0).double().mean()), float((logit_g <= 0).double().mean())
    acc = 0.5 * (acc_r + acc_g)
    return {"accuracy": acc, "score": abs(acc - 0.5), "accuracy_real": acc_r, "accuracy_generated": acc_g,
            "loss_trace": trace.cpu().tolist(), "n_train": n - n_test, "n_test": n_test}


def predictive_score(train_set, test_set, *, stats_from, seed: int, steps: int = 2000, batch_size: int = 128, lr: float = 1e-3,
                     d_model: int = 32, num_layers: int = 1, max_samples: int = 10_000) -> dict:
    """Train a next-step forecaster on `train_set`, test it on `test_set` (both (n, T, C), T >= 2): `mae`, the mean absolute one-step
    error over the test set in units of the per-channel deviation of `stats_from` (the real set), plus loss_trace.  Each set is cut
    to at most max_samples series by a seeded permutation."""
    train_set = _series(train_set, "train_set")
    test_set = _series(test_set, "test_set", tuple(train_set.shape[1:]))
    T, Cn = train_set.shape[1], train_set.shape[2]
    if T < 2:
        raise ValueError("the predictive score forecasts x[t + 1] from x[<= t] and needs series of at least 2 points")
    max_samples = _count("max_samples", max_samples, 1)
    rng = np.random.default_rng(seed)
    mean, inv_std = channel_stats(_series(stats_from, "stats_from", (T, Cn)))
    net = PosthocNetwork(Cn, T, d_model=d_model, num_layers=num_layers, seed=seed)
    dev = net.device
    rows_a = _subsample(train_set.shape[0], min(train_set.shape[0], max_samples), rng)
    rows_t = _subsample(test_set.shape[0], min(test_set.shape[0], max_samples), rng)
    train_d = _on_device(train_set, dev)[torch.from_numpy(rows_a).to(dev)]
    test_d = _on_device(test_set, dev)[torch.from_numpy(rows_t).to(dev)]
    trace = net.fit("predict", train_d, steps=steps, batch_size=batch_size, lr=lr, mean=mean, inv_std=inv_std)
    errors = net.evaluate("predict", standardise(test_d, mean, inv_std))
    mae = float(errors.sum()) / (test_d.shape[0] * (T - 1) * Cn)
    return {"mae": mae, "loss_trace": trace.cpu().tolist(), "n_train": int(train_d.shape[0]), "n_test": int(test_d.shape[0])}


def confusion_matrix(labels: torch.Tensor, pred: torch.Tensor, n_classes: int) -> torch.Tensor:
    """counts (K, K) int32 on the device of labels (n,) and pred (n,) int32 device tensors: rows are the true class
    (`fd_posthoc_confusion`)."""
    K = _n_classes(n_classes)
    labels, pred = labels.contiguous(), pred.contiguous()
    if labels.dtype != torch.int32 or pred.dtype != torch.int32 or labels.shape != pred.shape or labels.dim() != 1 or len(labels) < 1:
        raise ValueError("labels and pred must be int32 vectors of one non-zero length")
    counts = torch.empty((K, K), dtype=torch.int32, device=labels.device)
    lib, ctx = _C.lib(), _C.ctx(labels.device)
    _C.check(lib.fd_posthoc_confusion(ctx, labels.data_ptr(), pred.data_ptr(), labels.shape[0], K, counts.data_ptr(),
                                      _C.stream_of(labels)), ctx)
    return counts


def scores_from_confusion(confusion: np.ndarray) -> dict:
    """accuracy, balanced_accuracy (the mean recall over the classes present in the test set), macro_f1 (the mean F1 over the same
    classes) and per_class_recall (NaN for an absent class) of a (K, K) confusion matrix whose rows are the true class."""
    cm = np.asarray(confusion, dtype=np.float64)
    support, predicted, hit = cm.sum(axis=1), cm.sum(axis=0), np.diag(cm)
    present = support > 0
    recall = np.where(present, hit / np.where(present, support, 1.0), np.nan)
    f1 = 2.0 * hit / np.where(support + predicted > 0, support + predicted, 1.0)
    return {"accuracy": float(hit.sum() / cm.sum()), "balanced_accuracy": float(recall[present].mean()),
            "macro_f1": float(f1[present].mean()), "per_class_recall": [float(v) for v in recall]}


class Classifier:
    """A fitted K-way post-hoc classifier with the statistics it standardises by: `fit_classifier` makes one, `score` tests it on a
    labelled set.  (TRTS trains one on the real set and scores every batch of samples with it.)"""

    def __init__(self, net: PosthocNetwork, mean: torch.Tensor, inv_std: torch.Tensor, loss_trace: list, n_train: int, seed: int,
                 max_samples: int) -> None:
        self.net, self.mean, self.inv_std, self.loss_trace, self.n_train = net, mean, inv_std, loss_trace, n_train
        self.seed, self.max_samples = seed, max_samples

    def score(self, test_set, test_labels) -> dict:
        net, K = self.net, self.net.n_classes
        test_set = _series(test_set, "test_set", (net.max_len, net.n_channels))
        y = _labels(test_labels, test_set.shape[0], K, "test_labels")
        # a stream of its own, so that the cut does not depend on how many sets the classifier has scored before
        rows = _subsample(test_set.shape[0], min(test_set.shape[0], self.max_samples), np.random.default_rng([self.seed, 1]))
        dev = net.device
        test_d = _on_device(test_set, dev)[torch.from_numpy(rows).to(dev)]
        y_d = torch.from_numpy(y[rows].astype(np.int32)).to(dev)
        logp, pred = net.evaluate("multiclass", standardise(test_d, self.mean, self.inv_std))
        confusion = confusion_matrix(y_d, pred, K).cpu().numpy()
        nll = float(-logp.gather(1, y_d.long()[:, None]).sum()) / len(rows)
        return dict(scores_from_confusion(confusion), nll=nll, confusion=confusion.tolist(), loss_trace=list(self.loss_trace),
                    n_train=self.n_train, n_test=int(len(rows)))


def fit_classifier(train_set, train_labels, *, n_classes: int, stats_from, seed: int, steps: int = 2000, batch_size: int = 128,
                   lr: float = 1e-3, d_model: int = 32, num_layers: int = 1, balance: bool = False,
                   max_samples: int = 10_000) -> Classifier:
    """Train the K-way classifier on `train_set` (n, T, C) with `train_labels` (n,), standardised per channel by the statistics of
    `stats_from`; the set is cut to at most max_samples series by a seeded permutation."""
    K = _n_classes(n_classes)
    train_set = _series(train_set, "train_set")
    T, Cn = train_set.shape[1], train_set.shape[2]
    y = _labels(train_labels, train_set.shape[0], K, "train_labels")
    max_samples = _count("max_samples", max_samples, 1)
    mean, inv_std = channel_stats(_series(stats_from, "stats_from", (T, Cn)))
    rows = _subsample(train_set.shape[0], min(train_set.shape[0], max_samples), np.random.default_rng(seed))
    net = PosthocNetwork(Cn, T, d_model=d_model, num_layers=num_layers, seed=seed, n_classes=K)
    dev = net.device
    train_d = _on_device(train_set, dev)[torch.from_numpy(rows).to(dev)]
    trace = net.fit("multiclass", train_d, labels=y[rows], balance=balance, steps=steps, batch_size=batch_size, lr=lr, mean=mean,
                    inv_std=inv_std)
    return Classifier(net, mean, inv_std, trace.cpu().tolist(), int(train_d.shape[0]), seed, max_samples)


def classification_score(train_set, train_labels, test_set, test_labels, *, n_classes: int, stats_from, seed: int, steps: int = 2000,
                         batch_size: int = 128, lr: float = 1e-3, d_model: int = 32, num_layers: int = 1, balance: bool = False,
                         max_samples: int = 10_000) -> dict:
    """Train a K-way classifier on one labelled set, test it on another (both (n, T, C) with integer labels in [0, K)): train on the
    samples with the classes they were drawn for and test on real series (TSTR), the reverse (TRTS), or two real folds (TRTR).
    Returns accuracy, balanced_accuracy (the mean recall over the classes present in the test set), macro_f1, nll (the mean
    negative log-likelihood of the true class), per_class_recall, confusion (K x K, rows the true class), loss_trace, n_train and
    n_test.  Both sets are standardised by the statistics of `stats_from` (the real set) and cut to at most max_samples series by a
    seeded permutation."""
    test_set = _series(test_set, "test_set", tuple(_series(train_set, "train_set").shape[1:]))
    _labels(test_labels, test_set.shape[0], _n_classes(n_classes), "test_labels")
    clf = fit_classifier(train_set, train_labels, n_classes=n_classes, stats_from=stats_from, seed=seed, steps=steps,
                         batch_size=batch_size, lr=lr, d_model=d_model, num_layers=num_layers, balance=balance, max_samples=max_samples)
    return clf.score(test_set, test_labels)
