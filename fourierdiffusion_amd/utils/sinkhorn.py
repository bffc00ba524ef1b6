"""Entropic optimal transport between two sample sets on the HIP engine (not in the reference; Genevay et al. 2018, Feydy et al.
2019): the debiased Sinkhorn divergence

    S_eps(X, Y) = OT_eps(X, Y) - OT_eps(X, X) / 2 - OT_eps(Y, Y) / 2,    cost ||x - y||^2,

the usual estimate of the squared Wasserstein-2 distance of the two sets in their full sample space -- the quantity the sliced
metric stands in for.  It is >= 0, zero only for equal sets, tends to W2^2 as eps -> 0 and to an MMD as eps -> inf.

``softmin_pairs`` is fd_softmin_pairs (csrc/fd_sinkhorn.hip): one log-sum-exp over all pairs in one fused fp32-MFMA kernel, the
(n, m) matrix never exists.  ``sinkhorn_potentials`` is fd_sinkhorn_potentials: the whole iteration enqueued on the stream.
Everything after them is float64 host arithmetic.  Deterministic: the engine uses no atomics.

The schedule (``epsilon_schedule``) is eps-scaling: eps descends geometrically by scaling^2 from `start` to `reg`, then stays at
`reg` for `n_final` iterations; all in units of eps_base, the mean squared distance over the pooled pairs.  The defaults come from
a convergence study with the float64 reference on noisy sine waves (n, m in 200..400, 24..187 features): the pair distances reach
about 4 eps_base, so start = 4 puts the first iterations at the scale of the squared diameter, where one iteration converges; at
reg = 0.05 and scaling = 0.5 the divergence moves by less than 1e-3 of its value beyond n_final = 20 and the marginal error is
below 1e-2 (DESIGN.md 3.28 has the table).  ``SinkhornResult.marginal_error`` says whether that was enough for the data at hand."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _C
from ._pairs import call_with_workspace, same_pair
from .neighbours import _rows_features

MAX_STEPS = 256
DEFAULT_REG = 0.05


@dataclass
class SinkhornResult:
    divergence: float            # <a, f - p_x> + <b, g - p_y>
    w2: float                    # sqrt(max(divergence, 0))
    ot_xy: float                 # <a, f> + <b, g>: the entropic transport cost of x against y
    eps: float                   # the final eps, in the units of the squared distances
    marginal_error: float        # sum_i a_i |exp((f_i - softmin_Y(g)_i) / eps) - 1|: 0 at convergence
    cost_x: np.ndarray           # (n,) f - p_x: what every row of x pays
    cost_y: np.ndarray           # (m,) g - p_y


def _check_positive(name: str, value, what: str = "") -> float:
    v = float(value)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"{name}={value} must be finite and > 0{what}")
    return v


def _check_pair(x, y) -> tuple[int, int, int]:
    (n, dx), (m, dy) = _rows_features(x), _rows_features(y)
    if dx != dy:
        raise ValueError(f"x has {dx} features and y {dy}")
    if n * dx >= 2 ** 31 or m * dx >= 2 ** 31:
        raise ValueError(f"too large: n * d = {n * dx} and m * d = {m * dx} must stay below 2^31")
    return n, m, dx


def _check_weights(name: str, w, rows: int) -> Optional[np.ndarray]:
    if w is None:
        return None
    if isinstance(w, torch.Tensor):
        w = w.detach().cpu().numpy()
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.shape[0] != rows:
        raise ValueError(f"{name} has {w.shape[0]} entries for {rows} rows")
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError(f"{name} must be finite and > 0")
    if abs(w.sum() - 1.0) > 1e-9:
        raise ValueError(f"{name} must sum to 1, got {w.sum()}")
    return w


def epsilon_schedule(reg: float, scaling: float = 0.5, n_final: int = 20, start: float = 4.0) -> np.ndarray:
    """The eps of every iteration, in units of eps_base: start, start scaling^2, start scaling^4, ... while above reg, then reg
    n_final times."""
    reg, start = _check_positive("reg", reg), _check_positive("start", start)
    scaling = float(scaling)
    if not 0.0 < scaling < 1.0:
        raise ValueError(f"scaling={scaling} must lie in (0, 1)")
    if isinstance(n_final, bool) or int(n_final) != n_final or n_final < 1:
        raise ValueError(f"n_final={n_final} must be an integer >= 1")
    out = []
    eps = start
    while eps > reg:
        out.append(eps)
        eps *= scaling * scaling
    out.extend([reg] * int(n_final))
    if len(out) > MAX_STEPS:
        raise ValueError(f"{len(out)} iterations: at most {MAX_STEPS}")
    return np.asarray(out, dtype=np.float64)


def _check_schedule(schedule) -> np.ndarray:
    try:
        out = np.asarray([float(e) for e in schedule], dtype=np.float64)
    except TypeError:
        raise ValueError(f"schedule must be a sequence of numbers, got {schedule!r}") from None
    if not 1 <= len(out) <= MAX_STEPS:
        raise ValueError(f"schedule has {len(out)} iterations: between 1 and {MAX_STEPS} are supported")
    if not (np.isfinite(out).all() and (out > 0).all()):
        raise ValueError("schedule must be finite and > 0")
    return out


def _resolve_schedule(reg, epsilon, schedule) -> tuple[np.ndarray, bool]:
    """(the eps of every iteration, whether they are absolute): an absolute final `epsilon` rescales the schedule to end there."""
    sched = epsilon_schedule(reg) if schedule is None else _check_schedule(schedule)
    if epsilon is None:
        return sched, False
    return sched * (_check_positive("epsilon", epsilon, " (None: reg times the pooled mean squared pair distance)") / sched[-1]), True


def softmin_pairs(x, y, h, eps: float, splits: int = 0) -> torch.Tensor:
    """(n,) float64 on the device: out_i = -eps log sum_j exp((h_j - ||x_i - y_j||^2) / eps) for the rows x (n, ...) and y (m, ...)
    and the offsets h (m,).  splits: 0 = automatic; the result is the same for every value."""
    n, m, d = _check_pair(x, y)
    eps = _check_positive("eps", eps)
    if isinstance(splits, bool) or int(splits) != splits or splits < 0:
        raise ValueError(f"splits={splits} must be an integer >= 0")
    hshape = tuple(h.shape)
    if hshape != (m,):
        raise ValueError(f"h has shape {hshape}, expected ({m},)")
    xt, yt = same_pair(x, y)
    if isinstance(h, np.ndarray):
        h = torch.from_numpy(np.ascontiguousarray(h))
    ht = h.detach().to(device=xt.device, dtype=torch.float64).contiguous()
    L = _C.lib()
    out = torch.empty((n,), dtype=torch.float64, device=xt.device)
    same = 1 if xt is yt else 0
    call_with_workspace(xt, L.fd_softmin_pairs_workspace_bytes, (n, m, d, same, int(splits)), lambda hd, work, nbytes, stream:
                        L.fd_softmin_pairs(hd, xt.data_ptr(), n, yt.data_ptr(), m, d, ht.data_ptr(), eps, int(splits), out.data_ptr(),
                                           work, nbytes, stream))
    return out


def sinkhorn_potentials(x, y, reg: float = DEFAULT_REG, epsilon: Optional[float] = None, schedule: Optional[Sequence[float]] = None,
                        weights_x=None, weights_y=None) -> tuple[torch.Tensor, torch.Tensor, float]:
    """(f (n,), g (m,), eps): the dual potentials of the entropic transport of x (n, ...) against y (m, ...) as float64 device
    tensors, and the final eps in the units of the squared distances.  Passing the same object twice runs the symmetric iteration
    p <- (p + softmin(p)) / 2 and returns f = g = p.
      schedule   the eps of every iteration (None: epsilon_schedule(reg)), in units of eps_base, the mean squared distance over
                 the pooled pairs
      epsilon    an absolute final eps: the schedule is rescaled so that it ends there (schedule * epsilon / schedule[-1], in the
                 units of the squared distances); reg is then not used
      weights    positive and summing to 1; None: uniform"""
    n, m, d = _check_pair(x, y)
    sched, absolute = _resolve_schedule(reg, epsilon, schedule)
    a, b = _check_weights("weights_x", weights_x, n), _check_weights("weights_y", weights_y, m)
    symmetric = x is y
    if symmetric and b is not None and (a is None or not np.array_equal(a, b)):
        raise ValueError("one set against itself takes one weight vector: pass weights_x (and nothing else or the same as weights_y)")
    xt, yt = same_pair(x, y)
    at = None if a is None else torch.from_numpy(a).to(xt.device)
    bt = None if b is None or symmetric else torch.from_numpy(b).to(xt.device)
    L = _C.lib()
    f = torch.empty((n,), dtype=torch.float64, device=xt.device)
    g = torch.empty((m,), dtype=torch.float64, device=xt.device)
    base = torch.empty((1,), dtype=torch.float64, device=xt.device)
    ce = (C.c_double * len(sched))(*sched)
    call_with_workspace(xt, L.fd_sinkhorn_potentials_workspace_bytes, (n, m, d, 1 if symmetric else 0), lambda hd, work, nbytes, stream:
                        L.fd_sinkhorn_potentials(hd, xt.data_ptr(), n, yt.data_ptr(), m, d, 1 if symmetric else 0, _C.ptr(at), _C.ptr(bt),
                                                 ce, len(sched), 1 if absolute else 0, f.data_ptr(), g.data_ptr(), base.data_ptr(),
                                                 work, nbytes, stream))
    return f, g, float(sched[-1]) * (1.0 if absolute else float(base.item()))


def sinkhorn_divergence(x, y, reg: float = DEFAULT_REG, epsilon: Optional[float] = None, schedule: Optional[Sequence[float]] = None,
                        weights_x=None, weights_y=None) -> SinkhornResult:
    """The debiased Sinkhorn divergence of x (n, ...) against y (m, ...): three runs of the iteration -- x against y, whose eps
    (from the pooled rows of both sets) the other two take over, x against itself and y against itself -- and one more soft-min pass
    for the marginal error.  One object passed twice (with one weight vector) is one symmetric run: every potential is p, the
    divergence is exactly 0.  cost_x and cost_y carry the constant that (f + c, g - c) leaves free; the divergence does not."""
    n, m, _ = _check_pair(x, y)
    _resolve_schedule(reg, epsilon, schedule)
    a, b = _check_weights("weights_x", weights_x, n), _check_weights("weights_y", weights_y, m)
    one_set = x is y and (b is None or (a is not None and np.array_equal(a, b)))
    xt, yt = same_pair(x, y)
    if one_set:
        b = a
        f, _, eps = sinkhorn_potentials(xt, xt, reg=reg, epsilon=epsilon, schedule=schedule, weights_x=a)
        g = px = py = f
    else:
        if yt is xt:
            yt = xt.clone()                                       # two weight vectors on one set: the alternating iteration
        f, g, eps = sinkhorn_potentials(xt, yt, reg=reg, epsilon=epsilon, schedule=schedule, weights_x=a, weights_y=b)
        px, _, _ = sinkhorn_potentials(xt, xt, reg=reg, epsilon=eps, schedule=schedule, weights_x=a)
        py, _, _ = sinkhorn_potentials(yt, yt, reg=reg, epsilon=eps, schedule=schedule, weights_x=b)
    a = np.full(n, 1.0 / n) if a is None else a
    b = np.full(m, 1.0 / m) if b is None else b
    again = softmin_pairs(xt, yt, g + eps * torch.from_numpy(np.log(b)).to(g.device), eps).cpu().numpy()
    f, g, px, py = f.cpu().numpy(), g.cpu().numpy(), px.cpu().numpy(), py.cpu().numpy()
    cost_x, cost_y = f - px, g - py
    div = float(a @ cost_x + b @ cost_y)
    return SinkhornResult(divergence=div, w2=float(np.sqrt(max(div, 0.0))), ot_xy=float(a @ f + b @ g), eps=eps,
                          marginal_error=float((a * np.abs(np.exp((f - again) / eps) - 1.0)).sum()), cost_x=cost_x, cost_y=cost_y)
