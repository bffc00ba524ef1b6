"""Observation masks and observation operators of conditional sampling (an extension: not in the reference).  Pure functions on
the CPU: True = observed, False = hidden (what the sampler fills in).  ``LinearOperator`` and its constructors describe what is
observed when it is not single entries: y = P x for a fixed matrix P (``DiffusionSampler.impute(operator=...)``)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch


def observation_mask(kind: str, shape: Tuple[int, int, int], p: float = 0.5, horizon: int = 1,
                     generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """A bool mask of `shape` (n, T, C).

    kind "random":   every entry is hidden independently with probability `p` (0 <= p <= 1);
    kind "forecast": the last `horizon` time steps of every series are hidden (1 <= horizon <= T), all channels."""
    n, T, C = (int(v) for v in shape)
    if kind == "random":
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"mask.p must lie in [0, 1], got {p}")
        return torch.rand((n, T, C), generator=generator) >= float(p)
    if kind == "forecast":
        if not 1 <= int(horizon) <= T:
            raise ValueError(f"mask.horizon must lie in [1, {T}], got {horizon}")
        mask = torch.ones((n, T, C), dtype=torch.bool)
        mask[:, T - int(horizon):, :] = False
        return mask
    raise ValueError(f"unknown mask kind {kind!r} (random | forecast)")


def window_means(X: torch.Tensor, w: int) -> torch.Tensor:
    """The means of X (..., T, C) over consecutive windows of w time steps: (..., J, C), J = ceil(T / w); window j covers
    [j w, min((j + 1) w, T)), so the last one may be shorter.  What ``DiffusionSampler.impute(aggregate=w)`` observes."""
    if isinstance(w, bool) or not isinstance(w, int) or w < 1:
        raise ValueError(f"window_means: w must be an int >= 1, got {w!r}")
    if not isinstance(X, torch.Tensor) or X.dim() < 2 or not X.is_floating_point():
        raise ValueError("window_means: X must be a floating-point tensor (..., T, C)")
    T = int(X.shape[-2])
    if w > T:
        raise ValueError(f"window_means: w={w} exceeds T={T}")
    return torch.stack([X[..., lo:min(lo + w, T), :].mean(dim=-2) for lo in range(0, T, w)], dim=-2)


def lift_windows(Y: torch.Tensor, w: int, T: int) -> torch.Tensor:
    """The piecewise-constant lift of window values Y (..., J, C), J = ceil(T / w), to (..., T, C): entry t takes the value of
    its window t // w.  ``window_means(lift_windows(Y, w, T), w)`` is Y.  Works on bool masks as well."""
    for name, v in (("w", w), ("T", T)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"lift_windows: {name} must be an int >= 1, got {v!r}")
    if w > T:
        raise ValueError(f"lift_windows: w={w} exceeds T={T}")
    J = (T + w - 1) // w
    if not isinstance(Y, torch.Tensor) or Y.dim() < 2 or int(Y.shape[-2]) != J:
        raise ValueError(f"lift_windows: Y must be a tensor (..., {J}, C) for w={w}, T={T}")
    return Y.repeat_interleave(w, dim=-2)[..., :T, :]


# ------------------------------------------------------------------ dense linear observation operators (DiffusionSampler.impute(operator=...))
def _as_matrix(P, who: str) -> np.ndarray:
    if isinstance(P, torch.Tensor):
        P = P.detach().cpu().numpy()
    P = np.array(P, dtype=np.float64)
    if P.ndim != 2 or P.shape[0] < 1 or not np.isfinite(P).all():
        raise ValueError(f"{who}: P must be a finite (M, T) matrix, got shape {P.shape}")
    return np.ascontiguousarray(P)


class LinearOperator:
    """A fixed linear observation y = P v per channel, P (M, T), shared by all series and channels: what
    ``DiffusionSampler.impute(operator=...)`` conditions on.  T is the model's max_len, 1 <= M <= T <= 1024, and P must have full
    row rank.  Holds P and P^+ = pinv(P) (float64, so P P^+ = I), M, T, ``condition`` = cond(P) and ``rows_orthogonal`` (P P^T
    diagonal, off-diagonal entries at most 1e-10 of the largest diagonal one): only then is P^+ diag(m) the pseudo-inverse of
    diag(m) P, i.e. only then may replacement conditioning mask single rows.

    ValueError when rank(P) < M or cond(P) > max_condition (default 1e4; raise it per operator if you accept the loss): the
    engine's f32 bases lose about cond(P) 2^-24 relative accuracy.  The engine handle (fd_linop_create) is created on first use
    per context and freed with the object."""

    def __init__(self, P, max_condition: float = 1e4) -> None:
        P = _as_matrix(P, "LinearOperator")
        M, T = P.shape
        if not 1 <= M <= T <= 1024:
            raise ValueError(f"LinearOperator: P is ({M}, {T}), need 1 <= M <= T <= 1024")
        if isinstance(max_condition, bool) or not isinstance(max_condition, (int, float)) or not max_condition >= 1:
            raise ValueError(f"LinearOperator: max_condition must be a number >= 1, got {max_condition!r}")
        U, sv, Vt = np.linalg.svd(P, full_matrices=False)
        rank = int((sv > T * np.finfo(np.float64).eps * sv[0]).sum()) if sv[0] > 0 else 0
        if rank < M:
            raise ValueError(f"LinearOperator: P ({M}, {T}) has rank {rank} < M = {M}: its rows must be linearly independent")
        cond = float(sv[0] / sv[-1])
        if cond > max_condition:
            raise ValueError(f"LinearOperator: cond(P) = {cond:.3g} exceeds max_condition = {max_condition:g}; the engine's f32 bases "
                             f"lose about cond(P) 2^-24 = {cond * 2.0 ** -24:.1e} relative accuracy (raise max_condition to accept it)")
        self.P = P
        self.P_pinv = np.ascontiguousarray((Vt.T / sv) @ U.T)           # pinv(P) from the same decomposition (full row rank)
        self.M, self.T, self.condition, self.max_condition = M, T, cond, float(max_condition)
        gram = P @ P.T
        diag = np.diag(gram)
        self.rows_orthogonal = bool(np.abs(gram - np.diag(diag)).max() <= 1e-10 * diag.max())
        self._handles: dict = {}

    def check_row_mask(self, mask: torch.Tensor, who: str) -> None:
        """The rule of replacement conditioning: a mask over rows (..., M, C) may hide single rows only when the rows of P are
        mutually orthogonal; otherwise every (series, channel) column must be all True or all False (ValueError)."""
        if self.rows_orthogonal:
            return
        m = mask.bool()
        if not bool((m.all(dim=-2) | ~m.any(dim=-2)).all()):
            raise ValueError(f"{who}: conditioning='replace' with an operator whose rows are not mutually orthogonal (P P^T is not "
                             "diagonal) takes only masks whose (series, channel) columns are all True or all False: P^+ diag(m) is not "
                             "the pseudo-inverse of diag(m) P, so the update would not be the orthogonal projection onto the kept "
                             "rows' observations (it would also pin P x on the hidden rows).  Use conditioning='dps', or build the "
                             "operator from the observed rows alone")

    def handle(self, ctx):
        """The engine's fd_linop of this operator on the context `ctx` (``_C.ctx(device)``), created on first use."""
        from .. import _C
        key = int(ctx.value)
        if key not in self._handles:
            h = _C._vp()
            rc = _C.lib().fd_linop_create(ctx, self.T, self.M, self.P.ctypes.data, self.P_pinv.ctypes.data, C.byref(h))
            _C.check(rc, ctx)
            self._handles[key] = h
        return self._handles[key]

    def close(self) -> None:
        """Frees the engine handles (also on garbage collection); the operator can be used again afterwards."""
        handles, self._handles = getattr(self, "_handles", {}), {}
        for h in handles.values():
            try:
                from .. import _C
                _C.lib().fd_linop_destroy(h)
            except Exception:      # interpreter shutdown: the library may be gone already
                pass

    def __del__(self) -> None:
        self.close()


def as_operator(operator, max_condition: float = 1e4) -> LinearOperator:
    """``operator`` itself when it is a LinearOperator, else the LinearOperator of an (M, T) array or tensor."""
    return operator if isinstance(operator, LinearOperator) else LinearOperator(operator, max_condition)


def _matrix_of(P) -> np.ndarray:
    return P.P if isinstance(P, LinearOperator) else _as_matrix(P, "operator")


def apply_operator(x: torch.Tensor, P) -> torch.Tensor:
    """y = P x along the time axis: x (..., T, C) -> (..., M, C), in float64.  P: a LinearOperator or an (M, T) array / tensor."""
    Pm = torch.from_numpy(_matrix_of(P))
    if not isinstance(x, torch.Tensor) or x.dim() < 2 or int(x.shape[-2]) != Pm.shape[1]:
        raise ValueError(f"apply_operator: x must be a tensor (..., {Pm.shape[1]}, C)")
    return torch.einsum("mt,...tc->...mc", Pm, x.double().cpu())


def lift_operator(y: torch.Tensor, P) -> torch.Tensor:
    """The minimum-norm lift P^+ y along the row axis: y (..., M, C) -> (..., T, C), in float64; ``apply_operator(lift_operator(y,
    P), P)`` is y for a P of full row rank."""
    Pp = torch.from_numpy(P.P_pinv if isinstance(P, LinearOperator) else np.linalg.pinv(_as_matrix(P, "operator")))
    if not isinstance(y, torch.Tensor) or y.dim() < 2 or int(y.shape[-2]) != Pp.shape[1]:
        raise ValueError(f"lift_operator: y must be a tensor (..., {Pp.shape[1]}, C)")
    return torch.einsum("tm,...mc->...tc", Pp, y.double().cpu())


def _int_in(name: str, v, lo: int, hi: int, who: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{who}: {name} must be an int in [{lo}, {hi}], got {v!r}")
    return v


def lowpass_operator(T: int, n_freq: int) -> np.ndarray:
    """A band-limited recording: the DC row and the cos / sin pairs of bins 1 .. n_freq - 1 of the orthonormal real Fourier basis,
    (M, T) with M = 2 n_freq - 1 (one row less when the last bin is the Nyquist bin of an even T).  The rows are orthonormal, so
    row masks are allowed under replacement.  1 <= n_freq <= T // 2 + 1."""
    _int_in("T", T, 1, 1024, "lowpass_operator")
    _int_in("n_freq", n_freq, 1, T // 2 + 1, "lowpass_operator")
    t = np.arange(T, dtype=np.float64)
    rows = [np.full(T, 1.0 / np.sqrt(T))]
    for k in range(1, n_freq):
        if 2 * k == T:
            rows.append(np.cos(np.pi * t) / np.sqrt(T))
        else:
            rows.append(np.sqrt(2.0 / T) * np.cos(2.0 * np.pi * k * t / T))
            rows.append(np.sqrt(2.0 / T) * np.sin(2.0 * np.pi * k * t / T))
    return np.stack(rows)


def moving_average_operator(T: int, w: int, stride: int = 1) -> np.ndarray:
    """The means of the "valid" windows [j stride, j stride + w), j = 0 .. (T - w) // stride: overlapping when stride < w."""
    _int_in("T", T, 1, 1024, "moving_average_operator")
    _int_in("w", w, 1, T, "moving_average_operator")
    _int_in("stride", stride, 1, T, "moving_average_operator")
    starts = range(0, T - w + 1, stride)
    P = np.zeros((len(starts), T))
    for j, lo in enumerate(starts):
        P[j, lo:lo + w] = 1.0 / w
    return P


def difference_operator(T: int) -> np.ndarray:
    """Increments instead of levels: (P v)_j = v_{j+1} - v_j, (T - 1, T)."""
    _int_in("T", T, 2, 1024, "difference_operator")
    P = np.zeros((T - 1, T))
    idx = np.arange(T - 1)
    P[idx, idx] = -1.0
    P[idx, idx + 1] = 1.0
    return P


def gaussian_blur_operator(T: int, sigma: float, stride: int = 1) -> np.ndarray:
    """A sensor with a Gaussian response of standard deviation `sigma` time steps, read every `stride` steps: row j is
    exp(-(t - j stride)^2 / (2 sigma^2)) over t in [0, T), normalised to sum 1; (ceil(T / stride), T)."""
    _int_in("T", T, 1, 1024, "gaussian_blur_operator")
    _int_in("stride", stride, 1, T, "gaussian_blur_operator")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not np.isfinite(sigma) or sigma <= 0:
        raise ValueError(f"gaussian_blur_operator: sigma must be a finite number > 0, got {sigma!r}")
    t = np.arange(T, dtype=np.float64)
    centres = np.arange(0, T, stride, dtype=np.float64)
    P = np.exp(-0.5 * ((t[None, :] - centres[:, None]) / float(sigma)) ** 2)
    return P / P.sum(axis=1, keepdims=True)


def window_mean_operator(T: int, w: int) -> np.ndarray:
    """The matrix of ``window_means``: row j averages window [j w, min((j + 1) w, T)), (ceil(T / w), T).  ``impute(operator=this)``
    is ``impute(aggregate=w)`` up to f32 rounding (disjoint windows: orthogonal rows)."""
    _int_in("T", T, 1, 1024, "window_mean_operator")
    _int_in("w", w, 1, T, "window_mean_operator")
    P = np.zeros((-(-T // w), T))
    for j, lo in enumerate(range(0, T, w)):
        hi = min(lo + w, T)
        P[j, lo:hi] = 1.0 / (hi - lo)
    return P


OPERATOR_KINDS = ("lowpass", "moving_average", "difference", "gaussian_blur")


def operator_from_config(kind, T: int, n_freq: int = 8, w: int = 4, stride: int = 1, sigma: float = 2.0) -> Optional[np.ndarray]:
    """The operator of cmd/impute.py's ``operator`` block: kind null | lowpass (n_freq) | moving_average (w, stride) | difference |
    gaussian_blur (sigma, stride); None for kind null."""
    if kind is None or str(kind) in ("null", "None", "none"):
        return None
    kind = str(kind)
    if kind == "lowpass":
        return lowpass_operator(T, int(n_freq))
    if kind == "moving_average":
        return moving_average_operator(T, int(w), int(stride))
    if kind == "difference":
        return difference_operator(T)
    if kind == "gaussian_blur":
        return gaussian_blur_operator(T, float(sigma), int(stride))
    raise ValueError(f"unknown operator kind {kind!r} (null | {' | '.join(OPERATOR_KINDS)})")
