"""Observation masks of cmd/impute.py (conditional sampling, an extension: not in the reference).  Pure functions on the CPU:
True = observed, False = hidden (what the sampler fills in)."""
from __future__ import annotations

from typing import Optional, Tuple

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
