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
