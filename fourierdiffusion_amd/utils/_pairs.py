"""What the all-pairs metric wrappers share (neighbours.py, dtw.py, two_sample.py): argument checks whose error texts the tests
match on, and the "ask for the workspace bytes, allocate, call" sequence of the engine entries that take a caller's workspace."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _C
from .tensors import check_flat_array

MAX_K = 16


def same_pair(a, b) -> tuple[torch.Tensor, torch.Tensor]:
    """Both sets as flat float32 device arrays; the same object stays the same tensor (the engine then centres / transposes once,
    and exclude_self asks for it)."""
    x = check_flat_array(a)
    y = x if a is b else check_flat_array(b).to(x.device)
    return x, y


def check_k(k, references, exclude_self: bool, itself: str, allow_bool: bool) -> int:
    """k in [1, min(MAX_K, what the references can supply)]; `itself` names the excluded element in the error text."""
    limit = min(MAX_K, references.shape[0] - (1 if exclude_self else 0))
    if (not allow_bool and isinstance(k, bool)) or int(k) != k or not 1 <= k <= limit:
        raise ValueError(f"k={k} outside [1, {limit}] (at most {MAX_K}, and no more than the references "
                         f"{f'other than the {itself} itself ' if exclude_self else ''}can supply)")
    return int(k)


def check_radii(radii, references) -> torch.Tensor:
    """(m,) float32 radii on the host, one per reference, finite and >= 0."""
    if isinstance(radii, np.ndarray):
        radii = torch.from_numpy(np.ascontiguousarray(radii))
    rad = torch.as_tensor(radii).detach().float().reshape(-1)
    if rad.shape[0] != references.shape[0]:
        raise ValueError(f"{rad.shape[0]} radii for {references.shape[0]} references")
    if not bool((torch.isfinite(rad) & (rad >= 0)).all()):
        raise ValueError("radii must be finite and >= 0")
    return rad


def squared_on(rad: torch.Tensor, device) -> torch.Tensor:
    rad = rad.to(device).contiguous()
    return rad * rad


def call_with_workspace(x: torch.Tensor, bytes_fn, bytes_args, run) -> None:
    """bytes_fn(ctx, *bytes_args, &need); a uint8 workspace of that size on x's device; run(ctx, work pointer, need, stream)."""
    h = _C.ctx(x.device)
    need = C.c_size_t(0)
    _C.check(bytes_fn(h, *bytes_args, C.byref(need)), h)
    work = torch.empty((need.value,), dtype=torch.uint8, device=x.device)
    _C.check(run(h, work.data_ptr(), need.value, _C.stream_of(x)), h)
