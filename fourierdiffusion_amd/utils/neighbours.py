"""Nearest neighbours between two sample sets on the HIP engine (not in the reference): the two primitives every sample-space
metric of sampling/metrics.py is built from.

``knn`` is fd_knn_rows (csrc/fd_neighbours.hip): distances and selection in one fused fp32-MFMA kernel, the (n, m) distance matrix
never exists; the returned distances are recomputed exactly for the returned indices.  ``ball_counts`` is fd_ball_counts: the same
kernel with a compare-and-count epilogue.  Both are deterministic; ties go to the lower index."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _C
from .tensors import check_flat_array

MAX_K = 16


def _rows_features(x) -> tuple[int, int]:
    shape = tuple(x.shape)
    if len(shape) < 2 or min(shape) < 1:
        raise ValueError(f"a sample set must be a non-empty (n, ...) array, got shape {shape}")
    return shape[0], int(np.prod(shape[1:]))


def _check_pair(queries, references) -> None:
    """Shape errors are raised before anything is moved to the device."""
    (_, dq), (_, dr) = _rows_features(queries), _rows_features(references)
    if dq != dr:
        raise ValueError(f"queries have {dq} features and references {dr}")


def _pair(queries, references) -> tuple[torch.Tensor, torch.Tensor]:
    q = check_flat_array(queries)
    r = q if queries is references else check_flat_array(references).to(q.device)
    return q, r


def knn(queries, references, k: int, exclude_self: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """(dist (n, k) float32 Euclidean, idx (n, k) int64) on the device: the k nearest rows of `references` for every row of
    `queries`, ascending in (distance, index).  exclude_self: `queries` and `references` are the same set (pass the same object)
    and row i never returns itself."""
    _check_pair(queries, references)
    if exclude_self and queries is not references:
        raise ValueError("exclude_self needs the queries and the references to be the same array")
    limit = min(MAX_K, references.shape[0] - (1 if exclude_self else 0))
    if int(k) != k or not 1 <= k <= limit:
        raise ValueError(f"k={k} outside [1, {limit}] (at most {MAX_K}, and no more than the references "
                         f"{'other than the row itself ' if exclude_self else ''}can supply)")
    k = int(k)
    q, r = _pair(queries, references)
    n, d = q.shape
    m = r.shape[0]
    h, L = _C.ctx(q.device), _C.lib()
    need = C.c_size_t(0)
    _C.check(L.fd_knn_rows_workspace_bytes(h, n, m, d, k, C.byref(need)), h)
    work = torch.empty((need.value,), dtype=torch.uint8, device=q.device)
    dist2 = torch.empty((n, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=q.device)
    _C.check(L.fd_knn_rows(h, q.data_ptr(), n, r.data_ptr(), m, d, k, 1 if exclude_self else 0, dist2.data_ptr(), idx.data_ptr(),
                           work.data_ptr(), need.value, _C.stream_of(q)), h)
    return dist2.sqrt_(), idx.long()


def ball_counts(queries, references, radii) -> torch.Tensor:
    """counts (n,) int64 on the device: for every query the number of reference rows j with d(q_i, r_j) <= radii[j]."""
    _check_pair(queries, references)
    if isinstance(radii, np.ndarray):
        radii = torch.from_numpy(np.ascontiguousarray(radii))
    rad = torch.as_tensor(radii).detach().float().reshape(-1)
    if rad.shape[0] != references.shape[0]:
        raise ValueError(f"{rad.shape[0]} radii for {references.shape[0]} references")
    if not bool((torch.isfinite(rad) & (rad >= 0)).all()):
        raise ValueError("radii must be finite and >= 0")
    q, r = _pair(queries, references)
    rad = rad.to(q.device).contiguous()
    n, d = q.shape
    counts = torch.empty((n,), dtype=torch.int32, device=q.device)
    rad2 = rad * rad
    h = _C.ctx(q.device)
    _C.check(_C.lib().fd_ball_counts(h, q.data_ptr(), n, r.data_ptr(), r.shape[0], d, rad2.data_ptr(), counts.data_ptr(),
                                     _C.stream_of(q)), h)
    return counts.long()
