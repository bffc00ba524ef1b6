"""Nearest neighbours between two sample sets on the HIP engine (not in the reference): the two primitives every sample-space
metric of sampling/metrics.py is built from.

``knn`` is fd_knn_rows (csrc/fd_neighbours.hip): distances and selection in one fused fp32-MFMA kernel, the (n, m) distance matrix
never exists; the returned distances are recomputed exactly for the returned indices.  ``ball_counts`` is fd_ball_counts: the same
kernel with a compare-and-count epilogue.  Both are deterministic; ties go to the lower index."""
from __future__ import annotations

import numpy as np
import torch

from .. import _C
from ._pairs import MAX_K, call_with_workspace, check_k, check_radii, same_pair, squared_on  # noqa: F401  (MAX_K: public here)


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


def knn(queries, references, k: int, exclude_self: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """(dist (n, k) float32 Euclidean, idx (n, k) int64) on the device: the k nearest rows of `references` for every row of
    `queries`, ascending in (distance, index).  exclude_self: `queries` and `references` are the same set (pass the same object)
    and row i never returns itself."""
    _check_pair(queries, references)
    if exclude_self and queries is not references:
        raise ValueError("exclude_self needs the queries and the references to be the same array")
    k = check_k(k, references, exclude_self, "row", allow_bool=True)
    q, r = same_pair(queries, references)
    n, d = q.shape
    m = r.shape[0]
    L = _C.lib()
    dist2 = torch.empty((n, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=q.device)
    call_with_workspace(q, L.fd_knn_rows_workspace_bytes, (n, m, d, k), lambda h, work, nbytes, stream: L.fd_knn_rows(
        h, q.data_ptr(), n, r.data_ptr(), m, d, k, 1 if exclude_self else 0, dist2.data_ptr(), idx.data_ptr(), work, nbytes, stream))
    return dist2.sqrt_(), idx.long()


def ball_counts(queries, references, radii) -> torch.Tensor:
    """counts (n,) int64 on the device: for every query the number of reference rows j with d(q_i, r_j) <= radii[j]."""
    _check_pair(queries, references)
    rad = check_radii(radii, references)
    q, r = same_pair(queries, references)
    n, d = q.shape
    counts = torch.empty((n,), dtype=torch.int32, device=q.device)
    rad2 = squared_on(rad, q.device)
    h = _C.ctx(q.device)
    _C.check(_C.lib().fd_ball_counts(h, q.data_ptr(), n, r.data_ptr(), r.shape[0], d, rad2.data_ptr(), counts.data_ptr(),
                                     _C.stream_of(q)), h)
    return counts.long()
