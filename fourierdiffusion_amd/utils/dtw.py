"""Dynamic time warping under a Sakoe-Chiba band on the HIP engine (not in the reference): the time-warp-aware twins of
utils/neighbours.py, and the primitives of DTWPrecisionRecall / DTWMemorisation in sampling/metrics.py.

For series a, b of shape (T, C) and a window w in [0, T - 1]:

    c(i, j) = sum_c (a[i, c] - b[j, c])^2,    D(0, 0) = c(0, 0),
    D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1))    for |i - j| <= w,
    dtw(a, b; w) = sqrt(D(T-1, T-1)).

w = 0 is the Euclidean distance, w = T - 1 unconstrained DTW; all channels warp together.  ``window=None`` is the UCR convention
ceil(0.1 T), ``window="full"`` is T - 1.  Everything runs in csrc/fd_dtw.hip, one (query, reference) pair per lane: the (n, m)
matrix never exists, results are deterministic, ties go to the lower index, and the distance ``dtw_knn`` returns for a pair is bit
for bit ``dtw_pairs`` of that pair."""
from __future__ import annotations

import operator

import torch

from .. import _C
from ._pairs import MAX_K, call_with_workspace, check_k, check_radii, same_pair, squared_on  # noqa: F401  (MAX_K: public here)

MAX_LENGTH = 1024
MAX_BAND = 256        # the largest band column min(2 w + 1, T) the kernel stores


def default_window(T: int) -> int:
    """ceil(0.1 T), the UCR convention (never above T - 1)."""
    if isinstance(T, bool) or int(T) != T or T < 1:
        raise ValueError(f"T={T} must be a positive integer")
    T = int(T)
    return min(T - 1, (T + 9) // 10)


def _series_shape(x, what: str) -> tuple[int, int, int]:
    shape = tuple(x.shape)
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{what} must be a non-empty (n, T, C) or (n, T) array, got shape {tuple(x.shape)}")
    if shape[1] > MAX_LENGTH:
        raise ValueError(f"{what} have T={shape[1]} points, the kernel takes at most {MAX_LENGTH}")
    return shape


def _window(window, T: int) -> int:
    if window is None:
        w = default_window(T)
    elif isinstance(window, str):
        if window != "full":
            raise ValueError(f"window={window!r}: an integer in [0, T - 1], None (ceil(0.1 T)) or 'full'")
        w = T - 1
    else:
        try:
            w = None if isinstance(window, bool) else operator.index(window)
        except TypeError:
            w = None
        if w is None:
            raise ValueError(f"window={window!r}: an integer in [0, T - 1], None (ceil(0.1 T)) or 'full'")
        if not 0 <= w <= T - 1:
            raise ValueError(f"window={w} outside [0, T - 1 = {T - 1}]")
    if min(2 * w + 1, T) > MAX_BAND:
        raise ValueError(f"window={w} stores a band column of {min(2 * w + 1, T)} entries, the kernel takes at most {MAX_BAND}")
    return w


def _check_pair(a, b, what_a: str, what_b: str) -> tuple[int, int]:
    """(T, C) of both sets; shape errors are raised before anything is moved to the device."""
    (_, T, Cn), (_, Tb, Cb) = _series_shape(a, what_a), _series_shape(b, what_b)
    if (T, Cn) != (Tb, Cb):
        raise ValueError(f"{what_a} are series of shape {(T, Cn)} and {what_b} of shape {(Tb, Cb)}: equal lengths and channels only")
    return T, Cn


def dtw_pairs(a, b, window=None) -> torch.Tensor:
    """(n,) float32 on the device: dtw(a_i, b_i) of the rows of two (n, T, C) sets."""
    T, Cn = _check_pair(a, b, "a", "b")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"a has {a.shape[0]} series and b {b.shape[0]}")
    w = _window(window, T)
    x, y = same_pair(a, b)
    dist2 = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    h = _C.ctx(x.device)
    _C.check(_C.lib().fd_dtw_pairs(h, x.data_ptr(), y.data_ptr(), x.shape[0], T, Cn, w, dist2.data_ptr(), _C.stream_of(x)), h)
    return dist2.sqrt_()


def dtw_knn(queries, references, k: int, window=None, exclude_self: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """(dist (n, k) float32, idx (n, k) int64) on the device: the k nearest series of `references` under DTW for every series of
    `queries`, ascending in (distance, index).  exclude_self: `queries` and `references` are the same set (pass the same object)
    and series i never returns itself."""
    T, Cn = _check_pair(queries, references, "queries", "references")
    w = _window(window, T)
    if exclude_self and queries is not references:
        raise ValueError("exclude_self needs the queries and the references to be the same array")
    k = check_k(k, references, exclude_self, "series", allow_bool=False)
    q, r = same_pair(queries, references)
    n, m = q.shape[0], r.shape[0]
    L = _C.lib()
    dist2 = torch.empty((n, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=q.device)
    call_with_workspace(q, L.fd_dtw_knn_workspace_bytes, (n, m, T, Cn, w, k), lambda h, work, nbytes, stream: L.fd_dtw_knn(
        h, q.data_ptr(), n, r.data_ptr(), m, T, Cn, w, k, 1 if exclude_self else 0, dist2.data_ptr(), idx.data_ptr(), work, nbytes,
        stream))
    return dist2.sqrt_(), idx.long()


def dtw_ball_counts(queries, references, radii, window=None) -> torch.Tensor:
    """counts (n,) int64 on the device: for every query the number of reference series j with dtw(q_i, r_j) <= radii[j]."""
    T, Cn = _check_pair(queries, references, "queries", "references")
    w = _window(window, T)
    rad = check_radii(radii, references)
    q, r = same_pair(queries, references)
    n, m = q.shape[0], r.shape[0]
    rad2 = squared_on(rad, q.device)
    L = _C.lib()
    counts = torch.empty((n,), dtype=torch.int32, device=q.device)
    call_with_workspace(q, L.fd_dtw_ball_counts_workspace_bytes, (n, m, T, Cn, w), lambda h, work, nbytes, stream: L.fd_dtw_ball_counts(
        h, q.data_ptr(), n, r.data_ptr(), m, T, Cn, w, rad2.data_ptr(), counts.data_ptr(), work, nbytes, stream))
    return counts.long()
