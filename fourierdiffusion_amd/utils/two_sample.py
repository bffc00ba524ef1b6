"""Kernel two-sample test on the HIP engine (not in the reference; Gretton et al. 2012): the unbiased MMD^2 of two sample sets under a
Gaussian kernel mixture, with a p-value from permuting the pooled rows.  Where the other metrics return a number without a scale,
this one answers "can these samples be told apart from those at this sample size, and how surely".

``kernel_quadforms`` is fd_kernel_quadforms (csrc/fd_mmd.hip): for every column of a 0/1 membership matrix the quadratic form of the
kernel matrix, in one fused fp32-MFMA kernel; the (N, N) matrix never exists.  Everything after it is float64 host arithmetic
(``mmd2_from_quadforms``, ``permutation_p_value``).  Deterministic: the permutations come from numpy's Generator(seed), the engine
uses no atomics."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _C
from ._pairs import call_with_workspace
from .neighbours import _rows_features
from .tensors import check_flat_array

DEFAULT_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
MAX_SCALES = 8
MAX_COLUMNS = 1024


@dataclass
class MMDResult:
    mmd2: float                  # unbiased MMD^2 of the observed split
    p_value: float               # (1 + #{permutations with mmd2 >= observed}) / (1 + n_permutations)
    null: np.ndarray             # (n_permutations,) MMD^2 of the permuted splits
    bandwidth2: float            # base2 as used: the kernel is (1/Q) sum_q exp(-||a - b||^2 / (c_q base2))
    witness_x: np.ndarray        # (n,) witness function at the rows of x: mean k(., x') - mean k(., y'), the row itself left out
    witness_y: np.ndarray        # (m,)


def _check_scales(scales) -> tuple[float, ...]:
    try:
        out = tuple(float(c) for c in scales)
    except TypeError:
        raise ValueError(f"scales must be a sequence of numbers, got {scales!r}") from None
    if not 1 <= len(out) <= MAX_SCALES:
        raise ValueError(f"{len(out)} scales: between 1 and {MAX_SCALES} are supported")
    if not all(np.isfinite(c) and c > 0 for c in out):
        raise ValueError(f"scales must be finite and > 0, got {out}")
    return out


def _check_bandwidth2(bandwidth2) -> float:
    if bandwidth2 is None:
        return 0.0
    b = float(bandwidth2)
    if not (np.isfinite(b) and b > 0):
        raise ValueError(f"bandwidth2={bandwidth2} must be finite and > 0 (None: the pooled mean squared pair distance)")
    return b


def _check_count(name: str, value, lowest: int) -> int:
    if isinstance(value, bool) or int(value) != value or value < lowest:
        raise ValueError(f"{name}={value} must be an integer >= {lowest}")
    return int(value)


def permutation_members(n: int, m: int, n_permutations: int, seed: int) -> np.ndarray:
    """(n + m, 1 + n_permutations) uint8 memberships of the first group: column 0 is the first n rows, column p is
    default_rng(seed).permutation(n + m)[:n], the permutations drawn in order from one generator."""
    n, m = _check_count("n", n, 1), _check_count("m", m, 1)
    n_permutations = _check_count("n_permutations", n_permutations, 0)
    if 1 + n_permutations > MAX_COLUMNS:
        raise ValueError(f"n_permutations={n_permutations}: at most {MAX_COLUMNS - 1}")
    rng = np.random.default_rng(seed)
    member = np.zeros((n + m, 1 + n_permutations), dtype=np.uint8)
    member[:n, 0] = 1
    for p in range(1, 1 + n_permutations):
        member[rng.permutation(n + m)[:n], p] = 1
    return member


def kernel_quadforms(z, member, scales: Sequence[float] = DEFAULT_SCALES, bandwidth2: Optional[float] = None,
                     col_splits: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(quad (P,), rowsum (N,), col0 (N,), base2 (1,)) float64 on the device, for the rows z (N, ...) and the 0/1 memberships
    member (N, P) uint8 / bool:
      quad[p] = sum_{i != j} member[i, p] k(z_i, z_j) member[j, p]      rowsum[i] = sum_{j != i} k(z_i, z_j)
      col0[i] = sum_{j != i} k(z_i, z_j) member[j, 0]                   base2: bandwidth2, or the mean squared distance over i != j
    with k(a, b) = mean_q exp(-||a - b||^2 / (scales[q] base2)).  col_splits: 0 = automatic; the result is the same for every value."""
    N, d = _rows_features(z)
    if N < 2:
        raise ValueError(f"{N} row: a kernel two-sample statistic needs at least two")
    if isinstance(member, np.ndarray):
        byte_like = member.dtype in (np.dtype(np.uint8), np.dtype(np.bool_))
    elif isinstance(member, torch.Tensor):
        byte_like = member.dtype in (torch.uint8, torch.bool)
    else:
        raise ValueError(f"member must be a numpy array or a torch tensor, got {type(member)}")
    if not byte_like:
        raise ValueError(f"member must be uint8 or bool, got {member.dtype}")
    mshape = tuple(member.shape)
    if len(mshape) != 2 or mshape[0] != N:
        raise ValueError(f"member has shape {mshape}, expected ({N}, P)")
    P = mshape[1]
    if not 1 <= P <= MAX_COLUMNS:
        raise ValueError(f"member has {P} columns: between 1 and {MAX_COLUMNS} are supported")
    scales = _check_scales(scales)
    bw2 = _check_bandwidth2(bandwidth2)
    col_splits = _check_count("col_splits", col_splits, 0)
    if N * d >= 2 ** 31 or N * P >= 2 ** 31:
        raise ValueError(f"too large: N * d = {N * d} and N * P = {N * P} must stay below 2^31")

    zt = check_flat_array(z)
    if isinstance(member, np.ndarray):
        member = torch.from_numpy(np.ascontiguousarray(member).view(np.uint8))
    mt = member.detach().to(device=zt.device, dtype=torch.uint8).contiguous()
    L = _C.lib()
    quad = torch.empty((P,), dtype=torch.float64, device=zt.device)
    rowsum = torch.empty((N,), dtype=torch.float64, device=zt.device)
    col0 = torch.empty((N,), dtype=torch.float64, device=zt.device)
    base2 = torch.empty((1,), dtype=torch.float64, device=zt.device)
    cs = (C.c_double * len(scales))(*scales)
    call_with_workspace(zt, L.fd_kernel_quadforms_workspace_bytes, (N, d, P, col_splits), lambda h, work, nbytes, stream:
                        L.fd_kernel_quadforms(h, zt.data_ptr(), N, d, cs, len(scales), bw2, mt.data_ptr(), P, col_splits,
                                              quad.data_ptr(), rowsum.data_ptr(), col0.data_ptr(), base2.data_ptr(), work, nbytes,
                                              stream))
    return quad, rowsum, col0, base2


def _pair_term(total: np.ndarray, pairs: np.ndarray) -> np.ndarray:
    """total / pairs, 0 where a group has no pair."""
    return np.divide(total, pairs, out=np.zeros_like(total), where=pairs > 0)


def mmd2_from_quadforms(quad, rowsum, member) -> np.ndarray:
    """(P,) unbiased MMD^2 of every column, float64: with n = sum_i A[i,p], m = N - n, S = sum rowsum and ar = A[:,p] . rowsum, the
    cross sum is xy = ar - quad and the second group's yy = S - 2 ar + quad, and
      mmd2 = quad / (n (n - 1)) + yy / (m (m - 1)) - 2 xy / (n m)
    (a group of one row has no pair: its term is 0)."""
    quad, rowsum = np.asarray(quad, dtype=np.float64), np.asarray(rowsum, dtype=np.float64)
    A = np.asarray(member).astype(np.float64)
    N = A.shape[0]
    n = A.sum(axis=0)
    m = N - n
    if (n < 1).any() or (m < 1).any():
        raise ValueError("every column of member needs at least one row in each group")
    ar = A.T @ rowsum
    xy = ar - quad
    yy = rowsum.sum() - 2.0 * ar + quad
    return _pair_term(quad, n * (n - 1)) + _pair_term(yy, m * (m - 1)) - 2.0 * xy / (n * m)


def permutation_p_value(mmd2) -> float:
    """(1 + #{p >= 1 : mmd2[p] >= mmd2[0]}) / P: column 0 is the observed split and counts as one of the P arrangements."""
    mmd2 = np.asarray(mmd2, dtype=np.float64)
    return float(1 + int((mmd2[1:] >= mmd2[0]).sum())) / mmd2.shape[0]


def witness_from_quadforms(rowsum, col0, member0) -> np.ndarray:
    """(N,) witness values col0[i] / n' - (rowsum[i] - col0[i]) / m': the mean kernel value to the first group minus that to the
    second, where n' and m' leave the row itself out of its own group."""
    rowsum, col0 = np.asarray(rowsum, dtype=np.float64), np.asarray(col0, dtype=np.float64)
    a = np.asarray(member0).astype(np.float64)
    n = a.sum()
    m = a.shape[0] - n
    return _pair_term(col0, n - a) - _pair_term(rowsum - col0, m - (1.0 - a))


def mmd_permutation_test(x, y, n_permutations: int = 200, scales: Sequence[float] = DEFAULT_SCALES,
                         bandwidth2: Optional[float] = None, seed: int = 0) -> MMDResult:
    """The kernel two-sample test of x (n, ...) against y (m, ...): unbiased MMD^2 and its permutation p-value."""
    (n, dx), (m, dy) = _rows_features(x), _rows_features(y)
    if dx != dy:
        raise ValueError(f"x has {dx} features and y {dy}")
    if n < 2 or m < 2:
        raise ValueError(f"the unbiased MMD^2 needs at least two rows in each set, got {n} and {m}")
    member = permutation_members(n, m, n_permutations, seed)
    scales = _check_scales(scales)
    _check_bandwidth2(bandwidth2)
    xt = check_flat_array(x)
    z = torch.cat([xt, check_flat_array(y).to(xt.device)], dim=0)
    quad, rowsum, col0, base2 = kernel_quadforms(z, member, scales=scales, bandwidth2=bandwidth2)
    quad, rowsum, col0 = quad.cpu().numpy(), rowsum.cpu().numpy(), col0.cpu().numpy()
    mmd2 = mmd2_from_quadforms(quad, rowsum, member)
    witness = witness_from_quadforms(rowsum, col0, member[:, 0])
    return MMDResult(mmd2=float(mmd2[0]), p_value=permutation_p_value(mmd2), null=mmd2[1:].copy(), bandwidth2=float(base2.item()),
                     witness_x=witness[:n].copy(), witness_y=witness[n:].copy())
