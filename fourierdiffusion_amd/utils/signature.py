"""Path signatures on the HIP engine (not in the reference): the iterated integrals of a series up to depth m, the feature map behind
Sig-W1 (Ni et al. 2021, Sig-Wasserstein GANs) and the signature MMD (Chevyrev & Oberhauser).  Level 1 is the total increment, level 2
holds the Levy areas -- which channel leads which -- and the levels above hold asymmetries in time that no correlation sees: a series
played backwards has the same autocorrelation and spectrum and another signature.

The path of a series x (T, C), in this order (include/fdiff_hip.h, fd_series_signature):
    1. p[t, c] = channel_scale_c path_scale (x[t, c] - channel_offset_c), in double
    2. basepoint: the point 0 is prepended, so that the signature sees the starting value and not only the increments
    3. increments over S = T - 1 segments (T with a basepoint)
    4. lead_lag: 2 S segments over the 2 C channels [lead_0.., lag_0..], moved in turn
    5. time_augment: one last channel that moves by 1 / S' per segment
d is the final channel count and D = d + d^2 + ... + d^depth the number of features: levels 1..depth concatenated, a level row-major
over its words with the first letter slowest.  Everything runs in one fused kernel in double (csrc/fd_signature.hip); the set mean is
deterministic (no atomics) and a series' features depend on that series alone.  `expected_signature_distance` is host arithmetic in
float64 on the D-vectors."""
from __future__ import annotations

import math
import operator
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _C
from ._pairs import call_with_workspace

MAX_LENGTH = 1024
MAX_CHANNELS = 64
MAX_DEPTH = 6
MAX_FEATURES = 8192
CHUNK_SERIES = 32          # series per partial sum of the set mean (the engine's constant)
PER_SERIES = ("sig", "sqnorm")


@dataclass
class SeriesSignature:
    sig: Optional[torch.Tensor]      # (n, D) float32
    sqnorm: Optional[torch.Tensor]   # (n,) float64: sum_w S_w^2 of every series
    mean: torch.Tensor               # (D,) float64: the expected signature of the set
    d: int                           # letters
    depth: int
    levels: list                     # the slice of every level in the feature axis
    n: int                           # series in the set
    sqnorm_sum: Optional[float] = None   # sum_i ||S_i||^2, kept for the MMD when the per-series array is not


def _index(name: str, value, lo: int, hi: int) -> int:
    try:
        v = None if isinstance(value, bool) else operator.index(value)
    except TypeError:
        v = None
    if v is None or not lo <= v <= hi:
        raise ValueError(f"{name}={value!r} must be an integer in [{lo}, {hi}]")
    return v


def signature_dim(channels: int, depth: int, *, time_augment: bool = True, lead_lag: bool = False) -> tuple[int, int]:
    """(d, D): the letters of the augmented path and the number of signature features up to `depth`."""
    channels = _index("channels", channels, 1, MAX_CHANNELS)
    depth = _index("depth", depth, 1, MAX_DEPTH)
    d = channels * (2 if lead_lag else 1) + (1 if time_augment else 0)
    return d, sum(d ** k for k in range(1, depth + 1))


def level_slices(d: int, depth: int) -> list:
    """The slice of level k = 1..depth in the feature axis."""
    out, lo = [], 0
    for k in range(1, depth + 1):
        out.append(slice(lo, lo + d ** k))
        lo += d ** k
    return out


def _series_shape(x, what: str = "X") -> tuple[int, int, int]:
    shape = tuple(x.shape)
    if len(shape) != 3 or shape[0] < 1 or shape[1] < 2 or shape[2] < 1:
        raise ValueError(f"{what} must be an (n, T, C) array with n >= 1, T >= 2 and C >= 1, got shape {shape}")
    if shape[1] > MAX_LENGTH or shape[2] > MAX_CHANNELS:
        raise ValueError(f"{what} has T={shape[1]} points and C={shape[2]} channels, the kernel takes at most {MAX_LENGTH} and "
                         f"{MAX_CHANNELS}")
    return shape


def check_options(n: int, C: int, depth, time_augment: bool, lead_lag: bool) -> tuple[int, int, int]:
    """(depth, d, D) or a ValueError that names the limit."""
    depth = _index("depth", depth, 1, MAX_DEPTH)
    d, D = signature_dim(C, depth, time_augment=bool(time_augment), lead_lag=bool(lead_lag))
    if D > MAX_FEATURES:
        raise ValueError(f"{d} letters at depth {depth} give D = {D} features, at most {MAX_FEATURES}: lower the depth")
    if n * D >= 2 ** 31:
        raise ValueError(f"too large: n * D = {n * D} must stay below 2^31")
    return depth, d, D


def _channel_vector(name: str, value, C: int, fill: float, nonnegative: bool) -> np.ndarray:
    if value is None:
        return np.full((C,), fill, dtype=np.float64)
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    v = np.asarray(value, dtype=np.float64).reshape(-1)
    if v.shape[0] != C:
        raise ValueError(f"{name} has {v.shape[0]} entries for {C} channels")
    if not np.isfinite(v).all() or (nonnegative and (v < 0).any()):
        raise ValueError(f"{name} must be finite{' and >= 0' if nonnegative else ''}")
    return v


def _check_per_series(per_series: Sequence[str]) -> tuple[str, ...]:
    if isinstance(per_series, str):
        per_series = (per_series,)
    names = tuple(per_series)
    for name in names:
        if name not in PER_SERIES:
            raise ValueError(f"per_series names {name!r}: one of {PER_SERIES}")
    return names


def series_signature(X, depth: int = 3, *, time_augment: bool = True, basepoint: bool = False, lead_lag: bool = False,
                     channel_offset=None, channel_scale=None, path_scale: float = 1.0,
                     per_series: Sequence[str] = ()) -> SeriesSignature:
    """The signature of every series of X (n, T, C) and the expected signature of the set.  `per_series` names the per-series arrays
    to return, of ("sig", "sqnorm"); the set mean and the sum of the squared norms (what the MMD needs) are always computed.
    `path_scale` multiplies `channel_scale`: level k then scales by path_scale^k, except where the time letter occurs (it is not
    scaled)."""
    n, T, Cn = _series_shape(X)
    depth, d, D = check_options(n, Cn, depth, time_augment, lead_lag)
    names = _check_per_series(per_series)
    if n * T * Cn >= 2 ** 31:
        raise ValueError(f"too large: n * T * C = {n * T * Cn} must stay below 2^31")
    if isinstance(path_scale, bool) or not isinstance(path_scale, (int, float)) or not math.isfinite(path_scale) or path_scale < 0:
        raise ValueError(f"path_scale={path_scale!r} must be a finite number >= 0")
    offset = _channel_vector("channel_offset", channel_offset, Cn, 0.0, False)
    with np.errstate(over="ignore"):
        scale = _channel_vector("channel_scale", channel_scale, Cn, 1.0, True) * float(path_scale)
    if not np.isfinite(scale).all():
        raise ValueError("channel_scale * path_scale must be finite")
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X))
    if not isinstance(X, torch.Tensor):
        raise _C.FdError("X must be a torch.Tensor or a numpy array")
    if X.device.type != "cuda":
        if not torch.cuda.is_available():
            raise _C.FdError("series_signature runs on the HIP engine and no GPU is visible (no CPU fallback)")
        X = X.to("cuda")
    xt = _C.dev_f32(X.detach(), "X")
    lib = _C.lib()
    dev = xt.device
    flags = (_C.FD_SIG_BASEPOINT if basepoint else 0) | (_C.FD_SIG_LEAD_LAG if lead_lag else 0) | (_C.FD_SIG_TIME if time_augment else 0)
    off_d = torch.from_numpy(offset).to(dev)
    scl_d = torch.from_numpy(scale).to(dev)
    sig = torch.empty((n, D), dtype=torch.float32, device=dev) if "sig" in names else None
    sqnorm = torch.empty((n,), dtype=torch.float64, device=dev)
    mean = torch.empty((D,), dtype=torch.float64, device=dev)
    call_with_workspace(xt, lib.fd_series_signature_workspace_bytes, (n, T, Cn, depth, flags), lambda hd, work, nbytes, stream:
                        lib.fd_series_signature(hd, xt.data_ptr(), n, T, Cn, depth, flags, off_d.data_ptr(), scl_d.data_ptr(),
                                                _C.ptr(sig), sqnorm.data_ptr(), mean.data_ptr(), work, nbytes, stream))
    total = float(sqnorm.cpu().numpy().sum())            # a float64 sum on the host
    return SeriesSignature(sig=sig, sqnorm=sqnorm if "sqnorm" in names else None, mean=mean, d=d, depth=depth,
                           levels=level_slices(d, depth), n=n, sqnorm_sum=total)


def _own_term(s: SeriesSignature, mean: np.ndarray) -> float:
    """(||sum_i S_i||^2 - sum_i ||S_i||^2) / (n (n - 1)): the mean of <S_i, S_j> over i != j; 0 for a single series."""
    if s.n < 2:
        return 0.0
    total = s.sqnorm_sum if s.sqnorm_sum is not None else float(s.sqnorm.cpu().numpy().sum())
    return float((s.n * s.n * float(mean @ mean) - total) / (s.n * (s.n - 1)))


def expected_signature_distance(a: SeriesSignature, b: SeriesSignature) -> dict:
    """Between two sets, in float64 on the host from the expected signatures and the sums of the squared norms:
        sig_w1          ||mean_a - mean_b||_2 (Sig-W1)
        sig_w1_levels   the same norm level by level
        sig_mmd2        the unbiased MMD^2 under the linear kernel on signatures,
                        (||sum a||^2 - sum ||a_i||^2) / (n (n - 1)) + the same for b - 2 <mean_a, mean_b>;
                        a set of one series contributes 0 for its own term
    A p-value: `mmd_permutation_test(sig_a, sig_b)` (utils/two_sample.py) on the per-series feature rows."""
    if (a.d, a.depth) != (b.d, b.depth):
        raise ValueError(f"signatures of different shape: (d, depth) = {(a.d, a.depth)} and {(b.d, b.depth)}")
    ma, mb = a.mean.detach().cpu().numpy().astype(np.float64), b.mean.detach().cpu().numpy().astype(np.float64)
    diff = ma - mb
    return {"sig_w1": float(np.sqrt(diff @ diff)),
            "sig_w1_levels": [float(np.sqrt(diff[sl] @ diff[sl])) for sl in a.levels],
            "sig_mmd2": _own_term(a, ma) + _own_term(b, mb) - 2.0 * float(ma @ mb)}
