"""The dependence structure inside a series on the HIP engine (not in the reference): per series and channel the first four
moments, the normalised autocorrelation and the normalised cross-correlation between channels, plus their means over the set --
what the autocorrelation difference of TSGBench and the correlational score of Ni et al. / Diffusion-TS are made of.

For one series x (T, C) and channel c (the biased estimators of numpy / statsmodels):

    mu = mean_t x,  e = x - mu,  m_k = mean_t e^k,  moments = (mu, sqrt(m_2), m_3 / m_2^1.5, m_4 / m_2^2 - 3)
    acf[l-1, c]  = sum_{t < T-l} e[t,c] e[t+l,c] / (T m_2(c)),                l = 1..lags
    ccf[l, c, d] = sum_{t < T-l} e[t,c] e[t+l,d] / (T sqrt(m_2(c) m_2(d))),   l = 0..cross_lags, every ORDERED pair

A channel that is constant over a series has all its normalised features 0, not NaN.  Everything runs in one fused kernel
(csrc/fd_dependence.hip, fd_series_dependence): a series is read once, the (n, cross_lags + 1, C, C) array is only written when it
is asked for, and the set means are deterministic (no atomics).  A series' features depend on that series alone."""
from __future__ import annotations

import operator
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _C
from ._pairs import call_with_workspace

MAX_LENGTH = 1024
MAX_CHANNELS = 64
CHUNK_SERIES = 32          # series per partial sum of the set means (the engine's constant)
PER_SERIES = ("moments", "acf", "ccf")


@dataclass
class SetMean:
    moments: torch.Tensor            # (C, 4) float64
    acf: torch.Tensor                # (lags, C)
    ccf: Optional[torch.Tensor]      # (cross_lags + 1, C, C), None without ccf


@dataclass
class SeriesDependence:
    moments: Optional[torch.Tensor]  # (n, C, 4) float32: mean, deviation, skewness, excess kurtosis
    acf: Optional[torch.Tensor]      # (n, lags, C)
    ccf: Optional[torch.Tensor]      # (n, cross_lags + 1, C, C)
    set_mean: SetMean                # the mean over the n series of every feature
    lags: int
    cross_lags: int                  # -1: no ccf


def _series_shape(x, what: str = "X") -> tuple[int, int, int]:
    shape = tuple(x.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{what} must be a non-empty (n, T, C) array, got shape {shape}")
    if shape[1] > MAX_LENGTH or shape[2] > MAX_CHANNELS:
        raise ValueError(f"{what} has T={shape[1]} points and C={shape[2]} channels, the kernel takes at most {MAX_LENGTH} and "
                         f"{MAX_CHANNELS}")
    return shape


def _index(name: str, value, lo: int, hi: int, extra: str = "") -> int:
    try:
        v = None if isinstance(value, bool) else operator.index(value)
    except TypeError:
        v = None
    if v is None or not lo <= v <= hi:
        raise ValueError(f"{name}={value!r} must be an integer in [{lo}, {hi}]{extra}")
    return v


def resolve_lags(T: int, C: int, lags=None, cross_lags=None) -> tuple[int, int]:
    """(lags, cross_lags) as the engine takes them.  lags=None: max(1, T // 4), never above T - 1; cross_lags=None: min(lags, 8), and
    no ccf (-1) for one channel; cross_lags=-1 asks for none."""
    L = min(T - 1, max(1, T // 4)) if lags is None else _index("lags", lags, 0, T - 1, f" (T - 1 for T={T})")
    if cross_lags is None:
        Lx = -1 if C == 1 else min(L, 8)
    else:
        Lx = _index("cross_lags", cross_lags, -1, T - 1, f" (T - 1 for T={T}; -1: no cross-correlation)")
    return L, Lx


def _check_per_series(per_series: Sequence[str], Lx: int) -> tuple[str, ...]:
    if isinstance(per_series, str):
        per_series = (per_series,)
    names = tuple(per_series)
    for name in names:
        if name not in PER_SERIES:
            raise ValueError(f"per_series names {name!r}: one of {PER_SERIES}")
    if "ccf" in names and Lx < 0:
        raise ValueError("per_series asks for 'ccf' but there are no cross lags (one channel, or cross_lags=-1)")
    return names


def series_dependence(X, lags=None, cross_lags=None, *, per_series: Sequence[str] = ("moments", "acf")) -> SeriesDependence:
    """The features of every series of X (n, T, C) and their set means.  `per_series` names the per-series arrays to return (the
    set means are always computed; the ccf array is n (cross_lags + 1) C^2 floats, so it is off by default)."""
    n, T, Cn = _series_shape(X)
    L, Lx = resolve_lags(T, Cn, lags, cross_lags)
    names = _check_per_series(per_series, Lx)
    F = 4 * Cn + L * Cn + (Lx + 1) * Cn * Cn
    if n * F >= 2 ** 31 or n * T * Cn >= 2 ** 31:
        raise ValueError(f"too large: n * F = {n * F} and n * T * C = {n * T * Cn} must stay below 2^31")
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X))
    if not isinstance(X, torch.Tensor):
        raise _C.FdError("X must be a torch.Tensor or a numpy array")
    if X.device.type != "cuda":
        if not torch.cuda.is_available():
            raise _C.FdError("series_dependence runs on the HIP engine and no GPU is visible (no CPU fallback)")
        X = X.to("cuda")
    xt = _C.dev_f32(X.detach(), "X")
    lib = _C.lib()
    dev = xt.device
    moments = torch.empty((n, Cn, 4), dtype=torch.float32, device=dev) if "moments" in names else None
    acf = torch.empty((n, L, Cn), dtype=torch.float32, device=dev) if "acf" in names and L >= 1 else None
    ccf = torch.empty((n, Lx + 1, Cn, Cn), dtype=torch.float32, device=dev) if "ccf" in names else None
    mean = torch.empty((F,), dtype=torch.float64, device=dev)
    call_with_workspace(xt, lib.fd_series_dependence_workspace_bytes, (n, T, Cn, L, Lx), lambda hd, work, nbytes, stream:
                        lib.fd_series_dependence(hd, xt.data_ptr(), n, T, Cn, L, Lx, _C.ptr(moments), _C.ptr(acf), _C.ptr(ccf),
                                                 mean.data_ptr(), work, nbytes, stream))
    if "acf" in names and acf is None:
        acf = torch.empty((n, 0, Cn), dtype=torch.float32, device=dev)
    a0, c0 = 4 * Cn, 4 * Cn + L * Cn
    set_mean = SetMean(moments=mean[:a0].view(Cn, 4), acf=mean[a0:c0].view(L, Cn),
                       ccf=mean[c0:].view(Lx + 1, Cn, Cn) if Lx >= 0 else None)
    return SeriesDependence(moments=moments, acf=acf, ccf=ccf, set_mean=set_mean, lags=L, cross_lags=Lx)
