"""How the channels of a series relate as a function of frequency, on the HIP engine (not in the reference): Welch's averaged
periodogram of every series -- the power spectral density of every channel, the cross-spectral density of every channel pair and
three summaries of each channel's spectrum -- plus their means over the set, from which the set-level coherence and phase follow.

Conventions are scipy.signal.welch / csd's at fs = 1, scaling = "density", one-sided.  For one series x (T, C), segments of
S = nperseg points at 0, H, 2 H, ... (H = nperseg - noverlap) while start + S <= T (a tail is dropped), v = (segment - its mean) w:

    F[k, c]    = sum_s v[s, c] exp(-2 pi i k s / S),   k = 0..K-1,  K = S // 2 + 1,  f_k = k / S
    P[k, c, d] = scale_k / (nseg sum w^2) sum_seg conj(F[k, c]) F[k, d],    scale_k = 2, but 1 at k = 0 and at the Nyquist bin of an even S
    psd = the diagonal;  csd = the pairs c < d in row-major order, (Re, Im)
    summary[c] = (total power sum_k psd,  centroid sum f_k psd_k / sum psd_k,  entropy -sum p ln p / ln(K - 1)), the last two over
                 the bins k >= 1 (bin 0 holds only leakage after detrending)

A channel that is constant over a series has zeros everywhere it would divide, not NaN.  Everything runs in one fused kernel
(csrc/fd_spectral.hip, fd_series_spectra): a series is read once, the DFT is a product against a cached [cos | sin] basis on the
f32-input MFMA (any S: no radix), the (n, K, NP, 2) array is only written when it is asked for, and the set means are deterministic
(no atomics).  A series' features depend on that series alone."""
from __future__ import annotations

import operator
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _C
from ._pairs import call_with_workspace

MAX_LENGTH = 1024          # fd_series_spectra's own limits (csrc/fd_spectral.hip, SPEC_MAX_T / SPEC_MAX_C)
MAX_CHANNELS = 64
CHUNK_SERIES = 32          # series per partial sum of the set means (the engine's constant)
PER_SERIES = ("psd", "csd", "summary")
WINDOWS = ("hann", "boxcar")
DETRENDS = ("constant", None)
_WINDOW_CODE = {"boxcar": 0, "hann": 1}


def series_shape(x, what: str = "X") -> tuple[int, int, int]:
    """(n, T, C) of a non-empty array of series within the kernel's limits."""
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


def pair_indices(C: int) -> tuple[np.ndarray, np.ndarray]:
    """(c, d) of the C (C - 1) / 2 pairs c < d in the engine's row-major order."""
    return np.triu_indices(C, k=1)


@dataclass
class SetMean:
    psd: torch.Tensor                # (K, C) float64
    csd: torch.Tensor                # (K, C, C) complex128, Hermitian, filled from the pairs; its diagonal is psd
    summary: torch.Tensor            # (C, 3) float64

    def coherence(self) -> torch.Tensor:
        """(K, C, C) magnitude-squared coherence |P_cd|^2 / (P_cc P_dd) of the set-mean spectra, 0 where a denominator is 0.  It
        averages over n * n_segments segments, so it is meaningful with one segment per series."""
        den = self.psd[:, :, None] * self.psd[:, None, :]
        live = den > 0
        return torch.where(live, self.csd.abs() ** 2 / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(den))

    def phase(self) -> torch.Tensor:
        """(K, C, C) angle(P_cd): the lead of channel d over channel c at every bin, in radians."""
        return torch.angle(self.csd)


@dataclass
class SeriesSpectra:
    psd: Optional[torch.Tensor]      # (n, K, C) float32
    csd: Optional[torch.Tensor]      # (n, K, NP, 2) float32: Re / Im of the pairs c < d
    summary: Optional[torch.Tensor]  # (n, C, 3) float32: total power, spectral centroid, spectral entropy
    set_mean: SetMean                # the mean over the n series of every feature
    freqs: torch.Tensor              # (K,) float64, cycles per sample
    nperseg: int
    noverlap: int
    n_segments: int


def resolve_segments(T: int, nperseg=None, noverlap=None) -> tuple[int, int]:
    """(nperseg, noverlap) as the engine takes them.  nperseg=None: T for T < 32, else T // 2; noverlap=None: nperseg // 2."""
    if T < 2:
        raise ValueError(f"a series of T={T} points has no spectrum: T must be at least 2")
    S = (T if T < 32 else T // 2) if nperseg is None else _index("nperseg", nperseg, 2, T, f" (T for T={T})")
    ov = S // 2 if noverlap is None else _index("noverlap", noverlap, 0, S - 1, f" (nperseg - 1 for nperseg={S})")
    return S, ov


def check_options(window, detrend, per_series: Sequence[str], C: int) -> tuple[str, ...]:
    """The names of `per_series` as a tuple, after checking them, `window` and `detrend`."""
    if not isinstance(window, str) or window not in WINDOWS:
        raise ValueError(f"window={window!r}: one of {WINDOWS}")
    if detrend not in DETRENDS:
        raise ValueError(f"detrend={detrend!r}: one of {DETRENDS}")
    if isinstance(per_series, str):
        per_series = (per_series,)
    names = tuple(per_series)
    for name in names:
        if name not in PER_SERIES:
            raise ValueError(f"per_series names {name!r}: one of {PER_SERIES}")
    if "csd" in names and C < 2:
        raise ValueError("per_series asks for 'csd' but one channel has no pairs")
    return names


def assemble_set_mean(mean: torch.Tensor, K: int, C: int) -> SetMean:
    """The SetMean of a flat (K C + 2 K NP + 3 C) float64 vector in the engine's order psd | csd | summary."""
    NP = C * (C - 1) // 2
    psd = mean[: K * C].view(K, C)
    full = torch.zeros((K, C, C), dtype=torch.complex128, device=mean.device)
    idx = torch.arange(C, device=mean.device)
    full[:, idx, idx] = psd.to(torch.complex128)
    if NP:
        parts = mean[K * C: K * C + 2 * K * NP].view(K, NP, 2)
        pairs = torch.complex(parts[..., 0].contiguous(), parts[..., 1].contiguous())
        c, d = (torch.from_numpy(i).to(mean.device) for i in pair_indices(C))
        full[:, c, d] = pairs
        full[:, d, c] = pairs.conj()
    return SetMean(psd=psd, csd=full, summary=mean[K * C + 2 * K * NP:].view(C, 3))


def series_spectra(X, nperseg=None, noverlap=None, *, window: str = "hann", detrend: Optional[str] = "constant",
                   per_series: Sequence[str] = ("psd", "summary")) -> SeriesSpectra:
    """The spectra of every series of X (n, T, C) and their set means.  `per_series` names the per-series arrays to return (the set
    means are always computed; the csd array is n K C (C - 1) floats, so it is off by default)."""
    n, T, Cn = series_shape(X)
    S, ov = resolve_segments(T, nperseg, noverlap)
    names = check_options(window, detrend, per_series, Cn)
    K, NP = S // 2 + 1, Cn * (Cn - 1) // 2
    F = K * Cn + 2 * K * NP + 3 * Cn
    if n * F >= 2 ** 31 or n * T * Cn >= 2 ** 31:
        raise ValueError(f"too large: n * F = {n * F} and n * T * C = {n * T * Cn} must stay below 2^31")
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X))
    if not isinstance(X, torch.Tensor):
        raise _C.FdError("X must be a torch.Tensor or a numpy array")
    if X.device.type != "cuda":
        if not torch.cuda.is_available():
            raise _C.FdError("series_spectra runs on the HIP engine and no GPU is visible (no CPU fallback)")
        X = X.to("cuda")
    xt = _C.dev_f32(X.detach(), "X")
    lib = _C.lib()
    dev = xt.device
    psd = torch.empty((n, K, Cn), dtype=torch.float32, device=dev) if "psd" in names else None
    csd = torch.empty((n, K, NP, 2), dtype=torch.float32, device=dev) if "csd" in names else None
    summary = torch.empty((n, Cn, 3), dtype=torch.float32, device=dev) if "summary" in names else None
    mean = torch.empty((F,), dtype=torch.float64, device=dev)
    wcode, dcode = _WINDOW_CODE[window], 1 if detrend == "constant" else 0
    call_with_workspace(xt, lib.fd_series_spectra_workspace_bytes, (n, T, Cn, S, ov), lambda hd, work, nbytes, stream:
                        lib.fd_series_spectra(hd, xt.data_ptr(), n, T, Cn, S, ov, wcode, dcode, _C.ptr(psd), _C.ptr(csd),
                                              _C.ptr(summary), mean.data_ptr(), work, nbytes, stream))
    freqs = torch.arange(K, dtype=torch.float64, device=dev) / S
    return SeriesSpectra(psd=psd, csd=csd, summary=summary, set_mean=assemble_set_mean(mean, K, Cn), freqs=freqs, nperseg=S,
                         noverlap=ov, n_segments=(T - S) // (S - ov) + 1)
