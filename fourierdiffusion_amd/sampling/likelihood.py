"""Log-likelihood of series under the probability-flow ODE (an extension, not in the reference; Song et al. 2021, Sec. 4.3 and
App. D.2).  ``DiffusionSampler.log_likelihood`` runs the engine loop (fd_likelihood_run); this module holds the host pieces:
the result object, the drift part of the divergence integral, the change of variables to data space and bits per dimension.

    log p_0(x_0) = log p_1(x_1) + int_eps^1 div v(x(t), t) dt,   div v = -a(t) T C - 0.5 g(t)^2 tr(diag(G_k^2) ds/dx)

Sample space is what the score model sees: the series, through the packed DFT of ``utils.fourier`` when the model diffuses in the
frequency domain, then standardised by the training split's feature mean and std when the datamodule standardises.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

# estimator="exact" replicates every series over its T*C basis vectors: refused above this many dimensions per series
EXACT_MAX_DIMS = 1024
ESTIMATORS = ("rademacher", "gaussian", "exact")
# solver="rk45": the cap on score evaluations per row when the caller gives none (a row that would pass it stops, not converged)
RK45_MAX_EVALS = 20000


@dataclass
class LikelihoodResult:
    """Per-series results (CPU float64 tensors, shape (n,)) of ``DiffusionSampler.log_likelihood``, in sample space.

    log_prob = prior_log_prob + delta_log_prob; delta_log_prob = drift part + the mean over probes of the score part of the
    divergence integral.  latents: x_1 (n, T, C), float32.  std_err: the standard error of the probe mean (n_probes > 1, else
    None).  nfe: score evaluations per series (rk45: the maximum over its rows, counted as scipy's nfev; Euler / Heun: N / 2N).
    converged: bool per series (rk45: every row reached t = 1; a series that did not has log_prob NaN).  grid: rk45's accepted
    times per row, float64 (n, replicas, S), t = eps first, NaN-padded (None for Euler / Heun).  rtol / atol: rk45's tolerances.
    num_diffusion_steps is None for rk45."""
    log_prob: torch.Tensor
    prior_log_prob: torch.Tensor
    delta_log_prob: torch.Tensor
    latents: torch.Tensor
    std_err: Optional[torch.Tensor]
    estimator: str
    n_probes: int
    num_diffusion_steps: Optional[int]
    solver: str
    nfe: Optional[torch.Tensor] = None
    converged: Optional[torch.Tensor] = None
    grid: Optional[torch.Tensor] = None
    rtol: Optional[float] = None
    atol: Optional[float] = None

    def bits_per_dim(self, max_len: int, n_channels: int) -> torch.Tensor:
        return bits_per_dim(self.log_prob, max_len, n_channels)


def ode_weights(ts: Sequence[float], solver: str) -> list:
    """Quadrature of the solver on the grid ts (N + 1 points) as (t_j, w_j) pairs: Euler w = h_i at t_i; Heun h_i / 2 at t_i and
    t_{i+1} (its two stages)."""
    out = []
    for i in range(len(ts) - 1):
        t0, t1 = float(ts[i]), float(ts[i + 1])
        h = t1 - t0
        if solver == "euler":
            out.append((t0, h))
        else:
            out += [(t0, 0.5 * h), (t1, 0.5 * h)]
    return out


def drift_a(kind: int, p0: float, p1: float, t: float) -> float:
    """a(t) of the drift -a x: VP beta(t) / 2, VE 0 (as fd_sde_coef, in float64)."""
    return 0.5 * (p0 + t * (p1 - p0)) if kind == 0 else 0.0


def drift_integral(kind: int, p0: float, p1: float, t0: float, t1: float, dims: int) -> float:
    """The exact drift part of the divergence integral, -dims int_t0^t1 a(t) dt (float64; a is linear in t)."""
    if kind != 0:
        return 0.0
    return -dims * 0.5 * (p0 * (t1 - t0) + 0.5 * (p1 - p0) * (t1 * t1 - t0 * t0))


def drift_divergence(kind: int, p0: float, p1: float, ts: Sequence[float], solver: str, dims: int) -> float:
    """The drift part of the divergence integral, -dims * sum_j w_j a(t_j), over the solver's quadrature (float64)."""
    return -dims * math.fsum(w * drift_a(kind, p0, p1, t) for t, w in ode_weights(ts, solver))


def data_space_offset(max_len: int, n_channels: int, fourier_transform: bool,
                      feature_std: Optional[torch.Tensor] = None) -> float:
    """log |det d(sample) / d(series)| of the map from the series as the user holds them to sample space (float64):
    -sum log feature_std (standardisation) - [fourier_transform] C K log 2 with K = (T - 1) // 2.  The packed real DFT is not
    orthonormal: the Re / Im rows of the K interior frequencies have norm 1/sqrt(2)."""
    off = 0.0
    if feature_std is not None:
        std = feature_std.detach().to("cpu", torch.float64)
        if tuple(std.shape) != (max_len, n_channels):
            raise ValueError(f"feature_std must have shape {(max_len, n_channels)}, got {tuple(std.shape)}")
        if not bool((std > 0).all()):
            raise ValueError("feature_std must be positive")
        off -= float(torch.log(std).sum())
    if fourier_transform:
        off -= n_channels * ((max_len - 1) // 2) * math.log(2.0)
    return off


def to_data_space(log_prob: torch.Tensor, fourier_transform: bool, feature_std: Optional[torch.Tensor] = None, *,
                  max_len: Optional[int] = None, n_channels: Optional[int] = None) -> torch.Tensor:
    """Sample-space log densities (n,) -> log densities of the series as the user holds them (time domain, data scale):
    log p_data = log p_sample - sum_{t,c} log feature_std[t,c] - [fourier_transform] C ((T - 1) // 2) log 2.  feature_std: the
    (T, C) std the datamodule standardises with (None: not standardised; then max_len and n_channels give the shape)."""
    if feature_std is not None:
        max_len, n_channels = int(feature_std.shape[0]), int(feature_std.shape[1])
    if max_len is None or n_channels is None:
        raise ValueError("to_data_space: give feature_std or max_len and n_channels")
    return log_prob.to(torch.float64) + data_space_offset(max_len, n_channels, fourier_transform, feature_std)


def bits_per_dim(log_prob: torch.Tensor, max_len: int, n_channels: int) -> torch.Tensor:
    """-log p / (T C ln 2)."""
    return -log_prob.to(torch.float64) / (max_len * n_channels * math.log(2.0))
