"""Ensemble scores of probabilistic imputation / forecasting (an extension, not in the reference): the protocol of the diffusion
time-series literature (CSDI, TimeGrad, TSDiff) for ``DiffusionSampler.impute(..., num_samples=K)``.

``ensemble_scores`` runs the engine's per-entry kernel (fd_ensemble_scores: ensemble CRPS, linear sample quantiles, sample mean) in
chunks of series, once on the entries and once on the channel sums of the hidden entries, and ``aggregate`` reduces the per-entry
values over the hidden entries H (mask False) in float64.  ``aggregate`` is pure torch and runs on the CPU."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import torch

from .. import _C

DEFAULT_LEVELS = tuple(round(0.05 * i, 2) for i in range(1, 20))      # 0.05, 0.10, ..., 0.95
MAX_SAMPLES = 1024                                                      # the kernel's largest ensemble
CHUNK_BYTES = 1 << 28                                                   # samples of one kernel call (device memory bound)


@dataclass
class EnsembleScores:
    """Per-entry outputs of the kernel and their aggregates over the hidden entries.

    crps, mean: (n, T, C); quantiles: (L, n, T, C) at ``levels``; sum_crps (n, T), sum_quantiles (L, n, T): the same scores of
    the channel sums over the hidden channels (sum_truth (n, T) their truth, sum_mask (n, T) True where a channel is hidden);
    metrics: the aggregates of ``aggregate``."""
    levels: tuple
    crps: torch.Tensor
    quantiles: torch.Tensor
    mean: torch.Tensor
    sum_crps: torch.Tensor
    sum_quantiles: torch.Tensor
    sum_truth: torch.Tensor
    sum_mask: torch.Tensor
    metrics: Dict[str, float] = field(default_factory=dict)


def _check_levels(levels: Sequence[float]) -> tuple:
    lv = tuple(float(q) for q in levels)
    if not lv or any(not (0.0 <= q <= 1.0) for q in lv):
        raise ValueError(f"levels must be a non-empty sequence in [0, 1], got {levels}")
    for need in (0.05, 0.5, 0.95):
        if not any(abs(q - need) < 1e-12 for q in lv):
            raise ValueError(f"levels must include {need} (median and 90 % interval scores), got {lv}")
    return lv


def kernel_scores(samples: torch.Tensor, truth: torch.Tensor, levels: Sequence[float] = DEFAULT_LEVELS,
                  device: Optional[torch.device] = None):
    """(crps (n,T,C), quantiles (L,n,T,C), mean (n,T,C)) of fd_ensemble_scores on CPU float32, samples (n,K,T,C) and truth
    (n,T,C) anywhere; the kernel runs on ``device`` (default: the current CUDA device) in chunks of series."""
    if samples.dim() != 4 or truth.dim() != 3 or samples.shape[0] != truth.shape[0] or samples.shape[2:] != truth.shape[1:]:
        raise ValueError(f"samples (n, K, T, C) and truth (n, T, C) do not match: {tuple(samples.shape)}, {tuple(truth.shape)}")
    n, K, T, Cn = (int(v) for v in samples.shape)
    if not 1 <= K <= MAX_SAMPLES:
        raise ValueError(f"the ensemble size must lie in [1, {MAX_SAMPLES}], got {K}")
    lv = tuple(float(q) for q in levels)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    h = _C.ctx(dev)
    lv_d = torch.tensor(lv, dtype=torch.float64, device=dev)
    L = len(lv)
    crps, mean = torch.empty((n, T, Cn)), torch.empty((n, T, Cn))
    quant = torch.empty((L, n, T, Cn))
    step = max(1, CHUNK_BYTES // (4 * K * T * Cn))
    for lo in range(0, n, step):
        nb = min(step, n - lo)
        xs = _C.dev_f32(samples[lo:lo + nb].to(dev), "samples")
        y = _C.dev_f32(truth[lo:lo + nb].to(dev), "truth")
        oc, om = torch.empty((nb, T, Cn), device=dev), torch.empty((nb, T, Cn), device=dev)
        oq = torch.empty((L, nb, T, Cn), device=dev)
        rc = _C.lib().fd_ensemble_scores(h, xs.data_ptr(), y.data_ptr(), nb, K, T, Cn, lv_d.data_ptr(), L, oc.data_ptr(),
                                         oq.data_ptr(), om.data_ptr(), _C.stream_of(xs))
        _C.check(rc, h)
        crps[lo:lo + nb], mean[lo:lo + nb], quant[:, lo:lo + nb] = oc.cpu(), om.cpu(), oq.cpu()
    return crps, quant, mean


def channel_sums(samples: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor):
    """(sample sums (n,K,T,1), truth sums (n,T,1), sum mask (n,T)): per (series, t), the sums over the hidden channels, in float32
    (float64 accumulation); the mask is True where (series, t) has a hidden channel."""
    hid = ~mask.bool()
    xs = torch.where(hid[:, None], samples.double(), torch.zeros((), dtype=torch.float64)).sum(-1, keepdim=True)
    ys = torch.where(hid, truth.double(), torch.zeros((), dtype=torch.float64)).sum(-1, keepdim=True)
    return xs.float(), ys.float(), hid.any(-1)


def _quantile_crps(y: torch.Tensor, Q: torch.Tensor, levels: tuple) -> float:
    """CSDI's normalised quantile CRPS: (1/|L|) sum_q 2 sum_e |(y_e - Q_qe)(1{y_e <= Q_qe} - q)| / sum_e |y_e|; y (m,), Q (L, m)."""
    q = torch.tensor(levels, dtype=torch.float64)[:, None]
    loss = (2.0 * ((y[None] - Q) * ((y[None] <= Q).double() - q)).abs().sum(1)).mean()
    den = y.abs().sum()
    return float(loss / den) if float(den) > 0.0 else math.nan


def aggregate(truth: torch.Tensor, mask: torch.Tensor, crps: torch.Tensor, quantiles: torch.Tensor, mean: torch.Tensor,
              levels: Sequence[float], sum_truth: torch.Tensor, sum_quantiles: torch.Tensor, sum_mask: torch.Tensor) -> Dict[str, float]:
    """The aggregates over the hidden entries H (mask False), in float64; truth / mask / crps / mean (n,T,C), quantiles (L,n,T,C),
    sum_truth (n,T), sum_quantiles (L,n,T), sum_mask (n,T).  Keys: crps, crps_quantile, crps_sum_quantile, mae_median,
    rmse_median, mse_mean, coverage_90, width_90."""
    lv = _check_levels(levels)
    i05, i50, i95 = (min(range(len(lv)), key=lambda i: abs(lv[i] - q)) for q in (0.05, 0.5, 0.95))
    H = ~mask.bool()
    y = truth.double()[H]
    Q = quantiles.double()[:, H]
    med, lo, hi = Q[i50], Q[i05], Q[i95]
    ys = sum_truth.double()[sum_mask]
    Qs = sum_quantiles.double()[:, sum_mask]
    return {
        "crps": float(crps.double()[H].mean()),
        "crps_quantile": _quantile_crps(y, Q, lv),
        "crps_sum_quantile": _quantile_crps(ys, Qs, lv),
        "mae_median": float((y - med).abs().mean()),
        "rmse_median": float(((y - med) ** 2).mean().sqrt()),
        "mse_mean": float(((y - mean.double()[H]) ** 2).mean()),
        "coverage_90": float(((lo <= y) & (y <= hi)).double().mean()),
        "width_90": float((hi - lo).mean()),
    }


def ensemble_scores(samples: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor,
                    levels: Sequence[float] = DEFAULT_LEVELS, device: Optional[torch.device] = None) -> EnsembleScores:
    """Scores of an ensemble samples (n, K, T, C) against truth (n, T, C) over the hidden entries of mask (bool (n,T,C) or (T,C),
    True = observed), all in data scale and the time domain: the per-entry kernel on the entries and on the channel sums of the
    hidden entries (the kernel with C = 1), then ``aggregate``."""
    lv = _check_levels(levels)
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise ValueError(f"mask must be a bool tensor, got {getattr(mask, 'dtype', type(mask))}")
    mask = torch.broadcast_to(mask.cpu(), tuple(truth.shape))
    if not bool((~mask).any()):
        raise ValueError("the mask hides no entry: there is nothing to score")
    truth = truth.float().cpu()
    crps, quant, mean = kernel_scores(samples, truth, lv, device)
    xs, ys, smask = channel_sums(samples.cpu(), truth, mask)
    s_crps, s_quant, _ = kernel_scores(xs, ys, lv, device)
    s_crps, s_quant, ys = s_crps[..., 0], s_quant[..., 0], ys[..., 0]
    metrics = aggregate(truth, mask, crps, quant, mean, lv, ys, s_quant, smask)
    return EnsembleScores(levels=lv, crps=crps, quantiles=quant, mean=mean, sum_crps=s_crps, sum_quantiles=s_quant,
                          sum_truth=ys, sum_mask=smask, metrics=metrics)
