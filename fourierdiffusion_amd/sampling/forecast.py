"""Ensemble scores of probabilistic imputation / forecasting (an extension, not in the reference): the protocol of the diffusion
time-series literature (CSDI, TimeGrad, TSDiff) for ``DiffusionSampler.impute(..., num_samples=K)``.

``ensemble_scores`` runs the engine's per-entry kernel (fd_ensemble_scores: ensemble CRPS, linear sample quantiles, sample mean) in
chunks of series, once on the entries and once on the channel sums of the hidden entries, and ``aggregate`` reduces the per-entry
values over the hidden entries H (mask False) in float64.  ``aggregate`` is pure torch and runs on the CPU."""
from __future__ import annotations

import ctypes
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


# ------------------------------------------------------------------------------------------------------------------------------
# Multivariate scores (fd_energy_score, fd_variogram_score, fd_ensemble_ranks).  The scores above are marginal: they
# look at one entry's K values at a time, so an ensemble whose members were permuted independently at every entry scores the same
# as a coherent one.  The energy score and the variogram score see the joint draw, the rank histogram its calibration.
VARIOGRAM_ORDERS = {0.5: _C.FD_VARIOGRAM_HALF, 1.0: _C.FD_VARIOGRAM_ONE, 2.0: _C.FD_VARIOGRAM_TWO}
VARIOGRAM_WEIGHTS = ("inverse_lag", "uniform")


@dataclass
class MultivariateScores:
    """Per-series scores and the rank counts of an ensemble.

    energy, variogram (= variogram_num / variogram_den): float64 (n,), NaN where the score is not defined (no hidden entry; no
    pair of hidden entries within max_lag) or where a hidden entry holds a NaN; hidden: int32 (n,), the hidden entries per series;
    below, equal: int32 (n, T, C) of ``rank_counts``; rank_histogram: float64 (K + 1,); metrics: the aggregates."""
    energy: torch.Tensor
    variogram: torch.Tensor
    variogram_num: torch.Tensor
    variogram_den: torch.Tensor
    hidden: torch.Tensor
    below: torch.Tensor
    equal: torch.Tensor
    rank_histogram: torch.Tensor
    metrics: Dict[str, object] = field(default_factory=dict)


def _check_ensemble(samples, truth) -> tuple:
    if not isinstance(samples, torch.Tensor) or not isinstance(truth, torch.Tensor) or samples.dim() != 4 or truth.dim() != 3 \
            or samples.shape[0] != truth.shape[0] or samples.shape[2:] != truth.shape[1:]:
        raise ValueError("samples (n, K, T, C) and truth (n, T, C) do not match: "
                         f"{tuple(getattr(samples, 'shape', ()))}, {tuple(getattr(truth, 'shape', ()))}")
    n, K, T, Cn = (int(v) for v in samples.shape)
    if min(n, T, Cn) < 1:
        raise ValueError(f"samples (n, K, T, C) must not be empty, got {tuple(samples.shape)}")
    if not 1 <= K <= MAX_SAMPLES:
        raise ValueError(f"the ensemble size must lie in [1, {MAX_SAMPLES}], got {K}")
    return n, K, T, Cn


def _check_mask(mask, n: int, T: int, Cn: int) -> torch.Tensor:
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise ValueError(f"mask must be a bool tensor, got {getattr(mask, 'dtype', type(mask))}")
    if tuple(mask.shape) not in ((n, T, Cn), (T, Cn)):
        raise ValueError(f"mask must have shape {(n, T, Cn)} or {(T, Cn)}, got {tuple(mask.shape)}")
    return mask.cpu()


def _check_scale(scale, T: int, Cn: int) -> Optional[torch.Tensor]:
    if scale is None:
        return None
    try:
        sc = torch.broadcast_to(torch.as_tensor(scale, dtype=torch.float64).cpu(), (T, Cn))
    except (RuntimeError, TypeError, ValueError) as exc:
        raise ValueError(f"scale must broadcast to (T, C) = {(T, Cn)}: {exc}") from None
    if not bool((torch.isfinite(sc) & (sc > 0)).all()):
        raise ValueError("scale must be finite and positive everywhere")
    return sc.contiguous()


def _check_variogram(order, max_lag, weights) -> tuple:
    try:
        o = float(order)
    except (TypeError, ValueError):
        o = math.nan
    if o not in VARIOGRAM_ORDERS:
        raise ValueError(f"order must be one of 0.5, 1, 2, got {order}")
    if weights not in VARIOGRAM_WEIGHTS:
        raise ValueError(f"weights must be one of {VARIOGRAM_WEIGHTS}, got {weights!r}")
    if max_lag is not None and (int(max_lag) != max_lag or int(max_lag) < 0):
        raise ValueError(f"max_lag must be None (no limit) or an integer >= 0, got {max_lag}")
    return o, (None if max_lag is None else int(max_lag)), weights


def _run_multivariate(samples, truth, mask, scale, device, energy: Optional[dict], variogram: Optional[dict], ranks: bool) -> dict:
    """One pass over the series in chunks of CHUNK_BYTES of samples: every requested kernel runs on the chunk while it is on the
    device.  energy = {fair}, variogram = {order, max_lag, weights} (checked), or None.  All arguments are checked before the
    engine is touched.  The scores see samples / scale and truth / scale (float64 division, rounded once to fp32); the ranks see
    the data as it is."""
    n, K, T, Cn = _check_ensemble(samples, truth)
    if mask is not None or energy is not None or variogram is not None:
        mask = _check_mask(mask, n, T, Cn)
    sc = _check_scale(scale, T, Cn)
    if energy is not None and energy["fair"] and K < 2:
        raise ValueError("the fair energy score needs an ensemble of K >= 2 samples, got K = 1")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    h, L = _C.ctx(dev), _C.lib()
    per_series = mask is not None and mask.dim() == 3
    sc_d = None if sc is None else sc.to(dev)
    out = {}
    if energy is not None:
        out.update(energy=torch.empty(n, dtype=torch.float64), hidden=torch.empty(n, dtype=torch.int32))
    if variogram is not None:
        out.update(num=torch.empty(n, dtype=torch.float64), den=torch.empty(n, dtype=torch.float64))
        order, lag = VARIOGRAM_ORDERS[variogram["order"]], -1 if variogram["max_lag"] is None else min(variogram["max_lag"], T)
        inverse = 1 if variogram["weights"] == "inverse_lag" else 0
    if ranks:
        out.update(below=torch.empty((n, T, Cn), dtype=torch.int32), equal=torch.empty((n, T, Cn), dtype=torch.int32))
    need = ctypes.c_size_t(0)

    def workspace(rc):
        _C.check(rc, h)
        return torch.empty(max(1, need.value), dtype=torch.uint8, device=dev)

    step = max(1, CHUNK_BYTES // (4 * K * T * Cn))
    for lo in range(0, n, step):
        nb = min(step, n - lo)
        xs = _C.dev_f32(samples[lo:lo + nb].to(dev), "samples")
        y = _C.dev_f32(truth[lo:lo + nb].to(dev), "truth")
        stream = _C.stream_of(xs)
        if ranks:
            ob, oe = (torch.empty((nb, T, Cn), dtype=torch.int32, device=dev) for _ in range(2))
            _C.check(L.fd_ensemble_ranks(h, xs.data_ptr(), y.data_ptr(), nb, K, T, Cn, ob.data_ptr(), oe.data_ptr(), stream), h)
            out["below"][lo:lo + nb], out["equal"][lo:lo + nb] = ob.cpu(), oe.cpu()
        if energy is None and variogram is None:
            continue
        if sc_d is not None:
            xs, y = (xs.double() / sc_d).float(), (y.double() / sc_d).float()
        m8 = (mask[lo:lo + nb] if per_series else mask).to(torch.uint8).contiguous().to(dev)
        if energy is not None:
            work = workspace(L.fd_energy_score_workspace_bytes(h, nb, K, T, Cn, ctypes.byref(need)))
            oes, oh = torch.empty(nb, dtype=torch.float64, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)
            _C.check(L.fd_energy_score(h, xs.data_ptr(), y.data_ptr(), m8.data_ptr(), int(per_series), nb, K, T, Cn,
                                       int(bool(energy["fair"])), oes.data_ptr(), oh.data_ptr(), work.data_ptr(), work.numel(),
                                       stream), h)
            out["energy"][lo:lo + nb], out["hidden"][lo:lo + nb] = oes.cpu(), oh.cpu()
        if variogram is not None:
            work = workspace(L.fd_variogram_score_workspace_bytes(h, nb, K, T, Cn, lag, ctypes.byref(need)))
            on, od = (torch.empty(nb, dtype=torch.float64, device=dev) for _ in range(2))
            _C.check(L.fd_variogram_score(h, xs.data_ptr(), y.data_ptr(), m8.data_ptr(), int(per_series), nb, K, T, Cn, order, lag,
                                          inverse, on.data_ptr(), od.data_ptr(), None, work.data_ptr(), work.numel(), stream), h)
            out["num"][lo:lo + nb], out["den"][lo:lo + nb] = on.cpu(), od.cpu()
    return out


def energy_score(samples: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor, *, fair: bool = False, scale=None,
                 device: Optional[torch.device] = None) -> torch.Tensor:
    """Energy score per series over its hidden entries H (mask False), float64 (n,):
    (1/K) sum_k ||x_k - y||_H - 1/(2 K^2) sum_{j,k} ||x_j - x_k||_H, with 1/(2 K (K - 1)) when ``fair`` (K >= 2).  samples
    (n, K, T, C), truth (n, T, C), mask bool (n, T, C) or (T, C), True = observed.  ``scale`` broadcasts to (T, C) and divides
    samples and truth first: the norm mixes channels, so their units matter.  NaN for a series without a hidden entry or with a
    NaN at one."""
    return _run_multivariate(samples, truth, mask, scale, device, dict(fair=bool(fair)), None, False)["energy"]


def variogram_score(samples: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor, *, order: float = 0.5,
                    max_lag: Optional[int] = None, weights: str = "inverse_lag", scale=None,
                    device: Optional[torch.device] = None) -> torch.Tensor:
    """Variogram score of order p = ``order`` in {0.5, 1, 2} per series, float64 (n,): the weighted mean over the pairs a < b of
    hidden entries with |t_a - t_b| <= max_lag (None: every pair) of (|y_a - y_b|^p - (1/K) sum_k |x_ka - x_kb|^p)^2, weights
    1 / (1 + |t_a - t_b|) ("inverse_lag") or 1 ("uniform").  NaN for a series without such a pair or with a NaN at a hidden entry."""
    o, lag, w = _check_variogram(order, max_lag, weights)
    out = _run_multivariate(samples, truth, mask, scale, device, None, dict(order=o, max_lag=lag, weights=w), False)
    return out["num"] / out["den"]


def rank_counts(samples: torch.Tensor, truth: torch.Tensor, device: Optional[torch.device] = None):
    """(below, equal), int32 (n, T, C): for every entry the members below the truth and equal to it; -1 in both where the truth
    or a member is NaN."""
    out = _run_multivariate(samples, truth, None, None, device, None, None, True)
    return out["below"], out["equal"]


def rank_histogram(below: torch.Tensor, equal: torch.Tensor, mask: torch.Tensor, K: int) -> torch.Tensor:
    """Rank histogram over the hidden entries (mask False), float64 (K + 1,), summing to 1: the truth's rank among the K members
    is ``below`` plus a uniform draw from 0 .. ``equal`` under random tie-breaking, and every entry spreads its unit mass uniformly
    over those bins, which is that draw's expectation and deterministic.  Pure torch on the CPU.  NaN everywhere when no entry is
    hidden or a hidden entry is marked -1 (NaN data)."""
    K = int(K)
    if K < 1:
        raise ValueError(f"K must be >= 1, got {K}")
    if below.shape != equal.shape:
        raise ValueError(f"below and equal differ in shape: {tuple(below.shape)}, {tuple(equal.shape)}")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise ValueError(f"mask must be a bool tensor, got {getattr(mask, 'dtype', type(mask))}")
    H = ~torch.broadcast_to(mask.cpu(), tuple(below.shape))
    b, e = below.cpu()[H].long(), equal.cpu()[H].long()
    if b.numel() == 0 or bool((b < 0).any()) or bool((e < 0).any()):
        return torch.full((K + 1,), math.nan, dtype=torch.float64)
    if bool((b + e > K).any()):
        raise ValueError(f"below + equal exceeds K = {K}")
    share = 1.0 / (e.double() + 1.0)
    edge = torch.zeros(K + 2, dtype=torch.float64)
    edge.index_add_(0, b, share)                       # the mass enters at bin `below` ...
    edge.index_add_(0, b + e + 1, -share)              # ... and leaves behind bin `below + equal`
    return edge.cumsum(0)[:K + 1] / float(b.numel())


def reliability_index(hist: torch.Tensor) -> float:
    """sum_b |f_b - 1 / (K + 1)| of a rank histogram (Delle Monache et al. 2006): 0 for a flat one."""
    f = torch.as_tensor(hist, dtype=torch.float64)
    return float((f - 1.0 / f.numel()).abs().sum())


# ------------------------------------------------------------------------------------------------------------------------------
# Multivariate rank histograms (fd_multivariate_ranks).  The rank histogram above is per entry, so it too is blind to
# members permuted independently at every entry.  A pre-rank maps every point of a series (the truth and the K members) to one number
# that sees all of its hidden entries; the rank of the truth's pre-rank among the members' feeds the same histogram, one count per
# series.
PRERANKS = ("average", "band_depth", "dominance", "mst")
_PRERANK_KINDS = {"average": _C.FD_PRERANK_AVERAGE, "band_depth": _C.FD_PRERANK_BAND_DEPTH, "dominance": _C.FD_PRERANK_DOMINANCE,
                  "mst": _C.FD_PRERANK_MST}
MAX_RANKED_SAMPLES = 1023                                               # the truth is the 1024th point of a series


@dataclass
class MultivariateRanks:
    """prerank: float64 (n, K + 1), column 0 the truth's; below, equal: int32 (n,), the members whose pre-rank lies below the
    truth's / equals it; hidden: int32 (n,), the hidden entries per series.  A series with a NaN at a hidden entry has
    below = equal = -1 and pre-ranks -1 (NaN for "mst"); a series without a hidden entry has equal pre-ranks (below 0, equal K)."""
    prerank: torch.Tensor
    below: torch.Tensor
    equal: torch.Tensor
    hidden: torch.Tensor


def _check_prerank(kind) -> str:
    if kind not in PRERANKS:
        raise ValueError(f"kind must be one of {PRERANKS}, got {kind!r}")
    return kind


def multivariate_rank_counts(samples: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor, kind: str, *, scale=None,
                             device: Optional[torch.device] = None) -> MultivariateRanks:
    """Pre-ranks of the truth and of the K <= 1023 members of every series over its hidden entries (mask False), and the truth's
    rank among them.  kind: "average" (the sum over the hidden entries of the per-entry ranks), "band_depth" (the pairs of points
    whose band holds the point, summed likewise), "dominance" (the points that lie at or below the point at every hidden entry)
    or "mst" (the length of the Euclidean minimum spanning tree of the other points).  samples (n, K, T, C), truth (n, T, C),
    mask bool (n, T, C) or (T, C), True = observed.  ``scale`` broadcasts to (T, C) and divides samples and truth first, as in
    ``energy_score``: it matters for "mst" only, the other kinds are invariant under a positive scale per entry."""
    kind = _check_prerank(kind)
    n, K, T, Cn = _check_ensemble(samples, truth)
    if K > MAX_RANKED_SAMPLES:
        raise ValueError(f"the ensemble size must lie in [1, {MAX_RANKED_SAMPLES}] for multivariate ranks, got {K}")
    mask = _check_mask(mask, n, T, Cn)
    sc = _check_scale(scale, T, Cn)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    h, L = _C.ctx(dev), _C.lib()
    code = _PRERANK_KINDS[kind]
    per_series = mask.dim() == 3
    sc_d = None if sc is None else sc.to(dev)
    out = MultivariateRanks(prerank=torch.empty((n, K + 1), dtype=torch.float64), below=torch.empty(n, dtype=torch.int32),
                            equal=torch.empty(n, dtype=torch.int32), hidden=torch.empty(n, dtype=torch.int32))
    step = max(1, CHUNK_BYTES // (4 * K * T * Cn))
    if kind == "mst":                                                   # the (K + 1)^2 distances of a series live in the workspace
        step = max(1, min(step, CHUNK_BYTES // (8 * (K + 1) * (K + 1))))
    need = ctypes.c_size_t(0)
    for lo in range(0, n, step):
        nb = min(step, n - lo)
        xs = _C.dev_f32(samples[lo:lo + nb].to(dev), "samples")
        y = _C.dev_f32(truth[lo:lo + nb].to(dev), "truth")
        if sc_d is not None:
            xs, y = (xs.double() / sc_d).float(), (y.double() / sc_d).float()
        m8 = (mask[lo:lo + nb] if per_series else mask).to(torch.uint8).contiguous().to(dev)
        _C.check(L.fd_multivariate_ranks_workspace_bytes(h, code, nb, K, T, Cn, ctypes.byref(need)), h)
        work = torch.empty(max(1, need.value), dtype=torch.uint8, device=dev)
        pr = torch.empty((nb, K + 1), dtype=torch.float64, device=dev)
        ob, oe, oh = (torch.empty(nb, dtype=torch.int32, device=dev) for _ in range(3))
        _C.check(L.fd_multivariate_ranks(h, code, xs.data_ptr(), y.data_ptr(), m8.data_ptr(), int(per_series), nb, K, T, Cn,
                                         pr.data_ptr(), ob.data_ptr(), oe.data_ptr(), oh.data_ptr(), work.data_ptr(), work.numel(),
                                         _C.stream_of(xs)), h)
        out.prerank[lo:lo + nb], out.below[lo:lo + nb] = pr.cpu(), ob.cpu()
        out.equal[lo:lo + nb], out.hidden[lo:lo + nb] = oe.cpu(), oh.cpu()
    return out


def multivariate_rank_histogram(samples: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor,
                                kinds: Sequence[str] = PRERANKS[:2], *, scale=None,
                                device: Optional[torch.device] = None) -> Dict[str, dict]:
    """{kind: {"histogram": float64 (K + 1,), "reliability_index": float, "n_series_ranked": int}} of ``multivariate_rank_counts``:
    ``rank_histogram`` over the series that have a hidden entry, one count per series, ties spread uniformly.  NaN when no series
    has a hidden entry or one of them holds a NaN there."""
    if isinstance(kinds, str) or len(tuple(kinds)) == 0:
        raise ValueError(f"kinds must be a non-empty sequence out of {PRERANKS}, got {kinds!r}")
    kinds = tuple(_check_prerank(k) for k in kinds)
    K = int(samples.shape[1]) if isinstance(samples, torch.Tensor) and samples.dim() == 4 else 0
    out = {}
    for kind in kinds:
        r = multivariate_rank_counts(samples, truth, mask, kind, scale=scale, device=device)
        hist = rank_histogram(r.below, r.equal, r.hidden == 0, K)
        out[kind] = {"histogram": hist, "reliability_index": reliability_index(hist), "n_series_ranked": int((r.hidden > 0).sum())}
    return out


def _mean_where(v: torch.Tensor, defined: torch.Tensor) -> float:
    return float(v[defined].mean()) if bool(defined.any()) else math.nan


def multivariate_scores(samples: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor, *, fair: bool = False, order: float = 0.5,
                        max_lag: Optional[int] = None, weights: str = "inverse_lag", scale=None,
                        device: Optional[torch.device] = None) -> MultivariateScores:
    """Energy score, variogram score and rank histogram of an ensemble in one pass over the data (see ``energy_score``,
    ``variogram_score``, ``rank_counts``, ``rank_histogram``).  metrics: ``energy_score`` and ``variogram_score``, the means over
    the series where the score is defined (a hidden entry; a pair within max_lag) -- a series made NaN by NaN data is not dropped,
    it makes the mean NaN -- with ``n_series_scored_energy`` / ``n_series_scored_variogram``, ``rank_reliability_index``,
    ``rank_histogram`` (a list) and the options used."""
    o, lag, w = _check_variogram(order, max_lag, weights)
    out = _run_multivariate(samples, truth, mask, scale, device, dict(fair=bool(fair)), dict(order=o, max_lag=lag, weights=w), True)
    K = int(samples.shape[1])
    hist = rank_histogram(out["below"], out["equal"], mask, K)
    es, vs = out["energy"], out["num"] / out["den"]
    has_e, has_v = out["hidden"] > 0, out["den"] > 0
    metrics = {
        "energy_score": _mean_where(es, has_e),
        "variogram_score": _mean_where(vs, has_v),
        "n_series_scored_energy": int(has_e.sum()),
        "n_series_scored_variogram": int(has_v.sum()),
        "rank_reliability_index": reliability_index(hist),
        "rank_histogram": [float(v) for v in hist],
        "energy_fair": bool(fair),
        "variogram_order": o,
        "variogram_max_lag": lag,
        "variogram_weights": w,
    }
    return MultivariateScores(energy=es, variogram=vs, variogram_num=out["num"], variogram_den=out["den"], hidden=out["hidden"],
                              below=out["below"], equal=out["equal"], rank_histogram=hist, metrics=metrics)
