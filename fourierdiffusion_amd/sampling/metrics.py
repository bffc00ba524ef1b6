"""Evaluation metrics -- same surface as fdiff.sampling.metrics (reference: src/fdiff/sampling/metrics.py:13-217):
`Metric`, `MetricCollection`, `SlicedWasserstein`, `MarginalWasserstein`, same constructor arguments, same result keys.
The distances run on the HIP engine (utils/wasserstein.py); results are plain Python floats / lists as in the reference.

Not in the reference: `PrecisionRecall` and `Memorisation`, nearest-neighbour metrics in sample space (utils/neighbours.py), which
see what a projection-based distance cannot -- a generator that replays its training set, or one that covers a single mode; and
`KernelTwoSample`, the kernel two-sample test (utils/two_sample.py), which puts a p-value on "can the samples be told apart from
real data at this sample size"; and `DTWPrecisionRecall` / `DTWMemorisation`, the two nearest-neighbour metrics under banded dynamic
time warping (utils/dtw.py), which see a training series replayed a few samples early or late as the copy it is; and
`SinkhornDivergence`, the debiased entropic transport cost between the two sets in their full sample space (utils/sinkhorn.py): the
Wasserstein-2 distance that the sliced metric stands in for; and `TemporalDependence`, the first metric that looks INSIDE a series
(utils/dependence.py): differences of the mean autocorrelation, of the mean cross-correlation between channels and of the skewness
and kurtosis between the samples and the real set; and `DiscriminativeScore` / `PredictiveScore`, the two post-hoc scores of TimeGAN
and TSGBench (utils/posthoc.py): a small causal LSTM trained on the engine after the fact, to tell the samples from real series, and
to forecast real series after training on the samples; and `ClassificationScore`, the first metric that reads a LABEL (TSTR / TRTS
classification accuracy, utils/posthoc.py): a K-way classifier trained after the fact on the samples with the classes they were drawn
for and tested on real series, and the other way round; and `SignatureDistance`, the first metric that reads the ORDER of events inside a
series (utils/signature.py): Sig-W1 and the signature MMD between the expected path signatures of the two sets."""
from __future__ import annotations

import inspect
from abc import ABC, abstractmethod
from functools import partial
from typing import Any, Optional

import numpy as np
import torch

from ..utils.dependence import _series_shape as _dependence_shape
from ..utils.dependence import resolve_lags, series_dependence
from ..utils.dtw import _series_shape, _window, dtw_ball_counts, dtw_knn
from ..utils.fourier import dft, spectral_density
from ..utils.neighbours import MAX_K, ball_counts, knn
from ..utils.posthoc import MAX_CLASSES as POSTHOC_MAX_CLASSES
from ..utils.posthoc import MAX_D_MODEL as POSTHOC_MAX_D_MODEL
from ..utils.posthoc import discriminative_score, fit_classifier, predictive_score
from ..utils.signature import _series_shape as signature_shape
from ..utils.signature import check_options as signature_options
from ..utils.signature import expected_signature_distance, series_signature
from ..utils.sinkhorn import DEFAULT_REG, sinkhorn_divergence
from ..utils.spectral import check_options as spectral_options
from ..utils.spectral import pair_indices, resolve_segments, series_spectra
from ..utils.spectral import series_shape as spectral_shape
from ..utils.tensors import check_flat_array
from ..utils.two_sample import DEFAULT_SCALES, MAX_COLUMNS, _check_scales, mmd_permutation_test
from ..utils.wasserstein import WassersteinDistances


class Metric(ABC):
    views = ("time", "freq")          # the representations a MetricCollection binds the class in

    def __init__(self, original_samples: np.ndarray | torch.Tensor) -> None:
        self.original_samples = check_flat_array(original_samples)

    @abstractmethod
    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]: ...

    @property
    @abstractmethod
    def name(self) -> str: ...

    @property
    def baseline_metrics(self) -> dict[str, float]:
        return {}


def _as_tensor(x) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x


def _takes_holdout(make: partial) -> bool:
    return "holdout_samples" in inspect.signature(make.func).parameters


def _takes_labels(make: partial) -> bool:
    return "original_labels" in inspect.signature(make.func).parameters


def subsample_indices(n: int, size: int, seed: int) -> np.ndarray:
    """`size` of the n row indices, drawn without replacement from numpy's Generator(seed), ascending."""
    return np.sort(np.random.default_rng(seed).choice(n, size=size, replace=False))


class _View:
    """One representation of the samples a collection evaluates in: a key prefix, the map from time-domain samples into the
    representation, and the metrics bound to the ORIGINAL samples in that representation."""

    def __init__(self, prefix: str, transform, metrics: list) -> None:
        self.prefix, self.transform, self.metrics = prefix, transform, metrics

    def _prefixed(self, results) -> dict[str, Any]:
        return {f"{self.prefix}_{key}": val for res in results for key, val in res.items()}

    def evaluate(self, samples: torch.Tensor, labels=None) -> dict[str, Any]:
        if not self.metrics:
            return {}
        mapped = self.transform(samples)
        # the labels go only to the metrics that say they read them
        return self._prefixed(m(mapped, labels) if getattr(m, "needs_labels", False) else m(mapped) for m in self.metrics)

    def baselines(self) -> dict[str, Any]:
        return self._prefixed(m.baseline_metrics for m in self.metrics)


class MetricCollection:
    """Same surface and result keys as the reference's collection (metrics.py:28-99): every partially instantiated metric is bound
    to the original samples once per view its class names in `views` (every class of the reference: both) -- `time` (the samples as
    they are) and `freq` (their dft) -- and, on request, a marginal
    Wasserstein on the spectral densities forms a third view (`spectral`, seed 42, all distances kept, no baselines).  A call
    returns the union of the views' results (+ the time / freq baselines) sorted by key.

    `holdout_samples` (not in the reference): real samples the model was not trained on, mapped into each view like the original
    samples and handed to the metrics whose class takes them (`Memorisation`); without it nothing changes.

    `original_labels` / `holdout_labels` (not in the reference): the class of every original / held-out sample, handed to the metrics
    whose class takes `original_labels` (`ClassificationScore`); such a metric gets the held-out samples only together with their
    labels.  A call passes `other_labels`, the classes the samples were drawn for, to the metrics with `needs_labels` set and to no
    other: a collection without one returns the same with and without labels."""

    def __init__(self, metrics: list, original_samples: Optional[np.ndarray | torch.Tensor] = None,
                 include_baselines: bool = True, include_spectral_density: bool = False,
                 holdout_samples: Optional[np.ndarray | torch.Tensor] = None, original_labels=None, holdout_labels=None) -> None:
        factories = [m for m in metrics if isinstance(m, partial)]      # (like the reference, only partials are taken up)
        if factories and original_samples is None:
            raise AssertionError("Original samples must be provided for the metrics to be instantiated.")
        original = _as_tensor(original_samples) if original_samples is not None else None
        holdout = _as_tensor(holdout_samples) if holdout_samples is not None and len(holdout_samples) > 0 else None
        self._views = [_View("time", lambda x: x, []), _View("freq", dft, [])]
        for view in self._views:
            wanted = [make for make in factories if view.prefix in getattr(make.func, "views", Metric.views)]
            if wanted:
                bound_to = view.transform(original)
                held = view.transform(holdout) if holdout is not None else None
                for make in wanted:
                    extra: dict[str, Any] = {}
                    labelled = _takes_labels(make)
                    if labelled:
                        extra["original_labels"] = original_labels
                    if held is not None and _takes_holdout(make) and (not labelled or holdout_labels is not None):
                        extra["holdout_samples"] = held
                        if labelled:
                            extra["holdout_labels"] = holdout_labels
                    view.metrics.append(make(**extra, original_samples=bound_to))
        self.include_baselines = include_baselines
        self.metric_spectral = None
        self._spectral_view = None
        if include_spectral_density:
            self.metric_spectral = MarginalWasserstein(original_samples=spectral_density(original), random_seed=42,
                                                       save_all_distances=True)
            self._spectral_view = _View("spectral", spectral_density, [self.metric_spectral])

    # the reference's attribute names for the two bound lists
    @property
    def metrics_time(self) -> list:
        return self._views[0].metrics

    @property
    def metrics_freq(self) -> list:
        return self._views[1].metrics

    def __call__(self, other_samples: np.ndarray | torch.Tensor, other_labels=None) -> dict[str, Any]:
        samples = _as_tensor(other_samples)
        merged: dict[str, Any] = {}
        for view in self._views:
            merged.update(view.evaluate(samples, other_labels))
        if self.include_baselines:
            merged.update(self.baseline_metrics)
        if self._spectral_view is not None:
            merged.update(self._spectral_view.evaluate(samples))
        return {key: merged[key] for key in sorted(merged)}

    @property
    def baseline_metrics(self) -> dict[str, float]:
        merged: dict[str, float] = {}
        for view in self._views:
            merged.update(view.baselines())
        return merged


class _WassersteinMetric(Metric):
    kind = ""

    def _distances(self, original: torch.Tensor, other: torch.Tensor) -> np.ndarray:
        raise NotImplementedError

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        distances = self._distances(self.original_samples, check_flat_array(other_samples))
        metrics: dict[str, Any] = {f"{self.kind}_wasserstein_mean": float(np.mean(distances)),
                                   f"{self.kind}_wasserstein_max": float(np.max(distances))}
        if self.save_all_distances:
            metrics[f"{self.kind}_wasserstein_all"] = distances.tolist()
        return metrics

    @property
    def baseline_metrics(self) -> dict[str, float]:
        n_samples = self.original_samples.shape[0]
        # two folds of the original samples against each other (metrics.py:129-137)
        distances_self = self._distances(self.original_samples[: n_samples // 2].contiguous(),
                                         self.original_samples[n_samples // 2:].contiguous())
        # a generator that only outputs the average sample (metrics.py:139-147); the mean is a host-side reduction
        avg_sample = self.original_samples.mean(dim=0, keepdim=True)
        distances_dummy = self._distances(self.original_samples, avg_sample)
        return {f"{self.kind}_wasserstein_mean_self": float(np.mean(distances_self)),
                f"{self.kind}_wasserstein_max_self": float(np.max(distances_self)),
                f"{self.kind}_wasserstein_mean_dummy": float(np.mean(distances_dummy)),
                f"{self.kind}_wasserstein_max_dummy": float(np.max(distances_dummy))}

    @property
    def name(self) -> str:
        return f"{self.kind}_wasserstein"


class SlicedWasserstein(_WassersteinMetric):
    """metrics.py:100-160."""
    kind = "sliced"

    def __init__(self, original_samples: np.ndarray | torch.Tensor, random_seed: int, num_directions: int,
                 save_all_distances: bool = False) -> None:
        super().__init__(original_samples=original_samples)
        self.random_seed = random_seed
        self.num_directions = num_directions
        self.save_all_distances = save_all_distances

    def _distances(self, original, other):
        return WassersteinDistances(original_data=original, other_data=other, seed=self.random_seed).sliced_distances(
            self.num_directions)


class MarginalWasserstein(_WassersteinMetric):
    """metrics.py:163-217."""
    kind = "marginal"

    def __init__(self, original_samples: np.ndarray | torch.Tensor, random_seed: int, save_all_distances: bool = False) -> None:
        super().__init__(original_samples=original_samples)
        self.random_seed = random_seed
        self.save_all_distances = save_all_distances

    def _distances(self, original, other):
        return WassersteinDistances(original_data=original, other_data=other, seed=self.random_seed).marginal_distances()


class PrecisionRecall(Metric):
    """Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) of generated samples G
    against the real samples R in sample space.  NND_k(x) is the distance from x to its k-th nearest neighbour in its OWN set:
      precision  mean_i 1[count_i > 0], count_i = #{j : d(g_i, r_j) <= NND_k(r_j)}    density  sum_i count_i / (k |G|)
      recall     the same with the roles of R and G swapped                           coverage mean_j 1[min_i d(r_j, g_i) <= NND_k(r_j)]
    `max_original` evaluates against a seeded subsample of the real set."""

    def __init__(self, original_samples: np.ndarray | torch.Tensor, k: int = 5, max_original: Optional[int] = None,
                 random_seed: int = 0) -> None:
        if int(k) != k or not 1 <= k <= MAX_K:
            raise ValueError(f"k={k} must be an integer in [1, {MAX_K}]")
        if max_original is not None and (int(max_original) != max_original or max_original <= k):
            raise ValueError(f"max_original={max_original} must be an integer above k={k}")
        if len(original_samples) <= k:
            raise ValueError(f"{len(original_samples)} original samples cannot supply k={k} neighbours of a sample in its own set")
        super().__init__(original_samples=original_samples)
        self.k, self.max_original, self.random_seed = int(k), max_original, random_seed
        n = self.original_samples.shape[0]
        if max_original is not None and n > max_original:
            keep = torch.from_numpy(subsample_indices(n, int(max_original), random_seed)).to(self.original_samples.device)
            self.original_samples = self.original_samples[keep].contiguous()

    # the two distance primitives (flat (n, d) device rows in, as utils/neighbours.py): what a subclass under another distance swaps
    def _knn(self, queries: torch.Tensor, references: torch.Tensor, k: int, exclude_self: bool = False):
        return knn(queries, references, k, exclude_self=exclude_self)

    def _ball_counts(self, queries: torch.Tensor, references: torch.Tensor, radii: torch.Tensor) -> torch.Tensor:
        return ball_counts(queries, references, radii)

    def _radii(self, samples: torch.Tensor) -> torch.Tensor:
        return self._knn(samples, samples, self.k, exclude_self=True)[0][:, self.k - 1].contiguous()

    def _evaluate(self, real: torch.Tensor, generated: torch.Tensor) -> dict[str, float]:
        if generated.shape[0] <= self.k:
            raise ValueError(f"{generated.shape[0]} samples cannot supply k={self.k} neighbours of a sample in its own set")
        radii_real, radii_gen = self._radii(real), self._radii(generated)
        in_real = self._ball_counts(generated, real, radii_real)      # per generated sample: real balls it falls in
        in_gen = self._ball_counts(real, generated, radii_gen)
        nearest_gen = self._knn(real, generated, 1)[0][:, 0]
        return {"precision": float((in_real > 0).double().mean()),
                "recall": float((in_gen > 0).double().mean()),
                "density": float(in_real.sum()) / (self.k * generated.shape[0]),
                "coverage": float((nearest_gen <= radii_real).double().mean())}

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        return self._evaluate(self.original_samples, check_flat_array(other_samples))

    @property
    def baseline_metrics(self) -> dict[str, float]:
        n_samples = self.original_samples.shape[0]                    # two folds of the original samples, as the Wasserstein metrics
        if n_samples // 2 <= self.k:
            return {}
        folds = self._evaluate(self.original_samples[: n_samples // 2].contiguous(),
                               self.original_samples[n_samples // 2:].contiguous())
        return {f"{key}_self": val for key, val in folds.items()}

    @property
    def name(self) -> str:
        return "precision_recall"


class Memorisation(Metric):
    """Does the generator copy its training set?  With d_i the distance from sample g_i to its nearest training row r_j*:
      authenticity        share of samples with d_i > NND_1(r_j*) (Alaa et al. 2022): a copy sits nearer to a training row than that
                          row's own nearest training neighbour does
      nn_distance_min / nn_distance_median   of the d_i
      train_closer_share  (with `holdout_samples`) share of samples strictly nearer to the training set than to the held-out set,
                          ties one half; the training set is subsampled (seeded) to the held-out set's size when it is larger.
                          About 0.5: nothing memorised; towards 1: samples sit on training rows."""

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 random_seed: int = 0) -> None:
        if len(original_samples) < 2:
            raise ValueError("Memorisation needs at least two original samples")
        if holdout_samples is not None and len(holdout_samples) < 1:
            raise ValueError("holdout_samples is empty")
        super().__init__(original_samples=original_samples)
        self.random_seed = random_seed
        self.holdout_samples = self.train_subset = None
        if holdout_samples is not None:
            self.holdout_samples = check_flat_array(holdout_samples)
            if self.holdout_samples.shape[1] != self.original_samples.shape[1]:
                raise ValueError("original and held-out samples must have the same number of features")
            n, h = self.original_samples.shape[0], self.holdout_samples.shape[0]
            self.train_subset = self.original_samples
            if n > h:
                keep = torch.from_numpy(subsample_indices(n, h, random_seed)).to(self.original_samples.device)
                self.train_subset = self.original_samples[keep].contiguous()

    def _knn(self, queries: torch.Tensor, references: torch.Tensor, k: int, exclude_self: bool = False):
        """The distance primitive (flat (n, d) device rows in): what a subclass under another distance swaps."""
        return knn(queries, references, k, exclude_self=exclude_self)

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        samples = check_flat_array(other_samples)
        dist, nearest = self._knn(samples, self.original_samples, 1)
        dist, nearest = dist[:, 0], nearest[:, 0]
        own = self._knn(self.original_samples, self.original_samples, 1, exclude_self=True)[0][:, 0]
        host = dist.double().cpu().numpy()
        out = {"authenticity": float((dist > own[nearest]).double().mean()),
               "nn_distance_min": float(host.min()), "nn_distance_median": float(np.median(host))}
        if self.holdout_samples is not None:
            to_train = self._knn(samples, self.train_subset, 1)[0][:, 0]
            to_held = self._knn(samples, self.holdout_samples, 1)[0][:, 0]
            out["train_closer_share"] = float((to_train < to_held).double().mean() + 0.5 * (to_train == to_held).double().mean())
        return out

    @property
    def name(self) -> str:
        return "memorisation"


class _DTWDistance:
    """Mixin of the two DTW metrics: takes the series shape (T, C) from the original samples BEFORE the base class flattens them,
    resolves the window, and answers the base class's distance hooks with utils/dtw.py on the rows folded back to (n, T, C).  Result
    keys get the prefix `dtw_`.  Warping a spectrum is meaningless: bound in the time view only."""
    views = ("time",)

    def _take_shape(self, original_samples, window) -> None:
        if len(tuple(original_samples.shape)) != 3:
            raise ValueError(f"{type(self).__name__} needs the original samples as (n, T, C) series, got shape "
                             f"{tuple(original_samples.shape)}: a flat (n, d) array has lost its time axis")
        _, T, C = _series_shape(original_samples, "original samples")
        self.series_shape, self.window = (T, C), _window(window, T)

    def _fold(self, rows: torch.Tensor) -> torch.Tensor:
        T, C = self.series_shape
        if rows.dim() != 2 or rows.shape[1] != T * C:
            raise ValueError(f"samples of {tuple(rows.shape[1:])} features, the original samples are series of shape {(T, C)}")
        return rows.view(rows.shape[0], T, C)

    def _knn(self, queries, references, k, exclude_self=False):
        q = self._fold(queries)
        return dtw_knn(q, q if references is queries else self._fold(references), k, window=self.window, exclude_self=exclude_self)

    def _ball_counts(self, queries, references, radii):
        return dtw_ball_counts(self._fold(queries), self._fold(references), radii, window=self.window)


def _dtw_keys(results: dict[str, Any]) -> dict[str, Any]:
    return {f"dtw_{key}": val for key, val in results.items()}


class DTWPrecisionRecall(_DTWDistance, PrecisionRecall):
    """`PrecisionRecall` with every distance replaced by banded dynamic time warping (utils/dtw.py; `window`: an integer, None =
    ceil(0.1 T), or "full"): small phase jitter no longer costs precision or recall.  Same formulas and arguments; keys
    dtw_precision, dtw_recall, dtw_density, dtw_coverage and their `_self` baselines.  Needs (n, T, C) original samples."""

    def __init__(self, original_samples: np.ndarray | torch.Tensor, k: int = 5, max_original: Optional[int] = None,
                 random_seed: int = 0, window=None) -> None:
        self._take_shape(original_samples, window)
        super().__init__(original_samples=original_samples, k=k, max_original=max_original, random_seed=random_seed)

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        return _dtw_keys(super().__call__(other_samples))

    @property
    def baseline_metrics(self) -> dict[str, float]:
        return _dtw_keys(super().baseline_metrics)

    @property
    def name(self) -> str:
        return "dtw_precision_recall"


class DTWMemorisation(_DTWDistance, Memorisation):
    """`Memorisation` under banded dynamic time warping: a training series replayed a few samples early or late is found next to
    its source row, where the Euclidean nearest neighbour is usually another row and the replay passes for authentic.  Same
    formulas and arguments plus `window`; keys dtw_authenticity, dtw_nn_distance_min, dtw_nn_distance_median and (with a holdout)
    dtw_train_closer_share.  Needs (n, T, C) original samples."""

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 random_seed: int = 0, window=None) -> None:
        self._take_shape(original_samples, window)
        super().__init__(original_samples=original_samples, holdout_samples=holdout_samples, random_seed=random_seed)

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        return _dtw_keys(super().__call__(other_samples))

    @property
    def name(self) -> str:
        return "dtw_memorisation"


class KernelTwoSample(Metric):
    """Kernel two-sample test (Gretton et al. 2012) of the generated samples against real ones: the unbiased MMD^2 under a Gaussian
    kernel mixture (bandwidths `scales` times the pooled mean squared pair distance) and the p-value of `n_permutations`
    permutations of the pooled rows.
      mmd2, mmd_p_value                  against the original samples
      mmd2_holdout, mmd_p_value_holdout  (with `holdout_samples`) against real samples the model was not trained on
      mmd2_self, mmd_p_value_self        (baseline) the two folds of the original samples against each other
    A small p-value: the two sets can be told apart at this sample size.  `max_original` evaluates against a seeded subsample of the
    real set."""

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 n_permutations: int = 200, scales=DEFAULT_SCALES, max_original: Optional[int] = None, random_seed: int = 0) -> None:
        if isinstance(n_permutations, bool) or int(n_permutations) != n_permutations or not 1 <= n_permutations < MAX_COLUMNS:
            raise ValueError(f"n_permutations={n_permutations} must be an integer in [1, {MAX_COLUMNS - 1}]")
        if max_original is not None and (int(max_original) != max_original or max_original < 2):
            raise ValueError(f"max_original={max_original} must be an integer >= 2")
        if len(original_samples) < 2:
            raise ValueError("KernelTwoSample needs at least two original samples")
        if holdout_samples is not None and len(holdout_samples) < 2:
            raise ValueError("KernelTwoSample needs at least two held-out samples")
        self.scales = _check_scales(scales)
        super().__init__(original_samples=original_samples)
        self.n_permutations, self.max_original, self.random_seed = int(n_permutations), max_original, random_seed
        n = self.original_samples.shape[0]
        if max_original is not None and n > max_original:
            keep = torch.from_numpy(subsample_indices(n, int(max_original), random_seed)).to(self.original_samples.device)
            self.original_samples = self.original_samples[keep].contiguous()
        self.holdout_samples = None
        if holdout_samples is not None:
            self.holdout_samples = check_flat_array(holdout_samples)
            if self.holdout_samples.shape[1] != self.original_samples.shape[1]:
                raise ValueError("original and held-out samples must have the same number of features")

    def _test(self, samples: torch.Tensor, real: torch.Tensor, suffix: str) -> dict[str, float]:
        res = mmd_permutation_test(samples, real, n_permutations=self.n_permutations, scales=self.scales, seed=self.random_seed)
        return {f"mmd2{suffix}": float(res.mmd2), f"mmd_p_value{suffix}": float(res.p_value)}

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        samples = check_flat_array(other_samples)
        out = self._test(samples, self.original_samples, "")
        if self.holdout_samples is not None:
            out.update(self._test(samples, self.holdout_samples, "_holdout"))
        return out

    @property
    def baseline_metrics(self) -> dict[str, float]:
        n_samples = self.original_samples.shape[0]                    # two folds of the original samples, as the Wasserstein metrics
        if n_samples // 2 < 2:
            return {}
        return self._test(self.original_samples[: n_samples // 2].contiguous(), self.original_samples[n_samples // 2:].contiguous(),
                          "_self")

    @property
    def name(self) -> str:
        return "kernel_two_sample"


class SinkhornDivergence(Metric):
    """Debiased Sinkhorn divergence (Genevay et al. 2018, Feydy et al. 2019) of the generated samples against real ones, cost
    ||x - y||^2 on the flat rows, eps = `reg` times the mean squared distance over the pooled pairs:
      sinkhorn_divergence, sinkhorn_w2, sinkhorn_marginal_error    against the original samples
      ..._holdout                                                  (with `holdout_samples`) against real samples the model was not
                                                                   trained on
      ..._self                                                     (baseline) the two folds of the original samples
    sinkhorn_w2 = sqrt(max(divergence, 0)) estimates the Wasserstein-2 distance of the two sets in sample space; the marginal
    error says how far the iteration was from convergence (0: converged).  `max_original` evaluates against a seeded subsample of
    the real set."""

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 reg: float = DEFAULT_REG, max_original: Optional[int] = None, random_seed: int = 0) -> None:
        if isinstance(reg, bool) or not (np.isfinite(float(reg)) and float(reg) > 0):
            raise ValueError(f"reg={reg} must be finite and > 0")
        if max_original is not None and (int(max_original) != max_original or max_original < 2):
            raise ValueError(f"max_original={max_original} must be an integer >= 2")
        if len(original_samples) < 1:
            raise ValueError("SinkhornDivergence needs at least one original sample")
        if holdout_samples is not None and len(holdout_samples) < 1:
            raise ValueError("SinkhornDivergence needs at least one held-out sample")
        super().__init__(original_samples=original_samples)
        self.reg, self.max_original, self.random_seed = float(reg), max_original, random_seed
        n = self.original_samples.shape[0]
        if max_original is not None and n > max_original:
            keep = torch.from_numpy(subsample_indices(n, int(max_original), random_seed)).to(self.original_samples.device)
            self.original_samples = self.original_samples[keep].contiguous()
        self.holdout_samples = None
        if holdout_samples is not None:
            self.holdout_samples = check_flat_array(holdout_samples)
            if self.holdout_samples.shape[1] != self.original_samples.shape[1]:
                raise ValueError("original and held-out samples must have the same number of features")

    def _divergence(self, samples: torch.Tensor, real: torch.Tensor, suffix: str) -> dict[str, float]:
        res = sinkhorn_divergence(samples, real, reg=self.reg)
        return {f"sinkhorn_divergence{suffix}": float(res.divergence), f"sinkhorn_w2{suffix}": float(res.w2),
                f"sinkhorn_marginal_error{suffix}": float(res.marginal_error)}

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        samples = check_flat_array(other_samples)
        out = self._divergence(samples, self.original_samples, "")
        if self.holdout_samples is not None:
            out.update(self._divergence(samples, self.holdout_samples, "_holdout"))
        return out

    @property
    def baseline_metrics(self) -> dict[str, float]:
        n_samples = self.original_samples.shape[0]                    # two folds of the original samples, as the Wasserstein metrics
        if n_samples // 2 < 1:
            return {}
        return self._divergence(self.original_samples[: n_samples // 2].contiguous(),
                                self.original_samples[n_samples // 2:].contiguous(), "_self")

    @property
    def name(self) -> str:
        return "sinkhorn_divergence"


class TemporalDependence(Metric):
    """Does the generator reproduce the dependence structure inside a series?  Per series the normalised autocorrelation (lags
    1..`lags`), the normalised cross-correlation of every ordered channel pair (lags 0..`cross_lags`) and the skewness and excess
    kurtosis of every channel (utils/dependence.py); then, between the samples and the real set,
      acf_distance, acf_distance_max            mean / max over (lag, channel) of |mean ACF of the samples - mean ACF of the real set|
                                                (the autocorrelation difference of TSGBench)
      ccf_distance, ccf_distance_max            the same over (lag, c != d): the correlational score; omitted for one channel
      skewness_distance, kurtosis_distance      mean over channels of the absolute difference of the set means
      acf_marginal_wasserstein_mean, _max       Wasserstein-2 per (lag, channel) between the DISTRIBUTIONS of the per-series ACF
                                                values (MarginalWasserstein's arithmetic on the (n, lags C) feature rows)
      ..._holdout                               (with `holdout_samples`) against real series the model was not trained on
      ..._self                                  (baseline) the two folds of the original samples
    `lags=None` is max(1, T // 4), `cross_lags=None` is min(lags, 8).  `max_original` evaluates against a seeded subsample of the real
    set.  The real set's features are computed once, here.  Needs (n, T, C) original samples; a spectrum's "time" axis has no
    autocorrelation worth the name: bound in the time view only."""
    views = ("time",)

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 lags: Optional[int] = None, cross_lags: Optional[int] = None, max_original: Optional[int] = None,
                 random_seed: int = 0) -> None:
        if len(tuple(original_samples.shape)) != 3:
            raise ValueError(f"TemporalDependence needs the original samples as (n, T, C) series, got shape "
                             f"{tuple(original_samples.shape)}: a flat (n, d) array has lost its time axis")
        _, T, C = _dependence_shape(original_samples, "original samples")
        self.series_shape = (T, C)
        self.lags, self.cross_lags = resolve_lags(T, C, lags, cross_lags)
        if max_original is not None and (isinstance(max_original, bool) or int(max_original) != max_original or max_original < 2):
            raise ValueError(f"max_original={max_original} must be an integer >= 2")
        if len(original_samples) < 1:
            raise ValueError("TemporalDependence needs at least one original sample")
        if holdout_samples is not None:
            if len(holdout_samples) < 1:
                raise ValueError("TemporalDependence needs at least one held-out sample")
            if int(np.prod(tuple(holdout_samples.shape)[1:])) != T * C:
                raise ValueError("original and held-out samples must have the same number of features")
        super().__init__(original_samples=original_samples)
        self.max_original, self.random_seed = max_original, random_seed
        n = self.original_samples.shape[0]
        if max_original is not None and n > max_original:
            keep = torch.from_numpy(subsample_indices(n, int(max_original), random_seed)).to(self.original_samples.device)
            self.original_samples = self.original_samples[keep].contiguous()
            n = int(max_original)
        self._real = self._features(self.original_samples)
        self._held = self._features(check_flat_array(holdout_samples)) if holdout_samples is not None else None
        self._folds = None
        if n // 2 >= 1:
            self._folds = (self._features(self.original_samples[: n // 2].contiguous()),
                           self._features(self.original_samples[n // 2:].contiguous()))
        self._baseline: Optional[dict[str, float]] = None

    def _features(self, rows: torch.Tensor):
        T, C = self.series_shape
        if rows.dim() != 2 or rows.shape[1] != T * C:
            raise ValueError(f"samples of {tuple(rows.shape[1:])} features, the original samples are series of shape {(T, C)}")
        return series_dependence(rows.view(rows.shape[0], T, C), lags=self.lags, cross_lags=self.cross_lags, per_series=("acf",))

    def _compare(self, samples, real, suffix: str) -> dict[str, float]:
        C = self.series_shape[1]
        out: dict[str, float] = {}
        if self.lags >= 1:
            d = (samples.set_mean.acf - real.set_mean.acf).abs().cpu().numpy()
            out[f"acf_distance{suffix}"], out[f"acf_distance_max{suffix}"] = float(d.mean()), float(d.max())
        if C > 1 and real.set_mean.ccf is not None:
            d = (samples.set_mean.ccf - real.set_mean.ccf).abs().cpu().numpy()
            d = d[:, ~np.eye(C, dtype=bool)]
            out[f"ccf_distance{suffix}"], out[f"ccf_distance_max{suffix}"] = float(d.mean()), float(d.max())
        d = (samples.set_mean.moments - real.set_mean.moments).abs().cpu().numpy()
        out[f"skewness_distance{suffix}"], out[f"kurtosis_distance{suffix}"] = float(d[:, 2].mean()), float(d[:, 3].mean())
        if self.lags >= 1:
            w = WassersteinDistances(original_data=real.acf.reshape(real.acf.shape[0], -1),
                                     other_data=samples.acf.reshape(samples.acf.shape[0], -1), seed=self.random_seed).marginal_distances()
            out[f"acf_marginal_wasserstein_mean{suffix}"] = float(np.mean(w))
            out[f"acf_marginal_wasserstein_max{suffix}"] = float(np.max(w))
        return out

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        samples = self._features(check_flat_array(other_samples))
        out = self._compare(samples, self._real, "")
        if self._held is not None:
            out.update(self._compare(samples, self._held, "_holdout"))
        return out

    @property
    def baseline_metrics(self) -> dict[str, float]:
        if self._folds is None:
            return {}
        if self._baseline is None:                                    # two folds of the original samples, as the Wasserstein metrics
            self._baseline = self._compare(self._folds[0], self._folds[1], "_self")
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "temporal_dependence"


class SpectralDependence(Metric):
    """Does the generator reproduce how the channels relate as a function of frequency?  Per series Welch's power spectral density of
    every channel, the cross-spectral density of every channel pair and each channel's spectral centroid and entropy
    (utils/spectral.py); then, between the samples and the real set,
      psd_log_distance, psd_log_distance_max    mean / max over (bin >= 1, channel) of |10 log10(mean PSD of the samples / mean PSD of the
                                                real set)|, in dB; each set-mean PSD floored at 1e-12 of the channel's mean total power
      coherence_distance, coherence_distance_max  mean / max over (bin >= 1, c < d) of the absolute difference of the SET-LEVEL
                                                magnitude-squared coherences |P_cd|^2 / (P_cc P_dd); omitted for one channel
      phase_distance                            sum w |wrap(phase of the samples - phase of the real set)| / sum w over the same entries,
                                                w the real set's coherence (radians); omitted for one channel or when sum w = 0
      spectral_centroid_wasserstein, spectral_entropy_wasserstein   mean over channels of the Wasserstein-2 distance between the
                                                DISTRIBUTIONS of the per-series values (MarginalWasserstein's arithmetic)
      ..._holdout                               (with `holdout_samples`) against real series the model was not trained on
      ..._self                                  (baseline) the two folds of the original samples
    The set-level coherence averages over n * n_segments segments, so one segment per series (nperseg = T) is meaningful: a coupling
    at a lag longer than TemporalDependence's cross lags, or one confined to a band, shows here.  `nperseg=None` is T for T < 32, else
    T // 2; `noverlap=None` is nperseg // 2; `window` is "hann" or "boxcar".  `max_original` evaluates against a seeded subsample of
    the real set.  The real set's features are computed once, here.  Needs (n, T, C) original samples: bound in the time view only."""
    views = ("time",)

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 nperseg: Optional[int] = None, noverlap: Optional[int] = None, window: str = "hann",
                 max_original: Optional[int] = None, random_seed: int = 0) -> None:
        if len(tuple(original_samples.shape)) != 3:
            raise ValueError(f"SpectralDependence needs the original samples as (n, T, C) series, got shape "
                             f"{tuple(original_samples.shape)}: a flat (n, d) array has lost its time axis")
        _, T, C = spectral_shape(original_samples, "original samples")
        self.series_shape = (T, C)
        self.nperseg, self.noverlap = resolve_segments(T, nperseg, noverlap)
        spectral_options(window, "constant", (), C)
        self.window = window
        if max_original is not None and (isinstance(max_original, bool) or int(max_original) != max_original or max_original < 2):
            raise ValueError(f"max_original={max_original} must be an integer >= 2")
        if len(original_samples) < 1:
            raise ValueError("SpectralDependence needs at least one original sample")
        if holdout_samples is not None:
            if len(holdout_samples) < 1:
                raise ValueError("SpectralDependence needs at least one held-out sample")
            if int(np.prod(tuple(holdout_samples.shape)[1:])) != T * C:
                raise ValueError("original and held-out samples must have the same number of features")
        super().__init__(original_samples=original_samples)
        self.max_original, self.random_seed = max_original, random_seed
        n = self.original_samples.shape[0]
        if max_original is not None and n > max_original:
            keep = torch.from_numpy(subsample_indices(n, int(max_original), random_seed)).to(self.original_samples.device)
            self.original_samples = self.original_samples[keep].contiguous()
            n = int(max_original)
        self._real = self._features(self.original_samples)
        self._held = self._features(check_flat_array(holdout_samples)) if holdout_samples is not None else None
        self._folds = None
        if n // 2 >= 1:
            self._folds = (self._features(self.original_samples[: n // 2].contiguous()),
                           self._features(self.original_samples[n // 2:].contiguous()))
        self._baseline: Optional[dict[str, float]] = None

    def _features(self, rows: torch.Tensor):
        T, C = self.series_shape
        if rows.dim() != 2 or rows.shape[1] != T * C:
            raise ValueError(f"samples of {tuple(rows.shape[1:])} features, the original samples are series of shape {(T, C)}")
        return series_spectra(rows.view(rows.shape[0], T, C), nperseg=self.nperseg, noverlap=self.noverlap, window=self.window,
                              per_series=("summary",))

    def _compare(self, samples, real, suffix: str) -> dict[str, float]:
        C = self.series_shape[1]
        out: dict[str, float] = {}
        ps, pr = (torch.maximum(f.set_mean.psd, 1e-12 * f.set_mean.summary[:, 0][None, :]).cpu().numpy()[1:] for f in (samples, real))
        live = (ps > 0) & (pr > 0)                                    # a channel that is constant in a whole set has no spectrum
        d = np.where(live, np.abs(10.0 * np.log10(np.where(live, ps, 1.0) / np.where(live, pr, 1.0))), 0.0)
        out[f"psd_log_distance{suffix}"], out[f"psd_log_distance_max{suffix}"] = float(d.mean()), float(d.max())
        if C > 1:
            c, e = pair_indices(C)
            cs, cr = (f.set_mean.coherence().cpu().numpy()[1:, c, e] for f in (samples, real))
            d = np.abs(cs - cr)
            out[f"coherence_distance{suffix}"], out[f"coherence_distance_max{suffix}"] = float(d.mean()), float(d.max())
            dphi = (samples.set_mean.phase() - real.set_mean.phase()).cpu().numpy()[1:, c, e]
            dphi = np.abs((dphi + np.pi) % (2 * np.pi) - np.pi)
            if cr.sum() > 0:
                out[f"phase_distance{suffix}"] = float((cr * dphi).sum() / cr.sum())
        for i, name in ((1, "spectral_centroid_wasserstein"), (2, "spectral_entropy_wasserstein")):
            w = WassersteinDistances(original_data=real.summary[:, :, i], other_data=samples.summary[:, :, i],
                                     seed=self.random_seed).marginal_distances()
            out[f"{name}{suffix}"] = float(np.mean(w))
        return out

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        samples = self._features(check_flat_array(other_samples))
        out = self._compare(samples, self._real, "")
        if self._held is not None:
            out.update(self._compare(samples, self._held, "_holdout"))
        return out

    @property
    def baseline_metrics(self) -> dict[str, float]:
        if self._folds is None:
            return {}
        if self._baseline is None:                                    # two folds of the original samples, as the Wasserstein metrics
            self._baseline = self._compare(self._folds[0], self._folds[1], "_self")
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "spectral_dependence"


class SignatureDistance(Metric):
    """Does the generator reproduce the ORDER of events inside a series?  The path signature of every series (utils/signature.py): the
    iterated integrals up to `depth` of the path through its points -- level 2 holds the Levy areas (which channel leads which), the
    levels above asymmetries in time that no autocorrelation, spectrum or marginal sees (a series played backwards keeps all three).
    Between the samples and the real set,
      sig_w1            ||E S(samples) - E S(real)||_2, the Sig-W1 distance of Ni et al. 2021
      sig_w1_levels     the same norm level by level (a list of `depth` values)
      sig_mmd2          the unbiased MMD^2 under the linear kernel on signatures (Chevyrev & Oberhauser): it can be slightly negative
      ..._holdout       (with `holdout_samples`) against real series the model was not trained on
      ..._self          (baseline) the two folds of the original samples
    `time_augment` appends a time channel (without it the signature does not see the speed along the path), `basepoint` starts every
    path at 0 so that the starting value counts, `lead_lag` doubles the channels into lead and lag copies (the quadratic variation
    shows at level 2); `path_scale` multiplies every channel.  With `standardise` every set is centred and scaled per channel by the
    pooled mean and 1 / deviation of the ORIGINAL samples, computed once here in float64; a constant channel gets scale 0 and
    contributes exact zeros.  The real set's signature statistics are computed once, here.  No p-value is computed:
    `mmd_permutation_test(sig_a, sig_b)` on the feature rows of `series_signature(..., per_series=("sig",))` already gives one.
    Needs (n, T, C) original samples: bound in the time view only."""
    views = ("time",)

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 depth: int = 3, time_augment: bool = True, basepoint: bool = False, lead_lag: bool = False, path_scale: float = 1.0,
                 standardise: bool = True) -> None:
        if len(tuple(original_samples.shape)) != 3:
            raise ValueError(f"SignatureDistance needs the original samples as (n, T, C) series, got shape "
                             f"{tuple(original_samples.shape)}: a flat (n, d) array has lost its time axis")
        n, T, C = signature_shape(original_samples, "original samples")
        self.series_shape = (T, C)
        self.depth, self.d, self.features = signature_options(n, C, depth, time_augment, lead_lag)
        self.time_augment, self.basepoint, self.lead_lag = bool(time_augment), bool(basepoint), bool(lead_lag)
        self.path_scale, self.standardise = path_scale, bool(standardise)
        if holdout_samples is not None:
            if len(holdout_samples) < 1:
                raise ValueError("SignatureDistance needs at least one held-out sample")
            if int(np.prod(tuple(holdout_samples.shape)[1:])) != T * C:
                raise ValueError("original and held-out samples must have the same number of features")
        super().__init__(original_samples=original_samples)
        self.channel_offset = self.channel_scale = None
        if self.standardise:
            x = self.original_samples.cpu().numpy().astype(np.float64).reshape(-1, C)
            self.channel_offset = x.mean(axis=0)
            sd = x.std(axis=0)
            self.channel_scale = np.where(sd > 0, 1.0 / np.where(sd > 0, sd, 1.0), 0.0)
        self._real = self._features(self.original_samples)
        self._held = self._features(check_flat_array(holdout_samples)) if holdout_samples is not None else None
        self._folds = None
        if n // 2 >= 1:
            self._folds = (self._features(self.original_samples[: n // 2].contiguous()),
                           self._features(self.original_samples[n // 2:].contiguous()))
        self._baseline: Optional[dict[str, Any]] = None

    def _features(self, rows: torch.Tensor):
        T, C = self.series_shape
        if rows.dim() != 2 or rows.shape[1] != T * C:
            raise ValueError(f"samples of {tuple(rows.shape[1:])} features, the original samples are series of shape {(T, C)}")
        return series_signature(rows.view(rows.shape[0], T, C), depth=self.depth, time_augment=self.time_augment,
                                basepoint=self.basepoint, lead_lag=self.lead_lag, channel_offset=self.channel_offset,
                                channel_scale=self.channel_scale, path_scale=self.path_scale)

    @staticmethod
    def _compare(samples, real, suffix: str) -> dict[str, Any]:
        return {f"{key}{suffix}": val for key, val in expected_signature_distance(samples, real).items()}

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        samples = self._features(check_flat_array(other_samples))
        out = self._compare(samples, self._real, "")
        if self._held is not None:
            out.update(self._compare(samples, self._held, "_holdout"))
        return out

    @property
    def baseline_metrics(self) -> dict[str, Any]:
        if self._folds is None:
            return {}
        if self._baseline is None:                                    # two folds of the original samples, as the Wasserstein metrics
            self._baseline = self._compare(self._folds[0], self._folds[1], "_self")
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "signature_distance"


class _PosthocScore(Metric):
    """What the two post-hoc scores share (utils/posthoc.py): (n, T, C) original samples, the knobs of the network and its training,
    the rows of a flat array seen as series again."""
    views = ("time",)

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 steps: int = 2000, batch_size: int = 128, lr: float = 1e-3, d_model: int = 32, num_layers: int = 1,
                 max_samples: int = 10_000, random_seed: int = 0) -> None:
        who = type(self).__name__
        if len(tuple(original_samples.shape)) != 3:
            raise ValueError(f"{who} needs the original samples as (n, T, C) series, got shape {tuple(original_samples.shape)}: a "
                             "flat (n, d) array has lost its time axis")
        T, C = (int(v) for v in tuple(original_samples.shape)[1:])
        self.series_shape = (T, C)
        if len(original_samples) < 2:
            raise ValueError(f"{who} needs at least two original samples")
        if holdout_samples is not None:
            if len(holdout_samples) < 2:
                raise ValueError(f"{who} needs at least two held-out samples")
            if int(np.prod(tuple(holdout_samples.shape)[1:])) != T * C:
                raise ValueError("original and held-out samples must have the same number of features")
        if d_model % 2 != 0 or not 2 <= d_model <= POSTHOC_MAX_D_MODEL:
            raise ValueError(f"d_model={d_model} must be even and <= {POSTHOC_MAX_D_MODEL}, the widest LSTM the engine trains")
        super().__init__(original_samples=original_samples)
        self.holdout_samples = check_flat_array(holdout_samples) if holdout_samples is not None else None
        self.random_seed = random_seed
        self.knobs = dict(steps=steps, batch_size=batch_size, lr=lr, d_model=d_model, num_layers=num_layers, max_samples=max_samples)
        self._baseline: Optional[dict[str, float]] = None

    def _series(self, rows: torch.Tensor) -> torch.Tensor:
        T, C = self.series_shape
        if rows.dim() != 2 or rows.shape[1] != T * C:
            raise ValueError(f"samples of {tuple(rows.shape[1:])} features, the original samples are series of shape {(T, C)}")
        return rows.view(rows.shape[0], T, C)

    def _folds(self) -> tuple[torch.Tensor, torch.Tensor]:
        real = self._series(self.original_samples)
        return real[: real.shape[0] // 2], real[real.shape[0] // 2:]


class DiscriminativeScore(_PosthocScore):
    """Can a classifier trained after the fact tell the samples from real series (TimeGAN / TSGBench)?  A small causal LSTM is
    trained on the engine to separate the two sets, standardised with the real set's statistics, and tested on rows it has not seen:
      discriminative_score, discriminative_accuracy   |accuracy - 0.5| and the accuracy, samples against the original samples
      ..._holdout                                     (with `holdout_samples`) against real series the model was not trained on
      discriminative_score_self                       (baseline) two folds of the original samples against each other: about 0
    One training run per key pair, `steps` AdamW steps of `batch_size`; deterministic given `random_seed`.  Needs (n, T, C) original
    samples; bound in the time view only."""

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 steps: int = 2000, batch_size: int = 128, lr: float = 1e-3, d_model: int = 32, num_layers: int = 1,
                 test_fraction: float = 0.2, max_samples: int = 10_000, random_seed: int = 0) -> None:
        if not 0.0 < test_fraction < 1.0:
            raise ValueError(f"test_fraction={test_fraction} must lie strictly between 0 and 1")
        super().__init__(original_samples=original_samples, holdout_samples=holdout_samples, steps=steps, batch_size=batch_size, lr=lr,
                         d_model=d_model, num_layers=num_layers, max_samples=max_samples, random_seed=random_seed)
        self.knobs["test_fraction"] = test_fraction

    def _score(self, real: torch.Tensor, other: torch.Tensor) -> dict:
        return discriminative_score(real, other, seed=self.random_seed, **self.knobs)

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        samples = self._series(check_flat_array(other_samples))
        res = self._score(self._series(self.original_samples), samples)
        out = {"discriminative_score": res["score"], "discriminative_accuracy": res["accuracy"]}
        if self.holdout_samples is not None:
            res = self._score(self._series(self.holdout_samples), samples)
            out.update(discriminative_score_holdout=res["score"], discriminative_accuracy_holdout=res["accuracy"])
        return out

    @property
    def baseline_metrics(self) -> dict[str, float]:
        if self._baseline is None:
            self._baseline = {"discriminative_score_self": self._score(*self._folds())["score"]}
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "discriminative_score"


class PredictiveScore(_PosthocScore):
    """Are the samples as useful as real data for forecasting ("train on synthetic, test on real", TimeGAN / TSGBench)?  A small
    causal LSTM is trained on the engine to forecast the next point of the SAMPLES and tested on real series; the score is its mean
    absolute one-step error in units of the real set's per-channel deviation:
      predictive_score            trained on the samples, tested on the original samples
      predictive_score_holdout    (with `holdout_samples`) the same, tested on real series the model was not trained on
      predictive_score_self       (baseline) trained on one fold of the original samples, tested on the other
    Deterministic given `random_seed`.  Needs (n, T, C) original samples with T >= 2; bound in the time view only."""

    def __init__(self, original_samples: np.ndarray | torch.Tensor, holdout_samples: Optional[np.ndarray | torch.Tensor] = None,
                 steps: int = 2000, batch_size: int = 128, lr: float = 1e-3, d_model: int = 32, num_layers: int = 1,
                 max_samples: int = 10_000, random_seed: int = 0) -> None:
        super().__init__(original_samples=original_samples, holdout_samples=holdout_samples, steps=steps, batch_size=batch_size, lr=lr,
                         d_model=d_model, num_layers=num_layers, max_samples=max_samples, random_seed=random_seed)
        if self.series_shape[0] < 2:
            raise ValueError("PredictiveScore forecasts x[t + 1] from x[<= t] and needs series of at least 2 points")

    def _score(self, train_set: torch.Tensor, test_set: torch.Tensor) -> float:
        return predictive_score(train_set, test_set, stats_from=self._series(self.original_samples), seed=self.random_seed,
                                **self.knobs)["mae"]

    def __call__(self, other_samples: np.ndarray | torch.Tensor) -> dict[str, Any]:
        samples = self._series(check_flat_array(other_samples))
        out = {"predictive_score": self._score(samples, self._series(self.original_samples))}
        if self.holdout_samples is not None:
            out["predictive_score_holdout"] = self._score(samples, self._series(self.holdout_samples))
        return out

    @property
    def baseline_metrics(self) -> dict[str, float]:
        if self._baseline is None:
            self._baseline = {"predictive_score_self": self._score(*self._folds())}
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "predictive_score"


def _label_array(labels, n: int, what: str) -> np.ndarray:
    y = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if y.dtype == np.bool_ or not np.issubdtype(y.dtype, np.integer):
        raise ValueError(f"{what} must be integer classes, got dtype {y.dtype}")
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError(f"{what} of shape {tuple(y.shape)} for {n} samples: one class per sample")
    if n and y.min() < 0:
        raise ValueError(f"{what} must not be negative")
    return y.astype(np.int64)


class ClassificationScore(_PosthocScore):
    """Do the samples of a class look like that class (TSTR / TRTS: RCGAN, Esteban et al. 2017; the classification accuracy score of
    Ravuri & Vinyals 2019)?  A small causal LSTM with a K-way softmax head is trained on the engine after the fact:
      tstr_accuracy, tstr_balanced_accuracy   trained on the SAMPLES with the classes they were drawn for, tested on the original
                                              samples: drops when the samples of a class do not look like it, or cover it badly
      ..._holdout                             (with `holdout_samples` and `holdout_labels`) the same training, tested on real series
                                              the model was not trained on
      trts_accuracy, trts_balanced_accuracy   trained on the original samples (once per metric object), tested on the samples:
                                              label fidelity, also under guidance
      trtr_accuracy_self, trtr_balanced_accuracy_self   (baseline) trained on one real fold, tested on the other
    Balanced accuracy is the mean recall over the classes present in the test set.  `n_classes` defaults to the largest original
    label + 1; `balance=True` draws the training batches class by class.  A call takes the samples AND their classes
    (`needs_labels`); deterministic given `random_seed`.  Needs (n, T, C) original samples; bound in the time view only."""
    needs_labels = True

    def __init__(self, original_samples: np.ndarray | torch.Tensor, original_labels=None,
                 holdout_samples: Optional[np.ndarray | torch.Tensor] = None, holdout_labels=None, n_classes: Optional[int] = None,
                 balance: bool = False, steps: int = 2000, batch_size: int = 128, lr: float = 1e-3, d_model: int = 32,
                 num_layers: int = 1, max_samples: int = 10_000, random_seed: int = 0) -> None:
        # everything about the labels is checked before the samples move to the device
        if original_labels is None:
            raise ValueError("ClassificationScore needs original_labels, the class of every original sample (an unlabelled dataset "
                             "has no classification score)")
        labels = _label_array(original_labels, len(original_samples), "original_labels")
        if n_classes is None:
            n_classes = int(labels.max()) + 1
        if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 2 <= n_classes <= POSTHOC_MAX_CLASSES:
            raise ValueError(f"n_classes={n_classes} must be an integer from 2 to {POSTHOC_MAX_CLASSES} (by default the largest "
                             "original label + 1)")
        n_classes = int(n_classes)
        if labels.max() >= n_classes:
            raise ValueError(f"original_labels must lie in [0, {n_classes})")
        held_labels = None
        if holdout_samples is not None:
            if holdout_labels is None:
                raise ValueError("ClassificationScore got holdout_samples without holdout_labels")
            held_labels = _label_array(holdout_labels, len(holdout_samples), "holdout_labels")
            if held_labels.max() >= n_classes:
                raise ValueError(f"holdout_labels must lie in [0, {n_classes})")
        super().__init__(original_samples=original_samples, holdout_samples=holdout_samples, steps=steps, batch_size=batch_size, lr=lr,
                         d_model=d_model, num_layers=num_layers, max_samples=max_samples, random_seed=random_seed)
        self.original_labels, self.holdout_labels, self.n_classes = labels, held_labels, n_classes
        self.knobs["balance"] = bool(balance)
        self._real_classifier = None

    def _fit(self, train_set: torch.Tensor, train_labels: np.ndarray):
        return fit_classifier(train_set, train_labels, n_classes=self.n_classes, stats_from=self._series(self.original_samples),
                              seed=self.random_seed, **self.knobs)

    def __call__(self, other_samples: np.ndarray | torch.Tensor, other_labels=None) -> dict[str, Any]:
        if other_labels is None:
            raise ValueError("ClassificationScore needs other_labels, the classes the samples were drawn for: sample a "
                             "class-conditional model with sampler.labels set (a class, `balanced` or `data`) and pass the labels on")
        samples = self._series(check_flat_array(other_samples))
        labels = _label_array(other_labels, samples.shape[0], "other_labels")
        if labels.max() >= self.n_classes:
            raise ValueError(f"other_labels must lie in [0, {self.n_classes})")
        real = self._series(self.original_samples)
        on_samples = self._fit(samples, labels)
        res = on_samples.score(real, self.original_labels)
        out = {"tstr_accuracy": res["accuracy"], "tstr_balanced_accuracy": res["balanced_accuracy"]}
        if self.holdout_samples is not None:
            res = on_samples.score(self._series(self.holdout_samples), self.holdout_labels)
            out.update(tstr_accuracy_holdout=res["accuracy"], tstr_balanced_accuracy_holdout=res["balanced_accuracy"])
        if self._real_classifier is None:
            self._real_classifier = self._fit(real, self.original_labels)
        res = self._real_classifier.score(samples, labels)
        out.update(trts_accuracy=res["accuracy"], trts_balanced_accuracy=res["balanced_accuracy"])
        return out

    @property
    def baseline_metrics(self) -> dict[str, float]:
        if self._baseline is None:
            fold_a, fold_b = self._folds()
            half = fold_a.shape[0]
            res = self._fit(fold_a, self.original_labels[:half]).score(fold_b, self.original_labels[half:])
            self._baseline = {"trtr_accuracy_self": res["accuracy"], "trtr_balanced_accuracy_self": res["balanced_accuracy"]}
        return dict(self._baseline)

    @property
    def name(self) -> str:
        return "classification_score"
