#!/usr/bin/env python3
"""python cmd/impute.py model_id=XYZ mask.kind=forecast mask.horizon=20 ... -- conditional sampling from a trained score model
(an extension, not in the reference): hides entries of the test split (mask.kind random / forecast), fills them in with
DiffusionSampler.impute on the MI355X engine, maps the result back to the time domain and writes imputations.pt (the test
split's shape) next to the checkpoint, with the MSE / MAE over the hidden entries under the key `impute` of results.yaml.
num_samples_per_series=K > 1 draws an ensemble of K samples per series instead: imputations.pt is (n, K, T, C) and results.yaml
holds the ensemble scores of sampling/forecast.py (CRPS, quantile CRPS and CRPS-sum, median errors, 90 % interval coverage) in
place of the MSE / MAE.  conditioning=dps (guidance.scale, guidance.jacobian) replaces the projection by gradient guidance; the three
keys are then recorded in the `impute` block.  conditioning=smc (smc.obs_std, smc.twist_scale, smc.ess_threshold, guidance.jacobian;
num_samples_per_series = K >= 2 particles) runs the twisted particle filter instead and adds `smc_log_evidence_mean`,
`smc_ess_final_mean` (final ESS / K), `smc_resamples_mean` (resamples per series) and `smc_unique_final_mean` (distinct final
ancestors / K).  labels=data|<int> (class-conditional models) conditions every series on its test label
(`datamodule.y_test`) or on one class, cfg_scale=w sets the classifier-free guidance scale; both are recorded only when set.
resample=r jump_length=j (conditioning=replace) turn on RePaint resampling: every block of j steps runs r times with a forward re-noise
between two runs, r * num_diffusion_steps score evaluations; both are recorded when they are not 1.  aggregate=w > 1 conditions on
WINDOW MEANS instead (temporal super-resolution): mask.* is read in windows of w time steps (mask.horizon counts windows), the
observation is the window means of the test split, every full-resolution entry counts as hidden in the scores, and results.yaml records
`aggregate` and `max_abs_err_window_means`, the largest deviation of the result's window means over the observed windows.
operator.kind=lowpass|moving_average|difference|gaussian_blur (with operator.n_freq / w / stride / sigma; sampling/masks.py) conditions
on a GENERAL LINEAR observation y = P x instead: mask.* counts rows of P (under conditioning=replace a random mask needs orthogonal rows:
lowpass), the observation is P applied to the test split, every full-resolution entry counts as hidden in the scores, and
results.yaml records `operator` (kind, its parameters, M and cond(P)) and `max_abs_err_operator`, the largest deviation of P applied
to the result from the observation over the observed rows.  Not with aggregate > 1, labels / cfg_scale, resample or conditioning=smc.
multivariate_scores=true (K > 1) adds the scores that see the joint draw (energy score, variogram score with the `variogram` block's
order / max_lag / weights, rank histogram and its reliability index), on channels divided by their standard deviation.
multivariate_ranks=[average,band_depth,dominance,mst] (any subset, K > 1) adds the multivariate rank histograms, one count per series:
`rank_histogram_<kind>`, `rank_reliability_index_<kind>` and `n_series_ranked`.  num_series=n keeps the first n test series.  With several processes (torch.distributed.run) the rows are sharded over the ranks, as cmd/sample.py shards its batches."""
from __future__ import annotations

import logging
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import yaml  # noqa: E402

from fourierdiffusion_amd import _rng  # noqa: E402
from fourierdiffusion_amd.config import compose, instantiate, load_yaml, save_yaml  # noqa: E402
from fourierdiffusion_amd.parallel import bind_device, init_process_group, shard_range  # noqa: E402
from fourierdiffusion_amd.sampling.forecast import PRERANKS, ensemble_scores, multivariate_rank_histogram, multivariate_scores  # noqa: E402
from fourierdiffusion_amd.sampling.masks import LinearOperator, apply_operator, observation_mask, operator_from_config, window_means  # noqa: E402
from fourierdiffusion_amd.sampling.sampler import series_labels  # noqa: E402
from fourierdiffusion_amd.utils.extraction import dict_to_str, get_best_checkpoint, get_model_type  # noqa: E402
from fourierdiffusion_amd.utils.fourier import destandardize_idft, idft  # noqa: E402


def hidden_errors(X: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor) -> dict:
    """MSE / MAE of X against the ground truth over the hidden entries (mask False), and the largest deviation on the observed
    ones (the conditioning reproduces them up to f32 transform rounding)."""
    hid = ~mask
    diff = (X.double() - truth.double())
    out = {"num_series": int(X.shape[0]), "hidden_fraction": float(hid.double().mean())}
    if hid.any():
        out["mse_hidden"] = float((diff[hid] ** 2).mean())
        out["mae_hidden"] = float(diff[hid].abs().mean())
    if mask.any():
        out["max_abs_err_observed"] = float(diff[mask].abs().max())
    return out


def ensemble_results(X: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor) -> dict:
    """The results of an ensemble X (n, K, T, C): the shape of the split, the largest deviation on the observed entries over all
    samples, and the aggregates of sampling.forecast.ensemble_scores over the hidden entries."""
    out = {"num_series": int(X.shape[0]), "num_samples_per_series": int(X.shape[1]),
           "hidden_fraction": float((~mask).double().mean())}
    if mask.any():
        diff = X.double() - truth.double()[:, None]
        out["max_abs_err_observed"] = float(diff[mask[:, None].expand_as(diff)].abs().max())
    if (~mask).any():
        out.update(ensemble_scores(X, truth, mask).metrics)
    return out


def channel_std(truth: torch.Tensor) -> torch.Tensor:
    """Per-channel standard deviation of the scored truth split (float64; 1 where it is 0): the scale of the scores that mix channels."""
    std = truth.double().reshape(-1, truth.shape[-1]).std(0, unbiased=False)
    return torch.where(std > 0, std, torch.ones_like(std))


def multivariate_results(X: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor, opts=None) -> dict:
    """The multivariate scores of an ensemble X (n, K, T, C), K > 1 (sampling.forecast.multivariate_scores: energy score, variogram
    score, rank histogram), with every channel divided by the standard deviation of the scored truth split (float64; 1 where it
    is 0), since the energy score mixes channels.  opts: the `variogram` block of the config (order, max_lag, weights)."""
    if X.dim() != 4 or int(X.shape[1]) < 2:
        raise ValueError("multivariate_scores=true needs an ensemble: set num_samples_per_series=K > 1, got samples of shape "
                         f"{tuple(X.shape)}")
    opts = opts or {}
    std = channel_std(truth)
    max_lag = opts.get("max_lag", None)
    m = multivariate_scores(X, truth, mask, order=float(opts.get("order", 0.5)), max_lag=None if max_lag is None else int(max_lag),
                            weights=str(opts.get("weights", "inverse_lag")), scale=std).metrics
    return {**m, "multivariate_scale": "channel_std"}


def multivariate_rank_results(X: torch.Tensor, truth: torch.Tensor, mask: torch.Tensor, kinds) -> dict:
    """The multivariate rank histograms of an ensemble X (n, K, T, C), K > 1 (sampling.forecast.multivariate_rank_histogram), for
    every pre-rank in `kinds`: `rank_histogram_<kind>` (a list), `rank_reliability_index_<kind>` and `n_series_ranked`.  Channels
    are divided by the standard deviation of the scored truth split as in multivariate_results (it matters for mst only)."""
    if X.dim() != 4 or int(X.shape[1]) < 2:
        raise ValueError("multivariate_ranks needs an ensemble: set num_samples_per_series=K > 1, got samples of shape "
                         f"{tuple(X.shape)}")
    std = channel_std(truth)
    out = {}
    for kind, r in multivariate_rank_histogram(X, truth, mask, [str(k) for k in kinds], scale=std).items():
        out[f"rank_reliability_index_{kind}"] = r["reliability_index"]
        out[f"rank_histogram_{kind}"] = [float(v) for v in r["histogram"]]
        out["n_series_ranked"] = r["n_series_ranked"]
    return out


class ImputationRunner:
    def __init__(self, cfg) -> None:
        self.random_seed: int = cfg.random_seed
        torch.manual_seed(self.random_seed)
        logging.info(f"Welcome in the imputation script! You are using the following config:\n{dict_to_str(cfg)}")
        self.dist = init_process_group()
        _rng.set_rank(self.dist.rank)
        self.dev_index = bind_device()
        self.model_path = Path(cfg.model_path)
        self.model_id = cfg.model_id
        if self.model_id == "latest":
            runs = sorted(p for p in self.model_path.iterdir() if (p / "train_config.yaml").exists())
            self.model_id = runs[-1].name
        self.save_dir = self.model_path / self.model_id
        if self.dist.is_main:
            save_yaml(cfg, self.save_dir / "impute_config.yaml")
        train_cfg = load_yaml(self.save_dir / "train_config.yaml")
        self.datamodule = instantiate(train_cfg.datamodule)
        self.fourier_transform: bool = self.datamodule.fourier_transform
        self.datamodule.prepare_data()
        self.datamodule.setup()
        self.num_diffusion_steps: int = cfg.num_diffusion_steps
        self.num_samples: int = int(cfg.get("num_samples_per_series", 1))
        if self.num_samples < 1:
            raise ValueError(f"num_samples_per_series must be >= 1, got {self.num_samples}")
        self.num_series = cfg.get("num_series", None)
        self.mask_cfg = cfg.mask
        self.conditioning: str = str(cfg.get("conditioning", "replace"))
        guidance = cfg.get("guidance", None) or {}
        self.guidance_scale = float(guidance.get("scale", 1.0))
        self.guidance_jacobian = bool(guidance.get("jacobian", True))
        smc = cfg.get("smc", None) or {}
        self.smc = dict(obs_std=float(smc.get("obs_std", 0.1)), twist_scale=float(smc.get("twist_scale", 1.0)),
                        ess_threshold=float(smc.get("ess_threshold", 0.5)))
        self.labels = cfg.get("labels", None)
        self.cfg_scale = float(cfg.get("cfg_scale", 1.0))
        self.resample = int(cfg.get("resample", 1))
        self.jump_length = int(cfg.get("jump_length", 1))
        self.aggregate = int(cfg.get("aggregate", 1))
        self.operator_cfg = {k: v for k, v in dict(cfg.get("operator", None) or {}).items()}
        self.multivariate: bool = bool(cfg.get("multivariate_scores", False))
        self.variogram = dict(cfg.get("variogram", None) or {})
        if self.multivariate and self.num_samples < 2:
            raise ValueError("multivariate_scores=true needs an ensemble: set num_samples_per_series=K > 1")
        self.rank_kinds = [str(k) for k in (cfg.get("multivariate_ranks", None) or [])]
        if [k for k in self.rank_kinds if k not in PRERANKS]:
            raise ValueError(f"multivariate_ranks must be a list out of {PRERANKS}, got {self.rank_kinds}")
        if self.rank_kinds and self.num_samples < 2:
            raise ValueError("multivariate_ranks needs an ensemble: set num_samples_per_series=K > 1")
        best_checkpoint_path = get_best_checkpoint(self.save_dir / "checkpoints")
        model_type = get_model_type(train_cfg)
        self.score_model = model_type.load_from_checkpoint(checkpoint_path=best_checkpoint_path,
                                                             weights=cfg.get("weights", "auto"))
        logging.info(f"Running on the {'averaged (EMA)' if self.score_model.weights_loaded == 'ema' else 'raw'} weights of "
                     f"{best_checkpoint_path}.")
        self.score_model.to(device=torch.device("cuda", self.dev_index))
        self.sampler = instantiate(cfg.sampler)(score_model=self.score_model)

    def impute(self) -> None:
        truth = self.datamodule.X_test.float()
        if self.num_series is not None:
            truth = truth[:int(self.num_series)]
        K = self.num_samples
        # the mask from its own generator: every rank builds the same one, and torch's global generator (the Philox keys) is untouched
        gen = torch.Generator().manual_seed(self.random_seed)
        w = self.aggregate
        if not 1 <= w <= int(truth.shape[1]):
            raise ValueError(f"aggregate must lie in [1, {int(truth.shape[1])}], got {w}")
        coarse = truth if w == 1 else window_means(truth, w)                        # (n, J, C): what is observed, and its mask
        ocfg = self.operator_cfg
        Pm = operator_from_config(ocfg.get("kind", None), int(truth.shape[1]), **{k: ocfg[k] for k in ("n_freq", "w", "stride", "sigma")
                                                                                   if ocfg.get(k, None) is not None})
        op = None
        if Pm is not None:
            if w > 1:
                raise ValueError("operator.kind and aggregate > 1 do not go together")
            op = LinearOperator(Pm, max_condition=float(ocfg.get("max_condition", 1e4)))
            coarse = apply_operator(truth, op).float()                              # (n, M, C)
        mask = observation_mask(self.mask_cfg.kind, tuple(coarse.shape), p=float(self.mask_cfg.get("p", 0.5)),
                                horizon=int(self.mask_cfg.get("horizon", 1)), generator=gen)
        observed = coarse.masked_fill(~mask, float("nan"))                         # the sampler never sees a hidden entry
        agg = {} if w == 1 else dict(aggregate=w)
        if op is not None:
            agg = dict(operator=op)
        lo, hi = shard_range(int(truth.shape[0]), self.dist.rank, self.dist.world)  # independent rows: no exchange
        y = series_labels(self.labels, self.datamodule, int(truth.shape[0]), int(getattr(self.score_model, "n_classes", 0)))
        guided = {} if (y is None and self.cfg_scale == 1.0) else dict(y=None if y is None else y[lo:hi], cfg_scale=self.cfg_scale)
        repaint = {k: v for k, v in (("resample", self.resample), ("jump_length", self.jump_length)) if v != 1}
        mean = std = None
        if self.datamodule.standardize:
            mean, std = self.datamodule.feature_mean_and_std
        X = None
        smc_stats = None
        if hi > lo and self.conditioning == "smc":
            X, info = self.sampler.impute(observed[lo:hi], mask[lo:hi], self.num_diffusion_steps,
                                          fourier_transform=self.fourier_transform, feature_mean=mean, feature_std=std,
                                          num_samples=K, conditioning="smc", guidance_jacobian=self.guidance_jacobian,
                                          return_info=True, **self.smc, **guided, **repaint, **agg)
            unique = torch.tensor([[len(set(a.tolist())) for a in info.ancestors[-1]]], dtype=torch.float64) / K
            # per-series rows: evidence, final ESS / K, resamples, distinct final ancestors / K
            smc_stats = torch.stack([info.log_evidence, info.ess[-1] / K, info.resampled.double().sum(0), unique[0]], dim=1)
        if hi > lo:
            X = X if smc_stats is not None else self.sampler.impute(observed[lo:hi], mask[lo:hi], self.num_diffusion_steps, fourier_transform=self.fourier_transform,
                                    feature_mean=mean, feature_std=std, num_samples=None if K == 1 else K,
                                    conditioning=self.conditioning, guidance_scale=self.guidance_scale,
                                    guidance_jacobian=self.guidance_jacobian, **guided, **repaint, **agg)
            shape = X.shape
            X = X.reshape(-1, *shape[-2:])                                          # (rows, T, C) for the maps back
            if std is not None:
                X = destandardize_idft(X, mean, std) if self.fourier_transform else X * std.cpu() + mean.cpu()
            elif self.fourier_transform:
                X = idft(X)
            X = X.reshape(shape)
        if self.dist.world > 1:
            import torch.distributed as dist
            parts = [None] * self.dist.world
            dist.all_gather_object(parts, X)                                        # host-side gather of the results
            X = torch.cat([p for p in parts if p is not None], dim=0)
            if self.conditioning == "smc":
                stats = [None] * self.dist.world
                dist.all_gather_object(stats, smc_stats)
                smc_stats = torch.cat([p for p in stats if p is not None], dim=0)
        if self.dist.is_main:
            results_path = self.save_dir / "results.yaml"
            results = yaml.safe_load(open(results_path)) if results_path.exists() else None
            results = results if isinstance(results, dict) else {}
            # window means: no full-resolution entry was observed, so the scores run over all of them
            fine = mask if (w == 1 and op is None) else torch.zeros(truth.shape, dtype=torch.bool)
            scores = hidden_errors(X, truth, fine) if K == 1 else ensemble_results(X, truth, fine)
            results["impute"] = {"mask_kind": str(self.mask_cfg.kind), **scores}
            if self.multivariate and (~fine).any():
                results["impute"].update(multivariate_results(X, truth, fine, self.variogram))
            if self.rank_kinds and (~fine).any():
                results["impute"].update(multivariate_rank_results(X, truth, fine, self.rank_kinds))
            if w > 1:
                results["impute"]["aggregate"] = w
                if mask.any():
                    dev = (window_means(X.double(), w) - (coarse.double() if K == 1 else coarse.double()[:, None])).abs()
                    results["impute"]["max_abs_err_window_means"] = float(dev[(mask if K == 1 else mask[:, None]).expand_as(dev)].max())
            if op is not None:
                results["impute"]["operator"] = {"kind": str(ocfg["kind"]), "M": op.M, "condition": float(op.condition),
                                                 **{k: ocfg[k] for k in ("n_freq", "w", "stride", "sigma") if ocfg.get(k, None) is not None}}
                if mask.any():
                    dev = (apply_operator(X.double(), op) - (coarse.double() if K == 1 else coarse.double()[:, None])).abs()
                    results["impute"]["max_abs_err_operator"] = float(dev[(mask if K == 1 else mask[:, None]).expand_as(dev)].max())
            if self.conditioning == "smc":
                st = smc_stats.mean(0)
                results["impute"].update(conditioning="smc", guidance_jacobian=self.guidance_jacobian,
                                         **{f"smc_{k}": v for k, v in self.smc.items()}, smc_log_evidence_mean=float(st[0]),
                                         smc_ess_final_mean=float(st[1]), smc_resamples_mean=float(st[2]),
                                         smc_unique_final_mean=float(st[3]))
            elif self.conditioning != "replace":
                results["impute"].update(conditioning=self.conditioning, guidance_scale=self.guidance_scale,
                                         guidance_jacobian=self.guidance_jacobian)
            if guided:
                results["impute"].update(labels=None if y is None else str(self.labels), cfg_scale=self.cfg_scale)
            results["impute"].update(repaint)
            logging.info(f"Saving imputations and errors to {self.save_dir}.\n{dict_to_str(results['impute'])}")
            yaml.dump(data=results, stream=open(results_path, "w"))
            torch.save(X, self.save_dir / "imputations.pt")


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] %(message)s")
    cfg = compose(Path(__file__).parent / "conf", "impute", overrides=list(sys.argv[1:] if argv is None else argv))
    ImputationRunner(cfg).impute()


if __name__ == "__main__":
    main()
