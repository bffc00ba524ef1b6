#!/usr/bin/env python3
"""python cmd/sample.py model_id=XYZ ... -- sample from a trained score model (reference: cmd/sample.py:18-100).

Loads lightning_logs/<model_id>/train_config.yaml + the best checkpoint, draws num_samples series with
num_diffusion_steps reverse-diffusion steps on the MI355X engine, de-standardises, maps back to the time domain
(one fused kernel) and writes samples.pt + results.yaml next to the checkpoint.  With several processes
(torch.distributed.run) the sample batches are sharded over the ranks (no collective on the data path)."""
from __future__ import annotations

import logging
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import yaml  # noqa: E402

from fourierdiffusion_amd import _rng  # noqa: E402
from fourierdiffusion_amd.config import compose, instantiate, load_yaml, save_yaml  # noqa: E402
from fourierdiffusion_amd.sampling.sampler import parse_covariates, parse_labels  # noqa: E402
from fourierdiffusion_amd.parallel import bind_device, env, init_process_group, shard_range  # noqa: E402
from fourierdiffusion_amd.utils.extraction import dict_to_str, get_best_checkpoint, get_model_type  # noqa: E402
from fourierdiffusion_amd.utils.fourier import destandardize_idft, idft  # noqa: E402


class SamplingRunner:
    def __init__(self, cfg) -> None:
        self.random_seed: int = cfg.random_seed
        torch.manual_seed(self.random_seed)
        logging.info(f"Welcome in the sampling script! You are using the following config:\n{dict_to_str(cfg)}")
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
            save_yaml(cfg, self.save_dir / "sample_config.yaml")
        train_cfg = load_yaml(self.save_dir / "train_config.yaml")
        self.datamodule = instantiate(train_cfg.datamodule)
        self.fourier_transform: bool = self.datamodule.fourier_transform
        self.datamodule.prepare_data()
        self.datamodule.setup()
        self.num_samples: int = cfg.num_samples
        self.num_diffusion_steps: int = cfg.num_diffusion_steps
        best_checkpoint_path = get_best_checkpoint(self.save_dir / "checkpoints")
        model_type = get_model_type(train_cfg)
        self.score_model = model_type.load_from_checkpoint(checkpoint_path=best_checkpoint_path,
                                                             weights=cfg.get("weights", "auto"))
        logging.info(f"Running on the {'averaged (EMA)' if self.score_model.weights_loaded == 'ema' else 'raw'} weights of "
                     f"{best_checkpoint_path}.")
        self.score_model.to(device=torch.device("cuda", self.dev_index))
        self.sampler = instantiate(cfg.sampler)(score_model=self.score_model)
        # metrics against the training set, on the main rank only (reference cmd/sample.py:62-65)
        self.metrics = None
        if "metrics" in cfg and cfg.metrics is not None and self.dist.is_main:
            # a metrics config with `holdout: true` (metrics=neighbours) also gets the held-out split, for the memorisation metrics
            # and one with `labels: true` (metrics=conditional) the classes of both splits, for the label-aware metrics
            node = {k: v for k, v in cfg.metrics.items() if k not in ("holdout", "labels")}
            holdout = bool(cfg.metrics.get("holdout", False))
            bound = {"holdout_samples": self.datamodule.X_test} if holdout else {}
            if cfg.metrics.get("labels", False):
                if getattr(self.datamodule, "y_train", None) is None:
                    raise ValueError(f"the metrics config asks for labels (labels: true), but {type(self.datamodule).__name__} has no "
                                     "labels (y_train is None): use a labelled datamodule or a metrics config without `labels`")
                if self.score_model.n_classes <= 0 and self.sampler.labels is None:
                    raise ValueError("the metrics config asks for labels (labels: true), but no labels will be drawn: the model is "
                                     "not class-conditional and sampler.labels is null")
                bound["original_labels"] = self.datamodule.y_train
                if holdout:
                    bound["holdout_labels"] = self.datamodule.y_test
            self.metrics = instantiate(node)(original_samples=self.datamodule.X_train, **bound)

    def sample(self) -> None:
        bs = self.sampler.sample_batch_size
        num_batches = max(1, self.num_samples // bs)
        lo, hi = shard_range(num_batches, self.dist.rank, self.dist.world)       # independent units: no exchange
        n_local = (hi - lo) * min(bs, self.num_samples)
        X = labels = covariates = None
        if n_local:
            guide = {}
            cond_dim = int(getattr(self.score_model, "cond_dim", 0))
            spec = getattr(self.sampler, "covariates", None)
            if cond_dim > 0 or spec is not None:
                # sampler.covariates: `data`, a list in data units or null; the rows used (model units) are written next to the samples
                covariates = parse_covariates(spec, n_local, cond_dim, self.datamodule)
                guide = {"y": covariates, "cfg_scale": self.sampler.cfg_scale}
            elif self.score_model.n_classes > 0 or self.sampler.labels is not None or self.sampler.cfg_scale != 1.0:
                # sampler.labels: a class, `balanced` or null; the chosen labels are written next to the samples
                labels = parse_labels(self.sampler.labels, n_local, self.score_model.n_classes)
                guide = {"y": labels, "cfg_scale": self.sampler.cfg_scale}
            X = self.sampler.sample(num_samples=n_local, num_diffusion_steps=self.num_diffusion_steps, **guide)
        if X is not None:
            if self.datamodule.standardize:
                feature_mean, feature_std = self.datamodule.feature_mean_and_std
                if self.fourier_transform:
                    X = destandardize_idft(X, feature_mean, feature_std)            # cmd/sample.py:76-82 fused
                else:
                    X = X * feature_std.cpu() + feature_mean.cpu()
            elif self.fourier_transform:
                X = idft(X)
        if self.dist.world > 1:
            import torch.distributed as dist
            parts = [None] * self.dist.world
            dist.all_gather_object(parts, (X, labels, covariates))                  # host-side gather of the results
            X = torch.cat([p[0] for p in parts if p[0] is not None], dim=0)
            cov = [p[2] for p in parts if p[0] is not None]
            covariates = torch.cat(cov, dim=0) if cov and all(v is not None for v in cov) else None
            lab = [p[1] for p in parts if p[0] is not None]
            labels = torch.cat(lab, dim=0) if lab and all(v is not None for v in lab) else None
        if self.dist.is_main:
            results = {"num_samples": int(X.shape[0]), "sample_mean": float(X.mean()), "sample_std": float(X.std())}
            info = getattr(self.sampler, "last_info", None)
            if info is not None:      # sampler=ode_adaptive: what the tolerance cost (this rank's rows)
                results.update(nfe_mean=float(info.nfe.double().mean()), nfe_max=int(info.nfe.max()),
                               n_not_converged=int((~info.converged).sum()), row_evals_launched=int(info.row_evals_launched))
            if self.metrics is not None:
                # reference cmd/sample.py:84-86; the classes the samples were drawn for go to the label-aware metrics only
                results.update(self.metrics(X, other_labels=labels))
            logging.info(f"Saving samples ands metrics to {self.save_dir}.\n{dict_to_str(results)}")
            yaml.dump(data=results, stream=open(self.save_dir / "results.yaml", "w"))
            torch.save(X, self.save_dir / "samples.pt")
            if labels is not None:
                torch.save(labels, self.save_dir / "labels.pt")
            if covariates is not None:
                torch.save(covariates, self.save_dir / "covariates.pt")


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] %(message)s")
    cfg = compose(Path(__file__).parent / "conf", "sample", overrides=list(sys.argv[1:] if argv is None else argv))
    SamplingRunner(cfg).sample()


if __name__ == "__main__":
    main()
