#!/usr/bin/env python3
"""python cmd/likelihood.py model_id=XYZ num_diffusion_steps=100 solver=heun n_probes=4 -- held-out log-likelihood of a trained
score model (an extension, not in the reference): DiffusionSampler.log_likelihood on the test split (the probability-flow ODE with
a Hutchinson or exact divergence, on the MI355X engine), mapped to the series as the datamodule holds them (time domain, data
scale), so that a time-domain and a frequency-domain model are compared on one number.  Writes the key `likelihood` of
results.yaml: mean and standard error over series of the data-space NLL, bits per dimension, the sample-space NLL and the
settings; solver=rk45 (adaptive, rtol / atol) adds nfe_mean, nfe_max and n_not_converged and takes the NLL over the converged
series.  labels=data|<int> (class-conditional models) evaluates log p(x | y) on the test labels (`datamodule.y_test`) or one class,
recorded only when set.  With several processes (torch.distributed.run) the rows are sharded over the ranks, as cmd/impute.py does."""
from __future__ import annotations

import logging
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import yaml  # noqa: E402

from fourierdiffusion_amd import _rng  # noqa: E402
from fourierdiffusion_amd.config import compose, instantiate, load_yaml, save_yaml  # noqa: E402
from fourierdiffusion_amd.parallel import bind_device, init_process_group, shard_range  # noqa: E402
from fourierdiffusion_amd.sampling.likelihood import bits_per_dim, to_data_space  # noqa: E402
from fourierdiffusion_amd.sampling.sampler import series_labels  # noqa: E402
from fourierdiffusion_amd.utils.extraction import dict_to_str, get_best_checkpoint, get_model_type  # noqa: E402
from fourierdiffusion_amd.utils.fourier import dft  # noqa: E402


def mean_se(v: torch.Tensor) -> tuple:
    v = v.double()
    se = float(v.std() / math.sqrt(v.numel())) if v.numel() > 1 else float("nan")
    return float(v.mean()), se


class LikelihoodRunner:
    def __init__(self, cfg) -> None:
        self.random_seed: int = cfg.random_seed
        torch.manual_seed(self.random_seed)
        logging.info(f"Welcome in the likelihood script! You are using the following config:\n{dict_to_str(cfg)}")
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
            save_yaml(cfg, self.save_dir / "likelihood_config.yaml")
        train_cfg = load_yaml(self.save_dir / "train_config.yaml")
        self.datamodule = instantiate(train_cfg.datamodule)
        self.fourier_transform: bool = self.datamodule.fourier_transform
        self.datamodule.prepare_data()
        self.datamodule.setup()
        self.cfg = cfg
        best_checkpoint_path = get_best_checkpoint(self.save_dir / "checkpoints")
        model_type = get_model_type(train_cfg)
        self.score_model = model_type.load_from_checkpoint(checkpoint_path=best_checkpoint_path,
                                                             weights=cfg.get("weights", "auto"))
        logging.info(f"Running on the {'averaged (EMA)' if self.score_model.weights_loaded == 'ema' else 'raw'} weights of "
                     f"{best_checkpoint_path}.")
        self.score_model.to(device=torch.device("cuda", self.dev_index))
        self.sampler = instantiate(cfg.sampler)(score_model=self.score_model)

    def evaluate(self) -> None:
        cfg = self.cfg
        X = self.datamodule.X_test.float()
        if cfg.max_series is not None:
            X = X[: int(cfg.max_series)]
        dev = self.score_model.device
        std = None
        Xs = dft(X.to(dev)) if self.fourier_transform else X.to(dev)       # sample space, as the datamodule builds it
        if self.datamodule.standardize:
            mean, std = self.datamodule.feature_mean_and_std
            Xs = (Xs - mean.to(dev)) / std.to(dev)
        lo, hi = shard_range(int(X.shape[0]), self.dist.rank, self.dist.world)     # independent rows: no exchange
        y = series_labels(cfg.get("labels", None), self.datamodule, int(X.shape[0]), int(getattr(self.score_model, "n_classes", 0)))
        adaptive = str(cfg.solver) == "rk45"
        kw = dict(rtol=float(cfg.rtol), atol=float(cfg.atol), max_evals=int(cfg.max_evals)) if adaptive else {}
        lp, nfe = torch.empty(0, dtype=torch.float64), torch.empty(0, dtype=torch.int64)
        if hi > lo:
            res = self.sampler.log_likelihood(Xs[lo:hi], int(cfg.num_diffusion_steps), str(cfg.solver), estimator=str(cfg.estimator),
                                              n_probes=int(cfg.n_probes), **kw, **({} if y is None else dict(y=y[lo:hi])))
            lp, nfe = res.log_prob, res.nfe
        if self.dist.world > 1:
            import torch.distributed as dist
            parts = [None] * self.dist.world
            dist.all_gather_object(parts, (lp, nfe))                                 # host-side gather of the results
            lp = torch.cat([p[0] for p in parts if p is not None and p[0].numel()], dim=0)
            nfe = torch.cat([p[1] for p in parts if p is not None and p[1].numel()], dim=0)
        if self.dist.is_main:
            T, C = int(X.shape[1]), int(X.shape[2])
            n_series = int(lp.numel())
            if adaptive:      # a series whose integration did not converge has log_prob NaN: the NLL is over the others
                ok = ~torch.isnan(lp)
                extra = {"nfe_mean": float(nfe.double().mean()), "nfe_max": int(nfe.max()), "n_not_converged": int((~ok).sum()),
                         "rtol": float(cfg.rtol), "atol": float(cfg.atol), "max_evals": int(cfg.max_evals)}
                lp = lp[ok]
            lp_data = to_data_space(lp, self.fourier_transform, None if std is None else std.cpu(), max_len=T, n_channels=C)
            nll, nll_se = mean_se(-lp_data)
            bpd, bpd_se = mean_se(bits_per_dim(lp_data, T, C))
            nll_s, nll_s_se = mean_se(-lp)
            out = {"num_series": n_series, "nll_data": nll, "nll_data_se": nll_se, "bits_per_dim": bpd, "bits_per_dim_se": bpd_se,
                   "nll_sample": nll_s, "nll_sample_se": nll_s_se,
                   "num_diffusion_steps": None if adaptive else int(cfg.num_diffusion_steps),
                   "solver": str(cfg.solver), "estimator": str(cfg.estimator), "n_probes": int(cfg.n_probes),
                   "fourier_transform": bool(self.fourier_transform), "precision": self.score_model.precision_effective}
            if adaptive:
                out.update(extra)
            if y is not None:
                out["labels"] = str(cfg.labels)
            results_path = self.save_dir / "results.yaml"
            results = yaml.safe_load(open(results_path)) if results_path.exists() else None
            results = results if isinstance(results, dict) else {}
            results["likelihood"] = out
            logging.info(f"Saving the likelihood to {results_path}.\n{dict_to_str(out)}")
            yaml.dump(data=results, stream=open(results_path, "w"))


def main(argv=None) -> None:
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] %(message)s")
    cfg = compose(Path(__file__).parent / "conf", "likelihood", overrides=list(sys.argv[1:] if argv is None else argv))
    LikelihoodRunner(cfg).evaluate()


if __name__ == "__main__":
    main()
