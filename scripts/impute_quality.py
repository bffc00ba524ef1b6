#!/usr/bin/env python3
"""Ensemble scores of conditional sampling (DiffusionSampler.impute(num_samples=K), sampling/forecast.py) on one trained model.

The model and data are those of scripts/ode_quality.py: a default-width transformer (D = 72, L = 10, H = 12, VP-SDE, Fourier noise
scaling) trained on SyntheticDatamodule (sines, generated from the seed; frequency domain, standardised).  The first `--series`
held-out series are masked (a forecast mask of horizon `--horizon`, a random mask hiding each entry with probability `--p`, each
from a generator of its own), imputed with K = `--num-samples` samples per series at every step count of `--steps`, mapped back to
the time domain and scored over the hidden entries.  One run, one seed.  One JSON line per (mask, steps, conditioning); `--out FILE`
writes the table as JSON.

`--conditioning replace dps` adds rows of gradient guidance (impute(conditioning="dps")) for every `--guidance-scale` and every
`--jacobian` setting (on: with the network's Jacobian, off: Jacobian-free).  `--time-domain` trains the model on the time-domain
representation instead (standardised all the same).  `--conditioning ... smc` adds rows of the twisted particle filter
(impute(conditioning="smc"), K particles per series) for every `--obs-std` and every `--jacobian` setting, with the mean log
evidence, the final ESS / K and the resamples per series next to the scores.  The defaults reproduce the table of the projection
alone."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--train-samples", type=int, default=4096)
    ap.add_argument("--series", type=int, default=256)
    ap.add_argument("--num-samples", type=int, default=50)
    ap.add_argument("--steps", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--conditioning", nargs="+", choices=["replace", "dps", "smc"], default=["replace"])
    ap.add_argument("--obs-std", type=float, nargs="+", default=[0.1])
    ap.add_argument("--guidance-scale", type=float, nargs="+", default=[1.0])
    ap.add_argument("--jacobian", nargs="+", choices=["on", "off"], default=["on"])
    ap.add_argument("--time-domain", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.forecast import ensemble_scores
    from fourierdiffusion_amd.sampling.masks import observation_mask
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    from fourierdiffusion_amd.trainer import Trainer
    from fourierdiffusion_amd.utils.fourier import destandardize_idft

    fourier = not args.time_domain

    torch.manual_seed(args.seed)
    data_dir = tempfile.mkdtemp(prefix="impute_quality_")
    dm = SyntheticDatamodule(data_dir=data_dir, random_seed=args.seed, batch_size=64, fourier_transform=fourier, standardize=True,
                             max_len=args.T, num_samples=args.train_samples, n_channels=args.C)
    dm.prepare_data()
    dm.setup()
    steps = args.epochs * (args.train_samples // 64)
    sch = VPScheduler(fourier_noise_scaling=True)
    model = ScoreModule(n_channels=args.C, max_len=args.T, noise_scheduler=sch, fourier_noise_scaling=True, d_model=72, num_layers=10,
                        n_head=12, num_training_steps=steps)
    t0 = time.perf_counter()
    trainer = Trainer(max_epochs=args.epochs, gradient_clip_val=1.0, enable_progress_bar=False, callbacks=[], default_root_dir=data_dir)
    trainer.fit(model, dm)
    torch.cuda.synchronize()
    head = {"train": {"epochs": args.epochs, "steps": trainer.global_step, "seconds": round(time.perf_counter() - t0, 1),
                      "final_loss": trainer.history[-1] if trainer.history else None},
            "T": args.T, "C": args.C, "series": args.series, "K": args.num_samples, "seed": args.seed,
            "precision": model.precision_effective, "fourier_transform": fourier}
    print(json.dumps(head), flush=True)
    truth = dm.X_test[: args.series].float()
    mean, std = dm.feature_mean_and_std
    K = args.num_samples
    sampler = DiffusionSampler(score_model=model, sample_batch_size=2000)
    masks = {f"forecast_h{args.horizon}": observation_mask("forecast", tuple(truth.shape), horizon=args.horizon),
             f"random_p{args.p}": observation_mask("random", tuple(truth.shape), p=args.p,
                                                   generator=torch.Generator().manual_seed(args.seed))}
    variants = []      # (conditioning keyword arguments, the row's extra fields)
    for cond in args.conditioning:
        if cond == "replace":
            variants.append(({}, {}))
            continue
        if cond == "smc":
            for jac in args.jacobian:
                for sd in args.obs_std:
                    variants.append((dict(conditioning="smc", obs_std=sd, guidance_jacobian=jac == "on", return_info=True),
                                     {"conditioning": "smc", "obs_std": sd, "guidance_jacobian": jac == "on"}))
            continue
        for jac in args.jacobian:
            for zeta in args.guidance_scale:
                variants.append((dict(conditioning="dps", guidance_scale=zeta, guidance_jacobian=jac == "on"),
                                 {"conditioning": "dps", "guidance_scale": zeta, "guidance_jacobian": jac == "on"}))
    rows = []
    for name, mask in masks.items():
        observed = truth.masked_fill(~mask, float("nan"))
        for N in args.steps:
            for kw, extra in variants:
                torch.manual_seed(args.seed + N)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X = sampler.impute(observed, mask, N, fourier_transform=fourier, feature_mean=mean, feature_std=std, num_samples=K,
                                   **kw)
                if kw.get("return_info"):
                    X, info = X
                    extra = {**extra, "log_evidence_mean": float(info.log_evidence.mean()),
                             "ess_final_over_K": float(info.ess[-1].mean()) / K,
                             "resamples_per_series": float(info.resampled.double().sum(0).mean()),
                             "degenerate": int(info.degenerate.sum())}
                torch.cuda.synchronize()
                sec = time.perf_counter() - t0
                if fourier:
                    Xt = destandardize_idft(X.reshape(-1, args.T, args.C), mean, std).reshape(X.shape).cpu()
                else:
                    Xt = (X * std.cpu() + mean.cpu()).cpu()
                t1 = time.perf_counter()
                sc = ensemble_scores(Xt, truth, mask)
                rec = {"mask": name, "steps": N, "K": K, **extra, "impute_s": round(sec, 2),
                       "score_s": round(time.perf_counter() - t1, 2), **sc.metrics, "finite": bool(torch.isfinite(Xt).all())}
                print(json.dumps(rec), flush=True)
                rows.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"setup": head, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
