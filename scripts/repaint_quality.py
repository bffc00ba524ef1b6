#!/usr/bin/env python3
"""Quality of RePaint resampling (DiffusionSampler.impute(resample=r, jump_length=j)) against plain replacement at EQUAL numbers of
score evaluations, on one trained model.

The model and data are those of scripts/impute_quality.py: a default-width transformer (D = 72, L = 10, H = 12, VP-SDE, Fourier noise
scaling) trained on SyntheticDatamodule (sines, generated from the seed; frequency domain, standardised).  The first `--series`
held-out series are masked (a forecast mask of horizon `--horizon`, a random mask hiding each entry with probability `--p`, each from
a generator of its own) and imputed under every `--configs` entry N,r,j -- by default (200,1,1) against (50,4,1), (50,4,5) and
(25,8,1), 200 evaluations each.  Per (mask, config): the MSE over the hidden entries of one sample per series, and the ensemble CRPS
of K = `--num-samples` samples per series (sampling/forecast.py).  One run, one seed.  One JSON line per row; `--out FILE` writes
the table as JSON.  `--time-domain` trains the model on the time-domain representation instead."""
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
    ap.add_argument("--num-samples", type=int, default=8)
    ap.add_argument("--configs", nargs="+", default=["200,1,1", "50,4,1", "50,4,5", "25,8,1"], help="N,resample,jump_length")
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--seed", type=int, default=42)
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
    configs = [tuple(int(v) for v in c.split(",")) for c in args.configs]

    torch.manual_seed(args.seed)
    data_dir = tempfile.mkdtemp(prefix="repaint_quality_")
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
    sampler = DiffusionSampler(score_model=model, sample_batch_size=2048)
    masks = {f"forecast_h{args.horizon}": observation_mask("forecast", tuple(truth.shape), horizon=args.horizon),
             f"random_p{args.p}": observation_mask("random", tuple(truth.shape), p=args.p,
                                                   generator=torch.Generator().manual_seed(args.seed))}

    def to_time(X):
        if fourier:
            return destandardize_idft(X.reshape(-1, args.T, args.C), mean, std).reshape(X.shape).cpu()
        return (X * std.cpu() + mean.cpu()).cpu()

    rows = []
    for name, mask in masks.items():
        observed = truth.masked_fill(~mask, float("nan"))
        hid = ~mask
        for N, r, j in configs:
            kw = dict(fourier_transform=fourier, feature_mean=mean, feature_std=std, resample=r, jump_length=j)
            torch.manual_seed(args.seed + N)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            X1 = to_time(sampler.impute(observed, mask, N, **kw))
            XK = to_time(sampler.impute(observed, mask, N, num_samples=K, **kw))
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            diff = X1.double() - truth.double()
            sc = ensemble_scores(XK, truth, mask)
            rec = {"mask": name, "steps": N, "resample": r, "jump_length": j, "evaluations": N * r,
                   "mse_hidden": float((diff[hid] ** 2).mean()), "K": K, **sc.metrics, "impute_s": round(sec, 2),
                   "finite": bool(torch.isfinite(X1).all() and torch.isfinite(XK).all())}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"setup": head, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
