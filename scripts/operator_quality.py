#!/usr/bin/env python3
"""Ensemble scores of conditioning on a general linear observation (DiffusionSampler.impute(operator=P, num_samples=K)) on one
trained model per representation.

The models and data are those of scripts/impute_quality.py and scripts/aggregate_quality.py: a default-width transformer (D = 72,
L = 10, H = 12, VP-SDE, Fourier noise scaling) trained on SyntheticDatamodule (sines, generated from the seed; standardised), once
on the frequency-domain representation and once on the time-domain one.  The first `--series` held-out series are reduced to y = P x
for the four constructors of sampling.masks -- lowpass (bandwidth extension), moving_average (overlapping windows), difference
(increments) and gaussian_blur (deblurring), every row observed -- K = `--num-samples` full-resolution samples per series are drawn
at `--steps` steps under the projection and under Jacobian-free gradient guidance for every `--guidance-scale`, mapped back to the
time domain and scored over ALL entries (no full-resolution entry is observed).  Two baselines: an unconditional ensemble of the
same size, and the minimum-norm lift P^+ y (a point estimate: its MAE).  One run, one seed, no threshold.  One JSON line per row;
`--out FILE` writes the table as JSON."""
from __future__ import annotations

import argparse
import json
import math
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--guidance-scale", type=float, nargs="+", default=[0.1, 0.3])
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling import masks as M
    from fourierdiffusion_amd.sampling.forecast import ensemble_scores
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    from fourierdiffusion_amd.trainer import Trainer
    from fourierdiffusion_amd.utils.fourier import destandardize_idft

    T, C, K, N = args.T, args.C, args.num_samples, args.steps
    operators = {"lowpass": (M.lowpass_operator(T, 8), dict(n_freq=8)), "moving_average": (M.moving_average_operator(T, 5, 2), dict(w=5, stride=2)),
                 "difference": (M.difference_operator(T), {}), "gaussian_blur": (M.gaussian_blur_operator(T, 2.0, 4), dict(sigma=2.0, stride=4))}
    setups, rows = [], []
    for fourier in (False, True):
        torch.manual_seed(args.seed)
        data_dir = tempfile.mkdtemp(prefix="operator_quality_")
        dm = SyntheticDatamodule(data_dir=data_dir, random_seed=args.seed, batch_size=64, fourier_transform=fourier, standardize=True,
                                 max_len=T, num_samples=args.train_samples, n_channels=C)
        dm.prepare_data()
        dm.setup()
        steps = args.epochs * (args.train_samples // 64)
        model = ScoreModule(n_channels=C, max_len=T, noise_scheduler=VPScheduler(fourier_noise_scaling=True),
                            fourier_noise_scaling=True, d_model=72, num_layers=10, n_head=12, num_training_steps=steps)
        t0 = time.perf_counter()
        trainer = Trainer(max_epochs=args.epochs, gradient_clip_val=1.0, enable_progress_bar=False, callbacks=[],
                          default_root_dir=data_dir)
        trainer.fit(model, dm)
        torch.cuda.synchronize()
        head = {"train": {"epochs": args.epochs, "steps": trainer.global_step, "seconds": round(time.perf_counter() - t0, 1),
                          "final_loss": trainer.history[-1] if trainer.history else None},
                "T": T, "C": C, "series": args.series, "K": K, "steps": N, "seed": args.seed, "precision": model.precision_effective,
                "fourier_transform": fourier}
        print(json.dumps(head), flush=True)
        setups.append(head)
        truth = dm.X_test[: args.series].float()
        n = int(truth.shape[0])
        mean, std = dm.feature_mean_and_std
        hidden = torch.zeros(truth.shape, dtype=torch.bool)          # every full-resolution entry is scored
        sampler = DiffusionSampler(score_model=model, sample_batch_size=2000)

        def to_time(X):
            if fourier:
                return destandardize_idft(X.reshape(-1, T, C), mean, std).reshape(X.shape).cpu()
            return (X.cpu() * std.cpu() + mean.cpu())

        def record(extra, Xt, sec):
            sc = ensemble_scores(Xt, truth, hidden).metrics
            rec = {"fourier_transform": fourier, **extra, "crps": sc["crps"], "coverage_90": sc["coverage_90"],
                   "mae_median": sc.get("mae_median"), "finite": bool(torch.isfinite(Xt).all()), "impute_s": round(sec, 2)}
            print(json.dumps(rec), flush=True)
            rows.append(rec)

        torch.manual_seed(args.seed)
        t0 = time.perf_counter()
        U = DiffusionSampler(score_model=model, sample_batch_size=K * math.gcd(n, 32)).sample(num_samples=n * K, num_diffusion_steps=N)
        torch.cuda.synchronize()
        record({"method": "unconditional"}, to_time(U.reshape(n, K, T, C)), time.perf_counter() - t0)
        for i, (kind, (Pm, params)) in enumerate(operators.items()):
            op = M.LinearOperator(Pm)
            y = M.apply_operator(truth, op).float()
            lift = M.lift_operator(y, op).float()
            rec = {"fourier_transform": fourier, "method": "lift", "operator": kind, **params, "M": op.M, "condition": round(op.condition, 2),
                   "mae": float((lift - truth).abs().mean())}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            variants = [({}, {"method": "replace"})]
            variants += [(dict(conditioning="dps", guidance_scale=z, guidance_jacobian=False),
                          {"method": "dps", "guidance_scale": z, "guidance_jacobian": False}) for z in args.guidance_scale]
            for kw, extra in variants:
                torch.manual_seed(args.seed + 1 + i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X = sampler.impute(y, None, N, fourier_transform=fourier, feature_mean=mean, feature_std=std, num_samples=K, operator=op,
                                   **kw)
                torch.cuda.synchronize()
                sec = time.perf_counter() - t0
                Xt = to_time(X)
                extra = dict(extra, operator=kind, M=op.M,
                             max_abs_err_operator=float((M.apply_operator(Xt, op) - y.double()[:, None]).abs().max()))
                record(extra, Xt, sec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"setups": setups, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
