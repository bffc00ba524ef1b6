#!/usr/bin/env python3
"""Do labels help a forecast?  Ensemble scores of DiffusionSampler.impute(num_samples=K, y=labels, cfg_scale=w) on one trained
class-conditional model: a default-width transformer (D = 72, L = 10, H = 12, K = 3 classes, label dropout 0.1, VP-SDE, Fourier
noise scaling) trained on SyntheticClassesDatamodule (sines whose class sets the frequency band; frequency domain, standardised).
The first `--series` held-out series get a forecast mask of horizon `--horizon`, are forecast with `--num-samples` samples per series
under their test labels (`--labels data`) at every `--cfg-scale` -- w = 0 ignores the labels, w = 1 is the class-conditional model,
w = 2 guides --, mapped back to the time domain and scored over the hidden entries (CRPS, 90 % interval coverage and the other
aggregates of sampling/forecast.py).  One run, one seed.  One JSON line per scale; `--out FILE` writes the table as JSON."""
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--C", type=int, default=1)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--labels", choices=["data"], default="data")
    ap.add_argument("--cfg-scale", type=float, nargs="+", default=[0.0, 1.0, 2.0])
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticClassesDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.forecast import ensemble_scores
    from fourierdiffusion_amd.sampling.masks import observation_mask
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler, series_labels
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    from fourierdiffusion_amd.trainer import Trainer
    from fourierdiffusion_amd.utils.fourier import destandardize_idft

    torch.manual_seed(args.seed)
    data_dir = tempfile.mkdtemp(prefix="cfg_impute_quality_")
    dm = SyntheticClassesDatamodule(data_dir=data_dir, random_seed=args.seed, batch_size=64, fourier_transform=True, standardize=True,
                                    max_len=args.T, num_samples=args.train_samples, n_channels=args.C, n_classes=args.classes)
    dm.prepare_data()
    dm.setup()
    steps = args.epochs * (args.train_samples // 64)
    sch = VPScheduler(fourier_noise_scaling=True)
    model = ScoreModule(n_channels=args.C, max_len=args.T, noise_scheduler=sch, fourier_noise_scaling=True, d_model=72, num_layers=10,
                        n_head=12, num_training_steps=steps, n_classes=args.classes, label_dropout=0.1)
    t0 = time.perf_counter()
    trainer = Trainer(max_epochs=args.epochs, gradient_clip_val=1.0, enable_progress_bar=False, callbacks=[], default_root_dir=data_dir)
    trainer.fit(model, dm)
    torch.cuda.synchronize()
    head = {"train": {"epochs": args.epochs, "steps": trainer.global_step, "seconds": round(time.perf_counter() - t0, 1),
                      "final_loss": trainer.history[-1] if trainer.history else None},
            "T": args.T, "C": args.C, "n_classes": args.classes, "series": args.series, "K": args.num_samples, "steps": args.steps,
            "horizon": args.horizon, "seed": args.seed, "precision": model.precision_effective}
    print(json.dumps(head), flush=True)
    truth = dm.X_test[: args.series].float()
    n = int(truth.shape[0])
    y = series_labels(args.labels, dm, n, args.classes)
    mean, std = dm.feature_mean_and_std
    K = args.num_samples
    sampler = DiffusionSampler(score_model=model, sample_batch_size=2000)
    mask = observation_mask("forecast", tuple(truth.shape), horizon=args.horizon)
    observed = truth.masked_fill(~mask, float("nan"))
    rows = []
    for w in args.cfg_scale:
        torch.manual_seed(args.seed + args.steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X = sampler.impute(observed, mask, args.steps, fourier_transform=True, feature_mean=mean, feature_std=std, num_samples=K, y=y,
                           cfg_scale=w)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        Xt = destandardize_idft(X.reshape(-1, args.T, args.C), mean, std).reshape(X.shape).cpu()
        sc = ensemble_scores(Xt, truth, mask)
        rec = {"mask": f"forecast_h{args.horizon}", "labels": args.labels, "cfg_scale": w, "impute_s": round(sec, 2), **sc.metrics,
               "finite": bool(torch.isfinite(Xt).all())}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"setup": head, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
