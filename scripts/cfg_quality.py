#!/usr/bin/env python3
"""Class fidelity and sample quality of classifier-free guidance against the guidance scale, on one easy dataset.

The small transformer (D = 72, L = 2, H = 12, VP-SDE, Fourier noise scaling) is trained class-conditionally (label dropout 0.1) on
SyntheticClassesDatamodule: sines whose frequency band is set by the class.  Every class is then sampled at w in {0, 1, 2, 4}
(w = 0: unconditional, 1: class-conditional, > 1: guided) and two figures are reported per (class, w):
  in_band   the share of samples (channels) whose dominant frequency bin lies in the class's band (up to one bin width)
  sliced_w  the sliced Wasserstein distance to that class's held-out series
and the time per series.  One JSON line per row; --out writes them to a file.  Evidence for DESIGN 3.17 only: one run, one seed.

    python scripts/cfg_quality.py --out profiles/cfg_quality.txt
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SCALES = (0.0, 1.0, 2.0, 4.0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--train-samples", type=int, default=4096)
    ap.add_argument("--num-samples", type=int, default=512, help="per class and scale")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--directions", type=int, default=200)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticClassesDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.metrics import SlicedWasserstein
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    from fourierdiffusion_amd.trainer import Trainer
    from fourierdiffusion_amd.utils.fourier import destandardize_idft

    torch.manual_seed(args.seed)
    data_dir = tempfile.mkdtemp(prefix="cfg_quality_")
    K = args.classes
    dm = SyntheticClassesDatamodule(data_dir=data_dir, random_seed=args.seed, batch_size=64, fourier_transform=True, standardize=True,
                                    max_len=args.T, num_samples=args.train_samples, n_channels=args.C, n_classes=K)
    dm.prepare_data()
    dm.setup()
    steps = args.epochs * (args.train_samples // 64)
    model = ScoreModule(n_channels=args.C, max_len=args.T, noise_scheduler=VPScheduler(fourier_noise_scaling=True),
                        fourier_noise_scaling=True, d_model=72, num_layers=2, n_head=12, num_training_steps=steps, n_classes=K,
                        label_dropout=0.1)
    t0 = time.perf_counter()
    trainer = Trainer(max_epochs=args.epochs, gradient_clip_val=1.0, enable_progress_bar=False, callbacks=[], default_root_dir=data_dir)
    trainer.fit(model, dm)
    torch.cuda.synchronize()
    lines = [{"train": {"epochs": args.epochs, "steps": trainer.global_step, "seconds": round(time.perf_counter() - t0, 1),
                        "final": trainer.history[-1] if trainer.history else None},
              "T": args.T, "C": args.C, "classes": K, "num_samples": args.num_samples, "sde_steps": args.steps,
              "precision": model.precision_effective, "plan": model.plan(args.num_samples)[0]}]
    print(json.dumps(lines[0]), flush=True)
    mean, std = dm.feature_mean_and_std
    sampler = DiffusionSampler(score_model=model, sample_batch_size=args.num_samples)
    bin_w = 2.0 * np.pi / args.T
    for k in range(K):
        held = dm.X_test[dm.y_test == k]
        sw = SlicedWasserstein(original_samples=held, random_seed=args.seed, num_directions=args.directions)
        lo, hi = dm.class_band(k)
        for w in SCALES:
            torch.manual_seed(args.seed + 100 * k + int(10 * w))
            t0 = time.perf_counter()
            X = sampler.sample(args.num_samples, args.steps, y=k, cfg_scale=w)
            sec = time.perf_counter() - t0
            Xt = destandardize_idft(X, mean, std)
            f = dm.dominant_frequency(Xt)
            rec = {"class": k, "w": w, "band": [round(lo, 3), round(hi, 3)],
                   "in_band": float(((f > lo - bin_w) & (f < hi + bin_w)).double().mean()), **sw(Xt),
                   "ms_per_series": 1e3 * sec / X.shape[0], "finite": bool(torch.isfinite(Xt).all())}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
