#!/usr/bin/env python3
"""How well classifier-free guidance on real-valued covariates hits the attributes it is asked for, on one easy dataset.

The small transformer (D = 72, L = 2, H = 12, VP-SDE, Fourier noise scaling) is trained with cond_dim = 2 (covariate dropout 0.1) on
SyntheticCovariatesDatamodule: noisy sines whose frequency (cycles per window) and amplitude are the two covariates.  A grid of
requested (frequency, amplitude) pairs is then sampled at w in {0, 1, 2} (w = 0: the null vector, the baseline that ignores the
request; 1: conditional; 2: guided) and per (request, w) the mean absolute error between the request and what the samples show is
reported: the periodogram peak (cycles per window) against the frequency, sqrt(2) rms against the amplitude, over samples and
channels.  One JSON line per row; --out writes them to a file.  Evidence for DESIGN 3.35 only: one run, one seed, no threshold.

    python scripts/cov_quality.py --out profiles/cov_quality.txt
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

SCALES = (0.0, 1.0, 2.0)
FREQUENCIES = (1.5, 3.0, 4.5)
AMPLITUDES = (0.75, 1.5)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--train-samples", type=int, default=4096)
    ap.add_argument("--num-samples", type=int, default=256, help="per request and scale")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticCovariatesDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler, parse_covariates
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    from fourierdiffusion_amd.trainer import Trainer
    from fourierdiffusion_amd.utils.fourier import destandardize_idft

    torch.manual_seed(args.seed)
    data_dir = tempfile.mkdtemp(prefix="cov_quality_")
    dm = SyntheticCovariatesDatamodule(data_dir=data_dir, random_seed=args.seed, batch_size=64, fourier_transform=True,
                                       standardize=True, max_len=args.T, num_samples=args.train_samples, n_channels=args.C)
    dm.prepare_data()
    dm.setup()
    steps = args.epochs * (args.train_samples // 64)
    model = ScoreModule(n_channels=args.C, max_len=args.T, noise_scheduler=VPScheduler(fourier_noise_scaling=True),
                        fourier_noise_scaling=True, d_model=72, num_layers=2, n_head=12, num_training_steps=steps, cond_dim=2,
                        cond_dropout=0.1)
    t0 = time.perf_counter()
    trainer = Trainer(max_epochs=args.epochs, gradient_clip_val=1.0, enable_progress_bar=False, callbacks=[], default_root_dir=data_dir)
    trainer.fit(model, dm)
    torch.cuda.synchronize()
    lines = [{"train": {"epochs": args.epochs, "steps": trainer.global_step, "seconds": round(time.perf_counter() - t0, 1),
                        "final": trainer.history[-1] if trainer.history else None},
              "T": args.T, "C": args.C, "num_samples": args.num_samples, "sde_steps": args.steps,
              "precision": model.precision_effective, "plan": model.plan(args.num_samples)[0]}]
    print(json.dumps(lines[0]), flush=True)
    mean, std = dm.feature_mean_and_std
    sampler = DiffusionSampler(score_model=model, sample_batch_size=args.num_samples)
    for fi, f_req in enumerate(FREQUENCIES):
        for ai, a_req in enumerate(AMPLITUDES):
            c = parse_covariates([f_req, a_req], args.num_samples, 2, dm)
            for w in SCALES:
                torch.manual_seed(args.seed + 100 * fi + 10 * ai + int(w))
                t0 = time.perf_counter()
                X = sampler.sample(args.num_samples, args.steps, y=c, cfg_scale=w)
                sec = time.perf_counter() - t0
                Xt = destandardize_idft(X, mean, std).to(torch.float64)
                spec = torch.fft.rfft(Xt, dim=1).abs()
                peak = (spec[:, 1:].argmax(dim=1) + 1).to(torch.float64)               # cycles per window, (n, C)
                amp = np.sqrt(2.0) * Xt.pow(2).mean(dim=1).sqrt()                       # (n, C)
                rec = {"frequency": f_req, "amplitude": a_req, "w": w,
                       "mae_frequency": float((peak - f_req).abs().mean()), "mae_amplitude": float((amp - a_req).abs().mean()),
                       "mean_peak": float(peak.mean()), "mean_amplitude": float(amp.mean()),
                       "ms_per_series": 1e3 * sec / X.shape[0], "finite": bool(torch.isfinite(Xt).all())}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
