#!/usr/bin/env python3
"""Sample quality against the number of score evaluations: reverse-SDE sampling (Euler-Maruyama, the reference's sampler) against the
probability-flow ODE (Heun, Euler, deterministic DDIM, DPM-Solver++ 2M; on the time-uniform grid and on the log-SNR grid; and the
adaptive Dormand-Prince sampler at rtol = atol = 1e-3 and 1e-5, the ODE's own solution to that tolerance) on one trained model.

A default-width transformer (D = 72, L = 10, H = 12, VP-SDE, Fourier noise scaling) is trained on SyntheticDatamodule (sines, generated
locally from the seed; frequency domain, standardised), then every sampler draws `--num-samples` series; the series are mapped back to
the time domain and compared with the held-out split by sliced (`--directions` directions) and marginal Wasserstein-2
(fdiff.sampling.metrics).  The split's own two halves and its mean give the floor and the ceiling.  Wall-clock per series includes
the prior, the loop and the transfer to the host.  One JSON line per sampler; `--out FILE` writes the table as JSON."""
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

ROWS = [("sde", 1000), ("sde", 100), ("sde", 50), ("heun", 10), ("heun", 25), ("heun", 50), ("heun", 100), ("euler", 100)]
# (sampler, steps, schedule) rows behind them: the data-prediction solvers at 10-50 evaluations on both grids, Euler / Heun on the
# log-SNR grid at the evaluation counts of their time-grid rows
ROWS = [(k, n, "time") for k, n in ROWS] + \
       [(k, n, sc) for k in ("ddim", "dpmpp2m") for sc in ("time", "logsnr") for n in (10, 15, 20, 30, 50)] + \
       [("heun", 10, "logsnr"), ("heun", 25, "logsnr"), ("heun", 50, "logsnr"), ("euler", 50, "logsnr"), ("euler", 100, "logsnr")]
# the adaptive sampler (Dormand-Prince 5(4), sample_ode_adaptive) at rtol = atol: the ODE's own solution to that tolerance, the point
# the fixed-grid ODE rows converge to; evaluations are per row (nfe mean / max), launches of `--adaptive-batch` rows
RK45_TOLS = (1e-3, 1e-5)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--train-samples", type=int, default=4096)
    ap.add_argument("--num-samples", type=int, default=2048)
    ap.add_argument("--directions", type=int, default=1000)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    ap.add_argument("--adaptive-batch", type=int, default=512)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.metrics import MarginalWasserstein, SlicedWasserstein
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    from fourierdiffusion_amd.trainer import Trainer
    from fourierdiffusion_amd.utils.fourier import destandardize_idft

    torch.manual_seed(args.seed)
    data_dir = tempfile.mkdtemp(prefix="ode_quality_")
    dm = SyntheticDatamodule(data_dir=data_dir, random_seed=args.seed, batch_size=64, fourier_transform=True, standardize=True,
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
    train_s = time.perf_counter() - t0
    head = {"train": {"epochs": args.epochs, "steps": trainer.global_step, "seconds": round(train_s, 1),
                      "final_loss": trainer.history[-1] if trainer.history else None},
            "T": args.T, "C": args.C, "num_samples": args.num_samples, "precision": model.precision_effective}
    print(json.dumps(head), flush=True)
    held_out = dm.X_test[: args.num_samples]
    mean, std = dm.feature_mean_and_std
    sw = SlicedWasserstein(original_samples=held_out, random_seed=args.seed, num_directions=args.directions)
    mw = MarginalWasserstein(original_samples=held_out, random_seed=args.seed)
    base = {**sw.baseline_metrics, **mw.baseline_metrics}
    print(json.dumps({"baselines": base}), flush=True)
    sampler = DiffusionSampler(score_model=model, sample_batch_size=args.num_samples)
    rows = []
    for kind, N, schedule in ROWS:
        torch.manual_seed(args.seed + N)
        run = (lambda: sampler.sample(args.num_samples, N)) if kind == "sde" else \
            (lambda: sampler.sample_ode(args.num_samples, N, solver=kind, schedule=schedule))
        run() if N <= 100 else None       # (warm-up of short runs: the first launch of a shape builds images / workspace)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X = run()
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        Xt = destandardize_idft(X, mean, std)
        rec = {"sampler": kind, "schedule": schedule, "steps": N, "evals": N * (2 if kind == "heun" else 1),
               "ms_per_series": 1e3 * sec / X.shape[0],
               **sw(Xt), **mw(Xt), "finite": bool(torch.isfinite(Xt).all())}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    adaptive = DiffusionSampler(score_model=model, sample_batch_size=args.adaptive_batch)
    for tol in RK45_TOLS:
        torch.manual_seed(args.seed)
        run = lambda: adaptive.sample_ode_adaptive(args.num_samples, rtol=tol, atol=tol, return_info=True)      # noqa: E731
        run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X, info = run()
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        Xt = destandardize_idft(X, mean, std)
        rec = {"sampler": "rk45", "schedule": "adaptive", "rtol": tol, "atol": tol, "evals": float(info.nfe.double().mean()),
               "nfe_max": int(info.nfe.max()), "n_not_converged": int((~info.converged).sum()),
               "row_evals_launched": info.row_evals_launched, "row_evals_needed": info.row_evals_needed,
               "ms_per_series": 1e3 * sec / X.shape[0], **sw(Xt), **mw(Xt), "finite": bool(torch.isfinite(Xt).all())}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"setup": head, "baselines": base, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
