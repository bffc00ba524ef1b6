#!/usr/bin/env python3
"""Held-out likelihood of a time-domain and a frequency-domain score model against the number of ODE steps
(DiffusionSampler.log_likelihood, Heun, Rademacher probes), reported in the DATA space both models share (the series as the
datamodule holds them), with a closed-form anchor: the multivariate Gaussian fitted to the training split.

Two default-width transformers (D = 72, L = 10, H = 12, VP-SDE) are trained for `--epochs` on SyntheticDatamodule (sines, generated
locally from the seed; standardised), one on the series and one on their spectra (Fourier noise scaling).  Each then evaluates the
first `--num-series` held-out series at N = 25, 50, 100, 200 steps, then adaptively (solver="rk45") at each of `--rtols`
(rtol = atol): mean and max NFE, series not converged within `--max-evals` (left out of the NLL), and the difference to the
Heun-200 row.  Rows: mean data-space NLL per series and bits per dimension with their standard errors over series (the probe noise
is inside them).  `--precision` sets the likelihood arithmetic (default: the model's).  One JSON line per row; `--out FILE` writes
the table."""
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

STEPS = (25, 50, 100, 200)


def mean_se(v: torch.Tensor):
    v = v.double()
    return float(v.mean()), float(v.std() / math.sqrt(v.numel()))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--train-samples", type=int, default=4096)
    ap.add_argument("--num-series", type=int, default=256)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--rtols", default="1e-3,1e-5", help="rk45 tolerances (comma-separated; empty: no rk45 rows)")
    ap.add_argument("--max-evals", type=int, default=20000)
    ap.add_argument("--precision", choices=["bf16", "fp32"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticDatamodule
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.likelihood import bits_per_dim, to_data_space
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    from fourierdiffusion_amd.trainer import Trainer
    from fourierdiffusion_amd.utils.fourier import dft

    T, C, n = args.T, args.C, args.num_series
    rows = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        rows.append(rec)

    for fourier in (False, True):
        torch.manual_seed(args.seed)
        data_dir = tempfile.mkdtemp(prefix="ll_quality_")
        dm = SyntheticDatamodule(data_dir=data_dir, random_seed=args.seed, batch_size=64, fourier_transform=fourier, standardize=True,
                                 max_len=T, num_samples=args.train_samples, n_channels=C)
        dm.prepare_data()
        dm.setup()
        if not fourier:      # the anchor: a multivariate Gaussian fitted to the training split, evaluated on the same held-out series
            Xtr = dm.X_train.double().reshape(dm.X_train.shape[0], -1)
            Xte = dm.X_test[:n].double().reshape(n, -1)
            mu = Xtr.mean(0)
            cov = torch.cov(Xtr.T) + 1e-6 * torch.eye(T * C, dtype=torch.float64)
            lp = torch.distributions.MultivariateNormal(mu, covariance_matrix=cov).log_prob(Xte)
            nll, se = mean_se(-lp)
            b, bse = mean_se(bits_per_dim(lp, T, C))
            emit({"model": "gaussian fit (closed form)", "steps": None, "nll_data": nll, "nll_data_se": se, "bits_per_dim": b,
                  "bits_per_dim_se": bse})
        steps = args.epochs * (args.train_samples // 64)
        sch = VPScheduler(fourier_noise_scaling=fourier)
        model = ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, fourier_noise_scaling=fourier, d_model=72, num_layers=10,
                            n_head=12, num_training_steps=steps)
        t0 = time.perf_counter()
        trainer = Trainer(max_epochs=args.epochs, gradient_clip_val=1.0, enable_progress_bar=False, callbacks=[], default_root_dir=data_dir)
        trainer.fit(model, dm)
        torch.cuda.synchronize()
        tag = "frequency" if fourier else "time"
        print(json.dumps({"train": tag, "steps": trainer.global_step, "seconds": round(time.perf_counter() - t0, 1),
                          "final_loss": trainer.history[-1] if trainer.history else None, "precision": model.precision_effective}),
              flush=True)
        mean, std = dm.feature_mean_and_std
        X = dm.X_test[:n].float().cuda()
        Xs = ((dft(X) if fourier else X) - mean) / std
        if args.precision:
            model.precision = args.precision
        sampler = DiffusionSampler(score_model=model, sample_batch_size=256)
        heun200 = None
        for N in STEPS:
            t0 = time.perf_counter()
            res = sampler.log_likelihood(Xs, N, "heun", seed=args.seed)
            sec = time.perf_counter() - t0
            lp = to_data_space(res.log_prob, fourier, std.cpu())
            nll, se = mean_se(-lp)
            b, bse = mean_se(bits_per_dim(lp, T, C))
            emit({"model": f"{tag} domain", "steps": N, "evals": 2 * N, "nll_data": nll, "nll_data_se": se, "bits_per_dim": b,
                  "bits_per_dim_se": bse, "nll_sample": mean_se(-res.log_prob)[0], "ms_per_series": 1e3 * sec / n,
                  "finite": bool(torch.isfinite(lp).all()), "precision": model.precision_effective})
            if N == 200:
                heun200 = nll
        for rtol in [float(r) for r in args.rtols.split(",") if r.strip()]:
            t0 = time.perf_counter()
            res = sampler.log_likelihood(Xs, solver="rk45", rtol=rtol, atol=rtol, max_evals=args.max_evals, seed=args.seed)
            sec = time.perf_counter() - t0
            ok = res.converged
            lp = to_data_space(res.log_prob[ok], fourier, std.cpu())
            nll, se = mean_se(-lp) if lp.numel() > 1 else (float("nan"), float("nan"))
            b, bse = mean_se(bits_per_dim(lp, T, C)) if lp.numel() > 1 else (float("nan"), float("nan"))
            emit({"model": f"{tag} domain", "solver": "rk45", "rtol": rtol, "nfe_mean": float(res.nfe.double().mean()),
                  "nfe_max": int(res.nfe.max()), "n_not_converged": int((~ok).sum()), "nll_data": nll, "nll_data_se": se,
                  "bits_per_dim": b, "bits_per_dim_se": bse, "minus_heun200": None if heun200 is None else nll - heun200,
                  "ms_per_series": 1e3 * sec / n, "precision": model.precision_effective})
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"T": T, "C": C, "epochs": args.epochs, "num_series": n, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
