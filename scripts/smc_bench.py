#!/usr/bin/env python3
"""ms per diffusion step of DiffusionSampler.impute(conditioning="smc") against conditioning="dps" on the same rows, with and without
the network's Jacobian, on the bf16 path: the ecg shape (T = 100, C = 12) with B = 512 rows as 16 series x 32 particles, and T = 1024,
C = 16 with B = 64 rows as 4 series x 16; default-width model (D = 72, L = 10, H = 12), random weights, a random 50 % mask, Fourier
and standardised.  "dps" runs the same rows as ensembles of K samples per series.  The four variants are alternated `--reps` times
and the best of each is reported.  One JSON line per shape; `--out FILE` also writes them as a JSON list.  The particle filter's own
kernels are timed by a separate `rocprofv3 --kernel-trace` run of this script on one variant (`--variants`)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

VARIANTS = ["dps_jacobian", "smc_jacobian", "dps_no_jacobian", "smc_no_jacobian"]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["ecg", "long"], default=None)
    ap.add_argument("--variants", nargs="+", choices=VARIANTS, default=VARIANTS, help="run these only (a kernel trace of one variant)")
    ap.add_argument("--obs-std", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    args = ap.parse_args()
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    shapes = {"ecg": (dict(T=100, C=12, D=72, L=10, H=12), 16, 32), "long": (dict(T=1024, C=16, D=72, L=10, H=12), 4, 16)}
    out = []
    for name, (cfg, n, K) in shapes.items():
        if args.only and name != args.only:
            continue
        m, _, _ = make_model(cfg, precision="bf16")
        T, C = cfg["T"], cfg["C"]
        rs = np.random.RandomState(0)
        y = torch.from_numpy(rs.randn(n, T, C)).float()
        mask = torch.from_numpy(rs.rand(n, T, C) < 0.5)
        mean, std = torch.zeros(T, C), torch.from_numpy(rs.uniform(0.5, 2.0, (T, C))).float()
        s = DiffusionSampler(score_model=m, sample_batch_size=n * K, merge_batches=False)
        N = args.steps
        kw = dict(fourier_transform=True, feature_mean=mean, feature_std=std, num_samples=K)
        resamples = {}

        def smc(jac, tag):
            _, info = s.impute(y, mask, N, conditioning="smc", obs_std=args.obs_std, guidance_jacobian=jac, return_info=True, **kw)
            resamples[tag] = float(info.resampled.double().sum(0).mean())

        runs = {"dps_jacobian": lambda: s.impute(y, mask, N, conditioning="dps", guidance_scale=1.0, **kw),
                "smc_jacobian": lambda: smc(True, "smc_jacobian"),
                "dps_no_jacobian": lambda: s.impute(y, mask, N, conditioning="dps", guidance_scale=1.0, guidance_jacobian=False, **kw),
                "smc_no_jacobian": lambda: smc(False, "smc_no_jacobian")}
        runs = {k: v for k, v in runs.items() if k in args.variants}
        for fn in runs.values():                                                              # warm-up (code objects, buffers)
            fn()
        times = {k: [] for k in runs}
        for _ in range(args.reps):                                                            # alternate the variants
            for k, fn in runs.items():
                times[k].append(timed(fn))
        rec = {"shape": name, "T": T, "C": C, "B": n * K, "series": n, "particles": K, "steps": N}
        for k, ts in times.items():
            rec[f"{k}_ms_per_step"] = 1e3 * min(ts) / N
            rec[f"{k}_ms_per_step_all"] = [1e3 * t / N for t in ts]
        for tag in ("jacobian", "no_jacobian"):
            if f"smc_{tag}" in runs and f"dps_{tag}" in runs:
                rec[f"smc_over_dps_{tag}"] = rec[f"smc_{tag}_ms_per_step"] / rec[f"dps_{tag}_ms_per_step"]
        rec["resamples_per_series"] = resamples
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
