#!/usr/bin/env python3
"""ms per diffusion step of DiffusionSampler.impute() on a class-conditional model with labels and a guidance scale w = 2 (the two
evaluations of a step as one forward on 2B rows and one paired step kernel), `replace` and Jacobian-free `dps`, against the same
labelled model through the call without labels (one evaluation on B rows: the code path as it was before labels reached `impute`).
bf16, T = 100, C = 12, B = 512 series, default-width model (D = 72, L = 10, H = 12, K = 3 classes), random weights, a random 50 %
mask, Fourier and standardised, 50 steps.  The variants are alternated `--reps` times and the best of each is reported, one JSON
line; `--out FILE` also writes it.  Kernel times come from a separate `rocprofv3 --kernel-trace` run of this script per variant
(`--variants`).  The expectation to confirm or refute: a paired step costs about 2 x the step-wise forward plus one step kernel of
unchanged size."""
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

VARIANTS = ["replace_plain", "replace_cfg", "dps_plain", "dps_cfg"]


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
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--cfg-scale", type=float, default=2.0)
    ap.add_argument("--variants", nargs="+", choices=VARIANTS, default=VARIANTS, help="run these only (a kernel trace of one variant)")
    ap.add_argument("--out", default=None, help="also write the record to this JSON file")
    args = ap.parse_args()
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    T, C, K, B, N, w = 100, 12, 3, args.batch, args.steps, args.cfg_scale
    sch = VPScheduler(fourier_noise_scaling=True)
    sch.set_noise_scaling(T)
    torch.manual_seed(0)
    m = ScoreModule(n_channels=C, max_len=T, noise_scheduler=sch, fourier_noise_scaling=True, d_model=72, num_layers=10, n_head=12,
                    n_classes=K).to("cuda")
    m.precision = "bf16"
    rs = np.random.RandomState(0)
    obs = torch.from_numpy(rs.randn(B, T, C)).float()
    mask = torch.from_numpy(rs.rand(B, T, C) < 0.5)
    labels = torch.from_numpy(rs.randint(0, K, B))
    mean, std = torch.zeros(T, C), torch.from_numpy(rs.uniform(0.5, 2.0, (T, C))).float()
    # a paired launch holds sample_batch_size // 2 series: 2B keeps all B series in one launch, as the plain call has them
    s = DiffusionSampler(score_model=m, sample_batch_size=2 * B, merge_batches=False)
    kw = dict(fourier_transform=True, feature_mean=mean, feature_std=std)
    dps = dict(conditioning="dps", guidance_scale=1.0, guidance_jacobian=False)
    runs = {"replace_plain": lambda: s.impute(obs, mask, N, **kw),
            "replace_cfg": lambda: s.impute(obs, mask, N, y=labels, cfg_scale=w, **kw),
            "dps_plain": lambda: s.impute(obs, mask, N, **dps, **kw),
            "dps_cfg": lambda: s.impute(obs, mask, N, y=labels, cfg_scale=w, **dps, **kw)}
    runs = {k: v for k, v in runs.items() if k in args.variants}
    for fn in runs.values():                                                              # warm-up (code objects, buffers)
        fn()
    times = {k: [] for k in runs}
    for _ in range(args.reps):                                                            # alternate the variants
        for k, fn in runs.items():
            times[k].append(timed(fn))
    rec = {"T": T, "C": C, "B": B, "steps": N, "n_classes": K, "cfg_scale": w, "precision": "bf16"}
    for k, ts in times.items():
        rec[f"{k}_ms_per_step"] = 1e3 * min(ts) / N
        rec[f"{k}_ms_per_step_all"] = [1e3 * t / N for t in ts]
    for k in ("replace", "dps"):
        if f"{k}_cfg" in runs and f"{k}_plain" in runs:
            rec[f"{k}_cfg_over_plain"] = rec[f"{k}_cfg_ms_per_step"] / rec[f"{k}_plain_ms_per_step"]
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
