#!/usr/bin/env python3
"""Milliseconds per sampling step of a covariate-conditional model against its three baselines: the same model at
w = 1, a class-conditional model of the same size, and the unlabelled model on the persistent kernel.  Default shape T = 100,
C = 12, B = 512, d_model 72, 12 heads, 10 layers, bf16.  Each figure: the median over --repeats timed `sample` calls of --steps
steps (after --warmup untimed ones; host clock around a call that ends in a device synchronise, the copy of the samples to the host
included), divided by the steps; the rows alternate inside every repeat.  One JSON line per row; --out writes them to a file.

    python scripts/cov_step_bench.py --out profiles/cov_step_bench.txt
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--C", type=int, default=12)
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.schedulers.sde import VPScheduler

    def model(**kw):
        torch.manual_seed(0)
        sch = VPScheduler(fourier_noise_scaling=True)
        sch.set_noise_scaling(args.T)
        m = ScoreModule(n_channels=args.C, max_len=args.T, noise_scheduler=sch, d_model=72, num_layers=args.layers, n_head=12, **kw)
        return m.to("cuda")

    B = args.B
    c = torch.randn(B, 2)
    y = torch.arange(B) % 3
    cov, cls, plain = model(cond_dim=2), model(n_classes=3), model()
    rows = [("covariates w=2 (pair)", cov, dict(y=c, cfg_scale=2.0)), ("covariates w=1", cov, dict(y=c, cfg_scale=1.0)),
            ("classes w=2 (pair)", cls, dict(y=y, cfg_scale=2.0)), ("classes w=1", cls, dict(y=y, cfg_scale=1.0)),
            ("unlabelled", plain, {})]
    # the rows alternate inside every repeat, so that a drift of the machine meets all of them alike
    samplers = [DiffusionSampler(score_model=m, sample_batch_size=B) for _, m, _ in rows]
    ts = [[] for _ in rows]
    for i in range(args.warmup + args.repeats):
        for r, (_, _, kw) in enumerate(rows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            samplers[r].sample(B, args.steps, **kw)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts[r].append(1e3 * (time.perf_counter() - t0) / args.steps)
    lines = []
    for r, (name, m, _) in enumerate(rows):
        rec = {"row": name, "T": args.T, "C": args.C, "B": B, "layers": args.layers, "steps": args.steps,
               "ms_per_step_median": round(statistics.median(ts[r]), 4), "ms_per_step_min": round(min(ts[r]), 4),
               "ms_per_step_max": round(max(ts[r]), 4), "plan": m.plan(B)[0]}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
