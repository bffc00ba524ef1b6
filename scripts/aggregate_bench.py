#!/usr/bin/env python3
"""ms per diffusion step of DiffusionSampler.impute(aggregate=w) for w in `--windows` (w = 1: the coordinate-mask path), under the
projection (conditioning="replace") and Jacobian-free gradient guidance (conditioning="dps"), on the bf16 path, at the ecg shape
(T = 100, C = 12, B = 512) and at T = 1024, C = 16, B = 64; default-width model (D = 72, L = 10, H = 12), random weights, a random
50 % mask over windows, Fourier and standardised.  All variants are alternated `--reps` times and the best of each is reported with
the spread of its runs.  One JSON line per shape; `--out FILE` also writes them as a JSON list.  The kernels' own times come from a
separate `rocprofv3 --kernel-trace` run of this script (`--only`, `--windows`, `--conditionings` narrow it)."""
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
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--conditionings", nargs="+", choices=["replace", "dps"], default=["replace", "dps"])
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    args = ap.parse_args()
    from fourierdiffusion_amd.sampling.masks import window_means
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    shapes = {"ecg": (dict(T=100, C=12, D=72, L=10, H=12), 512), "long": (dict(T=1024, C=16, D=72, L=10, H=12), 64)}
    out = []
    for name, (cfg, B) in shapes.items():
        if args.only and name != args.only:
            continue
        m, _, _ = make_model(cfg, precision="bf16")
        T, C = cfg["T"], cfg["C"]
        rs = np.random.RandomState(0)
        fine = torch.from_numpy(rs.randn(B, T, C)).float()
        mean, std = torch.zeros(T, C), torch.from_numpy(rs.uniform(0.5, 2.0, (T, C))).float()
        s = DiffusionSampler(score_model=m, sample_batch_size=B, merge_batches=False)
        N = args.steps
        runs = {}
        for w in args.windows:
            y = window_means(fine, w)
            mask = torch.from_numpy(rs.rand(*y.shape) < 0.5)
            kw = dict(fourier_transform=True, feature_mean=mean, feature_std=std, aggregate=w)
            if "replace" in args.conditionings:
                runs[f"replace_w{w}"] = lambda y=y, mask=mask, kw=kw: s.impute(y, mask, N, **kw)
            if "dps" in args.conditionings:
                runs[f"dps_w{w}"] = lambda y=y, mask=mask, kw=kw: s.impute(y, mask, N, conditioning="dps", guidance_scale=1.0,
                                                                         guidance_jacobian=False, **kw)
        for fn in runs.values():                                                              # warm-up (code objects, bases, buffers)
            fn()
        times = {k: [] for k in runs}
        for _ in range(args.reps):                                                            # alternate the variants
            for k, fn in runs.items():
                times[k].append(timed(fn))
        rec = {"shape": name, "T": T, "C": C, "B": B, "steps": N}
        for k, ts in times.items():
            rec[f"{k}_ms_per_step"] = 1e3 * min(ts) / N
            rec[f"{k}_ms_per_step_all"] = [1e3 * t / N for t in ts]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
