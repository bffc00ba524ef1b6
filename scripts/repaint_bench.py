#!/usr/bin/env python3
"""ms per score evaluation of DiffusionSampler.impute(resample=r, jump_length=j) (RePaint resampling: the re-noise is fused into the
step + projection kernel) against ms per step of the plain impute(), on the bf16 path, at the benched ecg shape (T = 100, C = 12,
B = 2 x CUs) and at BASELINE configs[4] (T = 1024, C = 16, B = 64), default-width model (D = 72, L = 10, H = 12), random weights, a
random 50 % mask.  The variants of `--variants` (plain, or r,j pairs such as 4,1 4,5) are alternated `--reps` times; the plain
variant runs `--steps` steps, a resampled one `--steps` steps of r evaluations each.  One JSON line per shape; `--out FILE` also
writes them as a JSON list, `--tag` names the build in every record (a comparison alternates this script between two builds through
FDIFF_LIB, with `--variants plain` on the older one).  The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this
script with `--reps 1` and one variant."""
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
    ap.add_argument("--variants", nargs="+", default=["plain", "4,1", "4,5"], help="plain, or resample,jump_length")
    ap.add_argument("--tag", default="head", help="the build's name in the records")
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    args = ap.parse_args()
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = {"ecg": (dict(T=100, C=12, D=72, L=10, H=12), 2 * cus), "long": (dict(T=1024, C=16, D=72, L=10, H=12), 64)}
    out = []
    for name, (cfg, B) in shapes.items():
        if args.only and name != args.only:
            continue
        m, _, _ = make_model(cfg, precision="bf16")
        T, C = cfg["T"], cfg["C"]
        rs = np.random.RandomState(0)
        y = torch.from_numpy(rs.randn(B, T, C)).float()
        mask = torch.from_numpy(rs.rand(B, T, C) < 0.5)
        mean, std = torch.zeros(T, C), torch.from_numpy(rs.uniform(0.5, 2.0, (T, C))).float()
        s = DiffusionSampler(score_model=m, sample_batch_size=B, merge_batches=False)
        N = args.steps
        runs = {}
        for v in args.variants:
            kw = {} if v == "plain" else dict(zip(("resample", "jump_length"), (int(k) for k in v.split(","))))
            evals = N * kw.get("resample", 1)
            runs[v] = (lambda kw=kw: s.impute(y, mask, N, fourier_transform=True, feature_mean=mean, feature_std=std, **kw), evals)
        for fn, _ in runs.values():                                                          # warm-up (code objects, bases)
            fn()
        times = {v: [] for v in runs}
        for _ in range(args.reps):                                                           # alternate the variants
            for v, (fn, evals) in runs.items():
                times[v].append(1e3 * timed(fn) / evals)
        rec = {"shape": name, "T": T, "C": C, "B": B, "steps": N, "build": args.tag}
        for v, ts in times.items():
            rec[f"{v}_ms_per_eval"] = min(ts)
            rec[f"{v}_ms_per_eval_all"] = ts
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
