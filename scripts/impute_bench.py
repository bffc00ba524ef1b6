#!/usr/bin/env python3
"""ms per diffusion step of DiffusionSampler.sample() against DiffusionSampler.impute() (conditional sampling) on the bf16 path, at
the benched ecg shape (T = 100, C = 12, B = 2 x CUs) and at BASELINE configs[4] (T = 1024, C = 16, B = 64), default-width model
(D = 72, L = 10, H = 12), random weights, a random 50 % mask.  One JSON line per shape; `--out FILE` also writes them as a JSON list.
The fused step + projection kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.

`--num-samples K` (ensembles, DiffusionSampler.impute(num_samples=K)): at the ecg shape, the same `--rows` state rows (default
512) once as `rows` series at K = 1 (the default call) and once as rows / K series x K replicas, alternated; one JSON line."""
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


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["ecg", "long"], default=None)
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    ap.add_argument("--num-samples", type=int, default=None, help="ensemble mode: K replicas per series")
    ap.add_argument("--rows", type=int, default=512, help="ensemble mode: state rows per launch")
    args = ap.parse_args()
    if args.num_samples is not None:
        return ensemble(args)
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
        run_s = lambda: s.sample(num_samples=B, num_diffusion_steps=N)                     # noqa: E731
        run_i = lambda: s.impute(y, mask, N, fourier_transform=True, feature_mean=mean, feature_std=std)   # noqa: E731
        run_s(), run_i()                                                                      # warm-up (code objects, bases)
        ts, ti = [], []
        for _ in range(args.reps):                                                           # alternate the two
            ts.append(timed(run_s, 1))
            ti.append(timed(run_i, 1))
        rec = {"shape": name, "T": T, "C": C, "B": B, "steps": N, "sample_ms_per_step": 1e3 * min(ts) / N,
               "impute_ms_per_step": 1e3 * min(ti) / N, "sample_ms_per_step_all": [1e3 * t / N for t in ts],
               "impute_ms_per_step_all": [1e3 * t / N for t in ti]}
        rec["impute_over_sample"] = rec["impute_ms_per_step"] / rec["sample_ms_per_step"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def ensemble(args) -> None:
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    cfg, B, K, N = dict(T=100, C=12, D=72, L=10, H=12), args.rows, args.num_samples, args.steps
    if K < 1 or B % K:
        raise SystemExit(f"--rows {B} must be a multiple of --num-samples {K}")
    m, _, _ = make_model(cfg, precision="bf16")
    T, C = cfg["T"], cfg["C"]
    rs = np.random.RandomState(0)
    y = torch.from_numpy(rs.randn(B, T, C)).float()
    mask = torch.from_numpy(rs.rand(B, T, C) < 0.5)
    mean, std = torch.zeros(T, C), torch.from_numpy(rs.uniform(0.5, 2.0, (T, C))).float()
    s = DiffusionSampler(score_model=m, sample_batch_size=B, merge_batches=False)
    kw = dict(fourier_transform=True, feature_mean=mean, feature_std=std)
    n = B // K
    run_1 = lambda: s.impute(y, mask, N, **kw)                                               # noqa: E731
    run_k = lambda: s.impute(y[:n], mask[:n], N, num_samples=K, **kw)                         # noqa: E731
    run_1(), run_k()                                                                          # warm-up
    t1, tk = [], []
    for _ in range(args.reps):                                                               # alternate the two
        t1.append(timed(run_1, 1))
        tk.append(timed(run_k, 1))
    rec = {"shape": "ecg", "T": T, "C": C, "rows": B, "steps": N, "K": K, "series_at_K": n,
           "k1_ms_per_step": 1e3 * min(t1) / N, "ensemble_ms_per_step": 1e3 * min(tk) / N,
           "k1_ms_per_step_all": [1e3 * t / N for t in t1], "ensemble_ms_per_step_all": [1e3 * t / N for t in tk]}
    rec["ensemble_over_k1"] = rec["ensemble_ms_per_step"] / rec["k1_ms_per_step"]
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump([rec], f, indent=1)


if __name__ == "__main__":
    main()
