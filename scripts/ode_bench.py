#!/usr/bin/env python3
"""ms per score evaluation of DiffusionSampler.sample() (reverse SDE, Euler-Maruyama) against sample_ode (probability-flow ODE: Euler,
Heun, and the data-prediction solvers DDIM and DPM-Solver++ 2M on the log-SNR grid) on the bf16 path, default-width model (D = 72, L = 10, H = 12), random weights: at the benched ecg shape (T = 100, C = 12,
B = 2 x CUs: the persistent kernel) and at BASELINE configs[4] (T = 1024, C = 16, B = 64: layer launches + the fused
unembed / step / embed launch).  The same number of evaluations per run for every sampler (`--evals`, below the run-time
specialisation threshold, so all of them run the same ahead-of-time kernel), runs alternated over `--reps` rounds, the median kept.
One JSON line per shape; `--out FILE` also writes them as a JSON list."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=50, help="score evaluations per run (even)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["ecg", "long"], default=None)
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    args = ap.parse_args()
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = {"ecg": (dict(T=100, C=12, D=72, L=10, H=12), 2 * cus), "long": (dict(T=1024, C=16, D=72, L=10, H=12), 64)}
    E = args.evals
    out = []
    for name, (cfg, B) in shapes.items():
        if args.only and name != args.only:
            continue
        m, _, _ = make_model(cfg, precision="bf16")
        s = DiffusionSampler(score_model=m, sample_batch_size=B)
        runs = {"sde": lambda: s.sample(B, E), "ode_euler": lambda: s.sample_ode(B, E, solver="euler"),
                "ode_heun": lambda: s.sample_ode(B, E // 2, solver="heun"),
                "ode_ddim": lambda: s.sample_ode(B, E, solver="ddim", schedule="logsnr"),
                "ode_dpmpp2m": lambda: s.sample_ode(B, E, solver="dpmpp2m", schedule="logsnr")}
        for fn in runs.values():         # warm-up: images, workspace, first launches
            fn()
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                times[k].append(timed(fn))
        rec = {"shape": name, "T": cfg["T"], "C": cfg["C"], "B": B, "evals": E, "reps": args.reps,
               "plan": m.plan(B, "bf16")[0].split(" S=")[0]}
        for k, v in times.items():
            rec[f"{k}_ms_per_eval"] = 1e3 * statistics.median(v) / E
            rec[f"{k}_ms_per_eval_rounds"] = [round(1e3 * t / E, 5) for t in v]
        rec["heun_over_sde"] = rec["ode_heun_ms_per_eval"] / rec["sde_ms_per_eval"]
        rec["euler_over_sde"] = rec["ode_euler_ms_per_eval"] / rec["sde_ms_per_eval"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
