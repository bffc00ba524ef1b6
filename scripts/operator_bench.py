#!/usr/bin/env python3
"""ms per diffusion step of DiffusionSampler.impute(operator=P) under the projection (conditioning="replace") and Jacobian-free
gradient guidance (conditioning="dps"), on the bf16 path, at the ecg shape (T = 100, C = 12, B = 512) and at T = 1024, C = 16,
B = 64; default-width model (D = 72, L = 10, H = 12), random weights, standardised.  Variants (`--variants` narrows them):

    agg4        aggregate=4, the window operator (J = T / 4 windows): the yardstick, the same two product sizes as dense_m256 at T = 1024
    lowpass     lowpass_operator(T, 8), Fourier domain (M = 15), a random row mask
    blur        gaussian_blur_operator(T, 2, 4), Fourier domain (M = T / 4: 256 at T = 1024), a random (series, channel) column mask
    time_full   gaussian_blur_operator(T, 0.8, 1) on a time-domain model (M = T), a column mask

All variants are alternated `--reps` times and the best of each is reported with the spread of its runs.  `build`: the one-off cost of
a fresh operator at that shape -- the host's float64 SVD / pseudo-inverse, and the first engine call (upload of P and P^+, the basis
build on the device and the wait for it) minus a second call.  One JSON line per shape; `--out FILE` also writes them as a JSON
list.  The kernels' own times come from a separate `rocprofv3 --kernel-trace --output-format csv` run of this script;
`--summarise DIR` prints, per kernel of k_impute / k_dps_residual found in the *kernel_trace.csv files under DIR, the number of
launches and the median / min / max duration in us."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("agg4", "lowpass", "blur", "time_full")


def summarise(root: str) -> None:
    """Per (file, kernel): launches, median / min / max us of the conditional kernels in rocprofv3's kernel-trace CSVs under root."""
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        durs: dict = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if "k_impute<" not in name and "k_dps_residual<" not in name and "k_linop_" not in name:
                    continue
                name = name.replace("void ", "").replace("(anonymous namespace)::", "").replace("fdproj::", "").split("(")[0]
                durs.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        for name, d in sorted(durs.items()):
            print(f"{os.path.relpath(path, root)} | {name} | n={len(d)} median {statistics.median(d):.1f} min {min(d):.1f} "
                  f"max {max(d):.1f} us", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["ecg", "long"], default=None)
    ap.add_argument("--variants", nargs="+", choices=VARIANTS, default=list(VARIANTS))
    ap.add_argument("--conditionings", nargs="+", choices=["replace", "dps"], default=["replace", "dps"])
    ap.add_argument("--no-build", action="store_true", help="skip the one-off build timing")
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    ap.add_argument("--summarise", metavar="DIR", default=None, help="summarise rocprofv3 kernel-trace CSVs under DIR and exit")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise)
        return

    import numpy as np
    import torch

    from fourierdiffusion_amd.sampling import masks as M
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

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
        rows = torch.from_numpy(rs.rand(B, 1, C) < 0.5)        # whole (series, channel) columns
        matrices = {"lowpass": (lambda: M.lowpass_operator(T, 8), True, True), "blur": (lambda: M.gaussian_blur_operator(T, 2.0, 4), True, False),
                    "time_full": (lambda: M.gaussian_blur_operator(T, 0.8, 1), False, False)}
        runs, rec = {}, {"shape": name, "T": T, "C": C, "B": B, "steps": N}
        for v in args.variants:
            if v == "agg4":
                y = M.window_means(fine, 4)
                mask = torch.from_numpy(rs.rand(*y.shape) < 0.5)
                kw = dict(fourier_transform=True, feature_mean=mean, feature_std=std, aggregate=4)
            else:
                make, fourier, row_mask = matrices[v]
                t0 = time.perf_counter()
                op = M.LinearOperator(make())
                rec[f"{v}_M"], rec[f"{v}_cond"], rec[f"{v}_host_svd_ms"] = op.M, op.condition, 1e3 * (time.perf_counter() - t0)
                y = M.apply_operator(fine, op).float()
                mask = torch.from_numpy(rs.rand(*y.shape) < 0.5) if row_mask else rows.expand(B, op.M, C).contiguous()
                kw = dict(fourier_transform=fourier, feature_mean=mean, feature_std=std, operator=op)
                if not args.no_build:        # a fresh operator: first projection (upload, basis build, wait) against the second
                    x = torch.from_numpy(rs.randn(B, T, C)).float()
                    x0 = s.observed_to_sample_space(y, mask, **kw)
                    pk = dict(fourier_transform=fourier, feature_std=std, operator=op)
                    s.impute_project(x, x, torch.ones(T, C, dtype=torch.bool), None, fourier_transform=fourier,
                                     feature_std=std)                                          # (code objects and the context's own tables)
                    s.impute_project(x, x0, mask, None, fourier_transform=fourier, feature_std=std, operator=M.LinearOperator(op.P))
                    first = timed(lambda: s.impute_project(x, x0, mask, None, **pk))
                    second = timed(lambda: s.impute_project(x, x0, mask, None, **pk))
                    rec[f"{v}_build_ms"] = 1e3 * (first - second)
            if "replace" in args.conditionings:
                runs[f"replace_{v}"] = lambda y=y, mask=mask, kw=kw: s.impute(y, mask, N, **kw)
            if "dps" in args.conditionings:
                runs[f"dps_{v}"] = lambda y=y, mask=mask, kw=kw: s.impute(y, mask, N, conditioning="dps", guidance_scale=1.0,
                                                                         guidance_jacobian=False, **kw)
        for fn in runs.values():                                                              # warm-up (code objects, bases, buffers)
            fn()
        times = {k: [] for k in runs}
        for _ in range(args.reps):                                                            # alternate the variants
            for k, fn in runs.items():
                times[k].append(timed(fn))
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
