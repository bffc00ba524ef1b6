#!/usr/bin/env python3
"""Cost of the adaptive (RK45) ODE sampler (DiffusionSampler.sample_ode_adaptive, fd_sampler_run_ode_adaptive) on the default-width
model (D = 72, L = 10, H = 12), random weights, at the bench shape (T = 100, C = 12) with B = 200 rows, in bf16 and fp32:

* ms per launched evaluation (compaction off: every evaluation runs B rows) against ms per evaluation of the step-by-step Heun loop
  (fd_sampler_ode_loop with the persistent kernel off, FDIFF_SAMPLER_STEPWISE) -- the same forward, a lighter stage kernel and no
  host synchronisation -- and against the inference forward alone; the evaluation minus the forward is the stage kernel's and the
  host loop's share;
* row-evaluations launched over needed, and wall time, with compaction off and at each granule of `--granules`;
* for scale, the wall time of Heun-50 and DPM-Solver++-20 through their default path (the persistent kernel in bf16) on the same B.

Runs alternated over `--reps` rounds, the median kept.  One JSON line per (precision, tolerance); `--out FILE` writes them as well.

The stage kernel's own share needs a kernel trace, in a run of its own: `--trace bf16:1e-5` does nothing but a warm-up and `--reps`
uncompacted adaptive runs, to be started under a kernel tracer (rocprofv3 --kernel-trace --stats --output-format csv -- python
scripts/ode_adaptive_bench.py --trace ...), and `--stage-share KERNEL_STATS_CSV` reads the tracer's per-kernel totals and prints
k_ode_rk_stage's calls, mean time and share of all kernel time of that run."""
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


class env:
    """Sets environment variables for a block (the engine reads them at every call)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def trace_run(args) -> None:
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    prec, tol = args.trace.split(":")
    cfg, B = dict(T=100, C=12, D=72, L=10, H=12), args.batch
    m, _, _ = make_model(cfg, precision=prec)
    m.eval()
    s = DiffusionSampler(score_model=m, sample_batch_size=B, merge_batches=False)
    z = [torch.randn((B, cfg["T"], cfg["C"]), generator=torch.Generator().manual_seed(0)).cuda()]
    with env(FDIFF_RK_COMPACT="0"):
        for _ in range(1 + args.reps):
            _, info = s.sample_ode_adaptive(B, rtol=float(tol), atol=float(tol), prior_noise=z, return_info=True)
    torch.cuda.synchronize()
    print(json.dumps({"trace": args.trace, "B": B, "runs": 1 + args.reps, "evals_per_run": info.row_evals_launched // B}), flush=True)


def stage_share(path) -> None:
    import csv
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    name = next(k for k in rows[0] if k.lower() == "name")
    total = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    calls = next(k for k in rows[0] if k.lower() == "calls")
    all_ns = sum(float(r[total]) for r in rows)
    st = [r for r in rows if "k_ode_rk_stage" in r[name]]
    ns, n = sum(float(r[total]) for r in st), sum(int(r[calls]) for r in st)
    print(json.dumps({"stats": os.path.basename(path), "k_ode_rk_stage_calls": n, "k_ode_rk_stage_mean_us": 1e-3 * ns / max(n, 1),
                      "all_kernels_ms": 1e-6 * all_ns, "k_ode_rk_stage_share_of_kernel_time": ns / all_ns}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tols", default="1e-3,1e-5")
    ap.add_argument("--granules", default="1,8,25,50,100")
    ap.add_argument("--heun-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, metavar="PRECISION:TOL", help="only warm-up + --reps uncompacted adaptive runs (for a kernel tracer)")
    ap.add_argument("--stage-share", default=None, metavar="CSV", help="per-kernel totals of a traced run -> the stage kernel's share")
    args = ap.parse_args()
    if args.stage_share:
        return stage_share(args.stage_share)
    if args.trace:
        return trace_run(args)
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    from tests.gpu_util import make_model
    cfg = dict(T=100, C=12, D=72, L=10, H=12)
    B, N = args.batch, args.heun_steps
    granules = [int(g) for g in args.granules.split(",")]
    out = []
    for prec in ("bf16", "fp32"):
        m, _, _ = make_model(cfg, precision=prec)
        m.eval()
        s = DiffusionSampler(score_model=m, sample_batch_size=B, merge_batches=False)
        z = [torch.randn((B, cfg["T"], cfg["C"]), generator=torch.Generator().manual_seed(0)).cuda()]
        batch = DiffusableBatch(X=z[0].clone(), timesteps=torch.full((B,), 0.5, device="cuda"))

        def forward():
            return wall(lambda: [m(batch) for _ in range(20)])[0] / 20

        def heun_stepwise():
            with env(FDIFF_SAMPLER_STEPWISE="1"):
                return wall(lambda: s.sample_ode(B, N, solver="heun", prior_noise=z))[0] / (2 * N)

        def fixed(solver, n, schedule):
            return wall(lambda: s.sample_ode(B, n, solver=solver, schedule=schedule, prior_noise=z))[0]

        for tol in (float(t) for t in args.tols.split(",")):
            def adaptive(granule):
                e = dict(FDIFF_RK_COMPACT="0") if granule == 0 else dict(FDIFF_RK_COMPACT=None)
                with env(**e):
                    return wall(lambda: s.sample_ode_adaptive(B, rtol=tol, atol=tol, prior_noise=z, return_info=True,
                                                              compact_granule=granule))
            runs = {"forward": forward, "heun_stepwise": heun_stepwise, "heun50": lambda: fixed("heun", 50, "time"),
                    "dpmpp2m20": lambda: fixed("dpmpp2m", 20, "logsnr")}
            for fn in runs.values():      # warm-up: images, workspace, buffers
                fn()
            info = {g: adaptive(g)[1][1] for g in [0] + granules}
            times = {k: [] for k in list(runs) + [f"rk45_g{g}" for g in [0] + granules]}
            for _ in range(args.reps):
                for k, fn in runs.items():
                    times[k].append(fn())
                for g in [0] + granules:
                    times[f"rk45_g{g}"].append(adaptive(g)[0])
            med = {k: statistics.median(v) for k, v in times.items()}
            i0 = info[0]
            evals = i0.row_evals_launched // B      # compaction off: every evaluation ran B rows
            rec = {"T": cfg["T"], "C": cfg["C"], "B": B, "precision": prec, "rtol": tol, "reps": args.reps,
                   "nfe_mean": float(i0.nfe.double().mean()), "nfe_max": int(i0.nfe.max()), "n_not_converged": int((~i0.converged).sum()),
                   "evals_launched_uncompacted": evals,
                   "forward_ms": 1e3 * med["forward"], "heun_stepwise_ms_per_eval": 1e3 * med["heun_stepwise"],
                   "rk45_ms_per_eval": 1e3 * med["rk45_g0"] / evals}
            rec["rk45_over_heun_stepwise"] = rec["rk45_ms_per_eval"] / rec["heun_stepwise_ms_per_eval"]
            rec["stage_and_host_share"] = 1.0 - rec["forward_ms"] / rec["rk45_ms_per_eval"]
            rec["compaction"] = [{"granule": g, "wall_ms": 1e3 * med[f"rk45_g{g}"], "row_evals_launched": info[g].row_evals_launched,
                                  "launched_over_needed": info[g].row_evals_launched / info[g].row_evals_needed,
                                  "same_nfe_as_off": bool(torch.equal(info[g].nfe, i0.nfe))} for g in [0] + granules]
            rec["rk45_ms_per_series"] = min(c["wall_ms"] for c in rec["compaction"]) / B
            rec["heun50_ms_per_series"] = 1e3 * med["heun50"] / B
            rec["dpmpp2m20_ms_per_series"] = 1e3 * med["dpmpp2m20"] / B
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
