#!/usr/bin/env python3
"""ms per score evaluation of DiffusionSampler.log_likelihood (fd_likelihood_run: training forward + input-only VJP + the fused
stage kernel k_ll_stage) on the default-width model (D = 72, L = 10, H = 12), random weights, at the ecg shape (T = 100, C = 12)
and at a T = 252 training shape (C = 8), in bf16 and fp32, with its pieces timed alone: the training forward (dropout 0), forward +
fd_score_input_vjp, and forward + fd_score_backward (the parameter backward the VJP is compared against) at the same B.  The
stage's share is the evaluation minus forward + VJP.  Runs alternated over `--reps` rounds, the median kept.  One JSON line per
(shape, precision); `--out FILE` also writes them as a JSON list.

`--rk45 RTOL` times the adaptive solver instead (fd_likelihood_run_adaptive, k_ll_rk_stage) against Heun at the same B, in ms per
launched score evaluation: rk45 launches 2 + 6 attempts, one attempt more than its slowest row needs (the host reads the running-
row count of attempt k while attempt k + 1 runs).  waste = 1 - sum of per-row nfe / (B x launched evaluations): the share of
row-evaluations spent on rows already finished."""
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


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=40, help="Euler steps (= score evaluations) per likelihood run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", choices=["ecg", "t252"], default=None)
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    ap.add_argument("--rk45", type=float, default=None, help="time solver='rk45' at this rtol = atol against Heun")
    args = ap.parse_args()
    if args.rk45 is not None:
        return bench_rk45(args)
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    from tests.gpu_util import make_model
    shapes = {"ecg": dict(T=100, C=12, D=72, L=10, H=12), "t252": dict(T=252, C=8, D=72, L=10, H=12)}
    B, E = args.batch, args.evals
    out = []
    for name, cfg in shapes.items():
        if args.only and name != args.only:
            continue
        for prec in ("bf16", "fp32"):
            m, _, _ = make_model(cfg, precision=prec)
            m.dropout = 0.0
            s = DiffusionSampler(score_model=m, sample_batch_size=B)
            g = torch.Generator().manual_seed(0)
            X = torch.randn((B, cfg["T"], cfg["C"]), generator=g)
            xd = X.cuda()
            td = torch.full((B,), 0.5, device="cuda")
            d = torch.randn_like(xd)
            batch = DiffusableBatch(X=xd, timesteps=td)

            def fwd():
                m.train()
                m(batch)

            def fwd_vjp():
                fwd()
                m.input_vjp(d)

            def fwd_bwd():
                fwd()
                m.backward(d, accumulate=False)

            runs = {"forward": lambda: timed(fwd, 20), "forward_vjp": lambda: timed(fwd_vjp, 20),
                    "forward_backward": lambda: timed(fwd_bwd, 20),
                    "likelihood_eval": lambda: timed(lambda: s.log_likelihood(X, E, "euler", seed=1), 1) / E}
            for fn in runs.values():      # warm-up: images, workspace, buffers
                fn()
            times = {k: [] for k in runs}
            for _ in range(args.reps):
                for k, fn in runs.items():
                    times[k].append(fn())
            rec = {"shape": name, "T": cfg["T"], "C": cfg["C"], "B": B, "precision": prec, "train_mode": m.train_mode_effective,
                   "evals": E, "reps": args.reps}
            for k, v in times.items():
                rec[f"{k}_ms"] = 1e3 * statistics.median(v)
            rec["vjp_ms"] = rec["forward_vjp_ms"] - rec["forward_ms"]
            rec["backward_ms"] = rec["forward_backward_ms"] - rec["forward_ms"]
            rec["vjp_over_backward"] = rec["vjp_ms"] / rec["backward_ms"]
            rec["stage_and_host_ms"] = rec["likelihood_eval_ms"] - rec["forward_vjp_ms"]
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def bench_rk45(args) -> None:
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    shapes = {"ecg": dict(T=100, C=12, D=72, L=10, H=12), "t252": dict(T=252, C=8, D=72, L=10, H=12)}
    B, E, tol = args.batch, args.evals, args.rk45
    out = []
    for name, cfg in shapes.items():
        if args.only and name != args.only:
            continue
        for prec in ("bf16", "fp32"):
            m, _, _ = make_model(cfg, precision=prec)
            s = DiffusionSampler(score_model=m, sample_batch_size=B)
            X = torch.randn((B, cfg["T"], cfg["C"]), generator=torch.Generator().manual_seed(0))
            res = {}

            def heun():
                return timed(lambda: s.log_likelihood(X, E // 2, "heun", seed=1), 1) / (2 * (E // 2))

            def rk45():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res["r"] = s.log_likelihood(X, solver="rk45", rtol=tol, atol=tol, seed=1)
                torch.cuda.synchronize()
                launched = int(res["r"].nfe.max()) + 6
                return (time.perf_counter() - t0) / launched
            heun(), rk45()      # warm-up
            times = {"heun": [], "rk45": []}
            for _ in range(args.reps):
                times["heun"].append(heun())
                times["rk45"].append(rk45())
            r = res["r"]
            launched = int(r.nfe.max()) + 6
            rec = {"shape": name, "T": cfg["T"], "C": cfg["C"], "B": B, "precision": prec, "rtol": tol, "reps": args.reps,
                   "heun_ms_per_eval": 1e3 * statistics.median(times["heun"]), "rk45_ms_per_eval": 1e3 * statistics.median(times["rk45"]),
                   "nfe_mean": float(r.nfe.double().mean()), "nfe_max": int(r.nfe.max()), "launched_evals": launched,
                   "waste": 1.0 - float(r.nfe.double().sum()) / (B * launched), "n_not_converged": int((~r.converged).sum())}
            rec["rk45_over_heun"] = rec["rk45_ms_per_eval"] / rec["heun_ms_per_eval"]
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
