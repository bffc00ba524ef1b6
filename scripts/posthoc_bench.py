#!/usr/bin/env python3
"""Wall time of one post-hoc fit (utils/posthoc.py, csrc/fd_posthoc.hip) of 2000 steps at the two dataset shapes that bracket its work:

  ecg     series of (187, 1): a long recurrence, little per step
  mimic   series of (24, 40): a short recurrence, wide rows

at the defaults of the scores (d_model 32, one layer, batches of 128, lr 1e-3), for both tasks.  Two drivers of the SAME loop:

  one_call   fd_posthoc_fit: every step enqueued from C, one engine call per fit
  stepwise   the loop driven from Python, five ctypes calls per step (batch, training forward, head, backward, AdamW)

Both produce the same bits (checked here on the loss trace).  Timed is the whole `fit` call with a host clock, ending in a device
synchronise, after a warm-up fit of each driver; the drivers alternate, `--runs` fits each; best and spread are reported.  Raw lines go
to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CASES = {"ecg": (187, 1), "mimic": (24, 40)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--pool", type=int, default=4096, help="series per pool")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from fourierdiffusion_amd.utils.posthoc import PosthocNetwork, channel_stats
    dev = torch.device("cuda", 0)
    lines = [f"# scripts/posthoc_bench.py: {torch.cuda.get_device_name(0)}; seconds per fit of {args.steps} steps (host clock around the "
             f"call and a device synchronise), best of {args.runs}"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, (T, C) in CASES.items():
        a = torch.cumsum(torch.randn((args.pool, T, C), device=dev, generator=gen), dim=1) * 0.3
        b = torch.randn((args.pool, T, C), device=dev, generator=gen)
        mean, inv = channel_stats(a)
        for task in ("classify", "predict"):
            def fit(fused, steps):
                net = PosthocNetwork(C, T, seed=0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = net.fit(task, a, b if task == "classify" else None, steps=steps, batch_size=128, lr=1e-3, mean=mean, inv_std=inv,
                               fused=fused)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, loss

            fit(True, 50), fit(False, 50)
            times = {True: [], False: []}
            traces = {}
            for _ in range(args.runs):
                for fused in (True, False):
                    t, traces[fused] = fit(fused, args.steps)
                    times[fused].append(t)
            one, step = times[True], times[False]
            rec = {"case": name, "T": T, "C": C, "task": task, "steps": args.steps, "batch_size": 128, "d_model": 32,
                   "one_call_s": [round(t, 4) for t in one], "stepwise_s": [round(t, 4) for t in step],
                   "one_call_best_s": round(min(one), 4), "stepwise_best_s": round(min(step), 4),
                   "one_call_spread_s": round(max(one) - min(one), 4), "stepwise_spread_s": round(max(step) - min(step), 4),
                   "one_call_ms_per_step": round(1e3 * min(one) / args.steps, 4),
                   "stepwise_over_one_call": round(min(step) / min(one), 3),
                   "loss_traces_bit_equal": bool(torch.equal(traces[True], traces[False])),
                   "loss_first": float(traces[True][0]), "loss_last": float(traces[True][-1])}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
