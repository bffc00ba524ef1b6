#!/usr/bin/env python3
"""Wall time of one K-way post-hoc fit (`fd_posthoc_fit_multiclass`, utils/posthoc.py) of 2000 steps at the two dataset shapes that
bracket its work, next to the binary task of `fd_posthoc_fit` at the same shapes:

  ecg     series of (187, 1), K = 5: a long recurrence, little per step; the network widens from 1 to 5 channels
  mimic   series of (24, 40), K = 3: a short recurrence, wide rows; the network keeps its 40 channels

at the defaults of the scores (d_model 32, one layer, batches of 128, lr 1e-3).  The binary task is the comparison point, not a
target: it draws from two pools and reduces the last step to one logit, the K-way task draws from one labelled pool (uniformly, or
class by class: the `balanced` rows) and carries K logits.

Timed is the whole `fit` call with a host clock, ending in a device synchronise, after a warm-up fit of each variant; the variants
alternate, `--runs` fits each; best and spread are reported, with the date and the shader clock the board reported while the case
ran (bench.py's `BoardSampler`, hwmon; null where the node is missing).  The K-way fit's time includes its host-side label check
and class tables.  Raw lines go to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CASES = {"ecg": (187, 1, 5), "mimic": (24, 40, 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--pool", type=int, default=4096, help="series per pool")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from bench import BoardSampler
    from fourierdiffusion_amd.utils.posthoc import PosthocNetwork, channel_stats
    dev = torch.device("cuda", 0)
    date = time.strftime("%Y-%m-%d")
    lines = [f"# scripts/classification_bench.py: {torch.cuda.get_device_name(0)}; seconds per fit of {args.steps} steps (host clock "
             f"around the call and a device synchronise), best of {args.runs}, variants alternating"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, (T, C, K) in CASES.items():
        a = torch.cumsum(torch.randn((args.pool, T, C), device=dev, generator=gen), dim=1) * 0.3
        b = torch.randn((args.pool, T, C), device=dev, generator=gen)
        ya = torch.randint(0, K, (args.pool,), device=dev, generator=gen)
        a = a * (1.0 + ya.float())[:, None, None] / K          # the class sets the scale, so there is something to learn
        mean, inv = channel_stats(a)

        def fit(variant, steps):
            multi = variant != "binary"
            net = PosthocNetwork(C, T, seed=0, n_classes=K if multi else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if multi:
                loss = net.fit("multiclass", a, labels=ya, balance=variant == "balanced", steps=steps, batch_size=128, lr=1e-3, mean=mean,
                               inv_std=inv)
            else:
                loss = net.fit("classify", a, b, steps=steps, batch_size=128, lr=1e-3, mean=mean, inv_std=inv)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, loss

        variants = ("binary", "uniform", "balanced")
        for v in variants:
            fit(v, 50)
        times = {v: [] for v in variants}
        traces = {}
        board = BoardSampler()
        board.start()
        for _ in range(args.runs):
            for v in variants:
                t, traces[v] = fit(v, args.steps)
                times[v].append(t)
        clock = board.stop() or {}
        for v in variants:
            ts = times[v]
            rec = {"case": name, "T": T, "C": C, "K": K if v != "binary" else None, "task": "classify" if v == "binary" else "multiclass",
                   "draw": v, "net_channels": max(C, K) if v != "binary" else C, "steps": args.steps, "batch_size": 128, "d_model": 32,
                   "fit_s": [round(t, 4) for t in ts], "best_s": round(min(ts), 4), "spread_s": round(max(ts) - min(ts), 4),
                   "ms_per_step": round(1e3 * min(ts) / args.steps, 4), "over_binary": round(min(ts) / min(times["binary"]), 3),
                   "loss_first": float(traces[v][0]), "loss_last": float(traces[v][-1]), "date": date,
                   "sclk_mhz_mean": clock.get("sclk_mhz_mean"), "sclk_mhz_min": clock.get("sclk_mhz_min")}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
