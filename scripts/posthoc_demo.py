#!/usr/bin/env python3
"""What the two post-hoc scores (utils/posthoc.py) say about generators whose quality is known: an AR(1) process with phi = 0.9 and
unit marginal variance stands for the real data; the "generators" are a second draw of the same process (perfect), the process with
a wrong phi, and white noise (useless).

  discriminative score   about 0 for the second draw, 0.5 for noise
  predictive score       the one-step floor 0.798 sqrt(1 - phi^2) = 0.348 for the second draw; 0.798 (predicting zero) for noise

The table of the acceptance tests (tests/test_gpu_posthoc.py) at a larger size.  Lines go to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def ar1(n, T, C, phi, rng):
    e = rng.standard_normal((n, T, C))
    x = np.empty((n, T, C))
    x[:, 0] = e[:, 0]
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + np.sqrt(1.0 - phi * phi) * e[:, t]
    return x.astype(np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--length", type=int, default=48)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--seeds", type=int, default=3)
    args = ap.parse_args()
    from fourierdiffusion_amd.utils.posthoc import discriminative_score, predictive_score
    n, T, C = args.n, args.length, args.channels
    knobs = dict(steps=args.steps, batch_size=128, lr=1e-2, d_model=32, num_layers=1)
    lines = [f"# scripts/posthoc_demo.py: real = AR(1), phi 0.9; n={n} T={T} C={C}, {args.steps} steps; floor "
             f"{0.798 * np.sqrt(1 - 0.81):.3f}, predicting zero 0.798"]
    print(lines[0], flush=True)
    for seed in range(args.seeds):
        rng = np.random.default_rng(seed)
        real = ar1(n, T, C, 0.9, rng)
        generators = {"second draw (phi 0.9)": ar1(n, T, C, 0.9, rng), "wrong phi (0.5)": ar1(n, T, C, 0.5, rng),
                      "white noise": rng.standard_normal((n, T, C)).astype(np.float32)}
        for name, fake in generators.items():
            d = discriminative_score(real, fake, seed=seed, **knobs)
            p = predictive_score(fake, real, stats_from=real, seed=seed, **knobs)
            rec = {"seed": seed, "generator": name, "discriminative_score": round(d["score"], 4), "accuracy": round(d["accuracy"], 4),
                   "predictive_score": round(p["mae"], 4)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
