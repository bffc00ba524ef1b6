#!/usr/bin/env python3
"""What TemporalDependence is for: a generator that emits i.i.d. noise with the right marginal variance in place of an AR(1)
process.  800 real AR(1) series (phi = 0.8, T = 100) against 400 N(0, 1 / (1 - phi^2)) series and against 400 fresh AR(1) series,
through a MetricCollection of MarginalWasserstein and TemporalDependence: the marginal distance of the noise sits near its `_self`
baseline, the autocorrelation difference does not.  Prints the keys side by side; --out also writes them."""
from __future__ import annotations

import argparse
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PHI, T, LAGS = 0.8, 100, 25


def ar1(rng, n):
    x = np.empty((n, T))
    x[:, 0] = rng.standard_normal(n) / np.sqrt(1 - PHI * PHI)
    eps = rng.standard_normal((n, T))
    for t in range(1, T):
        x[:, t] = PHI * x[:, t - 1] + eps[:, t]
    return x[:, :, None].astype(np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    from fourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, TemporalDependence
    rng = np.random.default_rng(args.seed)
    real = ar1(rng, 800)
    noise = (rng.standard_normal((400, T, 1)) / np.sqrt(1 - PHI * PHI)).astype(np.float32)
    fresh = ar1(rng, 400)
    coll = MetricCollection(metrics=[partial(MarginalWasserstein, random_seed=0), partial(TemporalDependence, lags=LAGS)],
                            original_samples=torch.from_numpy(real))
    res_noise, res_fresh = coll(torch.from_numpy(noise)), coll(torch.from_numpy(fresh))
    keys = ["time_marginal_wasserstein_mean", "time_acf_distance", "time_acf_distance_max", "time_acf_marginal_wasserstein_mean",
            "time_skewness_distance", "time_kurtosis_distance"]
    lines = [f"# scripts/dependence_demo.py: AR(1) phi = {PHI}, T = {T}, lags = {LAGS}, seed {args.seed}; {torch.cuda.get_device_name(0)}",
             f"{'key':42s} {'iid noise':>12s} {'fresh AR(1)':>12s} {'_self':>12s}"]
    for key in keys:
        base = res_noise.get(f"{key}_self", float("nan"))
        lines.append(f"{key:42s} {res_noise[key]:12.5f} {res_fresh[key]:12.5f} {base:12.5f}")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
