#!/usr/bin/env python3
"""What SignatureDistance is for: a generator that plays its series BACKWARDS.  400 real series (T = 100): a stationary sawtooth with
a slow rise and a fast fall (period 37: the window is not a whole number of periods, see --period), a random phase and noise of
deviation 0.05.  Against them 400 fresh sawtooths played backwards and 400
fresh sawtooths as they are, through a MetricCollection of MarginalWasserstein, TemporalDependence and SignatureDistance (depth 4, time
channel): a reversed series has the same marginals, the same autocorrelation and the same spectrum, so the first two sit near their
`_self` baselines; the expected signature does not.  Prints the keys side by side; --out also writes them.

--period 25 shows the statistic's blind spot: over a whole number of periods the net increment of the wave is noise alone, its odd
moments -- through which a time-augmented signature of a stationary series sees the reversal most strongly -- vanish, and sig_w1 of
the reversed set falls to 1.3 times its baseline (0.24 against 0.18, seed 2025)."""
from __future__ import annotations

import argparse
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

T, RISE, PERIOD, NOISE, DEPTH = 100, 0.8, 37.0, 0.05, 4


def sawtooth(rng, n, period=PERIOD):
    phase = rng.uniform(0.0, 1.0, size=(n, 1))
    u = (np.arange(T)[None, :] / period + phase) % 1.0
    wave = np.where(u < RISE, u / RISE, (1.0 - u) / (1.0 - RISE))
    return (wave + NOISE * rng.standard_normal((n, T)))[:, :, None].astype(np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--period", type=float, default=PERIOD)
    args = ap.parse_args()
    period = args.period
    from fourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SignatureDistance, TemporalDependence
    rng = np.random.default_rng(args.seed)
    real = sawtooth(rng, 400, period)
    backwards = sawtooth(rng, 400, period)[:, ::-1].copy()
    fresh = sawtooth(rng, 400, period)
    coll = MetricCollection(metrics=[partial(MarginalWasserstein, random_seed=0), partial(TemporalDependence, lags=T // 4),
                                     partial(SignatureDistance, depth=DEPTH)], original_samples=torch.from_numpy(real))
    res_back, res_fresh = coll(torch.from_numpy(backwards)), coll(torch.from_numpy(fresh))
    keys = ["time_marginal_wasserstein_mean", "time_acf_distance", "time_acf_distance_max", "time_skewness_distance", "time_sig_w1",
            "time_sig_mmd2"]
    lines = [f"# scripts/signature_demo.py: sawtooth rise {RISE}, period {period}, noise {NOISE}, T = {T}, depth {DEPTH}, seed "
             f"{args.seed}; {torch.cuda.get_device_name(0)}",
             f"{'key':36s} {'played backwards':>17s} {'fresh':>12s} {'_self':>12s}"]
    for key in keys:
        lines.append(f"{key:36s} {res_back[key]:17.5f} {res_fresh[key]:12.5f} {res_back.get(f'{key}_self', float('nan')):12.5f}")
    for tag, res in (("played backwards", res_back), ("fresh", res_fresh), ("_self", {"time_sig_w1_levels": res_back["time_sig_w1_levels_self"]})):
        lines.append(f"time_sig_w1_levels, {tag}: " + " ".join(f"{v:.5f}" for v in res["time_sig_w1_levels"]))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
