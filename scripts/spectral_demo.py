#!/usr/bin/env python3
"""What SpectralDependence is for: a generator whose channels have the right spectra and no relation to one another.  512 real series
of shape (128, 2): channel 0 is AR(1) with phi = 0.5, channel 1 is channel 0 delayed by 20 steps plus noise of deviation 0.3.  The
fake set has the same two marginal processes, independent of each other.  The delay is beyond TemporalDependence's 8 cross lags and
the marginal spectra are equal by construction, so ccf_distance, acf_distance and psd_log_distance sit near their `_self`
baselines; the set-level coherence does not.  Prints the keys side by side for nperseg 64 and 128; --out also writes them."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, T, DELAY, PHI, NOISE = 512, 128, 20, 0.5, 0.3


def ar1(rng, n, length):
    x = np.empty((n, length))
    x[:, 0] = rng.standard_normal(n) / np.sqrt(1 - PHI * PHI)
    eps = rng.standard_normal((n, length))
    for t in range(1, length):
        x[:, t] = PHI * x[:, t - 1] + eps[:, t]
    return x


def coupled(rng, source):
    """(n, T, 2): the source from DELAY on, and the source DELAY steps late plus noise."""
    return np.stack([source[:, DELAY:], source[:, :T] + NOISE * rng.standard_normal((len(source), T))], axis=-1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from fourierdiffusion_amd.sampling.metrics import SpectralDependence, TemporalDependence
    rng = np.random.default_rng(args.seed)
    real = coupled(rng, ar1(rng, N, T + DELAY)).astype(np.float32)
    fake = np.stack([ar1(rng, N, T + DELAY)[:, DELAY:], coupled(rng, ar1(rng, N, T + DELAY))[..., 1]], axis=-1).astype(np.float32)
    real, fake = torch.from_numpy(real), torch.from_numpy(fake)
    lines = [f"# scripts/spectral_demo.py: {N} series of ({T}, 2), delay {DELAY}, seed {args.seed}; {torch.cuda.get_device_name(0)}",
             f"{'key':44s} {'fake':>12s} {'_self':>12s}"]
    temporal = TemporalDependence(real)
    res, base = temporal(fake), temporal.baseline_metrics
    for key in ("acf_distance", "ccf_distance", "ccf_distance_max"):
        lines.append(f"{'temporal ' + key:44s} {res[key]:12.5f} {base[key + '_self']:12.5f}")
    for nperseg in (64, 128):
        spectral = SpectralDependence(real, nperseg=nperseg)
        res, base = spectral(fake), spectral.baseline_metrics
        for key in ("psd_log_distance", "coherence_distance", "coherence_distance_max", "phase_distance",
                    "spectral_centroid_wasserstein", "spectral_entropy_wasserstein"):
            lines.append(f"{'spectral nperseg=' + str(nperseg) + ' ' + key:44s} {res[key]:12.5f} {base[key + '_self']:12.5f}")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
