#!/usr/bin/env python3
"""What the sliced Wasserstein distance cannot see: the synthetic datamodule's sines, 1000 training series, and three
"generators" of 500 samples each, scored by the nearest-neighbour metrics (sampling/metrics.py: PrecisionRecall, Memorisation) and
by the sliced Wasserstein distance in the time domain:

  (a) held-out  real series the "model" never saw (half of the test split; the other half is the holdout of the memorisation metric)
  (b) replay    training rows with a jitter of 1e-3
  (c) collapse  one training row, repeated

Prints one table; --out also writes it to a file."""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

COLUMNS = ["sliced_wasserstein_mean", "precision", "recall", "density", "coverage", "authenticity", "nn_distance_median",
           "train_closer_share"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticDatamodule
    from fourierdiffusion_amd.sampling.metrics import Memorisation, PrecisionRecall, SlicedWasserstein
    with tempfile.TemporaryDirectory() as tmp:
        dm = SyntheticDatamodule(data_dir=tmp, max_len=100, num_samples=1000, n_channels=1)
        dm.prepare_data()
        dm.setup()
    train, holdout, unseen = dm.X_train, dm.X_test[:500], dm.X_test[500:]
    g = torch.Generator().manual_seed(0)
    generators = {
        "(a) held-out": unseen,
        "(b) replay": train[:500] + 1e-3 * torch.randn(train[:500].shape, generator=g),
        "(c) collapse": train[:1].repeat(500, 1, 1),
    }
    metrics = [SlicedWasserstein(original_samples=train, random_seed=42, num_directions=200),
               PrecisionRecall(original_samples=train, k=5), Memorisation(original_samples=train, holdout_samples=holdout)]
    base = metrics[0].baseline_metrics
    lines = [f"# scripts/memorisation_demo.py: synthetic sines, T = 100, 1000 training series, 500 samples per generator, holdout 500; "
             f"{torch.cuda.get_device_name(0)}",
             f"# sliced Wasserstein of two real folds (the `_self` baseline): {base['sliced_wasserstein_mean_self']:.4f}; of the average "
             f"sample (`_dummy`): {base['sliced_wasserstein_mean_dummy']:.4f}",
             "generator      | " + " | ".join(COLUMNS)]
    for name, samples in generators.items():
        res = {}
        for metric in metrics:
            res.update(metric(samples))
        lines.append(f"{name:<14} | " + " | ".join(f"{res[c]:{len(c)}.4f}" for c in COLUMNS))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
