#!/usr/bin/env python3
"""The shifted-replay experiment on the `synthetic` datamodule, through MetricCollection: what the Euclidean memorisation metric
says about a generator that replays its training series a few samples late, and what the DTW one says.

  replay  every training series delayed by --shift samples, its first value repeated (a copy for every practical purpose)
  fresh   one half of the datamodule's held-out split (independent draws of the same process); the other half is the holdout

Both sets go through one collection holding PrecisionRecall / Memorisation and DTWPrecisionRecall / DTWMemorisation (window
--window, None = ceil(0.1 T)); the table prints the time-view keys side by side.  The data is written to --data-dir on first use
(the synthetic datamodule generates it; nothing is downloaded)."""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-samples", type=int, default=500)
    ap.add_argument("--max-len", type=int, default=100)
    ap.add_argument("--n-channels", type=int, default=1)
    ap.add_argument("--shift", type=int, default=3)
    ap.add_argument("--window", type=int, default=None)
    ap.add_argument("--data-dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticDatamodule
    from fourierdiffusion_amd.sampling.metrics import DTWMemorisation, DTWPrecisionRecall, Memorisation, MetricCollection, PrecisionRecall
    from fourierdiffusion_amd.utils.dtw import default_window
    data_dir = args.data_dir or os.path.join(tempfile.gettempdir(), "fdiff_dtw_replay_demo")
    dm = SyntheticDatamodule(data_dir=data_dir, random_seed=42, max_len=args.max_len, num_samples=args.num_samples,
                             n_channels=args.n_channels)
    dm.prepare_data()
    dm.setup()
    half = dm.X_test.shape[0] // 2
    train, held, fresh = dm.X_train, dm.X_test[:half].contiguous(), dm.X_test[half:].contiguous()
    replay = torch.cat([train[:, :1].expand(-1, args.shift, -1), train[:, : args.max_len - args.shift]], dim=1).contiguous()
    w = default_window(args.max_len) if args.window is None else args.window
    collection = MetricCollection(
        metrics=[partial(PrecisionRecall, k=5), partial(Memorisation), partial(DTWPrecisionRecall, k=5, window=w),
                 partial(DTWMemorisation, window=w)],
        original_samples=train, holdout_samples=held)
    results = {"replay": collection(replay), "fresh": collection(fresh)}
    keys = ["authenticity", "train_closer_share", "nn_distance_median", "precision", "recall", "coverage"]
    lines = [f"# scripts/dtw_replay_demo.py: synthetic datamodule, {args.num_samples} training series of shape ({args.max_len}, "
             f"{args.n_channels}), replays delayed by {args.shift} samples, window {w}",
             f"{'key (time view)':24s} {'replay euclid':>14s} {'replay dtw':>12s} {'fresh euclid':>14s} {'fresh dtw':>12s}"]
    for key in keys:
        lines.append(f"{key:24s} {results['replay']['time_' + key]:14.4f} {results['replay']['time_dtw_' + key]:12.4f} "
                     f"{results['fresh']['time_' + key]:14.4f} {results['fresh']['time_dtw_' + key]:12.4f}")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
