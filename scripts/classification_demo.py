#!/usr/bin/env python3
"""What ClassificationScore (sampling/metrics.py, utils/posthoc.py) says about conditional generators whose label fidelity is known,
on the labelled sines of `datamodule=synthetic_classes` (1000 training series of (100, 1), 3 classes that set the frequency band).
The training split is the real set, the test split the hold-out; three stand-ins for a generator are made of a fresh draw of the
same process:

  right labels       real series with their classes: a perfect conditional generator
  permuted labels    the same series with the classes shuffled: samples that ignore the class they were asked for
  one class          series of class 0 only, handed out under every label: a generator that collapsed onto one class

Every score key of the metric goes out as one JSON line per stand-in, to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from fourierdiffusion_amd.dataloaders.datamodules import SyntheticClassesDatamodule
    from fourierdiffusion_amd.sampling.metrics import ClassificationScore, MetricCollection

    def split(seed):
        dm = SyntheticClassesDatamodule(data_dir=tempfile.mkdtemp(prefix="classification_demo_"), random_seed=seed, batch_size=64,
                                        max_len=100, num_samples=1000, n_channels=1, n_classes=3)
        dm.prepare_data()
        dm.setup()
        return dm

    dm, fresh = split(42), split(43)
    knobs = dict(steps=args.steps, batch_size=128, lr=1e-2, d_model=32, num_layers=1, random_seed=args.seed)
    coll = MetricCollection([partial(ClassificationScore, **knobs)], original_samples=dm.X_train, original_labels=dm.y_train,
                            holdout_samples=dm.X_test, holdout_labels=dm.y_test)
    X, y = fresh.X_train, fresh.y_train.numpy()
    rng = np.random.default_rng(args.seed)
    zero = X[fresh.y_train == 0]
    stand_ins = {"right labels": (X, y), "permuted labels": (X, y[rng.permutation(len(y))]),
                 "one class": (zero[rng.integers(0, len(zero), size=len(y))], y)}
    lines = [f"# scripts/classification_demo.py: synthetic_classes (1000 x (100, 1), K=3), {args.steps} steps of 128, lr 1e-2, d_model 32; "
             "one run per row"]
    print(lines[0], flush=True)
    for name, (samples, labels) in stand_ins.items():
        res = coll(samples, other_labels=labels)
        lines.append(json.dumps(dict({"generator": name}, **{k: round(v, 4) for k, v in res.items()})))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
