#!/usr/bin/env python3
"""The experiment behind the multivariate rank histograms on the device: n series of a common level plus noise, K
members and the truth from one law (calibrated by construction), against the same ensemble with its members permuted
independently at every entry.  The per-entry rank histogram of sampling/forecast.py is the same for both; the histograms of
multivariate_rank_histogram are not.  Prints the reliability index of every histogram for both sets, one line per histogram;
`--out` also writes the lines to a file.  Nothing is asserted."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--K", type=int, default=19)
    ap.add_argument("--T", type=int, default=12)
    ap.add_argument("--C", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd.sampling import forecast as F
    from tests.mvrank_ref import coherent_and_shuffled
    truth, x, shuffled = (torch.from_numpy(v) for v in coherent_and_shuffled(args.n, args.K, args.T, args.C, args.seed))
    mask = torch.zeros((args.T, args.C), dtype=torch.bool)
    lines = [f"(n, K, T, C) = ({args.n}, {args.K}, {args.T}, {args.C}), every entry hidden, seed {args.seed}; reliability index "
             "sum_b |f_b - 1 / (K + 1)| of each rank histogram", f"{'histogram':<14}{'coherent':>10}{'shuffled':>10}"]
    rows = {}
    for name, v in (("coherent", x), ("shuffled", shuffled)):
        below, equal = F.rank_counts(v, truth)
        rows.setdefault("per-entry", {})[name] = F.reliability_index(F.rank_histogram(below, equal, mask, args.K))
        for kind, r in F.multivariate_rank_histogram(v, truth, mask, F.PRERANKS).items():
            rows.setdefault(kind, {})[name] = r["reliability_index"]
    for kind, r in rows.items():
        lines.append(f"{kind:<14}{r['coherent']:>10.3f}{r['shuffled']:>10.3f}")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
