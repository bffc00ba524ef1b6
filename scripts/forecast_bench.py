#!/usr/bin/env python3
"""fd_ensemble_scores (csrc/fd_forecast.hip) at the shapes of DESIGN 3.13: (n, K, T, C) = (512, 100, 100, 12) and (64, 100, 1024, 16),
19 quantile levels, random fp32 samples.  Per shape: the bytes the kernel must move (samples and truth read, crps / mean / quantiles
written), the event time per call (median of `--reps`), and that time against bytes over the 8.0 TB/s HBM peak.  One JSON line per
shape.  The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
SHAPES = [(512, 100, 100, 12), (64, 100, 1024, 16)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.forecast import DEFAULT_LEVELS
    dev = torch.device("cuda", 0)
    h = _C.ctx(dev)
    lv = torch.tensor(DEFAULT_LEVELS, dtype=torch.float64, device=dev)
    L = len(DEFAULT_LEVELS)
    out = []
    for n, K, T, C in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((n, K, T, C), device=dev, generator=g)
        y = torch.randn((n, T, C), device=dev, generator=g)
        crps, mean = torch.empty((n, T, C), device=dev), torch.empty((n, T, C), device=dev)
        q = torch.empty((L, n, T, C), device=dev)
        call = lambda: _C.check(_C.lib().fd_ensemble_scores(h, x.data_ptr(), y.data_ptr(), n, K, T, C, lv.data_ptr(), L,  # noqa: E731
                                                            crps.data_ptr(), q.data_ptr(), mean.data_ptr(), _C.stream_of(x)), h)
        for _ in range(3):
            call()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        ts.sort()
        t = ts[len(ts) // 2]
        read = 4 * (n * K * T * C + n * T * C)
        written = 4 * (2 + L) * n * T * C
        rec = {"n": n, "K": K, "T": T, "C": C, "levels": L, "bytes_read": read, "bytes_written": written, "us_median": 1e6 * t,
               "us_min": 1e6 * ts[0], "read_bound_us": 1e6 * read / PEAK_BYTES_PER_S,
               "bytes_bound_us": 1e6 * (read + written) / PEAK_BYTES_PER_S}
        rec["share_of_bytes_bound"] = rec["bytes_bound_us"] / rec["us_median"]
        rec["achieved_TBps"] = (read + written) / t / 1e12
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del x, y, crps, mean, q
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
