#!/usr/bin/env python3
"""fd_dtw_knn (csrc/fd_dtw.hip) at the reference's ECG scale against a chunked torch baseline on the same device: 10 000 random
fp32 series against 87 554, (T, C) = (187, 1), k = 5, at the default window ceil(0.1 T) = 19 and at the full window 186.

Per window: the event time of the whole call (image, kernel, merge, workspace allocation), the cell updates per second -- the cells
INSIDE the band, n m sum_i |{j : |i - j| <= w}|, what the definition needs and not what the kernel happens to touch -- and that
rate as a fraction of the derived issue bound: three VALU instructions per cell (subtract, FMA, min3) at 2 cycles per wave64
instruction on 4 SIMDs of each CU, 64 lanes / 6 cycles per SIMD at the nominal 2.4 GHz.  The bound is derived, not measured.

The baseline is what one writes without the kernel: the recurrence over anti-diagonals in torch on chunks of (queries x all
references) pairs, three (chunk, m, T + 1) float32 diagonals alive, then `topk`.  It runs on the first --baseline-queries queries
and its time is scaled by n / that; the subsample size is in the output.  On the subsample the two results are compared.
Raw lines go to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, M, T, K = 10000, 87554, 187, 5
INF = float("inf")


def band_cells(T: int, w: int) -> int:
    return sum(min(T - 1, i + w) - max(0, i - w) + 1 for i in range(T))


def torch_dtw2(q: torch.Tensor, r: torch.Tensor, w: int) -> torch.Tensor:
    """(Q, M) dtw2 of q (Q, T, C) against r (M, T, C): anti-diagonal d holds the cells (i, d - i); position p = i + 1 of a diagonal
    array, position 0 stays +inf (the absent row -1)."""
    Q, T_, _ = q.shape
    m = r.shape[0]
    prev2 = torch.full((Q, m, T_ + 1), INF, device=q.device)
    prev1 = torch.full((Q, m, T_ + 1), INF, device=q.device)
    for d in range(2 * T_ - 1):
        ilo, ihi = max(0, d - (T_ - 1), (d - w + 1) // 2), min(T_ - 1, d, (d + w) // 2)
        i = torch.arange(ilo, ihi + 1, device=q.device)
        cost = ((q[:, None, i, :] - r[None, :, d - i, :]) ** 2).sum(dim=3)                    # (Q, m, len)
        cur = torch.full((Q, m, T_ + 1), INF, device=q.device)
        if d == 0:
            cur[:, :, 1:2] = cost
        else:
            best = torch.minimum(torch.minimum(prev1[:, :, ilo + 1: ihi + 2], prev1[:, :, ilo: ihi + 1]), prev2[:, :, ilo: ihi + 1])
            cur[:, :, ilo + 1: ihi + 2] = cost + best
        prev2, prev1 = prev1, cur
    return prev1[:, :, T_]


def torch_dtw_knn(q, r, w, k, chunk):
    dist, idx = [], []
    for a in range(0, q.shape[0], chunk):
        d_, i_ = torch.topk(torch_dtw2(q[a: a + chunk], r, w), k, dim=1, largest=False)
        dist.append(d_)
        idx.append(i_)
    return torch.cat(dist).sqrt(), torch.cat(idx)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink n and m (a quick run)")
    ap.add_argument("--baseline-queries", type=int, default=16, help="queries the torch baseline runs on (its time is scaled to n); 0: no baseline (kernel ablations)")
    ap.add_argument("--baseline-chunk", type=int, default=4, help="queries per chunk of the torch baseline (three (chunk, m, T + 1) arrays)")
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    from fourierdiffusion_amd.utils.dtw import default_window, dtw_knn
    dev = torch.device("cuda", 0)
    n, m = max(K + 1, int(N * args.scale)), max(K + 2, int(M * args.scale))
    nb = min(n, max(0, args.baseline_queries))
    g = torch.Generator(device=dev).manual_seed(0)
    train = torch.randn((m, T, 1), device=dev, generator=g) * (0.6 + 0.8 * torch.rand((m, 1, 1), device=dev, generator=g))
    samples = torch.randn((n, T, 1), device=dev, generator=g) * (0.6 + 0.8 * torch.rand((n, 1, 1), device=dev, generator=g))
    props = torch.cuda.get_device_properties(0)
    clock_hz = 2.4e9                                             # the nominal peak engine clock the bound is stated at
    bound = props.multi_processor_count * 4 * 64 / 6.0 * clock_hz
    lines = [f"# scripts/dtw_bench.py: n = {n}, m = {m}, (T, C) = ({T}, 1), k = {K}; {torch.cuda.get_device_name(0)}, "
             f"{props.multi_processor_count} CUs at {clock_hz / 1e9:.2f} GHz: derived issue bound {bound:.3e} cells/s; ms per whole call, "
             f"{args.runs} runs each; " + (f"torch baseline on {nb} queries, scaled by {n / nb:.1f}" if nb else "no torch baseline")]
    print(lines[0], flush=True)
    for name, w in (("default", default_window(T)), ("full", T - 1)):
        cells = float(n) * m * band_cells(T, w)
        dtw_knn(samples[:64], train, K, window=w)                # warm-up: code objects, workspace
        if nb:
            torch_dtw_knn(samples[:1], train[:1024], w, K, 1)
        torch.cuda.synchronize()
        tf, tb = [], []
        for _ in range(args.runs):
            t, got = timed(lambda: dtw_knn(samples, train, K, window=w))
            tf.append(t)
            if nb:
                t, want = timed(lambda: torch_dtw_knn(samples[:nb], train, w, K, args.baseline_chunk))
                tb.append(t * n / nb)
        rate = cells / (min(tf) * 1e-3)
        rec = {"window": name, "w": w, "cells": cells, "fused_ms": [round(t, 2) for t in tf], "fused_best_ms": round(min(tf), 2),
               "fused_cells_per_s": float(f"{rate:.4e}"), "fraction_of_issue_bound": round(rate / bound, 4)}
        if nb:
            agree = float((got[1][:nb] == want[1]).double().mean())
            worst = float(((got[0][:nb] - want[0]).abs() / want[0]).max())
            rec.update({"torch_scaled_ms": [round(t, 1) for t in tb], "torch_best_scaled_ms": round(min(tb), 1), "torch_queries": nb,
                        "speedup_best": round(min(tb) / min(tf), 2), "index_agreement_with_torch_f32": round(agree, 6),
                        "max_rel_distance_difference": float(f"{worst:.3e}")})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
