#!/usr/bin/env python3
"""fd_knn_rows / fd_ball_counts (csrc/fd_neighbours.hip) at the reference's ECG scale against a chunked torch baseline on the same
device: random fp32 rows, d = 187, k = 5.

  knn     10 000 samples against the 87 554 training rows
  self    the training set's own k-NN radii: 87 554 x 87 554, exclude_self (2.9 TFLOP of distances; the matrix would be 30 GB)
  counts  10 000 samples in the 87 554 balls of those radii

The baseline is what one writes without the kernel: `torch.cdist` on chunks of query rows (the chunk's distance matrix is
materialised, 2048 rows = 0.7 GB) followed by `topk` (or a compare and a row sum).  The two variants alternate, three runs each,
event time per whole call (workspace allocation included on both sides); the best of three and the spread are reported.  Raw lines
go to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, M, D, K = 10000, 87554, 187, 5
CHUNK = 2048


def torch_knn(q, r, k, exclude_self):
    dist, idx = [], []
    for a in range(0, q.shape[0], CHUNK):
        block = torch.cdist(q[a: a + CHUNK], r)
        if exclude_self:
            rows = torch.arange(block.shape[0], device=q.device)
            block[rows, rows + a] = float("inf")
        d_, i_ = torch.topk(block, k, dim=1, largest=False)
        dist.append(d_)
        idx.append(i_)
    return torch.cat(dist), torch.cat(idx)


def torch_counts(q, r, radii):
    return torch.cat([(torch.cdist(q[a: a + CHUNK], r) <= radii[None, :]).sum(dim=1) for a in range(0, q.shape[0], CHUNK)])


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
    args = ap.parse_args()
    from fourierdiffusion_amd.utils.neighbours import ball_counts, knn
    dev = torch.device("cuda", 0)
    n, m = max(K + 1, int(N * args.scale)), max(K + 2, int(M * args.scale))
    g = torch.Generator(device=dev).manual_seed(0)
    train = torch.randn((m, D), device=dev, generator=g)
    samples = torch.randn((n, D), device=dev, generator=g) * 1.02
    lines = [f"# scripts/knn_bench.py: n = {n}, m = {m}, d = {D}, k = {K}; {torch.cuda.get_device_name(0)}; ms per whole call, "
             "variants alternated, three runs each"]
    print(lines[0], flush=True)
    radii = knn(train, train, K, exclude_self=True)[0][:, K - 1].contiguous()
    cases = [
        ("knn", n, lambda: knn(samples, train, K), lambda: torch_knn(samples, train, K, False)),
        ("self", m, lambda: knn(train, train, K, exclude_self=True), lambda: torch_knn(train, train, K, True)),
        ("counts", n, lambda: ball_counts(samples, train, radii), lambda: torch_counts(samples, train, radii)),
    ]
    for name, rows, fused, baseline in cases:
        fused(), baseline()                                      # warm-up: workspace, library handles
        torch.cuda.synchronize()
        tf, tb = [], []
        for _ in range(3):
            t, got = timed(fused)
            tf.append(t)
            t, want = timed(baseline)
            tb.append(t)
        if name == "counts":
            agree = float((got == want).double().mean())
        else:
            agree = float((got[1] == want[1]).double().mean())
        flop = 2.0 * rows * m * D
        rec = {"case": name, "rows": rows, "fused_ms": [round(t, 3) for t in tf], "torch_ms": [round(t, 3) for t in tb],
               "fused_best_ms": round(min(tf), 3), "torch_best_ms": round(min(tb), 3),
               "fused_spread_ms": round(max(tf) - min(tf), 3), "torch_spread_ms": round(max(tb) - min(tb), 3),
               "speedup_best": round(min(tb) / min(tf), 3), "fused_distance_TFLOPs": round(flop / (min(tf) * 1e-3) / 1e12, 2),
               "agreement_with_torch_f32": round(agree, 6)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
