#!/usr/bin/env python3
"""fd_softmin_pairs / fd_sinkhorn_potentials (csrc/fd_sinkhorn.hip) at the reference's ECG scale against a chunked torch baseline on
the same device: random fp32 rows, d = 187, 10 000 samples against the 87 554 training rows (8.8e8 pairs a pass; the cost matrix
would be 3.5 GB in fp32 and is rebuilt on every pass).

  pass_xy     one soft-min pass, the 10 000 rows owned and the 87 554 streamed
  pass_yx     the reverse pass of the same iteration
  divergence  a whole sinkhorn_divergence under the default schedule (24 iterations): x against y, x against x and y against y
              (7.7e9 pairs a pass), plus the pass of the marginal error

The baseline is what one writes without the kernel: `torch.cdist` squared on chunks of 2048 owned rows (the chunk's matrix is
materialised, 0.7 GB), then `torch.logsumexp` of (h - d2) / eps, potentials in float64; its iteration is the same alternating /
symmetric loop with the same schedule.  Timed is the whole Python call (workspace allocation included) with device events.  The
passes alternate the two variants, three runs each, best and spread reported; the whole divergence is run twice fused and once
in torch (after a warm-up of every shape), wall time around a synchronise.  Raw lines go to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, M, D = 10000, 87554, 187
CHUNK = 2048


def torch_softmin(x, y, h, eps):
    """out (n) float64: -eps logsumexp_j((h_j - ||x_i - y_j||^2) / eps), fp32 distances on chunks of owned rows."""
    out = []
    hf = h.float()
    for a in range(0, x.shape[0], CHUNK):
        d2 = torch.cdist(x[a: a + CHUNK], y) ** 2
        out.append(-eps * torch.logsumexp((hf[None, :] - d2) / eps, dim=1).double())
    return torch.cat(out)


def torch_potentials(x, y, sched, symmetric):
    n, m = x.shape[0], y.shape[0]
    if symmetric:
        p = torch.zeros(n, dtype=torch.float64, device=x.device)
        for eps in sched:
            p = 0.5 * (p + torch_softmin(x, x, p - eps * np.log(n), eps))
        return p, p
    f, g = None, torch.zeros(m, dtype=torch.float64, device=x.device)
    for eps in sched:
        f = torch_softmin(x, y, g - eps * np.log(m), eps)
        g = torch_softmin(y, x, f - eps * np.log(n), eps)
    return f, g


def torch_divergence(x, y, sched):
    f, g = torch_potentials(x, y, sched, False)
    px, _ = torch_potentials(x, x, sched, True)
    py, _ = torch_potentials(y, y, sched, True)
    torch_softmin(x, y, g - sched[-1] * np.log(y.shape[0]), sched[-1])          # (the pass of the marginal error)
    return float((f - px).mean() + (g - py).mean())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the row counts (a quick run)")
    ap.add_argument("--skip-torch-divergence", action="store_true", help="time the whole divergence on the fused side only")
    args = ap.parse_args()
    from fourierdiffusion_amd.utils.sinkhorn import epsilon_schedule, sinkhorn_divergence, sinkhorn_potentials, softmin_pairs
    dev = torch.device("cuda", 0)
    n, m = max(2, int(N * args.scale)), max(2, int(M * args.scale))
    lines = [f"# scripts/sinkhorn_bench.py: n = {n}, m = {m}, d = {D}, reg 0.05; {torch.cuda.get_device_name(0)}; ms per whole call"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((n, D), device=dev, generator=gen) * 1.02
    y = torch.randn((m, D), device=dev, generator=gen)
    _, _, eps = sinkhorn_potentials(x, y, schedule=[1.0, 0.05])                   # eps = 0.05 eps_base; warms the fused side up
    hx = torch.randn(n, dtype=torch.float64, device=dev, generator=gen) * eps
    hy = torch.randn(m, dtype=torch.float64, device=dev, generator=gen) * eps
    for name, (own, strm, h) in (("pass_xy", (x, y, hy)), ("pass_yx", (y, x, hx))):
        def fused():
            return softmin_pairs(own, strm, h, eps)

        def baseline():
            return torch_softmin(own, strm, h, eps)

        fused(), baseline()
        torch.cuda.synchronize()
        tf, tb = [], []
        for _ in range(3):
            t, got = timed(fused)
            tf.append(t)
            t, want = timed(baseline)
            tb.append(t)
        pairs = float(own.shape[0]) * strm.shape[0]
        rec = {"case": name, "owned": own.shape[0], "streamed": strm.shape[0], "fused_ms": [round(t, 3) for t in tf],
               "torch_ms": [round(t, 3) for t in tb], "fused_best_ms": round(min(tf), 3), "torch_best_ms": round(min(tb), 3),
               "fused_spread_ms": round(max(tf) - min(tf), 3), "torch_spread_ms": round(max(tb) - min(tb), 3),
               "speedup_best": round(min(tb) / min(tf), 3),
               "fused_TFLOPs_of_the_product": round(2.0 * pairs * D / (min(tf) * 1e-3) / 1e12, 2),
               "fused_Gpairs_per_s": round(pairs / (min(tf) * 1e-3) / 1e9, 1),
               "max_gap_to_torch_over_eps": float((got - want).abs().max() / eps)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    sched = epsilon_schedule(0.05)
    t_fused = []
    for _ in range(2):
        t, res = wall(lambda: sinkhorn_divergence(x, y))
        t_fused.append(t)
    rec = {"case": "divergence", "iterations": len(sched), "fused_wall_ms": [round(t, 1) for t in t_fused],
           "fused_best_ms": round(min(t_fused), 1), "divergence": res.divergence, "w2": res.w2, "marginal_error": res.marginal_error,
           "eps": res.eps}
    if not args.skip_torch_divergence:
        t, want = wall(lambda: torch_divergence(x, y, sched * (res.eps / sched[-1])))
        rec.update({"torch_wall_ms": round(t, 1), "speedup": round(t / min(t_fused), 3), "torch_divergence": want,
                    "gap_to_torch": abs(want - res.divergence)})
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
