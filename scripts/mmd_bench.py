#!/usr/bin/env python3
"""fd_kernel_quadforms (csrc/fd_mmd.hip) at the reference's ECG scale against a chunked torch baseline on the same device: random
fp32 rows, d = 187, 200 permutations (201 membership columns), the default five kernel scales.

  fold   10 000 samples against 10 000 real rows
  full   10 000 samples against the 87 554 training rows (9.5e9 pairs; the kernel matrix would be 38 GB)

The baseline is what one writes without the kernel: `torch.cdist` squared on chunks of 2048 rows (the chunk's matrix is
materialised, 0.8 GB at the full size), `exp` per scale, the diagonal zeroed, then `matmul` with the fp32 membership matrix and the
same float64 sums.  Both get the pooled rows and the memberships on the device and the same bandwidth; timed is the whole Python
call `kernel_quadforms` (workspace allocation included) against the baseline function.  The two variants alternate, three runs
each, event time; the best of three and the spread are reported, and the wall time of one whole `mmd_permutation_test` (host
permutations, transfers and float64 arithmetic included).  Raw lines go to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, D, PERMS = 10000, 187, 200
CASES = (("fold", 10000), ("full", 87554))
CHUNK = 2048


def torch_quadforms(z, member_f32, scales, base2):
    """(quad, rowsum, col0) float64 as fd_kernel_quadforms defines them; member_f32 (N, P + 1) with a last column of ones."""
    P = member_f32.shape[1] - 1
    quad = torch.zeros(P, dtype=torch.float64, device=z.device)
    rows = []
    for a in range(0, z.shape[0], CHUNK):
        d2 = torch.cdist(z[a: a + CHUNK], z) ** 2
        k = torch.zeros_like(d2)
        for c in scales:
            k += torch.exp(d2 * (-1.0 / (c * base2)))
        own = torch.arange(d2.shape[0], device=z.device)
        k[own, own + a] = 0.0
        t = (k @ member_f32).double() / len(scales)
        quad += (member_f32[a: a + CHUNK, :P].double() * t[:, :P]).sum(dim=0)
        rows.append(t[:, [P, 0]])
    rows = torch.cat(rows)
    return quad, rows[:, 0].contiguous(), rows[:, 1].contiguous()


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
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the row counts (a quick run)")
    args = ap.parse_args()
    from fourierdiffusion_amd.utils.two_sample import DEFAULT_SCALES, kernel_quadforms, mmd_permutation_test, permutation_members
    dev = torch.device("cuda", 0)
    lines = [f"# scripts/mmd_bench.py: d = {D}, {PERMS} permutations, scales {DEFAULT_SCALES}; {torch.cuda.get_device_name(0)}; ms per "
             "whole call, variants alternated, three runs each"]
    print(lines[0], flush=True)
    for name, rows in CASES:
        n, m = max(2, int(N * args.scale)), max(2, int(rows * args.scale))
        g = torch.Generator(device=dev).manual_seed(0)
        z = torch.cat([torch.randn((n, D), device=dev, generator=g) * 1.02, torch.randn((m, D), device=dev, generator=g)])
        member = torch.from_numpy(permutation_members(n, m, PERMS, 0)).to(dev)
        member_f32 = torch.cat([member.float(), torch.ones((n + m, 1), device=dev)], dim=1)
        base2 = float(kernel_quadforms(z, member)[3].item())           # (warm-up of the fused side)

        def fused():
            return kernel_quadforms(z, member, bandwidth2=base2)

        def baseline():
            return torch_quadforms(z, member_f32, DEFAULT_SCALES, base2)

        baseline()
        torch.cuda.synchronize()
        tf, tb = [], []
        for _ in range(3):
            t, got = timed(fused)
            tf.append(t)
            t, want = timed(baseline)
            tb.append(t)
        gap = float(((got[0] - want[0]).abs() / want[0].abs()).max())
        t0 = time.perf_counter()
        res = mmd_permutation_test(z[:n], z[n:], n_permutations=PERMS, seed=0)
        wall = (time.perf_counter() - t0) * 1e3
        pairs = float(n + m) ** 2
        rec = {"case": name, "n": n, "m": m, "fused_ms": [round(t, 3) for t in tf], "torch_ms": [round(t, 3) for t in tb],
               "fused_best_ms": round(min(tf), 3), "torch_best_ms": round(min(tb), 3),
               "fused_spread_ms": round(max(tf) - min(tf), 3), "torch_spread_ms": round(max(tb) - min(tb), 3),
               "speedup_best": round(min(tb) / min(tf), 3),
               "fused_TFLOPs_both_products": round(2.0 * pairs * (D + PERMS + 1) / (min(tf) * 1e-3) / 1e12, 2),
               "quad_max_relative_gap_to_torch_f32": gap, "whole_test_wall_ms": round(wall, 1), "mmd2": res.mmd2,
               "p_value": res.p_value}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del z, member, member_f32, got, want
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
