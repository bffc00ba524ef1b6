#!/usr/bin/env python3
"""fd_series_signature (csrc/fd_signature.hip) at the two dataset sizes that bracket its work, against a torch restatement on the same
device and against a plain device-to-device copy of x (the read floor: the kernel reads x once; the copy reads and writes it).

  ecg     87 554 x 187 x 1, depth 4, time channel: D = 30, two series per wave
  mimic   17 000 x 24 x 40, depth 2, time channel: D = 1722, one series per workgroup

Both return the per-series feature rows, the squared norms and the expected signature.  The torch restatement is what one writes
without the kernel: float64 tensors batched over the series, one Python step per segment, each level updated by the same Horner form.
Timed is the whole Python call with device events, after a warm-up, the three variants alternating, five runs each; best and spread
are reported.  Raw lines go to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CASES = {"ecg": (87554, 187, 1, 4), "mimic": (17000, 24, 40, 2)}


def torch_signature(x, depth):
    """(sig (n, D) float32, sqnorm (n,), mean (D,)) in float64 torch on x's device, time channel appended."""
    n, T, C = x.shape
    p = x.double()
    inc = p[:, 1:] - p[:, :-1]
    S = T - 1
    inc = torch.cat([inc, torch.full((n, S, 1), 1.0 / S, dtype=torch.float64, device=x.device)], dim=2)
    d = C + 1
    state = [torch.zeros((n, d ** k), dtype=torch.float64, device=x.device) for k in range(1, depth + 1)]
    for s in range(S):
        dl = inc[:, s, :]
        new = []
        for k in range(1, depth + 1):
            acc = dl / k
            for j in range(1, k):
                acc = ((acc + state[j - 1])[:, :, None] * dl[:, None, :] / (k - j)).reshape(n, -1)
            new.append(state[k - 1] + acc)
        state = new
    full = torch.cat(state, dim=1)
    return full.float(), (full * full).sum(dim=1), full.mean(dim=0)


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
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the series counts (a quick run)")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    from fourierdiffusion_amd.utils.signature import series_signature
    dev = torch.device("cuda", 0)
    lines = [f"# scripts/signature_bench.py: {torch.cuda.get_device_name(0)}; ms per whole call (device events), best of {args.runs}"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, (n, T, C, depth) in CASES.items():
        n = max(2, int(n * args.scale))
        x = torch.cumsum(torch.randn((n, T, C), device=dev, generator=gen), dim=1) * 0.1
        y = torch.empty_like(x)

        def fused():
            return series_signature(x, depth, per_series=("sig", "sqnorm"))

        def baseline():
            return torch_signature(x, depth)

        def copy():
            return y.copy_(x)

        fused(), baseline(), copy()
        torch.cuda.synchronize()
        tf, tb, tc = [], [], []
        for _ in range(args.runs):
            t, got = timed(fused)
            tf.append(t)
            t, want = timed(baseline)
            tb.append(t)
            t, _ = timed(copy)
            tc.append(t)
        rec = {"case": name, "n": n, "T": T, "C": C, "depth": depth, "D": int(got.mean.shape[0]), "MB_of_x": round(x.numel() * 4 / 1e6, 1),
               "fused_ms": [round(t, 3) for t in tf], "torch_ms": [round(t, 3) for t in tb], "copy_ms": [round(t, 3) for t in tc],
               "fused_best_ms": round(min(tf), 3), "torch_best_ms": round(min(tb), 3), "copy_best_ms": round(min(tc), 3),
               "fused_spread_ms": round(max(tf) - min(tf), 3), "speedup_over_torch": round(min(tb) / min(tf), 2),
               "fused_over_copy": round(min(tf) / min(tc), 2),
               "max_rel_gap_mean_to_torch": float(((got.mean - want[2]).abs() / want[2].abs().clamp_min(1e-300)).max()),
               "max_gap_sig_to_torch": float((got.sig - want[0]).abs().max())}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del x, y, got, want
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
