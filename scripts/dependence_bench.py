#!/usr/bin/env python3
"""fd_series_dependence (csrc/fd_dependence.hip) at the two dataset sizes that bracket its work, against a torch restatement on the
same device and against a plain device-to-device copy of x (the read floor: the kernel reads x once; the copy reads and writes it).

  ecg     87 554 x 187 x 1, default lags (46, no ccf): per-series moments and acf and the set means
  mimic   17 000 x 24 x 40, lags 6, cross lags 8: per-series moments and acf, the set means of all 14 800 features (the
          (n, 9, 40, 40) ccf array is never written)

The torch restatement is what one writes without the kernel: centre, `torch.fft.rfft` of the series zero-padded to 2 T, |X|^2 for
the acf and conj(X_c) X_d for the ccf, `irfft`, divide by the deviations, mean over the series; the ccf product is done on chunks of
2048 series (the chunk's (2048, T + 1, 40, 40) complex array is 0.5 GB).  Timed is the whole Python call with device events, after
a warm-up, the three variants alternating, five runs each; best and spread are reported.  Raw lines go to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CASES = {"ecg": (87554, 187, 1, None, None), "mimic": (17000, 24, 40, 6, 8)}
CHUNK = 2048


def torch_dependence(x, L, Lx):
    """(moments (n, C, 4), acf (n, L, C), mean acf (L, C), mean ccf (Lx + 1, C, C) or None) in float32 torch on x's device."""
    n, T, C = x.shape
    mu = x.mean(dim=1, keepdim=True)
    e = x - mu
    m2 = (e * e).mean(dim=1)
    sd = m2.sqrt()
    moments = torch.stack([mu[:, 0], sd, (e ** 3).mean(dim=1) / (m2 * sd), (e ** 4).mean(dim=1) / (m2 * m2) - 3.0], dim=-1)
    E = torch.fft.rfft(e, n=2 * T, dim=1)
    acf = torch.fft.irfft(E.real ** 2 + E.imag ** 2, n=2 * T, dim=1)[:, 1: L + 1] / (T * m2[:, None, :])
    ccf_mean = None
    if Lx >= 0:
        total = torch.zeros((Lx + 1, C, C), dtype=torch.float32, device=x.device)
        for a in range(0, n, CHUNK):
            Ec = E[a: a + CHUNK]
            cross = torch.fft.irfft(Ec.conj()[:, :, :, None] * Ec[:, :, None, :], n=2 * T, dim=1)[:, : Lx + 1]
            s = sd[a: a + CHUNK]
            total += (cross / (T * s[:, None, :, None] * s[:, None, None, :])).sum(dim=0)
        ccf_mean = total / n
    return moments, acf, acf.mean(dim=0), ccf_mean


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
    from fourierdiffusion_amd.utils.dependence import series_dependence
    dev = torch.device("cuda", 0)
    lines = [f"# scripts/dependence_bench.py: {torch.cuda.get_device_name(0)}; ms per whole call (device events), best of {args.runs}"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, (n, T, C, lags, cross) in CASES.items():
        n = max(2, int(n * args.scale))
        x = torch.cumsum(torch.randn((n, T, C), device=dev, generator=gen), dim=1) * 0.3 + torch.randn((n, T, C), device=dev, generator=gen)
        y = torch.empty_like(x)

        def fused():
            return series_dependence(x, lags=lags, cross_lags=cross, per_series=("moments", "acf"))

        res = fused()
        L, Lx = res.lags, res.cross_lags

        def baseline():
            return torch_dependence(x, L, Lx)

        def copy():
            return y.copy_(x)

        baseline(), copy()
        torch.cuda.synchronize()
        tf, tb, tc = [], [], []
        for _ in range(args.runs):
            t, got = timed(fused)
            tf.append(t)
            t, want = timed(baseline)
            tb.append(t)
            t, _ = timed(copy)
            tc.append(t)
        gap_acf = float((got.set_mean.acf.float() - want[2]).abs().max())
        rec = {"case": name, "n": n, "T": T, "C": C, "lags": L, "cross_lags": Lx, "MB_of_x": round(x.numel() * 4 / 1e6, 1),
               "fused_ms": [round(t, 3) for t in tf], "torch_ms": [round(t, 3) for t in tb], "copy_ms": [round(t, 3) for t in tc],
               "fused_best_ms": round(min(tf), 3), "torch_best_ms": round(min(tb), 3), "copy_best_ms": round(min(tc), 3),
               "fused_spread_ms": round(max(tf) - min(tf), 3), "speedup_over_torch": round(min(tb) / min(tf), 2),
               "fused_over_copy": round(min(tf) / min(tc), 2), "max_gap_mean_acf_to_torch": gap_acf}
        if Lx >= 0:
            rec["max_gap_mean_ccf_to_torch"] = float((got.set_mean.ccf.float() - want[3]).abs().max())
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
