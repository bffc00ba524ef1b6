#!/usr/bin/env python3
"""fd_series_spectra (csrc/fd_spectral.hip) at the two dataset sizes that bracket its work, against a torch restatement on the same
device and against a plain device-to-device copy of x (the read floor: the kernel reads x once; the copy reads and writes it).

  ecg     87 554 x 187 x 1, default segments (nperseg 93, noverlap 46: 3 segments): per-series psd and summaries and the set means
  mimic   17 000 x 24 x 40, default segments (nperseg 24: 1 segment): per-series psd and summaries, the set means of all 20 920
          features (the (n, 13, 780, 2) csd array is never written)

The torch restatement is what one writes without the kernel: `unfold` into segments, subtract the segment mean, multiply by the
window, `torch.fft.rfft`, `einsum` for conj(F_c) F_d summed over the segments, scale, the summaries from the psd, mean over the
series; the cross-products are done on chunks of 4096 series.  Timed is the whole Python call with device events, after a warm-up,
the variants alternating (`kernels` is the library call alone on preallocated buffers: the wrapper's allocations and its assembly of
the set mean are a dozen small launches), `--runs` runs of `--reps` = 400 back-to-back calls each (a call is about a
millisecond, so a timed window is several hundred);
best and spread per call are reported, with the DFT's floating-point operations over the best time.  Raw lines go to stdout and to
--out."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CASES = {"ecg": (87554, 187, 1), "mimic": (17000, 24, 40)}
CHUNK = 4096


def torch_spectra(x, S, noverlap):
    """(psd (n, K, C), summary (n, C, 3), mean psd (K, C), mean csd (K, C, C) complex) in float32 torch on x's device."""
    n, T, C = x.shape
    K = S // 2 + 1
    w = 0.5 - 0.5 * torch.cos(2 * math.pi * torch.arange(S, device=x.device) / S)
    seg = x.unfold(1, S, S - noverlap)                                       # (n, nseg, C, S)
    nseg = seg.shape[1]
    F = torch.fft.rfft((seg - seg.mean(dim=-1, keepdim=True)) * w, dim=-1)   # (n, nseg, C, K)
    scale = torch.full((K,), 2.0, device=x.device)
    scale[0] = 1.0
    if S % 2 == 0:
        scale[-1] = 1.0
    scale = scale / (nseg * (w * w).sum())
    psd = ((F.real ** 2 + F.imag ** 2).sum(dim=1) * scale).transpose(1, 2)   # (n, K, C)
    total = torch.zeros((K, C, C), dtype=torch.complex64, device=x.device)
    if C > 1:
        for a in range(0, n, CHUNK):
            Fc = F[a: a + CHUNK]
            total += torch.einsum("ngck,ngdk->kcd", Fc.conj(), Fc)
        total = total * scale[:, None, None] / n
    tail = psd[:, 1:]
    tot = tail.sum(dim=1)
    f = torch.arange(1, K, device=x.device) / S
    p = tail / tot[:, None, :]
    summary = torch.stack([psd.sum(dim=1), (f[None, :, None] * tail).sum(dim=1) / tot,
                           -(p * torch.log(p.clamp_min(1e-30))).sum(dim=1) / math.log(max(K - 1, 2))], dim=-1)
    return psd, summary, psd.mean(dim=0), total


def raw_call(x, S, noverlap):
    """fd_series_spectra alone on preallocated outputs and workspace (psd, summary and the set mean): the three kernels without the
    wrapper's allocations and the assembly of the set mean."""
    import ctypes

    from fourierdiffusion_amd import _C
    n, T, C = x.shape
    K, NP = S // 2 + 1, C * (C - 1) // 2
    h, lib = _C.ctx(x.device), _C.lib()
    psd = torch.empty((n, K, C), dtype=torch.float32, device=x.device)
    summary = torch.empty((n, C, 3), dtype=torch.float32, device=x.device)
    mean = torch.empty((K * C + 2 * K * NP + 3 * C,), dtype=torch.float64, device=x.device)
    need = ctypes.c_size_t(0)
    _C.check(lib.fd_series_spectra_workspace_bytes(h, n, T, C, S, noverlap, ctypes.byref(need)), h)
    work = torch.empty((need.value,), dtype=torch.uint8, device=x.device)
    stream = _C.stream_of(x)

    def run():
        _C.check(lib.fd_series_spectra(h, x.data_ptr(), n, T, C, S, noverlap, 1, 1, psd.data_ptr(), None, summary.data_ptr(),
                                       mean.data_ptr(), work.data_ptr(), need.value, stream), h)
        return mean
    return run


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the series counts (a quick run)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=400, help="back-to-back calls per timed window (a window of several hundred ms)")
    args = ap.parse_args()
    from fourierdiffusion_amd.utils.spectral import series_spectra
    dev = torch.device("cuda", 0)
    lines = [f"# scripts/spectral_dependence_bench.py: {torch.cuda.get_device_name(0)}; ms per whole call (device events over {args.reps} calls), "
             f"best of {args.runs}"]
    print(lines[0], flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, (n, T, C) in CASES.items():
        n = max(2, int(n * args.scale))
        x = torch.cumsum(torch.randn((n, T, C), device=dev, generator=gen), dim=1) * 0.3 + torch.randn((n, T, C), device=dev, generator=gen)
        y = torch.empty_like(x)

        def fused():
            return series_spectra(x, per_series=("psd", "summary"))

        res = fused()
        S, ov, nseg = res.nperseg, res.noverlap, res.n_segments

        raw = raw_call(x, S, ov)

        def baseline():
            return torch_spectra(x, S, ov)

        def copy():
            return y.copy_(x)

        baseline(), copy(), raw()
        torch.cuda.synchronize()
        tf, tb, tc, tk = [], [], [], []
        for _ in range(args.runs):
            t, got = timed(fused, args.reps)
            tf.append(t)
            t, want = timed(baseline, args.reps)
            tb.append(t)
            t, _ = timed(copy, args.reps)
            tc.append(t)
            t, _ = timed(raw, args.reps)
            tk.append(t)
        K = S // 2 + 1
        useful = 2.0 * n * nseg * C * S * 2 * K                              # the DFT as a dense product, useful columns only
        padded = 2.0 * n * (-(-S // 16) * 16) * (-(-2 * K // 16) * 16) * (-(-nseg * C // 16) * 16)
        scale_psd = float(want[2].abs().max())
        rec = {"case": name, "n": n, "T": T, "C": C, "nperseg": S, "noverlap": ov, "segments": nseg, "MB_of_x": round(x.numel() * 4 / 1e6, 1),
               "fused_ms": [round(t, 4) for t in tf], "torch_ms": [round(t, 4) for t in tb], "copy_ms": [round(t, 4) for t in tc],
               "kernels_ms": [round(t, 4) for t in tk], "kernels_best_ms": round(min(tk), 4), "kernels_over_copy": round(min(tk) / min(tc), 2),
               "fused_best_ms": round(min(tf), 4), "torch_best_ms": round(min(tb), 4), "copy_best_ms": round(min(tc), 4),
               "fused_spread_ms": round(max(tf) - min(tf), 4), "speedup_over_torch": round(min(tb) / min(tf), 2),
               "fused_over_copy": round(min(tf) / min(tc), 2), "dft_useful_gflop": round(useful / 1e9, 2),
               "dft_issued_gflop": round(padded / 1e9, 2), "useful_tflops_at_kernels_best": round(useful / (min(tk) * 1e-3) / 1e12, 2),
               "issued_tflops_at_kernels_best": round(padded / (min(tk) * 1e-3) / 1e12, 2),
               "max_rel_gap_mean_psd_to_torch": float((got.set_mean.psd.float() - want[2]).abs().max()) / scale_psd}
        if C > 1:
            rec["max_rel_gap_mean_csd_to_torch"] = float((got.set_mean.csd - want[3].to(torch.complex128)).abs().max()) / scale_psd
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
