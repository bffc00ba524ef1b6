#!/usr/bin/env python3
"""fd_energy_score, fd_variogram_score and fd_ensemble_ranks (csrc/fd_multivariate.hip) at the shapes of DESIGN 3.23:
(n, K, T, C) = (512, 100, 100, 12) with every pair and (64, 100, 1024, 16) with max_lag = 8, every entry hidden, p = 0.5,
inverse-lag weights, random fp32 samples.  Per shape and kernel: the event time per call (median of `--reps`), and the same score
as a chunked torch expression on the same device (torch.cdist for the energy score, a broadcast expression for the variogram
score; `--base-series` series at a time, timed on that many series and scaled to n).  One line per measurement; `--out` also
writes them to a file.  No ratio is asserted anywhere."""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(512, 100, 100, 12, None), (64, 100, 1024, 16, 8)]


def event_time(call, reps, warmup=2):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def torch_energy(x, y):
    """x (b, K, D), y (b, D), every entry hidden: (b,) float64."""
    K = x.shape[1]
    rows = torch.cat([x, y[:, None]], 1)
    d = torch.cdist(rows, rows, compute_mode="donot_use_mm_for_euclid_dist").double()
    return d[:, :K, K].sum(1) / K - d[:, :K, :K].sum((1, 2)) / (2.0 * K * K)


def torch_variogram(x, y, T, C, max_lag, block=64):
    """x (b, K, T C), y (b, T C), every entry hidden, p = 0.5, inverse-lag weights: num / den (b,) float64."""
    b, K, D = x.shape
    t = torch.arange(D, device=x.device) // C
    num = torch.zeros(b, dtype=torch.float64, device=x.device)
    den = torch.zeros((), dtype=torch.float64, device=x.device)
    for a0 in range(0, D, block):
        a1 = min(D, a0 + block)
        hi = D if max_lag is None else min(D, ((a1 - 1) // C + max_lag + 1) * C)      # the columns the band can reach
        lag = (t[None, a0:hi] - t[a0:a1, None])
        keep = (torch.arange(a0, hi, device=x.device)[None] > torch.arange(a0, a1, device=x.device)[:, None])
        if max_lag is not None:
            keep &= lag <= max_lag
        w = torch.where(keep, 1.0 / (1.0 + lag.double()), torch.zeros((), dtype=torch.float64, device=x.device))
        vx = (x[:, :, a0:a1, None] - x[:, :, None, a0:hi]).abs().sqrt().mean(1)
        vy = (y[:, a0:a1, None] - y[:, None, a0:hi]).abs().sqrt()
        num += (w * (vy - vx).double() ** 2).sum((1, 2))
        den += w.sum()
    return num / den


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--base-series", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd import _C
    dev = torch.device("cuda", 0)
    h, L = _C.ctx(dev), _C.lib()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for n, K, T, C, max_lag in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((n, K, T, C), device=dev, generator=g)
        y = torch.randn((n, T, C), device=dev, generator=g)
        m8 = torch.zeros((T, C), dtype=torch.uint8, device=dev)
        lag = -1 if max_lag is None else max_lag
        need = ctypes.c_size_t(0)
        _C.check(L.fd_energy_score_workspace_bytes(h, n, K, T, C, ctypes.byref(need)), h)
        work_e = torch.empty(max(1, need.value), dtype=torch.uint8, device=dev)
        _C.check(L.fd_variogram_score_workspace_bytes(h, n, K, T, C, lag, ctypes.byref(need)), h)
        work_v = torch.empty(max(1, need.value), dtype=torch.uint8, device=dev)
        es, num, den = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        hid = torch.empty(n, dtype=torch.int32, device=dev)
        below, equal = (torch.empty((n, T, C), dtype=torch.int32, device=dev) for _ in range(2))
        st = _C.stream_of(x)
        calls = {
            "fd_energy_score": lambda: _C.check(L.fd_energy_score(h, x.data_ptr(), y.data_ptr(), m8.data_ptr(), 0, n, K, T, C, 0,
                                                                  es.data_ptr(), hid.data_ptr(), work_e.data_ptr(), work_e.numel(),
                                                                  st), h),
            "fd_variogram_score": lambda: _C.check(L.fd_variogram_score(h, x.data_ptr(), y.data_ptr(), m8.data_ptr(), 0, n, K, T, C,
                                                                        _C.FD_VARIOGRAM_HALF, lag, 1, num.data_ptr(), den.data_ptr(),
                                                                        None, work_v.data_ptr(), work_v.numel(), st), h),
            "fd_ensemble_ranks": lambda: _C.check(L.fd_ensemble_ranks(h, x.data_ptr(), y.data_ptr(), n, K, T, C, below.data_ptr(),
                                                                      equal.data_ptr(), st), h),
        }
        tag = f"(n, K, T, C) = ({n}, {K}, {T}, {C}), max_lag = {max_lag}"
        times = {}
        for name, call in calls.items():
            med, lo = event_time(call, args.reps)
            times[name] = med
            say(f"{tag}: {name} {med:.3f} ms per call (median of {args.reps}, min {lo:.3f})")
        nb = min(args.base_series, n)
        xb, yb = x[:nb].reshape(nb, K, T * C), y[:nb].reshape(nb, T * C)
        base = {
            "fd_energy_score": lambda: torch_energy(xb, yb),
            "fd_variogram_score": lambda: torch_variogram(xb, yb, T, C, max_lag),
        }
        for name, call in base.items():
            med, _ = event_time(call, args.base_reps, warmup=1)
            scaled = med * n / nb
            say(f"{tag}: torch baseline of {name} {med:.3f} ms for {nb} series = {scaled:.1f} ms for {n} "
                f"(median of {args.base_reps}); kernel / baseline = {times[name] / scaled:.4f}")
        # the two agree (a sanity line, not a test: tests/test_gpu_multivariate.py compares against float64)
        e_err = float(((es[:nb] - torch_energy(xb, yb)).abs() / es[:nb].abs()).max())
        v = num[:nb] / den[:nb]
        v_err = float(((v - torch_variogram(xb, yb, T, C, max_lag)).abs() / v.abs()).max())
        say(f"{tag}: kernel against the torch baseline, largest relative difference: energy {e_err:.2e}, variogram {v_err:.2e}")
        del x, y, work_e, work_v
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
