#!/usr/bin/env python3
"""fd_multivariate_ranks (csrc/fd_mvrank.hip) at the shape of DESIGN 3.36: (n, K, T, C) = (1000, 100, 100, 12), a forecast mask
hiding the last 24 steps (288 hidden entries of 1200), random fp32 samples.  Per pre-rank: the event time per call (median of
`--reps`, and the minimum), the workspace, and the work the call does, counted from the shape.  One line per measurement; `--out`
also writes them to a file.  No threshold is asserted anywhere."""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--C", type=int, default=12)
    ap.add_argument("--horizon", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fourierdiffusion_amd import _C
    from fourierdiffusion_amd.sampling.forecast import PRERANKS
    n, K, T, C = args.n, args.K, args.T, args.C
    dev = torch.device("cuda", 0)
    h, L = _C.ctx(dev), _C.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((n, K, T, C), device=dev, generator=g)
    y = torch.randn((n, T, C), device=dev, generator=g)
    m8 = torch.ones((T, C), dtype=torch.uint8, device=dev)
    m8[T - args.horizon:] = 0
    m, d = K + 1, args.horizon * C
    pre = torch.empty((n, m), dtype=torch.float64, device=dev)
    below, equal, hid = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    work = {
        "average": f"{n * m * m * d:.3e} compares",
        "band_depth": f"{2 * n * m * m * d:.3e} compares",
        "dominance": f"{n * m * m * d:.3e} compares",
        "mst": f"{n * m * m * d:.3e} fp64 fused multiply-adds, then {n * m} Prim runs of {m - 2} steps",
    }
    lines = []
    tag = f"(n, K, T, C) = ({n}, {K}, {T}, {C}), last {args.horizon} steps hidden ({d} of {T * C} entries)"
    for code, kind in enumerate(PRERANKS):
        need = ctypes.c_size_t(0)
        _C.check(L.fd_multivariate_ranks_workspace_bytes(h, code, n, K, T, C, ctypes.byref(need)), h)
        ws = torch.empty(max(1, need.value), dtype=torch.uint8, device=dev)
        st = _C.stream_of(x)
        med, lo = event_time(lambda: _C.check(L.fd_multivariate_ranks(h, code, x.data_ptr(), y.data_ptr(), m8.data_ptr(), 0, n, K, T,
                                                                      C, pre.data_ptr(), below.data_ptr(), equal.data_ptr(),
                                                                      hid.data_ptr(), ws.data_ptr(), ws.numel(), st), h), args.reps)
        line = (f"{tag}: fd_multivariate_ranks {kind} {med:.3f} ms per call (median of {args.reps}, min {lo:.3f}); workspace "
                f"{need.value / 2 ** 20:.1f} MiB; {work[kind]}")
        print(line, flush=True)
        lines.append(line)
        del ws
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
