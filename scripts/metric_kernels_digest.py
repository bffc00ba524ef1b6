#!/usr/bin/env python3
"""One SHA-256 per case over the raw output bytes of the all-pairs metric entry points, for fixed seeds: knn, ball_counts
(csrc/fd_neighbours.hip), kernel_quadforms (csrc/fd_mmd.hip), dtw_pairs, dtw_knn, dtw_ball_counts (csrc/fd_dtw.hip).  The cases cover
every instantiation of k_nn, k_mmd and k_dtw and the edges of what they share (ragged query / reference tiles, a feature count that
is no multiple of 16, the self case, forced split counts).  Only public functions are called, so the same script runs on any commit
that has them: two commits compute the same thing exactly when every line is equal (profiles/metric_kernels_digest.txt)."""
from __future__ import annotations

import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def digest(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def rows(seed: int, *shape) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) + 0.5).cuda()


def knn_cases():
    from fourierdiffusion_amd.utils.neighbours import ball_counts, knn
    shapes = {"64x1000x187": (rows(1, 64, 187), rows(2, 1000, 187)), "300x257x62": (rows(3, 300, 62), rows(4, 257, 62))}
    own = rows(5, 130, 960)
    for splits in (1, 3):
        os.environ["FDIFF_KNN_SPLITS"] = str(splits)
        for k in (1, 5, 16):
            for name, (q, r) in shapes.items():
                yield f"knn {name} k={k} splits={splits}", digest(*knn(q, r, k))
            for excl in (False, True):
                yield f"knn self 130x960 k={k} exclude_self={int(excl)} splits={splits}", digest(*knn(own, own, k, exclude_self=excl))
        for name, (q, r) in shapes.items():
            radii = knn(r, r, 5, exclude_self=True)[0][:, -1] * 1.5
            yield f"ball_counts {name} splits={splits}", digest(ball_counts(q, r, radii))
    del os.environ["FDIFF_KNN_SPLITS"]


def mmd_cases():
    from fourierdiffusion_amd.utils.two_sample import kernel_quadforms
    for N in (130, 300):
        z = rows(10 + N, N, 62)
        for P in (3, 40, 100, 200, 300):
            g = torch.Generator().manual_seed(1000 * N + P)
            member = (torch.rand(N, P, generator=g) < 0.4).to(torch.uint8)
            for col_splits, scales, bw2 in itertools.product((1, 3), ((1.0,), (0.25, 0.5, 1.0, 2.0, 4.0)), (None, 90.0)):
                out = kernel_quadforms(z, member, scales=scales, bandwidth2=bw2, col_splits=col_splits)
                yield f"kernel_quadforms N={N} P={P} col_splits={col_splits} scales={len(scales)} bandwidth2={bw2}", digest(*out)


def dtw_cases():
    from fourierdiffusion_amd.utils.dtw import dtw_ball_counts, dtw_knn, dtw_pairs
    for C in (1, 3):
        q, r = rows(20 + C, 70, 48, C), rows(30 + C, 130, 48, C)
        for window in (0, 5, "full"):
            yield f"dtw_pairs C={C} window={window}", digest(dtw_pairs(q, r[:70], window=window))
            for splits in (1, 3):
                os.environ["FDIFF_DTW_SPLITS"] = str(splits)
                for k in (1, 5):
                    yield f"dtw_knn C={C} window={window} k={k} splits={splits}", digest(*dtw_knn(q, r, k, window=window))
                radii = dtw_knn(r, r, 5, window=window, exclude_self=True)[0][:, -1] * 1.5
                yield f"dtw_knn self C={C} window={window} k=5 splits={splits}", digest(*dtw_knn(r, r, 5, window=window, exclude_self=True))
                yield f"dtw_ball_counts C={C} window={window} splits={splits}", digest(dtw_ball_counts(q, r, radii, window=window))
    del os.environ["FDIFF_DTW_SPLITS"]


def main() -> None:
    assert torch.cuda.is_available(), "the digests are of GPU results"
    for cases in (knn_cases, mmd_cases, dtw_cases):
        for name, value in cases():
            print(f"{value}  {name}", flush=True)


if __name__ == "__main__":
    main()
