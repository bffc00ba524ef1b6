"""GPU: banded dynamic time warping (fd_dtw_pairs, fd_dtw_knn, fd_dtw_ball_counts: csrc/fd_dtw.hip), its Python surface
(utils/dtw.py) and the metrics built on it (DTWPrecisionRecall, DTWMemorisation) against the float64 recurrence of tests/dtw_ref.py.

The band.  eps = dtw_bound(T, C) = 1.01 (C + 2) (2 T - 1) 2^-24 bounds the relative error of a computed dtw2 (dtw_ref.dtw_bound:
derived, not tuned).  Selection may exchange two references whose float64 dtw2 differ by less than 2 eps D, and a pair within
eps D of its radius may be counted or not; everything outside those bands must be exact, a returned distance is within eps of the
float64 value of the returned index, and at most 1 % of the pairs of a case may fall inside a band (with Gaussian inputs the
reference puts essentially none there).

The kernel keeps a block of 8 query rows in registers and hands one row to the next block through the LDS; there is no second
column form and so no capacity boundary at 64 / 256: the cases `band64` / `band65` (band columns of 64 and 65 entries) stay at those
sizes, and what they cross here is the block structure (T = 64 a whole number of blocks, T = 70 not; w = 63 every column masked somewhere, w = 32 not)."""
import ctypes as C
import functools
import os
import subprocess
import sys
from functools import partial
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import dtw_ref as R
from tests import knn_ref as K

from .gpu_util import dev

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# (n, m, T, C, w, k, self)
CASES = {
    "degenerate": (1, 1, 1, 1, 0, 1, False),
    "full_ragged_lanes": (3, 70, 5, 1, 4, 1, False),
    "ragged_both_3ch": (70, 129, 24, 3, 2, 5, False),
    "k16": (9, 200, 48, 1, 5, 16, False),
    "odd_full_5ch": (5, 64, 37, 5, 36, 1, False),
    "band64": (4, 65, 64, 1, 63, 1, False),
    "band65": (4, 65, 70, 1, 32, 1, False),
    "ecg_default": (4, 65, 187, 1, 19, 3, False),
    "ecg_full": (4, 65, 187, 1, 186, 1, False),
    "droughts": (3, 66, 365, 13, 37, 1, False),
    "mimic_40ch": (2, 64, 24, 40, 3, 1, False),
    "self_exclude": (130, 130, 24, 2, 3, 5, True),
    "self_k_is_m-1": (17, 17, 5, 2, 1, 16, True),
}


class forced_splits:
    def __init__(self, splits):
        self.splits = splits

    def __enter__(self):
        self.old = os.environ.get("FDIFF_DTW_SPLITS")
        if self.splits is not None:
            os.environ["FDIFF_DTW_SPLITS"] = str(self.splits)
        else:
            os.environ.pop("FDIFF_DTW_SPLITS", None)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("FDIFF_DTW_SPLITS", None)
        else:
            os.environ["FDIFF_DTW_SPLITS"] = self.old


def knn_raw(q, r, w, k, exclude_self=False, splits=None):
    """fd_dtw_knn through the C ABI on (n, T, C) device tensors: (dist2 (n, k) float32, idx (n, k) int32) as numpy."""
    from fourierdiffusion_amd import _C
    n, T, Cn = q.shape
    m = r.shape[0]
    h, L = _C.ctx(q.device), _C.lib()
    with forced_splits(splits):
        need = C.c_size_t(0)
        _C.check(L.fd_dtw_knn_workspace_bytes(h, n, m, T, Cn, w, k, C.byref(need)), h)
        work = torch.empty((need.value,), dtype=torch.uint8, device=q.device)
        dist2 = torch.full((n, k), -1.0, dtype=torch.float32, device=q.device)
        idx = torch.full((n, k), -1, dtype=torch.int32, device=q.device)
        _C.check(L.fd_dtw_knn(h, q.data_ptr(), n, r.data_ptr(), m, T, Cn, w, k, int(exclude_self), dist2.data_ptr(), idx.data_ptr(),
                              work.data_ptr(), need.value, _C.stream_of(q)), h)
    return dist2.cpu().numpy(), idx.cpu().numpy()


def counts_raw(q, r, w, radius2, splits=None):
    from fourierdiffusion_amd import _C
    n, T, Cn = q.shape
    m = r.shape[0]
    h, L = _C.ctx(q.device), _C.lib()
    rad = torch.from_numpy(np.ascontiguousarray(radius2, dtype=np.float32)).to(q.device)
    counts = torch.full((n,), -1, dtype=torch.int32, device=q.device)
    with forced_splits(splits):
        need = C.c_size_t(0)
        _C.check(L.fd_dtw_ball_counts_workspace_bytes(h, n, m, T, Cn, w, C.byref(need)), h)
        work = torch.empty((need.value,), dtype=torch.uint8, device=q.device)
        _C.check(L.fd_dtw_ball_counts(h, q.data_ptr(), n, r.data_ptr(), m, T, Cn, w, rad.data_ptr(), counts.data_ptr(),
                                      work.data_ptr(), need.value, _C.stream_of(q)), h)
    return counts.cpu().numpy()


def pairs_raw(a, b, w):
    from fourierdiffusion_amd import _C
    n, T, Cn = a.shape
    h = _C.ctx(a.device)
    dist2 = torch.full((n,), -1.0, dtype=torch.float32, device=a.device)
    _C.check(_C.lib().fd_dtw_pairs(h, a.data_ptr(), b.data_ptr(), n, T, Cn, w, dist2.data_ptr(), _C.stream_of(a)), h)
    return dist2.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and the float64 reference of one case, computed once and shared (nothing below writes to them).  q2: queries that are
    not the references, for the counts and the pairs of the self cases (in a set against itself every reference has a query
    exactly ON its radius)."""
    n, m, T, Cn, w, k, self_ = CASES[name]
    rs = np.random.RandomState(len(name) * 1000 + n + m + T)
    # Gaussian series of a random scale each: equal scales make the distances of long series concentrate, and the float64 reference
    # alone then puts ranks inside the exchange band
    r = (rs.randn(m, T, Cn) * rs.uniform(0.6, 1.4, size=(m, 1, 1))).astype(np.float32)
    q2 = (rs.randn(n, T, Cn) * rs.uniform(0.6, 1.4, size=(n, 1, 1)) + 0.05).astype(np.float32)
    q = r if self_ else q2
    D = R.dtw2_matrix(q, r, w)
    D2 = D if not self_ else R.dtw2_matrix(q2, r, w)
    kk = min(k + 1, m - (1 if self_ else 0))                    # one rank more than asked: the gap behind the last rank
    ref_d, ref_i = R.knn(D, kk, exclude_self=self_)
    if m > 1:
        Drr = D if self_ else R.dtw2_self_matrix(r, w)
        radius2 = (R.nnd(Drr, min(k, m - 1)) ** 2).astype(np.float32)          # the references' NND_k, as the kernel receives it
    else:
        radius2 = (2.0 * D2.max(axis=0)).astype(np.float32)     # (no other reference: a radius the one query is well inside)
    return dict(q=q, r=r, q2=q2, w=w, k=k, self_=self_, D=D, D2=D2, eps=R.dtw_bound(T, Cn), ref_d=ref_d, ref_i=ref_i, radius2=radius2)


def check_knn(got_d, got_i, k, ref_d, ref_i, pair_d2, eps, self_, m):
    """The assertions of one k-NN result: got_* (n, k) from the engine; ref_* (n, k or k + 1) the float64 ranks; pair_d2 (n, k) the
    float64 dtw2 of every RETURNED pair; m references."""
    n = got_d.shape[0]
    got_d = got_d.astype(np.float64)
    # the returned distance is the distance of the returned index
    worst = np.abs(got_d - pair_d2) / np.maximum(pair_d2, 1e-300)
    print(f"[dtw knn] returned distance error / bound: max {worst.max() / eps:.3e}")
    assert (np.abs(got_d - pair_d2) <= eps * pair_d2).all()
    # ascending in (distance, index), no repeats, no self
    if k > 1:
        a, b = got_d[:, :-1], got_d[:, 1:]
        assert ((a < b) | ((a == b) & (got_i[:, :-1] < got_i[:, 1:]))).all()
    assert all(len(set(row.tolist())) == k for row in got_i)
    assert (got_i >= 0).all()
    if self_:
        assert (got_i != np.arange(n)[:, None]).all()
    # a rank separated from both neighbours by more than 2 eps D is decided
    behind = ref_d[:, k:k + 1] if ref_d.shape[1] > k else np.full((n, 1), np.inf)       # (no further row: nothing to swap with)
    padded = np.concatenate([np.full((n, 1), -np.inf), ref_d[:, :k], behind], axis=1)
    gap_before, gap_after = padded[:, 1:k + 1] - padded[:, 0:k], padded[:, 2:k + 2] - padded[:, 1:k + 1]
    band_before = 2 * eps * padded[:, 1:k + 1]
    band_after = 2 * eps * np.where(np.isfinite(padded[:, 2:k + 2]), padded[:, 2:k + 2], 0.0)
    decided = (gap_before > band_before) & (gap_after > band_after)
    inside = float((~decided).sum()) / (n * (m - (1 if self_ else 0)))
    print(f"[dtw knn] pairs inside the exchange band: {int((~decided).sum())} ranks, {inside:.4f} of the case's pairs")
    assert inside <= 0.01
    assert (got_i[decided] == ref_i[:, :k][decided]).all()


def check_counts(got, D, radius2, eps):
    """counts within [#{D (1 + eps) <= rad2}, #{D (1 - eps) <= rad2}]; at most 1 % of the pairs between the two."""
    sure = D * (1.0 + eps) <= radius2[None, :]
    maybe = D * (1.0 - eps) <= radius2[None, :]
    inside = float((maybe & ~sure).mean())
    print(f"[dtw counts] pairs inside the band: {inside:.4f}; counts {got.min()}..{got.max()}")
    assert inside <= 0.01
    assert ((got >= sure.sum(axis=1)) & (got <= maybe.sum(axis=1))).all()


@pytest.mark.parametrize("name", list(CASES))
def test_knn_against_float64(name):
    c = case(name)
    q = dev(c["q"])
    r = q if c["self_"] else dev(c["r"])
    got_d, got_i = knn_raw(q, r, c["w"], c["k"], c["self_"])                       # (outputs pre-filled with -1)
    pair = np.take_along_axis(c["D"], got_i.astype(np.int64), axis=1)
    check_knn(got_d, got_i, c["k"], c["ref_d"], c["ref_i"], pair, c["eps"], c["self_"], c["r"].shape[0])
    # two runs are bit-identical
    again_d, again_i = knn_raw(q, r, c["w"], c["k"], c["self_"])
    assert np.array_equal(bits(got_d), bits(again_d)) and np.array_equal(got_i, again_i)
    # and the returned distances are fd_dtw_pairs of the returned pairs, bit for bit
    rows = np.repeat(np.arange(got_i.shape[0]), c["k"])
    a, b = dev(c["q"][rows]), dev(c["r"][got_i.reshape(-1)])
    assert np.array_equal(bits(pairs_raw(a, b, c["w"])), bits(got_d.reshape(-1)))


@pytest.mark.parametrize("name", list(CASES))
def test_ball_counts_against_float64(name):
    c = case(name)
    q, r = dev(c["q2"]), dev(c["r"])
    got = counts_raw(q, r, c["w"], c["radius2"])
    assert (got >= 0).all()                                      # (the output was pre-filled with -1)
    check_counts(got, c["D2"], c["radius2"].astype(np.float64), c["eps"])
    assert np.array_equal(got, counts_raw(q, r, c["w"], c["radius2"]))              # two runs
    for splits in (1, 2, 3):
        assert np.array_equal(got, counts_raw(q, r, c["w"], c["radius2"], splits=splits)), splits


@pytest.mark.parametrize("name", list(CASES))
def test_pairs_against_float64_and_symmetric(name):
    c = case(name)
    p = min(c["q2"].shape[0], c["r"].shape[0])
    a, b = dev(c["q2"][:p]), dev(c["r"][:p])
    got = pairs_raw(a, b, c["w"])
    want = np.diagonal(c["D2"])[:p]
    err = np.abs(got.astype(np.float64) - want) / want
    print(f"[dtw pairs] error / bound: max {err.max() / c['eps']:.3e}")
    assert (got >= 0).all() and (err <= c["eps"]).all()
    assert np.array_equal(bits(got), bits(pairs_raw(b, a, c["w"])))                 # dtw2(a, b) == dtw2(b, a) bit for bit
    assert np.array_equal(bits(got), bits(pairs_raw(a, b, c["w"])))                 # two runs
    assert (pairs_raw(a, a, c["w"]) == 0.0).all()


def test_bit_copies_come_back_at_distance_zero_lower_index_first():
    c = case("ragged_both_3ch")
    q, r, w = c["q"].copy(), c["r"].copy(), c["w"]
    r[100] = r[31]                                               # one reference series twice
    q[0], q[40], q[69] = r[31], r[5], r[128]                     # three queries that are bit-copies of reference series
    got_d, got_i = knn_raw(dev(q), dev(r), w, 5)
    assert got_d[0, 0] == 0.0 and got_d[0, 1] == 0.0 and got_i[0, 0] == 31 and got_i[0, 1] == 100 and got_d[0, 2] > 0.0
    assert got_d[40, 0] == 0.0 and got_i[40, 0] == 5 and got_d[40, 1] > 0.0
    assert got_d[69, 0] == 0.0 and got_i[69, 0] == 128 and got_d[69, 1] > 0.0
    # and in a set against itself the duplicate is the nearest neighbour of its twin, not the series itself
    rr = dev(r)
    self_d, self_i = knn_raw(rr, rr, w, 5, exclude_self=True)
    assert self_i[31, 0] == 100 and self_i[100, 0] == 31 and self_d[31, 0] == 0.0 and self_d[100, 0] == 0.0
    assert (self_i != np.arange(129)[:, None]).all()


@pytest.mark.parametrize("name", ["k16", "ragged_both_3ch", "self_exclude"])
def test_knn_does_not_depend_on_the_split(name):
    c = case(name)
    q = dev(c["q"])
    r = q if c["self_"] else dev(c["r"])
    base_d, base_i = knn_raw(q, r, c["w"], c["k"], c["self_"], splits=1)
    for splits in (2, 3):
        d, i = knn_raw(q, r, c["w"], c["k"], c["self_"], splits=splits)
        assert np.array_equal(bits(base_d), bits(d)) and np.array_equal(base_i, i), splits
    d, i = knn_raw(q, r, c["w"], c["k"], c["self_"])             # and the split the engine picks by itself
    assert np.array_equal(bits(base_d), bits(d)) and np.array_equal(base_i, i)


def test_window_zero_agrees_with_the_euclidean_kernel():
    from tests.test_gpu_knn import knn_raw as euclid_raw
    n, m, T, Cn, k = 33, 70, 16, 2, 4
    rs = np.random.RandomState(16)
    q, r = (rs.randn(n, T, Cn) * 1.1).astype(np.float32), rs.randn(m, T, Cn).astype(np.float32)
    D = K.dist2(q, r)
    np.testing.assert_allclose(R.dtw2_matrix(q, r, 0), D, rtol=1e-13)
    got_d, got_i = knn_raw(dev(q), dev(r), 0, k)
    euc_d, euc_i = euclid_raw(dev(q).reshape(n, T * Cn), dev(r).reshape(m, T * Cn), k)
    eps = R.dtw_bound(T, Cn)
    pair = np.take_along_axis(D, got_i.astype(np.int64), axis=1)
    # each kernel's returned distance is within its own bound of the float64 distance of ITS index (1e-6: test_gpu_knn.py)
    assert (np.abs(got_d - pair) <= eps * pair).all()
    assert (np.abs(euc_d - np.take_along_axis(D, euc_i.astype(np.int64), axis=1)) <= 1e-6 * np.take_along_axis(D, euc_i.astype(np.int64), axis=1)).all()
    # the indices agree wherever a rank is outside both exchange bands (the Euclidean one: the centred expansion's error)
    ref_d, ref_i = R.knn(D, k + 1)
    delta = 2 * (K.expansion_bound(q, r).max(axis=1)[:, None] + eps * ref_d[:, 1:k + 1])
    padded = np.concatenate([np.full((n, 1), -np.inf), ref_d], axis=1)
    decided = (padded[:, 1:k + 1] - padded[:, 0:k] > delta) & (padded[:, 2:k + 2] - padded[:, 1:k + 1] > delta)
    assert decided.mean() >= 0.99
    assert (got_i[decided] == euc_i[decided]).all() and (got_i[decided] == ref_i[:, :k][decided]).all()
    assert (np.abs(got_d - euc_d)[decided] <= (eps + 1e-6) * ref_d[:, :k][decided]).all()


def test_python_surface():
    from fourierdiffusion_amd.utils.dtw import dtw_ball_counts, dtw_knn, dtw_pairs
    c = case("ragged_both_3ch")
    dist, idx = dtw_knn(c["q"], torch.from_numpy(c["r"]), 5, window=c["w"])
    assert dist.device.type == "cuda" and dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.shape == idx.shape == (70, 5)
    raw_d, raw_i = knn_raw(dev(c["q"]), dev(c["r"]), c["w"], 5)
    assert np.array_equal(idx.cpu().numpy(), raw_i)
    np.testing.assert_allclose(dist.cpu().numpy(), np.sqrt(raw_d), rtol=2.0 ** -22, atol=0)      # (the device's f32 square root)
    radii = np.sqrt(c["radius2"]) * 1.3
    counts = dtw_ball_counts(c["q"], c["r"], radii, window=c["w"])
    assert counts.dtype == torch.int64 and counts.shape == (70,)
    assert np.array_equal(counts.cpu().numpy(), counts_raw(dev(c["q"]), dev(c["r"]), c["w"], radii.astype(np.float32) ** 2))
    pd = dtw_pairs(c["q"][:60], c["r"][:60], window=c["w"])
    assert pd.shape == (60,) and pd.dtype == torch.float32 and pd.device.type == "cuda"
    np.testing.assert_allclose(pd.cpu().numpy(), np.sqrt(pairs_raw(dev(c["q"][:60]), dev(c["r"][:60]), c["w"])), rtol=2.0 ** -22)
    # window=None is ceil(0.1 T) = 3, "full" is T - 1; (n, T) is C = 1
    X = dev(c["r"])
    own_d, own_i = dtw_knn(X, X, 2, exclude_self=True)
    assert (own_i.cpu().numpy() != np.arange(129)[:, None]).all()
    assert np.array_equal(own_i.cpu().numpy(), knn_raw(X, X, 3, 2, True)[1])
    flat = c["r"][:, :, 0]
    full = dtw_pairs(flat[:64], flat[64:128], window="full")
    assert np.array_equal(bits(full.cpu().numpy()), bits(np.sqrt(pairs_raw(dev(flat[:64, :, None]), dev(flat[64:128, :, None]), 23))))


@pytest.mark.parametrize("T,Cn", [(24, 40), (134, 5), (187, 1), (251, 4), (252, 5), (365, 13)])
def test_every_dataset_shape_runs_at_the_default_window(T, Cn):
    from fourierdiffusion_amd.utils.dtw import default_window, dtw_knn
    rs = np.random.RandomState(T)
    q, r = rs.randn(2, T, Cn).astype(np.float32), rs.randn(5, T, Cn).astype(np.float32)
    dist, idx = dtw_knn(q, r, 1)
    D = R.dtw2_matrix(q, r, default_window(T))
    assert np.array_equal(idx.cpu().numpy()[:, 0], D.argmin(axis=1))
    np.testing.assert_allclose(dist.cpu().numpy()[:, 0] ** 2, D.min(axis=1), rtol=R.dtw_bound(T, Cn) + 2.0 ** -22)
    if (T, Cn) == (187, 1):
        dist, idx = dtw_knn(q, r, 1, window="full")
        D = R.dtw2_matrix(q, r, T - 1)
        assert np.array_equal(idx.cpu().numpy()[:, 0], D.argmin(axis=1))
        np.testing.assert_allclose(dist.cpu().numpy()[:, 0] ** 2, D.min(axis=1), rtol=R.dtw_bound(T, Cn) + 2.0 ** -22)


def test_widest_band_of_a_long_series():
    """T = 600, w = 127: a band column of 255 and the largest LDS ring the kernel asks for (262 rows, above 64 KiB)."""
    rs = np.random.RandomState(600)
    q, r = rs.randn(1, 600, 1).astype(np.float32), (rs.randn(3, 600, 1) * rs.uniform(0.6, 1.4, size=(3, 1, 1))).astype(np.float32)
    D = R.dtw2_matrix(q, r, 127)
    got_d, got_i = knn_raw(dev(q), dev(r), 127, 3)
    pair = np.take_along_axis(D, got_i.astype(np.int64), axis=1)
    assert (np.abs(got_d - pair) <= R.dtw_bound(600, 1) * pair).all() and np.array_equal(got_i, np.argsort(D, axis=1, kind="stable"))


# ---------------------------------------------------------------------------------------------- metrics
@functools.lru_cache(maxsize=None)
def metric_sets():
    rs = np.random.RandomState(91)
    X = rs.randn(60, 24, 2).astype(np.float32)
    Y = (rs.randn(60, 24, 2) * 1.05).astype(np.float32)
    w = 3
    return dict(X=X, Y=Y, w=w, D_yx=R.dtw2_matrix(Y, X, w), D_xx=R.dtw2_self_matrix(X, w), D_yy=R.dtw2_self_matrix(Y, w))


def _band_rows(D, radius2, eps):
    """(rows, pairs) of D within twice the band of a radius (twice: the radii themselves come from the engine)."""
    inside = np.abs(D - radius2[None, :]) <= 2 * eps * np.maximum(D, radius2[None, :])
    return int(inside.any(axis=1).sum()), int(inside.sum())


def test_dtw_precision_recall_matches_the_formulas_on_reference_distances():
    from fourierdiffusion_amd.sampling.metrics import DTWPrecisionRecall
    s = metric_sets()
    k, eps = 5, R.dtw_bound(24, 2)
    metric = DTWPrecisionRecall(original_samples=torch.from_numpy(s["X"]), k=k)          # window=None: ceil(2.4) = 3
    assert metric.window == 3 and metric.series_shape == (24, 2) and metric.name == "dtw_precision_recall"
    got, want = metric(s["Y"]), R.precision_recall(s["D_yx"], s["D_xx"], s["D_yy"], k)
    rad_x, rad_y = R.nnd(s["D_xx"], k) ** 2, R.nnd(s["D_yy"], k) ** 2
    (rows_p, pairs_p), (rows_r, _) = _band_rows(s["D_yx"], rad_x, eps), _band_rows(s["D_yx"].T, rad_y, eps)
    nearest = s["D_yx"].min(axis=0)
    rows_c = int((np.abs(nearest - rad_x) <= 2 * eps * np.maximum(nearest, rad_x)).sum())
    print(f"[dtw metrics] got {got}\n[dtw metrics] want {want}\n[dtw metrics] band rows: precision {rows_p}, recall {rows_r}, coverage {rows_c}")
    assert list(got) == ["dtw_precision", "dtw_recall", "dtw_density", "dtw_coverage"]
    assert abs(got["dtw_precision"] - want["precision"]) <= rows_p / 60 + 1e-12
    assert abs(got["dtw_density"] - want["density"]) <= pairs_p / (k * 60) + 1e-12
    assert abs(got["dtw_recall"] - want["recall"]) <= rows_r / 60 + 1e-12
    assert abs(got["dtw_coverage"] - want["coverage"]) <= rows_c / 60 + 1e-12
    assert 0.0 < want["precision"] and 0.0 < want["recall"] and 0.0 < want["coverage"] <= 1.0
    base = metric.baseline_metrics                               # the two folds of X against each other
    assert list(base) == ["dtw_precision_self", "dtw_recall_self", "dtw_density_self", "dtw_coverage_self"]
    D_gr, D_rr = s["D_xx"][30:, :30], s["D_xx"][:30, :30]
    folds = R.precision_recall(D_gr, D_rr, s["D_xx"][30:, 30:], k)
    rows_f, pairs_f = _band_rows(D_gr, R.nnd(D_rr, k) ** 2, eps)
    assert abs(base["dtw_precision_self"] - folds["precision"]) <= rows_f / 30 + 1e-12
    assert abs(base["dtw_density_self"] - folds["density"]) <= pairs_f / (k * 30) + 1e-12


def test_dtw_memorisation_matches_the_formulas_on_reference_distances():
    from fourierdiffusion_amd.sampling.metrics import DTWMemorisation
    s = metric_sets()
    eps = R.dtw_bound(24, 2)
    metric = DTWMemorisation(original_samples=s["X"], window=3)
    got, want = metric(torch.from_numpy(s["Y"])), R.memorisation(s["D_yx"], s["D_xx"])
    print(f"[dtw metrics] got {got}\n[dtw metrics] want {want}")
    assert list(got) == ["dtw_authenticity", "dtw_nn_distance_min", "dtw_nn_distance_median"] and metric.name == "dtw_memorisation"
    # band rows: a sample whose two nearest training series are within the exchange band of each other, or whose deciding comparison
    # is within the band
    two, near = R.knn(s["D_yx"], 2)
    own2 = R.nnd(s["D_xx"], 1)[near[:, 0]] ** 2
    rows_a = int(((two[:, 1] - two[:, 0] <= 2 * eps * two[:, 1]) | (np.abs(two[:, 0] - own2) <= 2 * eps * np.maximum(two[:, 0], own2))).sum())
    assert abs(got["dtw_authenticity"] - want["authenticity"]) <= rows_a / 60 + 1e-12
    assert got["dtw_nn_distance_min"] == pytest.approx(want["nn_distance_min"], rel=eps + 1e-6)
    assert got["dtw_nn_distance_median"] == pytest.approx(want["nn_distance_median"], rel=eps + 1e-6)
    # with a holdout the share appears, under its prefixed key
    H = np.random.RandomState(92).randn(60, 24, 2).astype(np.float32)
    held = DTWMemorisation(original_samples=s["X"], holdout_samples=H, window=3)(s["Y"])
    assert list(held) == ["dtw_authenticity", "dtw_nn_distance_min", "dtw_nn_distance_median", "dtw_train_closer_share"]
    to_train, to_held = s["D_yx"].min(axis=1), R.dtw2_matrix(s["Y"], H, 3).min(axis=1)
    share = float((to_train < to_held).mean() + 0.5 * (to_train == to_held).mean())
    rows_s = int((np.abs(to_train - to_held) <= 2 * eps * np.maximum(to_train, to_held)).sum())
    assert abs(held["dtw_train_closer_share"] - share) <= rows_s / 60 + 1e-12
    assert {key: held[key] for key in got} == got


def test_shifted_replays_through_the_collection_and_the_view_logic():
    """The point of the feature, through MetricCollection: replays delayed by three samples keep much of their Euclidean authenticity
    and have none under DTW; the DTW metrics exist in the time view only and leave every other key as it was."""
    from fourierdiffusion_amd.sampling.metrics import DTWMemorisation, DTWPrecisionRecall, Memorisation, MetricCollection, PrecisionRecall
    f = R.replay_fixture()
    train, replay, fresh, w = f["train"], f["replay"], f["fresh"], f["window"]
    euclid = [partial(PrecisionRecall, k=5), partial(Memorisation, random_seed=0)]
    dtw = [partial(DTWPrecisionRecall, k=5, window=w), partial(DTWMemorisation, random_seed=0, window=w)]
    both = MetricCollection(metrics=euclid + dtw, original_samples=torch.from_numpy(train))
    plain = MetricCollection(metrics=euclid, original_samples=torch.from_numpy(train))
    res, res_plain = both(torch.from_numpy(replay)), plain(torch.from_numpy(replay))
    assert list(res) == sorted(res)
    assert not any(key.startswith("freq_dtw_") for key in res) and len(both.metrics_freq) == 2 and len(both.metrics_time) == 4
    new_keys = sorted(set(res) - set(res_plain))
    assert new_keys == sorted(f"time_dtw_{key}" for key in (
        "precision", "recall", "density", "coverage", "precision_self", "recall_self", "density_self", "coverage_self",
        "authenticity", "nn_distance_min", "nn_distance_median"))
    assert {key: res[key] for key in res_plain} == res_plain     # every key of the Euclidean metrics is unchanged
    D_rt, D_tt, D_ft = R.dtw2_matrix(replay, train, w), R.dtw2_self_matrix(train, w), R.dtw2_matrix(fresh, train, w)
    want_replay, want_fresh = R.memorisation(D_rt, D_tt), R.memorisation(D_ft, D_tt)
    assert want_replay["authenticity"] == 0.0
    assert res["time_dtw_authenticity"] == want_replay["authenticity"]
    assert res["time_authenticity"] >= 0.3                       # the Euclidean metric calls many of the copies authentic
    got_fresh = both(torch.from_numpy(fresh))
    eps = R.dtw_bound(48, 1)
    two, near = R.knn(D_ft, 2)
    own2 = R.nnd(D_tt, 1)[near[:, 0]] ** 2
    rows = int(((two[:, 1] - two[:, 0] <= 2 * eps * two[:, 1]) | (np.abs(two[:, 0] - own2) <= 2 * eps * np.maximum(two[:, 0], own2))).sum())
    assert abs(got_fresh["time_dtw_authenticity"] - want_fresh["authenticity"]) <= rows / 40 + 1e-12
    assert want_fresh["authenticity"] > 0.25


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_sample_with_dtw_metrics(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=1", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=dtwrun"], tmp_path)
    _run([str(ROOT / "cmd" / "sample.py"), "model_id=dtwrun", "metrics=dtw", "num_diffusion_steps=5", "num_samples=64",
          "sampler.sample_batch_size=32"], tmp_path)
    res = yaml.safe_load(open(tmp_path / "lightning_logs" / "dtwrun" / "results.yaml"))
    for key in ("precision", "recall", "coverage", "authenticity", "train_closer_share", "precision_self", "coverage_self"):
        assert 0.0 <= res[f"time_dtw_{key}"] <= 1.0, key
        assert 0.0 <= res[f"time_{key}"] <= 1.0 and 0.0 <= res[f"freq_{key}"] <= 1.0, key
    for key in ("density", "density_self", "nn_distance_min", "nn_distance_median"):
        assert res[f"time_dtw_{key}"] >= 0.0 and np.isfinite(res[f"time_dtw_{key}"]), key
    assert not any(key.startswith("freq_dtw_") for key in res)
    # warping never lengthens a distance (to the two kernels' rounding)
    assert res["time_dtw_nn_distance_median"] <= res["time_nn_distance_median"] * (1 + R.dtw_bound(24, 4) + 1e-6)


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """Every new entry point refuses each bad argument with FD_ERR_ARG and a retrievable message."""
    from fourierdiffusion_amd import _C
    x, y = torch.zeros(8, 6, 2, device="cuda"), torch.zeros(6, 6, 2, device="cuda")
    d2, ix = torch.zeros(8, 3, device="cuda"), torch.zeros(8, 3, dtype=torch.int32, device="cuda")
    rad, cnt = torch.zeros(6, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    pd = torch.zeros(8, device="cuda")
    h, L = _C.ctx(x.device), _C.lib()
    need, need_c = C.c_size_t(0), C.c_size_t(0)
    assert L.fd_dtw_knn_workspace_bytes(h, 8, 6, 6, 2, 1, 3, C.byref(need)) == 0 and need.value > 0
    assert L.fd_dtw_ball_counts_workspace_bytes(h, 8, 6, 6, 2, 1, C.byref(need_c)) == 0 and need_c.value > 0
    work = torch.zeros(max(need.value, need_c.value), dtype=torch.uint8, device="cuda")
    p, q, dp, ip, wp, nb, nc = x.data_ptr(), y.data_ptr(), d2.data_ptr(), ix.data_ptr(), work.data_ptr(), need.value, need_c.value
    rp, cp, pp = rad.data_ptr(), cnt.data_ptr(), pd.data_ptr()
    big = 1 << 30
    cases = [
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 6, 2, 1, 3, None), b"null"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 0, 6, 6, 2, 1, 3, C.byref(need)), b"bad shape"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 0, 2, 0, 3, C.byref(need)), b"bad shape"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 6, 0, 1, 3, C.byref(need)), b"bad shape"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 1025, 1, 1, 3, C.byref(need)), b"bad shape"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 6, 2, -1, 3, C.byref(need)), b"window=-1"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 6, 2, 6, 3, C.byref(need)), b"window=6"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 600, 1, 128, 3, C.byref(need)), b"window=128"),       # band column 257
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 257, 1, 256, 3, C.byref(need)), b"window=256"),       # band column 257 = T
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 6, 2, 1, 0, C.byref(need)), b"k=0"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 6, 2, 1, 7, C.byref(need)), b"k=7"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 40, 6, 2, 1, 17, C.byref(need)), b"k=17"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, big, 6, 6, 2, 1, 3, C.byref(need)), b"too large"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, big, 6, 2, 1, 3, C.byref(need)), b"too large"),
        (lambda: L.fd_dtw_knn_workspace_bytes(h, 8, 6, 1024, big, 1, 3, C.byref(need)), b"too large"),
        (lambda: L.fd_dtw_knn(h, None, 8, q, 6, 6, 2, 1, 3, 0, dp, ip, wp, nb, None), b"null"),
        (lambda: L.fd_dtw_knn(h, p, 8, None, 6, 6, 2, 1, 3, 0, dp, ip, wp, nb, None), b"null"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 3, 0, None, ip, wp, nb, None), b"null"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 3, 0, dp, None, wp, nb, None), b"null"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 3, 0, dp, ip, None, nb, None), b"null"),
        (lambda: L.fd_dtw_knn(h, p, 0, q, 6, 6, 2, 1, 3, 0, dp, ip, wp, nb, None), b"bad shape"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 0, 6, 2, 1, 3, 0, dp, ip, wp, nb, None), b"bad shape"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, -1, 2, 0, 3, 0, dp, ip, wp, nb, None), b"bad shape"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 0, 1, 3, 0, dp, ip, wp, nb, None), b"bad shape"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, -1, 3, 0, dp, ip, wp, nb, None), b"window=-1"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 6, 3, 0, dp, ip, wp, nb, None), b"window=6"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 600, 1, 128, 3, 0, dp, ip, wp, nb, None), b"window=128"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 0, 0, dp, ip, wp, nb, None), b"k=0"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 7, 0, dp, ip, wp, nb, None), b"k=7"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 40, 6, 2, 1, 17, 0, dp, ip, wp, nb, None), b"k=17"),
        (lambda: L.fd_dtw_knn(h, p, 8, p, 8, 6, 2, 1, 8, 1, dp, ip, wp, nb, None), b"k=8"),          # only 7 other series
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 3, 1, dp, ip, wp, nb, None), b"exclude_self"),   # q != r
        (lambda: L.fd_dtw_knn(h, p, 8, p, 6, 6, 2, 1, 3, 1, dp, ip, wp, nb, None), b"exclude_self"),   # n != m
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 3, 0, dp, ip, wp, nb - 1, None), b"workspace"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 3, 0, dp, ip, wp, 0, None), b"workspace"),
        (lambda: L.fd_dtw_knn(h, p, big, q, 6, 6, 2, 1, 3, 0, dp, ip, wp, nb, None), b"too large"),
        (lambda: L.fd_dtw_knn(h, p, 8, q, big, 6, 2, 1, 3, 0, dp, ip, wp, nb, None), b"too large"),
        (lambda: L.fd_dtw_ball_counts_workspace_bytes(h, 8, 6, 6, 2, 1, None), b"null"),
        (lambda: L.fd_dtw_ball_counts_workspace_bytes(h, 8, 0, 6, 2, 1, C.byref(need_c)), b"bad shape"),
        (lambda: L.fd_dtw_ball_counts_workspace_bytes(h, 8, 6, 6, 2, 7, C.byref(need_c)), b"window=7"),
        (lambda: L.fd_dtw_ball_counts_workspace_bytes(h, 8, big, 6, 2, 1, C.byref(need_c)), b"too large"),
        (lambda: L.fd_dtw_ball_counts(h, None, 8, q, 6, 6, 2, 1, rp, cp, wp, nc, None), b"null"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, None, 6, 6, 2, 1, rp, cp, wp, nc, None), b"null"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, q, 6, 6, 2, 1, None, cp, wp, nc, None), b"null"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, q, 6, 6, 2, 1, rp, None, wp, nc, None), b"null"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, q, 6, 6, 2, 1, rp, cp, None, nc, None), b"null"),
        (lambda: L.fd_dtw_ball_counts(h, p, 0, q, 6, 6, 2, 1, rp, cp, wp, nc, None), b"bad shape"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, q, 6, 6, 0, 1, rp, cp, wp, nc, None), b"bad shape"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, q, 6, 6, 2, 6, rp, cp, wp, nc, None), b"window=6"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, q, 6, 600, 1, 128, rp, cp, wp, nc, None), b"window=128"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, q, 6, 6, 2, 1, rp, cp, wp, nc - 1, None), b"workspace"),
        (lambda: L.fd_dtw_ball_counts(h, p, 8, q, big, 6, 2, 1, rp, cp, wp, nc, None), b"too large"),
        (lambda: L.fd_dtw_pairs(h, None, p, 8, 6, 2, 1, pp, None), b"null"),
        (lambda: L.fd_dtw_pairs(h, p, None, 8, 6, 2, 1, pp, None), b"null"),
        (lambda: L.fd_dtw_pairs(h, p, p, 8, 6, 2, 1, None, None), b"null"),
        (lambda: L.fd_dtw_pairs(h, p, p, 0, 6, 2, 1, pp, None), b"bad shape"),
        (lambda: L.fd_dtw_pairs(h, p, p, 8, 0, 2, 0, pp, None), b"bad shape"),
        (lambda: L.fd_dtw_pairs(h, p, p, 8, 6, -2, 1, pp, None), b"bad shape"),
        (lambda: L.fd_dtw_pairs(h, p, p, 8, 6, 2, -1, pp, None), b"window=-1"),
        (lambda: L.fd_dtw_pairs(h, p, p, 8, 6, 2, 6, pp, None), b"window=6"),
        (lambda: L.fd_dtw_pairs(h, p, p, 8, 600, 1, 128, pp, None), b"window=128"),
        (lambda: L.fd_dtw_pairs(h, p, p, big, 6, 2, 1, pp, None), b"too large"),
    ]
    for i, (call, needle) in enumerate(cases):
        assert call() == -1, i
        assert needle in L.fd_last_error(h), (i, L.fd_last_error(h))
    assert L.fd_dtw_knn(None, p, 8, q, 6, 6, 2, 1, 3, 0, dp, ip, wp, nb, None) == -1          # no context: error code only
    assert L.fd_dtw_ball_counts(None, p, 8, q, 6, 6, 2, 1, rp, cp, wp, nc, None) == -1
    assert L.fd_dtw_pairs(None, p, p, 8, 6, 2, 1, pp, None) == -1
    # and the arguments they were derived from are accepted
    assert L.fd_dtw_knn(h, p, 8, q, 6, 6, 2, 1, 3, 0, dp, ip, wp, nb, None) == 0
    assert L.fd_dtw_ball_counts(h, p, 8, q, 6, 6, 2, 1, rp, cp, wp, nc, None) == 0
    assert L.fd_dtw_pairs(h, p, p, 8, 6, 2, 1, pp, None) == 0
    torch.cuda.synchronize()
    assert (ix.cpu().numpy() == np.array([0, 1, 2])[None]).all() and (cnt.cpu().numpy() == 6).all() and (pd.cpu().numpy() == 0).all()
