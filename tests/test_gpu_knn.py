"""GPU: the nearest-neighbour primitives (fd_knn_rows, fd_ball_counts: csrc/fd_neighbours.hip) and the metrics built on them
(PrecisionRecall, Memorisation) against the float64 brute force of tests/knn_ref.py.

The band.  With u = 2^-24 and mu the reference mean, delta_ij = 2 (d + 3) u (||q_i - mu||^2 + ||r_j - mu||^2) is the worst-case
error of the centred f32 expansion the selection and the counts run on (knn_ref.expansion_bound: derived, not tuned).  Selection may
therefore exchange two rows whose float64 distances differ by less than 2 delta, and a pair within delta of its radius may be
counted or not; everything outside the band must be exact, and a returned distance is always the direct-form distance of the
returned index to f32 rounding (rtol 1e-6: one f32 rounding of each difference, 2 u relative on each square, and one of the sum)."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import knn_ref as R

from .gpu_util import dev

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# (n, m, d, k, exclude_self, shift)
SHAPES = {
    "300x257x62": (300, 257, 62, 5, False, 0.0),
    "64x1000x187": (64, 1000, 187, 3, False, 0.0),
    "1x64x9": (1, 64, 9, 1, False, 0.0),
    "200x333x24": (200, 333, 24, 4, False, 0.0),
    "self130x960": (130, 130, 960, 5, True, 0.0),
    "300x257x62+3": (300, 257, 62, 5, False, 3.0),
    "40x17x5_k_is_m": (40, 17, 5, 16, False, 0.0),               # k = m - 1 and k = m
    "self17x5_k_is_m-1": (17, 17, 5, 16, True, 0.0),
}
NON_SELF = [name for name, s in SHAPES.items() if not s[4]]


class forced_splits:
    def __init__(self, splits):
        self.splits = splits

    def __enter__(self):
        self.old = os.environ.get("FDIFF_KNN_SPLITS")
        if self.splits is not None:
            os.environ["FDIFF_KNN_SPLITS"] = str(self.splits)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("FDIFF_KNN_SPLITS", None)
        else:
            os.environ["FDIFF_KNN_SPLITS"] = self.old


def knn_raw(q, r, k, exclude_self=False, splits=None):
    """fd_knn_rows through the C ABI on device tensors: (dist2 (n, k) float32, idx (n, k) int32) as numpy, squared distances."""
    from fourierdiffusion_amd import _C
    n, d = q.shape
    m = r.shape[0]
    h, L = _C.ctx(q.device), _C.lib()
    with forced_splits(splits):
        need = C.c_size_t(0)
        _C.check(L.fd_knn_rows_workspace_bytes(h, n, m, d, k, C.byref(need)), h)
        work = torch.empty((need.value,), dtype=torch.uint8, device=q.device)
        dist2 = torch.full((n, k), -1.0, dtype=torch.float32, device=q.device)
        idx = torch.full((n, k), -1, dtype=torch.int32, device=q.device)
        _C.check(L.fd_knn_rows(h, q.data_ptr(), n, r.data_ptr(), m, d, k, int(exclude_self), dist2.data_ptr(), idx.data_ptr(),
                               work.data_ptr(), need.value, _C.stream_of(q)), h)
    return dist2.cpu().numpy(), idx.cpu().numpy()


def counts_raw(q, r, radius2, splits=None):
    from fourierdiffusion_amd import _C
    h = _C.ctx(q.device)
    rad = torch.from_numpy(np.ascontiguousarray(radius2, dtype=np.float32)).to(q.device)
    counts = torch.full((q.shape[0],), -1, dtype=torch.int32, device=q.device)
    with forced_splits(splits):
        _C.check(_C.lib().fd_ball_counts(h, q.data_ptr(), q.shape[0], r.data_ptr(), r.shape[0], q.shape[1], rad.data_ptr(),
                                         counts.data_ptr(), _C.stream_of(q)), h)
    return counts.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and the float64 reference of one shape, computed once and shared (nothing below writes to them)."""
    n, m, d, k, self_, shift = SHAPES[name]
    rs = np.random.RandomState(len(name) * 1000 + n + m + d)
    r = (rs.randn(m, d) + shift).astype(np.float32)
    q = r if self_ else (rs.randn(n, d) * 1.1 + 0.05 + shift).astype(np.float32)
    D = R.dist2(q, r)
    kk = min(k + 1, m - (1 if self_ else 0))                    # one rank more than asked: the gap behind the last rank
    ref_d, ref_i = R.knn(q, r, kk, exclude_self=self_, D=D)
    return dict(q=q, r=r, k=k, self_=self_, D=D, delta=R.expansion_bound(q, r), ref_d=ref_d, ref_i=ref_i)


def check_knn(got_d, got_i, k, ref_d, ref_i, pair_d2, delta_row, self_):
    """The assertions of one k-NN result: got_* (n, k) from the engine; ref_* (n, k or k + 1) the float64 ranks; pair_d2 (n, k) the
    float64 direct distance of every RETURNED pair; delta_row (n) = max_j delta_ij."""
    n = got_d.shape[0]
    got_d = got_d.astype(np.float64)
    # the returned distance is the distance of the returned index
    assert (np.abs(got_d - pair_d2) <= 1e-6 * pair_d2).all(), np.abs(got_d - pair_d2).max()
    # rank by rank within the band of the float64 rank
    worst = np.abs(got_d - ref_d[:, :k]) / delta_row[:, None]
    print(f"[knn] rank distance error / band: max {worst.max():.3e}")
    assert (worst <= 1.0).all()
    # ascending in (distance, index), no repeats, no self
    if k > 1:
        a, b = got_d[:, :-1], got_d[:, 1:]
        assert ((a < b) | ((a == b) & (got_i[:, :-1] < got_i[:, 1:]))).all()
    assert all(len(set(row.tolist())) == k for row in got_i)
    assert (got_i >= 0).all()
    if self_:
        assert (got_i != np.arange(n)[:, None]).all()
    # a rank separated from both neighbours by more than twice the band is decided
    behind = ref_d[:, k:k + 1] if ref_d.shape[1] > k else np.full((n, 1), np.inf)       # (no further row: nothing to swap with)
    padded = np.concatenate([np.full((n, 1), -np.inf), ref_d[:, :k], behind], axis=1)
    gap_before, gap_after = padded[:, 1:k + 1] - padded[:, 0:k], padded[:, 2:k + 2] - padded[:, 1:k + 1]
    decided = (gap_before > 2 * delta_row[:, None]) & (gap_after > 2 * delta_row[:, None])
    print(f"[knn] decided ranks: {decided.mean():.4f}")
    assert decided.mean() >= 0.9                                 # (generic data: or the index check below checks nothing)
    assert (got_i[decided] == ref_i[:, :k][decided]).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_knn_rows_against_float64(name):
    c = case(name)
    q = dev(c["q"])
    r = q if c["self_"] else dev(c["r"])
    got_d, got_i = knn_raw(q, r, c["k"], c["self_"])
    pair = np.take_along_axis(c["D"], got_i.astype(np.int64), axis=1)
    check_knn(got_d, got_i, c["k"], c["ref_d"], c["ref_i"], pair, c["delta"].max(axis=1), c["self_"])
    # two runs are bit-identical
    again_d, again_i = knn_raw(q, r, c["k"], c["self_"])
    assert np.array_equal(got_d.view(np.uint32), again_d.view(np.uint32)) and np.array_equal(got_i, again_i)


def test_knn_rows_k_equal_to_m_returns_every_row():
    c = case("40x17x5_k_is_m")
    q, r = dev(c["q"]), dev(c["r"])
    got_d, got_i = knn_raw(q, r, 16)
    assert all(len(set(row.tolist())) == 16 and row.max() <= 16 for row in got_i)
    r16 = r[:16].contiguous()                                    # k = m
    got_d, got_i = knn_raw(q, r16, 16)
    assert (np.sort(got_i, axis=1) == np.arange(16)[None]).all() and (np.diff(got_d, axis=1) >= 0).all()


def test_knn_rows_exact_duplicates_come_back_at_distance_zero_lower_index_first():
    c = case("300x257x62")
    q, r = c["q"].copy(), c["r"].copy()
    r[200] = r[31]                                               # one reference row twice
    q[0], q[150], q[299] = r[31], r[5], r[256]                   # three queries that are bit-copies of reference rows
    got_d, got_i = knn_raw(dev(q), dev(r), 5)
    assert got_d[0, 0] == 0.0 and got_d[0, 1] == 0.0 and got_i[0, 0] == 31 and got_i[0, 1] == 200 and got_d[0, 2] > 0.0
    assert got_d[150, 0] == 0.0 and got_i[150, 0] == 5 and got_d[150, 1] > 0.0
    assert got_d[299, 0] == 0.0 and got_i[299, 0] == 256 and got_d[299, 1] > 0.0
    # and in a set against itself the duplicate is the nearest neighbour of its twin, not the row itself
    rr = dev(r)
    self_d, self_i = knn_raw(rr, rr, 5, exclude_self=True)
    assert self_i[31, 0] == 200 and self_i[200, 0] == 31 and self_d[31, 0] == 0.0 and self_d[200, 0] == 0.0
    assert (self_i != np.arange(257)[:, None]).all()
    D = R.dist2(q, r)
    ref_d, ref_i = R.knn(q, r, 6, D=D)
    check_knn(got_d, got_i, 5, ref_d, ref_i, np.take_along_axis(D, got_i.astype(np.int64), axis=1),
              R.expansion_bound(q, r).max(axis=1), False)


@pytest.mark.parametrize("name", ["64x1000x187", "300x257x62", "self130x960"])
def test_knn_rows_does_not_depend_on_the_split(name):
    c = case(name)
    q = dev(c["q"])
    r = q if c["self_"] else dev(c["r"])
    base_d, base_i = knn_raw(q, r, c["k"], c["self_"], splits=1)
    for splits in (2, 7):
        d, i = knn_raw(q, r, c["k"], c["self_"], splits=splits)
        assert np.array_equal(base_d.view(np.uint32), d.view(np.uint32)) and np.array_equal(base_i, i), splits
    d, i = knn_raw(q, r, c["k"], c["self_"])                     # and the split the engine picks by itself
    assert np.array_equal(base_d.view(np.uint32), d.view(np.uint32)) and np.array_equal(base_i, i)


def check_counts(got, D, radius2, delta):
    """counts within [#{d2 <= rad2 - delta}, #{d2 <= rad2 + delta}], and that interval is a single number for >= 95 % of rows."""
    lo = (D <= radius2[None, :] - delta).sum(axis=1)
    hi = (D <= radius2[None, :] + delta).sum(axis=1)
    open_rows = float((lo != hi).mean())
    print(f"[counts] rows with a pair inside the band: {open_rows:.4f}; counts {got.min()}..{got.max()}")
    assert open_rows <= 0.05
    assert ((got >= lo) & (got <= hi)).all()


@pytest.mark.parametrize("name", NON_SELF)
def test_ball_counts_against_float64(name):
    c = case(name)
    kr = min(c["k"], c["r"].shape[0] - 1)
    radius2 = (R.nnd(c["r"], kr) ** 2).astype(np.float32)        # the references' NND_k, as the kernel receives it
    q, r = dev(c["q"]), dev(c["r"])
    got = counts_raw(q, r, radius2)
    check_counts(got, c["D"], radius2.astype(np.float64), c["delta"])
    assert np.array_equal(got, counts_raw(q, r, radius2))        # two runs
    for splits in (1, 2, 7):
        assert np.array_equal(got, counts_raw(q, r, radius2, splits=splits)), splits


@functools.lru_cache(maxsize=None)
def mid_case():
    """n = 1000, m = 20 011, d = 187: the reference is chunked float64 torch.cdist on the device."""
    n, m, d, k = 1000, 20011, 187, 5
    g = torch.Generator().manual_seed(1234)
    r = torch.randn(m, d, generator=g).cuda()
    q = (torch.randn(n, d, generator=g) * 1.05).cuda()
    q64, r64 = q.double(), r.double()
    D = torch.cat([torch.cdist(q64[a: a + 250], r64) ** 2 for a in range(0, n, 250)])
    ref_d, ref_i = torch.sort(D, dim=1, stable=True)
    mu = r64.mean(dim=0)
    delta = 2.0 * (d + 3) * R.U * (((q64 - mu) ** 2).sum(1)[:, None] + ((r64 - mu) ** 2).sum(1)[None, :])
    nnd = torch.cat([torch.topk(torch.cdist(r64[a: a + 2048], r64), k + 1, dim=1, largest=False).values[:, k]
                     for a in range(0, m, 2048)])               # (rank 0 is the row itself)
    return dict(q=q, r=r, k=k, D=D, delta=delta, ref_d=ref_d[:, :k + 1].cpu().numpy(), ref_i=ref_i[:, :k + 1].cpu().numpy(),
                radius2=(nnd ** 2).float())


def test_mid_size_split_and_merge():
    c = mid_case()
    q, r, k = c["q"], c["r"], c["k"]
    got_d, got_i = knn_raw(q, r, k)
    gathered = r.double()[torch.from_numpy(got_i.astype(np.int64)).cuda()]                     # (n, k, d)
    pair = ((q.double()[:, None, :] - gathered) ** 2).sum(dim=2).cpu().numpy()
    check_knn(got_d, got_i, k, c["ref_d"], c["ref_i"], pair, c["delta"].max(dim=1).values.cpu().numpy(), False)
    for splits in (1, 2, 7):
        d, i = knn_raw(q, r, k, splits=splits)
        assert np.array_equal(got_d.view(np.uint32), d.view(np.uint32)) and np.array_equal(got_i, i), splits
    again_d, again_i = knn_raw(q, r, k)
    assert np.array_equal(got_d.view(np.uint32), again_d.view(np.uint32)) and np.array_equal(got_i, again_i)


def test_mid_size_ball_counts():
    c = mid_case()
    radius2 = c["radius2"]                                       # NND_5 of the references
    got = counts_raw(c["q"], c["r"], radius2.cpu().numpy())
    rad64 = radius2.double()[None, :]
    lo = (c["D"] <= rad64 - c["delta"]).sum(dim=1).cpu().numpy()
    hi = (c["D"] <= rad64 + c["delta"]).sum(dim=1).cpu().numpy()
    open_rows = float((lo != hi).mean())
    print(f"[counts] mid-size rows with a pair inside the band: {open_rows:.4f}; counts {got.min()}..{got.max()}")
    assert open_rows <= 0.05 and hi.max() > 0                    # (some query does fall into some ball)
    assert ((got >= lo) & (got <= hi)).all()
    for splits in (1, 7):
        assert np.array_equal(got, counts_raw(c["q"], c["r"], radius2.cpu().numpy(), splits=splits)), splits


def test_python_surface_returns_euclidean_distances_and_int64():
    from fourierdiffusion_amd.utils.neighbours import ball_counts, knn
    c = case("200x333x24")
    dist, idx = knn(c["q"].reshape(200, 6, 4), torch.from_numpy(c["r"]), 4)
    assert dist.device.type == "cuda" and dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.shape == idx.shape == (200, 4)
    raw_d, raw_i = knn_raw(dev(c["q"]), dev(c["r"]), 4)
    assert np.array_equal(idx.cpu().numpy(), raw_i)
    np.testing.assert_allclose(dist.cpu().numpy(), np.sqrt(raw_d), rtol=2.0 ** -22, atol=0)      # (the device's f32 square root)
    radii = R.nnd(c["r"], 4) * 1.6
    counts = ball_counts(c["q"], c["r"], radii)
    assert counts.dtype == torch.int64 and counts.shape == (200,)
    assert np.array_equal(counts.cpu().numpy(), counts_raw(dev(c["q"]), dev(c["r"]), radii.astype(np.float32) ** 2))
    X = dev(c["r"])
    own_d, own_i = knn(X, X, 2, exclude_self=True)
    assert (own_i.cpu().numpy() != np.arange(333)[:, None]).all()


# ---------------------------------------------------------------------------------------------- metrics
def _band(q, r, radius2):
    """(rows of q, pairs) within twice the expansion's band of a radius (twice: the radii themselves come from the engine)."""
    inside = np.abs(R.dist2(q, r) - radius2[None, :]) <= 2 * R.expansion_bound(q, r)
    return int(inside.any(axis=1).sum()), int(inside.sum())


def assert_precision_recall(got, want, real, generated, k):
    """Equal, but for 1 / n per row that has a pair inside the band (none on generic data)."""
    Xf, Yf = R.flat(real), R.flat(generated)
    rad_x, rad_y = R.nnd(Xf, k) ** 2, R.nnd(Yf, k) ** 2
    (rows_p, pairs_p), (rows_r, _) = _band(Yf, Xf, rad_x), _band(Xf, Yf, rad_y)
    nearest = R.dist2(Xf, Yf).min(axis=1)
    rows_c = int((np.abs(nearest - rad_x) <= 2 * R.expansion_bound(Xf, Yf).max()).sum())
    print(f"[metrics] got {got}\n[metrics] want {want}\n[metrics] band rows: precision {rows_p}, recall {rows_r}, coverage {rows_c}")
    assert list(got) == list(want) == ["precision", "recall", "density", "coverage"]
    assert abs(got["precision"] - want["precision"]) <= rows_p / Yf.shape[0] + 1e-12
    assert abs(got["density"] - want["density"]) <= pairs_p / (k * Yf.shape[0]) + 1e-12
    assert abs(got["recall"] - want["recall"]) <= rows_r / Xf.shape[0] + 1e-12
    assert abs(got["coverage"] - want["coverage"]) <= rows_c / Xf.shape[0] + 1e-12


@functools.lru_cache(maxsize=None)
def metric_sets():
    rs = np.random.RandomState(77)
    X = rs.randn(200, 31, 2).astype(np.float32)
    Y = (rs.randn(150, 31, 2) * 1.05).astype(np.float32)          # slightly too wide: all four numbers strictly inside (0, 1)
    H = rs.randn(120, 31, 2).astype(np.float32)
    return X, Y, H


def test_precision_recall_matches_the_restatement():
    from fourierdiffusion_amd.sampling.metrics import PrecisionRecall
    X, Y, _ = metric_sets()
    metric = PrecisionRecall(original_samples=torch.from_numpy(X), k=5)
    want = R.precision_recall(X, Y, k=5)
    assert_precision_recall(metric(Y), want, X, Y, 5)
    assert all(0.0 < val < 1.0 for val in want.values()) and len(set(want.values())) == 4    # (the case tells the four apart)
    assert metric.name == "precision_recall"
    # baselines: the two folds against each other
    base = metric.baseline_metrics
    assert list(base) == ["precision_self", "recall_self", "density_self", "coverage_self"]
    assert_precision_recall({key[:-5]: val for key, val in base.items()}, R.precision_recall(X[:100], X[100:], k=5), X[:100], X[100:], 5)
    # a seeded subsample of the real set
    sub = PrecisionRecall(original_samples=X, k=5, max_original=80, random_seed=3)
    keep = R.subsample_indices(200, 80, 3)
    assert np.array_equal(sub.original_samples.cpu().numpy(), R.flat(X)[keep].astype(np.float32))
    assert_precision_recall(sub(Y), R.precision_recall(X[keep], Y, k=5), X[keep], Y, 5)


def test_memorisation_matches_the_restatement():
    from fourierdiffusion_amd.sampling.metrics import Memorisation
    X, Y, H = metric_sets()
    metric = Memorisation(original_samples=X, holdout_samples=torch.from_numpy(H), random_seed=11)
    got, want = metric(Y), R.memorisation(X, Y, holdout=H, seed=11)
    print(f"[metrics] got {got}\n[metrics] want {want}")
    assert list(got) == list(want) == ["authenticity", "nn_distance_min", "nn_distance_median", "train_closer_share"]
    # band rows: a sample whose two nearest training rows are within the expansion's band of each other (another nearest row may be
    # chosen), or whose deciding comparison is a tie to f32 rounding
    Xf, Yf, Hf = R.flat(X), R.flat(Y), R.flat(H)
    keep = R.subsample_indices(200, 120, 11)
    two, near = R.knn(Yf, Xf, 2)
    own = R.nnd(Xf, 1)[near[:, 0]]
    to_sub, to_held = np.sqrt(R.knn(Yf, Xf[keep], 1)[0][:, 0]), np.sqrt(R.knn(Yf, Hf, 1)[0][:, 0])
    swap = (two[:, 1] - two[:, 0]) <= 2 * R.expansion_bound(Yf, Xf).max(axis=1)
    rows_a = int((swap | (np.abs(np.sqrt(two[:, 0]) - own) <= 1e-6 * own)).sum())
    rows_s = int((np.abs(to_sub - to_held) <= 1e-6 * to_held).sum())
    print(f"[metrics] band rows: authenticity {rows_a}, train_closer_share {rows_s}")
    assert abs(got["authenticity"] - want["authenticity"]) <= rows_a / 150 + 1e-12
    assert abs(got["train_closer_share"] - want["train_closer_share"]) <= rows_s / 150 + 1e-12
    assert got["nn_distance_min"] == pytest.approx(want["nn_distance_min"], rel=1e-5)
    assert got["nn_distance_median"] == pytest.approx(want["nn_distance_median"], rel=1e-5)
    assert np.array_equal(metric.train_subset.cpu().numpy(), Xf[keep].astype(np.float32))
    without = Memorisation(original_samples=X)(Y)
    assert list(without) == ["authenticity", "nn_distance_min", "nn_distance_median"]
    assert without == {key: got[key] for key in without} and metric.name == "memorisation"


def test_replayed_training_rows_beat_wasserstein_and_are_caught():
    """The point of the feature: a generator that replays its training set has a sliced Wasserstein distance BELOW the baseline of
    two real folds, full precision and recall -- and no authenticity at all."""
    from functools import partial

    from fourierdiffusion_amd.sampling.metrics import Memorisation, MetricCollection, PrecisionRecall, SlicedWasserstein
    X = metric_sets()[0]
    H = np.random.RandomState(78).randn(*X.shape).astype(np.float32)      # as large as the training set: compared with all of it
    replay = X + 1e-4 * np.random.RandomState(5).randn(*X.shape).astype(np.float32)
    mc = MetricCollection(metrics=[partial(SlicedWasserstein, random_seed=42, num_directions=50), partial(PrecisionRecall, k=5),
                                   partial(Memorisation, random_seed=0)], original_samples=torch.from_numpy(X),
                          holdout_samples=torch.from_numpy(H))
    res = mc(torch.from_numpy(replay))
    assert list(res) == sorted(res)
    for view in ("time", "freq"):
        assert res[f"{view}_sliced_wasserstein_mean"] < res[f"{view}_sliced_wasserstein_mean_self"]
        assert res[f"{view}_authenticity"] <= 0.02 and res[f"{view}_train_closer_share"] >= 0.98
        assert res[f"{view}_precision"] == 1.0 and res[f"{view}_recall"] == 1.0 and res[f"{view}_coverage"] == 1.0
        assert res[f"{view}_nn_distance_median"] < 1e-2 and f"{view}_precision_self" in res
    fresh = np.random.RandomState(79).randn(*X.shape).astype(np.float32)
    held = mc(torch.from_numpy(fresh))                           # an independent draw of the data: nothing memorised
    assert held["time_authenticity"] >= 0.3 and abs(held["time_train_closer_share"] - 0.5) <= 0.15      # (4 sigma of 200 fair coins)
    # without the holdout the collection has no share to report, and the Wasserstein keys are the ones it always had
    plain = MetricCollection(metrics=[partial(SlicedWasserstein, random_seed=42, num_directions=50)], original_samples=torch.from_numpy(X))
    same = plain(torch.from_numpy(replay))
    assert all(res[key] == val for key, val in same.items())


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_sample_with_neighbour_metrics(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=1", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=knnrun"], tmp_path)
    _run([str(ROOT / "cmd" / "sample.py"), "model_id=knnrun", "metrics=neighbours", "num_diffusion_steps=5", "num_samples=64",
          "sampler.sample_batch_size=32"], tmp_path)
    res = yaml.safe_load(open(tmp_path / "lightning_logs" / "knnrun" / "results.yaml"))
    for view in ("time", "freq"):
        for key in ("precision", "recall", "coverage", "authenticity", "train_closer_share", "precision_self", "coverage_self"):
            assert 0.0 <= res[f"{view}_{key}"] <= 1.0, (view, key)
        for key in ("density", "density_self", "nn_distance_min", "nn_distance_median"):
            assert res[f"{view}_{key}"] >= 0.0 and np.isfinite(res[f"{view}_{key}"]), (view, key)
    assert res["time_sliced_wasserstein_mean"] >= 0.0 and len(res["time_sliced_wasserstein_all"]) == 1000


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """Every new entry point refuses each bad argument with FD_ERR_ARG and a retrievable message."""
    from fourierdiffusion_amd import _C
    x, y = torch.zeros(8, 9, device="cuda"), torch.zeros(6, 9, device="cuda")
    d2, ix = torch.zeros(8, 3, device="cuda"), torch.zeros(8, 3, dtype=torch.int32, device="cuda")
    rad, cnt = torch.zeros(6, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    h, L = _C.ctx(x.device), _C.lib()
    need = C.c_size_t(0)
    assert L.fd_knn_rows_workspace_bytes(h, 8, 6, 9, 3, C.byref(need)) == 0 and need.value > 0
    work = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    p, q, dp, ip, wp, nb = x.data_ptr(), y.data_ptr(), d2.data_ptr(), ix.data_ptr(), work.data_ptr(), need.value
    big = 1 << 30
    cases = [
        (lambda: L.fd_knn_rows_workspace_bytes(h, 8, 6, 9, 3, None), b"null"),
        (lambda: L.fd_knn_rows_workspace_bytes(h, 0, 6, 9, 3, C.byref(need)), b"bad shape"),
        (lambda: L.fd_knn_rows_workspace_bytes(h, 8, 6, 0, 3, C.byref(need)), b"bad shape"),
        (lambda: L.fd_knn_rows_workspace_bytes(h, 8, 6, 9, 0, C.byref(need)), b"k=0"),
        (lambda: L.fd_knn_rows_workspace_bytes(h, 8, 6, 9, 7, C.byref(need)), b"k=7"),
        (lambda: L.fd_knn_rows_workspace_bytes(h, 8, 40, 9, 17, C.byref(need)), b"k=17"),
        (lambda: L.fd_knn_rows_workspace_bytes(h, big, 6, 9, 3, C.byref(need)), b"too large"),
        (lambda: L.fd_knn_rows_workspace_bytes(h, 8, big, 9, 3, C.byref(need)), b"too large"),
        (lambda: L.fd_knn_rows(h, None, 8, q, 6, 9, 3, 0, dp, ip, wp, nb, None), b"null"),
        (lambda: L.fd_knn_rows(h, p, 8, None, 6, 9, 3, 0, dp, ip, wp, nb, None), b"null"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, 9, 3, 0, None, ip, wp, nb, None), b"null"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, 9, 3, 0, dp, None, wp, nb, None), b"null"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, 9, 3, 0, dp, ip, None, nb, None), b"null"),
        (lambda: L.fd_knn_rows(h, p, 0, q, 6, 9, 3, 0, dp, ip, wp, nb, None), b"bad shape"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 0, 9, 3, 0, dp, ip, wp, nb, None), b"bad shape"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, -1, 3, 0, dp, ip, wp, nb, None), b"bad shape"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, 9, 0, 0, dp, ip, wp, nb, None), b"k=0"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, 9, 7, 0, dp, ip, wp, nb, None), b"k=7"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 40, 9, 17, 0, dp, ip, wp, nb, None), b"k=17"),
        (lambda: L.fd_knn_rows(h, p, 8, p, 8, 9, 8, 1, dp, ip, wp, nb, None), b"k=8"),          # only 7 other rows
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, 9, 3, 1, dp, ip, wp, nb, None), b"exclude_self"),   # q != r
        (lambda: L.fd_knn_rows(h, p, 8, p, 6, 9, 3, 1, dp, ip, wp, nb, None), b"exclude_self"),   # n != m
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, 9, 3, 0, dp, ip, wp, nb - 1, None), b"workspace"),
        (lambda: L.fd_knn_rows(h, p, 8, q, 6, 9, 3, 0, dp, ip, wp, 0, None), b"workspace"),
        (lambda: L.fd_knn_rows(h, p, big, q, 6, 9, 3, 0, dp, ip, wp, nb, None), b"too large"),
        (lambda: L.fd_knn_rows(h, p, 8, q, big, 9, 3, 0, dp, ip, wp, nb, None), b"too large"),
        (lambda: L.fd_ball_counts(h, None, 8, q, 6, 9, rad.data_ptr(), cnt.data_ptr(), None), b"null"),
        (lambda: L.fd_ball_counts(h, p, 8, None, 6, 9, rad.data_ptr(), cnt.data_ptr(), None), b"null"),
        (lambda: L.fd_ball_counts(h, p, 8, q, 6, 9, None, cnt.data_ptr(), None), b"null"),
        (lambda: L.fd_ball_counts(h, p, 8, q, 6, 9, rad.data_ptr(), None, None), b"null"),
        (lambda: L.fd_ball_counts(h, p, 0, q, 6, 9, rad.data_ptr(), cnt.data_ptr(), None), b"bad shape"),
        (lambda: L.fd_ball_counts(h, p, 8, q, 6, 0, rad.data_ptr(), cnt.data_ptr(), None), b"bad shape"),
        (lambda: L.fd_ball_counts(h, p, 8, q, big, 9, rad.data_ptr(), cnt.data_ptr(), None), b"too large"),
    ]
    for i, (call, needle) in enumerate(cases):
        assert call() == -1, i
        assert needle in L.fd_last_error(h), (i, L.fd_last_error(h))
    assert L.fd_knn_rows(None, p, 8, q, 6, 9, 3, 0, dp, ip, wp, nb, None) == -1          # no context: error code only
    assert L.fd_ball_counts(None, p, 8, q, 6, 9, rad.data_ptr(), cnt.data_ptr(), None) == -1
    # and the arguments they were derived from are accepted
    assert L.fd_knn_rows(h, p, 8, q, 6, 9, 3, 0, dp, ip, wp, nb, None) == 0
    assert L.fd_ball_counts(h, p, 8, q, 6, 9, rad.data_ptr(), cnt.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (ix.cpu().numpy() == np.array([0, 1, 2])[None]).all() and (cnt.cpu().numpy() == 6).all()
