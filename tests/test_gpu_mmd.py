"""GPU: the kernel two-sample test (fd_kernel_quadforms: csrc/fd_mmd.hip; utils/two_sample.py; sampling/metrics.py KernelTwoSample)
against the float64 brute force of tests/mmd_ref.py.

The bound.  With u = 2^-24, delta_ij the expansion error of the centred f32 distances (knn_ref.expansion_bound) and c the rows of the
longest fp32 addition chain (mmd_ref.group_rows), the contract is |quad~_p - quad_p| <= sum_{i != j} A_ip A_jp eps_ij + c u quad_p
with eps_ij = delta_ij / (min_q c_q base2) + 8 u, and the same with the sums over j for rowsum and col0 (mmd_ref.error_bounds:
derived, not tuned).  The MMD^2 values are further held to 8 times the deviation of the float32 numpy restatement of the same
arithmetic plus 1e-7: the worst case is far above what a different summation order and the hardware exponential can explain.

Measured on an MI355X (the table per case is in DESIGN.md 3.25): the largest error is 2.3e-5 to 1.9e-2 of the worst-case bound; the
MMD^2 error is 0.28 to 0.96 of the restatement's own deviation (2.7e-9 to 2.1e-7 against 6.5e-9 to 2.2e-7), except at (1, 40, 9, 1),
where a single column over 41 rows has nothing to average over: 2.1e-7 against 2.8e-8, 0.64 of the allowed 8 x + 1e-7.  No column of
the float64 reference lies within 2 Delta of its observed value at any case, and every p-value equals the reference's."""
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

from tests import mmd_ref as R

from .gpu_util import dev, log_line

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SCALES = R.DEFAULT_SCALES

# (n, m, d, P, kind): P counts every column, the observed split included
SHAPES = {
    "5+7x3_P17": (5, 7, 3, 17, "waves"),                         # below one tile
    "128+128x16_P65": (128, 128, 16, 65, "waves"),               # exact tiles
    "129+127x17_P64": (129, 127, 17, 64, "waves"),               # ragged everywhere
    "300+200x187_P201": (300, 200, 187, 201, "waves"),           # several tiles both ways
    "64+700x1200_P101": (64, 700, 1200, 101, "waves"),           # unbalanced; the bench width
    "200+200x62_P201_shifted": (200, 200, 62, 201, "shifted"),   # the centring: every row + 3, the second set scaled by 1.2
    "1+40x9_P1": (1, 40, 9, 1, "waves"),                         # the ends of the ranges
    "40+40x9_P1024": (40, 40, 9, 1024, "waves"),
    "2100+2000x6_P3": (2100, 2000, 6, 3, "waves"),               # 33 tiles: groups of two tiles, the fp32 chain crosses a tile
}
SPLIT_SHAPES = ["129+127x17_P64", "300+200x187_P201", "64+700x1200_P101", "2100+2000x6_P3"]


def quadforms_raw(z, A, scales=SCALES, bandwidth2=0.0, col_splits=0, with_col0=True):
    """fd_kernel_quadforms through the C ABI on device tensors: (quad, rowsum, col0, base2) as numpy float64."""
    from fourierdiffusion_amd import _C
    N, d = z.shape
    P = A.shape[1]
    h, L = _C.ctx(z.device), _C.lib()
    need = C.c_size_t(0)
    _C.check(L.fd_kernel_quadforms_workspace_bytes(h, N, d, P, col_splits, C.byref(need)), h)
    work = torch.empty((need.value,), dtype=torch.uint8, device=z.device)
    quad = torch.full((P,), -1.0, dtype=torch.float64, device=z.device)
    rowsum = torch.full((N,), -1.0, dtype=torch.float64, device=z.device)
    col0 = torch.full((N,), -1.0, dtype=torch.float64, device=z.device)
    base2 = torch.full((1,), -1.0, dtype=torch.float64, device=z.device)
    cs = (C.c_double * len(scales))(*scales)
    _C.check(L.fd_kernel_quadforms(h, z.data_ptr(), N, d, cs, len(scales), float(bandwidth2), A.data_ptr(), P, col_splits,
                                   quad.data_ptr(), rowsum.data_ptr(), col0.data_ptr() if with_col0 else None, base2.data_ptr(),
                                   work.data_ptr(), need.value, _C.stream_of(z)), h)
    return quad.cpu().numpy(), rowsum.cpu().numpy(), col0.cpu().numpy(), float(base2.cpu().numpy()[0])


def oracle(z, A, scales=SCALES, bandwidth2=None):
    """The float64 reference of one input and the bounds that go with it."""
    D = R.dist2(z, z, chunk=16)
    base2 = R.pooled_base2(D) if bandwidth2 is None else bandwidth2
    K = R.kernel_matrix(D, scales, base2)
    del D
    quad, rowsum, col0 = R.quadforms(K, A)
    b_quad, b_rowsum, b_col0 = R.error_bounds(z, A, scales, base2, K)
    return dict(z=z, A=A, K=K, base2=base2, quad=quad, rowsum=rowsum, col0=col0, b_quad=b_quad, b_rowsum=b_rowsum, b_col0=b_col0,
                mmd2=R.mmd2_from_sums(quad, rowsum, A))


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the float64 reference and the float32 restatement of one shape, computed once and shared (nothing below writes to
    them)."""
    n, m, d, P, kind = SHAPES[name]
    rng = np.random.default_rng(len(name) * 1000 + n + m + d)
    if kind == "shifted":
        x, y = rng.standard_normal((n, d)) + 3.0, 1.2 * rng.standard_normal((m, d)) + 3.0
    else:
        x, y = R.waves(rng, n, d), R.waves(rng, m, d)
    z = np.concatenate([x, y]).astype(np.float32)
    A = R.permutation_members(n, m, P - 1, seed=n + m)
    c = oracle(z, A)
    rq, rr, _ = R.restate_f32(z, A, SCALES, c["base2"])
    c["restate_dev"] = float(np.abs(R.mmd2_from_sums(rq, rr, A) - c["mmd2"]).max())
    return c


def check_against(c, got, tag):
    """The worst-case bound on the three outputs of one engine result against the reference c; returns the MMD^2 of every column."""
    quad, rowsum, col0, base2 = got
    assert abs(base2 - c["base2"]) <= 1e-12 * c["base2"]
    for key, val in (("quad", quad), ("rowsum", rowsum), ("col0", col0)):
        err, bound = np.abs(val - c[key]), c["b_" + key]
        ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)      # (a group of one row: no pair, bound 0, value 0)
        log_line(f"[mmd] {tag}: {key} error / worst-case bound: max {ratio.max():.3e}")
        assert (err <= bound).all(), (key, ratio.max())
    assert (rowsum <= len(rowsum) - 1).all() and (rowsum >= 0).all() and (col0 >= 0).all() and (col0 <= rowsum).all()
    return R.mmd2_from_sums(quad, rowsum, c["A"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_quadforms_and_p_value_against_float64(name):
    from fourierdiffusion_amd.utils.two_sample import mmd2_from_quadforms, permutation_p_value
    c = case(name)
    got = quadforms_raw(dev(c["z"]), torch.from_numpy(c["A"]).cuda())
    mmd2 = check_against(c, got, name)
    np.testing.assert_array_equal(mmd2_from_quadforms(got[0], got[1], c["A"]), mmd2)
    # precision: the restatement of the same arithmetic in numpy float32 sets the scale
    delta = float(np.abs(mmd2 - c["mmd2"]).max())
    log_line(f"[mmd] {name}: mmd2 error {delta:.3e}, restatement deviation {c['restate_dev']:.3e}, ratio "
             f"{delta / max(c['restate_dev'], 1e-300):.3f}; observed {c['mmd2'][0]:.3e}, null sd "
             f"{np.std(c['mmd2'][1:]) if len(mmd2) > 1 else 0.0:.3e}")
    assert delta <= 8.0 * c["restate_dev"] + 1e-7
    # p-value: the rule on the engine's own statistics; it can differ from the reference's only by the columns too close to call
    P = len(mmd2)
    p_engine, p_ref = permutation_p_value(mmd2), R.p_value(c["mmd2"])
    assert p_engine == (1 + int((mmd2[1:] >= mmd2[0]).sum())) / P
    close = int((np.abs(c["mmd2"][1:] - c["mmd2"][0]) <= 2.0 * delta).sum())
    log_line(f"[mmd] {name}: p-value {p_engine:.4f} (float64 {p_ref:.4f}), {close} of {P} columns within 2 Delta of the observed")
    assert close <= 0.05 * P
    assert abs(p_engine - p_ref) <= close / P + 1e-15
    if SHAPES[name][4] == "shifted":
        assert p_engine == 1 / 201 and p_ref == 1 / 201


@pytest.mark.parametrize("name", SPLIT_SHAPES)
def test_results_are_bit_identical_for_every_col_split_and_run(name):
    c = case(name)
    z, A = dev(c["z"]), torch.from_numpy(c["A"]).cuda()
    first = quadforms_raw(z, A, col_splits=1)
    for splits in (1, 2, 7, 0):
        again = quadforms_raw(z, A, col_splits=splits)
        for a, b in zip(first, again):
            np.testing.assert_array_equal(a, b, err_msg=f"col_splits={splits}")
    without = quadforms_raw(z, A, with_col0=False)                 # a NULL col0 leaves the rest alone (and the buffer untouched)
    np.testing.assert_array_equal(without[0], first[0])
    np.testing.assert_array_equal(without[1], first[1])
    assert (without[2] == -1.0).all()


def test_given_bandwidth_and_other_scales():
    n, m, d, P = 90, 70, 33, 40
    rng = np.random.default_rng(17)
    z = np.concatenate([R.waves(rng, n, d), R.waves(rng, m, d)]).astype(np.float32)
    A = R.permutation_members(n, m, P - 1, seed=2)
    for scales, bw2 in (((1.0,), 7.5), ((0.3, 0.7, 1.0, 1.5, 2.0, 3.0, 5.0, 9.0), None), ((2.0, 0.5), 30.0)):
        c = oracle(z, A, scales, bw2)
        got = quadforms_raw(dev(z), torch.from_numpy(A).cuda(), scales=scales, bandwidth2=0.0 if bw2 is None else bw2)
        check_against(c, got, f"scales={scales} bandwidth2={bw2}")


def test_planted_bit_copies_keep_the_bound_and_no_kernel_value_exceeds_one():
    n, m, d, P = 150, 170, 40, 33
    rng = np.random.default_rng(23)
    x, y = R.waves(rng, n, d).astype(np.float32), R.waves(rng, m, d).astype(np.float32)
    y[:60] = x[40:100]                                            # bit-copies across the two sets
    y[100:110] = y[99]                                            # and a run of equal rows inside one
    z = np.concatenate([x, y])
    A = R.permutation_members(n, m, P - 1, seed=5)
    c = oracle(z, A)
    got = quadforms_raw(dev(z), torch.from_numpy(A).cuda())
    check_against(c, got, "planted copies")
    assert (got[1] <= n + m - 1).all()
    same = quadforms_raw(dev(np.repeat(x[:1], 50, axis=0)), torch.from_numpy(A[:50]).cuda())       # base2 = 0: every value is 1
    assert same[3] == 0.0 and (same[1] == 49.0).all()
    k = A[:50].sum(axis=0).astype(np.float64)
    np.testing.assert_array_equal(same[0], k * (k - 1))


def test_permuting_the_pooled_rows_with_their_memberships_keeps_quad():
    c = case("129+127x17_P64")
    perm = np.random.default_rng(9).permutation(len(c["z"]))
    got = quadforms_raw(dev(c["z"][perm]), torch.from_numpy(np.ascontiguousarray(c["A"][perm])).cuda())
    assert (np.abs(got[0] - c["quad"]) <= c["b_quad"]).all()
    assert (np.abs(got[1] - c["rowsum"][perm]) <= c["b_rowsum"][perm]).all()
    straight = quadforms_raw(dev(c["z"]), torch.from_numpy(c["A"]).cuda())
    assert (np.abs(got[0] - straight[0]) <= 2.0 * c["b_quad"]).all()


# ---------------------------------------------------------------------------------------------- Python surface
def test_python_surface_against_float64():
    from fourierdiffusion_amd.utils.two_sample import kernel_quadforms, mmd_permutation_test
    name = "300+200x187_P201"
    c = case(name)
    n, m = SHAPES[name][:2]
    quad, rowsum, col0, base2 = kernel_quadforms(c["z"], c["A"])
    assert all(t.is_cuda and t.dtype == torch.float64 for t in (quad, rowsum, col0, base2))
    raw = quadforms_raw(dev(c["z"]), torch.from_numpy(c["A"]).cuda())
    np.testing.assert_array_equal(quad.cpu().numpy(), raw[0])
    np.testing.assert_array_equal(kernel_quadforms(torch.from_numpy(c["z"]), torch.from_numpy(c["A"]).bool(), col_splits=3)[1]
                                  .cpu().numpy(), raw[1])
    # the test itself draws the same memberships (seed = n + m in case()), so the reference's columns are its columns
    res = mmd_permutation_test(c["z"][:n], c["z"][n:], n_permutations=200, seed=n + m)
    tol = 8.0 * c["restate_dev"] + 1e-7
    assert abs(res.mmd2 - c["mmd2"][0]) <= tol and res.null.shape == (200,) and np.abs(res.null - c["mmd2"][1:]).max() <= tol
    assert res.p_value == (1 + int((res.null >= res.mmd2).sum())) / 201
    assert res.bandwidth2 == pytest.approx(c["base2"], rel=1e-12)
    want = R.witness(c["K"], c["A"][:, 0])
    a0 = c["A"][:, 0].astype(np.float64)
    slack = c["b_col0"] / (n - a0) + (c["b_rowsum"] + c["b_col0"]) / (m - (1.0 - a0))
    got = np.concatenate([res.witness_x, res.witness_y])
    assert res.witness_x.shape == (n,) and res.witness_y.shape == (m,) and (np.abs(got - want) <= slack).all()
    # 3-d samples are flattened, and a given bandwidth is used as it is
    shaped = mmd_permutation_test(c["z"][:n].reshape(n, 11, 17), c["z"][n:].reshape(m, 11, 17), n_permutations=200, seed=n + m)
    assert shaped.mmd2 == res.mmd2 and shaped.p_value == res.p_value
    assert mmd_permutation_test(c["z"][:n], c["z"][n:], n_permutations=5, bandwidth2=40.0).bandwidth2 == 40.0


@functools.lru_cache(maxsize=None)
def point_data():
    rng = np.random.default_rng(100)
    train, fresh = R.waves(rng, 400, 96), R.waves(rng, 400, 96)
    return train.astype(np.float32), fresh.astype(np.float32), (0.85 * R.waves(rng, 400, 96)).astype(np.float32)


def test_a_fresh_fold_is_not_told_apart_and_a_shrunk_generator_is():
    from fourierdiffusion_amd.utils.two_sample import mmd_permutation_test
    train, fresh, shrunk = point_data()
    same = mmd_permutation_test(fresh, train, n_permutations=200, seed=0)
    log_line(f"[mmd] fresh fold: mmd2 {same.mmd2:.3e}, p {same.p_value:.4f}, null sd {same.null.std():.3e}")
    assert same.p_value > 0.05
    apart = mmd_permutation_test(shrunk, train, n_permutations=200, seed=0)
    log_line(f"[mmd] amplitude x 0.85: mmd2 {apart.mmd2:.3e}, p {apart.p_value:.4f}, null sd {apart.null.std():.3e}")
    assert apart.p_value == 1 / 201
    assert apart.witness_x.mean() > apart.witness_y.mean()          # the witness is larger where the first set has the mass


def test_kernel_two_sample_metric_in_a_collection():
    from fourierdiffusion_amd.sampling.metrics import KernelTwoSample, MetricCollection
    train, fresh, shrunk = point_data()
    shape = (-1, 48, 2)
    held = R.waves(np.random.default_rng(101), 300, 96).astype(np.float32)
    mc = MetricCollection(metrics=[partial(KernelTwoSample, n_permutations=200, random_seed=0)],
                          original_samples=torch.from_numpy(train.reshape(shape)), holdout_samples=torch.from_numpy(held.reshape(shape)))
    res = mc(torch.from_numpy(shrunk.reshape(shape)))
    assert list(res) == sorted(res) and len(res) == 12
    # the time view is the test of the flat rows: against float64 with the same memberships
    for other, key in ((train, ""), (held, "_holdout")):
        z = np.concatenate([shrunk, other])
        A = R.permutation_members(400, len(other), 200, 0)
        c = oracle(z, A)
        rq, rr, _ = R.restate_f32(z, A, SCALES, c["base2"])
        tol = 8.0 * float(np.abs(R.mmd2_from_sums(rq, rr, A) - c["mmd2"]).max()) + 1e-7
        assert abs(res["time_mmd2" + key] - c["mmd2"][0]) <= tol
        assert res["time_mmd_p_value" + key] == R.p_value(c["mmd2"]) == 1 / 201
    for view in ("time", "freq"):
        assert res[f"{view}_mmd_p_value"] == 1 / 201 and res[f"{view}_mmd_p_value_holdout"] == 1 / 201
        assert res[f"{view}_mmd_p_value_self"] > 0.05 and abs(res[f"{view}_mmd2_self"]) < res[f"{view}_mmd2"]
    ok = mc(torch.from_numpy(fresh.reshape(shape)))
    assert ok["time_mmd_p_value"] > 0.05 and ok["time_mmd_p_value_holdout"] > 0.05
    sub = KernelTwoSample(torch.from_numpy(train), n_permutations=50, max_original=100, random_seed=3)
    assert sub.original_samples.shape == (100, 96) and 0 < sub(torch.from_numpy(fresh))["mmd_p_value"] <= 1


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_sample_with_two_sample_metric(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=1", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=mmdrun"], tmp_path)
    _run([str(ROOT / "cmd" / "sample.py"), "model_id=mmdrun", "metrics=two_sample", "num_diffusion_steps=5", "num_samples=64",
          "sampler.sample_batch_size=32"], tmp_path)
    res = yaml.safe_load(open(tmp_path / "lightning_logs" / "mmdrun" / "results.yaml"))
    for view in ("time", "freq"):
        for suffix in ("", "_holdout", "_self"):
            assert np.isfinite(res[f"{view}_mmd2{suffix}"]), (view, suffix)
            assert 0.0 < res[f"{view}_mmd_p_value{suffix}"] <= 1.0, (view, suffix)
    assert res["time_sliced_wasserstein_mean"] >= 0.0 and len(res["time_sliced_wasserstein_all"]) == 1000


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """Both entry points refuse each bad argument with FD_ERR_ARG and a retrievable message."""
    from fourierdiffusion_amd import _C
    z = torch.arange(72.0, device="cuda").reshape(8, 9)
    A = torch.zeros(8, 3, dtype=torch.uint8, device="cuda")
    A[:4] = 1
    quad, rows, col0 = (torch.zeros(k, dtype=torch.float64, device="cuda") for k in (3, 8, 8))
    base2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    h, L = _C.ctx(z.device), _C.lib()
    need = C.c_size_t(0)
    assert L.fd_kernel_quadforms_workspace_bytes(h, 8, 9, 3, 0, C.byref(need)) == 0 and need.value > 0
    work = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    zp, ap, qp, rp, cp, bp, wp, nb = (z.data_ptr(), A.data_ptr(), quad.data_ptr(), rows.data_ptr(), col0.data_ptr(), base2.data_ptr(),
                                      work.data_ptr(), need.value)
    sc = (C.c_double * 8)(0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)

    def call(z=zp, N=8, d=9, scales=sc, nq=5, bw2=0.0, member=ap, P=3, splits=0, quad=qp, rows=rp, col0=cp, base2=bp, work=wp,
             bytes_=nb):
        return L.fd_kernel_quadforms(h, z, N, d, scales, nq, bw2, member, P, splits, quad, rows, col0, base2, work, bytes_, None)

    def bad_scale(v):
        return (C.c_double * 2)(1.0, v)

    big = 1 << 30
    cases = [
        (lambda: L.fd_kernel_quadforms_workspace_bytes(h, 8, 9, 3, 0, None), b"null"),
        (lambda: L.fd_kernel_quadforms_workspace_bytes(h, 1, 9, 3, 0, C.byref(need)), b"bad shape"),
        (lambda: L.fd_kernel_quadforms_workspace_bytes(h, 8, 0, 3, 0, C.byref(need)), b"bad shape"),
        (lambda: L.fd_kernel_quadforms_workspace_bytes(h, 8, 9, 0, 0, C.byref(need)), b"P=0"),
        (lambda: L.fd_kernel_quadforms_workspace_bytes(h, 8, 9, 1025, 0, C.byref(need)), b"P=1025"),
        (lambda: L.fd_kernel_quadforms_workspace_bytes(h, 8, 9, 3, -1, C.byref(need)), b"col_splits"),
        (lambda: L.fd_kernel_quadforms_workspace_bytes(h, big, 9, 3, 0, C.byref(need)), b"too large"),
        (lambda: L.fd_kernel_quadforms_workspace_bytes(h, 1 << 22, 9, 1024, 0, C.byref(need)), b"too large"),
        (lambda: call(z=None), b"null"), (lambda: call(scales=None), b"null"), (lambda: call(member=None), b"null"),
        (lambda: call(quad=None), b"null"), (lambda: call(rows=None), b"null"), (lambda: call(base2=None), b"null"),
        (lambda: call(work=None), b"null"),
        (lambda: call(N=1), b"bad shape"), (lambda: call(N=0), b"bad shape"), (lambda: call(d=0), b"bad shape"),
        (lambda: call(d=-3), b"bad shape"),
        (lambda: call(P=0), b"P=0"), (lambda: call(P=1025), b"P=1025"), (lambda: call(splits=-2), b"col_splits"),
        (lambda: call(nq=0), b"n_scales=0"), (lambda: call(nq=9), b"n_scales=9"),
        (lambda: call(scales=bad_scale(0.0), nq=2), b"scale 1"), (lambda: call(scales=bad_scale(-1.0), nq=2), b"scale 1"),
        (lambda: call(scales=bad_scale(float("nan")), nq=2), b"scale 1"), (lambda: call(scales=bad_scale(float("inf")), nq=2), b"scale 1"),
        (lambda: call(bw2=float("nan")), b"bandwidth2"), (lambda: call(bw2=float("inf")), b"bandwidth2"),
        (lambda: call(N=big), b"too large"), (lambda: call(N=1 << 22, P=1024), b"too large"),
        (lambda: call(bytes_=nb - 1), b"workspace"), (lambda: call(bytes_=0), b"workspace"),
    ]
    for i, (fn, needle) in enumerate(cases):
        assert fn() == -1, i
        assert needle in L.fd_last_error(h), (i, L.fd_last_error(h))
    assert L.fd_kernel_quadforms(None, zp, 8, 9, sc, 5, 0.0, ap, 3, 0, qp, rp, cp, bp, wp, nb, None) == -1     # no context: the code only
    assert L.fd_kernel_quadforms_workspace_bytes(None, 8, 9, 3, 0, C.byref(need)) == -1
    # and the arguments they were derived from are accepted, with and without col0
    assert call() == 0 and call(col0=None, nq=8) == 0
    torch.cuda.synchronize()
    assert base2.item() > 0 and quad.cpu().numpy()[0] > 0 and (rows.cpu().numpy() > 0).all()
