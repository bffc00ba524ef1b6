"""GPU parity: the Philox normals (fd_randn / fd_randn4 of csrc/fd_philox.h) against the oracle's float64 restatement of Box-Muller
on the Philox words (engine_randn), and the streaming kernels of csrc/fd_sde.hip -- k_sde_step<NT> in both instantiations, k_prior,
k_perturb, k_langevin, k_dsm_loss -- against the float64 oracle at the shapes where their two-groups-per-thread loop, predicated
tails, row carries and grid-stride sweeps take another path.

NOISE_BOUND: max |fd_randn - engine_randn| over the bulk set (three (seed, offset) pairs x (2^20 + 3) draws) and the edge counters of
tests/noise_edges.py, measured on an MI355X against the float64 restatement (never against the kernel): 9.842e-7 (NOISE_MEASURED
below; the largest |z| among them 5.28, the extreme 5.887 is the edge counter's); the asserted bound is 4 x that, 3.937e-6, because the error of the hardware log / sine / cosine depends on the argument and 3 M draws visit a
vanishing part of the 2^48 (u1, u2) pairs.  Every other tolerance here is the one of the project's existing test of the
same kernel (tests/test_gpu_sde.py, tests/test_gpu_backbones.py)."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W

from . import noise_edges as NE
from .gpu_util import DEV, dev, host, log_line, oracle_sde, report_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

NOISE_MEASURED = 9.842e-7        # bulk 7.406e-7 / 6.229e-7 / 9.842e-7 for the three pairs, edges 1.703e-7
NOISE_BOUND = 4.0 * NOISE_MEASURED   # 3.937e-6
Z_MAX = 5.89                     # sqrt(-2 ln 2^-25) = 5.887: the largest radius fd_u01 allows

PAIRS = [(0, 0), (0x1234567890ABCDEF, 0xFFFFFFF0), (0xFFFFFFFFFFFFFFFF, (1 << 40) + 12345)]   # test_gpu_sde.py's generator test
N_BULK = (1 << 20) + 3
SDES = {"vp": (0, (0.1, 20.0)), "ve": (1, (0.01, 5.0))}
SEED, OFFSET = 0x1234567890ABCDEF, 0xFFFFFFF0        # the on-device draws of the kernel tests: counters cross 2^32 after 16 groups
GUARD = 5


# ------------------------------------------------------------------------------------------------------------ C ABI wrappers
def _eng():
    from fourierdiffusion_amd import _C
    return _C, _C.lib(), _C.ctx(torch.device("cuda", torch.cuda.current_device()))


def _guarded(n):
    return torch.full((n + GUARD,), 9.0, device=DEV)


def _take(buf, n):
    """The n outputs of a guarded buffer; the words behind them must be untouched."""
    torch.cuda.synchronize()
    assert bool((buf[n:] == 9.0).all()), "the kernel wrote past the end of its output"
    return buf[:n].clone()


def randn_dev(seed, offset, n):
    _C, L, h = _eng()
    buf = _guarded(n)
    _C.check(L.fd_randn(h, buf.data_ptr(), n, seed, offset, None), h)
    return _take(buf, n)


def _params(kind):
    from fourierdiffusion_amd import _C
    return _C.SdeParams(SDES[kind][0], *SDES[kind][1])


def step_dev(kind, G, x, score, z, t, dt, shape, seed=0, offset=0):
    _C, L, h = _eng()
    B, T, Cn = shape
    n = B * T * Cn
    buf, p = _guarded(n), _params(kind)
    _C.check(L.fd_sde_step(h, C.byref(p), G.data_ptr(), x.data_ptr(), score.data_ptr(), _C.ptr(z), seed, offset, float(t), float(dt),
                           buf.data_ptr(), B, T, Cn, None), h)
    return _take(buf, n)


def prior_dev(kind, G, z, shape, seed=0, offset=0):
    _C, L, h = _eng()
    B, T, Cn = shape
    n = B * T * Cn
    buf, p = _guarded(n), _params(kind)
    _C.check(L.fd_prior_sample(h, C.byref(p), G.data_ptr(), _C.ptr(z), seed, offset, buf.data_ptr(), B, T, Cn, None), h)
    return _take(buf, n)


def perturb_dev(kind, G, x, t, z, shape, seed=0, offset=0, aux=True):
    """(x_noisy, target, std); aux = False passes target = std_out = NULL."""
    _C, L, h = _eng()
    B, T, Cn = shape
    n = B * T * Cn
    xn, p = _guarded(n), _params(kind)
    tg, sd = (_guarded(n), _guarded(B * T)) if aux else (None, None)
    _C.check(L.fd_perturb(h, C.byref(p), G.data_ptr(), x.data_ptr(), t.data_ptr(), _C.ptr(z), seed, offset, xn.data_ptr(), _C.ptr(tg),
                          _C.ptr(sd), B, T, Cn, None), h)
    return (_take(xn, n), _take(tg, n), _take(sd, B * T)) if aux else (_take(xn, n), None, None)


def langevin_dev(G, x, score, z, shape, seed=0, offset=0, snr=0.16, alpha=0.93):
    _C, L, h = _eng()
    B, T, Cn = shape
    n = B * T * Cn
    buf = _guarded(n)
    _C.check(L.fd_langevin_step(h, G.data_ptr(), x.data_ptr(), score.data_ptr(), _C.ptr(z), seed, offset, snr, alpha, buf.data_ptr(),
                                B, T, Cn, None), h)
    return _take(buf, n)


def _flat(a):
    return np.asarray(a, dtype=np.float64).reshape(-1)


def _within(tag, got, ref, tol):
    """|got - ref| <= tol element by element (tol an array or a scalar); logs the worst error and its share of the tolerance."""
    got, ref = _flat(got), _flat(ref)
    err = np.abs(got - ref)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64).reshape(-1) if np.ndim(tol) else np.float64(tol), err.shape)
    i = int(np.argmax(err / tol))
    log_line(f"[parity] {tag}: max |err| = {err.max():.3e}, worst err / tol = {err[i] / tol[i]:.3f} (n = {err.size})")
    ok = bool(np.isfinite(got).all() and (err <= tol).all())
    return ok, f"{tag}: err {err[i]:.3e} > tol {tol[i]:.3e} at element {i} (got {got[i]!r}, ref {ref[i]!r})"


def _noise_coef(fn):
    """|d out / d z| of an oracle map that is affine in z, element by element: the map at z = 1 minus the map at z = 0."""
    return np.abs(_flat(fn(1.0)) - _flat(fn(0.0)))


# ------------------------------------------------------------------------------------------------------- B. fd_randn
def test_randn_bulk_vs_restatement():
    worst = 0.0
    for seed, offset in PAIRS:
        got = host(randn_dev(seed, offset, N_BULK))
        ref = O.engine_randn(seed, offset, N_BULK)
        assert np.isfinite(got).all(), (seed, offset)
        err = float(np.abs(got - ref).max())
        log_line(f"[parity] fd_randn vs float64 Box-Muller seed={seed:#x} offset={offset:#x} n={N_BULK}: max |err| = {err:.3e}, "
                 f"max |z| = {np.abs(got).max():.4f}")
        worst = max(worst, err)
        assert np.abs(got).max() <= Z_MAX, (seed, offset)
        assert err <= NOISE_BOUND, (seed, offset, err, int(np.argmax(np.abs(got - ref))))
    log_line(f"[parity] fd_randn bulk: max |fd_randn - engine_randn| = {worst:.3e} (recorded {NOISE_MEASURED:.3e}, bound {NOISE_BOUND:.3e})")


def test_randn_lane_layout():
    """fd_randn(offset = o, n = 4 k) is engine_randn's (k, 4): counter o + row, lane = column.  A permutation of the reference's
    lanes misses the bound by far more than 100 x, so the bound does see a layout error."""
    o, k = 0xFFFFFFF0, 1000
    got = host(randn_dev(7, o, 4 * k)).reshape(k, 4)
    ref = O.engine_randn(7, o, 4 * k).reshape(k, 4)
    assert np.abs(got - ref).max() <= NOISE_BOUND
    for row in (0, 15, 16, 999):                        # row 16 is the first counter past 2^32
        assert np.abs(got[row] - O.engine_randn(7, o + row, 4)).max() <= NOISE_BOUND
    for perm in ([1, 0, 3, 2], [2, 3, 0, 1], [0, 2, 1, 3], [3, 0, 1, 2]):     # sin <-> cos, the pairs swapped, ...
        assert np.abs(got - ref[:, perm]).max() > 100 * NOISE_BOUND, perm
    assert np.abs(got + ref).max() > 100 * NOISE_BOUND                        # a sign error
    assert np.abs(got[1:] - ref[:-1]).max() > 100 * NOISE_BOUND               # a counter off by one


def test_randn_edge_uniforms():
    """u1 == 1.0 (both normals exactly +-0), u1 one step below it (the hardware log must not come out positive: sqrt would give
    NaN), the smallest u1 (|z| = 5.887), u2 at the four quadrant boundaries of the hardware sine and cosine."""
    worst = 0.0
    for counter, lane, word in NE.ALL_EDGES:
        got = host(randn_dev(NE.EDGE_SEED, counter, 4))
        ref = O.engine_randn(NE.EDGE_SEED, counter, 4)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err)
        log_line(f"[parity] fd_randn edge counter {counter} (lane {lane} = {word:#010x}): {got.tolist()} max |err| = {err:.3e}")
        assert np.isfinite(got).all(), (counter, got)
        assert np.abs(got).max() <= Z_MAX and err <= NOISE_BOUND, (counter, got, ref)
    got = host(randn_dev(NE.EDGE_SEED, NE.U1_ONE[0], 4))
    assert got[2] == 0.0 and got[3] == 0.0 and got[0] != 0.0                  # (== holds for either sign of zero)
    got = host(randn_dev(NE.EDGE_SEED, NE.U1_SMALLEST[0], 4))
    assert 5.88 < np.hypot(got[0], got[1]) < Z_MAX
    got = host(randn_dev(NE.EDGE_SEED, NE.U1_BELOW_ONE[0], 4))
    assert 0.0 < np.hypot(got[0], got[1]) < 5e-4
    log_line(f"[parity] fd_randn edges: max |fd_randn - engine_randn| = {worst:.3e} (recorded {NOISE_MEASURED:.3e}, bound {NOISE_BOUND:.3e})")


# ------------------------------------------------------------------------------- C. step, prior, perturb at the edge shapes
# n % 4 in {0, 1, 2, 3}; odd and even group counts (the last thread's second group missing); C < 4 (divisions) and C >= 4 (carries) in
# group_rows; rows that end inside a group; T == 1; n < 4
SHAPES = [(1, 1, 1), (1, 1, 3), (3, 5, 1), (2, 7, 3), (5, 37, 3), (3, 5, 4), (3, 7, 5), (2, 3, 9), (9, 1, 5), (4, 100, 12)]
PERTURB_SHAPES = SHAPES + [(7, 1, 1), (5, 1, 3), (3, 2, 1)]          # T C < 4: a group spans up to four samples
_id = lambda s: "x".join(map(str, s))


def _inputs(tag, shape):
    return tuple(W.randn(f"np_{tag}_{k}", shape, 11) for k in ("x", "s", "z"))


def _device_noise(shape):
    n = int(np.prod(shape))
    return randn_dev(SEED, OFFSET, n), O.engine_randn(SEED, OFFSET, n).reshape(shape)


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_sde_step_edges(shape, kind, monkeypatch):
    T = shape[1]
    x, sc, z = _inputs("st", shape)
    osde = oracle_sde(kind, SDES[kind][1], True, T)
    G, xd, sd, zd = dev(osde.G), dev(x), dev(sc), dev(z)
    dt = float(O.timesteps(1000)[1])
    zdev, zeng = _device_noise(shape)
    for t in (0.37, 1e-5, 1.0):
        ref = O.sde_step(osde, sc, t, x, z, dt)
        ref_eng = O.sde_step(osde, sc, t, x, zeng, dt)
        coef = _noise_coef(lambda v: O.sde_step(osde, 0 * sc, t, 0 * x, np.full(shape, v), dt))
        outs = {}
        for nt in ("0", "1"):
            monkeypatch.setenv("FDIFF_SDE_NT", nt)                       # read per call: k_sde_step<false> / <true>
            inj = step_dev(kind, G, xd, sd, zd, t, dt, shape)
            np.testing.assert_allclose(host(inj), _flat(ref), rtol=2e-6, atol=2e-6)
            on = step_dev(kind, G, xd, sd, None, t, dt, shape, SEED, OFFSET)
            assert torch.equal(on, step_dev(kind, G, xd, sd, zdev, t, dt, shape)), (nt, t)
            outs[nt] = (inj, on)
        assert torch.equal(outs["0"][0], outs["1"][0]) and torch.equal(outs["0"][1], outs["1"][1]), t
        ok, msg = _within(f"fd_sde_step {kind} {_id(shape)} t={t:g} device noise vs engine_randn", host(outs["1"][1]), ref_eng,
                          2e-6 + 2e-6 * np.abs(_flat(ref_eng)) + coef * NOISE_BOUND)
        assert ok, msg
    report_err(f"fd_sde_step {kind} {_id(shape)} injected noise, t=1", host(outs["1"][0]), _flat(ref))


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_prior_edges(shape, kind):
    T = shape[1]
    _, _, z = _inputs("pr", shape)
    osde = oracle_sde(kind, SDES[kind][1], True, T)
    G = dev(osde.G)
    inj = prior_dev(kind, G, dev(z), shape)
    np.testing.assert_allclose(host(inj), _flat(O.prior_sampling(osde, z)), rtol=1e-6, atol=1e-7)
    zdev, zeng = _device_noise(shape)
    on = prior_dev(kind, G, None, shape, SEED, OFFSET)
    assert torch.equal(on, prior_dev(kind, G, zdev, shape))
    ref_eng = _flat(O.prior_sampling(osde, zeng))
    coef = _noise_coef(lambda v: O.prior_sampling(osde, np.full(shape, v)))
    ok, msg = _within(f"fd_prior_sample {kind} {_id(shape)} device noise vs engine_randn", host(on), ref_eng,
                      1e-7 + 1e-6 * np.abs(ref_eng) + coef * NOISE_BOUND)
    assert ok, msg


def _check_perturb(tag, got, want):
    (xn, tg, sd), (oxn, otg, ostd) = got, want
    np.testing.assert_allclose(host(xn), _flat(oxn), rtol=5e-6, atol=5e-6, err_msg=tag)
    np.testing.assert_allclose(host(sd), _flat(ostd), rtol=1e-5, err_msg=tag)
    np.testing.assert_allclose(host(tg), _flat(otg), rtol=2e-5, atol=1e-5, err_msg=tag)


@pytest.mark.parametrize("kind", ["vp", "ve"])
@pytest.mark.parametrize("shape", PERTURB_SHAPES, ids=_id)
def test_perturb_edges(shape, kind):
    B, T, _ = shape
    x, _, z = _inputs("pt", shape)
    t = W.uniform("np_pt_t", (B,), 11, 0.05, 1.0)
    osde = oracle_sde(kind, SDES[kind][1], True, T)
    G, xd, td = dev(osde.G), dev(x), dev(t)
    inj = perturb_dev(kind, G, xd, td, dev(z), shape)
    _check_perturb("injected", inj, O.perturb(osde, x, t, z))
    bare = perturb_dev(kind, G, xd, td, dev(z), shape, aux=False)            # target = std_out = NULL
    assert torch.equal(bare[0], inj[0])
    # on-device noise: the injected path fed with fd_randn's normals, bit for bit; those against the oracle fed with the same float32
    # normals (target = z / std amplifies a difference in z by 1 / std, up to 150 here), and x_noisy against the restated normals
    zdev, zeng = _device_noise(shape)
    on = perturb_dev(kind, G, xd, td, None, shape, SEED, OFFSET)
    via = perturb_dev(kind, G, xd, td, zdev, shape)
    for a, b, name in zip(on, via, ("x_noisy", "target", "std")):
        assert torch.equal(a, b), name
    _check_perturb("device noise", on, O.perturb(osde, x, t, host(zdev).reshape(shape)))
    assert torch.equal(perturb_dev(kind, G, xd, td, None, shape, SEED, OFFSET, aux=False)[0], on[0])
    oxn, _, ostd = O.perturb(osde, x, t, zeng)
    coef = np.repeat(_flat(ostd), shape[2])
    ok, msg = _within(f"fd_perturb {kind} {_id(shape)} device noise vs engine_randn", host(on[0]), oxn,
                      5e-6 + 5e-6 * np.abs(_flat(oxn)) + coef * NOISE_BOUND)
    assert ok, msg
    report_err(f"fd_perturb {kind} {_id(shape)} x_noisy, injected noise", host(inj[0]), _flat(O.perturb(osde, x, t, z)[0]))


# ------------------------------------------------------------------------------- D. grid-stride sweeps, in a fresh child process
def _factor_btc(candidates):
    """(B, T, C) with B T C among the candidates: C >= 4 and several series of a T that is no power of two where the number allows,
    else one series, else (1, n, 1)."""
    for n in candidates:
        for Cn in (5, 6, 7, 9, 11, 12, 10, 4, 8):
            if n % Cn == 0:
                rows = n // Cn
                for T in range(3, 1000):
                    if rows % T == 0 and T & (T - 1):
                        return rows // T, T, Cn
    for n in candidates:
        for Cn in (5, 6, 7, 9, 11, 12, 10, 4, 8):
            if n % Cn == 0:
                return 1, n // Cn, Cn
    return 1, candidates[0], 1


def _sweep_child_main():
    """Runs in the child of test_grid_stride_sweeps_in_a_fresh_process (FDIFF_SDE_GRIDMULT=1: the grid is capped at S = 256 num_cu
    threads) and exits non-zero when any comparison fails; the tolerances are those of part C."""
    assert os.environ.get("FDIFF_SDE_GRIDMULT") == "1"
    S = 256 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(5)
    fails = []

    def check(ok_msg):
        if not ok_msg[0]:
            fails.append(ok_msg[1])
            print("FAIL " + ok_msg[1])

    def same(tag, a, b):
        if not torch.equal(a, b):
            fails.append(f"{tag}: not bit-identical")
            print(f"FAIL {tag}: not bit-identical ({int((a != b).sum())} of {a.numel()} elements differ)")

    def draw(shape):
        return rng.standard_normal(shape, dtype=np.float32)

    dt = float(O.timesteps(1000)[1])
    # fd_sde_step (two groups per thread: sweep k covers groups [2 k S, 2 k S + 2 S)): the second sweep with no second group, n % 4 == 3;
    # then the third sweep begun, both instantiations
    # then the third sweep begun, both instantiations; then many series of (37, 5) (those two group counts leave few factorisations:
    # one long series on 256 CUs), 2.3 sweeps of one group per thread
    T, Cn = 37, 5
    many = ((23 * S // 10) * 4 // (T * Cn) + 1, T, Cn)
    ga, gb = 2 * S + S // 2 + 1, 4 * S + 7
    for kind, t, ng, shape in (("vp", 0.37, ga, _factor_btc([4 * ga - 1])),
                               ("ve", 1.0, gb, _factor_btc([4 * gb - 1, 4 * gb - 2, 4 * gb - 3, 4 * gb])),
                               ("vp", 1e-5, (int(np.prod(many)) + 3) // 4, many)):
        n = int(np.prod(shape))
        assert (n + 3) // 4 == ng
        x, sc, z = draw(shape), draw(shape), draw(shape)
        osde = oracle_sde(kind, SDES[kind][1], True, shape[1])
        G, xd, sd, zd = dev(osde.G), dev(x), dev(sc), dev(z)
        ref = _flat(O.sde_step(osde, sc, t, x, z, dt))
        zdev, zeng = _device_noise(shape)
        ref_eng = _flat(O.sde_step(osde, sc, t, x, zeng, dt))
        coef = _noise_coef(lambda v: O.sde_step(osde, 0 * sc, t, 0 * x, np.full(shape, v), dt))
        outs = {}
        for nt in ("0", "1"):
            os.environ["FDIFF_SDE_NT"] = nt
            tag = f"sweeps fd_sde_step {kind} {_id(shape)} ({ng} groups, n % 4 = {n % 4}) NT={nt}"
            inj = step_dev(kind, G, xd, sd, zd, t, dt, shape)
            check(_within(tag + " injected", host(inj), ref, 2e-6 + 2e-6 * np.abs(ref)))
            on = step_dev(kind, G, xd, sd, None, t, dt, shape, SEED, OFFSET)
            same(tag + " device noise vs injected fd_randn", on, step_dev(kind, G, xd, sd, zdev, t, dt, shape))
            check(_within(tag + " device noise vs engine_randn", host(on), ref_eng, 2e-6 + 2e-6 * np.abs(ref_eng) + coef * NOISE_BOUND))
            outs[nt] = (inj, on)
        same(f"sweeps fd_sde_step {kind} NT 0 vs 1, injected", outs["0"][0], outs["1"][0])
        same(f"sweeps fd_sde_step {kind} NT 0 vs 1, device noise", outs["0"][1], outs["1"][1])
        del os.environ["FDIFF_SDE_NT"]
    # one group per thread: about 2.3 sweeps of fd_randn, fd_prior_sample, fd_perturb
    shape = many
    B = shape[0]
    n = B * T * Cn
    zdev, zeng = _device_noise(shape)
    check(_within(f"sweeps fd_randn n={n}", host(zdev), zeng, NOISE_BOUND))
    x, z = draw(shape), draw(shape)
    tv = rng.uniform(0.05, 1.0, B).astype(np.float32)
    for kind in ("vp", "ve"):
        osde = oracle_sde(kind, SDES[kind][1], True, T)
        G, xd, zd, td = dev(osde.G), dev(x), dev(z), dev(tv)
        tag = f"sweeps fd_prior_sample {kind} {_id(shape)}"
        ref = _flat(O.prior_sampling(osde, z))
        check(_within(tag + " injected", host(prior_dev(kind, G, zd, shape)), ref, 1e-7 + 1e-6 * np.abs(ref)))
        on = prior_dev(kind, G, None, shape, SEED, OFFSET)
        same(tag + " device noise vs injected fd_randn", on, prior_dev(kind, G, zdev, shape))
        ref_eng = _flat(O.prior_sampling(osde, zeng))
        coef = _noise_coef(lambda v: O.prior_sampling(osde, np.full(shape, v)))
        check(_within(tag + " device noise vs engine_randn", host(on), ref_eng, 1e-7 + 1e-6 * np.abs(ref_eng) + coef * NOISE_BOUND))
        tag = f"sweeps fd_perturb {kind} {_id(shape)}"
        for name, zz, kw in (("injected", z, dict(z=zd)), ("device noise", host(zdev).reshape(shape), dict(z=None, seed=SEED, offset=OFFSET))):
            xn, tg, sdv = perturb_dev(kind, G, xd, td, shape=shape, **kw)
            oxn, otg, ostd = (_flat(a) for a in O.perturb(osde, x, tv, zz))
            check(_within(f"{tag} {name} x_noisy", host(xn), oxn, 5e-6 + 5e-6 * np.abs(oxn)))
            check(_within(f"{tag} {name} std", host(sdv), ostd, 1e-5 * np.abs(ostd)))
            check(_within(f"{tag} {name} target", host(tg), otg, 1e-5 + 2e-5 * np.abs(otg)))
            if kw["z"] is None:
                via = perturb_dev(kind, G, xd, td, zdev, shape)
                for a, b, nm in zip((xn, tg, sdv), via, ("x_noisy", "target", "std")):
                    same(f"{tag} device noise vs injected fd_randn, {nm}", a, b)
                oxe, _, ose = O.perturb(osde, x, tv, zeng)
                check(_within(f"{tag} device noise vs engine_randn, x_noisy", host(xn), oxe,
                              5e-6 + 5e-6 * np.abs(_flat(oxe)) + np.repeat(_flat(ose), Cn) * NOISE_BOUND))
    print(f"sweeps: {len(fails)} failures")
    sys.exit(1 if fails else 0)


def test_grid_stride_sweeps_in_a_fresh_process():
    """FDIFF_SDE_GRIDMULT is read once per process, so the capped grid needs a process of its own: ONE child, started fresh, no
    retry.  With the cap at one block per CU every kernel of part C runs its grid-stride loop two to three times at 0.6 - 1.0 M
    elements (on 256 CUs); the child compares each with the float64 oracle and exits non-zero on a mismatch."""
    env = dict(os.environ, FDIFF_SDE_GRIDMULT="1", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("FDIFF_SDE_NT", None)
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_noise_parity as m; m._sweep_child_main()"], cwd=str(ROOT), env=env,
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
    assert "sweeps: 0 failures" in r.stdout


# ---------------------------------------------------------------------------------------------- E. Langevin step, DSM loss
@pytest.mark.parametrize("shape,on_device", [((3, 100, 12), True), ((2, 300, 4), True), ((2, 1, 4), True), ((5, 37, 3), False)],
                         ids=["3x100x12", "2x300x4", "2x1x4", "5x37x3-injected"])
def test_langevin_step_edges(shape, on_device):
    """300 groups of four per series run the 256-thread strided loop twice; on-device noise is counter offset + (base >> 2) + gi."""
    T = shape[1]
    x, sc, z = _inputs("lv", shape)
    sc = (sc * np.float32(3.0)).astype(np.float32)
    osde = oracle_sde("vp", (0.1, 20.0), True, T)
    G, xd, sd = dev(osde.G), dev(x), dev(sc)
    ref = _flat(O.langevin_step(osde, sc, x, z, snr=0.16, alpha=0.93))
    out = langevin_dev(G, xd, sd, dev(z), shape)
    report_err(f"fd_langevin_step {_id(shape)} injected noise", host(out), ref)
    np.testing.assert_allclose(host(out), ref, atol=2e-6 * max(1.0, np.abs(ref).max()), rtol=0)
    if on_device:
        n = int(np.prod(shape))
        zdev = randn_dev(SEED, OFFSET, n)
        on = langevin_dev(G, xd, sd, None, shape, SEED, OFFSET)
        assert torch.equal(on, langevin_dev(G, xd, sd, zdev, shape))
        ref_dev = _flat(O.langevin_step(osde, sc, x, host(zdev).reshape(shape), snr=0.16, alpha=0.93))
        np.testing.assert_allclose(host(on), ref_dev, atol=2e-6 * max(1.0, np.abs(ref_dev).max()), rtol=0)


@pytest.mark.parametrize("lw", [False, True])
@pytest.mark.parametrize("shape", [(3, 300, 2), (1, 257, 1)], ids=_id)
def test_dsm_loss_and_gradient_edges(shape, lw):
    """T > 256 (the weight loop strides) and T C > 256 (the element loop strides); dscore element by element against the analytic
    float64 gradient 2 coef (score + target) / (B T C), coef = std^2 (likelihood weighting) or w_b = 1 / sum_k std^-2."""
    _C, L, h = _eng()
    B, T, Cn = shape
    n = B * T * Cn
    score, target, _ = _inputs("ds", shape)
    std = W.uniform("np_ds_std", (B, T), 11, 0.05, 1.5)
    sd, td, vd = dev(score), dev(target), dev(std)
    res = []
    for _ in range(2):
        loss, dscore = _guarded(1), _guarded(n)
        _C.check(L.fd_dsm_loss(h, sd.data_ptr(), td.data_ptr(), vd.data_ptr(), int(lw), loss.data_ptr(), dscore.data_ptr(), B, T, Cn,
                               None), h)
        res.append((_take(loss, 1), _take(dscore, n)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    s64, t64, v64 = (np.asarray(a, dtype=np.float64) for a in (score, target, std))
    want = O.dsm_loss(s64, t64, v64, lw)
    log_line(f"[parity] fd_dsm_loss {_id(shape)} lw={int(lw)}: loss {res[0][0].item():.8g} vs {want:.8g}, rel err "
             f"{abs(res[0][0].item() - want) / abs(want):.3e}")
    np.testing.assert_allclose(res[0][0].item(), want, rtol=2e-6)
    coef = v64[:, :, None] ** 2 if lw else (1.0 / np.sum(1.0 / v64 ** 2, axis=1))[:, None, None]
    grad = 2.0 * coef * (s64 + t64) / n
    report_err(f"fd_dsm_loss {_id(shape)} lw={int(lw)} dscore", host(res[0][1]), _flat(grad))
    np.testing.assert_allclose(host(res[0][1]), _flat(grad), rtol=2e-6, atol=1e-9)
