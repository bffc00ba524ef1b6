"""GPU: entropic optimal transport (fd_softmin_pairs, fd_sinkhorn_potentials: csrc/fd_sinkhorn.hip; utils/sinkhorn.py;
sampling/metrics.py SinkhornDivergence) against the float64 brute force of tests/sinkhorn_ref.py.

The bound.  The soft-min is 1-Lipschitz in its exponents h_j - d2_ij under the sup norm, so with u = 2^-24, delta_ij the expansion
error of the centred f32 distances and gt the tiles of a group, one pass obeys
  |out~_i - out_i| <= max_j (delta_ij + u |h_j|) + 6 u max_j |h_j - d2_ij| + eps (67 gt + 9) u
(sinkhorn_ref.error_bounds: derived, not tuned).  A potential after L passes is held to the sum of the L per-pass bounds (both
updates are non-expansive), the divergence to the sum of its four potentials' bounds.  Those worst cases are loose, so every
output is also held to 8 times the deviation of the float32 numpy restatement of the same arithmetic from the float64 reference,
plus a floor of 2 u max |h_j - d2_ij| per pass: the restatement rounds the exponent's product and sum separately and takes numpy's
exp2, the engine rounds one fma and takes v_exp_f32, and each of the two differences is one rounding of the exponent.

Measured on an MI355X (the tables per case are in DESIGN.md 3.28).  One pass: the largest error is 5.1e-4 to 6.9e-2 of the
worst-case bound and 0.69 to 2.58 of the restatement's own deviation (exactly 1.00 in half of the cases: at a small eps one term
dominates and both round the same distance), except (1, 40, 9) at reg 0.01, a single row: 2.0e-6 against 2.9e-7, a third of the
allowed 8 x + 6.2e-6.  After 12 iterations (24 passes) the potentials are within 4.8e-5 to 4.7e-3 of the summed bound and 0.69 to
3.69 of the restatement's deviation; the divergence end to end is within 2.5e-5 to 4.6e-5 of its bound.  At the ragged shapes a
row at the common mean with h = 0 -- a leaked padded row -- would move every result at reg 0.01 by 6e3 to 8e5 times the bound."""
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

from tests import mmd_ref as W
from tests import sinkhorn_ref as R

from .gpu_util import dev, log_line

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
U = R.U
REGS = (1.0, 0.05, 0.01)
STEPS = (4.0, 1.0, 0.25, 0.0625) + (0.05,) * 8              # 12 iterations under a descending schedule, units of eps_base

# (n, m, d, kind)
SHAPES = {
    "5+7x3": (5, 7, 3, "waves"),                             # below one tile
    "128+128x16": (128, 128, 16, "waves"),                   # exact tiles
    "129+127x17": (129, 127, 17, "waves"),                   # ragged everywhere
    "300+200x187": (300, 200, 187, "waves"),                 # several tiles both ways
    "64+700x1200": (64, 700, 1200, "waves"),                 # unbalanced; six groups
    "1+40x9": (1, 40, 9, "waves"),                           # the ends of the ranges
    "2100+2000x6": (2100, 2000, 6, "waves"),                 # 16 and 17 groups
    "40+4100x5": (40, 4100, 5, "waves"),                     # 33 tiles: groups of two tiles, the fp32 chain crosses a tile
    "200+200x62_shifted": (200, 200, 62, "shifted"),         # the centring: every row + 3
}
RAGGED = [name for name, s in SHAPES.items() if s[1] % 128]
SPLIT_SHAPES = ["300+200x187", "64+700x1200", "2100+2000x6", "40+4100x5"]
ITERATION_SHAPES = [name for name in SHAPES if name != "40+4100x5"]
WEIGHTED_SHAPES = [name for name in ITERATION_SHAPES if name != "2100+2000x6"]        # (the largest runs with uniform weights only)


def softmin_raw(x, y, h, eps, splits=0, sentinel=-7.0):
    """fd_softmin_pairs through the C ABI on device tensors: out (n) as numpy float64, pre-filled with a sentinel."""
    from fourierdiffusion_amd import _C
    (n, d), m = x.shape, y.shape[0]
    hd, L = _C.ctx(x.device), _C.lib()
    need = C.c_size_t(0)
    _C.check(L.fd_softmin_pairs_workspace_bytes(hd, n, m, d, 1 if x is y else 0, splits, C.byref(need)), hd)
    work = torch.empty((need.value,), dtype=torch.uint8, device=x.device)
    out = torch.full((n,), sentinel, dtype=torch.float64, device=x.device)
    _C.check(L.fd_softmin_pairs(hd, x.data_ptr(), n, y.data_ptr(), m, d, h.data_ptr(), float(eps), splits, out.data_ptr(),
                                work.data_ptr(), need.value, _C.stream_of(x)), hd)
    return out.cpu().numpy()


def potentials_raw(x, y, sched, a=None, b=None, symmetric=False, absolute=False, sentinel=-7.0):
    """fd_sinkhorn_potentials through the C ABI: (f, g, eps_base) as numpy float64."""
    from fourierdiffusion_amd import _C
    (n, d), m = x.shape, y.shape[0]
    hd, L = _C.ctx(x.device), _C.lib()
    need = C.c_size_t(0)
    _C.check(L.fd_sinkhorn_potentials_workspace_bytes(hd, n, m, d, 1 if symmetric else 0, C.byref(need)), hd)
    work = torch.empty((need.value,), dtype=torch.uint8, device=x.device)
    f = torch.full((n,), sentinel, dtype=torch.float64, device=x.device)
    g = torch.full((m,), sentinel, dtype=torch.float64, device=x.device)
    base = torch.full((1,), sentinel, dtype=torch.float64, device=x.device)
    at = None if a is None else torch.from_numpy(a).cuda()
    bt = None if b is None else torch.from_numpy(b).cuda()
    ce = (C.c_double * len(sched))(*sched)
    _C.check(L.fd_sinkhorn_potentials(hd, x.data_ptr(), n, y.data_ptr(), m, d, 1 if symmetric else 0, _C.ptr(at), _C.ptr(bt), ce,
                                      len(sched), 1 if absolute else 0, f.data_ptr(), g.data_ptr(), base.data_ptr(), work.data_ptr(),
                                      need.value, _C.stream_of(x)), hd)
    return f.cpu().numpy(), g.cpu().numpy(), float(base.cpu().numpy()[0])


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and the float64 distances of one shape, computed once and shared (nothing below writes to them).  h is random about
    -3 eps_base: the real exponents then lie below that of a row at the mean with h = 0, which is what a leaked padded row would be."""
    n, m, d, kind = SHAPES[name]
    rng = np.random.default_rng(len(name) * 1000 + n + m + d)
    x, y = W.waves(rng, n, d), W.waves(rng, m, d)
    if kind == "shifted":
        x, y = x + 3.0, 1.2 * y + 3.0
    x, y = x.astype(np.float32), y.astype(np.float32)
    base = R.eps_base_closed(x, y)
    h = base * (-3.0 + 0.25 * rng.standard_normal(m))
    wa, wb = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, m)
    return dict(x=x, y=y, n=n, m=m, base=base, h=h, D=R.dist2(x, y, chunk=16), a=wa / wa.sum(), b=wb / wb.sum())


@functools.lru_cache(maxsize=None)
def softmin_case(name, reg):
    """The float64 soft-min of one shape at eps = reg eps_base, its bound and the restatement's deviation."""
    c = case(name)
    eps = reg * c["base"]
    ref = R.softmin(c["D"], c["h"], eps)
    xc, yc, xn, yn = R.centred_f32(c["x"], c["y"])
    dev32 = float(np.abs(R.softmin_f32(xc, yc, xn, yn, c["h"], eps) - ref).max())
    floor = 2.0 * U * float(np.abs(c["h"][None, :] - c["D"]).max())
    return dict(eps=eps, ref=ref, bound=R.error_bounds(c["x"], c["y"], c["h"], eps, c["D"]), restate_dev=dev32, floor=floor)


@functools.lru_cache(maxsize=None)
def iteration_case(name, weighted):
    """The float64 potentials of one shape after STEPS, alternating and symmetric (on x), their bounds and the restatement's
    deviations."""
    c = case(name)
    a, b = (c["a"], c["b"]) if weighted else (R.uniform(c["n"]), R.uniform(c["m"]))
    sched = np.asarray(STEPS) * c["base"]
    f, g, bf, bg = R.potentials_with_bounds(c["x"], c["y"], a, b, sched, c["D"])
    f32, g32 = R.potentials_f32(c["x"], c["y"], a, b, sched)
    Dxx = R.dist2(c["x"], c["x"], chunk=16)
    base_x = R.eps_base_closed(c["x"])
    sched_x = np.asarray(STEPS) * base_x
    p, bp = R.symmetric_with_bound(c["x"], a, sched_x, Dxx)
    p32 = R.potentials_symmetric_f32(c["x"], a, sched_x)
    scale = float(max(np.abs(g[None, :] - c["D"]).max(), np.abs(f[:, None] - c["D"]).max()))
    return dict(a=a, b=b, f=f, g=g, bf=bf, bg=bg, p=p, bp=bp, base_x=base_x,
                dev_f=float(np.abs(f32 - f).max()), dev_g=float(np.abs(g32 - g).max()), dev_p=float(np.abs(p32 - p).max()),
                floor=2.0 * U * scale * 2 * len(STEPS), floor_p=2.0 * U * float(np.abs(p[None, :] - Dxx).max()) * len(STEPS))


# ---------------------------------------------------------------------------------------------- one pass
@pytest.mark.parametrize("reg", REGS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_softmin_pairs_against_float64(name, reg):
    c, s = case(name), softmin_case(name, reg)
    if reg == 0.01 and name in RAGGED:
        # the case cannot hide a leaked padded row: one more row at the common mean with h = 0 moves every result far past the bound
        mu = np.concatenate([c["x"], c["y"]]).astype(np.float64).mean(axis=0)
        leak = ((c["x"].astype(np.float64) - mu) ** 2).sum(axis=1)
        moved = R.softmin(np.concatenate([c["D"], leak[:, None]], axis=1), np.append(c["h"], 0.0), s["eps"])
        assert (np.abs(moved - s["ref"]) > 10.0 * s["bound"]).all()
    got = softmin_raw(dev(c["x"]), dev(c["y"]), torch.from_numpy(c["h"]).cuda(), s["eps"])
    assert np.isfinite(got).all() and (got != -7.0).all()                       # the sentinel is overwritten everywhere
    err = np.abs(got - s["ref"])
    log_line(f"[sinkhorn] {name} reg {reg}: soft-min error / worst-case bound max {(err / s['bound']).max():.3e}; error {err.max():.3e}, "
             f"restatement deviation {s['restate_dev']:.3e}, ratio {err.max() / max(s['restate_dev'], 1e-300):.3f}, floor {s['floor']:.3e}")
    assert (err <= s["bound"]).all(), (err / s["bound"]).max()
    assert err.max() <= 8.0 * s["restate_dev"] + s["floor"]


@pytest.mark.parametrize("name", SPLIT_SHAPES)
def test_results_are_bit_identical_for_every_split_and_run(name):
    c, s = case(name), softmin_case(name, 0.05)
    x, y, h = dev(c["x"]), dev(c["y"]), torch.from_numpy(c["h"]).cuda()
    first = softmin_raw(x, y, h, s["eps"], splits=1)
    for splits in (1, 2, 3, 64, 0):
        np.testing.assert_array_equal(softmin_raw(x, y, h, s["eps"], splits=splits), first, err_msg=f"splits={splits}")
    sched = np.asarray(STEPS[:6])
    one = potentials_raw(x, y, sched)
    for a, b in zip(one, potentials_raw(x, y, sched)):
        np.testing.assert_array_equal(a, b)


def test_one_set_against_itself_and_equal_rows():
    c, s = case("129+127x17"), softmin_case("129+127x17", 0.05)
    x = dev(c["x"])
    h = torch.from_numpy(c["h"][:1].repeat(129)).cuda()
    ref = R.softmin(R.dist2(c["x"], c["x"]), c["h"][:1].repeat(129), s["eps"])
    bound = R.error_bounds(c["x"], c["x"], c["h"][:1].repeat(129), s["eps"], same=True)
    assert (np.abs(softmin_raw(x, x, h, s["eps"]) - ref) <= bound).all()                    # the same array: centred once
    assert (np.abs(softmin_raw(x, x.clone(), h, s["eps"]) - ref) <= bound).all()
    # every row the same: d2 = 0, the soft-min is h - eps log m exactly up to the sum's rounding; eps_base falls back to 1
    ones = dev(np.repeat(c["x"][:1], 50, axis=0))
    got = softmin_raw(ones, ones, torch.zeros(50, dtype=torch.float64, device="cuda"), 0.5)
    assert np.abs(got + 0.5 * np.log(50.0)).max() <= 0.5 * (67 + 9) * U
    f, g, base = potentials_raw(ones, ones, [1.0, 0.5], symmetric=True)
    assert base == 1.0 and np.isfinite(f).all() and np.array_equal(f, g)


# ---------------------------------------------------------------------------------------------- the iteration
def check_potential(tag, got, ref, bound, restate_dev, floor):
    err = float(np.abs(got - ref).max())
    log_line(f"[sinkhorn] {tag}: error / {len(STEPS)}-step bound {err / bound:.3e}; error {err:.3e}, restatement deviation "
             f"{restate_dev:.3e}, ratio {err / max(restate_dev, 1e-300):.3f}, floor {floor:.3e}")
    assert np.isfinite(got).all() and err <= bound
    assert err <= 8.0 * restate_dev + floor


@pytest.mark.parametrize("name", ITERATION_SHAPES)
def test_potentials_against_float64_uniform(name):
    _check_iteration(name, False)


@pytest.mark.parametrize("name", WEIGHTED_SHAPES)
def test_potentials_against_float64_weighted(name):
    _check_iteration(name, True)


def _check_iteration(name, weighted):
    c, it = case(name), iteration_case(name, weighted)
    x, y = dev(c["x"]), dev(c["y"])
    a, b = (it["a"], it["b"]) if weighted else (None, None)
    f, g, base = potentials_raw(x, y, STEPS, a, b)
    assert abs(base - c["base"]) <= 1e-12 * c["base"]
    tag = f"{name} {'weighted' if weighted else 'uniform'}"
    check_potential(tag + " f", f, it["f"], it["bf"], it["dev_f"], it["floor"])
    check_potential(tag + " g", g, it["g"], it["bg"], it["dev_g"], it["floor"])
    p, q, base_x = potentials_raw(x, x, STEPS, a, None, symmetric=True)
    assert abs(base_x - it["base_x"]) <= 1e-12 * it["base_x"] and np.array_equal(p, q)
    check_potential(tag + " p", p, it["p"], it["bp"], it["dev_p"], it["floor_p"])
    if not weighted:
        # an absolute schedule is the same iteration
        fa, ga, _ = potentials_raw(x, y, np.asarray(STEPS) * base, absolute=True)
        assert np.abs(fa - f).max() <= 1e-12 * c["base"] and np.abs(ga - g).max() <= 1e-12 * c["base"]


# ---------------------------------------------------------------------------------------------- Python surface
@pytest.mark.parametrize("name,weighted", [("129+127x17", False), ("300+200x187", True), ("200+200x62_shifted", False)])
def test_divergence_end_to_end(name, weighted):
    from fourierdiffusion_amd.utils.sinkhorn import sinkhorn_divergence, sinkhorn_potentials, softmin_pairs
    c = case(name)
    a, b = (c["a"], c["b"]) if weighted else (None, None)
    ua, ub = (c["a"], c["b"]) if weighted else (R.uniform(c["n"]), R.uniform(c["m"]))
    sched = np.asarray(STEPS) * c["base"]
    eps = sched[-1]
    ref = R.divergence(c["x"], c["y"], sched, a, b)
    _, _, bf, bg = R.potentials_with_bounds(c["x"], c["y"], ua, ub, sched, c["D"])
    _, bpx = R.symmetric_with_bound(c["x"], ua, sched)
    _, bpy = R.symmetric_with_bound(c["y"], ub, sched)
    res = sinkhorn_divergence(c["x"], c["y"], schedule=STEPS, weights_x=a, weights_y=b)
    bound = bf + bg + bpx + bpy
    log_line(f"[sinkhorn] {name}: divergence {res.divergence:.6e} (float64 {ref['divergence']:.6e}), error / bound "
             f"{abs(res.divergence - ref['divergence']) / bound:.3e}, marginal error {res.marginal_error:.3e} ({ref['marginal_error']:.3e})")
    assert res.eps == pytest.approx(eps, rel=1e-12)
    assert abs(res.divergence - ref["divergence"]) <= bound and res.divergence > 0 and res.w2 == np.sqrt(res.divergence)
    assert abs(res.ot_xy - ref["ot_xy"]) <= bf + bg
    assert res.cost_x.shape == (c["n"],) and res.cost_y.shape == (c["m"],)
    assert np.abs(res.cost_x - ref["cost_x"]).max() <= bf + bpx and np.abs(res.cost_y - ref["cost_y"]).max() <= bg + bpy
    # the marginal error is a sum of a_i exp(t_i / eps) - 1 with t = f - softmin_Y(g), each t off by at most bf + bg + one more pass
    slack = bf + bg + float(R.error_bounds(c["x"], c["y"], ref["g"] + eps * np.log(ub), eps, c["D"]).max())
    assert abs(res.marginal_error - ref["marginal_error"]) <= (1.0 + ref["marginal_error"]) * np.expm1(slack / eps)
    # one object against itself: one symmetric run, the divergence is exactly 0; a copy runs the alternating iteration
    same = sinkhorn_divergence(c["x"], c["x"], schedule=STEPS, weights_x=a)
    assert same.divergence == 0.0 and same.w2 == 0.0 and not same.cost_x.any() and not same.cost_y.any()
    sched_copy = np.asarray(STEPS) * R.eps_base_closed(c["x"], c["x"])
    copy = sinkhorn_divergence(c["x"], c["x"].copy(), schedule=STEPS, weights_x=a, weights_y=a)
    ref_copy = R.divergence(c["x"], c["x"], sched_copy, a, a)
    _, _, cf, cg = R.potentials_with_bounds(c["x"], c["x"], ua, ua, sched_copy)
    assert abs(copy.divergence - ref_copy["divergence"]) <= cf + cg + 2.0 * R.symmetric_with_bound(c["x"], ua, sched_copy)[1]
    # the pieces are the public functions: float64 device tensors, 3-d samples flattened
    f, g, e = sinkhorn_potentials(torch.from_numpy(c["x"]).reshape(c["n"], -1, 1), c["y"], schedule=STEPS, weights_x=a, weights_y=b)
    assert f.is_cuda and f.dtype == torch.float64 and g.shape == (c["m"],) and e == res.eps
    assert np.abs(f.cpu().numpy() - ref["f"]).max() <= bf
    sm = softmin_pairs(c["x"], c["y"], c["h"], eps, splits=3)
    assert sm.is_cuda and sm.dtype == torch.float64
    np.testing.assert_array_equal(sm.cpu().numpy(), softmin_raw(dev(c["x"]), dev(c["y"]), torch.from_numpy(c["h"]).cuda(), eps))


def test_sinkhorn_metric_in_a_collection():
    from fourierdiffusion_amd.sampling.metrics import MarginalWasserstein, MetricCollection, SinkhornDivergence, SlicedWasserstein
    from fourierdiffusion_amd.utils.sinkhorn import epsilon_schedule
    rng = np.random.default_rng(100)
    train, fresh, shrunk, held = (s * W.waves(rng, k, 48).astype(np.float32) for k, s in ((160, 1.0), (120, 1.0), (120, 0.85), (100, 1.0)))
    shape = (-1, 24, 2)
    default = [partial(SlicedWasserstein, random_seed=42, num_directions=20), partial(MarginalWasserstein, random_seed=42)]
    kwargs = dict(original_samples=torch.from_numpy(train.reshape(shape)), holdout_samples=torch.from_numpy(held.reshape(shape)))
    before = MetricCollection(metrics=default, **kwargs)(torch.from_numpy(shrunk.reshape(shape)))
    mc = MetricCollection(metrics=default + [partial(SinkhornDivergence, random_seed=0)], **kwargs)
    res = mc(torch.from_numpy(shrunk.reshape(shape)))
    assert list(res) == sorted(res)
    new = {f"{view}_sinkhorn_{key}{suffix}" for view in ("time", "freq") for key in ("divergence", "w2", "marginal_error")
           for suffix in ("", "_holdout", "_self")}
    assert set(res) - set(before) == new and set(before) <= set(res)
    assert all(res[key] == before[key] for key in before)
    # the time view is the divergence of the flat rows: against float64 under the default schedule
    for other, key in ((train, ""), (held, "_holdout")):
        base = R.eps_base_closed(shrunk, other)
        sched = epsilon_schedule(0.05) * base
        ref = R.divergence(shrunk, other, sched)
        ua, ub = R.uniform(len(shrunk)), R.uniform(len(other))
        _, _, bf, bg = R.potentials_with_bounds(shrunk, other, ua, ub, sched)
        bound = bf + bg + R.symmetric_with_bound(shrunk, ua, sched)[1] + R.symmetric_with_bound(other, ub, sched)[1]
        assert abs(res["time_sinkhorn_divergence" + key] - ref["divergence"]) <= bound
        assert res["time_sinkhorn_w2" + key] == np.sqrt(res["time_sinkhorn_divergence" + key])
        assert 0 <= res["time_sinkhorn_marginal_error" + key] < 1
    # (at 80 to 160 rows of 48 features the sampling noise of the divergence exceeds the effect of the shrunk amplitude: no ordering
    # of the values is asserted)
    for key in new:
        assert np.isfinite(res[key]) and res[key] >= 0
    sub = SinkhornDivergence(torch.from_numpy(train), max_original=50, random_seed=3)
    assert sub.original_samples.shape == (50, 48) and sub(torch.from_numpy(fresh))["sinkhorn_w2"] > 0


def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_sample_with_sinkhorn_metric(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=1", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=sinkrun"], tmp_path)
    _run([str(ROOT / "cmd" / "sample.py"), "model_id=sinkrun", "metrics=sinkhorn", "num_diffusion_steps=5", "num_samples=64",
          "sampler.sample_batch_size=32"], tmp_path)
    res = yaml.safe_load(open(tmp_path / "lightning_logs" / "sinkrun" / "results.yaml"))
    for view in ("time", "freq"):
        for suffix in ("", "_holdout", "_self"):
            assert np.isfinite(res[f"{view}_sinkhorn_divergence{suffix}"]), (view, suffix)
            assert res[f"{view}_sinkhorn_w2{suffix}"] >= 0.0 and 0.0 <= res[f"{view}_sinkhorn_marginal_error{suffix}"] < 1.0, (view, suffix)
    assert res["time_sliced_wasserstein_mean"] >= 0.0 and len(res["time_sliced_wasserstein_all"]) == 1000


# ---------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """The four entry points refuse each bad argument with FD_ERR_ARG and a retrievable message."""
    from fourierdiffusion_amd import _C
    x = torch.arange(72.0, device="cuda").reshape(8, 9)
    y = torch.arange(45.0, device="cuda").reshape(5, 9)
    h = torch.zeros(5, dtype=torch.float64, device="cuda")
    f, g = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda")
    base = torch.zeros(1, dtype=torch.float64, device="cuda")
    hd, L = _C.ctx(x.device), _C.lib()
    need, need_it = C.c_size_t(0), C.c_size_t(0)
    assert L.fd_softmin_pairs_workspace_bytes(hd, 8, 5, 9, 0, 0, C.byref(need)) == 0 and need.value > 0
    assert L.fd_sinkhorn_potentials_workspace_bytes(hd, 8, 5, 9, 0, C.byref(need_it)) == 0 and need_it.value > 0
    work = torch.zeros(max(need.value, need_it.value), dtype=torch.uint8, device="cuda")
    xp, yp, hp, fp, gp, bp, wp = (t.data_ptr() for t in (x, y, h, f, g, base, work))
    eps3 = (C.c_double * 3)(1.0, 0.5, 0.25)

    def soft(x=xp, n=8, y=yp, m=5, d=9, h=hp, eps=1.0, splits=0, out=fp, work=wp, bytes_=need.value):
        return L.fd_softmin_pairs(hd, x, n, y, m, d, h, eps, splits, out, work, bytes_, None)

    def sink(x=xp, n=8, y=yp, m=5, d=9, symmetric=0, eps=eps3, steps=3, f=fp, g=gp, base=bp, work=wp, bytes_=need_it.value):
        return L.fd_sinkhorn_potentials(hd, x, n, y, m, d, symmetric, None, None, eps, steps, 0, f, g, base, work, bytes_, None)

    def bad_eps(v):
        return (C.c_double * 3)(1.0, v, 0.25)

    big = 1 << 30
    cases = [
        (lambda: L.fd_softmin_pairs_workspace_bytes(hd, 8, 5, 9, 0, 0, None), b"null"),
        (lambda: L.fd_softmin_pairs_workspace_bytes(hd, 0, 5, 9, 0, 0, C.byref(need)), b"bad shape"),
        (lambda: L.fd_softmin_pairs_workspace_bytes(hd, 8, 0, 9, 0, 0, C.byref(need)), b"bad shape"),
        (lambda: L.fd_softmin_pairs_workspace_bytes(hd, 8, 5, 0, 0, 0, C.byref(need)), b"bad shape"),
        (lambda: L.fd_softmin_pairs_workspace_bytes(hd, big, 5, 9, 0, 0, C.byref(need)), b"too large"),
        (lambda: L.fd_softmin_pairs_workspace_bytes(hd, 8, big, 9, 0, 0, C.byref(need)), b"too large"),
        (lambda: L.fd_softmin_pairs_workspace_bytes(hd, 8, 5, 9, 0, -1, C.byref(need)), b"splits"),
        (lambda: L.fd_softmin_pairs_workspace_bytes(hd, 8, 5, 9, 1, 0, C.byref(need)), b"same"),
        (lambda: L.fd_sinkhorn_potentials_workspace_bytes(hd, 8, 5, 9, 0, None), b"null"),
        (lambda: L.fd_sinkhorn_potentials_workspace_bytes(hd, 8, -1, 9, 0, C.byref(need)), b"bad shape"),
        (lambda: L.fd_sinkhorn_potentials_workspace_bytes(hd, big, 5, 9, 0, C.byref(need)), b"too large"),
        (lambda: L.fd_sinkhorn_potentials_workspace_bytes(hd, 8, 5, 9, 1, C.byref(need)), b"symmetric"),
        (lambda: soft(x=None), b"null"), (lambda: soft(y=None), b"null"), (lambda: soft(h=None), b"null"),
        (lambda: soft(out=None), b"null"), (lambda: soft(work=None), b"null"),
        (lambda: soft(n=0), b"bad shape"), (lambda: soft(m=0), b"bad shape"), (lambda: soft(d=-3), b"bad shape"),
        (lambda: soft(n=big), b"too large"), (lambda: soft(m=big), b"too large"), (lambda: soft(splits=-2), b"splits"),
        (lambda: soft(eps=0.0), b"eps="), (lambda: soft(eps=-1.0), b"eps="), (lambda: soft(eps=float("nan")), b"eps="),
        (lambda: soft(eps=float("inf")), b"eps="),
        (lambda: soft(bytes_=need.value - 1), b"workspace"), (lambda: soft(bytes_=0), b"workspace"),
        (lambda: sink(x=None), b"null"), (lambda: sink(y=None), b"null"), (lambda: sink(eps=None), b"null"),
        (lambda: sink(f=None), b"null"), (lambda: sink(g=None), b"null"), (lambda: sink(base=None), b"null"),
        (lambda: sink(work=None), b"null"),
        (lambda: sink(n=0), b"bad shape"), (lambda: sink(m=0), b"bad shape"), (lambda: sink(d=0), b"bad shape"),
        (lambda: sink(n=big), b"too large"), (lambda: sink(m=big), b"too large"),
        (lambda: sink(symmetric=1), b"symmetric"), (lambda: sink(y=xp, symmetric=1), b"symmetric"),
        (lambda: sink(steps=0), b"n_steps=0"), (lambda: sink(steps=257), b"n_steps=257"),
        (lambda: sink(eps=bad_eps(0.0)), b"eps 1"), (lambda: sink(eps=bad_eps(-2.0)), b"eps 1"),
        (lambda: sink(eps=bad_eps(float("nan"))), b"eps 1"), (lambda: sink(eps=bad_eps(float("inf"))), b"eps 1"),
        (lambda: sink(bytes_=need_it.value - 1), b"workspace"), (lambda: sink(bytes_=0), b"workspace"),
    ]
    for i, (fn, needle) in enumerate(cases):
        assert fn() == -1, i
        assert needle in L.fd_last_error(hd), (i, L.fd_last_error(hd))
    assert L.fd_softmin_pairs(None, xp, 8, yp, 5, 9, hp, 1.0, 0, fp, wp, need.value, None) == -1            # no context: the code only
    assert L.fd_sinkhorn_potentials_workspace_bytes(None, 8, 5, 9, 0, C.byref(need)) == -1
    # and the arguments they were derived from are accepted
    assert soft() == 0 and sink() == 0 and sink(y=xp, m=8, g=fp, symmetric=1) == 0
    torch.cuda.synchronize()
    assert base.item() > 0 and np.isfinite(f.cpu().numpy()).all() and np.isfinite(g.cpu().numpy()).all()
