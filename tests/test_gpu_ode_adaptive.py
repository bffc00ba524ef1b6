"""GPU: adaptive (RK45) ODE sampling, encoding and decoding (fd_sampler_run_ode_adaptive, csrc/fd_ode_adaptive.hip; an extension not
in the reference): the engine against the float64 restatement of scipy's RK45 in both directions (tests/ode_adaptive_ref.py), its
arithmetic on its own grid for the three backbones, convergence, reproducibility and row independence, row compaction, the
evaluation cap, bf16 at the default shape, classifier-free guidance, and the CLI end to end.  Measured errors are logged by
tests/gpu_util.report_err."""
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from oracle import weights as W
from oracle.make_golden import CFG_DEFAULT
from tests import cfg_ref
from tests import cov_ref
from tests import ode_adaptive_ref as A
from tests import ode_ref as R
from tests.gpu_util import dev, host, log_line, make_model, oracle_sde, report_err
from tests.test_gpu_likelihood import CFG_T8, ROOT, _model, _run

pytestmark = pytest.mark.gpu
CFG_T20 = dict(T=20, C=3, D=8, L=2, H=4)
EPS = 1e-5
VP, VE = ("vp", (0.1, 20.0)), ("ve", (0.01, 5.0))
GOLDEN = Path(__file__).resolve().parent / "golden" / "ode_adaptive_tight.npz"
# the project's bounds against a restatement (tests/test_gpu_rk45_likelihood.py): accepted times, and results of scale max(1, |ref|)
GRID_TOL, RES_TOL = 3e-5, 3e-5


def _sampler(m, bs=8):
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    return DiffusionSampler(m, sample_batch_size=bs)


def _t(a):
    return torch.from_numpy(np.asarray(a)).float()


def _rel(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def _grid_rows(info):
    g = info.grid.numpy()
    return [g[b][~np.isnan(g[b])] for b in range(g.shape[0])]


# ------------------------------------------------------------------------------------------------- 1. against the restatement
# (kind, p), backward?, rtol = atol, the restatement's nfe and rejected attempts per row (computed on the CPU when the fixtures were
# chosen; asserted below, with the distance of every accept / reject decision from its threshold)
FIXTURES = {
    "vp_back_1e-3": (VP, True, 1e-3, [56, 56, 56], [0, 0, 0]),
    "vp_back_1e-5": (VP, True, 1e-5, [152, 152, 164], [1, 1, 1]),
    "ve_back_1e-3": (VE, True, 1e-3, [56, 56, 56], [0, 0, 0]),
    "vp_encode_1e-3": (VP, False, 1e-3, [104, 80, 92], [5, 2, 3]),
    "ve_encode_1e-3": (VE, False, 1e-3, [92, 86, 104], [5, 5, 7]),
}
_CACHE = {}


def _fixture(name):
    """(model, sampler, start (3,T,C) float64 as the engine holds it, restatement rows, grid bound, result bound), computed once."""
    if name in _CACHE:
        return _CACHE[name]
    (kind, p), back, tol, nfe, rej = FIXTURES[name]
    cfg = CFG_T20
    m, sch, sd = make_model(cfg, kind=kind, p=p)
    s = _sampler(m)
    z = W.randn(f"rks_z_{kind}", (3, cfg["T"], cfg["C"]), 0)
    start = host(s.sample_prior(3, noise=dev(z))) if back else host(_t(z))
    osde = oracle_sde(kind, p, True, cfg["T"])
    score = R.model_score(sd, "transformer", cfg["H"])
    t0, t1 = (1.0, EPS) if back else (EPS, 1.0)
    rows, sens_t, sens_y = A.sensitivity(osde, score, start, t0, t1, tol, tol)
    closest = min(abs(en - 1.0) for r in rows for en in r["err_norms"])
    log_line(f"[fixture] rk45 ode {name}: nfe {[r['nfe'] for r in rows]}, rejects {[r['n_reject'] for r in rows]}, closest error "
             f"norm to 1 is {closest:.3e} away; float32 sensitivity: grid {sens_t:.3e}, result {sens_y:.3e} of scale")
    assert [r["nfe"] for r in rows] == nfe and [r["n_reject"] for r in rows] == rej
    assert closest >= 1e-3      # (a borderline accept / reject would make the fixture flaky)
    _CACHE[name] = (m, s, z, start, rows, max(GRID_TOL, 8 * sens_t), max(RES_TOL, 8 * sens_y))
    return _CACHE[name]


def _engine(name, **kw):
    (kind, p), back, tol, _, _ = FIXTURES[name]
    m, s, z, start, rows, _, _ = _fixture(name)
    if back:
        return s.sample_ode_adaptive(3, rtol=tol, atol=tol, prior_noise=[dev(z)], return_info=True, **kw)
    return s.encode_adaptive(_t(z), rtol=tol, atol=tol, return_info=True, **kw)


def _check_against_rows(tag, X, info, rows, grid_tol, res_tol):
    assert bool(info.converged.all()) and (info.status == 1).all()
    assert info.nfe.tolist() == [r["nfe"] for r in rows]
    grids = _grid_rows(info)
    assert [g.shape for g in grids] == [r["t"].shape for r in rows]
    dt = max(float(np.abs(g - r["t"]).max()) for g, r in zip(grids, rows))
    ref = np.stack([r["y"] for r in rows])
    log_line(f"[parity] rk45 ode grid {tag}: max |t_engine - t_restatement| = {dt:.3e} (bound {grid_tol:.3e})")
    report_err(f"rk45 ode result {tag} (bound {res_tol:.3e} of max(1, scale))", X.numpy(), ref)
    err = _rel(X.numpy(), ref)
    assert dt <= grid_tol
    assert err <= res_tol
    assert info.row_evals_needed == int(info.nfe.sum()) and info.row_evals_launched >= info.row_evals_needed


@pytest.mark.parametrize("name", list(FIXTURES))
def test_adaptive_run_against_the_restatement(name):
    m, s, z, start, rows, grid_tol, res_tol = _fixture(name)
    X, info = _engine(name)
    assert info.rtol == FIXTURES[name][2] and info.atol == FIXTURES[name][2]
    assert info.nfe.dtype == torch.int64 and info.converged.dtype == torch.bool and info.grid.dtype == torch.float64
    _check_against_rows(name, X, info, rows, grid_tol, res_tol)


# ------------------------------------------------------------------------------------------------- 2. arithmetic on its own grid
@pytest.mark.parametrize("back", [True, False], ids=["backward", "encode"])
@pytest.mark.parametrize("backbone,sde", [("transformer", VP), ("transformer", VE), ("mlp", VP), ("lstm", VP)])
def test_adaptive_arithmetic_on_its_own_grid(backbone, sde, back):
    """The controller aside: the restatement's fixed-step Dormand-Prince on the grid the engine chose gives the engine's result."""
    cfg, n, tol = CFG_T8, 2, 1e-3
    kind, p = sde
    if kind == "ve":
        m, sch, sd = make_model(cfg, kind=kind, p=p)
        score = R.model_score(sd, "transformer", cfg["H"])
    else:
        m, sch, sd, score = _model(backbone, cfg)
    s = _sampler(m)
    z = W.randn(f"rka_x_{backbone}_{kind}", (n, cfg["T"], cfg["C"]), 0)
    if back:
        start = host(s.sample_prior(n, noise=dev(z)))
        X, info = s.decode_adaptive(_t(start), rtol=tol, atol=tol, return_info=True)
    else:
        start = host(_t(z))
        X, info = s.encode_adaptive(_t(z), rtol=tol, atol=tol, return_info=True)
    assert bool(info.converged.all())
    g = info.grid.numpy()
    assert (g[:, 0] == (1.0 if back else EPS)).all()
    ref = A.on_grid(oracle_sde(kind, p, True, cfg["T"]), score, start, g)
    report_err(f"rk45 ode fixed-grid DP {backbone} {kind} {'backward' if back else 'encode'}", X.numpy(), ref)
    assert _rel(X.numpy(), ref) <= 1e-5


# ------------------------------------------------------------------------------------------------- 3. convergence
def test_convergence_with_the_tolerance():
    lat, _ = A.tight_reference()
    gold = np.load(GOLDEN)
    assert np.array_equal(gold["latents"], lat)      # (the reference on file is that of these inputs)
    m, sch, sd = make_model(CFG_T20)
    s = _sampler(m)
    out = {}
    for tol in (1e-3, 1e-5):
        X, info = s.decode_adaptive(_t(lat), rtol=tol, atol=tol, return_info=True)
        assert bool(info.converged.all())
        out[tol] = (info.nfe.numpy(), _rel(X.numpy(), gold["x"]))
        log_line(f"[parity] rk45 ode rtol={tol:g}: nfe {out[tol][0].tolist()}, |engine - restatement(1e-10)| = {out[tol][1]:.3e} of scale")
    assert (out[1e-3][0] < out[1e-5][0]).all()
    assert out[1e-5][1] < out[1e-3][1]
    X0 = _t(W.randn("rks_z_vp", (3, CFG_T20["T"], CFG_T20["C"]), 0))
    trip = {tol: float((s.decode_adaptive(s.encode_adaptive(X0, rtol=tol, atol=tol), rtol=tol, atol=tol) - X0).abs().max())
            for tol in (1e-3, 1e-5)}
    log_line(f"[parity] rk45 ode decode(encode(X)) - X: {trip[1e-3]:.3e} at 1e-3, {trip[1e-5]:.3e} at 1e-5")
    assert trip[1e-5] < trip[1e-3]


# ------------------------------------------------------------------------------------------------- 4. reproducible, row-independent
def _same(a, b):
    (Xa, ia), (Xb, ib) = a, b
    assert torch.equal(Xa, Xb) and torch.equal(ia.nfe, ib.nfe) and torch.equal(ia.status, ib.status)
    assert torch.equal(torch.nan_to_num(ia.grid, nan=-1.0), torch.nan_to_num(ib.grid, nan=-1.0))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_reproducible_and_row_independent(precision):
    cfg, n, tol = (CFG_T20, 3, 1e-3) if precision == "fp32" else (CFG_DEFAULT, 3, 1e-3)
    m, sch, sd = make_model(cfg, precision=precision)
    s = _sampler(m)
    X0 = _t(W.randn(f"rkb_x_{precision}", (n, cfg["T"], cfg["C"]), 0))
    kw = dict(rtol=tol, atol=tol, return_info=True)
    a = s.encode_adaptive(X0, **kw)
    assert bool(a[1].converged.all())
    _same(a, s.encode_adaptive(X0, **kw))
    lat = a[0]
    d = s.decode_adaptive(lat, **kw)
    _same(d, s.decode_adaptive(lat, **kw))
    if precision == "bf16":      # (the bf16 kernels round a row differently at another row count: B = 1 works, no more is asked)
        X1, i1 = s.encode_adaptive(X0[1:2], **kw)
        assert bool(i1.converged.all()) and bool(torch.isfinite(X1).all())
        return
    one = s.encode_adaptive(X0[1:2], **kw)      # B = 1
    assert bool(one[1].converged.all()) and int(one[1].nfe[0]) == int(a[1].nfe[1])
    g1, ga = _grid_rows(one[1])[0], _grid_rows(a[1])[1]
    assert g1.shape == ga.shape
    np.testing.assert_allclose(g1, ga, rtol=0, atol=1e-6)
    dx = _rel(one[0][0].numpy(), a[0][1].numpy().astype(np.float64))
    log_line(f"[parity] rk45 ode row independence: {dx:.3e} of scale")
    assert dx <= 1e-5


# ------------------------------------------------------------------------------------------------- 5. compaction
def test_compaction_changes_no_row(monkeypatch):
    name = "vp_encode_1e-3"      # rows finish four and two attempts apart
    m, s, z, start, rows, grid_tol, res_tol = _fixture(name)
    monkeypatch.setenv("FDIFF_RK_COMPACT", "0")
    Xoff, off = _engine(name)
    monkeypatch.delenv("FDIFF_RK_COMPACT")
    monkeypatch.setenv("FDIFF_RK_COMPACT_GRANULE", "1")
    Xon, on = _engine(name)
    monkeypatch.delenv("FDIFF_RK_COMPACT_GRANULE")
    Xarg, arg = _engine(name, compact_granule=1)
    _same((Xon, on), (Xarg, arg))
    assert arg.row_evals_launched == on.row_evals_launched
    assert torch.equal(on.nfe, off.nfe) and torch.equal(on.status, off.status)
    _check_against_rows(name + " compacted", Xon, on, rows, grid_tol, res_tol)
    _check_against_rows(name + " uncompacted", Xoff, off, rows, grid_tol, res_tol)
    B = 3
    assert off.row_evals_launched % B == 0      # every evaluation enqueued without compaction ran B rows
    log_line(f"[compaction] {name}: launched {on.row_evals_launched} with granule 1, {off.row_evals_launched} without, needed "
             f"{on.row_evals_needed}")
    assert on.row_evals_needed <= on.row_evals_launched < off.row_evals_launched
    # FDIFF_RK_COMPACT=0 wins over a granule
    monkeypatch.setenv("FDIFF_RK_COMPACT", "0")
    assert _engine(name, compact_granule=1)[1].row_evals_launched == off.row_evals_launched


def test_compaction_in_bf16_well_above_its_rounding():
    """bf16 at rtol = atol = 1e-3, rows of different magnitude so that they finish apart: the bf16 kernels round a row differently
    at another row count, which at this tolerance moves no step decision and moves the result by no more than bf16 against fp32
    does (BF16_BOUND) -- a row read from a wrong slot would do both."""
    cfg, tol = CFG_DEFAULT, 1e-3
    m, sch, sd = make_model(cfg, precision="bf16")
    s = _sampler(m)
    scale = torch.tensor([0.25, 1.0, 1.0, 2.0, 4.0]).view(5, 1, 1)
    X0 = _t(W.randn("rkq_x", (5, cfg["T"], cfg["C"]), 0)) * scale
    kw = dict(rtol=tol, atol=tol, return_info=True)
    Xoff, off = s.encode_adaptive(X0, **kw)      # (bf16: uncompacted by default)
    Xon, on = s.encode_adaptive(X0, compact_granule=1, **kw)
    d = _rel(Xon.numpy(), Xoff.numpy().astype(np.float64))
    log_line(f"[compaction] bf16 default shape rtol={tol:g}: nfe off {off.nfe.tolist()} on {on.nfe.tolist()}; launched {on.row_evals_launched} "
             f"with granule 1, {off.row_evals_launched} without, needed {on.row_evals_needed}; |on - off| = {d:.3e} of scale")
    assert bool(off.converged.all()) and bool(on.converged.all())
    assert len(set(off.nfe.tolist())) > 1 and off.row_evals_launched == 5 * (int(off.nfe.max()) + 6)      # the fixture: rows finish apart
    assert torch.equal(on.nfe, off.nfe) and torch.equal(on.status, off.status)
    assert [g.shape for g in _grid_rows(on)] == [g.shape for g in _grid_rows(off)]
    assert on.row_evals_needed <= on.row_evals_launched < off.row_evals_launched
    assert d <= BF16_BOUND


@pytest.mark.parametrize("slow_at", [0, 4], ids=["slow_first", "slow_last"])
def test_compaction_down_to_a_single_slot(slow_at):
    """All rows but one finish early: the launches shrink to one slot, which is row 0 (the slow row prepended) or row 4."""
    name = "vp_encode_1e-3"
    m, s, z, start, rows, grid_tol, res_tol = _fixture(name)
    order = [1, 1, 1, 1]
    order.insert(slow_at, 0)      # row 0 of the fixture needs 104 evaluations, row 1 needs 80
    X, info = s.encode_adaptive(_t(z[order]), rtol=1e-3, atol=1e-3, return_info=True, compact_granule=1)
    _check_against_rows(f"{name} single slot, slow row at {slow_at}", X, info, [rows[i] for i in order], grid_tol, res_tol)
    # 2 + 6 * 14 evaluations on 5 rows (row 1 freezes in attempt 13, the host knows one attempt later), the rest on one slot
    assert info.row_evals_launched < 5 * (2 + 6 * 15)


# ------------------------------------------------------------------------------------------------- 6. the evaluation cap
def test_evaluation_cap():
    cfg, n = CFG_T20, 3
    m, sch, sd = make_model(cfg)
    s = _sampler(m)
    X0 = _t(W.randn("rkm_x", (n, cfg["T"], cfg["C"]), 0))
    ref = s.encode_adaptive(X0, rtol=1e-3, atol=1e-3, return_info=True)
    with pytest.raises(RuntimeError, match=r"3 of 3 rows.*max_evals"):
        s.encode_adaptive(X0, rtol=1e-3, atol=1e-3, max_evals=8)
    X, info = s.encode_adaptive(X0, rtol=1e-3, atol=1e-3, max_evals=8, return_info=True)
    assert (info.nfe == 8).all() and not bool(info.converged.any()) and (info.status == 3).all()
    assert bool(torch.isfinite(X).all())
    g = _grid_rows(info)
    assert all(len(r) in (1, 2) and r[0] == EPS for r in g)      # one attempt: accepted or not
    assert all(len(r) == 2 or torch.equal(X[b], X0[b]) for b, r in enumerate(g))      # (nothing accepted: the state is the input)
    _same(s.encode_adaptive(X0, rtol=1e-3, atol=1e-3, return_info=True), ref)


# ------------------------------------------------------------------------------------------------- 7. bf16 at the default shape
# |bf16 - fp32| of the sample at rtol = atol = 1e-3, of scale max(1, |fp32|max): measured 1.785e-3 on an MI355X (both runs nfe 80 a
# row), the bound is that with 3.4x margin
BF16_BOUND = 6e-3


def test_bf16_at_the_default_shape():
    cfg, n, tol = CFG_DEFAULT, 3, 1e-3      # T C = 1200: no multiple of the block
    z = W.randn("rkh_z", (n, cfg["T"], cfg["C"]), 0)
    out = {}
    for precision in ("fp32", "bf16"):
        m, sch, sd = make_model(cfg, precision=precision)
        out[precision] = _sampler(m).sample_ode_adaptive(n, rtol=tol, atol=tol, prior_noise=[dev(z)], return_info=True)
    (Xf, f), (Xb, b) = out["fp32"], out["bf16"]
    d = _rel(Xb.numpy(), Xf.numpy().astype(np.float64))
    log_line(f"[parity] rk45 ode default shape rtol={tol:g}: nfe fp32 {f.nfe.tolist()} bf16 {b.nfe.tolist()}; |bf16 - fp32| = {d:.3e} of "
             f"scale {float(Xf.abs().max()):.3e}")
    assert bool(f.converged.all()) and bool(b.converged.all())
    assert bool(torch.isfinite(Xb).all())
    assert d <= BF16_BOUND


# ------------------------------------------------------------------------------------------------- 8. guided
def _cond_model(cfg):
    from tests.test_gpu_cfg import make_cond
    return make_cond(cfg, "fp32")


def test_guided_encode_with_labels(monkeypatch):
    cfg, n, tol = CFG_T8, 3, 1e-3
    m, sch, sd, tab = _cond_model(cfg)
    s = _sampler(m)
    osde = oracle_sde("vp", (0.1, 20.0), True, cfg["T"])
    z = W.randn("rkg_x", (n, cfg["T"], cfg["C"]), 0)
    y = [0, 2, 1]

    def ref_on(grid, w):
        return np.concatenate([A.on_grid(osde, cfg_ref.guided_score_fn(sd, tab, y[b:b + 1], w, cfg["H"]), host(_t(z[b:b + 1])), grid[b:b + 1])
                               for b in range(n)])
    X2, i2 = s.encode_adaptive(_t(z), rtol=tol, atol=tol, return_info=True, y=torch.tensor(y), cfg_scale=2.0)
    assert bool(i2.converged.all())
    report_err("rk45 ode guided w=2 (pair form) on its own grid", X2.numpy(), ref_on(i2.grid.numpy(), 2.0))
    assert _rel(X2.numpy(), ref_on(i2.grid.numpy(), 2.0)) <= 1e-5
    X1, i1 = s.encode_adaptive(_t(z), rtol=tol, atol=tol, return_info=True, y=torch.tensor(y), cfg_scale=1.0)
    assert _rel(X1.numpy(), ref_on(i1.grid.numpy(), 1.0)) <= 1e-5
    monkeypatch.setenv("FDIFF_CFG_FORCE_PAIR", "1")      # w = 1 in the two-evaluation form: the combine is exact
    Xp, ip = s.encode_adaptive(_t(z), rtol=tol, atol=tol, return_info=True, y=torch.tensor(y), cfg_scale=1.0)
    assert torch.equal(ip.nfe, i1.nfe)
    report_err("rk45 ode guided w=1: pair form against one evaluation", Xp.numpy(), X1.numpy())
    assert _rel(Xp.numpy(), X1.numpy().astype(np.float64)) <= 1e-5
    monkeypatch.delenv("FDIFF_CFG_FORCE_PAIR")
    # guided sampling from the prior goes through the same loop
    Xs, is_ = s.sample_ode_adaptive(n, rtol=tol, atol=tol, return_info=True, y=torch.tensor(y), cfg_scale=2.0,
                                    prior_noise=[dev(W.randn("rkg_z", (n, cfg["T"], cfg["C"]), 0))])
    assert bool(is_.converged.all()) and bool(torch.isfinite(Xs).all())


def test_labels_on_an_unlabelled_model_raise():
    m, sch, sd = make_model(CFG_T8)
    s = _sampler(m)
    X = torch.zeros(2, CFG_T8["T"], CFG_T8["C"])
    with pytest.raises(ValueError):
        s.encode_adaptive(X, rtol=1e-3, atol=1e-3, y=torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        s.sample_ode_adaptive(2, rtol=1e-3, atol=1e-3, cfg_scale=2.0)


def test_guided_encode_with_covariates():
    from tests.test_gpu_cov import make_cov
    cfg, n, tol = CFG_T8, 3, 1e-3
    m, sch, sd, enc = make_cov(cfg, "fp32")
    s = _sampler(m)
    osde = oracle_sde("vp", (0.1, 20.0), True, cfg["T"])
    z = W.randn("rkc_x", (n, cfg["T"], cfg["C"]), 0)
    c = cov_ref.covariates(n, tag="rk")
    X2, i2 = s.encode_adaptive(_t(z), rtol=tol, atol=tol, return_info=True, y=torch.from_numpy(c), cfg_scale=2.0)
    assert bool(i2.converged.all())
    e_c, e_0 = cov_ref.encode(enc, c), cov_ref.encode(enc, None, n=1)
    g = i2.grid.numpy()
    ref = np.concatenate([A.on_grid(osde, cov_ref.guided_score_fn(sd, e_c[b:b + 1], e_0, 2.0, cfg["H"]), host(_t(z[b:b + 1])), g[b:b + 1])
                          for b in range(n)])
    report_err("rk45 ode covariate-guided w=2 (pair form) on its own grid", X2.numpy(), ref)
    assert _rel(X2.numpy(), ref) <= 1e-5


# ------------------------------------------------------------------------------------------------- 9. CLI
def test_cli_train_then_sample_ode_adaptive(tmp_path):
    common = ["fourier_transform=true", "datamodule.max_len=24", "datamodule.num_samples=96", "datamodule.n_channels=4",
              "datamodule.batch_size=32"]
    _run([str(ROOT / "cmd" / "train.py"), *common, "score_model.d_model=24", "score_model.num_layers=2", "score_model.n_head=4",
          "trainer.max_epochs=2", "trainer.callbacks.2.every_n_epochs=2", "trainer.callbacks.2.num_samples=32",
          "trainer.callbacks.2.num_diffusion_steps=5", "run_id=rkode"], tmp_path)
    _run([str(ROOT / "cmd" / "sample.py"), "model_id=rkode", "sampler=ode_adaptive", "sampler.rtol=1e-3", "sampler.atol=1e-3",
          "num_samples=40", "sampler.sample_batch_size=20"], tmp_path)
    res = yaml.safe_load(open(tmp_path / "lightning_logs" / "rkode" / "results.yaml"))
    for k in ("nfe_mean", "nfe_max", "n_not_converged", "row_evals_launched"):
        assert k in res, k
    assert res["n_not_converged"] == 0 and res["nfe_max"] >= res["nfe_mean"] >= 8
    assert res["row_evals_launched"] >= 40 * res["nfe_mean"] - 1e-6
    for k, v in res.items():
        if isinstance(v, float):
            assert np.isfinite(v), k
    X = torch.load(tmp_path / "lightning_logs" / "rkode" / "samples.pt")
    assert X.shape == (40, 24, 4) and bool(torch.isfinite(X).all())
