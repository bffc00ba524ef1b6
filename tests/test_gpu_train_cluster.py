"""GPU tests of the cluster exchange of the persistent training forward (k_tr_fwd_layers, csrc/fd_train_persist.hip) on BOTH of its
paths, at the benched grid and over many optimizer steps.

A cluster of workgroups owns a series for every encoder layer and exchanges each layer's input rows through memory behind per-tile
flags.  The exchange has two forms, chosen per layer and cluster inside the kernel: when every workgroup of the cluster reports the
same XCD, plain stores and L1-bypassing (sc0) loads behind one `buffer_inv sc0` (the rows meet in that XCD's L2); otherwise, and for
the first layer of a launch, agent-scope (sc1) stores and loads through the memory side.  Which form runs depends on where the
dispatcher puts the workgroups: `xcd_deal` re-deals the workgroup ids so that a series' workgroups share an XCD (FDIFF_TR_XCD=1, the
default); FDIFF_TR_XCD=0 leaves them in hardware order, where the members of a cluster of two or more land on different XCDs.  By
its own header the hand-over "rests on the gfx950 memory pipeline, not on the HIP memory model", and a row read stale -- an L1 line
left from the previous training step at the same address, an L2 line on the wrong XCD -- would not crash: the step would quietly
train on old activations.

The exchange is deterministic (no atomics in any sum, a fixed order everywhere, placement changes no arithmetic), so every comparison
here is EXACT: `==` on the loss, `torch.equal` on gradients, parameters and Adam moments.  One stale or torn row changes a bf16 value
and therefore bits downstream.

  (a) one step of the default form is bit-identical under both placements, each behind a step on other inputs under that placement;
  (b) in the natural chunk order (FDIFF_TR_ROT=0, unsplit FFN kernels, 4 tiles per workgroup) the persistent launch equals the
      per-layer kernels bit for bit under EITHER placement at B = 64 (tests/test_gpu_train_persist.py: B <= 9 and B = 150, re-deal on);
  (c) 200 optimizer steps, a fresh batch per step (so every step overwrites the exchanged rows at the same addresses with other
      values): default form under both placements, and natural order persistent against per-layer -- equal losses step by step,
      equal final parameters and moments;
  (d) the two paths really ran: the publisher XCDs of the tile flags, read back through ScoreModule.train_cluster_xcds
      (fd_score_train_cluster_xcds), show at least one series on one XCD with the re-deal and at least one spread over several
      without it (counts logged);
  (e) the F-split hand-over of the FFN kernels (same mechanism, same caveat) is bit-identical under both placements, and equals its
      fence form under the other placement;
  (f) the argument and state errors of the read-out.

Shapes: the two benched training shapes at full depth and B = 64 -- 4 x 64 = 256 workgroups, one per CU, the only regime in which
every CU's L1 and every XCD's L2 take part -- plus T = 187, C = 1 (odd length, ragged last tile, clusters of three).  Dropout 0.1
throughout, so the decision buffers and the mask stream take part.
"""
import numpy as np
import pytest
import torch

from .gpu_util import DEV, make_model
from .test_gpu_train_persist import _data, _log, _step

pytestmark = pytest.mark.gpu

B = 64
BENCHED = {"nasdaq": dict(T=252, C=6, D=72, L=10, H=12),       # NT = 4, 4 x 64 workgroups
           "ecg": dict(T=100, C=12, D=72, L=10, H=12)}         # NT = 2, 4 x 64 workgroups
SHAPES = dict(BENCHED, ragged=dict(T=187, C=1, D=72, L=2, H=12))      # NT = 4, 3 x 64 workgroups
PLANS = {"nasdaq": "k_tr_fwd_layers NT=4, 4 x 64 workgroups", "ecg": "k_tr_fwd_layers NT=2, 4 x 64 workgroups",
         "ragged": "k_tr_fwd_layers NT=4, 3 x 64 workgroups"}
NATURAL = {"FDIFF_TR_ROT": "0", "FDIFF_TR_FSPLIT": "0", "FDIFF_TR_PERSIST_NT": "4"}
K_STEPS = 200


def _model(cfg):
    from fourierdiffusion_amd.utils.losses import get_sde_loss_fn
    m, sch, _ = make_model(cfg, precision="bf16")
    m.dropout = 0.1
    return m, get_sde_loss_fn(sch, train=True)


def _no_wait_gave_up(m):
    from fourierdiffusion_amd import _C
    ctx, _h = m._engine()
    assert _C.lib().fd_ctx_check(ctx) == 0, _C.lib().fd_last_error(ctx)


# ---------------------------------------------------------------------------------------------- (a) + (d): one step, both placements
_PLACEMENT = {}      # shape name -> {"1" | "0": (loss, flat gradient, publisher XCDs [series][tile])}: computed once, shared by (a) and (d)


def _placement_runs(monkeypatch, name):
    if name not in _PLACEMENT:
        cfg = SHAPES[name]
        X, z, t = _data(f"cluster_{name}", cfg, B)
        other = _data(f"cluster_other_{name}", cfg, B)
        m, fn = _model(cfg)
        monkeypatch.setenv("FDIFF_TR_PERSIST", "1")
        res = {}
        for xcd in ("1", "0"):
            monkeypatch.setenv("FDIFF_TR_XCD", xcd)
            # a step on OTHER inputs under the same placement first: it leaves its rows, at the addresses the compared step exchanges
            # through, in whatever cache the readers of that placement went through (a lone step in a fresh process meets clean caches)
            _step(m, fn, *other, seed=56)
            loss, g, _ = _step(m, fn, X, z, t)
            assert np.isfinite(loss) and bool(torch.isfinite(g).all())
            res[xcd] = (loss, g.cpu(), m.train_cluster_xcds(B))
        assert PLANS[name] in m.train_plan(B)[0], m.train_plan(B)[0]
        _no_wait_gave_up(m)
        _PLACEMENT[name] = res
    return _PLACEMENT[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_default_form_is_bit_identical_under_both_placements(monkeypatch, name):
    res = _placement_runs(monkeypatch, name)
    (l1, g1, _), (l0, g0, _) = res["1"], res["0"]
    nd = int((g1 != g0).sum().item())
    _log(f"[parity] cluster exchange, default form, {name} B={B}: loss {l1!r} (re-deal) vs {l0!r} (hardware order); gradient elements that "
         f"differ: {nd} of {g1.numel()}")
    assert l1 == l0 and nd == 0, "the step depends on where the dispatcher put the cluster's workgroups"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_both_exchange_paths_really_ran(monkeypatch, name):
    """Conditions, not measurements: a series whose tiles were all published from one XCD is exactly the kernel's `all_here`
    (same-XCD fast path from the second layer on); any other series took the memory-side path for every layer.  Nothing guarantees
    the dispatcher's deal, so "at least one", not "all"."""
    res = _placement_runs(monkeypatch, name)
    x1, x0 = res["1"][2], res["0"][2]
    KT = (SHAPES[name]["T"] + 15) // 16
    assert x1.shape == x0.shape == (B, KT)
    assert int(x1.min()) >= 0 and int(x0.min()) >= 0 and int(x1.max()) < 16 and int(x0.max()) < 16
    one1 = int((x1 == x1[:, :1]).all(dim=1).sum())
    one0 = int((x0 == x0[:, :1]).all(dim=1).sum())
    xcds = sorted(set(x1.flatten().tolist()) | set(x0.flatten().tolist()))
    _log(f"[path] cluster exchange {name} B={B} ({PLANS[name]}): series with every tile published from ONE XCD: {one1} of {B} with the re-deal "
         f"(FDIFF_TR_XCD=1), {one0} of {B} in hardware order (FDIFF_TR_XCD=0); XCDs seen: {xcds}")
    if len(xcds) == 1:
        pytest.skip(f"the device reports a single XCD ({xcds[0]}) for {B * x1.shape[1]} tiles under both placements: there is one path only")
    assert one1 >= 1, "no cluster ran on one XCD under the re-deal: the same-XCD fast path was never taken (xcd_deal does not do its job)"
    assert B - one0 >= 1, "every cluster ran on one XCD in hardware order: the memory-side path was taken for first layers only"


# ---------------------------------------------------------------------------------------------- (b): natural order vs per-layer kernels
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_natural_order_equals_the_per_layer_kernels_under_both_placements(monkeypatch, name):
    cfg = SHAPES[name]
    X, z, t = _data(f"cluster_nat_{name}", cfg, B)
    m, fn = _model(cfg)
    for k, v in NATURAL.items():
        monkeypatch.setenv(k, v)
    res = {}
    for xcd in ("0", "1"):
        monkeypatch.setenv("FDIFF_TR_XCD", xcd)
        for persist in ("0", "1"):
            monkeypatch.setenv("FDIFF_TR_PERSIST", persist)
            loss, g, _ = _step(m, fn, X, z, t)
            assert np.isfinite(loss) and bool(torch.isfinite(g).all())
            res[xcd, persist] = (loss, g)
            assert ("k_tr_fwd_layers NT=4" if persist == "1" else "2 kernels per layer") in m.train_plan(B)[0], m.train_plan(B)[0]
        nd = int((res[xcd, "1"][1] != res[xcd, "0"][1]).sum().item())
        _log(f"[parity] persistent forward vs per-layer kernels, natural chunk order, {name} B={B}, FDIFF_TR_XCD={xcd}: loss "
             f"{res[xcd, '1'][0]!r} vs {res[xcd, '0'][0]!r}; gradient elements that differ: {nd} of {res[xcd, '0'][1].numel()}")
        assert res[xcd, "1"][0] == res[xcd, "0"][0] and nd == 0, f"the persistent launch differs from the per-layer kernels (FDIFF_TR_XCD={xcd})"
    assert res["0", "1"][0] == res["1", "1"][0] and torch.equal(res["0", "1"][1], res["1", "1"][1]), "placement changed the persistent form's bits"
    assert res["0", "0"][0] == res["1", "0"][0] and torch.equal(res["0", "0"][1], res["1", "0"][1]), "placement changed the per-layer kernels' bits"
    _no_wait_gave_up(m)


# ---------------------------------------------------------------------------------------------- (c): many optimizer steps
_BATCHES = {}        # shape name -> (X, z, t) of every step on the device: drawn once from one seeded CPU generator, never modified


def _batches(name):
    if name not in _BATCHES:
        cfg = BENCHED[name]
        g = torch.Generator(device="cpu").manual_seed(20251)
        shape = (K_STEPS, B, cfg["T"], cfg["C"])
        X = torch.randn(shape, generator=g)
        z = torch.randn(shape, generator=g)
        t = torch.rand((K_STEPS, B), generator=g) * 0.95 + 0.05
        _BATCHES[name] = (X.to(DEV), z.to(DEV), t.to(DEV))
    return _BATCHES[name]


def _train(name, plan):
    """K_STEPS optimizer steps from the initial state of make_model: (loss of every step, final parameters, both Adam moments)."""
    from fourierdiffusion_amd.optim import FusedAdamW
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    X, z, t = _batches(name)
    m, fn = _model(BENCHED[name])
    opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0)
    losses = []
    for i in range(K_STEPS):
        opt.zero_grad()
        torch.manual_seed(1000 + i)
        losses.append(fn(m, DiffusableBatch(X=X[i], y=None, timesteps=t[i]), noise=z[i]))
        opt.step()
    losses = torch.stack(losses).tolist()
    assert m.train_mode_effective == "bf16" and plan in m.train_plan(B)[0], m.train_plan(B)[0]
    _no_wait_gave_up(m)
    assert all(np.isfinite(l) for l in losses), "non-finite loss"
    return losses, m.flat_parameters.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()


def _assert_same_run(what, a, b):
    first = next((i for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y), None)
    assert first is None, f"{what}: the losses differ from step {first} on ({a[0][first]!r} vs {b[0][first]!r}) of {len(a[0])} steps"
    for label, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), a[1:], b[1:]):
        nd = int((x != y).sum().item())
        assert nd == 0, f"{what}: {K_STEPS} equal losses, but {nd} of {x.numel()} elements of the final {label} differ"


@pytest.mark.parametrize("name", sorted(BENCHED))
def test_200_steps_default_form_are_bit_identical_under_both_placements(monkeypatch, name):
    """The default form (rotated chunk order, default tiles per workgroup) under the re-deal -- same-XCD fast path from the second layer
    of every launch on -- against hardware order -- memory-side path everywhere.  Each configuration runs once, for a fixed count."""
    monkeypatch.setenv("FDIFF_TR_PERSIST", "1")
    runs = {}
    for xcd in ("1", "0"):
        monkeypatch.setenv("FDIFF_TR_XCD", xcd)
        runs[xcd] = _train(name, PLANS[name])
    _log(f"[parity] cluster exchange, {K_STEPS} optimizer steps, default form, {name} B={B}: last loss {runs['1'][0][-1]!r} (re-deal) vs "
         f"{runs['0'][0][-1]!r} (hardware order)")
    _assert_same_run(f"{name}: FDIFF_TR_XCD=1 vs FDIFF_TR_XCD=0", runs["1"], runs["0"])


@pytest.mark.parametrize("name", sorted(BENCHED))
def test_200_steps_natural_order_equal_the_per_layer_kernels(monkeypatch, name):
    """The persistent launch against kernels that exchange nothing between workgroups, in the one order in which the two compute the
    same sums.  Default placement (the re-deal): the persistent run takes the same-XCD fast path, the one that reads rows another CU
    wrote without an acquire, 200 times over the same addresses."""
    for k, v in NATURAL.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("FDIFF_TR_XCD", "1")
    runs = {}
    for persist, plan in (("0", "2 kernels per layer"), ("1", "k_tr_fwd_layers NT=4")):
        monkeypatch.setenv("FDIFF_TR_PERSIST", persist)
        runs[persist] = _train(name, plan)
    _log(f"[parity] cluster exchange, {K_STEPS} optimizer steps, natural chunk order, {name} B={B}: last loss {runs['1'][0][-1]!r} (persistent) vs "
         f"{runs['0'][0][-1]!r} (per-layer kernels)")
    _assert_same_run(f"{name}: persistent launch vs per-layer kernels", runs["1"], runs["0"])


# ---------------------------------------------------------------------------------------------- (e): the F-split hand-over
def test_ffn_f_split_is_bit_identical_under_both_placements_and_equals_its_fence_form(monkeypatch):
    """The shape of test_ffn_f_split_survives_a_cotenant_kernel_and_its_fence_form_agrees: 125 token blocks -> 250 workgroups on 256
    CUs, both FFN kernels split (FDIFF_TR_FSPLIT=2), per-layer kernels.  A producer / finisher pair has consecutive workgroup ids: in
    hardware order the two sit on different XCDs."""
    cfg, Bf = dict(T=100, C=12, D=72, L=2, H=12), 80
    X, z, t = _data("cluster_fsplit", cfg, Bf)
    m, fn = _model(cfg)
    monkeypatch.setenv("FDIFF_TR_PERSIST", "0")
    monkeypatch.setenv("FDIFF_TR_FSPLIT", "0")
    l_un, g_un, _ = _step(m, fn, X, z, t, seed=91)
    monkeypatch.setenv("FDIFF_TR_FSPLIT", "2")
    res = {}
    for xcd in ("0", "1"):
        monkeypatch.setenv("FDIFF_TR_XCD", xcd)
        res[xcd] = _step(m, fn, X, z, t, seed=91)[:2]
    assert not torch.equal(res["1"][1], g_un), "the split form did not run (same bits as the unsplit kernels)"
    assert res["0"][0] == res["1"][0] and torch.equal(res["0"][1], res["1"][1]), "the F-split step depends on the placement of its pairs"
    monkeypatch.setenv("FDIFF_TR_XCD", "0")
    monkeypatch.setenv("FDIFF_TR_FSPLIT_FENCE", "1")
    lf, gf, _ = _step(m, fn, X, z, t, seed=91)
    assert lf == res["0"][0] and torch.equal(gf, res["0"][1]), "fence form and coherent-access form of the hand-over disagree in hardware order"
    _no_wait_gave_up(m)


# ---------------------------------------------------------------------------------------------- (f): the read-out's errors
def test_cluster_read_out_argument_and_state_errors(monkeypatch):
    import ctypes as C

    from fourierdiffusion_amd import _C
    cfg, Bs = dict(T=100, C=12, D=72, L=2, H=12), 9
    KT = 7
    X, z, t = _data("cluster_args", cfg, Bs)
    m, fn = _model(cfg)
    ctx, h = m._engine()
    lib = _C.lib()
    buf = (C.c_int * (2 * Bs * KT))()
    stream = _C.stream_of(m.flat_parameters)
    assert lib.fd_score_train_cluster_xcds(None, Bs, buf, stream) == -1                 # FD_ERR_ARG: no model
    with pytest.raises(_C.FdError, match="error -3.*not a persistent launch"):          # FD_ERR_STATE: before any training forward of this model
        m.train_cluster_xcds(Bs)
    monkeypatch.setenv("FDIFF_TR_PERSIST", "1")
    _step(m, fn, X, z, t)
    got = m.train_cluster_xcds(Bs)
    assert got.shape == (Bs, KT) and got.dtype == torch.int32 and int(got.min()) >= 0 and int(got.max()) < 16
    assert lib.fd_score_train_cluster_xcds(h, Bs, None, stream) == -1                   # FD_ERR_ARG: null pointer
    assert b"null pointer" in lib.fd_last_error(ctx)
    for bad in (Bs + 1, Bs - 1, 0):                                                     # FD_ERR_ARG: a B that is not the forward's
        assert lib.fd_score_train_cluster_xcds(h, bad, buf, stream) == -1, bad
    assert b"B=0" in lib.fd_last_error(ctx)
    with pytest.raises(_C.FdError, match=f"error -1.*B={Bs + 1}, the last persistent training forward ran B={Bs}"):
        m.train_cluster_xcds(Bs + 1)
    assert torch.equal(m.train_cluster_xcds(Bs), got)                                   # (a refused call changed nothing)
    for mode in ("0", "2"):             # per-layer kernels; the layer kernel launched once per layer (no cluster wait is ever exercised)
        monkeypatch.setenv("FDIFF_TR_PERSIST", mode)
        _step(m, fn, X, z, t)
        with pytest.raises(_C.FdError, match="error -3.*not a persistent launch"):
            m.train_cluster_xcds(Bs)
    monkeypatch.setenv("FDIFF_TR_PERSIST", "1")
    _step(m, fn, X, z, t)
    other, _ = _model(cfg)                                                              # another model on the same context
    with pytest.raises(_C.FdError, match="error -3"):
        other.train_cluster_xcds(Bs)
    assert m.train_cluster_xcds(Bs).shape == (Bs, KT)                                   # (... while the model that ran last still answers)
    _no_wait_gave_up(m)
