"""CPU: tests/bb_autograd_ref.py (the float64 autograd restatement of the MLP / LSTM backbones with injected dropout masks) pinned to
the oracle's forward, to central differences and to the reference project's own autograd (tests/golden/backbones.npz), its mask rule
checked element by element, and every case of tests/bb_shapes_ref.py checked on the reference alone: the relu guard, the split-K
claims of the case table, and the float32 error of the restatement, which is the floor under the GPU test's 1e-5 bound."""
import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W
from oracle.make_golden import CFG_BB
from tests import bb_autograd_ref as A
from tests import bb_shapes_ref as S
from tests.gpu_util import log_line, oracle_sde

ORACLE_FWD = {"mlp": O.mlp_score_forward, "lstm": O.lstm_score_forward}


def _small(kind):
    cfg, B = CFG_BB, 4
    sd = W.make_state_dict_backbone(kind, cfg["C"], cfg["T"], cfg["D"], cfg["L"], d_mlp=64, seed=4321)
    X = W.randn(f"bb_x_{kind}_small", (B, cfg["T"], cfg["C"]), 5)
    t = W.uniform(f"bb_t_{kind}_small", (B,), 5, 0.05, 1.0)
    z = W.randn(f"bb_z_{kind}_small", (B, cfg["T"], cfg["C"]), 5)
    return cfg, sd, X, t, z


@pytest.mark.parametrize("where", ["small_mlp", "small_lstm", "lstm_73", "mlp_tails"])
def test_forward_without_masks_is_the_oracle_forward(where):
    if where.startswith("small_"):
        kind = where[len("small_"):]
        _, sd, x, t, _ = _small(kind)
    else:
        kind, sd = S.CASES[where]["kind"], S.weights(where)
        x, t, _ = S.inputs(where, S.CASES[where]["seed"])
    ref = ORACLE_FWD[kind](sd, x, t)
    err = float(np.abs(A.score(kind, sd, x, t) - ref).max() / np.abs(ref).max())
    print(f"bb_autograd_ref forward {where}: {err:.2e} of the maximum")
    assert err <= 1e-12


def _phi(kind, sd, x, t, u, mask):
    """<score, u> in float64 and whether each relu unit is on."""
    net = A.Net(kind, sd)
    with torch.no_grad():
        out = net.forward(torch.tensor(np.asarray(x, dtype=np.float64)), t, mask).numpy()
    return float((out * u).sum()), [p.numpy() > 0 for p in net.pre]


@pytest.mark.parametrize("tag", list(S.CASES))
def test_gradients_against_central_differences(tag):
    """<grad, v> along three random parameter directions (every trainable tensor at once, each scaled to its tensor's maximum) and one
    input direction against a central difference of <score, u> in float64, masks on.  Step 1e-6: the truncation error is of the order
    of step^2 and the cancellation error 1e-16 / step of <score, u>, both far below the 1e-6 bound; the relu guard of the cases keeps
    every unit 3e-5 of its layer's maximum from its kink, and the test asserts that no unit changes sign over the step."""
    cs = S.case(tag)
    c, sd, mask = cs["cfg"], cs["sd"], cs["mask"]
    x, t, u = cs["x"].astype(np.float64), cs["t"], cs["u"].astype(np.float64)
    g = cs["ref"]
    step = 1e-6
    _, on0 = _phi(c["kind"], sd, x, t, u, mask)
    for i in range(4):
        if i < 3:
            v = {k: W.randn(f"bbcd_{tag}_{i}_{k}", sd[k].shape, 0).astype(np.float64) * np.abs(sd[k]).max() for k in g["grads"]}
            lhs = sum(float((g["grads"][k] * v[k]).sum()) for k in v)
            mv = lambda s: ({k: (np.asarray(a, dtype=np.float64) + s * v[k] if k in v else a) for k, a in sd.items()}, x)   # noqa: E731
        else:
            vx = W.randn(f"bbcd_{tag}_x", x.shape, 0).astype(np.float64)
            lhs = float((g["dx"] * vx).sum())
            mv = lambda s: (sd, x + s * vx)      # noqa: E731
        (hi, on_hi), (lo, on_lo) = _phi(c["kind"], *mv(step), t, u, mask), _phi(c["kind"], *mv(-step), t, u, mask)
        assert all(np.array_equal(a, b) and np.array_equal(a, o) for a, b, o in zip(on_hi, on_lo, on0)), \
            "the central difference crosses a relu kink"
        rhs = (hi - lo) / (2.0 * step)
        err = abs(lhs - rhs) / abs(rhs)
        print(f"bb_autograd_ref {tag} direction {'x' if i == 3 else i}: <grad, v> = {lhs:.6e}, central difference {rhs:.6e}, "
              f"relative {err:.2e}")
        assert err <= 1e-6, (i, lhs, rhs)


@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_gradients_reproduce_the_reference_projects_autograd(golden, kind):
    """The restatement chained through O.perturb and the DSM loss (O.dsm_loss's weighting: mean over the batch and over T C of
    w_b (score + target)^2, w_b = 1 / sum_t std^-2) at the configuration of the fixture, dropout 0, within the 3e-4 of each tensor's
    maximum that tests/test_gpu_backbones.py holds the engine to against the same file (float32 autograd of the reference project)."""
    g = golden("backbones")
    cfg, sd, X, t, z = _small(kind)
    sde = oracle_sde("vp", (0.1, 20.0), True, cfg["T"])
    Xn, target, std = O.perturb(sde, X, t, z)
    score = A.score(kind, sd, Xn, t)
    loss = O.dsm_loss(score, target, std, False)
    assert abs(loss - float(g[f"loss_{kind}_small"])) <= 2e-5 * abs(loss)
    w = 1.0 / np.sum(1.0 / std ** 2, axis=1)
    u = 2.0 * w[:, None, None] * (score + target) / score.size               # d loss / d score
    got = A.grads(kind, sd, Xn, t, u)["grads"]
    keys = [f for f in g.files if f.startswith(f"grad_{kind}_small/")]
    assert sorted(k.split("/", 1)[1] for k in keys) == sorted(got)
    worst = 0.0
    for key in keys:
        ref = g[key]
        err = float(np.abs(got[key.split("/", 1)[1]] - ref).max() / np.abs(ref).max())
        worst = max(worst, err)
        assert err <= 3e-4, (key, err)
    print(f"bb_autograd_ref {kind} vs the reference project's autograd: worst tensor {worst:.2e} of its maximum")


@pytest.mark.parametrize("n", [125, 250, 9216])
def test_mask_rule_element_by_element(n):
    """masks() against one Philox evaluation per ELEMENT with the float32 steps of fd_u01 spelled out on scalars ((word >> 8) + 0.5 does
    not fit 24 bits above 2^23: it rounds, and the rule is what float32 gives), and the kept fraction within 4 sigma of 1 - p."""
    key, offset, layer, site, p = S.dropout_key(), 7, 2, 1, 0.3
    got = A.masks(key, offset, layer, site, n, p)
    base = offset + ((4 * layer + site) << 40)
    ctr = np.array([base + e // 4 for e in range(n)], dtype=np.uint64)
    counter = np.stack([ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)], axis=-1)
    kk = np.broadcast_to(np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint64), (n, 2))
    words = O.philox4x32_10(counter, kk)
    p32 = np.float32(p)
    scale = 1.0 / (1.0 - float(p32))
    for e in range(n):
        r = np.float32(int(words[e, e % 4]) >> 8)
        r = np.float32(r + np.float32(0.5))
        uu = np.float32(r * np.float32(2.0 ** -24))
        assert got[e] == (scale if uu >= p32 else 0.0), e
    kept = float((got > 0).mean())
    assert abs(kept - (1.0 - p)) <= 4.0 * np.sqrt(p * (1.0 - p) / n), kept
    assert np.array_equal(A.masks(key, offset, layer, site, n, 0.0), np.ones(n))
    # another site, layer or offset is another mask
    for other in ((offset, layer, 0), (offset, layer + 1, site), (offset + 1, layer, site)):
        assert not np.array_equal(A.masks(key, other[0], other[1], other[2], n, p), got)


@pytest.mark.parametrize("tag", S.MLP_CASES)
def test_stored_seed_is_the_first_that_passes_the_relu_guard(tag):
    c = S.CASES[tag]
    first = S.first_guard_seed(tag)
    pre = S.case(tag)["ref"]["pre"]
    margin = min(float(np.abs(p).min() / np.abs(p).max()) for p in pre)
    log_line(f"[guard] {tag}: dropout key {S.dropout_key()}, first input seed in range(64) passing the relu guard = {first} "
             f"(stored {c['seed']}); smallest |pre| / max|pre| of a layer {margin:.3e} (guard {A.GUARD:.3e})")
    assert A.guard_ok(pre) and first == c["seed"]


@pytest.mark.parametrize("tag", list(S.CASES))
def test_split_k_claims_of_the_case_table(tag):
    """fd_gemm_f32.h's split formula on the host: every weight-gradient GEMM over the rows splits at the three split-K cases (4, 5 and
    4 ways) and none does elsewhere."""
    splits = {k: S.gemm_splits(*v) for k, v in S.weight_grad_gemms(tag).items()}
    print(f"split-K {tag}: {splits}")
    want = {"lstm_100": 4, "lstm_72_long": 5, "mlp_rows": 4}.get(tag, 1)
    assert (tag in S.SPLITK_CASES) == (want > 1)
    assert all(s == want for s in splits.values()), splits
    c = S.CASES[tag]
    rows = c["B"] if c["kind"] == "mlp" else c["B"] * c["T"]
    if tag in ("lstm_100", "mlp_rows"):                     # fd_colsum_det: 128-row blocks, a ragged last one
        assert (rows + 127) // 128 == 5 and rows % 128 == {"lstm_100": 64, "mlp_rows": 8}[tag]


@pytest.mark.parametrize("tag", list(S.CASES))
def test_float32_error_of_the_restatement(tag):
    """The same case through the restatement in float32: what float32 arithmetic alone costs, per tensor of its maximum.  At most
    2.5e-6, a quarter of the bound the engine is held to (tests/test_gpu_backbone_grads.py)."""
    e = S.f32_error(tag)
    worst = max(e, key=e.get)
    log_line(f"[f32 floor] {tag}: worst tensor {worst} max|g32 - g64| / max|g64| = {e[worst]:.3e}")
    assert e[worst] <= 2.5e-6, (worst, e[worst])
