"""CPU: the float64 restatement of the post-hoc scores (tests/posthoc_ref.py) is pinned on its own -- the heads' gradients against
central differences, the conventions at the kinks, the index rule's range -- and it LEARNS: on AR(1) against white noise it meets the
four conditions the GPU test (tests/test_gpu_posthoc.py) asks of the engine, with margin.  Plus the argument checks of
utils/posthoc.py that need no GPU."""
import numpy as np
import pytest
import torch

from oracle import weights as W
from tests import posthoc_ref as R

SEEDS = (0, 1, 2, 3, 4)
LEARN = dict(T=24, C=2, n=640, D=16, L=1, steps=200, B=128, lr=1e-2)


def _case(task, B, T, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, C))
    out = rng.standard_normal((B, T, C))
    if task == "predict":       # no |diff| within 1e-3 of 0: the L1 kink stays away from the central differences
        diff = out[:, :-1] - x[:, 1:]
        out[:, :-1] += np.where(np.abs(diff) < 1e-2, np.where(diff >= 0, 2e-2, -2e-2), 0.0)
        assert np.abs(out[:, :-1] - x[:, 1:]).min() > 1e-3
    label = (np.arange(B) % 2).astype(np.float64)
    return out, x, label


@pytest.mark.parametrize("task", ["predict", "classify"])
@pytest.mark.parametrize("B,T,C", [(3, 5, 1), (5, 17, 3), (4, 2, 1)])
def test_head_gradients_match_central_differences(task, B, T, C):
    out, x, label = _case(task, B, T, C, 11)
    g = R.head_with_grad(task, out, x, label)
    h = 1e-6
    num = np.zeros_like(out)
    for i in np.ndindex(*out.shape):
        up, dn = out.copy(), out.copy()
        up[i] += h
        dn[i] -= h
        num[i] = (R.head_with_grad(task, up, x, label)["loss"] - R.head_with_grad(task, dn, x, label)["loss"]) / (2 * h)
    np.testing.assert_allclose(g["dout"], num, atol=1e-8)


def test_kinks_and_exact_zeros():
    out, x, label = _case("predict", 4, 6, 2, 3)
    out[1, 2, 0] = x[1, 3, 0]                                # a zero difference
    g = R.head_with_grad("predict", out, x)
    assert g["dout"][1, 2, 0] == 0.0                        # sign(0) = 0
    assert np.all(g["dout"][:, -1] == 0.0)                  # nothing forecasts beyond the series
    live = np.ones(out.shape, dtype=bool)
    live[:, -1] = False
    live[1, 2, 0] = False
    assert np.all(np.abs(g["dout"][live]) == 1.0 / (4 * 5 * 2))
    np.testing.assert_allclose(g["per_series"].sum() / (4 * 5 * 2), g["loss"], rtol=1e-14)
    c = R.head_with_grad("classify", out, None, label)
    assert np.all(c["dout"][:, :-1] == 0.0)
    logit = out[:, -1].mean(axis=1)
    np.testing.assert_allclose(c["per_series"], logit, rtol=1e-14)
    np.testing.assert_allclose(c["dout"][:, -1, 0], (1.0 / (1.0 + np.exp(-logit)) - label) / (4 * 2), rtol=1e-12)


def test_softplus_is_finite_at_large_logits():
    for v, y, want in ((100.0, 0.0, 100.0), (100.0, 1.0, 0.0), (-100.0, 0.0, 0.0), (-100.0, 1.0, 100.0)):
        out = np.full((1, 3, 2), v)
        g = R.head_with_grad("classify", out, None, np.array([y]))
        assert np.isfinite(g["loss"]) and np.all(np.isfinite(g["dout"]))
        assert abs(g["loss"] - want) < 1e-12


@pytest.mark.parametrize("n", [1, 7, 100003])
def test_index_rule_stays_in_range(n):
    seen = []
    for step in range(40):
        idx, label = R.step_indices(99, 5, step, 130, n, n + 3)
        assert idx.shape == (130,) and idx.min() >= 0
        assert np.all(idx[:65] < n) and np.all(idx[65:] < n + 3)
        assert np.all(label[:65] == 1) and np.all(label[65:] == 0)
        seen.append(idx)
    words = np.array([[0, 0xFFFFFFFF, 0x80000000, 1]], dtype=np.uint32)
    idx, label = R.indices_from_words(words, 4, n)
    assert list(idx) == [0, n - 1, n // 2, 0] and list(label) == [1, 1, 1, 1]
    if n > 1:
        assert len(np.unique(np.stack(seen))) > 1
        assert not np.array_equal(seen[0], seen[1])           # another step, another counter window


def _state_dict(seed):
    c = LEARN
    return W.make_state_dict_backbone("lstm", c["C"], c["T"], c["D"], c["L"], seed=1000 + seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_learns_the_discriminative_score(seed):
    c = LEARN
    real = R.ar1(c["n"], c["T"], c["C"], 10 * seed + 1)
    apart = R.discriminative_score(_state_dict(seed), real, R.noise(c["n"], c["T"], c["C"], 10 * seed + 2), seed, c["steps"], c["B"], c["lr"])
    alike = R.discriminative_score(_state_dict(seed), real, R.ar1(c["n"], c["T"], c["C"], 10 * seed + 3), seed, c["steps"], c["B"], c["lr"])
    print(f"[posthoc ref] seed {seed}: AR against noise {apart:.3f}, AR against AR {alike:.3f}")
    assert apart >= 0.40
    assert alike <= 0.15


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_learns_the_predictive_score(seed):
    c = LEARN
    real = R.ar1(c["n"], c["T"], c["C"], 10 * seed + 1)
    good = R.predictive_score(_state_dict(seed), R.ar1(c["n"], c["T"], c["C"], 10 * seed + 3), real, seed, c["steps"], c["B"], c["lr"])
    bad = R.predictive_score(_state_dict(seed), R.noise(c["n"], c["T"], c["C"], 10 * seed + 2), real, seed, c["steps"], c["B"], c["lr"])
    print(f"[posthoc ref] seed {seed}: MAE trained on AR {good:.3f}, trained on noise {bad:.3f}")
    assert good <= 0.40          # the floor is 0.798 sqrt(1 - 0.81) = 0.348
    assert bad >= 0.65           # predicting zero gives 0.798


def test_float32_restatement_tracks_float64():
    """The yardstick behind the drift bound of the GPU test is usable: the same 20 steps in float32 and in float64 agree to four
    digits (a sanity check of the restatement's dtype switch, not a tolerance on the engine) and the loss goes down."""
    c = LEARN
    sd = _state_dict(0)
    a, b = R.ar1(64, c["T"], c["C"], 1), R.noise(64, c["T"], c["C"], 2)
    mean, inv = R.stats(a)
    for task in ("classify", "predict"):
        trace = R.index_trace(7, 20, 32, 64, 64 if task == "classify" else None)
        r64 = R.fit(task, sd, a, b, mean, inv, trace, 1e-2)
        r32 = R.fit(task, sd, a, b, mean, inv, trace, 1e-2, dtype=torch.float32)
        assert np.abs(r64["loss"] - r32["loss"]).max() < 1e-4
        assert r64["loss"][-1] < r64["loss"][0]


# ------------------------------------------------------------------------------------------------ utils/posthoc.py without a GPU
@pytest.mark.parametrize("d_model", [101, 33, 128, 0])
def test_network_refuses_a_width_the_engine_does_not_train(d_model):
    from fourierdiffusion_amd.utils.posthoc import PosthocNetwork
    with pytest.raises(ValueError, match="d_model"):
        PosthocNetwork(2, 24, d_model=d_model)
    if d_model > 1:
        with pytest.raises(ValueError, match="<= 100"):
            PosthocNetwork(2, 24, d_model=d_model)


def test_scores_refuse_bad_arguments():
    from fourierdiffusion_amd.utils import posthoc as P
    x = np.zeros((8, 24, 2), dtype=np.float32)
    with pytest.raises(ValueError, match=r"\(n, T, C\)"):
        P.discriminative_score(x.reshape(8, 48), x, seed=0)
    with pytest.raises(ValueError, match="expected"):
        P.discriminative_score(x, x[:, :12], seed=0)
    with pytest.raises(ValueError, match="test_fraction"):
        P.discriminative_score(x, x, seed=0, test_fraction=1.0)
    with pytest.raises(ValueError, match="at least 2 points"):
        P.predictive_score(x[:, :1], x[:, :1], stats_from=x[:, :1], seed=0)
    with pytest.raises(ValueError, match="task"):
        P._task("regress")


def test_channel_stats_are_float64_moments():
    from fourierdiffusion_amd.utils.posthoc import channel_stats, standardise
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((50, 7, 3)) * np.array([1.0, 10.0, 0.0]) + np.array([1000.0, -3.0, 5.0])).astype(np.float32)
    mean, inv = channel_stats(x)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(mean.numpy(), x64.mean(axis=(0, 1)), rtol=1e-7)
    np.testing.assert_allclose(inv.numpy()[:2], 1.0 / x64.std(axis=(0, 1))[:2], rtol=1e-6)
    assert inv[2] == 1.0                                     # a constant channel is left at its scale
    rm, ri = R.stats(x)
    np.testing.assert_array_equal(mean.numpy(), rm)
    np.testing.assert_array_equal(inv.numpy(), ri)
    z = standardise(torch.from_numpy(x), mean, inv).numpy()
    np.testing.assert_array_equal(z, R.gather(x, None, np.arange(50), np.ones(50), mean.numpy(), inv.numpy()))
