"""CPU: tests/autograd_ref.py (the float64 autograd restatement of the transformer score) pinned to the oracle, and the kink rule
checked on the reference alone, at every case of tests/shapes_ref.py that the GPU tests of input_vjp and DPS guidance use."""
import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W
from tests import autograd_ref as A
from tests import cfg_ref
from tests import dps_ref as R
from tests import likelihood_ref as LR
from tests import ode_ref
from tests import shapes_ref as S
from tests.gpu_util import log_line, oracle_sde

CFG_T8 = dict(T=8, C=3, D=8, L=2, H=4)              # tests/test_gpu_likelihood.py, tests/test_gpu_dps.py
SMALL = {"T8C3": CFG_T8, "T21C3": cfg_ref.CFG_TAIL}
Y = [0, 2, 3]
WG = 1.5


def _inputs(tag, cfg, nb=S.B):
    shape = (nb, cfg["T"], cfg["C"])
    return (W.randn(f"agr_x_{tag}", shape, 0).astype(np.float64), W.uniform(f"agr_t_{tag}", (nb,), 0, 0.05, 1.0),
            W.randn(f"agr_u_{tag}", shape, 1).astype(np.float64), W.randn(f"agr_v_{tag}", shape, 2).astype(np.float64))


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_forward_is_the_oracle_forward(name):
    """Measured: <= 1e-15 of the maximum at every shape."""
    cfg = S.SHAPES[name]
    sd, tab = S.cond_weights(cfg)
    x, t, _, _ = _inputs(name, cfg)
    ref = O.score_forward(sd, x, t, cfg["H"])
    err = float(np.abs(A.score(sd, x, t, cfg["H"]) - ref).max() / np.abs(ref).max())
    refl = cfg_ref.score(sd, tab, x, t, Y, cfg["H"])
    errl = float(np.abs(A.score(sd, x, t, cfg["H"], tab, Y) - refl).max() / np.abs(refl).max())
    refn = cfg_ref.score(sd, tab, x, t, None, cfg["H"])
    guided = A.score(sd, x, t, cfg["H"], tab, Y, WG)
    errg = float(np.abs(guided - (WG * refl + (1.0 - WG) * refn)).max() / np.abs(refl).max())
    print(f"autograd_ref forward {name}: {err:.2e} plain, {errl:.2e} labelled, {errg:.2e} guided, of the maximum")
    assert err <= 1e-12 and errl <= 1e-12 and errg <= 1e-12


@pytest.mark.parametrize("name", list(SMALL))
def test_vjp_elementwise_against_central_differences(name):
    """T C columns of the Jacobian by central differences of the oracle (tests/dps_ref.vjp), plain and guided.  The differences carry a
    truncation and cancellation error of about 1e-8 of the maximum at step 1e-7; 1e-6 bounds it."""
    cfg = SMALL[name]
    tab = cfg_ref.table(cfg["D"])
    sd, _ = cfg_ref.state_dict(cfg, tab)
    x, _, u, _ = _inputs(name, cfg)
    t = float(np.float32(0.4))
    for label, fn, kw in (("plain", ode_ref.model_score(sd, "transformer", cfg["H"]), {}),
                          ("guided", cfg_ref.guided_score_fn(sd, tab, Y, WG, cfg["H"]), dict(tab=tab, y=Y, w=WG))):
        ref = R.vjp(fn, x, t, u)
        got = A.vjp(sd, x, t, u, cfg["H"], **kw)
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"autograd_ref vjp {name} {label}: {err:.2e} of the maximum vs central differences")
        assert err <= 1e-6, (label, err)


# the central difference along v must itself cross no relu kink (one crossing costs it 1e-7 to 1e-5: measured at the plain tags of
# these three shapes); the inputs are chosen so, from the reference's own pre-activations, and the test asserts it
DIR_TAGS = {"mimic": "mimic_b", "default": "default_c", "long": "long_b"}


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_vjp_directional_against_central_differences(name):
    """<J^T u, v> = <u, J v>, J v by one central difference of the oracle score (as tests/test_gpu_likelihood.py's directional test),
    to 1e-8 of |J^T u| |v|.  Measured: 1.8e-11 (long) to 9.4e-11 (ragged)."""
    cfg = S.SHAPES[name]
    sd = S.weights(cfg)
    x, t, u, v = _inputs(DIR_TAGS.get(name, name), cfg)
    d = 1e-7 * max(1.0, float(np.abs(x).max()))               # the step of likelihood_ref.jvp
    lo, hi = A.preacts(sd, x - d * v, t, cfg["H"]), A.preacts(sd, x + d * v, t, cfg["H"])
    assert all(np.array_equal(p > 0, q > 0) for p, q in zip(lo, hi)), "the central difference crosses a kink: choose other inputs"
    got = A.vjp(sd, x, t, u, cfg["H"])
    jv = LR.jvp(lambda z, tt: O.score_forward(sd, z, tt, cfg["H"]), x, t, v)
    lhs, rhs = (got * v).sum(axis=(1, 2)), (u * jv).sum(axis=(1, 2))
    scale = np.linalg.norm(got.reshape(S.B, -1), axis=1) * np.linalg.norm(v.reshape(S.B, -1), axis=1)
    err = float((np.abs(lhs - rhs) / scale).max())
    print(f"autograd_ref vjp {name} directional: {err:.2e} of |J^T u| |v|")
    assert err <= 1e-8, err


@pytest.mark.parametrize("fourier", [True, False])
def test_guidance_with_autograd_vjp_is_the_default_guidance(fourier):
    cfg = CFG_T8
    sd = W.make_state_dict(cfg["C"], cfg["T"], cfg["D"], cfg["L"], seed=1234)
    x, _, _, _ = _inputs("g8", cfg)
    sde = oracle_sde("vp", (0.1, 20.0), True, cfg["T"])
    from tests import cfg_impute_ref as G
    mu, sigma, yn, mk, x0 = G.conditioning(cfg["T"], cfg["C"], S.B, "random", 3, fourier)
    fn = ode_ref.model_score(sd, "transformer", cfg["H"])
    for t in (0.7, 0.05):
        t32 = float(np.float32(t))
        g0, r0, _ = R.guidance(fn, sde, x, t32, x0, mk, sigma, fourier)
        g1, r1, _ = R.guidance(fn, sde, x, t32, x0, mk, sigma, fourier, vjp_fn=A.vjp_fn(sd, cfg["H"]))
        err = float(np.abs(g1 - g0).max() / np.abs(g0).max())
        print(f"dps_ref.guidance autograd vs central differences fourier={fourier} t={t}: {err:.2e}")
        assert err <= 1e-6 and np.array_equal(r0, r1)


# ------------------------------------------------------------------------------------------------------------------ the kink rule
def _record(tag, tau, near):
    log_line(f"[kink] {tag}: tau = {tau:.3e} (4 x the largest float32 - float64 pre-activation difference of the reference), "
             f"{near} units within tau")
    assert near <= A.MAX_FLIPS, (tag, near)


@pytest.mark.parametrize("name", S.VJP_F32)
def test_vjp_cases_have_few_units_near_a_kink(name):
    c = S.vjp_case(name, S.SHAPES[name])
    _record(f"input_vjp {name}", c["tau"], c["near"])


def test_guidance_cases_have_few_units_near_a_kink():
    for name in S.DPS_JAC:
        for t in S.DPS_T:
            c = S.guidance_jac_case(name, t)
            _record(f"dps guidance {name} t={t}", c["tau"], c["near"])
    for name in S.CFG_SHAPES:
        for w in (S.CFG_W, 1.0):
            c = S.guidance_cfg_case(name, True, w)
            _record(f"cfg dps guidance {name} w={w}", c["tau"], c["near"])


@pytest.mark.parametrize("name", ["mimic", "ragged"])
def test_trajectory_steps_have_few_units_near_a_kink(name):
    """On the reference's own states rounded to float32 (the engine's differ from them by rounding)."""
    states = S.traj_reference(name)
    assert np.isfinite(states[-1]).all()
    for i in range(S.TRAJ_STEPS):
        nxt, tau, near, flips, scale = S.traj_step_case(name, i, states[i].astype(np.float32))
        _record(f"dps trajectory {name} {S.TRAJ_SDE[name][0]} step {i}", tau, near)
        assert scale[1] == 0.0 and (scale[[0, 2]] > 0).all()          # the unobserved row takes no guidance
        assert np.abs(nxt - states[i + 1]).max() <= 1e-6 * np.abs(states[i + 1]).max()


def test_a_real_kink_crossing_is_explained_and_nothing_else_is():
    """Moves x across ONE unit's kink in float64 (x_b -> x_b - 2 a_k d_k / |d_k|^2 sends a_k to -a_k to first order; the step is of
    the order of tau, so every smooth change of J^T u is of that order too) and checks that the rule accepts the jump with
    coefficient +-1 -- and rejects the same jump at half its size, a jump along a direction that is no unit's, and a jump in a row
    that has no unit near its kink."""
    name, bound = "ragged", 1e-5
    cfg = S.SHAPES[name]
    sd = S.weights(cfg)
    c = S.vjp_case(name, cfg)
    x, t, u, ref = c["x"].astype(np.float64), c["t"], c["u"], c["ref"]
    flips = c["flips"]()
    assert 2 <= len(flips) <= A.MAX_FLIPS
    size = [abs(f["g"]) * np.abs(f["d"]).max() for f in flips]
    k = int(np.argmax(size))
    f = flips[k]
    assert size[k] > 10 * bound * np.abs(ref).max(), "the largest candidate jump is too small to test the rule with"
    x2 = x.copy()
    x2[f["b"]] -= 2.0 * f["a"] * f["d"] / (f["d"] ** 2).sum()
    moved = A.vjp(sd, x2, t, u, cfg["H"])
    ok, plain, left, fits = A.explained_by_flips(moved, ref, flips, bound)
    print(f"kink crossing {name}: unit {k} of {len(flips)}, a = {f['a']:.2e}; plain {plain:.2e}, after flips {left:.2e}, fitted {fits}")
    assert plain > bound and ok and left <= bound
    assert sorted(abs(round(cf)) for _, cf in fits).count(1) == 1       # one unit flipped, the others fitted to 0
    jump = moved - ref
    assert not A.explained_by_flips(ref + 0.5 * jump, ref, flips, bound)[0]           # half a flip is no flip
    noise = np.zeros_like(ref)
    noise[f["b"]] = W.randn("agr_kink_noise", ref.shape[1:], 0) * np.abs(jump).max()
    assert not A.explained_by_flips(ref + noise, ref, flips, bound)[0]                # not along any unit's direction
    other = [b for b in range(S.B) if all(g["b"] != b for g in flips)]
    if other:
        wrong = ref.copy()
        wrong[other[0]] += jump[f["b"]]
        assert not A.explained_by_flips(wrong, ref, flips, bound)[0]                  # a row without a unit near its kink


# ------------------------------------------------------------------------------------------------------------------ bf16 tiles
@pytest.mark.parametrize("tag", list(S.VJP_BF16))
def test_bf16_cases_have_no_hollow_tile(tag):
    """Every (series, 16-step time tile) of the reference carries at least a quarter of the whole tensor's rms (measured: 0.56 to
    1.55), so the per-tile bound of tests/test_gpu_vjp_shapes.py excludes nothing."""
    cfg, nb = S.VJP_BF16[tag]
    ref = S.vjp_case(f"bf16_{tag}", cfg, nb, flips=False)["ref"]
    whole = np.sqrt((ref ** 2).mean())
    ratios = [np.sqrt((ref[b, t0:t0 + 16] ** 2).mean()) / whole for b in range(nb) for t0 in range(0, cfg["T"], 16)]
    print(f"bf16 vjp {tag}: tile rms / whole between {min(ratios):.2f} and {max(ratios):.2f}")
    assert min(ratios) >= 0.25
