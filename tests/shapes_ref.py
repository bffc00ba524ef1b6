"""The dataset-shaped cases of tests/test_gpu_vjp_shapes.py and tests/test_gpu_dps_shapes.py with their float64 references
(tests/autograd_ref.py, tests/dps_ref.py), each computed once and cached at module level, and never changed afterwards.
tests/test_autograd_ref_cpu.py runs the same cases on the CPU to check that the reference alone keeps every case within the kink rule's
limits (at most autograd_ref.MAX_FLIPS units within tau).

Shapes (d_model 72, 12 heads, 2 layers unless said; B = 3): the smallest that cross each boundary of csrc/fd_dps.hip and the VJP.

    mimic     T=24,  C=40   three channel blocks, the last with 8 channels; Tp = 32
    ragged    T=130, C=17   Tp = 144 = 9 row tiles on 8 waves; the second block holds ONE channel; Nyquist row at 65; T C % 4 != 0
    default   T=100, C=12   10 layers: full depth, the persistent training forward in bf16
    droughts  T=365, C=13   odd T (no Nyquist row), 23 tiles, the per-layer forward
    long      T=1024, C=20  128 KiB dynamic + 4 KiB static LDS, two blocks (Jacobian-free only)
    d64_h8    T=100, C=12   d_model 64, 8 heads, 3 layers: head_dim 8
"""
import numpy as np

from oracle import weights as W
from tests import autograd_ref as A
from tests import cfg_impute_ref as G
from tests import cfg_ref
from tests import dps_ref as R
from tests import ode_ref
from tests.gpu_util import oracle_sde

B = 3
VP = ("vp", (0.1, 20.0))
SHAPES = {
    "mimic": dict(T=24, C=40, D=72, L=2, H=12),
    "ragged": dict(T=130, C=17, D=72, L=2, H=12),
    "default": dict(T=100, C=12, D=72, L=10, H=12),
    "droughts": dict(T=365, C=13, D=72, L=2, H=12),
    "long": dict(T=1024, C=20, D=72, L=2, H=12),
    "d64_h8": dict(T=100, C=12, D=64, L=3, H=8),
}
DEFAULT_L2 = dict(SHAPES["default"], L=2)
VJP_F32 = ["mimic", "ragged", "default", "droughts", "d64_h8"]
# bf16 VJP: shapes that tests/test_gpu_train_bf16.py and tests/test_gpu_widths.py train in bf16
VJP_BF16 = {
    "default_B1": (SHAPES["default"], 1), "default_B3": (SHAPES["default"], 3), "default_B16": (SHAPES["default"], 16),
    "T252C5": (dict(T=252, C=5, D=72, L=2, H=12), 3), "T365C3": (dict(T=365, C=3, D=72, L=2, H=12), 3),
    "d64_h8": (SHAPES["d64_h8"], 3), "d32_h4": (dict(T=48, C=3, D=32, L=2, H=4), 3),
}
DPS_T = (0.7, 0.05)
DPS_JAC = {"mimic": SHAPES["mimic"], "ragged": SHAPES["ragged"], "default": DEFAULT_L2, "droughts": SHAPES["droughts"]}
CFG_SHAPES = ["mimic", "ragged"]
CFG_W = 1.5
CFG_Y = [0, 2, 3]            # one null row (K = 3)
CFG_T = 0.3
TRAJ_STEPS = 4
TRAJ_ZETA = 0.3
VE = ("ve", (0.01, 2.0))
# four VP steps grow the state 30-fold; the float32 yardstick tau grows with it, and at (130, 17) more than 100 units lie within it at
# the last step.  The VE state stays put, so the larger shape runs VE and the smaller one VP.
TRAJ_SDE = {"mimic": VP, "ragged": VE}

# Input tags: chosen so that the float64 reference ALONE has at most autograd_ref.MAX_FLIPS units within tau in every case (checked
# by tests/test_autograd_ref_cpu.py); nothing measured on the engine enters the choice.  A case not listed uses its plain name.
TAGS = {"vjp_default": "default_24", "vjp_droughts": "droughts_96", "dps_droughts_0.7": "droughts_0.7_3",
        "dps_droughts_0.05": "droughts_0.05_0", "dps_ragged_0.3": "ragged_0.3_2"}

_CACHE = {}


class _Once:
    """A value computed at its first call: the flip directions take one backward pass per unit and are needed only where a
    comparison misses its plain bound."""

    def __init__(self, make):
        self.make, self.done = make, False

    def __call__(self):
        if not self.done:
            self.value, self.done = self.make(), True
        return self.value


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def cfg_key(cfg):
    return tuple(sorted(cfg.items()))


def weights(cfg):
    """The state dict tests/gpu_util.make_model loads (seed 1234), one object per configuration."""
    return _cached(("sd", cfg_key(cfg)), lambda: W.make_state_dict(cfg["C"], cfg["T"], cfg["D"], cfg["L"], seed=1234))


def cond_weights(cfg):
    """(sd, tab) of tests/test_gpu_cfg.make_cond."""
    def make():
        tab = cfg_ref.table(cfg["D"])
        return cfg_ref.state_dict(cfg, tab)[0], tab
    return _cached(("csd", cfg_key(cfg)), make)


# ------------------------------------------------------------------------------------------------------------------ input_vjp
def vjp_inputs(tag, cfg, nb):
    shape = (nb, cfg["T"], cfg["C"])
    return (W.randn(f"shp_vx_{tag}", shape, 0), W.uniform(f"shp_vt_{tag}", (nb,), 0, 0.05, 1.0), W.randn(f"shp_vu_{tag}", shape, 1))


def vjp_case(tag, cfg, nb=B, flips=True):
    """dict(x, t, u, ref = J^T u in float64, tau, near = the number of units within tau, flips = a function that returns
    autograd_ref.relu_flips) of one input_vjp comparison."""
    def make():
        sd = weights(cfg)
        x, t, u = vjp_inputs(TAGS.get(f"vjp_{tag}", tag), cfg, nb)
        out = dict(x=x, t=t, u=u, ref=A.vjp(sd, x, t, u, cfg["H"]))
        if flips:
            out["tau"] = A.tau_of(sd, x, t, cfg["H"])
            out["near"] = A.near_kink(sd, x, t, cfg["H"], out["tau"])
            out["flips"] = _Once(lambda: A.relu_flips(sd, x, t, u, cfg["H"], out["tau"]))
        return out
    return _cached(("vjp", tag, cfg_key(cfg), nb, flips), make)


# ------------------------------------------------------------------------------------------------------------------ guidance
def dps_x(name, cfg, t):
    return W.randn("shp_gx_" + TAGS.get(f"dps_{name}_{t}", f"{name}_{t}"), (B, cfg["T"], cfg["C"]), 0)


def conditioning(name, cfg, fourier, std_given, mask_kind):
    """(mu, sigma, observations, mask, x0_obs): tests/cfg_impute_ref.conditioning ("random": per series (B,T,C); "forecast": one
    shared (T,C) mask); feature_std None = no standardisation (sigma = 1)."""
    return _cached(("cond", name, fourier, std_given, mask_kind),
                   lambda: G.conditioning(cfg["T"], cfg["C"], B, mask_kind, 41, fourier, standardize=std_given))


def oracle_score(name, cfg, t):
    """The oracle's own score at the case's x (one evaluation per (shape, t), shared by every option of the Jacobian-free cases)."""
    return _cached(("score", name, cfg_key(cfg), t),
                   lambda: ode_ref.model_score(weights(cfg), "transformer", cfg["H"])(dps_x(name, cfg, t).astype(np.float64),
                                                                                       float(np.float32(t))))


def guidance_free_case(name, t, fourier, std_given, mask_kind):
    """(g, ||r||^2) of dps_ref.guidance(jacobian=False) on the oracle score."""
    cfg = SHAPES[name]

    def make():
        mu, sigma, yn, mk, x0 = conditioning(name, cfg, fourier, std_given, mask_kind)
        sde = oracle_sde("vp", VP[1], True, cfg["T"])
        g, rn2, _ = R.guidance(None, sde, dps_x(name, cfg, t), float(np.float32(t)), x0, mk, sigma, fourier, jacobian=False,
                               score=oracle_score(name, cfg, t))
        return g, rn2
    return _cached(("gfree", name, t, fourier, std_given, mask_kind), make)


def _flip_case(sd, cfg, x, t32, x0, mk, sigma, fourier, tab=None, y=None, w=None, sde=VP):
    """Reference guidance with the Jacobian by autograd, and the units near a kink: the VJP's cotangent is v = s^2 G^2 u, and a flip
    moves g = (2 / alpha) (u + J^T v) by +- (2 / alpha) g_k d_k."""
    sde = oracle_sde(*sde, True, cfg["T"])
    sfn, vfn = A.score_fn(sd, cfg["H"], tab, y, w), A.vjp_fn(sd, cfg["H"], tab, y, w)
    g, rn2, score = R.guidance(sfn, sde, x, t32, x0, mk, sigma, fourier, jacobian=True, vjp_fn=vfn)
    alpha, s = R.coef(sde, t32)
    _, u = R.residual(x, score, x0, mk, sigma, sde.G, alpha, s, fourier)
    v = (s * s) * (sde.G ** 2)[None, :, None] * u
    tb = np.full((x.shape[0],), t32, dtype=np.float32)
    tau = A.tau_of(sd, x, tb, cfg["H"], tab, y, w)
    near = A.near_kink(sd, x, tb, cfg["H"], tau, tab, y, w)
    flips = _Once(lambda: A.relu_flips(sd, x, tb, v, cfg["H"], tau, tab, y, w))
    return dict(g=g, rn2=rn2, tau=tau, near=near, flips=flips, scale=np.full((x.shape[0],), 2.0 / alpha))


def guidance_jac_case(name, t):
    cfg = DPS_JAC[name]

    def make():
        mu, sigma, yn, mk, x0 = conditioning(name, cfg, True, True, "random")
        return _flip_case(weights(cfg), cfg, dps_x(name, cfg, t).astype(np.float64), float(np.float32(t)), x0, mk, sigma, True)
    return _cached(("gjac", name, t), make)


def guidance_cfg_case(name, jac, w=CFG_W):
    """impute_guidance(y = CFG_Y, cfg_scale = w) on the K = 3 model at t = CFG_T."""
    cfg = SHAPES[name]

    def make():
        sd, tab = cond_weights(cfg)
        mu, sigma, yn, mk, x0 = conditioning(name, cfg, True, True, "random")
        x, t32 = dps_x(name, cfg, CFG_T).astype(np.float64), float(np.float32(CFG_T))
        if jac:
            return _flip_case(sd, cfg, x, t32, x0, mk, sigma, True, tab, CFG_Y, w)
        sde = oracle_sde("vp", VP[1], True, cfg["T"])
        g, rn2, _ = R.guidance(A.score_fn(sd, cfg["H"], tab, CFG_Y, w), sde, x, t32, x0, mk, sigma, True, jacobian=False)
        return dict(g=g, rn2=rn2)
    return _cached(("gcfg", name, jac, w), make)


# ------------------------------------------------------------------------------------------------------------------ trajectories
def traj_inputs(name):
    """Conditioning with row 1's mask entirely false (its ||r|| is 0: the row takes the plain reverse-SDE steps), prior and
    predictor noise."""
    cfg = SHAPES[name]

    def make():
        T, Cn = cfg["T"], cfg["C"]
        rs = np.random.RandomState(43)
        mu = (0.3 * rs.randn(T, Cn)).astype(np.float32).astype(np.float64)
        sigma = rs.uniform(0.5, 2.0, (T, Cn)).astype(np.float32).astype(np.float64)
        y = (np.sin(np.linspace(0, 6, T))[None, :, None] + 0.3 * rs.randn(B, T, Cn)).astype(np.float32)
        mk = rs.rand(B, T, Cn) < 0.5
        mk[1] = False
        yn = np.where(mk, y, np.nan).astype(np.float32)
        from tests import impute_ref as I
        x0 = I.x0_obs(yn, mk, mu, sigma, True)
        zp = W.randn(f"shp_tp_{name}", (B, T, Cn), 1)
        zs = np.stack([W.randn(f"shp_tz{i}_{name}", (B, T, Cn), 1) for i in range(TRAJ_STEPS)])
        return dict(mu=mu, sigma=sigma, yn=yn, mk=mk, x0=x0, zp=zp, zs=zs)
    return _cached(("traj_in", name), make)


def traj_reference(name):
    """The float64 trajectory with the Jacobian (autograd VJP) and its states X_0 .. X_N."""
    cfg = SHAPES[name]

    def make():
        from oracle import fdiff_oracle as O
        d = traj_inputs(name)
        sd = weights(cfg)
        sde = oracle_sde(*TRAJ_SDE[name], True, cfg["T"])
        ts, dt = O.timesteps(TRAJ_STEPS)
        X = O.prior_sampling(sde, d["zp"])
        states = [X]
        for i, t in enumerate(ts):
            X = R.step(A.score_fn(sd, cfg["H"]), sde, X, t, dt, d["zs"][i], d["x0"], d["mk"], d["sigma"], True, TRAJ_ZETA, True,
                       A.vjp_fn(sd, cfg["H"]))
            states.append(X)
        return states
    return _cached(("traj_ref", name), make)


def traj_step_case(name, i, X):
    """One reference step from the state X (float64 copy of the engine's X_i): (X_{i+1}, tau, near, flips, scale), scale = the
    (zeta / ||r||) (2 / alpha) that multiplies g_k d_k in row b of the step."""
    from oracle import fdiff_oracle as O
    cfg = SHAPES[name]
    d = traj_inputs(name)
    sd = weights(cfg)
    sde = oracle_sde(*TRAJ_SDE[name], True, cfg["T"])
    ts, dt = O.timesteps(TRAJ_STEPS)
    t = float(ts[i])
    X = np.asarray(X, dtype=np.float64)
    c = _flip_case(sd, cfg, X, t, d["x0"], d["mk"], d["sigma"], True, sde=TRAJ_SDE[name])
    nr = np.sqrt(c["rn2"])
    coef = np.where(nr > 0, TRAJ_ZETA / np.where(nr > 0, nr, 1.0), 0.0)
    score = A.score(sd, X, t, cfg["H"])
    nxt = O.sde_step(sde, score, t, X, d["zs"][i], float(dt)) + coef[:, None, None] * c["g"]
    return nxt, c["tau"], c["near"], c["flips"], coef * c["scale"]
