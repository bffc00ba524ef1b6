"""Float64 restatement of the adaptive ODE sampler / encoder (DiffusionSampler.sample_ode_adaptive / encode_adaptive /
decode_adaptive, csrc/fd_ode_adaptive.hip): every row is one ODE on its T*C values, dx/dt = v(x, t) (tests/ode_ref.py), under the
Dormand-Prince controller of tests/rk45_ref.py.  rk45_ref.rk45 integrates upward only, so the backward direction (1 -> eps) runs it
on the mirrored ODE, tau = -t, fun(tau, y) = -v(y, -tau), from -t0 to -t1: negation is exact in floating point, so that is scipy's
direction = -1 bit for bit (tests/test_ode_adaptive_cpu.py checks it against scipy.integrate.solve_ivp).  numpy only; shared with
tests/test_gpu_ode_adaptive.py."""
import numpy as np

from tests import ode_ref as R
from tests import rk45_ref as K


def row_velocity(sde, score_fn, T, C, round32=False):
    """v(t, y) of one row, y (T*C,).  round32: the score's input and output rounded to float32 (the sensitivity experiment: what
    rounding at the network's boundary alone does to a fixture)."""
    def fun(t, y):
        x = y.reshape(1, T, C)
        if round32:
            xs = x.astype(np.float32).astype(np.float64)
            s = np.asarray(score_fn(xs, t), dtype=np.float64).astype(np.float32).astype(np.float64)
        else:
            s = score_fn(x, t)
        return R.velocity(sde, s, t, x).ravel()
    return fun


def integrate(sde, score_fn, x0, t0, t1, rtol, atol, max_evals=None, round32=False):
    """Per row of x0 (B,T,C): rk45_ref.rk45's dict with t in the ODE's own time (t0 first), y (T,C), n_reject."""
    x0 = np.asarray(x0, dtype=np.float64)
    Bn, T, C = x0.shape
    v = row_velocity(sde, score_fn, T, C, round32)
    out = []
    for b in range(Bn):
        if t1 > t0:
            r = K.rk45(v, t0, x0[b].ravel(), t1, rtol, atol, max_evals)
        else:
            r = K.rk45(lambda tau, y: -v(-tau, y), -t0, x0[b].ravel(), -t1, rtol, atol, max_evals)
            r["t"] = -r["t"]
        r["y"] = r["y"].reshape(T, C)
        r["n_reject"] = sum(en >= 1 for en in r["err_norms"])
        out.append(r)
    return out


def on_grid(sde, score_fn, x0, grids):
    """The fixed-step Dormand-Prince solution of every row of x0 (B,T,C) on its grid (grids (B, S), NaN padding dropped; either
    direction): (B,T,C)."""
    x0 = np.asarray(x0, dtype=np.float64)
    Bn, T, C = x0.shape
    v = row_velocity(sde, score_fn, T, C)
    out = np.empty_like(x0)
    for b in range(Bn):
        ts = np.asarray(grids[b], dtype=np.float64)
        out[b] = K.dp_fixed(v, ts[~np.isnan(ts)], x0[b].ravel()).reshape(T, C)
    return out


def sensitivity(sde, score_fn, x0, t0, t1, rtol, atol, rows=None):
    """The float32 sensitivity of a fixture: (rows of the plain integration, max grid shift, max result shift of scale
    max(1, |y|max)) between the integration and the same with the score's input and output rounded to float32.  AssertionError when
    the rounding changes a row's nfe (no fixture then)."""
    rows = integrate(sde, score_fn, x0, t0, t1, rtol, atol) if rows is None else rows
    r32 = integrate(sde, score_fn, x0, t0, t1, rtol, atol, round32=True)
    dt = dy = 0.0
    for a, b in zip(rows, r32):
        assert a["nfe"] == b["nfe"] and a["t"].shape == b["t"].shape, (a["nfe"], b["nfe"])
        dt = max(dt, float(np.abs(a["t"] - b["t"]).max()))
        dy = max(dy, float(np.abs(a["y"] - b["y"]).max() / max(1.0, np.abs(a["y"]).max())))
    return rows, dt, dy


CFG_T20 = dict(T=20, C=3, D=8, L=2, H=4)
GOLDEN = "ode_adaptive_tight.npz"      # under tests/golden/


def tight_reference():
    """(latents (3,T,C) float32, run): the first fixture of tests/test_gpu_ode_adaptive.py -- CFG_T20, VP (0.1, 20), the prior of
    the draws "rks_z_vp" as float32 -- and run(rows) -> the float64 restatement of those rows (default: all) at rtol = atol = 1e-10
    from t = 1 to 1e-5 (7346 to 9476 evaluations a row, 25 s of CPU: kept on file with its input; `python -m tests.ode_adaptive_ref`
    writes it, tests/test_ode_adaptive_cpu.py recomputes its first row)."""
    from oracle import fdiff_oracle as O
    from oracle import weights as W
    cfg = CFG_T20
    sde = O.SDEParams("vp", 0.1, 20.0, O.noise_scaling(cfg["T"], True))
    lat = O.prior_sampling(sde, W.randn("rks_z_vp", (3, cfg["T"], cfg["C"]), 0)).astype(np.float32)
    score = R.model_score(W.make_state_dict(cfg["C"], cfg["T"], cfg["D"], cfg["L"], seed=1234), "transformer", cfg["H"])
    return lat, lambda rows=slice(None): np.stack([r["y"] for r in integrate(sde, score, lat[rows].astype(np.float64), 1.0, 1e-5, 1e-10,
                                                                            1e-10)])


if __name__ == "__main__":
    import os
    _lat, _run = tight_reference()
    _path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    np.savez(_path, latents=_lat, x=_run())
    print(f"wrote {_path}")
