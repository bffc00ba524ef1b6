"""GPU parity of k_mega's merged ragged tiles (csrc/fd_mega_kernel.h, RAGGED_MERGE; tests/test_mega_ragged_maps.py holds the
lane maps): series whose last token tile has <= 8 tokens and whose tile count is odd score both heads of a pair in one tile there
-- the last key tile of every unit, and the whole chain of the single-tile units, whose query tile is the ragged one.

  * the ecg static instantiation (T = 100: 6 full tiles + 4 tokens) at the smallest batch plan() still serves with two series
    per workgroup, (3 #CU) // 2 + 1, so that the last workgroup holds one series only: forward against the float64 oracle with the
    bounds of test_gpu_bench_instantiation.py's ecg test (1e-2 max / 7e-3 rms, 1.2e-2 per series), the per-series error taken
    separately over tokens 0..95 and over the four tokens 96..99 of the ragged tile -- a wrong row map shows in the ragged tile and
    would hide in a maximum over a hundred tokens;
  * the same with FDIFF_MEGA_DBG=32, which runs the exact two-pass form of every unit (the merged tile's per-head maxima);
  * one run-time specialised shape with an odd tile count and more than 4 ragged tokens (nasa discharge, (134, 5): 8 full tiles +
    6 tokens, rows [0, 8) / [8, 16) of the merged tile) at the batch and bounds of test_gpu_jit_shapes.py;
  * a 20-step bf16 sampler trajectory at the ecg static shape against the oracle's loop, bounds of
    test_gpu_sampler_parity_shapes.py's static instantiations (1e-2 max / 5e-3 rms of the trajectory scale, 1e-2 per series).
"""
import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O
from oracle import weights as W

from .gpu_util import DEV, log_line, make_model, oracle_sde, report_err
from .test_gpu_bench_instantiation import ECG, ECG_STATIC, _cu_count, _fwd, _rows, _run_sampler

pytestmark = pytest.mark.gpu

_cache = {}


def _ecg_case():
    """inputs, checked rows and the oracle's forward: computed once, shared (read-only) by the cases"""
    if "ecg" not in _cache:
        B = (3 * _cu_count()) // 2 + 1
        m, _, sd = make_model(ECG, precision="bf16")
        name, S = m.plan(B)
        assert ECG_STATIC in name and S == 2, name
        X = W.randn("rg_x_ecg", (B, ECG["T"], ECG["C"]), 2)
        t = W.uniform("rg_t_ecg", (B,), 2, 1e-5, 1.0)
        rows = _rows(B, S)
        assert B - 1 in rows and B % S == 1                # the last workgroup's only series
        ref = O.score_forward(sd, X[rows], t[rows], ECG["H"])
        ref.setflags(write=False)
        _cache["ecg"] = (B, m, X, t, rows, ref, name)
    return _cache["ecg"]


def _check_forward(tag, out, ref, rows, T):
    err, rms = report_err(tag, out[rows], ref)
    k0 = 16 * ((T - 1) // 16)
    worst = [0.0, 0.0]
    for i, r in enumerate(rows):
        scale = np.abs(ref[i]).max()
        e_full = np.abs(out[r][:k0] - ref[i][:k0]).max() / scale
        e_ragged = np.abs(out[r][k0:] - ref[i][k0:]).max() / scale
        worst = [max(worst[0], e_full), max(worst[1], e_ragged)]
        log_line(f"[parity] {tag}: series {r}: tokens 0..{k0 - 1} {e_full:.3e}, tokens {k0}..{T - 1} {e_ragged:.3e}")
    log_line(f"[parity] {tag}: worst per-series error, full tiles {worst[0]:.3e}, ragged tile {worst[1]:.3e}")
    assert err <= 1e-2 and rms <= 7e-3, (err, rms)
    assert worst[0] <= 1.2e-2 and worst[1] <= 1.2e-2, worst
    assert np.isfinite(out).all()


@pytest.mark.parametrize("dbg", [None, "32"])
def test_forward_ecg_static_merged_ragged_tile_vs_oracle(dbg, monkeypatch):
    B, m, X, t, rows, ref, name = _ecg_case()
    if dbg is None:
        monkeypatch.delenv("FDIFF_MEGA_DBG", raising=False)
    else:
        monkeypatch.setenv("FDIFF_MEGA_DBG", dbg)
    out = _fwd(m, X, t)
    _check_forward(f"ragged merge forward bf16 ecg B={B} dbg={dbg or 0}", out, ref, rows, ECG["T"])


def test_forward_specialised_134x5_merged_ragged_tile_vs_oracle(monkeypatch, tmp_path_factory):
    cfg = dict(T=134, C=5, D=72, L=10, H=12)
    B = 2 * _cu_count() - 1
    monkeypatch.setenv("FDIFF_CACHE_DIR", str(tmp_path_factory.getbasetemp() / "fdiff_jit_cache"))
    monkeypatch.setenv("FDIFF_MEGA_JIT", "1")
    monkeypatch.delenv("FDIFF_MEGA_DBG", raising=False)
    m, _, sd = make_model(cfg, precision="bf16")
    desc, S = m.plan(B)
    assert S == 1 and "(hiprtc)" in desc and "ShapeStatic<134,72,5,12,1," in desc, desc
    X = W.randn("rg_x_nasa", (B, cfg["T"], cfg["C"]), 2)
    t = W.uniform("rg_t_nasa", (B,), 2, 1e-5, 1.0)
    out = _fwd(m, X, t)
    rows = _rows(B, S)[:6]
    ref = O.score_forward(sd, X[rows], t[rows], cfg["H"])
    _check_forward(f"ragged merge forward bf16 hiprtc (134, 5) B={B}", out, ref, rows, cfg["T"])


def test_trajectory_ecg_static_merged_ragged_tile_vs_oracle(monkeypatch):
    monkeypatch.delenv("FDIFF_MEGA_DBG", raising=False)
    B = (3 * _cu_count()) // 2 + 1
    N = 20
    kind, p = "vp", (0.1, 20.0)
    m, sch, sd = make_model(ECG, kind=kind, p=p, precision="bf16")
    desc, S = m.plan(B)
    assert ECG_STATIC in desc and S == 2, desc
    g = torch.Generator(device="cpu").manual_seed(17)
    shape = (B, ECG["T"], ECG["C"])
    zp = torch.randn(shape, generator=g)
    zs = torch.randn((N,) + shape, generator=g)
    got = _run_sampler(m, B, N, zp.to(DEV), zs.to(DEV), stepwise=False)
    rows = [0, 1, B - 1]                       # both series of the first workgroup, the last workgroup's only one
    ref, _ = O.sample_trajectory(sd, oracle_sde(kind, p, True, ECG["T"]), zp.numpy()[rows].astype(np.float64),
                                 [z[rows].astype(np.float64) for z in zs.numpy()], ECG["H"])
    err, rms = report_err(f"ragged merge 20-step trajectory bf16 ecg B={B} rows={rows}", got[rows], ref)
    assert err <= 1e-2 and rms <= 5e-3, (err, rms)
    for i, r in enumerate(rows):
        e = np.abs(got[r] - ref[i]).max() / np.abs(ref).max()
        assert e <= 1e-2, (r, e)
    assert np.isfinite(got).all()
