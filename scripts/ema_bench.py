#!/usr/bin/env python3
"""What the weight average costs (fd_adamw_ema_step), at the default model's parameter count for the two training
shapes of `bench.py --mode train` (T = 100, C = 12 and T = 252, C = 6; d_model = 72, L = 10, H = 12):

  (a) fd_adamw_step of this build -- and of another build of the library (`--parent-lib PATH`, the parent commit's) beside it;
  (b) fd_adamw_ema_step;
  (c) the unfused alternative: fd_adamw_step, then `ema.lerp_(p, 1 - d)` on the shadow (a second launch);
  (d) the whole optimizer step of the training loop (zero_grad, forward + backward, clip + AdamW; B = 64, bf16) with and without
      `ema_decay`.

(a)-(c): device events around `--calls` back-to-back calls (clipping on, as the trainer runs it), the variants alternated `--reps`
times, the median and the spread reported, and the GB/s the algorithmic traffic (28 / 36 / 40 B per parameter) amounts to.
(d): a host clock around `--steps` steps ending in a synchronise, alternated `--train-reps` times.  The shader clock the context
measured at start-up is recorded.  One JSON line per shape; `--out FILE` also writes them as a JSON list."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

D, L, H = 72, 10, 12
SHAPES = {"ecg_T100_C12": (100, 12), "nasdaq_T252_C6": (252, 6)}
HP = (0.9, 0.999, 1e-8, 1e-2)


def make_model(T, Cn):
    from fourierdiffusion_amd.models.score_models import ScoreModule
    from fourierdiffusion_amd.schedulers.sde import VPScheduler
    sch = VPScheduler(beta_min=0.1, beta_max=20.0, fourier_noise_scaling=True)
    sch.set_noise_scaling(T)
    return ScoreModule(n_channels=Cn, max_len=T, noise_scheduler=sch, fourier_noise_scaling=True, d_model=D, num_layers=L, n_head=H)


def load_other(path):
    """A second build of the library with its own context (only the optimizer entry points are bound)."""
    from fourierdiffusion_amd import _C
    lib = C.CDLL(path)
    for name in ("fd_ctx_create", "fd_grad_sqnorm", "fd_adamw_step"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _C._PROTOS[name]
    h = C.c_void_p()
    assert lib.fd_ctx_create(torch.cuda.current_device(), C.byref(h)) == 0
    return lib, h


def kernel_rows(n, frozen, calls, reps, parent_lib):
    from fourierdiffusion_amd import _C
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, h = _C.lib(), _C.ctx(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    p0 = torch.randn(n, generator=g).to(dev)
    grad = (torch.randn(n, generator=g) * 1e-2).to(dev)
    sq = torch.zeros(1, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    state = {}

    def fresh(tag):
        state[tag] = dict(p=p0.clone(), m=torch.zeros_like(p0), v=torch.zeros_like(p0), e=p0.clone(), step=0)
        return state[tag]

    def plain(tag, L_, h_):
        s = state[tag]
        s["step"] += 1
        rc = L_.fd_adamw_step(h_, s["p"].data_ptr(), grad.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), n, s["step"], 1e-4, *HP,
                              sq.data_ptr(), 1.0, 1.0, frozen[0], frozen[1], stream)
        assert rc == 0, rc

    def fused(tag):
        s = state[tag]
        s["step"] += 1
        _C.check(lib.fd_adamw_ema_step(h, s["p"].data_ptr(), grad.data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), s["e"].data_ptr(),
                                       0.9999, n, s["step"], 1e-4, *HP, sq.data_ptr(), 1.0, 1.0, frozen[0], frozen[1], stream), h)

    def unfused(tag):
        plain(tag, lib, h)
        state[tag]["e"].lerp_(state[tag]["p"], 1.0 - 0.9999)

    _C.check(lib.fd_grad_sqnorm(h, grad.data_ptr(), n, sq.data_ptr(), stream), h)
    variants = {"adamw": lambda: plain("adamw", lib, h), "adamw_ema_fused": lambda: fused("adamw_ema_fused"),
                "adamw_then_lerp": lambda: unfused("adamw_then_lerp")}
    if parent_lib:
        pl, ph = load_other(parent_lib)
        variants["adamw_parent"] = lambda: plain("adamw_parent", pl, ph)
    for k in variants:
        fresh(k)
    for fn in variants.values():                                # warm-up: code objects, allocator
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):                                       # alternate the variants
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            times[k].append(1e3 * a.elapsed_time(b) / calls)    # us per call
    torch.cuda.synchronize()
    # the same update whether the average rides along or not (the timed state itself, after reps * calls + 20 steps)
    same = all(torch.equal(state["adamw"][x], state["adamw_ema_fused"][x]) for x in "pmv")
    bytes_per = {"adamw": 28, "adamw_parent": 28, "adamw_ema_fused": 36, "adamw_then_lerp": 40}
    rec = {"ema_leaves_update_bit_identical": bool(same)}
    for k, ts in times.items():
        med = statistics.median(ts)
        rec[k] = {"us_median": round(med, 3), "us_min": round(min(ts), 3), "us_max": round(max(ts), 3),
                  "algorithmic_GBps_at_median": round(bytes_per[k] * n / med / 1e3, 1)}
    rec["fused_over_adamw"] = round(rec["adamw_ema_fused"]["us_median"] / rec["adamw"]["us_median"], 4)
    rec["fused_over_unfused"] = round(rec["adamw_ema_fused"]["us_median"] / rec["adamw_then_lerp"]["us_median"], 4)
    if parent_lib:
        rec["adamw_over_parent"] = round(rec["adamw"]["us_median"] / rec["adamw_parent"]["us_median"], 4)
    return rec


def train_rows(T, Cn, steps, reps, B=64):
    from fourierdiffusion_amd.optim import FusedAdamW
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    dev = torch.device("cuda", torch.cuda.current_device())
    runs = {}
    for name, decay in (("plain", None), ("ema", 0.9999)):
        torch.manual_seed(42)
        m = make_model(T, Cn).to(dev)
        m.train_precision = "bf16"
        m.train()
        opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0, ema_decay=decay)
        X = torch.randn(B, T, Cn, generator=torch.Generator(device="cpu").manual_seed(1000)).to(dev)

        def one_step(i, m=m, opt=opt, X=X):
            m.zero_grad()
            m.training_step(DiffusableBatch(X=X), i)
            opt.step()

        runs[name] = (one_step, m)
    for one_step, _ in runs.values():
        for i in range(10):
            one_step(i)
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, (one_step, _) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                one_step(i)
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / steps)
    rec = {"B": B, "steps": steps, "train_mode": runs["plain"][1].train_mode_effective}
    for k, ts in times.items():
        rec[f"{k}_ms_per_step_median"] = round(statistics.median(ts), 4)
        rec[f"{k}_ms_per_step_all"] = [round(t, 4) for t in ts]
    rec["ema_over_plain"] = round(rec["ema_ms_per_step_median"] / rec["plain_ms_per_step_median"], 4)
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="back-to-back optimizer calls per timed window")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=100, help="training steps per timed window")
    ap.add_argument("--train-reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="another build of libfdiff_hip.so whose fd_adamw_step is timed beside this one's")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ema_bench.py measures on the GPU (there is no CPU timing of a GPU kernel)"
    from fourierdiffusion_amd import _C
    mhz = C.c_double(0.0)
    _C.lib().fd_prof_shader_clock_mhz(_C.ctx(torch.device("cuda", torch.cuda.current_device())), C.byref(mhz))
    out = []
    for name, (T, Cn) in SHAPES.items():
        m = make_model(T, Cn)
        n = m.flat_parameters.numel()
        frozen = [(off, off + numel) for _, off, numel, _, tr in m._layout if not tr][0]
        rec = {"shape": name, "T": T, "C": Cn, "n_params": n, "device": torch.cuda.get_device_name(0), "shader_clock_mhz": mhz.value,
               "calls": args.calls, "reps": args.reps}
        rec["optimizer_pass"] = kernel_rows(n, frozen, args.calls, args.reps, args.parent_lib)
        if not args.skip_train:
            rec["training_step"] = train_rows(T, Cn, args.steps, args.train_reps)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
