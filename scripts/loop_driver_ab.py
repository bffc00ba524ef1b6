"""Bitwise A/B and timing of the step-by-step sampling loops across two builds of the engine library (FDIFF_LIB selects the build;
one fresh process per build, nothing is compared inside one process):

    FDIFF_LIB=<before>/libfdiff_hip.so python scripts/loop_driver_ab.py run before OUT
    python scripts/loop_driver_ab.py run after OUT
    python scripts/loop_driver_ab.py compare OUT/before OUT/after        # exit status 1 unless every pair is identical
    [FDIFF_LIB=...] python scripts/loop_driver_ab.py time TAG OUT 4      # appends "<loop> <ms>" lines to OUT/timing_TAG.txt

The cases are those of tests/test_gpu_loop_driver.py (both models, both precisions, FDIFF_SAMPLER_STEPWISE=1), each with Philox and
with injected noise, and the guided ones once more in their two-evaluation form at w = 1 (FDIFF_CFG_FORCE_PAIR=1).  Timing: `sample`
and guided `sample_ode` (Heun, w = 2) in fp32 at (T=100, C=12), the default transformer, batch 64, 50 steps.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["FDIFF_SAMPLER_STEPWISE"] = "1"
import numpy as np  # noqa: E402


def run(tag, out):
    from tests.test_gpu_loop_driver import CASES, run_loop
    out = os.path.join(out, tag)
    os.makedirs(out, exist_ok=True)
    cases = [(mid, prec, loop, "") for mid, prec, loop in CASES]
    cases += [(mid, prec, (loop[0], loop[1], dict(loop[2], cfg_scale=1.0), True), "-forcepair_w1") for mid, prec, loop in CASES if loop[3]]
    for mid, prec, loop, suffix in cases:
        if suffix:
            os.environ["FDIFF_CFG_FORCE_PAIR"] = "1"
        for injected in (False, True):
            x = run_loop(mid, prec, loop, injected=injected)
            np.save(os.path.join(out, f"{mid}-{prec}-{loop[0]}{suffix}-{'injected' if injected else 'philox'}.npy"), x.numpy())
    print(f"{tag}: {2 * len(cases)} cases saved to {out}")


def compare(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b)), "the two runs saved different cases"
    bad = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and bool(np.isfinite(x).all()) and np.array_equal(x, y)
        bad += not same
        print(f"{f[:-4]:60s} {str(x.shape):14s} {'identical' if same else 'DIFFERENT'}")
    print(f"{len(names)} cases, {bad} different")
    return 1 if bad else 0


def timing(tag, out, reps):
    import torch
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    from tests.test_gpu_loop_driver import make_cond
    cfg, B, N = dict(T=100, C=12, D=72, L=10, H=12), 64, 50
    s = DiffusionSampler(score_model=make_model(cfg, precision="fp32")[0], sample_batch_size=B)
    sc = DiffusionSampler(score_model=make_cond(cfg, "fp32"), sample_batch_size=2 * B)
    y = torch.arange(B) % 3
    runs = {"sample": lambda: s.sample(B, N), "cfg_ode_heun_w2": lambda: sc.sample_ode(B, N, solver="heun", y=y, cfg_scale=2.0)}
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"timing_{tag}.txt"), "a") as f:
        for name, fn in runs.items():
            fn()                                        # warm-up: arena growth, weight images
            torch.cuda.synchronize()
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()                                    # (ends in a device-to-host copy: the call is complete on return)
                torch.cuda.synchronize()
                f.write(f"{name} {(time.perf_counter() - t0) * 1e3:.3f}\n")


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "run":
        run(sys.argv[2], sys.argv[3])
    elif cmd == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif cmd == "time":
        timing(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        sys.exit(__doc__)
