"""Restatement of the weight average that fd_adamw_ema_step keeps (an extension, not in the reference; score_sde's / torch-ema's
ExponentialMovingAverage): the warm-up schedule and the recurrence, the latter in float64 on the float32 parameters the device
produced -- what tests/test_gpu_ema.py compares the device's float32 average against."""
import numpy as np


def decay_at(k, decay, warmup=True):
    """Decay of the update that follows k earlier ones."""
    return min(float(decay), (1.0 + k) / (10.0 + k)) if warmup else float(decay)


def recurrence(e0, params, decays):
    """[e_1 .. e_K] with e_k = d_k e_{k-1} + w_k p_k in float64, where d_k is the decay rounded to float32 (what the C ABI takes)
    and w_k = float32(1) - d_k in float32 (what the kernel forms)."""
    e = np.asarray(e0, dtype=np.float64).copy()
    out = []
    for p, d in zip(params, decays):
        d32 = np.float32(d)
        w32 = np.float32(1.0) - d32
        e = np.float64(d32) * e + np.float64(w32) * np.asarray(p, dtype=np.float64)
        out.append(e.copy())
    return out


def tolerance(params, averages):
    """Per-element bound on |device - recurrence| after K = len(params) steps: each step rounds twice in float32 (the product
    w_k p_k, then the fused d_k e + product), each by at most half an ulp <= 2^-24 of a value no larger than max(|p_k|, |e_k|) --
    2^-23 of that magnitude per step, summed over the steps without credit for the decay d_k <= 1 shrinking the earlier errors."""
    K = len(params)
    mag = np.zeros_like(np.asarray(averages[0], dtype=np.float64))
    for p, e in zip(params, averages):
        mag = np.maximum(mag, np.maximum(np.abs(np.asarray(p, dtype=np.float64)), np.abs(e)))
    return K * 2.0 ** -23 * mag
