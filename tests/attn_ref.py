"""Float64 numpy reference of the self-attention core and its bf16 rounding yardstick.

``attention`` is softmax(q k^T / sqrt(head_dim)) v per head, from the packed projections the engine's attention kernels read:
rows [q | k | v] of (B*T, 3*H*head_dim), heads concatenated as nn.MultiheadAttention does (tests/test_attn_ref_cpu.py pins it to
torch's float64 multi_head_attention_forward).

``attention_bf16_contract`` is the same arithmetic in float64 with the operands rounded the way the headers of fd_attn_bf16.hip and
fd_attn_wide.hip state: q * log2(e)/sqrt(head_dim) computed in fp32 and rounded to bf16, k, v and P = exp2(S - max) rounded to bf16;
maxima, sums and accumulation exact.  Its difference from ``attention`` is the rounding yardstick of the bf16 tests: a property of
this reference alone (like autograd_ref.tau_of), never of the engine.  The packed kernel takes the softmax denominator from a row of
ones in V^T, i.e. it sums the ROUNDED P (``rounded_denominator=True``); the wide kernel sums the fp32 P on the VALU (False).

``make_case`` builds the test inputs: unit-scale v, q and k scaled to a target row logit range, and in the sharp regime the planted
rows of tests/test_gpu_attention_kernels.py.

Shared by tests/test_attn_ref_cpu.py and tests/test_gpu_attention_kernels.py."""
import math

import numpy as np

from oracle import weights as W

LOG2E = 1.4426950408889634


def bf16_round(a):
    """Round to the nearest bfloat16 (8 significant bits), ties to even; float64 in, float64 out.  Exponent range is not modelled
    (bf16 shares float32's; the values here stay far inside it)."""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)                       # a = m 2^e, 0.5 <= |m| < 1
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)       # np.rint: half to even


def split(qkv, B, T, H, hd):
    """(q, k, v), each (B, H, T, hd) float64."""
    D = H * hd
    x = np.asarray(qkv, dtype=np.float64).reshape(B, T, 3, H, hd)
    assert np.asarray(qkv).shape == (B * T, 3 * D)
    return tuple(x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))


def _merge(o):
    B, H, T, hd = o.shape
    return o.transpose(0, 2, 1, 3).reshape(B * T, H * hd)


def logits2(qkv, B, T, H, hd):
    """Base-2 logits q k^T log2(e) / sqrt(hd), (B, H, T, T) float64."""
    q, k, _ = split(qkv, B, T, H, hd)
    return (q @ k.transpose(0, 1, 3, 2)) * (LOG2E / math.sqrt(hd))


def attention(qkv, B, T, H, hd):
    """softmax(q k^T / sqrt(hd)) v per head, (B*T, H*hd) float64."""
    q, k, v = split(qkv, B, T, H, hd)
    s = (q @ k.transpose(0, 1, 3, 2)) / math.sqrt(hd)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return _merge((p @ v) / p.sum(axis=-1, keepdims=True))


def attention_bf16_contract(qkv, B, T, H, hd, rounded_denominator=False):
    """``attention`` with the bf16 kernels' operand rounding (module docstring), everything else exact."""
    q, k, v = split(qkv, B, T, H, hd)
    qscale = np.float32(np.float32(LOG2E) / np.sqrt(np.float32(hd)))
    qs = bf16_round((q.astype(np.float32) * qscale).astype(np.float32))
    s = qs @ bf16_round(k).transpose(0, 1, 3, 2)
    p = np.exp2(s - s.max(axis=-1, keepdims=True))
    pr = bf16_round(p)
    den = (pr if rounded_denominator else p).sum(axis=-1, keepdims=True)
    return _merge((pr @ bf16_round(v)) / den)


FLAT, SHARP = 2.0, 40.0          # target row logit range (max - min over the keys of a row, median over rows), base 2
PLANT = 30.0                     # |largest base-2 logit| of a planted row


def make_case(name, B, T, H, hd, regime):
    """(qkv float32 (B*T, 3*H*hd), planted) for one test case.  q and k are N(0,1) scaled by one common factor so that the median row
    logit range is ``regime`` (FLAT or SHARP, base 2); v is N(0,1).  SHARP plants two rows in head 0 of series 0:
      * ``last``: query 0, whose largest logit belongs to the LAST valid key T-1 (k[T-1] is given the largest norm of the head and
        the query points along it): a kernel that drops or mis-masks the tail of the last key tile loses the whole row;
      * ``pad`` (T >= 2): query T-1, every one of whose raw q.k is negative (the head's k get a positive first component, the query
        is a negative multiple of e_0), so a padded key -- zero in the staged tiles, raw score 0 -- would take the row's maximum if
        it were scored.
    ``planted`` maps those names to the query index; ``check_planted`` asserts the two properties in float64."""
    D = H * hd
    q = W.randn(f"attn_q_{name}", (B, T, H, hd), 11).astype(np.float64)
    k = W.randn(f"attn_k_{name}", (B, T, H, hd), 11).astype(np.float64)
    v = W.randn(f"attn_v_{name}", (B, T, H, hd), 11).astype(np.float64)
    c = LOG2E / math.sqrt(hd)
    logits = lambda: np.einsum("bihd,bjhd->bhij", q, k) * c      # noqa: E731
    s = logits()
    rng = float(np.median(s.max(axis=-1) - s.min(axis=-1)))
    a = math.sqrt(regime / rng) if rng > 0 else 1.0
    q, k = q * a, k * a
    planted = {}
    if regime == SHARP:
        if T >= 2:
            k[0, :, 0, 0] = np.abs(k[0, :, 0, 0]) + 0.05 * a
        norms = np.linalg.norm(k[0, :, 0], axis=-1)
        k[0, T - 1, 0] *= 1.1 * norms.max() / norms[T - 1]
        top = float(np.abs(logits()).max())      # (heavy tails at small head_dim: keep every logit inside the fp32 tolerance's premise)
        if top > 55.0:
            q, k = q * math.sqrt(55.0 / top), k * math.sqrt(55.0 / top)
        kl = k[0, T - 1, 0]
        q[0, 0, 0] = kl * (PLANT / (c * float(kl @ kl)))
        planted["last"] = 0
        if T >= 2:
            q[0, T - 1, 0] = 0.0
            q[0, T - 1, 0, 0] = -PLANT / (c * float(k[0, :, 0, 0].max()))
            planted["pad"] = T - 1
    qkv = np.concatenate([x.reshape(B * T, D) for x in (q, k, v)], axis=1).astype(np.float32)
    return qkv, planted


def check_planted(qkv, planted, B, T, H, hd):
    """The properties ``make_case`` promises, from the float32 inputs as the kernels see them."""
    if not planted:
        return
    q, k, _ = split(qkv, B, T, H, hd)
    raw = q[0, 0] @ k[0, 0].T                      # (T, T) raw q.k of head 0, series 0
    row = raw[planted["last"]]
    assert int(row.argmax()) == T - 1 and (T == 1 or row[T - 1] > np.delete(row, T - 1).max()), "planted row: last key is not the largest"
    if "pad" in planted:
        assert raw[planted["pad"]].max() < 0.0, "planted row: a padded (zero) key would not win"
    s = logits2(qkv, B, T, H, hd)
    assert np.abs(s).max() <= 60.0, np.abs(s).max()      # (the fp32 tolerance's premise)
