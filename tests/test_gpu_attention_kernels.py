"""GPU: every self-attention kernel class against float64 attention, element by element, through fd_attention_forward.

The models of the other test files reach the attention kernels at head_dim 4..8, 12 and 16 only and compare behind W_o, a residual
and a LayerNorm; here each kernel runs on its own, at every head_dim class and at the T where its tiling changes:

  kind 1  k_attention_f32<8,16,32,64>   (fd_score_f32.hip)   head_dim 1..64; 32-key tiles, 64-query blocks, 4 waves up to head_dim 16
  kind 2  k_attention_bf16              (fd_attn_bf16.hip)   head_dim 1..7, two heads per MFMA; bound-shifted fast path and the
                                                              exact path (FDIFF_ATTN_EXACT=1)
  kind 3  k_attention_wide<16>, <32>    (fd_attn_wide.hip)   head_dim 8..16 / 17..32; 16-byte staging when head_dim % 4 == 0, guarded
                                                              scalar staging otherwise; K / V^T of a head and series within 160 KiB
  kind 0  the dispatch of the layer stack's unfused form: kind 2, else kind 3, else kind 1

Inputs (tests/attn_ref.make_case): unit-scale v; q and k scaled to a "flat" (row logit range ~2, base 2) and a "sharp" (~40) regime,
the sharp one with two planted rows whose result is decided by the last valid key and by the mask of the padded keys.

Tolerances, each against the float64 reference (never against another engine path), every element checked:
  * f32: 2e-5 max|v| -- the suite's fp32 bound for long sums (test_gpu_widths.py); the output is a convex combination of v and the
    relative error of exp at |s| <= 60 stays below 1e-5, so the bound holds in the sharp regime too.
  * bf16: per element 4 |attention_bf16_contract - attention| + 2^-8 max|v|, evaluated on the CPU.  The first term is the rounding the
    kernels' contract allows (operands in bf16), with a factor 4 for what the contract leaves open: fp32 accumulation order, the
    hardware exp2 / rcp, the fast path's shift differing from the exact maximum.  The second is one bf16 ulp of the output scale.
    In the flat regime the bound itself must stay below the suite's bf16 contract, 2e-2 of the scale max|v| the bound is stated in
    (asserted on the CPU: the yardstick cannot silently become loose).
  * every bf16 case differs from the f32 kernel's output somewhere: a kind cannot silently run the f32 kernel.
The output buffer is NaN-filled before each call (an element the kernel skips fails) and carries a guard tail that must stay NaN.

Figures of one run: profiles/attention_tests_figures.txt (the "[attention]" lines this file logs)."""
import functools

import numpy as np
import pytest
import torch

from . import attn_ref as R
from .gpu_util import DEV, log_line

pytestmark = pytest.mark.gpu

AUTO, F32, PACKED, WIDE = 0, 1, 2, 3
UNSUPPORTED = -5
REGIMES = {"flat": R.FLAT, "sharp": R.SHARP}
GUARD = 256


@functools.lru_cache(maxsize=None)
def case(B, T, H, hd, regime):
    """Inputs and float64 references of one shape, computed once and shared (read-only) by every test that needs them."""
    qkv, planted = R.make_case(f"{B}_{T}_{H}_{hd}_{regime}", B, T, H, hd, REGIMES[regime])
    R.check_planted(qkv, planted, B, T, H, hd)
    ref = R.attention(qkv, B, T, H, hd)
    vmax = float(np.abs(qkv[:, 2 * H * hd:]).max())
    for a in (qkv, ref):
        a.setflags(write=False)
    return dict(qkv=qkv, ref=ref, vmax=vmax, dims=(B, T, H, hd), regime=regime)


@functools.lru_cache(maxsize=None)
def bf16_bound(B, T, H, hd, regime, rounded_denominator):
    c = case(B, T, H, hd, regime)
    con = R.attention_bf16_contract(c["qkv"], B, T, H, hd, rounded_denominator=rounded_denominator)
    bound = 4.0 * np.abs(con - c["ref"]) + 2.0 ** -8 * c["vmax"]
    if regime == "flat":
        assert bound.max() < 2e-2 * c["vmax"], (bound.max(), c["vmax"])
    bound.setflags(write=False)
    return bound


def run(c, kind):
    """(return code, output (B*T, D) float64 or None).  Poisoned output, guard tail checked."""
    from fourierdiffusion_amd import _C
    B, T, H, hd = c["dims"]
    D = H * hd
    x = torch.tensor(c["qkv"], device=DEV)
    buf = torch.full((B * T * D + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    h = _C.ctx(x.device)
    rc = _C.lib().fd_attention_forward(h, x.data_ptr(), buf.data_ptr(), B, T, H, hd, kind, _C.stream_of(x))
    if rc == UNSUPPORTED:
        assert b"no kernel" in _C.lib().fd_last_error(h)
        return rc, None
    _C.check(rc, h)
    got = buf.cpu().numpy().astype(np.float64)
    assert np.isnan(got[B * T * D:]).all(), "the kernel wrote behind its output"
    return rc, got[:B * T * D].reshape(B * T, D)


def share_of(got, c, bound):
    """max over the elements of |got - ref| / bound; NaN (an unwritten element) counts as infinite."""
    err = np.abs(got - c["ref"]) / bound
    return float(np.where(np.isnan(err), np.inf, err).max()), float(np.nanmax(np.abs(got - c["ref"])))


class Tally:
    """Worst share of the bound per kernel class, logged once per test; failures collected so that every shape is measured."""

    def __init__(self, what):
        self.what, self.worst, self.bad = what, {}, []

    def add(self, cls, c, share, err):
        key = (cls, c["regime"])
        if share > self.worst.get(key, (-1.0,))[0]:
            self.worst[key] = (share, err, c["dims"])
        if not share <= 1.0:
            self.bad.append((cls, c["regime"], c["dims"], share, err))

    def close(self):
        for (cls, regime), (share, err, dims) in sorted(self.worst.items()):
            log_line(f"[attention] {self.what:<28} {cls:<24} {regime:<5} worst at B,T,H,hd={dims}: max err {err:.3e}  share of bound {share:.4f}")
        assert not self.bad, self.bad


def f32_class(hd):
    return f"f32<{8 if hd <= 8 else 16 if hd <= 16 else 32 if hd <= 32 else 64}>"


def wide_class(hd):
    return f"wide<{16 if hd <= 16 else 32}> {'16-byte' if hd % 4 == 0 else 'scalar'}"


def check_f32(tally, c, got, cls=None):
    share, err = share_of(got, c, 2e-5 * c["vmax"])
    tally.add(cls or f32_class(c["dims"][3]), c, share, err)


def check_bf16(tally, c, got, cls, rounded_denominator):
    B, T, H, hd = c["dims"]
    share, err = share_of(got, c, bf16_bound(B, T, H, hd, c["regime"], rounded_denominator))
    tally.add(cls, c, share, err)
    _, f32 = run(c, F32)
    assert np.abs(got - f32).max() > 0, f"{cls} at {c['dims']}: bit-identical to the f32 kernel"


@pytest.mark.parametrize("hd", [1, 5, 8, 9, 16, 17, 32, 33, 48, 64])
def test_f32_kernel_vs_float64(hd):
    """T = 31 / 32 / 33: a 32-key tile boundary; 64 / 65, 129: a 64-query block boundary; T <= 96 at head_dim <= 16: some of the
    block's four waves get no key tile (T = 1, 31, 32: three of them)."""
    tally = Tally(f"f32 head_dim {hd}")
    for H in (1, 3):
        for T in (1, 31, 32, 33, 64, 65, 100, 129):
            for regime in REGIMES:
                c = case(2, T, H, hd, regime)
                rc, got = run(c, F32)
                assert rc == 0
                check_f32(tally, c, got)
    tally.close()


@pytest.mark.parametrize("hd", [8, 9, 12, 15, 16, 17, 18, 20, 24, 31, 32])
def test_wide_kernel_vs_float64(hd):
    """T = 33, 257: an odd key-tile count, the second half of the last V^T block is absent; T = 1, 17, 33, 100, 257: a ragged last
    tile; T = 16, 48: whole tiles; T = 1, 16: a unit whose second query tile does not exist."""
    tally = Tally(f"wide head_dim {hd}")
    for H in (1, 3):
        for T in (1, 16, 17, 33, 48, 100, 257):
            for regime in REGIMES:
                c = case(2, T, H, hd, regime)
                rc, got = run(c, WIDE)
                assert rc == 0
                check_bf16(tally, c, got, wide_class(hd), False)
    tally.close()


def wide_lds_bytes(T, hd):
    """The LDS image of fd_attention_bf16_wide: K rows [16 KT][4 lane groups][8 or 16 B] + V^T blocks [NJ][HDS / 16][1 KiB]."""
    HDS = 16 if hd <= 16 else 32
    KT = (T + 15) // 16
    NJ = (KT + 1) // 2
    return KT * 16 * 4 * (8 if HDS == 16 else 16) + NJ * (HDS // 16) * 1024


def wide_largest_T(hd):
    T = 1
    while wide_lds_bytes(T + 1, hd) <= 160 * 1024:
        T += 1
    return T


@pytest.mark.parametrize("hd", [16, 32])
def test_wide_kernel_long_series_and_lds_limit(hd):
    """B = H = 1: T = 1024 (several query slices per head), the largest T whose K / V^T image fits the 160 KiB, and one beyond it,
    which the kernel must refuse (the dispatch then runs the f32 kernel: test_auto_dispatch)."""
    tally = Tally(f"wide head_dim {hd} long")
    Tmax = wide_largest_T(hd)
    assert wide_lds_bytes(Tmax, hd) == 160 * 1024 and (hd != 32 or Tmax == 1280)
    for T in (1024, Tmax):
        for regime in REGIMES:
            c = case(1, T, 1, hd, regime)
            rc, got = run(c, WIDE)
            assert rc == 0
            check_bf16(tally, c, got, wide_class(hd), False)
    rc, got = run(case(1, Tmax + 1, 1, hd, "flat"), WIDE)
    assert rc == UNSUPPORTED and got is None
    tally.close()


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("hd", [1, 2, 3, 4, 5, 6, 7])
def test_packed_kernel_vs_float64(hd, exact, monkeypatch):
    """H = 1, 3: an unpaired last head; T = 15 / 16 / 17 a key-tile boundary, 127 / 128 / 129 a 128-key block boundary, 365 a partial
    last block padded to a whole one.  Both softmax forms: the bound-shifted fast path with its per-row rescue, and the exact two-pass
    path alone (FDIFF_ATTN_EXACT=1)."""
    if exact:
        monkeypatch.setenv("FDIFF_ATTN_EXACT", "1")
    else:
        monkeypatch.delenv("FDIFF_ATTN_EXACT", raising=False)
    for var in ("FDIFF_ATTN_SLICES", "FDIFF_ATTN_PAD_MIN"):
        monkeypatch.delenv(var, raising=False)
    tally = Tally(f"packed head_dim {hd}")
    for H in (1, 2, 3):
        for T in (1, 15, 16, 17, 127, 128, 129, 365):
            for regime in REGIMES:
                c = case(2, T, H, hd, regime)
                rc, got = run(c, PACKED)
                assert rc == 0
                check_bf16(tally, c, got, "packed exact" if exact else "packed fast", True)
    tally.close()


def test_packed_kernel_refuses_head_dim_8():
    rc, got = run(case(2, 33, 3, 8, "flat"), PACKED)
    assert rc == UNSUPPORTED and got is None


def test_wide_kernel_refuses_head_dim_33():
    rc, got = run(case(2, 33, 3, 33, "flat"), WIDE)
    assert rc == UNSUPPORTED and got is None


@pytest.mark.parametrize("B,T,H,hd,forced", [(2, 100, 3, 6, PACKED), (2, 100, 3, 12, WIDE), (2, 100, 3, 24, WIDE), (2, 100, 3, 40, F32),
                                             (1, 1281, 1, 32, F32)],
                         ids=["hd6_packed", "hd12_wide16", "hd24_wide32", "hd40_f32", "hd32_T1281_beyond_lds_f32"])
def test_auto_dispatch(B, T, H, hd, forced, monkeypatch):
    """Kind 0 is the chain the layer stack runs: one case per branch, bit for bit the forced kind's result; where it must fall back to
    the f32 kernel (head_dim > 32, K / V^T beyond the LDS) the result meets the f32 tolerance, which no bf16 kernel would."""
    for var in ("FDIFF_ATTN_F32", "FDIFF_ATTN_EXACT", "FDIFF_ATTN_SLICES", "FDIFF_ATTN_PAD_MIN"):
        monkeypatch.delenv(var, raising=False)
    tally = Tally(f"auto head_dim {hd} T {T}")
    for regime in REGIMES:
        c = case(B, T, H, hd, regime)
        rc, got = run(c, AUTO)
        rcf, want = run(c, forced)
        assert rc == 0 and rcf == 0
        assert np.array_equal(got, want), f"auto differs from kind {forced}"
        if forced == F32:
            check_f32(tally, c, got, "auto -> " + f32_class(hd))
            if hd <= 32:
                assert run(c, WIDE)[0] == UNSUPPORTED
        else:
            check_bf16(tally, c, got, "auto -> " + ("packed fast" if forced == PACKED else wide_class(hd)), forced == PACKED)
    tally.close()


def test_c_abi_argument_errors():
    """fd_attention_forward refuses bad arguments with FD_ERR_ARG and a message (include/fdiff_hip.h conventions)."""
    from fourierdiffusion_amd import _C
    x = torch.zeros(8, 3 * 8, device=DEV)
    y = torch.zeros(8, 8, device=DEV)
    h, L = _C.ctx(x.device), _C.lib()
    p, q = x.data_ptr(), y.data_ptr()
    cases = [
        (lambda: L.fd_attention_forward(h, None, q, 2, 4, 2, 4, 1, None), b"null"),
        (lambda: L.fd_attention_forward(h, p, None, 2, 4, 2, 4, 1, None), b"null"),
        (lambda: L.fd_attention_forward(h, p, p, 2, 4, 2, 4, 1, None), b"aliased"),
        (lambda: L.fd_attention_forward(h, p, q, 0, 4, 2, 4, 1, None), b"bad shape"),
        (lambda: L.fd_attention_forward(h, p, q, 2, 0, 2, 4, 1, None), b"bad shape"),
        (lambda: L.fd_attention_forward(h, p, q, 2, 4, 0, 4, 1, None), b"bad shape"),
        (lambda: L.fd_attention_forward(h, p, q, 2, 4, 2, 0, 1, None), b"bad shape"),
        (lambda: L.fd_attention_forward(h, p, q, 2, 4, 2, 65, 1, None), b"bad shape"),
        (lambda: L.fd_attention_forward(h, p, q, 70000, 4, 2, 4, 1, None), b"bad shape"),
        (lambda: L.fd_attention_forward(h, p, q, 60000, 60000, 2, 4, 1, None), b"too large"),
        (lambda: L.fd_attention_forward(h, p, q, 2, 4, 2, 4, 4, None), b"unknown kind"),
        (lambda: L.fd_attention_forward(h, p, q, 2, 4, 2, 4, -1, None), b"unknown kind"),
    ]
    for i, (call, needle) in enumerate(cases):
        assert call() == -1, i
        assert needle in L.fd_last_error(h), (i, L.fd_last_error(h))
    assert L.fd_attention_forward(None, p, q, 2, 4, 2, 4, 1, None) == -1          # no context: error code only
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0                                            # nothing was launched
