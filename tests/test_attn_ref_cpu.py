"""CPU: tests/attn_ref.py is what it claims to be -- ``attention`` equals torch's float64 multi_head_attention_forward with identity
projections, ``bf16_round`` is round-to-nearest-even against torch.bfloat16, and the inputs ``make_case`` builds have the properties
the GPU tests rely on (tests/test_gpu_attention_kernels.py)."""
import numpy as np
import pytest
import torch

from oracle import weights as W

from . import attn_ref as R


def _torch_mha(qkv, B, T, H, hd):
    """nn.functional.multi_head_attention_forward in float64 on already projected q, k, v: identity in- and out-projections."""
    D = H * hd
    x = torch.tensor(np.asarray(qkv, dtype=np.float64)).reshape(B, T, 3, D)
    q, k, v = (x[:, :, i].transpose(0, 1).contiguous() for i in range(3))        # (T, B, D)
    eye = torch.eye(D, dtype=torch.float64)
    out, _ = torch.nn.functional.multi_head_attention_forward(
        q, k, v, D, H, None, None, None, None, False, 0.0, eye, torch.zeros(D, dtype=torch.float64), training=False,
        need_weights=False, use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
    return out.transpose(0, 1).reshape(B * T, D).numpy()


@pytest.mark.parametrize("B,T,H,hd", [(2, 33, 3, 5), (1, 64, 2, 16), (3, 7, 1, 18)],
                         ids=["odd_T_hd5", "T64_hd16", "hd18_one_head"])
def test_attention_equals_torch_float64_mha(B, T, H, hd):
    qkv = W.randn(f"attn_cpu_{T}_{hd}", (B * T, 3 * H * hd), 4).astype(np.float64) * 1.7
    got = R.attention(qkv, B, T, H, hd)
    ref = _torch_mha(qkv, B, T, H, hd)
    assert got.shape == ref.shape == (B * T, H * hd)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13 * np.abs(ref).max())


def test_bf16_round_is_round_to_nearest_even():
    x = np.concatenate([W.randn("attn_cpu_bf", (4096,), 4) * np.float32(3.0), W.randn("attn_cpu_bf2", (4096,), 4) * np.float32(1e-6),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38 / 4, 2.0 ** -100], dtype=np.float32)])
    # ties: 1 + 2^-8 lies half way between 1 and 1 + 2^-7 (-> even: 1); 1 + 3 2^-8 half way between 1 + 2^-7 and 1 + 2^-6 (-> 1 + 2^-6)
    ref = torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy()
    got = R.bf16_round(x)
    assert np.array_equal(got, ref)
    assert R.bf16_round(1.00390625) == 1.0 and R.bf16_round(1.01171875) == 1.015625
    # float64 input is rounded once, not through float32: 1 + 2^-8 + 2^-40 is above the tie
    assert R.bf16_round(1.0 + 2.0 ** -8 + 2.0 ** -40) == 1.0078125


def test_contract_is_attention_up_to_bf16_rounding():
    """The yardstick is small where it should be, exactly 0 when every operand is bf16-representable and P is a power of two, and
    differs between the two denominators only by the rounding of P."""
    B, T, H, hd = 2, 40, 2, 12
    qkv, _ = R.make_case("cpu_contract", B, T, H, hd, R.FLAT)
    a = R.attention(qkv, B, T, H, hd)
    c0 = R.attention_bf16_contract(qkv, B, T, H, hd)
    c1 = R.attention_bf16_contract(qkv, B, T, H, hd, rounded_denominator=True)
    vmax = np.abs(qkv[:, 2 * H * hd:]).max()
    for c in (c0, c1):
        d = np.abs(c - a).max()
        assert 0 < d <= 2.0 ** -7 * vmax, d
    assert 0 < np.abs(c0 - c1).max() <= 2.0 ** -8 * vmax
    one = np.zeros((1, 3 * 4), dtype=np.float32)       # T = 1: softmax = 1, out = bf16(v)
    one[0, 8:] = [1.0, 1.00390625, -2.5, 0.3]
    got = R.attention_bf16_contract(one, 1, 1, 1, 4)
    assert np.array_equal(got[0], R.bf16_round(one[0, 8:]))


@pytest.mark.parametrize("T,hd", [(1, 3), (17, 1), (33, 18), (100, 64)])
def test_make_case_regimes_and_planted_rows(T, hd):
    B, H = 2, 3
    for regime in (R.FLAT, R.SHARP):
        qkv, planted = R.make_case(f"cpu_{T}_{hd}", B, T, H, hd, regime)
        assert qkv.dtype == np.float32 and qkv.shape == (B * T, 9 * hd)
        R.check_planted(qkv, planted, B, T, H, hd)
        s = R.logits2(qkv, B, T, H, hd)
        rng = np.median(s.max(axis=-1) - s.min(axis=-1))
        if T > 1:
            assert (rng <= 1.05 * regime) and (regime == R.SHARP or rng >= 0.95 * regime), (rng, regime)
            assert set(planted) == ({"last", "pad"} if regime == R.SHARP else set())
        assert 0.5 < np.abs(qkv[:, 6 * hd:]).std() < 2.0            # v: unit scale
