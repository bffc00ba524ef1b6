"""CPU: the oracle's restatement of the engine's normals (engine_u01, engine_randn: csrc/fd_philox.h's fd_u01, fd_box_muller and
fd_randn4 on the words of engine_philox_words) -- against a scalar evaluation with the math module, at the two ends of fd_u01, by its
moments, and the committed edge counters of tests/noise_edges.py against the words claimed for them."""
import math
import struct

import numpy as np

from oracle import fdiff_oracle as O

from . import noise_edges as NE


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _u01_scalar(word):
    """fd_u01 with one float32 rounding per operation, spelled without numpy."""
    return _f32(_f32(float(word >> 8) + 0.5) * 2.0 ** -24)


def _pair_scalar(a, b):
    u1, u2 = _u01_scalar(a), _u01_scalar(b)
    r = math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(2.0 * math.pi * u2), r * math.sin(2.0 * math.pi * u2)


HAND_WORDS = (0x00000000, 0x000000FF, 0x00000100, 0x12345678, 0x3FFFFFFF, 0x40000000, 0x7FFFFF00, 0x80000000, 0x80000100,
              0xC0000000, 0xDEADBEEF, 0xFFFFFE00, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF)


def test_u01_at_hand_picked_words_and_both_ends():
    got = O.engine_u01(np.array(HAND_WORDS, dtype=np.uint32))
    assert got.dtype == np.float32
    for w, g in zip(HAND_WORDS, got):
        assert float(g) == _u01_scalar(w), hex(w)
    assert float(O.engine_u01(np.uint32(0xFFFFFF00))) == 1.0                   # reachable: 16777215.5 rounds to 2^24
    assert float(O.engine_u01(np.uint32(0))) == 0.5 * 2.0 ** -24
    assert float(O.engine_u01(np.uint32(0xFFFFFE00))) == 1.0 - 2.0 ** -23      # the largest value below 1
    assert float(O.engine_u01(np.uint32(0x80000000))) == 0.5                   # upper half: the + 0.5 is rounded away (to even)
    assert float(O.engine_u01(np.uint32(0x80000100))) == 0.5 + 2.0 ** -23      # ... so odd tops round up to the even neighbour
    assert float(O.engine_u01(np.uint32(0x7FFFFF00))) == 0.5 - 2.0 ** -25      # lower half: centred, exact
    assert got.min() > 0.0 and got.max() == 1.0


def test_randn_layout_against_scalar_evaluation():
    """Element e <-> counter offset + e // 4, lane e % 4; (x, y) -> elements 0, 1 = (r cos, r sin), (z, w) -> elements 2, 3."""
    for seed, offset, n in ((0, 0, 13), (0x1234567890ABCDEF, 0xFFFFFFFE, 12), (0xFFFFFFFFFFFFFFFF, (1 << 40) + 12345, 7)):
        got = O.engine_randn(seed, offset, n)
        assert got.dtype == np.float64 and got.shape == (n,)
        words = O.engine_philox_words(seed, offset, (n + 3) // 4)
        for e in range(n):
            w = words[e // 4]
            pair = _pair_scalar(int(w[0]), int(w[1])) if e % 4 < 2 else _pair_scalar(int(w[2]), int(w[3]))
            assert abs(got[e] - pair[e % 2]) <= 1e-14 * max(1.0, abs(pair[e % 2])), (seed, offset, e)
    # a longer draw is a prefix-extension, and the offset addresses counters (4 elements each)
    a = O.engine_randn(7, 5, 64)
    assert np.array_equal(O.engine_randn(7, 5, 41), a[:41]) and np.array_equal(O.engine_randn(7, 9, 48), a[16:])
    # the known-answer words of counter 0, key 0 through the whole chain
    x, y, z, w = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    want = _pair_scalar(x, y) + _pair_scalar(z, w)
    np.testing.assert_allclose(O.engine_randn(0, 0, 4), want, rtol=1e-14)


def test_randn_moments():
    n = 1 << 20
    z = O.engine_randn(42, 0, n)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.89
    assert abs(z.mean()) < 4 / math.sqrt(n)
    assert abs(z.var() - 1.0) < 5e-3
    assert abs((z ** 3).mean()) < 2e-2
    assert abs((z ** 4).mean() - 3.0) < 5e-2
    # the two normals of a pair, and the two pairs of a counter, are uncorrelated
    q = z.reshape(-1, 4)
    c = np.corrcoef(q.T)
    assert np.abs(c - np.eye(4)).max() < 5 / math.sqrt(n / 4)


def test_committed_edge_counters_have_the_words_claimed():
    for counter, lane, word in NE.ALL_EDGES:
        w = O.engine_philox_words(NE.EDGE_SEED, counter, 1)[0]
        assert int(w[lane]) == word, (counter, lane, hex(int(w[lane])))
    u = lambda e: float(O.engine_u01(np.uint32(e[2])))
    assert NE.U1_ONE[1] == 2 and NE.U1_ONE[2] >> 8 == 0xFFFFFF and u(NE.U1_ONE) == 1.0
    assert NE.U1_BELOW_ONE[1] == 0 and NE.U1_BELOW_ONE[2] >> 8 == 0xFFFFFE and u(NE.U1_BELOW_ONE) == 1.0 - 2.0 ** -23
    assert NE.U1_SMALLEST[1] == 0 and NE.U1_SMALLEST[2] >> 8 == 0 and u(NE.U1_SMALLEST) == 2.0 ** -25
    tops = [e[2] >> 8 for e in NE.U2_QUADRANTS]
    assert tops == [0, 0, 1 << 22, 1 << 22, 1 << 23, 1 << 23, 3 << 22, 3 << 22]
    assert [e[1] for e in NE.U2_QUADRANTS] == [1, 3] * 4                       # the angle words: y and w
    assert [u(e) for e in NE.U2_QUADRANTS] == [2.0 ** -25, 2.0 ** -25, 0.25 + 2.0 ** -25, 0.25 + 2.0 ** -25, 0.5, 0.5, 0.75, 0.75]
    # what the restatement draws there: u1 == 1 gives +-0 in both elements of the pair, the smallest u1 the largest radius
    z = O.engine_randn(NE.EDGE_SEED, NE.U1_ONE[0], 4)
    assert z[2] == 0.0 and z[3] == 0.0 and z[0] != 0.0
    z = O.engine_randn(NE.EDGE_SEED, NE.U1_SMALLEST[0], 4)
    r = math.hypot(z[0], z[1])
    assert abs(r - math.sqrt(50.0 * math.log(2.0))) < 1e-12 and 5.88 < r < 5.89
    z = O.engine_randn(NE.EDGE_SEED, NE.U1_BELOW_ONE[0], 4)
    assert 0.0 < math.hypot(z[0], z[1]) < 5e-4
    for e in NE.ALL_EDGES:
        assert np.isfinite(O.engine_randn(NE.EDGE_SEED, e[0], 4)).all()
