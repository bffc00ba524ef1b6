"""Lane maps of k_mega's merged ragged key and query tiles (csrc/fd_mega_kernel.h, RAGGED_MERGE), restated in NumPy and checked by
brute force.

A series of T = 16 (KT - 1) + R tokens with R <= 8 leaves its last key tile less than half full.  The attention units then score
BOTH heads of a pair in one 16x16x16 tile: rows [0, RH) carry the even head's keys, rows [RH, 2 RH) the same keys for the odd head
(RH = 4 for R <= 4, else 8); the head is selected in the K operand, Q keeps both heads live.  The tile's P V product -- V^T rows
0-7 against the even head's rows, rows 8-15 against the odd head's -- is the first accumulator of both heads' P V chains.  The single-tile units, whose query tile is the ragged one, also put both heads into one chain of score tiles:
column tok < RH is query tok of the even head, column RH + tok the same query of the odd head.

This file emulates the MFMA tile arithmetic lane by lane in float64 (operands are small random bf16-rounded numbers, so the products
are exact enough to compare at 1e-12), builds the operands with the kernel's address and select expressions, and compares the unit's
epilogue with "softmax over the first T keys, per head" for R = 1 .. 8.  A wrong select or address shows here, without a GPU.
"""
import numpy as np
import pytest

NEG = -1.0e30
HD = 6            # head_dim of the default model (72 / 12): k-slot HD of a head carries the shift (Q) / the 1.0 (K) / the ones row (V^T)
LANES = np.arange(64)
TOK, G = LANES & 15, LANES >> 4


def _bf16(x):
    """round to nearest even bf16, returned as float64"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def mfma(a, b, c):
    """v_mfma_f32_16x16x{4 n}: a, b are [64 lanes][n] (row / column = lane & 15, k = n * (lane >> 4) + i), c and the result are
    [64][4] (row 4 (lane >> 4) + r, column lane & 15)."""
    n = a.shape[1]
    am = np.zeros((16, 4 * n))
    bm = np.zeros((4 * n, 16))
    for l in range(64):
        am[TOK[l], n * G[l]:n * G[l] + n] = a[l]
        bm[n * G[l]:n * G[l] + n, TOK[l]] = b[l]
    out = am @ bm
    d = np.empty((64, 4))
    for l in range(64):
        d[l] = out[4 * G[l]:4 * G[l] + 4, TOK[l]] + c[l]
    return d


class Unit:
    """One (head pair, series) with KT key tiles and one query tile, in the kernel's LDS layouts."""

    def __init__(self, KT, R, seed):
        rng = np.random.default_rng(seed)
        self.KT, self.R, self.T = KT, R, 16 * (KT - 1) + R
        self.RH = 4 if R <= 4 else 8
        ntok = 16 * KT
        # K rows [token][16 k-slots]: even head in slots 0-7, odd head in 8-15; slot HD of each head is the bias row's 1.0.  The padded
        # tokens hold finite junk, as in the kernel (they are projections of whatever the padded residual rows hold).
        k = _bf16(rng.standard_normal((ntok, 2, 8)))
        k[:, :, HD] = 1.0
        k[:, :, HD + 1:] = 0.0
        self.kbf = k.reshape(ntok, 4, 4)                       # [token][lane group g][4 slots]: 8-byte rows
        v = _bf16(rng.standard_normal((2, 8, ntok)))           # V^T [head][dim][token]
        v[:, HD, :] = 1.0                                      # the ones row: P V yields the softmax denominator
        v[:, HD + 1:, :] = 0.0
        self.v = v
        NJ = (KT + 1) // 2
        self.vbf = np.zeros((NJ, 4, 16, 8))                    # [32-key block][g][V^T row d][8]: tile 2 jb keys 4g+i, then tile 2 jb+1
        for kt in range(KT):
            for g in range(4):
                for d in range(16):
                    self.vbf[kt >> 1, g, d, 4 * (kt & 1):4 * (kt & 1) + 4] = v[d >> 3, d & 7, 16 * kt + 4 * g:16 * kt + 4 * g + 4]
        # (an odd tile count leaves the upper half of the last block zero: the kernel's K/V projection writes those zeros)
        q = _bf16(0.5 * rng.standard_normal((16, 2, 8)))       # one query tile [query][head][slot]
        q[:, :, HD:] = 0.0
        self.q = q
        # the softmax shift: any value >= the row maximum works; -bound sits in slot HD of each head
        s = np.einsum("qhd,khd->hqk", q[:, :, :HD], k[:self.T, :, :HD])
        self.bound = _bf16(s.max(axis=2).T + 1.0)              # [query][head]
        self.s = s

    # ---- operands as the kernel builds them (lane = column / row lane & 15, lane group g)
    def q_operand(self, head):
        """fast-path Q of one head (qs[q][hs]): own head's slots with -bound patched in, the other head's lane groups zero;
        head=None: both heads live (qsb[q])"""
        w = self.q.copy()
        w[:, :, HD] = -self.bound
        w = w.reshape(16, 4, 4)
        b = np.zeros((64, 4))
        for l in range(64):
            if head is None or (G[l] >> 1) == head:
                b[l] = w[TOK[l], G[l]]
        return b

    def k_operand(self, kt):
        return np.stack([self.kbf[16 * kt + TOK[l], G[l]] for l in range(64)])

    def v_operand(self, jb):
        return np.stack([self.vbf[jb, G[l], TOK[l]] for l in range(64)])

    def cmask(self):
        return np.array([[NEG if 16 * (self.KT - 1) + 4 * G[l] + r >= self.T else 0.0 for r in range(4)] for l in range(64)])

    # ---- the merged ragged tile
    def merged_k_operand(self):
        RH, k0 = self.RH, 16 * (self.KT - 1)
        a = np.zeros((64, 4))
        for l in range(64):
            keep = TOK[l] < 2 * RH and (TOK[l] < RH) == (G[l] < 2)
            if keep:
                a[l] = self.kbf[k0 + (TOK[l] & (RH - 1)), G[l]]
        return a

    def merged_cmask(self):
        RH = self.RH
        return np.array([[NEG if (4 * G[l] + r >= 2 * RH or ((4 * G[l] + r) & (RH - 1)) >= self.R) else 0.0 for r in range(4)]
                         for l in range(64)])

    def merged_v_operand(self):
        RH, NJ = self.RH, (self.KT + 1) // 2
        a = np.zeros((64, 8))
        for l in range(64):
            g = G[l]
            row_even = (g == 0) if RH == 4 else (g < 2)
            row_odd = (g == 1) if RH == 4 else (g >= 2)
            keep = row_even if TOK[l] < 8 else row_odd
            if keep:
                a[l, :4] = self.vbf[NJ - 1, g & (RH // 4 - 1), TOK[l], :4]
        return a

    # ---- one unit, fast path: returns the normalised head outputs [query][head][HD] the epilogue would store
    def run(self, merged):
        KT = self.KT
        zero4 = np.zeros((64, 4))
        o = [zero4.copy(), zero4.copy()]
        full_tiles = KT - 1 if merged else KT
        if merged:
            sc = np.exp2(mfma(self.merged_k_operand(), self.q_operand(None), self.merged_cmask()))
            rg = mfma(self.merged_v_operand(), np.concatenate([sc, zero4], axis=1), zero4)
            o = [rg.copy(), rg.copy()]
        for hs in range(2):
            qs = self.q_operand(hs)
            for jb in range((full_tiles + 1) // 2):
                p = []
                for kt in (2 * jb, 2 * jb + 1):
                    if kt < full_tiles:
                        p.append(np.exp2(mfma(self.k_operand(kt), qs, self.cmask() if kt == KT - 1 else zero4)))
                    else:
                        p.append(zero4)
                o[hs] = mfma(self.v_operand(jb), np.concatenate(p, axis=1), o[hs])
        # epilogue: lane (query = lane & 15, g) holds dims 4 (g & 1) + r of head g >> 1, taken from that head's accumulator
        out = np.zeros((16, 2, 8))
        for l in range(64):
            out[TOK[l], G[l] >> 1, 4 * (G[l] & 1):4 * (G[l] & 1) + 4] = o[G[l] >> 1][l]
        return out[:, :, :HD] / out[:, :, HD:HD + 1]

    # ---- the merged ragged QUERY tile (single-tile units): one chain serves both heads
    def merged_q_operand(self):
        """column tok < RH: query tok, even head's k-slot groups; column RH + tok: query tok, odd head's groups (the kernel moves
        those words by a DPP row shift of RH lanes inside lane groups 2-3); zero elsewhere"""
        RH = self.RH
        w = self.q.copy()
        w[:, :, HD] = -self.bound
        w = w.reshape(16, 4, 4)
        b = np.zeros((64, 4))
        for l in range(64):
            if TOK[l] < RH and G[l] < 2:
                b[l] = w[TOK[l], G[l]]
            elif RH <= TOK[l] < 2 * RH and G[l] >= 2:
                b[l] = w[TOK[l] - RH, G[l]]
        return b

    def merged_q_cmask(self):
        RH = self.RH
        c = np.zeros((64, 4))
        for l in range(64):
            for r in range(4):
                row = 4 * G[l] + r
                if row >= 2 * RH or (row & (RH - 1)) >= self.R or (TOK[l] < 2 * RH and (row < RH) != (TOK[l] < RH)):
                    c[l, r] = NEG
        return c

    def run_q_merged(self):
        """the whole single-tile unit: merged key tile first, then the full key tiles, the odd head's columns shifted back, and the
        epilogue every unit shares; returns (normalised outputs [query][head][HD], row sums [query][head])"""
        KT, RH = self.KT, self.RH
        zero4 = np.zeros((64, 4))
        qm = self.merged_q_operand()
        sc = np.exp2(mfma(self.merged_k_operand(), qm, self.merged_q_cmask()))
        o = mfma(self.merged_v_operand(), np.concatenate([sc, zero4], axis=1), zero4)
        for jb in range(KT // 2):
            p = [np.exp2(mfma(self.k_operand(kt), qm, zero4)) for kt in (2 * jb, 2 * jb + 1)]
            o = mfma(self.v_operand(jb), np.concatenate(p, axis=1), o)
        back = np.zeros((64, 4))                       # row shift left by RH lanes; lanes that receive nothing keep zeros
        for l in range(64):
            if TOK[l] + RH < 16:
                back[l] = o[l + RH]
        out = np.zeros((16, 2, 8))
        for l in range(64):
            out[TOK[l], G[l] >> 1, 4 * (G[l] & 1):4 * (G[l] & 1) + 4] = (o if G[l] < 2 else back)[l]
        sums = out[:, :, HD].copy()
        sums[RH:] = 1.0                                # columns that hold no query of the tile: row sum replaced, the store stays finite
        return out[:, :, :HD] / sums[:, :, None], sums

    def brute_force(self):
        p = np.exp2(self.s - self.s.max(axis=2, keepdims=True))            # [head][query][key < T]
        p /= p.sum(axis=2, keepdims=True)
        return np.einsum("hqk,hdk->qhd", p, self.v[:, :HD, :self.T])


@pytest.mark.parametrize("R", range(1, 9))
@pytest.mark.parametrize("KT", [1, 3])
def test_merged_ragged_key_tile_equals_softmax_over_the_first_T_keys(KT, R):
    u = Unit(KT, R, seed=100 * KT + R)
    ref = u.brute_force()
    plain = u.run(merged=False)
    assert np.abs(plain - ref).max() <= 1e-12, "the restatement of the unmerged unit is wrong"
    got = u.run(merged=True)
    assert np.abs(got - ref).max() <= 1e-12


@pytest.mark.parametrize("R", range(1, 9))
def test_merged_tile_rows_hold_each_key_once_per_head(R):
    """The score tile itself: row rho < RH is key rho of the even head, row RH + rho of the odd head, every other entry is masked."""
    u = Unit(3, R, seed=7 + R)
    RH, k0 = u.RH, 32
    sc = mfma(u.merged_k_operand(), u.q_operand(None), u.merged_cmask())
    tile = np.zeros((16, 16))
    for l in range(64):
        tile[4 * G[l]:4 * G[l] + 4, TOK[l]] = sc[l]
    for row in range(16):
        head, key = row // RH, row % RH
        if row < 2 * RH and key < R:
            want = u.s[head][:, k0 + key] - u.bound[:, head]
            assert np.abs(tile[row] - want).max() <= 1e-12, row
        else:
            assert (tile[row] <= -1e29).all(), row


@pytest.mark.parametrize("R", range(1, 9))
@pytest.mark.parametrize("KT", [1, 3])
def test_merged_ragged_query_tile_equals_softmax_per_head(KT, R):
    """The single-tile units: queries 0 .. RH-1 of the tile (the real ones are 0 .. R-1) come out for both heads; the other lanes
    (their row sum replaced by 1) store finite junk, as the padded queries of every ragged tile do, and cannot fail the bound test."""
    u = Unit(KT, R, seed=300 * KT + R)
    ref = u.brute_force()
    got, sums = u.run_q_merged()
    assert np.abs(got[:u.RH] - ref[:u.RH]).max() <= 1e-12
    assert np.isfinite(got).all() and (sums > 0).all() and np.isfinite(sums).all()
