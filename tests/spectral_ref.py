"""Float64 reference of the spectral features (include/fdiff_hip.h, fd_series_spectra): Welch's averaged periodogram straight from
the definitions (numpy's rfft of every centred, windowed segment), the derived per-entry error bound, a float32 restatement of the
engine's arithmetic and the metric's arithmetic on set means.  numpy only; the engine is never called here.

Definitions (scipy.signal.welch / csd at fs = 1, scaling = "density", one-sided), per series x (T, C):
    segments of S = nperseg points at 0, H, 2 H, ... (H = S - noverlap) while start + S <= T; v = (segment - its mean) w
    F[k, c] = sum_s v[s, c] exp(-2 pi i k s / S),  k = 0..K-1,  K = S // 2 + 1
    P[k, c, d] = scale_k / (nseg sum w^2) sum_seg conj(F[k, c]) F[k, d],   scale_k = 2, 1 at k = 0 and at the Nyquist bin of an even S
    psd[k, c] = P[k, c, c];  csd[k, p] = (Re, Im) P[k, c, d] for the pairs c < d in row-major order
    summary[c] = (sum_k psd,  sum_{k>=1} (k / S) psd / sum_{k>=1} psd,  -sum_{k>=1} p ln p / ln(K - 1)),  p_k = psd_k / sum_{k>=1} psd
A channel whose S entries are bit-equal in EVERY segment has v = 0: its psd, every csd entry it takes part in and its summaries are 0;
K = 2 gives entropy 0."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32
V64 = 2.0 ** -53          # and of float64
CHUNK_SERIES = 32         # the engine's chunk of the set means (fd_spectral.hip, SPEC_CHUNK)
WINDOWS = {"boxcar": 0, "hann": 1}

# the GPU test's cases (tests/test_gpu_spectral.py); the CPU test checks the bound on the same inputs
# (n, T, C, S, noverlap)
CASES = {
    "lower_ends": (1, 2, 1, 2, 0),
    "odd_S_hop_1": (3, 9, 2, 7, 6),
    "ecg": (7, 187, 1, 93, 46),
    "mimic": (5, 24, 40, 24, 12),
    "droughts": (4, 365, 13, 182, 91),
    "T_limit": (3, 1024, 2, 256, 128),
    "odd_everything": (65, 20, 17, 8, 3),
    "chunk_boundaries": (3 * CHUNK_SERIES + 1, 16, 3, 8, 4),
}
# (window, detrend): the kernel branches on detrend, the table build on the window
VARIANTS = [("hann", True), ("boxcar", False), ("boxcar", True), ("hann", False)]


@dataclass
class Spectra:
    psd: np.ndarray                   # (n, K, C)
    csd: Optional[np.ndarray]         # (n, K, NP, 2) or None for one channel
    summary: np.ndarray               # (n, C, 3)

    def flat(self) -> np.ndarray:
        """(n, F) in the engine's order psd | csd | summary."""
        n = self.psd.shape[0]
        parts = [self.psd.reshape(n, -1)]
        if self.csd is not None:
            parts.append(self.csd.reshape(n, -1))
        parts.append(self.summary.reshape(n, -1))
        return np.concatenate(parts, axis=1)

    def set_mean(self) -> np.ndarray:
        return self.flat().mean(axis=0)

    def astype(self, dtype) -> "Spectra":
        return Spectra(self.psd.astype(dtype), None if self.csd is None else self.csd.astype(dtype), self.summary.astype(dtype))


def get_window(window: str, S: int) -> np.ndarray:
    if window == "boxcar":
        return np.ones(S)
    assert window == "hann"
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(S) / S)             # periodic: scipy.signal.get_window("hann", S)


def pairs(C: int):
    c, d = np.triu_indices(C, k=1)                                          # row-major order of the pairs c < d
    return c, d


def _segments(x: np.ndarray, S: int, noverlap: int) -> np.ndarray:
    """(n, nseg, S, C)"""
    n, T, C = x.shape
    assert 2 <= S <= T and 0 <= noverlap <= S - 1
    starts = np.arange(0, T - S + 1, S - noverlap)
    return x[:, starts[:, None] + np.arange(S)[None, :], :]


def _scale(S: int) -> np.ndarray:
    K = S // 2 + 1
    scale = np.full(K, 2.0)
    scale[0] = 1.0
    if S % 2 == 0:
        scale[-1] = 1.0
    return scale


def _centred(seg: np.ndarray, detrend: bool):
    """The centred segments and where they are exactly zero (a constant segment under detrend)."""
    if not detrend:
        return seg.copy(), np.zeros(seg.shape[:2] + seg.shape[3:], dtype=bool)
    const = (seg == seg[:, :, :1, :]).all(axis=2)                           # (n, nseg, C)
    e = seg - seg.mean(axis=2, keepdims=True)
    e[np.broadcast_to(const[:, :, None, :], e.shape)] = 0.0
    return e, const


def _summaries(psd: np.ndarray, S: int) -> np.ndarray:
    """(n, C, 3) from a float64 psd (n, K, C)."""
    n, K, C = psd.shape
    tail = psd[:, 1:, :]
    tot = tail.sum(axis=1)
    live = tot > 0
    safe = np.where(live, tot, 1.0)
    f = np.arange(1, K) / S
    centroid = np.where(live, (f[None, :, None] * tail).sum(axis=1) / safe, 0.0)
    p = tail / safe[:, None, :]
    plogp = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    entropy = np.where(live & (K > 2), -plogp.sum(axis=1) / (np.log(K - 1) if K > 2 else 1.0), 0.0)
    return np.stack([psd.sum(axis=1), centroid, entropy], axis=-1)


def _from_dft(A: np.ndarray, B: np.ndarray, S: int, sw2: float) -> Spectra:
    """A, B (n, nseg, K, C) float64: F = A - i B.  Everything after the DFT, in float64."""
    n, nseg, K, C = A.shape
    norm = _scale(S) / (nseg * sw2)
    psd = (A * A + B * B).sum(axis=1) * norm[None, :, None]
    csd = None
    if C > 1:
        c, d = pairs(C)
        re = (A[..., c] * A[..., d] + B[..., c] * B[..., d]).sum(axis=1) * norm[None, :, None]
        im = (B[..., c] * A[..., d] - A[..., c] * B[..., d]).sum(axis=1) * norm[None, :, None]
        csd = np.stack([re, im], axis=-1)
    return Spectra(psd, csd, _summaries(psd, S))


def spectra_f64(x, S: int, noverlap: int, window: str = "hann", detrend: bool = True) -> Spectra:
    """The float64 reference.  x (n, T, C)."""
    x = np.asarray(x, dtype=np.float64)
    w = get_window(window, S)
    e, _ = _centred(_segments(x, S, noverlap), detrend)
    F = np.fft.rfft(e * w[None, None, :, None], axis=2)                     # (n, nseg, K, C)
    return _from_dft(F.real, -F.imag, S, float((w * w).sum()))


def basis_f32(S: int):
    """cos and sin (K, S) of the engine's basis: float64 with the angle reduced in integers first, rounded to float32 once."""
    K = S // 2 + 1
    m = (np.arange(K)[:, None] * np.arange(S)[None, :]) % S
    a = 2.0 * np.pi * m / S
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


def _fma32(acc: np.ndarray, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """float32 fma: the product of two floats is exact in float64 (the sum then rounds twice, a 2^-29 relative event)."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def spectra_f32(x, S: int, noverlap: int, window: str = "hann", detrend: bool = True) -> Spectra:
    """Restatement of the engine's arithmetic: the segment sum in float64, v = float32(((S x - sum) (1 / S)) w) with everything before
    the rounding in float64, the basis in float32, the DFT a float32 fma chain in the kernel's order (two accumulators: the terms
    s = 16 j + 4 q + i go to accumulator i mod 2 in the order (j, i, q); their sum), float64 from there on.  float32 enters exactly
    where it does in the kernel; what differs is the order of the float64 additions."""
    x32 = np.asarray(x, dtype=np.float32)
    seg = _segments(x32.astype(np.float64), S, noverlap)
    w = get_window(window, S)
    if detrend:
        e = (S * seg - seg.sum(axis=2, keepdims=True)) * (1.0 / S)
    else:
        e = seg
    v = (e * w[None, None, :, None]).astype(np.float32)                     # (n, nseg, S, C)
    cos32, sin32 = basis_f32(S)
    K = S // 2 + 1
    shape = (v.shape[0], v.shape[1], K, v.shape[3])
    acc = {("c", 0): np.zeros(shape, np.float32), ("c", 1): np.zeros(shape, np.float32),
           ("s", 0): np.zeros(shape, np.float32), ("s", 1): np.zeros(shape, np.float32)}
    for j in range(0, S, 16):
        for i in range(4):
            for q in range(4):
                s = j + 4 * q + i
                if s >= S:
                    continue                                                # the padding adds fma(0, 0, acc) = acc
                vs = v[:, :, s, None, :]
                acc[("c", i % 2)] = _fma32(acc[("c", i % 2)], cos32[None, None, :, s, None], vs)
                acc[("s", i % 2)] = _fma32(acc[("s", i % 2)], sin32[None, None, :, s, None], vs)
    A = (acc[("c", 0)] + acc[("c", 1)]).astype(np.float64)
    B = (acc[("s", 0)] + acc[("s", 1)]).astype(np.float64)
    out = _from_dft(A, B, S, float((w * w).sum()))
    # the summaries come from the double psd; the arrays are returned in float32
    return Spectra(out.psd.astype(np.float32), None if out.csd is None else out.csd.astype(np.float32), out.summary.astype(np.float32))


def _phi(t):
    """-t ln t, 0 at 0."""
    t = np.asarray(t, dtype=np.float64)
    return np.where(t > 0, -t * np.log(np.where(t > 0, t, 1.0)), 0.0)


def error_bounds(x, S: int, noverlap: int, window: str = "hann", detrend: bool = True, mean_of=None) -> Spectra:
    """Per-entry bound on |engine - float64 reference| (include/fdiff_hip.h), derived, nothing tuned.  u = 2^-24,
    v = 2^-53, gamma_m = m u / (1 - m u).

    The segment entry.  The engine's v~_s = v_s + eta_s with |eta_s| <= h_s = (u + 4 v) |v_s| + rho w_s: one float32 rounding, the
    double product, quotient and difference, and rho = (S + 2) v max_s |x_s| for the double sum of the S entries (0 without detrend;
    a constant segment is exact).
    The DFT.  A~ = fl32(sum_s b~_s v~_s) with b~ = b (1 + delta), |delta| <= u (+ the double cosine, inside the +1 below), |b| <= 1,
    an fma chain of at most S / 2 terms per accumulator and one final addition: at most S roundings stand over a term, so
        |A~ - A| <= eps = sum_s h_s + gamma_{S+1} sum_s (|v_s| + h_s),                                              likewise for B.
    The bound scales with the segment's 1-norm, hence with sqrt(S x the channel's total power), not with |F[k]| at the bin.
    The cross-spectrum.  conj(F_c) F_d = A_c A_d + B_c B_d + i (B_c A_d - A_c B_d); with |A| + |B| <= sqrt(2) |F| each part moves by
    at most sqrt(2) (eps_c |F_d| + eps_d |F_c|) + 2 eps_c eps_d per segment; the double sum over segments and the scaling add
    (nseg + 4) 2 v of the sum of the absolute terms; the returned float32 adds u |P| (+ the subnormal step 2^-150).
    The summaries are formed from the DOUBLE psd (its bound dP without the u |P|): total power sum_k dP_k; centroid N / D by the
    quotient rule (dN + centroid dD) / (D - dD) with dN = sum f_k dP_k, dD = sum_{k>=1} dP_k; entropy through p_k = P_k / D,
    |dp_k| <= delta_k = (dP_k + p_k dD) / (D - dD), and for phi(t) = -t ln t either the mean-value bound delta_k (|ln(p_k / 2)| + 1)
    when delta_k <= p_k / 2, or |phi(a) - phi(b)| <= phi(|a - b|) for |a - b| <= 1/2 (else the trivial ln(K - 1)); each divided by
    ln(K - 1), plus u |value| for the returned float32 and 8 (K + 4) v for the double chains and logarithms.  Centroid and entropy lie
    in [0, 1/2] and [0, 1]: the bounds are capped there.
    `mean_of`: the array whose max |x| sets rho when the features are compared with those of ANOTHER (unshifted) array."""
    x = np.asarray(x, dtype=np.float64)
    n, T, C = x.shape
    w = get_window(window, S)
    sw2 = float((w * w).sum())
    seg = _segments(x, S, noverlap)
    nseg, K = seg.shape[1], S // 2 + 1
    e, const = _centred(seg, detrend)
    vabs = np.abs(e * w[None, None, :, None])                               # (n, nseg, S, C)
    if detrend:
        big = np.abs(_segments(x if mean_of is None else np.asarray(mean_of, dtype=np.float64), S, noverlap)).max(axis=2)
        rho = np.where(const, 0.0, (S + 2) * V64 * big)                     # (n, nseg, C)
    else:
        rho = np.zeros((n, nseg, C))
    h = (U32 + 4 * V64) * vabs + rho[:, :, None, :] * w[None, None, :, None]
    gamma = (S + 1) * U32 / (1 - (S + 1) * U32)
    eps = h.sum(axis=2) + gamma * (vabs + h).sum(axis=2)                    # (n, nseg, C)
    F = np.fft.rfft(e * w[None, None, :, None], axis=2)
    Fa = np.abs(F)                                                          # (n, nseg, K, C)
    norm = (_scale(S) / (nseg * sw2))[None, :, None]
    chain = (nseg + 4) * 2 * V64
    r2 = np.sqrt(2.0)
    ec = eps[:, :, None, :]

    def pair_bound(c, d):
        per_seg = r2 * (ec[..., c] * Fa[..., d] + ec[..., d] * Fa[..., c]) + 2 * ec[..., c] * ec[..., d]
        mag = (Fa[..., c] + ec[..., c]) * (Fa[..., d] + ec[..., d])
        return (per_seg.sum(axis=1) + chain * 2 * mag.sum(axis=1)) * norm   # (n, K, len)

    ref = spectra_f64(x, S, noverlap, window, detrend)
    idx = np.arange(C)
    dP = pair_bound(idx, idx)                                               # the double psd
    b_psd = dP + U32 * (np.abs(ref.psd) + dP) + 2.0 ** -150
    b_csd = None
    if C > 1:
        c, d = pairs(C)
        dQ = pair_bound(c, d)
        mag = np.sqrt(ref.csd[..., 0] ** 2 + ref.csd[..., 1] ** 2)
        b = dQ + U32 * (mag + dQ) + 2.0 ** -150
        b_csd = np.stack([b, b], axis=-1)
    small = 8 * (K + 4) * V64
    total, centroid, entropy = ref.summary[..., 0], ref.summary[..., 1], ref.summary[..., 2]
    b_total = dP.sum(axis=1) + (U32 + small) * (total + dP.sum(axis=1)) + 2.0 ** -150
    tail, dtail = ref.psd[:, 1:, :], dP[:, 1:, :]
    D, dD = tail.sum(axis=1), dtail.sum(axis=1)
    dead = D == 0
    ok = ~dead & (D > dD)
    den = np.where(ok, D - dD, 1.0)
    f = (np.arange(1, K) / S)[None, :, None]
    b_cent = np.where(ok, ((f * dtail).sum(axis=1) + centroid * dD) / den, 0.5)
    b_cent = np.where(dead, 0.0, np.minimum(b_cent * (1 + U32) + (U32 + small) * centroid + 2.0 ** -150, 0.5))
    if K > 2:
        p = tail / np.where(dead, 1.0, D)[:, None, :]
        delta = np.where(ok[:, None, :], (dtail + p * dD[:, None, :]) / den[:, None, :], 1.0)
        smooth = delta * (np.abs(np.log(np.where(p > 0, p / 2, 1.0))) + 1.0)
        rough = np.where(delta <= 0.5, _phi(np.minimum(delta, 0.5)), np.log(K - 1))
        per_bin = np.where((p > 0) & (delta <= p / 2), smooth, rough)
        b_ent = per_bin.sum(axis=1) / np.log(K - 1)
        b_ent = np.where(dead, 0.0, np.minimum(b_ent * (1 + U32) + (U32 + small) * entropy + 2.0 ** -150, 1.0))
    else:
        b_ent = np.zeros_like(entropy)
    return Spectra(b_psd, b_csd, np.stack([b_total, b_cent, b_ent], axis=-1))


# ---------------------------------------------------------------------------------------------- set level and the metric's arithmetic
def full_csd(psd_mean: np.ndarray, csd_mean: Optional[np.ndarray]) -> np.ndarray:
    """(K, C, C) complex Hermitian from the set means psd (K, C) and csd (K, NP, 2)."""
    K, C = psd_mean.shape
    P = np.zeros((K, C, C), dtype=np.complex128)
    idx = np.arange(C)
    P[:, idx, idx] = psd_mean
    if C > 1:
        c, d = pairs(C)
        z = csd_mean[..., 0] + 1j * csd_mean[..., 1]
        P[:, c, d] = z
        P[:, d, c] = np.conj(z)
    return P


def coherence(P: np.ndarray) -> np.ndarray:
    """|P_cd|^2 / (P_cc P_dd), 0 where a denominator is 0."""
    diag = np.einsum("kcc->kc", P).real
    den = diag[:, :, None] * diag[:, None, :]
    return np.where(den > 0, np.abs(P) ** 2 / np.where(den > 0, den, 1.0), 0.0)


def w2_marginals(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Wasserstein-2 per column between two (n, k) / (m, k) samples with uniform weights (tests/dependence_ref.py's)."""
    a, b = np.sort(np.asarray(a, dtype=np.float64), axis=0), np.sort(np.asarray(b, dtype=np.float64), axis=0)
    n, m = a.shape[0], b.shape[0]
    grid = np.unique(np.concatenate([np.arange(n + 1) / n, np.arange(m + 1) / m]))
    mid, width = 0.5 * (grid[1:] + grid[:-1]), np.diff(grid)
    ia, ib = np.minimum((mid * n).astype(int), n - 1), np.minimum((mid * m).astype(int), m - 1)
    return np.sqrt((width[:, None] * (a[ia] - b[ib]) ** 2).sum(axis=0))


def metric_values(fs: Spectra, fr: Spectra, suffix: str = "") -> dict:
    """The keys of SpectralDependence from the features of the samples (fs) and of the real set (fr), in float64."""
    out = {}
    K, C = fs.psd.shape[1:]
    ps, pr = fs.psd.mean(axis=0), fr.psd.mean(axis=0)
    floor_s, floor_r = 1e-12 * fs.summary[..., 0].mean(axis=0), 1e-12 * fr.summary[..., 0].mean(axis=0)
    ps, pr = np.maximum(ps, floor_s[None, :]), np.maximum(pr, floor_r[None, :])
    ok = (ps[1:] > 0) & (pr[1:] > 0)
    d = np.where(ok, np.abs(10.0 * np.log10(np.where(ok, ps[1:], 1.0) / np.where(ok, pr[1:], 1.0))), 0.0)
    out[f"psd_log_distance{suffix}"], out[f"psd_log_distance_max{suffix}"] = float(d.mean()), float(d.max())
    if C > 1:
        Ps = full_csd(fs.psd.mean(axis=0), fs.csd.mean(axis=0))
        Pr = full_csd(fr.psd.mean(axis=0), fr.csd.mean(axis=0))
        c, dd = pairs(C)
        cs, cr = coherence(Ps)[1:, c, dd], coherence(Pr)[1:, c, dd]
        dc = np.abs(cs - cr)
        out[f"coherence_distance{suffix}"], out[f"coherence_distance_max{suffix}"] = float(dc.mean()), float(dc.max())
        dphi = np.angle(Ps[1:, c, dd]) - np.angle(Pr[1:, c, dd])
        dphi = np.abs((dphi + np.pi) % (2 * np.pi) - np.pi)
        if cr.sum() > 0:
            out[f"phase_distance{suffix}"] = float((cr * dphi).sum() / cr.sum())
    for i, name in ((1, "spectral_centroid_wasserstein"), (2, "spectral_entropy_wasserstein")):
        out[f"{name}{suffix}"] = float(w2_marginals(fs.summary[..., i], fr.summary[..., i]).mean())
    return out


def ar1(rng: np.random.Generator, n: int, T: int, phi: float) -> np.ndarray:
    """(n, T) stationary AR(1) with unit innovations."""
    x = np.empty((n, T))
    x[:, 0] = rng.standard_normal(n) / np.sqrt(1 - phi * phi)
    eps = rng.standard_normal((n, T))
    for t in range(1, T):
        x[:, t] = phi * x[:, t - 1] + eps[:, t]
    return x


def delayed_coupling(seed: int = 0, n: int = 512, T: int = 128, delay: int = 20, phi: float = 0.5, noise: float = 0.3):
    """The experiment of DESIGN.md 3.34: `real` (n, T, 2) has channel 1 = channel 0 delayed by `delay` steps plus noise; `fake` has
    the same two marginal processes, independent of each other."""
    rng = np.random.default_rng(seed)

    def coupled(source):
        return np.stack([source[:, delay:], source[:, :T] + noise * rng.standard_normal((n, T))], axis=-1)

    real = coupled(ar1(rng, n, T + delay, phi))
    fake = np.stack([ar1(rng, n, T + delay, phi)[:, delay:], coupled(ar1(rng, n, T + delay, phi))[..., 1]], axis=-1)
    return real, fake


def make_series(name: str) -> np.ndarray:
    """The inputs of a GPU case, float64 on the 1/1024 grid."""
    n, T, Cn, S, ov = CASES[name]
    rs = np.random.RandomState(len(name) * 100 + n + T + Cn)
    x = np.cumsum(rs.standard_normal((n, T, Cn)), axis=1) * 0.4 + rs.standard_normal((n, 1, Cn)) * 2.0 + rs.standard_normal((n, T, Cn))
    if Cn > 1:
        x[:, 1:, 1] += 0.8 * x[:, :-1, 0]                                  # a coupling for the cross-spectra to see
    x *= np.exp(rs.uniform(-2, 2, size=(1, 1, Cn)))                         # a different scale per channel
    return np.round(x * 1024) / 1024                                        # on a grid: x + 1000 stays exact in float32


def reference_series_spectra(X, nperseg=None, noverlap=None, *, window="hann", detrend="constant", per_series=("psd", "summary")):
    """utils.spectral.series_spectra's result from the float64 reference (the CPU tests' stand-in for the engine)."""
    import torch

    from fourierdiffusion_amd.utils.spectral import SeriesSpectra, assemble_set_mean, resolve_segments
    x = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
    n, T, Cn = x.shape
    S, ov = resolve_segments(T, nperseg, noverlap)
    f = spectra_f64(x, S, ov, window, detrend == "constant")
    return SeriesSpectra(psd=torch.from_numpy(f.psd) if "psd" in per_series else None,
                         csd=torch.from_numpy(f.csd) if "csd" in per_series else None,
                         summary=torch.from_numpy(f.summary) if "summary" in per_series else None,
                         set_mean=assemble_set_mean(torch.from_numpy(f.set_mean()), S // 2 + 1, Cn),
                         freqs=torch.arange(S // 2 + 1, dtype=torch.float64) / S, nperseg=S, noverlap=ov,
                         n_segments=(T - S) // (S - ov) + 1)
