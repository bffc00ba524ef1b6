"""GPU: the input-only VJP (fd_score_input_vjp, ScoreModule.input_vjp) element by element against float64 at dataset shapes.

The reference is tests/autograd_ref.vjp: the oracle network restated on nn.TransformerEncoder in float64 and differentiated by torch
autograd, pinned to the oracle by tests/test_autograd_ref_cpu.py.  Cases and references: tests/shapes_ref.py (computed once).

fp32: 1e-5 of max|ref| (what tests/test_gpu_likelihood.py holds at T = 8), or the kink rule of autograd_ref.explained_by_flips: J
jumps where an FFN pre-activation changes sign, so the comparison may differ by exactly +- g_k d_k for units within tau of their kink
and by nothing else.
bf16: against float64 directly, rms <= 5e-2 and cosine >= 0.998 over the whole tensor (tests/test_gpu_likelihood.py's figures against
the fp32 engine), and per (series, 16-step time tile) a relative rms <= 1e-1 of that tile's own rms: a dropped or garbled tile has
relative rms ~ 1, honest bf16 noise is uniform over tiles.  No tile is left out; every tile's reference rms is asserted >= 0.25 of the
whole tensor's, so that no input change can hollow the check out.

Every measured value is logged by tests/gpu_util.report_err."""
import numpy as np
import pytest

from tests import autograd_ref as A
from tests import shapes_ref as S
from tests.gpu_util import dev, host, make_model, report_err

pytestmark = pytest.mark.gpu


def _vjp(m, x, t, u):
    from fourierdiffusion_amd.utils.dataclasses import DiffusableBatch
    m.train()
    m.dropout = 0.0
    m(DiffusableBatch(X=dev(x), timesteps=dev(t)))
    return host(m.input_vjp(dev(u)))


@pytest.mark.parametrize("name", S.VJP_F32)
def test_input_vjp_fp32_elementwise_vs_float64(name):
    cfg = S.SHAPES[name]
    c = S.vjp_case(name, cfg)
    m, _, _ = make_model(cfg, precision="fp32")
    dx = _vjp(m, c["x"], c["t"], c["u"])
    assert m.train_mode_effective == "fp32"
    report_err(f"input_vjp fp32 {name} T={cfg['T']} C={cfg['C']} L={cfg['L']} vs float64 autograd (tau {c['tau']:.3e}, "
               f"{c['near']} units within tau)", dx, c["ref"])
    ok, plain, left, fits = A.explained_by_flips(dx, c["ref"], c["flips"], 1e-5)
    print(f"input_vjp fp32 {name}: plain {plain:.3e}, after flips {left:.3e}, fitted (row, coefficient / g_k) {fits}")
    assert ok, (plain, left, fits)


def tile_rel_rms(got, ref, tile=16):
    """(worst relative rms of got - ref over the (series, tile-step time tile)s, smallest tile rms of ref / whole-tensor rms)."""
    worst, low = 0.0, np.inf
    whole = np.sqrt((ref ** 2).mean())
    for b in range(ref.shape[0]):
        for t0 in range(0, ref.shape[1], tile):
            r, g = ref[b, t0:t0 + tile], got[b, t0:t0 + tile]
            rr = np.sqrt((r ** 2).mean())
            low = min(low, rr / whole)
            worst = max(worst, float(np.sqrt(((g - r) ** 2).mean()) / rr))
    return worst, float(low)


@pytest.mark.parametrize("tag", list(S.VJP_BF16))
def test_input_vjp_bf16_vs_float64(tag):
    cfg, nb = S.VJP_BF16[tag]
    c = S.vjp_case(f"bf16_{tag}", cfg, nb, flips=False)
    m, _, _ = make_model(cfg, precision="bf16")
    dx = _vjp(m, c["x"], c["t"], c["u"])
    assert m.train_mode_effective == "bf16"
    ref = c["ref"]
    err, rms = report_err(f"input_vjp bf16 {tag} T={cfg['T']} C={cfg['C']} D={cfg['D']} L={cfg['L']} B={nb} vs float64 autograd", dx, ref)
    a, b = dx.ravel(), ref.ravel()
    cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    worst, low = tile_rel_rms(dx, ref)
    report_err(f"input_vjp bf16 {tag} worst (series, 16-step tile) relative rms {worst:.3e}, cosine {cos:.6f}, smallest tile rms "
               f"of the reference {low:.2f} of the whole", dx, ref)
    assert low >= 0.25, low
    assert rms <= 5e-2 and cos >= 0.998, (rms, cos)
    assert worst <= 1e-1, worst
