"""GPU parity: fd_grad_sqnorm, fd_adamw_step and fd_adamw_ema_step (csrc/fd_optim.hip) past the grid cap.  The launch is capped at
num_cu * 8 blocks of 256 threads (524 288 elements on 256 CUs), so every optimizer step of a real model runs several sweeps of the
grid-stride loop, and k_sqnorm_final adds more than 64 block partials; here n = two full sweeps and a ragged third, against the float64
oracle (O.adamw_step, the float64 sum of squares) at the tolerances of the existing n = 257 test (tests/test_gpu_train.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import fdiff_oracle as O

from . import ema_ref as E
from .gpu_util import DEV, dev, host, log_line, report_err

pytestmark = pytest.mark.gpu
HP = (0.9, 0.999, 1e-8, 1e-2)                  # betas, eps, weight decay of the existing optimizer test
# ... as the float32 values the C ABI takes, for the float64 reference: float32(0.999) makes 1 - beta2 smaller by 1.3e-5 relative, which
# the second moment shows in full (the parameter does not: the bias correction is formed from the same float32 beta2)
HP32 = tuple(float(np.float32(h)) for h in HP)
STEPS = 3


def _cap():
    """Threads of the capped grid: one sweep of the loop."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


def _n():
    return 2 * _cap() + 300 + 3


@functools.lru_cache(maxsize=None)
def _data(n):
    """(p0, [g_1 .. g_STEPS]) float32, drawn once and never written."""
    rng = np.random.default_rng(6)
    out = rng.standard_normal(n, dtype=np.float32), [rng.standard_normal(n, dtype=np.float32) for _ in range(STEPS)]
    for a in (out[0], *out[1]):
        a.setflags(write=False)
    return out


def _eng():
    from fourierdiffusion_amd import _C
    return _C, _C.lib(), _C.ctx(torch.device("cuda", torch.cuda.current_device()))


def _sqnorm(g, n):
    _C, L, h = _eng()
    sq = torch.full((3,), 9.0, device=DEV)
    _C.check(L.fd_grad_sqnorm(h, g.data_ptr(), n, sq.data_ptr(), None), h)
    torch.cuda.synchronize()
    assert sq[1] == 9.0 and sq[2] == 9.0
    return sq


def _lr(it):
    return float(np.float32(1e-3 * (it + 1) / 3))


@pytest.mark.parametrize("n", [1, 255, 257, "sweeps"])
def test_grad_sqnorm_vs_float64(n):
    """The kernel accumulates in double and rounds once to float: two float ulps (2.4e-7 relative) hold any n."""
    n = _n() if n == "sweeps" else n
    g = (_data(_n())[1][0][:n] * np.float32(3.0)).astype(np.float32)
    want = float((g.astype(np.float64) ** 2).sum())
    got = float(_sqnorm(dev(g), n)[0].item())
    log_line(f"[parity] fd_grad_sqnorm n={n}: {got:.9g} vs float64 {want:.9g}, rel err {abs(got - want) / want:.3e}")
    np.testing.assert_allclose(got, want, rtol=2.4e-7)


# (gradient factor, max_norm or None for sqnorm = NULL, grad_scale, frozen range relative to the sweep boundary or None)
CASES = {
    "clipping-active": (3.0, 1.0, 1.0, None),
    "clipping-inactive": (1e-5, 1.0, 1.0, None),          # total norm ~ 1e-2: the coefficient clamps to 1
    "no-sqnorm-scale-0.5": (3.0, None, 0.5, None),
    "frozen-across-the-sweep-boundary": (3.0, 1.0, 1.0, (-5, 7)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_adamw_three_steps_past_the_grid_cap(case):
    _C, L, h = _eng()
    factor, max_norm, grad_scale, frozen = CASES[case]
    n, cap = _n(), _cap()
    fz = (cap + frozen[0], cap + frozen[1]) if frozen else (0, 0)
    p0, grads = _data(n)
    p, m, v = dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    rp, rm, rv = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for it in range(STEPS):
        g32 = (grads[it] * np.float32(factor)).astype(np.float32)
        g = dev(g32)
        g64 = g32.astype(np.float64)
        if max_norm is None:
            sq, coef = None, grad_scale
        else:
            sq = _sqnorm(g, n)
            coef = grad_scale * O.clip_grad_norm_scale(np.sqrt((g64 ** 2).sum()) * grad_scale, max_norm)
            assert (coef < 1e-3) if factor > 1 else (coef == 1.0)
        before = [a.clone() for a in (p, m, v)]
        _C.check(L.fd_adamw_step(h, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, it + 1, _lr(it), *HP,
                                 None if sq is None else sq.data_ptr(), 0.0 if max_norm is None else max_norm, grad_scale, fz[0], fz[1],
                                 None), h)
        torch.cuda.synchronize()
        np_, nm, nv = O.adamw_step(rp, g64 * coef, rm, rv, it + 1, _lr(it), *HP32)
        if frozen:
            for new, old in ((np_, rp), (nm, rm), (nv, rv)):
                new[fz[0]:fz[1]] = old[fz[0]:fz[1]]
            for a, b, name in zip((p, m, v), before, "pmv"):
                assert torch.equal(a[fz[0]:fz[1]], b[fz[0]:fz[1]]), (name, it)                      # bit-unchanged inside
                assert bool((a[fz[0] - 64:fz[0]] != b[fz[0] - 64:fz[0]]).all()), (name, it)        # changed on both sides
                assert bool((a[fz[1]:fz[1] + 64] != b[fz[1]:fz[1] + 64]).all()), (name, it)
        rp, rm, rv = np_, nm, nv
        for got, ref, name in ((p, rp, "p"), (m, rm, "m"), (v, rv, "v")):
            if it == STEPS - 1:
                report_err(f"fd_adamw_step n={n} {case} step {it + 1} {name}", host(got), ref)
            np.testing.assert_allclose(host(got), ref, rtol=2e-6, atol=1e-7, err_msg=f"{name} step {it + 1}")
    # every sweep moved its elements: the first, the boundaries, the ragged third
    moved = host(p) != p0
    moved[fz[0]:fz[1]] = True
    for lo in (0, cap - 256, cap + 7, 2 * cap - 256, 2 * cap, n - 303):
        assert moved[lo:lo + 256].all(), lo


def test_adamw_ema_past_the_grid_cap():
    """p, m, v bit-identical to the plain step at the same n; the average within tests/ema_ref.py's bound of the float64 recurrence."""
    _C, L, h = _eng()
    n, cap = _n(), _cap()
    fz = (cap - 5, cap + 7)
    p0, grads = _data(n)
    a = [dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [x.clone() for x in a]
    e0 = _data(n)[1][1]                                    # any start that is not the weights
    ema = dev(e0)
    ps, ds = [], []
    for it in range(STEPS):
        g = dev((grads[it] * np.float32(3.0)).astype(np.float32))
        sq = _sqnorm(g, n)
        d = E.decay_at(it, 0.9, True)
        _C.check(L.fd_adamw_step(h, a[0].data_ptr(), g.data_ptr(), a[1].data_ptr(), a[2].data_ptr(), n, it + 1, _lr(it), *HP,
                                 sq.data_ptr(), 1.0, 1.0, fz[0], fz[1], None), h)
        _C.check(L.fd_adamw_ema_step(h, b[0].data_ptr(), g.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), ema.data_ptr(), d, n, it + 1,
                                     _lr(it), *HP, sq.data_ptr(), 1.0, 1.0, fz[0], fz[1], None), h)
        torch.cuda.synchronize()
        for x, y, name in zip(a, b, "pmv"):
            assert torch.equal(x, y), (name, it)
        ps.append(b[0].cpu().numpy().copy())
        ds.append(d)
    got = host(ema)
    assert np.array_equal(got[fz[0]:fz[1]], e0[fz[0]:fz[1]].astype(np.float64))         # the frozen range keeps its average
    ref = E.recurrence(e0, ps, ds)
    tol = E.tolerance(ps, ref)
    free = np.ones(n, bool)
    free[fz[0]:fz[1]] = False
    err = np.abs(got - ref[-1])
    log_line(f"[parity] fd_adamw_ema_step n={n}: worst |device - float64| / bound = {(err[free] / tol[free]).max():.3f}")
    assert (tol[free] > 0).all() and (err[free] <= tol[free]).all()
    assert (got[free] != e0[free]).mean() > 0.999          # (d e + w p' == e bit for bit is possible for a stray element)
    for lo in (0, cap - 256, cap + 7, 2 * cap - 256, 2 * cap, n - 303):
        assert (got[lo:lo + 256] != e0[lo:lo + 256]).mean() > 0.98, lo
