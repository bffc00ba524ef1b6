#!/usr/bin/env python3
"""One SHA-256 per case over the raw output bytes of the conditional samplers, for fixed seeds: DiffusionSampler.impute,
impute_project and impute_guidance, whose kernels are k_impute (csrc/fd_impute.hip) and k_dps_residual (csrc/fd_dps.hip) on the
coordinate-mask and the window-mean operator (csrc/fd_project.h).  The cases cover every instantiation of the two kernels: both
domains, a shared and a per-series mask, the projection and both gradient modes, window means, RePaint resampling, classifier-free
guidance, the step-wise projection with and without re-noise; each with injected noise and with the engine's Philox stream.  The
shapes are the smallest at which the kernels can go wrong (tests/test_gpu_aggregate.py): a short last window and windows crossing the
4-row quads, a single window, odd T with a second channel block of one channel and Philox groups straddling series and blocks, nine
row tiles on eight waves with a window spanning row tiles.  Only public functions are called, so the same script runs on any commit
that has them: two commits compute the same thing exactly when every line is equal (profiles/conditional_kernels_digest.txt)."""
from __future__ import annotations

import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, N = 3, 4
SHAPES = [((20, 3), 3), ((20, 3), 20), ((37, 17), 2), ((130, 17), 24)]       # ((T, C), window)
K = 3                                                                         # classes of the conditional model


def digest(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def randn(seed: int, *shape) -> torch.Tensor:
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Problem:
    """Observations, masks and the representation of one ((T, C), aggregate)."""

    def __init__(self, T: int, C: int, w: int):
        from fourierdiffusion_amd.sampling.masks import window_means
        rs = np.random.RandomState(1000 * T + 10 * C + w)
        self.T, self.C, self.w = T, C, w
        self.obs = window_means(torch.from_numpy(rs.randn(B, T, C)).float(), w) if w > 1 else torch.from_numpy(rs.randn(B, T, C)).float()
        J = self.obs.shape[1]
        per = rs.rand(B, J, C) < 0.5
        per[:, 0, 0] = True
        self.masks = {"shared": torch.from_numpy(per[0].copy()), "per-series": torch.from_numpy(per)}
        self.mean = torch.from_numpy(rs.randn(T, C)).float()
        self.std = torch.from_numpy(rs.uniform(0.5, 2.0, (T, C))).float()

    def kw(self, fourier: bool) -> dict:
        kw = dict(fourier_transform=fourier, feature_mean=self.mean, feature_std=self.std)
        if self.w > 1:
            kw["aggregate"] = self.w
        return kw

    def noise(self, E: int, Kre: int = 0) -> tuple:
        """Injected noise of one launch of B rows, E executed steps and Kre re-noises: (keyword arguments, obs_noise)."""
        shape = (B, self.T, self.C)
        kw = dict(prior_noise=[randn(1, *shape)], step_noise=[randn(2, E, *shape)])
        if Kre:
            kw["renoise_noise"] = [randn(4, Kre, *shape)]
        return kw, [randn(3, E, *shape)]


def impute_cases(s, p: Problem, tag: str, extra: dict, repaint: bool):
    """impute under the projection and both gradient modes (the projection alone with RePaint), both domains, both masks, injected
    noise and Philox."""
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    E = Kre = 0
    if repaint:
        sched = DiffusionSampler.repaint_schedule(N, 2, 2)
        Kre = sum(1 for op in sched if op[0] == "renoise")
        E = len(sched) - Kre
        extra = dict(extra, resample=2, jump_length=2)
    conds = {"replace": dict(conditioning="replace")}
    if not repaint:
        conds["dps"] = dict(conditioning="dps", guidance_scale=1.0, guidance_jacobian=False)
        conds["dps+jacobian"] = dict(conditioning="dps", guidance_scale=1.0, guidance_jacobian=True)
    for fourier, (mname, mask), (cname, ckw), injected in itertools.product((True, False), p.masks.items(), conds.items(), (True, False)):
        kw = dict(p.kw(fourier), **ckw, **extra)
        if injected:
            nkw, zobs = p.noise(E or N, Kre)
            kw.update(nkw)
            if cname == "replace":
                kw["obs_noise"] = zobs
        torch.manual_seed(7)        # the Philox key of a call comes from torch's CPU generator
        out = s.impute(p.obs, mask, N, **kw)
        yield f"impute {tag} fourier={int(fourier)} mask={mname} {cname} noise={'injected' if injected else 'philox'}", digest(out)


def stepwise_cases(s, p: Problem, tag: str, labels):
    """impute_project (with and without re-noise; the mask alone re-noises) and impute_guidance (both gradient modes)."""
    X = randn(11, B, p.T, p.C).cuda()
    for fourier, (mname, mask) in itertools.product((True, False), p.masks.items()):
        kw = p.kw(fourier)
        agg = {k: v for k, v in kw.items() if k == "aggregate"}
        x0 = s.observed_to_sample_space(p.obs, mask, **kw)
        name = f"{tag} fourier={int(fourier)} mask={mname}"
        if labels is None:
            pkw = dict(fourier_transform=fourier, feature_std=p.std, **agg)
            for t, injected in itertools.product((None, 0.5), (True, False)):
                if t is None and not injected:
                    continue        # the exact projection draws nothing
                torch.manual_seed(8)
                z = randn(12, B, p.T, p.C).cuda() if injected else None
                yield f"impute_project {name} t={t} noise={'injected' if injected else 'philox'}", digest(
                    s.impute_project(X, x0, mask, t, noise=z, **pkw))
                if p.w == 1:
                    torch.manual_seed(9)
                    zr = randn(13, B, p.T, p.C).cuda() if injected else None
                    yield f"impute_project {name} t={t} renoise_to=0.8 noise={'injected' if injected else 'philox'}", digest(
                        s.impute_project(X, x0, mask, t, noise=z, renoise_to=0.8, renoise_noise=zr, **pkw))
        gkw = dict(fourier_transform=fourier, feature_std=p.std, **agg)
        if labels is not None:
            gkw.update(y=labels, cfg_scale=2.0)
        for jac in (False, True):
            yield f"impute_guidance {name} jacobian={int(jac)}", digest(*s.impute_guidance(X, x0, mask, 0.3, jacobian=jac, **gkw))


def cases():
    assert torch.cuda.is_available(), "the digests are of GPU results"
    from fourierdiffusion_amd.sampling.sampler import DiffusionSampler
    from tests.gpu_util import make_model
    from tests.test_gpu_cfg import make_cond
    labels = torch.arange(B) % K
    done = set()
    for (T, C), w in SHAPES:
        cfg = dict(T=T, C=C, D=8, L=1, H=4)
        m, _, _ = make_model(cfg, precision="fp32")
        s = DiffusionSampler(score_model=m, sample_batch_size=2 * B)
        for agg in (1, w):
            if (T, C, agg) in done:
                continue
            done.add((T, C, agg))
            p = Problem(T, C, agg)
            tag = f"T={T} C={C} aggregate={agg}"
            yield from impute_cases(s, p, tag, {}, repaint=False)
            yield from stepwise_cases(s, p, tag, None)
            if agg == 1:
                yield from impute_cases(s, p, tag + " resample=2 jump_length=2", {}, repaint=True)
                mc, _, _, _ = make_cond(cfg, "fp32")
                sc = DiffusionSampler(score_model=mc, sample_batch_size=2 * B)
                guide = dict(y=labels, cfg_scale=2.0)
                yield from impute_cases(sc, p, tag + " cfg_scale=2", guide, repaint=False)
                yield from impute_cases(sc, p, tag + " cfg_scale=2 resample=2 jump_length=2", guide, repaint=True)
                yield from stepwise_cases(sc, p, tag + " cfg_scale=2", labels)


if __name__ == "__main__":
    for name, value in cases():
        print(f"{value}  {name}", flush=True)
