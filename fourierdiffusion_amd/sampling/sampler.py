"""DiffusionSampler on the HIP engine -- same surface as fdiff.sampling.sampler.DiffusionSampler
(reference: src/fdiff/sampling/sampler.py:11-122).

Kept from the reference: batching rule ``max(1, num_samples // sample_batch_size)`` with the remainder
silently dropped (sampler.py:63), every grid point of ``linspace(1, eps, N)`` visited including t=eps
with noise still added, output on the CPU.  Changed underneath: the prior is drawn on the device, and
the N-step loop is ONE engine call (fd_sampler_run) with no per-step host synchronisation instead of
N Python iterations each ending in ``.item()`` (sampler.py:37).

Launch sizes (round 5): ``sample_batch_size`` is a memory knob of the reference (its default, 200 -- cmd/conf/sampler/
default.yaml -- with num_samples = 10 000, cmd/conf/sample.yaml); series never interact, so the SAME
``num_batches * batch_size`` series are handed to the engine in launches sized for the device: the persistent kernel
packs S series per workgroup and wants S x (number of CUs) of them per launch (512 at T = 100 on MI355X: 1190
series/s against 600 with launches of 200).  Injected-noise calls (parity tests) keep one launch per batch;
``merge_batches=False`` / FDIFF_SAMPLER_MERGE=0 keep the reference's launches.

Conditional sampling (an extension, not in the reference): ``impute`` fills in the unobserved entries of time-domain series
(imputation, forecasting) by projecting the state onto the observations after every reverse step (Song et al. 2021, Sec. 5,
App. I.2), the step and the projection fused in one engine launch (fd_sampler_run_impute); ``impute_project`` is the
projection alone.  ``impute(..., num_samples=K)`` draws an ensemble of K samples per series as K state rows that read one
observation row in place (fd_sampler_run_impute_rep); ``sampling.forecast`` scores such ensembles.

Probability-flow ODE (an extension, not in the reference): ``sample_ode`` integrates the deterministic ODE with the reverse SDE's
marginals (Song et al. 2021, Sec. 4.3) by Euler or Heun, the whole loop one engine call (fd_sampler_run_ode); ``encode`` /
``decode`` run it data -> latents and back.  ``ODESampler`` is a DiffusionSampler whose ``sample`` is ``sample_ode``
(hydra: ``sampler=ode``).  ``solver="ddim"`` / ``"dpmpp2m"`` sample the same ODE with the data-prediction exponential integrator
(DPM-Solver++, Lu et al. 2022: one evaluation per step, first order or second-order multistep; fd_sampler_run_dpm), and
``schedule="logsnr"`` puts any solver on a grid uniform in the log signal-to-noise ratio (hydra: ``sampler=dpm``).
``sample_ode_adaptive`` / ``encode_adaptive`` / ``decode_adaptive`` take a tolerance instead of a step count: Dormand-Prince 5(4)
under the step control of scipy's RK45, every row on its own grid (fd_sampler_run_ode_adaptive; ``AdaptiveODESampler``, hydra:
``sampler=ode_adaptive``); they evaluate the network step by step and report what the tolerance cost (``ODEInfo``).

Likelihood (an extension, not in the reference): ``log_likelihood`` evaluates log p(x) under the probability-flow ODE
(Song et al. 2021, Sec. 4.3, App. D.2): the ODE runs data -> latents with the divergence integral along it, one engine call
per launch (fd_likelihood_run); ``sampling.likelihood.to_data_space`` maps the result to the series as the user holds them.

Classifier-free guidance (an extension, not in the reference): on a class-conditional model (``ScoreModule(n_classes=K)``),
``sample`` / ``sample_ode`` take labels ``y`` and a guidance scale ``cfg_scale`` = w and follow the score
w s(x, t, y) + (1 - w) s(x, t, null): one evaluation per step at w = 1 (class-conditional sampling) and w = 0, else the two
evaluations as one forward on twice the rows and one fused step kernel (fd_sampler_run_cfg, fd_sampler_run_ode_cfg).
``impute`` (both conditionings, ensembles included) and ``impute_guidance`` take ``y`` (one label per series) and ``cfg_scale`` the
same way (fd_sampler_run_impute_cfg, fd_sampler_run_impute_dps_cfg, fd_impute_guidance_cfg), and ``log_likelihood`` takes ``y`` and
evaluates log p(x | y) -- no ``cfg_scale``: a guided vector field is the probability-flow ODE of no density.  The
predictor-corrector sampler and ``encode`` / ``decode`` take no labels and run a labelled model unconditionally.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from .. import _C, _rng
from ..models.score_models import _PRECISIONS, ScoreModule
from ..schedulers.sde import SDE
from ..utils.dataclasses import DiffusableBatch
from ..utils.fourier import dft, dft_standardize
from .masks import LinearOperator, as_operator
from .likelihood import ESTIMATORS, EXACT_MAX_DIMS, RK45_MAX_EVALS, LikelihoodResult, drift_divergence, drift_integral


@dataclass
class SMCInfo:
    """What ``impute(conditioning="smc", return_info=True)`` reports next to its samples, for n series, K particles and N steps (CPU
    tensors).  log_evidence (n,) float64: the estimate of log p(y), the Gaussian constant included, -inf for a degenerate series;
    log_weights (n, K) float64: the final log weights (0 after a final resample); ess (N + 1, n) float64, resampled (N + 1, n) bool
    and ancestors (N + 1, n, K) int32 (index inside the series) of every stage; degenerate (n,) bool: every particle of the series
    lost its weight (no resampling from then on)."""
    log_evidence: torch.Tensor
    log_weights: torch.Tensor
    ess: torch.Tensor
    resampled: torch.Tensor
    ancestors: torch.Tensor
    degenerate: torch.Tensor


@dataclass
class ODEInfo:
    """What the adaptive ODE calls (``sample_ode_adaptive``, ``encode_adaptive``, ``decode_adaptive``) report with return_info, for
    n rows (CPU tensors).  nfe (n,) int64: score evaluations as scipy's nfev (2 + 6 per attempted step); converged (n,) bool;
    status (n,) int64: 1 converged, 2 step under scipy's min_step, 3 the next attempt would pass max_evals; grid (n, S) float64: the
    accepted times, the start first, NaN-padded; rtol, atol: as given; row_evals_launched: the state rows the engine launched,
    summed over the evaluations of every launch; row_evals_needed = nfe.sum(), what the rows themselves consumed."""
    nfe: torch.Tensor
    converged: torch.Tensor
    status: torch.Tensor
    grid: torch.Tensor
    rtol: float
    atol: float
    row_evals_launched: int
    row_evals_needed: int


class DiffusionSampler:
    def __init__(self, score_model: ScoreModule, sample_batch_size: int, corrector_steps: int = 0, snr: float = 0.16,
                 merge_batches: bool = True, cfg_scale: float = 1.0, labels=None, covariates=None) -> None:
        """corrector_steps > 0 turns the predictor-only sampler of the reference into a predictor-corrector one
        (`corrector_steps` Langevin steps at signal-to-noise ratio `snr` before every predictor step; an extension, not in
        the reference: default off).  cfg_scale / labels: the front end's guidance settings (cmd/conf/sampler/*.yaml), kept for
        cmd/sample.py, which turns ``labels`` into the ``y`` of ``sample``; ``sample`` itself takes both as arguments.  covariates:
        the same for a covariate-conditional model (``parse_covariates``)."""
        self.cfg_scale = float(cfg_scale)
        self.labels = labels
        self.covariates = covariates
        self.corrector_steps = int(corrector_steps)
        self.snr = float(snr)
        self.score_model = score_model
        self.noise_scheduler = score_model.noise_scheduler
        self.sample_batch_size = sample_batch_size
        self.merge_batches = bool(merge_batches) and os.environ.get("FDIFF_SAMPLER_MERGE", "1") != "0"
        self.n_channels = score_model.n_channels
        self.max_len = score_model.max_len

    def reverse_diffusion_step(self, batch: DiffusableBatch, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One score evaluation + one SDE step (sampler.py:24-43); the fused loop in ``sample`` does not
        call this, it exists for API parity and step-wise debugging."""
        X, timesteps = batch.X, batch.timesteps
        assert timesteps is not None and timesteps.size(0) == len(batch)
        assert torch.min(timesteps) == torch.max(timesteps)
        score = self.score_model(batch)
        out = self.noise_scheduler.step(model_output=score, timestep=timesteps[0].item(), sample=X, noise=noise)
        return out.prev_sample

    def sample(self, num_samples: int, num_diffusion_steps: Optional[int] = None,
               prior_noise: Optional[Sequence[torch.Tensor]] = None,
               step_noise: Optional[Sequence[torch.Tensor]] = None,
               corrector_noise: Optional[Sequence[torch.Tensor]] = None, y=None, cfg_scale: float = 1.0) -> torch.Tensor:
        """Returns a CPU tensor (n, max_len, n_channels), n = num_batches * batch_size.

        prior_noise[b] (bs,T,C) and step_noise[b] (N,bs,T,C) inject the N(0,1) draws of batch b (parity
        tests); by default everything comes from the engine's Philox stream.

        y, cfg_scale (class-conditional models only; ValueError otherwise): the labels -- an int, or an integer tensor with one
        label per returned sample -- and the classifier-free guidance scale w.  y=None samples unconditionally; w = 1 samples the
        class, w > 1 trades diversity for class fidelity (two score evaluations per step, run as one forward on 2 x the rows)."""
        guided, pair = self._guided(y, cfg_scale)
        if guided and self.corrector_steps > 0:
            raise ValueError("sample: y / cfg_scale are not supported by the predictor-corrector sampler (corrector_steps=0)")
        self.score_model.eval()
        N, ts_arr, dt = self._sde_grid(num_diffusion_steps)
        ctx, h, p, G, mode = self._engine_args()
        all_samples: List[torch.Tensor] = []
        injected = not (prior_noise is None and step_noise is None and corrector_noise is None)
        sizes = self._batches(num_samples, mode, injected, pair=pair)
        labels = self._labels(y, sum(sizes)) if guided else None
        lo = 0
        for b, bs in enumerate(sizes):
            X = self.sample_prior(bs, noise=None if prior_noise is None else prior_noise[b])
            z = None if step_noise is None else self._noise(step_noise[b], (N, bs), "step_noise")
            key, off = (0, 0) if z is not None else _rng.stream()
            if guided:
                yb = None if labels is None else labels[lo:lo + bs].contiguous()
                lo += bs
                X = self._cfg_state(X, pair)      # (the state buffer is all a guided launch differs in, besides its entry point)
                run_guided = _C.lib().fd_sampler_run_cov if self.score_model.cond_dim > 0 else _C.lib().fd_sampler_run_cfg
                rc = run_guided(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), _C.ptr(yb),
                                                 float(cfg_scale), _C.ptr(z), key, off, bs, mode, _C.stream_of(X))
            elif self.corrector_steps > 0:
                zc = None
                if corrector_noise is not None:
                    zc = self._noise(corrector_noise[b], (N, self.corrector_steps, bs), "corrector_noise")
                if zc is None and z is not None:
                    key, off = _rng.stream()
                rc = _C.lib().fd_sampler_run_pc(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), _C.ptr(z), _C.ptr(zc),
                                                self.corrector_steps, self.snr, key, off, bs, mode, _C.stream_of(X))
            else:
                rc = _C.lib().fd_sampler_run(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), _C.ptr(z),
                                             key, off, bs, mode, _C.stream_of(X))
            _C.check(rc, ctx)
            all_samples.append(X[:bs])
        return torch.cat([x.cpu() for x in all_samples], dim=0)

    # ------------------------------------------------------------ probability-flow ODE (extension, not in the reference)
    _SOLVERS = {"euler": 0, "heun": 1}
    _DPM_SOLVERS = {"ddim": 2, "dpmpp2m": 3}      # data-prediction exponential integrators: sampling direction only
    _SCHEDULES = ("time", "logsnr")

    def sample_ode(self, num_samples: int, num_diffusion_steps: Optional[int] = None, solver: str = "heun",
                   prior_noise: Optional[Sequence[torch.Tensor]] = None, schedule: str = "time", y=None,
                   cfg_scale: float = 1.0) -> torch.Tensor:
        """Samples by the probability-flow ODE from t = 1 to t = eps in N steps: N score evaluations for Euler, 2N for Heun, N for
        "ddim" (the first-order exponential integrator in data-prediction form) and "dpmpp2m" (DPM-Solver++ 2M, its second-order
        multistep form).  schedule: "time", the grid ``linspace(1, eps, N + 1)``, or "logsnr", N + 1 points uniform in
        ``noise_scheduler.log_snr`` between t = 1 and t = eps.  Batching, launch merging and the prior as ``sample``;
        prior_noise[b] (bs,T,C) injects the prior draws of batch b.  y, cfg_scale: labels and classifier-free guidance scale as in
        ``sample`` (every solver).  Returns a CPU tensor (n, max_len, n_channels) in sample space."""
        model = self.score_model
        self._check_solver(solver, dpm=True)
        N = model.num_training_steps if num_diffusion_steps is None else int(num_diffusion_steps)
        grid = self._ode_grid(N, to_noise=False, schedule=schedule)
        guided, pair = self._guided(y, cfg_scale)
        sizes = self._batches(num_samples, _PRECISIONS[model.precision_effective], prior_noise is not None, pair=pair)
        labels = self._labels(y, sum(sizes)) if guided else None
        out: List[torch.Tensor] = []
        lo = 0
        for b, bs in enumerate(sizes):
            X = self.sample_prior(bs, noise=None if prior_noise is None else prior_noise[b])
            yb = None if labels is None else labels[lo:lo + bs].contiguous()
            lo += bs
            out.append(self._run_ode(self._cfg_state(X, pair), grid, solver, yb, float(cfg_scale), pair))
        return torch.cat([x.cpu() for x in out], dim=0)

    # ------------------------------------------------------------ classifier-free guidance (extension, not in the reference)
    def _guided(self, y, cfg_scale) -> tuple:
        """(guided, pair): whether the call runs a guided loop at all (labels or a non-default scale on a labelled model), and
        whether that loop evaluates the score twice per step (as one forward on 2 x the rows).  ValueError for labels or a scale
        on an unlabelled model, or a scale that is not a finite number."""
        if isinstance(cfg_scale, bool) or not isinstance(cfg_scale, (int, float)) or not math.isfinite(cfg_scale):
            raise ValueError(f"cfg_scale must be a finite number, got {cfg_scale!r}")
        if self.score_model.n_classes <= 0 and getattr(self.score_model, "cond_dim", 0) <= 0:
            if y is not None or float(cfg_scale) != 1.0:
                raise ValueError("y / cfg_scale need a class-conditional model (ScoreModule(n_classes=K)) or a covariate-conditional "
                                 "one (ScoreModule(cond_dim=P)); this one has n_classes = 0 and cond_dim = 0")
            return False, False
        guided = y is not None or float(cfg_scale) != 1.0
        # The engine takes the scale as a float and decides on that value (fd_guide_plan), so a scale that rounds to 0 or 1 there
        # is one evaluation here too.  (FDIFF_CFG_FORCE_PAIR, tests: the two-evaluation form also where the combine is exact; the
        # engine reads the same switch.)
        w32 = C.c_float(float(cfg_scale)).value
        pair = y is not None and (w32 not in (0.0, 1.0) or bool(os.environ.get("FDIFF_CFG_FORCE_PAIR")))
        return guided, pair

    def _labels(self, y, total: int) -> Optional[torch.Tensor]:
        """The labels of all ``total`` returned samples as an int32 device vector (None: unconditional); on a covariate model the
        covariates as a float32 device matrix (total, cond_dim), y being (total, cond_dim) or (cond_dim,) for every sample alike."""
        if getattr(self.score_model, "cond_dim", 0) > 0:
            if isinstance(y, torch.Tensor) and y.dim() == 2 and y.shape[0] != total:
                raise ValueError(f"y must hold one covariate row per returned sample: {total} (whole batches of sample_batch_size), "
                                 f"got {y.shape[0]}")
            return self.score_model.covariates_on_device(y, total, "y")
        if isinstance(y, torch.Tensor) and y.dim() == 1 and y.shape[0] != total:
            raise ValueError(f"y must hold one label per returned sample: {total} (whole batches of sample_batch_size), got {y.shape[0]}")
        return self.score_model.labels_on_device(y, total, "y")

    def _series_labels(self, y, n: int, who: str) -> Optional[torch.Tensor]:
        """The labels of ``n`` conditioning series (``impute``, ``impute_guidance``, ``log_likelihood``: one label per series) as an
        int32 device vector (None: unconditional).  Covariates are not built there: ValueError."""
        if getattr(self.score_model, "cond_dim", 0) > 0:
            raise ValueError(f"{who}: covariates (y / cfg_scale on a covariate-conditional model) are not built here; call it with "
                             "y=None to run the model on its null vector")
        if isinstance(y, torch.Tensor) and y.dim() == 1 and y.shape[0] != n:
            raise ValueError(f"{who}: y must hold one label per series: {n}, got {y.shape[0]}")
        return self.score_model.labels_on_device(y, n, "y")

    @staticmethod
    def _cfg_state(X: torch.Tensor, pair: bool) -> torch.Tensor:
        """The state buffer of a guided loop: X itself, or (2 bs, T, C) with X in its first half for the two-evaluation form."""
        if not pair:
            return X
        Xs = torch.empty((2 * X.shape[0],) + tuple(X.shape[1:]), device=X.device, dtype=X.dtype)
        Xs[:X.shape[0]].copy_(X)
        return Xs

    def encode(self, X: torch.Tensor, num_diffusion_steps: int, solver: str = "heun", schedule: str = "time") -> torch.Tensor:
        """Latents of X (n, max_len, n_channels) in sample space: the probability-flow ODE from t = eps to t = 1 by Euler or Heun
        (the data-prediction solvers sample only: ValueError).  Deterministic; ``decode`` inverts it up to the discretisation
        error.  Launches of at most ``sample_batch_size`` series; returns a CPU tensor."""
        self._check_solver(solver, dpm=False)
        return self._map_ode(X, self._ode_grid(int(num_diffusion_steps), to_noise=True, schedule=schedule), solver, "X")

    def decode(self, latents: torch.Tensor, num_diffusion_steps: int, solver: str = "heun", schedule: str = "time") -> torch.Tensor:
        """Series in sample space from latents at t = 1: the probability-flow ODE from t = 1 to t = eps (``sample_ode`` from given
        latents, any of its solvers and schedules).  Returns a CPU tensor."""
        self._check_solver(solver, dpm=True)
        return self._map_ode(latents, self._ode_grid(int(num_diffusion_steps), to_noise=False, schedule=schedule), solver, "latents")

    def _check_solver(self, solver: str, dpm: bool) -> None:
        """ValueError unless ``solver`` names an ODE solver (dpm: the data-prediction ones are allowed too)."""
        if solver in self._SOLVERS or (dpm and solver in self._DPM_SOLVERS):
            return
        if solver in self._DPM_SOLVERS:
            raise ValueError(f"solver {solver!r} integrates from noise to data only (sample_ode, decode); encode takes "
                             f"{sorted(self._SOLVERS)}")
        hint = (" (rk45 takes a tolerance, not a step count: sample_ode_adaptive, encode_adaptive, decode_adaptive; "
                "log_likelihood(solver='rk45'))") if solver == "rk45" else ""
        allowed = sorted(self._SOLVERS) + (sorted(self._DPM_SOLVERS) if dpm else [])
        raise ValueError(f"solver must be one of {allowed}, got {solver!r}{hint}")

    def _ode_grid(self, N: int, to_noise: bool, schedule: str = "time"):
        if schedule not in self._SCHEDULES:
            raise ValueError(f"schedule must be one of {list(self._SCHEDULES)}, got {schedule!r}")
        if N < 1:
            raise ValueError(f"num_diffusion_steps must be >= 1, got {N}")
        sch = self.noise_scheduler
        if sch.G is None:
            raise RuntimeError("the noise scheduler has no noise scaling yet (set_noise_scaling)")
        if schedule == "logsnr":
            ts = self.logsnr_grid(sch, N)
            if to_noise:
                ts = ts.flip(0)
        else:
            ts = torch.linspace(sch.eps, 1.0, N + 1) if to_noise else torch.linspace(1.0, sch.eps, N + 1)
        return (C.c_float * (N + 1))(*ts.to(torch.float32).tolist()), N

    @staticmethod
    def logsnr_grid(sch: SDE, N: int) -> torch.Tensor:
        """N + 1 float32 times from 1 down to ``sch.eps`` whose log-SNR (``sch.log_snr``) is uniformly spaced: computed in double,
        the end points exactly 1 and eps.  ValueError when the float32 grid is not strictly decreasing."""
        l1, l0 = sch.log_snr(1.0), sch.log_snr(sch.eps)
        ts = [1.0] + [sch.t_of_log_snr(l1 + (l0 - l1) * (i / N)) for i in range(1, N)] + [float(sch.eps)]
        out = torch.tensor(ts, dtype=torch.float64).to(torch.float32)
        if not bool((out[1:] < out[:-1]).all()):
            raise ValueError(f"the log-SNR grid of {N} steps between t = 1 and t = {sch.eps} is not strictly decreasing in float32")
        return out

    def _map_ode(self, X: torch.Tensor, grid, solver: str, name: str) -> torch.Tensor:
        self._check_series(X, name)
        dev = self.score_model.device
        out: List[torch.Tensor] = []
        for lo in range(0, X.shape[0], self.sample_batch_size):
            xb = X[lo:lo + self.sample_batch_size].to(device=dev, dtype=torch.float32).contiguous().clone()
            out.append(self._run_ode(xb, grid, solver))
        return torch.cat([x.cpu() for x in out], dim=0)

    def _run_ode(self, X: torch.Tensor, grid, solver: str, yb: Optional[torch.Tensor] = None, w: float = 1.0,
                 pair: bool = False) -> torch.Tensor:
        """X device float32, integrated in place over ``grid`` (ctypes float[N+1], N): (bs,T,C), or the (2 bs,T,C) state of a
        guided loop in its two-evaluation form (``pair``; ``_cfg_state``).  Labels yb or a scale w != 1 (``_guided``): the guided
        entry point.  Returns the bs integrated rows."""
        self._check_solver(solver, dpm=True)
        self.score_model.eval()
        ctx, h, p, G, mode = self._engine_args()
        ts_arr, N = grid
        bs = X.shape[0] // 2 if pair else X.shape[0]
        dpm = solver in self._DPM_SOLVERS
        sid = self._DPM_SOLVERS[solver] if dpm else self._SOLVERS[solver]
        if yb is not None or w != 1.0:
            run_guided = _C.lib().fd_sampler_run_ode_cov if self.score_model.cond_dim > 0 else _C.lib().fd_sampler_run_ode_cfg
            rc = run_guided(h, C.byref(p), G.data_ptr(), ts_arr, N, sid, X.data_ptr(), _C.ptr(yb), w, bs, mode,
                                                 _C.stream_of(X))
        else:
            run = _C.lib().fd_sampler_run_dpm if dpm else _C.lib().fd_sampler_run_ode
            rc = run(h, C.byref(p), G.data_ptr(), ts_arr, N, sid, X.data_ptr(), bs, mode, _C.stream_of(X))
        _C.check(rc, ctx)
        return X[:bs]

    # ------------------------------------------------------------ adaptive ODE (extension, not in the reference)
    def sample_ode_adaptive(self, num_samples: int, rtol: float = 1e-5, atol: float = 1e-5, max_evals: int = RK45_MAX_EVALS,
                            prior_noise: Optional[Sequence[torch.Tensor]] = None, y=None, cfg_scale: float = 1.0,
                            return_info: bool = False, compact_granule: int = 0):
        """Samples by the probability-flow ODE from t = 1 to t = eps with Dormand-Prince 5(4) under the step control of scipy's
        RK45 (Song et al. 2021's black-box sampler; fd_sampler_run_ode_adaptive): a tolerance instead of a step count, every row
        on its own grid, at most ``max_evals`` score evaluations per row.  Launches are the reference's batches of
        ``sample_batch_size`` rows (half of that for a guided loop in its two-evaluation form); nothing is merged, the loop
        evaluates the network step by step.  prior_noise[b], y, cfg_scale as ``sample_ode``.  compact_granule: rows by which the
        running count must fall before the launches shrink to the running rows (0: FDIFF_RK_COMPACT_GRANULE, else the engine's
        default -- 1 for the transformer in fp32, off otherwise, by measurement: DESIGN 3.37; guided calls never compact).
        Returns a CPU tensor (n, max_len, n_channels); with return_info, (samples, ODEInfo).  Without it a row that did not
        converge raises RuntimeError."""
        t0, rtol, atol, max_evals = self._adaptive_plan(rtol, atol, max_evals)
        guided, pair = self._guided(y, cfg_scale)
        bs = self.sample_batch_size
        sizes = [min(num_samples - b * bs, bs) for b in range(max(1, num_samples // bs))]
        if pair and prior_noise is None:
            half = max(1, bs // 2)
            sizes = [min(half, n - lo) for n in sizes for lo in range(0, n, half)]
        labels = self._labels(y, sum(sizes)) if guided else None
        out, infos, lo = [], [], 0
        for b, nb in enumerate(sizes):
            X = self.sample_prior(nb, noise=None if prior_noise is None else prior_noise[b])
            yb = None if labels is None else labels[lo:lo + nb].contiguous()
            lo += nb
            infos.append(self._run_ode_adaptive(X, 1.0, t0, rtol, atol, max_evals, yb, float(cfg_scale), guided, compact_granule))
            out.append(X.cpu())
        return self._adaptive_result(out, infos, rtol, atol, max_evals, return_info, "sample_ode_adaptive")

    def encode_adaptive(self, X: torch.Tensor, rtol: float = 1e-5, atol: float = 1e-5, max_evals: int = RK45_MAX_EVALS,
                        return_info: bool = False, y=None, cfg_scale: float = 1.0, compact_granule: int = 0):
        """Latents of X (n, max_len, n_channels): the probability-flow ODE from t = eps to t = 1 to the tolerance rtol / atol
        (``sample_ode_adaptive``'s integrator, run upward).  y (one label / covariate row per series) and cfg_scale encode along the
        guided field.  Returns a CPU tensor, or (latents, ODEInfo)."""
        return self._map_ode_adaptive(X, True, rtol, atol, max_evals, return_info, y, cfg_scale, compact_granule, "encode_adaptive")

    def decode_adaptive(self, latents: torch.Tensor, rtol: float = 1e-5, atol: float = 1e-5, max_evals: int = RK45_MAX_EVALS,
                        return_info: bool = False, y=None, cfg_scale: float = 1.0, compact_granule: int = 0):
        """Series from latents at t = 1: the same integration from t = 1 down to t = eps (``sample_ode_adaptive`` from given
        latents).  Returns a CPU tensor, or (series, ODEInfo)."""
        return self._map_ode_adaptive(latents, False, rtol, atol, max_evals, return_info, y, cfg_scale, compact_granule,
                                      "decode_adaptive")

    def _adaptive_plan(self, rtol, atol, max_evals) -> tuple:
        """Validates the tolerances of the adaptive calls before any engine work: (eps, rtol, atol, max_evals)."""
        def number(v):
            try:
                return None if isinstance(v, bool) else float(v)
            except (TypeError, ValueError):
                return None
        for name, v in (("rtol", rtol), ("atol", atol)):
            f = number(v)
            if f is None or not math.isfinite(f) or not f > 0:
                raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
        f = number(max_evals)
        if f is None or not math.isfinite(f) or f != int(f) or f < 8:
            raise ValueError(f"max_evals must be an integer >= 8 (the initial step and one attempt), got {max_evals!r}")
        sch = self.noise_scheduler
        if sch.G is None:
            raise RuntimeError("the noise scheduler has no noise scaling yet (set_noise_scaling)")
        eps = float(sch.eps)
        if not (math.isfinite(eps) and eps < 1.0):
            raise ValueError(f"the adaptive ODE integrates between eps and 1: need eps < 1, got {sch.eps}")
        return eps, float(rtol), float(atol), int(max_evals)

    def _map_ode_adaptive(self, X, to_noise, rtol, atol, max_evals, return_info, y, cfg_scale, compact_granule, who):
        eps, rtol, atol, max_evals = self._adaptive_plan(rtol, atol, max_evals)
        n = self._check_series(X, "X" if to_noise else "latents")
        guided, pair = self._guided(y, cfg_scale)
        labels = self._labels(y, n) if guided else None
        dev = self.score_model.device
        per = max(1, self.sample_batch_size // 2) if pair else self.sample_batch_size
        t0, t1 = (eps, 1.0) if to_noise else (1.0, eps)
        out, infos = [], []
        for lo in range(0, n, per):
            xb = X[lo:lo + per].to(device=dev, dtype=torch.float32).contiguous().clone()
            yb = None if labels is None else labels[lo:lo + per].contiguous()
            infos.append(self._run_ode_adaptive(xb, t0, t1, rtol, atol, max_evals, yb, float(cfg_scale), guided, compact_granule))
            out.append(xb.cpu())
        return self._adaptive_result(out, infos, rtol, atol, max_evals, return_info, who)

    def _run_ode_adaptive(self, X, t0, t1, rtol, atol, max_evals, yb, w, guided, compact_granule):
        """One launch: X (bs,T,C) device float32 integrated in place from t0 to t1; (nfe, status, grid, row-evaluations launched)."""
        self.score_model.eval()
        ctx, h, p, G, mode = self._engine_args()
        bs, gcap = X.shape[0], 1 + (max_evals - 2) // 6
        nfe = torch.empty(bs, device=X.device, dtype=torch.int32)
        st = torch.empty(bs, device=X.device, dtype=torch.int32)
        grid = torch.empty((bs, gcap), device=X.device, dtype=torch.float64)
        launched = C.c_longlong(0)
        head = (h, C.byref(p), G.data_ptr(), t0, t1, rtol, atol, max_evals, X.data_ptr())
        tail = (C.byref(launched), bs, mode, _C.stream_of(X))
        if guided:
            run = _C.lib().fd_sampler_run_ode_adaptive_cov if self.score_model.cond_dim > 0 else _C.lib().fd_sampler_run_ode_adaptive_cfg
            rc = run(*head, _C.ptr(yb), w, nfe.data_ptr(), st.data_ptr(), grid.data_ptr(), gcap, *tail)
        else:
            rc = _C.lib().fd_sampler_run_ode_adaptive(*head, nfe.data_ptr(), st.data_ptr(), grid.data_ptr(), gcap, int(compact_granule),
                                                      *tail)
        _C.check(rc, ctx)
        return nfe.cpu(), st.cpu(), grid.cpu(), int(launched.value)

    @staticmethod
    def _adaptive_result(out, infos, rtol, atol, max_evals, return_info, who):
        X = torch.cat(out, dim=0)
        status = torch.cat([i[1] for i in infos]).to(torch.int64)
        converged = status == 1
        if not return_info:
            bad = int((~converged).sum())
            if bad:
                raise RuntimeError(f"{who}: {bad} of {converged.numel()} rows did not converge within max_evals={max_evals} evaluations "
                                   f"at rtol={rtol}, atol={atol} (return_info=True returns their last accepted states and statuses)")
            return X
        width = max(int((~torch.isnan(i[2])).sum(dim=1).max()) for i in infos)
        grid = torch.full((X.shape[0], width), float("nan"), dtype=torch.float64)
        lo = 0
        for i in infos:
            w_i = min(width, i[2].shape[1])
            grid[lo:lo + i[2].shape[0], :w_i] = i[2][:, :w_i]
            lo += i[2].shape[0]
        nfe = torch.cat([i[0] for i in infos]).to(torch.int64)
        return X, ODEInfo(nfe=nfe, converged=converged, status=status, grid=grid, rtol=rtol, atol=atol,
                          row_evals_launched=sum(i[3] for i in infos), row_evals_needed=int(nfe.sum()))

    # ------------------------------------------------------------ likelihood (extension, not in the reference)
    _LL_SOLVERS = {"euler": 0, "heun": 1, "rk45": 2}

    def log_likelihood(self, X: torch.Tensor, num_diffusion_steps: int = 100, solver: str = "heun", *, estimator: str = "rademacher",
                       n_probes: int = 1, probes: Optional[torch.Tensor] = None, seed: Optional[int] = None, rtol: float = 1e-5,
                       atol: float = 1e-5, max_evals: int = RK45_MAX_EVALS, y=None, cfg_scale=None) -> LikelihoodResult:
        """Log-density of every series of X (n, max_len, n_channels), in sample space, under the probability-flow ODE:
        log p_1(x_1) + the divergence integral along the ODE from t = eps to t = 1 on ``linspace(eps, 1, N + 1)`` (the grid and
        solver of ``encode``).  The trace of the score Jacobian is estimated per series with ``n_probes`` Hutchinson probes
        (``rademacher`` or ``gaussian``, from the engine's Philox: one key from ``_rng.stream()``, or ``seed`` as the key), or
        exactly (``exact``: the T*C basis vectors, T*C <= EXACT_MAX_DIMS).  probes (n, n_probes, T, C) injects the probes.
        The probes of a series run as replicated rows of one launch: a launch holds max(1, sample_batch_size // replicas) series.
        solver="rk45" integrates adaptively instead (num_diffusion_steps is ignored): every row (series x probe) is one ODE on
        [x, divergence integral], run by Dormand-Prince 5(4) with the step control of scipy's RK45 at rtol / atol, at most
        max_evals score evaluations per row (Song et al. 2021 report likelihoods at rtol = atol = 1e-5).  A series any of whose
        rows stops early (max_evals, or a step under scipy's min_step) has converged False and log_prob NaN.
        y (class-conditional models only; ValueError otherwise): an int, or an integer tensor (n,) with one label per series --
        log p(x | y) then, the labels replicated over a series' probe rows and bound for the run (the binding found is back
        afterwards); both the fixed grids and rk45.  y=None evaluates the unconditional density (the null token).  There is no
        guidance here, and any ``cfg_scale`` other than None is a ValueError: the guided field w s(x, t, y) + (1 - w) s(x, t, null) is the
        probability-flow ODE of no model density for w outside {0, 1}, so its divergence integral is no log-likelihood.
        Returns a ``LikelihoodResult``; ``to_data_space`` converts ``log_prob`` to the series as the user holds them."""
        if cfg_scale is not None:
            raise ValueError("log_likelihood takes no cfg_scale: a guided vector field is not the probability-flow ODE of a model "
                             "density (pass y for log p(x | y))")
        self._guided(y, 1.0)
        adaptive = solver == "rk45"
        if adaptive:
            rtol, atol, max_evals = float(rtol), float(atol), int(max_evals)
        n, reps, N, grid, drift = self._ll_plan(X, num_diffusion_steps, solver, estimator, n_probes, probes, rtol, atol, max_evals)
        labels = self._series_labels(y, n, "log_likelihood") if y is not None else None
        ctx, h, p, G, mode = self._engine_args()
        dev = self.score_model.device
        T, Cn = self.max_len, self.n_channels
        key, off = 0, 0
        if probes is None and estimator != "exact":
            key, off = (int(seed), 0) if seed is not None else _rng.stream()
        per_launch = max(1, self.sample_batch_size // reps)
        launches = []
        for lo in range(0, n, per_launch):
            nb = min(per_launch, n - lo)
            x = X[lo:lo + nb].to(device=dev, dtype=torch.float32).repeat_interleave(reps, dim=0).contiguous()
            e, off = self._ll_probes(ctx, estimator, probes, lo, nb, reps, key, off)
            yb = None if labels is None else labels[lo:lo + nb].repeat_interleave(reps).contiguous()
            with self.score_model._labels_bound(h, ctx, yb, restore=True):
                if adaptive:
                    res = self._ll_run_adaptive(ctx, h, p, G, mode, x, e, grid, rtol, atol, max_evals)
                else:
                    res = self._ll_run(ctx, h, p, G, mode, x, e, grid, N, solver)
            x1 = x.view(nb, reps, T, Cn)[:, 0].contiguous()
            lp = torch.empty(nb, device=dev, dtype=torch.float32)
            _C.check(_C.lib().fd_prior_logp(ctx, C.byref(p), G.data_ptr(), x1.data_ptr(), lp.data_ptr(), nb, T, Cn, _C.stream_of(x1)), ctx)
            launches.append((lp.cpu(), x1.cpu()) + tuple(r.view(nb, reps, *r.shape[1:]).cpu() for r in res))
        return self._ll_result(launches, n, reps, N, drift, solver, estimator, rtol, atol)

    def _ll_plan(self, X, num_diffusion_steps, solver, estimator, n_probes, probes, rtol, atol, max_evals):
        """Validates the arguments of ``log_likelihood`` (before any device work); returns (n, replicas per series, N or None, the
        grid -- ctypes float[N + 1], or t0 for rk45 --, the drift part of the divergence integral)."""
        n = self._check_series(X, "X")
        T, Cn = self.max_len, self.n_channels
        if solver not in self._LL_SOLVERS:
            raise ValueError(f"solver must be one of {sorted(self._LL_SOLVERS)}, got {solver!r}")
        if estimator not in ESTIMATORS:
            raise ValueError(f"estimator must be one of {ESTIMATORS}, got {estimator!r}")
        adaptive = solver == "rk45"
        if adaptive:
            if not (math.isfinite(rtol) and rtol > 0 and math.isfinite(atol) and atol > 0):
                raise ValueError(f"rk45 needs finite rtol > 0 and atol > 0, got rtol={rtol}, atol={atol}")
            if max_evals < 8:
                raise ValueError(f"max_evals must be >= 8 (the initial step and one attempt), got {max_evals}")
            N = None
        else:
            N = int(num_diffusion_steps)
            if N < 1:
                raise ValueError(f"num_diffusion_steps must be >= 1, got {N}")
        if estimator == "exact":
            if T * Cn > EXACT_MAX_DIMS:
                raise ValueError(f"estimator='exact' replicates each series T*C = {T * Cn} times; it is allowed up to "
                                 f"{EXACT_MAX_DIMS} dimensions: use a Hutchinson estimator")
            if probes is not None:
                raise ValueError("probes cannot be injected with estimator='exact'")
            reps = T * Cn
        else:
            if int(n_probes) < 1:
                raise ValueError(f"n_probes must be >= 1, got {n_probes}")
            reps = int(n_probes)
            if probes is not None and (not isinstance(probes, torch.Tensor) or tuple(probes.shape) != (n, reps, T, Cn)):
                raise ValueError(f"probes must be a tensor of shape {(n, reps, T, Cn)}, got "
                                 f"{tuple(probes.shape) if isinstance(probes, torch.Tensor) else type(probes)}")
        sch = self.noise_scheduler
        if sch.G is None:
            raise RuntimeError("the noise scheduler has no noise scaling yet (set_noise_scaling)")
        kind, p0, p1 = sch.kind, *sch._params()
        if adaptive:
            t0 = float(sch.eps)
            if not (math.isfinite(t0) and t0 < 1.0):
                raise ValueError(f"rk45 integrates from eps to 1: need eps < 1, got {sch.eps}")
            # every row integrates the drift part itself (exactly: a(t) is linear); the exact estimator sums rows, so it is
            # removed from all but one (float32 parameters, as the engine reads them)
            p0f, p1f = (float(C.c_float(v).value) for v in (p0, p1))
            return n, reps, N, t0, drift_integral(kind, p0f, p1f, t0, 1.0, T * Cn)
        ts = torch.linspace(sch.eps, 1.0, N + 1).to(torch.float32)
        if not bool((ts[1:] > ts[:-1]).all()):
            raise ValueError(f"the likelihood grid linspace({sch.eps}, 1, {N + 1}) is not strictly increasing in float32")
        drift = drift_divergence(kind, float(p0), float(p1), ts.tolist(), solver, T * Cn)
        return n, reps, N, (C.c_float * (N + 1))(*ts.tolist()), drift

    def _ll_probes(self, ctx, estimator, probes, lo, nb, reps, key, off):
        """The probes (nb * reps, T, C) of one launch: the basis vectors (exact), the injected ones, or Philox draws at (key, off);
        returns them and the Philox offset after them."""
        T, Cn = self.max_len, self.n_channels
        dev = self.score_model.device
        if estimator == "exact":
            return torch.eye(T * Cn, device=dev, dtype=torch.float32).view(T * Cn, T, Cn).repeat(nb, 1, 1).contiguous(), off
        if probes is not None:
            e = probes[lo:lo + nb].to(device=dev, dtype=torch.float32).reshape(nb * reps, T, Cn).contiguous()
            return _C.dev_f32(e, "probes"), off
        e = torch.empty((nb * reps, T, Cn), device=dev, dtype=torch.float32)
        _C.check(_C.lib().fd_randn(ctx, e.data_ptr(), e.numel(), key, off, _C.stream_of(e)), ctx)
        off += (e.numel() + 3) // 4
        if estimator == "rademacher":
            e = torch.where(e >= 0, 1.0, -1.0).to(torch.float32).contiguous()
        return e, off

    def _ll_run(self, ctx, h, p, G, mode, x, e, ts_arr, N, solver):
        """fd_likelihood_run on the rows x (in place: latents on return): (score part of the divergence integral,) per row."""
        sdiv = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        rc = _C.lib().fd_likelihood_run(h, C.byref(p), G.data_ptr(), ts_arr, N, self._SOLVERS[solver], x.data_ptr(), e.data_ptr(),
                                        sdiv.data_ptr(), x.shape[0], mode, _C.stream_of(x))
        _C.check(rc, ctx)
        return (sdiv,)

    def _ll_run_adaptive(self, ctx, h, p, G, mode, x, e, t0, rtol, atol, max_evals):
        """fd_likelihood_run_adaptive on the rows x (in place): (divergence integral, nfe, status, accepted grid) per row."""
        rows, gcap = x.shape[0], 1 + (max_evals - 2) // 6
        sdiv = torch.empty(rows, device=x.device, dtype=torch.float64)
        nfe = torch.empty(rows, device=x.device, dtype=torch.int32)
        st = torch.empty(rows, device=x.device, dtype=torch.int32)
        grid = torch.empty((rows, gcap), device=x.device, dtype=torch.float64)
        rc = _C.lib().fd_likelihood_run_adaptive(h, C.byref(p), G.data_ptr(), t0, 1.0, rtol, atol, max_evals, x.data_ptr(), e.data_ptr(),
                                                 sdiv.data_ptr(), nfe.data_ptr(), st.data_ptr(), grid.data_ptr(), gcap, rows, mode,
                                                 _C.stream_of(x))
        _C.check(rc, ctx)
        return sdiv, nfe, st, grid

    @staticmethod
    def _ll_result(launches, n, reps, N, drift, solver, estimator, rtol, atol) -> LikelihoodResult:
        """LikelihoodResult from the launches' (prior log p, latents, divergence rows[, nfe, status, grid]) (CPU tensors)."""
        adaptive = solver == "rk45"
        prior, lat, score = ([launch[i] for launch in launches] for i in range(3))
        sd = torch.cat(score).to(torch.float64)
        if adaptive:
            sd = sd - drift      # the score part of every row (its drift part is the exact one to rounding)
        if estimator == "exact":
            div, se = sd.sum(dim=1), None
        else:
            div = sd.mean(dim=1)
            se = sd.std(dim=1) / math.sqrt(reps) if reps > 1 else None
        prior_lp = torch.cat(prior).to(torch.float64)
        delta = div + drift
        log_prob = prior_lp + delta
        if adaptive:
            nfe_s = torch.cat([launch[3] for launch in launches]).amax(dim=1).to(torch.int64)
            converged = (torch.cat([launch[4] for launch in launches]) == 1).all(dim=1)
            grid = torch.cat([launch[5] for launch in launches])
            width = int((~torch.isnan(grid)).sum(dim=2).max())
            grid = grid[:, :, :width].contiguous()
            log_prob = torch.where(converged, log_prob, torch.full_like(log_prob, float("nan")))
        else:
            nfe_s = torch.full((n,), N if solver == "euler" else 2 * N, dtype=torch.int64)
            converged, grid, rtol, atol = torch.ones(n, dtype=torch.bool), None, None, None
        return LikelihoodResult(log_prob=log_prob, prior_log_prob=prior_lp, delta_log_prob=delta, latents=torch.cat(lat),
                                std_err=se, estimator=estimator, n_probes=reps if estimator != "exact" else 0,
                                num_diffusion_steps=N, solver=solver, nfe=nfe_s, converged=converged, grid=grid, rtol=rtol,
                                atol=atol)

    # ------------------------------------------------------------ conditional sampling (extension, not in the reference)
    def impute(self, observed: torch.Tensor, mask: Optional[torch.Tensor], num_diffusion_steps: Optional[int] = None, *,
               fourier_transform: bool, feature_mean: Optional[torch.Tensor] = None, feature_std: Optional[torch.Tensor] = None,
               prior_noise: Optional[Sequence[torch.Tensor]] = None, step_noise: Optional[Sequence[torch.Tensor]] = None,
               obs_noise: Optional[Sequence[torch.Tensor]] = None, num_samples: Optional[int] = None,
               conditioning: str = "replace", guidance_scale: float = 1.0, guidance_jacobian: bool = True,
               resample: int = 1, jump_length: int = 1, renoise_noise: Optional[Sequence[torch.Tensor]] = None,
               aggregate: int = 1, operator=None, obs_std: Optional[float] = None, twist_scale: float = 1.0, ess_threshold: float = 0.5,
               final_resample: bool = True, resample_noise: Optional[Sequence[torch.Tensor]] = None, return_info: bool = False,
               y=None, cfg_scale: float = 1.0):
        """Samples conditioned on observations: returns a CPU tensor (n, max_len, n_channels) in SAMPLE space, as ``sample`` (map
        it back with the caller's destandardise / idft), one series per row of ``observed``.  ``num_samples`` = K >= 1: an
        ensemble of K samples per series instead, (n, K, max_len, n_channels); a launch holds max(1, sample_batch_size // K)
        series as K adjacent state rows each (the engine reads their observation in place: fd_sampler_run_impute_rep), and the
        injected noise of a launch has nb * K rows, series-major.

        observed (n, T, C): time-domain values at data scale (entries where ``mask`` is False are ignored, NaN allowed); mask: bool,
        (n, T, C) or (T, C), True = observed.  fourier_transform / feature_mean / feature_std: the datamodule's representation
        (``fourier_transform``, ``feature_mean_and_std`` when it standardises, else None).  Every reverse step of the grid of
        ``sample`` is followed by the projection onto the observations noised to the next time level; the last one is exact, so
        the observed entries of the result reproduce ``observed`` up to f32 transform rounding.  Launches of at most
        ``sample_batch_size`` series; launch b's noise: prior_noise[b] (nb,T,C), step_noise[b] / obs_noise[b] (N,nb,T,C)
        (slot N-1 of obs_noise is not read), else the engine's Philox stream, drawn in the order of ``sample``.

        conditioning="dps": gradient guidance instead of the projection (diffusion posterior sampling; fd_sampler_run_impute_dps).
        The state is never overwritten: every reverse step adds (guidance_scale / ||r||) (-grad ||r||^2), r = m . (y - A(x0_hat)) the
        residual of Tweedie's estimate x0_hat at the observations, and the observed entries of the result are NOT reproduced
        exactly.  guidance_jacobian=False drops the network's Jacobian from the gradient (d x0_hat / d x ~ I / alpha): about the
        cost of the projection, against a training forward and an input VJP per step.  guidance_scale: finite, >= 0.  obs_noise is
        an error under "dps" (no observation is noised).

        y, cfg_scale (class-conditional models only; ValueError otherwise): y an int or an integer tensor (n,), ONE label per series
        (the K rows of an ensemble share their series' label), cfg_scale = w the classifier-free guidance scale as in ``sample``:
        every reverse step follows w s(x, t, y) + (1 - w) s(x, t, null), under both conditionings (fd_sampler_run_impute_cfg,
        fd_sampler_run_impute_dps_cfg; under "dps" the gradient's Jacobian is the guided score's).  w = 1 conditions on the class
        with one evaluation per step, w = 0 ignores the labels; otherwise the two evaluations of a step run as one forward on
        twice the rows, and a launch holds max(1, sample_batch_size // (2 K)) series, so that the forward workspace stays that of
        ``sample_batch_size`` rows (the injected noise of a launch is shaped accordingly).  y=None, cfg_scale=1.0: the call
        without the two arguments, to the bit, on labelled and unlabelled models alike.

        resample = r, jump_length = j (conditioning="replace" only; RePaint, Lugmayr et al. 2022): the N steps are cut into blocks of
        j, every block is executed r times, and between two executions the state is diffused forward again from the block's last
        level to its first (``repaint_schedule``), so that the hidden part can harmonise with what the projection pasted in.
        E = r N score evaluations and K = (r - 1) ceil(N / j) re-noises, each fused into the kernel of the step before it
        (fd_sampler_run_impute_repaint).  With r > 1, step_noise[b] / obs_noise[b] are (E,nb,T,C) in execution order and
        renoise_noise[b] is (K,nb,T,C); the Philox stream is used only when all of them are absent.  r = 1 is the call without the
        arguments for every j, to the bit (renoise_noise is an error there).

        aggregate = w > 1 (1 <= w <= max_len): the observations are WINDOW MEANS, a series reported at a w times coarser rate
        (temporal super-resolution, disaggregation; forecasting from a coarse history with a mask over windows).  With
        J = ceil(T / w) windows, window j = [j w, min((j + 1) w, T)) (the last one may be shorter), ``observed`` is (n, J, C), the
        window means at data scale (``masks.window_means``), and ``mask`` is bool (n, J, C) or (J, C): True = the mean of that
        window is observed.  Under "replace" the projection becomes the one onto {x : P A(x) = y} (P the window-mean operator), and
        the window means of the result reproduce ``observed`` on the observed windows up to f32 rounding; under "dps" the residual
        is the one of the window means (fd_sampler_run_impute_agg, fd_sampler_run_impute_dps_agg).  ``feature_std`` is read in both
        domains (it varies inside a window).  Ensembles and both Jacobian modes work; y / cfg_scale and resample > 1 do not
        (ValueError), and max_len <= 1024.  aggregate=1: the call without the argument, to the bit.

        operator = P (a ``masks.LinearOperator``, or an (M, max_len) array / tensor wrapped on the fly): the observations are a
        GENERAL LINEAR summary y = P x per channel -- a band-limited recording, an overlapping moving average, a blur, increments
        (``masks.lowpass_operator`` and its siblings).  ``observed`` is (n, M, C) at data scale (``masks.apply_operator``), ``mask``
        bool (n, M, C), (M, C) or None (every row observed): True = row j of P is observed.  The formulas are those of
        ``aggregate`` with P, P^+ = pinv(P) and P^T general (fd_sampler_run_impute_op, fd_sampler_run_impute_dps_op); under
        "replace" P A(result) reproduces ``observed`` on the observed rows up to f32 rounding, and a mask may hide single rows
        only when the rows of P are mutually orthogonal (else every (series, channel) column of it is all True or all False:
        ValueError); "dps" takes any mask.  P must have full row rank and cond(P) <= the operator's max_condition (ValueError: the
        f32 bases lose about cond(P) 2^-24).  ``feature_std`` is read in both domains.  Ensembles and both Jacobian modes work;
        y / cfg_scale, resample > 1, conditioning="smc" and aggregate > 1 do not (ValueError), and max_len <= 1024.

        conditioning="smc" (num_samples = K in [2, 1024]): twisted sequential Monte Carlo, the Twisted Diffusion Sampler of Wu et
        al. 2023 (fd_sampler_run_impute_smc).  The observation model is y = A(x_0) + obs_std eps at the observed entries (obs_std
        > 0, data scale).  The K rows of a series are particles: the "dps" gradient, scaled by 1 / (2 v_i), v_i = obs_std^2 +
        twist_scale (s_i / alpha_i)^2, is the proposal; importance weights correct for what it gets wrong (exactly, with or
        without ``guidance_jacobian``); whenever the effective sample size of a series falls below ess_threshold K its particles
        are resampled on the device (systematic resampling).  final_resample=True resamples once more at the end, so the K
        returned samples are equally weighted and ``ensemble_scores`` / ``multivariate_scores`` apply unchanged; False never
        resamples at the end and returns the weighted particles (weights in ``SMCInfo.log_weights``).  resample_noise[b] (N + 1, nb): injected uniforms in [0, 1),
        one per (stage, series), else the call's Philox stream behind the predictor noise.  return_info=True: returns
        ``(samples, SMCInfo)``, the info holding the log evidence log p(y) per series (an unbiased estimate of p(y) under the
        discretised model), the final log weights, and the ESS, resample flags and ancestors of all N + 1 stages.  y / cfg_scale,
        aggregate > 1, resample > 1, obs_noise and guidance_scale do not apply (ValueError for the first four).  The other
        conditionings ignore these arguments (obs_std, resample_noise and return_info are errors there)."""
        self._check_aggregate(aggregate, "impute")
        op = self._operator(operator, aggregate, "impute")
        if op is not None:
            if y is not None or cfg_scale != 1.0:
                raise ValueError("impute: operator is not supported with y / cfg_scale (classifier-free guidance)")
            if isinstance(resample, int) and resample > 1:
                raise ValueError("impute: operator is not supported with resample > 1 (RePaint)")
            if conditioning == "smc":
                raise ValueError("impute: operator is not supported with conditioning='smc'")
            if mask is None:
                mask = torch.ones(op.M, self.n_channels, dtype=torch.bool)
        if conditioning == "smc":
            return self._impute_smc(observed, mask, num_diffusion_steps, fourier_transform, feature_mean, feature_std, prior_noise,
                                    step_noise, obs_noise, num_samples, guidance_jacobian, resample, renoise_noise, aggregate, y,
                                    cfg_scale, obs_std, twist_scale, ess_threshold, final_resample, resample_noise, return_info)
        if obs_std is not None or resample_noise is not None or return_info:
            raise ValueError("impute: obs_std, resample_noise and return_info go with conditioning='smc'")
        if aggregate > 1 and (y is not None or cfg_scale != 1.0):
            raise ValueError("impute: aggregate > 1 is not supported with y / cfg_scale (classifier-free guidance)")
        if aggregate > 1 and isinstance(resample, int) and resample > 1:
            raise ValueError("impute: aggregate > 1 is not supported with resample > 1 (RePaint)")
        guided, pair = self._guided(y, cfg_scale)
        for name, v in (("resample", resample), ("jump_length", jump_length)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"impute: {name} must be an int >= 1, got {v!r}")
        if resample > 1 and conditioning == "dps":
            raise ValueError("impute: resample > 1 is not supported with conditioning='dps' (the state is never projected)")
        if resample == 1 and renoise_noise is not None:
            raise ValueError("impute: renoise_noise is only read with resample > 1 (no state is re-noised)")
        if self.corrector_steps > 0:
            raise ValueError("impute: the predictor-corrector sampler is not supported with conditioning (corrector_steps=0)")
        if num_samples is not None and (isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1):
            raise ValueError(f"impute: num_samples must be None or an int >= 1, got {num_samples!r}")
        if conditioning not in ("replace", "dps"):
            raise ValueError(f"impute: conditioning must be 'replace', 'dps' or 'smc', got {conditioning!r}")
        if isinstance(guidance_scale, bool) or not isinstance(guidance_scale, (int, float)) or not math.isfinite(guidance_scale) \
                or guidance_scale < 0:
            raise ValueError(f"impute: guidance_scale must be a finite number >= 0, got {guidance_scale!r}")
        if not isinstance(guidance_jacobian, bool):
            raise ValueError(f"impute: guidance_jacobian must be a bool, got {guidance_jacobian!r}")
        dps = conditioning == "dps"
        if dps and obs_noise is not None:
            raise ValueError("impute: obs_noise is not used by conditioning='dps' (no observation is noised)")
        if op is not None and not dps and isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and mask.dim() >= 2:
            op.check_row_mask(mask, "impute")        # (before any device work; the shape is checked next)
        obs, mask_u8, per_series, mean, std = self._conditioning(observed, mask, feature_mean, feature_std, aggregate, op)
        self.score_model.eval()
        N, ts_arr, dt = self._sde_grid(num_diffusion_steps)
        ctx, h, p, G, mode = self._engine_args()
        # (the guidance weighs the residual by sigma in both domains, and sigma varies inside a window / along a row of P)
        fstd = std if (fourier_transform or dps or aggregate > 1 or op is not None) else None
        reps = 1 if num_samples is None else int(num_samples)
        n, bs = obs.shape[0], max(1, self.sample_batch_size // ((2 if pair else 1) * reps))
        labels = self._series_labels(y, n, "impute") if guided else None
        # executed steps and re-noises (resample = 1: N and 0, today's loop)
        sched = self.repaint_schedule(N, resample, jump_length) if resample > 1 else []
        K = sum(1 for op in sched if op[0] == "renoise")
        E = len(sched) - K if resample > 1 else N
        out: List[torch.Tensor] = []
        for b, lo in enumerate(range(0, n, bs)):
            nb = min(bs, n - lo)
            rows = nb * reps
            X = self.sample_prior(rows, noise=None if prior_noise is None else prior_noise[b])
            z = None if step_noise is None else self._noise(step_noise[b], (E, rows), "step_noise")
            zo = None if obs_noise is None else self._noise(obs_noise[b], (E, rows), "obs_noise")
            zr = None if renoise_noise is None else self._noise(renoise_noise[b], (K, rows), "renoise_noise")
            key, off = (0, 0) if (z is not None and (zo is not None or dps) and (zr is not None or K == 0)) else _rng.stream()
            m_b = mask_u8[lo:lo + nb] if per_series else mask_u8
            x0 = self._x0_obs(obs[lo:lo + nb], m_b, fourier_transform, mean, std, aggregate, self.max_len, op)
            if op is not None:
                if dps:
                    rc = _C.lib().fd_sampler_run_impute_dps_op(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(),
                                                               x0.data_ptr(), m_b.data_ptr(), int(per_series), _C.ptr(fstd),
                                                               int(bool(fourier_transform)), float(guidance_scale),
                                                               int(guidance_jacobian), _C.ptr(z), key, off, rows, reps,
                                                               op.handle(ctx), mode, _C.stream_of(X))
                else:
                    rc = _C.lib().fd_sampler_run_impute_op(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), x0.data_ptr(),
                                                           m_b.data_ptr(), int(per_series), _C.ptr(fstd),
                                                           int(bool(fourier_transform)), _C.ptr(z), _C.ptr(zo), key, off, rows, reps,
                                                           op.handle(ctx), mode, _C.stream_of(X))
            elif aggregate > 1:
                if dps:
                    rc = _C.lib().fd_sampler_run_impute_dps_agg(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(),
                                                                x0.data_ptr(), m_b.data_ptr(), int(per_series), _C.ptr(fstd),
                                                                int(bool(fourier_transform)), float(guidance_scale),
                                                                int(guidance_jacobian), _C.ptr(z), key, off, rows, reps,
                                                                int(aggregate), mode, _C.stream_of(X))
                else:
                    rc = _C.lib().fd_sampler_run_impute_agg(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), x0.data_ptr(),
                                                            m_b.data_ptr(), int(per_series), _C.ptr(fstd),
                                                            int(bool(fourier_transform)), _C.ptr(z), _C.ptr(zo), key, off, rows, reps,
                                                            int(aggregate), mode, _C.stream_of(X))
            elif resample > 1:
                yb = None if labels is None else labels[lo:lo + nb].repeat_interleave(reps).contiguous()
                X = self._cfg_state(X, pair)
                rc = _C.lib().fd_sampler_run_impute_repaint(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), x0.data_ptr(),
                                                            m_b.data_ptr(), int(per_series), _C.ptr(fstd),
                                                            int(bool(fourier_transform)), _C.ptr(z), _C.ptr(zo), key, off, rows, reps,
                                                            mode, _C.ptr(yb), float(cfg_scale) if guided else 1.0, _C.ptr(zr),
                                                            int(resample), int(jump_length), _C.stream_of(X))
                X = X[:rows]
            elif guided:
                yb = None if labels is None else labels[lo:lo + nb].repeat_interleave(reps).contiguous()
                X = self._cfg_state(X, pair)
                if dps:
                    rc = _C.lib().fd_sampler_run_impute_dps_cfg(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(),
                                                                x0.data_ptr(), m_b.data_ptr(), int(per_series), _C.ptr(fstd),
                                                                int(bool(fourier_transform)), float(guidance_scale),
                                                                int(guidance_jacobian), _C.ptr(z), key, off, rows, reps, mode,
                                                                _C.ptr(yb), float(cfg_scale), _C.stream_of(X))
                else:
                    rc = _C.lib().fd_sampler_run_impute_cfg(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), x0.data_ptr(),
                                                            m_b.data_ptr(), int(per_series), _C.ptr(fstd),
                                                            int(bool(fourier_transform)), _C.ptr(z), _C.ptr(zo), key, off, rows, reps,
                                                            mode, _C.ptr(yb), float(cfg_scale), _C.stream_of(X))
                X = X[:rows]
            elif dps:
                rc = _C.lib().fd_sampler_run_impute_dps(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), x0.data_ptr(),
                                                        m_b.data_ptr(), int(per_series), _C.ptr(fstd), int(bool(fourier_transform)),
                                                        float(guidance_scale), int(guidance_jacobian), _C.ptr(z), key, off, rows,
                                                        reps, mode, _C.stream_of(X))
            elif num_samples is None:
                rc = _C.lib().fd_sampler_run_impute(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), x0.data_ptr(),
                                                    m_b.data_ptr(), int(per_series), _C.ptr(fstd), int(bool(fourier_transform)),
                                                    _C.ptr(z), _C.ptr(zo), key, off, nb, mode, _C.stream_of(X))
            else:
                rc = _C.lib().fd_sampler_run_impute_rep(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), x0.data_ptr(),
                                                        m_b.data_ptr(), int(per_series), _C.ptr(fstd), int(bool(fourier_transform)),
                                                        _C.ptr(z), _C.ptr(zo), key, off, rows, reps, mode, _C.stream_of(X))
            _C.check(rc, ctx)
            out.append(X if num_samples is None else X.view(nb, reps, *X.shape[1:]))
        return torch.cat([x.cpu() for x in out], dim=0)

    def _impute_smc(self, observed, mask, num_diffusion_steps, fourier_transform, feature_mean, feature_std, prior_noise, step_noise,
                    obs_noise, num_samples, guidance_jacobian, resample, renoise_noise, aggregate, y, cfg_scale, obs_std, twist_scale,
                    ess_threshold, final_resample, resample_noise, return_info):
        """``impute(conditioning="smc")``: the argument checks, then one fd_sampler_run_impute_smc per launch."""
        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or not 2 <= num_samples <= 1024:
            raise ValueError(f"impute: conditioning='smc' needs num_samples (particles per series) in [2, 1024], got {num_samples!r}")
        if y is not None or cfg_scale != 1.0:
            raise ValueError("impute: y / cfg_scale are not supported with conditioning='smc'")
        if aggregate > 1:
            raise ValueError("impute: aggregate > 1 is not supported with conditioning='smc'")
        if resample != 1 or renoise_noise is not None:
            raise ValueError("impute: resample > 1 (RePaint) is not supported with conditioning='smc'")
        if obs_noise is not None:
            raise ValueError("impute: obs_noise is not used by conditioning='smc' (no observation is noised)")
        if self.corrector_steps > 0:
            raise ValueError("impute: the predictor-corrector sampler is not supported with conditioning (corrector_steps=0)")
        if not number(obs_std) or obs_std <= 0:
            raise ValueError(f"impute: conditioning='smc' needs obs_std, a finite number > 0, got {obs_std!r}")
        if not number(twist_scale) or twist_scale < 0:
            raise ValueError(f"impute: twist_scale must be a finite number >= 0, got {twist_scale!r}")
        if not number(ess_threshold) or not 0 <= ess_threshold <= 1:
            raise ValueError(f"impute: ess_threshold must lie in [0, 1], got {ess_threshold!r}")
        for name, v in (("final_resample", final_resample), ("guidance_jacobian", guidance_jacobian), ("return_info", return_info)):
            if not isinstance(v, bool):
                raise ValueError(f"impute: {name} must be a bool, got {v!r}")
        obs, mask_u8, per_series, mean, std = self._conditioning(observed, mask, feature_mean, feature_std, 1)
        self.score_model.eval()
        N, ts_arr, dt = self._sde_grid(num_diffusion_steps)
        ctx, h, p, G, mode = self._engine_args()
        K = int(num_samples)
        n, bs = obs.shape[0], max(1, self.sample_batch_size // K)
        dev = self.score_model.device
        out: List[torch.Tensor] = []
        info = {k: [] for k in ("log_evidence", "log_weights", "ess", "resampled", "ancestors")}
        for b, lo in enumerate(range(0, n, bs)):
            nb = min(bs, n - lo)
            rows = nb * K
            X = self.sample_prior(rows, noise=None if prior_noise is None else prior_noise[b])
            z = None if step_noise is None else self._noise(step_noise[b], (N, rows), "step_noise")
            u = None
            if resample_noise is not None:
                u = resample_noise[b].to(device=dev, dtype=torch.float64).contiguous()
                if tuple(u.shape) != (N + 1, nb) or not bool(((u >= 0) & (u < 1)).all()):
                    raise ValueError(f"resample_noise must have shape {(N + 1, nb)} and lie in [0, 1), got {tuple(u.shape)}")
            key, off = (0, 0) if (z is not None and u is not None) else _rng.stream()
            m_b = mask_u8[lo:lo + nb] if per_series else mask_u8
            x0 = self._x0_obs(obs[lo:lo + nb], m_b, fourier_transform, mean, std)
            lz = torch.empty(nb, dtype=torch.float64, device=dev)
            lw = torch.empty(rows, dtype=torch.float64, device=dev)
            es = torch.empty(N + 1, nb, dtype=torch.float64, device=dev)
            rs = torch.empty(N + 1, nb, dtype=torch.uint8, device=dev)
            an = torch.empty(N + 1, rows, dtype=torch.int32, device=dev)
            rc = _C.lib().fd_sampler_run_impute_smc(h, C.byref(p), G.data_ptr(), ts_arr, N, dt, X.data_ptr(), x0.data_ptr(),
                                                    m_b.data_ptr(), int(per_series), _C.ptr(std), int(bool(fourier_transform)),
                                                    int(guidance_jacobian), float(obs_std), float(twist_scale),
                                                    float(ess_threshold), int(final_resample), _C.ptr(z), _C.ptr(u), key, off, rows,
                                                    K, mode, lz.data_ptr(), lw.data_ptr(), es.data_ptr(), rs.data_ptr(),
                                                    an.data_ptr(), _C.stream_of(X))
            _C.check(rc, ctx)
            out.append(X.view(nb, K, *X.shape[1:]).cpu())
            n_obs = (m_b.reshape(nb, -1) if per_series else m_b.reshape(1, -1).expand(nb, -1)).sum(dim=1).to(torch.float64)
            info["log_evidence"].append((lz - 0.5 * n_obs * math.log(2.0 * math.pi * float(obs_std) ** 2)).cpu())
            info["log_weights"].append(lw.view(nb, K).cpu())
            info["ess"].append(es.cpu())
            info["resampled"].append(rs.bool().cpu())
            info["ancestors"].append(an.view(N + 1, nb, K).cpu())
        X = torch.cat(out, dim=0)
        if not return_info:
            return X
        le = torch.cat(info["log_evidence"])
        return X, SMCInfo(log_evidence=le, log_weights=torch.cat(info["log_weights"]), ess=torch.cat(info["ess"], dim=1),
                          resampled=torch.cat(info["resampled"], dim=1), ancestors=torch.cat(info["ancestors"], dim=1),
                          degenerate=torch.isinf(le) & (le < 0))

    @staticmethod
    def repaint_schedule(N: int, resample: int = 1, jump_length: int = 1) -> list:
        """The execution order of ``impute(resample=r, jump_length=j)`` over an N-step grid: ("step", i) for reverse step i with
        its projection at level i + 1, and ("renoise", i1, i0) for the forward transition from level i1 back to level i0 (level N
        is the clean one).  The steps are cut into blocks [i0, min(i0 + j, N)); a block runs r times, with a re-noise between two
        runs.  r N steps and (r - 1) ceil(N / j) re-noises; r = 1: the steps 0 .. N-1 alone."""
        for name, v in (("N", N), ("resample", resample), ("jump_length", jump_length)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"repaint_schedule: {name} must be an int >= 1, got {v!r}")
        ops = []
        for i0 in range(0, N, jump_length):
            i1 = min(i0 + jump_length, N)
            for rep in range(resample):
                ops += [("step", i) for i in range(i0, i1)]
                if rep + 1 < resample:
                    ops.append(("renoise", i1, i0))
        return ops

    def impute_project(self, X: torch.Tensor, x0_obs: torch.Tensor, mask: torch.Tensor, timestep: Optional[float] = None, *,
                       fourier_transform: bool, feature_std: Optional[torch.Tensor] = None,
                       noise: Optional[torch.Tensor] = None, renoise_to: Optional[float] = None,
                       renoise_noise: Optional[torch.Tensor] = None, aggregate: int = 1, operator=None) -> torch.Tensor:
        """The projection of ``impute`` alone (its step-wise twin, as ``reverse_diffusion_step`` is ``sample``'s): X (B,T,C) in
        sample space -> A^-1(m A(x_obs) + (1 - m) A(X)), x_obs = alpha x0_obs + s G z with (alpha, s) the perturbation kernel at
        ``timestep`` (None: alpha = 1, s = 0, the exact projection).  x0_obs from ``observed_to_sample_space``; noise: injected
        z (B,T,C) or None (Philox).  renoise_to = t' (>= ``timestep``): the projected state is then diffused forward from the level
        of ``timestep`` (None: the clean level) to t' in the same kernel (fd_impute_project_renoise), x <- a x + b G z_r with the
        transition kernel a = alpha(t') / alpha, b = sqrt(s(t')^2 - a^2 s^2); renoise_noise: injected z_r (B,T,C) or None (Philox,
        its own stream).  aggregate = w > 1: the projection on window means (fd_impute_project_agg), mask (B, J, C) or (J, C) over
        the J = ceil(T / w) windows, x0_obs from ``observed_to_sample_space(aggregate=w)``, feature_std read in both domains; not
        with renoise_to.  operator = P (``impute``): the projection on a dense operator (fd_impute_project_op), mask (B, M, C), (M, C)
        or None over the M rows of P under the row-mask rule of ``impute``, x0_obs from ``observed_to_sample_space(operator=P)``,
        feature_std read in both domains; not with renoise_to or aggregate > 1.  Returns a new device tensor."""
        self._check_aggregate(aggregate, "impute_project", int(X.shape[1]) if isinstance(X, torch.Tensor) and X.dim() == 3 else None)
        if aggregate > 1 and (renoise_to is not None or renoise_noise is not None):
            raise ValueError("impute_project: aggregate > 1 is not supported with renoise_to (RePaint)")
        op = self._operator(operator, aggregate, "impute_project", int(X.shape[1]) if isinstance(X, torch.Tensor) and X.dim() == 3 else None)
        if op is not None:
            if renoise_to is not None or renoise_noise is not None:
                raise ValueError("impute_project: operator is not supported with renoise_to (RePaint)")
            if mask is None:
                mask = torch.ones(op.M, int(X.shape[2]), dtype=torch.bool)
            if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and mask.dim() >= 2:
                op.check_row_mask(mask, "impute_project")        # (before any device work; the shape is checked below)
        xd = _C.dev_f32(X.to(self.score_model.device), "X")
        x0 = _C.dev_f32(x0_obs.to(xd.device), "x0_obs")
        if x0.shape != xd.shape or xd.dim() != 3:
            raise ValueError(f"impute_project: X {tuple(xd.shape)} and x0_obs {tuple(x0.shape)} must be the same (B,T,C) shape")
        B, T, Cn = xd.shape
        m_u8, per_series = self._mask_u8(mask, B, -(-T // aggregate) if op is None else op.M, Cn, xd.device)
        std = None
        if (fourier_transform or aggregate > 1 or op is not None) and feature_std is not None:
            std = _C.dev_f32(feature_std.to(xd.device), "feature_std")
            if tuple(std.shape) != (T, Cn):
                raise ValueError(f"impute_project: feature_std must have shape {(T, Cn)}, got {tuple(std.shape)}")
        sch = self.noise_scheduler
        alpha, sdev = (1.0, 0.0) if timestep is None else sch.marginal_coef(timestep)
        z = None if noise is None else self._noise(noise, (), "noise", B)
        zr = None if renoise_noise is None else self._noise(renoise_noise, (), "renoise_noise", B)
        # one Philox key per call, drawn only when a stream is needed; the re-noise counters lie behind the observation noise's
        key, off = (0, 0) if ((z is not None or sdev == 0.0) and (zr is not None or renoise_to is None)) else _rng.stream()
        out = torch.empty_like(xd)
        h = _C.ctx(xd.device)
        if renoise_to is None:
            if renoise_noise is not None:
                raise ValueError("impute_project: renoise_noise is only read with renoise_to")
        else:
            if isinstance(renoise_to, bool) or not isinstance(renoise_to, (int, float)) or not math.isfinite(renoise_to):
                raise ValueError(f"impute_project: renoise_to must be a finite number, got {renoise_to!r}")
            a_hi, s_hi = sch.marginal_coef(renoise_to)
            ra = a_hi / alpha
            rad = s_hi * s_hi - ra * ra * sdev * sdev
            if rad < -1e-12:
                raise ValueError(f"impute_project: renoise_to={renoise_to!r} lies below the level of timestep={timestep!r}")
            off_r = off + (xd.numel() + 3) // 4
            rc = _C.lib().fd_impute_project_renoise(h, xd.data_ptr(), x0.data_ptr(), m_u8.data_ptr(), int(per_series), _C.ptr(std),
                                                    int(bool(fourier_transform)), sch.G_on(xd.device).data_ptr(), float(alpha),
                                                    float(sdev), _C.ptr(z), key, off, float(ra), math.sqrt(max(rad, 0.0)),
                                                    _C.ptr(zr), off_r, out.data_ptr(), B, T, Cn, _C.stream_of(xd))
            _C.check(rc, h)
            return out
        if op is not None:
            rc = _C.lib().fd_impute_project_op(h, xd.data_ptr(), x0.data_ptr(), m_u8.data_ptr(), int(per_series), _C.ptr(std),
                                               int(bool(fourier_transform)), sch.G_on(xd.device).data_ptr(), float(alpha),
                                               float(sdev), _C.ptr(z), key, off, out.data_ptr(), B, T, Cn, op.handle(h),
                                               _C.stream_of(xd))
            _C.check(rc, h)
            return out
        if aggregate > 1:
            rc = _C.lib().fd_impute_project_agg(h, xd.data_ptr(), x0.data_ptr(), m_u8.data_ptr(), int(per_series), _C.ptr(std),
                                                int(bool(fourier_transform)), sch.G_on(xd.device).data_ptr(), float(alpha),
                                                float(sdev), _C.ptr(z), key, off, out.data_ptr(), B, T, Cn, int(aggregate),
                                                _C.stream_of(xd))
            _C.check(rc, h)
            return out
        rc = _C.lib().fd_impute_project(h, xd.data_ptr(), x0.data_ptr(), m_u8.data_ptr(), int(per_series), _C.ptr(std),
                                        int(bool(fourier_transform)), sch.G_on(xd.device).data_ptr(), float(alpha), float(sdev),
                                        _C.ptr(z), key, off, out.data_ptr(), B, T, Cn, _C.stream_of(xd))
        _C.check(rc, h)
        return out

    def impute_guidance(self, X: torch.Tensor, x0_obs: torch.Tensor, mask: torch.Tensor, timestep: float, *,
                        fourier_transform: bool, feature_std: Optional[torch.Tensor] = None, jacobian: bool = True,
                        aggregate: int = 1, operator=None, y=None, cfg_scale: float = 1.0) -> tuple:
        """One guidance evaluation of ``impute(conditioning="dps")`` alone (fd_impute_guidance): X (B,T,C) in sample space at
        ``timestep`` -> (g, rnorm2), g = -grad_X ||r||^2 (B,T,C) float32 and rnorm2 = ||r||^2 per row (B,) float64, both on the
        device.  x0_obs from ``observed_to_sample_space``; feature_std: the datamodule's std when it standardises (used in both
        domains), else None.  jacobian=False: the Jacobian-free gradient (the score from the sampler's forward).
        y, cfg_scale (class-conditional models only; ValueError otherwise): one label per row (an int, or an integer tensor (B,)) and
        the classifier-free guidance scale w -- the guidance of the guided score w s(x, t, y) + (1 - w) s(x, t, null), its Jacobian
        w J_c + (1 - w) J_u (fd_impute_guidance_cfg); g and rnorm2 for the B rows.
        aggregate = w > 1: the residual of the window means (fd_impute_guidance_agg), mask (B, J, C) or (J, C) over the
        J = ceil(T / w) windows, x0_obs from ``observed_to_sample_space(aggregate=w)``, rnorm2 the sum over windows; not with y /
        cfg_scale.  operator = P (``impute``): the residual of P's rows (fd_impute_guidance_op), any mask (B, M, C), (M, C) or None,
        x0_obs from ``observed_to_sample_space(operator=P)``, rnorm2 the sum over rows; not with y / cfg_scale or aggregate > 1."""
        self._check_aggregate(aggregate, "impute_guidance")
        if aggregate > 1 and (y is not None or cfg_scale != 1.0):
            raise ValueError("impute_guidance: aggregate > 1 is not supported with y / cfg_scale (classifier-free guidance)")
        op = self._operator(operator, aggregate, "impute_guidance")
        if op is not None:
            if y is not None or cfg_scale != 1.0:
                raise ValueError("impute_guidance: operator is not supported with y / cfg_scale (classifier-free guidance)")
            if mask is None:
                mask = torch.ones(op.M, self.n_channels, dtype=torch.bool)
        guided, _pair = self._guided(y, cfg_scale)
        T, Cn = self.max_len, self.n_channels
        if not (isinstance(X, torch.Tensor) and isinstance(x0_obs, torch.Tensor)) or x0_obs.shape != X.shape or X.dim() != 3 \
                or tuple(X.shape[1:]) != (T, Cn) or X.shape[0] == 0:
            raise ValueError(f"impute_guidance: X and x0_obs must be tensors of the same non-empty (B,{T},{Cn}) shape")
        if isinstance(timestep, bool) or not isinstance(timestep, (int, float)) or not math.isfinite(timestep) or timestep <= 0:
            raise ValueError(f"impute_guidance: timestep must be a finite number > 0, got {timestep!r}")
        if feature_std is not None and tuple(feature_std.shape) != (T, Cn):
            raise ValueError(f"impute_guidance: feature_std must have shape {(T, Cn)}, got {tuple(feature_std.shape)}")
        B = X.shape[0]
        m_u8, per_series = self._mask_u8(mask, B, -(-T // aggregate) if op is None else op.M, Cn, self.score_model.device)
        xd = _C.dev_f32(X.to(self.score_model.device), "X")
        x0 = _C.dev_f32(x0_obs.to(xd.device), "x0_obs")
        std = None if feature_std is None else _C.dev_f32(feature_std.to(xd.device), "feature_std")
        self.score_model.eval()
        ctx, h, p, G, mode = self._engine_args()
        g = torch.empty_like(xd)
        rn2 = torch.empty(B, dtype=torch.float64, device=xd.device)
        if guided:
            yb = self._series_labels(y, B, "impute_guidance")
            rc = _C.lib().fd_impute_guidance_cfg(h, C.byref(p), G.data_ptr(), float(timestep), xd.data_ptr(), x0.data_ptr(),
                                                 m_u8.data_ptr(), int(per_series), _C.ptr(std), int(bool(fourier_transform)),
                                                 int(bool(jacobian)), g.data_ptr(), rn2.data_ptr(), B, 1, mode, _C.ptr(yb),
                                                 float(cfg_scale), _C.stream_of(xd))
            _C.check(rc, ctx)
            return g, rn2
        if op is not None:
            rc = _C.lib().fd_impute_guidance_op(h, C.byref(p), G.data_ptr(), float(timestep), xd.data_ptr(), x0.data_ptr(),
                                                m_u8.data_ptr(), int(per_series), _C.ptr(std), int(bool(fourier_transform)),
                                                int(bool(jacobian)), g.data_ptr(), rn2.data_ptr(), B, 1, op.handle(ctx), mode,
                                                _C.stream_of(xd))
            _C.check(rc, ctx)
            return g, rn2
        if aggregate > 1:
            rc = _C.lib().fd_impute_guidance_agg(h, C.byref(p), G.data_ptr(), float(timestep), xd.data_ptr(), x0.data_ptr(),
                                                 m_u8.data_ptr(), int(per_series), _C.ptr(std), int(bool(fourier_transform)),
                                                 int(bool(jacobian)), g.data_ptr(), rn2.data_ptr(), B, 1, int(aggregate), mode,
                                                 _C.stream_of(xd))
            _C.check(rc, ctx)
            return g, rn2
        rc = _C.lib().fd_impute_guidance(h, C.byref(p), G.data_ptr(), float(timestep), xd.data_ptr(), x0.data_ptr(), m_u8.data_ptr(),
                                         int(per_series), _C.ptr(std), int(bool(fourier_transform)), int(bool(jacobian)),
                                         g.data_ptr(), rn2.data_ptr(), B, 1, mode, _C.stream_of(xd))
        _C.check(rc, ctx)
        return g, rn2

    def observed_to_sample_space(self, observed: torch.Tensor, mask: Optional[torch.Tensor], *, fourier_transform: bool,
                                 feature_mean: Optional[torch.Tensor] = None,
                                 feature_std: Optional[torch.Tensor] = None, aggregate: int = 1, operator=None) -> torch.Tensor:
        """x0_obs = A^-1(where(mask, observed, 0)) on the device (what ``impute`` conditions on; the input of ``impute_project``).
        aggregate = w > 1: observed and mask over the J = ceil(T / w) windows, x0_obs = A^-1(P^+ where(mask, observed, 0)) (n, T, C),
        P^+ the piecewise-constant lift.  operator = P (``impute``): observed and mask over the M rows of P (mask None: all observed),
        P^+ = pinv(P), the whole map in float64 on the host."""
        self._check_aggregate(aggregate, "observed_to_sample_space")
        op = self._operator(operator, aggregate, "observed_to_sample_space")
        if op is not None and mask is None:
            mask = torch.ones(op.M, self.n_channels, dtype=torch.bool)
        obs, mask_u8, _, mean, std = self._conditioning(observed, mask, feature_mean, feature_std, aggregate, op)
        return self._x0_obs(obs, mask_u8, fourier_transform, mean, std, aggregate, self.max_len, op)

    def _operator(self, operator, aggregate: int, who: str, T="max_len") -> Optional[LinearOperator]:
        """None, or the LinearOperator of ``operator`` (wrapped on the fly from an (M, T) array / tensor).  ValueError when it comes
        together with aggregate > 1 or its T is not this sampler's max_len (T: as in ``_check_aggregate``)."""
        if operator is None:
            return None
        if aggregate > 1:
            raise ValueError(f"{who}: aggregate > 1 is not supported together with operator (window means are "
                             "masks.window_mean_operator)")
        op = as_operator(operator)
        T = self.max_len if T == "max_len" else T
        if T is not None and op.T != T:
            raise ValueError(f"{who}: operator has T = {op.T} columns, expected {T}")
        return op

    def _check_aggregate(self, aggregate, who: str, T="max_len") -> None:
        """ValueError unless aggregate is an int in [1, T] (T: this sampler's max_len, or None to leave the upper end open)."""
        T = self.max_len if T == "max_len" else T
        if isinstance(aggregate, bool) or not isinstance(aggregate, int) or aggregate < 1 or (T is not None and aggregate > T):
            raise ValueError(f"{who}: aggregate must be an int in [1, {'T' if T is None else T}], got {aggregate!r}")

    def _conditioning(self, observed, mask, feature_mean, feature_std, aggregate: int = 1, op: Optional[LinearOperator] = None):
        """Validated device copies: observed (n,T,C) f32, mask as uint8 (n,T,C) or (T,C), per-series flag, mean, std.  aggregate = w
        > 1: observed and mask over the J = ceil(T / w) windows, (n,J,C) and (n,J,C) or (J,C); mean and std stay (T,C).  op: over
        the operator's M rows instead."""
        if not isinstance(mask, torch.Tensor):
            raise ValueError("observed and mask must be torch tensors")
        J = -(-self.max_len // aggregate) if op is None else op.M
        n = self._check_series(observed, "observed", J)
        if not observed.is_floating_point():
            raise ValueError(f"observed must be a floating-point tensor, got {observed.dtype}")
        T, Cn = self.max_len, self.n_channels
        dev = self.score_model.device
        m_u8, per_series = self._mask_u8(mask, n, J, Cn, dev)
        if (feature_mean is None) != (feature_std is None):
            raise ValueError("feature_mean and feature_std go together (both or neither)")
        mean = std = None
        if feature_std is not None:
            mean = _C.dev_f32(feature_mean.to(dev), "feature_mean")
            std = _C.dev_f32(feature_std.to(dev), "feature_std")
            if tuple(mean.shape) != (T, Cn) or tuple(std.shape) != (T, Cn):
                raise ValueError(f"feature_mean / feature_std must have shape {(T, Cn)}, got {tuple(mean.shape)} / {tuple(std.shape)}")
        return _C.dev_f32(observed.to(dev), "observed"), m_u8, per_series, mean, std

    @staticmethod
    def _mask_u8(mask: torch.Tensor, n: int, T: int, Cn: int, dev) -> tuple:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
            raise ValueError(f"mask must be a bool tensor, got {getattr(mask, 'dtype', type(mask))}")
        if tuple(mask.shape) == (n, T, Cn):
            per_series = True
        elif tuple(mask.shape) == (T, Cn):
            per_series = False
        else:
            raise ValueError(f"mask must have shape {(n, T, Cn)} or {(T, Cn)}, got {tuple(mask.shape)}")
        return mask.to(device=dev, dtype=torch.uint8).contiguous(), per_series

    def _noise(self, z: torch.Tensor, lead: tuple, name: str, nb: Optional[int] = None) -> torch.Tensor:
        zd = _C.dev_f32(z.to(self.score_model.device), name)
        want = tuple(lead) + ((nb,) if nb is not None else ()) + (self.max_len, self.n_channels)
        if tuple(zd.shape) != want:
            raise ValueError(f"{name} must have shape {want}, got {tuple(zd.shape)}")
        return zd

    @staticmethod
    def _x0_obs(obs: torch.Tensor, m_u8: torch.Tensor, fourier_transform: bool, mean, std, aggregate: int = 1,
                T: Optional[int] = None, op: Optional[LinearOperator] = None) -> torch.Tensor:
        y0 = torch.where(m_u8.bool(), obs, torch.zeros((), dtype=obs.dtype, device=obs.device))   # NaN at unobserved entries: gone
        if op is not None:     # A^-1(P^+ y0) once per call, in float64 on the host (not a hot path), then uploaded
            v = torch.einsum("tm,nmc->ntc", torch.from_numpy(op.P_pinv), y0.double().cpu())
            if fourier_transform:      # the packed ortho real DFT: Re X_0 .. Re X_{T/2}, then Im X_1 .. Im X_{ceil(T/2)-1}
                Xf = torch.fft.rfft(v, dim=1, norm="ortho")
                v = torch.cat([Xf.real, Xf.imag[:, 1:v.shape[1] - Xf.shape[1] + 1]], dim=1)
            if std is not None:
                v = (v - mean.double().cpu()) / std.double().cpu()
            return v.float().to(obs.device).contiguous()
        if aggregate > 1:      # P^+: every entry takes its window's value
            y0 = y0.repeat_interleave(aggregate, dim=1)[:, :T].contiguous()
        if fourier_transform:
            return dft_standardize(y0, mean, std) if std is not None else dft(y0)
        return ((y0 - mean) / std).contiguous() if std is not None else y0.contiguous()

    def _batches(self, num_samples: int, mode: int, injected: bool, pair: bool = False) -> List[int]:
        """Launch sizes of ``sample`` / ``sample_ode``: the reference's batches (``max(1, num_samples // sample_batch_size)`` of
        them, the last one possibly short), merged by ``_launch_sizes`` unless merge_batches is off, there is one batch, or noise is
        injected (one launch per batch then).  pair: a guided loop that evaluates 2 x the rows per step -- its launches are cut to
        half a batch, so that the forward workspace stays that of ``sample_batch_size`` rows (not with injected noise, whose
        tensors are shaped per batch)."""
        bs = self.sample_batch_size
        num_batches = max(1, num_samples // bs)
        sizes = [min(num_samples - b * bs, bs) for b in range(num_batches)]
        if self.merge_batches and num_batches > 1 and not injected:
            sizes = self._launch_sizes(sum(sizes), mode)
        if pair and not injected:
            half = max(1, bs // 2)
            sizes = [min(half, n - lo) for n in sizes for lo in range(0, n, half)]
        return sizes

    def _launch_sizes(self, total: int, mode: int) -> List[int]:
        """`total` series cut into launches the device runs full: multiples of (series per workgroup of the persistent kernel at a
        large batch) x (CUs), at most eight rounds of workgroups per launch; the step-by-step path (T > 256, other backbones) keeps
        the caller's batch size (its workspace grows with the batch)."""
        model = self.score_model
        # (the partition depends on the model and the device only, NOT on the arithmetic mode: a seed then gives the fp32 parity
        # path and the bf16 path the same launches, Philox keys and noise -- tests/test_gpu_bf16_distribution.py couples the two)
        try:
            _desc, spw = model.plan(1 << 16, "bf16")      # (a description: compiles nothing, fd_mega_rtc_get(compile = false))
        except _C.FdError:      # no bf16 kernels for this model (FD_ERR_UNSUPPORTED: other backbones, widths): the reference's launches
            spw = 0
        # (Known cost, ADVICE r5: a run that takes the step-by-step path with these merged launches -- fp32 parity mode, FDIFF_NO_MEGA --
        # needs ~1.1 MB of workspace per series, 4-6 GB at the default model.  Capping the launches for that path was tried and
        # reverted: the partition fixes the Philox key of every launch, and tests/test_gpu_bf16_distribution.py couples the fp32 and
        # bf16 paths through identical launches.  merge_batches=False / FDIFF_SAMPLER_MERGE=0 keeps the reference's batches.)
        if spw <= 0:
            n = self.sample_batch_size
            return [n] * (total // n) + ([total % n] if total % n else [])
        unit = spw * torch.cuda.get_device_properties(model.device).multi_processor_count
        cap = unit * 8
        out: List[int] = []
        left = total
        while left > 0:
            take = min(left, cap)
            if left > take and left - take < unit:      # do not leave a sliver for its own launch
                take = left
            out.append(take)
            left -= take
        return out

    def _engine_args(self):
        """(ctx, model handle, SDE parameters, G on the model's device, arithmetic mode) of one engine call."""
        model, sch = self.score_model, self.noise_scheduler
        ctx, h = model._engine()
        return ctx, h, sch._c_params(), sch.G_on(model.device), _PRECISIONS[model.precision_effective]

    def _sde_grid(self, num_diffusion_steps: Optional[int]):
        """N, the reverse-SDE grid ``linspace(1, eps, N)`` of the scheduler as ctypes float[N], and its step size."""
        sch = self.noise_scheduler
        N = self.score_model.num_training_steps if num_diffusion_steps is None else num_diffusion_steps
        sch.set_timesteps(N)
        return N, (C.c_float * N)(*sch.timesteps.to(torch.float32).tolist()), float(sch.step_size)

    def _check_series(self, X, name: str, rows: Optional[int] = None) -> int:
        """Raises ValueError unless X is a non-empty tensor (n, max_len, n_channels); returns n.  rows: in the place of max_len."""
        T, Cn = self.max_len if rows is None else rows, self.n_channels
        if not isinstance(X, torch.Tensor) or X.dim() != 3 or tuple(X.shape[1:]) != (T, Cn):
            raise ValueError(f"{name} must be a tensor of shape (n, {T}, {Cn}), got "
                             f"{tuple(X.shape) if isinstance(X, torch.Tensor) else type(X)}")
        if X.shape[0] == 0:
            raise ValueError(f"{name} is an empty batch")
        return int(X.shape[0])

    def sample_prior(self, batch_size: int, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        if isinstance(self.noise_scheduler, SDE):
            return self.noise_scheduler.prior_sampling((batch_size, self.max_len, self.n_channels), noise=noise,
                                                       device=self.score_model.device)
        raise NotImplementedError("Scheduler not recognized.")


def parse_labels(spec, n: int, n_classes: int, allow_balanced: bool = True) -> Optional[torch.Tensor]:
    """The ``labels`` setting of the sampler configs as the ``y`` of ``sample`` for n samples: None / "null" -> None (unconditional),
    an int (or its string) -> that class for every sample, "balanced" (unless ``allow_balanced`` is False) -> 0, 1, ...,
    n_classes - 1 cycled.  ValueError otherwise, for a class outside [0, n_classes), or for any labels on an unlabelled model."""
    if spec is None or (isinstance(spec, str) and spec.strip().lower() in ("null", "none", "")):
        return None
    if n_classes <= 0:
        raise ValueError(f"labels={spec!r}, but the model is not class-conditional (score_model.n_classes = 0)")
    if allow_balanced and isinstance(spec, str) and spec.strip().lower() == "balanced":
        return torch.arange(n, dtype=torch.int64) % n_classes
    allowed = "an int, 'balanced' or null" if allow_balanced else "'data', an int or null"
    if isinstance(spec, bool):
        raise ValueError(f"labels must be {allowed}, got {spec!r}")
    try:
        k = int(spec) if not isinstance(spec, float) or spec.is_integer() else None
    except (TypeError, ValueError):
        k = None
    if k is None:
        raise ValueError(f"labels must be {allowed}, got {spec!r}")
    if not 0 <= k < n_classes:
        raise ValueError(f"labels={k} is not a class of this model (0 .. {n_classes - 1})")
    return torch.full((n,), k, dtype=torch.int64)


def parse_covariates(spec, n: int, cond_dim: int, datamodule=None) -> Optional[torch.Tensor]:
    """The ``covariates`` setting of the sampler configs as the ``y`` of ``sample`` for n samples on a covariate-conditional model, a
    float32 tensor (n, cond_dim) in the model's (standardised) units: None / "null" -> None (the null vector); a list of cond_dim
    numbers in DATA units -> that row for every sample, standardised with the datamodule's ``cov_mean`` / ``cov_std`` when it has
    them; "data" -> the datamodule's (already standardised) ``y_test`` rows, cycled.  ValueError otherwise, and for any covariates on
    a model without them."""
    if spec is None or (isinstance(spec, str) and spec.strip().lower() in ("null", "none", "")):
        return None
    if cond_dim <= 0:
        raise ValueError(f"covariates={spec!r}, but the model has no covariates (score_model.cond_dim = 0)")
    if isinstance(spec, str) and spec.strip().lower() == "data":
        y = getattr(datamodule, "y_test", None)
        name = type(datamodule).__name__
        if y is None or not torch.as_tensor(y).is_floating_point():
            raise ValueError(f"covariates=data, but {name} has no float covariates (y_test): use datamodule=synthetic_covariates, "
                             "covariates=[v1, ..., vP] or covariates=null")
        y = torch.as_tensor(y).to(torch.float32)
        if y.dim() != 2 or y.shape[1] != cond_dim or y.shape[0] == 0:
            raise ValueError(f"covariates=data: the covariates of {name} have shape {tuple(y.shape)}, the model has cond_dim = {cond_dim}")
        return y[torch.arange(n) % y.shape[0]].contiguous()
    if isinstance(spec, str) or isinstance(spec, bool) or not hasattr(spec, "__len__"):
        raise ValueError(f"covariates must be 'data', a list of {cond_dim} numbers or null, got {spec!r}")
    vals = list(spec)
    if len(vals) != cond_dim or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in vals):
        raise ValueError(f"covariates must be 'data', a list of {cond_dim} numbers or null, got {spec!r}")
    row = torch.tensor([float(v) for v in vals], dtype=torch.float64)
    if not bool(torch.isfinite(row).all()):
        raise ValueError(f"covariates must be finite, got {spec!r}")
    mean, std = getattr(datamodule, "cov_mean", None), getattr(datamodule, "cov_std", None)
    if mean is not None and std is not None:
        row = (row - torch.as_tensor(mean, dtype=torch.float64)) / torch.as_tensor(std, dtype=torch.float64)
    return row.to(torch.float32).unsqueeze(0).expand(n, cond_dim).contiguous()


def series_labels(spec, datamodule, n: int, n_classes: int) -> Optional[torch.Tensor]:
    """The ``labels`` setting of cmd/impute.py and cmd/likelihood.py as the ``y`` of ``impute`` / ``log_likelihood`` for the first n
    test series: None / "null" -> None (the model runs unconditionally), an int (or its string) -> that class for every series,
    "data" -> ``datamodule.y_test[:n]``.  ValueError for any labels on an unlabelled model, a datamodule without labels, a label
    outside [0, n_classes), or anything else."""
    if not (isinstance(spec, str) and spec.strip().lower() == "data"):
        return parse_labels(spec, n, n_classes, allow_balanced=False)
    if n_classes <= 0:
        raise ValueError("labels=data, but the model is not class-conditional (score_model.n_classes = 0)")
    y = getattr(datamodule, "y_test", None)
    name = type(datamodule).__name__
    if y is None:
        raise ValueError(f"labels=data, but {name} has no labels (y_test is None): use a labelled datamodule "
                         "(datamodule=synthetic_classes, datamodule=ecg), labels=<int> or labels=null")
    y = torch.as_tensor(y)[:n].to(torch.int64)
    if y.shape[0] != n:
        raise ValueError(f"labels=data: {name} holds {y.shape[0]} test labels for {n} series")
    lo, hi = int(y.min()), int(y.max())
    if lo < 0 or hi >= n_classes:
        raise ValueError(f"labels=data: the test labels of {name} lie in [{lo}, {hi}], but the model has n_classes = {n_classes}")
    return y


class ODESampler(DiffusionSampler):
    """A DiffusionSampler whose ``sample`` integrates the probability-flow ODE (``sample_ode``) with the constructor's ``solver``
    ("heun", "euler", "ddim" or "dpmpp2m") and ``schedule`` ("time" or "logsnr"):
    ``python cmd/sample.py sampler=ode num_diffusion_steps=50``, ``python cmd/sample.py sampler=dpm num_diffusion_steps=20``."""

    def __init__(self, score_model: ScoreModule, sample_batch_size: int, solver: str = "heun", merge_batches: bool = True,
                 schedule: str = "time", cfg_scale: float = 1.0, labels=None, covariates=None) -> None:
        super().__init__(score_model=score_model, sample_batch_size=sample_batch_size, merge_batches=merge_batches,
                         cfg_scale=cfg_scale, labels=labels, covariates=covariates)
        self._check_solver(solver, dpm=True)
        if schedule not in self._SCHEDULES:
            raise ValueError(f"schedule must be one of {list(self._SCHEDULES)}, got {schedule!r}")
        self.solver = solver
        self.schedule = schedule

    def sample(self, num_samples: int, num_diffusion_steps: Optional[int] = None,
               prior_noise: Optional[Sequence[torch.Tensor]] = None, y=None, cfg_scale: float = 1.0) -> torch.Tensor:
        return self.sample_ode(num_samples, num_diffusion_steps, solver=self.solver, prior_noise=prior_noise, schedule=self.schedule,
                               y=y, cfg_scale=cfg_scale)


class AdaptiveODESampler(DiffusionSampler):
    """A DiffusionSampler whose ``sample`` integrates the probability-flow ODE to a tolerance (``sample_ode_adaptive``: Dormand-Prince
    5(4) under scipy's RK45 step control) instead of over a step count: ``python cmd/sample.py sampler=ode_adaptive
    sampler.rtol=1e-3 sampler.atol=1e-3``.  ``num_diffusion_steps`` is ignored.  ``last_info`` holds the ODEInfo of the last call (a
    row that did not converge is reported there -- cmd/sample.py writes ``n_not_converged`` -- rather than raised)."""

    def __init__(self, score_model: ScoreModule, sample_batch_size: int, rtol: float = 1e-5, atol: float = 1e-5,
                 max_evals: int = RK45_MAX_EVALS, cfg_scale: float = 1.0, labels=None, covariates=None) -> None:
        super().__init__(score_model=score_model, sample_batch_size=sample_batch_size, merge_batches=False, cfg_scale=cfg_scale,
                         labels=labels, covariates=covariates)
        _, self.rtol, self.atol, self.max_evals = self._adaptive_plan(rtol, atol, max_evals)
        self.last_info: Optional[ODEInfo] = None

    def sample(self, num_samples: int, num_diffusion_steps: Optional[int] = None,
               prior_noise: Optional[Sequence[torch.Tensor]] = None, y=None, cfg_scale: float = 1.0) -> torch.Tensor:
        X, self.last_info = self.sample_ode_adaptive(num_samples, rtol=self.rtol, atol=self.atol, max_evals=self.max_evals,
                                                     prior_noise=prior_noise, y=y, cfg_scale=cfg_scale, return_info=True)
        return X
