// fd_sampler.hip -- the reverse-diffusion loop of DiffusionSampler.sample
// (src/fdiff/sampling/sampler.py:83-104): n_steps x { score = model(x, t_i); x = sde.step(score, t_i, x) }.
// The reference syncs the device every step (`timesteps[0].item()`, sampler.py:37) and draws the prior on
// the CPU (sde.py:85); here the whole loop is enqueued on one stream with per-step coefficients computed on
// the host up front, and the noise comes from the on-device Philox stream unless injected.
//
// Every step-by-step loop of the engine runs through ONE driver, fd_step_loop (fd_loop.h): it lays the arena out (forward scratch,
// score, the loop's own buffers, t vectors), and evaluates the score at evaluation k.  Here: the driver, and the loops it serves but
// for the imputation one (fd_impute.hip) -- the reverse SDE (plain or guided: fd_sampler_sde_loop), the ODE solvers (plain or guided:
// fd_sampler_ode_loop) and the predictor-corrector sampler.
#include "fd_loop.h"
#include "fd_ode.h"
#include "fd_philox.h"
#include "fd_sde.h"

namespace {
__global__ __launch_bounds__(256) void k_fill(float* __restrict__ p, int n, float v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}
// t vectors of ALL steps in one launch: p[i*B + b] = ts[i]  (one k_fill launch per diffusion step was 4.5 us of a 1.5 ms step
// at T = 1024, and one more launch boundary between the SDE step and the next time embedding)
__global__ __launch_bounds__(256) void k_fill_steps(float* __restrict__ p, const float* __restrict__ ts, int B, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) p[i] = ts[i / B];
}
constexpr size_t kMaxStepTable = (size_t)16 << 20;     // floats: beyond this (n_steps * B) the t vector is refilled every step

// The fused loop forms (fd_score_bf16.hip) of the bf16 transformer, in order: the persistent kernel, then the layer form.
// FD_ERR_UNSUPPORTED when neither serves the model (or FDIFF_SAMPLER_STEPWISE asks for per-step launches; tests compare the two):
// the caller then runs step by step.
template <class Mega, class Layers>
int run_fused(const fd_score* m, int mode, Mega mega, Layers layers) {
    if (mode != FD_MODE_BF16 || m->backbone != FD_BACKBONE_TRANSFORMER || getenv("FDIFF_SAMPLER_STEPWISE")) return FD_ERR_UNSUPPORTED;
    const int rc = mega();
    return rc != FD_ERR_UNSUPPORTED ? rc : layers();
}
}  // namespace

int fd_loop_check(fd_score* m, const fd_sde_params* sde, int B, int mode, const char* who) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, sde, "%s: null pointer", who);
    FD_REQUIRE(ctx, sde->kind == 0 || sde->kind == 1, "%s: unknown SDE kind %d", who, sde->kind);
    FD_REQUIRE(ctx, B > 0, "%s: B=%d", who, B);
    FD_REQUIRE(ctx, mode == FD_MODE_F32 || mode == FD_MODE_BF16, "%s: unknown mode %d", who, mode);
    if (!m->prepared) return fd_fail(ctx, FD_ERR_STATE, "%s: call fd_score_prepare first", who);
    return FD_OK;
}

size_t fd_loop_fwd_workspace(const fd_score* m, int B) {
    return (m->backbone != FD_BACKBONE_TRANSFORMER) ? fd_bb_workspace(m, B, false) : fd_score_f32_workspace(m, B, false);
}

int fd_step_table(fd_ctx* ctx, size_t fwd, size_t own, const float* timesteps, int n_steps, int B, hipStream_t s, float** tvec,
                  size_t* stride) {
    const size_t nt = (size_t)n_steps * B;
    const bool table = nt <= kMaxStepTable && !getenv("FDIFF_SAMPLER_FILL_PER_STEP");
    const size_t extra = table ? fd_ws::padded(nt * sizeof(float)) + fd_ws::padded((size_t)n_steps * sizeof(float))
                               : fd_ws::padded((size_t)B * sizeof(float));
    if (int rc = fd_ws_reserve(ctx, fwd + own + extra)) return rc;
    *tvec = (float*)((char*)ctx->ws + fwd + own);
    *stride = table ? (size_t)B : 0;
    if (table) {
        float* ts = (float*)((char*)*tvec + fd_ws::padded(nt * sizeof(float)));
        // pageable source: the runtime stages the copy before returning
        FD_HIP(ctx, hipMemcpyAsync(ts, timesteps, (size_t)n_steps * sizeof(float), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fill_steps, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, *tvec, ts, B, nt);
    }
    return FD_OK;
}

void fd_fill(float* p, int n, float v, hipStream_t s) {
    hipLaunchKernelGGL(k_fill, dim3((n + 255) / 256), dim3(256), 0, s, p, n, v);
}

int fd_step_loop_open(fd_step_loop* lp, fd_score* m, int rows, int mode, size_t own_bytes, const float* t_eval, int n_eval,
                      hipStream_t s) {
    const size_t fwd = fd_loop_fwd_workspace(m, rows);
    const size_t sbytes = fd_ws::padded((size_t)rows * m->d.max_len * m->d.n_channels * sizeof(float));
    *lp = fd_step_loop{m, s, rows, mode, nullptr, nullptr, nullptr, 0, t_eval};
    if (int rc = fd_step_table(m->ctx, fwd, sbytes + own_bytes, t_eval, n_eval, rows, s, &lp->tvec0, &lp->tstride)) return rc;
    lp->score = (float*)((char*)m->ctx->ws + fwd);
    lp->own = (char*)lp->score + sbytes;
    return FD_OK;
}

int fd_step_loop_eval(fd_step_loop* lp, int k, const float* x) {
    float* tvec = lp->tvec0 + (size_t)k * lp->tstride;
    if (!lp->tstride) fd_fill(tvec, lp->rows, lp->t_eval[k], lp->s);
    return fd_score_forward_any(lp->m, x, tvec, lp->score, lp->rows, lp->mode, lp->s);
}

int fd_sampler_run_mega(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                        float dt, float* x, const float* z_steps, uint64_t seed, uint64_t offset, int B,
                        hipStream_t s);
int fd_sampler_run_layers(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                          float* x, const float* z_steps, uint64_t seed, uint64_t offset, int B, hipStream_t s);

// Reverse-SDE loop in place on x: the fused forms first (plain loop only), else step by step -- one score launch and one step launch
// per step, the guided pair's labels (2B) behind the score.  Philox counters: the noise of step i at offset + i * per_step.
int fd_sampler_sde_loop(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt, float* x,
                        const float* z_steps, uint64_t seed, uint64_t offset, int B, int mode, hipStream_t s, const fd_guide* g) {
    fd_ctx* ctx = m->ctx;
    if (!g) {
        const int rc_fused = run_fused(
            m, mode, [&] { return fd_sampler_run_mega(m, sde, G, timesteps, n_steps, dt, x, z_steps, seed, offset, B, s); },
            [&] { return fd_sampler_run_layers(m, sde, G, timesteps, n_steps, dt, x, z_steps, seed, offset, B, s); });
        if (rc_fused != FD_ERR_UNSUPPORTED) return rc_fused;
    }
    const int T = m->d.max_len, C = m->d.n_channels;
    const size_t n = (size_t)B * T * C;
    const int R = fd_guide_rows(g, B);
    fd_step_loop lp;
    if (int rc = fd_step_loop_open(&lp, m, R, mode, fd_guide_bytes(g, B), timesteps, n_steps, s)) return rc;
    int* lab = (int*)lp.own;
    if (int rc = fd_guide_begin(m, g, lab, x, B, s)) return rc;
    fd_guide_scope scope(m, g, lab, R);
    const uint64_t per_step = (uint64_t)((n + 3) / 4);
    for (int i = 0; i < n_steps; ++i) {
        if (int rc = fd_step_loop_eval(&lp, i, x)) return rc;
        const float* z = z_steps ? z_steps + (size_t)i * n : nullptr;
        const uint64_t ctr = offset + (uint64_t)i * per_step;
        const int rc = g && g->pair ? fd_cfg_sde_step(ctx, sde, G, x, lp.score, z, seed, ctr, (double)timesteps[i], dt, *g, B, T, C, s)
                                    : fd_sde_step(ctx, sde, G, x, lp.score, z, seed, ctr, (double)timesteps[i], dt, x, B, T, C, s);
        if (rc) return rc;
    }
    return FD_OK;
}

extern "C" int fd_sampler_run(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                              int n_steps, float dt, float* x, const float* z_steps, uint64_t seed, uint64_t offset,
                              int B, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run")) return rc;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x, "fd_sampler_run: null pointer");
    FD_REQUIRE(ctx, n_steps > 0, "fd_sampler_run: n_steps=%d", n_steps);
    FD_REQUIRE(ctx, dt > 0.f, "fd_sampler_run: step size must be > 0 (sde.py:158)");
    return fd_sampler_sde_loop(m, sde, G, timesteps, n_steps, dt, x, z_steps, seed, offset, B, mode, (hipStream_t)stream, nullptr);
}

// Probability-flow ODE loop (fd_ode.hip; not in the reference) over the rows of one solver (fd_solver_rows), in place on x, in the
// dispatch order of fd_sampler_sde_loop.  Step by step: one score launch and one stage launch per evaluation; behind the score the
// solver's state (nstate (B,T,C) buffers: Heun 2, DPM-Solver++ 2M 1), then the guided pair's labels.
int fd_sampler_ode_loop(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, int solver,
                        float* x, int B, int mode, hipStream_t s, const fd_guide* g) {
    fd_ctx* ctx = m->ctx;
    std::vector<fd_ode_step_coef> rows;
    std::vector<fd_dpm_coef> dpm_rows;      // the data-prediction solvers' second coefficient pairs, else empty
    int nstate = 0;
    if (int rc = fd_solver_rows(ctx, sde, timesteps, n_steps, solver, &rows, &dpm_rows, &nstate)) return rc;
    const std::vector<fd_dpm_coef>* dpm = dpm_rows.empty() ? nullptr : &dpm_rows;
    if (!g) {
        const int rc_fused = run_fused(m, mode, [&] { return fd_sampler_run_ode_mega(m, rows, G, x, B, s, dpm); },
                                       [&] { return fd_sampler_run_ode_layers(m, rows, G, x, B, s, dpm); });
        if (rc_fused != FD_ERR_UNSUPPORTED) return rc_fused;
    }
    const int T = m->d.max_len, C = m->d.n_channels;
    const int n_eval = (int)rows.size(), R = fd_guide_rows(g, B);
    const size_t buf = fd_ws::padded((size_t)B * T * C * sizeof(float));
    std::vector<float> t_eval(n_eval);
    for (int k = 0; k < n_eval; ++k) t_eval[k] = rows[k].t;
    fd_step_loop lp;
    if (int rc = fd_step_loop_open(&lp, m, R, mode, nstate * buf + fd_guide_bytes(g, B), t_eval.data(), n_eval, s)) return rc;
    float* x0 = nstate > 0 ? (float*)lp.own : nullptr;
    float* v0 = nstate > 1 ? (float*)(lp.own + buf) : nullptr;
    int* lab = (int*)(lp.own + nstate * buf);
    if (int rc = fd_guide_begin(m, g, lab, x, B, s)) return rc;
    fd_guide_scope scope(m, g, lab, R);
    for (int k = 0; k < n_eval; ++k) {
        if (int rc = fd_step_loop_eval(&lp, k, x)) return rc;
        if (int rc = fd_ode_stage(ctx, G, x, lp.score, x0, v0, rows[k], B, T, C, s, dpm ? &(*dpm)[k] : nullptr, g)) return rc;
    }
    return FD_OK;
}

// Euler (n_steps evaluations) or Heun (2 n_steps) over the grid timesteps[0 .. n_steps]
extern "C" int fd_sampler_run_ode(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                  int solver, float* x, int B, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_ode")) return rc;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x, "fd_sampler_run_ode: null pointer");
    FD_REQUIRE(ctx, n_steps > 0, "fd_sampler_run_ode: n_steps=%d", n_steps);
    FD_REQUIRE(ctx, solver == 0 || solver == 1, "fd_sampler_run_ode: solver %d (0 Euler, 1 Heun)", solver);
    return fd_sampler_ode_loop(m, sde, G, timesteps, n_steps, solver, x, B, mode, (hipStream_t)stream, nullptr);
}

// The data-prediction solvers over a sampling grid (t decreasing): solver 2 = deterministic DDIM, 3 = DPM-Solver++ 2M; n_steps
// evaluations either way
extern "C" int fd_sampler_run_dpm(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                  int solver, float* x, int B, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_dpm")) return rc;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x, "fd_sampler_run_dpm: null pointer");
    FD_REQUIRE(ctx, n_steps > 0, "fd_sampler_run_dpm: n_steps=%d", n_steps);
    FD_REQUIRE(ctx, solver == 2 || solver == 3, "fd_sampler_run_dpm: solver %d (2 DDIM, 3 DPM-Solver++ 2M)", solver);
    return fd_sampler_ode_loop(m, sde, G, timesteps, n_steps, solver, x, B, mode, (hipStream_t)stream, nullptr);
}

// Predictor-corrector variant (not in the reference; BASELINE.json configs[3] says "PC sampler"): n_corr Langevin corrector
// steps (fd_langevin_step, signal-to-noise ratio snr) before every predictor step.  zc_steps (nullable): injected corrector
// noise (n_steps, n_corr, B, T, C).  Step-by-step launches (the persistent kernel is predictor-only).
extern "C" int fd_sampler_run_pc(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                 float dt, float* x, const float* z_steps, const float* zc_steps, int n_corr, float snr,
                                 uint64_t seed, uint64_t offset, int B, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_pc")) return rc;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x, "fd_sampler_run_pc: null pointer");
    FD_REQUIRE(ctx, n_steps > 0 && n_corr >= 0, "fd_sampler_run_pc: n_steps=%d n_corr=%d", n_steps, n_corr);
    FD_REQUIRE(ctx, dt > 0.f && (n_corr == 0 || snr > 0.f), "fd_sampler_run_pc: dt=%f snr=%f", dt, snr);
    const int T = m->d.max_len, C = m->d.n_channels;
    const size_t n = (size_t)B * T * C;
    fd_step_loop lp;
    if (int rc = fd_step_loop_open(&lp, m, B, mode, 0, timesteps, n_steps, (hipStream_t)stream)) return rc;
    const uint64_t per_step = (uint64_t)((n + 3) / 4);
    // Philox counters: predictor noise of step i at offset + i*per_step (as fd_sampler_run); corrector noise behind them
    const uint64_t corr_base = offset + (uint64_t)n_steps * per_step;
    for (int i = 0; i < n_steps; ++i) {
        for (int k = 0; k < n_corr; ++k) {
            if (int rc = fd_step_loop_eval(&lp, i, x)) return rc;
            // alpha_t of Song et al.: 1 - beta(t) dt for the VP-SDE, 1 for the VE-SDE
            float alpha = 1.0f;
            if (sde->kind == 0) alpha = 1.0f - (sde->p0 + timesteps[i] * (sde->p1 - sde->p0)) * dt;
            if (alpha <= 0.f) alpha = 1e-6f;
            const float* zc = zc_steps ? zc_steps + ((size_t)i * n_corr + k) * n : nullptr;
            if (int rc = fd_langevin_step(ctx, G, x, lp.score, zc, seed, corr_base + ((uint64_t)i * n_corr + k) * per_step, snr, alpha,
                                          x, B, T, C, stream))
                return rc;
        }
        if (int rc = fd_step_loop_eval(&lp, i, x)) return rc;
        const float* z = z_steps ? z_steps + (size_t)i * n : nullptr;
        if (int rc = fd_sde_step(ctx, sde, G, x, lp.score, z, seed, offset + (uint64_t)i * per_step, (double)timesteps[i], dt, x, B, T,
                                 C, stream))
            return rc;
    }
    return FD_OK;
}
