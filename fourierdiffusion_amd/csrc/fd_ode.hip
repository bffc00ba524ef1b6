// fd_ode.hip -- probability-flow ODE of the score SDE (Song et al. 2021, Sec. 4.3; not in the reference, whose only sampler is
// Euler-Maruyama over the reverse SDE, src/fdiff/sampling/sampler.py:83-104):
//   dx/dt = v(x, t) = -a x - 0.5 (g G_k)^2 s(x, t)      (VP a = beta/2, g = sqrt(beta); VE a = 0, g of fd_sde_coef)
// integrated by Euler or Heun on a strictly monotone grid in either direction (t 1 -> eps samples / decodes, eps -> 1 encodes).
// Here: the velocity alone (fd_pf_ode_drift), the coefficient table every loop form runs from, and the elementwise stage of the
// step-by-step loop (fp32 parity mode, the MLP / LSTM backbones, FDIFF_SAMPLER_STEPWISE).  No random numbers are drawn.
//
// The data-prediction solvers (DDIM, DPM-Solver++ 2M; fd_mega_params.h) run on the same rows and through the same loop forms: their
// table (fd_dpm_table) and their step-wise entry point (fd_dpm_stage) are here as well.  ONE stage kernel (k_stage) serves both
// families, plain and under classifier-free guidance (fd_guide, fd_loop.h).
#include <cmath>

#include "fd_loop.h"
#include "fd_ode.h"
#include "fd_sde.h"

namespace {

constexpr int kBlock = 256;

// v = -a x - 0.5 (g G_k)^2 s, one element per thread and iteration
__global__ __launch_bounds__(kBlock) void k_ode_drift(const float* __restrict__ G, const float* __restrict__ x,
                                                        const float* __restrict__ score, float* __restrict__ v, size_t n, int T,
                                                        int C, float a_x, float g) {
    for (size_t e = blockIdx.x * (size_t)kBlock + threadIdx.x; e < n; e += (size_t)gridDim.x * kBlock) {
        const int t = (int)((e / (size_t)C) % (size_t)T);
        v[e] = fd_ode_velocity(x[e], score[e], a_x, g * G[t]);
    }
}

// One stage on (B,T,C), n = B T C elements.  V4 (C % 4 == 0): a thread owns four elements of one row, as the persistent kernel's
// epilogue lanes do.  DPM: a data-prediction stage (dw its second coefficient pair, x0 = D_prev, updated in place; v0 unused), else
// Euler / Heun with the Heun state x0 / v0.  PAIR (classifier-free guidance): x and score hold 2n elements, the score is
// fd_guided(score[e], score[n + e]) and the new state goes to both halves.
template <bool V4, bool DPM, bool PAIR>
__global__ __launch_bounds__(kBlock) void k_stage(const float* __restrict__ G, float* __restrict__ x, const float* __restrict__ score,
                                                    float* __restrict__ x0, float* __restrict__ v0, size_t n, int T, int C,
                                                    fd_ode_step_coef c, fd_dpm_coef dw, float w, float omw) {
    const size_t items = V4 ? n / 4 : n;
    for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < items; i += (size_t)gridDim.x * kBlock) {
        if (V4) {
            const size_t e = 4 * i;
            const float gk = c.g * G[(e / (size_t)C) % (size_t)T];
            const float4 xv = *reinterpret_cast<const float4*>(x + e);
            float4 sv = *reinterpret_cast<const float4*>(score + e);
            if (PAIR) {
                const float4 su = *reinterpret_cast<const float4*>(score + n + e);
                sv.x = fd_guided(sv.x, su.x, w, omw);
                sv.y = fd_guided(sv.y, su.y, w, omw);
                sv.z = fd_guided(sv.z, su.z, w, omw);
                sv.w = fd_guided(sv.w, su.w, w, omw);
            }
            const float4 o = DPM ? fd_dpm_stage4(xv, sv.x, sv.y, sv.z, sv.w, gk, c, dw, x0 + e)
                                 : fd_ode_stage4(xv, sv.x, sv.y, sv.z, sv.w, gk, c, x0 + e, v0 + e);
            *reinterpret_cast<float4*>(x + e) = o;
            if (PAIR) *reinterpret_cast<float4*>(x + n + e) = o;
        } else {
            const float gk = c.g * G[(i / (size_t)C) % (size_t)T];
            const float sv = PAIR ? fd_guided(score[i], score[n + i], w, omw) : score[i];
            const float o = DPM ? fd_dpm_stage1(x[i], sv, gk, c, dw, x0 + i) : fd_ode_stage1(x[i], sv, gk, c, x0 + i, v0 + i);
            x[i] = o;
            if (PAIR) x[n + i] = o;
        }
    }
}

template <bool V4, bool DPM>
void launch_stage(fd_ctx* ctx, const float* G, float* x, const float* score, float* x0, float* v0, size_t n, int T, int C,
                  const fd_ode_step_coef& c, const fd_dpm_coef& dw, const fd_guide* g, hipStream_t s) {
    const dim3 grid(fd_grid_for(V4 ? n / 4 : n, kBlock, ctx->num_cu));
    if (g && g->pair)
        hipLaunchKernelGGL((k_stage<V4, DPM, true>), grid, dim3(kBlock), 0, s, G, x, score, x0, v0, n, T, C, c, dw, g->w, g->omw);
    else
        hipLaunchKernelGGL((k_stage<V4, DPM, false>), grid, dim3(kBlock), 0, s, G, x, score, x0, v0, n, T, C, c, dw, 0.f, 0.f);
}

// (alpha, s, lambda = log(alpha / s)) of the perturbation kernel at t, in double (sde.py:108-123, 187-210).  VP: s^2 = 1 - alpha^2
// cancels at small t, so it comes from expm1.
struct Marginal {
    double alpha, s, lambda;
};
inline Marginal marginal(const fd_sde_params& p, double t) {
    if (p.kind == 0) {
        const double lmc = -0.25 * t * t * ((double)p.p1 - (double)p.p0) - 0.5 * t * (double)p.p0;
        const double s2 = -std::expm1(2.0 * lmc);
        return Marginal{std::exp(lmc), std::sqrt(s2), lmc - 0.5 * std::log(s2)};
    }
    const double ls = std::log((double)p.p0) + t * std::log((double)p.p1 / (double)p.p0);
    return Marginal{1.0, std::exp(ls), -ls};
}

// The coefficients of one step t -> t_next; h_prev > 0: the log-SNR step before it (second-order multistep weights), else first order.
// false when lambda does not strictly increase (or is not finite); *h_out: this step's log-SNR step.
inline bool dpm_step(const fd_sde_params& p, float t, float t_next, double h_prev, int stage, fd_ode_step_coef* row, fd_dpm_coef* w,
                     double* h_out) {
    const Marginal a = marginal(p, (double)t), b = marginal(p, (double)t_next);
    const double h = b.lambda - a.lambda;
    if (!(std::isfinite(h) && h > 0.0 && a.alpha > 0.0 && a.s > 0.0)) return false;
    const double cD = -b.alpha * std::expm1(-h);
    const double wt = h_prev > 0.0 ? h / (2.0 * h_prev) : 0.0;
    *row = fd_ode_step_coef{(float)(1.0 / a.alpha), (float)a.s, (float)(b.s / a.s), stage, t};
    *w = fd_dpm_coef{(float)(cD * (1.0 + wt)), (float)(-cD * wt)};
    *h_out = h;
    return true;
}

}  // namespace

int fd_dpm_table(fd_ctx* ctx, const fd_sde_params* sde, const float* ts, int n_steps, int solver, std::vector<fd_ode_step_coef>* rows,
                 std::vector<fd_dpm_coef>* dpm) {
    FD_REQUIRE(ctx, n_steps > 0 && (solver == 2 || solver == 3), "fd_sampler_run_dpm: n_steps=%d solver=%d", n_steps, solver);
    for (int i = 0; i <= n_steps; ++i)
        FD_REQUIRE(ctx, std::isfinite(ts[i]), "fd_sampler_run_dpm: timesteps[%d] is not finite", i);
    for (int i = 0; i < n_steps; ++i)
        FD_REQUIRE(ctx, ts[i + 1] < ts[i], "fd_sampler_run_dpm: the grid must be strictly decreasing (t[%d]=%g, t[%d]=%g)", i,
                   (double)ts[i], i + 1, (double)ts[i + 1]);
    rows->assign((size_t)n_steps, fd_ode_step_coef{});
    dpm->assign((size_t)n_steps, fd_dpm_coef{});
    double h_prev = 0.0;
    for (int i = 0; i < n_steps; ++i) {
        const int stage = solver == 2 ? FD_ODE_DDIM : (i == 0 ? FD_ODE_DPM_FIRST : FD_ODE_DPM_2M);
        double h = 0.0;
        FD_REQUIRE(ctx, dpm_step(*sde, ts[i], ts[i + 1], stage == FD_ODE_DPM_2M ? h_prev : 0.0, stage, &(*rows)[i], &(*dpm)[i], &h),
                   "fd_sampler_run_dpm: the log-SNR must be finite and strictly increasing along the grid (t[%d]=%g, t[%d]=%g)", i,
                   (double)ts[i], i + 1, (double)ts[i + 1]);
        h_prev = h;
    }
    return FD_OK;
}

int fd_ode_table(fd_ctx* ctx, const fd_sde_params* sde, const float* ts, int n_steps, int solver,
                 std::vector<fd_ode_step_coef>* rows) {
    FD_REQUIRE(ctx, n_steps > 0 && (solver == 0 || solver == 1), "fd_sampler_run_ode: n_steps=%d solver=%d", n_steps, solver);
    const double dir = (double)ts[1] - (double)ts[0];
    for (int i = 0; i <= n_steps; ++i)
        FD_REQUIRE(ctx, std::isfinite(ts[i]), "fd_sampler_run_ode: timesteps[%d] is not finite", i);
    for (int i = 0; i < n_steps; ++i) {
        const double h = (double)ts[i + 1] - (double)ts[i];
        FD_REQUIRE(ctx, h != 0.0 && (h > 0.0) == (dir > 0.0), "fd_sampler_run_ode: the grid must be strictly monotone (t[%d]=%g, t[%d]=%g)",
                   i, (double)ts[i], i + 1, (double)ts[i + 1]);
    }
    rows->clear();
    rows->reserve((size_t)n_steps * (solver + 1));
    auto row = [&](int i, int stage, float h) {
        const SdeCoef c = fd_sde_coef(*sde, (double)ts[i], 0.f);
        rows->push_back(fd_ode_step_coef{c.a_x, c.g, h, stage, ts[i]});
    };
    for (int i = 0; i < n_steps; ++i) {
        const float h = (float)((double)ts[i + 1] - (double)ts[i]);
        if (solver == 0) {
            row(i, FD_ODE_EULER, h);
        } else {
            row(i, FD_ODE_HEUN_PREDICT, h);
            row(i + 1, FD_ODE_HEUN_CORRECT, h);
        }
    }
    return FD_OK;
}

int fd_solver_rows(fd_ctx* ctx, const fd_sde_params* sde, const float* ts, int n_steps, int solver, std::vector<fd_ode_step_coef>* rows,
                   std::vector<fd_dpm_coef>* dpm, int* nstate) {
    *nstate = solver == 1 ? 2 : solver == 3 ? 1 : 0;
    dpm->clear();
    return solver >= 2 ? fd_dpm_table(ctx, sde, ts, n_steps, solver, rows, dpm) : fd_ode_table(ctx, sde, ts, n_steps, solver, rows);
}

int fd_ode_stage(fd_ctx* ctx, const float* G, float* x, const float* score, float* x0, float* v0, const fd_ode_step_coef& c, int B,
                 int T, int C, hipStream_t s, const fd_dpm_coef* w, const fd_guide* g) {
    const size_t n = (size_t)B * T * C;
    const bool v4 = C % 4 == 0, dpm = c.stage >= FD_ODE_DDIM;
    FD_REQUIRE(ctx, !dpm || (w && (x0 || c.stage == FD_ODE_DDIM)), "fd_ode_stage: a data-prediction stage needs its coefficients and state");
    const fd_dpm_coef dw = dpm ? *w : fd_dpm_coef{};
    if (v4 && dpm) launch_stage<true, true>(ctx, G, x, score, x0, v0, n, T, C, c, dw, g, s);
    else if (v4) launch_stage<true, false>(ctx, G, x, score, x0, v0, n, T, C, c, dw, g, s);
    else if (dpm) launch_stage<false, true>(ctx, G, x, score, x0, v0, n, T, C, c, dw, g, s);
    else launch_stage<false, false>(ctx, G, x, score, x0, v0, n, T, C, c, dw, g, s);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_pf_ode_drift(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* x, const float* score, double t,
                               float* v_out, int B, int T, int C, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, sde && G && x && score && v_out, "fd_pf_ode_drift: null pointer");
    FD_REQUIRE(ctx, sde->kind == 0 || sde->kind == 1, "fd_pf_ode_drift: unknown SDE kind %d", sde->kind);
    FD_REQUIRE(ctx, B > 0 && T > 0 && C > 0, "fd_pf_ode_drift: bad shape B=%d T=%d C=%d", B, T, C);
    FD_REQUIRE(ctx, std::isfinite(t), "fd_pf_ode_drift: t is not finite");
    const size_t n = (size_t)B * T * C;
    const SdeCoef c = fd_sde_coef(*sde, t, 0.f);
    hipLaunchKernelGGL(k_ode_drift, dim3(fd_grid_for(n, kBlock, ctx->num_cu)), dim3(kBlock), 0, (hipStream_t)stream, G, x, score, v_out, n, T, C,
                       c.a_x, c.g);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

// One data-prediction stage from t to t_next on given x, score and previous D: the step-wise twin of fd_sampler_run_dpm.
extern "C" int fd_dpm_stage(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* x, const float* score,
                            const float* d_prev, double t_prev, double t, double t_next, float* x_out, float* d_out, int B, int T,
                            int C, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, sde && G && x && score && x_out && d_out, "fd_dpm_stage: null pointer");
    FD_REQUIRE(ctx, sde->kind == 0 || sde->kind == 1, "fd_dpm_stage: unknown SDE kind %d", sde->kind);
    FD_REQUIRE(ctx, B > 0 && T > 0 && C > 0, "fd_dpm_stage: bad shape B=%d T=%d C=%d", B, T, C);
    FD_REQUIRE(ctx, x_out != d_out && score != x_out && score != d_out && x != d_out && d_prev != x_out,
               "fd_dpm_stage: x_out may alias x and d_out may alias d_prev only");
    const float tf = (float)t, tn = (float)t_next, tp = (float)t_prev;
    FD_REQUIRE(ctx, std::isfinite(tf) && std::isfinite(tn) && tn < tf, "fd_dpm_stage: need finite t_next < t (t=%g, t_next=%g)", t, t_next);
    double h_prev = 0.0, h = 0.0;
    fd_ode_step_coef row;
    fd_dpm_coef w;
    if (d_prev) {
        FD_REQUIRE(ctx, std::isfinite(tp) && tf < tp, "fd_dpm_stage: need finite t < t_prev with d_prev (t_prev=%g, t=%g)", t_prev, t);
        FD_REQUIRE(ctx, dpm_step(*sde, tp, tf, 0.0, FD_ODE_DPM_FIRST, &row, &w, &h_prev),
                   "fd_dpm_stage: the log-SNR must strictly increase from t_prev=%g to t=%g", t_prev, t);
    }
    FD_REQUIRE(ctx, dpm_step(*sde, tf, tn, h_prev, d_prev ? FD_ODE_DPM_2M : FD_ODE_DPM_FIRST, &row, &w, &h),
               "fd_dpm_stage: the log-SNR must strictly increase from t=%g to t_next=%g", t, t_next);
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)B * T * C * sizeof(float);
    if (x_out != x) FD_HIP(ctx, hipMemcpyAsync(x_out, x, bytes, hipMemcpyDeviceToDevice, s));
    if (d_prev && d_out != d_prev) FD_HIP(ctx, hipMemcpyAsync(d_out, d_prev, bytes, hipMemcpyDeviceToDevice, s));
    return fd_ode_stage(ctx, G, x_out, score, d_out, nullptr, row, B, T, C, s, &w);
}
