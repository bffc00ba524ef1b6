// fd_ode.hip -- probability-flow ODE of the score SDE (Song et al. 2021, Sec. 4.3; not in the reference, whose only sampler is
// Euler-Maruyama over the reverse SDE, src/fdiff/sampling/sampler.py:83-104):
//   dx/dt = v(x, t) = -a x - 0.5 (g G_k)^2 s(x, t)      (VP a = beta/2, g = sqrt(beta); VE a = 0, g of fd_sde_coef)
// integrated by Euler or Heun on a strictly monotone grid in either direction (t 1 -> eps samples / decodes, eps -> 1 encodes).
// Here: the velocity alone (fd_pf_ode_drift), the coefficient table every loop form runs from, and the elementwise stage of the
// step-by-step loop (fp32 parity mode, the MLP / LSTM backbones, FDIFF_SAMPLER_STEPWISE).  No random numbers are drawn.
#include <cmath>

#include "fd_ode.h"
#include "fd_sde.h"

namespace {

constexpr int kBlock = 256;

inline int grid_for(size_t items, int num_cu) {
    size_t blocks = (items + kBlock - 1) / kBlock;
    const size_t cap = (size_t)num_cu * 64;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

// v = -a x - 0.5 (g G_k)^2 s, one element per thread and iteration
__global__ __launch_bounds__(kBlock) void k_ode_drift(const float* __restrict__ G, const float* __restrict__ x,
                                                        const float* __restrict__ score, float* __restrict__ v, size_t n, int T,
                                                        int C, float a_x, float g) {
    for (size_t e = blockIdx.x * (size_t)kBlock + threadIdx.x; e < n; e += (size_t)gridDim.x * kBlock) {
        const int t = (int)((e / (size_t)C) % (size_t)T);
        v[e] = fd_ode_velocity(x[e], score[e], a_x, g * G[t]);
    }
}

// one stage on (B,T,C).  V4 (C % 4 == 0): a thread owns four elements of one row, as the persistent kernel's epilogue lanes do
template <bool V4>
__global__ __launch_bounds__(kBlock) void k_ode_stage(const float* __restrict__ G, float* __restrict__ x,
                                                        const float* __restrict__ score, float* __restrict__ x0,
                                                        float* __restrict__ v0, size_t n, int T, int C, fd_ode_step_coef c) {
    const size_t items = V4 ? n / 4 : n;
    for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < items; i += (size_t)gridDim.x * kBlock) {
        if (V4) {
            const size_t e = 4 * i;
            const float gk = c.g * G[(e / (size_t)C) % (size_t)T];
            const float4 xv = *reinterpret_cast<const float4*>(x + e);
            const float4 sv = *reinterpret_cast<const float4*>(score + e);
            *reinterpret_cast<float4*>(x + e) = fd_ode_stage4(xv, sv.x, sv.y, sv.z, sv.w, gk, c, x0 + e, v0 + e);
        } else {
            const float gk = c.g * G[(i / (size_t)C) % (size_t)T];
            x[i] = fd_ode_stage1(x[i], score[i], gk, c, x0 + i, v0 + i);
        }
    }
}

}  // namespace

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

int fd_ode_stage(fd_ctx* ctx, const float* G, float* x, const float* score, float* x0, float* v0, const fd_ode_step_coef& c, int B,
                 int T, int C, hipStream_t s) {
    const size_t n = (size_t)B * T * C;
    if (C % 4 == 0)
        hipLaunchKernelGGL(k_ode_stage<true>, dim3(grid_for(n / 4, ctx->num_cu)), dim3(kBlock), 0, s, G, x, score, x0, v0, n, T, C, c);
    else
        hipLaunchKernelGGL(k_ode_stage<false>, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, s, G, x, score, x0, v0, n, T, C, c);
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
    hipLaunchKernelGGL(k_ode_drift, dim3(grid_for(n, ctx->num_cu)), dim3(kBlock), 0, (hipStream_t)stream, G, x, score, v_out, n, T, C,
                       c.a_x, c.g);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
