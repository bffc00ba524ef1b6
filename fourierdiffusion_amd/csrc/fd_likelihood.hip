// fd_likelihood.hip -- log-likelihood of series under the probability-flow ODE (Song et al. 2021, Sec. 4.3 and App. D.2; not in
// the reference, which reports sample-based metrics only):
//   log p_0(x_0) = log p_1(x_1) + int_eps^1 div v(x(t), t) dt,      v(x, t) = -a x - 0.5 (g G_k)^2 s(x, t)
//   div v = -a T C - 0.5 g^2 tr(diag(G^2) ds/dx),     tr(diag(G^2) J) = E_e[e^T diag(G^2) J e] = E_e[<J^T (G^2 e), e>]
// The ODE runs forward in time (data -> latents) on the grid and solvers of fd_ode.hip.  Each score evaluation is the training
// forward (dropout 0: it keeps the activations) and the input-only backward with the constant dout = G^2 e, which gives
// J^T (G^2 e) for the probe e of every row; k_ll_stage then reduces <dx, e> per row, applies the ODE stage and accumulates the
// score part of the divergence integral.  The drift part, -a T C, does not depend on x: the host adds it (float64).
// Reductions are fixed-order in float64 (no atomics): two runs give bit-identical results.
#include <cmath>

#include "fd_ode.h"
#include "fd_score.h"
#include "fd_sde.h"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_ll_fill(float* __restrict__ p, int n, float v) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = v;
}

// dout = G_k^2 e  (built once per run: the input of the VJP is linear, the per-evaluation factor -0.5 g^2 is applied in k_ll_stage)
__global__ __launch_bounds__(kBlock) void k_ll_dout(const float* __restrict__ G, const float* __restrict__ probe,
                                                      float* __restrict__ dout, size_t n, int T, int C) {
    for (size_t e = blockIdx.x * (size_t)kBlock + threadIdx.x; e < n; e += (size_t)gridDim.x * kBlock) {
        const float gk = G[(e / (size_t)C) % (size_t)T];
        dout[e] = (gk * gk) * probe[e];
    }
}

// sum over the block's threads in a fixed order (LDS tree); the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// One workgroup per row b (n_row = T*C elements): r = <dx_b, e_b> (float64, fixed order), x_b <- ODE stage (fd_ode_stage1 of
// fd_mega_params.h), and the divergence integral of the row:
//   Euler           acc += h * (-0.5 g^2 r)
//   Heun predictor  d0 = -0.5 g(t_i)^2 r                    (x0 / v0: the state of fd_ode_stage1)
//   Heun corrector  acc += h/2 * (d0 - 0.5 g(t_{i+1})^2 r)   (the trapezoid of the two stages, as the state update)
// score_div[b] = (float)acc after every stage.
__global__ __launch_bounds__(kBlock) void k_ll_stage(const float* __restrict__ G, float* __restrict__ x, const float* __restrict__ score,
                                                       const float* __restrict__ dx, const float* __restrict__ probe,
                                                       float* __restrict__ x0, float* __restrict__ v0, double* __restrict__ acc,
                                                       double* __restrict__ d0, float* __restrict__ score_div, int T, int C,
                                                       fd_ode_step_coef c) {
    __shared__ double red[kBlock];
    const int n_row = T * C;
    const size_t base = (size_t)blockIdx.x * n_row;
    double r = 0.0;
    for (int i = threadIdx.x; i < n_row; i += kBlock) {
        const size_t e = base + i;
        r += (double)dx[e] * (double)probe[e];
        const float gk = c.g * G[i / C];
        x[e] = fd_ode_stage1(x[e], score[e], gk, c, x0 + e, v0 + e);
    }
    r = block_sum(r, red);
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;
    const double val = -0.5 * (double)c.g * (double)c.g * r;
    double a = acc[b];
    if (c.stage == FD_ODE_EULER) a += (double)c.h * val;
    else if (c.stage == FD_ODE_HEUN_PREDICT) d0[b] = val;
    else a += 0.5 * (double)c.h * (d0[b] + val);
    acc[b] = a;
    score_div[b] = (float)a;
}

// out[b] = sum_{t,c} log N(x_btc; 0, (sigma_p G_t)^2), one workgroup per series (float64, fixed order)
__global__ __launch_bounds__(kBlock) void k_ll_prior(const float* __restrict__ G, const float* __restrict__ x, float* __restrict__ out,
                                                       int T, int C, double sigma_p) {
    __shared__ double red[kBlock];
    const int n_row = T * C;
    const size_t base = (size_t)blockIdx.x * n_row;
    double q = 0.0, lg = 0.0;
    for (int i = threadIdx.x; i < n_row; i += kBlock) {
        const double sd = sigma_p * (double)G[i / C];
        const double z = (double)x[base + i] / sd;
        q += z * z;
        lg += log(sd);
    }
    const double s = block_sum(-0.5 * q - lg, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(s - 0.5 * (double)n_row * log(2.0 * M_PI));
}

// The stage state of one run, outside the arena (the training forward and its VJP own the arena between them): grow-only,
// freed with the context
struct LlBufs {
    float *tvec, *dout, *score, *dx, *x0, *v0;
    double *acc, *d0;
};
int ll_buffers(fd_ctx* ctx, int B, size_t n, bool heun, LlBufs* o) {
    auto fl = [](size_t k) { return fd_ws::padded(k * sizeof(float)); };
    const size_t need = fl(B) + (heun ? 5 : 3) * fl(n) + 2 * fd_ws::padded((size_t)B * sizeof(double));
    if (ctx->ll_bytes < need) {
        if (ctx->ll_buf) (void)hipFree(ctx->ll_buf);      // (synchronising: an earlier run on any stream has finished with it)
        ctx->ll_buf = nullptr;
        ctx->ll_bytes = 0;
        FD_HIP(ctx, hipMalloc(&ctx->ll_buf, need));
        ctx->ll_bytes = need;
    }
    char* p = (char*)ctx->ll_buf;
    auto take = [&](size_t bytes) { char* q = p; p += bytes; return q; };
    o->tvec = (float*)take(fl(B));
    o->dout = (float*)take(fl(n));
    o->score = (float*)take(fl(n));
    o->dx = (float*)take(fl(n));
    o->x0 = heun ? (float*)take(fl(n)) : nullptr;
    o->v0 = heun ? (float*)take(fl(n)) : nullptr;
    o->acc = (double*)take(fd_ws::padded((size_t)B * sizeof(double)));
    o->d0 = (double*)take(fd_ws::padded((size_t)B * sizeof(double)));
    return FD_OK;
}

// restores the model's training arithmetic when the run returns
struct TrainModeScope {
    fd_score* m;
    int saved;
    TrainModeScope(fd_score* mm, int mode) : m(mm), saved(mm->train_mode) { m->train_mode = mode; }
    ~TrainModeScope() { m->train_mode = saved; }
};

}  // namespace

extern "C" int fd_prior_logp(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* x, float* out, int B, int T, int C,
                             void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, sde && G && x && out, "fd_prior_logp: null pointer");
    FD_REQUIRE(ctx, sde->kind == 0 || sde->kind == 1, "fd_prior_logp: unknown SDE kind %d", sde->kind);
    FD_REQUIRE(ctx, B > 0 && T > 0 && C > 0, "fd_prior_logp: bad shape B=%d T=%d C=%d", B, T, C);
    const double sigma_p = (sde->kind == 1) ? (double)sde->p1 : 1.0;      // the scale of fd_prior_sample
    hipLaunchKernelGGL(k_ll_prior, dim3(B), dim3(kBlock), 0, (hipStream_t)stream, G, x, out, T, C, sigma_p);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_likelihood_run(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, int solver,
                                 float* x, const float* probes, float* score_div, int B, int mode, void* stream) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, sde && G && timesteps && x && probes && score_div, "fd_likelihood_run: null pointer");
    FD_REQUIRE(ctx, sde->kind == 0 || sde->kind == 1, "fd_likelihood_run: unknown SDE kind %d", sde->kind);
    FD_REQUIRE(ctx, n_steps > 0 && B > 0, "fd_likelihood_run: n_steps=%d B=%d", n_steps, B);
    FD_REQUIRE(ctx, solver == 0 || solver == 1, "fd_likelihood_run: solver %d (0 Euler, 1 Heun)", solver);
    FD_REQUIRE(ctx, mode == FD_MODE_F32 || mode == FD_MODE_BF16, "fd_likelihood_run: unknown mode %d", mode);
    FD_REQUIRE(ctx, (double)timesteps[1] > (double)timesteps[0], "fd_likelihood_run: the grid must increase (data -> latents)");
    if (!m->prepared) return fd_fail(ctx, FD_ERR_STATE, "fd_likelihood_run: call fd_score_prepare first");
    std::vector<fd_ode_step_coef> rows;
    if (int rc = fd_ode_table(ctx, sde, timesteps, n_steps, solver, &rows)) return rc;
    // bf16: the bf16 training kernels where the model has them, else (other backbones, widths) the exact-f32 ones
    const bool bf16 = mode == FD_MODE_BF16 && m->backbone == FD_BACKBONE_TRANSFORMER && fd_train_bf16_supported(m);
    TrainModeScope tm(m, bf16 ? FD_MODE_BF16 : FD_MODE_F32);
    hipStream_t s = (hipStream_t)stream;
    const int T = m->d.max_len, C = m->d.n_channels;
    const size_t n = (size_t)B * T * C;
    LlBufs b;
    if (int rc = ll_buffers(ctx, B, n, solver == 1, &b)) return rc;
    const unsigned ew = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, (size_t)ctx->num_cu * 16);
    hipLaunchKernelGGL(k_ll_dout, dim3(ew), dim3(kBlock), 0, s, G, probes, b.dout, n, T, C);
    FD_HIP(ctx, hipMemsetAsync(b.acc, 0, (size_t)B * sizeof(double), s));
    for (const fd_ode_step_coef& c : rows) {
        hipLaunchKernelGGL(k_ll_fill, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, s, b.tvec, B, c.t);
        if (int rc = fd_score_forward_train(m, x, b.tvec, b.score, B, 0.f, 0, 0, s)) return rc;
        if (int rc = fd_score_input_vjp(m, b.dout, b.dx, s)) return rc;
        hipLaunchKernelGGL(k_ll_stage, dim3(B), dim3(kBlock), 0, s, G, x, b.score, b.dx, probes, b.x0, b.v0, b.acc, b.d0, score_div, T,
                           C, c);
        FD_LAUNCH_CHECK(ctx);
    }
    return FD_OK;
}
