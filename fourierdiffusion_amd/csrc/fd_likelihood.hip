// fd_likelihood.hip -- log-likelihood of series under the probability-flow ODE (Song et al. 2021, Sec. 4.3 and App. D.2; not in
// the reference, which reports sample-based metrics only):
//   log p_0(x_0) = log p_1(x_1) + int_eps^1 div v(x(t), t) dt,      v(x, t) = -a x - 0.5 (g G_k)^2 s(x, t)
//   div v = -a T C - 0.5 g^2 tr(diag(G^2) ds/dx),     tr(diag(G^2) J) = E_e[e^T diag(G^2) J e] = E_e[<J^T (G^2 e), e>]
// The ODE runs forward in time (data -> latents) on the grid and solvers of fd_ode.hip.  Each score evaluation is the training
// forward (dropout 0: it keeps the activations) and the input-only backward with the constant dout = G^2 e, which gives
// J^T (G^2 e) for the probe e of every row; k_ll_stage then reduces <dx, e> per row, applies the ODE stage and accumulates the
// score part of the divergence integral.  The drift part, -a T C, does not depend on x: the host adds it (float64).
// Reductions are fixed-order in float64 (no atomics): two runs give bit-identical results.
// fd_likelihood_run_adaptive runs the same evaluation under per-row Dormand-Prince 5(4) step control (scipy's RK45), below.
#include <cmath>

#include "fd_engine.h"
#include "fd_loop.h"
#include "fd_ode.h"
#include "fd_sde.h"

namespace {

constexpr int kBlock = 256;

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

struct LlBufs {
    float *tvec, *dout, *score, *dx, *x0, *v0;
    double *acc, *d0;
};
int ll_buffers(fd_ctx* ctx, int B, size_t n, bool heun, LlBufs* o) {
    return fd_ll_carve(ctx, [&](auto take) {
        o->tvec = (float*)take(B * sizeof(float));
        o->dout = (float*)take(n * sizeof(float));
        o->score = (float*)take(n * sizeof(float));
        o->dx = (float*)take(n * sizeof(float));
        o->x0 = heun ? (float*)take(n * sizeof(float)) : nullptr;
        o->v0 = heun ? (float*)take(n * sizeof(float)) : nullptr;
        o->acc = (double*)take(B * sizeof(double));
        o->d0 = (double*)take(B * sizeof(double));
    });
}

// The frame of both runs around body(): the evaluations run in the training arithmetic (bf16: the bf16 training kernels where the
// model has them, else -- other backbones, widths -- the exact-f32 ones), and dout = G^2 e is built first
template <class Body>
int ll_frame(fd_score* m, int mode, const float* G, const float* probes, float* dout, int B, hipStream_t s, Body body) {
    fd_train_mode_scope tm(m, fd_diff_train_mode(m, mode));
    fd_label_dropout_scope ld(m, 0.f);      // log p(x | y) of the labels as bound (fd_score_set_labels)
    const int T = m->d.max_len, C = m->d.n_channels;
    const size_t n = (size_t)B * T * C;
    const unsigned ew = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, (size_t)m->ctx->num_cu * 16);
    hipLaunchKernelGGL(k_ll_dout, dim3(ew), dim3(kBlock), 0, s, G, probes, dout, n, T, C);
    return body();
}

// ---------------------------------------------------------------- adaptive integration (Dormand-Prince 5(4), scipy's RK45)
// Each row b is one ODE on the augmented state y_b = [x_b (T*C values), acc_b] from t0 to t_bound:
//   dx/dt = v(x, t),   dacc/dt = div v = -a(t) T C - 0.5 g(t)^2 <(ds/dx)^T (G^2 e_b), e_b>
// with the step control of scipy.integrate.RK45 (select_initial_step, min_step, error norm, SAFETY / MIN_FACTOR / MAX_FACTOR),
// every row on its own grid.  The host enqueues evaluations; every evaluation is training forward + input VJP + k_ll_rk_stage,
// which consumes the evaluation as stage `stage` of its row and writes the row's next network input (xin, tvec).  The controller
// (t, h, acc, stage divergences) is float64 per row, written by thread 0 of the row's workgroup; x and the stage vectors K_j are
// fp32, their combinations formed in float64.  x (the caller's buffer) holds the last accepted state.
enum RkStage { RK_INIT0 = -2, RK_INIT1 = -1, RK_FINAL = 6 };      // 1..5: the interior stages of an attempt
enum RkStatus { RK_RUNNING = 0, RK_CONVERGED = 1, RK_TOO_SMALL = 2, RK_MAX_EVALS = 3 };

__constant__ double kRkC[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
__constant__ double kRkA[6][5] = {{0, 0, 0, 0, 0},
                                  {1.0 / 5, 0, 0, 0, 0},
                                  {3.0 / 40, 9.0 / 40, 0, 0, 0},
                                  {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
                                  {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
                                  {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__constant__ double kRkB[6] = {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
__constant__ double kRkE[7] = {-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
constexpr double kRkSafety = 0.9, kRkMinFactor = 0.2, kRkMaxFactor = 10.0, kRkErrExp = -1.0 / 5;

struct RkRow {
    double t;          // last accepted time
    double t_eval;     // time of the row's next evaluation
    double h_abs;      // step magnitude (scipy's h_abs)
    double h;          // step of the current attempt (t_new - t)
    double t_new;      // end of the current attempt
    double min_step;   // 10 ulp(t)
    double acc;        // divergence integral up to t
    double acc_new;    // ... up to t_new (5th-order)
    double kacc[7];    // divergence at the stages (kacc[0]: FSAL, at t)
    double h0, d1;     // select_initial_step
    int status, nfe, n_grid, rejected;
};

struct RkArgs {
    const float* G;
    float* x;            // (B,T,C) last accepted state, in place
    float* xin;          // (B,T,C) the network input of the next evaluation
    const float* score;  // (B,T,C) s(xin, tvec)
    const float* dx;     // (B,T,C) (ds/dx)^T (G^2 e)
    const float* probe;  // (B,T,C) e
    float* K;            // 7 (B,T,C) stage vectors, K_j at K + j * n
    float* tvec;         // (B,) time the training forward reads
    RkRow* row;          // (B,)
    double* grid;        // (B, gcap) accepted times, t0 first
    size_t n;            // B*T*C
    int T, C, gcap, max_evals;
    fd_sde_params sde;
    double t_bound, rtol, atol;
    int stage;
};

// a(t), g(t) of fd_sde_coef (rounded to float as there), from a float64 t; a64: a(t) unrounded, for the drift part of div v (it
// depends on t alone and is linear in t, so every row's quadrature of it is exact to rounding: rows of one series agree on it)
__device__ __forceinline__ void rk_coef(const fd_sde_params& p, double t, float* a, float* g, double* a64) {
    if (p.kind == 0) {
        const double beta = (double)p.p0 + t * ((double)p.p1 - (double)p.p0);
        *a64 = 0.5 * beta;
        *a = (float)(0.5 * beta);
        *g = (float)sqrt(beta);
    } else {
        const double r = (double)p.p1 / (double)p.p0;
        *a64 = 0.0;
        *a = 0.f;
        *g = (float)((double)p.p0 * sqrt(2.0 * log(r)) * pow(r, t));
    }
}

// scipy's RungeKutta._step_impl from the top of its retry loop (thread 0): freeze the row or set up the attempt's first stage;
// returns whether the row still runs
__device__ bool rk_attempt(RkRow& r, const RkArgs& p) {
    if (r.h_abs < r.min_step) { r.status = RK_TOO_SMALL; return false; }
    if (r.nfe + 6 > p.max_evals) { r.status = RK_MAX_EVALS; return false; }
    r.nfe += 6;
    double t_new = r.t + r.h_abs;
    if (t_new > p.t_bound) t_new = p.t_bound;
    r.h = t_new - r.t;
    r.h_abs = fabs(r.h);
    r.t_new = t_new;
    r.t_eval = r.t + kRkC[1] * r.h;
    return true;
}
// the start of a new step from the accepted time r.t
__device__ bool rk_new_step(RkRow& r, const RkArgs& p) {
    r.min_step = 10.0 * fabs(nextafter(r.t, INFINITY) - r.t);
    if (r.h_abs < r.min_step) r.h_abs = r.min_step;
    r.rejected = 0;
    return rk_attempt(r, p);
}

__global__ __launch_bounds__(kBlock) void k_ll_rk_init(RkArgs p, double t0) {
    const int b = blockIdx.x, n_row = p.T * p.C;
    const size_t base = (size_t)b * n_row;
    for (int i = threadIdx.x; i < n_row; i += kBlock) p.xin[base + i] = p.x[base + i];
    if (threadIdx.x != 0) return;
    RkRow& r = p.row[b];
    r.t = r.t_eval = t0;
    r.h_abs = r.h = r.h0 = r.d1 = 0.0;
    r.t_new = t0;
    r.min_step = 0.0;
    r.acc = r.acc_new = 0.0;
    for (int j = 0; j < 7; ++j) r.kacc[j] = 0.0;
    r.status = RK_RUNNING;
    r.nfe = 0;
    r.rejected = 0;
    r.n_grid = 1;
    p.grid[(size_t)b * p.gcap] = t0;
    p.tvec[b] = (float)t0;
}

// One workgroup per row: consumes the evaluation (score, dx) at (xin, t_eval) as stage p.stage, writes the next input.
//   INIT0  f0 = K_0;  d0, d1 of select_initial_step;  next input y0 + h0 f0
//   INIT1  f1;  d2, h_abs;  nfe = 2;  first attempt: next input y + h A_10 K_0
//   1..5   K_s;  next input y + h sum_j A_{s+1,j} K_j  (stage 5: y_new = y + h sum_j B_j K_j, at t_new)
//   FINAL  K_6 = f(t_new, y_new);  error norm over the T*C + 1 components;  accept (x = y_new, K_0 = K_6, grid) or reject;
//          next attempt's first input
// Frozen rows return at once (their input and time stay as they were: the launch keeps its size).  Reductions: block_sum, fixed
// order, float64.
__global__ __launch_bounds__(kBlock) void k_ll_rk_stage(RkArgs p) {
    __shared__ double red[kBlock];
    __shared__ double bc[3];      // broadcast from thread 0: the factor of the next input, flags, the attempt's step
    const int b = blockIdx.x;
    RkRow* rp = p.row + b;
    if (rp->status != RK_RUNNING) return;
    const int n_row = p.T * p.C, st = p.stage;
    const size_t base = (size_t)b * n_row, n = p.n;
    float a, g;
    double a64;
    rk_coef(p.sde, rp->t_eval, &a, &g, &a64);
    const double h = rp->h;
    float* K = p.K;
    double r = 0.0, q0 = 0.0, q1 = 0.0;
    for (int i = threadIdx.x; i < n_row; i += kBlock) {
        const size_t e = base + i;
        r += (double)p.dx[e] * (double)p.probe[e];
        const float xi = p.xin[e];
        const float v = fd_ode_velocity(xi, p.score[e], a, g * p.G[i / p.C]);
        const double y = (double)p.x[e];
        if (st == RK_INIT0) {
            K[e] = v;
            const double sc = p.atol + fabs(y) * p.rtol;
            q0 += (y / sc) * (y / sc);
            q1 += ((double)v / sc) * ((double)v / sc);
        } else if (st == RK_INIT1) {
            const double sc = p.atol + fabs(y) * p.rtol;
            const double d = ((double)v - (double)K[e]) / sc;
            q0 += d * d;
        } else if (st < 5) {
            K[st * n + e] = v;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (j <= st) s += kRkA[st + 1][j] * (double)(j == st ? v : K[j * n + e]);
            p.xin[e] = (float)(y + s * h);
        } else if (st == 5) {
            K[5 * n + e] = v;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) s += (double)(j == 5 ? v : K[j * n + e]) * kRkB[j];
            p.xin[e] = (float)(y + h * s);
        } else {
            K[6 * n + e] = v;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) s += (double)(j == 6 ? v : K[j * n + e]) * kRkE[j];
            const double err = s * h;
            const double sc = p.atol + fmax(fabs(y), fabs((double)xi)) * p.rtol;
            q0 += (err / sc) * (err / sc);
        }
    }
    r = block_sum(r, red);
    if (st == RK_INIT0 || st == RK_INIT1 || st == RK_FINAL) q0 = block_sum(q0, red);
    if (st == RK_INIT0) q1 = block_sum(q1, red);
    if (threadIdx.x == 0) {
        RkRow& R = *rp;
        const double kacc = -a64 * (double)n_row - 0.5 * (double)g * (double)g * r;
        const double dims = (double)n_row + 1.0;
        const double interval = p.t_bound - R.t;
        double fac = 0.0;
        int flags = 0;      // bit 0: write the next input from (x, K_0), bit 1: accept (x = y_new, K_0 = K_6) first
        if (st == RK_INIT0) {
            R.kacc[0] = kacc;
            const double sc = p.atol;      // the acc component: y0 = 0
            const double d0 = sqrt(q0 / dims), d1 = sqrt((q1 + (kacc / sc) * (kacc / sc)) / dims);
            double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
            h0 = fmin(h0, interval);
            R.h0 = h0;
            R.d1 = d1;
            R.t_eval = R.t + h0;
            fac = h0;
            flags = 1;
        } else if (st == RK_INIT1) {
            const double dacc = (kacc - R.kacc[0]) / p.atol;
            const double d2 = sqrt((q0 + dacc * dacc) / dims) / R.h0;
            const double h1 = (R.d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, R.h0 * 1e-3) : pow(0.01 / fmax(R.d1, d2), 1.0 / 5);
            R.h_abs = fmin(fmin(100 * R.h0, h1), interval);
            R.nfe = 2;
            if (rk_new_step(R, p)) { fac = kRkA[1][0]; flags = 1; }
        } else if (st < 5) {
            R.kacc[st] = kacc;
            R.t_eval = R.t + kRkC[st + 1] * h;
        } else if (st == 5) {
            R.kacc[5] = kacc;
            double s = 0.0;
            for (int j = 0; j < 6; ++j) s += R.kacc[j] * kRkB[j];
            R.acc_new = R.acc + h * s;
            R.t_eval = R.t + h;      // (scipy evaluates f_new at t + h, not at t_new)
        } else {
            R.kacc[6] = kacc;
            double s = 0.0;
            for (int j = 0; j < 7; ++j) s += R.kacc[j] * kRkE[j];
            const double err = s * h;
            const double sc = p.atol + fmax(fabs(R.acc), fabs(R.acc_new)) * p.rtol;
            const double en = sqrt((q0 + (err / sc) * (err / sc)) / dims);
            if (en < 1.0) {
                double factor = en == 0.0 ? kRkMaxFactor : fmin(kRkMaxFactor, kRkSafety * pow(en, kRkErrExp));
                if (R.rejected) factor = fmin(1.0, factor);
                R.h_abs *= factor;
                R.t = R.t_new;
                R.acc = R.acc_new;
                R.kacc[0] = R.kacc[6];
                p.grid[(size_t)b * p.gcap + R.n_grid++] = R.t;
                flags = 2;
                if (R.t >= p.t_bound) R.status = RK_CONVERGED;
                else if (rk_new_step(R, p)) { fac = kRkA[1][0]; flags |= 1; }
            } else {
                R.h_abs *= fmax(kRkMinFactor, kRkSafety * pow(en, kRkErrExp));
                R.rejected = 1;
                if (rk_attempt(R, p)) { fac = kRkA[1][0]; flags = 1; }
            }
        }
        p.tvec[b] = (float)R.t_eval;
        bc[0] = fac;
        bc[1] = (double)flags;
        bc[2] = R.h;
    }
    if (st != RK_INIT0 && st != RK_INIT1 && st != RK_FINAL) return;
    __syncthreads();
    const int flags = (int)bc[1];
    if (flags == 0) return;
    const double fac = bc[0], hn = bc[2];      // (INIT0: the input y0 + h0 f0; else y + (A_10 K_0) h)
    for (int i = threadIdx.x; i < n_row; i += kBlock) {
        const size_t e = base + i;
        float xv = p.x[e], k0 = K[e];
        if (flags & 2) {      // accepted: y = y_new (the input of the last stage), K_0 = K_6 (FSAL)
            xv = p.xin[e];
            k0 = K[6 * n + e];
            p.x[e] = xv;
            K[e] = k0;
        }
        if (flags & 1) p.xin[e] = st == RK_INIT0 ? (float)((double)xv + fac * (double)k0) : (float)((double)xv + fac * (double)k0 * hn);
    }
}

// out[0] = the number of running rows (one workgroup)
__global__ __launch_bounds__(kBlock) void k_ll_rk_count(const RkRow* __restrict__ row, int B, int* __restrict__ out) {
    __shared__ int cnt[kBlock];
    int c = 0;
    for (int b = threadIdx.x; b < B; b += kBlock) c += row[b].status == RK_RUNNING;
    cnt[threadIdx.x] = c;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) cnt[threadIdx.x] += cnt[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = cnt[0];
}

// the per-row results: div_out, nfe_out, status_out, and the grid NaN-padded to grid_cap (grid_out may be null)
__global__ __launch_bounds__(kBlock) void k_ll_rk_out(const RkRow* __restrict__ row, const double* __restrict__ grid, int gcap,
                                                        double* __restrict__ div_out, int* __restrict__ nfe_out,
                                                        int* __restrict__ status_out, double* __restrict__ grid_out, int grid_cap) {
    const int b = blockIdx.x;
    const RkRow& r = row[b];
    if (threadIdx.x == 0) {
        div_out[b] = r.acc;
        nfe_out[b] = r.nfe;
        status_out[b] = r.status;
    }
    if (!grid_out) return;
    for (int i = threadIdx.x; i < grid_cap; i += kBlock)
        grid_out[(size_t)b * grid_cap + i] = i < r.n_grid ? grid[(size_t)b * gcap + i] : __longlong_as_double(0x7ff8000000000000LL);      // NaN (bits: -fno-honor-nans)
}

// the state of one adaptive run in the same grow-only buffer as fd_likelihood_run's (outside the arena)
struct RkBufs {
    float *tvec, *dout, *score, *dx, *xin, *K;
    RkRow* row;
    double* grid;
    int* count;
};
int rk_buffers(fd_ctx* ctx, int B, size_t n, int gcap, RkBufs* o) {
    return fd_ll_carve(ctx, [&](auto take) {
        o->tvec = (float*)take(B * sizeof(float));
        o->dout = (float*)take(n * sizeof(float));
        o->score = (float*)take(n * sizeof(float));
        o->dx = (float*)take(n * sizeof(float));
        o->xin = (float*)take(n * sizeof(float));
        o->K = (float*)take(7 * fd_ws::padded(n * sizeof(float)));
        o->row = (RkRow*)take(B * sizeof(RkRow));
        o->grid = (double*)take((size_t)B * gcap * sizeof(double));
        o->count = (int*)take(sizeof(int));
    });
}

// the two completion events of the host loop (destroyed on every return)
struct RkEvents {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~RkEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
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
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_likelihood_run")) return rc;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x && probes && score_div, "fd_likelihood_run: null pointer");
    FD_REQUIRE(ctx, n_steps > 0, "fd_likelihood_run: n_steps=%d", n_steps);
    FD_REQUIRE(ctx, solver == 0 || solver == 1, "fd_likelihood_run: solver %d (0 Euler, 1 Heun)", solver);
    FD_REQUIRE(ctx, (double)timesteps[1] > (double)timesteps[0], "fd_likelihood_run: the grid must increase (data -> latents)");
    std::vector<fd_ode_step_coef> rows;
    if (int rc = fd_ode_table(ctx, sde, timesteps, n_steps, solver, &rows)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int T = m->d.max_len, C = m->d.n_channels;
    LlBufs b;
    if (int rc = ll_buffers(ctx, B, (size_t)B * T * C, solver == 1, &b)) return rc;
    return ll_frame(m, mode, G, probes, b.dout, B, s, [&] {
        FD_HIP(ctx, hipMemsetAsync(b.acc, 0, (size_t)B * sizeof(double), s));
        for (const fd_ode_step_coef& c : rows) {
            fd_fill(b.tvec, B, c.t, s);
            if (int rc = fd_score_forward_train(m, x, b.tvec, b.score, B, 0.f, 0, 0, s)) return rc;
            if (int rc = fd_score_input_vjp(m, b.dout, b.dx, s)) return rc;
            hipLaunchKernelGGL(k_ll_stage, dim3(B), dim3(kBlock), 0, s, G, x, b.score, b.dx, probes, b.x0, b.v0, b.acc, b.d0, score_div,
                               T, C, c);
            FD_LAUNCH_CHECK(ctx);
        }
        return (int)FD_OK;
    });
}

extern "C" int fd_likelihood_run_adaptive(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol,
                                          double atol, int max_evals, float* x, const float* probes, double* div_out, int* nfe_out,
                                          int* status_out, double* grid_out, int grid_cap, int B, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_likelihood_run_adaptive")) return rc;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && x && probes && div_out && nfe_out && status_out, "fd_likelihood_run_adaptive: null pointer");
    FD_REQUIRE(ctx, std::isfinite(t0) && std::isfinite(t1) && t1 > t0, "fd_likelihood_run_adaptive: need finite t0 < t1 (%g, %g)",
               t0, t1);
    FD_REQUIRE(ctx, std::isfinite(rtol) && std::isfinite(atol) && rtol > 0 && atol > 0,
               "fd_likelihood_run_adaptive: need rtol > 0 and atol > 0 (%g, %g)", rtol, atol);
    FD_REQUIRE(ctx, max_evals >= 8, "fd_likelihood_run_adaptive: max_evals=%d < 8 (one step)", max_evals);
    const int max_attempts = (max_evals - 2) / 6, gcap = 1 + max_attempts;
    FD_REQUIRE(ctx, !grid_out || grid_cap >= gcap, "fd_likelihood_run_adaptive: grid_cap=%d < 1 + (max_evals - 2) / 6 = %d",
               grid_cap, gcap);
    hipStream_t s = (hipStream_t)stream;
    const int T = m->d.max_len, C = m->d.n_channels;
    const size_t n = (size_t)B * T * C;
    RkBufs b;
    if (int rc = rk_buffers(ctx, B, n, gcap, &b)) return rc;
    if (!ctx->ll_host) FD_HIP(ctx, hipHostMalloc((void**)&ctx->ll_host, 2 * sizeof(int), hipHostMallocDefault));
    RkEvents ev;
    for (hipEvent_t& e : ev.e) FD_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));

    RkArgs a{G, x, b.xin, b.score, b.dx, probes, b.K, b.tvec, b.row, b.grid, n, T, C, gcap, max_evals, *sde, t1, rtol, atol, 0};
    return ll_frame(m, mode, G, probes, b.dout, B, s, [&] {
        hipLaunchKernelGGL(k_ll_rk_init, dim3(B), dim3(kBlock), 0, s, a, t0);
        FD_LAUNCH_CHECK(ctx);
        auto eval = [&](int stage) {
            if (int rc = fd_score_forward_train(m, b.xin, b.tvec, b.score, B, 0.f, 0, 0, s)) return rc;
            if (int rc = fd_score_input_vjp(m, b.dout, b.dx, s)) return rc;
            a.stage = stage;
            hipLaunchKernelGGL(k_ll_rk_stage, dim3(B), dim3(kBlock), 0, s, a);
            FD_LAUNCH_CHECK(ctx);
            return (int)FD_OK;
        };
        if (int rc = eval(RK_INIT0)) return rc;
        if (int rc = eval(RK_INIT1)) return rc;
        // Attempt k (6 evaluations) ends with the count of the rows still running, copied to host word k % 2 and marked by event
        // k % 2.  The host reads attempt k's count once attempt k + 1 is queued: the device never waits on the host, and at most
        // one attempt runs after the last row froze.  Every row freezes within max_attempts attempts (an attempt past max_evals is
        // not started), so the loop needs no other bound.
        for (int k = 0; k < max_attempts; ++k) {
            for (int st = 1; st <= RK_FINAL; ++st)
                if (int rc = eval(st)) return rc;
            hipLaunchKernelGGL(k_ll_rk_count, dim3(1), dim3(kBlock), 0, s, b.row, B, b.count);
            FD_LAUNCH_CHECK(ctx);
            FD_HIP(ctx, hipMemcpyAsync(ctx->ll_host + (k & 1), b.count, sizeof(int), hipMemcpyDeviceToHost, s));
            FD_HIP(ctx, hipEventRecord(ev.e[k & 1], s));
            if (k > 0) {
                FD_HIP(ctx, hipEventSynchronize(ev.e[(k - 1) & 1]));
                if (ctx->ll_host[(k - 1) & 1] == 0) break;
            }
        }
        hipLaunchKernelGGL(k_ll_rk_out, dim3(B), dim3(kBlock), 0, s, b.row, b.grid, gcap, div_out, nfe_out, status_out, grid_out,
                           grid_cap);
        FD_LAUNCH_CHECK(ctx);
        return (int)FD_OK;
    });
}
