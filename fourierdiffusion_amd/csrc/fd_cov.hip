// fd_cov.hip -- covariate-conditional score models and classifier-free guidance on covariates.  NOT in the reference, whose
// ScoreModule drops batch.y (src/fdiff/models/score_models.py:67-94).
//
// A covariate model (fd_score_create_cov, cond_dim = P in [1, 64]) owns five more tensors behind every other one of the layout:
//   cov_encoder.0.weight (D, P), cov_encoder.0.bias (D), cov_encoder.2.weight (D, D), cov_encoder.2.bias (D), cov_encoder.null (D)
// and reads a float vector c_b (P) per series.  k_cov_embed, launched directly behind k_time_embed by both of its wrappers
// (fd_score_f32.hip), ends the time embedding with
//   temb[b, :] += keep_b ? W2 silu(W1 c_b + b1) + b2 : null                 (fp32, added last)
// which conditions every forward and training path outside the persistent sampling kernel, as the class table does (fd_cfg.hip).
// Here: the covariate path of the ABI (fd_score_set_covariates), covariate dropout (the keep bytes: k_cov_keep, the lane rule of
// k_label_dropout in its counter window), the encoder gradient (k_cov_bwd_rows, k_cov_bwd_reduce) and the guided entry points, which
// run the loop bodies of fd_sampler.hip with a covariate guide (fd_loop.h): one forward on 2B rows -- the covariates twice, keep =
// [1 .. 1 ; 0 .. 0] -- and the PAIR step kernels of fd_cfg.hip / fd_ode.hip, unchanged.
#include <cmath>

#include "fd_loop.h"
#include "fd_philox.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRowBlock = 128;      // k_cov_embed / k_cov_bwd_rows: one workgroup per row

// x sigmoid(x) as x / (1 + exp(-x)): expf and an IEEE division (exp(-x) = inf for x < -88.7 gives -0)
__device__ __forceinline__ float cov_silu(float x) { return x / (1.0f + expf(-x)); }
// d silu / d x = s (1 + x (1 - s)), s = sigmoid(x)
__device__ __forceinline__ float cov_dsilu(float x) {
    const float sg = 1.0f / (1.0f + expf(-x));
    return sg * (1.0f + x * (1.0f - sg));
}
// row b reads the encoder (else the null vector): covariates present and not dropped
__device__ __forceinline__ bool cov_kept(const float* c, const unsigned char* keep, int b) { return c && (!keep || keep[b] != 0); }

// LDS: cs[P] the row's covariates, hs[D] the hidden vector.  pre_j = b1_j + sum_i W1[j, i] c_i (fma, i ascending), h_j = silu(pre_j)
__device__ __forceinline__ void cov_hidden(const float* __restrict__ cb, const float* __restrict__ W1, const float* __restrict__ b1,
                                           float* cs, float* hs, float* pres, int P, int D) {
    for (int i = threadIdx.x; i < P; i += kRowBlock) cs[i] = cb[i];
    __syncthreads();
    for (int j = threadIdx.x; j < D; j += kRowBlock) {
        float pre = b1[j];
        const float* w = W1 + (size_t)j * P;
        for (int i = 0; i < P; ++i) pre = fmaf(w[i], cs[i], pre);
        hs[j] = cov_silu(pre);
        if (pres) pres[j] = pre;
    }
    __syncthreads();
}

// out[b, :] (+)= keep_b ? W2 h_b + b2 : null; add: onto the time embedding (the model's use), else written (fd_cov_embed)
__global__ __launch_bounds__(kRowBlock) void k_cov_embed(const float* __restrict__ c, const unsigned char* __restrict__ keep,
                                                           const float* __restrict__ W1, const float* __restrict__ b1,
                                                           const float* __restrict__ W2, const float* __restrict__ b2,
                                                           const float* __restrict__ nul, float* __restrict__ out, int P, int D,
                                                           int add) {
    extern __shared__ float lds[];
    const int b = blockIdx.x;
    float* o = out + (size_t)b * D;
    if (!cov_kept(c, keep, b)) {      // (uniform over the workgroup)
        for (int d = threadIdx.x; d < D; d += kRowBlock) o[d] = add ? o[d] + nul[d] : nul[d];
        return;
    }
    float* cs = lds;
    float* hs = lds + P;
    cov_hidden(c + (size_t)b * P, W1, b1, cs, hs, nullptr, P, D);
    for (int d = threadIdx.x; d < D; d += kRowBlock) {
        float acc = b2[d];
        const float* w = W2 + (size_t)d * D;
        for (int j = 0; j < D; ++j) acc = fmaf(w[j], hs[j], acc);
        o[d] = add ? o[d] + acc : acc;
    }
}

// keep[b] = 0 with probability p: row b is lane b % 4 of Philox counter ctr0 + b / 4, as k_label_dropout (fd_cfg.hip)
__global__ __launch_bounds__(kBlock) void k_cov_keep(unsigned char* __restrict__ keep, int B, float p, uint64_t seed, uint64_t ctr0) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    unsigned char v = 1;
    if (p > 0.f) {
        const fd_u4 r = fd_philox4x32_10(ctr0 + (uint64_t)(b >> 2), seed);
        const int l = b & 3;
        const uint32_t rv = l == 0 ? r.x : l == 1 ? r.y : l == 2 ? r.z : r.w;
        if (fd_u01(rv) < p) v = 0;
    }
    keep[b] = v;
}

// keep[0 .. B) = 1, keep[B .. 2B) = 0: the guided pair
__global__ __launch_bounds__(kBlock) void k_cov_pair_keep(unsigned char* __restrict__ keep, int B) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < 2 * B) keep[i] = i < B ? 1 : 0;
}

// Encoder gradient, kernel 1, one workgroup per kept row: pre_b and h_b recomputed from c_b (the forward's arithmetic),
// dpre_b[j] = (sum_d W2[d, j] dtemb[b, d]) silu'(pre_b[j]) (fma, d ascending); h (B, D) and dpre (B, D) go to the workspace.
// LDS: cs[P], hs[D], pres[D], gs[D] = dtemb[b, :].  Dropped rows write nothing: kernel 2 never reads their rows.
__global__ __launch_bounds__(kRowBlock) void k_cov_bwd_rows(const float* __restrict__ c, const unsigned char* __restrict__ keep,
                                                              const float* __restrict__ W1, const float* __restrict__ b1,
                                                              const float* __restrict__ W2, const float* __restrict__ dtemb,
                                                              float* __restrict__ h, float* __restrict__ dpre, int P, int D) {
    extern __shared__ float lds[];
    const int b = blockIdx.x;
    if (!cov_kept(c, keep, b)) return;
    float* cs = lds;
    float* hs = lds + P;
    float* pres = hs + D;
    float* gs = pres + D;
    for (int d = threadIdx.x; d < D; d += kRowBlock) gs[d] = dtemb[(size_t)b * D + d];
    cov_hidden(c + (size_t)b * P, W1, b1, cs, hs, pres, P, D);
    for (int j = threadIdx.x; j < D; j += kRowBlock) {
        float g = 0.f;
        for (int d = 0; d < D; ++d) g = fmaf(W2[(size_t)d * D + j], gs[d], g);
        h[(size_t)b * D + j] = hs[j];
        dpre[(size_t)b * D + j] = g * cov_dsilu(pres[j]);
    }
}

// Encoder gradient, kernel 2, one thread per output element, each summing over b ascending (no atomics: bit-reproducible and
// independent of the grid):
//   dW2[d, j] = sum_kept dtemb[b, d] h[b, j]     db2[d] = sum_kept dtemb[b, d]     dnull[d] = sum_dropped dtemb[b, d]
//   dW1[j, i] = sum_kept dpre[b, j] c[b, i]      db1[j] = sum_kept dpre[b, j]
struct CovGradOut {
    float *w1, *b1, *w2, *b2, *nul;
};
__global__ __launch_bounds__(kBlock) void k_cov_bwd_reduce(const float* __restrict__ c, const unsigned char* __restrict__ keep,
                                                             const float* __restrict__ dtemb, const float* __restrict__ h,
                                                             const float* __restrict__ dpre, CovGradOut g, int B, int P, int D,
                                                             int accumulate) {
    const int nW2 = D * D, nW1 = D * P;
    const int total = nW2 + nW1 + 3 * D;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    float acc = 0.f;
    float* o;
    if (e < nW2) {
        const int d = e / D, j = e - d * D;
        for (int b = 0; b < B; ++b)
            if (cov_kept(c, keep, b)) acc = fmaf(dtemb[(size_t)b * D + d], h[(size_t)b * D + j], acc);
        o = g.w2 + e;
    } else if (e < nW2 + nW1) {
        const int r = e - nW2, j = r / P, i = r - j * P;
        for (int b = 0; b < B; ++b)
            if (cov_kept(c, keep, b)) acc = fmaf(dpre[(size_t)b * D + j], c[(size_t)b * P + i], acc);
        o = g.w1 + r;
    } else {
        const int r = e - nW2 - nW1, which = r / D, d = r - which * D;      // 0: db2, 1: db1, 2: dnull
        for (int b = 0; b < B; ++b) {
            const bool kept = cov_kept(c, keep, b);
            if (which == 0 && kept) acc += dtemb[(size_t)b * D + d];
            if (which == 1 && kept) acc += dpre[(size_t)b * D + d];
            if (which == 2 && !kept) acc += dtemb[(size_t)b * D + d];
        }
        o = (which == 0 ? g.b2 : which == 1 ? g.b1 : g.nul) + d;
    }
    *o = accumulate ? *o + acc : acc;
}

// k_cov_bwd_rows's LDS use; D <= 1024, P <= 64: at most 12.5 KiB
size_t bwd_rows_lds(int P, int D) { return (size_t)(P + 3 * D) * sizeof(float); }

int cov_backward(fd_ctx* ctx, const float* c, const unsigned char* keep, const float* W1, const float* b1, const float* W2,
                 const float* dtemb, float* ws, CovGradOut g, int B, int P, int D, int accumulate, hipStream_t s) {
    float* h = ws;
    float* dpre = ws + (size_t)B * D;
    if (c) hipLaunchKernelGGL(k_cov_bwd_rows, dim3(B), dim3(kRowBlock), bwd_rows_lds(P, D), s, c, keep, W1, b1, W2, dtemb, h, dpre, P, D);
    const int total = D * D + D * P + 3 * D;
    hipLaunchKernelGGL(k_cov_bwd_reduce, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, s, c, keep, dtemb, (const float*)h,
                       (const float*)dpre, g, B, P, D, accumulate ? 1 : 0);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

bool dims_ok(int B, int P, int D) { return B > 0 && P >= 1 && P <= kMaxCondDim && D >= 1 && D <= 1024; }

int cov_guide_check(fd_score* m, const void* G, const void* timesteps, const void* x, int n_steps, float w, const char* who) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && timesteps && x, "%s: null pointer", who);
    FD_REQUIRE(ctx, n_steps > 0, "%s: n_steps=%d", who, n_steps);
    FD_REQUIRE(ctx, m->cond_dim > 0, "%s: the model has no covariate encoder (fd_score_create_cov with cond_dim > 0)", who);
    FD_REQUIRE(ctx, std::isfinite(w), "%s: the guidance scale is not finite", who);
    return FD_OK;
}

}  // namespace

// ------------------------------------------------------------------ the model's covariates
void fd_cov_embed_launch(const fd_cov& cov, float* temb, int B, int D, hipStream_t s) {
    if (cov.P <= 0) return;
    hipLaunchKernelGGL(k_cov_embed, dim3(B), dim3(kRowBlock), (size_t)(cov.P + D) * sizeof(float), s, cov.c, cov.keep, cov.w1, cov.b1,
                       cov.w2, cov.b2, cov.nul, temb, cov.P, D, 1);
}

int fd_cov_check(fd_score* m, int B, const char* who) {
    if (m->cov && m->cov_B != B)
        return fd_fail(m->ctx, FD_ERR_ARG, "%s: B=%d, but covariates are bound for B=%d (fd_score_set_covariates)", who, B, m->cov_B);
    return FD_OK;
}

int fd_cov_prepare_train(fd_score* m, int B, uint64_t seed, uint64_t offset, hipStream_t s) {
    if (m->cond_dim <= 0) return FD_OK;
    fd_ctx* ctx = m->ctx;
    const int P = m->cond_dim;
    if (m->cov_eff_cap < B) {      // grow-only; the frees synchronise, so no earlier reader is left behind
        if (m->cov_eff) (void)hipFree(m->cov_eff);
        if (m->keep_eff) (void)hipFree(m->keep_eff);
        m->cov_eff = nullptr;
        m->keep_eff = nullptr;
        m->cov_eff_cap = 0;
        const int cap = (B + 1023) & ~1023;
        FD_HIP(ctx, hipMalloc((void**)&m->cov_eff, (size_t)cap * P * sizeof(float)));
        FD_HIP(ctx, hipMalloc((void**)&m->keep_eff, (size_t)cap));
        m->cov_eff_cap = cap;
    }
    m->cov_eff_bound = m->cov != nullptr;
    if (m->cov) FD_HIP(ctx, hipMemcpyAsync(m->cov_eff, m->cov, (size_t)B * P * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_cov_keep, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, s, m->keep_eff, B, m->cov_dropout, seed,
                       offset + kLabelCtrBase);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

int fd_cov_backward(fd_score* m, const float* dtemb, float* grads, int B, int accumulate, hipStream_t s) {
    if (m->cond_dim <= 0) return FD_OK;
    fd_ctx* ctx = m->ctx;
    if (!m->keep_eff || m->cov_eff_cap < B)
        return fd_fail(ctx, FD_ERR_STATE, "covariate-encoder gradient: no training forward has set the covariates");
    const int D = m->d.d_model;
    if (m->cov_bwd_cap < B) {
        if (m->cov_bwd) (void)hipFree(m->cov_bwd);
        m->cov_bwd = nullptr;
        m->cov_bwd_cap = 0;
        const int cap = (B + 1023) & ~1023;
        FD_HIP(ctx, hipMalloc((void**)&m->cov_bwd, (size_t)2 * cap * D * sizeof(float)));
        m->cov_bwd_cap = cap;
    }
    const float* P = m->params;
    const CovGradOut g{grads + m->cov_w1, grads + m->cov_b1, grads + m->cov_w2, grads + m->cov_b2, grads + m->cov_null};
    return cov_backward(ctx, m->cov_eff_bound ? m->cov_eff : nullptr, m->keep_eff, P + m->cov_w1, P + m->cov_b1, P + m->cov_w2, dtemb,
                        m->cov_bwd, g, B, m->cond_dim, D, accumulate, s);
}

void fd_cov_destroy(fd_score* m) {
    if (m->cov_eff) (void)hipFree(m->cov_eff);
    if (m->keep_eff) (void)hipFree(m->keep_eff);
    if (m->cov_bwd) (void)hipFree(m->cov_bwd);
    m->cov_eff = nullptr;
    m->keep_eff = nullptr;
    m->cov_bwd = nullptr;
    m->cov_eff_cap = m->cov_bwd_cap = 0;
}

extern "C" int fd_score_set_covariates(fd_score* m, const float* c, int B) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    if (!c) {
        m->cov = nullptr;
        m->cov_keep = nullptr;
        m->cov_B = 0;
        return FD_OK;
    }
    FD_REQUIRE(ctx, m->cond_dim > 0, "fd_score_set_covariates: the model has no covariate encoder (fd_score_create_cov with cond_dim > 0)");
    FD_REQUIRE(ctx, B > 0, "fd_score_set_covariates: B=%d", B);
    m->cov = c;
    m->cov_keep = nullptr;
    m->cov_B = B;
    return FD_OK;
}

extern "C" int fd_score_get_covariates(fd_score* m, const float** c, int* B) {
    if (!m || !c || !B) return FD_ERR_ARG;
    *c = m->cov;
    *B = m->cov_B;
    return FD_OK;
}

extern "C" int fd_score_set_cov_dropout(fd_score* m, float p) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, p >= 0.f && p <= 1.f, "fd_score_set_cov_dropout: p=%f", p);
    FD_REQUIRE(ctx, m->cond_dim > 0 || p == 0.f, "fd_score_set_cov_dropout: the model has no covariate encoder");
    m->cov_dropout = p;
    return FD_OK;
}

// ------------------------------------------------------------------ the kernels alone, on raw pointers
extern "C" int fd_cov_dropout(fd_ctx* ctx, uint8_t* keep, int B, float p, uint64_t seed, uint64_t offset, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, keep && B > 0, "fd_cov_dropout: null output or B=%d", B);
    FD_REQUIRE(ctx, p >= 0.f && p <= 1.f, "fd_cov_dropout: p=%f", p);
    hipLaunchKernelGGL(k_cov_keep, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, keep, B, p, seed,
                       offset + kLabelCtrBase);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_cov_embed(fd_ctx* ctx, const float* w1, const float* b1, const float* w2, const float* b2, const float* nul,
                            const float* c, const uint8_t* keep, float* e, int B, int P, int D, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, w1 && b1 && w2 && b2 && nul && e, "fd_cov_embed: null pointer");
    FD_REQUIRE(ctx, dims_ok(B, P, D), "fd_cov_embed: B=%d P=%d (1 .. %d) D=%d (1 .. 1024)", B, P, kMaxCondDim, D);
    hipLaunchKernelGGL(k_cov_embed, dim3(B), dim3(kRowBlock), (size_t)(P + D) * sizeof(float), (hipStream_t)stream, c, keep, w1, b1, w2,
                       b2, nul, e, P, D, 0);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_cov_embed_backward(fd_ctx* ctx, const float* w1, const float* b1, const float* w2, const float* c, const uint8_t* keep,
                                     const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, float* dnull, int B, int P,
                                     int D, int accumulate, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, w1 && b1 && w2 && dtemb && dw1 && db1 && dw2 && db2 && dnull, "fd_cov_embed_backward: null pointer");
    FD_REQUIRE(ctx, dims_ok(B, P, D), "fd_cov_embed_backward: B=%d P=%d (1 .. %d) D=%d (1 .. 1024)", B, P, kMaxCondDim, D);
    if (int rc = fd_ws_reserve(ctx, fd_ws::padded((size_t)2 * B * D * sizeof(float)))) return rc;
    return cov_backward(ctx, c, keep, w1, b1, w2, dtemb, (float*)ctx->ws, CovGradOut{dw1, db1, dw2, db2, dnull}, B, P, D, accumulate,
                        (hipStream_t)stream);
}

// ------------------------------------------------------------------ guided loops
fd_guide fd_guide_plan_cov(const float* c, int P, float w) {
    const bool pair = c && ((w != 1.f && w != 0.f) || getenv("FDIFF_CFG_FORCE_PAIR"));
    fd_guide g{pair, nullptr, w, (float)(1.0 - (double)w)};
    g.c = (pair || w != 0.f) ? c : nullptr;
    g.P = P;
    return g;
}

int fd_guide_begin_cov(fd_score* m, const fd_guide* g, void* own, int B, hipStream_t s) {
    fd_ctx* ctx = m->ctx;
    const size_t row_bytes = (size_t)B * g->P * sizeof(float);
    FD_HIP(ctx, hipMemcpyAsync(own, g->c, row_bytes, hipMemcpyDeviceToDevice, s));
    FD_HIP(ctx, hipMemcpyAsync((char*)own + row_bytes, g->c, row_bytes, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_cov_pair_keep, dim3((2 * B + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                       (unsigned char*)own + fd_guide_cov_bytes(g, B), B);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_sampler_run_cov(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                                  float* x, const float* c, float w, const float* z_steps, uint64_t seed, uint64_t offset, int B,
                                  int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_cov")) return rc;
    fd_ctx* ctx = m->ctx;
    if (int rc = cov_guide_check(m, G, timesteps, x, n_steps, w, "fd_sampler_run_cov")) return rc;
    FD_REQUIRE(ctx, dt > 0.f, "fd_sampler_run_cov: step size must be > 0 (sde.py:158)");
    const fd_guide g = fd_guide_plan_cov(c, m->cond_dim, w);
    return fd_sampler_sde_loop(m, sde, G, timesteps, n_steps, dt, x, z_steps, seed, offset, B, mode, (hipStream_t)stream, &g);
}

// solver: 0 Euler, 1 Heun (fd_sampler_run_ode's grids), 2 DDIM, 3 DPM-Solver++ 2M (fd_sampler_run_dpm's)
extern "C" int fd_sampler_run_ode_cov(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                      int solver, float* x, const float* c, float w, int B, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_ode_cov")) return rc;
    fd_ctx* ctx = m->ctx;
    if (int rc = cov_guide_check(m, G, timesteps, x, n_steps, w, "fd_sampler_run_ode_cov")) return rc;
    FD_REQUIRE(ctx, solver >= 0 && solver <= 3, "fd_sampler_run_ode_cov: solver %d (0 Euler, 1 Heun, 2 DDIM, 3 DPM-Solver++ 2M)", solver);
    const fd_guide g = fd_guide_plan_cov(c, m->cond_dim, w);
    return fd_sampler_ode_loop(m, sde, G, timesteps, n_steps, solver, x, B, mode, (hipStream_t)stream, &g);
}
