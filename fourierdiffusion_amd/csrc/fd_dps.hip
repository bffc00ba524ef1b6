// fd_dps.hip -- gradient-guided conditional sampling: diffusion posterior sampling (DPS; Chung et al., ICLR 2023) and TSDiff's
// observation self-guidance (Kollovieh et al., NeurIPS 2023), NOT in the reference.  The state is never overwritten (the hard
// projection of fd_impute.hip is not used); every reverse step is nudged along -grad_x ||y - A(x0_hat(x))||^2 instead, x0_hat being
// Tweedie's denoised estimate.  Per state row b and step t_i -> t_{i+1}, with (alpha, s) the perturbation kernel at t_i (the std of
// frequency k is s G_k), A(x) = idft(sigma x + mu) and idft = F^T diag(1/rho) (F, rho of fd_impute.hip):
//
//   x0_hat = (x + s^2 G^2 . score) / alpha
//   r      = m . idft(sigma . (x0_obs - x0_hat))            = m . (y - A(x0_hat))   (fourier = 0: m . sigma . (x0_obs - x0_hat))
//   u      = sigma . idft^T(r) = sigma . diag(1/rho) F r                            (fourier = 0: sigma . r)
//   dx     = J^T (s^2 G^2 . u)                              (fd_score_input_vjp of the training forward; 0 without the Jacobian)
//   g      = (2 / alpha) (u + dx)                           = -grad_x ||r||^2
//   x'     = fd_sde_apply(x, score, z) + (zeta / ||r||) g   (0 where ||r|| = 0)
//
// The guidance is multiplied by sigma where the projection divides by it, so near-empty spectral bins receive almost nothing.
//
// k_dps_residual<FOURIER, PAIR, Op>: one workgroup per (row, block of 16 channels), on fd_impute.hip's basis and on the LDS images,
// product, block sum and launch of fd_project.h, which k_impute shares.  Phase 1: sigma (x0_obs - x0_hat) / rho into the k-quad LDS
// image U; phase 2: V = F^T U (v_mfma_f32_16x16x4_f32), masked into W = r, and the block's sum r^2 in double; phase 3: Y = F W,
// u = sigma Y / rho, dout = s^2 G^2 u.  The block's sum goes to part[b][block] (no atomics).  Op = WindowOp: the residual of window
// means (fd_aggregate.hip), r over windows, W = r / l, the bases A_w / B_w.  Op = DenseOp: the residual of a dense operator's rows
// (fd_linop.hip), both domains on the two products, phase 3 on the operator's adjoint basis F P^T (P^T in the time domain, rho = 1).
// k_dps_step: elementwise over k_sde_step's Philox groups; a row's ||r||^2 is the sum of its blocks in order, so
// runs are bit-identical.  Every stage buffer lives in ctx->ll_buf, outside the arena that holds the training forward's saved
// activations.
//
// Classifier-free guidance (fd_guide, fd_loop.h; the _cfg entry points): the score above is s = w s_c + (1 - w) s_u, the halves of ONE
// forward on 2B rows with the labels [y ; null], and its Jacobian is J = w J_c + (1 - w) J_u, so
//   dx = J^T v = w J_c^T v + (1 - w) J_u^T v,   v = s^2 G^2 u
// is ONE input VJP on 2B rows whose input is (w v ; (1 - w) v) -- the network treats its rows independently, so the conditional half
// of the VJP's output is J_c^T (w v) and the null half J_u^T ((1 - w) v) -- and the step kernel adds the two halves, conditional
// first.  k_dps_residual<.., PAIR> forms the guided score, writes u for B rows and the VJP input for 2B; k_dps_step<.., PAIR> steps
// with the guided score over the Philox groups of n = B T C and writes both halves of the state.
#include <algorithm>
#include <cmath>

#include "fd_aggregate.h"
#include "fd_common.h"
#include "fd_dps.h"
#include "fd_engine.h"
#include "fd_linop.h"
#include "fd_loop.h"
#include "fd_philox.h"
#include "fd_project.h"
#include "fd_sde.h"

namespace {

using namespace fdproj;

constexpr int kStepBlock = 256;

typedef fd_dps_res ResArgs;      // fd_dps.h
// PAIR: x and score are (2B,T,C), dout too (w v in the conditional half, (1 - w) v in the null half); u and part stay B rows
struct ResArgsPair : ResArgs {
    size_t half;             // B T C: where the null half starts
    float w, omw;            // the guidance scale and 1 - w
};
template <bool PAIR>
struct ResArgsOf { typedef ResArgs type; };
template <>
struct ResArgsOf<true> { typedef ResArgsPair type; };

// the score Tweedie's estimate reads at element e, and the VJP input s^2 G^2 u of element e
template <bool PAIR, class Args>
__device__ __forceinline__ float res_score(const Args& a, size_t e) {
    if constexpr (PAIR) return fd_guided(a.score[e], a.score[a.half + e], a.w, a.omw);
    else return a.score[e];
}
template <bool PAIR, class Args>
__device__ __forceinline__ void res_dout(const Args& a, size_t e, float v) {
    if constexpr (PAIR) {
        a.dout[e] = __fmul_rn(a.w, v);
        a.dout[a.half + e] = __fmul_rn(a.omw, v);
    } else {
        a.dout[e] = v;
    }
}

// Op (fd_project.h): the coordinate mask, or window means (fd_aggregate.hip) or a dense operator (fd_linop.hip), which go with no PAIR
template <bool FOURIER, bool PAIR, class Op>
__global__ __launch_bounds__(kThreads) void k_dps_residual(typename ResArgsOf<PAIR>::type a, Op op) {
    static_assert(!(Op::kWindow && PAIR), "window means go with no guide");
    static_assert(!(Op::kDense && PAIR), "a dense operator goes with no guide");
    constexpr bool PRODUCTS = FOURIER || Op::kDense;    // the two MFMA products: a dense operator in the time domain is the Fourier
                                                        // branch with rho = 1 on the time-domain bases
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.ncb, c0 = (blockIdx.x % a.ncb) * kCB;
    const int T = a.T, C = a.C, Tp = a.Tp, M = op.rows(T), Mp = op.rows_padded(Tp);
    const size_t TC = (size_t)T * C, base = (size_t)b * TC, obase = (size_t)(b / a.obs_rep) * TC;
    const uint8_t* mrow = a.mask + (a.mask_per_series ? (size_t)(b / a.obs_rep) * M * C : 0);
    double rr = 0.0;

    if constexpr (!FOURIER && !Op::kWindow && !Op::kDense) {
        // ---- the mask in the time domain selects elementwise: no LDS image
        for (int i = tid; i < T * kCB; i += kThreads) {
            const int t = i / kCB, c = c0 + i % kCB;
            if (c >= C) continue;
            const size_t tc = (size_t)t * C + c, e = base + tc;
            const float Gt = a.G[t], sg2 = a.s2 * (Gt * Gt);
            const float sd = a.stdv ? a.stdv[tc] : 1.0f;
            const float x0h = (a.x[e] + sg2 * res_score<PAIR>(a, e)) / a.alpha;
            const float r = mrow[tc] ? sd * (a.x0[obase + tc] - x0h) : 0.f;
            rr += (double)r * (double)r;
            const float uv = sd * r;
            a.u[e] = uv;
            if (a.dout) res_dout<PAIR>(a, e, sg2 * uv);
        }
    } else {
        float* U = lds;                            // PRODUCTS: sigma (x0_obs - x0_hat) / rho, packed rows (k-quad); else time rows [t][channel]
        float* W = lds + (size_t)Tp * kCB;         // PRODUCTS: the adjoint's input (r, or r / l), the operator's rows (k-quad)
        if (PRODUCTS) {
            for (int i = tid; i < Tp * kCB; i += kThreads) U[i] = 0.f;
            __syncthreads();
        }
        // ---- phase 1
        for (int i = tid; i < T * kCB; i += kThreads) {
            const int k = i / kCB, cl = i % kCB, c = c0 + cl;
            if (c >= C) continue;
            const size_t kc = (size_t)k * C + c, e = base + kc;
            const float Gk = a.G[k];
            const float sd = a.stdv ? a.stdv[kc] : 1.0f;
            const float x0h = (a.x[e] + a.s2 * (Gk * Gk) * res_score<PAIR>(a, e)) / a.alpha;
            const float dv = sd * (a.x0[obase + kc] - x0h);
            if (FOURIER) U[quad_idx(k, cl)] = dv * inv_r(k, T);
            else if (Op::kDense) U[quad_idx(k, cl)] = dv;
            else U[i] = dv;
        }
        __syncthreads();

        if constexpr (!PRODUCTS) {
            // ---- window means in the time domain: one thread per (window, channel), r = the masked mean in ascending t;
            // u = sigma r / l over the window
            for (int i = tid; i < M * kCB; i += kThreads) {
                const int j = i / kCB, cl = i % kCB, c = c0 + cl;
                if (c >= C) continue;
                const int t0 = j * op.window, l = win_len(j, op.window, T);
                float r = 0.f;
                if (mrow[(size_t)j * C + c]) {
                    float sum = 0.f;
                    for (int k = 0; k < l; ++k) sum += U[(t0 + k) * kCB + cl];
                    r = sum / (float)l;
                }
                rr += (double)r * (double)r;
                const float rl = r / (float)l;
                for (int k = 0; k < l; ++k) {
                    const int t = t0 + k;
                    const size_t tc = (size_t)t * C + c, e = base + tc;
                    const float sd = a.stdv ? a.stdv[tc] : 1.0f;
                    const float uv = sd * rl;
                    a.u[e] = uv;
                    if (a.dout) {
                        const float Gt = a.G[t];
                        res_dout<PAIR>(a, e, a.s2 * (Gt * Gt) * uv);
                    }
                }
            }
        } else {
            const int lane = tid & 63, wave = tid >> 6, nw = kThreads / 64;
            const int li = lane & 15, kq = lane >> 4;
            const int c = c0 + li;
            const float* Ao = op.to_obs(a.basis, Tp);
            const float* Bo = op.adjoint_basis(a.basis, Tp);
            // ---- phase 2: r = m . (Ao U) (row i of the tile = observation row j0 + i: a time step or a window), its squares in
            // double; W = the adjoint's input
            for (int tile = wave; tile < Mp / 16; tile += nw) {
                const int j0 = tile * 16;
                const f32x4 acc = tile_product(Ao, j0, Tp, U, li, kq);
                f32x4 w;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int j = j0 + 4 * kq + v;
                    const bool keep = j < M && c < C && mrow[(size_t)j * C + c];
                    const float rv = keep ? acc[v] : 0.f;
                    rr += (double)rv * (double)rv;
                    w[v] = keep ? op.adjoint(rv, j, T) : 0.f;
                }
                *reinterpret_cast<f32x4*>(W + ((j0 / 4 + kq) * kCB + li) * 4) = w;
            }
            __syncthreads();
            // ---- phase 3: Y = Bo W (row i of the tile = packed row r0 + i); u = sigma Y / rho, dout = s^2 G^2 u
            for (int tile = wave; tile < Tp / 16; tile += nw) {
                const int r0 = tile * 16;
                const f32x4 acc = tile_product(Bo, r0, Mp, W, li, kq);
                if (c >= C) continue;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int k = r0 + 4 * kq + v;
                    if (k >= T) continue;
                    const size_t kc = (size_t)k * C + c, e = base + kc;
                    const float sd = a.stdv ? a.stdv[kc] : 1.0f;
                    const float uv = FOURIER ? sd * inv_r(k, T) * acc[v] : sd * acc[v];
                    a.u[e] = uv;
                    if (a.dout) {
                        const float Gk = a.G[k];
                        res_dout<PAIR>(a, e, a.s2 * (Gk * Gk) * uv);
                    }
                }
            }
        }
    }
    block_sum(rr, a.part + blockIdx.x);
}

struct StepArgs {
    const float* G;
    float* x;                // (B,T,C) state, updated in place (STEP)
    const float* score;
    const float* zin;        // injected predictor noise or nullptr (Philox at offset)
    const float* u;
    const float* dx;         // J^T dout or nullptr
    const double* part;      // (B, ncb)
    float* gout;             // GRAD: g (B,T,C)
    double* rn2_out;         // GRAD: ||r||^2 per row
    size_t n, TC;
    int T, C, ncb;
    SdeCoef cf;
    float alpha;
    double zeta;
    uint64_t seed, offset;
};
// PAIR: x, score and dx are (2B,T,C), n = B T C the size of one half; u, part, gout and rn2_out stay B rows
struct StepArgsPair : StepArgs {
    float w, omw;
};
template <bool PAIR>
struct StepArgsOf { typedef StepArgs type; };
template <>
struct StepArgsOf<true> { typedef StepArgsPair type; };

// STEP: x' = fd_sde_apply(x, score, z) + (zeta / ||r||) g over the Philox groups of k_sde_step (group q = elements 4q .. 4q+3 of the
// whole (B,T,C) tensor, drawn at offset + q).  GRAD: g and ||r||^2 alone.  PAIR: the guided score, dx = the conditional half of the
// VJP plus the null half, and the new state to both halves; groups and counters those of the unpaired launch over n = B T C.
template <bool GRAD, bool PAIR = false>
__global__ __launch_bounds__(kStepBlock) void k_dps_step(typename StepArgsOf<PAIR>::type a) {
    const size_t ngroups = (a.n + 3) / 4;
    for (size_t q = blockIdx.x * (size_t)kStepBlock + threadIdx.x; q < ngroups; q += (size_t)gridDim.x * kStepBlock) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (!GRAD) {
            if (a.zin) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (q * 4 + j < a.n) z[j] = a.zin[q * 4 + j];
            } else {
                fd_randn4(a.offset + q, a.seed, z);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t e = q * 4 + j;
            if (e >= a.n) break;
            const size_t b = e / a.TC, loc = e - b * a.TC;
            double rn2 = 0.0;
            for (int k = 0; k < a.ncb; ++k) rn2 += a.part[b * a.ncb + k];
            float dxe = a.dx ? a.dx[e] : 0.f;
            if constexpr (PAIR)
                if (a.dx) dxe = __fadd_rn(dxe, a.dx[a.n + e]);
            const float gv = (2.0f / a.alpha) * (a.u[e] + dxe);
            if (GRAD) {
                a.gout[e] = gv;
                if (loc == 0) a.rn2_out[b] = rn2;
            } else {
                const int t = (int)(loc / a.C);
                float sc = a.score[e];
                if constexpr (PAIR) sc = fd_guided(sc, a.score[a.n + e], a.w, a.omw);
                float xv = fd_sde_apply(a.x[e], sc, z[j], a.G[t], a.cf);
                const float coef = rn2 > 0.0 ? (float)(a.zeta / sqrt(rn2)) : 0.f;
                if (coef != 0.f) xv += coef * gv;
                a.x[e] = xv;
                if constexpr (PAIR) a.x[a.n + e] = xv;
            }
        }
    }
}

typedef fd_dps_bufs DpsBufs;     // fd_dps.h

}  // namespace

int fd_dps_buffers(fd_ctx* ctx, int B, int R, size_t n, int ncb, bool jac, bool xpair, fd_dps_bufs* o) {
    return fd_ll_carve(ctx, [&](auto take) { fd_dps_take(take, B, R, n, ncb, jac, xpair, o); });
}

// checks and fills the conditioning / geometry fields shared by both entries
int fd_dps_prepare(fd_score* m, fd_dps_res& r, const float* G, const float* x, const float* x0, const uint8_t* mask,
                   int mask_per_series, const float* stdv, int fourier, int B, int obs_replicas, hipStream_t s, const char* who) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && x && x0 && mask, "%s: null pointer", who);
    FD_REQUIRE(ctx, obs_replicas > 0 && B % obs_replicas == 0, "%s: B=%d is not a multiple of obs_replicas=%d", who, B, obs_replicas);
    const int T = m->d.max_len, C = m->d.n_channels;
    FD_REQUIRE(ctx, !fourier || T <= 1024, "%s: max_len %d > 1024 (the LDS images of one series)", who, T);
    r.T = T; r.C = C;
    r.Tp = (T + 15) / 16 * 16;
    r.ncb = (C + kCB - 1) / kCB;
    FD_REQUIRE(ctx, (long long)B * r.ncb < (1ll << 31), "%s: B=%d too large for one launch", who, B);
    r.x0 = x0; r.mask = mask; r.mask_per_series = mask_per_series ? 1 : 0;
    r.obs_rep = obs_replicas;
    r.stdv = stdv;
    r.G = G;
    r.basis = nullptr;
    if (fourier) {
        r.basis = fd_impute_basis(ctx, T, r.Tp, s);
        if (!r.basis) return fd_fail(ctx, FD_ERR_HIP, "%s: could not build the transform basis of T=%d", who, T);
    }
    return FD_OK;
}

namespace {

template <bool FOURIER, bool PAIR, class Op = MaskOp>
int launch_residual(fd_ctx* ctx, const typename ResArgsOf<PAIR>::type& r, int B, hipStream_t s, Op op = Op()) {
    return launch_kernel<k_dps_residual<FOURIER, PAIR, Op>, 128 * 1024>(ctx, (unsigned)(B * r.ncb), image_bytes(op, r.T, r.Tp, FOURIER),
                                                                         s, r, op);
}

// the step (or, GRAD, the gradient) over the B rows of a.n; g: a paired guide, or null
template <bool GRAD>
int launch_step(fd_ctx* ctx, const StepArgs& a, const fd_guide* g, hipStream_t s) {
    const size_t ngroups = (a.n + 3) / 4;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((ngroups + kStepBlock - 1) / kStepBlock,
                                                                         (size_t)ctx->num_cu * 16));
    if (g) {
        StepArgsPair ap{};
        static_cast<StepArgs&>(ap) = a;
        ap.w = g->w;
        ap.omw = g->omw;
        hipLaunchKernelGGL((k_dps_step<GRAD, true>), dim3(grid), dim3(kStepBlock), 0, s, ap);
    } else {
        hipLaunchKernelGGL((k_dps_step<GRAD, false>), dim3(grid), dim3(kStepBlock), 0, s, a);
    }
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

}  // namespace

// One guidance evaluation at (x, tvec) on R network rows (B, or 2B under a paired guide g): the score (training forward with the
// Jacobian, else the sampler's forward), the residual of the B state rows, and the VJP; leaves score, u, dx and the block sums in
// the buffers
int fd_dps_eval(fd_score* m, fd_dps_res& r, const fd_dps_bufs& bf, const float* x, int B, int R, const fd_guide* g, bool jac,
                bool fourier, int mode, hipStream_t s, const fd_agg_plan* ag, const fdproj::DenseOp* dn) {
    fd_ctx* ctx = m->ctx;
    if (jac) {
        if (int rc = fd_score_forward_train(m, x, bf.tvec, bf.score, R, 0.f, 0, 0, s)) return rc;
    } else {
        if (int rc = fd_score_forward_any(m, x, bf.tvec, bf.score, R, mode, s)) return rc;
    }
    r.x = x;
    r.score = bf.score;
    if (ag) {        // window means (fd_aggregate.h): r.mask is (B/obs_rep,J,C) or (J,C)
        r.basis = ag->basis;
        if (int rc = fourier ? launch_residual<true, false>(ctx, r, B, s, ag->op) : launch_residual<false, false>(ctx, r, B, s, ag->op))
            return rc;
    } else if (dn) {        // a dense operator (fd_linop.h): r.mask is (B/obs_rep,M,C) or (M,C)
        if (int rc = fourier ? launch_residual<true, false>(ctx, r, B, s, *dn) : launch_residual<false, false>(ctx, r, B, s, *dn))
            return rc;
    } else if (g) {
        ResArgsPair rp{};
        static_cast<ResArgs&>(rp) = r;
        rp.half = (size_t)B * r.T * r.C;
        rp.w = g->w;
        rp.omw = g->omw;
        if (int rc = fourier ? launch_residual<true, true>(ctx, rp, B, s) : launch_residual<false, true>(ctx, rp, B, s)) return rc;
    } else {
        if (int rc = fourier ? launch_residual<true, false>(ctx, r, B, s) : launch_residual<false, false>(ctx, r, B, s)) return rc;
    }
    if (jac)
        if (int rc = fd_score_input_vjp(m, bf.dout, bf.dx, s)) return rc;
    return FD_OK;
}

// the residual of the B state rows alone, from the x and score r points at (no network evaluation)
int fd_dps_residual(fd_ctx* ctx, const fd_dps_res& r, int B, bool fourier, hipStream_t s) {
    return fourier ? launch_residual<true, false>(ctx, r, B, s) : launch_residual<false, false>(ctx, r, B, s);
}

namespace {

// the body of fd_impute_guidance (g == null) and fd_impute_guidance_cfg, the arguments checked under the name `who`
int dps_guidance(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x, const float* x0_obs,
                 const uint8_t* mask_u8, int mask_per_series, const float* feat_std, int fourier, int jacobian, float* g_out,
                 double* rnorm2_out, int B, int obs_replicas, int mode, hipStream_t s, const fd_guide* g, const char* who,
                 int window = 1, fd_linop* lop = nullptr) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, g_out && rnorm2_out, "%s: null pointer", who);
    FD_REQUIRE(ctx, std::isfinite(t) && t > 0.f, "%s: t=%g must be finite and > 0", who, (double)t);
    ResArgs r{};
    if (int rc = fd_dps_prepare(m, r, G, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, B, obs_replicas, s, who)) return rc;
    fd_agg_plan agg{};
    if (window > 1) {
        FD_REQUIRE(ctx, !g, "%s: window=%d goes with no guide", who, window);
        if (int rc = fd_agg_prepare(ctx, r.T, r.Tp, window, fourier, s, &agg, who)) return rc;
    }
    DenseOp dop{};
    if (lop) {
        FD_REQUIRE(ctx, !g && window == 1, "%s: an operator goes with no guide and no window", who);
        if (int rc = fd_linop_prepare(ctx, lop, r.T, fourier, s, &dop, who)) return rc;
    }
    const bool jac = jacobian != 0, pair = g && g->pair;
    const size_t n = (size_t)B * r.T * r.C;
    const int R = fd_guide_rows(g, B);
    DpsBufs bf;
    if (int rc = fd_dps_buffers(ctx, B, R, n, r.ncb, jac, pair, &bf)) return rc;
    double al = 1.0, sd = 0.0;
    fd_marginal_coef(*sde, (double)t, &al, &sd);
    r.alpha = (float)al;
    r.s2 = (float)(sd * sd);
    r.u = bf.u; r.dout = bf.dout; r.part = bf.part;
    if (pair) {      // the state twice, behind the caller's x
        FD_HIP(ctx, hipMemcpyAsync(bf.xpair, x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (int rc = fd_guide_begin(m, g, bf.lab, bf.xpair, B, s)) return rc;
        x = bf.xpair;
    }
    fd_guide_scope scope(m, g, bf.lab, R);
    fd_train_mode_scope tm(m, jac ? fd_diff_train_mode(m, mode) : m->train_mode);
    fd_label_dropout_scope ld(m, 0.f);
    fd_fill(bf.tvec, R, t, s);
    if (int rc = fd_dps_eval(m, r, bf, x, B, R, pair ? g : nullptr, jac, fourier != 0, mode, s, window > 1 ? &agg : nullptr,
                             lop ? &dop : nullptr))
        return rc;
    StepArgs a{};
    a.G = G; a.u = bf.u; a.dx = bf.dx; a.part = bf.part; a.gout = g_out; a.rn2_out = rnorm2_out;
    a.n = n; a.TC = (size_t)r.T * r.C; a.T = r.T; a.C = r.C; a.ncb = r.ncb;
    a.alpha = r.alpha;
    return launch_step<true>(ctx, a, pair ? g : nullptr, s);
}

// the body of fd_sampler_run_impute_dps (g == null) and fd_sampler_run_impute_dps_cfg; a paired guide runs on x (2B,T,C)
int dps_loop(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt, float* x,
             const float* x0_obs, const uint8_t* mask_u8, int mask_per_series, const float* feat_std, int fourier,
             float guidance_scale, int jacobian, const float* z_steps, uint64_t seed, uint64_t offset, int B, int obs_replicas, int mode,
             hipStream_t s, const fd_guide* g, const char* who, int window = 1, fd_linop* lop = nullptr) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, timesteps, "%s: null pointer", who);
    FD_REQUIRE(ctx, n_steps > 0, "%s: n_steps=%d", who, n_steps);
    FD_REQUIRE(ctx, dt > 0.f, "%s: step size must be > 0 (sde.py:158)", who);
    FD_REQUIRE(ctx, std::isfinite(guidance_scale) && guidance_scale >= 0.f, "%s: guidance_scale=%g must be finite and >= 0", who,
               (double)guidance_scale);
    ResArgs r{};
    if (int rc = fd_dps_prepare(m, r, G, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, B, obs_replicas, s, who)) return rc;
    fd_agg_plan agg{};
    if (window > 1) {
        FD_REQUIRE(ctx, !g, "%s: window=%d goes with no guide", who, window);
        if (int rc = fd_agg_prepare(ctx, r.T, r.Tp, window, fourier, s, &agg, who)) return rc;
    }
    DenseOp dop{};
    if (lop) {
        FD_REQUIRE(ctx, !g && window == 1, "%s: an operator goes with no guide and no window", who);
        if (int rc = fd_linop_prepare(ctx, lop, r.T, fourier, s, &dop, who)) return rc;
    }
    const bool jac = jacobian != 0, pair = g && g->pair;
    const size_t n = (size_t)B * r.T * r.C;
    const int R = fd_guide_rows(g, B);
    DpsBufs bf;
    if (int rc = fd_dps_buffers(ctx, B, R, n, r.ncb, jac, false, &bf)) return rc;
    r.u = bf.u; r.dout = bf.dout; r.part = bf.part;
    // per-step coefficients on the host up front: the SDE step's (fd_sde_coef, as fd_sampler_run) and Tweedie's (alpha, s) at t_i
    std::vector<SdeCoef> cf(n_steps);
    std::vector<float> al(n_steps), s2(n_steps);
    for (int i = 0; i < n_steps; ++i) {
        cf[i] = fd_sde_coef(*sde, (double)timesteps[i], dt);
        double aa = 1.0, ss = 0.0;
        fd_marginal_coef(*sde, (double)timesteps[i], &aa, &ss);
        al[i] = (float)aa;
        s2[i] = (float)(ss * ss);
    }
    if (int rc = fd_guide_begin(m, g, bf.lab, x, B, s)) return rc;
    fd_guide_scope scope(m, g, bf.lab, R);
    fd_train_mode_scope tm(m, jac ? fd_diff_train_mode(m, mode) : m->train_mode);
    fd_label_dropout_scope ld(m, 0.f);
    StepArgs a{};
    a.G = G; a.x = x; a.score = bf.score; a.u = bf.u; a.dx = bf.dx; a.part = bf.part;
    a.n = n; a.TC = (size_t)r.T * r.C; a.T = r.T; a.C = r.C; a.ncb = r.ncb;
    a.zeta = (double)guidance_scale;
    a.seed = seed;
    // Philox: predictor noise of step i at offset + i*ceil(BTC/4) (as fd_sampler_run)
    const uint64_t per_step = (uint64_t)((n + 3) / 4);
    for (int i = 0; i < n_steps; ++i) {
        fd_fill(bf.tvec, R, timesteps[i], s);
        r.alpha = al[i];
        r.s2 = s2[i];
        if (int rc = fd_dps_eval(m, r, bf, x, B, R, pair ? g : nullptr, jac, fourier != 0, mode, s, window > 1 ? &agg : nullptr,
                             lop ? &dop : nullptr))
            return rc;
        a.zin = z_steps ? z_steps + (size_t)i * n : nullptr;
        a.cf = cf[i];
        a.alpha = al[i];
        a.offset = offset + (uint64_t)i * per_step;
        if (int rc = launch_step<false>(ctx, a, pair ? g : nullptr, s)) return rc;
    }
    return FD_OK;
}

}  // namespace

extern "C" int fd_impute_guidance(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x, const float* x0_obs,
                                  const uint8_t* mask_u8, int mask_per_series, const float* feat_std, int fourier, int jacobian,
                                  float* g_out, double* rnorm2_out, int B, int obs_replicas, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_impute_guidance")) return rc;
    return dps_guidance(m, sde, G, t, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, jacobian, g_out, rnorm2_out, B,
                        obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_impute_guidance");
}

// fd_impute_guidance and fd_sampler_run_impute_dps on window means: mask_u8 (B/obs_replicas,J,C) or (J,C), J = ceil(T / window), the
// residual r (J,C) per row; window = 1 is the call without it
extern "C" int fd_impute_guidance_agg(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x,
                                      const float* x0_obs, const uint8_t* mask_u8, int mask_per_series, const float* feat_std,
                                      int fourier, int jacobian, float* g_out, double* rnorm2_out, int B, int obs_replicas, int window,
                                      int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_impute_guidance_agg")) return rc;
    FD_REQUIRE(m->ctx, window >= 1 && window <= m->d.max_len, "fd_impute_guidance_agg: window=%d must lie in [1, max_len=%d]", window,
               m->d.max_len);
    if (window == 1)
        return fd_impute_guidance(m, sde, G, t, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, jacobian, g_out, rnorm2_out, B,
                                  obs_replicas, mode, stream);
    return dps_guidance(m, sde, G, t, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, jacobian, g_out, rnorm2_out, B,
                        obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_impute_guidance_agg", window);
}

extern "C" int fd_sampler_run_impute_dps_agg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                                             int n_steps, float dt, float* x, const float* x0_obs, const uint8_t* mask_u8,
                                             int mask_per_series, const float* feat_std, int fourier, float guidance_scale,
                                             int jacobian, const float* z_steps, uint64_t seed, uint64_t offset, int B,
                                             int obs_replicas, int window, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_impute_dps_agg")) return rc;
    FD_REQUIRE(m->ctx, window >= 1 && window <= m->d.max_len, "fd_sampler_run_impute_dps_agg: window=%d must lie in [1, max_len=%d]",
               window, m->d.max_len);
    if (window == 1)
        return fd_sampler_run_impute_dps(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier,
                                         guidance_scale, jacobian, z_steps, seed, offset, B, obs_replicas, mode, stream);
    return dps_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, guidance_scale, jacobian,
                    z_steps, seed, offset, B, obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_sampler_run_impute_dps_agg", window);
}

// fd_impute_guidance and fd_sampler_run_impute_dps on a dense operator: mask_u8 (B/obs_replicas,M,C) or (M,C) over the M rows of
// `op`, the residual r (M,C) per row
extern "C" int fd_impute_guidance_op(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x,
                                     const float* x0_obs, const uint8_t* mask_u8, int mask_per_series, const float* feat_std,
                                     int fourier, int jacobian, float* g_out, double* rnorm2_out, int B, int obs_replicas, fd_linop* op,
                                     int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_impute_guidance_op")) return rc;
    FD_REQUIRE(m->ctx, op, "fd_impute_guidance_op: null operator handle");
    return dps_guidance(m, sde, G, t, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, jacobian, g_out, rnorm2_out, B,
                        obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_impute_guidance_op", 1, op);
}

extern "C" int fd_sampler_run_impute_dps_op(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                                            int n_steps, float dt, float* x, const float* x0_obs, const uint8_t* mask_u8,
                                            int mask_per_series, const float* feat_std, int fourier, float guidance_scale,
                                            int jacobian, const float* z_steps, uint64_t seed, uint64_t offset, int B,
                                            int obs_replicas, fd_linop* op, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_impute_dps_op")) return rc;
    FD_REQUIRE(m->ctx, op, "fd_sampler_run_impute_dps_op: null operator handle");
    return dps_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, guidance_scale, jacobian,
                    z_steps, seed, offset, B, obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_sampler_run_impute_dps_op", 1, op);
}

// fd_impute_guidance on a class-conditional model under classifier-free guidance: y (B) one label per row or null, w the scale;
// g_out and rnorm2_out for the B rows.  A paired call copies x twice into its own buffers.
extern "C" int fd_impute_guidance_cfg(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x,
                                      const float* x0_obs, const uint8_t* mask_u8, int mask_per_series, const float* feat_std,
                                      int fourier, int jacobian, float* g_out, double* rnorm2_out, int B, int obs_replicas, int mode,
                                      const int32_t* y, float cfg_scale, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_impute_guidance_cfg")) return rc;
    if (int rc = fd_guide_check(m, cfg_scale, "fd_impute_guidance_cfg")) return rc;
    const fd_guide g = fd_guide_plan(y, cfg_scale);
    return dps_guidance(m, sde, G, t, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, jacobian, g_out, rnorm2_out, B,
                        obs_replicas, mode, (hipStream_t)stream, &g, "fd_impute_guidance_cfg");
}

extern "C" int fd_sampler_run_impute_dps(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                         float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                         const float* feat_std, int fourier, float guidance_scale, int jacobian, const float* z_steps,
                                         uint64_t seed, uint64_t offset, int B, int obs_replicas, int mode, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_impute_dps")) return rc;
    return dps_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, guidance_scale, jacobian,
                    z_steps, seed, offset, B, obs_replicas, mode, (hipStream_t)stream, nullptr, "fd_sampler_run_impute_dps");
}

// fd_sampler_run_impute_dps under classifier-free guidance: y (B) one label per state row or null, w the scale.  A paired call
// (labels and w outside {0, 1}, or FDIFF_CFG_FORCE_PAIR) takes x (2B,T,C) with the state in its first half and leaves both halves
// equal; else one evaluation per step on B rows with y bound.
extern "C" int fd_sampler_run_impute_dps_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                                             int n_steps, float dt, float* x, const float* x0_obs, const uint8_t* mask_u8,
                                             int mask_per_series, const float* feat_std, int fourier, float guidance_scale,
                                             int jacobian, const float* z_steps, uint64_t seed, uint64_t offset, int B,
                                             int obs_replicas, int mode, const int32_t* y, float cfg_scale, void* stream) {
    if (int rc = fd_loop_check(m, sde, B, mode, "fd_sampler_run_impute_dps_cfg")) return rc;
    if (int rc = fd_guide_check(m, cfg_scale, "fd_sampler_run_impute_dps_cfg")) return rc;
    const fd_guide g = fd_guide_plan(y, cfg_scale);
    return dps_loop(m, sde, G, timesteps, n_steps, dt, x, x0_obs, mask_u8, mask_per_series, feat_std, fourier, guidance_scale, jacobian,
                    z_steps, seed, offset, B, obs_replicas, mode, (hipStream_t)stream, &g, "fd_sampler_run_impute_dps_cfg");
}
