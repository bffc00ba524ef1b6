// fd_mega_params.h -- parameter block of the persistent series-resident kernel (fd_mega_kernel.h).  Plain data and the one-line
// probability-flow velocity shared by every ODE epilogue: this header is also handed to hiprtc (fd_mega_rtc.hip), which has no host
// headers.
#pragma once
#ifndef __HIPCC_RTC__
#include <cstddef>
#endif

#ifndef FD_W1_SWAP34
#define FD_W1_SWAP34 1      // pair-form W1 image rows stored with index bits 3 <-> 4 swapped (LDS bank slots; 0 = natural order, A/B builds)
#endif
// Pair-form FFN (off_ffn32 image, ffn_loop32): the relu rides in the conversion.  v_cvt_pk_bf16_f32 is VOP3 and its clamp bit clamps
// the result to [0, 1] (scripts/ubench/cvt_clamp_probe.hip, profiles/cvt_clamp_probe.txt: every non-NaN input, both halves), so with
// W1 | b1 stored as 2^-k w the hidden value h 2^-k lies in (0, 1] whenever h > 0 and the clamped conversion IS relu + pack; W2 stored
// as 2^k w undoes the scale inside the second product.  Powers of two commute with bf16 rounding and fp32 accumulation: same bits.
// k = 40: a hidden pre-activation saturates only at 2^40 (LayerNorm'd inputs of O(1) against weights of O(1) stay below 2^10), and
// every scaled weight stays a normal bf16 for 2^-86 <= |W1|, |b1| and |W2| < 2^87 -- checked when the image is built; a model that
// fails gets no pair-form image and runs the 16x16x32 loop.  0 = the relu as v_pk_max_i16 on an unscaled image (A/B builds).
// Both macros change the image: fd_bf16_image_layout_defines() carries them to the run-time compilation and its cache key.
#ifndef FD_RELU_CLAMP
#define FD_RELU_CLAMP 1
#endif
#ifndef FD_RELU_CLAMP_SHIFT
#define FD_RELU_CLAMP_SHIFT 40
#endif
#define FD_MEGA_FORWARD 0  // one score-network forward: x, tvec -> score_out
#define FD_MEGA_SAMPLE 1    // nsteps x {forward, reverse-SDE step}, x updated in place
#define FD_MEGA_ODE 2       // nsteps x {forward, probability-flow ODE stage}: nsteps counts score evaluations, x updated in place

struct fd_sde_step_coef {
    float a_x, g, dt, sqrt_dt, t;   // SdeCoef of fd_sde.h + the timestep itself (time embedding)
};

// Probability-flow ODE (Song et al. 2021, Sec. 4.3): one row per score evaluation.  Stages: FD_ODE_EULER x' = x + h v;
// FD_ODE_HEUN_PREDICT x0 = x, v0 = v, x' = x + h v;  FD_ODE_HEUN_CORRECT x' = x0 + h/2 (v0 + v)  (x0, v0: (B,T,C) workspace,
// the same element owned by the same lane in both stages).  t sits where fd_sde_step_coef keeps it, so the time-embedding
// table builder (k_temb_table) reads either row type.
#define FD_ODE_EULER 0
#define FD_ODE_HEUN_PREDICT 1
#define FD_ODE_HEUN_CORRECT 2
struct fd_ode_step_coef {
    float a_x, g;   // SdeCoef of fd_sde.h at this evaluation's t
    float h;        // t_{i+1} - t_i of the step the evaluation belongs to (< 0 sampling, > 0 encoding)
    int stage;      // FD_ODE_*
    float t;        // time of the evaluation (time embedding)
};
static_assert(sizeof(fd_ode_step_coef) == sizeof(fd_sde_step_coef) &&
                  __builtin_offsetof(fd_ode_step_coef, t) == __builtin_offsetof(fd_sde_step_coef, t),
              "fd_ode_step_coef must keep t where fd_sde_step_coef has it");

// velocity of the probability-flow ODE: v = -a x - 0.5 (g G_k)^2 s  (fd_sde_apply's drift with the score term halved)
__device__ __forceinline__ float fd_ode_velocity(float x, float s, float a_x, float gk) {
    return -a_x * x - (0.5f * (gk * gk)) * s;
}
// one ODE stage on one element (x: state, s: score, gk = g G_k); x0 / v0 point at the element's Heun state
__device__ __forceinline__ float fd_ode_stage1(float x, float s, float gk, const fd_ode_step_coef& c, float* x0, float* v0) {
    const float v = fd_ode_velocity(x, s, c.a_x, gk);
    if (c.stage == FD_ODE_HEUN_CORRECT) return *x0 + (0.5f * c.h) * (*v0 + v);
    if (c.stage == FD_ODE_HEUN_PREDICT) { *x0 = x; *v0 = v; }
    return x + c.h * v;
}
// the same on four consecutive elements of one row (16-byte aligned: C % 4 == 0)
__device__ __forceinline__ float4 fd_ode_stage4(float4 x, float s0, float s1, float s2, float s3, float gk, const fd_ode_step_coef& c,
                                                float* x0, float* v0) {
    const float4 v = {fd_ode_velocity(x.x, s0, c.a_x, gk), fd_ode_velocity(x.y, s1, c.a_x, gk), fd_ode_velocity(x.z, s2, c.a_x, gk),
                      fd_ode_velocity(x.w, s3, c.a_x, gk)};
    if (c.stage == FD_ODE_HEUN_CORRECT) {
        const float4 a = *reinterpret_cast<const float4*>(x0), b = *reinterpret_cast<const float4*>(v0);
        const float hh = 0.5f * c.h;
        return float4{a.x + hh * (b.x + v.x), a.y + hh * (b.y + v.y), a.z + hh * (b.z + v.z), a.w + hh * (b.w + v.w)};
    }
    if (c.stage == FD_ODE_HEUN_PREDICT) {
        *reinterpret_cast<float4*>(x0) = x;
        *reinterpret_cast<float4*>(v0) = v;
    }
    return float4{x.x + c.h * v.x, x.y + c.h * v.y, x.z + c.h * v.z, x.w + c.h * v.w};
}

// Data-prediction exponential integrator (DPM-Solver++, Lu et al. 2022; its first order is deterministic DDIM) on the same rows, one
// score evaluation per step.  With (alpha, s) the perturbation kernel and lambda = log(alpha / s), h = lambda' - lambda > 0:
//   D  = (x + (s G_k)^2 score) / alpha                       Tweedie's estimate of x_0
//   x' = (s'/s) x + cD ((1 + w) D - w D_prev),   cD = -alpha' expm1(-h),  w = h / (2 h_prev)  (0: first order / first step)
// The row's fields are reused: a_x = 1 / alpha, g = s (so that gk = s G_k), h = s'/s.  The two weights of D and D_prev do not fit
// the row (its size is pinned to fd_sde_step_coef) and travel in a parallel array, fd_dpm_coef per evaluation.  D_prev is one
// (B,T,C) buffer (the Heun x0 buffer), the same element owned by the same lane in every evaluation.
//   FD_ODE_DDIM      x' = h x + c1 D                         (no state)
//   FD_ODE_DPM_FIRST the same, D stored
//   FD_ODE_DPM_2M    x' = h x + c1 D + c0 D_prev, D stored
#define FD_ODE_DDIM 3
#define FD_ODE_DPM_FIRST 4
#define FD_ODE_DPM_2M 5
struct fd_dpm_coef {
    float c1, c0;   // cD (1 + w), -cD w
};
__device__ __forceinline__ float fd_dpm_stage1(float x, float s, float gk, const fd_ode_step_coef& c, const fd_dpm_coef& w, float* dprev) {
    const float d = (x + (gk * gk) * s) * c.a_x;
    float o = c.h * x + w.c1 * d;
    if (c.stage == FD_ODE_DPM_2M) o += w.c0 * *dprev;
    if (c.stage != FD_ODE_DDIM) *dprev = d;
    return o;
}
__device__ __forceinline__ float4 fd_dpm_stage4(float4 x, float s0, float s1, float s2, float s3, float gk, const fd_ode_step_coef& c,
                                                const fd_dpm_coef& w, float* dprev) {
    const float g2 = gk * gk;
    const float4 d = {(x.x + g2 * s0) * c.a_x, (x.y + g2 * s1) * c.a_x, (x.z + g2 * s2) * c.a_x, (x.w + g2 * s3) * c.a_x};
    float4 o = {c.h * x.x + w.c1 * d.x, c.h * x.y + w.c1 * d.y, c.h * x.z + w.c1 * d.z, c.h * x.w + w.c1 * d.w};
    if (c.stage == FD_ODE_DPM_2M) {
        const float4 p = *reinterpret_cast<const float4*>(dprev);
        o.x += w.c0 * p.x; o.y += w.c0 * p.y; o.z += w.c0 * p.z; o.w += w.c0 * p.w;
    }
    if (c.stage != FD_ODE_DDIM) *reinterpret_cast<float4*>(dprev) = d;
    return o;
}

struct fd_mega_params {
    // shapes
    int B, T, KT /* ceil(T/16) */, C, D, H, hd, L, F;
    int S;        // series per workgroup
    int NPG;      // head pairs per attention group (K/V buffers hold one group)
    int KSE;      // k-steps of the embed GEMM  (ceil((C+1)/32))
    int CT;       // 16-row tiles of the unembed GEMM (ceil(C/16))
    int rot;      // rotation of the second wave set (SIMD load balance)
    int num_cu;   // CUs of the device (co-resident 4-wave workgroups alternate their tile split)
    int mode, nsteps;
    int lds_temb; // byte offset of the time-embedding scratch in LDS
    int lds_afr;  // byte offset of the attention-output fragments in LDS
    int dbg;      // debugging aid (FDIFF_MEGA_DBG): bit0 zero the attention output, bit1 skip the FFN
    unsigned long long* prof;   // profiling aid (FDIFF_MEGA_PROF): (phase, s_memtime) pairs of WG 0 / wave 0, steps 0-3
    unsigned long long* clk_out;   // measurement aid (fd_prof_begin .. fd_prof_end): workgroup 0 stores {shader-clock counter, 100 MHz wall
                                   // clock} at entry ([0], [1]) and behind its last step ([2], [3]): the shader clock the launch ran at
    unsigned* dbg_out;   // debugging aid: LDS image of workgroup 0 after layer 0's attention
    int dbg_bytes;
    // tensors
    float* x;
    float* score_out;
    const float* tvec;
    const float* params;
    long long pos, tW, td_w, td_b;
    // bf16 fragment images
    const char* img_emb;
    const char* img_unemb;
    const char* img_layers;
    size_t layer_stride;
    size_t off_wk, off_wv, off_wq, off_wo, off_ffn;
    size_t off_ffn32;                    // pair-form FFN image (32x32x16 H) of the layer, 0 when the model has none
    size_t off_lpar;                     // fp32 block [6][D] (bo, b2, g1, b1, g2, b2) of the layer, nlp KiB: fetched by DMA
    int nlp;
    // sampler
    const float* G;
    const fd_sde_step_coef* steps;       // device array [nsteps]
    const float* z_steps;                // injected noise (nsteps, B, T, C) or null
    const float* temb_table;             // (nsteps, D) time embedding of every step's t (sampler mode: t is shared by all
                                         // series, fd_mega_temb_table fills it before the launch) or null
    unsigned long long seed, offset, ctr_per_step, n_elem;
    // probability-flow ODE (FD_MEGA_ODE): `steps` then holds fd_ode_step_coef rows; Heun state (B,T,C), null for Euler
    float* ode_x0;
    float* ode_v0;
    // data-prediction stages (FD_ODE_DDIM and above): their second coefficient pair, device array [nsteps]; D_prev lives in ode_x0
    const fd_dpm_coef* dpm;
};
