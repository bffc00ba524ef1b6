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
#define FD_MEGA_FORWARD 0   // one score-network forward: x, tvec -> score_out
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
};
