// fd_loop.h -- the scaffolding of the step-by-step engine loops (fd_sampler.hip): the entry checks, the arena layout and t vectors of
// a loop (fd_step_loop), and classifier-free guidance as an option of the plain loops and of the conditional-sampling ones
// (fd_guide, fd_cfg.hip; fd_impute.hip, fd_dps.hip).
//
// A loop form contributes what is its own -- its coefficients, its buffers behind the score, its step launch -- and runs
//   fd_step_loop lp;  fd_step_loop_open(&lp, ...);  for (k ...) { fd_step_loop_eval(&lp, k, x);  <step kernel on lp.score> }
// fd_sampler_run_impute_dps, fd_impute_guidance and the likelihood loops stay separate: their score evaluation is the training
// forward, which owns the arena, so their buffers live outside it (fd_ll_carve) and they fill one t vector per evaluation.
#pragma once
#include "fd_score.h"

// the checks every loop entry point opens with: model, SDE kind, B > 0, mode, fd_score_prepare done (who: its name in the messages)
int fd_loop_check(fd_score* m, const fd_sde_params* sde, int B, int mode, const char* who);
// forward scratch of one step-by-step score evaluation (fd_score_forward_any), at the arena base
size_t fd_loop_fwd_workspace(const fd_score* m, int B);
// reserves fwd + own (+ the t vectors of every step) in the arena; returns the t vector of step 0 at ws + fwd + own and the stride
// between steps, 0 when one vector is refilled every step with fd_fill (FDIFF_SAMPLER_FILL_PER_STEP, or n_steps * B beyond 16 Mi)
int fd_step_table(fd_ctx* ctx, size_t fwd, size_t own, const float* timesteps, int n_steps, int B, hipStream_t s, float** tvec,
                  size_t* stride);
void fd_fill(float* p, int n, float v, hipStream_t s);      // p[0 .. n) = v

// One step-by-step loop over `rows` network rows.  Arena, in order: forward scratch of `rows`, score, the loop's own buffers, the t
// vectors (fd_step_table), the device copy of the evaluation times.
struct fd_step_loop {
    fd_score* m;
    hipStream_t s;
    int rows, mode;
    float* score;           // (rows,T,C)
    char* own;              // own_bytes of the loop's own buffers (solver state, labels)
    float* tvec0;           // t vector of evaluation 0
    size_t tstride;         // floats between evaluations; 0: one vector, refilled by every fd_step_loop_eval
    const float* t_eval;    // host, borrowed from the caller for the loop's lifetime
};
// reserves the arena and fills the t table of the n_eval evaluation times
int fd_step_loop_open(fd_step_loop* lp, fd_score* m, int rows, int mode, size_t own_bytes, const float* t_eval, int n_eval,
                      hipStream_t s);
// score = s(x, t_eval[k]) on the loop's rows
int fd_step_loop_eval(fd_step_loop* lp, int k, const float* x);

// Classifier-free guidance of a plain loop (fd_cfg.hip); a null guide is the plain loop.  pair: the two evaluations of a step run as one
// forward on 2B rows, x (2B,T,C) holds the state twice and the step kernel combines the halves of the score; else one evaluation on B
// rows with the labels y bound (null: the null token on every row).
// A covariate guide (fd_cov.hip, fd_guide_plan_cov) carries c (B, P) in place of y: P > 0, y null.
struct fd_guide {
    bool pair;
    const int* y;           // device int32[B]
    float w, omw;           // the guidance scale and 1 - w
    const float* c = nullptr;      // device float[B, P]
    int P = 0;
};
// What a guided loop runs (fd_cfg.hip): pair = labels present and w outside {0, 1}, or FDIFF_CFG_FORCE_PAIR; else one evaluation on B
// rows with y bound (w = 0 or y null: the null token on every row)
fd_guide fd_guide_plan(const int* y, float w);
// the same for covariates c (B, P): pair = covariates present and w outside {0, 1}, or FDIFF_CFG_FORCE_PAIR
fd_guide fd_guide_plan_cov(const float* c, int P, float w);
// the checks of every guided entry point: a class-conditional model (FD_ERR_ARG otherwise) and a finite guidance scale
int fd_guide_check(fd_score* m, float w, const char* who);
inline int fd_guide_rows(const fd_guide* g, int B) { return g && g->pair ? 2 * B : B; }
// the label vector of the paired forward, the last of the loop's own buffers; a covariate guide: the pair's covariates (2B, P), then
// its 2B keep bytes
inline size_t fd_guide_cov_bytes(const fd_guide* g, int B) { return fd_ws::padded((size_t)2 * B * g->P * sizeof(float)); }
inline size_t fd_guide_bytes(const fd_guide* g, int B) {
    if (!g || !g->pair) return 0;
    return g->P > 0 ? fd_guide_cov_bytes(g, B) + fd_ws::padded((size_t)2 * B) : fd_ws::padded((size_t)2 * B * sizeof(int));
}
// pair: lab[0 .. 2B) = (y, null tokens) -- a covariate guide: (c, c) and the keep bytes [1 .. 1 ; 0 .. 0] -- and x[B .. 2B) =
// x[0 .. B); no-op otherwise
int fd_guide_begin(fd_score* m, const fd_guide* g, void* lab, float* x, int B, hipStream_t s);
// binds a guided loop's labels for its forwards; the caller's binding is back when the scope ends (the kernels have taken their
// pointers at launch)
struct fd_guide_scope {
    fd_score* m;
    const int* y;
    int B;
    const float* c;
    const unsigned char* keep;
    int cB;
    fd_guide_scope(fd_score* mm, const fd_guide* g, const void* lab, int rows)
        : m(mm), y(mm->labels), B(mm->labels_B), c(mm->cov), keep(mm->cov_keep), cB(mm->cov_B) {
        if (!g) return;
        if (g->P > 0) {
            m->cov = g->pair ? (const float*)lab : g->c;
            m->cov_keep = g->pair ? (const unsigned char*)lab + fd_guide_cov_bytes(g, rows / 2) : nullptr;
            m->cov_B = m->cov ? rows : 0;
            return;
        }
        m->labels = g->pair ? (const int*)lab : g->y;
        m->labels_B = m->labels ? rows : 0;
    }
    ~fd_guide_scope() {
        m->labels = y;
        m->labels_B = B;
        m->cov = c;
        m->cov_keep = keep;
        m->cov_B = cB;
    }
};
// the guided score of one element; the intrinsics keep the two products and the sum from being contracted into an fma
__device__ __forceinline__ float fd_guided(float sc, float su, float w, float omw) {
    return __fadd_rn(__fmul_rn(w, sc), __fmul_rn(omw, su));
}
// the paired Euler-Maruyama step (k_cfg_sde_step): x (2B,T,C) in place from score (2B,T,C), arguments as fd_sde_step
int fd_cfg_sde_step(fd_ctx* ctx, const fd_sde_params* sde, const float* G, float* x, const float* score, const float* z, uint64_t seed,
                    uint64_t offset, double t, float dt, const fd_guide& g, int B, int T, int C, hipStream_t s);

// The stepwise bodies behind fd_sampler_run / fd_sampler_run_cfg and fd_sampler_run_ode / _dpm / _ode_cfg (fd_sampler.hip), the
// arguments checked by the entry point.  A guided loop has no fused form.
int fd_sampler_sde_loop(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt, float* x,
                        const float* z_steps, uint64_t seed, uint64_t offset, int B, int mode, hipStream_t s, const fd_guide* g);
// solver 0 .. 3 as fd_solver_rows (fd_ode.h)
int fd_sampler_ode_loop(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, int solver,
                        float* x, int B, int mode, hipStream_t s, const fd_guide* g);
