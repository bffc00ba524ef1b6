// fd_engine.h -- host pieces shared by the engine loops that differentiate the score network through its training forward and
// input VJP (fd_likelihood.hip, fd_dps.hip), and the transform pieces of conditional sampling (fd_impute.hip) reused by the
// gradient-guided form (fd_dps.hip).
#pragma once
#include "fd_score.h"

// The state of one run, outside the arena (the training forward and its VJP own the arena between them): grow-only, freed with the
// context.  layout(take) points the run's buffers at consecutive shares of ctx->ll_buf, take(bytes) returning the next one; it runs
// twice, first to size the buffer.
template <class Layout>
int fd_ll_carve(fd_ctx* ctx, Layout layout) {
    size_t need = 0;
    layout([&](size_t bytes) -> char* { need += fd_ws::padded(bytes); return nullptr; });
    if (ctx->ll_bytes < need) {
        if (ctx->ll_buf) (void)hipFree(ctx->ll_buf);      // (synchronising: an earlier run on any stream has finished with it)
        ctx->ll_buf = nullptr;
        ctx->ll_bytes = 0;
        FD_HIP(ctx, hipMalloc(&ctx->ll_buf, need));
        ctx->ll_bytes = need;
    }
    char* p = (char*)ctx->ll_buf;
    layout([&](size_t bytes) { char* q = p; p += fd_ws::padded(bytes); return q; });
    return FD_OK;
}

// restores the model's training arithmetic when the run returns
struct fd_train_mode_scope {
    fd_score* m;
    int saved;
    fd_train_mode_scope(fd_score* mm, int mode) : m(mm), saved(mm->train_mode) { m->train_mode = mode; }
    ~fd_train_mode_scope() { m->train_mode = saved; }
};

// The same for label dropout: the training forwards of an evaluation loop (fd_dps.hip, fd_likelihood.hip) read the bound labels as
// they are -- fd_labels_prepare_train draws a model's label_dropout on every training forward otherwise; covariate dropout
// (fd_cov_prepare_train) likewise
struct fd_label_dropout_scope {
    fd_score* m;
    float saved, saved_cov;
    fd_label_dropout_scope(fd_score* mm, float p) : m(mm), saved(mm->label_dropout), saved_cov(mm->cov_dropout) {
        m->label_dropout = p;
        m->cov_dropout = p;
    }
    ~fd_label_dropout_scope() {
        m->label_dropout = saved;
        m->cov_dropout = saved_cov;
    }
};

// the training arithmetic of an evaluation that differentiates the network: bf16 where the model has the bf16 training kernels
// (the transformer at its supported widths), else exact f32
inline int fd_diff_train_mode(const fd_score* m, int mode) {
    return mode == FD_MODE_BF16 && m->backbone == FD_BACKBONE_TRANSFORMER && fd_train_bf16_supported(m) ? FD_MODE_BF16 : FD_MODE_F32;
}

// fd_impute.hip: the packed-DFT basis F then F^T (Tp x Tp each, Tp = 16 ceil(T/16)), cached on the context (the first call for a T
// builds it and waits); nullptr when it cannot be built
const float* fd_impute_basis(fd_ctx* ctx, int T, int Tp, hipStream_t s);
// marginal mean coefficient and std of the perturbation kernel at t (x_t = alpha x_0 + s G z), in double
void fd_marginal_coef(const fd_sde_params& p, double t, double* alpha, double* sdev);
