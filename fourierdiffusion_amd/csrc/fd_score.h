// fd_score.h -- internal definition of the score-network object (fd_score) shared by the fp32
// parity path, the bf16 MFMA path, the backward pass and the sampler.
#pragma once
#include <vector>

#include "fd_common.h"

struct fd_layer_off {
    int64_t in_w, in_b, out_w, out_b, l1_w, l1_b, l2_w, l2_b, n1_w, n1_b, n2_w, n2_b;
};

struct fd_bf16_images;   // fd_score_bf16.hip

// parameter offsets of one layer of the MLP / LSTM backbones (fd_backbones.hip):
//   MLP : a = linear1.weight (d_mlp, D), b = its bias, c = linear2.weight (D, d_mlp), d = its bias
//   LSTM: a = weight_ih_l0 (4D, D), b = weight_hh_l0 (4D, D), c = bias_ih_l0 (4D), d = bias_hh_l0 (4D)
struct fd_bb_off {
    int64_t a, b, c, d;
};

struct fd_score {
    fd_ctx* ctx = nullptr;
    fd_model_dims d{};
    int64_t nparams = 0;
    int64_t pos = 0, tW = 0, td_w = 0, td_b = 0, emb_w = 0, emb_b = 0, un_w = 0, un_b = 0;
    std::vector<fd_layer_off> layers;
    int backbone = 0;               // FD_BACKBONE_TRANSFORMER / _MLP / _LSTM
    int d_mlp = 0;                  // hidden width of the MLP backbone
    std::vector<fd_bb_off> bb;      // per-layer offsets of the MLP / LSTM backbones
    float* params = nullptr;        // caller-owned flat fp32 masters (set by fd_score_prepare)
    bool prepared = false;
    bool bf16_stale = true;         // bf16 weight images older than the fp32 masters (rebuilt lazily: training never reads them)
    hipEvent_t prep_event = nullptr;   // completed by fd_score_prepare's last kernel (its launch's stop event): what a rebuild of the
    void* prep_stream = nullptr;       // weight images on another stream waits for, without an event packet on the caller's stream
    bool prep_event_bound = false;
    hipEvent_t img_event = nullptr;    // completed by a rebuild of the bf16 weight images that runs on a side stream (fd_train_bf16.hip)
    fd_bf16_images* bf16 = nullptr; // engine-owned bf16 weight images (built by prepare)
    // ---- training state (valid between forward_train and backward)
    bool have_saved = false;
    int saved_B = 0;
    float saved_p = 0.f;
    uint64_t saved_seed = 0, saved_offset = 0;
    const float* saved_x = nullptr;
    const float* saved_t = nullptr;
    // this model's last training forward that ran every layer as ONE persistent launch: the context's count of training forwards then, the
    // batch, the tiles per series and the value every tile flag carries behind it (epoch * 64 + layers published); 0 = none yet
    unsigned long long trp_serial = 0, trp_value = 0;
    int trp_B = 0, trp_KT = 0;
    int saved_mask_set = 0;         // which of the two sets of dropout-decision buffers the saved forward used (fd_train_bf16.hip)
    bool saved_bf16 = false;        // the training forward ran the bf16 MFMA kernels (fd_train_bf16.hip)
    int train_mode = 0;             // FD_MODE_F32 (exact-f32 kernels) or FD_MODE_BF16 for fd_score_forward_train
    uint64_t saved_ws_gen = 0;      // ctx->ws_gen right after the training forward carved the arena
    void* saved_ws = nullptr;       // arena base then (a regrow moves it)
    // ---- class conditioning (fd_score_create_cond; not in the reference): class_encoder.weight (n_classes + 1, D) at cls_w, the
    // LAST tensor of the layout; row n_classes is the null (unconditional) token.  n_classes == 0: an unlabelled model.
    int n_classes = 0;
    int64_t cls_w = 0;
    const int* labels = nullptr;    // borrowed device int32[labels_B] (fd_score_set_labels), or null: every row reads the null token
    int labels_B = 0;
    float label_dropout = 0.f;      // training forwards replace a label by the null token with this probability (fd_score_set_label_dropout)
    int* y_eff = nullptr;           // engine-owned device int32[y_eff_cap]: the labels the last training forward really used
    int y_eff_cap = 0;
    // ---- covariate conditioning (fd_score_create_cov, fd_cov.hip; not in the reference): a two-layer encoder of a float vector
    // c_b (cond_dim), e(c) = W2 silu(W1 c + b1) + b2, and a learned null vector, the LAST five tensors of the layout; k_cov_embed adds
    // e(c_b) or the null vector to the time embedding of series b.  cond_dim == 0: no covariates.  Never together with n_classes > 0.
    int cond_dim = 0;
    int64_t cov_w1 = 0, cov_b1 = 0, cov_w2 = 0, cov_b2 = 0, cov_null = 0;
    const float* cov = nullptr;     // borrowed device float[cov_B, cond_dim] (fd_score_set_covariates), or null: every row reads the null vector
    int cov_B = 0;
    const unsigned char* cov_keep = nullptr;   // borrowed keep bytes of the bound rows (a guided pair's [1..1 ; 0..0]), or null: all kept
    float cov_dropout = 0.f;        // training forwards read the null vector with this probability per row (fd_score_set_cov_dropout)
    // engine-owned, grow-only: what the last training forward really used (its backward reads them again) and the encoder
    // gradient's (h, dpre) rows
    float* cov_eff = nullptr;       // float[cov_eff_cap, cond_dim]: copy of the bound covariates
    unsigned char* keep_eff = nullptr;   // cov_eff_cap keep bytes behind covariate dropout
    int cov_eff_cap = 0;
    bool cov_eff_bound = false;     // covariates were bound at that forward (else every row read the null vector)
    float* cov_bwd = nullptr;       // float[2, cov_bwd_cap, d_model]
    int cov_bwd_cap = 0;
};

// the class-embedding operands of k_time_embed: y (B) int32 or null (every row the null token), table (K + 1, D) fp32; table == null:
// an unlabelled model, nothing is added
// the covariate operands of k_cov_embed, launched behind k_time_embed when P > 0: c (B, P) or null (every row the null vector), keep
// (B) bytes or null (every row kept), the encoder's five tensors
struct fd_cov {
    const float* c = nullptr;
    const unsigned char* keep = nullptr;
    const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *nul = nullptr;
    int P = 0;
};
struct fd_cls {
    const int* y = nullptr;
    const float* table = nullptr;
    int K = 0;
    fd_cov cov{};
};
inline fd_cov fd_cov_of(const fd_score* m, const float* c, const unsigned char* keep) {
    const float* P = m->params;
    return fd_cov{c, keep, P + m->cov_w1, P + m->cov_b1, P + m->cov_w2, P + m->cov_b2, P + m->cov_null, m->cond_dim};
}
inline fd_cls fd_cls_eval(const fd_score* m) {      // the labels bound by fd_score_set_labels / the covariates by fd_score_set_covariates
    if (m->cond_dim > 0) return fd_cls{nullptr, nullptr, 0, fd_cov_of(m, m->cov, m->cov_keep)};
    return m->n_classes > 0 ? fd_cls{m->labels, m->params + m->cls_w, m->n_classes} : fd_cls{};
}
inline fd_cls fd_cls_train(const fd_score* m) {     // the labels behind label dropout (fd_labels_prepare_train) / covariates (fd_cov_prepare_train)
    if (m->cond_dim > 0) return fd_cls{nullptr, nullptr, 0, fd_cov_of(m, m->cov_eff_bound ? m->cov_eff : nullptr, m->keep_eff)};
    return m->n_classes > 0 ? fd_cls{m->y_eff, m->params + m->cls_w, m->n_classes} : fd_cls{};
}
// Philox counters of label dropout under the training call's (seed, offset): label b is lane b % 4 of counter offset + kLabelCtrBase
// + b / 4 -- the window of (layer 16383, site 3) in fd_dropout_site_offset's numbering, which no encoder layer reaches
constexpr uint64_t kLabelCtrBase = (uint64_t)0xFFFF << 40;

// activations kept by the training forward, carved from the ctx workspace
struct fd_saved_layer {
    float* x0;     // (M,D)  layer input
    float* qkv;    // (M,3D)
    float* lse;    // (B,H,T) log-sum-exp of scaled scores
    float* att;    // (M,D)  concatenated head outputs
    float* s1;     // (M,D)  x0 + drop(out_proj)
    float* mr1;    // (M,2)  mean, rstd of LN1
    float* x1;     // (M,D)  LN1 output
    float* hact;   // (M,F)  drop(relu(linear1))
    float* s2;     // (M,D)  x1 + drop(linear2)
    float* mr2;    // (M,2)
};

struct fd_saved {
    float* emb;    // (B,D)  Gaussian-Fourier features (input of time_encoder.dense)
    float* temb;   // (B,D)
    float* hL;     // (M,D)  last layer output
    std::vector<fd_saved_layer> layers;
};

// fd_cfg.hip: class conditioning (not in the reference)
// FD_ERR_ARG when labels are bound for another batch size than B (who: the entry point's name in the message)
int fd_labels_check(fd_score* m, int B, const char* who);
// a labelled model's training forward: y_eff[0 .. B) = the bound labels (null token where none are bound or a label is out of range)
// behind label dropout from Philox(seed, offset + kLabelCtrBase); a no-op on an unlabelled model
int fd_labels_prepare_train(fd_score* m, int B, uint64_t seed, uint64_t offset, hipStream_t s);
// d class_encoder.weight[k, :] (+)= sum over the rows b with y_eff[b] == k of dtemb[b, :], b ascending (no atomics); no-op when unlabelled
int fd_class_table_backward(fd_score* m, const float* dtemb, float* grads, int B, int accumulate, hipStream_t s);
void fd_labels_destroy(fd_score* m);

// fd_cov.hip: covariate conditioning (not in the reference)
constexpr int kMaxCondDim = 64;
// temb[b, :] += keep_b ? e(c_b) : null, one workgroup per row behind k_time_embed; no-op when cov.P == 0
void fd_cov_embed_launch(const fd_cov& cov, float* temb, int B, int D, hipStream_t s);
// FD_ERR_ARG when covariates are bound for another batch size than B
int fd_cov_check(fd_score* m, int B, const char* who);
// a covariate model's training forward: copies the bound covariates and draws the keep bytes of covariate dropout from
// Philox(seed, offset + kLabelCtrBase), the lane rule of k_label_dropout; a no-op on any other model
int fd_cov_prepare_train(fd_score* m, int B, uint64_t seed, uint64_t offset, hipStream_t s);
// the encoder's gradient from dtemb (B, D) of the last training forward: b ascending, no atomics; no-op without covariates
int fd_cov_backward(fd_score* m, const float* dtemb, float* grads, int B, int accumulate, hipStream_t s);
void fd_cov_destroy(fd_score* m);

// fd_score_f32.hip
namespace fdf32 {
void time_embed_cls(const float* t, const float* W, const float* Wd, const float* bd, float* temb, int B, int D, hipStream_t s, fd_cls cls);
}
int fd_time_embed_train_cls(const float* t, const float* W, const float* Wd, const float* bd, float* emb, float* temb, int B, int D,
                            hipStream_t s, fd_cls cls);
int fd_score_forward_f32(fd_score* m, const float* x, const float* t, float* out, int B, hipStream_t s,
                         bool train, float dropout_p, uint64_t seed, uint64_t offset);
size_t fd_score_f32_workspace(const fd_score* m, int B, bool train);
void fd_score_carve_saved(const fd_score* m, int B, fd_ws& ws, fd_saved& sv);
size_t fd_score_bwd_workspace(const fd_score* m, int B);   // fd_score_bwd.hip

// fd_score_bf16.hip
int fd_bf16_create(fd_score* m);
void fd_bf16_destroy(fd_score* m);
int fd_bf16_prepare(fd_score* m, hipStream_t s, bool training_only = false, bool ffn32_only = false);
int fd_bf16_refresh(fd_score* m, hipStream_t s, bool training_only = false);   // (training_only: without the sampler-only images)
// rebuilds the images if the masters changed since the last build
int fd_score_forward_bf16(fd_score* m, const float* x, const float* t, float* out, int B, hipStream_t s);
// fd_backbones.hip: the reference's other two score backbones (MLPScoreModule / LSTMScoreModule), exact-f32
int fd_bb_forward(fd_score* m, const float* x, const float* t, float* out, int B, hipStream_t s, bool train, float p,
                  uint64_t seed, uint64_t offset);
int fd_bb_backward(fd_score* m, const float* dout, float* grads, int accumulate, hipStream_t s, float* dx_only = nullptr);
size_t fd_bb_workspace(const fd_score* m, int B, bool train);
// any backbone, eval mode (sampler loop, fd_score_forward)
int fd_score_forward_any(fd_score* m, const float* x, const float* t, float* out, int B, int mode, hipStream_t s);
// (the scaffolding of the step-by-step engine loops: fd_loop.h)
// fd_train_bf16.hip: bf16 MFMA training path (forward with dropout, backward)
bool fd_train_bf16_supported(const fd_score* m);
bool fd_score_train_dsm_bf16_supported(const fd_score* m, int B);
int fd_train_bf16_token_splits(const fd_score* m, int B, int* nblk);
void fd_train_bf16_forward_plan(const fd_score* m, int B, char* out, size_t n);   // "k_tr_fwd_layers NT=.. x .." or "2 kernels per layer"
int fd_train_bf16_cluster_xcds(fd_score* m, int B, int* xcd, hipStream_t s);      // host copy of the tile flags' publisher XCDs
int fd_score_forward_train_bf16(fd_score* m, const float* x, const float* t, float* out, int B, float p, uint64_t seed,
                                uint64_t offset, hipStream_t s);
int fd_score_backward_bf16(fd_score* m, const float* dout, float* grads, int accumulate, hipStream_t s);
// input-only backward of the bf16 path (fd_score_input_vjp): dx = (d s / d x)^T dout, no parameter gradient, no side stream
int fd_score_input_vjp_bf16(fd_score* m, const float* dout, float* dx, hipStream_t s);
int fd_score_train_dsm_bf16(fd_score* m, const float* x, const float* t, const float* target, const float* stdv, int lw,
                            float grad_weight, int B, float p, uint64_t seed, uint64_t offset, float* loss_out, float* grads,
                            int accumulate, hipStream_t s);
int fd_embed_backward(fd_score* m, const float* dh, const float* emb, float* dtemb, float* grads, int B, float* skp,
                      size_t skp_floats, hipStream_t s);   // fd_score_bwd.hip
// fd_attn_bf16.hip
// fd_linear_bf16.hip: bf16 MFMA projections of the step-by-step path (weight images [row tile][k-step], bias in k-slot K)
int fd_linear_bf16(fd_ctx* ctx, const float* x, const char* img, float* out, int M, int N, int K, int ks, hipStream_t s);
int fd_linear_res_ln_bf16(fd_ctx* ctx, const float* x, const char* img, const float* res, const float* gamma, const float* beta,
                          float* out, int M, int D, int ks, int dt, hipStream_t s);
// head_dim 8 .. 32, one head per contraction (fd_attn_wide.hip); qkv = packed projections (B*T, 3D)
int fd_attention_bf16_wide(fd_ctx* ctx, const float* qkv, float* out, int B, int T, int H, int hd, hipStream_t s);
int fd_attention_bf16(fd_ctx* ctx, const float* in, float* out, int B, int T, int H, int hd, hipStream_t s,
                      const char* wk = nullptr, const char* wv = nullptr, const char* wq = nullptr, int ks1 = 0, int out_bf16 = 0,
                      const void* in_rows = nullptr);
