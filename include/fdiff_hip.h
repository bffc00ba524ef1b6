/*
 * fdiff_hip.h -- C ABI of libfdiff_hip.so, the MI355X (gfx950) engine for the
 * score-matching hot path of JonathanCrabbe/FourierDiffusion.
 *
 * The reference has no FFI of its own for this path: it sits behind plain Python
 * classes.  Each entry point below therefore names the reference
 * *Python* interface it replaces (file:line relative to /root/reference); the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and lives in
 * fourierdiffusion_amd/_C.py.
 *
 * Conventions
 *   - extern "C"; plain pointers and sizes only (no torch types).
 *   - every function returns 0 on success, <0 on error (FD_ERR_*); the message is
 *     available from fd_last_error(ctx).
 *   - all data pointers are CALLER-OWNED DEVICE pointers (float32, row-major,
 *     contiguous (B,T,C)) unless marked "host".  bf16 exists only inside the engine.
 *   - asynchronous on the passed hipStream_t (void* to keep the header toolchain-free);
 *     no host synchronisation inside any call unless stated.
 *   - one fd_ctx per (process, device); a ctx and the models created from it are
 *     not thread-safe.
 */
#ifndef FDIFF_HIP_H
#define FDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_OK 0
#define FD_ERR_ARG (-1)      /* bad argument (shape, null pointer, unsupported size) */
#define FD_ERR_HIP (-2)      /* a HIP runtime call failed */
#define FD_ERR_STATE (-3)    /* call order violated (e.g. forward before prepare) */
#define FD_ERR_COMM (-4)     /* RCCL failure */
#define FD_ERR_UNSUPPORTED (-5)

typedef struct fd_ctx fd_ctx;
typedef struct fd_score fd_score;

/* ---------------------------------------------------------------- context */
int fd_version(void);
int fd_ctx_create(int device, fd_ctx** out);
int fd_ctx_destroy(fd_ctx* ctx);
const char* fd_last_error(fd_ctx* ctx);   /* host string, valid until the next call on ctx */
/* number of bytes currently held by the ctx workspace (activations, scratch) */
size_t fd_ctx_workspace_bytes(fd_ctx* ctx);
/* Asynchronous device-side errors recorded since the last report: FD_OK, or FD_ERR_STATE when a kernel of an earlier training
 * call gave up a bounded inter-workgroup wait (the F-split hand-over of the training FFN kernels, or a cluster exchange of the
 * persistent training forward: fd_last_error names the token block / layer and series; that step's gradients are invalid).  Never
 * synchronises -- call it behind a stream synchronisation to cover everything enqueued so far.  Every training / optimizer entry
 * point performs the same check on entry, i.e. DETECTION LAGS BY ONE CALL unless the stream is synchronised; the optimizer
 * kernel itself tests a device-resident copy of the error word in stream order and skips the update of such a step.  (The reference has no
 * counterpart: torch autograd, src/fdiff/models/score_models.py:96-108, has no inter-workgroup protocol to fail.) */
int fd_ctx_check(fd_ctx* ctx);
/* After a reported cluster timeout of the persistent training forward the context trains on the per-layer kernels (whatever kept a
 * cluster from becoming resident -- a co-tenant process, a CU mask -- may still be there).  This re-arms the persistent form once the
 * caller knows the cause is gone.  No reference counterpart (see fd_ctx_check). */
int fd_ctx_rearm(fd_ctx* ctx);

/* ---------------------------------------------------------- measurement hooks
 * bench.py's roofline leg: between fd_prof_begin and fd_prof_end the engine brackets every launch of its
 * dominant kernel (the persistent score-network/sampler kernel; the fused FFN kernel on the step-by-step
 * fallback path) with HIP events on the launch stream.  fd_prof_end synchronises those events and returns
 * the kernel name, the average launch duration, the launch count and the ALGORITHMIC flops of one launch
 * (SURVEY.md 8d formula x series x diffusion steps in the launch; padding flops are not counted). */
int fd_prof_begin(fd_ctx* ctx);
/* after fd_prof_begin: bracket only every `every`-th launch of each kernel (an event pair costs the stream ~5 us; the
 * training step launches its bracketed kernels 20 times) */
int fd_prof_stride(fd_ctx* ctx, int every);
int fd_prof_end(fd_ctx* ctx, char* name_out /* >= 128 bytes */, double* avg_us, int* launches,
                double* flops_per_launch);
/* after fd_prof_end: the shader clock (MHz) the window's last persistent-kernel launch ran at -- workgroup 0's shader-clock counter
 * against the 100 MHz wall clock between its entry and the end of its last step; 0 when the window held no such launch.  The chip is
 * power-limited on this kernel and boxes differ by +-2.5 %: the bench line records the clock beside the time. */
int fd_prof_shader_clock_mhz(fd_ctx* ctx, double* mhz);

/* --------------------------------------------- a1/a2 spectral representation
 * replaces fdiff.utils.fourier.dft   (src/fdiff/utils/fourier.py:8-45)
 *      and fdiff.utils.fourier.idft  (src/fdiff/utils/fourier.py:48-87)
 * y[b, 0:T/2+1, c] = Re X_k ; y[b, T/2+1:T, c] = Im X_k (k=1..), ortho norm.
 * In place (x == y) is NOT allowed. */
int fd_rfft_pack(fd_ctx* ctx, const float* x, float* y, int B, int T, int C, void* stream);
int fd_irfft_unpack(fd_ctx* ctx, const float* x, float* y, int B, int T, int C, void* stream);
/* fused dataset front-end (src/fdiff/dataloaders/datamodules.py:61-62, cmd/sample.py:76-82):
 *   fd_rfft_pack_standardize : y = (dft(x) - mean) / std      mean,std (T,C)
 *   fd_destandardize_irfft   : y = idft(x * std + mean)                              */
int fd_rfft_pack_standardize(fd_ctx* ctx, const float* x, const float* mean, const float* std,
                             float* y, int B, int T, int C, void* stream);
int fd_destandardize_irfft(fd_ctx* ctx, const float* x, const float* mean, const float* std,
                           float* y, int B, int T, int C, void* stream);
/* spectral utilities on the packed representation xt = dft(x) (dataset front-end); the Python surface
 * (fdiff.utils.fourier.spectral_density / localization_metrics / smooth_frequency) composes them with fd_rfft_pack /
 * fd_irfft_unpack exactly as the reference composes its own dft / idft:
 *   fd_spectral_density     replaces spectral_density(x, apply_dft=False)  (src/fdiff/utils/fourier.py:90-124)
 *                           dens (B, T/2+1, C) = Re X_k^2 + Im X_k^2
 *   fd_localization_metrics replaces localization_metrics(X)               (src/fdiff/utils/fourier.py:127-175)
 *                           x (B,T,C) and xt = dft(x); loc, spec_loc (B,) = min_s sum_t e_t min(|t-s|, T-|t-s|)^2 with e the
 *                           normalised energy per time step / per bin of the two-sided spectrum
 *   fd_frequency_smooth     replaces the Gaussian mixing of smooth_frequency(X, sigma)  (src/fdiff/utils/fourier.py:189-203)
 *                           out[b,s,c] = sum_t xt[b,t,c] G[t,s]; gauss_scratch = T*T floats (caller-owned, receives G);
 *                           T must be odd (the reference's frequency vector has T-1 entries for even T and its einsum fails) */
int fd_spectral_density(fd_ctx* ctx, const float* xt, float* dens, int B, int T, int C, void* stream);
int fd_localization_metrics(fd_ctx* ctx, const float* x, const float* xt, float* loc, float* spec_loc,
                            int B, int T, int C, void* stream);
int fd_frequency_smooth(fd_ctx* ctx, const float* xt, float sigma, float* gauss_scratch, float* out,
                        int B, int T, int C, void* stream);

/* ------------------------------------------------------------ a3..a8 SDE
 * kind 0 = VP  (p0 = beta_min,  p1 = beta_max)   fdiff.schedulers.sde.VPScheduler (sde.py:168-246)
 * kind 1 = VE  (p0 = sigma_min, p1 = sigma_max)  fdiff.schedulers.sde.VEScheduler (sde.py:90-165) */
typedef struct fd_sde_params {
    int kind;
    float p0, p1;
} fd_sde_params;

/* Standard normals from the engine's Philox4x32-10 stream: element i of the call uses
 * counter (offset + i/4), key = seed.  Used for the prior, the per-step noise and tests. */
int fd_randn(fd_ctx* ctx, float* out, size_t n, uint64_t seed, uint64_t offset, void* stream);
/* The generator underneath, for audits and tests: out[4 i .. 4 i + 3] = Philox4x32-10(counter = (offset + i, 0), key = seed)
 * (Salmon et al., SC'11; the stream torch.randn / nn.Dropout draw from on the reference's CUDA path is the same generator
 * with another counter layout, so the draws are equal in distribution, not bit for bit: SURVEY 7.2). */
int fd_philox_words(fd_ctx* ctx, uint32_t* out, size_t n_counters, uint64_t seed, uint64_t offset, void* stream);
/* The dropout decisions of the bf16 training path (replaces nn.Dropout's masks inside nn.TransformerEncoderLayer,
 * score_models.py:41-49): out[i] bit e = KEEP decision e of counter offset + i, e = 0..15.  Decision e compares the 16-bit
 * window at byte offset e of the 128-bit Philox output (little endian, wrapping) with thr16 = round(p * 65536): kept with
 * probability 1 - thr16 / 65536 exactly; windows overlap in one byte, so neighbours depend on each other only through ties
 * of the high byte (1 in 256). */
int fd_dropout_decisions(fd_ctx* ctx, uint16_t* out, size_t n_counters, float p, uint64_t seed, uint64_t offset,
                         void* stream);

/* replaces SDE.prior_sampling (sde.py:79-87) + VE override (sde.py:125-127):
 *   out = G[t] * z (VE: * sigma_max).  z == NULL -> z drawn on device (seed, offset). */
int fd_prior_sample(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* z,
                    uint64_t seed, uint64_t offset, float* out, int B, int T, int C, void* stream);

/* replaces VPScheduler.step (sde.py:215-246) / VEScheduler.step (sde.py:129-165):
 *   VP: out = x + (0.5*beta*x + beta*G^2*score)*dt + sqrt(dt*beta)*G*z
 *   VE: out = x + g^2*G^2*score*dt + sqrt(dt)*g*G*z
 * One fused pass (reads x, score [, z]; writes out; out may alias x).
 * z == NULL -> on-device Philox noise (seed, offset). t is the Python float the reference passes. */
int fd_sde_step(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* x,
                const float* score, const float* z, uint64_t seed, uint64_t offset, double t,
                float dt, float* out, int B, int T, int C, void* stream);

/* replaces the perturbation half of loss_fn (src/fdiff/utils/losses.py:66-85) with
 * marginal_prob (sde.py:108-123,187-210) and add_noise (sde.py:66-77) fused:
 *   std[b,k] = s(t_b)*G[k];  x_noisy = m(t_b)*x + std*z;  target = z/std
 * z == NULL -> Philox noise.  std_out (B,T) and target (B,T,C) may be NULL. */
int fd_perturb(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* x,
               const float* t, const float* z, uint64_t seed, uint64_t offset, float* x_noisy,
               float* target, float* std_out, int B, int T, int C, void* stream);

/* replaces the reduction half of loss_fn (losses.py:92-124, reduce_mean=True):
 *   likelihood_weighting == 0: mean_b mean_{t,c} w_b (score+target)^2, w_b = 1/sum_k std^-2
 *   likelihood_weighting == 1: mean_b mean_{t,c} (std (score+target))^2
 * loss_out: device float[1].  dscore (nullable): d loss / d score, (B,T,C). */
int fd_dsm_loss(fd_ctx* ctx, const float* score, const float* target, const float* std,
                int likelihood_weighting, float* loss_out, float* dscore, int B, int T, int C,
                void* stream);

/* ------------------------------------------------------- a9 score network
 * replaces fdiff.models.score_models.ScoreModule (score_models.py:22-166): transformer
 * encoder (post-LN, relu, dim_ff) between Linear embed/unembed, learned positional table
 * with max_norm, Gaussian-Fourier time embedding.                                       */
typedef struct fd_model_dims {
    int n_channels;   /* C */
    int max_len;      /* T */
    int d_model;      /* D */
    int n_head;       /* H, D % H == 0 */
    int num_layers;   /* L */
    int dim_ff;       /* F (torch default 2048) */
} fd_model_dims;

/* Flat fp32 parameter buffer layout.  Order = the reference's state_dict order
 * (SURVEY.md A.4); every tensor starts on a 16-byte boundary.  name uses the reference's
 * state_dict key.  Call with entries == NULL to get the count. */
typedef struct fd_param_entry {
    char name[96];
    int64_t offset;   /* in floats */
    int64_t numel;
    int32_t rows, cols;   /* cols == 0 for vectors */
    int32_t trainable;    /* 0 for time_encoder.W (requires_grad=False, transformer.py:72-74) */
} fd_param_entry;
/* Stand-alone encoders of src/fdiff/models/transformer.py (the fused score network does not call these; they
 * back the PositionalEncoding / GaussianFourierProjection classes of the fdiff surface):
 *   fd_positional_add: renorm rows of table (T,D) IN PLACE to max_norm (nn.Embedding(max_norm), :13-15), then
 *                      out[b,t,:] = x[b,t,:] + table[t,:]                                   (:17-29)
 *   fd_time_embed_add: e = cat[sin,cos](2*pi*t*W)[:D]; p = e Wd^T + bd; out = x + p (broadcast over the time
 *                      axis when T > 0; T == 0 means x is (B,D))                            (:77-91) */
int fd_positional_add(fd_ctx* ctx, const float* x, float* table, float* out, int B, int T, int D, float max_norm,
                      void* stream);
int fd_time_embed_add(fd_ctx* ctx, const float* x, const float* t, const float* W, const float* Wd,
                      const float* bd, float* out, int B, int T, int D, void* stream);
/* The self-attention kernels of the score network on their own (the network calls them through its layer stack; the tests pin each
 * kernel class to float64 attention through this entry): out = softmax(q k^T / sqrt(head_dim)) v per head, eval mode (no dropout).
 *   qkv (B*T, 3*H*head_dim) fp32 rows [q | k | v], out (B*T, H*head_dim) fp32, heads concatenated (torch MHA layout); head_dim 1..64.
 *   kind 0: the dispatch of the bf16 mode's unfused layer form -- packed bf16 kernel (head_dim <= 7), wide bf16 kernel (8..32), and
 *           the exact-f32 kernel for head_dim > 32 or when K / V^T of one head and series exceed the LDS
 *        1: exact f32 (any head_dim);  2: bf16 packed, two heads per MFMA (head_dim <= 7);  3: bf16 wide, one head per MFMA (<= 32)
 * Kinds 2 and 3 return FD_ERR_UNSUPPORTED where the kernel has no instantiation or its LDS image does not fit (no fallback). */
int fd_attention_forward(fd_ctx* ctx, const float* qkv, float* out, int B, int T, int H, int head_dim, int kind, void* stream);

int64_t fd_score_param_count(const fd_model_dims* dims);
int fd_score_layout(const fd_model_dims* dims, fd_param_entry* entries, int* n_entries);

int fd_score_create(fd_ctx* ctx, const fd_model_dims* dims, fd_score** out);

/* The reference's other two score backbones, behind the same fd_score handle and entry points
 * (forward, training pair, sampler loop, optimiser):
 *   FD_BACKBONE_MLP   replaces fdiff.models.score_models.MLPScoreModule  (score_models.py:169-246): the series is flattened
 *                     to (B, T*C), Linear embed, + time embedding, num_layers x { h += Linear(relu-dropout(Linear(h))) with
 *                     torchvision.ops.MLP(hidden=[d_mlp, d_model], dropout 0.1) }, Linear unembed; n_head / dim_ff unused.
 *   FD_BACKBONE_LSTM  replaces fdiff.models.score_models.LSTMScoreModule (score_models.py:249-317): Linear embed, + time
 *                     embedding, num_layers x { h += nn.LSTM(d_model, d_model, batch_first)(h) }, Linear unembed.
 * Both run exact-f32 kernels in either mode (no positional table: pos_encoder is None in the reference).
 * Limits, refused by the three calls below: MLP d_mlp > 0 and d_model <= 1024; LSTM d_model <= 100 (the backward through time
 * keeps W_hh, 4 d_model^2 floats, and 8 d_model more in the 160 KiB LDS).
 * State-dict names: backbone.{i}.0.weight|bias, backbone.{i}.3.weight|bias (MLP); backbone.{i}.weight_ih_l0,
 * weight_hh_l0, bias_ih_l0, bias_hh_l0 (LSTM, gate order i|f|g|o). */
#define FD_BACKBONE_TRANSFORMER 0
#define FD_BACKBONE_MLP 1
#define FD_BACKBONE_LSTM 2
int64_t fd_score_param_count_ex(const fd_model_dims* dims, int backbone, int d_mlp);
int fd_score_layout_ex(const fd_model_dims* dims, int backbone, int d_mlp, fd_param_entry* entries, int* n_entries);
int fd_score_create_ex(fd_ctx* ctx, const fd_model_dims* dims, int backbone, int d_mlp, fd_score** out);
int fd_score_destroy(fd_score* m);

/* Class-conditional score models (NOT in the reference: its ScoreModule.forward, score_models.py:67-94, never reads batch.y).
 * A transformer-backbone model with n_classes = K > 0 owns one more tensor, class_encoder.weight (K + 1, D), appended BEHIND every
 * tensor of fd_score_layout (no existing offset moves); row K is the null (unconditional) token.  Row y_b of the table is added to
 * the time embedding of series b, in fp32, inside the time-embedding kernel of every forward and training path.  n_classes = 0 is
 * fd_score_layout / fd_score_create exactly.  The persistent kernel shares one time embedding per diffusion step, so a labelled
 * model runs the per-layer kernels and every sampling loop step by step (fd_score_plan says so).
 *   fd_score_set_labels        binds a DEVICE int32 vector of B labels to the model (borrowed; y == NULL clears it).  While labels
 *                              are bound, fd_score_forward, fd_score_forward_train, fd_score_train_dsm and fd_score_input_vjp with
 *                              another B return FD_ERR_ARG.  With nothing bound every row reads the null token, so every entry
 *                              point that takes no labels runs a labelled model as its unconditional model.  A label outside
 *                              [0, K] reads the null token (the table is never read out of bounds).
 *   fd_score_set_label_dropout p in [0, 1]: every TRAINING forward replaces each row's label by the null token with probability p,
 *                              decided by the Philox stream of that call: label b is lane b % 4 (uniform < p) of counter
 *                              offset + (0xFFFF << 40) + b / 4 under the call's seed -- the counter window of encoder layer 16383,
 *                              which the dropout sites never reach.  Eval forwards never drop.  The class-table gradient
 *                              dTable[k] = sum_{b: y_b = k} dtemb[b] is summed over b in ascending order (no atomics).
 *   fd_score_get_labels        the binding as it stands: *y the bound vector (NULL: none) and *B its length, so that a caller can
 *                              bind labels for a run and put the earlier binding back (log_likelihood with labels does).
 *   fd_label_dropout           the decision kernel alone: y_out[b] = the label the training forward of (seed, offset) uses for
 *                              y[b] (y == NULL: all null).  y, y_out: device int32[B]. */
int64_t fd_score_param_count_cond(const fd_model_dims* dims, int n_classes);
int fd_score_layout_cond(const fd_model_dims* dims, int n_classes, fd_param_entry* entries, int* n_entries);
int fd_score_create_cond(fd_ctx* ctx, const fd_model_dims* dims, int n_classes, fd_score** out);
int fd_score_set_labels(fd_score* m, const int32_t* y, int B);
int fd_score_get_labels(fd_score* m, const int32_t** y, int* B);
int fd_score_set_label_dropout(fd_score* m, float p);
int fd_label_dropout(fd_ctx* ctx, const int32_t* y, int32_t* y_out, int B, int n_classes, float p, uint64_t seed, uint64_t offset,
                     void* stream);

/* Covariate-conditional score models (an extension, not in the reference).  A transformer-backbone model with cond_dim = P in
 * [1, 64] reads a float vector c_b (P) per series through a two-layer encoder e(c) = W2 silu(W1 c + b1) + b2 of hidden width
 * d_model, and owns five more tensors appended BEHIND every tensor of fd_score_layout (no existing offset moves):
 * cov_encoder.0.weight (D, P), cov_encoder.0.bias (D), cov_encoder.2.weight (D, D), cov_encoder.2.bias (D), cov_encoder.null (D).
 * One kernel behind the time-embedding kernel of every forward and training path ends the time embedding of series b with
 * + (keep_b ? e(c_b) : null), in fp32.  cond_dim = 0 is fd_score_layout_cond / fd_score_create_cond exactly; cond_dim > 0 together
 * with n_classes > 0 is FD_ERR_ARG.  As a class-conditional model, a covariate model runs the per-layer kernels and every sampling
 * loop step by step (fd_score_plan says so).
 *   fd_score_layout_cov       the layout (entries NULL: the count alone) and, n_params non-NULL, the float count of the flat buffer
 *                             (an extension, not in the reference).
 *   fd_score_create_cov       the model (an extension, not in the reference).
 *   fd_score_set_covariates   binds a DEVICE float matrix (B, P) to the model (borrowed; c == NULL unbinds).  While covariates are
 *                             bound, fd_score_forward, fd_score_forward_train, fd_score_train_dsm and fd_score_input_vjp with
 *                             another B return FD_ERR_ARG.  With nothing bound every row reads the null vector (an extension, not
 *                             in the reference).
 *   fd_score_get_covariates   the binding as it stands (an extension, not in the reference).
 *   fd_score_set_cov_dropout  p in [0, 1]: every TRAINING forward reads the null vector on a row with probability p, decided by the
 *                             Philox stream of that call in the counter window and by the lane rule of label dropout: the keep
 *                             bytes equal fd_label_dropout's output != n_classes for the same seed, offset and p.  Eval forwards
 *                             never drop (an extension, not in the reference).
 *   fd_cov_dropout            the keep bytes alone: keep[b] = 1 unless the training forward of (seed, offset) drops row b.  keep:
 *                             device uint8[B] (an extension, not in the reference).
 *   fd_cov_embed              the encoder kernel alone on raw device pointers: e[b, :] = keep_b ? e(c_b) : null, e (B, D); c NULL:
 *                             every row the null vector; keep NULL: every row kept (an extension, not in the reference).
 *   fd_cov_embed_backward     the encoder gradient alone from an injected dtemb (B, D): dW2, db2, dW1, db1 over the kept rows, dnull
 *                             over the dropped ones, summed over b ascending without atomics (bit-reproducible); accumulate != 0
 *                             adds to the outputs.  Uses the context workspace (an extension, not in the reference). */
int fd_score_layout_cov(const fd_model_dims* dims, int n_classes, int cond_dim, fd_param_entry* entries, int* n_entries,
                        int64_t* n_params);
int fd_score_create_cov(fd_ctx* ctx, const fd_model_dims* dims, int n_classes, int cond_dim, fd_score** out);
int fd_score_set_covariates(fd_score* m, const float* c, int B);
int fd_score_get_covariates(fd_score* m, const float** c, int* B);
int fd_score_set_cov_dropout(fd_score* m, float p);
int fd_cov_dropout(fd_ctx* ctx, uint8_t* keep, int B, float p, uint64_t seed, uint64_t offset, void* stream);
int fd_cov_embed(fd_ctx* ctx, const float* w1, const float* b1, const float* w2, const float* b2, const float* nul, const float* c,
                 const uint8_t* keep, float* e, int B, int P, int D, void* stream);
int fd_cov_embed_backward(fd_ctx* ctx, const float* w1, const float* b1, const float* w2, const float* c, const uint8_t* keep,
                          const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, float* dnull, int B, int P, int D,
                          int accumulate, void* stream);

/* Derive the engine-side weight images from the flat fp32 parameters (device pointer):
 * max_norm-renormed positional table (the reference renorms in place inside forward,
 * transformer.py:13-15,27), bf16 MFMA-fragment-ordered matrices, folded biases.
 * Must be called after every change of params (load, optimizer step) before forward.
 * The engine keeps the pointer `params` (no copy of the fp32 masters). */
int fd_score_prepare(fd_score* m, const float* params, void* stream);
/* Point a prepared model at another flat parameter buffer that has itself been through fd_score_prepare since it last changed
 * (not in the reference: the swap between the raw and the averaged weights, fd_adamw_ema_step): the pointer is replaced and the
 * derived images are marked stale, but the positional table is NOT renormalised again -- a second renormalisation moves the last
 * bits of rows that sit at the bound, and the swap must give the weights back bit for bit.  No device work. */
int fd_score_rebind(fd_score* m, const float* params);

#define FD_MODE_F32 0    /* fp32 parity path (exact-f32 arithmetic) */
#define FD_MODE_BF16 1   /* bf16 MFMA operands, fp32 accumulate / residual / LN / softmax */

/* ScoreModule.forward (score_models.py:67-94), eval mode: x (B,T,C), t (B) -> out (B,T,C) */
int fd_score_forward(fd_score* m, const float* x, const float* t, float* out, int B, int mode,
                     void* stream);

/* Introspection (no launch): writes a description of the kernel path that fd_score_forward / fd_sampler_run take for a
 * batch of B series in `mode` -- for the persistent kernel the template instantiation, series per workgroup S, grid and
 * LDS bytes.  The parity tests assert through it that the instantiation they target really runs (the ecg bench workload
 * is `ShapeStatic<100,72,12,12,2,...>` with S = 2 on a 256-CU device).  No reference counterpart. */
int fd_score_plan(fd_score* m, int B, int mode, char* out /* >= 192 bytes */, int* series_per_workgroup /* nullable */);

/* Run-time specialisation of the persistent kernel (csrc/fd_mega_rtc.hip).  The library carries static-shape instantiations of
 * k_mega for the BASELINE shapes only; any other (model class, series shape, workgroup plan) gets its own through hiprtc on first use
 * -- FDIFF_MEGA_JIT: unset = sampler loops of >= 100 diffusion steps, 1 = every launch, 0 = never -- cached on disk under
 * $FDIFF_CACHE_DIR (default ~/.cache/fdiff_hip).  This entry compiles ONE instantiation into that cache without loading it (no GPU
 * needed): key14 = {KS1, DT, KSO, MT, T, D, C, H, S, NPG, rot, L, F, FFN32} as fd_score_plan prints them; msg (nullable, n bytes)
 * receives the instantiation and where its code object came from.  FD_ERR_UNSUPPORTED when hiprtc is missing or the compilation
 * fails (the engine then runs its run-time-shape instantiation).  Replaces nothing in the reference: torch specialises nothing per
 * dataset shape (src/fdiff/models/score_models.py:57-62 builds one nn.TransformerEncoder for every (max_len, n_channels)). */
int fd_mega_jit_compile(const int* key14, char* msg, int n);

/* Arithmetic of the training pair below: FD_MODE_F32 (default; exact-f32 kernels, the parity anchor, any model) or
 * FD_MODE_BF16 (bf16 MFMA operands, fp32 accumulate/LayerNorm/softmax; five fused kernels per encoder layer, weight
 * gradients reduced in a fixed order: bit-reproducible).  FD_ERR_UNSUPPORTED when the bf16 kernels are not instantiated
 * for the model's dims (the mode then stays unchanged).  Replaces nothing in the reference (torch autograd is fp32). */
int fd_score_set_train_mode(fd_score* m, int mode);
/* The training launch plan of a batch of B series, nothing launched: out (>= 192 bytes) names the arithmetic and, on the bf16
 * path, the token splits of the weight-gradient kernel (also in *token_splits, nullable; 0 on the exact-f32 path). */
int fd_score_train_plan(fd_score* m, int B, char* out, int* token_splits);
/* Where the last training forward's clusters ran, for the parity tests (no reference counterpart): when the last training forward
 * on the model's context was the persistent bf16 form of THIS model at batch B (every encoder layer in one launch, a cluster of
 * workgroups per series), waits for `stream` and writes the XCD that published each 16-token tile of each series into the HOST
 * array xcd[B * ceil(max_len / 16)], laid out [series][tile].  A series whose tiles all carry one XCD exchanged its rows through
 * that XCD's L2, any other one through the memory-side path.  FD_ERR_ARG for a null pointer or a B other than that forward's;
 * FD_ERR_STATE when the last training forward was not that form (per-layer kernels, exact-f32 path, one layer, another model,
 * none yet) or a tile flag does not carry that launch's value. */
int fd_score_train_cluster_xcds(fd_score* m, int B, int* xcd, void* stream);

/* Training forward: keeps activations in the ctx workspace for fd_score_backward.
 * dropout_p > 0 applies the four dropout sites of nn.TransformerEncoderLayer with masks
 * from Philox(seed, offset) (regenerated in backward). */
int fd_score_forward_train(fd_score* m, const float* x, const float* t, float* out, int B,
                           float dropout_p, uint64_t seed, uint64_t offset, void* stream);
/* dout (B,T,C) -> grads (flat, same layout as params; ACCUMULATED into if accumulate != 0) */
int fd_score_backward(fd_score* m, const float* dout, float* grads, int accumulate, void* stream);
/* Input vector-Jacobian product of the last fd_score_forward_train: dx (B,T,C) = (d out / d x)^T dout.  Consumes the saved
 * forward as fd_score_backward does (same checks and error codes); forms no parameter gradient and touches no gradient buffer.
 * Every backbone and training arithmetic.  (Not in the reference; the likelihood loop below is its user.) */
int fd_score_input_vjp(fd_score* m, const float* dout, float* dx, void* stream);

/* One optimisation step's device work in one call: fd_score_forward_train -> fd_dsm_loss -> fd_score_backward
 * (the body of get_sde_loss_fn's loss_fn + loss.backward(), src/fdiff/utils/losses.py:39-125 and
 * score_models.py:96-120) with the unembedder, the loss and the unembedder's backward fused into one kernel.
 * x: the perturbed batch (B,T,C); target, std: fd_perturb's outputs; loss_out: device float[1];
 * grad_weight scales the gradient (not the loss); grads as in fd_score_backward.
 * FD_ERR_UNSUPPORTED when the model does not train on the bf16 transformer path: run the three calls. */
int fd_score_train_dsm(fd_score* m, const float* x, const float* t, const float* target, const float* std,
                       int likelihood_weighting, float grad_weight, int B, float dropout_p, uint64_t seed,
                       uint64_t offset, float* loss_out, float* grads, int accumulate, void* stream);
/* 1 when fd_score_train_dsm has a fused step for this (model, train mode, B), else 0 (it would return FD_ERR_UNSUPPORTED).
 * No side effects: the host asks before it draws the step's Philox key. */
int fd_score_train_dsm_supported(fd_score* m, int B);

/* ----------------------------------------------------------- a12 sampler
 * replaces the inner loop of DiffusionSampler.sample (src/fdiff/sampling/sampler.py:83-104):
 * for i in range(n_steps): score = model(x, t_i); x = sde.step(score, t_i, x).
 * timesteps: HOST float[n_steps] (the scheduler's linspace grid, sde.py:62-64).
 * x: device (B,T,C), in/out.  z_steps: device (n_steps,B,T,C) injected noise or NULL for
 * on-device Philox (seed; step i, element e uses offset + i*ceil(BTC/4) + e/4).
 * The whole loop is enqueued on `stream` without any host synchronisation. */
int fd_sampler_run(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps,
                   int n_steps, float dt, float* x, const float* z_steps, uint64_t seed,
                   uint64_t offset, int B, int mode, void* stream);

/* Predictor-corrector extension (NOT in the reference, whose sampler is predictor-only; default off in the Python surface;
 * parity unpinned -- follows Song et al. 2021, Alg. 4/5, in the coordinates whitened by G):
 *   fd_langevin_step : per series eps = 2 alpha (snr |z| / |G score|)^2 ; out = x + eps G^2 score + sqrt(2 eps) G z
 *                      (z == NULL: on-device Philox noise, needs T*C % 4 == 0; out may alias x)
 *   fd_sampler_run_pc: fd_sampler_run with n_corr corrector steps (a score evaluation each) before every predictor step;
 *                      alpha = 1 - beta(t) dt (VP) or 1 (VE); zc_steps (n_steps, n_corr, B, T, C) injected corrector noise or NULL */
int fd_langevin_step(fd_ctx* ctx, const float* G, const float* x, const float* score, const float* z, uint64_t seed,
                     uint64_t offset, float snr, float alpha, float* out, int B, int T, int C, void* stream);
int fd_sampler_run_pc(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                      float* x, const float* z_steps, const float* zc_steps, int n_corr, float snr, uint64_t seed,
                      uint64_t offset, int B, int mode, void* stream);

/* Conditional sampling extension (NOT in the reference): imputation and forecasting from observed time-domain values
 * (Song et al. 2021, Sec. 5 / App. I.2, score_sde's inpainter).  y (T,C) observations at data scale, m its 0/1 mask (1 =
 * observed, time domain), x0_obs = A^-1(where(m, y, 0)) in sample space with A(x) = idft(sigma x + mu) (fourier != 0) or
 * sigma x + mu.  The projection at time level tau, z ~ N(0, I) in sample space:
 *   d  = alpha(tau) x0_obs + s(tau) G z - x ;  x' = x + dft(m . idft(sigma . d)) / sigma   (fourier == 0: x' = m ? x_obs : x)
 * i.e. A^-1(m A(x_obs) + (1 - m) A(x)) with x_obs = alpha x0_obs + s G z (mu cancels).  mask_u8: (B,T,C) when mask_per_series,
 * else one (T,C) mask for every series.  feat_std: the (T,C) feature std of the standardised spectrum, NULL = 1 (read only
 * when fourier != 0).  T <= 1024 when fourier != 0.
 *   fd_impute_project    : the projection alone (out may alias x); z == NULL -> Philox (seed; element e at offset + e/4).
 *   fd_sampler_run_impute: fd_sampler_run with a projection behind every step, the reverse step and the projection fused in one
 *                          launch: step i projects at tau = t_{i+1} (alpha, s of marginal_prob; VE alpha = 1), the last step
 *                          hard (alpha = 1, s = 0).  One score launch per step (bf16: the persistent kernel in single-step mode).
 *                          Philox (seed): predictor noise of step i at offset + i*ceil(BTC/4) + e/4 (as fd_sampler_run),
 *                          observation noise at offset + (n_steps + i)*ceil(BTC/4) + e/4.  z_steps, zobs_steps: injected
 *                          (n_steps,B,T,C) noise or NULL (slot n_steps-1 of zobs_steps is not read).  No host synchronisation
 *                          in the loop (the first call for a T builds the transform basis and waits for it).
 *   fd_sampler_run_impute_rep: the same loop over B = n * obs_replicas state rows conditioned on n observations: state row r
 *                          reads observation row r / obs_replicas of x0_obs (n,T,C), and of mask_u8 when mask_per_series, so the
 *                          replicas of an observation are never materialised (an ensemble of obs_replicas samples per series in
 *                          one launch).  The Philox layout counts state rows (ceil(BTC/4) per step with B = n * obs_replicas), so
 *                          every replica draws its own noise; z_steps / zobs_steps are (n_steps,B,T,C).  B must be a multiple of
 *                          obs_replicas.  fd_sampler_run_impute is the obs_replicas = 1 case. */
int fd_impute_project(fd_ctx* ctx, const float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                      const float* feat_std, int fourier, const float* G, float alpha, float s, const float* z, uint64_t seed,
                      uint64_t offset, float* out, int B, int T, int C, void* stream);
int fd_sampler_run_impute(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                          float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series, const float* feat_std,
                          int fourier, const float* z_steps, const float* zobs_steps, uint64_t seed, uint64_t offset, int B,
                          int mode, void* stream);
int fd_sampler_run_impute_rep(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                              float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                              const float* feat_std, int fourier, const float* z_steps, const float* zobs_steps, uint64_t seed,
                              uint64_t offset, int B, int obs_replicas, int mode, void* stream);
/* fd_sampler_run_impute_rep on a class-conditional model (fd_score_create_cond, n_classes > 0; FD_ERR_ARG otherwise) under
 * classifier-free guidance: every step follows w s(x, t, y) + (1 - w) s(x, t, null).  y: device int32[B], one label per state row
 * (n_classes = the null token), or NULL; cfg_scale = w, finite.  Labels and w outside {0, 1} (or FDIFF_CFG_FORCE_PAIR): x is
 * (2B,T,C), the state in rows [0, B); the two evaluations run as one forward on 2B rows and one kernel steps and projects on the
 * guided score and writes both halves (bit-equal on return).  Otherwise x is (B,T,C) and every step is one evaluation with y bound
 * (w = 0 or y NULL: the null token) -- at w = 1 the numbers of fd_sampler_run_impute_rep with y bound by fd_score_set_labels.
 * Philox counters, the noise tensors (n_steps,B,T,C) and the observation rows are those of fd_sampler_run_impute_rep over B rows;
 * the caller's label binding is restored on return. */
int fd_sampler_run_impute_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                              float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                              const float* feat_std, int fourier, const float* z_steps, const float* zobs_steps, uint64_t seed,
                              uint64_t offset, int B, int obs_replicas, int mode, const int32_t* y, float cfg_scale, void* stream);
/* RePaint resampling of the replacement loop (Lugmayr et al. 2022): the n_steps steps are cut into consecutive blocks [i0, i1),
 * i1 = min(i0 + jump_length, n_steps); every block is executed `resample` times before the next one starts, and between two
 * executions the state is diffused forward from level i1 back to level i0 by the transition kernel x <- a x + b G z, with (alpha, s)
 * of marginal_prob at timesteps[i] (level n_steps: the clean one, alpha = 1, s = 0), a = alpha(i0) / alpha(i1) and
 * b = sqrt(s(i0)^2 - a^2 s(i1)^2), in double on the host.  The re-noise is fused into the last step's kernel of the execution (no
 * launch and no pass over the state is added).  E = resample * n_steps score evaluations, K = (resample - 1) * ceil(n_steps /
 * jump_length) re-noises; resample = 1 is fd_sampler_run_impute_cfg for every jump_length, to the bit.
 *   fd_sampler_run_impute_repaint: the arguments of fd_sampler_run_impute_cfg and zre_steps, resample, jump_length.  y == NULL and
 *                          cfg_scale == 1: the unguided loop (fd_sampler_run_impute_rep; any model), otherwise the rules of
 *                          fd_sampler_run_impute_cfg (a paired call takes x (2B,T,C)).  Philox (seed), per = ceil(BTC/4): predictor
 *                          noise of executed step e at offset + e*per + el/4, observation noise at offset + (E + e)*per + el/4,
 *                          re-noise k at offset + (2E + k)*per + el/4.  z_steps, zobs_steps (E,B,T,C) and zre_steps (K,B,T,C): injected
 *                          noise in execution order, or NULL (each on its own).
 *   fd_impute_project_renoise: fd_impute_project followed by out <- a out + b G z_re in the same kernel (the loop's fused kernel
 *                          without the step); z_re == NULL -> Philox (seed; element e at offset_re + e/4).  a, b finite, b >= 0;
 *                          a = 1, b = 0 gives fd_impute_project to the bit. */
int fd_impute_project_renoise(fd_ctx* ctx, const float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                              const float* feat_std, int fourier, const float* G, float alpha, float s, const float* z,
                              uint64_t seed, uint64_t offset, float a, float b, const float* z_re, uint64_t offset_re, float* out,
                              int B, int T, int C, void* stream);
int fd_sampler_run_impute_repaint(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                  float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                  const float* feat_std, int fourier, const float* z_steps, const float* zobs_steps, uint64_t seed,
                                  uint64_t offset, int B, int obs_replicas, int mode, const int32_t* y, float cfg_scale,
                                  const float* zre_steps, int resample, int jump_length, void* stream);

/* Gradient-guided conditional sampling extension (NOT in the reference; diffusion posterior sampling, Chung et al. 2023, and
 * TSDiff's observation self-guidance, Kollovieh et al. 2023).  The state is never overwritten; every reverse step is nudged along
 * -grad ||r||^2 of the observation residual of Tweedie's estimate.  Per state row b and step i (t_i -> t_{i+1}), with (alpha, s)
 * the perturbation kernel at t_i, A and x0_obs as above, idft = F^T diag(1/rho) (F the packed DFT as a matrix, rho = 1 at DC and
 * Nyquist, 1/2 elsewhere) and sigma = feat_std (NULL = 1; read in both domains here):
 *   x0_hat = (x + s^2 G^2 . score) / alpha
 *   r      = m . idft(sigma . (x0_obs - x0_hat))       (fourier == 0: m . sigma . (x0_obs - x0_hat))
 *   u      = sigma . diag(1/rho) F r                    (fourier == 0: sigma . r)
 *   dx     = J^T (s^2 G^2 . u)                          (fd_score_input_vjp of the training forward, dropout 0; 0 when jacobian == 0)
 *   g      = (2 / alpha) (u + dx)                       = -grad_x ||r||^2
 *   x'     = fd_sde_apply(x, score, z) + (guidance_scale / ||r||) g      (0 where ||r|| = 0)
 * jacobian != 0: the score is the training forward's (mode FD_MODE_BF16: the bf16 training kernels where the model has them, else
 * exact f32); jacobian == 0: the sampler's forward (bf16: the persistent kernel in single-step mode) and no VJP.  Stage buffers live
 * in the context buffer of fd_likelihood_run (outside the workspace; grown on first use: synchronising).  Per-row sums in double,
 * fixed order: bit-reproducible.  T <= 1024 when fourier != 0.
 *   fd_impute_guidance       : one evaluation at (x, t): g_out (B,T,C) and rnorm2_out[b] = ||r_b||^2 (device double[B]).
 *   fd_sampler_run_impute_dps: the whole loop in place on x (B = n * obs_replicas rows; row b reads observation b / obs_replicas as
 *                              fd_sampler_run_impute_rep).  Philox (seed): predictor noise of step i at offset + i*ceil(BTC/4) + e/4
 *                              (as fd_sampler_run); z_steps: injected (n_steps,B,T,C) or NULL.  guidance_scale finite, >= 0.  No
 *                              host synchronisation in the loop. */
int fd_impute_guidance(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x, const float* x0_obs,
                       const uint8_t* mask_u8, int mask_per_series, const float* feat_std, int fourier, int jacobian, float* g_out,
                       double* rnorm2_out, int B, int obs_replicas, int mode, void* stream);
int fd_sampler_run_impute_dps(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                              float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series, const float* feat_std,
                              int fourier, float guidance_scale, int jacobian, const float* z_steps, uint64_t seed, uint64_t offset,
                              int B, int obs_replicas, int mode, void* stream);
/* Twisted sequential Monte Carlo conditioning (NOT in the reference; the Twisted Diffusion Sampler, Wu et al. 2023) around the
 * evaluation above.  A series is carried by `particles` = K adjacent state rows that read its observation in place (as obs_replicas);
 * the observation model is y = A(x_0) + obs_std eps at the observed entries.  Per row and step i, with rho_i = ||r||^2 and g_i as
 * above, n = sqrt(dt) g(t_i) G_k z the noise term of fd_sde_apply per element and S = dt g(t_i)^2 G_k^2 its variance:
 *   v_i      = obs_std^2 + twist_scale (s_i / alpha_i)^2
 *   ltw_i(x) = -rho_i(x) / (2 v_i),   h_i = g_i / (2 v_i)
 *   x_{i+1}  = fd_sde_apply(x_i, score_i, z_i) + S . h_i                  (term skipped where h == 0)
 *   c1 = sum_e n_e h_e,  c2 = sum_e S_e h_e^2                             (per row, double, fixed order)
 *   logw    += -c1 - c2 / 2 + ltw_{i+1}(x_{i+1}) - ltw_i(x_i)             (logw = ltw_0(x_0) at the prior)
 * After step N-1 the twist is the likelihood: rho_N is the residual of x_N with alpha = 1, s = 0 (no network evaluation), v_N =
 * obs_std^2.  Stage j = 0 .. N (after evaluation j, before step j; stage N is the final one), per series over its K rows, in double:
 * W = softmax(logw), a NaN or infinite logw counting as weight 0; ESS = 1 / sum W^2; if ESS < ess_threshold K (always at stage N
 * when final_resample != 0): the evidence grows by logsumexp(logw) - log K, the rows are resampled systematically from ONE uniform
 * u, a[k] = min{j : cumW[j] > (u + k) / K} clamped to K - 1, and logw = 0; else logw is kept.  Stage N resamples under
 * final_resample alone (final_resample == 0: never, the weighted rows are returned and logsumexp - log K still goes to the evidence).  A series whose rows all have weight 0 is not resampled and its evidence becomes -inf.  The
 * constant -(n_obs / 2) log(2 pi obs_std^2) of the likelihood is NOT added.  2 <= particles <= 1024, B % particles == 0,
 * obs_std > 0, 0 <= ess_threshold <= 1, twist_scale finite and >= 0 (FD_ERR_ARG otherwise, before any device work).
 *   fd_sampler_run_impute_smc: the whole loop; x (B,T,C) holds the prior sample and receives the particles of stage N (resampled
 *       under final_resample).  Philox (seed): predictor noise as fd_sampler_run_impute_dps; the uniform of (stage j, series q) is
 *       ((word >> 8) + 0.5) / 2^24 of word (j n + q) % 4 of counter offset + n_steps*ceil(BTC/4) + (j n + q) / 4, n = B / particles
 *       (behind the last predictor group).  z_steps: injected (n_steps,B,T,C) or NULL; u_stages: injected double (n_steps+1, n) or
 *       NULL.  Outputs, device, each nullable: log_evidence double (n), log_weights double (B) (0 after a final resample), ess
 *       double (n_steps+1, n), resampled uint8 (n_steps+1, n), ancestors int32 (n_steps+1, B) (index inside the series).  No host
 *       synchronisation in the loop: the decision to resample stays on the device.
 *   fd_smc_resample: one stage alone on logw (n, particles), in place, with u (n): ancestors (n, particles), ess (n), resampled (n),
 *       dlogz (n) the evidence increment (0 when nothing is added; final_stage != 0 adds it without a resample too).
 *   fd_smc_step: one proposal alone: x_out row b from row (b / particles) particles + ancestors[b] of x, score, g (ancestors NULL:
 *       the identity), h = g inv2v, noise z (B,T,C) or NULL (Philox at offset + e / 4); c1, c2 double (B).  x_out != x. */
int fd_sampler_run_impute_smc(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                              float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series, const float* feat_std,
                              int fourier, int jacobian, double obs_std, double twist_scale, double ess_threshold,
                              int final_resample, const float* z_steps, const double* u_stages, uint64_t seed, uint64_t offset, int B,
                              int particles, int mode, double* log_evidence, double* log_weights, double* ess, uint8_t* resampled,
                              int32_t* ancestors, void* stream);
int fd_smc_resample(fd_ctx* ctx, double* logw, const double* u, int n, int particles, double ess_threshold, int force,
                    int final_stage, int32_t* ancestors, double* ess, uint8_t* resampled, double* dlogz, void* stream);
int fd_smc_step(fd_ctx* ctx, const fd_sde_params* sde, const float* G, double t, float dt, const float* x, const float* score,
                const float* g, const int32_t* ancestors, const float* z, uint64_t seed, uint64_t offset, double inv2v, float* x_out,
                double* c1, double* c2, int B, int particles, int T, int C, void* stream);
/* The two above under classifier-free guidance (class-conditional models; FD_ERR_ARG otherwise), y / cfg_scale and the pairing rule
 * as fd_sampler_run_impute_cfg.  The score in x0_hat and in the step is the guided one, and
 *   dx = w J_c^T v + (1 - w) J_u^T v,  v = s^2 G^2 . u:
 * one training forward and one input VJP on 2B rows with the labels [y ; null], the VJP's input (w v ; (1 - w) v), its two output
 * halves added (conditional first).  Label dropout is off in these forwards.
 *   fd_impute_guidance_cfg       : x (B,T,C) (a paired call copies it twice into its own buffers); g_out, rnorm2_out for the B rows.
 *   fd_sampler_run_impute_dps_cfg: a paired call takes x (2B,T,C), the state in rows [0, B), and leaves both halves equal; Philox
 *                                  and z_steps (n_steps,B,T,C) as fd_sampler_run_impute_dps over B rows. */
int fd_impute_guidance_cfg(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x, const float* x0_obs,
                           const uint8_t* mask_u8, int mask_per_series, const float* feat_std, int fourier, int jacobian,
                           float* g_out, double* rnorm2_out, int B, int obs_replicas, int mode, const int32_t* y, float cfg_scale,
                           void* stream);
int fd_sampler_run_impute_dps_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                  float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                  const float* feat_std, int fourier, float guidance_scale, int jacobian, const float* z_steps,
                                  uint64_t seed, uint64_t offset, int B, int obs_replicas, int mode, const int32_t* y,
                                  float cfg_scale, void* stream);

/* Conditioning on window means (NOT in the reference): the observation is a series reported at a coarser rate than the model's.
 * window = w in [1, T], J = ceil(T / w) windows, window j = [j w, min((j + 1) w, T)) of length l_j (the last may be short); per
 * channel (P v)_j = mean of v over window j, (P^+ r)_t = r_{j(t)}, (P^T r)_t = r_{j(t)} / l_{j(t)}.  mask_u8 is (B / obs_replicas,J,C)
 * when mask_per_series, else (J,C): 1 = the mean of that window is observed.  x0_obs stays (B / obs_replicas,T,C): A^-1(P^+ where(m,
 * y, 0)) for the window means y (J,C).  Replacement, d as above:
 *   x' = x + dft(P^+ (m . P idft(sigma . d))) / sigma      (fourier == 0: x' = x + P^+ (m . P (sigma . d)) / sigma)
 * guidance: r = m . P idft(sigma . (x0_obs - x0_hat)) (J,C), u = sigma . diag(1/rho) F P^T r (fourier == 0: P in the place of P idft,
 * u = sigma . P^T r); everything else as in the entries they extend.  feat_std is read in BOTH domains (sigma varies inside a window).
 * window == 1 forwards to the entry without the argument (bit-identical); window < 1 or > T: FD_ERR_ARG; window > 1 needs T <= 1024
 * in both domains.  No labels, no classifier-free guidance and no RePaint.  The first call for a (T, window) builds two rectangular
 * bases (Jp x Tp and Tp x Jp floats, Jp = 16 ceil(J/16)) and waits for them.  Philox layouts, noise tensors and obs_replicas as
 * fd_impute_project, fd_sampler_run_impute_rep, fd_impute_guidance and fd_sampler_run_impute_dps. */
int fd_impute_project_agg(fd_ctx* ctx, const float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                          const float* feat_std, int fourier, const float* G, float alpha, float s, const float* z, uint64_t seed,
                          uint64_t offset, float* out, int B, int T, int C, int window, void* stream);
int fd_sampler_run_impute_agg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                              float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                              const float* feat_std, int fourier, const float* z_steps, const float* zobs_steps, uint64_t seed,
                              uint64_t offset, int B, int obs_replicas, int window, int mode, void* stream);
int fd_impute_guidance_agg(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x, const float* x0_obs,
                           const uint8_t* mask_u8, int mask_per_series, const float* feat_std, int fourier, int jacobian,
                           float* g_out, double* rnorm2_out, int B, int obs_replicas, int window, int mode, void* stream);
int fd_sampler_run_impute_dps_agg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                  float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                  const float* feat_std, int fourier, float guidance_scale, int jacobian, const float* z_steps,
                                  uint64_t seed, uint64_t offset, int B, int obs_replicas, int window, int mode, void* stream);

/* Conditioning on a dense linear observation (NOT in the reference; replaces nothing in it): per channel y = P v for a matrix P
 * (M x T) of full row rank that the caller supplies, shared by all series and channels, T the model's max_len, 1 <= M <= T <= 1024
 * -- a band-limited recording, a moving average with overlapping windows, a blur, increments.  The window means above are one such P.
 * The formulas are those of the window-mean entries with P, P^+ = pinv(P) and P^T general:
 *   x' = x + dft(P^+ (m . P idft(sigma . d))) / sigma      (fourier == 0: x' = x + P^+ (m . P (sigma . d)) / sigma)
 *   r = m . P idft(sigma . (x0_obs - x0_hat)) (M,C), u = sigma . diag(1/rho) F P^T r      (fourier == 0: P for P idft, u = sigma . P^T r)
 * mask_u8 is (B / obs_replicas,M,C) when mask_per_series, else (M,C): 1 = row j of P is observed for that channel; x0_obs stays
 * (B / obs_replicas,T,C): A^-1(P^+ where(m, y, 0)).  The replacement is the orthogonal projection onto {x : m . P A(x) = m . y} only when the
 * rows of P are mutually orthogonal or every (series, channel) column of the mask is all 1 or all 0: the caller checks that, and the
 * rank and conditioning of P (the f32 bases lose about cond(P) 2^-24 relative accuracy); the engine does not.  feat_std is read in
 * BOTH domains.  No labels, no classifier-free guidance and no RePaint.
 *
 * fd_linop_create   (NOT in the reference; replaces nothing in it) the handle of one operator: P (M,T) and Pplus (T,M), row-major
 *                   doubles on the HOST, copied to the device before the call returns.  FD_ERR_ARG: null pointer, M < 1, M > T or
 *                   T > 1024.  The first call of an entry below for a (handle, domain) builds three f32 bases on the device in
 *                   double (Mp x Tp, Tp x Mp and Tp x Mp floats, Mp = 16 ceil(M/16)) and waits for them; they belong to the handle.
 * fd_linop_destroy  (NOT in the reference; replaces nothing in it) frees the handle and its device tables; the caller keeps it alive
 *                   until the work that reads it was enqueued, and destroys it before its context.  NULL is allowed.
 * fd_impute_project_op, fd_sampler_run_impute_op, fd_impute_guidance_op, fd_sampler_run_impute_dps_op
 *                   (NOT in the reference; replace nothing in it) fd_impute_project_agg, fd_sampler_run_impute_agg,
 *                   fd_impute_guidance_agg and fd_sampler_run_impute_dps_agg with the handle in the place of `window`: Philox layouts,
 *                   noise tensors and obs_replicas as there.  FD_ERR_ARG: a null handle, a handle of another context, one whose T is
 *                   not the call's, or M > T. */
typedef struct fd_linop fd_linop;
int fd_linop_create(fd_ctx* ctx, int T, int M, const double* P, const double* Pplus, fd_linop** out);
int fd_linop_destroy(fd_linop* op);
int fd_impute_project_op(fd_ctx* ctx, const float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                         const float* feat_std, int fourier, const float* G, float alpha, float s, const float* z, uint64_t seed,
                         uint64_t offset, float* out, int B, int T, int C, fd_linop* op, void* stream);
int fd_sampler_run_impute_op(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                             float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                             const float* feat_std, int fourier, const float* z_steps, const float* zobs_steps, uint64_t seed,
                             uint64_t offset, int B, int obs_replicas, fd_linop* op, int mode, void* stream);
int fd_impute_guidance_op(fd_score* m, const fd_sde_params* sde, const float* G, float t, const float* x, const float* x0_obs,
                          const uint8_t* mask_u8, int mask_per_series, const float* feat_std, int fourier, int jacobian,
                          float* g_out, double* rnorm2_out, int B, int obs_replicas, fd_linop* op, int mode, void* stream);
int fd_sampler_run_impute_dps_op(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                                 float dt, float* x, const float* x0_obs, const uint8_t* mask_u8, int mask_per_series,
                                 const float* feat_std, int fourier, float guidance_scale, int jacobian, const float* z_steps,
                                 uint64_t seed, uint64_t offset, int B, int obs_replicas, fd_linop* op, int mode, void* stream);

/* Probability-flow ODE extension (NOT in the reference, whose only sampler is Euler-Maruyama over the reverse SDE; Song et al. 2021,
 * Sec. 4.3): the deterministic ODE with the reverse SDE's marginals.  With a = a_x(t), g = g(t) of the SDE (VP: a = beta/2,
 * g = sqrt(beta); VE: a = 0, g = sigma_min sqrt(2 ln(sigma_max/sigma_min)) (sigma_max/sigma_min)^t) and s the score:
 *   v(x, t) = -a x - 0.5 (g G_k)^2 s(x, t)          (fd_sde_step's drift with the score term halved)
 * On a strictly monotone grid t_0 .. t_N, h_i = t_{i+1} - t_i (h < 0: noise -> data, sampling / decoding; h > 0: data -> noise,
 * encoding):
 *   Euler (solver 0): x_{i+1} = x_i + h_i v(x_i, t_i)                                               N score evaluations
 *   Heun  (solver 1): x~ = x_i + h_i v_i, v_i = v(x_i, t_i);  x_{i+1} = x_i + h_i/2 (v_i + v(x~, t_{i+1}))    2N evaluations
 * (the last step is corrected too).  No random numbers are drawn.
 *   fd_pf_ode_drift   : v_out = v(x, t) for the given score (out may alias x or score).  The step-wise building block.
 *   fd_sampler_run_ode: the whole Euler / Heun loop in place on x (B,T,C).  timesteps: HOST float[n_steps + 1], strictly monotone
 *                       and finite (FD_ERR_ARG otherwise).  Same dispatch as fd_sampler_run (bf16 transformer: the persistent
 *                       kernel, then the long-series fused launch, then per-op launches; FDIFF_SAMPLER_STEPWISE and
 *                       FDIFF_SAMPLER_UNFUSED_STEP select the later forms); no host synchronisation inside the loop. */
int fd_pf_ode_drift(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* x, const float* score, double t,
                    float* v_out, int B, int T, int C, void* stream);
int fd_sampler_run_ode(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, int solver,
                       float* x, int B, int mode, void* stream);

/* Data-prediction exponential integrators for the same ODE (NOT in the reference; DPM-Solver++, Lu et al. 2022, in its multistep
 * second-order form "2M", and its first order, deterministic DDIM, Song et al. 2021a).  With (alpha, s) the perturbation kernel
 * x_t = alpha x_0 + s G z, lambda = log(alpha / s) and h_i = lambda(t_{i+1}) - lambda(t_i) > 0 on a grid t_0 > ... > t_N:
 *   D_i     = (x_i + (s_i G_k)^2 score(x_i, t_i)) / alpha_i                                  Tweedie's estimate of x_0
 *   Dbar    = D_i  (solver 2: DDIM; solver 3: i = 0)   or   (1 + h_i / (2 h_{i-1})) D_i - h_i / (2 h_{i-1}) D_{i-1}  (solver 3: 2M)
 *   x_{i+1} = (s_{i+1} / s_i) x_i - alpha_{i+1} expm1(-h_i) Dbar
 * One score evaluation per step; the coefficients are computed on the host in double.  G_k cancels from every ratio.
 *   fd_sampler_run_dpm: the whole loop in place on x (B,T,C), arguments and dispatch as fd_sampler_run_ode.  timesteps: HOST
 *                       float[n_steps + 1], finite, strictly DECREASING, with lambda strictly increasing (FD_ERR_ARG otherwise).
 *                       solver: 2 or 3 (FD_ERR_ARG otherwise; fd_sampler_run_ode keeps 0 and 1).
 *   fd_dpm_stage      : one step t -> t_next on given x and score: x_out = x_{i+1}, d_out = D_i.  d_prev == NULL: first order;
 *                       else D_{i-1}, evaluated at t_prev > t (2M).  x_out may alias x, d_out may alias d_prev; no other aliasing.
 *                       The step-wise building block (the times are rounded to float first, as the loop's grid is). */
int fd_sampler_run_dpm(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, int solver,
                       float* x, int B, int mode, void* stream);
int fd_dpm_stage(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* x, const float* score, const float* d_prev,
                 double t_prev, double t, double t_next, float* x_out, float* d_out, int B, int T, int C, void* stream);

/* Classifier-free guidance (NOT in the reference; Ho & Salimans 2022) on a class-conditional model: every loop above with the score
 *   s = w s(x, t, y) + (1 - w) s(x, t, null)        (the two products as written: w = 1 is s(x, t, y), w = 0 is s(x, t, null), exactly)
 * y: device int32[B] labels or NULL.  w == 1: one evaluation per step with y bound; w == 0 or y == NULL: one evaluation with the
 * null token; x is (B,T,C) then and the loop is fd_sampler_run's / fd_sampler_run_ode's step-wise form.  Otherwise the two
 * evaluations of a step run as ONE forward on 2B rows and x is a (2B,T,C) buffer: rows [0, B) in/out, rows [B, 2B) the same state
 * evaluated with the null token (overwritten on entry and by every step).  One fused kernel per step reads x and both scores and
 * writes the new state to both halves.
 *   fd_sampler_run_cfg    : the reverse-SDE loop; timesteps, dt, z_steps (n_steps,B,T,C) and the Philox counters (n = B T C elements
 *                           per step) as fd_sampler_run.
 *   fd_sampler_run_ode_cfg: solver 0 Euler, 1 Heun (grid as fd_sampler_run_ode), 2 DDIM, 3 DPM-Solver++ 2M (grid as fd_sampler_run_dpm).
 * FD_ERR_ARG on an unlabelled model.  No host synchronisation inside the loops. */
int fd_sampler_run_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt, float* x,
                       const int32_t* y, float w, const float* z_steps, uint64_t seed, uint64_t offset, int B, int mode, void* stream);
int fd_sampler_run_ode_cfg(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, int solver,
                           float* x, const int32_t* y, float w, int B, int mode, void* stream);

/* The same two loops on a covariate-conditional model (an extension, not in the reference): c device float (B, P) covariates or NULL,
 * the score w s(x, t, c) + (1 - w) s(x, t, null).  w == 1: one evaluation per step with c bound; w == 0 or c == NULL: one evaluation
 * on the null vector, x (B,T,C); otherwise one forward on 2B rows (the covariates twice, the second half reading the null vector), x
 * a (2B,T,C) buffer, and the fused step kernels of the class-guided loops.  FD_ERR_ARG on a model without covariates. */
int fd_sampler_run_cov(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt, float* x,
                       const float* c, float w, const float* z_steps, uint64_t seed, uint64_t offset, int B, int mode, void* stream);
int fd_sampler_run_ode_cov(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, int solver,
                           float* x, const float* c, float w, int B, int mode, void* stream);

/* Adaptive ODE sampling, encoding and decoding (NOT in the reference; Song et al. 2021's black-box RK45 sampler):
 *   fd_sampler_run_ode_adaptive: integrates every row of x (B,T,C) in place from t0 to t1 (finite, t0 != t1: t0 > t1 samples /
 *                      decodes, t0 < t1 encodes; FD_ERR_ARG otherwise) by Dormand-Prince 5(4) with the step control of
 *                      scipy.integrate.RK45 as fd_likelihood_run_adaptive below states it, with scipy's `direction`: t_new = t +
 *                      direction h_abs, clamped when direction (t_new - t1) > 0, min_step = 10 |nextafter(t, direction inf) - t|.
 *                      The state is the T*C values alone (RMS error norm over them).  Each row has its own grid; a row that stops
 *                      early keeps its last accepted state.  Device outputs: nfe_out[b] scipy's nfev (2 + 6 per attempted step),
 *                      status_out[b] 1 converged, 2 step under min_step, 3 the next attempt would pass max_evals (>= 8); grid_out
 *                      (nullable) (B, grid_cap) doubles: the accepted times, t0 first, NaN-padded, grid_cap >= 1 + (max_evals - 2)
 *                      / 6.  rtol, atol > 0.  Every evaluation is the sampler's forward (mode: FD_MODE_F32 exact, FD_MODE_BF16 the
 *                      per-layer bf16 kernels) + one stage kernel; controller float64 per row, x and the stage vectors fp32;
 *                      fixed-order reductions: bit-reproducible.
 *                      Compaction: the forward runs on the rows still running once the count the host has read (one attempt late)
 *                      is below the launched rows by compact_granule rows; compact_granule 0: FDIFF_RK_COMPACT_GRANULE, else the
 *                      library's default (1 for the transformer in FD_MODE_F32, else off: measured); FDIFF_RK_COMPACT=0 keeps
 *                      every launch at B rows.  Which evaluations a row sees does not depend on it (the bf16 kernels round a row
 *                      differently at a different row count, as for any change of B).  *row_evals_out (HOST, nullable): the
 *                      state rows launched, summed over the evaluations.
 *                      The state lives in a context-owned buffer outside the workspace (grown on first use: synchronising).
 *                      SYNCHRONISES the stream once per attempted step, as fd_likelihood_run_adaptive.
 *   fd_sampler_run_ode_adaptive_cfg / _cov: the same under classifier-free guidance, y / c and w as fd_sampler_run_ode_cfg / _cov.
 *                      x stays (B,T,C) in every form: the pair form runs one forward on 2B rows of the loop's own input buffer and
 *                      the stage kernel combines the two halves of the score.  Guided loops run uncompacted (so does the plain
 *                      entry point when labels or covariates are bound to the model); row_evals_out counts state rows, each of
 *                      which is two network rows in the pair form. */
int fd_sampler_run_ode_adaptive(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol, double atol,
                                int max_evals, float* x, int* nfe_out, int* status_out, double* grid_out, int grid_cap,
                                int compact_granule, long long* row_evals_out, int B, int mode, void* stream);
int fd_sampler_run_ode_adaptive_cfg(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol,
                                    double atol, int max_evals, float* x, const int32_t* y, float w, int* nfe_out, int* status_out,
                                    double* grid_out, int grid_cap, long long* row_evals_out, int B, int mode, void* stream);
int fd_sampler_run_ode_adaptive_cov(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol,
                                    double atol, int max_evals, float* x, const float* c, float w, int* nfe_out, int* status_out,
                                    double* grid_out, int grid_cap, long long* row_evals_out, int B, int mode, void* stream);

/* Likelihood extension (NOT in the reference; Song et al. 2021, Sec. 4.3 and App. D.2): the exact log-density of the
 * probability-flow ODE above,
 *   log p_0(x_0) = log p_1(x_1) + int_eps^1 div v(x(t), t) dt,   div v = -a T C - 0.5 g^2 tr(diag(G_k^2) ds/dx)
 * with the trace estimated per row b as e_b^T diag(G_k^2) (ds/dx) e_b for a probe e_b (Hutchinson; the basis vectors give it exactly).
 *   fd_prior_logp    : out[b] = sum_{t,c} log N(x_btc; 0, (sigma_p G_t)^2), sigma_p = 1 (VP) or sigma_max (VE): the density of
 *                      fd_prior_sample.  out: device float[B].
 *   fd_likelihood_run: integrates the ODE in place on x (B,T,C) from data to latents over the HOST grid timesteps[0 .. n_steps]
 *                      (strictly increasing, finite; FD_ERR_ARG otherwise) by Euler or Heun exactly as fd_sampler_run_ode, and
 *                      writes score_div[b] = sum_i w_i (-0.5 g(t_i)^2) <(ds/dx)^T (G^2 e_b), e_b> over the same quadrature (Heun:
 *                      the trapezoid of its two stages).  probes: device (B,T,C), e_b per row (replicate a series over rows for
 *                      several probes).  The drift part of the divergence, -T C sum_i w_i a(t_i), is the caller's (host, float64).
 *                      Each evaluation is fd_score_forward_train (dropout 0) + fd_score_input_vjp + one fused stage kernel; mode
 *                      FD_MODE_BF16 runs the bf16 training kernels where the model has them (else exact f32).  Per-row sums in
 *                      float64, fixed order: bit-reproducible.  The stage state lives in a context-owned buffer outside the
 *                      workspace (grown on first use: synchronising).  No host synchronisation inside the loop. */
int fd_prior_logp(fd_ctx* ctx, const fd_sde_params* sde, const float* G, const float* x, float* out, int B, int T, int C, void* stream);
int fd_likelihood_run(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, int solver,
                      float* x, const float* probes, float* score_div, int B, int mode, void* stream);
/*   fd_likelihood_run_adaptive: the same integral with adaptive steps: every row b is one ODE on y_b = [x_b, acc_b] from t0 to t1
 *                      (finite, t0 < t1), dacc/dt = div v (drift part included), integrated by Dormand-Prince 5(4) with the step
 *                      control of scipy.integrate.RK45 (select_initial_step, min_step = 10 ulp(t), RMS error norm over the T*C + 1
 *                      components with scale atol + rtol max(|y|, |y_new|), SAFETY 0.9, factors in [0.2, 10]).  Each row has its
 *                      own grid.  x is integrated in place to the latents (a row that stops early keeps its last accepted state);
 *                      device outputs: div_out[b] (double) the whole divergence integral, nfe_out[b] scipy's nfev (2 + 6 per
 *                      attempted step), status_out[b] 1 converged, 2 step under min_step, 3 the next attempt would pass
 *                      max_evals (>= 8); grid_out (nullable) (B, grid_cap) doubles: the accepted times, t0 first, NaN-padded,
 *                      grid_cap >= 1 + (max_evals - 2) / 6.  rtol, atol > 0.  Evaluations and precision as fd_likelihood_run;
 *                      controller state float64 per row, x and the stage vectors fp32; fixed-order reductions: bit-reproducible,
 *                      and a row's result does not depend on the other rows of the launch.  SYNCHRONISES the stream once per
 *                      attempted step (the running-row count of attempt k is read while attempt k + 1 is queued). */
int fd_likelihood_run_adaptive(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol, double atol,
                               int max_evals, float* x, const float* probes, double* div_out, int* nfe_out, int* status_out,
                               double* grid_out, int grid_cap, int B, int mode, void* stream);

/* ------------------------------------------------------------ a11 optimiser
 * torch.optim.AdamW defaults + diffusers cosine-warmup + Lightning global-norm clip
 * (score_models.py:122-130, cmd/conf/trainer/default.yaml:4), fused over the flat buffer.
 * fd_grad_sqnorm: norm2_out[0] = sum(grads^2) (device float[1], fp32 accumulated in fp64 blocks).
 * fd_adamw_step : clip_coef is read from device: coef = min(1, max_norm/(sqrt(*sqnorm)+1e-6))
 *                 when sqnorm != NULL, else 1.  frozen [frozen_begin, frozen_end) is skipped.
 *                 The whole update is skipped ON THE DEVICE (parameters and moments unchanged) when a bounded wait of the
 *                 training step whose gradients these are timed out (see fd_ctx_check): the host only reports it, one call later. */
int fd_grad_sqnorm(fd_ctx* ctx, const float* grads, int64_t n, float* sqnorm_out, void* stream);
int fd_adamw_step(fd_ctx* ctx, float* params, const float* grads, float* exp_avg,
                  float* exp_avg_sq, int64_t n, int step, float lr, float beta1, float beta2,
                  float eps, float weight_decay, const float* sqnorm, float max_norm,
                  float grad_scale, int64_t frozen_begin, int64_t frozen_end, void* stream);
/* fd_adamw_ema_step: fd_adamw_step of the a11 row plus an exponential moving average of the weights in the same pass (an extension,
 *                 NOT in the reference: the ExponentialMovingAverage score-SDE code bases train with).  params, exp_avg and
 *                 exp_avg_sq come out bit-identical to fd_adamw_step on the same inputs; with p' the updated parameter,
 *                 ema[i] = fmaf(ema_decay, ema[i], (1 - ema_decay) * p'[i]), 0 <= ema_decay <= 1 (0: ema == p' bit for bit,
 *                 1: ema untouched).  ema: device float[n], same layout as params.  The frozen range and the on-device skip
 *                 leave ema untouched together with params and the moments.  36 B/param of traffic instead of 28. */
int fd_adamw_ema_step(fd_ctx* ctx, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                      float* ema, float ema_decay,
                      int64_t n, int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                      const float* sqnorm, float max_norm, float grad_scale,
                      int64_t frozen_begin, int64_t frozen_end, void* stream);

/* ----------------------------------------------------- (e) multi-GPU exchange
 * Data-parallel gradient all-reduce over RCCL/xGMI on ONE flat fp32 buffer.
 * unique_id: host bytes from fd_comm_unique_id on rank 0, broadcast by the launcher. */
#define FD_COMM_ID_BYTES 128
int fd_comm_unique_id(void* id_out /* host, FD_COMM_ID_BYTES */);
int fd_comm_init(fd_ctx* ctx, int rank, int nranks, const void* unique_id);
int fd_comm_destroy(fd_ctx* ctx);
/* path of the shared object the bound ncclAllReduce lives in (one RCCL image per process: an already mapped librccl --
 * torch's bundled one under the Python host -- is reused, never a second copy).  buf: host, n bytes. */
int fd_comm_rccl_path(char* buf, int n);
/* buf = sum over ranks (buf) * scale, in place */
int fd_allreduce_grads(fd_ctx* ctx, float* buf, int64_t n, float scale, void* stream);

/* ------------------------------------------- (f)3 evaluation metrics on the GPU
 * Sliced / marginal Wasserstein-2 between two sample sets (fdiff.sampling.metrics.SlicedWasserstein / MarginalWasserstein,
 * src/fdiff/sampling/metrics.py:100-217, over fdiff.utils.wasserstein.WassersteinDistances, src/fdiff/utils/wasserstein.py:95-199).
 * The host draws the directions exactly as the reference does (numpy Generator) and composes:
 *   fd_project_rows    out (K, n) = dirs (K, d) . x (n, d)^T      replaces WassersteinDistances._project  (wasserstein.py:150-153)
 *   fd_transpose_rows  out (d, n) = x (n, d)^T                    the marginal "directions" (standard basis, wasserstein.py:77-89)
 *   fd_sort_rows       every row of (K, n) sorted ascending; temp = fd_sort_rows_temp_bytes(K, n) caller-owned device bytes
 *   fd_w2_sorted_rows  out[k] = W2 between sorted row k of a (K, n) and of b (K, m), uniform weights, any n, m: the exact 1-D
 *                      transport POT's emd2_1d solves, then sqrt               (wasserstein.py:112-113, 139-141)            */
int fd_project_rows(fd_ctx* ctx, const float* x, const float* dirs, float* out, int n, int d, int K, void* stream);
int fd_transpose_rows(fd_ctx* ctx, const float* x, float* out, int n, int d, void* stream);
int fd_sort_rows_temp_bytes(fd_ctx* ctx, int K, int n, size_t* bytes);
int fd_sort_rows(fd_ctx* ctx, const float* in, float* out, int K, int n, void* temp, size_t temp_bytes, void* stream);
int fd_w2_sorted_rows(fd_ctx* ctx, const float* a, const float* b, float* out, int K, int n, int m, void* stream);

/* Ensemble scores of probabilistic imputation / forecasting (NOT in the reference; CSDI, TimeGrad, TSDiff report them): samples
 * (n, K, T, C) fp32 in data scale and the time domain, truth (n, T, C).  For every entry e = (series, t, c), x_1 .. x_K its
 * ensemble and y its truth:
 *   out_crps[e]         (1/K) sum_k |x_k - y| - (1/(2K^2)) sum_{j,k} |x_j - x_k|   (properscoring.crps_ensemble, fair = False)
 *   out_quantiles[q, e] sample quantile at levels[q] in [0, 1], linear between order statistics at position levels[q] (K - 1)
 *                       (numpy.quantile / torch.quantile "linear"); (n_levels, n, T, C)
 *   out_mean[e]         (1/K) sum_k x_k
 * 1 <= K <= 1024.  levels: device double[n_levels]; any output may be NULL (out_quantiles only when n_levels == 0).  A NaN sample
 * or truth makes that entry's outputs NaN and no other.  One workgroup sorts a tile of entries in LDS (bitonic), sums in double;
 * deterministic. */
int fd_ensemble_scores(fd_ctx* ctx, const float* samples, const float* truth, int n, int K, int T, int C, const double* levels,
                       int n_levels, float* out_crps, float* out_quantiles, float* out_mean, void* stream);

/* Nearest-neighbour primitives of the sample-space metrics (NOT in the reference: improved precision / recall, density / coverage,
 * authenticity and the train-versus-held-out nearest-neighbour share are built on them in sampling/metrics.py).  q (n, d) and
 * r (m, d) are dense row-major fp32 device arrays with finite entries; distances are SQUARED Euclidean.
 *   fd_knn_rows     for every query row the k nearest reference rows: dist2 (n, k) and idx (n, k), each row ascending in
 *                   (distance, index), no index repeated.  1 <= k <= 16 and k <= m - exclude_self.  exclude_self = 1 needs q == r
 *                   and n == m and never returns j == i (the k-NN radii of a set in itself).  Selection runs on the fp32-MFMA
 *                   expansion ||q||^2 + ||r||^2 - 2 q.r of both sets centred by the column mean of r (double, fixed order), the
 *                   n x m matrix never exists; the k selected pairs are then recomputed as sum (q - r)^2 (f32 differences, double
 *                   sum in ascending feature order) and re-sorted.  So a returned distance is the distance of the returned index
 *                   to f32 rounding, a bit-copy of a reference row returns that row at rank 0 with distance exactly 0, and a row
 *                   can lose its place to another only when their distances differ by less than the expansion's error,
 *                   2 (d + 3) 2^-24 (||q - mean||^2 + ||r - mean||^2).  Ties go to the lower index.  work: caller-owned device
 *                   bytes, at least fd_knn_rows_workspace_bytes(n, m, d, k).  Deterministic, independent of how the reference
 *                   rows are split over workgroups (the environment variable FDIFF_KNN_SPLITS forces a split count, read by
 *                   both calls).
 *   fd_ball_counts  counts[i] = #{ j : d2(q_i, r_j) <= radius2[j] }, radius2 (m) device fp32, on the same centred expansion
 *                   (so a pair within that error of its radius may fall on either side); scratch from the context's arena.  No
 *                   atomics: two runs are bit-identical.
 * FD_ERR_ARG: null pointer, a shape < 1, k out of range, exclude_self with q != r or n != m, a workspace that is too small,
 * n * k, n * d or m * d >= 2^31. */
int fd_knn_rows_workspace_bytes(fd_ctx* ctx, int n, int m, int d, int k, size_t* bytes);
int fd_knn_rows(fd_ctx* ctx, const float* q, int n, const float* r, int m, int d, int k, int exclude_self, float* dist2 /* (n, k) */,
                int32_t* idx /* (n, k) */, void* work, size_t work_bytes, void* stream);
int fd_ball_counts(fd_ctx* ctx, const float* q, int n, const float* r, int m, int d, const float* radius2 /* (m) */,
                   int32_t* counts /* (n) */, void* stream);

/* Dynamic time warping under a Sakoe-Chiba band, and the nearest-neighbour primitives under it (NOT in the reference; the
 * time-warp-aware twins of fd_knn_rows / fd_ball_counts: DTWPrecisionRecall and DTWMemorisation in sampling/metrics.py are built on
 * them).  Series a, b of shape (T, C), row-major as samples are stored, equal lengths, window w in [0, T - 1]:
 *   c(i, j) = sum_c (a[i, c] - b[j, c])^2          D(0, 0) = c(0, 0)
 *   D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1))   for |i - j| <= w, absent neighbours = +inf
 *   dtw2(a, b; w) = D(T-1, T-1)                    (w = 0: squared Euclidean distance; w = T - 1: unconstrained; all channels warp
 *                                                   together, "dependent" DTW)
 * q (n, T, C) and r (m, T, C) are dense fp32 device arrays with finite entries; every distance is the SQUARED dtw2.
 *   fd_dtw_pairs        dist2[i] = dtw2(a_i, b_i), a and b both (n, T, C); scratch from the context's arena.
 *   fd_dtw_knn          for every query the k nearest reference series: dist2 (n, k) and idx (n, k), each row ascending in
 *                       (distance, index), no index repeated.  1 <= k <= 16 and k <= m - exclude_self.  exclude_self = 1 needs
 *                       q == r and n == m and never returns j == i.  Ties go to the lower index.
 *   fd_dtw_ball_counts  counts[i] = #{ j : dtw2(q_i, r_j) <= radius2[j] }, radius2 (m) device fp32.
 * One kernel serves all three (csrc/fd_dtw.hip): a (query, reference) pair per lane, the references read from an image transposed
 * once into [tile of 64][t][c][lane], the query wave-uniform; the band is walked in blocks of 8 query rows held in registers, the
 * row a block hands to the next lives in the LDS (min(T, 2 w + 8) words per lane); the n x m matrix never exists.  A cell is
 *   D = fma(d_{C-1}, d_{C-1}, m + P),  m = the min of the three predecessors, d_c = a[i, c] - b[j, c] in fp32,
 *   P = fma(d_{C-2}, d_{C-2}, ... fma(d_0, d_0, 0))  (C = 1: D = fma(d_0, d_0, m)),
 * a pure function of the inputs: a value does not depend on the entry point, on the tiling or on the split, dtw2(a, b) ==
 * dtw2(b, a) bit for bit, the distance fd_dtw_knn returns is bit for bit fd_dtw_pairs of the returned pair, and a bit-copy of a
 * reference row returns that row at distance exactly 0.  All terms are non-negative and min is exact and monotone, so with D the
 * float64 value |computed - D| <= 1.01 (C + 2) (2 T - 1) 2^-24 D: selection may exchange two references whose dtw2 differ by less
 * than twice that, and a pair within it of its radius may be counted or not.
 * Limits: 1 <= T <= 1024, C >= 1, a stored band column min(2 w + 1, T) <= 256; n * T * C, m * T * C and n * k below 2^31.
 * work: caller-owned device bytes, at least the matching _workspace_bytes of the same shape (the image, and the per-split partial
 * lists or counts).  The reference tiles are split over workgroups when the queries alone do not fill the device; partial lists
 * are merged on (distance, index), partial counts are added in split order, no atomics: results are bit-identical between runs and
 * for every split (the environment variable FDIFF_DTW_SPLITS forces a split count, read by the _workspace_bytes calls too).
 * FD_ERR_ARG: null pointer, a shape < 1 or T > 1024, window outside [0, T - 1] or with a band column above 256, k out of range,
 * exclude_self with q != r or n != m, a workspace that is too small, n * T * C, m * T * C or n * k >= 2^31. */
int fd_dtw_pairs(fd_ctx* ctx, const float* a, const float* b, int n, int T, int C, int window, float* dist2 /* (n) */, void* stream);
int fd_dtw_knn_workspace_bytes(fd_ctx* ctx, int n, int m, int T, int C, int window, int k, size_t* bytes);
int fd_dtw_knn(fd_ctx* ctx, const float* q, int n, const float* r, int m, int T, int C, int window, int k, int exclude_self,
               float* dist2 /* (n, k) */, int32_t* idx /* (n, k) */, void* work, size_t work_bytes, void* stream);
int fd_dtw_ball_counts_workspace_bytes(fd_ctx* ctx, int n, int m, int T, int C, int window, size_t* bytes);
int fd_dtw_ball_counts(fd_ctx* ctx, const float* q, int n, const float* r, int m, int T, int C, int window,
                       const float* radius2 /* (m) */, int32_t* counts /* (n) */, void* work, size_t work_bytes, void* stream);

/* Multivariate scores of a sample ensemble, per series (NOT in the reference; Gneiting and Raftery 2007, Scheuerer and Hamill
 * 2015): the per-entry scores of fd_ensemble_scores cannot tell a coherent ensemble from one whose members were permuted
 * independently at every entry, these can.  samples (n, K, T, C) fp32, truth (n, T, C), 1 <= K <= 1024; mask_u8 as in
 * fd_impute_*: 1 = observed, (n, T, C) when mask_per_series, else one (T, C) mask.  H: the hidden entries of a series (mask 0).
 *   fd_energy_score     out_score[s] = (1/K) sum_k ||x_k - y||_H - 1/(2 K^2) sum_{j,k} ||x_j - x_k||_H, Euclidean norms over H;
 *                       fair != 0: 1/(2 K (K - 1)) in the second term, needs K >= 2.  NaN when H is empty.  out_hidden[s] = |H|.
 *   fd_variogram_score  out_num[s] = sum_{a<b in H} w_ab (|y_a - y_b|^p - (1/K) sum_k |x_ka - x_kb|^p)^2, out_den[s] = sum w_ab,
 *                       over the pairs of hidden entries a = (t_a, c_a), b = (t_b, c_b) (every channel pair) with
 *                       |t_a - t_b| <= max_lag (max_lag < 0: no limit); p = 0.5, 1, 2 for order = FD_VARIOGRAM_HALF, _ONE, _TWO;
 *                       w_ab = 1 / (1 + |t_a - t_b|) when inverse_lag, else 1.  The score is num / den.  A series with no such
 *                       pair: num NaN, den 0.  out_hidden (n) may be NULL.
 *   fd_ensemble_ranks   below[e] = #{k : x_k < y}, equal[e] = #{k : x_k == y}, int32 (n, T, C), for EVERY entry (no mask); an
 *                       entry with a NaN sample or truth gets -1 in both.
 * Observed entries are skipped by select: whatever they hold, NaN included, has no effect.  A NaN at a hidden entry, in the truth
 * or in any member, makes out_score / out_num of that series NaN and leaves the other series alone (out_den depends on the mask
 * only).  One tile kernel serves both scores (csrc/fd_multivariate.hip): differences in fp32 (never the Gram expansion), at most
 * 64 terms summed in fp32, then double; one partial per 64 x 64 tile of row pairs in work, added per series in fixed order by a
 * second kernel.  No atomics: two runs are bit-identical, and a series' outputs do not depend on n or on its position.  work:
 * caller-owned device bytes, at least *_workspace_bytes of the same shape (and max_lag).
 * FD_ERR_ARG: null pointer, a shape < 1, K outside [1, 1024], fair with K = 1, an unknown order, a workspace that is too small,
 * T*C or n times the tiles of a series >= 2^31 (fd_ensemble_ranks: n > 65535). */
enum { FD_VARIOGRAM_HALF = 0, FD_VARIOGRAM_ONE = 1, FD_VARIOGRAM_TWO = 2 };
int fd_energy_score_workspace_bytes(fd_ctx* ctx, int n, int K, int T, int C, size_t* bytes);
int fd_energy_score(fd_ctx* ctx, const float* samples, const float* truth, const uint8_t* mask_u8, int mask_per_series, int n, int K,
                    int T, int C, int fair, double* out_score /* (n) */, int32_t* out_hidden /* (n) */, void* work,
                    size_t work_bytes, void* stream);
int fd_variogram_score_workspace_bytes(fd_ctx* ctx, int n, int K, int T, int C, int max_lag, size_t* bytes);
int fd_variogram_score(fd_ctx* ctx, const float* samples, const float* truth, const uint8_t* mask_u8, int mask_per_series, int n,
                       int K, int T, int C, int order, int max_lag, int inverse_lag, double* out_num /* (n) */,
                       double* out_den /* (n) */, int32_t* out_hidden /* (n) or NULL */, void* work, size_t work_bytes,
                       void* stream);
int fd_ensemble_ranks(fd_ctx* ctx, const float* samples, const float* truth, int n, int K, int T, int C, int32_t* below,
                      int32_t* equal, void* stream);

/* Multivariate rank histograms of a sample ensemble, per series (NOT in the reference; Gneiting et al. 2008, Thorarinsdottir,
 * Scheuerer and Heinz 2016, Smith and Hansen 2004 / Wilks 2004): the ranks of fd_ensemble_ranks are per entry and cannot tell a
 * coherent ensemble from one whose members were permuted independently at every entry; the rank of the truth under a pre-rank
 * that sees the whole series can.  samples, truth, mask_u8, mask_per_series as in fd_energy_score, but 1 <= K <= 1023.  For one
 * series S = {x_0 = truth, x_1 .. x_K}, m = K + 1 points, H its hidden entries (mask 0); for candidate j and entry e, over all m
 * points i (j included), b = #{i : x_i[e] < x_j[e]} and a = #{i : x_i[e] > x_j[e]}, on the fp32 values as stored.  prerank[s][j]:
 *   FD_PRERANK_AVERAGE     sum_{e in H} (m - a), the count of x_i[e] <= x_j[e]
 *   FD_PRERANK_BAND_DEPTH  sum_{e in H} [C(m,2) - C(b,2) - C(a,2)], the pairs of points whose closed band holds x_j[e] (without
 *                          ties (m - r)(r - 1) + (m - 1) at rank r = b + 1)
 *   FD_PRERANK_DOMINANCE   #{i : x_i[e] <= x_j[e] for every e in H}, i = j included
 *   FD_PRERANK_MST         the length of the Euclidean minimum spanning tree, over H, of S without x_j (0 when fewer than two points
 *                          remain): differences, squares and sums in double from the fp32 inputs, in ascending entry order
 * below[s] = #{j >= 1 : prerank[s][j] < prerank[s][0]}, equal[s] = #{j >= 1 : prerank[s][j] == prerank[s][0]}, hidden[s] = |H|
 * (hidden may be NULL).  The three integer kinds accumulate in int64 and are written exactly as doubles.  Observed entries are
 * skipped by select: whatever they hold, NaN included, has no effect.  A NaN at a hidden entry, in the truth or in any member,
 * poisons that series and no other: below = equal = -1, its pre-ranks -1 (NaN for FD_PRERANK_MST).  A series without a hidden
 * entry has equal pre-ranks: below 0, equal K, hidden 0.  No atomics: two runs are bit-identical, and a series' outputs do not
 * depend on n or on its position (csrc/fd_mvrank.hip).  work: caller-owned device bytes, at least
 * fd_multivariate_ranks_workspace_bytes of the same kind and shape (FD_PRERANK_MST keeps the (n, m, m) distance matrices there).
 * FD_ERR_ARG: null pointer, an unknown kind, a shape < 1, K outside [1, 1023], a workspace that is too small, T*C >= 2^31 - 64,
 * C(m,2) * T*C >= 2^53, or n too large for one launch (2^31 workgroups). */
enum { FD_PRERANK_AVERAGE = 0, FD_PRERANK_BAND_DEPTH = 1, FD_PRERANK_DOMINANCE = 2, FD_PRERANK_MST = 3 };
int fd_multivariate_ranks_workspace_bytes(fd_ctx* ctx, int kind, int n, int K, int T, int C, size_t* bytes);
int fd_multivariate_ranks(fd_ctx* ctx, int kind, const float* samples, const float* truth, const uint8_t* mask_u8,
                          int mask_per_series, int n, int K, int T, int C, double* prerank /* (n, K + 1) */,
                          int32_t* below /* (n) */, int32_t* equal /* (n) */, int32_t* hidden /* (n) or NULL */, void* work,
                          size_t work_bytes, void* stream);

/* Quadratic forms of the kernel two-sample test (NOT in the reference; Gretton et al. 2012: the unbiased MMD^2 with a permutation
 * p-value is host arithmetic on them, utils/two_sample.py).  z (N, d) dense row-major fp32 device rows with finite entries, the two
 * samples stacked; member (N, P) device bytes, 0 / non-zero = outside / inside the first group: column 0 the observed split, every
 * other column a permutation of it.  scales: HOST doubles c_1..c_Q.
 *   base2       bandwidth2 when > 0, else the mean squared distance over the pairs i != j in its closed form
 *               2 sum_i ||z_i - mean||^2 / (N - 1), entirely in double (fixed order): pooled, the same under every permutation
 *   k(a, b)     (1/Q) sum_q exp(-||a - b||^2 / (c_q base2)); base2 == 0 (all rows equal): k = 1
 *   out_quad    (P) quad[p] = sum_{i != j} A[i,p] k(z_i, z_j) A[j,p]
 *   out_rowsum  (N) rowsum[i] = sum_{j != i} k(z_i, z_j)
 *   out_col0    (N) or NULL: col0[i] = sum_{j != i} k(z_i, z_j) A[j,0]
 *   out_base2   (1) base2 as used
 * One fused kernel (csrc/fd_mmd.hip): squared distances as in fd_knn_rows (rows centred by their column mean, fp32-MFMA expansion
 * ||a||^2 + ||b||^2 - 2 a.b, clamped at 0), Q hardware exponentials per pair, the diagonal excluded by INDEX, and the product with
 * the membership rows by a second fp32 MFMA fed from the first one's accumulator; the N x N matrix never exists.  The value of a
 * pair does not depend on the tile it falls in nor on its orientation (i, j) / (j, i): every column's quad is the quadratic form of
 * ONE symmetric matrix, so the permutation test is exactly level whatever the rounding.  P + 1 columns (one of ones, for rowsum)
 * are accumulated 256 at a time; beyond that the column chunks go on a grid dimension and the distances are recomputed
 * ceil((P + 1) / 256) times.
 * Error.  A term passes at most c = 2048 fp32 additions (128 * min(16, max(1, tiles / 16)) streamed rows, tiles = ceil(N / 128))
 * before it reaches double; everything after is double in a fixed order.  With u = 2^-24 and delta_ij the expansion error of
 * fd_knn_rows, 2 (d + 3) u (||z_i - mean||^2 + ||z_j - mean||^2):
 *   |quad~_p - quad_p| <= sum_{i != j} A_ip A_jp eps_ij + c u quad_p,   eps_ij = delta_ij / (min_q c_q base2) + 8 u
 * (8 u: rounding of the exponent factor and of its product with d2, at most 0.74 u on a value <= 1; 2 u for v_exp_f32; under 4.4 u for
 * the Q - 1 additions of the mixture); rowsum and col0 likewise with the sums over j.
 * col_splits: 0 = automatic, else the number of workgroup columns the streamed rows are divided over (clipped to the number of
 * row groups).  Partials go to work and are added in double in a fixed order by a second kernel; no atomics: results are
 * bit-identical between runs and for every col_splits.  work: caller-owned device bytes, at least
 * fd_kernel_quadforms_workspace_bytes of the same shape.
 * FD_ERR_ARG: null pointer (out_col0 excepted), N < 2, d < 1, P outside [1, 1024], n_scales outside [1, 8], a scale that is not
 * finite and > 0, a bandwidth2 that is not finite, col_splits < 0, N * d or N * P >= 2^31, a workspace that is too small. */
int fd_kernel_quadforms_workspace_bytes(fd_ctx* ctx, int N, int d, int P, int col_splits, size_t* bytes);
int fd_kernel_quadforms(fd_ctx* ctx, const float* z, int N, int d, const double* scales /* host */, int n_scales,
                        double bandwidth2 /* <= 0: pooled mean pair distance */, const uint8_t* member /* (N, P) device */, int P,
                        int col_splits /* 0: automatic */, double* out_quad /* (P) */, double* out_rowsum /* (N) */,
                        double* out_col0 /* (N) or NULL */, double* out_base2 /* (1) device */, void* work, size_t work_bytes,
                        void* stream);

/* Entropic optimal transport between two sample sets, cost ||x - y||^2 (NOT in the reference; Genevay et al. 2018, Feydy et al.
 * 2019; the debiased Sinkhorn divergence is host arithmetic on the potentials, utils/sinkhorn.py).  x (n, d), y (m, d) dense
 * row-major fp32 device rows with finite entries.
 *
 * fd_softmin_pairs: one pass, out[i] = -eps log sum_j exp((h[j] - ||x_i - y_j||^2) / eps); h (m) and out (n) device doubles, h
 * finite.  One fused kernel (csrc/fd_sinkhorn.hip): both sets centred by the mean of the pooled rows, squared distances as in
 * fd_knn_rows (fp32-MFMA expansion clamped at 0), the exponent (h_j - d2) s with s = f32(log2 e / eps) by one fma on d2, a running
 * (max, sum) per owned row with v_exp_f32 on the difference to the maximum; rows of the padding are masked by INDEX.  The n x m
 * matrix never exists.  `same`: x and y are one array (x == y and n == m is detected by the call itself).
 * Error.  With u = 2^-24, delta_ij the expansion error of fd_knn_rows about the pooled mean and c = 64 gt + 1 <= 1025 the longest
 * fp32 addition chain (gt = min(16, max(1, tiles / 16)), tiles = ceil(m / 128)):
 *   |out~_i - out_i| <= max_j (delta_ij + u |h_j|) + 6 u max_j |h_j - d2_ij| + eps (67 gt + 9) u
 * (the soft-min is 1-Lipschitz in its exponents under the sup norm: the roundings of s, s h_j, the fma and the subtraction of the
 * maximum; then 2 u per v_exp_f32, c u for the chain and 3 u per rescaling of the running sum.  DESIGN.md 3.28 derives the terms).
 * splits: 0 = automatic, else the number of workgroup columns the streamed row groups are divided over.  The groups' fp32 (max,
 * sum) pairs go to work and are merged in double in group order by a second kernel; no atomics: results are bit-identical between
 * runs and for every splits.
 *
 * fd_sinkhorn_potentials: the whole iteration, enqueued on the stream with no host synchronisation: centring once, then n_steps
 * iterations, iteration k at eps[k] eps_base (absolute != 0: at eps[k]); eps: n_steps HOST doubles.
 *   eps_base    the mean squared distance over the pooled pairs i != j in its closed form 2 sum ||z_i - mean||^2 / (N - 1), in
 *               double (as base2 of fd_kernel_quadforms); 1 when every row is the same
 *   a, b        device doubles (n) / (m), positive and summing to 1, or NULL = uniform; a soft-min over the rows of y runs on
 *               h_j = g_j + eps log b_j
 *   symmetric 0 f <- softmin_Y(g), g <- softmin_X(f) per iteration, from g = 0; ends on a g update
 *   symmetric 1 (x == y, n == m) p <- (p + softmin_X(p)) / 2 from p = 0 with the weights a; out_f = out_g = p
 *   out_f (n), out_g (m), out_eps_base (1): device doubles
 * Every soft-min obeys the bound above, and both updates are non-expansive in the sup norm: after L soft-min passes the error of a
 * potential is at most the sum of the L per-pass bounds.
 * work: caller-owned device bytes, at least the matching _workspace_bytes of the same shape.
 * FD_ERR_ARG: null pointer (a, b excepted), n, m or d < 1, n * d, m * d or n + m >= 2^31, an eps that is not finite and > 0,
 * splits < 0, n_steps outside [1, 256], same / symmetric with different sets, a workspace that is too small. */
int fd_softmin_pairs_workspace_bytes(fd_ctx* ctx, int n, int m, int d, int same, int splits, size_t* bytes);
int fd_softmin_pairs(fd_ctx* ctx, const float* x, int n, const float* y, int m, int d, const double* h /* (m) device */, double eps,
                     int splits /* 0: automatic */, double* out /* (n) device */, void* work, size_t work_bytes, void* stream);
int fd_sinkhorn_potentials_workspace_bytes(fd_ctx* ctx, int n, int m, int d, int symmetric, size_t* bytes);
int fd_sinkhorn_potentials(fd_ctx* ctx, const float* x, int n, const float* y, int m, int d, int symmetric,
                           const double* a /* (n) device or NULL */, const double* b /* (m) device or NULL */,
                           const double* eps /* (n_steps) host */, int n_steps, int absolute, double* out_f /* (n) */,
                           double* out_g /* (m) */, double* out_eps_base /* (1) device */, void* work, size_t work_bytes,
                           void* stream);

/* Dependence structure inside a series (NOT in the reference; the autocorrelation difference of TSGBench, the correlational score
 * of Ni et al. and Diffusion-TS; the metric is host arithmetic on the set means, utils/dependence.py).  x (n, T, C) dense
 * row-major fp32 device series with finite entries; L = acf_lags in [0, T - 1], Lx = ccf_lags in [-1, T - 1] (-1: no ccf).
 * For one series and channel c (the biased estimators of numpy / statsmodels: the lag matrices are positive semidefinite):
 *   mu_c = (1/T) sum_t x[t,c],  e[t,c] = x[t,c] - mu_c,  m_k = (1/T) sum_t e^k
 *   out_moments (n, C, 4) fp32 or NULL   (mu, sqrt(m_2), m_3 / m_2^1.5, m_4 / m_2^2 - 3)
 *   out_acf     (n, L, C) fp32 or NULL   acf[l-1, c] = sum_{t=0}^{T-1-l} e[t,c] e[t+l,c] / (T m_2(c)),  l = 1..L
 *   out_ccf     (n, Lx+1, C, C) fp32 or NULL   ccf[l, c, d] = sum_{t=0}^{T-1-l} e[t,c] e[t+l,d] / (T sqrt(m_2(c) m_2(d))),  l = 0..Lx,
 *               every ordered pair: a negative lag of (c, d) is the positive lag of (d, c)
 *   out_set_mean (F) DOUBLES or NULL     the mean over the n series of every fp32 feature as returned, in the order
 *               moments | acf | ccf, F = 4 C + L C + (Lx + 1) C^2; computed whether or not the per-series arrays are asked for
 * A channel whose T entries are bit-equal has e == 0 exactly (below): its skewness, kurtosis, acf and every ccf entry it takes
 * part in are 0, not NaN; its mean is the value and its deviation 0; no other entry is affected.
 * Arithmetic (csrc/fd_dependence.hip).  One fused kernel: a series is read once into the LDS, transposed.  mu is a DOUBLE sum (P
 * lanes per channel, strided, then a butterfly; P the largest power of two <= 64 / C) divided by T; T <= 1024 equal floats v make
 * every partial sum k v exact (34 bits), so mu = v and e = 0.  e = f32(x - mu) with the difference taken in double before any
 * product; every sum of products of e (S_k = sum e^k, and each lag's sum, over t ascending) is accumulated in double by fma;
 * value = f32(sum / sqrt(S_2(c) S_2(d))).  fp32 enters twice: once in e, once in the returned value.
 * Pure function per series: a series' features depend on that series and (T, C) alone -- not on n, its position, the grid,
 * L, Lx or which outputs are asked for.  ccf[l, c, c] is acf[l - 1, c] bit for bit (one product serves both), and ccf[0, c, c] is
 * exactly 1 for a non-constant channel (the two double sums of e^2 differ by at most T 2^-52 relative, far inside the fp32
 * rounding of 1).
 * Set means: series are cut into chunks of 32 (fd_series_dependence's own constant); a chunk's features are added in double in
 * series order by the one thread that owns the feature, the chunk sums go to work, a second kernel adds the chunks of every 64 in
 * chunk order and a third those sums in order: a grouping that depends on n alone.
 * No atomics: results are bit-identical between runs and for every grid (FDIFF_DEP_SPLITS forces the workgroup count).
 * Error against the float64 value, u = 2^-24, v = 2^-53, h_t = (u + 2 v) |e_t| + rho, rho = (T + 2) v max_t |x_t| (the mean's
 * share: centring survives an offset of 1000 at a cost of about 1e-11 of the deviation):
 *   acf, ccf   |r~ - r| <= (dN + |r| dD) / (D - dD) + u |r|,  D = sqrt(S_2(c) S_2(d)),  dN = sum (|e| h' + h |e'| + h h') + T v sum (|e| + h)(|e'| + h'),
 *              dD from dS_2 = sum (2 |e| h + h^2) + T v sum (|e| + h)^2; by Cauchy-Schwarz (sum |e e'| <= D) this is at most
 *              c u + O(rho / sd) with c = 5 + O(T 2^-29) for every T: the chains are double, so c does not grow with T
 *   skewness   the same quotient rule on sqrt(T) S_3 / S_2^1.5: about 3 u sum |e|^3 / (T m_2^1.5) + 4 u |skewness|
 *   kurtosis   on T S_4 / S_2^2 - 3: about 4 u sum e^4 / (T m_2^2) + 5 u (kurtosis + 3)
 *   mean, deviation  u |mu| + rho;  u sd + dS_2 / (2 T sd)
 * (tests/dependence_ref.py evaluates these per entry; DESIGN.md 3.29 derives them).
 * Limits: T <= 1024, C <= 64, and the series plus one double per feature of a series (lags padded to the kernel's lag block) within
 * 160 KiB of LDS -- every datamodule shape and T <= 1024 with C <= 16 at the default lags.  work: caller-owned device bytes, at
 * least fd_series_dependence_workspace_bytes of the same shape; needed (non-null) only with out_set_mean.
 * FD_ERR_ARG (nothing is launched): null x, n, T or C < 1, T > 1024 or C > 64, acf_lags outside [0, T - 1], ccf_lags outside
 * [-1, T - 1], every output null, out_acf with acf_lags = 0, out_ccf with ccf_lags = -1, more LDS than a CU has, n F or n T C >= 2^31,
 * out_set_mean with a workspace that is null or too small. */
int fd_series_dependence_workspace_bytes(fd_ctx* ctx, int n, int T, int C, int acf_lags, int ccf_lags, size_t* bytes);
int fd_series_dependence(fd_ctx* ctx, const float* x, int n, int T, int C, int acf_lags, int ccf_lags,
                         float* out_moments /* (n, C, 4) or NULL */, float* out_acf /* (n, L, C) or NULL */,
                         float* out_ccf /* (n, Lx + 1, C, C) or NULL */, double* out_set_mean /* (F) or NULL */, void* work,
                         size_t work_bytes, void* stream);

/* Spectral dependence: Welch's averaged periodogram of every series (NOT in the reference; scipy.signal.welch / csd's conventions at
 * fs = 1, scaling = "density", one-sided; the metric is host arithmetic on the set means, utils/spectral.py).
 * x (n, T, C) dense row-major fp32 device series with finite entries; S = nperseg in [2, T], noverlap in [0, S - 1], H = S - noverlap;
 * segments start at 0, H, 2 H, ... while start + S <= T (a tail is dropped), nseg = (T - S) / H + 1; K = S / 2 + 1 bins, f_k = k / S;
 * window 0 = boxcar, 1 = periodic Hann 0.5 - 0.5 cos(2 pi s / S); detrend 1 subtracts every segment's mean, 0 nothing.
 * For one series, v = (segment - its mean) w:
 *   F[k, c] = sum_s v[s, c] exp(-2 pi i k s / S)
 *   P[k, c, d] = scale_k / (nseg sum w^2) sum_seg conj(F[k, c]) F[k, d],  scale_k = 2, but 1 at k = 0 and at the Nyquist bin of an even S
 *   out_psd     (n, K, C) fp32 or NULL       P[k, c, c]
 *   out_csd     (n, K, NP, 2) fp32 or NULL   (Re, Im) P[k, c, d] of the NP = C (C - 1) / 2 pairs c < d in row-major pair order
 *   out_summary (n, C, 3) fp32 or NULL       total power sum_k psd; spectral centroid sum f_k psd_k / sum psd_k and spectral entropy
 *               -sum p ln p / ln(K - 1), p_k = psd_k / sum psd, both over the bins 1..K-1 (bin 0 holds only leakage after detrending)
 *   out_set_mean (F) DOUBLES, required      the mean over the n series of every fp32 feature as returned, in the order
 *               psd | csd | summary, F = K C + 2 K NP + 3 C
 * A channel whose S entries are bit-equal in every segment has v == 0 exactly under detrend (below): its psd, every csd entry it
 * takes part in and its summaries are 0, not NaN; no other entry is affected.  K = 2 gives entropy 0.
 * Arithmetic (csrc/fd_spectral.hip).  One fused kernel: a series is read once into the LDS.  The segment sum is a DOUBLE sum (16
 * lanes per (segment, channel), strided, then a butterfly); the entry is ((double)S x - sum) (1 / S): on floats of a grid S x and the
 * sum are exact, so x + 1000 gives the bits of x; S equal floats give 0.  It is multiplied by the double window and rounded to fp32
 * ONCE.  The DFT is a product against a [cos | sin] basis built on the device in
 * double (angle 2 pi (k s mod S) / S), rounded to fp32 once and cached on the context per (S, window); it runs on
 * v_mfma_f32_16x16x4_f32 with fp32 accumulation (any S: no radix).  conj(F_c) F_d is summed over the segments in segment order in
 * double, scaled and rounded to fp32; the summaries come from the double PSD.  fp32 enters three times: v, the basis with the DFT's
 * accumulation, the returned value.
 * Pure function per series: a series' features depend on that series and (T, C, S, noverlap, window, detrend) alone -- not on n, its
 * position, the grid or which outputs are asked for.  The PSD goes through the cross-spectrum's code: csd of a channel copied into two
 * columns has the PSD's bits as its real part and imaginary part 0.
 * Set means: series are cut into chunks of 32; a chunk's features are added in double in series order by the one thread that owns
 * the feature, into a cell of work; a second kernel adds the chunks of every 64 in chunk order and a third those sums in order: a
 * grouping that depends on n alone.  No atomics: bit-identical between runs and for every grid (FDIFF_SPEC_SPLITS forces the
 * workgroup count).
 * Error against the float64 value, u = 2^-24, v = 2^-53, gamma = (S + 1) u / (1 - (S + 1) u): a segment entry is off by at most
 * h_s = (u + 4 v) |v_s| + rho w_s, rho = (S + 2) v max |x| (0 without detrend); a cos or sin sum by at most
 * eps_c = sum_s h_s + gamma sum_s (|v_s| + h_s), which scales with the segment's 1-norm (with sqrt(S x total power)), not with the
 * bin's own magnitude; P[k, c, d] by at most scale_k / (nseg sum w^2) sum_seg (sqrt(2) (eps_c |F_d| + eps_d |F_c|) + 2 eps_c eps_d)
 * + u |P|; the summaries by the quotient rule on these (tests/spectral_ref.py evaluates them per entry; DESIGN.md 3.34 derives them).
 * Limits: T <= 1024, C <= 64, and the LDS plan of one series -- the series (4 T C bytes), the segment image and the DFT image
 * (4 Np (Sp + Mp) bytes with Sp, Mp, Np = S, 2 K and nseg C rounded up to 16), the double PSD (8 K C), the window (8 Sp), the pair
 * table (2 NP) and, while they take 8 KiB or less, the chunk sums (8 F) -- within 160 KiB: every datamodule shape at the default
 * nperseg.  work: caller-owned device bytes, at least
 * fd_series_spectra_workspace_bytes of the same shape.
 * FD_ERR_ARG (nothing is launched): null x, n, T or C < 1, T > 1024 or C > 64, nperseg outside [2, T], noverlap outside
 * [0, nperseg - 1], window or detrend neither 0 nor 1, more LDS than the plan may take, n F or n T C >= 2^31, null out_set_mean,
 * out_csd with C = 1, a workspace that is null or too small. */
int fd_series_spectra_workspace_bytes(fd_ctx* ctx, int n, int T, int C, int nperseg, int noverlap, size_t* bytes);
int fd_series_spectra(fd_ctx* ctx, const float* x, int n, int T, int C, int nperseg, int noverlap, int window, int detrend,
                      float* out_psd /* (n, K, C) or NULL */, float* out_csd /* (n, K, NP, 2) or NULL */,
                      float* out_summary /* (n, C, 3) or NULL */, double* out_set_mean /* (F) */, void* work, size_t work_bytes,
                      void* stream);

/* Path signatures (NOT in the reference; Sig-W1 of Ni et al. 2021, the signature MMD of Chevyrev & Oberhauser; the metrics are host
 * arithmetic on the outputs, utils/signature.py): the iterated integrals up to depth m of the piecewise linear path
 * through a series.  x (n, T, C) dense row-major fp32 device series with finite entries, n >= 1, 2 <= T <= 1024, 1 <= C <= 64,
 * 1 <= depth <= 6; channel_offset, channel_scale (C) device DOUBLES or NULL (0 and 1).  The path, in this order:
 *   1. p[t, c] = scale_c (x[t, c] - offset_c), in double
 *   2. FD_SIG_BASEPOINT: the point 0 is prepended (the signature then sees the starting value, not only the increments)
 *   3. D[s] = p[s + 1] - p[s] over S = T - 1 segments (T with a basepoint)
 *   4. FD_SIG_LEAD_LAG: 2 S segments over 2 C channels [lead_0..lead_{C-1}, lag_0..lag_{C-1}]; segment 2 k moves the lead channels by
 *      D[k], segment 2 k + 1 the lag channels by D[k]
 *   5. FD_SIG_TIME: one last channel that moves by 1.0 / S' per segment, S' the final number of segments
 * d = the final channel count, D = d + d^2 + ... + d^depth <= 8192 features: levels 1..depth concatenated, a level row-major over its
 * words with the first letter slowest.  Per segment and level-k word w (Chen's identity with the exponential of a linear segment, in
 * Horner form; every read is of the state before the segment):
 *   acc = D[w_1] / k;   acc = (acc + S_j[w_1..w_j]) D[w_{j+1}] / (k - j) for j = 1..k-1;   S_k[w] += acc
 *   sig    (n, D) fp32 or NULL      the state after the last segment, rounded once
 *   sqnorm (n) DOUBLES or NULL      sum_w S_w^2 of the double state
 *   mean   (D) DOUBLES, required    the mean over the n series of the double state
 * Arithmetic (csrc/fd_signature.hip).  The state and every operation are double, nothing is contracted into an fma: a repeated point
 * (a zero increment) leaves every bit of the state alone unless FD_SIG_TIME is set, and a channel with scale 0 gives exact zeros in
 * every word that holds its letter.  With u = 2^-53, l = sum_s ||D[s]||_1 and M_k = l^k / k!, a level-k entry is within
 * b_k = 32 S' u M_k of the exact value of the float64 path (tests/signature_ref.py; DESIGN.md 3.39 derives it).
 * Pure function per series: a series' sig and sqnorm depend on that series, (T, C, depth, flags) and the offsets and scales alone --
 * not on n, its position, the grid or which outputs are asked for.
 * Set mean: series are cut into chunks of 32; a chunk's states are added in double in series order by the one thread that owns the
 * word, the chunk sums go to work, a second kernel adds the chunks of every 64 in chunk order and a third those sums in order: a
 * grouping that depends on n alone.  No atomics: bit-identical between runs and for every grid (FDIFF_SIG_SPLITS forces the workgroup
 * count).  work: caller-owned device bytes, at least fd_series_signature_workspace_bytes of the same shape.
 * FD_ERR_ARG (nothing is launched): null x, n < 1, T < 2, C < 1, T > 1024 or C > 64, depth outside [1, 6], flags outside [0, 7],
 * D > 8192, n D or n T C >= 2^31, null mean, a workspace that is null or too small. */
#define FD_SIG_BASEPOINT 1
#define FD_SIG_LEAD_LAG 2
#define FD_SIG_TIME 4
int fd_series_signature_workspace_bytes(fd_ctx* ctx, int n, int T, int C, int depth, int flags, size_t* bytes);
int fd_series_signature(fd_ctx* ctx, const float* x, int n, int T, int C, int depth, int flags,
                        const double* channel_offset /* (C) or NULL */, const double* channel_scale /* (C) or NULL */,
                        float* sig /* (n, D) or NULL */, double* sqnorm /* (n) or NULL */, double* mean /* (D) */, void* work,
                        size_t work_bytes, void* stream);

/* Post-hoc discriminative and predictive scores (NOT in the reference; TimeGAN, Yoon et al. 2019, and TSGBench; DESIGN.md 3.31,
 * utils/posthoc.py): what a small network trained AFTER the fact needs around the causal LSTM backbone (fd_score_create_ex with
 * FD_BACKBONE_LSTM), whose output at time t sees the inputs <= t only -- out[:, t] regressed on x[:, t + 1] is a next-step
 * forecaster, the mean over channels of out[:, T - 1] a classifier logit.  Plain fp32 / fp64 kernels (csrc/fd_posthoc.hip), no
 * atomics, every sum in double in an order that depends on the shape alone: two runs are bit-identical.
 *
 * fd_posthoc_batch   one minibatch drawn and gathered on the device.  a (na, T, C), b (nb, T, C): dense fp32 device pools; mean,
 *                    inv_std: fp32[C].  x (B, T, C) = (row - mean) * inv_std (one subtraction, one product, each rounded once),
 *                    label (B) and idx (B) int32.  FD_POSTHOC_CLASSIFY (b non-null, B even): rows j < B / 2 come from a with label 1,
 *                    the others from b with label 0.  FD_POSTHOC_PREDICT: every row from a, label 1, b and nb ignored.
 *                    Index rule, restatable from fd_philox_words: row j of step s takes word j % 4 of counter
 *                    offset + s * ceil(B / 4) + j / 4 under the key seed; idx = (uint64(word) * n) >> 32, n the size of the pool the
 *                    row draws from (with replacement).
 * fd_posthoc_head    the task head, its loss and d loss / d out in one pass over out (B, T, C).
 *                    PREDICT:  loss = mean over b, t < T - 1, c of |out[b,t,c] - x[b,t+1,c]|; dout = sign(diff) / (B (T - 1) C) with
 *                              sign(0) = 0 and the rows t = T - 1 exactly 0; per_series[b] = that series' sum of absolute errors;
 *                              label unused (may be NULL); T < 2: FD_ERR_ARG.
 *                    CLASSIFY: logit_b = mean_c out[b, T - 1, c]; loss = mean_b (softplus(logit_b) - label_b logit_b), softplus(v) =
 *                              max(v, 0) + log1p(exp(-|v|)); dout[b, T - 1, c] = (sigmoid(logit_b) - label_b) / (B C), exactly 0
 *                              everywhere else; per_series[b] = logit_b; x unused (may be NULL); label may be NULL when loss and
 *                              dout both are (the logits alone).
 *                    Differences, sums, sigmoid and softplus in double; loss and dout are rounded to fp32 once.  per_series: B DOUBLES,
 *                    required.  loss == NULL: not computed; dout == NULL: evaluation only.
 * fd_posthoc_fit     the training loop as ONE call: for k = 0 .. steps - 1, with s = first_step + k, it enqueues fd_posthoc_batch
 *                    (step s) -> fd_score_forward_train (t = 0 on every row, dropout 0) -> fd_posthoc_head -> fd_score_backward
 *                    (accumulate 0) -> [fd_grad_sqnorm, when max_norm > 0] -> fd_adamw_step (step s + 1, constant lr, betas (0.9, 0.999),
 *                    eps 1e-8, weight_decay 1e-2, time_encoder.W skipped), with no host synchronisation; the same calls made one by
 *                    one give the same bits.  T and C are the model's.  params: the buffer fd_score_prepare bound (FD_ERR_ARG
 *                    otherwise); grads, exp_avg, exp_avg_sq: its size.  loss_trace: device float[steps], the loss of every step
 *                    BEFORE its update.  idx_trace: device int32[steps * B] or NULL, the indices of every step.  work: caller-owned
 *                    device bytes, at least fd_posthoc_fit_workspace_bytes(B, T, C).  The weights changed: call fd_score_prepare
 *                    (or mark the parameters changed) before the model is used through another entry point.
 *                    FD_ERR_UNSUPPORTED for a model whose backbone is not the LSTM (nothing is launched).
 * FD_ERR_ARG (nothing is launched): an unknown task, a null pointer other than those named optional, a shape < 1, B T C >= 2^31,
 * classify with b null, nb < 1 or an odd B, step or first_step < 0, steps < 1, lr <= 0, a workspace that is null or too small. */
#define FD_POSTHOC_CLASSIFY 0
#define FD_POSTHOC_PREDICT 1
int fd_posthoc_batch(fd_ctx* ctx, int task, const float* a, int na, const float* b /* or NULL */, int nb, const float* mean,
                     const float* inv_std, uint64_t seed, uint64_t offset, int step, int B, int T, int C, float* x /* (B, T, C) */,
                     int* label /* (B) */, int* idx /* (B) */, void* stream);
int fd_posthoc_head(fd_ctx* ctx, int task, const float* out, const float* x, const int* label, int B, int T, int C,
                    float* loss /* (1) or NULL */, float* dout /* (B, T, C) or NULL */, double* per_series /* (B) */, void* stream);
int fd_posthoc_fit_workspace_bytes(fd_ctx* ctx, int B, int T, int C, size_t* bytes);
int fd_posthoc_fit(fd_score* m, int task, float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* a, int na,
                   const float* b /* or NULL */, int nb, const float* mean, const float* inv_std, uint64_t seed, uint64_t offset,
                   int first_step, int steps, int B, float lr, float max_norm, float* loss_trace /* (steps) */,
                   int* idx_trace /* (steps, B) or NULL */, void* work, size_t work_bytes, void* stream);

/* Label-aware post-hoc scores (NOT in the reference; TSTR / TRTS of RCGAN, Esteban et al. 2017, and the classification accuracy
 * score of Ravuri & Vinyals 2019; DESIGN.md 3.32, utils/posthoc.py): the K-way task on the same causal LSTM.  The backbone maps
 * (B, T, Cn) to (B, T, Cn), so the network has Cn = max(C, K) channels: the series fill the input channels < C, the others are fed
 * +0.0, and the K logits of series b are out[b, T - 1, 0 .. K - 1], where the LSTM has seen the whole series.  mean and inv_std stay
 * fp32[C].  Same house rules as above: fp32 / fp64, no atomics, fixed-order double sums, bit-identical runs.
 *
 * fd_posthoc_batch_labelled   one minibatch from ONE labelled pool a (na, T, C), ya (na) int32 in [0, K) (the caller's contract).
 *                    Row j of step s takes the Philox word of fd_posthoc_batch (word j % 4 of counter offset + s * ceil(B / 4) + j / 4
 *                    under the key seed).  Uniform (order and class_start NULL): idx = (uint64(word) * na) >> 32.  Balanced (both
 *                    non-null): order (na) lists the rows sorted stably by class, class_start (K + 1) the offsets into it; with P
 *                    the number of classes that hold a row and c the ((uint64)s * B + j) % P-th of them in ascending order,
 *                    idx = order[class_start[c] + ((uint64(word) * count[c]) >> 32)].  x (B, T, Cn): channels < C are
 *                    (a[idx] - mean) * inv_std (one subtraction, one product, each rounded once), channels >= C are +0.0;
 *                    label[j] = ya[idx]; idx (B).  Indices read from a broken table are clamped into the pool.
 * fd_posthoc_head_multiclass   softmax cross-entropy on out (B, T, Cn), one workgroup per series; every output is optional.
 *                    logp (B, K) doubles: logit - max - log(sum exp(logit - max)), in double; pred (B) int32: the argmax, ties to
 *                    the lowest class; nll (B) doubles: -logp[b, label_b] (NaN for a label outside [0, K)); loss: float
 *                    mean_b nll[b], added in the fixed order of fd_posthoc_head's loss (needs nll); dout (B, T, Cn):
 *                    (softmax - onehot) / B at [b, T - 1, k < K], +0.0 everywhere else.  label may be NULL when loss, dout and nll
 *                    are.  T = 1 is allowed.
 * fd_posthoc_fit_multiclass    the loop of fd_posthoc_fit with those two stages: fd_posthoc_batch_labelled (step s) ->
 *                    fd_score_forward_train (t = 0, dropout 0) -> fd_posthoc_head_multiclass -> fd_score_backward ->
 *                    [fd_grad_sqnorm] -> fd_adamw_step, same optimiser constants, time_encoder.W skipped, no host
 *                    synchronisation; the same calls made one by one give the same bits.  The model is an LSTM of Cn = max(C, K)
 *                    channels; C is the pool's.  work: at least fd_posthoc_fit_multiclass_workspace_bytes(B, T, Cn).
 * fd_posthoc_confusion   counts (K, K) int32, counts[r, c] = #{i < n : label[i] == r, pred[i] == c}: rows are the true class.
 *                    Every entry is written; pairs outside [0, K) are counted nowhere.
 * FD_ERR_ARG (nothing is launched): K < 2 or K > FD_POSTHOC_MAX_CLASSES (one logit per thread of a workgroup), Cn != max(C, K)
 * (head: Cn < K), an empty pool (na < 1), order without class_start or the reverse, loss, dout or nll without label, loss without
 * nll, every head output NULL, n < 1, and what fd_posthoc_fit refuses.  FD_ERR_UNSUPPORTED: a model that is not the LSTM. */
#define FD_POSTHOC_MAX_CLASSES 256
int fd_posthoc_batch_labelled(fd_ctx* ctx, const float* a, int na, const int* ya, const int* order /* (na) or NULL */,
                              const int* class_start /* (K + 1) or NULL */, int K, const float* mean, const float* inv_std,
                              uint64_t seed, uint64_t offset, int step, int B, int T, int C, int Cn, float* x /* (B, T, Cn) */,
                              int* label /* (B) */, int* idx /* (B) */, void* stream);
int fd_posthoc_head_multiclass(fd_ctx* ctx, const float* out, const int* label /* (B) or NULL */, int B, int T, int Cn, int K,
                               double* logp /* (B, K) or NULL */, int* pred /* (B) or NULL */, float* loss /* (1) or NULL */,
                               float* dout /* (B, T, Cn) or NULL */, double* nll /* (B) or NULL */, void* stream);
int fd_posthoc_fit_multiclass_workspace_bytes(fd_ctx* ctx, int B, int T, int Cn, size_t* bytes);
int fd_posthoc_fit_multiclass(fd_score* m, int K, float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* a,
                              int na, const int* ya, const int* order /* or NULL */, const int* class_start /* or NULL */, int C,
                              const float* mean, const float* inv_std, uint64_t seed, uint64_t offset, int first_step, int steps,
                              int B, float lr, float max_norm, float* loss_trace /* (steps) */,
                              int* idx_trace /* (steps, B) or NULL */, void* work, size_t work_bytes, void* stream);
int fd_posthoc_confusion(fd_ctx* ctx, const int* label, const int* pred, int n, int K, int* counts /* (K, K) */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDIFF_HIP_H */
