// fd_posthoc.hip -- what a network trained AFTER the fact needs around the causal LSTM backbone (NOT in the reference; the
// discriminative and predictive scores of TimeGAN / TSGBench): the minibatch draw, the two task heads with their
// gradients, and the training loop as one call.
//
//   fd_posthoc_batch   k_posthoc_batch: row j of step s takes word j % 4 of Philox counter offset + s ceil(B / 4) + j / 4 under the key
//                      seed, idx = (uint64(word) n) >> 32 with n the size of the pool the row draws from, and gathers
//                      x[j] = (pool[idx] - mean) * inv_std per channel.  One workgroup per row.
//   fd_posthoc_head    k_posthoc_head (one workgroup per series: its sum of absolute errors, or its logit, in double, and d loss /
//                      d out) and k_posthoc_loss (one workgroup: the series' terms added in a fixed order).
//   fd_posthoc_fit     steps x { batch, fd_score_forward_train, head, fd_score_backward, fd_adamw_step } enqueued with no host
//                      synchronisation; the loss of every step goes to a device array.
//
// The K-way task (TSTR / TRTS classification accuracy) runs on a backbone of Cn = max(C, K) channels, whose output
// out[b, T - 1, 0 .. K - 1] holds the K logits of series b:
//   fd_posthoc_batch_labelled   k_posthoc_batch_labelled: the same Philox word per row, drawn from ONE labelled pool, uniformly or
//                               class by class (the row's class is fixed by its position, the word picks a row of that class);
//                               input channels >= C are +0.0.
//   fd_posthoc_head_multiclass  k_posthoc_head_mc (one workgroup per series, thread k owns logit k: log-softmax in double with the
//                               maximum subtracted first, argmax with ties to the lowest class, d loss / d out) and k_posthoc_loss.
//   fd_posthoc_fit_multiclass   the loop of fd_posthoc_fit (ph_fit_steps, shared) around those two stages.
//   fd_posthoc_confusion        k_posthoc_confusion: one workgroup per true class, thread c counts the predictions of class c.
//
// No atomics; every sum runs in double in an order that depends on the shape alone, so two runs are bit-identical.
#include "fd_philox.h"
#include "fd_score.h"

namespace {

constexpr int PH_BLOCK = 256;

__device__ __forceinline__ double ph_block_sum(double v, double* red) {      // the total, valid on thread 0
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(PH_BLOCK) void k_posthoc_batch(const float* __restrict__ a, unsigned na, const float* __restrict__ b,
                                                             unsigned nb, const float* __restrict__ mean,
                                                             const float* __restrict__ inv_std, uint64_t seed, uint64_t ctr0, int B, int TC,
                                                             int C, float* __restrict__ x, int* __restrict__ label, int* __restrict__ idx) {
    const int j = blockIdx.x;
    const bool from_b = b != nullptr && j >= B / 2;
    const fd_u4 r = fd_philox4x32_10(ctr0 + (uint64_t)(j >> 2), seed);
    const uint32_t w = (j & 3) == 0 ? r.x : (j & 3) == 1 ? r.y : (j & 3) == 2 ? r.z : r.w;
    const uint32_t row = (uint32_t)(((uint64_t)w * (uint64_t)(from_b ? nb : na)) >> 32);
    const float* src = (from_b ? b : a) + (size_t)row * TC;
    float* dst = x + (size_t)j * TC;
    for (int i = threadIdx.x; i < TC; i += PH_BLOCK) {
        const int c = i % C;
        dst[i] = __fmul_rn(__fsub_rn(src[i], mean[c]), inv_std[c]);
    }
    if (threadIdx.x == 0) {
        label[j] = from_b ? 0 : 1;
        idx[j] = (int)row;
    }
}

// predict: e runs over the (T - 1) C entries out[b, t, c] with t < T - 1, whose target x[b, t + 1, c] lies C floats further on
__global__ __launch_bounds__(PH_BLOCK) void k_posthoc_head(int predict, const float* __restrict__ out, const float* __restrict__ x,
                                                            const int* __restrict__ label, int T, int C, float g_scale,
                                                            double cls_scale, float* __restrict__ dout, double* __restrict__ per_series) {
    __shared__ double red[4];
    __shared__ float g_last;
    const int bi = blockIdx.x, TC = T * C, n = (T - 1) * C;
    const float* o = out + (size_t)bi * TC;
    float* d = dout ? dout + (size_t)bi * TC : nullptr;
    double acc = 0.0;
    if (predict) {
        const float* tgt = x + (size_t)bi * TC + C;
        for (int e = threadIdx.x; e < n; e += PH_BLOCK) {
            const double diff = (double)o[e] - (double)tgt[e];
            acc += fabs(diff);
            if (d) d[e] = diff > 0.0 ? g_scale : diff < 0.0 ? -g_scale : 0.f;
        }
        if (d)
            for (int e = n + threadIdx.x; e < TC; e += PH_BLOCK) d[e] = 0.f;
        const double sum = ph_block_sum(acc, red);
        if (threadIdx.x == 0) per_series[bi] = sum;
        return;
    }
    for (int c = threadIdx.x; c < C; c += PH_BLOCK) acc += (double)o[n + c];
    const double sum = ph_block_sum(acc, red);
    if (threadIdx.x == 0) {
        const double logit = sum / (double)C;
        per_series[bi] = logit;
        if (d) {
            const double ex = exp(-fabs(logit));                      // in (0, 1]: never overflows
            const double sig = logit >= 0.0 ? 1.0 / (1.0 + ex) : ex / (1.0 + ex);
            g_last = (float)((sig - (double)label[bi]) * cls_scale);
        }
    }
    if (!d) return;
    __syncthreads();
    const float g = g_last;
    for (int e = threadIdx.x; e < TC; e += PH_BLOCK) d[e] = e >= n ? g : 0.f;
}

// thread i adds the series i, i + 256, ... in that order, then the fixed tree of ph_block_sum
__global__ __launch_bounds__(PH_BLOCK) void k_posthoc_loss(int predict, const double* __restrict__ per_series,
                                                            const int* __restrict__ label, int B, double inv_count,
                                                            float* __restrict__ loss) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int bi = threadIdx.x; bi < B; bi += PH_BLOCK) {
        const double v = per_series[bi];
        // softplus(v) - y v, softplus(v) = max(v, 0) + log1p(exp(-|v|))
        acc += predict ? v : fmax(v, 0.0) + log1p(exp(-fabs(v))) - (double)label[bi] * v;
    }
    const double sum = ph_block_sum(acc, red);
    if (threadIdx.x == 0) *loss = (float)(sum * inv_count);
}

// One labelled pool.  Balanced (order != null): the row's class is the (row0 + j) % P-th of the P classes that hold a row, in
// ascending order, and the word picks one of that class's rows through order / class_start.  Indices are clamped to the pool, so a
// table that breaks the caller's contract cannot send the gather outside it.
__global__ __launch_bounds__(PH_BLOCK) void k_posthoc_batch_labelled(const float* __restrict__ a, unsigned na, const int* __restrict__ ya,
                                                                      const int* __restrict__ order,
                                                                      const int* __restrict__ class_start, int K,
                                                                      const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                                      uint64_t seed, uint64_t ctr0, uint64_t row0, int T, int C, int Cn,
                                                                      float* __restrict__ x, int* __restrict__ label,
                                                                      int* __restrict__ idx) {
    __shared__ unsigned row_s;
    const int j = blockIdx.x;
    if (threadIdx.x == 0) {
        const fd_u4 r = fd_philox4x32_10(ctr0 + (uint64_t)(j >> 2), seed);
        const uint32_t w = (j & 3) == 0 ? r.x : (j & 3) == 1 ? r.y : (j & 3) == 2 ? r.z : r.w;
        unsigned row = (unsigned)(((uint64_t)w * (uint64_t)na) >> 32);
        if (order) {
            int P = 0;
            for (int c = 0; c < K; ++c) P += class_start[c + 1] > class_start[c] ? 1 : 0;
            if (P > 0) {
                int want = (int)((row0 + (uint64_t)j) % (uint64_t)P), c = 0;
                for (; c < K; ++c)
                    if (class_start[c + 1] > class_start[c] && want-- == 0) break;
                const unsigned lo = (unsigned)class_start[c], count = (unsigned)(class_start[c + 1] - class_start[c]);
                unsigned at = lo + (unsigned)(((uint64_t)w * (uint64_t)count) >> 32);
                at = at < na ? at : na - 1;
                row = (unsigned)order[at];
            }
        }
        row = row < na ? row : na - 1;
        row_s = row;
        label[j] = ya[row];
        idx[j] = (int)row;
    }
    __syncthreads();
    const float* src = a + (size_t)row_s * T * C;
    float* dst = x + (size_t)j * T * Cn;
    for (int i = threadIdx.x; i < T * Cn; i += PH_BLOCK) {
        const int t = i / Cn, c = i - t * Cn;
        dst[i] = c < C ? __fmul_rn(__fsub_rn(src[t * C + c], mean[c]), inv_std[c]) : 0.f;
    }
}

// thread k < K owns logit k = out[b, T - 1, k].  The maximum and its lowest index come from a fixed tree over the 256 slots, the sum
// of exp(logit - max) from ph_block_sum; nll[b] = -logp[b, label_b] feeds k_posthoc_loss.
__global__ __launch_bounds__(PH_BLOCK) void k_posthoc_head_mc(const float* __restrict__ out, const int* __restrict__ label, int T, int Cn,
                                                               int K, double inv_B, double* __restrict__ logp, int* __restrict__ pred,
                                                               float* __restrict__ dout, double* __restrict__ nll) {
    __shared__ double red[4];
    __shared__ double best_v[PH_BLOCK];
    __shared__ int best_i[PH_BLOCK];
    __shared__ double total;
    const int bi = blockIdx.x, k = threadIdx.x, TC = T * Cn, n = (T - 1) * Cn;
    const bool on = k < K;
    const double logit = on ? (double)out[(size_t)bi * TC + n + k] : 0.0;
    best_v[k] = logit;
    best_i[k] = on ? k : K;                                  // K: an empty slot, which loses to every class
    __syncthreads();
    for (int o = PH_BLOCK / 2; o > 0; o >>= 1) {
        if (k < o) {
            const int ia = best_i[k], ib = best_i[k + o];
            const double va = best_v[k], vb = best_v[k + o];
            // the larger logit wins, and between equal logits the lower class
            if (ib < K && (ia >= K || vb > va || (vb == va && ib < ia))) {
                best_v[k] = vb;
                best_i[k] = ib;
            }
        }
        __syncthreads();
    }
    const double mx = best_v[0];
    const int arg = best_i[0];
    const double shifted = logit - mx;
    const double sum = ph_block_sum(on ? exp(shifted) : 0.0, red);
    if (k == 0) total = sum;
    __syncthreads();
    const double lp = shifted - log(total);
    const int y = label ? label[bi] : -1;
    if (on && logp) logp[(size_t)bi * K + k] = lp;
    if (k == 0 && pred) pred[bi] = arg;
    if (on && nll && k == y) nll[bi] = -lp;
    if (k == 0 && nll && (y < 0 || y >= K)) nll[bi] = __longlong_as_double(0x7ff8000000000000ll);      // a label outside [0, K)
    if (!dout) return;
    float* d = dout + (size_t)bi * TC;
    for (int e = k; e < n; e += PH_BLOCK) d[e] = 0.f;
    for (int c = k; c < Cn; c += PH_BLOCK) d[n + c] = c < K ? (float)((exp(lp) - (c == y ? 1.0 : 0.0)) * inv_B) : 0.f;
}

// counts[r, c] = #{i : label[i] == r, pred[i] == c}.  Workgroup r, thread c; the pairs pass through the LDS a block at a time.  Pairs
// outside [0, K) are counted nowhere.
__global__ __launch_bounds__(PH_BLOCK) void k_posthoc_confusion(const int* __restrict__ label, const int* __restrict__ pred, int n, int K,
                                                                 int* __restrict__ counts) {
    __shared__ int lab[PH_BLOCK], prd[PH_BLOCK];
    const int r = blockIdx.x, c = threadIdx.x;
    int count = 0;
    for (int i0 = 0; i0 < n; i0 += PH_BLOCK) {
        const int i = i0 + c, m = min(PH_BLOCK, n - i0);
        if (i < n) {
            lab[c] = label[i];
            prd[c] = pred[i];
        }
        __syncthreads();
        for (int e = 0; e < m; ++e) count += (lab[e] == r && prd[e] == c) ? 1 : 0;
        __syncthreads();
    }
    if (c < K) counts[(size_t)r * K + c] = count;
}

int ph_task_check(fd_ctx* ctx, const char* who, int task) {
    FD_REQUIRE(ctx, task == FD_POSTHOC_CLASSIFY || task == FD_POSTHOC_PREDICT, "%s: unknown task %d", who, task);
    return FD_OK;
}

int ph_shape_check(fd_ctx* ctx, const char* who, int B, int T, int C) {
    FD_REQUIRE(ctx, B >= 1 && T >= 1 && C >= 1, "%s: bad shape B=%d T=%d C=%d (all >= 1)", who, B, T, C);
    FD_REQUIRE(ctx, (long long)B * T * C < (1ll << 31), "%s: B * T * C = %lld must stay below 2^31", who, (long long)B * T * C);
    return FD_OK;
}

int ph_batch(fd_ctx* ctx, const char* who, int task, const float* a, int na, const float* b, int nb, const float* mean,
             const float* inv_std, uint64_t seed, uint64_t offset, int step, int B, int T, int C, float* x, int* label, int* idx,
             hipStream_t s) {
    if (int rc = ph_task_check(ctx, who, task)) return rc;
    if (int rc = ph_shape_check(ctx, who, B, T, C)) return rc;
    FD_REQUIRE(ctx, a && mean && inv_std && x && label && idx, "%s: null pointer", who);
    FD_REQUIRE(ctx, na >= 1 && step >= 0, "%s: na=%d (>= 1), step=%d (>= 0)", who, na, step);
    if (task == FD_POSTHOC_CLASSIFY) {
        FD_REQUIRE(ctx, b && nb >= 1, "%s: the classify task draws from two pools, b is null or nb=%d", who, nb);
        FD_REQUIRE(ctx, B % 2 == 0, "%s: the classify task takes half of the batch from each pool, B=%d is odd", who, B);
    } else {
        b = nullptr;
    }
    const uint64_t ctr0 = offset + (uint64_t)step * (uint64_t)fd_cdiv(B, 4);
    hipLaunchKernelGGL(k_posthoc_batch, dim3(B), dim3(PH_BLOCK), 0, s, a, (unsigned)na, b, (unsigned)nb, mean, inv_std, seed, ctr0, B,
                       T * C, C, x, label, idx);
    return FD_OK;
}

int ph_head(fd_ctx* ctx, const char* who, int task, const float* out, const float* x, const int* label, int B, int T, int C,
            float* loss, float* dout, double* per_series, hipStream_t s) {
    if (int rc = ph_task_check(ctx, who, task)) return rc;
    if (int rc = ph_shape_check(ctx, who, B, T, C)) return rc;
    const bool predict = task == FD_POSTHOC_PREDICT;
    FD_REQUIRE(ctx, out && per_series, "%s: null out or per_series", who);
    FD_REQUIRE(ctx, predict ? x != nullptr : (label != nullptr || (!loss && !dout)), "%s: the %s", who,
               predict ? "predict task needs x, the series the outputs forecast" : "classify task needs the labels for loss and dout");
    FD_REQUIRE(ctx, !predict || T >= 2, "%s: the predict task regresses out[:, t] on x[:, t + 1] and needs T >= 2, got T=%d", who, T);
    const double count = predict ? (double)B * (T - 1) * C : (double)B;
    hipLaunchKernelGGL(k_posthoc_head, dim3(B), dim3(PH_BLOCK), 0, s, predict ? 1 : 0, out, x, label, T, C, (float)(1.0 / count),
                       1.0 / ((double)B * C), dout, per_series);
    if (loss) hipLaunchKernelGGL(k_posthoc_loss, dim3(1), dim3(PH_BLOCK), 0, s, predict ? 1 : 0, per_series, label, B, 1.0 / count, loss);
    return FD_OK;
}

// the buffers of one fit, carved from the caller's workspace
struct PhWork {
    float *x, *out, *dout, *t, *sqnorm;
    int *label, *idx;
    double* per_series;
    size_t bytes;
};
PhWork ph_carve(char* base, int B, int T, int C) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += fd_ws::padded(bytes); return p; };
    const size_t n = (size_t)B * T * C;
    PhWork w;
    w.x = (float*)take(n * sizeof(float));
    w.out = (float*)take(n * sizeof(float));
    w.dout = (float*)take(n * sizeof(float));
    w.t = (float*)take((size_t)B * sizeof(float));
    w.sqnorm = (float*)take(sizeof(float));
    w.label = (int*)take((size_t)B * sizeof(int));
    w.idx = (int*)take((size_t)B * sizeof(int));
    w.per_series = (double*)take((size_t)B * sizeof(double));
    w.bytes = off + 256;          // room to align the base
    return w;
}

int ph_classes_check(fd_ctx* ctx, const char* who, int K) {
    FD_REQUIRE(ctx, K >= 2 && K <= FD_POSTHOC_MAX_CLASSES, "%s: K=%d classes, from 2 to %d (one logit per thread of a workgroup)", who, K,
               FD_POSTHOC_MAX_CLASSES);
    return FD_OK;
}

int ph_batch_labelled(fd_ctx* ctx, const char* who, const float* a, int na, const int* ya, const int* order, const int* class_start,
                      int K, const float* mean, const float* inv_std, uint64_t seed, uint64_t offset, int step, int B, int T, int C,
                      int Cn, float* x, int* label, int* idx, hipStream_t s) {
    if (int rc = ph_classes_check(ctx, who, K)) return rc;
    FD_REQUIRE(ctx, C >= 1 && Cn == (C > K ? C : K), "%s: Cn=%d must be max(C, K) = max(%d, %d): the network has one output channel per logit",
               who, Cn, C, K);
    if (int rc = ph_shape_check(ctx, who, B, T, Cn)) return rc;
    FD_REQUIRE(ctx, a && ya && mean && inv_std && x && label && idx, "%s: null pointer", who);
    FD_REQUIRE(ctx, (order == nullptr) == (class_start == nullptr), "%s: the balanced draw needs order and class_start together", who);
    FD_REQUIRE(ctx, na >= 1 && step >= 0, "%s: na=%d (>= 1, the pool is empty otherwise), step=%d (>= 0)", who, na, step);
    const uint64_t ctr0 = offset + (uint64_t)step * (uint64_t)fd_cdiv(B, 4);
    hipLaunchKernelGGL(k_posthoc_batch_labelled, dim3(B), dim3(PH_BLOCK), 0, s, a, (unsigned)na, ya, order, class_start, K, mean, inv_std,
                       seed, ctr0, (uint64_t)step * (uint64_t)B, T, C, Cn, x, label, idx);
    return FD_OK;
}

int ph_head_mc(fd_ctx* ctx, const char* who, const float* out, const int* label, int B, int T, int Cn, int K, double* logp, int* pred,
               float* loss, float* dout, double* nll, hipStream_t s) {
    if (int rc = ph_classes_check(ctx, who, K)) return rc;
    if (int rc = ph_shape_check(ctx, who, B, T, Cn)) return rc;
    FD_REQUIRE(ctx, Cn >= K, "%s: Cn=%d channels hold fewer than K=%d logits", who, Cn, K);
    FD_REQUIRE(ctx, out, "%s: null out", who);
    FD_REQUIRE(ctx, label || (!loss && !dout && !nll), "%s: loss, dout and nll need the labels", who);
    FD_REQUIRE(ctx, !loss || nll, "%s: loss adds up nll, the B doubles of the per-series terms, which is null", who);
    FD_REQUIRE(ctx, logp || pred || dout || nll, "%s: every output is null", who);
    hipLaunchKernelGGL(k_posthoc_head_mc, dim3(B), dim3(PH_BLOCK), 0, s, out, label, T, Cn, K, 1.0 / (double)B, logp, pred, dout, nll);
    // mean_b nll[b] in the order of the predict task's sum
    if (loss) hipLaunchKernelGGL(k_posthoc_loss, dim3(1), dim3(PH_BLOCK), 0, s, 1, nll, label, B, 1.0 / (double)B, loss);
    return FD_OK;
}

// What both fits ask of the model and of the loop's arguments, in the order fd_posthoc_fit has always asked it.
int ph_fit_check(fd_score* m, const char* who, const char* ws_name, bool pointers, const float* params, int first_step, int steps, int B,
                 float lr, float max_norm, const int* idx_trace, const void* work, size_t work_bytes) {
    fd_ctx* ctx = m->ctx;
    if (m->backbone != FD_BACKBONE_LSTM)
        return fd_fail(ctx, FD_ERR_UNSUPPORTED, "%s: the post-hoc network is the causal LSTM backbone (its output at time t sees "
                       "inputs <= t only); this model's backbone is %s", who, m->backbone == FD_BACKBONE_MLP ? "the MLP" : "the transformer");
    const int T = m->d.max_len, C = m->d.n_channels;
    FD_REQUIRE(ctx, pointers, "%s: null pointer", who);
    if (!m->prepared) return fd_fail(ctx, FD_ERR_STATE, "%s: call fd_score_prepare first", who);
    FD_REQUIRE(ctx, params == m->params, "%s: params is not the buffer fd_score_prepare bound", who);
    FD_REQUIRE(ctx, first_step >= 0 && steps >= 1 && (long long)first_step + steps < (1ll << 31), "%s: first_step=%d (>= 0), steps=%d (>= 1)",
               who, first_step, steps);
    FD_REQUIRE(ctx, lr > 0.f && lr == lr && max_norm == max_norm, "%s: lr=%g must be positive, max_norm=%g a number (<= 0: no clipping)", who,
               (double)lr, (double)max_norm);
    if (int rc = ph_shape_check(ctx, who, B, T, C)) return rc;
    FD_REQUIRE(ctx, !idx_trace || (long long)steps * B < (1ll << 31), "%s: steps * B = %lld indices to trace, at most 2^31", who,
               (long long)steps * B);
    const size_t need = ph_carve(nullptr, B, T, C).bytes;
    FD_REQUIRE(ctx, work && work_bytes >= need, "%s: workspace of %zu bytes, %s asks for %zu", who, work ? work_bytes : 0, ws_name, need);
    return FD_OK;
}

// The loop both fits share.  batch(w, step, idx) fills w.x, w.label and idx; head(w, k) reads w.out and writes loss_trace[k] and w.dout.
template <class Batch, class Head>
int ph_fit_steps(fd_score* m, float* params, float* grads, float* exp_avg, float* exp_avg_sq, int first_step, int steps, int B, float lr,
                 float max_norm, int* idx_trace, void* work, void* stream, Batch batch, Head head) {
    fd_ctx* ctx = m->ctx;
    hipStream_t s = (hipStream_t)stream;
    const PhWork w = ph_carve((char*)(((uintptr_t)work + 255) & ~(uintptr_t)255), B, m->d.max_len, m->d.n_channels);
    // the backbone never sees a diffusion time other than 0: its time embedding is one more learned constant per feature
    FD_HIP(ctx, hipMemsetAsync(w.t, 0, (size_t)B * sizeof(float), s));
    const bool clip = max_norm > 0.f;
    const int64_t fz0 = m->tW, fz1 = m->tW + (m->d.d_model + 1) / 2;      // time_encoder.W is not trained
    for (int k = 0; k < steps; ++k) {
        const int step = first_step + k;
        int* idx = idx_trace ? idx_trace + (size_t)k * B : w.idx;
        if (int rc = batch(w, step, idx)) return rc;
        if (int rc = fd_score_forward_train(m, w.x, w.t, w.out, B, 0.f, 0, 0, stream)) return rc;
        if (int rc = head(w, k)) return rc;
        if (int rc = fd_score_backward(m, w.dout, grads, 0, stream)) return rc;
        if (clip)
            if (int rc = fd_grad_sqnorm(ctx, grads, m->nparams, w.sqnorm, stream)) return rc;
        // torch.optim.AdamW's defaults: betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2
        if (int rc = fd_adamw_step(ctx, params, grads, exp_avg, exp_avg_sq, m->nparams, step + 1, lr, 0.9f, 0.999f, 1e-8f, 1e-2f,
                                   clip ? w.sqnorm : nullptr, max_norm, 1.0f, fz0, fz1, stream))
            return rc;
    }
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

}  // namespace

extern "C" int fd_posthoc_batch(fd_ctx* ctx, int task, const float* a, int na, const float* b, int nb, const float* mean,
                                const float* inv_std, uint64_t seed, uint64_t offset, int step, int B, int T, int C, float* x,
                                int* label, int* idx, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    if (int rc = ph_batch(ctx, "fd_posthoc_batch", task, a, na, b, nb, mean, inv_std, seed, offset, step, B, T, C, x, label, idx,
                          (hipStream_t)stream))
        return rc;
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_posthoc_head(fd_ctx* ctx, int task, const float* out, const float* x, const int* label, int B, int T, int C,
                               float* loss, float* dout, double* per_series, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    if (int rc = ph_head(ctx, "fd_posthoc_head", task, out, x, label, B, T, C, loss, dout, per_series, (hipStream_t)stream)) return rc;
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_posthoc_fit_workspace_bytes(fd_ctx* ctx, int B, int T, int C, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_posthoc_fit_workspace_bytes: null pointer");
    if (int rc = ph_shape_check(ctx, "fd_posthoc_fit_workspace_bytes", B, T, C)) return rc;
    *bytes = ph_carve(nullptr, B, T, C).bytes;
    return FD_OK;
}


extern "C" int fd_posthoc_fit(fd_score* m, int task, float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* a,
                              int na, const float* b, int nb, const float* mean, const float* inv_std, uint64_t seed, uint64_t offset,
                              int first_step, int steps, int B, float lr, float max_norm, float* loss_trace, int* idx_trace,
                              void* work, size_t work_bytes, void* stream) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    const char* who = "fd_posthoc_fit";
    if (int rc = ph_fit_check(m, who, "fd_posthoc_fit_workspace_bytes", params && grads && exp_avg && exp_avg_sq && loss_trace, params,
                              first_step, steps, B, lr, max_norm, idx_trace, work, work_bytes))
        return rc;
    const int T = m->d.max_len, C = m->d.n_channels;
    hipStream_t s = (hipStream_t)stream;
    return ph_fit_steps(
        m, params, grads, exp_avg, exp_avg_sq, first_step, steps, B, lr, max_norm, idx_trace, work, stream,
        [&](const PhWork& w, int step, int* idx) {
            return ph_batch(ctx, who, task, a, na, b, nb, mean, inv_std, seed, offset, step, B, T, C, w.x, w.label, idx, s);
        },
        [&](const PhWork& w, int k) { return ph_head(ctx, who, task, w.out, w.x, w.label, B, T, C, loss_trace + k, w.dout, w.per_series, s); });
}

extern "C" int fd_posthoc_batch_labelled(fd_ctx* ctx, const float* a, int na, const int* ya, const int* order, const int* class_start,
                                         int K, const float* mean, const float* inv_std, uint64_t seed, uint64_t offset, int step,
                                         int B, int T, int C, int Cn, float* x, int* label, int* idx, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    if (int rc = ph_batch_labelled(ctx, "fd_posthoc_batch_labelled", a, na, ya, order, class_start, K, mean, inv_std, seed, offset, step, B,
                                   T, C, Cn, x, label, idx, (hipStream_t)stream))
        return rc;
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_posthoc_head_multiclass(fd_ctx* ctx, const float* out, const int* label, int B, int T, int Cn, int K, double* logp,
                                          int* pred, float* loss, float* dout, double* nll, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    if (int rc = ph_head_mc(ctx, "fd_posthoc_head_multiclass", out, label, B, T, Cn, K, logp, pred, loss, dout, nll, (hipStream_t)stream))
        return rc;
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

extern "C" int fd_posthoc_fit_multiclass_workspace_bytes(fd_ctx* ctx, int B, int T, int Cn, size_t* bytes) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, bytes, "fd_posthoc_fit_multiclass_workspace_bytes: null pointer");
    if (int rc = ph_shape_check(ctx, "fd_posthoc_fit_multiclass_workspace_bytes", B, T, Cn)) return rc;
    *bytes = ph_carve(nullptr, B, T, Cn).bytes;
    return FD_OK;
}

extern "C" int fd_posthoc_fit_multiclass(fd_score* m, int K, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                                         const float* a, int na, const int* ya, const int* order, const int* class_start, int C,
                                         const float* mean, const float* inv_std, uint64_t seed, uint64_t offset, int first_step,
                                         int steps, int B, float lr, float max_norm, float* loss_trace, int* idx_trace, void* work,
                                         size_t work_bytes, void* stream) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    const char* who = "fd_posthoc_fit_multiclass";
    if (int rc = ph_fit_check(m, who, "fd_posthoc_fit_multiclass_workspace_bytes", params && grads && exp_avg && exp_avg_sq && loss_trace,
                              params, first_step, steps, B, lr, max_norm, idx_trace, work, work_bytes))
        return rc;
    const int T = m->d.max_len, Cn = m->d.n_channels;
    hipStream_t s = (hipStream_t)stream;
    return ph_fit_steps(
        m, params, grads, exp_avg, exp_avg_sq, first_step, steps, B, lr, max_norm, idx_trace, work, stream,
        [&](const PhWork& w, int step, int* idx) {
            return ph_batch_labelled(ctx, who, a, na, ya, order, class_start, K, mean, inv_std, seed, offset, step, B, T, C, Cn, w.x, w.label,
                                     idx, s);
        },
        [&](const PhWork& w, int k) {
            return ph_head_mc(ctx, who, w.out, w.label, B, T, Cn, K, nullptr, nullptr, loss_trace + k, w.dout, w.per_series, s);
        });
}

extern "C" int fd_posthoc_confusion(fd_ctx* ctx, const int* label, const int* pred, int n, int K, int* counts, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    const char* who = "fd_posthoc_confusion";
    if (int rc = ph_classes_check(ctx, who, K)) return rc;
    FD_REQUIRE(ctx, label && pred && counts, "%s: null pointer", who);
    FD_REQUIRE(ctx, n >= 1, "%s: n=%d pairs (>= 1)", who, n);
    hipLaunchKernelGGL(k_posthoc_confusion, dim3(K), dim3(PH_BLOCK), 0, (hipStream_t)stream, label, pred, n, K, counts);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}
