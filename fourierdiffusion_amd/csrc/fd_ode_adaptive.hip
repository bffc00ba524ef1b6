// fd_ode_adaptive.hip -- the probability-flow ODE of fd_ode.hip under per-row Dormand-Prince 5(4) step control (scipy's RK45; Song et
// al. 2021's black-box sampler; not in the reference): sampling / decoding (t0 > t1) and encoding (t0 < t1) to a tolerance instead
// of a step count.  Every row b of x (B,T,C) is one ODE on its T*C values,
//   dx/dt = v(x, t) = -a x - 0.5 (g G_k)^2 s(x, t)
// on its own grid, with the controller of fd_likelihood_run_adaptive (fd_likelihood.hip: select_initial_step, min_step, the RMS
// error norm -- here over the T*C values alone --, SAFETY / MIN_FACTOR / MAX_FACTOR) and scipy's `direction` handling added:
// t_new = t + direction h_abs, clamped when direction (t_new - t_bound) > 0, min_step = 10 |nextafter(t, direction inf) - t|.
// The arithmetic is k_ll_rk_stage's: the controller float64 per row (thread 0 of the row's workgroup), x and the 7 stage vectors
// fp32 with their combinations formed in float64, a and g from the float64 stage time, the network reading (float) t_stage.  The score
// evaluation is the sampler's forward (fd_score_forward_any), not the training one: no VJP, so the forward scratch is all the arena
// holds and the loop's buffers sit outside it (fd_ll_carve).
//
// Compaction.  Rows freeze (converged, step too small, evaluation cap) at different attempts; the network runs on the running rows
// only.  k_ode_rk_stage addresses its row through a slot -> row list, and the network input, its t vector and the score are indexed by
// slot.  The host reads the count of running rows one attempt late (the pinned word of the likelihood loop), so what it knows is
// an upper bound -- rows only ever freeze; when that bound is below the launched slots by at least a granule, k_ode_repack_list
// rebuilds the list from the row statuses (ascending by row, one workgroup, no atomics; -1 beyond the true count),
// k_ode_repack_move moves the pending inputs to their new slots in the SECOND input buffer, and every later forward and stage
// launch has that many slots.  The evaluations a row sees do not depend on any of it.
// Guided loops (a non-null fd_guide) and calls that find labels or covariates bound to the model run UNCOMPACTED: the label vector of
// a forward is indexed by network row, and this loop does not permute it.
#include <cmath>
#include <cstdlib>

#include "fd_engine.h"
#include "fd_loop.h"
#include "fd_mega_params.h"
#include "fd_sde.h"

namespace {

constexpr int kBlock = 256;
// The default compaction granule in rows (0: off), by measurement at T = 100, C = 12, B = 200: the transformer's exact-f32
// forward costs in proportion to its rows and granule 1 was the fastest (-6.7 % wall time at rtol = 1e-5); the bf16 forward is
// latency-bound there, compaction saved 9 % of the row-evaluations and no time, so it ships off -- as it does for the backbones it
// was not measured on.
constexpr int kDefaultGranuleF32 = 1, kDefaultGranuleOther = 0;

enum RkStage { RK_INIT0 = -2, RK_INIT1 = -1, RK_FINAL = 6 };      // 1..5: the interior stages of an attempt
enum RkStatus { RK_RUNNING = 0, RK_CONVERGED = 1, RK_TOO_SMALL = 2, RK_MAX_EVALS = 3 };      // fd_likelihood_run_adaptive's

// Dormand & Prince (1980), as fd_likelihood.hip (whose kernels and constants stay as they are)
__constant__ double kC[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
__constant__ double kA[6][5] = {{0, 0, 0, 0, 0},
                                {1.0 / 5, 0, 0, 0, 0},
                                {3.0 / 40, 9.0 / 40, 0, 0, 0},
                                {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
                                {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
                                {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__constant__ double kB5[6] = {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
__constant__ double kE[7] = {-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
constexpr double kSafety = 0.9, kMinFactor = 0.2, kMaxFactor = 10.0, kErrExp = -1.0 / 5;

struct OdeRow {
    double t;          // last accepted time
    double t_eval;     // time of the row's next evaluation
    double h_abs;      // step magnitude (scipy's h_abs)
    double h;          // signed step of the current attempt (t_new - t)
    double t_new;      // end of the current attempt
    double min_step;   // 10 ulp(t), towards t_bound
    double h0, d1;     // select_initial_step
    int status, nfe, n_grid, rejected;
};

struct OdeArgs {
    const float* G;
    float* x;              // (B,T,C) last accepted state, in place; by row
    float* xin;            // (slots,T,C) the network input of the next evaluation; by slot
    const float* score;    // (slots,T,C) s(xin, tvec); by slot
    float* K;              // 7 (B,T,C) stage vectors, K_j at K + j * n; by row
    float* tvec;           // (slots,) the time the forward reads
    OdeRow* row;           // (B,)
    double* grid;          // (B, gcap) accepted times, t0 first
    const int* slot_row;   // (launched slots,) the row of a slot, -1: none
    size_t n;              // B*T*C
    size_t half;           // paired guide: the second half of xin / score starts here (= n; its t vector at tvec + B); else 0
    int B, T, C, gcap, max_evals;
    fd_sde_params sde;
    double t_bound, dir, rtol, atol;
    float w, omw;          // paired guide: the scale and 1 - w
    int stage;
};

// sum over the block's threads in a fixed order (LDS tree); the result is valid in every thread
__device__ __forceinline__ double block_sum(double v, double* red) {
    __syncthreads();      // (red may still be read from the sum before)
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// a(t), g(t) of fd_sde_coef (rounded to float as there) from a float64 t: rk_coef of fd_likelihood.hip
__device__ __forceinline__ void ode_coef(const fd_sde_params& p, double t, float* a, float* g) {
    if (p.kind == 0) {
        const double beta = (double)p.p0 + t * ((double)p.p1 - (double)p.p0);
        *a = (float)(0.5 * beta);
        *g = (float)sqrt(beta);
    } else {
        const double r = (double)p.p1 / (double)p.p0;
        *a = 0.f;
        *g = (float)((double)p.p0 * sqrt(2.0 * log(r)) * pow(r, t));
    }
}

// scipy's RungeKutta._step_impl from the top of its retry loop (thread 0): freeze the row or set up the attempt's first stage;
// returns whether the row still runs
__device__ bool rk_attempt(OdeRow& r, const OdeArgs& p) {
    if (r.h_abs < r.min_step) { r.status = RK_TOO_SMALL; return false; }
    if (r.nfe + 6 > p.max_evals) { r.status = RK_MAX_EVALS; return false; }
    r.nfe += 6;
    double t_new = r.t + p.dir * r.h_abs;
    if (p.dir * (t_new - p.t_bound) > 0.0) t_new = p.t_bound;
    r.h = t_new - r.t;
    r.h_abs = fabs(r.h);
    r.t_new = t_new;
    r.t_eval = r.t + kC[1] * r.h;
    return true;
}
// the start of a new step from the accepted time r.t
__device__ bool rk_new_step(OdeRow& r, const OdeArgs& p) {
    r.min_step = 10.0 * fabs(nextafter(r.t, p.dir * (double)INFINITY) - r.t);
    if (r.h_abs < r.min_step) r.h_abs = r.min_step;
    r.rejected = 0;
    return rk_attempt(r, p);
}

// slot b = row b: the first input is the state itself (both halves of a pair), at t0
__global__ __launch_bounds__(kBlock) void k_ode_rk_init(OdeArgs p, double t0, int* __restrict__ slot_row, int* __restrict__ row_slot) {
    const int b = blockIdx.x, n_row = p.T * p.C;
    const size_t base = (size_t)b * n_row;
    for (int i = threadIdx.x; i < n_row; i += kBlock) {
        const float v = p.x[base + i];
        p.xin[base + i] = v;
        if (p.half) p.xin[p.half + base + i] = v;
    }
    if (threadIdx.x != 0) return;
    OdeRow& r = p.row[b];
    r.t = r.t_eval = r.t_new = t0;
    r.h_abs = r.h = r.h0 = r.d1 = r.min_step = 0.0;
    r.status = RK_RUNNING;
    r.nfe = 0;
    r.rejected = 0;
    r.n_grid = 1;
    p.grid[(size_t)b * p.gcap] = t0;
    p.tvec[b] = (float)t0;
    if (p.half) p.tvec[p.B + b] = (float)t0;
    slot_row[b] = b;
    row_slot[b] = b;
}

// One workgroup per slot: consumes the evaluation (score) at (xin, t_eval) as stage p.stage of the slot's row, writes the next input.
//   INIT0  f0 = K_0;  d0, d1 of select_initial_step;  next input y0 + direction h0 f0
//   INIT1  f1;  d2, h_abs;  nfe = 2;  first attempt: next input y + h A_10 K_0
//   1..5   K_s;  next input y + h sum_j A_{s+1,j} K_j  (stage 5: y_new = y + h sum_j B_j K_j, at t_new)
//   FINAL  K_6 = f(t_new, y_new);  error norm over the T*C values;  accept (x = y_new, K_0 = K_6, grid) or reject;  next attempt's
//          first input
// A slot without a row (-1) and a frozen row return at once (input and time stay as they were).  Paired guide: the score is
// fd_guided of the two halves, the next input and its time go to both.  Reductions: block_sum, fixed order, float64.
// The row record (status, t_eval, h) is read by all threads at the top and updated by thread 0 alone, behind a barrier that every
// stage passes.
__global__ __launch_bounds__(kBlock) void k_ode_rk_stage(OdeArgs p) {
    __shared__ double red[kBlock];
    __shared__ double bc[3];      // broadcast from thread 0: the factor of the next input, flags, the attempt's step
    const int slot = blockIdx.x;
    const int b = p.slot_row[slot];
    if (b < 0) return;
    OdeRow* rp = p.row + b;
    if (rp->status != RK_RUNNING) return;
    const int n_row = p.T * p.C, st = p.stage;
    const size_t base = (size_t)b * n_row, sbase = (size_t)slot * n_row, n = p.n, half = p.half;
    float a, g;
    ode_coef(p.sde, rp->t_eval, &a, &g);
    const double h = rp->h;
    float* K = p.K;
    double q0 = 0.0, q1 = 0.0;
    for (int i = threadIdx.x; i < n_row; i += kBlock) {
        const size_t e = base + i, se = sbase + i;
        const float xi = p.xin[se];
        const float sc = half ? fd_guided(p.score[se], p.score[half + se], p.w, p.omw) : p.score[se];
        const float v = fd_ode_velocity(xi, sc, a, g * p.G[i / p.C]);
        const double y = (double)p.x[e];
        float nxt = xi;
        if (st == RK_INIT0) {
            K[e] = v;
            const double s = p.atol + fabs(y) * p.rtol;
            q0 += (y / s) * (y / s);
            q1 += ((double)v / s) * ((double)v / s);
        } else if (st == RK_INIT1) {
            const double s = p.atol + fabs(y) * p.rtol;
            const double d = ((double)v - (double)K[e]) / s;
            q0 += d * d;
        } else if (st < 5) {
            K[st * n + e] = v;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (j <= st) s += kA[st + 1][j] * (double)(j == st ? v : K[j * n + e]);
            nxt = (float)(y + s * h);
        } else if (st == 5) {
            K[5 * n + e] = v;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) s += (double)(j == 5 ? v : K[j * n + e]) * kB5[j];
            nxt = (float)(y + h * s);
        } else {
            K[6 * n + e] = v;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) s += (double)(j == 6 ? v : K[j * n + e]) * kE[j];
            const double err = s * h;
            const double scl = p.atol + fmax(fabs(y), fabs((double)xi)) * p.rtol;
            q0 += (err / scl) * (err / scl);
        }
        if (st >= 1 && st <= 5) {
            p.xin[se] = nxt;
            if (half) p.xin[half + se] = nxt;
        }
    }
    if (st == RK_INIT0 || st == RK_INIT1 || st == RK_FINAL) q0 = block_sum(q0, red);
    if (st == RK_INIT0) q1 = block_sum(q1, red);
    __syncthreads();      // every thread has read the row record (status, t_eval, h) before thread 0 updates it: the interior stages
                          // have no reduction, hence no other barrier
    if (threadIdx.x == 0) {
        OdeRow& R = *rp;
        const double dims = (double)n_row;
        const double interval = fabs(p.t_bound - R.t);
        double fac = 0.0;
        int flags = 0;      // bit 0: write the next input from (x, K_0), bit 1: accept (x = y_new, K_0 = K_6) first
        if (st == RK_INIT0) {
            const double d0 = sqrt(q0 / dims), d1 = sqrt(q1 / dims);
            double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
            h0 = fmin(h0, interval);
            R.h0 = h0;
            R.d1 = d1;
            R.t_eval = R.t + h0 * p.dir;
            fac = h0 * p.dir;
            flags = 1;
        } else if (st == RK_INIT1) {
            const double d2 = sqrt(q0 / dims) / R.h0;
            const double h1 = (R.d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, R.h0 * 1e-3) : pow(0.01 / fmax(R.d1, d2), 1.0 / 5);
            R.h_abs = fmin(fmin(100 * R.h0, h1), interval);
            R.nfe = 2;
            if (rk_new_step(R, p)) { fac = kA[1][0]; flags = 1; }
        } else if (st < 5) {
            R.t_eval = R.t + kC[st + 1] * h;
        } else if (st == 5) {
            R.t_eval = R.t + h;      // (scipy evaluates f_new at t + h, not at t_new)
        } else {
            const double en = sqrt(q0 / dims);
            if (en < 1.0) {
                double factor = en == 0.0 ? kMaxFactor : fmin(kMaxFactor, kSafety * pow(en, kErrExp));
                if (R.rejected) factor = fmin(1.0, factor);
                R.h_abs *= factor;
                R.t = R.t_new;
                if (R.n_grid < p.gcap) p.grid[(size_t)b * p.gcap + R.n_grid++] = R.t;
                flags = 2;
                if (p.dir * (R.t - p.t_bound) >= 0.0) R.status = RK_CONVERGED;
                else if (rk_new_step(R, p)) { fac = kA[1][0]; flags |= 1; }
            } else {
                R.h_abs *= fmax(kMinFactor, kSafety * pow(en, kErrExp));
                R.rejected = 1;
                if (rk_attempt(R, p)) { fac = kA[1][0]; flags = 1; }
            }
        }
        const float tf = (float)R.t_eval;
        p.tvec[slot] = tf;
        if (half) p.tvec[p.B + slot] = tf;
        bc[0] = fac;
        bc[1] = (double)flags;
        bc[2] = R.h;
    }
    if (st != RK_INIT0 && st != RK_INIT1 && st != RK_FINAL) return;
    __syncthreads();
    const int flags = (int)bc[1];
    if (flags == 0) return;
    const double fac = bc[0], hn = bc[2];      // (INIT0: the input y0 + direction h0 f0; else y + (A_10 K_0) h)
    for (int i = threadIdx.x; i < n_row; i += kBlock) {
        const size_t e = base + i, se = sbase + i;
        float xv = p.x[e], k0 = K[e];
        if (flags & 2) {      // accepted: y = y_new (the input of the last stage), K_0 = K_6 (FSAL)
            xv = p.xin[se];
            k0 = K[6 * n + e];
            p.x[e] = xv;
            K[e] = k0;
        }
        if (flags & 1) {
            const float nxt = st == RK_INIT0 ? (float)((double)xv + fac * (double)k0) : (float)((double)xv + fac * (double)k0 * hn);
            p.xin[se] = nxt;
            if (half) p.xin[half + se] = nxt;
        }
    }
}

// out[0] = the number of running rows (one workgroup)
__global__ __launch_bounds__(kBlock) void k_ode_rk_count(const OdeRow* __restrict__ row, int B, int* __restrict__ out) {
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

// list[0 .. B): the running rows in ascending order, then -1 (one workgroup: thread i owns the rows [i chunk, (i + 1) chunk), the
// offsets are a serial scan of the 256 counts -- deterministic, no atomics)
__global__ __launch_bounds__(kBlock) void k_ode_repack_list(const OdeRow* __restrict__ row, int B, int* __restrict__ list) {
    __shared__ int off[kBlock + 1];
    const int chunk = (B + kBlock - 1) / kBlock;
    const int lo = min(B, (int)threadIdx.x * chunk), hi = min(B, lo + chunk);
    int c = 0;
    for (int b = lo; b < hi; ++b) c += row[b].status == RK_RUNNING;
    off[threadIdx.x + 1] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        off[0] = 0;
        for (int i = 1; i <= kBlock; ++i) off[i] += off[i - 1];
    }
    __syncthreads();
    int pos = off[threadIdx.x];
    for (int b = lo; b < hi; ++b)
        if (row[b].status == RK_RUNNING) list[pos++] = b;
    for (int i = off[kBlock] + threadIdx.x; i < B; i += kBlock) list[i] = -1;
}

// One workgroup per NEW slot: the pending input and time of its row move from the row's old slot (row_slot) in the old buffers to the
// new slot in the new ones; a slot without a row gets a finite input (zeros at t_fill), which no row reads
__global__ __launch_bounds__(kBlock) void k_ode_repack_move(const int* __restrict__ list, int* __restrict__ row_slot,
                                                              const float* __restrict__ xin_old, float* __restrict__ xin_new,
                                                              const float* __restrict__ tvec_old, float* __restrict__ tvec_new, int n_row,
                                                              float t_fill) {
    const int slot = blockIdx.x, b = list[slot];
    float* dst = xin_new + (size_t)slot * n_row;
    if (b < 0) {
        for (int i = threadIdx.x; i < n_row; i += kBlock) dst[i] = 0.f;
        if (threadIdx.x == 0) tvec_new[slot] = t_fill;
        return;
    }
    const int old = row_slot[b];
    __syncthreads();      // every thread has read the old slot before thread 0 replaces it
    const float* src = xin_old + (size_t)old * n_row;
    for (int i = threadIdx.x; i < n_row; i += kBlock) dst[i] = src[i];
    if (threadIdx.x == 0) {
        tvec_new[slot] = tvec_old[old];
        row_slot[b] = slot;
    }
}

// the per-row results: nfe_out, status_out, and the grid NaN-padded to grid_cap (grid_out may be null)
__global__ __launch_bounds__(kBlock) void k_ode_rk_out(const OdeRow* __restrict__ row, const double* __restrict__ grid, int gcap,
                                                         int* __restrict__ nfe_out, int* __restrict__ status_out,
                                                         double* __restrict__ grid_out, int grid_cap) {
    const int b = blockIdx.x;
    const OdeRow& r = row[b];
    if (threadIdx.x == 0) {
        nfe_out[b] = r.nfe;
        status_out[b] = r.status;
    }
    if (!grid_out) return;
    for (int i = threadIdx.x; i < grid_cap; i += kBlock)
        grid_out[(size_t)b * grid_cap + i] = (i < r.n_grid && i < gcap) ? grid[(size_t)b * gcap + i] : __longlong_as_double(0x7ff8000000000000LL);      // NaN (bits: -fno-honor-nans)
}

// the state of one run, in the grow-only buffer of the likelihood loops (outside the arena); R: the rows of a forward (B, or 2B for a
// paired guide, whose label vector comes last)
struct OdeBufs {
    float *tvec[2], *xin[2], *score, *K;
    OdeRow* row;
    double* grid;
    int *list[2], *row_slot, *count;
    void* lab;
};
int ode_buffers(fd_ctx* ctx, int B, int R, size_t n_row, int gcap, size_t guide_bytes, OdeBufs* o) {
    return fd_ll_carve(ctx, [&](auto take) {
        for (int i = 0; i < 2; ++i) o->tvec[i] = (float*)take(R * sizeof(float));
        for (int i = 0; i < 2; ++i) o->xin[i] = (float*)take(R * n_row * sizeof(float));
        o->score = (float*)take(R * n_row * sizeof(float));
        o->K = (float*)take(7 * B * n_row * sizeof(float));
        o->row = (OdeRow*)take(B * sizeof(OdeRow));
        o->grid = (double*)take((size_t)B * gcap * sizeof(double));
        for (int i = 0; i < 2; ++i) o->list[i] = (int*)take(B * sizeof(int));
        o->row_slot = (int*)take(B * sizeof(int));
        o->count = (int*)take(sizeof(int));
        o->lab = guide_bytes ? (void*)take(guide_bytes) : nullptr;
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

// the compaction granule in rows (0: off): FDIFF_RK_COMPACT=0 turns it off, else the argument (> 0), else FDIFF_RK_COMPACT_GRANULE
// (> 0), else the default dflt
int compact_granule(int arg, int dflt) {
    const char* on = getenv("FDIFF_RK_COMPACT");
    if (on && atoi(on) == 0) return 0;
    if (arg > 0) return arg;
    const char* e = getenv("FDIFF_RK_COMPACT_GRANULE");
    if (e && atoi(e) > 0) return atoi(e);
    return dflt;
}

int ode_adaptive_loop(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol, double atol,
                      int max_evals, float* x, int* nfe_out, int* status_out, double* grid_out, int grid_cap, int granule_arg,
                      long long* row_evals_out, int B, int mode, hipStream_t s, const fd_guide* g, const char* who) {
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, G && x && nfe_out && status_out, "%s: null pointer", who);
    FD_REQUIRE(ctx, std::isfinite(t0) && std::isfinite(t1) && t0 != t1, "%s: need finite t0 != t1 (%g, %g)", who, t0, t1);
    FD_REQUIRE(ctx, std::isfinite(rtol) && std::isfinite(atol) && rtol > 0 && atol > 0, "%s: need rtol > 0 and atol > 0 (%g, %g)", who,
               rtol, atol);
    FD_REQUIRE(ctx, max_evals >= 8, "%s: max_evals=%d < 8 (one step)", who, max_evals);
    FD_REQUIRE(ctx, granule_arg >= 0, "%s: compact_granule=%d", who, granule_arg);
    const int max_attempts = (max_evals - 2) / 6, gcap = 1 + max_attempts;
    FD_REQUIRE(ctx, !grid_out || grid_cap >= gcap, "%s: grid_cap=%d < 1 + (max_evals - 2) / 6 = %d", who, grid_cap, gcap);
    const int T = m->d.max_len, C = m->d.n_channels;
    const size_t n_row = (size_t)T * C, n = (size_t)B * n_row;
    const bool pair = g && g->pair;
    const int R0 = fd_guide_rows(g, B);
    // a forward's labels / covariates are indexed by network row: such a loop keeps every launch at B rows
    const bool f32 = mode == FD_MODE_F32 && m->backbone == FD_BACKBONE_TRANSFORMER;
    const int granule = (g || m->labels || m->cov) ? 0 : compact_granule(granule_arg, f32 ? kDefaultGranuleF32 : kDefaultGranuleOther);
    OdeBufs b;
    if (int rc = ode_buffers(ctx, B, R0, n_row, gcap, fd_guide_bytes(g, B), &b)) return rc;
    if (!ctx->ll_host) FD_HIP(ctx, hipHostMalloc((void**)&ctx->ll_host, 2 * sizeof(int), hipHostMallocDefault));
    RkEvents ev;
    for (hipEvent_t& e : ev.e) FD_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));

    OdeArgs a{};
    a.G = G; a.x = x; a.xin = b.xin[0]; a.score = b.score; a.K = b.K; a.tvec = b.tvec[0]; a.row = b.row; a.grid = b.grid;
    a.slot_row = b.list[0];
    a.n = n; a.half = pair ? n : 0;
    a.B = B; a.T = T; a.C = C; a.gcap = gcap; a.max_evals = max_evals;
    a.sde = *sde;
    a.t_bound = t1; a.dir = t1 > t0 ? 1.0 : -1.0; a.rtol = rtol; a.atol = atol;
    a.w = pair ? g->w : 0.f; a.omw = pair ? g->omw : 0.f;
    hipLaunchKernelGGL(k_ode_rk_init, dim3(B), dim3(kBlock), 0, s, a, t0, b.list[0], b.row_slot);
    FD_LAUNCH_CHECK(ctx);
    // the pair's labels (y, null tokens) or covariates; its copy of the state is a no-op here: k_ode_rk_init wrote both halves
    if (int rc = fd_guide_begin(m, g, b.lab, b.xin[0], B, s)) return rc;
    fd_guide_scope scope(m, g, b.lab, R0);

    int slots = B, cur = 0;      // the state slots of a launch (network rows: twice that for a pair), the buffers in use
    long long launched = 0;
    auto eval = [&](int stage) {
        if (int rc = fd_score_forward_any(m, a.xin, a.tvec, b.score, pair ? 2 * slots : slots, mode, s)) return rc;
        a.stage = stage;
        hipLaunchKernelGGL(k_ode_rk_stage, dim3(slots), dim3(kBlock), 0, s, a);
        FD_LAUNCH_CHECK(ctx);
        launched += slots;
        return (int)FD_OK;
    };
    if (int rc = eval(RK_INIT0)) return rc;
    if (int rc = eval(RK_INIT1)) return rc;
    // Attempt k (6 evaluations) ends with the count of the rows still running, copied to host word k % 2 and marked by event k % 2.
    // The host reads attempt k's count once attempt k + 1 is queued: the device never waits on the host, and at most one attempt
    // runs after the last row froze.  Every row freezes within max_attempts attempts (an attempt past max_evals is not started),
    // so the loop needs no other bound.  The count read is that of attempt k - 1: an upper bound of the rows running after attempt
    // k, which is where a repack lands in the stream.
    for (int k = 0; k < max_attempts; ++k) {
        for (int st = 1; st <= RK_FINAL; ++st)
            if (int rc = eval(st)) return rc;
        hipLaunchKernelGGL(k_ode_rk_count, dim3(1), dim3(kBlock), 0, s, b.row, B, b.count);
        FD_LAUNCH_CHECK(ctx);
        FD_HIP(ctx, hipMemcpyAsync(ctx->ll_host + (k & 1), b.count, sizeof(int), hipMemcpyDeviceToHost, s));
        FD_HIP(ctx, hipEventRecord(ev.e[k & 1], s));
        if (k == 0) continue;
        FD_HIP(ctx, hipEventSynchronize(ev.e[(k - 1) & 1]));
        const int running = ctx->ll_host[(k - 1) & 1];
        if (running <= 0) break;
        if (granule > 0 && running <= slots - granule) {
            const int nxt = cur ^ 1;
            hipLaunchKernelGGL(k_ode_repack_list, dim3(1), dim3(kBlock), 0, s, b.row, B, b.list[nxt]);
            hipLaunchKernelGGL(k_ode_repack_move, dim3(running), dim3(kBlock), 0, s, b.list[nxt], b.row_slot, b.xin[cur], b.xin[nxt],
                               b.tvec[cur], b.tvec[nxt], (int)n_row, (float)t1);
            FD_LAUNCH_CHECK(ctx);
            cur = nxt;
            slots = running;
            a.xin = b.xin[cur];
            a.tvec = b.tvec[cur];
            a.slot_row = b.list[cur];
        }
    }
    hipLaunchKernelGGL(k_ode_rk_out, dim3(B), dim3(kBlock), 0, s, b.row, b.grid, gcap, nfe_out, status_out, grid_out, grid_cap);
    FD_LAUNCH_CHECK(ctx);
    if (row_evals_out) *row_evals_out = launched;
    return FD_OK;
}

}  // namespace

extern "C" int fd_sampler_run_ode_adaptive(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol,
                                           double atol, int max_evals, float* x, int* nfe_out, int* status_out, double* grid_out,
                                           int grid_cap, int compact_granule, long long* row_evals_out, int B, int mode, void* stream) {
    const char* who = "fd_sampler_run_ode_adaptive";
    if (int rc = fd_loop_check(m, sde, B, mode, who)) return rc;
    return ode_adaptive_loop(m, sde, G, t0, t1, rtol, atol, max_evals, x, nfe_out, status_out, grid_out, grid_cap, compact_granule,
                             row_evals_out, B, mode, (hipStream_t)stream, nullptr, who);
}

extern "C" int fd_sampler_run_ode_adaptive_cfg(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol,
                                               double atol, int max_evals, float* x, const int32_t* y, float w, int* nfe_out,
                                               int* status_out, double* grid_out, int grid_cap, long long* row_evals_out, int B, int mode,
                                               void* stream) {
    const char* who = "fd_sampler_run_ode_adaptive_cfg";
    if (int rc = fd_loop_check(m, sde, B, mode, who)) return rc;
    if (int rc = fd_guide_check(m, w, who)) return rc;
    const fd_guide g = fd_guide_plan(y, w);
    return ode_adaptive_loop(m, sde, G, t0, t1, rtol, atol, max_evals, x, nfe_out, status_out, grid_out, grid_cap, 0, row_evals_out, B,
                             mode, (hipStream_t)stream, &g, who);
}

extern "C" int fd_sampler_run_ode_adaptive_cov(fd_score* m, const fd_sde_params* sde, const float* G, double t0, double t1, double rtol,
                                               double atol, int max_evals, float* x, const float* c, float w, int* nfe_out,
                                               int* status_out, double* grid_out, int grid_cap, long long* row_evals_out, int B, int mode,
                                               void* stream) {
    const char* who = "fd_sampler_run_ode_adaptive_cov";
    if (int rc = fd_loop_check(m, sde, B, mode, who)) return rc;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, m->cond_dim > 0, "%s: the model has no covariate encoder (fd_score_create_cov with cond_dim > 0)", who);
    FD_REQUIRE(ctx, std::isfinite(w), "%s: the guidance scale is not finite", who);
    const fd_guide g = fd_guide_plan_cov(c, m->cond_dim, w);
    return ode_adaptive_loop(m, sde, G, t0, t1, rtol, atol, max_evals, x, nfe_out, status_out, grid_out, grid_cap, 0, row_evals_out, B,
                             mode, (hipStream_t)stream, &g, who);
}
