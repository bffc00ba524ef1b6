// fd_aggregate.h -- conditional sampling on window-mean observations (fd_aggregate.hip): what the host loops of fd_impute.hip and
// fd_dps.hip hand to the aggregate kernels.  The loops, their Philox counters and every buffer are those of the mask path; only the
// kernel between the score evaluation and the next step changes.
#pragma once
#include "fd_common.h"
#include "fd_sde.h"

// The window geometry of one (T, window): J = ceil(T / window) windows, window j = [j w, min((j + 1) w, T)), Jp = 16 ceil(J / 16).
// basis (fourier only): A_w = P F^T (Jp x Tp) then B_w = F P^+ (Tp x Jp), both row-major, zero outside (J, T); cached on the
// context under a key of (T, window).
struct fd_agg_plan {
    int window, J, Jp;
    const float* basis;
};

// window in [2, T] (window = 1 is the mask path: the callers forward it), T <= 1024 in both domains (the LDS images of one series)
int fd_agg_prepare(fd_ctx* ctx, int T, int Tp, int window, int fourier, hipStream_t s, fd_agg_plan* out, const char* who);

// k_impute_agg: the fields of fd_impute.hip's ImpArgs; mask (B/obs_rep,J,C) or (J,C), stdv read in both domains
struct fd_agg_imp_args {
    const float *x, *score, *zstep, *x0;
    const uint8_t* mask;
    const float *stdv, *G, *zobs;
    float* out;
    int B, T, C, Tp, ncb, mask_per_series, obs_rep;
    SdeCoef cf;
    float alpha, s;
    uint64_t seed, off_step, off_obs;
    fd_agg_plan p;
};
int fd_agg_launch_impute(fd_ctx* ctx, const fd_agg_imp_args& a, bool step, bool fourier, hipStream_t s);

// k_dps_residual_agg: the fields of fd_dps.hip's ResArgs; part (B, ncb)
struct fd_agg_res_args {
    const float *x, *score, *x0;
    const uint8_t* mask;
    const float *stdv, *G;
    float *u, *dout;
    double* part;
    int T, C, Tp, ncb, mask_per_series, obs_rep;
    float alpha, s2;
    fd_agg_plan p;
};
int fd_agg_launch_residual(fd_ctx* ctx, const fd_agg_res_args& r, int B, bool fourier, hipStream_t s);
