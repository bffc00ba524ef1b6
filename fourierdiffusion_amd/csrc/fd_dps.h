// fd_dps.h -- the host pieces of one guidance evaluation (fd_dps.hip), shared with the particle filter built around them
// (fd_smc.hip): the arguments of k_dps_residual, the stage buffers of a run, and the evaluation itself.
#pragma once
#include "fd_aggregate.h"
#include "fd_loop.h"
#include "fd_score.h"

// the arguments of k_dps_residual (notation of fd_dps.hip)
struct fd_dps_res {
    const float* x;          // (B,T,C) state x_i
    const float* score;      // (B,T,C) s_theta(x_i, t_i)
    const float* x0;         // (B/obs_rep,T,C) A^-1(where(m, y, 0))
    const uint8_t* mask;     // (B/obs_rep,M,C) or (M,C), 1 = observed, over the operator's M rows (time steps / windows)
    const float* stdv;       // (T,C) feature std or nullptr (= 1)
    const float* G;          // (T)
    const float* basis;      // the operator's pair: F then F^T (Tp x Tp each), or A_w (Jp x Tp) then B_w (Tp x Jp); FOURIER only
    float* u;                // (B,T,C)
    float* dout;             // (B,T,C) s^2 G^2 u, or nullptr (no Jacobian)
    double* part;            // (B, ncb) sum r^2 of each channel block
    int T, C, Tp, ncb, mask_per_series, obs_rep;
    float alpha, s2;
};

// the stage buffers of one run (fd_ll_carve: outside the arena).  R: the rows of a forward (B, or 2B for a paired guide, whose label
// vector lab and -- fd_impute_guidance_cfg, whose x is the caller's -- state copy xpair follow the unpaired layout)
struct fd_dps_bufs {
    float *tvec, *score, *u, *dout, *dx;
    double* part;
    int* lab;
    float* xpair;
};
// the shares of the buffers above, in order, through take (the layout of fd_ll_carve); a caller with buffers of its own takes them
// behind these in the same carve
template <class Take>
void fd_dps_take(Take& take, int B, int R, size_t n, int ncb, bool jac, bool xpair, fd_dps_bufs* o) {
    const size_t nR = n / B * R;
    o->tvec = (float*)take(R * sizeof(float));
    o->score = (float*)take(nR * sizeof(float));
    o->u = (float*)take(n * sizeof(float));
    o->dout = jac ? (float*)take(nR * sizeof(float)) : nullptr;
    o->dx = jac ? (float*)take(nR * sizeof(float)) : nullptr;
    o->part = (double*)take((size_t)B * ncb * sizeof(double));
    o->lab = R != B ? (int*)take((size_t)R * sizeof(int)) : nullptr;
    o->xpair = xpair ? (float*)take(nR * sizeof(float)) : nullptr;
}
int fd_dps_buffers(fd_ctx* ctx, int B, int R, size_t n, int ncb, bool jac, bool xpair, fd_dps_bufs* o);

// checks and fills the conditioning / geometry fields shared by every entry
int fd_dps_prepare(fd_score* m, fd_dps_res& r, const float* G, const float* x, const float* x0, const uint8_t* mask,
                   int mask_per_series, const float* stdv, int fourier, int B, int obs_replicas, hipStream_t s, const char* who);
// One guidance evaluation at (x, tvec) on R network rows (B, or 2B under a paired guide g): the score (training forward with the
// Jacobian, else the sampler's forward), the residual of the B state rows, and the VJP; leaves score, u, dx and the block sums in
// the buffers
int fd_dps_eval(fd_score* m, fd_dps_res& r, const fd_dps_bufs& bf, const float* x, int B, int R, const fd_guide* g, bool jac,
                bool fourier, int mode, hipStream_t s, const fd_agg_plan* ag = nullptr, const fdproj::DenseOp* dn = nullptr);
// the residual of the B state rows alone, from the x and score r points at (no network evaluation)
int fd_dps_residual(fd_ctx* ctx, const fd_dps_res& r, int B, bool fourier, hipStream_t s);
