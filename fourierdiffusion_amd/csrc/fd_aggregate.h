// fd_aggregate.h -- conditional sampling on window-mean observations (fd_aggregate.hip): what the host loops of fd_impute.hip and
// fd_dps.hip need to run their kernels on the window operator.  The loops, their Philox counters and every buffer are those of the
// mask path; only the operator between the two products of k_impute / k_dps_residual changes (fd_project.h).
#pragma once
#include "fd_common.h"
#include "fd_project.h"

// The window geometry of one (T, window): J = ceil(T / window) windows, window j = [j w, min((j + 1) w, T)), Jp = 16 ceil(J / 16).
// basis (fourier only): A_w = P F^T (Jp x Tp) then B_w = F P^+ (Tp x Jp), both row-major, zero outside (J, T); cached on the
// context under a key of (T, window).  Under the window operator the mask is (B/obs_rep,J,C) or (J,C), the kernels' basis is this
// one, and the feature std is read in both domains.
struct fd_agg_plan {
    fdproj::WindowOp op;
    const float* basis;
};

// window in [2, T] (window = 1 is the mask path: the callers forward it), T <= 1024 in both domains (the LDS images of one series)
int fd_agg_prepare(fd_ctx* ctx, int T, int Tp, int window, int fourier, hipStream_t s, fd_agg_plan* out, const char* who);
