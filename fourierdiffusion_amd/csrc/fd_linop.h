// fd_linop.h -- conditional sampling on a dense linear observation y = P v (fd_linop.hip): the operator handle behind
// fd_linop_create, and what the host loops of fd_impute.hip and fd_dps.hip need to run their kernels on fd_project.h's DenseOp.  The
// loops, their Philox counters and every buffer are those of the mask path; only the operator between the two products changes.
#pragma once
#include "fd_common.h"
#include "fd_project.h"

// One operator P (M x T), shared by all series and channels.  P and P^+ stay on the device as the doubles the caller handed over;
// tab[fourier] holds the three f32 bases of that domain, A (Mp x Tp) then B (Tp x Mp) then Bt (Tp x Mp), built on first use.  The
// tables belong to the handle, not to the context's table cache: fd_linop_destroy frees them.
struct fd_linop {
    fd_ctx* ctx;
    int T, M, Tp, Mp;
    double *P, *Pplus;       // (M,T) and (T,M), row-major, on the device
    float* tab[2];           // [0] the time domain (P, P^+, P^T), [1] Fourier (P F^T, F P^+, F P^T); null until first used
};

// The DenseOp of `op` in the given domain for a model of length T, its bases built (and waited for) on first use.  FD_ERR_ARG for a
// null handle, a handle of another context or another T, or M > T.
int fd_linop_prepare(fd_ctx* ctx, fd_linop* op, int T, int fourier, hipStream_t s, fdproj::DenseOp* out, const char* who);
