// fd_linop.hip -- conditional sampling on a dense linear observation (NOT in the reference): the coordinate mask of fd_impute.hip /
// fd_dps.hip and the window means of fd_aggregate.hip are two instances of a linear observation operator; this one is a matrix the
// caller supplies.  Per channel y = P v, P (M x T) of full row rank, shared by all series and channels, 1 <= M <= T <= 1024; the
// caller also hands over P^+ = pinv(P) (computed in float64 on the host), so that P P^+ = I.  m (M,C) masks rows of P, y (M,C)
// holds observations at data scale and x0_obs = A^-1(P^+ where(m, y, 0)), A(x) = idft(sigma x + mu).  The formulas are those of
// fd_aggregate.hip with P, P^+ and P^T general:
//
//   x' = x + dft(P^+ (m . P idft(sigma . d))) / sigma          (fourier = 0: x' = x + P^+ (m . P (sigma . d)) / sigma)
//   r  = m . P idft(sigma . (x0_obs - x0_hat))   (M,C)          (fourier = 0: m . P (sigma . (x0_obs - x0_hat)))
//   u  = sigma . diag(1/rho) F P^T r                             (fourier = 0: sigma . P^T r)
//
// P^+ diag(m) is the pseudo-inverse of diag(m) P only when the rows of P are mutually orthogonal; the Python surface checks that
// (or that every column of the mask is all-or-nothing) before a replacement call reaches this file.  The guidance reads P and P^T
// alone and takes any mask.
//
// The kernels are k_impute and k_dps_residual themselves, instantiated on fd_project.h's DenseOp: phase 1 is unchanged (same Philox
// groups and counters), phase 2 is R = A U masked per row into a k-quad image of Mp x 16, Mp = 16 ceil(M / 16), phase 3 is Y = B R
// (the projection) or Y = Bt R (the guidance's adjoint) over the Tp packed rows.  Fourier: A = P F^T, B = F P^+, Bt = F P^T.  Time
// domain: the same two products with rho = 1 on A = P, B = P^+, Bt = P^T, and sigma is read there too (it varies along a row of
// P).  LDS = 64 (Tp + Mp) bytes, at most 128 KiB.  Every sum runs in a fixed order: two runs are bit-identical.
//
// This file holds what belongs to the operator alone: the handle (fd_linop.h) and its bases, built on the device in double -- F by
// k_impute_basis's formula into a temporary buffer, every product entry summed in ascending index order -- then rounded to f32 and
// zero-padded to (Mp, Tp).
#include <algorithm>
#include <cmath>
#include <new>

#include "fd_linop.h"

namespace {

// Ft[t][k] = F[k][t] (packed row k, time t) of the ortho packed real DFT, T x T doubles
__global__ __launch_bounds__(256) void k_linop_dft(double* __restrict__ Ft, int T) {
    const size_t n = (size_t)T * T;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i / T), r = (int)(i % T);
        const int n_real = T / 2 + 1;
        const bool im = r >= n_real;
        const int k = im ? r - n_real + 1 : r;
        double sn, cs;
        sincospi(2.0 * (double)(((long long)k * t) % T) / (double)T, &sn, &cs);
        Ft[i] = (im ? -sn : cs) / sqrt((double)T);
    }
}

// A (Mp x Tp), B (Tp x Mp), Bt (Tp x Mp) from P (M x T) and P^+ (T x M).  Ft != null: A[j][k] = sum_t P[j][t] F[k][t],
// B[k][j] = sum_t F[k][t] P^+[t][j], Bt[k][j] = sum_t F[k][t] P[j][t]; Ft == null: the entries of P, P^+ and P^T.  Zero outside
// [0, M) x [0, T); the sums in double in ascending t, then rounded.
__global__ __launch_bounds__(256) void k_linop_basis(float* __restrict__ A, float* __restrict__ B, float* __restrict__ Bt,
                                                     const double* __restrict__ P, const double* __restrict__ Pp,
                                                     const double* __restrict__ Ft, int T, int Tp, int M, int Mp) {
    const size_t n = (size_t)Mp * Tp;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int j = (int)(i / Tp), k = (int)(i % Tp);
        double a = 0.0, b = 0.0, bt = 0.0;
        if (j < M && k < T) {
            if (Ft) {
                for (int t = 0; t < T; ++t) {
                    const double f = Ft[(size_t)t * T + k];
                    const double p = P[(size_t)j * T + t];
                    a += p * f;
                    b += f * Pp[(size_t)t * M + j];
                    bt += f * p;
                }
            } else {
                a = bt = P[(size_t)j * T + k];
                b = Pp[(size_t)k * M + j];
            }
        }
        A[i] = (float)a;
        B[(size_t)k * Mp + j] = (float)b;
        Bt[(size_t)k * Mp + j] = (float)bt;
    }
}

}  // namespace

int fd_linop_prepare(fd_ctx* ctx, fd_linop* op, int T, int fourier, hipStream_t s, fdproj::DenseOp* out, const char* who) {
    FD_REQUIRE(ctx, op, "%s: null operator handle", who);
    FD_REQUIRE(ctx, op->ctx == ctx, "%s: the operator handle belongs to another context", who);
    FD_REQUIRE(ctx, op->T == T, "%s: the operator has T=%d columns, the call T=%d", who, op->T, T);
    FD_REQUIRE(ctx, op->M >= 1 && op->M <= op->T && T <= 1024, "%s: operator M=%d T=%d needs 1 <= M <= T <= 1024", who, op->M, op->T);
    const int d = fourier ? 1 : 0;
    const size_t n = (size_t)op->Mp * op->Tp;
    if (!op->tab[d]) {
        float* tab = nullptr;
        double* Ft = nullptr;
        FD_HIP(ctx, hipMalloc(&tab, 3 * n * sizeof(float)));
        hipError_t e = hipSuccess;
        const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
        if (fourier) {
            const size_t nf = (size_t)T * T;
            e = hipMalloc(&Ft, nf * sizeof(double));
            if (e == hipSuccess)
                hipLaunchKernelGGL(k_linop_dft, dim3((unsigned)std::min<size_t>((nf + 255) / 256, 4096)), dim3(256), 0, s, Ft, T);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_linop_basis, dim3(grid), dim3(256), 0, s, tab, tab + n, tab + 2 * n, op->P, op->Pplus, Ft, T, op->Tp,
                               op->M, op->Mp);
            e = hipGetLastError();
        }
        // synchronised, once per (handle, domain): later callers may use another stream, and Ft is freed behind the build
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (Ft) (void)hipFree(Ft);
        if (e != hipSuccess) {
            (void)hipFree(tab);
            return fd_fail(ctx, FD_ERR_HIP, "%s: could not build the operator bases of T=%d M=%d: %s", who, T, op->M, hipGetErrorString(e));
        }
        op->tab[d] = tab;
    }
    *out = fdproj::DenseOp{op->M, op->Mp, op->tab[d], op->tab[d] + n, op->tab[d] + 2 * n};
    return FD_OK;
}

extern "C" int fd_linop_create(fd_ctx* ctx, int T, int M, const double* P, const double* Pplus, fd_linop** out) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, P && Pplus && out, "fd_linop_create: null pointer");
    FD_REQUIRE(ctx, M >= 1 && M <= T && T <= 1024, "fd_linop_create: M=%d T=%d needs 1 <= M <= T <= 1024", M, T);
    *out = nullptr;
    FD_HIP(ctx, hipSetDevice(ctx->device));
    fd_linop* op = new (std::nothrow) fd_linop{ctx, T, M, (T + 15) / 16 * 16, (M + 15) / 16 * 16, nullptr, nullptr, {nullptr, nullptr}};
    if (!op) return fd_fail(ctx, FD_ERR_HIP, "fd_linop_create: out of host memory");
    const size_t bytes = (size_t)M * T * sizeof(double);
    hipError_t e = hipMalloc(&op->P, bytes);
    if (e == hipSuccess) e = hipMalloc(&op->Pplus, bytes);
    if (e == hipSuccess) e = hipMemcpy(op->P, P, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(op->Pplus, Pplus, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (op->P) (void)hipFree(op->P);
        if (op->Pplus) (void)hipFree(op->Pplus);
        delete op;
        return fd_fail(ctx, FD_ERR_HIP, "fd_linop_create: %s", hipGetErrorString(e));
    }
    *out = op;
    return FD_OK;
}

extern "C" int fd_linop_destroy(fd_linop* op) {
    if (!op) return FD_OK;
    for (void* p : {(void*)op->P, (void*)op->Pplus, (void*)op->tab[0], (void*)op->tab[1]})
        if (p) (void)hipFree(p);       // (hipFree waits for the kernels that read the buffer)
    delete op;
    return FD_OK;
}
