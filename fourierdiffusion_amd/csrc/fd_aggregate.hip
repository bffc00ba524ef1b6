// fd_aggregate.hip -- conditional sampling on window-mean observations (NOT in the reference): temporal super-resolution,
// disaggregation and forecasting from a series reported at a coarser rate than the model's.  The coordinate mask of fd_impute.hip and
// fd_dps.hip becomes a linear observation operator.  With w the window length, J = ceil(T / w) windows, window j = [j w,
// min((j + 1) w, T)) of length l_j (the last one may be short), per channel:
//
//   (P v)_j   = (1 / l_j) sum_{t in window j} v_t     (J x T, the window means)
//   (P^+ r)_t = r_{j(t)}                               (the broadcast; P P^+ = I)
//   (P^T r)_t = r_{j(t)} / l_{j(t)}
//
// m (J,C) masks windows, y (J,C) holds window means at data scale and x0_obs = A^-1(P^+ where(m, y, 0)), A(x) = idft(sigma x + mu).
// Replacement (Song et al. 2021 for a general linear observation: the orthogonal projector P^+ P in the place of the mask), d as in
// fd_impute.hip:
//   x' = x + dft(P^+ (m . P idft(sigma . d))) / sigma          (fourier = 0: x' = x + P^+ (m . P (sigma . d)) / sigma)
// Guidance (fd_dps.hip's derivation with the residual of the window means):
//   r = m . P idft(sigma . (x0_obs - x0_hat))   (J,C)          (fourier = 0: m . P (sigma . (x0_obs - x0_hat)))
//   u = sigma . diag(1/rho) F P^T r                              (fourier = 0: sigma . P^T r)
// sigma varies inside a window, so it no longer cancels in the time domain: both domains read it.
//
// Fourier path: idft = F^T diag(1/rho), so P idft(v) = (P F^T)(v / rho) and dft(P^+ R) = (F P^+) R: two RECTANGULAR bases per
// (T, w), A_w = P F^T (Jp x Tp) and B_w = F P^+ (Tp x Jp), Jp = 16 ceil(J / 16), built once on the device in double, rounded to f32
// and cached on the context.  F P^T = F P^+ diag(1 / l): the guidance divides the J masked means by l_j and reads the same B_w.
// The kernels are k_impute and k_dps_residual themselves, instantiated on fd_project.h's WindowOp: phase 1 is unchanged (same Philox
// groups and counters), phase 2 is R = A_w U masked per window into a k-quad image of Jp x 16, phase 3 is Y = B_w R over the T packed
// rows.  Both products are J/T of the mask path's.  LDS = 64 (Tp + Jp) bytes.  Time-domain path: sigma d goes to an LDS time image
// (T x 16); one thread per (window, channel) sums its window in ascending t and writes the masked mean back over the window.  Every
// sum runs in a fixed order: two runs are bit-identical.
//
// This file holds what belongs to the operator alone: the window geometry of a (T, w) and its two bases.
#include <algorithm>
#include <cmath>

#include "fd_aggregate.h"

namespace {

using fdproj::win_len;

// A_w[j][k] = (1 / l_j) sum_{t in window j} F[k][t] and B_w[k][j] = sum_{t in window j} F[k][t] (F of k_impute_basis: packed row k,
// time t), zero outside [0, J) x [0, T); the sums in double in ascending t, then rounded
__global__ __launch_bounds__(256) void k_agg_basis(float* __restrict__ Aw, float* __restrict__ Bw, int T, int Tp, int w, int J, int Jp) {
    const size_t n = (size_t)Jp * Tp;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int j = (int)(i / Tp), k = (int)(i % Tp);
        double sum = 0.0;
        int l = 1;
        if (j < J && k < T) {
            const int n_real = T / 2 + 1;
            const bool im = k >= n_real;
            const int kk = im ? k - n_real + 1 : k;
            l = win_len(j, w, T);
            for (int t = j * w; t < j * w + l; ++t) {
                double sn, cs;
                sincospi(2.0 * (double)(((long long)kk * t) % T) / (double)T, &sn, &cs);
                sum += im ? -sn : cs;
            }
            sum /= sqrt((double)T);
        }
        Aw[i] = (float)(sum / (double)l);
        Bw[(size_t)k * Jp + j] = (float)sum;
    }
}

}  // namespace

int fd_agg_prepare(fd_ctx* ctx, int T, int Tp, int window, int fourier, hipStream_t s, fd_agg_plan* out, const char* who) {
    FD_REQUIRE(ctx, window >= 1 && window <= T, "%s: window=%d must lie in [1, max_len=%d]", who, window, T);
    FD_REQUIRE(ctx, T <= 1024, "%s: max_len %d > 1024 with window > 1 (the LDS images of one series)", who, T);
    const int J = (T + window - 1) / window, Jp = (J + 15) / 16 * 16;
    out->op = fdproj::WindowOp{window, J, Jp};
    out->basis = nullptr;
    if (fourier) {
        const size_t n = (size_t)Jp * Tp;
        out->basis = fdproj::cached_table(ctx, -(3 << 20) - ((window - 1) * 1025 + T), 2 * n, s, [&](float* Aw) {
            hipLaunchKernelGGL(k_agg_basis, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, Aw, Aw + n, T, Tp,
                               window, J, Jp);
        });
        if (!out->basis) return fd_fail(ctx, FD_ERR_HIP, "%s: could not build the window bases of T=%d window=%d", who, T, window);
    }
    return FD_OK;
}
