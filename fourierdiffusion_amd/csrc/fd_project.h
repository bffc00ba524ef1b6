// fd_project.h -- what the projection kernels of conditional sampling share: k_impute (fd_impute.hip) and
// k_dps_residual (fd_dps.hip) include it, and fd_aggregate.hip for the window geometry and the table cache; every piece below exists
// once.  Both kernels are the same three phases on one 512-thread workgroup per (series, block of 16 channels): phase 1 elementwise
// into a k-quad LDS image U (Tp x 16), phase 2 a dense product with a basis into a second image of the observation's rows, masked row
// by row, phase 3 a second product back to the Tp packed rows with an elementwise epilogue.
//
//   operator        MaskOp / WindowOp / DenseOp: what stands between the two products.  The rows of the middle image (time steps /
//                   windows / the rows of a user's matrix), which basis each product reads (the adjoint's included), and the factor
//                   of the adjoint (1 / 1 over the window length / 1).
//   images          quad_idx (the k-quad order [(k / 4)][channel][k % 4]: the B operand of four consecutive MFMAs is one
//                   ds_read_b128 per lane), inv_r, win_len, image_bytes.
//   tile_product    16 rows of a row-major basis times an image on v_mfma_f32_16x16x4_f32: every phase 2 / phase 3 loop.
//   group walk      group_of / group_noise: which elements of a Philox group of 4 a workgroup owns, and their injected or drawn
//                   noise: phase 1 of k_impute, once per noise stream.
//   block_sum       the fixed-order double LDS tree behind part[blockIdx.x]: k_dps_residual.
//   launch_kernel   sets the kernel's dynamic-LDS maximum once per device, then launches.
//   cached_table    the device-built tables of ctx->fft_tw and their keys: fd_impute_basis and the window bases.
#pragma once
#include <hip/hip_runtime.h>

#include "fd_common.h"
#include "fd_philox.h"

namespace fdproj {

constexpr int kThreads = 512;    // 8 waves: the row tiles of a product are dealt round-robin
constexpr int kCB = 16;          // channels per workgroup = N of the MFMA tile

typedef __attribute__((ext_vector_type(4))) float f32x4;

// ---------------------------------------------------------------------------------------------- observation operators
// window j = [j w, min((j + 1) w, T)): its length (the last one may be short)
__device__ __forceinline__ int win_len(int j, int w, int T) { return min(w, T - j * w); }

// The coordinate mask: the middle image holds the Tp time rows, keep = mask[t][c].  basis = F (Tp x Tp) then F^T (Tp x Tp).
struct MaskOp {
    static constexpr bool kWindow = false, kDense = false;
    __host__ __device__ int rows(int T) const { return T; }
    __host__ __device__ int rows_padded(int Tp) const { return Tp; }
    __device__ const float* to_obs(const float* basis, int Tp) const { return basis + (size_t)Tp * Tp; }
    __device__ const float* from_obs(const float* basis, int) const { return basis; }
    __device__ const float* adjoint_basis(const float* basis, int Tp) const { return from_obs(basis, Tp); }
    __device__ float adjoint(float r, int, int) const { return r; }
};
// Window means (fd_aggregate.hip): the middle image holds the Jp window rows, keep = mask[j][c].  basis = A_w (Jp x Tp) then B_w
// (Tp x Jp); the adjoint P^T divides the masked means by the window length and reads the same B_w.
struct WindowOp {
    static constexpr bool kWindow = true, kDense = false;
    int window, J, Jp;
    __host__ __device__ int rows(int) const { return J; }
    __host__ __device__ int rows_padded(int) const { return Jp; }
    __device__ const float* to_obs(const float* basis, int) const { return basis; }
    __device__ const float* from_obs(const float* basis, int Tp) const { return basis + (size_t)Jp * Tp; }
    __device__ const float* adjoint_basis(const float* basis, int Tp) const { return from_obs(basis, Tp); }
    __device__ float adjoint(float r, int j, int T) const { return r / (float)win_len(j, window, T); }
};
// A dense linear observation y = P v, P (M x T) of full row rank (fd_linop.hip): the middle image holds the Mp = 16 ceil(M / 16) rows
// of P, keep = mask[j][c].  The operator carries its own bases (the kernels' `basis` argument is not read), row-major f32, zero
// outside (M, T): A (Mp x Tp) to the observation, B (Tp x Mp) back from it, Bt (Tp x Mp) the adjoint's, which no per-row factor of B
// expresses.  Fourier: A = P F^T, B = F P^+, Bt = F P^T; time domain: P, P^+, P^T themselves, and the kernels run their Fourier
// branch with rho = 1.
struct DenseOp {
    static constexpr bool kWindow = false, kDense = true;
    int M, Mp;
    const float *A, *B, *Bt;
    __host__ __device__ int rows(int) const { return M; }
    __host__ __device__ int rows_padded(int) const { return Mp; }
    __device__ const float* to_obs(const float*, int) const { return A; }
    __device__ const float* from_obs(const float*, int) const { return B; }
    __device__ const float* adjoint_basis(const float*, int) const { return Bt; }
    __device__ float adjoint(float r, int, int) const { return r; }
};

// dynamic LDS of one workgroup.  fourier (and the dense operator in both domains): U (Tp x 16) and the middle image; else the window
// operator's time image (T x 16), and nothing for the mask, which selects elementwise
template <class Op>
size_t image_bytes(const Op& op, int T, int Tp, bool fourier) {
    if (fourier || Op::kDense) return (size_t)(Tp + op.rows_padded(Tp)) * kCB * sizeof(float);
    return Op::kWindow ? (size_t)T * kCB * sizeof(float) : 0;
}

// ---------------------------------------------------------------------------------------------- the device-built tables
// ctx->fft_tw holds every per-shape device table of a context under an int key (T and window in [1, 1024]):
//   T, -T, -T - 2^20                          fd_fourier.hip: the FFT twiddles and packing tables, built on the host
//   -T - 2^21                                 fd_impute_basis: F and F^T of the packed real DFT
//   -3 2^20 - ((window - 1) 1025 + T)         fd_agg_prepare: A_w and B_w; below every key above
//   -8 2^20 - (2 S + window)                  fd_series_spectra (fd_spectral.hip): the double window and the [cos | sin] basis of nperseg S
// The table of `key` (n floats), built on first use by fill(table) on stream s; null if it could not be built.  The build is
// synchronised, once per (context, key): later callers may use another stream.
template <class Fill>
const float* cached_table(fd_ctx* ctx, int key, size_t n, hipStream_t s, Fill fill) {
    for (auto& e : ctx->fft_tw)
        if (e.first == key) return reinterpret_cast<const float*>(e.second);
    void* d = nullptr;
    if (hipMalloc(&d, sizeof(float) * n) != hipSuccess) return nullptr;
    fill(reinterpret_cast<float*>(d));
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    ctx->fft_tw.emplace_back(key, d);
    return reinterpret_cast<const float*>(d);
}

// ---------------------------------------------------------------------------------------------- launch
// one workgroup of kThreads per (row, channel block); MAX_LDS: the kernel's dynamic-LDS ceiling, set once per device before the first
// launch that uses any
template <auto Kernel, int MAX_LDS, class... Args>
int launch_kernel(fd_ctx* ctx, unsigned grid, size_t lds, hipStream_t s, const Args&... args) {
    static unsigned long long attr_set = 0;
    if (lds && fd_first_on_device(attr_set, ctx->device))
        FD_HIP(ctx, hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS));
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(kThreads), lds, s, args...);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------- images and products
// 1 / r of packed row k: 1 at DC and Nyquist (T even), 2 at every other bin (the Hermitian pair it stands for)
__device__ __forceinline__ float inv_r(int k, int T) { return (k == 0 || (2 * k == T)) ? 1.0f : 2.0f; }

// LDS image index of (k, channel) in k-quad order
__device__ __forceinline__ int quad_idx(int k, int c) { return ((k >> 2) * kCB + c) * 4 + (k & 3); }

// acc = M[row0 + li][0 .. K) . V[0 .. K)[li-th channel]: M row-major with row stride K (a multiple of 16), V a k-quad LDS image; the
// lane holds rows row0 + 4 kq + 0..3 of channel li, one k-quad of the next image
__device__ __forceinline__ f32x4 tile_product(const float* __restrict__ M, int row0, int K, const float* V, int li, int kq) {
    const float* arow = M + (size_t)(row0 + li) * K + 4 * kq;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 16) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(arow + k0);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(V + ((k0 / 4 + kq) * kCB + li) * 4);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[3], acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

// ---------------------------------------------------------------------------------------------- the phase-1 group walk
// Philox group g = elements 4g .. 4g+3 of the whole (B,T,C) tensor (k_sde_step's).  Of those, the workgroup of (series at `base`,
// channels [c0, c0 + kCB)) owns own[j], at offset loc[j] in its series; a group straddling two series or blocks is drawn by each.
// Returns whether it owns any.  (Plain arrays: handing the three back in one struct moved the SGPR count of k_impute across an
// occupancy step in two instantiations.)
__device__ __forceinline__ bool group_of(size_t g, size_t base, size_t TC, int C, int c0, int (&loc)[4], bool (&own)[4]) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const size_t e = g * 4 + j;
        own[j] = false;
        loc[j] = 0;
        if (e >= base && e < base + TC) {
            loc[j] = (int)(e - base);
            const int c = loc[j] % C;
            own[j] = c >= c0 && c < c0 + kCB;
        }
        any |= own[j];
    }
    return any;
}
// z = one noise stream of the group: the injected values of the owned elements (zin, the series at `base`), or the draw at `counter`
__device__ __forceinline__ void group_noise(const int (&loc)[4], const bool (&own)[4], const float* zin, size_t base, uint64_t counter,
                                            uint64_t seed, float (&z)[4]) {
    if (zin) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (own[j]) z[j] = zin[base + loc[j]];
    } else {
        fd_randn4(counter, seed, z);
    }
}

// ---------------------------------------------------------------------------------------------- block sum
// *dst = the sum of v over the workgroup: fixed-order LDS tree, so two runs are bit-identical (no atomics)
__device__ __forceinline__ void block_sum(double v, double* dst) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) *dst = red[0];
}

}  // namespace
}  // namespace fdproj
