// fd_pairs.hip -- the plain kernels of fd_pairs.h, compiled once: the sum of the splits' counts and the centring
// prologue of the Gram-tile kernels (column mean, centred padded copy, row norms).
#include "fd_pairs.h"

namespace fdp {
namespace {

// counts[i] = the partial counts pc (splits, n) of query i, added in split order
__global__ __launch_bounds__(256) void k_sum_counts(const int* __restrict__ pc, int splits, int n, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int s = 0;
    for (int z = 0; z < splits; ++z) s += pc[(size_t)z * n + i];
    counts[i] = s;
}

// partial column sums in double: block b = (row chunk b / ncb, column block b % ncb), rows in ascending order
__global__ __launch_bounds__(256) void k_col_partial(const float* __restrict__ x, double* __restrict__ part, int m, int d, int ncb) {
    const int chunk = blockIdx.x / ncb, c = (blockIdx.x - chunk * ncb) * 256 + threadIdx.x;
    if (c >= d) return;
    const int r0 = chunk * MEAN_ROWS, r1 = min(m, r0 + MEAN_ROWS);
    double s = 0.0;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) s += (double)x[(size_t)r * d + c];
    part[(size_t)chunk * d + c] = s;
}

// the column mean (partials in chunk order) rounded to f32 and, where meand is given, in double; 0 in the padded columns
__global__ __launch_bounds__(256) void k_col_mean(const double* __restrict__ part, double* __restrict__ meand, float* __restrict__ mean,
                                                  int chunks, int m, int d, int dp) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= dp) return;
    double s = 0.0;
    if (c < d)
        for (int z = 0; z < chunks; ++z) s += part[(size_t)z * d + c];
    s /= (double)m;
    if (meand) meand[c] = s;
    mean[c] = (float)s;
}

// xc (rows_pad, dp) = x - mean in f32, zero in the padding; norm[row] = ||xc[row]||^2 (double sum of the f32 values' squares).  Where
// meand / ss are given, ss[row] = ||x[row] - meand||^2 entirely in double.  One wave per row.
__global__ __launch_bounds__(256) void k_centre(const float* __restrict__ x, const float* __restrict__ mean,
                                                const double* __restrict__ meand, float* __restrict__ xc, float* __restrict__ norm,
                                                double* __restrict__ ss, int rows, int rows_pad, int d, int dp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows_pad) return;
    double s = 0.0, e = 0.0;
    for (int c = lane; c < dp; c += 64) {
        float v = 0.f;
        if (row < rows && c < d) {
            const float xv = x[(size_t)row * d + c];
            v = xv - mean[c];
            if (meand) {
                const double w = (double)xv - meand[c];
                e += w * w;
            }
        }
        xc[(size_t)row * dp + c] = v;
        s += (double)v * (double)v;
    }
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o); e += __shfl_down(e, o); }
    if (lane == 0) {
        norm[row] = (float)s;
        if (ss) ss[row] = e;
    }
}

}  // namespace

void sum_counts(const int* pc, int splits, int n, int32_t* counts, hipStream_t s) {
    hipLaunchKernelGGL(k_sum_counts, dim3(fd_cdiv(n, 256)), dim3(256), 0, s, pc, splits, n, counts);
}

void centre_mean(const float* x, int m, int d, double* part, double* meand, float* mean, hipStream_t s) {
    const int ncb = fd_cdiv(d, 256), chunks = mean_chunks(m), dp = padded_features(d);
    hipLaunchKernelGGL(k_col_partial, dim3((unsigned)chunks * ncb), dim3(256), 0, s, x, part, m, d, ncb);
    hipLaunchKernelGGL(k_col_mean, dim3(fd_cdiv(dp, 256)), dim3(256), 0, s, part, meand, mean, chunks, m, d, dp);
}

void centre_rows(const float* x, int rows, int d, const float* mean, const double* meand, float* xc, float* norm, double* ss,
                        hipStream_t s) {
    const int rows_pad = padded_rows(rows);
    hipLaunchKernelGGL(k_centre, dim3(rows_pad / 4), dim3(256), 0, s, x, mean, meand, xc, norm, ss, rows, rows_pad, d, padded_features(d));
}

}  // namespace fdp
