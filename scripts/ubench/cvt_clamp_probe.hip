// cvt_clamp_probe.hip -- does gfx950 honour the VOP3 clamp bit on v_cvt_pk_bf16_f32?
//
// The pair-form FFN loop of k_mega could drop its relu (one v_pk_max_i16 per two hidden values) if the conversion itself clamped
// to [0, 1].  The assembler encodes the modifier; this program asks the hardware what it does with it.
//
// Inputs: all 65 536 high-half patterns x the low halves below, each fed through a plain global load and converted in BOTH result
// halves (once as src0 with 0.5 beside it, once as src1).  Host reference for every non-NaN input: bf16_rne(min(max(x, 0), 1)).
// NaN inputs are only tallied (what the hardware returns is printed, nothing is asserted).
//
//   hipcc -O2 --offload-arch=gfx950 -o cvt_clamp_probe cvt_clamp_probe.hip && ./cvt_clamp_probe > profiles/cvt_clamp_probe.txt
// Exit status 0: every non-NaN input matches in both halves; 1: at least one deviates (the first ones are printed).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CK(x)                                                                         \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

static const uint32_t kLow[8] = {0x0000u, 0x0001u, 0x4000u, 0x7FFFu, 0x8000u, 0x8001u, 0xC000u, 0xFFFFu};

// out[2 i] = cvt_pk(x, 0.5) clamp, out[2 i + 1] = cvt_pk(0.5, x) clamp; out_plain the same without the modifier
__global__ void k_probe(const float* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ out_plain, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[i], half = 0.5f;
    uint32_t a, b, c, d;
    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2 clamp" : "=v"(a) : "v"(x), "v"(half));
    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2 clamp" : "=v"(b) : "v"(half), "v"(x));
    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(c) : "v"(x), "v"(half));
    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(d) : "v"(half), "v"(x));
    out[2 * i] = a;
    out[2 * i + 1] = b;
    out_plain[2 * i] = c;
    out_plain[2 * i + 1] = d;
}

static uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static uint16_t ref_clamp(float x) {
    const float c = x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;      // -0 -> +0, -inf -> 0, +inf -> 1
    return bf16_rne(c);
}

int main() {
    const int n = 65536 * 8;
    std::vector<uint32_t> bits(n);
    for (int hi = 0; hi < 65536; ++hi)
        for (int j = 0; j < 8; ++j) bits[hi * 8 + j] = ((uint32_t)hi << 16) | kLow[j];
    float* d_in;
    uint32_t *d_out, *d_plain;
    CK(hipMalloc(&d_in, n * 4));
    CK(hipMalloc(&d_out, n * 8));
    CK(hipMalloc(&d_plain, n * 8));
    CK(hipMemcpy(d_in, bits.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, n * 8));
    CK(hipMemset(d_plain, 0xA5, n * 8));
    k_probe<<<n / 256, 256>>>(d_in, d_out, d_plain, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> out(2 * n), plain(2 * n);
    CK(hipMemcpy(out.data(), d_out, n * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(plain.data(), d_plain, n * 8, hipMemcpyDeviceToHost));

    const uint16_t half_bf = 0x3F00;
    long checked = 0, bad = 0, bad_sub = 0, bad_plain = 0, bad_other = 0, nans = 0, subn = 0, subn_flushed_plain = 0;
    // NaN inputs: tally of the clamped result patterns (lo half of the src0 form, hi half of the src1 form)
    long nan_zero = 0, nan_nan = 0, nan_one = 0, nan_else = 0;
    uint32_t nan_example_in = 0, nan_example_out = 0;
    for (int i = 0; i < n; ++i) {
        float x;
        memcpy(&x, &bits[i], 4);
        const uint16_t lo_c = out[2 * i] & 0xFFFFu, hi_c = out[2 * i + 1] >> 16;
        const uint16_t other0 = out[2 * i] >> 16, other1 = out[2 * i + 1] & 0xFFFFu;
        const uint16_t lo_p = plain[2 * i] & 0xFFFFu, hi_p = plain[2 * i + 1] >> 16;
        if (std::isnan(x)) {
            ++nans;
            for (uint16_t r : {lo_c, hi_c}) {
                if (r == 0) ++nan_zero;
                else if ((r & 0x7F80u) == 0x7F80u && (r & 0x7Fu)) ++nan_nan;
                else if (r == 0x3F80u) ++nan_one;
                else ++nan_else;
            }
            if (!nan_example_in) nan_example_in = bits[i], nan_example_out = out[2 * i];
            continue;
        }
        ++checked;
        const bool sub = (bits[i] & 0x7F800000u) == 0 && (bits[i] & 0x007FFFFFu);
        subn += sub;
        const uint16_t want = ref_clamp(x), want_plain = bf16_rne(x);
        if (lo_p != want_plain || hi_p != want_plain) {
            ++bad_plain;
            if (sub && (lo_p & 0x7FFFu) == 0) ++subn_flushed_plain;
            else if (bad_plain - subn_flushed_plain <= 8)
                printf("PLAIN DEVIATES in=0x%08x lo=0x%04x hi=0x%04x want=0x%04x\n", bits[i], lo_p, hi_p, want_plain);
        }
        if (other0 != half_bf || other1 != half_bf) ++bad_other;
        if (lo_c != want || hi_c != want) {
            bad_sub += sub;
            if (++bad <= 16) printf("CLAMP DEVIATES in=0x%08x (%.9g) lo=0x%04x hi=0x%04x want=0x%04x\n", bits[i], x, lo_c, hi_c, want);
        }
    }
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    printf("device: %s\n", prop.gcnArchName);
    printf("inputs: %d (65536 high halves x 8 low halves), non-NaN checked: %ld (subnormal: %ld), NaN: %ld\n", n, checked, subn, nans);
    printf("reference: bf16_rne(min(max(x, 0), 1)), both result halves\n");
    printf("clamped conversion, non-NaN deviations: %ld (of which subnormal fp32 inputs: %ld)\n", bad, bad_sub);
    printf("companion half (0.5 beside every input) deviations: %ld\n", bad_other);
    printf("plain conversion vs bf16_rne(x), deviations: %ld (of which subnormal inputs flushed to zero: %ld)\n", bad_plain,
           subn_flushed_plain);
    printf("NaN inputs (reported only), clamped result halves: zero %ld, NaN %ld, one %ld, other %ld; e.g. in=0x%08x -> 0x%08x\n", nan_zero,
           nan_nan, nan_one, nan_else, nan_example_in, nan_example_out);
    printf("verdict: %s\n", bad == 0 && bad_other == 0 ? "PASS (the clamp bit is honoured: the conversion is a relu for inputs scaled into [0, 1])"
                                                      : "FAIL");
    return bad == 0 && bad_other == 0 ? 0 : 1;
}
