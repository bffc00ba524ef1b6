// fd_score_bf16.hip -- bf16 MFMA inference path of the score network (gfx950).
//
// Operand convention shared by every kernel here (v_mfma_f32_16x16x32_bf16, one wave = one 16x16 tile):
//   * the TOKEN index always rides on lane&15; lane>>4 (= g) selects an 8-wide k-slot group, so an
//     activation fragment is "for token lane&15: 8 consecutive features starting at 32*ks + 8*g".
//   * weights are the A operand (rows = output features), activations the B operand (columns = tokens):
//     every GEMM is computed TRANSPOSED (out^T = W . x^T), so the C tile comes out as
//     C[row = 4*g + r (feature), col = lane&15 (token)] -- again token-on-lane.  A C tile can therefore be
//     fed straight back as the next GEMM's B operand after a register-local relu/convert, with the k
//     order of the next weight matrix permuted to match (done once in fd_bf16_prepare): the 2048-wide
//     FFN hidden never leaves registers.
//   * biases ride in the zero padding of K (an extra "1.0" activation row), so padding FLOPs do work.
//   * weight images are stored in HBM in exact fragment order (1 KiB = 64 lanes x 16 B per block) and
//     streamed L2 -> LDS with global_load_lds (16 B/lane), double buffered, shared by all waves of the WG.
//
// Reference arithmetic: nn.TransformerEncoderLayer (post-LN, relu) as built at
// src/fdiff/models/score_models.py:57-62; SURVEY.md A.3.  fp32 everywhere except the MFMA operands.
#include <algorithm>
#include <cmath>
#include <map>

#include "fd_gemm_f32.h"
#include "fd_bf16_images.h"
#include "fd_mega.h"
#include "fd_ode.h"
#include "fd_philox.h"
#include "fd_score.h"
#include "fd_sde.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

// fd_score_f32.hip
void fd_attention_f32(const float* qkv, float* out, float* lse, int B, int T, int H, int hd, float drop_p,
                      uint64_t seed, uint64_t offset, hipStream_t s);


namespace {

// ------------------------------------------------------------------ weight images
// FFN image of one layer.  Block order inside a (F-half, chunk) group: W1 [ft 0..1][ks 0..KS1-1], W2 [dt].
//   W1 block (ft, ks): lane (row=l&15, g): k = 32ks+8g+j -> W1[f = fbase+16ft+row][k], k==D -> b1[f], else 0
//   W2 block (dt)    : lane (row=l&15, g): slot j<4 -> f = fbase+4g+j ; j>=4 -> f = fbase+16+4g+(j-4)
//                                          value W2[d = 16dt+row][f] (0 when d >= D)
// The W2 k-permutation is exactly the (token, 4g+r) register layout of the two 16x16 hidden tiles.
__device__ void build_ffn_block(const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                __bf16* __restrict__ img, int D, int F, int KS1, int DT, int chunk_major, int blk, int lane) {
    const int NB = 2 * KS1 + DT;
    const int NC = F / 64;                      // 32-wide chunks per F-half
    const int j = blk % NB;                     // blk = ((fh*NC + c)*NB + j)
    const int c = (blk / NB) % NC;
    const int fh = blk / (NB * NC);
    const int row = lane & 15, g = lane >> 4;
    const int fbase = fh * (F / 2) + c * 32;
    // chunk_major: [chunk][F-half][block] (the persistent kernel streams whole chunk pairs linearly);
    // otherwise [F-half][chunk][block] (k_ffn_ln: each workgroup half walks its own F-half)
    const int oblk = chunk_major ? (c * 2 + fh) * NB + j : blk;
    __bf16* dst = img + ((size_t)oblk * 64 + lane) * 8;
    if (j < 2 * KS1) {
        const int ft = j / KS1, ks = j % KS1;
        const int f = fbase + 16 * ft + row;
        for (int e = 0; e < 8; ++e) {
            const int k = 32 * ks + 8 * g + e;
            float v = 0.f;
            if (k < D) v = W1[(size_t)f * D + k];
            else if (k == D) v = b1[f];
            dst[e] = (__bf16)v;
        }
    } else {
        const int dt = j - 2 * KS1;
        const int d = 16 * dt + row;
        for (int e = 0; e < 8; ++e) {
            const int f = fbase + ((e < 4) ? (4 * g + e) : (16 + 4 * g + (e - 4)));
            dst[e] = (__bf16)((d < D) ? W2[(size_t)d * F + f] : 0.f);
        }
    }
}

// FFN image of the persistent kernel's PAIR form (fd_mega.hip, FFN32): H of a pair of token tiles by v_mfma_f32_32x32x16_bf16
// (M = 32 hidden units, N = 32 tokens, K = D + 1 bias slot padded to 16 DT instead of 32 KS1), W2 by the 16x16x32 form.
// Chunk-major: block ((c*2 + fh)*NB + j), NB = 2 DT, of chunk c (hidden units fbase = fh*F/2 + 32c .. +31):
//   j <  DT (ks)  : 32x32x16 A fragment rows, stored with row bits 3 and 4 swapped (LDS bank slots of the kernel's two readers): lane
//                   slot l holds hidden unit fbase + swap34(l & 31), k = 16 ks + 8 (l >> 5) + e (k == D -> b1, > D -> 0)
//   j >= DT (dt)  : 16x16x32 A fragment of W2 rows d = 16 dt + (l & 15); k-slot e of lane row q = l >> 4 is hidden unit
//                   fbase + 16 (q & 1) + 8 (e >> 2) + 4 (q >> 1) + (e & 3): the order in which four v_permlane16_swap leave a
//                   relu'd 32x32 C tile in the two 16x16x32 B fragments of the pair (relu_split32 in fd_mega.hip)
//
// FD_RELU_CLAMP (fd_mega_params.h): W1 | b1 are stored as 2^-k w and W2 as 2^k w, k = FD_RELU_CLAMP_SHIFT, scaled in fp32 before the
// conversion -- exact, and the same bf16 mantissas, as long as the scaled weight is a normal bf16: 2^(k-126) <= |w| for W1 | b1 (or
// w == 0) and |w| < 2^(127-k) for W2.  Anything else (non-finite values too) is counted into *bad: fd_bf16_prepare reads the counter
// back and a model that fails runs without this image (the 16x16x32 loop on the unscaled off_ffn image).
__device__ void build_ffn32_block(const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                  __bf16* __restrict__ img, int D, int F, int DT, int blk, int lane, int* __restrict__ bad) {
#if FD_RELU_CLAMP
    const float w1_min = ldexpf(1.f, FD_RELU_CLAMP_SHIFT - 126), w2_lim = ldexpf(1.f, 127 - FD_RELU_CLAMP_SHIFT);
    int nbad = 0;
#endif
    const int NB = 2 * DT;
    const int j = blk % NB, fh = (blk / NB) & 1, c = blk / (2 * NB);
    const int fbase = fh * (F / 2) + c * 32;
    __bf16* dst = img + ((size_t)blk * 64 + lane) * 8;
    if (j < DT) {
        const int row = lane & 31;
        const int f = fbase + (FD_W1_SWAP34 ? ((row & 7) | ((row & 8) << 1) | ((row & 16) >> 1)) : row);
        for (int e = 0; e < 8; ++e) {
            const int k = 16 * j + 8 * (lane >> 5) + e;
            float v = 0.f;
            if (k < D) v = W1[(size_t)f * D + k];
            else if (k == D) v = b1[f];
#if FD_RELU_CLAMP
            nbad += !(v == 0.f || (fabsf(v) >= w1_min && fabsf(v) <= 3.0e38f));
            v = ldexpf(v, -FD_RELU_CLAMP_SHIFT);
#endif
            dst[e] = (__bf16)v;
        }
    } else {
        const int d = 16 * (j - DT) + (lane & 15), q = lane >> 4;
        for (int e = 0; e < 8; ++e) {
            const int f = fbase + 16 * (q & 1) + 8 * (e >> 2) + 4 * (q >> 1) + (e & 3);
            float v = (d < D) ? W2[(size_t)d * F + f] : 0.f;
#if FD_RELU_CLAMP
            nbad += !(fabsf(v) < w2_lim);
            v = ldexpf(v, FD_RELU_CLAMP_SHIFT);
#endif
            dst[e] = (__bf16)v;
        }
    }
#if FD_RELU_CLAMP
    if (nbad) atomicAdd(bad, nbad);
#endif
}

// ------------------------------------------------------------------ persistent-kernel weight images
// One 64-lane block = one 1 KiB MFMA fragment: lane (row = l&15, g = l>>4) holds 8 bf16 = k-slots 8g..8g+7 of
// k-step ks for matrix row `row` of row tile rt.  kind selects how (rt, row, k) maps onto the fp32 weights.
enum { IMG_EMB = 0, IMG_UNEMB = 1, IMG_Q = 2, IMG_K = 3, IMG_V = 4, IMG_WO = 5 };
__device__ void build_image_block(int kind, const float* __restrict__ W, const float* __restrict__ bias,
                                  __bf16* __restrict__ img, int KS, int rows, int K, int H, int hd, int D, float scale,
                                  int blk, int lane) {
    const int rt = blk / KS, ks = blk - rt * KS;
    const int row = lane & 15, g = lane >> 4;
    __bf16* dst = img + ((size_t)blk * 64 + lane) * 8;
    for (int e = 0; e < 8; ++e) {
        const int k = 32 * ks + 8 * g + e;
        float v = 0.f;
        if (kind == IMG_EMB || kind == IMG_UNEMB) {
            // rows of W (rows x K) with the bias in k-slot K
            const int r = 16 * rt + row;
            if (r < rows) v = (k < K) ? W[(size_t)r * K + k] : (k == K ? bias[r] : 0.f);
        } else if (kind == IMG_Q || kind == IMG_K || kind == IMG_V) {
            // in_proj rows regrouped pair-major: row tile = head pair, 8 rows per head (hd real + zero pad)
            const int head = 2 * rt + (row >> 3), j = row & 7;
            if (head < H && j < hd) {
                const int src = (kind - IMG_Q) * D + hd * head + j;          // row of in_proj_weight (3D x D)
                v = (k < D) ? W[(size_t)src * D + k] : (k == D ? bias[src] : 0.f);
                v *= scale;
            } else if ((kind == IMG_V || kind == IMG_K) && head < H && j == hd) {
                // "ones" feature in the free dim slot hd (through the bias slot).  V: the P.V MFMAs then also deliver
                // sum_j P[q, j] (the softmax denominator) in row hd of the head's O^T block.  K: a constant placed in
                // Q's slot hd is added to every score of the row by the S MFMA itself (the softmax shift).
                v = (k == D) ? 1.f : 0.f;
            }
        } else {   // IMG_WO: k-slot group (ks, g) = head 4ks+g, slot e = head dim
            const int d = 16 * rt + row, head = 4 * ks + g;
            if (d < D && head < H && e < hd) v = W[(size_t)d * D + hd * head + e];
        }
        dst[e] = (__bf16)v;
    }
}

__global__ __launch_bounds__(64) void k_build_image(int kind, const float* __restrict__ W, const float* __restrict__ bias,
                                                     __bf16* __restrict__ img, int KS, int rows, int K, int H, int hd,
                                                     int D, float scale) {
    build_image_block(kind, W, bias, img, KS, rows, K, H, hd, D, scale, blockIdx.x, threadIdx.x);
}

// ---- transposed-weight blocks of the bf16 backward pass (fd_train_bf16.hip)
// FFN backward image, chunk-major like the persistent kernel's forward image: block (c*2 + fh)*NB + j of chunk c, F-half fh
// (hidden units fbase = fh*F/2 + 32c .. +31):
//   j <  2*KS1 (ft, ks): A rows = hidden unit fbase+16ft+row, k = d:            W2[d = 32ks+8g+e][f]     (d hidden^T = W2^T d out^T)
//   j >= 2*KS1 (dt)    : A rows = d = 16dt+row, k-slots in the C-tile order of the two hidden tiles (e<4: f = fbase+4g+e,
//                        e>=4: f = fbase+16+4g+e-4):                              W1[f][d]                 (d x^T += W1^T d hidden^T)
__device__ void build_ffn_bwd_block(const float* __restrict__ W1, const float* __restrict__ W2, __bf16* __restrict__ img, int D,
                                    int F, int KS1, int DT, int blk, int lane) {
    const int NB = 2 * KS1 + DT;
    const int j = blk % NB, fh = (blk / NB) & 1, c = blk / (2 * NB);
    const int row = lane & 15, g = lane >> 4;
    const int fbase = fh * (F / 2) + c * 32;
    __bf16* dst = img + ((size_t)blk * 64 + lane) * 8;
    if (j < 2 * KS1) {
        const int ft = j / KS1, ks = j % KS1;
        const int f = fbase + 16 * ft + row;
        for (int e = 0; e < 8; ++e) {
            const int k = 32 * ks + 8 * g + e;
            dst[e] = (__bf16)((k < D) ? W2[(size_t)k * F + f] : 0.f);
        }
    } else {
        const int dt = j - 2 * KS1, d = 16 * dt + row;
        for (int e = 0; e < 8; ++e) {
            const int f = fbase + ((e < 4) ? (4 * g + e) : (16 + 4 * g + (e - 4)));
            dst[e] = (__bf16)((d < D) ? W1[(size_t)f * D + d] : 0.f);
        }
    }
}
// W_o^T block (dt, ks): A rows = attention feature i = 16dt+row (natural order head*hd + e), k = d = 32ks+8g+e: W_o[d][i]
__device__ void build_wot_block(const float* __restrict__ Wo, __bf16* __restrict__ img, int D, int KS1, int blk, int lane) {
    const int dt = blk / KS1, ks = blk - dt * KS1;
    const int row = lane & 15, g = lane >> 4, i = 16 * dt + row;
    __bf16* dst = img + ((size_t)blk * 64 + lane) * 8;
    for (int e = 0; e < 8; ++e) {
        const int d = 32 * ks + 8 * g + e;
        dst[e] = (__bf16)((i < D && d < D) ? Wo[(size_t)d * D + i] : 0.f);
    }
}
// in_proj^T half-blocks (512 B = 64 lanes x 4 bf16, K=16 MFMA) of head pair `pair`, which in {q,k,v}, row tile dt:
// A rows = d = 16dt+row, k-slot 4g+e = dim 4(g&1)+e of head 2pair+(g>>1): in_proj_weight[which*D + head*hd + j][d]
__device__ void build_win_block(const float* __restrict__ Win, __bf16* __restrict__ img, int D, int H, int hd, int DT, int blk,
                                int lane) {
    const int dt = blk % DT, which = (blk / DT) % 3, pair = blk / (3 * DT);
    const int row = lane & 15, g = lane >> 4, d = 16 * dt + row, head = 2 * pair + (g >> 1);
    __bf16* dst = img + ((size_t)blk * 64 + lane) * 4;
    for (int e = 0; e < 4; ++e) {
        const int j = 4 * (g & 1) + e;
        dst[e] = (__bf16)((d < D && head < H && j < hd) ? Win[(size_t)(which * D + head * hd + j) * D + d] : 0.f);
    }
}

// Every per-layer image of every layer in ONE launch (an optimizer step invalidates them all; 7 launches per layer made
// the rebuild the largest launch count of a training step).  grid (blocks per layer, L), one 64-lane block per image block.
struct fd_img_build {
    const float* P;
    const long long* lofs;     // [L][12] fd_layer_off
    char* mimg; size_t off_layers, layer_stride, off_wk, off_wv, off_wq, off_wo, off_ffn, off_lpar, off_ffn32;
    int n_ffn32;               // blocks of the pair-form FFN image per layer (0: not built)
    int* ffn32_bad;            // FD_RELU_CLAMP: count of pair-form weights outside the range the scaled image can hold
    char* ffn; size_t ffn_layer_bytes;
    char* bimg; size_t b_layer_stride, boff_ffn, boff_wot, boff_win;
    int D, F, H, hd, KS1, DT, KSO, NP;
    int n_qkv, n_wo, n_ffn, n_wot, n_win, n_lp;   // block counts per layer (n_qkv = NP*KS1 per matrix)
    int mega, train;
    float qscale;
    int blk_first;      // block index of grid block 0 (a partial rebuild starts inside the block list)
};
__global__ __launch_bounds__(64) void k_build_layer_images(const fd_img_build B) {
    const int l = blockIdx.y, lane = threadIdx.x;
    int blk = blockIdx.x + B.blk_first;
    const long long* lo = B.lofs + (size_t)l * 12;      // in_w, in_b, out_w, out_b, l1_w, l1_b, l2_w, l2_b, ...
    const float* P = B.P;
    // (1) inference FFN image [F-half][chunk][block]
    if (blk < B.n_ffn) {
        build_ffn_block(P + lo[4], P + lo[5], P + lo[6], (__bf16*)(B.ffn + (size_t)l * B.ffn_layer_bytes), B.D, B.F, B.KS1, B.DT, 0, blk, lane);
        return;
    }
    blk -= B.n_ffn;
    if (!B.mega) return;
    char* limg = B.mimg + B.off_layers + (size_t)l * B.layer_stride;
    if (blk < B.n_qkv) { build_image_block(IMG_K, P + lo[0], P + lo[1], (__bf16*)(limg + B.off_wk), B.KS1, 0, B.D, B.H, B.hd, B.D, 1.f, blk, lane); return; }
    blk -= B.n_qkv;
    if (blk < B.n_qkv) { build_image_block(IMG_V, P + lo[0], P + lo[1], (__bf16*)(limg + B.off_wv), B.KS1, 0, B.D, B.H, B.hd, B.D, 1.f, blk, lane); return; }
    blk -= B.n_qkv;
    if (blk < B.n_qkv) { build_image_block(IMG_Q, P + lo[0], P + lo[1], (__bf16*)(limg + B.off_wq), B.KS1, 0, B.D, B.H, B.hd, B.D, B.qscale, blk, lane); return; }
    blk -= B.n_qkv;
    if (blk < B.n_wo) { build_image_block(IMG_WO, P + lo[2], nullptr, (__bf16*)(limg + B.off_wo), B.KSO, 0, B.D, B.H, B.hd, B.D, 1.f, blk, lane); return; }
    blk -= B.n_wo;
    if (blk < B.n_ffn) { build_ffn_block(P + lo[4], P + lo[5], P + lo[6], (__bf16*)(limg + B.off_ffn), B.D, B.F, B.KS1, B.DT, 1, blk, lane); return; }
    blk -= B.n_ffn;
    if (blk < B.n_lp) {   // the layer's small fp32 vectors as one DMA-able block: [6][D] out_b, l2_b, n1_w, n1_b, n2_w, n2_b
        const int vsel[6] = {3, 7, 8, 9, 10, 11};
        float4 v;
        float* ve = reinterpret_cast<float*>(&v);
        for (int e = 0; e < 4; ++e) {
            const int i = (blk * 64 + lane) * 4 + e, vi = i / B.D, d = i - vi * B.D;
            ve[e] = (vi < 6) ? P[lo[vsel[vi]] + d] : 0.f;
        }
        *reinterpret_cast<float4*>(limg + B.off_lpar + ((size_t)blk * 64 + lane) * 16) = v;
        return;
    }
    blk -= B.n_lp;
    if (blk < B.n_ffn32) { build_ffn32_block(P + lo[4], P + lo[5], P + lo[6], (__bf16*)(limg + B.off_ffn32), B.D, B.F, B.DT, blk, lane, B.ffn32_bad); return; }
    blk -= B.n_ffn32;
    if (!B.train) return;
    char* bl = B.bimg + (size_t)l * B.b_layer_stride;
    if (blk < B.n_ffn) { build_ffn_bwd_block(P + lo[4], P + lo[6], (__bf16*)(bl + B.boff_ffn), B.D, B.F, B.KS1, B.DT, blk, lane); return; }
    blk -= B.n_ffn;
    if (blk < B.n_wot) { build_wot_block(P + lo[2], (__bf16*)(bl + B.boff_wot), B.D, B.KS1, blk, lane); return; }
    blk -= B.n_wot;
    if (blk < B.n_win) build_win_block(P + lo[0], (__bf16*)(bl + B.boff_win), B.D, B.H, B.hd, B.DT, blk, lane);
}

// ------------------------------------------------------------------ fused FFN + residual + LayerNorm
// out[m,:] = LN(x[m,:] + relu(x[m,:] W1^T + b1) W2^T + b2)   for the tokens of one workgroup.
//
// 8 waves = (2 token halves: mh) x (4 quarters of F: fq), two waves per SIMD; waves 0-3 (one per SIMD)
// take the first MT token tiles, waves 4-7 the rest, so every SIMD carries the same tile count.
// Each wave keeps DT x MT accumulator tiles in registers and walks its quarter of F in 32-wide chunks:
//   hidden^T(32 x 16 tokens) = W1 chunk . x^T      (2*KS1 MFMAs per token tile, bias through the K padding)
//   relu + bf16 in registers                         (the C tiles ARE the next B fragment)
//   out^T(D x 16 tokens)   += W2 chunk . hidden^T   (DT MFMAs per token tile)
// x^T B-fragments live in LDS (bf16, fragment order); the weight stream for all four F quarters is
// double-buffered in LDS by global_load_lds; one barrier per chunk step.
__device__ __forceinline__ float relu_bits(float x) {
    int i = __builtin_bit_cast(int, x);        // v_max_i32: relu on the IEEE bit pattern, no canonicalise
    i = i > 0 ? i : 0;
    return __builtin_bit_cast(float, i);
}
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    // vector fptrunc selects v_cvt_pk_bf16_f32 AND lets hipcc place the MFMA->VALU wait states itself
    // (an inline-asm cvt reading an MFMA result directly is not padded by the compiler: measured wrong data)
    typedef __attribute__((ext_vector_type(2))) float f32x2_t;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
__device__ __forceinline__ bf16x8 relu_pack(f32x4 a, f32x4 b) {
    u32x4 r;
    r[0] = cvt_pk_bf16(relu_bits(a[0]), relu_bits(a[1]));
    r[1] = cvt_pk_bf16(relu_bits(a[2]), relu_bits(a[3]));
    r[2] = cvt_pk_bf16(relu_bits(b[0]), relu_bits(b[1]));
    r[3] = cvt_pk_bf16(relu_bits(b[2]), relu_bits(b[3]));
    return __builtin_bit_cast(bf16x8, r);
}

// Wave roles: 8 waves = 4 token quarters (mq) x 2 halves of F (fh), two waves per SIMD.  The token tiles of
// the workgroup are dealt to the quarters as evenly as possible (e.g. 13 tiles -> 4,3,3,3) and the second
// set of waves is rotated by one quarter, so the two waves sharing a SIMD carry (4+3, 3+3, 3+3, 3+4) tiles.
// Optional fused prologue (KSO > 0): x is not read but computed in the kernel as
//   x = LayerNorm1(h0 + att . Wo^T + bo)      (attention out-projection + residual + norm1 of the encoder layer)
// from the attention output `att` (M, D) and the layer input `h0`: one launch and two (M, D) fp32 round trips less per
// layer on the step-by-step path.  The tile's fp32 x then never leaves the CU: it seeds the owner wave's accumulators.
struct fd_ffn_pre {
    const float* att;     // (M, D) concatenated head outputs, fp32 rows -- or bf16 rows when att_bf16 (k_attention_bf16 out_bf16)
    int att_bf16;
    const float* h0;      // (M, D) layer input (residual)
    const char* wo_img;   // [DT][KSO] 1 KiB fragment blocks of W_o (IMG_WO)
    const float* bo;
    const float* g1;
    const float* b1;
    int H, hd;
    // the layer OUTPUT also as bf16 rows (M, 32 KS1 k-slots; 1.0 in slot D, zero padding) for the next layer's attention staging
    // (k_attention_bf16's ROWS form), or null
    __bf16* out_rows;
};

#ifndef FD_FFN_JOINT
#define FD_FFN_JOINT 1          // bit 0: the fused prologue runs a wave's two tiles in one basic block; bit 1: the epilogue too (measured slower)
#endif
#ifdef FD_FFN_PROF           // variant build: in-kernel phase clocks of k_ffn_ln (workgroup 3, waves 0 and 4), printed after 40 launches
__device__ unsigned long long fd_ffn_dbg[2 * 8];
#define FFN_STAMP(slot, t_prev)                                                                          \
    do {                                                                                                 \
        const unsigned long long now_ = __builtin_readcyclecounter();                                    \
        if (blockIdx.x == 3 && lane == 0 && (wave & 3) == 0) fd_ffn_dbg[(wave >> 2) * 8 + (slot)] += now_ - (t_prev); \
        (t_prev) = now_;                                                                                 \
    } while (0)
#else
#define FFN_STAMP(slot, t_prev) do { } while (0)
#endif
template <int KS1, int DT, int MT, int KSO>
__global__ __launch_bounds__(512, 2) void k_ffn_ln(const float* __restrict__ x, float* __restrict__ out,
                                                    const char* __restrict__ wimg, const float* __restrict__ b2,
                                                    const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, int M, int D, int F,
                                                    int tok_per_wg, fd_ffn_pre pre) {
    constexpr int NB = 2 * KS1 + DT;            // 1 KiB fragment blocks per (F-half, 32-wide chunk)
    constexpr int SUB = 2;                      // chunks per barrier step
    constexpr int WBUF = 2 * SUB * NB * 1024;   // both F-halves of one step
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fh = wave >> 2;
    const int mq = (wave + fh) & 3;
    const int tok = lane & 15, g = lane >> 4;
    const int NS = F / (64 * SUB);              // barrier steps per F-half
    const int m_wg = blockIdx.x * tok_per_wg;
    const int m_end = min(M, m_wg + tok_per_wg);
    const int tiles = (m_end - m_wg + 15) >> 4;
    const int tbase = tiles >> 2, trem = tiles & 3;
    const int ntile = tbase + (mq < trem ? 1 : 0);                 // this wave's token tiles (<= MT)
    const int tile0 = mq * tbase + (mq < trem ? mq : trem);

    // ---- weight stream: L2 -> LDS, 1 KiB per wave-instruction, blocks dealt round-robin to the 8 waves.
    // image order: [fh][step][sub][NB]  ->  LDS buffer [fh][sub][NB]
    constexpr int NDMA = (2 * SUB * NB + 7) / 8;           // DMA instructions per wave and step (padding copies repeat a block)
    auto issue_dma = [&](int st, int buf) {
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            int b = wave + 8 * i;
            b -= (b >= 2 * SUB * NB) ? 2 * SUB * NB : 0;
            {
                const int h = b / (SUB * NB);
                const int j = b - h * (SUB * NB);
                const char* src = wimg + ((((size_t)h * NS + st) * SUB * NB + j) * 64 + lane) * 16;
                char* dst = smem + buf * WBUF + b * 1024;
                __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(dst), 16, 0, 0);
            }
        }
    };
    unsigned long long tprev = __builtin_readcyclecounter();
    (void)tprev;
    issue_dma(0, 0);
    // The six small fp32 vectors of the kernel (b_o, gamma1, beta1 of the fused prologue; b2, gamma2, beta2 of the epilogue) go to
    // LDS once per workgroup, [vector][4 DT float4], zero beyond D.  Read where they were used -- inside the lane-divergent
    // `if (d0 < D)` / `if (valid)` branches of the per-tile code -- every load was waited for at the end of its branch: about ten
    // dependent L2 round trips per token tile, 11.7 K cycles per tile in the phase clocks (profiles/r05_long_ffn_ln_phase_clocks.txt);
    // hoisted into registers instead they pushed the kernel (256 VGPRs, two waves per SIMD) into spills and made it slower.
    constexpr size_t XFR_BYTES = KSO > 0 ? (size_t)4 * MT * KS1 * 1024 : 0;
    float4* const lvec = reinterpret_cast<float4*>(smem + 2 * WBUF + XFR_BYTES);       // (behind the ring and the x fragments)
    float4 lval = {0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x < 6 * 4 * DT) {
        const int v = threadIdx.x / (4 * DT), c = threadIdx.x - v * (4 * DT);
        const float* src = v == 0 ? pre.bo : v == 1 ? pre.g1 : v == 2 ? pre.b1 : v == 3 ? b2 : v == 4 ? gamma : beta;
        if (4 * c < D && (KSO > 0 || v >= 3)) lval = *reinterpret_cast<const float4*>(src + 4 * c);
    }
    auto lvec_store = [&]() {                               // (in front of the first barrier behind the load)
        if (threadIdx.x < 6 * 4 * DT) lvec[threadIdx.x] = lval;
    };

    // ---- activations -> bf16 B fragments in registers (token on lane&15, 8 features per lane, "1.0" in slot D)
    bf16x8 xf[MT][KS1];
    f32x4 acc[DT][MT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int tt = 0; tt < MT; ++tt) acc[dt][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (KSO > 0) {
        char* const xfr = smem + 2 * WBUF;                 // [4*MT tiles][KS1][64][16 B]: x fragments of this workgroup
        // W_o fragment image -> ring buffer 1 (free until the chunk loop's first step refills it behind the prologue's barrier):
        // 60 VGPRs of fragments per wave became 15 LDS reads per tile, which is what lets a wave hold BOTH of its tiles' input
        // rows in flight below.
        char* const wos = smem + WBUF;
        constexpr int KSOn = KSO > 0 ? KSO : 1;
#pragma unroll
        for (int i = 0; i < (DT * KSOn + 7) / 8; ++i) {
            const int bq = wave + 8 * i;
            if (bq < DT * KSOn)
                __builtin_amdgcn_global_load_lds(GLB_PTR(pre.wo_img + ((size_t)bq * 64 + lane) * 16), LDS_PTR(wos + bq * 1024), 16, 0, 0);
        }
        // The input rows of this wave's (at most two) tiles: the attention rows of its heads and the residual rows, unconditional
        // loads from clamped addresses (selected at their use), all issued before the first wait.
        typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
        struct TileIn {
            u32x4 a[KSOn];
            float4 r[DT];
        };
        TileIn tin[2];
        auto tile_load = [&](int tt, TileIn& in) {
            const int m = m_wg + (tile0 + tt) * 16 + tok;
            const int mr = m < m_end ? m : m_wg;
            if (pre.att_bf16) {
#pragma unroll
                for (int ks = 0; ks < KSO; ++ks) {
                    const int head = 4 * ks + g, hc = head < pre.H ? head : pre.H - 1;
                    in.a[ks] = *reinterpret_cast<const u32x4_a4*>(reinterpret_cast<const __bf16*>(pre.att) + (size_t)mr * D + hc * pre.hd);
                }
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d0 = 16 * dt + 4 * g, dr = d0 < D ? d0 : 0;
                in.r[dt] = *reinterpret_cast<const float4*>(pre.h0 + (size_t)mr * D + dr);
            }
        };
#pragma unroll
        for (int tt = 0; tt < MT; ++tt) {
            if (tt >= ntile || (tt & 1) != fh) continue;   // the two waves of a token quarter split its tiles
            tile_load(tt, tin[tt >> 1]);
        }
        // (the first weight buffer requested LAST and not waited for here -- all 256 workgroups fetch the same 44 KiB at the same
        //  moment -- measured slower: 2.456 -> 2.495 ms per step at the droughts shape, 1.340 -> 1.348 at T = 1024)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // first weight buffer (own share), W_o image, vectors, the tiles' rows
        lvec_store();
        __syncthreads();
        FFN_STAMP(6, tprev);          // requests issued, landed, barrier
        // out-projection + residual + LayerNorm1 of NT (1 or 2) tiles in ONE basic block: the two tiles a wave owns in the common
        // case (tt = fh, fh + 2 of a full quarter) are two independent chains of LDS reads -> MFMAs -> cross-lane sums -> LDS writes;
        // one after the other (a predicated `continue` per tile) each ran at its own latency, 5 K cycles per tile in the phase clocks.
        auto pro_tiles = [&](auto t0c, auto t1c) {
            constexpr int T0 = decltype(t0c)::value, T1 = decltype(t1c)::value, NT = T1 >= 0 ? 2 : 1;
            constexpr int TT[2] = {T0, T1 >= 0 ? T1 : T0};
            int m[NT];
            bool valid[NT];
            f32x4 o[NT][DT];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                m[i] = m_wg + (tile0 + TT[i]) * 16 + tok;
                valid[i] = m[i] < m_end;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ks = 0; ks < KSO; ++ks) {
                const int head = 4 * ks + g;               // k-slot group g of k-step ks = the 8 (padded) dims of one head
                bf16x8 af[NT];
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const TileIn& in = tin[TT[i] >> 1];
                    u32x4 pk;
                    const int mc = valid[i] ? m[i] : m_wg, hc = head < pre.H ? head : pre.H - 1;
                    const bool ok = valid[i] && head < pre.H;
                    if (pre.att_bf16) {
                        // bf16 rows written by k_attention_bf16 (the rounding this prologue would do, done at the producer): ONE
                        // 16-byte load per (token, head) at a dword-aligned address (head_dim even), slot pairs >= head_dim cleared
#pragma unroll
                        for (int e = 0; e < 4; ++e) pk[e] = (ok && 2 * e < pre.hd) ? in.a[ks][e] : 0u;
                    } else {
                        // fp32 rows (odd head_dim): the head's 8 dim slots as two dword-aligned 16-byte loads from a clamped address,
                        // selected afterwards (slots >= head_dim read the next head / row: `att` is carved with 8 floats of slack)
                        float v[8];
                        typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
                        const f32x4_a4* p8 = reinterpret_cast<const f32x4_a4*>(pre.att + (size_t)mc * D + hc * pre.hd);
                        const f32x4_a4 lo = p8[0], hi = p8[1];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[e] = (ok && e < pre.hd) ? lo[e] : 0.f;
                            v[4 + e] = (ok && 4 + e < pre.hd) ? hi[e] : 0.f;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) pk[e] = cvt_pk_bf16(v[2 * e], v[2 * e + 1]);
                    }
                    af[i] = __builtin_bit_cast(bf16x8, pk);
                }
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wos + ((size_t)(dt * KSOn + ks) * 64 + lane) * 16);
#pragma unroll
                    for (int i = 0; i < NT; ++i) o[i][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[i], o[i][dt], 0, 0, 0);
                }
            }
            float sm[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) sm[i] = 0.f;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d0 = 16 * dt + 4 * g;
                const float4 bb = lvec[0 * 4 * DT + 4 * dt + g];        // (zero beyond D)
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const float4 zero4 = {0.f, 0.f, 0.f, 0.f};
                    const float4 r0 = valid[i] ? tin[TT[i] >> 1].r[dt] : zero4;
                    if (d0 < D) {
                        o[i][dt][0] += bb.x + r0.x; o[i][dt][1] += bb.y + r0.y; o[i][dt][2] += bb.z + r0.z; o[i][dt][3] += bb.w + r0.w;
                        sm[i] += (o[i][dt][0] + o[i][dt][1]) + (o[i][dt][2] + o[i][dt][3]);
                    } else {
                        o[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
            }
            float mean[NT], rstd[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                sm[i] += __shfl_xor(sm[i], 16);
                sm[i] += __shfl_xor(sm[i], 32);
                mean[i] = sm[i] / (float)D;
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                float q = 0.f;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    if (16 * dt + 4 * g < D) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float c = o[i][dt][r] - mean[i];
                            q += c * c;
                        }
                    }
                q += __shfl_xor(q, 16);
                q += __shfl_xor(q, 32);
                rstd[i] = rsqrtf(q / (float)D + 1e-5f);
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d0 = 16 * dt + 4 * g;
                const float4 gm = lvec[1 * 4 * DT + 4 * dt + g];
                const float4 bt = lvec[2 * 4 * DT + 4 * dt + g];
                // C layout (feature 16dt + 4g + r) -> B fragment k-slot of the same feature index
                const int ks = dt >> 1, gd = 2 * (dt & 1) + (g >> 1);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    u32x2 pk = {0u, 0u};
                    if (d0 < D) {
                        o[i][dt][0] = valid[i] ? (o[i][dt][0] - mean[i]) * rstd[i] * gm.x + bt.x : 0.f;
                        o[i][dt][1] = valid[i] ? (o[i][dt][1] - mean[i]) * rstd[i] * gm.y + bt.y : 0.f;
                        o[i][dt][2] = valid[i] ? (o[i][dt][2] - mean[i]) * rstd[i] * gm.z + bt.z : 0.f;
                        o[i][dt][3] = valid[i] ? (o[i][dt][3] - mean[i]) * rstd[i] * gm.w + bt.w : 0.f;
                        pk[0] = cvt_pk_bf16(o[i][dt][0], o[i][dt][1]);
                        pk[1] = cvt_pk_bf16(o[i][dt][2], o[i][dt][3]);
                    } else if (d0 == D && valid[i]) {
                        pk[0] = 0x00003F80u;                   // bf16(1.0): bias row of the K padding
                    }
                    if (ks < KS1)
                        *reinterpret_cast<u32x2*>(xfr + (((size_t)(tile0 + TT[i]) * KS1 + ks) * 64 + gd * 16 + tok) * 16 + 8 * (g & 1)) = pk;
                    acc[dt][TT[i]] = o[i][dt];                 // residual of the FFN block: out = x + b2 + W2 relu(..)
                }
            }
            // k-slots beyond 16*DT (K padding of the last k-step) must read as zero
            if (16 * DT < 32 * KS1) {
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int slot = 16 * DT + 4 * g; slot < 32 * KS1; slot += 16)
                        *reinterpret_cast<u32x2*>(xfr + (((size_t)(tile0 + TT[i]) * KS1 + (slot >> 5)) * 64 + ((slot & 31) >> 3) * 16 + tok) * 16 +
                                                  8 * ((slot >> 2) & 1)) = u32x2{0u, 0u};
            }
        };
        using std::integral_constant;
        if ((FD_FFN_JOINT & 1) && MT == 4 && ntile == MT) {
            if (fh == 0) pro_tiles(integral_constant<int, 0>{}, integral_constant<int, (MT == 4 ? 2 : -1)>{});
            else pro_tiles(integral_constant<int, (MT == 4 ? 1 : 0)>{}, integral_constant<int, (MT == 4 ? 3 : -1)>{});
        } else {
            if (0 < ntile && fh == 0) pro_tiles(integral_constant<int, 0>{}, integral_constant<int, -1>{});
            if (MT > 1 && 1 < ntile && fh == 1) pro_tiles(integral_constant<int, (MT > 1 ? 1 : 0)>{}, integral_constant<int, -1>{});
            if (MT > 2 && 2 < ntile && fh == 0) pro_tiles(integral_constant<int, (MT > 2 ? 2 : 0)>{}, integral_constant<int, -1>{});
            if (MT > 3 && 3 < ntile && fh == 1) pro_tiles(integral_constant<int, (MT > 3 ? 3 : 0)>{}, integral_constant<int, -1>{});
        }
        FFN_STAMP(0, tprev);          // prologue: out-projection + LN1 of this wave's tiles, fragments written
        __syncthreads();
        FFN_STAMP(1, tprev);          // barrier
#pragma unroll
        for (int tt = 0; tt < MT; ++tt)
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks)
                xf[tt][ks] = (tt < ntile) ? *reinterpret_cast<const bf16x8*>(xfr + (((size_t)(tile0 + tt) * KS1 + ks) * 64 + lane) * 16)
                                          : bf16x8{};
    } else
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
        const int m = m_wg + (tile0 + tt) * 16 + tok;
        const bool valid = (tt < ntile) && (m < m_end);
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            const int k0 = 32 * ks + 8 * g;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
            if (valid) {
                if (k0 + 8 <= D) {
                    const float4 a = *reinterpret_cast<const float4*>(x + (size_t)m * D + k0);
                    const float4 b = *reinterpret_cast<const float4*>(x + (size_t)m * D + k0 + 4);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
                    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int k = k0 + e;
                        if (k < D) v[e] = x[(size_t)m * D + k];
                        else if (k == D) v[e] = 1.0f;          // bias row of the K padding
                    }
                }
            }
            u32x4 pk;
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[e] = cvt_pk_bf16(v[2 * e], v[2 * e + 1]);
            xf[tt][ks] = __builtin_bit_cast(bf16x8, pk);
        }
    }

    if (KSO == 0) lvec_store();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    FFN_STAMP(2, tprev);              // fragments read, first weight buffer landed, barrier

    // The chunk loop is instantiated for "every tile present" (the common case: one basic block per chunk, the tiles' LDS reads /
    // MFMAs / relu interleave) and once with the per-tile guard; with the guard alone every tile was its own basic block and
    // ran H -> relu -> W2 strictly in sequence (the finding of fd_mega.hip's FFN loop, never applied here).
    auto chunk_loop = [&](auto fullc) {
    constexpr bool FULL = decltype(fullc)::value;
    int buf = 0;
    for (int st = 0; st < NS; ++st) {
#ifndef FD_ABLATE_NODMA
        if (st + 1 < NS) issue_dma(st + 1, buf ^ 1);
#endif
#pragma unroll
        for (int sub = 0; sub < SUB; ++sub) {
#ifdef FD_ABLATE_NOMFMA
            if (st > 0) continue;
#endif
            const char* wb = smem + buf * WBUF + (fh * SUB + sub) * NB * 1024 + lane * 16;
            bf16x8 w1[2][KS1], w2[DT];
#pragma unroll
            for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks)
                    w1[ft][ks] = *reinterpret_cast<const bf16x8*>(wb + (ft * KS1 + ks) * 1024);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                w2[dt] = *reinterpret_cast<const bf16x8*>(wb + (2 * KS1 + dt) * 1024);
#pragma unroll
            for (int tt = 0; tt < MT; ++tt) {
                if (FULL || tt < ntile) {
                    f32x4 h0 = f32x4{0.f, 0.f, 0.f, 0.f}, h1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS1; ++ks) {
                        h0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[0][ks], xf[tt][ks], h0, 0, 0, 0);
                        h1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[1][ks], xf[tt][ks], h1, 0, 0, 0);
                    }
#ifdef FD_ABLATE_NORELU
                    u32x4 hraw = {__builtin_bit_cast(unsigned, h0[0]), __builtin_bit_cast(unsigned, h0[1]),
                                  __builtin_bit_cast(unsigned, h1[0]), __builtin_bit_cast(unsigned, h1[1])};
                    const bf16x8 hb = __builtin_bit_cast(bf16x8, hraw);
#else
                    const bf16x8 hb = relu_pack(h0, h1);
#endif
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        acc[dt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[dt], hb, acc[dt][tt], 0, 0, 0);
                }
            }
        }
#ifndef FD_ABLATE_NOBAR
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
#endif
    }
    };
    if (ntile == MT) chunk_loop(std::true_type{});
    else chunk_loop(std::false_type{});
    FFN_STAMP(3, tprev);              // chunk loop

#ifdef FD_ABLATE_NOEPI
    if (acc[0][0][0] != 12345.678f) return;
#endif
    // ---- combine the two F-halves through LDS; tile tt is finalised by the wave with (tt & 1) == fh
    f32x4* xch = reinterpret_cast<f32x4*>(smem);       // [mq][tt][dt][lane]
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
        if (tt < ntile && (tt & 1) != fh) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) xch[((mq * MT + tt) * DT + dt) * 64 + lane] = acc[dt][tt];
        }
    }
    __syncthreads();
    FFN_STAMP(4, tprev);              // exchange of the F-halves
    // residual + b2 + LayerNorm2 + stores of NT (1 or 2) tiles in one basic block (see the prologue)
    auto epi_tiles = [&](auto t0c, auto t1c) {
        constexpr int T0 = decltype(t0c)::value, T1 = decltype(t1c)::value, NT = T1 >= 0 ? 2 : 1;
        constexpr int TT[2] = {T0, T1 >= 0 ? T1 : T0};
        int m[NT];
        bool valid[NT];
        float v[NT][DT][4];
        float sum[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            m[i] = m_wg + (tile0 + TT[i]) * 16 + tok;
            valid[i] = m[i] < m_end;
            sum[i] = 0.f;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d0 = 16 * dt + 4 * g;
            const bool dv = d0 < D;                          // D % 4 == 0: a 4-group is all-valid or all-pad
            const float4 bb = lvec[3 * 4 * DT + 4 * dt + g];     // (zero beyond D)
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const f32x4 tot = acc[dt][TT[i]] + xch[((mq * MT + TT[i]) * DT + dt) * 64 + lane];
                float4 res = {0.f, 0.f, 0.f, 0.f};
                if (KSO == 0) {                              // (fused prologue: the residual is already in acc)
                    const int mr = valid[i] ? m[i] : m_wg, dr = dv ? d0 : 0;
                    const float4 rr = *reinterpret_cast<const float4*>(x + (size_t)mr * D + dr);
                    if (valid[i] && dv) res = rr;
                }
                v[i][dt][0] = dv ? tot[0] + bb.x + res.x : 0.f;
                v[i][dt][1] = dv ? tot[1] + bb.y + res.y : 0.f;
                v[i][dt][2] = dv ? tot[2] + bb.z + res.z : 0.f;
                v[i][dt][3] = dv ? tot[3] + bb.w + res.w : 0.f;
                sum[i] += (v[i][dt][0] + v[i][dt][1]) + (v[i][dt][2] + v[i][dt][3]);
            }
        }
        float mean[NT], rstd[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            sum[i] += __shfl_xor(sum[i], 16);
            sum[i] += __shfl_xor(sum[i], 32);
            mean[i] = sum[i] / (float)D;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            float q = 0.f;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (16 * dt + 4 * g < D) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float cdev = v[i][dt][r] - mean[i];
                        q += cdev * cdev;
                    }
                }
            }
            q += __shfl_xor(q, 16);
            q += __shfl_xor(q, 32);
            rstd[i] = rsqrtf(q / (float)D + 1e-5f);
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d0 = 16 * dt + 4 * g;
            const float4 gm = lvec[4 * 4 * DT + 4 * dt + g];
            const float4 bt = lvec[5 * 4 * DT + 4 * dt + g];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                if (valid[i] && d0 < D) {
                    float4 o;
                    o.x = (v[i][dt][0] - mean[i]) * rstd[i] * gm.x + bt.x;
                    o.y = (v[i][dt][1] - mean[i]) * rstd[i] * gm.y + bt.y;
                    o.z = (v[i][dt][2] - mean[i]) * rstd[i] * gm.z + bt.z;
                    o.w = (v[i][dt][3] - mean[i]) * rstd[i] * gm.w + bt.w;
                    *reinterpret_cast<float4*>(out + (size_t)m[i] * D + d0) = o;
                    v[i][dt][0] = o.x; v[i][dt][1] = o.y; v[i][dt][2] = o.z; v[i][dt][3] = o.w;
                }
            }
        }
        if (pre.out_rows) {
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                if (!valid[i]) continue;
                __bf16* rrow = pre.out_rows + (size_t)m[i] * (32 * KS1);
#pragma unroll
                for (int dt = 0; dt < 2 * KS1; ++dt) {
                    const int d0 = 16 * dt + 4 * g;
                    u32x2 pk = {0u, 0u};
                    if (dt < DT && d0 < D) {
                        pk[0] = cvt_pk_bf16(v[i][dt < DT ? dt : 0][0], v[i][dt < DT ? dt : 0][1]);
                        pk[1] = cvt_pk_bf16(v[i][dt < DT ? dt : 0][2], v[i][dt < DT ? dt : 0][3]);
                    } else if (d0 == D) {
                        pk[0] = 0x00003F80u;
                    }
                    *reinterpret_cast<u32x2*>(rrow + d0) = pk;
                }
            }
        }
    };
    {
        using std::integral_constant;
        if ((FD_FFN_JOINT & 2) && MT == 4 && ntile == MT) {
            if (fh == 0) epi_tiles(integral_constant<int, 0>{}, integral_constant<int, (MT == 4 ? 2 : -1)>{});
            else epi_tiles(integral_constant<int, (MT == 4 ? 1 : 0)>{}, integral_constant<int, (MT == 4 ? 3 : -1)>{});
        } else {
            if (0 < ntile && fh == 0) epi_tiles(integral_constant<int, 0>{}, integral_constant<int, -1>{});
            if (MT > 1 && 1 < ntile && fh == 1) epi_tiles(integral_constant<int, (MT > 1 ? 1 : 0)>{}, integral_constant<int, -1>{});
            if (MT > 2 && 2 < ntile && fh == 0) epi_tiles(integral_constant<int, (MT > 2 ? 2 : 0)>{}, integral_constant<int, -1>{});
            if (MT > 3 && 3 < ntile && fh == 1) epi_tiles(integral_constant<int, (MT > 3 ? 3 : 0)>{}, integral_constant<int, -1>{});
        }
    }
    FFN_STAMP(5, tprev);              // LN2 + stores of this wave's tiles
}

template <int KS1, int DT, int MT, int KSO>
int launch_ffn(fd_ctx* ctx, const float* x, float* out, const char* wimg, const float* b2, const float* gamma,
               const float* beta, int M, int D, int F, int tok_per_wg, const fd_ffn_pre& pre, hipStream_t s) {
    constexpr int NB = 2 * KS1 + DT;
    constexpr size_t lds_main = 2 * (size_t)2 * 2 * NB * 1024;         // 2 buffers x 2 F-halves x SUB chunks
    constexpr size_t lds_xch = (size_t)4 * MT * DT * 1024;
    constexpr size_t lds_xfr = KSO > 0 ? (size_t)4 * MT * KS1 * 1024 : 0;   // fused prologue: x fragments behind the ring
    constexpr size_t lds_vec = (size_t)6 * 4 * DT * 16;                       // the six fp32 vectors as float4 [vector][4 DT]
    static_assert(lds_main >= lds_xch, "the vectors sit behind ring + x fragments: the exchange area must not reach them");
    const size_t lds = lds_main + lds_xfr + lds_vec;
    auto kern = k_ffn_ln<KS1, DT, MT, KSO>;
    static unsigned long long attr = 0;
    if (fd_first_on_device(attr, ctx->device))
        FD_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int grid = (M + tok_per_wg - 1) / tok_per_wg;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, s, x, out, wimg, b2, gamma, beta, M, D, F, tok_per_wg, pre);
    FD_LAUNCH_CHECK(ctx);
#ifdef FD_FFN_PROF
    {
        static int calls = 0;
        if (++calls == 40) {
            unsigned long long h[16];
            hipStreamSynchronize(s);
            hipMemcpyFromSymbol(h, HIP_SYMBOL(fd_ffn_dbg), sizeof(h));
            for (int w = 0; w < 2; ++w)
                fprintf(stderr, "[ffn_ln dbg] MT=%d tok_per_wg=%d grid=%d wave %d over %d launches: requests + wait + barrier %llu, out-proj + LN1 of the tiles %llu, barrier %llu, frags + first buffer %llu, chunk loop %llu, exchange %llu, epilogue %llu cycles\n",
                        MT, tok_per_wg, grid, 4 * w, calls, h[w * 8 + 6] / calls, h[w * 8 + 0] / calls, h[w * 8 + 1] / calls, h[w * 8 + 2] / calls, h[w * 8 + 3] / calls,
                        h[w * 8 + 4] / calls, h[w * 8 + 5] / calls);
        }
    }
#endif
    return FD_OK;
}

// tokens per workgroup: whole "rounds" of one workgroup per CU, each WG at most 4*MTMAX tiles.  MTMAX = 4 (256 tokens) for the
// widths up to d_model 95; the wider classes hold DT x MT accumulator tiles + MT x KS1 fragments per wave in 256 VGPRs only
// with fewer token tiles per wave (d_model 96..127: 3, d_model 128..143: 2).
template <int KS1, int DT, int KSO, int MTMAX = 4>
int dispatch_ffn(fd_ctx* ctx, const float* x, float* out, const char* wimg, const float* b2, const float* gamma,
                 const float* beta, int M, int D, int F, const fd_ffn_pre& pre, hipStream_t s) {
    const long long tcap = 64LL * MTMAX;
    const long long cap = tcap * ctx->num_cu;
    const int rounds = (int)((M + cap - 1) / cap);
    int tok = (int)((M + (long long)rounds * ctx->num_cu - 1) / ((long long)rounds * ctx->num_cu));
    if (tok > tcap) tok = (int)tcap;
    if (tok < 16) tok = 16;
    const int mt = ((tok + 15) / 16 + 3) / 4;       // tiles of the fullest token quarter
    if (mt <= 1) return launch_ffn<KS1, DT, 1, KSO>(ctx, x, out, wimg, b2, gamma, beta, M, D, F, tok, pre, s);
    if (mt == 2) return launch_ffn<KS1, DT, 2, KSO>(ctx, x, out, wimg, b2, gamma, beta, M, D, F, tok, pre, s);
    if constexpr (MTMAX >= 3) {
        if (mt == 3) return launch_ffn<KS1, DT, 3, KSO>(ctx, x, out, wimg, b2, gamma, beta, M, D, F, tok, pre, s);
    }
    if constexpr (MTMAX >= 4) return launch_ffn<KS1, DT, 4, KSO>(ctx, x, out, wimg, b2, gamma, beta, M, D, F, tok, pre, s);
    return fd_fail(ctx, FD_ERR_UNSUPPORTED, "k_ffn_ln: %d token tiles per wave exceed this width class", mt);
}

// x != nullptr: out = LN2(x + FFN(x)).  x == nullptr: x = LN1(h0 + att Wo^T + bo) is computed in the kernel (fused
// prologue; needs the persistent kernel's W_o image), then the same.
int run_ffn(fd_score* m, const float* x, float* out, int layer, int M, hipStream_t s, const float* att = nullptr,
            const float* h0 = nullptr, int att_bf16 = 0, __bf16* out_rows = nullptr) {
    fd_ctx* ctx = m->ctx;
    const fd_bf16_images* im = m->bf16;
    const fd_layer_off& lo = m->layers[layer];
    const float* P = m->params;
    const char* wimg = im->ffn + (size_t)layer * im->ffn_layer_bytes;
    const int D = m->d.d_model, F = m->d.dim_ff;
    fd_ffn_pre pre{};
    pre.out_rows = out_rows;
    if (!x) {
        pre.att = att; pre.h0 = h0; pre.att_bf16 = att_bf16;
        pre.wo_img = im->mimg + im->off_layers + (size_t)layer * im->layer_stride + im->off_wo;
        pre.bo = P + lo.out_b; pre.g1 = P + lo.n1_w; pre.b1 = P + lo.n1_b;
        pre.H = m->d.n_head; pre.hd = D / m->d.n_head;
        if (im->ks1 == 3 && im->dt == 5 && im->kso == 3)
            return dispatch_ffn<3, 5, 3>(ctx, x, out, wimg, P + lo.l2_b, P + lo.n2_w, P + lo.n2_b, M, D, F, pre, s);
        if (im->ks1 == 2 && im->dt == 4 && im->kso == 3)
            return dispatch_ffn<2, 4, 3>(ctx, x, out, wimg, P + lo.l2_b, P + lo.n2_w, P + lo.n2_b, M, D, F, pre, s);
        return fd_fail(ctx, FD_ERR_UNSUPPORTED, "fused out-proj + FFN kernel not instantiated for d_model=%d", D);
    }
#define FD_FFN_CASE(K, T_, MTMAX_)                                                                             \
    if (im->ks1 == K && im->dt == T_)                                                                          \
        return dispatch_ffn<K, T_, 0, MTMAX_>(ctx, x, out, wimg, P + lo.l2_b, P + lo.n2_w, P + lo.n2_b, M, D, F, pre, s);
    // (KS1, DT) = (k-steps of d_model + 1 bias slot, 16-row tiles of d_model + 1 ones row): every d_model % 4 == 0 up to 143
    FD_FFN_CASE(3, 5, 4)   // d_model 64 .. 79 (72: hydra default)
    FD_FFN_CASE(2, 4, 4)   // d_model 48 .. 63 (60: class default)
    FD_FFN_CASE(1, 2, 4)   // d_model 16 .. 31
    FD_FFN_CASE(1, 1, 4)   // d_model  4 .. 15
    FD_FFN_CASE(2, 3, 4)   // d_model 32 .. 47
    FD_FFN_CASE(3, 6, 4)   // d_model 80 .. 95
    FD_FFN_CASE(4, 7, 3)   // d_model 96 .. 111
    FD_FFN_CASE(4, 8, 3)   // d_model 112 .. 127
    FD_FFN_CASE(5, 9, 2)   // d_model 128 .. 143
#undef FD_FFN_CASE
    return fd_fail(ctx, FD_ERR_UNSUPPORTED, "bf16 FFN kernel not instantiated for d_model=%d", D);
}

}  // namespace

// ------------------------------------------------------------------ object plumbing
int fd_bf16_create(fd_score* m) {
    fd_bf16_images* im = new fd_bf16_images();
    const int D = m->d.d_model, F = m->d.dim_ff, H = m->d.n_head, C = m->d.n_channels, L = m->d.num_layers;
    const int hd = D / H;
    im->ks1 = (D + 1 + 31) / 32;
    // 16-row tiles of the d_model features PLUS the ones row (bias column of the weight gradients, softmax denominator row ...):
    // always one spare row, so d_model = 16, 48, 64, ... share the class of the next larger widths instead of having none
    im->dt = (D + 1 + 15) / 16;
    im->kso = (8 * H + 31) / 32;
    im->kse = (C + 1 + 31) / 32;
    im->ct = (C + 15) / 16;
    im->np = (H + 1) / 2;
    // FFN kernel instantiations (run_ffn): every d_model % 4 == 0 up to 143; the persistent kernel, the fused attention
    // kernel and the bf16 training kernels exist for the four classes of `inst_mega` and head_dim <= 7 -- outside them the
    // bf16 mode runs fp32-MFMA projections + (head_dim <= 7: bf16, else exact-f32) attention + the bf16 FFN kernel
    const bool inst = (im->ks1 == 3 && im->dt == 5) || (im->ks1 == 2 && im->dt == 4) ||
                      (im->ks1 == 1 && im->dt == 2) || (im->ks1 == 1 && im->dt == 1) ||
                      (im->ks1 == 2 && im->dt == 3) || (im->ks1 == 3 && im->dt == 6) ||
                      (im->ks1 == 4 && im->dt == 7) || (im->ks1 == 4 && im->dt == 8) || (im->ks1 == 5 && im->dt == 9);
    im->supported = inst && (D % 4 == 0) && (F % 128 == 0) && L > 0;
    const bool inst_mega = (im->ks1 == 3 && im->dt == 5 && im->kso == 3) || (im->ks1 == 2 && im->dt == 4 && im->kso == 3) ||
                           (im->ks1 == 1 && im->dt == 2 && im->kso == 1) || (im->ks1 == 1 && im->dt == 1 && im->kso == 1);
    // hd <= 7: a free slot per head carries the softmax shift / the row of ones; hd == 8 in the class <3,5,2> (d_model 64, 8 heads):
    // the persistent kernel's exact two-pass form with the denominators from an all-ones MFMA (fd_mega.hip HD8)
    const bool mega_hd8 = hd == 8 && ((im->ks1 == 3 && im->dt == 5 && im->kso == 2) || (im->ks1 == 2 && im->dt == 3 && im->kso == 1));
    im->mega = im->supported && ((inst_mega && hd <= 7) || mega_hd8) && D < 16 * im->dt && C <= 40;
    // bf16 training kernels (fd_train_bf16.hip): the persistent kernel's classes, plus head_dim 8 (two heads still share the 16
    // k-slots of one score MFMA; the training kernels sum their softmax rows on the VALU and need no free slot) in the
    // d_model 64..79 class with 8 heads (kso = 2) and the d_model 32..47 class with 4 heads (kso = 1)
    const bool inst_train = inst_mega || (im->ks1 == 3 && im->dt == 5 && im->kso == 2) || (im->ks1 == 2 && im->dt == 3 && im->kso == 1);
    im->train = im->supported && inst_train && hd <= 8 && D < 16 * im->dt;
    m->bf16 = im;
    if (!im->supported) return FD_OK;
    const int NB = 2 * im->ks1 + im->dt;
    im->ffn_layer_bytes = (size_t)2 * (F / 64) * NB * 1024;
    if (hipMalloc((void**)&im->ffn, im->ffn_layer_bytes * L) != hipSuccess) {
        delete im;
        m->bf16 = nullptr;
        return fd_fail(m->ctx, FD_ERR_HIP, "fd_bf16_create: hipMalloc of the FFN weight images failed");
    }
    if (im->mega || im->train) {          // (the training kernels read the per-layer W_k | W_v | W_q | W_o | FFN images too)
        const size_t KB = 1024;
        im->off_emb = 0;
        im->off_unemb = im->off_emb + (size_t)im->dt * im->kse * KB;
        im->off_layers = im->off_unemb + (size_t)im->ct * im->ks1 * KB;
        im->off_wk = 0;
        im->off_wv = im->off_wk + (size_t)im->np * im->ks1 * KB;
        im->off_wq = im->off_wv + (size_t)im->np * im->ks1 * KB;
        im->off_wo = im->off_wq + (size_t)im->np * im->ks1 * KB;
        im->off_ffn = im->off_wo + (size_t)im->dt * im->kso * KB;
        im->off_lpar = im->off_ffn + im->ffn_layer_bytes;
        im->nlp = (24 * D + 1023) / 1024;
        // pair-form FFN image (32x32x16 H): built for the hydra default width class, the only one with static-shape
        // instantiations of the persistent kernel that use it
        im->off_ffn32 = im->off_lpar + (size_t)im->nlp * KB;
        im->ffn32_layer_bytes = (im->mega && im->ks1 == 3 && im->dt == 5) ? (size_t)2 * (F / 64) * 2 * im->dt * KB : 0;
        im->layer_stride = im->off_ffn32 + im->ffn32_layer_bytes;
        const size_t total = im->off_layers + im->layer_stride * L;
        if (hipMalloc((void**)&im->mimg, total) != hipSuccess || (im->ffn32_layer_bytes && hipMalloc((void**)&im->ffn32_bad, sizeof(int)) != hipSuccess)) {
            fd_bf16_destroy(m);
            return fd_fail(m->ctx, FD_ERR_HIP, "fd_bf16_create: hipMalloc of the persistent-kernel images failed");
        }
    }
    {   // parameter offsets of every layer for the single-launch image build
        std::vector<long long> lofs((size_t)L * 12);
        for (int i = 0; i < L; ++i) {
            const fd_layer_off& lo = m->layers[i];
            const long long v[12] = {lo.in_w, lo.in_b, lo.out_w, lo.out_b, lo.l1_w, lo.l1_b, lo.l2_w, lo.l2_b, lo.n1_w, lo.n1_b, lo.n2_w, lo.n2_b};
            for (int k = 0; k < 12; ++k) lofs[(size_t)i * 12 + k] = v[k];
        }
        if (hipMalloc((void**)&im->layer_off_tab, sizeof(long long) * lofs.size()) != hipSuccess ||
            hipMemcpy(im->layer_off_tab, lofs.data(), sizeof(long long) * lofs.size(), hipMemcpyHostToDevice) != hipSuccess) {
            fd_bf16_destroy(m);
            return fd_fail(m->ctx, FD_ERR_HIP, "fd_bf16_create: upload of the layer offset table failed");
        }
    }
    if (!im->mega || hd > 7) {      // (head_dim 8 beyond the persistent kernel's length limit runs the projection kernels)
        im->nrt_in = (3 * D + 15) / 16;
        im->poff_wo = (size_t)im->nrt_in * im->ks1 * 1024;
        im->p_layer_stride = im->poff_wo + (size_t)im->dt * im->ks1 * 1024;
        if (hipMalloc((void**)&im->pimg, im->p_layer_stride * L) != hipSuccess) {
            fd_bf16_destroy(m);
            return fd_fail(m->ctx, FD_ERR_HIP, "fd_bf16_create: hipMalloc of the projection images failed");
        }
    }
    // bf16 training kernels (fd_train_bf16.hip) exist for the persistent kernel's model family; their transposed-weight
    // images: FFN backward (same block count as the forward image) | W_o^T (dt x ks1) | in_proj^T half-blocks (np x 3 x dt)
    if (im->train) {
        im->boff_ffn = 0;
        im->boff_wot = im->ffn_layer_bytes;
        im->boff_win = im->boff_wot + (size_t)im->dt * im->ks1 * 1024;
        im->b_layer_stride = im->boff_win + (size_t)im->np * 3 * im->dt * 512;
        if (hipMalloc((void**)&im->bimg, im->b_layer_stride * L) != hipSuccess) {
            fd_bf16_destroy(m);
            return fd_fail(m->ctx, FD_ERR_HIP, "fd_bf16_create: hipMalloc of the backward weight images failed");
        }
    }
    return FD_OK;
}

void fd_bf16_destroy(fd_score* m) {
    if (!m->bf16) return;
    if (m->bf16->ffn) (void)hipFree(m->bf16->ffn);
    if (m->bf16->mimg) (void)hipFree(m->bf16->mimg);
    if (m->bf16->ffn32_bad) (void)hipFree(m->bf16->ffn32_bad);
    if (m->bf16->layer_off_tab) (void)hipFree(m->bf16->layer_off_tab);
    if (m->bf16->bimg) (void)hipFree(m->bf16->bimg);
    if (m->bf16->pimg) (void)hipFree(m->bf16->pimg);
    delete m->bf16;
    m->bf16 = nullptr;
}

int fd_bf16_prepare(fd_score* m, hipStream_t s, bool training_only, bool ffn32_only) {
    fd_bf16_images* im = m->bf16;
    if (!im || !im->supported) return FD_OK;
    // Images only the INFERENCE kernels read -- the step-by-step path's FFN image, the persistent kernel's pair-form FFN image, the
    // embedding / unembedding images, the projection images of the other widths -- are skipped by a training step's rebuild
    // (`training_only`: it sits on the step's critical path, in front of the first attention kernel: 53 us of builds on a side stream
    // against 81 us of prologue on the caller's, rocprofv3 time line) and left marked stale; the next inference call then builds just
    // those (`ffn32_only` = inference-only part; the parameters have not changed in between).  The persistent kernel's fp32 layer
    // vectors (n_lp blocks, a few KiB) sit between the training images in the block list and are built by BOTH rebuilds.  Something is
    // skipped only for a model with the persistent-kernel images (B.mega below): without them a training rebuild builds everything.
    im->ffn32_stale = training_only && im->mimg != nullptr;
    const int D = m->d.d_model, F = m->d.dim_ff, H = m->d.n_head, C = m->d.n_channels, hd = D / H, L = m->d.num_layers;
    const int NB = 2 * im->ks1 + im->dt;
    const float* P = m->params;
    fd_img_build B{};
    B.P = P; B.lofs = im->layer_off_tab;
    B.mimg = im->mimg; B.off_layers = im->off_layers; B.layer_stride = im->layer_stride;
    B.off_wk = im->off_wk; B.off_wv = im->off_wv; B.off_wq = im->off_wq; B.off_wo = im->off_wo; B.off_ffn = im->off_ffn;
    B.off_lpar = im->off_lpar; B.n_lp = im->mimg ? im->nlp : 0;
    B.off_ffn32 = im->off_ffn32; B.n_ffn32 = (im->mega && !training_only) ? (int)(im->ffn32_layer_bytes / 1024) : 0;
    B.ffn32_bad = im->ffn32_bad;
    const bool check_ffn32 = FD_RELU_CLAMP && B.n_ffn32 > 0 && im->ffn32_bad && L > 0;
    if (check_ffn32 && hipMemsetAsync(im->ffn32_bad, 0, sizeof(int), s) != hipSuccess)
        return fd_fail(m->ctx, FD_ERR_HIP, "fd_bf16_prepare: reset of the pair-form range counter failed");
    B.ffn = im->ffn; B.ffn_layer_bytes = im->ffn_layer_bytes;
    B.bimg = im->bimg; B.b_layer_stride = im->b_layer_stride; B.boff_ffn = im->boff_ffn; B.boff_wot = im->boff_wot; B.boff_win = im->boff_win;
    B.D = D; B.F = F; B.H = H; B.hd = hd; B.KS1 = im->ks1; B.DT = im->dt; B.KSO = im->kso; B.NP = im->np;
    B.n_qkv = im->np * im->ks1; B.n_wo = im->dt * im->kso; B.n_ffn = 2 * (F / 64) * NB; B.n_wot = im->dt * im->ks1; B.n_win = im->np * 3 * im->dt;
    B.mega = im->mimg ? 1 : 0; B.train = (im->train && im->bimg) ? 1 : 0;
    // softmax scale and log2(e) folded into W_q / b_q: the kernels' softmax is exp2(s - max)
    B.qscale = (float)(1.4426950408889634 / std::sqrt((double)hd));
    int per_layer = B.n_ffn;
    if (B.mega) per_layer += 3 * B.n_qkv + B.n_wo + B.n_ffn + B.n_lp + B.n_ffn32;
    if (B.mega && B.train) per_layer += B.n_ffn + B.n_wot + B.n_win;
    if (ffn32_only) {
        // inference-only part: blocks [0, n_ffn) (step-by-step FFN image) and the layer vectors + pair-form image of the persistent kernel
        if (L > 0) hipLaunchKernelGGL(k_build_layer_images, dim3(B.n_ffn, L), dim3(64), 0, s, B);
        if (L > 0 && B.mega && B.n_lp + B.n_ffn32 > 0) {
            fd_img_build B2 = B;
            B2.blk_first = B.n_ffn + 3 * B.n_qkv + B.n_wo + B.n_ffn;
            hipLaunchKernelGGL(k_build_layer_images, dim3(B.n_lp + B.n_ffn32, L), dim3(64), 0, s, B2);
        }
    } else if (training_only && B.mega) {
        B.blk_first = B.n_ffn;                                 // (skips the step-by-step FFN image; n_ffn32 is already 0)
        if (L > 0) hipLaunchKernelGGL(k_build_layer_images, dim3(per_layer - B.n_ffn, L), dim3(64), 0, s, B);
        FD_LAUNCH_CHECK(m->ctx);
        return FD_OK;
    } else
    if (L > 0) hipLaunchKernelGGL(k_build_layer_images, dim3(per_layer, L), dim3(64), 0, s, B);
    if (im->pimg) {
        for (int i = 0; i < L; ++i) {
            const fd_layer_off& lo = m->layers[i];
            char* pl = im->pimg + (size_t)i * im->p_layer_stride;
            hipLaunchKernelGGL(k_build_image, dim3(im->nrt_in * im->ks1), dim3(64), 0, s, IMG_EMB, P + lo.in_w, P + lo.in_b, (__bf16*)pl,
                               im->ks1, 3 * D, D, H, hd, D, 1.f);
            hipLaunchKernelGGL(k_build_image, dim3(im->dt * im->ks1), dim3(64), 0, s, IMG_EMB, P + lo.out_w, P + lo.out_b,
                               (__bf16*)(pl + im->poff_wo), im->ks1, D, D, H, hd, D, 1.f);
        }
    }
    if (im->mimg) {
        hipLaunchKernelGGL(k_build_image, dim3(im->dt * im->kse), dim3(64), 0, s, IMG_EMB, P + m->emb_w, P + m->emb_b,
                           (__bf16*)(im->mimg + im->off_emb), im->kse, D, C, H, hd, D, 1.f);
        hipLaunchKernelGGL(k_build_image, dim3(im->ct * im->ks1), dim3(64), 0, s, IMG_UNEMB, P + m->un_w, P + m->un_b,
                           (__bf16*)(im->mimg + im->off_unemb), im->ks1, C, D, H, hd, D, 1.f);
    }
    FD_LAUNCH_CHECK(m->ctx);
    if (check_ffn32) {      // one read-back per rebuild of the inference images (a training step's rebuild skips the image and this)
        int nbad = 0;
        if (hipMemcpyAsync(&nbad, im->ffn32_bad, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return fd_fail(m->ctx, FD_ERR_HIP, "fd_bf16_prepare: read-back of the pair-form range counter failed");
        im->ffn32_ok = nbad == 0;
    }
    return FD_OK;
}

// ------------------------------------------------------------------ persistent-kernel planning
struct MegaPlan {
    bool ok = false;
    int S = 1, KT = 1, mt = 1, rot = 1, grid = 0, npg = 1, nw = 8;
    size_t lds = 0;
    int lds_temb = 0, lds_afr = 0;
};

// Workgroup shape: nw = 8 waves, one workgroup per CU (<= 160 KiB LDS, <= 16 token tiles).  (nw = 4, two co-resident
// workgroups per CU, was measured slower and is not instantiated; the arithmetic below stays general.)
static MegaPlan plan_mega_nw(const fd_score* m, int B, int nw) {
    MegaPlan pl;
    pl.nw = nw;
    const fd_bf16_images* im = m->bf16;
    if (!im || !im->mega) return pl;
    const int T = m->d.max_len, D = m->d.d_model;
    const int KT = (T + 15) / 16;
    const int MQ = nw / 2, max_tiles = MQ * 4;
    if (KT > max_tiles) return pl;                            // one series must fit the workgroup's token tiles
    const int NB = 2 * im->ks1 + im->dt;
    const int NP = im->np;
    const size_t ring = (size_t)4 * 2 * NB * 1024;                // 4 chunk buffers x 2 F-halves (fd_mega.hip NBUF)
    const size_t half_ring = ring / 2;
    const size_t lds_cap = (size_t)(nw == 8 ? 160 : 80) * 1024;
    const int wg_per_cu = nw == 8 ? 1 : 2;
    const int slots = m->ctx->num_cu * wg_per_cu;
    const int want = std::max(1, (B + slots - 1) / slots);        // series per WG for one round of workgroups
    for (int S = std::min(want, max_tiles / KT); S >= 1; --S) {
        const int NTILE = S * KT, NTOK = NTILE * 16, NJ = (KT + 1) / 2;
        const int mt = (NTILE + MQ - 1) / MQ;
        const size_t xfr = (size_t)NTILE * im->ks1 * 1024;
        const size_t afr = (size_t)NTILE * im->kso * 1024;
        const size_t xch = (size_t)MQ * mt * im->dt * 1024;
        for (int ng = 1; ng <= NP; ++ng) {                        // head-pair groups: fewer pairs -> smaller K/V
            const int npg = (NP + ng - 1) / ng;
            const size_t wkv = (size_t)3 * npg * im->ks1 * 1024 + (size_t)npg * NTOK * 32 + (size_t)npg * S * NJ * 4 * 16 * 16;
            // FFN ring buffer 0 is filled while the out-proj still reads afr: it must fit in front of afr
            const size_t front = std::max(wkv, half_ring);
            const size_t mid = std::max(front + afr, std::max(ring, xch));
            // time embedding + its scratch, the layer's fp32 vectors, max|K| table of the attention group
            // (the layer vectors arrive by DMA: whole KiB blocks at a 16-byte aligned offset -- fd_mega.hip's LDS map)
            const size_t temb = (((size_t)((2 * S * D + 3) & ~3) + (size_t)im->nlp * 256 + (size_t)npg * S * 16) * sizeof(float) + 15) & ~size_t(15);
            const size_t total = xfr + mid + temb;
            if (total > lds_cap) continue;
            pl.ok = true;
            pl.S = S; pl.KT = KT; pl.mt = mt; pl.npg = npg;
            pl.lds = total;
            pl.lds_afr = (int)(xfr + front);
            pl.lds_temb = (int)(xfr + mid);
            pl.grid = (B + S - 1) / S;
            // rotation of the second wave set: minimise the heaviest SIMD (tiles of the two waves sharing it)
            int best = 1 << 30;
            const int tb = NTILE / MQ, tr = NTILE % MQ;
            for (int rot = 1; rot < std::max(2, MQ); ++rot) {
                int worst = 0;
                for (int q = 0; q < MQ; ++q) {
                    const int a = tb + (q < tr), b = tb + (((q + rot) % MQ) < tr);
                    worst = std::max(worst, a + b);
                }
                if (worst < best) { best = worst; pl.rot = rot; }
            }
            return pl;
        }
    }
    return pl;
}

static MegaPlan plan_mega(const fd_score* m, int B) {
    const fd_bf16_images* im = m->bf16;
    if (!im || !im->mega) return MegaPlan{};
    // a class-conditional model's time embedding differs per series; the persistent kernel shares one per step (temb_table): not ok,
    // so that its forward takes the per-layer kernels and every loop runs step by step
    if (m->n_classes > 0 || m->cond_dim > 0) return MegaPlan{};      // (covariates: e(c_b) per series, fd_cov.hip)
    return plan_mega_nw(m, B, 8);
}

static int fill_mega_params(const fd_score* m, const MegaPlan& pl, int B, fd_mega_params& P) {
    fd_bf16_images* im = m->bf16;
    memset(&P, 0, sizeof P);
    P.B = B; P.T = m->d.max_len; P.KT = pl.KT; P.C = m->d.n_channels; P.D = m->d.d_model; P.H = m->d.n_head;
    P.hd = P.D / P.H; P.L = m->d.num_layers; P.F = m->d.dim_ff;
    if (const char* d2 = getenv("FDIFF_MEGA_DBG")) P.dbg = atoi(d2);
    if (const char* dbg = getenv("FDIFF_MEGA_LAYERS")) P.L = std::min(P.L, atoi(dbg));   // debugging aid
    P.S = pl.S; P.NPG = pl.npg; P.KSE = im->kse; P.CT = im->ct; P.rot = pl.rot;
    P.lds_temb = pl.lds_temb; P.lds_afr = pl.lds_afr; P.num_cu = m->ctx->num_cu;
    P.params = m->params;
    P.pos = m->pos; P.tW = m->tW; P.td_w = m->td_w; P.td_b = m->td_b;
    P.img_emb = im->mimg + im->off_emb;
    P.img_unemb = im->mimg + im->off_unemb;
    P.img_layers = im->mimg + im->off_layers;
    P.layer_stride = im->layer_stride;
    P.off_wk = im->off_wk; P.off_wv = im->off_wv; P.off_wq = im->off_wq; P.off_wo = im->off_wo; P.off_ffn = im->off_ffn;
    P.off_lpar = im->off_lpar; P.nlp = im->nlp;
    P.off_ffn32 = (im->ffn32_layer_bytes && im->ffn32_ok) ? im->off_ffn32 : 0;
    return FD_OK;
}

// fd_score_f32.hip kernels reused by the hybrid path
namespace fdf32 {
void time_embed(const float* t, const float* W, const float* Wd, const float* bd, float* temb, int B, int D,
                hipStream_t s);
void embed(const float* x, const float* We, const float* be, const float* pe, const float* temb, float* h, int M,
           int T, int C, int D, hipStream_t s);
void add_layernorm(const float* a, const float* r, const float* gamma, const float* beta, float* y, int M, int D,
                   hipStream_t s);
}  // namespace fdf32

int fd_bf16_refresh(fd_score* m, hipStream_t s, bool training_only) {
    if (!m->bf16_stale && (training_only || !m->bf16 || !m->bf16->ffn32_stale)) return FD_OK;
    const bool ffn32_only = !m->bf16_stale;          // (=> !training_only && ffn32_stale)
    if (int rc = fd_bf16_prepare(m, s, training_only, ffn32_only)) return rc;
    m->bf16_stale = false;
    return FD_OK;
}

// activation buffers of the step-by-step path, carved from the context arena (fd_score_f32_workspace covers them)
struct LayerBufs {
    float *temb, *h0, *h1, *qkv, *att, *tmp;
    __bf16* xrb;          // (M, 32 ks1) bf16 rows of the CURRENT layer input h0 when xrb_ok (k_attention_bf16's ROWS form)
    bool xrb_ok;
};
static LayerBufs carve_layer_bufs(const fd_score* m, int B, fd_ws& ws) {
    const size_t M = (size_t)B * m->d.max_len, D = m->d.d_model;
    LayerBufs lb;
    lb.temb = ws.take<float>((size_t)B * D);
    lb.h0 = ws.take<float>(M * D);
    lb.h1 = ws.take<float>(M * D);
    lb.qkv = ws.take<float>(M * 3 * D);
    // + 8 floats: k_ffn_ln's fused prologue reads a head's 8 (padded) dim slots as two 16-byte loads, i.e. up to 2 floats past the
    // last row's last head when head_dim < 8 (values discarded by the select that follows) -- the slack is part of the contract
    lb.att = ws.take<float>(M * D + 8);
    lb.tmp = ws.take<float>(M * D);
    lb.xrb = m->bf16 ? ws.take<__bf16>(M * 32 * (size_t)m->bf16->ks1) : nullptr;
    lb.xrb_ok = false;
    return lb;
}
static int bf16_layer_stack(fd_score* m, int B, LayerBufs& lb, hipStream_t s);
// FDIFF_ATT_XROWS (default on): k_ffn_ln hands the layer output to the next layer's attention as bf16 rows (bf16_layer_stack)
static bool att_xrows_on() {
    static const bool on = !(getenv("FDIFF_ATT_XROWS") && atoi(getenv("FDIFF_ATT_XROWS")) == 0);
    return on;
}

int fd_score_forward_bf16(fd_score* m, const float* x, const float* t, float* out, int B, hipStream_t s) {
    fd_ctx* ctx = m->ctx;
    if (!m->bf16 || !m->bf16->supported)
        return fd_fail(ctx, FD_ERR_UNSUPPORTED,
                       "bf16 MFMA path supports d_model %% 4 == 0, d_model <= 143, dim_ff %% 128 == 0; use FD_MODE_F32");
    if (int rc = fd_bf16_refresh(m, s)) return rc;
    {
        const MegaPlan pl = plan_mega(m, B);
        if (pl.ok && !getenv("FDIFF_NO_MEGA")) {
            fd_mega_params MP;
            if (int rc = fill_mega_params(m, pl, B, MP)) return rc;
            MP.mode = FD_MEGA_FORWARD;
            MP.nsteps = 1;
            MP.x = const_cast<float*>(x);
            MP.score_out = out;
            MP.tvec = t;
            if (const char* dump = getenv("FDIFF_MEGA_DUMP")) {      // debugging aid: LDS image of workgroup 0
                unsigned* dbuf = nullptr;
                FD_HIP(ctx, hipMalloc((void**)&dbuf, pl.lds));
                MP.dbg_out = dbuf;
                MP.dbg_bytes = (int)pl.lds;
                int rc = fd_mega_launch(ctx, MP, m->bf16->ks1, m->bf16->dt, m->bf16->kso, pl.mt, pl.nw, pl.grid, pl.lds, s);
                FD_HIP(ctx, hipStreamSynchronize(s));
                std::vector<char> hostbuf(pl.lds);
                FD_HIP(ctx, hipMemcpy(hostbuf.data(), dbuf, pl.lds, hipMemcpyDeviceToHost));
                if (FILE* f = fopen(dump, "wb")) {
                    fwrite(hostbuf.data(), 1, pl.lds, f);
                    fclose(f);
                }
                (void)hipFree(dbuf);
                fprintf(stderr, "[fdiff] LDS dump: S=%d KT=%d mt=%d rot=%d npg=%d lds=%zu afr@%d temb@%d\n", pl.S, pl.KT, pl.mt,
                        pl.rot, pl.npg, pl.lds, pl.lds_afr, pl.lds_temb);
                return rc;
            }
            return fd_mega_launch(ctx, MP, m->bf16->ks1, m->bf16->dt, m->bf16->kso, pl.mt, pl.nw, pl.grid, pl.lds, s);
        }
    }
    const int T = m->d.max_len, C = m->d.n_channels, D = m->d.d_model;
    const int M = B * T;
    const float* P = m->params;
    if (int rc = fd_ws_reserve(ctx, fd_score_f32_workspace(m, B, false))) return rc;
    fd_ws ws(ctx);
    LayerBufs lb = carve_layer_bufs(m, B, ws);
    fdf32::time_embed_cls(t, P + m->tW, P + m->td_w, P + m->td_b, lb.temb, B, D, s, fd_cls_eval(m));
    fdf32::embed(x, P + m->emb_w, P + m->emb_b, P + m->pos, lb.temb, lb.h0, M, T, C, D, s);
    if (int rc = bf16_layer_stack(m, B, lb, s)) return rc;
    fdgemm::linear_fwd(lb.h0, P + m->un_w, P + m->un_b, out, M, C, D, false, s);
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

// Attention of the unfused form, from the packed projections qkv (B*T, 3D) to att (B*T, D): the packed bf16 kernel (head_dim <= 7),
// else the wide one (head_dim 8 .. 32), else -- head_dim > 32, K / V^T of a series beyond the LDS, FDIFF_ATTN_F32 -- the exact-f32
// kernel.  One chain for the layer stack below and for fd_attention_forward's kind 0.
static int attention_unfused(fd_ctx* ctx, const float* qkv, float* att, int B, int T, int H, int hd, hipStream_t s) {
    int arc = getenv("FDIFF_ATTN_F32") ? FD_ERR_UNSUPPORTED : fd_attention_bf16(ctx, qkv, att, B, T, H, hd, s);
    if (arc == FD_ERR_UNSUPPORTED && hd > 7 && !getenv("FDIFF_ATTN_F32"))       // head_dim 8 .. 32: one head per contraction
        arc = fd_attention_bf16_wide(ctx, qkv, att, B, T, H, hd, s);
    if (arc == FD_ERR_UNSUPPORTED) {
        fd_attention_f32(qkv, att, nullptr, B, T, H, hd, 0.f, 0, 0, s);
        arc = FD_OK;
    }
    return arc;
}

// The attention kernels on their own (include/fdiff_hip.h): kind 0 = the chain above, 1 = exact f32, 2 = bf16 packed, 3 = bf16 wide.
extern "C" int fd_attention_forward(fd_ctx* ctx, const float* qkv, float* out, int B, int T, int H, int head_dim, int kind, void* stream) {
    if (!ctx) return FD_ERR_ARG;
    FD_REQUIRE(ctx, qkv && out && (const float*)out != qkv, "fd_attention_forward: null or aliased pointer");
    FD_REQUIRE(ctx, B > 0 && T > 0 && H > 0 && head_dim > 0 && head_dim <= 64 && H <= 65535 && B <= 65535,
               "fd_attention_forward: bad shape B=%d T=%d H=%d head_dim=%d (head_dim 1..64, B and H up to 65535)", B, T, H, head_dim);
    FD_REQUIRE(ctx, (long long)B * T * 3 * H * head_dim < 2147483647LL, "fd_attention_forward: too large");
    FD_REQUIRE(ctx, kind >= 0 && kind <= 3, "fd_attention_forward: unknown kind %d", kind);
    hipStream_t s = (hipStream_t)stream;
    int rc = FD_OK;
    if (kind == 0) rc = attention_unfused(ctx, qkv, out, B, T, H, head_dim, s);
    else if (kind == 1) fd_attention_f32(qkv, out, nullptr, B, T, H, head_dim, 0.f, 0, 0, s);
    else if (kind == 2) rc = fd_attention_bf16(ctx, qkv, out, B, T, H, head_dim, s);
    else rc = fd_attention_bf16_wide(ctx, qkv, out, B, T, H, head_dim, s);
    if (rc == FD_ERR_UNSUPPORTED)
        return fd_fail(ctx, rc, "fd_attention_forward: kind %d has no kernel for T=%d head_dim=%d", kind, T, head_dim);
    if (rc != FD_OK) return rc;
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

// the encoder layers of the step-by-step path: lb.h0 = layer input on entry, the last layer's output on return
static int bf16_layer_stack(fd_score* m, int B, LayerBufs& lb, hipStream_t s) {
    fd_ctx* ctx = m->ctx;
    const int T = m->d.max_len, D = m->d.d_model, H = m->d.n_head;
    const int L = m->d.num_layers, hd = D / H;
    const int M = B * T;
    const float* P = m->params;
    float*& h0 = lb.h0;
    float*& h1 = lb.h1;
    float* const qkv = lb.qkv;
    float* const att = lb.att;
    float* const tmp = lb.tmp;
    for (int i = 0; i < L; ++i) {
        const fd_layer_off& lo = m->layers[i];
        const fd_bf16_images* imq = m->bf16;
        int arc = FD_ERR_UNSUPPORTED;
        const bool fuse = imq->mega && imq->kso == 3 && (imq->ks1 == 3 || imq->ks1 == 2) && !getenv("FDIFF_FFN_UNFUSED");
        // attention output handed to k_ffn_ln's fused prologue as bf16 rows (bit-identical results: the prologue rounds the rows
        // to bf16 MFMA operands either way; FDIFF_ATT_F32ROWS=1 keeps the fp32 rows for A/B runs)
        static const bool att_f32rows = getenv("FDIFF_ATT_F32ROWS") != nullptr;
        int att_bf16 = (fuse && !(hd & 1) && !att_f32rows) ? 1 : 0;
        if (imq->mega && hd <= 7 && !getenv("FDIFF_ATTN_F32") && !getenv("FDIFF_ATTN_UNFUSED")) {
            // Q/K/V projections inside the attention kernel (the persistent kernel's per-layer weight images)
            const char* limg = imq->mimg + imq->off_layers + (size_t)i * imq->layer_stride;
            // measurement hook (bench.py --workload long): in-projection + attention of M tokens
            fd_prof_scope scope(ctx, s, "k_attention_bf16 (fused Q/K/V projection + softmax attention, one launch per layer)",
                                (double)M * (6.0 * D * D + 4.0 * T * D));
            arc = fd_attention_bf16(ctx, h0, att, B, T, H, hd, s, limg + imq->off_wk, limg + imq->off_wv, limg + imq->off_wq, imq->ks1, att_bf16,
                                    lb.xrb_ok ? lb.xrb : nullptr);
        }
        if (arc == FD_ERR_UNSUPPORTED) att_bf16 = 0;
        if (arc == FD_ERR_UNSUPPORTED) {
            const bool pbf = imq->pimg && !getenv("FDIFF_PROJ_F32");       // bf16 MFMA projections (fd_linear_bf16.hip)
            int prc = FD_ERR_UNSUPPORTED;
            if (pbf) prc = fd_linear_bf16(ctx, h0, imq->pimg + (size_t)i * imq->p_layer_stride, qkv, M, 3 * D, D, imq->ks1, s);
            if (prc == FD_ERR_UNSUPPORTED) fdgemm::linear_fwd(h0, P + lo.in_w, P + lo.in_b, qkv, M, 3 * D, D, false, s);
            else if (prc != FD_OK) return prc;
            arc = attention_unfused(ctx, qkv, att, B, T, H, hd, s);
        }
        if (arc != FD_OK) return arc;
        const fd_bf16_images* im = m->bf16;
        if (fuse) {
            // out-proj + residual + LN1 + FFN + LN2 in one kernel (it reads its own output location last: out = h1 is
            // a different buffer from the residual input h0)
            fd_prof_scope scope(ctx, s, "k_ffn_ln (out-proj + LN1 + FFN + LN2, one launch per layer)",
                                (double)M * (2.0 * D * D + 4.0 * D * m->d.dim_ff));
            // the layer output also as bf16 rows for the next layer's attention staging (not behind the last layer: its reader is the
            // unembedding; FDIFF_ATT_XROWS=0 keeps the fp32 staging for A/B runs)
            const bool rows_next = att_xrows_on() && lb.xrb && i + 1 < L && imq->mega && hd <= 7;
            if (int rc = run_ffn(m, nullptr, h1, i, M, s, att, h0, att_bf16, rows_next ? lb.xrb : nullptr)) return rc;
            lb.xrb_ok = rows_next;
            std::swap(h0, h1);
        } else {
            int orc = FD_ERR_UNSUPPORTED;
            if (im->pimg && !getenv("FDIFF_PROJ_F32"))
                orc = fd_linear_res_ln_bf16(ctx, att, im->pimg + (size_t)i * im->p_layer_stride + im->poff_wo, h0, P + lo.n1_w, P + lo.n1_b, h1,
                                            M, D, im->ks1, im->dt, s);
            if (orc == FD_ERR_UNSUPPORTED) {
                fdgemm::linear_fwd(att, P + lo.out_w, P + lo.out_b, tmp, M, D, D, false, s);
                fdf32::add_layernorm(h0, tmp, P + lo.n1_w, P + lo.n1_b, h1, M, D, s);
            } else if (orc != FD_OK) {
                return orc;
            }
            if (int rc = run_ffn(m, h1, h0, i, M, s)) return rc;
            lb.xrb_ok = false;
        }
    }
    lb.xrb_ok = false;
    return FD_OK;
}

// ------------------------------------------------------------------ step-by-step sampler, T > 256 (one series no longer fits a workgroup)
// Between the last encoder layer of diffusion step i and the first of step i + 1 the step-by-step loop ran four launches: the
// unembedding GEMM, fd_sde_step, the time embedding and the embedding (45 us of a 1.49 ms step at T = 1024, B = 64, all of them
// walking the same 65 536 token rows).  k_unembed_step_embed is those four as ONE launch with the persistent kernel's arithmetic
// (score_models.py:78-90, sde.py:129-165, 215-246): a wave owns 16 token rows; score^T = W_u h^T by MFMA from the rows' bf16
// fragments, the Euler-Maruyama step on the lane's four channels with the standalone kernel's Philox stream (counter q = the
// normals of elements 4q .. 4q+3 of the flattened (B,T,C) array), x written back, the new x through LDS into the embedding GEMM's
// B fragment, + positional row + the NEXT step's time embedding (every series of a sampler step shares t: one table row, computed
// for all steps before the loop), next step's layer-0 input written.  h == nullptr: embedding only (first step).
struct StepFuseArgs {
    const float* h;        // (M, D) last layer's output, or null
    float* x;              // (B, T, C) state, updated in place
    float* hn;             // (M, D) next step's layer-0 input, or null (last step)
    __bf16* hn_rows;       // the same as bf16 rows (M, 32 KS1) for k_attention_bf16's ROWS form, or null
    const float* G;        // (T) noise scaling
    const float* z;        // (B, T, C) injected noise of this step, or null (Philox)
    const float* pos;      // (max_len, D) positional table
    const float* temb;     // (D) time embedding of the next step's t
    const char* img_unemb;
    const char* img_emb;
    fd_sde_step_coef cf;
    unsigned long long seed, ctr0;
    int M, T, C, D, KSE, CT;
    // probability-flow ODE form (ODE = true): the evaluation's row and the Heun state (B,T,C) (null for Euler)
    fd_ode_step_coef oc;
    float* x0;
    float* v0;
    fd_dpm_coef dc;        // second coefficient pair of a data-prediction stage (FD_ODE_DDIM and above; D_prev in x0)
};
// ODE: the epilogue runs the probability-flow ODE stage of fd_ode.hip instead of the Euler-Maruyama step (no noise)
template <int KS1, int DT, bool ODE = false>
__global__ __launch_bounds__(256) void k_unembed_step_embed(const StepFuseArgs A) {
    constexpr int XS = 41;                                  // floats per token row of the x stash (C <= 40; odd: conflict-free columns)
    __shared__ float xs_all[4][16 * XS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tok = lane & 15, g = lane >> 4;
    float* const xs = xs_all[wave];
    const int m = (blockIdx.x * 4 + wave) * 16 + tok;
    const bool valid = m < A.M;
    const int mc = valid ? m : A.M - 1;
    const int t = mc % A.T;
    const int C = A.C, D = A.D;
    float* const xrow = A.x + (size_t)mc * C;
    auto gfrag = [&](const char* img, int blk) -> bf16x8 {
        return *reinterpret_cast<const bf16x8*>(img + ((size_t)blk * 64 + lane) * 16);
    };
    if (A.h) {
        // ---- the rows' B fragments: k-slots 32 ks + 8 g .. + 7 of token row m (slot D carries 1.0: the bias row of the image)
        bf16x8 hf[KS1];
        const float* hrow = A.h + (size_t)mc * D;
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = 32 * ks + 8 * g + 4 * q;          // D % 4 == 0: a group of four lies inside the row, is the bias group, or beyond
                const float4 w = *reinterpret_cast<const float4*>(hrow + (k < D ? k : D - 4));
                v[4 * q + 0] = k < D ? w.x : (k == D ? 1.0f : 0.f);
                v[4 * q + 1] = k < D ? w.y : 0.f;
                v[4 * q + 2] = k < D ? w.z : 0.f;
                v[4 * q + 3] = k < D ? w.w : 0.f;
            }
            u32x4 pk = {cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7])};
            hf[ks] = __builtin_bit_cast(bf16x8, pk);
        }
        const float Gk = A.G[t];
        const float gk = (ODE ? A.oc.g : A.cf.g) * Gk;
        for (int ct = 0; ct < A.CT; ++ct) {
            f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gfrag(A.img_unemb, ct * KS1 + ks), hf[ks], sc, 0, 0, 0);
            const int c0 = 16 * ct + 4 * g;
            if (c0 < C) {
                const size_t e0 = (size_t)mc * C + c0;
                float o[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (ODE) {
                    // (only valid rows: a padding lane shares row M-1 with a valid one and must not touch its Heun state)
                    if (valid && A.oc.stage >= FD_ODE_DDIM) {
                        // data-prediction stage (DDIM / DPM-Solver++ 2M): D_prev in x0
                        if ((C & 3) == 0) {
                            const float4 xv = *reinterpret_cast<const float4*>(A.x + e0);
                            const float4 r = fd_dpm_stage4(xv, sc[0], sc[1], sc[2], sc[3], gk, A.oc, A.dc, A.x0 + e0);
                            *reinterpret_cast<float4*>(A.x + e0) = r;
                            o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (c0 + r < C) {
                                    o[r] = fd_dpm_stage1(A.x[e0 + r], sc[r], gk, A.oc, A.dc, A.x0 + e0 + r);
                                    A.x[e0 + r] = o[r];
                                }
                            }
                        }
                    } else if (valid && (C & 3) == 0) {
                        const float4 xv = *reinterpret_cast<const float4*>(A.x + e0);
                        const float4 r = fd_ode_stage4(xv, sc[0], sc[1], sc[2], sc[3], gk, A.oc, A.x0 + e0, A.v0 + e0);
                        *reinterpret_cast<float4*>(A.x + e0) = r;
                        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
                    } else if (valid) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (c0 + r < C) {
                                o[r] = fd_ode_stage1(A.x[e0 + r], sc[r], gk, A.oc, A.x0 + e0 + r, A.v0 + e0 + r);
                                A.x[e0 + r] = o[r];
                            }
                        }
                    }
                } else if ((C & 3) == 0) {
                    const float4 xv = *reinterpret_cast<const float4*>(A.x + e0);
                    float z[4];
                    if (A.z) {
                        const float4 zz = *reinterpret_cast<const float4*>(A.z + e0);
                        z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w;
                    } else {
                        fd_randn4(A.ctr0 + (e0 >> 2), A.seed, z);
                    }
                    o[0] = xv.x - (-A.cf.a_x * xv.x - (gk * gk) * sc[0]) * A.cf.dt + A.cf.sqrt_dt * (gk * z[0]);
                    o[1] = xv.y - (-A.cf.a_x * xv.y - (gk * gk) * sc[1]) * A.cf.dt + A.cf.sqrt_dt * (gk * z[1]);
                    o[2] = xv.z - (-A.cf.a_x * xv.z - (gk * gk) * sc[2]) * A.cf.dt + A.cf.sqrt_dt * (gk * z[2]);
                    o[3] = xv.w - (-A.cf.a_x * xv.w - (gk * gk) * sc[3]) * A.cf.dt + A.cf.sqrt_dt * (gk * z[3]);
                    if (valid) *reinterpret_cast<float4*>(A.x + e0) = float4{o[0], o[1], o[2], o[3]};
                } else {
                    float za[4] = {0.f, 0.f, 0.f, 0.f}, zb[4] = {0.f, 0.f, 0.f, 0.f};
                    const int sh = (int)(e0 & 3);
                    if (!A.z) {
                        const unsigned long long q0 = A.ctr0 + (e0 >> 2);
                        fd_randn4(q0, A.seed, za);
                        fd_randn4(q0 + 1, A.seed, zb);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (c0 + r < C) {
                            float z;
                            if (A.z) z = A.z[e0 + r];
                            else z = (sh + r < 4) ? za[(sh + r) & 3] : zb[(sh + r) & 3];
                            const float xv = A.x[e0 + r];
                            o[r] = xv - (-A.cf.a_x * xv - (gk * gk) * sc[r]) * A.cf.dt + A.cf.sqrt_dt * (gk * z);
                            if (valid) A.x[e0 + r] = o[r];
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (c0 + r < C) xs[tok * XS + c0 + r] = o[r];
            }
        }
    } else {
        for (int c = g; c < C; c += 4) xs[tok * XS + c] = xrow[c];
    }
    if (!A.hn) return;
    // the stash was written by other lanes of this wave (LDS operations of a wave execute in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // ---- embedding of the new x (score_models.py:78-84): h = x We^T + be + pe[t] + temb
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < A.KSE; ++ks) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 32 * ks + 8 * g + e;
            v[e] = (k < C) ? xs[tok * XS + k] : (k == C ? 1.0f : 0.f);
        }
        u32x4 pk = {cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7])};
        const bf16x8 xb = __builtin_bit_cast(bf16x8, pk);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gfrag(A.img_emb, dt * A.KSE + ks), xb, acc[dt], 0, 0, 0);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int d0 = 16 * dt + 4 * g;
        if (d0 < D && valid) {
            const float4 pe = *reinterpret_cast<const float4*>(A.pos + (size_t)t * D + d0);
            const float4 te = *reinterpret_cast<const float4*>(A.temb + d0);
            float4 o;
            o.x = acc[dt][0] + (pe.x + te.x);
            o.y = acc[dt][1] + (pe.y + te.y);
            o.z = acc[dt][2] + (pe.z + te.z);
            o.w = acc[dt][3] + (pe.w + te.w);
            *reinterpret_cast<float4*>(A.hn + (size_t)m * D + d0) = o;
            acc[dt] = f32x4{o.x, o.y, o.z, o.w};
        }
    }
    if (A.hn_rows && valid) {
        __bf16* rrow = A.hn_rows + (size_t)m * (32 * KS1);
#pragma unroll
        for (int dt = 0; dt < 2 * KS1; ++dt) {
            const int d0 = 16 * dt + 4 * g;
            u32x2 pk = {0u, 0u};
            if (dt < DT && d0 < D) {
                pk[0] = cvt_pk_bf16(acc[dt < DT ? dt : 0][0], acc[dt < DT ? dt : 0][1]);
                pk[1] = cvt_pk_bf16(acc[dt < DT ? dt : 0][2], acc[dt < DT ? dt : 0][3]);
            } else if (d0 == D) {
                pk[0] = 0x00003F80u;
            }
            *reinterpret_cast<u32x2*>(rrow + d0) = pk;
        }
    }
}

template <bool ODE>
static void launch_step_fuse(const fd_bf16_images* im, const StepFuseArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.M + 63) / 64)), block(256);
    if (im->ks1 == 3 && im->dt == 5) hipLaunchKernelGGL((k_unembed_step_embed<3, 5, ODE>), grid, block, 0, s, a);
    else if (im->ks1 == 2 && im->dt == 4) hipLaunchKernelGGL((k_unembed_step_embed<2, 4, ODE>), grid, block, 0, s, a);
    else if (im->ks1 == 1 && im->dt == 2) hipLaunchKernelGGL((k_unembed_step_embed<1, 2, ODE>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_unembed_step_embed<1, 1, ODE>), grid, block, 0, s, a);
}

// The SDE rows of the two fused forms: fd_sde_coef at every grid point, t kept for the time-embedding table
static std::vector<fd_sde_step_coef> sde_rows(const fd_sde_params& sde, const float* timesteps, int n_steps, float dt) {
    std::vector<fd_sde_step_coef> tab(n_steps);
    for (int i = 0; i < n_steps; ++i) {
        const SdeCoef c = fd_sde_coef(sde, (double)timesteps[i], dt);
        tab[i] = fd_sde_step_coef{c.a_x, c.g, c.dt, c.sqrt_dt, timesteps[i]};
    }
    return tab;
}

// Device tables of the two fused forms, reserved at ctx->ws + base: one row per score evaluation (fd_sde_step_coef, or the
// layout-compatible fd_ode_step_coef: t where the SDE rows keep it, so the time-embedding table is built from either unchanged),
// the time-embedding table (temb = false: not built, its space still reserved), the (B,T,C) state buffers of the ODE solver
// (nstate: 2 for Heun, 1 for DPM-Solver++ 2M, else 0) and, behind them, the data-prediction solvers' second coefficient array.
struct StepTables {
    const fd_sde_step_coef* rows;
    float *temb, *x0, *v0;
    const fd_dpm_coef* dpm;
};
static int ode_state_bufs(int first_stage) {
    return first_stage == FD_ODE_HEUN_PREDICT ? 2 : first_stage == FD_ODE_DPM_FIRST ? 1 : 0;
}
template <class Row>
static int step_tables(fd_ctx* ctx, const fd_score* m, const std::vector<Row>& rows, size_t base, size_t n, int nstate, bool temb,
                       hipStream_t s, StepTables* o, const std::vector<fd_dpm_coef>* dpm = nullptr) {
    static_assert(sizeof(Row) == sizeof(fd_sde_step_coef), "rows share the layout of fd_sde_step_coef");
    const size_t ne = rows.size();
    const size_t tab_bytes = fd_ws::padded(sizeof(Row) * ne);
    const size_t temb_bytes = fd_ws::padded(sizeof(float) * ne * m->d.d_model);
    const size_t buf = fd_ws::padded(n * sizeof(float));
    const size_t dpm_bytes = dpm ? fd_ws::padded(sizeof(fd_dpm_coef) * ne) : 0;
    if (int rc = fd_ws_reserve(ctx, base + tab_bytes + temb_bytes + nstate * buf + dpm_bytes)) return rc;
    char* p = (char*)ctx->ws + base;
    o->rows = reinterpret_cast<const fd_sde_step_coef*>(p);
    o->temb = temb ? reinterpret_cast<float*>(p + tab_bytes) : nullptr;
    o->x0 = nstate > 0 ? reinterpret_cast<float*>(p + tab_bytes + temb_bytes) : nullptr;
    o->v0 = nstate > 1 ? reinterpret_cast<float*>(p + tab_bytes + temb_bytes + buf) : nullptr;
    o->dpm = dpm ? reinterpret_cast<const fd_dpm_coef*>(p + tab_bytes + temb_bytes + nstate * buf) : nullptr;
    // pageable source: the runtime stages the copy before returning, so `rows` may go out of scope
    FD_HIP(ctx, hipMemcpyAsync(p, rows.data(), sizeof(Row) * ne, hipMemcpyHostToDevice, s));
    if (dpm) FD_HIP(ctx, hipMemcpyAsync((void*)o->dpm, dpm->data(), sizeof(fd_dpm_coef) * ne, hipMemcpyHostToDevice, s));
    if (temb) {
        fd_mega_params MP;
        memset(&MP, 0, sizeof MP);
        MP.params = m->params; MP.tW = m->tW; MP.td_w = m->td_w; MP.td_b = m->td_b; MP.D = m->d.d_model;
        MP.steps = o->rows; MP.nsteps = (int)ne;
        fd_mega_temb_table(MP, o->temb, s);
    }
    return FD_OK;
}

// The layer form of both loops, for the persistent kernel's model family when the persistent kernel itself does not fit (T > 256):
// per score evaluation the 2 L layer launches + ONE launch for unembed / SDE step or ODE stage / next embedding.  Returns
// FD_ERR_UNSUPPORTED (x untouched) when this model has no such path.  ODE: rows are fd_ode_step_coef, no noise is read.
template <bool ODE, class Row>
static int run_layers(fd_score* m, const std::vector<Row>& rows, const float* G, float* x, const float* z_steps, uint64_t seed,
                      uint64_t offset, int B, hipStream_t s, const std::vector<fd_dpm_coef>* dpm = nullptr) {
    fd_ctx* ctx = m->ctx;
    const fd_bf16_images* im = m->bf16;
    if (!im || !im->supported || !im->mega || getenv("FDIFF_SAMPLER_UNFUSED_STEP")) return FD_ERR_UNSUPPORTED;
    if (m->n_classes > 0 || m->cond_dim > 0) return FD_ERR_UNSUPPORTED;      // (k_unembed_step_embed shares one time embedding per step, as the persistent kernel)
    const bool k35 = im->ks1 == 3 && im->dt == 5, k24 = im->ks1 == 2 && im->dt == 4, k12 = im->ks1 == 1 && im->dt == 2,
               k11 = im->ks1 == 1 && im->dt == 1;
    if (!(k35 || k24 || k12 || k11) || m->d.n_channels > 40 || m->d.d_model % 4 != 0) return FD_ERR_UNSUPPORTED;
    if (int rc = fd_bf16_refresh(m, s)) return rc;
    const int T = m->d.max_len, C = m->d.n_channels, D = m->d.d_model;
    const int M = B * T;
    const int ne = (int)rows.size();
    const size_t n = (size_t)M * C;
    int nstate = 0;
    if constexpr (ODE) nstate = ode_state_bufs(rows[0].stage);
    StepTables tb;
    if (int rc = step_tables(ctx, m, rows, fd_score_f32_workspace(m, B, false), n, nstate, true, s, &tb)) return rc;
    fd_ws ws(ctx);
    LayerBufs lb = carve_layer_bufs(m, B, ws);
    StepFuseArgs A{};
    A.x = x; A.G = G; A.pos = m->params + m->pos;
    A.img_unemb = im->mimg + im->off_unemb; A.img_emb = im->mimg + im->off_emb;
    A.seed = seed; A.M = M; A.T = T; A.C = C; A.D = D; A.KSE = im->kse; A.CT = im->ct;
    A.x0 = tb.x0; A.v0 = tb.v0;
    const unsigned long long per_step = (unsigned long long)((n + 3) / 4);
    // the layer stack's fused attention + k_ffn_ln path: its first attention reads the rows
    const bool rows0 = att_xrows_on() && lb.xrb && m->d.num_layers > 0 && m->d.d_model / m->d.n_head <= 7 &&
                       (im->ks1 == 3 || im->ks1 == 2) && im->kso == 3;
    A.h = nullptr; A.hn = lb.h0; A.hn_rows = rows0 ? lb.xrb : nullptr; A.temb = tb.temb;
    launch_step_fuse<ODE>(im, A, s);      // first evaluation's embedding
    lb.xrb_ok = rows0;
    for (int k = 0; k < ne; ++k) {
        if (int rc = bf16_layer_stack(m, B, lb, s)) return rc;
        A.h = lb.h0;
        A.hn = (k + 1 < ne) ? lb.h1 : nullptr;
        A.hn_rows = (rows0 && k + 1 < ne) ? lb.xrb : nullptr;
        A.temb = tb.temb + (size_t)(k + 1 < ne ? k + 1 : k) * D;
        if constexpr (ODE) {
            A.oc = rows[k];
            if (dpm) A.dc = (*dpm)[k];
        } else {
            A.cf = rows[k];
            A.z = z_steps ? z_steps + (size_t)k * n : nullptr;
            A.ctr0 = offset + (unsigned long long)k * per_step;
        }
        launch_step_fuse<ODE>(im, A, s);
        lb.xrb_ok = rows0 && k + 1 < ne;
        std::swap(lb.h0, lb.h1);
    }
    FD_LAUNCH_CHECK(ctx);
    return FD_OK;
}

int fd_sampler_run_layers(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps, float dt,
                          float* x, const float* z_steps, uint64_t seed, uint64_t offset, int B, hipStream_t s) {
    return run_layers<false>(m, sde_rows(*sde, timesteps, n_steps, dt), G, x, z_steps, seed, offset, B, s);
}

int fd_sampler_run_ode_layers(fd_score* m, const std::vector<fd_ode_step_coef>& rows, const float* G, float* x, int B, hipStream_t s,
                              const std::vector<fd_dpm_coef>* dpm) {
    return run_layers<true>(m, rows, G, x, nullptr, 0, 0, B, s, dpm);
}

// FDIFF_MEGA_PROF (profiling aid, reverse-SDE loop): the launch with the kernel's per-phase cycle record of workgroup 0 / wave 0,
// printed to stderr
static int mega_launch_prof(fd_score* m, const MegaPlan& pl, fd_mega_params& MP, hipStream_t s) {
    fd_ctx* ctx = m->ctx;
    const size_t nent = 8300;
    unsigned long long* pb = nullptr;
    FD_HIP(ctx, hipMalloc((void**)&pb, nent * 16));
    FD_HIP(ctx, hipMemsetAsync(pb, 0xff, nent * 16, s));
    MP.prof = pb;
    int rc = fd_mega_launch(ctx, MP, m->bf16->ks1, m->bf16->dt, m->bf16->kso, pl.mt, pl.nw, pl.grid, pl.lds, s);
    FD_HIP(ctx, hipStreamSynchronize(s));
    std::vector<unsigned long long> hb(nent * 2);
    FD_HIP(ctx, hipMemcpy(hb.data(), pb, nent * 16, hipMemcpyDeviceToHost));
    (void)hipFree(pb);
    static const char* names[] = {"step begin->", "time-embed+embed", "QKV weight DMA wait", "K/V projection", "att: last epilogue + barrier",
                                  "out-proj + LN1", "FFN loop", "FFN combine + LN2", "unembed + SDE",
                                  " att: prev epilogue/loop", " att: Q proj + frag loads", " att: pass 1 (max)", " att: softmax stats", " att: pass 2 + PV"};
    double acc[14] = {0};
    unsigned long long prev = 0, first = 0, last = 0;
    size_t n = 0;
    for (; n < 4000 && hb[2 * n] != ~0ull; ++n) {
        const int ph = (int)hb[2 * n];
        const unsigned long long tm = hb[2 * n + 1];
        if (n == 0) first = tm;
        else if (ph >= 1 && ph <= 13) acc[ph] += (double)(tm - prev);   // (ph == 0 intervals = unprofiled steps)
        prev = tm;
        last = tm;
    }
    for (size_t i = 4000; i < 4032 && i < nent; ++i)
        if (hb[2 * i] != ~0ull)
            fprintf(stderr, "[fdiff prof]   unit loop, group %zu wave %zu: %llu cycles\n", (i - 4000) / 8, (i - 4000) % 8, hb[2 * i + 1]);
    {   // residency of every workgroup: start / end (100 MHz wall clock), XCC and CU it ran on
        unsigned long long t0 = ~0ull, t1 = 0;
        const int ng = std::min(pl.grid, 2048);
        for (int i = 0; i < ng; ++i) { t0 = std::min(t0, hb[2 * (4100 + i)]); t1 = std::max(t1, hb[2 * (4100 + i) + 1]); }
        int late = 0;
        std::map<unsigned long long, int> per_cu;
        for (int i = 0; i < ng; ++i) {
            const unsigned long long st = hb[2 * (4100 + i)] - t0;
            if (st > (t1 - t0) / 10) ++late;
            const unsigned long long id = hb[2 * (4100 + 2048 + i)];
            const unsigned hw = (unsigned)id, xcc = (unsigned)(id >> 32) & 0xf;
            // HW_ID: [3:0] wave, [5:4] simd, [7:6] pipe, [11:8] cu, [12] sh, [15:13] se
            const unsigned long long key = ((unsigned long long)xcc << 16) | (((hw >> 13) & 7) << 8) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15);
            per_cu[key]++;
        }
        std::vector<double> dur;
        for (int i = 0; i < ng; ++i) dur.push_back((hb[2 * (4100 + i) + 1] - hb[2 * (4100 + i)]) / 1e5);
        std::vector<double> sd = dur;
        std::sort(sd.begin(), sd.end());
        fprintf(stderr, "[fdiff prof] workgroup durations (ms): wg0 %.3f min %.3f p10 %.3f median %.3f p90 %.3f max %.3f\n", dur[0],
                sd.front(), sd[sd.size() / 10], sd[sd.size() / 2], sd[sd.size() * 9 / 10], sd.back());
        int hist[8] = {0};
        for (auto& kv : per_cu) hist[std::min(7, kv.second)]++;
        fprintf(stderr, "[fdiff prof] %d workgroups, launch span %.3f ms, %d started after 10%% of the span; distinct CUs %zu, "
                "workgroups per CU histogram 1:%d 2:%d 3:%d 4+:%d\n", ng, (t1 - t0) / 1e5, late, per_cu.size(), hist[1], hist[2], hist[3],
                hist[4] + hist[5] + hist[6] + hist[7]);
    }
    {   // duration of every step (workgroup 0): shows drift / clock changes after the profiled first steps
        unsigned long long pt = 0;
        int k = 0;
        for (size_t i = 0; i < n; ++i)
            if (hb[2 * i] == 0) {
                if (pt && (k % 8 == 0)) fprintf(stderr, "[fdiff prof]   step %d: %llu cycles\n", k, hb[2 * i + 1] - pt);
                pt = hb[2 * i + 1];
                ++k;
            }
    }
    int steps_seen = 0;
    for (size_t i = 0; i < n; ++i) steps_seen += (hb[2 * i] == 0);
    fprintf(stderr, "[fdiff prof] nw=%d S=%d npg=%d mt=%d rot=%d lds=%zu: %d steps, %.0f cycles/step\n", pl.nw, pl.S, pl.npg, pl.mt, pl.rot,
            pl.lds, steps_seen, (double)(last - first) / std::max(1, steps_seen));
    const int steps_prof = std::max(1, std::min(4, steps_seen));      // phases are recorded for the first 4 steps
    double acc_all = 0;
    for (int ph = 1; ph <= 13; ++ph) acc_all += acc[ph];
    for (int ph = 1; ph <= 13; ++ph)
        fprintf(stderr, "[fdiff prof]   %-22s %10.0f cycles/step  %5.1f%%\n", names[ph], acc[ph] / steps_prof,
                100.0 * acc[ph] / std::max(1.0, acc_all));
    return rc;
}

// The persistent kernel's share of both loop modes: plan, weight images, device tables at the arena base, launch parameters.
// FD_ERR_UNSUPPORTED (x untouched) when the shape does not fit, so that the caller can fall back to another loop form.
template <class Row>
static int mega_prepare(fd_score* m, const std::vector<Row>& rows, int nstate, bool temb, const float* G, float* x, int B,
                        hipStream_t s, MegaPlan* pl, fd_mega_params* MP, const std::vector<fd_dpm_coef>* dpm = nullptr) {
    *pl = plan_mega(m, B);
    if (!pl->ok || getenv("FDIFF_NO_MEGA")) return FD_ERR_UNSUPPORTED;
    if (int rc = fd_bf16_refresh(m, s)) return rc;
    const size_t n = (size_t)B * m->d.max_len * m->d.n_channels;
    StepTables tb;
    if (int rc = step_tables(m->ctx, m, rows, 0, n, nstate, temb, s, &tb, dpm)) return rc;
    if (int rc = fill_mega_params(m, *pl, B, *MP)) return rc;
    MP->nsteps = (int)rows.size();
    MP->x = x;
    MP->G = G;
    MP->steps = tb.rows;
    MP->temb_table = tb.temb;
    MP->ode_x0 = tb.x0;
    MP->ode_v0 = tb.v0;
    MP->dpm = tb.dpm;
    MP->n_elem = n;
    return FD_OK;
}

// the launch, timed by fd_prof_scope with its algorithmic flops (per series per forward x B x evaluations)
static int mega_launch(fd_score* m, const MegaPlan& pl, fd_mega_params& MP, int B, const char* label, hipStream_t s) {
    fd_ctx* ctx = m->ctx;
    const double T = m->d.max_len, D = m->d.d_model, F = m->d.dim_ff, C = m->d.n_channels, L = m->d.num_layers;
    const double per_fwd = T * (L * (2 * D * 3 * D + 2 * D * D + 4 * D * F + 4 * T * D) + 4 * C * D) + 2 * D * D;
    fd_prof_scope scope(ctx, s, label, per_fwd * B * MP.nsteps);
    if (ctx->prof_on) {
        if (!ctx->prof_clk) FD_HIP(ctx, hipMalloc((void**)&ctx->prof_clk, 4 * sizeof(unsigned long long)));
        FD_HIP(ctx, hipMemsetAsync(ctx->prof_clk, 0, 4 * sizeof(unsigned long long), s));
        MP.clk_out = ctx->prof_clk;
    }
    return fd_mega_launch(ctx, MP, m->bf16->ks1, m->bf16->dt, m->bf16->kso, pl.mt, pl.nw, pl.grid, pl.lds, s);
}

// Whole reverse-diffusion loop in the persistent kernel; FD_ERR_UNSUPPORTED (x untouched) when the shape does not fit
int fd_sampler_run_mega(fd_score* m, const fd_sde_params* sde, const float* G, const float* timesteps, int n_steps,
                        float dt, float* x, const float* z_steps, uint64_t seed, uint64_t offset, int B,
                        hipStream_t s) {
    MegaPlan pl;
    fd_mega_params MP;
    // (FDIFF_MEGA_NO_TEMB_TABLE: compute the time embedding inside the kernel every step, as in forward mode)
    if (int rc = mega_prepare(m, sde_rows(*sde, timesteps, n_steps, dt), 0, !getenv("FDIFF_MEGA_NO_TEMB_TABLE"), G, x, B, s,
                              &pl, &MP))
        return rc;
    MP.mode = FD_MEGA_SAMPLE;
    MP.z_steps = z_steps;
    MP.seed = seed;
    MP.offset = offset;
    MP.ctr_per_step = (MP.n_elem + 3) / 4;
    if (getenv("FDIFF_MEGA_PROF")) return mega_launch_prof(m, pl, MP, s);
    return mega_launch(m, pl, MP, B, "k_mega (persistent score-net + reverse-SDE loop)", s);
}

// The probability-flow ODE loop of fd_sampler_run_ode (fd_ode.hip) in the persistent kernel: the device table holds one
// fd_ode_step_coef per score evaluation, the solver's state (Heun: two (B,T,C) workspace buffers, DPM-Solver++ 2M: one) behind it,
// then the data-prediction solvers' fd_dpm_coef array (dpm: one per row, or null for Euler / Heun)
int fd_sampler_run_ode_mega(fd_score* m, const std::vector<fd_ode_step_coef>& rows, const float* G, float* x, int B, hipStream_t s,
                            const std::vector<fd_dpm_coef>* dpm) {
    MegaPlan pl;
    fd_mega_params MP;
    if (int rc = mega_prepare(m, rows, ode_state_bufs(rows[0].stage), true, G, x, B, s, &pl, &MP, dpm)) return rc;
    MP.mode = FD_MEGA_ODE;
    return mega_launch(m, pl, MP, B, "k_mega (persistent score-net + probability-flow ODE loop)", s);
}

// Which kernel path serves a batch of B series in `mode` (no launch, no device work).  The parity tests use it to assert
// that the instantiation they mean to exercise -- e.g. the two-series-per-workgroup static kernel the bench times -- is
// the one that ran; environment switches (FDIFF_NO_MEGA, FDIFF_MEGA_GENERIC, FDIFF_SAMPLER_STEPWISE) are honoured exactly as
// the product entry points honour them.
extern "C" int fd_score_plan(fd_score* m, int B, int mode, char* out /* >= 192 bytes */, int* series_per_workgroup) {
    if (!m) return FD_ERR_ARG;
    fd_ctx* ctx = m->ctx;
    FD_REQUIRE(ctx, out && B > 0, "fd_score_plan: null output or B=%d", B);
    if (series_per_workgroup) *series_per_workgroup = 0;
    if (m->backbone != FD_BACKBONE_TRANSFORMER) {
        snprintf(out, 192, "%s backbone: exact-f32 kernels (fd_backbones.hip)", m->backbone == FD_BACKBONE_MLP ? "MLP" : "LSTM");
        return FD_OK;
    }
    if (mode == FD_MODE_F32) {
        char cov[48] = "";
        if (m->cond_dim > 0) snprintf(cov, sizeof cov, "; covariate-conditional (%d)", m->cond_dim);
        snprintf(out, 192, "fp32 parity path (per-op kernels, fd_score_f32.hip)%s%s", m->n_classes > 0 ? "; class-conditional" : "", cov);
        return FD_OK;
    }
    FD_REQUIRE(ctx, mode == FD_MODE_BF16, "fd_score_plan: unknown mode %d", mode);
    if (!m->bf16 || !m->bf16->supported) return fd_fail(ctx, FD_ERR_UNSUPPORTED, "fd_score_plan: bf16 path unsupported for this model");
    const MegaPlan pl = plan_mega(m, B);
    if (pl.ok && !getenv("FDIFF_NO_MEGA")) {
        fd_mega_params MP;
        if (int rc = fill_mega_params(m, pl, B, MP)) return rc;
        if (series_per_workgroup) *series_per_workgroup = pl.S;
        return fd_mega_launch(ctx, MP, m->bf16->ks1, m->bf16->dt, m->bf16->kso, pl.mt, pl.nw, pl.grid, pl.lds, nullptr, out);
    }
    {
        const fd_bf16_images* im = m->bf16;
        const int hd = m->d.d_model / m->d.n_head;
        const bool fuse = im->mega && im->kso == 3 && (im->ks1 == 3 || im->ks1 == 2);
        char cls[48] = "";
        if (m->n_classes > 0) snprintf(cls, sizeof cls, "; class-conditional (%d classes)", m->n_classes);
        if (m->cond_dim > 0) snprintf(cls, sizeof cls, "; covariate-conditional (%d)", m->cond_dim);
        snprintf(out, 192, "per-layer bf16 kernels (k_attention_bf16 + k_ffn_ln): attention %s, k_ffn_ln<%d,%d>%s%s",
                 hd > 32 ? "exact-f32 kernel (head_dim > 32) on bf16-MFMA projections"
                 : hd > 7 ? "bf16 k_attention_wide (one head per contraction) on bf16-MFMA projections"
                        : (im->mega ? "bf16 with fused Q/K/V projections" : "bf16 on bf16-MFMA projections"),
                 im->ks1, im->dt, fuse ? " with fused out-proj + LN1" : "", cls);
    }
    return FD_OK;
}

// The macros of THIS translation unit that fix the layout of the images the persistent kernel reads (fd_mega_params.h); the run-time
// compilation (fd_mega_rtc.hip) passes them on, so that a variant build of the image builder never meets a default-macro kernel.
#define FD_STR2(x) #x
#define FD_STR(x) FD_STR2(x)
const char* fd_bf16_image_layout_defines() {
    return "-DFD_W1_SWAP34=" FD_STR(FD_W1_SWAP34) " -DFD_RELU_CLAMP=" FD_STR(FD_RELU_CLAMP) " -DFD_RELU_CLAMP_SHIFT=" FD_STR(FD_RELU_CLAMP_SHIFT);
}
