// gfx950 (MI355X / CDNA4) kernels for the ResNeSt-50 backbone (reference backbone_nets/ResNeSt/resnet.py:29-324, splat.py:11-98; radix 2,
// cardinality 1, deep stem, avg_down, avd after the split-attention convolution).  Activations are NHWC fp32.  Every convolution product
// runs on v_mfma_f32_16x16x4_f32 (exact fp32) with the operand roles of gn_pointwise_kernel (ghostnet_kernels.hip): output channels on
// the A side, pixels on the B side, so an accumulator is a float4 of four consecutive output channels of one pixel and the epilogue is
// lane-local.  Means, the gate's two small layers, the softmax and the pools are plain fp32 in a fixed order; there is no fp16 piece and
// no atomic, so a result does not depend on scheduling, on the batch or on a face's position in it.
//
//   rs_stem_kernel      the first stem convolution 3 -> 32, stride 2, from uint8 HWC or fp32 crops, the normalisation inside, BN + ReLU
//   rs_conv3x3_kernel   3x3 / 1, pad 1, `groups` groups in one launch, pitched input slice, BN + ReLU: the stem's second and third
//                       convolution (groups = 1) and conv2.conv of every bottleneck (groups = 2: the two radix branches)
//   rs_gate_kernel      one workgroup per face: mean over the pixels of U[c] + U[C + c], fc1 + BN + ReLU, fc2, softmax over the two radix
//                       halves -> att [B][2C]
//   rs_gemm_kernel      1x1 convolution + BN (+ residual) (+ ReLU) on a tensor in HBM: conv1, the downsample of layer1.0 and of layer4.0,
//                       and every 1x1 of the per-layer schedule
//   rs_tail_kernel      the fused tail: the same GEMM with the pixel operand built once per workgroup into LDS (OP):
//                         kRsCombine  V = att0 U0 + att1 U1                                  (conv3 of a stride-1 block)
//                         kRsAvd      the 3x3 / 2 pad-1 average (divisor 9 everywhere) of V   (conv3 of layer2.0 / 3.0 / 4.0)
//                         kRsDsPool   the 2x2 / 2 ceil-mode average, divisor = samples inside  (the downsample of layer2.0 / 3.0)
//                       V and the pooled tensors never reach HBM there.
//   rs_combine_kernel, rs_avd_kernel, rs_dspool_kernel   the same three operands written to HBM, one launch each: the per-layer
//                       schedule.  They call the device functions the fused loads call, so both schedules feed bit-identical operands
//                       to the same GEMM loop.
// The max pool is maxpool3x3s2_kernel and the pool + heads pool_fc_generic_kernel (resnet_kernels.hip): the same operators, unchanged.
#include "syn_internal.h"

namespace syn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// V = att0 * U0 + att1 * U1, written with an explicit fma so that every caller rounds alike
__device__ __forceinline__ f32x4 rs_combine(f32x4 u0, f32x4 u1, f32x4 a0, f32x4 a1) {
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = __builtin_fmaf(a1[t], u1[t], a0[t] * u0[t]);
    return o;
}

__device__ __forceinline__ int rs_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The 3x3 / 2 pad-1 average of V at output pixel (oy, ox) of face b, channels k .. k + 3: nine terms in (ky, kx) order, a padded tap
// loads from a clamped address and adds zero, the sum times 1 / 9 (count_include_pad).  U [B][H][H][2C], att [B][2C].
__device__ __forceinline__ f32x4 rs_avd_value(const float *__restrict__ U, const float *__restrict__ att, int b, int oy, int ox, int H,
                                              int C, int k) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 a0 = *(const f32x4 *)&att[(size_t)b * 2 * C + k], a1 = *(const f32x4 *)&att[(size_t)b * 2 * C + C + k];
    f32x4 acc = zero;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky, iyc = rs_clamp(iy, H - 1);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx, ixc = rs_clamp(ix, H - 1);
            const float *u = U + ((size_t)(b * H + iyc) * H + ixc) * (2 * C) + k;
            const f32x4 v = rs_combine(*(const f32x4 *)u, *(const f32x4 *)(u + C), a0, a1);
            acc += (iy == iyc && ix == ixc) ? v : zero;
        }
    }
    return acc * (1.0f / 9.0f);
}

// The 2x2 / 2 ceil-mode average without the padding in the divisor (AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False)): at an
// odd H the last row and column hold one sample per axis and divide by 2 (edge) or 1 (corner).  X [B][H][H][C].
__device__ __forceinline__ f32x4 rs_dspool_value(const float *__restrict__ X, int b, int oy, int ox, int H, int C, int k) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc = zero;
    int cnt = 0;
#pragma unroll
    for (int ky = 0; ky < 2; ++ky) {
        const int iy = 2 * oy + ky, iyc = iy < H ? iy : H - 1;
#pragma unroll
        for (int kx = 0; kx < 2; ++kx) {
            const int ix = 2 * ox + kx, ixc = ix < H ? ix : H - 1;
            const bool ok = iy == iyc && ix == ixc;
            const f32x4 v = *(const f32x4 *)&X[((size_t)(b * H + iyc) * H + ixc) * C + k];
            acc += ok ? v : zero;
            cnt += ok ? 1 : 0;
        }
    }
    return acc * (1.0f / (float)cnt);      // 1, 1/2, 1/4: exact
}


// =====================================================================================
// Y[m][n] = act(scale[n] * sum_k A[m][k] W[n][k] + shift[n] (+ res[m][n])).  A rows of pitch lda, W [N][K] row-major; K % 16 == 0,
// N % 32 == 0 (64 .. 2048 here).  A wave owns 4 pixel tiles of 16 x 2 channel tiles of 16, the 4 waves of a block stack along M,
// blockIdx.y = channel pair.  A k step is 16 wide: lane (r, g) carries k0 + 4g .. k0 + 4g + 3 of row r on both sides, element s feeds
// MFMA step s.  Pixel tiles wholly past M are skipped (wave-uniform); the rows past M of the last live tile are clamped and their stores
// masked.
// =====================================================================================
__global__ __launch_bounds__(256) void rs_gemm_kernel(const float *__restrict__ A, int lda, const float *__restrict__ W,
                                                      const float *__restrict__ scale, const float *__restrict__ shift,
                                                      const float *__restrict__ res, float *__restrict__ Y, int M, int K, int N, int relu) {
    constexpr int MT = 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 4 + wave) * (MT * 16);
    const int n0 = blockIdx.y * 32;
    if (m0 >= M) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float *wp[2] = {W + (size_t)(n0 + r16) * K, W + (size_t)(n0 + 16 + r16) * K};
    bool tv[MT];
    const float *ap[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        tv[j] = m0 + j * 16 < M;                              // (wave-uniform)
        int m = m0 + j * 16 + r16;
        m = m < M ? m : M - 1;
        ap[j] = A + (size_t)m * lda;
    }
    f32x4 acc[MT][2];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j][0] = acc[j][1] = zero;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int k = k0 + 4 * g;
        const f32x4 w0 = *(const f32x4 *)(wp[0] + k), w1 = *(const f32x4 *)(wp[1] + k);
        f32x4 af[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) af[j] = tv[j] ? *(const f32x4 *)(ap[j] + k) : zero;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                if (!tv[j]) continue;
                acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[s], af[j][s], acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[s], af[j][s], acc[j][1], 0, 0, 0);
            }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + 16 * i + 4 * g;
        const f32x4 sc = *(const f32x4 *)&scale[n], sh = *(const f32x4 *)&shift[n];
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int m = m0 + j * 16 + r16;
            if (!tv[j] || m >= M) continue;
            f32x4 o;
#pragma unroll
            for (int t = 0; t < 4; ++t) o[t] = __builtin_fmaf(acc[j][i][t], sc[t], sh[t]);
            if (res) o += *(const f32x4 *)&res[(size_t)m * N + n];
            if (relu) {
#pragma unroll
                for (int t = 0; t < 4; ++t) o[t] = fmaxf(o[t], 0.0f);
            }
            *(f32x4 *)&Y[(size_t)m * N + n] = o;
        }
    }
}

// =====================================================================================
// The fused tail: the GEMM of rs_gemm_kernel with the pixel operand built ONCE per workgroup.  A workgroup owns PT = 16 MT consecutive
// output pixels and ALL N output channels:
//   1. thread = (pixel, channel quad) computes the operand (rs_combine / rs_avd_value / rs_dspool_value, the functions the per-layer
//      kernels store with) into the LDS tile T[PT][K + 4]; the tile is never written to HBM
//   2. barrier; wave w walks the channel pairs w, w + 4, ...: the k walk, the fragment roles and the epilogue of rs_gemm_kernel, the
//      pixel fragments read from T -- so every output is the same sum in the same order as in the per-layer schedule.
// Where that gives fewer than kRsTailGroups workgroups, blockIdx.y splits the channels into up to N / 128 ranges (each range stages the
// tile again: a small batch has CUs to spare, not bandwidth to save); an output's sum does not depend on the split.
// PT K = 8192 floats (MT = 4 for K <= 128, 2 for 256, 1 for 512): 33 KiB of LDS, four workgroups per CU.  The pitch K + 4 is 4 mod 32
// dwords: the float4 fragment reads of lane (r, g) -- row r, dwords k0 + 4g .. -- of consecutive rows start 4 banks apart.
// =====================================================================================
template <int OP, int MT>
__global__ __launch_bounds__(256) void rs_tail_kernel(const float *__restrict__ A, const float *__restrict__ att,
                                                      const float *__restrict__ W, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, const float *__restrict__ res,
                                                      float *__restrict__ Y, int M, int K, int N, int Hin, int Ho, int relu) {
    extern __shared__ __attribute__((aligned(16))) float T[];
    constexpr int PT = 16 * MT;
    const int pitch = K + 4, K4 = K >> 2, HWo = Ho * Ho;
    const int m0 = blockIdx.x * PT;
    for (int idx = threadIdx.x; idx < PT * K4; idx += 256) {
        const int row = idx / K4, k = 4 * (idx - row * K4);
        int m = m0 + row;
        m = m < M ? m : M - 1;                               // rows past M: a copy of the last one, never stored
        const int b = m / HWo, p = m - b * HWo, oy = p / Ho, ox = p - oy * Ho;
        f32x4 v;
        if (OP == kRsCombine) {
            const float *u = A + (size_t)m * 2 * K + k, *a = att + (size_t)b * 2 * K + k;
            v = rs_combine(*(const f32x4 *)u, *(const f32x4 *)(u + K), *(const f32x4 *)a, *(const f32x4 *)(a + K));
        } else if (OP == kRsAvd) v = rs_avd_value(A, att, b, oy, ox, Hin, K, k);
        else v = rs_dspool_value(A, b, oy, ox, Hin, K, k);
        *(f32x4 *)&T[row * pitch + k] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    bool tv[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) tv[j] = m0 + j * 16 < M;    // (wave-uniform)
    const int nr = N / gridDim.y, n_lo = blockIdx.y * nr;      // this workgroup's channel range: a multiple of 128 wide
    for (int n0 = n_lo + wave * 32; n0 < n_lo + nr; n0 += 128) {
        const float *w0p = W + (size_t)(n0 + r16) * K, *w1p = W + (size_t)(n0 + 16 + r16) * K;
        f32x4 acc[MT][2];
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[j][0] = acc[j][1] = zero;
        for (int k0 = 0; k0 < K; k0 += 16) {
            const int k = k0 + 4 * g;
            const f32x4 w0 = *(const f32x4 *)(w0p + k), w1 = *(const f32x4 *)(w1p + k);
            f32x4 af[MT];
#pragma unroll
            for (int j = 0; j < MT; ++j) af[j] = tv[j] ? *(const f32x4 *)&T[(j * 16 + r16) * pitch + k] : zero;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    if (!tv[j]) continue;
                    acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[s], af[j][s], acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[s], af[j][s], acc[j][1], 0, 0, 0);
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = n0 + 16 * i + 4 * g;
            const f32x4 sc = *(const f32x4 *)&scale[n], sh = *(const f32x4 *)&shift[n];
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int m = m0 + j * 16 + r16;
                if (!tv[j] || m >= M) continue;
                f32x4 o;
#pragma unroll
                for (int t = 0; t < 4; ++t) o[t] = __builtin_fmaf(acc[j][i][t], sc[t], sh[t]);
                if (res) o += *(const f32x4 *)&res[(size_t)m * N + n];
                if (relu) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) o[t] = fmaxf(o[t], 0.0f);
                }
                *(f32x4 *)&Y[(size_t)m * N + n] = o;
            }
        }
    }
}

template <int OP>
static void launch_rs_tail(const float *A, const float *att, const float *W, const float *scale, const float *shift, const float *res,
                           float *Y, int M, int K, int N, int Hin, int Ho, int relu, hipStream_t s) {
    const int mt = K <= 128 ? 4 : (K == 256 ? 2 : 1), pt = 16 * mt;
    const size_t lds = (size_t)pt * (K + 4) * sizeof(float);
    int split = 1;                                             // channel ranges: until the grid has kRsTailGroups workgroups or a range is 128 wide
    while (((M + pt - 1) / pt) * split < kRsTailGroups && N / (2 * split) >= 128 && N % (256 * split) == 0) split *= 2;
    const dim3 grid((M + pt - 1) / pt, split);
    if (mt == 4) rs_tail_kernel<OP, 4><<<grid, 256, lds, s>>>(A, att, W, scale, shift, res, Y, M, K, N, Hin, Ho, relu);
    else if (mt == 2) rs_tail_kernel<OP, 2><<<grid, 256, lds, s>>>(A, att, W, scale, shift, res, Y, M, K, N, Hin, Ho, relu);
    else rs_tail_kernel<OP, 1><<<grid, 256, lds, s>>>(A, att, W, scale, shift, res, Y, M, K, N, Hin, Ho, relu);
}

void launch_rs_gemm(int op, const float *A, int lda, const float *att, const float *W, const float *scale, const float *shift,
                    const float *res, float *Y, int B, int Hin, int Ho, int K, int N, int relu, hipStream_t s) {
    const int M = B * Ho * Ho;
    if (op == kRsCombine) launch_rs_tail<kRsCombine>(A, att, W, scale, shift, res, Y, M, K, N, Hin, Ho, relu, s);
    else if (op == kRsAvd) launch_rs_tail<kRsAvd>(A, att, W, scale, shift, res, Y, M, K, N, Hin, Ho, relu, s);
    else if (op == kRsDsPool) launch_rs_tail<kRsDsPool>(A, att, W, scale, shift, res, Y, M, K, N, Hin, Ho, relu, s);
    else rs_gemm_kernel<<<dim3((M + 255) / 256, N / 32), 256, 0, s>>>(A, lda, W, scale, shift, res, Y, M, K, N, relu);
}
bool rs_tail_exists(int K, int N) { return K <= 512 && N % 128 == 0; }

// =====================================================================================
// Stem convolution 1: 3x3 / 2, pad 1, 3 -> 32, + BN + ReLU (resnet.py:183-185).  Thread = (output pixel, 4 output channels); the 27 x 32
// filter sits in LDS.  IN = 0: fp32 NCHW crops, already normalised; 1: uint8 HWC crops, (x - 127.5) / 128 applied here; 2: fp32 HWC,
// normalised (the block hook's input).  The padding is zero in the NORMALISED domain: a padded tap contributes nothing.
// =====================================================================================
template <int IN>
__global__ __launch_bounds__(256) void rs_stem_kernel(const float *__restrict__ img, const uint8_t *__restrict__ img8,
                                                      const float *__restrict__ w, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, float *__restrict__ out, int npix) {
    constexpr int C0 = 32, G = C0 / 4;
    __shared__ __attribute__((aligned(16))) float sw[27 * C0];
    for (int i = threadIdx.x; i < 27 * C0; i += 256) sw[i] = w[i];
    __syncthreads();
    const int g = threadIdx.x % G;
    const int p = blockIdx.x * (256 / G) + threadIdx.x / G;
    if (p >= npix) return;
    const int b = p / 3600, r = p - b * 3600;
    const int oy = r / 60, ox = r - oy * 60;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            const bool ok = (iy >= 0) & (iy < kImg) & (ix >= 0) & (ix < kImg);
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                float v = 0.f;
                if (ok) {
                    if (IN == 1) v = ((float)img8[((size_t)(b * kImg + iy) * kImg + ix) * 3 + ci] - 127.5f) * 0.0078125f;
                    else if (IN == 2) v = img[((size_t)(b * kImg + iy) * kImg + ix) * 3 + ci];
                    else v = img[((size_t)(b * 3 + ci) * kImg + iy) * kImg + ix];
                }
                const f32x4 wv = *(const f32x4 *)&sw[(ci * 9 + ky * 3 + kx) * C0 + 4 * g];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_fmaf(v, wv[t], acc[t]);
            }
        }
    }
    const f32x4 sc = *(const f32x4 *)&scale[4 * g], sh = *(const f32x4 *)&shift[4 * g];
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = fmaxf(__builtin_fmaf(acc[t], sc[t], sh[t]), 0.0f);
    *(f32x4 *)&out[(size_t)p * C0 + 4 * g] = o;
}

void launch_rs_stem(const float *img, const uint8_t *img8, int img_hwc, const float *w, const float *scale, const float *shift, float *out,
                    int B, hipStream_t s) {
    const int npix = B * 3600, grid = (npix + 31) / 32;
    if (img8) rs_stem_kernel<1><<<grid, 256, 0, s>>>(nullptr, img8, w, scale, shift, out, npix);
    else if (img_hwc) rs_stem_kernel<2><<<grid, 256, 0, s>>>(img, nullptr, w, scale, shift, out, npix);
    else rs_stem_kernel<0><<<grid, 256, 0, s>>>(img, nullptr, w, scale, shift, out, npix);
}

// =====================================================================================
// 3x3 / 1 convolution, pad 1, `groups` groups, + BN + ReLU.  X [B][H][H] rows of pitch ldx, group q reads channels q Cg .. q Cg + Cg - 1;
// W packed [n][tap][Cg] (tap = ky * 3 + kx); Y [B][H][H][N], group q writes channels q Ng .. (N = groups * Ng).  Cg % 16 == 0, Ng % 32 == 0.
// The GEMM of rs_gemm_kernel with K = 9 Cg walked tap by tap: a padded tap loads from a clamped address and feeds zeros, so every output
// has 9 Cg terms in the same order.  Every pixel is decoded to (face, y, x): a tile may straddle faces.
// =====================================================================================
__global__ __launch_bounds__(256) void rs_conv3x3_kernel(const float *__restrict__ X, int ldx, const float *__restrict__ W,
                                                         const float *__restrict__ scale, const float *__restrict__ shift,
                                                         float *__restrict__ Y, int M, int H, int Cg, int Ng, int N) {
    constexpr int MT = 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 4 + wave) * (MT * 16);
    const int n0 = blockIdx.y * 32;
    if (m0 >= M) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int HW = H * H, grp = n0 / Ng, K = 9 * Cg;
    const float *wp[2] = {W + (size_t)(n0 + r16) * K, W + (size_t)(n0 + 16 + r16) * K};
    const float *xg = X + grp * Cg;
    bool tv[MT];
    int pb[MT], py[MT], px[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        tv[j] = m0 + j * 16 < M;
        int m = m0 + j * 16 + r16;
        m = m < M ? m : M - 1;
        pb[j] = m / HW;
        const int p = m - pb[j] * HW;
        py[j] = p / H;
        px[j] = p - py[j] * H;
    }
    f32x4 acc[MT][2];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j][0] = acc[j][1] = zero;
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        const float *tp[MT];
        bool ok[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int iy = py[j] + dy, ix = px[j] + dx, iyc = rs_clamp(iy, H - 1), ixc = rs_clamp(ix, H - 1);
            ok[j] = iy == iyc && ix == ixc;
            tp[j] = xg + ((size_t)(pb[j] * H + iyc) * H + ixc) * ldx;
        }
        for (int c0 = 0; c0 < Cg; c0 += 16) {
            const int c = c0 + 4 * g;
            const f32x4 w0 = *(const f32x4 *)(wp[0] + tap * Cg + c), w1 = *(const f32x4 *)(wp[1] + tap * Cg + c);
            f32x4 af[MT];
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                af[j] = zero;
                if (!tv[j]) continue;
                const f32x4 v = *(const f32x4 *)(tp[j] + c);
                af[j] = ok[j] ? v : zero;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    if (!tv[j]) continue;
                    acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[s], af[j][s], acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[s], af[j][s], acc[j][1], 0, 0, 0);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + 16 * i + 4 * g;
        const f32x4 sc = *(const f32x4 *)&scale[n], sh = *(const f32x4 *)&shift[n];
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int m = m0 + j * 16 + r16;
            if (!tv[j] || m >= M) continue;
            f32x4 o;
#pragma unroll
            for (int t = 0; t < 4; ++t) o[t] = fmaxf(__builtin_fmaf(acc[j][i][t], sc[t], sh[t]), 0.0f);
            *(f32x4 *)&Y[(size_t)m * N + n] = o;
        }
    }
}

void launch_rs_conv3x3(const float *X, int ldx, const float *W, const float *scale, const float *shift, float *Y, int B, int H, int Cg,
                       int Ng, int groups, hipStream_t s) {
    const int M = B * H * H, N = groups * Ng;
    const dim3 grid((M + 255) / 256, N / 32);
    rs_conv3x3_kernel<<<grid, 256, 0, s>>>(X, ldx, W, scale, shift, Y, M, H, Cg, Ng, N);
}

// =====================================================================================
// The split-attention gate of one face per workgroup (splat.py:55-72).  U [B][HW][2C]; W1t [C][I] and W2t [I][2C] are the two layers
// transposed, so thread j reads consecutive addresses; s1 / h1 = conv2.bn1 folded with fc1's bias; b2 = fc2's bias; att [B][2C].
//   1. thread (slice s, channel quad q) adds U[p][4q ..] + U[p][C + 4q ..] over the pixels p = s, s + S, ... (S = 1024 / C slices);
//      the S partial sums of a channel are added in slice order and multiplied by 1 / HW: a fixed order, no atomics
//   2. hidden[j] = ReLU(s1[j] * sum_k gap[k] W1t[k][j] + h1[j]), k ascending      3. z[n] = sum_k hidden[k] W2t[k][n] + b2[n]
//   4. att[r][c] = softmax over r of z[r C + c]
// C = 64 .. 512, I = 32 .. 256.
// =====================================================================================
__global__ __launch_bounds__(256) void rs_gate_kernel(const float *__restrict__ U, const float *__restrict__ W1t,
                                                      const float *__restrict__ s1, const float *__restrict__ h1,
                                                      const float *__restrict__ W2t, const float *__restrict__ b2,
                                                      float *__restrict__ att, int HW, int C, int I) {
    __shared__ __attribute__((aligned(16))) float part[1024];
    __shared__ float gap[512], hid[256], z[1024];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int C4 = C >> 2, S = 256 / C4, q = tid % C4, sl = tid / C4;
    const float *ub = U + (size_t)b * HW * 2 * C + 4 * q;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    int p = sl;
    for (; p + 3 * S < HW; p += 4 * S) {
        f32x4 v0[4], v1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v0[i] = *(const f32x4 *)&ub[(size_t)(p + i * S) * 2 * C];
            v1[i] = *(const f32x4 *)&ub[(size_t)(p + i * S) * 2 * C + C];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) a += v0[i] + v1[i];
    }
    for (; p < HW; p += S) a += *(const f32x4 *)&ub[(size_t)p * 2 * C] + *(const f32x4 *)&ub[(size_t)p * 2 * C + C];
    *(f32x4 *)&part[sl * C + 4 * q] = a;
    __syncthreads();
    const float inv = 1.0f / (float)HW;
    for (int c = tid; c < C; c += 256) {
        float t = 0.f;
        for (int s = 0; s < S; ++s) t += part[s * C + c];
        gap[c] = t * inv;
    }
    __syncthreads();
    for (int j = tid; j < I; j += 256) {
        float d = 0.f;
        for (int k = 0; k < C; ++k) d = __builtin_fmaf(gap[k], W1t[(size_t)k * I + j], d);
        hid[j] = fmaxf(__builtin_fmaf(d, s1[j], h1[j]), 0.0f);
    }
    __syncthreads();
    for (int n = tid; n < 2 * C; n += 256) {
        float d = 0.f;
        for (int k = 0; k < I; ++k) d = __builtin_fmaf(hid[k], W2t[(size_t)k * 2 * C + n], d);
        z[n] = d + b2[n];
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float z0 = z[c], z1 = z[C + c], m = fmaxf(z0, z1);
        const float e0 = expf(z0 - m), e1 = expf(z1 - m), r = 1.0f / (e0 + e1);
        att[(size_t)b * 2 * C + c] = e0 * r;
        att[(size_t)b * 2 * C + C + c] = e1 * r;
    }
}

void launch_rs_gate(const float *U, const float *W1t, const float *s1, const float *h1, const float *W2t, const float *b2, float *att,
                    int B, int HW, int C, int I, hipStream_t s) {
    rs_gate_kernel<<<B, 256, 0, s>>>(U, W1t, s1, h1, W2t, b2, att, HW, C, I);
}

// ---- the per-layer schedule: the three operands of the fused loads, stored ----
// thread = (output pixel, channel quad)
__global__ __launch_bounds__(256) void rs_combine_kernel(const float *__restrict__ U, const float *__restrict__ att, float *__restrict__ V,
                                                         long total, int HW, int C4) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int k = 4 * (int)(idx % C4), C = 4 * C4;
    const long m = idx / C4;
    const int b = (int)(m / HW);
    const float *u = U + (size_t)m * 2 * C + k, *a = att + (size_t)b * 2 * C + k;
    *(f32x4 *)&V[(size_t)m * C + k] = rs_combine(*(const f32x4 *)u, *(const f32x4 *)(u + C), *(const f32x4 *)a, *(const f32x4 *)(a + C));
}

// V [B][Hin][Hin][C] -> [B][Ho][Ho][C]: rs_avd_value's sum over stored V
__global__ __launch_bounds__(256) void rs_avd_kernel(const float *__restrict__ V, float *__restrict__ out, long total, int Hin, int Ho,
                                                     int C4) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int k = 4 * (int)(idx % C4), C = 4 * C4;
    const long m = idx / C4;
    const int ox = (int)(m % Ho), oy = (int)((m / Ho) % Ho), b = (int)(m / ((long)Ho * Ho));
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc = zero;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky, iyc = rs_clamp(iy, Hin - 1);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx, ixc = rs_clamp(ix, Hin - 1);
            const f32x4 v = *(const f32x4 *)&V[((size_t)(b * Hin + iyc) * Hin + ixc) * C + k];
            acc += (iy == iyc && ix == ixc) ? v : zero;
        }
    }
    *(f32x4 *)&out[(size_t)m * C + k] = acc * (1.0f / 9.0f);
}

__global__ __launch_bounds__(256) void rs_dspool_kernel(const float *__restrict__ X, float *__restrict__ out, long total, int Hin, int Ho,
                                                        int C4) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int k = 4 * (int)(idx % C4), C = 4 * C4;
    const long m = idx / C4;
    const int ox = (int)(m % Ho), oy = (int)((m / Ho) % Ho), b = (int)(m / ((long)Ho * Ho));
    *(f32x4 *)&out[(size_t)m * C + k] = rs_dspool_value(X, b, oy, ox, Hin, C, k);
}

void launch_rs_combine(const float *U, const float *att, float *V, int B, int HW, int C, hipStream_t s) {
    const long total = (long)B * HW * (C / 4);
    rs_combine_kernel<<<(int)((total + 255) / 256), 256, 0, s>>>(U, att, V, total, HW, C / 4);
}
void launch_rs_avd(const float *V, float *out, int B, int Hin, int Ho, int C, hipStream_t s) {
    const long total = (long)B * Ho * Ho * (C / 4);
    rs_avd_kernel<<<(int)((total + 255) / 256), 256, 0, s>>>(V, out, total, Hin, Ho, C / 4);
}
void launch_rs_dspool(const float *X, float *out, int B, int Hin, int Ho, int C, hipStream_t s) {
    const long total = (long)B * Ho * Ho * (C / 4);
    rs_dspool_kernel<<<(int)((total + 255) / 256), 256, 0, s>>>(X, out, total, Hin, Ho, C / 4);
}

}  // namespace syn
