// gfx950 (MI355X / CDNA4) kernels for the MobileNetV1 backbone (reference backbone_nets/mobilenetv1_backbone.py:21-140):
// one 3x3 / 2 stem and 13 blocks of depthwise 3x3 + BN + ReLU -> pointwise 1x1 + BN + ReLU, no residuals, no ReLU6.
// Activations are NHWC fp32, act[b][y][x][c]; every pointwise product runs on v_mfma_f32_16x16x4_f32 (exact fp32), with the
// operand roles of pointwise_kernel (backbone_kernels.hip): channels on the A side, pixels on the B side, so an accumulator is a
// float4 of four consecutive output channels of one pixel and the epilogue is lane-local.
//
//   mb1_stem_kernel        conv1 + bn1 + ReLU from uint8 HWC or fp32 CHW crops
//   mb1_block_kernel       one whole block per launch: the depthwise output lives in LDS only (the default schedule from 128 faces on)
//   mb1_depthwise_kernel   } the same block as two launches through HBM (smaller batches; SYNERGY_HIP_FUSION=0: always, the cross-check):
//   mb1_pointwise_kernel   } operands straight from global memory, no LDS -- nothing shared with mb1_block_kernel but the arithmetic
// The pool + heads tail is pool_fc_generic_kernel (resnet_kernels.hip), which takes the pool width as an argument.
#include "syn_internal.h"

namespace syn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = fmaxf(v[t], 0.0f);
    return o;
}

// =====================================================================================
// Stem: 3x3 stride-2 conv 3 -> C0 + BN + ReLU (:57-64, :109-111), C0 = 16 | 32 | 64.  Thread = (output pixel, 4 output channels);
// the 27 x C0 filter sits in LDS.  U8 fuses the HWC read and (x - 127.5) / 128 (synergy3DMM.py:189-192); the zero padding is zero in
// the NORMALISED domain, i.e. a padded tap contributes nothing (it is not pixel value 0, which would be -0.996).
// =====================================================================================
template <bool U8>
__global__ __launch_bounds__(256) void mb1_stem_kernel(const float *__restrict__ img, const uint8_t *__restrict__ img8,
                                                       const float *__restrict__ w, const float *__restrict__ scale,
                                                       const float *__restrict__ shift, float *__restrict__ out, int npix, int C0) {
    __shared__ __attribute__((aligned(16))) float sw[27 * 64];
    for (int i = threadIdx.x; i < 27 * C0; i += 256) sw[i] = w[i];
    __syncthreads();
    const int G = C0 >> 2;                                   // channel quads per pixel: 4 | 8 | 16
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
                    if (U8) v = ((float)img8[((size_t)(b * kImg + iy) * kImg + ix) * 3 + ci] - 127.5f) * 0.0078125f;
                    else    v = img[((size_t)(b * 3 + ci) * kImg + iy) * kImg + ix];
                }
                const f32x4 wv = *(const f32x4 *)&sw[(ci * 9 + ky * 3 + kx) * C0 + 4 * g];
                acc += v * wv;
            }
        }
    }
    const f32x4 sc = *(const f32x4 *)&scale[4 * g];
    const f32x4 sh = *(const f32x4 *)&shift[4 * g];
    *(f32x4 *)&out[(size_t)p * C0 + 4 * g] = relu4(acc * sc + sh);
}

void launch_mb1_stem(const float *img, const uint8_t *img8, const float *w, const float *scale, const float *shift, float *out,
                     int C0, int B, hipStream_t s) {
    const int npix = B * 3600, per_block = 256 / (C0 / 4);
    const int grid = (npix + per_block - 1) / per_block;
    if (img8) mb1_stem_kernel<true><<<grid, 256, 0, s>>>(nullptr, img8, w, scale, shift, out, npix, C0);
    else      mb1_stem_kernel<false><<<grid, 256, 0, s>>>(img, nullptr, w, scale, shift, out, npix, C0);
}

// =====================================================================================
// Fused block: depthwise 3x3 (stride 1 | 2, pad 1) + BN + ReLU -> pointwise 1x1 + BN + ReLU, one launch, one NHWC store.
//
// A workgroup (4 waves) owns kMb1Pix = 64 consecutive output pixels of the flattened B * Hout * Hout index and 64 * NT output
// channels; blockIdx.y walks the channel groups, so the depthwise part of a tile is recomputed N / (64 NT) times (9 FMAs per element
// next to a dot product of 64 NT terms per element).  K = the block's input channels is walked in chunks of KC = min(K, 128):
//   1. all 256 threads compute the depthwise output of the tile's 64 pixels x KC channels, one float4 of channels per pixel, and store
//      it to LDS as the pixel-side operand tile T[pixel][KC + 8].  The row pitch is 8 mod 64 dwords: the float4 fragment reads
//      below (lane (r, g) -> row r, dwords 4g .. 4g + 3) then touch 64 distinct banks in each of ds_read_b128's four lane groups.
//      A tile straddles faces (15^2 = 225 and 4^2 = 16 pixels per face are no multiples of 64): every pixel is decoded to
//      (face, oy, ox) on its own and its taps are bounds-checked against ITS face, so no tap reads a neighbouring face;
//      pixels past the end of the batch store zeros.
//   2. wave w multiplies: A fragments = weight rows of its 16 NT channels straight from global memory (row-major [N][K], float4 per
//      lane per 16 k, as pointwise_kernel reads them), B fragments = float4 reads of T.  Element s of both float4 feeds MFMA step s:
//      hardware k slot g of step s is logical k = k0 + 4g + s on both sides, so the sum is complete.
// The accumulators (4 pixel tiles x NT channel tiles of float4) stay in registers across the chunks.  LDS: 64 x 136 x 4 B = 34 KiB,
// whatever K is (K = 2048 of mobilenet_2 included), so four workgroups fit a CU and one's depthwise stage overlaps another's MFMAs.
// N = 32 (mobilenet_05's first block) leaves waves 2, 3 of an NT = 1 workgroup without channels: they take part in the depthwise
// stage and the barriers and skip the GEMM.
// =====================================================================================
constexpr int kMb1Pix = 64, kMb1Kc = 128, kMb1Pitch = kMb1Kc + 8;

template <int NT>
__global__ __launch_bounds__(256) void mb1_block_kernel(const float *__restrict__ X, const float *__restrict__ Wd,
                                                        const float *__restrict__ d_scale, const float *__restrict__ d_shift,
                                                        const float *__restrict__ Wp, const float *__restrict__ p_scale,
                                                        const float *__restrict__ p_shift, float *__restrict__ Y, int M, int Hin,
                                                        int Hout, int K, int N, int stride) {
    __shared__ __attribute__((aligned(16))) float T[kMb1Pix * kMb1Pitch];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * kMb1Pix;
    const int nb = (blockIdx.y * 4 + wave) * (NT * 16);      // this wave's first output channel
    const bool gemm = nb < N;                                // (wave-uniform)
    const int KC = K < kMb1Kc ? K : kMb1Kc, kq = KC >> 2;    // channel quads per chunk
    const int HW = Hout * Hout;

    const float *wp[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        int n = nb + i * 16 + r16;
        n = n < N ? n : N - 1;                               // clamp rows past N (their stores are masked)
        wp[i] = Wp + (size_t)n * K + 4 * g;
    }
    f32x4 acc[4][NT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int kc = 0; kc < K; kc += KC) {
        if (kc) __syncthreads();                             // the previous chunk's fragments have been read
        // ---- depthwise + BN + ReLU of 64 pixels x KC channels -> T ----
        // kq is a power of two that divides 256: a thread keeps ONE channel quad for the whole chunk (its filter, scale and shift are
        // loaded once) and walks the pixels pr, pr + R, ...; two pixels per trip.  Every tap is loaded from a clamped, always valid
        // address and zeroed afterwards where it lies in the padding, so the 18 loads of a trip are issued back to back.
        {
            const int q = threadIdx.x & (kq - 1), pr = threadIdx.x / kq, R = 256 / kq;
            const int c = kc + 4 * q;
            f32x4 wv[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) wv[t] = *(const f32x4 *)&Wd[t * K + c];
            const f32x4 dsc = *(const f32x4 *)&d_scale[c], dsh = *(const f32x4 *)&d_shift[c];
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            auto dw = [&](int pl) -> f32x4 {
                int m = m0 + pl;
                const bool live = m < M;
                m = live ? m : M - 1;
                const int b = m / HW, r = m - b * HW;
                const int oy = r / Hout, ox = r - oy * Hout;
                const float *xb = X + (size_t)b * Hin * Hin * K + c;
                f32x4 v[9];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int iy = oy * stride - 1 + ky, iyc = iy < 0 ? 0 : (iy >= Hin ? Hin - 1 : iy);
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int ix = ox * stride - 1 + kx, ixc = ix < 0 ? 0 : (ix >= Hin ? Hin - 1 : ix);
                        const f32x4 ld = *(const f32x4 *)&xb[(size_t)(iyc * Hin + ixc) * K];
                        v[ky * 3 + kx] = (iy == iyc && ix == ixc) ? ld : zero;      // a padded tap contributes nothing
                    }
                }
                f32x4 a = zero;
#pragma unroll
                for (int t = 0; t < 9; ++t) a += v[t] * wv[t];
                const f32x4 o = relu4(a * dsc + dsh);
                return live ? o : zero;
            };
            for (int pl = pr; pl < kMb1Pix; pl += 2 * R) {
                const bool two = pl + R < kMb1Pix;           // (false only for KC = 16: one pixel per thread)
                const f32x4 o0 = dw(pl);
                const f32x4 o1 = two ? dw(pl + R) : zero;
                *(f32x4 *)&T[pl * kMb1Pitch + 4 * q] = o0;
                if (two) *(f32x4 *)&T[(pl + R) * kMb1Pitch + 4 * q] = o1;
            }
        }
        __syncthreads();
        // ---- pointwise GEMM over this chunk ----
        if (gemm) {
            f32x4 wf[NT], wn[NT], af[4];
#pragma unroll
            for (int i = 0; i < NT; ++i) wn[i] = *(const f32x4 *)(wp[i] + kc);
            for (int k0 = 0; k0 < KC; k0 += 16) {
#pragma unroll
                for (int i = 0; i < NT; ++i) wf[i] = wn[i];
                if (k0 + 16 < KC) {                          // the next step's weight fragments are in flight during this step's MFMAs
#pragma unroll
                    for (int i = 0; i < NT; ++i) wn[i] = *(const f32x4 *)(wp[i] + kc + k0 + 16);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) af[j] = *(const f32x4 *)&T[(j * 16 + r16) * kMb1Pitch + k0 + 4 * g];
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < NT; ++i)
                            acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i][s], af[j][s], acc[j][i], 0, 0, 0);
            }
        }
    }
    if (!gemm) return;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int n = nb + i * 16 + 4 * g;
        if (n >= N) continue;                                // N % 16 == 0
        const f32x4 sc = *(const f32x4 *)&p_scale[n];
        const f32x4 sh = *(const f32x4 *)&p_shift[n];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + j * 16 + r16;
            if (m >= M) continue;
            *(f32x4 *)&Y[(size_t)m * N + n] = relu4(acc[j][i] * sc + sh);
        }
    }
}

// NT, the channel tiles per wave: a workgroup covers 64 NT channels, so NT = 4 recomputes the depthwise stage least often and reuses
// a pixel fragment most; narrow layers take the widest NT that still gives all four waves channels.  (Measured at B = 32 .. 1024 with
// NT capped at 2 and at 1: the cap costs 10 % at B >= 512, changes nothing at B = 128, and NT = 1 everywhere is 1.5-2x slower.)
int mb1_block_nt(int N) { return N >= 256 ? 4 : (N >= 128 ? 2 : 1); }

void launch_mb1_block(const float *X, const float *Wd, const float *d_scale, const float *d_shift, const float *Wp,
                      const float *p_scale, const float *p_shift, float *Y, int B, int Hin, int Hout, int K, int N, int stride,
                      hipStream_t s) {
    const int M = B * Hout * Hout, NT = mb1_block_nt(N);
    const dim3 grid((M + kMb1Pix - 1) / kMb1Pix, (N + 64 * NT - 1) / (64 * NT));
    if (NT == 4)      mb1_block_kernel<4><<<grid, 256, 0, s>>>(X, Wd, d_scale, d_shift, Wp, p_scale, p_shift, Y, M, Hin, Hout, K, N, stride);
    else if (NT == 2) mb1_block_kernel<2><<<grid, 256, 0, s>>>(X, Wd, d_scale, d_shift, Wp, p_scale, p_shift, Y, M, Hin, Hout, K, N, stride);
    else              mb1_block_kernel<1><<<grid, 256, 0, s>>>(X, Wd, d_scale, d_shift, Wp, p_scale, p_shift, Y, M, Hin, Hout, K, N, stride);
}

// =====================================================================================
// Per-layer schedule (SYNERGY_HIP_FUSION=0): the cross-check of mb1_block_kernel.  The depthwise output goes through HBM and the
// GEMM takes both operands from global memory, so neither the LDS tile nor the per-pixel face decode of the fused kernel is involved.
// =====================================================================================
// Thread = (output pixel, 4 channels): consecutive lanes take consecutive channel quads of one pixel.
__global__ __launch_bounds__(256) void mb1_depthwise_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                            const float *__restrict__ scale, const float *__restrict__ shift,
                                                            float *__restrict__ out, long total, int Hin, int Hout, int C4, int stride) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    long p = idx / C4;
    const int ox = (int)(p % Hout);
    p /= Hout;
    const int oy = (int)(p % Hout);
    const int b = (int)(p / Hout);
    const int C = C4 * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - 1 + ky;
        if (iy < 0 || iy >= Hin) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * stride - 1 + kx;
            if (ix < 0 || ix >= Hin) continue;
            const f32x4 v = *(const f32x4 *)&in[((size_t)(b * Hin + iy) * Hin + ix) * C + 4 * c4];
            const f32x4 wv = *(const f32x4 *)&w[(ky * 3 + kx) * C + 4 * c4];
            acc += v * wv;
        }
    }
    const f32x4 sc = *(const f32x4 *)&scale[4 * c4];
    const f32x4 sh = *(const f32x4 *)&shift[4 * c4];
    *(f32x4 *)&out[(size_t)idx * 4] = relu4(acc * sc + sh);
}

void launch_mb1_depthwise(const float *in, const float *w, const float *scale, const float *shift, float *out, int B, int Hin,
                          int Hout, int C, int stride, hipStream_t s) {
    const long total = (long)B * Hout * Hout * (C / 4);
    mb1_depthwise_kernel<<<(int)((total + 255) / 256), 256, 0, s>>>(in, w, scale, shift, out, total, Hin, Hout, C / 4, stride);
}

// C[m][n] = relu(scale[n] * sum_k A[m][k] W[n][k] + shift[n]); A [M,K], W [N,K], K % 16 == 0, N % 16 == 0.  A wave owns 16 MT
// pixels x 16 channels, the 4 waves of a block stack along M; blockIdx.y = channel tile.
template <int MT>
__global__ __launch_bounds__(256) void mb1_pointwise_kernel(const float *__restrict__ A, const float *__restrict__ W,
                                                            const float *__restrict__ scale, const float *__restrict__ shift,
                                                            float *__restrict__ C, int M, int K, int N) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 4 + wave) * (MT * 16);
    const int n0 = blockIdx.y * 16;
    if (m0 >= M) return;
    const float *wp = W + (size_t)(n0 + r16) * K + 4 * g;
    const float *ap[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        int m = m0 + j * 16 + r16;
        m = m < M ? m : M - 1;                               // clamp tail rows (stores are masked)
        ap[j] = A + (size_t)m * K + 4 * g;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 16) {
        const f32x4 wf = *(const f32x4 *)(wp + k0);
        f32x4 af[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) af[j] = *(const f32x4 *)(ap[j] + k0);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], af[j][s], acc[j], 0, 0, 0);
    }
    const int n = n0 + 4 * g;
    const f32x4 sc = *(const f32x4 *)&scale[n];
    const f32x4 sh = *(const f32x4 *)&shift[n];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const int m = m0 + j * 16 + r16;
        if (m >= M) continue;
        *(f32x4 *)&C[(size_t)m * N + n] = relu4(acc[j] * sc + sh);
    }
}

void launch_mb1_pointwise(const float *A, const float *W, const float *scale, const float *shift, float *C, int M, int K, int N,
                          hipStream_t s) {
    const dim3 grid((M + 255) / 256, N / 16);
    mb1_pointwise_kernel<4><<<grid, 256, 0, s>>>(A, W, scale, shift, C, M, K, N);
}

}  // namespace syn
