// gfx950 (MI355X / CDNA4) kernels for the BasicBlock ResNets, resnet18 and resnet34 (reference backbone_nets/resnet_backbone.py:50-87,
// 282-301).  Activations are NHWC fp32.  Every convolution product runs on v_mfma_f32_16x16x4_f32 (exact fp32) with the operand roles of
// rs_gemm_kernel (resnest_kernels.hip): output channels on the A side, pixels on the B side, so an accumulator is a float4 of four
// consecutive output channels of one pixel and the epilogue is lane-local.  No fp16 piece, no atomic: a result does not depend on
// scheduling, on the batch or on a face's position in it.
//
//   bb_conv3x3_kernel      3x3, pad 1, stride 1 or 2, + BN (+ residual) (+ ReLU), the nine taps straight from global memory: the
//                          per-layer (cross-check) schedule
//   bb_down1x1_kernel      the 1x1 stride-2 downsample + BN of layer2.0 / 3.0 / 4.0 as its own launch (per-layer schedule)
//   bb_conv3x3_lds_kernel  the same convolution with its input -- a band of rows with the halo, or whole faces of the 8^2 / 4^2 maps --
//                          staged ONCE per workgroup in LDS; with DS it also produces the downsample + BN output from the centre-tap
//                          fragments it already holds
// An output element is, in all of them, the same sequence of MFMAs: taps in (ky, kx) order, inside a tap the channels in steps of 16,
// lane (r, g) carrying channels k0 + 4g .. k0 + 4g + 3 on both sides, element s feeding MFMA step s; a padded tap feeds zeros.  The
// downsample sums its C channels ascending in the same steps.  So the two schedules are bit-identical.
// The stem is resnet_stem_kernel, the max pool maxpool3x3s2_kernel and the pool + heads pool_fc_generic_kernel (resnet_kernels.hip).
#include "syn_internal.h"

namespace syn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int bb_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the epilogue of every kernel here: BN (+ residual) (+ ReLU) on four consecutive channels of one pixel
__device__ __forceinline__ void bb_store(f32x4 acc, f32x4 sc, f32x4 sh, const float *__restrict__ res, float *__restrict__ Y, size_t off,
                                         int relu) {
    f32x4 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = __builtin_fmaf(acc[t], sc[t], sh[t]);
    if (res) o += *(const f32x4 *)&res[off];
    if (relu) {
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = fmaxf(o[t], 0.0f);
    }
    *(f32x4 *)&Y[off] = o;
}

// =====================================================================================
// 3x3, pad 1, stride S, one group.  X [B][Hin][Hin][C], W packed [n][tap][C] (tap = ky * 3 + kx), Y [B][Ho][Ho][N]; C % 16 == 0,
// N % 32 == 0.  A wave owns 4 pixel tiles of 16 x 2 channel tiles of 16, the 4 waves of a block stack along the pixels, blockIdx.y =
// channel pair.  A padded tap loads from a clamped address and feeds zeros, so every output has 9 C terms in the same order.  Every
// pixel is decoded to (face, y, x): a tile may straddle faces.
// =====================================================================================
__global__ __launch_bounds__(256) void bb_conv3x3_kernel(const float *__restrict__ X, const float *__restrict__ W,
                                                         const float *__restrict__ scale, const float *__restrict__ shift,
                                                         const float *__restrict__ res, float *__restrict__ Y, int M, int Hin, int Ho,
                                                         int C, int N, int stride, int relu) {
    constexpr int MT = 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 4 + wave) * (MT * 16);
    const int n0 = blockIdx.y * 32;
    if (m0 >= M) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int HWo = Ho * Ho, K = 9 * C;
    const float *wp[2] = {W + (size_t)(n0 + r16) * K, W + (size_t)(n0 + 16 + r16) * K};
    bool tv[MT];
    int pb[MT], py[MT], px[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        tv[j] = m0 + j * 16 < M;                              // (wave-uniform)
        int m = m0 + j * 16 + r16;
        m = m < M ? m : M - 1;
        pb[j] = m / HWo;
        const int p = m - pb[j] * HWo;
        py[j] = p / Ho;
        px[j] = p - py[j] * Ho;
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
            const int iy = py[j] * stride + dy, ix = px[j] * stride + dx, iyc = bb_clamp(iy, Hin - 1), ixc = bb_clamp(ix, Hin - 1);
            ok[j] = iy == iyc && ix == ixc;
            tp[j] = X + ((size_t)(pb[j] * Hin + iyc) * Hin + ixc) * C;
        }
        for (int c0 = 0; c0 < C; c0 += 16) {
            const int c = c0 + 4 * g;
            const f32x4 w0 = *(const f32x4 *)(wp[0] + tap * C + c), w1 = *(const f32x4 *)(wp[1] + tap * C + c);
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
            bb_store(acc[j][i], sc, sh, res, Y, (size_t)m * N + n, relu);
        }
    }
}

void launch_bb_conv3x3(const float *X, const float *W, const float *scale, const float *shift, const float *res, float *Y, int B, int Hin,
                       int Ho, int C, int N, int stride, int relu, hipStream_t s) {
    const int M = B * Ho * Ho;
    bb_conv3x3_kernel<<<dim3((M + 255) / 256, N / 32), 256, 0, s>>>(X, W, scale, shift, res, Y, M, Hin, Ho, C, N, stride, relu);
}

// =====================================================================================
// The downsample of layer2.0 / 3.0 / 4.0: 1x1, stride 2, + BN.  Output pixel (oy, ox) reads input pixel (2 oy, 2 ox); W [N][C].  The
// tiling of bb_conv3x3_kernel with one tap.
// =====================================================================================
__global__ __launch_bounds__(256) void bb_down1x1_kernel(const float *__restrict__ X, const float *__restrict__ W,
                                                         const float *__restrict__ scale, const float *__restrict__ shift,
                                                         float *__restrict__ Y, int M, int Hin, int Ho, int C, int N) {
    constexpr int MT = 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 4 + wave) * (MT * 16);
    const int n0 = blockIdx.y * 32;
    if (m0 >= M) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int HWo = Ho * Ho;
    const float *wp[2] = {W + (size_t)(n0 + r16) * C, W + (size_t)(n0 + 16 + r16) * C};
    bool tv[MT];
    const float *ap[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        tv[j] = m0 + j * 16 < M;                              // (wave-uniform)
        int m = m0 + j * 16 + r16;
        m = m < M ? m : M - 1;
        const int b = m / HWo, p = m - b * HWo, oy = p / Ho, ox = p - oy * Ho;
        ap[j] = X + ((size_t)(b * Hin + 2 * oy) * Hin + 2 * ox) * C;
    }
    f32x4 acc[MT][2];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j][0] = acc[j][1] = zero;
    for (int c0 = 0; c0 < C; c0 += 16) {
        const int c = c0 + 4 * g;
        const f32x4 w0 = *(const f32x4 *)(wp[0] + c), w1 = *(const f32x4 *)(wp[1] + c);
        f32x4 af[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) af[j] = tv[j] ? *(const f32x4 *)(ap[j] + c) : zero;
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
            bb_store(acc[j][i], sc, sh, nullptr, Y, (size_t)m * N + n, 0);
        }
    }
}

void launch_bb_down1x1(const float *X, const float *W, const float *scale, const float *shift, float *Y, int B, int Hin, int Ho, int C,
                       int N, hipStream_t s) {
    const int M = B * Ho * Ho;
    bb_down1x1_kernel<<<dim3((M + 255) / 256, N / 32), 256, 0, s>>>(X, W, scale, shift, Y, M, Hin, Ho, C, N);
}

// =====================================================================================
// The LDS-tiled convolution.  A workgroup owns the channels n_lo .. n_lo + N / gridDim.y - 1 (blockIdx.y = channel range) of
//   bands (FACES = false; blockIdx.x = face * nb + band): output rows oy0 .. oy0 + rows - 1 of ONE face.  It stages input rows
//     S oy0 - 1 .. S (oy0 + rows - 1) + 1, columns -1 .. Hin, all C channels, into T[row][Hin + 2][C + 4]; a position outside the face
//     holds zeros (the padding; never the neighbouring face's pixels), so tap (ky, kx) of pixel (y, x) is T[S y + ky][S x + kx]
//   whole faces (FACES = true; blockIdx.x = group of F faces): the small maps, where a face without its halo fits (8^2 at 256 channels:
//     one face, 4^2 at 512: two).  It stages the faces as they are, T[face][Hin][Hin][C + 4]; a padded tap reads a clamped position of
//     its OWN face and feeds zeros, as bb_conv3x3_kernel does.  (With the halo, 4^2 x 512 channels is 74 KiB a face: one tile of 16
//     pixels per 9.4 MB of weights streamed.)
// Then, after one barrier, wave w takes the work items w, w + 4, ..: an item is up to 4 pixel tiles of 16 x one channel pair (32
// channels).  It walks the nine taps and the channels exactly as bb_conv3x3_kernel does, the pixel fragments read from T, the weights
// streamed from L2; the loads of step k + 1 are issued before the MFMAs of step k, and an item has 2 x its tiles independent
// accumulators.
// DS (stride 2 only): the centre tap of pixel (y, x) is input pixel (2 y, 2 x), the operand of the 1x1 stride-2 downsample: the same
// fragments also feed a second set of accumulators with the downsample's weights, k ascending.
// The pitch C + 4 is 4 mod 32 dwords: the float4 fragment reads of consecutive pixels start 4 banks apart (8 at stride 2).
// C is a power of two (64 .. 512).  LDS: at most kBbLdsBytes, so that two workgroups share a CU.
// =====================================================================================
template <int STRIDE, bool DS, bool FACES>
__global__ __launch_bounds__(256) void bb_conv3x3_lds_kernel(const float *__restrict__ X, const float *__restrict__ W,
                                                             const float *__restrict__ scale, const float *__restrict__ shift,
                                                             const float *__restrict__ res, float *__restrict__ Y,
                                                             const float *__restrict__ Wd, const float *__restrict__ dscale,
                                                             const float *__restrict__ dshift, float *__restrict__ Yd, int Hin, int Ho,
                                                             int C, int lgC, int N, int R /* rows per band | faces per workgroup */,
                                                             int nb /* bands per face | faces in the batch */, int relu) {
    extern __shared__ __attribute__((aligned(16))) float T[];
    constexpr int MT = 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int pitch = C + 4, Wp = Hin + 2, C4 = C >> 2, HWi = Hin * Hin, HWo = Ho * Ho;
    int b, oy0 = 0, P;                                         // first (only) face, first output row, output pixels of this workgroup
    if (FACES) {
        b = blockIdx.x * R;
        const int nf = nb - b < R ? nb - b : R;
        P = nf * HWo;
        const float *src = X + (size_t)b * HWi * C;
        for (int idx = threadIdx.x; idx < nf * HWi * C4; idx += 256) {
            const int c = 4 * (idx & (C4 - 1)), pos = idx >> (lgC - 2);
            *(f32x4 *)&T[pos * pitch + c] = *(const f32x4 *)&src[(size_t)pos * C + c];
        }
    } else {
        b = blockIdx.x / nb;
        oy0 = (blockIdx.x - b * nb) * R;
        const int rows = Ho - oy0 < R ? Ho - oy0 : R;
        P = rows * Ho;
        const int iy0 = oy0 * STRIDE - 1, npos = ((rows - 1) * STRIDE + 3) * Wp;
        for (int idx = threadIdx.x; idx < npos * C4; idx += 256) {
            const int c = 4 * (idx & (C4 - 1)), pos = idx >> (lgC - 2);
            const int row = pos / Wp, iy = iy0 + row, ix = pos - row * Wp - 1;
            f32x4 v = zero;
            if (iy >= 0 && iy < Hin && ix >= 0 && ix < Hin) v = *(const f32x4 *)&X[((size_t)(b * Hin + iy) * Hin + ix) * C + c];
            *(f32x4 *)&T[pos * pitch + c] = v;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int tiles = (P + 15) >> 4, groups = (tiles + MT - 1) / MT;
    const int nr = N / gridDim.y, n_lo = blockIdx.y * nr, pairs = nr >> 5;
    const int K = 9 * C;
    for (int item = wave; item < groups * pairs; item += 4) {
        const int grp = item / pairs, n0 = n_lo + 32 * (item - grp * pairs);
        bool tv[MT], ok[MT];
        int pf[MT], py[MT], px[MT], pm[MT], toff[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int t = grp * MT + j, p = t * 16 + r16, pc = p < P ? p : P - 1;      // pixels past the end: a copy of the last one, never stored
            tv[j] = t < tiles;                                                        // (wave-uniform)
            const int f = FACES ? pc / HWo : 0, q = pc - f * HWo, y = q / Ho, x = q - y * Ho;
            pf[j] = f * HWi; py[j] = y * STRIDE; px[j] = x * STRIDE;
            pm[j] = p < P ? (FACES ? b * HWo + p : (b * Ho + oy0 + y) * Ho + x) : -1;
            ok[j] = true;
        }
        // the LDS offset of this lane's fragment of tap (ky, kx), channels 4g ..; FACES: a tap outside the face reads a clamped one, not ok
        auto set_tap = [&](int tap) {
            const int ky = (tap * 11) >> 5, kx = tap - 3 * ky;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                if (FACES) {
                    const int iy = py[j] + ky - 1, ix = px[j] + kx - 1, iyc = bb_clamp(iy, Hin - 1), ixc = bb_clamp(ix, Hin - 1);
                    ok[j] = iy == iyc && ix == ixc;
                    toff[j] = (pf[j] + iyc * Hin + ixc) * pitch + 4 * g;
                } else toff[j] = ((py[j] + ky) * Wp + px[j] + kx) * pitch + 4 * g;
            }
        };
        const float *w0p = W + (size_t)(n0 + r16) * K + 4 * g, *w1p = w0p + (size_t)16 * K;
        f32x4 acc[MT][2], accd[MT][2];
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[j][0] = acc[j][1] = accd[j][0] = accd[j][1] = zero;
        f32x4 w0 = *(const f32x4 *)w0p, w1 = *(const f32x4 *)w1p, af[MT];
        set_tap(0);
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            af[j] = *(const f32x4 *)&T[toff[j]];
            if (FACES) af[j] = ok[j] ? af[j] : zero;
        }
        for (int kk = 0; kk < K; kk += 16) {
            const int kn = kk + 16 < K ? kk + 16 : kk, cn = kn & (C - 1);             // (the last step loads itself again)
            if (cn == 0) set_tap(kn >> lgC);                                          // (wave-uniform) the next step opens a tap
            const f32x4 w0n = *(const f32x4 *)(w0p + kn), w1n = *(const f32x4 *)(w1p + kn);
            f32x4 afn[MT];
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                afn[j] = *(const f32x4 *)&T[toff[j] + cn];
                if (FACES) afn[j] = ok[j] ? afn[j] : zero;
            }
            const bool centre = DS && (kk >> lgC) == 4;                               // (wave-uniform)
            f32x4 d0 = zero, d1 = zero;
            if (centre) {
                const float *dp = Wd + (size_t)(n0 + r16) * C + (kk & (C - 1)) + 4 * g;
                d0 = *(const f32x4 *)dp;
                d1 = *(const f32x4 *)(dp + (size_t)16 * C);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    if (!tv[j]) continue;
                    acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[s], af[j][s], acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[s], af[j][s], acc[j][1], 0, 0, 0);
                }
            if (centre) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int j = 0; j < MT; ++j) {
                        if (!tv[j]) continue;
                        accd[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(d0[s], af[j][s], accd[j][0], 0, 0, 0);
                        accd[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(d1[s], af[j][s], accd[j][1], 0, 0, 0);
                    }
            }
            w0 = w0n;
            w1 = w1n;
#pragma unroll
            for (int j = 0; j < MT; ++j) af[j] = afn[j];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = n0 + 16 * i + 4 * g;
            const f32x4 sc = *(const f32x4 *)&scale[n], sh = *(const f32x4 *)&shift[n];
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                if (!tv[j] || pm[j] < 0) continue;
                bb_store(acc[j][i], sc, sh, res, Y, (size_t)pm[j] * N + n, relu);
            }
            if (DS) {
                const f32x4 dsc = *(const f32x4 *)&dscale[n], dsh = *(const f32x4 *)&dshift[n];
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    if (!tv[j] || pm[j] < 0) continue;
                    bb_store(accd[j][i], dsc, dsh, nullptr, Yd, (size_t)pm[j] * N + n, 0);
                }
            }
        }
    }
}

// The launcher's grid.  `split` channel ranges: the channels are split while the grid has fewer than kBbLdsGroups workgroups and every
// wave still has an item.  Whole faces (q.faces > 0) where the output map is at most 64 pixels (one item's four tiles), an input face
// without its halo fits kBbLdsBytes -- as many faces as fit and as make 64 output pixels -- and that grid has a workgroup for every CU
// (kBbFacesMinGroups).  Else bands: `rows` output rows per band (nb bands per face); among the band heights whose tile with its halo
// fits, the one with the fewest rounds of work items over the face is taken (a round = the four waves of a workgroup busy with one item
// each), ties to the taller band (less halo), the bands then evened out.  A small batch has CUs to spare: the finer bands finish
// sooner there (measured at 1 and 32 faces), the whole faces stream half the weights per pixel.  The result does not depend on any of this.
BbLdsGrid bb_lds_grid(int B, int Hin, int Ho, int C, int N, int stride) {
    auto split = [&](int wgs, int groups) {
        int sp = 1;
        while ((long)wgs * sp < kBbLdsGroups && N % (64 * sp) == 0 && groups * (N / (64 * sp)) >= 4) sp *= 2;
        return sp;
    };
    BbLdsGrid q{};
    const size_t face = (size_t)Hin * Hin * (C + 4) * sizeof(float);
    if (Ho * Ho <= 64 && face <= kBbLdsBytes) {
        q.faces = (int)(kBbLdsBytes / face);
        if (q.faces > 64 / (Ho * Ho)) q.faces = 64 / (Ho * Ho);
        q.lds = q.faces * face;
        q.gridx = (B + q.faces - 1) / q.faces;
        q.split = split(q.gridx, 1);
        if ((long)q.gridx * q.split >= kBbFacesMinGroups) return q;
        q = BbLdsGrid{};
    }
    auto bytes = [&](int r) { return (size_t)((r - 1) * stride + 3) * (Hin + 2) * (C + 4) * sizeof(float); };
    long best = -1;
    for (int r = 1; r <= Ho && bytes(r) <= kBbLdsBytes; ++r) {
        const int nb = (Ho + r - 1) / r, tiles = (r * Ho + 15) / 16, items = ((tiles + 3) / 4) * (N / 32);
        const long cost = (long)nb * ((items + 3) / 4);
        if (best < 0 || cost <= best) { best = cost; q.rows = r; }
    }
    q.nb = (Ho + q.rows - 1) / q.rows;
    q.rows = (Ho + q.nb - 1) / q.nb;
    q.nb = (Ho + q.rows - 1) / q.rows;
    q.lds = bytes(q.rows);
    q.gridx = B * q.nb;
    q.split = split(q.gridx, ((q.rows * Ho + 15) / 16 + 3) / 4);
    return q;
}

template <int STRIDE, bool DS, bool FACES>
static void bb_lds_launch(const BbLdsGrid &q, const float *X, const float *W, const float *scale, const float *shift, const float *res,
                          float *Y, const float *Wd, const float *dscale, const float *dshift, float *Yd, int B, int Hin, int Ho, int C,
                          int lgC, int N, int relu, hipStream_t s) {
    // (more than 64 KiB of dynamic LDS has to be asked for; per device, so on every launch)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&bb_conv3x3_lds_kernel<STRIDE, DS, FACES>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBbLdsBytes);
    bb_conv3x3_lds_kernel<STRIDE, DS, FACES><<<dim3(q.gridx, q.split), 256, q.lds, s>>>(X, W, scale, shift, res, Y, Wd, dscale, dshift, Yd, Hin,
                                                                                      Ho, C, lgC, N, FACES ? q.faces : q.rows,
                                                                                      FACES ? B : q.nb, relu);
}

void launch_bb_conv3x3_lds(const float *X, const float *W, const float *scale, const float *shift, const float *res, float *Y,
                           const float *Wd, const float *dscale, const float *dshift, float *Yd, int B, int Hin, int Ho, int C, int N,
                           int stride, int relu, hipStream_t s) {
    const BbLdsGrid q = bb_lds_grid(B, Hin, Ho, C, N, stride);
    int lgC = 0;
    while ((1 << lgC) < C) ++lgC;
#define SYN_BB_LDS(S, D, F) bb_lds_launch<S, D, F>(q, X, W, scale, shift, res, Y, Wd, dscale, dshift, Yd, B, Hin, Ho, C, lgC, N, relu, s)
    // (every stride-2 convolution of these networks comes with a downsample: there is no <2, false, .>)
    if (stride == 1) { if (q.faces) SYN_BB_LDS(1, false, true); else SYN_BB_LDS(1, false, false); }
    else { if (q.faces) SYN_BB_LDS(2, true, true); else SYN_BB_LDS(2, true, false); }
#undef SYN_BB_LDS
}

}  // namespace syn
