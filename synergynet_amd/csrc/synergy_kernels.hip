// Synergy refinement (reference backbone_nets/pointnet_backbone.py MLP_for / MLP_rev, model_building.py:149-153) for gfx950.
// Every GEMM runs on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32 with the operand roles of pointwise_kernel
// (backbone_kernels.hip):
//   MFMA "A" operand (rows i) = 16 output channels n,  lane l holds W[n0 + (l&15)][k]
//   MFMA "B" operand (cols j) = 16 points / faces m,   lane l holds X[m0 + (l&15)][k]
//   D: lane l owns column j = l&15 (one point) and rows i = 4*(l>>4)+r (4 consecutive channels)
// K is walked 16 at a time: a lane fetches ONE float4 (k0+4g .. k0+4g+3, g = l>>4) per operand row and feeds element s of it to MFMA
// step s, so hardware k-slot g of step s is logical k = k0+4g+s for both operands.  Weights are row-major [N][K] with N and K zero
// padded (syn_load_synergy), BatchNorm folded to scale / shift per output channel (syn_fold_synergy_host).
//
// Four kernels:
//   syn_trunk_kernel       conv1-conv5 + max-pool over a face's 68 points, 4 faces (272 rows = 17 MFMA tiles) per workgroup
//   syn_face_concat_kernel [pool | shape | expr] behind the global feature: the per-face input row of conv6
//   syn_face_gemm_kernel   one row per FACE: the per-face half of conv6 (raw sums), and MLP_rev's 62 x 1024 head (BN + ReLU)
//   syn_point_head_kernel  conv6 (per-point half + the face's sums) - conv7 - conv8 - conv9, Lr = Lc + 0.05 res, optional ROI affine
// Nothing here accumulates across faces or with atomics: a face's result does not depend on the batch it is in.
#include "syn_internal.h"

namespace syn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kGrpFaces = 4;                          // faces per trunk workgroup
constexpr int kGrpRows = kGrpFaces * kSynPts;         // 272 = 17 x 16: no padding rows in a full group
constexpr int kGrpTiles = kGrpRows / 16;
constexpr int kLdT = 132;                             // LDS row stride of the trunk (128 channels + 4: rows 4 banks apart)
static_assert(kGrpRows % 16 == 0, "a full group must be whole MFMA tiles");

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = fmaxf(v[c], 0.f);
    return r;
}

__device__ __forceinline__ f32x4 mfma4(f32x4 w, f32x4 x, f32x4 acc) {
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], x[s], acc, 0, 0, 0);
    return acc;
}

// One 64-input layer of a row tile, in place: `row` = this lane's LDS row (+ 4 g), xf = the row's 64 inputs already in registers.
template <int N>
__device__ __forceinline__ void layer64(const f32x4 (&xf)[4], float *row, const float *__restrict__ W, const float *__restrict__ scale,
                                        const float *__restrict__ shift, int r16, int g, float *pf_row /*nullable: global copy of the output*/) {
#pragma unroll
    for (int i = 0; i < N / 16; ++i) {
        const float *wp = W + (size_t)(16 * i + r16) * 64 + 4 * g;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc = mfma4(*(const f32x4 *)(wp + 16 * kk), xf[kk], acc);
        const f32x4 v = relu4(acc * *(const f32x4 *)&scale[16 * i + 4 * g] + *(const f32x4 *)&shift[16 * i + 4 * g]);
        *(f32x4 *)(row + 16 * i) = v;
        if (pf_row) *(f32x4 *)(pf_row + 16 * i) = v;
    }
}

}  // namespace

// -------------------------------------------------------------------------------------
// Trunk: conv1 (3->64) conv2 (64->64) conv3 (64->64) conv4 (64->128) conv5 (128->1024), each BN + ReLU, then the max over the 68
// points of a face.  512 threads = 8 waves take 4 faces.
//   layers 1-4: a wave owns row tiles wave, wave + 8, wave + 16 and walks them through the four layers IN PLACE in LDS (a tile's
//               inputs are in registers before its outputs are written); MLP_for also stores conv2's output [B*68, 64].
//   conv5:      a wave owns 128 of the 1024 channels, 32 at a time with their weights in registers, and runs all 17 row tiles past
//               them; the [B,1024,68] tensor never exists -- each lane keeps the running max of its rows per face, 16 lanes are
//               combined by shuffles at the end.  Post-ReLU values are >= 0, so rows of another face, and the rows of a ragged
//               last group, enter a face's max as 0 and cannot change it.
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void syn_trunk_kernel(SynTrunkW w, const float *__restrict__ lmk /*[B,3,68]*/, int B,
                                                        float *__restrict__ pf /*nullable [B*68,64]*/, float *__restrict__ gf, int gf_pitch,
                                                        float *__restrict__ gf2 /*nullable [B,1024]*/) {
    __shared__ __attribute__((aligned(16))) float act[kGrpRows * kLdT];
    const int b0 = blockIdx.x * kGrpFaces;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;

    for (int j = tid; j < kGrpRows; j += 512) {            // [x y z 0] per row; rows of faces past the batch are zero
        const int f = j / kSynPts, p = j - f * kSynPts;
        const bool ok = b0 + f < B;
        const float *src = lmk + (size_t)(ok ? b0 + f : B - 1) * 3 * kSynPts + p;
        f32x4 v = {src[0], src[kSynPts], src[2 * kSynPts], 0.f};
        if (!ok) v = (f32x4){0.f, 0.f, 0.f, 0.f};
        *(f32x4 *)&act[j * kLdT] = v;
    }
    __syncthreads();

    for (int it = 0; it < (kGrpTiles + 7) / 8; ++it) {
        const int t = wave + 8 * it;
        const bool live = t < kGrpTiles;                    // wave-uniform; the barriers below stay outside of it
        const int j = 16 * (live ? t : 0) + r16;
        float *row = &act[j * kLdT + 4 * g];
        const int f = j / kSynPts;
        float *pf_row = (pf && live && b0 + f < B) ? pf + ((size_t)b0 * kSynPts + j) * 64 + 4 * g : nullptr;
        // conv1: K = 3 padded to 4, one MFMA step (k slot g)
        float x1 = 0.f;
        if (live) x1 = act[j * kLdT + g];
        __syncthreads();
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.W[0][(16 * i + r16) * 4 + g], x1, acc, 0, 0, 0);
                *(f32x4 *)(row + 16 * i) = relu4(acc * *(const f32x4 *)&w.scale[0][16 * i + 4 * g] + *(const f32x4 *)&w.shift[0][16 * i + 4 * g]);
            }
        }
        __syncthreads();
        f32x4 xf[4] = {};
#pragma unroll
        for (int L = 1; L <= 3; ++L) {
            if (live) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) xf[kk] = *(const f32x4 *)(row + 16 * kk);
            }
            __syncthreads();
            if (live) {
                if (L == 1) layer64<64>(xf, row, w.W[1], w.scale[1], w.shift[1], r16, g, pf_row);
                else if (L == 2) layer64<64>(xf, row, w.W[2], w.scale[2], w.shift[2], r16, g, nullptr);
                else layer64<128>(xf, row, w.W[3], w.scale[3], w.shift[3], r16, g, nullptr);
            }
            __syncthreads();
        }
    }

    // conv5 + max-pool
    for (int pass = 0; pass < 4; ++pass) {
        const int n0 = wave * 128 + pass * 32;
        f32x4 wf[2][8], sc[2], sh[2], mx[2][kGrpFaces];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float *wp = w.W[4] + (size_t)(n0 + 16 * i + r16) * 128 + 4 * g;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) wf[i][kk] = *(const f32x4 *)(wp + 16 * kk);
            sc[i] = *(const f32x4 *)&w.scale[4][n0 + 16 * i + 4 * g];
            sh[i] = *(const f32x4 *)&w.shift[4][n0 + 16 * i + 4 * g];
#pragma unroll
            for (int f = 0; f < kGrpFaces; ++f) mx[i][f] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        for (int t = 0; t < kGrpTiles; ++t) {
            const int j = 16 * t + r16;
            const float *row = &act[j * kLdT + 4 * g];
            f32x4 xf[8];
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) xf[kk] = *(const f32x4 *)(row + 16 * kk);
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i] = mfma4(wf[i][kk], xf[kk], acc[i]);
            const int f = j / kSynPts;
            const bool ok = b0 + f < B;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const f32x4 v = relu4(acc[i] * sc[i] + sh[i]);
#pragma unroll
                for (int ff = 0; ff < kGrpFaces; ++ff) {
                    const bool mine = ok && f == ff;
#pragma unroll
                    for (int c = 0; c < 4; ++c) mx[i][ff][c] = fmaxf(mx[i][ff][c], mine ? v[c] : 0.f);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int ff = 0; ff < kGrpFaces; ++ff) {
                f32x4 m;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float x = mx[i][ff][c];
#pragma unroll
                    for (int d = 1; d < 16; d <<= 1) x = fmaxf(x, __shfl_xor(x, d));
                    m[c] = x;
                }
                if (r16 == 0 && b0 + ff < B) {
                    *(f32x4 *)&gf[(size_t)(b0 + ff) * gf_pitch + n0 + 16 * i + 4 * g] = m;
                    if (gf2) *(f32x4 *)&gf2[(size_t)(b0 + ff) * kSynGlobal + n0 + 16 * i + 4 * g] = m;
                }
            }
    }
}

void launch_syn_trunk(const SynTrunkW &w, const float *lmk, int B, float *pf, float *gf, int gf_pitch, float *gf2, hipStream_t s) {
    syn_trunk_kernel<<<(B + kGrpFaces - 1) / kGrpFaces, 512, 0, s>>>(w, lmk, B, pf, gf, gf_pitch, gf2);
}

// -------------------------------------------------------------------------------------
// X6[b] = [global 1024 (written by the trunk) | pool 1280 | shape 40 | expr 10 | 0 x 14]: columns 1024 .. 2367
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void syn_face_concat_kernel(const float *__restrict__ pool, const float *__restrict__ param, float *__restrict__ X6, int B) {
    const int b = blockIdx.x;
    float *dst = X6 + (size_t)b * kSynFaceKpad + kSynGlobal;
    for (int i = threadIdx.x; i < kSynFaceKpad - kSynGlobal; i += 256) {
        float v = 0.f;
        if (i < kPool) v = pool[(size_t)b * kPool + i];
        else if (i < kPool + 50) v = param[(size_t)b * kParam + 12 + (i - kPool)];      // whitened shape | expression codes
        dst[i] = v;
    }
}

void launch_syn_face_concat(const float *pool, const float *param, float *X6, int B, hipStream_t s) {
    syn_face_concat_kernel<<<B, 256, 0, s>>>(pool, param, X6, B);
}

// -------------------------------------------------------------------------------------
// out[b][n] = epi(sum_k W[n][k] X[b][k]): one wave per (16 faces, 32 channels); W [Npad][Kpad], X rows ldx apart and readable up to
// Kpad; scale == nullptr: raw sums (conv6's per-face half), else relu(scale * sum + shift)
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void syn_face_gemm_kernel(const float *__restrict__ X, int ldx, const float *__restrict__ W, int Kpad,
                                                           const float *__restrict__ scale, const float *__restrict__ shift,
                                                           float *__restrict__ out, int ldo, int N, int B) {
    const int lane = threadIdx.x, r16 = lane & 15, g = lane >> 4;
    const int m = blockIdx.x * 16 + r16, n0 = blockIdx.y * 32;
    const float *xp = X + (size_t)(m < B ? m : B - 1) * ldx + 4 * g;                   // clamp tail rows (stores are masked)
    const float *wp0 = W + (size_t)(n0 + r16) * Kpad + 4 * g, *wp1 = wp0 + (size_t)16 * Kpad;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = 0; k0 < Kpad; k0 += 16) {
        const f32x4 x = *(const f32x4 *)(xp + k0);
        acc0 = mfma4(*(const f32x4 *)(wp0 + k0), x, acc0);
        acc1 = mfma4(*(const f32x4 *)(wp1 + k0), x, acc1);
    }
    if (m >= B) return;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        f32x4 v = i ? acc1 : acc0;
        const int n = n0 + 16 * i + 4 * g;
        if (scale) v = relu4(v * *(const f32x4 *)&scale[n] + *(const f32x4 *)&shift[n]);      // scale / shift are padded like W
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (n + c < N) out[(size_t)m * ldo + n + c] = v[c];
    }
}

void launch_syn_face_gemm(const float *X, int ldx, const float *W, int Kpad, const float *scale, const float *shift, float *out, int ldo,
                          int N, int B, hipStream_t s) {
    syn_face_gemm_kernel<<<dim3((B + 15) / 16, (N + 31) / 32), 64, 0, s>>>(X, ldx, W, Kpad, scale, shift, out, ldo, N, B);
}

// -------------------------------------------------------------------------------------
// Point head: 32 consecutive rows (points) of the flattened [B*68] batch per workgroup of 8 waves; the waves split the output
// channels of each layer, activations go through two LDS images P [32][516] and Q [32][260]:
//   pf -> Q;  conv6: Q -> P (512, + the face's g6);  conv7: P -> Q (256);  conv8: Q -> P (128);  conv9: P -> 3 channels
// then Lr = Lc + 0.05 res and the optional ROI affine (x sx + x0, y sy + y0, z (sx + sy) / 2 with sx = (ex - x0) / 120).
// -------------------------------------------------------------------------------------
namespace {
constexpr int kHeadRows = 32, kLdP = 516, kLdQ = 260;

// rows [0,32) x channels [n0, n0 + 16 NT) of one layer: X = LDS input image (row stride ldx), W [N][K]
template <int K, int NT>
__device__ __forceinline__ void head_tile(const float *X, int ldx, const float *__restrict__ W, int n0, int r16, int g, f32x4 (&acc)[2][NT]) {
    const float *x0 = X + r16 * ldx + 4 * g, *x1 = x0 + 16 * ldx;
    const float *wp = W + (size_t)(n0 + r16) * K + 4 * g;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 16) {
        const f32x4 a0 = *(const f32x4 *)(x0 + k0), a1 = *(const f32x4 *)(x1 + k0);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const f32x4 wf = *(const f32x4 *)(wp + (size_t)16 * i * K + k0);
            acc[0][i] = mfma4(wf, a0, acc[0][i]);
            acc[1][i] = mfma4(wf, a1, acc[1][i]);
        }
    }
}
}  // namespace

__global__ __launch_bounds__(512) void syn_point_head_kernel(SynHeadW w, const float *__restrict__ pf /*[B*68,64]*/, const float *__restrict__ g6 /*[B,512]*/,
                                                             const float *__restrict__ lmk_in /*[B,3,68]*/, const float *__restrict__ roi /*nullable [B,5]*/,
                                                             float *__restrict__ out /*[B,3,68]*/, int rows) {
    __shared__ __attribute__((aligned(16))) float sm[kHeadRows * (kLdP + kLdQ)];      // ONE shared object (see resnet_kernels.hip conv_lt_kernel)
    float *const P = sm, *const Q = sm + kHeadRows * kLdP;
    const int m0 = blockIdx.x * kHeadRows;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    {                                                       // 32 rows x 64 floats = 512 float4: one per thread; tail rows are clamped copies
        const int r = tid >> 4, c = (tid & 15) * 4;
        const int m = m0 + r < rows ? m0 + r : rows - 1;
        *(f32x4 *)&Q[r * kLdQ + c] = *(const f32x4 *)&pf[(size_t)m * 64 + c];
    }
    __syncthreads();
    // conv6: 512 channels, 64 per wave
    {
        int face[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + 16 * j + r16;
            face[j] = (m < rows ? m : rows - 1) / kSynPts;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n0 = wave * 64 + h * 32;
            f32x4 acc[2][2];
            head_tile<64, 2>(Q, kLdQ, w.W6p, n0, r16, g, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int n = n0 + 16 * i + 4 * g;
                const f32x4 sc = *(const f32x4 *)&w.scale6[n], sh = *(const f32x4 *)&w.shift6[n];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const f32x4 gv = *(const f32x4 *)&g6[(size_t)face[j] * 512 + n];
                    *(f32x4 *)&P[(16 * j + r16) * kLdP + n] = relu4((acc[j][i] + gv) * sc + sh);
                }
            }
        }
    }
    __syncthreads();
    // conv7: 256 channels, 32 per wave
    {
        const int n0 = wave * 32;
        f32x4 acc[2][2];
        head_tile<512, 2>(P, kLdP, w.W7, n0, r16, g, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = n0 + 16 * i + 4 * g;
            const f32x4 sc = *(const f32x4 *)&w.scale7[n], sh = *(const f32x4 *)&w.shift7[n];
#pragma unroll
            for (int j = 0; j < 2; ++j) *(f32x4 *)&Q[(16 * j + r16) * kLdQ + n] = relu4(acc[j][i] * sc + sh);
        }
    }
    __syncthreads();
    // conv8: 128 channels, 16 per wave
    {
        const int n0 = wave * 16;
        f32x4 acc[2][1];
        head_tile<256, 1>(Q, kLdQ, w.W8, n0, r16, g, acc);
        const int n = n0 + 4 * g;
        const f32x4 sc = *(const f32x4 *)&w.scale8[n], sh = *(const f32x4 *)&w.shift8[n];
#pragma unroll
        for (int j = 0; j < 2; ++j) *(f32x4 *)&P[(16 * j + r16) * kLdP + n] = relu4(acc[j][0] * sc + sh);
    }
    __syncthreads();
    // conv9: 3 channels (W9 padded to 16 rows), waves 0 and 1 take one row tile each; lanes g = 0 hold channels 0..3 of their row
    if (wave < 2) {
        const float *x0 = P + (16 * wave + r16) * kLdP + 4 * g;
        const float *wp = w.W9 + (size_t)r16 * 128 + 4 * g;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k0 = 0; k0 < 128; k0 += 16) acc = mfma4(*(const f32x4 *)(wp + k0), *(const f32x4 *)(x0 + k0), acc);
        const f32x4 res = relu4(acc * *(const f32x4 *)&w.scale9[4 * g] + *(const f32x4 *)&w.shift9[4 * g]);
        const int m = m0 + 16 * wave + r16;
        if (g == 0 && m < rows) {
            const int b = m / kSynPts, p = m - b * kSynPts;
            float s3[3] = {1.f, 1.f, 1.f}, o3[3] = {0.f, 0.f, 0.f};
            if (roi) {
                const float sx = roi[b * 5 + 0], sy = roi[b * 5 + 1], ex = roi[b * 5 + 2], ey = roi[b * 5 + 3];
                const float scx = (ex - sx) / 120.0f, scy = (ey - sy) / 120.0f;
                s3[0] = scx; s3[1] = scy; s3[2] = (scx + scy) * 0.5f;
                o3[0] = sx; o3[1] = sy;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t at = ((size_t)b * 3 + c) * kSynPts + p;
                const float lr = lmk_in[at] + 0.05f * res[c];
                out[at] = roi ? lr * s3[c] + o3[c] : lr;
            }
        }
    }
}

void launch_syn_point_head(const SynHeadW &w, const float *pf, const float *g6, const float *lmk_in, const float *roi, float *out, int B,
                           hipStream_t s) {
    const int rows = B * kSynPts;
    syn_point_head_kernel<<<(rows + kHeadRows - 1) / kHeadRows, 512, 0, s>>>(w, pf, g6, lmk_in, roi, out, rows);
}

}  // namespace syn
