// gfx950 (MI355X / CDNA4) kernels for the GhostNet backbone (reference backbone_nets/ghostnet_backbone.py:76-233): a 3x3 / 2 stem
// (mb1_stem_kernel, mobilenet1_kernels.hip, C0 = 16), 16 GhostBottlenecks, a 1x1 ConvBnAct 160 -> 960, pool, conv_head, heads.
// A GhostModule is a 1x1 convolution (`primary`) followed by a depthwise 3x3 on ITS OWN OUTPUT (`cheap`), the two concatenated:
// the reverse order of a MobileNetV1 block.  Activations are NHWC fp32; every 1x1 product (K = 16 .. 960) runs on
// v_mfma_f32_16x16x4_f32 with the operand roles of mb1_pointwise_kernel (channels on the A side, pixels on the B side: an
// accumulator is a float4 of four consecutive output channels of one pixel); depthwise taps and the squeeze-and-excite means are
// plain fp32 FMAs in a fixed order.  No fp16 piece, no atomics: a result does not depend on scheduling.
//
//   gn_pointwise_kernel   1x1 convolution, K and N any multiples of 4 (ragged last 16-wide tiles are masked), row pitches and a channel
//                         offset (`primary` writes the first half of the concatenated tensor in place), scale / shift, ReLU or hard
//                         sigmoid, optional per-(face, k) gate multiplied into the pixel operand as it is loaded (SE applied on read)
//   gn_depthwise_kernel   depthwise 3x3 s1 / 3x3 s2 / 5x5 s2, pad k / 2, channel slices in and out, BN, optional ReLU and residual
//   gn_mean_kernel        per-face channel means (the SE squeeze and the global pool); the two SE convolutions and conv_head are
//                         gn_pointwise launches with M = faces, so a weight fragment serves 16 faces
//   gn_ghost_kernel       a whole GhostModule per launch for the 15^2, 8^2 and 4^2 maps: `primary` lives in LDS
#include "syn_internal.h"

namespace syn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// act: 0 none, 1 ReLU, 2 hard sigmoid relu6(v + 3) / 6 (ghostnet_backbone.py:34-38)
__device__ __forceinline__ f32x4 gn_act(f32x4 v, int act) {
    f32x4 o = v;
    if (act == 1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = fmaxf(v[t], 0.0f);
    } else if (act == 2) {
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = fminf(fmaxf(v[t] + 3.0f, 0.0f), 6.0f) / 6.0f;
    }
    return o;
}

// =====================================================================================
// C[m][coff + n] = act(scale[n] * sum_k (A[m][k] * gate[m / HW][k]) W[n][k] + shift[n]).  A [M] rows of pitch lda, W [N][K] row-major,
// C rows of pitch ldc.  K % 4 == 0, N % 4 == 0, every pitch and offset a multiple of 4 (16-byte accesses).  A wave owns 16 MT pixels x
// 16 channels, the 4 waves of a block stack along M, blockIdx.y = channel tile.  A k step is 16 wide: lane (r, g) carries k0 + 4g ..
// k0 + 4g + 3 of row r on both sides, element s feeds MFMA step s.  Where k0 + 4g >= K (K = 24, 40, 72, 120, 184, 200 are 8 mod 16) the
// lane loads from a clamped address and both fragments are zeroed; weight rows past N are clamped and their stores masked.
// =====================================================================================
template <int MT>
__global__ __launch_bounds__(256) void gn_pointwise_kernel(const float *__restrict__ A, int lda, const float *__restrict__ W,
                                                           const float *__restrict__ scale, const float *__restrict__ shift,
                                                           const float *__restrict__ gate, int HW, float *__restrict__ C, int ldc,
                                                           int M, int K, int N, int act) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 4 + wave) * (MT * 16);
    const int n0 = blockIdx.y * 16;
    if (m0 >= M) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int nr = n0 + r16 < N ? n0 + r16 : N - 1;
    const float *wp = W + (size_t)nr * K;
    const float *ap[MT], *gp[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        int m = m0 + j * 16 + r16;
        m = m < M ? m : M - 1;                               // clamp tail rows (stores are masked)
        ap[j] = A + (size_t)m * lda;
        gp[j] = gate ? gate + (size_t)(m / HW) * K : nullptr;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] = zero;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int k = k0 + 4 * g;
        const bool kv = k < K;
        const int kc = kv ? k : K - 4;
        f32x4 wf = *(const f32x4 *)(wp + kc);
        wf = kv ? wf : zero;
        f32x4 af[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            f32x4 a = *(const f32x4 *)(ap[j] + kc);
            if (gate) a = a * *(const f32x4 *)(gp[j] + kc);
            af[j] = kv ? a : zero;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], af[j][s], acc[j], 0, 0, 0);
    }
    const int n = n0 + 4 * g;
    if (n >= N) return;                                      // N % 4 == 0: a lane's four channels are all inside or all outside
    const f32x4 one = {1.f, 1.f, 1.f, 1.f};
    const f32x4 sc = scale ? *(const f32x4 *)&scale[n] : one;
    const f32x4 sh = *(const f32x4 *)&shift[n];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const int m = m0 + j * 16 + r16;
        if (m >= M) continue;
        *(f32x4 *)&C[(size_t)m * ldc + n] = gn_act(acc[j] * sc + sh, act);
    }
}

void launch_gn_pointwise(const float *A, int lda, const float *W, const float *scale, const float *shift, const float *gate, int HW,
                         float *C, int ldc, int M, int K, int N, int act, hipStream_t s) {
    const dim3 grid((M + 255) / 256, (N + 15) / 16);
    gn_pointwise_kernel<4><<<grid, 256, 0, s>>>(A, lda, W, scale, shift, gate, HW, C, ldc, M, K, N, act);
}

// =====================================================================================
// Depthwise KS x KS, stride 1 | 2, pad KS / 2, + BN (+ ReLU) (+ residual).  Thread = (output pixel, 4 channels).  `in` and `out` point
// at the first channel of their slices; ldi / ldo / ldr are the row pitches of the tensors they live in.  Every pixel is decoded to
// (face, y, x) and its taps are tested against its own face; a padded tap is loaded from a clamped address and zeroed, so the sum
// always has KS^2 terms in the same order (as the LDS stage of gn_ghost_kernel).  pass_out (stride 1 only): the input's own pixel, plus
// pass_res, is stored there too -- ghost2's `primary` half receives the shortcut in the launch that reads it last, since `cheap`
// needs the values without the shortcut.
// =====================================================================================
template <int KS>
__global__ __launch_bounds__(256) void gn_depthwise_kernel(const float *__restrict__ in, int ldi, const float *__restrict__ w,
                                                           const float *__restrict__ scale, const float *__restrict__ shift,
                                                           float *__restrict__ out, int ldo, const float *__restrict__ res, int ldr,
                                                           float *__restrict__ pass_out, const float *__restrict__ pass_res, long total,
                                                           int Hin, int Hout, int C4, int stride, int relu) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = 4 * (int)(idx % C4), C = 4 * C4;
    const long p = idx / C4;                                 // output pixel of the flattened [B][Hout][Hout]
    const int ox = (int)(p % Hout);
    const long q = p / Hout;
    const int oy = (int)(q % Hout);
    const long b = q / Hout;
    const float *xb = in + (size_t)b * Hin * Hin * ldi + c;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc = zero;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
        const int iy = oy * stride - KS / 2 + ky, iyc = iy < 0 ? 0 : (iy >= Hin ? Hin - 1 : iy);
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int ix = ox * stride - KS / 2 + kx, ixc = ix < 0 ? 0 : (ix >= Hin ? Hin - 1 : ix);
            const f32x4 ld = *(const f32x4 *)&xb[(size_t)(iyc * Hin + ixc) * ldi];
            const f32x4 v = (iy == iyc && ix == ixc) ? ld : zero;      // a padded tap contributes nothing
            acc += v * *(const f32x4 *)&w[(ky * KS + kx) * C + c];
        }
    }
    f32x4 o = gn_act(acc * *(const f32x4 *)&scale[c] + *(const f32x4 *)&shift[c], relu);
    if (res) o += *(const f32x4 *)&res[(size_t)p * ldr + c];
    *(f32x4 *)&out[(size_t)p * ldo + c] = o;
    if (pass_out) {
        f32x4 v = *(const f32x4 *)&xb[(size_t)(oy * Hin + ox) * ldi];
        if (pass_res) v += *(const f32x4 *)&pass_res[(size_t)p * ldr + c];
        *(f32x4 *)&pass_out[(size_t)p * ldo + c] = v;
    }
}

void launch_gn_depthwise(const float *in, int ldi, const float *w, const float *scale, const float *shift, float *out, int ldo,
                         const float *res, int ldr, float *pass_out, const float *pass_res, int B, int Hin, int Hout, int C, int ks,
                         int stride, int relu, hipStream_t s) {
    const long total = (long)B * Hout * Hout * (C / 4);
    const int grid = (int)((total + 255) / 256);
    if (ks == 5)
        gn_depthwise_kernel<5><<<grid, 256, 0, s>>>(in, ldi, w, scale, shift, out, ldo, res, ldr, pass_out, pass_res, total, Hin, Hout, C / 4, stride, relu);
    else
        gn_depthwise_kernel<3><<<grid, 256, 0, s>>>(in, ldi, w, scale, shift, out, ldo, res, ldr, pass_out, pass_res, total, Hin, Hout, C / 4, stride, relu);
}

// Per-face channel means: in [B][HW] rows of pitch ld (C channels used), out [B][C].  Thread = (face, 4 channels); the HW terms are
// added in pixel order, eight loads in flight.
__global__ __launch_bounds__(256) void gn_mean_kernel(const float *__restrict__ in, int ld, float *__restrict__ out, int total, int HW,
                                                      int C4) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = 4 * (idx % C4), b = idx / C4;
    const float *f = in + (size_t)b * HW * ld + c;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    int p = 0;
    for (; p + 8 <= HW; p += 8) {
        f32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *(const f32x4 *)&f[(size_t)(p + i) * ld];
#pragma unroll
        for (int i = 0; i < 8; ++i) a += v[i];
    }
    for (; p < HW; ++p) a += *(const f32x4 *)&f[(size_t)p * ld];
    *(f32x4 *)&out[(size_t)b * (4 * C4) + c] = a * (1.0f / (float)HW);
}

void launch_gn_mean(const float *in, int ld, float *out, int B, int HW, int C, hipStream_t s) {
    const int total = B * (C / 4);
    gn_mean_kernel<<<(total + 255) / 256, 256, 0, s>>>(in, ld, out, total, HW, C / 4);
}

// =====================================================================================
// Fused GhostModule: Y[.., 0 .. N1) = primary (+ shortcut), Y[.., N1 .. 2 N1) = cheap(primary) (+ shortcut), one launch, one store.
//
// `cheap` is depthwise, so an output channel needs only the same `primary` channel -- over the whole map.  A workgroup (4 waves) owns
// F faces x kGnCG = 32 primary channels (blockIdx.y walks the channel groups): F = 1 at 15^2 (225 pixels, 15 pixel tiles of 16 with the
// last one partly empty), F = 1 or 2 at 8^2 (4 or 8 tiles) and F = 4 at 4^2 (4 tiles, one face each), so a wave has up to four pixel
// tiles that reuse one weight fragment.  Tile t belongs to wave t % 4.
//   1. GEMM exactly as gn_pointwise_kernel (same k walk, same clamps, same gate on the operand load): 2 channel tiles per pixel tile.
//   2. scale / shift (+ ReLU) and a float4 store to T[face-local row][kGnPitch]; rows of padded pixels are never stored.
//   3. barrier; thread = (row, channel quad) walks the F * HW rows: the 9 taps come from T, bounds-tested against the row's own face
//      (a padded tap reads a clamped row and is zeroed), BN (+ ReLU), and both halves of the concatenation are stored with the
//      matching halves of the shortcut added.  `primary` never reaches HBM without the shortcut.
// T is 225 rows x 36 floats = 31.6 KiB: five workgroups fit a CU's 160 KiB.  The pitch 36 = 4 mod 32 dwords: the eight float4 of a row
// are one 128-byte run and consecutive rows start 4 banks further on, so the GEMM stage's float4 stores (lane (r, g): row r) spread
// over all banks, and a stage-3 wave (8 consecutive rows x 8 quads per tap) covers 8 runs that overlap pairwise in at most 4 banks.
// =====================================================================================
constexpr int kGnCG = 32, kGnPitch = 36, kGnRows = 225;

__global__ __launch_bounds__(256) void gn_ghost_kernel(const float *__restrict__ X, int ldx, const float *__restrict__ gate,
                                                       const float *__restrict__ Wp, const float *__restrict__ p_scale,
                                                       const float *__restrict__ p_shift, const float *__restrict__ Wd,
                                                       const float *__restrict__ d_scale, const float *__restrict__ d_shift,
                                                       const float *__restrict__ res, int ldr, float *__restrict__ Y, int B, int H,
                                                       int K, int N1, int F, int relu) {
    __shared__ __attribute__((aligned(16))) float T[kGnRows * kGnPitch];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int HW = H * H, tpf = (HW + 15) >> 4, ntiles = F * tpf;
    const int b0 = blockIdx.x * F, c0 = blockIdx.y * kGnCG;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // ---- 1. primary = X (* gate) . Wp^T for this workgroup's faces and 32 channels ----
    bool tv[4];
    int trow[4];                                             // face-local LDS row of this lane's pixel, -1 for a padded pixel
    const float *ap[4], *gp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = wave + 4 * j;
        const int f = t / tpf, lt = t - f * tpf;
        tv[j] = t < ntiles && b0 + f < B;                    // (wave-uniform)
        const int face = b0 + f < B ? b0 + f : B - 1;
        const int pix = lt * 16 + r16;
        trow[j] = pix < HW ? f * HW + pix : -1;
        const int pc = pix < HW ? pix : HW - 1;
        ap[j] = X + ((size_t)face * HW + pc) * ldx;
        gp[j] = gate ? gate + (size_t)face * K : nullptr;
    }
    const float *wp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = c0 + i * 16 + r16;
        wp[i] = Wp + (size_t)(n < N1 ? n : N1 - 1) * K;
    }
    f32x4 acc[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = zero;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int k = k0 + 4 * g;
        const bool kv = k < K;
        const int kc = kv ? k : K - 4;
        f32x4 wf[2], af[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            wf[i] = *(const f32x4 *)(wp[i] + kc);
            wf[i] = kv ? wf[i] : zero;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            af[j] = zero;
            if (tv[j]) {
                f32x4 a = *(const f32x4 *)(ap[j] + kc);
                if (gate) a = a * *(const f32x4 *)(gp[j] + kc);
                af[j] = kv ? a : zero;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!tv[j]) continue;
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i][s], af[j][s], acc[j][i], 0, 0, 0);
            }
    }
    // ---- 2. BN (+ ReLU) -> T ----
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = c0 + i * 16 + 4 * g;
        const bool nv = n < N1;
        const f32x4 sc = nv ? *(const f32x4 *)&p_scale[n] : zero;
        const f32x4 sh = nv ? *(const f32x4 *)&p_shift[n] : zero;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (tv[j] && trow[j] >= 0) *(f32x4 *)&T[trow[j] * kGnPitch + i * 16 + 4 * g] = gn_act(acc[j][i] * sc + sh, relu);
    }
    __syncthreads();
    // ---- 3. cheap = depthwise 3x3 of T, and the one store of both halves ----
    const int q = threadIdx.x & 7, c = c0 + 4 * q;
    if (c >= N1) return;
    f32x4 wv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = *(const f32x4 *)&Wd[t * N1 + c];
    const f32x4 dsc = *(const f32x4 *)&d_scale[c], dsh = *(const f32x4 *)&d_shift[c];
    const int rows = F * HW, ldy = 2 * N1;
    for (int row = threadIdx.x >> 3; row < rows; row += 32) {
        const int f = row / HW, pix = row - f * HW;
        if (b0 + f >= B) break;
        const int oy = pix / H, ox = pix - oy * H;
        f32x4 a = zero;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy - 1 + ky, iyc = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox - 1 + kx, ixc = ix < 0 ? 0 : (ix >= H ? H - 1 : ix);
                const f32x4 ld = *(const f32x4 *)&T[(f * HW + iyc * H + ixc) * kGnPitch + 4 * q];
                const f32x4 v = (iy == iyc && ix == ixc) ? ld : zero;
                a += v * wv[ky * 3 + kx];
            }
        }
        f32x4 o1 = gn_act(a * dsc + dsh, relu);
        f32x4 o0 = *(const f32x4 *)&T[row * kGnPitch + 4 * q];
        const size_t m = (size_t)(b0 + f) * HW + pix;
        if (res) {
            o0 += *(const f32x4 *)&res[m * ldr + c];
            o1 += *(const f32x4 *)&res[m * ldr + N1 + c];
        }
        *(f32x4 *)&Y[m * ldy + c] = o0;
        *(f32x4 *)&Y[m * ldy + N1 + c] = o1;
    }
}

// gn_ghost_exists: the maps whose whole face fits the LDS tile; gn_ghost_faces: faces per workgroup there (F * H * H <= kGnRows).
// Measured (DESIGN 5.14, B = 32 / 128 / 1024): at 4^2, 4 faces beat 1, 2, 8 and 16 at every size; at 8^2, 1 face is the fastest at 32 and 128
// faces and 2 faces at 1024 (4 lose everywhere), so 8^2 takes 2 from kGnTwoFacesMinBatch faces on -- the smallest size at which 2 were
// measured faster -- and 1 below.  Results do not depend on F: a pixel's sums are the same.
bool gn_ghost_exists(int H) { return H == 15 || H == 8 || H == 4; }
int gn_ghost_faces(int H, int B) { return H == 4 ? 4 : (H == 8 && B >= kGnTwoFacesMinBatch ? 2 : 1); }

void launch_gn_ghost(const float *X, int ldx, const float *gate, const float *Wp, const float *p_scale, const float *p_shift,
                     const float *Wd, const float *d_scale, const float *d_shift, const float *res, int ldr, float *Y, int B, int H,
                     int K, int N1, int relu, hipStream_t s) {
    const int F = gn_ghost_faces(H, B);
    const dim3 grid((B + F - 1) / F, (N1 + kGnCG - 1) / kGnCG);
    gn_ghost_kernel<<<grid, 256, 0, s>>>(X, ldx, gate, Wp, p_scale, p_shift, Wd, d_scale, d_shift, res, ldr, Y, B, H, K, N1, F, relu);
}

}  // namespace syn
