// Backward of the loss head of the training graph for gfx950: the two loss modules (reference loss_definition.py WingLoss /
// ParamLoss) on their own, and head_backward_kernel below -- the data gradients of MLP_rev, MLP_for and the landmark reconstruction
// (model_building.py:141-157) down to d param [B,62] and d pool [B,1280].
//
//   WingLoss   d loss / d pred[e] = g slope sign(pred - target) / n,   slope = omega / (epsilon + d) for d < omega, 1 for d >= omega,
//              d = |target - pred| (fp32, as the forward forms it), n = the number of elements of the whole batch that took a branch.
//              d == 0: sign is 0, gradient 0.  NaN d: neither branch, not counted, gradient 0 (a select, never 0 x NaN).  d = inf: linear
//              branch, +-1 / n.  n == 0 (every d NaN): every gradient is 0 -- the reference's masks route nothing to any element.
//   ParamLoss  L = sqrt(mean_a + mean_b):  d L / d input[k] = g diff[k] / (count L) with count = 12 (k < 12) or 50 (normal), 50 for the
//              first 50 inputs of only_3dmm (the other 12 receive 0); the target receives the negative, at the target's own (misaligned)
//              positions.  L == 0 gives 0 / 0 = NaN for the face's whole row, as torch's sqrt'(0) x 0 does; it stays in that row.
//
// Arithmetic: the difference in fp32, everything after it in fp64, ONE rounding to fp32 per gradient element.
// Order: no floating-point atomics, and no floating-point sum across elements at all in the WingLoss gradient: n is an INTEGER count,
// formed per fixed chunk of kWingChunk elements and folded by the workgroup that draws the last ticket (the protocol of loss_kernels.hip).
// A face's ParamLoss gradient is a function of that face's 124 numbers alone: every lane of the face's wave walks the same serial sum as
// the forward's param_loss_face, so L has the forward's bits.
#pragma clang fp contract(off)

#include "syn_internal.h"

namespace syn {

namespace {

constexpr int kGradThreads = 256;

// d < omega | d >= omega | neither (NaN)
__device__ __forceinline__ bool wing_counted(float pred, float target, float omega) {
    const float d = fabsf(target - pred);
    return d < omega || d >= omega;
}

}  // namespace

// -------------------------------------------------------------------------------------
// n of the batch: one workgroup per kWingChunk elements stores its count, the last one to finish folds them into count[gridDim.x].
// Integer sums: any order gives the same n.
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGradThreads) void wing_count_kernel(const float *__restrict__ pred, const float *__restrict__ target, size_t N,
                                                                  float omega, unsigned long long *count, unsigned *counter) {
    __shared__ unsigned long long lds[kGradThreads];
    __shared__ unsigned ticket;
    const int t = threadIdx.x;
    const size_t e0 = (size_t)blockIdx.x * kWingChunk;
    const size_t e1 = e0 + kWingChunk < N ? e0 + kWingChunk : N;
    unsigned long long n = 0;
    for (size_t e = e0 + t; e < e1; e += kGradThreads) n += wing_counted(pred[e], target[e], omega) ? 1u : 0u;
    lds[t] = n;
    __syncthreads();
    for (int s = kGradThreads / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    if (t == 0) count[blockIdx.x] = lds[0];
    __threadfence();                                      // the chunk's count before the ticket
    __syncthreads();
    if (t == 0) ticket = atomicAdd(counter, 1u);
    __syncthreads();
    if (ticket != gridDim.x - 1) return;
    __threadfence();                                      // the other workgroups' counts after their tickets
    if (t == 0) *counter = 0u;
    unsigned long long p = 0;
    for (unsigned c = t; c < gridDim.x; c += kGradThreads) p += count[c];
    __syncthreads();
    lds[t] = p;
    __syncthreads();
    for (int s = kGradThreads / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    if (t == 0) count[gridDim.x] = lds[0];
}

// one thread per element; total = &count[chunks] of the launch above
__global__ __launch_bounds__(kGradThreads) void wing_grad_kernel(const float *__restrict__ pred, const float *__restrict__ target, size_t N,
                                                                 float omega, float epsilon, const float *__restrict__ g /*nullable: 1*/,
                                                                 const unsigned long long *__restrict__ total, float *__restrict__ d_pred) {
    const size_t e = (size_t)blockIdx.x * kGradThreads + threadIdx.x;
    if (e >= N) return;
    const double up = g ? (double)g[0] : 1.0, n = (double)total[0];
    const float p = pred[e], t = target[e];
    const float d = fabsf(t - p);
    const float diff = p - t;
    const double sign = diff > 0.f ? 1.0 : diff < 0.f ? -1.0 : 0.0;             // NaN and 0: 0
    const double slope = d < omega ? (double)omega / ((double)epsilon + (double)d) : 1.0;
    const bool counted = d < omega || d >= omega;
    const double v = up * slope * sign / n;
    d_pred[e] = (counted && sign != 0.0) ? (float)v : 0.f;
}

void launch_wing_loss_backward(const float *pred, const float *target, size_t N, float omega, float epsilon, const float *g,
                               unsigned long long *count, unsigned *counter, float *d_pred, hipStream_t s) {
    const unsigned chunks = wing_chunks(N);
    wing_count_kernel<<<chunks, kGradThreads, 0, s>>>(pred, target, N, omega, count, counter);
    wing_grad_kernel<<<(unsigned)((N + kGradThreads - 1) / kGradThreads), kGradThreads, 0, s>>>(pred, target, N, omega, epsilon, g, count + chunks,
                                                                                              d_pred);
}

// -------------------------------------------------------------------------------------
// ParamLoss backward: one wave per face, four faces per workgroup; lane k owns parameter k of both outputs
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGradThreads) void param_loss_backward_kernel(const float *__restrict__ input, const float *__restrict__ target, int B,
                                                                           int mode, const float *__restrict__ g /*nullable [B]: ones*/,
                                                                           float *__restrict__ d_input /*nullable*/,
                                                                           float *__restrict__ d_target /*nullable*/) {
    const int b = blockIdx.x * (kGradThreads / 64) + (threadIdx.x >> 6), k = threadIdx.x & 63;
    if (b >= B || k >= kParam) return;
    const float *a = input + (size_t)b * kParam, *t = target + (size_t)b * kParam;
    const double up = g ? (double)g[b] : 1.0;
    float di = 0.f, dt = 0.f;
    if (mode == 0) {                                      // the sums of loss_kernels.hip param_loss_face, term for term
        double s0 = 0.0, s1 = 0.0;
        for (int j = 0; j < 12; ++j) { const float d = a[j] - t[j]; s0 += (double)d * (double)d; }
        for (int j = 12; j < kParam; ++j) { const float d = a[j] - t[j]; s1 += (double)d * (double)d; }
        const double L = sqrt(s0 / 12.0 + s1 / 50.0);
        const float d = a[k] - t[k];
        const double v = up * (double)d / ((k < 12 ? 12.0 : 50.0) * L);
        di = (float)v;
        dt = (float)-v;
    } else {
        double s = 0.0;
        for (int j = 0; j < 50; ++j) { const float d = a[j] - t[12 + j]; s += (double)d * (double)d; }
        const double L = sqrt(s / 50.0);
        if (k < 50) di = (float)(up * (double)(a[k] - t[12 + k]) / (50.0 * L));
        if (k >= 12) dt = (float)-(up * (double)(a[k - 12] - t[k]) / (50.0 * L));
    }
    if (d_input) d_input[(size_t)b * kParam + k] = di;
    if (d_target) d_target[(size_t)b * kParam + k] = dt;
}

void launch_param_loss_backward(const float *input, const float *target, int B, int mode, const float *g, float *d_input, float *d_target,
                                hipStream_t s) {
    constexpr int faces = kGradThreads / 64;
    param_loss_backward_kernel<<<(B + faces - 1) / faces, kGradThreads, 0, s>>>(input, target, B, mode, g, d_input, d_target);
}


void launch_wing_count(const float *pred, const float *target, size_t N, float omega, unsigned long long *count, unsigned *counter, hipStream_t s) {
    wing_count_kernel<<<wing_chunks(N), kGradThreads, 0, s>>>(pred, target, N, omega, count, counter);
}

// -------------------------------------------------------------------------------------
// Backward of the whole loss head: head_backward_kernel<0..3> hold ONE face per workgroup and walk it through the
// recomputed forward (for the ReLU signs and the arg-max routing) and the data gradients of MLP_rev, MLP_for and the landmark
// reconstruction; the products that have one row per FACE run between them as launches across faces (syn_face_gemm_kernel,
// face_tgemm_kernel).  Everything of a face is computed in an order fixed by the source, from that face's inputs and the two integer
// counts n0 / n1: a face's gradient has the same bits wherever it stands.  The layers' matrix products and their transposes run on the
// exact-fp32 matrix instruction (gemm_nt / gemm_nn / conv5_argmax below); conv1, conv9's transpose, the gather behind conv5 and the
// per-face vectors are plain fp32 fused multiply-adds in ascending order.  A face's activations and gradients live in its workgroup's
// scratch image (kHeadWs floats) from phase 0 to phase 3.
// -------------------------------------------------------------------------------------
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kHB = 256;                                  // threads per workgroup
static_assert(kSynPts % 4 == 0, "row tiles of four");       // kP = 68 = 17 x 4 rows
using namespace headimg;                                  // the workgroup's scratch image (syn_internal.h)
static_assert(headimg::kP == kSynPts, "one row per point");

// The matrix products run on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32 with the operand roles and the K walk of the
// forward (synergy_kernels.hip): MFMA rows = 16 outputs, MFMA columns = 16 points, K 16 at a time, a lane fetches one float4 (k0 + 4 g ..)
// per operand row and feeds element s to step s.  So a recomputed activation has the bits the forward launches produced for it, and the
// backward's ReLU signs are those of the values that went into Lr.  The 68 points are 5 row tiles; the 12 tail rows of the last tile
// are clamped copies of row 67 whose results are dropped (no conditional loads).  A wave owns 16 output columns at a time and runs
// the five row tiles past one weight fragment: five independent accumulators.
__device__ __forceinline__ float bn_relu(float acc, float sc, float sh) { return fmaxf(__builtin_fmaf(acc, sc, sh), 0.f); }

__device__ __forceinline__ f32x4 mfma4(f32x4 w, f32x4 x, f32x4 acc) {
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], x[s], acc, 0, 0, 0);
    return acc;
}

constexpr int kRowTiles = (kP + 15) / 16;                  // 5

// epi(m, n, sum_k X[m][k] W[n][k]) for m < 68, n < N (N a multiple of 64, K of 16)
template <class Epi>
__device__ __forceinline__ void gemm_nt(const float *X, int ldx, const float *__restrict__ W, int ldw, int K, int N, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const float *xp[kRowTiles];
#pragma unroll
    for (int t = 0; t < kRowTiles; ++t) { const int m = 16 * t + r16; xp[t] = X + (size_t)(m < kP ? m : kP - 1) * ldx + 4 * g; }
    for (int n0 = 16 * wave; n0 < N; n0 += 16 * (kHB / 64)) {
        const float *wp = W + (size_t)(n0 + r16) * ldw + 4 * g;
        f32x4 acc[kRowTiles];
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int k0 = 0; k0 < K; k0 += 16) {
            const f32x4 wf = *(const f32x4 *)(wp + k0);
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) acc[t] = mfma4(wf, *(const f32x4 *)(xp[t] + k0), acc[t]);
        }
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) {
            const int m = 16 * t + r16;
            if (m < kP) {
#pragma unroll
                for (int c = 0; c < 4; ++c) epi(m, n0 + 4 * g + c, acc[t][c]);
            }
        }
    }
    __syncthreads();
}

// epi(m, k, sum_n G[m][n] W[n][k]) for m < 68, k < K (K a multiple of 64, N of 16): the transposed product of a data gradient.  The
// weight fragment is read down a column of W: 16 lanes side by side, one dword per step.
template <class Epi>
__device__ __forceinline__ void gemm_nn(const float *G, int ldg, const float *__restrict__ W, int ldw, int N, int K, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const float *gp[kRowTiles];
#pragma unroll
    for (int t = 0; t < kRowTiles; ++t) { const int m = 16 * t + r16; gp[t] = G + (size_t)(m < kP ? m : kP - 1) * ldg + 4 * g; }
    for (int k0 = 16 * wave; k0 < K; k0 += 16 * (kHB / 64)) {
        const float *wp = W + (size_t)(4 * g) * ldw + k0 + r16;
        f32x4 acc[kRowTiles];
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int n0 = 0; n0 < N; n0 += 16) {
            f32x4 wf;
#pragma unroll
            for (int s = 0; s < 4; ++s) wf[s] = wp[(size_t)(n0 + s) * ldw];
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) acc[t] = mfma4(wf, *(const f32x4 *)(gp[t] + n0), acc[t]);
        }
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) {
            const int m = 16 * t + r16;
            if (m < kP) {
#pragma unroll
                for (int c = 0; c < 4; ++c) epi(m, k0 + 4 * g + c, acc[t][c]);
            }
        }
    }
    __syncthreads();
}


// Y = relu(scale (X W^T) + shift), [68][N]
__device__ __forceinline__ void layer_fwd(const float *X, int ldx, const float *W, int K, const float *sc, const float *sh, int N, float *Y) {
    gemm_nt(X, ldx, W, K, K, N, [=](int m, int n, float a) { Y[m * N + n] = bn_relu(a, sc[n], sh[n]); });
}

// conv1 from landmarks [3][68] (W [64][4], column 3 zero)
__device__ __forceinline__ void conv1_fwd(const float *L, const float *W, const float *sc, const float *sh, float *Y) {
    for (int idx = threadIdx.x; idx < kP * 64; idx += kHB) {
        const int m = idx >> 6, n = idx & 63;
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) a = __builtin_fmaf(W[n * 4 + c], L[c * kP + m], a);
        Y[idx] = bn_relu(a, sc[n], sh[n]);
    }
    __syncthreads();
}

// D <- (Y > 0 ? D scale : 0): the gradient at a layer's matrix product from the gradient at its ReLU output (a select, as torch's)
// Gu (nullable): the same gradient WITHOUT the scale, for the weight products; what D receives does not depend on it
__device__ __forceinline__ void mask_scale(float *D, const float *Y, const float *sc, int N, float *Gu = nullptr) {
    for (int idx = threadIdx.x; idx < kP * N; idx += kHB) {
        const float u = D[idx];
        const float d = u * sc[idx % N];
        const bool on = Y[idx] > 0.f;
        D[idx] = on ? d : 0.f;
        if (Gu) Gu[idx] = on ? u : 0.f;
    }
    __syncthreads();
}

// conv1's data gradient: out[c][m] = base(c, m) + sum_n D[m][n] W[n][c]   (D already masked and scaled)
template <class Base>
__device__ __forceinline__ void conv1_bwd(const float *D, const float *W, float *out, Base base) {
    for (int idx = threadIdx.x; idx < 3 * kP; idx += kHB) {
        const int c = idx / kP, m = idx - c * kP;
        float a = 0.f;
        for (int n = 0; n < 64; ++n) a = __builtin_fmaf(D[m * 64 + n], W[n * 4 + c], a);
        out[idx] = base(c, m) + a;
    }
    __syncthreads();
}

// conv5 (128 -> 1024) + max over the 68 points with the FIRST point that attains it (255: the maximum is 0, ReLU passes nothing), on
// the matrix unit with the trunk's K walk.  A lane holds 4 channels of the rows r16, 16 + r16, ...: it walks them in ascending order
// with a strict comparison, then the 16 lanes of its channel group fold (value, row) pairs -- the larger value, of equal values the
// smaller row.  A pair whose value is 0 carries row 255, and so do the clamped tail rows.
__device__ __forceinline__ void conv5_argmax(const float *A4, const float *__restrict__ W5, const float *sc, const float *sh, float *gf /*nullable*/,
                                          int *arg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const float *xp[kRowTiles];
#pragma unroll
    for (int t = 0; t < kRowTiles; ++t) { const int m = 16 * t + r16; xp[t] = A4 + (size_t)(m < kP ? m : kP - 1) * 128 + 4 * g; }
    for (int n0 = 16 * wave; n0 < kSynGlobal; n0 += 16 * (kHB / 64)) {
        const float *wp = W5 + (size_t)(n0 + r16) * 128 + 4 * g;
        f32x4 acc[kRowTiles];
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int k0 = 0; k0 < 128; k0 += 16) {
            const f32x4 wf = *(const f32x4 *)(wp + k0);
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) acc[t] = mfma4(wf, *(const f32x4 *)(xp[t] + k0), acc[t]);
        }
        const f32x4 s4 = *(const f32x4 *)&sc[n0 + 4 * g], h4 = *(const f32x4 *)&sh[n0 + 4 * g];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float best = 0.f;
            int at = 255;
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) {
                const int m = 16 * t + r16;
                const float v = m < kP ? bn_relu(acc[t][c], s4[c], h4[c]) : 0.f;
                const bool up = v > best;
                best = up ? v : best;
                at = up ? m : at;
            }
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const float ov = __shfl_xor(best, d);
                const int oa = __shfl_xor(at, d);
                const bool take = ov > best || (ov == best && oa < at);
                best = take ? ov : best;
                at = take ? oa : at;
            }
            if (r16 == 0) {
                if (gf) gf[n0 + 4 * g + c] = best;
                arg[n0 + 4 * g + c] = at;
            }
        }
    }
    __syncthreads();
}

// dA4[p][k] = sum over the channels c routed to point p of dgf[c] scale[c] W5[c][k]: thread (k, half) walks its 512 channels in order
// into its own LDS column, the two halves fold in a fixed order.  Loads are unconditional, the routing is a select.
__device__ __forceinline__ void conv5_gather(const float *dgf, const float *sc, const int *arg, const float *__restrict__ W5, float *lds, float *dA4) {
    for (int i = threadIdx.x; i < 2 * kP * 128; i += kHB) lds[i] = 0.f;
    __syncthreads();
    const int k = threadIdx.x & 127, half = threadIdx.x >> 7;
    float *acc = lds + half * kP * 128 + k;
    for (int c0 = half * 512; c0 < half * 512 + 512; c0 += 8) {      // eight channels' loads in flight, then their adds in channel order
        float coef[8], w[8];
        int p[8];
        bool on[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int a = arg[c0 + i];
            on[i] = a != 255;
            coef[i] = on[i] ? dgf[c0 + i] * sc[c0 + i] : 0.f;
            p[i] = on[i] ? a : 0;
            w[i] = W5[(size_t)(c0 + i) * 128 + k];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[p[i] * 128] = on[i] ? __builtin_fmaf(coef[i], w[i], acc[p[i] * 128]) : acc[p[i] * 128];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kP * 128; i += kHB) dA4[i] = lds[i] + lds[kP * 128 + i];
    __syncthreads();
}

__device__ __forceinline__ float wing_elem(float pred, float target, double up, double n, float omega, float epsilon) {
    const float d = fabsf(target - pred), diff = pred - target;
    const double sign = diff > 0.f ? 1.0 : diff < 0.f ? -1.0 : 0.0;
    const double slope = d < omega ? (double)omega / ((double)epsilon + (double)d) : 1.0;
    const bool counted = d < omega || d >= omega;
    return (counted && sign != 0.0) ? (float)(up * slope * sign / n) : 0.f;
}

}  // namespace

// -------------------------------------------------------------------------------------
// out[b][k] = sum_n G[b][n] W[n][k]: the transposed per-FACE product of a data gradient (d g6 -> d [gf | pool | shape | expr], d S2 ->
// d gf_rev), one wave per (16 faces, 32 outputs) as syn_face_gemm_kernel: MFMA rows = outputs, columns = faces.  W is the forward's
// [N][K] matrix, read down its columns; N a multiple of 16, K of 32.  A face's row depends on that face alone.
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void face_tgemm_kernel(const float *__restrict__ G, int ldg, const float *__restrict__ W, int ldw, int N,
                                                        float *__restrict__ out, int ldo, int B) {
    const int lane = threadIdx.x, r16 = lane & 15, g = lane >> 4;
    const int m = blockIdx.x * 16 + r16, k0 = blockIdx.y * 32;
    const float *gp = G + (size_t)(m < B ? m : B - 1) * ldg + 4 * g;                   // clamp tail rows (stores are masked)
    const float *wp = W + (size_t)(4 * g) * ldw + k0 + r16;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < N; n0 += 16) {
        f32x4 w0, w1;
#pragma unroll
        for (int s = 0; s < 4; ++s) { w0[s] = wp[(size_t)(n0 + s) * ldw]; w1[s] = wp[(size_t)(n0 + s) * ldw + 16]; }
        const f32x4 x = *(const f32x4 *)(gp + n0);
        acc0 = mfma4(w0, x, acc0);
        acc1 = mfma4(w1, x, acc1);
    }
    if (m >= B) return;
    *(f32x4 *)&out[(size_t)m * ldo + k0 + 4 * g] = acc0;
    *(f32x4 *)&out[(size_t)m * ldo + k0 + 16 + 4 * g] = acc1;
}

void launch_face_tgemm(const float *G, int ldg, const float *W, int ldw, int N, float *out, int ldo, int K, int B, hipStream_t s) {
    face_tgemm_kernel<<<dim3((B + 15) / 16, K / 32), 64, 0, s>>>(G, ldg, W, ldw, N, out, ldo, B);
}

// The walk of a face is cut where a product runs ACROSS faces (face_tgemm_kernel above, syn_face_gemm_kernel for MLP_rev's heads):
//   PH 0  recompute MLP_for and MLP_rev's trunk                                   -> gf_rev [B,1024]
//         S2 = MLP_rev's heads (syn_face_gemm_kernel, the forward's launch)
//   PH 1  the three ParamLosses                                                   -> d S2 (masked, scaled) [B,64], direct d param [B,64]
//         d gf_rev = d S2 Wrev (face_tgemm_kernel)
//   PH 2  MLP_rev backward, WingLoss of LMK_pointNet, MLP_for's conv9 .. conv6    -> d g6 [B,512]
//         d [gf | pool | shape | expr] = d g6 W6[:,64:] (face_tgemm_kernel)
//   PH 3  d pool, MLP_for's trunk backward, WingLoss of LMK_f0, reconstruction    -> d param
// Workgroup i of a launch holds face b0 + i; its image (slot i) carries the activations from PH 0 to PH 3.
template <int PH>
__global__ __launch_bounds__(kHB) void head_backward_kernel(HeadBwdArgs A, int b0) {
    __shared__ __attribute__((aligned(16))) float lds[2 * kP * 128];
    __shared__ float sS[3 * kP], sdv[3 * kP], sdS[3 * kP], sp[64];
    const int tid = threadIdx.x, B = A.B;
    const SynTrunkW &tf = A.tf, &tr = A.tr;
    const SynHeadW &hw = A.hw;
    const float omega = 10.f, epsilon = 2.f;
    {
        const int b = b0 + blockIdx.x;
        float *ws = A.ws + (size_t)blockIdx.x * kHeadWs;
        float *A1 = ws + oA1, *A3 = ws + oA3, *A4 = ws + oA4, *H6 = ws + oH6, *H7 = ws + oH7, *H8 = ws + oH8;
        float *B1 = ws + oB1, *B2 = ws + oB2, *B3 = ws + oB3, *B4 = ws + oB4, *D0 = ws + oD0, *D1 = ws + oD1, *DA2X = ws + oDA2X;
        float *M9 = ws + oM9, *DLR = ws + oDLR, *DLC = ws + oDLC;
        float *GFR = A.GFRg + (size_t)b * kSynGlobal, *S2 = A.S2g + (size_t)b * 64, *GS2 = A.GS2g + (size_t)b * 64, *DPAR = A.DPARg + (size_t)b * 64;
        float *DGF = A.DGFRg + (size_t)b * kSynGlobal, *DG6 = A.DG6g + (size_t)b * 512, *DX6 = A.DX6g + (size_t)b * kSynFaceKpad;
        int *ARGF = (int *)(ws + oARGF), *ARGR = (int *)(ws + oARGR);
        float *wg = A.wg ? A.wg + (size_t)blockIdx.x * kHeadWg : nullptr;      // unscaled gradients for the weight products
        auto gu = [wg](int off) -> float * { return wg ? wg + off : nullptr; };
        const float *Lc = A.Lc + (size_t)b * 3 * kP, *Lgt = A.Lgt + (size_t)b * 3 * kP, *Lr = A.Lr + (size_t)b * 3 * kP;
        const float *A2 = A.pf + (size_t)b * kP * 64, *G6 = A.G6 + (size_t)b * 512;
        const float *pa = A.param + (size_t)b * kParam, *tg = A.target + (size_t)b * kParam;

        if constexpr (PH == 0) {
        // ---- the forward again, for signs and routing: MLP_for
        conv1_fwd(Lc, tf.W[0], tf.scale[0], tf.shift[0], A1);
        layer_fwd(A2, 64, tf.W[2], 64, tf.scale[2], tf.shift[2], 64, A3);
        layer_fwd(A3, 64, tf.W[3], 64, tf.scale[3], tf.shift[3], 128, A4);
        conv5_argmax(A4, tf.W[4], tf.scale[4], tf.shift[4], nullptr, ARGF);
        gemm_nt(A2, 64, hw.W6p, 64, 64, 512, [=](int m, int n, float a) { H6[m * 512 + n] = bn_relu(a + G6[n], hw.scale6[n], hw.shift6[n]); });
        layer_fwd(H6, 512, hw.W7, 512, hw.scale7, hw.shift7, 256, H7);
        layer_fwd(H7, 256, hw.W8, 256, hw.scale8, hw.shift8, 128, H8);
        // conv9 with the forward's walk (W9 is padded to 16 rows): is the residual positive?
        gemm_nt(H8, 128, hw.W9, 128, 128, 16, [=](int m, int n, float a) { if (n < 4) M9[m * 4 + n] = n < 3 ? bn_relu(a, hw.scale9[n], hw.shift9[n]) : 0.f; });
        // ---- MLP_rev on the refined landmarks
        conv1_fwd(Lr, tr.W[0], tr.scale[0], tr.shift[0], B1);
        layer_fwd(B1, 64, tr.W[1], 64, tr.scale[1], tr.shift[1], 64, B2);
        layer_fwd(B2, 64, tr.W[2], 64, tr.scale[2], tr.shift[2], 64, B3);
        layer_fwd(B3, 64, tr.W[3], 64, tr.scale[3], tr.shift[3], 128, B4);
        conv5_argmax(B4, tr.W[4], tr.scale[4], tr.shift[4], GFR, ARGR);
        }
        if constexpr (PH == 1) {
        // ---- the three ParamLosses (fp32 differences, fp64 behind them, one rounding)
        if (tid < 64) {
            const int k = tid;
            const double g0 = A.g_per_face ? (double)A.g_per_face[b] : 1.0 / B;
            const double g1 = A.g_per_face ? (double)A.g_per_face[(size_t)B + b] : 1.0 / B;
            const double g2 = A.g_per_face ? (double)A.g_per_face[(size_t)2 * B + b] : 1.0 / B;
            double s0 = 0.0, s1 = 0.0, t1 = 0.0, t2 = 0.0;
            for (int j = 0; j < 12; ++j) { const float d = pa[j] - tg[j]; s0 += (double)d * (double)d; }
            for (int j = 12; j < kParam; ++j) { const float d = pa[j] - tg[j]; s1 += (double)d * (double)d; }
            for (int j = 0; j < 50; ++j) {
                const float d1 = S2[j] - tg[12 + j], d2 = S2[j] - pa[12 + j];
                t1 += (double)d1 * (double)d1;
                t2 += (double)d2 * (double)d2;
            }
            const double L0 = sqrt(s0 / 12.0 + s1 / 50.0), L1 = sqrt(t1 / 50.0), L2 = sqrt(t2 / 50.0);
            double dpar = 0.0, ds2 = 0.0;
            if (k < kParam) dpar = g0 * 0.02 * (double)(pa[k] - tg[k]) / ((k < 12 ? 12.0 : 50.0) * L0);
            if (k < 50) ds2 = g1 * 0.02 * (double)(S2[k] - tg[12 + k]) / (50.0 * L1) + g2 * 0.001 * (double)(S2[k] - pa[12 + k]) / (50.0 * L2);
            if (k >= 12 && k < kParam) dpar -= g2 * 0.001 * (double)(S2[k - 12] - pa[k]) / (50.0 * L2);
            GS2[k] = (k < kParam && S2[k] > 0.f) ? (float)ds2 * A.sc_rev[k] : 0.f;
            if (A.GS2Ug) A.GS2Ug[(size_t)b * 64 + k] = (k < kParam && S2[k] > 0.f) ? (float)ds2 : 0.f;
            DPAR[k] = k < kParam ? (float)dpar : 0.f;
        }
        __syncthreads();

        }
        if constexpr (PH == 2) {
        // ---- MLP_rev backward behind the heads' transpose: max routing, conv5 .. conv1
        conv5_gather(DGF, tr.scale[4], ARGR, tr.W[4], lds, D0);
        mask_scale(D0, B4, tr.scale[3], 128, gu(wR4));
        gemm_nn(D0, 128, tr.W[3], 64, 128, 64, [=](int m, int k, float a) { D1[m * 64 + k] = a; });
        mask_scale(D1, B3, tr.scale[2], 64, gu(wR3));
        gemm_nn(D1, 64, tr.W[2], 64, 64, 64, [=](int m, int k, float a) { D0[m * 64 + k] = a; });
        mask_scale(D0, B2, tr.scale[1], 64, gu(wR2));
        gemm_nn(D0, 64, tr.W[1], 64, 64, 64, [=](int m, int k, float a) { D1[m * 64 + k] = a; });
        mask_scale(D1, B1, tr.scale[0], 64, gu(wR1));
        {
            const double up = (A.g_scalars ? (double)A.g_scalars[1] : 1.0) * 0.05, n1 = (double)A.n1[0];
            conv1_bwd(D1, tr.W[0], DLR, [=](int c, int m) { return wing_elem(Lr[c * kP + m], Lgt[c * kP + m], up, n1, omega, epsilon); });
        }

        // ---- MLP_for backward: conv9 .. conv6
        for (int idx = tid; idx < kP * 128; idx += kHB) {
            const int m = idx >> 7, k = idx & 127;
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float g = M9[m * 4 + c] > 0.f ? 0.05f * DLR[c * kP + m] * hw.scale9[c] : 0.f;
                a = __builtin_fmaf(g, hw.W9[c * 128 + k], a);
            }
            D0[idx] = a;
        }
        if (wg)
            for (int idx = tid; idx < kP * 4; idx += kHB) {
                const int m = idx >> 2, c = idx & 3;
                wg[wG9 + idx] = (c < 3 && M9[m * 4 + c] > 0.f) ? 0.05f * DLR[c * kP + m] : 0.f;
            }
        __syncthreads();
        mask_scale(D0, H8, hw.scale8, 128, gu(wG8));
        gemm_nn(D0, 128, hw.W8, 256, 128, 256, [=](int m, int k, float a) { D1[m * 256 + k] = a; });
        mask_scale(D1, H7, hw.scale7, 256, gu(wG7));
        gemm_nn(D1, 256, hw.W7, 512, 256, 512, [=](int m, int k, float a) { D0[m * 512 + k] = a; });
        mask_scale(D0, H6, hw.scale6, 512, gu(wG6));                    // D0 = the gradient at conv6's sums [68][512]
        gemm_nn(D0, 512, hw.W6p, 64, 512, 64, [=](int m, int k, float a) { DA2X[m * 64 + k] = a; });
        for (int n = tid; n < 512; n += kHB) {                   // the per-face half: the sum over the face's points, in point order
            float a = 0.f;
            for (int p = 0; p < kP; ++p) a += D0[p * 512 + n];
            DG6[n] = a;
        }
        if (wg)
            for (int n = tid; n < 512; n += kHB) {               // the same sum of the unscaled gradient
                float a = 0.f;
                for (int p = 0; p < kP; ++p) a += wg[wG6 + p * 512 + n];
                A.DG6Ug[(size_t)b * 512 + n] = a;
            }
        __syncthreads();
        }
        if constexpr (PH == 3) {
        for (int i = tid; i < kPool; i += kHB) A.d_pool[(size_t)b * kPool + i] = DX6[kSynGlobal + i];
        // ---- max routing, conv5 .. conv1 of MLP_for; conv6's per-point half joins at conv2's output
        conv5_gather(DX6, tf.scale[4], ARGF, tf.W[4], lds, D0);
        mask_scale(D0, A4, tf.scale[3], 128, gu(wF4));
        gemm_nn(D0, 128, tf.W[3], 64, 128, 64, [=](int m, int k, float a) { D1[m * 64 + k] = a; });
        mask_scale(D1, A3, tf.scale[2], 64, gu(wF3));
        gemm_nn(D1, 64, tf.W[2], 64, 64, 64, [=](int m, int k, float a) { D0[m * 64 + k] = a + DA2X[m * 64 + k]; });
        mask_scale(D0, A2, tf.scale[1], 64, gu(wF2));
        gemm_nn(D0, 64, tf.W[1], 64, 64, 64, [=](int m, int k, float a) { D1[m * 64 + k] = a; });
        mask_scale(D1, A1, tf.scale[0], 64, gu(wF1));
        {
            const double up = (A.g_scalars ? (double)A.g_scalars[0] : 1.0) * 0.05, n0 = (double)A.n0[0];
            conv1_bwd(D1, tf.W[0], DLC, [=](int c, int m) { return DLR[c * kP + m] + wing_elem(Lc[c * kP + m], Lgt[c * kP + m], up, n0, omega, epsilon); });
        }

        // ---- landmark reconstruction backward (crop space, transform = 1: row 1 is flipped)
        if (tid < kParam) sp[tid] = __builtin_fmaf(pa[tid], A.stdv[tid], A.mean[tid]);
        if (tid < 3 * kP) sdv[tid] = (tid / kP == 1) ? -DLC[tid] : DLC[tid];
        __syncthreads();
        if (tid < kP) {                                          // the unposed landmark, as lmk_pose_kernel forms it
            const int T = tid >> 5, j = tid & 31;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *bc = A.basis + ((size_t)T * 3 + c) * (kBasisK * 32);
                float acc = 0.f;
                for (int k = 0; k < 48; ++k) acc = __builtin_fmaf(bc[lmk_tile_offset(j, k)], sp[12 + k], acc);
                acc = __builtin_fmaf(bc[lmk_tile_offset(j, 48)], sp[60], acc);
                acc = __builtin_fmaf(bc[lmk_tile_offset(j, 49)], sp[61], acc);
                acc += bc[lmk_tile_offset(j, 50)];
                sS[c * kP + tid] = acc;
            }
#pragma unroll
            for (int c2 = 0; c2 < 3; ++c2) {                     // d V = p^T d v
                float a = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) a = __builtin_fmaf(sp[4 * c + c2], sdv[c * kP + tid], a);
                sdS[c2 * kP + tid] = a;
            }
        }
        __syncthreads();
        if (tid < kParam) {
            float a = 0.f;
            if (tid < 12) {
                const int c = tid >> 2, c2 = tid & 3;
                if (c2 < 3) for (int p = 0; p < kP; ++p) a = __builtin_fmaf(sdv[c * kP + p], sS[c2 * kP + p], a);      // d p = d v V^T
                else for (int p = 0; p < kP; ++p) a += sdv[c * kP + p];                                                  // d offset
            } else {
                const int k = tid - 12;                          // d alpha = w_base^T d V
                for (int p = 0; p < kP; ++p) {
                    const int T = p >> 5, j = p & 31;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float *bc = A.basis + ((size_t)T * 3 + c) * (kBasisK * 32);
                        const float w = bc[lmk_tile_offset(j, k)];
                        a = __builtin_fmaf(w, sdS[c * kP + p], a);
                    }
                }
            }
            const float direct = tid >= 12 ? DPAR[tid] + DX6[kSynGlobal + kPool + (tid - 12)] : DPAR[tid];
            A.d_param[(size_t)b * kParam + tid] = __builtin_fmaf(a, A.stdv[tid], direct);
        }
        }
    }
}

void launch_head_backward_phase(int phase, const HeadBwdArgs &a, int b0, int faces, hipStream_t s) {
    if (phase == 0) head_backward_kernel<0><<<faces, kHB, 0, s>>>(a, b0);
    else if (phase == 1) head_backward_kernel<1><<<faces, kHB, 0, s>>>(a, b0);
    else if (phase == 2) head_backward_kernel<2><<<faces, kHB, 0, s>>>(a, b0);
    else head_backward_kernel<3><<<faces, kHB, 0, s>>>(a, b0);
}

}  // namespace syn
