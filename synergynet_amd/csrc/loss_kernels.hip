// The five losses of the training graph's forward (reference model_building.py:141-157, loss_definition.py) and the CenterCrop of the
// reference's benchmark loader (utils/ddfa.py:162-243, mode 'test') for gfx950.  DESIGN 5.17.
//
//   WingLoss(pred, target)   d = |target - pred| (fp32, as the reference forms it);  d < omega: omega log(1 + d / eps),  d >= omega: d - C,
//                            C = omega - omega log(1 + omega / eps);  sum of the terms / number of elements that took a branch.  A NaN d
//                            takes neither (both comparisons are false): it is neither summed nor counted.  d == omega is linear.
//   ParamLoss(a, b)          normal:    sqrt(mean((a[:12] - b[:12])^2) + mean((a[12:62] - b[12:62])^2))
//                            only_3dmm: sqrt(mean((a[:50] - b[12:62])^2))          (the reference's own misaligned slices)
//
// Arithmetic: differences in fp32 (the reference's), everything after them in fp64, ONE rounding to fp32 at the end.
// Order: no floating-point atomics anywhere.  A per-face loss is a serial sum of one thread over the face's 62 values: the same bits
// wherever the face stands.  A batch sum is cut into fixed chunks (kWingChunk elements / kLossFaces faces per workgroup -- constants, not
// launch parameters); inside a chunk thread t sums elements t, t + 256, ... and the 256 sums fold as a binary tree; every workgroup
// stores its chunk sum, takes a ticket from an INTEGER counter, and the workgroup that draws the last ticket folds the chunk sums the
// same way (thread t: chunks t, t + 256, ..., then the tree).  The result is a function of the element count alone.
#pragma clang fp contract(off)

#include "syn_internal.h"

namespace syn {

namespace {

constexpr int kLossThreads = 256;
constexpr int kLossLmk = 3 * kSynPts;                     // 204 landmark coordinates per face

struct WingSum { double s; long long n; };

__device__ __forceinline__ void wing_add(WingSum &a, float pred, float target, float omega, double inv_eps, double C) {
    const float d = fabsf(target - pred);
    if (d < omega) { a.s += (double)omega * log1p((double)d * inv_eps); a.n += 1; }
    else if (d >= omega) { a.s += (double)d - C; a.n += 1; }                    // NaN: neither branch
}

__device__ __forceinline__ double wing_C(float omega, float epsilon) {
    return (double)omega - (double)omega * log(1.0 + (double)omega / (double)epsilon);
}

// binary tree over the workgroup's 256 values, in place; every thread returns the total
__device__ __forceinline__ double tree_sum(double *lds, double v) {
    const int t = threadIdx.x;
    __syncthreads();                                      // the previous use of lds is over
    lds[t] = v;
    __syncthreads();
    for (int s = kLossThreads / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

// Takes a ticket after this workgroup's stores; true in the workgroup that drew the last one, with every other workgroup's stores visible.
// The counter is left at 0 for the next launch.
__device__ __forceinline__ bool last_workgroup(unsigned *counter) {
    __shared__ unsigned ticket;
    __threadfence();                                      // this thread's partial sums before the ticket
    __syncthreads();
    if (threadIdx.x == 0) ticket = atomicAdd(counter, 1u);
    __syncthreads();
    const bool last = ticket == gridDim.x - 1;
    if (last) {
        __threadfence();                                  // the other workgroups' partial sums after their tickets
        if (threadIdx.x == 0) *counter = 0u;
    }
    return last;
}

__device__ __forceinline__ double param_loss_face(const float *a, const float *b, int mode) {
    if (mode == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int k = 0; k < 12; ++k) { const float d = a[k] - b[k]; s0 += (double)d * (double)d; }
        for (int k = 12; k < kParam; ++k) { const float d = a[k] - b[k]; s1 += (double)d * (double)d; }
        return sqrt(s0 / 12.0 + s1 / 50.0);
    }
    double s = 0.0;
    for (int k = 0; k < 50; ++k) { const float d = a[k] - b[12 + k]; s += (double)d * (double)d; }
    return sqrt(s / 50.0);
}

}  // namespace

// -------------------------------------------------------------------------------------
// WingLoss of two flat arrays of N elements: one workgroup per kWingChunk elements; partial = [gridDim.x][2] doubles (sum, count)
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLossThreads) void wing_loss_kernel(const float *__restrict__ pred, const float *__restrict__ target, size_t N,
                                                                 float omega, float epsilon, double *partial, unsigned *counter,
                                                                 float *__restrict__ loss) {
    __shared__ double lds[kLossThreads];
    const int t = threadIdx.x;
    const double inv_eps = 1.0 / (double)epsilon, C = wing_C(omega, epsilon);
    const size_t e0 = (size_t)blockIdx.x * kWingChunk;
    const size_t e1 = e0 + kWingChunk < N ? e0 + kWingChunk : N;
    WingSum a = {0.0, 0};
    for (size_t e = e0 + t; e < e1; e += kLossThreads) wing_add(a, pred[e], target[e], omega, inv_eps, C);
    const double s = tree_sum(lds, a.s), n = tree_sum(lds, (double)a.n);      // counts are integers below 2^53: exact in fp64
    if (t == 0) { partial[2 * blockIdx.x] = s; partial[2 * blockIdx.x + 1] = n; }
    if (!last_workgroup(counter)) return;
    double ps = 0.0, pn = 0.0;
    for (unsigned c = t; c < gridDim.x; c += kLossThreads) { ps += partial[2 * c]; pn += partial[2 * c + 1]; }
    const double S = tree_sum(lds, ps), Nn = tree_sum(lds, pn);
    if (t == 0) loss[0] = (float)(S / Nn);                // no element in either branch: 0 / 0 = NaN, as the reference
}

void launch_wing_loss(const float *pred, const float *target, size_t N, float omega, float epsilon, double *partial, unsigned *counter,
                      float *loss, hipStream_t s) {
    wing_loss_kernel<<<wing_chunks(N), kLossThreads, 0, s>>>(pred, target, N, omega, epsilon, partial, counter, loss);
}

// -------------------------------------------------------------------------------------
// ParamLoss: one thread per face
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLossThreads) void param_loss_kernel(const float *__restrict__ input, const float *__restrict__ target, int B, int mode,
                                                                  float *__restrict__ loss) {
    const int b = blockIdx.x * kLossThreads + threadIdx.x;
    if (b >= B) return;
    loss[b] = (float)param_loss_face(input + (size_t)b * kParam, target + (size_t)b * kParam, mode);
}

void launch_param_loss(const float *input, const float *target, int B, int mode, float *loss, hipStream_t s) {
    param_loss_kernel<<<(B + kLossThreads - 1) / kLossThreads, kLossThreads, 0, s>>>(input, target, B, mode, loss);
}

// -------------------------------------------------------------------------------------
// The five weighted losses of model_building.py:146-155 in one launch.  Workgroup g takes faces [kLossFaces g, kLossFaces (g + 1)):
// their 204 landmark coordinates of both WingLosses and their three ParamLosses (thread 3 f + i: loss i of face f).
//   partial [gridDim.x][8] doubles: wing sum / count of LMK_f0, of LMK_pointNet, the chunk's sums of the three ROUNDED weighted
//   per-face losses (face order), one pad.
// The last workgroup folds them, writes the two scalars and adds the batch to the meter (nullable):
//   meter[i] += mean_i B (i = 0..4, dict order), meter[5] += (sum of the five means) B, meter[6] += B, meter[7] += 1
// -- AverageMeter.update(mean, B) of main_train.py:128-134 on the fp32 values the caller sees.  One launch at a time per meter.
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLossThreads) void synergy_losses_kernel(const float *__restrict__ param, const float *__restrict__ target,
                                                                      const float *__restrict__ lmk /*[B,3,68] of param*/,
                                                                      const float *__restrict__ lmk_gt /*of target*/,
                                                                      const float *__restrict__ lmk_refined, const float *__restrict__ param_rev,
                                                                      int B, double *partial, unsigned *counter, float *__restrict__ scalars /*[2]*/,
                                                                      float *__restrict__ per_face /*[3][B]*/, double *meter /*nullable [8]*/) {
    __shared__ double lds[kLossThreads];
    __shared__ float face_loss[3 * kLossFaces];
    const int t = threadIdx.x;
    const float omega = 10.f, epsilon = 2.f;
    const double inv_eps = 1.0 / (double)epsilon, C = wing_C(omega, epsilon);
    const int b0 = blockIdx.x * kLossFaces;
    const int nf = B - b0 < kLossFaces ? B - b0 : kLossFaces;
    const size_t e0 = (size_t)b0 * kLossLmk;
    const int ne = nf * kLossLmk;
    WingSum a0 = {0.0, 0}, a1 = {0.0, 0};
    for (int e = t; e < ne; e += kLossThreads) {
        const float gt = lmk_gt[e0 + e];
        wing_add(a0, lmk[e0 + e], gt, omega, inv_eps, C);
        wing_add(a1, lmk_refined[e0 + e], gt, omega, inv_eps, C);
    }
    if (t < 3 * kLossFaces) {
        const int f = t / 3, i = t - 3 * f;
        float v = 0.f;
        if (f < nf) {
            const size_t at = (size_t)(b0 + f) * kParam;
            const double l = i == 0 ? 0.02 * param_loss_face(param + at, target + at, 0)
                           : i == 1 ? 0.02 * param_loss_face(param_rev + at, target + at, 1)
                                    : 0.001 * param_loss_face(param_rev + at, param + at, 1);
            v = (float)l;
            per_face[(size_t)i * B + b0 + f] = v;
        }
        face_loss[3 * f + i] = v;
    }
    double w[4];
    w[0] = tree_sum(lds, a0.s); w[1] = tree_sum(lds, (double)a0.n);
    w[2] = tree_sum(lds, a1.s); w[3] = tree_sum(lds, (double)a1.n);           // (tree_sum's barriers also publish face_loss)
    if (t < 4) partial[8 * blockIdx.x + t] = w[t];
    if (t >= 4 && t < 7) {
        double s = 0.0;
        for (int f = 0; f < nf; ++f) s += (double)face_loss[3 * f + (t - 4)];
        partial[8 * blockIdx.x + t] = s;
    }
    if (!last_workgroup(counter)) return;
    double tot[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        double p = 0.0;
        for (unsigned c = t; c < gridDim.x; c += kLossThreads) p += partial[8 * c + q];
        tot[q] = tree_sum(lds, p);
    }
    if (t != 0) return;
    const float f0 = (float)(0.05 * (tot[0] / tot[1])), f1 = (float)(0.05 * (tot[2] / tot[3]));
    scalars[0] = f0;
    scalars[1] = f1;
    if (meter) {
        const double n = (double)B;
        const double mean[5] = {(double)f0, (double)f1, tot[4] / n, tot[5] / n, tot[6] / n};
        double total = 0.0;
        for (int i = 0; i < 5; ++i) { meter[i] += mean[i] * n; total += mean[i]; }
        meter[5] += total * n;
        meter[6] += n;
        meter[7] += 1.0;
    }
}

void launch_synergy_losses(const float *param, const float *target, const float *lmk, const float *lmk_gt, const float *lmk_refined,
                           const float *param_rev, int B, double *partial, unsigned *counter, float *scalars, float *per_face, double *meter,
                           hipStream_t s) {
    synergy_losses_kernel<<<loss_groups(B), kLossThreads, 0, s>>>(param, target, lmk, lmk_gt, lmk_refined, param_rev, B, partial, counter,
                                                                  scalars, per_face, meter);
}

// -------------------------------------------------------------------------------------
// CenterCrop(margin, mode='test') on uint8 [B,H,W,C]: bytes of pixels outside [margin, H - margin) x [margin, W - margin) become 0, the
// rest is copied.  Every thread reads and writes the same four byte positions, so in == out is safe.
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void center_crop_u8_kernel(const uint8_t *in, uint8_t *out, size_t total, int H, int W, int C, int margin,
                                                             int words) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; 4 * q < total; q += stride) {
        const size_t i0 = 4 * q;
        const int nb = total - i0 < 4 ? (int)(total - i0) : 4;
        uint8_t v[4] = {0, 0, 0, 0};
        if (words && nb == 4) {
            const uint32_t u = *(const uint32_t *)(in + i0);
            v[0] = u & 255; v[1] = (u >> 8) & 255; v[2] = (u >> 16) & 255; v[3] = u >> 24;
        } else {
            for (int k = 0; k < nb; ++k) v[k] = in[i0 + k];
        }
        for (int k = 0; k < nb; ++k) {
            const size_t pix = (i0 + k) / (size_t)C;
            const int x = (int)(pix % (size_t)W), y = (int)((pix / (size_t)W) % (size_t)H);
            if (!(y >= margin && y < H - margin && x >= margin && x < W - margin)) v[k] = 0;
        }
        if (words && nb == 4) *(uint32_t *)(out + i0) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
        else
            for (int k = 0; k < nb; ++k) out[i0 + k] = v[k];
    }
}

void launch_center_crop_u8(const uint8_t *in, uint8_t *out, int B, int H, int W, int C, int margin, hipStream_t s) {
    const size_t total = (size_t)B * H * W * C;
    const int words = ((uintptr_t)in % 4 == 0) && ((uintptr_t)out % 4 == 0);
    const size_t groups = (total + 3) / 4;
    const size_t blocks = (groups + 255) / 256;
    center_crop_u8_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>(in, out, total, H, W, C, margin, words);
}

}  // namespace syn
