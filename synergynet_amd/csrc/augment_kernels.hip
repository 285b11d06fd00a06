// Train-time augmentation on the device: the reference's training transform (main_train.py:199-208,
// Compose_GT([ColorJitter(0.4, 0.4, 0.4), ToTensor(), CenterCrop(5), Normalize(127.5, 128)]), utils/ddfa.py + PIL's ImageEnhance /
// Image.blend / convert('L')) on a resident uint8 set, byte for byte, one launch per batch.
//
//   grey        L = (19595 c0 + 38470 c1 + 7471 c2 + 32768) >> 16            (channel 0 = the first byte in memory)
//   blend       t = fp32(d) + fp32(f * fp32(x - d)): the product rounded, then the sum -- NEVER one fused multiply-add (a single rounding
//               changes bytes at f = 0.6, 0.8, 1.2).  0 <= f <= 1: trunc(t); otherwise 0 for t <= 0, 255 for t >= 255, trunc(t) between.
//   brightness  d = 0          saturation  d = L of the pixel          contrast  d = floor((2 sum L + n) / (2 n)) over the image as it
//               stands when the step runs (PIL's int(mean + 0.5); an integer sum: the order of the reduction cannot matter)
//   crop, mask  pixels outside [margin, H - margin) x [margin, W - margin), and outside the box of the mask kind, become 0
//   normalise   fp32(fp32(byte - mean) / std), a correctly rounded division, written CHW
//
// One workgroup per output face.  The face is gathered by its record's src_index into LDS (16-byte loads when the face's first byte
// is 16-byte aligned, byte loads otherwise -- the branch is per workgroup, outside the loops), the steps run as passes over LDS in
// groups of four pixels (12 bytes = three aligned words per lane, stride 3 words: no bank conflict), and the last pass applies
// crop and mask, normalises and stores: one 16-byte store per colour plane and one 12-byte store of the bytes per lane, consecutive
// lanes consecutive addresses.  No atomics: the grey sum is a wave reduction plus one LDS word per wave.
// A record that names no face of the set, a step above 3 or a mask kind above 7 gives an all-zero face and reads nothing.
#pragma clang fp contract(off)

#include "../../include/synergy_hip.h"
#include "syn_internal.h"

namespace syn {

namespace {

constexpr int kAugThreads = 256;
constexpr int kAugWaves = kAugThreads / 64;

struct __attribute__((packed, aligned(4))) AugF4 { float v[4]; };        // 16-byte store that needs 4-byte alignment only
struct __attribute__((packed, aligned(4))) AugU3 { uint32_t v[3]; };     // 12-byte store

__device__ __forceinline__ uint32_t aug_grey(uint32_t c0, uint32_t c1, uint32_t c2) {
    return (19595u * c0 + 38470u * c1 + 7471u * c2 + 32768u) >> 16;
}

// PIL's ImagingBlend on one byte: degenerate d, image x, factor f (the two roundings are the point: see the head of the file)
__device__ __forceinline__ uint32_t aug_blend(uint32_t d, uint32_t x, float f, bool inside) {
    // plain operators under this file's `fp contract(off)`: the runtime header's __fmul_rn / __fadd_rn are compiled in front of the
    // pragma and DO contract into one v_fma_f32 here
    const float prod = f * (float)((int)x - (int)d);
    const float t = (float)(int)d + prod;
    if (inside) return (uint32_t)(int)t & 255u;
    return t <= 0.f ? 0u : t >= 255.f ? 255u : (uint32_t)(int)t;
}

// one colour step on one pixel; m = the contrast step's mean
__device__ __forceinline__ void aug_step(int op, float f, bool inside, uint32_t m, uint32_t &c0, uint32_t &c1, uint32_t &c2) {
    uint32_t d = 0;
    if (op == 2) d = m;
    else if (op == 3) d = aug_grey(c0, c1, c2);
    c0 = aug_blend(d, c0, f, inside); c1 = aug_blend(d, c1, f, inside); c2 = aug_blend(d, c2, f, inside);
}

__device__ __forceinline__ void aug_unpack(const uint32_t w[3], uint32_t c[4][3]) {
    c[0][0] = w[0] & 255; c[0][1] = (w[0] >> 8) & 255; c[0][2] = (w[0] >> 16) & 255;
    c[1][0] = w[0] >> 24; c[1][1] = w[1] & 255; c[1][2] = (w[1] >> 8) & 255;
    c[2][0] = (w[1] >> 16) & 255; c[2][1] = w[1] >> 24; c[2][2] = w[2] & 255;
    c[3][0] = (w[2] >> 8) & 255; c[3][1] = (w[2] >> 16) & 255; c[3][2] = w[2] >> 24;
}

__device__ __forceinline__ void aug_pack(const uint32_t c[4][3], uint32_t w[3]) {
    w[0] = c[0][0] | c[0][1] << 8 | c[0][2] << 16 | c[1][0] << 24;
    w[1] = c[1][1] | c[1][2] << 8 | c[2][0] << 16 | c[2][1] << 24;
    w[2] = c[2][2] | c[3][0] << 8 | c[3][1] << 16 | c[3][2] << 24;
}

struct AugBox { int r0, r1, c0, c1; };      // what crop and mask keep: rows [r0, r1) x columns [c0, c1)

__device__ __forceinline__ float aug_norm(uint32_t byte, float mean, float stdv) { return __fdiv_rn(__fsub_rn((float)(int)byte, mean), stdv); }

// The last pass over the face in LDS: crop and mask, then the stores.  F32 / U8: which outputs exist; U8W: the face's bytes start on a
// 4-byte boundary (12-byte stores), otherwise byte stores.
template <bool F32, bool U8, bool U8W>
__device__ __forceinline__ void aug_write(const uint8_t *lds, int npx, int W, AugBox box, float mean, float stdv, float *of /*this face's planes*/,
                                          uint8_t *ou /*this face's bytes*/) {
    const uint32_t *lw = (const uint32_t *)lds;
    const int groups = npx >> 2;
    for (int g = threadIdx.x; g < groups; g += kAugThreads) {
        uint32_t w[3] = {lw[3 * g], lw[3 * g + 1], lw[3 * g + 2]}, c[4][3];
        aug_unpack(w, c);
        int y = (4 * g) / W, x = (4 * g) - y * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            while (x >= W) { x -= W; ++y; }
            const bool keep = y >= box.r0 && y < box.r1 && x >= box.c0 && x < box.c1;
            if (!keep) c[k][0] = c[k][1] = c[k][2] = 0;
            ++x;
        }
        if (F32) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                AugF4 v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v.v[k] = aug_norm(c[k][ch], mean, stdv);
                *(AugF4 *)(of + (size_t)ch * npx + 4 * (size_t)g) = v;
            }
        }
        if (U8) {
            aug_pack(c, w);
            if (U8W) {
                AugU3 v = {{w[0], w[1], w[2]}};
                *(AugU3 *)(ou + 12 * (size_t)g) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) ou[12 * (size_t)g + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
    // the last npx % 4 pixels
    const int p = 4 * groups + (int)threadIdx.x;
    if ((int)threadIdx.x < (npx & 3)) {
        const int y = p / W, x = p - y * W;
        const bool keep = y >= box.r0 && y < box.r1 && x >= box.c0 && x < box.c1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t b = keep ? lds[3 * p + ch] : 0u;
            if (F32) of[(size_t)ch * npx + p] = aug_norm(b, mean, stdv);
            if (U8) ou[3 * (size_t)p + ch] = (uint8_t)b;
        }
    }
}

__global__ __launch_bounds__(kAugThreads) void train_transform_kernel(const uint8_t *__restrict__ src, int N, int H, int W,
                                                                      const syn_train_record *__restrict__ records, int margin, float mean,
                                                                      float stdv, float *__restrict__ out_f32, uint8_t *__restrict__ out_u8) {
    extern __shared__ __attribute__((aligned(16))) uint8_t aug_lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int npx = H * W, nbytes = 3 * npx, groups = npx >> 2;
    const int face_lds = (nbytes + 15) & ~15;
    uint32_t *red = (uint32_t *)(aug_lds + face_lds);       // kAugWaves words (the launch reserves 16)
    uint32_t *lw = (uint32_t *)aug_lds;
    const size_t b = blockIdx.x;

    const syn_train_record rec = records[b];
    const bool valid = rec.src_index >= 0 && rec.src_index < N && rec.op[0] <= 3 && rec.op[1] <= 3 && rec.op[2] <= 3 && rec.mask <= 7;

    AugBox box = {0, 0, 0, 0};
    if (valid) {
        int r0 = 0, r1 = H, c0 = 0, c1 = W;
        const int k = rec.mask;
        if (k == 1 || k == 2 || k == 4) r1 = H / 2;
        if (k == 3) r0 = H / 2;
        if (k == 1 || k == 3 || k == 4 || k == 5) c1 = W / 2;
        if (k == 2 || k == 6) c0 = W / 2;
        if (k == 7) { r0 = H / 4; r1 = H - (H + 3) / 4; c0 = W / 4; c1 = W - (W + 3) / 4; }
        box.r0 = r0 > margin ? r0 : margin; box.r1 = r1 < H - margin ? r1 : H - margin;
        box.c0 = c0 > margin ? c0 : margin; box.c1 = c1 < W - margin ? c1 : W - margin;
    }
    const bool empty = !(box.r0 < box.r1 && box.c0 < box.c1);     // nothing survives: the colour steps cannot matter

    if (!empty) {
        const uint8_t *face = src + (size_t)rec.src_index * (size_t)nbytes;
        if (((uintptr_t)face & 15) == 0) {
            const int chunks = nbytes >> 4;
            const uint4 *f4 = (const uint4 *)face;
            uint4 *l4 = (uint4 *)aug_lds;
            for (int i = t; i < chunks; i += kAugThreads) l4[i] = f4[i];
            if (t < (nbytes & 15)) aug_lds[16 * chunks + t] = face[16 * chunks + t];
        } else {
            for (int i = t; i < nbytes; i += kAugThreads) aug_lds[i] = face[i];
        }
        __syncthreads();

        for (int s = 0; s < 3; ++s) {
            const int op = rec.op[s];
            if (op == 0) continue;
            const float f = rec.factor[s];
            const bool inside = f >= 0.f && f <= 1.f;
            uint32_t m = 0;
            if (op == 2) {
                uint32_t acc = 0;
                for (int g = t; g < groups; g += kAugThreads) {
                    uint32_t w[3] = {lw[3 * g], lw[3 * g + 1], lw[3 * g + 2]}, c[4][3];
                    aug_unpack(w, c);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc += aug_grey(c[k][0], c[k][1], c[k][2]);
                }
                if (t < (npx & 3)) {
                    const int p = 4 * groups + t;
                    acc += aug_grey(aug_lds[3 * p], aug_lds[3 * p + 1], aug_lds[3 * p + 2]);
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
                if (lane == 0) red[wave] = acc;
                __syncthreads();
                uint32_t sum = 0;
#pragma unroll
                for (int k = 0; k < kAugWaves; ++k) sum += red[k];
                m = (2u * sum + (uint32_t)npx) / (2u * (uint32_t)npx);        // sum <= 255 npx < 2^24: no overflow
            }
            for (int g = t; g < groups; g += kAugThreads) {
                uint32_t w[3] = {lw[3 * g], lw[3 * g + 1], lw[3 * g + 2]}, c[4][3];
                aug_unpack(w, c);
#pragma unroll
                for (int k = 0; k < 4; ++k) aug_step(op, f, inside, m, c[k][0], c[k][1], c[k][2]);
                aug_pack(c, w);
                lw[3 * g] = w[0]; lw[3 * g + 1] = w[1]; lw[3 * g + 2] = w[2];
            }
            if (t < (npx & 3)) {
                const int p = 4 * groups + t;
                uint32_t c0 = aug_lds[3 * p], c1 = aug_lds[3 * p + 1], c2 = aug_lds[3 * p + 2];
                aug_step(op, f, inside, m, c0, c1, c2);
                aug_lds[3 * p] = (uint8_t)c0; aug_lds[3 * p + 1] = (uint8_t)c1; aug_lds[3 * p + 2] = (uint8_t)c2;
            }
            __syncthreads();        // the step's bytes before the next pass; red[] is read before any wave can write it again
        }
    }
    // an empty box zeroes every pixel in aug_write: what LDS holds (nothing was loaded) is read and discarded, never stored

    float *of = out_f32 ? out_f32 + b * 3 * (size_t)npx : nullptr;
    uint8_t *ou = out_u8 ? out_u8 + b * (size_t)nbytes : nullptr;
    const bool u8w = ((uintptr_t)ou & 3) == 0;
    if (of && ou) {
        if (u8w) aug_write<true, true, true>(aug_lds, npx, W, box, mean, stdv, of, ou);
        else aug_write<true, true, false>(aug_lds, npx, W, box, mean, stdv, of, ou);
    } else if (of) {
        aug_write<true, false, false>(aug_lds, npx, W, box, mean, stdv, of, ou);
    } else {
        if (u8w) aug_write<false, true, true>(aug_lds, npx, W, box, mean, stdv, of, ou);
        else aug_write<false, true, false>(aug_lds, npx, W, box, mean, stdv, of, ou);
    }
}

}  // namespace

static_assert(sizeof(syn_train_record) == 20, "syn_train_record: {int32, float[3], uint8[3], uint8}");
static_assert(SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES + 64 == 160 * 1024 && SYN_TRAIN_TRANSFORM_MAX_FACE_BYTES % 16 == 0,
              "the face (rounded up to 16 bytes) and 16 reduction words fill one workgroup's LDS");

hipError_t launch_train_transform(const uint8_t *src, int N, int H, int W, const syn_train_record *records, int B, int margin, float mean,
                                  float stdv, float *out_f32, uint8_t *out_u8, hipStream_t s) {
    const size_t lds = (((size_t)3 * H * W + 15) & ~(size_t)15) + 64;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&train_transform_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024);
        if (e != hipSuccess) return e;
    }
    train_transform_kernel<<<(unsigned)B, kAugThreads, lds, s>>>(src, N, H, W, records, margin, mean, stdv, out_f32, out_u8);
    return hipSuccess;
}

}  // namespace syn
