// Weight gradients of the loss head for gfx950: the reductions ACROSS faces behind head_backward_kernel<0..3>
// (loss_backward_kernels.hip), and the fold of a flat state on the device (syn_update_synergy_device).
//
// A layer is y = relu(scale (W x) + shift), scale = gamma rstd, shift = (bias - mean) scale + beta.  With g the gradient at y behind the
// ReLU mask and BEFORE the multiplication by scale (the phases leave it in the images of kHeadWg floats), all the kernels here produce is
//     Gx[c][k] = sum g[c] x[k]        s[c] = sum g[c]            (over the faces and, for per-point layers, the 68 points)
// and wgrad_final_kernel turns them into dW = scale Gx, dbias = scale s, dbeta = s, dgamma = rstd (sum_k W Gx + (bias - mean) s).
//
//   wgrad_gemm_kernel   one wave per 16 channels x 64 columns of Gx (four tiles fed by one g fragment) on the exact-fp32 matrix instruction: MFMA rows = channels, MFMA
//                       columns = input columns, the K of the instruction = four rows of the reduction (points or faces).  68 = 17 x 4, so
//                       a face's points are 17 whole steps and no padded row exists; where rows are faces, the rows past the last one
//                       are loaded clamped and replaced by 0 in BOTH operands.  The column behind the last one is the constant 1: s.
//                       conv1 (K = 3) and conv9 (N = 3) run through it with the other rows / columns of the tile zeroed.
//   wgrad_conv5_kernel  conv5 of a trunk: g is non-zero at row arg[c] of each face only, so Gx's row is a gather over faces, an ordered
//                       chain of fused multiply-adds per (channel, column).
// Order: the per-point products cut a pass into chunks of `chunk` faces (test knob wgrad_chunk): a wave walks its chunk's faces in
// ascending order and a face's rows in ascending order into one tile of partial sums, and wgrad_fold_kernel adds the chunks' tiles to
// the accumulator in ascending chunk order, one thread per element; the per-face products and conv5's gather walk the pass's faces in
// ascending order from what the last pass stored.  No atomics: the order is a function of B, the pass size and the chunk alone.
#pragma clang fp contract(off)

#include "syn_internal.h"

namespace syn {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
using namespace headimg;

constexpr int pad16(int x) { return (x + 15) / 16 * 16; }

struct LayerDim { int cin, cout; };
constexpr LayerDim kFor[9] = {{3, 64}, {64, 64}, {64, 64}, {64, 128}, {128, 1024}, {64 + kSynFaceK, 512}, {512, 256}, {256, 128}, {128, 3}};
constexpr LayerDim kRev[8] = {{3, 64}, {64, 64}, {64, 64}, {64, 128}, {128, 1024}, {1024, 12}, {1024, 40}, {1024, 10}};
constexpr size_t mlp_count(const LayerDim *L, int n, int per_channel) {
    size_t c = 0;
    for (int i = 0; i < n; ++i) c += (size_t)L[i].cin * L[i].cout + (size_t)per_channel * L[i].cout;
    return c;
}

// leading dimensions of the accumulators: pad16(K + 1), the s column included
constexpr int kLd3 = 16, kLd64 = 80, kLd128 = 144, kLd256 = 272, kLd512 = 528, kLd1024 = 1040;
constexpr int kTrunkLd[5] = {kLd3, kLd64, kLd64, kLd64, kLd128};
constexpr int kTrunkN[5] = {64, 64, 64, 128, 1024};

struct WgProd {
    const float *G; size_t g_face; int g_row;            // g[f][r][c] = G[f g_face + r g_row + c]
    const float *X; size_t x_face; int x_row, x_col;     // x[f][r][k] = X[f x_face + r x_row + k x_col]
    int N, K;                                            // valid channels and columns
    int F, R;                                            // faces, reduced rows per face
    float *out; int ldo;                                 // [pad16(N)][ldo]
    int first, ones;                                     // start from 0 | continue from out;  column K = s
    float *part; int chunk;                              // not null: faces [z chunk, (z + 1) chunk) from 0 into part + z rows ldo
};

constexpr int kWgCols = 4;                               // column tiles of a wave: one g fragment feeds four products

__global__ __launch_bounds__(64) void wgrad_gemm_kernel(WgProd p) {
    const int lane = threadIdx.x, r16 = lane & 15, g = lane >> 4;
    const int c = blockIdx.x * 16 + r16;
    const bool c_in = c < p.N;
    const int cc = c_in ? c : p.N - 1;
    const int ntiles = (p.K + p.ones + 15) / 16, t0 = blockIdx.y * kWgCols;
    const int live = ntiles - t0 < kWgCols ? ntiles - t0 : kWgCols;      // column tiles of this wave that exist (>= 1)
    int kc[kWgCols];
    bool k_in[kWgCols];
    float x_out[kWgCols];
#pragma unroll
    for (int j = 0; j < kWgCols; ++j) {
        const int k = (t0 + j) * 16 + r16;
        k_in[j] = k < p.K;
        kc[j] = k_in[j] ? k : p.K - 1;                   // clamped: the load is unconditional, the value is replaced
        x_out[j] = (p.ones && k == p.K) ? 1.f : 0.f;
    }
    float *base = p.part ? p.part + (size_t)blockIdx.z * gridDim.x * 16 * p.ldo : p.out;
    float *o = base + (size_t)(blockIdx.x * 16 + 4 * g) * p.ldo + t0 * 16 + r16;
    f32x4 acc[kWgCols];
#pragma unroll
    for (int j = 0; j < kWgCols; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (!p.part && !p.first) {
#pragma unroll
        for (int j = 0; j < kWgCols; ++j)
            if (j < live) {
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[j][v] = o[(size_t)v * p.ldo + 16 * j];
            }
    }
    const int f0 = p.part ? blockIdx.z * p.chunk : 0, f1 = p.part ? (f0 + p.chunk < p.F ? f0 + p.chunk : p.F) : p.F;
    for (int f = f0; f < f1; ++f) {
        const float *gp = p.G + (size_t)f * p.g_face + cc;
        const float *xp = p.X + (size_t)f * p.x_face;
        if (p.R == kSynPts) {                            // a face's points: 17 whole steps, every load issued before the first product
            constexpr int S = kSynPts / 4;
            float a[S], b[kWgCols][S];
#pragma unroll
            for (int i = 0; i < S; ++i) a[i] = gp[(size_t)(4 * i + g) * p.g_row];
#pragma unroll
            for (int j = 0; j < kWgCols; ++j)
                if (j < live) {
#pragma unroll
                    for (int i = 0; i < S; ++i) b[j][i] = xp[(size_t)kc[j] * p.x_col + (size_t)(4 * i + g) * p.x_row];
                }
#pragma unroll
            for (int j = 0; j < kWgCols; ++j)
                if (j < live) {
#pragma unroll
                    for (int i = 0; i < S; ++i)
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(c_in ? a[i] : 0.f, k_in[j] ? b[j][i] : x_out[j], acc[j], 0, 0, 0);
                }
            continue;
        }
#pragma unroll 2
        for (int r0 = 0; r0 < p.R; r0 += 4) {
            const int r = r0 + g;
            const bool valid = r < p.R;
            const int rc = valid ? r : p.R - 1;
            float a = gp[(size_t)rc * p.g_row];          // unconditional loads, then selects
            a = (valid && c_in) ? a : 0.f;
#pragma unroll
            for (int j = 0; j < kWgCols; ++j)
                if (j < live) {
                    const float b = xp[(size_t)kc[j] * p.x_col + (size_t)rc * p.x_row];
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, valid ? (k_in[j] ? b : x_out[j]) : 0.f, acc[j], 0, 0, 0);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < kWgCols; ++j)
        if (j < live) {
#pragma unroll
            for (int v = 0; v < 4; ++v) o[(size_t)v * p.ldo + 16 * j] = acc[j][v];
        }
}

void gemm(const WgProd &p, hipStream_t s) {
    const int ntiles = (p.K + p.ones + 15) / 16;
    wgrad_gemm_kernel<<<dim3(pad16(p.N) / 16, (ntiles + kWgCols - 1) / kWgCols, p.part ? (p.F + p.chunk - 1) / p.chunk : 1), 64, 0, s>>>(p);
}

constexpr int kFoldLayers = 12;                          // the per-point layers: conv1 .. conv4 of both trunks, conv6 .. conv9
struct WgFold { float *acc[kFoldLayers]; const float *part[kFoldLayers]; unsigned n[kFoldLayers]; int chunks, first; };

// acc[i] (+)= the chunks' partial sums in ascending chunk order: one thread per element
__global__ __launch_bounds__(256) void wgrad_fold_kernel(WgFold A) {
    const int l = blockIdx.y;
    const unsigned n = A.n[l];
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        float a = A.first ? 0.f : A.acc[l][i];
        for (int c = 0; c < A.chunks; ++c) a += A.part[l][(size_t)c * n + i];
        A.acc[l][i] = a;
    }
}

struct WgGather {
    const float *dgf; size_t d_face;                     // the gradient at the max-pooled feature, [F][1024 ..]
    const int *arg; const float *X; size_t img;          // arg [1024] and conv4's output [68][128] inside the face's image
    int F;
    float *out;                                          // [1024][kLd128]
    int first;
};

// one workgroup per channel, thread k owns column k; thread 0 also carries s
__global__ __launch_bounds__(128) void wgrad_conv5_kernel(WgGather p) {
    const int c = blockIdx.x, k = threadIdx.x;
    float *o = p.out + (size_t)c * kLd128;
    float acc = p.first ? 0.f : o[k], s = p.first ? 0.f : o[128];
    for (int f = 0; f < p.F; ++f) {
        const int a = p.arg[(size_t)f * p.img + c];
        const bool on = a != 255;                        // 255: the maximum is 0, nothing passes
        const float coef = p.dgf[(size_t)f * p.d_face + c];
        const float x = p.X[(size_t)f * p.img + (size_t)(on ? a : 0) * 128 + k];
        acc = on ? __builtin_fmaf(coef, x, acc) : acc;
        s = on ? s + coef : s;
    }
    o[k] = acc;
    if (k == 0) o[128] = s;
}

struct WgLayerOut {
    size_t w, bias, bn;                                  // flat offsets
    int N, K, KA;                                        // columns [0, KA) from gxA, [KA, K) from gxB
    const float *gxA, *gxB;
    int ldA, ldB;
};
struct WgFinalArgs { WgLayerOut L[kSynFlatLayers]; const float *flat; float *d_flat; };

// one wave per (layer, channel): lane-strided columns, the 64 partial sums of dgamma fold through a fixed butterfly in fp64
__global__ __launch_bounds__(64) void wgrad_final_kernel(WgFinalArgs A) {
    const WgLayerOut &L = A.L[blockIdx.y];
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= L.N) return;
    const float *fl = A.flat;
    const float gamma = fl[L.bn + c], mean = fl[L.bn + 2 * (size_t)L.N + c], var = fl[L.bn + 3 * (size_t)L.N + c], bias = fl[L.bias + c];
    const double rstd = 1.0 / sqrt((double)var + 1e-5);
    const float scale = (float)((double)gamma * rstd);   // the forward's scale (fold_mlp)
    const float s = L.gxA[(size_t)c * L.ldA + L.KA];
    double part = 0.0;
    for (int k = lane; k < L.K; k += 64) {
        const float gx = k < L.KA ? L.gxA[(size_t)c * L.ldA + k] : L.gxB[(size_t)c * L.ldB + (k - L.KA)];
        const size_t at = L.w + (size_t)c * L.K + k;
        A.d_flat[at] = scale * gx;
        part += (double)fl[at] * (double)gx;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d);
    if (lane == 0) {
        A.d_flat[L.bias + c] = scale * s;
        A.d_flat[L.bn + c] = (float)(rstd * (part + ((double)bias - (double)mean) * (double)s));
        A.d_flat[L.bn + (size_t)L.N + c] = s;
        A.d_flat[L.bn + 2 * (size_t)L.N + c] = 0.f;      // running statistics: frozen
        A.d_flat[L.bn + 3 * (size_t)L.N + c] = 0.f;
    }
}

struct FoldArgs { SynFlatLayer F[kSynFlatLayers]; SynFoldTable T; const float *flat; float *blob; };
constexpr int kFoldBlocks = 64, kFoldThreads = 256;

// workgroup (j, layer): the layer's weights into their padded rows (the padding stays as syn_load_synergy left it: zero), scale and
// shift folded in fp64 and rounded once, as fold_mlp on the host
__global__ __launch_bounds__(kFoldThreads) void syn_fold_kernel(FoldArgs A) {
    const SynFlatLayer &F = A.F[blockIdx.y];
    const SynFoldLayer &T = A.T.L[blockIdx.y];
    const size_t nw = (size_t)F.N * F.K;
    for (size_t i = (size_t)blockIdx.x * kFoldThreads + threadIdx.x; i < nw; i += (size_t)kFoldBlocks * kFoldThreads) {
        const int r = (int)(i / F.K), k = (int)(i % F.K);
        const float w = A.flat[F.w + i];
        if (k < T.KA) A.blob[T.dstA + (size_t)r * T.ldA + k] = w;
        else A.blob[T.dstB + (size_t)r * T.ldB + (k - T.KA)] = w;
    }
    for (int c = blockIdx.x * kFoldThreads + threadIdx.x; c < F.N; c += kFoldBlocks * kFoldThreads) {
        const float *bn = A.flat + F.bn;
        const double sc = (double)bn[c] / sqrt((double)bn[3 * (size_t)F.N + c] + 1e-5);
        A.blob[T.dstScale + c] = (float)sc;
        A.blob[T.dstShift + c] = (float)(((double)A.flat[F.bias + c] - (double)bn[2 * (size_t)F.N + c]) * sc + (double)bn[(size_t)F.N + c]);
    }
}

}  // namespace

SynFlatLayer syn_flat_layer(int i) {
    const bool rev = i >= 9;
    const LayerDim *L = rev ? kRev : kFor;
    const int n = rev ? 8 : 9, j = rev ? i - 9 : i;
    const size_t base = rev ? mlp_count(kFor, 9, 5) : 0;
    SynFlatLayer f;
    f.w = base + mlp_count(L, j, 1);
    f.bias = f.w + (size_t)L[j].cin * L[j].cout;
    size_t bn = base + mlp_count(L, n, 1);
    for (int q = 0; q < j; ++q) bn += 4 * (size_t)L[q].cout;
    f.bn = bn;
    f.N = L[j].cout;
    f.K = L[j].cin;
    return f;
}
size_t syn_flat_total() { return mlp_count(kFor, 9, 5) + mlp_count(kRev, 8, 5); }

size_t head_wgrad_acc_floats() {
    size_t n = 0;
    for (int i = 0; i < 5; ++i) n += 2 * (size_t)kTrunkN[i] * kTrunkLd[i];
    return n + (size_t)512 * kLd64 + (size_t)512 * kSynFaceKpad + (size_t)256 * kLd512 + (size_t)128 * kLd256 + (size_t)16 * kLd128 + (size_t)64 * kLd1024;
}

// floats of one chunk's partial tiles over the per-point layers
static size_t part_floats_per_chunk() {
    size_t n = 0;
    for (int i = 0; i < 4; ++i) n += 2 * (size_t)kTrunkN[i] * kTrunkLd[i];
    return n + (size_t)512 * kLd64 + (size_t)256 * kLd512 + (size_t)128 * kLd256 + (size_t)16 * kLd128;
}
size_t head_wgrad_part_floats(int pass, int chunk) { return (size_t)((pass + chunk - 1) / chunk) * part_floats_per_chunk(); }

void head_wgrad_acc_carve(float *base, HeadWgAcc &acc) {
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 5; ++i) { acc.t[t][i] = base; base += (size_t)kTrunkN[i] * kTrunkLd[i]; }
    acc.c6p = base; base += (size_t)512 * kLd64;
    acc.c6f = base; base += (size_t)512 * kSynFaceKpad;
    acc.c7 = base; base += (size_t)256 * kLd512;
    acc.c8 = base; base += (size_t)128 * kLd256;
    acc.c9 = base; base += (size_t)16 * kLd128;
    acc.rev = base;
}

void launch_head_wgrad_pass(const HeadBwdArgs &a, const HeadWgAcc &acc, const float *X6, int b0, int nb, bool first, hipStream_t s) {
    const int P = kSynPts;
    const float *ws = a.ws, *wg = a.wg;
    const size_t iw = kHeadWs, ig = kHeadWg;
    const int fi = first ? 1 : 0, chunks = (nb + acc.chunk - 1) / acc.chunk;
    WgFold fold;
    fold.chunks = chunks;
    fold.first = fi;
    int nf = 0;
    float *part = acc.part;
    // a per-point layer: g image [68][g_row] in wg, x[r][k] = X[r x_row + k x_col] with its own face stride; chunk partials, folded below
    auto per_point = [&](int g_off, int g_row, int N, const float *X, size_t x_face, int x_row, int x_col, int K, float *out, int ldo) {
        gemm(WgProd{wg + g_off, ig, g_row, X, x_face, x_row, x_col, N, K, nb, P, out, ldo, fi, 1, part, acc.chunk}, s);
        fold.acc[nf] = out;
        fold.part[nf] = part;
        fold.n[nf] = (unsigned)(pad16(N) * ldo);
        part += (size_t)chunks * fold.n[nf];
        ++nf;
    };
    const float *pf = a.pf + (size_t)b0 * P * 64;
    for (int t = 0; t < 2; ++t) {                             // MLP_for's trunk, MLP_rev's trunk
        const int g1 = t ? wR1 : wF1, g2 = t ? wR2 : wF2, g3 = t ? wR3 : wF3, g4 = t ? wR4 : wF4;
        // conv1 reads landmarks [3][68]: row stride 1, column stride 68
        per_point(g1, 64, 64, (t ? a.Lr : a.Lc) + (size_t)b0 * 3 * P, (size_t)3 * P, 1, P, 3, acc.t[t][0], kLd3);
        per_point(g2, 64, 64, ws + (t ? oB1 : oA1), iw, 64, 1, 64, acc.t[t][1], kLd64);
        if (t) per_point(g3, 64, 64, ws + oB2, iw, 64, 1, 64, acc.t[t][2], kLd64);
        else per_point(g3, 64, 64, pf, (size_t)P * 64, 64, 1, 64, acc.t[t][2], kLd64);      // conv2's output comes from the forward launches' scratch
        per_point(g4, 128, 128, ws + (t ? oB3 : oA3), iw, 64, 1, 64, acc.t[t][3], kLd64);
        wgrad_conv5_kernel<<<kSynGlobal, 128, 0, s>>>(WgGather{t ? a.DGFRg + (size_t)kSynGlobal * b0 : a.DX6g + (size_t)kSynFaceKpad * b0,
                                                               t ? (size_t)kSynGlobal : (size_t)kSynFaceKpad,
                                                               (const int *)(ws + (t ? oARGR : oARGF)), ws + (t ? oB4 : oA4), iw, nb, acc.t[t][4], fi});
    }
    // MLP_for's head: conv6's per-point half (K = 64, carries s), conv7 .. conv9 (N = 3 of the image's 4 columns)
    per_point(wG6, 512, 512, pf, (size_t)P * 64, 64, 1, 64, acc.c6p, kLd64);
    per_point(wG7, 256, 256, ws + oH6, iw, 512, 1, 512, acc.c7, kLd512);
    per_point(wG8, 128, 128, ws + oH7, iw, 256, 1, 256, acc.c8, kLd256);
    per_point(wG9, 4, 3, ws + oH8, iw, 128, 1, 128, acc.c9, kLd128);
    wgrad_fold_kernel<<<dim3(64, kFoldLayers), 256, 0, s>>>(fold);
    // rows = faces: conv6's per-face half and MLP_rev's three heads as one [62][1024] layer
    gemm(WgProd{a.DG6Ug + (size_t)512 * b0, 0, 512, X6 + (size_t)kSynFaceKpad * b0, 0, kSynFaceKpad, 1, 512, kSynFaceK, 1, nb, acc.c6f, kSynFaceKpad,
                fi, 0, nullptr, 0}, s);
    gemm(WgProd{a.GS2Ug + (size_t)64 * b0, 0, 64, a.GFRg + (size_t)kSynGlobal * b0, 0, kSynGlobal, 1, kParam, kSynGlobal, 1, nb, acc.rev, kLd1024,
                fi, 1, nullptr, 0}, s);
}

void launch_head_wgrad_final(const HeadWgAcc &acc, const float *flat, float *d_flat, hipStream_t s) {
    WgFinalArgs A;
    A.flat = flat;
    A.d_flat = d_flat;
    int row = 0;
    for (int i = 0; i < kSynFlatLayers; ++i) {
        const SynFlatLayer f = syn_flat_layer(i);
        WgLayerOut &L = A.L[i];
        L.w = f.w; L.bias = f.bias; L.bn = f.bn; L.N = f.N; L.K = f.K; L.KA = f.K;
        L.gxB = nullptr; L.ldB = 0;
        if (i < 5) { L.gxA = acc.t[0][i]; L.ldA = kTrunkLd[i]; }
        else if (i == 5) { L.gxA = acc.c6p; L.ldA = kLd64; L.KA = 64; L.gxB = acc.c6f; L.ldB = kSynFaceKpad; }
        else if (i == 6) { L.gxA = acc.c7; L.ldA = kLd512; }
        else if (i == 7) { L.gxA = acc.c8; L.ldA = kLd256; }
        else if (i == 8) { L.gxA = acc.c9; L.ldA = kLd128; }
        else if (i < 14) { L.gxA = acc.t[1][i - 9]; L.ldA = kTrunkLd[i - 9]; }
        else { L.gxA = acc.rev + (size_t)row * kLd1024; L.ldA = kLd1024; row += f.N; }
    }
    wgrad_final_kernel<<<dim3(kSynGlobal, kSynFlatLayers), 64, 0, s>>>(A);
}

void launch_syn_fold_device(const float *flat, float *blob, const SynFoldTable &t, hipStream_t s) {
    FoldArgs A;
    for (int i = 0; i < kSynFlatLayers; ++i) A.F[i] = syn_flat_layer(i);
    A.T = t;
    A.flat = flat;
    A.blob = blob;
    syn_fold_kernel<<<dim3(kFoldBlocks, kSynFlatLayers), kFoldThreads, 0, s>>>(A);
}

}  // namespace syn
