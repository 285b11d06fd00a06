// The loss head's forward under BatchNorm BATCH statistics for gfx950: MLP_for / MLP_rev as the reference runs them in
// train().  A batch-wide reduction stands behind every convolution, so the head runs layer by layer with rows = the points of all
// faces (M = 68 B; the three heads of MLP_rev and conv6's per-face half with rows = faces).
//
//   train_layer_kernel  z = W a + bias (+ the face's row of conv6's per-face half) on v_mfma_f32_16x16x4_f32: MFMA rows = 16 output
//                       channels, MFMA columns = 16 rows of the batch, K 16 at a time in ascending order (one float4 per operand row
//                       feeds the four steps, the forward's walk).  a = relu((z_prev - mean) (gamma rstd) + beta), the CENTRED form,
//                       applied while the operand is loaded.  A row is one MFMA column that no other column enters and every row goes
//                       through the same instructions: its z does not depend on the tile or the position it sits in.  One wave owns
//                       16 channels of one BLOCK of `rows` rows (kTrainRows; test knob train_rows), walks the block's tiles in
//                       ascending order, four at a time past one weight fragment, and leaves the block's sum of z and of z z per
//                       channel in fp64: lane (channel, r) adds rows r, r + 16, ... of the block in ascending order, the 16 lanes of a
//                       channel fold through a fixed butterfly.  Rows >= M enter nothing.  Where rows are faces (the heads) a block
//                       holds rows / 16 faces, at least 16; conv6's per-face half has no statistics and runs 32 faces per wave.
//   train_stats_kernel  one thread per channel folds the blocks' partials in ascending block order in fp64: mean, var = max(sum z z / n -
//                       mean mean, 0), each rounded once to fp32 (batch_stats); rstd and gamma rstd; the running update
//                       (1 - m) running + m stat with the variance in its unbiased form n / (n - 1), written into the flat state.
//   train_max_kernel    max over a face's 68 points of relu(BatchNorm(z5)) from the MATERIALISED z5 [M][1024]: a channel with gamma < 0
//                       thereby takes its smallest z, one with gamma = 0 gives relu(beta).
//   train_finish_kernel refined landmarks = Lc + 0.05 relu(BatchNorm(z9)) | S2 = relu(BatchNorm(heads)).
// No floating-point atomics: the bits are a function of the inputs, B and the block size alone.
#pragma clang fp contract(off)

#include "syn_internal.h"

namespace syn {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int pad16(int x) { return (x + 15) / 16 * 16; }
constexpr int kRowTiles = 4;                               // row tiles of a wave's step: one weight fragment feeds four products
constexpr int kStatLd = 1024;                              // floats per statistics vector (the widest layer)

enum { kInBn = 0, kInLandmarks = 1, kInRaw = 2 };

struct TrainLayer {
    const float *X; int ldx, mode;                         // kInBn: z_prev [M][ldx] | kInLandmarks: [B][3][68] | kInRaw: rows [M][ldx]
    const float *in_mean, *in_g, *in_beta;                 // kInBn: the input layer's statistics, [K] each
    const float *W; int ldw, K;                            // [pad16(N)][ldw] zero padded; K % 4 == 0 columns are walked
    int N;                                                 // valid channels
    const float *bias[3]; int bias_end[3];                 // segment q: channels [bias_end[q - 1], bias_end[q]); null: no bias
    const float *add; int ld_add;                          // nullable: [M / 68][ld_add], the row of the face added BEFORE the statistics
    float *Z; int ldz;                                     // [M][ldz], ldz = N rounded up to 4; the columns past N receive 0
    double *part; int ldp;                                 // nullable: [blocks][2][ldp] sums of z | z z per block of rows
    int M, rows;
};

__global__ __launch_bounds__(64) void train_layer_kernel(TrainLayer p) {
    const int lane = threadIdx.x, r16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int m_begin = blockIdx.y * p.rows, m_end = m_begin + p.rows < p.M ? m_begin + p.rows : p.M;
    const float *wrow = p.W + (size_t)(n0 + r16) * p.ldw;
    const int c4 = n0 + 4 * g;                             // this lane's four output channels
    float bv[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int c = c4 + v;
        float b = 0.f;
        int lo = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (p.bias[q] && c >= lo && c < p.bias_end[q]) b = p.bias[q][c - lo];
            lo = p.bias_end[q];
        }
        bv[v] = b;
    }
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m0 = m_begin; m0 < m_end; m0 += 16 * kRowTiles) {
        const float *xp[kRowTiles];
        int mrow[kRowTiles];
        bool ok[kRowTiles];
#pragma unroll
        for (int j = 0; j < kRowTiles; ++j) {
            const int m = m0 + 16 * j + r16;
            ok[j] = m < m_end;
            mrow[j] = ok[j] ? m : m_end - 1;               // clamped: the loads are unconditional, the column is dropped
            xp[j] = p.mode == kInLandmarks ? p.X + (size_t)(mrow[j] / kSynPts) * (3 * kSynPts) + mrow[j] % kSynPts
                                           : p.X + (size_t)mrow[j] * p.ldx;
        }
        f32x4 acc[kRowTiles];
#pragma unroll
        for (int j = 0; j < kRowTiles; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < p.K; k0 += 16) {
            const int k = k0 + 4 * g;
            const bool kin = k < p.K;
            const int kc = kin ? k : 0;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            f32x4 w = *reinterpret_cast<const f32x4 *>(wrow + kc);
            w = kin ? w : zero;
            f32x4 mu = zero, sc = zero, be = zero;
            if (p.mode == kInBn) {
                mu = *reinterpret_cast<const f32x4 *>(p.in_mean + kc);
                sc = *reinterpret_cast<const f32x4 *>(p.in_g + kc);
                be = *reinterpret_cast<const f32x4 *>(p.in_beta + kc);
            }
#pragma unroll
            for (int j = 0; j < kRowTiles; ++j) {
                if (m0 + 16 * j >= m_end) continue;        // wave-uniform: the tile does not exist
                f32x4 a;
                if (p.mode == kInLandmarks) a = (f32x4){xp[j][0], xp[j][kSynPts], xp[j][2 * kSynPts], 0.f};      // K = 4: x, y, z, 0
                else a = *reinterpret_cast<const f32x4 *>(xp[j] + kc);
                if (p.mode == kInBn) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[e] = fmaxf(__builtin_fmaf(a[e] - mu[e], sc[e], be[e]), 0.f);
                }
                a = kin ? a : zero;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[e], a[e], acc[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < kRowTiles; ++j) {
            if (m0 + 16 * j >= m_end) continue;
            f32x4 z;
#pragma unroll
            for (int v = 0; v < 4; ++v) z[v] = acc[j][v] + bv[v];
            if (p.add) {
                const f32x4 ad = *reinterpret_cast<const f32x4 *>(p.add + (size_t)(mrow[j] / kSynPts) * p.ld_add + c4);
#pragma unroll
                for (int v = 0; v < 4; ++v) z[v] = z[v] + ad[v];
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) z[v] = c4 + v < p.N ? z[v] : 0.f;
            if (ok[j]) {
                if (c4 < p.ldz) *reinterpret_cast<f32x4 *>(p.Z + (size_t)mrow[j] * p.ldz + c4) = z;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    s1[v] += (double)z[v];
                    s2[v] += (double)z[v] * (double)z[v];
                }
            }
        }
    }
    if (!p.part) return;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            s1[v] += __shfl_xor(s1[v], d);
            s2[v] += __shfl_xor(s2[v], d);
        }
    }
    if (r16 == 0) {
        double *o = p.part + (size_t)blockIdx.y * 2 * p.ldp + c4;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            o[v] = s1[v];
            o[p.ldp + v] = s2[v];
        }
    }
}

struct TrainSeg { int c0, N; size_t bn; int bs; };         // channels [c0, c0 + N): the BatchNorm at flat offset bn, at bs in batch_stats
struct TrainStats {
    const double *part; int ldp, blocks;
    double n;                                              // values per channel
    TrainSeg seg[3]; int nseg;
    float *flat;                                           // gamma, beta read; running_mean / running_var written when momentum >= 0
    float *mean, *g, *beta;                                // [ldp] for the consumer: fp32 mean, gamma rstd, beta (0 past the layer)
    float *batch_stats;                                    // nullable [2][kSynBnChannels]
    float momentum;
};

__global__ __launch_bounds__(256) void train_stats_kernel(TrainStats p) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.ldp) return;
    int q = -1;
    for (int i = 0; i < p.nseg; ++i)
        if (c >= p.seg[i].c0 && c < p.seg[i].c0 + p.seg[i].N) q = i;
    if (q < 0) {
        p.mean[c] = 0.f; p.g[c] = 0.f; p.beta[c] = 0.f;
        return;
    }
    const TrainSeg sg = p.seg[q];
    const int cc = c - sg.c0;
    double S1 = 0.0, S2 = 0.0;
    for (int b0 = 0; b0 < p.blocks; b0 += 8) {             // ascending block order; eight blocks' loads in flight, then their adds in order
        double t1[8], t2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int b = b0 + j < p.blocks ? b0 + j : p.blocks - 1;
            t1[j] = p.part[(size_t)b * 2 * p.ldp + c];
            t2[j] = p.part[((size_t)b * 2 + 1) * p.ldp + c];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (b0 + j < p.blocks) {
                S1 += t1[j];
                S2 += t2[j];
            }
        }
    }
    const double mean = S1 / p.n;
    double var = S2 / p.n - mean * mean;
    var = var < 0.0 ? 0.0 : var;
    float *bn = p.flat + sg.bn;
    const double rstd = 1.0 / sqrt(var + 1e-5);
    p.mean[c] = (float)mean;
    p.g[c] = (float)((double)bn[cc] * rstd);
    p.beta[c] = bn[sg.N + cc];
    if (p.batch_stats) {
        p.batch_stats[sg.bs + cc] = (float)mean;
        p.batch_stats[kSynBnChannels + sg.bs + cc] = (float)var;
    }
    if (p.momentum >= 0.f) {
        const double m = (double)p.momentum;
        float *rm = bn + 2 * (size_t)sg.N + cc, *rv = bn + 3 * (size_t)sg.N + cc;
        *rm = (float)((1.0 - m) * (double)*rm + m * mean);
        *rv = (float)((1.0 - m) * (double)*rv + m * (var * (p.n / (p.n - 1.0))));
    }
}

// out[b pitch + c] = max over the face's 68 points of relu((z5 - mean) g + beta)
__global__ __launch_bounds__(256) void train_max_kernel(const float *Z, const float *mean, const float *g, const float *beta, float *out, int pitch) {
    const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    const float mu = mean[c], sc = g[c], be = beta[c];
    const float *z = Z + (size_t)b * kSynPts * kSynGlobal + c;
    float best = 0.f;                                      // relu: no point below 0 counts
#pragma unroll 4
    for (int pt = 0; pt < kSynPts; ++pt) {
        const float y = __builtin_fmaf(z[(size_t)pt * kSynGlobal] - mu, sc, be);
        best = y > best ? y : best;
    }
    out[(size_t)b * pitch + c] = best;
}

// heads == 0: Lr [B][3][68] = Lc + 0.05 relu(BatchNorm(z9 [M][4]));  heads == 1: S2 [B][62] = relu(BatchNorm(zh [B][64]))
__global__ __launch_bounds__(256) void train_finish_kernel(const float *Z, const float *mean, const float *g, const float *beta, const float *Lc,
                                                           float *out, int B, int heads) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (heads) {
        if (i >= (size_t)B * kParam) return;
        const int c = (int)(i % kParam);
        const size_t b = i / kParam;
        out[i] = fmaxf(__builtin_fmaf(Z[b * 64 + c] - mean[c], g[c], beta[c]), 0.f);
        return;
    }
    if (i >= (size_t)B * 3 * kSynPts) return;
    const int pt = (int)(i % kSynPts), c = (int)(i / kSynPts % 3);
    const size_t b = i / (3 * kSynPts);
    const float res = fmaxf(__builtin_fmaf(Z[(b * kSynPts + pt) * 4 + c] - mean[c], g[c], beta[c]), 0.f);
    out[i] = __builtin_fmaf(0.05f, res, Lc[i]);
}

}  // namespace

size_t train_scratch_floats(int B) {
    const size_t M = (size_t)B * kSynPts;
    return (size_t)(kSynFaceKpad + 512 + kSynGlobal + 64) * B + M * (64 + 512 + 512 + kSynGlobal) + (size_t)kSynFlatLayers * 3 * kStatLd;
}
// the per-point layers' blocks; the heads' blocks (rows / 16 faces, at least 16) are never more
size_t train_part_doubles(int B, int rows) { return (((size_t)B * kSynPts + rows - 1) / rows + 1) * 2 * kStatLd; }

void launch_synergy_train_head(const SynTrainArgs &a, hipStream_t s) {
    const int B = a.B, M = B * kSynPts;
    // scratch: X6 | g6 | gf_rev | heads' z | z2 | two ping-pong images of at most 512 columns | z5 | statistics vectors
    float *X6 = a.scratch, *g6 = X6 + (size_t)kSynFaceKpad * B, *gfr = g6 + (size_t)512 * B, *zh = gfr + (size_t)kSynGlobal * B;
    float *z2 = zh + (size_t)64 * B, *zA = z2 + (size_t)64 * M, *zB = zA + (size_t)512 * M, *z5 = zB + (size_t)512 * M;
    float *stat = z5 + (size_t)kSynGlobal * M;
    int bs[kSynFlatLayers + 1];
    bs[0] = 0;
    for (int i = 0; i < kSynFlatLayers; ++i) bs[i + 1] = bs[i] + syn_flat_layer(i).N;
    auto st = [&](int layer, int which) { return stat + ((size_t)layer * 3 + which) * kStatLd; };
    // layers l0 .. l0 + nl - 1 side by side along the channels (nl = 3: the heads of MLP_rev; nl = 0: a product without bias and statistics)
    auto run = [&](int l0, int nl, const float *X, int ldx, int mode, int in_layer, const float *W, int ldw, int K, int N, const float *add,
                   float *Z, int rowsM) {
        TrainLayer L = {};
        L.X = X; L.ldx = ldx; L.mode = mode;
        if (mode == kInBn) { L.in_mean = st(in_layer, 0); L.in_g = st(in_layer, 1); L.in_beta = st(in_layer, 2); }
        L.W = W; L.ldw = ldw; L.K = K; L.N = N;
        L.add = add; L.ld_add = 512;
        L.Z = Z; L.ldz = (N + 3) / 4 * 4;
        L.part = nl ? a.part : nullptr; L.ldp = pad16(N);
        // blocks: `rows` points; where rows are faces, rows / 16 faces (at least one tile) -- 1024 faces in 4 blocks of 256 would leave most
        // of the device idle --; a product without statistics has no order to keep and takes two tiles per wave
        const int rows = !nl ? 32 : rowsM == M ? a.rows : (a.rows / 16 > 16 ? a.rows / 16 : 16);
        L.M = rowsM; L.rows = rows;
        TrainStats S = {};
        int c0 = 0;
        for (int q = 0; q < 3; ++q) {
            L.bias[q] = nullptr; L.bias_end[q] = c0;
            if (q >= nl) continue;
            const SynFlatLayer f = syn_flat_layer(l0 + q);
            L.bias[q] = a.flat + f.bias;
            S.seg[q] = {c0, f.N, f.bn, bs[l0 + q]};
            c0 += f.N;
            L.bias_end[q] = c0;
        }
        const int blocks = (rowsM + rows - 1) / rows;
        train_layer_kernel<<<dim3(pad16(N) / 16, blocks), 64, 0, s>>>(L);
        if (!nl) return;
        S.part = a.part; S.ldp = L.ldp; S.blocks = blocks; S.n = (double)rowsM; S.nseg = nl;
        S.flat = a.flat; S.mean = st(l0, 0); S.g = st(l0, 1); S.beta = st(l0, 2);
        S.batch_stats = a.batch_stats; S.momentum = a.momentum;
        train_stats_kernel<<<(L.ldp + 255) / 256, 256, 0, s>>>(S);
    };
    auto trunk = [&](int which, const float *lmk, float *zc2, float *gf, int pitch) {
        const int l = which * 9;
        float *zc1 = zA, *zc3 = zA, *zc4 = zB;             // MLP_rev keeps z2 in zB: dead once conv3 has read it
        run(l + 0, 1, lmk, 0, kInLandmarks, 0, a.Wt[which][0], 4, 4, 64, nullptr, zc1, M);
        run(l + 1, 1, zc1, 64, kInBn, l + 0, a.Wt[which][1], 64, 64, 64, nullptr, zc2, M);
        run(l + 2, 1, zc2, 64, kInBn, l + 1, a.Wt[which][2], 64, 64, 64, nullptr, zc3, M);
        run(l + 3, 1, zc3, 64, kInBn, l + 2, a.Wt[which][3], 64, 64, 128, nullptr, zc4, M);
        run(l + 4, 1, zc4, 128, kInBn, l + 3, a.Wt[which][4], 128, 128, kSynGlobal, nullptr, z5, M);
        train_max_kernel<<<dim3(B, kSynGlobal / 256), 256, 0, s>>>(z5, st(l + 4, 0), st(l + 4, 1), st(l + 4, 2), gf, pitch);
    };
    // MLP_for
    trunk(0, a.Lc, z2, X6, kSynFaceKpad);
    launch_syn_face_concat(a.pool, a.param, X6, B, s);
    run(0, 0, X6, kSynFaceKpad, kInRaw, 0, a.W6f, kSynFaceKpad, kSynFaceKpad, 512, nullptr, g6, B);            // conv6's per-face half: rows = faces
    run(5, 1, z2, 64, kInBn, 1, a.W6p, 64, 64, 512, g6, zA, M);                                                // the statistics are those of the sum
    run(6, 1, zA, 512, kInBn, 5, a.W7, 512, 512, 256, nullptr, zB, M);
    run(7, 1, zB, 256, kInBn, 6, a.W8, 256, 256, 128, nullptr, zA, M);
    run(8, 1, zA, 128, kInBn, 7, a.W9, 128, 128, 3, nullptr, zB, M);
    train_finish_kernel<<<(B * 3 * kSynPts + 255) / 256, 256, 0, s>>>(zB, st(8, 0), st(8, 1), st(8, 2), a.Lc, a.Lr, B, 0);
    // MLP_rev on the refined landmarks
    trunk(1, a.Lr, zB, gfr, kSynGlobal);
    run(14, 3, gfr, kSynGlobal, kInRaw, 0, a.Wrev, kSynGlobal, kSynGlobal, kParam, nullptr, zh, B);
    train_finish_kernel<<<(B * kParam + 255) / 256, 256, 0, s>>>(zh, st(14, 0), st(14, 1), st(14, 2), nullptr, a.S2, B, 1);
}

}  // namespace syn
